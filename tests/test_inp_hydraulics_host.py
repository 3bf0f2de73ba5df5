"""``wdn_io.parse_inp_hydraulics`` / ``HydraulicNetwork.from_inp`` on the host: the hand-written fixture tests/golden/wdn_pumped.inp
gives the arrays written out below by hand, in SI units; every flow unit converts; each refusal names its offender;
``solve_ref`` converges on what was read.  No GPU."""
import math
import os

import numpy as np
import pytest

import hydraulics_refs as HR

H, G = HR.H, HR.G
io = G.wdn_io
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wdn_pumped.inp")

NODES = ["J1", "J2", "J3", "J4", "J5", "J6", "J7", "J8", "J9", "J10", "R1", "T1"]
LINKS = ["P1", "P2", "P3", "P4", "P5", "P6", "P7", "P8", "P9", "P10", "PU1", "PU2", "V1"]
# a link runs from its first node to its second, as the file has them
ENDS = [(0, 1), (1, 2), (2, 3), (3, 4), (1, 5), (5, 6), (6, 2), (7, 8), (11, 9), (6, 3), (10, 0), (4, 7), (8, 9)]
ELEVATION = [10, 12, 15, 14, 16, 11, 13, 30, 32, 33, 20, 55]
DEMAND = [0, 2.0e-3, 1.5e-3, 1.0e-3, 0.5e-3, 1.2e-3, 0.8e-3, 1.0e-3, 0.6e-3, 0.4e-3, 0, 0]                      # m3/s (LPS / 1000)
LENGTH = [300, 250, 200, 150, 400, 350, 100, 500, 120, 220, 0, 0, 0]
DIAMETER = [0.3, 0.25, 0.2, 0.2, 0.15, 0.15, 0.1, 0.2, 0.25, 0.15, io.NOMINAL_PUMP_DIAMETER, io.NOMINAL_PUMP_DIAMETER, 0.2]
ROUGHNESS = [120, 110, 100, 100, 90, 95, 100, 130, 125, 105, 100, 100, 100]
MINOR_K = [0, 0.5, 0, 0, 0, 1.2, 0, 0, 0, 0, 0, 0, 8.0]
CHECK = [0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 1, 0]                   # P5 is a CV pipe; a pump is always CHECK
CLOSED = [0, 0, 0, 0, 0, 0, 1, 0, 0, 1, 0, 0, 0]                  # P7 by [PIPES], P10 by [STATUS]
MULTIPLIERS = [[1.0, 1.0, 1.0, 1.0], [0.8, 1.0, 1.2, 1.0], [1.1, 0.9, 1.1, 0.9]]      # constant, DAY (two lines), NIGHT (wrapped)
PATTERN_OF_NODE = [0, 1, 1, 0, 2, 1, 2, 1, 0, 2, 0, 0]


@pytest.fixture(scope="module")
def parsed():
    return io.parse_inp_hydraulics(FIXTURE)


def test_the_fixture_gives_the_arrays_written_out_by_hand(parsed):
    net = parsed.network
    assert parsed.node_names == NODES and parsed.link_names == LINKS and parsed.pattern_names[1:] == ["DAY", "NIGHT"]
    assert (net.num_nodes, net.num_pipes, net.num_pumps, net.num_tanks) == (12, 13, 2, 1)
    assert net.pipes.tolist() == [list(e) for e in ENDS]
    assert np.array_equal(net.elevation, np.array(ELEVATION, dtype=np.float64))
    assert np.allclose(parsed.demand, DEMAND, rtol=1e-15, atol=0) and np.array_equal(parsed.roughness, np.array(ROUGHNESS, dtype=np.float64))
    assert np.array_equal(net.length, np.array(LENGTH, dtype=np.float64)) and np.allclose(net.diameter, DIAMETER, rtol=1e-15, atol=0)
    assert np.array_equal(net.minor_loss, np.array(MINOR_K)) and np.array_equal(net.check_valve, np.array(CHECK, dtype=bool))
    assert np.array_equal(net.closed, np.array(CLOSED, dtype=bool)) and net.link_kind.tolist() == [0] * 10 + [1, 1, 0]
    # m = 8 K / (pi^2 g D^4), by hand for the three links that have one
    for p in (1, 5, 12):
        assert net.minor[p] == pytest.approx(8.0 * MINOR_K[p] / (math.pi ** 2 * 9.80665 * DIAMETER[p] ** 4), rel=1e-14)
    assert net.fixed_nodes.tolist() == [10, 11] and net.fixed_head[[10, 11]].tolist() == [20.0, 58.0]      # the tank: 55 + 3
    assert net.tank_nodes.tolist() == [11] and net.tank_diameter.tolist() == [10.0]
    assert net.tank_min_level.tolist() == [0.5] and net.tank_max_level.tolist() == [6.0]
    assert np.array_equal(parsed.multipliers, np.array(MULTIPLIERS)) and parsed.pattern_of_node.tolist() == PATTERN_OF_NODE
    # PU1: (0, 60), (40 L/s, 50), (80 L/s, 20): n = ln(40 / 10) / ln 2 = 2, rp = 10 / 0.04^2 = 6250
    assert net.pump_links.tolist() == [10, 11] and net.pump_h0.tolist() == [60.0, 1.33 * 30.0]
    assert net.pump_n[0] == pytest.approx(2.0, rel=1e-14) and net.pump_r[0] == pytest.approx(6250.0, rel=1e-12)
    # PU2: one point (20 L/s, 30): shut-off 39.9, zero head at 40 L/s: n = ln(39.9 / 9.9) / ln 2, rp = 9.9 / 0.02^n
    n2 = math.log(39.9 / 9.9) / math.log(2.0)
    assert net.pump_n[1] == pytest.approx(n2, rel=1e-14) and net.pump_r[1] == pytest.approx(9.9 / 0.02 ** n2, rel=1e-12)
    assert parsed.pump_speed.tolist() == [1.0, 1.1]
    same = H.HydraulicNetwork.from_inp(FIXTURE)
    assert np.array_equal(same.pipes, net.pipes) and np.array_equal(same.coef, net.coef) and np.array_equal(same.pump_r, net.pump_r)


def test_what_was_read_solves_and_its_links_stand_as_the_file_says(parsed):
    net = parsed.network
    for solver in ("dense", "banded"):
        ref = H.solve_ref(net, parsed.demand[None], parsed.roughness[None], solver=solver, pump_speed=parsed.pump_speed[None])
        assert ref.converged.all() and ref.link_state[0].tolist() == [2 if c else 0 for c in CLOSED]
        mass, energy = H.hydraulic_residuals(net, ref.head, ref.flow, parsed.demand[None], parsed.roughness[None],
                                             pump_speed=parsed.pump_speed[None])
        assert mass.max() <= 1e-6 and energy.max() <= 1e-3
        assert ref.flow[0, 10] == pytest.approx(parsed.demand.sum() - ref.flow[0, 8], rel=1e-9)       # the pump feeds demand and tank
    series = H.simulate_series_ref(net, parsed.demand[None], parsed.roughness[None], parsed.multipliers, 300.0,
                                   pattern_of_node=parsed.pattern_of_node, pump_speed=parsed.pump_speed[None])
    assert series.converged.all() and series.level.shape == (1, 5, 1) and series.level[0, 0, 0] == 3.0


@pytest.mark.parametrize("units", sorted(io.FLOW_UNITS))
def test_every_flow_unit_converts_to_si(units):
    text = (f"[JUNCTIONS]\n J1 100 6\n[RESERVOIRS]\n R1 200\n[PIPES]\n P1 R1 J1 1000 12 100 0 Open\n"
            f"[OPTIONS]\n UNITS {units}\n HEADLOSS H-W\n[END]\n")
    r = io.parse_inp_hydraulics(text=text)
    per_unit = {"LPS": 1e-3, "LPM": 1e-3 / 60, "MLD": 1000.0 / 86400, "CMH": 1.0 / 3600, "CMD": 1.0 / 86400,
                "GPM": 3.785411784e-3 / 60, "CFS": 0.3048 ** 3, "MGD": 3785.411784 / 86400}[units]
    us = units in ("GPM", "CFS", "MGD")
    assert r.demand[0] == pytest.approx(6 * per_unit, rel=1e-14)
    assert r.network.length[0] == pytest.approx(304.8 if us else 1000.0, rel=1e-14)
    assert r.network.diameter[0] == pytest.approx(0.3048 if us else 0.012, rel=1e-14)
    assert r.network.elevation[0] == pytest.approx(30.48 if us else 100.0, rel=1e-14)
    assert r.network.fixed_head[1] == pytest.approx(60.96 if us else 200.0, rel=1e-14)


BASE = ("[JUNCTIONS]\n J1 10 1\n J2 10 1\n[RESERVOIRS]\n R1 50\n[PIPES]\n P1 R1 J1 100 200 100 0 Open\n P2 J1 J2 100 200 100 0 Open\n"
        "{extra}[OPTIONS]\n UNITS LPS\n HEADLOSS {formula}\n[END]\n")


@pytest.mark.parametrize("extra, formula, kw, offender", (
    ("", "D-W", {}, "D-W"),
    ("", "C-M", {}, "C-M"),
    ("[PUMPS]\n PU9 R1 J2 POWER 15\n", "H-W", {}, "PU9"),
    ("[PUMPS]\n PU8 R1 J2 HEAD C7\n", "H-W", {}, "PU8"),
    ("[VALVES]\n V7 J1 J2 200 PRV 30 0\n", "H-W", {}, "V7"),
    ("[VALVES]\n V6 J1 J2 200 FCV 5 0\n", "H-W", {"unsupported_valves": "open"}, "V6"),          # open, but without a loss: no law
    ("[CONTROLS]\n LINK P2 CLOSED IF NODE J2 ABOVE 20\n", "H-W", {}, "CONTROLS"),
    ("[RULES]\n RULE 1\n IF TANK T1 LEVEL ABOVE 5\n THEN PUMP PU1 STATUS IS CLOSED\n", "H-W", {}, "RULES"),
    ("[STATUS]\n P77 Closed\n", "H-W", {}, "P77"),
    ("[PIPES]\n P3 J2 J9 10 100 100 0 Open\n", "H-W", {}, "P3"),
))
def test_each_refusal_names_its_offender(extra, formula, kw, offender):
    with pytest.raises(ValueError, match=offender):
        io.parse_inp_hydraulics(text=BASE.format(extra=extra, formula=formula), **kw)


def test_units_outside_the_list_are_refused_and_switches_open_what_they_say():
    with pytest.raises(ValueError, match="AFD"):
        io.parse_inp_hydraulics(text=BASE.format(extra="", formula="H-W").replace("UNITS LPS", "UNITS AFD"))
    valve = "[VALVES]\n V7 J1 J2 200 PRV 30 2.5\n"
    r = io.parse_inp_hydraulics(text=BASE.format(extra=valve, formula="H-W"), unsupported_valves="open")
    assert r.link_names == ["P1", "P2", "V7"] and r.network.minor_loss.tolist() == [0, 0, 2.5] and r.network.length[2] == 0
    assert not r.network.closed.any() and not r.network.check_valve.any()
    ctl = "[CONTROLS]\n LINK P2 CLOSED IF NODE J2 ABOVE 20\n"
    r = io.parse_inp_hydraulics(text=BASE.format(extra=ctl, formula="H-W"), ignore_controls=True)
    assert r.link_names == ["P1", "P2"] and not r.network.has_links
    with pytest.raises(ValueError, match="refuse"):
        io.parse_inp_hydraulics(text=BASE.format(extra="", formula="H-W"), unsupported_valves="close")
