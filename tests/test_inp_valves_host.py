"""``wdn_io.parse_inp_hydraulics(regulating="model")`` on the host: the hand-written fixture tests/golden/wdn_valved.inp gives the
kinds, the settings in metres and the orientation written out below; the pressure units convert; without the keyword the file is
refused exactly as it always was; ``solve_ref`` converges on what was read and the zones sit where the valves hold them.  No GPU."""
import os

import numpy as np
import pytest

import hydraulics_refs as HR

H, G = HR.H, HR.G
io = G.wdn_io
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wdn_valved.inp")
NODES = ["J1", "J2", "J3", "J4", "J5", "J6", "J7", "J8", "J9", "J10", "R1", "R2"]
LINKS = ["P1", "P2", "P3", "P4", "P5", "P6", "P7", "P8", "P9", "P10", "V1", "V2"]


@pytest.fixture(scope="module")
def parsed():
    return io.parse_inp_hydraulics(FIXTURE, regulating="model")


def test_the_fixture_parses_to_kinds_settings_in_metres_and_orientation(parsed):
    net = parsed.network
    assert parsed.node_names == NODES and parsed.link_names == LINKS
    assert (net.num_nodes, net.num_pipes, net.num_valves, net.num_pumps) == (12, 12, 2, 0)
    assert net.valve_links.tolist() == [10, 11] and net.valve_kind_names == ("PRV", "PSV")
    assert net.valve_kind.tolist() == [H.LINK_PRV, H.LINK_PSV] and net.link_kind.tolist() == [0] * 10 + [2, 3]
    assert net.valve_setting.tolist() == [30.0, 40.0]                       # LPS: metres
    assert net.pipes[10].tolist() == [1, 2] and net.pipes[11].tolist() == [6, 7]      # J2 -> J3, J7 -> J8, as the file has them
    assert net.valve_node.tolist() == [2, 6]                                # PRV: downstream J3; PSV: upstream J7
    assert net.minor_loss[10] == 2.5 and net.minor_loss[11] == 0.0 and net.coef[10] == 0 and net.coef[11] == 0
    assert np.isclose(net.diameter[10], 0.2) and np.isclose(net.diameter[11], 0.15)


def test_pressure_units_convert():
    text = open(FIXTURE).read()
    kpa = io.parse_inp_hydraulics(text=text.replace(" HEADLOSS   H-W", " HEADLOSS   H-W\n PRESSURE   KPA"), regulating="model").network
    assert np.allclose(kpa.valve_setting, np.array([30.0, 40.0]) * 0.3048 / 0.4333 / 6.895, rtol=1e-15)
    psi = io.parse_inp_hydraulics(text=text.replace("UNITS      LPS", "UNITS      GPM"), regulating="model").network
    assert np.allclose(psi.valve_setting, np.array([30.0, 40.0]) * 0.3048 / 0.4333, rtol=1e-15)      # 1 psi = 0.7034 m of water
    with pytest.raises(ValueError, match="PRESSURE"):
        io.parse_inp_hydraulics(text=text.replace(" HEADLOSS   H-W", " HEADLOSS   H-W\n PRESSURE   PSI"), regulating="model")
    with pytest.raises(ValueError, match="regulating"):
        io.parse_inp_hydraulics(FIXTURE, regulating="open")


def test_without_the_keyword_the_file_is_refused_as_ever():
    for kw in ({}, {"regulating": None}):
        with pytest.raises(ValueError) as err:
            io.parse_inp_hydraulics(FIXTURE, **kw)
        assert str(err.value) == '[VALVES] V1: a PRV valve is not modelled (unsupported_valves="open" makes it an open link)'
    with pytest.raises(ValueError, match="V2: an open valve without a loss coefficient"):      # V2 has K = 0: as ever
        io.parse_inp_hydraulics(FIXTURE, unsupported_valves="open")


def test_other_regulating_valves_still_go_by_unsupported_valves():
    text = open(FIXTURE).read().replace("PSV    40        0", "FCV    40        1.0")
    with pytest.raises(ValueError, match="V2: a FCV valve is not modelled"):
        io.parse_inp_hydraulics(text=text, regulating="model")
    net = io.parse_inp_hydraulics(text=text, regulating="model", unsupported_valves="open").network
    assert net.num_valves == 1 and net.valve_kind_names == ("PRV",) and net.minor_loss[11] == 1.0


def test_status_may_close_a_regulating_valve_but_not_fix_it_open():
    text = open(FIXTURE).read()
    shut = io.parse_inp_hydraulics(text=text.replace("[PATTERNS]", "[STATUS]\n V1   Closed\n\n[PATTERNS]"), regulating="model").network
    assert shut.closed.tolist() == [False] * 10 + [True, False] and shut.num_valves == 2
    with pytest.raises(ValueError) as err:
        io.parse_inp_hydraulics(text=text.replace("[PATTERNS]", "[STATUS]\n V2   Open\n\n[PATTERNS]"), regulating="model")
    assert str(err.value) == "[STATUS] V2: a fixed OPEN status of a regulating valve is not modelled"


def test_the_zones_sit_where_the_valves_hold_them(parsed):
    net = parsed.network
    T = parsed.multipliers.shape[1]
    ref = H.simulate_series_ref(net, parsed.demand[None, :], parsed.roughness[None, :], parsed.multipliers, 3600.0,
                                pattern_of_node=parsed.pattern_of_node)
    print(ref.iterations.tolist(), ref.link_state[0, :, 10:].tolist(), (ref.head[0] - net.elevation)[:, [2, 6]].tolist())
    assert ref.converged.all() and T == 2
    assert (ref.link_state[0, :, 10] == H.VALVE_ACTIVE).all()               # the PRV holds J3 at 30 m
    assert (ref.head[0, :, 2] == 10.0 + 30.0).all()
    state = ref.link_state[0, :, 11]
    active = state == H.VALVE_ACTIVE
    assert (ref.head[0, active, 6] == 22.0 + 40.0).all() and ((ref.head[0, :, 6] - 22.0) >= 40.0 - 1e-9).all()
    from_inp = H.HydraulicNetwork.from_inp(FIXTURE, regulating="model")
    assert from_inp.valve_links.tolist() == [10, 11]
