"""``wdn_io.parse_inp_hydraulics(demand_model="model")`` on the host: the hand-written fixture tests/golden/wdn_deficient.inp, in US
units, gives the demand model of [OPTIONS] and its pressures in metres, checked against values computed here; the pressure units
convert; the default call gives what it always gave (the file is read as demand-driven); a bad model word, a required pressure
too close to the minimum and values that are no numbers are refused by name; ``solve_ref`` converges on what was read, the
junction above the source head gets nothing and the one below the required pressure a part.  No GPU."""
import os

import numpy as np
import pytest

import hydraulics_refs as HR

H, G = HR.H, HR.G
io = G.wdn_io
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wdn_deficient.inp")
NODES = ["J1", "J2", "J3", "J4", "J5", "J6", "SRC"]
M_PER_PSI = 0.3048 / 0.4333                                 # EPANET's own constants, as the valve settings use them
PMIN_PSI, PREQ_PSI, EXPONENT = 5.0, 25.0, 0.5               # as the file has them


@pytest.fixture(scope="module")
def parsed():
    return io.parse_inp_hydraulics(FIXTURE, demand_model="model")


def pdd_kw(p):
    return dict(demand_model=p.demand_model, minimum_pressure=p.minimum_pressure, required_pressure=p.required_pressure,
                pressure_exponent=p.pressure_exponent)


def test_the_fixture_parses_to_the_model_and_its_pressures_in_metres(parsed):
    net = parsed.network
    assert parsed.node_names == NODES and (net.num_nodes, net.num_pipes) == (7, 7)
    print("minimum, required", parsed.minimum_pressure, parsed.required_pressure, "computed here", PMIN_PSI * M_PER_PSI, PREQ_PSI * M_PER_PSI)
    assert parsed.demand_model == "pda" and parsed.pressure_exponent == EXPONENT
    assert parsed.minimum_pressure == PMIN_PSI * M_PER_PSI and parsed.required_pressure == PREQ_PSI * M_PER_PSI
    assert np.isclose(parsed.minimum_pressure, 3.5172, atol=1e-4) and np.isclose(parsed.required_pressure, 17.586, atol=1e-3)
    assert np.isclose(net.elevation[5], 230 * 0.3048) and np.isclose(net.fixed_head[6], 200 * 0.3048)


def test_the_default_call_reads_the_file_as_it_always_did(parsed):
    old = io.parse_inp_hydraulics(FIXTURE)
    assert old.demand_model is None and old.minimum_pressure is None and old.required_pressure is None and old.pressure_exponent is None
    for k in ("pipes", "coef", "elevation", "fixed", "fixed_head", "q_start", "order", "position"):
        assert np.array_equal(getattr(old.network, k), getattr(parsed.network, k)), k
    assert np.array_equal(old.demand, parsed.demand) and np.array_equal(old.multipliers, parsed.multipliers)
    net = H.HydraulicNetwork.from_inp(FIXTURE, demand_model="model")
    assert np.array_equal(net.coef, parsed.network.coef)


def test_pressure_units_and_defaults_convert():
    text = open(FIXTURE).read()
    si = text.replace("UNITS               GPM", "UNITS               LPS")
    metres = io.parse_inp_hydraulics(text=si, demand_model="model")
    assert (metres.minimum_pressure, metres.required_pressure) == (5.0, 25.0)
    kpa = io.parse_inp_hydraulics(text=si.replace(" HEADLOSS            H-W", " HEADLOSS            H-W\n PRESSURE   KPA"), demand_model="model")
    assert np.allclose([kpa.minimum_pressure, kpa.required_pressure], np.array([5.0, 25.0]) * M_PER_PSI / 6.895, rtol=1e-15)
    dda = io.parse_inp_hydraulics(text=text.replace("DEMAND MODEL        PDA", "DEMAND MODEL        DDA"), demand_model="model")
    assert dda.demand_model == "dda" and dda.required_pressure == PREQ_PSI * M_PER_PSI
    ref = H.solve_ref(dda.network, dda.demand[None, :], dda.roughness[None, :], **pdd_kw(dda))      # the scalars are handed on, not read
    old = H.solve_ref(dda.network, dda.demand[None, :], dda.roughness[None, :])
    assert ref.head.tobytes() == old.head.tobytes() and np.array_equal(ref.demand_delivered[0, :6], dda.demand[:6])
    bare = "\n".join(ln for ln in si.splitlines() if not any(w in ln for w in ("DEMAND MODEL", "MUM PRESSURE", "RED PRESSURE", "RE EXPONENT")))
    none = io.parse_inp_hydraulics(text=bare, demand_model="model")             # EPANET's defaults: DDA, 0, 0.1, 0.5
    assert (none.demand_model, none.minimum_pressure, none.required_pressure, none.pressure_exponent) == ("dda", 0.0, 0.1, 0.5)


@pytest.mark.parametrize("old,new,match", (
    ("DEMAND MODEL        PDA", "DEMAND MODEL        FIXED", r"DEMAND MODEL FIXED"),
    ("REQUIRED PRESSURE   25", "REQUIRED PRESSURE   5.1", r"REQUIRED PRESSURE 5.1.*at least 0.1 m"),
    ("REQUIRED PRESSURE   25", "REQUIRED PRESSURE   4", r"REQUIRED PRESSURE 4"),
    ("MINIMUM PRESSURE    5", "MINIMUM PRESSURE    nan", r"MINIMUM PRESSURE nan"),
    ("REQUIRED PRESSURE   25", "REQUIRED PRESSURE   inf", r"REQUIRED PRESSURE inf"),
    ("REQUIRED PRESSURE   25", "REQUIRED PRESSURE   high", r"REQUIRED PRESSURE high"),
    ("PRESSURE EXPONENT   0.5", "PRESSURE EXPONENT   0", r"PRESSURE EXPONENT 0"),
    ("PRESSURE EXPONENT   0.5", "PRESSURE EXPONENT   -1", r"PRESSURE EXPONENT -1"),
))
def test_refusals_name_the_offender(old, new, match):
    text = open(FIXTURE).read()
    assert old in text
    with pytest.raises(ValueError, match=match):
        io.parse_inp_hydraulics(text=text.replace(old, new), demand_model="model")
    io.parse_inp_hydraulics(text=text.replace(old, new))   # without the keyword the options are not read, as they never were


def test_the_keyword_itself_is_checked():
    with pytest.raises(ValueError, match="demand_model must be"):
        io.parse_inp_hydraulics(FIXTURE, demand_model="pda")
    with pytest.raises(ValueError, match="PRESSURE METERS does not go with UNITS GPM"):
        io.parse_inp_hydraulics(text=open(FIXTURE).read().replace(" HEADLOSS            H-W", " HEADLOSS            H-W\n PRESSURE   METERS"),
                                demand_model="model")


def test_solve_ref_on_what_was_read_starves_the_high_junctions(parsed, capsys):
    net = parsed.network
    demand, rough = parsed.demand[None, :], parsed.roughness[None, :]
    ref = H.solve_ref(net, demand, rough, **pdd_kw(parsed))
    old = H.solve_ref(net, demand, rough)
    p = (ref.head - net.elevation)[0]
    share = ref.demand_delivered[0, :6] / parsed.demand[:6].clip(1e-300)
    with capsys.disabled():
        print(f"wdn_deficient: iterations {ref.iterations.tolist()}  pressures {p[:6].round(2).tolist()} m  delivered share {share.round(3).tolist()}  "
              f"demand-driven pressures {(old.head - net.elevation)[0, :6].round(2).tolist()}")
    assert ref.converged.all() and old.converged.all()
    assert p[5] < parsed.minimum_pressure and ref.demand_delivered[0, 5] <= 0                        # J6: above the source head
    assert parsed.minimum_pressure < p[4] < parsed.required_pressure and 0.05 < share[4] < 0.95       # J5: below Preq
    assert (p[1:4] > parsed.required_pressure).all() and np.allclose(share[1:4], 1.0, rtol=1e-4)
    assert ref.demand_delivered[0, 0] == 0 and ref.demand_delivered[0, 6] == 0                        # no demand; the reservoir
    mass, energy = H.hydraulic_residuals(net, ref.head, ref.flow, demand, rough, link_state=ref.link_state,
                                         demand_delivered=ref.demand_delivered, **pdd_kw(parsed))
    assert mass.max() <= 10 * H.ACCURACY and energy.max() <= 1e-5
    ser = H.simulate_series_ref(net, demand, rough, parsed.multipliers, 3600.0, pattern_of_node=parsed.pattern_of_node, **pdd_kw(parsed))
    assert ser.converged.all() and ser.demand_delivered.shape == (1, 2, 7)
