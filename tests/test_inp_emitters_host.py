"""``wdn_io.parse_inp_hydraulics(emitters="model")`` on the host: the hand-written fixture tests/golden/wdn_leaky.inp gives the
emitter junctions, the exponent of [OPTIONS] and the coefficients in SI units, checked against values computed here; the pressure
units convert; the default call gives the network it always gave (the file is read as tight); an emitter on a reservoir is
refused by name; ``solve_ref`` converges on what was read and the leaks obey q = C p^gamma.  No GPU."""
import os

import numpy as np
import pytest

import hydraulics_refs as HR

H, G = HR.H, HR.G
io = G.wdn_io
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wdn_leaky.inp")
NODES = ["K1", "K2", "K3", "K4", "K5", "K6", "K7", "K8", "SRC"]
FILE_COEF, GAMMA = np.array([0.35, 0.05]), 0.6             # L/s per m^0.6, as the file has them


@pytest.fixture(scope="module")
def parsed():
    return io.parse_inp_hydraulics(FIXTURE, emitters="model")


def test_the_fixture_parses_to_junctions_exponent_and_coefficients_in_si(parsed):
    net = parsed.network
    assert parsed.node_names == NODES and (net.num_nodes, net.num_pipes, net.num_emitters) == (9, 9, 2)
    assert net.emitter_nodes.tolist() == [3, 7] and net.emitter_exponent == GAMMA and net.has_emitters
    want = FILE_COEF * 1e-3                                 # LPS and metres: the pressure unit is the metre, so only the flow converts
    print("emitter_coefficient", parsed.emitter_coefficient.tolist(), "computed here", want.tolist())
    assert parsed.emitter_coefficient.dtype == np.float64 and np.array_equal(parsed.emitter_coefficient, want)


def test_flow_and_pressure_units_convert():
    text = open(FIXTURE).read()
    kpa = io.parse_inp_hydraulics(text=text.replace(" HEADLOSS           H-W", " HEADLOSS           H-W\n PRESSURE   KPA"), emitters="model")
    m_per_kpa = 0.3048 / 0.4333 / 6.895                     # EPANET's own constants, as the valve settings use them
    assert np.allclose(kpa.emitter_coefficient, FILE_COEF * 1e-3 / m_per_kpa ** GAMMA, rtol=1e-15)
    gpm = io.parse_inp_hydraulics(text=text.replace("UNITS              LPS", "UNITS              GPM"), emitters="model")
    m_per_psi = 0.3048 / 0.4333
    assert np.allclose(gpm.emitter_coefficient, FILE_COEF * (3.785411784e-3 / 60.0) / m_per_psi ** GAMMA, rtol=1e-15)
    default = io.parse_inp_hydraulics(text=text.replace(" EMITTER EXPONENT   0.6\n", ""), emitters="model")
    assert default.network.emitter_exponent == 0.5 and np.array_equal(default.emitter_coefficient, FILE_COEF * 1e-3)
    with pytest.raises(ValueError, match="PRESSURE"):
        io.parse_inp_hydraulics(text=text.replace(" HEADLOSS           H-W", " HEADLOSS           H-W\n PRESSURE   PSI"), emitters="model")
    with pytest.raises(ValueError, match="emitters"):
        io.parse_inp_hydraulics(FIXTURE, emitters="read")


def test_the_default_call_gives_the_network_it_always_gave(parsed):
    text = open(FIXTURE).read()
    start, end = text.index("[EMITTERS]"), text.index("[PATTERNS]")
    tight = io.parse_inp_hydraulics(text=text[:start] + text[end:])
    for kw in ({}, {"emitters": None}):
        r = io.parse_inp_hydraulics(FIXTURE, **kw)
        assert r.emitter_coefficient is None and r.network.num_emitters == 0 and not r.network.has_emitters
        for k in ("pipes", "length", "diameter", "elevation", "fixed_head", "coef", "q_start", "minor_loss", "order"):
            assert np.array_equal(getattr(r.network, k), getattr(tight.network, k)), k
        assert np.array_equal(r.demand, tight.demand) and np.array_equal(r.multipliers, tight.multipliers)
        assert r.node_names == tight.node_names and r.link_names == tight.link_names
    for k in ("pipes", "length", "diameter", "elevation", "fixed_head", "coef", "q_start"):      # the emitters change nothing else
        assert np.array_equal(getattr(parsed.network, k), getattr(tight.network, k)), k


@pytest.mark.parametrize("old, new, match", [
    (" K8         0.05", " SRC        0.05", r"\[EMITTERS\] SRC: an emitter sits on a junction"),
    (" K8         0.05", " K9         0.05", r"\[EMITTERS\] K9: no such node"),
    (" K8         0.05", " K4         0.05", r"\[EMITTERS\] K4: listed twice"),
    (" K8         0.05", " K8         -0.05", r"\[EMITTERS\] K8: the coefficient -0.05"),
    (" K8         0.05", " K8", r"\[EMITTERS\] K8: needs a junction and a coefficient"),
])
def test_bad_emitter_lines_are_refused_by_name(old, new, match):
    text = open(FIXTURE).read().replace(old, new)
    with pytest.raises(ValueError, match=match):
        io.parse_inp_hydraulics(text=text, emitters="model")
    io.parse_inp_hydraulics(text=text)                      # (not read by default: as ever)


def test_solve_ref_converges_on_what_was_read_and_the_leaks_obey_their_law(parsed):
    net = parsed.network
    demand, rough = parsed.demand[None, :], parsed.roughness[None, :]
    ref = H.solve_ref(net, demand, rough, emitter_coefficient=parsed.emitter_coefficient, solver="banded")
    tight = H.solve_ref(io.parse_inp_hydraulics(FIXTURE).network, demand, rough, solver="banded")
    p = ref.head[0, net.emitter_nodes] - net.elevation[net.emitter_nodes]
    print("iterations", ref.iterations.tolist(), "pressures at the emitters", p.tolist(), "leaks", ref.emitter_flow[0].tolist())
    assert ref.converged.all() and tight.converged.all()
    assert np.allclose(ref.emitter_flow[0], parsed.emitter_coefficient * p ** GAMMA, rtol=10 * H.ACCURACY)
    assert (ref.head[0, ~net.fixed] < tight.head[0, ~net.fixed]).all()       # a leak lowers every junction's head
    mass, energy = H.hydraulic_residuals(net, ref.head, ref.flow, demand, rough, link_state=ref.link_state,
                                         emitter_flow=ref.emitter_flow, emitter_coefficient=parsed.emitter_coefficient)
    assert mass.max() < 1e-9 and energy.max() < 1e-9
