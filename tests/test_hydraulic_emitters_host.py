"""The emitters (leaks) of the hydraulic solver on the host: the symbols and what the constructor refuses; ``emitter_headloss`` on
its four branches; the draws against ``mix64`` worked by hand; the closed forms and the bisection roots of
hydraulic_emitters_refs.py from ``solve_ref``; planted wrong answers caught by ``hydraulic_residuals``; a network whose
coefficients are all 0 has every bit of the network without emitters; the series reference before and after an onset, and its
volume balance with and without the leaked volume.  No GPU.  Every figure is printed before it is asserted."""
import os
import re

import numpy as np
import pytest

import hydraulic_emitters_refs as ER
import hydraulics_refs as HR

H, G = HR.H, HR.G
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK = (1 << 64) - 1


# ---- symbols and refusals ---------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_the_abi_stays():
    header = open(os.path.join(ROOT, "include", "gatres.h")).read()
    for name in ("gatres_hydraulic_solve_emitters", "gatres_hydraulic_series_emitters"):
        assert re.search(r"\bint " + name + r"\(", header) and name in G._native.SIGNATURES
    assert "THE EMITTERS" in header and "#define GATRES_ABI_VERSION 9" in header and G._native.ABI_VERSION == 9
    for name in ("HydraulicEmittersResult", "HydraulicSeriesEmittersResult", "emitter_headloss", "hydraulic_emitter_draws"):
        assert name in G.__all__ and hasattr(G, name)
    assert H.HydraulicEmittersResult._fields == H.HydraulicValvesResult._fields + ("emitter_flow",)
    assert H.HydraulicSeriesEmittersResult._fields == H.HydraulicSeriesValvesResult._fields + ("emitter_flow",)


def test_lds_need_is_the_valves_launch_and_48_bytes_per_emitter():
    assert H.emitters_lds_bytes(40, 44, 5, 1, 2, 0) == H.valves_lds_bytes(40, 44, 5, 1, 2)
    assert H.emitters_lds_bytes(40, 44, 5, 1, 2, 3) == H.valves_lds_bytes(40, 44, 5, 1, 2) + 144
    assert H.series_emitters_lds_bytes(40, 44, 5, 2, 1, 2, 3) == H.series_valves_lds_bytes(40, 44, 5, 2, 1, 2) + 144
    header = open(os.path.join(ROOT, "include", "gatres.h")).read()
    assert "48 Ke" in header


def _chain_net(**kw):
    args = dict(edge_index=HR._edge_index([(0, 1), (1, 2), (2, 3)]), length=[100.0, 0.0, 100.0], diameter=np.full(3, 0.2),
                elevation=np.zeros(4), fixed_nodes=[0], fixed_head=[50.0])
    args.update(kw)
    return H.HydraulicNetwork(**args)


@pytest.mark.parametrize("kw, match", [
    (dict(emitter_nodes=[1], emitter_exponent=float("nan")), "emitter_exponent"),
    (dict(emitter_nodes=[1], emitter_exponent=float("inf")), "emitter_exponent"),
    (dict(emitter_nodes=[1], emitter_exponent=0.0), "emitter_exponent"),
    (dict(emitter_nodes=[1], emitter_exponent=-0.5), "emitter_exponent"),
    (dict(emitter_nodes=[1], emitter_exponent=1e-320), "emitter_exponent"),
    (dict(emitter_nodes=[4]), "distinct nodes"),
    (dict(emitter_nodes=[-1]), "distinct nodes"),
    (dict(emitter_nodes=[1, 1]), "distinct nodes"),
    (dict(emitter_nodes=[0]), "fixed-head"),
    (dict(emitter_nodes=[2], minor_loss=[0.0, 2.0, 0.0], valve_links=[1], valve_kind="PRV", valve_setting=[30.0]), "controlled node"),
])
def test_the_constructor_refuses_what_the_header_refuses(kw, match):
    with pytest.raises(ValueError, match=match):
        _chain_net(length=[100.0, 100.0 if "valve_links" not in kw else 0.0, 100.0], **kw)


def test_an_emitter_beside_a_valve_is_accepted_at_the_uncontrolled_end():
    net = _chain_net(emitter_nodes=[1, 3], minor_loss=[0.0, 2.0, 0.0], valve_links=[1], valve_kind="PRV", valve_setting=[30.0])
    assert net.num_emitters == 2 and net.has_emitters and net.emitter_exponent == 0.5 and net.valve_node.tolist() == [2]
    plain = _chain_net(length=[100.0, 100.0, 100.0])
    assert plain.num_emitters == 0 and not plain.has_emitters


def test_the_references_refuse_a_network_with_emitters_without_coefficients():
    c = ER.case("chain_hw")
    with pytest.raises(ValueError, match="emitter_coefficient"):
        H.solve_ref(c["net"], c["demand"], c["roughness"])
    with pytest.raises(ValueError, match="emitter_flow"):
        H.hydraulic_residuals(c["net"], np.zeros((3, 2)), np.zeros((3, 1)), c["demand"], c["roughness"], link_state=np.zeros((3, 1)))


# ---- the law ----------------------------------------------------------------------------------------------------------------------------
def test_emitter_headloss_on_its_four_branches():
    # forward: h = (q / C)^(1 / gamma), g = h / (gamma q)
    for gamma, C, q in ((0.5, 1e-3, 5e-3), (1.0, 2e-5, 1e-3), (1.18, 1e-4, 2e-3), (ER.GAMMA_HW, 2e-3, 1e-2)):
        h, g = H.emitter_headloss(q, C, gamma)
        print(f"forward gamma={gamma}: h {float(h):.17g} g {float(g):.17g}")
        assert np.isclose(h, (q / C) ** (1.0 / gamma), rtol=1e-14) and np.isclose(g, h / (gamma * q), rtol=1e-14)
        assert H.LINEAR_GRADIENT <= g <= H.SHUT_GRADIENT
    # the linear floor: gamma < 1 at q -> 0 (g = n ce q^(n - 1) -> 0)
    h, g = H.emitter_headloss([0.0, 1e-14], 1e-3, 0.5)
    assert (g == H.LINEAR_GRADIENT).all() and (h == H.LINEAR_GRADIENT * np.array([0.0, 1e-14])).all()
    # the cap: gamma > 1 at q -> 0 (g -> inf, at q = 0 not finite), and a coefficient so small that ce overflows
    h, g = H.emitter_headloss([0.0, 1e-300], 1e-4, 1.18)
    assert (g == H.SHUT_GRADIENT).all() and (h == H.SHUT_GRADIENT * np.array([0.0, 1e-300])).all()
    h, g = H.emitter_headloss([0.0, 1e-3], 1e-200, 0.5)
    assert (g == H.SHUT_GRADIENT).all() and (h == H.SHUT_GRADIENT * np.array([0.0, 1e-3])).all()
    # gamma = 1 at q = 0: pow(0, 0) is 1, g = 1 / C
    h, g = H.emitter_headloss(0.0, 1e-3, 1.0)
    assert h == 0.0 and np.isclose(g, 1e3, rtol=1e-15)
    # reverse: a leak takes no water in
    h, g = H.emitter_headloss([-1e-9, -0.5], 1e-3, 0.5)
    assert (g == H.SHUT_GRADIENT).all() and (h == H.SHUT_GRADIENT * np.array([-1e-9, -0.5])).all()
    # continuous and monotone across q = 0 up to the jump of the floor
    q = np.linspace(-1e-6, 1e-2, 2001)
    h, _ = H.emitter_headloss(q, 1e-3, 0.5)
    assert (np.diff(h) > 0).all()


# ---- the draws ----------------------------------------------------------------------------------------------------------------------------
def _mix64(z):
    z &= MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def _uniform(seed, scenario, cell):
    """The uniform number of the 1-based ``cell`` of the global ``scenario``, with Python integers."""
    stream = _mix64(seed + 0x9E3779B97F4A7C15 * (scenario + 1))
    return (_mix64(stream + 0xBF58476D1CE4E5B9 * cell) >> 11) * 2.0 ** -53


def test_emitter_draws_against_mix64_by_hand():
    net = G.wdn_synth.make_hydraulic_network(37, 41, 1, seed=3, num_prvs=1, valve_seed=6, num_emitters=2)
    N, P, Kp, Kv, Ke = net.num_nodes, net.num_pipes, net.num_pumps, net.num_valves, net.num_emitters
    ranges = net.draw_ranges((1e-4, 1e-3), H.ROUGHNESS_RANGE)
    seed, first, S, c_rng, prob, o_rng = 21, 5, 6, (1e-5, 3e-4), 0.6, (2, 9)
    d, r, w, cl, vs, coef, onset = H.hydraulic_emitter_draws(seed, first, S, *ranges, Kp, Kv, Ke, c_rng, prob, o_rng)
    assert coef.shape == (S, Ke) and onset.shape == (S, Ke) and onset.dtype == np.int32 and vs.shape == (S, Kv) and not vs.any()
    base = N + 2 * P + Kp + Kv                              # the cells before the emitters', 1-based cells start at base + 1
    for s, k in ((0, 0), (3, 1), (5, 0)):
        u_c, u_p, u_o = (_uniform(seed, first + s, base + j * Ke + k + 1) for j in range(3))
        want = c_rng[0] + (c_rng[1] - c_rng[0]) * u_c if u_p < prob else 0.0
        print(f"draws[{s},{k}]: u {u_c:.17g} {u_p:.17g} {u_o:.17g}  C {coef[s, k]:.17g}  onset {onset[s, k]}")
        assert coef[s, k] == want and onset[s, k] == int(np.floor(o_rng[0] + (o_rng[1] - o_rng[0]) * u_o))
    assert (coef == 0).any() and (coef > 0).any() and onset.min() >= 2 and onset.max() < 9
    # the cells before are what they are without the emitters
    d0, r0 = H.hydraulic_draws(seed, first, S, *ranges)
    assert d.tobytes() == d0.tobytes() and r.tobytes() == r0.tobytes()
    d1, r1, w1, cl1, vs1 = H.hydraulic_valve_draws(seed, first, S, *ranges, Kp, Kv, (20.0, 40.0))
    got = H.hydraulic_emitter_draws(seed, first, S, *ranges, Kp, Kv, Ke, c_rng, valve_setting_range=(20.0, 40.0))
    assert got[4].tobytes() == vs1.tobytes() and got[3].tobytes() == cl1.tobytes() and got[6] is None and (got[5] > 0).all()


def test_make_hydraulic_network_places_emitters_after_everything_else():
    base = G.wdn_synth.make_hydraulic_network(40, 44, 2, seed=5, num_prvs=2, num_psvs=1, valve_seed=3)
    net = G.wdn_synth.make_hydraulic_network(40, 44, 2, seed=5, num_prvs=2, num_psvs=1, valve_seed=3, num_emitters=3,
                                             emitter_exponent=1.18)
    for k in ("pipes", "length", "diameter", "elevation", "fixed_head", "valve_links", "valve_setting", "minor_loss"):
        assert np.array_equal(getattr(base, k), getattr(net, k)), k
    assert net.num_emitters == 3 and net.emitter_exponent == 1.18 and np.unique(net.emitter_nodes).size == 3
    assert not net.fixed[net.emitter_nodes].any() and not np.isin(net.emitter_nodes, net.valve_node).any()
    other = G.wdn_synth.make_hydraulic_network(40, 44, 2, seed=5, num_emitters=3, emitter_seed=1)
    assert not np.array_equal(np.sort(other.emitter_nodes), np.sort(net.emitter_nodes))
    with pytest.raises(ValueError, match="num_emitters"):
        G.wdn_synth.make_hydraulic_network(4, 3, 1, seed=1, num_emitters=4)


# ---- closed forms and bisection roots from solve_ref -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tuple(n for n in ER.CHAINS if n != "chain_shut"))
@pytest.mark.parametrize("solver", ("dense", "banded"))
def test_solve_ref_meets_the_closed_forms_and_the_bisection_roots(name, solver, capsys):
    """Newton stops at sum |dq| <= ACCURACY x sum |q|, so no flow is determined better than ACCURACY x the flow: that is the
    bound (the last step is quadratic, the error far below it)."""
    c, exact = ER.case(name), ER.chain_exact(name)
    ref = ER.solve(c, solver)
    err = np.abs(ref.emitter_flow[:, 0] - exact) / exact
    with capsys.disabled():
        print(f"{name} {solver}: iterations {ref.iterations.tolist()}  q_e {ref.emitter_flow[:, 0].tolist()}  relative error {err.tolist()}")
    assert ref.converged.all() and not ref.failed.any()
    assert (err <= H.ACCURACY).all()
    e = int(c["net"].emitter_nodes[0])
    p = ref.head[:, e] - c["net"].elevation[e]
    assert np.allclose(ref.emitter_flow[:, 0], c["coef"][:, 0] * p ** c["net"].emitter_exponent, rtol=10 * H.ACCURACY)      # q = C p^gamma


def test_a_shut_emitter_carries_the_negative_pressure_over_1e8(capsys):
    c, ref = ER.case("chain_shut"), ER.reference("chain_shut")["dense"]
    p = ref.head[:, 1] - c["net"].elevation[1]
    with capsys.disabled():
        print(f"chain_shut: pressure {p.tolist()}  q_e {ref.emitter_flow[:, 0].tolist()}")
    assert (p < 0).all() and (ref.emitter_flow[:, 0] <= 0).all() and (np.abs(ref.emitter_flow[:, 0]) <= np.abs(p) / 1e8 * (1 + 1e-9)).all()


# ---- planted wrong answers ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("chain_hw", "chain3_g118", "net37_e2_g1", "net40_e3_g118"))
@pytest.mark.parametrize("kind", ER.WRONG)
def test_hydraulic_residuals_catch_planted_wrong_answers(name, kind, capsys):
    c, ref = ER.case(name), ER.reference(name)
    mass, energy = ER.wrong_residuals(kind, c, ref["dense"])
    with capsys.disabled():
        print(f"{name} {kind}: mass {mass.max():.3e} (right {ref['mass'].max():.3e})  energy {energy.max():.3e} (right {ref['energy'].max():.3e})")
    if kind == "leak_forgotten":                            # the imbalance left at an emitter's junction is its |q_e|
        d = ref["dense"]
        left = np.abs(d.emitter_flow).max(axis=1) / np.abs(d.flow).sum(axis=1)
        assert (mass >= 0.99 * left).all() and mass.max() > 1e-3 and mass.max() > 1e6 * ref["mass"].max()
    else:
        assert (energy > 1e-2).any() and energy.max() > 1e6 * ref["energy"].max()


# ---- no emitter that is on: every bit of the network without emitters -----------------------------------------------------------------------
@pytest.mark.parametrize("name", ("net37_e2_g1", "net40_e2_g05"))
def test_all_coefficients_zero_give_every_bit_of_the_network_without_emitters(name):
    c = ER.case(name)
    args = ER.SYNTHETIC[name]
    plain = G.wdn_synth.make_hydraulic_network(*args[:3], seed=args[4], num_prvs=args[6], num_psvs=args[7], valve_seed=args[8])
    zero = H.solve_ref(c["net"], c["demand"], c["roughness"], valve_setting=c["setting"], emitter_coefficient=np.zeros_like(c["coef"]),
                       solver="banded")
    old = H.solve_ref(plain, c["demand"], c["roughness"], valve_setting=c["setting"], valves=True, solver="banded")
    for k in ("head", "flow", "iterations", "converged", "failed", "final_dq", "link_state", "valve_changes"):
        assert getattr(zero, k).tobytes() == getattr(old, k).tobytes(), k
    assert zero.emitter_flow.shape == c["coef"].shape and not zero.emitter_flow.any() and not np.signbit(zero.emitter_flow).any()
    one = c["coef"].copy()
    one[:, 1:] = 0.0                                        # one emitter on, the others off: the off ones stay at +0.0
    mixed = H.solve_ref(c["net"], c["demand"], c["roughness"], valve_setting=c["setting"], emitter_coefficient=one, solver="banded")
    assert mixed.converged.all() and not mixed.emitter_flow[:, 1:].any() and mixed.emitter_flow[:, 0].any()


def test_a_bad_coefficient_fails_its_scenario_alone():
    c = ER.case("net40_e2_g05")
    good = ER.solve(c, "banded")
    for bad_value in (-1e-5, np.nan, np.inf):
        coef = c["coef"].copy()
        coef[2, 1] = bad_value
        bad = H.solve_ref(c["net"], c["demand"], c["roughness"], emitter_coefficient=coef, solver="banded")
        assert bad.failed.tolist() == [False, False, True, False] and np.isnan(bad.head[2]).all() and np.isnan(bad.emitter_flow[2]).all()
        for k in ("head", "flow", "emitter_flow"):
            assert getattr(bad, k)[[0, 1, 3]].tobytes() == getattr(good, k)[[0, 1, 3]].tobytes(), k


# ---- the series reference -----------------------------------------------------------------------------------------------------------------
def leaky_series():
    """reservoir 0 (60 m) -- 1 -- 2 with the demand and a leak -- tank 3 (bottom at 30 m, 3 m of water)."""
    net = H.HydraulicNetwork(HR._edge_index([(0, 1), (1, 2), (2, 3)]), [400.0, 100.0, 200.0], np.full(3, 0.2), [0.0, 0.0, 5.0, 30.0],
                             [0, 3], [60.0, 33.0], tank_nodes=[3], tank_diameter=[8.0], emitter_nodes=[2, 1])
    plain = H.HydraulicNetwork(HR._edge_index([(0, 1), (1, 2), (2, 3)]), [400.0, 100.0, 200.0], np.full(3, 0.2), [0.0, 0.0, 5.0, 30.0],
                               [0, 3], [60.0, 33.0], tank_nodes=[3], tank_diameter=[8.0])
    demand = np.zeros((2, 4))
    demand[:, 2] = [0.01, 0.015]
    coef = np.array([[1e-3, 0.0], [2e-3, 5e-4]])
    onset = np.array([[3, 0], [2, 4]])
    return net, plain, demand, np.full((2, 3), 100.0), np.array([[0.8, 1.0, 1.2, 1.0, 0.9, 1.1]]), 600.0, coef, onset


@pytest.mark.parametrize("warm", (True, False))
def test_series_reference_onset_and_volume_balance(warm, capsys):
    net, plain, demand, rough, mult, dt, coef, onset = leaky_series()
    ref = H.simulate_series_ref(net, demand, rough, mult, dt, warm_start=warm, emitter_coefficient=coef, emitter_onset=onset)
    old = H.simulate_series_ref(plain, demand, rough, mult, dt, warm_start=warm, valves=True)
    assert ref.converged.all() and ref.emitter_flow.shape == (2, 6, 2)
    T = mult.shape[1]
    on = (np.arange(T)[None, :, None] >= onset[:, None, :]) & (coef[:, None, :] > 0)
    assert ((ref.emitter_flow > 0) == on).all() and not np.signbit(ref.emitter_flow[~on]).any()
    first = np.where(coef > 0, onset, T).min(axis=1)       # the first step at which any emitter of the series is on
    assert first.tolist() == [3, 2]
    for s in range(2):                                      # before the first onset: the bits of the series without emitters
        for k in ("head", "flow", "iterations", "final_dq"):
            assert getattr(ref, k)[s, :first[s]].tobytes() == getattr(old, k)[s, :first[s]].tobytes(), (s, k)
        assert ref.level[s, :first[s] + 1].tobytes() == old.level[s, :first[s] + 1].tobytes()
        assert ref.head[s, first[s]].tobytes() != old.head[s, first[s]].tobytes()
    bal = np.abs(H.series_volume_balance(net, ref, demand, mult, dt))
    without = H.series_volume_balance(net, ref, demand, mult, dt, count_leaks=False)
    leaked = dt * ref.emitter_flow.sum(axis=2)
    qmax = np.abs(ref.flow).max()
    with capsys.disabled():
        print(f"leaky_series warm={warm}: iterations {ref.iterations.tolist()}  balance {bal.max():.3e} m3  "
              f"leaked up to {leaked.max():.3e} m3  balance without the leak {np.abs(without).max():.3e} m3")
    assert bal.max() <= dt * H.ACCURACY * qmax               # what the stop rule leaves open in one step
    assert np.abs(without + leaked).max() <= dt * H.ACCURACY * qmax and leaked.max() > 1e3 * dt * H.ACCURACY * qmax


def test_a_bad_coefficient_fails_its_series_from_step_0():
    net, plain, demand, rough, mult, dt, coef, onset = leaky_series()
    coef = coef.copy()
    coef[1, 1] = -1.0                                       # (its onset is step 4: the series fails from step 0 all the same)
    ref = H.simulate_series_ref(net, demand, rough, mult, dt, emitter_coefficient=coef, emitter_onset=onset)
    assert ref.failed[1].all() and not ref.failed[0].any() and np.isnan(ref.emitter_flow[1]).all()


# ---- the generated store's scenarios, on the host ---------------------------------------------------------------------------------------------
def test_the_store_parameters_keep_64_of_64_on_the_host(capsys):
    """What test_gpu_hydraulic_emitters.py relies on: ``solve_ref`` alone converges inside the pressure range on all 64 scenarios
    that ``generate_store`` draws with the parameters of hydraulic_emitters_refs.py, with leaking and tight emitters among them."""
    net = ER.store_network()
    ranges = net.draw_ranges(ER.STORE_DEMAND, H.ROUGHNESS_RANGE)
    d, r, _, _, _, coef, _ = H.hydraulic_emitter_draws(ER.STORE_SEED, 0, ER.STORE_SCENARIOS, *ranges, 0, 0, net.num_emitters,
                                                       ER.STORE_COEF, ER.STORE_LEAK_P)
    ref = H.solve_ref(net, d, r, emitter_coefficient=coef, solver="banded")
    p = (ref.head - net.elevation[None, :])[:, ~net.fixed].astype(np.float32)
    inside = ((p >= ER.STORE_PRESSURE[0]) & (p <= ER.STORE_PRESSURE[1])).all(axis=1)
    with capsys.disabled():
        print(f"store scenarios on the host: converged {int(ref.converged.sum())} of {ER.STORE_SCENARIOS}, iterations "
              f"{int(ref.iterations.min())} .. {int(ref.iterations.max())}, pressures {p.min():.2f} .. {p.max():.2f} m, "
              f"leaking emitters {int((coef > 0).sum())} of {coef.size}")
    assert ref.converged.all() and not ref.failed.any() and inside.all()
    assert (coef > 0).any() and (coef == 0).any() and ((ref.emitter_flow > 0) == (coef > 0)).all()
