"""Pressure-driven demand in the host statements of the hydraulic solver (hydraulics.py: ``demand_headloss``, ``solve_ref`` and
``simulate_series_ref`` with ``demand_model="pda"``, ``hydraulic_residuals``, ``series_volume_balance``): the law on its branches,
the closed forms and the shooting roots of hydraulic_pdd_refs.py, a junction above the required and one below the minimum
pressure, agreement with the demand-driven solver where every junction is well supplied, an inflow that stays an inflow, planted
wrong answers, the series, the LDS sums and the refusals.  No GPU.  Every figure is printed before it is asserted."""
import os
import re

import numpy as np
import pytest

import hydraulic_pdd_refs as PR
import hydraulics_refs as HR

H, G = HR.H, HR.G
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_declared_exported_and_the_abi_stays():
    header = open(os.path.join(ROOT, "include", "gatres.h")).read()
    for name in ("gatres_hydraulic_solve_pdd", "gatres_hydraulic_series_pdd"):
        assert re.search(r"\bint " + name + r"\(", header) and name in G._native.SIGNATURES
    assert "THE PRESSURE-DRIVEN DEMAND" in header and "#define GATRES_ABI_VERSION 9" in header and G._native.ABI_VERSION == 9
    for name in ("HydraulicPddResult", "HydraulicSeriesPddResult", "demand_headloss", "pdd_lds_bytes", "series_pdd_lds_bytes"):
        assert name in G.__all__ and hasattr(G, name)
    assert H.HydraulicPddResult._fields == H.HydraulicEmittersResult._fields + ("demand_delivered",)
    assert H.HydraulicSeriesPddResult._fields == H.HydraulicSeriesEmittersResult._fields + ("demand_delivered",)
    assert len(G._native.SIGNATURES["gatres_hydraulic_solve_pdd"][1]) == len(G._native.SIGNATURES["gatres_hydraulic_solve_emitters"][1]) + 5


def test_lds_need_is_the_emitters_launch_and_32_bytes_per_node():
    assert H.pdd_lds_bytes(40, 44, 5, 1, 2, 3, 0) == H.emitters_lds_bytes(40, 44, 5, 1, 2, 3)
    assert H.pdd_lds_bytes(40, 44, 5, 1, 2, 3) == H.emitters_lds_bytes(40, 44, 5, 1, 2, 3) + 32 * 40
    assert H.series_pdd_lds_bytes(40, 44, 5, 2, 1, 2, 3) == H.series_emitters_lds_bytes(40, 44, 5, 2, 1, 2, 3) + 32 * 40
    assert H.series_pdd_lds_bytes(40, 44, 5, 2, 1, 2, 3, 0) == H.series_emitters_lds_bytes(40, 44, 5, 2, 1, 2, 3)
    net = PR.case("net388")["net"]                          # the figures of the 388-node network
    assert H.emitters_lds_bytes(388, 430, net.half_bandwidth, 0, 0, 0) == 92264
    assert H.pdd_lds_bytes(388, 430, net.half_bandwidth, 0, 0, 0) == 92264 + 12416 <= H.LDS_BUDGET
    header = open(os.path.join(ROOT, "include", "gatres.h")).read()
    assert "32 N" in header


def test_demand_headloss_on_its_branches():
    D, dp = 0.01, 25.0
    for e in (0.5, PR.E_HW, 1.0):                           # inside: h = dp (q / D)^n, g = n h / q
        n = 1.0 / e
        q = np.array([0.002, 0.005, 0.01])
        h, g = H.demand_headloss(q, D, dp, e)
        assert np.allclose(h, dp * (q / D) ** n, rtol=1e-14) and np.allclose(g, n * h / q, rtol=1e-14)
        assert (np.diff(h) > 0).all() and np.isclose(h[-1], dp, rtol=1e-14)
    h, g = H.demand_headloss(np.array([-1e-9, -0.5]), D, dp, 0.5)                 # no demand node feeds the network
    assert (g == H.SHUT_GRADIENT).all() and (h == H.SHUT_GRADIENT * np.array([-1e-9, -0.5])).all()
    h, g = H.demand_headloss(np.array([0.0100001, 0.02]), D, dp, 0.5)             # above the required pressure
    assert (g == H.SHUT_GRADIENT).all() and (h == dp + H.SHUT_GRADIENT * (np.array([0.0100001, 0.02]) - D)).all()
    h, g = H.demand_headloss(np.array([0.0, 1e-14]), D, dp, 0.5)                  # the linear floor at rest (n = 2: g -> 0)
    assert (g == H.LINEAR_GRADIENT).all() and (h == H.LINEAR_GRADIENT * np.array([0.0, 1e-14])).all()
    h, g = H.demand_headloss(np.array([0.0, 1e-300]), D, dp, 2.0)                 # n = 1 / 2: g -> inf at rest
    assert (g == H.SHUT_GRADIENT).all() and (h == H.SHUT_GRADIENT * np.array([0.0, 1e-300])).all()
    h, g = H.demand_headloss(0.0, D, dp, 1.0)                                     # n = 1: pow(0, 0) is 1
    assert h == 0.0 and np.isclose(g, dp / D, rtol=1e-15)


@pytest.mark.parametrize("solver", ("dense", "banded"))
@pytest.mark.parametrize("name", PR.CLOSED_FORMS)
def test_solve_ref_meets_the_closed_forms_and_the_shooting_roots(name, solver, capsys):
    """Within what the stop rule leaves open: a relative error of ACCURACY."""
    c, exact = PR.case(name), PR.chain_exact(name)
    ref = PR.solve(c, solver)
    err = np.abs(ref.demand_delivered[:, 1:] - exact) / exact
    with capsys.disabled():
        print(f"{name} {solver}: iterations {ref.iterations.tolist()}  q_d {ref.demand_delivered[:, 1:].tolist()}  exact {exact.tolist()}  "
              f"relative error {err.max():.3e}")
    assert ref.converged.all() and not ref.failed.any()
    assert (err <= H.ACCURACY).all()
    pmin, preq, e = c["pdd"]
    p = ref.head[:, 1:] - c["net"].elevation[1:]
    assert np.allclose(ref.demand_delivered[:, 1:], c["demand"][:, 1:] * ((p - pmin) / (preq - pmin)) ** e, rtol=10 * H.ACCURACY)
    assert (ref.demand_delivered[:, 0] == 0).all()          # 0 at the fixed-head node


def test_above_the_required_pressure_the_demand_is_delivered_to_within_the_leak_of_a_shut_link(capsys):
    c = PR.case("chain_full")
    ref = PR.solve(c)
    p = ref.head[:, 1] - c["net"].elevation[1]
    over = ref.demand_delivered[:, 1] - c["demand"][:, 1]
    with capsys.disabled():
        print(f"chain_full: iterations {ref.iterations.tolist()}  pressure {p.tolist()}  q_d - D {over.tolist()}")
    assert ref.converged.all() and (p > c["pdd"][1]).all() and (over >= 0).all()
    assert (over <= (p - c["pdd"][1]) / 1e8 * (1 + 1e-6) + 4 * HR.EPS * c["demand"][:, 1]).all()


def test_below_the_minimum_pressure_the_junction_carries_the_shortfall_over_1e8(capsys):
    c = PR.case("chain_above")
    ref = PR.solve(c)
    p = ref.head[:, 1] - c["net"].elevation[1]
    q = ref.demand_delivered[:, 1]
    with capsys.disabled():
        print(f"chain_above: iterations {ref.iterations.tolist()}  pressure {p.tolist()}  q_d {q.tolist()}")
    assert ref.converged.all() and (p < c["pdd"][0]).all() and (q <= 0).all()
    assert (np.abs(q) <= np.abs(p - c["pdd"][0]) / 1e8 * (1 + 1e-9)).all()
    assert np.abs(ref.flow[:, 0]).max() <= 100.0 / 1e8


@pytest.mark.parametrize("name", ("net37", "net388"))
def test_with_the_required_pressure_far_below_every_pressure_the_heads_are_the_demand_driven_ones(name, capsys):
    """Every junction is on the branch q_d = D + (p - Preq) / 1e8: the delivered flows exceed the demands by at most the largest
    (p - Preq) / 1e8, and the heads move by no more than that surplus flowing through the whole network can move them.  A head
    loss goes with q^1.852, so raising every flow by the share x = total surplus / total demand raises every head loss by
    1.852 x to first order, and no head moves by more than 1.852 x times the span of the heads; the bound takes 2 x span, and
    adds what the stop rule leaves open."""
    net, demand, roughness, _ = HR.case({"net37": "net37_s3", "net388": "net388_s3"}[name])
    dda = H.solve_ref(net, demand, roughness, solver="banded")
    p_dda = (dda.head - net.elevation)[:, ~net.fixed]
    preq = float(np.floor(p_dda.min())) - 400.0
    pda = H.solve_ref(net, demand, roughness, solver="banded", demand_model="pda", minimum_pressure=preq - 1.0, required_pressure=preq)
    surplus = (pda.demand_delivered - demand)[:, ~net.fixed]
    leak = (p_dda.max() - preq) / 1e8
    span = dda.head.max(axis=1) - dda.head.min(axis=1)
    bound = 2.0 * span / demand[:, ~net.fixed].sum(axis=1) * surplus.sum(axis=1) + H.ACCURACY * span
    moved = np.abs(pda.head - dda.head).max(axis=1)
    with capsys.disabled():
        print(f"{name}: Preq {preq}  surplus up to {surplus.max():.3e} (leak bound {leak:.3e})  heads moved {moved.tolist()} / {bound.tolist()}")
    assert pda.converged.all() and (surplus >= 0).all() and (surplus <= leak * (1 + 1e-6)).all()
    assert (moved <= bound).all()


def test_a_junction_with_a_negative_demand_keeps_its_inflow():
    c = PR.case("chain3_e05")
    demand = c["demand"].copy()
    demand[:, 2] = -0.003                                   # an inflow at the middle junction
    ref = H.solve_ref(c["net"], demand, c["roughness"], **PR.pdd_kw(c))
    assert ref.converged.all() and (ref.demand_delivered[:, 2] == -0.003).all()
    assert ((ref.demand_delivered[:, [1, 3]] > 0) & (ref.demand_delivered[:, [1, 3]] <= demand[:, [1, 3]])).all()
    mass, energy = H.hydraulic_residuals(c["net"], ref.head, ref.flow, demand, c["roughness"], link_state=ref.link_state,
                                         demand_delivered=ref.demand_delivered, **PR.pdd_kw(c))
    assert mass.max() <= H.ACCURACY and energy.max() <= 1e-6
    zero = demand.copy()
    zero[:, 2] = 0.0                                        # and a junction without demand is not pressure-driven either
    ref0 = H.solve_ref(c["net"], zero, c["roughness"], **PR.pdd_kw(c))
    assert ref0.converged.all() and (ref0.demand_delivered[:, 2] == 0).all() and not np.signbit(ref0.demand_delivered[:, 2]).any()


WRONG_CASES = tuple((name, kind) for name in ("chain3_e1", "net40_prv_e1", "net388") for kind in PR.WRONG
                    if not (kind == "pmin_left_out" and PR.BUILDERS[name]()["pdd"][0] == 0.0))


@pytest.mark.parametrize("name,kind", WRONG_CASES)
def test_hydraulic_residuals_catch_planted_wrong_answers(name, kind, capsys):
    """Each wrong answer is the converged solution of a wrong model, so its mass balances; held to the right law, the energy
    residual of its virtual links is metres, a million times the reference's own."""
    c, ref = PR.case(name), PR.reference(name)
    mass, energy = PR.wrong_residuals(kind, c)
    with capsys.disabled():
        print(f"{name} {kind}: mass {mass.tolist()}  energy {energy.tolist()}  (reference {ref['mass'].max():.3e}, {ref['energy'].max():.3e})")
    assert (energy > 0.5).all() and energy.min() > 1e6 * ref["energy"].max()


def test_the_synthetic_cases_have_the_three_regimes_and_are_decisive(capsys):
    """What the cases were chosen for (``reference`` asserts it too), and what the PRV case is for: the valve is ACTIVE while its
    controlled node gets part of its demand, and the emitter leaks beside a demand that is delivered in part."""
    for name in PR.SYNTHETIC:
        c, ref = PR.case(name), PR.reference(name)
        zero, part, full = PR.regimes(c, ref["dense"].demand_delivered)
        with capsys.disabled():
            print(f"{name}: iterations {ref['dense'].iterations.tolist()}  q_d <= 0 {zero.tolist()}  partial {part.tolist()}  full {full.tolist()}  "
                  f"delivered {(ref['dense'].demand_delivered.sum(axis=1) / c['demand'][:, ~c['net'].fixed].sum(axis=1)).round(3).tolist()}")
        assert ref["decisive"].all() and (zero > 0).all() and (part > 0).all() and (full > 0).all()
    c, d = PR.case("net40_prv_e1"), PR.reference("net40_prv_e1")["dense"]
    net = c["net"]
    active = d.link_state[:, net.valve_links[0]] == H.VALVE_ACTIVE
    share = d.demand_delivered[:, net.valve_node[0]] / c["demand"][:, net.valve_node[0]]
    assert active.any() and ((share > 0.5) & (share < 0.95))[active].all()
    e_share = d.demand_delivered[:, net.emitter_nodes[0]] / c["demand"][:, net.emitter_nodes[0]]
    assert (d.emitter_flow > 0).all() and ((e_share > 0.5) & (e_share < 0.99)).any()


# ---- the series ---------------------------------------------------------------------------------------------------------------------------
def test_a_series_of_one_step_is_solve_ref():
    net, demand, rough, mult, dt, kw = PR.short_series()
    ser = H.simulate_series_ref(net, demand, rough, mult[:, :1], dt, **kw)
    pdd = {k: v for k, v in kw.items() if k != "pattern_of_node"}
    one = H.solve_ref(net, demand * mult[[0, 0, 1, 0], 0], rough, **pdd)
    assert type(ser).__name__ == "HydraulicSeriesPddReference" and type(one).__name__ == "HydraulicPddReference"
    for k in ("head", "flow", "demand_delivered", "iterations", "final_dq"):
        assert getattr(ser, k)[:, 0].tobytes() == getattr(one, k).tobytes(), k
    assert ser.converged.all() and ((ser.demand_delivered[:, 0, 1:3] > 0) & (ser.demand_delivered[:, 0, 1:3] < demand[:, 1:3])).all()


@pytest.mark.parametrize("warm", (True, False))
def test_a_multiplier_of_zero_switches_a_junction_off_and_on_and_the_volume_balances(warm, capsys):
    net, demand, rough, mult, dt, kw = PR.short_series()
    ref = H.simulate_series_ref(net, demand, rough, mult, dt, warm_start=warm, **kw)
    q2 = ref.demand_delivered[:, :, 2]
    off = mult[1] == 0
    assert ref.converged.all() and (q2[:, off] == 0).all() and not np.signbit(q2[:, off]).any() and (q2[:, ~off] > 0).all()
    full = demand[:, None, :] * mult[[0, 0, 1, 0]].T[None, :, :]
    assert (ref.demand_delivered <= full).all() and (ref.demand_delivered[:, :, [0, 3]] == 0).all()
    if not warm:                                            # a cold step is the steady solve at the step's levels
        heads = np.tile(net.fixed_head, (2, 1))
        heads[:, 3] = net.elevation[3] + ref.level[:, 3, 0]
        pdd = {k: v for k, v in kw.items() if k != "pattern_of_node"}
        one = H.solve_ref(net, full[:, 3], rough, heads, **pdd)
        assert one.demand_delivered.tobytes() == ref.demand_delivered[:, 3].tobytes() and one.head.tobytes() == ref.head[:, 3].tobytes()
    bal = np.abs(H.series_volume_balance(net, ref, demand, mult, dt, pattern_of_node=kw["pattern_of_node"]))
    Demanded = type("Demanded", (), {"flow": ref.flow, "level": ref.level})
    off_by = H.series_volume_balance(net, Demanded, demand, mult, dt, pattern_of_node=kw["pattern_of_node"])
    short = dt * (full - ref.demand_delivered).sum(axis=2)
    qmax = np.abs(ref.flow).max()
    with capsys.disabled():
        print(f"short_series warm={warm}: iterations {ref.iterations.tolist()}  balance with the delivered volume {bal.max():.3e} m3, with "
              f"the demanded one {np.abs(off_by).max():.3e} m3 (undelivered up to {short.max():.3e} m3)")
    assert bal.max() <= dt * H.ACCURACY * qmax              # what the stop rule leaves open in one step
    assert np.abs(off_by - short).max() <= dt * H.ACCURACY * qmax and short.max() > 1e3 * dt * H.ACCURACY * qmax


def test_a_starved_network_drains_its_tank_more_slowly():
    net, demand, rough, mult, dt, kw = PR.short_series()
    pda = H.simulate_series_ref(net, demand, rough, mult, dt, **kw)
    dda = H.simulate_series_ref(net, demand, rough, mult, dt, pattern_of_node=kw["pattern_of_node"])
    assert pda.converged.all() and dda.converged.all() and (pda.level[:, 1:] > dda.level[:, 1:]).all()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,match", (
    (dict(demand_model="pda"), "needs required_pressure"),
    (dict(demand_model="PDA", required_pressure=20.0), "demand_model must be"),
    (dict(required_pressure=20.0), "need demand_model"),
    (dict(minimum_pressure=5.0), "need demand_model"),
    (dict(demand_model="pda", required_pressure=float("nan")), "finite"),
    (dict(demand_model="pda", required_pressure=20.0, minimum_pressure=float("inf")), "finite"),
    (dict(demand_model="pda", required_pressure=5.05, minimum_pressure=5.0), "at least 0.1"),
    (dict(demand_model="pda", required_pressure=20.0, pressure_exponent=0.0), "pressure_exponent"),
    (dict(demand_model="pda", required_pressure=20.0, pressure_exponent=-0.5), "pressure_exponent"),
    (dict(demand_model="pda", required_pressure=20.0, pressure_exponent=1e-320), "pressure_exponent"),
    (dict(demand_model="pda", required_pressure=20.0, pressure_exponent=float("nan")), "pressure_exponent"),
))
def test_bad_arguments_are_refused_by_name(kw, match):
    c = PR.case("chain_hw")
    with pytest.raises(ValueError, match=match):
        H.solve_ref(c["net"], c["demand"], c["roughness"], **kw)
    with pytest.raises(ValueError, match=match):
        H.simulate_series_ref(c["net"], c["demand"], c["roughness"], np.ones((1, 2)), 300.0, **kw)
    with pytest.raises(ValueError, match=match):
        H.pdd_arguments(kw.get("demand_model"), kw.get("minimum_pressure", 0.0), kw.get("required_pressure"),
                        kw.get("pressure_exponent", H.PRESSURE_EXPONENT))


def test_residuals_need_the_delivered_flows_and_an_elevation_that_is_not_finite_fails_the_scenario():
    c = PR.case("chain_hw")
    ref = PR.solve(c)
    with pytest.raises(ValueError, match="demand_delivered"):
        H.hydraulic_residuals(c["net"], ref.head, ref.flow, c["demand"], c["roughness"], link_state=ref.link_state, **PR.pdd_kw(c))
    bad = H.HydraulicNetwork.__new__(H.HydraulicNetwork)
    bad.__dict__.update(c["net"].__dict__)
    bad.elevation = c["net"].elevation.copy()
    bad.elevation[1] = np.inf
    out = H.solve_ref(bad, c["demand"], c["roughness"], **PR.pdd_kw(c))
    assert out.failed.all() and np.isnan(out.demand_delivered).all()


def test_the_store_parameters_drop_three_scenarios_demand_driven_and_none_pressure_driven(capsys):
    d, r, kept_dda, kept_pda, pda = PR.store_reference()
    net = PR.store_network()
    short = (pda.demand_delivered < d * (1 - 1e-6))[:, ~net.fixed]
    with capsys.disabled():
        print(f"store 388 / 430 / 3, demand {PR.STORE_DEMAND}: solve_ref keeps {int(kept_dda.sum())} of {d.shape[0]} demand-driven, "
              f"{int(kept_pda.sum())} pressure-driven (iterations up to {pda.iterations.max()}); junctions short of their demand "
              f"{int(short.sum())} in {int(short.any(axis=1).sum())} scenarios")
    assert d.shape[0] == PR.STORE_SCENARIOS and pda.converged.all()
    assert int((~kept_dda).sum()) == PR.STORE_DDA_DROPPED and kept_pda.all() and short.any()
