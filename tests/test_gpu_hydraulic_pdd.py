"""Pressure-driven demand on the device (k_hydraulic_network.hip, LV 2) against its host statements (hydraulics.py): the closed forms and
shooting roots of hydraulic_pdd_refs.py, a junction above the required and one below the minimum pressure; residuals, agreement
with ``solve_ref`` and EQUAL iterations, statuses and valve changes on three networks (N < 64; a PRV whose controlled node is
pressure-driven beside an emitter; N > 256); with ``demand_model="dda"`` every bit of the emitters launches; the capped grid; the
series -- cold steps against the steady launch, a warm series against ``simulate_series_ref`` with its levels and its volume
balance, a junction switched off and on by its multiplier, sticky failure; bad scalars fail every scenario; the LDS budget; the
generated stores and their labels.  Every figure is printed before it is asserted (profiles/hydraulic_pdd_margins.txt holds
them)."""
import gc

import numpy as np
import pytest
import torch

import hydraulic_emitters_refs as ER
import hydraulic_pdd_refs as PR
import hydraulics_refs as HR

pytestmark = pytest.mark.gpu
H, G = HR.H, HR.G
EPS = HR.EPS
STEADY = ("pressure", "head", "flow", "status", "final_dq", "link_state", "valve_changes", "emitter_flow")
SERIES = ("pressure", "head", "flow", "level", "status", "final_dq", "link_state", "valve_changes", "emitter_flow")
PDD = ("demand_delivered",)


@pytest.fixture(scope="module", autouse=True)
def own_memory_pool():
    """This module's device memory comes from a pool of its own and goes back when the module ends, with the cached cases: the
    caching allocator then hands the tests that run after it the blocks it would hand them without this module."""
    pool = torch.cuda.MemPool()
    routed = torch.cuda.use_mem_pool(pool)
    routed.__enter__()
    yield
    for cached in (PR.case, PR.reference, PR.store_network, PR.store_reference, ER.case, ER.reference, ER.store_network):
        cached.cache_clear()
    gc.collect()
    torch.cuda.synchronize()
    routed.__exit__(None, None, None)


def host(result, fields):
    torch.cuda.synchronize()
    return {k: getattr(result, k).cpu().numpy() for k in fields}


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def run(c, **kw):
    return host(c["net"].simulate(c["demand"], c["roughness"], valve_setting=c["setting"], emitter_coefficient=c["coef"],
                                  **dict(PR.pdd_kw(c), **kw)), STEADY + PDD)


# ---- 1. closed forms ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PR.CLOSED_FORMS)
def test_closed_forms_and_shooting_roots_on_the_device(name, capsys):
    """device-to-exact <= EXACT_FACTOR x max(reference-to-exact, the delivered flow's floor of hydraulic_pdd_refs.py)."""
    c, ref = PR.case(name), PR.reference(name)
    exact = PR.chain_exact(name)
    got = run(c)
    dev_err, ref_err = np.abs(got["demand_delivered"][:, 1:] - exact), np.abs(ref["dense"].demand_delivered[:, 1:] - exact)
    bound = HR.bound(ref_err, ref["floors"]["delivered"][:, 1:], HR.EXACT_FACTOR)
    with capsys.disabled():
        print(f"{name}: iterations {got['status'][:, 0].tolist()} (reference {ref['dense'].iterations.tolist()})  "
              f"q_d {got['demand_delivered'][:, 1:].tolist()}  device-to-exact {dev_err.tolist()}  reference-to-exact {ref_err.tolist()}  "
              f"bound {bound.tolist()}")
    assert got["status"][:, 1].all() and not got["status"][:, 2].any()
    assert (dev_err <= bound).all()
    dec = ref["decisive"]
    assert np.array_equal(got["status"][dec, 0], ref["dense"].iterations[dec])
    assert (got["demand_delivered"][:, 0] == 0).all() and got["emitter_flow"].shape == (c["demand"].shape[0], 0)


def test_above_the_required_pressure_and_below_the_minimum_pressure(capsys):
    """chain_full: q_d - D in [0, (p - Preq) / 1e8]; chain_above: q_d in [-|p - Pmin| / 1e8, 0] (evaluated in fp64: the update and
    these quotients round differently, four roundings in all)."""
    c = PR.case("chain_full")
    got = run(c)
    p = got["head"][:, 1] - c["net"].elevation[1]
    over = got["demand_delivered"][:, 1] - c["demand"][:, 1]
    with capsys.disabled():
        print(f"chain_full: iterations {got['status'][:, 0].tolist()}  pressure {p.tolist()}  q_d - D {over.tolist()}")
    assert got["status"][:, 1].all() and (p > c["pdd"][1]).all() and (over >= 0).all()
    assert (over <= (p - c["pdd"][1]) / 1e8 * (1 + 1e-6) + 4 * EPS * c["demand"][:, 1]).all()
    c = PR.case("chain_above")
    got = run(c)
    p, q = got["head"][:, 1] - c["net"].elevation[1], got["demand_delivered"][:, 1]
    with capsys.disabled():
        print(f"chain_above: iterations {got['status'][:, 0].tolist()}  pressure {p.tolist()}  q_d {q.tolist()}")
    assert got["status"][:, 1].all() and (p < c["pdd"][0]).all() and (q <= 0).all()
    assert (np.abs(q) <= np.abs(p - c["pdd"][0]) / 1e8 * (1.0 + 4.0 * EPS)).all()
    assert np.abs(got["flow"][:, 0]).max() <= 100.0 / 1e8


# ---- 2. networks ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tuple(PR.SYNTHETIC))
def test_residuals_agreement_and_iterations(name, capsys):
    """Mass (with the delivered flows) and energy (with the virtual links' |H - z - Pmin - h(q_d)|) within PHYSICS_FACTOR x the
    reference's own residual; heads, flows, delivered flows and emitter flows within AGREEMENT_FACTOR x the dense-to-banded
    distance of the case (floors as in hydraulics_refs.py); iterations, link_state and valve_changes EQUAL to the reference's:
    every scenario of these cases is decisive."""
    c, ref = PR.case(name), PR.reference(name)
    net, dense, fl = c["net"], ref["dense"], ref["floors"]
    got = run(c)
    mass, energy = PR.residuals(c, got["head"], got["flow"], got["link_state"], got["emitter_flow"], got["demand_delivered"])
    dh, _ = HR.distances(net, got["head"], got["flow"], dense)
    h_bound = HR.bound(ref["dh"].max(), fl["dh"], HR.AGREEMENT_FACTOR)
    qmax = np.abs(dense.flow).max(axis=1)
    dq = np.abs(got["flow"] - dense.flow) / qmax[:, None]
    q_bound = HR.bound(ref["dq"].max(), fl["flow"] / qmax[:, None], HR.AGREEMENT_FACTOR)
    dd = np.abs(got["demand_delivered"] - dense.demand_delivered) / qmax[:, None]
    d_bound = HR.bound(ref["dd"].max(), fl["delivered"] / qmax[:, None], HR.AGREEMENT_FACTOR)
    zero, part, full = PR.regimes(c, got["demand_delivered"])
    with capsys.disabled():
        print(f"{name}: iterations {got['status'][:, 0].tolist()} (reference {dense.iterations.tolist()}, decisive "
              f"{ref['decisive'].tolist()})  changes {got['valve_changes'].tolist()}  q_d <= 0 / partial / full {zero.tolist()} / "
              f"{part.tolist()} / {full.tolist()}  "
              f"mass {mass.max():.3e} / {HR.bound(ref['mass'], fl['mass'], HR.PHYSICS_FACTOR).min():.3e}  "
              f"energy {energy.max():.3e} / {HR.bound(ref['energy'], fl['energy'], HR.PHYSICS_FACTOR).min():.3e}  "
              f"dh {dh.tolist()} / {h_bound.tolist()}  dq/bound {(dq / q_bound).max():.3e}  dd/bound {(dd / d_bound).max():.3e}")
    assert got["status"][:, 1].all() and not got["status"][:, 2].any()
    assert ref["decisive"].all()
    assert np.array_equal(got["status"][:, 0], dense.iterations), (got["status"][:, 0], dense.iterations)
    assert np.array_equal(got["link_state"], dense.link_state) and np.array_equal(got["valve_changes"], dense.valve_changes)
    assert (mass <= HR.bound(ref["mass"], fl["mass"], HR.PHYSICS_FACTOR)).all()
    assert (energy <= HR.bound(ref["energy"], fl["energy"], HR.PHYSICS_FACTOR)).all()
    assert (dh <= h_bound).all() and (dq <= q_bound).all() and (dd <= d_bound).all()
    assert (zero > 0).all() and (part > 0).all() and (full > 0).all()       # the three regimes, in every scenario
    if net.num_emitters:
        de = np.abs(got["emitter_flow"] - dense.emitter_flow) / qmax[:, None]
        e_bound = HR.bound(ref["de"].max(), fl["emitter_flow"] / qmax[:, None], HR.AGREEMENT_FACTOR)
        with capsys.disabled():
            print(f"{name}: q_e {got['emitter_flow'].ravel().tolist()}  de/bound {(de / e_bound).max():.3e}  valve states "
                  f"{got['link_state'][:, net.valve_links].ravel().tolist()}")
        assert (de <= e_bound).all()


# ---- 3. bits ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ER.NAMES)
def test_demand_driven_the_pdd_launch_has_every_bit_of_the_emitters_launch(name):
    c = ER.BUILDERS[name]()                                 # (a network of its own: its arrays live in this module's pool)
    kw = dict(valve_setting=c["setting"], emitter_coefficient=c["coef"])
    old = host(c["net"].simulate(c["demand"], c["roughness"], **kw), STEADY)
    new = host(c["net"].simulate(c["demand"], c["roughness"], demand_model="dda", **kw), STEADY + PDD)
    for k in STEADY:
        assert same_bits(old[k], new[k]), (name, k)
    assert same_bits(new["demand_delivered"], np.where(c["net"].fixed[None, :], 0.0, c["demand"])) and np.isfinite(old["head"]).all()


def leaky_series():
    """The series case of test_gpu_hydraulic_emitters.py: reservoir 0 (60 m) -- 1 with a leak -- 2 with the demand and a leak --
    tank 3; the leaks of the two series begin at different steps."""
    net = H.HydraulicNetwork(HR._edge_index([(0, 1), (1, 2), (2, 3)]), [400.0, 100.0, 200.0], np.full(3, 0.2), [0.0, 0.0, 5.0, 30.0],
                             [0, 3], [60.0, 33.0], tank_nodes=[3], tank_diameter=[8.0], emitter_nodes=[2, 1])
    demand = np.zeros((2, 4))
    demand[:, 2] = [0.01, 0.015]
    kw = dict(step_seconds=600.0, emitter_coefficient=np.array([[1e-3, 0.0], [2e-3, 5e-4]]), emitter_onset=np.array([[3, 0], [2, 4]]))
    return net, demand, np.full((2, 3), 100.0), np.array([[0.8, 1.0, 1.2, 1.0, 0.9, 1.1]]), kw


@pytest.mark.parametrize("warm", (True, False))
def test_demand_driven_the_series_pdd_launch_has_every_bit_of_the_series_emitters_launch(warm):
    net, demand, rough, mult, kw = leaky_series()
    old = host(net.simulate_series(demand, rough, mult, warm_start=warm, **kw), SERIES)
    new = host(net.simulate_series(demand, rough, mult, warm_start=warm, demand_model="dda", **kw), SERIES + PDD)
    for k in SERIES:
        assert same_bits(old[k], new[k]), k
    assert (old["emitter_flow"] > 0).any() and old["status"][..., 1].all()
    assert same_bits(new["demand_delivered"], demand[:, None, :] * mult[0][None, :, None] * ~net.fixed[None, None, :])


def test_a_scenario_past_the_capped_grid_has_the_bits_of_a_launch_of_its_own():
    c = PR.case("chain3_e05")
    net, S = c["net"], HR.ABOVE_CAP
    demand = np.zeros((S, 4))
    demand[:, 1], demand[:, 2], demand[:, 3] = np.linspace(0.002, 0.02, S), np.linspace(0.01, 0.003, S), 0.006
    demand[5, 2] = demand[S - 2, 2] = 0.0                   # a junction that is not pressure-driven, below and past the cap
    rough = np.full((S, 3), 100.0)
    whole = host(net.simulate(demand, rough, **PR.pdd_kw(c)), STEADY + PDD)
    assert whole["status"][:, 1].all() and ((whole["demand_delivered"][:, 2] > 0) == (demand[:, 2] > 0)).all()
    assert not np.signbit(whole["demand_delivered"][[5, S - 2], 2]).any()
    for rows in (slice(0, 7), slice(S - 3, S)):
        part = host(net.simulate(demand[rows], rough[rows], **PR.pdd_kw(c)), STEADY + PDD)
        for k in part:
            assert same_bits(part[k], whole[k][rows]), k


# ---- 4. the series ------------------------------------------------------------------------------------------------------------------------
def test_a_cold_step_has_every_bit_of_the_steady_launch_and_a_multiplier_of_zero_switches_a_junction_off_and_on():
    net, demand, rough, mult, dt, kw = PR.short_series()
    T = mult.shape[1]
    got = host(net.simulate_series(demand, rough, mult, step_seconds=dt, warm_start=False, **kw), SERIES + PDD)
    assert got["status"][..., 1].all() and not got["status"][..., 2:].any()
    pdd = {k: v for k, v in kw.items() if k != "pattern_of_node"}
    for t in range(T):
        heads = np.tile(net.fixed_head, (2, 1))
        heads[:, 3] = net.elevation[3] + got["level"][:, t, 0]
        step = host(net.simulate(demand * mult[kw["pattern_of_node"], t], rough, fixed_head=heads, **pdd), STEADY + PDD)
        for k in STEADY + PDD:
            assert same_bits(step[k], got[k][:, t]), (t, k)
    off = mult[1] == 0
    q2 = got["demand_delivered"][:, :, 2]
    assert off.tolist() == [False, True, True, False, False, False]
    assert (q2[:, off] == 0).all() and not np.signbit(q2[:, off]).any() and (q2[:, ~off] > 0).all()
    warm = host(net.simulate_series(demand, rough, mult, step_seconds=dt, warm_start=True, **kw), SERIES + PDD)
    w2 = warm["demand_delivered"][:, :, 2]
    assert warm["status"][..., 1].all() and (w2[:, off] == 0).all() and not np.signbit(w2[:, off]).any() and (w2[:, ~off] > 0).all()
    assert (warm["status"][:, 1:, 0] <= got["status"][:, 1:, 0]).all() and (warm["status"][:, 1:, 0] < got["status"][:, 1:, 0]).any()


def test_a_warm_series_against_the_reference_and_its_volume_balance(capsys):
    """Levels and delivered flows within AGREEMENT_FACTOR x the dense-to-banded distance, floored by what the stop rule leaves
    open (a flow is determined to ACCURACY x the largest flow; it moves a level by dt / A times that in every step); iterations
    equal; the volume balance with the delivered volume within PHYSICS_FACTOR x the reference's own (floor: dt x that flow
    accuracy), and with the demanded volume off by the undelivered volume to the same bound."""
    net, demand, rough, mult, dt, kw = PR.short_series()
    dense, banded = (H.simulate_series_ref(net, demand, rough, mult, dt, solver=s, **kw) for s in ("dense", "banded"))
    assert dense.converged.all() and banded.converged.all() and np.array_equal(dense.iterations, banded.iterations)
    assert ER.stop_rule_decisive(lambda **a: H.simulate_series_ref(net, demand, rough, mult, dt, **kw, **a), dense.iterations).all()
    got = host(net.simulate_series(demand, rough, mult, step_seconds=dt, **kw), SERIES + PDD)
    qmax, T = np.abs(dense.flow).max(), mult.shape[1]
    l_floor = T * dt / net.tank_area[0] * H.ACCURACY * qmax
    l_bound = HR.bound(np.abs(dense.level - banded.level).max(), l_floor, HR.AGREEMENT_FACTOR)
    l_err = np.abs(got["level"] - dense.level).max()
    d_bound = HR.bound(np.abs(dense.demand_delivered - banded.demand_delivered).max(), H.ACCURACY * qmax, HR.AGREEMENT_FACTOR)
    d_err = np.abs(got["demand_delivered"] - dense.demand_delivered).max()
    Got = type("Got", (), {"flow": got["flow"], "level": got["level"], "demand_delivered": got["demand_delivered"]})
    pat = kw["pattern_of_node"]
    bal = np.abs(H.series_volume_balance(net, Got, demand, mult, dt, pattern_of_node=pat))
    bal_ref = np.abs(H.series_volume_balance(net, dense, demand, mult, dt, pattern_of_node=pat))
    bal_bound = HR.bound(bal_ref.max(), dt * H.ACCURACY * qmax, HR.PHYSICS_FACTOR)
    Demanded = type("Demanded", (), {"flow": got["flow"], "level": got["level"]})
    off_by = H.series_volume_balance(net, Demanded, demand, mult, dt, pattern_of_node=pat)
    short = dt * (demand[:, None, :] * mult[pat].T[None, :, :] - got["demand_delivered"]).sum(axis=2)
    with capsys.disabled():
        print(f"short_series warm: iterations {got['status'][..., 0].tolist()}  level error {l_err:.3e} / {l_bound:.3e}  delivered flow "
              f"error {d_err:.3e} / {d_bound:.3e}  volume balance {bal.max():.3e} / {bal_bound:.3e} m3 (reference {bal_ref.max():.3e})  "
              f"undelivered up to {short.max():.3e} m3, balance with the demanded volume {np.abs(off_by).max():.3e} m3")
    assert got["status"][..., 1].all() and not got["status"][..., 2:].any()
    assert np.array_equal(got["status"][..., 0], dense.iterations)
    assert l_err <= l_bound and d_err <= d_bound and bal.max() <= bal_bound
    assert np.abs(off_by - short).max() <= bal_bound and short.max() > 1e3 * bal_bound


def test_failure_is_sticky_in_a_series_with_pressure_driven_demand():
    net, demand, rough, mult, dt, kw = PR.short_series()
    good = host(net.simulate_series(demand, rough, mult, step_seconds=dt, **kw), SERIES + PDD)
    bad_mult = np.tile(mult, (2, 1, 1))
    bad_mult[1, 0, 3] = np.nan                              # series 1 fails at step 3 and stays failed
    bad = host(net.simulate_series(demand, rough, bad_mult, step_seconds=dt, **kw), SERIES + PDD)
    assert bad["status"][1, 3:, 2].all() and not bad["status"][1, :3, 2].any() and not bad["status"][0, :, 2].any()
    assert np.isnan(bad["demand_delivered"][1, 3:]).all() and np.isnan(bad["head"][1, 3:]).all() and np.isnan(bad["level"][1, 4:]).all()
    for k in SERIES + PDD:
        assert same_bits(bad[k][0], good[k][0]), k
        upto = 4 if k == "level" else 3
        assert same_bits(bad[k][1, :upto], good[k][1, :upto]), k


# ---- 5. bad inputs ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scalars", ((float("nan"), 20.0, 0.5), (0.0, float("nan"), 0.5), (float("inf"), 20.0, 0.5),
                                     (0.0, float("inf"), 0.5), (-float("inf"), 20.0, 0.5), (5.0, 5.05, 0.5), (5.0, 4.0, 0.5),
                                     (0.0, 20.0, float("nan")), (0.0, 20.0, float("inf")), (0.0, 20.0, 0.0), (0.0, 20.0, -0.5),
                                     (0.0, 20.0, 1e-320)))
def test_bad_scalars_fail_every_scenario_and_fault_nothing(scalars, monkeypatch):
    """Python refuses these with ``ValueError`` (test_hydraulic_pdd_host.py); handed to the launch behind its back, the kernel
    checks them before it uses them and fails every scenario."""
    c = PR.case("net37")
    good = run(c)
    monkeypatch.setattr(H, "pdd_arguments", lambda *a: (1,) + scalars)
    got = run(c)
    assert (got["status"] == [0, 0, 1, 0]).all() and np.isnan(got["head"]).all() and np.isnan(got["flow"]).all()
    assert np.isnan(got["pressure"]).all() and np.isnan(got["demand_delivered"]).all() and not got["link_state"].any()
    net, demand, rough, mult, dt, kw = PR.short_series()
    ser = host(net.simulate_series(demand, rough, mult, step_seconds=dt, **kw), SERIES + PDD)
    assert (ser["status"] == [0, 0, 1, 0]).all() and np.isnan(ser["demand_delivered"]).all() and np.isnan(ser["level"][:, 1:]).all()
    monkeypatch.undo()
    again = run(c)                                          # the device is as it was
    for k in good:
        assert same_bits(good[k], again[k]), k


def test_python_refuses_bad_arguments_before_any_launch():
    c = PR.case("net37")
    for kw, match in ((dict(demand_model="pda"), "needs required_pressure"), (dict(required_pressure=20.0), "need demand_model"),
                      (dict(demand_model="pda", required_pressure=0.05), "at least 0.1"),
                      (dict(demand_model="pda", required_pressure=20.0, pressure_exponent=0.0), "pressure_exponent"),
                      (dict(demand_model="pressure", required_pressure=20.0), "demand_model must be")):
        with pytest.raises(ValueError, match=match):
            c["net"].simulate(c["demand"], c["roughness"], **kw)
        with pytest.raises(ValueError, match=match):
            c["net"].simulate_series(c["demand"], c["roughness"], np.ones((1, 2)), step_seconds=300.0, **kw)
        with pytest.raises(ValueError, match=match):
            c["net"].generate_store(4, 1, **kw)
    assert type(c["net"].simulate(c["demand"], c["roughness"])).__name__ == "HydraulicResult"      # the launch it always took


def test_a_shape_above_the_lds_budget_is_refused_before_any_launch(monkeypatch):
    """A path of 138 nodes with 8 doubled pipes, given the full band: 162 716 bytes demand-driven (past the 64 KB a kernel gets
    unasked), 4 416 more with pressure-driven demand, of 163 840: demand-driven it runs, pressure-driven it is refused -- by
    Python's sum with ``ValueError``, and by the launch itself with GATRES_E_BADARG where that sum is put out of the way."""
    N = 138
    pairs = [(i, i + 1) for i in range(N - 1)] + [(i, i + 1) for i in range(100, 108)]
    P = len(pairs)
    net = H.HydraulicNetwork(HR._edge_index(pairs), np.full(P, 100.0), np.full(P, 0.2), np.zeros(N), [0], [80.0])
    net.order = np.arange(N, dtype=np.int32)                # the given order with the full band, as hydraulics_refs._small does
    net.position = net.order.copy()
    net.half_bandwidth = N - 1
    assert H.pdd_lds_bytes(N, P, N - 1, 0, 0, 0, 0) == 162716 <= H.LDS_BUDGET < H.pdd_lds_bytes(N, P, N - 1, 0, 0, 0) == 162716 + 32 * N
    demand = np.zeros((1, N))
    demand[0, 1:] = 2e-5
    rough = np.full((1, P), 100.0)
    got = host(net.simulate(demand, rough, demand_model="dda"), STEADY + PDD)
    assert got["status"][0, 1] == 1
    with pytest.raises(ValueError, match="bytes of LDS"):
        net.simulate(demand, rough, demand_model="pda", required_pressure=20.0)
    with pytest.raises(ValueError, match="bytes of LDS"):
        net.simulate_series(demand, rough, np.ones((1, 2)), step_seconds=300.0, demand_model="pda", required_pressure=20.0)
    monkeypatch.setattr(H, "pdd_lds_bytes", lambda *a: 0)
    with pytest.raises(RuntimeError, match="GATRES_E_BADARG"):
        net.simulate(demand, rough, demand_model="pda", required_pressure=20.0)
    monkeypatch.undo()
    again = host(net.simulate(demand, rough, demand_model="dda"), STEADY + PDD)      # nothing was launched, nothing is broken
    for k in got:
        assert same_bits(got[k], again[k]), k


# ---- 6. generation --------------------------------------------------------------------------------------------------------------------------
def test_a_call_without_the_new_arguments_gives_the_store_it_always_gave_and_drops_three_scenarios(capsys):
    """``generate_store`` without the new arguments against its pass written out with the launch it always took; demand-driven,
    it drops as out_of_range the scenarios that ``solve_ref`` leaves with a negative pressure."""
    net = PR.store_network()
    S = PR.STORE_SCENARIOS
    d, r, kept_dda, _, _ = PR.store_reference()
    store, report = net.generate_store(S, PR.STORE_SEED, demand_range=PR.STORE_DEMAND, pressure_range=PR.STORE_PRESSURE)
    res = net.simulate(d, r, want_head=False, want_flow=False)
    assert type(res).__name__ == "HydraulicResult"
    ok = net.valid(res, PR.STORE_PRESSURE).cpu().numpy() != 0
    rows = res.pressure.cpu().numpy()[ok][:, net.junctions]
    want = G.SnapshotStore(torch.from_numpy(rows).to(net._dev()), net.junction_edge_index, device=net._dev())
    with capsys.disabled():
        print(f"store 388 / 430 / 3 demand-driven: {report}")
    assert same_bits(store.data.cpu().numpy(), want.data.cpu().numpy()) and store.mean == want.mean and store.std == want.std
    assert "supply" not in report and report["kept"] == int(ok.sum()) and np.array_equal(ok, kept_dda)
    assert report["out_of_range"] == PR.STORE_DDA_DROPPED and report["converged"] == S


def test_the_pressure_driven_store_keeps_what_the_reference_keeps_and_its_labels_match_a_re_simulation(capsys):
    """Every scenario that ``solve_ref`` converges and keeps pressure-driven (all 32: test_hydraulic_pdd_host.py) is kept; the
    labels are the delivered flows of a re-simulation of the kept scenarios and their full demands, bit for bit."""
    net = PR.store_network()
    S = PR.STORE_SCENARIOS
    pmin, preq, e = PR.STORE_PDD
    kw = dict(demand_model="pda", minimum_pressure=pmin, required_pressure=preq, pressure_exponent=e)
    d, r, _, kept_pda, ref = PR.store_reference()
    store, report = net.generate_store(S, PR.STORE_SEED, demand_range=PR.STORE_DEMAND, pressure_range=PR.STORE_PRESSURE, normalize=False, **kw)
    supply = {k: v.cpu().numpy() for k, v in report.pop("supply").items()}
    again = host(net.simulate(d, r, **kw), STEADY + PDD)
    ok = net.valid(net.simulate(d, r, **kw), PR.STORE_PRESSURE).cpu().numpy() != 0
    short = supply["delivered"] < supply["full"] * (1 - 1e-6)
    with capsys.disabled():
        print(f"store 388 / 430 / 3 pressure-driven: {report}  the reference keeps {int(kept_pda.sum())}  junctions short of their demand "
              f"{int(short.sum())} in {int(short.any(axis=1).sum())} scenarios  iterations {again['status'][:, 0].max()} at most "
              f"(reference {ref.iterations.max()})")
    assert report["drawn"] == S and report["failed"] == 0
    assert ok[kept_pda].all() and report["kept"] == int(ok.sum()) >= int(kept_pda.sum()) == S
    assert set(supply) == {"delivered", "full"} and supply["delivered"].shape == (report["kept"], net.num_nodes)
    assert same_bits(supply["delivered"], again["demand_delivered"][ok]) and same_bits(supply["full"], d[ok])
    assert same_bits(store.data.cpu().numpy(), np.ascontiguousarray(again["pressure"][ok][:, net.junctions]))
    assert short.any() and (supply["delivered"][:, net.fixed] == 0).all()


def test_a_pressure_driven_series_store_returns_its_labels_per_step():
    net = G.wdn_synth.make_hydraulic_network(37, 41, 1, seed=3, num_tanks=1)
    E, T = 3, 4
    mult = np.array([[1.0, 0.5, 1.3, 0.7]])
    kw = dict(step_seconds=300.0, multipliers=mult, demand_range=(1e-4, 1e-3), pressure_range=(-1e3, 1e3), allow_limited=True)
    plain, rep0 = net.generate_series_store(E, T, 5, normalize=False, **kw)
    store, rep = net.generate_series_store(E, T, 5, normalize=False, demand_model="pda", required_pressure=20.0, **kw)
    supply = {k: v.cpu().numpy() for k, v in rep.pop("supply").items()}
    assert "supply" not in rep0 and rep["kept"] == E and supply["delivered"].shape == supply["full"].shape == (E, T, net.num_nodes)
    d, _ = H.hydraulic_draws(5, 0, E, *net.draw_ranges((1e-4, 1e-3), H.ROUGHNESS_RANGE))
    assert same_bits(supply["full"], d[:, None, :] * mult[0][None, :, None])
    assert (supply["delivered"] <= supply["full"] + 130.0 / 1e8).all()      # (at most (p - Preq) / 1e8 above: no head is above 130 m)
    assert (supply["delivered"][:, 0] < supply["full"][:, 0] * 0.99).any()
