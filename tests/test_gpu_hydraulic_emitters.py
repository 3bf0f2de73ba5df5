"""Pressure-dependent emitters (leaks) on the device (k_hydraulic_network.hip, LV 1) against their host statements (hydraulics.py): the
closed forms and bisection roots of hydraulic_emitters_refs.py and a shut emitter; residuals, agreement with ``solve_ref`` and
EQUAL iterations where the reference is decisive, on networks with one to three emitters beside regulating valves; with no
emitter, or with every coefficient 0, every bit of the valves launches; the capped grid; the series -- cold steps against the
steady launch, steps before an onset against the series without emitters, a warm series against ``simulate_series_ref``, the
volume balance with and without the leaked volume, sticky failure; bad inputs fail what gatres.h says they fail; the generated
stores and their labels.  Every figure is printed before it is asserted (profiles/hydraulic_emitters_margins.txt holds them)."""
import gc

import numpy as np
import pytest
import torch

import hydraulic_emitters_refs as ER
import hydraulic_valves_refs as VR
import hydraulics_refs as HR

pytestmark = pytest.mark.gpu
H, G = HR.H, HR.G
EPS = HR.EPS
STEADY = ("pressure", "head", "flow", "status", "final_dq", "link_state")
SERIES = ("pressure", "head", "flow", "level", "status", "final_dq", "link_state")
EMIT = ("valve_changes", "emitter_flow")


@pytest.fixture(scope="module", autouse=True)
def own_memory_pool():
    """This module's device memory comes from a pool of its own and goes back when the module ends, with the cached cases: the
    caching allocator then hands the tests that run after it the blocks it would hand them without this module."""
    pool = torch.cuda.MemPool()
    routed = torch.cuda.use_mem_pool(pool)
    routed.__enter__()
    yield
    for cached in (ER.case, ER.reference, ER.store_network):
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
    return host(c["net"].simulate(c["demand"], c["roughness"], valve_setting=c["setting"], emitter_coefficient=c["coef"], **kw),
                STEADY + EMIT)


def plain_network(name):
    """The network of a synthetic case built without its emitters."""
    a = ER.SYNTHETIC[name]
    return G.wdn_synth.make_hydraulic_network(*a[:3], seed=a[4], num_prvs=a[6], num_psvs=a[7], valve_seed=a[8])


# ---- 1. closed forms ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tuple(n for n in ER.CHAINS if n != "chain_shut"))
def test_closed_forms_and_bisection_roots_on_the_device(name, capsys):
    """device-to-exact <= EXACT_FACTOR x max(reference-to-exact, the emitter's flow floor of hydraulic_emitters_refs.py)."""
    c, ref = ER.case(name), ER.reference(name)
    exact = ER.chain_exact(name)
    got = run(c)
    dev_err, ref_err = np.abs(got["emitter_flow"][:, 0] - exact), np.abs(ref["dense"].emitter_flow[:, 0] - exact)
    bound = HR.bound(ref_err, ref["floors"]["emitter_flow"][:, 0], HR.EXACT_FACTOR)
    with capsys.disabled():
        print(f"{name}: iterations {got['status'][:, 0].tolist()} (reference {ref['dense'].iterations.tolist()})  "
              f"q_e {got['emitter_flow'][:, 0].tolist()}  device-to-exact {dev_err.tolist()}  reference-to-exact {ref_err.tolist()}  "
              f"bound {bound.tolist()}")
    assert got["status"][:, 1].all() and not got["status"][:, 2].any()
    assert (dev_err <= bound).all()
    dec = ref["decisive"]
    assert np.array_equal(got["status"][dec, 0], ref["dense"].iterations[dec])
    e = int(c["net"].emitter_nodes[0])                      # the link into the emitter's junction carries the leak and the demand there
    dq = np.abs(got["flow"][:, e - 1] - (exact + c["demand"][:, e]))
    q_bound = HR.bound(np.abs(ref["dense"].flow[:, e - 1] - (exact + c["demand"][:, e])), ref["floors"]["flow"][:, e - 1], HR.EXACT_FACTOR)
    assert (dq <= q_bound).all(), (dq, q_bound)


def test_a_shut_emitter_carries_the_negative_pressure_over_1e8(capsys):
    """The junction lies above the source head: |q_e| <= |p| / 1e8 (evaluated in fp64: the update q_e = (H - z) (1 / 1e8) and this
    quotient round differently, four roundings in all)."""
    c = ER.case("chain_shut")
    got = run(c)
    p = got["head"][:, 1] - c["net"].elevation[1]
    with capsys.disabled():
        print(f"chain_shut: iterations {got['status'][:, 0].tolist()}  pressure {p.tolist()}  q_e {got['emitter_flow'][:, 0].tolist()}")
    assert got["status"][:, 1].all() and (p < 0).all() and (got["emitter_flow"][:, 0] <= 0).all()
    assert (np.abs(got["emitter_flow"][:, 0]) <= np.abs(p) / 1e8 * (1.0 + 4.0 * EPS)).all()
    assert np.abs(got["flow"][:, 0]).max() <= 100.0 / 1e8


# ---- 2. networks ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tuple(ER.SYNTHETIC))
def test_residuals_agreement_and_iterations(name, capsys):
    """Mass (with q_e) and energy (with the emitters' |H - z - h(q_e)|) within PHYSICS_FACTOR x the reference's own residual;
    heads, flows and emitter flows within AGREEMENT_FACTOR x the dense-to-banded distance of the case (floors as in
    hydraulics_refs.py); iterations, link_state and valve_changes equal to the reference's where it is decisive."""
    c, ref = ER.case(name), ER.reference(name)
    net, dense, fl = c["net"], ref["dense"], ref["floors"]
    got = run(c)
    mass, energy = ER.residuals(c, got["head"], got["flow"], got["link_state"], got["emitter_flow"])
    dh, _ = HR.distances(net, got["head"], got["flow"], dense)
    h_bound = HR.bound(ref["dh"].max(), fl["dh"], HR.AGREEMENT_FACTOR)
    qmax = np.abs(dense.flow).max(axis=1)
    dq = np.abs(got["flow"] - dense.flow) / qmax[:, None]
    q_bound = HR.bound(ref["dq"].max(), fl["flow"] / qmax[:, None], HR.AGREEMENT_FACTOR)
    de = np.abs(got["emitter_flow"] - dense.emitter_flow) / qmax[:, None]
    e_bound = HR.bound(ref["de"].max(), fl["emitter_flow"] / qmax[:, None], HR.AGREEMENT_FACTOR)
    with capsys.disabled():
        print(f"{name}: iterations {got['status'][:, 0].tolist()} (reference {dense.iterations.tolist()}, decisive "
              f"{ref['decisive'].tolist()})  changes {got['valve_changes'].tolist()}  q_e {got['emitter_flow'].ravel().tolist()}  "
              f"mass {mass.max():.3e} / {HR.bound(ref['mass'], fl['mass'], HR.PHYSICS_FACTOR).min():.3e}  "
              f"energy {energy.max():.3e} / {HR.bound(ref['energy'], fl['energy'], HR.PHYSICS_FACTOR).min():.3e}  "
              f"dh {dh.tolist()} / {h_bound.tolist()}  dq/bound {(dq / q_bound).max():.3e}  de/bound {(de / e_bound).max():.3e}")
    assert got["status"][:, 1].all() and not got["status"][:, 2].any()
    dec = ref["decisive"]
    assert np.array_equal(got["status"][dec, 0], dense.iterations[dec]), (got["status"][:, 0], dense.iterations)
    assert np.array_equal(got["link_state"][dec], dense.link_state[dec]) and np.array_equal(got["valve_changes"][dec], dense.valve_changes[dec])
    assert (mass <= HR.bound(ref["mass"], fl["mass"], HR.PHYSICS_FACTOR)).all()
    assert (energy <= HR.bound(ref["energy"], fl["energy"], HR.PHYSICS_FACTOR)).all()
    assert (dh <= h_bound).all() and (dq <= q_bound).all() and (de <= e_bound).all()


def test_the_cases_converge_decisively_with_an_active_valve_beside_an_emitter():
    """What the cases were chosen for, from the host reference alone: every scenario converges (asserted when a reference is
    built), most are decisive, the three exponents occur, and a valve is ACTIVE in a scenario in which an emitter leaks."""
    beside, gammas, decisive = False, set(), []
    for name in ER.SYNTHETIC:
        c, ref = ER.case(name), ER.reference(name)
        gammas.add(c["net"].emitter_exponent)
        decisive += ref["decisive"].tolist()
        if c["net"].num_valves:
            active = (ref["dense"].link_state[:, c["net"].valve_links] == H.VALVE_ACTIVE).any(axis=1)
            beside |= bool((active & (ref["dense"].emitter_flow > 0).any(axis=1)).any())
    assert beside and gammas == {0.5, 1.0, 1.18} and np.mean(decisive) >= 0.75


# ---- 3. bits ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", VR.NAMES)
def test_without_emitters_the_emitters_launch_has_every_bit_of_the_valves_launch(name):
    c = VR.BUILDERS[name]()                                 # (a network of its own: its arrays live in this module's pool)
    kw = dict(valve_setting=c["setting"])
    old = host(c["net"].simulate(c["demand"], c["roughness"], **kw), STEADY + ("valve_changes",))
    new = host(c["net"].simulate(c["demand"], c["roughness"], emitters=True, **kw), STEADY + EMIT)
    for k in STEADY + ("valve_changes",):
        assert same_bits(old[k], new[k]), (name, k)
    assert new["emitter_flow"].shape == (c["demand"].shape[0], 0) and np.isfinite(old["head"]).all()


def tank_below_prv(**kw):
    """The series case of test_gpu_hydraulic_valves.py: reservoir 0 (60 m) -- 1 -- PRV (40 m) -- 2 -- 3 with the demand -- tank 4."""
    net = H.HydraulicNetwork(HR._edge_index([(0, 1), (1, 2), (2, 3), (3, 4)]), [400.0, 0.0, 100.0, 200.0], np.full(4, 0.2),
                             [0.0, 0.0, 0.0, 0.0, 30.0], [0, 4], [60.0, 33.0], tank_nodes=[4], tank_diameter=[8.0],
                             minor_loss=[0.0, 2.0, 0.0, 0.0], valve_links=[1], valve_kind="PRV", valve_setting=[40.0], **kw)
    demand = np.zeros((2, 5))
    demand[:, 3] = [0.02, 0.03]
    return net, demand, np.full((2, 4), 100.0), np.array([[0.5, 1.0, 2.5, 4.0, 1.5, 0.2]]), 600.0


@pytest.mark.parametrize("warm", (True, False))
def test_without_emitters_the_series_emitters_launch_has_every_bit_of_the_series_valves_launch(warm):
    net, demand, rough, mult, dt = tank_below_prv()
    old = host(net.simulate_series(demand, rough, mult, step_seconds=dt, warm_start=warm), SERIES + ("valve_changes",))
    new = host(net.simulate_series(demand, rough, mult, step_seconds=dt, warm_start=warm, emitters=True), SERIES + EMIT)
    for k in SERIES + ("valve_changes",):
        assert same_bits(old[k], new[k]), k
    assert new["emitter_flow"].shape == (2, 6, 0) and len(set(old["link_state"][..., 1].ravel().tolist())) > 1
    # and with emitters whose coefficients are all 0, and one that never begins
    leaky = tank_below_prv(emitter_nodes=[3, 1])[0]
    for kw in (dict(emitter_coefficient=np.zeros(2)), dict(emitter_coefficient=[1e-3, 1e-3], emitter_onset=[6, 7])):
        off = host(leaky.simulate_series(demand, rough, mult, step_seconds=dt, warm_start=warm, **kw), SERIES + EMIT)
        for k in SERIES + ("valve_changes",):
            assert same_bits(old[k], off[k]), (k, kw)
        assert not off["emitter_flow"].any() and not np.signbit(off["emitter_flow"]).any()


@pytest.mark.parametrize("name", tuple(ER.SYNTHETIC))
def test_all_coefficients_zero_give_every_bit_of_the_network_without_emitters(name):
    c, plain = ER.case(name), plain_network(name)
    old = host(plain.simulate(c["demand"], c["roughness"], valve_setting=c["setting"], valves=True), STEADY + ("valve_changes",))
    new = run(dict(c, coef=np.zeros_like(c["coef"])))
    for k in STEADY + ("valve_changes",):
        assert same_bits(old[k], new[k]), (name, k)
    assert new["emitter_flow"].shape == c["coef"].shape and not new["emitter_flow"].any() and not np.signbit(new["emitter_flow"]).any()
    one = c["coef"].copy()
    one[:, 1:] = 0.0                                        # one emitter on: the others stay at +0.0
    mixed = run(dict(c, coef=one))
    assert mixed["status"][:, 1].all() and not mixed["emitter_flow"][:, 1:].any() and mixed["emitter_flow"][:, 0].any()
    assert not np.signbit(mixed["emitter_flow"][:, 1:]).any()


def test_a_scenario_past_the_capped_grid_has_the_bits_of_a_launch_of_its_own():
    c = ER.case("chain3_g118")
    net, S = c["net"], HR.ABOVE_CAP
    demand = np.zeros((S, 3))
    demand[:, 1] = np.linspace(0.002, 0.008, S)
    rough = np.full((S, 2), 100.0)
    coef = np.linspace(2e-5, 3e-4, S)[::-1].copy()[:, None]
    coef[5] = coef[S - 2] = 0.0                             # an emitter that is off, below and past the cap
    whole = host(net.simulate(demand, rough, emitter_coefficient=coef), STEADY + EMIT)
    assert whole["status"][:, 1].all() and ((whole["emitter_flow"][:, 0] > 0) == (coef[:, 0] > 0)).all()
    for rows in (slice(0, 7), slice(S - 3, S)):
        part = host(net.simulate(demand[rows], rough[rows], emitter_coefficient=coef[rows]), STEADY + EMIT)
        for k in part:
            assert same_bits(part[k], whole[k][rows]), k


# ---- 4. the series ------------------------------------------------------------------------------------------------------------------------
def leaky_series():
    """reservoir 0 (60 m) -- 1 with a leak -- 2 with the demand and a leak -- tank 3 (bottom at 30 m, 3 m of water); the leaks of
    the two series begin at different steps, and one emitter of series 0 never leaks."""
    args = (HR._edge_index([(0, 1), (1, 2), (2, 3)]), [400.0, 100.0, 200.0], np.full(3, 0.2), [0.0, 0.0, 5.0, 30.0], [0, 3], [60.0, 33.0])
    kw = dict(tank_nodes=[3], tank_diameter=[8.0])
    net, plain = H.HydraulicNetwork(*args, emitter_nodes=[2, 1], **kw), H.HydraulicNetwork(*args, **kw)
    demand = np.zeros((2, 4))
    demand[:, 2] = [0.01, 0.015]
    coef = np.array([[1e-3, 0.0], [2e-3, 5e-4]])
    onset = np.array([[3, 0], [2, 4]])
    return net, plain, demand, np.full((2, 3), 100.0), np.array([[0.8, 1.0, 1.2, 1.0, 0.9, 1.1]]), 600.0, coef, onset


def test_a_cold_step_has_every_bit_of_the_steady_launch_and_steps_before_the_onset_those_of_the_series_without_emitters():
    net, plain, demand, rough, mult, dt, coef, onset = leaky_series()
    T = mult.shape[1]
    got = host(net.simulate_series(demand, rough, mult, step_seconds=dt, warm_start=False, emitter_coefficient=coef,
                                   emitter_onset=onset), SERIES + EMIT)
    old = host(plain.simulate_series(demand, rough, mult, step_seconds=dt, warm_start=False, valves=True), SERIES)
    assert got["status"][..., 1].all() and not got["status"][..., 2:].any()
    for t in range(T):
        heads = np.tile(net.fixed_head, (2, 1))
        heads[:, 3] = net.elevation[3] + got["level"][:, t, 0]
        c_t = np.where(t < onset, 0.0, coef)
        step = host(net.simulate(demand * mult[0, t], rough, fixed_head=heads, emitter_coefficient=c_t), STEADY + EMIT)
        for k in STEADY + EMIT:
            assert same_bits(step[k], got[k][:, t]), (t, k)
    first = np.where(coef > 0, onset, T).min(axis=1)
    assert first.tolist() == [3, 2]
    for s in range(2):
        for k in SERIES:
            upto = first[s] + 1 if k == "level" else first[s]
            assert same_bits(got[k][s, :upto], old[k][s, :upto]), (s, k)
        assert not same_bits(got["head"][s, first[s]], old["head"][s, first[s]])
    on = (np.arange(T)[None, :, None] >= onset[:, None, :]) & (coef[:, None, :] > 0)
    assert ((got["emitter_flow"] > 0) == on).all() and not np.signbit(got["emitter_flow"][~on]).any()


def test_a_warm_series_against_the_reference_and_its_volume_balance(capsys):
    """Levels and emitter flows within AGREEMENT_FACTOR x the dense-to-banded distance, floored by what the stop rule leaves open
    (a flow is determined to ACCURACY x the largest flow; it moves a level by dt / A times that in every step); iterations equal;
    the volume balance with the leaked volume within PHYSICS_FACTOR x the reference's own (floor: dt x that flow accuracy), and
    without it off by the leaked volume to the same bound."""
    net, plain, demand, rough, mult, dt, coef, onset = leaky_series()
    kw = dict(emitter_coefficient=coef, emitter_onset=onset)
    dense, banded = (H.simulate_series_ref(net, demand, rough, mult, dt, solver=s, **kw) for s in ("dense", "banded"))
    assert dense.converged.all() and banded.converged.all() and np.array_equal(dense.iterations, banded.iterations)
    assert ER.stop_rule_decisive(lambda **a: H.simulate_series_ref(net, demand, rough, mult, dt, **kw, **a), dense.iterations).all()
    got = host(net.simulate_series(demand, rough, mult, step_seconds=dt, **kw), SERIES + EMIT)
    qmax, T = np.abs(dense.flow).max(), mult.shape[1]
    l_floor = T * dt / net.tank_area[0] * H.ACCURACY * qmax
    l_bound = HR.bound(np.abs(dense.level - banded.level).max(), l_floor, HR.AGREEMENT_FACTOR)
    l_err = np.abs(got["level"] - dense.level).max()
    e_bound = HR.bound(np.abs(dense.emitter_flow - banded.emitter_flow).max(), H.ACCURACY * qmax, HR.AGREEMENT_FACTOR)
    e_err = np.abs(got["emitter_flow"] - dense.emitter_flow).max()
    Got = type("Got", (), {"flow": got["flow"], "level": got["level"], "emitter_flow": got["emitter_flow"]})
    bal, bal_ref = np.abs(H.series_volume_balance(net, Got, demand, mult, dt)), np.abs(H.series_volume_balance(net, dense, demand, mult, dt))
    bal_bound = HR.bound(bal_ref.max(), dt * H.ACCURACY * qmax, HR.PHYSICS_FACTOR)
    without = H.series_volume_balance(net, Got, demand, mult, dt, count_leaks=False)
    leaked = dt * got["emitter_flow"].sum(axis=2)
    with capsys.disabled():
        print(f"leaky_series warm: iterations {got['status'][..., 0].tolist()}  level error {l_err:.3e} / {l_bound:.3e}  emitter flow "
              f"error {e_err:.3e} / {e_bound:.3e}  volume balance {bal.max():.3e} / {bal_bound:.3e} m3 (reference {bal_ref.max():.3e})  "
              f"leaked up to {leaked.max():.3e} m3, balance without it {np.abs(without).max():.3e} m3")
    assert got["status"][..., 1].all() and not got["status"][..., 2:].any()
    assert np.array_equal(got["status"][..., 0], dense.iterations)
    assert l_err <= l_bound and e_err <= e_bound and bal.max() <= bal_bound
    assert np.abs(without + leaked).max() <= bal_bound and leaked.max() > 1e3 * bal_bound
    on = (np.arange(T)[None, :, None] >= onset[:, None, :]) & (coef[:, None, :] > 0)
    assert ((got["emitter_flow"] > 0) == on).all()


def test_failure_is_sticky_in_a_series_with_emitters():
    net, plain, demand, rough, mult, dt, coef, onset = leaky_series()
    kw = dict(step_seconds=dt, emitter_coefficient=coef, emitter_onset=onset)
    good = host(net.simulate_series(demand, rough, mult, **kw), SERIES + EMIT)
    bad_mult = np.tile(mult, (2, 1, 1))
    bad_mult[1, 0, 3] = np.nan                              # series 1 fails at step 3 and stays failed
    bad = host(net.simulate_series(demand, rough, bad_mult, **kw), SERIES + EMIT)
    assert bad["status"][1, 3:, 2].all() and not bad["status"][1, :3, 2].any() and not bad["status"][0, :, 2].any()
    assert np.isnan(bad["emitter_flow"][1, 3:]).all() and np.isnan(bad["head"][1, 3:]).all() and np.isnan(bad["level"][1, 4:]).all()
    for k in SERIES + EMIT:
        assert same_bits(bad[k][0], good[k][0]), k
        upto = 4 if k == "level" else 3
        assert same_bits(bad[k][1, :upto], good[k][1, :upto]), k
    worse = coef.copy()
    worse[1, 1] = -1.0                                      # (its onset is step 4: the series fails from step 0 all the same)
    neg = host(net.simulate_series(demand, rough, mult, step_seconds=dt, emitter_coefficient=worse, emitter_onset=onset), SERIES + EMIT)
    assert neg["status"][1, :, 2].all() and np.isnan(neg["emitter_flow"][1]).all() and (neg["status"][1, :, 0] == 0).all()
    for k in SERIES + EMIT:
        assert same_bits(neg[k][0], good[k][0]), k


# ---- 5. bad inputs ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", (-1e-5, float("nan"), float("inf")))
def test_a_bad_coefficient_fails_its_scenario_alone(value):
    c = ER.case("net40_e3_g118")
    coef = c["coef"].copy()
    coef[1, 2] = value
    good, bad = run(c), run(dict(c, coef=coef))
    assert bad["status"][1].tolist() == [0, 0, 1, 0] and np.isnan(bad["head"][1]).all() and np.isnan(bad["flow"][1]).all()
    assert np.isnan(bad["pressure"][1]).all() and np.isnan(bad["final_dq"][1]) and not bad["link_state"][1].any()
    assert np.isnan(bad["emitter_flow"][1]).all() and bad["valve_changes"][1] == 0
    rest = [0, 2, 3]
    for k in good:
        assert same_bits(good[k][rest], bad[k][rest]), k


@pytest.mark.parametrize("what", ("out_of_range", "negative", "duplicate", "fixed_node", "controlled_node"))
def test_bad_static_emitter_arrays_fail_every_scenario_and_fault_nothing(what):
    name = "net40_e3_g118"
    c = ER.BUILDERS[name]()                                 # (a network of its own: the test overwrites its uploaded array)
    net = c["net"]
    net._emitter_args(1, (1,), c["coef"][0])                # uploads the emitter array
    st = net.static()
    node = st["emitter_node"].clone()
    node[1] = {"out_of_range": net.num_nodes, "negative": -1, "duplicate": int(node[0]), "fixed_node": int(net.fixed_nodes[0]),
               "controlled_node": int(net.valve_node[0])}[what]
    st["emitter_node"] = node
    got = run(c)
    assert (got["status"] == [0, 0, 1, 0]).all() and np.isnan(got["head"]).all() and np.isnan(got["flow"]).all()
    assert np.isnan(got["pressure"]).all() and np.isnan(got["emitter_flow"]).all() and not got["link_state"].any()
    good = run(ER.case(name))                               # the device is as it was
    assert good["status"][:, 1].all()


@pytest.mark.parametrize("gamma", (float("nan"), float("inf"), 0.0, -0.5, 1e-320))
def test_a_bad_exponent_fails_every_scenario(gamma):
    c = ER.BUILDERS["net37_e1_g05"]()
    c["net"].emitter_exponent = gamma                       # (the constructor refuses it: set behind its back)
    got = run(c)
    assert (got["status"] == [0, 0, 1, 0]).all() and np.isnan(got["head"]).all() and np.isnan(got["emitter_flow"]).all()
    mult = np.ones((1, 2))
    ser = host(c["net"].simulate_series(c["demand"], c["roughness"], mult, step_seconds=300.0, valve_setting=c["setting"],
                                        emitter_coefficient=c["coef"]), SERIES + EMIT)
    assert (ser["status"] == [0, 0, 1, 0]).all() and np.isnan(ser["emitter_flow"]).all()


def test_a_shape_above_the_lds_budget_is_refused_before_any_launch():
    """A path of 138 nodes with 8 doubled pipes, given the full band: 162 716 bytes without emitters (past the 64 KB a kernel gets
    unasked), 48 more per emitter, of 163 840: 23 emitters fit and run, the 24th is refused -- by the constructor's sum with
    ``ValueError``, and by the launch itself with GATRES_E_BADARG where the network was widened behind the constructor's back."""
    N = 138
    pairs = [(i, i + 1) for i in range(N - 1)] + [(i, i + 1) for i in range(100, 108)]
    P = len(pairs)

    def build(Ke):
        net = H.HydraulicNetwork(HR._edge_index(pairs), np.full(P, 100.0), np.full(P, 0.2), np.zeros(N), [0], [80.0],
                                 emitter_nodes=np.arange(1, Ke + 1))
        net.order = np.arange(N, dtype=np.int32)            # the given order with the full band, as hydraulics_refs._small does
        net.position = net.order.copy()
        net.half_bandwidth = N - 1
        return net
    net = build(23)
    assert H.emitters_lds_bytes(N, P, N - 1, 0, 0, 23) == 163820 <= H.LDS_BUDGET < H.emitters_lds_bytes(N, P, N - 1, 0, 0, 24)
    demand = np.zeros((1, N))
    demand[0, 1:] = 2e-5
    rough = np.full((1, P), 100.0)
    coef = np.full(23, 1e-5)
    got = host(net.simulate(demand, rough, emitter_coefficient=coef), STEADY + EMIT)
    ref = H.solve_ref(net, demand, rough, emitter_coefficient=coef, solver="banded")
    assert got["status"][0, 1] == 1 and (got["emitter_flow"] > 0).all() and ref.converged.all()
    assert np.abs(got["emitter_flow"] - ref.emitter_flow).max() <= HR.AGREEMENT_FACTOR * H.ACCURACY * np.abs(ref.flow).max()
    with pytest.raises(ValueError, match="bytes of LDS"):
        net.simulate_series(demand, rough, np.ones((1, 2)), step_seconds=300.0, emitter_coefficient=coef)
    wide = build(23)
    wide.emitter_nodes, wide.num_emitters = np.arange(1, 25), 24
    with pytest.raises(RuntimeError, match="GATRES_E_BADARG"):
        wide.simulate(demand, rough, emitter_coefficient=np.full(24, 1e-5))
    again = host(net.simulate(demand, rough, emitter_coefficient=coef), STEADY + EMIT)      # nothing was launched, nothing is broken
    for k in got:
        assert same_bits(got[k], again[k]), k


def test_python_refuses_shapes_and_missing_coefficients():
    c = ER.case("net37_e2_g1")
    net = c["net"]
    with pytest.raises(ValueError, match="emitter_coefficient"):
        net.simulate(c["demand"], c["roughness"], valve_setting=c["setting"])
    with pytest.raises(ValueError, match="emitter_coefficient must be"):
        net.simulate(c["demand"], c["roughness"], valve_setting=c["setting"], emitter_coefficient=np.zeros((3, 2)))
    with pytest.raises(ValueError, match="emitter_onset"):
        net.simulate_series(c["demand"], c["roughness"], np.ones((1, 2)), step_seconds=300.0, valve_setting=c["setting"],
                            emitter_coefficient=c["coef"], emitter_onset=np.zeros(3, dtype=np.int64))
    with pytest.raises(ValueError, match="emitter_coefficient_range"):
        net.generate_store(4, 1)
    with pytest.raises(ValueError, match="network with emitters"):
        plain_network("net37_e2_g1").generate_store(4, 1, emitter_coefficient_range=(1e-5, 1e-4))


# ---- 6. generation --------------------------------------------------------------------------------------------------------------------------
def test_device_draws_equal_their_numpy_restatement():
    net = ER.case("net40_e3_g118")["net"]
    S, seed, first = 37, 23, 11
    ranges = net.draw_ranges((1e-4, 1e-3), H.ROUGHNESS_RANGE)
    dev = [torch.from_numpy(a).to(net._dev()) for a in ranges]
    for onset_range, vs_range, prob in (((2, 9), (20.0, 40.0), 0.5), (None, None, 1.0)):
        want = H.hydraulic_emitter_draws(seed, first, S, *ranges, 0, net.num_valves, net.num_emitters, (1e-5, 3e-4), prob, onset_range,
                                         valve_setting_range=vs_range)
        x = net._emitter_draw_setup(ranges, None, 0.0, vs_range, (1e-5, 3e-4), prob, onset_range)
        got = net.draw_emitters(S, seed, first, dev[0], dev[1], *x, 0.0, prob)
        torch.cuda.synchronize()
        for i, (g, w) in enumerate(zip(got, want)):
            assert (g is None and w is None) or same_bits(g.cpu().numpy(), w), i
        assert (want[5] > 0).any() and ((want[5] == 0).any() == (prob < 1.0))


def test_a_call_without_the_new_arguments_gives_the_store_it_always_gave():
    """``generate_store`` without the emitter arguments against its pass written out with the launches it always took."""
    net = plain_network("net40_e3_g118")
    S, seed, d_rng, p_rng, s_rng = 48, 7, (1e-4, 1e-3), (-1e3, 1e3), (20.0, 60.0)
    store, report = net.generate_store(S, seed, demand_range=d_rng, pressure_range=p_rng, valve_setting_range=s_rng)
    ranges = net.draw_ranges(d_rng, H.ROUGHNESS_RANGE)
    dev = [torch.from_numpy(a).to(net._dev()) for a in ranges]
    x = net._link_draw_setup(ranges, None, 0.0, s_rng)
    demand, rough, _, closed, setting = net.draw_valves(S, seed, 0, dev[0], dev[1], *x, 0.0)
    res = net.simulate(demand, rough, want_head=False, want_flow=False, link_closed=closed, valve_setting=setting)
    assert type(res).__name__ == "HydraulicValvesResult"
    ok = net.valid(res, p_rng).cpu().numpy() != 0
    rows = res.pressure.cpu().numpy()[ok][:, net.junctions]
    want = G.SnapshotStore(torch.from_numpy(rows).to(net._dev()), net.junction_edge_index, device=net._dev())
    assert same_bits(store.data.cpu().numpy(), want.data.cpu().numpy()) and store.mean == want.mean and store.std == want.std
    assert "leak" not in report and report["kept"] == int(ok.sum()) > 0
    pipes = G.wdn_synth.make_hydraulic_network(37, 41, 1, seed=3)
    assert type(pipes.simulate(*pipes.draw(2, 1, 0, *[torch.from_numpy(a).to(pipes._dev()) for a in pipes.draw_ranges()]))).__name__ == \
        "HydraulicResult"                                   # a network without emitters takes the launches it takes today


def test_generated_store_keeps_64_of_64_and_its_labels_match_a_re_simulation(capsys):
    """The 388-node network with three emitters, each leaking with probability 1/2: ``solve_ref`` alone converges inside the
    pressure range on all 64 drawn scenarios (test_hydraulic_emitters_host.py checks that on the CPU), so the device keeps all 64;
    the labels are the drawn coefficients and the leaked flows of a re-simulation of the kept scenarios, bit for bit."""
    net = ER.store_network()
    S = ER.STORE_SCENARIOS
    store, report = net.generate_store(S, ER.STORE_SEED, demand_range=ER.STORE_DEMAND, pressure_range=ER.STORE_PRESSURE,
                                       emitter_coefficient_range=ER.STORE_COEF, leak_probability=ER.STORE_LEAK_P, normalize=False)
    leak = {k: v.cpu().numpy() for k, v in report.pop("leak").items()}
    with capsys.disabled():
        print(f"store 388 / 430 / 3 with 3 emitters: {report}  leaking emitters {int((leak['coefficient'] > 0).sum())} of {leak['coefficient'].size}")
    assert report["drawn"] == S and report["failed"] == 0 and report["kept"] == S
    ranges = net.draw_ranges(ER.STORE_DEMAND, H.ROUGHNESS_RANGE)
    d, r, _, _, _, coef, onset = H.hydraulic_emitter_draws(ER.STORE_SEED, 0, S, *ranges, 0, 0, net.num_emitters, ER.STORE_COEF,
                                                          ER.STORE_LEAK_P)
    again = host(net.simulate(d, r, emitter_coefficient=coef), STEADY + EMIT)
    assert onset is None and set(leak) == {"coefficient", "flow"}
    assert same_bits(leak["coefficient"], coef) and same_bits(leak["flow"], again["emitter_flow"])
    assert same_bits(store.data.cpu().numpy(), np.ascontiguousarray(again["pressure"][:, net.junctions]))
    assert ((leak["flow"] > 0) == (coef > 0)).all() and (coef == 0).any() and (coef > 0).any()


def test_a_leak_series_store_goes_through_the_monitor_and_lowers_every_mean_pressure(capsys):
    """One reservoir, constant demand, one leak that begins in the middle of each series: all water comes through the
    reservoir's pipes, so the leak lowers every junction's head; each junction's mean pressure after the onset is not above
    its mean before it.  The store goes through ``monitor_store`` (calibrated on the same network without the leak)."""
    T, E, dt = 12, 4, 300.0
    tight = G.wdn_synth.make_hydraulic_network(37, 41, 1, seed=3)
    net = G.wdn_synth.make_hydraulic_network(37, 41, 1, seed=3, num_emitters=1)
    kw = dict(step_seconds=dt, multipliers=np.ones((1, T)), demand_range=(1e-4, 5e-4), pressure_range=(-1e3, 1e3))
    clean, rep0 = tight.generate_series_store(E, T, 5, **kw)
    raw, rep = net.generate_series_store(E, T, 6, normalize=False, emitter_coefficient_range=(1e-3, 3e-3), leak_onset_range=(4, 9), **kw)
    leak = {k: v.cpu().numpy() for k, v in rep.pop("leak").items()}
    assert "leak" not in rep0 and rep["kept"] == E == rep0["kept"] and set(leak) == {"coefficient", "flow", "onset"}
    assert leak["flow"].shape == (E, T, 1) and leak["onset"].dtype == np.int32 and ((4 <= leak["onset"]) & (leak["onset"] < 9)).all()
    ranges = net.draw_ranges((1e-4, 5e-4), H.ROUGHNESS_RANGE)
    want = H.hydraulic_emitter_draws(6, 0, E, *ranges, 0, 0, 1, (1e-3, 3e-3), 1.0, (4, 9))
    assert same_bits(leak["coefficient"], want[5]) and same_bits(leak["onset"], want[6])
    steps = np.arange(T)[None, :, None]
    assert ((leak["flow"] > 0) == (steps >= leak["onset"][:, None, :])).all()
    p = raw.data.cpu().numpy().astype(np.float64).reshape(E, T, -1)
    worst = -np.inf
    for s in range(E):
        t0 = int(leak["onset"][s, 0])
        before, after = p[s, :t0].mean(axis=0), p[s, t0:].mean(axis=0)
        worst = max(worst, float((after - before).max()))
        assert (after <= before).all(), (s, (after - before).max())
    test = G.SnapshotStore(raw.data, net.junction_edge_index, device=net._dev(), mean=clean.mean, std=clean.std)      # the first store's scale
    model = G.GATResMeanConv(num_blocks=2, nc=8).to(net._dev())
    est = G.PressureEstimator.for_store(model, clean, [1, 9, 20, 30], batch_size=8)
    res = est.monitor_store(test, est.calibrate_monitor(clean), series_length=T)
    torch.cuda.synchronize()
    with capsys.disabled():
        print(f"leak series store: {rep}  onsets {leak['onset'].ravel().tolist()}  the least pressure drop of a junction "
              f"{-worst:.3e} m  latched {res.latched.cpu().numpy().tolist()}")
    assert tuple(res.latched.shape)[0] == E
