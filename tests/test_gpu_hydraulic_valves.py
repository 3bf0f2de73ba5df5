"""Pressure-reducing and pressure-sustaining valves on the device (k_hydraulic_network.hip, LV 0) against their host statements
(hydraulics.py): the closed forms of hydraulic_valves_refs.py; residuals, agreement with ``solve_ref`` and EQUAL iterations,
``link_state`` and ``valve_changes`` on networks with one to three valves (the references are decisive, see
hydraulic_valves_refs.py); the capped grid; with no valve the two valves launches give every bit of the links launches; a series
with a tank below a PRV, warm and cold, against ``simulate_series_ref``; bad inputs fail what gatres.h says they fail; the
generated store.  Every figure is printed before it is asserted (profiles/hydraulic_valves_margins.txt holds them)."""
import numpy as np
import pytest
import torch

import hydraulic_links_refs as LR
import hydraulic_series_refs as SR
import hydraulic_valves_refs as VR
import hydraulics_refs as HR

pytestmark = pytest.mark.gpu
H = HR.H
STEADY = ("pressure", "head", "flow", "status", "final_dq", "link_state")
SERIES = ("pressure", "head", "flow", "level", "status", "final_dq", "link_state")


def host(result, fields):
    torch.cuda.synchronize()
    return {k: getattr(result, k).cpu().numpy() for k in fields}


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def run(c, **kw):
    return host(c["net"].simulate(c["demand"], c["roughness"], valve_setting=c["setting"], **kw), STEADY + ("valve_changes",))


def equal_to_reference(name, got, ref):
    """What a decisive reference fixes: iterations, convergence, link_state and valve_changes."""
    assert got["status"][:, 1].all() and not got["status"][:, 2].any(), name
    assert np.array_equal(got["status"][:, 0], ref.iterations), (name, got["status"][:, 0], ref.iterations)
    assert np.array_equal(got["link_state"], ref.link_state), name
    assert np.array_equal(got["valve_changes"], ref.valve_changes), (name, got["valve_changes"], ref.valve_changes)


# ---- 1. closed forms --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tuple(VR.CHAINS))
def test_closed_forms_on_the_device(name, capsys):
    """device-to-exact <= EXACT_FACTOR x max(reference-to-exact, the floors of hydraulics_refs.py).  Where the valve is CLOSED
    the closed form leaves out what the valve still passes, dh / 1e8; the reference's own distance carries that leak, so the
    bound needs nothing for it."""
    c, ref, floors = VR.case(name), VR.reference(name)["dense"], VR.reference(name)["floors"]
    got = run(c)
    heads, flows = VR.chain_exact(name)
    closed = VR.CHAIN_STATE[name] == H.VALVE_CLOSED
    with capsys.disabled():
        for what, table, dev, host_ref in (("head", heads, got["head"], ref.head), ("flow", flows, got["flow"], ref.flow)):
            for i, exact in table.items():
                dev_err, ref_err = np.abs(dev[:, i] - exact).max(), np.abs(host_ref[:, i] - exact).max()
                floor = floors["energy"].max() if what == "head" else floors["flow"][:, i].max()      # (hydraulics_refs.py)
                bound = HR.bound(ref_err, floor, HR.EXACT_FACTOR)
                print(f"{name} {what}[{i}]: device-to-exact {dev_err:.3e}  reference-to-exact {ref_err:.3e}  bound {bound:.3e}")
                assert dev_err <= bound, (name, what, i)
        print(f"{name}: iterations {got['status'][:, 0].tolist()}  valve state {got['link_state'][:, 1].tolist()}  "
              f"changes {got['valve_changes'].tolist()}")
    assert (got["link_state"][:, 1] == VR.CHAIN_STATE[name]).all()
    if closed:
        assert np.abs(got["flow"][:, 1]).max() <= 100.0 / 1e8
    if name == "prv_active":
        assert (got["head"][:, 2] == 40.0).all()            # the identity row: hset in every bit
    equal_to_reference(name, got, ref)


# ---- 2. networks: residuals, agreement, and the statuses equal ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", tuple(VR.SYNTHETIC))
def test_residuals_agreement_and_statuses(name, capsys):
    """Mass and energy (an ACTIVE valve: |H_c - hset|) within PHYSICS_FACTOR x the reference's own residual, heads and flows
    within AGREEMENT_FACTOR x the dense-to-banded distance of the case (floors as in hydraulics_refs.py); iterations, link_state
    and valve_changes equal to the decisive reference's."""
    c, ref = VR.case(name), VR.reference(name)
    net = c["net"]
    got = run(c)
    mass, energy = VR.residuals(c, got["head"], got["flow"], got["link_state"])
    dh, _ = HR.distances(net, got["head"], got["flow"], ref["dense"])
    fl = ref["floors"]
    h_bound = HR.bound(ref["dh"].max(), fl["dh"], HR.AGREEMENT_FACTOR)
    qmax = np.abs(ref["dense"].flow).max(axis=1)
    dq = np.abs(got["flow"] - ref["dense"].flow) / qmax[:, None]
    q_bound = HR.bound(ref["dq"].max(), fl["flow"] / qmax[:, None], HR.AGREEMENT_FACTOR)
    states = sorted(set(got["link_state"][:, net.valve_links].ravel().tolist()))
    with capsys.disabled():
        print(f"{name}: iterations {got['status'][:, 0].tolist()} (reference {ref['dense'].iterations.tolist()})  "
              f"changes {got['valve_changes'].tolist()}  valve states {states}  "
              f"mass {mass.max():.3e} / {HR.bound(ref['mass'], fl['mass'], HR.PHYSICS_FACTOR).min():.3e}  "
              f"energy {energy.max():.3e} / {HR.bound(ref['energy'], fl['energy'], HR.PHYSICS_FACTOR).min():.3e}  "
              f"dh {dh.tolist()} / {h_bound.tolist()} (dense-to-banded {ref['dh'].tolist()})  "
              f"dq/bound {(dq / q_bound).max():.3e}  margins {ref['dense'].margin.min(axis=0).tolist()}")
    equal_to_reference(name, got, ref["dense"])
    assert (mass <= HR.bound(ref["mass"], fl["mass"], HR.PHYSICS_FACTOR)).all()
    assert (energy <= HR.bound(ref["energy"], fl["energy"], HR.PHYSICS_FACTOR)).all()
    assert (dh <= h_bound).all()
    assert (dq <= q_bound).all()


def test_all_three_statuses_occur_over_the_networks():
    seen = set()
    for name in VR.SYNTHETIC:
        c, ref = VR.case(name), VR.reference(name)["dense"]
        seen |= set(ref.link_state[:, c["net"].valve_links].ravel().tolist())
    assert seen == {H.VALVE_OPEN, H.VALVE_ACTIVE, H.VALVE_CLOSED}


# ---- 3. the capped grid -----------------------------------------------------------------------------------------------------------------
def test_a_scenario_past_the_capped_grid_has_the_bits_of_a_launch_of_its_own():
    c = VR.case("prv_active")
    net, S = c["net"], HR.ABOVE_CAP
    demand = np.zeros((S, 4))
    demand[:, 3] = np.linspace(0.005, 0.03, S)
    rough = np.full((S, 3), 100.0)
    whole = host(net.simulate(demand, rough), STEADY + ("valve_changes",))
    assert whole["status"][:, 1].all() and (whole["link_state"][:, 1] == H.VALVE_ACTIVE).all() and (whole["head"][:, 2] == 40.0).all()
    assert np.abs(whole["flow"] - demand[:, 3:4]).max() <= H.ACCURACY * 0.03      # q = the demand, to the stop rule
    for rows in (slice(0, 3), slice(S - 3, S)):
        part = host(net.simulate(demand[rows], rough[rows]), STEADY + ("valve_changes",))
        for k in part:
            assert same_bits(part[k], whole[k][rows]), k


# ---- 4. no valve: the bits of the links launches ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("net37_links", "net40_links"))
def test_without_valves_the_valves_launch_has_every_bit_of_the_links_launch(name):
    c = LR.case(name)
    kw = dict(pump_speed=c["speed"], link_closed=c["closed"])
    old = host(c["net"].simulate(c["demand"], c["roughness"], links=True, **kw), STEADY)
    new = host(c["net"].simulate(c["demand"], c["roughness"], valves=True, **kw), STEADY + ("valve_changes",))
    for k in STEADY:
        assert same_bits(old[k], new[k]), (name, k)
    assert not new["valve_changes"].any() and np.isfinite(old["head"]).all()


@pytest.mark.parametrize("name", SR.NAMES[:2])
def test_without_valves_the_series_valves_launch_has_every_bit_of_the_series_links_launch(name):
    c = SR.case(name)
    kw = dict(step_seconds=c["dt"], initial_level=c["level0"], pattern_of_node=c["pattern"], fixed_head=c["heads"])
    old = host(c["net"].simulate_series(c["demand"], c["roughness"], c["mult"], links=True, **kw), SERIES)
    new = host(c["net"].simulate_series(c["demand"], c["roughness"], c["mult"], valves=True, **kw), SERIES + ("valve_changes",))
    for k in SERIES:
        assert same_bits(old[k], new[k]), (name, k)
    assert not new["valve_changes"].any()


def test_without_valves_a_series_with_pumps_and_check_valves_has_every_bit_of_the_series_links_launch():
    c = LR.case("net40_links")
    mult = np.array([[0.8, 1.0, 1.2]])
    kw = dict(step_seconds=300.0, pump_speed=c["speed"], speed_multipliers=np.array([[1.0, 0.0, 1.1]]))
    old = host(c["net"].simulate_series(c["demand"], c["roughness"], mult, links=True, **kw), SERIES)
    new = host(c["net"].simulate_series(c["demand"], c["roughness"], mult, valves=True, **kw), SERIES + ("valve_changes",))
    for k in SERIES:
        assert same_bits(old[k], new[k]), k
    assert not new["valve_changes"].any() and (old["link_state"] != 0).any()


# ---- 5. the series: a tank below a PRV ----------------------------------------------------------------------------------------------------
def tank_below_prv():
    """reservoir 0 (60 m) -- pipe -- 1 -- PRV (40 m) -- 2 -- pipe -- 3 with the demand -- pipe -- tank 4 (bottom at 30 m, 3 m of
    water): the valve feeds the demand and fills or drains the tank as the demand follows its pattern; at the pattern's peak the
    long pipe from the reservoir loses more than 20 m and the valve is OPEN."""
    net = H.HydraulicNetwork(HR._edge_index([(0, 1), (1, 2), (2, 3), (3, 4)]), [400.0, 0.0, 100.0, 200.0], np.full(4, 0.2),
                             [0.0, 0.0, 0.0, 0.0, 30.0], [0, 4], [60.0, 33.0], tank_nodes=[4], tank_diameter=[8.0],
                             minor_loss=[0.0, 2.0, 0.0, 0.0], valve_links=[1], valve_kind="PRV", valve_setting=[40.0])
    demand = np.zeros((2, 5))
    demand[:, 3] = [0.02, 0.03]
    mult = np.array([[0.5, 1.0, 2.5, 4.0, 1.5, 0.2]])
    return net, demand, np.full((2, 4), 100.0), mult, 600.0


@pytest.mark.parametrize("warm", (True, False))
def test_series_with_a_tank_below_a_prv(warm, capsys):
    """Levels within AGREEMENT_FACTOR x the dense-to-banded distance, floored by what the stop rule leaves open: a flow is
    determined to ACCURACY x the largest flow, which moves a level by dt / A times that in every step.  Statuses, iterations and
    valve_changes equal; the volume balance within PHYSICS_FACTOR x the reference's own (floor: the same dt x flow accuracy)."""
    net, demand, rough, mult, dt = tank_below_prv()
    refs = [H.simulate_series_ref(net, demand, rough, mult, dt, solver=s, warm_start=warm) for s in ("dense", "banded")]
    for r in refs:
        assert r.converged.all() and r.margin[..., 0].min() >= VR.DECISIVE_H and r.margin[..., 1].min() >= VR.DECISIVE_Q
    dense, banded = refs
    got = host(net.simulate_series(demand, rough, mult, step_seconds=dt, warm_start=warm), SERIES + ("valve_changes",))
    qmax, T = np.abs(dense.flow).max(), mult.shape[1]
    floor = T * dt / net.tank_area[0] * H.ACCURACY * qmax
    bound = HR.bound(np.abs(dense.level - banded.level).max(), floor, HR.AGREEMENT_FACTOR)
    err = np.abs(got["level"] - dense.level).max()
    Got = type("Got", (), {"flow": got["flow"], "level": got["level"]})
    bal, bal_ref = np.abs(H.series_volume_balance(net, Got, demand, mult, dt)), np.abs(H.series_volume_balance(net, dense, demand, mult, dt))
    bal_bound = HR.bound(bal_ref.max(), dt * H.ACCURACY * qmax, HR.PHYSICS_FACTOR)
    with capsys.disabled():
        print(f"tank_below_prv warm={warm}: iterations {got['status'][..., 0].tolist()}  changes {got['valve_changes'].tolist()}  "
              f"valve states {got['link_state'][..., 1].tolist()}  level error {err:.3e} / {bound:.3e}  "
              f"volume balance {bal.max():.3e} / {bal_bound:.3e} m3 (reference {bal_ref.max():.3e})")
    assert got["status"][..., 1].all() and not got["status"][..., 2:].any()
    assert np.array_equal(got["status"][..., 0], dense.iterations) and np.array_equal(got["link_state"], dense.link_state)
    assert np.array_equal(got["valve_changes"], dense.valve_changes)
    assert err <= bound and bal.max() <= bal_bound
    assert len(set(dense.link_state[..., 1].ravel().tolist())) > 1          # (the valve does change its status along the series)


# ---- 6. bad inputs ----------------------------------------------------------------------------------------------------------------------
def test_a_setting_of_nan_fails_its_scenario_alone():
    c = VR.case("net40_v2")
    setting = c["setting"].copy()
    setting[1, 0] = np.nan
    good, bad = run(c), run(dict(c, setting=setting))
    assert bad["status"][1].tolist() == [0, 0, 1, 0] and np.isnan(bad["head"][1]).all() and np.isnan(bad["flow"][1]).all()
    assert np.isnan(bad["pressure"][1]).all() and np.isnan(bad["final_dq"][1]) and not bad["link_state"][1].any()
    assert bad["valve_changes"][1] == 0
    rest = [0, 2, 3]
    for k in good:
        assert same_bits(good[k][rest], bad[k][rest]), k


@pytest.mark.parametrize("what", ("out_of_range", "duplicate", "kind_mismatch", "negative"))
def test_bad_static_valve_arrays_fail_every_scenario_and_fault_nothing(what):
    """``duplicate`` runs on two PRVs, so that the kinds match, and turns the link that loses its valve into a throttle valve of
    kind PIPE (r = 0, m > 0: a legal link), so that nothing but the second listing of the link is wrong."""
    name = "net40_v3" if what == "duplicate" else "net40_v2"
    c = VR.BUILDERS[name]()                                 # (a network of its own: the test overwrites its uploaded arrays)
    net = c["net"]
    net._valve_args(1, (1,), None)                          # uploads the valve arrays
    net._link_args(1, (1, net.num_pipes), None, None)       # and the link arrays
    st = net.static()
    link = st["valve_link"].clone()
    if what == "out_of_range":
        link[1] = net.num_pipes
    elif what == "negative":
        link[0] = -1
    elif what == "duplicate":
        assert net.valve_kind[0] == net.valve_kind[1] == H.LINK_PRV and net.minor[net.valve_links[1]] > 0
        kind = st["link_kind"].clone()
        kind[int(net.valve_links[1])] = H.LINK_PIPE
        st["link_kind"] = kind
        link[1] = link[0]
    else:
        st["valve_kind"] = st["valve_kind"].flip(0).contiguous()      # PRV <-> PSV
        assert net.valve_kind[0] != net.valve_kind[1]
    st["valve_link"] = link
    got = run(c)
    assert (got["status"] == [0, 0, 1, 0]).all() and np.isnan(got["head"]).all() and np.isnan(got["flow"]).all()
    assert np.isnan(got["pressure"]).all() and not got["link_state"].any() and not got["valve_changes"].any()
    good = run(VR.case(name))                               # the device is as it was
    assert good["status"][:, 1].all()


def test_a_series_that_does_not_fit_the_lds_is_refused_where_the_steady_launch_fits():
    """A path of 138 nodes with 8 doubled pipes and a PRV, given the full band: 162 740 bytes for the steady launch (past the
    64 KB a kernel gets unasked), 8 N more for the series, of 163 840."""
    N = 138
    pairs = [(i, i + 1) for i in range(N - 1)] + [(i, i + 1) for i in range(100, 108)]
    P = len(pairs)
    minor = np.zeros(P)
    minor[60] = 2.5
    net = H.HydraulicNetwork(HR._edge_index(pairs), np.full(P, 100.0), np.full(P, 0.2), np.zeros(N), [0], [80.0], minor_loss=minor,
                             valve_links=[60], valve_kind="PRV", valve_setting=[50.0])
    assert tuple(net.pipes[60]) == (60, 61)
    net.order = np.arange(N, dtype=np.int32)                # the given order with the full band, as hydraulics_refs._small does
    net.position = net.order.copy()
    net.half_bandwidth = N - 1
    assert H.valves_lds_bytes(N, P, N - 1, 0, 1) == 162740 <= H.LDS_BUDGET < H.series_valves_lds_bytes(N, P, N - 1, 0, 0, 1)
    demand = np.zeros((1, N))
    demand[0, 1:] = 2e-5
    rough = np.full((1, P), 100.0)
    got = host(net.simulate(demand, rough), STEADY + ("valve_changes",))
    ref = H.solve_ref(net, demand, rough, solver="banded")
    assert got["status"][0, 1] == 1 and got["link_state"][0, 60] == H.VALVE_ACTIVE and got["head"][0, 61] == 50.0
    assert np.array_equal(got["link_state"], ref.link_state) and np.array_equal(got["status"][:, 0], ref.iterations)
    with pytest.raises(ValueError, match="bytes of LDS"):
        net.simulate_series(demand, rough, np.ones((1, 2)), step_seconds=300.0)


# ---- 7. the generated store ---------------------------------------------------------------------------------------------------------------
def test_generated_store_with_drawn_settings(capsys):
    """64 scenarios of the 40-node case with three valves and settings drawn per scenario and valve: the host reference alone
    keeps all 64 (checked here), the device must keep at least 48; the draws are ``hydraulic_valve_draws`` bit for bit."""
    net = VR.case(VR.STORE_CASE)["net"]
    S = VR.STORE_SCENARIOS
    ranges = net.draw_ranges(VR.STORE_DEMAND, H.ROUGHNESS_RANGE)
    d, r, _, _, setting = H.hydraulic_valve_draws(VR.STORE_SEED, 0, S, *ranges, 0, net.num_valves, VR.STORE_SETTING)
    ref = H.solve_ref(net, d, r, valve_setting=setting, solver="banded")
    assert ref.converged.all()
    dev = [torch.from_numpy(a).to(net._dev()) for a in ranges]
    x = net._link_draw_setup(ranges, None, 0.0, VR.STORE_SETTING)
    drawn = net.draw_valves(S, VR.STORE_SEED, 0, dev[0], dev[1], *x, 0.0)
    assert same_bits(drawn[0].cpu().numpy(), d) and same_bits(drawn[1].cpu().numpy(), r) and same_bits(drawn[4].cpu().numpy(), setting)
    store, report = net.generate_store(S, VR.STORE_SEED, demand_range=VR.STORE_DEMAND, pressure_range=VR.STORE_PRESSURE,
                                       valve_setting_range=VR.STORE_SETTING)
    with capsys.disabled():
        print(f"store {VR.STORE_CASE}: {report}  host reference: {int(ref.converged.sum())} of {S} converged, "
              f"iterations up to {int(ref.iterations.max())}")
    assert report["drawn"] == S and report["failed"] == 0 and report["kept"] >= VR.STORE_MIN_KEPT
