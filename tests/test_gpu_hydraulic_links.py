"""Pumps, check valves, closed links and minor losses on the device (k_hydraulic_links.hip) against their host statements
(hydraulics.py): with no special link the two links launches give every bit of the pipe-only launches; flags that never engage
change nothing; the closed forms of hydraulic_links_refs.py; residuals under THE LINK LAW, agreement with ``solve_ref`` and
``link_state`` on networks with pumps and check valves; a scenario's bits do not depend on the launch; bad inputs fail what
gatres.h says they fail; the series launch against ``simulate_series_ref`` with a pump that is switched off for a step.  Every
figure is printed before it is asserted (profiles/hydraulic_links_margins.txt holds them)."""
import numpy as np
import pytest
import torch

import hydraulic_links_refs as LR
import hydraulic_series_refs as SR
import hydraulics_refs as HR

pytestmark = pytest.mark.gpu
H = HR.H
STEADY = ("pressure", "head", "flow", "status", "final_dq")
SERIES = ("pressure", "head", "flow", "level", "status", "final_dq")


def host(result, fields):
    torch.cuda.synchronize()
    return {k: getattr(result, k).cpu().numpy() for k in fields}


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def run(c, **kw):
    out = c["net"].simulate(c["demand"], c["roughness"], pump_speed=c["speed"], link_closed=c["closed"], links=True, **kw)
    return host(out, STEADY + ("link_state",))


# ---- 1. no special link: the bits of the pipe-only launches ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", HR.NAMES)
def test_without_special_links_the_links_launch_has_every_bit_of_the_pipe_launch(name):
    net, demand, roughness, heads = HR.case(name)
    assert not net.has_links
    old = host(net.simulate(demand, roughness, heads), STEADY)
    if H.links_lds_bytes(net.num_nodes, net.num_pipes, net.half_bandwidth, 0) > H.LDS_BUDGET:
        # path139_full_s3 fills the LDS to 908 bytes: the 12 P bytes of the link arrays do not fit beside it, and the call says so
        assert name == "path139_full_s3"
        with pytest.raises(RuntimeError, match="BADARG"):
            net.simulate(demand, roughness, heads, links=True)
        return
    new = host(net.simulate(demand, roughness, heads, links=True), STEADY + ("link_state",))
    for k in STEADY:
        assert same_bits(old[k], new[k]), (name, k)
    assert not new["link_state"].any() and np.isfinite(old["head"]).all()


@pytest.mark.parametrize("name", SR.NAMES)
def test_without_special_links_the_series_links_launch_has_every_bit_of_the_series_launch(name):
    c = SR.case(name)
    kw = dict(step_seconds=c["dt"], initial_level=c["level0"], pattern_of_node=c["pattern"], fixed_head=c["heads"])
    old = host(c["net"].simulate_series(c["demand"], c["roughness"], c["mult"], **kw), SERIES)
    new = host(c["net"].simulate_series(c["demand"], c["roughness"], c["mult"], links=True, **kw), SERIES + ("link_state",))
    for k in SERIES:
        assert same_bits(old[k], new[k]), (name, k)
    assert not new["link_state"].any()


def test_flags_that_never_engage_change_no_bit():
    """Check valves that point downhill (along the only flow there can be) on every second pipe of path12_s3, and no pump."""
    net, demand, roughness, heads = HR.case("path12_s3")
    cv = H.HydraulicNetwork(net.edge_index, net.length, net.diameter, net.elevation, net.fixed_nodes, [80.0],
                            check_valve=np.arange(net.num_pipes) % 2 == 0)
    assert cv.has_links and np.array_equal(cv.pipes, net.pipes)
    old, new = host(net.simulate(demand, roughness), STEADY), host(cv.simulate(demand, roughness), STEADY + ("link_state",))
    for k in STEADY:
        assert same_bits(old[k], new[k]), k
    assert not new["link_state"].any()


# ---- 2. closed forms ------------------------------------------------------------------------------------------------------------------
def exact_check(what, got, ref, exact, scale, log):
    """device-to-exact <= EXACT_FACTOR x max(reference-to-exact, 64 ulp of the scale)."""
    dev_err, ref_err = np.abs(got - exact).max(), np.abs(ref - exact).max()
    bound = HR.bound(ref_err, HR.FLOOR_ULPS * HR.EPS * scale, HR.EXACT_FACTOR)
    log(f"{what}: device-to-exact {dev_err:.3e}  reference-to-exact {ref_err:.3e}  bound {bound:.3e}")
    assert dev_err <= bound, what


def test_closed_forms_on_the_device(capsys):
    with capsys.disabled():
        log = print
        for n, c in LR.pump_two().items():
            got, ref = run(c), LR.solve(c)
            exact_check(f"pump_two n={n} head", got["head"][:, 1], ref.head[:, 1], LR.pump_two_exact(c), 100.0, log)
            assert got["status"][:, 1].all() and not got["link_state"].any()
        c = LR.pump_shut()
        got, ref, exact = run(c), LR.solve(c), LR.pump_shut_exact(c)
        for s in range(4):                          # a flow's scale: 64 ulp of the heads (80 m) over the link's gradient
            g = 1e8 if s < 3 else 2.0 * 2000.0 * exact[s]
            for p in range(2):
                exact_check(f"pump_shut w={c['speed'][s, 0]} q{p}", got["flow"][s, p], ref.flow[s, p], exact[s], 80.0 / g, log)
        assert np.array_equal(got["link_state"], ref.link_state) and got["link_state"][:, 0].tolist() == [1, 1, 1, 0]
        c = LR.cv_reverse()
        got, ref = run(c), LR.solve(c)
        exact_check("cv_reverse q", got["flow"][:, 1], ref.flow[:, 1], -(70.0 - ref.head[:, 1]) / 1e8, 70.0 / 1e8, log)
        exact_check("cv_reverse feed", got["flow"][:, 0], ref.flow[:, 0], c["demand"][:, 1] + ref.flow[:, 1], c["demand"].max(), log)
        assert (got["link_state"] == [0, 1]).all()
        c = LR.closed_loop()
        got, ref = run(c), LR.solve(c)
        th, tq = H.tree_solution(c["tree"], c["demand"], c["roughness"][:, :2])
        exact_check("closed_loop head", got["head"], ref.head, th, 60.0, log)
        assert (got["link_state"] == [0, 0, 2]).all() and np.abs(got["flow"][:, 2]).max() <= 60.0 / 1e8
        for k, c in LR.minor_and_tcv().items():
            got, ref = run(c), LR.solve(c)
            exact_check(f"{k} head", got["head"][:, 1], ref.head[:, 1], LR.single_link_exact(c), 45.0, log)


# ---- 3. residuals, agreement and link_state ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LR.NAMES)
def test_residuals_agreement_and_link_state(name, capsys):
    """Mass and energy under the link law within PHYSICS_FACTOR x the reference's own residual, heads and flows within
    AGREEMENT_FACTOR x the dense-to-banded distance of the CASE (its largest scenario, as test_gpu_hydraulics.py takes it: the
    two host solvers differ from one another by an amount that changes fivefold between the scenarios of one network, so one
    scenario's own distance says little; floors as in hydraulics_refs.py), link_state equal."""
    c, ref = LR.case(name), LR.reference(name)
    net = c["net"]
    assert ref["dense"].converged.all() and ref["banded"].converged.all() and (ref["margin"] > LR.DECISIVE).all()
    got = run(c)
    mass, energy = LR.residuals(c, got["head"], got["flow"])
    dh, _ = HR.distances(net, got["head"], got["flow"], ref["dense"])
    fl = ref["floors"]
    h_bound = HR.bound(ref["dh"].max(), fl["dh"], HR.AGREEMENT_FACTOR)                                     # [S]
    qmax = np.abs(ref["dense"].flow).max(axis=1)
    dq = np.abs(got["flow"] - ref["dense"].flow) / qmax[:, None]                                           # [S, P]
    q_bound = HR.bound(ref["dq"].max(), fl["flow"] / qmax[:, None], HR.AGREEMENT_FACTOR)                   # [S, P]
    with capsys.disabled():
        print(f"{name}: iterations {got['status'][:, 0].tolist()} (reference {ref['dense'].iterations.tolist()})  "
              f"mass {mass.max():.3e} / {HR.bound(ref['mass'], fl['mass'], HR.PHYSICS_FACTOR).min():.3e}  "
              f"energy {energy.max():.3e} / {HR.bound(ref['energy'], fl['energy'], HR.PHYSICS_FACTOR).min():.3e}  "
              f"dh {dh.tolist()} / {h_bound.tolist()} (dense-to-banded {ref['dh'].tolist()})  "
              f"dq/bound {(dq / q_bound).max():.3e}  margin {ref['margin'].min():.3e} m")
    assert got["status"][:, 1].all() and not got["status"][:, 2].any()
    assert (mass <= HR.bound(ref["mass"], fl["mass"], HR.PHYSICS_FACTOR)).all()
    assert (energy <= HR.bound(ref["energy"], fl["energy"], HR.PHYSICS_FACTOR)).all()
    assert (dh <= h_bound).all()
    assert (dq <= q_bound).all()
    assert np.array_equal(got["link_state"], ref["dense"].link_state)


# ---- 4. isolation -----------------------------------------------------------------------------------------------------------------------
def _pumped_path():
    """reservoir 0 -- pump -- 1 -- ... -- 11: twelve nodes, one pump."""
    rng = np.random.RandomState(41)
    return H.HydraulicNetwork(HR._edge_index([(i, i + 1) for i in range(11)]), rng.uniform(50, 500, 11), rng.uniform(0.1, 0.3, 11),
                              rng.uniform(0, 20, 12), [0], [30.0], pump_links=[0], pump_h0=[60.0], pump_r=[500.0])


def test_a_scenario_has_the_bits_it_has_alone_past_the_grid_cap():
    net, S = _pumped_path(), HR.ABOVE_CAP
    demand, roughness = HR._draws(net, S, 42, 2e-3)
    speed = np.random.RandomState(43).choice([0.8, 1.0, 1.2], (S, 1))
    fields = STEADY + ("link_state",)
    many = host(net.simulate(demand, roughness, pump_speed=speed), fields)
    assert many["status"][:, 1].all()
    for s in (0, H.GRID_CAP - 1, H.GRID_CAP, S - 1):
        one = host(net.simulate(demand[s:s + 1], roughness[s:s + 1], pump_speed=speed[s:s + 1]), fields)
        for k in fields:
            assert same_bits(one[k][0], many[k][s]), (s, k)


# ---- 5. failure -------------------------------------------------------------------------------------------------------------------------
def test_a_bad_speed_fails_its_scenario_alone():
    net = _pumped_path()
    demand, roughness = HR._draws(net, 4, 44, 2e-3)
    good = host(net.simulate(demand, roughness), STEADY)
    for bad in (np.nan, -1.0, np.inf):
        speed = np.ones((4, 1))
        speed[2, 0] = bad
        got = host(net.simulate(demand, roughness, pump_speed=speed), STEADY + ("link_state",))
        assert got["status"][:, 2].tolist() == [0, 0, 1, 0] and np.isnan(got["head"][2]).all() and np.isnan(got["flow"][2]).all()
        for k in STEADY:
            assert same_bits(np.delete(got[k], 2, axis=0), np.delete(good[k], 2, axis=0)), (bad, k)
    closed = np.zeros((4, net.num_pipes), dtype=np.uint8)
    closed[1, 3] = 2                                # a closed byte above 1
    got = host(net.simulate(demand, roughness, link_closed=closed), STEADY)
    assert got["status"][:, 2].tolist() == [0, 1, 0, 0]


@pytest.mark.parametrize("what", ("kind", "flags", "pump_link", "pump_twice", "no_pump", "n", "rp", "h0", "minor", "r0m0"))
def test_a_bad_static_array_fails_every_scenario_and_the_call_returns(what):
    net = _pumped_path()
    demand, roughness = HR._draws(net, 3, 45, 2e-3)
    net.static()
    net._link_args(3, (3, net.num_pipes), None, None)          # (uploads the link arrays)
    st = net._static
    dev = st["minor"].device
    if what == "kind":
        st["link_kind"] = st["link_kind"].clone(); st["link_kind"][4] = 2
    elif what == "flags":
        st["link_flags"] = st["link_flags"].clone(); st["link_flags"][4] = 4
    elif what == "pump_link":
        st["pump_link"] = torch.tensor([net.num_pipes], dtype=torch.int32, device=dev)
    elif what == "pump_twice":
        net.num_pumps = 2
        for k, v in (("pump_link", [0, 0]), ("pump_h0", [60.0, 60.0]), ("pump_r", [500.0, 500.0]), ("pump_n", [2.0, 2.0]), ("speed1", [1.0, 1.0])):
            st[k] = torch.tensor(v, dtype=st[k].dtype, device=dev)
    elif what == "no_pump":
        st["link_kind"] = st["link_kind"].clone(); st["link_kind"][5] = 1
    elif what == "n":
        st["pump_n"] = torch.tensor([0.5], dtype=torch.float64, device=dev)
    elif what == "rp":
        st["pump_r"] = torch.tensor([0.0], dtype=torch.float64, device=dev)
    elif what == "h0":
        st["pump_h0"] = torch.tensor([float("nan")], dtype=torch.float64, device=dev)
    elif what == "minor":
        st["minor"] = st["minor"].clone(); st["minor"][3] = -1.0
    elif what == "r0m0":
        st["coef"] = st["coef"].clone(); st["coef"][3] = 0.0
    got = host(net.simulate(demand, roughness), STEADY + ("link_state",))
    assert got["status"][:, 2].all() and not got["status"][:, 1].any() and np.isnan(got["head"]).all() and not got["link_state"].any()


def test_a_closed_byte_that_cuts_a_junction_off_ends_within_max_iter():
    net = _pumped_path()
    demand, roughness = HR._draws(net, 2, 46, 2e-3)
    closed = np.zeros((2, net.num_pipes), dtype=np.uint8)
    closed[1, 5] = 1                                # nodes 6 .. 11 lose their source
    got = host(net.simulate(demand, roughness, link_closed=closed), STEADY + ("link_state",))
    valid = net.valid(net.simulate(demand, roughness, link_closed=closed), (0.0, 150.0)).cpu().numpy()
    assert got["status"][0, 1] == 1 and got["status"][1, 0] <= H.MAX_ITER and valid.tolist() == [1, 0]
    assert got["link_state"][1, 5] == 2


# ---- 6. the series ----------------------------------------------------------------------------------------------------------------------
def _pumped_tank():
    """reservoir 0 -- pump -- junction 1 -- pipe -- tank 2, four series of six steps; the pump is off in step 3."""
    net = H.HydraulicNetwork(HR._edge_index([(0, 1), (1, 2)]), [10.0, 300.0], [0.3, 0.25], [0.0, 5.0, 30.0], [0, 2], [10.0, 32.0],
                             tank_nodes=[2], tank_diameter=[6.0], pump_links=[0], pump_h0=[45.0], pump_r=[3000.0])
    demand, roughness = HR._draws(net, 4, 47, 1e-2)
    mult = G_patterns(6)
    smult = np.array([[1.0, 1.1, 0.9, 0.0, 1.0, 1.2]])
    speed = np.array([[1.0], [0.9], [1.1], [1.0]])
    return net, demand, roughness, mult, smult, speed


def G_patterns(T):
    return HR.G.wdn_synth.make_demand_patterns(1, T, 300.0, 48)


@pytest.mark.parametrize("warm", (True, False))
def test_series_with_a_pump_that_is_switched_off_for_a_step(warm, capsys):
    net, demand, roughness, mult, smult, speed = _pumped_tank()
    kw = dict(pump_speed=speed, speed_multipliers=smult, warm_start=warm)
    ref = {s: H.simulate_series_ref(net, demand, roughness, mult, 300.0, solver=s, **kw) for s in ("dense", "banded")}
    got = host(net.simulate_series(demand, roughness, mult, step_seconds=300.0, **kw), SERIES + ("link_state",))
    assert ref["dense"].converged.all() and not ref["dense"].limited.any()
    assert np.array_equal(got["link_state"], ref["dense"].link_state) and (got["link_state"][:, 3, 0] == 2).all()
    assert (got["link_state"][:, [0, 1, 2, 4, 5], 0] == 0).all() and got["status"][:, :, 1].all()
    assert (np.diff(got["level"][:, 3:5, 0], axis=1) < 0).all()           # pump off: the tank drains through the demand
    own_q = np.abs(ref["banded"].flow - ref["dense"].flow).max()
    own_l = np.abs(ref["banded"].level - ref["dense"].level).max()
    dq, dl = np.abs(got["flow"] - ref["dense"].flow).max(), np.abs(got["level"] - ref["dense"].level).max()
    qmax = np.abs(ref["dense"].flow).max()
    # floors: a flow is no better than the solver's accuracy times the largest flow; a level adds six such steps of dt / A
    q_bound = HR.AGREEMENT_FACTOR * max(own_q, H.ACCURACY * qmax)
    l_bound = HR.AGREEMENT_FACTOR * max(own_l, 6 * H.ACCURACY * qmax * 300.0 / net.tank_area[0])
    result = H.HydraulicSeriesReference(*[got[k] if k in got else None for k in H.HydraulicSeriesReference._fields])
    balance = np.abs(H.series_volume_balance(net, result, demand, mult, 300.0)).max()
    ref_balance = np.abs(H.series_volume_balance(net, ref["dense"], demand, mult, 300.0)).max()
    b_bound = HR.PHYSICS_FACTOR * max(ref_balance, HR.FLOOR_ULPS * HR.EPS * 300.0 * np.abs(ref["dense"].flow).sum(axis=2).max())
    with capsys.disabled():
        print(f"pumped tank warm={warm}: dq {dq:.3e} / {q_bound:.3e}  dlevel {dl:.3e} / {l_bound:.3e}  "
              f"volume balance {balance:.3e} / {b_bound:.3e} m3  iterations {got['status'][0, :, 0].tolist()}")
    assert dq <= q_bound and dl <= l_bound and balance <= b_bound


def test_a_cold_series_step_has_every_bit_of_the_steady_links_launch():
    net, demand, roughness, mult, smult, speed = _pumped_tank()
    ser = host(net.simulate_series(demand, roughness, mult, step_seconds=300.0, pump_speed=speed, speed_multipliers=smult,
                                   warm_start=False), SERIES + ("link_state",))
    for t in (0, 2, 3, 5):
        heads = np.tile(net.fixed_head, (4, 1))
        heads[:, 2] = net.elevation[2] + ser["level"][:, t, 0]
        one = host(net.simulate(demand * mult[0, t], roughness, heads, pump_speed=speed * smult[0, t]), STEADY + ("link_state",))
        for k in ("pressure", "head", "flow", "status", "final_dq", "link_state"):
            assert same_bits(one[k], np.ascontiguousarray(ser[k][:, t])), (t, k)


# ---- 7. the generated store -------------------------------------------------------------------------------------------------------------
def test_generate_store_with_drawn_pump_speeds_equals_simulate_of_the_kept_draws(pkg):
    """64 scenarios of net40_links with speeds drawn in (0.8, 1.2): at most a quarter is dropped (solve_ref alone keeps seven
    eighths: test_hydraulic_link_generation_host.py), the rows are ``simulate`` of the kept draws, the report adds up, a call
    without the link arguments takes no link draw, and one ``fit_epoch`` runs on the store."""
    net, S = LR.case("net40_links")["net"], LR.STORE_SCENARIOS
    kw = dict(demand_range=LR.STORE_DEMAND, pressure_range=LR.STORE_PRESSURE, normalize=False)
    store, report = net.generate_store(S, LR.STORE_SEED, chunk=24, pump_speed_range=LR.STORE_SPEED, **kw)
    print(f"\nstore of net40_links: {report}")
    assert report["drawn"] == S and report["kept"] >= S - S // 4 and report["kept"] == len(store)
    assert report["kept"] + report["out_of_range"] + report["not_converged"] + report["failed"] == S
    ranges = net.draw_ranges(LR.STORE_DEMAND, H.ROUGHNESS_RANGE)
    d, c, speed, closed = H.hydraulic_link_draws(LR.STORE_SEED, 0, S, *ranges, net.num_pumps, LR.STORE_SPEED, 0.0)
    assert not closed.any()
    out = net.simulate(d, c, pump_speed=speed)
    ok = net.valid(out, LR.STORE_PRESSURE).cpu().numpy().astype(bool)
    assert report["kept"] == int(ok.sum()) and report["not_converged"] == int((~out.converged.cpu().numpy()).sum())
    assert same_bits(store.data.cpu().numpy(), out.pressure.cpu().numpy()[ok][:, ~net.fixed])
    # closures: drawn per scenario and link, the rows are again simulate of the kept draws, and what is cut off is counted
    shut, rep2 = net.generate_store(S, LR.STORE_SEED, pump_speed_range=LR.STORE_SPEED, closed_probability=0.05, **kw)
    d2, c2, speed2, closed2 = H.hydraulic_link_draws(LR.STORE_SEED, 0, S, *ranges, net.num_pumps, LR.STORE_SPEED, 0.05)
    assert same_bits(d2, d) and same_bits(speed2, speed) and closed2.any()
    out2 = net.simulate(d2, c2, pump_speed=speed2, link_closed=closed2)
    ok2 = net.valid(out2, LR.STORE_PRESSURE).cpu().numpy().astype(bool)
    assert rep2["kept"] == int(ok2.sum()) > 0 and rep2["not_converged"] == int((~out2.converged.cpu().numpy()).sum())
    assert rep2["kept"] + rep2["out_of_range"] + rep2["not_converged"] + rep2["failed"] == S
    assert same_bits(shut.data.cpu().numpy(), out2.pressure.cpu().numpy()[ok2][:, ~net.fixed])
    model = pkg.GATResMeanConv(num_blocks=2, nc=8).to(store.data.device)
    normed, _ = net.generate_store(S, LR.STORE_SEED, pump_speed_range=LR.STORE_SPEED, demand_range=LR.STORE_DEMAND,
                                   pressure_range=LR.STORE_PRESSURE)
    trainer = pkg.GATResTrainer.for_store(model, normed, batch_size=16)
    loss, _ = trainer.fit_epoch(normed, batch_size=16)
    assert np.isfinite(loss)
