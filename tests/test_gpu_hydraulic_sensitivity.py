"""Hydraulic sensitivities and leak localisation on the device (k_hydraulic_sensitivity.hip) against their host statements
(hydraulics.py): the shared outputs are those of ``simulate(links=True)`` bit for bit; ``dh_ddemand`` and ``dh_droughness`` against
``sensitivity_ref`` at the device's own returned flows, within the project's rule for device against reference; the shapes where
the kernel turns over (one sensor, a full chunk and one more, the first and the last solver row, a fixed-head sensor, duplicates,
W = 1 and the full band, a grid past its cap); a scenario's bits do not depend on the launch, on the outputs asked for or on the
chunk; the fused localisation against ``leak_scores_ref`` on the device's own matrix and residuals, ``best`` exactly the argmax of
the read-back scores; a planted leak end to end through the emitters launch; no read-back; the Python refusals.  Every figure is
printed before it is asserted (profiles/hydraulic_sensitivity_margins.txt holds them)."""
import numpy as np
import pytest
import torch

import hydraulic_sensitivity_refs as SR

pytestmark = pytest.mark.gpu
HR, LR, H = SR.HR, SR.LR, SR.H
DEV = "cuda:0"
GUARD = 32                     # elements of sentinel on either side of every output
F_SENT, I_SENT = -777.25, -777
SHARED = ("pressure", "head", "flow", "status", "final_dq", "link_state")
SENS = ("dh_ddemand", "dh_droughness")
LOC = ("residual", "leak_flow", "score", "best")
DTYPES = dict(pressure=torch.float32, status=torch.int32, link_state=torch.uint8, best=torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def up(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def raw(lib, net, demand, roughness, sensors, want=SHARED + SENS, heads=None, speed=None, closed=None, readings=None, chunk=0,
        accuracy=H.ACCURACY, max_iter=H.MAX_ITER, rc=0):
    """One launch of gatres_hydraulic_sensitivity into sentinel-filled, padded buffers, with exactly the outputs in ``want``; the
    outputs as numpy, after checking that every guard word is intact."""
    st = net.static()
    S, N, P, Kp, K = demand.shape[0], net.num_nodes, net.num_pipes, net.num_pumps, len(sensors)
    shapes = dict(pressure=(S, N), head=(S, N), flow=(S, P), status=(S, H.HYD_STATUS), final_dq=(S,), link_state=(S, P),
                  dh_ddemand=(S, K, N), dh_droughness=(S, K, P), residual=(S, K), leak_flow=(S, N), score=(S, N), best=(S,))
    dem, rough, sens = up(demand, np.float64), up(roughness, np.float64), up(sensors, np.int32)
    fh = st["fixed_head"] if heads is None else up(heads, np.float64)
    spd = st["speed1"] if speed is None else up(speed, np.float64)
    cl = None if closed is None else up(closed, np.uint8)
    rd = None if readings is None else up(readings, np.float64)
    bufs = {}
    for name in want:
        dtype = DTYPES.get(name, torch.float64)
        fill = 0xA5 if dtype == torch.uint8 else (I_SENT if dtype == torch.int32 else F_SENT)
        n = int(np.prod(shapes[name]))
        buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
        bufs[name] = (buf, buf[GUARD:GUARD + n], fill, n)
    ptr = lambda name: bufs[name][1].data_ptr() if name in bufs else None
    pumps = [t.data_ptr() if Kp else None for t in (st["pump_link"], st["pump_h0"], st["pump_r"], st["pump_n"], spd)]
    got = lib.gatres_hydraulic_sensitivity(
        st["pipe_a"].data_ptr(), st["pipe_b"].data_ptr(), st["coef"].data_ptr(), st["q_start"].data_ptr(), st["fixed"].data_ptr(),
        st["elevation"].data_ptr(), st["order"].data_ptr(), st["position"].data_ptr(), net.half_bandwidth, dem.data_ptr(),
        rough.data_ptr(), fh.data_ptr(), 0 if fh.dim() == 1 else N, S, N, P, accuracy, max_iter, ptr("pressure"), ptr("head"),
        ptr("flow"), ptr("status"), ptr("final_dq"), st["link_kind"].data_ptr(), st["link_flags"].data_ptr(), st["minor"].data_ptr(),
        *pumps[:4], Kp, pumps[4], 0 if spd.dim() == 1 else Kp, None if cl is None else cl.data_ptr(),
        0 if cl is None or cl.dim() == 1 else P, ptr("link_state"), sens.data_ptr(), K, chunk, None if rd is None else rd.data_ptr(),
        *[ptr(n) for n in SENS + LOC], None)
    assert got == rc
    torch.cuda.synchronize()
    out = {}
    for name, (buf, _, fill, n) in bufs.items():
        host = buf.cpu().numpy()
        assert (host[:GUARD] == fill).all() and (host[GUARD + n:] == fill).all(), f"{name}: guard words overwritten"
        out[name] = host[GUARD:GUARD + n].reshape(shapes[name]).copy()
    return out


def run(lib, name, K, **kw):
    net, demand, roughness, heads, speed, closed = SR.links_case(name)
    sens = kw.pop("sensors", None)
    sens = SR.sensors_of(net, K) if sens is None else np.asarray(sens, dtype=np.int32)
    return raw(lib, net, demand, roughness, sens, heads=heads, speed=speed, closed=closed, **kw), sens


def check_against_ref(name, out, sens, log):
    """``SR.compare`` on a launch's matrices at its own flows: printed, then asserted."""
    net, demand, roughness, heads, speed, closed = SR.links_case(name)
    res = SR.compare(out.get("dh_ddemand"), out.get("dh_droughness"), net, demand, roughness, sens, out["flow"], heads, speed, closed)
    for k, (fig, bound) in res.items():
        log(f"{name} K={len(sens)} {k}: device-to-reference {fig.max():.3e} per scenario {np.array2string(fig, precision=2)}  bound {bound:.3e}")
    for k, (fig, bound) in res.items():
        assert (fig <= bound).all(), (name, k)


# ---- 1. the shared outputs, and the matrices against the reference ------------------------------------------------------------------------
CASES = ("two_s3", "k5_s3", "path12_s3", "net37_s3", "net40_heads_s3", "net388_s3") + LR.NAMES


@pytest.mark.parametrize("name", CASES)
def test_shared_outputs_are_those_of_the_links_launch_and_the_matrices_agree_with_the_reference(lib, name, capsys):
    net, demand, roughness, heads, speed, closed = SR.links_case(name)
    old = net.simulate(demand, roughness, heads, pump_speed=speed, link_closed=closed, links=True)
    torch.cuda.synchronize()
    old = {k: getattr(old, k).cpu().numpy() for k in SHARED}
    out, sens = run(lib, name, 8)
    for k in SHARED:
        assert same_bits(old[k], out[k]), (name, k)
    assert not out["status"][:, 2].any() and np.isfinite(out["dh_ddemand"]).all() and np.isfinite(out["dh_droughness"]).all()
    fixed = net.fixed
    assert (out["dh_ddemand"][:, :, fixed] == 0).all() and not np.signbit(out["dh_ddemand"][:, :, fixed]).any()
    assert (out["dh_ddemand"][:, :, ~fixed] <= 0).all() and (out["dh_droughness"][:, :, net.is_pump] == 0).all()
    with capsys.disabled():
        print()
        check_against_ref(name, out, sens, print)


# ---- 2. where the kernel turns over -------------------------------------------------------------------------------------------------------
def test_one_sensor_first_and_last_row_fixed_sensor_and_duplicates(lib, capsys):
    name = "net37_s3"
    net = HR.case(name)[0]
    N = net.num_nodes
    first, last = int(net.order[0]), int(net.order[N - 1 - int(net.fixed.sum())])      # (the fixed nodes come last in solver order)
    assert not net.fixed[first] and not net.fixed[last] and net.position[first] == 0
    fixed_node = int(net.fixed_nodes[0])
    with capsys.disabled():
        print()
        one, s1 = run(lib, name, 1, sensors=[first])                         # K = 1: W * Kc below 256 work items per column
        check_against_ref(name, one, s1, print)
        many, sm = run(lib, name, 0, sensors=[first, last, fixed_node, first, int(net.order[N - 1]), last])
        check_against_ref(name, many, sm, print)
    assert net.fixed[int(net.order[N - 1])]                                  # a sensor at solver row N - 1, a fixed-head row here
    for k in SENS:
        assert same_bits(one[k][:, 0], many[k][:, 0]) and same_bits(many[k][:, 0], many[k][:, 3])     # duplicates: equal bits
        assert same_bits(many[k][:, 1], many[k][:, 5])
        for row in (2, 4):                                                   # a fixed-head sensor: a row of zeros, +0.0 in dh_ddemand
            assert (many[k][:, row] == 0).all() and not (k == "dh_ddemand" and np.signbit(many[k][:, row]).any())


def test_a_full_chunk_and_one_more(lib, capsys):
    """K = Kc and K = Kc + 1 on the network and with the Kc that ``sensitivity_chunk`` gives; the 388-node band has W * Kc above 256
    work items per column."""
    name = "net388_s3"
    net, demand, roughness, _ = HR.case(name)
    Kc = H.sensitivity_chunk(net.num_nodes, net.num_pipes, net.half_bandwidth, 0, 10 ** 6)
    assert 1 < Kc < net.junctions.size and net.half_bandwidth * Kc > 256
    sens = SR.sensors_of(net, Kc + 1)
    with capsys.disabled():
        print(f"\n{name}: W = {net.half_bandwidth}, Kc = {Kc}, LDS {H.sensitivity_lds_bytes(net.num_nodes, net.num_pipes, net.half_bandwidth, 0, Kc)} bytes")
        full, _ = run(lib, name, 0, sensors=sens[:Kc])
        more, _ = run(lib, name, 0, sensors=sens)
        check_against_ref(name, more, sens, print)
    last, _ = run(lib, name, 0, sensors=sens[Kc:])
    for k in SENS:
        assert same_bits(full[k], more[k][:, :Kc]) and same_bits(last[k], more[k][:, Kc:]), k
    for k in SHARED:
        assert same_bits(full[k], more[k])


def test_w_one_and_the_full_band(lib, capsys):
    with capsys.disabled():
        print()
        for name, W in (("two_s3", 1), ("path12_s3", 1), ("k5_s3", 4)):
            net = HR.case(name)[0]
            assert net.half_bandwidth == W
            out, sens = run(lib, name, 0, sensors=net.junctions)
            check_against_ref(name, out, sens, print)


def test_no_room_for_a_single_right_hand_side_is_refused(lib):
    net, demand, roughness, _ = HR.case("path139_full_s3")
    raw(lib, net, demand, roughness, net.junctions[:2].astype(np.int32), rc=-1)
    with pytest.raises(ValueError, match="right-hand side"):
        net.sensitivity(demand, roughness, net.junctions[:2])


def test_past_the_grid_cap_and_alone_against_in_a_batch(lib):
    name = "path12_cap"
    net, demand, roughness, _ = HR.case(name)
    S = demand.shape[0]
    assert S > H.GRID_CAP
    sens = SR.sensors_of(net, 3)
    rd = np.random.RandomState(5).uniform(40.0, 80.0, (S, 3))
    batch = raw(lib, net, demand, roughness, sens, want=SHARED + SENS + LOC, readings=rd)
    assert np.isfinite(batch["dh_ddemand"]).all() and np.isfinite(batch["score"][:, ~net.fixed]).all() and (batch["best"] >= 0).all()
    for s in (0, H.GRID_CAP - 1, H.GRID_CAP, S - 1):                          # a scenario alone: the bits it has inside the batch
        alone = raw(lib, net, demand[s:s + 1], roughness[s:s + 1], sens, want=SHARED + SENS + LOC, readings=rd[s:s + 1])
        for k in SHARED + SENS + LOC:
            assert same_bits(alone[k], batch[k][s:s + 1]), (s, k)


def test_outputs_one_at_a_time_have_the_bits_of_all_at_once(lib):
    name = "net37_links"
    net, demand, roughness, heads, speed, closed = SR.links_case(name)
    sens = SR.sensors_of(net, 5)
    rd = np.random.RandomState(6).uniform(20.0, 60.0, (demand.shape[0], 5))
    kw = dict(heads=heads, speed=speed, closed=closed)
    every = raw(lib, net, demand, roughness, sens, want=SHARED + SENS + LOC, readings=rd, **kw)
    for k in SHARED + SENS + LOC:
        one = raw(lib, net, demand, roughness, sens, want=(k,), readings=rd if k in LOC else None, **kw)
        assert list(one) == [k] and same_bits(one[k], every[k]), k
    none = raw(lib, net, demand, roughness, sens, want=("status",), **kw)   # (no matrix asked for: the links launch alone)
    assert same_bits(none["status"], every["status"])


def test_a_failed_scenario_is_nan_and_touches_no_neighbour(lib):
    name = "net37_s3"
    net, demand, roughness, _ = HR.case(name)
    sens = SR.sensors_of(net, 4)
    rd = np.random.RandomState(8).uniform(20.0, 60.0, (3, 4))
    good = raw(lib, net, demand, roughness, sens, want=SHARED + SENS + LOC, readings=rd)
    bad_demand = demand.copy()
    bad_demand[1, net.junctions[3]] = np.nan
    bad = raw(lib, net, bad_demand, roughness, sens, want=SHARED + SENS + LOC, readings=rd)
    assert bad["status"][1].tolist() == [0, 0, 1, 0] and bad["best"][1] == -1
    for k in SENS + ("residual", "leak_flow", "score"):
        assert np.isnan(bad[k][1]).all(), k
    for k in SHARED + SENS + LOC:
        assert same_bits(bad[k][[0, 2]], good[k][[0, 2]]), k
    # a sensor outside the network fails every scenario of the launch, as a bad static array does
    out = raw(lib, net, demand, roughness, np.array([int(sens[0]), net.num_nodes], dtype=np.int32), want=SHARED + SENS)
    assert (out["status"][:, 2] == 1).all() and np.isnan(out["dh_ddemand"]).all() and np.isnan(out["head"]).all()
    # out of iterations is no failure: the matrices come from the returned flows
    short = raw(lib, net, demand, roughness, sens, max_iter=3)
    assert (short["status"][:, 0] == 3).all() and not short["status"][:, 1:3].any() and np.isfinite(short["dh_ddemand"]).all()
    res = SR.compare(short["dh_ddemand"], short["dh_droughness"], net, demand, roughness, sens, short["flow"])
    assert SR.accepted(res)


# ---- 3. the fused localisation ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,K", (("net37_s3", 8), ("net40_heads_s3", 5), ("net388_s3", 30), ("net37_links", 8)))
def test_fused_localisation_equals_leak_scores_ref_on_the_devices_own_matrix(lib, name, K, capsys):
    net, demand, roughness, heads, speed, closed = SR.links_case(name)
    S = demand.shape[0]
    sens = SR.sensors_of(net, K)
    rng = np.random.RandomState(11)
    model = net.simulate(demand, roughness, heads, pump_speed=speed, link_closed=closed, links=True).head.cpu().numpy()
    rd = (model - net.elevation[None, :])[:, sens] - rng.uniform(0.0, 0.05, (S, K))           # pressures a little below the model's
    rd[0, 2] = np.nan                                                        # a missing sensor in scenario 0
    kw = dict(heads=heads, speed=speed, closed=closed, readings=rd)
    out = raw(lib, net, demand, roughness, sens, want=SHARED + SENS + LOC, **kw)
    assert np.array_equal(np.isnan(out["residual"]), np.isnan(rd))
    pressure64 = (out["head"] - net.elevation[None, :])[:, sens]
    assert same_bits(out["residual"][~np.isnan(rd)], (rd - pressure64)[~np.isnan(rd)])         # one fp64 subtraction of the fp64 pressure
    score, leak, best = H.leak_scores_ref(out["dh_ddemand"], out["residual"])
    assert np.array_equal(np.isnan(score), np.isnan(out["score"])) and np.array_equal(np.isnan(leak), np.isnan(out["leak_flow"]))
    assert np.isnan(out["score"][:, net.fixed]).all() and np.isnan(out["leak_flow"][:, net.fixed]).all()
    d_score = float(np.nanmax(np.abs(out["score"] - score)))
    with np.errstate(all="ignore"):
        d_leak = float(np.nanmax(np.abs(out["leak_flow"] - leak) / SR.leak_flow_bound(K, out["dh_ddemand"], out["residual"])))
    with capsys.disabled():
        print(f"\n{name} K={K}: score device-to-reference {d_score:.3e} (bound {SR.score_bound(K):.3e}); leak_flow, in units of its "
              f"bound {d_leak:.3e}; best {out['best'].tolist()}")
    assert d_score <= SR.score_bound(K) and d_leak <= 1.0
    assert np.array_equal(out["best"], H.best_score_ref(out["score"])) and out["best"].dtype == np.int32      # exact, on the device's bits
    # without the matrix in memory: the same bits
    lean = raw(lib, net, demand, roughness, sens, want=LOC, **kw)
    for k in LOC:
        assert same_bits(lean[k], out[k]), k
    # a NaN reading is the launch without that sensor
    keep = [k for k in range(K) if k != 2]
    less = raw(lib, net, demand[:1], roughness[:1], sens[keep], want=LOC, heads=None if heads is None else heads[:1],
               speed=None if speed is None else speed[:1], closed=closed, readings=rd[:1, keep])
    for k in ("leak_flow", "score", "best"):
        assert same_bits(less[k], out[k][:1]), k
    # chunked: the sums accumulate in the same order
    for chunk in (1, 3):
        cut = raw(lib, net, demand, roughness, sens, want=SENS + LOC, chunk=chunk, **kw)
        for k in SENS + LOC:
            assert same_bits(cut[k], out[k]), (chunk, k)


def test_localisation_without_a_score(lib):
    net, demand, roughness, _ = HR.case("net37_s3")
    sens = SR.sensors_of(net, 4)
    head = raw(lib, net, demand, roughness, sens, want=("head",))["head"]
    rd = (head - net.elevation[None, :])[:, sens]                            # the model's own pressures: a zero residual
    rd[1] = np.nan                                                           # no sensor at all
    rd[2] += 0.01
    out = raw(lib, net, demand, roughness, sens, want=LOC, readings=rd)
    assert (out["residual"][0] == 0).all() and np.isnan(out["score"][:2]).all() and out["best"].tolist()[:2] == [-1, -1]
    assert (out["leak_flow"][0, ~net.fixed] == 0).all() and np.isnan(out["leak_flow"][1]).all() and out["best"][2] >= 0
    # a planted exact tie goes to the lower index: with one sensor every column is a multiple of every other, and
    # <z, rho> / (sqrt(z z) * sqrt(rho rho)) is -1 in every bit wherever the sensor sees the node (sqrt(x * x) is |x|)
    out = raw(lib, net, demand, roughness, sens[:1], want=LOC + ("dh_ddemand",), readings=rd[:, :1] + 0.02)
    seen = out["dh_ddemand"][0, 0] != 0
    assert seen.sum() > 1 and (out["score"][0, seen] == -1.0).all() and np.isnan(out["score"][0, ~seen]).all()
    assert out["best"][0] == np.flatnonzero(seen)[0] and np.array_equal(out["best"], H.best_score_ref(out["score"]))


# ---- 4. end to end: a planted leak through the emitters launch ------------------------------------------------------------------------------
def test_a_planted_leak_is_found_within_the_recorded_deficit(lib, capsys):
    """net37_s3's network with an emitter at every junction; in scenario j only junction j leaks, its coefficient sized for
    LEAK_FRACTION of the total demand at the reference's nominal pressure.  Some junctions of net37_s3 stand above their head
    (down to -8 m of pressure), where an emitter takes nothing out; elevations enter nothing but the emitters and the pressures,
    so the copy lowers every junction by one shift that leaves the lowest nominal pressure at 10 m -- the heads, and with them
    the recorded figures of the host test, stay those of net37_s3.  Readings: the emitters launch's pressures (fp64 head -
    elevation) at 8 sensors; model: the same demand without a leak; both at the tight accuracy of the host test."""
    c = SR.leak_case("net37_s3", 8)
    base, sens = c["net"], c["sensors"]
    J = base.junctions.size
    nominal_pressure = c["nominal"].head[0, base.junctions] - base.elevation[base.junctions]
    elevation = base.elevation.copy()
    elevation[base.junctions] -= 10.0 - nominal_pressure.min()
    nominal_pressure = c["nominal"].head[0, base.junctions] - elevation[base.junctions]
    assert nominal_pressure.min() > 9.99
    net = H.HydraulicNetwork(base.edge_index, base.length, base.diameter, elevation, base.fixed_nodes,
                             base.fixed_head[base.fixed_nodes], emitter_nodes=base.junctions)
    assert np.array_equal(net.pipes, base.pipes) and np.array_equal(net.position, base.position)
    coef = np.zeros((J, J))
    coef[np.arange(J), np.arange(J)] = c["leak"] / np.sqrt(nominal_pressure)
    demand, roughness = np.array(c["demand"]), np.array(c["roughness"])
    leaking = net.simulate(demand, roughness, emitter_coefficient=coef, accuracy=SR.TIGHT)
    readings = (leaking.head - net.static()["elevation"][None, :])[:, torch.as_tensor(sens.astype(np.int64), device=DEV)]
    loc = net.localize_leaks(readings, demand, roughness, sens, accuracy=SR.TIGHT)
    torch.cuda.synchronize()
    flow = leaking.emitter_flow.cpu().numpy()[np.arange(J), np.arange(J)]
    report = H.localization_report(net, loc, base.junctions, tolerance=SR.DEFICIT_RECORDED + SR.score_bound(8))
    deficit, rel = SR.leak_figures(loc.score.cpu().numpy(), loc.leak_flow.cpu().numpy(), base.junctions, flow)
    with capsys.disabled():
        print(f"\nnet37 with emitters, 8 sensors: emitter flows {flow.min():.3e} .. {flow.max():.3e} (sized for {c['leak']:.3e}); "
              f"deficit of the true node {deficit.max():.3e} (recorded {SR.DEFICIT_RECORDED:.0e} + {SR.score_bound(8):.1e}); leak_flow "
              f"error {rel.max():.3e} (recorded {SR.LEAK_FLOW_RECORDED:.0e}); hops from best to the leak: mean "
              f"{report['hops'].mean():.2f}, max {report['hops'].max()}; candidates above the true node: {report['above'].max()}; "
              f"converged {int(leaking.converged.sum())} + {int((loc.status[:, 1] != 0).sum())} of 2 x {J}")
    assert not leaking.failed.any() and not (loc.status[:, 2] != 0).any()
    assert np.allclose(report["deficit"], deficit, rtol=0, atol=0) and (report["best"] == loc.best.cpu().numpy()).all()
    assert (deficit <= SR.DEFICIT_RECORDED + SR.score_bound(8)).all()
    assert (rel <= SR.LEAK_FLOW_RECORDED).all()
    assert report["above"].max() == 0                                       # nobody scores more than the tolerance above the leak


# ---- 5. no read-back, and the Python refusals -----------------------------------------------------------------------------------------------
def test_no_read_back_in_the_launches_and_one_in_the_report(monkeypatch):
    net, demand, roughness, _ = HR.case("net37_s3")
    sens = SR.sensors_of(net, 4)
    net.static()                                                             # (the static arrays are uploaded before the count)
    dem, rough = up(demand, np.float64), up(roughness, np.float64)
    rd = torch.full((3, 4), 30.0, dtype=torch.float64, device=DEV)
    reads = {"cpu": 0, "item": 0, "tolist": 0, "numpy": 0}
    real = {k: getattr(torch.Tensor, k) for k in reads}

    def counted(key):
        def f(self, *a, **k):
            if self.is_cuda:
                reads[key] += 1
            return real[key](self, *a, **k)
        return f

    for k in reads:
        monkeypatch.setattr(torch.Tensor, k, counted(k))
    res = net.sensitivity(dem, rough, sens, want_roughness=True)
    loc = net.localize_leaks(rd, dem, rough, sens)
    assert sum(reads.values()) == 0, reads
    report = H.localization_report(net, loc, int(net.junctions[0]))
    for k in reads:
        monkeypatch.setattr(torch.Tensor, k, real[k])
    assert reads == {"cpu": 1, "item": 0, "tolist": 0, "numpy": 0}, reads
    assert res.dh_ddemand.shape == (3, 4, net.num_nodes) and res.dh_droughness.shape == (3, 4, net.num_pipes) and res.dh_ddemand.is_cuda
    assert loc.dh_ddemand is None and loc.score.is_cuda and loc.best.dtype == torch.int32 and set(report) == {"hops", "deficit", "above", "best"}
    assert net.sensitivity(dem, rough, sens).dh_droughness is None
    full = net.localize_leaks(rd, dem, rough, sens, want_sensitivity=True)
    assert torch.equal(full.dh_ddemand, res.dh_ddemand) and same_bits(full.score.cpu().numpy(), loc.score.cpu().numpy())


def test_python_refusals():
    import hydraulic_valves_refs as VR
    valves = next(c for c in (VR.case(n) for n in VR.NAMES) if c["net"].has_valves)
    for call in (lambda n, d, r: n.sensitivity(d, r, [int(n.junctions[0])]),
                 lambda n, d, r: n.localize_leaks(np.zeros((d.shape[0], 1)), d, r, [int(n.junctions[0])])):
        with pytest.raises(ValueError, match="regulating valves"):
            call(valves["net"], valves["demand"], valves["roughness"])
    net, demand, roughness, _ = HR.case("net37_s3")
    for bad in ([], [[1, 2]], [1.5], [True]):
        with pytest.raises(ValueError, match="sensor_nodes"):
            net.sensitivity(demand, roughness, bad)
    with pytest.raises(ValueError, match="chunk"):
        net.sensitivity(demand, roughness, [1], chunk=0)
    with pytest.raises(ValueError, match="readings"):
        net.localize_leaks(None, demand, roughness, [1])
    with pytest.raises(ValueError, match="readings"):
        net.localize_leaks(np.zeros((3, 2)), demand, roughness, [1])
    with pytest.raises(TypeError):
        net.sensitivity(demand, roughness, [1], demand_model="pda")        # not offered
    # a network with emitters is accepted, its emitters taken as not leaking: the bits of the network without them
    leaky = H.HydraulicNetwork(net.edge_index, net.length, net.diameter, net.elevation, net.fixed_nodes, net.fixed_head[net.fixed_nodes],
                               emitter_nodes=net.junctions[:3])
    a, b = net.sensitivity(demand, roughness, [5, 9]), leaky.sensitivity(demand, roughness, [5, 9])
    assert torch.equal(a.dh_ddemand, b.dh_ddemand) and torch.equal(a.head, b.head)
