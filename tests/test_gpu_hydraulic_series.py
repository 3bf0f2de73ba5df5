"""The hydraulic series on the device (k_hydraulics.hip: gatres_hydraulic_series, gatres_hydraulic_series_valid) against its host
statements (hydraulics.py).  Cold start: every step equals, in every bit, ``gatres_hydraulic_solve`` on that step's inputs -- which
ties the series' Newton to the kernel that test_gpu_hydraulics.py holds to the physics.  The level update and the clamp flag equal
their numpy statement in every bit.  Warm start goes through THE CHECKER of hydraulic_series_refs.py (physics, volume balance,
agreement with ``simulate_series_ref``, iteration counts), whose bounds are formed from the reference's own error.  Isolation,
failure, guard words, the filter, ``generate_series_store`` against its pass written out, and the monitor and the trainer on a
generated series store.  Every figure is printed before it is asserted; profiles/hydraulic_series_margins.txt holds them."""
import numpy as np
import pytest
import torch

import hydraulic_series_refs as SR

pytestmark = pytest.mark.gpu
HR, H = SR.HR, SR.H
DEV = "cuda:0"
GUARD = 32                     # elements of sentinel on either side of every output
F_SENT, I_SENT = -777.25, -777
same_bits = SR.same_bits


def padded(n, dtype):
    fill = 0xA5 if dtype == torch.uint8 else (I_SENT if dtype == torch.int32 else F_SENT)
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n], fill


def unpad(buf, n, fill, what):
    host = buf.cpu().numpy()
    assert (host[:GUARD] == fill).all() and (host[GUARD + n:] == fill).all(), f"{what}: guard words overwritten"
    return host[GUARD:GUARD + n].copy()


def up(a, dtype):
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).to(DEV)          # (a copy: the references are read-only)


def raw_series(lib, c, warm=True, want_head=True, want_flow=True, max_iter=H.MAX_ITER, **change):
    """One launch of gatres_hydraulic_series into sentinel-filled, padded buffers; the outputs as an ``SR.Out``.  ``change``
    replaces inputs of the case (demand, roughness, mult, heads, level0) for this launch."""
    c = {**c, **change}
    net = c["net"]
    st = net.static()
    S, N, P, K = c["demand"].shape[0], net.num_nodes, net.num_pipes, net.num_tanks
    mult = up(c["mult"], np.float64)
    M, T = mult.shape[-2], mult.shape[-1]
    dem, rough, pattern = up(c["demand"], np.float64), up(c["roughness"], np.float64), up(c["pattern"], np.int32)
    fh = st["fixed_head"] if c["heads"] is None else up(c["heads"], np.float64)
    level0 = up(c["level0"][:S], np.float64)
    pb, p, pf = padded(S * T * N, torch.float32)
    hb, h, hf = padded(S * T * N, torch.float64)
    qb, q, qf = padded(S * T * P, torch.float64)
    lb, lv, lf = padded(S * (T + 1) * K, torch.float64)
    sb, s, sf = padded(S * T * H.HYD_STATUS, torch.int32)
    eb, e, ef = padded(S * T, torch.float64)
    tp = (lambda t: t.data_ptr()) if K else (lambda t: None)
    rc = lib.gatres_hydraulic_series(st["pipe_a"].data_ptr(), st["pipe_b"].data_ptr(), st["coef"].data_ptr(), st["q_start"].data_ptr(),
                                     st["fixed"].data_ptr(), st["elevation"].data_ptr(), st["order"].data_ptr(),
                                     st["position"].data_ptr(), net.half_bandwidth, tp(st["tank_node"]), tp(st["tank_area"]),
                                     tp(st["tank_min"]), tp(st["tank_max"]), K, pattern.data_ptr(), mult.data_ptr(),
                                     M * T if mult.dim() == 3 else 0, M, dem.data_ptr(), rough.data_ptr(), fh.data_ptr(),
                                     N if fh.dim() == 2 else 0, tp(level0), S, T, N, P, c["dt"], 1 if warm else 0, H.ACCURACY, max_iter,
                                     p.data_ptr(), h.data_ptr() if want_head else None, q.data_ptr() if want_flow else None, tp(lv),
                                     s.data_ptr(), e.data_ptr(), None)
    assert rc == 0
    torch.cuda.synchronize()
    out = SR.Out(unpad(hb, S * T * N, hf, "head").reshape(S, T, N), unpad(qb, S * T * P, qf, "flow").reshape(S, T, P),
                 unpad(lb, S * (T + 1) * K, lf, "level").reshape(S, T + 1, K), unpad(sb, S * T * 4, sf, "status").reshape(S, T, 4),
                 unpad(eb, S * T, ef, "final_dq").reshape(S, T), unpad(pb, S * T * N, pf, "pressure").reshape(S, T, N))
    if not want_head:
        assert (out.head == F_SENT).all()
    if not want_flow:
        assert (out.flow == F_SENT).all()
    return out


FIELDS = ("pressure", "head", "flow", "level", "status", "final_dq")


def differing(a, b, rows=None):
    """The fields of ``a`` that differ in some bit from those of ``b`` (from ``b[rows]`` where given)."""
    return [k for k in FIELDS if not same_bits(getattr(a, k), getattr(b, k) if rows is None else getattr(b, k)[rows])]


_RUNS = {}


def device_run(lib, name, warm=True):
    """The device's answer on a case: launched twice into fresh buffers, the same bits both times; computed once per case."""
    if (name, warm) not in _RUNS:
        a, b = raw_series(lib, SR.case(name), warm), raw_series(lib, SR.case(name), warm)
        assert differing(a, b) == [], f"{name}: two launches differ"
        _RUNS[(name, warm)] = a
    return _RUNS[(name, warm)]


# ---- 1. cold start: every step is gatres_hydraulic_solve, bit for bit -----------------------------------------------------------------
@pytest.mark.parametrize("name", ("two_t2", "net37_t12", "net40_t24", "net40_k0_t12", "net388_t4", "two_drain_t12"))
def test_cold_start_steps_equal_the_steady_kernel_in_every_bit(lib, name):
    """Step (s, t) against ``gatres_hydraulic_solve`` on demand * mult (one fp64 product, formed by torch on the device) and the
    fixed heads elevation + level[s][t] (from the series' own level output): pressure, head, flow, the first three status words
    and final_dq.  M = 1 and 3, both mult strides and both fixed_head strides are among the cases."""
    c = SR.case(name)
    net, S, T = c["net"], c["S"], c["T"]
    out = device_run(lib, name, warm=False)
    mult = up(c["mult"] if c["mult"].ndim == 3 else np.broadcast_to(c["mult"], (S,) + c["mult"].shape), np.float64)      # [S, M, T]
    per_node = mult.transpose(1, 2)[:, :, torch.from_numpy(c["pattern"].astype(np.int64)).to(DEV)]                      # [S, T, N]
    demand = (up(c["demand"], np.float64)[:, None, :] * per_node).reshape(S * T, -1)
    heads = up(np.broadcast_to(net.fixed_head if c["heads"] is None else c["heads"], (S, net.num_nodes)), np.float64)
    heads = heads[:, None, :].repeat(1, T, 1)
    tanks = torch.from_numpy(net.tank_nodes).to(DEV)
    heads[:, :, tanks] = up(net.elevation[net.tank_nodes], np.float64)[None, None, :] + up(out.level[:, :T], np.float64)
    rough = up(c["roughness"], np.float64)[:, None, :].repeat(1, T, 1).reshape(S * T, -1)
    one = net.simulate(demand, rough, heads.reshape(S * T, -1))
    wrong = [k for k, a, b in (("pressure", out.pressure, one.pressure), ("head", out.head, one.head), ("flow", out.flow, one.flow),
                               ("final_dq", out.final_dq, one.final_dq))
             if not same_bits(a.reshape(S * T, -1), b.cpu().numpy().reshape(S * T, -1))]
    if not np.array_equal(out.status[:, :, :3].reshape(S * T, 3), one.status.cpu().numpy()[:, :3]):
        wrong.append("status")
    print(f"\n[{name}] cold: {S * T} steps, iterations {out.status[:, :, 0].sum()}, fields that differ: {wrong}")
    assert wrong == []
    assert (out.status[:, :, 1] == 1).all() and (out.status[:, :, 2] == 0).all()
    assert np.array_equal(out.status[:, :, 0], SR.reference(name)["cold"].iterations)
    log = []
    missed = SR.check_series(name, out, agreement=False, start="cold", log=log)        # the level update, the flags, the physics, the balance
    print("\n".join(log))
    assert missed == []


# ---- 2. the level update, the flags, the physics, the balance, the agreement: THE CHECKER -----------------------------------------------
@pytest.mark.parametrize("name", SR.NAMES)
def test_warm_start_series_pass_the_checker(lib, name):
    """Warm start, every case: level[t + 1] and the clamp flag are ``level_update_ref`` of the device's own flows and levels in
    every bit (with and without clamping); heads, flows and levels agree with ``simulate_series_ref(warm_start=True)`` under the
    yardsticks of test_gpu_hydraulics.py (PHYSICS_FACTOR x the reference's residuals and balance, AGREEMENT_FACTOR x the
    dense-to-banded distance, the same floors; the level floor adds up dt / A_k times the flow floors of the tank's pipes over the
    earlier steps); the iteration counts per step are the reference's."""
    out, log = device_run(lib, name, warm=True), []
    missed = SR.check_series(name, out, agreement=True, log=log)
    print("\n" + "\n".join(log))
    assert missed == []
    ref = SR.reference(name)
    assert np.array_equal(out.status[:, :, 3] != 0, ref["dense"].limited)
    if name in SR.CLAMPED:
        assert 0 < (out.status[:, :, 3] != 0).sum() < out.status[:, :, 3].size


# ---- 3. isolation and failure ---------------------------------------------------------------------------------------------------------
def test_a_series_has_its_bits_alone_in_a_batch_and_past_the_grid_cap(lib):
    c = SR.case("two_t2")
    S = H.GRID_CAP + 3
    d_lo, d_hi, c_lo, c_hi = c["net"].draw_ranges((2e-4, 2e-3), H.ROUGHNESS_RANGE)
    demand, roughness = H.hydraulic_draws(77, 0, S, d_lo, d_hi, c_lo, c_hi)
    level0 = np.linspace(3.0, 6.0, S)[:, None]
    big = raw_series(lib, c, demand=demand, roughness=roughness, level0=level0)
    assert (big.status[:, :, 1] == 1).all()
    for s in (0, 1, H.GRID_CAP - 1, H.GRID_CAP, H.GRID_CAP + 2):         # the last two are taken by the second trip of the loop
        alone = raw_series(lib, c, demand=demand[s:s + 1], roughness=roughness[s:s + 1], level0=level0[s:s + 1])
        assert differing(alone, big, slice(s, s + 1)) == [], s
    batch = raw_series(lib, c, demand=demand[:3], roughness=roughness[:3], level0=level0[:3])
    assert differing(batch, big, slice(0, 3)) == []


def test_a_bad_series_fails_alone_and_from_its_step_on(lib):
    c = SR.case("net37_t12")
    mult = np.tile(c["mult"][None, :, :4], (c["S"], 1, 1))                 # four steps, a day per series
    good = raw_series(lib, c, mult=mult)
    assert (good.status[:, :, 1] == 1).all()
    rough = c["roughness"].copy()
    rough[1, 3] = np.nan                                                   # a NaN roughness: series 1 fails from step 0
    out = raw_series(lib, c, mult=mult, roughness=rough)
    assert (out.status[1] == np.array([0, 0, 1, 0], dtype=np.int32)).all()
    assert all(np.isnan(getattr(out, k)[1]).all() for k in ("pressure", "head", "flow", "final_dq")) and np.isnan(out.level[1, 1:]).all()
    assert same_bits(out.level[1, 0], c["level0"][1])
    assert [k for k in FIELDS if not same_bits(getattr(out, k)[[0, 2]], getattr(good, k)[[0, 2]])] == []
    for bad_value in (np.nan, -0.5):                                       # a bad multiplier at step 2: failed from there on
        m = mult.copy()
        m[1, 2, 2] = bad_value
        out = raw_series(lib, c, mult=m)
        assert out.status[1, :, 2].tolist() == [0, 0, 1, 1] and (out.status[1, 2:] == np.array([0, 0, 1, 0], dtype=np.int32)).all()
        for k in ("pressure", "head", "flow", "final_dq", "status"):
            assert same_bits(getattr(out, k)[1, :2], getattr(good, k)[1, :2]) and same_bits(getattr(out, k)[[0, 2]], getattr(good, k)[[0, 2]]), k
        assert all(np.isnan(getattr(out, k)[1, 2:]).all() for k in ("pressure", "head", "flow", "final_dq"))
        assert same_bits(out.level[1, :3], good.level[1, :3]) and np.isnan(out.level[1, 3:]).all() and same_bits(out.level[[0, 2]], good.level[[0, 2]])
        ref = H.simulate_series_ref(c["net"], c["demand"], c["roughness"], m, c["dt"], initial_level=c["level0"], pattern_of_node=c["pattern"])
        assert np.array_equal(out.status[:, :, 2] != 0, ref.failed) and np.array_equal(out.status[:, :, 0], ref.iterations)
    # static arrays that are not what gatres.h states: every series fails, nothing is read out of bounds
    net = c["net"]
    saved = dict(net.static())
    try:
        for key, change in (("tank_node", lambda t: torch.full_like(t, int(net.junctions[0]))),      # a junction
                            ("tank_node", lambda t: torch.full_like(t, net.num_nodes)),              # out of range
                            ("tank_area", lambda t: torch.zeros_like(t)),
                            ("tank_min", lambda t: torch.full_like(t, float("nan")))):
            net._static[key] = change(saved[key])
            out = raw_series(lib, c, mult=mult)
            assert (out.status == np.array([0, 0, 1, 0], dtype=np.int32)).all() and np.isnan(out.head).all(), key
            net._static[key] = saved[key]
    finally:
        net._static.update(saved)
    out = raw_series(lib, {**c, "pattern": np.full(net.num_nodes, 3, dtype=np.int32)}, mult=mult)      # a pattern index of M
    assert (out.status[:, :, 2] == 1).all() and np.isnan(out.flow).all()
    assert differing(raw_series(lib, c, mult=mult), good) == []


def test_optional_outputs_max_iter_two_and_the_method(lib):
    name = "net40_t24"
    c, full = SR.case(name), device_run(lib, name)
    for want_head, want_flow in ((False, False), (True, False), (False, True)):
        part = raw_series(lib, c, want_head=want_head, want_flow=want_flow)
        keep = ("pressure", "level", "status", "final_dq") + (("head",) if want_head else ()) + (("flow",) if want_flow else ())
        assert [k for k in keep if not same_bits(getattr(part, k), getattr(full, k))] == []
    few = raw_series(lib, c, max_iter=2)                                   # unconverged steps: finite outputs, the series goes on
    assert (few.status[:, :, :3] == np.array([2, 0, 0], dtype=np.int32)).all()
    assert all(np.isfinite(getattr(few, k)).all() for k in FIELDS) and (few.final_dq > H.ACCURACY).all()
    ref = SR.run_ref(c, max_iter=2)
    assert np.allclose(few.level, ref.level, rtol=1e-6) and not ref.converged.any()
    # HydraulicNetwork.simulate_series is the same launch; its fields stay on the device
    net = c["net"]
    res = net.simulate_series(c["demand"], c["roughness"], c["mult"], step_seconds=c["dt"], initial_level=c["level0"],
                              pattern_of_node=c["pattern"], fixed_head=c["heads"])
    assert all(t.is_cuda for t in res)
    for k in FIELDS:
        assert same_bits(getattr(res, k).cpu().numpy(), getattr(full, k)), k
    assert res.converged.all() and not res.failed.any() and not res.limited.any()
    assert np.array_equal(res.iterations.cpu().numpy(), full.status[:, :, 0])
    lean = net.simulate_series(c["demand"], c["roughness"], c["mult"], step_seconds=c["dt"], initial_level=c["level0"],
                               pattern_of_node=c["pattern"], fixed_head=c["heads"], want_head=False, want_flow=False)
    assert lean.head is None and lean.flow is None and same_bits(lean.pressure.cpu().numpy(), full.pressure)
    with pytest.raises(ValueError, match="pattern_of_node"):            # host data outside [0, M) is refused before the launch
        net.simulate_series(c["demand"], c["roughness"], c["mult"], step_seconds=c["dt"], pattern_of_node=np.full(net.num_nodes, 3))
    # the default initial level is fixed_head - elevation at the tanks; a network without tanks works
    c0 = SR.case("net40_k0_t12")
    res = c0["net"].simulate_series(c0["demand"], c0["roughness"], c0["mult"], step_seconds=c0["dt"], pattern_of_node=c0["pattern"])
    assert tuple(res.level.shape) == (3, 13, 0) and same_bits(res.head.cpu().numpy(), device_run(lib, "net40_k0_t12").head)
    c1 = SR.case("net37_t12")
    res = c1["net"].simulate_series(c1["demand"], c1["roughness"], c1["mult"], step_seconds=c1["dt"], pattern_of_node=c1["pattern"])
    assert same_bits(res.level.cpu().numpy(), device_run(lib, "net37_t12").level)


# ---- 4. the filter ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("allow_limited", (False, True))
def test_series_valid_equals_numpy(lib, allow_limited):
    net = SR.case("net37_t12")["net"]
    N, T, S = net.num_nodes, 5, 4200                                     # past the 4096 workgroups of the capped grid
    rng = np.random.RandomState(1)
    pressure = rng.uniform(10.0, 90.0, (S, T, N)).astype(np.float32)
    hit = rng.rand(S) < 0.15
    pressure[hit, rng.randint(0, T), rng.randint(0, N)] = 95.0           # above the range at one node of one step
    pressure[5, :, net.fixed_nodes[0]] = np.nan                          # a fixed node is not looked at
    pressure[6, T - 1, net.junctions[-1]] = np.nan                       # a junction is
    pressure[7, 0, net.junctions[0]] = np.float32(90.0)                  # the ends of the range belong to it
    pressure[8, T - 1, net.junctions[1]] = np.nextafter(np.float32(10.0), np.float32(0.0))
    status = np.zeros((S, T, 4), dtype=np.int32)
    status[:, :, 0], status[:, :, 1] = 7, 1
    status[rng.rand(S) < 0.1, rng.randint(0, T), 1] = 0                  # one step not converged
    status[rng.rand(S) < 0.05, T - 1, 2] = 1                             # the last step failed
    status[rng.rand(S) < 0.1, rng.randint(0, T), 3] = 1                  # one step clamped
    status[4100, 0, 3] = 1
    want = H.series_valid_ref(net, pressure, status, (10.0, 90.0), allow_limited)
    assert 0 < want.sum() < S and want[7] == 1 and want[8] == 0 and want[6] == 0 and want[4100] == int(allow_limited)
    vb, v, vf = padded(S, torch.uint8)
    p, s = up(pressure, np.float32), up(status, np.int32)
    assert lib.gatres_hydraulic_series_valid(p.data_ptr(), s.data_ptr(), net.static()["fixed"].data_ptr(), S, T, N, 10.0, 90.0,
                                             int(allow_limited), v.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(unpad(vb, S, vf, "valid"), want)


# ---- 5. the store ---------------------------------------------------------------------------------------------------------------------
def series_network(pkg):
    return pkg.wdn_synth.make_hydraulic_network(37, 41, 2, seed=32, elevation_range=(0.0, 30.0), num_tanks=1)


def test_generate_series_store_equals_its_pass_written_out(pkg, lib, monkeypatch):
    net = series_network(pkg)
    S, T, chunk, seed, dt = 20, 12, 8, 99, 300.0
    demand_range, pressure_range, level_range = (1e-4, 1e-3), (54.0, 120.0), (1.0, 5.0)
    mult = pkg.wdn_synth.make_demand_patterns(2, T, dt, 5)
    pattern = (np.arange(net.num_nodes) % 2).astype(np.int32)
    reads = {"cpu": 0, "item": 0}
    real_cpu, real_item = torch.Tensor.cpu, torch.Tensor.item

    def counted(key, fn):
        def f(self, *a, **k):
            if self.is_cuda:
                reads[key] += 1
            return fn(self, *a, **k)
        return f

    net.static()
    monkeypatch.setattr(torch.Tensor, "cpu", counted("cpu", real_cpu))
    monkeypatch.setattr(torch.Tensor, "item", counted("item", real_item))
    store, report = net.generate_series_store(S, T, seed, step_seconds=dt, multipliers=mult, pattern_of_node=pattern,
                                              level_range=level_range, demand_range=demand_range, pressure_range=pressure_range,
                                              chunk=chunk)
    monkeypatch.setattr(torch.Tensor, "cpu", real_cpu)
    monkeypatch.setattr(torch.Tensor, "item", real_item)
    chunks = -(-S // chunk)
    print(f"\nread-backs {reads} in {chunks} chunks; report {report}")
    assert reads["cpu"] == chunks and reads["item"] <= 3                 # one read-back per chunk; the store's own statistics
    # the pass written out with the public calls, in one piece
    demand, roughness = H.hydraulic_draws(seed, 0, S, *net.draw_ranges(demand_range, H.ROUGHNESS_RANGE))
    lo, hi = net.level_ranges(level_range)
    level0, _ = H.hydraulic_draws((seed + 0x74616E6B) % (1 << 64), 0, S, lo, hi, np.zeros(1), np.zeros(1))
    assert (lo.tolist(), hi.tolist()) == ([1.0], [5.0]) and level0.shape == (S, 1) and (level0 >= 1.0).all() and (level0 < 5.0).all()
    res = net.simulate_series(demand, roughness, mult, step_seconds=dt, initial_level=level0, pattern_of_node=pattern)
    status, pressure = res.status.cpu().numpy(), res.pressure.cpu().numpy()
    ok = H.series_valid_ref(net, pressure, status, pressure_range).astype(bool)
    assert np.array_equal(net.series_valid(res, pressure_range).cpu().numpy().astype(bool), ok)
    rows = pressure[ok][:, :, ~net.fixed].reshape(int(ok.sum()) * T, -1)                       # series-major: E * T rows
    want = pkg.SnapshotStore(up(rows, np.float32), net.junction_edge_index, device=DEV)
    assert same_bits(store.data.cpu().numpy(), want.data.cpu().numpy()) and store.mean == want.mean and store.std == want.std
    assert len(store) == int(ok.sum()) * T and store.nodes_per_graph == 35
    assert report == H.series_report(status, ok) and report["drawn"] == S and 0 < report["kept"] == int(ok.sum())
    assert report["drawn"] == report["kept"] + report["failed"] + report["not_converged"] + report["limited"] + report["out_of_range"]
    assert report["series_length"] == T and report["mean_iterations_first_step"] > report["mean_iterations"]       # warm start pays
    raw, _ = net.generate_series_store(S, T, seed, step_seconds=dt, multipliers=mult, pattern_of_node=pattern, level_range=level_range,
                                       demand_range=demand_range, pressure_range=pressure_range, chunk=S, normalize=False)
    assert same_bits(raw.data.cpu().numpy(), rows)
    with pytest.raises(RuntimeError, match="no series"):
        net.generate_series_store(4, T, seed, multipliers=mult, pattern_of_node=pattern, pressure_range=(1e6, 2e6))
    with pytest.raises(ValueError):
        net.generate_series_store(0, T, seed)


def test_monitor_and_trainer_run_on_a_generated_series_store(pkg):
    """No accuracy claim: the drift monitor is calibrated on one series store and run on another whose rows ARE consecutive states
    of one network, and the trainer takes one epoch on it, without error and finite."""
    net = series_network(pkg)
    T = 12
    kw = dict(demand_range=(1e-4, 5e-4), pressure_range=(-1e3, 1e3))
    clean, rep = net.generate_series_store(4, T, 5, **kw)
    raw, rep2 = net.generate_series_store(4, T, 6, normalize=False, **kw)
    test = pkg.SnapshotStore(raw.data, net.junction_edge_index, device=DEV, mean=clean.mean, std=clean.std)      # the first store's scale
    assert len(clean) == 4 * T == len(test) and rep["kept"] == 4 and rep2["series_length"] == T
    model = pkg.GATResMeanConv(num_blocks=2, nc=8).to(DEV)
    est = pkg.PressureEstimator.for_store(model, clean, [1, 9, 20, 30], batch_size=8)
    mb = est.calibrate_monitor(clean)
    res = est.monitor_store(test, mb, series_length=T)
    assert tuple(res.latched.shape)[0] == 4
    trainer = pkg.GATResTrainer.for_store(model, clean, batch_size=8)
    loss, _ = trainer.fit_epoch(clean, batch_size=8)
    assert np.isfinite(loss)
