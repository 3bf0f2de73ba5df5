"""The hydraulic snapshot generator on the device (k_hydraulics.hip) against its host statements (hydraulics.py): the draws bit for
bit; the solver against closed forms and the tree solution, against the physics (``hydraulic_residuals``) and against
``solve_ref``, each bound formed in hydraulics_refs.py from the reference's own error; pressure bits, determinism and independence
of a scenario's position; bad inputs; the filter; ``generate_store`` against its pass written out; and one end-to-end run of the
trainer and the estimator on a generated store.  Every figure is printed before it is asserted.

Measured on the MI355X (profiles/hydraulic_margins.txt holds every case): see that file."""
import numpy as np
import pytest
import torch

import hydraulics_refs as HR

pytestmark = pytest.mark.gpu
H = HR.H
DEV = "cuda:0"
GUARD = 32                     # elements of sentinel on either side of every output
F_SENT, I_SENT = -777.25, -777


def padded(n, dtype):
    fill = I_SENT if dtype in (torch.int32, torch.uint8) else F_SENT
    if dtype == torch.uint8:
        fill = 0xA5
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n], fill


def unpad(buf, n, fill, what):
    """The written part as numpy, after checking that the guard words are intact."""
    host = buf.cpu().numpy()
    assert (host[:GUARD] == fill).all() and (host[GUARD + n:] == fill).all(), f"{what}: guard words overwritten"
    return host[GUARD:GUARD + n].copy()


def up(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def raw_draw(lib, net, S, seed, first, ranges):
    N, P = net.num_nodes, net.num_pipes
    dev = [up(a, np.float64) for a in ranges]
    db, d, df = padded(S * N, torch.float64)
    rb, r, rf = padded(S * P, torch.float64)
    rc = lib.gatres_hydraulic_draw(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), S, N, P, seed, first,
                                   d.data_ptr(), r.data_ptr(), None)
    assert rc == 0
    torch.cuda.synchronize()
    return unpad(db, S * N, df, "demand").reshape(S, N), unpad(rb, S * P, rf, "roughness").reshape(S, P)


def raw_solve(lib, net, demand, roughness, heads=None, want_head=True, want_flow=True, accuracy=H.ACCURACY, max_iter=H.MAX_ITER):
    """One launch of gatres_hydraulic_solve into sentinel-filled, padded buffers; the outputs as numpy."""
    st = net.static()
    S, N, P = demand.shape[0], net.num_nodes, net.num_pipes
    dem, rough = up(demand, np.float64), up(roughness, np.float64)
    fh = st["fixed_head"] if heads is None else up(heads, np.float64)
    stride = 0 if fh.dim() == 1 else N
    pb, p, pf = padded(S * N, torch.float32)
    hb, h, hf = padded(S * N, torch.float64)
    qb, q, qf = padded(S * P, torch.float64)
    sb, s, sf = padded(S * H.HYD_STATUS, torch.int32)
    eb, e, ef = padded(S, torch.float64)
    rc = lib.gatres_hydraulic_solve(st["pipe_a"].data_ptr(), st["pipe_b"].data_ptr(), st["coef"].data_ptr(), st["q_start"].data_ptr(),
                                    st["fixed"].data_ptr(), st["elevation"].data_ptr(), st["order"].data_ptr(),
                                    st["position"].data_ptr(), net.half_bandwidth, dem.data_ptr(), rough.data_ptr(), fh.data_ptr(),
                                    stride, S, N, P, accuracy, max_iter, p.data_ptr(), h.data_ptr() if want_head else None,
                                    q.data_ptr() if want_flow else None, s.data_ptr(), e.data_ptr(), None)
    assert rc == 0
    torch.cuda.synchronize()
    out = {"pressure": unpad(pb, S * N, pf, "pressure").reshape(S, N), "head": unpad(hb, S * N, hf, "head").reshape(S, N),
           "flow": unpad(qb, S * P, qf, "flow").reshape(S, P), "status": unpad(sb, S * H.HYD_STATUS, sf, "status").reshape(S, -1),
           "final_dq": unpad(eb, S, ef, "final_dq")}
    if not want_head:
        assert (out["head"] == F_SENT).all()
    if not want_flow:
        assert (out["flow"] == F_SENT).all()
    return out


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


_RUNS = {}


def device_run(lib, name):
    """The device's answer on a case: launched twice into fresh buffers, the same bits both times; computed once per case."""
    if name not in _RUNS:
        net, demand, roughness, heads = HR.case(name)
        a = raw_solve(lib, net, demand, roughness, heads)
        b = raw_solve(lib, net, demand, roughness, heads)
        for k in a:
            assert same_bits(a[k], b[k]), f"{name}: {k} differs between two launches"
        _RUNS[name] = a
    return _RUNS[name]


# ---- 1. the draws -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,S", [("two_s1", 1), ("net37_s3", 3), ("net40_s3", 5), ("net388_s3", 1300)])
def test_draw_equals_hydraulic_draws_bit_for_bit(lib, name, S):
    """S = 1300 at 818 cells per scenario is past the 4096 x 256 threads of the capped grid."""
    net = HR.case(name)[0]
    ranges = net.draw_ranges((1e-5, 2e-3), H.ROUGHNESS_RANGE)
    seed, first = 0xFEEDFACECAFEBEEF, 12345678901
    want = H.hydraulic_draws(seed, first, S, *ranges)
    got = raw_draw(lib, net, S, seed, first, ranges)
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
    assert (got[0][:, net.fixed] == 0.0).all()
    if S >= 3:                                      # two chunks are one call
        k = S // 3
        a, b = raw_draw(lib, net, k, seed, first, ranges), raw_draw(lib, net, S - k, seed, first + k, ranges)
        assert same_bits(np.concatenate([a[0], b[0]]), want[0]) and same_bits(np.concatenate([a[1], b[1]]), want[1])
    dev = [up(a, np.float64) for a in ranges]
    d, r = net.draw(S, seed, first, *dev)           # the method is the same launch
    assert same_bits(d.cpu().numpy(), want[0]) and same_bits(r.cpu().numpy(), want[1])


# ---- 2. the solver ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", HR.NAMES)
def test_solve_converges_and_pressure_is_fp32_of_head_minus_elevation(lib, name):
    net, demand, roughness, heads = HR.case(name)
    out = device_run(lib, name)
    st = out["status"]
    print(f"\n[{name}] iterations {st[:, 0].min()}..{st[:, 0].max()} (reference {HR.reference(name)['dense'].iterations.max()}), "
          f"final dq max {out['final_dq'].max():.3e}")
    assert (st[:, 1] == 1).all() and (st[:, 2] == 0).all() and (st[:, 3] == 0).all()
    assert (st[:, 0] >= 1).all() and (st[:, 0] <= H.MAX_ITER).all() and (out["final_dq"] <= H.ACCURACY).all()
    assert np.isfinite(out["head"]).all() and np.isfinite(out["flow"]).all()
    assert same_bits(out["pressure"], (out["head"] - net.elevation[None, :]).astype(np.float32))
    fixed_heads = np.broadcast_to(net.fixed_head if heads is None else heads, out["head"].shape)
    assert same_bits(out["head"][:, net.fixed], np.ascontiguousarray(fixed_heads[:, net.fixed]))


@pytest.mark.parametrize("name", HR.NAMES)
def test_solve_satisfies_the_physics_as_well_as_the_reference_does(lib, name):
    """mass / sum |q| and energy in metres of the device's (head, flow), per scenario, <= 8 x the larger of the two host solvers'
    own residuals on the same scenario (floored at 64 ulp of the scale where that is zero)."""
    net, demand, roughness, heads = HR.case(name)
    out, ref = device_run(lib, name), HR.reference(name)
    mass, energy = H.hydraulic_residuals(net, out["head"], out["flow"], demand, roughness, heads)
    b_mass = HR.bound(ref["mass"], ref["floors"]["mass"], HR.PHYSICS_FACTOR)
    b_energy = HR.bound(ref["energy"], ref["floors"]["energy"], HR.PHYSICS_FACTOR)
    i, j = int(np.argmax(mass / b_mass)), int(np.argmax(energy / b_energy))
    print(f"\n[{name}] mass dev {mass[i]:.3e} ref {ref['mass'][i]:.3e} bound {b_mass[i]:.3e} | energy dev {energy[j]:.3e} m "
          f"ref {ref['energy'][j]:.3e} bound {b_energy[j]:.3e}")
    assert (mass <= b_mass).all() and (energy <= b_energy).all()


@pytest.mark.parametrize("name", HR.NAMES)
def test_solve_agrees_with_the_reference_as_its_two_solvers_agree(lib, name):
    """|H_dev - H_ref| / (max H - min H) and |q_dev - q_ref| / max |q| against the dense reference, for every scenario, <= 4 x the
    same quantity between solve_ref dense and banded ON THAT CASE (its largest over the case's scenarios: two runs of one
    algorithm that differ in rounding alone are two draws of one noise, and a single scenario's draw may come out 5 x another's
    -- a numpy emulation of the kernel's arithmetic shows the same spread against the two host solvers).  The floors of
    hydraulics_refs.py lie under it: 64 ulp of the largest head for the heads, and per pipe 64 ulp of the largest head over
    the pipe's gradient for the flows."""
    net, demand, roughness, heads = HR.case(name)
    out, ref = device_run(lib, name), HR.reference(name)
    dh, dq = HR.distances(net, out["head"], out["flow"], ref["dense"])
    b_h = HR.bound(ref["dh"].max(), ref["floors"]["dh"], HR.AGREEMENT_FACTOR)                            # [S]
    qmax = np.abs(ref["dense"].flow).max(axis=1)
    dq_pipe = np.abs(out["flow"] - ref["dense"].flow) / qmax[:, None]                                     # [S, P]
    b_q = HR.bound(ref["dq"].max(), ref["floors"]["flow"] / qmax[:, None], HR.AGREEMENT_FACTOR)          # [S, P]
    i = int(np.argmax(dh / b_h))
    j = np.unravel_index(int(np.argmax(dq_pipe / b_q)), b_q.shape)
    dh_b, dq_b = HR.distances(net, out["head"], out["flow"], ref["banded"])
    print(f"\n[{name}] head dev-dense {dh[i]:.3e} (dev-banded {dh_b.max():.3e}) dense-banded {ref['dh'].max():.3e} bound {b_h[i]:.3e} | "
          f"flow dev-dense {dq_pipe[j]:.3e} (max {dq.max():.3e}, dev-banded {dq_b.max():.3e}) dense-banded {ref['dq'].max():.3e} "
          f"bound {b_q[j]:.3e}")
    assert (dh <= b_h).all() and (dq_pipe <= b_q).all()


@pytest.mark.parametrize("name", HR.EXACT)
def test_solve_meets_the_closed_forms_and_the_tree_solution(lib, name):
    """Against an answer that needs no Newton: the device's distance from it <= 4 x the reference's own distance from it on the
    same case (the larger of the two host solvers'; the floors of hydraulics_refs.py under it, per pipe for the flows)."""
    net = HR.case(name)[0]
    out, ref = device_run(lib, name), HR.reference(name)
    head, flow = HR.exact(name)
    err = lambda h, q: (np.abs(h - head).max(), np.abs(q - flow).max())
    ref_h, ref_q = np.maximum(err(ref["dense"].head, ref["dense"].flow), err(ref["banded"].head, ref["banded"].flow))
    dev_h, dev_q = err(out["head"], out["flow"])
    b_h = HR.EXACT_FACTOR * max(ref_h, HR.FLOOR_ULPS * HR.EPS * np.abs(head).max())
    b_q = HR.EXACT_FACTOR * np.maximum(ref_q, ref["floors"]["flow"])                                      # [S, P]
    print(f"\n[{name}] exact: head dev {dev_h:.3e} m ref {ref_h:.3e} bound {b_h:.3e} | flow dev {dev_q:.3e} ref {ref_q:.3e} "
          f"bound {b_q.min():.3e} .. {b_q.max():.3e}")
    assert dev_h <= b_h and (np.abs(out["flow"] - flow) <= b_q).all()


def test_a_scenario_has_its_bits_alone_and_past_the_grid_cap(lib):
    net, demand, roughness, _ = HR.case("path12_cap")
    out = device_run(lib, "path12_cap")
    assert demand.shape[0] > H.GRID_CAP
    for s in (0, H.GRID_CAP - 1, H.GRID_CAP, H.GRID_CAP + 2):       # the last two are taken by the second trip of the loop
        alone = raw_solve(lib, net, demand[s:s + 1], roughness[s:s + 1])
        for k in alone:
            assert same_bits(alone[k], out[k][s:s + 1]), (s, k)
    net, demand, roughness, _ = HR.case("net388_s3")                # and on the large network: scenario 2 alone
    alone, out = raw_solve(lib, net, demand[2:3], roughness[2:3]), device_run(lib, "net388_s3")
    for k in alone:
        assert same_bits(alone[k], out[k][2:3]), k


def test_optional_outputs_strides_and_the_method(lib):
    net, demand, roughness, heads = HR.case("net40_heads_s3")
    full = device_run(lib, "net40_heads_s3")
    for want_head, want_flow in ((False, False), (True, False), (False, True)):
        part = raw_solve(lib, net, demand, roughness, heads, want_head=want_head, want_flow=want_flow)
        for k in ("pressure", "status", "final_dq") + (("head",) if want_head else ()) + (("flow",) if want_flow else ()):
            assert same_bits(part[k], full[k]), (want_head, want_flow, k)
    # one shared row of fixed heads (stride 0) is the same as that row repeated per scenario (stride N)
    shared = device_run(lib, "net40_s3")
    tiled = raw_solve(lib, net, demand, roughness, np.tile(net.fixed_head, (3, 1)))
    for k in shared:
        assert same_bits(shared[k], tiled[k]), k
    assert not same_bits(shared["head"], full["head"])              # (the per-scenario heads are other heads)
    # HydraulicNetwork.simulate is the same launch; its fields stay on the device
    res = net.simulate(demand, roughness, heads)
    assert all(t.is_cuda for t in (res.pressure, res.head, res.flow, res.iterations, res.converged, res.failed, res.final_dq))
    assert same_bits(res.pressure.cpu().numpy(), full["pressure"]) and same_bits(res.head.cpu().numpy(), full["head"])
    assert same_bits(res.flow.cpu().numpy(), full["flow"]) and same_bits(res.status.cpu().numpy(), full["status"])
    assert res.converged.all() and not res.failed.any() and (res.iterations.cpu().numpy() == full["status"][:, 0]).all()
    lean = net.simulate(torch.from_numpy(demand), up(roughness, np.float64), up(heads, np.float64), want_head=False, want_flow=False)
    assert lean.head is None and lean.flow is None and same_bits(lean.pressure.cpu().numpy(), full["pressure"])


# ---- 3. bad inputs ----------------------------------------------------------------------------------------------------------------
def test_max_iter_two_stops_unconverged_with_finite_outputs(lib):
    for name in ("net37_s3", "net388_s3"):
        net, demand, roughness, heads = HR.case(name)
        out = raw_solve(lib, net, demand, roughness, heads, max_iter=2)
        assert (out["status"] == np.array([2, 0, 0, 0], dtype=np.int32)).all()
        assert np.isfinite(out["head"]).all() and np.isfinite(out["flow"]).all() and np.isfinite(out["pressure"]).all()
        assert (out["final_dq"] > H.ACCURACY).all() and np.isfinite(out["final_dq"]).all()
        # the same two iterations on the host (a flat pipe's flow is determined to 1e-6 of the largest, hydraulics_refs.py)
        ref = H.solve_ref(net, demand, roughness, heads, max_iter=2)
        assert not ref.converged.any() and np.allclose(out["flow"], ref.flow, rtol=1e-6, atol=1e-5 * np.abs(ref.flow).max())


def test_zero_demand_on_the_device_as_on_the_host(lib):
    """test_hydraulics_host.py states what holds at zero demand and what does not (the flows do not settle on the linear
    branch, the stop rule is not met); the device is held to the same: nothing fails or is NaN, every head is the fixed head
    to 1e-6 m, and the head loss of every returned flow is below 2e-6 m."""
    for name in ("net37_s3", "tree37_s3"):
        net, _, roughness, _ = HR.case(name)
        out = raw_solve(lib, net, np.zeros((3, net.num_nodes)), roughness)
        assert (out["status"][:, 2] == 0).all() and all(np.isfinite(out[k]).all() for k in ("head", "flow", "pressure", "final_dq"))
        h, g = H.pipe_headloss(out["flow"], net.coef[None, :] / roughness ** 1.852)
        print(f"\n[{name}] zero demand: iterations {out['status'][:, 0]}, converged {out['status'][:, 1]}, {int((g > 1e-7).sum())} of "
              f"{g.size} flows off the linear branch, heads off by {np.abs(out['head'] - net.fixed_head[net.fixed][0]).max():.2e} m, "
              f"max |h(q)| {np.abs(h).max():.2e} m")
        assert np.abs(out["head"] - net.fixed_head[net.fixed][0]).max() <= 1e-6 and np.abs(h).max() <= 2e-6


def test_a_bad_scenario_fails_alone_and_its_neighbours_keep_their_bits(lib):
    net, demand, roughness, heads = HR.case("net37_s3")
    good = device_run(lib, "net37_s3")
    j = int(net.junctions[5])
    f = int(net.fixed_nodes[0])
    cases = []
    d = demand.copy(); d[1, j] = np.nan; cases.append(("a NaN demand", d, roughness, None))
    d = demand.copy(); d[1, j] = np.inf; cases.append(("an infinite demand", d, roughness, None))
    r = roughness.copy(); r[1, 7] = 0.0; cases.append(("a zero roughness", demand, r, None))
    r = roughness.copy(); r[1, 7] = -100.0; cases.append(("a negative roughness", demand, r, None))
    r = roughness.copy(); r[1, 7] = np.nan; cases.append(("a NaN roughness", demand, r, None))
    h = np.tile(net.fixed_head, (3, 1)); h[1, f] = np.nan; cases.append(("a NaN fixed head", demand, roughness, h))
    for what, d, r, h in cases:
        out = raw_solve(lib, net, d, r, h)
        assert (out["status"][1] == np.array([0, 0, 1, 0], dtype=np.int32)).all(), what
        assert np.isnan(out["head"][1]).all() and np.isnan(out["flow"][1]).all() and np.isnan(out["pressure"][1]).all(), what
        assert np.isnan(out["final_dq"][1]), what
        for k in out:
            assert same_bits(out[k][[0, 2]], good[k][[0, 2]]), (what, k)
    # a NaN where nothing reads it changes nothing: the demand of a fixed node, the fixed head of a junction
    d = demand.copy(); d[1, f] = np.nan
    h = np.tile(net.fixed_head, (3, 1)); h[1, j] = np.nan
    out = raw_solve(lib, net, d, roughness, h)
    for k in out:
        assert same_bits(out[k], good[k]), k
    # static arrays that are not what the header states: every scenario fails, nothing is read out of bounds
    saved = dict(net.static())
    try:
        for key, change in (("pipe_b", lambda t: t.clone().index_fill_(0, torch.tensor([3], device=DEV), net.num_nodes)),
                            ("pipe_a", lambda t: t.clone().index_fill_(0, torch.tensor([0], device=DEV), -1)),
                            ("position", lambda t: torch.zeros_like(t)),
                            ("order", lambda t: t.flip(0).contiguous())):
            net._static[key] = change(saved[key])
            out = raw_solve(lib, net, demand, roughness)
            assert (out["status"] == np.array([0, 0, 1, 0], dtype=np.int32)).all(), key
            assert np.isnan(out["head"]).all() and np.isnan(out["flow"]).all() and np.isnan(out["pressure"]).all(), key
            net._static[key] = saved[key]
    finally:
        net._static.update(saved)
    out = raw_solve(lib, net, demand, roughness)
    for k in out:
        assert same_bits(out[k], good[k]), k


# ---- 4. the filter and the store --------------------------------------------------------------------------------------------------
def test_valid_equals_numpy(lib):
    net = HR.case("net37_s3")[0]
    N, S = net.num_nodes, 300
    rng = np.random.RandomState(0)
    pressure = rng.uniform(10.0, 90.0, (S, N)).astype(np.float32)
    pressure[rng.rand(S) < 0.2, rng.randint(0, N)] = 95.0               # above the range at one node
    pressure[5, net.fixed_nodes[0]] = np.nan                            # a fixed node is not looked at
    pressure[6, net.junctions[-1]] = np.nan                             # a junction is
    pressure[7, net.junctions[0]] = np.float32(90.0)                    # the ends of the range belong to it
    pressure[8, net.junctions[1]] = np.float32(10.0)
    pressure[9, net.junctions[2]] = np.nextafter(np.float32(10.0), np.float32(0.0))
    status = np.zeros((S, 4), dtype=np.int32)
    status[:, 0] = 7
    status[:, 1] = rng.rand(S) < 0.9
    status[:, 2] = rng.rand(S) < 0.05
    lo, hi = 10.0, 90.0
    inside = ((pressure.astype(np.float64) >= lo) & (pressure.astype(np.float64) <= hi))[:, ~net.fixed].all(axis=1)
    want = ((status[:, 1] != 0) & (status[:, 2] == 0) & inside).astype(np.uint8)
    assert 0 < want.sum() < S
    vb, v, vf = padded(S, torch.uint8)
    p, s = up(pressure, np.float32), up(status, np.int32)
    assert lib.gatres_hydraulic_valid(p.data_ptr(), s.data_ptr(), net.static()["fixed"].data_ptr(), S, N, lo, hi, v.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert (unpad(vb, S, vf, "valid") == want).all()


def test_generate_store_equals_its_pass_written_out(pkg, lib, monkeypatch):
    net = pkg.wdn_synth.make_hydraulic_network(37, 41, 1, seed=3, elevation_range=(0.0, 30.0))
    S, chunk, seed = 50, 16, 99
    demand_range, pressure_range = (1e-4, 2e-3), (20.0, 110.0)
    reads = {"cpu": 0, "item": 0}
    real_cpu, real_item = torch.Tensor.cpu, torch.Tensor.item

    def counted(key, fn):
        def f(self, *a, **k):
            if self.is_cuda:
                reads[key] += 1
            return fn(self, *a, **k)
        return f

    net.static()                                                     # (the static arrays are uploaded before the count)
    monkeypatch.setattr(torch.Tensor, "cpu", counted("cpu", real_cpu))
    monkeypatch.setattr(torch.Tensor, "item", counted("item", real_item))
    store, report = net.generate_store(S, seed, demand_range=demand_range, pressure_range=pressure_range, chunk=chunk)
    monkeypatch.setattr(torch.Tensor, "cpu", real_cpu)
    monkeypatch.setattr(torch.Tensor, "item", real_item)
    chunks = -(-S // chunk)
    print(f"\nread-backs {reads} in {chunks} chunks; report {report}")
    assert reads["cpu"] == chunks                                    # one read-back per chunk ...
    assert reads["item"] <= 3                                        # ... and the store's own statistics (mean, std, edge check)
    # the pass written out, in one piece: draw, solve, valid, select, SnapshotStore
    ranges = net.draw_ranges(demand_range, H.ROUGHNESS_RANGE)
    demand, roughness = H.hydraulic_draws(seed, 0, S, *ranges)
    out = raw_solve(lib, net, demand, roughness)
    p64 = out["pressure"].astype(np.float64)[:, ~net.fixed]
    ok = (out["status"][:, 1] == 1) & (out["status"][:, 2] == 0) & ((p64 >= pressure_range[0]) & (p64 <= pressure_range[1])).all(axis=1)
    rows = up(out["pressure"][ok][:, ~net.fixed], np.float32)
    want = pkg.SnapshotStore(rows, net.junction_edge_index, device=DEV)
    assert same_bits(store.data.cpu().numpy(), want.data.cpu().numpy()) and store.mean == want.mean and store.std == want.std
    assert store.nodes_per_graph == 36 and len(store) == int(ok.sum()) and store.norm_type == "znorm"
    assert torch.equal(store.edge_index_single.cpu(), net.junction_edge_index)
    assert report["drawn"] == S and report["kept"] == int(ok.sum()) and 0 < report["kept"] < S
    assert report["kept"] + report["out_of_range"] + report["not_converged"] + report["failed"] == report["drawn"]
    assert report["converged"] == int(out["status"][:, 1].sum()) and report["failed"] == 0
    assert report["max_iterations"] == int(out["status"][:, 0].max())
    assert report["mean_iterations"] == pytest.approx(out["status"][:, 0].mean(), rel=1e-12)
    raw, _ = net.generate_store(S, seed, demand_range=demand_range, pressure_range=pressure_range, chunk=S, normalize=False)
    assert same_bits(raw.data.cpu().numpy(), out["pressure"][ok][:, ~net.fixed]) and raw.norm_type == "unused"
    with pytest.raises(RuntimeError, match="no scenario"):           # a range that keeps nothing
        net.generate_store(8, seed, demand_range=demand_range, pressure_range=(1e6, 2e6))
    with pytest.raises(ValueError):
        net.generate_store(0, seed)


# ---- 5. end to end ----------------------------------------------------------------------------------------------------------------
def test_trainer_and_estimator_run_on_a_generated_store(pkg):
    """No accuracy claim: two optimisation steps and one estimation pass on physical data, without error and finite."""
    net = pkg.wdn_synth.make_hydraulic_network(37, 41, 1, seed=3, elevation_range=(0.0, 30.0))
    deg = np.bincount(net.junction_edge_index[0].numpy(), minlength=36)
    assert (deg > 0).all()                                           # (no junction hangs on the reservoir alone)
    store, report = net.generate_store(4, 5, demand_range=(1e-4, 5e-4), pressure_range=(-1e3, 1e3))
    assert len(store) == 4 and report["kept"] == 4
    model = pkg.GATResMeanConv(num_blocks=2, nc=8).to(DEV)
    trainer = pkg.GATResTrainer.for_store(model, store, batch_size=2)
    loss, _ = trainer.fit_epoch(store, batch_size=2)                 # two steps
    assert np.isfinite(loss)
    est = pkg.PressureEstimator.for_store(model, store, [1, 9, 20, 30], batch_size=2)
    estimate = est.estimate_store(store)
    assert tuple(estimate.shape)[0] == 4 and torch.isfinite(estimate).all()
