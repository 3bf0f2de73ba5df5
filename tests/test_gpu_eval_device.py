"""The evaluation epoch on the device (evaluation.evaluate_store): the mask sampler with required nodes, the masked-metric
moments kernel, agreement with the host loop's functions over the same masks, and the epoch's single synchronisation."""
import math

import numpy as np
import pytest
import torch

import metric_moments_ref as MR      # noqa: E402

pytestmark = pytest.mark.gpu

NODES, PIPES = 388, 430
SENSORS = [3, 17, 100, 101, 250, 387]


def make_store(pkg, S, seed=1):
    ei = pkg.wdn_synth.make_wdn_topology(NODES, PIPES, seed=0)
    snaps = pkg.wdn_synth.make_snapshots(S, NODES, seed=seed) * 12.5 + 50.0      # pressures around 50 m
    return pkg.SnapshotStore(snaps, ei, device="cuda:0")


def make_model(pkg, nb, nc, seed, fused=True, dtype="fp32"):
    torch.manual_seed(seed)
    m = pkg.GATResMeanConv(num_blocks=nb, nc=nc, fused=fused).cuda()
    if dtype != "fp32":
        m.set_compute_dtype(dtype)
    return m


def node_ptr(B, n=NODES):
    return torch.arange(0, (B + 1) * n, n, dtype=torch.int32, device="cuda:0")


def stage_required(pkg, lib, B, rate, seed, step, required, n=NODES):
    data = torch.zeros((B, n), dtype=torch.float32, device="cuda:0")
    rows = torch.arange(B, dtype=torch.int64, device="cuda:0")
    x = torch.empty(B * n, dtype=torch.float32, device="cuda:0")
    mask = torch.empty(B * n, dtype=torch.uint8, device="cuda:0")
    steps = torch.tensor([step], dtype=torch.int64, device="cuda:0")
    req = torch.tensor(required, dtype=torch.int32, device="cuda:0") if required else None
    pkg._native.check(lib.gatres_stage_rows_mask_required(
        data.data_ptr(), rows.data_ptr(), n, x.data_ptr(), None, node_ptr(B, n).data_ptr(), B, rate, seed, steps.data_ptr(),
        pkg._native.ptr(req), len(required), mask.data_ptr(), pkg._native.current_stream(x.device)),
        "gatres_stage_rows_mask_required")
    return mask.view(B, n)


# ---- the sampler ---------------------------------------------------------------------------------------------------------
def test_required_nodes_always_masked_and_the_rest_uniform(pkg, lib):
    B, rate = 64, 0.5
    k = int(NODES * rate)
    free = np.setdiff1d(np.arange(NODES), SENSORS)
    hits = np.zeros(NODES, dtype=np.int64)
    draws = 0
    for step in range(40):
        m = stage_required(pkg, lib, B, rate, 1234, step, SENSORS).cpu().numpy().astype(np.int64)
        assert (m.sum(axis=1) == k).all()
        assert (m[:, SENSORS] == 1).all()
        hits += m.sum(axis=0)
        draws += B
    # uniform over the non-required nodes: chi-square of their hit counts (367 degrees of freedom; mean 367, sd ~27)
    expect = draws * (k - len(SENSORS)) / len(free)
    chi2 = float((((hits[free] - expect) ** 2) / expect).sum())
    assert chi2 < len(free) - 1 + 6 * math.sqrt(2 * (len(free) - 1)), chi2


def test_required_nodes_on_graphs_beyond_the_all_pairs_rank(pkg, lib):
    """Graphs of more than 2048 nodes take the radix-select path of the sampler (k_mask.h)."""
    n, B, rate = 3000, 3, 0.3
    k = int(n * rate)
    req = [0, 5, 1999, 2048, 2500, 2999]
    free = np.setdiff1d(np.arange(n), req)
    hits = np.zeros(n, dtype=np.int64)
    for step in range(6):
        m = stage_required(pkg, lib, B, rate, 99, step, req, n=n).cpu().numpy().astype(np.int64)
        assert (m.sum(axis=1) == k).all()
        assert (m[:, req] == 1).all()
        hits += m.sum(axis=0)
    assert hits[free].sum() == 6 * B * (k - len(req))
    assert (hits[free] > 0).mean() > 0.8             # the sampled part spreads over the non-required nodes
    # and without a required list, the same masks as the training sampler
    counter = torch.tensor([4], dtype=torch.int64, device="cuda:0")
    ref = torch.empty(B * n, dtype=torch.uint8, device="cuda:0")
    pkg._native.check(lib.gatres_mask_generate(node_ptr(B, n).data_ptr(), B, rate, 99, counter.data_ptr(), ref.data_ptr(),
                                               pkg._native.current_stream(ref.device)), "gatres_mask_generate")
    assert torch.equal(stage_required(pkg, lib, B, rate, 99, 4, [], n=n).reshape(-1), ref)


def test_required_count_at_or_above_the_mask_length_is_refused(pkg, lib):
    rate = 0.02                                       # int(388 * 0.02) = 7
    stage_required(pkg, lib, 2, rate, 1, 0, SENSORS)  # 6 < 7: fine
    with pytest.raises(RuntimeError, match="BADARG"):
        stage_required(pkg, lib, 2, rate, 1, 0, SENSORS + [5])
    st = make_store(pkg, 8)
    with pytest.raises(ValueError, match="mask length"):
        pkg.evaluation.evaluate_store(make_model(pkg, 2, 8, 0), st, 4, rate, do_test_on_sensors=True,
                                      required_idx=SENSORS + [5])


def test_training_masks_unchanged_without_required_nodes(pkg, lib):
    B, rate, seed = 16, 0.95, 77
    for step in (0, 5, 123456):
        counter = torch.tensor([step], dtype=torch.int64, device="cuda:0")
        ref = torch.empty(B * NODES, dtype=torch.uint8, device="cuda:0")
        pkg._native.check(lib.gatres_mask_generate(node_ptr(B).data_ptr(), B, rate, seed, counter.data_ptr(), ref.data_ptr(),
                                                   pkg._native.current_stream(ref.device)), "gatres_mask_generate")
        got = stage_required(pkg, lib, B, rate, seed, step, [])
        assert torch.equal(got.reshape(-1), ref)


# ---- the moments kernel --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale,offset", [(12.81, 51.37), (12.81, 0.0)])
def test_moments_kernel_record_counts_exact_and_deterministic(pkg, lib, scale, offset):
    E = pkg.evaluation
    g = torch.Generator().manual_seed(3)
    N = 32 * NODES
    y = torch.randn(N, generator=g)
    out = y + 0.08 * torch.randn(N, generator=g)
    y[:50] = 0.0                                      # offset 0: some |t| <= 0.01, not kept
    mask = (torch.rand(N, generator=g) < 0.95)
    d_out, d_y, d_m = out.cuda(), y.cuda(), mask.to(torch.uint8).cuda()
    table = torch.zeros((3, E.METRICS_RECORD), dtype=torch.float64, device="cuda:0")
    cursor = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    s = pkg._native.current_stream(d_out.device)
    for _ in range(2):                                # slots 0 and 1 through the cursor ...
        pkg._native.check(lib.gatres_masked_metrics(d_out.data_ptr(), d_y.data_ptr(), d_m.data_ptr(), N, scale, offset,
                                                    table.data_ptr(), 0, 3, cursor.data_ptr(), s), "gatres_masked_metrics")
    pkg._native.check(lib.gatres_masked_metrics(d_out.data_ptr(), d_y.data_ptr(), d_m.data_ptr(), N, scale, offset,
                                                table.data_ptr(), 2, 3, None, s), "gatres_masked_metrics")    # ... slot 2 directly
    T = table.cpu().numpy()
    assert int(cursor.item()) == 2
    assert T[0].tobytes() == T[1].tobytes() == T[2].tobytes()          # fixed-order reduction: the same bits every run
    ref = MR.masked_metric_moments(out.numpy(), y.numpy(), mask.numpy(), scale, offset)
    # torch on the device, as test_one_epoch computes it
    m = d_m.bool()
    p = E.descale(d_out[m], "znorm", mean=offset, std=scale)
    t = E.descale(d_y[m], "znorm", mean=offset, std=scale)
    assert T[0][0] == int(m.sum())
    assert T[0][9] == int((t.abs() > 0.01).sum()) == ref[9]
    assert T[0][11] == int(((t - p).abs() <= t * 0.1).sum()) == ref[11]
    np.testing.assert_allclose(T[0], ref, rtol=1e-9, atol=1e-9)


# ---- the epoch against the host loop -------------------------------------------------------------------------------------
def host_metrics(pkg, model, store, caps, prefix="test"):
    """test_one_epoch's per-batch arithmetic on the device masks: the model call on x1 with x1[mask] = 0, MSELoss on scaled
    values, the reference's functions on descaled values, weighted by graph count.  Also checks the predictions bitwise."""
    E = pkg.evaluation
    fns = E.get_metric_fn_collection(prefix)
    total_loss, total, n = 0.0, {k: 0.0 for k in fns}, 0
    for mask, out, x, g in caps:
        m = mask.bool()
        y = x.reshape(-1, 1)
        x1 = y.clone()
        x1[m] = 0
        with torch.no_grad():
            o = model(x1, store.edge_index(g))
        assert torch.equal(o, out), "predictions differ from model(x1, edge_index)"
        yp, yt = o[m], y[m]
        pr = E.descale(yp, store.norm_type, mean=store.mean, std=store.std)
        tr = E.descale(yt, store.norm_type, mean=store.mean, std=store.std)
        total_loss += float(torch.nn.MSELoss()(yp, yt)) * g
        for k, fn in fns.items():
            total[k] += float(fn(pr, tr)) * g
        n += g
    return total_loss / n, {k: v / n for k, v in total.items()}


def check_epoch(pkg, model, store, bs, rate, prefix="test", **kw):
    E = pkg.evaluation
    caps = []
    loss, m = E.evaluate_store(model, store, bs, rate, prefix=prefix, gpu_warmup_times=2, _capture=caps, **kw)
    sizes = [c[3] for c in caps]
    assert sum(sizes) == len(store) and sizes == [min(bs, len(store) - i * bs) for i in range(len(sizes))]
    npg = store.nodes_per_graph
    req = sorted(set(kw.get("required_idx", ()))) if kw.get("do_test_on_sensors") else []
    for b, (mask, _, x, g) in enumerate(caps):
        assert torch.equal(x, store.data[b * bs: b * bs + g].reshape(-1))     # the staging launch collated these rows
        mm = mask.view(g, npg)
        assert (mm.sum(dim=1) == int(npg * rate)).all()
        if req:
            assert (mm[:, req] == 1).all()
    h_loss, h_m = host_metrics(pkg, model, store, caps, prefix)
    post = "_sensor" if kw.get("do_test_on_sensors") else ""
    assert list(m) == [k + post for k in E.get_metric_fn_collection(prefix)] + [f"{prefix}_time{post}", f"{prefix}_throughput{post}"]
    assert loss == pytest.approx(h_loss, rel=1e-5)
    for k, v in h_m.items():
        got = m[k + post]
        if math.isnan(v):
            assert math.isnan(got), k
        else:
            assert got == pytest.approx(v, rel=1e-5, abs=1e-7), k
    assert m[f"{prefix}_time{post}"] > 0 and m[f"{prefix}_throughput{post}"] > 0
    return loss, m, caps


def test_gatres_small_fp32_window_kernel_with_ragged_tail(pkg):
    st = make_store(pkg, 70)
    model = make_model(pkg, 15, 32, seed=11)
    plan = model.plan_for(st.edge_index(32), 32 * NODES)
    assert model._call_state(plan)["window"], "gatres_small at bs 32 should take the window kernel"
    check_epoch(pkg, model, st, 32, 0.95)


def test_per_op_configuration(pkg):
    st = make_store(pkg, 20, seed=4)
    model = make_model(pkg, 4, 16, seed=12, fused=False)
    check_epoch(pkg, model, st, 8, 0.9, prefix="val")


def test_bf16_gatres_large_small_batch(pkg):
    st = make_store(pkg, 5, seed=5)
    model = make_model(pkg, 25, 128, seed=13, dtype="bf16")
    check_epoch(pkg, model, st, 2, 0.95)


def test_sensor_pass_and_same_mask(pkg):
    st = make_store(pkg, 40, seed=6)
    model = make_model(pkg, 15, 32, seed=14)
    _, m, caps = check_epoch(pkg, model, st, 16, 0.95, do_test_on_sensors=True, required_idx=SENSORS, seed=9)
    assert all(k.endswith("_sensor") for k in m)
    _, _, caps = check_epoch(pkg, model, st, 16, 0.95, use_same_mask=True, seed=9)
    assert torch.equal(caps[0][0], caps[1][0])                   # full batches share one mask ...
    assert caps[2][0].numel() != caps[0][0].numel()              # ... the ragged one has its own
    _, _, caps2 = check_epoch(pkg, model, st, 16, 0.95, seed=9)
    assert not torch.equal(caps2[0][0], caps2[1][0])             # without use_same_mask every batch draws afresh


def test_same_seed_same_result(pkg):
    st = make_store(pkg, 33, seed=7)
    model = make_model(pkg, 15, 32, seed=15)
    a = pkg.evaluation.evaluate_store(model, st, 16, 0.95, seed=3, gpu_warmup_times=0)
    b = pkg.evaluation.evaluate_store(model, st, 16, 0.95, seed=3, gpu_warmup_times=0)
    c = pkg.evaluation.evaluate_store(model, st, 16, 0.95, seed=4, gpu_warmup_times=0)
    strip = lambda r: (r[0], {k: v for k, v in r[1].items() if not k.endswith(("_time", "_throughput"))})
    assert strip(a) == strip(b)
    assert strip(a) != strip(c)


def test_evaluate_store_trials(pkg):
    st = make_store(pkg, 24, seed=8)
    model = make_model(pkg, 15, 32, seed=16)
    losses, m, s_losses, s_m = pkg.evaluation.evaluate_store_trials(model, st, 16, 2, 0.95, required_idx=SENSORS, seed=5,
                                                                    gpu_warmup_times=1)
    assert len(losses) == len(s_losses) == 2
    assert losses[0] != losses[1] and losses[0] != s_losses[0]     # every pass draws masks of its own
    assert set(m) == {k for k in pkg.evaluation.get_metric_fn_collection("test")} | {"test_time", "test_throughput"}
    assert set(s_m) == {k + "_sensor" for k in m}
    assert all(len(v) == 2 for v in list(m.values()) + list(s_m.values()))


def test_one_synchronisation_per_epoch(pkg, monkeypatch):
    st = make_store(pkg, 70, seed=9)
    model = make_model(pkg, 15, 32, seed=17)
    E = pkg.evaluation
    E.evaluate_store(model, st, 32, 0.95, gpu_warmup_times=1)         # plans and buffers exist from here on
    torch.cuda.synchronize()
    calls = {"synchronize": 0, "item": 0, "cpu": 0, "tolist": 0, "float": 0, "stream_sync": 0, "event_sync": 0}

    def spy(name, fn):
        def wrapped(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return wrapped

    monkeypatch.setattr(torch.cuda, "synchronize", spy("synchronize", torch.cuda.synchronize))
    monkeypatch.setattr(torch.Tensor, "item", spy("item", torch.Tensor.item))
    monkeypatch.setattr(torch.Tensor, "cpu", spy("cpu", torch.Tensor.cpu))
    monkeypatch.setattr(torch.Tensor, "tolist", spy("tolist", torch.Tensor.tolist))
    monkeypatch.setattr(torch.Tensor, "__float__", spy("float", torch.Tensor.__float__))
    monkeypatch.setattr(torch.cuda.Stream, "synchronize", spy("stream_sync", torch.cuda.Stream.synchronize))
    monkeypatch.setattr(torch.cuda.Event, "synchronize", spy("event_sync", torch.cuda.Event.synchronize))
    loss, m = E.evaluate_store(model, st, 32, 0.95, gpu_warmup_times=1)
    assert calls == {"synchronize": 1, "item": 0, "cpu": 1, "tolist": 0, "float": 0, "stream_sync": 0, "event_sync": 0}
    assert math.isfinite(loss) and math.isfinite(m["test_mae"])
