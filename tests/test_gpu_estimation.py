"""Pressure estimation on the device (estimation.PressureEstimator, k_estimate.hip): the staging and write-back launches bit
for bit against torch statements, the readings layout against the store's own normalisation, the pass against a hand-written
loop / the module / the oracle, the back-test report against fp64 numpy, and the passes' freedom from synchronisation.

Shapes: graphs of 37 nodes (no multiple of 4 or 64: every chunk alignment of the element kernels, one partial wave of the
moments kernel) in batches of 3 over 7 snapshots (3, 3 and a ragged 1); 40 nodes where a kernel takes another path for rows that
are multiples of four; 388 nodes once, for gatres_small at batch size 32 on the window kernel."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from estimation_refs import garbage, torch_stage      # noqa: E402,F401
from test_gpu_model import build, relerr      # noqa: E402

DEV = "cuda:0"
N37, PIPES37 = 37, 41
OBS = [36, 0, 5]                                  # unsorted on purpose: column k of the readings is node OBS[k]
_CACHE = {}


def topology(pkg, n=N37, pipes=PIPES37):
    key = ("ei", n, pipes)
    if key not in _CACHE:
        _CACHE[key] = pkg.wdn_synth.make_wdn_topology(n, pipes, seed=0)
    return _CACHE[key]


def raw_snapshots(pkg, S, n=N37, seed=1):
    return pkg.wdn_synth.make_snapshots(S, n, seed=seed) * 12.5 + 50.0      # pressures around 50 m


def make_store(pkg, S, n=N37, pipes=PIPES37, seed=1, **kw):
    return pkg.SnapshotStore(raw_snapshots(pkg, S, n, seed), topology(pkg, n, pipes), device=DEV, **kw)


def small_model(pkg, oracle, nb=2, nc=8, fused=True, dtype="fp32", seed=3):
    model, p = build(pkg, oracle, nb, nc, seed=seed, fused=fused)
    if dtype != "fp32":
        model.set_compute_dtype(dtype)
    return model, p


def stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def stage(pkg, lib, src, layout, rows, first, n, g, observed, normalise=0, offset=0.0, factor=1.0):
    x, mask = garbage(g * n)
    obs = torch.tensor(observed, dtype=torch.int32, device=DEV)
    pkg._native.check(lib.gatres_stage_observed(src.data_ptr(), layout, src.shape[0], pkg._native.ptr(rows), first, n, g,
                                                obs.data_ptr(), len(observed), normalise, offset, factor, x.data_ptr(),
                                                mask.data_ptr(), stream()), "gatres_stage_observed")
    return x, mask


# ---- 1. staging --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("observed", [OBS, [17], [v for v in range(N37) if v != 20]], ids=["K3", "K1", "K36"])
def test_staging_full_rows_bitwise(pkg, lib, observed):
    S, bs = 7, 3
    store = make_store(pkg, S)
    perm = torch.tensor([4, 0, 6, 2, 5, 1, 3], dtype=torch.int64, device=DEV)
    for first in range(0, S, bs):
        g = min(bs, S - first)
        # in store order, by first_row
        x, mask = stage(pkg, lib, store.data, 0, None, first, N37, g, observed)
        ex, em = torch_stage(store.data[first:first + g][:, observed], N37, observed)
        assert torch.equal(x, ex) and torch.equal(mask, em), first
        # by a rows array (a permutation of the store); first_row is then ignored
        rows = perm[first:first + g].contiguous()
        x, mask = stage(pkg, lib, store.data, 0, rows, 5, N37, g, observed)
        ex, em = torch_stage(store.data[rows][:, observed], N37, observed)
        assert torch.equal(x, ex) and torch.equal(mask, em), first


def test_staging_rows_that_are_multiples_of_four_and_unaligned_targets(pkg, lib):
    """40 nodes: every chunk of every graph is whole.  A target that starts one float past a 16-byte boundary takes the
    element-by-element stores."""
    n, g = 40, 3
    store = make_store(pkg, 4, n=n, pipes=45)
    observed = [39, 3, 4, 5, 0]
    x, mask = stage(pkg, lib, store.data, 0, None, 1, n, g, observed)
    ex, em = torch_stage(store.data[1:4][:, observed], n, observed)
    assert torch.equal(x, ex) and torch.equal(mask, em)
    xb, mb = garbage(g * N37 + 4)
    st37 = make_store(pkg, 3)
    obs = torch.tensor(OBS, dtype=torch.int32, device=DEV)
    pkg._native.check(lib.gatres_stage_observed(st37.data.data_ptr(), 0, 3, None, 0, N37, g, obs.data_ptr(), 3, 0, 0.0, 1.0,
                                                xb.data_ptr() + 4, mb.data_ptr() + 1, stream()), "gatres_stage_observed")
    ex, em = torch_stage(st37.data[:, OBS], N37, OBS)
    assert torch.equal(xb[1:1 + g * N37], ex) and torch.equal(mb[1:1 + g * N37], em)
    assert torch.isnan(xb[0]) and torch.isnan(xb[1 + g * N37:]).all() and int(mb[0]) == 0xAB      # nothing outside the batch


# ---- 2. the readings layout -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", [True, False], ids=["znorm", "unused"])
def test_readings_layout_equals_the_stores_normalisation_bitwise(pkg, lib, oracle, normalize):
    S = 7
    raw = raw_snapshots(pkg, S)
    store = pkg.SnapshotStore(raw, topology(pkg), device=DEV, normalize=normalize)
    model, _ = small_model(pkg, oracle)
    est = pkg.PressureEstimator.for_store(model, store, OBS, batch_size=3)
    readings = raw.to(DEV)[:, OBS].contiguous()
    # the staged inputs themselves ...
    factor = store.std + 1e-8 if normalize else 1.0
    x, mask = stage(pkg, lib, readings, 1, None, 2, N37, 3, OBS, est._normalise, store.mean if normalize else 0.0, factor)
    ex, em = torch_stage(store.data[2:5][:, OBS], N37, OBS)
    assert torch.equal(x, ex) and torch.equal(mask, em)
    # ... and the two passes
    a, b = est.estimate(readings), est.estimate_store(store)
    assert a.shape == (S, N37) and torch.equal(a, b)
    assert torch.isfinite(a).all()


# ---- 3. write-back ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,stride", [(37, 40), (40, 44), (40, 41)], ids=["odd", "vector_rows", "odd_stride"])
@pytest.mark.parametrize("keep", [1, 0])
def test_write_back_bitwise(pkg, lib, n, stride, keep):
    g, first, rows = 3, 2, 7
    scale, offset = 12.81, 51.37
    gen = torch.Generator().manual_seed(n + stride + keep)
    out = torch.randn(g * n, generator=gen).to(DEV)
    x = torch.randn(g * n, generator=gen).to(DEV)
    mask = (torch.rand(g * n, generator=gen) < 0.7).to(torch.uint8).to(DEV)
    dst = torch.full((rows, stride), -777.25, dtype=torch.float32, device=DEV)
    pkg._native.check(lib.gatres_estimate_write(out.data_ptr(), x.data_ptr(), mask.data_ptr(), n, g, scale, offset, keep,
                                                dst.data_ptr(), rows, stride, first, stream()), "gatres_estimate_write")
    want = torch.where(mask.bool(), out * scale + offset, x * scale + offset) if keep else out * scale + offset
    assert torch.equal(dst[first:first + g, :n], want.view(g, n))
    dst[first:first + g, :n] = -777.25
    assert (dst == -777.25).all()                                  # the other rows and the columns past n stay untouched


# ---- 4. the pass ------------------------------------------------------------------------------------------------------------------
def hand_loop(pkg, model, store, observed, bs, keep_observed=True):
    """The pass written out: staging with torch, the forward through the estimator's plan and entry on the torch-filled
    buffers, ``store.descale``.  Returns (estimates [S, N], per batch (x1, scaled predictions, graphs))."""
    E = pkg.evaluation
    lib = pkg._native.load()
    n, S = store.nodes_per_graph, len(store)
    res = torch.empty((S, n), dtype=torch.float32, device=DEV)
    batches = []
    for first in range(0, S, bs):
        g = min(bs, S - first)
        P = E._eval_plan(model, store, g)
        x1, mask = torch_stage(store.data[first:first + g][:, observed], n, observed)
        P.x.copy_(x1)
        P.mask.copy_(mask)
        E._enqueue_forward(lib, model.flat_parameters, P, stream())
        pred = P.out.clone().reshape(-1)
        m = mask.bool()
        merged = torch.where(m, store.descale(pred), store.descale(x1)) if keep_observed else store.descale(pred)
        res[first:first + g] = merged.view(g, n)
        batches.append((x1, pred, g))
    return res, batches


def check_against_module(pkg, model, store, batches, bf16=False):
    for x1, pred, g in batches:
        with torch.no_grad():
            o = model(x1.view(-1, 1), store.edge_index(g)).reshape(-1)
        if bf16:         # test_gpu_bf16.py's forward bounds: 1e-2 in the L2 norm, 2.5e-2 at the worst node
            e_l2 = float((pred.double() - o.double()).norm() / o.double().norm())
            print("bf16 pass vs module: rel-L2", e_l2, "max-norm", relerr(pred, o))
            assert e_l2 < 1e-2 and relerr(pred, o) < 2.5e-2
        else:
            print("pass vs module: relerr", relerr(pred, o))
            assert relerr(pred, o) < 1e-5


def check_against_oracle(oracle, p, nb, store, batches):
    for x1, pred, g in batches:
        ref = oracle.gatres_forward(p, x1.view(-1, 1).cpu(), store.edge_index(g).cpu(), num_blocks=nb).reshape(-1)
        print("pass vs oracle: relerr", relerr(pred, ref))
        assert relerr(pred, ref) < 1e-5


@pytest.mark.parametrize("fused,keep", [(True, True), (False, True), (True, False)], ids=["fused", "per_op", "fused_predictions"])
def test_pass_equals_the_hand_written_loop_fp32(pkg, oracle, fused, keep):
    store = make_store(pkg, 7)
    model, p = small_model(pkg, oracle, fused=fused)
    est = pkg.PressureEstimator.for_store(model, store, OBS, batch_size=3, keep_observed=keep)
    got = est.estimate_store(store)
    want, batches = hand_loop(pkg, model, store, OBS, 3, keep)
    assert [b[2] for b in batches] == [3, 3, 1]
    assert torch.equal(got, want)
    if keep:             # the sensors' own values come back through the descale round trip
        assert torch.equal(got[:, OBS], store.descale(store.data[:, OBS]))
    check_against_module(pkg, model, store, batches)
    check_against_oracle(oracle, p, 2, store, batches)


def test_pass_equals_the_hand_written_loop_bf16(pkg, oracle):
    store = make_store(pkg, 7)
    model, _ = small_model(pkg, oracle, nb=2, nc=32, dtype="bf16")
    est = pkg.PressureEstimator.for_store(model, store, OBS, batch_size=3)
    got = est.estimate_store(store)
    want, batches = hand_loop(pkg, model, store, OBS, 3)
    assert torch.equal(got, want)
    check_against_module(pkg, model, store, batches, bf16=True)


def test_gatres_small_at_batch_32_takes_the_window_kernel(pkg, oracle):
    n, pipes, S = 388, 430, 40
    store = make_store(pkg, S, n=n, pipes=pipes, seed=4)
    model, p = small_model(pkg, oracle, nb=15, nc=32, seed=11)
    plan = model.plan_for(store.edge_index(32), 32 * n)
    assert model._call_state(plan)["window"], "gatres_small at bs 32 should take the window kernel"
    sensors = [3, 17, 100, 101, 250, 387, 42, 9, 300, 77, 211, 5, 64, 128, 199, 350, 1, 260, 333, 150]
    est = pkg.PressureEstimator.for_store(model, store, sensors, batch_size=32)
    got = est.estimate_store(store)
    want, batches = hand_loop(pkg, model, store, sensors, 32)
    assert [b[2] for b in batches] == [32, 8]
    assert torch.equal(got, want)
    check_against_module(pkg, model, store, batches)
    check_against_oracle(oracle, p, 15, store, batches[1:])          # (the ragged batch: 8 graphs on the host)


def test_from_checkpoint_and_the_plain_constructor_give_the_same_estimates(pkg, oracle, tmp_path):
    store = make_store(pkg, 4)
    model, _ = small_model(pkg, oracle)
    want = pkg.PressureEstimator.for_store(model, store, OBS, batch_size=3).estimate_store(store)
    path = str(tmp_path / "best.pth")
    pkg.wdn_io.save_checkpoint(path, model_state_dict=model.state_dict(), mean=store.mean, std=store.std, norm_type="znorm")
    fresh = pkg.GATResMeanConv(num_blocks=2, nc=8).cuda()
    est = pkg.PressureEstimator.from_checkpoint(fresh, path, topology(pkg), N37, OBS, batch_size=3)
    assert est.mean == store.mean and est.std == store.std and est.norm_type == "znorm"
    assert torch.equal(est.estimate_store(store), want)
    out = torch.empty_like(want)
    assert est.estimate(raw_snapshots(pkg, 4).to(DEV)[:, OBS].contiguous(), out=out) is out and torch.equal(out, want)


def test_refusals_on_the_device(pkg, oracle):
    store = make_store(pkg, 4)
    model, _ = small_model(pkg, oracle)
    est = pkg.PressureEstimator.for_store(model, store, OBS)
    good = torch.zeros((4, 3), dtype=torch.float32, device=DEV)
    for bad in (good.cpu(), good.double(), good[:, :2], torch.zeros((4, 6), device=DEV)[:, ::2], good.reshape(-1), good[:0]):
        with pytest.raises(ValueError, match="readings"):
            est.estimate(bad)
    with pytest.raises(ValueError, match="out must"):
        est.estimate(good, out=torch.empty((4, N37 + 1), device=DEV))
    with pytest.raises(ValueError, match="nodes per graph"):
        est.estimate_store(make_store(pkg, 4, n=40, pipes=45))
    with pytest.raises(ValueError, match="mean / std"):
        est.estimate_store(make_store(pkg, 4, seed=9))
    with pytest.raises(ValueError, match="norm_type"):
        est.error_map(make_store(pkg, 4, normalize=False))


# ---- 5. hidden nodes ----------------------------------------------------------------------------------------------------------------
def test_hidden_nodes_never_leak(pkg, oracle):
    S = 7
    raw = raw_snapshots(pkg, S)
    store = pkg.SnapshotStore(raw, topology(pkg), device=DEV)
    other = raw.clone()
    hidden = [v for v in range(N37) if v not in OBS]
    other[:, hidden] = other[:, hidden] * -3.0 + 500.0
    changed = pkg.SnapshotStore(other, topology(pkg), device=DEV, mean=store.mean, std=store.std)
    assert torch.equal(changed.data[:, OBS], store.data[:, OBS]) and not torch.equal(changed.data, store.data)
    model, _ = small_model(pkg, oracle)
    est = pkg.PressureEstimator.for_store(model, store, OBS, batch_size=3)
    assert torch.equal(est.estimate_store(store), est.estimate_store(changed))


# ---- 6. the report ------------------------------------------------------------------------------------------------------------------
def moments_table(pkg, lib, est_m, truth, scale, offset, observed):
    n = truth.shape[1]
    obs = torch.tensor(observed, dtype=torch.int32, device=DEV)
    table = torch.full((n, 8), float("nan"), dtype=torch.float64, device=DEV)
    pkg._native.check(lib.gatres_node_error_moments(est_m.data_ptr(), truth.data_ptr(), truth.shape[0], n, scale, offset,
                                                    obs.data_ptr(), len(observed), table.data_ptr(), stream()),
                      "gatres_node_error_moments")
    return table.cpu().numpy()


@pytest.mark.parametrize("S", [1, 70, 65], ids=["S1", "S70", "one_past_the_chunk"])
@pytest.mark.parametrize("normalize", [True, False], ids=["znorm", "unused"])
def test_error_moments_and_error_map(pkg, lib, oracle, S, normalize):
    assert pkg._native.NODE_ERROR_CHUNK == 64
    raw = raw_snapshots(pkg, S, seed=S)
    if not normalize:
        raw = raw - 50.0
        raw[::2, 7] = 0.0                                          # some |t| <= 0.01 ...
        raw[:, 11] = 0.004                                         # ... and a node without any kept snapshot
    store = pkg.SnapshotStore(raw, topology(pkg), device=DEV, normalize=normalize)
    model, _ = small_model(pkg, oracle)
    est = pkg.PressureEstimator.for_store(model, store, OBS, batch_size=32)
    p = est.estimate_store(store)
    scale, offset = (store.std, store.mean) if normalize else (1.0, 0.0)
    T = moments_table(pkg, lib, p, store.data, scale, offset, OBS)
    assert T.tobytes() == moments_table(pkg, lib, p, store.data, scale, offset, OBS).tobytes()      # the same bits every run
    # the same fp32 e and t, formed by torch on the device
    t32 = store.descale(store.data)
    e32 = p - t32
    e, t = e32.double().cpu().numpy(), t32.double().cpu().numpy()
    keep = t32.abs() > 0.01
    assert (T[:, 0] == S).all()
    np.testing.assert_array_equal(T[:, 5], keep.sum(0).cpu().numpy())
    np.testing.assert_array_equal(T[:, 7], [1.0 if v in OBS else 0.0 for v in range(N37)])
    np.testing.assert_array_equal(T[:, 4], e32.abs().max(0).values.double().cpu().numpy())
    k = keep.cpu().numpy()
    np.testing.assert_allclose(T[:, 1], e.sum(0), rtol=1e-12, atol=0)
    np.testing.assert_allclose(T[:, 2], np.abs(e).sum(0), rtol=1e-12, atol=0)
    np.testing.assert_allclose(T[:, 3], (e * e).sum(0), rtol=1e-12, atol=0)
    np.testing.assert_allclose(T[:, 6], np.where(k, np.abs(e) / np.where(k, np.abs(t), 1.0), 0.0).sum(0), rtol=1e-12, atol=0)
    if not normalize:
        # (stated on the host from the fp32 input, which is t itself here: the zeroed rows of node 7 are not kept, and of the
        #  others those whose random value exceeds the threshold -- at S = 70 and 65 one of them does not)
        kept7 = int((raw[1::2, 7].abs() > 0.01).sum())
        assert T[11, 5] == 0 and T[7, 5] == kept7 <= S - (S + 1) // 2
    # the report: error_map on the same estimates, and on estimates it forms itself
    m = est.error_map(store, estimates=p)
    ref = pkg.estimation.error_map_from_moments(T)
    for key, v in ref.items():
        np.testing.assert_array_equal(m[key], v, err_msg=key)
    hidden = [v for v in range(N37) if v not in OBS]
    assert m["hidden_mae"] == pytest.approx(np.abs(e[:, hidden]).mean(), rel=1e-12)
    assert m["hidden_rmse"] == pytest.approx(np.sqrt((e[:, hidden] ** 2).mean()), rel=1e-12)
    np.testing.assert_allclose(m["mae"], np.abs(e).mean(0), rtol=1e-12)
    assert m["observed"].tolist() == [v in OBS for v in range(N37)]
    assert (m["max_abs"][OBS] <= 1e-4).all()                      # sensors: the descale round trip only
    if not normalize:
        assert np.isnan(m["rel_error"][11])
    m2 = est.error_map(store)
    for key in ref:
        np.testing.assert_array_equal(m2[key], m[key], err_msg=key)


# ---- 7. synchronisation ---------------------------------------------------------------------------------------------------------------
def test_no_read_back_in_the_passes_and_one_in_error_map(pkg, oracle, monkeypatch):
    store = make_store(pkg, 7)
    model, _ = small_model(pkg, oracle)
    est = pkg.PressureEstimator.for_store(model, store, OBS, batch_size=3)
    readings = raw_snapshots(pkg, 7).to(DEV)[:, OBS].contiguous()
    est.estimate_store(store)                                       # plans and buffers exist from here on
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
    a = est.estimate_store(store)
    b = est.estimate(readings)
    assert all(v == 0 for v in calls.values()), calls
    m = est.error_map(store, estimates=a)
    assert calls == {"synchronize": 0, "item": 0, "cpu": 1, "tolist": 0, "float": 0, "stream_sync": 0, "event_sync": 0}
    monkeypatch.undo()
    assert torch.equal(a, b) and np.isfinite(m["hidden_mae"])
