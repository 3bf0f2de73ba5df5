"""The screening of sensor readings on the device (PressureEstimator.loo_residuals / calibrate_screening / screen /
estimate_screened / screening_report; k_screen.hip): the two launches bit for bit against their numpy statements, called directly
into garbage-filled, padded buffers; the leave-one-out pass bit for bit against ``reading_residuals``, whose K passes it replaces;
the calibration against ``node_error_bounds`` and against K ``calibrate_bounds`` calls; ``screen`` / ``estimate_screened`` against
the pass written out; an exact end-to-end case that rests on locality (sensors more than 3 hops apart under one block); the
back-test against its four passes written out; read-backs and allocations counted; the refusals.

Shapes: graphs of 37 and 40 nodes with 8 sensors in batches of 4, so every batch straddles snapshots; K and G around the lane
count and the block size of the two launches, one launch each past its grid cap; 388 nodes once for gatres_small on the window
kernel.  A float matrix is compared bit for bit, but for the payload of a NaN that an arithmetic operation made
(``screening_refs.same_floats``)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import screening_refs as SR      # noqa: E402
import sensitivity_refs as R      # noqa: E402
import turnover_cases as T      # noqa: E402
from estimation_refs import DEV, numpy_descale      # noqa: E402
from test_gpu_model import build, note      # noqa: E402

PAD = 4                       # elements of garbage in front of and behind every target
FILL = -777.25
OBS8 = [36, 0, 5, 17, 22, 9, 30, 13]
SENSORS388 = [3, 17, 100, 101, 250, 387, 42, 9, 300, 77, 211, 5, 64, 128, 199, 350, 1, 260, 333, 150]
_CACHE = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def host(t):
    return t.detach().cpu().numpy()


def topology(pkg, n, pipes):
    key = ("ei", n, pipes)
    if key not in _CACHE:
        _CACHE[key] = pkg.wdn_synth.make_wdn_topology(n, pipes, seed=0)
    return _CACHE[key]


def raw_snapshots(pkg, S, n, seed=1):
    return pkg.wdn_synth.make_snapshots(S, n, seed=seed) * 12.5 + 50.0


def make_store(pkg, S, n, pipes, seed=1, **kw):
    return pkg.SnapshotStore(raw_snapshots(pkg, S, n, seed), topology(pkg, n, pipes), device=DEV, **kw)


def readings_of(pkg, S, n, observed, seed=1):
    return raw_snapshots(pkg, S, n, seed).to(DEV)[:, observed].contiguous()


# ---- 1. gatres_loo_residuals ------------------------------------------------------------------------------------------------------
def loo_case(pkg, lib, N, K, G, full_rows, znorm, with_available, nan_is_missing, first=None):
    """One launch into garbage-filled pred / resid that start PAD elements into their allocations, against the numpy statement.
    The batch starts in the middle of a snapshot and, with more graphs than sensors left in it, straddles snapshots.  Planted:
    a NaN reading, an unavailable reading, a pair whose mask is 0 at its own sensor, a NaN prediction."""
    rng = np.random.default_rng(1000 * N + 10 * K + G + full_rows)
    first = K + 1 if first is None else first
    S = (first + G + K - 1) // K + 1                            # (one snapshot behind the batch: nothing of it is written)
    observed = [int(v) for v in rng.permutation(N)[:K]]
    out = rng.standard_normal((G, N)).astype(np.float32)
    mask = (rng.random((G, N)) < 0.5).astype(np.uint8)
    p = first + np.arange(G)
    s, k = p // K, p % K
    mask[np.arange(G), np.asarray(observed)[k]] = 1             # a pair hides its own sensor ...
    src = rng.standard_normal((S, N)).astype(np.float32) if full_rows else \
        (rng.standard_normal((S, K)) * 12.5 + 50.0).astype(np.float32)
    available = (rng.random((S, K)) < 0.8).astype(np.uint8) if with_available else None
    g_nan, g_gone, g_seen, g_bad = 0, G // 2, G - 1, G // 3
    if full_rows:
        src[s[g_nan], observed[k[g_nan]]] = np.float32("nan")
    else:
        src[s[g_nan], k[g_nan]] = np.float32("nan")
    if with_available:
        available[s[g_nan], k[g_nan]] = 1
        if G > 1:
            available[s[g_gone], k[g_gone]] = 0
    if G > 2:
        mask[g_seen, observed[k[g_seen]]] = 0                   # ... but for this one
    if G > 3:
        out[g_bad, observed[k[g_bad]]] = np.float32("nan")
    scale, offset = (12.81, 50.3) if znorm else (1.0, 0.0)
    pred = torch.full((S * K + 2 * PAD,), FILL, dtype=torch.float32, device=DEV)
    resid = torch.full((S * K + 2 * PAD,), FILL, dtype=torch.float32, device=DEV)
    d = [dev(out), dev(mask), dev(src), dev(np.asarray(observed, dtype=np.int32)), None if available is None else dev(available)]
    pkg._native.check(lib.gatres_loo_residuals(
        d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), 0 if full_rows else 1, S, first, N, G, d[3].data_ptr(), K, scale, offset,
        pkg._native.ptr(d[4]), nan_is_missing, pred.data_ptr() + 4 * PAD, resid.data_ptr() + 4 * PAD, stream()),
        "gatres_loo_residuals")
    fill = np.full((S, K), np.float32(FILL))
    want_pred, want_resid = SR.numpy_loo_residuals(pkg, out, mask, src, full_rows, N, K, first, observed, scale, offset, available,
                                                   nan_is_missing, fill, fill)
    got_pred, got_resid = host(pred), host(resid)
    what = f"N{N} K{K} G{G} full{full_rows} znorm{znorm} av{with_available} nan{nan_is_missing}"
    for got, want in ((got_pred, want_pred), (got_resid, want_resid)):
        assert (got[:PAD] == np.float32(FILL)).all() and (got[-PAD:] == np.float32(FILL)).all(), what
        SR.same_floats(got[PAD:-PAD].reshape(S, K), want, what)
    body = got_resid[PAD:-PAD].view(np.uint32)
    assert np.isnan(got_resid[PAD + p[g_nan]]), what            # a NaN reading: a NaN, flagged as missing or not
    if nan_is_missing:
        assert body[p[g_nan]] == SR.NAN_BITS, what
    if with_available and G > 1:
        assert body[p[g_gone]] == SR.NAN_BITS and not np.isnan(got_pred[PAD + p[g_gone]]), what
    if G > 2:
        assert body[p[g_seen]] == SR.NAN_BITS and not np.isnan(got_pred[PAD + p[g_seen]]), what
    if G >= 4:
        assert np.isfinite(got_resid[PAD + p]).sum() >= G // 2, what          # (and numbers, too)
    return got_resid[PAD:-PAD].reshape(S, K)


@pytest.mark.parametrize("G", SR.LOO_G)
@pytest.mark.parametrize("K", SR.LOO_K)
def test_loo_residuals_bitwise(pkg, lib, K, G):
    for full_rows in (0, 1):
        for znorm in (True, False):
            for with_available, nan_is_missing in ((False, 0), (True, 0), (False, 1), (True, 1)):
                loo_case(pkg, lib, 37, K, G, full_rows, znorm, with_available, nan_is_missing)
    loo_case(pkg, lib, 37, K, G, 0, True, True, 1, first=0)     # from the very first pair


def test_loo_residuals_above_the_grid_cap(pkg, lib):
    c = SR.LOO_CAPPED
    assert c["G"] > SR.grid_cap("gatres_loo_residuals") * SR.constants()["LR_T"]
    for full_rows in (0, 1):
        got = loo_case(pkg, lib, c["N"], c["K"], c["G"], full_rows, True, True, 0)
        assert np.isfinite(got).sum() > c["G"] // 2


# ---- 2. gatres_screen_reject ------------------------------------------------------------------------------------------------------
def reject_inputs(S, K):
    rng = np.random.default_rng(100 * S + K)
    bound = rng.choice(np.float32([0.5, 1.0, 2.0, 4.0]), size=K).astype(np.float32)
    resid = (rng.standard_normal((S, K)) * 2).astype(np.float32)
    if K >= 7:
        bound[0], bound[1], bound[3], bound[4], bound[5] = 1.0, 2.0, 0.0, np.inf, np.nan
        resid[::3, 0] *= 8
        resid[::3, 1] = -2 * resid[::3, 0]                      # equal scores, and large ones, at k = 0 and 1
        resid[:, 3] = np.where(rng.random(S) < 0.5, np.float32(0.0), np.float32(-0.0))      # at a zero bound: no candidates ...
        resid[::5, 3] = 1e-20                                   # ... but these, whose score is +inf
        resid[::4, 4] = np.inf                                  # an infinite residual never exceeds an infinite bound
    else:
        bound[:] = [1.0, 2.0]
        resid[::3, 1] = -2 * resid[::3, 0]
    holes = rng.random((S, K))
    resid[holes < 0.05] = np.nan
    resid[(holes >= 0.05) & (holes < 0.08)] = np.inf
    resid[(holes >= 0.08) & (holes < 0.10)] = -np.inf
    avail = (rng.random((S, K)) < 0.9).astype(np.uint8)
    avail[::2] = 1                                              # every other snapshot has all its readings
    return resid, bound, avail


def reject_case(pkg, lib, S, K):
    resid, bound, avail = reject_inputs(S, K)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = (np.float32(1.0) / bound).astype(np.float32)
    d_resid, d_bound, d_inv = dev(resid), dev(bound), dev(inv)
    seen = set()
    for min_sensors in sorted({1, max(1, K - 1), K}):
        want_avail, want_rej, want_flag = pkg.screen_reject_ref(resid, bound, avail, min_sensors)
        seen.add(int((want_rej >= 0).sum()))
        for rnd in (0, 1):
            for with_flagged in (True, False):
                d_avail = torch.full((S * K + 2 * PAD,), 0xAB, dtype=torch.uint8, device=DEV)
                d_avail[PAD:PAD + S * K] = dev(avail).reshape(-1)
                rejected = torch.full((S * 2 + 2 * PAD,), -7, dtype=torch.int32, device=DEV)
                flagged = torch.full((S * K + 2 * PAD,), 0xAB, dtype=torch.uint8, device=DEV)
                pkg._native.check(lib.gatres_screen_reject(
                    d_resid.data_ptr(), d_bound.data_ptr(), d_inv.data_ptr(), d_avail.data_ptr() + PAD, S, K, min_sensors, rnd, 2,
                    rejected.data_ptr() + 4 * PAD, flagged.data_ptr() + PAD if with_flagged else None, stream()),
                    "gatres_screen_reject")
                what = f"S{S} K{K} min{min_sensors} round{rnd} flagged{with_flagged}"
                a, r, f = host(d_avail), host(rejected), host(flagged)
                for buf, fill in ((a, 0xAB), (r, -7), (f, 0xAB)):
                    assert (buf[:PAD] == fill).all() and (buf[-PAD:] == fill).all(), what
                np.testing.assert_array_equal(a[PAD:-PAD].reshape(S, K), want_avail, err_msg=what)
                r = r[PAD:-PAD].reshape(S, 2)
                np.testing.assert_array_equal(r[:, rnd], want_rej, err_msg=what)
                assert (r[:, 1 - rnd] == -7).all(), what        # the other round's column is untouched
                if with_flagged:
                    np.testing.assert_array_equal(f[PAD:-PAD].reshape(S, K), want_flag, err_msg=what)
                else:
                    assert (f == 0xAB).all(), what
    return seen, want_flag


@pytest.mark.parametrize("K", SR.REJECT_K)
@pytest.mark.parametrize("S", SR.REJECT_S)
def test_screen_reject_bitwise(pkg, lib, S, K):
    seen, flagged = reject_case(pkg, lib, S, K)
    assert 0 in seen                                            # min_sensors = K blocks every rejection
    if S > 1:
        assert max(seen) > 0 and flagged.sum() > 0


def test_screen_reject_above_the_grid_cap(pkg, lib):
    c = SR.REJECT_CAPPED
    assert c["S"] > SR.grid_cap("gatres_screen_reject") * SR.constants()["SR_WAVES"]
    seen, _ = reject_case(pkg, lib, c["S"], c["K"])
    assert max(seen) > c["S"] // 8


# ---- 3. the pass against reading_residuals ------------------------------------------------------------------------------------------
def never_flagging(pkg, n, observed):
    """An ``ErrorBounds`` whose bound is +inf at every node: ``reading_residuals`` with it flags nothing."""
    return pkg.ErrorBounds((0.9,), torch.full((1, n), float("inf"), device=DEV), torch.ones(n, dtype=torch.float64, device=DEV), observed)


def compare_with_reading_residuals(pkg, est, readings, n, observed, label, pairs_sizes):
    """``loo_residuals`` against the residuals of ``reading_residuals`` (its K passes of ``estimate``), without gaps and with
    NaN readings as gaps; ``available`` gives what the NaN readings give.  The figures are printed before they are judged."""
    S, K, bs = readings.shape[0], len(observed), est.batch_size
    assert [min(bs, S * K - f) for f in range(0, S * K, bs)] == pairs_sizes
    eb = never_flagging(pkg, n, observed)
    want, flagged = est.reading_residuals(readings, eb)
    resid, pred = est.loo_residuals(readings)
    assert resid.shape == (S, K) and pred.shape == (S, K) and resid.dtype == torch.float32 and not bool(flagged.any())
    got, want = host(resid).copy(), host(want)
    differ = int((got.view(np.int32) != want.view(np.int32)).sum())
    worst = float(np.abs(got.astype(np.float64) - want).max())
    print(f"{label}: loo_residuals against reading_residuals: {differ} of {got.size} entries differ in bits, largest "
          f"|difference| {worst:.3e} at |residual| up to {float(np.abs(want).max()):.3e}")
    note(f"screening {label}: entries of loo_residuals that differ from reading_residuals in bits / largest |difference|",
         [differ, worst])
    assert np.isfinite(want).all() and float(np.abs(want).max()) > 0
    np.testing.assert_array_equal(got.view(np.int32), want.view(np.int32))
    # with gaps
    av = T.availability(S, K, 0.3, seed=4)
    holed = readings.clone()
    holed[dev(av) == 0] = float("nan")
    want, _ = est.reading_residuals(holed, eb, nan_is_missing=True)
    got_nan = host(est.loo_residuals(holed, nan_is_missing=True)[0]).copy()
    got_av = host(est.loo_residuals(readings, available=dev(av))[0]).copy()
    want = host(want)
    differ = int(((got_nan.view(np.int32) != want.view(np.int32)) & ~np.isnan(want)).sum())
    print(f"{label}, with gaps: {differ} of {int((~np.isnan(want)).sum())} numbers differ in bits")
    assert np.isnan(want[av == 0]).all() and np.isfinite(want[av != 0]).all()
    SR.same_floats(got_nan, want, label)
    assert (got_nan.view(np.uint32)[av == 0] == SR.NAN_BITS).all() and (got_av.view(np.uint32)[av == 0] == SR.NAN_BITS).all()
    np.testing.assert_array_equal(got_av.view(np.int32), got_nan.view(np.int32))
    return got


@pytest.mark.parametrize("n,pipes,nc", [(37, 43, 8), (40, 47, 16)])
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "per_op"])
def test_pass_equals_reading_residuals_fp32(pkg, oracle, fused, n, pipes, nc):
    S, bs = 3, 4
    store = make_store(pkg, S, n, pipes)
    model, _ = build(pkg, oracle, 2, nc, seed=3, fused=fused)
    est = pkg.PressureEstimator.for_store(model, store, OBS8, batch_size=bs)
    readings = readings_of(pkg, S, n, OBS8)
    compare_with_reading_residuals(pkg, est, readings, n, OBS8, f"n{n} nc{nc} {'fused' if fused else 'per-op'}", [4] * 6)
    # the store entry point stages the same values (the store's normalisation, bit for bit): the same predictions, and the
    # residuals of its own readings, the store's values descaled
    _, pred = est.loo_residuals(readings)
    pred = pred.clone()
    resid_s, pred_s = est.loo_residuals_store(store)
    assert torch.equal(pred_s, pred)
    reading = numpy_descale(host(store.data)[:, OBS8], store.std, store.mean)
    want, _ = pkg.loo_residuals_from_estimates(reading, host(pred_s))
    np.testing.assert_array_equal(host(resid_s).view(np.int32), want.view(np.int32))


def test_pass_equals_reading_residuals_bf16(pkg, oracle):
    S, bs, n, pipes = 3, 4, 37, 43
    store = make_store(pkg, S, n, pipes)
    model, _ = build(pkg, oracle, 2, 32, seed=3, fused=False)
    model.set_compute_dtype("bf16")
    est = pkg.PressureEstimator.for_store(model, store, OBS8, batch_size=bs)
    compare_with_reading_residuals(pkg, est, readings_of(pkg, S, n, OBS8), n, OBS8, "n37 nc32 bf16 per-op", [4] * 6)


def test_gatres_small_at_batch_32_on_the_window_kernel(pkg, oracle):
    n, pipes, S = 388, 430, 3
    store = make_store(pkg, S, n, pipes, seed=4)
    model, _ = build(pkg, oracle, 15, 32, seed=11)
    plan = model.plan_for(store.edge_index(32), 32 * n)
    assert model._call_state(plan)["window"], "gatres_small at bs 32 should take the window kernel"
    est = pkg.PressureEstimator.for_store(model, store, SENSORS388, batch_size=32)
    compare_with_reading_residuals(pkg, est, readings_of(pkg, S, n, SENSORS388, seed=4), n, SENSORS388, "n388 gatres_small window",
                                   [32, 28])


# ---- 4. the calibration -----------------------------------------------------------------------------------------------------------
def calibration_case(pkg, oracle):
    if "cal" not in _CACHE:
        n, pipes, S = 37, 43, 24
        store = make_store(pkg, S, n, pipes, seed=7)
        model, _ = build(pkg, oracle, 2, 8, seed=3)
        est = pkg.PressureEstimator.for_store(model, store, OBS8, batch_size=4)
        _CACHE["cal"] = (store, model, est)
    return _CACHE["cal"]


@pytest.mark.parametrize("levels", [(0.9,), (0.5, 0.8, 0.9)])
@pytest.mark.parametrize("gaps", [False, True], ids=["complete", "gaps"])
def test_calibrate_screening_equals_node_error_bounds(pkg, oracle, levels, gaps):
    store, _, est = calibration_case(pkg, oracle)
    S, K = len(store), len(OBS8)
    av = T.availability(S, K, 0.3, seed=9) if gaps else None
    d_av = None if av is None else dev(av)
    sb = est.calibrate_screening(store, levels, available=d_av)
    assert isinstance(sb, pkg.ScreeningBounds) and sb.levels == levels and sb.observed_idx == OBS8
    assert sb.bounds.shape == (len(levels), K) and sb.bounds.device == torch.device(DEV) and sb.counts.shape == (K,)
    resid, pred = est.loo_residuals_store(store, available=d_av)
    reading = numpy_descale(host(store.data)[:, OBS8], store.std, store.mean)
    present = np.ones((S, K), dtype=bool) if av is None else av != 0
    want_b, want_c = pkg.node_error_bounds(host(pred), reading, levels, hidden=present)
    np.testing.assert_array_equal(host(sb.bounds).view(np.int32), want_b.view(np.int32))
    np.testing.assert_array_equal(host(sb.counts), want_c)
    # the same order statistic of |resid|, where the reading is there
    r = np.abs(host(resid))
    for k in range(K):
        col = np.sort(r[present[:, k], k])
        for q, level in enumerate(levels):
            rank = int(pkg.conformal_rank(col.size, level))
            assert host(sb.bounds)[q, k] == (col[rank - 1] if rank <= col.size else np.float32("inf"))
    if gaps:
        assert want_c[0] == 0 and np.isinf(host(sb.bounds)[:, 0]).all() and want_c[1] == S      # T.availability's sensors 0 and 1
    else:
        assert (want_c == S).all() and np.isfinite(want_b).all() and (want_b > 0).all()
    back = pkg.ScreeningBounds.from_state_dict(sb.state_dict(), device=DEV)
    assert torch.equal(back.bounds, sb.bounds) and torch.equal(back.counts, sb.counts) and back.device == torch.device(DEV)


def test_calibrate_screening_replaces_k_calibrate_bounds_calls(pkg, oracle):
    store, _, est = calibration_case(pkg, oracle)
    S, K = len(store), len(OBS8)
    got = host(est.calibrate_screening(store, (0.9,)).bounds)[0].copy()
    want = np.empty(K, dtype=np.float32)
    for k in range(K):
        a = torch.ones((S, K), dtype=torch.uint8, device=DEV)
        a[:, k] = 0
        want[k] = float(est.calibrate_bounds(store, (0.9,), available=a).bounds[0, OBS8[k]])
    print(f"calibrate_screening against K calibrate_bounds calls: {int((got.view(np.int32) != want.view(np.int32)).sum())} of {K} "
          f"bounds differ in bits, largest |difference| {float(np.abs(got.astype(np.float64) - want).max()):.3e}")
    np.testing.assert_array_equal(got.view(np.int32), want.view(np.int32))


# ---- 5. screen and estimate_screened against the pass written out -------------------------------------------------------------------
def screen_written_out(pkg, est, readings, bound, max_reject, min_sensors, available=None):
    S, K = readings.shape
    avail = np.ones((S, K), dtype=np.uint8) if available is None else available.copy()

    def residuals(a):
        return host(est.loo_residuals(readings, available=dev(a))[0]).copy()

    return pkg.screen_ref(residuals, bound, avail, max_reject, min_sensors)


@pytest.mark.parametrize("max_reject", [1, 2])
def test_screen_and_estimate_screened_equal_the_pass_written_out(pkg, oracle, max_reject):
    store, _, est = calibration_case(pkg, oracle)
    n, K = store.nodes_per_graph, len(OBS8)
    sb = est.calibrate_screening(store, (0.5, 0.9))
    S = 6
    readings = readings_of(pkg, S, n, OBS8, seed=2)
    readings[1, 2] += 300.0                                     # planted offsets: one sensor, two sensors, a small one
    readings[3, 5] -= 450.0
    readings[3, 0] += 250.0
    readings[4, 6] += 0.5
    bound = host(sb.bounds)[1].copy()
    for min_sensors, av in ((1, None), (K - 1, None), (2, T.availability(S, K, 0.3, seed=4))):
        d_av = None if av is None else dev(av)
        want_a, want_r, want_resid0, want_f0 = screen_written_out(pkg, est, readings, bound, max_reject, min_sensors, av)
        a, r, resid0, f0 = est.screen(readings, sb, 0.9, max_reject=max_reject, min_sensors=min_sensors, available=d_av)
        assert a.dtype == torch.uint8 and r.dtype == torch.int32 and f0.dtype == torch.uint8 and r.shape == (S, max_reject)
        np.testing.assert_array_equal(host(a), want_a)
        np.testing.assert_array_equal(host(r), want_r)
        np.testing.assert_array_equal(host(f0), want_f0)
        SR.same_floats(host(resid0), want_resid0)
        if av is None:
            assert host(r)[1, 0] == 2 and host(r)[3, 0] in (0, 5)
            if max_reject == 2 and min_sensors == 1:
                assert sorted(host(r)[3].tolist()) == [0, 5]
            if max_reject == 2 and min_sensors == K - 1:
                assert (host(r)[:, 1] == -1).all()              # a second rejection would leave K - 2 readings
        out = torch.empty((S, n), dtype=torch.float32, device=DEV)
        e, r2 = est.estimate_screened(readings, sb, 0.9, out=out, max_reject=max_reject, min_sensors=min_sensors, available=d_av)
        assert e is out and torch.equal(r2, r)
        want_e = est.estimate(readings, available=dev(want_a))
        assert torch.equal(e, want_e)
        # a rejected sensor's node carries the model's estimate, not its reading
        assert abs(float(e[1, OBS8[2]]) - float(readings[1, 2])) > 10.0 or av is not None
    e2, _ = est.estimate_screened(readings, sb, 0.9, max_reject=max_reject)
    assert e2 is not out and torch.equal(e2, est.estimate(readings, available=dev(screen_written_out(
        pkg, est, readings, bound, max_reject, 1)[0])))


# ---- 6. an exact end-to-end case resting on locality --------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "per_op"])
def test_a_far_fault_is_found_and_nothing_else_moves(pkg, oracle, fused):
    n, pipes, nb, S, bs = 40, 47, 1, 6, 4
    sensors, K = SR.FAR_SENSORS, len(SR.FAR_SENSORS)
    dist = R.graph_distances(topology(pkg, n, pipes).numpy(), n)[np.ix_(sensors, sensors)]
    assert (dist[~np.eye(K, dtype=bool)] > 3 * nb).all()        # nothing moves beyond 3 hops per block (test_gpu_sensitivity.py)
    store = make_store(pkg, S, n, pipes)
    model, _ = build(pkg, oracle, nb, 8, seed=3, fused=fused)
    est = pkg.PressureEstimator.for_store(model, store, sensors, batch_size=bs)
    clean = readings_of(pkg, S, n, sensors)
    resid_clean = host(est.loo_residuals(clean)[0]).copy()
    assert np.isfinite(resid_clean).all()
    worst = np.abs(resid_clean).max(axis=0)
    assert (worst > 0).all()
    sb = pkg.ScreeningBounds((0.99,), (2 * worst)[None, :], np.full(K, float(S)), sensors, device=DEV)
    a, r, resid0, f0 = est.screen(clean, sb, max_reject=2)
    assert (host(r) == -1).all() and (host(f0) == 0).all() and (host(a) == 1).all()
    np.testing.assert_array_equal(host(resid0).view(np.int32), resid_clean.view(np.int32))
    k_star, rows = 3, [1, 4]
    faulted = clean.clone()
    faulted[rows, k_star] += float(4 * worst[k_star] + 1)
    a, r, resid0, f0 = est.screen(faulted, sb, max_reject=2)
    got = host(resid0).copy()
    moved = np.zeros((S, K), dtype=bool)
    moved[rows, k_star] = True
    np.testing.assert_array_equal(got.view(np.int32)[~moved], resid_clean.view(np.int32)[~moved])        # nothing else moved
    assert (np.abs(got[moved]) > 2 * worst[k_star]).all()
    want_r = np.full((S, 2), -1, dtype=np.int32)
    want_r[rows, 0] = k_star
    np.testing.assert_array_equal(host(r), want_r)
    np.testing.assert_array_equal(host(f0), moved.astype(np.uint8))
    without = np.ones((S, K), dtype=np.uint8)
    without[rows, k_star] = 0
    np.testing.assert_array_equal(host(a), without)
    e, r2 = est.estimate_screened(faulted, sb, max_reject=2)
    np.testing.assert_array_equal(host(r2), want_r)
    assert torch.equal(e, est.estimate(faulted, available=dev(without)))
    assert not torch.equal(e, est.estimate(faulted))


# ---- 7. the back-test -----------------------------------------------------------------------------------------------------------------
def test_screening_report_equals_its_four_passes_written_out(pkg, oracle):
    store, _, est = calibration_case(pkg, oracle)
    S, K = len(store), len(OBS8)
    sb = est.calibrate_screening(store, (0.9,))
    offset = [300.0, -250.0, 400.0, 350.0, -300.0, 280.0, 330.0, -450.0]
    rep = est.screening_report(store, sb, fault_offset=offset, fault_share=0.5, seed=3, max_reject=2)
    fault_col = pkg.fault_draws(3, S, K, 0.5)
    np.testing.assert_array_equal(rep["fault_col"], fault_col)
    rows = np.nonzero(fault_col >= 0)[0]
    assert rows.size == S // 2
    readings = store.descale(store.data[:, OBS8]).contiguous()
    faulted = readings.clone()
    shift = torch.tensor(np.float32(offset)[fault_col[rows]], device=DEV)
    faulted[dev(rows), dev(fault_col[rows])] += shift
    without = np.ones((S, K), dtype=np.uint8)
    without[rows, fault_col[rows]] = 0
    screened, rejected = est.estimate_screened(faulted, sb, max_reject=2)
    rejected = host(rejected).copy()
    want = {"clean": est.estimate(readings), "faulted": est.estimate(faulted), "screened": screened,
            "oracle": est.estimate(faulted, available=dev(without))}
    for name, e in want.items():
        assert rep["nonsensor_mae"][name] == float(est.error_map(store, estimates=e)["hidden_mae"]), name
    np.testing.assert_array_equal(rep["rejected"], rejected)
    rates = pkg.screening_rates(rejected, fault_col)
    for name, v in rates.items():
        assert rep[name] == v or (np.isnan(v) and np.isnan(rep[name])), name
    print("screening_report:", {k: v for k, v in rep.items() if k not in ("fault_col", "rejected")})
    assert rep["detection_rate"] > 0 and rep["num_faulted"] == S // 2           # offsets far beyond every bound
    m = rep["nonsensor_mae"]
    assert m["faulted"] != m["clean"] and all(np.isfinite(v) for v in m.values())
    one = est.screening_report(store, sb, fault_offset=300.0, fault_share=1.0, seed=1)
    assert one["num_clean"] == 0 and np.isnan(one["false_rejection_rate_clean"]) and one["rejected"].shape == (S, 1)


# ---- 8. read-backs and allocations ----------------------------------------------------------------------------------------------------
def test_no_read_back_no_allocation_and_one_read_back_per_pass_in_the_report(pkg, oracle, monkeypatch):
    store, _, est = calibration_case(pkg, oracle)
    n, S, K = store.nodes_per_graph, 6, len(OBS8)
    sb = est.calibrate_screening(store, (0.9,))
    readings = readings_of(pkg, S, n, OBS8, seed=2)
    readings[1, 2] += 300.0
    d_av = dev(T.availability(S, K, 0.3, seed=4))
    out = torch.empty((S, n), dtype=torch.float32, device=DEV)

    def passes():
        resid, _ = est.loo_residuals(readings, available=d_av)
        est.screen(readings, sb, max_reject=2)
        e, r2 = est.estimate_screened(readings, sb, out=out, max_reject=2, min_sensors=2)
        return resid, e, r2

    small = pkg.SnapshotStore(raw_snapshots(pkg, S, n, 2), topology(pkg, n, 43), device=DEV, mean=store.mean, std=store.std)
    est.screening_report(small, sb, fault_offset=300.0, max_reject=2)
    first = tuple(t.clone() for t in passes())                  # plans, layouts, scratch and the bounds' inverse exist from here on
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
    before = torch.cuda.memory_stats(DEV)["allocation.all.allocated"]
    again = passes()
    allocated = torch.cuda.memory_stats(DEV)["allocation.all.allocated"] - before
    assert all(v == 0 for v in calls.values()), calls
    assert allocated == 0, allocated
    again = tuple(t.clone() for t in again)                     # (the results are a scratch: the report below overwrites it)
    est.screening_report(small, sb, fault_offset=300.0, max_reject=2)
    assert calls == {"synchronize": 0, "item": 0, "cpu": 4, "tolist": 0, "float": 0, "stream_sync": 0, "event_sync": 0}
    monkeypatch.undo()
    for got, want in zip(again, first):
        if got.dtype == torch.float32:
            SR.same_floats(host(got), host(want))
        else:
            assert torch.equal(got, want)


# ---- 9. the refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_on_the_device(pkg, oracle):
    store, model, est = calibration_case(pkg, oracle)
    S, K, n = 6, len(OBS8), store.nodes_per_graph
    sb = est.calibrate_screening(store, (0.9,))
    good = torch.zeros((S, K), dtype=torch.float32, device=DEV)
    for bad in (good.cpu(), good.double(), good[:, :2], good.reshape(-1), good[:0]):
        for call in (lambda b: est.loo_residuals(b), lambda b: est.screen(b, sb), lambda b: est.estimate_screened(b, sb)):
            with pytest.raises(ValueError, match="readings"):
                call(bad)
    av = torch.ones((S, K), dtype=torch.uint8, device=DEV)
    for bad in (av[:2], av.float(), av.cpu()):
        with pytest.raises(ValueError, match="available"):
            est.loo_residuals(good, available=bad)
        with pytest.raises(ValueError, match="available"):
            est.screen(good, sb, available=bad)
    with pytest.raises(ValueError, match="available"):
        est.loo_residuals_store(store, available=av)            # [len(store), K] is what it takes
    with pytest.raises(ValueError, match="available"):
        est.calibrate_screening(store, available=av)
    single = pkg.PressureEstimator.for_store(model, store, [5], batch_size=4)
    one = torch.zeros((S, 1), dtype=torch.float32, device=DEV)
    for call in (lambda: single.loo_residuals(one), lambda: single.loo_residuals_store(store),
                 lambda: single.calibrate_screening(store)):
        with pytest.raises(ValueError, match="two sensors"):
            call()
    other = pkg.ScreeningBounds((0.9,), sb.bounds.clone(), sb.counts.clone(), OBS8[::-1])
    with pytest.raises(ValueError, match="sensors"):
        est.screen(good, other)
    with pytest.raises(ValueError, match="must be on"):
        est.screen(good, pkg.ScreeningBounds.from_state_dict(sb.state_dict()))      # on the host
    with pytest.raises(ValueError, match="ScreeningBounds"):
        est.screen(good, est.calibrate_bounds(store, (0.9,)))
    with pytest.raises(ValueError, match="level"):
        est.screen(good, sb, 0.5)
    with pytest.raises(ValueError, match="levels"):
        est.calibrate_screening(store, (0.9, 0.5))
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="max_reject"):
            est.screen(good, sb, max_reject=bad)
        with pytest.raises(ValueError, match="max_reject"):
            est.screening_report(store, sb, fault_offset=1.0, max_reject=bad)
    for bad in (0, K + 1, 2.0):
        with pytest.raises(ValueError, match="min_sensors"):
            est.estimate_screened(good, sb, min_sensors=bad)
    with pytest.raises(ValueError, match="out must"):
        est.estimate_screened(good, sb, out=torch.empty((S, n + 1), device=DEV))
    for bad in ([1.0, 2.0], float("nan"), "x"):
        with pytest.raises(ValueError, match="fault_offset"):
            est.screening_report(store, sb, fault_offset=bad)
    with pytest.raises(ValueError, match="share"):
        est.screening_report(store, sb, fault_offset=1.0, fault_share=1.5)
    with pytest.raises(ValueError, match="nodes per graph"):
        est.loo_residuals_store(make_store(pkg, 2, 40, 47))
    multi = pkg.MultiSnapshotStore([(raw_snapshots(pkg, 3, n), topology(pkg, n, 43))] * 2, device="cpu")
    for call in (lambda: est.loo_residuals_store(multi), lambda: est.calibrate_screening(multi),
                 lambda: est.screening_report(multi, sb, fault_offset=1.0)):
        with pytest.raises(ValueError, match="MultiSnapshotStore"):
            call()
