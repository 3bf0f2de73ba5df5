"""Calibrated per-node error bounds on the device (k_bounds.hip, PressureEstimator.calibrate_bounds / coverage_report): the
radix select bit for bit against the sort-based statement ``estimation.node_error_bounds``, the coverage launch exactly against a
numpy restatement, the two tied together by the rank, and the estimator's methods against the same statements on read-back
estimates.  The kernels are driven directly on synthetic matrices; only the last section needs a model.

Shapes: N = 37 / 64 / 65 / 388 (below a wave, one wave, one past it, the C-Town size: 5 to 49 workgroups of 8 nodes in the
select, with a ragged last one at 37, 65 and 388); S = 1 ... 1000 around GATRES_NODE_ERROR_CHUNK = 64 (the coverage launch's
chunk), the select's 128 row slots and its trip of 512 rows.  Bounds are compared as uint32 patterns, so +inf and NaN compare."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_estimation import DEV, N37, OBS, make_store, raw_snapshots, small_model, stream, topology      # noqa: E402

LEVELS8 = (0.05, 0.25, 0.5, 0.75, 0.9, 0.95, 0.99, 0.999)
GUARD = 64                                       # elements of garbage on either side of an output
SCALINGS = ((7.3, 41.0), (1.0, 0.0))


def descaled(truth, scale, offset):
    """D(truth) of include/gatres.h on the host: a product and a sum, each rounded to fp32."""
    return truth * np.float32(scale) + np.float32(offset)


def guarded(n, dtype, fill):
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def untouched(buf, n, fill):
    left, right = buf[:GUARD].cpu().numpy(), buf[GUARD + n:].cpu().numpy()
    return bool((left == fill).all() and (right == fill).all())


def device_inputs(observed, available):
    obs = None if observed is None else torch.tensor(observed, dtype=torch.int32, device=DEV)
    av = None if available is None else torch.from_numpy(np.ascontiguousarray(available, dtype=np.uint8)).to(DEV)
    return obs, av


def run_quantiles(pkg, lib, est, truth, scale, offset, levels, observed=None, available=None):
    """One gatres_node_error_quantiles launch on device copies of the numpy matrices.  Returns (bounds as uint32 [Q, N], counts
    [N]) and asserts that nothing around either output was written."""
    import ctypes
    S, N = est.shape
    Q = len(levels)
    d_est, d_truth = torch.from_numpy(est).to(DEV), torch.from_numpy(truth).to(DEV)
    obs, av = device_inputs(observed, available)
    bbuf, bounds = guarded(Q * N, torch.float32, -777.25)
    cbuf, counts = guarded(N, torch.float64, -555.5)
    pkg._native.check(lib.gatres_node_error_quantiles(
        d_est.data_ptr(), d_truth.data_ptr(), S, N, scale, offset, pkg._native.ptr(obs), 0 if observed is None else len(observed),
        pkg._native.ptr(av), (ctypes.c_double * Q)(*levels), Q, bounds.data_ptr(), counts.data_ptr(), stream()),
        "gatres_node_error_quantiles")
    assert untouched(bbuf, Q * N, -777.25) and untouched(cbuf, N, -555.5), "the launch wrote outside bounds / counts"
    return bounds.cpu().numpy().view(np.uint32).reshape(Q, N), counts.cpu().numpy()


def run_coverage(pkg, lib, est, truth, scale, offset, bounds, observed=None, available=None):
    S, N = est.shape
    Q = bounds.shape[0]
    d_est, d_truth = torch.from_numpy(est).to(DEV), torch.from_numpy(truth).to(DEV)
    d_bounds = torch.from_numpy(np.ascontiguousarray(bounds, dtype=np.float32)).to(DEV)
    obs, av = device_inputs(observed, available)
    tbuf, table = guarded(N * 9, torch.float64, -555.5)
    pkg._native.check(lib.gatres_node_bound_coverage(
        d_est.data_ptr(), d_truth.data_ptr(), S, N, scale, offset, pkg._native.ptr(obs), 0 if observed is None else len(observed),
        pkg._native.ptr(av), d_bounds.data_ptr(), Q, table.data_ptr(), stream()), "gatres_node_bound_coverage")
    assert untouched(tbuf, N * 9, -555.5), "the launch wrote outside the table"
    return table.cpu().numpy().reshape(N, 9)


def hidden_mask(S, N, observed, available):
    """The counted entries of a launch with an availability: all but (s, observed[k]) where available[s, k] != 0."""
    hidden = np.ones((S, N), dtype=np.bool_)
    for k, v in enumerate(observed):
        hidden[:, v] = np.asarray(available)[:, k] == 0
    return hidden


def numpy_coverage(est, truth, scale, offset, bounds, hidden=None):
    """The table of gatres_node_bound_coverage by numpy: float comparisons of |e| with the bounds, over the counted entries."""
    S, N = est.shape
    ae = np.abs(est - descaled(truth, scale, offset))
    counted = np.ones((S, N), dtype=np.bool_) if hidden is None else hidden
    table = np.zeros((N, 9))
    table[:, 0] = counted.sum(0)
    with np.errstate(invalid="ignore"):
        for q in range(bounds.shape[0]):
            table[:, 1 + q] = ((ae <= bounds[q][None, :]) & counted).sum(0)
    return table


def random_matrices(S, N, seed):
    rng = np.random.default_rng(seed)
    truth = rng.standard_normal((S, N)).astype(np.float32)
    est = (truth * np.float32(7.3) + np.float32(41.0) + rng.standard_normal((S, N)).astype(np.float32) * np.float32(0.3))
    return est.astype(np.float32), truth


def expect(pkg, est, truth, scale, offset, levels, hidden=None):
    b, n = pkg.estimation.node_error_bounds(est, descaled(truth, scale, offset), levels, hidden=hidden)
    return b.view(np.uint32), n


# ---- 1. the select against the sort -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 2, 7, 63, 64, 65, 129, 1000])
@pytest.mark.parametrize("N", [37, 64, 65, 388])
def test_quantiles_equal_the_sorted_statement_bitwise(pkg, lib, N, S):
    est, truth = random_matrices(S, N, seed=1000 * N + S)
    for scale, offset in SCALINGS:
        for levels in ((0.9,), LEVELS8):
            got, counts = run_quantiles(pkg, lib, est, truth, scale, offset, levels)
            want, n = expect(pkg, est, truth, scale, offset, levels)
            np.testing.assert_array_equal(counts, n)
            assert (counts == S).all()
            np.testing.assert_array_equal(got, want, err_msg=f"scale {scale} levels {levels}")
    if S == 7:            # n = 7: the ranks ceil(8 q) are 1, 2, 4, 6, 8, 8, 8, 8 -- r = 1 and r = n + 1 (+inf), but no r = n: a launch of its own
        ranks = [int(pkg.estimation.conformal_rank(7, q)) for q in LEVELS8]
        assert ranks[0] == 1 and 7 not in ranks and ranks[4:] == [8] * 4
        assert (got[4:] == 0x7f800000).all() and (got[:4] < 0x7f800000).all()
        seven, _ = run_quantiles(pkg, lib, est, truth, 1.0, 0.0, (0.8,))          # ceil(6.4) = 7: r == n, the maximum
        np.testing.assert_array_equal(seven[0], np.abs(est - truth).view(np.uint32).max(0))


def from_bits(bits, rng):
    """Floats with the given magnitude patterns and random signs."""
    sign = (rng.integers(0, 2, size=bits.shape, dtype=np.uint32) << np.uint32(31))
    return (bits.astype(np.uint32) | sign).view(np.float32)


def special_matrix(S=1000, N=37, seed=5):
    """Errors a radix select gets wrong when a pass, a tie or the order of the patterns is mishandled.  truth = 0 and
    (scale, offset) = (1, 0): e is est itself."""
    rng = np.random.default_rng(seed)
    est = rng.standard_normal((S, N)).astype(np.float32)
    est[:, 0] = rng.choice(np.float32([0.125, 0.25, 0.375, 3.0, 1e-3]), size=S) * rng.choice(np.float32([-1, 1]), size=S)
    est[:, 1] = np.float32(-2.71828)                                               # all equal
    est[:, 2] = from_bits(np.zeros(S, dtype=np.uint32), rng)                       # zeros of both signs
    est[:, 3] = from_bits(np.uint32(0x3f800000) | rng.integers(0, 256, size=S, dtype=np.uint32), rng)           # the lowest byte
    est[:, 4] = from_bits((rng.integers(0, 128, size=S, dtype=np.uint32) << np.uint32(24)) | np.uint32(0x123456), rng)   # the highest
    est[:, 5] = from_bits(rng.integers(1, 1 << 23, size=S, dtype=np.uint32), rng)  # denormals
    est[:, 6] = from_bits(rng.integers(0, 4, size=S, dtype=np.uint32), rng)        # zeros and the three smallest denormals
    est[::7, 7] = np.inf                                                           # 143 of 1000: the upper levels are +inf
    est[::3, 8] = np.nan                                                           # 334 of 1000: NaN above every number
    est[1::3, 8] = -np.inf                                                         # ... and above the infinities below it
    est[::50, 9] = np.nan
    est[5::50, 9] = np.inf
    est[:, 10] = np.arange(S, dtype=np.float32) * np.float32(0.5)                  # ascending
    est[:, 11] = np.arange(S, 0, -1, dtype=np.float32) * np.float32(-0.5)          # descending in magnitude
    est[:, 12] = from_bits(np.uint32(0x7f7fff00) | rng.integers(0, 256, size=S, dtype=np.uint32), rng)          # next to +inf
    return est, np.zeros((S, N), dtype=np.float32)


@pytest.mark.parametrize("levels", [(0.5,), LEVELS8], ids=["Q1", "Q8"])
def test_quantiles_on_values_where_a_radix_select_goes_wrong(pkg, lib, levels):
    est, truth = special_matrix()
    got, counts = run_quantiles(pkg, lib, est, truth, 1.0, 0.0, levels)
    want, n = expect(pkg, est, truth, 1.0, 0.0, levels)
    np.testing.assert_array_equal(counts, n)
    for v in range(est.shape[1]):
        np.testing.assert_array_equal(got[:, v], want[:, v], err_msg=f"column {v}")
    if len(levels) == 8:
        assert (got[:, 1] == np.float32(2.71828).view(np.uint32)).all() and (got[:, 2] == 0).all()
        assert got[7, 7] == 0x7f800000 and got[0, 7] < 0x7f800000                # an infinite error, not a missing bound
        assert got[4, 7] == 0x7f800000 and got[3, 7] < 0x7f800000                # 143 infinities: the ranks from 858 on
        assert got[1, 8] < 0x7f800000 and got[2, 8] == 0x7f800000                # 333 numbers, 333 infinities: rank 251, rank 501
        assert (got[3:, 8] > 0x7f800000).all()                                   # NaN above +inf: the ranks from 667 on
        assert 0 < got[4, 5] < 0x00800000                                        # a denormal bound stays a denormal


def test_quantiles_with_more_rows_than_one_trip_per_thread(pkg, lib):
    """S = 1100 at 16 nodes: more than two trips of 512 rows, on two whole workgroups, with quantised errors (every pass ties)."""
    rng = np.random.default_rng(11)
    est = rng.integers(-3, 4, size=(1100, 16)).astype(np.float32) * np.float32(0.1)
    truth = np.zeros_like(est)
    got, counts = run_quantiles(pkg, lib, est, truth, 1.0, 0.0, LEVELS8)
    want, n = expect(pkg, est, truth, 1.0, 0.0, LEVELS8)
    np.testing.assert_array_equal(counts, n)
    np.testing.assert_array_equal(got, want)


# ---- 2. an availability -------------------------------------------------------------------------------------------------------------
def availability_case(S=129, N=388, seed=3):
    est, truth = random_matrices(S, N, seed=seed)
    observed = [387, 5, 100]                       # workgroups 48, 0 and 12 of the select; 6, 0 and 1 of the coverage launch
    rng = np.random.default_rng(seed)
    available = np.zeros((S, 3), dtype=np.uint8)
    available[:, 0] = 1                            # always there: never counted
    available[:, 2] = rng.random(S) < 0.3          # (column 1: never there)
    available[0, 2], available[S - 1, 2] = 1, 0    # (mixed at every S; the last row's byte is the one a row past the end reads)
    return est, truth, observed, available


@pytest.mark.parametrize("S", [2, 63, 64, 65, 129, 1000])
def test_quantiles_over_the_hidden_entries(pkg, lib, S):
    est, truth, observed, available = availability_case(S)
    S, N = est.shape
    hidden = hidden_mask(S, N, observed, available)
    for scale, offset in SCALINGS:
        got, counts = run_quantiles(pkg, lib, est, truth, scale, offset, LEVELS8, observed, available)
        want, n = expect(pkg, est, truth, scale, offset, LEVELS8, hidden=hidden)
        np.testing.assert_array_equal(counts, n)
        np.testing.assert_array_equal(got, want)
        plain, plain_counts = run_quantiles(pkg, lib, est, truth, scale, offset, LEVELS8)
        assert counts[387] == 0 and (got[:, 387] == 0x7f800000).all()           # present in every snapshot
        assert counts[5] == S and (got[:, 5] == plain[:, 5]).all()              # never present: a hidden node like any other
        assert 0 < counts[100] == S - available[:, 2].sum() < S
        others = [v for v in range(N) if v not in observed]
        np.testing.assert_array_equal(got[:, others], plain[:, others])
        np.testing.assert_array_equal(counts[others], plain_counts[others])


# ---- 3. the coverage launch -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 2, 7, 63, 64, 65, 129, 1000])
@pytest.mark.parametrize("N", [37, 64, 65, 388])
def test_coverage_equals_numpy_exactly(pkg, lib, N, S):
    est, truth = random_matrices(S, N, seed=77 * N + S)
    est[::5, 3] = np.nan                           # NaN errors: never inside
    est[S // 2, 4] = np.inf                        # an infinite error: inside an infinite bound only
    levels = (0.5, 0.9, 0.99)
    for scale, offset in SCALINGS:
        bits, _ = expect(pkg, est, truth, scale, offset, levels)
        bounds = bits.view(np.float32).copy()
        bounds[0, 1], bounds[1, 2], bounds[2, 3], bounds[1, 4], bounds[0, 5] = np.inf, np.nan, np.inf, np.inf, 0.0
        got = run_coverage(pkg, lib, est, truth, scale, offset, bounds)
        want = numpy_coverage(est, truth, scale, offset, bounds)
        np.testing.assert_array_equal(got, want)
        assert (got[:, 0] == S).all() and (got[:, 4:] == 0).all()
        assert got[1, 1] == S and got[2, 2] == 0 and got[4, 2] == S              # inf covers all, NaN nothing, inf covers inf
        assert got[3, 3] == S - len(range(0, S, 5))                              # inf covers all but the NaNs
    # one level: the other slots are zero
    one = run_coverage(pkg, lib, est, truth, 1.0, 0.0, bounds[:1])
    np.testing.assert_array_equal(one, numpy_coverage(est, truth, 1.0, 0.0, bounds[:1]))


@pytest.mark.parametrize("S", [2, 63, 64, 65, 129, 1000])
def test_coverage_over_the_hidden_entries(pkg, lib, S):
    est, truth, observed, available = availability_case(S)
    S, N = est.shape
    hidden = hidden_mask(S, N, observed, available)
    bits, _ = expect(pkg, est, truth, 7.3, 41.0, LEVELS8, hidden=hidden)
    bounds = bits.view(np.float32)
    got = run_coverage(pkg, lib, est, truth, 7.3, 41.0, bounds, observed, available)
    np.testing.assert_array_equal(got, numpy_coverage(est, truth, 7.3, 41.0, bounds, hidden))
    assert got[387].tolist() == [0.0] * 9 and got[5, 0] == S


def test_the_bounds_cover_their_own_calibration_data_by_the_rank(pkg, lib):
    """What ties the two launches together: on the calibration matrix itself at least r entries lie inside the bound of rank r,
    exactly r where the |e| of a column are distinct."""
    rng = np.random.default_rng(21)
    S, N = 129, 65
    # distinct magnitudes per column: a permutation of 0.25, 0.5, ..., S / 4 with random signs (exact in fp32; truth = 0)
    est = np.stack([rng.permutation(S) + 1 for _ in range(N)], axis=1).astype(np.float32) * np.float32(0.25)
    est *= rng.choice(np.float32([-1, 1]), size=(S, N))
    truth = np.zeros_like(est)
    ranks = np.array([pkg.estimation.conformal_rank(S, q) for q in LEVELS8])
    assert ranks[-1] > S and (ranks[:-1] <= S).all()                             # 0.999 needs 999 samples
    bits, counts = run_quantiles(pkg, lib, est, truth, 1.0, 0.0, LEVELS8)
    table = run_coverage(pkg, lib, est, truth, 1.0, 0.0, bits.view(np.float32))
    for q, r in enumerate(ranks):
        np.testing.assert_array_equal(table[:, 1 + q], np.full(N, S if r > S else r), err_msg=f"level {LEVELS8[q]}")
    # with ties (and an availability) the count may exceed the rank, never fall short of it
    est, truth, observed, available = availability_case()
    bits, counts = run_quantiles(pkg, lib, np.round(est, 1), truth, 7.3, 41.0, LEVELS8, observed, available)
    table = run_coverage(pkg, lib, np.round(est, 1), truth, 7.3, 41.0, bits.view(np.float32), observed, available)
    np.testing.assert_array_equal(table[:, 0], counts)
    for q, level in enumerate(LEVELS8):
        r = pkg.estimation.conformal_rank(counts, level)
        assert (table[:, 1 + q] >= np.where(r <= counts, r, counts)).all(), level


# ---- 4. the estimator ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def calibration(pkg, oracle):
    """The 37-node store of 70 snapshots, the small model and its estimator at batch size 32 (32, 32 and a ragged 6), shared by
    the tests below; nothing here is changed by them."""
    store = make_store(pkg, 70)
    model, _ = small_model(pkg, oracle)
    est = pkg.PressureEstimator.for_store(model, store, OBS, batch_size=32)
    truth = store.descale(store.data).cpu().numpy()
    return store, est, truth


def bits_of(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("mode", ["plain", "available", "noise"])
def test_calibrate_bounds_equals_the_sorted_statement(pkg, calibration, mode):
    store, est, truth = calibration
    levels = (0.5, 0.9, 0.95)
    kw, hidden = {}, None
    if mode == "available":
        rng = np.random.default_rng(4)
        a = np.ones((70, 3), dtype=np.uint8)
        a[:, 1] = 0
        a[:, 2] = rng.random(70) < 0.5
        kw["available"] = torch.from_numpy(a).to(DEV)
        hidden = hidden_mask(70, N37, OBS, a)
    if mode == "noise":
        kw.update(noise_std=0.3, noise_seed=12)
    eb = est.calibrate_bounds(store, levels, **kw)
    assert isinstance(eb, pkg.ErrorBounds) and eb.levels == levels and eb.observed_idx == OBS
    assert eb.bounds.device == store.device and eb.bounds.shape == (3, N37) and eb.counts.dtype == torch.float64
    p = est.estimate_store(store, **kw).cpu().numpy()
    want, n = pkg.estimation.node_error_bounds(p, truth, levels, hidden=hidden)
    np.testing.assert_array_equal(eb.counts.cpu().numpy(), n)
    np.testing.assert_array_equal(bits_of(eb.bounds), want.view(np.uint32))
    # given the estimates, the same bounds
    again = est.calibrate_bounds(store, levels, estimates=torch.from_numpy(p).to(DEV), available=kw.get("available"))
    assert torch.equal(bits_of_t(again.bounds), bits_of_t(eb.bounds))
    hidden_nodes = [v for v in range(N37) if v not in OBS]
    assert np.isfinite(want[:, hidden_nodes]).all() and (want[0, hidden_nodes] <= want[2, hidden_nodes]).all()
    if mode == "plain":                            # keep_observed: a sensor's bound is that of its own round trip
        assert (want[:, OBS] <= 1e-4).all()
    if mode == "available":
        assert n[OBS[0]] == 0 and np.isposinf(want[:, OBS[0]]).all() and n[OBS[1]] == 70
    if mode == "noise":
        quiet = pkg.estimation.node_error_bounds(est.estimate_store(store).cpu().numpy(), truth, levels)[0]
        assert not np.array_equal(quiet, want) and (want[:, OBS] > 1e-3).all()     # the sensors' bounds now hold their noise


def bits_of_t(t):
    return t.view(torch.int32)


def test_calibrate_bounds_at_388_nodes_behind_the_window_kernel(pkg, oracle):
    n, pipes, S = 388, 430, 64
    store = make_store(pkg, S, n=n, pipes=pipes, seed=4)
    model, _ = small_model(pkg, oracle, nb=15, nc=32, seed=11)
    plan = model.plan_for(store.edge_index(32), 32 * n)
    assert model._call_state(plan)["window"], "gatres_small at bs 32 should take the window kernel"
    sensors = [3, 17, 100, 101, 250, 387, 42, 9, 300, 77, 211, 5, 64, 128, 199, 350, 1, 260, 333, 150]
    est = pkg.PressureEstimator.for_store(model, store, sensors, batch_size=32)
    levels = (0.5, 0.9, 0.95)
    eb = est.calibrate_bounds(store, levels)
    want, n_v = pkg.estimation.node_error_bounds(est.estimate_store(store).cpu().numpy(), store.descale(store.data).cpu().numpy(),
                                                 levels)
    np.testing.assert_array_equal(bits_of(eb.bounds), want.view(np.uint32))
    np.testing.assert_array_equal(eb.counts.cpu().numpy(), n_v)
    assert np.isfinite(want).all()                 # 64 samples: ceil(65 * 0.95) = 62


def test_coverage_report_equals_the_report_of_a_numpy_table(pkg, calibration):
    store, est, truth = calibration
    levels = (0.5, 0.9)
    eb = est.calibrate_bounds(store, levels)
    test_store = pkg.SnapshotStore(raw_snapshots(pkg, 45, seed=8), topology(pkg), device=DEV, mean=store.mean, std=store.std)
    rep = est.coverage_report(test_store, eb)
    p = est.estimate_store(test_store).cpu().numpy()
    b = eb.bounds.cpu().numpy()
    ae = np.abs(p - test_store.descale(test_store.data).cpu().numpy())
    table = np.zeros((N37, 9))
    table[:, 0] = 45
    for q in range(2):
        table[:, 1 + q] = (ae <= b[q][None, :]).sum(0)
    want = pkg.estimation.coverage_from_table(table, b, levels, OBS)
    assert sorted(rep) == sorted(want) and rep["levels"] == levels
    for key in want:
        np.testing.assert_array_equal(rep[key], want[key], err_msg=key)
    assert rep["coverage"].shape == (2, N37) and rep["unbounded"].tolist() == [0, 0]
    assert 0.0 < rep["nonsensor_coverage"][0] <= rep["nonsensor_coverage"][1] <= 1.0
    # on the calibration store itself: at least the level, by construction
    own = est.coverage_report(store, eb)
    assert (own["min_coverage"] >= np.array(levels)).all()
    # with an availability, over the hidden entries
    a = np.ones((45, 3), dtype=np.uint8)
    a[::2, 0] = 0
    av = torch.from_numpy(a).to(DEV)
    rep = est.coverage_report(test_store, eb, available=av)
    p = est.estimate_store(test_store, available=av).cpu().numpy()
    hidden = hidden_mask(45, N37, OBS, a)
    ae = np.abs(p - test_store.descale(test_store.data).cpu().numpy())
    table[:, 0] = hidden.sum(0)
    for q in range(2):
        table[:, 1 + q] = ((ae <= b[q][None, :]) & hidden).sum(0)
    want = pkg.estimation.coverage_from_table(table, b, levels, OBS)
    for key in want:
        np.testing.assert_array_equal(rep[key], want[key], err_msg=key)
    assert np.isnan(rep["coverage"][:, OBS[1]]).all() and not np.isnan(rep["coverage"][:, OBS[0]]).any()


def test_estimate_with_bounds_is_estimate_and_two_broadcasts(pkg, calibration):
    store, est, _ = calibration
    eb = est.calibrate_bounds(store, (0.5, 0.9))
    readings = raw_snapshots(pkg, 9, seed=2).to(DEV)[:, OBS].contiguous()
    p, lo, hi = est.estimate_with_bounds(readings, eb, 0.9)
    want = est.estimate(readings)
    assert torch.equal(bits_of_t(p), bits_of_t(want))
    assert torch.equal(bits_of_t(lo), bits_of_t(want - eb.bounds[1])) and torch.equal(bits_of_t(hi), bits_of_t(want + eb.bounds[1]))
    assert lo.shape == (9, N37) and (lo <= p).all() and (p <= hi).all()
    with pytest.raises(ValueError, match="level"):
        est.estimate_with_bounds(readings, eb)                     # two levels: name one
    with pytest.raises(ValueError, match="level"):
        est.estimate_with_bounds(readings, eb, 0.95)
    one = est.calibrate_bounds(store)
    assert one.levels == (0.9,)
    p1, lo1, _ = est.estimate_with_bounds(readings, one, nan_is_missing=True)
    assert torch.equal(p1, want) and torch.equal(lo1, lo)


def test_reading_residuals_flag_what_leaves_the_leave_one_out_bound(pkg, calibration):
    store, est, _ = calibration
    K = len(OBS)
    each = []
    for k in range(K):
        a = torch.ones((70, K), dtype=torch.uint8, device=DEV)
        a[:, k] = 0
        each.append(est.calibrate_bounds(store, (0.9,), available=a))
    raw = raw_snapshots(pkg, 6, seed=2).to(DEV)[:, OBS].contiguous()
    readings = raw.clone()
    readings[2, 1] += 500.0                                         # one reading far off
    residual, flagged = est.reading_residuals(readings, each)
    assert residual.shape == (6, K) and flagged.dtype == torch.bool and flagged.shape == (6, K)
    for k in range(K):
        a = torch.ones((6, K), dtype=torch.uint8, device=DEV)
        a[:, k] = 0
        pred = est.estimate(readings, available=a)[:, OBS[k]]
        assert torch.equal(residual[:, k], readings[:, k] - pred)
        assert torch.equal(flagged[:, k], residual[:, k].abs() > each[k].bounds[0, OBS[k]])
    assert bool(flagged[2, 1]) and float(residual[2, 1]) > 400.0
    with pytest.raises(ValueError, match="one per sensor"):
        est.reading_residuals(readings, each[:2])


def test_calibrate_bounds_reads_nothing_back_and_coverage_report_once(pkg, calibration, monkeypatch):
    store, est, _ = calibration
    est.calibrate_bounds(store, (0.5, 0.9))                         # plans, buffers and the kernel's attributes exist from here on
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
    eb = est.calibrate_bounds(store, (0.5, 0.9))
    p = est.estimate_store(store)
    eb2 = est.calibrate_bounds(store, (0.5, 0.9), estimates=p)
    assert all(v == 0 for v in calls.values()), calls
    rep = est.coverage_report(store, eb, estimates=p)
    assert calls == {"synchronize": 0, "item": 0, "cpu": 1, "tolist": 0, "float": 0, "stream_sync": 0, "event_sync": 0}
    monkeypatch.undo()
    assert torch.equal(bits_of_t(eb.bounds), bits_of_t(eb2.bounds)) and np.isfinite(rep["nonsensor_coverage"]).all()


def test_bounds_refusals_on_the_device(pkg, oracle, calibration):
    store, est, _ = calibration
    with pytest.raises(ValueError, match="mean / std"):
        est.calibrate_bounds(make_store(pkg, 8, seed=9))            # a store with other statistics
    with pytest.raises(ValueError, match="increasing"):
        est.calibrate_bounds(store, (0.9, 0.5))
    with pytest.raises(ValueError, match="levels"):
        est.calibrate_bounds(store, tuple(0.1 * i for i in range(1, 10)))       # nine
    with pytest.raises(ValueError, match="levels"):
        est.calibrate_bounds(store, (0.5, 1.0))
    with pytest.raises(ValueError, match="available"):
        est.calibrate_bounds(store, available=torch.ones((69, 3), dtype=torch.uint8, device=DEV))
    eb = est.calibrate_bounds(store)
    other = pkg.PressureEstimator.for_store(est.model, store, [36, 0, 6], batch_size=32)
    with pytest.raises(ValueError, match="sensor layout"):
        other.coverage_report(store, eb)                            # bounds from another layout
    with pytest.raises(ValueError, match="sensor layout"):
        other.estimate_with_bounds(torch.zeros((2, 3), device=DEV), eb)
    with pytest.raises(ValueError, match="ErrorBounds"):
        est.coverage_report(store, eb.bounds)
    on_host = pkg.ErrorBounds.from_state_dict(eb.state_dict(), "cpu")
    with pytest.raises(ValueError, match="contiguous on"):
        est.coverage_report(store, on_host)
    back = pkg.ErrorBounds.from_state_dict(eb.state_dict(), DEV)
    assert est.coverage_report(store, back)["levels"] == (0.9,)
    fewer = pkg.ErrorBounds((0.9,), eb.bounds[:, :36].contiguous(), eb.counts[:36].contiguous(), OBS)
    with pytest.raises(ValueError, match="nodes"):
        est.coverage_report(store, fewer)
