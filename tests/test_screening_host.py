"""The screening of sensor readings, on the host: the two new symbols of k_screen.hip are declared, exported and bound without an
ABI change and refuse their bad arguments before any launch; the numpy statements of screening.py hold on hand-computed cases;
``ScreeningBounds`` round-trips; the Python refusals that need no device; and the shapes the device tests use lie past the
constants of the kernels.  No GPU, no kernel launches."""
import os
import re

import numpy as np
import pytest
import torch

import screening_refs as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gatres_loo_residuals", "gatres_screen_reject")
P = 4096                       # (any non-null address: a refused call never reads it)
Q = 8192
NAN = np.float32("nan")
INF = np.float32("inf")


def header():
    with open(os.path.join(ROOT, "include", "gatres.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


# ---- 1. symbols and refusals ----------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound_and_the_abi_stays(pkg, lib):
    hdr = header()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in pkg._native.SIGNATURES
    S = pkg._native.SIGNATURES
    assert len(S["gatres_loo_residuals"][1]) == 17 and len(S["gatres_screen_reject"][1]) == 12
    assert "#define GATRES_ABI_VERSION 9" in hdr and pkg._native.ABI_VERSION == 9
    assert b"abi9" in lib.gatres_version()
    assert "k_screen.hip" in pkg._build.SOURCES
    for name in ("ScreeningBounds", "loo_layouts", "loo_residuals_from_estimates", "screen_reject_ref", "screen_ref", "fault_draws",
                 "screening_rates"):
        assert name in pkg.__all__ and hasattr(pkg, name), name
    assert pkg.screen_reject_ref is pkg.screening.screen_reject_ref is pkg.estimation.screen_reject_ref


def loo(lib, out=P, mask=Q, src=2 * Q, layout=0, src_rows=8, first_pair=4, n=37, graphs=3, observed=3 * Q, k=5, scale=2.0,
        offset=1.0, available=4 * Q, nan_is_missing=0, pred=5 * Q, resid=6 * Q):
    return lib.gatres_loo_residuals(out, mask, src, layout, src_rows, first_pair, n, graphs, observed, k, scale, offset, available,
                                    nan_is_missing, pred, resid, None)


def test_loo_residuals_checks_its_arguments_before_any_launch(lib):
    for name in ("out", "mask", "src", "observed", "pred", "resid"):
        assert loo(lib, **{name: None}) == -1, name
    assert loo(lib, layout=2) == -1 and loo(lib, layout=-1) == -1
    assert loo(lib, n=0) == -1 and loo(lib, graphs=0) == -1
    assert loo(lib, k=0) == -1 and loo(lib, k=38) == -1        # sensors outside [1, N]
    assert loo(lib, src_rows=0) == -1
    assert loo(lib, src_rows=2 ** 62) == -1                    # (the source's bytes do not fit)
    # the pair range: 8 rows x 5 sensors = 40 pairs
    assert loo(lib, first_pair=-1) == -1
    assert loo(lib, first_pair=38) == -1                       # pairs 38, 39, 40 of 40
    assert loo(lib, first_pair=40, graphs=1) == -1
    # overlaps.  The batch's entries are 3 floats = 12 bytes from pred + 16 and from resid + 16; out is 3 * 37 floats = 444 bytes
    # from P, mask 111 bytes from Q, src 8 * 37 floats = 1184 bytes from 2 * Q (8 * 5 floats = 160 in the readings layout),
    # observed 20 bytes from 3 * Q, available 40 bytes from 4 * Q
    assert loo(lib, resid=5 * Q) == -1                         # resid is pred
    assert loo(lib, resid=5 * Q + 8) == -1 and loo(lib, resid=5 * Q - 8) == -1
    for name in ("pred", "resid"):
        assert loo(lib, **{name: P - 16}) == -1, name                       # the batch's first entry is out
        assert loo(lib, **{name: P - 16 + 444 - 4}) == -1, name             # ... starts on the last float of out
        assert loo(lib, **{name: P - 16 - 12 + 4}) == -1, name              # ... ends on the first float of out
        assert loo(lib, **{name: Q - 16 + 110}) == -1, name                 # the last byte of mask
        assert loo(lib, **{name: 2 * Q - 16 + 1184 - 4}) == -1, name        # the last float of the full rows
        assert loo(lib, **{name: 2 * Q - 16 + 160 - 4}, layout=1) == -1, name
        assert loo(lib, **{name: 3 * Q - 16 + 16}) == -1, name              # the last sensor index
        assert loo(lib, **{name: 4 * Q - 16 + 39}) == -1, name              # the last byte of available
    assert loo(lib, pred=2 * Q - 16 + 160, layout=1, k=0) == -1             # (past the readings is legal: k is what is refused)
    assert loo(lib, available=None, k=0) == -1                              # (NULL is legal: k is what is refused)


def reject(lib, resid=P, bound=Q, inv_bound=2 * Q, available=3 * Q, S=6, K=5, min_sensors=1, rnd=0, max_rounds=2, rejected=4 * Q,
           flagged=5 * Q):
    return lib.gatres_screen_reject(resid, bound, inv_bound, available, S, K, min_sensors, rnd, max_rounds, rejected, flagged, None)


def test_screen_reject_checks_its_arguments_before_any_launch(lib):
    for name in ("resid", "bound", "inv_bound", "available", "rejected"):
        assert reject(lib, **{name: None}) == -1, name
    assert reject(lib, S=0) == -1 and reject(lib, K=0) == -1
    assert reject(lib, min_sensors=0) == -1 and reject(lib, min_sensors=-2) == -1
    assert reject(lib, max_rounds=0) == -1
    assert reject(lib, rnd=-1) == -1 and reject(lib, rnd=2) == -1           # round outside [0, max_rounds)
    assert reject(lib, S=2 ** 61) == -1
    # overlaps: resid 6 * 5 floats = 120 bytes from P, bound and inv_bound 20 bytes, available and flagged 30 bytes, rejected
    # 6 * 2 ints = 48 bytes
    for name, size in (("available", 30), ("rejected", 48), ("flagged", 30)):
        assert reject(lib, **{name: P}) == -1, name
        assert reject(lib, **{name: P + 120 - 1}) == -1, name               # the last byte of resid
        assert reject(lib, **{name: P - size + 1}) == -1, name              # ends on the first byte of resid
        assert reject(lib, **{name: Q + 19}) == -1, name                    # the last byte of bound
        assert reject(lib, **{name: 2 * Q + 19}) == -1, name                # the last byte of inv_bound
    assert reject(lib, rejected=3 * Q + 29) == -1                           # the last byte of available
    assert reject(lib, flagged=3 * Q + 29) == -1
    assert reject(lib, flagged=4 * Q + 47) == -1                            # the last byte of rejected
    assert reject(lib, flagged=None, K=0) == -1                             # (NULL is legal: K is what is refused)


# ---- 2. the shapes of the device tests against the kernels' constants ---------------------------------------------------------------
def test_turnover_shapes_lie_past_the_constants():
    C = SR.constants()
    for name in ("LR_T", "SR_T", "SR_LANES", "SR_WAVES"):
        assert C.get(name, 0) > 0, name
    assert C["SR_LANES"] == 64 and C["SR_WAVES"] * C["SR_LANES"] == C["SR_T"]
    src = SR.source()
    assert "g += (long long)gridDim.x * LR_T" in src and "s += (long long)gridDim.x * SR_WAVES" in src
    assert "k += SR_LANES" in src
    c = SR.LOO_CAPPED
    assert c["G"] > SR.grid_cap("gatres_loo_residuals") * C["LR_T"] and c["K"] <= c["N"]                    # the grid-stride trip
    assert min(SR.LOO_G) == 1 and any(g % k for g in SR.LOO_G for k in SR.LOO_K)                             # ragged batches
    c = SR.REJECT_CAPPED
    assert c["S"] > SR.grid_cap("gatres_screen_reject") * C["SR_WAVES"]
    K = SR.REJECT_K
    assert C["SR_LANES"] in K and C["SR_LANES"] + 1 in K and min(K) < C["SR_LANES"] and max(K) > 9 * C["SR_LANES"]
    assert any(s > C["SR_WAVES"] for s in SR.REJECT_S) and any(s % C["SR_WAVES"] for s in SR.REJECT_S)      # blocks, a ragged one


# ---- 3. the numpy statements ------------------------------------------------------------------------------------------------------
def test_loo_layouts_and_residuals_from_estimates(pkg):
    np.testing.assert_array_equal(pkg.loo_layouts(3), np.array([[0, 1, 1], [1, 0, 1], [1, 1, 0]], dtype=np.uint8))
    assert pkg.loo_layouts(2).dtype == np.uint8
    with pytest.raises(ValueError):
        pkg.loo_layouts(1)
    r = np.array([[50.5, NAN, 3.0], [1.0, 2.0, 3.0]], dtype=np.float32)
    e = np.array([[50.0, 1.0, 3.5], [0.1, 2.0, NAN]], dtype=np.float32)
    resid, pred = pkg.loo_residuals_from_estimates(r, e, present=[[1, 1, 0], [1, 1, 1]])
    assert resid.dtype == np.float32 and pred.dtype == np.float32
    np.testing.assert_array_equal(pred.view(np.int32), e.view(np.int32))
    assert resid[0, 0] == 0.5 and resid[1, 0] == np.float32(1.0) - np.float32(0.1) and resid[1, 1] == 0.0
    assert np.isnan(resid[0, 1]) and np.isnan(resid[1, 2])
    assert resid.view(np.uint32)[0, 2] == SR.NAN_BITS                        # the reading is not there: the quiet NaN


def one_round(pkg, resid, bound, available=None, min_sensors=1):
    resid = np.asarray([resid], dtype=np.float32)
    available = np.ones_like(resid, dtype=np.uint8) if available is None else np.asarray([available], dtype=np.uint8)
    before = available.copy()
    a, r, f = pkg.screen_reject_ref(resid, np.asarray(bound, dtype=np.float32), available, min_sensors)
    np.testing.assert_array_equal(available, before)                       # (the input stays)
    assert a.dtype == np.uint8 and r.dtype == np.int32 and f.dtype == np.uint8
    return a[0].tolist(), int(r[0]), f[0].tolist()


def test_screen_reject_ref_by_hand(pkg):
    b = [1.0, 2.0, 0.5]
    assert one_round(pkg, [0.5, -1.5, 0.25], b) == ([1, 1, 1], -1, [0, 0, 0])                 # no candidate
    assert one_round(pkg, [1.0, -2.0, 0.5], b) == ([1, 1, 1], -1, [0, 0, 0])                  # at the bound is inside
    assert one_round(pkg, [0.5, -3.0, 0.25], b) == ([1, 0, 1], 1, [0, 1, 0])                  # one candidate
    assert one_round(pkg, [0.0, -3.0, 1.0], b) == ([1, 1, 0], 2, [0, 1, 1])                   # scores 1.5 and 2: the smaller residual
    assert one_round(pkg, [2.0, 4.0, 0.0], b) == ([0, 1, 1], 0, [1, 1, 0])                    # scores 2 and 2: the smallest k
    assert one_round(pkg, [0.0, -4.0, 1.0], b) == ([1, 0, 1], 1, [0, 1, 1])
    assert one_round(pkg, [NAN, 0.0, 0.0], b) == ([1, 1, 1], -1, [0, 0, 0])                   # a NaN residual is no candidate
    assert one_round(pkg, [NAN, -3.0, 0.0], b) == ([1, 0, 1], 1, [0, 1, 0])
    assert one_round(pkg, [INF, -3.0, 0.0], b) == ([0, 1, 1], 0, [1, 1, 0])                   # an infinite residual is
    assert one_round(pkg, [9.0, -3.0, 0.0], b, available=[0, 1, 1]) == ([0, 0, 1], 1, [0, 1, 0])      # an unavailable one is not
    # bounds of NaN, +inf and 0
    assert one_round(pkg, [5.0, 5.0, 0.0], [NAN, INF, 0.0]) == ([1, 1, 1], -1, [0, 0, 0])     # 0 > 0 is false
    assert one_round(pkg, [5.0, INF, -0.0], [NAN, INF, 0.0]) == ([1, 1, 1], -1, [0, 0, 0])
    assert one_round(pkg, [5.0, 5.0, 1e-30], [NAN, INF, 0.0]) == ([1, 1, 0], 2, [0, 0, 1])    # score +inf
    assert one_round(pkg, [1.0, 2.0, 100.0], [0.0, 0.0, 1.0]) == ([0, 1, 1], 0, [1, 1, 1])    # +inf twice: the smallest k
    # min_sensors: the snapshot must keep that many
    assert one_round(pkg, [0.5, -3.0, 0.25], b, min_sensors=2) == ([1, 0, 1], 1, [0, 1, 0])
    assert one_round(pkg, [0.5, -3.0, 0.25], b, min_sensors=3) == ([1, 1, 1], -1, [0, 1, 0])  # blocked: flagged all the same
    assert one_round(pkg, [0.5, -3.0, 0.25], b, available=[0, 1, 1], min_sensors=2) == ([0, 1, 1], -1, [0, 1, 0])
    assert one_round(pkg, [0.5, -3.0, 0.25], b, available=[0, 1, 1], min_sensors=1) == ([0, 0, 1], 1, [0, 1, 0])
    with pytest.raises(ValueError):
        pkg.screen_reject_ref(np.zeros((2, 3), np.float32), np.ones(3, np.float32), np.ones((2, 3), np.uint8), 0)
    with pytest.raises(ValueError):
        pkg.screen_reject_ref(np.zeros((2, 3), np.float32), np.ones(2, np.float32), np.ones((2, 3), np.uint8))


def test_screen_reject_ref_is_the_total_order_written_out(pkg):
    """Against a plain Python loop over (score descending, k ascending) on random rows with planted ties."""
    rng = np.random.default_rng(3)
    S, K = 40, 9
    resid = rng.standard_normal((S, K)).astype(np.float32)
    bound = np.float32([2.0, 4.0, 1.0, 2.0, 8.0, 0.5, 2.0, 4.0, 2.0])
    resid[::3, 3] = resid[::3, 0]                                           # equal scores at k = 0, 3
    resid[::4, 7] = -2 * resid[::4, 6]                                      # ... and at k = 6, 7
    resid[5, 2] = NAN
    avail = (rng.random((S, K)) < 0.8).astype(np.uint8)
    a, r, f = pkg.screen_reject_ref(resid, bound, avail, 6)
    inv = np.float32(1.0) / bound
    for s in range(S):
        best, best_k = None, -1
        for k in range(K):
            cand = bool(avail[s, k]) and not np.isnan(resid[s, k]) and np.abs(resid[s, k]) > bound[k]
            assert f[s, k] == cand
            score = np.float32(np.abs(resid[s, k]) * inv[k])
            if cand and (best is None or score > best):
                best, best_k = score, k
        if best_k >= 0 and avail[s].sum() - 1 < 6:
            best_k = -1
        assert r[s] == best_k, s
        want = avail[s].copy()
        if best_k >= 0:
            want[best_k] = 0
        np.testing.assert_array_equal(a[s], want)
    assert (r >= 0).sum() > 5 and (r < 0).sum() > 5 and f.sum() > (r >= 0).sum()


def test_screen_ref_over_two_rounds_with_a_fake_residual_callable(pkg):
    bound = np.float32([1.0, 1.0, 1.0])
    calls = []

    def residuals(avail, heal):
        calls.append(avail.copy())
        resid = np.float32([[3.0, 0.0, 1.2], [0.0, 0.5, 0.0]]).copy()
        resid[avail == 0] = NAN
        if heal:                                                            # without sensor 0 its neighbour is plausible again
            resid[avail[:, 0] == 0, 2] = 0.1
        return resid

    a, r, resid0, flagged0 = pkg.screen_ref(lambda av: residuals(av, True), bound, np.ones((2, 3), np.uint8), max_reject=2)
    np.testing.assert_array_equal(r, [[0, -1], [-1, -1]])
    np.testing.assert_array_equal(a, [[0, 1, 1], [1, 1, 1]])
    np.testing.assert_array_equal(flagged0, [[1, 0, 1], [0, 0, 0]])
    np.testing.assert_array_equal(resid0, np.float32([[3.0, 0.0, 1.2], [0.0, 0.5, 0.0]]))
    assert len(calls) == 2 and calls[0].all() and calls[1].tolist() == [[0, 1, 1], [1, 1, 1]]
    a, r, _, _ = pkg.screen_ref(lambda av: residuals(av, False), bound, np.ones((2, 3), np.uint8), max_reject=2)
    np.testing.assert_array_equal(r, [[0, 2], [-1, -1]])
    np.testing.assert_array_equal(a, [[0, 1, 0], [1, 1, 1]])
    a, r, _, _ = pkg.screen_ref(lambda av: residuals(av, False), bound, np.ones((2, 3), np.uint8), max_reject=2, min_sensors=2)
    np.testing.assert_array_equal(r, [[0, -1], [-1, -1]])                   # the second rejection would leave one reading
    a, r, _, _ = pkg.screen_ref(lambda av: residuals(av, False), bound, np.ones((2, 3), np.uint8), max_reject=1)
    assert r.shape == (2, 1) and r[:, 0].tolist() == [0, -1]
    with pytest.raises(ValueError):
        pkg.screen_ref(lambda av: residuals(av, False), bound, np.ones((2, 3), np.uint8), max_reject=0)


def test_fault_draws_on_known_answers(pkg):
    assert (pkg.fault_draws(0, 7, 3, 0.0) == -1).all()
    every = pkg.fault_draws(0, 7, 3, 1.0)
    assert every.dtype == np.int64 and ((every >= 0) & (every < 3)).all()
    half = pkg.fault_draws(5, 10, 4, 0.5)
    assert (half >= 0).sum() == 5 and half.max() < 4 and half.min() == -1
    np.testing.assert_array_equal(half, pkg.fault_draws(5, 10, 4, 0.5))
    assert not np.array_equal(half, pkg.fault_draws(6, 10, 4, 0.5))
    rng = np.random.default_rng(5)                                          # the statement, replayed
    rows = np.sort(rng.choice(10, size=5, replace=False))
    cols = rng.integers(0, 4, size=5)
    np.testing.assert_array_equal(np.nonzero(half >= 0)[0], rows)
    np.testing.assert_array_equal(half[rows], cols)
    assert (pkg.fault_draws(1, 9, 2, 0.3) >= 0).sum() == 3                  # round(2.7)
    for bad in (dict(S=0, K=3, share=0.5), dict(S=4, K=0, share=0.5), dict(S=4, K=3, share=1.5), dict(S=4, K=3, share=-0.1)):
        with pytest.raises(ValueError):
            pkg.fault_draws(0, **bad)


def test_screening_rates_on_known_answers(pkg):
    rejected = [[2, -1], [1, -1], [-1, -1], [0, 3], [-1, -1], [1, -1]]
    fault_col = [2, 0, 1, 3, -1, -1]
    r = pkg.screening_rates(rejected, fault_col)
    assert r == {"detection_rate": 0.5, "misidentification_rate": 0.25, "false_rejection_rate_faulted": 0.5,
                 "false_rejection_rate_clean": 0.5, "num_faulted": 4, "num_clean": 2}
    r = pkg.screening_rates([[1], [-1]], [1, 0])
    assert r["detection_rate"] == 0.5 and np.isnan(r["false_rejection_rate_clean"]) and r["num_clean"] == 0
    r = pkg.screening_rates([[1], [-1]], [-1, -1])
    assert np.isnan(r["detection_rate"]) and np.isnan(r["misidentification_rate"]) and r["false_rejection_rate_clean"] == 0.5
    with pytest.raises(ValueError):
        pkg.screening_rates([[1], [-1]], [1, 0, 2])


# ---- 4. ScreeningBounds and the refusals that need no device ----------------------------------------------------------------------
def test_screening_bounds_round_trip_and_refuse_wrong_shapes(pkg):
    bounds = np.float32([[0.5, 2.0, 0.0], [1.0, INF, 0.25]])
    sb = pkg.ScreeningBounds((0.9, 0.99), bounds, [10.0, 3.0, 10.0], [7, 1, 30])        # from arrays
    assert sb.levels == (0.9, 0.99) and sb.observed_idx == [7, 1, 30] and sb.device == torch.device("cpu")
    assert sb.bounds.dtype == torch.float32 and sb.counts.dtype == torch.float64
    assert sb.level_index(0.99) == 1 and sb.level_index(0.9) == 0
    with pytest.raises(ValueError, match="level"):
        sb.level_index(None)
    with pytest.raises(ValueError, match="level"):
        sb.level_index(0.95)
    np.testing.assert_array_equal(sb.inverse.numpy(), np.float32([[2.0, 0.5, INF], [1.0, 0.0, 4.0]]))
    d = sb.state_dict()
    assert d["levels"] == [0.9, 0.99] and d["observed_idx"] == [7, 1, 30]
    back = pkg.ScreeningBounds.from_state_dict(d)
    assert torch.equal(back.bounds, sb.bounds) and torch.equal(back.counts, sb.counts)
    assert back.levels == sb.levels and back.observed_idx == sb.observed_idx
    one = pkg.ScreeningBounds((0.99,), torch.ones((1, 3)), torch.ones(3, dtype=torch.float64), [7, 1, 30])
    assert one.level_index(None) == 0
    for bad in (bounds[:1], bounds[:, :2], torch.from_numpy(bounds).double(), torch.from_numpy(bounds).t()):
        with pytest.raises(ValueError, match="bounds"):
            pkg.ScreeningBounds((0.9, 0.99), bad, [10.0, 3.0, 10.0], [7, 1, 30])
    with pytest.raises(ValueError, match="counts"):
        pkg.ScreeningBounds((0.9, 0.99), bounds, [10.0, 3.0], [7, 1, 30])
    with pytest.raises(ValueError, match="levels"):
        pkg.ScreeningBounds((0.99, 0.9), bounds, [10.0, 3.0, 10.0], [7, 1, 30])


def test_the_estimator_has_the_public_methods(pkg):
    for name in ("loo_residuals", "loo_residuals_store", "calibrate_screening", "screen", "estimate_screened", "screening_report"):
        assert callable(getattr(pkg.PressureEstimator, name)), name


def test_screening_arguments_are_refused_without_a_device(pkg):
    est = object.__new__(pkg.PressureEstimator)                # (the checks read nothing but these)
    est.observed_idx, est.device, est._loo_layouts = [7], torch.device("cpu"), None
    with pytest.raises(ValueError, match="two sensors"):
        est._loo_ready()
    est.observed_idx = [7, 1, 30]
    sb = pkg.ScreeningBounds((0.9, 0.99), np.ones((2, 3), np.float32), np.ones(3), [7, 1, 30])
    assert est._check_screening(sb, 0.99, 2, 3) == (1, 2, 3)
    other = pkg.ScreeningBounds((0.9, 0.99), np.ones((2, 3), np.float32), np.ones(3), [7, 30, 1])
    with pytest.raises(ValueError, match="sensors"):
        est._check_screening(other, 0.9, 1, 1)
    eb = pkg.ErrorBounds((0.9,), torch.ones((1, 3)), torch.ones(3, dtype=torch.float64), [7, 1, 30])
    with pytest.raises(ValueError, match="ScreeningBounds"):
        est._check_screening(eb, None, 1, 1)
    with pytest.raises(ValueError, match="level"):
        est._check_screening(sb, None, 1, 1)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="max_reject"):
            est._check_screening(sb, 0.9, bad, 1)
    for bad in (0, 4, 2.0, False):
        with pytest.raises(ValueError, match="min_sensors"):
            est._check_screening(sb, 0.9, 1, bad)
    est.device = torch.device("meta")
    with pytest.raises(ValueError, match="must be on"):
        est._check_screening(sb, 0.9, 1, 1)
