"""The drift monitor of sensor readings, on the host: the two new symbols of k_monitor.hip are declared, exported and bound without
an ABI change and refuse their bad arguments before any launch; the numpy statements of monitoring.py hold on hand-computed cases;
the pair operator is associative and the slice-wise evaluation the kernel uses equals the loop; ``MonitorBaseline`` round-trips;
the Python refusals that need no device; and the shapes the device tests use lie past the constants of the kernels.  No GPU, no
kernel launches."""
import os
import re

import numpy as np
import pytest
import torch

import monitoring_refs as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gatres_cusum_scan", "gatres_monitor_latch")
NEW_NAMES = ("MonitorBaseline", "MonitorResult", "monitoring", "cusum_scan_ref", "cusum_fixed", "cusum_compose", "monitor_latch_ref",
             "monitor_ref", "monitor_baseline_from_moments", "drift_draws", "drift_offsets", "monitoring_rates")
P = 4096                       # (any non-null address: a refused call never reads it)
Q = 8192
NAN = np.float32("nan")
INF = np.float32("inf")
ONE = 65536


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
    assert len(S["gatres_cusum_scan"][1]) == 16 and len(S["gatres_monitor_latch"][1]) == 13
    assert "#define GATRES_ABI_VERSION 9" in hdr and pkg._native.ABI_VERSION == 9
    assert b"abi9" in lib.gatres_version()
    assert "k_monitor.hip" in pkg._build.SOURCES
    assert "#define GATRES_CUSUM_STATE 4" in hdr and "#define GATRES_CUSUM_RECORD 6" in hdr
    assert (pkg._native.CUSUM_STATE, pkg._native.CUSUM_RECORD) == (4, 6) == (pkg.monitoring.CUSUM_STATE, pkg.monitoring.CUSUM_RECORD)
    for name in NEW_NAMES:
        assert name in pkg.__all__ and hasattr(pkg, name), name
    assert pkg.cusum_scan_ref is pkg.monitoring.cusum_scan_ref is pkg.estimation.cusum_scan_ref
    assert pkg.monitoring_rates is pkg.estimation.monitoring_rates


def scan(lib, resid=P, mu=Q, inv_sigma=2 * Q, available=3 * Q, S=6, K=5, T=3, t0=0, kappa_q=ONE // 2, h_q=5 * ONE, state_in=4 * Q,
         state_out=5 * Q, records=6 * Q, stat_pos=7 * Q, stat_neg=8 * Q):
    return lib.gatres_cusum_scan(resid, mu, inv_sigma, available, S, K, T, t0, kappa_q, h_q, state_in, state_out, records, stat_pos,
                                 stat_neg, None)


def test_cusum_scan_checks_its_arguments_before_any_launch(lib):
    for name in ("resid", "mu", "inv_sigma", "records"):
        assert scan(lib, **{name: None}) == -1, name
    assert scan(lib, S=0) == -1 and scan(lib, K=0) == -1 and scan(lib, T=0) == -1 and scan(lib, S=-3, T=-3) == -1
    assert scan(lib, S=6, T=4) == -1 and scan(lib, S=6, T=7) == -1             # no whole number of series
    assert scan(lib, S=2 ** 30, T=2 ** 30) == -1                               # T >= 2^30
    assert scan(lib, t0=-1) == -1
    assert scan(lib, kappa_q=-1) == -1 and scan(lib, kappa_q=2 ** 31 + 1) == -1
    assert scan(lib, h_q=-1) == -1 and scan(lib, h_q=2 ** 31 + 1) == -1
    assert scan(lib, stat_pos=None) == -1 and scan(lib, stat_neg=None) == -1   # both or neither
    # overlaps: resid 6 * 5 floats = 120 bytes from P, mu and inv_sigma 20 bytes, available 30 bytes, state_in and state_out
    # 2 * 5 * 4 int64 = 320 bytes, records 2 * 5 * 6 int64 = 480 bytes, the paths 120 bytes each
    for name, size in (("state_out", 320), ("records", 480), ("stat_pos", 120), ("stat_neg", 120)):
        assert scan(lib, **{name: P}) == -1, name
        assert scan(lib, **{name: P + 120 - 1}) == -1, name                    # the last byte of resid
        assert scan(lib, **{name: P - size + 1}) == -1, name                   # ends on the first byte of resid
        assert scan(lib, **{name: Q + 19}) == -1, name                         # the last byte of mu
        assert scan(lib, **{name: 2 * Q + 19}) == -1, name                     # the last byte of inv_sigma
        assert scan(lib, **{name: 3 * Q + 29}) == -1, name                     # the last byte of available
        assert scan(lib, **{name: 4 * Q + 319}) == -1, name                    # the last byte of state_in
        if name != "state_out":
            assert scan(lib, **{name: 4 * Q}) == -1, name                      # state_in itself: only state_out may be it
            assert scan(lib, **{name: 5 * Q + 319}) == -1, name                # the last byte of state_out
    assert scan(lib, state_out=4 * Q + 8) == -1 and scan(lib, state_out=4 * Q - 8) == -1      # nearly state_in
    assert scan(lib, stat_pos=6 * Q + 479) == -1 and scan(lib, stat_neg=7 * Q + 119) == -1 and scan(lib, stat_neg=7 * Q) == -1
    # what is legal is not what these calls are refused for
    assert scan(lib, state_out=4 * Q, K=0) == -1                               # state_out == state_in
    assert scan(lib, available=None, state_in=None, state_out=None, stat_pos=None, stat_neg=None, K=0) == -1
    assert scan(lib, kappa_q=0, h_q=2 ** 31, K=0) == -1


def latch(lib, records=P, available=Q, S=6, K=5, T=3, t0=0, since=0, min_sensors=1, rnd=0, max_rounds=2, latched=2 * Q,
          latched_rec=3 * Q):
    return lib.gatres_monitor_latch(records, available, S, K, T, t0, since, min_sensors, rnd, max_rounds, latched, latched_rec, None)


def test_monitor_latch_checks_its_arguments_before_any_launch(lib):
    for name in ("records", "available", "latched", "latched_rec"):
        assert latch(lib, **{name: None}) == -1, name
    assert latch(lib, S=0) == -1 and latch(lib, K=0) == -1 and latch(lib, T=0) == -1
    assert latch(lib, S=6, T=4) == -1 and latch(lib, S=2 ** 30, T=2 ** 30) == -1
    assert latch(lib, t0=-1) == -1
    assert latch(lib, since=2) == -1 and latch(lib, since=-1) == -1
    assert latch(lib, min_sensors=0) == -1 and latch(lib, min_sensors=-2) == -1
    assert latch(lib, max_rounds=0) == -1
    assert latch(lib, rnd=-1) == -1 and latch(lib, rnd=2) == -1                # round outside [0, max_rounds)
    # overlaps: records 2 * 5 * 6 int64 = 480 bytes from P, available 30 bytes, latched 2 * 2 ints = 16 bytes, latched_rec
    # 2 * 2 * 6 int64 = 192 bytes
    for name, size in (("available", 30), ("latched", 16), ("latched_rec", 192)):
        assert latch(lib, **{name: P}) == -1, name
        assert latch(lib, **{name: P + 480 - 1}) == -1, name                   # the last byte of records
        assert latch(lib, **{name: P - size + 1}) == -1, name                  # ends on the first byte of records
    assert latch(lib, latched=Q + 29) == -1 and latch(lib, latched_rec=Q + 29) == -1          # the last byte of available
    assert latch(lib, latched_rec=2 * Q + 15) == -1                            # the last byte of latched
    assert latch(lib, since=1, rnd=1, min_sensors=5, K=0) == -1                # (legal: K is what is refused)


# ---- 2. the shapes of the device tests against the kernels' constants ---------------------------------------------------------------
def test_turnover_shapes_lie_past_the_constants():
    C = MR.constants()
    for name in ("CS_T", "CS_LANES", "CS_WAVES", "ML_T", "ML_LANES"):
        assert C.get(name, 0) > 0, name
    assert C["CS_LANES"] == 64 and C["CS_WAVES"] * C["CS_LANES"] == C["CS_T"] and C["ML_LANES"] == 64
    src = MR.source()
    assert "pair += gridDim.x" in src and "e += gridDim.x" in src and "k += ML_LANES" in src and "t += ML_T" in src
    assert "const int per = (T + CS_T - 1) / CS_T;" in src                      # the slices MR.slice_bounds restates
    W = C["CS_T"]
    lengths = MR.scan_lengths(W)
    assert {1, 2, W - 1, W, W + 1, 3 * W + 5} <= set(lengths) and 69000 < MR.SCAN_LONG < 71000 and MR.SCAN_LONG in lengths
    sizes = {T: sorted({hi - lo for lo, hi in MR.slice_bounds(T, W)}) for T in lengths}
    assert sizes[1] == [0, 1] and sizes[W - 1] == [0, 1] and sizes[W] == [1] and sizes[W + 1] == [0, 1, 2]
    assert sizes[3 * W + 5] == [0, 1, 4]                                        # a ragged last slice, and empty ones behind it
    assert len(sizes[MR.SCAN_LONG]) >= 2 and max(sizes[MR.SCAN_LONG]) > 256     # long slices, the last one ragged
    for T in lengths:
        cuts = MR.slice_bounds(T, W)
        assert cuts[0][0] == 0 and cuts[-1][1] == T and all(a[1] == b[0] for a, b in zip(cuts, cuts[1:]))
    c = MR.SCAN_CAPPED
    assert c["E"] * c["K"] > MR.grid_cap("gatres_cusum_scan") and c["T"] == 2
    c = MR.LATCH_CAPPED
    assert c["E"] > MR.grid_cap("gatres_monitor_latch")


# ---- 3. the numpy statements ------------------------------------------------------------------------------------------------------
def test_cusum_fixed_is_llrint(pkg):
    f = pkg.cusum_fixed
    assert f(0) == 0 and f(0.5) == 32768 and f(5.0) == 5 * ONE and f(32768) == 2 ** 31 and f(1) == ONE
    assert f(2.0 ** -17) == 0 and f(3 * 2.0 ** -17) == 2                        # ties to even
    assert f(0.1) == int(np.rint(0.1 * 65536.0)) == 6554
    for bad in (-0.001, 32768.5, float("nan"), float("inf"), "x", None, True):
        with pytest.raises(ValueError):
            f(bad)


def run(pkg, resid, mu=0.0, inv_sigma=1.0, available=None, T=None, t0=0, kappa=0.5, h=4.0, state=None):
    """One sensor, one series: (state_out [4], record [6], stat_pos, stat_neg) as lists."""
    resid = np.asarray(resid, dtype=np.float32).reshape(-1, 1)
    available = None if available is None else np.asarray(available, dtype=np.uint8).reshape(-1, 1)
    state = None if state is None else np.asarray(state, dtype=np.int64).reshape(1, 1, 4)
    st, rec, pos, neg = pkg.cusum_scan_ref(resid, np.float32([mu]), np.float32([inv_sigma]), available, T or len(resid), t0, kappa,
                                           h, state)
    assert st.dtype == np.int64 and rec.dtype == np.int64 and pos.dtype == np.float32 and neg.dtype == np.float32
    assert st.shape == (1, 1, 4) and rec.shape == (1, 1, 6) and pos.shape == resid.shape
    return st[0, 0].tolist(), rec[0, 0].tolist(), pos[:, 0].tolist(), neg[:, 0].tolist()


def test_cusum_scan_ref_by_hand(pkg):
    # an alarm at the first row: P = 5 - 0.5 = 4.5 > 4
    st, rec, pos, neg = run(pkg, [5.0, 0.0], t0=7)
    assert rec == [7, 1, 7, 1, 5 * ONE, 9 * ONE // 2] and pos == [4.5, 4.0] and neg == [0.0, 0.0]
    assert st == [4 * ONE, 0, 7, 9]                                            # (zM: one past the last row, where M was 0)
    # a statistic equal to h_q is no alarm: P = 4.0, then 4.5
    st, rec, pos, _ = run(pkg, [4.5, 1.0])
    assert pos == [4.0, 4.5] and rec == [1, 1, 0, 2, 11 * ONE // 2, 9 * ONE // 2]
    _, rec, pos, _ = run(pkg, [4.5, 0.5])
    assert pos == [4.0, 4.0] and rec == [-1, 0, 0, 0, 0, 0]
    # the minus side, and an onset after a zero: M = 0, 0, 2.5, 5.0
    st, rec, pos, neg = run(pkg, [1.0, 0.2, -3.0, -3.0], t0=100)
    assert neg == [0.0, 0.0, 2.5, 5.0] and rec == [103, -1, 102, 2, -6 * ONE, 5 * ONE]
    assert st[1] == 5 * ONE and st[3] == 102 and st[2] == 104                   # P fell to zero at the last row
    # both sides alarm at the same step from a carried state: the larger statistic wins, a tie goes to +
    carried = [6 * ONE, 7 * ONE, 3, 4]
    _, rec, _, _ = run(pkg, [0.0], t0=10, state=carried)
    assert rec == [10, -1, 4, 1, 0, 13 * ONE // 2]                             # M = 6.5 > P = 5.5; the onset is the carried zM
    _, rec, _, _ = run(pkg, [0.0], t0=10, state=[7 * ONE, 7 * ONE, 3, 4])
    assert rec == [10, 1, 3, 1, 0, 13 * ONE // 2]                              # a tie: +
    _, rec, _, _ = run(pkg, [0.0], t0=2, state=[7 * ONE, 7 * ONE, 9, 9])
    assert rec == [2, 1, 9, 0, 0, 13 * ONE // 2]                               # a carried onset behind the alarm: nothing to count
    # an onset from a carried zP: the excursion began in an earlier chunk; n and sum q count this call's rows only
    st, rec, pos, _ = run(pkg, [1.0, 1.5], t0=20, state=[3 * ONE, 0, 17, 20])
    assert pos == [3.5, 4.5] and rec == [21, 1, 17, 2, 5 * ONE // 2, 9 * ONE // 2] and st == [9 * ONE // 2, 0, 17, 22]
    # a carried state is clamped into [0, 2^61]
    st, _, _, _ = run(pkg, [NAN], state=[-5, 2 ** 62, 1, 1])
    assert st == [0, 2 ** 61, 1, 1]
    # a gap holds the state: unavailable, a NaN residual
    st, rec, pos, _ = run(pkg, [2.5, 9.0, NAN, 2.5, 0.5], available=[1, 0, 1, 1, 1])
    assert pos == [2.0, 2.0, 2.0, 4.0, 4.0] and rec == [-1, 0, 0, 0, 0, 0] and st == [4 * ONE, 0, 0, 5]
    _, rec, pos, _ = run(pkg, [2.5, 9.0, NAN, 2.5, 0.75], available=[1, 0, 1, 1, 1])
    assert rec == [4, 1, 0, 3, 23 * ONE // 4, 17 * ONE // 4]                   # n counts the counted entries only
    # an infinite residual clamps to 32768 sigma; so does 1e30
    for big in (INF, 1e30):
        st, rec, _, neg = run(pkg, [big, -big])
        assert rec == [0, 1, 0, 1, 2 ** 31, 2 ** 31 - ONE // 2] and st[0] == 0 and st[1] == 2 ** 31 - ONE // 2
    # a zero sigma (inv_sigma = +inf): z is NaN where the residual equals mu, and that entry is not counted
    st, rec, pos, _ = run(pkg, [0.25, 0.25, 1.0], mu=0.25, inv_sigma=INF, h=32768.0)
    assert pos[:2] == [0.0, 0.0] and rec[0] == -1 and st[2] == 0 and st[0] == 2 ** 31 - ONE // 2       # (never reset: never counted at 0)
    # a NaN mu: nothing is counted, the state is what came in
    st, rec, pos, neg = run(pkg, [1.0, 2.0], mu=NAN, t0=5, state=[ONE, 2 * ONE, 1, 2])
    assert st == [ONE, 2 * ONE, 1, 2] and rec == [-1, 0, 0, 0, 0, 0] and pos == [1.0, 1.0] and neg == [2.0, 2.0]
    # z is formed with two roundings: fp32(resid - mu), then the product
    r, m, s = np.float32(1.0000001), np.float32(0.3333333), np.float32(3.0000002)
    _, _, pos, _ = run(pkg, [r], mu=m, inv_sigma=s, kappa=0.0, h=100.0)
    z = np.float32(np.float32(r - m) * s)
    assert pos == [float(np.float32(np.float64(int(np.rint(np.float64(z) * 65536.0)))) * np.float32(2.0 ** -16))]


def test_cusum_scan_ref_series_and_shapes(pkg):
    resid = np.float32([[5.0, 0.0], [0.0, 0.0], [0.0, -5.0], [0.0, -5.0]])
    st, rec, pos, neg = pkg.cusum_scan_ref(resid, np.zeros(2, np.float32), np.ones(2, np.float32), None, 2, 3, 0.5, 4.0)
    assert st.shape == (2, 2, 4) and rec.shape == (2, 2, 6)
    np.testing.assert_array_equal(rec[:, :, 0], [[3, -1], [-1, 3]])             # every series starts at first_index
    np.testing.assert_array_equal(rec[1, 1], [3, -1, 3, 1, -5 * ONE, 9 * ONE // 2])
    _, _, none, _ = pkg.cusum_scan_ref(resid, np.zeros(2, np.float32), np.ones(2, np.float32), None, 2, 3, 0.5, 4.0, paths=False)
    assert none is None
    for bad in (dict(T=3), dict(T=0), dict(first_index=-1), dict(kappa=-1.0), dict(h=40000.0),
                dict(state=np.zeros((2, 2, 4), np.int32)), dict(state=np.zeros((1, 2, 4), np.int64))):
        kw = dict(T=2, first_index=0, kappa=0.5, h=4.0, state=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            pkg.cusum_scan_ref(resid, np.zeros(2, np.float32), np.ones(2, np.float32), None, kw["T"], kw["first_index"], kw["kappa"],
                               kw["h"], kw["state"])


def test_ll2float_rounds_once(pkg):
    f = pkg.monitoring._ll2float
    v = (1 << 60) + (1 << 36) + 1                                              # just above a tie of fp32 at 2^60
    assert f(v) == np.float32(2.0 ** 60 + 2.0 ** 37) and np.float32(np.float64(v)) == np.float32(2.0 ** 60)      # fp64 first: down
    assert f((1 << 60) + (1 << 36)) == np.float32(2.0 ** 60) and f(3) == 3.0 and f(-v) == -f(v) and f(2 ** 62) == np.float32(2.0 ** 62)


def test_cusum_compose_is_associative_and_slices_equal_the_loop(pkg):
    rng = np.random.default_rng(5)
    ops = [(int(a), int(c)) for a, c in zip(rng.integers(-9, 10, 60), rng.integers(-5, 6, 60))] + [pkg.monitoring.CUSUM_IDENTITY]
    for _ in range(400):
        x, y, z = (ops[i] for i in rng.integers(0, len(ops), 3))
        assert pkg.cusum_compose(pkg.cusum_compose(x, y), z) == pkg.cusum_compose(x, pkg.cusum_compose(y, z))
    for x in ops[:10]:
        for g in range(0, 12):
            y = ops[11]
            one = max(y[1], max(x[1], g + x[0]) + y[0])                         # x, then y
            both = pkg.cusum_compose(x, y)
            assert max(both[1], g + both[0]) == one
    ident = pkg.monitoring.CUSUM_IDENTITY
    assert pkg.cusum_compose(ident, (3, 0)) == (3, 0) and pkg.cusum_compose((3, 0), ident) == (3, 0)
    assert pkg.cusum_compose(ident, ident) == ident
    # the slice-wise evaluation against the loop, for every slice count from 1 to T + 1 (empty slices included)
    T = 23
    for trial in range(6):
        a = rng.integers(-5, 4, T)
        g0 = int(rng.integers(0, 6))
        g, loop = g0, []
        for t in range(T):
            g = max(0, g + int(a[t]))
            loop.append(g)
        assert 0 in loop and max(loop) > 0
        for W in range(1, T + 2):
            assert MR.slicewise_cusum(pkg, a, g0, MR.slice_bounds(T, W)) == loop, (trial, W)
        cuts = [(0, 0), (0, 5), (5, 5), (5, 6), (6, T), (T, T)]
        assert MR.slicewise_cusum(pkg, a, g0, cuts) == loop


def test_monitor_latch_ref_ties_and_ranges(pkg):
    T, K = 4, 4
    rec = np.zeros((1, K, 6), dtype=np.int64)
    rec[0, :, 0] = -1

    def go(records, before=None, since=0, min_sensors=1, t0=0, available=None):
        available = np.ones((T, K), dtype=np.uint8) if available is None else available
        keep = available.copy()
        a, lat, lr = pkg.monitor_latch_ref(records, available, T, t0, before, since, min_sensors)
        np.testing.assert_array_equal(available, keep)                         # (the input stays)
        assert a.dtype == np.uint8 and lat.dtype == np.int32 and lr.dtype == np.int64
        return a, int(lat[0]), lr[0].tolist()

    a, k, lr = go(rec)
    assert k == -1 and lr == [0] * 6 and a.all()                               # no candidate
    r = rec.copy()
    r[0, 1] = [3, 1, 2, 2, 9, 50]
    r[0, 2] = [2, -1, 1, 2, -9, 40]
    a, k, lr = go(r)
    assert k == 2 and lr == [2, -1, 1, 2, -9, 40]                              # the smaller alarm index
    np.testing.assert_array_equal(a[:, 2], [1, 0, 0, 0])                       # from its onset on
    assert a[:, [0, 1, 3]].all()
    a, k, _ = go(r, since=1)
    np.testing.assert_array_equal(a[:, 2], [1, 1, 0, 0])                       # from its alarm on
    r[0, 3] = [2, 1, 0, 3, 9, 41]
    assert go(r)[1] == 3                                                       # a tie on the index: the larger statistic
    r[0, 0] = [2, 1, 0, 3, 9, 41]
    assert go(r)[1] == 0                                                       # a tie on both: the smaller k
    assert go(r, before=[[0]])[1] == 3 and go(r, before=[[0, 3]])[1] == 2       # a latched sensor is no candidate
    assert go(r, before=[[-1, 0]])[1] == 3
    # min_sensors: K - #latched - 1 sensors stay
    assert go(r, min_sensors=3)[1] == 0 and go(r, min_sensors=4)[1] == -1
    assert go(r, before=[[0]], min_sensors=2)[1] == 3 and go(r, before=[[0]], min_sensors=3)[1] == -1
    assert go(r, before=[[-1]], min_sensors=3)[1] == 0                          # a round that latched nothing took nothing
    a, k, lr = go(r, before=[[0]], min_sensors=3)
    assert lr == [0] * 6 and a.all()
    # an onset before first_index: from row 0 on; an alarm is a global index
    r2 = rec.copy()
    r2[0, 1] = [12, 1, 5, 3, 9, 50]
    a, k, _ = go(r2, t0=10)
    assert k == 1 and not a[:, 1].any()
    a, k, _ = go(r2, t0=10, since=1)
    np.testing.assert_array_equal(a[:, 1], [1, 1, 0, 0])
    gaps = np.ones((T, K), dtype=np.uint8)
    gaps[3, 0] = gaps[0, 1] = 0
    a, _, _ = go(r2, t0=10, since=1, available=gaps)
    np.testing.assert_array_equal(a[:, 0], [1, 1, 1, 0])                       # what was missing stays missing
    np.testing.assert_array_equal(a[:, 1], [0, 1, 0, 0])
    for bad in (dict(since=2), dict(min_sensors=0)):
        with pytest.raises(ValueError):
            pkg.monitor_latch_ref(r, np.ones((T, K), np.uint8), T, 0, None, **bad)
    with pytest.raises(ValueError):
        pkg.monitor_latch_ref(r, np.ones((T + 1, K), np.uint8), T, 0)


def test_monitor_ref_over_two_rounds_with_a_fake_residual_callable(pkg):
    T, K = 6, 3
    mu, inv = np.zeros(K, np.float32), np.ones(K, np.float32)
    calls = []

    def residuals(avail, heal):
        calls.append(avail.copy())
        resid = np.zeros((T, K), dtype=np.float32)
        resid[2:, 0] = 3.0                                                     # sensor 0 drifts from row 2 on ...
        resid[3:, 2] = -2.0                                                    # ... and bends sensor 2's residual
        if heal:
            resid[avail[:, 0] == 0, 2] = 0.0                                   # without sensor 0 its neighbour is plausible again
        return resid

    out = pkg.monitor_ref(lambda a: residuals(a, True), mu, inv, np.ones((T, K), np.uint8), T, 0, 0.5, 4.0, max_latch=2)
    np.testing.assert_array_equal(out["latched"], [[0, -1]])
    np.testing.assert_array_equal(out["latched_rec"][0, 0], [3, 1, 2, 2, 6 * ONE, 5 * ONE])
    np.testing.assert_array_equal(out["available_out"][:, 0], [1, 1, 0, 0, 0, 0])
    assert out["available_out"][:, 1:].all() and len(calls) == 2 and calls[0].all()
    np.testing.assert_array_equal(calls[1], out["available_out"])
    np.testing.assert_array_equal(out["records0"][0, :, 0], [3, -1, 5])         # round 0 saw sensor 2 alarm later
    assert out["stat_pos"].shape == (T, K) and out["stat_pos"][3, 0] == 5.0 and out["stat_neg"][5, 2] == 4.5
    # the last round's state: sensor 0 is not counted from row 2 on, so it holds what rows 0 and 1 left
    np.testing.assert_array_equal(out["state"][0, 0], [0, 0, 2, 2])
    out = pkg.monitor_ref(lambda a: residuals(a, False), mu, inv, np.ones((T, K), np.uint8), T, 0, 0.5, 4.0, max_latch=2)
    np.testing.assert_array_equal(out["latched"], [[0, 2]])
    np.testing.assert_array_equal(out["available_out"][:, 2], [1, 1, 1, 0, 0, 0])
    out = pkg.monitor_ref(lambda a: residuals(a, False), mu, inv, np.ones((T, K), np.uint8), T, 0, 0.5, 4.0, max_latch=2,
                          min_sensors=2)
    np.testing.assert_array_equal(out["latched"], [[0, -1]])                   # a second latch would leave one sensor
    out = pkg.monitor_ref(lambda a: residuals(a, False), mu, inv, np.ones((T, K), np.uint8), T, 0, 0.5, 4.0, since=1)
    np.testing.assert_array_equal(out["available_out"][:, 0], [1, 1, 1, 0, 0, 0])
    assert out["latched"].shape == (1, 1)
    with pytest.raises(ValueError):
        pkg.monitor_ref(lambda a: residuals(a, False), mu, inv, np.ones((T, K), np.uint8), T, 0, 0.5, 4.0, max_latch=0)


def test_monitor_baseline_from_moments_by_hand(pkg):
    # e = prediction - reading; sensor 0: e = {1, 3}, sensor 1: e = {-2, -2, -2, -2}, sensor 2: no samples
    table = np.zeros((3, 8))
    table[0, :4] = [2, 4, 4, 10]
    table[1, :4] = [4, -8, 8, 16]
    b = pkg.monitor_baseline_from_moments(table)
    np.testing.assert_array_equal(b["mu"][:2], [-2.0, 2.0])
    np.testing.assert_array_equal(b["sigma"][:2], [1.0, 0.0])
    assert b["inv_sigma"].dtype == np.float32 and b["inv_sigma"][0] == 1.0 and np.isinf(b["inv_sigma"][1])
    assert np.isnan(b["mu"][2]) and np.isnan(b["sigma"][2]) and np.isnan(b["inv_sigma"][2])
    np.testing.assert_array_equal(b["counts"], [2, 4, 0])
    table[0, :4] = [3, 0.3, 0.5, 0.05]                                          # a variance that cancels below zero clamps to 0
    table[0, 3] = 0.03 * (1 - 1e-12)
    assert table[0, 3] / 3 - (0.3 / 3) ** 2 < 0
    assert pkg.monitor_baseline_from_moments(table)["sigma"][0] == 0.0
    table[0, :4] = [4, -6.0, 6.0, 11.0]                                         # mu = 1.5, var = 2.75 - 2.25 = 0.5
    b = pkg.monitor_baseline_from_moments(table)
    assert b["mu"][0] == 1.5 and b["sigma"][0] == np.sqrt(0.5) and b["inv_sigma"][0] == np.float32(1.0 / np.sqrt(0.5))


def test_drift_draws_and_offsets_on_known_answers(pkg):
    assert (pkg.drift_draws(0, 5, 20, 3, 0.0, 4) == -1).all()
    every = pkg.drift_draws(0, 5, 20, 3, 1.0, 4)
    assert every.dtype == np.int64 and every.shape == (5, 2)
    assert ((every[:, 0] >= 0) & (every[:, 0] < 3)).all() and ((every[:, 1] >= 4) & (every[:, 1] < 16)).all()
    half = pkg.drift_draws(5, 10, 30, 4, 0.5, 7)
    assert (half[:, 0] >= 0).sum() == 5 and ((half[:, 0] < 0) == (half[:, 1] < 0)).all()
    np.testing.assert_array_equal(half, pkg.drift_draws(5, 10, 30, 4, 0.5, 7))
    assert not np.array_equal(half, pkg.drift_draws(6, 10, 30, 4, 0.5, 7))
    rng = np.random.default_rng(5)                                              # the statement, replayed
    series = np.sort(rng.choice(10, size=5, replace=False))
    sensors = rng.integers(0, 4, size=5)
    onsets = rng.integers(7, 23, size=5)
    np.testing.assert_array_equal(np.nonzero(half[:, 0] >= 0)[0], series)
    np.testing.assert_array_equal(half[series, 0], sensors)
    np.testing.assert_array_equal(half[series, 1], onsets)
    assert (pkg.drift_draws(1, 9, 10, 2, 0.3, 0)[:, 0] >= 0).sum() == 3          # round(2.7)
    for bad in (dict(E=0, T=10, K=3, share=0.5, min_lead=1), dict(E=4, T=10, K=0, share=0.5, min_lead=1),
                dict(E=4, T=10, K=3, share=1.5, min_lead=1), dict(E=4, T=10, K=3, share=0.5, min_lead=5),
                dict(E=4, T=10, K=3, share=0.5, min_lead=-1)):
        with pytest.raises(ValueError):
            pkg.drift_draws(0, **bad)
    off = pkg.drift_offsets([[1, 2], [-1, -1], [0, 3]], 4, 2, [0.5, 0.1])
    assert off.dtype == np.float32 and off.shape == (12, 2)
    want = np.zeros((12, 2), dtype=np.float32)
    want[2:4, 1] = np.float32(0.1) * np.float32([1, 2])
    want[11, 0] = 0.5
    np.testing.assert_array_equal(off.view(np.int32), want.view(np.int32))
    np.testing.assert_array_equal(pkg.drift_offsets([[1, 0]], 3, 2, 2.0), np.float32([[0, 2], [0, 4], [0, 6]]))
    for bad in ([1.0], float("nan"), "x", [[1.0, 2.0]]):
        with pytest.raises(ValueError, match="drift_rate"):
            pkg.drift_offsets([[1, 0]], 3, 2, bad)
    with pytest.raises(ValueError):
        pkg.drift_offsets([[2, 0]], 3, 2, 1.0)
    with pytest.raises(ValueError):
        pkg.drift_offsets([[1, 3]], 3, 2, 1.0)


def test_monitoring_rates_on_known_answers(pkg):
    draws = [[2, 10], [0, 5], [1, 8], [3, 4], [-1, -1], [-1, -1]]
    latched = [[2, -1], [1, -1], [-1, -1], [0, 3], [-1, -1], [1, -1]]
    rec = np.zeros((6, 2, 6), dtype=np.int64)
    rec[0, 0] = [14, 1, 9, 5, 0, 0]                                            # delay 4, onset error 1
    rec[1, 0] = [9, 1, 7, 2, 0, 0]
    rec[3, 0] = [6, 1, 5, 1, 0, 0]
    rec[3, 1] = [13, -1, 7, 6, 0, 0]                                           # delay 9, onset error 3 (round 1 found it)
    rec[5, 0] = [3, 1, 2, 1, 0, 0]
    r = pkg.monitoring_rates(rec, latched, draws)
    assert r == {"detection_rate": 0.5, "misidentification_rate": 0.25, "false_alarm_rate_clean": 0.5, "mean_delay": 6.5,
                 "median_delay": 6.5, "mean_onset_error": 2.0, "num_drifted": 4, "num_clean": 2}
    r = pkg.monitoring_rates(rec[:2, :1], [[2], [-1]], [[2, 10], [0, 5]])
    assert r["detection_rate"] == 0.5 and np.isnan(r["false_alarm_rate_clean"]) and r["num_clean"] == 0 and r["mean_delay"] == 4.0
    r = pkg.monitoring_rates(rec[:2, :1], [[2], [-1]], [[-1, -1], [-1, -1]])
    assert np.isnan(r["detection_rate"]) and np.isnan(r["mean_delay"]) and np.isnan(r["median_delay"])
    assert np.isnan(r["mean_onset_error"]) and r["false_alarm_rate_clean"] == 0.5
    with pytest.raises(ValueError):
        pkg.monitoring_rates(rec, latched, draws[:5])
    with pytest.raises(ValueError):
        pkg.monitoring_rates(rec[:, :1], latched, draws)


# ---- 4. MonitorBaseline, MonitorResult and the refusals that need no device ---------------------------------------------------------
def test_monitor_baseline_round_trips_and_refuses_wrong_shapes(pkg):
    mb = pkg.MonitorBaseline([0.5, -1.0, 0.1], [2.0, 0.0, float("nan")], [10.0, 3.0, 0.0], [7, 1, 30])
    assert mb.observed_idx == [7, 1, 30] and mb.device == torch.device("cpu")
    assert mb.mu.dtype == torch.float32 and mb.inv_sigma.dtype == torch.float32
    assert mb.sigma.dtype == torch.float64 and mb.counts.dtype == torch.float64
    np.testing.assert_array_equal(mb.mu.numpy(), np.float32([0.5, -1.0, 0.1]))
    inv = mb.inv_sigma.numpy()
    assert inv[0] == 0.5 and np.isinf(inv[1]) and np.isnan(inv[2])
    third = pkg.MonitorBaseline([0.0], [3.0], [1.0], [4])
    assert third.inv_sigma.numpy()[0] == np.float32(1.0 / 3.0)                  # float32(1 / sigma), from fp64
    d = mb.state_dict()
    assert d["observed_idx"] == [7, 1, 30] and set(d) == {"mu", "sigma", "counts", "observed_idx"}
    back = pkg.MonitorBaseline.from_state_dict(d)
    for name in ("mu", "inv_sigma", "sigma", "counts"):
        a, b = getattr(back, name).numpy(), getattr(mb, name).numpy()
        np.testing.assert_array_equal(a.view(np.int32 if a.dtype == np.float32 else np.int64),
                                      b.view(np.int32 if b.dtype == np.float32 else np.int64), err_msg=name)
    assert back.observed_idx == mb.observed_idx
    from_tensors = pkg.MonitorBaseline(torch.tensor([0.5, -1.0, 0.1]), torch.tensor([2.0, 0.0, 1.0], dtype=torch.float64),
                                       torch.ones(3), [7, 1, 30])
    assert torch.equal(from_tensors.mu, mb.mu) and from_tensors.device == torch.device("cpu")
    for bad in (dict(mu=[0.5, 1.0]), dict(sigma=[[2.0, 1.0, 1.0]]), dict(counts=[1.0])):
        kw = dict(mu=[0.5, -1.0, 0.1], sigma=[2.0, 1.0, 1.0], counts=[1.0, 1.0, 1.0])
        kw.update(bad)
        with pytest.raises(ValueError, match=next(iter(bad))):
            pkg.MonitorBaseline(kw["mu"], kw["sigma"], kw["counts"], [7, 1, 30])


def test_monitor_result_shift_on_known_answers(pkg):
    mb = pkg.MonitorBaseline([0.0, 0.0, 0.0], [2.0, 0.5, 1.0], [1.0, 1.0, 1.0], [7, 1, 30])
    rec = torch.zeros((2, 2, 6), dtype=torch.int64)
    rec[0, 0] = torch.tensor([9, 1, 5, 4, 6 * ONE, 5 * ONE])                   # mean z = 1.5 at sensor 1: 0.75
    rec[1, 1] = torch.tensor([9, -1, 5, 2, -5 * ONE, 5 * ONE])                 # mean z = -2.5 at sensor 0: -5
    res = pkg.MonitorResult(None, torch.tensor([[1, -1], [-1, 0]], dtype=torch.int32), rec, None, None)
    s = res.shift(mb)
    assert s.dtype == torch.float64 and s.shape == (2, 2)
    assert float(s[0, 0]) == 0.75 and float(s[1, 1]) == -5.0 and bool(torch.isnan(s[0, 1])) and bool(torch.isnan(s[1, 0]))


def test_the_estimator_has_the_public_methods(pkg):
    for name in ("calibrate_monitor", "monitor", "monitor_store", "estimate_monitored", "monitoring_report"):
        assert callable(getattr(pkg.PressureEstimator, name)), name
    doc = pkg.PressureEstimator.monitor.__doc__
    assert "465" in doc and "autocorrelated" in doc and "No coverage statement" in doc
    assert "read-back" in pkg.PressureEstimator.calibrate_monitor.__doc__


def test_monitoring_arguments_are_refused_without_a_device(pkg):
    est = object.__new__(pkg.PressureEstimator)                # (the checks read nothing but these)
    est.observed_idx, est.device = [7, 1, 30], torch.device("cpu")
    mb = pkg.MonitorBaseline([0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [5.0, 5.0, 5.0], [7, 1, 30])

    def check(S=12, kappa=0.5, threshold=5.0, series_length=None, first_index=0, max_latch=1, min_sensors=1, since="onset",
              state=None, baseline=mb):
        return est._check_monitor(baseline, S, kappa, threshold, series_length, first_index, max_latch, min_sensors, since, state)

    assert check() == (32768, 5 * ONE, 1, 12, 0, 1, 1, 0)
    assert check(series_length=4, first_index=9, max_latch=2, min_sensors=3, since="alarm", kappa=0, threshold=32768) == \
        (0, 2 ** 31, 3, 4, 9, 2, 3, 1)
    assert check(series_length=4, state=torch.zeros((3, 3, 4), dtype=torch.int64))[2] == 3
    other = pkg.MonitorBaseline([0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [5.0, 5.0, 5.0], [7, 30, 1])
    with pytest.raises(ValueError, match="sensors"):
        check(baseline=other)
    sb = pkg.ScreeningBounds((0.9,), np.ones((1, 3), np.float32), np.ones(3), [7, 1, 30])
    with pytest.raises(ValueError, match="MonitorBaseline"):
        check(baseline=sb)
    for bad in (-0.5, 32769.0, float("nan"), "x"):
        with pytest.raises(ValueError, match="kappa"):
            check(kappa=bad)
        with pytest.raises(ValueError, match="threshold"):
            check(threshold=bad)
    for bad in (5, 0, -1, 2.0, 24):
        with pytest.raises(ValueError, match="series_length"):
            check(series_length=bad)
    for bad in (-1, 1.0, True):
        with pytest.raises(ValueError, match="first_index"):
            check(first_index=bad)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="max_latch"):
            check(max_latch=bad)
    for bad in (0, 4, 2.0, False):
        with pytest.raises(ValueError, match="min_sensors"):
            check(min_sensors=bad)
    for bad in ("both", 0, None, "Onset"):
        with pytest.raises(ValueError, match="since"):
            check(since=bad)
    for bad in (torch.zeros((1, 3, 4), dtype=torch.int32), torch.zeros((2, 3, 4), dtype=torch.int64),
                torch.zeros((1, 3, 6), dtype=torch.int64), np.zeros((1, 3, 4), np.int64),
                torch.zeros((1, 3, 4), dtype=torch.int64, device="meta")):
        with pytest.raises(ValueError, match="state"):
            check(state=bad)
    est.device = torch.device("meta")
    with pytest.raises(ValueError, match="must be on"):
        check()
