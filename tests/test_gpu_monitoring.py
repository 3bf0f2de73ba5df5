"""The drift monitor of sensor readings on the device (PressureEstimator.calibrate_monitor / monitor / monitor_store /
estimate_monitored / monitoring_report; k_monitor.hip): ``gatres_cusum_scan`` bit for bit against the sequential loop of
``cusum_scan_ref``, called directly into garbage-filled, padded buffers, at series lengths around the workgroup size (slices of
length 0, 1 and 2, ragged and long slices) and past the grid cap; two calls on consecutive chunks against one call;
``gatres_monitor_latch`` against ``monitor_latch_ref``; the calibration against its table and against numpy's mean and standard
deviation within the fp64 reordering bound; ``monitor`` / ``estimate_monitored`` against the pass written out; an exact end-to-end
case that rests on locality (sensors more than 3 hops apart under one block); the back-test against its passes written out;
read-backs and allocations counted; the refusals.  A float matrix is compared bit for bit (``screening_refs.same_floats``), every
int64 exactly."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import monitoring_refs as MR      # noqa: E402
import sensitivity_refs as R      # noqa: E402
import turnover_cases as TC      # noqa: E402
from estimation_refs import DEV, U      # noqa: E402
from test_gpu_model import build      # noqa: E402

PAD = 4                       # elements of garbage in front of and behind every target
FILL_F = -777.25
FILL_I = -777
OBS8 = [36, 0, 5, 17, 22, 9, 30, 13]
SENSORS388 = [3, 17, 100, 101, 250, 387, 42, 9, 300, 77, 211, 5, 64, 128, 199, 350, 1, 260, 333, 150]
W = MR.constants()["CS_T"]
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


def padded(n, dtype, fill):
    """A garbage-filled allocation of n elements with PAD more on either side, and the address of element PAD."""
    t = torch.full((n + 2 * PAD,), fill, dtype=dtype, device=DEV)
    return t, t.data_ptr() + PAD * t.element_size()


def body(t, shape, fill, what):
    a = host(t)
    assert (a[:PAD] == fill).all() and (a[-PAD:] == fill).all(), what
    return a[PAD:-PAD].reshape(shape)


# ---- 1. gatres_cusum_scan ---------------------------------------------------------------------------------------------------------
def device_scan(pkg, lib, resid, mu, inv_sigma, available, T, t0, kappa, h, state, alias, paths):
    """One launch into garbage-filled, padded targets.  Returns (state_out, records, stat_pos, stat_neg) as numpy."""
    S, K = resid.shape
    E = S // T
    d = [dev(resid), dev(mu), dev(inv_sigma), None if available is None else dev(available)]
    what = f"E{E} T{T} K{K} t0 {t0} av{available is not None} state{state is not None} alias{alias} paths{paths}"
    st_out, st_ptr = padded(E * K * 4, torch.int64, FILL_I)
    st_in_ptr = None
    if state is not None:
        if alias:
            st_out[PAD:-PAD] = dev(state).reshape(-1)
            st_in_ptr = st_ptr
        else:
            d.append(dev(state))
            st_in_ptr = d[-1].data_ptr()
    rec, rec_ptr = padded(E * K * 6, torch.int64, FILL_I)
    pos, pos_ptr = padded(S * K, torch.float32, FILL_F)
    neg, neg_ptr = padded(S * K, torch.float32, FILL_F)
    pkg._native.check(lib.gatres_cusum_scan(
        d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), pkg._native.ptr(d[3]), S, K, T, t0, pkg.cusum_fixed(kappa),
        pkg.cusum_fixed(h), st_in_ptr, st_ptr, rec_ptr, pos_ptr if paths else None, neg_ptr if paths else None, stream()),
        "gatres_cusum_scan")
    got_pos, got_neg = body(pos, (S, K), np.float32(FILL_F), what), body(neg, (S, K), np.float32(FILL_F), what)
    if not paths:
        assert (got_pos == np.float32(FILL_F)).all() and (got_neg == np.float32(FILL_F)).all(), what
    return body(st_out, (E, K, 4), FILL_I, what), body(rec, (E, K, 6), FILL_I, what), got_pos, got_neg, what


def carried_state(E, K, t0, seed):
    rng = np.random.default_rng(seed)
    st = np.zeros((E, K, 4), dtype=np.int64)
    st[:, :, :2] = rng.integers(0, 3 * 65536, size=(E, K, 2))
    st[:, :, 2:] = t0 - rng.integers(0, 50, size=(E, K, 2))
    st[0, 0, :2] = [-5, 2 ** 62]                                 # clamped into [0, 2^61] on entry
    return st


def scan_case(pkg, lib, E, T, K, variant, seed, drift_rows=None, kappa=0.5, h=4.0):
    gaps, specials, with_state, alias, paths = variant
    t0 = 1000 if with_state else (17 if seed % 2 else 0)
    drift_at = None
    if drift_rows is not None:
        drift_at = [(drift_rows[e % len(drift_rows)], 0, 1 if (e + seed) % 2 else -1) for e in range(E)]
    resid, mu, inv_sigma, available = MR.scan_inputs(E, T, K, seed, gaps, specials)
    if drift_at is not None:                                    # (a shift of 8 sigma on sensor 0: an alarm at that very row)
        for e, (row, k, sign) in enumerate(drift_at):
            resid[e * T + row:(e + 1) * T, k] = mu[k] + np.float32(sign * 8.0)
            if available is not None:
                available[e * T + row, k] = 1
    state = carried_state(E, K, t0, seed) if with_state else None
    want = pkg.cusum_scan_ref(resid, mu, inv_sigma, available, T, t0, kappa, h, state, paths=True)
    got_state, got_rec, got_pos, got_neg, what = device_scan(pkg, lib, resid, mu, inv_sigma, available, T, t0, kappa, h, state, alias,
                                                             paths)
    np.testing.assert_array_equal(got_state, want[0], err_msg=what)
    np.testing.assert_array_equal(got_rec, want[1], err_msg=what)
    if paths:
        MR.same_floats(got_pos, want[2], what)
        MR.same_floats(got_neg, want[3], what)
    return want, drift_at, t0


# (gaps, planted specials, a carried state, state_out == state_in, paths)
VARIANTS = [(False, False, False, False, True), (True, True, True, False, True), (True, False, True, True, False),
            (False, True, False, False, False), (False, False, True, True, True)]


@pytest.mark.parametrize("K", MR.SCAN_K)
@pytest.mark.parametrize("T", [t for t in MR.scan_lengths(W) if t != MR.SCAN_LONG])
def test_cusum_scan_bitwise(pkg, lib, T, K):
    cuts = [c for c in MR.slice_bounds(T, W) if c[1] > c[0]]
    rows = sorted({0, cuts[len(cuts) // 2][0], T - 1})          # the first, a middle and the last non-empty slice
    zeros = alarms = 0
    hit = set()
    for E in MR.SCAN_E:
        for i, variant in enumerate(VARIANTS):
            plain = not variant[1]
            want, drift_at, t0 = scan_case(pkg, lib, E, T, K, variant, 100 * T + 10 * K + E + i, drift_rows=rows if plain else None)
            rec = want[1]
            alarms += int((rec[:, :, 0] >= 0).sum())
            if plain:
                zeros += int(((want[2] == 0) & (np.roll(want[2], 1, axis=0) > 0)).sum())
                for e, (row, k, sign) in enumerate(drift_at):
                    if not variant[2]:                          # (a carried state may alarm before the planted row)
                        assert 0 <= rec[e, k, 0] <= t0 + row and (rec[e, k, 0] < t0 + row or rec[e, k, 1] == sign), (E, variant, e)
                        if rec[e, k, 0] == t0 + row:
                            hit.add((row, sign))
    assert alarms > 0
    assert {r for r, _ in hit} == set(rows) and {s for _, s in hit} == {1, -1}       # every slice, both sides
    if T >= W - 1:
        assert zeros > 0                                        # the statistic did return to zero after an excursion


@pytest.mark.parametrize("K", MR.SCAN_K)
def test_cusum_scan_bitwise_on_a_long_series(pkg, lib, K):
    T = MR.SCAN_LONG
    per = (T + W - 1) // W
    want, _, _ = scan_case(pkg, lib, 1, T, K, (True, K > 1, True, False, True), 7 + K, drift_rows=[150 * per + 3])
    assert (want[2] > 0).any() and ((want[2] == 0) & (np.roll(want[2], 1, axis=0) > 0)).sum() > 100
    assert want[1][0, 0, 0] >= 0


def test_cusum_scan_above_the_grid_cap(pkg, lib):
    c = MR.SCAN_CAPPED
    assert c["E"] * c["K"] > MR.grid_cap("gatres_cusum_scan")
    want, _, _ = scan_case(pkg, lib, c["E"], c["T"], c["K"], (True, False, False, False, True), 3, kappa=0.25, h=0.25)
    assert (want[1][-40:, :, 0] >= 0).any() and (want[1][-40:, :, 0] < 0).any()      # the series beyond the first trip, too


# ---- 2. continuation --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T1", [1, 3 * W + 4, 4 * 40, 4 * 40 + 2])
def test_two_calls_on_consecutive_chunks_equal_one_call(pkg, lib, T1):
    E, T, K, t0, kappa, h = 2, 3 * W + 5, 3, 40, 0.5, 3.0
    assert 0 < T1 < T and (T + W - 1) // W == 4                   # 160: a slice boundary of the one call, 162: inside a slice
    resid, mu, inv_sigma, available = MR.scan_inputs(E, T, K, 11, True, False)
    resid[T + 500:2 * T, 1] += np.float32(2.0)                    # series 1, sensor 1 drifts late: its alarm lies in chunk two
    resid[300:T, 2] -= np.float32(2.0)
    resid[150:T, 0] = mu[0] + np.float32(0.7)                     # series 0, sensor 0 creeps: 0.2 sigma per step from row 150 on
    state0 = carried_state(E, K, t0, 5)
    state0[0, 0, :2] = [30000, 0]
    whole = device_scan(pkg, lib, resid, mu, inv_sigma, available, T, t0, kappa, h, state0, False, True)
    want = pkg.cusum_scan_ref(resid, mu, inv_sigma, available, T, t0, kappa, h, state0)
    np.testing.assert_array_equal(whole[0], want[0])
    np.testing.assert_array_equal(whole[1], want[1])

    def chunk(a, lo, hi):
        return None if a is None else np.concatenate([a[e * T + lo:e * T + hi] for e in range(E)])

    one = device_scan(pkg, lib, chunk(resid, 0, T1), mu, inv_sigma, chunk(available, 0, T1), T1, t0, kappa, h, state0, False, True)
    two = device_scan(pkg, lib, chunk(resid, T1, T), mu, inv_sigma, chunk(available, T1, T), T - T1, t0 + T1, kappa, h, one[0], True,
                      True)
    np.testing.assert_array_equal(two[0], whole[0])             # the final state
    for i in (2, 3):                                            # the paths concatenate
        joined = np.concatenate([np.concatenate([one[i][e * T1:(e + 1) * T1], two[i][e * (T - T1):(e + 1) * (T - T1)]])
                                 for e in range(E)])
        MR.same_floats(joined, whole[i], f"T1 {T1} path {i}")
    first = np.where(one[1][:, :, :1] >= 0, one[1], two[1])     # the first alarm: chunk one's if it had one
    for f in (0, 1, 2, 5):                                      # ([3] and [4] count the rows of their own call)
        np.testing.assert_array_equal(first[:, :, f], whole[1][:, :, f], err_msg=f"T1 {T1} field {f}")
    in_two = (one[1][:, :, 0] < 0) & (two[1][:, :, 0] >= 0)
    print(f"T1 {T1}: {int((one[1][:, :, 0] >= 0).sum())} first alarms in chunk one, {int(in_two.sum())} in chunk two, "
          f"{int((two[1][:, :, 2][in_two] < t0 + T1).sum())} of those with an onset in chunk one")
    assert (in_two.any() if T1 < 300 else (one[1][:, :, 0] >= 0).any()) and (whole[1][:, :, 0] >= 0).any()
    if T1 in (160, 162):                                        # the creep began in chunk one and alarmed in chunk two
        assert in_two[0, 0] and 150 <= two[1][0, 0, 2] - t0 < T1 <= two[1][0, 0, 0] - t0


# ---- 3. gatres_monitor_latch ------------------------------------------------------------------------------------------------------
def latch_records(E, K, T, t0, seed):
    """Records with ties on the alarm index and on the statistic, series without an alarm, onsets before first_index."""
    rng = np.random.default_rng(seed)
    rec = np.zeros((E, K, 6), dtype=np.int64)
    alarm = t0 + rng.integers(0, max(T, 2) // 2 + 1, size=(E, K))
    has = rng.random((E, K)) < 0.6
    rec[:, :, 0] = np.where(has, alarm, -1)
    rec[:, :, 1] = np.where(has, rng.choice([-1, 1], size=(E, K)), 0)
    rec[:, :, 2] = np.where(has, alarm - rng.integers(0, 4, size=(E, K)), 0)          # (some of them before t0)
    rec[:, :, 3] = np.where(has, rng.integers(1, 5, size=(E, K)), 0)
    rec[:, :, 4] = np.where(has, rng.integers(-9, 10, size=(E, K)) * 65536, 0)
    rec[:, :, 5] = np.where(has, rng.integers(1, 4, size=(E, K)) * 2 ** 40, 0)         # few values: ties; beyond 32 bits
    if K >= 3:
        rec[0, :3] = [[t0 + 1, 1, t0 - 2, 3, 7, 9], [t0 + 1, -1, t0, 2, -7, 9], [t0 + 1, 1, t0 + 1, 1, 7, 8]]      # a tie on both
    return rec


def latch_case(pkg, lib, E, K, T, t0, seed):
    rec = latch_records(E, K, T, t0, seed)
    rng = np.random.default_rng(seed + 1)
    avail = (rng.random((E * T, K)) < 0.9).astype(np.uint8)
    d_rec = dev(rec)
    seen = set()
    for rnd in (0, 1):
        before = None
        if rnd == 1:
            before = pkg.monitor_latch_ref(rec, avail, T, t0, None, 0, 1)[1].astype(np.int64)[:, None]      # round 0's choice
            before[::3] = -1                                    # (and series in which round 0 latched nothing)
        for since in (0, 1):
            for min_sensors in sorted({1, max(1, K - 1), K}):
                want_a, want_l, want_r = pkg.monitor_latch_ref(rec, avail, T, t0, before, since, min_sensors)
                seen.add(int((want_l >= 0).sum()))
                d_avail, a_ptr = padded(E * T * K, torch.uint8, 0xAB)
                d_avail[PAD:-PAD] = dev(avail).reshape(-1)
                latched, l_ptr = padded(E * 2, torch.int32, FILL_I)
                if before is not None:
                    latched[PAD:-PAD].reshape(E, 2)[:, 0] = dev(before[:, 0].astype(np.int32))
                lrec, r_ptr = padded(E * 2 * 6, torch.int64, FILL_I)
                pkg._native.check(lib.gatres_monitor_latch(d_rec.data_ptr(), a_ptr, E * T, K, T, t0, since, min_sensors, rnd, 2, l_ptr,
                                                           r_ptr, stream()), "gatres_monitor_latch")
                what = f"E{E} K{K} T{T} t0 {t0} round{rnd} since{since} min{min_sensors}"
                np.testing.assert_array_equal(body(d_avail, (E * T, K), 0xAB, what), want_a, err_msg=what)      # every byte
                got_l, got_r = body(latched, (E, 2), FILL_I, what), body(lrec, (E, 2, 6), FILL_I, what)
                np.testing.assert_array_equal(got_l[:, rnd], want_l, err_msg=what)
                np.testing.assert_array_equal(got_r[:, rnd], want_r, err_msg=what)
                assert (got_r[:, 1 - rnd] == FILL_I).all(), what                # the other round's row is untouched
                if rnd == 0:
                    assert (got_l[:, 1] == FILL_I).all(), what
                else:
                    np.testing.assert_array_equal(got_l[:, 0], before[:, 0], err_msg=what)
                    assert ((want_l < 0) | (want_l != before[:, 0])).all(), what       # an already latched sensor is not taken
    return seen


@pytest.mark.parametrize("K", [1, 3, 7, 70])
@pytest.mark.parametrize("E,T,t0", [(1, 1, 0), (3, 5, 2), (2, 300, 1000)])
def test_monitor_latch_against_its_statement(pkg, lib, E, T, t0, K):
    seen = latch_case(pkg, lib, E, K, T, t0, 100 * E + K + T)
    assert 0 in seen                                            # min_sensors = K blocks every latch
    if K >= 3 and E > 1:
        assert max(seen) > 0


def test_monitor_latch_above_the_grid_cap(pkg, lib):
    c = MR.LATCH_CAPPED
    assert c["E"] > MR.grid_cap("gatres_monitor_latch")
    seen = latch_case(pkg, lib, c["E"], c["K"], c["T"], 3, 9)
    assert max(seen) > c["E"] // 2


# ---- 4. the calibration -----------------------------------------------------------------------------------------------------------
def calibration_case(pkg, oracle):
    if "cal" not in _CACHE:
        n, pipes, S = 37, 43, 24
        store = make_store(pkg, S, n, pipes, seed=7)
        model, _ = build(pkg, oracle, 2, 8, seed=3)
        est = pkg.PressureEstimator.for_store(model, store, OBS8, batch_size=4)
        _CACHE["cal"] = (store, model, est)
    return _CACHE["cal"]


@pytest.mark.parametrize("gaps", [False, True], ids=["complete", "gaps"])
def test_calibrate_monitor_equals_its_table_and_numpy(pkg, lib, oracle, gaps):
    store, _, est = calibration_case(pkg, oracle)
    S, K = len(store), len(OBS8)
    av = TC.availability(S, K, 0.3, seed=9) if gaps else None
    d_av = None if av is None else dev(av)
    mb = est.calibrate_monitor(store, available=d_av)
    assert isinstance(mb, pkg.MonitorBaseline) and mb.observed_idx == OBS8 and mb.device == torch.device(DEV)
    assert mb.mu.shape == (K,) and mb.mu.dtype == torch.float32 and mb.inv_sigma.dtype == torch.float32
    # exactly: the table of the same launch, read back, through monitor_baseline_from_moments
    resid, pred = est.loo_residuals_store(store, available=d_av)
    resid = host(resid).copy()
    truth = store.data[:, OBS8].contiguous()
    sensors = torch.arange(K, dtype=torch.int32, device=DEV)
    table = torch.empty((K, 8), dtype=torch.float64, device=DEV)
    if gaps:
        missing = dev((av == 0).astype(np.uint8))
        pkg._native.check(lib.gatres_node_error_moments_available(
            pred.data_ptr(), truth.data_ptr(), S, K, est.scale, est.offset, sensors.data_ptr(), K, missing.data_ptr(),
            table.data_ptr(), stream()), "gatres_node_error_moments_available")
    else:
        pkg._native.check(lib.gatres_node_error_moments(pred.data_ptr(), truth.data_ptr(), S, K, est.scale, est.offset,
                                                        sensors.data_ptr(), K, table.data_ptr(), stream()), "gatres_node_error_moments")
    want = pkg.monitor_baseline_from_moments(host(table))
    np.testing.assert_array_equal(host(mb.mu).view(np.int32), want["mu"].astype(np.float32).view(np.int32))
    np.testing.assert_array_equal(host(mb.sigma).view(np.int64), want["sigma"].view(np.int64))
    np.testing.assert_array_equal(host(mb.inv_sigma).view(np.int32), want["inv_sigma"].view(np.int32))
    np.testing.assert_array_equal(host(mb.counts), want["counts"])
    # against numpy on the residuals read back.  The table's e is -resid exactly, and e and e^2 are exact in fp64, so the
    # kernel's sums and numpy's differ by the order of the additions alone: each lies within (n - 1) * 2^-53 * sum |term| of the
    # exact sum, the two within twice that of each other.  Propagated: mu = -sum / n adds one rounding; the variance
    # sum e^2 / n - mu^2 adds three roundings of magnitude <= sum e^2 / n + mu^2 on either side, and numpy's two-pass
    # variance (np.std) is within (n + 3) * 2^-53 of itself; sigma_a - sigma_b = (var_a - var_b) / (sigma_a + sigma_b).
    present = np.ones((S, K), dtype=bool) if av is None else av != 0
    for k in range(K):
        r = resid[present[:, k], k].astype(np.float64)
        n = r.size
        assert n == want["counts"][k]
        if n == 0:
            assert np.isnan(want["mu"][k]) and np.isnan(want["sigma"][k])
            continue
        assert np.isfinite(r).all()
        d_sum, d_sq = 2 * (n - 1) * U * np.abs(r).sum(), 2 * (n - 1) * U * (r * r).sum()
        mu_np, sd_np = r.mean(), r.std()
        d_mu = d_sum / n + 2 * U * abs(mu_np)
        second = (r * r).sum() / n + mu_np * mu_np
        d_var = d_sq / n + 2 * abs(mu_np) * d_mu + d_mu * d_mu + 8 * U * second + (n + 3) * U * sd_np * sd_np
        print(f"sensor {k}: n {n}  |mu - numpy| {abs(want['mu'][k] - mu_np):.3e} (bound {d_mu:.3e})  "
              f"|sigma - numpy| {abs(want['sigma'][k] - sd_np):.3e} (bound {d_var / (want['sigma'][k] + sd_np) + 2 * U * sd_np:.3e})")
        assert abs(want["mu"][k] - mu_np) <= d_mu
        assert abs(want["sigma"][k] - sd_np) <= d_var / (want["sigma"][k] + sd_np) + 2 * U * sd_np
    if gaps:
        assert want["counts"][0] == 0 and want["counts"][1] == S                # TC.availability's sensors 0 and 1
    else:
        assert (want["counts"] == S).all() and (want["sigma"] > 0).all()
    back = pkg.MonitorBaseline.from_state_dict(mb.state_dict(), device=DEV)
    assert back.device == torch.device(DEV) and torch.equal(back.mu[1:], mb.mu[1:]) and torch.equal(back.sigma[1:], mb.sigma[1:])
    assert torch.equal(back.inv_sigma[1:], mb.inv_sigma[1:])


# ---- 5. monitor, monitor_store and estimate_monitored against the pass written out --------------------------------------------------
def compare_result(res, want, paths, what):
    np.testing.assert_array_equal(host(res.available_out), want["available_out"], err_msg=what)
    np.testing.assert_array_equal(host(res.latched), want["latched"], err_msg=what)
    np.testing.assert_array_equal(host(res.latched_rec), want["latched_rec"], err_msg=what)
    np.testing.assert_array_equal(host(res.records0), want["records0"], err_msg=what)
    np.testing.assert_array_equal(host(res.state), want["state"], err_msg=what)
    assert res.latched.dtype == torch.int32 and res.latched_rec.dtype == torch.int64 and res.available_out.dtype == torch.uint8
    if paths:
        MR.same_floats(host(res.stat_pos), want["stat_pos"], what)
        MR.same_floats(host(res.stat_neg), want["stat_neg"], what)
    else:
        assert res.stat_pos is None and res.stat_neg is None


def monitor_against_the_pass_written_out(pkg, est, store, observed, label, T_values=(12, 4), rounds=(1, 2)):
    """``store``: S = 12 clean snapshots; the baseline is calibrated on them, ramps are planted on two sensors."""
    S, K, n = len(store), len(observed), store.nodes_per_graph
    mb = est.calibrate_monitor(store)
    mu, inv, sigma = host(mb.mu).copy(), host(mb.inv_sigma).copy(), host(mb.sigma).copy()
    assert np.isfinite(inv).all() and (sigma > 0).all()
    readings = store.descale(store.data[:, observed]).contiguous()
    ramp = np.zeros((S, K), dtype=np.float32)
    ramp[2:, 2] = 2.0 * sigma[2] * np.arange(1, S - 1)             # sensor 2 climbs from row 2 on
    ramp[6:, 5] = -3.0 * sigma[5] * np.arange(1, S - 5)            # sensor 5 falls from row 6 on
    drifted = (readings + dev(ramp)).contiguous()
    latches = 0
    for T in T_values:
        for R in rounds:
            for since, min_sensors, av, with_state in (("onset", 1, None, False), ("alarm", K - 1, None, True),
                                                       ("onset", 2, TC.availability(S, K, 0.3, seed=4), False)):
                E, t0 = S // T, (25 if with_state else 0)
                d_av = None if av is None else dev(av)
                state = carried_state(E, K, t0, 3) if with_state else None
                what = f"{label} T{T} R{R} since {since} min{min_sensors} av{av is not None} state{with_state}"

                def residuals(a):
                    return host(est.loo_residuals(drifted, available=dev(a))[0]).copy()

                want = pkg.monitor_ref(residuals, mu, inv, np.ones((S, K), np.uint8) if av is None else av, T, t0, 0.5, 2.0, R,
                                       min_sensors, pkg.monitoring.SINCE[since], state)
                kw = dict(kappa=0.5, threshold=2.0, series_length=T, first_index=t0, max_latch=R, min_sensors=min_sensors,
                          since=since, available=d_av, state=None if state is None else dev(state))
                res = est.monitor(drifted, mb, paths=True, **kw)
                compare_result(res, want, True, what)
                assert res.latched.shape == (E, R) and res.latched_rec.shape == (E, R, 6) and res.state.shape == (E, K, 4)
                latches += int((want["latched"] >= 0).sum())
                out = torch.empty((S, n), dtype=torch.float32, device=DEV)
                e, res2 = est.estimate_monitored(drifted, mb, out=out, **kw)
                assert e is out
                compare_result(res2, want, False, what)
                assert torch.equal(e, est.estimate(drifted, available=dev(want["available_out"])))
    # the store entry point: the store's own readings, through loo_residuals_store
    def residuals_store(a):
        return host(est.loo_residuals_store(store, available=dev(a))[0]).copy()

    want = pkg.monitor_ref(residuals_store, mu, inv, np.ones((S, K), np.uint8), T_values[-1], 0, 0.25, 0.5, rounds[-1], 1, 0, None)
    res = est.monitor_store(store, mb, kappa=0.25, threshold=0.5, series_length=T_values[-1], max_latch=rounds[-1], paths=True)
    compare_result(res, want, True, label + " store")
    print(f"{label}: {latches} latches over the cases; the store pass latched {int((want['latched'] >= 0).sum())}")
    assert latches > 0
    return mb, drifted


@pytest.mark.parametrize("n,pipes,nc", [(37, 43, 8), (40, 47, 16)])
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "per_op"])
def test_monitor_equals_the_pass_written_out_fp32(pkg, oracle, fused, n, pipes, nc):
    store = make_store(pkg, 12, n, pipes)
    model, _ = build(pkg, oracle, 2, nc, seed=3, fused=fused)
    est = pkg.PressureEstimator.for_store(model, store, OBS8, batch_size=4)
    mb, drifted = monitor_against_the_pass_written_out(pkg, est, store, OBS8, f"n{n} nc{nc} {'fused' if fused else 'per-op'}")
    # the shift estimate: sigma[k*] * sum q / (65536 n), where something was latched
    res = est.monitor(drifted, mb, threshold=2.0, max_latch=2)
    lat, rec, shift = host(res.latched), host(res.latched_rec), host(res.shift(mb))
    sigma = host(mb.sigma)
    assert shift.shape == lat.shape and (lat >= 0).any()
    for e in range(lat.shape[0]):
        for r in range(lat.shape[1]):
            if lat[e, r] >= 0:
                assert shift[e, r] == sigma[lat[e, r]] * (float(rec[e, r, 4]) / (65536.0 * float(rec[e, r, 3])))
            else:
                assert np.isnan(shift[e, r])


def test_monitor_equals_the_pass_written_out_bf16(pkg, oracle):
    store = make_store(pkg, 12, 37, 43)
    model, _ = build(pkg, oracle, 2, 32, seed=3, fused=False)
    model.set_compute_dtype("bf16")
    est = pkg.PressureEstimator.for_store(model, store, OBS8, batch_size=4)
    monitor_against_the_pass_written_out(pkg, est, store, OBS8, "n37 nc32 bf16 per-op", T_values=(4,), rounds=(2,))


def test_gatres_small_at_batch_32_on_the_window_kernel(pkg, oracle):
    n, pipes, S = 388, 430, 12
    store = make_store(pkg, S, n, pipes, seed=4)
    model, _ = build(pkg, oracle, 15, 32, seed=11)
    plan = model.plan_for(store.edge_index(32), 32 * n)
    assert model._call_state(plan)["window"], "gatres_small at bs 32 should take the window kernel"
    est = pkg.PressureEstimator.for_store(model, store, SENSORS388, batch_size=32)
    assert (S * len(SENSORS388)) % 32 != 0                       # a ragged last batch
    monitor_against_the_pass_written_out(pkg, est, store, SENSORS388, "n388 gatres_small window", T_values=(4,), rounds=(2,))


# ---- 6. an exact end-to-end case resting on locality --------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "per_op"])
def test_a_far_drift_is_found_at_its_onset_and_nothing_else_moves(pkg, oracle, fused):
    n, pipes, nb, S, bs = 40, 47, 1, 12, 4
    sensors, K = MR.FAR_SENSORS, len(MR.FAR_SENSORS)
    dist = R.graph_distances(topology(pkg, n, pipes).numpy(), n)[np.ix_(sensors, sensors)]
    assert (dist[~np.eye(K, dtype=bool)] > 3 * nb).all()        # nothing moves beyond 3 hops per block (test_gpu_sensitivity.py)
    store = make_store(pkg, S, n, pipes)
    model, _ = build(pkg, oracle, nb, 8, seed=3, fused=fused)
    est = pkg.PressureEstimator.for_store(model, store, sensors, batch_size=bs)
    clean = readings_of(pkg, S, n, sensors)
    resid_clean = host(est.loo_residuals(clean)[0]).copy()
    assert np.isfinite(resid_clean).all()
    worst = np.abs(resid_clean).max(axis=0).astype(np.float64)
    assert (worst > 0).all()
    # mu = 0, sigma = twice the worst clean residual, kappa = 1: every clean |z| is about 1/2, every step falls, the statistics
    # are exactly 0 everywhere and nothing exceeds a threshold of 0
    mb = pkg.MonitorBaseline(np.zeros(K), 2 * worst, np.full(K, float(S)), sensors, device=DEV)
    res = est.monitor(clean, mb, kappa=1.0, threshold=0.0, max_latch=2, paths=True)
    assert (host(res.latched) == -1).all() and (host(res.available_out) == 1).all() and (host(res.latched_rec) == 0).all()
    assert (host(res.stat_pos) == 0).all() and (host(res.stat_neg) == 0).all()
    np.testing.assert_array_equal(host(res.records0)[0, :, 0], np.full(K, -1))
    np.testing.assert_array_equal(host(res.state)[0], np.tile(np.int64([0, 0, S, S]), (K, 1)))
    k_star, onset = 3, 5
    drifted = clean.clone()
    ramp = np.zeros(S, dtype=np.float32)
    ramp[onset:] = np.float32(3 * 2 * worst[k_star]) * np.arange(1, S - onset + 1, dtype=np.float32)
    drifted[:, k_star] += dev(ramp)
    got = host(est.loo_residuals(drifted)[0]).copy()
    moved = np.zeros((S, K), dtype=bool)
    moved[onset:, k_star] = True
    np.testing.assert_array_equal(got.view(np.int32)[~moved], resid_clean.view(np.int32)[~moved])        # nothing else moved
    res = est.monitor(drifted, mb, kappa=1.0, threshold=0.0, paths=True)
    rec = host(res.latched_rec)[0, 0]
    assert host(res.latched).tolist() == [[k_star]] and rec[0] == onset and rec[1] == 1 and rec[2] == onset and rec[3] == 1
    without = np.ones((S, K), dtype=np.uint8)
    without[onset:, k_star] = 0
    np.testing.assert_array_equal(host(res.available_out), without)
    pos = host(res.stat_pos)
    assert (pos[:, np.arange(K) != k_star] == 0).all() and (pos[:onset, k_star] == 0).all() and (np.diff(pos[onset - 1:, k_star]) > 1).all()
    assert 2.0 < float(res.shift(mb)[0, 0]) / (2 * worst[k_star]) < 4.0             # about the first step of the ramp
    e, res2 = est.estimate_monitored(drifted, mb, kappa=1.0, threshold=0.0)
    assert host(res2.latched).tolist() == [[k_star]]
    assert torch.equal(e, est.estimate(drifted, available=dev(without)))
    assert not torch.equal(e, est.estimate(drifted))


# ---- 7. the back-test -----------------------------------------------------------------------------------------------------------------
def test_monitoring_report_equals_its_passes_written_out(pkg, oracle):
    store, _, est = calibration_case(pkg, oracle)
    S, K, T = len(store), len(OBS8), 8
    E = S // T
    mb = est.calibrate_monitor(store)
    rate = (2.0 * host(mb.sigma)).tolist()
    kw = dict(threshold=3.0, max_latch=2)
    rep = est.monitoring_report(store, mb, series_length=T, drift_rate=rate, drift_share=0.67, min_lead=2, seed=3, **kw)
    draws = pkg.drift_draws(3, E, T, K, 0.67, 2)
    np.testing.assert_array_equal(rep["draws"], draws)
    assert (draws[:, 0] >= 0).sum() == 2
    readings = store.descale(store.data[:, OBS8]).contiguous()
    drifted = (readings + dev(pkg.drift_offsets(draws, T, K, rate))).contiguous()
    without = np.ones((S, K), dtype=np.uint8)
    for e, (k, onset) in enumerate(draws.tolist()):
        if k >= 0:
            without[e * T + onset:(e + 1) * T, k] = 0
    monitored, res = est.estimate_monitored(drifted, mb, series_length=T, **kw)
    latched, latched_rec = host(res.latched).copy(), host(res.latched_rec).copy()
    want = {"clean": est.estimate(readings), "drifted": est.estimate(drifted), "monitored": monitored,
            "oracle": est.estimate(drifted, available=dev(without))}
    for name, e in want.items():
        assert rep["nonsensor_mae"][name] == float(est.error_map(store, estimates=e)["hidden_mae"]), name
    np.testing.assert_array_equal(rep["latched"], latched)
    np.testing.assert_array_equal(rep["latched_rec"], latched_rec)
    assert rep["latched"].dtype == np.int64 and rep["latched_rec"].shape == (E, 2, 6)
    rates = pkg.monitoring_rates(latched_rec, latched, draws)
    for name, v in rates.items():
        assert rep[name] == v or (np.isnan(v) and np.isnan(rep[name])), name
    print("monitoring_report:", {k: v for k, v in rep.items() if k not in ("draws", "latched", "latched_rec")})
    assert rep["num_drifted"] == 2 and rep["num_clean"] == 1 and rep["detection_rate"] > 0
    m = rep["nonsensor_mae"]
    assert m["drifted"] != m["clean"] and all(np.isfinite(v) for v in m.values())
    one = est.monitoring_report(store, mb, series_length=S, drift_rate=1.0, drift_share=1.0, seed=1)
    assert one["num_clean"] == 0 and np.isnan(one["false_alarm_rate_clean"]) and one["latched"].shape == (1, 1)


# ---- 8. read-backs and allocations ----------------------------------------------------------------------------------------------------
def test_no_read_back_no_allocation_and_the_counted_read_backs(pkg, oracle, monkeypatch):
    store, _, est = calibration_case(pkg, oracle)
    n, S, K = store.nodes_per_graph, 12, len(OBS8)
    mb = est.calibrate_monitor(store)
    readings = readings_of(pkg, S, n, OBS8, seed=2)
    readings[4:, 2] += 40.0
    d_av = dev(TC.availability(S, K, 0.3, seed=4))
    out = torch.empty((S, n), dtype=torch.float32, device=DEV)
    carried = dev(carried_state(3, K, 9, 1))

    def passes():
        a = est.monitor(readings, mb, series_length=4, max_latch=2, available=d_av, paths=True)
        keep = (a.latched.clone(), a.state.clone(), a.stat_pos.clone())
        b = est.monitor(readings, mb, series_length=4, max_latch=2, first_index=9, state=carried, since="alarm")
        b = est.monitor(readings, mb, series_length=4, max_latch=2, first_index=21, state=b.state)      # its own scratch as the state
        e, c = est.estimate_monitored(readings, mb, out=out, series_length=4, threshold=2.0, max_latch=2, min_sensors=2)
        return keep + (b.state, e, c.latched, c.available_out)

    small = pkg.SnapshotStore(raw_snapshots(pkg, S, n, 2), topology(pkg, n, 43), device=DEV, mean=store.mean, std=store.std)
    est.monitoring_report(small, mb, series_length=4, drift_rate=5.0, max_latch=2)
    est.monitor_store(small, mb, series_length=4, max_latch=2)
    first = passes()
    first = tuple(t.clone() for t in passes())                  # plans, layouts and scratch exist from here on; the scratch is
                                                                # kept while its shapes stay: every call below has E = 3, R = 2
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
    est.monitor(readings, mb, series_length=4, max_latch=2, available=d_av, paths=True)
    b = est.monitor(readings, mb, series_length=4, max_latch=2, first_index=9, state=carried, since="alarm")
    est.monitor(readings, mb, series_length=4, max_latch=2, first_index=21, state=b.state)
    est.monitor_store(small, mb, series_length=4, max_latch=2)
    est.estimate_monitored(readings, mb, out=out, series_length=4, threshold=2.0, max_latch=2, min_sensors=2)
    allocated = torch.cuda.memory_stats(DEV)["allocation.all.allocated"] - before
    assert all(v == 0 for v in calls.values()), calls
    assert allocated == 0, allocated
    est.calibrate_monitor(small)
    assert calls == {"synchronize": 0, "item": 0, "cpu": 1, "tolist": 0, "float": 0, "stream_sync": 0, "event_sync": 0}
    est.monitoring_report(small, mb, series_length=4, drift_rate=5.0, max_latch=2)
    assert calls == {"synchronize": 0, "item": 0, "cpu": 5, "tolist": 0, "float": 0, "stream_sync": 0, "event_sync": 0}
    monkeypatch.undo()
    again = passes()
    for got, want in zip(again, first):
        if got.dtype == torch.float32:
            MR.same_floats(host(got), host(want))
        else:
            assert torch.equal(got, want)


# ---- 9. the refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_on_the_device(pkg, oracle):
    store, model, est = calibration_case(pkg, oracle)
    S, K, n = 12, len(OBS8), store.nodes_per_graph
    mb = est.calibrate_monitor(store)
    good = torch.zeros((S, K), dtype=torch.float32, device=DEV)
    for bad in (good.cpu(), good.double(), good[:, :2], good.reshape(-1), good[:0]):
        for call in (lambda b: est.monitor(b, mb), lambda b: est.estimate_monitored(b, mb)):
            with pytest.raises(ValueError, match="readings"):
                call(bad)
    av = torch.ones((S, K), dtype=torch.uint8, device=DEV)
    for bad in (av[:2], av.float(), av.cpu()):
        with pytest.raises(ValueError, match="available"):
            est.monitor(good, mb, available=bad)
    with pytest.raises(ValueError, match="available"):
        est.monitor_store(store, mb, available=av)              # [len(store), K] is what it takes
    with pytest.raises(ValueError, match="available"):
        est.calibrate_monitor(store, available=av)
    single = pkg.PressureEstimator.for_store(model, store, [5], batch_size=4)
    one = pkg.MonitorBaseline([0.0], [1.0], [1.0], [5], device=DEV)
    for call in (lambda: single.monitor(torch.zeros((S, 1), device=DEV), one), lambda: single.calibrate_monitor(store),
                 lambda: single.monitoring_report(store, one, series_length=8, drift_rate=1.0)):
        with pytest.raises(ValueError, match="two sensors"):
            call()
    other = pkg.MonitorBaseline(mb.mu.clone(), mb.sigma.clone(), mb.counts.clone(), OBS8[::-1])
    with pytest.raises(ValueError, match="sensors"):
        est.monitor(good, other)
    with pytest.raises(ValueError, match="must be on"):
        est.monitor(good, pkg.MonitorBaseline.from_state_dict(mb.state_dict()))      # on the host
    with pytest.raises(ValueError, match="MonitorBaseline"):
        est.monitor(good, est.calibrate_screening(store, (0.9,)))
    for bad in (-1.0, 32768.5, float("nan")):
        with pytest.raises(ValueError, match="kappa"):
            est.monitor(good, mb, kappa=bad)
        with pytest.raises(ValueError, match="threshold"):
            est.estimate_monitored(good, mb, threshold=bad)
        with pytest.raises(ValueError, match="threshold"):
            est.monitoring_report(store, mb, series_length=8, drift_rate=1.0, threshold=bad)
    for bad in (5, 0, 24, 4.0):
        with pytest.raises(ValueError, match="series_length"):
            est.monitor(good, mb, series_length=bad)
    with pytest.raises(ValueError, match="series_length"):
        est.monitoring_report(store, mb, series_length=7, drift_rate=1.0)
    with pytest.raises(ValueError, match="first_index"):
        est.monitor(good, mb, first_index=-1)
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="max_latch"):
            est.monitor(good, mb, max_latch=bad)
    for bad in (0, K + 1, 2.0):
        with pytest.raises(ValueError, match="min_sensors"):
            est.estimate_monitored(good, mb, min_sensors=bad)
    with pytest.raises(ValueError, match="since"):
        est.monitor(good, mb, since="both")
    state = torch.zeros((1, K, 4), dtype=torch.int64, device=DEV)
    for bad in (state.cpu(), state.int(), state[:, :2], torch.zeros((2, K, 4), dtype=torch.int64, device=DEV)):
        with pytest.raises(ValueError, match="state"):
            est.monitor(good, mb, state=bad)
    with pytest.raises(ValueError, match="out must"):
        est.estimate_monitored(good, mb, out=torch.empty((S, n + 1), device=DEV))
    for bad in ([1.0, 2.0], float("nan"), "x"):
        with pytest.raises(ValueError, match="drift_rate"):
            est.monitoring_report(store, mb, series_length=8, drift_rate=bad)
    with pytest.raises(ValueError, match="share"):
        est.monitoring_report(store, mb, series_length=8, drift_rate=1.0, drift_share=1.5)
    with pytest.raises(ValueError, match="min_lead"):
        est.monitoring_report(store, mb, series_length=8, drift_rate=1.0, min_lead=4)
    with pytest.raises(ValueError, match="nodes per graph"):
        est.monitor_store(make_store(pkg, 2, 40, 47), mb)
    multi = pkg.MultiSnapshotStore([(raw_snapshots(pkg, 3, n), topology(pkg, n, 43))] * 2, device="cpu")
    for call in (lambda: est.monitor_store(multi, mb), lambda: est.calibrate_monitor(multi),
                 lambda: est.monitoring_report(multi, mb, series_length=3, drift_rate=1.0)):
        with pytest.raises(ValueError, match="MultiSnapshotStore"):
            call()
