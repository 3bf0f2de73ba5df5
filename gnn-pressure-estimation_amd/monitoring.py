"""The drift monitor of sensor readings of ``estimation.PressureEstimator`` (``calibrate_monitor`` / ``monitor`` /
``estimate_monitored`` / ``monitoring_report``) restated on the host, in numpy, without a device: the two launches of
csrc/k_monitor.hip (include/gatres.h states them), the rounds of ``monitor``, the baseline from a moments table, the draws of the
back-test and its rates.  The CUSUM state is integer (units of 2^-16 sigma), walked by a plain sequential loop in Python integers;
fp32 values are formed with one rounding per operation, as the kernels form them."""
from __future__ import annotations

from typing import Callable, Dict, Optional, Tuple

import numpy as np

CUSUM_STATE, CUSUM_RECORD = 4, 6               # GATRES_CUSUM_STATE, GATRES_CUSUM_RECORD
CUSUM_ONE = 65536                              # the fixed point: one sigma
CUSUM_ARG_MAX = 32768.0                        # kappa and the threshold lie in [0, 32768] sigma
CUSUM_FLOOR = -(1 << 62)                       # C of the identity of ``cusum_compose``
CUSUM_IDENTITY = (0, CUSUM_FLOOR)
_STATE_MAX = 1 << 61
SINCE = {"onset": 0, "alarm": 1}               # monitor(since=...): the `since` of gatres_monitor_latch


def cusum_fixed(kappa) -> int:
    """``llrint(kappa * 65536.0)``: an allowance or a threshold in sigma as the int64 the launches take.  One fp64 product, rounded
    to the nearest integer, ties to even.  A value outside ``[0, 32768]`` (a NaN included) is a ``ValueError``."""
    try:
        v = float(kappa)
    except (TypeError, ValueError):
        raise ValueError(f"a number in [0, {CUSUM_ARG_MAX:g}] is needed; got {kappa!r}") from None
    if isinstance(kappa, bool) or not 0.0 <= v <= CUSUM_ARG_MAX:
        raise ValueError(f"a number in [0, {CUSUM_ARG_MAX:g}] is needed; got {kappa!r}")
    return int(np.rint(np.float64(v) * 65536.0))


def cusum_compose(x, y) -> Tuple[int, int]:
    """The pair operator of the scan: ``(A, C)`` is the map ``g -> max(C, g + A)``, one counted step of a side is ``(a, 0)``,
    and ``cusum_compose(x, y)`` is "x, then y": ``(A1 + A2, max(C2, C1 + A2))``.  Associative; ``CUSUM_IDENTITY`` is neutral for
    every map a run of steps composes to and for statistics >= 0."""
    return int(x[0]) + int(y[0]), max(int(y[1]), int(x[1]) + int(y[0]))


def _ll2float(v: int) -> np.float32:
    """``__ll2float_rn``: an integer to fp32 with ONE rounding (through fp64 it would round twice above 2^53)."""
    v = int(v)
    if abs(v) < (1 << 53):
        return np.float32(np.float64(v))
    shift = abs(v).bit_length() - 53
    top = abs(v) >> shift
    if abs(v) & ((1 << shift) - 1):
        top |= 1                               # (round to odd: 53 bits keep what the rounding to 24 needs)
    f = np.ldexp(np.float32(np.float64(top)), shift).astype(np.float32)
    return np.float32(-f) if v < 0 else np.float32(f)


def cusum_entries(resid, mu, inv_sigma, available=None) -> Tuple[np.ndarray, np.ndarray]:
    """``(counted bool [S, K], q int64 [S, K])`` of ``gatres_cusum_scan``: an entry is counted when it is available, its residual
    is no NaN and ``z = fp32(fp32(resid - mu[k]) * inv_sigma[k])`` is no NaN; z is clamped to +-32768 and
    ``q = llrint(z * 65536)`` (0 where the entry is not counted)."""
    resid = np.asarray(resid, dtype=np.float32)
    mu, inv_sigma = np.asarray(mu, dtype=np.float32), np.asarray(inv_sigma, dtype=np.float32)
    if resid.ndim != 2 or mu.shape != (resid.shape[1],) or inv_sigma.shape != mu.shape:
        raise ValueError("resid must be [S, K], mu and inv_sigma [K]")
    with np.errstate(invalid="ignore", over="ignore"):
        z = ((resid - mu[None, :]).astype(np.float32) * inv_sigma[None, :]).astype(np.float32)
    counted = ~np.isnan(resid) & ~np.isnan(z)
    if available is not None:
        here = np.asarray(available) != 0
        if here.shape != resid.shape:
            raise ValueError(f"available must be {list(resid.shape)}")
        counted &= here
    z = np.clip(np.where(counted, z, np.float32(0)), np.float32(-32768.0), np.float32(32768.0))
    return counted, np.rint(z.astype(np.float64) * 65536.0).astype(np.int64)


def _series(S: int, T) -> Tuple[int, int]:
    T = int(T)
    if T < 1 or S < 1 or S % T:
        raise ValueError(f"the {S} rows are no whole number of series of length {T}")
    return S // T, T


def cusum_scan_ref(resid, mu, inv_sigma, available, T, first_index, kappa, h, state=None, paths: bool = True):
    """``gatres_cusum_scan`` on the host, as the sequential loop.  ``resid`` fp32 ``[S, K]`` read as ``E = S / T`` series of ``T``
    rows; ``first_index`` the global index of row 0 of every series; ``kappa`` and ``h`` in sigma (``cusum_fixed`` makes the
    integers); ``state``: int64 ``[E, K, 4]`` = ``{P, M, zP, zM}`` or ``None`` for ``{0, 0, t0, t0}``.  Returns ``(state_out
    int64 [E, K, 4], records int64 [E, K, 6], stat_pos, stat_neg fp32 [S, K]`` (``None`` without ``paths``)``)``; the record is
    ``[alarm, side, onset, n, sum q, statistic]`` as include/gatres.h states it."""
    counted, q = cusum_entries(resid, mu, inv_sigma, available)
    S, K = counted.shape
    E, T = _series(S, T)
    t0, kq, hq = int(first_index), cusum_fixed(kappa), cusum_fixed(h)
    if t0 < 0:
        raise ValueError("first_index must not be negative")
    if state is not None:
        state = np.asarray(state)
        if state.shape != (E, K, CUSUM_STATE) or state.dtype != np.int64:
            raise ValueError(f"state must be int64 [{E}, {K}, {CUSUM_STATE}]")
    state_out = np.zeros((E, K, CUSUM_STATE), dtype=np.int64)
    records = np.zeros((E, K, CUSUM_RECORD), dtype=np.int64)
    pos = np.zeros((S, K), dtype=np.float32) if paths else None
    neg = np.zeros((S, K), dtype=np.float32) if paths else None
    for e in range(E):
        for k in range(K):
            P, M, zP, zM = (0, 0, t0, t0) if state is None else (int(v) for v in state[e, k])
            P, M = min(max(P, 0), _STATE_MAX), min(max(M, 0), _STATE_MAX)
            alarm, side, onset, stat = -1, 0, 0, 0
            col_c, col_q = counted[e * T:(e + 1) * T, k].tolist(), q[e * T:(e + 1) * T, k].tolist()
            path_p, path_m = [0] * T, [0] * T
            for t in range(T):
                if col_c[t]:
                    tau = t0 + t
                    P, M = max(0, P + col_q[t] - kq), max(0, M - col_q[t] - kq)
                    if P == 0:
                        zP = tau + 1
                    if M == 0:
                        zM = tau + 1
                    if alarm < 0 and (P > hq or M > hq):
                        plus = P > hq and (not M > hq or P >= M)
                        alarm, side, onset, stat = tau, (1 if plus else -1), (zP if plus else zM), (P if plus else M)
                path_p[t], path_m[t] = P, M
            state_out[e, k] = [P, M, zP, zM]
            if alarm >= 0:
                a, b = max(onset, t0) - t0, alarm - t0 + 1
                n = sum(1 for t in range(a, b) if col_c[t])
                sq = sum(col_q[t] for t in range(a, b) if col_c[t])
                records[e, k] = [alarm, side, onset, n, sq, stat]
            else:
                records[e, k, 0] = -1
            if paths:
                for path, dst in ((path_p, pos), (path_m, neg)):
                    small = max(path) < (1 << 53)
                    col = np.asarray(path, dtype=np.float64).astype(np.float32) if small else \
                        np.asarray([_ll2float(v) for v in path], dtype=np.float32)
                    dst[e * T:(e + 1) * T, k] = col * np.float32(1.0 / 65536.0)
    return state_out, records, pos, neg


def monitor_latch_ref(records, available, T, first_index, latched_before=None, since: int = 0, min_sensors: int = 1):
    """One round of ``gatres_monitor_latch`` on the host.  ``records`` int64 ``[E, K, 6]``, ``available`` ``[E * T, K]``,
    ``latched_before`` int ``[E, round]`` (the earlier rounds' columns; ``None``: round 0).  Sensor ``k`` is a candidate of series
    ``e`` when ``records[e, k, 0] >= 0`` and it is not in ``latched_before[e]``; the one with the smallest alarm index is chosen,
    ties to the larger ``records[.., 5]``, then to the smaller ``k``, if ``K - #{latched_before[e] >= 0} - 1 >= min_sensors``.
    Its column of ``available`` is zeroed for the rows of the series with ``tau >= max(onset, first_index)`` (``since == 0``) or
    ``tau >= alarm`` (``since == 1``).  Returns ``(available uint8 [E * T, K]`` after the round, ``latched int32 [E]`` (-1:
    none), ``latched_rec int64 [E, 6]`` (zeros: none)``)``."""
    records = np.asarray(records, dtype=np.int64)
    if records.ndim != 3 or records.shape[2] != CUSUM_RECORD:
        raise ValueError(f"records must be [E, K, {CUSUM_RECORD}]")
    E, K = records.shape[:2]
    avail = (np.asarray(available) != 0).astype(np.uint8)
    T, t0 = int(T), int(first_index)
    if avail.shape != (E * T, K):
        raise ValueError(f"available must be [{E * T}, {K}]")
    if since not in (0, 1):
        raise ValueError("since must be 0 (onset) or 1 (alarm)")
    if int(min_sensors) < 1:
        raise ValueError("min_sensors must be at least 1")
    before = np.full((E, 0), -1, dtype=np.int64) if latched_before is None else np.asarray(latched_before, dtype=np.int64)
    if before.ndim != 2 or before.shape[0] != E:
        raise ValueError(f"latched_before must be [{E}, round]")
    latched = np.full(E, -1, dtype=np.int32)
    latched_rec = np.zeros((E, CUSUM_RECORD), dtype=np.int64)
    for e in range(E):
        cand = [k for k in range(K) if records[e, k, 0] >= 0 and k not in before[e].tolist()]
        if not cand or K - int((before[e] >= 0).sum()) - 1 < int(min_sensors):
            continue
        k = min(cand, key=lambda c: (int(records[e, c, 0]), -int(records[e, c, 5]), c))
        latched[e], latched_rec[e] = k, records[e, k]
        start = int(records[e, k, 2]) if since == 0 else int(records[e, k, 0])
        avail[e * T + min(max(start - t0, 0), T):(e + 1) * T, k] = 0
    return avail, latched, latched_rec


def monitor_ref(residuals: Callable[[np.ndarray], np.ndarray], mu, inv_sigma, available, T, first_index, kappa, h,
                max_latch: int = 1, min_sensors: int = 1, since: int = 0, state=None) -> Dict[str, np.ndarray]:
    """The rounds of ``PressureEstimator.monitor``: ``max_latch`` times ``resid = residuals(available)`` (the leave-one-out
    residuals under the current availability, ``[S, K]``), one ``cusum_scan_ref`` from ``state`` and one ``monitor_latch_ref``.
    Returns a dict: ``available_out``, ``latched [E, R]``, ``latched_rec [E, R, 6]``, ``records0``, ``stat_pos`` / ``stat_neg``
    (round 0) and ``state`` (the last round's)."""
    R = int(max_latch)
    if R < 1:
        raise ValueError("max_latch must be at least 1")
    avail = (np.asarray(available) != 0).astype(np.uint8)
    E, T = _series(avail.shape[0], T)
    latched = np.full((E, R), -1, dtype=np.int32)
    latched_rec = np.zeros((E, R, CUSUM_RECORD), dtype=np.int64)
    out = {}
    for rnd in range(R):
        resid = np.asarray(residuals(avail.copy()), dtype=np.float32)
        state_out, records, pos, neg = cusum_scan_ref(resid, mu, inv_sigma, avail, T, first_index, kappa, h, state, paths=rnd == 0)
        if rnd == 0:
            out.update(records0=records, stat_pos=pos, stat_neg=neg, resid0=resid)
        avail, latched[:, rnd], latched_rec[:, rnd] = monitor_latch_ref(records, avail, T, first_index, latched[:, :rnd], since,
                                                                        min_sensors)
    out.update(available_out=avail, latched=latched, latched_rec=latched_rec, state=state_out)
    return out


def monitor_baseline_from_moments(table) -> Dict[str, np.ndarray]:
    """The in-control mean and spread of every sensor's leave-one-out residual from a ``gatres_node_error_moments`` (or
    ``..._available``) table ``[K, 8]`` over the ``[S, K]`` matrices, in fp64.  The table's ``e`` is prediction - reading and the
    residual is reading - prediction, so ``mu = -sum e / n``; ``sigma = sqrt(max(sum e^2 / n - mu^2, 0))`` and ``inv_sigma =
    float32(1 / sigma)``.  ``counts`` is ``n`` (slot 0).  A sensor without samples has NaN ``mu`` and ``sigma``: it is never
    counted."""
    t = np.asarray(table, dtype=np.float64).reshape(-1, 8)
    n = t[:, 0]
    with np.errstate(invalid="ignore", divide="ignore"):
        mu = -t[:, 1] / n
        sigma = np.sqrt(np.maximum(t[:, 3] / n - mu * mu, 0.0))
        inv = (1.0 / sigma).astype(np.float32)
    return {"mu": mu, "sigma": sigma, "inv_sigma": inv, "counts": n.copy()}


def drift_draws(seed: int, E: int, T: int, K: int, share: float, min_lead: int) -> np.ndarray:
    """The drifts of ``monitoring_report``: int64 ``[E, 2]``, per series the drifting sensor and the onset row, ``[-1, -1]`` for a
    clean series.  ``round(share * E)`` series, chosen without replacement by ``numpy.random.default_rng(seed)``, get one sensor
    (uniform in ``[0, K)``) and then one onset (uniform in ``[min_lead, T - min_lead)``) each, by the same generator."""
    E, T, K, min_lead = int(E), int(T), int(K), int(min_lead)
    if E < 1 or T < 1 or K < 1:
        raise ValueError("drift_draws needs E >= 1, T >= 1 and K >= 1")
    if not 0.0 <= float(share) <= 1.0:
        raise ValueError(f"share must lie in [0, 1]; got {share!r}")
    if min_lead < 0 or T - min_lead <= min_lead:
        raise ValueError(f"min_lead must leave an onset in [min_lead, T - min_lead); got {min_lead} with T = {T}")
    rng = np.random.default_rng(seed)
    n = min(E, int(round(float(share) * E)))
    series = np.sort(rng.choice(E, size=n, replace=False))
    draws = np.full((E, 2), -1, dtype=np.int64)
    draws[series, 0] = rng.integers(0, K, size=n)
    draws[series, 1] = rng.integers(min_lead, T - min_lead, size=n)
    return draws


def drift_offsets(draws, T: int, K: int, rate) -> np.ndarray:
    """The planted ramps: fp32 ``[E * T, K]``, ``float32(rate[k]) * float32(t - onset + 1)`` (one rounding) in column ``k`` of
    series ``e`` from its onset row on, where ``draws[e] = [k, onset]``; 0 elsewhere.  ``rate``: one value or ``K``."""
    draws = np.asarray(draws, dtype=np.int64)
    T, K = int(T), int(K)
    if draws.ndim != 2 or draws.shape[1] != 2:
        raise ValueError("draws must be [E, 2]")
    try:
        rate = np.asarray(rate, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"drift_rate must be a number or a sequence of {K} of them") from None
    if rate.ndim == 0:
        rate = np.full(K, float(rate))
    if rate.shape != (K,) or not np.isfinite(rate).all():
        raise ValueError(f"drift_rate must be a finite number or a sequence of {K} of them, one per sensor")
    rate = rate.astype(np.float32)
    E = draws.shape[0]
    out = np.zeros((E * T, K), dtype=np.float32)
    for e, (k, onset) in enumerate(draws.tolist()):
        if k >= 0:
            if not (0 <= k < K and 0 <= onset < T):
                raise ValueError(f"draw {e} = [{k}, {onset}] lies outside [0, {K}) x [0, {T})")
            out[e * T + onset:(e + 1) * T, k] = rate[k] * np.arange(1, T - onset + 1, dtype=np.float32)
    return out


def monitoring_rates(latched_rec, latched, draws) -> Dict[str, float]:
    """What a monitoring did, per series, from ``latched`` (int ``[E, R]``, -1: nothing), ``latched_rec`` (int64 ``[E, R, 6]``)
    and ``draws`` (``[E, 2]``, -1: a clean series): ``detection_rate`` (of the drifted series: the drifting sensor is among the
    latched), ``misidentification_rate`` (of the drifted series: something was latched, the drifting sensor was not),
    ``false_alarm_rate_clean`` (of the clean series: anything was latched), ``mean_delay`` / ``median_delay`` (alarm - true
    onset, over the detected), ``mean_onset_error`` (``|onset estimate - true onset|``, over the detected), with
    ``num_drifted`` and ``num_clean``.  Indices are rows of the series (``first_index`` taken off by the caller).  A rate or a
    mean over nothing is NaN."""
    lat = np.asarray(latched, dtype=np.int64)
    rec = np.asarray(latched_rec, dtype=np.int64)
    draws = np.asarray(draws, dtype=np.int64)
    if lat.ndim != 2 or rec.shape != lat.shape + (CUSUM_RECORD,) or draws.shape != (lat.shape[0], 2):
        raise ValueError("latched must be [E, R], latched_rec [E, R, 6] and draws [E, 2]")
    drifted, clean = draws[:, 0] >= 0, draws[:, 0] < 0
    match = (lat == draws[:, :1]) & drifted[:, None]
    hit = match.any(axis=1)
    some = (lat >= 0).any(axis=1)
    first = match.argmax(axis=1)
    mine = rec[np.arange(lat.shape[0]), first]                 # the record of the drifting sensor, where it was latched
    delay = (mine[:, 0] - draws[:, 1])[hit].astype(np.float64)
    onset_error = np.abs(mine[:, 2] - draws[:, 1])[hit].astype(np.float64)

    def rate(what, pool):
        return float(what[pool].mean()) if pool.any() else float("nan")

    def mean(v, f=np.mean):
        return float(f(v)) if v.size else float("nan")

    return {"detection_rate": rate(hit, drifted), "misidentification_rate": rate(some & ~hit, drifted),
            "false_alarm_rate_clean": rate(some, clean), "mean_delay": mean(delay), "median_delay": mean(delay, np.median),
            "mean_onset_error": mean(onset_error), "num_drifted": int(drifted.sum()), "num_clean": int(clean.sum())}
