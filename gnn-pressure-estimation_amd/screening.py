"""The screening of sensor readings of ``estimation.PressureEstimator`` (``loo_residuals`` / ``screen`` / ``estimate_screened`` /
``screening_report``) restated on the host, in numpy, without a device: the layouts of the leave-one-out pass, the two launches
of csrc/k_screen.hip (include/gatres.h states them), the rounds of ``screen``, the draws of the back-test and its rates.  fp32
values are formed with one rounding per operation, as the kernels form them."""
from __future__ import annotations

from typing import Callable, Dict, Tuple

import numpy as np

_NAN32 = np.array([0x7FC00000], dtype=np.uint32).view(np.float32)[0]      # the quiet NaN gatres_loo_residuals writes


def loo_layouts(K: int) -> np.ndarray:
    """The layouts of the leave-one-out pass: uint8 ``[K, K]``, all ones with a zero diagonal -- layout ``k`` is every sensor
    but ``k``."""
    K = int(K)
    if K < 2:
        raise ValueError(f"leave-one-out needs at least two sensors; got K={K}")
    return (1 - np.eye(K, dtype=np.uint8)).astype(np.uint8)


def loo_residuals_from_estimates(readings, est_per_sensor, present=None) -> Tuple[np.ndarray, np.ndarray]:
    """``gatres_loo_residuals`` on the host.  ``readings``: fp32 ``[S, K]`` in physical units; ``est_per_sensor``: fp32 ``[S, K]``,
    entry ``[s, k]`` the model's (descaled) prediction at the node of sensor ``k`` with sensor ``k`` hidden; ``present``: ``[S, K]``,
    zero where the reading is not there (``None``: every reading is).  Returns ``(resid, pred)``: ``resid = fp32(readings - pred)``,
    the quiet NaN 0x7fc00000 where the reading is not there."""
    r = np.asarray(readings, dtype=np.float32)
    pred = np.array(est_per_sensor, dtype=np.float32, copy=True)
    if r.ndim != 2 or pred.shape != r.shape:
        raise ValueError("readings and est_per_sensor must be [S, K]")
    with np.errstate(invalid="ignore", over="ignore"):
        resid = (r - pred).astype(np.float32)
    if present is not None:
        here = np.asarray(present) != 0
        if here.shape != r.shape:
            raise ValueError("present must be [S, K]")
        resid[~here] = _NAN32
    return resid, pred


def _score_keys(score: np.ndarray) -> np.ndarray:
    """The scores as unsigned keys in IEEE order (-0 below +0), a NaN score below everything: ``screen_key`` of k_screen.hip."""
    u = np.ascontiguousarray(score, dtype=np.float32).view(np.uint32)
    o = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    return np.where(np.isnan(score), np.uint32(0), o).astype(np.uint64)


def screen_reject_ref(resid, bound, available, min_sensors: int = 1) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """One round of ``gatres_screen_reject`` on the host.  ``resid`` fp32 ``[S, K]``, ``bound`` fp32 ``[K]``, ``available``
    ``[S, K]`` (non-zero: present).  Sensor ``k`` of snapshot ``s`` is a candidate when it is available, its residual is no NaN
    and ``|resid| > bound[k]`` in fp32 (a NaN or +inf bound never yields one); the candidate with the largest
    ``fp32(|resid| * (float32(1) / bound[k]))`` is rejected, ties to the smallest ``k``, if the snapshot keeps at least
    ``min_sensors`` available readings afterwards.  Returns ``(available uint8 [S, K]`` after the round, ``rejected int32 [S]``
    (-1: none), ``flagged uint8 [S, K]`` (the candidates)``)``."""
    resid = np.asarray(resid, dtype=np.float32)
    bound = np.asarray(bound, dtype=np.float32)
    if resid.ndim != 2 or bound.shape != (resid.shape[1],):
        raise ValueError("resid must be [S, K] and bound [K]")
    S, K = resid.shape
    avail = (np.asarray(available) != 0).astype(np.uint8)
    if avail.shape != (S, K):
        raise ValueError(f"available must be [{S}, {K}]")
    if int(min_sensors) < 1:
        raise ValueError("min_sensors must be at least 1")
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        inv = (np.float32(1.0) / bound).astype(np.float32)
        ar = np.abs(resid)
        cand = (avail != 0) & ~np.isnan(resid) & (ar > bound[None, :])
        score = (ar * inv[None, :]).astype(np.float32)
    key = (_score_keys(score) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.arange(K, dtype=np.uint64))[None, :]
    key = np.where(cand, key, np.uint64(0))
    best = key.argmax(axis=1)                                   # (keys are distinct among the candidates of a row)
    room = avail.sum(axis=1, dtype=np.int64) - 1 >= int(min_sensors)
    take = cand.any(axis=1) & room
    rejected = np.where(take, best, -1).astype(np.int32)
    avail[np.nonzero(take)[0], best[take]] = 0
    return avail, rejected, cand.astype(np.uint8)


def screen_ref(residuals: Callable[[np.ndarray], np.ndarray], bound, available, max_reject: int = 1,
               min_sensors: int = 1) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """The rounds of ``PressureEstimator.screen``: ``max_reject`` times ``resid = residuals(available)`` (the leave-one-out
    residuals under the current availability, ``[S, K]``) and one ``screen_reject_ref``.  Returns ``(available_out [S, K] uint8,
    rejected [S, max_reject] int32, resid0, flagged0)``, the last two from round 0."""
    R = int(max_reject)
    if R < 1:
        raise ValueError("max_reject must be at least 1")
    avail = (np.asarray(available) != 0).astype(np.uint8)
    rejected = np.full((avail.shape[0], R), -1, dtype=np.int32)
    resid0 = flagged0 = None
    for rnd in range(R):
        resid = np.asarray(residuals(avail.copy()), dtype=np.float32)
        avail, rejected[:, rnd], flagged = screen_reject_ref(resid, bound, avail, min_sensors)
        if rnd == 0:
            resid0, flagged0 = resid, flagged
    return avail, rejected, resid0, flagged0


def fault_draws(seed: int, S: int, K: int, share: float) -> np.ndarray:
    """The faults of ``screening_report``: int64 ``[S]``, the faulty sensor (a column of the readings) of every snapshot, -1 for
    a clean one.  ``round(share * S)`` snapshots, chosen without replacement by ``numpy.random.default_rng(seed)``, get one
    sensor each, drawn uniformly by the same generator."""
    S, K = int(S), int(K)
    if S < 1 or K < 1:
        raise ValueError("fault_draws needs S >= 1 and K >= 1")
    if not 0.0 <= float(share) <= 1.0:
        raise ValueError(f"share must lie in [0, 1]; got {share!r}")
    rng = np.random.default_rng(seed)
    n = min(S, int(round(float(share) * S)))
    rows = np.sort(rng.choice(S, size=n, replace=False))
    col = np.full(S, -1, dtype=np.int64)
    col[rows] = rng.integers(0, K, size=n)
    return col


def screening_rates(rejected, fault_col) -> Dict[str, float]:
    """What a screening did, from ``rejected`` (int ``[S, R]``, -1: nothing) and ``fault_col`` (``[S]``, -1: a clean snapshot):
    ``detection_rate`` (of the faulted snapshots: the faulty sensor is among the rejected), ``misidentification_rate`` (of the
    faulted snapshots: something was rejected, the faulty sensor was not), ``false_rejection_rate_faulted`` (of the faulted
    snapshots: a sensor other than the faulty one was rejected), ``false_rejection_rate_clean`` (of the clean snapshots:
    anything was rejected), with ``num_faulted`` and ``num_clean``.  A rate over no snapshots is NaN."""
    rej = np.asarray(rejected, dtype=np.int64)
    col = np.asarray(fault_col, dtype=np.int64)
    if rej.ndim != 2 or col.shape != (rej.shape[0],):
        raise ValueError("rejected must be [S, R] and fault_col [S]")
    faulted, clean = col >= 0, col < 0
    hit = (rej == col[:, None]).any(axis=1) & faulted
    other = ((rej >= 0) & (rej != col[:, None])).any(axis=1)
    some = (rej >= 0).any(axis=1)

    def rate(what, pool):
        return float(what[pool].mean()) if pool.any() else float("nan")

    return {"detection_rate": rate(hit, faulted), "misidentification_rate": rate(some & ~hit, faulted),
            "false_rejection_rate_faulted": rate(other, faulted), "false_rejection_rate_clean": rate(some, clean),
            "num_faulted": int(faulted.sum()), "num_clean": int(clean.sum())}
