"""Pressure estimation with a fixed sensor set: the task ``GATResMeanConv`` is trained for -- the readings of the sensors in, the
pressure at every junction out -- as a device pass, for deployment and for back-testing a sensor layout over a snapshot store.

The reference has no such entry point: a caller writes ``test_one_epoch``'s loop body by hand (evaluation.py:298-330: ``x1`` built
with an index assignment, ``model(x1, edge_index)``, a boolean gather, ``descale`` with torch ops, batch by batch).  Here a pass is
three launches per batch on the current stream -- ``gatres_stage_observed`` (zeros and mask = 1 everywhere but at the sensors),
``gatres_model_forward`` in inference form with that mask, ``gatres_estimate_write`` (descaled into the pass's result matrix) --
with the plans and the forward's call state of ``evaluation.evaluate_store``.  Nothing is read back and nothing synchronises: the
result is a device tensor, ordered on the stream.  ``error_map`` is the back-test report: one ``gatres_node_error_moments`` launch
and one read-back.

Every pass below is ``PressureEstimator._pair_pass`` over S x W (snapshot, something) pairs, snapshot-major -- W = 1, the M
members, the L layouts, the T targets, the K left-out sensors -- cut into batches of ``batch_size`` once, from pair 0, in chunks of
whole snapshots and whole batches (``pass_schedule``; a pass that keeps every pair's result is one chunk).  What a pass
contributes is its batch closure -- the launches of one batch -- and, where it chunks, its fold.

Telemetry has gaps.  With ``available`` (uint8 / bool ``[S, K]`` on the device) or ``nan_is_missing`` the staging launch is
``gatres_stage_observed_available``: a sensor without a reading in a snapshot is one more hidden node there (``x = 0``,
``mask = 1``), which is what the model's training masks taught it.  Still three launches per batch, still nothing read back: no
host scan for NaN.  ``error_map(available=...)`` reports over the hidden entries, ``sensor_failure_report`` is the leave-one-out
back-test of a sensor layout (what does the loss of sensor k cost?) as K + 1 passes of one estimator.

Readings carry error.  ``noise_std`` on the two passes stages one noisy realisation (``gatres_stage_observed_noisy``: the noise
is drawn in the staging launch from ``(seed, member, snapshot, sensor)``, ``reading_noise`` restates it on the host);
``estimate_ensemble`` / ``estimate_store_ensemble`` run M members per snapshot as one long pass over the S * M (snapshot, member)
pairs and reduce them on the device (``gatres_ensemble_reduce``) to the mean and the standard deviation per junction, so the M
result matrices never exist; ``noise_report`` adds the back-test error of the mean and the per-node spread
(``gatres_node_spread_moments``): which junctions are sensitive to sensor error.

Where to put the sensors.  ``layout_errors`` scores L sensor layouts -- subsets of the estimator's ``observed_idx``, the candidate
sensors -- over a store as one long pass over the S * L (snapshot, layout) pairs, again three launches per batch:
``gatres_stage_observed_layouts`` (a sensor the pair's layout leaves out is one more hidden node), the forward, and
``gatres_layout_pair_errors``, which reduces the batch's error against the store's truth to one small record per pair while the
predictions are still in the batch buffers; ``gatres_layout_error_reduce`` folds the records per layout.  No estimate matrix, no
per-node table, no read-back: the result is a device table ``[L, LAYOUT_ERROR_RECORD]`` (``layout_scores_from_table``).
``place_sensors`` is greedy forward selection on top of it (``greedy_selection`` holds the rule): one ``layout_errors`` call and
one read-back per round.

How far off may an estimate be.  ``calibrate_bounds`` is split-conformal calibration over a held-out store: per junction ONE order
statistic of ``|estimate - truth|`` per level, from one ``gatres_node_error_quantiles`` launch (an exact radix select per column
of the error matrix, which is never formed or sorted); the ``ErrorBounds`` stay on the device.  If a new snapshot is exchangeable
with the calibration ones, ``p_v +- b_v`` holds with probability >= level, per junction.  ``coverage_report`` counts, on another
store, how often it did (``gatres_node_bound_coverage``, one read-back); ``estimate_with_bounds`` and ``reading_residuals`` use the
bounds.  ``conformal_rank`` / ``node_error_bounds`` / ``coverage_from_table`` restate all of it in numpy, without a device.

Which sensor does an estimate rest on.  ``sensitivity`` / ``sensitivity_store`` give the Jacobian ``J[s, j, k] = d estimate_j /
d reading_k`` in reverse mode: one graph of a batch carries ONE target junction, so the S * T (snapshot, target) pairs are one
long pass with four launches per batch -- ``gatres_stage_observed_targets`` (the staging launch, which also writes the seeds
``g_out = e_j``), ``gatres_model_forward`` keeping the activations, ``gatres_model_backward`` with ``g_x``, and
``gatres_sensitivity_gather`` (the sensors' entries of ``g_x``, in physical units per physical unit, 0 where a reading is
missing).  ``sensitivity_map`` folds the rows per (junction, sensor) over a store without ever forming ``[S, T, K]``
(``gatres_sensitivity_fold``), ``influence_report`` reads that table back once, ``linear_spread`` is the first-order, noise-free
counterpart of ``estimate_ensemble``'s standard deviation (``gatres_sensitivity_spread``).  sensitivity.py restates the launches.

A reading that is present and wrong.  ``loo_residuals`` / ``loo_residuals_store`` give every reading's LEAVE-ONE-OUT residual,
the reading against the model's prediction at its node with that one sensor hidden: "every sensor but k" is a layout, so the
S * K (snapshot, left-out sensor) pairs are one long pass with three launches per batch -- ``gatres_stage_observed_layouts``
with the K x K layouts "all ones, zero diagonal", the forward and ``gatres_loo_residuals`` -- and no ``[S, N]`` matrix.
``calibrate_screening`` turns the residuals of a held-out store into per-sensor split-conformal bounds (``ScreeningBounds``; one
``gatres_node_error_quantiles`` launch on the ``[S, K]`` matrices), ``screen`` rejects, per snapshot and round, the available
sensor that exceeds its bound by the largest factor (``gatres_screen_reject``), ``estimate_screened`` estimates without the
rejected readings, ``screening_report`` back-tests all of it with planted faults.  screening.py restates the launches.

A sensor that drifts.  A reading that is off by a fraction of its bound for a long time passes every per-snapshot screening.
``monitor`` / ``monitor_store`` read the S snapshots as a time series: per round the leave-one-out pass, ``gatres_cusum_scan`` (a
two-sided CUSUM per sensor along time as one parallel scan in int64 fixed point, against the ``MonitorBaseline`` of
``calibrate_monitor``) and ``gatres_monitor_latch`` (per series the sensor that alarmed first leaves the availability from its
estimated onset on); ``estimate_monitored`` estimates without it, ``monitoring_report`` back-tests with planted ramps.  The state
is carried, so readings may arrive in chunks.  monitoring.py restates the launches.
"""
from __future__ import annotations

import ctypes
import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native
from .evaluation import _enqueue_forward, _eval_plan
from .sensitivity import (SENSITIVITY_RECORD, influence_from_table, linear_spread_ref, sensitivity_fold_ref,  # noqa: F401
                          sensitivity_rows_from_gx, sensitivity_seeds)
from .screening import (fault_draws, loo_layouts, loo_residuals_from_estimates, screen_ref, screen_reject_ref,  # noqa: F401
                        screening_rates)
from .monitoring import (SINCE as MONITOR_SINCE, cusum_compose, cusum_fixed, cusum_scan_ref, drift_draws,  # noqa: F401
                         drift_offsets, monitor_baseline_from_moments, monitor_latch_ref, monitor_ref, monitoring_rates)
from .snapshot_store import SnapshotStore

NODE_ERROR_RECORD = _native.NODE_ERROR_RECORD
NODE_ERROR_AVAIL_RECORD = _native.NODE_ERROR_AVAIL_RECORD
NODE_SPREAD_RECORD = _native.NODE_SPREAD_RECORD
LAYOUT_PAIR_RECORD = _native.LAYOUT_PAIR_RECORD
LAYOUT_ERROR_RECORD = _native.LAYOUT_ERROR_RECORD
NODE_QUANTILE_MAX_LEVELS = _native.NODE_QUANTILE_MAX_LEVELS
NODE_COVERAGE_RECORD = _native.NODE_COVERAGE_RECORD
PLACEMENT_CRITERIA = ("mae", "rmse", "max_abs")   # place_sensors(criterion=...): entries of layout_scores_from_table


def observed_from_names(node_names: Sequence[str], sensor_names: Sequence[str]) -> List[int]:
    """Node indices of the sensors, in the order of ``sensor_names``; ``node_names``: the store's node order (``kept`` of
    ``wdn_io.load_wdn``).  An unknown name, or one that occurs twice, is a ``ValueError``."""
    index: Dict[str, int] = {}
    for i, n in enumerate(node_names):
        if n in index:
            raise ValueError(f"node name {n!r} occurs twice in node_names")
        index[n] = i
    out, seen = [], set()
    for s in sensor_names:
        if s not in index:
            raise ValueError(f"sensor {s!r} is not a node of the network")
        if s in seen:
            raise ValueError(f"sensor {s!r} is listed twice")
        seen.add(s)
        out.append(index[s])
    return out


def error_map_from_moments(table, available: bool = False, observed_idx=None) -> Dict[str, np.ndarray]:
    """The per-node report from a ``gatres_node_error_moments`` table ``[N, NODE_ERROR_RECORD]`` (include/gatres.h), in fp64:
    ``mae``, ``rmse``, ``bias``, ``max_abs``, ``rel_error`` (NaN where no \\|t\\| > 0.01), ``observed`` (bool) per node, and
    ``hidden_mae`` / ``hidden_rmse`` pooled over the unobserved nodes (NaN when every node is observed).

    ``available=True``: ``table`` is a ``gatres_node_error_moments_available`` table ``[N, NODE_ERROR_AVAIL_RECORD]`` and
    ``observed_idx`` the sensors' nodes (the table cannot tell a sensor that never delivered from a node without a sensor).
    The per-node values are then over the node's HIDDEN entries (NaN where it was never hidden), with ``hidden_count`` and
    ``observed`` (the node is in ``observed_idx``) beside them, and the pooled values are ``hidden_mae`` / ``hidden_rmse`` over
    all hidden entries, ``nonsensor_mae`` / ``nonsensor_rmse`` over the nodes outside ``observed_idx`` (today's ``hidden_*`` when
    every reading is available) and ``missing_sensor_mae`` / ``missing_sensor_rmse`` over the hidden entries at sensor nodes
    (NaN when there are none)."""
    if available:
        return _error_map_from_available_moments(table, observed_idx)
    T = np.asarray(table, dtype=np.float64).reshape(-1, NODE_ERROR_RECORD)
    S = T[:, 0]
    observed = T[:, 7] != 0.0
    hidden = ~observed
    with np.errstate(invalid="ignore", divide="ignore"):
        out = {"mae": T[:, 2] / S, "rmse": np.sqrt(T[:, 3] / S), "bias": T[:, 1] / S, "max_abs": T[:, 4].copy(),
               "rel_error": np.where(T[:, 5] > 0, T[:, 6] / T[:, 5], np.nan), "observed": observed,
               "hidden_mae": np.float64(T[hidden, 2].sum() / S[hidden].sum()) if hidden.any() else np.float64("nan"),
               "hidden_rmse": np.float64(np.sqrt(T[hidden, 3].sum() / S[hidden].sum())) if hidden.any() else np.float64("nan")}
    return out


def _error_map_from_available_moments(table, observed_idx) -> Dict[str, np.ndarray]:
    if observed_idx is None:
        raise ValueError("available=True needs observed_idx: the sensors' node indices")
    T = np.asarray(table, dtype=np.float64).reshape(-1, NODE_ERROR_AVAIL_RECORD)
    H = T[:, 0]                                     # hidden entries per node
    sensor = np.zeros(T.shape[0], dtype=np.bool_)
    sensor[np.asarray(list(observed_idx), dtype=np.int64)] = True

    def pooled(rows):
        n = H[rows].sum()
        if not n > 0:
            return np.float64("nan"), np.float64("nan")
        return np.float64(T[rows, 2].sum() / n), np.float64(np.sqrt(T[rows, 3].sum() / n))

    with np.errstate(invalid="ignore", divide="ignore"):
        out = {"mae": T[:, 2] / H, "rmse": np.sqrt(T[:, 3] / H), "bias": T[:, 1] / H,
               "max_abs": np.where(H > 0, T[:, 4], np.nan),
               "rel_error": np.where(T[:, 5] > 0, T[:, 6] / np.where(T[:, 5] > 0, T[:, 5], 1.0), np.nan),
               "hidden_count": H.copy(), "observed": sensor}
    everything = np.ones(T.shape[0], dtype=np.bool_)
    out["hidden_mae"], out["hidden_rmse"] = pooled(everything)
    out["nonsensor_mae"], out["nonsensor_rmse"] = pooled(~sensor)
    out["missing_sensor_mae"], out["missing_sensor_rmse"] = pooled(sensor)
    return out


def _mix64(z: np.ndarray) -> np.ndarray:
    """``mix64`` of csrc/gatres_common.h on uint64 arrays (numpy's unsigned array arithmetic is modulo 2^64)."""
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _check_seed(seed) -> int:
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 1 << 64:
        raise ValueError(f"the noise seed must be an integer in [0, 2**64); got {seed!r}")
    return int(seed)


def _noise_bits(seed, members: int, rows: int, num_sensors: int, member0: int = 0) -> np.ndarray:
    """``h`` of the generator (include/gatres.h, gatres_stage_observed_noisy) as uint64 ``[rows, members, K]``."""
    seed = _check_seed(seed)
    members, rows, K, member0 = int(members), int(rows), int(num_sensors), int(member0)
    if members < 1 or rows < 1 or K < 1 or member0 < 0:
        raise ValueError("reading_noise needs members, rows, num_sensors >= 1 and member0 >= 0")
    member = np.arange(member0, member0 + members, dtype=np.uint64)
    stream = _mix64(np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15) * (member + np.uint64(1)))
    cell = np.arange(1, rows * K + 1, dtype=np.uint64).reshape(rows, 1, K)          # row * K + k + 1
    return _mix64(stream.reshape(1, members, 1) + np.uint64(0xBF58476D1CE4E5B9) * cell)


def reading_noise(seed, members: int, rows: int, num_sensors: int, member0: int = 0) -> np.ndarray:
    """The standard normal draws of ``gatres_stage_observed_noisy``, restated on the host: float64 ``[rows, members, K]``,
    entry ``[r, m, k]`` the ``z`` of (``seed``, member ``member0 + m``, source row ``r``, sensor ``k``).  The integers are formed
    in numpy ``uint64`` exactly as on the device; Box-Muller is evaluated in fp64 (the device evaluates it in fp32: the two
    agree to a few 1e-6)."""
    h = _noise_bits(seed, members, rows, num_sensors, member0)
    u1 = ((h >> np.uint64(40)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
    u2 = ((h >> np.uint64(8)) & np.uint64(0xFFFFFF)).astype(np.float64) * 2.0 ** -24
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def noise_std_vector(noise_std, num_sensors: int) -> np.ndarray:
    """``noise_std`` -- one non-negative finite number or ``num_sensors`` of them, physical units -- as float64 ``[K]``."""
    K = int(num_sensors)
    try:
        v = np.asarray(noise_std, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"noise_std must be a non-negative number or a sequence of {K} of them") from None
    if v.ndim == 0:
        v = np.full(K, float(v))
    if v.shape != (K,):
        raise ValueError(f"noise_std must be a non-negative number or a sequence of {K} of them, one per sensor; got shape "
                         f"{tuple(v.shape)}")
    if not np.isfinite(v).all() or (v < 0).any():
        raise ValueError("noise_std must be finite and non-negative")
    return v


def noise_sigma(noise_std, num_sensors: int, norm_type: str, std: Optional[float], eps: float, full_rows: bool) -> np.ndarray:
    """``noise_std`` (physical units) as the float32 ``sigma[K]`` of the noisy staging launches (gatres_stage_observed_noisy,
    gatres_stage_rows_mask_sensors_noisy), in the units of the launch's source: divided by ``std + eps`` for the full rows of a
    z-normalised store, unchanged for raw readings and for an ``unused`` store.  The one statement of that conversion:
    ``PressureEstimator`` and ``SensorLayout`` both come here."""
    v = noise_std_vector(noise_std, num_sensors)
    if full_rows and norm_type == "znorm":
        v = v / (float(std) + float(eps))
    return v.astype(np.float32)


def ensemble_chunk(num_snapshots: int, members: int, batch_size: int, row_bytes: int, max_scratch_bytes: int) -> int:
    """Snapshots per chunk of the ensemble's scratch matrix (``row_bytes`` per pair).  The pass over the S * M pairs is cut into
    batches of ``batch_size`` once, from pair 0; a chunk must hold whole snapshots AND whole batches, so it is a multiple of the
    unit ``lcm(batch_size, M) / M`` snapshots: as many units as ``max_scratch_bytes`` holds, at least one, and the whole pass
    when that is less.  The batch partition therefore does not depend on the budget."""
    S, M, bs = int(num_snapshots), int(members), int(batch_size)
    unit = bs // math.gcd(bs, M)                                    # lcm(bs, M) / M
    units = max(1, int(max_scratch_bytes) // (unit * M * int(row_bytes)))
    return min(S, units * unit)


def pass_schedule(num_snapshots: int, width: int, batch_size: int, chunk: Optional[int] = None):
    """The cut of a pass over the S * W pairs (snapshot-major, W = ``width`` pairs per snapshot): one ``(s0, c, batches)`` per
    chunk of ``chunk`` snapshots (``ensemble_chunk``; ``None``: one chunk of all S) -- the chunk holds the snapshots ``[s0, s0 +
    c)`` -- with ``batches`` its ``(first_pair, g, off)``: ``g`` pairs from pair ``first_pair = s0 * W + off`` on, ``off`` the
    batch's first pair inside the chunk.  A chunk of ``ensemble_chunk`` starts a batch, so the batches are those of the one
    chunk, whatever the chunk.  ``batches`` is an iterator: a long pass enqueues its first batch before the last is cut."""
    S, W, bs = int(num_snapshots), int(width), int(batch_size)
    C = S if chunk is None else int(chunk)

    def batches(first, pairs):
        for off in range(0, pairs, bs):
            yield first + off, min(bs, pairs - off), off

    for s0 in range(0, S, C):
        c = min(C, S - s0)
        yield s0, c, batches(s0 * W, c * W)


def pass_batch_sizes(num_snapshots: int, width: int, batch_size: int) -> set:
    """The batch sizes that occur in ``pass_schedule``: the first batch's and the last one's."""
    P, bs = int(num_snapshots) * int(width), int(batch_size)
    return {min(bs, P), P - (P - 1) // bs * bs}


def _level_index(levels: Tuple[float, ...], level) -> int:
    """The row of a bounds matrix for ``level``: an exact match of one of ``levels`` (``None``: the only one)."""
    if level is None:
        if len(levels) != 1:
            raise ValueError(f"level=None needs bounds with one level; these hold {levels}")
        return 0
    if float(level) not in levels:
        raise ValueError(f"level {level!r} is not one of the calibrated levels {levels}")
    return levels.index(float(level))


def noise_report_from_moments(table, observed_idx) -> Dict[str, np.ndarray]:
    """The per-node spread report from a ``gatres_node_spread_moments`` table ``[N, NODE_SPREAD_RECORD]`` (include/gatres.h), in
    fp64: ``spread`` = sqrt(sum std^2 / S), the root-mean-square standard deviation of the node's estimate over the snapshots,
    ``max_std``, ``mean_std``, ``nonsensor_spread`` pooled over the nodes outside ``observed_idx`` (NaN when every node is a
    sensor) and ``most_sensitive``, the node indices by descending ``spread`` (ties in node order)."""
    T = np.asarray(table, dtype=np.float64).reshape(-1, NODE_SPREAD_RECORD)
    S = T[:, 0]
    sensor = np.zeros(T.shape[0], dtype=np.bool_)
    sensor[np.asarray(list(observed_idx), dtype=np.int64)] = True
    spread = np.sqrt(T[:, 1] / S)
    pooled = np.float64(np.sqrt(T[~sensor, 1].sum() / S[~sensor].sum())) if (~sensor).any() else np.float64("nan")
    return {"spread": spread, "max_std": T[:, 2].copy(), "mean_std": T[:, 3] / S, "nonsensor_spread": pooled,
            "most_sensitive": np.argsort(-spread, kind="stable")}


def layout_scores_from_table(table) -> Dict[str, np.ndarray]:
    """The per-layout scores from a ``gatres_layout_error_reduce`` table ``[L, LAYOUT_ERROR_RECORD]`` (include/gatres.h), in fp64:
    ``count`` (the entries scored: hidden nodes times snapshots), ``mae``, ``rmse`` and ``max_abs`` over them.  A layout with
    ``count == 0`` (every scored node carries a sensor) gives NaN."""
    T = np.asarray(table, dtype=np.float64).reshape(-1, LAYOUT_ERROR_RECORD)
    n = T[:, 0]
    some = n > 0
    d = np.where(some, n, 1.0)
    return {"count": n.copy(), "mae": np.where(some, T[:, 1] / d, np.nan), "rmse": np.where(some, np.sqrt(T[:, 2] / d), np.nan),
            "max_abs": np.where(some, T[:, 3], np.nan)}


def conformal_rank(n, level):
    """The split-conformal rank of ``gatres_node_error_quantiles`` (include/gatres.h), 1-based, in numpy fp64:
    ``ceil(float64(n + 1) * float64(level))`` -- one product, one ceil.  ``n`` may be an array.  A rank above ``n`` means too few
    samples for the level: the bound is +inf."""
    return np.ceil((np.asarray(n, dtype=np.int64) + 1).astype(np.float64) * np.float64(level))


def _check_levels(levels) -> Tuple[float, ...]:
    try:
        lv = tuple(float(q) for q in levels)
    except TypeError:
        raise ValueError(f"levels must be a sequence of 1 to {NODE_QUANTILE_MAX_LEVELS} floats in (0, 1)") from None
    if not 1 <= len(lv) <= NODE_QUANTILE_MAX_LEVELS:
        raise ValueError(f"levels must hold 1 to {NODE_QUANTILE_MAX_LEVELS} values; got {len(lv)}")
    if any(not 0.0 < q < 1.0 for q in lv):
        raise ValueError(f"levels must lie in the open interval (0, 1); got {lv}")
    if any(b <= a for a, b in zip(lv, lv[1:])):
        raise ValueError(f"levels must be strictly increasing; got {lv}")
    return lv


def node_error_bounds(est, truth_descaled, levels, hidden=None) -> Tuple[np.ndarray, np.ndarray]:
    """The statement ``gatres_node_error_quantiles`` is held to, in numpy (no device): ``e = float32(est) - float32(truth_descaled)``
    rounded to fp32, the ``uint32`` patterns of ``|e|`` sorted per column -- over the entries where ``hidden`` (bool ``[S, N]``) is
    true, when given -- and per level the element of rank ``conformal_rank(n_v, level)``, +inf where the rank exceeds ``n_v``.
    As unsigned integers the patterns are in IEEE order, with a NaN above +inf.  Returns ``(bounds[Q, N] float32, counts[N]
    float64)``.  ``levels``: any floats in (0, 1)."""
    e = np.asarray(est, dtype=np.float32) - np.asarray(truth_descaled, dtype=np.float32)
    if e.ndim != 2:
        raise ValueError("est and truth_descaled must be [S, N]")
    lv = [float(q) for q in levels]
    if not lv or any(not 0.0 < q < 1.0 for q in lv):
        raise ValueError("levels must be floats in the open interval (0, 1), at least one")
    S, N = e.shape
    keys = np.ascontiguousarray(np.abs(e)).view(np.uint32)
    counted = np.ones((S, N), dtype=np.bool_) if hidden is None else np.asarray(hidden, dtype=np.bool_)
    if counted.shape != (S, N):
        raise ValueError(f"hidden must be bool [{S}, {N}]")
    bounds = np.full((len(lv), N), np.inf, dtype=np.float32)
    bits = bounds.view(np.uint32)
    counts = counted.sum(axis=0).astype(np.int64)
    for v in range(N):
        col = np.sort(keys[counted[:, v], v])
        for q, level in enumerate(lv):
            r = int(conformal_rank(counts[v], level))
            if r <= counts[v]:
                bits[q, v] = col[r - 1]
    return bounds, counts.astype(np.float64)


def coverage_from_table(table, bounds, levels, observed_idx) -> Dict[str, object]:
    """The coverage report from a ``gatres_node_bound_coverage`` table ``[N, NODE_COVERAGE_RECORD]`` (include/gatres.h) and the
    ``bounds[Q, N]`` it was counted against, in fp64: ``levels``, ``coverage[Q, N]`` = hits / n_v (NaN where n_v == 0), and over
    the nodes outside ``observed_idx`` ``nonsensor_coverage[Q]`` (sum of hits / sum of counts; NaN without any), ``min_coverage[Q]``
    with ``worst_node[Q]`` (the first node that attains it; NaN and -1 when no such node has an entry), ``mean_width[Q]`` = the
    mean of ``2 * bounds`` over those of them with a finite bound (NaN without any) and ``unbounded[Q]``, the number of them with
    an infinite bound."""
    T = np.asarray(table, dtype=np.float64).reshape(-1, NODE_COVERAGE_RECORD)
    lv = [float(q) for q in levels]
    Q, N = len(lv), T.shape[0]
    B = np.asarray(bounds, dtype=np.float64).reshape(Q, N)
    n, hits = T[:, 0], T[:, 1:1 + Q].T
    some = n > 0
    coverage = np.where(some, hits / np.where(some, n, 1.0), np.nan)
    free = np.ones(N, dtype=np.bool_)
    free[np.asarray(list(observed_idx), dtype=np.int64)] = False
    pool = free & some
    out = {"levels": tuple(lv), "coverage": coverage,
           "nonsensor_coverage": np.full(Q, np.nan), "min_coverage": np.full(Q, np.nan),
           "worst_node": np.full(Q, -1, dtype=np.int64), "mean_width": np.full(Q, np.nan),
           "unbounded": np.zeros(Q, dtype=np.int64)}
    nodes = np.nonzero(pool)[0]
    for q in range(Q):
        if nodes.size:
            out["nonsensor_coverage"][q] = hits[q, pool].sum() / n[pool].sum()
            worst = nodes[np.argmin(coverage[q, nodes])]
            out["min_coverage"][q], out["worst_node"][q] = coverage[q, worst], worst
        finite = free & np.isfinite(B[q])
        if finite.any():
            out["mean_width"][q] = (2.0 * B[q, finite]).mean()
        out["unbounded"][q] = int((free & np.isinf(B[q])).sum())
    return out


class ErrorBounds:
    """Calibrated per-node error bounds: ``levels`` (a tuple of floats), ``bounds`` (fp32 ``[Q, N]``: ``|estimate - truth| <=
    bounds[q, v]`` at node ``v`` with probability >= ``levels[q]``; +inf: too few calibration samples), ``counts`` (fp64 ``[N]``:
    the samples behind each node's bounds) and ``observed_idx``, the sensor layout they were calibrated for.  The tensors stay
    where ``calibrate_bounds`` left them, on the device."""

    def __init__(self, levels, bounds: torch.Tensor, counts: torch.Tensor, observed_idx):
        self.levels = tuple(float(q) for q in levels)
        if (not isinstance(bounds, torch.Tensor) or bounds.dtype != torch.float32 or bounds.dim() != 2
                or bounds.shape[0] != len(self.levels)):
            raise ValueError(f"bounds must be an fp32 tensor [{len(self.levels)}, N]")
        if (not isinstance(counts, torch.Tensor) or counts.dtype != torch.float64 or tuple(counts.shape) != (bounds.shape[1],)
                or counts.device != bounds.device):
            raise ValueError(f"counts must be an fp64 tensor [{bounds.shape[1]}] on {bounds.device}")
        self.bounds, self.counts = bounds, counts
        self.observed_idx = [int(i) for i in observed_idx]

    @property
    def nodes_per_graph(self) -> int:
        return int(self.bounds.shape[1])

    @property
    def device(self) -> torch.device:
        return self.bounds.device

    def level_index(self, level=None) -> int:
        """The row of ``bounds`` for ``level``: an exact match of a stored level (``None``: the only one)."""
        return _level_index(self.levels, level)

    def interval(self, estimates: torch.Tensor, level=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """``(estimates - b, estimates + b)`` with ``b = bounds[level_index(level)]`` broadcast over the rows of ``estimates``
        (``[..., N]`` on the bounds' device): two torch element passes, nothing read back."""
        b = self.bounds[self.level_index(level)]
        return estimates - b, estimates + b

    def state_dict(self) -> Dict[str, object]:
        """CPU tensors and plain lists (one read-back of each tensor): what ``wdn_io.save_checkpoint(path, ...,
        error_bounds=eb.state_dict())`` can carry."""
        return {"levels": list(self.levels), "bounds": self.bounds.detach().cpu(), "counts": self.counts.detach().cpu(),
                "observed_idx": list(self.observed_idx)}

    @classmethod
    def from_state_dict(cls, d, device=None) -> "ErrorBounds":
        bounds, counts = torch.as_tensor(d["bounds"], dtype=torch.float32), torch.as_tensor(d["counts"], dtype=torch.float64)
        if device is not None:
            bounds, counts = bounds.to(device), counts.to(device)
        return cls(d["levels"], bounds, counts, d["observed_idx"])


class ScreeningBounds:
    """Calibrated bounds on the leave-one-out residuals of a sensor set: ``levels`` (a tuple of floats), ``bounds`` (fp32
    ``[Q, K]``: ``|reading - leave-one-out prediction| <= bounds[q, k]`` for sensor ``observed_idx[k]`` with probability >=
    ``levels[q]`` while every other reading is present; +inf: too few calibration samples), ``counts`` (fp64 ``[K]``: the samples
    behind each sensor's bounds) and ``observed_idx``.  ``calibrate_screening`` leaves the tensors on the device; arrays are taken
    too (``device``: where to put them).  ``inverse`` is ``float32(1) / bounds`` formed in numpy on the host (so that the
    statement of ``gatres_screen_reject`` holds no device division) the first time it is asked for -- one read-back of ``bounds``,
    once -- and kept."""

    def __init__(self, levels, bounds, counts, observed_idx, device=None):
        self.levels = _check_levels(levels)
        self.observed_idx = [int(i) for i in observed_idx]
        if not isinstance(bounds, torch.Tensor):
            bounds = torch.from_numpy(np.ascontiguousarray(bounds, dtype=np.float32))
        if not isinstance(counts, torch.Tensor):
            counts = torch.from_numpy(np.ascontiguousarray(counts, dtype=np.float64))
        if device is not None:
            bounds, counts = bounds.to(device), counts.to(device)
        Q, K = len(self.levels), len(self.observed_idx)
        if bounds.dtype != torch.float32 or tuple(bounds.shape) != (Q, K) or not bounds.is_contiguous():
            raise ValueError(f"bounds must be fp32 contiguous [{Q}, {K}]: one row per level, one column per sensor")
        if counts.dtype != torch.float64 or tuple(counts.shape) != (K,) or counts.device != bounds.device:
            raise ValueError(f"counts must be fp64 [{K}] on {bounds.device}")
        self.bounds, self.counts = bounds, counts
        self._inverse = None

    @property
    def device(self) -> torch.device:
        return self.bounds.device

    def level_index(self, level=None) -> int:
        """The row of ``bounds`` for ``level``: an exact match of a stored level (``None``: the only one)."""
        return _level_index(self.levels, level)

    @property
    def inverse(self) -> torch.Tensor:
        if self._inverse is None:
            with np.errstate(divide="ignore", invalid="ignore"):
                inv = (np.float32(1.0) / self.bounds.detach().cpu().numpy()).astype(np.float32)
            self._inverse = torch.from_numpy(inv).to(self.device)
        return self._inverse

    def state_dict(self) -> Dict[str, object]:
        """CPU tensors and plain lists (one read-back of each tensor), for ``torch.save``."""
        return {"levels": list(self.levels), "bounds": self.bounds.detach().cpu(), "counts": self.counts.detach().cpu(),
                "observed_idx": list(self.observed_idx)}

    @classmethod
    def from_state_dict(cls, d, device=None) -> "ScreeningBounds":
        return cls(d["levels"], torch.as_tensor(d["bounds"], dtype=torch.float32).contiguous(),
                   torch.as_tensor(d["counts"], dtype=torch.float64), d["observed_idx"], device=device)


class MonitorBaseline:
    """The in-control behaviour of the leave-one-out residuals of a sensor set, for the drift monitor: ``mu`` and ``inv_sigma``
    (fp32 ``[K]`` on the device: what ``gatres_cusum_scan`` reads), ``sigma`` and ``counts`` (fp64 ``[K]`` on the device) and
    ``observed_idx``.  Built from ``mu`` and ``sigma`` as arrays or tensors (read to the host here, once; ``device``: where to
    put the result): ``inv_sigma = float32(1 / sigma)`` is formed on the host in fp64, so that the statement of the scan holds
    no device division.  A zero or NaN ``sigma`` leaves a sensor whose entries are never counted."""

    def __init__(self, mu, sigma, counts, observed_idx, device=None):
        self.observed_idx = [int(i) for i in observed_idx]
        K = len(self.observed_idx)

        def host(v, what):
            a = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
            if a.shape != (K,):
                raise ValueError(f"{what} must hold {K} values, one per sensor")
            return np.ascontiguousarray(a, dtype=np.float64)

        if device is None:
            device = mu.device if isinstance(mu, torch.Tensor) else "cpu"
        mu, sigma, counts = host(mu, "mu"), host(sigma, "sigma"), host(counts, "counts")
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = (1.0 / sigma).astype(np.float32)
        self.mu = torch.from_numpy(mu.astype(np.float32)).to(device)
        self.inv_sigma = torch.from_numpy(inv).to(device)
        self.sigma = torch.from_numpy(sigma).to(device)
        self.counts = torch.from_numpy(counts).to(device)

    @property
    def device(self) -> torch.device:
        return self.mu.device

    def state_dict(self) -> Dict[str, object]:
        """CPU tensors and plain lists (one read-back of each tensor), for ``torch.save``."""
        return {"mu": self.mu.detach().cpu(), "sigma": self.sigma.detach().cpu(), "counts": self.counts.detach().cpu(),
                "observed_idx": list(self.observed_idx)}

    @classmethod
    def from_state_dict(cls, d, device=None) -> "MonitorBaseline":
        return cls(torch.as_tensor(d["mu"]), torch.as_tensor(d["sigma"]), torch.as_tensor(d["counts"]), d["observed_idx"],
                   device="cpu" if device is None else device)


class MonitorResult:
    """What ``PressureEstimator.monitor`` leaves, all on the device: ``available_out`` (uint8 ``[S, K]``), ``latched`` (int32
    ``[E, R]``: the sensor round ``r`` latched in series ``e``, -1: none), ``latched_rec`` (int64 ``[E, R, 6]``: its record
    ``[alarm, side, onset, n, sum q, statistic]``), ``records0`` (int64 ``[E, K, 6]``: every sensor's record of round 0),
    ``state`` (int64 ``[E, K, 4]``: the last round's state after the last row, what the next chunk's call takes) and
    ``stat_pos`` / ``stat_neg`` (fp32 ``[S, K]``, round 0's paths in sigma; ``None`` unless asked for).  The tensors are a
    scratch kept on the estimator: the next ``monitor`` / ``estimate_monitored`` overwrites them."""

    def __init__(self, available_out, latched, latched_rec, records0, state, stat_pos=None, stat_neg=None):
        self.available_out, self.latched, self.latched_rec, self.records0 = available_out, latched, latched_rec, records0
        self.state, self.stat_pos, self.stat_neg = state, stat_pos, stat_neg

    def shift(self, baseline: MonitorBaseline) -> torch.Tensor:
        """The estimated size of each latched sensor's shift, fp64 ``[E, R]`` in physical units: the mean standardised
        residual over the excursion that alarmed, ``sigma[k*] * sum q / (65536 n)``; NaN where nothing was latched.  Device
        torch operations, nothing read back."""
        k = self.latched.clamp(min=0).long()
        mean_z = self.latched_rec[..., 4].double() / (65536.0 * self.latched_rec[..., 3].double())
        nan = torch.full_like(mean_z, float("nan"))
        return torch.where(self.latched >= 0, baseline.sigma[k] * mean_z, nan)


def greedy_selection(score_round, candidates: Sequence[int], num: int) -> Tuple[List[int], List[float]]:
    """Greedy forward selection of ``num`` of ``candidates``.  Each round calls ``score_round(chosen, remaining)`` -- the
    candidates chosen so far in order of choice, and the others in ``candidates`` order -- which returns one score per
    remaining candidate: the score of ``chosen`` plus that candidate.  The smallest score wins; a NaN counts as worse than any
    number; ties (and a round of NaNs) go to the earliest candidate in ``candidates`` order.  Returns the chosen candidates in
    order of choice and the winning score of each round."""
    remaining = [int(c) for c in candidates]
    if len(set(remaining)) != len(remaining):
        raise ValueError("candidates holds duplicates")
    if isinstance(num, bool) or not isinstance(num, (int, np.integer)) or not 0 <= int(num) <= len(remaining):
        raise ValueError(f"num must be an integer in [0, {len(remaining)}]; got {num!r}")
    chosen: List[int] = []
    scores: List[float] = []
    for _ in range(int(num)):
        sc = np.asarray(score_round(list(chosen), list(remaining)), dtype=np.float64).reshape(-1)
        if sc.shape[0] != len(remaining):
            raise ValueError(f"score_round returned {sc.shape[0]} scores for {len(remaining)} candidates")
        best = 0
        for i in range(1, len(remaining)):
            if not np.isnan(sc[i]) and (np.isnan(sc[best]) or sc[i] < sc[best]):
                best = i
        chosen.append(remaining.pop(best))
        scores.append(float(sc[best]))
    return chosen, scores


def _check_placement(nodes_per_graph: int, num_sensors, candidates, fixed, criterion) -> Tuple[List[int], List[int]]:
    """The refusals of ``place_sensors`` (no device needed): returns (fixed, candidates) as lists."""
    N = int(nodes_per_graph)
    if criterion not in PLACEMENT_CRITERIA:
        raise ValueError(f"criterion={criterion!r}: one of {', '.join(repr(c) for c in PLACEMENT_CRITERIA)}")
    fix = [int(i) for i in fixed]
    cand = [v for v in range(N) if v not in set(fix)] if candidates is None else [int(i) for i in candidates]
    both = sorted(set(fix) & set(cand))
    if both:
        raise ValueError(f"fixed and candidates overlap at node {both[0]}")
    if isinstance(num_sensors, bool) or not isinstance(num_sensors, (int, np.integer)) or not 1 <= int(num_sensors) <= len(cand):
        raise ValueError(f"num_sensors must be an integer in [1, {len(cand)}] (the number of candidates); got {num_sensors!r}")
    _check_observed(fix + cand, N)                     # (range and duplicates, in observed_idx's wording)
    return fix, cand


_RECIPROCAL: Dict[str, bool] = {}


def _divides_by_reciprocal(device: torch.device) -> bool:
    """How this torch build forms ``fp32 tensor / Python float`` on ``device``: by the fp32 reciprocal of the scalar (True) or
    by a true division (False, what the CPU does).  ``SnapshotStore`` normalises with that expression; the readings layout of
    ``gatres_stage_observed`` must round the same way.  Asked once per device type, on 256 values."""
    got = _RECIPROCAL.get(device.type)
    if got is None:
        x = torch.arange(1, 257, dtype=torch.float32)
        on_dev = (x.to(device) / 3.0).cpu()
        recip, true_div = x * float(np.float32(1.0) / np.float32(3.0)), x / 3.0
        if torch.equal(recip, true_div) or not (torch.equal(on_dev, recip) or torch.equal(on_dev, true_div)):
            raise RuntimeError("cannot tell how torch divides an fp32 tensor by a scalar on " + str(device))
        got = _RECIPROCAL[device.type] = torch.equal(on_dev, recip)
    return got


def _check_observed(observed_idx, nodes_per_graph: int) -> List[int]:
    obs = [int(i) for i in observed_idx]
    if not obs:
        raise ValueError("observed_idx is empty: the estimator needs at least one sensor")
    bad = [i for i in obs if i < 0 or i >= nodes_per_graph]
    if bad:
        raise ValueError(f"observed_idx must lie in [0, {nodes_per_graph}); got {bad[0]}")
    if len(set(obs)) != len(obs):
        raise ValueError("observed_idx holds duplicates")
    return obs


def _refuse_multi(store) -> None:
    from .multi_snapshot_store import MultiSnapshotStore
    if isinstance(store, MultiSnapshotStore):
        raise ValueError("a MultiSnapshotStore is out of scope for PressureEstimator (sensor sets belong to one network): "
                         "build one estimator per network's SnapshotStore")


class PressureEstimator:
    """``model`` with a fixed sensor layout ``observed_idx`` (node indices inside a graph, in the column order of the readings)
    on the topology ``edge_index`` (int64 ``[2, E]`` of ONE graph of ``nodes_per_graph`` nodes).  ``norm_type="znorm"``:
    readings are normalised with ``mean`` / ``std`` / ``eps`` exactly as ``SnapshotStore`` normalises, estimates are descaled as
    ``SnapshotStore.descale`` does; ``"unused"``: neither.  ``keep_observed``: the result carries the sensors' own values (after
    the normalise / descale round trip) at the observed nodes instead of the model's prediction there.  The observed indices
    are uploaded once, here."""

    def __init__(self, model, edge_index, nodes_per_graph: int, observed_idx, *, mean: Optional[float] = None,
                 std: Optional[float] = None, norm_type: str = "znorm", eps: float = 1e-8, batch_size: int = 32,
                 keep_observed: bool = True, _topology=None):
        if norm_type == "minmax":
            raise ValueError("norm_type='minmax': the snapshot stores are z-normalised ('znorm') or not normalised ('unused')")
        if norm_type not in ("znorm", "unused"):
            raise ValueError(f"norm_type={norm_type!r}: 'znorm' or 'unused'")
        if norm_type == "znorm" and (mean is None or std is None):
            raise ValueError("norm_type='znorm' needs mean and std (the training store's)")
        if int(nodes_per_graph) <= 0:
            raise ValueError("nodes_per_graph must be positive")
        if int(batch_size) <= 0:
            raise ValueError("batch_size must be positive")
        self.nodes_per_graph = int(nodes_per_graph)
        self.observed_idx = _check_observed(observed_idx, self.nodes_per_graph)
        self.norm_type, self.eps = norm_type, float(eps)
        self.mean = float(mean) if norm_type == "znorm" else None
        self.std = float(std) if norm_type == "znorm" else None
        self.batch_size, self.keep_observed = int(batch_size), bool(keep_observed)
        self.model = model
        dev = model.flat_parameters.device
        if dev.type != "cuda":
            raise ValueError(f"the model must live on a ROCm device (got {dev}); this engine has no CPU path")
        self.device = dev
        # (the topology in the form the evaluation plans take it: nodes_per_graph, device, edge_index(batch size))
        self._topo = _topology if _topology is not None else SnapshotStore(
            torch.zeros((1, self.nodes_per_graph)), edge_index, device=dev, normalize=False)
        if self._topo.device != dev:
            raise ValueError(f"model is on {dev}, the store on {self._topo.device}")
        self.scale, self.offset = (self.std, self.mean) if norm_type == "znorm" else (1.0, 0.0)     # descale: no eps, as the stores
        self._factor = self.std + self.eps if norm_type == "znorm" else 1.0           # normalise: with eps, as the stores
        self._normalise = _native.NORMALISE_NONE
        if norm_type == "znorm":
            self._normalise = _native.NORMALISE_RECIPROCAL if _divides_by_reciprocal(dev) else _native.NORMALISE_DIVIDE
        self._observed = torch.tensor(self.observed_idx, dtype=torch.int32).to(dev)
        self._sigma_cache = {}                      # layout -> (bytes, device sigma[K]) of the last noise_std: uploaded when it changes
        self._score_cache = None                    # (nodes, device score[N]) of the last score_nodes: uploaded when it changes
        self._targets_cache = None                  # (targets, device int32[T]) of the last targets: uploaded when they change
        self._sens_buffers = {}                     # plan key -> (saved, g_out, g_x, grads) of the sensitivity pass
        self._sens_scratch = {}                     # name -> the pass's scratch matrix, kept while its shape stays
        self._loo_layouts = None                    # device uint8 [K, K] of the leave-one-out pass: all ones, zero diagonal

    @classmethod
    def for_store(cls, model, store, observed_idx, **kw) -> "PressureEstimator":
        """Topology and statistics from a ``SnapshotStore`` (its plans are then shared with ``evaluate_store``)."""
        _refuse_multi(store)
        return cls(model, store.edge_index_single, store.nodes_per_graph, observed_idx, mean=store.mean, std=store.std,
                   norm_type=store.norm_type, _topology=store, **kw)

    @classmethod
    def from_checkpoint(cls, model, path: str, edge_index, nodes_per_graph: int, observed_idx, **kw) -> "PressureEstimator":
        """Weights, ``mean``, ``std`` and ``norm_type`` from a checkpoint of ``GATResTrainer.fit`` or of the reference's train.py
        (``wdn_io.load_checkpoint``); ``model`` is on its device already."""
        from .wdn_io import load_checkpoint
        _, cp = load_checkpoint(path, model, map_location=model.flat_parameters.device)
        stats = {k: cp.get(k) for k in ("mean", "std")}
        stats["norm_type"] = cp.get("norm_type", "znorm")
        return cls(model, edge_index, nodes_per_graph, observed_idx, **{**stats, **kw})

    # ---- the pass -------------------------------------------------------------------------------------------------------------
    def _check_store(self, store) -> None:
        _refuse_multi(store)
        if store.nodes_per_graph != self.nodes_per_graph:
            raise ValueError(f"the store has {store.nodes_per_graph} nodes per graph, the estimator {self.nodes_per_graph}")
        if store.norm_type != self.norm_type:
            raise ValueError(f"the store's norm_type is {store.norm_type!r}, the estimator's {self.norm_type!r}")
        if self.norm_type == "znorm" and (float(store.mean) != self.mean or float(store.std) != self.std):
            raise ValueError(f"the store's mean / std ({store.mean}, {store.std}) differ from the estimator's "
                             f"({self.mean}, {self.std})")
        if store.device != self.device:
            raise ValueError(f"model is on {self.device}, the store on {store.device}")
        if len(store) == 0:
            raise ValueError("empty store")

    def _out(self, out: Optional[torch.Tensor], shape, dtype=torch.float32) -> torch.Tensor:
        """A caller's ``out`` if it is what the pass writes -- contiguous ``shape`` of ``dtype`` on the device --, a new tensor
        for ``None``."""
        shape = tuple(shape)
        if out is None:
            return torch.empty(shape, dtype=dtype, device=self.device)
        if (not isinstance(out, torch.Tensor) or out.dtype != dtype or out.device != self.device or tuple(out.shape) != shape
                or not out.is_contiguous()):
            raise ValueError(f"out must be {'fp64' if dtype == torch.float64 else 'fp32'} contiguous "
                             f"[{', '.join(str(n) for n in shape)}] on {self.device}")
        return out

    def _result(self, S: int, out: Optional[torch.Tensor]) -> torch.Tensor:
        return self._out(out, (S, self.nodes_per_graph))

    def _staging_tail(self, normalise: int) -> tuple:
        """The arguments ``(observed, K, normalise, offset, factor)`` every staging launch ends its source description with."""
        return self._observed.data_ptr(), len(self.observed_idx), normalise, self.offset, self._factor

    def _parameters(self) -> torch.Tensor:
        """The model's parameter vector, for a pass's closure (one look-up per pass: the property walks every parameter)."""
        flat = self.model.flat_parameters
        if flat.device != self.device:
            raise ValueError(f"the model moved to {flat.device}; the estimator was built on {self.device}")
        return flat

    def _pair_pass(self, S: int, width: int, chunk: Optional[int], batch, fold=None) -> None:
        """One pass over the ``S * width`` pairs in the cut of ``pass_schedule``: ``batch(P, first_pair, g, off)`` enqueues the
        launches of one batch on the plan ``P`` of its size, ``fold(s0, c)`` what follows a chunk.  The plans of the two batch
        sizes that occur are fetched up front.  (The closure holds the parameter vector of ``_parameters``, which is where a
        model that moved is refused: the vector is looked up once per pass.)"""
        model = self.model
        model.eval()
        with torch.cuda.device(self.device):
            plans = {g: _eval_plan(model, self._topo, g) for g in sorted(pass_batch_sizes(S, width, self.batch_size))}
            for s0, c, batches in pass_schedule(S, width, self.batch_size, chunk):
                for first_pair, g, off in batches:
                    batch(plans[g], first_pair, g, off)
                if fold is not None:
                    fold(s0, c)

    def _error_moments(self, est: torch.Tensor, truth: torch.Tensor, rows: int, cols: int, observed: torch.Tensor,
                       available: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The fp64 device table of one ``gatres_node_error_moments`` launch over ``est`` / ``truth`` (``[rows, cols]``, ``truth``
        scaled) -- with ``available`` (``[rows, len(observed)]``: an entry at an observed node counts unless this is non-zero)
        of one ``gatres_node_error_moments_available`` launch."""
        lib, head = _native.load(), (est.data_ptr(), truth.data_ptr(), rows, cols, self.scale, self.offset, observed.data_ptr(),
                                     int(observed.numel()))
        with torch.cuda.device(self.device):
            stream = _native.current_stream(self.device)
            if available is None:
                table = torch.empty((cols, NODE_ERROR_RECORD), dtype=torch.float64, device=self.device)
                _native.check(lib.gatres_node_error_moments(*head, table.data_ptr(), stream), "gatres_node_error_moments")
            else:
                table = torch.empty((cols, NODE_ERROR_AVAIL_RECORD), dtype=torch.float64, device=self.device)
                _native.check(lib.gatres_node_error_moments_available(*head, available.data_ptr(), table.data_ptr(), stream),
                              "gatres_node_error_moments_available")
        return table

    def _judged(self, store, est: torch.Tensor, ints: Sequence[torch.Tensor] = ()) -> Tuple[float, np.ndarray]:
        """What a back-test report reads of one of its passes, in ONE read-back: the MAE of ``est`` over the nodes outside
        ``observed_idx`` (``error_map``'s ``hidden_mae``, from one moments launch) and, flat behind one another, the integer
        device tensors ``ints`` as host int64.  The integers travel as the bits of doubles: exact at any size."""
        n = self.nodes_per_graph * NODE_ERROR_RECORD
        table = self._error_moments(est, store.data, len(store), self.nodes_per_graph, self._observed)
        flat = torch.cat([table.reshape(-1)] + [t.to(torch.int64).reshape(-1).view(torch.float64) for t in ints])
        host = flat.cpu().numpy()
        return float(error_map_from_moments(host[:n])["hidden_mae"]), host[n:].view(np.int64)

    def _check_available(self, available, S: int) -> None:
        K = len(self.observed_idx)
        if (not isinstance(available, torch.Tensor) or available.dtype not in (torch.uint8, torch.bool)
                or tuple(available.shape) != (S, K) or available.device != self.device or not available.is_contiguous()):
            raise ValueError(f"available must be uint8 or bool, contiguous [{S}, {K}] on {self.device}")

    def _sigma(self, noise_std, layout: int) -> torch.Tensor:
        """``noise_std`` (physical units; one value or K of them) as the device ``sigma[K]`` of gatres_stage_observed_noisy: in
        the units of the launch's source, that is divided by ``std + eps`` for the full rows of a z-normalised store."""
        v = noise_sigma(noise_std, len(self.observed_idx), self.norm_type, self.std, self.eps,
                        full_rows=layout == _native.OBSERVED_FULL_ROWS)
        cached = self._sigma_cache.get(layout)
        if cached is None or cached[0] != v.tobytes():
            cached = self._sigma_cache[layout] = (v.tobytes(), torch.from_numpy(v).to(self.device))
        return cached[1]

    def _launches(self, src: torch.Tensor, layout: int, normalise: int, available, nan_is_missing: bool, noise,
                  dst: torch.Tensor):
        """The three launches of one batch as a function ``batch(P, first, g, off)`` for ``_pair_pass``: stage the ``g`` graphs
        from ``first`` on (source rows -- or, with ``noise = (sigma, seed, members, member0)``, pairs) into the plan ``P``, run
        the forward, write rows ``off ...`` of ``dst`` (a chunk's rows: the pass's result when it is one chunk)."""
        N, lib, flat, check = self.nodes_per_graph, _native.load(), self._parameters(), _native.check
        S, src_p, avail_p = int(src.shape[0]), src.data_ptr(), _native.ptr(available)
        dst_p, dst_rows = dst.data_ptr(), int(dst.shape[0])
        stream, nan, tail = _native.current_stream(self.device), int(bool(nan_is_missing)), self._staging_tail(normalise)
        with_gaps = available is not None or bool(nan_is_missing)
        scale, offset, keep = self.scale, self.offset, int(self.keep_observed)
        if noise is not None:
            sigma, seed, members, member0 = noise
            sigma_p = sigma.data_ptr()

        def batch(P, first, g, off):
            x, mask = P.x.data_ptr(), P.mask.data_ptr()
            if noise is not None:
                check(lib.gatres_stage_observed_noisy(src_p, layout, S, first, members, member0, N, g, *tail, x, mask, avail_p, nan,
                                                      sigma_p, seed, stream), "gatres_stage_observed_noisy")
            elif with_gaps:
                check(lib.gatres_stage_observed_available(src_p, layout, S, None, first, N, g, *tail, x, mask, avail_p, nan, stream),
                      "gatres_stage_observed_available")
            else:
                check(lib.gatres_stage_observed(src_p, layout, S, None, first, N, g, *tail, x, mask, stream), "gatres_stage_observed")
            _enqueue_forward(lib, flat, P, stream)
            check(lib.gatres_estimate_write(P.out.data_ptr(), x, mask, N, g, scale, offset, keep, dst_p, dst_rows, N, off, stream),
                  "gatres_estimate_write")

        return batch

    def _noise(self, noise_std, noise_seed, noise_member, layout: int):
        if noise_std is None:
            return None
        if isinstance(noise_member, bool) or not isinstance(noise_member, (int, np.integer)) or not 0 <= int(noise_member) < 1 << 62:
            raise ValueError(f"noise_member must be a non-negative integer; got {noise_member!r}")
        return self._sigma(noise_std, layout), _check_seed(noise_seed), 1, int(noise_member)

    def _run(self, src: torch.Tensor, layout: int, normalise: int, out: Optional[torch.Tensor],
             available: Optional[torch.Tensor] = None, nan_is_missing: bool = False, noise=None) -> torch.Tensor:
        S = int(src.shape[0])
        if available is not None:
            self._check_available(available, S)
        out = self._result(S, out)
        self._pair_pass(S, 1, None, self._launches(src, layout, normalise, available, nan_is_missing, noise, out))
        return out

    def _run_ensemble(self, src: torch.Tensor, layout: int, normalise: int, noise_std, members, seed, available,
                      nan_is_missing: bool, mean_out, std_out, max_scratch_bytes) -> Tuple[torch.Tensor, torch.Tensor]:
        N, S = self.nodes_per_graph, int(src.shape[0])
        if isinstance(members, bool) or not isinstance(members, (int, np.integer)) or int(members) < 1:
            raise ValueError(f"members must be a positive integer; got {members!r}")
        M = int(members)
        if int(max_scratch_bytes) <= 0:
            raise ValueError("max_scratch_bytes must be positive")
        if available is not None:
            self._check_available(available, S)
        noise = (self._sigma(noise_std, layout), _check_seed(seed), M, 0)
        mean, std = self._result(S, mean_out), self._result(S, std_out)
        if mean_out is not None and mean_out is std_out:
            raise ValueError("mean_out and std_out must be different tensors")
        C = ensemble_chunk(S, M, self.batch_size, 4 * N, max_scratch_bytes)
        lib, stream = _native.load(), _native.current_stream(self.device)
        scratch = torch.empty((C * M, N), dtype=torch.float32, device=self.device)

        def fold(s0, c):
            _native.check(lib.gatres_ensemble_reduce(scratch.data_ptr(), c, M, N, N, mean.data_ptr(), std.data_ptr(), S, N, s0,
                                                     stream), "gatres_ensemble_reduce")

        self._pair_pass(S, M, C, self._launches(src, layout, normalise, available, nan_is_missing, noise, scratch), fold)
        return mean, std

    def _check_readings(self, readings) -> None:
        K = len(self.observed_idx)
        if (not isinstance(readings, torch.Tensor) or readings.dtype != torch.float32 or readings.dim() != 2
                or readings.shape[1] != K or readings.shape[0] == 0 or readings.device != self.device
                or not readings.is_contiguous()):
            raise ValueError(f"readings must be fp32 contiguous [S, {K}] on {self.device}")

    def estimate(self, readings: torch.Tensor, out: Optional[torch.Tensor] = None, *,
                 available: Optional[torch.Tensor] = None, nan_is_missing: bool = False, noise_std=None, noise_seed: int = 0,
                 noise_member: int = 0) -> torch.Tensor:
        """``readings``: fp32 contiguous ``[S, K]`` on the model's device, in physical units, column ``k`` the sensor at
        ``observed_idx[k]``.  Returns the pressures ``[S, N_g]`` in physical units (``out``: write them there), a device tensor
        ordered on the current stream.

        ``available``: uint8 or bool contiguous ``[S, K]`` on the same device, non-zero where the reading is present;
        ``nan_is_missing``: a NaN reading is missing (decided on the device: nothing is scanned on the host).  A missing reading
        is not used: its node is hidden in that snapshot and, with ``keep_observed``, carries the model's prediction.  A
        snapshot without any reading is legal (the model's output on an all-zero input).

        ``noise_std`` (``None``: exactly the launches above): one noisy realisation of the readings.  A non-negative float, or
        a sequence of K of them, in physical units: every present reading ``r`` of sensor ``k`` in snapshot ``s`` is taken as
        ``r + float32(noise_std[k]) * z`` with ``z = reading_noise(noise_seed, 1, S, K, member0=noise_member)[s, 0, k]``, drawn
        in the staging launch (``gatres_stage_observed_noisy``); a missing reading draws nothing.  With ``keep_observed`` the
        sensor nodes of the result carry the NOISY reading after the normalise / descale round trip, not the one passed in."""
        self._check_readings(readings)
        noise = self._noise(noise_std, noise_seed, noise_member, _native.OBSERVED_READINGS)
        return self._run(readings, _native.OBSERVED_READINGS, self._normalise, out, available, nan_is_missing, noise)

    def estimate_store(self, store, out: Optional[torch.Tensor] = None, *,
                       available: Optional[torch.Tensor] = None, noise_std=None, noise_seed: int = 0,
                       noise_member: int = 0) -> torch.Tensor:
        """The same for every snapshot of a ``SnapshotStore``, in store order, with everything but the sensors hidden --
        and, with ``available`` (``[len(store), K]``), the sensors without a reading too.  ``noise_std`` (physical units, as in
        ``estimate``): the store's normalised sensor entries get ``float32(noise_std[k] / (std + eps)) * z`` (``float32(noise_std[k])
        * z`` for an ``unused`` store); with ``keep_observed`` the sensor nodes carry the noisy value."""
        self._check_store(store)
        noise = self._noise(noise_std, noise_seed, noise_member, _native.OBSERVED_FULL_ROWS)
        return self._run(store.data, _native.OBSERVED_FULL_ROWS, _native.NORMALISE_NONE, out, available, False, noise)

    def fine_tune(self, train_store, val_store, epochs: int, *, lr: float, batch_size: Optional[int] = None,
                  sensor_dropout: float = 0.0, layout_share: float = 1.0, mask_rate: float = 0.95, noise_std=None,
                  noise_seed: Optional[int] = None, **fit_kw):
        """Fine-tune the estimator's model to its own sensor layout: ``GATResTrainer.for_store(model, train_store, batch_size,
        lr=lr, mask_rate=mask_rate)``, ``set_sensor_layout(observed_idx, sensor_dropout=..., layout_share=...)`` and
        ``fit(train_store, val_store, epochs, **fit_kw)`` -- validated under the layout mask unless ``val_layout=False`` is
        passed on.  ``batch_size`` defaults to the estimator's.  Returns the ``FitHistory``.  The training happens in the model's
        own parameter vector, which every estimate reads at its launches: the estimator estimates with the tuned parameters
        from the next call on, nothing is refreshed.  The trainer's constructor arguments other than ``lr`` and ``mask_rate``
        keep their defaults: build the trainer yourself for anything else.

        ``noise_std`` / ``noise_seed`` (``set_sensor_layout``'s: physical units, one value or one per sensor; the seed defaults to
        the trainer's): fine-tune under measurement noise on the kept readings -- what makes a model that ``noise_report`` shows
        to be fragile robust.  ``fit`` then validates under the same ``noise_std`` with a fixed realisation (``val_noise``,
        ``val_noise_seed`` in ``fit_kw``)."""
        from .train_step import GATResTrainer
        self._check_store(train_store)
        self._check_store(val_store)
        bs = self.batch_size if batch_size is None else int(batch_size)
        trainer = GATResTrainer.for_store(self.model, train_store, bs, lr=lr, mask_rate=mask_rate)
        trainer.set_sensor_layout(self.observed_idx, sensor_dropout=sensor_dropout, layout_share=layout_share,
                                  noise_std=noise_std, noise_seed=noise_seed)
        return trainer.fit(train_store, val_store, int(epochs), batch_size=bs, **fit_kw)

    def estimate_ensemble(self, readings: torch.Tensor, noise_std, members: int, *, seed: int = 0,
                          available: Optional[torch.Tensor] = None, nan_is_missing: bool = False,
                          mean_out: Optional[torch.Tensor] = None, std_out: Optional[torch.Tensor] = None,
                          max_scratch_bytes: int = 64 << 20) -> Tuple[torch.Tensor, torch.Tensor]:
        """A Monte-Carlo ensemble under measurement noise: for every snapshot of ``readings`` (as in ``estimate``) the mean and
        the sample standard deviation (``M - 1`` in the denominator; 0 for one member), per junction, of the estimates from
        ``members`` noisy realisations -- member ``m`` is ``estimate(readings, noise_std=noise_std, noise_seed=seed,
        noise_member=m)`` up to the batch it is computed in.  Returns ``(mean, std)``, fp32 ``[S, N_g]`` device tensors in
        physical units ordered on the current stream (``mean_out`` / ``std_out``: write them there).

        One pass over the S * M (snapshot, member) pairs -- one snapshot's 32 members at batch size 32 are ONE forward launch --
        with the three launches of ``estimate`` per batch.  The members' estimates go to a scratch matrix of at most
        ``max_scratch_bytes`` (``ensemble_chunk``, at least one unit of it), one ``gatres_ensemble_reduce`` launch per chunk folds
        them in fp64 in member order.  The bits of the result depend on neither the budget nor the run.  Nothing is read back,
        nothing synchronises."""
        self._check_readings(readings)
        return self._run_ensemble(readings, _native.OBSERVED_READINGS, self._normalise, noise_std, members, seed, available,
                                  nan_is_missing, mean_out, std_out, max_scratch_bytes)

    def estimate_store_ensemble(self, store, noise_std, members: int, *, seed: int = 0,
                                available: Optional[torch.Tensor] = None, mean_out: Optional[torch.Tensor] = None,
                                std_out: Optional[torch.Tensor] = None,
                                max_scratch_bytes: int = 64 << 20) -> Tuple[torch.Tensor, torch.Tensor]:
        """``estimate_ensemble`` over the snapshots of a ``SnapshotStore`` (noise in physical units, scaled as in
        ``estimate_store``)."""
        self._check_store(store)
        return self._run_ensemble(store.data, _native.OBSERVED_FULL_ROWS, _native.NORMALISE_NONE, noise_std, members, seed,
                                  available, False, mean_out, std_out, max_scratch_bytes)

    def noise_report(self, store, noise_std, members: int, *, seed: int = 0,
                     available: Optional[torch.Tensor] = None) -> Dict[str, object]:
        """Which junctions are sensitive to sensor error: ``estimate_store_ensemble(store, noise_std, members, seed=seed,
        available=available)``, then ``error`` = ``error_map(store, estimates=mean, available=available)`` of the ensemble mean
        and, from one ``gatres_node_spread_moments`` launch over the standard deviations, the entries of
        ``noise_report_from_moments``: ``spread``, ``max_std``, ``mean_std`` per node, ``nonsensor_spread`` and
        ``most_sensitive``.  Two read-backs: the error table and the spread table."""
        mean, std = self.estimate_store_ensemble(store, noise_std, members, seed=seed, available=available)
        out: Dict[str, object] = {"error": self.error_map(store, estimates=mean, available=available)}
        table = torch.empty((self.nodes_per_graph, NODE_SPREAD_RECORD), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            _native.check(_native.load().gatres_node_spread_moments(
                std.data_ptr(), len(store), self.nodes_per_graph, table.data_ptr(), _native.current_stream(self.device)),
                "gatres_node_spread_moments")
        out.update(noise_report_from_moments(table.cpu().numpy(), self.observed_idx))
        return out

    def _score_mask(self, score_nodes) -> Optional[torch.Tensor]:
        """``score_nodes`` as the device uint8 ``[N]`` of gatres_layout_pair_errors (``None``: every node); uploaded when it
        changes."""
        if score_nodes is None:
            return None
        N = self.nodes_per_graph
        nodes = [int(v) for v in score_nodes]
        bad = [v for v in nodes if v < 0 or v >= N]
        if bad or not nodes:
            raise ValueError(f"score_nodes must be node indices in [0, {N}), at least one; got {bad[0] if bad else 'none'}")
        if len(set(nodes)) != len(nodes):
            raise ValueError("score_nodes holds duplicates")
        key = tuple(nodes)
        cached = self._score_cache
        if cached is None or cached[0] != key:
            m = np.zeros(N, dtype=np.uint8)
            m[nodes] = 1
            cached = self._score_cache = (key, torch.from_numpy(m).to(self.device))
        return cached[1]

    def layout_errors(self, store, layouts: torch.Tensor, *, available: Optional[torch.Tensor] = None, score_nodes=None,
                      out: Optional[torch.Tensor] = None, max_scratch_bytes: int = 64 << 20) -> torch.Tensor:
        """The back-test error of L sensor layouts over the store's snapshots, on the device.  ``layouts``: uint8 or bool,
        contiguous ``[L, K]`` on the model's device, non-zero where sensor ``observed_idx[k]`` is installed in the layout: the
        estimator's sensors are the CANDIDATES, a layout is a subset of them (an empty layout is legal).  Returns the fp64
        device table ``[L, LAYOUT_ERROR_RECORD]`` (``out``: write it there), ordered on the current stream: per layout the
        number of entries scored, sum |e|, sum e^2 and max |e| (``layout_scores_from_table``), ``e`` the error of the model's
        prediction against the store's descaled value as in ``error_map``.  Scored are the nodes HIDDEN in the layout (every
        node without an installed sensor with a reading, as ``error_map(available=...)``'s ``hidden_*``) -- with ``score_nodes``
        (node indices) only those of them: a pool disjoint from the candidates gives every layout the same pool.
        ``available`` (``[len(store), K]``) takes readings away in every layout, as in ``estimate_store``.

        One pass over the S * L (snapshot, layout) pairs with three launches per batch (``gatres_stage_observed_layouts``, the
        forward, ``gatres_layout_pair_errors``): the estimates are never written out.  The pairs' records go to a scratch of at
        most ``max_scratch_bytes`` (``ensemble_chunk``), one ``gatres_layout_error_reduce`` launch per chunk folds them in
        snapshot order: the bits of the table depend on neither the budget nor the run.  Nothing is read back, nothing
        synchronises."""
        self._check_store(store)
        K, N, S = len(self.observed_idx), self.nodes_per_graph, len(store)
        if (not isinstance(layouts, torch.Tensor) or layouts.dtype not in (torch.uint8, torch.bool) or layouts.dim() != 2
                or layouts.shape[1] != K or layouts.shape[0] == 0 or layouts.device != self.device or not layouts.is_contiguous()):
            raise ValueError(f"layouts must be uint8 or bool, contiguous [L, {K}] on {self.device}")
        L = int(layouts.shape[0])
        if available is not None:
            self._check_available(available, S)
        if int(max_scratch_bytes) <= 0:
            raise ValueError("max_scratch_bytes must be positive")
        score = self._score_mask(score_nodes)
        out = self._out(out, (L, LAYOUT_ERROR_RECORD), torch.float64)
        C = ensemble_chunk(S, L, self.batch_size, 8 * LAYOUT_PAIR_RECORD, max_scratch_bytes)
        lib, flat, stream, check = _native.load(), self._parameters(), _native.current_stream(self.device), _native.check
        rec = torch.empty((C * L, LAYOUT_PAIR_RECORD), dtype=torch.float64, device=self.device)
        stage, errors, full_rows = lib.gatres_stage_observed_layouts, lib.gatres_layout_pair_errors, _native.OBSERVED_FULL_ROWS
        src_p, rec_p, rec_rows, scale, offset = store.data.data_ptr(), rec.data_ptr(), C * L, self.scale, self.offset
        avail_p, layouts_p, score_p = _native.ptr(available), layouts.data_ptr(), _native.ptr(score)
        # (a store's rows are normalised already.  Under NORMALISE_NONE the staging launch reads neither the tail's offset nor
        # its factor -- obs_normalise returns the value, the scale stays 1 -- so they may be the estimator's: the same bits)
        tail = self._staging_tail(_native.NORMALISE_NONE)

        def batch(P, first, g, off):
            mask = P.mask.data_ptr()
            check(stage(src_p, full_rows, S, first, L, N, g, *tail, P.x.data_ptr(), mask, avail_p, 0, layouts_p, stream),
                  "gatres_stage_observed_layouts")
            _enqueue_forward(lib, flat, P, stream)
            check(errors(P.out.data_ptr(), mask, src_p, S, N, g, first, L, scale, offset, score_p, rec_p, rec_rows, off,
                         stream), "gatres_layout_pair_errors")

        def fold(s0, c):
            check(lib.gatres_layout_error_reduce(rec_p, c, L, out.data_ptr(), int(s0 > 0), stream), "gatres_layout_error_reduce")

        self._pair_pass(S, L, C, batch, fold)
        return out

    @classmethod
    def place_sensors(cls, model, store, num_sensors: int, *, candidates: Optional[Sequence[int]] = None,
                      fixed: Sequence[int] = (), criterion: str = "mae", score_nodes=None, batch_size: int = 32,
                      available: Optional[torch.Tensor] = None, **kw) -> Dict[str, object]:
        """Where to put ``num_sensors`` sensors: greedy forward selection (``greedy_selection``) among ``candidates`` (node
        indices; ``None``: every node not in ``fixed``) on top of the sensors ``fixed`` that are there already (may be empty:
        the first round then scores single-sensor layouts), by the back-test error over ``store``.  ``criterion``: ``"mae"``,
        ``"rmse"`` or ``"max_abs"`` of ``layout_scores_from_table``.

        One estimator with ``observed_idx = list(fixed) + list(candidates)`` serves every round (``batch_size`` and ``**kw`` go to
        ``for_store``; ``available``: ``[len(store), len(fixed) + len(candidates)]`` in that column order).  A round is ONE
        ``layout_errors`` call -- the layouts ``fixed + chosen + {c}``, one per remaining candidate ``c`` -- and ONE read-back of
        its table.  The error is pooled over the nodes hidden in the layout, so the pool shrinks by the node a candidate
        occupies; ``score_nodes`` restricts it to those of the given nodes that are hidden, and a pool disjoint from the
        candidates and from ``fixed`` gives every layout the same pool.

        Returns ``observed_idx`` (``fixed`` plus the chosen nodes in order of choice: ready for ``for_store``), ``chosen``,
        ``scores`` (the winning score of each round) and ``rounds``: per round a dict with ``candidates`` (the remaining nodes,
        in ``candidates`` order) and the ``layout_scores_from_table`` entries, one value per candidate."""
        _refuse_multi(store)
        fix, cand = _check_placement(store.nodes_per_graph, num_sensors, candidates, fixed, criterion)
        est = cls.for_store(model, store, fix + cand, batch_size=batch_size, **kw)
        F, K = len(fix), len(fix) + len(cand)
        column = {c: F + i for i, c in enumerate(cand)}
        rounds: List[Dict[str, object]] = []

        def score_round(chosen, remaining):
            lay = np.zeros((len(remaining), K), dtype=np.uint8)
            lay[:, :F] = 1
            lay[:, [column[c] for c in chosen]] = 1
            lay[np.arange(len(remaining)), [column[c] for c in remaining]] = 1
            table = est.layout_errors(store, torch.from_numpy(lay).to(est.device), available=available, score_nodes=score_nodes)
            scores = layout_scores_from_table(table.cpu().numpy())
            rounds.append({"candidates": list(remaining), **scores})
            return scores[criterion]

        chosen, scores = greedy_selection(score_round, cand, int(num_sensors))
        return {"observed_idx": fix + chosen, "chosen": chosen, "scores": scores, "rounds": rounds}

    def error_map(self, store, estimates: Optional[torch.Tensor] = None, *,
                  available: Optional[torch.Tensor] = None) -> Dict[str, np.ndarray]:
        """Back-test report per node over the store's snapshots (``error_map_from_moments``): the estimates (``None``:
        ``estimate_store(store)``) against the store's descaled values.  One ``gatres_node_error_moments`` launch, one
        read-back.  With ``available`` (``[len(store), K]``) the estimates it forms itself use it and the report is over the
        hidden entries (``error_map_from_moments(table, available=True, observed_idx=...)``), from one
        ``gatres_node_error_moments_available`` launch."""
        self._check_store(store)
        if available is not None:
            self._check_available(available, len(store))
        est = self.estimate_store(store, available=available) if estimates is None else self._result(len(store), estimates)
        table = self._error_moments(est, store.data, len(store), self.nodes_per_graph, self._observed, available)
        if available is None:
            return error_map_from_moments(table.cpu().numpy())
        return error_map_from_moments(table.cpu().numpy(), available=True, observed_idx=self.observed_idx)

    # ---- calibrated error bounds ------------------------------------------------------------------------------------------------
    def _error_inputs(self, store, estimates, available, noise_std, noise_seed) -> torch.Tensor:
        self._check_store(store)
        if available is not None:
            self._check_available(available, len(store))
        if estimates is None:
            return self.estimate_store(store, available=available, noise_std=noise_std, noise_seed=noise_seed)
        return self._result(len(store), estimates)

    def calibrate_bounds(self, store, levels=(0.9,), *, estimates: Optional[torch.Tensor] = None,
                         available: Optional[torch.Tensor] = None, noise_std=None, noise_seed: int = 0) -> ErrorBounds:
        """Split-conformal error bounds per junction from a held-out ``store`` (not the training data): for every level ``q`` of
        ``levels`` (1 to 8 floats in (0, 1), strictly increasing) and every node ``v`` the element of rank
        ``conformal_rank(n_v, q)`` of ``|estimate - truth|`` over the store's snapshots.  If a new snapshot is exchangeable with
        the store's, ``|estimate - truth| <= bounds[q, v]`` holds with probability >= ``q``, per node (not jointly over the
        nodes); with fewer than ``q / (1 - q)`` snapshots no finite bound has that coverage and the bound is +inf.

        The estimates are ``estimates`` (fp32 ``[len(store), N_g]`` on the device) or ``estimate_store(store, available=,
        noise_std=, noise_seed=)``.  With ``noise_std`` the calibration errors contain one noisy realisation of the readings per
        snapshot, so one number covers model error and sensor error.  With ``available`` (``[len(store), K]``) the bound at a
        sensor node is over the snapshots in which its reading was missing (as ``error_map(available=)``): a sensor that
        always delivered gets ``counts = 0`` and +inf.  With ``keep_observed`` the bounds at sensor nodes are those of the
        normalise / descale round trip of the reading itself (about 0), not of the model; the reports pool over the nodes
        outside ``observed_idx``, as ``error_map`` does.

        One ``gatres_node_error_quantiles`` launch behind the pass.  Nothing is read back and nothing synchronises: the
        ``ErrorBounds`` hold device tensors ordered on the current stream."""
        lv = _check_levels(levels)
        est = self._error_inputs(store, estimates, available, noise_std, noise_seed)
        N, Q = self.nodes_per_graph, len(lv)
        bounds = torch.empty((Q, N), dtype=torch.float32, device=self.device)
        counts = torch.empty((N,), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            _native.check(_native.load().gatres_node_error_quantiles(
                est.data_ptr(), store.data.data_ptr(), len(store), N, self.scale, self.offset, self._observed.data_ptr(),
                len(self.observed_idx), _native.ptr(available), (ctypes.c_double * Q)(*lv), Q, bounds.data_ptr(),
                counts.data_ptr(), _native.current_stream(self.device)), "gatres_node_error_quantiles")
        return ErrorBounds(lv, bounds, counts, self.observed_idx)

    def _check_bounds(self, bounds) -> None:
        if not isinstance(bounds, ErrorBounds):
            raise ValueError("bounds must be the ErrorBounds of calibrate_bounds")
        if bounds.observed_idx != self.observed_idx:
            raise ValueError(f"the bounds were calibrated for the sensor layout {bounds.observed_idx}, the estimator's is "
                             f"{self.observed_idx}")
        if bounds.nodes_per_graph != self.nodes_per_graph:
            raise ValueError(f"the bounds cover {bounds.nodes_per_graph} nodes, the estimator {self.nodes_per_graph}")
        if bounds.device != self.device or not bounds.bounds.is_contiguous():
            raise ValueError(f"the bounds must be contiguous on {self.device} (got {bounds.device})")

    def coverage_report(self, store, bounds: ErrorBounds, *, estimates: Optional[torch.Tensor] = None,
                        available: Optional[torch.Tensor] = None, noise_std=None, noise_seed: int = 0) -> Dict[str, object]:
        """How often the bounds held over ``store`` (a test store: on the calibration store itself the coverage is at least the
        level by construction): the entries of ``coverage_from_table``.  The estimates as in ``calibrate_bounds``.  One
        ``gatres_node_bound_coverage`` launch and one read-back, of the table and the bounds together."""
        self._check_bounds(bounds)
        est = self._error_inputs(store, estimates, available, noise_std, noise_seed)
        N, Q = self.nodes_per_graph, len(bounds.levels)
        table = torch.empty((N, NODE_COVERAGE_RECORD), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            _native.check(_native.load().gatres_node_bound_coverage(
                est.data_ptr(), store.data.data_ptr(), len(store), N, self.scale, self.offset, self._observed.data_ptr(),
                len(self.observed_idx), _native.ptr(available), bounds.bounds.data_ptr(), Q, table.data_ptr(),
                _native.current_stream(self.device)), "gatres_node_bound_coverage")
        # (one transfer: fp32 -> fp64 is exact)
        both = torch.cat([table.reshape(-1), bounds.bounds.reshape(-1).to(torch.float64)]).cpu().numpy()
        return coverage_from_table(both[:N * NODE_COVERAGE_RECORD], both[N * NODE_COVERAGE_RECORD:].reshape(Q, N),
                                   bounds.levels, self.observed_idx)

    def estimate_with_bounds(self, readings: torch.Tensor, bounds: ErrorBounds, level=None,
                             **estimate_kw) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """``est = estimate(readings, **estimate_kw)`` and ``(lo, hi) = bounds.interval(est, level)`` (``level=None``: the
        bounds hold one level): the pressure at every junction with its calibrated interval, all on the device.  No launch
        beyond those of ``estimate`` and torch's two element passes."""
        self._check_bounds(bounds)
        bounds.level_index(level)                                   # (refused before the pass)
        est = self.estimate(readings, **estimate_kw)
        lo, hi = bounds.interval(est, level)
        return est, lo, hi

    def reading_residuals(self, readings: torch.Tensor, bounds, level=None, *,
                          nan_is_missing: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
        """Is a reading plausible given the others?  For every sensor column ``k`` one ``estimate(readings, available=)`` with
        column ``k`` unavailable in every snapshot; ``residual[:, k]`` = reading - prediction at ``observed_idx[k]`` and
        ``flagged[:, k]`` = ``|residual| > b_k``, ``b_k`` the bound at that node with the reading hidden.  Returns
        ``(residual[S, K] fp32, flagged[S, K] bool)`` on the device; K passes, nothing read back.

        ``bounds``: a list of K ``ErrorBounds``, the k-th from ``calibrate_bounds(store, available=a_k)`` with ``a_k`` all ones
        but column ``k``, which is all zero -- the same column hidden as here; or ONE ``ErrorBounds`` that holds such a bound
        at every sensor node (for a single sensor: made with ``available`` all zero in its column).  Bounds calibrated
        without ``available`` are those of the sensors' own values (about 0 with ``keep_observed``) and would flag
        everything.  A missing reading (``nan_is_missing``) gives a NaN residual and is not flagged."""
        self._check_readings(readings)
        K, S = len(self.observed_idx), int(readings.shape[0])
        each = list(bounds) if isinstance(bounds, (list, tuple)) else [bounds] * K
        if len(each) != K:
            raise ValueError(f"bounds must be one ErrorBounds or a list of {K}, one per sensor; got {len(each)}")
        for b in each:
            self._check_bounds(b)
        rows = [b.bounds[b.level_index(level)] for b in each]
        available = torch.ones((S, K), dtype=torch.uint8, device=self.device)
        est = torch.empty((S, self.nodes_per_graph), dtype=torch.float32, device=self.device)
        residual = torch.empty((S, K), dtype=torch.float32, device=self.device)
        flagged = torch.empty((S, K), dtype=torch.bool, device=self.device)
        for k, v in enumerate(self.observed_idx):
            available[:, k] = 0
            self.estimate(readings, out=est, available=available, nan_is_missing=nan_is_missing)
            available[:, k] = 1
            residual[:, k] = readings[:, k] - est[:, v]
            flagged[:, k] = residual[:, k].abs() > rows[k][v]
        return residual, flagged

    def sensor_failure_report(self, store, sensors: Optional[Sequence[int]] = None) -> Dict[str, object]:
        """Leave-one-out back-test of the sensor layout over ``store``: a baseline pass with every reading available, then for
        each position ``k`` of ``sensors`` (columns of the readings; ``None``: all K) one ``estimate_store`` + ``error_map``
        with column ``k`` unavailable in every snapshot.  One ``available`` buffer and one estimates buffer serve every pass;
        one read-back per pass.  Returns ``sensors``, ``baseline`` (that pass's report), and per failed sensor
        ``nonsensor_mae`` / ``nonsensor_rmse`` (over the nodes outside ``observed_idx``: the same pool as the baseline's),
        ``failed_sensor_mae`` (the MAE at node ``observed_idx[k]`` while it is failed) and ``delta_nonsensor_mae`` =
        ``nonsensor_mae - baseline["nonsensor_mae"]``."""
        self._check_store(store)
        K, S = len(self.observed_idx), len(store)
        cols = list(range(K)) if sensors is None else [int(k) for k in sensors]
        bad = [k for k in cols if k < 0 or k >= K]
        if bad:
            raise ValueError(f"sensors are positions in observed_idx, in [0, {K}); got {bad[0]}")
        available = torch.ones((S, K), dtype=torch.uint8, device=self.device)
        est = torch.empty((S, self.nodes_per_graph), dtype=torch.float32, device=self.device)

        def one_pass():
            self.estimate_store(store, out=est, available=available)
            return self.error_map(store, estimates=est, available=available)

        baseline = one_pass()
        mae, rmse, failed = (np.full(len(cols), np.nan, dtype=np.float64) for _ in range(3))
        for i, k in enumerate(cols):
            available[:, k] = 0
            m = one_pass()
            available[:, k] = 1
            mae[i], rmse[i], failed[i] = m["nonsensor_mae"], m["nonsensor_rmse"], m["mae"][self.observed_idx[k]]
        return {"sensors": cols, "baseline": baseline, "nonsensor_mae": mae, "nonsensor_rmse": rmse,
                "failed_sensor_mae": failed, "delta_nonsensor_mae": mae - baseline["nonsensor_mae"]}

    # ---- sensitivity ------------------------------------------------------------------------------------------------------------
    def _targets(self, targets) -> Tuple[List[int], Optional[torch.Tensor]]:
        """``targets`` (node indices; ``None``: every junction, in node order) as (list, device int32 ``[T]`` or ``None`` for
        all); uploaded when they change."""
        N = self.nodes_per_graph
        if targets is None:
            return list(range(N)), None
        try:
            nodes = [int(v) for v in targets]
        except (TypeError, ValueError):
            raise ValueError(f"targets must be node indices in [0, {N})") from None
        bad = [v for v in nodes if v < 0 or v >= N]
        if bad or not nodes:
            raise ValueError(f"targets must be node indices in [0, {N}), at least one; got {bad[0] if bad else 'none'}")
        key = tuple(nodes)
        cached = self._targets_cache
        if cached is None or cached[0] != key:
            cached = self._targets_cache = (key, torch.tensor(nodes, dtype=torch.int32).to(self.device))
        return nodes, cached[1]

    def _sensitivity_buffers(self, P):
        """The backward's buffers for the plan ``P``: the saved activations, the seeds, ``g_x`` and the throw-away parameter
        gradient.  Allocated once per plan and kept."""
        flat = self.model.flat_parameters
        key = (P.num_nodes, int(P.state["saved_floats"]), int(flat.numel()))
        bufs = self._sens_buffers.get(key)
        if bufs is None:
            f32 = dict(dtype=torch.float32, device=self.device)
            bufs = self._sens_buffers[key] = (torch.empty(P.state["saved_floats"], **f32), torch.empty(P.num_nodes, **f32),
                                              torch.empty(P.num_nodes, **f32), torch.empty(flat.numel(), **f32))
        return bufs

    def _scratch(self, name: str, shape, dtype=torch.float32) -> torch.Tensor:
        buf = self._sens_scratch.get(name)
        if buf is None or tuple(buf.shape) != tuple(shape) or buf.dtype != dtype:
            buf = self._sens_scratch[name] = torch.empty(tuple(shape), dtype=dtype, device=self.device)
        return buf

    def _sensitivity_launches(self, src: torch.Tensor, layout: int, normalise: int, targets_dev, T: int, available,
                              nan_is_missing: bool, J: torch.Tensor):
        """The four launches of one batch of (snapshot, target) pairs as a function ``batch(P, first_pair, g, off)`` for
        ``_pair_pass``: stage the ``g`` pairs from ``first_pair`` on into the plan ``P`` with their seeds, run the forward keeping
        the activations and the backward with ``g_x`` -- the two calls the module's autograd node enqueues, with the training
        model reference and a throw-away parameter gradient --, gather the sensors' entries into rows ``off ...`` of ``J`` (a
        chunk's rows of K: the pass's result when it is one chunk)."""
        N, K, lib, check = self.nodes_per_graph, len(self.observed_idx), _native.load(), _native.check
        S, J_p, J_rows = int(src.shape[0]), J.data_ptr(), J.numel() // K
        unit = self.scale / self._factor                        # d physical estimate / d physical reading per d out / d x
        stream, nan, tail = _native.current_stream(self.device), int(bool(nan_is_missing)), self._staging_tail(normalise)
        flat_p, src_p, observed_p = self._parameters().data_ptr(), src.data_ptr(), self._observed.data_ptr()
        targets_p, avail_p = _native.ptr(targets_dev), _native.ptr(available)

        def batch(P, first_pair, g, off):
            saved, g_out, g_x, grads = self._sensitivity_buffers(P)
            st = P.state
            x, mask, scratch = P.x.data_ptr(), P.mask.data_ptr(), st["scratch"].data_ptr()
            check(lib.gatres_stage_observed_targets(src_p, layout, S, first_pair, T, targets_p, N, g, *tail, x, mask,
                                                    g_out.data_ptr(), avail_p, nan, stream), "gatres_stage_observed_targets")
            check(lib.gatres_model_forward(st["mref"], st["gref"], flat_p, x, None, P.out.data_ptr(), saved.data_ptr(), scratch,
                                           stream), "gatres_model_forward")
            check(lib.gatres_model_backward(st["mref"], st["gref"], flat_p, x, None, g_out.data_ptr(), saved.data_ptr(), scratch,
                                            grads.data_ptr(), g_x.data_ptr(), stream), "gatres_model_backward")
            # (fault: the last float of the parameter gradient, lin1.bias -- a NaN there marks a failed split launch)
            check(lib.gatres_sensitivity_gather(g_x.data_ptr(), mask, grads.data_ptr() + 4 * (grads.numel() - 1), N, g, observed_p,
                                                K, unit, J_p, J_rows, K, off, stream), "gatres_sensitivity_gather")

        return batch

    def _run_sensitivity(self, src: torch.Tensor, layout: int, normalise: int, targets, available, nan_is_missing: bool,
                         out: Optional[torch.Tensor]) -> torch.Tensor:
        S, K = int(src.shape[0]), len(self.observed_idx)
        nodes, targets_dev = self._targets(targets)
        T = len(nodes)
        if available is not None:
            self._check_available(available, S)
        out = self._out(out, (S, T, K))
        self._pair_pass(S, T, None, self._sensitivity_launches(src, layout, normalise, targets_dev, T, available,
                                                               nan_is_missing, out))
        return out

    def _store_rows(self, store, first, count) -> Tuple[torch.Tensor, int]:
        """The snapshots ``[first, first + count)`` of ``store`` (``count=None``: to the end) as a view of its matrix."""
        self._check_store(store)
        n = len(store)
        for name, v in (("first", first), ("count", count)):
            if v is not None and (isinstance(v, bool) or not isinstance(v, (int, np.integer))):
                raise ValueError(f"{name} must be an integer; got {v!r}")
        first = int(first)
        count = n - first if count is None else int(count)
        if first < 0 or count < 1 or first + count > n:
            raise ValueError(f"first / count must name snapshots inside the store: [{first}, {first + count}) of {n}")
        return store.data[first:first + count], count

    def sensitivity(self, readings: torch.Tensor, *, targets=None, available: Optional[torch.Tensor] = None,
                    nan_is_missing: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Which readings an estimate rests on, and by how much: the Jacobian ``J[s, t, k] = d p[s, targets[t]] / d
        readings[s, k]`` of the model's prediction ``p`` (physical units) at the junction ``targets[t]`` with respect to the
        reading of the sensor at ``observed_idx[k]`` (physical units), for every snapshot of ``readings`` (as in ``estimate``).
        ``targets``: node indices (``None``: every junction, in node order).  Returns fp32 ``[S, T, K]`` (``out``: write it
        there), a device tensor ordered on the current stream; nothing is read back.

        The rows describe the MODEL'S PREDICTION at every node, sensor nodes included, whatever ``keep_observed`` says: the
        self-entry ``J[s, t, k]`` at ``targets[t] == observed_idx[k]`` is how far the model's own prediction at a sensor
        follows that sensor (with ``keep_observed`` the estimate there is the reading itself, whose derivative is trivially 1).
        A missing reading (``available`` / ``nan_is_missing``, as in ``estimate``) is no input of that snapshot: its column is
        exactly 0 there.  The network is piecewise linear in the readings up to the attention softmax, so ``J`` is the exact
        derivative at these readings, not a finite difference.

        Reverse mode: one pass over the S * T (snapshot, target) pairs, four launches per batch:
        ``gatres_stage_observed_targets`` (the staging of ``estimate`` plus the pair's seed ``e_j``), the forward keeping its
        activations, the backward with ``g_x``, ``gatres_sensitivity_gather``.  A full Jacobian of one snapshot is ``ceil(N_g /
        batch_size)`` batches.  The backward's buffers are allocated once per plan and kept on the estimator."""
        self._check_readings(readings)
        return self._run_sensitivity(readings, _native.OBSERVED_READINGS, self._normalise, targets, available, nan_is_missing, out)

    def sensitivity_store(self, store, *, first: int = 0, count: Optional[int] = None, targets=None,
                          available: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``sensitivity`` for the snapshots ``[first, first + count)`` of a ``SnapshotStore`` (``count=None``: to the end), with
        everything but the sensors hidden; ``available``: ``[count, K]``, row ``i`` for snapshot ``first + i``.  In physical
        units per physical unit, as ``sensitivity``."""
        src, _ = self._store_rows(store, first, count)
        return self._run_sensitivity(src, _native.OBSERVED_FULL_ROWS, _native.NORMALISE_NONE, targets, available, False, out)

    def sensitivity_map(self, store, *, first: int = 0, count: Optional[int] = None, targets=None,
                        available: Optional[torch.Tensor] = None, max_scratch_bytes: int = 64 << 20) -> "SensitivityMap":
        """The influence of the sensor layout over a store: ``sensitivity_store`` folded per (junction, sensor) over the
        snapshots on the device -- the number of non-zero entries, sum J, sum \\|J\\|, sum J^2 and max \\|J\\|
        (``gatres_sensitivity_fold``; ``influence_from_table`` reads the table).  The ``[S, T, K]`` tensor is never formed: the
        pass runs in chunks of snapshots whose rows fit ``max_scratch_bytes`` (``ensemble_chunk``: whole snapshots and whole
        batches, so the batches are those of ``sensitivity_store``), one fold per chunk in snapshot order: the bits of the
        table depend on neither the budget nor the run.  Nothing is read back."""
        src, S = self._store_rows(store, first, count)
        if isinstance(max_scratch_bytes, bool) or int(max_scratch_bytes) <= 0:
            raise ValueError("max_scratch_bytes must be positive")
        nodes, targets_dev = self._targets(targets)
        T, K = len(nodes), len(self.observed_idx)
        if available is not None:
            self._check_available(available, S)
        C = ensemble_chunk(S, T, self.batch_size, 4 * K, max_scratch_bytes)
        table = torch.empty((T, K, SENSITIVITY_RECORD), dtype=torch.float64, device=self.device)
        lib, stream, J = _native.load(), _native.current_stream(self.device), self._scratch("map", (C * T, K))

        def fold(s0, c):
            _native.check(lib.gatres_sensitivity_fold(J.data_ptr(), c, T, K, K, table.data_ptr(), int(s0 > 0), stream),
                          "gatres_sensitivity_fold")

        self._pair_pass(S, T, C, self._sensitivity_launches(src, _native.OBSERVED_FULL_ROWS, _native.NORMALISE_NONE, targets_dev,
                                                            T, available, False, J), fold)
        return SensitivityMap(table, nodes, self.observed_idx, S)

    def influence_report(self, store_or_map, **kw) -> Dict[str, object]:
        """``influence_from_table`` of a ``SensitivityMap`` -- or of ``sensitivity_map(store, **kw)`` when given a store: per
        (junction, sensor) the mean, mean absolute and rms sensitivity, per junction the dominant sensor, its share and the
        participation ratio, per sensor its total influence, the junctions it dominates and its self-entry.  ONE read-back:
        the table."""
        if isinstance(store_or_map, SensitivityMap) and kw:
            raise ValueError("influence_report of a SensitivityMap takes no further arguments")
        m = store_or_map if isinstance(store_or_map, SensitivityMap) else self.sensitivity_map(store_or_map, **kw)
        return influence_from_table(m.table.cpu().numpy(), m.targets, m.observed_idx, m.num_snapshots)

    def _run_linear_spread(self, src: torch.Tensor, layout: int, normalise: int, noise_std, available, nan_is_missing: bool,
                           out: Optional[torch.Tensor]) -> torch.Tensor:
        S, N, K = int(src.shape[0]), self.nodes_per_graph, len(self.observed_idx)
        # (J is in physical units per PHYSICAL unit of a reading in both layouts: sigma in physical units)
        sigma = self._sigma(noise_std, _native.OBSERVED_READINGS)
        out = self._result(S, out)
        J = self._run_sensitivity(src, layout, normalise, None, available, nan_is_missing, self._scratch("spread", (S, N, K)))
        with torch.cuda.device(self.device):
            _native.check(_native.load().gatres_sensitivity_spread(J.data_ptr(), S * N, K, K, sigma.data_ptr(), out.data_ptr(),
                                                                   _native.current_stream(self.device)),
                          "gatres_sensitivity_spread")
        return out

    def linear_spread(self, readings: torch.Tensor, noise_std, *, available: Optional[torch.Tensor] = None,
                      nan_is_missing: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The FIRST-ORDER spread of the estimates under independent reading errors of standard deviation ``noise_std``
        (physical units; one value or K, as in ``estimate``): ``sqrt(sum_k (J[s, j, k] * noise_std[k])^2)`` per junction, fp32
        ``[S, N_g]`` in physical units (``out``: write it there), from ``sensitivity`` over every junction and one
        ``gatres_sensitivity_spread`` launch.  A missing reading contributes nothing.  As ``sensitivity``, it describes the
        model's prediction at every node, sensor nodes included.

        It is the linearised, noise-free counterpart of ``estimate_ensemble``'s standard deviation: no seed, no sampling error
        (M members carry a relative error of about ``1 / sqrt(2 (M - 1))``), but only the first order -- where the noise carries
        a reading across a kink of the network the two differ.  Cost per snapshot: ``ceil(N_g / batch_size)`` batches of a
        forward AND a backward, against ``ceil(M / batch_size)`` forwards of the ensemble: the ensemble is cheaper whenever
        ``M < N_g``.  The ``[S, N_g, K]`` Jacobian is a scratch kept on the estimator."""
        self._check_readings(readings)
        return self._run_linear_spread(readings, _native.OBSERVED_READINGS, self._normalise, noise_std, available,
                                       nan_is_missing, out)

    def linear_spread_store(self, store, noise_std, *, first: int = 0, count: Optional[int] = None,
                            available: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``linear_spread`` for the snapshots ``[first, first + count)`` of a ``SnapshotStore`` (noise in physical units)."""
        src, _ = self._store_rows(store, first, count)
        return self._run_linear_spread(src, _native.OBSERVED_FULL_ROWS, _native.NORMALISE_NONE, noise_std, available, False, out)

    # ---- screening: a reading that is present and wrong ---------------------------------------------------------------------------
    def _loo_ready(self) -> int:
        K = len(self.observed_idx)
        if K < 2:
            raise ValueError(f"leave-one-out residuals need at least two sensors; the estimator has {K}")
        if self._loo_layouts is None:                               # (built once per estimator)
            self._loo_layouts = torch.from_numpy(loo_layouts(K)).to(self.device)
        return K

    def _working_available(self, name: str, S: int, available: Optional[torch.Tensor]) -> torch.Tensor:
        """The availability the rounds of a screening or monitoring call take readings out of: the scratch ``name`` (uint8
        ``[S, K]``), set to ``available`` (``None``: every reading is there)."""
        avail = self._scratch(name, (S, len(self.observed_idx)), torch.uint8)
        if available is None:
            avail.fill_(1)
        else:
            avail.copy_(available)
        return avail

    def _run_loo(self, src: torch.Tensor, layout: int, normalise: int, available, nan_is_missing: bool, resid: torch.Tensor,
                 pred: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """The leave-one-out pass over the S * K (snapshot, left-out sensor) pairs of ``src`` into ``resid`` / ``pred``
        (``[S, K]``): per batch ``gatres_stage_observed_layouts`` under the layouts "all ones, zero diagonal", the forward,
        ``gatres_loo_residuals``."""
        S, N, K = int(src.shape[0]), self.nodes_per_graph, len(self.observed_idx)
        lib, flat, stream, check = _native.load(), self._parameters(), _native.current_stream(self.device), _native.check
        stage, residuals, nan = lib.gatres_stage_observed_layouts, lib.gatres_loo_residuals, int(bool(nan_is_missing))
        tail, observed_p, scale, offset = self._staging_tail(normalise), self._observed.data_ptr(), self.scale, self.offset
        src_p, avail_p, layouts_p = src.data_ptr(), _native.ptr(available), self._loo_layouts.data_ptr()
        pred_p, resid_p = pred.data_ptr(), resid.data_ptr()

        def batch(P, first, g, off):
            mask = P.mask.data_ptr()
            check(stage(src_p, layout, S, first, K, N, g, *tail, P.x.data_ptr(), mask, avail_p, nan, layouts_p, stream),
                  "gatres_stage_observed_layouts")
            _enqueue_forward(lib, flat, P, stream)
            check(residuals(P.out.data_ptr(), mask, src_p, layout, S, first, N, g, observed_p, K, scale, offset, avail_p, nan,
                            pred_p, resid_p, stream), "gatres_loo_residuals")

        self._pair_pass(S, K, None, batch)
        return resid, pred

    def loo_residuals(self, readings: torch.Tensor, *, available: Optional[torch.Tensor] = None,
                      nan_is_missing: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
        """Is a reading plausible given the others?  ``(resid, pred)``, fp32 ``[S, K]`` on the device, in physical units:
        ``pred[s, k]`` is the model's prediction at node ``observed_idx[k]`` from every reading of snapshot ``s`` but that one,
        ``resid[s, k] = readings[s, k] - pred[s, k]``.  ``readings``, ``available``, ``nan_is_missing`` as in ``estimate``; a
        reading that is not there has a NaN residual (its ``pred`` is still the prediction from the others).  The numbers are
        those of ``reading_residuals``, bit for bit, from ONE pass over the S * K (snapshot, left-out sensor) pairs, three
        launches per batch -- ``gatres_stage_observed_layouts`` with the layouts "all ones, zero diagonal", the forward,
        ``gatres_loo_residuals``.  No ``[S, N]`` matrix is written, nothing is read back, and the two results are a scratch
        kept on the estimator: nothing is allocated after the first call, and the next call of this method overwrites them
        (``clone()`` what must outlive it).  Needs K >= 2."""
        self._check_readings(readings)
        K, S = self._loo_ready(), int(readings.shape[0])
        if available is not None:
            self._check_available(available, S)
        return self._run_loo(readings, _native.OBSERVED_READINGS, self._normalise, available, nan_is_missing,
                             self._scratch("loo_resid", (S, K)), self._scratch("loo_pred", (S, K)))

    def loo_residuals_store(self, store, *, available: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """``loo_residuals`` for every snapshot of a ``SnapshotStore``: the readings are the store's values at the sensors
        (descaled as ``gatres_estimate_write`` descales), everything else is hidden."""
        self._check_store(store)
        K, S = self._loo_ready(), len(store)
        if available is not None:
            self._check_available(available, S)
        return self._run_loo(store.data, _native.OBSERVED_FULL_ROWS, _native.NORMALISE_NONE, available, False,
                             self._scratch("loo_resid", (S, K)), self._scratch("loo_pred", (S, K)))

    def calibrate_screening(self, store, levels=(0.99,), *, available: Optional[torch.Tensor] = None) -> ScreeningBounds:
        """Split-conformal bounds on the leave-one-out residuals, per sensor, from a held-out ``store`` (not the training
        data): one ``loo_residuals_store`` pass and one ``gatres_node_error_quantiles`` launch on the ``[S, K]`` matrices --
        ``pred`` as the estimates, the store's values at the sensors as the truth, the K sensors as the K "nodes".  For every
        level ``q`` (1 to 8 floats in (0, 1), strictly increasing) and sensor ``k`` the element of rank ``conformal_rank(n_k,
        q)`` of ``|reading - leave-one-out prediction|`` over the ``n_k`` snapshots in which the reading was there
        (``available``: ``[len(store), K]``; a missing reading is left out through that launch's own rule for counted
        entries).  In numpy: ``node_error_bounds(pred, reading, levels, hidden=present)``.  It replaces K ``calibrate_bounds``
        calls with hand-built ``available`` matrices, and gives their values at the sensor nodes.  If a new snapshot is
        exchangeable with the store's and every other reading is present and right, a right reading of sensor ``k`` exceeds
        ``bounds[q, k]`` with probability <= 1 - q.  Nothing is read back."""
        lv = _check_levels(levels)
        _, pred = self.loo_residuals_store(store, available=available)
        S, K, Q = len(store), len(self.observed_idx), len(lv)
        truth = store.data.index_select(1, self._observed).contiguous()          # (scaled: the launch descales it as the pass did)
        sensors = torch.arange(K, dtype=torch.int32, device=self.device)
        missing = None if available is None else (available == 0).to(torch.uint8)  # (counted: unless that entry is non-zero)
        bounds = torch.empty((Q, K), dtype=torch.float32, device=self.device)
        counts = torch.empty((K,), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            _native.check(_native.load().gatres_node_error_quantiles(
                pred.data_ptr(), truth.data_ptr(), S, K, self.scale, self.offset, sensors.data_ptr(), K, _native.ptr(missing),
                (ctypes.c_double * Q)(*lv), Q, bounds.data_ptr(), counts.data_ptr(), _native.current_stream(self.device)),
                "gatres_node_error_quantiles")
        return ScreeningBounds(lv, bounds, counts, self.observed_idx)

    def _check_screening(self, bounds, level, max_reject, min_sensors) -> Tuple[int, int, int]:
        K = len(self.observed_idx)
        if not isinstance(bounds, ScreeningBounds):
            raise ValueError("bounds must be the ScreeningBounds of calibrate_screening")
        if bounds.observed_idx != self.observed_idx:
            raise ValueError(f"the bounds were calibrated for the sensors {bounds.observed_idx}, the estimator's are "
                             f"{self.observed_idx}")
        if bounds.device != self.device:
            raise ValueError(f"the bounds must be on {self.device} (got {bounds.device})")
        for name, v, lo, hi in (("max_reject", max_reject, 1, None), ("min_sensors", min_sensors, 1, K)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo or (hi is not None and v > hi):
                raise ValueError(f"{name} must be an integer in [{lo}, {'...' if hi is None else hi}]; got {v!r}")
        return bounds.level_index(level), int(max_reject), int(min_sensors)

    def screen(self, readings: torch.Tensor, bounds: ScreeningBounds, level=None, *, max_reject: int = 1, min_sensors: int = 1,
               available: Optional[torch.Tensor] = None,
               nan_is_missing: bool = False) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """Which readings are not to be believed?  ``max_reject`` rounds of one ``loo_residuals`` pass under the current
        availability and one ``gatres_screen_reject``: in every snapshot the available sensor whose ``|residual|`` exceeds its
        bound ``bounds[level, k]`` by the largest factor (ties: the first) is taken out, as long as ``min_sensors`` readings
        stay.  ONE rejection per round on purpose: a wrong reading also bends the leave-one-out predictions of its
        neighbours, so the largest standardised residual goes first and the others are judged again without it.  Returns
        ``(available_out [S, K] uint8, rejected [S, max_reject] int32`` (column ``r``: the sensor round ``r`` rejected, -1:
        none), ``resid0 [S, K], flagged0 [S, K] uint8)``; the last two are round 0's residuals and its exceedances (what
        ``reading_residuals`` returns).  All on the device, nothing read back (but the bounds' ``inverse`` the first time they
        are used); the results are a scratch kept on the estimator, overwritten by the next ``screen`` / ``estimate_screened``.

        The bounds are calibrated with every OTHER reading present.  From round 1 on they are applied under an availability
        that a rejection has changed (and, with ``available`` gaps, in round 0 too): the coverage statement of
        ``calibrate_screening`` holds for round 0 of complete readings only; later rounds are a heuristic with the same
        numbers.  A round after a clean round repeats it and rejects nothing: skipping it would need a read-back."""
        self._check_readings(readings)
        K, S = self._loo_ready(), int(readings.shape[0])
        qi, R, min_sensors = self._check_screening(bounds, level, max_reject, min_sensors)
        if available is not None:
            self._check_available(available, S)
        bound, inv = bounds.bounds[qi], bounds.inverse[qi]
        avail = self._working_available("screen_available", S, available)
        rejected = self._scratch("screen_rejected", (S, R), torch.int32)
        resid0, flagged0 = self._scratch("screen_resid0", (S, K)), self._scratch("screen_flagged0", (S, K), torch.uint8)
        later, pred = (self._scratch("screen_resid", (S, K)) if R > 1 else None), self._scratch("screen_pred", (S, K))
        lib = _native.load()
        for rnd in range(R):
            resid = resid0 if rnd == 0 else later
            self._run_loo(readings, _native.OBSERVED_READINGS, self._normalise, avail, nan_is_missing, resid, pred)
            with torch.cuda.device(self.device):
                _native.check(lib.gatres_screen_reject(
                    resid.data_ptr(), bound.data_ptr(), inv.data_ptr(), avail.data_ptr(), S, K, min_sensors, rnd, R,
                    rejected.data_ptr(), flagged0.data_ptr() if rnd == 0 else None, _native.current_stream(self.device)),
                    "gatres_screen_reject")
        return avail, rejected, resid0, flagged0

    def estimate_screened(self, readings: torch.Tensor, bounds: ScreeningBounds, level=None, *,
                          out: Optional[torch.Tensor] = None, max_reject: int = 1, min_sensors: int = 1,
                          available: Optional[torch.Tensor] = None,
                          nan_is_missing: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
        """Readings in; estimates, and which sensors were not believed, out: ``screen`` and then the ordinary three-launch
        ``estimate`` pass with ``available_out``.  Returns ``(est [S, N_g], rejected [S, max_reject] int32)``; ``out`` as in
        ``estimate``.  A rejected sensor's node carries the model's estimate, not its reading, whatever ``keep_observed``
        says about the others.  Nothing is read back."""
        self._check_readings(readings)
        if out is not None:
            self._result(int(readings.shape[0]), out)               # (refused before the pass)
        avail, rejected, _, _ = self.screen(readings, bounds, level, max_reject=max_reject, min_sensors=min_sensors,
                                            available=available, nan_is_missing=nan_is_missing)
        return self.estimate(readings, out, available=avail, nan_is_missing=nan_is_missing), rejected

    def screening_report(self, store, bounds: ScreeningBounds, *, fault_offset, fault_share: float = 0.5, seed: int = 0,
                         max_reject: int = 1, level=None) -> Dict[str, object]:
        """Back-test of the screening over ``store`` with planted faults.  ``fault_draws(seed, S, K, fault_share)`` chooses one
        faulty sensor in a ``fault_share`` of the snapshots (on the host, uploaded once); its reading -- the store's descaled
        value -- is shifted by ``fault_offset`` (physical units; one value or K).  Four passes, one read-back each: the clean
        readings, the faulted readings unscreened, the faulted readings through ``estimate_screened``, and the faulted readings
        with the faulty sensor taken out by hand (the best a screening can do).  Returns ``screening_rates`` of the third
        pass's ``rejected`` (detection, misidentification and the false-rejection rates over faulted and clean snapshots),
        ``nonsensor_mae`` (a dict: ``clean``, ``faulted``, ``screened``, ``oracle``: the MAE over the nodes outside
        ``observed_idx``, as ``error_map`` pools it), ``fault_col`` and ``rejected`` (numpy)."""
        self._check_store(store)
        K, S, N = self._loo_ready(), len(store), self.nodes_per_graph
        self._check_screening(bounds, level, max_reject, 1)
        try:
            shift = np.asarray(fault_offset, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"fault_offset must be a number or a sequence of {K} of them") from None
        if shift.ndim == 0:
            shift = np.full(K, float(shift))
        if shift.shape != (K,) or not np.isfinite(shift).all():
            raise ValueError(f"fault_offset must be a finite number or a sequence of {K} of them, one per sensor")
        fault_col = fault_draws(seed, S, K, fault_share)
        rows = np.nonzero(fault_col >= 0)[0]
        plan = np.zeros((2, S, K), dtype=np.float32)                # [0] the shift of every reading, [1] 1 where it is faulty
        plan[0, rows, fault_col[rows]] = shift[fault_col[rows]].astype(np.float32)
        plan[1, rows, fault_col[rows]] = 1.0
        plan = torch.from_numpy(plan).to(self.device)
        readings = store.descale(store.data.index_select(1, self._observed)).contiguous()
        faulted = (readings + plan[0]).contiguous()
        without = (plan[1] == 0).to(torch.uint8).contiguous()
        est = torch.empty((S, N), dtype=torch.float32, device=self.device)
        mae = {}
        self.estimate(readings, est)
        mae["clean"], _ = self._judged(store, est)
        self.estimate(faulted, est)
        mae["faulted"], _ = self._judged(store, est)
        _, rejected = self.estimate_screened(faulted, bounds, level, out=est, max_reject=max_reject)
        mae["screened"], rej = self._judged(store, est, (rejected,))
        rej = rej.reshape(S, int(max_reject)).copy()
        self.estimate(faulted, est, available=without)
        mae["oracle"], _ = self._judged(store, est)
        return {**screening_rates(rej, fault_col), "nonsensor_mae": mae, "fault_col": fault_col, "rejected": rej}

    # ---- monitoring: a sensor that drifts --------------------------------------------------------------------------------------
    def calibrate_monitor(self, store, *, available: Optional[torch.Tensor] = None) -> MonitorBaseline:
        """The in-control mean and spread of every sensor's leave-one-out residual, from a clean held-out ``store``: one
        ``loo_residuals_store`` pass and one ``gatres_node_error_moments`` launch on the ``[S, K]`` matrices -- ``pred`` as the
        estimates, the store's values at the sensors as the truth, the K sensors as the K "nodes" (with ``available`` gaps:
        ``gatres_node_error_moments_available``, which counts the readings that are there).  ONE read-back, of that ``[K, 8]``
        table; on the host in fp64 ``mu = -sum e / n`` (the table's ``e`` is prediction - reading), ``sigma = sqrt(max(sum e^2
        / n - mu^2, 0))`` and ``inv_sigma = float32(1 / sigma)``: ``monitor_baseline_from_moments``."""
        _, pred = self.loo_residuals_store(store, available=available)
        S, K = len(store), len(self.observed_idx)
        truth = store.data.index_select(1, self._observed).contiguous()          # (scaled: the launch descales it as the pass did)
        sensors = torch.arange(K, dtype=torch.int32, device=self.device)
        missing = None if available is None else (available == 0).to(torch.uint8)  # (counted: unless that entry is non-zero)
        b = monitor_baseline_from_moments(self._error_moments(pred, truth, S, K, sensors, missing).cpu().numpy())
        return MonitorBaseline(b["mu"], b["sigma"], b["counts"], self.observed_idx, device=self.device)

    def _check_monitor(self, baseline, S: int, kappa, threshold, series_length, first_index, max_latch, min_sensors, since,
                       state) -> Tuple[int, int, int, int, int, int, int, int]:
        """``(kappa_q, h_q, E, T, t0, R, min_sensors, since)`` of a monitoring call, or a ``ValueError``."""
        K = len(self.observed_idx)
        if not isinstance(baseline, MonitorBaseline):
            raise ValueError("baseline must be the MonitorBaseline of calibrate_monitor")
        if baseline.observed_idx != self.observed_idx:
            raise ValueError(f"the baseline was calibrated for the sensors {baseline.observed_idx}, the estimator's are "
                             f"{self.observed_idx}")
        if baseline.device != self.device:
            raise ValueError(f"the baseline must be on {self.device} (got {baseline.device})")
        fixed = []
        for name, v in (("kappa", kappa), ("threshold", threshold)):
            try:
                fixed.append(cusum_fixed(v))
            except ValueError:
                raise ValueError(f"{name} must be a number in [0, 32768] (in sigma); got {v!r}") from None
        for name, v, lo, hi in (("max_latch", max_latch, 1, None), ("min_sensors", min_sensors, 1, K),
                                ("first_index", first_index, 0, 2 ** 61 - 1),
                                ("series_length", S if series_length is None else series_length, 1, 2 ** 30 - 1)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo or (hi is not None and v > hi):
                raise ValueError(f"{name} must be an integer in [{lo}, {'...' if hi is None else hi}]; got {v!r}")
        T = S if series_length is None else int(series_length)
        if S % T:
            raise ValueError(f"the {S} snapshots are no whole number of series of series_length {T}")
        if since not in MONITOR_SINCE:
            raise ValueError(f"since must be one of {sorted(MONITOR_SINCE)}; got {since!r}")
        E = S // T
        if state is not None and (not isinstance(state, torch.Tensor) or state.dtype != torch.int64
                                  or tuple(state.shape) != (E, K, _native.CUSUM_STATE) or state.device != self.device
                                  or not state.is_contiguous()):
            raise ValueError(f"state must be int64 contiguous [{E}, {K}, {_native.CUSUM_STATE}] on {self.device}: the state of "
                             "an earlier call's result")
        return fixed[0], fixed[1], E, T, int(first_index), int(max_latch), int(min_sensors), MONITOR_SINCE[since]

    def _run_monitor(self, src: torch.Tensor, layout: int, normalise: int, S: int, baseline, kappa, threshold, series_length,
                     first_index, max_latch, min_sensors, since, available, nan_is_missing: bool, state,
                     paths: bool) -> MonitorResult:
        K = self._loo_ready()
        kq, hq, E, T, t0, R, min_sensors, since = self._check_monitor(baseline, S, kappa, threshold, series_length, first_index,
                                                                      max_latch, min_sensors, since, state)
        if available is not None:
            self._check_available(available, S)
        i64, rec = torch.int64, _native.CUSUM_RECORD
        avail = self._working_available("monitor_available", S, available)
        latched = self._scratch("monitor_latched", (E, R), torch.int32)
        latched_rec = self._scratch("monitor_latched_rec", (E, R, rec), i64)
        records0 = self._scratch("monitor_records0", (E, K, rec), i64)
        later = self._scratch("monitor_records", (E, K, rec), i64) if R > 1 else None
        state_out = self._scratch("monitor_state", (E, K, _native.CUSUM_STATE), i64)
        resid, pred = self._scratch("monitor_resid", (S, K)), self._scratch("monitor_pred", (S, K))
        pos = self._scratch("monitor_stat_pos", (S, K)) if paths else None
        neg = self._scratch("monitor_stat_neg", (S, K)) if paths else None
        state_in = None
        if state is not None:                                       # (every round starts from it; it may be `state_out` itself)
            state_in = self._scratch("monitor_state_in", (E, K, _native.CUSUM_STATE), i64)
            state_in.copy_(state)
        lib = _native.load()
        for rnd in range(R):
            # (round 0 of complete readings is the pass without an availability: the same bits, nothing to load per pair)
            self._run_loo(src, layout, normalise, avail if rnd > 0 or available is not None else None, nan_is_missing, resid, pred)
            records = records0 if rnd == 0 else later
            with torch.cuda.device(self.device):
                stream = _native.current_stream(self.device)
                _native.check(lib.gatres_cusum_scan(
                    resid.data_ptr(), baseline.mu.data_ptr(), baseline.inv_sigma.data_ptr(), avail.data_ptr(), S, K, T, t0, kq, hq,
                    _native.ptr(state_in), state_out.data_ptr(), records.data_ptr(), _native.ptr(pos if rnd == 0 else None),
                    _native.ptr(neg if rnd == 0 else None), stream), "gatres_cusum_scan")
                _native.check(lib.gatres_monitor_latch(
                    records.data_ptr(), avail.data_ptr(), S, K, T, t0, since, min_sensors, rnd, R, latched.data_ptr(),
                    latched_rec.data_ptr(), stream), "gatres_monitor_latch")
        return MonitorResult(avail, latched, latched_rec, records0, state_out, pos, neg)

    def monitor(self, readings: torch.Tensor, baseline: MonitorBaseline, *, kappa: float = 0.5, threshold: float = 5.0,
                series_length: Optional[int] = None, first_index: int = 0, max_latch: int = 1, min_sensors: int = 1,
                since: str = "onset", available: Optional[torch.Tensor] = None, nan_is_missing: bool = False,
                state: Optional[torch.Tensor] = None, paths: bool = False) -> MonitorResult:
        """Which sensor has been drifting, and since when?  The S rows of ``readings`` are a TIME SERIES here (``series_length``:
        E = S / series_length independent series of consecutive rows; ``None``: one).  ``max_latch`` rounds of one leave-one-out
        pass under the current availability, one ``gatres_cusum_scan`` and one ``gatres_monitor_latch``: per sensor a two-sided
        CUSUM of the standardised residual ``z = (resid - mu) / sigma`` with allowance ``kappa`` and threshold ``threshold``
        (both in sigma), ``P = max(0, P + z - kappa)``, ``M = max(0, M - z - kappa)``, in int64 fixed point (2^-16 sigma), so
        the result is a function of the inputs alone; an entry that is missing, NaN or of a sensor without a spread is not
        counted and holds the state.  The first step with ``P`` or ``M`` above the threshold is the sensor's alarm, the step
        after the statistic's last zero before it the estimated onset.  Per series and round the sensor that alarmed first
        (ties: the larger statistic, then the first) is LATCHED: taken out of the availability from its onset on
        (``since="alarm"``: from the alarm on), as long as ``min_sensors`` sensors stay.  ONE latch per round, for the reason
        ``screen`` gives: a drifting sensor bends its neighbours' leave-one-out predictions, so they are judged again without
        it.  A round after a clean round repeats it and latches nothing: skipping it would need a read-back.

        Readings that arrive in chunks: pass ``state=previous.state`` and ``first_index=`` the number of rows seen so far; the
        paths, the final state, the first alarm and its onset are those of one call over all rows (a record's ``n`` and
        ``sum q`` count this call's rows only).  Every round starts from ``state``; nothing is reset after an alarm.

        Returns a ``MonitorResult``: all on the device, nothing is read back, and the tensors are a scratch kept on the
        estimator -- nothing is allocated after the first call, the next ``monitor`` / ``estimate_monitored`` overwrites them.
        ``paths=True`` adds round 0's ``stat_pos`` / ``stat_neg``.

        What the numbers mean: with independent standard-normal ``z``, ``kappa=0.5`` and ``threshold=5`` give the textbook
        two-sided in-control run length of about 465 counted readings.  What they do not: real leave-one-out residuals are
        autocorrelated in time, so the defaults are a starting point; the clean-series false-alarm rate of
        ``monitoring_report`` on a held-out store of one's own is the number to tune against.  No coverage statement is made."""
        self._check_readings(readings)
        return self._run_monitor(readings, _native.OBSERVED_READINGS, self._normalise, int(readings.shape[0]), baseline, kappa,
                                 threshold, series_length, first_index, max_latch, min_sensors, since, available, nan_is_missing,
                                 state, paths)

    def monitor_store(self, store, baseline: MonitorBaseline, *, kappa: float = 0.5, threshold: float = 5.0,
                      series_length: Optional[int] = None, first_index: int = 0, max_latch: int = 1, min_sensors: int = 1,
                      since: str = "onset", available: Optional[torch.Tensor] = None, state: Optional[torch.Tensor] = None,
                      paths: bool = False) -> MonitorResult:
        """``monitor`` over the snapshots of a ``SnapshotStore`` in their order: the readings are the store's values at the
        sensors, as in ``loo_residuals_store``."""
        self._check_store(store)
        return self._run_monitor(store.data, _native.OBSERVED_FULL_ROWS, _native.NORMALISE_NONE, len(store), baseline, kappa,
                                 threshold, series_length, first_index, max_latch, min_sensors, since, available, False, state,
                                 paths)

    def estimate_monitored(self, readings: torch.Tensor, baseline: MonitorBaseline, *, out: Optional[torch.Tensor] = None,
                           nan_is_missing: bool = False, **kw) -> Tuple[torch.Tensor, MonitorResult]:
        """Readings in; estimates, and which sensors were latched as drifting, out: ``monitor`` (its keywords) and then the
        ordinary three-launch ``estimate`` pass with ``available_out``.  Returns ``(est [S, N_g], result)``; ``out`` as in
        ``estimate``.  A latched sensor's node carries the model's estimate from its onset on.  Nothing is read back."""
        self._check_readings(readings)
        if out is not None:
            self._result(int(readings.shape[0]), out)               # (refused before the pass)
        result = self.monitor(readings, baseline, nan_is_missing=nan_is_missing, **kw)
        return self.estimate(readings, out, available=result.available_out, nan_is_missing=nan_is_missing), result

    def monitoring_report(self, store, baseline: MonitorBaseline, *, series_length: int, drift_rate, drift_share: float = 0.5,
                          min_lead: Optional[int] = None, seed: int = 0, kappa: float = 0.5, threshold: float = 5.0,
                          max_latch: int = 1, min_sensors: int = 1, since: str = "onset") -> Dict[str, object]:
        """Back-test of the monitor over ``store``, read as series of ``series_length`` snapshots, with planted drifts.
        ``drift_draws(seed, E, T, K, drift_share, min_lead)`` chooses one drifting sensor and one onset in ``[min_lead, T -
        min_lead)`` (default ``T // 4``) in a ``drift_share`` of the series; ``drift_offsets`` adds the ramp ``drift_rate[k] *
        (t - onset + 1)`` (physical units per step; one value or K) to the store's descaled readings (host, uploaded once).
        Four passes, one read-back each: the clean readings, the drifted readings unmonitored, the drifted readings through
        ``estimate_monitored``, and the drifted readings with the drifting sensor taken out by hand from its true onset (the
        best a monitor can do).  Returns ``monitoring_rates`` of the third pass (detection, misidentification, the
        false-alarm rate on clean series, detection delays, the onset error), ``nonsensor_mae`` (a dict: ``clean``,
        ``drifted``, ``monitored``, ``oracle``: the MAE over the nodes outside ``observed_idx``, as ``error_map`` pools it),
        ``draws``, ``latched`` and ``latched_rec`` (numpy)."""
        self._check_store(store)
        K, S, N = self._loo_ready(), len(store), self.nodes_per_graph
        _, _, E, T, _, R, _, _ = self._check_monitor(baseline, S, kappa, threshold, series_length, 0, max_latch, min_sensors,
                                                     since, None)
        draws = drift_draws(seed, E, T, K, drift_share, T // 4 if min_lead is None else min_lead)
        offsets = drift_offsets(draws, T, K, drift_rate)
        without = np.ones((S, K), dtype=np.uint8)
        for e, (k, onset) in enumerate(draws.tolist()):
            if k >= 0:
                without[e * T + onset:(e + 1) * T, k] = 0
        readings = store.descale(store.data.index_select(1, self._observed)).contiguous()
        drifted = (readings + torch.from_numpy(offsets).to(self.device)).contiguous()
        without = torch.from_numpy(without).to(self.device)
        est = torch.empty((S, N), dtype=torch.float32, device=self.device)
        mae = {}
        self.estimate(readings, est)
        mae["clean"], _ = self._judged(store, est)
        self.estimate(drifted, est)
        mae["drifted"], _ = self._judged(store, est)
        _, res = self.estimate_monitored(drifted, baseline, out=est, kappa=kappa, threshold=threshold, series_length=T,
                                         max_latch=max_latch, min_sensors=min_sensors, since=since)
        mae["monitored"], ints = self._judged(store, est, (res.latched, res.latched_rec))
        latched = ints[:E * R].reshape(E, R).copy()
        latched_rec = ints[E * R:].reshape(E, R, _native.CUSUM_RECORD).copy()
        self.estimate(drifted, est, available=without)
        mae["oracle"], _ = self._judged(store, est)
        return {**monitoring_rates(latched_rec, latched, draws), "nonsensor_mae": mae, "draws": draws, "latched": latched,
                "latched_rec": latched_rec}


class SensitivityMap:
    """The folded sensitivities of a sensor layout over ``num_snapshots`` snapshots: ``table`` fp64 ``[T, K,
    SENSITIVITY_RECORD]`` on the device (per junction ``targets[t]`` and sensor ``observed_idx[k]``: the entries that are not 0,
    sum J, sum \\|J\\|, sum J^2, max \\|J\\|).  ``influence_from_table`` / ``PressureEstimator.influence_report`` read it."""

    def __init__(self, table: torch.Tensor, targets, observed_idx, num_snapshots: int):
        self.targets = [int(v) for v in targets]
        self.observed_idx = [int(v) for v in observed_idx]
        self.num_snapshots = int(num_snapshots)
        if (not isinstance(table, torch.Tensor) or table.dtype != torch.float64
                or tuple(table.shape) != (len(self.targets), len(self.observed_idx), SENSITIVITY_RECORD)):
            raise ValueError(f"table must be fp64 [{len(self.targets)}, {len(self.observed_idx)}, {SENSITIVITY_RECORD}]")
        if self.num_snapshots < 1:
            raise ValueError("num_snapshots must be positive")
        self.table = table

    @property
    def device(self) -> torch.device:
        return self.table.device

    def state_dict(self) -> Dict[str, object]:
        """Plain values and a CPU tensor, for ``torch.save``."""
        return {"table": self.table.detach().cpu(), "targets": list(self.targets), "observed_idx": list(self.observed_idx),
                "num_snapshots": self.num_snapshots}

    @classmethod
    def from_state_dict(cls, d, device=None) -> "SensitivityMap":
        table = torch.as_tensor(d["table"], dtype=torch.float64)
        return cls(table if device is None else table.to(device), d["targets"], d["observed_idx"], d["num_snapshots"])
