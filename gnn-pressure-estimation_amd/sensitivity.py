"""The sensitivity pass of ``estimation.PressureEstimator`` restated on the host, in numpy, without a device: the seeds of
``gatres_stage_observed_targets``, the three launches of csrc/k_sensitivity.hip (include/gatres.h states them) and the report
``influence_report`` makes of a folded table.  fp32 values are formed with one rounding per operation, as the kernels form them;
the fp64 sums run in the kernels' order, as Python loops over the axis the kernels fix (snapshots in the fold, sensors in the
spread)."""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np

SENSITIVITY_RECORD = 5          # GATRES_SENSITIVITY_RECORD: [#nonzero, sum J, sum |J|, sum J^2, max |J|]


def sensitivity_seeds(first_pair: int, num_graphs: int, nodes_per_graph: int, num_targets: int,
                      targets: Optional[Sequence[int]] = None) -> np.ndarray:
    """``g_out`` of ``gatres_stage_observed_targets``: fp32 ``[num_graphs, N]``, graph ``g`` is pair ``p = first_pair + g`` and
    carries 1.0 at the node of target ``p % T`` (``targets[p % T]``; ``targets=None``: node ``p % T``), 0.0 elsewhere.  A
    target outside ``[0, N)`` seeds nothing."""
    G, N, T = int(num_graphs), int(nodes_per_graph), int(num_targets)
    if G < 1 or N < 1 or T < 1 or int(first_pair) < 0:
        raise ValueError("sensitivity_seeds needs num_graphs, nodes_per_graph, num_targets >= 1 and first_pair >= 0")
    if targets is None:
        if T > N:
            raise ValueError(f"without targets, target t is node t: num_targets={T} exceeds the {N} nodes")
        nodes = np.arange(T, dtype=np.int64)
    else:
        nodes = np.asarray(list(targets), dtype=np.int64)
        if nodes.shape != (T,):
            raise ValueError(f"targets must hold num_targets={T} node indices")
    t = (int(first_pair) + np.arange(G, dtype=np.int64)) % T
    return (np.arange(N, dtype=np.int64)[None, :] == nodes[t][:, None]).astype(np.float32)


def sensitivity_rows_from_gx(g_x, mask, observed: Sequence[int], unit: float, fault=None) -> np.ndarray:
    """``gatres_sensitivity_gather``: ``g_x`` fp32 and ``mask`` uint8 ``[G, N]``; returns fp32 ``[G, K]`` with entry ``[g, k]``
    exactly 0 where ``mask[g, observed[k]] != 0`` and ``fp32(g_x[g, observed[k]] * fp32(unit))`` elsewhere; all NaN when
    ``fault`` is a NaN."""
    g_x = np.asarray(g_x, dtype=np.float32)
    mask = np.asarray(mask)
    obs = np.asarray(list(observed), dtype=np.int64)
    if g_x.ndim != 2 or mask.shape != g_x.shape:
        raise ValueError("g_x and mask must be [G, N]")
    with np.errstate(invalid="ignore", over="ignore"):
        rows = (g_x[:, obs] * np.float32(unit)).astype(np.float32)
    rows = np.where(mask[:, obs] != 0, np.float32(0.0), rows).astype(np.float32)
    if fault is not None and np.isnan(np.float32(fault)):
        rows[:] = np.nan
    return rows


def sensitivity_fold_ref(J, table=None) -> np.ndarray:
    """``gatres_sensitivity_fold``: ``J`` fp32 ``[S, T, K]``; returns fp64 ``[T, K, SENSITIVITY_RECORD]``, per (target, sensor)
    strictly in snapshot order: [0] the entries that are not exactly 0, [1] sum J, [2] sum \\|J\\|, [3] sum J^2, [4] max \\|J\\|
    (``fmax``: a NaN is ignored there).  ``table``: continue from it (``accumulate``), so a fold in chunks equals one fold."""
    J = np.asarray(J, dtype=np.float32)
    if J.ndim != 3:
        raise ValueError("J must be [S, T, K]")
    S, T, K = J.shape
    t = np.zeros((T, K, SENSITIVITY_RECORD), dtype=np.float64) if table is None else np.array(table, dtype=np.float64, copy=True)
    if t.shape != (T, K, SENSITIVITY_RECORD):
        raise ValueError(f"table must be [{T}, {K}, {SENSITIVITY_RECORD}]")
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(S):
            j = J[s].astype(np.float64)
            t[:, :, 0] = t[:, :, 0] + (J[s] != 0)
            t[:, :, 1] = t[:, :, 1] + j
            t[:, :, 2] = t[:, :, 2] + np.abs(j)
            t[:, :, 3] = t[:, :, 3] + j * j
            t[:, :, 4] = np.fmax(t[:, :, 4], np.abs(j))
    return t


def linear_spread_ref(J, sigma) -> np.ndarray:
    """``gatres_sensitivity_spread``: ``J`` fp32 ``[..., K]``, ``sigma`` fp32 ``[K]``; returns fp32 ``[...]``,
    ``(float)sqrt(sum_k ((double)J[..., k] * (double)sigma[k])^2)`` summed in sensor order in fp64."""
    J = np.asarray(J, dtype=np.float32)
    sigma = np.asarray(sigma, dtype=np.float32)
    if sigma.shape != (J.shape[-1],):
        raise ValueError("sigma must hold one value per column of J")
    acc = np.zeros(J.shape[:-1], dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(J.shape[-1]):
            p = J[..., k].astype(np.float64) * np.float64(sigma[k])
            acc = acc + p * p
        return np.sqrt(acc).astype(np.float32)


def influence_from_table(table, targets: Sequence[int], observed_idx: Sequence[int], num_snapshots: int) -> Dict[str, object]:
    """The influence report of a folded table ``[T, K, SENSITIVITY_RECORD]`` over ``num_snapshots`` snapshots, in fp64; row ``t``
    is the junction ``targets[t]``, column ``k`` the sensor at ``observed_idx[k]``.  The means run over ALL snapshots: a reading
    that was missing in a snapshot has sensitivity 0 there.

    Per (junction, sensor) ``[T, K]``: ``mean`` (of J), ``mean_abs`` (of \\|J\\|), ``rms``, ``max_abs`` and ``nonzero`` (the
    snapshots with J != 0).  Per junction ``[T]``, with ``a = mean_abs[t]``: ``dominant_sensor`` (the column of the largest
    ``a``, the first on a tie; -1 where every ``a`` is 0), ``dominant_share`` = ``a.max() / a.sum()`` and ``participation`` =
    ``a.sum()**2 / (a**2).sum()``, the effective number of sensors the estimate rests on (1: a single sensor; K: all alike);
    both NaN where every ``a`` is 0.  Per sensor ``[K]``: ``sensor_total`` = ``sum_t mean_abs``, ``sensor_dominates`` (the
    junctions it dominates) and ``self_entry`` = ``mean[t, k]`` at ``targets[t] == observed_idx[k]``, how far the model's own
    prediction at the sensor's node follows that sensor (NaN where the node is no target).  ``targets``, ``observed_idx`` and
    ``num_snapshots`` are returned beside them."""
    tgt = [int(v) for v in targets]
    obs = [int(v) for v in observed_idx]
    S = int(num_snapshots)
    if S < 1:
        raise ValueError("num_snapshots must be positive")
    t = np.asarray(table, dtype=np.float64)
    if t.shape != (len(tgt), len(obs), SENSITIVITY_RECORD):
        raise ValueError(f"table must be [{len(tgt)}, {len(obs)}, {SENSITIVITY_RECORD}]; got {tuple(t.shape)}")
    mean, mean_abs, rms = t[:, :, 1] / S, t[:, :, 2] / S, np.sqrt(t[:, :, 3] / S)
    total = mean_abs.sum(axis=1)
    some = total > 0
    safe = np.where(some, total, 1.0)
    sq = np.where(some, (mean_abs * mean_abs).sum(axis=1), 1.0)
    dominant = np.where(some, mean_abs.argmax(axis=1), -1)
    self_entry = np.full(len(obs), np.nan)
    where = {}
    for i, v in enumerate(tgt):
        where.setdefault(v, i)
    for k, v in enumerate(obs):
        if v in where:
            self_entry[k] = mean[where[v], k]
    return {"mean": mean, "mean_abs": mean_abs, "rms": rms, "max_abs": t[:, :, 4].copy(), "nonzero": t[:, :, 0].copy(),
            "dominant_sensor": dominant, "dominant_share": np.where(some, mean_abs.max(axis=1) / safe, np.nan),
            "participation": np.where(some, total * total / sq, np.nan),
            "sensor_total": mean_abs.sum(axis=0), "sensor_dominates": np.bincount(dominant[some], minlength=len(obs)),
            "self_entry": self_entry, "targets": tgt, "observed_idx": obs, "num_snapshots": S}
