"""Pressure estimation with a fixed sensor set: the task ``GATResMeanConv`` is trained for -- the readings of the sensors in, the
pressure at every junction out -- as a device pass, for deployment and for back-testing a sensor layout over a snapshot store.

The reference has no such entry point: a caller writes ``test_one_epoch``'s loop body by hand (evaluation.py:298-330: ``x1`` built
with an index assignment, ``model(x1, edge_index)``, a boolean gather, ``descale`` with torch ops, batch by batch).  Here a pass is
three launches per batch on the current stream -- ``gatres_stage_observed`` (zeros and mask = 1 everywhere but at the sensors),
``gatres_model_forward`` in inference form with that mask, ``gatres_estimate_write`` (descaled into the pass's result matrix) --
with the plans and the forward's call state of ``evaluation.evaluate_store``.  Nothing is read back and nothing synchronises: the
result is a device tensor, ordered on the stream.  ``error_map`` is the back-test report: one ``gatres_node_error_moments`` launch
and one read-back.

Telemetry has gaps.  With ``available`` (uint8 / bool ``[S, K]`` on the device) or ``nan_is_missing`` the staging launch is
``gatres_stage_observed_available``: a sensor without a reading in a snapshot is one more hidden node there (``x = 0``,
``mask = 1``), which is what the model's training masks taught it.  Still three launches per batch, still nothing read back: no
host scan for NaN.  ``error_map(available=...)`` reports over the hidden entries, ``sensor_failure_report`` is the leave-one-out
back-test of a sensor layout (what does the loss of sensor k cost?) as K + 1 passes of one estimator.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _native
from .evaluation import _enqueue_forward, _eval_plan
from .snapshot_store import SnapshotStore

NODE_ERROR_RECORD = _native.NODE_ERROR_RECORD
NODE_ERROR_AVAIL_RECORD = _native.NODE_ERROR_AVAIL_RECORD


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
        self._normalise = _native.NORMALISE_NONE
        if norm_type == "znorm":
            self._normalise = _native.NORMALISE_RECIPROCAL if _divides_by_reciprocal(dev) else _native.NORMALISE_DIVIDE
        self._observed = torch.tensor(self.observed_idx, dtype=torch.int32).to(dev)

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

    def _result(self, S: int, out: Optional[torch.Tensor]) -> torch.Tensor:
        if out is None:
            return torch.empty((S, self.nodes_per_graph), dtype=torch.float32, device=self.device)
        if (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.device != self.device
                or tuple(out.shape) != (S, self.nodes_per_graph) or not out.is_contiguous()):
            raise ValueError(f"out must be fp32 contiguous [{S}, {self.nodes_per_graph}] on {self.device}")
        return out

    def _check_available(self, available, S: int) -> None:
        K = len(self.observed_idx)
        if (not isinstance(available, torch.Tensor) or available.dtype not in (torch.uint8, torch.bool)
                or tuple(available.shape) != (S, K) or available.device != self.device or not available.is_contiguous()):
            raise ValueError(f"available must be uint8 or bool, contiguous [{S}, {K}] on {self.device}")

    def _run(self, src: torch.Tensor, layout: int, normalise: int, out: Optional[torch.Tensor],
             available: Optional[torch.Tensor] = None, nan_is_missing: bool = False) -> torch.Tensor:
        model, N, S = self.model, self.nodes_per_graph, int(src.shape[0])
        if available is not None:
            self._check_available(available, S)
        with_gaps = available is not None or bool(nan_is_missing)
        out = self._result(S, out)
        model.eval()
        flat = model.flat_parameters
        if flat.device != self.device:
            raise ValueError(f"the model moved to {flat.device}; the estimator was built on {self.device}")
        lib = _native.load()
        factor = self.std + self.eps if self.norm_type == "znorm" else 1.0
        with torch.cuda.device(self.device):
            stream = _native.current_stream(self.device)
            sizes = [min(self.batch_size, S - first) for first in range(0, S, self.batch_size)]
            plans = {g: _eval_plan(model, self._topo, g) for g in sorted(set(sizes))}
            for b, g in enumerate(sizes):
                P, first = plans[g], b * self.batch_size
                if with_gaps:
                    _native.check(lib.gatres_stage_observed_available(
                        src.data_ptr(), layout, S, None, first, N, g, self._observed.data_ptr(), len(self.observed_idx),
                        normalise, self.offset, factor, P.x.data_ptr(), P.mask.data_ptr(), _native.ptr(available),
                        int(bool(nan_is_missing)), stream), "gatres_stage_observed_available")
                else:
                    _native.check(lib.gatres_stage_observed(
                        src.data_ptr(), layout, S, None, first, N, g, self._observed.data_ptr(), len(self.observed_idx),
                        normalise, self.offset, factor, P.x.data_ptr(), P.mask.data_ptr(), stream), "gatres_stage_observed")
                _enqueue_forward(lib, flat, P, stream)
                _native.check(lib.gatres_estimate_write(
                    P.out.data_ptr(), P.x.data_ptr(), P.mask.data_ptr(), N, g, self.scale, self.offset, int(self.keep_observed),
                    out.data_ptr(), S, N, first, stream), "gatres_estimate_write")
        return out

    def estimate(self, readings: torch.Tensor, out: Optional[torch.Tensor] = None, *,
                 available: Optional[torch.Tensor] = None, nan_is_missing: bool = False) -> torch.Tensor:
        """``readings``: fp32 contiguous ``[S, K]`` on the model's device, in physical units, column ``k`` the sensor at
        ``observed_idx[k]``.  Returns the pressures ``[S, N_g]`` in physical units (``out``: write them there), a device tensor
        ordered on the current stream.

        ``available``: uint8 or bool contiguous ``[S, K]`` on the same device, non-zero where the reading is present;
        ``nan_is_missing``: a NaN reading is missing (decided on the device: nothing is scanned on the host).  A missing reading
        is not used: its node is hidden in that snapshot and, with ``keep_observed``, carries the model's prediction.  A
        snapshot without any reading is legal (the model's output on an all-zero input)."""
        K = len(self.observed_idx)
        if (not isinstance(readings, torch.Tensor) or readings.dtype != torch.float32 or readings.dim() != 2
                or readings.shape[1] != K or readings.shape[0] == 0 or readings.device != self.device
                or not readings.is_contiguous()):
            raise ValueError(f"readings must be fp32 contiguous [S, {K}] on {self.device}")
        return self._run(readings, _native.OBSERVED_READINGS, self._normalise, out, available, nan_is_missing)

    def estimate_store(self, store, out: Optional[torch.Tensor] = None, *,
                       available: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The same for every snapshot of a ``SnapshotStore``, in store order, with everything but the sensors hidden --
        and, with ``available`` (``[len(store), K]``), the sensors without a reading too."""
        self._check_store(store)
        return self._run(store.data, _native.OBSERVED_FULL_ROWS, _native.NORMALISE_NONE, out, available)

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
        lib = _native.load()
        with torch.cuda.device(self.device):
            stream = _native.current_stream(self.device)
            if available is None:
                table = torch.empty((self.nodes_per_graph, NODE_ERROR_RECORD), dtype=torch.float64, device=self.device)
                _native.check(lib.gatres_node_error_moments(
                    est.data_ptr(), store.data.data_ptr(), len(store), self.nodes_per_graph, self.scale, self.offset,
                    self._observed.data_ptr(), len(self.observed_idx), table.data_ptr(), stream), "gatres_node_error_moments")
            else:
                table = torch.empty((self.nodes_per_graph, NODE_ERROR_AVAIL_RECORD), dtype=torch.float64, device=self.device)
                _native.check(lib.gatres_node_error_moments_available(
                    est.data_ptr(), store.data.data_ptr(), len(store), self.nodes_per_graph, self.scale, self.offset,
                    self._observed.data_ptr(), len(self.observed_idx), available.data_ptr(), table.data_ptr(), stream),
                    "gatres_node_error_moments_available")
        if available is None:
            return error_map_from_moments(table.cpu().numpy())
        return error_map_from_moments(table.cpu().numpy(), available=True, observed_idx=self.observed_idx)

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
