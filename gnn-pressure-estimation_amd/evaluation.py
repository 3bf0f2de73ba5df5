"""Evaluation path for GATRes: forward-only passes under fresh masks, the reference's seven metrics on de-normalised
masked predictions, and event-timed latency / throughput.

Mirrors gnn_pressure_estimation/evaluation.py:240-351 (``test_one_epoch``: the all-nodes pass and the sensor pass, whose
masks always contain ``required_idx``) and :355-403 (the trial loop that runs both passes per trial) for the configuration
the GATRes models run with (``use_data_batch=False``, no edge attributes), utils/auxil.py:101-140,185-203 (metric functions
and their registry) and utils/timer.py:12-66 (``Timer``: warm-up, then one event pair per inference call).  The sensor
indices themselves come from a secrets file the reference does not ship (evaluation.py:27-66: without it ``get_sensors``
returns empty lists and the second pass equals the first); here they are an argument.
The model call is the fused forward kernel (no activations kept under ``torch.no_grad()``); everything else in
``test_one_epoch`` is caller-side tensor arithmetic, exactly as in the reference.

``evaluate_store`` is the same epoch on the device for a ``SnapshotStore``: per batch one staging launch (collation + a mask
that holds the sensor nodes on the sensor pass), the forward, and one launch that writes the batch's masked-metric moments
(``gatres_masked_metrics``) into a device table; one synchronisation and one read-back per epoch, then
``metrics_from_moments`` forms the loss and the seven metrics on the host in fp64.
"""
from __future__ import annotations

import weakref
from functools import partial
from typing import Callable, Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from .wdn_synth import generate_batch_mask


# ---- metrics (auxil.py:101-140) -----------------------------------------------------------------------------------
def calculate_nse(y_pred, y_true, exponent=2):
    p, t = y_pred.reshape(-1), y_true.reshape(-1)
    return 1.0 - (p - t).pow(exponent).sum() / ((t - t.mean()).pow(exponent).sum() + 1e-12)


def calculate_rmse(y_pred, y_true):
    return ((y_pred - y_true) ** 2).mean().sqrt()


def calculate_rel_error(y_pred, y_true):
    keep = y_true.abs() > 0.01
    return ((y_true - y_pred).abs()[keep] / y_true[keep]).abs().mean()


def calculate_accuracy(y_pred, y_true, threshold=0.2):
    return ((y_true - y_pred).abs() <= y_true * threshold).float().mean()


def calculate_correlation_coefficient(y_pred, y_true):
    vx, vy = y_pred - y_pred.mean(), y_true - y_true.mean()
    return ((vx * vy).sum() / (vx.pow(2).sum().sqrt() * vy.pow(2).sum().sqrt())).clamp(-1.0, 1.0)


def calculate_r2(y_pred, y_true):
    return calculate_correlation_coefficient(y_pred, y_true) ** 2


# ---- training criteria (train.py:354-368, --criterion {mse,mae,sce}) ---------------------------------------------------
def sce_loss(x: torch.Tensor, y: torch.Tensor, alpha: int = 3) -> torch.Tensor:
    """The reference's scaled cosine error: ``mean((1 - <x^, y^>)^alpha)`` with ``x^``, ``y^`` the rows of ``x``, ``y``
    L2-normalised along the last dimension (``F.normalize``, eps 1e-12).  On the masked predictions of a GATRes model
    (``[M, 1]``) ``x^`` is +-1 wherever ``|x| >= 1e-12``, so the loss is flat there: its gradient is zero (in exact
    arithmetic; torch's fp32 autograd returns rounding noise) and training with it moves the parameters by weight decay only.
    ``GATResTrainer(criterion="sce")`` computes the exact value (gatres.h: GATRES_LOSS_SCE)."""
    xn = F.normalize(x, p=2, dim=-1)
    yn = F.normalize(y, p=2, dim=-1)
    return torch.pow(1.0 - torch.sum(xn * yn, dim=-1), alpha).mean()


CRITERIA = ("mse", "mae", "sce")


def get_criterion(name: str) -> Callable:
    """The callable ``train.py --criterion name`` trains and validates with: ``nn.MSELoss()``, ``nn.L1Loss()`` or
    ``sce_loss``.  ``test_one_epoch(criterion=get_criterion(name))`` gives the reference's validation loss."""
    if name == "mse":
        return torch.nn.MSELoss(reduction="mean")
    if name == "mae":
        return torch.nn.L1Loss(reduction="mean")
    if name == "sce":
        return sce_loss
    raise KeyError(f"criterion {name} is not supported (choices: {', '.join(CRITERIA)})")


def get_metric_fn_collection(prefix: str) -> Dict[str, Callable]:
    """auxil.py:185-203: same keys, same order."""
    return {f"{prefix}_error": calculate_rel_error, f"{prefix}_0.1": partial(calculate_accuracy, threshold=0.1),
            f"{prefix}_corr": calculate_correlation_coefficient, f"{prefix}_r2": calculate_r2,
            f"{prefix}_mae": F.l1_loss, f"{prefix}_rmse": calculate_rmse,
            f"{prefix}_mynse": partial(calculate_nse, exponent=2)}


def descale(scaled_data, norm_type="minmax", mean=None, std=None, min=None, max=None):
    """auxil.py:42-64."""
    if norm_type == "minmax":
        return scaled_data * (max - min) + min
    if norm_type == "znorm":
        return scaled_data * std + mean
    return scaled_data


# ---- gradient flow (auxil.py:295-313) -----------------------------------------------------------------------------------
GRAD_FLOW_WORDS = ("block", "mlp", "res")


def gradient_flow_names(model: torch.nn.Module) -> List[str]:
    """The parameters ``get_gradient_norm`` reports, in ``named_parameters()`` order: those whose name contains ``block``,
    ``mlp`` or ``res``.  For ``GATResMeanConv`` that is every parameter of ``blocks`` (``blocks.0.conv1.att_src``, ...): eight
    per block, without ``lin0`` / ``lin1``."""
    return [n for n, _ in model.named_parameters() if any(w in n for w in GRAD_FLOW_WORDS)]


def get_gradient_norm(model: torch.nn.Module, norm_type=2) -> Tuple[torch.Tensor, List[torch.Tensor], List[str]]:
    """The reference's per-epoch gradient report on the host, for a module trained through ``loss.backward()``:
    ``(total_norm, block_norms, block_names)`` -- the ``norm_type`` norm of ``p.grad`` for every parameter of
    ``gradient_flow_names(model)`` and the norm of those norms.  Plain torch ops on whatever device the gradients are on.
    ``GATResTrainer.gradient_flow()`` is the same report for the native step, computed by one launch."""
    names = gradient_flow_names(model)
    params = dict(model.named_parameters())
    missing = [n for n in names if params[n].grad is None]
    if missing:
        raise ValueError(f"no gradient on {missing[0]} (and {len(missing) - 1} more): call loss.backward() first")
    if not names:
        raise ValueError("the model has no parameter whose name contains " + ", ".join(GRAD_FLOW_WORDS))
    block_norms = [torch.norm(params[n].grad.detach(), p=norm_type) for n in names]
    return torch.norm(torch.stack(block_norms), norm_type), block_norms, names


# ---- timing (timer.py:12-66) --------------------------------------------------------------------------------------
class Timer:
    """One HIP event pair per inference call after ``gpu_warmup_times`` untimed calls (timer.py:22-41)."""

    def __init__(self) -> None:
        self.reset()

    def reset(self) -> None:
        self.timings, self.num_graphs, self.finished_warmup = [], [], False

    def auto_measure(self, inference_func: Callable, num_graphs_per_batch: int, gpu_warmup_times: int = 10) -> Callable:
        def inference(*args, **kwargs):
            if gpu_warmup_times > 0 and not self.finished_warmup:
                for _ in range(gpu_warmup_times):
                    inference_func(*args, **kwargs)
                self.finished_warmup = True
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            out = inference_func(*args, **kwargs)
            end.record()
            torch.cuda.synchronize()
            self.timings.append(start.elapsed_time(end))
            self.num_graphs.append(num_graphs_per_batch)
            return out
        return inference

    def compute_time(self, len_dataset: int) -> float:
        """mean milliseconds per graph, timer.py:43-51 (batch time weighted by its graph count)."""
        return float(np.dot(np.array(self.timings), np.array(self.num_graphs)) / len_dataset)

    def compute_throughput(self, len_dataset: int) -> float:
        """graphs per second as the reference defines it, timer.py:53-66."""
        total_s = float(np.sum(np.array(self.timings) * np.array(self.num_graphs) / len_dataset / 1000.0))
        return float(len(self.timings) * max(self.num_graphs)) / total_s


# ---- the loop (evaluation.py:240-351) -----------------------------------------------------------------------------
def test_one_epoch(model: torch.nn.Module, loader: Iterable[Tuple[torch.Tensor, torch.Tensor, int]], mask_rate: float,
                   mean=None, std=None, min_val=None, max_val=None, norm_type: str = "znorm",
                   criterion: Optional[Callable] = None, metric_fn_dict: Optional[Dict[str, Callable]] = None,
                   nodes_per_graph: Optional[int] = None, gpu_warmup_times: int = 10, use_same_mask: bool = False,
                   rng: Optional[np.random.RandomState] = None, do_test_on_sensors: bool = False,
                   required_idx: Sequence[int] = ()) -> Tuple[float, Dict[str, float]]:
    """``loader`` yields ``(x, edge_index, num_graphs)`` with x == y (e.g. ``SnapshotStore.batches``).  Returns
    ``(loss, metrics)`` with the reference's keys plus ``{prefix}_time`` (ms/graph) and ``{prefix}_throughput``.
    ``do_test_on_sensors`` (evaluation.py:288-294): every mask contains ``required_idx`` (node indices inside a graph) and
    the metric keys carry the ``_sensor`` postfix; with an empty ``required_idx`` it is the plain pass under other keys."""
    model.eval()
    criterion = criterion or torch.nn.MSELoss()
    metric_fn_dict = metric_fn_dict or get_metric_fn_collection("test")
    rng = rng or np.random
    required = list(required_idx) if do_test_on_sensors else []
    postfix = "_sensor" if do_test_on_sensors else ""
    total_loss, total = 0.0, {k: 0.0 for k in metric_fn_dict}
    timer, all_mask, n_graphs = Timer(), None, 0
    with torch.no_grad():
        for x, edge_index, num_graphs in loader:
            y = x
            npg = nodes_per_graph or x.shape[0] // num_graphs
            if all_mask is None or not use_same_mask or all_mask.shape[0] != x.shape[0]:
                all_mask = generate_batch_mask([npg] * num_graphs, mask_rate, rng, required)
            x1 = x.clone()
            x1[all_mask] = 0
            out = timer.auto_measure(model, num_graphs, gpu_warmup_times)(x1, edge_index, None, None)
            y_pred, y_true = out[all_mask], y[all_mask]
            p_r = descale(y_pred, norm_type, mean, std, min_val, max_val)
            t_r = descale(y_true, norm_type, mean, std, min_val, max_val)
            total_loss += float(criterion(y_pred, y_true)) * num_graphs
            for k, fn in metric_fn_dict.items():
                total[k] += float(fn(p_r, t_r)) * num_graphs
            n_graphs += num_graphs
    metrics = {k: v / n_graphs for k, v in total.items()}
    prefix = list(metric_fn_dict.keys())[0].split("_")[0]
    metrics[prefix + "_time"] = timer.compute_time(n_graphs)
    metrics[prefix + "_throughput"] = timer.compute_throughput(n_graphs)
    return total_loss / n_graphs, {k + postfix: v for k, v in metrics.items()}


def test_trials(model: torch.nn.Module, make_loader: Callable[[], Iterable], num_test_trials: int, mask_rate: float,
                required_idx: Sequence[int] = (), **kw):
    """The trial loop of evaluation.py:355-403: ``num_test_trials`` times an all-nodes pass and a sensor pass over a fresh
    loader, results collected per trial.  Returns ``(test_losses, test_metrics, sensor_losses, sensor_metrics)`` with the
    metric dicts mapping a key to the list of its per-trial values (``defaultdict(list)`` in the reference)."""
    from collections import defaultdict
    losses, metrics, s_losses, s_metrics = [], defaultdict(list), [], defaultdict(list)
    for _ in range(int(num_test_trials)):
        loss, m = test_one_epoch(model, make_loader(), mask_rate, do_test_on_sensors=False, **kw)
        s_loss, s_m = test_one_epoch(model, make_loader(), mask_rate, do_test_on_sensors=True, required_idx=required_idx, **kw)
        losses.append(loss); s_losses.append(s_loss)
        for k, v in m.items():
            metrics[k].append(v)
        for k, v in s_m.items():
            s_metrics[k].append(v)
    return losses, dict(metrics), s_losses, dict(s_metrics)



# ---- the epoch on the device (gatres_stage_rows_mask_required + gatres_model_forward + gatres_masked_metrics) ----------------
METRICS_RECORD = 16            # GATRES_METRICS_RECORD of include/gatres.h: doubles per batch in the moment table


def metrics_from_moments(table, graphs_per_batch: Sequence[int], prefix: str = "test") -> Tuple[float, Dict[str, float]]:
    """The loss (``MSELoss`` on scaled values) and the seven metrics of ``get_metric_fn_collection(prefix)`` from a moment
    table ``[B, METRICS_RECORD]``, each batch's value weighted by its graph count and divided by the dataset size
    (train.py:278-279, evaluation.py:340-345).  fp64.  torch's NaN cases carry over: no kept element gives ``error`` NaN,
    zero variance gives ``corr`` / ``r2`` NaN, an empty mask gives NaN everywhere but ``mynse``, which is 1.0 there as
    ``calculate_nse`` is on empty tensors (0 / (0 + 1e-12))."""
    T = np.asarray(table, dtype=np.float64).reshape(-1, METRICS_RECORD)
    w = [int(g) for g in graphs_per_batch]
    if len(w) != T.shape[0]:
        raise ValueError(f"{T.shape[0]} records for {len(w)} batches")
    with np.errstate(invalid="ignore", divide="ignore"):
        M = T[:, 0]
        corr = np.clip(T[:, 8] / (np.sqrt(T[:, 6]) * np.sqrt(T[:, 7])), -1.0, 1.0)
        per = {"loss": T[:, 1] / M,
               f"{prefix}_error": T[:, 10] / T[:, 9],
               f"{prefix}_0.1": T[:, 11] / M,
               f"{prefix}_corr": corr,
               f"{prefix}_r2": corr * corr,
               f"{prefix}_mae": T[:, 2] / M,
               f"{prefix}_rmse": np.sqrt(T[:, 3] / M),
               f"{prefix}_mynse": 1.0 - T[:, 3] / (T[:, 7] + 1e-12)}
    n = sum(w)
    out = {}
    for k, v in per.items():
        acc = 0.0
        for b, g in enumerate(w):          # the host loop's order: total += metric * num_graphs, batch by batch
            acc += float(v[b]) * g
        out[k] = acc / n
    return out.pop("loss"), out


def _same_fn(a, b) -> bool:
    if isinstance(a, partial) and isinstance(b, partial):
        return a.func is b.func and a.args == b.args and a.keywords == b.keywords
    return a is b


def _check_reference_metrics(criterion, metric_fn_dict, prefix: str) -> None:
    if criterion is not None and not (isinstance(criterion, torch.nn.MSELoss) and criterion.reduction == "mean"):
        raise ValueError(f"evaluate_store computes MSELoss(reduction='mean') only; got {criterion!r}")
    if metric_fn_dict is not None:
        ref = get_metric_fn_collection(prefix)
        if list(metric_fn_dict) != list(ref) or not all(_same_fn(metric_fn_dict[k], ref[k]) for k in ref):
            raise ValueError("evaluate_store computes get_metric_fn_collection(prefix) only (the reference's seven metrics); "
                             "use test_one_epoch for other metric functions")


class _EvalPlan:
    """Static buffers of one batch size: staged inputs / targets, mask, predictions, the plan and the forward's call state."""

    def __init__(self, model, store, num_graphs: int, recipe=None):
        if recipe is None:
            npg = store.nodes_per_graph
            self.num_nodes, self.edge_index, sizes = num_graphs * npg, store.edge_index(num_graphs), [npg] * num_graphs
        else:          # a MultiSnapshotStore's batch: ``recipe[k]`` graphs of network k
            self.num_nodes, self.edge_index, sizes = store.num_nodes(recipe), store.edge_index(recipe), store.nodes_per_graph(recipe)
        self.num_graphs, self.recipe = num_graphs, recipe
        self.plan = model.plan_for(self.edge_index, self.num_nodes)
        self.node_ptr = self.plan.node_ptr_for(sizes)
        dev = store.device
        self.x = torch.empty(self.num_nodes, dtype=torch.float32, device=dev)
        self.mask = torch.empty(self.num_nodes, dtype=torch.uint8, device=dev)
        self.out = torch.empty((self.num_nodes, 1), dtype=torch.float32, device=dev)

    def refresh(self, model) -> "_EvalPlan":
        """The forward's call state and buffers as the model holds them now (through its caches: no device work)."""
        self.state = model._call_state(self.plan)
        self.saved = model._eval_saved_for(self.plan, self.state["buf_key"]) if self.state["window"] else None
        return self


# model -> {(edge_index identity, nodes, engine configuration): _EvalPlan}.  The model's own plan cache remembers ONE edge_index
# tensor by identity and hashes any other (a device hash and a read-back): the full and the ragged batch size alternate every
# epoch, and each switch would cost a synchronisation.
_EVAL_PLANS = weakref.WeakKeyDictionary()
_EVAL_PLANS_MAX = 32          # (a multi-network schedule has one plan per distinct recipe: the main one and its tails)


def _eval_plan(model, store, num_graphs: int, recipe=None) -> _EvalPlan:
    ei = store.edge_index(num_graphs if recipe is None else recipe)
    nodes = num_graphs * store.nodes_per_graph if recipe is None else store.num_nodes(recipe)
    # (the recipe is part of the key: a one-network recipe shares its edge_index tensor with that network's SnapshotStore)
    key = (ei.data_ptr(), ei._version, nodes, str(ei.device), bool(model.fused), None if recipe is None else tuple(recipe))
    plans = _EVAL_PLANS.setdefault(model, {})
    P = plans.get(key)
    if P is None or P.edge_index is not ei:
        if len(plans) >= _EVAL_PLANS_MAX:
            plans.clear()
        P = plans[key] = _EvalPlan(model, store, num_graphs, recipe)
    return P.refresh(model)


def _enqueue_stage(lib, store, P: _EvalPlan, rows: torch.Tensor, mask_rate: float, seed64: int, step_ptr: int, req_dev,
                   num_required: int, stream) -> None:
    """Collation of the snapshots ``rows`` into the plan's ``x`` + the batch's mask (sampler step read from ``step_ptr``)."""
    from . import _native
    _native.check(lib.gatres_stage_rows_mask_required(
        store.data.data_ptr(), rows.data_ptr(), store.nodes_per_graph, P.x.data_ptr(), None, P.node_ptr.data_ptr(), P.num_graphs,
        float(mask_rate), seed64, step_ptr, _native.ptr(req_dev), num_required, P.mask.data_ptr(), stream),
        "gatres_stage_rows_mask_required")


def _enqueue_stage_multi(lib, store, P: _EvalPlan, rows_ptr: int, mask_rate: float, seed64: int, step_ptr: int, req_ptr,
                         req_idx, stream) -> None:
    """``_enqueue_stage`` for a ``MultiSnapshotStore``: the rows (at device address ``rows_ptr``) name snapshots inside their
    networks; the required nodes are a CSR per network."""
    from . import _native
    _native.check(lib.gatres_stage_multi_rows_mask_required(
        store.table.data_ptr(), store.num_networks, store.net_of_graph(P.recipe).data_ptr(), rows_ptr, P.node_ptr.data_ptr(),
        P.num_graphs, P.x.data_ptr(), None, float(mask_rate), seed64, step_ptr, _native.ptr(req_ptr), _native.ptr(req_idx),
        P.mask.data_ptr(), stream), "gatres_stage_multi_rows_mask_required")


def _enqueue_forward(lib, flat: torch.Tensor, P: _EvalPlan, stream) -> None:
    """The inference forward on the staged batch, as ``model(x1, edge_index)`` with ``x1[mask] = 0`` computes it."""
    from . import _native
    st = P.state
    _native.check(lib.gatres_model_forward(st["mref_infer"], st["gref"], flat.data_ptr(), P.x.data_ptr(), P.mask.data_ptr(),
                                           P.out.data_ptr(), _native.ptr(P.saved), st["scratch"].data_ptr(), stream),
                  "gatres_model_forward")


def _enqueue_moments(lib, P: _EvalPlan, scale: float, offset: float, table: torch.Tensor, slot: int, stream) -> None:
    from . import _native
    _native.check(lib.gatres_masked_metrics(P.out.data_ptr(), P.x.data_ptr(), P.mask.data_ptr(), P.num_nodes, scale, offset,
                                            table.data_ptr(), slot, table.shape[0], None, stream), "gatres_masked_metrics")


def _store_descale(store, norm_type: Optional[str]) -> Tuple[float, float]:
    norm_type = store.norm_type if norm_type is None else norm_type
    if norm_type == "znorm":
        return float(store.std), float(store.mean)
    if norm_type == "unused":
        return 1.0, 0.0
    raise ValueError(f"norm_type={norm_type!r}: a SnapshotStore is z-normalised ('znorm') or not normalised ('unused')")


def _mix_seed(seed: int, *salt: int) -> int:
    z = int(seed) & 0xFFFFFFFFFFFFFFFF
    for s in salt:
        z = (z + 0x9E3779B97F4A7C15 * (int(s) + 1)) & 0xFFFFFFFFFFFFFFFF
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
        z ^= z >> 31
    return z


def evaluate_store(model: torch.nn.Module, store, batch_size: int, mask_rate: float, *, prefix: str = "test",
                   do_test_on_sensors: bool = False, required_idx: Sequence[int] = (), use_same_mask: bool = False,
                   seed: int = 0, gpu_warmup_times: int = 10, norm_type: Optional[str] = None,
                   criterion: Optional[Callable] = None, metric_fn_dict: Optional[Dict[str, Callable]] = None,
                   per_network: bool = False, graphs_per_network: Optional[Sequence[int]] = None,
                   observed_idx: Optional[Sequence[int]] = None, noise_std=None, noise_seed: int = 0,
                   _capture: Optional[List] = None) -> Tuple[float, Dict[str, float]]:
    """``test_one_epoch`` over a ``SnapshotStore`` on the device: the same ``(loss, metrics)`` keys -- the reference's seven
    metrics, ``{prefix}_time`` (ms/graph) and ``{prefix}_throughput``, ``_sensor`` postfixed on the sensor pass.

    The store is taken in order (no shuffle) in batches of ``batch_size``; a ragged last batch runs on its own plan.  Per
    batch, three launches on the current stream: staging + mask (``gatres_stage_rows_mask_required``: exactly
    ``int(n * mask_rate)`` masked nodes per graph, the ``required_idx`` ones always on the sensor pass), the inference forward
    with the mask (``gatres_model_forward``, as ``model(x1, edge_index)`` with ``x1[mask] = 0`` computes it), and the moments
    (``gatres_masked_metrics``).  ``Timer``'s definition is kept: ``gpu_warmup_times`` untimed forwards on the first batch, then
    one event pair around each forward; the events are read after the epoch's one synchronisation.  Masks come from the device
    sampler (seeded by ``seed`` and the batch index; ``use_same_mask``: one mask per batch size, as the host loop reuses its
    mask while the batch shape stays), not from numpy: the metrics agree with ``test_one_epoch`` given the same masks.  The
    same ``seed`` draws the same masks: a validation pass per training epoch that wants fresh masks, as the host loop's numpy
    stream gives it, passes ``seed=epoch``.
    ``norm_type``: ``None`` takes the store's (``znorm``: descaled with its mean / std; ``unused``: not descaled).
    Only ``MSELoss`` and ``get_metric_fn_collection(prefix)`` are computed; anything else passed as ``criterion`` /
    ``metric_fn_dict`` is refused -- ``get_criterion("mae")`` / ``("sce")`` included, whatever criterion the model was trained
    with (the moment record carries no such sums): their validation loss comes from ``test_one_epoch``.  ``_capture`` (tests): a list that receives ``(mask, out, x, num_graphs)`` per batch.

    ``observed_idx`` (a fixed sensor layout: node indices inside a graph, distinct): every batch is staged by
    ``gatres_stage_rows_mask_sensors`` without dropout and with every graph under the layout -- all nodes hidden but these, the
    mask a ``PressureEstimator`` of that layout is deployed under.  The mask is deterministic: ``seed`` and ``mask_rate`` do not
    enter.  Forward, moments, keys and prefixes are unchanged.  Refused together with ``do_test_on_sensors``, ``required_idx``,
    ``use_same_mask`` and a ``MultiSnapshotStore``.

    ``noise_std`` (with ``observed_idx`` only; one non-negative finite number or one per sensor, physical units) and
    ``noise_seed``: the layout pass under one realisation of measurement noise.  Every batch is staged by
    ``gatres_stage_rows_mask_sensors_noisy`` (dropout 0, share 1, no step counter: member 0), so the staged ``x`` at the sensors
    is bit for bit that of ``PressureEstimator.estimate_store(store, noise_std=, noise_seed=, noise_member=0)``; the targets at
    the hidden nodes stay clean.  A ``noise_std`` of zeros is the clean layout pass.

    A ``MultiSnapshotStore`` is taken by its schedule (``store.schedule(batch_size, drop_last=False)``, the recipe the
    default or ``graphs_per_network``), every network's snapshots in order, staged by ``gatres_stage_multi_rows_mask_required``.
    ``required_idx`` is then a sequence of K sequences, one per network (sensor sets differ between networks).
    ``per_network=True`` returns ``(loss, metrics, per_network)``: the third value lists, per network, ``{"loss": ..,
    "{prefix}_error": .., ...}`` over that network's masked nodes only, each batch weighted by its graphs of that network --
    from one more moments launch per network and batch over the network's node range; without it the launches are those of a
    single store."""
    from . import _native
    from .multi_snapshot_store import MultiSnapshotStore
    _check_reference_metrics(criterion, metric_fn_dict, prefix)
    if batch_size <= 0:
        raise ValueError("batch_size must be positive")
    multi = isinstance(store, MultiSnapshotStore)
    if not multi and (per_network or graphs_per_network is not None):
        raise ValueError("per_network / graphs_per_network belong to a MultiSnapshotStore")
    if observed_idx is not None:
        _check_layout_options(multi, do_test_on_sensors, required_idx, use_same_mask)
    elif noise_std is not None:
        raise ValueError("noise_std belongs to the layout pass: pass observed_idx (the sensors whose readings are noisy)")
    scale, offset = _store_descale(store, norm_type)
    S = len(store)
    if S == 0:
        raise ValueError("empty store")
    if observed_idx is not None:
        cut = _SingleBatches(store, batch_size, mask_rate, observed=observed_idx, noise_std=noise_std, noise_seed=noise_seed)
    else:
        cut = (_MultiBatches if multi else _SingleBatches)(store, batch_size, mask_rate,
                                                            required_idx if do_test_on_sensors else None, graphs_per_network)
    postfix = "_sensor" if do_test_on_sensors else ""
    model.eval()
    if not model._flat_is_current():
        model._flatten_parameters()
    flat = model._flat
    dev = store.device
    if flat.device != dev:
        raise ValueError(f"model is on {flat.device}, the store on {dev}")
    lib = _native.load()
    sizes, nb = cut.sizes, len(cut.sizes)
    with torch.cuda.device(dev):
        stream = _native.current_stream(dev)
        plans = cut.plans(model)
        # the sampler's step of each batch: the batch index, or one mask per kind of batch under use_same_mask
        steps = [cut.kind(b) if use_same_mask else b for b in range(nb)]
        # (uploads from pinned memory, asynchronous: a pageable copy would synchronise the stream; the host tensors stay
        #  alive until the epoch's synchronisation below)
        steps_host = torch.tensor(steps, dtype=torch.int64).pin_memory()
        steps_dev = steps_host.to(dev, non_blocking=True)
        pinned = cut.upload(pinned=True)
        table = torch.zeros((nb, METRICS_RECORD), dtype=torch.float64, device=dev)
        net_tables = torch.zeros((store.num_networks, nb, METRICS_RECORD), dtype=torch.float64, device=dev) if per_network else None
        events = []
        seed64 = int(seed) & 0xFFFFFFFFFFFFFFFF

        def forward(P: _EvalPlan) -> None:
            _enqueue_forward(lib, flat, P, stream)

        for b, g in enumerate(sizes):
            P = plans[cut.keys[b]]
            cut.stage(lib, P, b, mask_rate, seed64, steps_dev.data_ptr() + 8 * b, True, stream)
            if b == 0:
                for _ in range(max(int(gpu_warmup_times), 0)):
                    forward(P)
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            forward(P)
            end.record()
            events.append((start, end))
            _enqueue_moments(lib, P, scale, offset, table, b, stream)
            if per_network:          # one more moments launch per network of the batch, over that network's node range
                for k, (lo, hi) in enumerate(store.node_ranges(cut.keys[b])):
                    if hi > lo:
                        _native.check(lib.gatres_masked_metrics(
                            P.out.data_ptr() + 4 * lo, P.x.data_ptr() + 4 * lo, P.mask.data_ptr() + lo, hi - lo, scale, offset,
                            net_tables[k].data_ptr(), b, nb, None, stream), "gatres_masked_metrics")
            if _capture is not None:
                _capture.append((P.mask.clone(), P.out.clone(), P.x.clone(), g))
        torch.cuda.synchronize(dev)
        host = table.cpu().numpy()
        net_host = net_tables.cpu().numpy() if per_network else None
        del steps_host, pinned
    timer = Timer()
    timer.timings = [s.elapsed_time(e) for s, e in events]
    timer.num_graphs = list(sizes)
    loss, metrics = metrics_from_moments(host, sizes, prefix)
    key = list(metrics.keys())[0].split("_")[0]            # (test_one_epoch's derivation of the timing keys' prefix)
    metrics[key + "_time"] = timer.compute_time(S)
    metrics[key + "_throughput"] = timer.compute_throughput(S)
    metrics = {k + postfix: v for k, v in metrics.items()}
    if not per_network:
        return loss, metrics
    nets = []
    for k in range(store.num_networks):
        used = [b for b, r in enumerate(cut.keys) if r[k] > 0]
        if not used:
            nets.append({})
            continue
        l_k, m_k = metrics_from_moments(net_host[k][used], [cut.keys[b][k] for b in used], prefix)
        nets.append({"loss": l_k, **{name + postfix: v for name, v in m_k.items()}})
    return loss, metrics, nets


def _check_layout_options(multi: bool, do_test_on_sensors: bool, required_idx, use_same_mask: bool) -> None:
    """What ``evaluate_store(observed_idx=...)`` excludes: the layout IS the mask, so the sampler's options have no meaning."""
    if multi:
        raise NotImplementedError("observed_idx with a MultiSnapshotStore is not implemented (a layout per network would be "
                                  "needed): evaluate one network's SnapshotStore")
    if do_test_on_sensors or len(tuple(required_idx or ())) > 0:
        raise ValueError("observed_idx fixes the mask (everything hidden but the sensors): do_test_on_sensors / required_idx "
                         "belong to the sampled masks")
    if use_same_mask:
        raise ValueError("observed_idx fixes the mask: use_same_mask belongs to the sampled masks")


def required_csr(store, required_idx, mask_rate: float):
    """Per-network required nodes of a ``MultiSnapshotStore`` as host CSR lists ``(req_ptr [K + 1], req_idx)``: ``required_idx``
    must be a sequence of K sequences (a flat list is refused for K > 1: sensor sets belong to a network), every index inside
    its network, and every network must keep a positive sampled part (utils/auxil.py:151-153)."""
    K = store.num_networks
    seq = list(required_idx)
    flat = all(isinstance(i, (int, np.integer)) for i in seq)
    if flat and seq and K > 1:
        raise ValueError(f"required_idx is a flat list, the store holds {K} networks: pass one sequence per network")
    if flat:
        seq = [seq] + [[] for _ in range(K - 1)] if seq else [[] for _ in range(K)]
    if len(seq) != K:
        raise ValueError(f"required_idx holds {len(seq)} sequences for {K} networks")
    ptr, idx = [0], []
    for k, r in enumerate(seq):
        r = sorted(set(int(i) for i in r))
        n = store.nodes_per_graph_of(k)
        if r and (r[0] < 0 or r[-1] >= n):
            raise ValueError(f"required_idx of network {k} must lie in [0, {n})")
        if int(n * mask_rate) - len(r) <= 0:
            raise ValueError(f"mask length must be positive (network {k})")
        idx += r
        ptr.append(len(idx))
    return ptr, idx


class _SingleBatches:
    """How an evaluation pass cuts a ``SnapshotStore`` into batches -- in order, ``batch_size`` at a time, a ragged last one --
    and stages batch ``b``.  ``keys[b]`` names the batch's plan (its graph count); ``required``: the sensor nodes (None: no
    sensor pass)."""

    def __init__(self, store, batch_size: int, mask_rate: float, required=None, graphs_per_network=None, observed=None,
                 noise_std=None, noise_seed: int = 0):
        npg, S = store.nodes_per_graph, len(store)
        self.required = sorted(set(int(i) for i in required)) if required is not None else []
        if self.required and (self.required[0] < 0 or self.required[-1] >= npg):
            raise ValueError(f"required_idx must lie in [0, {npg})")
        # observed: a fixed sensor layout -- every batch gets its mask (gatres_stage_rows_mask_sensors without dropout, every
        # graph under the layout) and the sampler draws nothing
        self.observed = None
        if observed is not None:
            from .estimation import _check_observed
            self.observed = _check_observed(observed, npg)
            # noise_std: one realisation of measurement noise on the sensors' readings (gatres_stage_rows_mask_sensors_noisy,
            # member 0); sigma in the store's units, by the statement PressureEstimator uses for full rows.  All zeros: none.
            if noise_std is not None:
                from .estimation import _check_seed, noise_sigma
                self.noise_seed = _check_seed(noise_seed)
                sigma = noise_sigma(noise_std, len(self.observed), store.norm_type, store.std, getattr(store, "eps", 1e-8),
                                    full_rows=True)
                self.sigma_host = sigma if sigma.any() else None
        elif int(npg * mask_rate) - len(self.required) <= 0:
            raise ValueError("mask length must be positive")
        self.obs = None
        if observed is None or noise_std is None:
            self.sigma_host, self.noise_seed = None, 0
        self.sigma = None
        self.store, self.batch_size = store, int(batch_size)
        nb = (S + batch_size - 1) // batch_size
        self.sizes = [min(batch_size, S - b * batch_size) for b in range(nb)]
        self.keys = list(self.sizes)
        self.offsets = [b * batch_size for b in range(nb)]
        self.rows = self.req = None

    def kind(self, b: int) -> int:
        """Which of the pass's batch shapes batch ``b`` has (``use_same_mask``: one mask per shape)."""
        return 0 if self.sizes[b] == self.batch_size else 1

    def plans(self, model) -> dict:
        return {g: _eval_plan(model, self.store, g) for g in sorted(set(self.sizes))}

    def upload(self, pinned: bool) -> list:
        """Rows and required nodes onto the device; returns the pinned host tensors, to be kept alive until the pass's
        synchronisation (``pinned=False``: plain copies, for buffers made once)."""
        dev = self.store.device
        self.rows = torch.arange(len(self.store), dtype=torch.int64, device=dev)
        keep = []
        if self.required:
            host = torch.tensor(self.required, dtype=torch.int32)
            keep = [host.pin_memory()] if pinned else [host]
            self.req = keep[0].to(dev, non_blocking=pinned)
        if self.observed is not None:
            host = torch.tensor(self.observed, dtype=torch.int32)
            keep.append(host.pin_memory() if pinned else host)
            self.obs = keep[-1].to(dev, non_blocking=pinned)
            if self.sigma_host is not None:
                host = torch.from_numpy(self.sigma_host)
                keep.append(host.pin_memory() if pinned else host)
                self.sigma = keep[-1].to(dev, non_blocking=pinned)
        return keep

    def stage(self, lib, P: _EvalPlan, b: int, mask_rate: float, seed64: int, step_ptr: int, sensors: bool, stream) -> None:
        rows = self.rows[self.offsets[b]: self.offsets[b] + self.sizes[b]]
        if self.observed is not None:
            from .sensor_layout import stage_rows
            stage_rows(lib, self.store.data, rows.data_ptr(), self.store.nodes_per_graph, P.x, None, P.node_ptr, P.num_graphs,
                       self.obs, len(self.observed), 0.0, 1.0, min(max(float(mask_rate), 0.0), 1.0), seed64,
                       step_ptr if self.sigma is None else None, P.mask, stream, sigma=self.sigma, noise_seed=self.noise_seed)
            return
        _enqueue_stage(lib, self.store, P, rows, mask_rate, seed64, step_ptr, self.req if sensors else None,
                       len(self.required) if sensors else 0, stream)


class _MultiBatches(_SingleBatches):
    """``_SingleBatches`` for a ``MultiSnapshotStore``: the batches of its in-order schedule (``drop_last=False``), a plan per
    distinct recipe (``keys[b]``: batch b's recipe), staged by ``gatres_stage_multi_rows_mask_required`` with the required
    nodes as a CSR per network."""

    def __init__(self, store, batch_size: int, mask_rate: float, required=None, graphs_per_network=None):
        self.req_ptr_l, self.req_idx_l = required_csr(
            store, required if required is not None else [[] for _ in range(store.num_networks)], mask_rate)
        self.store, self.batch_size = store, int(batch_size)
        recipe = store.recipe(batch_size, graphs_per_network)
        self.schedule = store.schedule(batch_size, recipe, drop_last=False)
        self.keys = [self.schedule.recipe] * self.schedule.nfull + list(self.schedule.tails)
        self.sizes = self.schedule.sizes
        self.offsets = [0]
        for r in self.keys[:-1]:
            self.offsets.append(self.offsets[-1] + sum(r))
        self.kinds = list(dict.fromkeys(self.keys))
        self.rows = self.req = self.req_ptr = None

    def kind(self, b: int) -> int:
        return self.kinds.index(self.keys[b])

    def plans(self, model) -> dict:
        return {r: _eval_plan(model, self.store, sum(r), r) for r in self.kinds}

    def upload(self, pinned: bool) -> list:
        dev = self.store.device
        host = [self.store.epoch_rows_host(self.schedule, shuffle=False)]
        if self.req_idx_l:
            host += [torch.tensor(self.req_ptr_l, dtype=torch.int32), torch.tensor(self.req_idx_l, dtype=torch.int32)]
        keep = [t.pin_memory() for t in host] if pinned else host
        on_dev = [t.to(dev, non_blocking=pinned) for t in keep]
        self.rows = on_dev[0]
        if self.req_idx_l:
            self.req_ptr, self.req = on_dev[1], on_dev[2]
        return keep

    def stage(self, lib, P: _EvalPlan, b: int, mask_rate: float, seed64: int, step_ptr: int, sensors: bool, stream) -> None:
        _enqueue_stage_multi(lib, self.store, P, self.rows.data_ptr() + 8 * self.offsets[b], mask_rate, seed64, step_ptr,
                             self.req_ptr if sensors else None, self.req if sensors else None, stream)


class _ValidationPass:
    """The validation epoch of ``GATResTrainer.fit``: ``evaluate_store``'s launches per batch -- staging + mask, inference
    forward, masked-metric moments -- plus, for the ``mae`` / ``sce`` criteria, one ``gatres_masked_loss`` launch whose fp32
    loss goes into a per-batch array (the reference's ``criterion(y_pred, y_true)``).  Nothing is read back and nothing
    synchronises: the moment table, the loss array and the per-batch graph counts stay on the device for
    ``gatres_epoch_control``.  Everything static (row order, sampler steps, graph counts, tables) is made once; with the same
    ``seed`` the moment table is bit for bit the one ``evaluate_store(seed=seed, gpu_warmup_times=0)`` forms.  ``store``: a
    ``SnapshotStore`` or a ``MultiSnapshotStore`` (then the batches are its in-order schedule's).  ``observed_idx``: the pass
    of ``evaluate_store(observed_idx=...)`` -- everything hidden but a fixed sensor layout; ``noise_std`` / ``noise_seed``: that
    pass under one fixed realisation of measurement noise, ``evaluate_store(observed_idx=, noise_std=, noise_seed=)``'s."""

    def __init__(self, model, store, batch_size: int, mask_rate: float, criterion: str = "mse",
                 observed_idx: Optional[Sequence[int]] = None, noise_std=None, noise_seed: int = 0):
        from . import _native
        from .multi_snapshot_store import MultiSnapshotStore
        multi = isinstance(store, MultiSnapshotStore)
        if observed_idx is not None:
            _check_layout_options(multi, False, (), False)
        if batch_size <= 0:
            raise ValueError("batch_size must be positive")
        if len(store) == 0:
            raise ValueError("empty store")
        if observed_idx is None and noise_std is not None:
            raise ValueError("noise_std belongs to the layout pass: pass observed_idx")
        if observed_idx is not None:          # (the layout mask of evaluate_store(observed_idx=...): deterministic, no sampler)
            self.cut = _SingleBatches(store, int(batch_size), float(mask_rate), observed=observed_idx, noise_std=noise_std,
                                      noise_seed=noise_seed)
        else:
            self.cut = (_MultiBatches if multi else _SingleBatches)(store, int(batch_size), float(mask_rate))
        self.cut.upload(pinned=False)
        self.model, self.store, self.batch_size, self.mask_rate = model, store, int(batch_size), float(mask_rate)
        self.criterion = _native.CRITERIA[criterion]
        self.scale, self.offset = _store_descale(store, None)
        dev = store.device
        self.sizes = self.cut.sizes
        nb = len(self.sizes)
        self.steps = torch.arange(nb, dtype=torch.int64, device=dev)          # the sampler's step of a batch: its index
        self.graphs = torch.tensor(self.sizes, dtype=torch.int32).to(dev)
        self.table = torch.zeros((nb, METRICS_RECORD), dtype=torch.float64, device=dev)
        self.losses = self.g_out = None
        if self.criterion != _native.LOSS_MSE:
            nodes = max(store.num_nodes(r) for r in self.cut.keys) if multi else batch_size * store.nodes_per_graph
            self.losses = torch.zeros(nb, dtype=torch.float32, device=dev)
            self.g_out = torch.empty(nodes, dtype=torch.float32, device=dev)

    def enqueue(self, seed: int, _capture: Optional[List] = None) -> None:
        from . import _native
        model, store, cut = self.model, self.store, self.cut
        flat = model.flat_parameters
        if flat.device != store.device:
            raise ValueError(f"model is on {flat.device}, the store on {store.device}")
        lib = _native.load()
        seed64 = int(seed) & 0xFFFFFFFFFFFFFFFF
        with torch.cuda.device(store.device):
            stream = _native.current_stream(store.device)
            plans = cut.plans(model)
            for b, g in enumerate(self.sizes):
                P = plans[cut.keys[b]]
                cut.stage(lib, P, b, self.mask_rate, seed64, self.steps.data_ptr() + 8 * b, False, stream)
                _enqueue_forward(lib, flat, P, stream)
                _enqueue_moments(lib, P, self.scale, self.offset, self.table, b, stream)
                if self.losses is not None:
                    _native.check(lib.gatres_masked_loss(P.out.data_ptr(), P.x.data_ptr(), P.mask.data_ptr(), self.criterion,
                                                         self.losses.data_ptr() + 4 * b, self.g_out.data_ptr(), P.num_nodes,
                                                         stream), "gatres_masked_loss")
                if _capture is not None:
                    _capture.append((P.mask.clone(), P.out.clone(), P.x.clone(), g))


def evaluate_store_trials(model: torch.nn.Module, store, batch_size: int, num_test_trials: int, mask_rate: float,
                          required_idx: Sequence[int] = (), seed: int = 0, **kw):
    """``test_trials`` on the device: per trial an all-nodes pass and a sensor pass of ``evaluate_store``, each with masks of
    its own (the mask seed is derived from ``seed``, the trial and the pass).  Returns ``(test_losses, test_metrics,
    sensor_losses, sensor_metrics)``, the metric dicts mapping a key to the list of its per-trial values."""
    from collections import defaultdict
    losses, metrics, s_losses, s_metrics = [], defaultdict(list), [], defaultdict(list)
    for t in range(int(num_test_trials)):
        loss, m = evaluate_store(model, store, batch_size, mask_rate, do_test_on_sensors=False,
                                 seed=_mix_seed(seed, t, 0), **kw)
        s_loss, s_m = evaluate_store(model, store, batch_size, mask_rate, do_test_on_sensors=True, required_idx=required_idx,
                                     seed=_mix_seed(seed, t, 1), **kw)
        losses.append(loss); s_losses.append(s_loss)
        for k, v in m.items():
            metrics[k].append(v)
        for k, v in s_m.items():
            s_metrics[k].append(v)
    return losses, dict(metrics), s_losses, dict(s_metrics)
