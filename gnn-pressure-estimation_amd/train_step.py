"""Native training step for GATRes: the reference's inner loop body (train.py:159-190) as one stream-ordered
launch sequence -- device mask sampling (auxil.py:143-182), ``x[mask] = 0``, forward, the criterion (MSE, MAE or SCE:
train.py --criterion) on the masked nodes, backward, [RCCL gradient all-reduce], Adam(lr, weight_decay) -- captured once into a hipGraph and replayed.

Data-parallel: one process per GPU, snapshots sharded by graph across ranks, every rank holds the same topology
plan and an identical replica of the flat parameter vector; the only exchange is ONE all-reduce of the flat fp32
gradient per step (RCCL over xGMI; `torch.distributed` backend "nccl"), after which each rank applies the same Adam
update with the gradient scaled by 1/world_size.  Equal masked-node counts per graph make the average of per-rank
mean-losses equal the global-batch mean loss, so the result matches single-process training on the global batch.
"""
from __future__ import annotations

import ctypes as C
import os
import warnings
from collections import OrderedDict
from typing import Callable, Dict, Optional, Sequence, Tuple

import torch

from . import _native, dp
from .epoch_loop import EpochLoop
from .fit_loop import FitHistory, FitLoop, internal_train  # noqa: F401  (part of this module's interface)
from .grad_flow import GradFlow
from .graph_models import GATResMeanConv
from .graph_plan import GraphPlan
from .sensor_layout import SensorLayout, refuse_layout_data_parallel, stage_rows as _stage_rows_sensors

PHASE_MASK, PHASE_FORWARD, PHASE_BACKWARD, PHASE_ADAM = 1, 2, 4, 8
STATUS_FAULT_COUNT, STATUS_DROPPED_STEPS = 1, 3      # words of the fused path's status block (csrc/gatres_layout.h: FUSED_STATUS_*)
PART_FIRST, PART_LAST, PART_REDUCE = 1, 2, 4
FLAG_PER_OP, FLAG_WT_VALID, FLAG_GRADS_DEFERRED, FLAG_GRADS_ONLY, FLAG_MASK_NEXT = 1, 2, 4, 8, 16
FLAG_LOSS_MAE, FLAG_LOSS_SCE = 32, 64
_CRITERION_FLAGS = {"mse": 0, "mae": FLAG_LOSS_MAE, "sce": FLAG_LOSS_SCE}
MAX_CACHED_GRAPHS = 40          # floor of the captured-step cache; bind_batches() sizes it from the number of bound batches
_STEP = PHASE_FORWARD | PHASE_BACKWARD | PHASE_ADAM          # a whole step on a mask that is in place


class _TrainStepC(C.Structure):
    """gatres_train_step_t"""
    _fields_ = [("model", _native.GatresModel), ("graph", C.POINTER(_native.GatresGraph)),
                ("params", C.c_void_p), ("grads", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p),
                ("step_counter", C.c_void_p), ("x", C.c_void_p), ("y", C.c_void_p), ("mask", C.c_void_p),
                ("node_ptr", C.c_void_p), ("num_graphs", C.c_int32), ("phases", C.c_int32),
                ("mask_rate", C.c_double), ("seed", C.c_uint64),
                ("out", C.c_void_p), ("g_out", C.c_void_p), ("loss", C.c_void_p), ("saved", C.c_void_p),
                ("scratch", C.c_void_p),
                ("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double),
                ("weight_decay", C.c_double), ("grad_scale", C.c_float), ("flags", C.c_int32),
                ("hparams", C.c_void_p), ("block_lo", C.c_int32), ("block_hi", C.c_int32), ("mask_next", C.c_void_p),
                ("autoclip", C.POINTER(_native.GatresAutoClip))]


class _AutoClipState:
    """AutoClip's device state (``gatres_autoclip_t``; reference utils/gradient_clipping.py ``GradientClipping``): the norm
    history as a log in step order and as a sorted copy in two ping-pong buffers, the count, and the last step's norm / clip
    value / coefficient.  One object per optimizer state: a sibling trainer shares it like it shares the Adam moments.

    The history never leaves the device while training.  Its buffers are pre-sized; ``reserve(k)`` -- called before every
    launch sequence that can run k updates -- grows them (a copy into buffers of twice the size) before the count could get
    there.  Captured steps hold the buffers' addresses, so a growth bumps ``generation`` and the trainers capture again."""

    def __init__(self, percentile: float, num_params: int, device, capacity: int):
        self.percentile = float(percentile)
        self.device = device
        f64 = dict(dtype=torch.float64, device=device)
        self.ctl = torch.zeros(8, dtype=torch.int64, device=device)
        self.partials = torch.zeros(max(int(_native.load().gatres_autoclip_partials(num_params)), 1), **f64)
        self.out = torch.zeros(3, **f64)                  # {norm, clip value, coefficient}
        self.capacity = 0
        self.log = self.sorted0 = self.sorted1 = None
        self.upper = 0           # host-side bound on the count: updates enqueued since the last reset
        self.generation = 0
        self._alloc(max(int(capacity), 1))

    def _alloc(self, capacity: int) -> None:
        f64 = dict(dtype=torch.float64, device=self.device)
        new = [torch.zeros(capacity, **f64) for _ in range(3)]
        for dst, src in zip(new, (self.log, self.sorted0, self.sorted1)):
            if src is not None:
                dst[:src.numel()].copy_(src)              # (stream-ordered behind every update enqueued so far)
        self.log, self.sorted0, self.sorted1 = new
        self.capacity = capacity
        self.generation += 1
        self.c = _native.GatresAutoClip(
            self.log.data_ptr(), (C.c_void_p * 2)(self.sorted0.data_ptr(), self.sorted1.data_ptr()), self.ctl.data_ptr(),
            self.partials.data_ptr(), self.out[0:1].data_ptr(), self.out[1:2].data_ptr(), self.out[2:3].data_ptr(),
            capacity, self.partials.numel(), 0, self.percentile)

    def reserve(self, updates: int) -> None:
        self.upper += int(updates)
        if self.upper > self.capacity:
            self._alloc(max(2 * self.capacity, self.upper))

    def reset(self) -> None:
        self.ctl[0:1].zero_()
        self.upper = 0

    def save(self):
        return [t.clone() for t in (self.ctl, self.out, self.sorted0, self.sorted1)]

    def restore(self, saved) -> None:
        for dst, src in zip((self.ctl, self.out, self.sorted0, self.sorted1), saved):
            dst[:src.numel()].copy_(src)


def _save(tensors, clip: Optional[_AutoClipState] = None) -> Callable[[], None]:
    """Clone ``tensors`` (and AutoClip's device state) now; the function returned puts them back (stream-ordered copies)."""
    kept = [(t, t.clone()) for t in tensors]
    kept_clip = clip.save() if clip is not None else None

    def restore() -> None:
        for t, c in kept:
            t.copy_(c)
        if clip is not None:              # (the count, and the sorted copy a multi-step warm-up overwrote)
            clip.restore(kept_clip)
    return restore


class _GraphCache(OrderedDict):
    """One trainer's captured launch sequences (``torch.cuda.CUDAGraph``) by graph key, least recently replayed first."""

    def __init__(self, device):
        super().__init__()
        self.device = device

    def drop_all(self) -> None:
        """Forget every graph (the buffers they hold addresses of are going away)."""
        if self:
            torch.cuda.synchronize(self.device)      # (a replay may still be in flight on the stream)
            self.clear()

    def lookup(self, key: tuple):
        g = self.get(key)
        if g is not None:
            self.move_to_end(key)
        return g

    def capture(self, key: tuple, enqueue: Callable[[], None], rollback: Callable[[], None], limit: int, may_fail: bool):
        """Warm-up launch outside capture (module load, lazy init, RCCL communicator), then the same sequence captured, with
        ``rollback()`` after each; the graph goes into the cache, which then evicts down to ``limit`` entries.  ``may_fail``: a
        capture that raises is survived -- capture mode ended, state rolled back, cache emptied, None returned."""
        enqueue()
        torch.cuda.synchronize(self.device)
        rollback()
        g = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(g):
                enqueue()
        except Exception as e:                     # noqa: BLE001
            if not may_fail:
                raise
            warnings.warn(f"hipGraph capture of the data-parallel step failed ({type(e).__name__}: {e}); "
                          f"continuing with eager launches")
            try:                                   # (a failed capture may leave the stream in capture mode: end it)
                if torch.cuda.is_current_stream_capturing():
                    g.capture_end()
            except Exception:                      # noqa: BLE001
                pass
            torch.cuda.synchronize(self.device)
            rollback()
            self.clear()
            return None
        rollback()
        self[key] = g
        while len(self) > limit:
            torch.cuda.synchronize(self.device)      # (its last replay may still be in flight on the stream)
            self.popitem(last=False)
        return g


class GATResTrainer(EpochLoop, FitLoop, GradFlow):
    """Owns the static buffers of one (model, topology, batch size) and runs training steps on them.

    ``step(x, y)`` draws a fresh device-side mask; ``step(x, y, mask=...)`` uses the caller's mask (bool/uint8 [N]),
    e.g. one produced by the reference's host sampler, for bit-for-bit comparable runs."""

    def __init__(self, model: GATResMeanConv, edge_index: torch.Tensor, num_nodes: int,
                 nodes_per_graph: Optional[Sequence[int]] = None, lr: float = 5e-4, weight_decay: float = 6e-6,
                 betas=(0.9, 0.999), eps: float = 1e-8, mask_rate: float = 0.95, seed: int = 0,
                 process_group=None, use_graph: bool = True, fused: bool = True,
                 force_collective_path: bool = False, targets_are_inputs: bool = False,
                 blocks_per_bucket: int = 5, use_gradient_clipping: bool = False, percentile: float = 10.0,
                 grad_history_capacity: int = 1 << 16, criterion: str = "mse",
                 _share_state_with: Optional["GATResTrainer"] = None):
        """``use_gradient_clipping`` / ``percentile``: the reference's ``--use_gradient_clipping True --percentile p``
        (train.py:611-617): AutoClip in front of every Adam update -- the gradient is clipped to the p-th percentile of all
        gradient norms seen so far (``grad_norm_history()``).  ``grad_history_capacity``: entries the device history holds
        before it is grown.

        ``criterion``: the reference's ``--criterion`` (train.py:354-368) -- ``"mse"`` (nn.MSELoss), ``"mae"`` (nn.L1Loss) or
        ``"sce"`` (evaluation.sce_loss), over the masked nodes; every step entry point trains with it and ``loss`` is its
        value.  Fixed for the trainer's lifetime (``criterion`` is read-only)."""
        if criterion not in _CRITERION_FLAGS:
            raise ValueError(f"criterion must be one of {sorted(_CRITERION_FLAGS)} (got {criterion!r})")
        self._criterion = criterion
        self.lib = _native.load()
        if not 0.0 <= float(percentile) <= 100.0:
            raise ValueError(f"percentile must lie in [0, 100] (got {percentile})")
        self.model = model
        params = model.flat_parameters
        if not params.is_cuda:
            raise ValueError("move the model to the ROCm device first; this engine has no CPU path")
        dev = params.device
        self.device = dev
        self.plan: GraphPlan = GraphPlan(edge_index, num_nodes, device=dev, segments=fused)
        self.fused = bool(fused and self.lib.gatres_fused_supported(model._cmodel_ref(), self.plan.ref()))
        # the plan struct this trainer's launches take: with the part tables of this model's split on the fused path
        self._gstruct = self.plan.bound(model._cmodel_ref()) if self.fused else self.plan.c
        N = num_nodes
        self.N = N
        self.P = params.numel()
        f32 = dict(dtype=torch.float32, device=dev)
        self.grads = torch.zeros(self.P, **f32)
        self.hparams = dict(lr=lr, weight_decay=weight_decay, beta1=betas[0], beta2=betas[1], eps=eps)
        if _share_state_with is not None:            # a sibling trainer for another batch size: ONE optimizer state
            self.exp_avg, self.exp_avg_sq = _share_state_with.exp_avg, _share_state_with.exp_avg_sq
            self.step_counter = _share_state_with.step_counter
            self.hp = _share_state_with.hp
            # ... and ONE host copy of the hyper-parameters beside the one device buffer: set_hparams() on either trainer
            # is seen by both (a sibling's set_lr left the parent's host copy stale, and the parent's next
            # set_hparams(weight_decay=...) pushed the old lr back)
            self.hparams = _share_state_with.hparams
            self._clip = _share_state_with._clip             # ... and ONE gradient-norm history
        else:
            self.exp_avg = torch.zeros(self.P, **f32)
            self.exp_avg_sq = torch.zeros(self.P, **f32)
            self.step_counter = torch.zeros(2, dtype=torch.int64, device=dev)
            # the hyper-parameters the update kernels read (gatres_train_step_t.hparams): a captured step follows
            # set_lr() without being captured again
            self.hp = torch.tensor(self._hp_list(), dtype=torch.float64, device=dev)
            self._clip = _AutoClipState(percentile, self.P, dev, grad_history_capacity) if use_gradient_clipping else None
        self._clip_gen = self._clip.generation if self._clip is not None else 0
        self.x = torch.zeros(N, **f32)
        # targets_are_inputs: the reference's snapshots have data.y == data.x until the loop masks x (train.py:162-166),
        # and the masking happens inside the kernels here (x itself is never overwritten): one buffer serves both
        self.targets_are_inputs = bool(targets_are_inputs)
        self.y = self.x if self.targets_are_inputs else torch.zeros(N, **f32)
        self.mask = torch.zeros(N, dtype=torch.uint8, device=dev)         # the mask of the step that ran last / is staged
        self._mask_spare = torch.zeros(N, dtype=torch.uint8, device=dev)  # where the update launch samples the NEXT step's mask
        self.out = torch.zeros(N, **f32)
        self.g_out = torch.zeros(N, **f32)
        self.loss = torch.zeros(1, **f32)
        self.saved = torch.empty(model._saved_floats(self.plan), **f32)
        self.scratch = model._scratch_for(self.plan)
        self.node_ptr = self.plan.node_ptr_for(nodes_per_graph) if nodes_per_graph is not None else None
        self.num_graphs = len(nodes_per_graph) if nodes_per_graph is not None else 0
        self._npg_list = [int(n) for n in nodes_per_graph] if nodes_per_graph is not None else None
        self.pg = process_group
        self.world, self.rank = 1, 0
        if process_group is not None or (torch.distributed.is_available() and torch.distributed.is_initialized()):
            self.world = torch.distributed.get_world_size(process_group)
            self.rank = torch.distributed.get_rank(process_group)
        # every rank draws its own masks (its shard holds different snapshots): the rank is mixed into the sampler's seed
        self.mask_rate, self.seed = mask_rate, int(seed) * max(self.world, 1) + self.rank
        # force_collective_path: run the multi-GPU sequence (backward | all-reduce | Adam) even at world size 1
        self.split = force_collective_path or self.world > 1
        if self.world > 1 and _share_state_with is None:
            dp.broadcast_params_(params, src=0, group=process_group)      # identical replicas, whatever each rank initialised
        self.reducer = dp.BucketedAllReduce(self.grads, process_group, force=force_collective_path) if self.split else None
        self.blocks_per_bucket = int(blocks_per_bucket)
        # Gradient buckets of the fused path's data-parallel step.  1 (default): the single-GPU step's own launches (window
        # kernel, parameter gradients, slab sum) + ONE all-reduce of the flat gradient + the Adam launch.  2: the backward chain,
        # then the parameter gradients of the upper and of the lower blocks as range launches, the first bucket on the wire
        # under the second launch (DESIGN.md section 5 has the measured cost of either form on one GPU).
        self.fused_buckets = 1
        self.epoch_graph_steps = 20          # fit_epoch: full batches per captured launch sequence; 1 = step by step
        self.epoch_copy_limit_bytes = 16 << 30   # fit_epoch trains on a shuffled device copy of the store up to this size (else: steps_rows)
        self._max_graphs = MAX_CACHED_GRAPHS
        # Multi-rank steps run as EAGER launch sequences unless GATRES_DP_GRAPH=1: a captured step would hold the RCCL
        # all-reduce, which has only ever been captured with a one-rank group here (no multi-GPU box is reachable), and
        # eager costs nothing on this path (one-rank nccl group, gatres_small bs 32: 0.428 ms/step eager vs 0.432 captured;
        # the step is a handful of native launch sequences, far from host-bound).  One-rank groups (force_collective_path)
        # keep the capture, so the in-graph form stays tested.
        self.use_graph = use_graph and (self.world <= 1 or os.environ.get("GATRES_DP_GRAPH") == "1")
        self._graphs = _GraphCache(dev)
        self._params_ptr = params.data_ptr()
        self._wt_sig = None
        self._siblings: Dict[int, "GATResTrainer"] = {}
        off = self.lib.gatres_fused_status_offset(model._cmodel_ref(), self.plan.ref()) if self.fused else -1
        self._status = self.scratch[off:off + 4].view(torch.int32) if off >= 0 else None
        # Single-GPU fused step: the update launch samples the NEXT step's device mask into the spare buffer
        # (GATRES_FLAG_MASK_NEXT); a step that finds it still valid swaps the buffers and leaves the sampler's launch out.
        # self.mask always is the mask of the step that ran last.  _mask_sig: what the spare buffer's mask was sampled for.
        # (only where the parameter gradients fold: their launch leaves the step count / fault snapshot the sampling tail
        #  reads -- models of nc 4 / 8 form them with param_grads_kernel and keep the sampler's own launch)
        # (the data-parallel step -- one gradient bucket -- does the same from its Adam launch, gatres_adam_step_ex)
        self._mask_next = bool(self.fused and self.node_ptr is not None
                               and self.lib.gatres_fused_finish_folds(model._cmodel_ref(), self.plan.ref())
                               and not os.environ.get("GATRES_NO_MASK_NEXT"))
        self._mask_sig = None
        self._bound: list = []                      # bind_batches(): (x, y) tensors the captured steps read directly
        # the fused path's parameter gradients can be formed range by range (a bucket's all-reduce starts in between)
        self._ranges = bool(self.fused and self.lib.gatres_fused_finish_folds(model._cmodel_ref(), self.plan.ref()))
        self._faults_seen = 0
        # fit_epoch(device_metrics=True): the moment table, its cursor and the descale affine while such an epoch runs (None
        # otherwise: then no launch and no graph key changes)
        self._metrics: Optional[dict] = None
        self._metrics_table = self._metrics_cursor = None      # ... and what backs it, kept from epoch to epoch
        # allocated on first use: prefetch_batch()'s two staging slots, their side stream and events; steps_rows()'s row window
        # and loss vector; the in-place epoch's buffer, its batch views and loss vector; fit()'s buffers
        self._stage = self._copy_stream = self._ready = self._free = None
        self._slot_in = self._slot_out = 0
        self._rows_win = self._loss_seq = None
        self._epoch_buf = self._epoch_bound = self._epoch_losses = None
        self._fit: Optional[dict] = None
        self._grad_flow_out: Optional[torch.Tensor] = None      # gradient_flow()'s output buffer
        self._grad_flow_names: Optional[list] = None          # ... and its names (named_parameters() is walked once)
        # the trainer that ran the last step of the last fit_epoch: a sibling, or None for this one (no reference to itself:
        # a trainer's buffers go when its last reference goes)
        self._last_stepper: Optional["GATResTrainer"] = None
        self._recipe = None                  # for_store() on a MultiSnapshotStore: the batch's graphs per network
        # set_sensor_layout(): the fixed sensor layout the store-fed steps train under (None: the sampler's random masks); a
        # sibling takes its parent's
        self._layout: Optional[SensorLayout] = _share_state_with._layout if _share_state_with is not None else None
        # (norm_type, std, eps) of the store the batches come from -- for_store() takes it from the store -- or None: what
        # converts set_sensor_layout(noise_std=...) from physical units into the store's
        self.store_norm: Optional[Tuple[str, Optional[float], float]] = (
            _share_state_with.store_norm if _share_state_with is not None else None)
        self._warn_if_the_chip_is_not_ours()

    @classmethod
    def for_store(cls, model: GATResMeanConv, store, batch_size: int, graphs_per_network: Optional[Sequence[int]] = None,
                  **kw) -> "GATResTrainer":
        """The trainer of ``fit_epoch(store)`` / ``fit(store, ...)`` for batches of ``batch_size`` graphs: ``edge_index``, node
        count and per-graph node counts come from the store, targets are the inputs.  ``store``: a ``SnapshotStore`` or a
        ``MultiSnapshotStore`` -- for the latter the batch's composition is the store's default recipe (proportional to the
        networks' snapshot counts) or ``graphs_per_network``.  ``kw``: the constructor's other arguments."""
        from .multi_snapshot_store import MultiSnapshotStore
        kw.setdefault("targets_are_inputs", True)
        if isinstance(store, MultiSnapshotStore):
            recipe = store.recipe(batch_size, graphs_per_network)
            t = cls(model, store.edge_index(recipe), store.num_nodes(recipe), nodes_per_graph=store.nodes_per_graph(recipe), **kw)
            t._recipe = recipe
            return t
        if graphs_per_network is not None:
            raise ValueError("graphs_per_network belongs to a MultiSnapshotStore")
        bs = int(batch_size)
        t = cls(model, store.edge_index(bs), bs * store.nodes_per_graph, nodes_per_graph=[store.nodes_per_graph] * bs, **kw)
        t.store_norm = (store.norm_type, store.std, store.eps)
        return t

    def _warn_if_the_chip_is_not_ours(self) -> None:
        """A split launch (several workgroups per snapshot, spin-waiting on each other's granules) needs EVERY workgroup of
        its grid resident at once, one per CU.  The native library sizes the split from the device's CU count; what it cannot
        see is a CU mask or other work on the device.  A partner that never gets a CU costs a DROPPED step (counted in
        ``fault_count``), never a wrong one -- but a trainer that silently skips updates is not what anyone wants: say so at
        construction, and let ``check_no_dropped_steps()`` (called by ``fit_epoch`` and by bench.py) turn drops into an error."""
        if not self.fused:
            return
        cus = int(self.lib.gatres_fused_cus_per_segment(self.model._cmodel_ref(), self.plan.ref()))
        if cus < 2:
            return
        padded = ((self.plan.num_segments + 7) // 8) * 8
        need = padded * cus
        have = int(torch.cuda.get_device_properties(self.device).multi_processor_count)
        if need > have and ((padded // 2 + 7) // 8) * 8 * cus <= have:
            need = ((padded // 2 + 7) // 8) * 8 * cus       # (batches of 49 - 96 snapshots go in two rounds of half the segments)
        masked = [k for k in ("HSA_CU_MASK", "ROC_GLOBAL_CU_MASK") if os.environ.get(k)]
        if need > have or masked:
            warnings.warn(f"GATResTrainer: the per-snapshot kernel launches {need} co-resident workgroups (one per CU, {cus} per "
                          f"snapshot) on a device that reports {have} CUs"
                          + (f" under {', '.join(masked)}" if masked else "") +
                          "; workgroups that cannot be resident together time out and the step is DROPPED (fault_count). "
                          "Set GATRES_FUSED_SPLIT to fewer parts per snapshot or use fused=False.", RuntimeWarning, stacklevel=3)

    def check_no_dropped_steps(self, _counts: Optional[Tuple[int, int]] = None) -> None:
        """Raise if any step was dropped since the last call (a split launch that timed out waiting for a partner workgroup,
        or a data-parallel step whose all-reduced gradient carried a fault mark).  Synchronises (``_counts``: the caller has
        read ``(fault_count, dropped_steps)`` already)."""
        faults, dropped = (self.fault_count, self.dropped_steps) if _counts is None else _counts
        n = faults + dropped
        new, self._faults_seen = n - self._faults_seen, n
        if new > 0:
            raise RuntimeError(f"{new} training step(s) were DROPPED (no update): a workgroup of the per-snapshot kernel was not "
                               f"co-resident with its partners (is the GPU shared, partitioned or CU-masked?) or a replica "
                               f"faulted; fault_count={faults}, dropped_steps={dropped}")

    # ------------------------------------------------------------------------------------------
    def _hp_list(self):
        h = self.hparams
        return [h["lr"], h["beta1"], h["beta2"], h["eps"], h["weight_decay"]]

    def _push_hparams(self) -> None:
        """Host values -> the device buffer (one small stream-ordered copy; never inside a capture)."""
        self.hp.copy_(torch.tensor(self._hp_list(), dtype=torch.float64), non_blocking=False)

    def _desc(self, phases: int, device_mask: bool, wt_valid: bool = False, flags: int = 0, block_lo: int = 0,
              block_hi: int = 0, batch=None, masks=None, loss=None) -> _TrainStepC:
        m = self.model
        bx, by = (self.x, self.y) if batch is None else batch
        mask, mask_next = (self.mask, self._mask_spare) if masks is None else masks
        params = m.flat_parameters
        if params.data_ptr() != self._params_ptr:
            raise RuntimeError("the model's parameter storage moved (e.g. .to()/deepcopy); build a new GATResTrainer")
        h = self.hparams
        return _TrainStepC(
            _native.GatresModel(m.num_blocks, m.nc, m._cmodel.act_dtype, 0), C.pointer(self._gstruct), params.data_ptr(), self.grads.data_ptr(),
            self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), self.step_counter.data_ptr(), bx.data_ptr(),
            by.data_ptr(), mask.data_ptr(),
            self.node_ptr.data_ptr() if (device_mask and self.node_ptr is not None) else None,
            self.num_graphs, phases, self.mask_rate, self.seed, self.out.data_ptr(), self.g_out.data_ptr(),
            (self.loss if loss is None else loss).data_ptr(), self.saved.data_ptr(), self.scratch.data_ptr(), h["lr"], h["beta1"], h["beta2"],
            h["eps"], h["weight_decay"], 1.0 / self.world,
            (0 if self.fused else FLAG_PER_OP) | (FLAG_WT_VALID if wt_valid else 0) | _CRITERION_FLAGS[self._criterion] | flags,
            self.hp.data_ptr(),
            block_lo, block_hi, mask_next.data_ptr(), C.pointer(self._clip.c) if self._clip is not None else None)

    def _count_native_update(self, n: int = 1) -> None:
        """A native kernel (fused Adam pass, Adam-only phase) just changed the parameters without touching torch's
        version counters.  The count lives on the MODEL: trainers that share it (``fit_epoch``'s sibling for the ragged
        last batch, a trainer per batch size) each keep transposed conv weights in their OWN scratch buffer, and a step
        of one must invalidate the copies of the others (the sibling's step left the main trainer's W^T one
        update behind while its signature still matched)."""
        self.model._native_updates += n

    def _committed(self, updates: int = 0, wt: Optional[bool] = None, mask_ahead: Optional[bool] = None,
                   swap: bool = False) -> None:
        """The ledger of what launches left behind -- with ``_unknown`` the only writer of these facts.  ``updates`` native updates
        ran to completion; ``swap``: the two mask buffers traded places an odd number of times; ``wt``: scratch holds / does not
        hold the transposes of the current weights; ``mask_ahead``: the spare buffer holds / does not hold the next step's mask
        (None: that fact stays as it was)."""
        if updates:
            self._count_native_update(updates)
        if swap:
            self.mask, self._mask_spare = self._mask_spare, self.mask
        if wt is not None:
            self._wt_sig = self._param_signature() if wt else None
        if mask_ahead is not None:
            self._mask_sig = self._mask_key() if mask_ahead else None

    def _unknown(self) -> None:
        """An unknown part of a launch sequence ran (it raised), or the training state was replaced under the trainer: siblings
        must not trust their transposed weights (one update is counted), and neither scratch's transposes nor a mask sampled
        ahead is taken for current -- the next step samples its own mask and re-derives the transposes."""
        self._committed(1, wt=False, mask_ahead=False)

    def _param_signature(self) -> Tuple[int, int, int]:
        """Changes whenever anything wrote to the parameters THROUGH TORCH: the flat vector or any of the nn.Parameters
        that are views of it (every Parameter has its own version counter: ``load_state_dict``, ``torch.optim`` steps,
        ``init_`` / ``clip_`` calls bump those, not the flat vector's).  Writes that bypass autograd's bookkeeping
        (``p.data.mul_()``) are invisible to it: call ``invalidate_weights()`` after such an edit."""
        return (self.model.flat_parameters._version, sum(p._version for p in self.model._param_list),
                self.model._native_updates)

    def _wt_current(self) -> bool:
        """scratch's transposed conv weights are current: our last fused Adam step wrote them and nothing has modified
        the parameters since (our kernels do not go through torch, so they leave the signature alone)."""
        return self._wt_sig is not None and self._wt_sig == self._param_signature()

    def invalidate_weights(self) -> None:
        """The parameters were edited behind torch's back: re-derive the transposed weights at the next step."""
        self._committed(wt=False)

    def set_lr(self, lr: float) -> None:
        """Learning-rate schedules (the reference runs ReduceLROnPlateau, train.py:349-350,510).  The update kernels read
        the hyper-parameters from a device buffer (``gatres_train_step_t.hparams``), so the captured step is NOT captured
        again: the new value is one 40-byte copy in stream order."""
        self.set_hparams(lr=lr)

    def set_hparams(self, **kw) -> None:
        changed = False
        for k, v in kw.items():
            if k == "mask_rate":
                self.mask_rate = float(v)
            elif k in self.hparams:
                changed = changed or self.hparams[k] != float(v)
                self.hparams[k] = float(v)
            else:
                raise KeyError(k)
        if changed:
            self._push_hparams()                       # (siblings share both the dict and the device buffer)

    # ---- fine-tuning to a fixed sensor layout -----------------------------------------------------------------------------
    def set_sensor_layout(self, observed_idx: Sequence[int], *, sensor_dropout: float = 0.0, layout_share: float = 1.0,
                          noise_std=None, noise_seed: Optional[int] = None) -> None:
        """Train the store-fed steps (``step_rows``, ``steps_rows``, ``fit_epoch``, ``fit``) under the mask of a FIXED sensor
        layout: every node hidden but ``observed_idx`` (node indices inside a graph, distinct -- the layout of a
        ``PressureEstimator``).  Per step and graph, each sensor loses its reading with probability ``sensor_dropout`` (in
        ``[0, 1)``; a graph may lose all of them: it then trains all-hidden), and with probability ``1 - layout_share`` the graph
        takes the sampler's random mask of ``mask_rate`` instead, so that the model keeps the general task.  The batch is staged
        by ``gatres_stage_rows_mask_sensors`` -- collation and mask in one launch, as without a layout; the step's own launches
        are untouched.  The indices are uploaded once, here.  ``sensor_layout_draws(self.seed, step, ...)`` restates the draws.

        While a layout is set the epoch goes through the row-gather steps (the in-place epoch has no staging launch), and the
        calls that would train under the sampler's mask alone raise ``ValueError``: ``step(x, y)`` without a mask,
        ``run_step(device_mask=True)``, ``step_prefetched``, ``bind_batches`` / ``step_bound`` / ``steps_bound``.
        ``step(x, y, mask)`` with the caller's mask stays.  Siblings (the ragged batch's trainer) follow.  Data parallelism and a
        ``MultiSnapshotStore`` are refused (``NotImplementedError``).

        ``noise_std`` (``None`` or all zeros: today's launch and today's bits): measurement noise on the readings.  One
        non-negative finite number, or one per sensor, in PHYSICAL units.  A sensor that keeps its reading in a layout-mode
        graph is then staged as ``r + sigma[k] * z`` -- ``sigma`` is ``noise_std`` in the store's units (divided by ``std + eps``
        for a z-normalised store; ``store_norm``, which ``for_store`` takes from the store, says which: without it ``noise_std``
        is refused), uploaded once, here; ``z = sensor_layout_noise(noise_seed, step, rows, K)[g, k]`` is drawn in the batch's own
        staging launch (``gatres_stage_rows_mask_sensors_noisy``) from the optimizer's step count, read on the device, so every
        step of a captured sequence draws its own noise.  No launch, read-back or per-step tensor is added.  Dropped sensors,
        random-mode graphs and the targets stay clean: the noise sits where ``mask == 0`` and the loss reads its target where
        ``mask == 1``, so a trainer whose targets ARE its inputs trains on clean targets.  ``noise_seed`` (an integer in
        ``[0, 2**64)``) defaults to the trainer's effective seed.  Whatever a layout refuses, noise refuses with it."""
        refuse_layout_data_parallel(self.world)
        if self._recipe is not None:
            raise NotImplementedError("a sensor layout with a MultiSnapshotStore is not implemented (a layout per network would "
                                      "be needed): fine-tune on one network's SnapshotStore")
        if self.node_ptr is None or not self._npg_list or len(set(self._npg_list)) != 1:
            raise ValueError("a sensor layout needs nodes_per_graph at construction, the same for every graph of the batch")
        if noise_std is not None and noise_seed is None:
            noise_seed = int(self.seed) & 0xFFFFFFFFFFFFFFFF
        self._adopt_layout(SensorLayout(observed_idx, self._npg_list[0], sensor_dropout, layout_share, self.device,
                                        noise_std=noise_std, noise_seed=noise_seed, norm=getattr(self, "store_norm", None)))

    def clear_sensor_layout(self) -> None:
        """Back to the sampler's random masks: every path, graph key and launch is the one of a trainer that never had a layout."""
        self._adopt_layout(None)

    def _adopt_layout(self, layout: Optional[SensorLayout]) -> None:
        for t in [self] + list(self._siblings.values()):
            t._layout = layout
            t._committed(mask_ahead=False)      # (a mask sampled ahead belongs to the setting that was replaced)

    @property
    def sensor_layout(self) -> Optional[dict]:
        """``{"observed_idx", "sensor_dropout", "layout_share"}`` of the layout set (a copy), or None; under measurement noise
        also ``"noise_std"`` (K floats, physical units) and ``"noise_seed"``."""
        return None if self._layout is None else self._layout.describe()

    def _refuse_under_layout(self, what: str) -> None:
        if self._layout is not None:
            raise ValueError(f"{what} would train under the sampler's random mask, not under the sensor layout that is set: use "
                             f"step_rows / steps_rows / fit_epoch / fit, pass a mask of your own, or clear_sensor_layout()")

    def _graph_key(self, what, device_mask: bool, wt_valid: bool) -> tuple:
        # (no hyper-parameter in here: the kernels read them from self.hp; which of the two mask buffers is current is)
        return (what, device_mask, wt_valid, self.mask_rate, self.seed, self.world, self.mask.data_ptr())

    def _take_mask_ahead(self) -> bool:
        """If the previous step's update launch sampled THIS step's mask and nothing has moved since, make that buffer the
        current one (True); else the caller samples / stages a mask into self.mask as before."""
        taken = self._mask_next and self._mask_current()
        self._committed(mask_ahead=False, swap=taken)
        return taken

    @property
    def criterion(self) -> str:
        """The training criterion this trainer's steps use: ``"mse"``, ``"mae"`` or ``"sce"`` (fixed at construction)."""
        return self._criterion

    @property
    def num_captured_graphs(self) -> int:
        return len(self._graphs)

    @property
    def dropped_steps(self) -> int:
        """Data-parallel steps whose update was skipped because the all-reduced gradient carried a fault mark -- the mark is
        "entry 0 is NaN", so a diverging run that puts a NaN there shows up here too (it would otherwise freeze silently:
        ADVICE r3).  Synchronises."""
        return int(self._status[STATUS_DROPPED_STEPS].item()) if self._status is not None else 0

    @property
    def fault_count(self) -> int:
        """Split launches that gave up waiting for a partner workgroup so far (each cost exactly one dropped step: loss
        NaN, no update).  Synchronises."""
        return int(self._status[STATUS_FAULT_COUNT].item()) if self._status is not None else 0

    def _enqueue(self, phases: int, device_mask: bool, wt_valid: bool = False, flags: int = 0, block_lo: int = 0,
                 block_hi: int = 0, batch=None, masks=None, loss=None) -> None:
        if self._clip is not None and (phases & PHASE_ADAM) and not torch.cuda.is_current_stream_capturing():
            self._clip.reserve(1)        # (a direct call; the step paths reserve for their replays too: a bound, not a count)
        ts = self._desc(phases, device_mask, wt_valid, flags, block_lo, block_hi, batch, masks, loss)
        _native.check(self.lib.gatres_train_step(C.byref(ts), _native.current_stream(self.device)),
                      "gatres_train_step")
        if self._metrics is not None and (phases & PHASE_FORWARD):
            self._enqueue_metrics(batch, masks)

    def _enqueue_metrics(self, batch=None, masks=None) -> None:
        """The masked-metric moments of the step just enqueued (fit_epoch(device_metrics=True)): ``out`` is written by its
        forward and the step's mask is still in place -- the update launch samples the NEXT step's mask into the other buffer,
        and in a captured sequence the step after this one overwrites it only in its own update launch.  The record goes to
        the slot the table's device cursor names; the kernel advances the cursor, so replayed sequences and the sibling
        trainer of the ragged batch write consecutive slots."""
        met = self._metrics
        by = self.y if batch is None else batch[1]
        mask = self.mask if masks is None else masks[0]
        _native.check(self.lib.gatres_masked_metrics(
            self.out.data_ptr(), by.data_ptr(), mask.data_ptr(), self.N, met["scale"], met["offset"], met["table"].data_ptr(),
            0, met["table"].shape[0], met["cursor"].data_ptr(), _native.current_stream(self.device)), "gatres_masked_metrics")

    def _mask_key(self):
        """What a mask sampled by the update launch is valid for: the optimizer state as this trainer left it (a sibling's or a
        FusedAdam step moves the shared step count: the sampler's key would differ) and the sampler's own settings."""
        return (self.model._native_updates, self.mask_rate, self.seed)

    def _mask_current(self) -> bool:
        """The spare buffer holds the next step's mask: an update launch sampled it and nothing has moved since."""
        return self._mask_sig is not None and self._mask_sig == self._mask_key()

    def _step(self, device_mask: bool, premasked: bool = False, batch=None, slot=None) -> None:
        """THE step runner: one optimisation step on ``batch`` (default: the static buffers) -- [mask sampler,] forward, loss,
        backward, Adam as one launch on a single GPU; backward pieces | bucketed all-reduce | Adam under data parallelism, which
        with one gradient bucket on the fused path is the single-GPU step's launch sequence with the slab sum and the update as
        two launches around ONE all-reduce.  ``premasked``: the step's mask is in ``self.mask`` already, staged with the batch --
        such a caller samples every step's mask itself, so the update launch does not sample the next one.  Otherwise, where
        the update launch can (``_mask_next``; data parallel: one gradient bucket), it samples the NEXT step's mask, and a step
        that finds that mask still valid leaves the sampler's launch out.  ``slot`` names ``batch`` in the graph key."""
        if device_mask and self.node_ptr is None:
            raise ValueError("device mask sampling needs nodes_per_graph at construction")
        # (fused path: the Adam pass / Adam-only phase leaves the transposed conv weights of the NEW parameters in scratch)
        wt_valid = self.fused and self._wt_current()
        ahead = bool(not premasked and device_mask and self._mask_next and (not self.split or self._one_piece()))
        if ahead and self._take_mask_ahead():
            premasked = True                       # the previous step's update launch has sampled this step's mask already
        flags = FLAG_MASK_NEXT if ahead else 0
        if self.split:
            what = ("split", premasked, flags, slot)

            def enqueue():
                dp.run_data_parallel_step(self._backward_pieces(device_mask, wt_valid, premasked, batch, flags), self.reducer,
                                          lambda: self._enqueue(PHASE_ADAM, device_mask, flags=flags))
        else:
            phases = _STEP if premasked else PHASE_MASK | _STEP
            what = (phases, flags, slot)

            def enqueue():
                self._enqueue(phases, device_mask, wt_valid, flags=flags, batch=batch)
        self._launch(self._graph_key(what, device_mask, wt_valid), enqueue, wt_valid, 1, wt=self.fused, mask_ahead=ahead)

    def _launch(self, key: tuple, enqueue: Callable[[], None], wt_valid: bool, updates: int, wt: bool, mask_ahead: bool,
                swap: bool = False) -> None:
        """What every runner does around its launch sequence of ``updates`` steps: room in the gradient-norm history, ``_replay``,
        and the ledger -- ``_committed`` with the facts the sequence establishes, ``_unknown`` if it raised."""
        if self._clip is not None:
            self._clip.reserve(updates)
        try:
            self._replay(key, enqueue, wt_valid)
        except BaseException:
            self._unknown()
            raise
        self._committed(updates, wt, mask_ahead, swap)

    def _prepare_backward(self) -> None:
        """Derive scratch's transposed conv weights from the parameters as they are now (the promise behind ``wt_valid``)."""
        _native.check(self.lib.gatres_fused_prepare_backward(
            self.model._cmodel_ref(), C.byref(self._gstruct), self.model.flat_parameters.data_ptr(),
            self.scratch.data_ptr(), _native.current_stream(self.device)), "gatres_fused_prepare_backward")

    def _training_state(self) -> list:
        return [self.step_counter, self.model.flat_parameters, self.exp_avg, self.exp_avg_sq]

    def _replay(self, key: tuple, enqueue: Callable[[], None], wt_valid: bool = False) -> None:
        """Run ``enqueue`` -- eagerly, or captured once into a hipGraph (cached by ``key``) and replayed."""
        met = self._metrics
        if met is not None:            # (a step with the metrics launch is another graph than the same step without it)
            key = key + (("metrics", met["table"].data_ptr(), met["cursor"].data_ptr(), met["scale"], met["offset"]),)
        if self._layout is not None:   # (a sequence that stages under a layout holds its buffer and its probabilities)
            key = key + (self._layout.key(),)
        if not self.use_graph:
            enqueue()
            return
        if self._clip is not None and self._clip_gen != self._clip.generation:
            self._graphs.drop_all()      # the gradient-norm history was grown: captured steps hold the old buffers' addresses
            self._clip_gen = self._clip.generation
        g = self._graphs.lookup(key)
        if g is None:
            # the warm-up runs real steps: the training state comes back after it, with both mask buffers (a warm-up that ran the
            # sampler's launch re-sampled self.mask: same bits; a multi-step sequence samples into BOTH, two steps ahead of the
            # rollback) and the metrics cursor (the warm-up's records are overwritten by the real steps: same slots)
            rollback = _save(self._training_state() + [self.mask, self._mask_spare] + ([met["cursor"]] if met is not None else []),
                             self._clip)
            # A multi-rank step holds RCCL collectives; if this runtime cannot capture them (every rank fails the same way: the
            # sequence is identical), run the launch sequence eagerly from here on instead of dying.  Single-rank captures hold
            # only this library's kernels: a failure there is a bug and is raised.
            g = self._graphs.capture(key, enqueue, rollback, self._max_graphs, may_fail=self.world > 1)
            if wt_valid:
                # the warm-up step left the transposes of ITS updated weights in scratch; the parameters were rolled back, so
                # make the promise this sequence relies on true again
                self._prepare_backward()
            if g is None:
                self.use_graph = False
                enqueue()
                return
        if self.fused:
            # a captured split launch cannot order itself behind one on another stream (include/gatres.h)
            _native.check(self.lib.gatres_fused_serialize(_native.current_stream(self.device)), "gatres_fused_serialize")
        g.replay()

    # ---- the multi-rank step: backward pieces | bucketed all-reduce | Adam, as ONE launch sequence / hipGraph ---------
    def _one_piece(self) -> bool:
        """The fused data-parallel step as ONE gradient bucket (the single-GPU step's own launches in front of the all-reduce)."""
        return self.fused and (not self._ranges or self.model.num_blocks < 2 or self.fused_buckets < 2)

    def _backward_pieces(self, device_mask: bool, wt_valid: bool, premasked: bool = False, batch=None, flags: int = 0):
        """Pieces for ``dp.run_data_parallel_step``.  Fused path (gatres_small): one piece -- mask, forward, loss and the
        whole backward are a single launch whose gradient exists only after the slab reduction that ends it.  Per-op
        path (gatres_large, large graphs): forward, then one piece per ``blocks_per_bucket`` blocks in reverse order,
        each ending with the slab reduction of exactly its parameters."""
        if self.fused:
            m = self.model
            head = (0 if premasked else PHASE_MASK) | PHASE_FORWARD | PHASE_BACKWARD
            if self._one_piece():
                # (flags: GATRES_FLAG_MASK_NEXT makes the parameter-gradient launch leave the step-count snapshot that the
                #  Adam launch's sampling tail reads)
                def whole():
                    self._enqueue(head, device_mask, wt_valid, flags=flags, batch=batch)
                    return 0, self.P
                return [whole]
            # Two pieces: the backward chain + the parameter gradients of the UPPER blocks (whose bucket closes the flat
            # vector: it carries lin1), then the lower blocks (+ lin0).  The first bucket's all-reduce runs on the process
            # group's stream while the second launch forms the rest of the gradient ("a single bucket launched
            # after the last K1b and hidden behind ..."): 130 KB on the wire under ~19 us of kernel.
            k = m.num_blocks // 2
            cut = 2 * m.nc + k * (9 * m.nc + 4 * m.nc * m.nc)

            def upper():
                self._enqueue(head, device_mask, wt_valid, flags=FLAG_GRADS_DEFERRED, batch=batch)
                self._enqueue(PHASE_BACKWARD, device_mask, flags=FLAG_GRADS_ONLY, block_lo=k, block_hi=m.num_blocks)
                return cut, self.P

            def lower():
                self._enqueue(PHASE_BACKWARD, device_mask, flags=FLAG_GRADS_ONLY, block_lo=0, block_hi=k)
                return 0, cut
            return [upper, lower]
        m = self.model
        pieces = []
        bx = self.x if batch is None else batch[0]
        for k, (b_hi, b_lo, lo, hi) in enumerate(dp.block_buckets(m.num_blocks, m.nc, self.blocks_per_bucket)):
            def piece(k=k, b_hi=b_hi, b_lo=b_lo, lo=lo, hi=hi):
                if k == 0:
                    self._enqueue((0 if premasked else PHASE_MASK) | PHASE_FORWARD, device_mask, batch=batch)
                flags = PART_REDUCE | (PART_FIRST if b_hi == m.num_blocks else 0) | (PART_LAST if b_lo == 0 else 0)
                _native.check(self.lib.gatres_model_backward_per_op_part(
                    m._cmodel_ref(), C.byref(self._gstruct), m.flat_parameters.data_ptr(), bx.data_ptr(),
                    self.mask.data_ptr(), self.g_out.data_ptr(), self.saved.data_ptr(), self.scratch.data_ptr(),
                    self.grads.data_ptr(), None, b_hi, b_lo, flags, _native.current_stream(self.device)),
                    "gatres_model_backward_per_op_part")
                return lo, hi
            pieces.append(piece)
        return pieces

    # ------------------------------------------------------------------------------------------
    def load_batch(self, x: torch.Tensor, y: torch.Tensor, mask: Optional[torch.Tensor] = None) -> None:
        """Stage a batch into the static buffers (async copies on the current stream)."""
        self.x.copy_(x.reshape(-1), non_blocking=True)
        if not self.targets_are_inputs:
            self.y.copy_(y.reshape(-1), non_blocking=True)
        if mask is not None:
            self.mask.copy_(mask.reshape(-1).to(torch.uint8), non_blocking=True)
            self._committed(mask_ahead=False)    # (the caller's mask replaced whatever the update launch had sampled)

    def prefetch_batch(self, x: torch.Tensor, y: Optional[torch.Tensor] = None) -> None:
        """Start copying the NEXT batch (typically pinned host memory) into a staging buffer on a side stream, so the
        PCIe transfer overlaps the step that is running; ``commit_batch()`` then moves it into place with a device copy.
        Two staging slots: at most one prefetch may be outstanding per ``commit_batch()``."""
        if self._stage is None:
            f32 = dict(dtype=torch.float32, device=self.device)
            n = self.x.numel()
            self._stage = [(torch.empty(n, **f32), None if self.targets_are_inputs else torch.empty(n, **f32))
                           for _ in range(2)]
            self._copy_stream = torch.cuda.Stream(device=self.device)
            self._ready = [torch.cuda.Event() for _ in range(2)]
            self._free = [torch.cuda.Event() for _ in range(2)]
            for ev in self._free:
                ev.record(torch.cuda.current_stream(self.device))
        k = self._slot_in
        sx, sy = self._stage[k]
        with torch.cuda.stream(self._copy_stream):
            self._copy_stream.wait_event(self._free[k])
            sx.copy_(x.reshape(-1), non_blocking=True)
            if sy is not None:
                sy.copy_((x if y is None else y).reshape(-1), non_blocking=True)
            self._ready[k].record(self._copy_stream)
        self._slot_in = 1 - k

    def commit_batch(self) -> None:
        """Make the prefetched batch the current one (device-to-device copies on the compute stream)."""
        k = self._slot_out
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(self._ready[k])
        sx, sy = self._stage[k]
        self.x.copy_(sx, non_blocking=True)
        if sy is not None:
            self.y.copy_(sy, non_blocking=True)
        self._free[k].record(cur)
        self._slot_out = 1 - k

    def step_prefetched(self) -> torch.Tensor:
        """One optimisation step (device-sampled mask) on the prefetched batch IN PLACE: the kernels read the staging slot the
        side stream filled -- they never write x -- so there is no device copy and, with the mask sampled ahead by the previous
        update launch, no sampler launch either: the bound-batch step's three launches, the PCIe transfer of the next batch
        under them.  ``commit_batch()`` + ``run_step()`` is the same step through the static buffers (two launches more)."""
        self._refuse_under_layout("step_prefetched")
        k = self._slot_out
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(self._ready[k])
        sx, sy = self._stage[k]
        batch = (sx, sx if sy is None else sy)
        self._step_on(batch)
        self._free[k].record(cur)                  # (the slot may be refilled once this step has read it)
        self._slot_out = 1 - k
        return self.loss

    def run_step(self, device_mask: bool = True) -> None:
        """One optimisation step on the staged batch.  Nothing is synchronised; read ``self.loss`` afterwards."""
        if device_mask:
            self._refuse_under_layout("run_step(device_mask=True)")
        self._step(device_mask)

    def _stage_with_mask(self, x: torch.Tensor, y: torch.Tensor) -> bool:
        """Device-resident batch + device mask: the copy into the static buffers rides on the mask
        sampler's launch (``gatres_stage_batch_mask``) -- one small kernel and one kernel boundary less per step than
        ``load_batch`` followed by the sampler.  Returns False when the batch has to go through ``load_batch``."""
        if self.node_ptr is None or os.environ.get("GATRES_NO_STAGE_MASK"):
            return False
        n = self.x.numel()
        for t in (x, y):
            if not (t.is_cuda and t.device == self.x.device and t.dtype == torch.float32 and t.numel() == n and t.is_contiguous()):
                return False
        # (a mask the previous update launch may have sampled ahead is NOT used here: the batch needs a staging launch anyway,
        #  and copy + sampling in one launch is cheaper than a copy launch of its own -- measured 0.4204 vs 0.4237 ms/step;
        #  step_bound() / run_step() are the paths without a staging launch)
        self._committed(mask_ahead=False)
        ys = None if self.targets_are_inputs else y
        _native.check(self.lib.gatres_stage_batch_mask(
            x.data_ptr(), None if ys is None else ys.data_ptr(), self.x.data_ptr(), None if ys is None else self.y.data_ptr(), n,
            self.node_ptr.data_ptr(), self.num_graphs, self.mask_rate, self.seed, self.step_counter.data_ptr(),
            self.mask.data_ptr(), _native.current_stream(self.device)), "gatres_stage_batch_mask")
        return True

    def step_rows(self, data: torch.Tensor, rows: torch.Tensor) -> bool:
        """One step on the snapshots ``rows`` (device int64 ``[num_graphs]``) of the device-resident matrix ``data``
        ``[S, N_g]`` (a ``SnapshotStore``): the batch is collated INSIDE the mask sampler's launch
        (``gatres_stage_rows_mask``) -- no ``index_select``, no copy.  Returns False (nothing done) when this trainer
        cannot take the path (no per-graph node counts, switched off)."""
        if not (self._rows_path_ok(data) and rows.is_cuda and rows.dtype == torch.int64 and rows.numel() == self.num_graphs
                and rows.is_contiguous()):
            return False
        self._stage_rows(data, rows.data_ptr())
        self._step(True, premasked=True)
        return True

    def _rows_path_ok(self, data: torch.Tensor) -> bool:
        npg = self.N // max(self.num_graphs, 1)
        return (self.node_ptr is not None and not os.environ.get("GATRES_NO_STAGE_MASK") and data.is_cuda
                and data.device == self.x.device and data.dtype == torch.float32 and data.dim() == 2
                and data.shape[1] == npg and data.is_contiguous())

    def _stage_rows(self, data: torch.Tensor, rows_ptr: int) -> None:
        """Collate the snapshots named by the ``num_graphs`` int64 row indices at device address ``rows_ptr`` into the static
        buffers and sample the step's mask, in one launch -- under a sensor layout, the layout's mask."""
        lay = self._layout
        if lay is not None:
            _stage_rows_sensors(self.lib, data, rows_ptr, self.N // max(self.num_graphs, 1), self.x,
                                None if self.targets_are_inputs else self.y, self.node_ptr, self.num_graphs, lay.observed,
                                len(lay.observed_idx), lay.sensor_dropout, lay.layout_share, self.mask_rate, self.seed,
                                self.step_counter.data_ptr(), self.mask, _native.current_stream(self.device),
                                sigma=lay.sigma, noise_seed=lay.noise_seed or 0)
            return
        _native.check(self.lib.gatres_stage_rows_mask(
            data.data_ptr(), rows_ptr, self.N // max(self.num_graphs, 1), self.x.data_ptr(),
            None if self.targets_are_inputs else self.y.data_ptr(), self.node_ptr.data_ptr(), self.num_graphs, self.mask_rate,
            self.seed, self.step_counter.data_ptr(), self.mask.data_ptr(), _native.current_stream(self.device)),
            "gatres_stage_rows_mask")

    def _stage_multi(self, store, recipe, rows_ptr: int) -> None:
        """``_stage_rows`` for a ``MultiSnapshotStore``: the batch's graphs come from several matrices (``recipe``: how many
        of each network; ``rows_ptr``: their int64 rows, each inside its network), collated and masked in one launch."""
        _native.check(self.lib.gatres_stage_multi_rows_mask_required(
            store.table.data_ptr(), store.num_networks, store.net_of_graph(recipe).data_ptr(), rows_ptr, self.node_ptr.data_ptr(),
            self.num_graphs, self.x.data_ptr(), None if self.targets_are_inputs else self.y.data_ptr(), self.mask_rate, self.seed,
            self.step_counter.data_ptr(), None, None, self.mask.data_ptr(), _native.current_stream(self.device)),
            "gatres_stage_multi_rows_mask_required")

    def steps_rows(self, data: torch.Tensor, rows: torch.Tensor, total: Optional[torch.Tensor] = None) -> bool:
        """``step_rows`` for k consecutive batches -- ``rows`` is a device int64 ``[k * num_graphs]`` slice of an epoch's
        snapshot order -- as ONE captured launch sequence (k x [collation + mask sampler, window kernel, parameter gradients,
        update]): an epoch then pays the host's per-step work and the gap between two graph launches once per k steps.  The
        rows are copied into a window buffer the captured kernels read (5 KB per 20 steps) and step i's update launch writes
        its loss into entry i of a k-vector; every launch, and so every bit of the result, is the single calls'.  ``total``
        (float64 ``[1]``): += sum of the k losses x num_graphs -- in double, where a sum of fp32 losses is exact, so it does not
        matter that the k terms are added at once.  Steady state only (single GPU, fused path, hipGraph replay, transposed
        weights current); returns False (nothing done) otherwise."""
        bs = self.num_graphs
        k = rows.numel() // max(bs, 1)
        if not (k > 1 and rows.numel() == k * bs and self.use_graph and self.fused and not self.split and self._rows_path_ok(data)
                and rows.is_cuda and rows.dtype == torch.int64 and self._wt_current()):
            return False
        win = self._rows_win
        if win is None or win.numel() < k * bs:
            win = self._rows_win = torch.zeros(k * bs, dtype=torch.int64, device=self.device)
            self._loss_seq = torch.zeros(k, dtype=torch.float32, device=self.device)
        win[:k * bs].copy_(rows)
        lseq = self._loss_seq

        def enqueue():
            for i in range(k):
                self._stage_rows(data, win.data_ptr() + 8 * i * bs)
                self._enqueue(_STEP, True, True, flags=0, loss=lseq[i:i + 1])

        self._launch(("rowseq", k, data.data_ptr(), win.data_ptr(), lseq.data_ptr(), self.mask_rate, self.seed, self.world),
                     enqueue, True, k, wt=True, mask_ahead=False)
        self.loss.copy_(lseq[k - 1:k])                   # (the loss of the step that ran last, as after single steps)
        if total is not None:
            total.add_(lseq[:k].double().sum(), alpha=float(bs))
        return True

    def step(self, x: torch.Tensor, y: torch.Tensor, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Reference-shaped call: one iteration of train.py:159-190.  Returns the (device) loss tensor."""
        if mask is None:
            self._refuse_under_layout("step(x, y) without a mask")
        if mask is None and self._stage_with_mask(x, y):
            self._step(True, premasked=True)                                    # (the mask of this step is in place)
        else:
            self.load_batch(x, y, mask)
            self.run_step(device_mask=mask is None)
        return self.loss

    # ---- bound batches: the captured step reads the caller's buffers, nothing is copied -------------------------------------
    def bind_batches(self, xs, ys=None, precapture: bool = True, sequences=()) -> int:
        """Register device-resident batches (flat fp32 ``[N]`` tensors; ``ys`` defaults to ``xs``: y == x before masking,
        train.py:162-166) that ``step_bound(i)`` then trains on IN PLACE: the kernels mask x on the fly and never write it,
        so no staging copy is needed -- one captured step per buffer and mask-buffer orientation.  ``precapture``: capture
        every one of those steps NOW (``precapture_bound()``), so that no ``step_bound`` call ever pays for a capture.  The
        trainer keeps the tensors alive; do not resize them.  Returns the number of bound batches."""
        self._refuse_under_layout("bind_batches")
        ys = xs if ys is None else ys
        bound = []
        for x, y in zip(xs, ys):
            for t in (x, y):
                _native.require_gpu_tensor(t, "a bound batch")
                if t.numel() != self.N or t.device != self.x.device:
                    raise ValueError(f"a bound batch must hold {self.N} values on {self.x.device}")
            bound.append((x.reshape(-1), y.reshape(-1)))
        self._graphs.drop_all()                       # (captured steps of the previous binding read other buffers)
        self._bound = bound
        # two captured steps per bound batch (the two mask buffers take turns) + the first-step variants + whatever else this
        # trainer replays: the cache must hold them all, or FIFO eviction makes every step pay for a capture
        self._max_graphs = max(MAX_CACHED_GRAPHS, 2 * len(bound) + 16 + 2 * len(tuple(sequences)))
        if precapture:
            self.precapture_bound(sequences)
        return len(bound)

    def precapture_bound(self, sequences=()) -> int:
        """Capture the steady-state step of every (bound batch, mask-buffer orientation) pair by RUNNING steps, then put the
        training state back exactly where it was (parameters, Adam moments, step count) -- with the transposed weights current
        and the first step's mask sampled ahead, so that the first real ``step_bound`` call already replays a steady-state
        graph.  Nothing is captured inside a caller's timed region afterwards (bench.py's first timed block held
        four captures).  ``sequences``: tuples of bound-batch indices that the caller will run through ``steps_bound`` -- each is
        captured too, under both orientations of the mask buffers.  Under data parallelism every rank runs the same number of
        steps (the collectives match).  Returns the number of captured graphs."""
        if not (self.use_graph and self._bound and self.node_ptr is not None):
            return len(self._graphs)
        dev = self.device
        torch.cuda.synchronize(dev)
        restore = _save(self._training_state() + [self.loss], self._clip)
        try:
            n = len(self._bound)
            # (mask-ahead: the two mask buffers take turns, so a batch has two steady-state graphs; without it, one)
            ahead_ok = self._mask_next and (not self.split or self._one_piece())
            ptrs = (self.mask.data_ptr(), self._mask_spare.data_ptr()) if ahead_ok else (None,)
            need = {(i, p) for i in range(n) for p in ptrs}
            steps = 0
            while need and steps < 4 * n + 8:
                # the step about to run is a steady-state one iff the weights' transposes are current and (mask-ahead) a mask was
                # sampled ahead; it then trains with the (current) spare buffer as its mask
                steady = ((not self.fused) or self._wt_current()) and (not ahead_ok or self._mask_current())
                ptr = self._mask_spare.data_ptr() if ahead_ok and steady else None
                i = next((j for j in range(n) if (j, ptr) in need), 0)
                self.step_bound(i)
                if steady:
                    need.discard((i, ptr))
                steps += 1
            # multi-step sequences (steps_bound): each one under both start orientations of the mask buffers
            for seq in sequences:
                seq = tuple(int(i) for i in seq)
                if len(seq) < 2 or not ahead_ok or self.split:
                    continue
                seen = set()
                for _ in range(4):
                    if len(seen) == 2:
                        break
                    start = self._mask_spare.data_ptr()
                    if start in seen:
                        self.step_bound(seq[0])            # (flip the orientation)
                        continue
                    self.steps_bound(seq)
                    seen.add(start)
            self._max_graphs = max(self._max_graphs, len(self._graphs) + 16)
        finally:
            # whatever happened above (a capture or a launch may raise midway): the caller's model, moments and step count
            # come back, and neither the sampled-ahead mask nor scratch's transposed weights is taken for current
            torch.cuda.synchronize(dev)
            restore()
            self._unknown()                            # (siblings / other trainers of this model: their copies are stale too)
        if self.fused:
            # scratch holds the transposes of the LAST pre-capture step's weights: re-derive them for the restored parameters
            self._prepare_backward()
        if ahead_ok:
            # the first step's mask, sampled where the previous step's update launch would have left it (same key: same bits)
            _native.check(self.lib.gatres_mask_generate(
                self.node_ptr.data_ptr(), self.num_graphs, self.mask_rate, self.seed, self.step_counter.data_ptr(),
                self._mask_spare.data_ptr(), _native.current_stream(dev)), "gatres_mask_generate")
        self._committed(wt=self.fused, mask_ahead=ahead_ok)
        torch.cuda.synchronize(dev)
        self._faults_seen = self.fault_count + self.dropped_steps
        return len(self._graphs)

    def step_bound(self, i: int) -> torch.Tensor:
        """One optimisation step (train.py:159-190) on bound batch ``i`` with a device-sampled mask.  On the single-GPU fused
        path this is three launches -- the per-snapshot kernel, the parameter gradients, the update (which also samples the
        next step's mask) -- replayed from one hipGraph; the first step (and any step after the optimizer state moved under
        the trainer) runs the sampler's launch first."""
        self._refuse_under_layout("step_bound")
        return self._step_on(self._bound[i], slot=i)

    def steps_bound(self, indices, bound=None, losses: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``step_bound(i)`` for every i of ``indices``, in order -- as ONE captured launch sequence when the trainer is in its
        steady state (single GPU, fused path, transposed weights current, the first mask sampled ahead): 3 k kernels in one
        hipGraph, so the ~8 us between two graph launches are paid once per k steps instead of once per step.  The two mask
        buffers take turns inside the sequence exactly as they do between ``step_bound`` calls (step j trains on the mask the
        update launch of step j - 1 sampled), so the results are those of the single calls bit for bit.  Anything else (first
        step, data-parallel trainer, eager launches) falls back to the single calls.  ``bound``: another list of resident
        ``(x, y)`` batches than the one ``bind_batches`` registered (``fit_epoch``'s epoch buffer); ``losses``: a float32 vector
        whose entry j receives step j's loss.  Returns the last step's loss tensor."""
        self._refuse_under_layout("steps_bound")
        idx = tuple(int(i) for i in indices)
        bnd = self._bound if bound is None else bound
        if losses is not None and losses.numel() < len(idx):
            raise ValueError(f"`losses` holds {losses.numel()} entries for {len(idx)} steps")
        steady = (len(idx) > 1 and self.use_graph and self.fused and not self.split and self._mask_next and self._wt_current()
                  and self._mask_current() and self.node_ptr is not None)
        if not steady:
            for j, i in enumerate(idx):
                self._step_on(bnd[i], slot=i if bound is None else None)
                if losses is not None:
                    losses[j:j + 1].copy_(self.loss)
            return self.loss
        m0, m1 = self._mask_spare, self.mask          # step 0 trains on the mask sampled ahead and samples step 1's into the other

        def enqueue():
            a, b = m0, m1
            for j, i in enumerate(idx):
                self._enqueue(_STEP, True, True, flags=FLAG_MASK_NEXT, batch=bnd[i], masks=(a, b),
                              loss=None if losses is None else losses[j:j + 1])
                a, b = b, a

        # (the last update launch samples the next step's mask into the spare buffer; an odd number of steps leaves the buffers
        #  swapped)
        self._launch(("seq", idx, self.mask_rate, self.seed, self.world, m0.data_ptr(), bnd[idx[0]][0].data_ptr(),
                      None if losses is None else losses.data_ptr()), enqueue, True, len(idx), wt=True, mask_ahead=True,
                     swap=len(idx) % 2 == 1)
        if losses is not None:
            self.loss.copy_(losses[len(idx) - 1:len(idx)])
        return self.loss

    def _step_on(self, batch, slot=None) -> torch.Tensor:
        """``step_bound`` on a resident ``(x, y)`` batch: the kernels read it in place.  ``slot`` names it in the graph cache --
        the index of a bound batch; for any other batch (None) the buffers' addresses."""
        self._step(True, batch=batch, slot=("at", batch[0].data_ptr(), batch[1].data_ptr()) if slot is None else slot)
        return self.loss

    def forward_backward(self, x: torch.Tensor, y: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
        """Forward + loss + gradients only (no optimiser update); gradients land in ``self.grads``."""
        self.load_batch(x, y, mask)
        self._enqueue(PHASE_FORWARD | PHASE_BACKWARD, False)
        return self.loss

    @property
    def optimizer_step(self) -> int:
        return int(self.step_counter[0].item())

    # ---- AutoClip (use_gradient_clipping=True) -----------------------------------------------------------------------
    def _clip_state(self) -> _AutoClipState:
        if self._clip is None:
            raise RuntimeError("gradient clipping is off: construct the trainer with use_gradient_clipping=True")
        return self._clip

    @property
    def percentile(self) -> float:
        return self._clip_state().percentile

    def grad_norm_history(self):
        """The gradient norms of every update so far, in step order (float64 numpy): the reference's
        ``GradientClipping.grad_history``.  Synchronises."""
        st = self._clip_state()
        ctl = st.ctl.cpu()
        if int(ctl[4]) != 0:
            raise RuntimeError("the gradient-norm history overflowed its device buffers and updates were skipped")
        return st.log[:int(ctl[0])].cpu().numpy()

    @property
    def last_grad_norm(self) -> torch.Tensor:
        """Gradient norm of the last update that was not dropped (0-d float64 device tensor; no synchronisation)."""
        return self._clip_state().out[0]

    @property
    def last_clip_value(self) -> torch.Tensor:
        """Clip value (the percentile of the history) of that update (0-d float64 device tensor)."""
        return self._clip_state().out[1]

    @property
    def last_clip_coef(self) -> torch.Tensor:
        """The factor that update multiplied the gradient with, ``min(1, clip / (norm + 1e-6))`` (0-d float64 device tensor)."""
        return self._clip_state().out[2]

    def reset_gradient_clipping(self) -> None:
        """``GradientClipping.reset()``: forget the history (stream-ordered; captured steps stay valid)."""
        self._clip_state().reset()
