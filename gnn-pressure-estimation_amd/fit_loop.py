"""The training loop of ``GATResTrainer`` -- ``internal_train`` (train.py:340-535) with its epoch boundary on the device:
``fit``, the best-state snapshot, ``FitHistory`` and ``internal_train``.  ``FitLoop`` is a mixin: its methods run on a
``GATResTrainer`` and use its epoch loop (``epoch_loop.py``) and its buffers."""
from __future__ import annotations

import ctypes as C
import math
import os
from collections import OrderedDict
from typing import Callable, Dict, Optional

import torch

from . import _native, dp
from .graph_models import GATResMeanConv


class FitLoop:
    def _fit_buffers(self, epochs: int, val_batches: int) -> dict:
        """Device and pinned-host buffers of ``fit``: the epoch's four sums {train loss sum, train graphs, validation loss sum,
        validation graphs}, the controller's state, the history table, the best checkpoint, and the pinned block the epoch's
        one read-back lands in (history record, validation moment table, the trainers' status words)."""
        from .epoch_control import RECORD, STATE
        from .evaluation import METRICS_RECORD
        fb = self._fit
        dev = self.device
        if fb is None:
            f32 = dict(dtype=torch.float32, device=dev)
            fb = self._fit = {"sums": torch.zeros(4, dtype=torch.float64, device=dev),
                              "state": torch.zeros(STATE, dtype=torch.float64, device=dev),
                              "best": [torch.zeros(self.P, **f32) for _ in range(3)],
                              "best_step": torch.zeros(1, dtype=torch.int64, device=dev),
                              "event": torch.cuda.Event(), "history": None, "host": None, "status_host": None}
        if fb["history"] is None or fb["history"].shape[0] < epochs:
            fb["history"] = torch.zeros((epochs, RECORD), dtype=torch.float64, device=dev)
        rows = 1 + val_batches * METRICS_RECORD // RECORD
        if fb["host"] is None or fb["host"].shape[0] < rows:
            fb["host"] = torch.zeros((rows, RECORD), dtype=torch.float64).pin_memory()
            fb["status_host"] = torch.zeros((8, 4), dtype=torch.int32).pin_memory()
        fb["state"].zero_()
        fb["state"][1] = float("inf")          # GATRES_EPOCH_S_BEST_LOSS
        fb["state"][6] = float("inf")          # GATRES_EPOCH_S_SCHED_BEST
        fb["best_valid"] = False
        return fb

    def _grad_flow_buffers(self) -> None:
        """``fit(log_gradient=True)``: the epoch's device row {total norm, 8 * num_blocks tensor norms, model update} and the
        pinned row its copy lands in with the epoch's read-back.  ``first_out`` (epoch 1's output) is taken inside ``fit``."""
        fb = self._fit
        n = 2 + 8 * self.model.num_blocks
        if fb.get("flow") is None or fb["flow"].numel() != n:
            fb["flow"] = torch.zeros(n, dtype=torch.float64, device=self.device)
            fb["flow_host"] = torch.zeros(n, dtype=torch.float64).pin_memory()
        fb["first_out"] = None

    def _snapshot(self, restore: bool = False) -> None:
        """``gatres_snapshot_if``: live state -> best buffers if the controller's `improved` flag is set (read on the device), or,
        ``restore``, best buffers -> live state unconditionally."""
        fb = self._fit
        live = [self.model.flat_parameters, self.exp_avg, self.exp_avg_sq]
        src, dst = (fb["best"], live) if restore else (live, fb["best"])
        s_step, d_step = (fb["best_step"], self.step_counter) if restore else (self.step_counter, fb["best_step"])
        flag = None if restore else fb["state"].data_ptr() + 8 * 8          # GATRES_EPOCH_S_IMPROVED
        _native.check(self.lib.gatres_snapshot_if(flag, src[0].data_ptr(), src[1].data_ptr(), src[2].data_ptr(), s_step.data_ptr(),
                                                  dst[0].data_ptr(), dst[1].data_ptr(), dst[2].data_ptr(), d_step.data_ptr(),
                                                  self.P, _native.current_stream(self.device)), "gatres_snapshot_if")

    def best_state(self) -> Dict[str, torch.Tensor]:
        """The best epoch's checkpoint that ``fit`` keeps on the device, as tensors (clones): the flat ``params``, ``exp_avg``,
        ``exp_avg_sq`` and the optimizer ``step`` (0-d int64).  Stream-ordered; nothing synchronises."""
        fb = self._fit
        if fb is None or not fb.get("best_valid"):
            raise RuntimeError("no best state: fit() has not run, or no epoch had a validation loss below +inf")
        p, m, v = (t.clone() for t in fb["best"])
        return {"params": p, "exp_avg": m, "exp_avg_sq": v, "step": fb["best_step"][0].clone()}

    def _state_dict_of(self, flat: torch.Tensor) -> "OrderedDict[str, torch.Tensor]":
        """``model.state_dict()`` with the values taken from another flat parameter vector (same layout)."""
        base = self.model.flat_parameters
        lo, hi = base.data_ptr(), base.data_ptr() + 4 * base.numel()
        out = OrderedDict()
        for k, v in self.model.state_dict().items():
            if lo <= v.data_ptr() < hi:
                off = (v.data_ptr() - lo) // 4
                out[k] = flat[off:off + v.numel()].view(v.shape).clone()
            else:
                out[k] = v.clone()
        return out

    def fit(self, train_store, val_store, epochs: int, *, batch_size: Optional[int] = None, val_batch_size: Optional[int] = None,
            patience: int = 100, min_delta: float = 1e-4, scheduler: Optional[str] = "ReduceLROnPlateau",
            scheduler_patience: int = 2, shuffle: bool = True, generator: Optional[torch.Generator] = None, val_seed: int = 0,
            train_metrics: bool = False, save_path: Optional[str] = None, model_name: Optional[str] = None,
            variant: Optional[str] = None, save_best: str = "reference", restore_best: bool = False,
            checkpoint_extra: Optional[dict] = None, log_gradient: bool = False,
            on_epoch: Optional[Callable[[int, dict], None]] = None, val_layout: bool = True, val_noise: bool = True,
            val_noise_seed: int = 0) -> "FitHistory":
        """The reference's training loop (train.py:376-511 ``internal_train``) with its epoch boundary on the device.

        Per epoch e = 1 .. ``epochs``: ``fit_epoch`` on ``train_store`` (with the ``"train"`` metric collection computed on the
        device when ``train_metrics``); a validation pass over ``val_store`` in order, in batches of ``val_batch_size``
        (default: ``batch_size``), with the trainer's ``mask_rate`` and device masks of seed ``val_seed + e`` --
        ``evaluation.evaluate_store(model, val_store, val_batch_size, mask_rate, seed=val_seed + e, prefix="val",
        gpu_warmup_times=0)``'s launches, plus one ``gatres_masked_loss`` launch per batch when the trainer's criterion is
        ``mae`` / ``sce`` (the validation loss is the trainer's criterion, as in the reference); then ONE launch
        (``gatres_epoch_control``) that forms both losses, keeps the best loss / epoch, runs
        ``EarlyStopping(mode="min", min_delta, patience)`` (fp32, on ``torch.tensor(val_loss)`` as the reference does) and, unless
        that stopped, ``ReduceLROnPlateau(mode="min", patience=scheduler_patience)`` (fp64, torch's defaults) writing the new
        learning rate straight into the buffer the update kernels read (no capture, no copy); then ``gatres_snapshot_if``, which
        keeps parameters, Adam moments and step count of an improving epoch in a device buffer.  The host reads one small
        pinned block per epoch (one event wait) and learns from it whether to stop; ``hparams["lr"]`` follows the device.
        ``scheduler``: ``"ReduceLROnPlateau"`` or ``None``.  ``epoch_control.EpochController`` states the controller in Python.

        Checkpoints (``save_path`` given; ``wdn_io.save_checkpoint``, the reference's keys plus ``checkpoint_extra``):
        ``last_{model_name}_{variant}.pth`` at epoch 1 and every 5th epoch unless the training loss is NaN;
        ``best_{model_name}_{variant}.pth`` at every improving epoch (``save_best="reference"``) or once, from the device
        snapshot, when ``fit`` returns (``"end"``: no file I/O inside improving epochs).  ``restore_best``: the best epoch's
        parameters, moments and step count are loaded back at the end (``best_state()`` hands them out either way).

        ``log_gradient`` (the reference's ``--log_gradient``, train.py:476-493): after the epoch's training pass, one
        ``gatres_grad_flow`` launch on the trainer that ran the epoch's last step (``gradient_flow()``: this trainer, or the
        sibling of a ragged last batch) and one ``gatres_mean_abs_diff`` launch of that trainer's ``out`` against a device copy
        taken in epoch 1 -- ``model_update = mean |out - first_out|``, 0 in epoch 1 -- into a device row that travels with the
        epoch's read-back (no further synchronisation).  The history then holds ``total_grad_norm``, ``block_norms`` (a numpy
        array per epoch, in the order of ``block_names``), ``model_update`` and its running sum ``accum_model_update``.  A later
        epoch whose last batch has another size than epoch 1's raises ``ValueError``.  Off (default): none of this is enqueued.

        ``on_epoch(epoch, info)``: called once per epoch after its read-back and checkpoints, before early stopping ends the
        loop -- where the reference calls ``log_metrics_on_wandb`` (train.py:476-504).  ``info``: ``tr_loss``, ``val_loss``,
        ``best_loss``, ``best_epoch``, ``lr`` (the rate the epoch trained with), ``improved``, ``val_metric_dict``,
        ``train_metric_dict`` (with ``train_metrics``) and, with ``log_gradient``, ``total_grad_norm``, ``block_norms``,
        ``model_update``, ``accum_model_update``.  An exception it raises propagates.

        Sensor layout (``set_sensor_layout``): the training epochs stage under the layout, and the validation pass masks
        everything but the layout's sensors -- ``evaluate_store(..., observed_idx=layout, seed=val_seed + e)``'s launches, the
        deployment mask without dropout -- so ``val_loss``, early stopping, the scheduler and ``best_metric_dict`` speak of the
        deployed error.  ``val_layout=False`` keeps the random-mask validation.  Checkpoints then carry ``sensor_layout``
        (``observed_idx``, ``sensor_dropout``, ``layout_share``) beside ``checkpoint_extra``.  Without a layout ``val_layout`` is
        not looked at.

        Measurement noise (``set_sensor_layout(noise_std=...)``): the training batches are staged under it, and the layout
        validation pass is staged under the same ``noise_std`` -- ``evaluate_store(..., observed_idx=layout, noise_std=noise_std,
        noise_seed=val_noise_seed)``'s launches, member 0.  The seed is FIXED and the member is 0 in every epoch: the noise
        realisation of the validation set is the same each epoch, so early stopping and ``ReduceLROnPlateau`` compare like with
        like (a fresh realisation per epoch would add the realisation's own variance to every comparison).  ``val_noise=False``
        validates on exact readings; ``val_layout=False`` implies that (the random-mask pass carries no noise).  Checkpoints'
        ``sensor_layout`` then also carries ``noise_std`` (physical units) and ``noise_seed``.

        Data parallel: every rank passes its shards; the epoch's four sums are all-reduced (one collective per epoch), so all
        ranks take the same decision; metric dicts and ``model_update`` describe the rank's own shard, the gradient norms the
        all-reduced gradient (the same on every rank).  Returns a ``FitHistory``."""
        from . import evaluation as E, wdn_io
        from .epoch_control import RECORD_FIELDS
        from .train_step import STATUS_DROPPED_STEPS, STATUS_FAULT_COUNT
        if save_best not in ("reference", "end"):
            raise ValueError("save_best must be 'reference' or 'end'")
        if scheduler not in (None, "ReduceLROnPlateau"):
            raise ValueError("scheduler must be 'ReduceLROnPlateau' or None")
        epochs = int(epochs)
        if epochs <= 0:
            raise ValueError("epochs must be positive")
        if save_path is not None and (model_name is None or variant is None):
            raise ValueError("save_path needs model_name and variant (the files are best_/last_{model_name}_{variant}.pth)")
        bs = int(batch_size) if batch_size is not None else self.num_graphs
        vbs = int(val_batch_size) if val_batch_size is not None else bs
        from .multi_snapshot_store import MultiSnapshotStore
        from .sensor_layout import refuse_layout_data_parallel, refuse_layout_multi_store
        layout = self._layout
        if layout is not None:
            refuse_layout_data_parallel(self.world)
            refuse_layout_multi_store(train_store)
            refuse_layout_multi_store(val_store)
        multi = isinstance(train_store, MultiSnapshotStore)
        if multi:
            # (several networks: the batch's recipe is the trainer's, GATResTrainer.for_store; one device only)
            self._multi_recipe(train_store, bs)
            if isinstance(val_store, MultiSnapshotStore) and val_store.num_networks != train_store.num_networks:
                raise ValueError(f"the validation store holds {val_store.num_networks} networks, the training store "
                                 f"{train_store.num_networks}: a multi-network validation store must have the same networks")
        elif bs != self.num_graphs or train_store.nodes_per_graph * bs != self.N:
            raise ValueError(f"this trainer was built for batches of {self.num_graphs} graphs x {self.N // max(self.num_graphs, 1)} nodes")
        if isinstance(val_store, MultiSnapshotStore) and not multi:
            raise ValueError("a multi-network validation store needs a multi-network training store (same number of networks)")
        cfg = _native.GatresEpochConfig(float(min_delta), 0.1, 1e-4, 0.0, 1e-8, int(patience), int(scheduler_patience),
                                        int(scheduler is not None), 0)
        val = E._ValidationPass(self.model, val_store, vbs, self.mask_rate, self._criterion,
                                observed_idx=layout.observed_idx if layout is not None and val_layout else None,
                                noise_std=layout.noise_std if layout is not None and val_layout and val_noise else None,
                                noise_seed=val_noise_seed)
        extra = dict(checkpoint_extra or {})
        if layout is not None:
            extra["sensor_layout"] = layout.describe()
        nvb = len(val.sizes)
        fb = self._fit_buffers(epochs, nvb)
        sums, state, history, host, status_host, event = (fb[k] for k in ("sums", "state", "history", "host", "status_host", "event"))
        train_fns = E.get_metric_fn_collection("train") if train_metrics else None
        R = {k: i for i, k in enumerate(RECORD_FIELDS)}
        hist = FitHistory()
        if log_gradient:
            self._grad_flow_buffers()
            hist.block_names = self.gradient_flow_names()
        accum_update = 0.0
        best_table = None
        paths = None
        if save_path is not None:
            os.makedirs(save_path, exist_ok=True)
            paths = {k: os.path.join(save_path, f"{k}_{model_name}_{variant}.pth") for k in ("best", "last")}
        stats = dict(mean=train_store.mean, std=train_store.std, min=getattr(train_store, "min", None),
                     max=getattr(train_store, "max", None), norm_type=train_store.norm_type)

        def val_metrics(table) -> Dict[str, float]:
            return E.metrics_from_moments(table, val.sizes, "val")[1]

        def save(which: str, rec, table, model_sd=None, adam=None) -> None:
            wdn_io.save_checkpoint(
                paths[which], model_state_dict=self.model.state_dict() if model_sd is None else model_sd,
                optimizer_state_dict=wdn_io.adam_state_dict(self, lr=rec[R["lr_used"]]) if adam is None else adam,
                epoch=int(rec[R["best_epoch"]]), loss=float(rec[R["best_loss"]]), val_metric_dict=val_metrics(table),
                **stats, **extra)

        stream = _native.current_stream(self.device)
        best_rec = None
        for e in range(1, epochs + 1):
            sums.zero_()
            if train_metrics:
                seen, tr_m = self._fit_epoch_device_metrics(train_store, bs, shuffle, self.world > 1, generator, train_fns,
                                                            total=sums[0:1])
                hist.train_metrics.append(tr_m)
            else:
                seen, _ = self._fit_epoch_sums(train_store, bs, shuffle, False, generator, None, sums[0:1], check=False)
            sums[1:2].fill_(float(seen))
            if log_gradient:
                # (before the validation pass; epoch 1 also pays one device copy of `out`)
                last = self.last_step_trainer
                if fb["first_out"] is None:
                    fb["first_out"] = last.out.clone()
                elif fb["first_out"].numel() != last.out.numel():
                    raise ValueError(f"log_gradient: the last training batch of epoch {e} holds {last.out.numel()} nodes, that of "
                                     f"epoch 1 held {fb['first_out'].numel()}: model_update = mean |out - first_out| needs the same "
                                     f"batch size at the end of every epoch (a fixed store and drop_last)")
                last._enqueue_grad_flow(fb["flow"])
                last._enqueue_model_update(fb["first_out"], fb["flow"][-1:])
            val.enqueue(val_seed + e)
            if self.world > 1:
                _native.check(self.lib.gatres_epoch_val_sums(_native.ptr(val.table if val.losses is None else None),
                                                             _native.ptr(val.losses), val.graphs.data_ptr(), nvb,
                                                             sums[2:].data_ptr(), stream), "gatres_epoch_val_sums")
                dp.all_reduce_sums_(sums, self.pg)
                _native.check(self.lib.gatres_epoch_control(sums.data_ptr(), None, None, None, 0, sums[2:].data_ptr(), C.byref(cfg),
                                                            self.hp.data_ptr(), state.data_ptr(), history.data_ptr(),
                                                            history.shape[0], stream), "gatres_epoch_control")
            else:
                _native.check(self.lib.gatres_epoch_control(sums.data_ptr(), _native.ptr(val.table if val.losses is None else None),
                                                            _native.ptr(val.losses), val.graphs.data_ptr(), nvb, None, C.byref(cfg),
                                                            self.hp.data_ptr(), state.data_ptr(), history.data_ptr(),
                                                            history.shape[0], stream), "gatres_epoch_control")
            self._snapshot()
            # the epoch's one read-back: its history record, the validation moments and every trainer's status words
            trainers = [t for t in [self] + list(self._siblings.values()) if t._status is not None][:status_host.shape[0]]
            host[0].copy_(history[e - 1], non_blocking=True)
            host[1:].view(-1)[:val.table.numel()].copy_(val.table.view(-1), non_blocking=True)
            for i, t in enumerate(trainers):
                status_host[i].copy_(t._status, non_blocking=True)
            if log_gradient:
                fb["flow_host"].copy_(fb["flow"], non_blocking=True)
            event.record(torch.cuda.current_stream(self.device))
            event.synchronize()
            rec = host[0].numpy().copy()
            for i, t in enumerate(trainers):
                t.check_no_dropped_steps((int(status_host[i, STATUS_FAULT_COUNT]), int(status_host[i, STATUS_DROPPED_STEPS])))
            self.hparams["lr"] = float(rec[R["lr_after"]])          # (the device buffer holds it already; siblings share the dict)
            improved, stop = bool(rec[R["improved"]]), bool(rec[R["stop"]])
            hist.tr_loss.append(float(rec[R["tr_loss"]])); hist.val_loss.append(float(rec[R["val_loss"]]))
            hist.lr.append(float(rec[R["lr_used"]])); hist.improved.append(improved)
            hist.records.append(rec)
            if log_gradient:
                flow = fb["flow_host"].numpy().copy()
                accum_update += float(flow[-1])
                hist.total_grad_norm.append(float(flow[0])); hist.block_norms.append(flow[1:-1])
                hist.model_update.append(float(flow[-1])); hist.accum_model_update.append(accum_update)
            if improved:
                fb["best_valid"] = True
                best_rec = rec
                best_table = host[1:].view(-1)[:val.table.numel()].numpy().copy()
                if paths is not None and save_best == "reference":
                    save("best", rec, best_table)
            if paths is not None and (e == 1 or e % 5 == 0) and not math.isnan(rec[R["tr_loss"]]):
                save("last", rec, host[1:].view(-1)[:val.table.numel()].numpy())
            if on_epoch is not None:
                info = dict(tr_loss=hist.tr_loss[-1], val_loss=hist.val_loss[-1], best_loss=float(rec[R["best_loss"]]),
                            best_epoch=int(rec[R["best_epoch"]]), lr=hist.lr[-1], improved=improved,
                            val_metric_dict=val_metrics(host[1:].view(-1)[:val.table.numel()].numpy()))
                if train_metrics:
                    info["train_metric_dict"] = hist.train_metrics[-1]
                if log_gradient:
                    info.update(total_grad_norm=hist.total_grad_norm[-1], block_norms=hist.block_norms[-1],
                                model_update=hist.model_update[-1], accum_model_update=hist.accum_model_update[-1])
                on_epoch(e, info)
            if stop:
                hist.stopped_epoch = e
                break
        hist.best_loss = float(rec[R["best_loss"]])
        hist.best_epoch = int(rec[R["best_epoch"]])
        hist.final_lr = float(rec[R["lr_after"]])
        if best_table is not None:
            hist.best_metric_dict = val_metrics(best_table)
            if paths is not None and save_best == "end":
                b = self.best_state()
                save("best", best_rec, best_table, model_sd=self._state_dict_of(b["params"]),
                     adam=wdn_io.adam_state_dict(self, exp_avg=b["exp_avg"], exp_avg_sq=b["exp_avg_sq"], step=int(b["step"]),
                                                 lr=best_rec[R["lr_used"]]))
        if restore_best and fb["best_valid"]:
            self._snapshot(restore=True)
            # the parameters and the step count moved behind every trainer of this model: transposed weights in scratch and a
            # mask sampled ahead belong to the state that was replaced
            for t in [self] + list(self._siblings.values()):
                t._unknown()
        return hist


class FitHistory:
    """What ``GATResTrainer.fit`` returns: per-epoch lists -- ``tr_loss``, ``val_loss``, ``lr`` (the rate the epoch trained
    with), ``improved`` -- ``best_loss``, ``best_epoch``, ``stopped_epoch`` (None: ran all epochs), ``best_metric_dict`` (the
    validation metrics of the best epoch, keys of ``get_metric_fn_collection("val")``), ``train_metrics`` (one dict per epoch
    when asked for), ``final_lr`` and ``records`` (the controller's raw history records, ``epoch_control.RECORD_FIELDS``).  With
    ``fit(log_gradient=True)`` also per epoch ``total_grad_norm``, ``block_norms`` (a float64 numpy array ``[8 * num_blocks]`` in
    the order of ``block_names``), ``model_update`` and ``accum_model_update``; empty lists otherwise."""

    def __init__(self) -> None:
        self.tr_loss, self.val_loss, self.lr, self.improved, self.records, self.train_metrics = [], [], [], [], [], []
        self.best_loss, self.best_epoch, self.stopped_epoch, self.final_lr = float("inf"), 0, None, None
        self.best_metric_dict: Dict[str, float] = {}
        self.total_grad_norm, self.block_norms, self.block_names, self.model_update, self.accum_model_update = [], [], [], [], []


def internal_train(args, model: GATResMeanConv, train_store, val_store, **fit_kw):
    """``train.py``'s ``internal_train`` over the native loop: an ``argparse.Namespace`` with train.py's names (``lr``,
    ``weight_decay``, ``epochs``, ``mask_rate``, ``criterion``, ``batch_size``, ``patience``, ``min_delta``, ``scheduler``,
    ``scheduler_patience``, ``use_gradient_clipping``, ``percentile``, ``save_path``, ``model_name``, ``variant``) becomes a
    ``GATResTrainer`` and one ``fit`` call.  Returns ``(best_loss, best_metric_dict)``.  ``fit_kw`` goes to ``fit``
    (``generator``, ``val_seed``, ``save_best``, ``log_gradient``, ``on_epoch``, ...)."""
    from .train_step import GATResTrainer
    bs = int(args.batch_size)
    # (a SnapshotStore or, for several networks, a MultiSnapshotStore: the batch's composition is the store's default recipe)
    trainer = GATResTrainer.for_store(model, train_store, bs, lr=args.lr, weight_decay=args.weight_decay,
                                      mask_rate=args.mask_rate, criterion=getattr(args, "criterion", None) or "mse",
                                      use_gradient_clipping=bool(getattr(args, "use_gradient_clipping", False)),
                                      percentile=float(getattr(args, "percentile", 10.0)))
    hist = trainer.fit(train_store, val_store, int(args.epochs), batch_size=bs, patience=int(args.patience),
                       min_delta=float(args.min_delta),
                       scheduler="ReduceLROnPlateau" if getattr(args, "scheduler", None) == "ReduceLROnPlateau" else None,
                       scheduler_patience=int(getattr(args, "scheduler_patience", 2)), save_path=getattr(args, "save_path", None),
                       model_name=getattr(args, "model_name", None), variant=getattr(args, "variant", None), **fit_kw)
    return hist.best_loss, hist.best_metric_dict
