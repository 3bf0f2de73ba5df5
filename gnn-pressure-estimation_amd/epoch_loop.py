"""The epoch loop of ``GATResTrainer`` -- ``train_one_epoch`` (train.py:112-202) over a device-resident ``SnapshotStore``:
``fit_epoch`` and what only it needs (the in-place epoch buffer, the device-metrics table, the sibling trainer of the ragged
last batch).  A mixin: the methods run on a ``GATResTrainer`` and use its step API (``train_step.py``)."""
from __future__ import annotations

from typing import Callable, Dict, Optional, Tuple

import torch

from .sensor_layout import refuse_layout_multi_store


def refuse_multi_store_data_parallel(world: int) -> None:
    """A ``MultiSnapshotStore`` trains on one device: sharding a batch's recipe across ranks is not implemented."""
    if world > 1:
        raise NotImplementedError(f"data-parallel training (world size {world}) from a MultiSnapshotStore is not implemented: a "
                                  f"batch's recipe would have to be sharded across the ranks; train each rank's networks from "
                                  f"SnapshotStore shards or on one device")


class EpochLoop:
    def _epoch_in_place(self, store, order: torch.Tensor, nfull: int, kseq: int, total: torch.Tensor) -> None:
        from .train_step import MAX_CACHED_GRAPHS
        bs, npg = self.num_graphs, store.nodes_per_graph
        buf = self._epoch_buf
        if buf is None or tuple(buf.shape) != (nfull * bs, npg):
            if buf is not None:
                self.release_epoch_buffer()
            buf = self._epoch_buf = torch.empty(nfull * bs, npg, dtype=torch.float32, device=self.device)
            views = [buf[j * bs:(j + 1) * bs].reshape(-1) for j in range(nfull)]
            self._epoch_bound = [(v, v) for v in views]            # (x is also y: train.py:162-166)
            self._epoch_losses = None
        if self._epoch_losses is None or self._epoch_losses.numel() < max(kseq, 2):
            # (also when epoch_graph_steps was raised between two epochs on the same store: a step's loss slot must exist --
            #  ADVICE r5; the losses pointer is part of the sequences' graph key, so no stale graph meets the new vector)
            self._epoch_losses = torch.zeros(max(kseq, 2), dtype=torch.float32, device=self.device)
            # sequences of k (one graph per run of the epoch and mask orientation), single steps where a run starts or ends
            self._max_graphs = max(self._max_graphs, MAX_CACHED_GRAPHS + 2 * (nfull // kseq + 1) + 2 * kseq + 8)
        torch.index_select(store.data, 0, order[:nfull * bs], out=buf)
        self._train_epoch_buffer(nfull, kseq, total)

    def _train_epoch_buffer(self, nfull: int, kseq: int, total: torch.Tensor) -> None:
        """Train on the ``nfull`` batches that lie in the epoch buffer, ``kseq`` per captured launch sequence."""
        bs = self.num_graphs
        eb, lseq = self._epoch_bound, self._epoch_losses
        j = 0
        while j < nfull:
            k = min(kseq, nfull - j) if self._wt_current() and self._mask_current() else 1
            if k > 1:
                self.steps_bound(range(j, j + k), bound=eb, losses=lseq)
                total.add_(lseq[:k].double().sum(), alpha=float(bs))
            else:
                self._step_on(eb[j])       # (its slot names the buffers: a re-allocated epoch buffer never meets a stale graph)
                total.add_(self.loss.double(), alpha=float(bs))
            j += k

    def _epoch_in_place_multi(self, store, recipe, rows: torch.Tensor, nfull: int, kseq: int, total: torch.Tensor) -> None:
        """``_epoch_in_place`` for a ``MultiSnapshotStore``: the epoch's full batches are gathered from the networks' matrices by
        ONE launch (``gatres_gather_multi_rows``) into the buffer ``[nfull, N]``, batch by batch, and trained there."""
        from . import _native
        from .train_step import MAX_CACHED_GRAPHS
        buf = self._epoch_buf
        stride = self._epoch_stride()
        if buf is None or tuple(buf.shape) != (nfull, stride):
            if buf is not None:
                self.release_epoch_buffer()
            buf = self._epoch_buf = torch.empty(nfull, stride, dtype=torch.float32, device=self.device)
            self._epoch_bound = [(buf[j, :self.N], buf[j, :self.N]) for j in range(nfull)]
            self._epoch_losses = None
        if self._epoch_losses is None or self._epoch_losses.numel() < max(kseq, 2):
            self._epoch_losses = torch.zeros(max(kseq, 2), dtype=torch.float32, device=self.device)
            self._max_graphs = max(self._max_graphs, MAX_CACHED_GRAPHS + 2 * (nfull // kseq + 1) + 2 * kseq + 8)
        _native.check(self.lib.gatres_gather_multi_rows(
            store.table.data_ptr(), store.num_networks, store.net_of_graph(recipe).data_ptr(), rows.data_ptr(),
            self.node_ptr.data_ptr(), self.num_graphs, nfull, buf.data_ptr(), stride, _native.current_stream(self.device)),
            "gatres_gather_multi_rows")
        self._train_epoch_buffer(nfull, kseq, total)

    def _epoch_stride(self) -> int:
        """Floats between two batches of the multi-network epoch buffer: every batch starts on a 16-byte boundary."""
        return (self.N + 3) // 4 * 4

    def _epoch_copy_fits(self, rows: int, npg: int) -> bool:
        """May ``fit_epoch`` keep a device copy of the epoch's shuffled batches (``rows`` x ``npg`` floats: as large as the store
        itself, i.e. the store's footprint doubles)?  Yes if it already exists, or if it is within ``epoch_copy_limit_bytes``
        AND leaves a quarter of the device's free memory untouched; otherwise the epoch goes through the row-gather steps
        (``steps_rows``), which need no copy."""
        buf = self._epoch_buf
        if buf is not None and tuple(buf.shape) == (rows, npg):
            return True
        need = 4 * rows * npg
        if need > int(self.epoch_copy_limit_bytes):
            return False
        held = 0 if buf is None else buf.numel() * 4          # (a buffer of another shape is released first)
        free, _ = torch.cuda.mem_get_info(self.device)
        return need <= 0.75 * (free + held)

    def release_epoch_buffer(self) -> None:
        """Free ``fit_epoch``'s device copy of the epoch (and the graphs captured on it)."""
        if self._epoch_buf is not None:
            self._graphs.drop_all()
            self._epoch_buf = self._epoch_bound = self._epoch_losses = None

    def _fit_epoch_device_metrics(self, store, bs: int, shuffle: bool, drop_last: bool, generator,
                                  metric_fn_dict, total: Optional[torch.Tensor] = None):
        """fit_epoch with the metrics launch in every step (device_metrics=True).  ``total`` (``fit``): the epoch's loss sum is
        added to that device tensor and the graph count is returned in place of the mean loss."""
        from . import evaluation as E
        keys = list(metric_fn_dict or {})
        if not keys or not keys[0].endswith("_error"):
            raise ValueError("device_metrics=True computes evaluation.get_metric_fn_collection(prefix) only; "
                             "pass that collection as metric_fn_dict")
        prefix = keys[0][:-len("_error")]
        E._check_reference_metrics(None, metric_fn_dict, prefix)
        if store.norm_type == "znorm":
            scale, offset = float(store.std), float(store.mean)
        else:
            scale, offset = 1.0, 0.0
        from .multi_snapshot_store import MultiSnapshotStore
        if isinstance(store, MultiSnapshotStore):
            sizes = store.schedule(bs, self._multi_recipe(store, bs), drop_last).sizes
        else:
            S = store.num_snapshots
            sizes = [bs] * (S // bs) + ([S % bs] if S % bs and not drop_last else [])
        if not sizes:
            raise ValueError("the store yielded no batch")
        table = self._metrics_table
        if table is None or table.shape[0] < len(sizes):
            # persistent across epochs: its address is part of the captured steps' graph keys
            table = self._metrics_table = torch.zeros((len(sizes), E.METRICS_RECORD), dtype=torch.float64, device=self.device)
            self._metrics_cursor = torch.zeros(1, dtype=torch.int64, device=self.device)
        table.zero_()
        self._metrics_cursor.zero_()
        met = {"table": table, "cursor": self._metrics_cursor, "scale": scale, "offset": offset}
        self._metrics = met                 # (_sibling() hands it on to the ragged batch's trainer)
        try:
            if total is None:
                loss, _ = self.fit_epoch(store, bs, shuffle=shuffle, drop_last=drop_last, generator=generator)
            else:
                loss, _ = self._fit_epoch_sums(store, bs, shuffle, drop_last, generator, None, total, check=False)
        finally:
            self._metrics = None
            for t in self._siblings.values():
                t._metrics = None
        written = int(self._metrics_cursor.item())
        if written != len(sizes):
            raise RuntimeError(f"the epoch wrote {written} metric records for {len(sizes)} batches")
        _, metrics = E.metrics_from_moments(table[:len(sizes)].cpu().numpy(), sizes, prefix)
        return loss, metrics

    def _sibling(self, num_graphs: int, nodes_per_graph: int, edge_index: torch.Tensor) -> "GATResTrainer":
        """Trainer for another batch size of the same dataset (the ragged last batch of an epoch): its own plan and
        buffers, the SAME model, Adam moments and step counter."""
        return self._sibling_for(num_graphs, edge_index, [nodes_per_graph] * num_graphs)

    def _sibling_for(self, key, edge_index: torch.Tensor, nodes_per_graph) -> "GATResTrainer":
        """The sibling trainer kept under ``key`` (a graph count; ``("recipe", recipe)`` for a ``MultiSnapshotStore``'s tail
        batch), built on first use for the batch that ``edge_index`` / ``nodes_per_graph`` describe."""
        from .train_step import GATResTrainer
        t = self._siblings.get(key)
        if t is None:
            t = GATResTrainer(self.model, edge_index, sum(nodes_per_graph),
                              nodes_per_graph=nodes_per_graph, lr=self.hparams["lr"],
                              weight_decay=self.hparams["weight_decay"],
                              betas=(self.hparams["beta1"], self.hparams["beta2"]), eps=self.hparams["eps"],
                              mask_rate=self.mask_rate, seed=0, process_group=self.pg, use_graph=self.use_graph,
                              fused=self.fused, force_collective_path=self.split and self.world == 1,
                              targets_are_inputs=True, blocks_per_bucket=self.blocks_per_bucket,
                              criterion=self._criterion, _share_state_with=self)
            t.seed = self.seed
            self._siblings[key] = t
        t.mask_rate = self.mask_rate
        t._layout = self._layout            # (a sensor layout set or cleared since the sibling was built)
        t.store_norm = self.store_norm
        t._metrics = self._metrics          # (device_metrics: the ragged batch writes the epoch's last record)
        return t

    def _sibling_recipe(self, store, recipe) -> "GATResTrainer":
        """``_sibling`` for a tail batch of a ``MultiSnapshotStore``: the trainer of another recipe, kept under the recipe --
        single-store siblings stay under their graph counts."""
        t = self._sibling_for(("recipe", tuple(recipe)), store.edge_index(recipe), store.nodes_per_graph(recipe))
        t._recipe = tuple(recipe)
        return t

    def _multi_recipe(self, store, bs: int):
        """The recipe this trainer's batches of ``bs`` graphs have in ``store`` (a ``MultiSnapshotStore``), checked against what
        the trainer was built for."""
        refuse_multi_store_data_parallel(self.world)
        recipe = self._recipe if self._recipe is not None else store.recipe(bs)
        if (bs != self.num_graphs or len(recipe) != store.num_networks or sum(recipe) != bs
                or store.nodes_per_graph(recipe) != self._npg_list):
            raise ValueError(f"this trainer was not built for batches of {bs} graphs of this store's recipe {tuple(recipe)}: "
                             f"use GATResTrainer.for_store(model, store, batch_size)")
        return tuple(recipe)

    def _fit_epoch_multi_sums(self, store, bs: int, shuffle: bool, drop_last: bool, generator, metric_fn_dict,
                              total: torch.Tensor, check: bool = True) -> Tuple[int, Dict[str, float]]:
        """``_fit_epoch_sums`` over a ``MultiSnapshotStore``: the schedule's full batches through the in-place epoch buffer (one
        gather launch per epoch, captured k-step sequences) where the single-store conditions hold, step by step through
        ``gatres_stage_multi_rows_mask_required`` otherwise; every tail batch on the sibling trainer of its recipe.  The
        epoch's rows go to the device once; nothing is read back per batch."""
        recipe = self._multi_recipe(store, bs)
        if self._layout is not None:
            refuse_layout_multi_store(store)
        sched = store.schedule(bs, recipe, drop_last)
        host_metrics = bool(metric_fn_dict)
        sums = {k: 0.0 for k in (metric_fn_dict or {})}
        if not sched.sizes:
            raise ValueError("the store yielded no batch")
        rows = store.epoch_rows(sched, shuffle=shuffle, generator=generator)
        nfull = sched.nfull
        kseq = int(self.epoch_graph_steps)
        if not (self.use_graph and self.fused and not self.split):
            kseq = 1
        first = 0
        if (kseq > 1 and not host_metrics and nfull >= 2 and self._mask_next and self.node_ptr is not None
                and self._epoch_copy_fits(nfull, self._epoch_stride())):
            self._epoch_in_place_multi(store, recipe, rows, nfull, kseq, total)
            first = nfull
        seen = first * bs
        last = self

        def one(tr, rcp, offset: int, ng: int) -> None:
            nonlocal seen, last
            tr._stage_multi(store, rcp, rows.data_ptr() + 8 * offset)
            tr._step(True, premasked=True)
            last = tr
            total.add_(tr.loss.double(), alpha=float(ng))
            if host_metrics:
                m = tr.mask.bool()
                p, t = store.descale(tr.out[m]), store.descale(tr.x[m])
                for k, fn in metric_fn_dict.items():
                    sums[k] += float(fn(p, t)) * ng
            seen += ng

        for j in range(first, nfull):
            one(self, recipe, j * bs, bs)
        offset = nfull * bs
        for t in sched.tails:
            one(self._sibling_recipe(store, t), t, offset, sum(t))
            offset += sum(t)
        self._last_stepper = None if last is self else last      # (whose grads / out describe the epoch's last batch)
        if check:
            self.check_no_dropped_steps()
            for t in self._siblings.values():
                t.check_no_dropped_steps()
        return seen, sums

    def fit_epoch(self, store, batch_size: Optional[int] = None, shuffle: bool = True, drop_last: bool = False,
                  generator: Optional[torch.Generator] = None, metric_fn_dict: Optional[Dict[str, Callable]] = None,
                  device_metrics: bool = False) -> Tuple[float, Dict[str, float]]:
        """One epoch over a ``SnapshotStore`` -- the loop of ``train_one_epoch`` (train.py:159-198): shuffled batches, a
        fresh per-graph mask every batch, one optimisation step each, loss weighted by the batch's graph count.
        Batches are row gathers of the device-resident store (no host collation, no H2D); a ragged last batch runs on
        a sibling trainer that shares this one's optimizer state.  Returns ``(mean loss, metrics)``; metrics (the
        reference's de-normalised per-batch metrics, train.py:179-198) are only computed when ``metric_fn_dict`` is
        given, since they need a boolean gather per batch.  Under data parallelism every rank passes its own shard of
        the snapshots (``dp.shard_graphs``).

        ``device_metrics=True`` (with ``metric_fn_dict`` = ``evaluation.get_metric_fn_collection(prefix)``, the only collection
        it computes): every step's forward is followed by the masked-metric moments launch (``gatres_masked_metrics``) inside
        the same launch sequence -- the in-place epoch and the captured k-step sequences stay on -- and the metrics are formed
        from the epoch's moment table at the end (``evaluation.metrics_from_moments``).  Training itself is untouched: the
        same parameters, moments and loss bit for bit as without metrics.  ``device_metrics=False`` (default): nothing of
        this runs."""
        from .multi_snapshot_store import MultiSnapshotStore
        bs = int(batch_size) if batch_size is not None else self.num_graphs
        if self._layout is not None:
            refuse_layout_multi_store(store)
        if isinstance(store, MultiSnapshotStore):
            self._multi_recipe(store, bs)
        elif bs != self.num_graphs or store.nodes_per_graph * bs != self.N:
            raise ValueError(f"this trainer was built for batches of {self.num_graphs} graphs x {self.N // max(self.num_graphs, 1)} nodes")
        if self.world > 1:
            drop_last = True                 # equal graph counts on every rank keep plain gradient averaging exact
        if device_metrics:
            return self._fit_epoch_device_metrics(store, bs, shuffle, drop_last, generator, metric_fn_dict)
        # the epoch's loss sum in DOUBLE (train.py:196 accumulates Python floats): a sum of fp32 losses is exact there, so a
        # sequence's k losses added at once and the same losses added one by one give the same bits
        total = torch.zeros(1, dtype=torch.float64, device=self.device)
        seen, sums = self._fit_epoch_sums(store, bs, shuffle, drop_last, generator, metric_fn_dict, total)
        mean_loss = float(total.item()) / seen
        return mean_loss, {k: v / seen for k, v in sums.items()}

    def _fit_epoch_sums(self, store, bs: int, shuffle: bool, drop_last: bool, generator, metric_fn_dict,
                        total: torch.Tensor, check: bool = True) -> Tuple[int, Dict[str, float]]:
        """The body of ``fit_epoch``: the epoch's loss sum (loss x graphs, fp64) is ADDED to the device tensor ``total`` and never
        read here; returns the graph count and the host metrics' sums.  ``check=False``: the caller looks for dropped steps
        itself (``fit`` does, with the epoch's one read-back)."""
        from .multi_snapshot_store import MultiSnapshotStore
        if isinstance(store, MultiSnapshotStore):
            return self._fit_epoch_multi_sums(store, bs, shuffle, drop_last, generator, metric_fn_dict, total, check)
        npg = store.nodes_per_graph
        if self.world > 1:
            drop_last = True
        host_metrics = bool(metric_fn_dict)
        sums = {k: 0.0 for k in (metric_fn_dict or {})}
        seen = 0
        # the epoch's snapshot order goes to the device ONCE; a batch is a slice of it, collated inside the mask sampler's
        # launch (step_rows) -- the reference collates on the host and copies every iteration (train.py:302-303).  Runs of
        # `epoch_graph_steps` full batches go through ONE captured sequence each (steps_rows); what is left -- the first step
        # of a run whose transposed weights are not current, the epoch's last few batches, the ragged one -- goes step by step.
        kseq = int(self.epoch_graph_steps)
        if not (self.use_graph and self.fused and not self.split and self._rows_path_ok(store.data)):
            kseq = 1                                     # (eager / data-parallel / per-op trainers: step by step)
        order = store.epoch_order(shuffle=shuffle, generator=generator)
        first = 0                                        # batches [0, first) are done by the in-place path below
        nfull = store.num_snapshots // bs
        # (under a sensor layout every batch needs its staging launch -- the layout's mask is written there: no in-place epoch)
        if (kseq > 1 and not host_metrics and nfull >= 2 and self._mask_next and self.node_ptr is not None
                and self._layout is None and self._epoch_copy_fits(nfull * bs, npg)):
            # The epoch's full batches as ONE device gather into a persistent buffer (the shuffled store: S x N_g floats), then
            # trained IN PLACE, k per captured launch sequence, with the mask sampled ahead by the update launches -- the
            # bound-batch step of bench.py, three launches and nothing else: no collation launch, no per-step host work.
            self._epoch_in_place(store, order, nfull, kseq, total)
            first, seen = nfull, nfull * bs
        pending = []                                     # full batches waiting for a sequence
        last = self                                      # the trainer of the epoch's last step: a ragged batch's sibling, or this one

        def flush(n_keep: int = 0):
            nonlocal seen
            while len(pending) > n_keep:
                rows_one = pending.pop(0)
                if not self.step_rows(store.data, rows_one):
                    x = store.batch(rows_one)
                    self.load_batch(x, x)
                    self.run_step(device_mask=True)
                total.add_(self.loss.double(), alpha=float(bs))
                seen += bs

        for rows, edge_index, ng in store.row_batches(bs, drop_last=drop_last, order=order, first=first):
            if ng == bs and not host_metrics and kseq > 1:
                pending.append(rows)
                if len(pending) == kseq:
                    # (row_batches yields consecutive slices of ONE order tensor: the run is its slice too)
                    run = torch.cat(pending) if pending[0].data_ptr() + 8 * bs * (kseq - 1) != pending[-1].data_ptr() else \
                        torch.as_strided(pending[0], (kseq * bs,), (1,))
                    if self.steps_rows(store.data, run, total):
                        seen += kseq * bs
                        pending.clear()
                    else:
                        flush(n_keep=kseq - 1)           # one step by itself (it makes the weights current), then try again
                continue
            flush()
            tr = self if ng == bs else self._sibling(ng, npg, edge_index)
            if not tr.step_rows(store.data, rows):
                x = store.batch(rows)
                tr.load_batch(x, x)
                tr.run_step(device_mask=True)
            last = tr
            total.add_(tr.loss.double(), alpha=float(ng))
            if host_metrics:
                m = tr.mask.bool()
                p, t = store.descale(tr.out[m]), store.descale(tr.x[m])
                for k, fn in metric_fn_dict.items():
                    sums[k] += float(fn(p, t)) * ng
            seen += ng
        flush()
        if seen == 0:
            raise ValueError("the store yielded no batch")
        self._last_stepper = None if last is self else last
        # a dropped step (a split launch whose workgroups were not co-resident) trained on nothing: an epoch that contains one
        # is an error, not a slightly smaller epoch
        if check:
            self.check_no_dropped_steps()
            for t in self._siblings.values():
                t.check_no_dropped_steps()
        return seen, sums
