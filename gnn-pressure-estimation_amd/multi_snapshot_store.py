"""Device-resident snapshots of SEVERAL water networks: the multi-network form of ``SnapshotStore``.

The reference's ``WDNDataset`` (utils/DataLoader.py:61-183) takes lists of networks, normalises all of them with ONE set of
statistics over the concatenation of all arrays (:142-147) and lets the PyG loader shuffle the snapshots of all networks
together, so that a batch holds graphs of different topologies side by side.  Here:

  * every network k keeps its own dense fp32 matrix ``[S_k, N_k]`` on the device and its own single-graph ``edge_index``;
  * ``mean`` / ``std`` / ``min`` / ``max`` are taken over all values of all networks (``np.mean`` / ``np.std`` semantics) or
    passed in (validation and test stores take the training store's, train.py:67-86); the scaling is ``SnapshotStore``'s
    ``(x - mean) / (std + 1e-8)``;
  * a batch of ``B`` graphs has a FIXED composition, its *recipe* ``(b_0, .., b_{K-1})``: ``b_k`` graphs of network k, in
    network order.  This is a deliberate deviation from the reference's uniform shuffle across networks, where the composition
    of a batch is random: with a fixed recipe one ``edge_index`` tensor, one graph plan and one captured launch sequence serve
    every full batch of every epoch.  The default recipe is proportional to the networks' snapshot counts (largest remainder),
    so over an epoch every snapshot of every network is still visited exactly once, in a per-network random order;
  * an epoch's schedule is a pure function of ``(lengths, B, recipe, drop_last)``: ``nfull = min_k floor(S_k / b_k)`` full
    batches, then -- ``drop_last=False`` -- tail batches of at most ``B`` graphs whose recipes come from the same rule applied to
    what is left, until nothing is left.  Tail recipes depend on the lengths alone: their plans are built once.

With one network the store is a ``SnapshotStore`` of that network: same statistics, same ``edge_index``, same schedule, and
``fit_epoch`` gives the same parameters bit for bit.  One limit: where the epoch's device copy does not fit
(``trainer.epoch_copy_limit_bytes``) a ``SnapshotStore`` epoch still runs captured k-step sequences (``steps_rows``), a
``MultiSnapshotStore`` epoch goes one staging launch and one step at a time -- the same results, more host work per step.
Tail batches always run step by step; a network that dominates the snapshot counts makes most of a default-recipe epoch tails
(INTEGRATION.md): pass ``graphs_per_network`` then.
"""
from __future__ import annotations

import builtins
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch

from .snapshot_store import SnapshotStore

Recipe = Tuple[int, ...]


def batch_recipe(lengths: Sequence[int], batch_size: int) -> Recipe:
    """``b_k`` graphs of network k in a batch of ``batch_size``: proportional to ``lengths`` by the largest-remainder method
    (ties: the lower index), then every non-empty network that was left with none takes one graph from the network that holds
    the most (ties: the lower index).  At most ``sum(lengths)`` graphs are handed out.  ``batch_size`` below the number of
    networks is refused."""
    lengths = [int(s) for s in lengths]
    K, B = len(lengths), int(batch_size)
    if K == 0 or any(s < 0 for s in lengths):
        raise ValueError("lengths must be a non-empty sequence of non-negative snapshot counts")
    if B < K:
        raise ValueError(f"a batch of {B} graphs cannot hold a graph of each of {K} networks (batch_size >= num_networks)")
    total = sum(lengths)
    if total == 0:
        return tuple([0] * K)
    B = min(B, total)
    b = [B * s // total for s in lengths]
    rem = [B * s % total for s in lengths]
    for k in sorted(range(K), key=lambda k: (-rem[k], k))[:B - sum(b)]:
        b[k] += 1
    for k in range(K):
        if lengths[k] >= 1 and b[k] == 0:
            j = max(range(K), key=lambda j: (b[j], -j))
            if b[j] < 2:
                break                       # (fewer graphs than non-empty networks: only a tail of the last snapshots gets here)
            b[j] -= 1
            b[k] = 1
    return tuple(b)


class Schedule(NamedTuple):
    """An epoch's batches: ``nfull`` batches of ``recipe``, then one batch per entry of ``tails`` (a recipe each)."""
    recipe: Recipe
    nfull: int
    tails: Tuple[Recipe, ...]

    @property
    def sizes(self) -> List[int]:
        return [sum(self.recipe)] * self.nfull + [sum(t) for t in self.tails]


def epoch_schedule(lengths: Sequence[int], batch_size: int, recipe: Optional[Sequence[int]] = None,
                   drop_last: bool = False) -> Schedule:
    """The schedule as a pure function of its arguments (module docstring).  ``recipe=None``: ``batch_recipe``."""
    lengths = [int(s) for s in lengths]
    B = int(batch_size)
    recipe = batch_recipe(lengths, B) if recipe is None else tuple(int(b) for b in recipe)
    if len(recipe) != len(lengths) or any(b < 0 for b in recipe) or sum(recipe) not in (B, min(B, sum(lengths))):
        raise ValueError(f"graphs_per_network={recipe} does not describe a batch of {B} graphs of {len(lengths)} networks")
    if sum(recipe) == 0:
        return Schedule(recipe, 0, ())
    nfull = min(s // b for s, b in zip(lengths, recipe) if b > 0)
    tails: List[Recipe] = []
    if not drop_last:
        left = [s - nfull * b for s, b in zip(lengths, recipe)]
        while sum(left) > 0:
            t = batch_recipe(left, max(min(B, sum(left)), len(left)))
            tails.append(t)
            left = [s - b for s, b in zip(left, t)]
    return Schedule(recipe, nfull, tuple(tails))


class MultiSnapshotStore:
    def __init__(self, networks: Sequence[Tuple[torch.Tensor, torch.Tensor]], device=None, normalize: bool = True,
                 mean: Optional[float] = None, std: Optional[float] = None, min: Optional[float] = None,
                 max: Optional[float] = None, eps: float = 1e-8):
        """``networks``: K >= 1 pairs ``(snapshots [S_k, N_k], edge_index_k int64 [2, E_k] of ONE graph)``.  ``mean`` / ``std`` /
        ``min`` / ``max``: use these instead of the data's own (a validation or test store takes the training store's)."""
        networks = list(networks)
        if not networks:
            raise ValueError("a MultiSnapshotStore needs at least one network")
        for snaps, ei in networks:
            if snaps.dim() != 2:
                raise ValueError("snapshots must be [S_k, N_k]")
            if ei.dim() != 2 or ei.shape[0] != 2 or ei.dtype != torch.int64:
                raise ValueError("edge_index must be int64 [2, E] of ONE graph")
        device = torch.device(device if device is not None else networks[0][0].device)
        raw = [snaps.to(device=device, dtype=torch.float32) for snaps, _ in networks]
        count = sum(d.numel() for d in raw)
        if len(raw) == 1:
            # (one network: SnapshotStore's own arithmetic, so the scaled data are its data bit for bit)
            own_mean = float(raw[0].mean()) if mean is None else None
            own_std = float(raw[0].std(unbiased=False)) if std is None else None
        else:
            # all values of all networks as ONE array (DataLoader.py:142-147), two passes in double without building it
            own_mean = float(sum(d.double().sum() for d in raw) / count) if mean is None else None
            own_std = None
            if std is None:
                m = own_mean if mean is None else float(sum(d.double().sum() for d in raw) / count)
                own_std = float((sum(((d.double() - m) ** 2).sum() for d in raw) / count).sqrt())
        self.mean = own_mean if mean is None else float(mean)
        self.std = own_std if std is None else float(std)
        nonempty = [d for d in raw if d.numel()]
        self.min = float(min) if min is not None else (float(builtins.min(float(d.min()) for d in nonempty)) if nonempty else None)
        self.max = float(max) if max is not None else (float(builtins.max(float(d.max()) for d in nonempty)) if nonempty else None)
        self.norm_type = "znorm" if normalize else "unused"
        self.device = device
        self.stores: List[SnapshotStore] = []
        for d, (_, ei) in zip(raw, networks):
            data = ((d - self.mean) / (self.std + eps)).contiguous() if normalize else d.contiguous()
            self.stores.append(SnapshotStore(data, ei, device=device, normalize=False))
        for s in self.stores:
            s.mean, s.std, s.norm_type = self.mean, self.std, self.norm_type
        self.lengths: Tuple[int, ...] = tuple(len(s) for s in self.stores)
        self.num_snapshots = sum(self.lengths)
        # the device table of the matrices' addresses that the collation kernels read (include/gatres.h)
        self.table = torch.tensor([s.data.data_ptr() for s in self.stores], dtype=torch.int64).to(device)
        self._edge_index: Dict[Recipe, torch.Tensor] = {}
        self._net_of_graph: Dict[Recipe, torch.Tensor] = {}
        self._schedules: Dict[tuple, Schedule] = {}

    @classmethod
    def from_stores(cls, stores: Sequence[SnapshotStore]) -> "MultiSnapshotStore":
        """From per-network stores that are scaled already, all with the SAME statistics (nothing is rescaled or copied)."""
        stores = list(stores)
        if not stores:
            raise ValueError("a MultiSnapshotStore needs at least one network")
        first = stores[0]
        for s in stores[1:]:
            if (s.mean, s.std, s.norm_type, s.device) != (first.mean, first.std, first.norm_type, first.device):
                raise ValueError("the stores of a MultiSnapshotStore share one normalisation and one device")
        self = cls.__new__(cls)
        self.mean, self.std, self.norm_type, self.device = first.mean, first.std, first.norm_type, first.device
        self.min = self.max = None
        self.stores = stores
        self.lengths = tuple(len(s) for s in stores)
        self.num_snapshots = sum(self.lengths)
        self.table = torch.tensor([s.data.data_ptr() for s in stores], dtype=torch.int64).to(first.device)
        self._edge_index, self._net_of_graph, self._schedules = {}, {}, {}
        return self

    # ---- what evaluation / checkpoint code reads of a store --------------------------------------------------------------------
    def __len__(self) -> int:
        return self.num_snapshots

    @property
    def num_networks(self) -> int:
        return len(self.stores)

    def nodes_per_graph_of(self, k: int) -> int:
        return self.stores[k].nodes_per_graph

    def data_of(self, k: int) -> torch.Tensor:
        return self.stores[k].data

    def descale(self, scaled: torch.Tensor) -> torch.Tensor:
        return scaled * self.std + self.mean if self.norm_type == "znorm" else scaled

    # ---- recipes -------------------------------------------------------------------------------------------------------------------
    def recipe(self, batch_size: int, graphs_per_network: Optional[Sequence[int]] = None) -> Recipe:
        """The composition of a batch of ``batch_size`` graphs: the caller's ``graphs_per_network`` (checked) or the default."""
        if int(batch_size) < self.num_networks:
            raise ValueError(f"a batch of {batch_size} graphs cannot hold a graph of each of {self.num_networks} networks")
        if graphs_per_network is None:
            r = batch_recipe(self.lengths, batch_size)
            if sum(r) != int(batch_size):
                raise ValueError(f"the store holds {self.num_snapshots} snapshots: no batch of {batch_size}")
            return r
        r = tuple(int(b) for b in graphs_per_network)
        if len(r) != self.num_networks or any(b < 0 for b in r) or sum(r) != int(batch_size):
            raise ValueError(f"graphs_per_network={r} does not describe a batch of {batch_size} graphs of {self.num_networks} networks")
        return r

    def _check_recipe(self, recipe: Sequence[int]) -> Recipe:
        r = tuple(int(b) for b in recipe)
        if len(r) != self.num_networks or any(b < 0 for b in r) or sum(r) <= 0:
            raise ValueError(f"{r} is not a recipe of {self.num_networks} networks")
        return r

    def nodes_per_graph(self, recipe: Sequence[int]) -> List[int]:
        """Node counts of the batch's graphs, in batch order: what ``GATResTrainer(nodes_per_graph=...)`` takes."""
        r = self._check_recipe(recipe)
        return [self.stores[k].nodes_per_graph for k, b in enumerate(r) for _ in range(b)]

    def num_nodes(self, recipe: Sequence[int]) -> int:
        return sum(self.stores[k].nodes_per_graph * int(b) for k, b in enumerate(recipe))

    def node_ranges(self, recipe: Sequence[int]) -> List[Tuple[int, int]]:
        """``[lo, hi)`` of every network's nodes in a batch of ``recipe`` (a batch is in network order)."""
        out, lo = [], 0
        for k, b in enumerate(recipe):
            hi = lo + self.stores[k].nodes_per_graph * int(b)
            out.append((lo, hi))
            lo = hi
        return out

    def edge_index(self, recipe: Sequence[int]) -> torch.Tensor:
        """Block-diagonal ``edge_index`` of a batch of ``recipe`` (PyG ``Batch`` convention), cached: the SAME tensor object on
        every call, so the engine's plan cache takes its identity path."""
        r = self._check_recipe(recipe)
        ei = self._edge_index.get(r)
        if ei is None:
            if sum(1 for b in r if b) == 1:
                k = next(k for k, b in enumerate(r) if b)
                ei = self.stores[k].edge_index(r[k])           # (one network: its store's own cached tensor)
            else:
                blocks, off = [], 0
                for k, b in enumerate(r):
                    if b:
                        blocks.append(self.stores[k].edge_index(b) + off)
                        off += b * self.stores[k].nodes_per_graph
                ei = torch.cat(blocks, dim=1).contiguous()
            self._edge_index[r] = ei
        return ei

    def net_of_graph(self, recipe: Sequence[int]) -> torch.Tensor:
        """Device int32 ``[sum(recipe)]``: the network of every graph of the batch."""
        r = self._check_recipe(recipe)
        t = self._net_of_graph.get(r)
        if t is None:
            t = torch.tensor([k for k, b in enumerate(r) for _ in range(b)], dtype=torch.int32).to(self.device)
            self._net_of_graph[r] = t
        return t

    # ---- the epoch -----------------------------------------------------------------------------------------------------------------
    def schedule(self, batch_size: int, recipe: Optional[Sequence[int]] = None, drop_last: bool = False) -> Schedule:
        key = (int(batch_size), None if recipe is None else tuple(int(b) for b in recipe), bool(drop_last))
        s = self._schedules.get(key)
        if s is None:
            s = self._schedules[key] = epoch_schedule(self.lengths, batch_size, recipe, drop_last)
        return s

    def epoch_rows_host(self, schedule: Schedule, shuffle: bool = True,
                        generator: Optional[torch.Generator] = None) -> torch.Tensor:
        """The epoch's row indices (host int64), batch after batch in schedule order, each batch's graphs in network order;
        a row is an index INTO ITS NETWORK's matrix.  Network k's snapshots are taken in the order of a permutation of its
        own (drawn from ``generator`` in network order), so every snapshot occurs at most once -- exactly once when the
        schedule has its tails."""
        perms = [torch.randperm(S, generator=generator) if shuffle else torch.arange(S) for S in self.lengths]
        n, r = schedule.nfull, schedule.recipe
        parts = []
        if n:
            parts.append(torch.cat([p[:n * b].view(n, b) for p, b in zip(perms, r)], dim=1).reshape(-1))
        cur = [n * b for b in r]
        for t in schedule.tails:
            for k, b in enumerate(t):
                parts.append(perms[k][cur[k]:cur[k] + b])
                cur[k] += b
        for k, c in enumerate(cur):
            if c > self.lengths[k]:
                raise ValueError(f"the schedule takes {c} snapshots of network {k}, which holds {self.lengths[k]}")
        return torch.cat(parts) if parts else torch.zeros(0, dtype=torch.int64)

    def epoch_rows(self, schedule: Schedule, shuffle: bool = True, generator: Optional[torch.Generator] = None) -> torch.Tensor:
        """``epoch_rows_host`` on the device (one upload per epoch)."""
        return self.epoch_rows_host(schedule, shuffle, generator).to(self.device)

    def batch(self, recipe: Sequence[int], rows: torch.Tensor) -> torch.Tensor:
        """``[N, 1]`` node features of one batch (a torch gather; the training path collates inside its kernels instead)."""
        rows = rows.to(self.device)
        out, at = [], 0
        for k, b in enumerate(recipe):
            if b:
                out.append(self.stores[k].data.index_select(0, rows[at:at + b]).reshape(-1))
                at += b
        return torch.cat(out).reshape(-1, 1)

