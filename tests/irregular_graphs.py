"""Seeded irregular graphs for the kernel tests (torch + numpy only; imported by tests, not a conftest).

wdn_synth's WDN topologies are symmetric, loop-free and duplicate-free with node degrees <= 5, so every CSR row of their
plans has at most 6 entries and the kernels' longer-row code never runs on them.  The graphs here are built around named
features instead:

  * rows at the slot-path boundaries: GATConv in-rows (in-degree + the self loop GATConv adds) of 6 / 7 entries and of
    32 / 33 entries, and the same for out-rows (the transposed CSR) in the directed graphs;
  * one long row (7 .. 32 entries) in a 64-row wave whose other rows are short, while most waves have rows of <= 4;
  * a long row, or a hub of more than 32 entries, in the ragged last 64-row wave;
  * isolated nodes, self loops, duplicate edges and directed edges;
  * node counts that are not multiples of 16, 32 or 64;
  * local node order (chains of consecutive ids, long rows fed by their nearest free nodes) or a shuffled one.

Every ordinary node ends with at most 3 edges into and out of it (rows of at most 4 entries); only the named special
nodes are longer.  ``row_counts`` restates the plan's row lengths in numpy so the CPU test can hold each graph to its
features, and the GPU tests can rely on them."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

SYMMETRIC, DEG_LE32, DEG_LE6 = 1, 2, 4          # GATRES_GRAPH_* (include/gatres.h)
WAVE = 64


@dataclass
class IrregularGraph:
    name: str
    edge_index: torch.Tensor                     # int64 [2, E]
    num_nodes: int
    flags: int                                   # the GATRES_GRAPH_* bits the graph is built to have
    in_rows: Dict[int, int] = field(default_factory=dict)     # GATConv in-row length -> node
    out_rows: Dict[int, int] = field(default_factory=dict)    # GATConv out-row length -> node
    last_wave: Optional[int] = None              # a long row (or hub) in the ragged last wave
    isolated: List[int] = field(default_factory=list)
    self_loops: List[int] = field(default_factory=list)
    duplicates: int = 0
    directed: int = 0                            # single directed edges among ordinary nodes


def row_counts(edge_index: torch.Tensor, n: int) -> Dict[str, np.ndarray]:
    """Row lengths of the plan's CSRs (include/gatres.h, graph plan): GATConv drops self loops and adds one per node,
    SimpleConv keeps the edge list as it is; `in` = destination-sorted rows, `out` = the transposes."""
    s, d = edge_index[0].numpy(), edge_index[1].numpy()
    nl = s != d
    return {"gat_in": np.bincount(d[nl], minlength=n) + 1, "gat_out": np.bincount(s[nl], minlength=n) + 1,
            "mean_in": np.bincount(d, minlength=n), "mean_out": np.bincount(s, minlength=n)}


def build_graph(name: str, n: int, *, symmetric: bool, in_rows: Sequence[int] = (), out_rows: Sequence[int] = (),
                last_wave: Optional[int] = None, isolated: int = 3, self_loops: int = 4, duplicates: int = 4,
                directed: int = 0, chain: int = 40, at: Optional[int] = None, spacing: int = 3, shuffle: bool = False,
                seed: int = 0) -> IrregularGraph:
    """``in_rows`` / ``out_rows``: GATConv row lengths (degree + 1) of special nodes placed ``spacing`` ids apart from
    ``at`` (symmetric graphs: in == out, ``out_rows`` unused); ``last_wave``: the row length of one more special node in
    the ragged last wave.  Ordinary nodes lie on chains of ``chain`` consecutive ids
    (``chain >= n``: one path, so that a snapshot is one segment of the fused kernels).  ``spacing=1`` with an even ``at``
    and in_rows starting (6, 7, ...) puts a row of exactly 6 entries and one of 7 into one aligned pair of rows: the same
    wave whatever the rows per wave (2 .. 64), so that the row of 6 takes the kernels' mixed-wave slot branch."""
    rng = np.random.RandomState(seed)
    at = n // 3 if at is None else at
    ind, outd = np.zeros(n, np.int64), np.zeros(n, np.int64)
    edges: List[tuple] = []
    special: Dict[int, tuple] = {}               # node -> (in-degree, out-degree) it must end with

    def add(u, v, both):
        edges.append((u, v)); outd[u] += 1; ind[v] += 1
        if both:
            edges.append((v, u)); outd[v] += 1; ind[u] += 1

    # special nodes first (ids fixed), isolated nodes away from them
    spec_in = [(at + spacing * k, r) for k, r in enumerate(in_rows)]
    spec_out = [] if symmetric else [(at + spacing * (len(in_rows) + k) + 1, r) for k, r in enumerate(out_rows)]
    for v, r in spec_in:
        special[v] = (r - 1, r - 1) if symmetric else (r - 1, None)
    for v, r in spec_out:
        special[v] = (None, r - 1)
    lw = None
    if last_wave is not None:
        assert n % WAVE, "the last wave must be ragged"
        lw = n - 1 - (n % WAVE) // 2
        special[lw] = (last_wave - 1, last_wave - 1) if symmetric else (last_wave - 1, None)
    free = [v for v in range(n) if v not in special and all(abs(v - s) > 2 for s in special)]
    iso = sorted(rng.choice(free[len(free) // 2:], isolated, replace=False).tolist()) if isolated else []
    skip = set(iso)
    # chains of consecutive ids (both directions, bridging the isolated nodes): every ordinary node has degree <= 2 here
    ids = [v for v in range(n) if v not in skip]
    for u, v in zip(ids, ids[1:]):
        if u // chain == v // chain:
            add(u, v, True)

    def donors(v, need, room):
        """The `need` nodes nearest to v (local order) that can take one more edge without a row above 4 entries."""
        got, dist = [], 1
        while len(got) < need:
            assert dist < n, "graph too small for its special rows"
            for u in (v - dist, v + dist):
                if 0 <= u < n and len(got) < need and u not in special and u not in skip and room(u) and \
                        (u, v) not in edge_set and (v, u) not in edge_set:
                    got.append(u)
            dist += 1
        return got

    for v, (want_in, want_out) in special.items():
        edge_set = set(edges)
        if symmetric:
            for u in donors(v, want_in - ind[v], lambda u: ind[u] < 3 and outd[u] < 3):
                add(u, v, True)
        else:
            if want_in is not None and want_in > ind[v]:
                for u in donors(v, want_in - ind[v], lambda u: outd[u] < 3):
                    add(u, v, False)
            if want_out is not None and want_out > outd[v]:
                for u in donors(v, want_out - outd[v], lambda u: ind[u] < 3):
                    add(v, u, False)
    ordinary = [v for v in range(n) if v not in special and v not in skip and all(abs(v - s) > 1 for s in special)]
    pick = iter(rng.permutation(ordinary).tolist())

    def next_with(cond):
        for u in pick:
            if cond(u):
                return u
        raise AssertionError("ran out of ordinary nodes")

    loops = []
    for _ in range(self_loops):                  # (a self loop counts for SimpleConv's rows, not for GATConv's)
        u = next_with(lambda u: ind[u] < 3 and outd[u] < 3)
        add(u, u, False); loops.append(u)
    edge_set = set(edges)
    chain_edges = [(u, v) for (u, v) in edge_set if v == u + 1 and u // chain == v // chain]
    chain_edges.sort()
    order = rng.permutation(len(chain_edges))
    dups = 0
    for i in order:                              # duplicates of chain edges (both directions in symmetric graphs)
        if dups == duplicates:
            break
        u, v = chain_edges[i]
        if max(ind[u], outd[u], ind[v], outd[v]) < 3 and u not in special and v not in special:
            add(u, v, symmetric); dups += 1
    ndir = 0
    while ndir < (0 if symmetric else directed):  # single directed edges between ordinary nodes
        u = next_with(lambda u: outd[u] < 3)
        w = next_with(lambda w: ind[w] < 3 and w != u)
        add(u, w, False); ndir += 1
    ei = torch.tensor(edges, dtype=torch.int64).t().contiguous()
    ei = ei[:, torch.from_numpy(rng.permutation(ei.shape[1]))]          # (edge order is the caller's business)
    relabel = np.arange(n)
    if shuffle:
        relabel = rng.permutation(n)
        if lw is not None:                       # (the last-wave row keeps its id)
            j = int(np.nonzero(relabel == lw)[0][0])
            relabel[lw], relabel[j] = lw, relabel[lw]
        ei = torch.from_numpy(relabel)[ei]
    rl = lambda v: int(relabel[v])
    flags = (SYMMETRIC if symmetric else 0) | (DEG_LE32 if max(ind.max(), outd.max()) + 1 <= 32 else 0) | \
        (DEG_LE6 if max(ind.max(), outd.max()) + 1 <= 6 else 0)
    g = IrregularGraph(name, ei, n, flags, isolated=[rl(v) for v in iso], self_loops=[rl(v) for v in loops],
                       duplicates=dups, directed=ndir)
    for v, r in spec_in:
        g.in_rows[r] = rl(v)
        if symmetric:
            g.out_rows[r] = rl(v)
    for v, r in spec_out:
        g.out_rows[r] = rl(v)
    if lw is not None:
        g.last_wave = rl(lw)
    return g


# Named graphs: name -> (builder arguments, the GATRES_GRAPH_* flags gatres_graph_flags_host must report).
# 1001 = 15 * 64 + 41 (and 9 past a 16-row tile, 9 past a 32-row phase); 725 = 11 * 64 + 21; 389 = 6 * 64 + 5.
SPECS = {
    # rows of 6, 7 and 32 entries in one wave, a 20-entry row in the last wave: LE32 without LE6
    "sym_le32": (dict(n=1001, symmetric=True, in_rows=(6, 7, 32), last_wave=20, at=334, spacing=1, seed=1),
                 SYMMETRIC | DEG_LE32),
    "sym_le32_shuffled": (dict(n=1001, symmetric=True, in_rows=(6, 7, 32), last_wave=20, at=334, spacing=1, shuffle=True,
                               seed=1),
                          SYMMETRIC | DEG_LE32),
    # in-rows and out-rows (transposed CSR) of 6, 7 and 32 entries at different nodes, directed edges
    "dir_le32": (dict(n=1001, symmetric=False, in_rows=(6, 7, 32), out_rows=(6, 7, 32), last_wave=17, directed=8,
                      at=334, spacing=1, seed=3), DEG_LE32),
    # rows of 32 and 33 entries, a 48-entry hub in the last wave: the per-op kernels' whole-wave hub path
    "sym_hub": (dict(n=725, symmetric=True, in_rows=(6, 7, 32, 33), last_wave=48, seed=4), SYMMETRIC),
    "dir_hub": (dict(n=725, symmetric=False, in_rows=(7, 33), out_rows=(6, 7, 32, 33, 50), last_wave=40, directed=8,
                     seed=5), 0),
    "dir_hub_shuffled": (dict(n=725, symmetric=False, in_rows=(7, 33), out_rows=(6, 7, 32, 33, 50), last_wave=40,
                              directed=8, shuffle=True, seed=5), 0),
    # one snapshot of the fused-path batches (collated bs times): C-Town-sized, rows of 7 .. 32 entries / a hub
    "snap_sym": (dict(n=389, symmetric=True, in_rows=(6, 7, 32), last_wave=12, chain=389, at=130, spacing=1, seed=7),
                 SYMMETRIC | DEG_LE32),
    "snap_dir_hub": (dict(n=389, symmetric=False, in_rows=(6, 7, 33), out_rows=(32, 40), last_wave=36, directed=6, chain=389,
                          seed=8), 0),
}


def named(name: str) -> IrregularGraph:
    kw, _ = SPECS[name]
    return build_graph(name, **kw)


def collate(g: IrregularGraph, bs: int) -> torch.Tensor:
    """edge_index of a batch of ``bs`` copies of g (PyG Batch: node ids offset per snapshot)."""
    return torch.cat([g.edge_index + k * g.num_nodes for k in range(bs)], dim=1)


# ------------------------------------------------------------------------------------- random graphs (fuzz tests)
def random_graph(rng: np.random.RandomState, n: int, wdn_topology=None) -> torch.Tensor:
    """One random snapshot: WDN-like (``wdn_topology(n, edges, seed)``, local order), or a random tree with a locality
    window plus extra edges -- undirected ones (degrees beyond 6), directed ones with self loops, or many edges into a
    hub in node 0's neighbourhood -- in local or (30 %) shuffled node order."""
    kind = rng.randint(4)
    if kind == 0:
        return wdn_topology(n, n - 1 + rng.randint(0, max(1, n // 8)), seed=int(rng.randint(1 << 30)))
    src, dst = [], []
    for v in range(1, n):
        u = rng.randint(max(0, v - rng.randint(1, 40)), v)
        src += [u, v]; dst += [v, u]
    extra = rng.randint(0, n)
    for _ in range(extra):
        u, v = rng.randint(n), rng.randint(n)
        if kind == 1 and u != v:
            src += [u, v]; dst += [v, u]
        elif kind == 2:
            src.append(u); dst.append(v)
        elif kind == 3 and u != v:
            w = rng.randint(min(n, 5))
            src += [u, w]; dst += [w, u]
    ei = torch.tensor([src, dst], dtype=torch.int64)
    if rng.rand() < 0.3:
        perm = torch.from_numpy(rng.permutation(n))
        ei = perm[ei]
    return ei[:, torch.argsort(ei[0], stable=True)]


def random_batch(rng: np.random.RandomState, sizes: Sequence[int], wdn_topology=None) -> torch.Tensor:
    tops = [random_graph(rng, n, wdn_topology) for n in sizes]
    offs = np.cumsum([0] + list(sizes))
    return torch.cat([t + int(o) for t, o in zip(tops, offs[:-1])], dim=1)
