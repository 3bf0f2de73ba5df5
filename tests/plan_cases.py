"""The graphs of the plan-table tests, each named for what it reaches, and ``features``: a numpy statement of which of
the builder's turnovers a graph reaches when its segments are carried by M parts (derived from edge_index alone).

  * every named graph of tests/irregular_graphs.py, alone and collated twice, and three seeded random batches;
  * one-segment graphs of n = 1, 15, 16, 17 and 16 M - 1, 16 M, 16 M + 1 nodes for M = 2 .. 8 (a path plus a few chords):
    empty parts, parts of one tile, parts of a single row;
  * an edgeless graph, a directed path, fans of directed edges (parts without out-edges / without in-edges of their own),
    a SimpleConv row of 0 entries next to a self loop, crossing duplicates, and the ragged batch [17, 130, 389]."""
from __future__ import annotations

from typing import Dict, List, Set, Tuple

import numpy as np
import torch

import irregular_graphs as IG
from plan_refs import part_rows, segments_ref

MS = tuple(range(2, 9))
RAGGED_SIZES = (17, 130, 389)


def _ei(pairs) -> torch.Tensor:
    return torch.tensor(sorted(pairs) if isinstance(pairs, set) else list(pairs), dtype=torch.int64).reshape(-1, 2).t().contiguous()


def path_with_chords(n: int) -> torch.Tensor:
    """Symmetric path 0 - 1 - ... - n-1 with a chord (i, i + 5) at every 7th node: one segment, rows of at most 5 entries."""
    pairs = []
    for i in range(n - 1):
        pairs += [(i, i + 1), (i + 1, i)]
    for i in range(0, n - 5, 7):
        pairs += [(i, i + 5), (i + 5, i)]
    return _ei(pairs)


def edgeless(n: int = 40) -> torch.Tensor:
    return torch.zeros((2, 0), dtype=torch.int64)


def directed_path(n: int = 50) -> torch.Tensor:
    """i -> i + 1 only: the first row has no SimpleConv in-edge, the last no out-edge (inside a part that has some)."""
    return _ei([(i, i + 1) for i in range(n - 1)])


def fan_out(n: int = 130) -> torch.Tensor:
    """Nodes 0 .. 15 are sources, every other node a sink fed by node j % 16: the parts past the first tile have no
    out-edges of their own, the first tile's out-rows have more than 6 entries."""
    return _ei([(j % 16, j) for j in range(16, n)])


def fan_in(n: int = 130) -> torch.Tensor:
    return fan_out(n).flip(0).contiguous()


def loop_next_to_empty_row(n: int = 40) -> torch.Tensor:
    """A directed path with a self loop on node 1: row 0 has no SimpleConv entry, its neighbour row 1 has the loop, which
    SimpleConv keeps and GATConv replaces."""
    return torch.cat([directed_path(n), _ei([(1, 1), (1, 1), (n - 2, n - 2)])], dim=1)


def crossing_duplicates(n: int = 131) -> torch.Tensor:
    """A symmetric path whose edges across every 16-row boundary are listed twice, the higher row's first, plus long directed
    chords listed far row first: duplicate remote edges, and remote out-edges whose saved ids are not in row order."""
    pairs = []
    for i in range(n - 1):
        rep = 2 if (i + 1) % 16 == 0 else 1
        pairs += [(i + 1, i), (i, i + 1)] * rep
    for i in range(0, n - 40, 9):
        pairs += [(i, i + 40), (i, i + 20)]
    return _ei(pairs)


def ragged_batch() -> Tuple[torch.Tensor, List[int]]:
    """Snapshots of 17, 130 and 389 nodes (water-network-like, local order): a segment of 2 tiles next to one of 25."""
    from gnn_pressure_estimation_amd import wdn_synth
    tops = [wdn_synth.make_wdn_topology(n, n + max(1, n // 9), seed=40 + k) for k, n in enumerate(RAGGED_SIZES)]
    offs = np.cumsum([0] + list(RAGGED_SIZES))
    return torch.cat([t + int(o) for t, o in zip(tops, offs[:-1])], dim=1), list(RAGGED_SIZES)


def small_sizes() -> List[int]:
    return sorted({1, 15, 16, 17} | {16 * m + d for m in MS for d in (-1, 0, 1)})


_CASES: Dict[str, Tuple[torch.Tensor, int]] = {}


def cases() -> Dict[str, Tuple[torch.Tensor, int]]:
    """name -> (edge_index, num_nodes); built once."""
    if _CASES:
        return _CASES
    from gnn_pressure_estimation_amd import wdn_synth
    for name in IG.SPECS:
        g = IG.named(name)
        _CASES[name] = (g.edge_index, g.num_nodes)
        _CASES[name + "_x2"] = (IG.collate(g, 2), 2 * g.num_nodes)
    for seed, sizes in ((11, [17, 33, 60, 200]), (12, [388, 120, 450]), (13, [200, 17, 388, 33])):
        ei = IG.random_batch(np.random.RandomState(seed), sizes, wdn_synth.make_wdn_topology)
        _CASES[f"random_batch_{seed}"] = (ei, int(sum(sizes)))
    for n in small_sizes():
        _CASES[f"path_{n}"] = (path_with_chords(n), n)
    _CASES["edgeless_40"] = (edgeless(40), 40)
    _CASES["directed_path_50"] = (directed_path(50), 50)
    _CASES["fan_out_130"] = (fan_out(130), 130)
    _CASES["fan_in_130"] = (fan_in(130), 130)
    _CASES["loop_next_to_empty_row_40"] = (loop_next_to_empty_row(40), 40)
    _CASES["crossing_duplicates_131"] = (crossing_duplicates(131), 131)
    ei, sizes = ragged_batch()
    _CASES["ragged_17_130_389"] = (ei, int(sum(sizes)))
    return _CASES


# Every feature must be reached by some case at EVERY M = 2 .. 8 (each can occur at each: test_plan_tables_host.py).
FEATURES = (
    "empty_part",                          # more parts than 16-row tiles
    "short_part",                          # a part of fewer than 16 rows
    "one_tile_part",                       # a part of exactly 16 rows
    "several_segments", "ragged_segments",
    "gat_in_row_gt6", "gat_out_row_gt6", "mean_in_row_gt6", "mean_out_row_gt6",
    "mean_in_row_zero", "mean_out_row_zero_among_out_edges", "part_without_mean_out_edges", "part_without_mean_in_edges",
    "self_loop", "mean_in_row_zero_next_to_self_loop", "duplicate_edge",
    "remote_edge_both_directions", "remote_edge_one_direction", "duplicate_remote_edge",
    "remote_out_edges_not_in_saved_order",        # the sort of b_hedge moves something
    "padded_out_slot_names_row_without_in_edges",  # mout's max(in-degree, 1) is what is stored
    "window_wider_than_own_rows", "directed",
)


def features(ei: torch.Tensor, n: int, M: int, merge_upto: int = 64) -> Set[str]:
    src, dst = ei[0].numpy().astype(np.int64), ei[1].numpy().astype(np.int64)
    seg = segments_ref(ei, n, merge_upto)[0]
    ns = len(seg) - 1
    part = np.empty(n, dtype=np.int64)
    rows = np.zeros(ns * M, dtype=np.int64)
    for s in range(ns):
        a, cnt = int(seg[s]), int(seg[s + 1] - seg[s])
        for p in range(M):
            lo, hi = part_rows(cnt, p, M)
            part[a + lo:a + hi] = s * M + p
            rows[s * M + p] = hi - lo
    nl = src != dst
    got = set()
    put = lambda name, cond: got.add(name) if bool(cond) else None
    put("empty_part", (rows == 0).any())
    put("short_part", ((rows > 0) & (rows < 16)).any())
    put("one_tile_part", (rows == 16).any())
    put("several_segments", ns > 1)
    put("ragged_segments", len(set(np.diff(seg).tolist())) > 1)
    m_in, m_out = np.bincount(dst, minlength=n), np.bincount(src, minlength=n)
    put("gat_in_row_gt6", (np.bincount(dst[nl], minlength=n) + 1 > 6).any())
    put("gat_out_row_gt6", (np.bincount(src[nl], minlength=n) + 1 > 6).any())
    put("mean_in_row_gt6", (m_in > 6).any())
    put("mean_out_row_gt6", (m_out > 6).any())
    put("mean_in_row_zero", (m_in == 0).any())
    part_out = np.bincount(part, weights=m_out, minlength=ns * M)
    part_in = np.bincount(part, weights=m_in, minlength=ns * M)
    put("mean_out_row_zero_among_out_edges", ((m_out == 0) & (part_out[part] > 0)).any())
    put("part_without_mean_out_edges", ((rows > 0) & (part_out == 0)).any())
    put("part_without_mean_in_edges", ((rows > 0) & (part_in == 0)).any())
    loops = np.zeros(n, dtype=bool)
    loops[src[~nl]] = True
    put("self_loop", loops.any())
    z = m_in == 0
    put("mean_in_row_zero_next_to_self_loop",
        (z[:-1] & loops[1:] & (part[:-1] == part[1:])).any() or (z[1:] & loops[:-1] & (part[:-1] == part[1:])).any())
    pairs = src * n + dst
    put("duplicate_edge", np.unique(pairs).size < pairs.size)
    cross = nl & (part[src] != part[dst])
    cp = pairs[cross]
    back = set((dst[cross] * n + src[cross]).tolist())
    have = set(pairs.tolist())
    put("remote_edge_both_directions", any(k in have for k in back))
    put("remote_edge_one_direction", any(k not in have for k in back))
    put("duplicate_remote_edge", np.unique(cp).size < cp.size)
    put("window_wider_than_own_rows", cross.any())
    put("directed", any((d * n + s) not in have for s, d in zip(src[nl].tolist(), dst[nl].tolist())))
    # saved-edge ids (positions in the destination-sorted GATConv edge list) of the remote out-edges of a part, in the
    # order the source-sorted list visits them
    gs, gd = np.concatenate([src[nl], np.arange(n)]), np.concatenate([dst[nl], np.arange(n)])
    order = np.argsort(gd, kind="stable")
    pos = np.empty_like(order); pos[order] = np.arange(order.size)
    t = np.argsort(gs, kind="stable")
    t = t[part[gs[t]] != part[gd[t]]]
    owner, ids = part[gs[t]], pos[t]
    put("remote_out_edges_not_in_saved_order", ((owner[1:] == owner[:-1]) & (ids[1:] < ids[:-1])).any())
    put("padded_out_slot_names_row_without_in_edges", ((m_in == 0) & (m_out < 6)).any())
    return got
