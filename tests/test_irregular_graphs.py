"""The irregular-graph builder (tests/irregular_graphs.py) against its own promises, on the CPU: the plan flags the library
derives (gatres_graph_flags_host) and the intended row classes, counted with numpy.  The GPU tests that run kernels on
these graphs rely on what is checked here to reach the code paths they name."""
import ctypes as C

import numpy as np
import pytest
import torch

import irregular_graphs as IG


def _flags(lib, g):
    f = C.c_int32(-1)
    ei = g.edge_index.contiguous()
    assert lib.gatres_graph_flags_host(ei.data_ptr(), ei.shape[1], g.num_nodes, C.byref(f)) == 0
    return int(f.value)


@pytest.mark.parametrize("name", sorted(IG.SPECS))
def test_named_graph_has_its_features(lib, name):
    g = IG.named(name)
    _, want = IG.SPECS[name]
    n, ei = g.num_nodes, g.edge_index
    assert ei.dtype == torch.int64 and ei.shape[0] == 2 and int(ei.min()) >= 0 and int(ei.max()) < n
    assert g.flags == want and _flags(lib, g) == want, (g.flags, want)
    assert not want & IG.DEG_LE6                                     # every graph has a row of more than 6 entries
    assert n % 16 and n % 32 and n % 64                              # ragged tiles, phases and waves
    rc = IG.row_counts(ei, n)
    special = set(g.in_rows.values()) | set(g.out_rows.values()) | ({g.last_wave} if g.last_wave is not None else set())
    for r, v in g.in_rows.items():                                   # the exact boundaries
        assert rc["gat_in"][v] == r, (r, v)
    for r, v in g.out_rows.items():
        assert rc["gat_out"][v] == r, (r, v)
    if want & IG.SYMMETRIC:
        assert set(g.in_rows) >= {6, 7, 32}
    else:
        assert {6, 7, 32} <= set(g.in_rows) | set(g.out_rows)
        assert g.out_rows and set(g.out_rows.values()).isdisjoint(g.in_rows.values())      # out-rows of their own
    if not want & IG.DEG_LE32:
        assert 33 in g.in_rows or 33 in g.out_rows
    # everything else is short: rows of at most 4 entries in every CSR
    ordinary = np.ones(n, bool)
    ordinary[list(special)] = False
    for k in ("gat_in", "gat_out", "mean_in", "mean_out"):
        assert rc[k][ordinary].max() <= 4, k
    longest = max(rc["gat_in"].max(), rc["gat_out"].max())
    assert (longest <= 32) == bool(want & IG.DEG_LE32)
    # a long row (7 .. 32 entries) in a 64-row wave of short rows; waves whose rows are all <= 4 entries
    gin = rc["gat_in"]
    waves = [gin[w:w + IG.WAVE] for w in range(0, n, IG.WAVE)]
    assert any(((w >= 7) & (w <= 32)).any() and (w <= 6).sum() >= 32 for w in waves)
    assert sum(int(w.max() <= 4) for w in waves) >= len(waves) // 2
    if IG.SPECS[name][0].get("spacing") == 1 and not IG.SPECS[name][0].get("shuffle"):
        pair = gin[g.in_rows[6] & ~1:(g.in_rows[6] & ~1) + 2]              # rows 6 and 7 share an aligned pair of rows
        assert sorted(pair.tolist()) == [6, 7]
    # a long row (LE32 graphs) or a hub of more than 32 entries in the ragged last wave
    last = slice(n - n % IG.WAVE, n)
    assert g.last_wave is not None and last.start <= g.last_wave < n
    lw = gin[g.last_wave]
    assert (7 <= lw <= 32) if want & IG.DEG_LE32 else lw > 32
    # isolated nodes, self loops, duplicates, directed edges
    s, d = ei[0].numpy(), ei[1].numpy()
    for v in g.isolated:
        assert rc["mean_in"][v] == 0 and rc["mean_out"][v] == 0 and rc["gat_in"][v] == 1
    assert len(g.isolated) >= 2 and len(g.self_loops) >= 2 and all(((s == v) & (d == v)).any() for v in g.self_loops)
    pairs = s.astype(np.int64) * n + d
    assert g.duplicates >= 2 and len(pairs) - len(np.unique(pairs)) >= g.duplicates
    rev = set((d.astype(np.int64) * n + s).tolist())
    one_way = sum(1 for p, a, b in zip(pairs.tolist(), s, d) if a != b and p not in rev)
    assert (one_way == 0) == bool(want & IG.SYMMETRIC)


def test_local_and_shuffled_orders():
    """Local order: special rows fed by nearby ids (edges span few ids); the shuffled twins spread the same degrees."""
    for local, shuffled in (("sym_le32", "sym_le32_shuffled"), ("dir_hub", "dir_hub_shuffled")):
        a, b = IG.named(local), IG.named(shuffled)
        span = lambda g: float((g.edge_index[0] - g.edge_index[1]).abs().double().median())
        assert span(a) <= 2 and span(b) > 50
        for k in ("gat_in", "gat_out"):
            assert sorted(IG.row_counts(a.edge_index, a.num_nodes)[k]) == sorted(IG.row_counts(b.edge_index, b.num_nodes)[k])


def test_builder_is_seeded():
    a, b = IG.named("dir_le32"), IG.named("dir_le32")
    assert torch.equal(a.edge_index, b.edge_index)
    assert IG.collate(a, 3).shape[1] == 3 * a.edge_index.shape[1] and int(IG.collate(a, 3).max()) < 3 * a.num_nodes
