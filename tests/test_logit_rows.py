"""The large-logit row builder (tests/logit_rows.py) against its own promises, on the CPU: every graph the softmax tests run
on (tests/test_gpu_softmax_range.py) holds every row family at the places the kernels branch on, read back from the
logits with numpy.  Without this, a later change to the graph builders could leave the GPU tests comparing rows that no
longer reach the code they name."""
import numpy as np
import pytest

import logit_rows as LR

GRAPHS = ("sym_le32", "dir_le32", "sym_hub", "dir_hub_shuffled", "ops_hub", "ops_star")
FEW, MIXED = 4, 6               # the slot paths' row classes: waves whose rows all have <= 4 entries, waves with 5 or 6
# ops_star: node 0 feeds every row and three hubs share their sources, so no row of it can hold tied or saturated maxima and
# only the first hub of a variant its dominant edge where placed; the other graphs hold every family and every hub column
FAMILIES_OF = {"ops_star": ("dominant", "negative", "spread")}


def _case(name, H):
    ei, n = LR.graph(name)
    rows = LR.build(ei, n, H, seed=len(name))
    return rows, LR.families_of(rows)


@pytest.mark.parametrize("H", [1, 2])
@pytest.mark.parametrize("name", GRAPHS)
def test_every_graph_holds_every_family_where_the_kernels_branch(name, H):
    rows, F = _case(name, H)
    n, N = rows.copy_nodes, rows.num_nodes
    deg = F.deg
    dom = F.fam["dominant"]
    for h in range(H):
        for f in FAMILIES_OF.get(name, LR.FAMILIES):
            assert F.fam[f][:, h].sum() >= 4, (f, h)
        # the dominant edge at every slot of every row length 1 .. 6 the graph has
        for d in sorted(set(deg[deg <= 6].tolist())):
            got = set(F.argmax[(deg == d) & dom[:, h], h].tolist())
            assert got == set(range(d)), (h, d, sorted(got))
    # rows of 7 .. 32 entries (the edge-after-edge loop): dominant and all-negative ones
    long_ = (deg >= 7) & (deg <= 32)
    assert long_.any()
    assert (long_ & dom[:, 0]).any() and (long_ & F.fam["negative"][:, 0]).any()
    # hub rows (> 32 entries): dominant in every head, the argmax in every slot column of the hub path (S = 64 / lanes per
    # row: 2 .. 32 columns; slot k takes entries k, k + S, ...)
    hub = deg > 32
    if name == "ops_star":
        assert hub.sum() == 3 * rows.variants and dom[hub].mean() >= 1 / 3
    elif name not in ("sym_le32", "dir_le32"):
        assert hub.any() and dom[hub].all()
        for S in (2, 4, 8, 16, 32):
            assert set((F.argmax[hub, 0] % S).tolist()) == set(range(S)), S
    else:
        assert not hub.any()
    # H = 2: the heads' maxima at different slots
    if H == 2:
        both = dom[:, 0] & dom[:, 1] & (deg >= 2)
        assert both.any() and (F.argmax[both, 0] != F.argmax[both, 1]).mean() > 0.75
        for d in sorted(set(deg[(deg >= 2) & (deg <= 6)].tolist())) if name != "ops_star" else ():
            sel = both & (deg == d)
            assert (F.argmax[sel, 0] != F.argmax[sel, 1]).any(), d
    # waves of 64 rows: the ragged last one, ones whose rows all have <= 4 entries and ones with rows of 5 or 6
    waves = [slice(w, min(w + LR.WAVE, N)) for w in range(0, N, LR.WAVE)]
    fam0 = {f: F.fam[f][:, 0] for f in LR.FAMILIES}

    def families_in(w):
        return {f for f in LR.FAMILIES if fam0[f][w].any()}

    assert N % LR.WAVE, "the union's last wave must be ragged"
    irregular = not name.startswith("ops_")           # (irregular_graphs.py: a long row or hub in the last wave, short waves)
    assert families_in(waves[-1]) >= ({"dominant", "negative"} if irregular else {"negative"})
    few = [w for w in waves if deg[w].max() <= FEW]
    mixed = [w for w in waves if ((deg[w] > FEW) & (deg[w] <= MIXED)).any()]
    want = set(FAMILIES_OF.get(name, LR.FAMILIES))
    if irregular:
        assert few and set().union(*(families_in(w) for w in few)) == want
    if (deg[:n] == 5).any() or (deg[:n] == 6).any():
        assert mixed and set().union(*(families_in(w) for w in mixed)) == want
        in_mixed = np.zeros(N, bool)
        for w in mixed:
            in_mixed[w] = True
        short = in_mixed & (deg <= FEW) & dom[:, 0]        # short rows that take the 6-slot branch: every slot
        assert set(F.argmax[short, 0].tolist()) == set(range(FEW))


def test_all_graphs_together_reach_every_row_length_and_slot():
    """Rows of 1 .. 6 entries with the dominant edge at every slot, rows of 7 .. 32 and hubs, over the graphs together."""
    seen = {}
    for name in GRAPHS:
        _, F = _case(name, 1)
        for d in range(1, 7):
            seen.setdefault(d, set()).update(F.argmax[(F.deg == d) & F.fam["dominant"][:, 0], 0].tolist())
        seen.setdefault("long", set()).update(F.deg[(F.deg >= 7) & (F.deg <= 32)].tolist())
        seen.setdefault("hub", set()).update(F.deg[F.deg > 32].tolist())
    for d in range(1, 7):
        assert seen[d] == set(range(d)), (d, seen[d])
    assert {7, 32} <= seen["long"] and min(seen["hub"]) == 33


def test_exact_families_are_exact_in_fp32():
    """tied / saturated rows: logits formed in fp32 (exact sums of quarter multiples, the LeakyReLU product) keep the exact
    maximum ties and the gaps that make every other alpha exactly 0 in fp32."""
    rows, F = _case("sym_hub", 2)
    src, dst, rowptr = LR.csr(rows.edge_index, rows.num_nodes)
    pre = rows.a_src.numpy()[src] + rows.a_dst.numpy()[dst]                  # fp32
    s = np.where(pre > 0, pre, np.float32(LR.NEG_SLOPE) * pre).astype(np.float32)
    for fam, top in (("tied", None), ("saturated", 150.0)):
        want = LR.exact_rows(rows, F, fam)
        for i, h in zip(*np.nonzero(F.fam[fam])):
            b, e = rowptr[i], rowptr[i + 1]
            r, w = s[b:e, h], want[b:e, h]
            m = r.max()
            assert (r[w > 0] == m).all() and (r[w == 0] <= m - LR.TIE_GAP).all()
            if top is not None:
                assert m == top and (r[w == 0] == -100).all()
            p = np.exp((r - m).astype(np.float32))
            assert (p[w == 0] == 0).all() and (p[w > 0] == 1).all()
