"""Attention-logit rows at large and saturated logits for the softmax tests (numpy + torch CPU; imported by tests, not a
conftest).

GATConv's softmax subtracts the row's maximum logit m before the exponential.  Any m that is uniform across a row gives the
right alpha while every s_e - m stays within about +-80 (fp32 exp neither overflows nor underflows), so unit-scale inputs
cannot tell a wrong m from the right one.  ``build`` places per-node a_src and per-row a_dst (fp32 [N, H]) on a graph so
that its GATConv rows (logits s_e = leaky(a_src[j] + a_dst[i]), after the LeakyReLU) fall into named families:

  * dominant:  one edge at least 100 above every other (a row of one entry: its logit is >= 100); the argmax is placed at
               every CSR slot of rows of 1 .. 6 entries, at cycling slots of longer rows, and at slot (v + 16 q) of the q-th
               hub row of variant v, so that 16 variants and two hubs (32 variants, one hub) reach every hub slot column (S <= 32);
  * negative:  every logit <= -100 (pre-activations <= -500): a row-uniform m of 0 underflows the whole row;
  * tied:      two edges share the exact maximum, every other is >= 104 below it: alpha = 0.5, 0.5 and exactly 0;
  * saturated: one edge at +150, every other at exactly -100: alpha = 1 and exactly 0;
  * spread:    a_src within 80 of each other (pre-activations in [-40, 40]): a well-conditioned control.

Every a_src / a_dst is a multiple of 1/4 below 2^20, so a_src + a_dst is exact in fp32 and the tied / saturated rows have
exact alphas.  H = 2: head 1 is placed on its own, its argmax one slot after head 0's.  ``union`` stacks V variants of a
graph as one disjoint union (node ids offset per copy), so one launch covers all of them.  ``classify`` reads the families
back from the logits themselves (the tests and the CPU coverage test rely on it, not on what ``build`` intended)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional

import numpy as np
import torch

FAMILIES = ("dominant", "negative", "tied", "saturated", "spread")
GAP = 100.0            # dominant: top-two logit gap
TIE_GAP = 104.0        # tied: exp(-104) rounds to 0 in fp32
NEG_SLOPE = 0.2
VARIANTS = 16
WAVE = 64
_STEP = 200.0          # a_src gap below a row's maximum (logit gap >= 0.8 top + 40 >= 120 with the top at >= 100)
_LIMIT = 2.0 ** 19


def csr(edge_index: torch.Tensor, n: int):
    """(src, dst, rowptr) of GATConv's edges in the plan's destination-sorted order (self loops dropped, one added per node
    after a node's other in-edges: include/gatres.h, graph plan)."""
    ei = edge_index[:, edge_index[0] != edge_index[1]]
    loops = torch.arange(n, dtype=ei.dtype)
    src, dst = torch.cat([ei[0], loops]), torch.cat([ei[1], loops])
    order = torch.sort(dst, stable=True).indices
    src, dst = src[order].numpy(), dst[order].numpy()
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=n))])
    return src, dst, rowptr


def _q(x):
    return np.round(np.asarray(x, np.float64) * 4.0) / 4.0


def _place_head(src, rowptr, n, h, variant, rng):
    """Greedy placement of one head: rows in priority order (hubs, long rows, then the rest), each given a target family
    and argmax slot; a source already fixed by an earlier row constrains the later ones, and a row whose target cannot be
    met with them becomes 'negative' (always possible: a_dst alone moves the whole row below -100)."""
    val = np.full(n, np.nan)
    a_dst = np.zeros(n)
    deg = np.diff(rowptr)
    rank = np.where(deg > 32, 0, np.where((deg == 5) | (deg == 6), 1, np.where(deg > 6, 2, 7 - np.minimum(deg, 4))))
    order = np.argsort(rank, kind="stable")          # hubs, rows of 5 / 6, rows of 7 .. 32, then by length in CSR order
    seen: Dict[int, int] = {}
    hubs = 0

    def free_below(js, top, lo=_STEP, span=800):
        for j in js:
            if np.isnan(val[j]):
                val[j] = _q(top - lo - 0.25 * rng.randint(0, 4 * span))

    for i in order:
        b, e = rowptr[i], rowptr[i + 1]
        d = e - b
        js = src[b:e]
        k = seen.get(min(d, 33), 0)
        seen[min(d, 33)] = k + 1
        if d > 32:
            fam, p = "dominant", (variant + 16 * hubs + h) % d
            hubs += 1
        elif d == 1:
            fam, p = ("dominant", "negative")[(k + variant + h) % 2], 0
        else:
            fam = FAMILIES[(k // d + variant // d) % 5] if d <= 6 else FAMILIES[(k + variant) % 5]
            p = (k + variant + h) % d
        got = val[js]
        known = ~np.isnan(got)
        centre = float(np.mean(got[known])) if known.any() else _q(rng.uniform(-300, 300))
        ok = False
        if fam == "dominant" and d > 32:                            # hubs: the first feasible slot of p's column mod 32
            for p in range(p, d, 32):
                jp = js[p]
                others = js[js != jp]
                om = np.nanmax(val[others]) if not np.isnan(val[others]).all() else -np.inf
                if (js == jp).sum() == 1 and (np.isnan(val[jp]) or val[jp] - om >= _STEP):
                    break
        if fam == "dominant":
            jp = js[p]
            others = js[js != jp]
            if (js == jp).sum() == 1:
                om = np.nanmax(val[others]) if len(others) and not np.isnan(val[others]).all() else -np.inf
                if np.isnan(val[jp]):
                    val[jp] = _q((om if np.isfinite(om) else centre) + _STEP + 0.25 * rng.randint(0, 400))
                if val[jp] - om >= _STEP and abs(val[jp]) < _LIMIT:
                    free_below(others, val[jp])
                    a_dst[i] = _q(100 + 0.25 * rng.randint(0, 200) - val[jp])
                    ok = True
        elif fam == "saturated":
            jp = js[p]
            others = js[js != jp]
            if (js == jp).sum() == 1:
                ov = val[others][~np.isnan(val[others])]
                if len(np.unique(ov)) <= 1 and not (len(ov) and not np.isnan(val[jp]) and ov[0] != val[jp] - 650):
                    if np.isnan(val[jp]):
                        val[jp] = ov[0] + 650 if len(ov) else _q(centre + 650)
                    val[others] = val[jp] - 650
                    a_dst[i] = 150 - val[jp]
                    ok = abs(val[jp]) < _LIMIT
        elif fam == "tied":
            q = (p + 1) % d
            jp, jq = js[p], js[q]
            others = js[(js != jp) & (js != jq)]
            if jp != jq and (js == jp).sum() == 1 and (js == jq).sum() == 1:
                top = [val[jp], val[jq]]
                kt = [t for t in top if not np.isnan(t)]
                om = np.nanmax(val[others]) if len(others) and not np.isnan(val[others]).all() else -np.inf
                if len(kt) < 2 or kt[0] == kt[1]:
                    t = kt[0] if kt else _q(max(centre, om + _STEP) + 0.25 * rng.randint(0, 400))
                    if t - om >= _STEP and abs(t) < _LIMIT:
                        val[jp] = val[jq] = t
                        free_below(others, t)
                        a_dst[i] = _q(100 + 0.25 * rng.randint(0, 200) - t)
                        ok = True
        elif fam == "spread":
            kv = got[known]
            lo, hi = (kv.min(), kv.max()) if len(kv) else (centre, centre)
            if hi - lo <= 80:
                mid = (lo + hi) / 2
                for j in js:
                    if np.isnan(val[j]):
                        val[j] = _q(np.clip(mid + rng.uniform(-40, 40), hi - 80, lo + 80))
                v = val[js]
                a_dst[i] = -_q((v.min() + v.max()) / 2)
                ok = True
        if not ok:                                                  # negative: every pre-activation <= -500
            for j in js:
                if np.isnan(val[j]):
                    val[j] = _q(centre + rng.uniform(-300, 300))
            a_dst[i] = _q(-np.max(val[js]) - 500 - 0.25 * rng.randint(0, 400))
    return val, a_dst


@dataclass
class Rows:
    edge_index: torch.Tensor       # int64 [2, E] of the union of the variants
    num_nodes: int
    a_src: torch.Tensor            # fp32 [N, H]
    a_dst: torch.Tensor            # fp32 [N, H]
    variants: int
    copy_nodes: int                # nodes per variant


def graph(name: str):
    """(edge_index, num_nodes) of the graphs the softmax tests run on: tests/irregular_graphs.py's named graphs, and the
    random graphs of test_gpu_ops.py with a 39-entry hub row ("ops_hub") or whole-wave hubs in and out ("ops_star")."""
    if name == "ops_hub":
        from test_gpu_ops import graph as ops_graph
        return ops_graph(97, 260, 7, self_loops=3, dup=5, hub=True), 97
    if name == "ops_star":
        from test_gpu_ops import graph as ops_graph
        return ops_graph(203, 500, 7, self_loops=2, dup=4, star=True), 203
    import irregular_graphs as IG
    g = IG.named(name)
    return g.edge_index, g.num_nodes


def union(edge_index: torch.Tensor, n: int, variants: int) -> torch.Tensor:
    return torch.cat([edge_index + k * n for k in range(variants)], dim=1)


def build(edge_index: torch.Tensor, n: int, H: int, variants: Optional[int] = None, seed: int = 0) -> Rows:
    """a_src / a_dst for ``variants`` copies of the graph (one disjoint union; default 16, and 32 for graphs of fewer than
    500 nodes, whose one hub needs 32 variants to reach 32 hub slot columns); see the module's docstring."""
    variants = variants or (VARIANTS if n >= 500 else 2 * VARIANTS)
    ei = union(edge_index, n, variants)
    src, _, rowptr = csr(edge_index, n)
    a_s = np.zeros((variants * n, H))
    a_d = np.zeros((variants * n, H))
    for v in range(variants):
        for h in range(H):
            rng = np.random.RandomState(seed * 7919 + 31 * v + h)
            val, ad = _place_head(src, rowptr, n, h, v, rng)
            a_s[v * n:(v + 1) * n, h] = val
            a_d[v * n:(v + 1) * n, h] = ad
    assert np.isfinite(a_s).all() and np.abs(a_s).max() < 2.0 ** 20 and np.abs(a_d).max() < 2.0 ** 20
    assert (_q(a_s) == a_s).all() and (_q(a_d) == a_d).all()
    return Rows(ei, variants * n, torch.from_numpy(a_s).float(), torch.from_numpy(a_d).float(), variants, n)


def logits(src, dst, a_s, a_d):
    """fp64 logits [E', H] after the LeakyReLU (exact pre-activations: the inputs are multiples of 1/4)."""
    pre = a_s.double().numpy()[src] + a_d.double().numpy()[dst]
    return np.where(pre > 0, pre, NEG_SLOPE * pre)


def weighted_scale(s, dst, n):
    """[N, H]: the largest |s| over each row's edges that carry weight in fp32 (s >= m - 104), the maximum m included --
    the logit scale L of the tolerance the softmax tests use."""
    H = s.shape[1]
    m = np.full((n, H), -np.inf)
    np.maximum.at(m, dst, s)
    live = s >= m[dst] - TIE_GAP
    L = np.zeros((n, H))
    np.maximum.at(L, dst, np.where(live, np.abs(s), 0.0))
    return L


@dataclass
class Families:
    fam: Dict[str, np.ndarray]     # family -> bool [N, H]
    argmax: np.ndarray             # int [N, H]: CSR slot of the row's maximum (first one)
    deg: np.ndarray                # int [N]
    span: np.ndarray               # [N, H]: max_e |a_src[j] + a_dst[i]| over the row (the tolerance's logit scale)


def classify(src, dst, rowptr, s, pre_abs) -> Families:
    """Families of every (row, head) read from its logits ``s`` [E', H] (rows: CSR ``rowptr``)."""
    n, H = len(rowptr) - 1, s.shape[1]
    deg = np.diff(rowptr)
    fam = {f: np.zeros((n, H), bool) for f in FAMILIES}
    arg = np.zeros((n, H), np.int64)
    span = np.zeros((n, H))
    for i in range(n):
        b, e = rowptr[i], rowptr[i + 1]
        for h in range(H):
            r = s[b:e, h]
            span[i, h] = pre_abs[b:e, h].max()
            srt = np.sort(r)[::-1]
            arg[i, h] = int(np.argmax(r))
            top = srt[0]
            fam["negative"][i, h] = top <= -100
            if len(r) == 1:
                fam["dominant"][i, h] = top >= GAP
                continue
            fam["dominant"][i, h] = top - srt[1] >= GAP
            fam["tied"][i, h] = srt[0] == srt[1] and (len(r) == 2 or top - srt[2] >= TIE_GAP)
            fam["saturated"][i, h] = top == 150 and (np.sort(r)[:-1] == -100).all()
            fam["spread"][i, h] = top - srt[-1] <= 80 and np.abs(r).max() <= 40
    return Families(fam, arg, deg, span)


def families_of(rows: Rows) -> Families:
    src, dst, rowptr = csr(rows.edge_index, rows.num_nodes)
    s = logits(src, dst, rows.a_src, rows.a_dst)
    pre = np.abs(rows.a_src.double().numpy()[src] + rows.a_dst.double().numpy()[dst])
    return classify(src, dst, rowptr, s, pre)


def exact_rows(rows: Rows, F: Families, which: str):
    """(edge positions, expected alpha) of every tied / saturated row: alpha 0.5 / 1 on the maxima, exactly 0 elsewhere."""
    src, dst, rowptr = csr(rows.edge_index, rows.num_nodes)
    s = logits(src, dst, rows.a_src, rows.a_dst)
    want = np.full(s.shape, np.nan)
    for i, h in zip(*np.nonzero(F.fam[which])):
        b, e = rowptr[i], rowptr[i + 1]
        r = s[b:e, h]
        want[b:e, h] = np.where(r == r.max(), 0.5 if which == "tied" else 1.0, 0.0)
    return want
