"""Batches on either side of every size at which the fused path's LDS plan turns over, found by SEARCH with the restatement
(tests/fused_plan_refs.py) on the figures of the ``GraphPlan`` the batch really gets -- its relabelling moves the window
figures, so no size is written down here.

A batch is ``[n, 40]``: one seeded ``make_wdn_topology(n, 11 n / 10)`` snapshot and a 40-node one behind it, so the batch is
ragged and its second segment has fewer 16-row tiles (3) than the launch has parts.  Two segments leave the split at its
maximum of 8 on 256 CUs.  For every width nc in NCS and every turnover the module returns the LARGEST n on the low side and the
SMALLEST on the high side (adjacent sizes n, n + 1):

  keep        window kernel with keep-in-LDS       -> window kernel without (training launch)
  rows64      window parts of at most 64 own rows  -> of 80 (launch fact 0x1000 dropped)
  window      window kernel                        -> whole-segment kernel at min(B, 4) parts
  cache       whole-segment kernel, cached tables  -> uncached; unsplit (GATRES_FUSED_SPLIT=1), at the split the plan chooses,
                                                      and at a forced split of 2 or 4 where that is the whole-segment kernel
  wslot       cached kernel, private W slot        -> borrowed (decided in the kernel; the restatement's priv_w_slot)
  supported   uncached kernel                      -> per-op path (nocache_fits, or the 4096-node cap)

A turnover that no size from LO to HI reaches at some width (or whose far side is not the kind it should be) is listed in
``unreachable()`` with the reason, and is not forced."""
from __future__ import annotations

import functools

import torch

import fused_plan_refs as FR

NCS = (8, 16, 32)
SMALL, SMALL_PIPES = 40, 44
TOPO_SEED = 3
LO, HI, STEP = 48, 4200, 128            # sizes searched: a coarse grid, then bisection between two grid points


def batch(n):
    """(edge_index, nodes per graph) of the batch [n, 40]."""
    import gnn_pressure_estimation_amd as G
    big = G.wdn_synth.make_wdn_topology(n, (11 * n) // 10, seed=TOPO_SEED)
    small = G.wdn_synth.make_wdn_topology(SMALL, SMALL_PIPES, seed=TOPO_SEED + 1)
    return torch.cat([big, small + n], dim=1), [n, SMALL]


@functools.lru_cache(maxsize=None)
def figures(n):
    """The figures of the plan the batch [n, 40] gets (segments, relabelling and windows as GraphPlan decides them)."""
    import gnn_pressure_estimation_amd as G
    ei, npg = batch(n)
    f = FR.figures_of(G.GraphPlan(ei, sum(npg), device="cpu"))
    assert f.num_segments == 2 and f.nodes == n
    return f


def _is(window=None, keep=None, ow64=None, cached=None, parts=None):
    def check(rc, p):
        return (rc == 0 and (window is None or p["window"] == window) and (keep is None or p["keep"] == keep)
                and (ow64 is None or bool(p["facts"] & FR.FACT_OW64) == ow64) and (cached is None or p["cached"] == cached)
                and (parts is None or p["parts"] == parts))
    return check


def _priv(want):
    def check(rc, p, nc, f):
        return rc == 0 and not p["window"] and p["cached"] == 1 and FR.priv_w_slot(nc, f.nodes, f.edges_gat, f.edges_mean) == want
    return check


# turnover -> (nb, the GATRES_FUSED_SPLIT values tried in turn (0: the plan's choice), low side, high side)
TURNOVERS = {
    "keep": (2, (0,), _is(window=1, keep=1), _is(window=1, keep=0)),
    "rows64": (2, (0,), _is(window=1, ow64=True), _is(window=1, ow64=False)),
    "window": (2, (0,), _is(window=1), _is(window=0, parts=4)),
    "cache_unsplit": (2, (1,), _is(window=0, cached=1, parts=1), _is(window=0, cached=0, parts=1)),
    "cache_chosen": (2, (0,), _is(window=0, cached=1), _is(window=0, cached=0)),
    "cache_split": (2, (2, 4), _is(window=0, cached=1), _is(window=0, cached=0)),
    "wslot_unsplit": (2, (1,), _priv(True), _priv(False)),
    "wslot_split": (2, (2, 4), _priv(True), _priv(False)),
    "supported": (1, (0,), _is(window=0, cached=0), lambda rc, p: rc == FR.E_UNSUPPORTED),
}


def _side(check, nb, nc, n, split):
    f = figures(n)
    rc, p = FR.fused_plan(nb, nc, f, cus=256, split=split)
    try:
        return check(rc, p)
    except TypeError:
        return check(rc, p, nc, f)


def _boundary(low):
    """Adjacent sizes (n, n + 1) with low(n) and not low(n + 1): the first such pair going up the coarse grid."""
    prev = None
    for n in range(LO, HI + 1, STEP):
        if low(n):
            prev = n
        elif prev is not None:
            a, b = prev, n
            while b - a > 1:
                mid = (a + b) // 2
                a, b = (mid, b) if low(mid) else (a, mid)
            return a, b
    return None


@functools.lru_cache(maxsize=None)
def _search():
    cases, missing = [], []
    for nc in NCS:
        for name, (nb, splits, low, high) in TURNOVERS.items():
            why = None
            for split in splits:
                pair = _boundary(lambda n: _side(low, nb, nc, n, split))
                if pair is None:
                    why = f"no size from {LO} to {HI} has the low side next to another kind (GATRES_FUSED_SPLIT={split})"
                    continue
                if not _side(high, nb, nc, pair[1], split):
                    rc, p = FR.fused_plan(nb, nc, figures(pair[1]), split=split)
                    why = f"above n = {pair[0]} the plan is '{FR.kind(p, rc)}', not the high side (GATRES_FUSED_SPLIT={split})"
                    continue
                for side, n in zip(("low", "high"), pair):
                    rc, p = FR.fused_plan(nb, nc, figures(n), split=split)
                    cases.append(dict(id=f"nc{nc}_{name}_{side}_n{n}", turnover=name, side=side, nc=nc, nb=nb, n=n, split=split,
                                      neighbour=pair[1] if side == "low" else pair[0], rc=rc, plan=p, kind=FR.kind(p, rc)))
                why = None
                break
            if why:
                missing.append((nc, name, why))
    return tuple(cases), tuple(missing)


def cases():
    """Every case: dict(id, turnover, side, nc, nb, n, split (GATRES_FUSED_SPLIT, 0 = unset), neighbour (the size on the other
    side), rc and plan (the restatement's answer for a training launch at 256 CUs), kind)."""
    return list(_search()[0])


def unreachable():
    """(nc, turnover, reason) of every turnover that is not reached."""
    return list(_search()[1])


def markdown_table(sizes=(389, 512, 513, 600, 700, 1100, 1500, 2000, 2500, 3000, 3700, 4000, 4096, 4097), nb=2):
    """The "which kernel at which size" table of DESIGN.md 3.1 (python tests/fused_plan_cases.py): batches [n, 40], 256 CUs."""
    rows = FR.table(nb, NCS, sizes, figures)
    lines = ["| n | " + " | ".join(f"nc {nc}" for nc in NCS) + " |", "|---|" + "---|" * len(NCS)]
    lines += [f"| {n} | " + " | ".join(kinds) + " |" for n, kinds in rows]
    return "\n".join(lines)


def check_side(case):
    """The restated plan of ``case`` is on the side the case is named for."""
    nb, _, low, high = TURNOVERS[case["turnover"]]
    return _side(low if case["side"] == "low" else high, nb, case["nc"], case["n"], case["split"])


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print(markdown_table())
    for c in cases():
        print(f"{c['id']:<36} nb{c['nb']} GATRES_FUSED_SPLIT={c['split']}  {c['kind']}")
    for nc, name, why in unreachable():
        print(f"nc{nc} {name}: not reached: {why}")
