"""Plain-Python restatement of what a fused launch decides from the size of the plan's largest segment: the LDS budget
formulas of csrc/k_fused_dev.h (topo_*_bytes, wl_bytes, cache_fits, nocache_fits, win_*_bytes), the split rules of
csrc/gatres_layout.h (rounds_parts_for, split_max_for) and the decision of csrc/k_fused_host.hip (window_kernel_fits,
fused_split, the facts word, keep-in-LDS, the rounds of a launch), word for word as ``gatres_fused_plan`` reports them, plus the
one rule the cached whole-segment kernel decides for itself (k_fused_whole.hip: the private W slot).

The inputs are a plan's FIGURES only (``Figures``: num_segments, max_segment_*, the 28 window / halo figures, flags) and the
model's (nb, nc) -- never anything the library answered.  Integers throughout; the tests compare with equality."""
from __future__ import annotations

from collections import namedtuple

LDS_BYTES = 163840
PHASE_FORWARD, PHASE_BACKWARD, PHASE_LOSS = 2, 4, 16
TRAIN = PHASE_FORWARD | PHASE_LOSS | PHASE_BACKWARD
GRAPH_DEG_LE6 = 4
MODEL_INFERENCE = 1
E_UNSUPPORTED = -2
FACT_DEG_LE6, FACT_OW64, FACT_INFERENCE, FACT_PROBED = 0x400, 0x1000, 0x2000, 0x4000
WORDS = ("parts", "window", "cached", "keep", "facts", "launches", "per_launch", "grid", "threads", "part_rows", "cus",
         "reserved")
MAX_FUSED_NODES = 4096

# windows: 7 x (window rows, window GATConv edges, window SimpleConv edges) for M = 2 .. 8, then 7 halo figures
Figures = namedtuple("Figures", "num_segments nodes edges_gat edges_mean windows flags")


def figures_of(plan):
    """The figures of a ``GraphPlan``."""
    return Figures(plan.num_segments, plan.max_segment_nodes, plan.max_segment_edges_gat, plan.max_segment_edges_mean,
                   tuple(plan.windows), plan.flags)


def even(v):
    return (v + 1) & ~1


def topo_fwd_bytes(n, eg, em):
    return 2 * (2 * even(n + 1) + even(eg) + even(em))


def topo_bwd_bytes(n, eg, em):
    return 2 * (4 * even(n + 1) + 3 * even(eg) + 2 * even(em))


def wl_floats(nc):
    return 2 * nc * (2 * nc + 4) + 4 * nc


def wl_bytes(nc):
    f = 4 * wl_floats(nc)
    return f + 16 if f <= 40960 else 0


def threads_for(nc):
    return 1024 if nc <= 32 else (512 if nc == 64 else 256)


def cached_fwd_bytes(nc, n, eg, em):
    """Forward LDS of the cached whole-segment kernel: h1 [n][2nc], h2 [n][nc], a_src / a_dst [n][2] each, the topology."""
    return 4 * n * (3 * nc + 4) + topo_fwd_bytes(n, eg, em)


def cache_fits(nc, threads, n, eg, em):
    bwd = 12 * threads + 4 * n * 2 * nc + 8 * even(eg) + 16 * n + topo_bwd_bytes(n, eg, em) + wl_bytes(nc)
    return cached_fwd_bytes(nc, n, eg, em) <= LDS_BYTES and bwd <= LDS_BYTES and max(n, eg, em) <= 65535


def nocache_fits(nc, threads, n, eg, em):
    return 12 * threads + topo_bwd_bytes(n, eg, em) + wl_bytes(nc) <= LDS_BYTES and max(n, eg, em) <= 65535


def priv_w_slot(nc, n, eg, em):
    """The cached kernel's forward: a W slot of its own at the end of LDS if the tables leave room, else proj1 borrows the
    h2 table and proj2 the h1 table."""
    return cached_fwd_bytes(nc, n, eg, em) + 4 * wl_floats(nc) + 16 <= LDS_BYTES


def win_fwd_bytes(nc, wr, ow, ge, gm, hl):
    return (4 * (wr * (3 * nc + 2) + ow * (3 * nc + 2 + 8)) + 2 * (4 * wl_floats(nc) + 16)
            + 2 * (2 * even(ow + 2) + even(ge) + even(gm)) + 64 + 4 * (hl + 4) + 32 * ow + 16 + ow + 16)


def win_bwd_bytes(nc, threads, wr, ow, ge, gm, hl):
    return (12 * threads + 4 * (wr * (4 * nc + 2) + ow * (2 * nc + 4 + 4) + 4 * even(ge)) + 2 * (4 * wl_floats(nc) + 16)
            + 2 * (3 * even(ow + 2) + 3 * even(ge) + even(wr + 2) + even(gm)) + 64 + 8 * (hl + 4) + 80 * ow + 16 + ow + 16)


def win_keep_bytes(nb, ow):
    return (12 * nb * ow + 15) & ~15


def tiles_of(n):
    return (n + 15) // 16


def own_rows(n, M):
    """Own rows of the largest part: the segment's 16-row tiles dealt out over M parts."""
    return 16 * ((tiles_of(n) + M - 1) // M)


def padded8(v):
    return ((v + 7) // 8) * 8


def rounds_parts_for(num_segments):
    padded = padded8(num_segments)
    if padded <= 48 or padded > 96:
        return 0
    return min(8, 256 // padded8(padded // 2))


def split_max_for(num_segments):
    padded = padded8(num_segments)
    if padded <= 0 or padded > 256:
        return 1
    rp = rounds_parts_for(num_segments)
    if rp:
        return rp
    return max(1, min(8, 256 // padded))


def fused_supported(nb, nc, f):
    if f.num_segments <= 0 or not (4 <= nc <= 128 and nc & (nc - 1) == 0) or nc > 32:
        return False
    if f.nodes > MAX_FUSED_NODES:
        return False
    return nocache_fits(nc, threads_for(nc), f.nodes, f.edges_gat, f.edges_mean)


def has_xch(nc, f):
    """Layout.xch_stride > 0: the granule exchange regions exist (split_max > 1, nc <= 32, a fused plan)."""
    return 0 < f.nodes <= MAX_FUSED_NODES and split_max_for(f.num_segments) > 1 and nc <= 32


def window_kernel_fits(nb, nc, f, M, keep=False, ow_tiles_off=0):
    """``ow_tiles_off``: the planted error of the tests (own rows off by that many tiles); 0 is the statement."""
    if M < 2 or M > 8 or nc > 32 or threads_for(nc) != 1024:
        return False
    k = M - 2
    wr, ge, gm, hl = f.windows[3 * k], f.windows[3 * k + 1], f.windows[3 * k + 2], f.windows[21 + k]
    if wr <= 0 or not has_xch(nc, f):
        return False
    ow = own_rows(f.nodes, M) + 16 * ow_tiles_off
    kb = win_keep_bytes(nb, ow) if keep else 0
    return (win_fwd_bytes(nc, wr, ow, ge, gm, hl) + kb <= LDS_BYTES
            and win_bwd_bytes(nc, 1024, wr, ow, ge, gm, hl) + kb + (4 * ow * nc + 16 if keep else 0) <= LDS_BYTES
            and max(wr, ge, gm) <= 65535)


def fused_split(nb, nc, f, cus, split=0, no_rounds=False, **kw):
    """Parts per segment.  ``split``: GATRES_FUSED_SPLIT; ``no_rounds``: GATRES_FUSED_NO_ROUNDS."""
    tiles, padded = tiles_of(f.nodes), padded8(f.num_segments)
    split_max = split_max_for(f.num_segments) if 0 < f.nodes <= MAX_FUSED_NODES else 1
    rp = rounds_parts_for(f.num_segments)
    if rp:
        per = padded8(padded // 2)
        if (split_max == rp and tiles >= rp and nb > 0 and per * rp <= cus and not split and not no_rounds
                and window_kernel_fits(nb, nc, f, rp, **kw)):
            return rp
    B = split_max
    while B > 1 and (B > tiles or nb == 0 or padded * B > cus):
        B -= 1
    if split and 1 <= split <= B:
        return split
    if B >= 2 and window_kernel_fits(nb, nc, f, B, **kw):
        return B
    m = 1
    while m * 2 <= B and m < 4:
        m *= 2
    return m


def fused_plan(nb, nc, f, phases=TRAIN, cus=256, inference=False, probed=False, split=0, no_keep=False, no_rounds=False,
               nocache=False, ow_tiles_off=0):
    """(rc, dict of WORDS) as gatres_fused_plan(model, plan, phases, cus) answers: a launch that is given a saved buffer."""
    zero = dict.fromkeys(WORDS, 0)
    if not fused_supported(nb, nc, f):
        return E_UNSUPPORTED, zero
    kw = dict(ow_tiles_off=ow_tiles_off)
    threads = threads_for(nc)
    M = fused_split(nb, nc, f, cus, split=split, no_rounds=no_rounds, **kw)
    p = dict(zero, parts=M, threads=threads, cus=cus)
    p["window"] = int(threads == 1024 and nc <= 32 and window_kernel_fits(nb, nc, f, M, **kw))
    p["cached"] = int(not nocache and cache_fits(nc, threads, f.nodes, f.edges_gat, f.edges_mean))
    p["part_rows"] = own_rows(f.nodes, M)
    p["facts"] = ((FACT_DEG_LE6 if f.flags & GRAPH_DEG_LE6 else 0) | (FACT_OW64 if p["part_rows"] <= 64 else 0)
                  | (FACT_INFERENCE if inference and phases == PHASE_FORWARD else 0) | (FACT_PROBED if probed else 0))
    p["keep"] = int(bool(phases & PHASE_FORWARD) and bool(phases & PHASE_BACKWARD) and not no_keep
                    and window_kernel_fits(nb, nc, f, M, keep=True, **kw))
    per = f.num_segments
    if M > 1 and padded8(f.num_segments) * M > cus:
        padded, fit = padded8(f.num_segments), (cus // M) & ~7
        rounds = (padded + fit - 1) // fit if fit > 0 else 0
        per = padded8((padded + rounds - 1) // rounds) if rounds > 0 else 0
    p["per_launch"] = per
    p["launches"] = (f.num_segments + per - 1) // per if per > 0 else 0
    p["grid"] = padded8(min(f.num_segments, per)) * M if per > 0 else 0
    return (0 if per > 0 else E_UNSUPPORTED), p


def kind(p, rc=0):
    """A short name of what the plan launches: the kernel, and what the cases distinguish."""
    if rc != 0:
        return "per-op"
    if p["window"]:
        return f"window x{p['parts']}" + (" keep" if p["keep"] else "") + ("" if p["facts"] & FACT_OW64 else " rows>64")
    return f"whole x{p['parts']} " + ("cached" if p["cached"] else "uncached")


def table(nb, nc_list, sizes, figures_for, cus=256):
    """Rows (n, kind per nc) of the "which kernel at which size" table of DESIGN.md 3.1: ``figures_for(n)`` -> Figures."""
    rows = []
    for n in sizes:
        f = figures_for(n)
        rows.append((n, [kind(*reversed(fused_plan(nb, nc, f, cus=cus))) for nc in nc_list]))
    return rows
