"""Plans that agree in every TOTAL (nodes, GATConv edges, segments) and differ in their LARGEST SEGMENT, and the helpers of
the work-buffer tests (tests/test_work_buffers_host.py, tests/test_gpu_work_buffers.py).  A plain module, not a conftest.

The fused kernels take raw pointers to two work buffers and trust the caller for their size.  Both sizes follow the largest
segment (csrc/gatres_layout.h: ``make_layout`` takes ``fused_nodes_of(g)`` and ``max_segment_edges_gat``; the segment-major
``saved`` buffer is ``num_segments * make_seg_layout(.., max_segment_nodes, max_segment_edges_gat).total``), and so do the
parts per segment (k_fused_host.hip: ``fused_split``), whose hand-off epochs persist in the flag lines of scratch.

A batch is a list of seeded ``make_wdn_topology(n, pipes)`` snapshots concatenated with node offsets; a WDN topology is
connected, so every snapshot is one segment, and its plan has ``2 * pipes + n`` GATConv edges.

This module also restates, once, where the persisted hand-off state lies in scratch (``layout_offsets``): ``Layout`` of
csrc/gatres_layout.h up to ``scratch_total``, so that the host test can hold the restatement to the library's
``gatres_scratch_floats`` and ``gatres_fused_status_offset`` before a GPU test writes through it."""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import torch

import fused_plan_refs as FR

NB, NC = 2, 32
TOPO_SEED = 11
FLAG_STRIDE = 32          # words of one part's flag line (k_fused_dev.h); 8 lines per segment
WORD_SYNC, WORD_XCD, WORD_GRANULE = 0, 1, 2          # group_sync epoch | XCD id | granule (hand-off) epoch

# name -> ((nodes per snapshot, pipes per snapshot) of plan A, the same of plan B, whether the GPU tests alternate the two)
PAIRS = {
    # both take the window kernel at 8 parts (14 and 25 tiles); scratch and saved differ through the 214- / 388-row tables
    "same_split": (((214, 214), (236, 236)), ((388, 40), (428, 44)), True),
    # 7 tiles -> at most 7 parts; 11 tiles -> 8
    "different_split": (((112, 112), (124, 124)), ((176, 48), (195, 53)), True),
    # 4100 rows: past the fused path's 4096-row limit, fused_nodes_of() == 0 for B (host only)
    "across_fused_limit": (((2100, 2100), (2310, 2310)), ((4100, 100), (4510, 110)), False),
}
CONTROL = ((388, 40), (428, 44))          # built twice as distinct GraphPlan objects: equal in everything
MIXED_SYM = ((388, 388), (430, 430))      # 8 parts, window kernel, two-sided halos


def batch(sizes, pipes, seed=TOPO_SEED):
    """(edge_index, nodes per graph) of the snapshots ``sizes`` with ``pipes`` pipes each."""
    import gnn_pressure_estimation_amd as G
    tops, off = [], 0
    for k, (n, p) in enumerate(zip(sizes, pipes)):
        tops.append(G.wdn_synth.make_wdn_topology(n, p, seed=seed + k) + off)
        off += n
    return torch.cat(tops, dim=1), [int(n) for n in sizes]


def host_plan(case):
    import gnn_pressure_estimation_amd as G
    ei, npg = batch(*case)
    return G.GraphPlan(ei, sum(npg), device="cpu")


def totals(plan):
    return plan.num_nodes, plan.num_edges_gat, plan.num_segments


def largest(plan):
    return plan.max_segment_nodes, plan.max_segment_edges_gat


def model_struct(nb=NB, nc=NC, flags=0):
    import gnn_pressure_estimation_amd as G
    return G._native.GatresModel(nb, nc, G._native.DTYPE_F32, flags)


def need_floats(lib, plan, nb=NB, nc=NC):
    """(scratch floats, saved floats) the library asks for."""
    m = model_struct(nb, nc)
    return int(lib.gatres_scratch_floats(C.byref(m), plan.ref())), int(lib.gatres_saved_floats(C.byref(m), plan.ref()))


def parts_at(lib, plan, cus=256, nb=NB, nc=NC):
    """GATRES_FUSED_PLAN_PARTS of a training launch on ``cus`` CUs (0: the plan is not fused)."""
    m = model_struct(nb, nc)
    out = (C.c_int32 * len(FR.WORDS))()
    rc = lib.gatres_fused_plan(C.byref(m), plan.ref(), FR.TRAIN, cus, out)
    return int(out[0]) if rc == 0 else 0


# ------------------------------------------------------------------------------------------ the layout, restated
def r4(v):
    return (v + 3) & ~3


def num_slabs_for(P, N):
    cap = (2048 << 20) // (4 * max(P, 1))
    cap = max(16, min(cap, 1024))
    s = min((N + 63) // 64, cap)
    if s > 256:
        s = (s // 256) * 256
    return max(s, 1)


Offsets = namedtuple("Offsets", "sc_flags flag_words status sc_xch xch_stride hb split_max scratch_total")


def layout_offsets(nb, nc, N, Eg, S, mn, me):
    """csrc/gatres_layout.h ``make_layout(m, N, Eg, S, fused_nodes, fused_edges)``, in floats: where the flag lines, the status
    block and the granule exchange regions lie, and the total.  ``mn`` / ``me``: the largest segment's rows / GATConv edges;
    ``mn`` = 0 where the plan is not fused (``fused_nodes_of``)."""
    w = 2 * nc * nc
    P = 2 * nc + nb * (9 * nc + 2 * w) + nc + 1
    s_stride = (r4(N * nc) + r4(N * 2 * nc) + 2 * r4(N * 2) + r4(Eg * 2) + r4(N * 2 * nc) + r4(N * nc) + 2 * r4(N) + r4(Eg))
    o = r4(N * nc) + s_stride + 5 * r4(N * nc)                          # y2 | ev | xa xb gpa gpb gy2
    o += r4(Eg * 2) + 2 * r4(N * 2) + 2 * r4(N * 2 * nc)                # ge | gad gas | gh go1
    o += r4(nb * 2 * w)                                                 # wt
    o += r4(Eg) + 2 * r4(N) + r4(N * nc)                                # ge2 | gad2 gas2 | gh2
    slab_rows = max(num_slabs_for(P, N), S)
    o += slab_rows * r4(P)
    split_max = FR.split_max_for(S) if mn > 0 else 1
    o += r4(max(S * split_max, slab_rows) + 1)                          # loss_part
    keep = r4(N * 2 * nc) + r4(N * nc) + 2 * r4(N * 2) + 2 * r4(N)
    if mn > 0:
        o += nb * keep
    sc_flags = o
    flag_words = r4(FR.padded8(S) * 8 * FLAG_STRIDE + 32)
    col_words = r4(2 * nb + 8)
    if mn > 0:
        o += flag_words + col_words
    if split_max > 1:
        o += S * split_max * r4(P)                                      # part_slabs
    sc_xch, xch_stride, hb = o, 0, 0
    if split_max > 1 and nc <= 32:
        hb = mn * (8 * nc + 3) + 3 * me                                 # make_xch_layout: granules in front of the heartbeats
        xch_stride = 2 * ((hb + 6 * 8 + 15) & ~15)
        o += S * xch_stride
        o += FR.padded8(S) * 8 * 128                                    # urec
    o += r4(nb * 4 * nc * nc)                                           # wb
    o += 4 * r4(N) + r4((N + 3) // 4)                                   # px pout pgout pgx | pmask
    return Offsets(sc_flags, flag_words, sc_flags + flag_words - 32, sc_xch, xch_stride, hb, split_max, o)


def offsets_of(plan, nb=NB, nc=NC):
    mn = plan.max_segment_nodes if plan.num_segments > 0 and 0 < plan.max_segment_nodes <= FR.MAX_FUSED_NODES else 0
    return layout_offsets(nb, nc, plan.num_nodes, plan.num_edges_gat, plan.num_segments, mn, plan.max_segment_edges_gat)


def flags_offset_from_status(status_offset, num_segments):
    """Float index of the flag lines in scratch from what ``gatres_fused_status_offset`` answers: the status block is the last 32
    words of the flag region (gatres_layout.h: fused_status_offset)."""
    return status_offset + 32 - r4(FR.padded8(num_segments) * 8 * FLAG_STRIDE + 32)


# ------------------------------------------------------------------------------------------ the persisted state (GPU tests)
def flag_words_view(scratch, sc_flags, num_segments):
    """int32 view [segments, 8 parts, 32 words] of the flag lines inside ``scratch``."""
    n = num_segments * 8 * FLAG_STRIDE
    assert 0 <= sc_flags and sc_flags + n <= scratch.numel()
    return scratch[sc_flags:sc_flags + n].view(torch.int32).view(num_segments, 8, FLAG_STRIDE)


def read_epochs(scratch, sc_flags, num_segments):
    """(word 0, word 2) of every part of every segment as unsigned values: two int64 tensors [segments, 8] on the host."""
    torch.cuda.synchronize()
    v = flag_words_view(scratch, sc_flags, num_segments).cpu().to(torch.int64) & 0xFFFFFFFF
    return v[:, :, WORD_SYNC].clone(), v[:, :, WORD_GRANULE].clone()


def set_epochs(scratch, offs, num_segments, value, granule=None):
    """Word 0 of every part of every segment = ``value`` (mod 2^32), word 2 = ``granule`` (default: the same value) and the
    heartbeat granules' tags with it -- the state a launch leaves behind after that many hand-offs: every part's last heartbeat
    carries the epoch it stopped at.  The row / edge granules stay zeroed, so no hand-off of the run that follows may carry epoch
    0 before its table has been written once (an unwritten granule would pass for it)."""
    def signed(v):
        v &= 0xFFFFFFFF
        return v - (1 << 32) if v >= (1 << 31) else v
    granule = value if granule is None else granule
    f = flag_words_view(scratch, offs.sc_flags, num_segments)
    f[:, :, WORD_SYNC] = signed(value)
    f[:, :, WORD_GRANULE] = signed(granule)
    if offs.xch_stride > 0:
        assert offs.sc_xch + num_segments * offs.xch_stride <= scratch.numel()
        for s in range(num_segments):
            g0 = offs.sc_xch + s * offs.xch_stride + 2 * offs.hb            # granule = {value, tag}: floats 2 g, 2 g + 1
            scratch[g0:g0 + 2 * 8].view(torch.int32)[1::2] = signed(granule)
    torch.cuda.synchronize()
