"""numpy restatements of the host plan builder (csrc/graph_plan.hip), for the host tests.

Everything here is derived from ``edge_index``, ``N``, ``merge_upto`` and ``M`` alone -- never from an array the library
returned.  ``ref_plan`` restates gatres_graph_build_host, ``segments_ref`` gatres_graph_segments_host, ``windows_ref``
gatres_graph_windows_host and ``part_record_ref`` one record of gatres_graph_part_tables_host, table by table as the
layout comment of that function and k_window_stages.h (build_nbr_in / build_nbr_out) state them.  ``decode_record`` takes
a record of the library apart into the same dict.  All values are integers: the tests compare with equality."""
from __future__ import annotations

import numpy as np

PT_FIELDS = ("MAGIC", "M", "N0", "N", "E0", "EM0", "T0", "MT0", "LO", "HI", "WLO", "WHI", "ELO", "OEG", "EWLO", "WEG",
             "MELO", "OEM", "TLO", "OTG", "MTLO", "OTM", "F_IMG", "F_IMG_WORDS", "F_HLIST", "F_HCNT", "F_ELIST", "F_ECNT",
             "B_IMG", "B_IMG_WORDS", "B_HROW", "B_HRCNT", "B_HEDGE", "B_HECNT", "B_EROW", "B_ERCNT", "B_EEDGE", "B_EECNT")
PT_HEADER = 48                       # GATRES_PT_HEADER (include/gatres.h); words 38 .. 47 are reserved zeros
PT_MAGIC = 0x47545031
MAXD = 6                             # slots of an edge descriptor (k_fused_dev.h)
LISTS = ("f_hlist", "f_elist", "b_hrow", "b_hedge", "b_erow", "b_eedge")
F_TABLES = ("rpo", "colo", "mrpo", "mcolo", "nbin", "mbin")
B_TABLES = ("b_rpo", "b_colo", "trpo", "teido", "tdsto", "mrpw", "mtrpo", "mtdsto", "b_nbin", "tout", "mout")
E_BADARG, E_UNSUPPORTED, E_GRAPH = -1, -2, -3


def _np(ei):
    ei = ei.numpy() if hasattr(ei, "numpy") else np.asarray(ei)
    return ei[0].astype(np.int64), ei[1].astype(np.int64)


def ref_plan(ei, n):
    """numpy restatement of the plan: PyG edge order, stable sorts."""
    src, dst = _np(ei)
    keep = src != dst
    gs = np.concatenate([src[keep], np.arange(n)])
    gd = np.concatenate([dst[keep], np.arange(n)])
    order = np.argsort(gd, kind="stable")
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(gd, minlength=n))])
    col = gs[order]
    pos = np.empty_like(order); pos[order] = np.arange(order.size)
    torder = np.argsort(gs, kind="stable")
    t_rowptr = np.concatenate([[0], np.cumsum(np.bincount(gs, minlength=n))])
    morder = np.argsort(dst, kind="stable")
    m_rowptr = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=n))])
    mtorder = np.argsort(src, kind="stable")
    return dict(rowptr=rowptr, col=col, t_rowptr=t_rowptr, t_eid=pos[torder], t_dst=gd[torder], m_rowptr=m_rowptr,
                m_col=src[morder], mt_rowptr=np.concatenate([[0], np.cumsum(np.bincount(src, minlength=n))]),
                mt_dst=dst[mtorder])


def segments_ref(ei, n, merge_upto=64):
    """(seg_ptr, most nodes, most GATConv edges, most SimpleConv edges of one segment).  The finest cuts: after node i iff
    no edge joins a node <= i with a node > i.  Then, left to right, a piece joins the running segment unless the two
    together would hold more than ``merge_upto`` nodes (a piece alone may: it is never cut)."""
    src, dst = _np(ei)
    crossing = np.zeros(n + 1, dtype=np.int64)               # crossing[i] = edges that join a node < i with a node >= i
    a, b = np.minimum(src, dst), np.maximum(src, dst)
    np.add.at(crossing, a + 1, 1)
    np.add.at(crossing, b + 1, -1)
    crossing = np.cumsum(crossing)
    ends = [i for i in range(1, n + 1) if crossing[i] == 0]
    seg, start, cur = [0], 0, 0
    for end in ends:
        if cur > start and end - start > merge_upto:
            seg.append(cur)
            start = cur
        cur = end
    seg.append(cur)
    seg = np.array(seg, dtype=np.int64)
    indeg_all = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=n))])
    indeg_gat = np.concatenate([[0], np.cumsum(np.bincount(dst[src != dst], minlength=n) + 1)])
    return (seg, int(np.diff(seg).max()), int(np.diff(indeg_gat[seg]).max()), int(np.diff(indeg_all[seg]).max()))


def part_rows(n, p, M):
    """Own rows [lo, hi) of part p of M of a segment of n rows: its 16-row tiles dealt out evenly."""
    tiles = (n + 15) // 16
    return 16 * (tiles * p // M), min(n, 16 * (tiles * (p + 1) // M))


def windows_ref(ei, n, seg):
    """The 28 figures of gatres_graph_windows_host: for M = 2 .. 8 the largest window (own rows of a part plus every row an
    edge joins them to, as one contiguous range) in rows, GATConv in-edges and SimpleConv in-edges of its rows, then for
    M = 2 .. 8 the most edges (self loops apart, duplicates counted) between one part and the other parts of its segment,
    into it or out of it."""
    src, dst = _np(ei)
    seg = np.asarray(seg, dtype=np.int64)
    ns = len(seg) - 1
    indeg_gat = np.concatenate([[0], np.cumsum(np.bincount(dst[src != dst], minlength=n) + 1)])
    indeg_all = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=n))])
    seg_of = np.searchsorted(seg[1:], np.arange(n), side="right")
    nl = src != dst
    u, v = src[nl], dst[nl]
    su = seg_of[u]
    assert np.array_equal(su, seg_of[v]), "an edge leaves its segment"
    out, halo = [], []
    for M in range(2, 9):
        part_of = np.empty(n, dtype=np.int64)
        wlo, whi = np.empty((ns, M), dtype=np.int64), np.empty((ns, M), dtype=np.int64)
        for s in range(ns):
            a, cnt = int(seg[s]), int(seg[s + 1] - seg[s])
            for p in range(M):
                lo, hi = part_rows(cnt, p, M)
                part_of[a + lo:a + hi] = p
                wlo[s, p], whi[s, p] = a + lo, a + hi
        pu, pv = part_of[u], part_of[v]
        x = pu != pv
        hin, hout = np.zeros((ns, M), dtype=np.int64), np.zeros((ns, M), dtype=np.int64)
        np.add.at(hout, (su[x], pu[x]), 1)
        np.add.at(hin, (su[x], pv[x]), 1)
        np.minimum.at(wlo, (su[x], pu[x]), v[x]); np.maximum.at(whi, (su[x], pu[x]), v[x] + 1)
        np.minimum.at(wlo, (su[x], pv[x]), u[x]); np.maximum.at(whi, (su[x], pv[x]), u[x] + 1)
        out += [int((whi - wlo).max()), int((indeg_gat[whi] - indeg_gat[wlo]).max()),
                int((indeg_all[whi] - indeg_all[wlo]).max())]
        halo.append(int(max(hin.max(), hout.max())))
    return out + halo


def _even(v):
    return (v + 1) & ~1


def _rows_of(ptr, idx, a, b):
    """list of the rows a .. b-1 of a CSR, as arrays"""
    return [idx[ptr[r]:ptr[r + 1]] for r in range(a, b)]


def part_record_ref(ei, n, seg_ptr, s, p, M, plan=None):
    """Every header field (by its name in PT_FIELDS) and every table of the record of part p of segment s, for M parts per
    segment; ``total_words`` is the record's length and ``padding`` the u16 padding it contains (zeros).  ``plan``: a
    ``ref_plan(ei, n)`` computed before (it depends on nothing else)."""
    P = plan if plan is not None else ref_plan(ei, n)
    n0, cnt = int(seg_ptr[s]), int(seg_ptr[s + 1] - seg_ptr[s])
    lo, hi = part_rows(cnt, p, M)
    ow = hi - lo
    e0, em0, t0, mt0 = (int(P[k][n0]) for k in ("rowptr", "m_rowptr", "t_rowptr", "mt_rowptr"))
    # the four adjacencies of the own rows, in segment-local row numbers
    ins = [c - n0 for c in _rows_of(P["rowptr"], P["col"], n0 + lo, n0 + hi)]            # GATConv sources
    outs = [c - n0 for c in _rows_of(P["t_rowptr"], P["t_dst"], n0 + lo, n0 + hi)]       # GATConv destinations
    oute = [c - e0 for c in _rows_of(P["t_rowptr"], P["t_eid"], n0 + lo, n0 + hi)]       # ... and their saved-edge ids
    mins = [c - n0 for c in _rows_of(P["m_rowptr"], P["m_col"], n0 + lo, n0 + hi)]       # SimpleConv sources
    mouts = [c - n0 for c in _rows_of(P["mt_rowptr"], P["mt_dst"], n0 + lo, n0 + hi)]    # SimpleConv destinations
    cat = lambda rows: np.concatenate(rows).astype(np.int64) if rows else np.zeros(0, dtype=np.int64)
    colo, tdsto, teido, mcolo, mtdsto = cat(ins), cat(outs), cat(oute), cat(mins), cat(mouts)
    near = np.concatenate([colo, tdsto, mcolo, mtdsto])
    wlo = min(lo, int(near.min())) if near.size else lo
    whi = max(hi, int(near.max()) + 1) if near.size else hi
    wr = whi - wlo
    f = dict(MAGIC=PT_MAGIC, M=M, N0=n0, N=cnt, E0=e0, EM0=em0, T0=t0, MT0=mt0, LO=lo, HI=hi, WLO=wlo, WHI=whi)
    f["ELO"], f["OEG"] = int(P["rowptr"][n0 + lo]) - e0, colo.size
    f["EWLO"], f["WEG"] = int(P["rowptr"][n0 + wlo]) - e0, int(P["rowptr"][n0 + whi] - P["rowptr"][n0 + wlo])
    f["MELO"], f["OEM"] = int(P["m_rowptr"][n0 + lo]) - em0, mcolo.size
    f["TLO"], f["OTG"] = int(P["t_rowptr"][n0 + lo]) - t0, tdsto.size
    f["MTLO"], f["OTM"] = int(P["mt_rowptr"][n0 + lo]) - mt0, mtdsto.size
    ptr_of = lambda rows: np.concatenate([[0], np.cumsum([len(r) for r in rows], dtype=np.int64)]).astype(np.int64)
    rpo, trpo, mrpo, mtrpo = ptr_of(ins), ptr_of(outs), ptr_of(mins), ptr_of(mouts)
    mrpw = (P["m_rowptr"][n0 + wlo:n0 + whi + 1] - P["m_rowptr"][n0 + wlo]).astype(np.int64)
    mean_indeg = np.diff(P["m_rowptr"])[n0:n0 + cnt]      # SimpleConv in-degree of the segment's rows
    # ---- edge descriptors, one row of 8 (in) or 16 (out) half-words per own row
    nbin, mbin = np.zeros((ow, 8), dtype=np.int64), np.zeros((ow, 8), dtype=np.int64)
    tout, mout = np.zeros((ow, 16), dtype=np.int64), np.zeros((ow, 16), dtype=np.int64)
    for r in range(ow):
        own = lo + r
        a = ins[r]                                         # (never empty: GATConv's self loop)
        nbin[r, 0], nbin[r, 1] = rpo[r], len(a)
        nbin[r, 2:8] = [a[min(k, len(a) - 1)] for k in range(MAXD)]
        a = mins[r]
        mbin[r, 0], mbin[r, 1] = mrpo[r], len(a)
        mbin[r, 2:8] = [a[k] if k < len(a) else own for k in range(MAXD)]
        a, x = outs[r], oute[r]
        tout[r, 0] = len(a)
        tout[r, 2:8] = [a[min(k, len(a) - 1)] for k in range(MAXD)]
        tout[r, 8:14] = [x[min(k, len(a) - 1)] for k in range(MAXD)]
        a = mouts[r]
        named = [a[k] if k < len(a) else own for k in range(MAXD)]
        mout[r, 0] = len(a)
        mout[r, 2:8] = named
        mout[r, 8:14] = [max(int(mean_indeg[j]), 1) for j in named]
    # ---- hand-off lists
    remote = lambda j: (j < lo) | (j >= hi)
    lists = dict(
        f_hlist=np.unique(colo[remote(colo)]),                                                  # rows to import, forward
        f_elist=np.array([lo + r for r in range(ow) if remote(outs[r]).any()], dtype=np.int64),  # rows to export, forward
        b_hrow=np.unique(tdsto[remote(tdsto)]),
        b_hedge=np.unique(teido[remote(tdsto)]),
        b_erow=np.array([lo + r for r in range(ow) if remote(ins[r]).any()], dtype=np.int64),
        b_eedge=f["ELO"] + np.nonzero(remote(colo))[0])
    # ---- layout (u16 half-words; every table padded to whole words, 16 bytes before the descriptors)
    half, pad = 0, 0
    def place(tables):
        nonlocal half, pad
        start = half
        for i, (length, before16) in enumerate(tables):
            if before16:
                extra = -(half - start) % 8
                half += extra; pad += extra
            half += _even(length); pad += _even(length) - length
        return (half - start) // 2
    f["F_IMG"] = PT_HEADER
    f["F_IMG_WORDS"] = place([(ow + 1, 0), (colo.size, 0), (ow + 1, 0), (mcolo.size, 0), (8 * ow, 1), (8 * ow, 0)])
    f["B_IMG"] = PT_HEADER + half // 2
    f["B_IMG_WORDS"] = place([(ow + 1, 0), (colo.size, 0), (ow + 1, 0), (tdsto.size, 0), (tdsto.size, 0), (wr + 1, 0),
                              (ow + 1, 0), (mtdsto.size, 0), (8 * ow, 1), (16 * ow, 0), (16 * ow, 0)])
    for name, off, cntf in zip(LISTS, ("F_HLIST", "F_ELIST", "B_HROW", "B_HEDGE", "B_EROW", "B_EEDGE"),
                               ("F_HCNT", "F_ECNT", "B_HRCNT", "B_HECNT", "B_ERCNT", "B_EECNT")):
        f[off], f[cntf] = PT_HEADER + half // 2, int(lists[name].size)
        place([(int(lists[name].size), 0)])
    rec = dict(f)
    rec.update(rpo=rpo, colo=colo, mrpo=mrpo, mcolo=mcolo, nbin=nbin, mbin=mbin, b_rpo=rpo, b_colo=colo, trpo=trpo,
               teido=teido, tdsto=tdsto, mrpw=mrpw, mtrpo=mtrpo, mtdsto=mtdsto, b_nbin=nbin, tout=tout, mout=mout, **lists)
    rec["reserved"] = np.zeros(PT_HEADER - len(PT_FIELDS), dtype=np.int64)
    rec["padding"] = np.zeros(pad, dtype=np.int64)
    rec["total_words"] = PT_HEADER + half // 2
    return rec


def stride_ref(totals):
    """The record stride: the largest record, rounded up to 4 words (16 bytes)."""
    return (max(totals) + 3) & ~3


def decode_header(words, stride, s, p, M):
    rec = np.asarray(words)[(s * M + p) * stride:(s * M + p + 1) * stride]
    return {k: int(rec[i]) for i, k in enumerate(PT_FIELDS)}


def decode_record(words, stride, s, p, M):
    """The record of (s, p) in the library's words, taken apart by its OWN header into the dict of part_record_ref.  The
    images are walked table by table from their offsets; ``total_words`` is where the last list ends."""
    rec = np.ascontiguousarray(np.asarray(words)[(s * M + p) * stride:(s * M + p + 1) * stride]).astype(np.int32)
    h = rec.view(np.uint16).astype(np.int64)
    f = {k: int(rec[i]) for i, k in enumerate(PT_FIELDS)}
    ow, wr = f["HI"] - f["LO"], f["WHI"] - f["WLO"]
    out = dict(f)
    out["reserved"] = rec[len(PT_FIELDS):PT_HEADER].astype(np.int64)
    pads = []

    def walk(start_word, spec):
        at = start = 2 * start_word
        for name, length, shape, before16 in spec:
            if before16:
                extra = -(at - start) % 8
                pads.append(h[at:at + extra]); at += extra
            v = h[at:at + length]
            out[name] = v.reshape(shape) if shape else v
            pads.append(h[at + length:at + _even(length)])
            at += _even(length)
        return (at - start) // 2

    fw = walk(f["F_IMG"], [("rpo", ow + 1, None, 0), ("colo", f["OEG"], None, 0), ("mrpo", ow + 1, None, 0),
                           ("mcolo", f["OEM"], None, 0), ("nbin", 8 * ow, (ow, 8), 1), ("mbin", 8 * ow, (ow, 8), 0)])
    bw = walk(f["B_IMG"], [("b_rpo", ow + 1, None, 0), ("b_colo", f["OEG"], None, 0), ("trpo", ow + 1, None, 0),
                           ("teido", f["OTG"], None, 0), ("tdsto", f["OTG"], None, 0), ("mrpw", wr + 1, None, 0),
                           ("mtrpo", ow + 1, None, 0), ("mtdsto", f["OTM"], None, 0), ("b_nbin", 8 * ow, (ow, 8), 1),
                           ("tout", 16 * ow, (ow, 16), 0), ("mout", 16 * ow, (ow, 16), 0)])
    out["walked_image_words"] = (fw, bw)
    end = f["B_IMG"] + bw
    for name, off, cntf in zip(LISTS, ("F_HLIST", "F_ELIST", "B_HROW", "B_HEDGE", "B_EROW", "B_EEDGE"),
                               ("F_HCNT", "F_ECNT", "B_HRCNT", "B_HECNT", "B_ERCNT", "B_EECNT")):
        walk(f[off], [(name, f[cntf], None, 0)])
        end = f[off] + _even(f[cntf]) // 2
    out["padding"] = np.concatenate(pads) if pads else np.zeros(0, dtype=np.int64)
    out["total_words"] = end
    out["tail"] = rec[end:].astype(np.int64)
    return out


def record_mismatches(got, want):
    """Names of the fields / tables of a decoded record that differ from the restatement (empty = word-for-word equal)."""
    bad = []
    for k, v in want.items():
        g = got.get(k)
        if isinstance(v, np.ndarray):
            if g is None or g.shape != v.shape or not np.array_equal(g, v):
                bad.append(k)
        elif g != v:
            bad.append(k)
    if got["walked_image_words"] != (got["F_IMG_WORDS"], got["B_IMG_WORDS"]):
        bad.append("image word counts")
    if got["tail"].any():
        bad.append("words beyond the last list")
    return bad
