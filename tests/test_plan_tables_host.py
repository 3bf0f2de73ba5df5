"""gatres_graph_part_tables_host held word for word to a numpy restatement (tests/plan_refs.py) on graphs chosen for the
builder's turnovers (tests/plan_cases.py), for every part count M = 2 .. 8; the invariants the window kernel relies on;
agreement with the LDS sizing figures of gatres_graph_windows_host; the segment table, the window figures and the
relabelling against their restatements; the 16-bit limits.  Host only: integers, equality, no tolerance."""
import ctypes as C

import numpy as np
import pytest
import torch

import plan_cases as PC
import plan_refs as PR

MS = PC.MS
PLAN_KEYS = ("rowptr", "col", "t_rowptr", "t_eid", "t_dst", "m_rowptr", "m_col", "mt_rowptr", "mt_dst")
CASE_NAMES = sorted(PC.cases())
GUARD, SENTINEL = 64, 0x5A5A5A5A


def lib_segments(lib, ei, n, merge_upto=64):
    ei = ei.contiguous()
    seg = torch.full((n + 1,), -7, dtype=torch.int32)
    ns, mx, mg, mm = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
    rc = lib.gatres_graph_segments_host(ei.data_ptr(), ei.shape[1], n, merge_upto, seg.data_ptr(), C.byref(ns), C.byref(mx),
                                        C.byref(mg), C.byref(mm))
    assert rc == 0
    return seg[:ns.value + 1].clone(), mx.value, mg.value, mm.value


def lib_windows(lib, ei, n, seg):
    ei = ei.contiguous()
    win = torch.full((28,), -7, dtype=torch.int32)
    rc = lib.gatres_graph_windows_host(ei.data_ptr(), ei.shape[1], n, seg.data_ptr(), seg.numel() - 1, win.data_ptr())
    return rc, win.tolist()


def lib_plan(lib, ei, n):
    """The library's own plan arrays (host tensors), the input of gatres_graph_part_tables_host."""
    ei = ei.contiguous()
    eg = C.c_int64(0)
    assert lib.gatres_graph_count_host(ei.data_ptr(), ei.shape[1], n, C.byref(eg)) == 0
    E = ei.shape[1]
    size = dict(rowptr=n + 1, col=eg.value, t_rowptr=n + 1, t_eid=eg.value, t_dst=eg.value, m_rowptr=n + 1, m_col=max(E, 1),
                mt_rowptr=n + 1, mt_dst=max(E, 1))
    host = {k: torch.zeros(size[k], dtype=torch.int32) for k in PLAN_KEYS}
    assert lib.gatres_graph_build_host(ei.data_ptr(), E, n, *[host[k].data_ptr() for k in PLAN_KEYS]) == 0
    return host


def lib_tables(lib, host, seg, M, stride=None):
    """(rc, words incl. guards, stride): the sizing call unless ``stride`` is given, then the filling call into a buffer
    of sentinels with GUARD sentinel words on either side."""
    ptrs = [host[k].data_ptr() for k in PLAN_KEYS]
    ns = seg.numel() - 1
    st = C.c_int64(-1)
    if stride is None:
        rc = lib.gatres_graph_part_tables_host(*ptrs, seg.data_ptr(), ns, M, None, 0, C.byref(st))
        if rc != 0:
            return rc, None, None
        stride = st.value
    buf = torch.full((2 * GUARD + ns * M * stride,), SENTINEL, dtype=torch.int32)
    st2 = C.c_int64(-1)
    rc = lib.gatres_graph_part_tables_host(*ptrs, seg.data_ptr(), ns, M, buf.data_ptr() + 4 * GUARD, stride, C.byref(st2))
    return rc, buf.numpy(), (stride, st2.value)


_DECODED = {}


def decoded(lib, name):
    """For one case: the library's segment table and plan, the restated plan, and for every M the decoded records of the
    library next to the restated ones.  Built once per case."""
    if name in _DECODED:
        return _DECODED[name]
    ei, n = PC.cases()[name]
    seg_t = lib_segments(lib, ei, n)[0]
    seg = PR.segments_ref(ei, n)[0]
    assert seg_t.tolist() == seg.tolist()
    host = lib_plan(lib, ei, n)
    plan = PR.ref_plan(ei, n)
    per_m = {}
    for M in MS:
        rc, buf, (stride, stride2) = lib_tables(lib, host, seg_t, M)
        assert rc == 0 and stride == stride2 and stride % 4 == 0
        assert (buf[:GUARD] == SENTINEL).all() and (buf[-GUARD:] == SENTINEL).all()
        words = buf[GUARD:-GUARD]
        recs = [(s, p, PR.decode_record(words, stride, s, p, M), PR.part_record_ref(ei, n, seg, s, p, M, plan=plan))
                for s in range(len(seg) - 1) for p in range(M)]
        per_m[M] = (stride, recs)
    _DECODED[name] = dict(ei=ei, n=n, seg=seg, seg_t=seg_t, host=host, plan=plan, per_m=per_m)
    return _DECODED[name]


def test_cases_reach_the_features_they_are_named_for():
    """numpy alone.  Every feature of plan_cases.FEATURES is reached by at least one case at every M = 2 .. 8 (each of
    them can occur at each M), and the purpose-built cases reach what their names say."""
    cases = PC.cases()
    reached = {M: {name: PC.features(ei, n, M) for name, (ei, n) in cases.items()} for M in MS}
    for M in MS:
        for feat in PC.FEATURES:
            assert any(feat in f for f in reached[M].values()), (M, feat)
    for M in MS:
        r = reached[M]
        assert "empty_part" in r["path_1"] and "empty_part" in r["path_15"] and "empty_part" in r["path_16"]
        assert "short_part" in r["path_17"] and "short_part" in r[f"path_{16 * M - 1}"]
        assert "one_tile_part" in r[f"path_{16 * M}"] and "empty_part" not in r[f"path_{16 * M}"]
        assert {"part_without_mean_out_edges", "part_without_mean_in_edges"} <= r["edgeless_40"]
        assert {"mean_out_row_zero_among_out_edges", "mean_in_row_zero", "directed", "remote_edge_one_direction",
                "padded_out_slot_names_row_without_in_edges"} <= r["directed_path_50"]
        assert {"part_without_mean_out_edges", "mean_out_row_gt6", "gat_out_row_gt6"} <= r["fan_out_130"]
        assert {"part_without_mean_in_edges", "mean_in_row_gt6", "gat_in_row_gt6"} <= r["fan_in_130"]
        assert {"self_loop", "mean_in_row_zero_next_to_self_loop", "duplicate_edge"} <= r["loop_next_to_empty_row_40"]
        assert {"duplicate_remote_edge", "remote_out_edges_not_in_saved_order", "remote_edge_both_directions",
                "remote_edge_one_direction"} <= r["crossing_duplicates_131"]
        assert {"several_segments", "ragged_segments"} <= r["ragged_17_130_389"]
        assert ("empty_part" in r["ragged_17_130_389"]) == (M > 2)          # (17 nodes: two tiles)
        for name in ("snap_dir_hub_x2", "dir_hub"):
            assert {"gat_in_row_gt6", "gat_out_row_gt6", "directed", "self_loop", "duplicate_edge"} <= r[name]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_plan_arrays_equal_restatement(lib, name):
    d = decoded(lib, name)
    for k, v in d["plan"].items():
        assert np.array_equal(d["host"][k].numpy()[:v.size], v), k


@pytest.mark.parametrize("name", CASE_NAMES)
def test_records_equal_restatement(lib, name):
    """Every record of every M, field by field and table by table; the padding inside it and the words beyond its last
    list are zero (the buffer held sentinels: the library writes every word of a record); the stride is the largest record
    rounded up to 16 bytes."""
    d = decoded(lib, name)
    for M in MS:
        stride, recs = d["per_m"][M]
        for s, p, got, want in recs:
            bad = PR.record_mismatches(got, want)
            assert not bad, (name, M, s, p, bad, {k: (got.get(k), want[k]) for k in bad[:2] if k in want})
        assert stride == PR.stride_ref([want["total_words"] for _, _, _, want in recs]), (name, M)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_record_invariants_the_kernel_relies_on(lib, name):
    """On the decoded library output alone: nested ranges, own rows that tile the segment, every descriptor index inside
    the LDS window, every saved-edge id inside the segment, list entries remote or own as defined, and on a symmetric
    graph the forward and backward lists the same."""
    d = decoded(lib, name)
    src, dst = d["ei"][0].numpy(), d["ei"][1].numpy()
    nl = src != dst
    fwd = set((src[nl] * d["n"] + dst[nl]).tolist())
    symmetric = fwd == set((dst[nl] * d["n"] + src[nl]).tolist())
    seg_gat = np.diff(d["plan"]["rowptr"][d["seg"]])
    for M in MS:
        _, recs = d["per_m"][M]
        at = {}
        for s, p, g, _ in recs:
            n, lo, hi, wlo, whi = g["N"], g["LO"], g["HI"], g["WLO"], g["WHI"]
            assert 0 <= wlo <= lo <= hi <= whi <= n, (M, s, p)
            assert lo == at.get(s, 0), (M, s, p)
            at[s] = hi
            if p == M - 1:
                assert hi == n
            assert g["WEG"] <= seg_gat[s] and g["EWLO"] + g["WEG"] <= seg_gat[s]
            inside = lambda v: ((v >= wlo) & (v < whi)).all()
            own = lambda v: ((v >= lo) & (v < hi)).all()
            for tab in ("nbin", "mbin", "b_nbin"):
                assert inside(g[tab][:, 2:8]), (M, s, p, tab)
            for tab in ("tout", "mout"):
                assert inside(g[tab][:, 2:8]), (M, s, p, tab)
                assert not g[tab][:, 1].any() and not g[tab][:, 14:16].any()
            assert (g["tout"][:, 8:14] < seg_gat[s]).all() and (g["mout"][:, 8:14] >= 1).all()
            for tab in ("colo", "mcolo", "tdsto", "mtdsto"):
                assert inside(g[tab]), (M, s, p, tab)
            assert (g["teido"] < seg_gat[s]).all()
            for lst in ("f_hlist", "b_hrow"):
                assert inside(g[lst]) and not ((g[lst] >= lo) & (g[lst] < hi)).any(), (M, s, p, lst)
                assert (np.diff(g[lst]) > 0).all()
            for lst in ("f_elist", "b_erow"):
                assert own(g[lst]) and (np.diff(g[lst]) > 0).all(), (M, s, p, lst)
            assert (g["b_hedge"] < seg_gat[s]).all() and (np.diff(g["b_hedge"]) > 0).all()
            assert ((g["b_eedge"] >= g["ELO"]) & (g["b_eedge"] < g["ELO"] + g["OEG"])).all() and (np.diff(g["b_eedge"]) > 0).all()
            if symmetric:
                assert np.array_equal(g["f_hlist"], g["b_hrow"]) and np.array_equal(g["f_elist"], g["b_erow"]), (M, s, p)
        assert all(at[s] == int(d["seg"][s + 1] - d["seg"][s]) for s in at)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_records_fill_what_the_window_figures_size(lib, name):
    """gatres_graph_windows_host sizes the window kernel's LDS (window[M - 2], halo[M - 2]); the records fill it.  The two
    must agree: the largest window of any record in rows, GATConv edges and SimpleConv edges IS the figure, and no list is
    longer than the halo figure."""
    d = decoded(lib, name)
    rc, win = lib_windows(lib, d["ei"], d["n"], d["seg_t"])
    assert rc == 0
    assert win == PR.windows_ref(d["ei"], d["n"], d["seg"])
    for M in MS:
        _, recs = d["per_m"][M]
        k = M - 2
        assert max(g["WHI"] - g["WLO"] for _, _, g, _ in recs) == win[3 * k]
        assert max(g["WEG"] for _, _, g, _ in recs) == win[3 * k + 1]
        assert max(int(g["mrpw"][-1]) for _, _, g, _ in recs) == win[3 * k + 2]
        for s, p, g, _ in recs:
            for lst in PR.LISTS:
                assert g[lst].size <= win[21 + k], (M, s, p, lst)


@pytest.mark.parametrize("name", ["ragged_17_130_389", "snap_dir_hub_x2", "path_17", "edgeless_40", "crossing_duplicates_131"])
def test_sizing_call_and_short_stride(lib, name):
    """out = NULL returns the stride of the filling call; a stride one word short is GATRES_E_BADARG, with nothing written at
    or past the first record that does not fit, nor outside the buffer."""
    d = decoded(lib, name)
    for M in MS:
        stride, recs = d["per_m"][M]
        rc, _, st = lib_tables(lib, d["host"], d["seg_t"], M)
        assert rc == 0 and st == (stride, stride)
        short = stride - 1
        while short > 0 and not any(want["total_words"] > short for *_, want in recs):
            short -= 1                                     # (the stride is rounded up: go below the largest record)
        rc, buf, (_, st_out) = lib_tables(lib, d["host"], d["seg_t"], M, stride=short)
        assert rc == PR.E_BADARG and st_out == -1
        first = next(i for i, (*_, want) in enumerate(recs) if want["total_words"] > short)
        assert (buf[:GUARD] == SENTINEL).all() and (buf[GUARD + first * short:] == SENTINEL).all(), (M, first)
        for i in range(first):                             # ... and the records before it are complete
            got = PR.decode_record(buf[GUARD:-GUARD], short, recs[i][0], recs[i][1], M)
            assert not PR.record_mismatches(got, recs[i][3])


@pytest.mark.parametrize("name", CASE_NAMES)
def test_segments_and_windows_equal_restatement(lib, name):
    ei, n = PC.cases()[name]
    for merge in (0, 1, 4, 40, 64):
        seg, mx, mg, mm = lib_segments(lib, ei, n, merge)
        want = PR.segments_ref(ei, n, merge)
        assert seg.tolist() == want[0].tolist() and (mx, mg, mm) == want[1:], (merge,)
        rc, win = lib_windows(lib, ei, n, seg)
        assert rc == 0 and win == PR.windows_ref(ei, n, want[0]), (merge,)


def test_window_is_the_union_over_all_four_csrs(lib):
    """In a plan of gatres_graph_build_host the SimpleConv neighbours of a row are among its GATConv neighbours, so two of the
    builder's four `widen` calls never move a window there.  The kernel, though, indexes its LDS window with SimpleConv's
    columns too (mbin, mout, mrpw): here the SimpleConv arrays come from a LARGER edge list than the GATConv arrays
    (extra directed chords), and the window must hold them -- part 0's upper end only through the transposed SimpleConv
    rows (row 2 names 90), a later part's lower end only through SimpleConv's in-rows (row 90 names 2, row 60 names 5)."""
    n = 100
    gat_ei = _sym_path(n)
    mean_ei = torch.cat([gat_ei, torch.tensor([[5, 70, 2], [60, 20, 90]])], dim=1)
    seg = torch.tensor([0, n], dtype=torch.int32)
    host, plan = lib_plan(lib, gat_ei, n), PR.ref_plan(gat_ei, n)
    mean_host, mean_plan = lib_plan(lib, mean_ei, n), PR.ref_plan(mean_ei, n)
    for k in ("m_rowptr", "m_col", "mt_rowptr", "mt_dst"):
        host[k], plan[k] = mean_host[k], mean_plan[k]
    for M in MS:
        rc, buf, (stride, _) = lib_tables(lib, host, seg, M)
        assert rc == 0
        for p in range(M):
            want = PR.part_record_ref(gat_ei, n, seg.numpy(), 0, p, M, plan=plan)
            got = PR.decode_record(buf[GUARD:-GUARD], stride, 0, p, M)
            assert not PR.record_mismatches(got, want), (M, p, PR.record_mismatches(got, want))
            if got["LO"] <= 2 < got["HI"]:
                assert got["WHI"] == 91
            if 16 <= got["LO"] <= 90 < got["HI"]:
                assert got["WLO"] == 2                     # (row 90's SimpleConv in-row names row 2)
            elif 16 <= got["LO"] <= 60 < got["HI"]:
                assert got["WLO"] == 5
            for tab in ("mbin", "mout"):
                assert ((got[tab][:, 2:8] >= got["WLO"]) & (got[tab][:, 2:8] < got["WHI"])).all()


def _sym_path(n):
    a = torch.arange(n - 1)
    return torch.stack([torch.cat([a, a + 1]), torch.cat([a + 1, a])]).contiguous()


def test_sixteen_bit_limits(lib):
    """A symmetric path of n nodes has 3 n - 2 GATConv edges: 21845 nodes is the largest one-segment path inside the 16-bit
    tables (65533 edges) and equals the restatement; one node more (65536 edges) and 65535 nodes are GATRES_E_UNSUPPORTED;
    M = 1 and M = 9 are GATRES_E_BADARG."""
    n = 21845
    ei = _sym_path(n)
    seg = lib_segments(lib, ei, n)[0]
    assert seg.tolist() == [0, n]
    host = lib_plan(lib, ei, n)
    plan = PR.ref_plan(ei, n)
    assert plan["rowptr"][-1] == 65533
    for M in (2, 8):
        rc, buf, (stride, _) = lib_tables(lib, host, seg, M)
        assert rc == 0
        totals = []
        for p in range(M):
            want = PR.part_record_ref(ei, n, seg.numpy(), 0, p, M, plan=plan)
            assert not PR.record_mismatches(PR.decode_record(buf[GUARD:-GUARD], stride, 0, p, M), want), (M, p)
            totals.append(want["total_words"])
        assert stride == PR.stride_ref(totals)
    for M in (1, 9, 0, -1):
        assert lib_tables(lib, host, seg, M)[0] == PR.E_BADARG
    for big in (n + 1, 65535):
        ei = _sym_path(big)
        seg = lib_segments(lib, ei, big)[0]
        assert seg.tolist() == [0, big]
        assert lib_tables(lib, lib_plan(lib, ei, big), seg, 4)[0] == PR.E_UNSUPPORTED


def test_part_tables_refuse_a_plan_that_is_not_one(lib):
    """What the builder can check without the arrays' lengths: a segment table or row pointers that decrease
    (GATRES_E_BADARG), a neighbour or a saved-edge id outside its segment (GATRES_E_GRAPH) -- before anything is written."""
    d = decoded(lib, "ragged_17_130_389")
    seg = d["seg_t"]

    def rc_with(key, index, value, seg_t=seg):
        host = {k: v.clone() for k, v in d["host"].items()}
        if key is not None:
            host[key][index] = value
        rc, buf, _ = lib_tables(lib, host, seg_t, 4, stride=d["per_m"][4][0])
        assert (buf == SENTINEL).all()
        return rc

    assert rc_with(None, 0, 0, seg_t=torch.tensor([0, 147, 17, 536], dtype=torch.int32)) == PR.E_BADARG
    assert rc_with(None, 0, 0, seg_t=torch.tensor([-1, 17, 147, 536], dtype=torch.int32)) == PR.E_BADARG
    for key in ("rowptr", "t_rowptr", "m_rowptr", "mt_rowptr"):
        assert rc_with(key, 20, int(d["host"][key][22]) + 1) == PR.E_BADARG, key
    for key in ("col", "t_dst", "m_col", "mt_dst"):
        assert rc_with(key, 3, 17) == PR.E_GRAPH, key            # (entry 3 belongs to the segment [0, 17))
        assert rc_with(key, int(d["host"][key.replace("col", "rowptr").replace("dst", "rowptr")][17]), 16) == PR.E_GRAPH, key
        assert rc_with(key, 3, -1) == PR.E_GRAPH, key
    assert rc_with("t_eid", 3, int(d["host"]["rowptr"][17])) == PR.E_GRAPH


@pytest.mark.parametrize("name", CASE_NAMES)
def test_reorder_is_a_deterministic_permutation_of_every_segment(lib, pkg, name):
    """gatres_graph_reorder_host: a permutation of each segment's own ids, the same on every call, and the plan GraphPlan
    builds with it is exactly ref_plan of the relabelled edge list (every row keeps PyG's edge order)."""
    ei, n = PC.cases()[name]
    ei = ei.contiguous()
    seg = lib_segments(lib, ei, n)[0]
    perms = []
    for _ in range(2):
        perm = torch.full((n,), -1, dtype=torch.int32)
        assert lib.gatres_graph_reorder_host(ei.data_ptr(), ei.shape[1], n, seg.data_ptr(), seg.numel() - 1, perm.data_ptr()) == 0
        perms.append(perm)
    assert torch.equal(perms[0], perms[1])
    perm = perms[0].long()
    for a, b in zip(seg[:-1].tolist(), seg[1:].tolist()):
        assert sorted(perm[a:b].tolist()) == list(range(a, b))
    old2new = torch.empty(n, dtype=torch.int64)
    old2new[perm] = torch.arange(n)
    want = PR.ref_plan(old2new[ei], n)
    host = lib_plan(lib, old2new[ei], n)
    for k, v in want.items():
        assert np.array_equal(host[k].numpy()[:v.size], v), k
    if ei.shape[1] == 0 or max(b - a for a, b in zip(seg[:-1].tolist(), seg[1:].tolist())) <= 32:
        return                                             # (GraphPlan takes no relabelling for such plans)
    plan = pkg.GraphPlan(ei, n, device="cpu", reorder=True)
    assert torch.equal(plan.perm_host, perms[0])
    for k, v in want.items():
        assert np.array_equal(plan.arrays[k].numpy()[:v.size], v), k
