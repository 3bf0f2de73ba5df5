"""The per-plan work buffers of ``GATResMeanConv`` (scratch, the inference launch's throw-away ``saved``) on plans that agree
in every total and differ in their largest segment (tests/work_buffer_cases.py) -- no GPU: the plans and the module live on
the host, the sizes come from the library's own ``gatres_scratch_floats`` / ``gatres_saved_floats`` / ``gatres_fused_plan``.

  * the cases are decisive: equal totals, different sizes of both buffers, different parts where the case says so;
  * the restated layout (``work_buffer_cases.layout_offsets``) is the library's, on every plan and on known figures;
  * on ONE module, in either order of a pair: every buffer is at least as large as the library asks for its plan, plans whose
    sizes or parts differ never share storage, the same plan -- or an equal topology built again -- gets its buffer back
    (the barrier state inside is what the LRU is for), the LRU keeps its bound, a cached buffer that is too small is refused;
  * the call state of a forward and the evaluation runner's plan draw the same scratch.

Integers and identities only."""
import ctypes as C

import pytest
import torch

import fused_plan_refs as FR
import work_buffer_cases as WC

NB, NC = WC.NB, WC.NC
LRU_BOUND = 6


@pytest.fixture(scope="module")
def plans():
    out = {name: (WC.host_plan(a), WC.host_plan(b)) for name, (a, b, _) in WC.PAIRS.items()}
    out["control"] = (WC.host_plan(WC.CONTROL), WC.host_plan(WC.CONTROL))
    return out


def _model(pkg):
    return pkg.GATResMeanConv(num_blocks=NB, nc=NC)


def _storage(t):
    return t.untyped_storage().data_ptr()


def test_the_pairs_are_decisive(pkg, lib, plans):
    for name in WC.PAIRS:
        a, b = plans[name]
        assert WC.totals(a) == WC.totals(b) and a.num_segments == 2, name
        assert WC.largest(a) != WC.largest(b), name
        (sa, va), (sb, vb) = WC.need_floats(lib, a), WC.need_floats(lib, b)
        assert min(sa, va, sb, vb) > 0 and sa != sb and va != vb, (name, sa, sb, va, vb)
    a, b = plans["same_split"]
    assert WC.parts_at(lib, a) == WC.parts_at(lib, b) == 8
    assert WC.need_floats(lib, a) < WC.need_floats(lib, b)          # (A first: every launch of B past the end of A's buffers)
    a, b = plans["different_split"]
    assert (WC.parts_at(lib, a), WC.parts_at(lib, b)) == (7, 8)
    a, b = plans["across_fused_limit"]
    assert WC.parts_at(lib, a) > 0 and WC.parts_at(lib, b) == 0 and b.max_segment_nodes > FR.MAX_FUSED_NODES
    a, b = plans["control"]
    assert a is not b and WC.totals(a) == WC.totals(b) and WC.largest(a) == WC.largest(b)
    assert WC.need_floats(lib, a) == WC.need_floats(lib, b) and tuple(a.windows) == tuple(b.windows)
    # the alternating GPU cases: at most 428 nodes per batch, window kernel on both sides
    m = WC.model_struct()
    for name, (ca, cb, gpu) in WC.PAIRS.items():
        if gpu:
            assert sum(ca[0]) <= 428 and sum(cb[0]) <= 428
            for p in plans[name]:
                out = (C.c_int32 * len(FR.WORDS))()
                assert lib.gatres_fused_plan(C.byref(m), p.ref(), FR.TRAIN, 256, out) == 0 and out[1] == 1, name


def test_the_restated_layout_is_the_librarys(pkg, lib, plans):
    """``layout_offsets`` against gatres_scratch_floats (its last word) and gatres_fused_status_offset (the flag region) on
    every plan of the cases, and against figures worked out by hand for one."""
    m = WC.model_struct()
    every = [p for pair in plans.values() for p in pair] + [WC.host_plan(WC.MIXED_SYM)]
    for p in every:
        o = WC.offsets_of(p)
        assert o.scratch_total == WC.need_floats(lib, p)[0], WC.totals(p)
        st = int(lib.gatres_fused_status_offset(C.byref(m), p.ref()))
        if p.max_segment_nodes <= FR.MAX_FUSED_NODES:
            assert st == o.status and WC.flags_offset_from_status(st, p.num_segments) == o.sc_flags
            assert o.sc_flags + o.flag_words <= o.sc_xch <= o.sc_xch + p.num_segments * o.xch_stride <= o.scratch_total
        else:
            assert st == -1 and o.xch_stride == 0 and o.split_max == 1
    # known figures: 2 x 388 nodes, 430 pipes each -> N 776, Eg 2 * 860 + 776 = 2496, largest segment 388 rows / 1248 edges.
    #   P = 64 + 2 * (288 + 4096) + 33 = 8865 parameters: slab stride 8868; (776 + 63) / 64 = 13 slabs; loss_part r4(16 + 1) = 20;
    #   col_words r4(2 * 2 + 8) = 12; 8 nc + 3 = 259 granules per row and 3 per edge in front of the heartbeats
    o = WC.layout_offsets(2, 32, 776, 2496, 2, 388, 1248)
    nc_rows = 776 * 32
    s_stride = 2 * nc_rows + 2 * (2 * nc_rows) + 2 * 1552 + 4992 + 2 * 776 + 2496
    front = nc_rows + s_stride + 5 * nc_rows + 4992 + 2 * 1552 + 2 * (2 * nc_rows) + 2 * 2 * 2048 + 2496 + 2 * 776 + nc_rows
    keep = 2 * nc_rows + nc_rows + 2 * 1552 + 2 * 776
    assert o.sc_flags == front + 13 * 8868 + 20 + 2 * keep
    assert o.flag_words == 8 * 8 * 32 + 32 and o.status == o.sc_flags + 8 * 8 * 32 and o.split_max == 8
    assert o.hb == 388 * 259 + 3 * 1248 and o.xch_stride == 2 * ((o.hb + 48 + 15) // 16 * 16)
    assert o.sc_xch == o.sc_flags + o.flag_words + 12 + 2 * 8 * 8868
    assert WC.offsets_of(WC.host_plan(WC.MIXED_SYM)) == o


def _orders():
    for name in list(WC.PAIRS) + ["control"]:
        for order in ((0, 1), (1, 0)):
            yield pytest.param(name, order, id=f"{name}-{'AB' if order == (0, 1) else 'BA'}")


@pytest.mark.parametrize("name,order", list(_orders()))
def test_buffers_are_large_enough_and_shared_only_by_equal_plans(pkg, lib, plans, name, order):
    model = _model(pkg)
    pair = [plans[name][k] for k in order]
    got = []
    for visit in range(2):                              # A, B, A, B
        for p in pair:
            scratch, saved = model._scratch_for(p), model._eval_saved_for(p)
            need_scratch, need_saved = WC.need_floats(lib, p)
            assert scratch.numel() >= need_scratch, (name, order, visit, scratch.numel(), need_scratch)
            assert saved.numel() >= need_saved, (name, order, visit, saved.numel(), need_saved)
            assert scratch.dtype == saved.dtype == torch.float32 and _storage(scratch) != _storage(saved)
            got.append((_storage(scratch), _storage(saved)))
    assert got[0] == got[2] and got[1] == got[3]          # the same plan asked again: the same storage, state and all
    if name == "control":
        assert got[0] == got[1]                           # an equal topology, another GraphPlan object: still that storage
    else:
        assert got[0][0] != got[1][0] and got[0][1] != got[1][1]
    assert len(model._scratch) <= LRU_BOUND


def test_the_key_holds_the_largest_segment_the_sizes_and_the_parts(pkg, lib, plans, monkeypatch):
    from gnn_pressure_estimation_amd import graph_models as GM
    m = WC.model_struct()
    keys = {}
    for name, (a, b) in plans.items():
        ka, kb = GM.work_buffer_key(C.byref(m), a, 256), GM.work_buffer_key(C.byref(m), b, 256)
        keys[name] = ka, kb
        for k, p in ((ka, a), (kb, b)):
            assert k[:5] == WC.totals(p) + WC.largest(p)
            assert (k[GM.KEY_SCRATCH_FLOATS], k[GM.KEY_SAVED_FLOATS]) == WC.need_floats(lib, p)
            assert k[GM.KEY_PARTS] == WC.parts_at(lib, p)
        assert (ka == kb) == (name == "control"), name
        hash(ka)
    assert [k[GM.KEY_PARTS] for k in keys["different_split"]] == [7, 8]
    # one plan, another split (GATRES_FUSED_SPLIT): sizes and figures equal, the parts alone tell the keys apart
    a = plans["same_split"][1]
    monkeypatch.setenv("GATRES_FUSED_SPLIT", "2")
    k2 = GM.work_buffer_key(C.byref(m), a, 256)
    k8 = keys["same_split"][1]
    assert k2 != k8 and k2[:GM.KEY_PARTS] == k8[:GM.KEY_PARTS] and k2[GM.KEY_PARTS + 1:] == k8[GM.KEY_PARTS + 1:]
    assert (k2[GM.KEY_PARTS], k8[GM.KEY_PARTS]) == (2, 8)
    # a narrower model on the same plan: other sizes
    assert GM.work_buffer_key(C.byref(WC.model_struct(nc=16)), a, 256)[GM.KEY_SCRATCH_FLOATS] != k8[GM.KEY_SCRATCH_FLOATS]


def test_the_lru_keeps_its_bound_and_the_recent_buffers(pkg, lib, plans):
    model = _model(pkg)
    first = plans["control"][0]
    s0 = _storage(model._scratch_for(first))
    seen = 0
    for name in WC.PAIRS:
        for p in plans[name]:
            model._scratch_for(p)
            model._eval_saved_for(p)
            seen += 2
            assert len(model._scratch) <= LRU_BOUND
            assert _storage(model._scratch_for(first)) == s0          # (asked in between: most recently used, never evicted)
    assert seen > LRU_BOUND and len(model._scratch) == LRU_BOUND


def test_a_cached_buffer_that_is_too_small_is_refused(pkg, lib, plans):
    model = _model(pkg)
    p = plans["same_split"][1]
    good = model._scratch_for(p)
    (key,) = [k for k in model._scratch if k[0] != "eval_saved"]
    model._scratch[key] = torch.zeros(good.numel() - 1)
    with pytest.raises(RuntimeError, match="scratch"):
        model._scratch_for(p)
    model = _model(pkg)
    good = model._eval_saved_for(p)
    (key,) = list(model._scratch)
    assert key[0] == "eval_saved"
    model._scratch[key] = torch.empty(good.numel() - 1)
    with pytest.raises(RuntimeError, match="saved"):
        model._eval_saved_for(p)


def test_forward_call_state_and_evaluation_plan_draw_the_same_scratch(pkg, lib, plans):
    """Whoever asks for a plan's scratch gets the LRU's: the forward's call state, the evaluation runner's ``_EvalPlan.refresh``
    on another GraphPlan object of the topology (its constructor takes the plan from the model's device plan cache, so the
    object is made without it here), a direct ask -- on both plans of a pair.  (A GATResTrainer needs the device:
    tests/test_gpu_work_buffers.py holds it and a whole ``_EvalPlan`` to the same buffer.)"""
    from gnn_pressure_estimation_amd import evaluation as EV
    model = _model(pkg)
    for case, p in zip(WC.PAIRS["same_split"][:2], plans["same_split"]):
        st = model._call_state(p)
        P = object.__new__(EV._EvalPlan)
        P.plan = WC.host_plan(case)
        P.refresh(model)
        assert P.plan is not p and WC.totals(P.plan) == WC.totals(p)
        assert _storage(P.state["scratch"]) == _storage(st["scratch"]) == _storage(model._scratch_for(p))
        assert P.state["scratch"].numel() >= WC.need_floats(lib, p)[0]
        assert P.saved is None or P.saved.numel() >= WC.need_floats(lib, p)[1]
    a, b = plans["same_split"]
    assert _storage(model._call_state(a)["scratch"]) != _storage(model._call_state(b)["scratch"])
