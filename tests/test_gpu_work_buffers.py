"""The per-plan work buffers and the hand-off state that persists inside them, on the device (tests/work_buffer_cases.py).

  * ALTERNATING PLANS: two plans of equal totals and different largest segments take turns (A, B, A, B) on one module -- module
    forward + backward, the no-grad inference forward, a ``GATResTrainer.step`` of trainers that share the model, the evaluation
    runner's forward -- and every visit equals, bit for bit, the same call on a fresh module with the same parameters that
    has only ever seen that plan;
  * MIXED LAUNCH KINDS on one scratch buffer (window kernel at 8 parts: a symmetric plan, and a directed one whose hand-offs are
    paced by heartbeats): training step, inference forward, forward with ``saved`` and backward-only, forward + backward in one
    launch, forward without ``saved`` (whole-segment kernel), training steps replayed from a hipGraph, an eager step again.
    After every launch the flag lines are read back: word 0 (``group_sync`` epoch) equal over the parts of a segment, word 2
    (granule epoch) equal and advanced by 3 nb per forward / backward phase run; results equal a module whose barrier state
    is reset before every launch;
  * WRAP-AROUND: both epochs of every part start at 2^32 - k, with k chosen from the hand-offs a step was measured to pass, so
    that the counter wraps in the forward of the second of three training steps, or is exactly 0 at the first hand-off of that
    step; outputs, loss, gradients and parameters of all three steps equal a run on a fresh (zeroed) scratch buffer.

Everything is ``torch.equal``; no step may fault or be dropped."""
import numpy as np
import pytest
import torch

import irregular_graphs as IG
import work_buffer_cases as WC
from test_gpu_model import build, note

pytestmark = pytest.mark.gpu

NB, NC = WC.NB, WC.NC
SEED = 41


def _st():
    import gnn_pressure_estimation_amd as G
    return G._native.current_stream(torch.device("cuda"))


def _batch_inputs(pkg, npg, seed):
    """(y [N, 1], mask bool [N]) on the device."""
    N = int(sum(npg))
    y = torch.randn(N, 1, generator=torch.Generator().manual_seed(seed))
    mask = torch.from_numpy(pkg.wdn_synth.generate_batch_mask(npg, 0.95, np.random.RandomState(seed)))
    return y.cuda(), mask.cuda()


def _fresh_like(pkg, model):
    """A fresh module with ``model``'s parameters as they are now."""
    m = pkg.GATResMeanConv(num_blocks=model.num_blocks, nc=model.nc).cuda()
    with torch.no_grad():
        m.flat_parameters.copy_(model.flat_parameters)
    torch.cuda.synchronize()
    return m


def _status_words(pkg, lib, model, plan):
    """(fault, fault count, dropped steps) of the plan's scratch on ``model``."""
    off = int(lib.gatres_fused_status_offset(model._cmodel_ref(), plan.ref()))
    assert off >= 0
    torch.cuda.synchronize()
    w = model._scratch_for(plan)[off:off + 4].view(torch.int32).cpu()
    return int(w[0]), int(w[1]), int(w[3])


class _Store:
    """What evaluation._EvalPlan reads of a store, for one ragged batch."""

    def __init__(self, ei, npg):
        self._ei, self._npg, self.device = ei, npg, ei.device

    def num_nodes(self, recipe):
        return sum(self._npg)

    def edge_index(self, recipe):
        return self._ei

    def nodes_per_graph(self, recipe):
        return self._npg


class _Side:
    """One plan on one module: the batch, and the objects a kind of call needs, made on first use."""

    def __init__(self, pkg, lib, model, ei, npg, seed):
        self.pkg, self.lib, self.model, self.ei, self.npg = pkg, lib, model, ei.cuda(), npg
        self.N = int(sum(npg))
        self.y, self.mask = _batch_inputs(pkg, npg, seed)
        self.x = self.y.clone()
        self.x[self.mask] = 0
        self.trainer = self.eval_plan = None

    def plan(self):
        return self.model.plan_for(self.ei, self.N)

    def get_trainer(self):
        if self.trainer is None:
            self.trainer = self.pkg.GATResTrainer(self.model, self.ei, self.N, nodes_per_graph=self.npg, use_graph=False)
            assert self.trainer.fused
        return self.trainer

    def run(self, kind):
        """The results of one call of ``kind`` (clones)."""
        model = self.model
        if kind == "module":
            model.zero_grad()
            out = model(self.x, self.ei)
            torch.nn.functional.mse_loss(out[self.mask], self.y[self.mask]).backward()
            return [out.detach().clone(), model.flat_grad().clone()]
        if kind == "inference":
            with torch.no_grad():
                return [model(self.x, self.ei).clone()]
        if kind == "trainer":
            tr = self.get_trainer()
            loss = tr.step(self.y, self.y, self.mask)
            return [tr.out.clone(), loss.clone(), tr.grads.clone(), model.flat_parameters.clone()]
        assert kind == "eval"
        from gnn_pressure_estimation_amd import evaluation as EV
        if self.eval_plan is None:
            self.eval_plan = EV._EvalPlan(model, _Store(self.ei, self.npg), len(self.npg), recipe=(len(self.npg),))
        P = self.eval_plan.refresh(model)
        assert P.state["window"] and P.saved is not None
        P.x.copy_(self.y.reshape(-1))
        P.mask.copy_(self.mask.to(torch.uint8))
        EV._enqueue_forward(self.lib, model.flat_parameters, P, _st())
        return [P.out.clone()]


@pytest.mark.parametrize("kind", ["module", "inference", "trainer", "eval"])
@pytest.mark.parametrize("pair", [n for n, c in WC.PAIRS.items() if c[2]])
def test_alternating_plans_of_equal_totals_equal_fresh_modules(pkg, lib, oracle, pair, kind):
    """A, B, A, B on one module.  The buffers are the plans' own (large enough, distinct, the same on every visit, shared with
    the trainer and the evaluation plan), and every visit's results are those of a fresh module that has the same parameters
    (and, for the trainer, the same Adam state) and has seen only that plan."""
    case_a, case_b, _ = WC.PAIRS[pair]
    model, _ = build(pkg, oracle, NB, NC, seed=SEED)
    sides = [_Side(pkg, lib, model, *WC.batch(*c), seed=SEED + k) for k, c in enumerate((case_a, case_b))]
    seen = {}
    for visit in range(4):
        s = sides[visit % 2]
        ref_model = _fresh_like(pkg, model)
        ref = _Side(pkg, lib, ref_model, s.ei, s.npg, seed=SEED + visit % 2)
        assert torch.equal(ref.y, s.y) and torch.equal(ref.mask, s.mask)
        if kind == "trainer":
            tr, rt = s.get_trainer(), ref.get_trainer()
            for dst, src in ((rt.exp_avg, tr.exp_avg), (rt.exp_avg_sq, tr.exp_avg_sq), (rt.step_counter, tr.step_counter)):
                dst.copy_(src)
        got, want = s.run(kind), ref.run(kind)
        torch.cuda.synchronize()
        for i, (g, w) in enumerate(zip(got, want)):
            assert torch.isfinite(g).all() and torch.equal(g, w), (pair, kind, visit, i, float((g - w).abs().max()))
        plan = s.plan()
        scratch = model._scratch_for(plan)
        need_scratch, need_saved = WC.need_floats(lib, plan)
        assert scratch.numel() >= need_scratch and model._eval_saved_for(plan).numel() >= need_saved
        assert seen.setdefault(visit % 2, scratch.data_ptr()) == scratch.data_ptr()          # the plan's own, every visit
        assert _status_words(pkg, lib, model, plan) == (0, 0, 0), (pair, kind, visit)
        if kind == "trainer":
            assert s.trainer.scratch.data_ptr() == scratch.data_ptr()
            assert s.trainer.fault_count == 0 and s.trainer.dropped_steps == 0
        if kind == "eval":
            assert s.eval_plan.state["scratch"].data_ptr() == scratch.data_ptr()
            assert s.eval_plan.saved.data_ptr() == model._eval_saved_for(plan).data_ptr()
    assert seen[0] != seen[1]
    pa, pb = sides[0].plan(), sides[1].plan()
    assert WC.totals(pa) == WC.totals(pb) and WC.largest(pa) != WC.largest(pb)
    parts = [int(lib.gatres_fused_cus_per_segment(model._cmodel_ref(), p.ref())) for p in (pa, pb)]
    assert parts == ([7, 8] if pair == "different_split" else [8, 8]), parts


def test_trainer_and_evaluation_plan_share_the_modules_scratch(pkg, lib, oracle):
    model, _ = build(pkg, oracle, NB, NC, seed=SEED)
    s = _Side(pkg, lib, model, *WC.batch(*WC.CONTROL), seed=SEED)
    s.run("eval")
    tr = s.get_trainer()
    assert tr.plan is not s.eval_plan.plan
    assert tr.scratch.data_ptr() == s.eval_plan.state["scratch"].data_ptr() == model._scratch_for(tr.plan).data_ptr()
    assert tr.scratch.numel() == WC.need_floats(lib, tr.plan)[0] == WC.offsets_of(tr.plan).scratch_total


# ------------------------------------------------------------------------------------------ mixed launch kinds
def _mixed_plan(pkg, which):
    if which == "symmetric":
        return WC.batch(*WC.MIXED_SYM)
    g = IG.named("snap_dir_hub")
    return IG.collate(g, 2), [g.num_nodes] * 2


def _forward_without_saved(pkg, lib, model, plan, x):
    """The forward launch with no ``saved`` buffer: the whole-segment kernel at the plan's parts."""
    st = model._call_state(plan)
    out = torch.empty((plan.num_nodes, 1), dtype=torch.float32, device=x.device)
    pkg._native.check(lib.gatres_model_forward(st["mref"], st["gref"], model.flat_parameters.data_ptr(), x.data_ptr(), None,
                                               out.data_ptr(), None, st["scratch"].data_ptr(), _st()), "gatres_model_forward")
    return out


def _mixed_sequence(pkg, lib, side, graph_trainer):
    """[(name, call -> results, forward / backward phase runs of the window kernel it may make)]."""
    tr = side.get_trainer()
    model = side.model

    def step(t):
        def run():
            loss = t.step(side.y, side.y, side.mask)
            return [t.out.clone(), loss.clone(), t.grads.clone(), model.flat_parameters.clone()]
        return run

    def fwd_bwd():
        loss = tr.forward_backward(side.y, side.y, side.mask)
        return [tr.out.clone(), loss.clone(), tr.grads.clone()]

    def whole():
        return [_forward_without_saved(pkg, lib, model, side.plan(), side.x).clone()]

    # a captured step is warmed up once outside the capture (and rolled back) the first time its graph key is seen: 2 or 4
    return [("step", step(tr), (2,)), ("inference", lambda: side.run("inference"), (1,)),
            ("forward_saved+backward", lambda: side.run("module"), (2,)), ("forward_backward", fwd_bwd, (2,)),
            ("forward_without_saved", whole, (0,)),
            ("graph_step_1", step(graph_trainer), (2, 4)), ("graph_step_2", step(graph_trainer), (2, 4)),
            ("graph_step_3", step(graph_trainer), (2,)), ("step_again", step(tr), (2,))]


@pytest.mark.parametrize("which", ["symmetric", "directed"])
def test_mixed_launch_kinds_keep_the_parts_epochs_together(pkg, lib, oracle, which):
    ei, npg = _mixed_plan(pkg, which)
    models = [build(pkg, oracle, NB, NC, seed=SEED + 3)[0] for _ in range(2)]
    sides = [_Side(pkg, lib, m, ei, npg, seed=SEED + 5) for m in models]
    graph_trainers = [pkg.GATResTrainer(s.model, s.ei, s.N, nodes_per_graph=npg, use_graph=True) for s in sides]
    seqs = [_mixed_sequence(pkg, lib, s, g) for s, g in zip(sides, graph_trainers)]
    side, model = sides[0], models[0]
    tr = side.get_trainer()
    plan, S = tr.plan, tr.plan.num_segments
    assert bool(plan.flags & IG.SYMMETRIC) == (which == "symmetric")
    M = int(lib.gatres_fused_cus_per_segment(model._cmodel_ref(), plan.ref()))
    assert M == 8 and lib.gatres_fused_window_kernel(model._cmodel_ref(), plan.ref()) == 1
    offs = WC.offsets_of(plan)
    st_off = int(lib.gatres_fused_status_offset(model._cmodel_ref(), plan.ref()))
    assert offs.status == st_off and WC.flags_offset_from_status(st_off, S) == offs.sc_flags
    assert offs.scratch_total == tr.scratch.numel()
    assert graph_trainers[0].scratch.data_ptr() == tr.scratch.data_ptr() == model._scratch_for(side.plan()).data_ptr()
    w0, w2 = WC.read_epochs(tr.scratch, offs.sc_flags, S)
    assert not w0.any() and not w2.any()
    ref_tr = sides[1].get_trainer()
    log = []
    for (name, call, runs), (_, ref_call, _) in zip(*seqs):
        got = call()
        n0, n2 = WC.read_epochs(tr.scratch, offs.sc_flags, S)
        pkg._native.check(lib.gatres_fused_reset_sync(models[1]._cmodel_ref(), ref_tr.plan.ref(), ref_tr.scratch.data_ptr(), _st()),
                          "gatres_fused_reset_sync")
        want = ref_call()
        torch.cuda.synchronize()
        d0, d2 = (n0 - w0)[:, :M], (n2 - w2)[:, :M]
        log.append((name, int(d0[0, 0]), int(d2[0, 0])))
        assert (n0[:, :M] == n0[:, :1]).all(), (name, n0)                    # word 0: the parts of a segment agree
        assert (n2[:, :M] == n2[:, :1]).all(), (name, n2)                    # word 2: and so do their granule epochs
        assert (d2 == d2[0, 0]).all() and int(d2[0, 0]) in [3 * NB * r for r in runs], (name, d2, runs)
        assert (d0 == d0[0, 0]).all() and int(d0[0, 0]) >= 0, (name, d0)
        if name == "forward_without_saved":
            assert int(d0[0, 0]) > 0, "the whole-segment kernel meets in group_sync"
        for i, (g, w) in enumerate(zip(got, want)):
            assert torch.isfinite(g).all() and torch.equal(g, w), (which, name, i)
        assert tr.fault_count == 0 and tr.dropped_steps == 0, name
        w0, w2 = n0, n2
    note(f"work buffers, mixed launch kinds ({which}): (launch, word 0 advance, word 2 advance)", log)
    assert ref_tr.fault_count == 0 and graph_trainers[0].fault_count == 0


# ------------------------------------------------------------------------------------------ wrap-around
WRAP_KINDS = {"symmetric": ("symmetric", None), "directed": ("directed", None), "whole_split2": ("symmetric", "2")}
_WRAP_REF = {}


def _three_steps(pkg, lib, oracle, which, preset=None):
    """Three training steps on a fresh module and trainer.  ``preset``: function(trainer, offsets) run before the first step.
    Returns (per-step results, per-step epochs read back [(word 0, word 2)], trainer, offsets, side)."""
    ei, npg = _mixed_plan(pkg, which)
    model, _ = build(pkg, oracle, NB, NC, seed=SEED + 7)
    side = _Side(pkg, lib, model, ei, npg, seed=SEED + 9)
    tr = side.get_trainer()
    offs = WC.offsets_of(tr.plan)
    assert offs.status == int(lib.gatres_fused_status_offset(model._cmodel_ref(), tr.plan.ref()))
    assert offs.scratch_total == tr.scratch.numel()
    if preset is not None:
        preset(tr, offs)
    S = tr.plan.num_segments
    epochs = [WC.read_epochs(tr.scratch, offs.sc_flags, S)]
    results = []
    for k in range(3):
        y, mask = _batch_inputs(pkg, npg, SEED + 20 + k)
        loss = tr.step(y, y, mask)
        results.append([tr.out.clone(), loss.clone(), tr.grads.clone(), model.flat_parameters.clone()])
        epochs.append(WC.read_epochs(tr.scratch, offs.sc_flags, S))
    assert tr.fault_count == 0 and tr.dropped_steps == 0
    return results, epochs, tr, offs, side


def _wrap_reference(pkg, lib, oracle, kind):
    """The fresh-scratch run of ``kind`` (once per kind) and the hand-offs it was measured to pass: (results, word that counts
    them, per training step, per forward, parts)."""
    if kind not in _WRAP_REF:
        which, _ = WRAP_KINDS[kind]
        results, epochs, tr, offs, side = _three_steps(pkg, lib, oracle, which)
        model = side.model
        M = int(lib.gatres_fused_cus_per_segment(model._cmodel_ref(), tr.plan.ref()))
        window = int(lib.gatres_fused_window_kernel(model._cmodel_ref(), tr.plan.ref()))
        word = 1 if window else 0                              # (index into read_epochs' pair: word 2 | word 0)
        assert not epochs[0][0].any() and not epochs[0][1].any()
        steps = [epochs[k + 1][word][:, :M] - epochs[k][word][:, :M] for k in range(3)]
        per_step = int(steps[0][0, 0])
        assert per_step > 0 and all((d == per_step).all() for d in steps), steps
        side.run("inference")
        after = WC.read_epochs(tr.scratch, offs.sc_flags, tr.plan.num_segments)
        fwd = after[word][:, :M] - epochs[3][word][:, :M]
        per_fwd = int(fwd[0, 0])
        assert 0 < per_fwd < per_step and (fwd == per_fwd).all(), fwd
        sync = [epochs[k + 1][0][:, :M] - epochs[k][0][:, :M] for k in range(3)]
        assert all((d == sync[0][0, 0]).all() for d in sync), sync
        _WRAP_REF[kind] = (results, word, per_step, per_fwd, M, window, int(sync[0][0, 0]))
    return _WRAP_REF[kind]


def _wrapped_run_equals_fresh(pkg, lib, oracle, kind, k, word, d, M, what, granule=None):
    """Three steps from words 0 and 2 = 2^32 - k (``granule``: another value for word 2) against the fresh-scratch run of
    ``kind``; ``word`` (read_epochs' index) must have advanced by ``d`` per step, through the wrap.  Returns the epochs read
    back after each step."""
    which, _ = WRAP_KINDS[kind]
    want = _wrap_reference(pkg, lib, oracle, kind)[0]
    start = (1 << 32) - k

    def preset(tr, offs):
        WC.set_epochs(tr.scratch, offs, tr.plan.num_segments, start, granule)
        w0, w2 = WC.read_epochs(tr.scratch, offs.sc_flags, tr.plan.num_segments)
        assert (w0 == start).all() and (w2 == (start if granule is None else granule)).all()

    got, epochs, tr, offs, side = _three_steps(pkg, lib, oracle, which, preset)
    note(f"work buffers, wrap ({kind}, {what}): hand-offs per step, k, the counting word after each step",
         [d, k, [int(e[word][0, 0]) for e in epochs]])
    for s in range(3):
        e = epochs[s + 1][word][:, :M]
        assert (e == (start + (s + 1) * d) % (1 << 32)).all(), (s, e)                 # wrapped after step 2: (s + 1) d - k
        assert (epochs[s + 1][0][:, :M] == epochs[s + 1][0][:, :1]).all() and (epochs[s + 1][1][:, :M] == epochs[s + 1][1][:, :1]).all()
        for i, (g, w) in enumerate(zip(got[s], want[s])):
            assert torch.isfinite(g).all() and torch.equal(g, w), (kind, what, s, i)
    assert int(epochs[1][word][0, 0]) > (1 << 31) and int(epochs[2][word][0, 0]) < d
    assert tr.fault_count == 0 and tr.dropped_steps == 0
    return epochs


@pytest.mark.parametrize("where", ["inside_second_forward", "zero_at_first_hand_off_of_second_step"])
@pytest.mark.parametrize("kind", list(WRAP_KINDS))
def test_epoch_counters_wrap_without_a_trace(pkg, lib, oracle, kind, where, monkeypatch):
    """Words 0 and 2 of every part = 2^32 - k (tests/work_buffer_cases.set_epochs: the state the kernels reach after that many
    hand-offs -- the heartbeat granules carry the same tag, the row / edge granules are still zeroed).  k from the MEASURED
    hand-offs d of one training step and f of one forward on the word the launch counts with (word 2: window kernel; word 0:
    whole-segment kernel): k = d + ceil(f / 2) wraps in the middle of the second step's forward, k = d + 1 makes the first
    hand-off of the second step carry epoch 0.  Granule tags are compared for equality and group_sync / the heartbeat by a signed
    difference, so nothing may change: three steps, bit for bit the fresh-scratch run."""
    _, split = WRAP_KINDS[kind]
    if split:
        monkeypatch.setenv("GATRES_FUSED_SPLIT", split)
    _, word, d, f, M, window, _ = _wrap_reference(pkg, lib, oracle, kind)
    assert (M, window) == ((2, 0) if split else (8, 1)), (M, window)
    assert window == 0 or (d, f) == (6 * NB, 3 * NB)
    k = d + (f + 1) // 2 if where == "inside_second_forward" else d + 1
    assert d < k <= d + f
    _wrapped_run_equals_fresh(pkg, lib, oracle, kind, k, word, d, M, where)


def test_window_kernels_group_sync_epoch_wraps_on_the_directed_plan(pkg, lib, oracle):
    """The window kernel on a directed plan also meets in ``group_sync`` (word 0) a measured number of times d0 per launch, far
    fewer than its granule hand-offs.  Word 0 = 2^32 - (d0 + 1): the first meeting of the second step carries epoch 0.  Word 2
    stays 0 as on a fresh buffer: from the same value it would reach 0 in the first forward, where an exchange table that was
    never written holds tag 0 -- a state no run arrives at."""
    _, word, d, f, M, window, d0 = _wrap_reference(pkg, lib, oracle, "directed")
    assert window == 1 and 0 < d0 < d
    epochs = _wrapped_run_equals_fresh(pkg, lib, oracle, "directed", d0 + 1, 0, d0, M, "group_sync", granule=0)
    assert [int(e[1][0, 0]) for e in epochs[1:]] == [s * d for s in (1, 2, 3)]
