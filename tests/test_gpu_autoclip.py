"""AutoClip gradient-norm clipping (reference utils/gradient_clipping.py; train.py:186-187 with --use_gradient_clipping True
--percentile p) in the native training step: the update kernel against numpy / torch.optim.Adam through
``gatres_autoclip_adam_step``, and ``GATResTrainer(use_gradient_clipping=True)`` through every way a step is enqueued --
fused + hipGraph against the oracle, per-op fp32 and bf16, fit_epoch with a ragged tail, a dropped step, world size 2.

The clipping rule is restated here from its definition: n = ||g||_2, history += [n], c = np.percentile(history, p),
g *= min(1, c / (n + 1e-6)) (always), then Adam."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from test_gpu_model import build, relerr

pytestmark = pytest.mark.gpu
NB, NC, BS, NODES, PIPES = 15, 32, 32, 388, 430
LR, WD = 5e-4, 6e-6


def _clip_rule(history, n, percentile):
    c = float(np.percentile(np.asarray(history, dtype=np.float64), percentile))
    return c, min(1.0, c / (n + 1e-6))


class _ClipOracle:
    """The oracle's training step (oracle.OracleTrainer: torch.optim.Adam, MSELoss) with the clipping rule in front of Adam."""

    def __init__(self, oracle, params, percentile, bf16=False):
        self.t = oracle.OracleTrainer(params, lr=LR, weight_decay=WD, bf16=bf16)
        self.percentile = percentile
        self.history, self.clips = [], []

    def step(self, x, y, edge_index, mask):
        t = self.t
        t.opt.zero_grad()
        m = torch.as_tensor(mask, dtype=torch.bool)
        xin = x.clone()
        xin[m] = 0
        out = t.forward(t.params, xin, edge_index)
        loss = torch.nn.functional.mse_loss(out[m], y[m])
        loss.backward()
        n = math.sqrt(sum(float(v.grad.double().pow(2).sum()) for v in t.params.values()))
        self.history.append(n)
        c, coef = _clip_rule(self.history, n, self.percentile)
        self.clips.append(c)
        for v in t.params.values():
            v.grad.mul_(coef)
        t.opt.step()
        return loss.detach(), out.detach()


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


# ---------------------------------------------------------------------------------------------------------------- kernel
def _grad_sequence(P, steps, seed):
    """Flat fp32 gradients of mixed scales, exact repeats (ties in the history) and norms around 1e-5 (coefficient ~0.91)."""
    g = torch.Generator().manual_seed(seed)
    out, prev = [], None
    for i in range(steps):
        if prev is not None and i % 7 == 3:
            v = prev.clone()                                             # the same vector again: an exact tie
        elif i % 11 == 5:
            v = torch.randn(P, generator=g)
            v = v * (1e-5 / float(v.double().norm()))                    # ||g|| ~ 1e-5
        else:
            v = torch.randn(P, generator=g) * float(10.0 ** (torch.rand(1, generator=g) * 6 - 4))
        out.append(v.float())
        prev = out[-1]
    return out


def _api_run(pkg, P, grads, percentile, capacity, graph=False, seed=0):
    from gnn_pressure_estimation_amd import _native, train_step as TS
    lib = _native.load()
    dev = torch.device("cuda", 0)
    st = TS._AutoClipState(percentile, P, dev, capacity)
    params = (torch.randn(P, generator=torch.Generator().manual_seed(seed)) * 0.1).to(dev)
    p0 = params.clone()
    m, v = torch.zeros(P, device=dev), torch.zeros(P, device=dev)
    sc = torch.zeros(2, dtype=torch.int64, device=dev)
    gbuf = torch.zeros(P, device=dev)
    k = len(grads)
    rec = torch.zeros(k, 3, dtype=torch.float64, device=dev)
    gens = set()

    def one():
        _native.check(lib.gatres_autoclip_adam_step(params.data_ptr(), gbuf.data_ptr(), m.data_ptr(), v.data_ptr(),
                                                    sc.data_ptr(), P, LR, 0.9, 0.999, 1e-8, WD, 1.0, C.byref(st.c),
                                                    _native.current_stream(dev)), "gatres_autoclip_adam_step")
    g = None
    if graph:
        st.reserve(k)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            one()
    for i, gi in enumerate(grads):
        gbuf.copy_(gi.to(dev))
        if graph:
            g.replay()
        else:
            st.reserve(1)                   # (grows the buffers before the count gets to their capacity)
            gens.add(st.generation)
            one()
        rec[i].copy_(st.out)
    torch.cuda.synchronize()
    cnt = int(st.ctl[0])
    return dict(p0=p0.cpu(), params=params.cpu(), m=m.cpu(), v=v.cpu(), step=int(sc[0]), rec=rec.cpu().numpy(),
                log=st.log[:cnt].cpu().numpy(), sorted=(st.sorted1 if cnt & 1 else st.sorted0)[:cnt].cpu().numpy(),
                growths=len(gens) - 1, overflow=int(st.ctl[4]))


@pytest.mark.parametrize("percentile", [0.0, 10.0, 37.5, 50.0, 100.0])
def test_autoclip_kernel_vs_numpy_and_torch_adam(pkg, percentile):
    P, steps = 3001, 600
    grads = _grad_sequence(P, steps, seed=int(percentile * 8) + 1)
    r = _api_run(pkg, P, grads, percentile, capacity=128, seed=3)
    assert r["growths"] >= 2 and r["overflow"] == 0 and r["step"] == steps
    norms = np.array([math.sqrt(float(gi.double().pow(2).sum())) for gi in grads])
    assert len(r["log"]) == steps and _rel(r["log"], norms) < 1e-12
    assert np.array_equal(r["sorted"], np.sort(r["log"]))                    # bitwise
    rec = r["rec"]
    clip_ref = np.array([np.percentile(r["log"][:i + 1], percentile) for i in range(steps)])
    coef_ref = np.minimum(1.0, clip_ref / (r["log"] + 1e-6))
    assert np.array_equal(rec[:, 0], r["log"])
    assert _rel(rec[:, 1], clip_ref) < 1e-12 and _rel(rec[:, 2], coef_ref) < 1e-12
    # c == n (the first step; n is the percentile itself): the coefficient is n / (n + 1e-6), never a shortcut to 1
    same = [i for i in range(steps) if rec[i, 1] == rec[i, 0]]
    assert 0 in same and all(rec[i, 2] < 1.0 for i in same)
    tiny = [i for i in same if i % 11 == 5 and i % 7 != 3]
    for i in tiny:                                                           # the 1e-6 term: ~0.91 for ||g|| ~ 1e-5
        assert abs(rec[i, 2] - 1e-5 / (1e-5 + 1e-6)) < 1e-3
    if percentile == 0.0:
        assert tiny
    # torch.optim.Adam on the clipped gradient (the kernel's coefficient, rounded to fp32 as the kernel multiplies)
    p = r["p0"].clone().cuda().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=LR, weight_decay=WD)
    for i, gi in enumerate(grads):
        p.grad = gi.cuda() * torch.tensor(rec[i, 2], dtype=torch.float32).cuda()
        opt.step()
    s = opt.state[p]
    assert relerr(r["params"], p.detach()) < 1e-6
    assert relerr(r["m"], s["exp_avg"]) < 1e-6 and relerr(r["v"], s["exp_avg_sq"]) < 1e-6


def test_autoclip_kernel_graph_replay_equals_eager(pkg):
    P, steps = 3001, 300
    grads = _grad_sequence(P, steps, seed=77)
    eager = _api_run(pkg, P, grads, 10.0, capacity=steps, seed=5)
    graph = _api_run(pkg, P, grads, 10.0, capacity=steps, graph=True, seed=5)
    for k in ("params", "m", "v"):
        assert torch.equal(eager[k], graph[k]), k
    for k in ("log", "sorted", "rec"):
        assert np.array_equal(eager[k], graph[k]), k
    assert eager["step"] == graph["step"] == steps


# ------------------------------------------------------------------------------------------------------------- trainer
def _trainer(pkg, oracle, nb=NB, nc=NC, bs=BS, seed=3, **kw):
    model, p = build(pkg, oracle, nb, nc, seed=seed, fused=kw.get("fused", True))
    ei = pkg.wdn_synth.collate_edge_index(pkg.wdn_synth.make_wdn_topology(NODES, PIPES, seed=0), NODES, bs)
    tr = pkg.GATResTrainer(model, ei.cuda(), NODES * bs, nodes_per_graph=[NODES] * bs, **kw)
    return model, p, tr, ei


def test_percentile_is_validated_and_clipping_off_has_no_history(pkg, oracle):
    with pytest.raises(ValueError):
        _trainer(pkg, oracle, nb=2, nc=32, bs=2, use_gradient_clipping=True, percentile=100.5)
    _, _, tr, _ = _trainer(pkg, oracle, nb=2, nc=32, bs=2)
    with pytest.raises(RuntimeError):
        tr.grad_norm_history()


def _vs_oracle(pkg, oracle, tr, p, ei, bs, steps, bf16=False, tol=1e-5, seed=6):
    ref = _ClipOracle(oracle, p, 10.0, bf16=bf16)
    snaps = pkg.wdn_synth.make_snapshots(steps * bs, NODES, seed=seed)
    rng = np.random.RandomState(1)
    coefs, clips = [], []
    for it in range(steps):
        y = pkg.wdn_synth.collate_snapshots(snaps, range(it * bs, (it + 1) * bs))
        mask = torch.from_numpy(pkg.wdn_synth.generate_batch_mask([NODES] * bs, 0.95, rng))
        l_ref, o_ref = ref.step(y.clone(), y, ei, mask)
        loss = tr.step(y.cuda(), y.cuda(), mask.cuda())
        assert relerr(tr.out, o_ref) < tol and relerr(loss, l_ref) < tol, it
        coefs.append(float(tr.last_clip_coef))
        clips.append(float(tr.last_clip_value))
        assert tr.last_grad_norm.dim() == 0 and tr.last_grad_norm.is_cuda
    hist = tr.grad_norm_history()
    assert hist.dtype == np.float64 and len(hist) == steps and tr.optimizer_step == steps
    assert _rel(hist, ref.history) < tol and _rel(clips, ref.clips) < tol
    return coefs


def test_headline_config_with_autoclip_vs_oracle(pkg, oracle, lib):
    model, p, tr, ei = _trainer(pkg, oracle, use_graph=True, use_gradient_clipping=True, percentile=10)
    assert tr.fused and tr.use_graph
    assert lib.gatres_fused_cus_per_segment(model._cmodel_ref(), tr.plan.ref()) == 8
    coefs = _vs_oracle(pkg, oracle, tr, p, ei, BS, 6)
    assert coefs[0] < 1.0 and sum(c < 1.0 for c in coefs) >= 3
    assert sum(c < 0.999 for c in coefs) >= 2                  # clipped for real, not only by the 1e-6 term
    assert tr.num_captured_graphs >= 1


def _shadow_check(tr, p0_flat, record):
    """Any path: every history entry is the fp64 norm of that step's (unclipped) gradient, the clip value its percentile,
    and the parameters are torch.optim.Adam's on the clipped gradients."""
    hist = tr.grad_norm_history()
    norms = np.array([math.sqrt(float(g.double().pow(2).sum())) for g, _ in record])
    assert _rel(hist, norms) < 1e-12
    p = p0_flat.clone().cuda().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=LR, weight_decay=WD)
    for i, (g, rec) in enumerate(record):
        c, coef = _clip_rule(hist[:i + 1], hist[i], tr.percentile)
        assert _rel([rec[1], rec[2]], [c, coef]) < 1e-12
        p.grad = g.cuda() * torch.tensor(rec[2], dtype=torch.float32).cuda()
        opt.step()
    assert relerr(tr.model.flat_parameters, p.detach()) < 1e-6


@pytest.mark.parametrize("use_graph", [False, True])
def test_per_op_path_with_autoclip_vs_oracle(pkg, oracle, use_graph):
    model, p, tr, ei = _trainer(pkg, oracle, nb=3, nc=32, bs=2, fused=False, use_graph=use_graph,
                                use_gradient_clipping=True, percentile=10)
    assert not tr.fused
    p0 = model.flat_parameters.detach().clone().cpu()
    _vs_oracle(pkg, oracle, tr, p, ei, 2, 6)
    # and the same trainer again from its initial state, against its own gradients (restated rule + torch Adam)
    model2, _, tr2, _ = _trainer(pkg, oracle, nb=3, nc=32, bs=2, fused=False, use_graph=use_graph,
                                 use_gradient_clipping=True, percentile=10)
    snaps = pkg.wdn_synth.make_snapshots(12, NODES, seed=6).cuda()
    record = []
    for it in range(6):
        y = snaps[2 * it:2 * it + 2].reshape(-1)
        tr2.step(y, y)
        record.append((tr2.grads.clone().cpu(), tr2._clip.out.cpu().numpy()))
    _shadow_check(tr2, p0, record)


def test_gatres_large_bf16_small_batch_with_autoclip(pkg, oracle):
    model, p = build(pkg, oracle, 2, 128, seed=4, fused=False)
    model.set_compute_dtype("bf16")
    bs = 2
    ei = pkg.wdn_synth.collate_edge_index(pkg.wdn_synth.make_wdn_topology(NODES, PIPES, seed=0), NODES, bs)
    tr = pkg.GATResTrainer(model, ei.cuda(), NODES * bs, nodes_per_graph=[NODES] * bs, use_graph=True,
                           use_gradient_clipping=True, percentile=10)
    assert not tr.fused
    p0 = model.flat_parameters.detach().clone().cpu()
    snaps = pkg.wdn_synth.make_snapshots(12, NODES, seed=9).cuda()
    record = []
    for it in range(6):
        y = snaps[2 * it:2 * it + 2].reshape(-1)
        assert torch.isfinite(tr.step(y, y)).all()
        record.append((tr.grads.clone().cpu(), tr._clip.out.cpu().numpy()))
    _shadow_check(tr, p0, record)
    # the first step against the bf16-rounding oracle: the same norm to bf16 accuracy
    model2, _ = build(pkg, oracle, 2, 128, seed=4, fused=False)
    model2.set_compute_dtype("bf16")
    tr2 = pkg.GATResTrainer(model2, ei.cuda(), NODES * bs, nodes_per_graph=[NODES] * bs, use_graph=False,
                            use_gradient_clipping=True, percentile=10)
    y = pkg.wdn_synth.collate_snapshots(pkg.wdn_synth.make_snapshots(bs, NODES, seed=2), range(bs))
    mask = torch.from_numpy(pkg.wdn_synth.generate_batch_mask([NODES] * bs, 0.95, np.random.RandomState(3)))
    ref = _ClipOracle(oracle, p, 10.0, bf16=True)
    ref.step(y.clone(), y, ei, mask)
    tr2.step(y.cuda(), y.cuda(), mask.cuda())
    assert _rel(tr2.grad_norm_history(), ref.history) < 2e-2


@pytest.mark.parametrize("use_graph", [False, True])
def test_fit_epoch_ragged_tail_with_autoclip_equals_single_steps(pkg, oracle, use_graph):
    one = pkg.wdn_synth.make_wdn_topology()
    raw = pkg.wdn_synth.make_snapshots(11, 388, seed=3) * 6 + 35
    st = pkg.SnapshotStore(raw, one, device="cuda")
    nb, nc, bs = 3, 32, 4
    model, _ = build(pkg, oracle, nb, nc, seed=8)
    tr = pkg.GATResTrainer(model, st.edge_index(bs), 388 * bs, nodes_per_graph=[388] * bs, seed=5, targets_are_inputs=True,
                           use_graph=use_graph, use_gradient_clipping=True, percentile=10)
    losses = [tr.fit_epoch(st, bs, shuffle=True, generator=torch.Generator().manual_seed(7 + ep))[0] for ep in range(2)]
    tr.set_lr(2e-4)                                     # (read from the device buffer by the captured steps)
    losses.append(tr.fit_epoch(st, bs, shuffle=True, generator=torch.Generator().manual_seed(9))[0])
    assert tr.optimizer_step == 9 and len(tr.grad_norm_history()) == 9          # one entry per step, main + sibling
    assert len(tr._siblings) == 1 and next(iter(tr._siblings.values()))._clip is tr._clip
    twin, _ = build(pkg, oracle, nb, nc, seed=8)
    t4 = pkg.GATResTrainer(twin, st.edge_index(bs), 388 * bs, nodes_per_graph=[388] * bs, seed=5, targets_are_inputs=True,
                           use_graph=False, use_gradient_clipping=True, percentile=10)
    t3 = pkg.GATResTrainer(twin, st.edge_index(3), 388 * 3, nodes_per_graph=[388] * 3, seed=5, targets_are_inputs=True,
                           use_graph=False, _share_state_with=t4)
    for ep, seed in enumerate((7, 8, 9)):
        if ep == 2:
            t4.set_lr(2e-4)
        tot, n = 0.0, 0
        for xb, eib, ng in st.batches(bs, shuffle=True, generator=torch.Generator().manual_seed(seed)):
            t = t4 if ng == bs else t3
            t.invalidate_weights()
            tot += float(t.step(xb, xb)) * ng
            n += ng
        assert abs(losses[ep] - tot / n) < 1e-6 * abs(tot / n), ep
    assert torch.equal(model.flat_parameters, twin.flat_parameters)
    assert np.array_equal(tr.grad_norm_history(), t4.grad_norm_history())
    tr.reset_gradient_clipping()
    assert len(tr.grad_norm_history()) == 0


def test_dropped_step_adds_no_history_entry(pkg, oracle):
    from gnn_pressure_estimation_amd import train_step as TS
    model, p, tr, ei = _trainer(pkg, oracle, bs=2, use_graph=False, force_collective_path=True,
                                use_gradient_clipping=True, percentile=10)
    y = pkg.wdn_synth.make_snapshots(2, NODES, seed=2).reshape(-1).cuda()
    tr.step(y, y)
    assert tr.dropped_steps == 0 and tr.optimizer_step == 1 and len(tr.grad_norm_history()) == 1
    before = model.flat_parameters.clone()
    state = tr._clip.out.clone()
    tr.grads[0] = float("nan")
    tr._enqueue(TS.PHASE_ADAM, True)
    torch.cuda.synchronize()
    assert tr.dropped_steps == 1 and tr.optimizer_step == 1 and len(tr.grad_norm_history()) == 1
    assert torch.equal(model.flat_parameters, before) and torch.equal(tr._clip.out, state)
    tr.step(y, y)
    assert tr.dropped_steps == 1 and tr.optimizer_step == 2 and len(tr.grad_norm_history()) == 2
    assert torch.isfinite(tr.loss).all() and float(tr.last_grad_norm) == tr.grad_norm_history()[-1]


# ---------------------------------------------------------------------------------------------------------- two ranks
def _rank_main_clip(rank, world, port, out_dir, case):
    import os
    import sys
    from test_gpu_two_ranks import CASES, NODES as N, ROOT, STEPS, _build, _data
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import gnn_pressure_estimation_amd as G
        from oracle import gatres_oracle as O
        c = CASES[case]
        torch.cuda.set_device(0)
        one, snaps, masks, B = _data(G, case, world)
        rows = G.dp.shard_graphs(B, rank, world)
        per = len(rows)
        ei = G.wdn_synth.collate_edge_index(one, N, per).cuda()
        model = _build(G, O, c, seed=1 + 10 * rank)
        tr = G.GATResTrainer(model, ei, N * per, nodes_per_graph=[N] * per, seed=5, use_graph=False, fused=c["fused"],
                             blocks_per_bucket=1, use_gradient_clipping=True, percentile=10)
        assert tr.split
        for s in range(STEPS):
            x = G.wdn_synth.collate_snapshots(snaps[s], rows).cuda()
            tr.step(x, x, masks[s][rows[0] * N:(rows[-1] + 1) * N].cuda())
        torch.cuda.synchronize()
        torch.save({"params": model.flat_parameters.clone().cpu(), "hist": tr.grad_norm_history(),
                    "steps": tr.optimizer_step}, os.path.join(out_dir, f"c{rank}.pt"))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def _single_main_clip(out_dir, case, world=2):
    import os
    import sys
    from test_gpu_two_ranks import CASES, NODES as N, ROOT, STEPS, _build, _data
    sys.path.insert(0, ROOT)
    import gnn_pressure_estimation_amd as G
    from oracle import gatres_oracle as O
    c = CASES[case]
    one, snaps, masks, B = _data(G, case, world)
    ei = G.wdn_synth.collate_edge_index(one, N, B).cuda()
    model = _build(G, O, c, seed=1)
    tr = G.GATResTrainer(model, ei, N * B, nodes_per_graph=[N] * B, seed=5, use_graph=False, fused=c["fused"],
                         use_gradient_clipping=True, percentile=10)
    for s in range(STEPS):
        x = G.wdn_synth.collate_snapshots(snaps[s], range(B)).cuda()
        tr.step(x, x, masks[s].cuda())
    torch.save({"params": model.flat_parameters.clone().cpu(), "hist": tr.grad_norm_history()},
               os.path.join(out_dir, "csingle.pt"))


@pytest.mark.parametrize("case", ["fused", "per_op"])
def test_autoclip_at_world_size_two_on_one_gpu(case, tmp_path, fork_ctx):
    from test_gpu_two_ranks import STEPS, _free_port, _run_all
    port = _free_port()
    _run_all([fork_ctx.Process(target=_single_main_clip, args=(str(tmp_path), case))])
    _run_all([fork_ctx.Process(target=_rank_main_clip, args=(r, 2, port, str(tmp_path), case)) for r in range(2)])
    r0, r1 = (torch.load(tmp_path / f"c{r}.pt", weights_only=False) for r in range(2))
    one = torch.load(tmp_path / "csingle.pt", weights_only=False)
    assert r0["steps"] == r1["steps"] == STEPS and len(r0["hist"]) == STEPS
    assert np.array_equal(r0["hist"], r1["hist"]) and torch.equal(r0["params"], r1["params"])
    assert _rel(r0["hist"], one["hist"]) < 1e-5
    assert float((r0["params"] - one["params"]).abs().max()) < 2e-5
