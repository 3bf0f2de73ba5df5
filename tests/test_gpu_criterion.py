"""The reference's training criteria (train.py --criterion {mse,mae,sce}) in the native step: ``gatres_masked_loss`` on
constructed vectors, one step of every path ``gatres_train_step`` takes against the fp64 oracle (``oracle.gatres_forward``
in float64, seeded with the criterion's gradient and taken through torch autograd; Adam as ``oracle.train_step`` does it),
the window kernel's instantiations bit for bit, SCE's two branches, MSE unchanged, ``fit_epoch``, the data-parallel step and
AutoClip with MAE.

Semantics (include/gatres.h, GATRES_LOSS_*), over the M masked nodes with d = out - y:
  mse  sum d^2 / M,  g_out 2 d / M;   mae  sum |d| / M,  g_out sign(d) / M;
  sce  o^ = out / max(|out|, eps), y^ = y / max(|y|, eps), t = 1 - o^ y^ (eps 1e-12): sum t^3 / M,
       g_out -3 t^2 y^ / (eps M) where |out| < eps, else 0 (exactly: torch's fp32 autograd leaves rounding noise there)."""
import math
import os

import numpy as np
import pytest
import torch

from test_gpu_model import build, note, relerr

pytestmark = pytest.mark.gpu
NB, NC, NODES, PIPES = 15, 32, 388, 430
EPS = float(np.float32(1e-12))           # the fp32 eps the kernels (and torch's fp32 clamp_min) compare against
LR, WD, B1, B2, AEPS = 5e-4, 6e-6, 0.9, 0.999, 1e-8


def table(crit, out, y, mask):
    """(loss, g_out) of the criterion in fp64 (cpu tensors)."""
    o, t = out.detach().double().cpu().reshape(-1), y.detach().double().cpu().reshape(-1)
    m = torch.as_tensor(mask).bool().cpu().reshape(-1)
    M = int(m.sum())
    d = o - t
    if crit == "mse":
        term, seed = d * d, 2 * d
    elif crit == "mae":
        term, seed = d.abs(), torch.sign(d)
    else:
        oh, yh = o / o.abs().clamp_min(EPS), t / t.abs().clamp_min(EPS)
        tt = 1 - oh * yh
        term, seed = tt ** 3, torch.where(o.abs() < EPS, -3 * tt * tt * yh / EPS, torch.zeros_like(o))
    loss = term[m].sum() / M if M else torch.tensor(float("nan"), dtype=torch.float64)
    g = torch.where(m, seed / max(M, 1), torch.zeros_like(o)) if M else torch.zeros_like(o)
    return loss, g


def _close(got, want, tol):
    """max-norm relative error, or exact zeros where the reference is all zero"""
    got = got.detach().double().cpu().reshape(-1)
    want = want.detach().double().cpu().reshape(-1)
    if float(want.abs().max()) == 0.0:
        return bool((got == 0).all())
    return relerr(got, want) < tol


def adam64(p, grads, wd=WD):
    """One torch.optim.Adam step from zero moments (oracle.train_step's arithmetic) in fp64: the flat parameters after it."""
    out = []
    for k, w in p.items():
        w = w.double()
        g = grads[k] + wd * w
        mk, vk = (1 - B1) * g, (1 - B2) * g * g
        denom = vk.sqrt() / math.sqrt(1 - B2) + AEPS
        out.append((w - (LR / (1 - B1)) * (mk / denom)).reshape(-1))
    return torch.cat(out)


def _batch(pkg, bs, seed=6, mseed=1):
    ei = pkg.wdn_synth.collate_edge_index(pkg.wdn_synth.make_wdn_topology(NODES, PIPES, seed=0), NODES, bs)
    y = pkg.wdn_synth.collate_snapshots(pkg.wdn_synth.make_snapshots(bs, NODES, seed=seed), range(bs))
    mask = torch.from_numpy(pkg.wdn_synth.generate_batch_mask([NODES] * bs, 0.95, np.random.RandomState(mseed)))
    return ei, y, mask


# ------------------------------------------------------------------------------------------------ gatres_masked_loss
def test_masked_loss_on_constructed_vectors(pkg, lib):
    N = 3 * 1024 + 517                                   # not a multiple of the workgroup
    g = torch.Generator().manual_seed(5)
    out = torch.randn(N, generator=g)
    y = torch.randn(N, generator=g)
    mask = (torch.rand(N, generator=g) < 0.7).to(torch.uint8)
    out[10:20] = y[10:20]                                # ties: d = 0
    out[20:25] = torch.tensor([5e-13, -5e-13, 1e-12, -1e-12, 2e-12])      # |out| below, at, above eps
    out[25:30] = 0.0                                     # out = 0 ...
    y[28:33] = 0.0                                       # ... and y = 0 (both at 28, 29)
    y[20:25] = torch.tensor([2.0, 3.0, -1.0, 1.0, -4.0])
    y[40:42] = torch.tensor([3e-13, -7e-13])             # targets below eps
    out[40:42] = torch.tensor([1e-13, 1e-13])
    mask[10:42] = 1
    assert float(out[22]) == EPS
    st = pkg._native.current_stream(torch.device("cuda"))

    def run(crit, mk, fn="loss"):
        loss = torch.full((1,), -1.0, device="cuda")
        go = torch.full((N,), 7.0, device="cuda")
        o, t, m = out.cuda(), y.cuda(), mk.cuda()
        if fn == "mse":
            rc = lib.gatres_masked_mse(o.data_ptr(), t.data_ptr(), m.data_ptr(), loss.data_ptr(), go.data_ptr(), N, st)
        else:
            rc = lib.gatres_masked_loss(o.data_ptr(), t.data_ptr(), m.data_ptr(), pkg._native.CRITERIA[crit], loss.data_ptr(),
                                        go.data_ptr(), N, st)
        assert rc == 0
        torch.cuda.synchronize()
        return loss.cpu(), go.cpu()

    for crit in ("mse", "mae", "sce"):
        loss, go = run(crit, mask)
        l64, g64 = table(crit, out, y, mask)
        assert abs(float(loss) - float(l64)) <= 2e-6 * abs(float(l64)), (crit, float(loss), float(l64))
        assert relerr(go, g64) < 2e-6, crit
        assert (go[mask == 0] == 0).all()
        if crit == "mae":
            assert (go[10:20] == 0).all()                # sign(0) = 0
        if crit == "sce":
            # the clamped branch: below eps only (at exactly eps the norm branch is live); y = 0 gives y^ = 0
            assert (go[20:22] != 0).all() and (go[22:25] == 0).all() and (go[25:28] != 0).all() and (go[28:30] == 0).all()
            assert (go[40:42] != 0).all()
        # an empty mask: loss NaN, gradient 0
        loss0, go0 = run(crit, torch.zeros(N, dtype=torch.uint8))
        assert math.isnan(float(loss0)) and (go0 == 0).all()
    # MSE: the same bits as gatres_masked_mse
    a, b = run("mse", mask), run("mse", mask, fn="mse")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # an unknown criterion is refused
    o = torch.zeros(N, device="cuda")
    assert lib.gatres_masked_loss(o.data_ptr(), o.data_ptr(), o.data_ptr(), 3, o.data_ptr(), o.data_ptr(), N, st) == -1


# ------------------------------------------------------------------------------ one step of every path vs fp64
CONFIGS = {
    # the headline configuration: gatres_small, bs 32, hipGraph, window kernel at 8 CUs per snapshot
    "headline": dict(nb=NB, nc=NC, bs=32, kw=dict(use_graph=True)),
    "runtime_phases": dict(nb=3, nc=NC, bs=8, env={"GATRES_WINDOW_RUNTIME_PHASES": "1"}),
    "no_keep": dict(nb=3, nc=NC, bs=8, env={"GATRES_FUSED_NO_KEEP": "1"}),
    "nc8": dict(nb=3, nc=8, bs=8),                                        # the non-templated window kernel
    "rounds_bs64": dict(nb=3, nc=NC, bs=64),                              # the window kernel in two rounds
    "whole_bs64": dict(nb=3, nc=NC, bs=64, env={"GATRES_FUSED_NO_ROUNDS": "1"}),      # whole-segment tables
    "per_op": dict(nb=3, nc=NC, bs=8, kw=dict(fused=False)),
    "bf16": dict(nb=2, nc=64, bs=4, bf16=True),
}


@pytest.mark.parametrize("crit", ["mse", "mae", "sce"])
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_one_step_against_fp64(pkg, oracle, lib, monkeypatch, cfg, crit):
    c = CONFIGS[cfg]
    for k, v in c.get("env", {}).items():
        monkeypatch.setenv(k, v)
    nb, nc, bs = c["nb"], c["nc"], c["bs"]
    kw = dict(use_graph=False)
    kw.update(c.get("kw", {}))
    model, p = build(pkg, oracle, nb, nc, seed=3, fused=kw.get("fused", True))
    if c.get("bf16"):
        model.set_compute_dtype("bf16")
    ei, y, mask = _batch(pkg, bs)
    tr = pkg.GATResTrainer(model, ei.cuda(), NODES * bs, nodes_per_graph=[NODES] * bs, criterion=crit, **kw)
    assert tr.criterion == crit
    if cfg == "headline":
        assert tr.fused and tr.use_graph
        assert lib.gatres_fused_cus_per_segment(model._cmodel_ref(), tr.plan.ref()) == 8
        assert lib.gatres_fused_window_kernel(model._cmodel_ref(), tr.plan.ref()) == 1
    if cfg in ("runtime_phases", "no_keep", "nc8", "rounds_bs64"):
        assert tr.fused and lib.gatres_fused_window_kernel(model._cmodel_ref(), tr.plan.ref()) == 1
    if cfg == "whole_bs64":
        assert tr.fused and lib.gatres_fused_window_kernel(model._cmodel_ref(), tr.plan.ref()) == 0
    if cfg == "per_op":
        assert not tr.fused
    loss = tr.step(y.cuda(), y.cuda(), mask.cuda())
    torch.cuda.synchronize()
    assert tr.fault_count == 0
    # the loss stage on the kernels' own predictions: the table, to fp32 rounding
    l_k, g_k = table(crit, tr.out, y, mask)
    assert abs(float(loss) - float(l_k)) <= 1e-5 * abs(float(l_k)) + 1e-30, (float(loss), float(l_k))
    assert _close(tr.g_out, g_k, 1e-6)
    # the forward and backward against the oracle, seeded with that gradient
    xin = y.clone()
    xin[mask] = 0
    if c.get("bf16"):
        leaves = {k: v.clone().requires_grad_(True) for k, v in p.items()}
        o_ref = oracle.gatres_forward_bf16(leaves, xin, ei, num_blocks=nb)
    else:
        leaves = {k: v.double().clone().requires_grad_(True) for k, v in p.items()}
        o_ref = oracle.gatres_forward(leaves, xin.double(), ei, num_blocks=nb)
    gr = torch.autograd.grad(o_ref, list(leaves.values()), grad_outputs=g_k.to(o_ref.dtype).reshape(o_ref.shape))
    g_ref = dict(zip(leaves, (t.double() for t in gr)))
    flat_ref = torch.cat([t.reshape(-1) for t in g_ref.values()])
    if c.get("bf16"):
        o_b = o_ref.detach().double().reshape(-1)
        e_out = float((tr.out.cpu().double().reshape(-1) - o_b).norm() / o_b.norm())
        assert e_out < 2e-3, e_out
        if float(flat_ref.abs().max()) == 0.0:
            assert bool((tr.grads == 0).all())
        else:
            e_g = float((tr.grads.cpu().double() - flat_ref).norm() / flat_ref.norm())
            assert e_g < 2e-3, e_g
    else:
        e_out = relerr(tr.out, o_ref)
        assert e_out < 1e-5, e_out
        assert _close(tr.grads, flat_ref, 1e-4), relerr(tr.grads, flat_ref)
    if c.get("bf16"):
        return                    # (bf16 gradients are judged above; Adam's sign-like first step would amplify their rounding)
    # Adam (from zero moments) on that gradient
    diff = (model.flat_parameters.detach().cpu().double() - adam64(p, g_ref)).abs()
    note(f"criterion {crit}, {cfg}: out error, flat gradient error, max |dp|, fraction of params off by > 1e-5",
         [e_out, relerr(tr.grads, flat_ref) if float(flat_ref.abs().max()) else 0.0, float(diff.max()),
          float((diff > 1e-5).double().mean())])
    assert float(diff.max()) <= 2 * LR * 1.01 and float((diff > 1e-5).double().mean()) < 0.01
    if crit == "sce":
        # a generic batch: no prediction below 1e-12 -- the gradient is exactly zero, the update weight decay through Adam
        assert float(tr.out.abs().min()) >= EPS and bool((tr.grads == 0).all())
        assert float(diff.max()) < 1e-6


@pytest.mark.parametrize("crit", ["mse", "mae", "sce"])
def test_blocked_launches_equal_the_per_op_pair(pkg, oracle, monkeypatch, crit):
    """nc 128, bf16: GATRES_BLOCKED=1 and the per-op kernels give the same bits with every criterion."""
    nb, nc, bs = 3, 128, 4
    ei, y, mask = _batch(pkg, bs, seed=11, mseed=2)
    res = []
    for blocked in (True, False):
        if blocked:
            monkeypatch.setenv("GATRES_BLOCKED", "1")
        else:
            monkeypatch.delenv("GATRES_BLOCKED", raising=False)
        model, p = build(pkg, oracle, nb, nc, seed=11)
        model.set_compute_dtype("bf16")
        tr = pkg.GATResTrainer(model, ei.cuda(), NODES * bs, nodes_per_graph=[NODES] * bs, use_graph=False, fused=False,
                               criterion=crit)
        assert bool(pkg._native.load().gatres_blocked_supported(model._cmodel_ref(), tr.plan.ref())) == blocked
        losses = [float(tr.step(y.cuda(), y.cuda(), mask.cuda())) for _ in range(2)]
        res.append((tr.out.clone(), losses, tr.grads.clone(), model.flat_parameters.clone(), tr.g_out.clone()))
    assert res[0][1] == res[1][1]
    for a, b in zip(res[0], res[1]):
        if torch.is_tensor(a):
            assert torch.equal(a, b)
    l_k, g_k = table(crit, res[0][0], y, mask)
    assert abs(res[0][1][1] - float(l_k)) <= 1e-5 * abs(float(l_k)) and _close(res[0][4], g_k, 1e-6)


# ------------------------------------------------------------------ window kernel instantiations, bit for bit
@pytest.mark.parametrize("crit", ["mae", "sce"])
def test_window_kernel_instantiations_are_bit_identical(pkg, oracle, lib, monkeypatch, crit):
    """The training launches with another criterion than MSE take instantiations of their own (k_window.hip: key bit 0x8000,
    0xdf16 / 0x9f16) or the run-time-phases kernel: every one, and the launch without keep-in-LDS (the stand-alone loss pass),
    gives the bits of the run-time-phases kernel."""
    bs = 8
    ei, y, mask = _batch(pkg, bs, seed=9, mseed=4)
    ei, y, mask = ei.cuda(), y.cuda(), mask.cuda()

    def run(env):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        model, _ = build(pkg, oracle, NB, NC, seed=13)
        if crit == "sce":                                 # (a live SCE gradient: predictions of 0 on every node)
            with torch.no_grad():
                model.lin1.weight.zero_()
                model.lin1.bias.zero_()
        tr = pkg.GATResTrainer(model, ei, NODES * bs, nodes_per_graph=[NODES] * bs, use_graph=False, criterion=crit)
        assert lib.gatres_fused_window_kernel(model._cmodel_ref(), tr.plan.ref()) == 1
        out = {}
        tr.step(y, y, mask)
        out["pred"], out["loss"], out["grads"], out["g_out"] = tr.out.clone(), tr.loss.clone(), tr.grads.clone(), tr.g_out.clone()
        tr.step(y, y, mask)
        out["params"], out["loss2"] = model.flat_parameters.clone(), tr.loss.clone()
        for k in env:
            monkeypatch.delenv(k)
        return out

    ref = run({"GATRES_WINDOW_RUNTIME_PHASES": "1"})
    if crit == "sce":
        assert float(ref["grads"].abs().max()) > 0
    for m in ("65535", "49151", "7167", "4095", "2047", "1023", "511"):        # (49151 = 0xbfff: without the probed dispatch)
        got = run({"GATRES_WINDOW_PH_MASK": m})
        for k, v in ref.items():
            assert torch.equal(v, got[k]), (m, k)
    got = run({"GATRES_FUSED_NO_KEEP": "1"})
    for k, v in ref.items():
        assert torch.equal(v, got[k]), ("no-keep", k)


# --------------------------------------------------------------------------------------------------- SCE branches
def test_sce_clamped_branch_against_fp64(pkg, oracle, lib):
    """lin1.weight = 0 and lin1.bias = 0: every prediction is 0 (below eps), the gradient -3 y^ / (eps M) on the masked nodes
    -- the large gradients reach lin1 only (a zero weight passes nothing further down)."""
    bs = 32
    model, p = build(pkg, oracle, NB, NC, seed=3)
    with torch.no_grad():
        model.lin1.weight.zero_()
        model.lin1.bias.zero_()
    p = {k: v.clone() for k, v in p.items()}
    p["lin1.weight"].zero_()
    p["lin1.bias"].zero_()
    ei, y, mask = _batch(pkg, bs)
    tr = pkg.GATResTrainer(model, ei.cuda(), NODES * bs, nodes_per_graph=[NODES] * bs, use_graph=True, criterion="sce")
    loss = tr.step(y.cuda(), y.cuda(), mask.cuda())
    torch.cuda.synchronize()
    assert bool((tr.out == 0).all())
    l_k, g_k = table("sce", tr.out, y, mask)
    assert float(loss) == pytest.approx(float(l_k), rel=1e-6) and float(l_k) == 1.0
    assert relerr(tr.g_out, g_k) < 1e-6 and float(g_k.abs().max()) > 1e8
    xin = y.clone().double()
    xin[mask] = 0
    leaves = {k: v.double().clone().requires_grad_(True) for k, v in p.items()}
    o = oracle.gatres_forward(leaves, xin, ei, num_blocks=NB)
    gr = dict(zip(leaves, torch.autograd.grad(o, list(leaves.values()), grad_outputs=g_k.reshape(o.shape))))
    flat = torch.cat([t.reshape(-1) for t in gr.values()])
    e = relerr(tr.grads, flat)
    note("criterion sce, clamped branch (out = 0): flat gradient error vs fp64", e)
    assert e < 1e-5, e
    assert float(flat.abs().max()) > 1e8
    diff = (model.flat_parameters.detach().cpu().double() - adam64(p, gr)).abs()
    assert float(diff.max()) <= 2 * LR * 1.01 and float((diff > 1e-5).double().mean()) < 0.01


# ----------------------------------------------------------------------------------------------- MSE unchanged
def test_explicit_mse_equals_the_default(pkg, oracle):
    res = []
    for kw in ({}, {"criterion": "mse"}):
        model, _ = build(pkg, oracle, NB, NC, seed=5)
        ei, y, mask = _batch(pkg, 32)
        tr = pkg.GATResTrainer(model, ei.cuda(), NODES * 32, nodes_per_graph=[NODES] * 32, use_graph=True, **kw)
        assert tr.criterion == "mse"
        snaps = pkg.wdn_synth.make_snapshots(3 * 32, NODES, seed=6).cuda()
        losses = []
        for it in range(3):
            x = snaps[it * 32:(it + 1) * 32].reshape(-1)
            losses.append(tr.step(x, x).clone())
        res.append((torch.cat(losses), model.flat_parameters.clone(), tr.exp_avg.clone(), tr.exp_avg_sq.clone(),
                    tr.out.clone()))
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_criterion_is_read_only(pkg, oracle):
    model, _ = build(pkg, oracle, 3, NC, seed=5)
    ei, _, _ = _batch(pkg, 2)
    tr = pkg.GATResTrainer(model, ei.cuda(), NODES * 2, nodes_per_graph=[NODES] * 2, criterion="mae")
    with pytest.raises(AttributeError):
        tr.criterion = "mse"
    assert tr.criterion == "mae"


# ------------------------------------------------------------------------------------------------ fit_epoch
@pytest.mark.parametrize("device_metrics", [False, True])
def test_fit_epoch_mae_with_a_ragged_tail_equals_single_steps(pkg, oracle, device_metrics):
    """Two epochs of 4 + 4 + 3 graphs through fit_epoch (the in-place / captured sequences, the ragged batch on the sibling
    trainer) with MAE equal, bit for bit, the same batches stepped one by one on the same device masks."""
    one = pkg.wdn_synth.make_wdn_topology()
    raw = pkg.wdn_synth.make_snapshots(11, 388, seed=3) * 6 + 35
    st = pkg.SnapshotStore(raw, one, device="cuda")
    nb, nc, bs = 3, 32, 4
    model, _ = build(pkg, oracle, nb, nc, seed=8)
    tr = pkg.GATResTrainer(model, st.edge_index(bs), 388 * bs, nodes_per_graph=[388] * bs, seed=5, targets_are_inputs=True,
                           use_graph=True, criterion="mae")
    kw = dict(metric_fn_dict=pkg.evaluation.get_metric_fn_collection("train"), device_metrics=True) if device_metrics else {}
    losses = [tr.fit_epoch(st, bs, shuffle=True, generator=torch.Generator().manual_seed(7 + ep), **kw)[0] for ep in range(2)]
    assert tr.optimizer_step == 6
    sib = tr._siblings[3]
    assert sib.criterion == "mae"
    l_k, _ = table("mae", sib.out, sib.x, sib.mask)        # the ragged batch's loss is the MAE of its predictions
    assert abs(float(sib.loss) - float(l_k)) <= 1e-5 * float(l_k)
    twin, _ = build(pkg, oracle, nb, nc, seed=8)
    t4 = pkg.GATResTrainer(twin, st.edge_index(bs), 388 * bs, nodes_per_graph=[388] * bs, seed=5, targets_are_inputs=True,
                           use_graph=False, criterion="mae")
    t3 = pkg.GATResTrainer(twin, st.edge_index(3), 388 * 3, nodes_per_graph=[388] * 3, seed=5, targets_are_inputs=True,
                           use_graph=False, criterion="mae", _share_state_with=t4)
    for ep in range(2):
        tot, n = 0.0, 0
        for xb, eib, ng in st.batches(bs, shuffle=True, generator=torch.Generator().manual_seed(7 + ep)):
            t = t4 if ng == bs else t3
            t.invalidate_weights()
            loss = float(t.step(xb, xb)) * ng
            l_k, _ = table("mae", t.out, xb, t.mask)
            assert abs(loss / ng - float(l_k)) <= 1e-5 * float(l_k)
            tot += loss
            n += ng
        assert abs(losses[ep] - tot / n) < 1e-6 * abs(tot / n), ep
    assert torch.equal(model.flat_parameters, twin.flat_parameters)


# ---------------------------------------------------------------------------------------------- data parallel
@pytest.mark.parametrize("buckets", [1, 2])
def test_mae_collective_path_at_world_one_equals_the_plain_step(pkg, oracle, buckets):
    bs = 32
    snaps = pkg.wdn_synth.make_snapshots(3 * bs, NODES, seed=8).cuda()
    ei, _, _ = _batch(pkg, bs)
    for use_graph in (False, True):
        res = []
        for split in (False, True):
            model, _ = build(pkg, oracle, NB, NC, seed=2)
            tr = pkg.GATResTrainer(model, ei.cuda(), NODES * bs, nodes_per_graph=[NODES] * bs, use_graph=use_graph,
                                   force_collective_path=split, criterion="mae")
            tr.seed = 77
            tr.fused_buckets = buckets
            assert tr.split == split
            losses = []
            for it in range(3):
                y = snaps[it * bs:(it + 1) * bs].reshape(-1)
                losses.append(float(tr.step(y, y)))
                l_k, _ = table("mae", tr.out, y, tr.mask)
                assert abs(losses[-1] - float(l_k)) <= 1e-5 * float(l_k)
                if split:
                    assert len(tr.reducer.last_buckets) == buckets
            res.append((losses, model.flat_parameters.clone(), tr.mask.clone(), tr.grads.clone()))
        assert res[0][0] == res[1][0], use_graph
        assert torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2]) and torch.equal(res[0][3], res[1][3])


def _rank_main_mae(rank, world, port, out_dir):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist
    import test_gpu_two_ranks as T
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import gnn_pressure_estimation_amd as G
        from oracle import gatres_oracle as O
        c = T.CASES["fused"]
        torch.cuda.set_device(0)
        one, snaps, masks, B = T._data(G, "fused", world)
        rows = G.dp.shard_graphs(B, rank, world)
        per = len(rows)
        ei = G.wdn_synth.collate_edge_index(one, NODES, per).cuda()
        model = T._build(G, O, c, seed=1)
        tr = G.GATResTrainer(model, ei, NODES * per, nodes_per_graph=[NODES] * per, seed=5, use_graph=False, fused=True,
                             blocks_per_bucket=1, criterion="mae")
        assert tr.world == world and tr.split
        grads0, losses = None, []
        for s in range(T.STEPS):
            x = G.wdn_synth.collate_snapshots(snaps[s], rows).cuda()
            m = masks[s][rows[0] * NODES:(rows[-1] + 1) * NODES].cuda()
            loss = tr.step(x, x, m)
            if s == 0:
                grads0 = tr.grads.clone().cpu()
            l = loss.detach().clone().cpu()
            dist.all_reduce(l)
            losses.append(float(l) / world)
        torch.cuda.synchronize()
        torch.save({"grads0": grads0, "losses": losses, "params": model.flat_parameters.clone().cpu(),
                    "faults": tr.fault_count}, os.path.join(out_dir, f"r{rank}.pt"))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def _single_main_mae(out_dir, world):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import test_gpu_two_ranks as T
    import gnn_pressure_estimation_amd as G
    from oracle import gatres_oracle as O
    one, snaps, masks, B = T._data(G, "fused", world)
    ei = G.wdn_synth.collate_edge_index(one, NODES, B).cuda()
    model = T._build(G, O, T.CASES["fused"], seed=1)
    tr = G.GATResTrainer(model, ei, NODES * B, nodes_per_graph=[NODES] * B, seed=5, use_graph=False, fused=True,
                         criterion="mae")
    grads0, losses = None, []
    for s in range(T.STEPS):
        x = G.wdn_synth.collate_snapshots(snaps[s], range(B)).cuda()
        loss = tr.step(x, x, masks[s].cuda())
        if s == 0:
            grads0 = tr.grads.clone().cpu()
        losses.append(float(loss))
    torch.save({"grads0": grads0, "losses": losses, "params": model.flat_parameters.clone().cpu()},
               os.path.join(out_dir, "single.pt"))


def test_mae_two_ranks_on_one_gpu_equal_one_process(tmp_path, fork_ctx):
    import test_gpu_two_ranks as T
    world = 2
    port = T._free_port()
    T._run_all([fork_ctx.Process(target=_single_main_mae, args=(str(tmp_path), world))])
    T._run_all([fork_ctx.Process(target=_rank_main_mae, args=(r, world, port, str(tmp_path))) for r in range(world)])
    rk = [torch.load(tmp_path / f"r{r}.pt") for r in range(world)]
    one = torch.load(tmp_path / "single.pt")
    for r in rk:
        assert r["faults"] == 0
        assert torch.equal(r["grads0"], rk[0]["grads0"]) and torch.equal(r["params"], rk[0]["params"])
    g = one["grads0"]
    assert float((rk[0]["grads0"] / world - g).abs().max() / g.abs().max()) < 2e-5
    for a, b in zip(rk[0]["losses"], one["losses"]):
        assert abs(a - b) < 1e-5 * abs(b)
    assert float((rk[0]["params"] - one["params"]).abs().max()) < 2e-5


# ---------------------------------------------------------------------------------------------------- AutoClip
def test_mae_with_autoclip_clips_the_mae_gradient(pkg, oracle):
    """The clip sees the MAE gradient: the norm of every update against the fp64 gradient of the MAE (seeded on the kernels'
    predictions), the clip value against the percentile of that history (the reference's rule, restated)."""
    nb, bs, pct = 3, 8, 30.0
    model, _ = build(pkg, oracle, nb, NC, seed=4)
    ei, _, _ = _batch(pkg, bs)
    tr = pkg.GATResTrainer(model, ei.cuda(), NODES * bs, nodes_per_graph=[NODES] * bs, use_graph=True, criterion="mae",
                           use_gradient_clipping=True, percentile=pct)
    snaps = pkg.wdn_synth.make_snapshots(4 * bs, NODES, seed=12)
    rng = np.random.RandomState(5)
    hist = []
    names = list(oracle.param_shapes(nb, NC))
    for it in range(4):
        y = pkg.wdn_synth.collate_snapshots(snaps, range(it * bs, (it + 1) * bs))
        mask = torch.from_numpy(pkg.wdn_synth.generate_batch_mask([NODES] * bs, 0.95, rng))
        flat = model.flat_parameters.detach().cpu().double()
        p, off = {}, 0
        for k, shp in oracle.param_shapes(nb, NC).items():
            n = int(np.prod(shp))
            p[k] = flat[off:off + n].reshape(shp).clone().requires_grad_(True)
            off += n
        tr.step(y.cuda(), y.cuda(), mask.cuda())
        torch.cuda.synchronize()
        _, g_k = table("mae", tr.out, y, mask)
        xin = y.double().clone()
        xin[mask] = 0
        o = oracle.gatres_forward(p, xin, ei, num_blocks=nb)
        gr = torch.autograd.grad(o, [p[k] for k in names], grad_outputs=g_k.reshape(o.shape))
        n64 = math.sqrt(sum(float(t.pow(2).sum()) for t in gr))
        hist.append(n64)
        c = float(np.percentile(np.asarray(hist), pct))
        assert abs(float(tr.last_grad_norm) - n64) <= 1e-4 * n64, (it, float(tr.last_grad_norm), n64)
        assert abs(float(tr.last_clip_value) - c) <= 1e-4 * c, it
        assert abs(float(tr.last_clip_coef) - min(1.0, c / (n64 + 1e-6))) <= 1e-4, it
    h = tr.grad_norm_history()
    assert len(h) == 4 and np.allclose(h, hist, rtol=1e-4)
