"""Kernels on irregular graphs (tests/irregular_graphs.py: rows of 6 / 7 / 32 / 33 entries, hubs in ragged last waves,
isolated nodes, self loops, duplicate and directed edges) against plain fp64 statements of the same operations.

  * bf16 sparse kernels, one launch each, element by element against tests/sparse_refs.py on the same bf16 inputs:
    bf16 stores |got - ref| <= 2^-8 |ref| + C_BF16 ref_abs, fp32 side outputs |got - ref| <= C_F32 ref_abs, where ref_abs
    is the operation on absolute values (it bounds fp32 summation error under cancellation);
  * fp32 fused training steps (window kernel, split segments, a seeded fuzz) against the oracle: predictions and loss
    within 2e-5, the flat gradient per tensor against fp64 (test_gpu_model.check_gradients_vs_fp64);
  * bf16 whole models on a hub graph and on rows of 7 .. 32 entries (blocked kernels on and off) against the
    bf16-rounding oracle at the shallow-model bounds of test_gpu_bf16.py."""
import numpy as np
import pytest
import torch

import irregular_graphs as IG
import sparse_refs as R
from test_gpu_model import build, check_gradients_vs_fp64, note, relerr      # noqa: E402

pytestmark = pytest.mark.gpu

BF16 = 1
# Element-wise bounds, each about 4x the worst c measured over every graph, width and lane-feature instance below and the
# blocked kernels' outputs (parity report, "irregular bf16 ..."): bf16 stores 2.3e-8, alpha 5.2e-7, the other fp32 side
# outputs (g_e, g_a_dst, g_a_src, lin1) 1.1e-7.
C_BF16 = 9e-8
C_ALPHA = 2e-6
C_F32 = 4.3e-7
KERNEL_GRAPHS = ("sym_le32", "dir_le32", "sym_hub", "dir_hub_shuffled")


def _st():
    import gnn_pressure_estimation_amd as G
    return G._native.current_stream(torch.device("cuda"))


def _bf(g, *shape):
    return torch.randn(*shape, generator=g).bfloat16().cuda()


def _f(g, *shape):
    return torch.randn(*shape, generator=g).cuda()


def _plan(pkg, g):
    plan = pkg.GraphPlan(g.edge_index.cuda(), g.num_nodes, device="cuda", segments=False)   # (caller order = plan order)
    assert plan.flags == g.flags and not plan.flags & 4
    return plan


@pytest.mark.parametrize("H,C", [(1, 32), (2, 32), (1, 64), (2, 64), (1, 128), (2, 128)])
def test_bf16_sparse_kernels_vs_fp64(pkg, lib, H, C, monkeypatch):
    """gatres_t_gat_aggregate_fwd / _bwd_dst / _bwd_src (and, width C, gatres_t_mean_residual_relu_fwd / gatres_t_mean_bwd)
    at dtype = bf16 on rows of 6 / 7 / 32 / 33+ entries -- slot paths, the edge loops and the whole-wave hub path of
    k_aggregate.hip -- with 4 and 8 features per lane."""
    chk = pkg._native.check
    HC = H * C
    need = {}
    for name in KERNEL_GRAPHS:
        g = IG.named(name)
        n, ei = g.num_nodes, g.edge_index
        plan = _plan(pkg, g)
        rc = IG.row_counts(ei, n)
        assert rc["gat_in"].max() > 32 or name.endswith("le32")          # hub rows reach the whole-wave path
        Eg = plan.num_edges_gat
        gp = plan.ref()
        gen = torch.Generator().manual_seed(100 * H + C + len(name))
        h, a_s, a_d, bias = _bf(gen, n, HC), _f(gen, n, H), _f(gen, n, H), _f(gen, HC)
        g_out, g_e_in, g_ad_in = _bf(gen, n, HC), _f(gen, Eg, H), _f(gen, n, H)
        att_s, att_d = _f(gen, HC), _f(gen, HC)
        y, x0, g_pre = _bf(gen, n, C), _bf(gen, n, C), _bf(gen, n, C)
        src, dst = R.gat_edges(ei, n)
        assert len(src) == Eg
        out_ref, out_abs, al_ref = R.gat_aggregate_fwd(src, dst, h.cpu(), a_s.cpu(), a_d.cpu(), bias.cpu(), n, H, True)
        alpha_in = al_ref.float().cuda()
        ge_ref, ge_abs, gad_ref, gad_abs = R.gat_aggregate_bwd_dst(src, dst, g_out.cpu(), h.cpu(), alpha_in.cpu(), a_s.cpu(),
                                                                   a_d.cpu(), n, H)
        gh_ref, gh_abs, gas_ref, gas_abs = R.gat_aggregate_bwd_src(src, dst, g_out.cpu(), alpha_in.cpu(), g_e_in.cpu(),
                                                                   g_ad_in.cpu(), att_s.cpu(), att_d.cpu(), n, H)
        m_ref, m_abs = R.mean_residual_relu(ei, y.cpu(), x0.cpu(), n)
        mb_ref, mb_abs = R.mean_bwd(ei, g_pre.cpu(), n)
        only_loop = torch.from_numpy(np.nonzero(rc["gat_in"] == 1)[0])       # rows whose only entry is the self loop
        assert len(only_loop) >= len(g.isolated) >= 2
        loop_pos = torch.searchsorted(dst.contiguous(), only_loop)         # (dst-sorted: the row's one position)
        for lf in ("4", "8"):
            monkeypatch.setenv("GATRES_AGG_LANE_FEATURES", lf)
            out = torch.full((n, HC), float("nan"), device="cuda").bfloat16()
            alpha = torch.full((Eg, H), float("nan"), device="cuda")
            chk(lib.gatres_t_gat_aggregate_fwd(gp, h.data_ptr(), a_s.data_ptr(), a_d.data_ptr(), bias.data_ptr(), out.data_ptr(),
                                               alpha.data_ptr(), H, C, 1, BF16, _st()), "agg fwd")
            g_e, g_ad = torch.full((Eg, H), float("nan"), device="cuda"), torch.full((n, H), float("nan"), device="cuda")
            chk(lib.gatres_t_gat_aggregate_bwd_dst(gp, g_out.data_ptr(), h.data_ptr(), alpha_in.data_ptr(), a_s.data_ptr(),
                                                   a_d.data_ptr(), g_e.data_ptr(), g_ad.data_ptr(), H, C, BF16, _st()), "bwd dst")
            g_h = torch.full((n, HC), float("nan"), device="cuda").bfloat16()
            g_as = torch.full((n, H), float("nan"), device="cuda")
            chk(lib.gatres_t_gat_aggregate_bwd_src(gp, g_out.data_ptr(), alpha_in.data_ptr(), g_e_in.data_ptr(),
                                                   g_ad_in.data_ptr(), att_s.data_ptr(), att_d.data_ptr(), g_h.data_ptr(),
                                                   g_as.data_ptr(), H, C, BF16, _st()), "bwd src")
            res = [("out", out, out_ref, out_abs, 2.0 ** -8, C_BF16), ("alpha", alpha, al_ref, al_ref, 0.0, C_ALPHA),
                   ("g_e", g_e, ge_ref, ge_abs, 0.0, C_F32), ("g_a_dst", g_ad, gad_ref, gad_abs, 0.0, C_F32),
                   ("g_h", g_h, gh_ref, gh_abs, 2.0 ** -8, C_BF16), ("g_a_src", g_as, gas_ref, gas_abs, 0.0, C_F32)]
            if H == 1:                                                       # (the mean kernels have width C only)
                mo = torch.full((n, C), float("nan"), device="cuda").bfloat16()
                chk(lib.gatres_t_mean_residual_relu_fwd(gp, y.data_ptr(), x0.data_ptr(), mo.data_ptr(), C, BF16, _st()), "mean")
                gy = torch.full((n, C), float("nan"), device="cuda").bfloat16()
                chk(lib.gatres_t_mean_bwd(gp, g_pre.data_ptr(), gy.data_ptr(), C, BF16, _st()), "mean bwd")
                res += [("mean", mo, m_ref, m_abs, 2.0 ** -8, C_BF16), ("mean_bwd", gy, mb_ref, mb_abs, 2.0 ** -8, C_BF16)]
            torch.cuda.synchronize()
            for what, got, ref, ref_abs, rel, _ in res:
                key = ("bf16 " if rel else "fp32 ") + what
                need[key] = max(need.get(key, 0.0), R.excess(got, ref, ref_abs, rel))
            note(f"irregular bf16 sparse kernels H{H} C{C}: worst c needed per output (bounds: C_BF16 {C_BF16:.2g}, "
                 f"C_ALPHA {C_ALPHA:.2g}, C_F32 {C_F32:.2g})", need)
            for what, got, ref, ref_abs, rel, c in res:
                R.assert_within(f"{name} lane features {lf}: {what}", got, ref, ref_abs, rel, c)
            # exact: a row whose only entry is its self loop has alpha = 1 and passes its own row through
            assert torch.equal(alpha.cpu()[loop_pos], torch.ones(len(only_loop), H))
            iso = torch.tensor(g.isolated)
            assert torch.equal(out.cpu()[iso], (h.float().cpu()[iso] + bias.cpu()).relu().bfloat16())
            if H == 1:                                                       # mean of an isolated node = 0
                assert torch.equal(mo.cpu()[iso], x0.cpu()[iso].relu())
                assert not gy.cpu()[iso].float().any()


@pytest.mark.parametrize("H,C", [(2, 32), (1, 64)])
@pytest.mark.parametrize("dtype", [0, BF16], ids=["fp32", "bf16"])
def test_sparse_kernels_wide_offset_instances(pkg, lib, dtype, H, C, monkeypatch):
    """Every sparse kernel of k_aggregate.hip is compiled twice: with 32-bit byte offsets, and with 64-bit ones for tables of
    4 GiB and more (offsets_fit_32), which the launchers take by themselves there.  GATRES_AGG_WIDE_OFFSETS=1 takes the wide
    instance at any size.  Only the addressing differs, so the five kernels' outputs must equal the narrow instance's BYTE FOR
    BYTE -- on hub graphs (slot paths, edge loops, the whole-wave path), fp32 and bf16, 4 and 8 features per lane -- and they
    are held to tests/sparse_refs.py by the bounds above (fp32 stores: the bound of the fp32 results)."""
    chk = pkg._native.check
    HC = H * C
    cast = (lambda t: t.bfloat16()) if dtype == BF16 else (lambda t: t)
    rel, c_store = (2.0 ** -8, C_BF16) if dtype == BF16 else (0.0, C_F32)
    for name in ("sym_hub", "dir_hub_shuffled"):
        g = IG.named(name)
        n, ei = g.num_nodes, g.edge_index
        plan = _plan(pkg, g)
        Eg, gp = plan.num_edges_gat, plan.ref()
        gen = torch.Generator().manual_seed(7 * H + C + dtype + len(name))
        h, g_out, y, x0, g_pre = (cast(_f(gen, n, w)) for w in (HC, HC, C, C, C))
        a_s, a_d, bias, g_ad_in = _f(gen, n, H), _f(gen, n, H), _f(gen, HC), _f(gen, n, H)
        g_e_in, att_s, att_d = _f(gen, Eg, H), _f(gen, HC), _f(gen, HC)
        src, dst = R.gat_edges(ei, n)
        out_ref, out_abs, al_ref = R.gat_aggregate_fwd(src, dst, h.cpu(), a_s.cpu(), a_d.cpu(), bias.cpu(), n, H, True)
        alpha_in = al_ref.float().cuda()
        ge_ref, ge_abs, gad_ref, gad_abs = R.gat_aggregate_bwd_dst(src, dst, g_out.cpu(), h.cpu(), alpha_in.cpu(), a_s.cpu(),
                                                                   a_d.cpu(), n, H)
        gh_ref, gh_abs, gas_ref, gas_abs = R.gat_aggregate_bwd_src(src, dst, g_out.cpu(), alpha_in.cpu(), g_e_in.cpu(),
                                                                   g_ad_in.cpu(), att_s.cpu(), att_d.cpu(), n, H)
        m_ref, m_abs = R.mean_residual_relu(ei, y.cpu(), x0.cpu(), n)
        mb_ref, mb_abs = R.mean_bwd(ei, g_pre.cpu(), n)
        refs = {"out": (out_ref, out_abs, rel, c_store), "alpha": (al_ref, al_ref, 0.0, C_ALPHA),
                "g_e": (ge_ref, ge_abs, 0.0, C_F32), "g_a_dst": (gad_ref, gad_abs, 0.0, C_F32),
                "g_h": (gh_ref, gh_abs, rel, c_store), "g_a_src": (gas_ref, gas_abs, 0.0, C_F32),
                "mean": (m_ref, m_abs, rel, c_store), "mean_bwd": (mb_ref, mb_abs, rel, c_store)}

        def run():
            nan = lambda *s: cast(torch.full(s, float("nan"), device="cuda"))
            nanf = lambda *s: torch.full(s, float("nan"), device="cuda")
            o = dict(out=nan(n, HC), alpha=nanf(Eg, H), g_e=nanf(Eg, H), g_a_dst=nanf(n, H), g_h=nan(n, HC), g_a_src=nanf(n, H),
                     mean=nan(n, C), mean_bwd=nan(n, C))
            chk(lib.gatres_t_gat_aggregate_fwd(gp, h.data_ptr(), a_s.data_ptr(), a_d.data_ptr(), bias.data_ptr(),
                                               o["out"].data_ptr(), o["alpha"].data_ptr(), H, C, 1, dtype, _st()), "agg fwd")
            chk(lib.gatres_t_gat_aggregate_bwd_dst(gp, g_out.data_ptr(), h.data_ptr(), alpha_in.data_ptr(), a_s.data_ptr(),
                                                   a_d.data_ptr(), o["g_e"].data_ptr(), o["g_a_dst"].data_ptr(), H, C, dtype,
                                                   _st()), "bwd dst")
            chk(lib.gatres_t_gat_aggregate_bwd_src(gp, g_out.data_ptr(), alpha_in.data_ptr(), g_e_in.data_ptr(),
                                                   g_ad_in.data_ptr(), att_s.data_ptr(), att_d.data_ptr(), o["g_h"].data_ptr(),
                                                   o["g_a_src"].data_ptr(), H, C, dtype, _st()), "bwd src")
            chk(lib.gatres_t_mean_residual_relu_fwd(gp, y.data_ptr(), x0.data_ptr(), o["mean"].data_ptr(), C, dtype, _st()), "mean")
            chk(lib.gatres_t_mean_bwd(gp, g_pre.data_ptr(), o["mean_bwd"].data_ptr(), C, dtype, _st()), "mean bwd")
            torch.cuda.synchronize()
            return o

        need = {}
        for lf in ("4", "8"):
            monkeypatch.setenv("GATRES_AGG_LANE_FEATURES", lf)
            monkeypatch.delenv("GATRES_AGG_WIDE_OFFSETS", raising=False)
            narrow = run()
            monkeypatch.setenv("GATRES_AGG_WIDE_OFFSETS", "1")
            wide = run()
            for what, (ref, ref_abs, r, c) in refs.items():
                need[what] = max(need.get(what, 0.0), R.excess(wide[what], ref, ref_abs, r))
            note(f"irregular sparse kernels, wide offsets, {'bf16' if dtype == BF16 else 'fp32'} H{H} C{C} {name}: worst c needed "
                 f"per output (bounds: stores {c_store:.2g}, C_ALPHA {C_ALPHA:.2g}, C_F32 {C_F32:.2g})", need)
            for what, (ref, ref_abs, r, c) in refs.items():
                assert torch.equal(wide[what].view(torch.uint8), narrow[what].view(torch.uint8)), (name, lf, what)
                R.assert_within(f"{name} lane features {lf}, wide offsets: {what}", wide[what], ref, ref_abs, r, c)


@pytest.mark.parametrize("nc", [32, 64, 128])
def test_bf16_lin0_lin1_vs_fp64(pkg, lib, nc):
    """gatres_t_lin0_fwd (bf16 store of xm w + b) and gatres_t_lin1_fwd (fp32 sum over bf16 rows) on a ragged row count."""
    n = 1001
    gen = torch.Generator().manual_seed(nc)
    x, w0, b0 = _f(gen, n), _f(gen, nc), _f(gen, nc)
    mask = (torch.rand(n, generator=gen) < 0.3).to(torch.uint8).cuda()
    out = torch.full((n, nc), float("nan"), device="cuda").bfloat16()
    pkg._native.check(lib.gatres_t_lin0_fwd(x.data_ptr(), mask.data_ptr(), w0.data_ptr(), b0.data_ptr(), out.data_ptr(), n,
                                            nc, BF16, _st()), "lin0")
    z, w1, b1 = _bf(gen, n, nc), _f(gen, nc), _f(gen, 1)
    o1 = torch.full((n,), float("nan"), device="cuda")
    pkg._native.check(lib.gatres_t_lin1_fwd(z.data_ptr(), w1.data_ptr(), b1.data_ptr(), o1.data_ptr(), n, nc, BF16, _st()),
                      "lin1")
    torch.cuda.synchronize()
    xm = torch.where(mask.bool(), torch.zeros_like(x), x).double().cpu()
    ref0 = xm[:, None] * w0.double().cpu()[None] + b0.double().cpu()[None]
    abs0 = (xm[:, None] * w0.double().cpu()[None]).abs() + b0.double().cpu().abs()[None]
    ref1 = z.double().cpu() @ w1.double().cpu() + b1.double().cpu()
    abs1 = z.double().cpu().abs() @ w1.double().cpu().abs() + b1.double().cpu().abs()
    need = [R.excess(out, ref0, abs0, 2.0 ** -8), R.excess(o1, ref1, abs1, 0.0)]
    note(f"irregular bf16 lin0 / lin1 nc{nc}: worst c needed", need)
    R.assert_within("lin0", out, ref0, abs0, 2.0 ** -8, C_BF16)
    R.assert_within("lin1", o1, ref1, abs1, 0.0, C_F32)
    assert torch.equal(out.cpu()[mask.cpu().bool()], b0.cpu().bfloat16()[None].expand(int(mask.sum()), nc))  # masked rows: b


# ------------------------------------------------------------------------------------- fp32 fused steps vs the oracle
_G64 = {}


def _split(flat, shapes):
    out, o = {}, 0
    for k, s in shapes.items():
        c = int(np.prod(s))
        out[k] = flat[o:o + c].view(s)
        o += c
    assert o == flat.numel()
    return out


def _fused_case(pkg, oracle, ei, npg, nb, nc, seed, use_graph=False, key=None, split=None, window=True):
    """Two native training steps against OracleTrainer, the first step's gradient per tensor against fp64, then the module's
    forward / backward and its inference launch.  Returns the measured errors."""
    lib = pkg._native.load()
    N = int(sum(npg))
    g = torch.Generator().manual_seed(seed)
    ys = [torch.randn(N, 1, generator=g) for _ in range(2)]
    masks = [torch.from_numpy(pkg.wdn_synth.generate_batch_mask(npg, 0.95, np.random.RandomState(seed + k))) for k in range(2)]
    model, p = build(pkg, oracle, nb, nc, seed=seed, fused=True)
    # the module first (initial parameters): forward / backward, and the inference launch equals the training forward
    xin = ys[0].clone()
    xin[masks[0]] = 0
    dx, dei, dm = xin.cuda(), ei.cuda(), masks[0].cuda()
    out = model(dx, dei)
    torch.nn.functional.mse_loss(out[dm], ys[0].cuda()[dm]).backward()
    with torch.no_grad():
        assert torch.equal(model(dx, dei), out.detach())
    leaves = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    o32 = oracle.gatres_forward(leaves, xin, ei, num_blocks=nb)
    torch.nn.functional.mse_loss(o32[masks[0]], ys[0][masks[0]]).backward()
    ref32 = {k: v.grad for k, v in leaves.items()}
    p64 = {k: v.double() for k, v in p.items()}

    def grads64(params64):
        lv = {k: v.clone().requires_grad_(True) for k, v in params64.items()}
        o = oracle.gatres_forward(lv, xin.double(), ei, num_blocks=nb)
        torch.nn.functional.mse_loss(o[masks[0]], ys[0].double()[masks[0]]).backward()
        return {k: v.grad for k, v in lv.items()}

    e_mod = relerr(out, o32)
    assert e_mod < 2e-5
    hip = {k: prm.grad for k, prm in zip(leaves, model.parameters())}
    key = key or (nb, nc, seed, N)
    m_rel, m_ratio, m_branch = check_gradients_vs_fp64(hip, ref32, grads64, p64, _G64, key)
    # the native step
    tr = pkg.GATResTrainer(model, dei, N, nodes_per_graph=npg, use_graph=use_graph)
    assert tr.fused and not tr.plan.flags & 4
    cus = int(lib.gatres_fused_cus_per_segment(model._cmodel_ref(), tr.plan.ref()))
    win = int(lib.gatres_fused_window_kernel(model._cmodel_ref(), tr.plan.ref()))
    if split is not None:
        assert cus == split
    if window:
        assert win == 1
    ref = oracle.OracleTrainer(p)
    errs = []
    for it in range(2):
        l_ref, o_ref = ref.step(ys[it].clone(), ys[it], ei, masks[it])
        loss = tr.step(ys[it].cuda(), ys[it].cuda(), masks[it].cuda())
        e_o, e_l = relerr(tr.out, o_ref), relerr(loss, l_ref)
        assert e_o < 2e-5 and e_l < 2e-5, (it, e_o, e_l)
        errs += [e_o, e_l]
        if it == 0:
            t_hip = _split(tr.grads.detach().cpu(), oracle.param_shapes(nb, nc))
            t_rel, t_ratio, t_branch = check_gradients_vs_fp64(t_hip, ref.grads(), grads64, p64, _G64, key)
    assert tr.fault_count == 0
    return dict(cus=cus, window=win, module_out=e_mod, module_grad=[m_rel, m_ratio, m_branch], steps_out_loss=errs,
                step_grad=[t_rel, t_ratio, t_branch])


@pytest.mark.parametrize("name,nc,use_graph", [("snap_sym", 32, False), ("snap_sym", 32, True), ("snap_dir_hub", 32, False),
                                               ("snap_sym", 16, False), ("snap_dir_hub", 8, False)])
def test_fused_window_kernel_on_irregular_graphs_vs_oracle(pkg, oracle, name, nc, use_graph):
    """The window kernel on plans without GATRES_GRAPH_DEG_LE6: at nc = 32 a symmetric plan takes the 0x1b16 instantiation
    ("a plan with hub rows"), a directed one the generic kernel; nc = 8 / 16 their own instantiations.  Batches of 3
    snapshots of 389 nodes (ragged tiles) with rows of 6 / 7 / 32 / 33+ entries."""
    g = IG.named(name)
    bs = 3
    ei = IG.collate(g, bs)
    r = _fused_case(pkg, oracle, ei, [g.num_nodes] * bs, 3, nc, seed=nc + len(name), use_graph=use_graph)
    assert (IG.row_counts(ei, g.num_nodes * bs)["gat_in"] > 6).any()
    note(f"irregular fused fp32 {name} nc{nc} graph={use_graph}: CUs / window kernel / errors", r)


@pytest.mark.parametrize("split", [1, 2, 4, 8])
def test_fused_split_on_irregular_graph_vs_oracle(pkg, oracle, split, monkeypatch):
    monkeypatch.setenv("GATRES_FUSED_SPLIT", str(split))
    g = IG.named("snap_sym")
    bs = 3
    # (2 parts of a 389-row snapshot: row windows too large for the window kernel's LDS -- the whole-segment kernel, split)
    r = _fused_case(pkg, oracle, IG.collate(g, bs), [g.num_nodes] * bs, 2, 32, seed=70, split=split, window=split >= 4,
                    key=("split", 2, 32, 70))
    note(f"irregular fused fp32 snap_sym nc32 split {split}: CUs / window kernel / errors", r)


def test_fused_fuzz_vs_oracle(pkg, oracle):
    """12 seeded random batches (tests/irregular_graphs.random_batch: directed / undirected extras, hubs, self loops,
    shuffled orders, ragged sizes) through whichever fused kernel the plan selects, each against the fp64 oracle."""
    rng = np.random.RandomState(2024)
    seen = []
    for case in range(12):
        nb, nc = int(rng.choice([1, 2, 3])), int(rng.choice([8, 16, 32, 32]))
        sizes = []
        while len(sizes) < 4:
            s = int(rng.choice([17, 33, 60, 120, 200, 388, 450]))
            if sum(sizes) + s > 1500:
                break
            sizes.append(s)
        ei = IG.random_batch(rng, sizes, pkg.wdn_synth.make_wdn_topology)
        r = _fused_case(pkg, oracle, ei, sizes, nb, nc, seed=500 + case, window=False, key=("fuzz", case))
        seen.append((nb, nc, len(sizes), r["cus"], r["window"], r["step_grad"][0]))
    note("irregular fused fp32 fuzz: (nb, nc, snapshots, CUs/segment, window kernel, worst grad err / |g|max)", seen)
    assert any(s[4] for s in seen) and any(s[3] > 1 for s in seen)


# ------------------------------------------------------------------------------------- bf16 whole model
@pytest.mark.parametrize("name", ["sym_hub", "sym_le32"])
def test_bf16_model_on_irregular_graph_vs_bf16_oracle(pkg, oracle, name, monkeypatch):
    """nb = 2, nc = 128 in bf16.  sym_hub: rows of more than 32 entries, the per-op kernels' hub path.  sym_le32: rows of
    7 .. 32 entries, with the blocked kernels (GATRES_BLOCKED=1) and without; the two must agree bit for bit."""
    nb, nc = 2, 128
    g = IG.named(name)
    n, ei = g.num_nodes, g.edge_index
    gen = torch.Generator().manual_seed(len(name))
    y = torch.randn(n, generator=gen)
    mask = torch.from_numpy(pkg.wdn_synth.generate_batch_mask([n], 0.95, np.random.RandomState(3)))
    xin = y.clone()
    xin[mask] = 0
    p = oracle.init_params(nb, nc, seed=8)
    lb = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    ob = oracle.gatres_forward_bf16(lb, xin[:, None], ei, num_blocks=nb)
    loss_b = torch.nn.functional.mse_loss(ob[mask], y[:, None][mask])
    loss_b.backward()
    g_b = torch.cat([v.grad.reshape(-1) for v in lb.values()])
    res = []
    for blocked in ((False, True) if name == "sym_le32" else (False,)):
        if blocked:
            monkeypatch.setenv("GATRES_BLOCKED", "1")
        else:
            monkeypatch.delenv("GATRES_BLOCKED", raising=False)
        model, _ = build(pkg, oracle, nb, nc, seed=8)
        model.set_compute_dtype("bf16")
        tr = pkg.GATResTrainer(model, ei.cuda(), n, nodes_per_graph=[n], use_graph=False, fused=False)
        assert not tr.plan.flags & 4 and bool(tr.plan.flags & 2) == (name == "sym_le32")
        assert bool(pkg._native.load().gatres_blocked_supported(model._cmodel_ref(), tr.plan.ref())) == blocked
        loss = tr.forward_backward(y.cuda(), y.cuda(), mask.cuda())
        torch.cuda.synchronize()
        f_l2 = float((tr.out.cpu().double() - ob.detach().reshape(-1).double()).norm() / ob.detach().double().norm())
        f_g2 = float((tr.grads.cpu().double() - g_b.double()).norm() / g_b.double().norm())
        f_loss = relerr(loss, loss_b)
        note(f"irregular bf16 2x128 {name} blocked={blocked}: predictions rel-L2, loss, flat gradient rel-L2 vs the "
             f"bf16-rounding oracle", [f_l2, f_loss, f_g2])
        assert f_l2 < 2e-3 and f_loss < 2e-3 and f_g2 < 1e-3, (f_l2, f_loss, f_g2)
        res.append((tr.out.clone(), tr.grads.clone()))
    if len(res) == 2:
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
