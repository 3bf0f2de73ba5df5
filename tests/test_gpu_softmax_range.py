"""GATConv's attention softmax at large and saturated logits against fp64.

alpha_e = exp(s_e - m) / (sum_k exp(s_k - m) + 1e-16) does not depend on m in exact arithmetic, and in fp32 it does not
either while every s_e - m stays within about +-80: a softmax maximum that is wrong but uniform across the row passes every
unit-scale test.  Here the rows spread by 100 and more (tests/logit_rows.py: dominant, all-negative, tied, saturated and
spread rows, the argmax at every slot of the slot paths and in every slot column of the hub path), so a wrong m overflows
exp (NaN), underflows the whole row (alpha 0) or moves alpha by e^(gap).

  * per-op kernels, fp32 and bf16, C in {8, 32, 64, 128}, H in {1, 2}, 4 and 8 features per lane, on the irregular graphs
    (rows of 6 / 7 / 32 / 33+ entries, hubs in ragged last waves) and the star / hub graphs of test_gpu_ops.py;
  * the blocked bf16 kernels (nc = 128) against the per-op pair, bit for bit;
  * whole models at inputs x 100 (the reference's --norm_type unused) with attention vectors x 5, the regime proven by
    oracle.logit_regime: the window kernel (training and inference instantiations, split segments, run-time phases), the
    per-op path and the bf16 gatres_large path."""
import functools

import numpy as np
import pytest
import torch

import irregular_graphs as IG
import logit_rows as LR
import sparse_refs as R
from test_gpu_model import check_gradients_vs_fp64, judge_gradients, load_params, note, relerr   # noqa: E402

pytestmark = pytest.mark.gpu

FP32, BF16 = 0, 1
EPS32 = 2.0 ** -23
FLT_MIN = 2.0 ** -126
# alpha_e = exp(s_e - m) / Z.  In fp32 a logit of magnitude |s| carries an error of ~eps32 |s| (the LeakyReLU product, the
# slope 0.2f against 0.2, the subtraction s - m), and alpha_e moves relatively by its own (s_e - m) error plus the
# alpha-weighted mean of the row's: |d alpha_e| <~ alpha_e (2 eps32 L + a few ulps of exp / sum / divide), where L is the
# largest |s| over the row's edges that carry weight (s >= m - 104) -- the maximum included.  The bound used is
#     |alpha - alpha64| <= C_SOFT alpha64 (1 + L) + FLT_MIN           (FLT_MIN: exp results that fall to denormals)
#     |out - out64|     <= 2^-8 |out64| (bf16 stores) + C_SOFT (1 + L) out_abs64
# with out_abs the aggregation on |h| (+ |bias|), the same judge as sparse_refs.assert_within.  C_SOFT = 8 eps32.
C_SOFT = 8 * EPS32
C_F32 = 4.3e-7                 # the backward's bounds of test_gpu_irregular.py (alpha enters the backward as an input)
C_BF16 = 9e-8
GRAPHS = ("sym_le32", "dir_le32", "sym_hub", "dir_hub_shuffled", "ops_hub", "ops_star")


def _st():
    import gnn_pressure_estimation_amd as G
    return G._native.current_stream(torch.device("cuda"))


@functools.lru_cache(maxsize=None)
def rows_case(name, H):
    """(Rows, Families, src, dst, per-edge and per-row logit scale L) of a graph's variants (cached: CPU work)."""
    ei, n = LR.graph(name)
    rows = LR.build(ei, n, H, seed=len(name))
    F = LR.families_of(rows)
    src, dst = R.gat_edges(rows.edge_index, rows.num_nodes)
    s, _, rowptr = LR.csr(rows.edge_index, rows.num_nodes)
    assert np.array_equal(s, src.numpy())
    lg = LR.logits(src.numpy(), dst.numpy(), rows.a_src, rows.a_dst)
    L = LR.weighted_scale(lg, dst.numpy(), rows.num_nodes)                     # [N, H]
    return rows, F, src, dst, rowptr, torch.from_numpy(L)


def _judge_alpha(what, alpha, al_ref, L_edge):
    R.assert_within(what, alpha, al_ref, al_ref * (1 + L_edge) + FLT_MIN / C_SOFT, 0.0, C_SOFT)
    return R.excess(alpha, al_ref, al_ref * (1 + L_edge) + FLT_MIN / C_SOFT, 0.0)


def _exact_checks(what, rows, F, src, alpha, out, h, bias, H, C, fp32_out):
    """tied / saturated rows: alpha exactly 0.5 / 1 and 0; fp32 outputs fl(fl(0.5 h1 + 0.5 h2) + bias) / fl(h + bias), ReLU."""
    al = alpha.cpu().double().numpy()
    for fam in ("tied", "saturated"):
        want = LR.exact_rows(rows, F, fam)
        sel = ~np.isnan(want)                   # (tests/test_logit_rows.py: which graphs hold which families)
        bad = al[sel] != want[sel]
        assert not bad.any(), f"{what}: {fam} rows, {int(bad.sum())} of {int(sel.sum())} alphas not exact"
        if not fp32_out:
            continue
        hc, oc, bc = h.cpu().float().view(-1, H, C), out.cpu().float().view(-1, H, C), bias.cpu().float().view(H, C)
        _, _, rowptr = LR.csr(rows.edge_index, rows.num_nodes)
        for i, hd in zip(*np.nonzero(F.fam[fam])):
            b, e = rowptr[i], rowptr[i + 1]
            top = [src[k].item() for k in range(b, e) if want[k, hd] > 0]
            if fam == "tied":
                exp = (0.5 * hc[top[0], hd] + 0.5 * hc[top[1], hd]) + bc[hd]
            else:
                exp = hc[top[0], hd] + bc[hd]
            assert torch.equal(oc[i, hd], exp.relu()), f"{what}: {fam} row {i} head {hd}"


@pytest.mark.parametrize("H", [1, 2])
@pytest.mark.parametrize("C", [8, 32, 64, 128])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", GRAPHS)
def test_aggregate_softmax_at_large_logits_vs_fp64(pkg, lib, name, dtype, C, H, monkeypatch):
    """gatres_t_gat_aggregate_fwd / _bwd_dst / _bwd_src on rows placed by tests/logit_rows.py (16 variants of the graph in
    one launch), with 4 and 8 features per lane: alpha and the outputs against tests/sparse_refs.py within the logit-scaled
    bound above, the exact families bit for bit, the backward (alpha and g_e given) within test_gpu_irregular.py's bounds
    plus FLT_MIN (an alpha below FLT_MIN makes its edge's g_e a denormal) and g_e exactly 0 on every zero-alpha edge of a
    saturated row."""
    chk = pkg._native.check
    rows, F, src, dst, rowptr, L = rows_case(name, H)
    n, HC, DT = rows.num_nodes, H * C, {"fp32": FP32, "bf16": BF16}[dtype]
    plan = pkg.GraphPlan(rows.edge_index.cuda(), n, device="cuda", reorder=False, segments=False)
    Eg, gp = plan.num_edges_gat, plan.ref()
    assert Eg == len(src)
    gen = torch.Generator().manual_seed(C * 10 + H + len(name))
    rn = lambda *s: torch.randn(*s, generator=gen)
    tdt = torch.float32 if dtype == "fp32" else torch.bfloat16
    h, bias, g_out = rn(n, HC).to(tdt).cuda(), rn(HC).cuda(), rn(n, HC).to(tdt).cuda()
    att_s, att_d = rn(HC).cuda(), rn(HC).cuda()
    a_s, a_d = rows.a_src.cuda(), rows.a_dst.cuda()
    out_ref, out_abs, al_ref = R.gat_aggregate_fwd(src, dst, h.cpu(), rows.a_src, rows.a_dst, bias.cpu(), n, H, True)
    L_edge = L[dst]
    L_out = (1 + L).repeat_interleave(C, dim=1)
    alpha_in = al_ref.float()
    ge_ref, ge_abs, gad_ref, gad_abs = R.gat_aggregate_bwd_dst(src, dst, g_out.cpu(), h.cpu(), alpha_in, rows.a_src,
                                                               rows.a_dst, n, H)
    ge_in, gad_in = ge_ref.float(), gad_ref.float()
    gh_ref, gh_abs, gas_ref, gas_abs = R.gat_aggregate_bwd_src(src, dst, g_out.cpu(), alpha_in, ge_in, gad_in, att_s.cpu(),
                                                               att_d.cpu(), n, H)
    rel = 0.0 if dtype == "fp32" else 2.0 ** -8
    sat = ~np.isnan(LR.exact_rows(rows, F, "saturated"))
    sat_zero = torch.from_numpy(sat & (alpha_in.numpy() == 0))
    need = {}
    for lf in ("4", "8"):
        monkeypatch.setenv("GATRES_AGG_LANE_FEATURES", lf)
        out = torch.full((n, HC), float("nan"), device="cuda").to(tdt)
        alpha = torch.full((Eg, H), float("nan"), device="cuda")
        chk(lib.gatres_t_gat_aggregate_fwd(gp, h.data_ptr(), a_s.data_ptr(), a_d.data_ptr(), bias.data_ptr(), out.data_ptr(),
                                           alpha.data_ptr(), H, C, 1, DT, _st()), "agg fwd")
        ai = alpha_in.cuda()
        g_e, g_ad = torch.full((Eg, H), float("nan"), device="cuda"), torch.full((n, H), float("nan"), device="cuda")
        chk(lib.gatres_t_gat_aggregate_bwd_dst(gp, g_out.data_ptr(), h.data_ptr(), ai.data_ptr(), a_s.data_ptr(),
                                               a_d.data_ptr(), g_e.data_ptr(), g_ad.data_ptr(), H, C, DT, _st()), "bwd dst")
        gei, gadi = ge_in.cuda(), gad_in.cuda()
        g_h = torch.full((n, HC), float("nan"), device="cuda").to(tdt)
        g_as = torch.full((n, H), float("nan"), device="cuda")
        chk(lib.gatres_t_gat_aggregate_bwd_src(gp, g_out.data_ptr(), ai.data_ptr(), gei.data_ptr(), gadi.data_ptr(),
                                               att_s.data_ptr(), att_d.data_ptr(), g_h.data_ptr(), g_as.data_ptr(), H, C, DT,
                                               _st()), "bwd src")
        torch.cuda.synchronize()
        what = f"{name} {dtype} H{H} C{C} lane features {lf}"
        assert torch.isfinite(alpha).all() and torch.isfinite(out.float()).all(), what
        need["alpha"] = max(need.get("alpha", 0.0), _judge_alpha(f"{what}: alpha", alpha, al_ref, L_edge))
        R.assert_within(f"{what}: out", out, out_ref, out_abs * L_out, rel, C_SOFT)
        need["out"] = max(need.get("out", 0.0), R.excess(out, out_ref, out_abs * L_out, rel))
        _exact_checks(what, rows, F, src, alpha, out, h, bias, H, C, dtype == "fp32")
        for k, got, ref, ref_abs, r, c in (("g_e", g_e, ge_ref, ge_abs, 0.0, C_F32), ("g_a_dst", g_ad, gad_ref, gad_abs, 0.0, C_F32),
                                           ("g_h", g_h, gh_ref, gh_abs, rel, C_BF16 if rel else C_F32),
                                           ("g_a_src", g_as, gas_ref, gas_abs, 0.0, C_F32)):
            ref_abs = ref_abs + FLT_MIN / c                  # (alphas below FLT_MIN give denormal g_e: absolute noise)
            R.assert_within(f"{what}: {k}", got, ref, ref_abs, r, c)
            need[k] = max(need.get(k, 0.0), R.excess(got, ref, ref_abs, r))
        assert not g_e.cpu()[sat_zero].any(), f"{what}: g_e on the saturated rows' zero-alpha edges"
    note(f"softmax range {name} {dtype} H{H} C{C}: worst c needed (bounds: alpha / out C_SOFT {C_SOFT:.2g} x (1 + L), "
         f"backward C_F32 {C_F32:.2g} / C_BF16 {C_BF16:.2g})", need)


@pytest.mark.parametrize("name", ["sym_le32", "dir_le32"])
def test_blocked_aggregation_at_large_logits_equals_the_per_op_kernel(pkg, lib, name):
    """gatres_bf16_agg_proj_fwd (nc = 128, H = 2, DEG_LE32 plans) against gatres_t_gat_aggregate_fwd + _proj_attn_fwd on the
    large-logit rows: o1, alpha and the projected rows bit for bit, the exact families exact."""
    nc, H = 128, 2
    chk = pkg._native.check
    rows, F, src, dst, rowptr, L = rows_case(name, H)
    N = rows.num_nodes
    plan = pkg.GraphPlan(rows.edge_index.cuda(), N, device="cuda", segments=False)
    assert plan.flags & 2
    Eg, gp = plan.num_edges_gat, plan.ref()
    g = torch.Generator().manual_seed(11)
    rn = lambda *s: torch.randn(*s, generator=g).cuda()
    h1, bias = rn(N, 256).bfloat16(), rn(256)
    a_s, a_d = rows.a_src.cuda(), rows.a_dst.cuda()
    W2 = (rn(128, 256) / 16).bfloat16()
    att_s, att_d = rn(128), rn(128)
    o_a, al_a = torch.empty(N, 256, dtype=torch.bfloat16, device="cuda"), torch.zeros(Eg, 2, device="cuda")
    h2_a, as_a, ad_a = torch.empty(N, 128, dtype=torch.bfloat16, device="cuda"), torch.empty(N, device="cuda"), torch.empty(N, device="cuda")
    chk(lib.gatres_t_gat_aggregate_fwd(gp, h1.data_ptr(), a_s.data_ptr(), a_d.data_ptr(), bias.data_ptr(), o_a.data_ptr(),
                                       al_a.data_ptr(), 2, nc, 1, BF16, _st()), "agg")
    chk(lib.gatres_t_proj_attn_fwd(o_a.data_ptr(), W2.data_ptr(), att_s.data_ptr(), att_d.data_ptr(), h2_a.data_ptr(),
                                   as_a.data_ptr(), ad_a.data_ptr(), N, 256, 1, nc, BF16, _st()), "proj")
    o_b, al_b = torch.zeros_like(o_a), torch.zeros_like(al_a)
    h2_b, as_b, ad_b = torch.zeros_like(h2_a), torch.zeros_like(as_a), torch.zeros_like(ad_a)
    chk(lib.gatres_bf16_agg_proj_fwd(gp, h1.data_ptr(), a_s.data_ptr(), a_d.data_ptr(), bias.data_ptr(), o_b.data_ptr(),
                                     al_b.data_ptr(), W2.data_ptr(), att_s.data_ptr(), att_d.data_ptr(), h2_b.data_ptr(),
                                     as_b.data_ptr(), ad_b.data_ptr(), nc, _st()), "agg_proj")
    torch.cuda.synchronize()
    assert torch.equal(o_a, o_b) and torch.equal(al_a, al_b)
    assert torch.equal(h2_a, h2_b) and torch.equal(as_a, as_b) and torch.equal(ad_a, ad_b)
    ref, ref_abs, al_ref = R.gat_aggregate_fwd(src, dst, h1.cpu(), rows.a_src, rows.a_dst, bias.cpu(), N, 2, True)
    c_al = _judge_alpha(f"blocked {name}: alpha", al_b, al_ref, L[dst])
    L_out = (1 + L).repeat_interleave(nc, dim=1)
    R.assert_within(f"blocked {name}: o1", o_b, ref, ref_abs * L_out, 2.0 ** -8, C_SOFT)
    _exact_checks(f"blocked {name}", rows, F, src, al_b, o_b, h1, bias, H, nc, False)
    note(f"softmax range blocked bf16 {name}: worst c needed (alpha, o1)", [c_al, R.excess(o_b, ref, ref_abs * L_out, 2.0 ** -8)])


# ------------------------------------------------------------------------------------- whole models at inputs x 100
SCALE, KAPPA = 100.0, 5.0
SEED16, SEED8 = 22, 30           # (seeds whose fp64 forward reaches the regime _regime asserts)
_G64 = {}


def _scaled_params(oracle, nb, nc, seed):
    p = oracle.init_params(nb, nc, seed=seed)
    return {k: (v * KAPPA if ".att_" in k else v) for k, v in p.items()}


def _batch(pkg, name, bs, seed):
    g = IG.named(name)
    ei = IG.collate(g, bs)
    npg = [g.num_nodes] * bs
    N = g.num_nodes * bs
    y = torch.randn(N, 1, generator=torch.Generator().manual_seed(seed)) * SCALE
    mask = torch.from_numpy(pkg.wdn_synth.generate_batch_mask(npg, 0.95, np.random.RandomState(seed)))
    xin = y.clone()
    xin[mask] = 0
    return ei, npg, N, y, mask, xin


def _regime(oracle, p, xin, ei, nb, what):
    """The fp64 forward's logits must reach the regime: in every conv some rows have a top-two gap above 90 (at least 1 % of
    them, in the first conv 5 %), the largest gap exceeds 100, and some rows of the model have every logit below -90."""
    f = oracle.logit_regime(p, xin, ei, num_blocks=nb)
    note(f"softmax range regime {what}: per conv (max top-two gap, share of rows above 90, rows with max < -90, max |s|)",
         [[round(d["max_gap"], 1), round(d["share_above"], 4), d["neg_max_rows"], round(d["max_abs"], 1)] for d in f])
    assert all(d["max_gap"] > 100 and d["share_above"] > 0.01 for d in f), f
    assert f[0]["share_above"] > 0.05, f
    assert sum(d["neg_max_rows"] for d in f) > 0, f
    return f


def _model_case(pkg, oracle, name, nb, nc, seed, fused, bs=3, step=True, key=None):
    """Module forward / backward (+ the inference forward) and one native training step at inputs x 100 against the fp32
    and fp64 oracles: predictions, loss and gradients judged by their error against fp64 next to the fp32 oracle's own
    (test_gpu_model.judge_gradients / check_gradients_vs_fp64), the parameters after one Adam step within 1e-6 of that
    step taken in fp64 from the native gradient."""
    ei, npg, N, y, mask, xin = _batch(pkg, name, bs, seed)
    p = _scaled_params(oracle, nb, nc, seed)
    p0 = oracle.flatten(p).double()
    _regime(oracle, p, xin, ei, nb, f"{name} {nb}x{nc}")
    model = pkg.GATResMeanConv(num_blocks=nb, nc=nc, fused=fused)
    load_params(model, p)
    model = model.cuda()
    dx, dei, dm = xin.cuda(), ei.cuda(), mask.cuda()
    out = model(dx, dei)
    loss = torch.nn.functional.mse_loss(out[dm], y.cuda()[dm])
    loss.backward()
    with torch.no_grad():
        out_inf = model(dx, dei)
    assert torch.equal(out_inf, out.detach())                                     # the inference instantiation
    leaves = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    o32 = oracle.gatres_forward(leaves, xin, ei, num_blocks=nb)
    l32 = torch.nn.functional.mse_loss(o32[mask], y[mask])
    l32.backward()
    ref32 = {k: v.grad for k, v in leaves.items()}
    p64 = {k: v.double() for k, v in p.items()}
    with torch.no_grad():
        o64 = oracle.gatres_forward(p64, xin.double(), ei, num_blocks=nb)
    l64 = torch.nn.functional.mse_loss(o64[mask], y.double()[mask])
    bad, e_out, r_out, _ = judge_gradients({"out": out.detach(), "loss": loss.detach().reshape(1)},
                                           {"out": o32.detach(), "loss": l32.detach().reshape(1)},
                                           {"out": o64, "loss": l64.reshape(1)})
    assert not bad, bad
    assert torch.isfinite(out).all()

    def grads64(params64):
        lv = {k: v.clone().requires_grad_(True) for k, v in params64.items()}
        o = oracle.gatres_forward(lv, xin.double(), ei, num_blocks=nb)
        torch.nn.functional.mse_loss(o[mask], y.double()[mask]).backward()
        return {k: v.grad for k, v in lv.items()}

    key = key or (name, nb, nc, seed)
    hip = {k: prm.grad for k, prm in zip(leaves, model.parameters())}
    g_rel, g_ratio, g_branch = check_gradients_vs_fp64(hip, ref32, grads64, p64, _G64, key)
    res = dict(out_vs_fp64=e_out, out_ratio_to_fp32_oracle=r_out, grad=[g_rel, g_ratio, g_branch])
    if step:
        model.zero_grad()
        tr = pkg.GATResTrainer(model, dei, N, nodes_per_graph=npg, use_graph=False)
        ref = oracle.OracleTrainer(p)
        l_ref, o_ref = ref.step(y.clone(), y, ei, mask)
        l_hip = tr.step(y.cuda(), y.cuda(), dm)
        torch.cuda.synchronize()
        bad, e_step, _, _ = judge_gradients({"out": tr.out.detach().reshape(-1), "loss": l_hip.detach().reshape(1)},
                                            {"out": o_ref.detach().reshape(-1), "loss": l_ref.detach().reshape(1)},
                                            {"out": o64.reshape(-1), "loss": l64.reshape(1)})
        assert not bad, bad
        shapes = oracle.param_shapes(nb, nc)
        flat, o = tr.grads.detach().cpu(), 0
        t_hip = {}
        for k, s in shapes.items():
            c = int(np.prod(s))
            t_hip[k] = flat[o:o + c].view(s)
            o += c
        t_rel, t_ratio, t_branch = check_gradients_vs_fp64(t_hip, ref.grads(), grads64, p64, _G64, key)
        # Adam's first step moves each parameter by lr g / (|g| + eps) (g with the weight decay folded in): where a gradient
        # is cancellation noise (att_dst, judged above against the fp32 oracle's own noise) so is that step, for the oracle
        # too -- so the parameters are held to the step the native gradient makes, in fp64, and the gradient to fp64 above
        g = flat.double() + 6e-6 * p0
        e_par = relerr(model.flat_parameters, p0 - 5e-4 * g / (g.abs() + 1e-8))
        assert e_par < 1e-6, e_par
        assert tr.fault_count == 0
        res.update(step_out_vs_fp64=e_step, step_grad=[t_rel, t_ratio, t_branch], params_after_adam=e_par,
                   fused=bool(tr.fused))
        if fused:
            lib = pkg._native.load()
            res["window"] = int(lib.gatres_fused_window_kernel(model._cmodel_ref(), tr.plan.ref()))
            res["cus"] = int(lib.gatres_fused_cus_per_segment(model._cmodel_ref(), tr.plan.ref()))
    return res


@pytest.mark.parametrize("name,nc,seed", [("snap_sym", 32, 21), ("snap_dir_hub", 32, 21), ("snap_sym", 16, SEED16),
                                           ("snap_dir_hub", 8, SEED8)])
def test_window_kernel_at_large_logits_vs_fp64(pkg, oracle, name, nc, seed):
    """The window kernel on C-Town-sized snapshots: at gatres_small width (nc = 32) the symmetric hub-row instantiation and
    the generic one (softmax fused with the gather: win_fwd_agg), at nc = 16 / 8 their own instantiations (the separate
    slot softmax, win_softmax); training and inference launches, one native step."""
    r = _model_case(pkg, oracle, name, 2, nc, seed=seed, fused=True)
    assert r["fused"] and r["window"] == 1
    note(f"softmax range window kernel {name} 2x{nc} inputs x{SCALE:g} att x{KAPPA:g}", r)


@pytest.mark.parametrize("split", [1, 2, 4, 8])
def test_fused_split_at_large_logits_vs_fp64(pkg, oracle, split, monkeypatch):
    monkeypatch.setenv("GATRES_FUSED_SPLIT", str(split))
    r = _model_case(pkg, oracle, "snap_sym", 2, 32, seed=21, fused=True, key=("split", 21))
    assert r["fused"] and r["cus"] == split and (r["window"] == 1) == (split >= 4)
    note(f"softmax range fused split {split} snap_sym 2x32", r)


def test_window_runtime_phases_at_large_logits_bit_identical(pkg, oracle, monkeypatch):
    """GATRES_WINDOW_RUNTIME_PHASES=1 (phases read at run time) against the instantiated kernels: the same bits."""
    ei, npg, N, y, mask, xin = _batch(pkg, "snap_sym", 3, 21)
    p = _scaled_params(oracle, 2, 32, 21)
    _regime(oracle, p, xin, ei, 2, "snap_sym 2x32 runtime phases")
    res = []
    for v in ("0", "1"):
        monkeypatch.setenv("GATRES_WINDOW_RUNTIME_PHASES", v)
        model = pkg.GATResMeanConv(num_blocks=2, nc=32, fused=True)
        load_params(model, p)
        model = model.cuda()
        out = model(xin.cuda(), ei.cuda())
        torch.nn.functional.mse_loss(out[mask.cuda()], y.cuda()[mask.cuda()]).backward()
        with torch.no_grad():
            inf = model(xin.cuda(), ei.cuda())
        tr = pkg.GATResTrainer(model, ei.cuda(), N, nodes_per_graph=npg, use_graph=False)
        assert int(pkg._native.load().gatres_fused_window_kernel(model._cmodel_ref(), tr.plan.ref())) == 1
        grads = torch.cat([q.grad.reshape(-1) for q in model.parameters()]).clone()
        model.zero_grad()
        loss = tr.step(y.cuda(), y.cuda(), mask.cuda())
        torch.cuda.synchronize()
        res.append((out.detach(), inf, grads, tr.out.clone(), loss.clone(), tr.grads.clone(), model.flat_parameters.clone()))
    for a, b in zip(*res):
        assert torch.isfinite(a).all() and torch.equal(a, b)


def test_per_op_model_at_large_logits_vs_fp64(pkg, oracle):
    r = _model_case(pkg, oracle, "snap_dir_hub", 2, 32, seed=21, fused=False, step=False)
    note("softmax range per-op model snap_dir_hub 2x32", r)


def test_bf16_large_model_at_large_logits_vs_bf16_oracle(pkg, oracle):
    """gatres_large width (nc = 128, bf16 storage) on one snapshot at inputs x 100 against the bf16-rounding oracle:
    predictions and loss at the shallow-model bound of test_gpu_bf16.py (2e-3).  The gradient is judged against the
    conditioning of this regime: here one bf16 rounding of an activation moves the gradient by ~20x what it does at unit
    scale (the bf16 oracle itself is 1 - 20 % off the fp64 gradient per tensor, against ~0.1 % at unit scale), so the kernels'
    fp32 sums landing on the other side of a bf16 rounding boundary than the oracle's show as ~1 bf16 ulp of rel-L2 (measured
    5e-3, parity report).  A rounding point that differs from the oracle's would put the kernels as far from the oracle as
    the oracle is from fp64: the flat gradient must stay within a fifth of that distance, and every tensor no further from
    fp64 than twice the bf16 oracle."""
    nb, nc = 2, 128
    ei, npg, N, y, mask, xin = _batch(pkg, "snap_sym", 1, 21)
    p = _scaled_params(oracle, nb, nc, 21)
    _regime(oracle, p, xin, ei, nb, "snap_sym 2x128")
    lb = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    ob = oracle.gatres_forward_bf16(lb, xin, ei, num_blocks=nb)
    loss_b = torch.nn.functional.mse_loss(ob[mask], y[mask])
    loss_b.backward()
    g_b = torch.cat([v.grad.reshape(-1) for v in lb.values()]).double()
    l64 = {k: v.double().clone().requires_grad_(True) for k, v in p.items()}
    o64 = oracle.gatres_forward(l64, xin.double(), ei, num_blocks=nb)
    torch.nn.functional.mse_loss(o64[mask], y.double()[mask]).backward()
    model = pkg.GATResMeanConv(num_blocks=nb, nc=nc)
    load_params(model, p)
    model = model.cuda()
    model.set_compute_dtype("bf16")
    tr = pkg.GATResTrainer(model, ei.cuda(), N, nodes_per_graph=npg, use_graph=False, fused=False)
    loss = tr.forward_backward(y.reshape(-1).cuda(), y.reshape(-1).cuda(), mask.reshape(-1).cuda())
    torch.cuda.synchronize()
    assert torch.isfinite(tr.out).all() and torch.isfinite(tr.grads).all()
    f_l2 = float((tr.out.cpu().double() - ob.detach().reshape(-1).double()).norm() / ob.detach().double().norm())
    f_loss = relerr(loss, loss_b)
    g_h = tr.grads.cpu().double()
    g_64 = torch.cat([v.grad.reshape(-1) for v in l64.values()])
    f_g2, b_g2 = float((g_h - g_b).norm() / g_64.norm()), float((g_b - g_64).norm() / g_64.norm())
    per, o = {}, 0
    for k, v in l64.items():
        c = v.numel()
        n64 = float(v.grad.norm())
        per[k] = (float((g_h[o:o + c] - v.grad.reshape(-1)).norm()) / n64, float((g_b[o:o + c] - v.grad.reshape(-1)).norm()) / n64)
        o += c
    note("softmax range bf16 2x128 snap_sym: predictions rel-L2, loss vs the bf16-rounding oracle; flat gradient rel-L2 "
         "kernels vs bf16 oracle, bf16 oracle vs fp64; per tensor (kernels vs fp64, bf16 oracle vs fp64)",
         [f_l2, f_loss, f_g2, b_g2, per])
    assert f_l2 < 2e-3 and f_loss < 2e-3, (f_l2, f_loss)
    assert f_g2 < 0.2 * b_g2, (f_g2, b_g2)
    assert all(a <= 2 * b for a, b in per.values()), per
