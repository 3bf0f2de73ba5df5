"""What the dense projection kernels of csrc/k_proj.hip must compute, in float64, and how far an output may lie from it.

Inputs are seeded normal rows (W scaled by K^-1/2); for bf16 storage the operands are rounded to bf16 first and the reference is
the float64 product of the ROUNDED operands.  Every output is held element by element, nothing is normalised by a maximum:

  u32 = 2^-24, ub = 2^-8, A = |X| |W|^T (the product of the operands' magnitudes)

  fp32 outputs     |got - ref| <= 2 K u32 A.  A rounded sum of K terms in any order stays within (K - 1) u32 A (each partial sum is
                   rounded once and is bounded by the sum of magnitudes); the factor 2 covers roundings inside the matrix-core
                   instruction that the ISA does not spell out.
  bf16 outputs     <= ub |ref| + 2 K u32 A: products of bf16 operands are exact in fp32, the fp32 accumulation is followed by ONE
                   rounding to bf16 (8 significand bits: half an ulp is at most 2^-8 |v|, reached at the bottom of a binade, so
                   the ub term is tight and what the accumulation adds to it falls under the doubled second term).
  dX               the same with K + 1 terms and A + |resid| where a residual is added; exactly 0.0 wherever relu_ref is not > 0,
                   both signed zeros included.
  logits           <= 2 (K + C) u32 sum_c A[n, hC + c] |att[hC + c]|: they are taken from the unrounded accumulators (no ub term).
  conv_param_grads the attention-vector / bias column sums, slab by slab like dW: one fused multiply-add per row and wave plus three
                   adds across the four waves, at most nps roundings of partial sums bounded by A_s; the same 2 nps u32 A_s.
  dW               slab by slab: slab s against the float64 product over its own rows within 2 nps u32 A_s, empty slabs exactly
                   zero, the float64 sum of the slabs against the whole product within the sum of the slabs' bounds.

The bounds come from the number formats, not from what the kernels were seen to give; tests/test_proj_turnover_host.py holds
torch's own CPU products to them and shows that they reject one dropped k step, one swapped pair of rows, one zeroed tile.
Every ``hold_*`` returns the worst ratio error / bound it saw (profiles/proj_turnover_margins.txt)."""
import torch

import proj_cases as PC

U32 = 2.0 ** -24
UB = 2.0 ** -8
TORCH_DTYPE = {"f32": torch.float32, "bf16": torch.bfloat16}


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def fwd_inputs(K, M, rows, dtype, seed):
    """X [rows, K], W [M, K] (scaled by K^-1/2) in the storage type, att_src / att_dst [M] in fp32."""
    g = _gen(seed)
    t = TORCH_DTYPE[dtype]
    return {"X": torch.randn(rows, K, generator=g).to(t), "W": (torch.randn(M, K, generator=g) / K ** 0.5).to(t),
            "att_src": torch.randn(M, generator=g), "att_dst": torch.randn(M, generator=g)}


def dx_inputs(K, M, rows, dtype, seed):
    """g_h [rows, K] (the reduction runs over its K columns), Wt [M, K], resid / relu_ref [rows, M] in the storage type."""
    g = _gen(seed)
    t = TORCH_DTYPE[dtype]
    return {"X": torch.randn(rows, K, generator=g).to(t), "W": (torch.randn(M, K, generator=g) / K ** 0.5).to(t),
            "resid": torch.randn(rows, M, generator=g).to(t), "relu_ref": torch.randn(rows, M, generator=g).to(t)}


def dw_inputs(HC, K, rows, dtype, seed):
    g = _gen(seed)
    t = TORCH_DTYPE[dtype]
    return {"G": torch.randn(rows, HC, generator=g).to(t), "X": torch.randn(rows, K, generator=g).to(t)}


def plant_zeros(relu_ref):
    """+0.0 / -0.0 into the rows and columns of tests/proj_cases.py (in place; ``relu_ref`` has exactly N rows)."""
    N, M = relu_ref.shape
    plus, minus = PC.zero_cols(M)
    for r in PC.zero_rows(N):
        relu_ref[r, plus] = 0.0
        relu_ref[r, minus] = -0.0
    return relu_ref


def with_guard_rows(t, N):
    """Rows [0, N) of ``t`` followed by GUARD_ROWS rows of NaN (allocated memory an unclamped row index would read)."""
    out = torch.full((N + PC.GUARD_ROWS, t.shape[1]), float("nan"), dtype=t.dtype, device=t.device)
    out[:N] = t[:N]
    return out


# ---- the reference ------------------------------------------------------------------------------------------------------------------
def product(X, W):
    """(X W^T, |X| |W|^T) in float64."""
    Xd, Wd = X.double(), W.double()
    return Xd @ Wd.t(), Xd.abs() @ Wd.abs().t()


def slab_products(G, X, N, S):
    """(G_s^T X_s, |G_s|^T |X_s|) in float64 for every slab s: [S, HC, K] each."""
    nps, _ = PC.slab_bounds(N, S)

    def padded(t):
        out = torch.zeros(S * nps, t.shape[1], dtype=torch.float64, device=t.device)
        out[:N] = t[:N].double()
        return out.view(S, nps, t.shape[1])
    Gp, Xp = padded(G), padded(X)
    return torch.bmm(Gp.transpose(1, 2), Xp), torch.bmm(Gp.abs().transpose(1, 2), Xp.abs())


# ---- the bounds ---------------------------------------------------------------------------------------------------------------------
def hold(got, ref, bound, what):
    """Every element of ``got`` within ``bound`` of ``ref`` (a NaN fails); returns the worst error / bound."""
    err = (got.double() - ref).abs()
    ok = err <= bound
    if not bool(ok.all()):
        bad = (~ok).nonzero()
        i = tuple(int(v) for v in bad[0])
        raise AssertionError(f"{what}: {bad.shape[0]} of {ok.numel()} outside the bound, first at {i}: got {float(got[i])!r}, "
                             f"reference {float(ref[i])!r}, error {float(err[i]):.3e} > bound {float(bound[i]):.3e}")
    pos = bound > 0
    return float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0


def hold_fwd(h, a_src, a_dst, X, W, att_src, att_dst, H, dtype, what=""):
    N, K = X.shape
    M = W.shape[0]
    C = M // H
    ref, A = product(X, W)
    bound = 2 * K * U32 * A
    if dtype == "bf16":
        bound = bound + UB * ref.abs()
    out = {"h": hold(h, ref, bound, what + " h")}
    for name, got, att in (("a_src", a_src, att_src), ("a_dst", a_dst, att_dst)):
        attd = att.double().view(1, H, C)
        ref_a = (ref.view(N, H, C) * attd).sum(-1)
        bound_a = 2 * (K + C) * U32 * (A.view(N, H, C) * attd.abs()).sum(-1)
        out[name] = hold(got, ref_a, bound_a, what + " " + name)
    return out


def dx_reference(X, W, resid, relu_ref, dtype):
    """(reference, bound, keep): ``keep`` marks the outputs that are not masked (None: no mask)."""
    K = X.shape[1]
    ref, A = product(X, W)
    terms = K
    if resid is not None:
        ref, A, terms = ref + resid.double(), A + resid.double().abs(), K + 1
    bound = 2 * terms * U32 * A
    if dtype == "bf16":
        bound = bound + UB * ref.abs()
    keep = None
    if relu_ref is not None:
        keep = relu_ref > 0                                # false for +0.0, -0.0 and everything below
        ref, bound = ref * keep, bound * keep              # exactly 0.0 where masked
    return ref, bound, keep


def hold_dx(g_x, X, W, resid, relu_ref, dtype, what=""):
    ref, bound, keep = dx_reference(X, W, resid, relu_ref, dtype)
    if keep is not None:
        masked = g_x[~keep]
        assert bool((masked == 0).all()), f"{what} g_x: {int((masked != 0).sum())} masked outputs are not exactly 0.0"
    return {"g_x": hold(g_x, ref, bound, what + " g_x")}


def hold_dw(slabs, G, X, N, S, what=""):
    """``slabs`` [S, HC * K + SLAB_PAD] as the kernel left it, pre-filled with NaN."""
    HC, K = G.shape[1], X.shape[1]
    nps, rows = PC.slab_bounds(N, S)
    assert slabs.shape == (S, HC * K + PC.SLAB_PAD)
    assert bool(torch.isnan(slabs[:, HC * K:]).all()), f"{what}: the pad words behind a slab's matrix were written"
    got = slabs[:, :HC * K].reshape(S, HC, K)
    unwritten = torch.isnan(got).reshape(S, -1).any(1)
    assert not bool(unwritten.any()), f"{what}: slabs {unwritten.nonzero().flatten().tolist()} keep NaN from before the launch"
    ref, A = slab_products(G, X, N, S)
    bound = 2 * nps * U32 * A
    empty = [s for s, (beg, end) in enumerate(rows) if beg >= end]
    if empty:
        assert bool((got[empty] == 0).all()), f"{what}: an empty slab is not exactly zero"
    return {"slab": hold(got, ref, bound, what + " slab"),
            "sum": hold(got.double().sum(0), ref.sum(0), bound.sum(0), what + " sum of slabs")}


def conv_grad_inputs(H, C, rows, dtype, seed):
    g = _gen(seed)
    t = TORCH_DTYPE[dtype]
    return {"h": torch.randn(rows, H * C, generator=g).to(t), "g_out": torch.randn(rows, H * C, generator=g).to(t),
            "g_a_src": torch.randn(rows, H, generator=g), "g_a_dst": torch.randn(rows, H, generator=g)}


def hold_conv_grads(slabs, h, g_a_src, g_a_dst, g_out, N, S, H, what=""):
    """``slabs`` [S, 3 HC + SLAB_PAD] pre-filled with NaN: per slab the att_src, att_dst and bias partial sums, HC columns each."""
    HC = h.shape[1]
    C = HC // H
    nps, rows = PC.slab_bounds(N, S)
    assert slabs.shape == (S, 3 * HC + PC.SLAB_PAD)
    assert bool(torch.isnan(slabs[:, 3 * HC:]).all()), f"{what}: the pad words behind a slab's sums were written"
    assert not bool(torch.isnan(slabs[:, :3 * HC]).any()), f"{what}: a slab keeps NaN from before the launch"

    def sums(t):                                   # per-slab column sums of the rows' terms and of their magnitudes
        out = torch.zeros(S * nps, HC, dtype=torch.float64, device=t.device)
        out[:N] = t[:N]
        out = out.view(S, nps, HC)
        return out.sum(1), out.abs().sum(1)
    hd = h.double()
    terms = (g_a_src.double().repeat_interleave(C, dim=1) * hd, g_a_dst.double().repeat_interleave(C, dim=1) * hd, g_out.double())
    empty = [s for s, (beg, end) in enumerate(rows) if beg >= end]
    out = {}
    for k, name in enumerate(("att_src", "att_dst", "bias")):
        got = slabs[:, k * HC:(k + 1) * HC]
        ref, A = sums(terms[k])
        if empty:
            assert bool((got[empty] == 0).all()), f"{what}: an empty slab is not exactly zero"
        out[name] = hold(got, ref, 2 * nps * U32 * A, f"{what} {name} slab")
        out[name + " sum"] = hold(got.double().sum(0), ref.sum(0), 2 * nps * U32 * A.sum(0), f"{what} {name} sum of slabs")
    return out


def noisy(ref, A, dtype, seed):
    """The float64 reference plus fp32-level noise (uniform in +-u32 A), rounded to the storage type: a right answer."""
    g = _gen(seed)
    noise = (torch.rand(ref.shape, generator=g, dtype=torch.float64) * 2 - 1) * U32 * A
    return (ref + noise).float().to(TORCH_DTYPE[dtype])
