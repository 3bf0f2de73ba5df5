"""What the small per-op kernels of csrc/k_misc.hip must compute, and how far an output may lie from it.

Seeded inputs, the references and the bounds of tests/test_gpu_misc_turnover.py (tests/misc_cases.py says at which sizes).  Where
a kernel's arithmetic is one rounded operation per element the reference is that operation in fp32 and the comparison is bit for
bit; where it is a sum the reference is the float64 sum and the bound comes from the formats (u32 = 2^-24):

  lin0 forward      bit for bit fp32(fp32(xm * w) + b) -- the library is built with -ffp-contract=off --, rounded to nearest-even for
                    bf16 storage; xm = 0 on a masked node whatever x holds there.
  lin1 forward      |got - ref| <= nc u32 sum_c |x_c w_c| + u32 |ref| per row: a rounded sum of nc terms in any order stays within
                    (nc - 1) u32 of the sum of magnitudes (fewer roundings still with fused multiply-adds), the second term is the
                    bias add.  bf16 rows widen exactly: the reference is the float64 dot product of the rounded operands.
  lin0 / lin1 slabs slab s against the float64 sum over its own rows within 2 nps u32 A_s, A_s = sum |g| |x| (bias sums: sum |g|):
                    the bound tests/proj_refs.py uses for dW; empty slabs exactly +0.0; the float64 sum of the slabs within the sum
                    of the slabs' bounds.
  lin1 g_x          bit for bit fp32(g_out * w), rounded to nearest-even for bf16; exactly 0.0 where relu_mask is set and x is not > 0.
  reduce_slabs      bit for bit the fp32 sum in slab order from +0.0f.
  weight re-layouts bit for bit the element the header's layout names (bf16: its round-to-nearest-even).
  permute / gather  bit for bit; the hash: the sum modulo 2^64 the header states, in Python integers.
  masked loss       g_out within 4 u32 |ref| per element (one subtraction, one scale; SCE: the max-norm 1e-6 of
                    test_gpu_criterion.py's clamped-branch check), exactly 0 off the mask; the loss within (N / 1024 + 11) u32
                    sum |term| / M (per-thread partial sums of at most ceil(N / 1024) terms, then a 10-level tree).

None of the bounds is tuned to what the kernels give; tests/test_misc_turnover_host.py holds float32 restatements of each sum, taken
in another order, to them and shows that they reject planted faults.  Every ``hold_*`` returns the worst error / bound it saw."""
import numpy as np
import torch

import misc_cases as MC
from proj_cases import slab_bounds
from proj_refs import TORCH_DTYPE, U32, hold
from sampler_ref import GOLDEN, M64, mix64

HASH_DST = 0xD1B54A32D192ED03
# NaN bit patterns no kernel here produces: outputs are pre-filled with them, a word that still holds one was not written
SENTINEL = {"f32": (torch.int32, 0xFFC0DEAD - (1 << 32)), "bf16": (torch.int16, 0x7FA5), "u8": (torch.uint8, 0xA5),
            "i64": (torch.int64, 0x7FF8DEADBEEF0001)}
STORE = dict(TORCH_DTYPE, u8=torch.uint8, i64=torch.int64)
NEG_DENORMAL = -1e-40


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- sentinels and bits -------------------------------------------------------------------------------------------------------------
def sentinel(shape, dtype, device="cpu"):
    idt, value = SENTINEL[dtype]
    t = torch.empty(shape, dtype=STORE[dtype], device=device)
    t.view(idt).fill_(value)
    return t


def is_sentinel(t, dtype):
    idt, value = SENTINEL[dtype]
    return t.view(idt) == value


def bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool((bits(a) == bits(b)).all())


def guarded_vector(v, N, fill):
    """v[:N] followed by GUARD_ROWS elements of ``fill`` (a vector's guard rows)."""
    out = torch.full((N + MC.GUARD_ROWS,), fill, dtype=v.dtype, device=v.device)
    out[:N] = v[:N]
    return out


# ---- lin0 / lin1 forward ------------------------------------------------------------------------------------------------------------
def lin0_inputs(nc, rows, dtype, seed):
    """x [rows], mask [rows] (0 / 1, a third of the nodes), x_masked (NaN, +Inf, -Inf on the masked nodes), w, b [nc], g [rows, nc]."""
    g = _gen(seed)
    x = torch.randn(rows, generator=g)
    mask = (torch.rand(rows, generator=g) < 1 / 3).to(torch.uint8)
    w, b = torch.randn(nc, generator=g), torch.randn(nc, generator=g)
    grad = torch.randn(rows, nc, generator=g).to(TORCH_DTYPE[dtype])
    x_masked = x.clone()
    idx = mask.nonzero().flatten()
    x_masked[idx] = torch.tensor([float("nan"), float("inf"), float("-inf")])[torch.arange(idx.numel()) % 3]
    return {"x": x, "mask": mask, "x_masked": x_masked, "w": w, "b": b, "g": grad}


def masked_x(x, mask):
    return x if mask is None else torch.where(mask != 0, torch.zeros_like(x), x)


def lin0_fwd_ref(x, mask, w, b, dtype):
    """fp32 product, then fp32 sum (two roundings, no fused multiply-add), rounded to the storage type."""
    prod = masked_x(x, mask).float()[:, None] * w.float()[None, :]
    return (prod + b.float()[None, :]).to(TORCH_DTYPE[dtype])


def lin1_inputs(nc, rows, dtype, seed):
    """x [rows, nc] in the storage type, w [nc] (scaled by nc^-1/2), b [1], g_out [rows]."""
    g = _gen(seed)
    return {"x": torch.randn(rows, nc, generator=g).to(TORCH_DTYPE[dtype]), "w": torch.randn(nc, generator=g) / nc ** 0.5,
            "b": torch.randn(1, generator=g), "g_out": torch.randn(rows, generator=g)}


def lin1_fwd_reference(x, w, b):
    """(reference, bound) per row in float64."""
    xd, wd = x.double(), w.double()
    ref = xd @ wd + (0.0 if b is None else b.double()[0])
    return ref, x.shape[1] * U32 * (xd.abs() @ wd.abs()) + U32 * ref.abs()


def hold_lin1_fwd(out, x, w, b, what=""):
    ref, bound = lin1_fwd_reference(x, w, b)
    return {"out": hold(out, ref, bound, what + " out")}


# ---- lin0 / lin1 backward -----------------------------------------------------------------------------------------------------------
def plant_relu(x):
    """+0.0, -0.0 and a negative denormal into the first, middle and last elements of x [N, nc] (in place), twice over where it
    has eight elements or more so that every value also sits away from column 0."""
    flat = x.view(-1)
    n = flat.numel()
    vals = [0.0, -0.0, NEG_DENORMAL]
    for k, pos in enumerate([0, n // 2, n - 1]):
        flat[pos] = vals[k]
    if n >= 8:
        for k, pos in enumerate([1, n // 2 + 1, n - 2]):
            flat[pos] = vals[(k + 1) % 3]
    return x


def lin1_bwd_operands(p, N):
    """(g_out [N], x [N, nc]) of a lin1 backward case: x with the planted zeros and denormals, and g_out = +-2 on the rows that
    hold a denormal.  The product of a denormal with anything but a power of two is rounded on the denormal grid -- an absolute
    error of 2^-150 that the relative bounds (the formats' normal range) do not describe and that a slab of one row would show;
    with a power of two the product is exact and every sum it enters is rounded like any other."""
    x = plant_relu(p["x"][:N].clone())
    g_out = p["g_out"][:N].clone()
    tiny = ((x != 0) & (x.float().abs() < 2.0 ** -126)).any(1)
    g_out[tiny] = torch.where(g_out[tiny] < 0, -2.0, 2.0)
    return g_out, x


def slab_sums(terms, N, S):
    """Per-slab column sums of ``terms`` [N, P] (float64) and of their magnitudes: [S, P] each."""
    nps, _ = slab_bounds(N, S)
    out = torch.zeros(S * nps, terms.shape[1], dtype=torch.float64, device=terms.device)
    out[:N] = terms[:N]
    out = out.view(S, nps, -1)
    return out.sum(1), out.abs().sum(1)


def lin0_bwd_terms(g, x, mask):
    """{output: terms [N, nc]}: slab_w sums g * xm, slab_b sums g."""
    gd = g.double()
    return {"slab_w": gd * masked_x(x, mask).double()[:, None], "slab_b": gd}


def lin1_bwd_terms(g_out, x):
    """slab_w sums g_out * x [N, nc], slab_b sums g_out [N, 1]."""
    god = g_out.double()[:, None]
    return {"slab_w": god * x.double(), "slab_b": god}


def lin1_gx_ref(g_out, x, w, relu_mask, dtype):
    prod = g_out.float()[:, None] * w.float()[None, :]
    if relu_mask:
        prod = torch.where(x > 0, prod, torch.zeros_like(prod))
    return prod.to(TORCH_DTYPE[dtype])


def hold_gx(g_x, g_out, x, w, relu_mask, dtype, what=""):
    """Bit for bit on the outputs that pass, exactly 0.0 on those the ReLU mask zeroes."""
    ref = lin1_gx_ref(g_out, x, w, relu_mask, dtype)
    keep = (x > 0) if relu_mask else torch.ones_like(x, dtype=torch.bool)
    assert bool((g_x[~keep] == 0).all()), f"{what} g_x: {int((g_x[~keep] != 0).sum())} masked outputs are not exactly 0.0"
    diff = bits(g_x)[keep] != bits(ref)[keep]
    assert not bool(diff.any()), f"{what} g_x: {int(diff.sum())} of {int(keep.sum())} outputs differ from fp32(g_out * w)"


def hold_slabs(buf, terms, N, S, what=""):
    """``buf`` [S, stride] as the launch left it, pre-filled with the fp32 sentinel; ``terms``: {name: [N, width] float64} in the
    order the sums lie in a slab, from word 0.  Every sum written, every word behind them untouched, empty slabs +0.0 bit for
    bit, each slab and the sum of the slabs within their bounds."""
    used = sum(t.shape[1] for t in terms.values())
    nps, rows = slab_bounds(N, S)
    assert buf.shape[0] == S and buf.shape[1] > used
    assert bool(is_sentinel(buf[:, used:], "f32").all()), f"{what}: the pad words behind a slab's sums were written"
    left = is_sentinel(buf[:, :used], "f32").any(1)
    assert not bool(left.any()), f"{what}: slabs {left.nonzero().flatten().tolist()} keep words from before the launch"
    empty = [s for s, (beg, end) in enumerate(rows) if beg >= end]
    if empty:
        assert bool((bits(buf[empty, :used]) == 0).all()), f"{what}: an empty slab is not exactly +0.0"
    out, off = {}, 0
    for name, t in terms.items():
        got = buf[:, off:off + t.shape[1]]
        off += t.shape[1]
        ref, A = slab_sums(t, N, S)
        bound = 2 * nps * U32 * A
        out[name] = hold(got, ref, bound, f"{what} {name} slab")
        out[name + " sum"] = hold(got.double().sum(0), ref.sum(0), bound.sum(0), f"{what} {name} sum of slabs")
    return out


def slab_bound(terms, N, S):
    """{name: bound [S, width]}: the bound alone (the two forms of a backward agree within the sum of their bounds)."""
    nps, _ = slab_bounds(N, S)
    return {name: 2 * nps * U32 * slab_sums(t, N, S)[1] for name, t in terms.items()}


# ---- gatres_reduce_slabs ------------------------------------------------------------------------------------------------------------
def reduce_inputs(num_slabs, count, seed, minus_zero_column=None):
    """slabs [num_slabs, count + REDUCE_PAD]: normal values, NaN in the pad words, one column of -0.0."""
    g = _gen(seed)
    slabs = torch.full((num_slabs, count + MC.REDUCE_PAD), float("nan"))
    slabs[:, :count] = torch.randn(num_slabs, count, generator=g)
    if minus_zero_column is not None:
        slabs[:, minus_zero_column] = -0.0
    return slabs


def reduce_ref(slabs, count, skip=()):
    """The fp32 sum in slab order from +0.0f: one rounded add per slab, nothing fused."""
    a = slabs.cpu().numpy().astype(np.float32)
    acc = np.zeros(count, dtype=np.float32)
    for s in range(a.shape[0]):
        if s not in skip:
            acc = (acc + a[s, :count]).astype(np.float32)
    return torch.from_numpy(acc)


# ---- the weight re-layouts ----------------------------------------------------------------------------------------------------------
BF16_NORMALS = 0x7F80 - 0x0080          # positive normal bf16 values: 32512, fewer than the 32768 elements of a weight at nc = 128


def weight_params(num_blocks, nc, kind, seed=0):
    """The flat parameter vector.  "index": element i holds float(i) (distinct, exact in fp32).  "bf16": NaN everywhere but in the
    conv weights, whose elements are bf16-exact: conv1's positive, conv2's negative, distinct over the whole vector up to nc = 32;
    at nc = 128 a matrix has more elements than bf16 has positive normal values and element e repeats element e - 32512.
    "random": normal values (their conversion rounds)."""
    count = MC.param_count(num_blocks, nc)
    if kind == "index":
        return torch.arange(count, dtype=torch.float32)
    if kind == "random":
        return torch.randn(count, generator=_gen(seed))
    per = 2 * nc * nc
    p = np.full(count, np.nan, dtype=np.float32)
    for b, (o1, o2) in enumerate(MC.conv_weight_offsets(num_blocks, nc)):
        k = np.arange(per, dtype=np.int64) + b * 2 * per
        pos = ((0x0080 + k % BF16_NORMALS) << 16).astype(np.uint32)
        neg = ((0x0080 + (k + per) % BF16_NORMALS) << 16).astype(np.uint32) | np.uint32(0x80000000)
        p[o1:o1 + per] = pos.view(np.float32)
        p[o2:o2 + per] = neg.view(np.float32)
    return torch.from_numpy(p)


def conv_weights(params, num_blocks, nc):
    """[(W1 [2nc, nc], W2 [nc, 2nc])] per block: views of the flat vector (include/gatres.h, flat parameter layout)."""
    per = 2 * nc * nc
    return [(params[o1:o1 + per].view(2 * nc, nc), params[o2:o2 + per].view(nc, 2 * nc))
            for o1, o2 in MC.conv_weight_offsets(num_blocks, nc)]


def transposed_layout(params, num_blocks, nc, swap=None):
    """[W1^T | W2^T] per block, flat.  ``swap`` = (i, j): the fault of a transposed index pair, element [i, j] of every W1^T taken
    from W1[i, j] instead of W1[j, i] (the host test plants it)."""
    out = []
    for W1, W2 in conv_weights(params, num_blocks, nc):
        t1 = W1.t().contiguous()
        if swap is not None:
            i, j = swap
            t1[i, j] = W1.reshape(-1)[i * 2 * nc + j]
        out += [t1.reshape(-1), W2.t().reshape(-1)]
    return torch.cat(out)


def converted_layout(params, num_blocks, nc):
    """[W1 | W2 | W1^T | W2^T] per block, flat, in fp32 (the caller rounds to bf16)."""
    out = []
    for W1, W2 in conv_weights(params, num_blocks, nc):
        out += [W1.reshape(-1), W2.reshape(-1), W1.t().reshape(-1), W2.t().reshape(-1)]
    return torch.cat(out)


# ---- permute / gather / hash --------------------------------------------------------------------------------------------------------
def permute_inputs(N, seed):
    """src [N] fp32 with two NaN payloads and -0.0 among normal values, bytes [N] in 0..99, perm [N] int32."""
    g = _gen(seed)
    src = torch.randn(N, generator=g)
    b = bits(src)
    for k, pattern in enumerate((0x7FC00001, 0xFFC12345 - (1 << 32), 0x80000000 - (1 << 32))):
        b[(k * 97 + N // 2) % N] = pattern
    return {"src": src, "bytes": torch.randint(0, 100, (N,), generator=g, dtype=torch.uint8),
            "perm": torch.randperm(N, generator=g).to(torch.int32)}


def edge_inputs(E, seed, nodes=1000):
    """edge_index [2, E] int64: node ids below ``nodes``, and two large ones where there is room."""
    ei = torch.randint(0, nodes, (2, E), generator=_gen(seed), dtype=torch.int64)
    if E >= 8:
        ei[0, 3], ei[1, 5] = 2 ** 31 - 1, 2 ** 40 + 7
    return ei


def edge_hash_ref(ei, skip_last=False):
    """sum over the edges of mix64(mix64(src + GOLDEN * (e + 1)) ^ (dst + 0xD1B54A32D192ED03)) modulo 2^64."""
    src, dst = ei[0].tolist(), ei[1].tolist()
    h = 0
    for e in range(len(src) - (1 if skip_last else 0)):
        a = mix64(src[e] + GOLDEN * (e + 1))
        h = (h + mix64(a ^ ((dst[e] + HASH_DST) & M64))) & M64
    return h


# ---- masked loss --------------------------------------------------------------------------------------------------------------------
def loss_inputs(N, seed, density=MC.LOSS_DENSITY):
    """out, y [N] normal, mask [N] at the density; from 1023 nodes on two masked predictions below SCE's eps = 1e-12 (one of them
    next to the last node), so that SCE's gradient is not zero everywhere."""
    g = _gen(seed)
    out, y = torch.randn(N, generator=g), torch.randn(N, generator=g)
    mask = (torch.rand(N, generator=g) < density).to(torch.uint8)
    mask[0] = 1                                            # (never an empty mask: M == 0 is test_gpu_criterion.py's case)
    if N >= 1023:
        for pos, v in ((5, 5e-13), (N - 2, -3e-13)):
            out[pos], mask[pos] = v, 1
    return out, y, mask


def last_node_mask(N):
    mask = torch.zeros(N, dtype=torch.uint8)
    mask[N - 1] = 1
    return mask


def hold_loss(crit, loss, g_out, out, y, mask, table, what=""):
    """``table``: tests/test_gpu_criterion.py's fp64 table.  Every criterion's terms are non-negative (d^2, |d|, (1 - o^ y^)^3 with
    o^ y^ in [-1, 1]), so sum |term| / M is the reference loss itself."""
    N = out.numel()
    l64, g64 = table(crit, out, y, mask)
    m = mask.bool().cpu()
    g = g_out.detach().cpu()
    assert bool((g[~m] == 0).all()), f"{what}: g_out is not exactly 0 off the mask"
    res = {}
    if crit == "sce":
        gd = g.double()
        if float(g64.abs().max()) == 0.0:
            assert bool((gd == 0).all()), f"{what}: g_out is not zero where the reference is"
            res["g_out"] = 0.0
        else:
            e = float((gd - g64).abs().max() / g64.abs().max())
            assert e < 1e-6, f"{what}: g_out max-norm error {e:.3e} >= 1e-6"
            res["g_out"] = e / 1e-6
    else:
        res["g_out"] = hold(g, g64, 4 * U32 * g64.abs(), what + " g_out")
    bound = (N / MC.LOSS_THREADS + 11) * U32 * l64.abs().reshape(1)
    res["loss"] = hold(loss.detach().cpu().reshape(1), l64.reshape(1), bound, what + " loss")
    return res
