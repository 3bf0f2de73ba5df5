"""The dense projection kernels of csrc/k_proj.hip at the sizes where their tiling turns over, against float64: the seven the
product library launches (proj_kernel, proj_lds_kernel, proj_bf16_kernel, proj_bf16_tile_kernel, dw_kernel, dw_bf16_kernel,
dw2d_bf16_kernel; the streaming kernel exists in the diagnostic build only, the hidden co-launch entry point is not called) and
the two conv_param_grads kernels that share the weight gradient's slabs.

tests/proj_cases.py says which sizes and why (a workgroup's second and third trip, a last workgroup or tile of one row, the grid
caps, slabs that end inside a trip, empty slabs, the 2-D weight-gradient form with and without its workgroup renumbering);
tests/proj_refs.py states the float64 reference and the element-wise bounds; tests/test_proj_turnover_host.py holds both
against the kernel source on the host.  Each launch here goes through the C ABI on buffers this module owns:

  * outputs carry 16 guard rows of a sentinel bit pattern behind row N, slab buffers are NaN with 8 pad words per slab: nothing
    outside the result may change, nothing inside it may be left;
  * inputs carry 16 rows of NaN behind row N (allocated memory): a row index that is not clamped shows as a NaN in the result;
  * every output is held to its bound element by element, masked outputs are exactly 0.0 (relu_ref = +0.0 and -0.0 included);
  * rows are independent, bit for bit: the launch on X[perm] returns OUT[perm] -- a row computed from a neighbour's prefetched
    fragment fails this where a tolerance might not;
  * proj_lds_kernel equals proj_kernel bit for bit down to its threshold of 16384 rows.
The worst error / bound per kernel and output goes into the parity report (profiles/proj_turnover_margins.txt)."""
import pytest
import torch

import proj_cases as PC
import proj_refs as R
from test_gpu_model import note

pytestmark = pytest.mark.gpu

SENTINEL = {"f32": (torch.int32, 0xFFC0DEAD - (1 << 32)), "bf16": (torch.int16, 0x7FA5)}       # both are NaN bit patterns
BADARG, UNSUPPORTED = -1, -2
WORST = {}


@pytest.fixture(scope="module")
def ops():
    from tests import hipops
    return hipops


def _record(kernel, ratios):
    for name, r in ratios.items():
        key = f"{kernel} {name}"
        WORST[key] = max(WORST.get(key, 0.0), r)


@pytest.fixture(autouse=True)
def _note_worst():
    """One entry of the parity report for the module, rewritten once per test."""
    yield
    if WORST:
        note("projection turnover: worst |kernel - fp64| / bound per kernel and output", dict(sorted(WORST.items())))


def _out(rows, cols, dtype):
    """[rows + GUARD_ROWS, cols] filled with the sentinel, guard rows included."""
    idt, value = SENTINEL[dtype]
    t = torch.empty(rows + PC.GUARD_ROWS, cols, dtype=R.TORCH_DTYPE[dtype], device="cuda")
    t.view(idt).fill_(value)
    return t


def _guards_intact(t, rows, dtype):
    idt, value = SENTINEL[dtype]
    return bool((t.view(idt)[rows:] == value).all())


def _cuda(d):
    return {k: v.cuda() for k, v in d.items()}


def _perm(N, seed):
    return torch.randperm(N, generator=torch.Generator().manual_seed(seed)).cuda()


def _seed(*shape):
    return 1000003 * shape[0] + 1009 * shape[1] + shape[2]


def _shape_id(shape):
    return "x".join(map(str, shape))


def _set_knobs(monkeypatch, knobs):
    for k in knobs:
        monkeypatch.setenv(PC.KNOBS[k], "1")


def _fwd(ops, X, p, N, K, M, H, dtype):
    """One forward launch on rows X [N, K]: (h, a_src, a_dst), each [N, ...], guard rows checked."""
    x = R.with_guard_rows(X, N)
    h, a_s, a_d = _out(N, M, dtype), _out(N, H, "f32"), _out(N, H, "f32")
    rc = ops.t_proj_attn_fwd(x, p["W"], p["att_src"], p["att_dst"], h, a_s, a_d, N, K, H, M // H, dtype)
    assert rc == 0, rc
    assert _guards_intact(h, N, dtype) and _guards_intact(a_s, N, "f32") and _guards_intact(a_d, N, "f32"), "wrote behind row N"
    return h[:N], a_s[:N], a_d[:N]


def _dx(ops, X, W, resid, relu_ref, N, K, M, dtype):
    """One data-gradient launch: g_x [N, M] from g_h = X [N, K] (reduction over K), Wt = W [M, K]."""
    g_x = _out(N, M, dtype)
    guard = lambda t: None if t is None else R.with_guard_rows(t, N)      # noqa: E731
    rc = ops.t_proj_bwd_dx(guard(X), W, guard(resid), guard(relu_ref), g_x, N, M, K, dtype)
    assert rc == 0, rc
    assert _guards_intact(g_x, N, dtype), "wrote behind row N"
    return g_x[:N]


def _run_fwd_case(ops, kernel, dtype, shape, sizes, below=()):
    K, M, H = shape
    p = _cuda(R.fwd_inputs(K, M, max(sizes), dtype, _seed(*shape)))
    for N in sizes:
        assert PC.plan("fwd", dtype, N, K, M, H)["kernel"] == ("proj_kernel" if N in below else kernel)
        what = f"{kernel} fwd {shape} N={N}"
        X = p["X"][:N]
        h, a_s, a_d = _fwd(ops, X, p, N, K, M, H, dtype)
        _record(kernel + " fwd", R.hold_fwd(h, a_s, a_d, X, p["W"], p["att_src"], p["att_dst"], H, dtype, what))
        pi = _perm(N, N)
        hp, sp, dp = _fwd(ops, X[pi], p, N, K, M, H, dtype)
        assert torch.equal(hp, h[pi]) and torch.equal(sp, a_s[pi]) and torch.equal(dp, a_d[pi]), what + ": rows depend on their place"


def _run_dx_case(ops, kernel, dtype, shape, sizes, n_all, below=()):
    K, M, _ = shape
    p = _cuda(R.dx_inputs(K, M, max(sizes), dtype, _seed(*shape) + 1))
    for N in sizes:
        assert PC.plan("dx", dtype, N, K, M)["kernel"] == ("proj_kernel" if N in below else kernel)
        X, resid, relu = p["X"][:N], p["resid"][:N], R.plant_zeros(p["relu_ref"][:N].clone())
        for with_resid, with_mask in (PC.OPERANDS if N == n_all else PC.OPERANDS[:1]):
            what = f"{kernel} dx {shape} N={N} resid={with_resid} mask={with_mask}"
            r, m = (resid if with_resid else None), (relu if with_mask else None)
            g_x = _dx(ops, X, p["W"], r, m, N, K, M, dtype)
            _record(kernel + " dx", R.hold_dx(g_x, X, p["W"], r, m, dtype, what))
            if with_resid and with_mask:
                pi = _perm(N, N + 1)
                gp = _dx(ops, X[pi], p["W"], resid[pi], relu[pi], N, K, M, dtype)
                assert torch.equal(gp, g_x[pi]), what + ": rows depend on their place"


# ---- forward and data gradient ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["fwd", "dx"])
@pytest.mark.parametrize("shape", PC.PROJ_F32["shapes"], ids=_shape_id)
def test_proj_kernel(ops, kind, shape):
    sizes = dict(PC.proj_cases(PC.PROJ_F32))[shape]
    if kind == "fwd":
        _run_fwd_case(ops, "proj_kernel", "f32", shape, sizes)
    else:
        _run_dx_case(ops, "proj_kernel", "f32", shape, sizes, PC.PROJ_F32["N_all_epilogues"])


@pytest.mark.parametrize("kind", ["fwd", "dx"])
@pytest.mark.parametrize("shape", PC.PROJ_LDS["shapes"], ids=_shape_id)
def test_proj_lds_kernel(ops, kind, shape):
    sizes = dict(PC.proj_cases(PC.PROJ_LDS))[shape]
    below = [n for n in sizes if n < PC.LDS_MIN_ROWS]
    if kind == "fwd":
        _run_fwd_case(ops, "proj_lds_kernel", "f32", shape, sizes, below)
    else:
        _run_dx_case(ops, "proj_lds_kernel", "f32", shape, sizes, PC.PROJ_LDS["N_all_epilogues"], below)


@pytest.mark.parametrize("kind", ["fwd", "dx"])
@pytest.mark.parametrize("shape", PC.PROJ_BF16_TILE["shapes"], ids=_shape_id)
def test_proj_bf16_tile_kernel(ops, kind, shape):
    sizes = dict(PC.proj_cases(PC.PROJ_BF16_TILE))[shape]
    if kind == "fwd":
        _run_fwd_case(ops, "proj_bf16_tile_kernel", "bf16", shape, sizes)
    else:
        _run_dx_case(ops, "proj_bf16_tile_kernel", "bf16", shape, sizes, PC.PROJ_BF16_TILE["N_all_epilogues"])


@pytest.mark.parametrize("kind", ["fwd", "dx"])
@pytest.mark.parametrize("shape", PC.PROJ_BF16_ROWS["shapes"], ids=_shape_id)
def test_proj_bf16_kernel(ops, kind, shape):
    sizes = dict(PC.proj_cases(PC.PROJ_BF16_ROWS))[shape]
    if kind == "fwd":
        _run_fwd_case(ops, "proj_bf16_kernel", "bf16", shape, sizes)
    else:
        _run_dx_case(ops, "proj_bf16_kernel", "bf16", shape, sizes, PC.PROJ_BF16_ROWS["N_all_epilogues"])


@pytest.mark.parametrize("shape", PC.PROJ_LDS["shapes"], ids=_shape_id)
def test_proj_lds_kernel_equals_proj_kernel_down_to_its_threshold(ops, shape, monkeypatch):
    """The claim of test_wide_projection_on_many_rows_matches_the_tile_kernel (20037 rows) at 16384 rows, with a last workgroup of
    one row and with a second trip of one row: outputs, logits and the masked data gradient, bit for bit."""
    K, M, H = shape
    sizes = PC.PROJ_LDS["N_equal"]
    f, d = _cuda(R.fwd_inputs(K, M, max(sizes), "f32", _seed(*shape) + 2)), _cuda(R.dx_inputs(K, M, max(sizes), "f32", _seed(*shape) + 3))
    got = {}
    for knobs in ((), ("no_proj_lds",)):
        _set_knobs(monkeypatch, knobs)
        for N in sizes:
            assert PC.plan("fwd", "f32", N, K, M, H, knobs=knobs)["kernel"] == ("proj_kernel" if knobs else "proj_lds_kernel")
            relu = R.plant_zeros(d["relu_ref"][:N].clone())
            got[knobs, N] = _fwd(ops, f["X"][:N], f, N, K, M, H, "f32") + (_dx(ops, d["X"][:N], d["W"], d["resid"][:N], relu, N, K, M, "f32"),)
    for N in sizes:
        for a, b in zip(got[(), N], got[("no_proj_lds",), N]):
            assert torch.equal(a, b), (shape, N)


# ---- weight gradient ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,dtype,shape,knobs,cases", PC.dw_cases(),
                         ids=["-".join([c[0], c[1], "%dx%d" % c[2], *c[3], "%d" % len(c[4])]) for c in PC.dw_cases()])
def test_dw_kernels(ops, kernel, dtype, shape, knobs, cases, monkeypatch):
    HC, K = shape
    _set_knobs(monkeypatch, knobs)
    p = _cuda(R.dw_inputs(HC, K, max(n for n, _ in cases), dtype, _seed(HC, K, 7)))
    stride = HC * K + PC.SLAB_PAD
    for N, S in cases:
        assert PC.plan("dw", dtype, N, K, HC, S=S, knobs=knobs)["kernel"] == kernel
        G, X = p["G"][:N], p["X"][:N]
        slabs = torch.full((S, stride), float("nan"), device="cuda")
        rc = ops.t_proj_bwd_dw(R.with_guard_rows(G, N), R.with_guard_rows(X, N), slabs, S, stride, N, K, HC, dtype)
        assert rc == 0, rc
        _record(kernel + ("" if dtype == "f32" or kernel != "dw_kernel" else " (bf16 storage)"),
                R.hold_dw(slabs, G, X, N, S, f"{kernel} {dtype} {shape} N={N} S={S}"))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("H,C", PC.CONV_GRADS["shapes"])
def test_conv_param_grads_slabs(ops, H, C, dtype):
    """The attention-vector / bias column sums share the weight gradient's slab bounds: the same sentinel rule, slab by slab."""
    HC = H * C
    cases = PC.CONV_GRADS["NS"]
    p = _cuda(R.conv_grad_inputs(H, C, max(n for n, _ in cases), dtype, _seed(H, C, 9)))
    stride = 3 * HC + PC.SLAB_PAD
    for N, S in cases:
        slabs = torch.full((S, stride), float("nan"), device="cuda")
        g = {k: R.with_guard_rows(v, N) for k, v in p.items()}
        rc = ops.t_conv_param_grads(g["h"], g["g_a_src"], g["g_a_dst"], g["g_out"], slabs, S, stride, N, H, C, dtype)
        assert rc == 0, rc
        _record(f"conv_param_grads {dtype}", R.hold_conv_grads(slabs, p["h"][:N], p["g_a_src"][:N], p["g_a_dst"][:N], p["g_out"][:N],
                                                                N, S, H, f"conv_param_grads {dtype} H={H} C={C} N={N} S={S}"))


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_misaligned_empty_and_unsupported_calls_are_refused_without_a_launch(ops):
    """A pointer 4 bytes off a 16-byte boundary or num_nodes = 0: GATRES_E_BADARG; K = 48 (no such width) or bf16 at nc = 16 (the
    bf16 matrix-core step is 32 long): GATRES_E_UNSUPPORTED.  The output buffers keep their sentinels."""
    N = 64

    def attempt(dtype, K, M, H, off=0, n=N, dw=True):
        x, W, att = _out(N, K, dtype), _out(M, K, dtype), _out(M, 1, "f32")
        h, a_s, a_d, g_x = _out(N, M, dtype), _out(N, H, "f32"), _out(N, H, "f32"), _out(N, M, dtype)
        res, ref = _out(N, M, dtype), _out(N, M, dtype)
        slabs = _out(2, M * K, "f32")
        rcs = (ops.t_proj_attn_fwd(x.data_ptr() + off, W, att, att, h, a_s, a_d, n, K, H, M // H, dtype),
               ops.t_proj_bwd_dx(x.data_ptr() + off, W, res, ref, g_x, n, M, K, dtype),
               ops.t_proj_bwd_dw(h, x.data_ptr() + off, slabs, 2, M * K, n, K, M, dtype) if dw else None)
        torch.cuda.synchronize()
        for t, d in ((h, dtype), (a_s, "f32"), (a_d, "f32"), (g_x, dtype), (slabs, "f32")):
            assert _guards_intact(t, 0, d), "a refused call wrote to its output"
        return rcs

    for dtype, K, M, H in (("f32", 32, 64, 2), ("bf16", 32, 64, 2)):
        assert attempt(dtype, K, M, H, off=4) == (BADARG,) * 3
        assert attempt(dtype, K, M, H, n=0) == (BADARG,) * 3
    assert attempt("f32", 48, 96, 2) == (UNSUPPORTED,) * 3
    assert attempt("bf16", 48, 96, 2) == (UNSUPPORTED,) * 3
    # (the weight gradient takes narrow bf16 tables: dw_kernel widens them to fp32, tests/proj_cases.py DW_F32["bf16_shapes"])
    assert attempt("bf16", 16, 32, 2, dw=False) == (UNSUPPORTED, UNSUPPORTED, None)
    x, W = _out(N, 32, "f32"), _out(64, 32, "f32")
    for bad in ({"h": 4}, {"W": 4}):
        h, a = _out(N, 64, "f32"), _out(N, 2, "f32")
        att = _out(64, 1, "f32")
        assert ops.t_proj_attn_fwd(x, W.data_ptr() + bad.get("W", 0), att, att, h.data_ptr() + bad.get("h", 0), a, a, N, 32, 2, 32,
                                   "f32") == BADARG
        torch.cuda.synchronize()
        assert _guards_intact(h, 0, "f32")
    g_x, res = _out(N, 64, "f32"), _out(N, 64, "f32")
    assert ops.t_proj_bwd_dx(x, W, res.data_ptr() + 4, None, g_x, N, 64, 32, "f32") == BADARG
    assert ops.t_proj_bwd_dx(x, W, None, res.data_ptr() + 4, g_x, N, 64, 32, "f32") == BADARG
    slabs = _out(2, 64 * 32, "f32")
    assert ops.t_proj_bwd_dw(g_x, x, slabs, 0, 64 * 32, N, 32, 64, "f32") == BADARG
    torch.cuda.synchronize()
    assert _guards_intact(g_x, 0, "f32") and _guards_intact(slabs, 0, "f32")
