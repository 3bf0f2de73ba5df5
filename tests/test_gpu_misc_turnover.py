"""The small per-op kernels of csrc/k_misc.hip where their lanes, trips and slabs turn over, against fp32 bit for bit or float64:
lin0 / lin1 forward, their backward in the rows form and the wave form, gatres_reduce_slabs, the two weight re-layouts, the node
relabelling copies, the edge_index hash and the masked loss.  (conv_param_grads: tests/test_gpu_proj_turnover.py; the region
reduction: tests/test_gpu_bf16.py; adam_kernel: tests/test_gpu_adam_elementwise.py.)

tests/misc_cases.py says which sizes and why, tests/misc_refs.py states the references and the bounds, and
tests/test_misc_turnover_host.py holds both against the kernel source on the host.  Each launch here goes through the C ABI on
buffers this module owns:

  * outputs are pre-filled with a NaN sentinel bit pattern: row outputs carry 16 guard rows behind row N, slab buffers a stride
    larger than the parameter count -- every word of the result is written, no other word changes, empty slabs are +0.0f;
  * inputs carry 16 rows of NaN (the mask: a non-zero byte) behind row N;
  * every launch is made twice and gives the same bits;
  * a slab does not depend on its neighbours: the launch on its rows alone gives the same bits;
  * refused calls return the documented code and leave the sentinel in place.
The worst error / bound per kernel and output goes into the parity report (profiles/misc_turnover_margins.txt)."""
import pytest
import torch

import misc_cases as MC
import misc_refs as R
from proj_refs import with_guard_rows
from test_gpu_criterion import table
from test_gpu_model import note

pytestmark = pytest.mark.gpu

G = MC.GUARD_ROWS
WORST = {}
NAN = float("nan")


@pytest.fixture(scope="module")
def abi(pkg):
    """(library, dtype codes, criterion codes, the current stream)."""
    N_ = pkg._native
    return {"lib": N_.load(), "f32": N_.DTYPE_F32, "bf16": N_.DTYPE_BF16, "crit": N_.CRITERIA, "stream": N_.current_stream("cuda")}


def _record(kernel, ratios):
    for name, r in ratios.items():
        key = f"{kernel} {name}"
        WORST[key] = max(WORST.get(key, 0.0), r)


@pytest.fixture(autouse=True)
def _note_worst():
    """One entry of the parity report for the module, rewritten once per test."""
    yield
    if WORST:
        note("misc turnover: worst |kernel - reference| / bound per kernel and output", dict(sorted(WORST.items())))


def _p(t):
    return t if t is None or isinstance(t, int) else t.data_ptr()


def _cuda(d):
    return {k: v.cuda() for k, v in d.items()}


def _twice(launch, outputs):
    """Run ``launch`` (which fills and returns fresh output tensors) twice: the same bits both times; returns the first result."""
    first, second = launch(), launch()
    torch.cuda.synchronize()
    for name, a, b in zip(outputs, first, second):
        assert R.same_bits(a, b), f"{name}: two launches on the same inputs differ"
    return first


def _off_by_one(t, dtype):
    """A copy of ``t`` whose storage starts one element behind a 16-byte boundary, and the buffer that holds it (its first
    element keeps the sentinel)."""
    buf = R.sentinel((t.numel() + 1,), dtype, t.device)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == t.element_size()
    return view, buf


# ---- 1. lin0 forward ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("nc", MC.LIN0_FWD["nc"])
def test_lin0_fwd_is_the_fp32_product_and_sum_bit_for_bit(abi, nc, dtype):
    p = _cuda(R.lin0_inputs(nc, max(MC.LIN0_FWD["N"]), dtype, 100 + nc))
    for N in MC.LIN0_FWD["N"]:
        assert MC.lin0_fwd_plan(N, nc) is not None
        for with_mask in (False, True):
            what = f"lin0 fwd {dtype} nc={nc} N={N} mask={with_mask}"
            x = R.guarded_vector(p["x_masked"] if with_mask else p["x"], N, NAN)
            mask = R.guarded_vector(p["mask"], N, 1) if with_mask else None

            def launch():
                out = R.sentinel((N + G, nc), dtype, "cuda")
                rc = abi["lib"].gatres_t_lin0_fwd(_p(x), _p(mask), _p(p["w"]), _p(p["b"]), _p(out), N, nc, abi[dtype], abi["stream"])
                assert rc == 0, (what, rc)
                return (out,)
            out, = _twice(launch, ["out"])
            assert bool(R.is_sentinel(out[N:], dtype).all()), what + ": wrote behind row N"
            assert not bool(R.is_sentinel(out[:N], dtype).any()), what + ": left outputs unwritten"
            ref = R.lin0_fwd_ref(x[:N], None if mask is None else mask[:N], p["w"], p["b"], dtype)
            assert R.same_bits(out[:N], ref), what + f": {int((R.bits(out[:N]) != R.bits(ref)).sum())} outputs differ"
            if with_mask:                                   # a masked node holds the bias whatever x holds there
                m = p["mask"][:N] != 0
                assert R.same_bits(out[:N][m], p["b"].to(out.dtype).expand(int(m.sum()), nc).contiguous())


def test_lin0_fwd_refusals(abi):
    N, nc = 8, 8
    for dtype in ("f32", "bf16"):
        x, w, b = torch.ones(N, device="cuda"), torch.ones(nc + 4, device="cuda"), torch.ones(nc + 4, device="cuda")
        out = R.sentinel((N + G, nc), dtype, "cuda")
        call = lambda w_=w, b_=b, o_=out, nc_=nc: abi["lib"].gatres_t_lin0_fwd(  # noqa: E731
            _p(x), None, _p(w_), _p(b_), _p(o_), N, nc_, abi[dtype], abi["stream"])
        assert call(nc_=MC.LIN0_FWD["refused_nc"]) == MC.UNSUPPORTED and MC.lin0_fwd_plan(N, MC.LIN0_FWD["refused_nc"]) is None
        assert call(w_=w.data_ptr() + 4) == MC.BADARG and call(b_=b.data_ptr() + 4) == MC.BADARG
        assert call(o_=out.data_ptr() + out.element_size()) == MC.BADARG
        torch.cuda.synchronize()
        assert bool(R.is_sentinel(out, dtype).all()), "a refused call wrote to its output"


# ---- 2. lin1 forward ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("nc", MC.LIN1_FWD["nc"])
def test_lin1_fwd_rows_against_fp64(abi, nc, dtype):
    p = _cuda(R.lin1_inputs(nc, max(MC.LIN1_FWD["N"]), dtype, 200 + nc))

    def run(X, N, b, what):
        x = with_guard_rows(X, N)

        def launch():
            out = R.sentinel((N + G,), "f32", "cuda")
            rc = abi["lib"].gatres_t_lin1_fwd(_p(x), _p(p["w"]), _p(b), _p(out), N, nc, abi[dtype], abi["stream"])
            assert rc == 0, (what, rc)
            return (out,)
        out, = _twice(launch, ["out"])
        assert bool(R.is_sentinel(out[N:], "f32").all()), what + ": wrote behind row N"
        assert not bool(R.is_sentinel(out[:N], "f32").any()), what + ": left rows unwritten"
        return out[:N]

    for N in MC.LIN1_FWD["N"]:
        assert MC.lin1_fwd_plan(N, nc)["G"] == nc // 4
        X = p["x"][:N]
        for b in (p["b"], None):
            what = f"lin1 fwd {dtype} nc={nc} N={N} bias={b is not None}"
            out = run(X, N, b, what)
            _record(f"lin1_fwd_kernel {dtype}", R.hold_lin1_fwd(out, X, p["w"], b, what))
            pi = torch.randperm(N, generator=torch.Generator().manual_seed(N)).cuda()
            assert R.same_bits(run(X[pi], N, b, what + " permuted"), out[pi]), what + ": rows depend on their place"


def test_lin1_fwd_refusals(abi):
    N = 8
    for nc in MC.LIN1_FWD["refused_nc"]:
        assert MC.lin1_fwd_plan(N, nc) is None
        x, w = torch.ones(N, nc, device="cuda"), torch.ones(nc, device="cuda")
        out = R.sentinel((N + G,), "f32", "cuda")
        assert abi["lib"].gatres_t_lin1_fwd(_p(x), _p(w), None, _p(out), N, nc, abi["f32"], abi["stream"]) == MC.UNSUPPORTED
        torch.cuda.synchronize()
        assert bool(R.is_sentinel(out, "f32").all())


# ---- 3. / 4. lin0 and lin1 backward -------------------------------------------------------------------------------------------------
def _lin0_bwd(abi, g, x, mask, N, S, nc, dtype, what, misaligned=False):
    """One lin0 backward on rows [0, N): the slab buffer [S, 2 nc + SLAB_PAD] as the launch left it (slab_w | slab_b | pad)."""
    stride = 2 * nc + MC.SLAB_PAD
    gg, xg = with_guard_rows(g, N), R.guarded_vector(x, N, NAN)
    mg = None if mask is None else R.guarded_vector(mask, N, 1)
    keep = None
    if misaligned:
        gg, keep = _off_by_one(gg, dtype)

    def launch():
        buf = R.sentinel((S, stride), "f32", "cuda")
        rc = abi["lib"].gatres_t_lin0_bwd(_p(gg), _p(xg), _p(mg), buf.data_ptr(), buf.data_ptr() + 4 * nc, S, stride, N, nc,
                                          abi[dtype], abi["stream"])
        assert rc == 0, (what, rc)
        return (buf,)
    buf, = _twice(launch, ["slabs"])
    del keep
    return buf


def _lin1_bwd(abi, g_out, x, w, N, S, nc, relu_mask, dtype, what, misaligned=()):
    """One lin1 backward: (slab buffer [S, nc + 1 + SLAB_PAD] (slab_w | slab_b | pad), g_x [N, nc]); g_x's guards are checked."""
    stride = nc + 1 + MC.SLAB_PAD
    gog, xg = R.guarded_vector(g_out, N, NAN), with_guard_rows(x, N)
    keep = None
    if "x" in misaligned:
        xg, keep = _off_by_one(xg, dtype)

    def launch():
        buf = R.sentinel((S, stride), "f32", "cuda")
        g_x = R.sentinel((N + G, nc), dtype, "cuda")
        hold = None
        if "g_x" in misaligned:
            g_x, hold = _off_by_one(g_x, dtype)
        rc = abi["lib"].gatres_t_lin1_bwd(_p(gog), _p(xg), _p(w), _p(g_x), buf.data_ptr(), buf.data_ptr() + 4 * nc, S, stride, N, nc,
                                          relu_mask, abi[dtype], abi["stream"])
        assert rc == 0, (what, rc)
        if hold is not None:
            torch.cuda.synchronize()
            assert bool(R.is_sentinel(hold[:1], dtype).all()), what + ": wrote in front of g_x"
            g_x = g_x.clone()
        return buf, g_x
    buf, g_x = _twice(launch, ["slabs", "g_x"])
    del keep
    assert bool(R.is_sentinel(g_x[N:], dtype).all()), what + ": g_x written behind row N"
    assert not bool(R.is_sentinel(g_x[:N], dtype).any()), what + ": g_x left unwritten"
    return buf, g_x[:N]


def _run_lin0_bwd_case(abi, p, N, S, nc, dtype, kernel, what, with_mask=True, misaligned=False, knobs=()):
    assert MC.lin_bwd_plan(N, S, nc, aligned=not misaligned, knobs=knobs)["kernel"] == kernel, what
    g, x = p["g"][:N], (p["x_masked"] if with_mask else p["x"])[:N]
    mask = p["mask"][:N] if with_mask else None
    buf = _lin0_bwd(abi, g, x, mask, N, S, nc, dtype, what, misaligned)
    terms = R.lin0_bwd_terms(g, x, mask)
    ratios = R.hold_slabs(buf, terms, N, S, what)
    # a slab depends on its own rows alone: the launch on them as ONE slab gives its bits
    for s, (beg, end) in enumerate(MC.slab_bounds(N, S)[1]):
        if end > beg and S > 1:
            alone = _lin0_bwd(abi, g[beg:end], x[beg:end], None if mask is None else mask[beg:end], end - beg, 1, nc, dtype,
                              what + f" slab {s} alone", misaligned)
            assert R.same_bits(alone[0, :2 * nc], buf[s, :2 * nc]), what + f": slab {s} depends on rows outside it"
    return buf, terms, ratios


def _run_lin1_bwd_case(abi, p, N, S, nc, dtype, kernel, what, relu_mask=1, misaligned=(), knobs=()):
    assert MC.lin_bwd_plan(N, S, nc, aligned=not misaligned, knobs=knobs)["kernel"] == kernel, what
    g_out, x = R.lin1_bwd_operands(p, N)
    buf, g_x = _lin1_bwd(abi, g_out, x, p["w"], N, S, nc, relu_mask, dtype, what, misaligned)
    R.hold_gx(g_x, g_out, x, p["w"], relu_mask, dtype, what)
    terms = R.lin1_bwd_terms(g_out, x)
    ratios = R.hold_slabs(buf, terms, N, S, what)
    for s, (beg, end) in enumerate(MC.slab_bounds(N, S)[1]):
        if end > beg and S > 1:
            alone, gx1 = _lin1_bwd(abi, g_out[beg:end], x[beg:end], p["w"], end - beg, 1, nc, relu_mask, dtype,
                                   what + f" slab {s} alone", misaligned)
            assert R.same_bits(alone[0, :nc + 1], buf[s, :nc + 1]), what + f": slab {s} depends on rows outside it"
            assert R.same_bits(gx1, g_x[beg:end]), what + f": g_x of slab {s} depends on rows outside it"
    return buf, terms, ratios


def _forms_agree(a, b, terms, N, S, what):
    """Two forms of one backward on the same rows: slab by slab within the sum of their two bounds."""
    off = 0
    for name, bound in R.slab_bound(terms, N, S).items():
        w = bound.shape[1]
        err = (a[:, off:off + w].double() - b[:, off:off + w].double()).abs()
        assert bool((err <= 2 * bound).all()), f"{what} {name}: the rows form and the wave form differ by more than their bounds"
        off += w


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("nc", MC.ROWS_NC)
@pytest.mark.parametrize("op", ["lin0", "lin1"])
def test_lin_bwd_rows_form_slab_by_slab(abi, op, nc, dtype):
    cases = MC.rows_cases(nc)
    rows = max(c[0] for c in cases)
    p = _cuda(R.lin0_inputs(nc, rows, dtype, 300 + nc) if op == "lin0" else R.lin1_inputs(nc, rows, dtype, 400 + nc))
    run = _run_lin0_bwd_case if op == "lin0" else _run_lin1_bwd_case
    for N, S, L, branch in cases:
        what = f"{op} bwd rows {dtype} nc={nc} N={N} S={S} (slab of {L}: {branch})"
        _record(f"{op}_bwd_rows_kernel {dtype}", run(abi, p, N, S, nc, dtype, "rows", what)[2])
    N, S, L, _ = MC.rows_null_case(nc)
    if op == "lin0":
        what = f"lin0 bwd rows {dtype} nc={nc} N={N} S={S} mask=NULL"
        _record(f"lin0_bwd_rows_kernel {dtype}", run(abi, p, N, S, nc, dtype, "rows", what, with_mask=False)[2])
    else:
        what = f"lin1 bwd rows {dtype} nc={nc} N={N} S={S} relu_mask=0"
        _record(f"lin1_bwd_rows_kernel {dtype}", run(abi, p, N, S, nc, dtype, "rows", what, relu_mask=0)[2])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("nc", MC.WAVE_BY_WIDTH)
@pytest.mark.parametrize("op", ["lin0", "lin1"])
def test_lin_bwd_wave_form_by_width(abi, op, nc, dtype):
    rows = max(n for n, _ in MC.WAVE_NS)
    p = _cuda(R.lin0_inputs(nc, rows, dtype, 500 + nc) if op == "lin0" else R.lin1_inputs(nc, rows, dtype, 600 + nc))
    run = _run_lin0_bwd_case if op == "lin0" else _run_lin1_bwd_case
    for N, S in MC.WAVE_NS:
        what = f"{op} bwd wave {dtype} nc={nc} N={N} S={S}"
        _record(f"{op}_bwd_kernel {dtype}", run(abi, p, N, S, nc, dtype, "wave", what)[2])
    N, S = MC.WAVE_NS[-1]
    if op == "lin0":
        _record(f"lin0_bwd_kernel {dtype}", run(abi, p, N, S, nc, dtype, "wave", f"lin0 bwd wave {dtype} nc={nc} mask=NULL", with_mask=False)[2])
    else:
        _record(f"lin1_bwd_kernel {dtype}", run(abi, p, N, S, nc, dtype, "wave", f"lin1 bwd wave {dtype} nc={nc} relu_mask=0", relu_mask=0)[2])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("nc", MC.WAVE_BY_SWITCH)
@pytest.mark.parametrize("op", ["lin0", "lin1"])
def test_lin_bwd_wave_form_by_switch_agrees_with_the_rows_form(abi, op, nc, dtype, monkeypatch):
    rows = max(n for n, _ in MC.WAVE_NS)
    p = _cuda(R.lin0_inputs(nc, rows, dtype, 700 + nc) if op == "lin0" else R.lin1_inputs(nc, rows, dtype, 800 + nc))
    run = _run_lin0_bwd_case if op == "lin0" else _run_lin1_bwd_case
    got = {}
    for knobs in ((), ("lin_bwd_wave",)):
        for k in knobs:
            monkeypatch.setenv(MC.KNOBS[k], "1")
        kernel = "wave" if knobs else "rows"
        for N, S in MC.WAVE_NS:
            what = f"{op} bwd {kernel} {dtype} nc={nc} N={N} S={S} knobs={knobs}"
            got[knobs, N, S] = run(abi, p, N, S, nc, dtype, kernel, what, knobs=knobs)
            _record(f"{op}_bwd_kernel {dtype}" if knobs else f"{op}_bwd_rows_kernel {dtype}", got[knobs, N, S][2])
    for N, S in MC.WAVE_NS:
        _forms_agree(got[(), N, S][0], got[("lin_bwd_wave",), N, S][0], got[(), N, S][1], N, S, f"{op} bwd {dtype} nc={nc} N={N} S={S}")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("nc", MC.WAVE_BY_POINTER)
@pytest.mark.parametrize("op,misaligned", [("lin0", ("g",)), ("lin1", ("x",)), ("lin1", ("g_x",)), ("lin1", ("x", "g_x"))])
def test_lin_bwd_with_a_misaligned_pointer_is_still_right(abi, op, misaligned, nc, dtype):
    """An activation one element off a 16-byte boundary cannot be read in 16-byte pieces: the call falls back to the wave form.
    The values are held, not which kernel ran."""
    rows = max(n for n, _ in MC.WAVE_NS)
    p = _cuda(R.lin0_inputs(nc, rows, dtype, 900 + nc) if op == "lin0" else R.lin1_inputs(nc, rows, dtype, 950 + nc))
    for N, S in MC.WAVE_NS:
        what = f"{op} bwd {dtype} nc={nc} N={N} S={S} misaligned {misaligned}"
        if op == "lin0":
            a = _run_lin0_bwd_case(abi, p, N, S, nc, dtype, "rows", what + " (aligned twin)")
            b = _run_lin0_bwd_case(abi, p, N, S, nc, dtype, "wave", what, misaligned=True)
        else:
            a = _run_lin1_bwd_case(abi, p, N, S, nc, dtype, "rows", what + " (aligned twin)")
            b = _run_lin1_bwd_case(abi, p, N, S, nc, dtype, "wave", what, misaligned=misaligned)
        _record(f"{op} bwd misaligned {dtype}", b[2])
        _forms_agree(a[0], b[0], a[1], N, S, what)


def test_lin_bwd_refusals(abi):
    N, S = 8, 2
    for nc in (0, 257):
        assert MC.lin_bwd_plan(N, S, nc)["kernel"] is None
        t = torch.ones(N, 260, device="cuda")
        buf, g_x = R.sentinel((S, 600), "f32", "cuda"), R.sentinel((N, 260), "f32", "cuda")
        lib, st = abi["lib"], abi["stream"]
        assert lib.gatres_t_lin0_bwd(_p(t), _p(t), None, _p(buf), buf.data_ptr() + 1200, S, 600, N, nc, abi["f32"], st) == MC.UNSUPPORTED
        assert lib.gatres_t_lin1_bwd(_p(t), _p(t), _p(t), _p(g_x), _p(buf), buf.data_ptr() + 1200, S, 600, N, nc, 1, abi["f32"],
                                     st) == MC.UNSUPPORTED
    assert lib.gatres_t_lin0_bwd(_p(t), _p(t), None, _p(buf), buf.data_ptr() + 1200, 0, 600, N, 8, abi["f32"], st) == MC.BADARG
    assert lib.gatres_t_lin1_bwd(_p(t), _p(t), _p(t), _p(g_x), _p(buf), buf.data_ptr() + 1200, S, 600, 0, 8, 1, abi["f32"], st) == MC.BADARG
    torch.cuda.synchronize()
    assert bool(R.is_sentinel(buf, "f32").all()) and bool(R.is_sentinel(g_x, "f32").all()), "a refused call wrote to its output"


# ---- 5. gatres_reduce_slabs ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_slabs", MC.REDUCE["num_slabs"])
def test_reduce_slabs_sums_in_slab_order_bit_for_bit(abi, num_slabs):
    for count in MC.REDUCE["count"]:
        columns = [None, 0] if count == 1 else [count // 2]
        for col in columns:
            what = f"reduce_slabs S={num_slabs} count={count} -0.0 column {col}"
            host = R.reduce_inputs(num_slabs, count, 1000 * num_slabs + count, col)
            slabs = host.cuda()

            def launch():
                out = R.sentinel((count + G,), "f32", "cuda")
                rc = abi["lib"].gatres_reduce_slabs(_p(slabs), num_slabs, count + MC.REDUCE_PAD, count, _p(out), abi["stream"])
                assert rc == 0, (what, rc)
                return (out,)
            out, = _twice(launch, ["out"])
            assert bool(R.is_sentinel(out[count:], "f32").all()), what + ": wrote behind the last parameter"
            assert R.same_bits(out[:count].cpu(), R.reduce_ref(host, count)), what
            if col is not None:
                assert int(R.bits(out[col:col + 1])) == 0, what + ": the sum of -0.0 from +0.0f is +0.0f"


def test_reduce_slabs_refusals(abi):
    slabs, out = torch.ones(4, 16, device="cuda"), R.sentinel((16,), "f32", "cuda")
    call = lambda S, stride, count: abi["lib"].gatres_reduce_slabs(_p(slabs), S, stride, count, _p(out), abi["stream"])  # noqa: E731
    assert call(4, 7, 8) == MC.BADARG and call(4, 16, 0) == MC.BADARG and call(0, 16, 8) == MC.BADARG
    torch.cuda.synchronize()
    assert bool(R.is_sentinel(out, "f32").all())


# ---- 6. the weight re-layouts -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_blocks,nc", MC.WEIGHTS)
def test_transpose_conv_weights_places_every_element(abi, num_blocks, nc):
    assert abi["lib"].gatres_param_count(num_blocks, nc) == MC.param_count(num_blocks, nc)
    host = R.weight_params(num_blocks, nc, "index")
    params, total = host.cuda(), num_blocks * 4 * nc * nc

    def launch(nb=num_blocks):
        wt = R.sentinel((G + total + G,), "f32", "cuda")
        rc = abi["lib"].gatres_transpose_conv_weights(_p(params), wt.data_ptr() + 4 * G, nb, nc, abi["stream"])
        assert rc == 0, rc
        return (wt,)
    wt, = _twice(launch, ["wt"])
    assert bool(R.is_sentinel(wt[:G], "f32").all()) and bool(R.is_sentinel(wt[G + total:], "f32").all()), "wrote outside the output"
    assert R.same_bits(wt[G:G + total].cpu(), R.transposed_layout(host, num_blocks, nc))
    none, = launch(nb=0)
    torch.cuda.synchronize()
    assert bool(R.is_sentinel(none, "f32").all()), "num_blocks == 0 wrote something"


@pytest.mark.parametrize("num_blocks,nc", MC.WEIGHTS)
def test_convert_conv_weights_bf16_places_and_rounds_every_element(abi, num_blocks, nc):
    total = num_blocks * 8 * nc * nc
    for kind in ("bf16", "random"):
        host = R.weight_params(num_blocks, nc, kind, seed=nc)
        params = host.cuda()

        def launch(nb=num_blocks):
            wb = R.sentinel((G + total + G,), "bf16", "cuda")
            rc = abi["lib"].gatres_convert_conv_weights_bf16(_p(params), wb.data_ptr() + 2 * G, nb, nc, abi["stream"])
            assert rc == 0, rc
            return (wb,)
        wb, = _twice(launch, ["wb"])
        assert bool(R.is_sentinel(wb[:G], "bf16").all()) and bool(R.is_sentinel(wb[G + total:], "bf16").all()), "wrote outside the output"
        want = R.converted_layout(host, num_blocks, nc)
        if kind == "bf16":
            assert bool((want.to(torch.bfloat16).float() == want).all())          # exact: a mismatch is a misplaced element
        assert R.same_bits(wb[G:G + total].cpu(), want.to(torch.bfloat16)), kind
        none, = launch(nb=0)
        torch.cuda.synchronize()
        assert bool(R.is_sentinel(none, "bf16").all()), "num_blocks == 0 wrote something"


# ---- 7. permute / gather ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", MC.PERMUTE_N)
def test_permute_f32_and_gather_u8(abi, N):
    host = R.permute_inputs(N, 40 + N)
    p = _cuda(host)
    perm = R.guarded_vector(p["perm"], N, 0)              # (a thread behind N would copy element 0 into the guard words)
    src, byts = R.guarded_vector(p["src"], N, NAN), R.guarded_vector(p["bytes"], N, 0xEE)
    lib, st = abi["lib"], abi["stream"]

    def permute(source, scatter):
        def launch():
            dst = R.sentinel((N + G,), "f32", "cuda")
            assert lib.gatres_permute_f32(_p(source), _p(perm), _p(dst), N, scatter, st) == 0
            return (dst,)
        dst, = _twice(launch, ["dst"])
        assert bool(R.is_sentinel(dst[N:], "f32").all()), "wrote behind element N"
        return dst
    idx = host["perm"].long()
    gathered = permute(src, 0)
    assert R.same_bits(gathered[:N].cpu(), host["src"][idx])
    inverse = torch.empty_like(host["src"])
    inverse[idx] = host["src"]
    scattered = permute(src, 1)
    assert R.same_bits(scattered[:N].cpu(), inverse)
    back = permute(R.guarded_vector(gathered[:N], N, NAN), 1)
    assert R.same_bits(back[:N].cpu(), host["src"]), "scatter after gather is not the identity"

    def launch_u8():
        dst = R.sentinel((N + G,), "u8", "cuda")
        assert lib.gatres_gather_u8(_p(byts), _p(perm), _p(dst), N, st) == 0
        return (dst,)
    dst, = _twice(launch_u8, ["dst"])
    assert bool(R.is_sentinel(dst[N:], "u8").all()) and R.same_bits(dst[:N].cpu(), host["bytes"][idx])


# ---- 8. the edge_index hash ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", MC.HASH_E)
def test_edge_index_hash_is_the_stated_sum(abi, E):
    lib, st = abi["lib"], abi["stream"]
    sent = R.SENTINEL["i64"][1]

    def device_hash(ei, start=0):
        cell = torch.tensor([sent, start, sent], dtype=torch.int64, device="cuda")
        d = ei.contiguous().cuda()
        assert lib.gatres_edge_index_hash(_p(d) if E else None, E, cell.data_ptr() + 8, st) == 0
        torch.cuda.synchronize()
        c = cell.tolist()
        assert c[0] == sent and c[2] == sent, "wrote beside hash_out"
        return c[1] & R.M64

    ei = R.edge_inputs(E, 70 + E)
    if E == 0:
        assert device_hash(ei, start=12345) == 12345          # no launch: hash_out untouched
        return
    want = R.edge_hash_ref(ei)
    assert device_hash(ei) == want and device_hash(ei) == want   # the sum is order-free: the atomics cannot change it
    moved = ei.clone()
    moved[1, E - 1] += 1                                     # one endpoint of the LAST edge
    assert device_hash(moved) == R.edge_hash_ref(moved) != want
    if E >= 2:
        swapped = ei.clone()
        swapped[:, [0, E - 1]] = ei[:, [E - 1, 0]]
        if not torch.equal(swapped, ei):
            assert device_hash(swapped) == R.edge_hash_ref(swapped) != want


def test_edge_index_hash_refusals(abi):
    cell = torch.zeros(1, dtype=torch.int64, device="cuda")
    assert abi["lib"].gatres_edge_index_hash(None, 4, _p(cell), abi["stream"]) == MC.BADARG
    assert abi["lib"].gatres_edge_index_hash(_p(cell), -1, _p(cell), abi["stream"]) == MC.BADARG
    assert abi["lib"].gatres_edge_index_hash(_p(cell), 1, None, abi["stream"]) == MC.BADARG


# ---- 9. the masked loss -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("crit", MC.CRITERIA)
@pytest.mark.parametrize("N", MC.LOSS_N)
def test_masked_loss_around_the_workgroup_and_the_four_stride_loop(abi, N, crit):
    out, y, mask = R.loss_inputs(N, 80 + N)
    o, t = R.guarded_vector(out.cuda(), N, NAN), R.guarded_vector(y.cuda(), N, NAN)
    for name, mk in (("density", mask), ("last node alone", R.last_node_mask(N))):
        what = f"masked_loss {crit} N={N} mask: {name}"
        m = R.guarded_vector(mk.cuda(), N, 1)

        def launch():
            loss, g_out = R.sentinel((1 + G,), "f32", "cuda"), R.sentinel((N + G,), "f32", "cuda")
            rc = abi["lib"].gatres_masked_loss(_p(o), _p(t), _p(m), abi["crit"][crit], _p(loss), _p(g_out), N, abi["stream"])
            assert rc == 0, (what, rc)
            return loss, g_out
        loss, g_out = _twice(launch, ["loss", "g_out"])
        assert bool(R.is_sentinel(loss[1:], "f32").all()) and bool(R.is_sentinel(g_out[N:], "f32").all()), what + ": wrote behind its outputs"
        assert not bool(R.is_sentinel(g_out[:N], "f32").any()), what + ": left g_out unwritten"
        _record(f"masked_loss_kernel {crit}", R.hold_loss(crit, loss[:1], g_out[:N], out, y, mk, table, what))
        if name != "density" and crit != "sce":           # M = 1: the tail node's gradient is 2 d or sign(d), not 0
            assert int(mk.sum()) == 1 and float(g_out[N - 1]) != 0, what + ": the last node was never visited"
