"""tests/misc_cases.py and tests/misc_refs.py against the kernel source, on the host.

tests/test_gpu_misc_turnover.py runs the small kernels of csrc/k_misc.hip at sizes chosen to lie just past a row lane, an unrolled
trip, a workgroup.  Those sizes are only as good as the constants they were chosen against: this module reads the literals from
the source and asserts that misc_cases.py restates them and that every case still reaches the branch it names.  It also holds
float32 restatements of every sum, taken in another order than the kernel's, to the bounds of misc_refs.py, and shows that the
same checks reject planted faults: one dropped row, a slab boundary moved by one row, two swapped columns, one slab left out of
the reduction, a transposed index pair, a hash that skips the last edge.  No GPU, no kernel launches."""
import os
import re

import numpy as np
import pytest
import torch

import misc_cases as MC
import misc_refs as R
from proj_cases import slab_bounds
from proj_refs import U32, hold
from test_gpu_criterion import table
from test_proj_turnover_host import body_of, one, rejected

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "gnn-pressure-estimation_amd", "csrc", "k_misc.hip")) as _f:
    SRC = _f.read()


def kernel(name):
    return body_of(SRC, "void " + name + "(", "\n}\n")


def launcher(name):
    return body_of(SRC, 'extern "C" int ' + name + "(", "\n}\n")


# ---- 1. the literals ----------------------------------------------------------------------------------------------------------------
def test_cases_restate_the_literals_of_k_misc():
    assert "int nps = (N + num_slabs - 1) / num_slabs;\n  return (nps + 3) & ~3;" in SRC
    for name in ("lin0_bwd_rows_kernel", "lin1_bwd_rows_kernel"):
        k = kernel(name)
        assert "G4 = 1 << lgG4" in k and one(r"R = (\d+) >> lgG4", k) == str(MC.WG)
        assert one(r"for \(; n \+ (\d+) \* R < nend; n \+= (\d+) \* R\)", k) == (str(MC.ROWS_UNROLL - 1), str(MC.ROWS_UNROLL))
        assert "int n = nbeg + r;" in k and "for (; n < nend; n += R)" in k and "nend = min(N, nbeg + nps)" in k
        assert one(r"__launch_bounds__\((\d+)\) void " + name, SRC) == str(MC.WG)
    for name in ("lin0_bwd_kernel", "lin1_bwd_kernel"):
        k = kernel(name)
        assert set(re.findall(r"lane \+ (\d+) \* cc", k)) == {str(MC.WAVE)} and set(re.findall(r"cc < (\d+)", k)) == {str(MC.WAVE_COLS)}
        assert one(r"__launch_bounds__\((\d+)\) void " + name, SRC) == str(MC.WAVE)
        assert "for (int n = nbeg; n < nend; ++n)" in k
    assert MC.WAVE * MC.WAVE_COLS == MC.LIN_MAX_NC
    form = body_of(SRC, "static inline bool lin_rows_form(", "\n}\n")
    assert "return nc >= 4 && nc <= %d && gatres_is_pow2(nc) && gatres_aligned16(act) && !gatres_knobs()->lin_bwd_wave;" % MC.LIN_MAX_NC in form
    for name, act in (("gatres_t_lin0_bwd", "lin_rows_form(nc, g)"), ("gatres_t_lin1_bwd", "lin_rows_form(nc, x) && gatres_aligned16(g_x)")):
        ln = launcher(name)
        assert act in ln and "if (nc < 1 || nc > %d) return GATRES_E_UNSUPPORTED;" % MC.LIN_MAX_NC in ln
        assert "dim3(num_slabs), dim3(%d)" % MC.WG in ln and "dim3(num_slabs), dim3(%d)" % MC.WAVE in ln and "ilog2_(nc / 4)" in ln
    knobs = body_of(SRC, "void read_knobs(", "\n}\n").split("#ifdef GATRES_DIAG_BUILD")[0]
    for field, env in MC.KNOBS.items():
        assert re.search(r'k->%s = env_flag\("%s"\)' % (field, env), knobs), env
    # forward
    assert "if (nc < 4 || nc % 4) return GATRES_E_UNSUPPORTED;" in launcher("gatres_t_lin0_fwd")
    l1 = launcher("gatres_t_lin1_fwd")
    assert "if (nc < 4 || !gatres_is_pow2(nc) || nc > %d) return GATRES_E_UNSUPPORTED;" % MC.LIN_MAX_NC in l1 and "const int G = nc / 4;" in l1
    k = kernel("lin1_fwd_kernel")
    assert "if (!valid) row = N - 1;" in k and "for (int off = G >> 1; off > 0; off >>= 1)" in k
    assert one(r"blockIdx.x \* (\d+) \+ threadIdx.x", k) == str(MC.WG)
    # the reducer, the loss, the hash
    k = kernel("reduce_slabs_kernel")
    assert one(r"for \(; s \+ (\d+) <= num_slabs; s \+= (\d+)\)", k) == (str(MC.REDUCE_UNROLL),) * 2 and "float acc = 0.f;" in k
    k = kernel("masked_loss_kernel")
    assert one(r"for \(; n \+ (\d+) \* (\d+) < N; n \+= (\d+) \* (\d+)\)", k) == (
        str(MC.LOSS_STRIDES - 1), str(MC.LOSS_THREADS), str(MC.LOSS_STRIDES), str(MC.LOSS_THREADS))
    assert one(r"for \(int off = (\d+); off > 0; off >>= 1\)", k) == str(MC.LOSS_THREADS // 2) and 2 ** 10 == MC.LOSS_THREADS
    assert launcher("gatres_masked_loss").count("dim3(1), dim3(%d)" % MC.LOSS_THREADS) == 3
    k = kernel("edge_hash_kernel")
    assert "0x%XULL * (uint64_t)(e + 1)" % R.GOLDEN in k and "ei[E + e] + 0x%XULL" % R.HASH_DST in k
    # the flat parameter vector
    for name in ("transpose_conv_weights_kernel", "convert_conv_weights_bf16_kernel"):
        k = kernel(name)
        assert "2LL * nc + (long long)b * (9LL * nc + 4LL * nc * nc)" in k and "6LL * nc : 6LL * nc + per + 3LL * nc" in k
    assert MC.param_count(15, 32) == 65857 and MC.conv_weight_offsets(2, 8)[1] == (16 + 328 + 48, 16 + 328 + 48 + 128 + 24)
    with open(os.path.join(ROOT, "gnn-pressure-estimation_amd", "_build.py")) as f:
        assert '"-ffp-contract=off"' in f.read()              # lin0 forward is held bit for bit to a product and a sum


def test_the_header_states_the_widths_these_launchers_take():
    with open(os.path.join(ROOT, "include", "gatres.h")) as f:
        hdr = f.read()
    assert "4 <= nc <= 128  (gatres_small" not in hdr
    for phrase in ("any multiple of 4", "a power of two, 4 <= nc <= 256", "1 <= nc <= 256"):
        assert phrase in hdr, phrase


# ---- 2. every case lands where it claims --------------------------------------------------------------------------------------------
def test_forward_cases_reach_their_lanes_and_ragged_ends():
    plans = {(nc, N): MC.lin0_fwd_plan(N, nc) for nc in MC.LIN0_FWD["nc"] for N in MC.LIN0_FWD["N"]}
    assert all(plans.values()) and MC.lin0_fwd_plan(8, MC.LIN0_FWD["refused_nc"]) is None
    assert plans[4, 1] == {"grid": 1, "idle": 255, "pow2": True} and plans[4, 1001]["grid"] > 1
    assert {nc for (nc, _), p in plans.items() if not p["pow2"]} == {12, 200}                    # multiples of 4, no power of two
    assert all(p["idle"] > 0 for p in plans.values())                                             # a ragged last workgroup everywhere
    plans = {(nc, N): MC.lin1_fwd_plan(N, nc) for nc in MC.LIN1_FWD["nc"] for N in MC.LIN1_FWD["N"]}
    assert all(plans.values()) and all(MC.lin1_fwd_plan(8, nc) is None for nc in MC.LIN1_FWD["refused_nc"])
    assert plans[4, 1]["shuffles"] == 0 and plans[4, 1]["G"] == 1                                 # one lane per row: no shuffle
    assert plans[256, 1]["G"] == MC.WAVE and plans[256, 1]["shuffles"] == 6                        # a row is a whole wave
    for nc in MC.LIN1_FWD["nc"]:
        assert plans[nc, 1]["grid"] == 1 and plans[nc, 1]["clamped"] == MC.WG - nc // 4          # below one workgroup
        assert any(plans[nc, N]["clamped"] > 0 and plans[nc, N]["grid"] > 1 for N in MC.LIN1_FWD["N"]) or nc == 4
        assert any(plans[nc, N]["grid"] > 1 for N in MC.LIN1_FWD["N"])
    assert plans[4, 1000]["clamped"] == 24 and plans[4, 1000]["grid"] == 4


def test_rows_cases_reach_the_branches_they_name():
    assert MC.ROWS_NC == [4, 8, 32, 128, 256]
    for nc in MC.ROWS_NC:
        G4, R = MC.rows_geometry(nc)
        assert G4 * 4 == nc and G4 * R == MC.WG
        cases = MC.rows_cases(nc)
        assert [c[2] for c in cases[:-1]] == [1, R - 1, R, 3 * R, 3 * R + 1, 4 * R, 4 * R + 1, 7 * R + 2]
        for N, S, L, branch in cases:
            p = MC.lin_bwd_plan(N, S, nc)
            assert p["kernel"] == "rows" and p["R"] == R
            lens = [e - b for b, e in p["slabs"]]
            assert L in lens, (nc, N, S, L)
            assert lens[-1] < lens[0] and sum(lens) == N                         # the last slab is shorter
            if L % 4 == 0 and S == 3:
                assert lens[0] == lens[1] == L                                   # a full slab has that length
            trips = [MC.lane_trips(L, R, r) for r in range(R)]
            if "shorter than the R row lanes" in branch:
                assert L == 1 and trips[0] == (0, 1) and all(t == (0, 0) for t in trips[1:])
            elif "without a row" in branch:
                assert trips[R - 1] == (0, 0) and all(t == (0, 1) for t in trips[:R - 1])
            elif "one row per lane" in branch:
                assert all(t == (0, 1) for t in trips)
            elif "not entered" in branch:
                assert all(t == (0, 3) for t in trips)
            elif "lane 0 alone enters" in branch:
                assert trips[0] == (1, 0) and all(t == (0, 3) for t in trips[1:]) and p["unrolled_lanes"][lens.index(L)] == 1
            elif "no tail" in branch:
                assert all(t == (1, 0) for t in trips)
            elif "tail row behind" in branch:
                assert trips[0] == (1, 1) and all(t == (1, 0) for t in trips[1:])
            elif "second unrolled trip" in branch:
                assert trips[0] == trips[1] == (2, 0) and all(t == (1, 3) for t in trips[2:])
            else:
                assert "empty" in branch and lens.count(0) == 5 and p["behind"] >= 2
        assert MC.rows_null_case(nc)[2] == 4 * R + 1
    assert MC.lane_trips(0, 4, 0) == (0, 0)


def test_wave_cases_reach_the_wave_form_three_ways():
    for nc in MC.WAVE_BY_WIDTH:
        assert not MC.lin_rows_form(nc) and all(MC.lin_bwd_plan(N, S, nc)["kernel"] == "wave" for N, S in MC.WAVE_NS)
    assert {MC.lin_bwd_plan(8, 1, nc)["column_trips"] for nc in MC.WAVE_BY_WIDTH} == {1, 2, 4}
    assert 24 in MC.WAVE_BY_WIDTH and 24 % 4 == 0 and not MC.is_pow2(24)
    for nc in MC.WAVE_BY_SWITCH + MC.WAVE_BY_POINTER:
        assert MC.lin_bwd_plan(8, 1, nc)["kernel"] == "rows"
    for nc in MC.WAVE_BY_SWITCH:
        assert MC.lin_bwd_plan(8, 1, nc, knobs=("lin_bwd_wave",))["kernel"] == "wave"
    for nc in MC.WAVE_BY_POINTER:
        assert MC.lin_bwd_plan(8, 1, nc, aligned=False)["kernel"] == "wave"
    assert MC.lin_bwd_plan(8, 1, 0)["kernel"] is None and MC.lin_bwd_plan(8, 1, 257)["kernel"] is None
    plans = [MC.lin_bwd_plan(N, S, 24) for N, S in MC.WAVE_NS]
    assert any(p["behind"] >= 2 for p in plans) and any(len(p["slabs"]) == 1 for p in plans)
    assert any(0 < p["slabs"][-1][1] - p["slabs"][-1][0] < p["nps"] for p in plans if len(p["slabs"]) > 1)


def test_the_other_cases_reach_their_trips():
    r = {S: MC.reduce_plan(S, 1) for S in MC.REDUCE["num_slabs"]}
    assert [(r[S]["unrolled"], r[S]["tail"]) for S in (1, 7, 8, 9, 16, 17)] == [(0, 1), (0, 7), (1, 0), (1, 1), (2, 0), (2, 1)]
    assert {MC.reduce_plan(1, c)["grid"] for c in MC.REDUCE["count"]} == {1, 2, 4} and MC.reduce_plan(1, 256)["idle"] == 0
    assert [MC.grid_plan(N)["grid"] for N in MC.PERMUTE_N] == [1, 1, 1, 2, 4] and MC.grid_plan(257)["idle"] == 255
    assert MC.HASH_E[0] == 0 and {63, 64, 65, 256, 257} <= set(MC.HASH_E)        # either side of a wave and of a workgroup
    lp = {N: MC.loss_plan(N) for N in MC.LOSS_N}
    assert lp[1]["busy"] == 1 and lp[1023]["busy"] == 1023 and lp[1024]["busy"] == lp[1025]["busy"] == 1024
    assert (lp[1024]["unrolled"], lp[1024]["tail"]) == (0, 1) and (lp[1025]["unrolled"], lp[1025]["tail"]) == (0, 2)
    assert lp[3072]["unrolled_threads"] == 0 and (lp[3072]["unrolled"], lp[3072]["tail"]) == (0, 3)
    assert lp[3073]["unrolled_threads"] == 1 and (lp[3073]["unrolled"], lp[3073]["tail"]) == (1, 0)
    assert lp[4096]["unrolled_threads"] == 1024 and lp[4097]["tail"] == 1
    assert lp[7169]["unrolled"] == 2 and MC.loss_plan(7168)["unrolled"] == 1
    assert all(nb * 8 * nc * nc < 2 ** 31 for nb, nc in MC.WEIGHTS) and (1, 128) in MC.WEIGHTS and (3, 4) in MC.WEIGHTS
    assert len(MC.describe()) > 100


# ---- 3. float32 restatements in another order stay inside the bounds; planted faults do not ---------------------------------------
def _f32_slabs(terms, N, S, stride, boundaries=None, drop=None, swap=None):
    """A slab buffer as a correct kernel would leave it, each sum taken in float32 from the LAST row to the first (the kernels
    go forward, lane by lane).  ``boundaries``: other slab rows; ``drop``: a row left out; ``swap``: two columns of the first
    output exchanged."""
    rows = boundaries or slab_bounds(N, S)[1]
    buf = R.sentinel((S, stride), "f32")
    for s, (b, e) in enumerate(rows):
        off = 0
        for k, t in enumerate(terms.values()):
            acc = np.zeros(t.shape[1], dtype=np.float32)
            for n in range(e - 1, b - 1, -1):
                if n != drop:
                    acc = (acc + t[n].numpy().astype(np.float32)).astype(np.float32)
            if swap and k == 0:
                acc[list(swap)] = acc[list(swap)[::-1]]
            buf[s, off:off + t.shape[1]] = torch.from_numpy(acc)
            off += t.shape[1]
    return buf


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("op", ["lin0", "lin1"])
def test_the_slab_checker_accepts_another_order_and_rejects_planted_faults(op, dtype):
    nc, N, S = 8, 130, 4
    if op == "lin0":
        p = R.lin0_inputs(nc, N, dtype, 3)
        terms = R.lin0_bwd_terms(p["g"], p["x_masked"], p["mask"])
    else:
        p = R.lin1_inputs(nc, N, dtype, 4)
        g_out, x = R.lin1_bwd_operands(p, N)
        assert int((g_out.abs() == 2).sum()) == 2 and int(((x != 0) & (x.float().abs() < 2.0 ** -126)).sum()) == 2
        terms = R.lin1_bwd_terms(g_out, x)
    used = sum(t.shape[1] for t in terms.values())
    stride = used + MC.SLAB_PAD
    nps, rows = slab_bounds(N, S)
    assert nps == 36 and rows[-1] == (108, 130)
    right = _f32_slabs(terms, N, S, stride)
    ratios = R.hold_slabs(right, terms, N, S)
    assert all(0 <= r <= 1 for r in ratios.values()) and max(ratios.values()) > 0
    # one dropped row (an unmasked one, of a slab's last trip)
    row = next(n for n in range(71, 36, -1) if float(terms["slab_w"][n].abs().min()) > 1e-3)
    assert rejected(R.hold_slabs, _f32_slabs(terms, N, S, stride, drop=row), terms, N, S)
    # the boundary between slabs 0 and 1 moved by ONE row: the sum of the slabs is unchanged, the slabs are not
    moved = _f32_slabs(terms, N, S, stride, boundaries=[(0, 37), (37, 72)] + rows[2:])
    whole = {k: (t.sum(0), 2 * nps * U32 * t.abs().sum(0)) for k, t in terms.items()}
    assert hold(moved[:, :terms["slab_w"].shape[1]].double().sum(0), *whole["slab_w"], "sum") <= 1
    assert rejected(R.hold_slabs, moved, terms, N, S)
    # two swapped columns of the weight sums
    assert rejected(R.hold_slabs, _f32_slabs(terms, N, S, stride, swap=(2, 5)), terms, N, S)
    # an empty slab left unwritten, one with something in it, a pad word written, -0.0 in an empty slab
    n2, s2 = 5, 7
    t2 = {k: t[:n2] for k, t in terms.items()}
    right2 = _f32_slabs(t2, n2, s2, stride)
    assert max(R.hold_slabs(right2, t2, n2, s2).values()) <= 1 and bool((R.bits(right2[2:, :used]) == 0).all())
    for edit in (lambda b: b[6, :used].copy_(R.sentinel((used,), "f32")), lambda b: b[3, 1].fill_(1e-30),
                 lambda b: b[1, used + 2].fill_(0.0), lambda b: b[4, 0].fill_(-0.0)):
        wrong = right2.clone()
        edit(wrong)
        assert rejected(R.hold_slabs, wrong, t2, n2, s2)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_lin1_forward_bound_and_the_bitwise_references(dtype):
    for nc in (4, 32, 256):
        N = 65
        p = R.lin1_inputs(nc, N, dtype, nc)
        x, w = p["x"].float().numpy(), p["w"].numpy()
        acc = np.zeros(N, dtype=np.float32)
        for c in range(nc - 1, -1, -1):                                # last column first, products rounded: no fused multiply-add
            acc = (acc + (x[:, c] * w[c]).astype(np.float32)).astype(np.float32)
        out = torch.from_numpy((acc + p["b"].numpy()[0]).astype(np.float32))
        assert 0 < R.hold_lin1_fwd(out, p["x"], p["w"], p["b"])["out"] <= 1
        assert R.hold_lin1_fwd(torch.from_numpy(acc), p["x"], p["w"], None)["out"] <= 1
        assert rejected(R.hold_lin1_fwd, out, p["x"], p["w"], None)                          # the bias matters
        wrong = p["x"].clone()
        wrong[:, [0, nc - 1]] = p["x"][:, [nc - 1, 0]]                 # two swapped columns
        ref, _ = R.lin1_fwd_reference(wrong, p["w"], p["b"])
        assert rejected(R.hold_lin1_fwd, ref.float(), p["x"], p["w"], p["b"])
        clamp = out.clone()
        clamp[N - 1] = out[N - 2]                                      # the last row computed from its neighbour
        assert rejected(R.hold_lin1_fwd, clamp, p["x"], p["w"], p["b"])
    # lin0 forward / lin1 g_x: the references are two roundings and one, a fused multiply-add differs somewhere
    q = R.lin0_inputs(32, 1001, dtype, 9)
    ref = R.lin0_fwd_ref(q["x_masked"], q["mask"], q["w"], q["b"], "f32")
    assert not bool(torch.isnan(ref).any()) and bool((ref[q["mask"] != 0] == q["b"]).all())
    fused = (q["x"].double()[:, None] * q["w"].double() + q["b"].double()).float()
    assert not R.same_bits(R.lin0_fwd_ref(q["x"], None, q["w"], q["b"], "f32"), fused)
    l1 = R.lin1_inputs(8, 9, dtype, 2)
    x = R.plant_relu(l1["x"].clone())
    assert int((x == 0).sum()) >= 2 and bool(torch.signbit(x[x == 0]).any()) and int(((x < 0) & (x.float().abs() < 1e-38)).sum()) >= 1
    gx = R.lin1_gx_ref(l1["g_out"], x, l1["w"], 1, dtype)
    R.hold_gx(gx, l1["g_out"], x, l1["w"], 1, dtype)
    assert bool((gx[~(x > 0)] == 0).all()) and rejected(R.hold_gx, R.lin1_gx_ref(l1["g_out"], x, l1["w"], 0, dtype), l1["g_out"], x, l1["w"], 1, dtype)
    ge = R.lin1_gx_ref(l1["g_out"], torch.where(x == 0, torch.ones_like(x), x), l1["w"], 1, dtype)      # the mask as x >= 0
    assert rejected(R.hold_gx, ge, l1["g_out"], x, l1["w"], 1, dtype)


def test_reduce_reference_order_and_a_slab_left_out():
    S, count = 17, 257
    slabs = R.reduce_inputs(S, count, 5, minus_zero_column=100)
    ref = R.reduce_ref(slabs, count)
    assert int(R.bits(ref[100:101])) == 0 and not bool(torch.isnan(ref).any())
    exact = slabs[:, :count].double().sum(0)
    A = slabs[:, :count].double().abs().sum(0)
    assert hold(ref, exact, S * U32 * A, "slab order") <= 1
    backwards = R.reduce_ref(slabs.flip(0), count)
    assert hold(backwards, exact, S * U32 * A, "reverse order") <= 1 and not R.same_bits(backwards, ref)      # the order shows in the bits
    for s in (0, 8, 16):                                               # the first, the first behind an unrolled trip, the last
        assert not R.same_bits(R.reduce_ref(slabs, count, skip=(s,)), ref)
    assert int(R.bits(R.reduce_ref(torch.full((3, 1 + MC.REDUCE_PAD), -0.0), 1))) == 0


def test_weight_layouts_and_a_transposed_index_pair():
    for nb, nc in MC.WEIGHTS:
        per = 2 * nc * nc
        idx = R.weight_params(nb, nc, "index")
        assert idx.numel() == MC.param_count(nb, nc) < 2 ** 24
        t = R.transposed_layout(idx, nb, nc)
        assert t.numel() == nb * 2 * per and t.unique().numel() == t.numel()
        o1, o2 = MC.conv_weight_offsets(nb, nc)[-1]
        blk = (nb - 1) * 2 * per
        assert float(t[blk + 1 * 2 * nc + 3 % (2 * nc)]) == o1 + (3 % (2 * nc)) * nc + 1          # W1^T[1, 3] = W1[3, 1]
        assert float(t[blk + per + 2 * nc + 1]) == o2 + 1 * 2 * nc + 2                             # W2^T[2, 1] = W2[1, 2]
        assert not torch.equal(R.transposed_layout(idx, nb, nc, swap=(1, 2)), t)                   # one transposed index pair
        b = R.weight_params(nb, nc, "bf16")
        c = R.converted_layout(b, nb, nc)
        assert c.numel() == nb * 4 * per and bool((c.to(torch.bfloat16).float() == c).all()) and not bool(torch.isnan(c).any())
        assert int(torch.isnan(b).sum()) == b.numel() - nb * 2 * per
        W1, W2 = R.conv_weights(b, nb, nc)[0]
        assert bool((W1 > 0).all()) and bool((W2 < 0).all())
        distinct = c[:2 * per].unique().numel()
        assert distinct == 2 * per if nc < 128 else distinct == 2 * R.BF16_NORMALS
        assert torch.equal(c[2 * per:3 * per].view(nc, 2 * nc), W1.t()) and torch.equal(c[3 * per:4 * per].view(2 * nc, nc), W2.t())
    big = R.conv_weights(R.weight_params(1, 128, "bf16"), 1, 128)[0][0].reshape(-1)
    assert float(big[0]) == 2.0 ** -126 and bool(torch.isfinite(big).all()) and float(big[R.BF16_NORMALS]) == float(big[0])
    r = R.converted_layout(R.weight_params(1, 4, "random", 1), 1, 4)
    assert not bool((r.to(torch.bfloat16).float() == r).all())                                     # the second input rounds


def test_hash_reference_and_a_hash_that_skips_the_last_edge():
    assert R.edge_hash_ref(torch.zeros(2, 0, dtype=torch.int64)) == 0
    one_edge = torch.tensor([[3], [9]])
    assert R.edge_hash_ref(one_edge) == R.mix64(R.mix64(3 + R.GOLDEN) ^ (9 + R.HASH_DST))
    for E in MC.HASH_E[1:]:
        ei = R.edge_inputs(E, E)
        h = R.edge_hash_ref(ei)
        assert 0 <= h <= R.M64 and R.edge_hash_ref(ei, skip_last=True) != h
        moved = ei.clone()
        moved[1, E - 1] += 1
        assert R.edge_hash_ref(moved) != h and R.edge_hash_ref(moved, skip_last=True) == R.edge_hash_ref(ei, skip_last=True)
        if E >= 2 and not torch.equal(ei[:, 0], ei[:, E - 1]):
            sw = ei.clone()
            sw[:, [0, E - 1]] = ei[:, [E - 1, 0]]
            assert R.edge_hash_ref(sw) != h
    big = R.edge_inputs(64, 1)
    assert int(big.max()) > 2 ** 40


def test_permute_inputs_carry_payloads_and_minus_zero():
    for N in MC.PERMUTE_N:
        p = R.permute_inputs(N, N)
        assert sorted(p["perm"].tolist()) == list(range(N)) and int(p["bytes"].max()) < 100 < R.SENTINEL["u8"][1]
        if N >= 255:
            b = R.bits(p["src"])
            assert int(torch.isnan(p["src"]).sum()) == 2 and int((b == -2 ** 31).sum()) == 1
            assert not bool(R.is_sentinel(p["src"], "f32").any())
    s = R.sentinel((3, 4), "bf16")
    assert bool(torch.isnan(s).all()) and bool(torch.isnan(R.sentinel((2,), "f32")).all()) and bool(R.is_sentinel(s, "bf16").all())


@pytest.mark.parametrize("crit", MC.CRITERIA)
def test_loss_bounds_accept_float32_sums_and_reject_a_tail_never_visited(crit):
    for N in (1, 1025, 4097, 7169):
        out, y, mask = R.loss_inputs(N, N)
        l64, g64 = table(crit, out, y, mask)
        M = int(mask.sum())
        assert M >= 1 and float(l64) >= 0
        # float32: the gradient of the table rounded, the loss summed in another order
        terms = {"mse": lambda d: d * d, "mae": np.abs}.get(crit)
        if terms is None:
            o, t = out.double(), y.double()
            oh, yh = o / o.abs().clamp_min(1e-12), t / t.abs().clamp_min(1e-12)
            vals = ((1 - oh * yh) ** 3).float().numpy()
        else:
            vals = terms((out - y).numpy().astype(np.float32)).astype(np.float32)
        # (the bound is that of 1024 partial sums and a 10-level tree: the restatement keeps that depth, not the order -- each
        #  partial sum runs from its last node to its first, the tree adds NEIGHBOURS where the kernel's halves the array)
        part = np.zeros(MC.LOSS_THREADS, dtype=np.float32)
        for n in range(N - 1, -1, -1):
            if mask[n]:
                part[n % MC.LOSS_THREADS] = np.float32(part[n % MC.LOSS_THREADS] + vals[n])
        while part.size > 1:
            part = (part[0::2] + part[1::2]).astype(np.float32)
        loss = torch.tensor([part[0] / np.float32(M)], dtype=torch.float32)
        g = g64.float()
        r = R.hold_loss(crit, loss, g, out, y, mask, table)
        assert r["loss"] <= 1 and r["g_out"] <= 1
        if N >= 1023 and crit == "sce":
            assert float(g64.abs().max()) > 1e8 and float(g64[N - 2]) != 0
        # a tail that is never visited: the last node alone in the mask, the kernel sees no masked node at all
        last = R.last_node_mask(N)
        l1, g1 = table(crit, out, y, last)
        if float(l1) != 0:
            assert rejected(R.hold_loss, crit, torch.tensor([float("nan")]), torch.zeros(N), out, y, last, table)
            assert rejected(R.hold_loss, crit, torch.zeros(1), g1.float(), out, y, last, table)
        wrong = g.clone()
        off = int((mask == 0).nonzero()[0]) if M < N else None
        if off is not None:
            wrong[off] = 1e-30
            assert rejected(R.hold_loss, crit, loss, wrong, out, y, mask, table)
