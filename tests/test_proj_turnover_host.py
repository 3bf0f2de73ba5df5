"""tests/proj_cases.py and tests/proj_refs.py against the kernel source, on the host.

tests/test_gpu_proj_turnover.py runs csrc/k_proj.hip at sizes chosen to lie just past a workgroup's first trip, a grid cap, a
slab's last full chunk.  Those sizes are only as good as the constants they were chosen against: this module reads the literals
from the source and asserts that ``plan()`` restates them and that every case table still reaches the branch it names, so that
retuning a constant fails here -- and says which case has to move -- instead of the device tests quietly going back to one
trip.  It also shows that the checker bites (six wrong results built from the float64 reference are each rejected, the
noisy-but-right one passes) and that torch's own CPU products stay inside the bounds.  No GPU, no kernel launches."""
import os
import re

import pytest
import torch

import proj_cases as PC
import proj_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "gnn-pressure-estimation_amd", "csrc", "k_proj.hip")) as _f:
    SRC = _f.read()


def body(start, end):
    """The source between the first occurrence of ``start`` and the next occurrence of ``end`` behind it."""
    a = SRC.index(start)
    return SRC[a:SRC.index(end, a + len(start))]


def body_of(text, start, end):
    a = text.index(start)
    return text[a:text.index(end, a + len(start))]


def one(pattern, text):
    found = re.findall(pattern, text)
    assert len(found) == 1, (pattern, found)
    return found[0]


# ---- 1. the literals ----------------------------------------------------------------------------------------------------------------
def test_plan_restates_the_literals_of_the_launch_code():
    launch_f32 = body("int launch_proj(", "\n}\n")
    assert int(one(r"N >= (\d+) && !gatres_knobs\(\)->no_proj_lds", launch_f32)) == PC.LDS_MIN_ROWS
    assert int(one(r"const int grid = (\d+);", launch_f32)) == PC.LDS_GRID
    assert "rows = (rows + 63) & ~63;" in launch_f32 and "K * M >= 64 * 128" in launch_f32
    assert one(r"<= (\d+) \* 1024\)", launch_f32) == str(PC.LDS_MAX_BYTES // 1024)
    launch_bf16 = SRC[SRC.index("int launch_proj_bf16("):SRC.index("int launch_proj(")]
    tile, rows = launch_bf16.split("proj_bf16_tile_kernel<K, M, H, EPI>), dim3(grid)")
    tile = tile[tile.index("#endif"):]                                     # (behind the diagnostic build's streaming kernel)
    assert one(r"if \(grid > (\d+)\) grid = (\d+);", tile) == (str(PC.TILE_GRID_CAP),) * 2
    assert "int grid = (ntiles + 7) / 8;" in tile and PC.TILE_TRIP == 8
    assert one(r"if \(grid > (\d+)\) grid = (\d+);", rows) == (str(PC.ROWS_GRID_CAP),) * 2
    assert "int grid = (N + 63) / 64;" in rows and "rows = (rows + 63) & ~63;" in rows and "if (rows < 64) rows = 64;" in rows
    # the trips of the row loops
    tile_kernel = body("void proj_bf16_tile_kernel(", "\n}\n")
    assert one(r"tile \+= (\d+)\)", tile_kernel) == str(PC.TILE_TRIP) and "if (!first) load_x(tile, xf);" in tile_kernel
    for name in ("void proj_lds_kernel(", "void proj_bf16_kernel("):
        k = body(name, "\n}\n")
        assert one(r"n0 \+= (\d+)\)", k) == str(PC.ROWS_TRIP), name
        assert one(r"if \(n0 \+ (\d+) < r1\)", k) == str(PC.ROWS_TRIP) and "r1 - 1)" in k, name
    # the weight gradient: the slab length, the chunk of each kernel's slab loop, the switch between the two bf16 forms
    assert SRC.count("= (nps + 3) & ~3;") == 3 and "npg = (npg + 3) & ~3;" in SRC
    dw = body("void dw_kernel(", "\n}\n")
    assert int(one(r"constexpr int STEPS = (\d+);", dw)) == PC.DW_STEPS and "nb += 4 * STEPS" in dw
    assert PC.DW_CHUNK["dw_kernel"] == 4 * PC.DW_STEPS == 16
    dw1 = body("void dw_bf16_kernel(", "\n}\n")
    assert int(one(r"n0 < nend; n0 \+= (\d+)\)", dw1)) == PC.DW_CHUNK["dw_bf16_kernel"] == 32
    assert one(r"if \(n0 \+ (\d+) < nend\)", dw1) == "32"
    dw2 = body("void dw2d_bf16_kernel(", "\n}\n")
    assert int(one(r"CH = (\d+);", dw2)) == PC.DW_CHUNK["dw2d_bf16_kernel"] == 64 and "n0 < nend; n0 += CH)" in dw2
    assert one(r"if \(\(groups & (\d+)\) == 0\)", dw2) == str(PC.DW2D_RENUMBER - 1)
    limits = one(r"num_slabs \* OB <= (\d+) && num_slabs <= (\d+) && !gatres_knobs\(\)->dw_1d", SRC)
    assert limits == (str(PC.DW2D_MAX_WGS), str(PC.DW2D_MAX_SLABS))
    assert "K_ >= 32 && M_ >= 32 && !gatres_knobs()->dw_fp32" in SRC


def test_every_switch_the_cases_set_is_read_by_the_product_build():
    """A switch that only the diagnostic build reads is 0 in the library under test whatever the environment says: a case
    that sets it would pass plan() and run another kernel.  GATRES_DW_FP32 is such a switch, which is why the tables hold
    no wide bf16 shape for dw_kernel."""
    with open(os.path.join(ROOT, "gnn-pressure-estimation_amd", "csrc", "k_misc.hip")) as f:
        knobs = body_of(f.read(), "void read_knobs(", "\n}\n")
    product, diag = knobs.split("#ifdef GATRES_DIAG_BUILD")
    for field, env in PC.KNOBS.items():
        assert re.search(r'k->%s = env_\w+\("%s"' % (field, env), product), env
        assert "gatres_knobs()->" + field in SRC, field
    assert 'env_flag("GATRES_DW_FP32")' in diag and "GATRES_DW_FP32" not in product and "k->dw_fp32 = 0;" in product
    wide_bf16 = [c for c in PC.dw_cases() if c[0] == "dw_kernel" and c[1] == "bf16" and min(c[2]) >= 32]
    assert not wide_bf16 and "dw_fp32" not in PC.KNOBS


def test_plan_by_hand():
    p = PC.plan("fwd", "bf16", 65537, 64, 128, 2)
    assert p["kernel"] == "proj_bf16_tile_kernel" and p["grid"] == 512 and p["ntiles"] == 4097 and p["shares"][-1] == (4088, 4097)
    assert [hi - lo for lo, hi in p["shares"]].count(9) == 1
    p = PC.plan("fwd", "f32", 16449, 128, 64, 1)
    assert (p["kernel"], p["grid"], p["rows_per_wg"], p["wgs"][-1]) == ("proj_lds_kernel", 129, 128, (16384, 16449))
    assert PC.plan("fwd", "f32", 16449, 128, 64, 1, knobs=("no_proj_lds",))["kernel"] == "proj_kernel"
    assert PC.plan("fwd", "f32", 33000, 32, 64, 2)["kernel"] == "proj_kernel"                   # too narrow for the LDS copy of W
    p = PC.plan("dx", "bf16", 40000, 128, 64)
    assert (p["kernel"], p["grid"], p["rows_per_wg"]) == ("proj_bf16_kernel", 209, 192)
    assert PC.plan("fwd", "bf16", 100, 16, 32, 2)["kernel"] is None
    p = PC.plan("dw", "bf16", 1007, 64, 128, S=8)
    assert (p["kernel"], p["grid"], p["nps"], p["renumber"], p["slabs"][-1]) == ("dw2d_bf16_kernel", 16, 128, True, (896, 1007))
    assert PC.plan("dw", "bf16", 8300, 64, 128, S=129)["kernel"] == "dw_bf16_kernel"
    p = PC.plan("dw", "bf16", 9000, 128, 256, S=128)                                            # on both limits: 128 slabs x 8 blocks
    assert (p["kernel"], p["grid"]) == ("dw2d_bf16_kernel", PC.DW2D_MAX_WGS)
    assert PC.plan("dw", "bf16", 1007, 16, 32, S=8)["kernel"] == "dw_kernel" and PC.plan("dw", "f32", 1007, 64, 128, S=8)["kernel"] == "dw_kernel"
    p = PC.plan("dw", "f32", 5, 4, 8, S=7)
    assert p["nps"] == 4 and p["slabs"] == [(0, 4), (4, 5)] + [(5, 5)] * 5 and p["grid"] == 2


# ---- 2. every case lands where it claims --------------------------------------------------------------------------------------------
def _plans(table, dtype, kinds=("fwd", "dx")):
    for (K, M, H), sizes in PC.proj_cases(table):
        for kind in kinds:
            for N in sizes:
                yield (K, M, H), kind, N, PC.plan(kind, dtype, N, K, M, H if kind == "fwd" else 1)


def test_projection_cases_reach_their_kernels_trips_and_ragged_ends():
    for shape, kind, N, p in _plans(PC.PROJ_F32, "f32"):
        assert p["kernel"] == "proj_kernel", (shape, N)
    assert {N for _, _, N, p in _plans(PC.PROJ_F32, "f32") if p["grid"] > 1} >= {65, 257}
    for shape in PC.PROJ_F32["narrow"]:
        assert shape[1] % 16 != 0 and shape[0] // 4 in (1, 2) and shape in PC.PROJ_F32["shapes"]      # M guards, KQ = 1 / 2
    assert {s[0] // 4 for s in PC.PROJ_F32["narrow"]} == {1, 2}

    seen = {}
    for shape, kind, N, p in _plans(PC.PROJ_LDS, "f32"):
        assert p["kernel"] == ("proj_lds_kernel" if N >= PC.LDS_MIN_ROWS else "proj_kernel"), (shape, N)
        seen[N] = p
    assert min(PC.PROJ_LDS["N"]) == PC.LDS_MIN_ROWS - 1 and PC.LDS_MIN_ROWS in PC.PROJ_LDS["N"]
    assert PC.trips(seen[16384]) == 1 and seen[16384]["grid"] == PC.LDS_GRID
    assert PC.trips(seen[16385]) == 2 and seen[16385]["wgs"][-1] == (16384, 16385)                     # a last workgroup of one row
    assert seen[16449]["wgs"][-1][1] - seen[16449]["wgs"][-1][0] == PC.ROWS_TRIP + 1                   # a second trip of one row
    assert PC.trips(seen[33000]) == 3 and (seen[33000]["wgs"][-1][1] - seen[33000]["wgs"][-1][0]) % 16 != 0
    assert set(PC.PROJ_LDS["N_equal"]) <= set(PC.PROJ_LDS["N"]) and PC.PROJ_LDS["N_all_epilogues"] in PC.PROJ_LDS["N"]

    seen = {}
    for shape, kind, N, p in _plans(PC.PROJ_BF16_TILE, "bf16"):
        assert p["kernel"] == "proj_bf16_tile_kernel", (shape, kind, N)
        assert p["shares"][0][0] == 0 and p["shares"][-1][1] == p["ntiles"]
        assert all(a[1] == b[0] for a, b in zip(p["shares"], p["shares"][1:]))
        seen[N] = p
    assert seen[128]["grid"] == 1 and seen[129]["grid"] == 2 and seen[127]["ntiles"] == 8
    assert seen[65536]["grid"] == PC.TILE_GRID_CAP and PC.trips(seen[65536]) == 1                       # the cap binds, one trip still
    nine = [b for b, (lo, hi) in enumerate(seen[65537]["shares"]) if hi - lo > PC.TILE_TRIP]
    assert nine == [PC.TILE_GRID_CAP - 1] and 65537 % 16 == 1                                           # ONE second trip, of one row
    assert sum(hi - lo > PC.TILE_TRIP for lo, hi in seen[65589]["shares"]) == 4 and 65589 % 16 == 5
    assert 65589 * 256 * 2 < 34 << 20                                                                   # (the largest table: 33 MB)

    seen = {}
    for shape, kind, N, p in _plans(PC.PROJ_BF16_ROWS, "bf16"):
        assert p["kernel"] == "proj_bf16_kernel", (shape, kind, N)
        seen[N] = p
    assert seen[64]["grid"] == 1 and seen[65]["wgs"] == [(0, 64), (64, 65)]
    assert seen[16384]["grid"] == PC.ROWS_GRID_CAP and PC.trips(seen[16384]) == 1
    assert PC.trips(seen[16385]) == 2 and seen[16385]["wgs"][-1] == (16384, 16385)
    assert seen[16449]["wgs"][-1] == (16384, 16449) and PC.trips(seen[40000]) == 3
    for table in (PC.PROJ_F32, PC.PROJ_LDS, PC.PROJ_BF16_TILE, PC.PROJ_BF16_ROWS):
        assert table["N_all_epilogues"] in table["N"]
    assert len(PC.OPERANDS) == 4 and PC.OPERANDS[0] == (True, True) and len(set(PC.OPERANDS)) == 4


def test_weight_gradient_cases_reach_their_kernels_empty_slabs_and_mid_chunk_ends():
    reached = {}
    for kernel, dtype, (HC, K), knobs, cases in PC.dw_cases():
        for N, S in cases:
            p = PC.plan("dw", dtype, N, K, HC, S=S, knobs=knobs)
            assert p["kernel"] == kernel, (kernel, dtype, HC, K, knobs, N, S)
            assert p["slabs"][0][0] == 0 and max(e for _, e in p["slabs"]) == N and p["nps"] % 4 == 0
            r = reached.setdefault(kernel, {"empty": 0, "mid": 0, "renumber": set(), "dtypes": set(), "trips": set()})
            r["empty"] += any(b >= e for b, e in p["slabs"])
            r["mid"] += any(e > b and (e - b) % p["chunk"] for b, e in p["slabs"][:-1]) or (S == 1 and N % p["chunk"] != 0)
            r["renumber"].add(p["renumber"])
            r["dtypes"].add(dtype)
            r["trips"].add(min(3, PC.cdiv(p["slabs"][0][1], p["chunk"])))
    assert set(reached) == {"dw_kernel", "dw_bf16_kernel", "dw2d_bf16_kernel"}
    for kernel, r in reached.items():
        assert r["empty"] >= 1 and r["mid"] >= 1 and r["trips"] == {1, 2, 3}, kernel
    assert reached["dw2d_bf16_kernel"]["renumber"] == {False, True} and reached["dw_kernel"]["dtypes"] == {"f32", "bf16"}
    renumbered = {S for _, S in PC.DW2D_BF16["NS"] if S % PC.DW2D_RENUMBER == 0}
    assert renumbered == {8, 16, 64, 128} and (1007, 3) in PC.DW2D_BF16["NS"]
    assert PC.plan("dw", "f32", 5, 4, 8, S=7)["slabs"].count((5, 5)) == 5                                # five of seven slabs empty
    # either side of each kernel's first trip with one slab
    for table, chunk in ((PC.DW_F32, 16), (PC.DW_BF16, 32), (PC.DW2D_BF16, 64)):
        one_slab = {N for N, S in table["NS"] if S == 1}
        assert {chunk - 1, chunk + 1} <= one_slab and 1 in one_slab, chunk


def test_conv_grad_cases_share_the_slab_bounds_and_the_checker_rejects_an_unwritten_slab():
    with open(os.path.join(ROOT, "gnn-pressure-estimation_amd", "csrc", "k_misc.hip")) as f:
        misc = f.read()
    assert "int nps = (N + num_slabs - 1) / num_slabs;\n  return (nps + 3) & ~3;" in misc
    assert any(b >= e for N, S in PC.CONV_GRADS["NS"] for b, e in PC.slab_bounds(N, S)[1])
    assert all(H * C <= 256 and C % 2 == 0 for H, C in PC.CONV_GRADS["shapes"]) and (2, 128) in PC.CONV_GRADS["shapes"]
    H, C, N, S = 2, 4, 5, 7
    p = R.conv_grad_inputs(H, C, N, "f32", 3)
    nps, rows = PC.slab_bounds(N, S)
    slabs = torch.full((S, 3 * H * C + PC.SLAB_PAD), float("nan"))
    gs, gd = p["g_a_src"].repeat_interleave(C, dim=1), p["g_a_dst"].repeat_interleave(C, dim=1)
    for s, (b, e) in enumerate(rows):
        slabs[s, :3 * H * C] = torch.cat([(gs[b:e] * p["h"][b:e]).sum(0), (gd[b:e] * p["h"][b:e]).sum(0), p["g_out"][b:e].sum(0)])
    args = (p["h"], p["g_a_src"], p["g_a_dst"], p["g_out"], N, S, H)
    assert max(R.hold_conv_grads(slabs, *args).values()) < 1
    moved = slabs.clone()                                           # row 3 counted in slab 1 instead of slab 0: the sums agree
    row3 = torch.cat([gs[3] * p["h"][3], gd[3] * p["h"][3], p["g_out"][3]])
    moved[0, :3 * H * C] -= row3
    moved[1, :3 * H * C] += row3
    assert rejected(R.hold_conv_grads, moved, *args)
    left = slabs.clone()
    left[4, :3 * H * C] = float("nan")
    assert rejected(R.hold_conv_grads, left, *args)


def test_planted_zeros_are_where_the_tables_say():
    for N, M in ((1, 4), (17, 8), (65537, 128)):
        ref = R.plant_zeros(torch.ones(N, M))
        plus, minus = PC.zero_cols(M)
        rows = PC.zero_rows(N)
        assert set(rows) >= {0, N - 1, 16 * ((N - 1) // 16)} and not set(plus) & set(minus)
        zero = ref == 0
        assert int(zero.sum()) == len(rows) * (len(set(plus)) + len(set(minus)))
        assert not torch.signbit(ref[rows][:, plus]).any() and torch.signbit(ref[rows][:, minus]).all()
        assert not (ref > 0)[rows][:, plus + minus].any()


# ---- 3. the checker bites -----------------------------------------------------------------------------------------------------------
def rejected(fn, *a, **k):
    with pytest.raises(AssertionError):
        fn(*a, **k)
    return True


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_the_projection_checker_rejects_wrong_results_and_passes_a_noisy_right_one(dtype):
    K, M, H, N = 64, 128, 2, 129 + 64
    p = R.fwd_inputs(K, M, N, dtype, 5)
    X, W = p["X"], p["W"]
    ref, A = R.product(X, W)
    C = M // H

    def logits(h64, att):
        return (h64.view(N, H, C) * att.double().view(1, H, C)).sum(-1).float()
    right = R.noisy(ref, A, dtype, 6)
    args = (X, W, p["att_src"], p["att_dst"], H, dtype)
    ratios = R.hold_fwd(right, logits(ref, p["att_src"]), logits(ref, p["att_dst"]), *args)
    assert 0 < ratios["h"] < 1 and ratios["a_src"] < 0.1
    # the last tile of the first workgroup's share left at zero (the tile kernel's shares at this size)
    share = PC.plan("fwd", "bf16", N, K, M, H)["shares"][0]
    wrong = right.clone()
    wrong[16 * (share[1] - 1):16 * share[1]] = 0
    assert rejected(R.hold_fwd, wrong, logits(ref, p["att_src"]), logits(ref, p["att_dst"]), *args)
    # rows n and n + 64 swapped (a row computed from the fragment prefetched for the next trip)
    wrong = right.clone()
    wrong[[5, 69]] = right[[69, 5]]
    assert rejected(R.hold_fwd, wrong, logits(ref, p["att_src"]), logits(ref, p["att_dst"]), *args)
    # ... in the logits alone
    s = logits(ref, p["att_src"])
    s[[5, 69]] = s[[69, 5]]
    assert rejected(R.hold_fwd, right, s, logits(ref, p["att_dst"]), *args)
    # one k step of 32 dropped: on nearly every output
    short, _ = R.product(X[:, :32], W[:, :32])
    wrong = R.noisy(short, A, dtype, 7)
    assert rejected(R.hold_fwd, wrong, logits(ref, p["att_src"]), logits(ref, p["att_dst"]), *args)
    bound = 2 * K * R.U32 * A + (R.UB * ref.abs() if dtype == "bf16" else 0)
    assert float(((wrong.double() - ref).abs() > bound).double().mean()) > 0.98
    # the data gradient: the mask skipped at -0.0 only
    d = R.dx_inputs(K, M, N, dtype, 8)
    relu = R.plant_zeros(d["relu_ref"].clone())
    full, bnd, keep = R.dx_reference(d["X"], d["W"], d["resid"], None, dtype)
    masked, _, _ = R.dx_reference(d["X"], d["W"], d["resid"], relu, dtype)
    _, Adx = R.product(d["X"], d["W"])
    Adx = Adx + d["resid"].double().abs()
    right = R.noisy(masked, Adx * (relu > 0), dtype, 9)
    assert 0 < R.hold_dx(right, d["X"], d["W"], d["resid"], relu, dtype)["g_x"] < 1
    wrong = right.clone()
    minus_zero = (relu == 0) & torch.signbit(relu)
    assert int(minus_zero.sum()) == 2 * len(PC.zero_rows(N))
    wrong[minus_zero] = R.noisy(full, Adx, dtype, 9)[minus_zero]
    assert rejected(R.hold_dx, wrong, d["X"], d["W"], d["resid"], relu, dtype)
    assert rejected(R.hold_dx, R.noisy(full, Adx, dtype, 9), d["X"], d["W"], d["resid"], relu, dtype)      # no mask at all
    assert rejected(R.hold_dx, right, d["X"], d["W"], None, relu, dtype)                                     # the residual matters
    nan = right.clone()
    nan[N - 1, 3] = float("nan")
    assert rejected(R.hold_dx, nan, d["X"], d["W"], d["resid"], relu, dtype)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_the_slab_checker_rejects_a_moved_boundary_and_an_unwritten_slab(dtype):
    HC, K, N, S = 64, 32, 130, 4
    p = R.dw_inputs(HC, K, N, dtype, 11)
    G, X = p["G"], p["X"]
    nps, rows = PC.slab_bounds(N, S)
    assert nps == 36 and rows[-1] == (108, 130)

    def slabs_of(bounds, seed=12):
        out = torch.full((len(bounds), HC * K + PC.SLAB_PAD), float("nan"))
        for s, (b, e) in enumerate(bounds):
            ref, A = R.product(G[b:e].t(), X[b:e].t())
            out[s, :HC * K] = R.noisy(ref, A, "f32", seed + s).reshape(-1)
        return out
    right = slabs_of(rows)
    r = R.hold_dw(right, G, X, N, S)
    assert 0 < r["slab"] < 1 and 0 < r["sum"] < 1
    # the boundary between slabs 0 and 1 off by 4 rows: the sum is unchanged, the slabs are not
    moved = slabs_of([(0, 40), (40, 72)] + rows[2:])
    whole, Aw = R.product(G.t(), X.t())
    assert R.hold(moved[:, :HC * K].double().sum(0).view(HC, K), whole, 2 * nps * R.U32 * Aw, "sum") < 1
    assert rejected(R.hold_dw, moved, G, X, N, S)
    # an empty slab left unwritten; pad words written; an empty slab with something in it
    n2, s2 = 5, 7
    rows2 = PC.slab_bounds(n2, s2)[1]
    right2 = slabs_of(rows2)
    assert (right2[2:, :HC * K] == 0).all() and R.hold_dw(right2, G[:n2], X[:n2], n2, s2)["slab"] < 1
    left = right2.clone()
    left[6, :HC * K] = float("nan")
    assert rejected(R.hold_dw, left, G[:n2], X[:n2], n2, s2)
    stale = right2.clone()
    stale[3, 17] = 1e-30
    assert rejected(R.hold_dw, stale, G[:n2], X[:n2], n2, s2)
    pad = right.clone()
    pad[1, HC * K + 2] = 0.0
    assert rejected(R.hold_dw, pad, G, X, N, S)


# ---- 4. the bounds hold on torch's own products -------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,M,H", [(4, 8, 2), (64, 128, 2), (256, 128, 1)])
def test_cpu_products_stay_inside_the_bounds(K, M, H):
    N = 257
    for dtype in ("f32", "bf16"):
        p = R.fwd_inputs(K, M, N, dtype, K + M)
        X, W = p["X"], p["W"]
        h = X @ W.t()                                                    # torch's CPU product in the storage type
        acc = X.float() @ W.float().t()
        C = M // H
        a = [(acc.view(N, H, C) * p[k].view(1, H, C)).sum(-1) for k in ("att_src", "att_dst")]
        r = R.hold_fwd(h, a[0], a[1], X, W, p["att_src"], p["att_dst"], H, dtype)
        assert 0 < r["h"] <= 1 and r["a_src"] <= 1 and r["a_dst"] <= 1
        d = R.dx_inputs(K, M, N, dtype, K + M + 1)
        relu = R.plant_zeros(d["relu_ref"].clone())
        g = ((d["X"].float() @ d["W"].float().t() + d["resid"].float()) * (relu > 0)).to(R.TORCH_DTYPE[dtype])
        assert R.hold_dx(g, d["X"], d["W"], d["resid"], relu, dtype)["g_x"] <= 1
    w = R.dw_inputs(M, K, 1007, "f32", 3)
    nps, rows = PC.slab_bounds(1007, 8)
    slabs = torch.full((8, M * K + PC.SLAB_PAD), float("nan"))
    for s, (b, e) in enumerate(rows):
        slabs[s, :M * K] = (w["G"][b:e].t() @ w["X"][b:e]).reshape(-1)
    assert R.hold_dw(slabs, w["G"], w["X"], 1007, 8)["slab"] <= 1
