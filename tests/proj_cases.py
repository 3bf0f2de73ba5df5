"""The launch geometry of csrc/k_proj.hip (product build) restated on the host, and the shapes the dense projection kernels are run at.

``plan()`` says, for one call of gatres_t_proj_attn_fwd / gatres_t_proj_bwd_dx / gatres_t_proj_bwd_dw, which of the kernels
runs and how its rows are dealt to workgroups; tests/test_proj_turnover_host.py holds the constants below against the
literals in the source and every case table against the branch it is meant to reach, tests/test_gpu_proj_turnover.py
launches the cases.  numpy / plain Python only, no device.

Shapes are written (K, M, H): K the reduction length, M the number of outputs per row, H heads (forward only).  The data
gradient takes the same (reduction, outputs) pairs with H = 1, i.e. gatres_t_proj_bwd_dx(HC = K, K = M).  Weight-gradient
shapes are written (HC, K) as in ``slab[s][c, k] = sum_n G[n, c] X[n, k]``."""

# ---- the constants of k_proj.hip's launch code (tests/test_proj_turnover_host.py reads them back from the source) ----------------
TILE_ROWS = 16                 # rows of one wave tile
LDS_MIN_ROWS = 16384           # launch_proj: ``N >= 16384`` takes proj_lds_kernel
LDS_MAX_BYTES = 160 * 1024
LDS_GRID = 256                 # launch_proj: ``const int grid = 256``
ROWS_GRID_CAP = 256            # launch_proj_bf16: ``if (grid > 256) grid = 256`` (proj_bf16_kernel)
ROWS_TRIP = 64                 # proj_lds_kernel / proj_bf16_kernel: ``n0 += 64`` (four waves of 16 rows)
TILE_GRID_CAP = 512            # launch_proj_bf16: ``if (grid > 512) grid = 512`` (proj_bf16_tile_kernel)
TILE_TRIP = 8                  # proj_bf16_tile_kernel: ``tile += 8`` (eight waves, one tile each)
DW_STEPS = 4                   # dw_kernel: STEPS MFMA steps of 4 rows in flight
DW_CHUNK = {"dw_kernel": 4 * DW_STEPS, "dw_bf16_kernel": 32, "dw2d_bf16_kernel": 64}    # rows per trip of the slab loop
DW2D_MAX_WGS = 1024            # launch_dw_bf16: ``num_slabs * OB <= 1024 && num_slabs <= 128``
DW2D_MAX_SLABS = 128
DW2D_RENUMBER = 8              # dw2d_bf16_kernel: ``(groups & 7) == 0`` deals the workgroups of a row group to one XCD

# The switches the cases set.  Only switches the PRODUCT library reads belong here (csrc/k_misc.hip read_knobs, outside its
# GATRES_DIAG_BUILD block): GATRES_DW_FP32, which would send wide bf16 tables to dw_kernel, is read by the diagnostic build
# alone -- in the library under test it is always 0, so dw_kernel sees bf16 storage only at the narrow shapes and that case
# is not in the tables.
KNOBS = {"no_proj_lds": "GATRES_NO_PROJ_LDS", "dw_1d": "GATRES_DW_1D"}


def cdiv(a, b):
    return -(-a // b)


def roundup(a, b):
    return cdiv(a, b) * b


def slab_bounds(N, S):
    """``nodes_per_slab`` of every parameter-gradient kernel, roundup4(ceil(N / S)), and the rows [beg, end) of each slab;
    slabs behind the last row are empty (beg >= end is written as (N, N))."""
    nps = roundup(cdiv(N, S), 4)
    return nps, [(min(N, s * nps), min(N, (s + 1) * nps)) for s in range(S)]


def plan(kind, dtype, N, K, M, H=1, S=1, knobs=()):
    """kind: "fwd" | "dx" | "dw"; dtype: "f32" | "bf16"; for "dw" (K, M) = (K, HC).  Returns a dict with ``kernel`` (None:
    the call is refused with GATRES_E_UNSUPPORTED), ``grid`` and
      proj_kernel                         ``wgs``: rows [r0, r1) per workgroup (four wave tiles of 16 rows)
      proj_lds_kernel / proj_bf16_kernel  ``rows_per_wg`` and ``wgs``; a workgroup walks its rows in trips of 64
      proj_bf16_tile_kernel               ``shares``: row tiles [t_lo, t_hi) per workgroup, walked in trips of 8
      dw kernels                          ``nps``, ``slabs`` (rows [beg, end) per slab), ``chunk``, ``renumber``."""
    assert kind in ("fwd", "dx", "dw") and dtype in ("f32", "bf16") and N >= 1 and set(knobs) <= set(KNOBS)
    if kind == "dw":
        return _plan_dw(dtype, N, K, M, S, knobs)
    if kind == "dx":
        assert H == 1
    if dtype == "f32":
        wide = K % 16 == 0 and M % 16 == 0 and K * M >= 64 * 128 and (M * (K + 4) + 2 * M) * 4 <= LDS_MAX_BYTES
        if wide and N >= LDS_MIN_ROWS and "no_proj_lds" not in knobs:
            rows = roundup(cdiv(N, LDS_GRID), ROWS_TRIP)
            return _rows_plan("proj_lds_kernel", N, rows)
        grid = cdiv(cdiv(N, TILE_ROWS), 4)
        return {"kernel": "proj_kernel", "grid": grid, "wgs": [(b * 64, min(N, b * 64 + 64)) for b in range(grid)]}
    C = M // H
    if K % 32 == 0 and M % 128 == 0 and M <= 256 and (kind == "dx" or C in (128, 64, 32)):
        ntiles = cdiv(N, TILE_ROWS)
        grid = min(TILE_GRID_CAP, cdiv(ntiles, TILE_TRIP))
        return {"kernel": "proj_bf16_tile_kernel", "grid": grid, "ntiles": ntiles,
                "shares": [(ntiles * b // grid, ntiles * (b + 1) // grid) for b in range(grid)]}
    if K % 32 == 0 and M % 32 == 0 and H in (1, 2, 4):
        grid = min(ROWS_GRID_CAP, cdiv(N, ROWS_TRIP))
        rows = max(ROWS_TRIP, roundup(cdiv(N, grid), ROWS_TRIP))
        return _rows_plan("proj_bf16_kernel", N, rows)
    return {"kernel": None}


def _rows_plan(kernel, N, rows):
    grid = cdiv(N, rows)
    return {"kernel": kernel, "grid": grid, "rows_per_wg": rows, "wgs": [(b * rows, min(N, (b + 1) * rows)) for b in range(grid)]}


def trips(p):
    """Trips of the longest-running workgroup's row loop (rows kernels: 64 rows per trip; tile kernel: 8 tiles per trip)."""
    if p["kernel"] == "proj_bf16_tile_kernel":
        return max(cdiv(hi - lo, TILE_TRIP) for lo, hi in p["shares"])
    if p["kernel"] in ("proj_lds_kernel", "proj_bf16_kernel"):
        return max(cdiv(r1 - r0, ROWS_TRIP) for r0, r1 in p["wgs"])
    return 1


def _plan_dw(dtype, N, K, HC, S, knobs):
    nps, slabs = slab_bounds(N, S)
    out = {"nps": nps, "slabs": slabs, "renumber": False}
    if dtype == "bf16" and K >= 32 and HC >= 32:
        if HC % 64 == 0 and K % 64 == 0:
            OB = (HC // 64) * (K // 64)
            if S * OB <= DW2D_MAX_WGS and S <= DW2D_MAX_SLABS and "dw_1d" not in knobs:
                out.update(kernel="dw2d_bf16_kernel", grid=S * OB, renumber=S % DW2D_RENUMBER == 0)
        if "kernel" not in out:
            tiles = (HC // 16) * (K // 16)
            ok = HC % 16 == 0 and K % 16 == 0 and tiles >= 4 and tiles % 4 == 0 and (HC + K) * 80 <= LDS_MAX_BYTES
            out.update(kernel="dw_bf16_kernel" if ok else None, grid=S)
    else:
        CB = 64 if HC >= 64 else max(16, HC)
        KB = 64 if K >= 64 else max(16, K)
        out.update(kernel="dw_kernel", grid=cdiv(S * cdiv(HC, CB) * cdiv(K, KB), 4))
    if out["kernel"]:
        out["chunk"] = DW_CHUNK[out["kernel"]]
    return out


# ---- the case tables ----------------------------------------------------------------------------------------------------------------
# fp32 proj_kernel: every (K, M) family of the dispatch table's narrow end and both wide ones below the LDS threshold.  N = 1 / 17 / 65:
# one row, one row into the second wave tile, one row into the second workgroup.  The two narrowest shapes carry the M % 16 != 0 guards
# and the KQ = 1 and 2 load paths, so they also take the sizes either side of a tile and a workgroup, and five workgroups.
PROJ_F32 = {
    "shapes": [(4, 8, 2), (8, 4, 1), (8, 16, 2), (32, 64, 2), (64, 32, 1), (128, 256, 2), (256, 128, 1)],
    "N": [1, 17, 65],
    "narrow": [(4, 8, 2), (8, 4, 1)],
    "N_narrow": [15, 16, 63, 64, 257],
    "N_all_epilogues": 65,
}
# fp32 proj_lds_kernel: 16383 is the last size of proj_kernel; 16384 gives 256 workgroups of exactly one trip; at 16385 the rows per
# workgroup double and the last workgroup owns ONE row; at 16449 it owns 65, its second trip holds one row (every prefetched row index is
# clamped to it); 33000 gives 192 rows per workgroup: three trips, the last workgroup ragged.
PROJ_LDS = {
    "shapes": [(64, 128, 2), (128, 64, 1), (128, 256, 2), (256, 128, 1)],
    "N": [16383, 16384, 16385, 16449, 33000],
    "N_all_epilogues": 16449,
    "N_equal": [16384, 16385, 16449],
}
# bf16 proj_bf16_tile_kernel: 127 / 128 / 129 rows are 8 tiles with a ragged last one, 8 full tiles, 9 tiles in two workgroups; the grid
# cap binds past 65536 rows: at 65537 exactly one workgroup takes a ninth tile (its second trip) and that tile holds one row; at 65589
# four workgroups do and the last tile holds five rows.
PROJ_BF16_TILE = {
    "shapes": [(64, 128, 2), (128, 256, 2), (256, 128, 1)],
    "N": [1, 127, 128, 129, 65536, 65537, 65589],
    "N_all_epilogues": 65537,
}
# bf16 proj_bf16_kernel: one workgroup of one trip up to 64 rows, a second workgroup of one row at 65; 16384 is the last size with 64 rows
# per workgroup, 16385 doubles them (second trip, last workgroup of one row), 16449 leaves 65 rows to the last one, 40000 gives three trips.
PROJ_BF16_ROWS = {
    "shapes": [(32, 64, 2), (64, 32, 1), (128, 64, 1)],
    "N": [1, 63, 64, 65, 16384, 16385, 16449, 40000],
    "N_all_epilogues": 16449,
}
# dW.  (5, 7): slabs of 4 rows, five of the seven empty; (15, 1) / (17, 1): one row short of and one row past dw_kernel's 16-row trip;
# (67, 2), (130, 3): slabs of 36 / 44 rows end inside a trip; (12416, 194), (8300, 129): more slabs than the 2-D form takes.
DW_F32 = {
    "shapes": [(8, 4), (4, 8), (16, 8), (64, 32), (256, 128)],
    "bf16_shapes": [(32, 16), (16, 32)],               # bf16 storage too narrow for the bf16 matrix-core kernels
    "NS": [(1, 1), (5, 7), (15, 1), (17, 1), (67, 2), (130, 3), (1007, 7), (12416, 194)],
}
DW_BF16 = {
    "shapes": [(64, 32), (32, 64)],
    "wide_shapes": [(128, 64), (256, 128)],              # reach dw_bf16_kernel at S = 129 and under GATRES_DW_1D=1
    "NS": [(1, 1), (31, 1), (32, 1), (33, 1), (65, 1), (5, 7), (130, 3), (1007, 8), (8300, 129)],
    "NS_wide": [(8300, 129)],
}
DW2D_BF16 = {
    "shapes": [(128, 64), (64, 128), (256, 128), (128, 256)],
    "NS": [(1, 1), (63, 1), (64, 1), (65, 1), (129, 1), (5, 7), (1007, 3), (1007, 8), (1007, 16), (12416, 64), (9000, 128)],
}
# conv_param_grads (k_conv_grads.h: the attention-vector / bias column sums of a convolution's backward) cuts its rows into the SAME
# slabs; (H, C) from one lane group of columns to all 256, at the three (N, S) with empty slabs and slabs that end inside a trip.
CONV_GRADS = {
    "shapes": [(2, 4), (1, 64), (2, 128)],
    "NS": [(5, 7), (67, 2), (130, 3)],
}

GUARD_ROWS = 16                # rows behind row N: sentinels in outputs, NaN in inputs
SLAB_PAD = 8                   # slab_stride = HC * K + SLAB_PAD
OPERANDS = [(True, True), (True, False), (False, True), (False, False)]       # dX: (residual, ReLU mask)


def zero_rows(N):
    """Rows of relu_ref that carry planted signed zeros: the first, the last, the first of the last 16-row tile."""
    return sorted({0, N - 1, TILE_ROWS * ((N - 1) // TILE_ROWS)})


def zero_cols(M):
    """(columns planted with +0.0, columns planted with -0.0)."""
    return [0, M - 2], [1, M - 1]


def proj_cases(table):
    """[(shape, [N, ...])] of a projection table."""
    out = []
    for shape in table["shapes"]:
        sizes = list(table["N"])
        if shape in table.get("narrow", ()):
            sizes += table["N_narrow"]
        out.append((shape, sizes))
    return out


def dw_cases():
    """[(kernel, dtype, (HC, K), knobs, [(N, S), ...])]: every weight-gradient launch of the tables."""
    out = []
    for s in DW_F32["shapes"]:
        out.append(("dw_kernel", "f32", s, (), DW_F32["NS"]))
    for s in DW_F32["bf16_shapes"]:
        out.append(("dw_kernel", "bf16", s, (), DW_F32["NS"]))
    for s in DW_BF16["shapes"]:
        out.append(("dw_bf16_kernel", "bf16", s, (), DW_BF16["NS"]))
    for s in DW_BF16["wide_shapes"]:
        out.append(("dw_bf16_kernel", "bf16", s, (), DW_BF16["NS_wide"]))
        out.append(("dw_bf16_kernel", "bf16", s, ("dw_1d",), DW_BF16["NS"]))
    for s in DW2D_BF16["shapes"]:
        out.append(("dw2d_bf16_kernel", "bf16", s, (), DW2D_BF16["NS"]))
    return out
