"""The launch geometry of csrc/k_misc.hip's small per-op kernels restated on the host, and the sizes they are run at.

lin0 / lin1 forward, their backward in both forms (256 threads per slab for a power-of-two width, one wave per slab otherwise),
the slab reducer, the two weight re-layouts, the node relabelling copies, the edge_index hash and the masked loss.  Each case
table names the branch a size is meant to reach; tests/test_misc_turnover_host.py holds the constants below against the
literals in the source and every case against ``*_plan()``, tests/test_gpu_misc_turnover.py launches the cases.  Plain Python
only, no device.  (conv_param_grads and the slab bounds are in tests/proj_cases.py; adam_kernel in tests/adam_ref.py.)"""
from proj_cases import cdiv, roundup, slab_bounds

# ---- the constants of k_misc.hip (tests/test_misc_turnover_host.py reads them back from the source) --------------------------------
WG = 256                       # threads of every kernel here but the wave forms and the loss
LIN_MAX_NC = 256               # lin1 forward and both backward launchers: ``nc > 256`` is refused
ROWS_UNROLL = 4                # rows form: ``n + 3 * R < nend; n += 4 * R``
WAVE = 64                      # wave form: one wave per slab, columns ``lane + 64 * cc``
WAVE_COLS = 4                  # ... ``cc < 4``
REDUCE_UNROLL = 8              # reduce_slabs_kernel: ``s + 8 <= num_slabs; s += 8``
LOSS_THREADS = 1024            # masked_loss_kernel: one workgroup
LOSS_STRIDES = 4               # ... ``n + 3 * 1024 < N; n += 4 * 1024``
KNOBS = {"lin_bwd_wave": "GATRES_LIN_BWD_WAVE"}
BADARG, UNSUPPORTED = -1, -2

GUARD_ROWS = 16                # rows behind row N: sentinels in outputs, NaN in inputs (as tests/proj_cases.py)
SLAB_PAD = 8                   # sentinel words behind a slab's sums
REDUCE_PAD = 5                 # gatres_reduce_slabs cases: slab_stride = count + 5


def is_pow2(v):
    return v > 0 and v & (v - 1) == 0


# ---- forward ------------------------------------------------------------------------------------------------------------------------
def lin0_fwd_plan(N, nc):
    """One thread per (row, four columns).  None: refused (GATRES_E_UNSUPPORTED)."""
    if nc < 4 or nc % 4:
        return None
    threads = N * (nc // 4)
    return {"grid": cdiv(threads, WG), "idle": cdiv(threads, WG) * WG - threads, "pow2": is_pow2(nc)}


def lin1_fwd_plan(N, nc):
    """G = nc / 4 lanes per row; lanes behind the last row are clamped to row N - 1 (they take part in the shuffles)."""
    if nc < 4 or not is_pow2(nc) or nc > LIN_MAX_NC:
        return None
    G = nc // 4
    grid = cdiv(N * G, WG)
    return {"G": G, "shuffles": G.bit_length() - 1, "grid": grid, "clamped": grid * WG - N * G}


# ---- backward -----------------------------------------------------------------------------------------------------------------------
def rows_geometry(nc):
    """(G4 lanes per row, R rows per trip) of the rows form."""
    G4 = nc // 4
    return G4, WG // G4


def lin_rows_form(nc, aligned=True, knobs=()):
    return 4 <= nc <= LIN_MAX_NC and is_pow2(nc) and aligned and "lin_bwd_wave" not in knobs


def lane_trips(L, R, r):
    """Row lane r of a slab of L rows: (trips of the unrolled loop, trips of the tail loop behind it)."""
    n, unrolled = r, 0
    while n + (ROWS_UNROLL - 1) * R < L:
        n += ROWS_UNROLL * R
        unrolled += 1
    return unrolled, (cdiv(L - n, R) if n < L else 0)


def lin_bwd_plan(N, S, nc, aligned=True, knobs=()):
    """``kernel`` "rows" | "wave" | None (refused), ``nps``, ``slabs`` (rows [beg, end) per slab, (N, N) when empty), ``behind``
    (slabs whose first row lies behind row N: ``nbeg > N``) and for the rows form ``R`` and per slab the lanes in the unrolled loop."""
    if nc < 1 or nc > LIN_MAX_NC:
        return {"kernel": None}
    nps, slabs = slab_bounds(N, S)
    out = {"nps": nps, "slabs": slabs, "behind": sum(s * nps > N for s in range(S))}
    if lin_rows_form(nc, aligned, knobs):
        G4, R = rows_geometry(nc)
        out.update(kernel="rows", G4=G4, R=R,
                   unrolled_lanes=[sum(lane_trips(e - b, R, r)[0] > 0 for r in range(R)) for b, e in slabs])
    else:
        out.update(kernel="wave", column_trips=cdiv(nc, WAVE))
    return out


def _rows_case(L):
    """(N, S) with a slab of exactly L rows.  A slab that is not the last one holds nps rows, a multiple of four: such an L is the
    length of the two full slabs in front of a shorter one; any other L is the length of the last slab behind two of roundup4(L)."""
    if L % 4 == 0:
        return 3 * L - 3, 3
    return 2 * roundup(L, 4) + L, 3


def rows_cases(nc):
    """[(N, S, L, branch)] of the rows form at width nc: the slab lengths around the R row lanes and the four-trip loop."""
    _, R = rows_geometry(nc)
    table = [(1, "a slab shorter than the R row lanes: lane 0 alone has a row"),
             (R - 1, "one row lane without a row"),
             (R, "one row per lane, tail loop only"),
             (3 * R, "three tail trips, the unrolled loop is not entered"),
             (3 * R + 1, "row lane 0 alone enters the unrolled loop"),
             (4 * R, "one unrolled trip on every lane, no tail"),
             (4 * R + 1, "lane 0 takes a tail row behind its unrolled trip"),
             (7 * R + 2, "lanes 0 and 1 take a second unrolled trip, the others three tail rows")]
    out = [_rows_case(L) + (L, branch) for L, branch in table]
    out.append((5, 7, 4, "five of seven slabs empty, each with its first row behind row N"))
    return out


ROWS_NC = [4, 8, 32, 128, 256]


def rows_null_case(nc):
    """The case repeated with mask == NULL (lin0) and relu_mask == 0 (lin1): the slab of 4R + 1 rows."""
    _, R = rows_geometry(nc)
    return next(c for c in rows_cases(nc) if c[2] == 4 * R + 1)


WAVE_NS = [(1, 1), (5, 7), (67, 2), (130, 3)]              # one row; empty slabs; slabs of 36 and 44 rows with a shorter last one
WAVE_BY_WIDTH = [1, 3, 24, 65, 200]                        # one column; no multiple of 4; a multiple of 4, no power of two; 64 + 1; 3 * 64 + 8
WAVE_BY_SWITCH = [64, 256]                                 # GATRES_LIN_BWD_WAVE=1: one and four column trips
WAVE_BY_POINTER = [32]                                     # the activation (lin1: also g_x) one element off a 16-byte boundary

# ---- the other tables ---------------------------------------------------------------------------------------------------------------
LIN0_FWD = {"nc": [4, 12, 32, 200], "N": [1, 63, 65, 1001], "refused_nc": 6}
LIN1_FWD = {"nc": [4, 8, 32, 128, 256], "N": [1, 7, 64, 65, 1000], "refused_nc": [24, 512]}
REDUCE = {"num_slabs": [1, 7, 8, 9, 16, 17], "count": [1, 255, 256, 257, 1000]}
WEIGHTS = [(1, 4), (3, 4), (2, 8), (1, 32), (1, 128)]      # (num_blocks, nc)
PERMUTE_N = [1, 255, 256, 257, 1001]
HASH_E = [0, 1, 63, 64, 65, 256, 257, 1000]
LOSS_N = [1, 1023, 1024, 1025, 3072, 3073, 4096, 4097, 7169]
LOSS_DENSITY = 0.7
CRITERIA = ["mse", "mae", "sce"]


def reduce_plan(num_slabs, count):
    return {"unrolled": num_slabs // REDUCE_UNROLL, "tail": num_slabs % REDUCE_UNROLL, "grid": cdiv(count, WG),
            "idle": cdiv(count, WG) * WG - count}


def loss_plan(N):
    """Thread 0 of the loss workgroup: (unrolled trips, tail trips); ``busy``: threads with at least one node."""
    unrolled, tail = lane_trips(N, LOSS_THREADS, 0)
    return {"unrolled": unrolled, "tail": tail, "busy": min(N, LOSS_THREADS),
            "unrolled_threads": sum(lane_trips(N, LOSS_THREADS, t)[0] > 0 for t in range(LOSS_THREADS))}


def grid_plan(N):
    """The one-thread-per-element kernels (permute, gather, hash): workgroups and idle threads of the last one."""
    return {"grid": cdiv(N, WG), "idle": cdiv(N, WG) * WG - N}


# ---- the flat parameter vector (include/gatres.h) -------------------------------------------------------------------------------------
def param_count(num_blocks, nc):
    return 2 * nc + num_blocks * (9 * nc + 4 * nc * nc) + nc + 1


def conv_weight_offsets(num_blocks, nc):
    """[(offset of conv1.lin.weight [2nc, nc], offset of conv2.lin.weight [nc, 2nc])] per block."""
    per = 2 * nc * nc
    out = []
    for b in range(num_blocks):
        blk = 2 * nc + b * (9 * nc + 2 * per)
        out.append((blk + 6 * nc, blk + 6 * nc + per + 3 * nc))
    return out


def describe():
    """Every case with the branch it reaches, as text (profiles/misc_turnover_margins.txt)."""
    lines = []
    for nc in LIN0_FWD["nc"]:
        for N in LIN0_FWD["N"]:
            p = lin0_fwd_plan(N, nc)
            lines.append(f"lin0 fwd nc={nc} N={N}: {p['grid']} workgroup(s), {p['idle']} idle threads in the last"
                         + ("" if p["pow2"] else ", width no power of two"))
    for nc in LIN1_FWD["nc"]:
        for N in LIN1_FWD["N"]:
            p = lin1_fwd_plan(N, nc)
            lines.append(f"lin1 fwd nc={nc} N={N}: G={p['G']} ({p['shuffles']} shuffle steps), {p['grid']} workgroup(s), "
                         f"{p['clamped']} lanes clamped to row N-1")
    for nc in ROWS_NC:
        _, R = rows_geometry(nc)
        for N, S, L, branch in rows_cases(nc):
            lines.append(f"lin0/lin1 bwd rows nc={nc} (R={R}) N={N} S={S}: slab of {L} rows: {branch}")
    for how, widths in (("width", WAVE_BY_WIDTH), ("GATRES_LIN_BWD_WAVE=1", WAVE_BY_SWITCH), ("misaligned pointer", WAVE_BY_POINTER)):
        for nc in widths:
            lines.append(f"lin0/lin1 bwd wave nc={nc} by {how}: {cdiv(nc, WAVE)} column trip(s), (N, S) in {WAVE_NS}")
    for S in REDUCE["num_slabs"]:
        p = reduce_plan(S, 1)
        lines.append(f"reduce_slabs num_slabs={S}: {p['unrolled']} unrolled trip(s) of 8 + {p['tail']} single; count in {REDUCE['count']}")
    for nb, nc in WEIGHTS:
        lines.append(f"transpose / convert conv weights num_blocks={nb} nc={nc}: {cdiv(nb * 4 * nc * nc, WG)} / {cdiv(nb * 8 * nc * nc, WG)} workgroup(s)")
    for N in PERMUTE_N:
        p = grid_plan(N)
        lines.append(f"permute_f32 / gather_u8 N={N}: {p['grid']} workgroup(s), {p['idle']} idle threads")
    for E in HASH_E:
        lines.append(f"edge_index_hash E={E}: " + ("no launch" if E == 0 else f"{cdiv(E, WG)} workgroup(s), {cdiv(E, WAVE)} wave(s) with an edge, "
                                                   f"last wave holds {E - (cdiv(E, WAVE) - 1) * WAVE}"))
    for N in LOSS_N:
        p = loss_plan(N)
        lines.append(f"masked_loss N={N}: thread 0 takes {p['unrolled']} unrolled + {p['tail']} tail trip(s), {p['unrolled_threads']} thread(s) "
                     f"in the unrolled loop, {p['busy']} with a node")
    return lines
