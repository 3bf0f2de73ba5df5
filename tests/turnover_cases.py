"""The shapes and the inputs of the turnover tests of k_estimate.hip and k_grad_flow.hip: every shape lies just past a point
where a loop of a kernel takes a second trip, a grid reaches its cap or a second tile / workgroup begins.
tests/test_gpu_estimation_turnover.py launches the kernels at these shapes; tests/test_estimation_turnover_host.py reads the
loop constants from the kernel sources and asserts, without a device, that every shape still lies on the intended side of its
constant, and that the inputs built here have the properties the device tests rely on.  Everything here is numpy on the host."""
import numpy as np

SCALE, OFFSET = 12.81, 51.37                        # the descale of the write-back, the moments and the pair errors
OBS = [36, 0, 5]                                    # the sensors of tests/test_gpu_estimation.py, unsorted

# ---- 1. staging -------------------------------------------------------------------------------------------------------------------
STAGE_MANY_GRAPHS = dict(N=37, G=300, S=300, observed=OBS)                     # G > OBS_MAX_GY: the g += gridDim.y loop
STAGE_SECOND_TILE = dict(N=1030, G=2, S=4, first_row=1, observed=[1019, 1020, 1023, 1024, 1029])      # N > 4 * OBS_T - 4
STAGE_MANY_SENSORS = dict(N=1030, G=5, S=7, first_row=2, K=300)                # K > OBS_T: the k += OBS_T loop
STAGE_PAIRS = dict(members=3, layouts=3, first_pair=1, G=5)                    # the noisy / layouts launch at K = 300
# ---- 2. write-back ----------------------------------------------------------------------------------------------------------------
WRITE_SMALL = dict(N=(1, 2, 3, 5), G=7)                                        # N < 4: chunks that span several graphs
WRITE_CAPPED = {"odd_rows": dict(N=1027, G=4100, stride=1027), "vector_rows": dict(N=1028, G=4090, stride=1032)}
# ---- 3. ensemble reduce -----------------------------------------------------------------------------------------------------------
REDUCE_CAPPED = {"W1": dict(N=37, stride=37, M=2, C=14200, W=1), "W4": dict(N=40, stride=40, M=2, C=52500, W=4)}
# ---- 4. per-node moments ----------------------------------------------------------------------------------------------------------
MOMENTS_SMALL = [(N, S) for N in (64, 65, 388) for S in (65, 130)]
MOMENTS_LARGE = dict(N=1030, K=600, S=9)
MOMENT_NODES = (0, 63, 64, 127, 128)                                           # sensors on the 64-node boundaries
# ---- 5. layout errors -------------------------------------------------------------------------------------------------------------
PAIRS = dict(N=(256, 257, 300, 1030), G=9, L=3, first_pair=(6, 7), truth_rows=6, empty_graph=3)
FOLD = [(8, 6), (9, 6), (17, 130)]
FOLD_CUT = (9, 8)                                                              # S = 17 in two launches
# ---- 6. mean |a - b| --------------------------------------------------------------------------------------------------------------
MEAN_ABS_DIFF_N = [8191, 8192, 8193, 20001]


def pressures(S, N, seed):
    """fp32 [S, N]: pressures around 50 m."""
    return (np.random.default_rng(seed).standard_normal((S, N)) * 12.5 + 50.0).astype(np.float32)


# ---- staging inputs -----------------------------------------------------------------------------------------------------------------
def many_sensors(N=STAGE_MANY_SENSORS["N"], K=STAGE_MANY_SENSORS["K"]):
    """K distinct nodes of N in no order; nodes 0, 1019 .. 1024 and 1029 among them at positions k >= 256, so that the second
    trip of the slot[] loop places sensors in both tile columns."""
    forced = [1029, 0, 1022, 1019, 1024, 1021, 1020, 1023]
    rest = [int(v) for v in np.random.default_rng(K).permutation(N) if int(v) not in forced][:K - len(forced)]
    return rest[:260] + forced + rest[260:]


def rows_with_a_repeat(S, seed=3):
    """int64 [S]: a permutation of the S source rows in which row rows[S - 1] is named a second time, at position 7."""
    rows = np.random.default_rng(seed).permutation(S).astype(np.int64)
    rows[7] = rows[S - 1]
    return rows


def availability(S, K, zeros, seed):
    """uint8 [S, K] with about ``zeros`` of the entries 0: sensor 0 is never available, sensor 1 always."""
    a = (np.random.default_rng(seed).random((S, K)) >= zeros).astype(np.uint8)
    a[:, 0] = 0
    a[:, 1] = 1
    return a


def nan_holes(S, K, seed):
    """bool [S, K]: about a tenth of the readings, sensor 1's (always available) in row 0 among them."""
    h = np.random.default_rng(seed).random((S, K)) < 0.1
    h[0, 1] = True
    return h


def pair_layouts(L, K, seed=9):
    """uint8 [L, K]: about half of the sensors installed in each layout."""
    return (np.random.default_rng(seed).random((L, K)) < 0.5).astype(np.uint8)


# ---- moments inputs -----------------------------------------------------------------------------------------------------------------
def moment_sensors(N):
    """The sensors of the moments cases, unsorted.  N <= 388: the nodes of MOMENT_NODES that exist, N - 1, and inner nodes where
    there is room.  N = 1030: 600 distinct nodes with 1029, 1024 (the last workgroup), 0, 63 and 64 at positions k >= 512."""
    if N == MOMENTS_LARGE["N"]:
        K = MOMENTS_LARGE["K"]
        forced = [1029, 64, 0, 1024, 63]
        rest = [int(v) for v in np.random.default_rng(K).permutation(N) if int(v) not in forced][:K - len(forced)]
        return rest[:520] + forced + rest[520:]
    nodes = [v for v in (128, 63, 0, 127, 64) if v < N] + [v for v in (300, 200, 257) if v < N - 1]
    return nodes + ([N - 1] if N - 1 not in nodes else [])


def zero_column(N):
    return N // 2


def moments_inputs(N, S, seed=None):
    """(est, truth) fp32 [S, N]: ``truth`` in the store's units with descaled values around 50 m -- but column zero_column(N),
    whose descaled values lie within +-0.008 m, under the 0.01 m threshold of the relative error: nothing is kept there --,
    ``est`` in metres, the descaled truth plus an error of about half a metre."""
    rng = np.random.default_rng(1000 * N + S if seed is None else seed)
    phys = rng.standard_normal((S, N)) * 12.5 + 50.0
    phys[:, zero_column(N)] = np.linspace(-0.008, 0.008, S)
    truth = ((phys - OFFSET) / SCALE).astype(np.float32)
    t32 = ((truth * np.float32(SCALE)).astype(np.float32) + np.float32(OFFSET)).astype(np.float32)
    est = (t32 + (0.5 * rng.standard_normal((S, N))).astype(np.float32)).astype(np.float32)
    return est, truth


def spread_inputs(N, S):
    """fp32 [S, N] standard deviations in [0, 0.8), one large entry and one all-zero column."""
    sd = (np.random.default_rng(7 * N + S).random((S, N)) * 0.8).astype(np.float32)
    sd[S // 2, N - 1] = 3.5
    sd[:, 9] = 0.0
    return sd


# ---- layout error inputs --------------------------------------------------------------------------------------------------------------
def pair_inputs(N, scored):
    """(out [G, N], mask [G, N], truth [truth_rows, N], score [N] or None): about 70 % of the nodes counted, the last node of
    graph 0 among them, none in graph ``empty_graph``; with ``scored`` about half of the nodes scored, the last one among them."""
    rng = np.random.default_rng(10 * N + int(scored))
    G, rows = PAIRS["G"], PAIRS["truth_rows"]
    out = rng.standard_normal((G, N)).astype(np.float32)
    truth = rng.standard_normal((rows, N)).astype(np.float32)
    mask = (rng.random((G, N)) < 0.7).astype(np.uint8)
    mask[0, N - 1] = 1
    mask[PAIRS["empty_graph"]] = 0
    score = None
    if scored:
        score = (rng.random(N) < 0.5).astype(np.uint8)
        score[N - 1] = 1
    return out, mask, truth, score


def fold_records(S, L):
    """fp64 [S * L, 4] pair records: a count, two positive sums, a maximum; one pair with nothing counted."""
    rng = np.random.default_rng(100 * S + L)
    rec = rng.random((S * L, 4)) * 3.0 + 0.1
    rec[:, 0] = rng.integers(0, 40, S * L)
    rec[L + 1] = 0.0
    return rec
