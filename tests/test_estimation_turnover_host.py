"""The turnover shapes of tests/turnover_cases.py against the kernels' constants, on the host.

tests/test_gpu_estimation_turnover.py runs k_estimate.hip (and tests/test_gpu_grad_flow.py ``gatres_mean_abs_diff``) at shapes
chosen to lie just past a loop's first trip, a tile or workgroup boundary or a grid cap.  Those shapes are only as good as the
constants they were chosen against: this module reads the constants from the kernel sources and asserts that every shape still
lies on the intended side, so that retuning a constant fails here -- and says which shape has to move -- instead of the device
tests quietly going back to one trip.  It also pins the inputs: the properties the device tests rely on hold, and the numpy
statements are deterministic.  No GPU, no kernel launches."""
import os
import re

import numpy as np

import turnover_cases as T
from estimation_refs import (numpy_fold, numpy_node_moments, numpy_normalise, numpy_pair_errors, numpy_reduce, numpy_spread_moments,
                             numpy_stage, numpy_write_back)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gnn-pressure-estimation_amd", "csrc")
NAMES = ("OBS_T", "OBS_MAX_GY", "EW_T", "ER_T", "NE_WAVES", "NE_U", "NE_T", "PE_WAVES", "LR_U", "LR_T", "GF_U", "GF_T")


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def constants():
    """The ``constexpr int`` constants of the two kernel files and GATRES_WAVE; a constant given as a product of earlier ones
    (NE_T = NE_WAVES * GATRES_WAVE) is multiplied out."""
    known = {"GATRES_WAVE": int(re.search(r"#define GATRES_WAVE (\d+)", source("gatres_common.h")).group(1))}
    for name in ("k_estimate.hip", "k_grad_flow.hip"):
        for key, expr in re.findall(r"constexpr int (\w+) = ([^;]+);", source(name)):
            value = 1
            for factor in expr.split("*"):
                factor = factor.strip()
                if not (factor.isdigit() or factor in known):
                    break
                value *= int(factor) if factor.isdigit() else known[factor]
            else:
                known[key] = value
    return known


def grid_cap(entry):
    """The workgroup cap in the wrapper ``entry`` of k_estimate.hip: ``if (wgs > CAP) wgs = CAP;``."""
    m = re.search(r'extern "C" int %s\(.*?if \(wgs > (\d+)\) wgs = (\d+);' % entry, source("k_estimate.hip"), flags=re.S)
    assert m and m.group(1) == m.group(2), entry
    assert source("k_estimate.hip")[m.start() + 10:m.end()].count('extern "C"') == 0, entry      # (the cap of this wrapper)
    return int(m.group(1))


C = constants()
WAVE = C["GATRES_WAVE"]


def test_every_constant_is_found():
    for name in NAMES:
        assert name in C and C[name] > 0, name
    assert C["NE_T"] == C["NE_WAVES"] * WAVE and WAVE == 64
    assert grid_cap("gatres_estimate_write") == 4096 and grid_cap("gatres_ensemble_reduce") == 2048
    src = source("k_estimate.hip")
    assert "OBS_TILE = 4 * OBS_T + 4" in src                       # a tile column: 4 * OBS_T nodes plus the alignment shift
    # the strides the shapes are held against: of a lane over a graph's chunks, of a wave over the rows, of a thread over a vector
    assert "v0 += 4 * GATRES_WAVE" in src and "s0 += (long long)NE_U * NE_WAVES" in src and "s0 += LR_U" in src
    assert "i0 += (long long)GF_U * GF_T" in source("k_grad_flow.hip")


# ---- 1. staging -------------------------------------------------------------------------------------------------------------------
def test_staging_shapes_pass_the_grid_rows_the_tile_and_the_slot_loop():
    many, tile, sensors = T.STAGE_MANY_GRAPHS, T.STAGE_SECOND_TILE, T.STAGE_MANY_SENSORS
    assert many["G"] > C["OBS_MAX_GY"] and many["S"] >= many["G"]                 # the g += gridDim.y loop
    assert many["N"] % 4 != 0                                                      # (every alignment shift occurs)
    column = 4 * C["OBS_T"] - 4                                                    # nodes >= this lie in the second column for some shift
    for c in (tile, sensors):
        assert c["N"] > column and (c["N"] + 3) // 4 + 1 > C["OBS_T"]             # two workgroup columns
        assert c["first_row"] > 0 and c["first_row"] + c["G"] <= c["S"]
    assert min(tile["observed"]) < column <= max(tile["observed"]) and tile["N"] - 1 in tile["observed"]
    assert sensors["K"] > C["OBS_T"]                                               # the k += OBS_T loop
    obs = T.many_sensors()
    assert len(obs) == sensors["K"] == len(set(obs)) and min(obs) == 0 and max(obs) == sensors["N"] - 1
    assert obs != sorted(obs)
    late = obs[C["OBS_T"]:]                                                        # placed by the loop's second trip
    assert {0, 1019, 1020, 1021, 1022, 1023, 1024, 1029} <= set(late)
    assert any(v < column for v in late) and any(v >= column + 4 for v in late)    # ... in both tile columns
    rows = T.rows_with_a_repeat(many["S"])
    assert len(set(rows.tolist())) == many["S"] - 1 and rows.min() >= 0 and rows.max() < many["S"]
    p = T.STAGE_PAIRS
    for count in (p["members"], p["layouts"]):
        pair = p["first_pair"] + np.arange(p["G"])
        assert len(set((pair // count).tolist())) > 1 and pair.max() < sensors["S"] * count


def test_availability_has_its_gaps_and_its_two_special_sensors():
    for S, K, zeros in ((300, 3, 0.2), (T.STAGE_MANY_SENSORS["S"], 300, 0.2), (130, 9, 0.3), (9, 600, 0.3)):
        a = T.availability(S, K, zeros, seed=1)
        assert a.dtype == np.uint8 and a.shape == (S, K) and (a[:, 0] == 0).all() and (a[:, 1] == 1).all()
        if K > 2 and S * K > 500:
            assert abs(1.0 - a[:, 2:].mean() - zeros) < 0.05
    a, holes = T.availability(300, 3, 0.2, seed=2), T.nan_holes(300, 3, seed=4)
    assert (holes & (a != 0)).any() and (holes & (a == 0)).any() and 0.05 < holes.mean() < 0.15
    lay = T.pair_layouts(3, 300)
    assert (lay.sum(1) > 100).all() and (lay.sum(1) < 200).all() and len({r.tobytes() for r in lay}) == 3


# ---- 2. write-back and 3. ensemble reduce -----------------------------------------------------------------------------------------
def test_write_back_and_reduce_shapes_pass_their_grid_caps():
    per_trip = grid_cap("gatres_estimate_write") * 4 * C["EW_T"]
    assert per_trip == 4096 * 1024
    odd, vec = T.WRITE_CAPPED["odd_rows"], T.WRITE_CAPPED["vector_rows"]
    for c in (odd, vec):
        assert per_trip < c["N"] * c["G"] < 2 * per_trip and c["stride"] >= c["N"]
        assert 4 * c["N"] * c["G"] < 32 << 20                                      # (tens of MB per array, no more)
    assert odd["N"] % 4 != 0 and vec["N"] % 4 == 0 and vec["stride"] % 4 == 0 and vec["stride"] > vec["N"]
    assert all(n < 4 or n % 4 for n in T.WRITE_SMALL["N"]) and sum(n < 4 for n in T.WRITE_SMALL["N"]) == 3
    chunks = grid_cap("gatres_ensemble_reduce") * C["ER_T"]
    w1, w4 = T.REDUCE_CAPPED["W1"], T.REDUCE_CAPPED["W4"]
    assert w1["N"] % 4 != 0 and w1["C"] * w1["N"] > chunks                        # one node per chunk
    assert w4["N"] % 4 == 0 and w4["stride"] % 4 == 0 and w4["C"] * (w4["N"] // 4) > chunks
    for c in (w1, w4):
        assert c["M"] > 1 and 4 * c["C"] * c["M"] * c["stride"] < 32 << 20


# ---- 4. per-node moments ----------------------------------------------------------------------------------------------------------
def test_moment_shapes_pass_the_first_workgroup_the_sensor_loop_and_two_row_trips():
    chunk = C["NE_WAVES"] * C["NE_U"]
    sizes = sorted({n for n, _ in T.MOMENTS_SMALL})
    assert sizes[0] == WAVE and sizes[1] == WAVE + 1 and sizes[2] > 2 * WAVE and sizes[2] % WAVE != 0
    assert max(s for _, s in T.MOMENTS_SMALL) > 2 * chunk and min(s for _, s in T.MOMENTS_SMALL) == chunk + 1
    big = T.MOMENTS_LARGE
    assert big["K"] > C["NE_T"] and big["N"] > 16 * WAVE
    for N in sizes + [big["N"]]:
        obs = T.moment_sensors(N)
        assert len(set(obs)) == len(obs) and obs != sorted(obs) and 0 <= min(obs) and max(obs) == N - 1
        assert {v for v in T.MOMENT_NODES if v < N} <= set(obs)
    obs = T.moment_sensors(big["N"])
    assert len(obs) == big["K"]
    groups = (big["N"] + WAVE - 1) // WAVE
    assert {v // WAVE for v in obs} == set(range(groups)) and groups == 17        # sensors in every workgroup
    late = obs[C["NE_T"]:]                                                         # placed by the loop's second trip
    assert {1029, 1024, 0, 63, 64} <= set(late) and {v // WAVE for v in late} >= {0, 1, groups - 1}


def test_moment_inputs_keep_nothing_in_the_zero_column_and_everything_elsewhere():
    for N, S in T.MOMENTS_SMALL + [(T.MOMENTS_LARGE["N"], T.MOMENTS_LARGE["S"])]:
        est, truth = T.moments_inputs(N, S)
        assert est.dtype == truth.dtype == np.float32 and est.shape == truth.shape == (S, N)
        t32 = ((truth * np.float32(T.SCALE)).astype(np.float32) + np.float32(T.OFFSET)).astype(np.float32)
        zc = T.zero_column(N)
        assert (np.abs(t32[:, zc]) <= np.float32(0.01)).all()                      # |D(t)| <= 0.01 in fp32 in every row
        assert (np.abs(np.delete(t32, zc, axis=1)) > np.float32(1.0)).all()        # far from the threshold elsewhere
        assert 30.0 < float(np.delete(t32, zc, axis=1).mean()) < 70.0              # around 50 m
        table = numpy_node_moments(est, truth, T.SCALE, T.OFFSET, T.moment_sensors(N))
        assert table[zc, 5] == 0 and (np.delete(table[:, 5], zc) == S).all()
        sd = T.spread_inputs(N, S)
        assert sd.dtype == np.float32 and (sd >= 0).all() and sd[:, N - 1].max() == 3.5 and (sd[:, 9] == 0).all()


# ---- 5. layout errors -------------------------------------------------------------------------------------------------------------
def test_pair_and_fold_shapes_pass_a_lanes_first_trip_and_the_first_fold_trip():
    trip = 4 * WAVE                                                                # nodes a wave covers per trip
    sizes = T.PAIRS["N"]
    assert sizes[0] == trip and sizes[1] == trip + 1                               # exactly one trip; one node into the second
    assert any(n > trip and n % 4 == 0 for n in sizes) and any(n > 4 * trip and n % 4 for n in sizes)
    G, L = T.PAIRS["G"], T.PAIRS["L"]
    assert G > 5 and (G + C["PE_WAVES"] - 1) // C["PE_WAVES"] == 3 and G % C["PE_WAVES"] == 1      # a last workgroup of one wave
    for first in T.PAIRS["first_pair"]:
        s = (first + np.arange(G)) // L
        assert len(set(s.tolist())) >= 3 and s.max() < T.PAIRS["truth_rows"]
    assert any(first % L for first in T.PAIRS["first_pair"])                       # (a pass that starts inside a snapshot)
    for N in sizes:
        for scored in (False, True):
            out, mask, truth, score = T.pair_inputs(N, scored)
            counted = (mask != 0) if score is None else (mask != 0) & (score != 0)[None, :]
            n = counted.sum(1)
            assert n[T.PAIRS["empty_graph"]] == 0 and (np.delete(n, T.PAIRS["empty_graph"]) >= 1).all()
            assert counted[0, N - 1]                                               # the last node, in a later trip when N > 256
    u = C["LR_U"]
    assert [s for s, _ in T.FOLD] == [u, u + 1, 2 * u + 1] and T.FOLD[0][1] < C["LR_T"] < 2 * C["LR_T"] < T.FOLD[2][1]
    assert sum(T.FOLD_CUT) == T.FOLD[2][0] and T.FOLD_CUT[0] > u                   # the first launch of the cut takes two trips


# ---- 6. mean |a - b| --------------------------------------------------------------------------------------------------------------
def test_mean_abs_diff_sizes_straddle_the_first_trip():
    trip = C["GF_U"] * C["GF_T"]
    assert T.MEAN_ABS_DIFF_N[:3] == [trip - 1, trip, trip + 1] and T.MEAN_ABS_DIFF_N[3] > 2 * trip


# ---- the statements -----------------------------------------------------------------------------------------------------------------
def test_the_numpy_statements_are_deterministic_and_state_small_cases_by_hand():
    def twice(f):
        a, b = f(), f()
        a, b = (a, b) if isinstance(a, tuple) else ((a,), (b,))
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
        return a if len(a) > 1 else a[0]

    N, S = 65, 65
    est, truth = T.moments_inputs(N, S)
    obs = T.moment_sensors(N)
    av = T.availability(S, len(obs), 0.3, seed=1)
    twice(lambda: numpy_node_moments(est, truth, T.SCALE, T.OFFSET, obs))
    hidden = twice(lambda: numpy_node_moments(est, truth, T.SCALE, T.OFFSET, obs, av))
    assert hidden[obs[0], 0] == S and hidden[obs[1]].tolist() == [0.0] * 7 + [float(S)]
    twice(lambda: numpy_spread_moments(T.spread_inputs(N, S)))
    out, mask, truth_p, score = T.pair_inputs(257, True)
    twice(lambda: numpy_pair_errors(out, mask, truth_p[(7 + np.arange(T.PAIRS["G"])) // T.PAIRS["L"]], T.SCALE, T.OFFSET, score))
    twice(lambda: numpy_fold(T.fold_records(17, 130), 17, 130))
    twice(lambda: numpy_reduce(T.pressures(6, 37, seed=3).reshape(3, 2, 37)))
    # staging by hand: two graphs of five nodes, sensors at nodes 3 and 0, the second graph without sensor 0's reading
    x, mask = twice(lambda: numpy_stage(np.array([[1.5, 2.5], [3.5, 4.5]], dtype=np.float32), 5, [3, 0], np.array([[1, 1], [0, 1]])))
    assert x.view(np.float32).tolist() == [2.5, 0, 0, 1.5, 0, 4.5, 0, 0, 0, 0] and mask.tolist() == [0, 1, 1, 0, 1, 0, 1, 1, 1, 1]
    # (v - offset) / factor with each step rounded to fp32, and by the fp32 reciprocal
    v = np.array([50.25], dtype=np.float32)
    c = np.float32(v[0] - np.float32(0.1))
    assert numpy_normalise(v, 0, 0.1, 3.0)[0] == v[0]
    assert numpy_normalise(v, 1, 0.1, 3.0)[0] == np.float32(c / np.float32(3.0))
    assert numpy_normalise(v, 2, 0.1, 3.0)[0] == np.float32(c * np.float32(np.float32(1.0) / np.float32(3.0)))
    # write-back by hand: two graphs of three nodes into rows 1 and 2 of a [4, 4] matrix, the observed nodes keep x
    start = np.full((4, 4), -1.0, dtype=np.float32)
    res = twice(lambda: numpy_write_back(np.arange(6, dtype=np.float32), np.full(6, 10.0, dtype=np.float32),
                                         np.array([1, 0, 1, 1, 1, 0], dtype=np.uint8), 3, 2.0, 0.5, 1, start, 1))
    assert res.tolist() == [[-1.0] * 4, [0.5, 20.5, 4.5, -1.0], [6.5, 8.5, 20.5, -1.0], [-1.0] * 4] and (start == -1.0).all()
