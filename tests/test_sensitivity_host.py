"""The sensitivity pass, on the host: the four new symbols (gatres_stage_observed_targets of k_estimate.hip and the three launches
of k_sensitivity.hip) are declared, exported and bound without an ABI change and refuse their bad arguments before any launch; the
numpy statements of sensitivity.py hold on hand-computed cases; ``influence_from_table`` on a hand-made table; the Python refusals
that need no device; and the locality rule the device tests hold the kernels to is pinned on the fp64 oracle's Jacobian.  No GPU,
no kernel launches."""
import os
import re

import numpy as np
import pytest
import torch

import sensitivity_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gatres_stage_observed_targets", "gatres_sensitivity_gather", "gatres_sensitivity_fold", "gatres_sensitivity_spread")
P = 4096                       # (any non-null address: a refused call never reads it)
Q = 8192


def header():
    with open(os.path.join(ROOT, "include", "gatres.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


# ---- 1. symbols and refusals ----------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound_and_the_abi_stays(pkg, lib):
    hdr = header()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in pkg._native.SIGNATURES
    S = pkg._native.SIGNATURES
    # the arguments of gatres_stage_observed_layouts without layouts, plus targets and g_out
    assert len(S["gatres_stage_observed_targets"][1]) == len(S["gatres_stage_observed_layouts"][1]) - 1 + 2
    assert len(S["gatres_sensitivity_gather"][1]) == 13 and len(S["gatres_sensitivity_fold"][1]) == 8
    assert len(S["gatres_sensitivity_spread"][1]) == 7
    assert "#define GATRES_ABI_VERSION 9" in hdr and pkg._native.ABI_VERSION == 9
    assert b"abi9" in lib.gatres_version()
    assert "k_sensitivity.hip" in pkg._build.SOURCES
    assert re.search(r"#define GATRES_SENSITIVITY_RECORD\s+%d\b" % pkg._native.SENSITIVITY_RECORD, hdr)
    assert pkg._native.SENSITIVITY_RECORD == 5 == pkg.estimation.SENSITIVITY_RECORD == pkg.sensitivity.SENSITIVITY_RECORD
    assert pkg.influence_from_table is pkg.estimation.influence_from_table is pkg.sensitivity.influence_from_table


def stage(lib, src=P, layout=0, src_rows=8, first_pair=0, num_targets=6, targets=7 * Q, n=37, graphs=3, observed=P + 2048, k=3,
          normalise=0, offset=0.0, factor=1.0, x=Q, mask=Q + 4096, g_out=2 * Q, available=3 * Q, nan_is_missing=0):
    return lib.gatres_stage_observed_targets(src, layout, src_rows, first_pair, num_targets, targets, n, graphs, observed, k,
                                             normalise, offset, factor, x, mask, g_out, available, nan_is_missing, None)


def test_stage_observed_targets_checks_its_arguments_before_any_launch(lib):
    # the pair range: 8 rows x 6 targets = 48 pairs
    assert stage(lib, first_pair=-1) == -1
    assert stage(lib, first_pair=46) == -1                     # pairs 46, 47, 48 of 48
    assert stage(lib, first_pair=8, num_targets=1) == -1       # as a plain pass: row 8 of 8
    assert stage(lib, src_rows=0) == -1
    assert stage(lib, src_rows=2 ** 62, num_targets=4) == -1   # (src_rows * num_targets does not fit)
    assert stage(lib, num_targets=0) == -1
    assert stage(lib, num_targets=-3) == -1
    assert stage(lib, targets=None, num_targets=38) == -1      # target t is node t: 38 targets of 37 nodes
    # g_out: 3 * 37 floats = 444 bytes; x_dst the same from Q, mask 111 bytes from Q + 4096; src 8 * 37 floats = 1184 bytes from
    # P; targets 6 ints = 24 bytes
    assert stage(lib, g_out=None) == -1
    assert stage(lib, g_out=Q) == -1                           # g_out is x_dst
    assert stage(lib, g_out=Q + 444 - 4) == -1                 # starts on the last float of x_dst
    assert stage(lib, g_out=Q - 444 + 4) == -1                 # ends on the first float of x_dst
    assert stage(lib, g_out=Q + 4096 + 111 - 1) == -1          # the last byte of mask
    assert stage(lib, g_out=P + 1184 - 4) == -1                # the last float of src
    assert stage(lib, g_out=7 * Q + 24 - 4) == -1              # the last target
    assert stage(lib, g_out=7 * Q - 444 + 4) == -1             # ends on the first target
    assert stage(lib, targets=Q + 4) == -1                     # targets inside x_dst
    assert stage(lib, targets=Q + 4096) == -1                  # targets inside mask
    # those of the sibling entry points
    assert stage(lib, k=0) == -1
    assert stage(lib, k=38) == -1
    assert stage(lib, graphs=0) == -1
    assert stage(lib, n=0) == -1
    for name in ("src", "observed", "x", "mask"):
        assert stage(lib, **{name: None}) == -1, name
    assert stage(lib, layout=2) == -1
    assert stage(lib, normalise=3) == -1
    assert stage(lib, layout=1, normalise=1, factor=0.0) == -1
    assert stage(lib, x=P) == -1                               # in place
    assert stage(lib, available=Q) == -1                       # available is x_dst
    assert stage(lib, available=Q + 4096 + 3 * 37 - 1) == -1   # the last byte of mask
    assert stage(lib, available=None, nan_is_missing=0, k=0) == -1      # (NULL is legal here: k is what is refused)


def gather(lib, g_x=P, mask=Q, fault=None, n=37, graphs=3, observed=3 * Q, k=3, unit=0.5, J=8 * Q, J_rows=9, J_stride=4, first_row=2):
    return lib.gatres_sensitivity_gather(g_x, mask, fault, n, graphs, observed, k, unit, J, J_rows, J_stride, first_row, None)


def test_sensitivity_gather_checks_its_arguments_before_any_launch(lib):
    for name in ("g_x", "mask", "observed", "J"):
        assert gather(lib, **{name: None}) == -1, name
    assert gather(lib, n=0) == -1 and gather(lib, graphs=0) == -1
    assert gather(lib, k=0) == -1 and gather(lib, k=38) == -1
    assert gather(lib, J_stride=2) == -1                       # below K
    assert gather(lib, first_row=-1) == -1
    assert gather(lib, first_row=7) == -1                      # rows 7, 8, 9 of 9
    assert gather(lib, J_rows=0) == -1
    assert gather(lib, J_rows=2, first_row=0) == -1
    # overlaps: the batch's rows are 3 * 4 floats = 48 bytes from J + 2 * 16; g_x 444 bytes from P, mask 111 from Q, observed 12
    assert gather(lib, J=P - 32) == -1                         # the batch's first row is g_x
    assert gather(lib, J=P - 32 + 444 - 4) == -1               # ... starts on the last float of g_x
    assert gather(lib, J=P - 32 - 48 + 4) == -1                # ... ends on the first float of g_x
    assert gather(lib, J=Q - 32 + 110) == -1                   # the last byte of mask
    assert gather(lib, J=3 * Q - 32 + 8) == -1                 # the last sensor index
    assert gather(lib, fault=8 * Q + 32 + 44) == -1            # fault is the batch's last float
    assert gather(lib, fault=8 * Q + 32 + 48, k=0) == -1       # (one past it is legal: k is what is refused)


def fold(lib, J=P, S=4, T=3, K=5, stride=6, table=16 * Q, accumulate=0):
    return lib.gatres_sensitivity_fold(J, S, T, K, stride, table, accumulate, None)


def test_sensitivity_fold_checks_its_arguments_before_any_launch(lib):
    assert fold(lib, J=None) == -1 and fold(lib, table=None) == -1
    assert fold(lib, S=0) == -1 and fold(lib, T=0) == -1 and fold(lib, K=0) == -1
    assert fold(lib, stride=4) == -1                           # below K
    assert fold(lib, S=2 ** 61) == -1                          # (the matrix's bytes do not fit)
    # J is 4 * 3 * 6 floats = 288 bytes from P, the table 3 * 5 * 5 doubles = 600 bytes
    assert fold(lib, table=P) == -1
    assert fold(lib, table=P + 288 - 8) == -1                  # starts on the last bytes of J
    assert fold(lib, table=P - 600 + 8) == -1                  # ends on the first bytes of J


def spread(lib, J=P, rows=7, K=5, stride=6, sigma=4 * Q, out=5 * Q):
    return lib.gatres_sensitivity_spread(J, rows, K, stride, sigma, out, None)


def test_sensitivity_spread_checks_its_arguments_before_any_launch(lib):
    for name in ("J", "sigma", "out"):
        assert spread(lib, **{name: None}) == -1, name
    assert spread(lib, rows=0) == -1 and spread(lib, K=0) == -1
    assert spread(lib, stride=4) == -1                         # below K
    assert spread(lib, rows=2 ** 61) == -1
    # J is 7 * 6 floats = 168 bytes from P, sigma 20 bytes, out 28 bytes
    assert spread(lib, out=P) == -1 and spread(lib, out=P + 168 - 4) == -1 and spread(lib, out=P - 28 + 4) == -1
    assert spread(lib, out=4 * Q + 16) == -1                   # the last sigma
    assert spread(lib, sigma=P + 164) == -1                    # sigma on the last float of J


# ---- 2. the shapes of the device tests against the kernels' constants ---------------------------------------------------------------
def test_turnover_shapes_lie_past_the_constants():
    C = R.constants()
    for name in ("SG_T", "SF_T", "SF_U", "SS_T"):
        assert C.get(name, 0) > 0, name
    src = R.source()
    assert "i += (long long)gridDim.x * SG_T" in src and "s0 += SF_U" in src
    c = R.GATHER_CAPPED
    assert c["G"] * c["K"] > R.grid_cap("gatres_sensitivity_gather") * C["SG_T"] and c["K"] <= c["N"]      # the grid-stride trip
    S = [s for s, _, _ in R.FOLD_TRIPS]
    assert C["SF_U"] in S and C["SF_U"] + 1 in S and max(S) > 2 * C["SF_U"]                                 # one trip, two, three
    assert any(t * k > C["SF_T"] for _, t, k in R.FOLD_TRIPS)                                               # a second workgroup
    S, T, K, cut = R.FOLD_CUT
    assert 0 < cut < S and cut % C["SF_U"] != 0 and T * K > C["SF_T"]


# ---- 3. the numpy statements ------------------------------------------------------------------------------------------------------
def test_seeds_with_and_without_targets(pkg):
    s = pkg.sensitivity_seeds(0, 3, 4, 3)                      # pairs 0, 1, 2 of T = 3: nodes 0, 1, 2
    np.testing.assert_array_equal(s, np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], dtype=np.float32))
    assert s.dtype == np.float32
    s = pkg.sensitivity_seeds(2, 4, 5, 3, targets=[4, 0, 2])   # pairs 2, 3, 4, 5: targets 2, 0, 1, 2 -> nodes 2, 4, 0, 2
    np.testing.assert_array_equal(s.argmax(1), [2, 4, 0, 2])
    np.testing.assert_array_equal(s.sum(1), [1, 1, 1, 1])
    with pytest.raises(ValueError):
        pkg.sensitivity_seeds(0, 3, 4, 5)                      # five targets of four nodes, unnamed
    with pytest.raises(ValueError):
        pkg.sensitivity_seeds(0, 3, 4, 2, targets=[1])


def test_rows_from_gx_masks_scales_and_reports_a_fault(pkg):
    g_x = np.array([[1.5, np.nan, -2.0, 0.25], [3.0, 7.0, np.nan, 1.0]], dtype=np.float32)
    mask = np.array([[0, 1, 0, 1], [1, 0, 1, 0]], dtype=np.uint8)
    rows = pkg.sensitivity_rows_from_gx(g_x, mask, [2, 1, 0], 0.5)
    np.testing.assert_array_equal(rows, np.array([[-1.0, 0.0, 0.75], [0.0, 3.5, 0.0]], dtype=np.float32))      # (NaNs under the mask)
    unit = 12.81 / (12.81 + 1e-8)
    one = pkg.sensitivity_rows_from_gx(np.float32([[0.1]]), np.uint8([[0]]), [0], unit)
    assert one.dtype == np.float32 and one[0, 0] == np.float32(0.1) * np.float32(unit)
    assert np.isnan(pkg.sensitivity_rows_from_gx(g_x, mask, [2, 1, 0], 0.5, fault=np.float32("nan"))).all()
    np.testing.assert_array_equal(pkg.sensitivity_rows_from_gx(g_x, mask, [2, 1, 0], 0.5, fault=0.0), rows)


def test_fold_by_hand_and_in_two_chunks(pkg):
    J = np.zeros((3, 1, 2), dtype=np.float32)
    J[:, 0, 0] = [0.5, -2.0, 0.0]
    J[:, 0, 1] = [0.0, 0.0, 0.0]
    t = pkg.sensitivity_fold_ref(J)
    np.testing.assert_array_equal(t[0, 0], [2.0, -1.5, 2.5, 4.25, 2.0])
    np.testing.assert_array_equal(t[0, 1], [0.0, 0.0, 0.0, 0.0, 0.0])
    J = np.random.default_rng(1).standard_normal((11, 4, 3)).astype(np.float32)
    J[3, 1, 2] = 0.0
    whole = pkg.sensitivity_fold_ref(J)
    cut = pkg.sensitivity_fold_ref(J[4:], table=pkg.sensitivity_fold_ref(J[:4]))
    np.testing.assert_array_equal(whole, cut)
    assert whole[1, 2, 0] == 10 and whole[0, 0, 0] == 11
    # fp64 sums of fp32 values: not the fp32 sums
    np.testing.assert_array_equal(whole[:, :, 4], np.abs(J.astype(np.float64)).max(0))
    np.testing.assert_allclose(whole[:, :, 1], J.astype(np.float64).sum(0), rtol=1e-14, atol=1e-15)


def test_spread_by_hand_and_with_a_zero_column(pkg):
    J = np.array([[3.0, 100.0, 4.0], [0.0, 5.0, 0.0]], dtype=np.float32)
    sigma = np.array([1.0, 0.0, 0.5], dtype=np.float32)
    out = pkg.linear_spread_ref(J, sigma)
    assert out.dtype == np.float32
    np.testing.assert_array_equal(out, np.array([np.sqrt(9.0 + 4.0), 0.0], dtype=np.float32))
    J = np.random.default_rng(2).standard_normal((2, 5, 7)).astype(np.float32)
    sigma = np.random.default_rng(3).random(7).astype(np.float32)
    want = np.sqrt(((J.astype(np.float64) * sigma.astype(np.float64)) ** 2).sum(-1))
    got = pkg.linear_spread_ref(J, sigma)
    assert got.shape == (2, 5) and np.abs(got - want).max() <= 2.0 ** -23 * want.max()
    with pytest.raises(ValueError):
        pkg.linear_spread_ref(J, sigma[:6])


def test_influence_from_a_hand_made_table(pkg):
    # two snapshots, junctions 4, 1 and 7, sensors at nodes 1 and 9
    J = np.array([[[0.5, 0.0], [0.25, 0.25], [0.0, 0.0]],
                  [[0.25, 0.0], [0.75, -0.25], [0.0, 0.0]]], dtype=np.float32)
    r = pkg.influence_from_table(pkg.sensitivity_fold_ref(J), [4, 1, 7], [1, 9], 2)
    np.testing.assert_array_equal(r["mean"], [[0.375, 0.0], [0.5, 0.0], [0.0, 0.0]])
    np.testing.assert_array_equal(r["mean_abs"], [[0.375, 0.0], [0.5, 0.25], [0.0, 0.0]])
    np.testing.assert_array_equal(r["rms"], np.sqrt(np.array([[0.3125 / 2, 0.0], [0.625 / 2, 0.125 / 2], [0.0, 0.0]])))
    np.testing.assert_array_equal(r["max_abs"], [[0.5, 0.0], [0.75, 0.25], [0.0, 0.0]])
    np.testing.assert_array_equal(r["nonzero"], [[2, 0], [2, 2], [0, 0]])
    np.testing.assert_array_equal(r["dominant_sensor"], [0, 0, -1])
    np.testing.assert_array_equal(r["dominant_share"][:2], [1.0, 0.5 / 0.75])
    np.testing.assert_array_equal(r["participation"][:2], [1.0, 0.75 ** 2 / (0.25 + 0.0625)])
    assert np.isnan(r["dominant_share"][2]) and np.isnan(r["participation"][2])
    np.testing.assert_array_equal(r["sensor_total"], [0.875, 0.25])
    np.testing.assert_array_equal(r["sensor_dominates"], [2, 0])
    assert r["self_entry"][0] == 0.5 and np.isnan(r["self_entry"][1])          # node 1 is target 1; node 9 is no target
    assert r["targets"] == [4, 1, 7] and r["observed_idx"] == [1, 9] and r["num_snapshots"] == 2
    with pytest.raises(ValueError):
        pkg.influence_from_table(np.zeros((3, 2, 4)), [4, 1, 7], [1, 9], 2)
    with pytest.raises(ValueError):
        pkg.influence_from_table(np.zeros((3, 2, 5)), [4, 1, 7], [1, 9], 0)


# ---- 4. Python refusals that need no device ---------------------------------------------------------------------------------------
def test_the_sensitivity_map_holds_its_table_and_refuses_a_wrong_one(pkg):
    table = torch.arange(30, dtype=torch.float64).reshape(3, 2, 5)
    m = pkg.SensitivityMap(table, [4, 1, 7], [1, 9], 6)
    d = m.state_dict()
    assert d["targets"] == [4, 1, 7] and d["observed_idx"] == [1, 9] and d["num_snapshots"] == 6
    back = pkg.SensitivityMap.from_state_dict(d)
    assert torch.equal(back.table, table) and back.targets == m.targets and back.num_snapshots == 6
    assert back.device == torch.device("cpu")
    for bad in (table.float(), table[:2], table.reshape(2, 3, 5)):
        with pytest.raises(ValueError, match="table"):
            pkg.SensitivityMap(bad, [4, 1, 7], [1, 9], 6)
    with pytest.raises(ValueError, match="num_snapshots"):
        pkg.SensitivityMap(table, [4, 1, 7], [1, 9], 0)


def test_the_estimator_has_the_public_methods(pkg):
    for name in ("sensitivity", "sensitivity_store", "sensitivity_map", "influence_report", "linear_spread", "linear_spread_store"):
        assert callable(getattr(pkg.PressureEstimator, name)), name


def test_targets_are_refused_without_a_device(pkg):
    est = object.__new__(pkg.PressureEstimator)                # (the checks read nothing but the node count and the cache)
    est.nodes_per_graph, est._targets_cache = 37, None
    assert est._targets(None) == (list(range(37)), None)
    for bad in ([], [37], [-1], [3, 40], "ab", 5):
        with pytest.raises(ValueError, match="targets"):
            est._targets(bad)


# ---- 5. locality of the fp64 oracle's Jacobian ------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb,n,pipes", R.LOCALITY_CASES)
def test_the_oracles_jacobian_is_exactly_zero_beyond_three_hops_per_block(pkg, oracle, nb, n, pipes):
    ei = pkg.wdn_synth.make_wdn_topology(n, pipes, seed=0)
    p = oracle.init_params(nb, 8, seed=3)
    x = pkg.wdn_synth.make_snapshots(1, n, seed=5)[0]
    J = R.oracle_jacobian(oracle, p, x, ei, nb).numpy()
    dist = R.graph_distances(ei.numpy(), n)
    far = dist > 3 * nb
    expected = {(0, 12): 132, (1, 40): 1044, (2, 40): 172, (2, 37): 120}[(nb, n)]
    assert int(far.sum()) == expected
    assert (J[far] == 0.0).all()
    assert (J[~far] != 0.0).mean() > 0.5                       # (and it is no all-zero matrix)
