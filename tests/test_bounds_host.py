"""Calibrated per-node error bounds, on the host: the two symbols of k_bounds.hip are declared, exported and bound without an ABI
change and refuse their bad arguments before any launch; ``conformal_rank``, ``node_error_bounds`` and ``coverage_from_table`` hold
on hand-computed cases; ``ErrorBounds`` finds its levels and round-trips through its state dict.  No GPU, no kernel launches."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gatres_node_error_quantiles", "gatres_node_bound_coverage")
# (any non-null addresses: a refused call never reads them.)  S = 5 snapshots of N = 37 nodes, K = 3 sensors, Q = 2 levels:
# est and truth 5 * 37 floats = 740 bytes, available 15 bytes, observed 12 bytes, bounds 2 * 37 floats = 296 bytes, counts 37
# doubles = 296 bytes, table 37 * 9 doubles = 2664 bytes
EST, TRUTH, AVAIL, OBSERVED, BOUNDS, COUNTS, TABLE = 1 << 16, 2 << 16, 3 << 16, 4 << 16, 5 << 16, 6 << 16, 7 << 16
INPUTS = {"est": (EST, 740), "truth": (TRUTH, 740), "available": (AVAIL, 15), "observed": (OBSERVED, 12)}


def header():
    with open(os.path.join(ROOT, "include", "gatres.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def host_levels(values):
    return (C.c_double * max(1, len(values)))(*values)


# ---- 1. symbols and refusals ----------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound_and_the_abi_stays(pkg, lib):
    hdr = header()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in pkg._native.SIGNATURES
    S = pkg._native.SIGNATURES
    assert len(S["gatres_node_error_quantiles"][1]) == 14 and len(S["gatres_node_bound_coverage"][1]) == 13
    assert "#define GATRES_ABI_VERSION 9" in hdr and pkg._native.ABI_VERSION == 9
    assert b"abi9" in lib.gatres_version()
    assert "k_bounds.hip" in pkg._build.SOURCES


def test_the_macro_equals_the_python_constants(pkg):
    N = pkg._native
    assert re.search(r"#define GATRES_NODE_QUANTILE_MAX_LEVELS\s+%d\b" % N.NODE_QUANTILE_MAX_LEVELS, header())
    assert N.NODE_QUANTILE_MAX_LEVELS == 8 == pkg.estimation.NODE_QUANTILE_MAX_LEVELS
    assert N.NODE_COVERAGE_RECORD == 9 == pkg.estimation.NODE_COVERAGE_RECORD
    for name in ("ErrorBounds", "conformal_rank", "node_error_bounds", "coverage_from_table"):
        assert getattr(pkg, name) is getattr(pkg.estimation, name), name


def quantiles(lib, est=EST, truth=TRUTH, S=5, n=37, observed=OBSERVED, k=3, available=AVAIL, levels=(0.5, 0.9), num_levels=None,
              bounds=BOUNDS, counts=COUNTS):
    lv = None if levels is None else host_levels(levels)
    return lib.gatres_node_error_quantiles(est, truth, S, n, 12.5, 50.0, observed, k, available, lv,
                                           len(levels) if num_levels is None else num_levels, bounds, counts, None)


def coverage(lib, est=EST, truth=TRUTH, S=5, n=37, observed=OBSERVED, k=3, available=AVAIL, bounds=BOUNDS, num_levels=2,
             table=TABLE):
    return lib.gatres_node_bound_coverage(est, truth, S, n, 12.5, 50.0, observed, k, available, bounds, num_levels, table, None)


@pytest.mark.parametrize("call", [quantiles, coverage], ids=["quantiles", "coverage"])
def test_the_shared_refusals_come_before_any_launch(lib, call):
    for name in ("est", "truth", "bounds"):
        assert call(lib, **{name: None}) == -1, name
    assert call(lib, S=0) == -1
    assert call(lib, S=-3) == -1
    assert call(lib, S=2 ** 31) == -1             # (the select's histograms count in 32 bits: gatres.h)
    assert call(lib, n=0) == -1
    assert call(lib, n=-1) == -1
    assert call(lib, num_levels=0) == -1
    assert call(lib, num_levels=9) == -1
    assert call(lib, num_levels=-1) == -1
    # with an availability the sensors are needed ...
    assert call(lib, observed=None) == -1
    assert call(lib, k=0) == -1
    assert call(lib, k=38) == -1
    assert call(lib, k=-2) == -1
    # ... without one they are not looked at: these pass the checks and fail only at the launch, for want of a device
    if not torch.cuda.is_available():
        assert call(lib, available=None, observed=None, k=0) > 0
        assert call(lib, available=None, k=99) > 0


def test_quantiles_refuses_its_own_bad_arguments_before_any_launch(lib):
    assert quantiles(lib, counts=None) == -1
    assert quantiles(lib, levels=None, num_levels=2) == -1
    for bad in (0.0, 1.0, -0.1, float("nan"), 1.5, float("inf")):
        assert quantiles(lib, levels=(0.5, bad)) == -1, bad
        assert quantiles(lib, levels=(bad,)) == -1, bad
    assert quantiles(lib, levels=(0.1,) * 9) == -1
    # bounds and counts against every input, at the first and at the last byte of the input
    for out, size in (("bounds", 296), ("counts", 296)):
        for name, (base, nbytes) in INPUTS.items():
            assert quantiles(lib, **{out: base}) == -1, (out, name)
            assert quantiles(lib, **{out: base + nbytes - 1}) == -1, (out, name)        # starts on the input's last byte
            assert quantiles(lib, **{out: base - size + 1}) == -1, (out, name)          # ends on the input's first byte
    # ... and against each other
    assert quantiles(lib, counts=BOUNDS) == -1
    assert quantiles(lib, counts=BOUNDS + 295) == -1
    assert quantiles(lib, counts=BOUNDS - 295) == -1
    if not torch.cuda.is_available():       # (one byte further apart they do not overlap: the checks pass, the launch has no device)
        assert quantiles(lib, counts=BOUNDS + 296) > 0
        assert quantiles(lib, bounds=EST + 740) > 0
        assert quantiles(lib, bounds=EST - 296) > 0


def test_coverage_refuses_its_own_bad_arguments_before_any_launch(lib):
    assert coverage(lib, table=None) == -1
    for name, (base, nbytes) in list(INPUTS.items()) + [("bounds", (BOUNDS, 296))]:
        assert coverage(lib, table=base) == -1, name
        assert coverage(lib, table=base + nbytes - 1) == -1, name
        assert coverage(lib, table=base - 2664 + 1) == -1, name
    if not torch.cuda.is_available():
        assert coverage(lib, table=BOUNDS + 296) > 0
        assert coverage(lib, table=BOUNDS - 2664) > 0


# ---- 2. the rank ------------------------------------------------------------------------------------------------------------------
def test_conformal_rank_on_hand_computed_cases(pkg):
    rank = pkg.estimation.conformal_rank
    assert rank(9, 0.9) == 9                      # ceil(10 * 0.9): 10 * 0.9 is exactly 9.0 in fp64
    assert rank(10, 0.9) == 10                    # ceil(9.9)
    assert rank(8, 0.9) == 9                      # ceil(8.1) = 9 > 8: unbounded
    assert rank(1, 0.5) == 1
    for level in (0.05, 0.5, 0.999):
        assert rank(0, level) == 1                # > 0: no sample, no bound
    got = rank(np.array([9, 10, 8, 1, 0]), 0.9)
    assert got.dtype == np.float64 and got.tolist() == [9.0, 10.0, 9.0, 2.0, 1.0]
    assert rank(19, 0.95) == 19 and rank(18, 0.95) == 19          # the smallest n with a finite 95 % bound is 19


# ---- 3. the sort-based statement ---------------------------------------------------------------------------------------------------
def test_node_error_bounds_on_a_hand_written_matrix(pkg):
    nan = np.float32("nan")
    # column 0: |e| = 3, 1, 1, 2, 0 (a tie, and a zero that is -0.0); column 1: 0.5, NaN, 0.25, 4, 1; column 2: 1 .. 5
    est = np.array([[3.0, 0.5, 1.0], [-1.0, nan, 2.0], [1.0, -0.25, 3.0], [-2.0, 4.0, 4.0], [-0.0, -1.0, 5.0]], dtype=np.float32)
    truth = np.zeros((5, 3), dtype=np.float32)
    levels = (0.3, 0.5, 0.8)                       # n = 5: ranks ceil(1.8), ceil(3.0), ceil(4.8) = 2, 3, 5
    assert [int(pkg.estimation.conformal_rank(5, q)) for q in levels] == [2, 3, 5]
    b, n = pkg.estimation.node_error_bounds(est, truth, levels)
    assert b.dtype == np.float32 and b.shape == (3, 3) and n.tolist() == [5.0, 5.0, 5.0]
    assert b[:, 0].tolist() == [1.0, 1.0, 3.0]                      # sorted: 0, 1, 1, 2, 3
    assert b[0, 1] == 0.5 and b[1, 1] == 1.0 and np.isnan(b[2, 1])  # sorted: 0.25, 0.5, 1, 4, NaN -- the NaN is last
    assert b[:, 2].tolist() == [2.0, 3.0, 5.0]
    # -0.0 and +0.0 are one element: the smallest of column 0 has the pattern of +0.0
    b0, _ = pkg.estimation.node_error_bounds(est, truth, (0.1,))    # rank ceil(0.6) = 1
    assert b0.view(np.uint32)[0, 0] == 0 and b0[0, 1] == 0.25
    # a mask: column 0 keeps rows 0 and 3 (|e| = 3, 2), column 1 nothing, column 2 everything but the NaN-free row 4
    hidden = np.array([[1, 0, 1], [0, 0, 1], [0, 0, 1], [1, 0, 1], [0, 0, 0]], dtype=np.bool_)
    b, n = pkg.estimation.node_error_bounds(est, truth, (0.3, 0.5, 0.8), hidden=hidden)
    assert n.tolist() == [2.0, 0.0, 4.0]
    assert b[:, 0].tolist() == [2.0, 3.0, np.inf]                   # n = 2: ranks ceil(0.9), ceil(1.5), ceil(2.4) = 1, 2, 3 > 2
    assert np.isposinf(b[:, 1]).all()                               # an emptied column: +inf at every level
    assert b[:, 2].tolist() == [2.0, 3.0, 4.0]                      # n = 4: ranks ceil(1.5), ceil(2.5), ceil(4.0) = 2, 3, 4
    # the error is formed in fp32 against the descaled truth
    b, _ = pkg.estimation.node_error_bounds(np.float32([[1.0]]), np.float32([[1.0 + 2.0 ** -23]]), (0.5,))
    assert b[0, 0] == np.float32(2.0 ** -23)
    with pytest.raises(ValueError, match="levels"):
        pkg.estimation.node_error_bounds(est, truth, (0.5, 1.0))
    with pytest.raises(ValueError, match="hidden"):
        pkg.estimation.node_error_bounds(est, truth, (0.5,), hidden=hidden[:4])


# ---- 4. the coverage report ---------------------------------------------------------------------------------------------------------
def test_coverage_from_table_on_hand_computed_records(pkg):
    """Four nodes, two levels; node 1 is the sensor.  Node 0: 10 entries, 8 and 10 inside; node 1: 10, 10 and 10; node 2: never
    counted, bounds +inf; node 3: 5 entries, 3 inside the first bound, the second is +inf (5 inside)."""
    table = np.zeros((4, 9))
    table[0, :3] = [10, 8, 10]
    table[1, :3] = [10, 10, 10]
    table[3, :3] = [5, 3, 5]
    inf = np.inf
    bounds = np.array([[0.5, 1e-6, inf, 0.25], [1.0, 2e-6, inf, inf]], dtype=np.float32)
    m = pkg.estimation.coverage_from_table(table, bounds, (0.8, 0.95), [1])
    assert sorted(m) == ["coverage", "levels", "mean_width", "min_coverage", "nonsensor_coverage", "unbounded",
                         "worst_node"]
    assert m["levels"] == (0.8, 0.95)
    np.testing.assert_array_equal(m["coverage"][:, [0, 1, 3]], [[0.8, 1.0, 0.6], [1.0, 1.0, 1.0]])
    assert np.isnan(m["coverage"][:, 2]).all()
    np.testing.assert_array_equal(m["nonsensor_coverage"], [11.0 / 15.0, 1.0])       # nodes 0 and 3 (node 2 adds nothing)
    np.testing.assert_array_equal(m["min_coverage"], [0.6, 1.0])
    assert m["worst_node"].tolist() == [3, 0]                                          # ties: the first node
    np.testing.assert_array_equal(m["mean_width"], [2.0 * (0.5 + 0.25) / 2.0, 2.0])    # finite bounds outside the sensor
    assert m["unbounded"].tolist() == [1, 2]
    # every node a sensor, or no node with an entry: nothing to pool
    m = pkg.estimation.coverage_from_table(table, bounds, (0.8, 0.95), [0, 1, 2, 3])
    assert np.isnan(m["nonsensor_coverage"]).all() and np.isnan(m["mean_width"]).all() and m["worst_node"].tolist() == [-1, -1]
    assert m["unbounded"].tolist() == [0, 0]
    # a flat table is accepted, as the read-back delivers it
    m = pkg.estimation.coverage_from_table(table.reshape(-1), bounds.reshape(-1), (0.8, 0.95), [1])
    assert m["coverage"].shape == (2, 4)


# ---- 5. ErrorBounds -----------------------------------------------------------------------------------------------------------------
def test_error_bounds_levels_intervals_and_state_dict(pkg):
    EB = pkg.estimation.ErrorBounds
    bounds = torch.tensor([[0.5, 1.0, float("inf")], [1.5, 2.0, float("inf")]], dtype=torch.float32)
    counts = torch.tensor([7.0, 7.0, 0.0], dtype=torch.float64)
    eb = EB((0.8, 0.95), bounds, counts, [2])
    assert eb.levels == (0.8, 0.95) and eb.nodes_per_graph == 3 and eb.observed_idx == [2]
    assert eb.level_index(0.8) == 0 and eb.level_index(0.95) == 1
    for bad in (0.9, 0.80001, 0, None):
        with pytest.raises(ValueError, match="level"):
            eb.level_index(bad)
    est = torch.tensor([[10.0, 20.0, 30.0], [11.0, 21.0, 31.0]])
    lo, hi = eb.interval(est, 0.95)
    assert torch.equal(lo, est - bounds[1]) and torch.equal(hi, est + bounds[1])
    assert lo[0].tolist() == [8.5, 18.0, -float("inf")] and hi[1].tolist() == [12.5, 23.0, float("inf")]
    one = EB((0.9,), bounds[:1].clone(), counts, [2])
    assert one.level_index(None) == 0 and torch.equal(one.interval(est)[0], est - bounds[0])
    d = eb.state_dict()
    assert d["levels"] == [0.8, 0.95] and d["observed_idx"] == [2]
    assert isinstance(d["levels"], list) and d["bounds"].device.type == "cpu" and d["counts"].dtype == torch.float64
    back = EB.from_state_dict(d, "cpu")
    assert back.levels == eb.levels and back.observed_idx == eb.observed_idx
    assert torch.equal(back.bounds, bounds) and torch.equal(back.counts, counts)
    with pytest.raises(ValueError, match="bounds"):
        EB((0.8,), bounds, counts, [2])                                 # two rows for one level
    with pytest.raises(ValueError, match="counts"):
        EB((0.8, 0.95), bounds, counts[:2], [2])


def test_state_dict_travels_in_a_checkpoint(pkg, tmp_path):
    EB = pkg.estimation.ErrorBounds
    eb = EB((0.9,), torch.tensor([[0.25, float("inf")]]), torch.tensor([40.0, 3.0], dtype=torch.float64), [0])
    path = str(tmp_path / "with_bounds.pth")
    pkg.wdn_io.save_checkpoint(path, mean=1.0, std=2.0, error_bounds=eb.state_dict())
    back = EB.from_state_dict(torch.load(path)["error_bounds"])
    assert back.levels == (0.9,) and torch.equal(back.bounds, eb.bounds) and torch.equal(back.counts, eb.counts)


def test_levels_are_checked_without_a_device(pkg):
    check = pkg.estimation._check_levels
    assert check((0.9,)) == (0.9,) and check([0.5, 0.9, 0.99]) == (0.5, 0.9, 0.99)
    for bad in ((), (0.1,) * 9, (0.9, 0.5), (0.5, 0.5), (0.0,), (1.0,), (-0.1,), (float("nan"),), 0.9):
        with pytest.raises(ValueError, match="levels"):
            check(bad)
