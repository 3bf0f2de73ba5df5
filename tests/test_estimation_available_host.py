"""Estimation with missing sensor readings, on the host: the two new symbols of k_estimate.hip are declared, exported and
bound without an ABI change, their argument checks return before any launch, and the availability formulas of
``error_map_from_moments`` hold on a hand-computed case.  No GPU, no kernel launches."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gatres_stage_observed_available", "gatres_node_error_moments_available")
P = 4096                       # (any non-null address: a refused call never reads it)
Q = 8192


def test_new_symbols_are_declared_exported_and_bound(pkg, lib):
    with open(os.path.join(ROOT, "include", "gatres.h")) as f:
        text = f.read()
    assert "symbols only: the ABI stays" in text
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in pkg._native.SIGNATURES
    # the new entry points take the old ones' arguments plus (available, nan_is_missing) / (available)
    S = pkg._native.SIGNATURES
    assert len(S["gatres_stage_observed_available"][1]) == len(S["gatres_stage_observed"][1]) + 2
    assert len(S["gatres_node_error_moments_available"][1]) == len(S["gatres_node_error_moments"][1]) + 1


def test_the_record_macro_equals_the_python_constant_and_the_abi_stays(pkg):
    with open(os.path.join(ROOT, "include", "gatres.h")) as f:
        hdr = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    N = pkg._native
    assert re.search(r"#define GATRES_NODE_ERROR_AVAIL_RECORD\s+%d\b" % N.NODE_ERROR_AVAIL_RECORD, hdr)
    assert N.NODE_ERROR_AVAIL_RECORD == 8 == pkg.estimation.NODE_ERROR_AVAIL_RECORD
    assert "#define GATRES_ABI_VERSION 9" in hdr and N.ABI_VERSION == 9


def stage(lib, src=P, layout=0, src_rows=8, rows=None, first_row=0, n=37, graphs=3, observed=P, k=3, normalise=0, offset=0.0,
          factor=1.0, x=Q, mask=Q + 4096, available=3 * Q, nan_is_missing=0):
    return lib.gatres_stage_observed_available(src, layout, src_rows, rows, first_row, n, graphs, observed, k, normalise, offset,
                                               factor, x, mask, available, nan_is_missing, None)


def test_stage_observed_available_checks_its_arguments_before_any_launch(lib):
    # those of gatres_stage_observed ...
    assert stage(lib, k=0) == -1
    assert stage(lib, k=38) == -1
    assert stage(lib, k=-2) == -1
    assert stage(lib, graphs=0) == -1
    assert stage(lib, graphs=-4) == -1
    assert stage(lib, n=0) == -1
    for name in ("src", "observed", "x", "mask"):
        assert stage(lib, **{name: None}) == -1, name
    assert stage(lib, layout=2) == -1
    assert stage(lib, layout=1, rows=P) == -1                  # readings are taken in order
    assert stage(lib, first_row=-1) == -1
    assert stage(lib, first_row=6) == -1                       # rows 6, 7, 8 of 8
    assert stage(lib, src_rows=0) == -1
    assert stage(lib, normalise=3) == -1
    assert stage(lib, layout=1, normalise=1, factor=0.0) == -1
    assert stage(lib, x=P) == -1                               # in place
    # ... and those of the availability
    assert stage(lib, available=None, nan_is_missing=0) == -1  # nothing that could say "missing"
    assert stage(lib, available=Q) == -1                       # available is x_dst
    assert stage(lib, available=Q + 4096) == -1                # available is mask
    assert stage(lib, available=Q + 4 * 3 * 37 - 1) == -1      # the last byte of x_dst: 3 graphs of 37 floats
    assert stage(lib, available=Q - 8 * 3 + 1) == -1           # [8][3] bytes that end on the first byte of x_dst
    assert stage(lib, available=Q + 4096 + 3 * 37 - 1) == -1   # the last byte of mask
    assert stage(lib, available=None, nan_is_missing=1, layout=1, k=0) == -1      # (NULL is legal here: k is what is refused)


def moments(lib, est=P, truth=Q, S=5, n=37, observed=3 * Q, k=3, available=5 * Q, table=4 * Q):
    return lib.gatres_node_error_moments_available(est, truth, S, n, 12.5, 50.0, observed, k, available, table, None)


def test_node_error_moments_available_checks_its_arguments_before_any_launch(lib):
    assert moments(lib, k=0) == -1
    assert moments(lib, k=38) == -1
    assert moments(lib, S=0) == -1
    assert moments(lib, n=0) == -1
    for name in ("est", "truth", "observed", "available", "table"):
        assert moments(lib, **{name: None}) == -1, name
    assert moments(lib, available=4 * Q) == -1                 # available is the table


def test_python_refusals_that_need_no_device(pkg):
    with pytest.raises(ValueError, match="observed_idx"):
        pkg.estimation.error_map_from_moments(np.zeros((4, 8)), available=True)


def test_error_map_availability_formulas_on_a_hand_computed_case(pkg):
    """3 snapshots, 4 nodes; sensors at nodes 1 and 3.  Node 1 delivers in every snapshot (never hidden), node 3 is missing
    in snapshots 0 and 2.  Only hidden entries count:
        p - t per node:   node 0: +1, -1, +2     node 1: (0, 0, 0)   node 2: -0.5, -0.5, -2     node 3: 3, (0), -1
        |t|:              node 0: 10, 20, 40     node 1: 50, 50, 50  node 2: 5, 0.005, 4        node 3: 6, (7), 0.001"""
    e = np.array([[1.0, 0.0, -0.5, 3.0], [-1.0, 0.0, -0.5, 0.0], [2.0, 0.0, -2.0, -1.0]])
    t = np.array([[10.0, 50.0, 5.0, 6.0], [20.0, 50.0, 0.005, 7.0], [40.0, 50.0, 4.0, 0.001]])
    hid = np.array([[1, 0, 1, 1], [1, 0, 1, 0], [1, 0, 1, 1]], dtype=bool)
    keep = (np.abs(t) > 0.01) & hid
    table = np.zeros((4, pkg.estimation.NODE_ERROR_AVAIL_RECORD))
    table[:, 0] = hid.sum(0)
    table[:, 1] = np.where(hid, e, 0.0).sum(0)
    table[:, 2] = np.where(hid, np.abs(e), 0.0).sum(0)
    table[:, 3] = np.where(hid, e * e, 0.0).sum(0)
    table[:, 4] = np.where(hid, np.abs(e), 0.0).max(0)
    table[:, 5] = keep.sum(0)
    table[:, 6] = np.where(keep, np.abs(e) / np.where(keep, np.abs(t), 1.0), 0.0).sum(0)
    table[:, 7] = 3 - table[:, 0]
    m = pkg.estimation.error_map_from_moments(table, available=True, observed_idx=[3, 1])
    assert m["hidden_count"].tolist() == [3.0, 0.0, 3.0, 2.0]
    assert m["observed"].dtype == np.bool_ and m["observed"].tolist() == [False, True, False, True]
    for key in ("mae", "rmse", "bias", "max_abs", "rel_error"):           # a node never hidden
        assert m[key].shape == (4,) and m[key].dtype == np.float64 and np.isnan(m[key][1]), key
    idx = [0, 2, 3]
    np.testing.assert_allclose(m["mae"][idx], [4 / 3, 1.0, 2.0], rtol=1e-15)
    np.testing.assert_allclose(m["rmse"][idx], [np.sqrt(2.0), np.sqrt(1.5), np.sqrt(5.0)], rtol=1e-15)
    np.testing.assert_allclose(m["bias"][idx], [2 / 3, -1.0, 1.0], rtol=1e-15)
    np.testing.assert_array_equal(m["max_abs"][idx], [2.0, 2.0, 3.0])
    np.testing.assert_allclose(m["rel_error"][idx], [(0.1 + 0.05 + 0.05) / 3, (0.1 + 0.5) / 2, 0.5], rtol=1e-15)
    # pooled: all 8 hidden entries; the 6 at nodes 0 and 2; the 2 at the sensor node 3
    assert m["hidden_mae"] == pytest.approx((4 + 3 + 4) / 8, rel=1e-15)
    assert m["hidden_rmse"] == pytest.approx(np.sqrt((6 + 4.5 + 10) / 8), rel=1e-15)
    assert m["nonsensor_mae"] == pytest.approx((4 + 3) / 6, rel=1e-15)
    assert m["nonsensor_rmse"] == pytest.approx(np.sqrt((6 + 4.5) / 6), rel=1e-15)
    assert m["missing_sensor_mae"] == pytest.approx(4 / 2, rel=1e-15)
    assert m["missing_sensor_rmse"] == pytest.approx(np.sqrt(10 / 2), rel=1e-15)
    # no missing sensor entry: node 3 delivers throughout as well
    table[3] = [0, 0, 0, 0, 0, 0, 0, 3]
    m = pkg.estimation.error_map_from_moments(table, available=True, observed_idx=[3, 1])
    assert np.isnan(m["missing_sensor_mae"]) and np.isnan(m["missing_sensor_rmse"]) and np.isnan(m["mae"][3])
    assert m["hidden_mae"] == m["nonsensor_mae"] == pytest.approx(7 / 6, rel=1e-15)
    # ... where the non-sensor pool is what the report without availability calls hidden, to the bit
    old = np.zeros((4, pkg.estimation.NODE_ERROR_RECORD))
    old[:, 0] = 3
    old[:, 1:7] = table[:, 1:7]
    old[[1, 3], 7] = 1.0
    ref = pkg.estimation.error_map_from_moments(old)
    assert m["nonsensor_mae"] == ref["hidden_mae"] and m["nonsensor_rmse"] == ref["hidden_rmse"]
    # every node a sensor that always delivers: nothing is hidden anywhere
    none = np.zeros((2, 8))
    none[:, 7] = 3
    m = pkg.estimation.error_map_from_moments(none, available=True, observed_idx=[0, 1])
    for key in ("hidden_mae", "hidden_rmse", "nonsensor_mae", "nonsensor_rmse", "missing_sensor_mae", "missing_sensor_rmse"):
        assert np.isnan(m[key]), key
