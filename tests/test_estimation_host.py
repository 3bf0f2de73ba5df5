"""Pressure estimation on the host: ``observed_from_names``, the refusals of ``PressureEstimator`` that need no device, the
argument checks of the entry points of k_estimate.hip (they return before any launch) and the formulas of ``error_map``.
No GPU, no kernel launches."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gatres_stage_observed", "gatres_estimate_write", "gatres_node_error_moments")
P = 4096                       # (any non-null address: a refused call never reads it)
Q = 8192


def test_observed_from_names_keeps_the_sensor_order(pkg):
    nodes = ["J1", "J2", "J10", "T1", "J3"]
    assert pkg.observed_from_names(nodes, ["J10", "J1", "J3"]) == [2, 0, 4]
    assert pkg.observed_from_names(nodes, ("T1",)) == [3]
    assert pkg.observed_from_names(nodes, []) == []


def test_observed_from_names_refuses_unknown_and_duplicate_names(pkg):
    nodes = ["J1", "J2", "J3"]
    with pytest.raises(ValueError, match="J9"):
        pkg.observed_from_names(nodes, ["J1", "J9"])
    with pytest.raises(ValueError, match="twice"):
        pkg.observed_from_names(nodes, ["J2", "J1", "J2"])
    with pytest.raises(ValueError, match="twice"):
        pkg.observed_from_names(["J1", "J2", "J1"], ["J2"])


def _ctor(pkg, observed, **kw):
    model = pkg.GATResMeanConv(num_blocks=1, nc=4)
    ei = pkg.wdn_synth.make_wdn_topology(12, 14, seed=0)
    kw.setdefault("mean", 50.0)
    kw.setdefault("std", 12.5)
    return pkg.PressureEstimator(model, ei, 12, observed, **kw)


@pytest.mark.parametrize("observed,word", [([], "empty"), ([0, 12], "lie in"), ([-1, 3], "lie in"), ([3, 5, 3], "duplicates")])
def test_constructor_refuses_bad_observed_idx(pkg, observed, word):
    with pytest.raises(ValueError, match=word):
        _ctor(pkg, observed)


def test_constructor_refuses_minmax_missing_statistics_and_a_host_model(pkg):
    with pytest.raises(ValueError, match="minmax"):
        _ctor(pkg, [1, 2], norm_type="minmax")
    with pytest.raises(ValueError, match="norm_type"):
        _ctor(pkg, [1, 2], norm_type="robust")
    with pytest.raises(ValueError, match="mean and std"):
        _ctor(pkg, [1, 2], mean=None)
    with pytest.raises(ValueError, match="batch_size"):
        _ctor(pkg, [1, 2], batch_size=0)
    with pytest.raises(ValueError, match="ROCm device"):          # every other argument is fine: the model is on the host
        _ctor(pkg, [1, 2])


def test_a_multi_snapshot_store_is_refused_as_out_of_scope(pkg):
    ei = pkg.wdn_synth.make_wdn_topology(12, 14, seed=0)
    snaps = pkg.wdn_synth.make_snapshots(3, 12)
    multi = pkg.MultiSnapshotStore([(snaps, ei), (snaps, ei)], device="cpu")
    model = pkg.GATResMeanConv(num_blocks=1, nc=4)
    with pytest.raises(ValueError, match="out of scope"):
        pkg.PressureEstimator.for_store(model, multi, [1, 2])


def test_new_symbols_are_declared_exported_and_bound(pkg, lib):
    with open(os.path.join(ROOT, "include", "gatres.h")) as f:
        hdr = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in pkg._native.SIGNATURES
    N = pkg._native
    for macro, value in (("GATRES_NODE_ERROR_RECORD", N.NODE_ERROR_RECORD), ("GATRES_NODE_ERROR_CHUNK", N.NODE_ERROR_CHUNK),
                         ("GATRES_OBSERVED_FULL_ROWS", N.OBSERVED_FULL_ROWS), ("GATRES_OBSERVED_READINGS", N.OBSERVED_READINGS),
                         ("GATRES_NORMALISE_NONE", N.NORMALISE_NONE), ("GATRES_NORMALISE_DIVIDE", N.NORMALISE_DIVIDE),
                         ("GATRES_NORMALISE_RECIPROCAL", N.NORMALISE_RECIPROCAL)):
        assert re.search(r"#define %s\s+%d\b" % (macro, value), hdr), macro
    assert N.NODE_ERROR_RECORD == 8
    assert "#define GATRES_ABI_VERSION 9" in hdr and N.ABI_VERSION == 9        # symbols only: the ABI stays


def stage(lib, src=P, layout=0, src_rows=8, rows=None, first_row=0, n=37, graphs=3, observed=P, k=3, normalise=0, offset=0.0,
          factor=1.0, x=Q, mask=Q + 4096):
    return lib.gatres_stage_observed(src, layout, src_rows, rows, first_row, n, graphs, observed, k, normalise, offset, factor, x,
                                     mask, None)


def test_stage_observed_checks_its_arguments_before_any_launch(lib):
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


def write(lib, out=P, x=Q, mask=Q + 4096, n=37, graphs=3, keep=1, dst=3 * Q, dst_rows=8, stride=40, first_row=0):
    return lib.gatres_estimate_write(out, x, mask, n, graphs, 12.5, 50.0, keep, dst, dst_rows, stride, first_row, None)


def test_estimate_write_checks_its_arguments_before_any_launch(lib):
    assert write(lib, graphs=0) == -1
    assert write(lib, graphs=-1) == -1
    assert write(lib, n=0) == -1
    assert write(lib, out=None) == -1
    assert write(lib, dst=None) == -1
    assert write(lib, x=None) == -1 and write(lib, mask=None) == -1       # keep_observed reads both
    assert write(lib, stride=36) == -1
    assert write(lib, first_row=6) == -1
    assert write(lib, first_row=-1) == -1
    assert write(lib, dst_rows=0) == -1
    assert write(lib, dst=P) == -1


def moments(lib, est=P, truth=Q, S=5, n=37, observed=3 * Q, k=3, table=4 * Q):
    return lib.gatres_node_error_moments(est, truth, S, n, 12.5, 50.0, observed, k, table, None)


def test_node_error_moments_checks_its_arguments_before_any_launch(lib):
    assert moments(lib, k=0) == -1
    assert moments(lib, k=38) == -1
    assert moments(lib, S=0) == -1
    assert moments(lib, n=0) == -1
    for name in ("est", "truth", "observed", "table"):
        assert moments(lib, **{name: None}) == -1, name


def test_error_map_formulas_on_a_hand_computed_case(pkg):
    """3 snapshots, 4 nodes; node 1 is the sensor, node 3's truth is 0 throughout (no relative error).
        p - t per node:   node 0: +1, -1, +2     node 1: 0, 0, 0     node 2: -0.5, -0.5, -2     node 3: 3, 0, 0
        |t|:              node 0: 10, 20, 40     node 1: 50, 50, 50  node 2: 5, 0.005, 4        node 3: 0, 0, 0"""
    e = np.array([[1.0, 0.0, -0.5, 3.0], [-1.0, 0.0, -0.5, 0.0], [2.0, 0.0, -2.0, 0.0]])
    t = np.array([[10.0, 50.0, 5.0, 0.0], [20.0, 50.0, 0.005, 0.0], [40.0, 50.0, 4.0, 0.0]])
    keep = np.abs(t) > 0.01
    table = np.zeros((4, pkg.estimation.NODE_ERROR_RECORD))
    table[:, 0] = 3
    table[:, 1] = e.sum(0)
    table[:, 2] = np.abs(e).sum(0)
    table[:, 3] = (e * e).sum(0)
    table[:, 4] = np.abs(e).max(0)
    table[:, 5] = keep.sum(0)
    table[:, 6] = np.where(keep, np.abs(e) / np.where(keep, np.abs(t), 1.0), 0.0).sum(0)
    table[1, 7] = 1.0
    m = pkg.estimation.error_map_from_moments(table)
    np.testing.assert_allclose(m["mae"], [4 / 3, 0.0, 1.0, 1.0], rtol=1e-15)
    np.testing.assert_allclose(m["rmse"], [np.sqrt(2.0), 0.0, np.sqrt(1.5), np.sqrt(3.0)], rtol=1e-15)
    np.testing.assert_allclose(m["bias"], [2 / 3, 0.0, -1.0, 1.0], rtol=1e-15)
    np.testing.assert_array_equal(m["max_abs"], [2.0, 0.0, 2.0, 3.0])
    np.testing.assert_allclose(m["rel_error"][:3], [(0.1 + 0.05 + 0.05) / 3, 0.0, (0.1 + 0.5) / 2], rtol=1e-15)
    assert np.isnan(m["rel_error"][3])
    assert m["observed"].dtype == np.bool_ and m["observed"].tolist() == [False, True, False, False]
    # pooled over the 9 hidden entries (nodes 0, 2, 3)
    assert m["hidden_mae"] == pytest.approx((4 + 3 + 3) / 9, rel=1e-15)
    assert m["hidden_rmse"] == pytest.approx(np.sqrt((6 + 4.5 + 9) / 9), rel=1e-15)
    for k in ("mae", "rmse", "bias", "max_abs", "rel_error", "observed"):
        assert m[k].shape == (4,), k
    table[:, 7] = 1.0                                           # every node a sensor: nothing to pool
    m = pkg.estimation.error_map_from_moments(table)
    assert np.isnan(m["hidden_mae"]) and np.isnan(m["hidden_rmse"])
