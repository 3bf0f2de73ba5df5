"""Pressure estimation when some sensor readings are missing (``available`` / ``nan_is_missing`` of estimation.PressureEstimator,
gatres_stage_observed_available and gatres_node_error_moments_available of k_estimate.hip): the staging launch bit for bit
against a torch statement, the pass against the hand-written loop / the module / the oracle, a missing sensor against an
estimator built without it, the moments over the hidden entries against fp64 numpy, the leave-one-out report against its passes
written out, and the passes' freedom from synchronisation.

Shapes are those of test_gpu_estimation.py, for its reasons: 37 nodes (no multiple of 4 or 64) with the unsorted sensors
[36, 0, 5] in batches of 3 over 7 snapshots (3, 3 and a ragged 1); 40 nodes for whole chunks; 388 nodes once, for gatres_small
at batch size 32 on the window kernel.  The availability patterns are written out, not drawn, so that the cases certainly
occur: a snapshot with every reading, one with none, mixed rows (ROWS7); a sensor missing in every snapshot, one never missing
(COLS7, ``column_pattern``)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_gpu_estimation as E      # noqa: E402
from estimation_refs import torch_stage_available      # noqa: E402
from test_gpu_estimation import (DEV, N37, OBS, check_against_module, check_against_oracle, garbage, hand_loop, make_store,      # noqa: E402
                                 moments_table, raw_snapshots, small_model, stream, topology, torch_stage)

# column k is the sensor at node OBS[k]
ROWS7 = [[1, 1, 1],      # every reading
         [0, 0, 0],      # none: the model's output on an all-zero input
         [1, 0, 1],
         [0, 1, 1],
         [0, 0, 1],
         [1, 1, 0],
         [0, 1, 0]]      # (the ragged batch)
COLS7 = [[1, 0, 1],      # column 0 never missing, column 1 missing in every snapshot, column 2 mixed
         [1, 0, 0],
         [1, 0, 1],
         [1, 0, 1],
         [1, 0, 0],
         [1, 0, 0],
         [1, 0, 1]]


def avail(rows):
    return torch.tensor(rows, dtype=torch.uint8, device=DEV)


def row_pattern(S, K):
    """[S, K] for any K: row 0 has every reading, row 1 none, the others miss the readings with (5 s + 3 k) % 4 == 0."""
    a = [[0 if (5 * s + 3 * k) % 4 == 0 else 1 for k in range(K)] for s in range(S)]
    a[0] = [1] * K
    if S > 1:
        a[1] = [0] * K
    return avail(a)


def column_pattern(S):
    """[S, 3]: column 0 never missing, column 1 missing in every snapshot, column 2 missing in every third snapshot."""
    return avail([[1, 0, 0 if s % 3 == 0 else 1] for s in range(S)])


def stage_available(pkg, lib, src, layout, rows, first, n, g, observed, available, nan_is_missing=0, normalise=0, offset=0.0,
                    factor=1.0):
    x, mask = garbage(g * n)
    obs = torch.tensor(observed, dtype=torch.int32, device=DEV)
    pkg._native.check(lib.gatres_stage_observed_available(
        src.data_ptr(), layout, src.shape[0], pkg._native.ptr(rows), first, n, g, obs.data_ptr(), len(observed), normalise,
        offset, factor, x.data_ptr(), mask.data_ptr(), pkg._native.ptr(available), nan_is_missing, stream()),
        "gatres_stage_observed_available")
    return x, mask


def same_bits(a, b):
    """torch.equal that takes a NaN for equal to a NaN at the same place (a staged NaN reading)."""
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=-4096.0),
                                                                       torch.nan_to_num(b, nan=-4096.0))


def hand_loop_available(pkg, monkeypatch, model, store, observed, bs, available, keep_observed=True):
    """``hand_loop`` of test_gpu_estimation.py with its torch staging statement taking ``available``: the statement is called
    once per batch, in store order, and takes the batch's rows of ``available``."""
    at = {"first": 0}

    def staged(values, n, obs):
        g = values.shape[0]
        rows = available[at["first"]:at["first"] + g]
        at["first"] += g
        return torch_stage_available(values, n, obs, rows)

    with monkeypatch.context() as patch:
        patch.setattr(E, "torch_stage", staged)
        return hand_loop(pkg, model, store, observed, bs, keep_observed)


# ---- 1. staging --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("observed", [OBS, [17], [v for v in range(N37) if v != 20]], ids=["K3", "K1", "K36"])
def test_staging_full_rows_bitwise(pkg, lib, observed):
    S, bs, K = 7, 3, len(observed)
    store = make_store(pkg, S)
    patterns = [row_pattern(S, K)] + ([avail(ROWS7), avail(COLS7)] if K == 3 else [])
    perm = torch.tensor([4, 0, 6, 2, 5, 1, 3], dtype=torch.int64, device=DEV)
    for av in patterns:
        for first in range(0, S, bs):
            g = min(bs, S - first)
            # in store order, by first_row
            x, mask = stage_available(pkg, lib, store.data, 0, None, first, N37, g, observed, av)
            ex, em = torch_stage_available(store.data[first:first + g][:, observed], N37, observed, av[first:first + g])
            assert torch.equal(x, ex) and torch.equal(mask, em), first
            # by a rows array (a permutation of the store): available is indexed by the SOURCE row, like the store
            rows = perm[first:first + g].contiguous()
            x, mask = stage_available(pkg, lib, store.data, 0, rows, 5, N37, g, observed, av)
            ex, em = torch_stage_available(store.data[rows][:, observed], N37, observed, av[rows])
            assert torch.equal(x, ex) and torch.equal(mask, em), first
            # nan_is_missing belongs to the readings layout: here available alone decides
            x, mask = stage_available(pkg, lib, store.data, 0, rows, 5, N37, g, observed, av, nan_is_missing=1)
            assert torch.equal(x, ex) and torch.equal(mask, em), first
    # in the full-rows layout a NaN in the store is a value like any other, with nan_is_missing and without available as well
    holed = store.data.clone()
    holed[1, observed[0]] = float("nan")
    x, mask = stage_available(pkg, lib, holed, 0, None, 0, N37, 3, observed, None, nan_is_missing=1)
    ex, em = torch_stage(holed[0:3][:, observed], N37, observed)
    assert same_bits(x, ex) and torch.equal(mask, em) and int(torch.isnan(x).sum()) == 1


@pytest.mark.parametrize("normalize", [True, False], ids=["znorm", "unused"])
def test_staging_readings_layout_and_nan_readings_bitwise(pkg, lib, oracle, normalize):
    S, g, first = 7, 3, 2
    raw = raw_snapshots(pkg, S)
    store = pkg.SnapshotStore(raw, topology(pkg), device=DEV, normalize=normalize)
    model, _ = small_model(pkg, oracle)
    est = pkg.PressureEstimator.for_store(model, store, OBS, batch_size=3)
    factor = store.std + 1e-8 if normalize else 1.0
    norm = (est._normalise, store.mean if normalize else 0.0, factor)
    readings = raw.to(DEV)[:, OBS].contiguous()
    values = store.data[:, OBS].contiguous()                       # what the store's own normalisation makes of them
    av = avail(ROWS7)
    sl = slice(first, first + g)
    x, mask = stage_available(pkg, lib, readings, 1, None, first, N37, g, OBS, av, 0, *norm)
    ex, em = torch_stage_available(values[sl], N37, OBS, av[sl])
    assert torch.equal(x, ex) and torch.equal(mask, em)
    # NaN readings where available says "present": (2, 0), (3, 1), (3, 2) -- and one where it says "missing": (4, 0)
    assert [ROWS7[2][0], ROWS7[3][1], ROWS7[3][2], ROWS7[4][0]] == [1, 1, 1, 0]
    holes = torch.zeros((S, 3), dtype=torch.bool, device=DEV)
    for s, k in ((2, 0), (3, 1), (3, 2), (4, 0)):
        holes[s, k] = True
    nan_readings = torch.where(holes, torch.full_like(readings, float("nan")), readings)
    nan_values = torch.where(holes, torch.full_like(values, float("nan")), values)
    # nan_is_missing on: they are missing
    x, mask = stage_available(pkg, lib, nan_readings, 1, None, first, N37, g, OBS, av, 1, *norm)
    ex, em = torch_stage_available(values[sl], N37, OBS, (av.bool() & ~holes)[sl])
    assert torch.equal(x, ex) and torch.equal(mask, em) and torch.isfinite(x).all()
    # nan_is_missing off: the NaN is staged as the value it is
    x, mask = stage_available(pkg, lib, nan_readings, 1, None, first, N37, g, OBS, av, 0, *norm)
    ex, em = torch_stage_available(nan_values[sl], N37, OBS, av[sl])
    assert same_bits(x, ex) and torch.equal(mask, em) and int(torch.isnan(x).sum()) == 3
    # available = NULL with nan_is_missing: the NaNs alone say what is missing
    x, mask = stage_available(pkg, lib, nan_readings, 1, None, first, N37, g, OBS, None, 1, *norm)
    ex, em = torch_stage_available(values[sl], N37, OBS, (~holes)[sl])
    assert torch.equal(x, ex) and torch.equal(mask, em)


def test_staging_rows_that_are_multiples_of_four_and_unaligned_targets(pkg, lib):
    """40 nodes: every chunk of every graph is whole.  A target that starts one float past a 16-byte boundary takes the
    element-by-element stores; nothing is written outside the batch."""
    n, g = 40, 3
    store = make_store(pkg, 4, n=n, pipes=45)
    observed = [39, 3, 4, 5, 0]
    av = row_pattern(4, 5)
    x, mask = stage_available(pkg, lib, store.data, 0, None, 1, n, g, observed, av)
    ex, em = torch_stage_available(store.data[1:4][:, observed], n, observed, av[1:4])
    assert torch.equal(x, ex) and torch.equal(mask, em)
    xb, mb = garbage(g * N37 + 4)
    st37 = make_store(pkg, 3)
    obs = torch.tensor(OBS, dtype=torch.int32, device=DEV)
    av = avail(ROWS7[:3])
    pkg._native.check(lib.gatres_stage_observed_available(
        st37.data.data_ptr(), 0, 3, None, 0, N37, g, obs.data_ptr(), 3, 0, 0.0, 1.0, xb.data_ptr() + 4, mb.data_ptr() + 1,
        av.data_ptr(), 0, stream()), "gatres_stage_observed_available")
    ex, em = torch_stage_available(st37.data[:, OBS], N37, OBS, av)
    assert torch.equal(xb[1:1 + g * N37], ex) and torch.equal(mb[1:1 + g * N37], em)
    assert torch.isnan(xb[0]) and torch.isnan(xb[1 + g * N37:]).all() and int(mb[0]) == 0xAB      # nothing outside the batch
    assert (mb[1 + g * N37:] == 0xAB).all()


# ---- 2. all present equals the old path ---------------------------------------------------------------------------------------
def test_everything_available_equals_the_path_without_availability(pkg, lib, oracle):
    S = 7
    raw = raw_snapshots(pkg, S)
    store = pkg.SnapshotStore(raw, topology(pkg), device=DEV)
    ones = torch.ones((S, 3), dtype=torch.uint8, device=DEV)
    perm = torch.tensor([4, 0, 6], dtype=torch.int64, device=DEV)
    for rows, first in ((None, 2), (perm, 0)):
        x, mask = stage_available(pkg, lib, store.data, 0, rows, first, N37, 3, OBS, ones)
        ox, om = E.stage(pkg, lib, store.data, 0, rows, first, N37, 3, OBS)
        assert torch.equal(x, ox) and torch.equal(mask, om)
    model, _ = small_model(pkg, oracle)
    est = pkg.PressureEstimator.for_store(model, store, OBS, batch_size=3)
    readings = raw.to(DEV)[:, OBS].contiguous()
    norm = (est._normalise, store.mean, store.std + 1e-8)
    for nan in (0, 1):
        x, mask = stage_available(pkg, lib, readings, 1, None, 4, N37, 3, OBS, ones, nan, *norm)
        ox, om = E.stage(pkg, lib, readings, 1, None, 4, N37, 3, OBS, *norm)
        assert torch.equal(x, ox) and torch.equal(mask, om)
    want = est.estimate(readings)
    assert torch.equal(est.estimate(readings, available=ones), want)
    assert torch.equal(est.estimate(readings, available=ones.bool()), want)
    assert torch.equal(est.estimate(readings, nan_is_missing=True), want)
    assert torch.equal(est.estimate_store(store, available=ones), est.estimate_store(store))


# ---- 3. the pass ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused,keep", [(True, True), (False, True), (True, False)], ids=["fused", "per_op", "fused_predictions"])
def test_pass_equals_the_hand_written_loop_fp32(pkg, oracle, monkeypatch, fused, keep):
    store = make_store(pkg, 7)
    model, p = small_model(pkg, oracle, fused=fused)
    est = pkg.PressureEstimator.for_store(model, store, OBS, batch_size=3, keep_observed=keep)
    for av in (avail(ROWS7), avail(COLS7)):
        got = est.estimate_store(store, available=av)
        want, batches = hand_loop_available(pkg, monkeypatch, model, store, OBS, 3, av, keep)
        assert [b[2] for b in batches] == [3, 3, 1]
        assert torch.equal(got, want)
        assert torch.isfinite(got).all()                           # (ROWS7: the snapshot without any reading among them)
        if keep:         # a present sensor's own value comes back through the descale round trip, a missing one's does not
            own = store.descale(store.data[:, OBS])
            assert torch.equal(got[:, OBS][av.bool()], own[av.bool()])
            assert not torch.equal(got[:, OBS], own)
        check_against_module(pkg, model, store, batches)
        check_against_oracle(oracle, p, 2, store, batches)
    # the readings form of the same pass, with the gaps told by NaN
    readings = raw_snapshots(pkg, 7).to(DEV)[:, OBS].contiguous()
    readings[~av.bool()] = float("nan")
    assert torch.equal(est.estimate(readings, nan_is_missing=True), got)


def test_pass_equals_the_hand_written_loop_bf16(pkg, oracle, monkeypatch):
    store = make_store(pkg, 7)
    model, _ = small_model(pkg, oracle, nb=2, nc=32, dtype="bf16")
    est = pkg.PressureEstimator.for_store(model, store, OBS, batch_size=3)
    av = avail(ROWS7)
    got = est.estimate_store(store, available=av)
    want, batches = hand_loop_available(pkg, monkeypatch, model, store, OBS, 3, av)
    assert torch.equal(got, want) and torch.isfinite(got).all()
    check_against_module(pkg, model, store, batches, bf16=True)


# ---- 4. missing means "not a sensor" ----------------------------------------------------------------------------------------------
def test_a_sensor_that_is_always_missing_equals_an_estimator_built_without_it(pkg, oracle):
    S = 7
    raw = raw_snapshots(pkg, S)
    store = pkg.SnapshotStore(raw, topology(pkg), device=DEV)
    model, _ = small_model(pkg, oracle)
    three = pkg.PressureEstimator.for_store(model, store, OBS, batch_size=3)
    two = pkg.PressureEstimator.for_store(model, store, OBS[:2], batch_size=3)
    av = avail([[1, 1, 0]] * S)
    want = two.estimate_store(store)
    assert torch.equal(three.estimate_store(store, available=av), want)
    assert not torch.equal(three.estimate_store(store), want)
    r3 = raw.to(DEV)[:, OBS].contiguous()
    assert torch.equal(three.estimate(r3, available=av), two.estimate(r3[:, :2].contiguous()))
    assert torch.equal(three.estimate(r3, available=av), want)


# ---- 5. hidden nodes ----------------------------------------------------------------------------------------------------------------
def test_hidden_nodes_and_missing_readings_never_leak(pkg, oracle):
    S = 7
    raw = raw_snapshots(pkg, S)
    store = pkg.SnapshotStore(raw, topology(pkg), device=DEV)
    av = avail(ROWS7)
    other = raw.clone()
    hidden = [v for v in range(N37) if v not in OBS]
    other[:, hidden] = other[:, hidden] * -3.0 + 500.0
    for s in range(S):
        for k in range(3):
            if not ROWS7[s][k]:
                other[s, OBS[k]] = other[s, OBS[k]] * -3.0 + 500.0
    changed = pkg.SnapshotStore(other, topology(pkg), device=DEV, mean=store.mean, std=store.std)
    present = av.bool()
    assert torch.equal(changed.data[:, OBS][present], store.data[:, OBS][present])
    assert not torch.equal(changed.data[:, OBS], store.data[:, OBS]) and not torch.equal(changed.data[:, hidden], store.data[:, hidden])
    model, _ = small_model(pkg, oracle)
    est = pkg.PressureEstimator.for_store(model, store, OBS, batch_size=3)
    assert torch.equal(est.estimate_store(store, available=av), est.estimate_store(changed, available=av))
    assert not torch.equal(est.estimate_store(store), est.estimate_store(changed))      # (without it the changed readings count)


# ---- 6. the report ------------------------------------------------------------------------------------------------------------------
def moments_table_available(pkg, lib, est_m, truth, scale, offset, observed, available):
    n = truth.shape[1]
    obs = torch.tensor(observed, dtype=torch.int32, device=DEV)
    table = torch.full((n, 8), float("nan"), dtype=torch.float64, device=DEV)
    pkg._native.check(lib.gatres_node_error_moments_available(
        est_m.data_ptr(), truth.data_ptr(), truth.shape[0], n, scale, offset, obs.data_ptr(), len(observed),
        available.data_ptr(), table.data_ptr(), stream()), "gatres_node_error_moments_available")
    return table.cpu().numpy()


@pytest.mark.parametrize("S", [1, 70, 65], ids=["S1", "S70", "one_past_the_chunk"])
@pytest.mark.parametrize("normalize", [True, False], ids=["znorm", "unused"])
def test_error_moments_and_error_map_over_the_hidden_entries(pkg, lib, oracle, S, normalize):
    raw = raw_snapshots(pkg, S, seed=S)
    if not normalize:
        raw = raw - 50.0
        raw[::2, 7] = 0.0                                          # some |t| <= 0.01 ...
        raw[:, 11] = 0.004                                         # ... and a node without any kept snapshot
    store = pkg.SnapshotStore(raw, topology(pkg), device=DEV, normalize=normalize)
    model, _ = small_model(pkg, oracle)
    est = pkg.PressureEstimator.for_store(model, store, OBS, batch_size=32)
    scale, offset = (store.std, store.mean) if normalize else (1.0, 0.0)
    outside = [v for v in range(N37) if v not in OBS]
    t32 = store.descale(store.data)
    keep = (t32.abs() > 0.01).cpu().numpy()
    t = t32.double().cpu().numpy()
    for av in (column_pattern(S), row_pattern(S, 3)):
        p = est.estimate_store(store, available=av)
        T = moments_table_available(pkg, lib, p, store.data, scale, offset, OBS, av)
        assert T.tobytes() == moments_table_available(pkg, lib, p, store.data, scale, offset, OBS, av).tobytes()
        # a node outside OBS: the record of the kernel without availability, byte for byte
        T0 = moments_table(pkg, lib, p, store.data, scale, offset, OBS)
        assert T[outside].tobytes() == T0[outside].tobytes()
        # the same fp32 e and t, formed by torch on the device; H: the hidden entries
        e32 = p - t32
        e = e32.double().cpu().numpy()
        H = np.ones((S, N37), dtype=bool)
        H[:, OBS] = av.cpu().numpy() == 0
        np.testing.assert_array_equal(T[:, 0], H.sum(0))
        np.testing.assert_array_equal(T[:, 7], S - H.sum(0))
        np.testing.assert_array_equal(T[:, 5], (keep & H).sum(0))
        np.testing.assert_array_equal(T[:, 4], np.where(H, e32.abs().double().cpu().numpy(), 0.0).max(0))
        np.testing.assert_allclose(T[:, 1], np.where(H, e, 0.0).sum(0), rtol=1e-12, atol=0)
        np.testing.assert_allclose(T[:, 2], np.where(H, np.abs(e), 0.0).sum(0), rtol=1e-12, atol=0)
        np.testing.assert_allclose(T[:, 3], np.where(H, e * e, 0.0).sum(0), rtol=1e-12, atol=0)
        k = keep & H
        np.testing.assert_allclose(T[:, 6], np.where(k, np.abs(e) / np.where(k, np.abs(t), 1.0), 0.0).sum(0), rtol=1e-12, atol=0)
        # the report: error_map on the same estimates, and on estimates it forms itself
        ref = pkg.estimation.error_map_from_moments(T, available=True, observed_idx=OBS)
        for m in (est.error_map(store, estimates=p, available=av), est.error_map(store, available=av)):
            assert sorted(m) == sorted(ref)
            for key, v in ref.items():
                np.testing.assert_array_equal(m[key], v, err_msg=key)
        m = ref
        assert m["observed"].tolist() == [v in OBS for v in range(N37)]
        np.testing.assert_array_equal(m["hidden_count"], H.sum(0))
        some = H.sum(0) > 0
        np.testing.assert_allclose(m["mae"][some], (np.where(H, np.abs(e), 0.0).sum(0) / np.maximum(H.sum(0), 1))[some], rtol=1e-12)
        assert np.isnan(m["mae"][~some]).all() and np.isnan(m["max_abs"][~some]).all() and np.isnan(m["rmse"][~some]).all()
        sens = np.zeros(N37, dtype=bool)
        sens[OBS] = True
        for name, pool in (("hidden", H), ("nonsensor", H & ~sens[None, :]), ("missing_sensor", H & sens[None, :])):
            if pool.any():
                assert m[name + "_mae"] == pytest.approx(np.abs(e[pool]).mean(), rel=1e-12), name
                assert m[name + "_rmse"] == pytest.approx(np.sqrt((e[pool] ** 2).mean()), rel=1e-12), name
            else:
                assert np.isnan(m[name + "_mae"]) and np.isnan(m[name + "_rmse"]), name
        if S == 1 and av[0].all():                                 # (row_pattern: the one snapshot has every reading)
            assert np.isnan(m["missing_sensor_mae"])
    # a sensor that is present in every snapshot: nothing hidden, zero sums (column 0 of column_pattern)
    T = moments_table_available(pkg, lib, p, store.data, scale, offset, OBS, column_pattern(S))
    assert T[OBS[0]].tolist() == [0.0] * 7 + [float(S)] and T[OBS[1]][0] == S and T[OBS[1]][7] == 0
    # everything available: the non-sensor pool is today's hidden pool, to the bit
    ones = torch.ones((S, 3), dtype=torch.uint8, device=DEV)
    p1 = est.estimate_store(store)
    new, old = est.error_map(store, estimates=p1, available=ones), est.error_map(store, estimates=p1)
    assert new["nonsensor_mae"] == old["hidden_mae"] and new["nonsensor_rmse"] == old["hidden_rmse"]
    assert new["hidden_mae"] == old["hidden_mae"] and np.isnan(new["missing_sensor_mae"])


# ---- 7. the leave-one-out report ------------------------------------------------------------------------------------------------------
def test_sensor_failure_report_equals_its_passes_written_out(pkg, oracle):
    S = 7
    store = make_store(pkg, S)
    model, _ = small_model(pkg, oracle)
    est = pkg.PressureEstimator.for_store(model, store, OBS, batch_size=3)
    rep = est.sensor_failure_report(store)
    assert rep["sensors"] == [0, 1, 2]
    passes = []
    for k in (None, 0, 1, 2):
        av = torch.ones((S, 3), dtype=torch.uint8, device=DEV)
        if k is not None:
            av[:, k] = 0
        p = est.estimate_store(store, available=av)
        passes.append(est.error_map(store, estimates=p, available=av))
    base, failed = passes[0], passes[1:]
    assert sorted(rep["baseline"]) == sorted(base)
    for key, v in base.items():
        np.testing.assert_array_equal(rep["baseline"][key], v, err_msg=key)
    np.testing.assert_array_equal(rep["nonsensor_mae"], [m["nonsensor_mae"] for m in failed])
    np.testing.assert_array_equal(rep["nonsensor_rmse"], [m["nonsensor_rmse"] for m in failed])
    np.testing.assert_array_equal(rep["failed_sensor_mae"], [m["mae"][OBS[k]] for k, m in enumerate(failed)])
    np.testing.assert_array_equal(rep["delta_nonsensor_mae"], [m["nonsensor_mae"] - base["nonsensor_mae"] for m in failed])
    assert np.isfinite(rep["failed_sensor_mae"]).all() and np.isnan(base["mae"][OBS]).all()
    assert base["nonsensor_mae"] == est.error_map(store)["hidden_mae"]
    for m in failed:                                               # like against like: the same pool of 34 nodes x 7 snapshots
        assert m["hidden_count"].sum() - S == base["hidden_count"].sum() == S * (N37 - 3)
    part = est.sensor_failure_report(store, sensors=[2, 0])
    assert part["sensors"] == [2, 0]
    np.testing.assert_array_equal(part["nonsensor_mae"], rep["nonsensor_mae"][[2, 0]])
    np.testing.assert_array_equal(part["failed_sensor_mae"], rep["failed_sensor_mae"][[2, 0]])
    with pytest.raises(ValueError, match="sensors"):
        est.sensor_failure_report(store, sensors=[3])


# ---- 8. synchronisation ---------------------------------------------------------------------------------------------------------------
def test_no_read_back_in_the_passes_with_gaps_and_one_in_error_map(pkg, oracle, monkeypatch):
    store = make_store(pkg, 7)
    model, _ = small_model(pkg, oracle)
    est = pkg.PressureEstimator.for_store(model, store, OBS, batch_size=3)
    av = avail(ROWS7)
    readings = raw_snapshots(pkg, 7).to(DEV)[:, OBS].contiguous()
    nan_readings = readings.clone()
    nan_readings[~av.bool()] = float("nan")
    est.estimate_store(store)                                       # plans and buffers exist from here on
    torch.cuda.synchronize()
    calls = {"synchronize": 0, "item": 0, "cpu": 0, "tolist": 0, "float": 0, "stream_sync": 0, "event_sync": 0}

    def spy(name, fn):
        def wrapped(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return wrapped

    monkeypatch.setattr(torch.cuda, "synchronize", spy("synchronize", torch.cuda.synchronize))
    monkeypatch.setattr(torch.Tensor, "item", spy("item", torch.Tensor.item))
    monkeypatch.setattr(torch.Tensor, "cpu", spy("cpu", torch.Tensor.cpu))
    monkeypatch.setattr(torch.Tensor, "tolist", spy("tolist", torch.Tensor.tolist))
    monkeypatch.setattr(torch.Tensor, "__float__", spy("float", torch.Tensor.__float__))
    monkeypatch.setattr(torch.cuda.Stream, "synchronize", spy("stream_sync", torch.cuda.Stream.synchronize))
    monkeypatch.setattr(torch.cuda.Event, "synchronize", spy("event_sync", torch.cuda.Event.synchronize))
    a = est.estimate_store(store, available=av)
    b = est.estimate(readings, available=av)
    c = est.estimate(nan_readings, nan_is_missing=True)
    d = est.estimate(nan_readings, available=av, nan_is_missing=True)
    assert all(v == 0 for v in calls.values()), calls
    m = est.error_map(store, estimates=a, available=av)
    assert calls == {"synchronize": 0, "item": 0, "cpu": 1, "tolist": 0, "float": 0, "stream_sync": 0, "event_sync": 0}
    monkeypatch.undo()
    assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d) and np.isfinite(m["missing_sensor_mae"])


# ---- 9. gatres_small ----------------------------------------------------------------------------------------------------------------
def test_gatres_small_at_batch_32_takes_the_window_kernel(pkg, oracle, monkeypatch):
    n, pipes, S = 388, 430, 40
    store = make_store(pkg, S, n=n, pipes=pipes, seed=4)
    model, p = small_model(pkg, oracle, nb=15, nc=32, seed=11)
    plan = model.plan_for(store.edge_index(32), 32 * n)
    assert model._call_state(plan)["window"], "gatres_small at bs 32 should take the window kernel"
    sensors = [3, 17, 100, 101, 250, 387, 42, 9, 300, 77, 211, 5, 64, 128, 199, 350, 1, 260, 333, 150]
    av = (torch.rand((S, len(sensors)), generator=torch.Generator().manual_seed(7)) >= 0.3).to(torch.uint8).to(DEV)
    assert 0.2 < 1.0 - float(av.float().mean()) < 0.4
    est = pkg.PressureEstimator.for_store(model, store, sensors, batch_size=32)
    got = est.estimate_store(store, available=av)
    want, batches = hand_loop_available(pkg, monkeypatch, model, store, sensors, 32, av)
    assert [b[2] for b in batches] == [32, 8]
    assert torch.equal(got, want)
    check_against_module(pkg, model, store, batches)
    check_against_oracle(oracle, p, 15, store, batches[1:])          # (the ragged batch: 8 graphs on the host)


# ---- 10. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_on_the_device(pkg, oracle):
    store = make_store(pkg, 4)
    model, _ = small_model(pkg, oracle)
    est = pkg.PressureEstimator.for_store(model, store, OBS)
    readings = torch.zeros((4, 3), dtype=torch.float32, device=DEV)
    good = torch.ones((4, 3), dtype=torch.uint8, device=DEV)
    bad = {"host": good.cpu(), "dtype": good.float(), "int": good.int(), "shape": good[:, :2].contiguous(), "flat": good.reshape(-1),
           "non_contiguous": torch.ones((4, 6), dtype=torch.uint8, device=DEV)[:, ::2],
           "length": torch.ones((5, 3), dtype=torch.uint8, device=DEV), "list": [[1, 1, 1]] * 4}
    for name, b in bad.items():
        with pytest.raises(ValueError, match="available"):
            est.estimate(readings, available=b)
        with pytest.raises(ValueError, match="available"):
            est.estimate(readings, available=b, nan_is_missing=True)
        with pytest.raises(ValueError, match="available"):
            est.estimate_store(store, available=b)
        with pytest.raises(ValueError, match="available"):
            est.error_map(store, available=b)
        with pytest.raises(ValueError, match="available"):
            est.error_map(store, estimates=torch.empty((4, N37), device=DEV), available=b)
    assert est.estimate(readings, available=good).shape == (4, N37)          # (the good one passes)
    multi = pkg.MultiSnapshotStore([(raw_snapshots(pkg, 3), topology(pkg))] * 2, device="cpu")
    for call in (est.sensor_failure_report, est.estimate_store, est.error_map):          # MultiSnapshotStore stays refused
        with pytest.raises(ValueError, match="out of scope"):
            call(multi)
