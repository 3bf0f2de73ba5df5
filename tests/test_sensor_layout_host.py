"""Fine-tuning to a fixed sensor layout, on the host: ``gatres_stage_rows_mask_sensors`` is declared, exported and bound without
an ABI change and refuses its bad arguments before any launch; ``sensor_layout_draws`` holds on known answers (computed with
an independent restatement of the header's draws); ``set_sensor_layout`` and ``evaluate_store(observed_idx=...)`` refuse what
they can refuse without a device.  No GPU, no kernel launches."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "gatres_stage_rows_mask_sensors"
P = 4096                       # (any non-null address: a refused call never reads it)
Q = 8192
BADARG = -1


def header():
    with open(os.path.join(ROOT, "include", "gatres.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


# ---- 1. the symbol and its refusals ---------------------------------------------------------------------------------------------
def test_the_symbol_is_declared_exported_and_bound_and_the_abi_stays(pkg, lib):
    hdr = header()
    assert re.search(r"\b%s\s*\(" % SYMBOL, hdr)
    assert hdr.index("gatres_stage_rows_mask_required(") < hdr.index(SYMBOL + "(") < hdr.index("gatres_stage_multi_rows_mask_required(")
    assert hasattr(lib, SYMBOL), f"{SYMBOL} is not exported"
    assert len(pkg._native.SIGNATURES[SYMBOL][1]) == 16
    assert "#define GATRES_ABI_VERSION 9" in hdr and pkg._native.ABI_VERSION == 9
    assert pkg.sensor_layout_draws is pkg.sensor_layout.sensor_layout_draws


def stage(lib, data=P, rows=2 * P, n=37, x=Q, y=None, node_ptr=3 * P, graphs=3, observed=5 * P, k=5, dropout=0.3, share=0.6,
          rate=0.95, seed=9, step=None, mask=3 * Q):
    return lib.gatres_stage_rows_mask_sensors(data, rows, n, x, y, node_ptr, graphs, observed, k, dropout, share, rate, seed, step,
                                              mask, None)


def test_the_symbol_checks_its_arguments_before_any_launch(pkg, lib):
    assert pkg._native.ERRORS[BADARG]                            # (GATRES_E_BADARG)
    for name in ("data", "rows", "x", "node_ptr", "observed", "mask"):
        assert stage(lib, **{name: None}) == BADARG, name
    assert stage(lib, x=P) == BADARG                             # data == x_dst
    assert stage(lib, graphs=0) == BADARG and stage(lib, graphs=-2) == BADARG
    assert stage(lib, n=0) == BADARG and stage(lib, n=-1) == BADARG
    assert stage(lib, k=0) == BADARG and stage(lib, k=-1) == BADARG and stage(lib, k=38) == BADARG
    for bad in (-0.01, 1.0, 1.5, float("nan")):
        assert stage(lib, dropout=bad) == BADARG, bad
    for bad in (-0.01, 1.01, float("nan")):
        assert stage(lib, share=bad) == BADARG, bad
        assert stage(lib, rate=bad) == BADARG, bad


# ---- 2. the host restatement ----------------------------------------------------------------------------------------------------
def test_the_hashes_and_thresholds_on_known_answers(pkg):
    L = pkg.sensor_layout
    assert L.mode_hashes(9, 0, [0, 1, 2]).tolist() == [1023227, 11581052, 15940783]
    assert L.node_hashes(9, 0, [0, 3, 37, 72]).tolist() == [2773164, 13380171, 765258, 11351884]
    assert L.threshold(0.3) == 5033164 and L.threshold(0.6) == 10066329
    assert L.threshold(0.0) == 0 and L.threshold(1.0) == 1 << 24


def test_sensor_layout_draws_on_a_full_case(pkg):
    mode, keep = pkg.sensor_layout_draws(9, 0, 5, 37, [0, 3, 17, 35, 36], 0.3, 0.6)
    T, F = True, False
    assert mode.dtype == np.bool_ and keep.dtype == np.bool_ and mode.shape == (5,) and keep.shape == (5, 5)
    assert mode.tolist() == [T, F, F, T, T]
    assert keep.tolist() == [[F, T, T, T, T], [F, T, T, T, F], [T, T, F, T, F], [T, T, F, F, F], [T, F, T, T, F]]
    # the step enters: other draws
    mode1, keep1 = pkg.sensor_layout_draws(9, 1, 5, 37, [0, 3, 17, 35, 36], 0.3, 0.6)
    assert mode1.tolist() != mode.tolist() or keep1.tolist() != keep.tolist()
    # 64-bit wrap-around of seed + golden * (step + 1) is modular, not an error
    pkg.sensor_layout_draws((1 << 64) - 1, (1 << 63), 2, 37, [1], 0.5, 0.5)


def test_the_limits_of_dropout_and_share(pkg):
    obs = [0, 3, 17, 35, 36]
    for seed, step in ((9, 0), (9, 1), (123456789, 77)):
        mode, keep = pkg.sensor_layout_draws(seed, step, 33, 37, obs, 0.0, 1.0)
        assert keep.all() and mode.all()
        mode, _ = pkg.sensor_layout_draws(seed, step, 33, 37, obs, 0.3, 0.0)
        assert not mode.any()
    for bad in (-0.1, 1.0):
        with pytest.raises(ValueError, match="sensor_dropout"):
            pkg.sensor_layout_draws(9, 0, 5, 37, obs, bad, 0.5)
    for bad in (-0.1, 1.1):
        with pytest.raises(ValueError, match="layout_share"):
            pkg.sensor_layout_draws(9, 0, 5, 37, obs, 0.1, bad)


# ---- 3. refusals in Python ------------------------------------------------------------------------------------------------------
def stub_trainer(pkg, world=1, recipe=None, npg=(37, 37)):
    """What set_sensor_layout reads of a trainer before it uploads anything."""
    import torch
    t = pkg.GATResTrainer.__new__(pkg.GATResTrainer)
    t.world, t._recipe, t._npg_list, t._siblings, t._layout = world, recipe, list(npg) if npg else None, {}, None
    t.node_ptr = None if not npg else torch.zeros(len(npg) + 1, dtype=torch.int32)
    t.device = torch.device("cpu")
    t._mask_sig = None
    return t


def test_set_sensor_layout_refusals_that_need_no_device(pkg):
    t = stub_trainer(pkg)
    with pytest.raises(ValueError, match="empty"):
        t.set_sensor_layout([])
    with pytest.raises(ValueError, match="observed_idx"):
        t.set_sensor_layout([0, 37])
    with pytest.raises(ValueError, match="observed_idx"):
        t.set_sensor_layout([-1])
    with pytest.raises(ValueError, match="duplicates"):
        t.set_sensor_layout([1, 2, 1])
    with pytest.raises(ValueError, match="sensor_dropout"):
        t.set_sensor_layout([1, 2], sensor_dropout=1.0)
    with pytest.raises(ValueError, match="layout_share"):
        t.set_sensor_layout([1, 2], layout_share=1.5)
    assert t.sensor_layout is None
    with pytest.raises(NotImplementedError, match="world size 2"):
        stub_trainer(pkg, world=2).set_sensor_layout([1, 2])
    with pytest.raises(NotImplementedError, match="MultiSnapshotStore"):
        stub_trainer(pkg, recipe=(1, 1)).set_sensor_layout([1, 2])
    with pytest.raises(ValueError, match="nodes_per_graph"):
        stub_trainer(pkg, npg=None).set_sensor_layout([1, 2])
    with pytest.raises(ValueError, match="nodes_per_graph"):
        stub_trainer(pkg, npg=(37, 38)).set_sensor_layout([1, 2])
    # a good one is held, described and handed to the siblings that exist; clearing takes it from them too
    sib = stub_trainer(pkg, npg=(37,))
    t._siblings[1] = sib
    t.set_sensor_layout([3, 1, 36], sensor_dropout=0.25, layout_share=0.5)
    want = {"observed_idx": [3, 1, 36], "sensor_dropout": 0.25, "layout_share": 0.5}
    assert t.sensor_layout == want and sib.sensor_layout == want
    assert t._layout.observed.tolist() == [3, 1, 36] and str(t._layout.observed.dtype) == "torch.int32"
    for call in (lambda: t.step(None, None), lambda: t.run_step(), lambda: t.bind_batches([]), lambda: t.step_bound(0),
                 lambda: t.steps_bound([0, 1]), lambda: t.step_prefetched()):
        with pytest.raises(ValueError, match="sensor layout"):
            call()
    t.clear_sensor_layout()
    assert t.sensor_layout is None and sib.sensor_layout is None


def test_evaluate_store_refuses_the_options_a_layout_excludes(pkg):
    class Store:                                                 # (what evaluate_store reads of a store before the refusals)
        nodes_per_graph = 37

    ev = pkg.evaluation.evaluate_store
    model = object()
    with pytest.raises(ValueError, match="do_test_on_sensors"):
        ev(model, Store(), 4, 0.95, observed_idx=[1, 2], do_test_on_sensors=True, required_idx=[5])
    with pytest.raises(ValueError, match="required_idx"):
        ev(model, Store(), 4, 0.95, observed_idx=[1, 2], required_idx=[5])
    with pytest.raises(ValueError, match="use_same_mask"):
        ev(model, Store(), 4, 0.95, observed_idx=[1, 2], use_same_mask=True)
    multi = pkg.MultiSnapshotStore.__new__(pkg.MultiSnapshotStore)
    with pytest.raises(NotImplementedError, match="MultiSnapshotStore"):
        ev(model, multi, 4, 0.95, observed_idx=[1, 2])
    with pytest.raises(NotImplementedError, match="MultiSnapshotStore"):
        pkg.evaluation._ValidationPass(model, multi, 4, 0.95, observed_idx=[1, 2])
