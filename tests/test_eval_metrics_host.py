"""CPU tests of the host half of the device evaluation epoch: ``metrics_from_moments`` over moment records (the layout
``gatres_masked_metrics`` writes, computed here by ``masked_metric_moments``) against the reference's metric functions and
``MSELoss`` on the same tensors, the graph-count weighting, and the refusal of other criteria / metric collections.
No GPU."""
import math

import numpy as np
import pytest
import torch

import metric_moments_ref as MR      # noqa: E402


def reference_batch(E, out, y, mask, norm, **kw):
    """What test_one_epoch computes for one batch: MSELoss on scaled values, the seven metrics on descaled values."""
    o, t, m = torch.from_numpy(out), torch.from_numpy(y), torch.from_numpy(mask)
    yp, yt = o[m], t[m]
    pr, tr = E.descale(yp, norm, **kw), E.descale(yt, norm, **kw)
    res = {"loss": float(torch.nn.MSELoss()(yp, yt))}
    for k, fn in E.get_metric_fn_collection("test").items():
        res[k] = float(fn(pr, tr))
    return res


def affine(norm, kw):
    """(scale, offset) of descale(): znorm -> (std, mean), minmax -> (max - min, min)."""
    return (kw["std"], kw["mean"]) if norm == "znorm" else (kw["max"] - kw["min"], kw["min"])


def assert_close(a, b, rel, what):
    if math.isnan(b):
        assert math.isnan(a), f"{what}: {a} vs NaN"
        return
    assert abs(a - b) <= rel * max(abs(b), 1e-30), f"{what}: {a} vs {b}"


NORMS = [("znorm", dict(mean=51.37, std=12.81)), ("minmax", dict(min=3.25, max=97.6))]


@pytest.mark.parametrize("norm,kw", NORMS)
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_metrics_from_moments_matches_reference_functions(pkg, norm, kw, seed):
    E = pkg.evaluation
    rng = np.random.RandomState(seed)
    n = 32 * 388
    y = (rng.rand(n).astype(np.float32) if norm == "minmax" else rng.randn(n).astype(np.float32))
    out = (y + 0.05 * rng.randn(n).astype(np.float32)).astype(np.float32)       # a trained model's predictions
    mask = rng.rand(n) < 0.95
    scale, offset = affine(norm, kw)
    rec = MR.masked_metric_moments(out, y, mask, scale, offset)
    loss, m = E.metrics_from_moments(rec[None], [32], "test")
    ref = reference_batch(E, out, y, mask, norm, **kw)
    assert_close(loss, ref["loss"], 1e-6, "loss")
    for k, v in m.items():
        assert_close(v, ref[k], 1e-6, k)
    # the two counts are exact: the record's predicates round as torch's do
    t = E.descale(torch.from_numpy(y)[torch.from_numpy(mask)], norm, **kw)
    p = E.descale(torch.from_numpy(out)[torch.from_numpy(mask)], norm, **kw)
    assert rec[9] == int((t.abs() > 0.01).sum())
    assert rec[11] == int(((t - p).abs() <= t * 0.1).sum())
    assert rec[0] == int(mask.sum())


def test_no_kept_element_gives_nan_error(pkg):
    E = pkg.evaluation
    rng = np.random.RandomState(5)
    y = (0.004 * rng.rand(500)).astype(np.float32)              # every |t| <= 0.01 after descale(mean 0, std 1)
    out = (y + 0.001 * rng.randn(500)).astype(np.float32)
    mask = rng.rand(500) < 0.5
    rec = MR.masked_metric_moments(out, y, mask, 1.0, 0.0)
    assert rec[9] == 0
    _, m = E.metrics_from_moments(rec[None], [1], "test")
    ref = reference_batch(E, out, y, mask, "znorm", mean=0.0, std=1.0)
    assert math.isnan(ref["test_error"]) and math.isnan(m["test_error"])
    for k in ("test_0.1", "test_corr", "test_mae", "test_rmse", "test_mynse"):
        assert_close(m[k], ref[k], 1e-6, k)


def test_constant_targets_give_nan_corr_and_r2(pkg):
    E = pkg.evaluation
    rng = np.random.RandomState(6)
    y = np.full(600, 0.5, dtype=np.float32)                     # descaled: exactly 50.0 (scale 4, offset 48)
    out = (y + 0.02 * rng.randn(600)).astype(np.float32)
    mask = rng.rand(600) < 0.6
    rec = MR.masked_metric_moments(out, y, mask, 4.0, 48.0)
    assert rec[7] == 0.0
    loss, m = E.metrics_from_moments(rec[None], [1], "test")
    ref = reference_batch(E, out, y, mask, "znorm", mean=48.0, std=4.0)
    assert math.isnan(ref["test_corr"]) and math.isnan(ref["test_r2"])
    assert math.isnan(m["test_corr"]) and math.isnan(m["test_r2"])
    assert_close(loss, ref["loss"], 1e-6, "loss")
    for k in ("test_error", "test_0.1", "test_mae", "test_rmse", "test_mynse"):
        assert_close(m[k], ref[k], 1e-6, k)


def test_graph_count_weighting_is_the_reference_formula(pkg):
    """train.py:278-279 / evaluation.py:340-345: total += metric(batch) * num_graphs; metric = total / len(dataset)."""
    E = pkg.evaluation
    rng = np.random.RandomState(7)
    graphs = [32, 32, 32, 7]
    recs, per = [], []
    for g in graphs:
        n = g * 50
        y = rng.randn(n).astype(np.float32)
        out = (y + 0.1 * rng.randn(n)).astype(np.float32)
        mask = rng.rand(n) < 0.9
        recs.append(MR.masked_metric_moments(out, y, mask, 12.5, 50.0))
        per.append(E.metrics_from_moments(recs[-1][None], [g], "val"))
    loss, m = E.metrics_from_moments(np.stack(recs), graphs, "val")
    n = sum(graphs)
    assert loss == pytest.approx(sum(l * g for (l, _), g in zip(per, graphs)) / n, rel=1e-14)
    assert list(m) == list(E.get_metric_fn_collection("val"))
    for k in m:
        assert m[k] == pytest.approx(sum(p[k] * g for (_, p), g in zip(per, graphs)) / n, rel=1e-14)
    with pytest.raises(ValueError):
        E.metrics_from_moments(np.stack(recs), graphs[:-1], "val")


def test_evaluate_store_refuses_other_criteria_and_metrics(pkg):
    E = pkg.evaluation
    with pytest.raises(ValueError, match="MSELoss"):
        E.evaluate_store(None, None, 32, 0.95, criterion=torch.nn.L1Loss())
    fns = E.get_metric_fn_collection("test")
    fns["test_mae"] = E.calculate_rmse
    with pytest.raises(ValueError, match="get_metric_fn_collection"):
        E.evaluate_store(None, None, 32, 0.95, metric_fn_dict=fns)
    with pytest.raises(ValueError, match="get_metric_fn_collection"):
        E.evaluate_store(None, None, 32, 0.95, prefix="val", metric_fn_dict=E.get_metric_fn_collection("test"))
    # the reference's own collection and criterion are accepted (the call then fails on the missing store, not on them)
    with pytest.raises(AttributeError):
        E.evaluate_store(None, None, 32, 0.95, criterion=torch.nn.MSELoss(), metric_fn_dict=E.get_metric_fn_collection("test"))
