"""CPU side of the training criteria (train.py --criterion {mse,mae,sce}): evaluation.sce_loss / get_criterion against hand
values, GATResTrainer's refusal of an unknown criterion before it touches the library or the device, and the criterion
constants of include/gatres.h against the ctypes side.  No GPU."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "gatres.h")).read()


def _define(name):
    m = re.search(rf"#define\s+{name}\s+(\d+)", _header())
    assert m, name
    return int(m.group(1))


def test_get_criterion_returns_the_references_callables(pkg):
    E = pkg.evaluation
    assert isinstance(E.get_criterion("mse"), torch.nn.MSELoss) and E.get_criterion("mse").reduction == "mean"
    assert isinstance(E.get_criterion("mae"), torch.nn.L1Loss) and E.get_criterion("mae").reduction == "mean"
    assert E.get_criterion("sce") is E.sce_loss
    with pytest.raises(KeyError):
        E.get_criterion("huber")
    o = torch.tensor([[0.5], [-2.0], [3.0]])
    y = torch.tensor([[1.0], [1.0], [3.0]])
    assert float(E.get_criterion("mse")(o, y)) == pytest.approx((0.25 + 9.0 + 0.0) / 3)
    assert float(E.get_criterion("mae")(o, y)) == pytest.approx((0.5 + 3.0 + 0.0) / 3)


def test_sce_loss_hand_values_and_the_eps_branch(pkg):
    sce = pkg.evaluation.sce_loss
    d = torch.float64
    # [M, 1]: the normalised values are +-1, t = 1 - sign(o) sign(y) is 0 or 2, the loss the mean of t^3
    o = torch.tensor([[0.5], [-2.0], [3.0], [-1.0]], dtype=d)
    y = torch.tensor([[1.0], [1.0], [3.0], [-7.0]], dtype=d)
    assert float(sce(o, y)) == pytest.approx((0 + 8 + 0 + 0) / 4)
    # below eps the prediction is divided by eps, not by its norm: o = 5e-13 -> o^ = 0.5, t = 0.5, t^3 = 0.125
    o = torch.tensor([[5e-13], [0.0]], dtype=d)
    y = torch.tensor([[2.0], [0.0]], dtype=d)
    assert float(sce(o, y)) == pytest.approx((0.125 + 1.0) / 2)
    # its gradient there: -3 t^2 y^ / (eps M); at |o| >= eps the (exact) gradient vanishes
    o = torch.tensor([[5e-13], [1e-12], [0.3]], dtype=d, requires_grad=True)
    y = torch.tensor([[2.0], [2.0], [2.0]], dtype=d)
    sce(o, y).backward()
    g = o.grad.reshape(-1)
    assert float(g[0]) == pytest.approx(-3 * 0.25 * 1.0 / (1e-12 * 3), rel=1e-12)
    assert abs(float(g[1])) < 1e-3 * abs(float(g[0])) and abs(float(g[2])) < 1e-9
    # multi-column rows: a cosine error
    a = torch.tensor([[1.0, 0.0], [1.0, 1.0]], dtype=d)
    b = torch.tensor([[0.0, 2.0], [2.0, 2.0]], dtype=d)
    assert float(sce(a, b)) == pytest.approx((1.0 + 0.0) / 2)


def test_trainer_refuses_an_unknown_criterion_before_touching_the_device(pkg, monkeypatch):
    def no_library():
        raise AssertionError("the criterion must be checked before the library is loaded")

    monkeypatch.setattr(pkg._native, "load", no_library)
    for bad in ("huber", "MSE", "", None, 1):
        with pytest.raises(ValueError, match="criterion"):
            pkg.GATResTrainer(None, None, 0, criterion=bad)


def test_criterion_constants_of_the_header_and_the_python_side(pkg):
    N = pkg._native
    TS = pkg.train_step
    assert _define("GATRES_ABI_VERSION") == N.ABI_VERSION == 9
    assert (_define("GATRES_LOSS_MSE"), _define("GATRES_LOSS_MAE"), _define("GATRES_LOSS_SCE")) == \
        (N.LOSS_MSE, N.LOSS_MAE, N.LOSS_SCE) == (0, 1, 2)
    assert N.CRITERIA == {"mse": 0, "mae": 1, "sce": 2}
    assert (_define("GATRES_FLAG_LOSS_MAE"), _define("GATRES_FLAG_LOSS_SCE")) == (TS.FLAG_LOSS_MAE, TS.FLAG_LOSS_SCE) == (32, 64)
    flags = [_define(k) for k in ("GATRES_FLAG_PER_OP", "GATRES_FLAG_WT_VALID", "GATRES_FLAG_GRADS_DEFERRED",
                                  "GATRES_FLAG_GRADS_ONLY", "GATRES_FLAG_MASK_NEXT", "GATRES_FLAG_LOSS_MAE",
                                  "GATRES_FLAG_LOSS_SCE")]
    assert sum(flags) == 127 and len(set(flags)) == 7                   # distinct bits
    phases = [_define(k) for k in ("GATRES_PHASE_FORWARD", "GATRES_PHASE_BACKWARD", "GATRES_PHASE_LOSS",
                                   "GATRES_PHASE_LOSS_MAE", "GATRES_PHASE_LOSS_SCE")]
    assert sum(phases) == 2 + 4 + 16 + 32 + 64
    # gatres_masked_loss(out, y, mask, criterion, loss, g_out, num_nodes, stream)
    import ctypes as C
    res, args = N.SIGNATURES["gatres_masked_loss"]
    assert res is C.c_int and len(args) == 8 and args[3] is C.c_int32 and args[6] is C.c_int32
    assert re.search(r"int gatres_masked_loss\(const float\* out, const float\* y, const uint8_t\* mask, int32_t criterion,\s*"
                     r"float\* loss, float\* g_out,\s*int32_t num_nodes, void\* stream\);", _header())
