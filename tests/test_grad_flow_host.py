"""Gradient flow on the host: ``evaluation.get_gradient_norm`` (the reference's utils/auxil.py:295-313 for a module trained
through ``loss.backward()``) and the C-ABI side of the device report -- the symbols of k_grad_flow.hip, declared in
include/gatres.h and bound in _native.py.  No GPU, no kernel launches."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gatres_grad_flow", "gatres_grad_flow_count", "gatres_mean_abs_diff")


def _model_with_grads(pkg, nb=2, nc=4, seed=5):
    torch.manual_seed(seed)
    model = pkg.GATResMeanConv(num_blocks=nb, nc=nc)
    g = torch.Generator().manual_seed(seed + 1)
    for p in model.parameters():
        p.grad = torch.randn(p.shape, generator=g) * 3.0
    return model


def test_get_gradient_norm_reports_the_block_parameters_in_named_parameters_order(pkg):
    model = _model_with_grads(pkg)
    total, norms, names = pkg.evaluation.get_gradient_norm(model, norm_type=2)
    want = [n for n, _ in model.named_parameters() if "block" in n]
    assert names == want and len(names) == 8 * model.num_blocks == len(norms)
    assert [n.rsplit(".", 1)[-1] for n in names[:8]] == ["att_src", "att_dst", "bias", "weight"] * 2
    assert all(n.startswith("blocks.0.conv1.") for n in names[:4]) and all(n.startswith("blocks.0.conv2.") for n in names[4:8])
    assert not any(n.startswith(("lin0", "lin1")) for n in names)
    params = dict(model.named_parameters())
    for n, v in zip(names, norms):
        assert torch.equal(v, torch.norm(params[n].grad, p=2)), n
    assert torch.equal(total, torch.norm(torch.stack(norms), 2))
    assert total.dim() == 0 and float(total) > 0.0


def test_get_gradient_norm_ignores_lin0_and_lin1_and_follows_norm_type(pkg):
    model = _model_with_grads(pkg)
    total, norms, _ = pkg.evaluation.get_gradient_norm(model)
    model.lin0.weight.grad.mul_(100.0)
    model.lin1.bias.grad.fill_(float("nan"))
    total2, norms2, _ = pkg.evaluation.get_gradient_norm(model)
    assert torch.equal(total, total2) and all(torch.equal(a, b) for a, b in zip(norms, norms2))
    t1, n1, names = pkg.evaluation.get_gradient_norm(model, norm_type=1)
    params = dict(model.named_parameters())
    assert all(torch.equal(v, torch.norm(params[n].grad, p=1)) for n, v in zip(names, n1))
    assert torch.equal(t1, torch.norm(torch.stack(n1), 1))


def test_get_gradient_norm_refuses_a_model_without_gradients(pkg):
    model = pkg.GATResMeanConv(num_blocks=1, nc=4)
    with pytest.raises(ValueError, match="backward"):
        pkg.evaluation.get_gradient_norm(model)


def test_layout_order_is_named_parameters_order(pkg):
    """gatres_grad_flow walks the flat layout; the names come from named_parameters(): both must be the same sequence of
    tensors -- per block 2nc, 2nc, 2nc, 2nc * nc, nc, nc, nc, nc * 2nc floats, right behind lin0's 2nc."""
    for nb, nc in ((1, 4), (3, 32)):
        model = pkg.GATResMeanConv(num_blocks=nb, nc=nc)
        flat = model.flat_parameters
        params = dict(model.named_parameters())
        off = 2 * nc
        sizes = [2 * nc, 2 * nc, 2 * nc, 2 * nc * nc, nc, nc, nc, 2 * nc * nc]
        for i, n in enumerate(pkg.evaluation.gradient_flow_names(model)):
            p = params[n]
            assert p.numel() == sizes[i % 8], n
            assert p.data_ptr() == flat.data_ptr() + 4 * off, n
            off += p.numel()
        assert off + nc + 1 == flat.numel()


def test_new_symbols_are_declared_exported_and_bound(pkg, lib):
    with open(os.path.join(ROOT, "include", "gatres.h")) as f:
        hdr = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in pkg._native.SIGNATURES
    assert "#define GATRES_ABI_VERSION 9" in hdr and pkg._native.ABI_VERSION == 9        # symbols only: the ABI stays


@pytest.mark.parametrize("nb,nc", [(1, 4), (2, 8), (15, 32), (25, 128)])
def test_grad_flow_count(lib, nb, nc):
    assert lib.gatres_grad_flow_count(nb, nc) == 8 * nb
    assert lib.gatres_grad_flow_count(0, nc) == 0


def test_entry_points_check_their_arguments_before_any_launch(pkg, lib):
    """Null pointers, sizes and widths are refused on the host (no device is touched)."""
    N = pkg._native
    import ctypes as C
    m = N.GatresModel(2, 8, 0, 0)
    p = 4096                       # (any non-null address: a refused call never reads it)
    assert lib.gatres_grad_flow(None, p, 1.0, None, p, None) == -1
    assert lib.gatres_grad_flow(C.byref(m), None, 1.0, None, p, None) == -1
    assert lib.gatres_grad_flow(C.byref(m), p, 1.0, None, None, None) == -1
    assert lib.gatres_grad_flow(C.byref(N.GatresModel(0, 8, 0, 0)), p, 1.0, None, p, None) == -1
    assert lib.gatres_grad_flow(C.byref(N.GatresModel(2, 12, 0, 0)), p, 1.0, None, p, None) == -2
    assert lib.gatres_grad_flow(C.byref(N.GatresModel(2, 256, 0, 0)), p, 1.0, None, p, None) == -2
    assert lib.gatres_mean_abs_diff(None, p, 4, p, None) == -1
    assert lib.gatres_mean_abs_diff(p, None, 4, p, None) == -1
    assert lib.gatres_mean_abs_diff(p, p, 4, None, None) == -1
    assert lib.gatres_mean_abs_diff(p, p, 0, p, None) == -1
    assert lib.gatres_mean_abs_diff(p, p, -3, p, None) == -1


def test_fit_history_has_the_gradient_lists_empty(pkg):
    h = pkg.FitHistory()
    assert h.total_grad_norm == [] and h.block_norms == [] and h.block_names == [] and h.model_update == []
    assert h.accum_model_update == []
