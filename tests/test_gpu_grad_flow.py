"""Gradient flow and model update per epoch (the reference's ``--log_gradient``, train.py:476-504) on the device:

* ``gatres_grad_flow`` against fp64 torch on the tensors of the flat layout -- both sides sum exact fp64 products of fp32
  values, so each sum is off by at most n * 2^-53 <= 3.7e-12 for n <= 32 768: ``rtol = 1e-11``;
* ``gatres_mean_abs_diff`` against ``(a - b).abs().double().mean()`` (n <= 4097 terms: ``rtol = 1e-12``), and past the
  kernel's first trip of 8192 elements against numpy within the reordering bound 2 n 2^-53;
* ``GATResTrainer.gradient_flow()`` on the fused and the per-op path, with AutoClip, under bf16 storage;
* ``fit(log_gradient=True, on_epoch=...)``: training untouched bit for bit, the report equal bit for bit to a hand-written loop
  over ``fit_epoch`` + ``gradient_flow()`` + ``gatres_mean_abs_diff``."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from turnover_cases import MEAN_ABS_DIFF_N      # noqa: E402

DEV = "cuda:0"
RTOL = 1e-11
NODES, PIPES = 24, 28


def tensor_sizes(nc):
    """Floats of the eight parameter tensors of one block, in the flat layout's (= named_parameters()) order."""
    return [2 * nc, 2 * nc, 2 * nc, 2 * nc * nc, nc, nc, nc, 2 * nc * nc]


def tensor_ranges(nb, nc):
    off, out = 2 * nc, []
    for _ in range(nb):
        for n in tensor_sizes(nc):
            out.append((off, off + n))
            off += n
    return out


def expected_flow(flat, nb, nc, factor=1.0):
    """[total, norm_0, ...] in fp64 torch on the CPU from a flat fp32 vector."""
    f = flat.detach().cpu()
    norms = torch.stack([torch.linalg.vector_norm(f[lo:hi].double()) for lo, hi in tensor_ranges(nb, nc)])
    return torch.cat([torch.linalg.vector_norm(norms).reshape(1), norms]) * factor


def run_flow(pkg, lib, flat, nb, nc, scale, coef, guard=4):
    m = pkg._native.GatresModel(nb, nc, 0, 0)
    T = 8 * nb
    out = torch.full((1 + T + guard,), -7.25, dtype=torch.float64, device=DEV)
    rc = lib.gatres_grad_flow(C.byref(m), flat.data_ptr(), scale, None if coef is None else coef.data_ptr(), out.data_ptr(), None)
    assert rc == 0
    torch.cuda.synchronize()
    assert bool((out[1 + T:] == -7.25).all())                                   # nothing behind the 1 + 8 * num_blocks values
    return out[:1 + T].cpu()


def close(got, want, rtol):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return bool(np.all(np.abs(got - want) <= rtol * np.abs(want)))


# ---- 1. the kernel against fp64 torch -------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb,nc", [(1, 4), (2, 8), (3, 32), (2, 128)])
def test_grad_flow_kernel_equals_fp64_torch(pkg, lib, nb, nc):
    P = int(lib.gatres_param_count(nb, nc))
    assert lib.gatres_grad_flow_count(nb, nc) == 8 * nb
    ranges = tensor_ranges(nb, nc)
    assert ranges[-1][1] + nc + 1 == P
    g = torch.Generator().manual_seed(100 * nb + nc)
    flat = (torch.randn(P, generator=g) * torch.logspace(-3, 2, P)[torch.randperm(P, generator=g)]).float()
    zeroed = len(ranges) // 2
    flat[ranges[zeroed][0]:ranges[zeroed][1]] = 0.0
    dflat = flat.to(DEV)
    want = expected_flow(flat, nb, nc)
    assert want[1 + zeroed] == 0.0 and bool((want[torch.arange(len(want)) != 1 + zeroed] > 0).all())
    coef = torch.tensor([0.25], dtype=torch.float64, device=DEV)
    a = run_flow(pkg, lib, dflat, nb, nc, 0.5, coef)
    assert close(a, want * 0.125, RTOL), (a - want * 0.125) / want
    assert a[1 + zeroed] == 0.0                                                   # an all-zero tensor gives 0
    b = run_flow(pkg, lib, dflat, nb, nc, 0.5, None)
    assert close(b, want * 0.5, RTOL)
    assert torch.equal(a, b * 0.25)                                               # (powers of two scale exactly)
    assert torch.equal(run_flow(pkg, lib, dflat, nb, nc, -0.5, None), b)          # |scale|
    assert torch.equal(run_flow(pkg, lib, dflat, nb, nc, 0.5, coef).view(torch.int64), a.view(torch.int64))    # the same bits again
    # floats in lin0 / lin1 change nothing
    moved = dflat.clone()
    moved[:2 * nc] = 1e6
    moved[-(nc + 1):] = float("nan")
    assert torch.equal(run_flow(pkg, lib, moved, nb, nc, 0.5, coef).view(torch.int64), a.view(torch.int64))
    # a NaN in one tensor: NaN there and in the total, every other value untouched
    t_nan = 3 if nb == 1 else 8 + 6                                               # a weight matrix / a short vector
    bad = dflat.clone()
    lo, hi = ranges[t_nan]
    bad[lo + (hi - lo) // 2] = float("nan")
    c = run_flow(pkg, lib, bad, nb, nc, 0.5, coef)
    assert math.isnan(c[0]) and math.isnan(c[1 + t_nan])
    keep = torch.ones(1 + 8 * nb, dtype=torch.bool)
    keep[0] = keep[1 + t_nan] = False
    assert torch.equal(c[keep].view(torch.int64), a[keep].view(torch.int64))


# ---- 2. mean |a - b| ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097] + MEAN_ABS_DIFF_N)
def test_mean_abs_diff_equals_torch(pkg, lib, n):
    """n <= 4097: one trip of the kernel's loop (GF_U * GF_T = 8192 elements), against torch within 1e-12.  The sizes of
    tests/turnover_cases.py straddle the trip: against numpy on the host -- the difference in fp32, the sum in fp64 -- within
    2 n 2^-53 relative (n non-negative terms that are exact in fp64: only the order of the additions can differ, and either
    order is within (n - 1) 2^-53 of the exact sum)."""
    g = torch.Generator().manual_seed(n)
    a = (torch.randn(n, generator=g) * 3.0).float()
    b = (a + torch.randn(n, generator=g) * torch.logspace(-3, 0, n)).float()
    da, db = a.to(DEV), b.to(DEV)
    out = torch.full((3,), -7.25, dtype=torch.float64, device=DEV)
    assert lib.gatres_mean_abs_diff(da.data_ptr(), db.data_ptr(), n, out[1:].data_ptr(), None) == 0
    torch.cuda.synchronize()
    if n in MEAN_ABS_DIFF_N:
        d32 = a.numpy() - b.numpy()
        assert d32.dtype == np.float32
        want, bound = float(np.abs(d32).astype(np.float64).sum() / n), 2.0 * n * 2.0 ** -53
    else:
        want, bound = float((a - b).abs().double().mean()), 1e-12
    print(f"n = {n}: relative difference {abs(float(out[1]) - want) / want:.3e} (bound {bound:.3e})")
    assert want > 0.0 and abs(float(out[1]) - want) <= bound * want, (float(out[1]), want)
    assert float(out[0]) == -7.25 and float(out[2]) == -7.25
    assert lib.gatres_mean_abs_diff(da.data_ptr(), da.data_ptr(), n, out[1:].data_ptr(), None) == 0
    assert float(out[1].item()) == 0.0                                            # a == b: exactly 0
    assert lib.gatres_mean_abs_diff(da.data_ptr(), da.clone().data_ptr(), n, out[1:].data_ptr(), None) == 0
    assert float(out[1].item()) == 0.0


# ---- 3. the trainer -------------------------------------------------------------------------------------------------------
def _topology(pkg):
    return pkg.wdn_synth.make_wdn_topology(NODES, PIPES, seed=0, locality=6)


def _step_trainer(pkg, nb, nc, bs, fused, bf16=False, **kw):
    torch.manual_seed(11)
    model = pkg.GATResMeanConv(num_blocks=nb, nc=nc, fused=fused).cuda()
    if bf16:
        model.set_compute_dtype("bf16")
    ei = pkg.wdn_synth.collate_edge_index(_topology(pkg), NODES, bs).cuda()
    tr = pkg.GATResTrainer(model, ei, bs * NODES, nodes_per_graph=[NODES] * bs, targets_are_inputs=True, fused=fused, lr=5e-3,
                           mask_rate=0.5, **kw)
    x = pkg.wdn_synth.make_snapshots(bs, NODES, seed=2).reshape(-1).cuda()
    tr.load_batch(x, x)
    return model, tr


@pytest.mark.parametrize("case", ["fused", "per_op", "fused_clip", "per_op_clip", "per_op_bf16"])
def test_trainer_gradient_flow_describes_the_last_steps_gradient(pkg, lib, case):
    fused, clip, bf16 = case.startswith("fused"), case.endswith("clip"), case.endswith("bf16")
    nb, nc = (2, 32) if bf16 else (2, 8)
    model, tr = _step_trainer(pkg, nb, nc, 4, fused, bf16=bf16, use_gradient_clipping=clip, percentile=0.0)
    assert tr.fused == fused                             # (24-node snapshots at nc = 8 fit the per-snapshot kernel)
    for _ in range(3):                                   # (AutoClip, percentile 0: clipped to the smallest norm so far, coef < 1)
        tr.run_step()
    state = [t.clone() for t in (tr.grads, model.flat_parameters, tr.exp_avg, tr.exp_avg_sq, tr.step_counter)]
    total, norms, names = tr.gradient_flow()
    total2, norms2, _ = tr.gradient_flow()               # (the same buffer, the same bits)
    got = torch.cat([total.reshape(1), norms]).cpu()
    torch.cuda.synchronize()
    assert total.dtype == torch.float64 and total.dim() == 0 and total.is_cuda and tuple(norms.shape) == (8 * nb,)
    assert names == [n for n, _ in model.named_parameters() if "block" in n]
    factor = float(tr.last_clip_coef) if clip else 1.0
    if clip:
        assert 0.0 < factor < 1.0
    want = expected_flow(tr.grads, nb, nc, factor)
    assert bool((want > 0).all()) and close(got, want, RTOL), (got - want) / want
    assert torch.equal(torch.cat([total2.reshape(1), norms2]).cpu(), got)
    for before, now in zip(state, (tr.grads, model.flat_parameters, tr.exp_avg, tr.exp_avg_sq, tr.step_counter)):
        assert torch.equal(before.view(torch.int32) if before.dtype == torch.float32 else before,
                           now.view(torch.int32) if now.dtype == torch.float32 else now)


# ---- 4. fit ---------------------------------------------------------------------------------------------------------------
GRAD_KEYS = {"total_grad_norm", "block_norms", "model_update", "accum_model_update"}
BASE_KEYS = {"tr_loss", "val_loss", "best_loss", "best_epoch", "lr", "improved", "val_metric_dict"}


def _fit_setup(pkg, nc, bs=4, **trainer_kw):
    ei = _topology(pkg)
    train = pkg.SnapshotStore(pkg.wdn_synth.make_snapshots(10, NODES, seed=3) * 12.5 + 50.0, ei, device=DEV)
    val = pkg.SnapshotStore(pkg.wdn_synth.make_snapshots(6, NODES, seed=4) * 12.5 + 50.0, ei, device=DEV, mean=train.mean,
                            std=train.std)

    def trainer():
        torch.manual_seed(21)
        model = pkg.GATResMeanConv(num_blocks=2, nc=nc).cuda()
        return model, pkg.GATResTrainer.for_store(model, train, bs, lr=5e-3, mask_rate=0.5, **trainer_kw)
    return train, val, trainer


def bits(values):
    return np.asarray(values, dtype=np.float64).view(np.int64).tolist()


@pytest.mark.parametrize("nc,clip", [(8, False), (32, False), (32, True)])
def test_fit_log_gradient_equals_the_hand_written_loop_and_leaves_training_alone(pkg, lib, nc, clip):
    """``clip``: AutoClip on -- the sibling trainer of the ragged batch reads the coefficient of the optimizer state it shares."""
    bs, epochs = 4, 3
    train, val, trainer = _fit_setup(pkg, nc, bs, **(dict(use_gradient_clipping=True, percentile=0.0) if clip else {}))
    kw = dict(batch_size=bs, scheduler=None, val_seed=40)
    calls = []
    model_a, tr_a = trainer()
    a = tr_a.fit(train, val, epochs, generator=torch.Generator().manual_seed(7), log_gradient=True,
                 on_epoch=lambda e, info: calls.append((e, info)), **kw)
    plain_calls = []
    model_b, tr_b = trainer()
    b = tr_b.fit(train, val, epochs, generator=torch.Generator().manual_seed(7), on_epoch=lambda e, info: plain_calls.append((e, info)),
                 **kw)
    torch.cuda.synchronize()
    # (a) the option changes nothing of the training
    assert torch.equal(model_a.flat_parameters, model_b.flat_parameters)
    assert torch.equal(tr_a.exp_avg, tr_b.exp_avg) and torch.equal(tr_a.exp_avg_sq, tr_b.exp_avg_sq)
    assert tr_a.optimizer_step == tr_b.optimizer_step == epochs * 3
    assert bits(a.tr_loss) == bits(b.tr_loss) and bits(a.val_loss) == bits(b.val_loss) and a.lr == b.lr
    assert a.best_epoch == b.best_epoch and a.best_loss == b.best_loss
    # (d) off: the new lists stay empty
    assert b.total_grad_norm == [] and b.block_norms == [] and b.block_names == [] and b.model_update == []
    assert b.accum_model_update == []
    # (b) the hand-written loop from the same start
    model_c, tr_c = trainer()
    gen = torch.Generator().manual_seed(7)
    want = dict(total=[], norms=[], update=[], accum=[], update_torch=[])
    first, accum = None, 0.0
    one = torch.zeros(1, dtype=torch.float64, device=DEV)
    for e in range(1, epochs + 1):
        tr_c.fit_epoch(train, bs, generator=gen)
        last = tr_c.last_step_trainer
        assert last is tr_c._siblings[2] and last.num_graphs == 2                 # batches of 4, 4 and 2: the sibling ran last
        total, norms, names = last.gradient_flow()
        if clip:
            # the report is the unclipped gradient's times the coefficient of the update that just ran (< 1 at percentile 0)
            coef = float(tr_c.last_clip_coef)
            assert 0.0 < coef < 1.0 and last._clip is tr_c._clip
            got = torch.cat([total.reshape(1), norms]).cpu()
            assert close(got, expected_flow(last.grads, 2, nc, coef), RTOL)
        if first is None:
            first = last.out.clone()
        assert lib.gatres_mean_abs_diff(last.out.data_ptr(), first.data_ptr(), first.numel(), one.data_ptr(), None) == 0
        want["total"].append(float(total)); want["norms"].append(norms.cpu().numpy().copy())
        want["update"].append(float(one)); accum += float(one); want["accum"].append(accum)
        want["update_torch"].append(float((last.out - first).abs().double().mean()))
        pkg.evaluation.evaluate_store(model_c, val, bs, tr_c.mask_rate, seed=40 + e, prefix="val", gpu_warmup_times=0)
    assert torch.equal(model_c.flat_parameters, model_a.flat_parameters)
    assert a.block_names == names == [n for n, _ in model_a.named_parameters() if "block" in n]
    assert len(a.total_grad_norm) == len(a.block_norms) == len(a.model_update) == len(a.accum_model_update) == epochs
    assert bits(a.total_grad_norm) == bits(want["total"])
    assert all(x.dtype == np.float64 and x.shape == (16,) and bits(x) == bits(y) for x, y in zip(a.block_norms, want["norms"]))
    assert bits(a.model_update) == bits(want["update"]) and bits(a.accum_model_update) == bits(want["accum"])
    assert a.model_update[0] == 0.0 and all(u > 0.0 for u in a.model_update[1:])
    assert close(a.model_update[1:], want["update_torch"][1:], 1e-12)
    assert all(t > 0.0 and math.isfinite(t) for t in a.total_grad_norm)
    # ... and the report is the gradient's: the norm of the norms
    for t, n in zip(a.total_grad_norm, a.block_norms):
        assert abs(t - float(np.sqrt((n * n).sum()))) <= 1e-11 * t
    # (c) on_epoch: once per epoch, in order, the history's values
    assert [e for e, _ in calls] == [1, 2, 3] == [e for e, _ in plain_calls]
    for (e, info), (_, plain) in zip(calls, plain_calls):
        assert set(info) == BASE_KEYS | GRAD_KEYS and set(plain) == BASE_KEYS
        i = e - 1
        assert info["tr_loss"] == a.tr_loss[i] and bits([info["val_loss"]]) == bits([a.val_loss[i]]) and info["lr"] == a.lr[i]
        assert info["improved"] == a.improved[i] and info["best_loss"] == a.records[i][6] and info["best_epoch"] == int(a.records[i][7])
        assert list(info["val_metric_dict"]) == list(pkg.evaluation.get_metric_fn_collection("val"))
        assert info["total_grad_norm"] == a.total_grad_norm[i] and info["block_norms"] is a.block_norms[i]
        assert info["model_update"] == a.model_update[i] and info["accum_model_update"] == a.accum_model_update[i]
    assert calls[-1][1]["best_loss"] == a.best_loss and calls[-1][1]["best_epoch"] == a.best_epoch
    assert bits(list(calls[a.best_epoch - 1][1]["val_metric_dict"].values())) == bits(list(a.best_metric_dict.values()))


def test_on_epoch_gets_the_train_metrics_and_its_exception_propagates(pkg):
    train, val, trainer = _fit_setup(pkg, 8)
    model, tr = trainer()
    seen = []
    h = tr.fit(train, val, 2, batch_size=4, scheduler=None, train_metrics=True, log_gradient=True,
               on_epoch=lambda e, info: seen.append(info))
    assert [set(i) for i in seen] == [BASE_KEYS | GRAD_KEYS | {"train_metric_dict"}] * 2
    assert seen[1]["train_metric_dict"] is h.train_metrics[1]
    assert list(seen[0]["train_metric_dict"]) == list(pkg.evaluation.get_metric_fn_collection("train"))

    class Boom(Exception):
        pass

    def boom(e, info):
        if e == 2:
            raise Boom(e)

    with pytest.raises(Boom):
        tr.fit(train, val, 3, batch_size=4, scheduler=None, on_epoch=boom)
    # internal_train hands both options on to fit
    import argparse
    args = argparse.Namespace(lr=5e-3, weight_decay=6e-6, epochs=2, mask_rate=0.5, criterion="mse", batch_size=4, patience=10,
                              min_delta=1e-4, scheduler=None, scheduler_patience=2)
    torch.manual_seed(21)
    got = []
    pkg.internal_train(args, pkg.GATResMeanConv(num_blocks=2, nc=8).cuda(), train, val, log_gradient=True,
                       on_epoch=lambda e, info: got.append((e, info["model_update"])))
    assert [e for e, _ in got] == [1, 2] and got[0][1] == 0.0 and got[1][1] > 0.0


def test_fit_log_gradient_refuses_a_last_batch_of_another_size(pkg):
    """With a fixed store the last batch keeps its size, so the size of epoch 1's copy is changed behind ``fit``'s back."""
    train, val, trainer = _fit_setup(pkg, 8)
    model, tr = trainer()

    def shrink(e, info):
        tr._fit["first_out"] = tr._fit["first_out"][:-1].clone()

    with pytest.raises(ValueError, match="last training batch of epoch 2"):
        tr.fit(train, val, 3, batch_size=4, scheduler=None, log_gradient=True, on_epoch=shrink)


def test_last_step_trainer_without_a_reference_to_itself(pkg):
    """The trainer that ran the epoch's last step is the sibling after a ragged batch, else the trainer itself -- which it
    does not hold a reference to (its buffers go with its last reference, no cycle collector needed)."""
    train, val, trainer = _fit_setup(pkg, 8)
    model, tr = trainer()
    assert tr.last_step_trainer is tr and tr._last_stepper is None
    tr.fit_epoch(train, 4)
    assert tr.last_step_trainer is tr._siblings[2] and tr._siblings[2].last_step_trainer is tr._siblings[2]
    tr.fit_epoch(train, 4, drop_last=True)
    assert tr.last_step_trainer is tr and tr._last_stepper is None
    assert not any(v is tr for v in vars(tr).values()) and not any(v is t for t in tr._siblings.values() for v in vars(t).values())
