"""``GATResTrainer.fit``: the reference's training loop with its epoch boundary on the device.

* ``gatres_epoch_control`` against the host mirror (``epoch_control.EpochController``) on the recorded sequences and on random
  ones, fed through synthetic loss sums, moment tables and per-batch losses;
* ``gatres_snapshot_if``: flag clear / set, sizes with and without a vector body, guard words, restore;
* ``fit`` against the hand-written loop -- ``fit_epoch`` + ``evaluate_store`` + the host mirror + ``set_lr`` -- bit for bit;
* the best snapshot, the checkpoint files, AutoClip, ``internal_train``.

Every check is an equality: ``fit`` runs the hand loop's kernels on the hand loop's inputs, and the controller is integer
logic plus a handful of IEEE operations."""
import argparse
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODES, PIPES = 388, 430


def dec(s):
    return {"nan": math.nan, "inf": math.inf, "-inf": -math.inf}.get(s) if s in ("nan", "inf", "-inf") else float.fromhex(s)


def eq(a, b):
    """Equal values, NaN where NaN (a NaN's sign and payload are not pinned by IEEE arithmetic)."""
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)


# ---- the controller kernel -------------------------------------------------------------------------------------------------
def _run_controller(pkg, lib, val_losses, lr, patience, min_delta, sp, mode, rng, use_scheduler=True):
    """Feed per-epoch validation losses through the kernel and the mirror; returns nothing, asserts everything."""
    M, N = pkg.epoch_control, pkg._native
    dev = "cuda:0"
    n = len(val_losses)
    ctl = M.EpochController(lr, patience=patience, min_delta=min_delta, scheduler=use_scheduler, scheduler_patience=sp)
    cfg = N.GatresEpochConfig(min_delta, 0.1, 1e-4, 0.0, 1e-8, patience, sp, int(use_scheduler), 0)
    hp0 = [lr, 0.9, 0.999, 1e-8, 6e-6]
    hp = torch.tensor(hp0, dtype=torch.float64, device=dev)
    state = torch.zeros(M.STATE, dtype=torch.float64, device=dev)
    state[1] = math.inf
    state[6] = math.inf
    history = torch.zeros((n, M.RECORD), dtype=torch.float64, device=dev)
    stream = N.current_stream(torch.device(dev))
    want = []
    for v in val_losses:
        B = int(rng.randint(1, 150))
        graphs = rng.randint(1, 33, size=B).astype(np.int32)
        tot, seen = float(rng.rand() * 100), float(rng.randint(1, 5000))
        sums = torch.tensor([tot, seen, 0.0, 0.0], dtype=torch.float64, device=dev)
        g_dev = torch.from_numpy(graphs).to(dev)
        table = losses = None
        if mode in ("sums", "exact"):      # the data-parallel form: {sum loss * g, n} handed in ("exact": n = 1, val_loss == v)
            if mode == "exact":
                graphs = np.ones(1, dtype=np.int32)
            nv = float(graphs.sum())
            sums[2], sums[3] = v * nv, nv
            val = (v * nv) / nv
            rc = lib.gatres_epoch_control(sums.data_ptr(), None, None, None, 0, sums[2:].data_ptr(), C.byref(cfg), hp.data_ptr(),
                                          state.data_ptr(), history.data_ptr(), n, stream)
        elif mode == "losses":             # per-batch fp32 losses (mae / sce)
            per = (np.float32(v) * (1 + 0.1 * rng.randn(B))).astype(np.float32) if not math.isnan(v) else np.full(B, np.nan, np.float32)
            if B > 1 and not math.isnan(v):
                per[:] = np.float32(v)     # every batch the same fp32 value: the weighted mean is that value unless rounding moves it
            losses = torch.from_numpy(per).to(dev)
            val = M.weighted_mean(per, graphs)
            rc = lib.gatres_epoch_control(sums.data_ptr(), None, losses.data_ptr(), g_dev.data_ptr(), B, None, C.byref(cfg),
                                          hp.data_ptr(), state.data_ptr(), history.data_ptr(), n, stream)
        else:                              # moment records: loss_b = [1] / [0]
            T = np.zeros((B, 16))
            T[:, 0] = rng.randint(1, 400, size=B)
            T[:, 1] = (v if not math.isnan(v) else np.nan) * T[:, 0] * (1 + 0.05 * rng.randn(B))
            table = torch.from_numpy(T).to(dev)
            val = pkg.evaluation.metrics_from_moments(T, graphs.tolist(), "val")[0]
            rc = lib.gatres_epoch_control(sums.data_ptr(), table.data_ptr(), None, g_dev.data_ptr(), B, None, C.byref(cfg),
                                          hp.data_ptr(), state.data_ptr(), history.data_ptr(), n, stream)
        assert rc == 0
        rec = ctl.step(tot / seen, val, float(graphs.sum()))
        want.append(ctl.record_vector(rec))
        torch.cuda.synchronize()
        k = ctl.epoch - 1
        got = history[k].cpu().numpy()
        assert eq(got, want[-1]), (k, dict(zip(M.RECORD_FIELDS, zip(got, want[-1]))))
        assert eq(state.cpu().numpy(), ctl.state_vector()), (k, state.cpu().numpy(), ctl.state_vector())
        h = hp.cpu().numpy()
        assert h[0] == ctl.lr and list(h[1:]) == hp0[1:]
        if ctl.stopped:
            break
    assert eq(history[:len(want)].cpu().numpy(), np.stack(want))
    assert not history[len(want):].any()
    return ctl


def _traces():
    with open(os.path.join(ROOT, "tests", "golden", "epoch_control_traces.json")) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("case", _traces(), ids=lambda c: c["name"])
def test_controller_kernel_equals_the_mirror_on_the_recorded_sequences(pkg, lib, case):
    rng = np.random.RandomState(3)
    vals = [dec(v) for v in case["val_losses"]]
    ctl = _run_controller(pkg, lib, vals, dec(case["lr"]), case["patience"], dec(case["min_delta"]), case["scheduler_patience"],
                          "exact", rng)
    # ... and so the kernel reproduced the recorded results of the reference's classes
    assert ctl.stopped == case["epochs"][-1]["stop"] and ctl.epoch == len(case["epochs"])
    assert ctl.lr == dec(case["epochs"][-1]["lr"])


@pytest.mark.parametrize("mode", ["table", "losses", "sums"])
def test_controller_kernel_equals_the_mirror_on_random_sequences(pkg, lib, mode):
    rng = np.random.RandomState({"table": 1, "losses": 2, "sums": 4}[mode])
    stops = drops = 0
    for trial in range(40):
        n = int(rng.randint(3, 25))
        if trial % 3 == 0:
            seq = np.abs(1.0 + np.cumsum(rng.randn(n) * 0.03))
        elif trial % 3 == 1:
            seq = np.round(rng.rand(n) + 0.1, 1)
        else:
            seq = np.exp(-np.arange(n) * 0.3 * rng.rand()) + 1e-5 * rng.randn(n)
        if trial % 7 == 6:
            seq[rng.randint(n)] = np.nan
        lr = float(10.0 ** rng.uniform(-8, -2))
        ctl = _run_controller(pkg, lib, [float(v) for v in seq], lr, int(rng.choice([0, 1, 2, 3, 6])),
                              float(rng.choice([0.0, 1e-4, 1e-2])), int(rng.randint(0, 4)), mode, rng,
                              use_scheduler=trial % 5 != 4)
        stops += ctl.stopped
        drops += ctl.lr < lr
    assert stops >= 5 and drops >= 5


def test_controller_refuses_bad_arguments(pkg, lib):
    N = pkg._native
    cfg = N.GatresEpochConfig(1e-4, 0.1, 1e-4, 0.0, 1e-8, 3, 2, 1, 0)
    t = torch.zeros(64, dtype=torch.float64, device="cuda:0")
    p = t.data_ptr()
    assert lib.gatres_epoch_control(p, p, p, p, 4, None, C.byref(cfg), p, p, p, 2, None) == -1       # table AND losses
    assert lib.gatres_epoch_control(p, None, None, p, 4, None, C.byref(cfg), p, p, p, 2, None) == -1  # neither
    assert lib.gatres_epoch_control(p, None, None, None, 0, None, C.byref(cfg), p, p, p, 2, None) == -1  # no sums either
    assert lib.gatres_epoch_control(p, p, None, p, 4, None, C.byref(cfg), p, p, p, 0, None) == -1     # no history room
    bad = N.GatresEpochConfig(1e-4, 0.1, 1e-4, 0.0, 1e-8, -1, 2, 1, 0)
    assert lib.gatres_epoch_control(p, p, None, p, 4, None, C.byref(bad), p, p, p, 2, None) == -1
    assert lib.gatres_epoch_val_sums(p, p, p, 4, p, None) == -1


def test_val_sums_kernel_equals_the_controllers_accumulation(pkg, lib):
    rng = np.random.RandomState(8)
    for B in (1, 63, 64, 65, 300):
        T = np.zeros((B, 16))
        T[:, 0] = rng.randint(1, 400, size=B)
        T[:, 1] = rng.rand(B) * T[:, 0]
        g = rng.randint(1, 33, size=B).astype(np.int32)
        out = torch.zeros(2, dtype=torch.float64, device="cuda:0")
        td, gd = torch.from_numpy(T).cuda(), torch.from_numpy(g).cuda()
        assert lib.gatres_epoch_val_sums(td.data_ptr(), None, gd.data_ptr(), B, out.data_ptr(), None) == 0
        acc = 0.0
        for b in range(B):
            acc += float(T[b, 1] / T[b, 0]) * int(g[b])
        assert out.cpu().tolist() == [acc, float(g.sum())]


# ---- the snapshot kernel -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [3, 65857, 1667585])
@pytest.mark.parametrize("shift", [0, 1])
def test_snapshot_if_copies_only_when_the_flag_is_set(pkg, lib, P, shift):
    """shift = 1: the destinations start one float past a 16-byte boundary (a scalar head in front of the vector body)."""
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(P)
    src = [torch.randn(P, device=dev, generator=g) for _ in range(3)]
    G = 8                                                                      # guard floats on either side
    SENT = -7.25
    raw = [torch.full((G + shift + P + G,), SENT, device=dev) for _ in range(3)]
    dst = [r[G + shift: G + shift + P] for r in raw]
    step = torch.tensor([41, 7], dtype=torch.int64, device=dev)
    dstep = torch.tensor([-1, -2, -3], dtype=torch.int64, device=dev)
    flag = torch.zeros(1, dtype=torch.float64, device=dev)

    def call(f, s, sstep, d, dstep_ptr):
        assert lib.gatres_snapshot_if(f, s[0].data_ptr(), s[1].data_ptr(), s[2].data_ptr(), sstep, d[0].data_ptr(),
                                      d[1].data_ptr(), d[2].data_ptr(), dstep_ptr, P, None) == 0
        torch.cuda.synchronize()

    call(flag.data_ptr(), src, step.data_ptr(), dst, dstep[1:].data_ptr())
    assert all(bool((r == SENT).all()) for r in raw) and dstep.tolist() == [-1, -2, -3]            # flag clear: untouched
    flag.fill_(1.0)
    call(flag.data_ptr(), src, step.data_ptr(), dst, dstep[1:].data_ptr())
    for s, d, r in zip(src, dst, raw):
        assert torch.equal(s.view(torch.int32), d.view(torch.int32))                                # bit-equal copy
        assert bool((r[:G + shift] == SENT).all()) and bool((r[G + shift + P:] == SENT).all())      # guards intact
    assert dstep.tolist() == [-1, 41, -3]
    # restore: sources and destinations exchanged, no flag
    live = [torch.zeros(P, device=dev) for _ in range(3)]
    lstep = torch.tensor([99, 5], dtype=torch.int64, device=dev)
    call(None, dst, dstep[1:].data_ptr(), live, lstep.data_ptr())
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(live, src))
    assert lstep.tolist() == [41, 5]                                                                # (the ticket word stays)
    assert lib.gatres_snapshot_if(None, src[0].data_ptr(), src[1].data_ptr(), src[2].data_ptr(), None, dst[0].data_ptr(),
                                  dst[1].data_ptr(), dst[2].data_ptr(), dstep.data_ptr(), P, None) == -1
    assert lib.gatres_snapshot_if(None, src[0].data_ptr(), src[1].data_ptr(), src[2].data_ptr(), None, dst[0].data_ptr(),
                                  dst[1].data_ptr(), dst[2].data_ptr(), None, 0, None) == -1


# ---- fit against the hand-written loop -----------------------------------------------------------------------------------
def _stores(pkg, S_train, S_val, seed=3):
    ei = pkg.wdn_synth.make_wdn_topology(NODES, PIPES, seed=0)
    tr = pkg.SnapshotStore(pkg.wdn_synth.make_snapshots(S_train, NODES, seed=seed) * 12.5 + 50.0, ei, device="cuda:0")
    va = pkg.SnapshotStore(pkg.wdn_synth.make_snapshots(S_val, NODES, seed=seed + 1) * 12.5 + 50.0, ei, device="cuda:0",
                           mean=tr.mean, std=tr.std)
    return tr, va


def _trainer(pkg, store, nb, bs, use_graph=True, seed=21, **kw):
    torch.manual_seed(seed)
    model = pkg.GATResMeanConv(num_blocks=nb, nc=32).cuda()
    tr = pkg.GATResTrainer(model, store.edge_index(bs), bs * NODES, nodes_per_graph=[NODES] * bs, targets_are_inputs=True,
                           use_graph=use_graph, **kw)
    tr.epoch_graph_steps = 3
    return model, tr


def _hand_loop(pkg, tr, model, train_store, val_store, epochs, bs, vbs, gen, val_seed, patience, min_delta, sp, on_best=None):
    """The loop a user writes today: fit_epoch + evaluate_store (+ gatres_masked_loss for mae / sce) + the mirror + set_lr."""
    E, lib = pkg.evaluation, pkg._native.load()
    ctl = pkg.epoch_control.EpochController(tr.hparams["lr"], patience=patience, min_delta=min_delta, scheduler_patience=sp)
    out = dict(tr_loss=[], val_loss=[], lr=[], metrics=[])
    for e in range(1, epochs + 1):
        tr_loss, _ = tr.fit_epoch(train_store, bs, generator=gen)
        caps = []
        val_loss, m = E.evaluate_store(model, val_store, vbs, tr.mask_rate, seed=val_seed + e, prefix="val",
                                       gpu_warmup_times=0, _capture=caps)
        if tr.criterion != "mse":
            per, graphs = [], []
            for mask, o, x, g in caps:
                loss = torch.zeros(1, device="cuda:0")
                gout = torch.empty(o.numel(), device="cuda:0")
                assert lib.gatres_masked_loss(o.data_ptr(), x.data_ptr(), mask.data_ptr(), pkg._native.CRITERIA[tr.criterion],
                                              loss.data_ptr(), gout.data_ptr(), o.numel(), None) == 0
                per.append(float(loss))
                graphs.append(g)
            val_loss = pkg.epoch_control.weighted_mean(per, graphs)
        out["lr"].append(ctl.lr)
        rec = ctl.step(tr_loss, val_loss)
        out["tr_loss"].append(tr_loss); out["val_loss"].append(val_loss); out["metrics"].append(m)
        if ctl.improved and on_best is not None:
            on_best(e)
        if ctl.stopped:
            break
        tr.set_lr(ctl.lr)
    out["ctl"] = ctl
    return out


def _assert_same_run(pkg, a, tr_a, model_a, hand, tr_b, model_b):
    ctl = hand["ctl"]
    assert a.tr_loss == hand["tr_loss"] and eq(a.val_loss, hand["val_loss"]) and a.lr == hand["lr"]
    assert a.best_epoch == ctl.best_epoch and a.best_loss == ctl.best_loss
    assert a.stopped_epoch == (ctl.epoch if ctl.stopped else None)
    assert a.final_lr == ctl.lr == tr_a.hparams["lr"] and float(tr_a.hp[0]) == ctl.lr
    assert [bool(r["improved"]) for r in ctl.history] == a.improved
    torch.cuda.synchronize()
    assert torch.equal(model_a.flat_parameters, model_b.flat_parameters)
    assert torch.equal(tr_a.exp_avg, tr_b.exp_avg) and torch.equal(tr_a.exp_avg_sq, tr_b.exp_avg_sq)
    assert tr_a.optimizer_step == tr_b.optimizer_step
    assert tr_a.num_captured_graphs == tr_b.num_captured_graphs
    for k in pkg.evaluation.get_metric_fn_collection("val"):
        assert eq(a.best_metric_dict[k], hand["metrics"][ctl.best_epoch - 1][k]), k


CASES = {
    # name: (blocks, batch, train snapshots, val snapshots, epochs, lr, patience, min_delta, scheduler_patience)
    "small": (4, 8, 8 * 4 + 3, 8 * 2 + 5, 8, 5e-3, 3, 1e-4, 0),
    "headline": (15, 32, 32 * 3 + 7, 32 + 9, 6, 5e-3, 100, 1e-4, 0),
    "small_stops": (4, 8, 8 * 4 + 3, 8 * 2 + 5, 10, 2e-3, 2, 10.0, 0),         # a min_delta nothing can beat: stops at epoch 3
}


@pytest.mark.parametrize("criterion", ["mse", "mae", "sce"])
@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("case", list(CASES))
def test_fit_equals_the_hand_written_loop(pkg, case, use_graph, criterion):
    nb, bs, St, Sv, epochs, lr, patience, min_delta, sp = CASES[case]
    train_store, val_store = _stores(pkg, St, Sv)
    model_a, tr_a = _trainer(pkg, train_store, nb, bs, use_graph, lr=lr, criterion=criterion)
    model_b, tr_b = _trainer(pkg, train_store, nb, bs, use_graph, lr=lr, criterion=criterion)
    assert torch.equal(model_a.flat_parameters, model_b.flat_parameters)
    a = tr_a.fit(train_store, val_store, epochs, batch_size=bs, patience=patience, min_delta=min_delta, scheduler_patience=sp,
                 generator=torch.Generator().manual_seed(7), val_seed=100)
    hand = _hand_loop(pkg, tr_b, model_b, train_store, val_store, epochs, bs, bs, torch.Generator().manual_seed(7), 100,
                      patience, min_delta, sp)
    _assert_same_run(pkg, a, tr_a, model_a, hand, tr_b, model_b)
    assert len(set(a.val_loss)) > 1 and (St % bs) in tr_a._siblings            # fresh masks every epoch; the ragged batch ran
    if case == "small_stops":
        assert a.stopped_epoch == 3 and a.stopped_epoch < epochs               # early stopping fired before `epochs`
    else:
        # the rate dropped at least once (scheduler_patience 0: any epoch that does not improve by 1e-4 relative drops it;
        # sce's loss is flat by construction and the other runs overshoot at this learning rate)
        assert a.final_lr < lr or min(a.lr) < lr, (a.lr, a.val_loss)
    if use_graph:
        assert tr_a.num_captured_graphs > 0


def test_fit_with_autoclip_and_train_metrics_equals_the_hand_loop(pkg):
    nb, bs, St, Sv, epochs, lr, patience, min_delta, sp = CASES["small"]
    train_store, val_store = _stores(pkg, St, Sv)
    kw = dict(lr=lr, use_gradient_clipping=True, percentile=10.0)
    model_a, tr_a = _trainer(pkg, train_store, nb, bs, True, **kw)
    model_b, tr_b = _trainer(pkg, train_store, nb, bs, True, **kw)
    a = tr_a.fit(train_store, val_store, epochs, batch_size=bs, patience=patience, min_delta=min_delta, scheduler_patience=sp,
                 generator=torch.Generator().manual_seed(7), val_seed=5)
    hand = _hand_loop(pkg, tr_b, model_b, train_store, val_store, epochs, bs, bs, torch.Generator().manual_seed(7), 5, patience,
                      min_delta, sp)
    _assert_same_run(pkg, a, tr_a, model_a, hand, tr_b, model_b)
    assert np.array_equal(tr_a.grad_norm_history(), tr_b.grad_norm_history()) and len(tr_a.grad_norm_history()) > 0
    # train_metrics=True: the same training, plus the "train" collection per epoch
    model_c, tr_c = _trainer(pkg, train_store, nb, bs, True, **kw)
    c = tr_c.fit(train_store, val_store, epochs, batch_size=bs, patience=patience, min_delta=min_delta, scheduler_patience=sp,
                 generator=torch.Generator().manual_seed(7), val_seed=5, train_metrics=True)
    assert c.tr_loss == a.tr_loss and eq(c.val_loss, a.val_loss) and torch.equal(model_c.flat_parameters, model_a.flat_parameters)
    assert len(c.train_metrics) == len(c.tr_loss) and list(c.train_metrics[0]) == list(pkg.evaluation.get_metric_fn_collection("train"))


def test_best_snapshot_restore_and_checkpoints(pkg, tmp_path):
    nb, bs, St, Sv = 4, 8, 8 * 3 + 3, 8 + 5
    epochs, lr = 10, 0.1               # (a rate that overshoots: the best epoch comes early, the run goes on)
    train_store, val_store = _stores(pkg, St, Sv)
    model_b, tr_b = _trainer(pkg, train_store, nb, bs, True, lr=lr)
    kept = {}

    def on_best(e):
        kept.update(params=model_b.flat_parameters.detach().clone(), m=tr_b.exp_avg.clone(), v=tr_b.exp_avg_sq.clone(),
                    step=tr_b.optimizer_step, epoch=e)

    hand = _hand_loop(pkg, tr_b, model_b, train_store, val_store, epochs, bs, bs, torch.Generator().manual_seed(9), 0, 100, 1e-4, 0,
                      on_best=on_best)
    assert hand["ctl"].best_epoch < epochs                                     # the best epoch is not the last: restoring matters
    runs = {}
    for mode in ("reference", "end"):
        model, tr = _trainer(pkg, train_store, nb, bs, True, lr=lr)
        d = tmp_path / mode
        written = []
        orig = pkg.wdn_io.save_checkpoint

        def spy(path, _orig=orig, _written=written, _tr=tr, **k):
            _written.append((os.path.basename(path), int(_tr._fit["state"][0])))       # (file, epochs decided when it is written)
            return _orig(path, **k)

        pkg.wdn_io.save_checkpoint = spy
        try:
            hist = tr.fit(train_store, val_store, epochs, batch_size=bs, patience=100, min_delta=1e-4, scheduler_patience=0,
                          generator=torch.Generator().manual_seed(9), val_seed=0, save_path=str(d), model_name="gatres",
                          variant="t", save_best=mode, restore_best=True, checkpoint_extra={"note": "x"})
        finally:
            pkg.wdn_io.save_checkpoint = orig
        assert [ep for f, ep in written if f.startswith("last_")] == [1, 5, 10]
        runs[mode] = (model, tr, hist, [w[0] for w in written])
        assert hist.best_epoch == kept["epoch"] == hand["ctl"].best_epoch
        # restore_best: the model, the moments and the step count are the best epoch's
        assert torch.equal(model.flat_parameters, kept["params"]) and torch.equal(tr.exp_avg, kept["m"])
        assert torch.equal(tr.exp_avg_sq, kept["v"]) and tr.optimizer_step == kept["step"]
        b = tr.best_state()
        assert torch.equal(b["params"], kept["params"]) and int(b["step"]) == kept["step"]
    files = {m: [w for w in runs[m][3]] for m in runs}
    assert files["end"].count("last_gatres_t.pth") == 3 and files["end"].count("best_gatres_t.pth") == 1   # epochs 1, 5, 10; once
    assert files["end"][-1] == "best_gatres_t.pth"
    assert files["reference"].count("last_gatres_t.pth") == 3
    assert files["reference"].count("best_gatres_t.pth") == sum(runs["reference"][2].improved)
    cps = {}
    for mode in runs:
        fresh = pkg.GATResMeanConv(num_blocks=nb, nc=32)
        _, cp = pkg.wdn_io.load_checkpoint(str(tmp_path / mode / "best_gatres_t.pth"), fresh)
        assert torch.equal(fresh.flat_parameters, kept["params"].cpu())
        fresh2 = pkg.GATResMeanConv(num_blocks=nb, nc=32)
        _, last = pkg.wdn_io.load_checkpoint(str(tmp_path / mode / "last_gatres_t.pth"), fresh2)
        assert last["epoch"] == cp["epoch"] == kept["epoch"] and cp["note"] == "x" and cp["norm_type"] == "znorm"
        assert set(cp) >= {"model_state_dict", "optimizer_state_dict", "epoch", "loss", "val_metric_dict", "mean", "std", "min",
                           "max", "norm_type"}
        assert list(cp["val_metric_dict"]) == list(pkg.evaluation.get_metric_fn_collection("val"))
        cps[mode] = cp
    a, b = cps["reference"], cps["end"]
    assert list(a["model_state_dict"]) == list(b["model_state_dict"])
    assert all(torch.equal(a["model_state_dict"][k].cpu(), b["model_state_dict"][k].cpu()) for k in a["model_state_dict"])
    sa, sb = a["optimizer_state_dict"], b["optimizer_state_dict"]
    assert sa["param_groups"] == sb["param_groups"] and a["loss"] == b["loss"] and eq(list(a["val_metric_dict"].values()),
                                                                                     list(b["val_metric_dict"].values()))
    for i in sa["state"]:
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(sa["state"][i][k].cpu(), sb["state"][i][k].cpu()), (i, k)
    # one more step on the restored trainer == a step on a fresh trainer loaded with those tensors (this fails if the
    # transposed weights in scratch were not invalidated)
    model, tr = runs["end"][0], runs["end"][1]
    twin_model, twin = _trainer(pkg, train_store, nb, bs, True, lr=lr)
    with torch.no_grad():
        twin_model.flat_parameters.copy_(kept["params"])
    twin.invalidate_weights()
    twin.exp_avg.copy_(kept["m"]); twin.exp_avg_sq.copy_(kept["v"]); twin.step_counter[0] = kept["step"]
    twin.set_lr(tr.hparams["lr"])
    x = train_store.batch(torch.arange(bs)).reshape(-1)
    la, lb = tr.step(x, x).clone(), twin.step(x, x).clone()
    torch.cuda.synchronize()
    assert torch.equal(la, lb) and torch.equal(model.flat_parameters, twin_model.flat_parameters)
    assert torch.equal(tr.exp_avg, twin.exp_avg)


def test_internal_train_returns_what_fit_returns(pkg, tmp_path):
    nb, bs, St, Sv = 4, 8, 8 * 3 + 3, 8 + 5
    train_store, val_store = _stores(pkg, St, Sv)
    args = argparse.Namespace(lr=5e-3, weight_decay=6e-6, epochs=4, mask_rate=0.9, criterion="mae", batch_size=bs, patience=3,
                              min_delta=1e-4, scheduler="ReduceLROnPlateau", scheduler_patience=0, use_gradient_clipping=True,
                              percentile=20.0, save_path=str(tmp_path), model_name="m", variant="v")
    torch.manual_seed(21)
    model = pkg.GATResMeanConv(num_blocks=nb, nc=32).cuda()
    best_loss, best_metrics = pkg.internal_train(args, model, train_store, val_store, generator=torch.Generator().manual_seed(2))
    model_b, tr_b = _trainer(pkg, train_store, nb, bs, True, lr=5e-3, weight_decay=6e-6, mask_rate=0.9, criterion="mae",
                             use_gradient_clipping=True, percentile=20.0)
    tr_b.epoch_graph_steps = 20
    h = tr_b.fit(train_store, val_store, 4, batch_size=bs, patience=3, min_delta=1e-4, scheduler_patience=0,
                 generator=torch.Generator().manual_seed(2))
    assert best_loss == h.best_loss and eq(list(best_metrics.values()), list(h.best_metric_dict.values()))
    assert list(best_metrics) == list(pkg.evaluation.get_metric_fn_collection("val"))
    assert torch.equal(model.flat_parameters, model_b.flat_parameters)
    assert os.path.exists(tmp_path / "best_m_v.pth") and os.path.exists(tmp_path / "last_m_v.pth")
