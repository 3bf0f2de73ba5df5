"""Fine-tuning to a fixed sensor layout on the device: ``gatres_stage_rows_mask_sensors`` bit for bit against the host
restatement (``sensor_layout_draws``) and against its neighbours (``gatres_stage_rows_mask`` for random-mode graphs,
``gatres_stage_observed`` for the deployment mask); the store-fed steps, sequences and epochs under a layout; ``evaluate_store``,
``fit`` and ``PressureEstimator.fine_tune`` under it; the refusals.  Every check but one is an equality: the launches under a
layout are today's launches on another mask.  The one tolerance (``evaluate_store`` against ``layout_errors``) is worked out
where it is used."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NODES, PIPES = 388, 430
SEED, DROP, SHARE, RATE = 9, 0.3, 0.6, 0.95
OBS8 = [0, 57, 101, 160, 222, 300, 345, 387]


def _stage(lib, data, rows, G, N, obs_dev, K, drop, share, rate, seed, step, with_y=True, sensors=True):
    """One staging launch into fresh buffers filled with a sentinel; returns (x, y, mask) on the host."""
    x = torch.full((G * N,), -7.25, device=DEV)
    y = torch.full((G * N,), -7.25, device=DEV) if with_y else None
    mask = torch.full((G * N + 8,), 77, dtype=torch.uint8, device=DEV)       # (8 guard bytes behind the batch)
    node_ptr = torch.arange(0, (G + 1) * N, N, dtype=torch.int32, device=DEV)
    ctr = torch.tensor([step, 0], dtype=torch.int64, device=DEV)
    yp = None if y is None else y.data_ptr()
    if sensors:
        rc = lib.gatres_stage_rows_mask_sensors(data.data_ptr(), rows.data_ptr(), N, x.data_ptr(), yp, node_ptr.data_ptr(), G,
                                                obs_dev.data_ptr(), K, drop, share, rate, seed, ctr.data_ptr(), mask.data_ptr(), None)
    else:
        rc = lib.gatres_stage_rows_mask(data.data_ptr(), rows.data_ptr(), N, x.data_ptr(), yp, node_ptr.data_ptr(), G, rate, seed,
                                        ctr.data_ptr(), mask.data_ptr(), None)
    assert rc == 0
    torch.cuda.synchronize()
    assert mask[G * N:].eq(77).all()                                          # nothing written behind the batch
    return x.cpu(), None if y is None else y.cpu(), mask[:G * N].cpu().numpy().reshape(G, N)


def _expected_mask(pkg, random_mask, G, N, obs, drop, share, seed, step):
    mode, keep = pkg.sensor_layout_draws(seed, step, G, N, obs, drop, share)
    want = np.ones((G, N), dtype=np.uint8)
    for g in range(G):
        if mode[g]:
            want[g, np.asarray(obs)[keep[g]]] = 0
        else:
            want[g] = random_mask[g]
    return want, mode, keep


KERNEL_CASES = {
    # name: (graphs, nodes, sensors, steps)
    "5x37": (5, 37, [0, 3, 17, 35, 36], (0, 1)),                  # N not a multiple of 4; first and last node
    "33x37": (33, 37, [0, 3, 17, 35, 36], (0, 1)),                # more graphs than one round of anything
    "3x388": (3, NODES, OBS8, (0, 1)),                            # the workload's graph
    "2x2100": (2, 2100, [0, 1024, 2047, 2048, 2099], (0,)),       # the sampler's radix path; sensors around a slice boundary
}


@pytest.mark.parametrize("case", list(KERNEL_CASES))
def test_kernel_equals_the_host_restatement_bit_for_bit(pkg, lib, case):
    G, N, obs, steps = KERNEL_CASES[case]
    S = G + 6
    data = torch.from_numpy(np.random.RandomState(G * N).randn(S, N).astype(np.float32)).to(DEV)
    perm = np.random.RandomState(5).permutation(S)[:G]
    perm[-1] = perm[0]                                            # shuffled rows with a repeat
    rows = torch.from_numpy(perm.astype(np.int64)).to(DEV)
    obs_dev = torch.tensor(obs, dtype=torch.int32, device=DEV)
    want_x = data[rows].reshape(-1).cpu()
    seen_layout = seen_random = seen_kept = seen_dropped = 0
    for step in steps:
        rx, ry, rmask = _stage(lib, data, rows, G, N, obs_dev, len(obs), DROP, SHARE, RATE, SEED, step, sensors=False)
        x, y, mask = _stage(lib, data, rows, G, N, obs_dev, len(obs), DROP, SHARE, RATE, SEED, step)
        want, mode, keep = _expected_mask(pkg, rmask, G, N, obs, DROP, SHARE, SEED, step)
        assert torch.equal(x, want_x) and torch.equal(y, want_x) and torch.equal(rx, want_x)
        assert np.array_equal(mask, want), (case, step, np.argwhere(mask != want)[:8])
        assert keep[mode].any(axis=1).all()                       # no graph of these inputs lost all its sensors
        seen_layout += int(mode.sum()); seen_random += int((~mode).sum())
        seen_kept += int(keep[mode].sum()); seen_dropped += int((~keep[mode]).sum())
        # without y_dst: the same x and mask
        x2, _, mask2 = _stage(lib, data, rows, G, N, obs_dev, len(obs), DROP, SHARE, RATE, SEED, step, with_y=False)
        assert torch.equal(x2, want_x) and np.array_equal(mask2, want)
    assert seen_layout and seen_random and seen_kept and seen_dropped


def test_kernel_limits_and_the_step_counter(pkg, lib):
    G, N, obs = 5, 37, [0, 3, 17, 35, 36]
    data = torch.from_numpy(np.random.RandomState(1).randn(G + 3, N).astype(np.float32)).to(DEV)
    rows = torch.tensor([4, 0, 7, 2, 4], dtype=torch.int64, device=DEV)
    obs_dev = torch.tensor(obs, dtype=torch.int32, device=DEV)
    # (dropout 0, share 1): the mask bytes of gatres_stage_observed on full rows, whatever seed, step and mask_rate are
    x0 = torch.empty(G * N, device=DEV)
    m0 = torch.empty(G * N, dtype=torch.uint8, device=DEV)
    N_ = pkg._native
    assert lib.gatres_stage_observed(data.data_ptr(), N_.OBSERVED_FULL_ROWS, data.shape[0], rows.data_ptr(), 0, N, G,
                                     obs_dev.data_ptr(), len(obs), N_.NORMALISE_NONE, 0.0, 1.0, x0.data_ptr(), m0.data_ptr(), None) == 0
    torch.cuda.synchronize()
    for seed, step, rate in ((SEED, 0, RATE), (SEED + 1, 5, 0.2), (2 ** 64 - 1, 2 ** 40, 0.0)):
        x, _, mask = _stage(lib, data, rows, G, N, obs_dev, len(obs), 0.0, 1.0, rate, seed, step)
        assert np.array_equal(mask, m0.cpu().numpy().reshape(G, N))
        assert torch.equal(x, data[rows].reshape(-1).cpu())                  # (x keeps the full row: the forward masks it)
        assert torch.equal(torch.where(torch.from_numpy(mask.reshape(-1)).bool(), torch.zeros(()), x), x0.cpu())
    # share 0: gatres_stage_rows_mask in everything
    for step in (0, 1):
        a = _stage(lib, data, rows, G, N, obs_dev, len(obs), DROP, 0.0, RATE, SEED, step)
        b = _stage(lib, data, rows, G, N, obs_dev, len(obs), DROP, 0.0, RATE, SEED, step, sensors=False)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    # the step counter is read on the device: the same launch after a bump draws the new step's masks
    x = torch.empty(G * N, device=DEV)
    mask = torch.empty(G * N, dtype=torch.uint8, device=DEV)
    node_ptr = torch.arange(0, (G + 1) * N, N, dtype=torch.int32, device=DEV)
    ctr = torch.zeros(2, dtype=torch.int64, device=DEV)
    got = []
    for step in (0, 1):
        assert lib.gatres_stage_rows_mask_sensors(data.data_ptr(), rows.data_ptr(), N, x.data_ptr(), None, node_ptr.data_ptr(), G,
                                                  obs_dev.data_ptr(), len(obs), DROP, SHARE, RATE, SEED, ctr.data_ptr(),
                                                  mask.data_ptr(), None) == 0
        torch.cuda.synchronize()
        got.append(mask.cpu().numpy().reshape(G, N).copy())
        rmask = _stage(lib, data, rows, G, N, obs_dev, len(obs), DROP, SHARE, RATE, SEED, step, sensors=False)[2]
        assert np.array_equal(got[-1], _expected_mask(pkg, rmask, G, N, obs, DROP, SHARE, SEED, step)[0]), step
        ctr[0] += 1
    assert not np.array_equal(got[0], got[1])


# ---- the trainer -----------------------------------------------------------------------------------------------------------------
def _store(pkg, S, seed=13, like=None):
    ei = pkg.wdn_synth.make_wdn_topology(NODES, PIPES, seed=0)
    kw = {} if like is None else dict(mean=like.mean, std=like.std)
    return pkg.SnapshotStore(pkg.wdn_synth.make_snapshots(S, NODES, seed=seed) * 12.5 + 50.0, ei, device=DEV, **kw)


def _trainer(pkg, store, bs, nb=3, seed=21, **kw):
    torch.manual_seed(seed)
    model = pkg.GATResMeanConv(num_blocks=nb, nc=32).to(DEV)
    tr = pkg.GATResTrainer.for_store(model, store, bs, seed=SEED, **kw)
    return model, tr


def _state(model, tr):
    torch.cuda.synchronize()
    return [model.flat_parameters.detach().clone(), tr.exp_avg.clone(), tr.exp_avg_sq.clone()]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _layout_mask(pkg, tr, G, obs, drop, share, step, random_mask):
    """The mask a store-fed step of ``tr`` trains under at optimizer step ``step`` (random-mode graphs from ``random_mask``)."""
    return _expected_mask(pkg, random_mask, G, NODES, obs, drop, share, tr.seed, step)[0]


def test_steps_under_a_layout_equal_steps_on_the_masks_read_back(pkg, lib):
    bs = 2
    store = _store(pkg, 8)
    model_a, a = _trainer(pkg, store, bs)
    model_b, b = _trainer(pkg, store, bs)
    a.set_sensor_layout(OBS8, sensor_dropout=DROP, layout_share=SHARE)
    assert a.sensor_layout == {"observed_idx": OBS8, "sensor_dropout": DROP, "layout_share": SHARE}
    obs_dev = torch.tensor(OBS8, dtype=torch.int32, device=DEV)
    counts = []
    for i in range(3):
        rows = torch.tensor([2 * i + 1, 2 * i], dtype=torch.int64, device=DEV)
        assert a.step_rows(store.data, rows)
        mask = a.mask.clone()
        x = store.data[rows].reshape(-1)
        assert torch.equal(a.x, x)
        # the mask is the restatement's at the step count the staging launch read (i)
        rmask = _stage(lib, store.data, rows, bs, NODES, obs_dev, len(OBS8), DROP, SHARE, a.mask_rate, a.seed, i, sensors=False)[2]
        assert np.array_equal(mask.cpu().numpy().reshape(bs, NODES), _layout_mask(pkg, a, bs, OBS8, DROP, SHARE, i, rmask)), i
        b.step(x, x, mask)
        torch.cuda.synchronize()
        assert torch.equal(a.loss, b.loss) and torch.equal(a.out, b.out), i
        assert _same(_state(model_a, a), _state(model_b, b)), i
        counts.append(int(mask.sum()))
    assert a.optimizer_step == 3 and len(set(counts)) > 1, counts           # M differs between steps: it comes from the mask


def test_epoch_sequences_under_a_layout_equal_single_steps(pkg):
    """Two epochs over 23 snapshots in batches of 2 (11 full batches, a ragged one on the sibling) under a layout: captured
    4-step sequences of [staging, the step's launches] must equal the same epochs step by step, bit for bit; the in-place epoch
    (its "seq" graphs) is not taken."""
    bs = 2
    store = _store(pkg, 23)
    res = []
    for kseq in (4, 1):
        model, tr = _trainer(pkg, store, bs)
        tr.epoch_graph_steps = kseq
        tr.set_sensor_layout(OBS8, sensor_dropout=DROP, layout_share=SHARE)
        losses = [tr.fit_epoch(store, bs, shuffle=True, generator=torch.Generator().manual_seed(31 + ep))[0] for ep in range(2)]
        assert tr.optimizer_step == 24 and tr.dropped_steps == 0
        taken = {k[0] for k in tr._graphs if isinstance(k[0], str)}
        assert "seq" not in taken and tr._epoch_buf is None
        assert ("rowseq" in taken) == (kseq > 1), taken
        sib = tr._siblings[1]
        assert sib.sensor_layout == tr.sensor_layout
        res.append((losses, _state(model, tr) + [tr.mask.clone(), sib.mask.clone()]))
    assert res[0][0] == res[1][0], (res[0][0], res[1][0])
    assert _same(res[0][1], res[1][1])
    # the sibling's last mask is a layout mask: only sensors are open, all of them hidden elsewhere
    m = res[0][1][-1].cpu().numpy()
    open_nodes = set(np.flatnonzero(m == 0).tolist())
    assert open_nodes <= set(OBS8) or int(m.sum()) == int(NODES * RATE)        # (or that graph drew the random mode)


def test_set_change_and_clear_between_steps(pkg, lib):
    bs = 2
    store = _store(pkg, 12)
    model, tr = _trainer(pkg, store, bs)
    sib = tr._sibling(1, NODES, store.edge_index(1))                          # (built BEFORE any layout is set: it follows)
    obs_b = [5, 6, 200]
    settings = [None, (OBS8, 0.0, 1.0), (obs_b, 0.0, 1.0), (OBS8, DROP, SHARE), None, (OBS8, 0.0, 1.0)]
    for i, cfg in enumerate(settings):
        if cfg is None:
            tr.clear_sensor_layout()
        else:
            tr.set_sensor_layout(cfg[0], sensor_dropout=cfg[1], layout_share=cfg[2])
        rows = torch.tensor([i, 11 - i], dtype=torch.int64, device=DEV)
        assert tr.step_rows(store.data, rows)
        mask = tr.mask.cpu().numpy().reshape(bs, NODES)
        obs, drop, share = cfg if cfg is not None else (OBS8, 0.0, 0.0)
        obs_dev = torch.tensor(obs, dtype=torch.int32, device=DEV)
        rmask = _stage(lib, store.data, rows, bs, NODES, obs_dev, len(obs), drop, share, tr.mask_rate, tr.seed, i, sensors=False)[2]
        if cfg is None:
            assert np.array_equal(mask, rmask), i
        else:
            assert np.array_equal(mask, _layout_mask(pkg, tr, bs, obs, drop, share, i, rmask)), i
        assert sib.sensor_layout == tr.sensor_layout
    assert tr.optimizer_step == len(settings)
    # a trainer that set and cleared a layout ends an epoch with the bits of one that never had it
    res = []
    for touch in (False, True):
        model, tr = _trainer(pkg, store, bs)
        tr.epoch_graph_steps = 3
        if touch:
            tr.set_sensor_layout(OBS8, sensor_dropout=DROP, layout_share=SHARE)
            tr.clear_sensor_layout()
        loss = tr.fit_epoch(store, bs, shuffle=True, generator=torch.Generator().manual_seed(3))[0]
        # (the graph keys without their buffer addresses: what was captured, and how many keys carry a layout -- none)
        kinds = sorted(str(k[0]) for k in tr._graphs) + [sum(isinstance(e, tuple) and e[:1] == ("layout",) for k in tr._graphs for e in k)]
        res.append((loss, _state(model, tr) + [tr.mask.clone()], kinds))
    assert res[1][2][-1] == 0
    assert res[0][0] == res[1][0] and _same(res[0][1], res[1][1]) and res[0][2] == res[1][2]


# ---- evaluate_store, fit, fine_tune ----------------------------------------------------------------------------------------------
def test_evaluate_store_under_a_layout(pkg):
    bs = 4
    store = _store(pkg, 14)                                                   # 4 + 4 + 4 + 2: a ragged batch
    model, _ = _trainer(pkg, store, bs)
    E = pkg.evaluation
    want = np.ones(NODES, dtype=np.uint8)
    want[OBS8] = 0
    tables = []
    for seed in (0, 12345):
        caps = []
        loss, m = E.evaluate_store(model, store, bs, RATE, seed=seed, gpu_warmup_times=0, observed_idx=OBS8, _capture=caps)
        assert [c[3] for c in caps] == [4, 4, 4, 2]
        for b, (mask, out, x, g) in enumerate(caps):
            assert np.array_equal(mask.cpu().numpy().reshape(g, NODES), np.tile(want, (g, 1))), b
            assert torch.equal(x, store.data[b * bs: b * bs + g].reshape(-1))
        tables.append((loss, {k: v for k, v in m.items() if not k.endswith(("_time", "_throughput"))}))
        assert list(m) == list(E.evaluate_store(model, store, bs, RATE, seed=seed, gpu_warmup_times=0)[1])      # the keys stay
    assert tables[0] == tables[1]                                             # the seed does not enter
    # against layout_errors' MAE of the all-ones layout, on a store that is a multiple of the batch.  Both average
    # |descale(out) - descale(x)| (fp32 values, fp64 sums) over the same (S * (N - K)) hidden entries; evaluate_store forms one
    # fp64 MAE per batch and averages those with equal weights -- the same number up to fp64 summation order, ~1e-15 -- so 1e-6
    # relative (the rounding of fp32 per-batch values, were any formed) is ample.
    full = _store(pkg, 12, like=store)
    _, m = E.evaluate_store(model, full, bs, RATE, gpu_warmup_times=0, observed_idx=OBS8)
    est = pkg.PressureEstimator.for_store(model, full, OBS8, batch_size=bs)
    table = est.layout_errors(full, torch.ones((1, len(OBS8)), dtype=torch.uint8, device=DEV))
    scores = pkg.layout_scores_from_table(table.cpu().numpy())
    assert scores["count"][0] == 12 * (NODES - len(OBS8))
    print("test_mae", m["test_mae"], "layout_errors mae", scores["mae"][0])
    assert abs(m["test_mae"] - scores["mae"][0]) <= 1e-6 * abs(scores["mae"][0])


def _hand_loop(pkg, tr, model, train_store, val_store, epochs, bs, gen, val_seed, patience, min_delta, sp, observed):
    E = pkg.evaluation
    ctl = pkg.epoch_control.EpochController(tr.hparams["lr"], patience=patience, min_delta=min_delta, scheduler_patience=sp)
    out = dict(tr_loss=[], val_loss=[], lr=[], metrics=[])
    for e in range(1, epochs + 1):
        tr_loss, _ = tr.fit_epoch(train_store, bs, generator=gen)
        val_loss, m = E.evaluate_store(model, val_store, bs, tr.mask_rate, seed=val_seed + e, prefix="val", gpu_warmup_times=0,
                                       observed_idx=observed)
        out["lr"].append(ctl.lr)
        ctl.step(tr_loss, val_loss)
        out["tr_loss"].append(tr_loss); out["val_loss"].append(val_loss); out["metrics"].append(m)
        if ctl.stopped:
            break
        tr.set_lr(ctl.lr)
    out["ctl"] = ctl
    return out


@pytest.mark.parametrize("val_layout", [True, False])
@pytest.mark.parametrize("use_graph", [True, False])
def test_fit_under_a_layout_equals_the_hand_written_loop(pkg, use_graph, val_layout, tmp_path):
    nb, bs, St, Sv, epochs, lr, patience, min_delta, sp = 4, 8, 8 * 4 + 3, 8 * 2 + 5, 6, 5e-3, 3, 1e-4, 0
    train_store = _store(pkg, St, seed=3)
    val_store = _store(pkg, Sv, seed=4, like=train_store)
    runs = []
    for _ in range(2):
        model, tr = _trainer(pkg, train_store, bs, nb=nb, use_graph=use_graph, lr=lr)
        tr.epoch_graph_steps = 3
        tr.set_sensor_layout(OBS8, sensor_dropout=0.1, layout_share=0.7)
        runs.append((model, tr))
    (model_a, tr_a), (model_b, tr_b) = runs
    a = tr_a.fit(train_store, val_store, epochs, batch_size=bs, patience=patience, min_delta=min_delta, scheduler_patience=sp,
                 generator=torch.Generator().manual_seed(7), val_seed=100, val_layout=val_layout, save_path=str(tmp_path),
                 model_name="gatres", variant="t")
    hand = _hand_loop(pkg, tr_b, model_b, train_store, val_store, epochs, bs, torch.Generator().manual_seed(7), 100, patience,
                      min_delta, sp, OBS8 if val_layout else None)
    ctl = hand["ctl"]
    eq = lambda u, v: np.array_equal(np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64), equal_nan=True)
    assert a.tr_loss == hand["tr_loss"] and eq(a.val_loss, hand["val_loss"]) and a.lr == hand["lr"]
    assert a.best_epoch == ctl.best_epoch and a.best_loss == ctl.best_loss
    assert a.stopped_epoch == (ctl.epoch if ctl.stopped else None) and a.final_lr == ctl.lr
    assert _same(_state(model_a, tr_a), _state(model_b, tr_b)) and tr_a.optimizer_step == tr_b.optimizer_step
    for k in pkg.evaluation.get_metric_fn_collection("val"):
        assert eq(a.best_metric_dict[k], hand["metrics"][ctl.best_epoch - 1][k]), k
    assert (St % bs) in tr_a._siblings and tr_a._epoch_buf is None
    # the checkpoint says what the model was tuned for
    fresh = pkg.GATResMeanConv(num_blocks=nb, nc=32)
    _, cp = pkg.wdn_io.load_checkpoint(str(tmp_path / "best_gatres_t.pth"), fresh)
    assert cp["sensor_layout"] == {"observed_idx": OBS8, "sensor_dropout": 0.1, "layout_share": 0.7}


def test_fine_tune_is_its_three_calls_and_the_estimator_follows(pkg):
    bs, St, Sv, epochs = 4, 4 * 3 + 1, 4 + 2, 2
    train_store = _store(pkg, St, seed=3)
    val_store = _store(pkg, Sv, seed=4, like=train_store)
    torch.manual_seed(21)
    model_a = pkg.GATResMeanConv(num_blocks=3, nc=32).to(DEV)
    torch.manual_seed(21)
    model_b = pkg.GATResMeanConv(num_blocks=3, nc=32).to(DEV)
    est = pkg.PressureEstimator.for_store(model_a, train_store, OBS8, batch_size=bs)
    before = est.estimate_store(val_store).clone()
    kw = dict(patience=100, scheduler_patience=0, generator=None, val_seed=5)
    ha = est.fine_tune(train_store, val_store, epochs, lr=5e-3, sensor_dropout=0.1, layout_share=0.7, mask_rate=0.9,
                       **{**kw, "generator": torch.Generator().manual_seed(2)})
    tr = pkg.GATResTrainer.for_store(model_b, train_store, bs, lr=5e-3, mask_rate=0.9)
    tr.set_sensor_layout(OBS8, sensor_dropout=0.1, layout_share=0.7)
    hb = tr.fit(train_store, val_store, epochs, batch_size=bs, **{**kw, "generator": torch.Generator().manual_seed(2)})
    torch.cuda.synchronize()
    assert ha.tr_loss == hb.tr_loss and ha.val_loss == hb.val_loss and ha.best_epoch == hb.best_epoch
    assert torch.equal(model_a.flat_parameters, model_b.flat_parameters)
    after = est.estimate_store(val_store)
    fresh = pkg.PressureEstimator.for_store(model_b, train_store, OBS8, batch_size=bs).estimate_store(val_store)
    torch.cuda.synchronize()
    assert torch.equal(after, fresh) and not torch.equal(after, before)


def test_refusals_on_the_device(pkg):
    bs = 2
    store = _store(pkg, 6)
    model, tr = _trainer(pkg, store, bs)
    tr.set_sensor_layout(OBS8)
    x = store.data[:bs].reshape(-1)
    params = model.flat_parameters.detach().clone()
    with pytest.raises(ValueError, match="sensor layout"):
        tr.step(x, x)
    with pytest.raises(ValueError, match="sensor layout"):
        tr.run_step(device_mask=True)
    with pytest.raises(ValueError, match="sensor layout"):
        tr.bind_batches([x])
    with pytest.raises(ValueError, match="sensor layout"):
        tr.step_bound(0)
    with pytest.raises(ValueError, match="sensor layout"):
        tr.steps_bound([0, 0])
    one = pkg.wdn_synth.make_wdn_topology(NODES, PIPES, seed=0)
    multi = pkg.MultiSnapshotStore([(pkg.wdn_synth.make_snapshots(4, NODES, seed=1) * 12.5 + 50.0, one),
                                    (pkg.wdn_synth.make_snapshots(4, NODES, seed=2) * 12.5 + 50.0, one)], device=DEV)
    with pytest.raises(NotImplementedError, match="MultiSnapshotStore"):
        tr.fit_epoch(multi, bs)
    with pytest.raises(NotImplementedError, match="MultiSnapshotStore"):
        tr.fit(multi, store, 1, batch_size=bs)
    _, tm = _trainer(pkg, multi, bs)
    with pytest.raises(NotImplementedError, match="MultiSnapshotStore"):
        tm.set_sensor_layout(OBS8)
    torch.cuda.synchronize()
    assert tr.optimizer_step == 0 and torch.equal(model.flat_parameters, params)        # nothing trained
    # the caller's own mask stays allowed
    tr.step(x, x, torch.ones(bs * NODES, dtype=torch.uint8, device=DEV))
    assert tr.optimizer_step == 1
