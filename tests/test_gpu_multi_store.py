"""Training and evaluation from a ``MultiSnapshotStore`` on the device: the multi-matrix collation kernels, a mixed-batch step
against the oracle, ``fit_epoch`` / ``evaluate_store`` / ``fit`` against hand-written loops.  Three synthetic networks of
different sizes, one C-Town-sized, none a multiple of 64 nodes."""
import math

import numpy as np
import pytest
import torch

from test_gpu_model import build, check_gradients_vs_fp64, relerr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NETS = [(388, 430), (150, 163), (501, 560)]            # (nodes, pipes)


def make_nets(pkg, lengths, seed=0):
    out = []
    for k, ((n, p), S) in enumerate(zip(NETS, lengths)):
        ei = pkg.wdn_synth.make_wdn_topology(n, p, seed=k)
        out.append((pkg.wdn_synth.make_snapshots(S, n, seed=seed + 10 * k + 1) * (12.5 - 3 * k) + 50.0 - 10 * k, ei))
    return out


def make_store(pkg, lengths, seed=0, **kw):
    return pkg.MultiSnapshotStore(make_nets(pkg, lengths, seed), device=DEV, **kw)


def node_ptr_of(sizes):
    return torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32, device=DEV)


def stage_multi(pkg, lib, store, recipe, rows, rate, seed, step, required=None, with_y=False):
    """One call of gatres_stage_multi_rows_mask_required into fresh buffers: (x, mask[, y])."""
    sizes = store.nodes_per_graph(recipe)
    N = sum(sizes)
    x = torch.full((N,), float("nan"), device=DEV)
    y = torch.full((N,), float("nan"), device=DEV) if with_y else None
    mask = torch.full((N,), 7, dtype=torch.uint8, device=DEV)
    steps = torch.tensor([step], dtype=torch.int64, device=DEV)
    rp = ri = None
    if required is not None:
        ptr, idx = pkg.evaluation.required_csr(store, required, rate)
        rp = torch.tensor(ptr, dtype=torch.int32, device=DEV)
        ri = torch.tensor(idx if idx else [0], dtype=torch.int32, device=DEV)
    rows = rows.to(DEV)
    pkg._native.check(lib.gatres_stage_multi_rows_mask_required(
        store.table.data_ptr(), store.num_networks, store.net_of_graph(recipe).data_ptr(), rows.data_ptr(),
        node_ptr_of(sizes).data_ptr(), len(sizes), x.data_ptr(), pkg._native.ptr(y), rate, seed, steps.data_ptr(),
        pkg._native.ptr(rp), pkg._native.ptr(ri), mask.data_ptr(), pkg._native.current_stream(x.device)),
        "gatres_stage_multi_rows_mask_required")
    torch.cuda.synchronize()
    return (x, mask, y) if with_y else (x, mask)


# ---- the collation kernels ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("required", [[], [3, 17, 100, 387]])
def test_staging_one_network_is_the_single_matrix_call_byte_for_byte(pkg, lib, required):
    n, B, rate, seed, step = 388, 5, 0.95, 1234, 9
    snaps, ei = make_nets(pkg, [23])[0]
    store = pkg.MultiSnapshotStore([(snaps, ei)], device=DEV)
    rows = torch.tensor([22, 0, 7, 7, 13], dtype=torch.int64, device=DEV)
    x0 = torch.empty(B * n, device=DEV)
    m0 = torch.empty(B * n, dtype=torch.uint8, device=DEV)
    steps = torch.tensor([step], dtype=torch.int64, device=DEV)
    req = torch.tensor(required, dtype=torch.int32, device=DEV) if required else None
    pkg._native.check(lib.gatres_stage_rows_mask_required(
        store.data_of(0).data_ptr(), rows.data_ptr(), n, x0.data_ptr(), None, node_ptr_of([n] * B).data_ptr(), B, rate, seed,
        steps.data_ptr(), pkg._native.ptr(req), len(required), m0.data_ptr(), pkg._native.current_stream(x0.device)), "single")
    x1, m1, y1 = stage_multi(pkg, lib, store, (B,), rows, rate, seed, step, required=[required], with_y=True)
    assert torch.equal(x1, x0) and torch.equal(y1, x0) and torch.equal(m1, m0)
    if not required:                                       # req_ptr == NULL: no required nodes, the same bytes again
        x2, m2 = stage_multi(pkg, lib, store, (B,), rows, rate, seed, step, required=None)
        assert torch.equal(x2, x0) and torch.equal(m2, m0)


def test_staging_three_networks(pkg, lib):
    store = make_store(pkg, [9, 6, 5])
    recipe, rate = (3, 2, 2), 0.95
    rows = torch.tensor([8, 0, 4, 5, 1, 4, 2], dtype=torch.int64)
    required = [[3, 17, 387], [], [0, 250, 499, 500]]
    want = torch.cat([store.data_of(k)[r] for k, r in zip([0, 0, 0, 1, 1, 2, 2], rows.tolist())])
    sizes = store.nodes_per_graph(recipe)
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    masks = {}
    for req in (None, required):
        for step in (4, 5, 4):
            x, mask = stage_multi(pkg, lib, store, recipe, rows, rate, 77, step, required=req)
            assert torch.equal(x, want)                                # the gather, restated with torch
            for g, n in enumerate(sizes):
                mg = mask[ptr[g]:ptr[g + 1]]
                assert int(mg.sum()) == int(n * rate) and int(mg.max()) == 1          # exactly int(n * rate) ones per graph
                if req is not None:
                    k = [0, 0, 0, 1, 1, 2, 2][g]
                    assert bool((mg[req[k]] == 1).all()) if req[k] else True          # a network's sensors are always masked
            key = (req is not None, step)
            if key in masks:
                assert torch.equal(masks[key], mask)                   # the same (seed, step): the same mask
            masks[key] = mask
        assert not torch.equal(masks[(req is not None, 4)], masks[(req is not None, 5)])    # another step: another mask
    # graphs of one network draw different masks (the key holds the node's place in the batch)
    m = masks[(False, 4)]
    assert not torch.equal(m[ptr[0]:ptr[1]], m[ptr[1]:ptr[2]])


def test_bad_arguments_are_refused(pkg, lib):
    store = make_store(pkg, [3, 3, 3])
    recipe = (1, 1, 1)
    sizes = store.nodes_per_graph(recipe)
    x = torch.empty(sum(sizes), device=DEV)
    mask = torch.empty(sum(sizes), dtype=torch.uint8, device=DEV)
    rows = torch.zeros(3, dtype=torch.int64, device=DEV)
    nog, ptr = store.net_of_graph(recipe), node_ptr_of(sizes)
    ok = (store.table.data_ptr(), 3, nog.data_ptr(), rows.data_ptr(), ptr.data_ptr(), 3, x.data_ptr(), None, 0.9, 1, None, None,
          None, mask.data_ptr(), None)
    for i, bad in [(0, None), (1, 0), (2, None), (3, None), (4, None), (5, 0), (6, None), (8, 1.5), (13, None), (11, ptr.data_ptr())]:
        args = list(ok)
        args[i] = bad
        assert lib.gatres_stage_multi_rows_mask_required(*args) == -1, i
    okg = (store.table.data_ptr(), 3, nog.data_ptr(), rows.data_ptr(), ptr.data_ptr(), 3, 1, x.data_ptr(), sum(sizes), None)
    for i, bad in [(0, None), (1, 0), (2, None), (3, None), (4, None), (5, 0), (6, 0), (7, None), (8, 0)]:
        args = list(okg)
        args[i] = bad
        assert lib.gatres_gather_multi_rows(*args) == -1, i
    # a network index outside the table is never followed: that graph is left as it was
    x.fill_(-1.0)
    bad_net = torch.tensor([0, 5, 2], dtype=torch.int32, device=DEV)
    args = list(okg)
    args[2] = bad_net.data_ptr()
    assert lib.gatres_gather_multi_rows(*args) == 0
    torch.cuda.synchronize()
    assert bool((x[sizes[0]:sizes[0] + sizes[1]] == -1.0).all()) and torch.equal(x[:sizes[0]], store.data_of(0)[0])


def test_epoch_gather_equals_the_per_batch_staging(pkg, lib):
    store = make_store(pkg, [40, 17, 23])
    B = 7
    recipe = store.recipe(B)
    sched = store.schedule(B, recipe)
    assert sched.nfull >= 4
    rows = store.epoch_rows(sched, shuffle=True, generator=torch.Generator().manual_seed(3))
    sizes = store.nodes_per_graph(recipe)
    N = sum(sizes)
    for stride in (N, (N + 3) // 4 * 4 + 4):
        buf = torch.full((sched.nfull * stride + 8,), -5.0, device=DEV)
        pkg._native.check(lib.gatres_gather_multi_rows(
            store.table.data_ptr(), 3, store.net_of_graph(recipe).data_ptr(), rows.data_ptr(), node_ptr_of(sizes).data_ptr(), B,
            sched.nfull, buf.data_ptr(), stride, pkg._native.current_stream(buf.device)), "gather")
        torch.cuda.synchronize()
        for j in range(sched.nfull):
            x, _ = stage_multi(pkg, lib, store, recipe, rows[j * B:(j + 1) * B], 0.9, 1, j)
            assert torch.equal(buf[j * stride:j * stride + N], x), j
            assert bool((buf[j * stride + N:(j + 1) * stride] == -5.0).all())      # nothing is written between two batches
        assert bool((buf[sched.nfull * stride:] == -5.0).all())


# ---- a mixed-batch step against the oracle ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False])
def test_mixed_batch_steps_against_the_oracle(pkg, oracle, lib, fused):
    """Three optimisation steps on batches of (3, 2, 2) graphs of the three networks, the masks sampled by the staging launch,
    read back and given to the oracle's training loop.  Bounds: those of tests/test_gpu_headline.py
    (test_headline_config_training_steps_vs_oracle) for single-topology batches -- predictions and loss within 1e-5 (relative
    to the largest value); the gradient of step 0 within 1e-4 as a flat vector AND tensor by tensor under the fp64 arbiter of
    tests/test_gpu_model.py (``check_gradients_vs_fp64`` / ``judge_gradients``: no tensor off the fp64 gradient by more than
    twice the fp32 oracle's own error or the noise floor, a demonstrated kink excepted); parameters after Adam within
    steps x lr x 1.01 with fewer than 1 % of them off by more than 1e-5."""
    NB, NC, steps = 15, 32, 3
    store = make_store(pkg, [12, 8, 7])        # (z-normalised, as every batch the trainer sees and as the headline test's inputs)
    recipe = (3, 2, 2)
    model, p = build(pkg, oracle, NB, NC, seed=5, fused=fused)
    tr = pkg.GATResTrainer.for_store(model, store, 7, graphs_per_network=recipe, fused=fused, seed=4)
    assert tr.fused == fused
    ref = oracle.OracleTrainer(p)
    ei = store.edge_index(recipe).cpu()
    sched = store.schedule(7, recipe)
    rows = store.epoch_rows(sched, shuffle=True, generator=torch.Generator().manual_seed(8))
    errs = []
    for it in range(steps):
        x, mask = stage_multi(pkg, lib, store, recipe, rows[it * 7:(it + 1) * 7], 0.95, tr.seed, it)
        y = x.cpu().reshape(-1, 1)
        hmask = mask.cpu().bool()
        if it == 0:
            xin = y.double().clone()
            xin[hmask] = 0
            p64 = {k: v.double() for k, v in p.items()}

            def grads64(params64):
                l = {k: v.clone().requires_grad_(True) for k, v in params64.items()}
                o = oracle.gatres_forward(l, xin, ei, num_blocks=NB)
                torch.nn.functional.mse_loss(o[hmask], y.double()[hmask]).backward()
                return {k: v.grad for k, v in l.items()}
        l_ref, o_ref = ref.step(y.clone(), y, ei, hmask)
        loss = tr.step(x, x, mask)
        e_out, e_loss = relerr(tr.out, o_ref), relerr(loss, l_ref)
        errs.append((e_out, e_loss))
        print(f"mixed batch fused={fused} step {it}: out {e_out:.3e} loss {e_loss:.3e}")
        assert e_out < 1e-5 and e_loss < 1e-5, (it, e_out, e_loss)
        if it == 0:
            e_flat = relerr(tr.grads, ref.flat("grads"))
            print(f"mixed batch fused={fused} step 0: flat grad {e_flat:.3e}")
            assert e_flat < 1e-4, e_flat
            g_hip, hip, off = tr.grads.detach().cpu(), {}, 0
            for k, v in ref.params.items():
                hip[k] = g_hip[off:off + v.numel()].reshape(v.shape)
                off += v.numel()
            assert off == g_hip.numel()
            ref32 = {k: v.grad.detach().clone() for k, v in ref.params.items()}
            worst_rel, worst_ratio, branch = check_gradients_vs_fp64(hip, ref32, grads64, p64, {}, "mixed")
            print(f"mixed batch fused={fused} step 0: worst tensor error over |g|max vs fp64 {worst_rel:.3e}, worst ratio to the "
                  f"fp32 oracle's error {worst_ratio:.2f}, fp64 kink branch {branch}")
    assert tr.optimizer_step == steps and tr.fault_count == 0
    diff = (model.flat_parameters.detach().cpu().double() - ref.flat("params").double()).abs()
    print(f"mixed batch fused={fused}: max |dp| {float(diff.max()):.3e}, off by > 1e-5: {float((diff > 1e-5).double().mean()):.4f}")
    assert float(diff.max()) <= steps * 5e-4 * 1.01 and float((diff > 1e-5).double().mean()) < 0.01


# ---- fit_epoch ----------------------------------------------------------------------------------------------------------------------
def _model(pkg, nb, seed):
    torch.manual_seed(seed)
    return pkg.GATResMeanConv(num_blocks=nb, nc=32).cuda()


def _hand_epoch(pkg, lib, store, tr, siblings, bs, gen, drop_last=False):
    """The loop a user writes: per batch of the schedule, the mask of the step captured from the staging launch (the sampler's
    key is the optimizer's step count) and ``trainer.step(x, y, mask=captured_mask)`` on the trainer of the batch's recipe."""
    recipe = tr._recipe
    sched = store.schedule(bs, recipe, drop_last)
    rows = store.epoch_rows(sched, shuffle=True, generator=gen)
    total, seen, at, masks = 0.0, 0, 0, []
    for r in [recipe] * sched.nfull + list(sched.tails):
        t = tr if r == recipe else siblings[r]
        g = sum(r)
        x, mask = stage_multi(pkg, lib, store, r, rows[at:at + g], t.mask_rate, t.seed, tr.optimizer_step)
        loss = t.step(x, x, mask=mask)
        total += float(loss.double()) * g
        masks.append(mask)
        seen += g
        at += g
    return total / seen, masks


@pytest.mark.parametrize("use_graph,kseq", [(True, 3), (True, 1), (False, 1)])
def test_fit_epoch_equals_the_hand_written_loop(pkg, lib, use_graph, kseq):
    """Two epochs over (29, 13, 9) snapshots in batches of 6 = (3, 2, 1): six full batches (in place, sequences of 3, when
    captured) and tails of two other recipes on sibling trainers -- parameters, Adam moments, step count and the epoch loss bit
    for bit those of single ``step(x, y, mask=...)`` calls over the same schedule."""
    store = make_store(pkg, [29, 13, 9])
    bs = 6
    model_a, model_b = _model(pkg, 4, 3), _model(pkg, 4, 3)
    tr_a = pkg.GATResTrainer.for_store(model_a, store, bs, seed=11, use_graph=use_graph)
    tr_a.epoch_graph_steps = kseq
    tr_b = pkg.GATResTrainer.for_store(model_b, store, bs, seed=11, use_graph=False)
    recipe = tr_a._recipe
    sched = store.schedule(bs, recipe)
    assert recipe == (3, 2, 1) and sched.nfull == 6 and len(set(sched.tails)) >= 2 and recipe not in sched.tails
    siblings = {r: pkg.GATResTrainer(model_b, store.edge_index(r), store.num_nodes(r), nodes_per_graph=store.nodes_per_graph(r),
                                     seed=11, targets_are_inputs=True, use_graph=False, _share_state_with=tr_b)
                for r in set(sched.tails)}
    for ep in range(2):
        la, _ = tr_a.fit_epoch(store, bs, generator=torch.Generator().manual_seed(50 + ep))
        lb, _ = _hand_epoch(pkg, lib, store, tr_b, siblings, bs, torch.Generator().manual_seed(50 + ep))
        assert la == lb, (ep, la, lb)
    torch.cuda.synchronize()
    assert tr_a.optimizer_step == tr_b.optimizer_step == 2 * len(sched.sizes)
    assert torch.equal(model_a.flat_parameters, model_b.flat_parameters)
    assert torch.equal(tr_a.exp_avg, tr_b.exp_avg) and torch.equal(tr_a.exp_avg_sq, tr_b.exp_avg_sq)
    assert {("recipe", t) for t in sched.tails} == set(tr_a._siblings)
    if use_graph and kseq > 1:
        assert "seq" in {k[0] for k in tr_a._graphs if isinstance(k[0], str)}          # the captured k-step sequences ran
    # drop_last: the full batches only
    before = tr_a.optimizer_step
    tr_a.fit_epoch(store, bs, drop_last=True, generator=torch.Generator().manual_seed(1))
    assert tr_a.optimizer_step == before + sched.nfull


def test_fit_epoch_device_metrics_and_host_metrics_agree(pkg):
    store = make_store(pkg, [29, 13, 9])
    fns = pkg.evaluation.get_metric_fn_collection("train")
    res = []
    for device_metrics in (True, False):
        model = _model(pkg, 4, 3)
        tr = pkg.GATResTrainer.for_store(model, store, 6, seed=11)
        res.append(tr.fit_epoch(store, 6, generator=torch.Generator().manual_seed(2), metric_fn_dict=fns,
                                device_metrics=device_metrics) + (model.flat_parameters.clone(),))
    assert res[0][0] == res[1][0] and torch.equal(res[0][2], res[1][2])       # training is untouched by the metrics launch
    for k, v in res[1][1].items():
        assert res[0][1][k] == pytest.approx(v, rel=1e-5, abs=1e-7), k         # (tests/test_gpu_eval_device.py's agreement rule)


def test_fit_epoch_on_one_network_equals_the_snapshot_store_path(pkg):
    snaps, ei = make_nets(pkg, [71])[0]
    single = pkg.SnapshotStore(snaps, ei, device=DEV)
    multi = pkg.MultiSnapshotStore([(snaps, ei)], device=DEV)
    bs, res = 8, []
    for store in (single, multi):
        model = _model(pkg, 4, 9)
        tr = pkg.GATResTrainer.for_store(model, store, bs, seed=6)
        tr.epoch_graph_steps = 3
        losses = [tr.fit_epoch(store, bs, generator=torch.Generator().manual_seed(20 + ep))[0] for ep in range(2)]
        assert tr.optimizer_step == 2 * 9
        res.append((losses, model.flat_parameters.clone(), tr.exp_avg.clone(), tr.exp_avg_sq.clone()))
    assert res[0][0] == res[1][0], (res[0][0], res[1][0])
    for a, b in zip(res[0][1:], res[1][1:]):
        assert torch.equal(a, b)


# ---- evaluate_store ---------------------------------------------------------------------------------------------------------------
def _host_eval(pkg, model, store, caps, recipes, prefix):
    """``test_one_epoch``'s per-batch arithmetic on the device masks (tests/test_gpu_eval_device.py ``host_metrics``, with the
    batch's ``edge_index`` taken by recipe), for the whole batch and for every network's node range."""
    E = pkg.evaluation
    fns = E.get_metric_fn_collection(prefix)
    K = store.num_networks
    tot = {"loss": 0.0, **{k: 0.0 for k in fns}}
    net = [{"loss": 0.0, **{k: 0.0 for k in fns}} for _ in range(K)]
    n, net_n = 0, [0] * K
    for (mask, out, x, g), r in zip(caps, recipes):
        m = mask.bool()
        y = x.reshape(-1, 1)
        x1 = y.clone()
        x1[m] = 0
        with torch.no_grad():
            o = model(x1, store.edge_index(r))
        assert torch.equal(o, out), "predictions differ from model(x1, edge_index)"

        def add(acc, sel, w):
            yp, yt = o[sel], y[sel]
            acc["loss"] += float(torch.nn.MSELoss()(yp, yt)) * w
            pr = E.descale(yp, store.norm_type, mean=store.mean, std=store.std)
            tr = E.descale(yt, store.norm_type, mean=store.mean, std=store.std)
            for k, fn in fns.items():
                acc[k] += float(fn(pr, tr)) * w

        add(tot, m, g)
        n += g
        for k, (lo, hi) in enumerate(store.node_ranges(r)):
            if hi > lo:
                sel = torch.zeros_like(m)
                sel[lo:hi] = m[lo:hi]
                add(net[k], sel, r[k])
                net_n[k] += r[k]
    return {k: v / n for k, v in tot.items()}, [{k: v / net_n[i] for k, v in d.items()} for i, d in enumerate(net)]


def _close(got, want, name):
    if math.isnan(want):
        assert math.isnan(got), name
    else:
        assert got == pytest.approx(want, rel=1e-5, abs=1e-7), name


@pytest.mark.parametrize("sensors", [False, True])
def test_evaluate_store_against_the_host_loop(pkg, sensors):
    store = make_store(pkg, [29, 13, 9], seed=4)
    model = _model(pkg, 15, 14)
    E = pkg.evaluation
    bs, rate, prefix = 6, 0.95, "test"
    required = [[3, 17, 100, 387], [149], [0, 1, 250, 499, 500]]
    kw = dict(do_test_on_sensors=True, required_idx=required) if sensors else {}
    caps = []
    loss, m, nets = E.evaluate_store(model, store, bs, rate, prefix=prefix, gpu_warmup_times=2, seed=5, per_network=True,
                                     _capture=caps, **kw)
    sched = store.schedule(bs)
    recipes = [sched.recipe] * sched.nfull + list(sched.tails)
    assert [c[3] for c in caps] == sched.sizes and sum(sched.sizes) == len(store)
    rows = store.epoch_rows_host(sched, shuffle=False)
    at = 0
    for (mask, _, x, g), r in zip(caps, recipes):
        assert torch.equal(x, store.batch(r, rows[at:at + g]).reshape(-1))                # taken in store order
        at += g
        off = 0
        for k, b in enumerate(r):
            n = store.nodes_per_graph_of(k)
            for _ in range(b):
                mg = mask[off:off + n]
                assert int(mg.sum()) == int(n * rate)
                if sensors:
                    assert bool((mg[required[k]] == 1).all())
                off += n
    post = "_sensor" if sensors else ""
    assert list(m) == [k + post for k in E.get_metric_fn_collection(prefix)] + [f"{prefix}_time{post}", f"{prefix}_throughput{post}"]
    h, h_nets = _host_eval(pkg, model, store, caps, recipes, prefix)
    _close(loss, h.pop("loss"), "loss")
    for k, v in h.items():
        _close(m[k + post], v, k)
    assert len(nets) == 3
    for k in range(3):
        _close(nets[k]["loss"], h_nets[k].pop("loss"), f"net {k} loss")
        for name, v in h_nets[k].items():
            _close(nets[k][name + post], v, f"net {k} {name}")
    # the default call returns the same loss and metrics (the per-network launches change nothing else)
    loss2, m2 = E.evaluate_store(model, store, bs, rate, prefix=prefix, gpu_warmup_times=0, seed=5, **kw)
    assert loss2 == loss and all(m2[k] == m[k] for k in m if "time" not in k and "throughput" not in k)


# ---- fit ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("criterion", ["mse", "mae"])
def test_fit_equals_the_hand_written_loop(pkg, criterion):
    """``fit(multi_train, multi_val)`` against fit_epoch + evaluate_store + the host controller, under the comparison rule of
    tests/test_gpu_fit.py (its ``_hand_loop`` and ``_assert_same_run``, which take any store): the same losses, decisions,
    learning rates, parameters and moments."""
    import test_gpu_fit as TF
    train = make_store(pkg, [29, 13, 9], seed=1)
    val = make_store(pkg, [11, 5, 4], seed=2, mean=train.mean, std=train.std)
    bs, epochs, lr, patience, min_delta, sp = 6, 6, 5e-3, 3, 1e-4, 0
    runs = []
    for _ in range(2):
        model = _model(pkg, 4, 21)
        tr = pkg.GATResTrainer.for_store(model, train, bs, lr=lr, criterion=criterion)
        tr.epoch_graph_steps = 3
        runs.append((model, tr))
    (model_a, tr_a), (model_b, tr_b) = runs
    a = tr_a.fit(train, val, epochs, batch_size=bs, patience=patience, min_delta=min_delta, scheduler_patience=sp,
                 generator=torch.Generator().manual_seed(7), val_seed=100)
    hand = TF._hand_loop(pkg, tr_b, model_b, train, val, epochs, bs, bs, torch.Generator().manual_seed(7), 100, patience,
                         min_delta, sp)
    TF._assert_same_run(pkg, a, tr_a, model_a, hand, tr_b, model_b)
    assert len(set(a.val_loss)) > 1 and any(isinstance(k, tuple) for k in tr_a._siblings)


def test_internal_train_takes_multi_network_stores(pkg):
    import argparse
    train = make_store(pkg, [29, 13, 9], seed=1)
    val = make_store(pkg, [11, 5, 4], seed=2, mean=train.mean, std=train.std)
    args = argparse.Namespace(lr=5e-3, weight_decay=6e-6, epochs=2, mask_rate=0.95, criterion="mse", batch_size=6, patience=5,
                              min_delta=1e-4, scheduler="ReduceLROnPlateau", scheduler_patience=2)
    best, metrics = pkg.internal_train(args, _model(pkg, 4, 2), train, val, generator=torch.Generator().manual_seed(1))
    assert math.isfinite(best) and set(metrics) == set(pkg.evaluation.get_metric_fn_collection("val"))


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals(pkg):
    train = make_store(pkg, [29, 13, 9], seed=1)
    model = _model(pkg, 2, 1)
    with pytest.raises(ValueError, match="flat"):
        pkg.evaluation.evaluate_store(model, train, 6, 0.95, do_test_on_sensors=True, required_idx=[3, 17])
    tr = pkg.GATResTrainer.for_store(model, train, 6)
    two = pkg.MultiSnapshotStore(make_nets(pkg, [7, 5])[:2], device=DEV, mean=train.mean, std=train.std)
    with pytest.raises(ValueError, match="networks"):
        tr.fit(train, two, 1, batch_size=6)
    with pytest.raises(ValueError):
        pkg.GATResTrainer.for_store(model, train, 2)                              # fewer graphs than networks
    other = pkg.GATResTrainer.for_store(model, train, 6, graphs_per_network=(2, 2, 2))
    assert other._recipe == (2, 2, 2)
    single = pkg.SnapshotStore(*make_nets(pkg, [9])[0], device=DEV)
    with pytest.raises(ValueError):
        pkg.GATResTrainer.for_store(model, single, 4).fit_epoch(train, 4)          # a trainer of another composition
    # data parallel: refused by name (the one-rank collective-path trainer has world == 1 and trains; the check itself is what a
    # second rank would meet)
    one_rank = pkg.GATResTrainer.for_store(_model(pkg, 2, 1), train, 6, force_collective_path=True)
    one_rank.fit_epoch(train, 6, generator=torch.Generator().manual_seed(0))
    one_rank.world = 2
    with pytest.raises(NotImplementedError, match="MultiSnapshotStore"):
        one_rank.fit_epoch(train, 6)
    one_rank.world = 1
