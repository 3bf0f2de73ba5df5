"""Fine-tuning under sensor noise on the device: ``gatres_stage_rows_mask_sensors_noisy`` bit for bit against the noise-free
launch (masks, clean elements), against the generator of ``gatres_stage_observed_noisy`` (the draws) and against the host
restatement (``sensor_layout_noise``); the store-fed steps, sequences and epochs under noise; ``evaluate_store``, ``fit`` and
``PressureEstimator.fine_tune`` under it.  Every check but two is an equality: the launches under noise are the layout's
launches on another ``x``.  The two tolerances -- the device's fp32 Box-Muller against the fp64 restatement, 1e-5 absolute, the
bound tests/test_gpu_estimation_noise.py derives for this generator, and ``evaluate_store`` against ``error_map``, 1e-6
relative, the bound tests/test_gpu_sensor_layout.py works out for that pairing -- are named where they are used.

Shapes of the launch: N = 37 (no multiple of 4), 388 (the workload's graph), 2 100 (slices of 525 nodes: the radix path of the
random mask, sensors around the slice boundaries, K = 1 500 for the k-loop's second trip) and 16 500 (slices of 4 125 nodes: the
LDS tile's second pass, sensors on both sides of node 4 096 of a slice)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_sensor_layout import DEV, DROP, NODES, OBS8, RATE, SEED, SHARE, _same, _state, _store, _trainer      # noqa: E402

NSEED = 20260
SENT = -7.25


def _sigma(K):
    """Per sensor, every third one exact (sigma = 0)."""
    return [(0.3, 0.0, 0.7, 0.1, 0.2, 0.0)[k % 6] for k in range(K)]


def _launch(lib, data, rows, G, N, obs_dev, K, drop, share, step, sigma=None, y="own", xoff=0, moff=0, seed=SEED, nseed=NSEED,
            rate=RATE, plain=False):
    """One staging launch into sentinel-filled buffers with guards on both sides; ``sigma`` None: the noise-free symbol
    (``plain``: gatres_stage_rows_mask).  ``y``: "own" buffer, "none" (NULL) or "x" (y_dst == x_dst); ``xoff`` floats / ``moff``
    bytes move the targets off their alignment.  Returns (x [G, N], y or None, mask [G, N]) on the host."""
    pad = 8
    xb = torch.full((pad + xoff + G * N + pad,), SENT, device=DEV)
    yb = torch.full((pad + xoff + G * N + pad,), SENT, device=DEV)
    mb = torch.full((pad + moff + G * N + pad,), 77, dtype=torch.uint8, device=DEV)
    x, yv, mask = xb[pad + xoff: pad + xoff + G * N], yb[pad + xoff: pad + xoff + G * N], mb[pad + moff: pad + moff + G * N]
    node_ptr = torch.arange(0, (G + 1) * N, N, dtype=torch.int32, device=DEV)
    ctr = torch.tensor([step, 0], dtype=torch.int64, device=DEV)
    yp = {"own": yv.data_ptr(), "none": None, "x": x.data_ptr()}[y]
    head = (data.data_ptr(), rows.data_ptr(), N, x.data_ptr(), yp, node_ptr.data_ptr(), G)
    if plain:
        rc = lib.gatres_stage_rows_mask(*head, rate, seed, ctr.data_ptr(), mask.data_ptr(), None)
    elif sigma is None:
        rc = lib.gatres_stage_rows_mask_sensors(*head, obs_dev.data_ptr(), K, drop, share, rate, seed, ctr.data_ptr(), mask.data_ptr(),
                                                None)
    else:
        rc = lib.gatres_stage_rows_mask_sensors_noisy(*head, obs_dev.data_ptr(), K, drop, share, rate, seed, ctr.data_ptr(),
                                                      mask.data_ptr(), sigma.data_ptr(), nseed, None)
    assert rc == 0
    torch.cuda.synchronize()
    for buf, lo, sent in ((xb, pad + xoff, SENT), (mb, pad + moff, 77)):          # nothing written around the batch
        assert buf[:lo].eq(sent).all() and buf[lo + G * N:].eq(sent).all()
    if y == "own":
        assert yb[:pad + xoff].eq(SENT).all() and yb[pad + xoff + G * N:].eq(SENT).all()
    else:
        assert yb.eq(SENT).all()
    return x.cpu().view(G, N), yv.cpu().view(G, N) if y == "own" else None, mask.cpu().numpy().reshape(G, N)


def _device_z(pkg, lib, S, N, obs, step, nseed=NSEED):
    """The draws of gatres_stage_observed_noisy's generator for (seed, member = step, row, k), fp32 ``[S, K]`` on the host: zero
    full rows with sigma = 1, one pair per row (members = 1, member0 = step), read at the sensors."""
    K = len(obs)
    src = torch.zeros((S, N), dtype=torch.float32, device=DEV)
    x = torch.full((S * N,), SENT, device=DEV)
    mask = torch.empty(S * N, dtype=torch.uint8, device=DEV)
    obs_dev = torch.tensor(obs, dtype=torch.int32, device=DEV)
    ones = torch.ones(K, dtype=torch.float32, device=DEV)
    pkg._native.check(lib.gatres_stage_observed_noisy(
        src.data_ptr(), pkg._native.OBSERVED_FULL_ROWS, S, 0, 1, step, N, S, obs_dev.data_ptr(), K, pkg._native.NORMALISE_NONE, 0.0,
        1.0, x.data_ptr(), mask.data_ptr(), None, 0, ones.data_ptr(), nseed, None), "gatres_stage_observed_noisy")
    torch.cuda.synchronize()
    return x.view(S, N)[:, obs].cpu()


def _want_x(data_host, rows, obs, sigma, Z, mode, keep):
    """fp32(row + fp32(sigma * z)) at the kept sensors of layout-mode graphs, the clean row everywhere else (torch on the host:
    a product and a sum, each rounded to fp32).  sigma = 0: the row's value itself."""
    want = data_host[rows].clone()
    sig = torch.tensor(sigma, dtype=torch.float32)
    obs_t = torch.tensor(obs, dtype=torch.int64)
    for g, r in enumerate(rows):
        if mode[g]:
            k = torch.from_numpy(np.flatnonzero(keep[g]))
            r = int(r)
            noisy = data_host[r, obs_t[k]] + sig[k] * Z[r, k]
            want[g, obs_t[k]] = torch.where(sig[k] == 0, data_host[r, obs_t[k]], noisy)
    return want


def _perm(n, k, seed):
    return np.random.RandomState(seed).permutation(n)[:k].tolist()


KERNEL_CASES = {
    # name: (graphs, nodes, sensors, steps, alignment offsets also run)
    "5x37": (5, 37, [0, 3, 17, 35, 36], (0, 1), True),                       # first and last node
    "33x37": (33, 37, [0, 3, 17, 35, 36], (0, 1), False),                    # more graphs than one round of anything
    "3x388": (3, NODES, OBS8, (0, 1), True),                                 # the workload's graph
    "2x2100-slices": (2, 2100, [0, 524, 525, 526, 1049, 1050, 1051, 1574, 1575, 2099], (0,), False),      # slice boundaries
    "2x2100-K1500": (2, 2100, _perm(2100, 1500, 3), (0,), False),            # the k-loop's second trip (1 024 threads)
    # slices [0, 4125), [4125, 8250), ...: tiles start at the slice's first aligned word, 0 and 4124; their second passes at
    # nodes 4096 and 8220
    "1x16500": (1, 16500, [4095, 0, 4096, 4124, 4125, 8219, 8220, 8249, 8250, 12374, 12375, 16467, 16468, 16499, 4097, 8221],
                (0,), False),
    "5x37-K1": (5, 37, [17], (0, 1, 2, 3), False),
    "5x37-KN": (5, 37, _perm(37, 37, 4), (0, 1), False),
}


@pytest.mark.parametrize("case", list(KERNEL_CASES))
def test_the_launch_bit_for_bit(pkg, lib, case):
    G, N, obs, steps, offsets = KERNEL_CASES[case]
    K, S = len(obs), G + 6
    data = torch.from_numpy(np.random.RandomState(G * N).randn(S, N).astype(np.float32)).to(DEV)
    data_host = data.cpu()
    perm = np.random.RandomState(5).permutation(S)[:G]
    if G > 1:
        perm[-1] = perm[0]                                        # shuffled rows with a repeat
    rows = torch.from_numpy(perm.astype(np.int64)).to(DEV)
    obs_dev = torch.tensor(obs, dtype=torch.int32, device=DEV)
    sigma = _sigma(K)
    sig_dev = torch.tensor(sigma, dtype=torch.float32, device=DEV)
    clean = data_host[perm]
    seen = dict(layout=0, random=0, kept=0, dropped=0, noisy=0, exact=0)
    # dropout 0.3 and share 0.6 at every step, and once every sensor of every graph kept: all of them are then staged noisy
    for drop, share, step in [(DROP, SHARE, s) for s in steps] + [(0.0, 1.0, steps[0])]:
        Z = _device_z(pkg, lib, S, N, obs, step)
        ref = pkg.sensor_layout_noise(NSEED, step, range(S), K)
        err = float(np.abs(Z.double().numpy() - ref).max())
        print(f"{case} step {step}: device draws vs sensor_layout_noise max |dz| = {err:.3e}")
        assert err <= 1e-5                                        # (the generator's bound: tests/test_gpu_estimation_noise.py)
        mode, keep = pkg.sensor_layout_draws(SEED, step, G, N, obs, drop, share)
        want = _want_x(data_host, perm, obs, sigma, Z, mode, keep)
        x0, y0, m0 = _launch(lib, data, rows, G, N, obs_dev, K, drop, share, step)                     # the noise-free symbol
        x, y, m = _launch(lib, data, rows, G, N, obs_dev, K, drop, share, step, sigma=sig_dev)
        assert torch.equal(x0, clean) and torch.equal(y0, clean)
        assert np.array_equal(m, m0), (case, step, np.argwhere(m != m0)[:8])
        assert torch.equal(x, want), (case, step, torch.nonzero(x != want)[:8])
        assert torch.equal(y, clean)
        # noise sits only where the mask is open, and only where sigma is not 0
        moved = (x != clean).numpy()
        assert not (moved & (m == 1)).any()
        counted = drop == DROP
        for g in range(G):
            for k in np.flatnonzero(keep[g]) if mode[g] else ():
                assert m[g, obs[k]] == 0 and (sigma[k] != 0 or not moved[g, obs[k]])
                if counted:
                    seen["noisy"] += int(moved[g, obs[k]]); seen["exact"] += int(sigma[k] == 0)
        if not counted:
            assert mode.all() and keep.all() and int(moved.sum()) > 0.99 * G * sum(1 for v in sigma if v != 0)
        # without y_dst, and with y_dst == x_dst: the same x and mask
        for yarg in ("none", "x"):
            x2, _, m2 = _launch(lib, data, rows, G, N, obs_dev, K, drop, share, step, sigma=sig_dev, y=yarg)
            assert torch.equal(x2, want) and np.array_equal(m2, m0), yarg
        if offsets:                                               # x_dst 1, 2, 3 floats and the mask 1 byte off their alignment
            for xoff, yarg in ((1, "own"), (2, "none"), (3, "own")):
                x3, y3, m3 = _launch(lib, data, rows, G, N, obs_dev, K, drop, share, step, sigma=sig_dev, y=yarg, xoff=xoff, moff=1)
                assert torch.equal(x3, want) and np.array_equal(m3, m0) and (y3 is None or torch.equal(y3, clean)), xoff
        if counted:
            seen["layout"] += int(mode.sum()); seen["random"] += int((~mode).sum())
            seen["kept"] += int(keep[mode].sum()); seen["dropped"] += int((~keep[mode]).sum())
    print(case, seen)
    assert seen["layout"] and seen["kept"] and seen["dropped"] and seen["noisy"], seen
    assert seen["random"] or G == 1, seen
    assert seen["exact"] or K == 1, seen


def test_the_draws_are_the_generators_own_and_z_itself_on_zero_data(pkg, lib):
    """data = 0, sigma = 1: x at the kept sensors IS z -- bit-equal to the z of gatres_stage_observed_noisy(member0 = step,
    members = 1) for the same (row, k), and within 1e-5 absolute of ``sensor_layout_noise`` (the fp32 Box-Muller against fp64:
    the bound tests/test_gpu_estimation_noise.py derives for this generator)."""
    G, N, obs = 33, 37, [36, 0, 5, 1, 2, 3, 4, 35, 34, 20, 19, 18, 7, 8, 30, 12]
    K, S = len(obs), 40
    data = torch.zeros((S, N), dtype=torch.float32, device=DEV)
    rows_host = np.random.RandomState(2).permutation(S)[:G]
    rows = torch.from_numpy(rows_host.astype(np.int64)).to(DEV)
    obs_dev = torch.tensor(obs, dtype=torch.int32, device=DEV)
    ones = torch.ones(K, dtype=torch.float32, device=DEV)
    worst = 0.0
    for step in (0, 1, 1 << 40):
        Z = _device_z(pkg, lib, S, N, obs, step)
        x, y, m = _launch(lib, data, rows, G, N, obs_dev, K, DROP, SHARE, step, sigma=ones)
        mode, keep = pkg.sensor_layout_draws(SEED, step, G, N, obs, DROP, SHARE)
        ref = pkg.sensor_layout_noise(NSEED, step, rows_host, K)
        assert (y == 0).all()
        got = x[:, obs]
        for g in range(G):
            on = torch.from_numpy(keep[g] & bool(mode[g]))
            assert torch.equal(got[g][on], Z[rows_host[g]][on]), (step, g)
            assert (got[g][~on] == 0).all()
            if on.any():
                worst = max(worst, float(np.abs(got[g][on].double().numpy() - ref[g][on.numpy()]).max()))
        hidden = [v for v in range(N) if v not in obs]
        assert (x[:, hidden] == 0).all()
    print(f"x at kept sensors vs sensor_layout_noise: max |dz| = {worst:.3e}")
    assert 0.0 < worst <= 1e-5


def test_independence_of_position_batch_size_and_other_sensors(pkg, lib):
    N, obs = 37, [0, 3, 17, 35, 36]
    K = len(obs)
    data = torch.from_numpy(np.random.RandomState(1).randn(9, N).astype(np.float32)).to(DEV)
    obs_dev = torch.tensor(obs, dtype=torch.int32, device=DEV)
    sig = torch.tensor([0.3, 0.5, 0.7, 0.1, 0.2], dtype=torch.float32, device=DEV)

    def at_sensors(rows_list, step, drop=0.0, share=1.0):
        rows = torch.tensor(rows_list, dtype=torch.int64, device=DEV)
        x, _, m = _launch(lib, data, rows, len(rows_list), N, obs_dev, K, drop, share, step, sigma=sig)
        return x[:, obs], m[:, obs]

    for step in (0, 1):
        a, _ = at_sensors([4, 0, 7, 2, 4], step)
        b, _ = at_sensors([7, 4], step)
        c, _ = at_sensors([2, 2, 2, 0, 7, 8, 1, 4, 3, 5, 6], step)
        assert torch.equal(a[0], a[4]) and torch.equal(b[1], a[0]) and torch.equal(b[0], a[2])
        assert torch.equal(c[0], a[3]) and torch.equal(c[1], a[3]) and torch.equal(c[3], a[1]) and torch.equal(c[7], a[0])
        assert not torch.equal(a[0], data[4].cpu()[obs])
        # other sensors' dropout does not move a bit of a kept sensor's value
        d, md = at_sensors([4, 0, 7, 2, 4], step, drop=0.5)
        keep = md == 0
        assert keep.any() and (~keep).any()
        assert torch.equal(d[torch.from_numpy(keep)], a[torch.from_numpy(keep)])
        assert torch.equal(d[torch.from_numpy(~keep)], data[[4, 0, 7, 2, 4]].cpu()[:, obs][torch.from_numpy(~keep)])
    assert not torch.equal(at_sensors([4, 0], 0)[0], at_sensors([4, 0], 1)[0])
    # the step counter is read on the device: the same launch after a bump gives the next step's draws
    G = 5
    rows = torch.tensor([4, 0, 7, 2, 4], dtype=torch.int64, device=DEV)
    x = torch.empty(G * N, device=DEV)
    mask = torch.empty(G * N, dtype=torch.uint8, device=DEV)
    node_ptr = torch.arange(0, (G + 1) * N, N, dtype=torch.int32, device=DEV)
    ctr = torch.zeros(2, dtype=torch.int64, device=DEV)
    for step in (0, 1):
        assert lib.gatres_stage_rows_mask_sensors_noisy(data.data_ptr(), rows.data_ptr(), N, x.data_ptr(), None, node_ptr.data_ptr(), G,
                                                        obs_dev.data_ptr(), K, 0.0, 1.0, RATE, SEED, ctr.data_ptr(), mask.data_ptr(),
                                                        sig.data_ptr(), NSEED, None) == 0
        torch.cuda.synchronize()
        assert torch.equal(x.cpu().view(G, N)[:, obs], at_sensors([4, 0, 7, 2, 4], step)[0]), step
        ctr[0] += 1
    # a NULL step counter is step 0; another noise seed gives other draws, the same masks
    assert lib.gatres_stage_rows_mask_sensors_noisy(data.data_ptr(), rows.data_ptr(), N, x.data_ptr(), None, node_ptr.data_ptr(), G,
                                                    obs_dev.data_ptr(), K, 0.0, 1.0, RATE, SEED, None, mask.data_ptr(), sig.data_ptr(),
                                                    NSEED, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(x.cpu().view(G, N)[:, obs], at_sensors([4, 0, 7, 2, 4], 0)[0])
    xa, _, ma = _launch(lib, data, rows, G, N, obs_dev, K, DROP, SHARE, 0, sigma=sig, nseed=NSEED + 1)
    xb, _, mb = _launch(lib, data, rows, G, N, obs_dev, K, DROP, SHARE, 0, sigma=sig)
    assert np.array_equal(ma, mb) and not torch.equal(xa, xb)


def test_limits(pkg, lib):
    """sigma = 0 is gatres_stage_rows_mask_sensors in every byte; share 0 is gatres_stage_rows_mask in every byte."""
    for G, N, obs in ((5, 37, [0, 3, 17, 35, 36]), (3, NODES, OBS8), (2, 2100, [0, 524, 525, 2099])):
        K = len(obs)
        data = torch.from_numpy(np.random.RandomState(N).randn(G + 3, N).astype(np.float32)).to(DEV)
        rows = torch.from_numpy(np.random.RandomState(6).permutation(G + 3)[:G].astype(np.int64)).to(DEV)
        obs_dev = torch.tensor(obs, dtype=torch.int32, device=DEV)
        zero = torch.zeros(K, dtype=torch.float32, device=DEV)
        sig = torch.tensor(_sigma(K), dtype=torch.float32, device=DEV)
        for step in (0, 1):
            a = _launch(lib, data, rows, G, N, obs_dev, K, DROP, SHARE, step, sigma=zero)
            b = _launch(lib, data, rows, G, N, obs_dev, K, DROP, SHARE, step)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and np.array_equal(a[2], b[2])
            a = _launch(lib, data, rows, G, N, obs_dev, K, DROP, 0.0, step, sigma=sig)
            b = _launch(lib, data, rows, G, N, obs_dev, K, DROP, 0.0, step, plain=True)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and np.array_equal(a[2], b[2])


# ---- the trainer -----------------------------------------------------------------------------------------------------------------
BS = 8
NOISE = [0.4, 0.0, 0.9, 0.2, 0.2, 0.0, 0.6, 0.3]          # physical units, per sensor of OBS8; two of them exact


def _sigma_of(store, noise=NOISE):
    return [float(np.float32(v / (store.std + 1e-8))) for v in noise]


def _expected_step_x(pkg, lib, store, rows_host, tr, step, drop, share, noise=NOISE, nseed=None):
    Z = _device_z(pkg, lib, len(store), NODES, OBS8, step, nseed=tr.seed if nseed is None else nseed)
    mode, keep = pkg.sensor_layout_draws(tr.seed, step, len(rows_host), NODES, OBS8, drop, share)
    return _want_x(store.data.cpu(), np.asarray(rows_host), OBS8, _sigma_of(store, noise), Z, mode, keep).reshape(-1)


def test_step_rows_under_noise_equals_a_step_on_the_arrays_read_back(pkg, lib):
    store = _store(pkg, 3 * BS)
    model_a, a = _trainer(pkg, store, BS)                                     # targets are the inputs: y IS x
    model_c, c = _trainer(pkg, store, BS, targets_are_inputs=False)           # y is a buffer of its own
    model_b, b = _trainer(pkg, store, BS, targets_are_inputs=False)           # steps on what is read back
    for t in (a, c):
        t.set_sensor_layout(OBS8, sensor_dropout=DROP, layout_share=SHARE, noise_std=NOISE)
    assert a.sensor_layout == {"observed_idx": OBS8, "sensor_dropout": DROP, "layout_share": SHARE, "noise_std": NOISE,
                               "noise_seed": a.seed}
    assert a.y is a.x and c.y is not c.x
    moved = 0
    for i in range(3):
        rows_host = [(5 * i + 3 * j) % (3 * BS) for j in range(BS)]
        rows = torch.tensor(rows_host, dtype=torch.int64, device=DEV)
        assert a.step_rows(store.data, rows) and c.step_rows(store.data, rows)
        x_noisy, mask = a.x.clone(), a.mask.clone()
        clean = store.data[rows].reshape(-1)
        assert torch.equal(x_noisy.cpu(), _expected_step_x(pkg, lib, store, rows_host, a, i, DROP, SHARE)), i
        assert torch.equal(c.x, x_noisy) and torch.equal(c.y, clean) and torch.equal(c.mask, mask)
        assert not ((x_noisy != clean) & (mask == 1)).any()                  # the targets the loss reads are clean
        moved += int((x_noisy != clean).sum())
        b.step(x_noisy, clean, mask)
        torch.cuda.synchronize()
        assert torch.equal(a.loss, b.loss) and torch.equal(a.out, b.out), i
        assert torch.equal(c.loss, b.loss) and torch.equal(c.out, b.out), i
        assert _same(_state(model_a, a), _state(model_b, b)) and _same(_state(model_c, c), _state(model_b, b)), i
    assert moved > 0 and a.optimizer_step == 3


def test_epoch_sequences_under_noise_equal_single_steps(pkg):
    """Two epochs over 8 * 5 + 3 snapshots in batches of 8 (5 full batches, a ragged one on the sibling) under noise: captured
    3-step sequences must equal the same epochs step by step, bit for bit -- every step of a sequence reads the step counter on
    the device and draws its own noise."""
    store = _store(pkg, BS * 5 + 3)
    res = []
    for kseq in (3, 1):
        model, tr = _trainer(pkg, store, BS)
        tr.epoch_graph_steps = kseq
        tr.set_sensor_layout(OBS8, sensor_dropout=DROP, layout_share=SHARE, noise_std=NOISE, noise_seed=77)
        losses = [tr.fit_epoch(store, BS, shuffle=True, generator=torch.Generator().manual_seed(31 + ep))[0] for ep in range(2)]
        assert tr.optimizer_step == 12 and tr.dropped_steps == 0
        taken = {k[0] for k in tr._graphs if isinstance(k[0], str)}
        assert "seq" not in taken and tr._epoch_buf is None
        assert ("rowseq" in taken) == (kseq > 1), taken
        sib = tr._siblings[3]
        assert sib.sensor_layout == tr.sensor_layout and sib.sensor_layout["noise_seed"] == 77
        res.append((losses, _state(model, tr) + [tr.mask.clone(), tr.x.clone(), sib.mask.clone(), sib.x.clone()]))
    assert res[0][0] == res[1][0], (res[0][0], res[1][0])
    assert _same(res[0][1], res[1][1])
    # and the noise entered: the same epochs without it end elsewhere
    model, tr = _trainer(pkg, store, BS)
    tr.epoch_graph_steps = 3
    tr.set_sensor_layout(OBS8, sensor_dropout=DROP, layout_share=SHARE)
    for ep in range(2):
        tr.fit_epoch(store, BS, shuffle=True, generator=torch.Generator().manual_seed(31 + ep))
    assert not torch.equal(_state(model, tr)[0], res[0][1][0])


def test_set_change_and_clear_noise_between_steps(pkg, lib):
    """Two steps per setting -- the first captures the setting's graph, the second replays it -- each equal to a step on the
    arrays read back; a setting met again (noise, a layout without it, no layout) stages as it did the first time."""
    store = _store(pkg, 2 * BS)
    model, tr = _trainer(pkg, store, BS)
    model_b, b = _trainer(pkg, store, BS, targets_are_inputs=False)
    other = [0.1] * 8
    # (noise, seed) per setting; noise None or 0: a layout without noise; "off": no layout
    settings = [(NOISE, None), (None, None), (NOISE, None), (other, None), (NOISE, 5), "off", (NOISE, None), (0.0, None)]
    i = 0
    for cfg in settings:
        if cfg == "off":
            tr.clear_sensor_layout()
        else:
            tr.set_sensor_layout(OBS8, sensor_dropout=DROP, layout_share=SHARE, noise_std=cfg[0], noise_seed=cfg[1])
        for _ in range(2):
            rows_host = [(i + 2 * j) % (2 * BS) for j in range(BS)]
            rows = torch.tensor(rows_host, dtype=torch.int64, device=DEV)
            assert tr.step_rows(store.data, rows)
            clean = store.data[rows].reshape(-1)
            if cfg == "off" or cfg[0] is None or cfg[0] == 0.0:
                assert torch.equal(tr.x, clean), i
                assert tr.sensor_layout is None or "noise_std" not in tr.sensor_layout
            else:
                want = _expected_step_x(pkg, lib, store, rows_host, tr, i, DROP, SHARE, noise=cfg[0], nseed=cfg[1])
                assert torch.equal(tr.x.cpu(), want) and not torch.equal(tr.x, clean), i
            b.step(tr.x.clone(), clean, tr.mask.clone())
            torch.cuda.synchronize()
            assert torch.equal(tr.loss, b.loss) and _same(_state(model, tr), _state(model_b, b)), i
            i += 1
    assert tr.optimizer_step == 2 * len(settings)


def test_no_read_back_and_no_allocation_after_the_first_step(pkg, monkeypatch):
    store = _store(pkg, 4 * BS)
    counts = {}
    for noise in (None, NOISE):
        model, tr = _trainer(pkg, store, BS)
        tr.epoch_graph_steps = 2
        tr.set_sensor_layout(OBS8, sensor_dropout=DROP, layout_share=SHARE, noise_std=noise)
        rows = [torch.arange(i * BS, (i + 1) * BS, dtype=torch.int64, device=DEV) for i in range(4)]
        seq = torch.arange(0, 2 * BS, dtype=torch.int64, device=DEV)
        # the first step derives the transposed weights (a graph of its own); after these every graph, the row window and the
        # loss vector exist
        for r in rows[:2]:
            assert tr.step_rows(store.data, r)
        assert tr.steps_rows(store.data, seq) and tr.step_rows(store.data, rows[2]) and tr.steps_rows(store.data, seq)
        torch.cuda.synchronize()
        calls = {"synchronize": 0, "item": 0, "cpu": 0, "tolist": 0, "float": 0, "stream_sync": 0, "event_sync": 0}

        def spy(name, fn):
            def wrapped(*a, **k):
                calls[name] += 1
                return fn(*a, **k)
            return wrapped

        sync = torch.cuda.synchronize
        monkeypatch.setattr(torch.cuda, "synchronize", spy("synchronize", torch.cuda.synchronize))
        monkeypatch.setattr(torch.Tensor, "item", spy("item", torch.Tensor.item))
        monkeypatch.setattr(torch.Tensor, "cpu", spy("cpu", torch.Tensor.cpu))
        monkeypatch.setattr(torch.Tensor, "tolist", spy("tolist", torch.Tensor.tolist))
        monkeypatch.setattr(torch.Tensor, "__float__", spy("float", torch.Tensor.__float__))
        monkeypatch.setattr(torch.cuda.Stream, "synchronize", spy("stream_sync", torch.cuda.Stream.synchronize))
        monkeypatch.setattr(torch.cuda.Event, "synchronize", spy("event_sync", torch.cuda.Event.synchronize))
        before = torch.cuda.memory_stats(DEV)["allocation.all.allocated"]
        graphs_before = len(list(tr._graphs))
        for r in rows[1:]:
            assert tr.step_rows(store.data, r)
        allocated_steps = torch.cuda.memory_stats(DEV)["allocation.all.allocated"] - before
        assert tr.steps_rows(store.data, seq)
        monkeypatch.undo()
        sync()
        assert len(list(tr._graphs)) == graphs_before, (noise, graphs_before, sorted(str(k[0]) for k in tr._graphs))     # replays only
        assert all(v == 0 for v in calls.values()), (noise, str(calls))
        assert allocated_steps == 0, (noise, allocated_steps)
        counts[noise is not None] = (sorted(str(k[0]) for k in tr._graphs), tr.optimizer_step)
    assert counts[True] == counts[False], counts                              # the layout's graphs, no launch sequence more


# ---- evaluate_store, fit, fine_tune ----------------------------------------------------------------------------------------------
def test_evaluate_store_under_noise_is_the_estimators_noisy_pass(pkg):
    bs = 4
    store = _store(pkg, 12)                                                   # a multiple of the batch: equal batch weights
    model, _ = _trainer(pkg, store, bs)
    E = pkg.evaluation
    caps = []
    loss, m = E.evaluate_store(model, store, bs, RATE, gpu_warmup_times=0, observed_idx=OBS8, noise_std=NOISE, noise_seed=NSEED,
                               _capture=caps)
    est = pkg.PressureEstimator.for_store(model, store, OBS8, batch_size=bs)
    raw = pkg.PressureEstimator.for_store(model, store, OBS8, batch_size=bs, keep_observed=False)
    kept = est.estimate_store(store, noise_std=NOISE, noise_seed=NSEED, noise_member=0)
    pred = raw.estimate_store(store, noise_std=NOISE, noise_seed=NSEED, noise_member=0)
    want_mask = np.ones(NODES, dtype=np.uint8)
    want_mask[OBS8] = 0
    hidden = torch.from_numpy(want_mask.astype(bool)).to(DEV)
    zero = [k for k, v in enumerate(NOISE) if v == 0.0]
    for b, (mask, out, x, g) in enumerate(caps):
        s = slice(b * bs, b * bs + g)
        x, out = x.view(g, NODES), out.view(g, NODES)
        assert np.array_equal(mask.cpu().numpy().reshape(g, NODES), np.tile(want_mask, (g, 1)))
        # the staged x: clean at the hidden nodes; at the sensors bit for bit the estimator's noisy reading (which it hands
        # out descaled, as SnapshotStore.descale forms it)
        assert torch.equal(x[:, hidden], store.data[s][:, hidden])
        assert torch.equal(x[:, OBS8] * store.std + store.mean, kept[s][:, OBS8])
        assert not torch.equal(x[:, OBS8], store.data[s][:, OBS8])
        assert torch.equal(x[:, OBS8][:, zero], store.data[s][:, OBS8][:, zero])
        # the predictions are the estimator's
        assert torch.equal(out * store.std + store.mean, pred[s]), b
    # MAE: evaluate_store averages per-batch fp64 MAEs of equal weight, error_map pools the same S * (N - K) hidden entries in
    # fp64 -- the pairing tests/test_gpu_sensor_layout.py bounds by 1e-6 relative
    em = est.error_map(store, kept)
    print("test_mae", m["test_mae"], "error_map hidden_mae", em["hidden_mae"])
    assert abs(m["test_mae"] - em["hidden_mae"]) <= 1e-6 * abs(em["hidden_mae"])
    # noise_std = 0 is the clean layout pass, exactly; the noisy one differs
    clean = E.evaluate_store(model, store, bs, RATE, gpu_warmup_times=0, observed_idx=OBS8)
    for zeros in (0.0, [0.0] * 8):
        again = E.evaluate_store(model, store, bs, RATE, gpu_warmup_times=0, observed_idx=OBS8, noise_std=zeros, noise_seed=3)
        timing = ("_time", "_throughput")
        assert again[0] == clean[0] and {k: v for k, v in again[1].items() if not k.endswith(timing)} == \
            {k: v for k, v in clean[1].items() if not k.endswith(timing)}
    assert loss != clean[0] and list(m) == list(clean[1])
    # the realisation is the seed's: the same seed the same table, another seed another
    same = E.evaluate_store(model, store, bs, RATE, seed=99, gpu_warmup_times=0, observed_idx=OBS8, noise_std=NOISE, noise_seed=NSEED)
    diff = E.evaluate_store(model, store, bs, RATE, gpu_warmup_times=0, observed_idx=OBS8, noise_std=NOISE, noise_seed=NSEED + 1)
    assert same[0] == loss and diff[0] != loss


def _hand_loop(pkg, tr, model, train_store, val_store, epochs, bs, gen, val_seed, patience, min_delta, sp, observed, noise, nseed):
    E = pkg.evaluation
    ctl = pkg.epoch_control.EpochController(tr.hparams["lr"], patience=patience, min_delta=min_delta, scheduler_patience=sp)
    out = dict(tr_loss=[], val_loss=[], lr=[], metrics=[])
    for e in range(1, epochs + 1):
        tr_loss, _ = tr.fit_epoch(train_store, bs, generator=gen)
        val_loss, m = E.evaluate_store(model, val_store, bs, tr.mask_rate, seed=val_seed + e, prefix="val", gpu_warmup_times=0,
                                       observed_idx=observed, noise_std=noise, noise_seed=nseed)
        out["lr"].append(ctl.lr)
        ctl.step(tr_loss, val_loss)
        out["tr_loss"].append(tr_loss); out["val_loss"].append(val_loss); out["metrics"].append(m)
        if ctl.stopped:
            break
        tr.set_lr(ctl.lr)
    out["ctl"] = ctl
    return out


@pytest.mark.parametrize("val", ["noisy", "clean", "random"])
def test_fit_under_noise_equals_the_hand_written_loop(pkg, val, tmp_path):
    nb, bs, St, Sv, epochs, lr, patience, min_delta, sp = 4, BS, BS * 4 + 3, BS * 2 + 5, 5, 5e-3, 3, 1e-4, 0
    train_store = _store(pkg, St, seed=3)
    val_store = _store(pkg, Sv, seed=4, like=train_store)
    runs = []
    for _ in range(2):
        model, tr = _trainer(pkg, train_store, bs, nb=nb, lr=lr)
        tr.epoch_graph_steps = 3
        tr.set_sensor_layout(OBS8, sensor_dropout=0.1, layout_share=0.7, noise_std=NOISE, noise_seed=11)
        runs.append((model, tr))
    (model_a, tr_a), (model_b, tr_b) = runs
    kw = {"noisy": dict(val_noise_seed=42), "clean": dict(val_noise=False), "random": dict(val_layout=False)}[val]
    a = tr_a.fit(train_store, val_store, epochs, batch_size=bs, patience=patience, min_delta=min_delta, scheduler_patience=sp,
                 generator=torch.Generator().manual_seed(7), val_seed=100, save_path=str(tmp_path), model_name="gatres",
                 variant="t", **kw)
    hand = _hand_loop(pkg, tr_b, model_b, train_store, val_store, epochs, bs, torch.Generator().manual_seed(7), 100, patience,
                      min_delta, sp, None if val == "random" else OBS8, NOISE if val == "noisy" else None, 42)
    ctl = hand["ctl"]
    eq = lambda u, v: np.array_equal(np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64), equal_nan=True)
    assert a.tr_loss == hand["tr_loss"] and eq(a.val_loss, hand["val_loss"]) and a.lr == hand["lr"]
    assert a.best_epoch == ctl.best_epoch and a.best_loss == ctl.best_loss
    assert a.stopped_epoch == (ctl.epoch if ctl.stopped else None) and a.final_lr == ctl.lr
    assert _same(_state(model_a, tr_a), _state(model_b, tr_b)) and tr_a.optimizer_step == tr_b.optimizer_step
    for k in pkg.evaluation.get_metric_fn_collection("val"):
        assert eq(a.best_metric_dict[k], hand["metrics"][ctl.best_epoch - 1][k]), k
    # the checkpoint says what the model was tuned for, the noise included
    fresh = pkg.GATResMeanConv(num_blocks=nb, nc=32)
    _, cp = pkg.wdn_io.load_checkpoint(str(tmp_path / "best_gatres_t.pth"), fresh)
    assert cp["sensor_layout"] == {"observed_idx": OBS8, "sensor_dropout": 0.1, "layout_share": 0.7, "noise_std": NOISE,
                                   "noise_seed": 11}


def test_fine_tune_under_noise_is_its_three_calls(pkg):
    bs, St, Sv, epochs = 4, 4 * 3 + 1, 4 + 2, 2
    train_store = _store(pkg, St, seed=3)
    val_store = _store(pkg, Sv, seed=4, like=train_store)
    torch.manual_seed(21)
    model_a = pkg.GATResMeanConv(num_blocks=3, nc=32).to(DEV)
    torch.manual_seed(21)
    model_b = pkg.GATResMeanConv(num_blocks=3, nc=32).to(DEV)
    torch.manual_seed(21)
    model_c = pkg.GATResMeanConv(num_blocks=3, nc=32).to(DEV)
    est = pkg.PressureEstimator.for_store(model_a, train_store, OBS8, batch_size=bs)
    kw = dict(patience=100, scheduler_patience=0, val_seed=5, val_noise_seed=8)
    ha = est.fine_tune(train_store, val_store, epochs, lr=5e-3, sensor_dropout=0.1, layout_share=0.7, mask_rate=0.9,
                       noise_std=NOISE, noise_seed=13, generator=torch.Generator().manual_seed(2), **kw)
    tr = pkg.GATResTrainer.for_store(model_b, train_store, bs, lr=5e-3, mask_rate=0.9)
    tr.set_sensor_layout(OBS8, sensor_dropout=0.1, layout_share=0.7, noise_std=NOISE, noise_seed=13)
    hb = tr.fit(train_store, val_store, epochs, batch_size=bs, generator=torch.Generator().manual_seed(2), **kw)
    torch.cuda.synchronize()
    assert ha.tr_loss == hb.tr_loss and ha.val_loss == hb.val_loss and ha.best_epoch == hb.best_epoch
    assert torch.equal(model_a.flat_parameters, model_b.flat_parameters)
    # without noise_std it is the fine_tune of before: other parameters
    est_c = pkg.PressureEstimator.for_store(model_c, train_store, OBS8, batch_size=bs)
    est_c.fine_tune(train_store, val_store, epochs, lr=5e-3, sensor_dropout=0.1, layout_share=0.7, mask_rate=0.9,
                    generator=torch.Generator().manual_seed(2), patience=100, scheduler_patience=0, val_seed=5)
    torch.cuda.synchronize()
    assert not torch.equal(model_a.flat_parameters, model_c.flat_parameters)
