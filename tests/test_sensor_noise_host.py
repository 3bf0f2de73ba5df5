"""Fine-tuning under sensor noise, on the host: ``gatres_stage_rows_mask_sensors_noisy`` is declared, exported and bound without
an ABI change and refuses its bad arguments before any launch; ``sensor_layout_noise`` holds against ``reading_noise`` and on
two answers computed here with plain Python integers; ``SensorLayout`` converts units by the statement ``PressureEstimator``
uses; ``set_sensor_layout`` and ``evaluate_store`` refuse what they can refuse without a device.  No GPU, no kernel launches."""
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "gatres_stage_rows_mask_sensors_noisy"
P = 4096                       # (any non-null address: a refused call never reads it)
Q = 1 << 20
BADARG = -1
M64 = (1 << 64) - 1


def header():
    with open(os.path.join(ROOT, "include", "gatres.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


# ---- 1. the symbol and its refusals ---------------------------------------------------------------------------------------------
def test_the_symbol_is_declared_exported_and_bound_and_the_abi_stays(pkg, lib):
    hdr = header()
    assert re.search(r"\b%s\s*\(" % SYMBOL, hdr)
    assert hdr.index("gatres_stage_rows_mask_sensors(") < hdr.index(SYMBOL + "(") < hdr.index("gatres_stage_multi_rows_mask_required(")
    assert hasattr(lib, SYMBOL), f"{SYMBOL} is not exported"
    S = pkg._native.SIGNATURES
    # the noise-free symbol's arguments, sigma and noise_seed in front of the stream
    N = pkg._native
    assert S[SYMBOL][1] == S["gatres_stage_rows_mask_sensors"][1][:-1] + [N._P, N._U64, N._P] and len(S[SYMBOL][1]) == 18
    assert "#define GATRES_ABI_VERSION 9" in hdr and pkg._native.ABI_VERSION == 9
    assert pkg.sensor_layout_noise is pkg.sensor_layout.sensor_layout_noise and "sensor_layout_noise" in pkg.__all__


def stage(lib, data=P, rows=2 * P, n=37, x=Q, y=None, node_ptr=3 * P, graphs=3, observed=5 * P, k=5, dropout=0.3, share=0.6,
          rate=0.95, seed=9, step=None, mask=3 * Q, sigma=5 * Q, noise_seed=4):
    return lib.gatres_stage_rows_mask_sensors_noisy(data, rows, n, x, y, node_ptr, graphs, observed, k, dropout, share, rate, seed,
                                                    step, mask, sigma, noise_seed, None)


def test_the_symbol_checks_its_arguments_before_any_launch(pkg, lib):
    assert pkg._native.ERRORS[BADARG]                            # (GATRES_E_BADARG)
    # whatever the noise-free symbol refuses
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
    # its own: sigma NULL; sigma (5 floats) inside or across an end of x_dst / y_dst (3 * 37 floats) or mask (3 * 37 bytes)
    assert stage(lib, sigma=None) == BADARG
    total = 3 * 37
    for base, nbytes in ((Q, 4 * total), (3 * Q, total)):
        for off in (0, 4, nbytes - 4, -16):                      # (first byte, inside, last word, the last float of sigma reaches in)
            assert stage(lib, sigma=base + off) == BADARG, (base, off)
    for off in (0, 4 * total - 4, -16):
        assert stage(lib, y=7 * Q, sigma=7 * Q + off) == BADARG, off


# ---- 2. the host restatement ----------------------------------------------------------------------------------------------------
def _mix(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def _z(seed, step, row, K, k):
    """include/gatres.h's generator in Python integers and math: (u1 numerator, u2 numerator, z)."""
    stream = _mix(seed + 0x9E3779B97F4A7C15 * (step + 1))
    h = _mix(stream + 0xBF58476D1CE4E5B9 * (row * K + k + 1))
    a, b = (h >> 40) + 1, (h >> 8) & 0xFFFFFF
    return a, b, math.sqrt(-2.0 * math.log(a * 2.0 ** -24)) * math.cos(2.0 * math.pi * (b * 2.0 ** -24))


def test_sensor_layout_noise_against_reading_noise(pkg):
    rows, K = [4, 0, 7, 2, 4], 5
    for seed, step in ((9, 0), (9, 1), ((1 << 64) - 1, 1 << 40)):
        z = pkg.sensor_layout_noise(seed, step, rows, K)
        full = pkg.reading_noise(seed, 1, 8, K, member0=step)
        assert z.dtype == np.float64 and z.shape == (5, K)
        assert np.array_equal(z, full[rows, 0, :])
        assert np.array_equal(z[0], z[4])                        # the same row: the same draws, wherever it stands in the batch
        assert np.array_equal(pkg.sensor_layout_noise(seed, step, rows[::-1], K), z[::-1])
    # the step is the member, K enters the key
    assert not np.array_equal(pkg.sensor_layout_noise(9, 0, rows, K), pkg.sensor_layout_noise(9, 1, rows, K))
    assert not np.array_equal(pkg.sensor_layout_noise(9, 0, rows, K)[:, :4], pkg.sensor_layout_noise(9, 0, rows, 4))
    with pytest.raises(ValueError):
        pkg.sensor_layout_noise(9, 0, [], K)
    with pytest.raises(ValueError):
        pkg.sensor_layout_noise(9, 0, [-1], K)
    with pytest.raises(ValueError, match="seed"):
        pkg.sensor_layout_noise(1 << 64, 0, [0], K)


def test_sensor_layout_noise_on_two_integer_cases(pkg):
    # (seed, step, row, K, k) -> the two 24-bit integers of the hash, worked out with Python integers
    assert _z(9, 0, 4, 5, 2)[:2] == (9816179, 431299)
    assert _z((1 << 64) - 1, 3, 0, 8, 7)[:2] == (3345867, 9143082)
    a = pkg.sensor_layout_noise(9, 0, [4, 1, 4], 5)
    assert a[0, 2] == pytest.approx(1.0218874322278961, abs=1e-14) and a[2, 2] == a[0, 2]
    assert a[0, 2] == pytest.approx(_z(9, 0, 4, 5, 2)[2], abs=1e-14)
    b = pkg.sensor_layout_noise((1 << 64) - 1, 3, [0], 8)
    assert b[0, 7] == pytest.approx(-1.724507554448248, abs=1e-14)
    assert b[0, 7] == pytest.approx(_z((1 << 64) - 1, 3, 0, 8, 7)[2], abs=1e-14)
    for k in range(8):
        assert b[0, k] == pytest.approx(_z((1 << 64) - 1, 3, 0, 8, k)[2], abs=1e-14)


# ---- 3. units -------------------------------------------------------------------------------------------------------------------
def test_the_layout_converts_units_as_the_estimator_does(pkg):
    import torch
    L, E = pkg.sensor_layout, pkg.estimation
    obs, std, eps = [3, 1, 36], 12.5, 1e-8
    est = pkg.PressureEstimator.__new__(pkg.PressureEstimator)    # (what _sigma reads of an estimator)
    est.observed_idx, est.norm_type, est.std, est.eps, est._sigma_cache, est.device = obs, "znorm", std, eps, {}, torch.device("cpu")
    for noise in (0.25, [0.5, 0.0, 2.0]):
        lay = L.SensorLayout(obs, 37, 0.0, 1.0, "cpu", noise_std=noise, noise_seed=7, norm=("znorm", std, eps))
        want = est._sigma(noise, pkg._native.OBSERVED_FULL_ROWS)
        assert lay.sigma.dtype == torch.float32 and torch.equal(lay.sigma, want)
        v = np.full(3, noise) if np.isscalar(noise) else np.asarray(noise)
        assert np.array_equal(lay.sigma.numpy(), (v / (std + eps)).astype(np.float32))
        assert lay.noise_std == [float(x) for x in v] and lay.noise_seed == 7
        assert lay.key()[-2:] == (lay.sigma.data_ptr(), 7) and len(lay.key()) == 7
        assert lay.describe()["noise_std"] == [float(x) for x in v] and lay.describe()["noise_seed"] == 7
    # a store that is not normalised: physical units are the store's
    est.norm_type = "unused"
    lay = L.SensorLayout(obs, 37, 0.0, 1.0, "cpu", noise_std=[0.5, 0.0, 2.0], noise_seed=7, norm=("unused", None, 0.0))
    assert torch.equal(lay.sigma, est._sigma([0.5, 0.0, 2.0], pkg._native.OBSERVED_FULL_ROWS))
    assert lay.sigma.tolist() == [0.5, 0.0, 2.0]
    # the readings layout is never divided, whatever the store (the statement both callers share)
    assert np.array_equal(E.noise_sigma(0.5, 3, "znorm", std, eps, full_rows=False), np.full(3, 0.5, dtype=np.float32))
    # None and all zeros: no noise at all -- today's key and today's three keys
    for noise in (None, 0.0, [0.0, 0.0, 0.0]):
        lay = L.SensorLayout(obs, 37, 0.25, 0.5, "cpu", noise_std=noise, noise_seed=7, norm=("znorm", std, eps))
        assert lay.sigma is None and len(lay.key()) == 5
        assert lay.describe() == {"observed_idx": obs, "sensor_dropout": 0.25, "layout_share": 0.5}
    # physical units need the store's normalisation
    with pytest.raises(ValueError, match="store_norm"):
        L.SensorLayout(obs, 37, 0.0, 1.0, "cpu", noise_std=0.5, noise_seed=7, norm=None)


# ---- 4. refusals in Python ------------------------------------------------------------------------------------------------------
def stub_trainer(pkg, world=1, recipe=None, npg=(37, 37), norm=("znorm", 12.5, 1e-8)):
    """What set_sensor_layout reads of a trainer before it uploads anything."""
    import torch
    t = pkg.GATResTrainer.__new__(pkg.GATResTrainer)
    t.world, t._recipe, t._npg_list, t._siblings, t._layout = world, recipe, list(npg) if npg else None, {}, None
    t.node_ptr = None if not npg else torch.zeros(len(npg) + 1, dtype=torch.int32)
    t.device = torch.device("cpu")
    t._mask_sig = None
    t.seed, t.store_norm = 21, norm
    return t


def test_the_sensor_layout_dict_without_noise_is_the_three_keys(pkg):
    t = stub_trainer(pkg)
    want = {"observed_idx": [3, 1, 36], "sensor_dropout": 0.25, "layout_share": 0.5}
    for kw in ({}, {"noise_std": None}, {"noise_std": 0.0}, {"noise_std": [0.0, 0.0, 0.0], "noise_seed": 5}):
        t.set_sensor_layout([3, 1, 36], sensor_dropout=0.25, layout_share=0.5, **kw)
        assert t.sensor_layout == want and list(t.sensor_layout) == list(want), kw
        assert t._layout.sigma is None
    # with noise: the two more keys; the seed defaults to the trainer's effective seed; siblings follow
    sib = stub_trainer(pkg, npg=(37,))
    t._siblings[1] = sib
    t.set_sensor_layout([3, 1, 36], sensor_dropout=0.25, layout_share=0.5, noise_std=0.5)
    assert t.sensor_layout == {**want, "noise_std": [0.5, 0.5, 0.5], "noise_seed": 21} and sib.sensor_layout == t.sensor_layout
    t.set_sensor_layout([3, 1, 36], noise_std=[0.5, 0.0, 1.0], noise_seed=(1 << 64) - 1)
    assert t.sensor_layout["noise_std"] == [0.5, 0.0, 1.0] and t.sensor_layout["noise_seed"] == (1 << 64) - 1
    t.clear_sensor_layout()
    assert t.sensor_layout is None and sib.sensor_layout is None


def test_set_sensor_layout_refuses_bad_noise(pkg):
    t = stub_trainer(pkg)
    for bad in (-0.1, [0.5, -1.0, 0.5]):
        with pytest.raises(ValueError, match="non-negative"):
            t.set_sensor_layout([3, 1, 36], noise_std=bad)
    for bad in (float("nan"), float("inf"), [0.5, float("inf"), 0.5]):
        with pytest.raises(ValueError, match="finite"):
            t.set_sensor_layout([3, 1, 36], noise_std=bad)
    for bad in ([0.5, 0.5], [0.5] * 4, [[0.5, 0.5, 0.5]], "abc"):
        with pytest.raises(ValueError, match="noise_std"):
            t.set_sensor_layout([3, 1, 36], noise_std=bad)
    for bad in (-1, 1 << 64, 1.5, True):
        with pytest.raises(ValueError, match="seed"):
            t.set_sensor_layout([3, 1, 36], noise_std=0.5, noise_seed=bad)
    assert t.sensor_layout is None
    # physical units without the store's normalisation: refused, and the message says how to supply it
    with pytest.raises(ValueError, match="for_store.*store_norm"):
        stub_trainer(pkg, norm=None).set_sensor_layout([3, 1, 36], noise_std=0.5)
    # whatever a layout refuses, noise refuses with it
    with pytest.raises(NotImplementedError, match="world size 2"):
        stub_trainer(pkg, world=2).set_sensor_layout([1, 2], noise_std=0.5)
    with pytest.raises(NotImplementedError, match="MultiSnapshotStore"):
        stub_trainer(pkg, recipe=(1, 1)).set_sensor_layout([1, 2], noise_std=0.5)
    with pytest.raises(ValueError, match="duplicates"):
        t.set_sensor_layout([1, 2, 1], noise_std=0.5)
    with pytest.raises(ValueError, match="sensor_dropout"):
        t.set_sensor_layout([1, 2], sensor_dropout=1.0, noise_std=0.5)


def test_evaluate_store_refuses_noise_without_a_layout_and_bad_noise(pkg):
    class Store:                                                 # (what evaluate_store reads of a store before the refusals)
        nodes_per_graph = 37
        norm_type, mean, std, eps = "znorm", 50.0, 12.5, 1e-8

        def __len__(self):
            return 4

    ev = pkg.evaluation.evaluate_store
    model = object()
    with pytest.raises(ValueError, match="observed_idx"):
        ev(model, Store(), 4, 0.95, noise_std=0.5)
    with pytest.raises(ValueError, match="observed_idx"):
        pkg.evaluation._ValidationPass(model, Store(), 4, 0.95, noise_std=0.5)
    with pytest.raises(ValueError, match="non-negative"):
        ev(model, Store(), 4, 0.95, observed_idx=[1, 2], noise_std=-1.0)
    with pytest.raises(ValueError, match="noise_std"):
        ev(model, Store(), 4, 0.95, observed_idx=[1, 2], noise_std=[0.5] * 3)
    with pytest.raises(ValueError, match="seed"):
        ev(model, Store(), 4, 0.95, observed_idx=[1, 2], noise_std=0.5, noise_seed=-1)
    multi = pkg.MultiSnapshotStore.__new__(pkg.MultiSnapshotStore)
    with pytest.raises(NotImplementedError, match="MultiSnapshotStore"):
        ev(model, multi, 4, 0.95, observed_idx=[1, 2], noise_std=0.5)
