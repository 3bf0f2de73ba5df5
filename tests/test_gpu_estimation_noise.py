"""Estimation under sensor noise on the device (``noise_std`` / ``estimate_ensemble`` / ``noise_report`` of
estimation.PressureEstimator; gatres_stage_observed_noisy, gatres_ensemble_reduce and gatres_node_spread_moments of
k_estimate.hip): the draws against ``reading_noise``, the noisy staging and the reduce bit for bit against torch / numpy
statements, the ensemble against its pass written out, the report against its passes and formulas, and the passes' freedom from
synchronisation.

Shapes: 37 nodes (no multiple of 4) with the unsorted sensors [36, 0, 5]; 40 nodes for whole chunks and the vector paths; one
graph of 1 030 nodes with sensors on both sides of the staging kernel's tile boundary at node 1 024; S = 5 snapshots of M = 3
members at batch size 4 -- the 15 pairs fall as 4, 4, 4, 3: a snapshot's members straddle batches and the last batch is ragged
--; 388 nodes once, for gatres_small at batch size 32 on the window kernel."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_estimation import (DEV, N37, OBS, garbage, hand_loop, make_store, raw_snapshots, small_model, stage,      # noqa: E402
                                 stream, topology, torch_stage)
from estimation_refs import numpy_reduce, torch_stage_available      # noqa: E402,F401
from test_gpu_model import relerr      # noqa: E402

SEED = 20260
S5, M3, BS4 = 5, 3, 4
OBS40 = [39, 3, 4, 5, 0]
SIGMA = {3: [0.3, 0.0, 0.7], 5: [0.3, 0.0, 0.7, 0.1, 0.2]}      # per sensor, one of them exact
# [S5, 3]: a snapshot with every reading, one with none, mixed rows
AVAIL5 = [[1, 1, 1], [0, 0, 0], [1, 0, 1], [0, 1, 1], [1, 1, 0]]


def stage_noisy(pkg, lib, src, layout, first_pair, members, member0, n, g, observed, sigma, seed, available=None, nan_is_missing=0,
                normalise=0, offset=0.0, factor=1.0, target=None):
    """One gatres_stage_observed_noisy launch into a garbage-filled target (``target``: the two addresses to write to instead).
    Returns the target."""
    x, mask = garbage(g * n)
    xp, mp = (x.data_ptr(), mask.data_ptr()) if target is None else target
    obs = torch.tensor(observed, dtype=torch.int32, device=DEV)
    sig = torch.as_tensor(sigma, dtype=torch.float32).to(DEV)
    assert sig.shape == (len(observed),)
    pkg._native.check(lib.gatres_stage_observed_noisy(
        src.data_ptr(), layout, src.shape[0], first_pair, members, member0, n, g, obs.data_ptr(), len(observed), normalise, offset,
        factor, xp, mp, pkg._native.ptr(available), nan_is_missing, sig.data_ptr(), seed, stream()), "gatres_stage_observed_noisy")
    return x, mask


def device_z(pkg, lib, seed, members, rows, observed, n, member0=0):
    """The device's own draws, fp32 ``[rows, members, K]``: zero readings (full rows, nothing normalised) with sigma = 1 staged
    for every pair in one launch, read at the sensors."""
    src = torch.zeros((rows, n), dtype=torch.float32, device=DEV)
    x, _ = stage_noisy(pkg, lib, src, 0, 0, members, member0, n, rows * members, observed, [1.0] * len(observed), seed)
    return x.view(rows, members, n)[:, :, observed].contiguous()


def pair_values(values, sigma, Z):
    """``values`` [S, K] and the draws ``Z`` [S, M, K] -> the noisy values of the S * M pairs, snapshot-major [S * M, K], formed
    by torch in fp32: a product and a sum, each rounded."""
    sig = torch.as_tensor(sigma, dtype=torch.float32).to(DEV)
    return (values.unsqueeze(1) + sig * Z).reshape(-1, values.shape[1])


def avail(rows):
    return torch.tensor(rows, dtype=torch.uint8, device=DEV)


# ---- 1. the draws -----------------------------------------------------------------------------------------------------------------
def test_the_draws_equal_reading_noise_and_depend_on_seed_member_row_and_sensor_alone(pkg, lib):
    """64 rows x 16 members x 16 sensors.  Bound against the fp64 restatement: 1e-5 absolute (|z| <= 5.8, sqrtf correctly
    rounded, logf and cosf good to a few ulp, the fp32 rounding of the cosine's argument <= 1.4e-6: about 2.5e-6 in the worst
    case; an fp32 numpy evaluation of the same formula deviates by 1.44e-6; measured on an MI355X: 1.195e-6).  Beyond it the
    kernel computes another formula."""
    rows, members, n = 64, 16, N37
    observed = [36, 0, 5, 1, 2, 3, 4, 35, 34, 20, 19, 18, 7, 8, 30, 12]
    K = len(observed)
    src = torch.zeros((rows, n), dtype=torch.float32, device=DEV)
    ones = [1.0] * K
    Z = torch.empty((rows * members, K), dtype=torch.float32, device=DEV)
    hidden = [v for v in range(n) if v not in observed]
    for first, g in ((0, 300), (300, 1), (301, 723)):               # the 1 024 pairs in three launches
        x, mask = stage_noisy(pkg, lib, src, 0, first, members, 0, n, g, observed, ones, SEED)
        x, mask = x.view(g, n), mask.view(g, n)
        assert (x[:, hidden] == 0).all() and (mask[:, hidden] == 1).all() and (mask[:, observed] == 0).all()
        Z[first:first + g] = x[:, observed]
    Z = Z.view(rows, members, K)
    want = pkg.estimation.reading_noise(SEED, members, rows, K)
    err = float(np.abs(Z.double().cpu().numpy() - want).max())
    print(f"device draws vs reading_noise (fp64): max |dz| = {err:.3e} over {Z.numel()} draws, max |z| = {float(Z.abs().max()):.3f}")
    assert err <= 1e-5
    # the same (seed, member, row, k) from other launches, positions, member splits and layouts: the same bits
    assert torch.equal(device_z(pkg, lib, SEED, members, rows, observed, n), Z)
    x, _ = stage_noisy(pkg, lib, src, 0, 10, 1, 5, n, 20, observed, ones, SEED)                 # rows 10 .. 29 as member 5 alone
    assert torch.equal(x.view(20, n)[:, observed], Z[10:30, 5])
    x, _ = stage_noisy(pkg, lib, src, 0, 7, 4, 8, n, 50, observed, ones, SEED)                  # members 8 .. 11, pairs 7 .. 56
    got = x.view(50, n)[:, observed]
    for i, p in enumerate(range(7, 57)):
        assert torch.equal(got[i], Z[p // 4, 8 + p % 4]), p
    readings = torch.zeros((rows, K), dtype=torch.float32, device=DEV)                             # the readings layout
    x, _ = stage_noisy(pkg, lib, readings, 1, 33, members, 0, n, 40, observed, ones, SEED)
    assert torch.equal(x.view(40, n)[:, observed], Z.view(-1, K)[33:73])
    # another seed or another member: other values
    other = device_z(pkg, lib, SEED + 1, members, rows, observed, n)
    assert float((other == Z).float().mean()) < 1e-3
    shifted = device_z(pkg, lib, SEED, members, rows, observed, n, member0=1)
    assert torch.equal(shifted[:, :-1], Z[:, 1:]) and float((shifted == Z).float().mean()) < 1e-3


# ---- 2. staging -------------------------------------------------------------------------------------------------------------------
def staging_case(pkg, oracle, n, normalize):
    observed, pipes = (OBS, 41) if n == N37 else (OBS40, 45)
    raw = raw_snapshots(pkg, S5, n)
    store = pkg.SnapshotStore(raw, topology(pkg, n, pipes), device=DEV, normalize=normalize)
    model, _ = small_model(pkg, oracle)
    est = pkg.PressureEstimator.for_store(model, store, observed, batch_size=BS4)
    readings = raw.to(DEV)[:, observed].contiguous()
    norm = (est._normalise, store.mean if normalize else 0.0, store.std + 1e-8 if normalize else 1.0)

    def normalise(t):                                               # torch's own, as SnapshotStore forms it
        return (t - store.mean) / (store.std + 1e-8) if normalize else t

    return observed, store, readings, norm, normalise


@pytest.mark.parametrize("n", [N37, 40], ids=["n37", "n40"])
@pytest.mark.parametrize("normalize", [True, False], ids=["znorm", "unused"])
def test_noisy_staging_bitwise_in_both_layouts(pkg, lib, oracle, n, normalize):
    observed, store, readings, norm, normalise = staging_case(pkg, oracle, n, normalize)
    K = len(observed)
    sigma = SIGMA[K]
    Z = device_z(pkg, lib, SEED, M3, S5, observed, n)
    noisy_readings = normalise(pair_values(readings, sigma, Z))                     # physical units, then normalised
    noisy_rows = pair_values(store.data[:, observed], sigma, Z)                     # the store's entries: sigma in their units
    batches = [(first, min(BS4, S5 * M3 - first)) for first in range(0, S5 * M3, BS4)]
    assert [g for _, g in batches] == [4, 4, 4, 3]
    for first, g in batches:
        x, mask = stage_noisy(pkg, lib, readings, 1, first, M3, 0, n, g, observed, sigma, SEED, None, 0, *norm)
        ex, em = torch_stage(noisy_readings[first:first + g], n, observed)
        assert torch.equal(x, ex) and torch.equal(mask, em), first
        x, mask = stage_noisy(pkg, lib, store.data, 0, first, M3, 0, n, g, observed, sigma, SEED)
        ex, em = torch_stage(noisy_rows[first:first + g], n, observed)
        assert torch.equal(x, ex) and torch.equal(mask, em), first
    assert not torch.equal(noisy_rows, pair_values(store.data[:, observed], [0.0] * K, Z))      # (the noise is there)
    col = SIGMA[K].index(0.0)                                                       # ... but not at the exact sensor
    assert torch.equal(noisy_rows.view(S5, M3, K)[:, :, col], store.data[:, observed][:, col:col + 1].expand(S5, M3))
    # sigma = 0 is gatres_stage_observed, bit for bit, in both layouts
    for src, layout, nm in ((readings, 1, norm), (store.data, 0, (0, 0.0, 1.0))):
        x, mask = stage_noisy(pkg, lib, src, layout, 1, 1, 9, n, 3, observed, [0.0] * K, SEED, None, 0, *nm)
        ox, om = stage(pkg, lib, src, layout, None, 1, n, 3, observed, *nm)
        assert torch.equal(x, ox) and torch.equal(mask, om)


def test_noisy_staging_on_an_unaligned_target(pkg, lib):
    """A target one float past a 16-byte boundary takes the element-by-element stores; nothing is written outside the batch."""
    g = 3
    store = make_store(pkg, S5)
    sigma = SIGMA[3]
    Z = device_z(pkg, lib, SEED, M3, S5, OBS, N37)
    xb, mb = garbage(g * N37 + 4)
    stage_noisy(pkg, lib, store.data, 0, 5, M3, 0, N37, g, OBS, sigma, SEED, target=(xb.data_ptr() + 4, mb.data_ptr() + 1))
    ex, em = torch_stage(pair_values(store.data[:, OBS], sigma, Z)[5:5 + g], N37, OBS)
    assert torch.equal(xb[1:1 + g * N37], ex) and torch.equal(mb[1:1 + g * N37], em)
    assert torch.isnan(xb[0]) and torch.isnan(xb[1 + g * N37:]).all() and int(mb[0]) == 0xAB and (mb[1 + g * N37:] == 0xAB).all()


@pytest.mark.parametrize("normalize", [True, False], ids=["znorm", "unused"])
def test_noisy_staging_with_missing_readings(pkg, lib, oracle, normalize):
    """A missing reading (by ``available`` or as a NaN) is staged as gatres_stage_observed_available stages it; the present ones
    keep the draws they had with everything available."""
    observed, store, readings, norm, normalise = staging_case(pkg, oracle, N37, normalize)
    sigma = SIGMA[3]
    Z = device_z(pkg, lib, SEED, M3, S5, observed, N37)                             # (drawn with every reading present)
    av = avail(AVAIL5)
    av_pairs = av.repeat_interleave(M3, dim=0)
    noisy_readings = normalise(pair_values(readings, sigma, Z))
    noisy_rows = pair_values(store.data[:, observed], sigma, Z)
    holes = ~av.bool()
    nan_readings = torch.where(holes, torch.full_like(readings, float("nan")), readings)
    for first, g in ((0, 4), (4, 4), (8, 4), (12, 3)):
        sl = slice(first, first + g)
        ex, em = torch_stage_available(noisy_rows[sl], N37, observed, av_pairs[sl])
        x, mask = stage_noisy(pkg, lib, store.data, 0, first, M3, 0, N37, g, observed, sigma, SEED, av)
        assert torch.equal(x, ex) and torch.equal(mask, em), first
        ex, em = torch_stage_available(noisy_readings[sl], N37, observed, av_pairs[sl])
        x, mask = stage_noisy(pkg, lib, readings, 1, first, M3, 0, N37, g, observed, sigma, SEED, av, 0, *norm)
        assert torch.equal(x, ex) and torch.equal(mask, em), first
        x, mask = stage_noisy(pkg, lib, nan_readings, 1, first, M3, 0, N37, g, observed, sigma, SEED, None, 1, *norm)
        assert torch.equal(x, ex) and torch.equal(mask, em) and torch.isfinite(x).all(), first
        x, mask = stage_noisy(pkg, lib, nan_readings, 1, first, M3, 0, N37, g, observed, sigma, SEED, av, 1, *norm)
        assert torch.equal(x, ex) and torch.equal(mask, em), first


def test_noisy_staging_across_the_tile_boundary(pkg, lib):
    """One graph of 1 030 nodes: the staging kernel's second workgroup column starts at node 1 020 + shift."""
    n, observed = 1030, [1019, 1020, 1023, 1024, 1029]
    sigma = SIGMA[5]
    src = torch.randn((2, n), generator=torch.Generator().manual_seed(5)).to(DEV)
    Z = device_z(pkg, lib, SEED, M3, 2, observed, n)
    noisy = pair_values(src[:, observed], sigma, Z)
    for first, g in ((4, 1), (0, 1), (0, 6), (1, 5)):
        x, mask = stage_noisy(pkg, lib, src, 0, first, M3, 0, n, g, observed, sigma, SEED)
        ex, em = torch_stage(noisy[first:first + g], n, observed)
        assert torch.equal(x, ex) and torch.equal(mask, em), (first, g)
    assert not torch.equal(noisy, src[:, observed].repeat_interleave(M3, 0))


# ---- 3. the reduce ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [37, 40], ids=["odd", "vector"])
@pytest.mark.parametrize("M", [1, 2, 3, 17])
def test_ensemble_reduce_bitwise(pkg, lib, M, n):
    C, stride, first, rows = 5, 40, 2, 9
    gen = torch.Generator().manual_seed(100 * M + n)
    mat = (50.0 + 0.1 * torch.randn((C * M, stride), generator=gen)).to(DEV)
    const = 50.0 + torch.arange(C, dtype=torch.float32, device=DEV) * 0.37          # column 7: the same value in every member
    mat.view(C, M, stride)[:, :, 7] = const.unsqueeze(1)
    mean = torch.full((rows, stride), -777.25, dtype=torch.float32, device=DEV)
    sd = torch.full((rows, stride), -777.25, dtype=torch.float32, device=DEV)
    pkg._native.check(lib.gatres_ensemble_reduce(mat.data_ptr(), C, M, n, stride, mean.data_ptr(), sd.data_ptr(), rows, stride,
                                                 first, stream()), "gatres_ensemble_reduce")
    want_mean, want_sd = numpy_reduce(mat.view(C, M, stride)[:, :, :n].cpu().numpy())
    got_mean, got_sd = mean[first:first + C, :n].cpu().numpy(), sd[first:first + C, :n].cpu().numpy()
    assert got_mean.tobytes() == want_mean.tobytes()
    assert got_sd.tobytes() == want_sd.tobytes()
    assert (got_sd[:, 7] == 0).all() and got_mean[:, 7].tobytes() == const.cpu().numpy().tobytes()
    if M == 1:
        assert (got_sd == 0).all() and torch.equal(mean[first:first + C, :n], mat[:, :n])
    else:
        assert (np.delete(got_sd, 7, axis=1) > 0).all()
    for t in (mean, sd):                                           # the other rows and the columns past n stay untouched
        t[first:first + C, :n] = -777.25
        assert (t == -777.25).all()


# ---- 4. spread moments --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [5, 130], ids=["S5", "more_than_two_chunks"])
def test_node_spread_moments(pkg, lib, S):
    assert pkg._native.NODE_ERROR_CHUNK == 64
    sd = (torch.rand((S, N37), generator=torch.Generator().manual_seed(S)) * 0.8).to(DEV)
    sd[S // 2, 4] = 3.5
    sd[:, 9] = 0.0

    def table():
        t = torch.full((N37, pkg._native.NODE_SPREAD_RECORD), float("nan"), dtype=torch.float64, device=DEV)
        pkg._native.check(lib.gatres_node_spread_moments(sd.data_ptr(), S, N37, t.data_ptr(), stream()), "gatres_node_spread_moments")
        return t.cpu().numpy()

    T = table()
    assert T.tobytes() == table().tobytes()                        # the same bits every run
    x = sd.double().cpu().numpy()
    assert (T[:, 0] == S).all()
    np.testing.assert_allclose(T[:, 1], (x * x).sum(0), rtol=1e-12, atol=0)
    np.testing.assert_array_equal(T[:, 2], x.max(0))
    np.testing.assert_allclose(T[:, 3], x.sum(0), rtol=1e-12, atol=0)
    assert T[4, 2] == 3.5 and T[9].tolist() == [S, 0.0, 0.0, 0.0]


# ---- 5. one realisation -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", [True, False], ids=["znorm", "unused"])
def test_one_noisy_realisation_equals_the_pass_on_perturbed_readings(pkg, lib, oracle, normalize):
    S, member = 7, 2
    raw = raw_snapshots(pkg, S)
    store = pkg.SnapshotStore(raw, topology(pkg), device=DEV, normalize=normalize)
    model, _ = small_model(pkg, oracle)
    est = pkg.PressureEstimator.for_store(model, store, OBS, batch_size=3)
    readings = raw.to(DEV)[:, OBS].contiguous()
    sigma = SIGMA[3]
    z = device_z(pkg, lib, SEED, 1, S, OBS, N37, member0=member)[:, 0]              # [S, K]
    sig32 = torch.tensor(sigma, dtype=torch.float32, device=DEV)
    got = est.estimate(readings, noise_std=sigma, noise_seed=SEED, noise_member=member)
    plain = est.estimate(readings)
    assert torch.equal(got, est.estimate((readings + sig32 * z).contiguous())) and not torch.equal(got, plain)
    # with keep_observed the sensor nodes carry the noisy reading (the exact sensor: its own)
    assert torch.equal(got[:, OBS[1]], plain[:, OBS[1]]) and not torch.equal(got[:, OBS[0]], plain[:, OBS[0]])
    # a scalar noise_std is every sensor's
    assert torch.equal(est.estimate(readings, noise_std=0.25, noise_seed=SEED, noise_member=member),
                       est.estimate((readings + torch.tensor(0.25, device=DEV) * z).contiguous()))
    # the store form: the store's sensor columns perturbed in ITS units
    scale = store.std + 1e-8 if normalize else 1.0
    sig_n = torch.tensor(np.asarray(sigma, dtype=np.float64) / scale, dtype=torch.float32, device=DEV)
    perturbed = copy.copy(store)
    perturbed.data = store.data.clone()
    perturbed.data[:, OBS] = store.data[:, OBS] + sig_n * z
    got = est.estimate_store(store, noise_std=sigma, noise_seed=SEED, noise_member=member)
    assert torch.equal(got, est.estimate_store(perturbed)) and not torch.equal(got, est.estimate_store(store))
    # with gaps: the missing readings draw nothing, the others keep their draws
    av = avail([[1, 1, 1], [0, 0, 0], [1, 0, 1], [0, 1, 1], [0, 0, 1], [1, 1, 0], [0, 1, 0]])
    assert torch.equal(est.estimate_store(store, available=av, noise_std=sigma, noise_seed=SEED, noise_member=member),
                       est.estimate_store(perturbed, available=av))
    # noise_std=None: today's launches, today's bits
    want, _ = hand_loop(pkg, model, store, OBS, 3)
    assert torch.equal(est.estimate_store(store, noise_std=None, noise_seed=5, noise_member=1), want)
    assert torch.equal(est.estimate(readings, noise_std=None), plain)


# ---- 6. the ensemble ----------------------------------------------------------------------------------------------------------------
def ensemble_hand_loop(pkg, model, store, observed, bs, noisy, keep_observed=True):
    """The ensemble's pass written out (``hand_loop`` of test_gpu_estimation.py over the pairs): ``noisy`` [S * M, K] are the
    pairs' staged sensor values; torch staging, the forward through the estimator's plan and entry at the batch's size,
    ``store.descale``.  Returns the members' estimates [S * M, N]."""
    E = pkg.evaluation
    lib = pkg._native.load()
    n, pairs = store.nodes_per_graph, noisy.shape[0]
    res = torch.empty((pairs, n), dtype=torch.float32, device=DEV)
    sizes = []
    for first in range(0, pairs, bs):
        g = min(bs, pairs - first)
        P = E._eval_plan(model, store, g)
        x1, mask = torch_stage(noisy[first:first + g], n, observed)
        P.x.copy_(x1)
        P.mask.copy_(mask)
        E._enqueue_forward(lib, model.flat_parameters, P, stream())
        pred = P.out.clone().reshape(-1)
        merged = torch.where(mask.bool(), store.descale(pred), store.descale(x1)) if keep_observed else store.descale(pred)
        res[first:first + g] = merged.view(g, n)
        sizes.append(g)
    return res, sizes


def store_sigma(store, sigma):
    """What estimate_store uploads: float32(noise_std / (std + eps)) for a z-normalised store, float32(noise_std) otherwise."""
    scale = store.std + 1e-8 if store.norm_type == "znorm" else 1.0
    return torch.tensor(np.asarray(sigma, dtype=np.float64) / scale, dtype=torch.float32)


@pytest.mark.parametrize("kind", ["fused", "per_op", "bf16"])
def test_ensemble_equals_its_pass_written_out(pkg, lib, oracle, kind):
    store = make_store(pkg, S5)
    model, _ = small_model(pkg, oracle, fused=kind != "per_op") if kind != "bf16" else small_model(pkg, oracle, nb=2, nc=32, dtype="bf16")
    est = pkg.PressureEstimator.for_store(model, store, OBS, batch_size=BS4)
    sigma = SIGMA[3]
    Z = device_z(pkg, lib, SEED, M3, S5, OBS, N37)
    members, sizes = ensemble_hand_loop(pkg, model, store, OBS, BS4, pair_values(store.data[:, OBS], store_sigma(store, sigma), Z))
    assert sizes == [4, 4, 4, 3]
    want_mean, want_sd = numpy_reduce(members.view(S5, M3, N37).cpu().numpy())
    mean, sd = est.estimate_store_ensemble(store, sigma, M3, seed=SEED)
    assert mean.shape == sd.shape == (S5, N37) and mean.dtype == sd.dtype == torch.float32
    assert mean.cpu().numpy().tobytes() == want_mean.tobytes() and sd.cpu().numpy().tobytes() == want_sd.tobytes()
    assert float(sd[:, OBS[0]].min()) > 0 and torch.isfinite(mean).all()
    # the budget changes the chunks (one unit of 4 snapshots, then 1; everything), not the batches: the same bits
    assert pkg.estimation.ensemble_chunk(S5, M3, BS4, 4 * N37, 1) == 4
    m1, s1 = est.estimate_store_ensemble(store, sigma, M3, seed=SEED, max_scratch_bytes=1)
    assert torch.equal(m1, mean) and torch.equal(s1, sd)
    # mean_out / std_out
    mo, so = torch.full_like(mean, float("nan")), torch.full_like(mean, float("nan"))
    a, b = est.estimate_store_ensemble(store, sigma, M3, seed=SEED, mean_out=mo, std_out=so)
    assert a is mo and b is so and torch.equal(mo, mean) and torch.equal(so, sd)
    for bad in (torch.empty((S5, N37 + 1), device=DEV), torch.empty((S5, N37), device=DEV).double(), torch.empty((S5, N37))):
        with pytest.raises(ValueError, match="out must"):
            est.estimate_store_ensemble(store, sigma, M3, mean_out=bad)
        with pytest.raises(ValueError, match="out must"):
            est.estimate_store_ensemble(store, sigma, M3, std_out=bad)
    with pytest.raises(ValueError, match="different"):
        est.estimate_store_ensemble(store, sigma, M3, mean_out=mo, std_out=mo)
    # another seed: another ensemble
    assert not torch.equal(est.estimate_store_ensemble(store, sigma, M3, seed=SEED + 1)[0], mean)
    if kind == "bf16":
        return
    # each member against the single realisation of the same (seed, member): another batch composition, so within the bound
    # fp32 passes are held to, not to the bit
    for m in range(M3):
        one = est.estimate_store(store, noise_std=sigma, noise_seed=SEED, noise_member=m)
        e = relerr(members.view(S5, M3, N37)[:, m], one)
        print(f"member {m} vs its single realisation: relerr {e:.2e}")
        assert e < 1e-5


def test_ensemble_on_raw_readings_equals_the_store_form(pkg, lib, oracle):
    """Bit for bit where both forms stage the same arithmetic, that is for a store that is not normalised (r + float32(sigma) z
    either way).  For a z-normalised store the readings form rounds normalise(r + sigma z), the store form
    normalise(r) + (sigma / (std + eps)) z: inputs a few fp32 ulp apart, so the estimates agree as two fp32 passes do (max-norm
    relative error < 1e-5, test_gpu_estimation.check_against_module's bound) and the standard deviations, which are 1-Lipschitz
    in the members up to sqrt(M / (M - 1)), within that factor times the same absolute error."""
    sigma = SIGMA[3]
    model, _ = small_model(pkg, oracle)
    raw = raw_snapshots(pkg, S5)
    readings = raw.to(DEV)[:, OBS].contiguous()
    for normalize in (False, True):
        store = pkg.SnapshotStore(raw, topology(pkg), device=DEV, normalize=normalize)
        est = pkg.PressureEstimator.for_store(model, store, OBS, batch_size=BS4)
        mean, sd = est.estimate_store_ensemble(store, sigma, M3, seed=SEED)
        rmean, rsd = est.estimate_ensemble(readings, sigma, M3, seed=SEED)
        if not normalize:
            assert torch.equal(rmean, mean) and torch.equal(rsd, sd)
        else:
            e = relerr(rmean, mean)
            d = float((rsd - sd).abs().max())
            print(f"znorm, readings form vs store form: mean relerr {e:.2e}, max |d std| {d:.2e}")
            assert e < 1e-5 and d < np.sqrt(M3 / (M3 - 1)) * 1e-5 * float(mean.abs().max())
        # gaps told by NaN readings and by available: the same ensemble
        av = avail(AVAIL5)
        nan_readings = torch.where(av.bool(), readings, torch.full_like(readings, float("nan")))
        a = est.estimate_ensemble(readings, sigma, M3, seed=SEED, available=av)
        b = est.estimate_ensemble(nan_readings, sigma, M3, seed=SEED, nan_is_missing=True)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and not torch.equal(a[0], rmean)
        assert (a[1][1] == 0).all()                                 # the snapshot without any reading: every member the same


def test_ensemble_in_three_chunks_equals_the_ensemble_in_one(pkg, oracle):
    """S = 5 snapshots of M = 6 members at batch size 4: the 30 pairs fall as seven batches of 4 and a ragged 2, a snapshot's
    members straddle batches, and a chunk is a multiple of lcm(4, 6) / 6 = 2 snapshots -- the smallest budget gives the chunks
    2, 2 and 1, the last one short.  The bits are those of the pass in one chunk, in both forms."""
    M6 = 6
    store = make_store(pkg, S5)
    model, _ = small_model(pkg, oracle)
    est = pkg.PressureEstimator.for_store(model, store, OBS, batch_size=BS4)
    readings = raw_snapshots(pkg, S5).to(DEV)[:, OBS].contiguous()
    assert pkg.estimation.ensemble_chunk(S5, M6, BS4, 4 * N37, 1) == 2
    assert pkg.estimation.ensemble_chunk(S5, M6, BS4, 4 * N37, 1 << 40) == S5
    av = avail(AVAIL5)
    for run in (lambda budget: est.estimate_store_ensemble(store, SIGMA[3], M6, seed=SEED, max_scratch_bytes=budget),
                lambda budget: est.estimate_ensemble(readings, SIGMA[3], M6, seed=SEED, available=av, max_scratch_bytes=budget)):
        mean, sd = run(1 << 40)
        m3, s3 = run(1)
        assert torch.equal(m3, mean) and torch.equal(s3, sd)
        assert torch.isfinite(mean).all() and float(sd.max()) > 0


def test_without_noise_the_ensemble_is_the_plain_pass(pkg, oracle):
    store = make_store(pkg, S5)
    model, _ = small_model(pkg, oracle)
    est = pkg.PressureEstimator.for_store(model, store, OBS, batch_size=BS4)
    for zero in (0.0, [0.0, 0.0, 0.0]):
        mean, sd = est.estimate_store_ensemble(store, zero, M3, seed=SEED)
        assert (sd == 0).all()
        assert torch.equal(mean, est.estimate_store(store))


# ---- 7. gatres_small ----------------------------------------------------------------------------------------------------------------
def test_gatres_small_at_batch_32_takes_the_window_kernel(pkg, lib, oracle):
    n, pipes, S, M = 388, 430, 4, 16
    store = make_store(pkg, S, n=n, pipes=pipes, seed=4)
    model, _ = small_model(pkg, oracle, nb=15, nc=32, seed=11)
    plan = model.plan_for(store.edge_index(32), 32 * n)
    assert model._call_state(plan)["window"], "gatres_small at bs 32 should take the window kernel"
    sensors = [3, 17, 100, 101, 250, 387, 42, 9, 300, 77, 211, 5, 64, 128, 199, 350, 1, 260, 333, 150]
    est = pkg.PressureEstimator.for_store(model, store, sensors, batch_size=32)
    Z = device_z(pkg, lib, SEED, M, S, sensors, n)
    noisy = pair_values(store.data[:, sensors], store_sigma(store, 0.5).expand(len(sensors)), Z)
    members, sizes = ensemble_hand_loop(pkg, model, store, sensors, 32, noisy)
    assert sizes == [32, 32]
    want_mean, want_sd = numpy_reduce(members.view(S, M, n).cpu().numpy())
    mean, sd = est.estimate_store_ensemble(store, 0.5, M, seed=SEED)
    assert mean.cpu().numpy().tobytes() == want_mean.tobytes() and sd.cpu().numpy().tobytes() == want_sd.tobytes()
    assert float(sd.max()) > 0


# ---- 8. the report ------------------------------------------------------------------------------------------------------------------
def test_noise_report_equals_its_passes_and_formulas(pkg, lib, oracle):
    """With ``keep_observed`` a sensor node carries D(v + s z) = fl(fl(fl(v + fl(s z)) * std) + mean) with s = float32(sigma /
    (std + eps)), so its standard deviation over the members is sigma * sd(z) up to the roundings of that round trip.  For
    |v + s z| < 4, std < 16 and pressures below 128 (asserted): fl(s z) <= 3e-8 (4e-7 after the scaling by std), the sum half an
    ulp of 4 (2.4e-7, 3.0e-6 after the scaling), the product and the final sum half an ulp of 128 each (3.8e-6): 1.1e-5 per
    member, times sqrt(M / (M - 1)) = 1.07 for the standard deviation of M = 8 members, plus the relative 1.2e-7 of s and of the
    result's own rounding: the bound is 1.5e-5 absolute, 3e-5 of the spread itself at sigma = 0.5."""
    S, M, sigma = 7, 8, [0.5, 0.0, 0.25]
    store = make_store(pkg, S)
    model, _ = small_model(pkg, oracle)
    est = pkg.PressureEstimator.for_store(model, store, OBS, batch_size=BS4)
    rep = est.noise_report(store, sigma, M, seed=SEED)
    mean, sd = est.estimate_store_ensemble(store, sigma, M, seed=SEED)
    error = est.error_map(store, estimates=mean)
    assert sorted(rep) == sorted(["error", "spread", "max_std", "mean_std", "nonsensor_spread", "most_sensitive"])
    assert sorted(rep["error"]) == sorted(error)
    for key, v in error.items():
        np.testing.assert_array_equal(rep["error"][key], v, err_msg=key)
    x = sd.double().cpu().numpy()
    np.testing.assert_allclose(rep["spread"], np.sqrt((x * x).sum(0) / S), rtol=1e-12)
    np.testing.assert_array_equal(rep["max_std"], x.max(0))
    np.testing.assert_allclose(rep["mean_std"], x.mean(0), rtol=1e-12)
    outside = [v for v in range(N37) if v not in OBS]
    assert rep["nonsensor_spread"] == pytest.approx(np.sqrt((x[:, outside] ** 2).mean()), rel=1e-12)
    assert rep["most_sensitive"].tolist() == np.argsort(-rep["spread"], kind="stable").tolist()
    assert sorted(rep["most_sensitive"].tolist()) == list(range(N37))
    # the exact sensor is among the nodes without any spread, which come last (a node the noisy sensors do not reach is another)
    still = rep["most_sensitive"][rep["spread"][rep["most_sensitive"]] == 0].tolist()
    assert OBS[1] in still and still == rep["most_sensitive"][-len(still):].tolist() and OBS[0] not in still
    # the sensors' own spread
    assert float(store.data[:, OBS].abs().max()) + 0.5 / store.std * 5.8 < 4 and store.std < 16
    assert float(store.descale(store.data[:, OBS]).abs().max()) + 0.5 * 5.8 < 128
    z = pkg.estimation.reading_noise(SEED, M, S, 3)                                  # [S, M, K]
    want = np.asarray(sigma) * np.sqrt((z.std(axis=1, ddof=1) ** 2).mean(axis=0))
    got = rep["spread"][OBS]
    print("sensor spread: got", got, "sigma * sd(z)", want, "max |d|", np.abs(got - want).max())
    np.testing.assert_allclose(got, want, rtol=0, atol=1.5e-5)
    assert got[1] == 0.0 and rep["nonsensor_spread"] > 0
    # with gaps the error is over the hidden entries, as error_map(available=...)
    av = avail([[1, 1, 1], [0, 0, 0], [1, 0, 1], [0, 1, 1], [0, 0, 1], [1, 1, 0], [0, 1, 0]])
    rep = est.noise_report(store, sigma, M, seed=SEED, available=av)
    mean, sd = est.estimate_store_ensemble(store, sigma, M, seed=SEED, available=av)
    error = est.error_map(store, estimates=mean, available=av)
    for key, v in error.items():
        np.testing.assert_array_equal(rep["error"][key], v, err_msg=key)
    np.testing.assert_array_equal(rep["max_std"], sd.double().cpu().numpy().max(0))


# ---- 9. synchronisation -------------------------------------------------------------------------------------------------------------
def test_no_read_back_in_the_ensemble_passes_and_two_in_noise_report(pkg, oracle, monkeypatch):
    store = make_store(pkg, S5)
    model, _ = small_model(pkg, oracle)
    est = pkg.PressureEstimator.for_store(model, store, OBS, batch_size=BS4)
    readings = raw_snapshots(pkg, S5).to(DEV)[:, OBS].contiguous()
    sigma = SIGMA[3]
    est.estimate_store_ensemble(store, sigma, M3)                   # plans (4 and 3 graphs; 1 for the plain pass) and buffers
    est.estimate_store(store)                                       # exist from here on
    torch.cuda.synchronize()
    calls = {"synchronize": 0, "item": 0, "cpu": 0, "tolist": 0, "float": 0, "stream_sync": 0, "event_sync": 0}

    def spy(name, fn):
        def wrapped(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return wrapped

    monkeypatch.setattr(torch.cuda, "synchronize", spy("synchronize", torch.cuda.synchronize))
    monkeypatch.setattr(torch.Tensor, "item", spy("item", torch.Tensor.item))
    monkeypatch.setattr(torch.Tensor, "cpu", spy("cpu", torch.Tensor.cpu))
    monkeypatch.setattr(torch.Tensor, "tolist", spy("tolist", torch.Tensor.tolist))
    monkeypatch.setattr(torch.Tensor, "__float__", spy("float", torch.Tensor.__float__))
    monkeypatch.setattr(torch.cuda.Stream, "synchronize", spy("stream_sync", torch.cuda.Stream.synchronize))
    monkeypatch.setattr(torch.cuda.Event, "synchronize", spy("event_sync", torch.cuda.Event.synchronize))
    a = est.estimate_store_ensemble(store, sigma, M3, seed=SEED)
    b = est.estimate_store_ensemble(store, sigma, M3, seed=SEED, max_scratch_bytes=1)
    c = est.estimate_ensemble(readings, sigma, M3, seed=SEED)
    d = est.estimate_store(store, noise_std=sigma, noise_seed=SEED, noise_member=1)
    assert all(v == 0 for v in calls.values()), calls
    rep = est.noise_report(store, sigma, M3, seed=SEED)
    assert calls == {"synchronize": 0, "item": 0, "cpu": 2, "tolist": 0, "float": 0, "stream_sync": 0, "event_sync": 0}
    monkeypatch.undo()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.isfinite(c[0]).all() and torch.isfinite(d).all()
    assert np.isfinite(rep["nonsensor_spread"])
