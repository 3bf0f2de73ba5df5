"""Estimation under sensor noise, on the host: the three new symbols of k_estimate.hip are declared, exported and bound without
an ABI change and refuse their bad arguments before any launch; ``reading_noise`` restates the device generator (checked on
integers worked out in plain Python integers, and on its moments); the formulas of ``noise_report_from_moments`` and the chunk
rule of the ensemble hold on hand-computed cases.  No GPU, no kernel launches."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gatres_stage_observed_noisy", "gatres_ensemble_reduce", "gatres_node_spread_moments")
P = 4096                       # (any non-null address: a refused call never reads it)
Q = 8192
SEEDS = (0, 1, 20260, 2 ** 63 + 5)


def header():
    with open(os.path.join(ROOT, "include", "gatres.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


# ---- 1. symbols and refusals ----------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound_and_the_abi_stays(pkg, lib):
    hdr = header()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in pkg._native.SIGNATURES
    S = pkg._native.SIGNATURES
    # the arguments of gatres_stage_observed_available without rows, plus members, member0, sigma, seed
    assert len(S["gatres_stage_observed_noisy"][1]) == len(S["gatres_stage_observed_available"][1]) - 1 + 4
    assert "#define GATRES_ABI_VERSION 9" in hdr and pkg._native.ABI_VERSION == 9
    assert b"abi9" in lib.gatres_version()


def test_the_spread_record_macro_equals_the_python_constant(pkg):
    N = pkg._native
    assert re.search(r"#define GATRES_NODE_SPREAD_RECORD\s+%d\b" % N.NODE_SPREAD_RECORD, header())
    assert N.NODE_SPREAD_RECORD == 4 == pkg.estimation.NODE_SPREAD_RECORD


def stage(lib, src=P, layout=0, src_rows=8, first_pair=0, members=3, member0=0, n=37, graphs=3, observed=P, k=3, normalise=0,
          offset=0.0, factor=1.0, x=Q, mask=Q + 4096, available=3 * Q, nan_is_missing=0, sigma=5 * Q, seed=7):
    return lib.gatres_stage_observed_noisy(src, layout, src_rows, first_pair, members, member0, n, graphs, observed, k, normalise,
                                           offset, factor, x, mask, available, nan_is_missing, sigma, seed, None)


def test_stage_observed_noisy_checks_its_arguments_before_any_launch(lib):
    # the pair range: 8 rows x 3 members = 24 pairs
    assert stage(lib, first_pair=-1) == -1
    assert stage(lib, first_pair=22) == -1                     # pairs 22, 23, 24 of 24
    assert stage(lib, first_pair=8, members=1) == -1           # as a plain pass: row 8 of 8
    assert stage(lib, first_pair=6, members=1) == -1           # rows 6, 7, 8 of 8
    assert stage(lib, src_rows=0) == -1
    assert stage(lib, src_rows=2 ** 62, members=4) == -1       # (src_rows * members does not fit)
    assert stage(lib, members=0) == -1
    assert stage(lib, members=-3) == -1
    assert stage(lib, member0=-1) == -1
    assert stage(lib, sigma=None) == -1
    assert stage(lib, sigma=Q) == -1                           # sigma is x_dst
    assert stage(lib, sigma=Q + 4 * 3 * 37 - 1) == -1          # the last byte of x_dst
    assert stage(lib, sigma=Q + 4096 + 3 * 37 - 1) == -1       # the last byte of mask
    # those of gatres_stage_observed_available
    assert stage(lib, k=0) == -1
    assert stage(lib, k=38) == -1
    assert stage(lib, graphs=0) == -1
    assert stage(lib, n=0) == -1
    for name in ("src", "observed", "x", "mask"):
        assert stage(lib, **{name: None}) == -1, name
    assert stage(lib, layout=2) == -1
    assert stage(lib, normalise=3) == -1
    assert stage(lib, layout=1, normalise=1, factor=0.0) == -1
    assert stage(lib, x=P) == -1                               # in place
    assert stage(lib, available=Q) == -1                       # available is x_dst
    assert stage(lib, available=Q + 4096 + 3 * 37 - 1) == -1   # the last byte of mask
    assert stage(lib, available=None, nan_is_missing=0, k=0) == -1      # (NULL is legal here: k is what is refused)


def reduce(lib, mem=P, S=5, M=3, n=37, stride=40, mean=64 * Q, std=128 * Q, out_rows=9, out_stride=40, first_row=2):
    return lib.gatres_ensemble_reduce(mem, S, M, n, stride, mean, std, out_rows, out_stride, first_row, None)


def test_ensemble_reduce_checks_its_arguments_before_any_launch(lib):
    assert reduce(lib, M=0) == -1
    assert reduce(lib, M=-1) == -1
    assert reduce(lib, S=0) == -1
    assert reduce(lib, n=0) == -1
    for name in ("mem", "mean", "std"):
        assert reduce(lib, **{name: None}) == -1, name
    assert reduce(lib, stride=36) == -1
    assert reduce(lib, out_stride=36) == -1
    assert reduce(lib, first_row=-1) == -1
    assert reduce(lib, first_row=5) == -1                      # rows 5 .. 9 of 9
    # overlaps.  The source is 5 * 3 rows of 40 floats = 2400 bytes from P; a destination is the 5 rows of 40 floats = 800 bytes
    # from row 2, that is from its base + 320
    assert reduce(lib, mean=P) == -1
    assert reduce(lib, std=P) == -1
    assert reduce(lib, mean=P + 2400 - 320 - 4) == -1          # its row 2 starts on the last float of the source
    assert reduce(lib, std=P - 320 - 800 + 4) == -1            # its row 6 ends on the first float of the source
    assert reduce(lib, mean=64 * Q, std=64 * Q) == -1          # mean is std
    assert reduce(lib, mean=64 * Q, std=64 * Q + 796) == -1    # the last float of mean's rows


def test_node_spread_moments_checks_its_arguments_before_any_launch(lib):
    assert lib.gatres_node_spread_moments(None, 5, 37, Q, None) == -1
    assert lib.gatres_node_spread_moments(P, 5, 37, None, None) == -1
    assert lib.gatres_node_spread_moments(P, 0, 37, Q, None) == -1
    assert lib.gatres_node_spread_moments(P, 5, 0, Q, None) == -1
    assert lib.gatres_node_spread_moments(P, 5, 37, P, None) == -1


# ---- 3. the generator -----------------------------------------------------------------------------------------------------------
M64 = (1 << 64) - 1


def mix64(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def integers(seed, member, row, k, K):
    """h, (h >> 40) + 1 and (h >> 8) & 0xFFFFFF of include/gatres.h in Python integers."""
    stream = mix64(seed + 0x9E3779B97F4A7C15 * (member + 1))
    h = mix64(stream + 0xBF58476D1CE4E5B9 * (row * K + k + 1))
    return h, (h >> 40) + 1, (h >> 8) & 0xFFFFFF


def test_reading_noise_on_hand_computed_integers(pkg):
    E = pkg.estimation
    # (seed, member, row, k, K) -> h, 2^24 u1, 2^24 u2, worked out once with the function above and written down
    cases = {(0, 0, 0, 0, 16): (0x377507B6BFBF0784, 3634440, 12566279),
             (20260, 5, 63, 15, 16): (0x30CEF854704FB8B5, 3198713, 7360440),
             (2 ** 63 + 5, 18, 7, 2, 3): (0x0982C8BC5E85FB70, 623305, 6194683)}
    for (seed, member, row, k, K), (h, a, b) in cases.items():
        assert integers(seed, member, row, k, K) == (h, a, b)
        bits = E._noise_bits(seed, member + 1, row + 1, K)
        assert bits.dtype == np.uint64 and bits.shape == (row + 1, member + 1, K)
        assert int(bits[row, member, k]) == h
        z = np.sqrt(-2.0 * np.log(a * 2.0 ** -24)) * np.cos(2.0 * np.pi * (b * 2.0 ** -24))
        got = E.reading_noise(seed, member + 1, row + 1, K)
        assert got.dtype == np.float64 and got.shape == (row + 1, member + 1, K)
        assert got[row, member, k] == z
        # with member0: the same draw as member 0 of a one-member call
        assert E.reading_noise(seed, 1, row + 1, K, member0=member)[row, 0, k] == z
    # u1 and u2 are exact in fp32
    assert np.float32(3634440 * 2.0 ** -24) == 3634440 * 2.0 ** -24 and np.float32(2.0 ** -24 * (2 ** 24 - 1)) == 1 - 2.0 ** -24


def test_reading_noise_layout_and_member_offset(pkg):
    E = pkg.estimation
    z = E.reading_noise(20260, 7, 5, 3)
    assert z.shape == (5, 7, 3)
    for j in (1, 4):
        np.testing.assert_array_equal(E.reading_noise(20260, 3, 5, 3, member0=j), z[:, j:j + 3])
    np.testing.assert_array_equal(E.reading_noise(20260, 7, 2, 3), z[:2])              # a row's draws do not depend on the rows
    assert not np.array_equal(E.reading_noise(20261, 7, 5, 3), z)
    assert len(np.unique(z)) == z.size                                                   # no member, row or sensor repeats another
    assert E.reading_noise(np.int64(5), 1, 1, 1)[0, 0, 0] == E.reading_noise(5, 1, 1, 1)[0, 0, 0]


@pytest.mark.parametrize("seed", SEEDS)
def test_reading_noise_moments(pkg, seed):
    """64 x 16 x 16 draws: mean, variance and the lag-1 correlations along the rows, the members and the sensors inside their
    5-sigma bounds (the standard errors of n independent standard normals: 1 / sqrt(n), sqrt(2 / n), 1 / sqrt(n'))."""
    z = pkg.estimation.reading_noise(seed, 16, 64, 16)
    n = z.size
    assert n == 16384
    print(f"seed {seed}: mean {z.mean():+.5f} var {z.var():.5f} max |z| {np.abs(z).max():.3f}")
    assert abs(z.mean()) <= 5 / np.sqrt(n)
    assert abs(z.var() - 1.0) <= 5 * np.sqrt(2.0 / n)
    assert np.abs(z).max() < 5.8
    c = z - z.mean()
    for axis, name in enumerate(("rows", "members", "sensors")):
        a, b = np.moveaxis(c, axis, 0)[:-1], np.moveaxis(c, axis, 0)[1:]
        r = float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))
        print(f"  lag-1 along {name}: {r:+.5f} (n' = {a.size})")
        assert abs(r) <= 5 / np.sqrt(a.size), name


# ---- 4. the report's formulas ---------------------------------------------------------------------------------------------------
def test_noise_report_formulas_on_a_hand_computed_table(pkg):
    """4 snapshots, 5 nodes, sensors at nodes 3 and 1.  Standard deviations per node over the snapshots:
        node 0: 1, 1, 1, 1      node 1: 0.5, 0.5, 0.5, 0.5      node 2: 3, 0, 4, 0      node 3: 0, 0, 0, 0      node 4: 2, 2, 2, 2"""
    sd = np.array([[1, 0.5, 3, 0, 2], [1, 0.5, 0, 0, 2], [1, 0.5, 4, 0, 2], [1, 0.5, 0, 0, 2]], dtype=np.float64)
    table = np.stack([np.full(5, 4.0), (sd * sd).sum(0), sd.max(0), sd.sum(0)], axis=1)
    assert table.shape == (5, pkg.estimation.NODE_SPREAD_RECORD)
    m = pkg.estimation.noise_report_from_moments(table, [3, 1])
    np.testing.assert_array_equal(m["spread"], [1.0, 0.5, 2.5, 0.0, 2.0])             # sqrt(25 / 4) = 2.5
    np.testing.assert_array_equal(m["max_std"], [1.0, 0.5, 4.0, 0.0, 2.0])
    np.testing.assert_array_equal(m["mean_std"], [1.0, 0.5, 1.75, 0.0, 2.0])
    assert m["nonsensor_spread"] == pytest.approx(np.sqrt((4 + 25 + 16) / 12), rel=1e-15)      # nodes 0, 2, 4: 12 entries
    assert m["most_sensitive"].tolist() == [2, 4, 0, 1, 3]
    for key in ("spread", "max_std", "mean_std"):
        assert m[key].dtype == np.float64 and m[key].shape == (5,)
    # ties keep the node order; every node a sensor: no pool
    tie = np.array([[4.0, 4.0, 1.0, 4.0]] * 3)
    m = pkg.estimation.noise_report_from_moments(tie, [0, 1, 2])
    assert m["most_sensitive"].tolist() == [0, 1, 2] and np.isnan(m["nonsensor_spread"])


# ---- 5. the chunk rule ------------------------------------------------------------------------------------------------------------
def test_ensemble_chunk_rule_on_hand_computed_cases(pkg):
    chunk = pkg.estimation.ensemble_chunk
    # S = 5, M = 3, bs = 4: lcm(4, 3) / 3 = 4 snapshots (12 pairs, 3 batches) per unit; 148 bytes per pair of 37 nodes
    unit_bytes = 4 * 3 * 148
    assert chunk(5, 3, 4, 148, 1) == 4                          # a budget below one unit: one unit
    assert chunk(5, 3, 4, 148, unit_bytes) == 4
    assert chunk(5, 3, 4, 148, 2 * unit_bytes - 1) == 4
    assert chunk(5, 3, 4, 148, 2 * unit_bytes) == 5             # two units hold the whole pass: C = S
    assert chunk(5, 3, 4, 148, 1 << 30) == 5
    assert chunk(3, 3, 4, 148, 1) == 3                          # one unit is more than the pass
    # M a multiple of bs: every snapshot is whole batches, the unit is one snapshot
    assert chunk(100, 32, 32, 1552, 3 * 32 * 1552) == 3
    assert chunk(100, 64, 32, 1552, 1) == 1
    # bs a multiple of M: bs / M snapshots per unit
    assert chunk(2048, 8, 32, 1552, 64 << 20) == 2048           # 2048 * 8 * 1552 bytes = 24.25 MiB fit
    assert chunk(2048, 8, 32, 1552, 1 << 20) == 84 // 4 * 4     # 84 snapshots fit, 21 units of 4
    # M = 1: the unit is a batch
    assert chunk(10, 1, 4, 148, 5 * 148) == 4
    for S, M, bs, budget in ((5, 3, 4, 1), (50, 6, 4, 5000), (50, 5, 32, 1 << 16), (7, 17, 3, 4000)):
        C = chunk(S, M, bs, 148, budget)
        assert 1 <= C <= S and (C == S or (C * M) % bs == 0), (S, M, bs, budget)


# ---- 6. refusals in Python ----------------------------------------------------------------------------------------------------------
def test_python_refusals_that_need_no_device(pkg):
    E = pkg.estimation
    for seed in (-1, 2 ** 64, 1.5, "7", None, True):
        with pytest.raises(ValueError, match="seed"):
            E.reading_noise(seed, 2, 2, 2)
    for bad in ((0, 2, 2), (2, 0, 2), (2, 2, 0)):
        with pytest.raises(ValueError, match="reading_noise"):
            E.reading_noise(1, *bad)
    with pytest.raises(ValueError, match="reading_noise"):
        E.reading_noise(1, 2, 2, 2, member0=-1)

    class Stub:                                                  # what _sigma, _noise and _run_ensemble read of an estimator
        observed_idx, norm_type, std, eps, device, batch_size, nodes_per_graph = [36, 0, 5], "znorm", 12.5, 1e-8, "cpu", 4, 37
        _sigma_cache = {}
        _sigma, _noise, _run_ensemble = (getattr(E.PressureEstimator, n) for n in ("_sigma", "_noise", "_run_ensemble"))

    est = Stub()
    for bad in (-0.1, float("nan"), float("inf"), [0.1, 0.2], [0.1, 0.2, 0.3, 0.4], [0.1, -0.2, 0.3], [[0.1, 0.2, 0.3]], "x",
                [0.1, float("nan"), 0.3]):
        with pytest.raises(ValueError, match="noise_std"):
            est._sigma(bad, pkg._native.OBSERVED_READINGS)
        with pytest.raises(ValueError, match="noise_std"):
            est._noise(bad, 0, 0, pkg._native.OBSERVED_READINGS)
    with pytest.raises(ValueError, match="seed"):
        est._noise(0.1, -1, 0, pkg._native.OBSERVED_READINGS)
    with pytest.raises(ValueError, match="seed"):
        est._noise(0.1, 2 ** 64, 0, pkg._native.OBSERVED_READINGS)
    for bad in (-1, 0.5, None):
        with pytest.raises(ValueError, match="noise_member"):
            est._noise(0.1, 0, bad, pkg._native.OBSERVED_READINGS)
    assert est._noise(None, -1, -1, pkg._native.OBSERVED_READINGS) is None          # no noise: nothing else is looked at
    # the uploaded sigma: physical for readings, divided by std + eps for the full rows of a z-normalised store
    sigma, seed, members, member0 = est._noise([0.25, 0.0, 1.0], 2 ** 64 - 1, 3, pkg._native.OBSERVED_READINGS)
    assert sigma.dtype.is_floating_point and sigma.tolist() == [0.25, 0.0, 1.0] and (seed, members, member0) == (2 ** 64 - 1, 1, 3)
    got = est._sigma(0.25, pkg._native.OBSERVED_FULL_ROWS).numpy()
    assert got.dtype == np.float32 and got.tolist() == [float(np.float32(0.25 / (12.5 + 1e-8)))] * 3
    src = np.zeros((5, 37), dtype=np.float32)
    for bad in (0, -2, 1.5, None, True):
        with pytest.raises(ValueError, match="members"):
            est._run_ensemble(src, 0, 0, 0.1, bad, 0, None, False, None, None, 1 << 20)
    with pytest.raises(ValueError, match="max_scratch_bytes"):
        est._run_ensemble(src, 0, 0, 0.1, 3, 0, None, False, None, None, 0)
