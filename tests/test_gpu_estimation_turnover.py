"""The kernels of k_estimate.hip where their loops, tiles and capped grids turn over: every case calls an ``extern "C"`` entry
point directly, at a shape of tests/turnover_cases.py that lies just past such a point (a second trip of a loop, a second tile
column or workgroup, a grid at its cap), and compares the result with a numpy statement of the kernel formed on the host
(tests/estimation_refs.py) -- bit for bit where the kernel fixes every rounding, within the reordering bound 2 * terms * 2^-53 of
fp64 sums of exact terms otherwise.  Targets are filled with garbage and compared as a whole: what a launch must not write is
checked with what it must.  tests/test_estimation_turnover_host.py asserts, without a device, that the shapes lie on the intended
side of the kernels' constants.

    staging      G = 300 graphs (the g += gridDim.y loop, row = first_row + g and rows[g]); N = 1030 (the second tile column);
                 K = 300 sensors (the second trip of the slot[] loop), in all four instantiations
    write-back   N < 4 (a chunk spans graphs); total > 4096 * 1024 elements (the grid-stride trip), element and vector stores
    reduce       more chunks than 2048 * 256, W = 1 and W = 4
    moments      N > 64 (workgroups with v_lo > 0, sensors on 64-node boundaries), K = 600 (the k += NE_T loop), S = 130 (a third
                 row trip of the error moments)
    pair errors  N > 256 (a lane's second trip, partial chunks there), G = 9 (a last workgroup with one live wave)
    fold         S > 8 (the second LR_U trip), a pass cut in two launches"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import turnover_cases as T      # noqa: E402
from estimation_refs import (DEV, check_moments, check_records, check_sums, garbage, numpy_fold,      # noqa: E402
                             numpy_node_moments, numpy_normalise, numpy_pair_errors, numpy_reduce, numpy_spread_moments,
                             numpy_stage, numpy_write_back)

PAD = 4                       # elements of garbage in front of and behind every staging target
NAN_BITS = 0x7FC00000         # torch.full(..., nan) in a garbage target
FILL = -777.25                # the other targets


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ---- 1. staging -------------------------------------------------------------------------------------------------------------------
def launch_stage(pkg, lib, entry, src, layout, n, g, observed, *, rows=None, first=0, norm=(0, 0.0, 1.0), available=None, nan=0,
                 shift=0, count=1, member0=0, sigma=None, seed=0, layouts=None):
    """One launch of a staging entry point into a garbage target that starts PAD + ``shift`` elements into its allocation
    (``shift`` = 1: one float past a 16-byte boundary).  Asserts that nothing outside the g * n elements was written; returns
    (x as int32 bits, mask) of the batch, on the host."""
    x, mask = garbage(g * n + 2 * PAD)
    at = PAD + shift
    xp, mp = x.data_ptr() + 4 * at, mask.data_ptr() + at
    ptr = pkg._native.ptr
    d_src, obs, K = dev(src), dev(np.asarray(observed, dtype=np.int32)), len(observed)
    d_rows = None if rows is None else dev(rows)
    d_av = None if available is None else dev(available)
    S = src.shape[0]
    if entry == "plain":
        rc = lib.gatres_stage_observed(d_src.data_ptr(), layout, S, ptr(d_rows), first, n, g, obs.data_ptr(), K, *norm, xp, mp,
                                       stream())
    elif entry == "available":
        rc = lib.gatres_stage_observed_available(d_src.data_ptr(), layout, S, ptr(d_rows), first, n, g, obs.data_ptr(), K, *norm,
                                                 xp, mp, ptr(d_av), nan, stream())
    elif entry == "noisy":
        d_sigma = dev(np.asarray(sigma, dtype=np.float32))
        rc = lib.gatres_stage_observed_noisy(d_src.data_ptr(), layout, S, first, count, member0, n, g, obs.data_ptr(), K, *norm,
                                             xp, mp, ptr(d_av), nan, d_sigma.data_ptr(), seed, stream())
    else:
        d_lay = dev(np.asarray(layouts, dtype=np.uint8))
        rc = lib.gatres_stage_observed_layouts(d_src.data_ptr(), layout, S, first, count, n, g, obs.data_ptr(), K, *norm, xp, mp,
                                               ptr(d_av), nan, d_lay.data_ptr(), stream())
    pkg._native.check(rc, "gatres_stage_observed (" + entry + ")")
    xb, mb = x.cpu().numpy().view(np.int32), mask.cpu().numpy()
    lo, hi = at, at + g * n
    assert (xb[:lo] == NAN_BITS).all() and (xb[hi:] == NAN_BITS).all(), "x written outside the batch"
    assert (mb[:lo] == 0xAB).all() and (mb[hi:] == 0xAB).all(), "mask written outside the batch"
    return xb[lo:hi], mb[lo:hi]


def assert_staged(got, want, what=""):
    (x, mask), (ex, em) = got, want
    wrong = np.nonzero((x != ex) | (mask != em))[0]
    assert wrong.size == 0, f"{what}: {wrong.size} elements differ, the first at flat index {int(wrong[0])}"


def znorm(readings):
    """The offset and factor a znorm store hands to the readings layout: its mean, and its std plus the reference's 1e-8."""
    return float(readings.astype(np.float64).mean()), float(readings.astype(np.float64).std()) + 1e-8


@pytest.mark.parametrize("form", ["first_row", "rows", "readings_divide", "readings_reciprocal"])
@pytest.mark.parametrize("entry", ["plain", "available"])
def test_staging_more_graphs_than_grid_rows(pkg, lib, entry, form):
    c = T.STAGE_MANY_GRAPHS
    N, G, S, observed = c["N"], c["G"], c["S"], c["observed"]
    K = len(observed)
    src = T.pressures(S, N, seed=1)
    av = T.availability(S, K, 0.2, seed=2) if entry == "available" else None
    if form in ("first_row", "rows"):
        rows = T.rows_with_a_repeat(S) if form == "rows" else None
        order = np.arange(G) if rows is None else rows
        assert len(set(order.tolist())) == (G if rows is None else G - 1)
        got = launch_stage(pkg, lib, entry, src, 0, N, G, observed, rows=rows, first=5 if form == "rows" else 0, available=av)
        want = numpy_stage(src[order][:, observed], N, observed, None if av is None else av[order])
        assert_staged(got, want, form)
        return
    mode = 1 if form == "readings_divide" else 2
    readings = np.ascontiguousarray(src[:, observed])
    offset, factor = znorm(readings)
    values = numpy_normalise(readings, mode, offset, factor)
    got = launch_stage(pkg, lib, entry, readings, 1, N, G, observed, norm=(mode, offset, factor), available=av)
    assert_staged(got, numpy_stage(values, N, observed, av), form)
    if entry == "available":                                       # NaN readings are missing readings, with available and alone
        holes = T.nan_holes(S, K, seed=4)
        assert (holes & (av != 0)).any() and (holes & (av == 0)).any()
        holed = np.where(holes, np.float32("nan"), readings).astype(np.float32)
        got = launch_stage(pkg, lib, entry, holed, 1, N, G, observed, norm=(mode, offset, factor), available=av, nan=1)
        assert_staged(got, numpy_stage(values, N, observed, (av != 0) & ~holes), form + " with NaN readings")
        got = launch_stage(pkg, lib, entry, holed, 1, N, G, observed, norm=(mode, offset, factor), nan=1)
        assert_staged(got, numpy_stage(values, N, observed, ~holes), form + " with NaN readings alone")


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "one_float_past"])
@pytest.mark.parametrize("entry", ["plain", "available"])
def test_staging_around_the_second_tile_column(pkg, lib, entry, shift):
    c = T.STAGE_SECOND_TILE
    N, G, S, first, observed = c["N"], c["G"], c["S"], c["first_row"], c["observed"]
    src = T.pressures(S, N, seed=5)
    av = T.availability(S, len(observed), 0.2, seed=6) if entry == "available" else None
    got = launch_stage(pkg, lib, entry, src, 0, N, G, observed, first=first, available=av, shift=shift)
    sl = slice(first, first + G)
    assert_staged(got, numpy_stage(src[sl][:, observed], N, observed, None if av is None else av[sl]))


def many_sensors_case():
    c = T.STAGE_MANY_SENSORS
    observed = T.many_sensors()
    src = T.pressures(c["S"], c["N"], seed=7)
    return c["N"], c["G"], c["S"], c["first_row"], observed, src, T.availability(c["S"], c["K"], 0.2, seed=8)


@pytest.mark.parametrize("entry", ["plain", "available"])
def test_staging_more_sensors_than_threads(pkg, lib, entry):
    N, G, S, first, observed, src, av = many_sensors_case()
    av = av if entry == "available" else None
    sl = slice(first, first + G)
    got = launch_stage(pkg, lib, entry, src, 0, N, G, observed, first=first, available=av)
    assert_staged(got, numpy_stage(src[sl][:, observed], N, observed, None if av is None else av[sl]), "full rows")
    readings = np.ascontiguousarray(src[:, observed])
    offset, factor = znorm(readings)
    holes = T.nan_holes(S, len(observed), seed=9) if entry == "available" else np.zeros(readings.shape, dtype=bool)
    holed = np.where(holes, np.float32("nan"), readings).astype(np.float32)
    present = ~holes if av is None else (av != 0) & ~holes
    got = launch_stage(pkg, lib, entry, holed, 1, N, G, observed, first=first, norm=(2, offset, factor), available=av,
                       nan=int(entry == "available"))
    assert_staged(got, numpy_stage(numpy_normalise(readings, 2, offset, factor)[sl], N, observed, present[sl]), "readings")


def test_layouts_staging_more_sensors_than_threads(pkg, lib):
    N, _, S, _, observed, src, av = many_sensors_case()
    p = T.STAGE_PAIRS
    L, first, G = p["layouts"], p["first_pair"], p["G"]
    lay = T.pair_layouts(L, len(observed))
    pair = first + np.arange(G)
    row, l = pair // L, pair % L
    assert len(set(row.tolist())) > 1
    for available in (av, None):
        got = launch_stage(pkg, lib, "layouts", src, 0, N, G, observed, first=first, count=L, layouts=lay, available=available)
        present = lay[l] if available is None else lay[l] & available[row]
        assert_staged(got, numpy_stage(src[row][:, observed], N, observed, present))


def test_noisy_staging_more_sensors_than_threads(pkg, lib):
    """sigma = 0: the launch is the one without noise, bit for bit.  sigma > 0: the mask and the zeros bit for bit; a present
    reading r is staged as r + sigma z with the device's fp32 z, which tests/test_gpu_estimation_noise.py holds within 1e-5 of
    ``reading_noise`` (fp64): |x - (r + sigma z)| <= sigma * 1e-5 + 2^-23 (|r| + sigma |z|), the second term for the two fp32
    roundings of the product and the sum."""
    N, _, S, _, observed, src, av = many_sensors_case()
    p = T.STAGE_PAIRS
    M, first, G, seed = p["members"], p["first_pair"], p["G"], 20260
    K = len(observed)
    pair = first + np.arange(G)
    row, member = pair // M, pair % M
    assert len(set(row.tolist())) > 1
    values, present = src[row][:, observed], av[row]
    want = numpy_stage(values, N, observed, present)
    got = launch_stage(pkg, lib, "noisy", src, 0, N, G, observed, first=first, count=M, sigma=np.zeros(K), seed=seed, available=av)
    assert_staged(got, want, "sigma = 0")
    sigma = (0.1 + 0.6 * np.random.default_rng(10).random(K)).astype(np.float32)
    x, mask = launch_stage(pkg, lib, "noisy", src, 0, N, G, observed, first=first, count=M, sigma=sigma, seed=seed, available=av)
    assert (mask == want[1]).all()
    x = x.view(np.float32).reshape(G, N)
    assert (x.view(np.int32)[mask.reshape(G, N) != 0] == 0).all()
    z = pkg.estimation.reading_noise(seed, M, S, K)[row, member]                   # [G, K]
    exact = values.astype(np.float64) + sigma.astype(np.float64) * z
    bound = sigma.astype(np.float64) * 1e-5 + 2.0 ** -23 * (np.abs(values) + sigma * np.abs(z))
    err = np.abs(x[:, observed].astype(np.float64) - exact)
    here = present != 0
    print(f"noisy staging at K = {K}: max error / bound {float((err / bound)[here].max()):.3f} over {int(here.sum())} readings")
    assert (err <= bound)[here].all()
    assert (x[:, observed][here] != values[here]).mean() > 0.99                    # (the noise is there)


# ---- 2. write-back ----------------------------------------------------------------------------------------------------------------
def write_back_case(pkg, lib, N, G, stride, keep, first, rows):
    rng = np.random.default_rng(N * 7 + G + keep)
    out = rng.standard_normal(G * N).astype(np.float32)
    x = rng.standard_normal(G * N).astype(np.float32)
    mask = (rng.random(G * N) < 0.7).astype(np.uint8)
    start = np.full((rows, stride), FILL, dtype=np.float32)
    dst = dev(start)
    d_out, d_x, d_mask = dev(out), dev(x), dev(mask)
    pkg._native.check(lib.gatres_estimate_write(d_out.data_ptr(), d_x.data_ptr(), d_mask.data_ptr(), N, G, T.SCALE, T.OFFSET, keep,
                                                dst.data_ptr(), rows, stride, first, stream()), "gatres_estimate_write")
    want = numpy_write_back(out, x, mask, N, T.SCALE, T.OFFSET, keep, start, first)
    wrong = np.nonzero(bits(dst.cpu().numpy()) != bits(want))
    assert wrong[0].size == 0, f"{wrong[0].size} elements differ, the first at row {int(wrong[0][0])}, column {int(wrong[1][0])}"


@pytest.mark.parametrize("keep", [0, 1])
@pytest.mark.parametrize("N", T.WRITE_SMALL["N"])
def test_write_back_of_graphs_shorter_than_a_chunk(pkg, lib, N, keep):
    for stride in (N + 1, N):                                       # (no N here is a multiple of four: element stores)
        write_back_case(pkg, lib, N, T.WRITE_SMALL["G"], stride, keep, first=2, rows=T.WRITE_SMALL["G"] + 4)


@pytest.mark.parametrize("case", sorted(T.WRITE_CAPPED))
def test_write_back_above_the_grid_cap(pkg, lib, case):
    c = T.WRITE_CAPPED[case]
    write_back_case(pkg, lib, c["N"], c["G"], c["stride"], 1, first=3, rows=c["G"] + 5)


# ---- 3. ensemble reduce -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(T.REDUCE_CAPPED))
def test_ensemble_reduce_above_the_grid_cap(pkg, lib, case):
    c = T.REDUCE_CAPPED[case]
    N, stride, M, C = c["N"], c["stride"], c["M"], c["C"]
    first, rows = 1, C + 2
    mat = (50.0 + 0.1 * np.random.default_rng(C).standard_normal((C * M, stride))).astype(np.float32)
    d_mat = dev(mat)
    mean, sd = dev(np.full((rows, stride), FILL, dtype=np.float32)), dev(np.full((rows, stride), FILL, dtype=np.float32))
    pkg._native.check(lib.gatres_ensemble_reduce(d_mat.data_ptr(), C, M, N, stride, mean.data_ptr(), sd.data_ptr(), rows, stride,
                                                 first, stream()), "gatres_ensemble_reduce")
    want_mean, want_sd = numpy_reduce(mat.reshape(C, M, stride)[:, :, :N])
    for name, got, want in (("mean", mean, want_mean), ("sd", sd, want_sd)):
        full = np.full((rows, stride), FILL, dtype=np.float32)
        full[first:first + C, :N] = want
        wrong = np.nonzero(bits(got.cpu().numpy()) != bits(full))
        assert wrong[0].size == 0, f"{name}: {wrong[0].size} elements differ, the first at row {int(wrong[0][0])}"
    assert (want_sd > 0).mean() > 0.99                             # (two members can hold the same fp32 value)


# ---- 4. per-node moments ----------------------------------------------------------------------------------------------------------
def moments_table(pkg, lib, est, truth, observed, available=None):
    """One launch into a NaN-filled table with a guard record behind it; the table on the host."""
    S, N = est.shape
    obs = dev(np.asarray(observed, dtype=np.int32))
    table = torch.full((N + 1, 8), float("nan"), dtype=torch.float64, device=DEV)
    if available is None:
        rc = lib.gatres_node_error_moments(est.data_ptr(), truth.data_ptr(), S, N, T.SCALE, T.OFFSET, obs.data_ptr(), len(observed),
                                           table.data_ptr(), stream())
    else:
        rc = lib.gatres_node_error_moments_available(est.data_ptr(), truth.data_ptr(), S, N, T.SCALE, T.OFFSET, obs.data_ptr(),
                                                     len(observed), available.data_ptr(), table.data_ptr(), stream())
    pkg._native.check(rc, "gatres_node_error_moments")
    t = table.cpu().numpy()
    assert np.isnan(t[N]).all(), "a record behind the table was written"
    return t[:N]


MOMENT_SHAPES = T.MOMENTS_SMALL + [(T.MOMENTS_LARGE["N"], T.MOMENTS_LARGE["S"])]


@pytest.mark.parametrize("N,S", MOMENT_SHAPES)
def test_error_moments_beyond_the_first_workgroup(pkg, lib, N, S):
    observed = T.moment_sensors(N)
    K = len(observed)
    est, truth = T.moments_inputs(N, S)
    d_est, d_truth = dev(est), dev(truth)
    plain = moments_table(pkg, lib, d_est, d_truth, observed)
    assert plain.tobytes() == moments_table(pkg, lib, d_est, d_truth, observed).tobytes()        # the same bits every run
    check_moments(plain, numpy_node_moments(est, truth, T.SCALE, T.OFFSET, observed), S)
    zc = T.zero_column(N)
    assert plain[zc, 5] == 0 and plain[zc, 6] == 0 and (np.delete(plain[:, 5], zc) == S).all()
    # some readings missing
    av = T.availability(S, K, 0.3, seed=N + S)
    d_av = dev(av)
    hidden = moments_table(pkg, lib, d_est, d_truth, observed, d_av)
    assert hidden.tobytes() == moments_table(pkg, lib, d_est, d_truth, observed, d_av).tobytes()
    check_moments(hidden, numpy_node_moments(est, truth, T.SCALE, T.OFFSET, observed, av), S)
    sensor = np.zeros(N, dtype=bool)
    sensor[observed] = True
    # (sensor 0 is never available: every entry hidden, the sums of the kernel without availability; sensor 1 always is)
    assert hidden[observed[0]].tobytes() == np.concatenate(([float(S)], plain[observed[0], 1:7], [0.0])).tobytes()
    assert hidden[observed[1]].tolist() == [0.0] * 7 + [float(S)]
    # every reading present: a node outside the sensors has the record of the kernel without availability, bit for bit; a
    # sensor has no hidden entry
    ones = moments_table(pkg, lib, d_est, d_truth, observed, dev(np.ones((S, K), dtype=np.uint8)))
    assert ones[~sensor].tobytes() == plain[~sensor].tobytes()
    assert (ones[sensor] == np.array([0.0] * 7 + [float(S)])).all()
    # no reading present: no lane skips an entry, and the sums [1..6] of EVERY node are those of the kernel without
    # availability, bit for bit
    none = moments_table(pkg, lib, d_est, d_truth, observed, dev(np.zeros((S, K), dtype=np.uint8)))
    assert none[:, 1:7].tobytes() == plain[:, 1:7].tobytes()
    assert (none[:, 0] == S).all() and (none[:, 7] == 0).all()


@pytest.mark.parametrize("N,S", MOMENT_SHAPES)
def test_spread_moments_beyond_the_first_workgroup(pkg, lib, N, S):
    sd = T.spread_inputs(N, S)
    d_sd = dev(sd)

    def table():
        t = torch.full((N + 1, 4), float("nan"), dtype=torch.float64, device=DEV)
        pkg._native.check(lib.gatres_node_spread_moments(d_sd.data_ptr(), S, N, t.data_ptr(), stream()), "gatres_node_spread_moments")
        t = t.cpu().numpy()
        assert np.isnan(t[N]).all(), "a record behind the table was written"
        return t[:N]

    got, want = table(), numpy_spread_moments(sd)
    assert got.tobytes() == table().tobytes()                      # the same bits every run
    np.testing.assert_array_equal(got[:, 0], want[:, 0])
    np.testing.assert_array_equal(got[:, 2], want[:, 2])
    check_sums(got[:, 1], want[:, 1], S, "sum sd^2")
    check_sums(got[:, 3], want[:, 3], S, "sum sd")
    assert got[N - 1, 2] == 3.5 and got[9].tolist() == [S, 0.0, 0.0, 0.0]


# ---- 5. layout errors -------------------------------------------------------------------------------------------------------------
def one_past(a):
    """``a`` on the device, starting one element past a 16-byte boundary."""
    flat = np.ascontiguousarray(a).reshape(-1)
    buf = torch.empty(flat.size + 1, dtype=torch.from_numpy(flat).dtype, device=DEV)
    buf[1:] = torch.from_numpy(flat).to(DEV)
    return buf[1:]


@pytest.mark.parametrize("first_pair", T.PAIRS["first_pair"])
@pytest.mark.parametrize("scored", [False, True], ids=["every_node", "score"])
@pytest.mark.parametrize("N", T.PAIRS["N"])
def test_pair_errors_beyond_a_lanes_first_trip(pkg, lib, N, scored, first_pair):
    G, L, rows = T.PAIRS["G"], T.PAIRS["L"], T.PAIRS["truth_rows"]
    rec_rows, rec_first = G + 4, 2
    out, mask, truth, score = T.pair_inputs(N, scored)
    s = (first_pair + np.arange(G)) // L
    assert len(set(s.tolist())) >= 3 and s.max() < rows

    def launch(place):
        o, m, t = place(out), place(mask), place(truth)
        sc = None if score is None else place(score)
        rec = torch.full((rec_rows, 4), FILL, dtype=torch.float64, device=DEV)
        pkg._native.check(lib.gatres_layout_pair_errors(
            o.data_ptr(), m.data_ptr(), t.data_ptr(), rows, N, G, first_pair, L, T.SCALE, T.OFFSET, pkg._native.ptr(sc),
            rec.data_ptr(), rec_rows, rec_first, stream()), "gatres_layout_pair_errors")
        return rec.cpu().numpy()

    rec = launch(dev)
    assert rec.tobytes() == launch(dev).tobytes()                  # the same bits every run
    assert rec.tobytes() == launch(one_past).tobytes()             # element loads: the same additions in the same order
    got = rec[rec_first:rec_first + G]
    check_records(got, numpy_pair_errors(out, mask, truth[s], T.SCALE, T.OFFSET, score), N)
    empty = T.PAIRS["empty_graph"]
    assert got[empty].tolist() == [0.0] * 4 and (np.delete(got[:, 0], empty) > 0).all()
    assert (np.delete(rec, np.s_[rec_first:rec_first + G], axis=0) == FILL).all()               # the neighbouring records


def fold(pkg, lib, rec, S, L, table, accumulate):
    pkg._native.check(lib.gatres_layout_error_reduce(rec.data_ptr(), S, L, table.data_ptr(), accumulate, stream()),
                      "gatres_layout_error_reduce")


@pytest.mark.parametrize("S,L", T.FOLD)
def test_layout_error_reduce_beyond_the_first_trip(pkg, lib, S, L):
    rec = T.fold_records(S, L)
    d_rec = dev(rec)
    want = numpy_fold(rec, S, L)
    table = torch.full((L + 1, 4), float("nan"), dtype=torch.float64, device=DEV)      # (garbage: accumulate = 0 starts from zero)
    fold(pkg, lib, d_rec, S, L, table, 0)
    assert table[:L].cpu().numpy().tobytes() == want.tobytes()
    assert torch.isnan(table[L]).all()                              # nothing past the table
    if S != sum(T.FOLD_CUT):
        return
    a, b = T.FOLD_CUT                                               # the same pass in two launches: the same bits
    two = torch.full((L, 4), float("nan"), dtype=torch.float64, device=DEV)
    fold(pkg, lib, d_rec[:a * L], a, L, two, 0)
    assert two.cpu().numpy().tobytes() == numpy_fold(rec[:a * L], a, L).tobytes()
    fold(pkg, lib, d_rec[a * L:], b, L, two, 1)
    assert two.cpu().numpy().tobytes() == want.tobytes()
