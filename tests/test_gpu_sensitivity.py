"""The sensitivity pass on the device (PressureEstimator.sensitivity / sensitivity_map / linear_spread; k_sensitivity.hip and
gatres_stage_observed_targets of k_estimate.hip): the staging with targets and the three small launches bit for bit against
their numpy statements, the pass bit for bit against the hand-written autograd loop it replaces, its rows against the fp64
oracle's Jacobian under the project's gradient yardstick, the locality rule exactly, and the other public methods.  These are
the first tests of ``g_x`` of gatres_model_backward on the window, the whole-segment and the per-op path.

Shapes: graphs of 37 and 40 nodes (odd and 16-byte phases) with 1, 5 and N targets in batches of 4, so batches straddle
snapshots; the staging kernel's three turnovers of tests/turnover_cases.py; 388 nodes once for gatres_small on the window
kernel."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import sensitivity_refs as R      # noqa: E402
import turnover_cases as T      # noqa: E402
from estimation_refs import DEV, garbage, numpy_normalise, numpy_stage, torch_stage, torch_stage_available      # noqa: E402
from test_gpu_model import build, check_gradients_vs_fp64, note      # noqa: E402

PAD = 4                       # elements of garbage in front of and behind every target
NAN_BITS = 0x7FC00000
FILL = -777.25
OBS = [36, 0, 5]              # unsorted: column k is node OBS[k]
OBS8 = [36, 0, 5, 17, 22, 9, 30, 13]
_CACHE = {}
_J64_CACHE = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def topology(pkg, n, pipes):
    key = ("ei", n, pipes)
    if key not in _CACHE:
        _CACHE[key] = pkg.wdn_synth.make_wdn_topology(n, pipes, seed=0)
    return _CACHE[key]


def make_store(pkg, S, n, pipes, seed=1, **kw):
    raw = pkg.wdn_synth.make_snapshots(S, n, seed=seed) * 12.5 + 50.0
    return pkg.SnapshotStore(raw, topology(pkg, n, pipes), device=DEV, **kw)


# ---- 1. staging with targets ----------------------------------------------------------------------------------------------------
def launch_targets(pkg, lib, src, layout, n, g, observed, first, num_targets, targets=None, *, norm=(0, 0.0, 1.0), available=None,
                   nan=0, shift=0, gshift=0):
    """One launch of gatres_stage_observed_targets into garbage targets that start PAD + ``shift`` (x, mask) and PAD +
    ``gshift`` (g_out) elements into their allocations.  Asserts that nothing outside the g * n elements was written; returns
    (x as int32 bits, mask, g_out as int32 bits) of the batch, on the host."""
    x, mask = garbage(g * n + 2 * PAD)
    seeds, _ = garbage(g * n + 2 * PAD)
    at, gat = PAD + shift, PAD + gshift
    ptr = pkg._native.ptr
    d_src, obs = dev(src), dev(np.asarray(observed, dtype=np.int32))
    d_t = None if targets is None else dev(np.asarray(targets, dtype=np.int32))
    d_av = None if available is None else dev(available)
    rc = lib.gatres_stage_observed_targets(d_src.data_ptr(), layout, src.shape[0], first, num_targets, ptr(d_t), n, g,
                                           obs.data_ptr(), len(observed), *norm, x.data_ptr() + 4 * at, mask.data_ptr() + at,
                                           seeds.data_ptr() + 4 * gat, ptr(d_av), nan, stream())
    pkg._native.check(rc, "gatres_stage_observed_targets")
    xb, mb, sb = x.cpu().numpy().view(np.int32), mask.cpu().numpy(), seeds.cpu().numpy().view(np.int32)
    assert (xb[:at] == NAN_BITS).all() and (xb[at + g * n:] == NAN_BITS).all(), "x written outside the batch"
    assert (mb[:at] == 0xAB).all() and (mb[at + g * n:] == 0xAB).all(), "mask written outside the batch"
    assert (sb[:gat] == NAN_BITS).all() and (sb[gat + g * n:] == NAN_BITS).all(), "g_out written outside the batch"
    return xb[at:at + g * n], mb[at:at + g * n], sb[gat:gat + g * n]


def expect_targets(pkg, values, n, observed, present, first, g, num_targets, targets):
    """The statement the launch is held to: the pair's source row staged as gatres_stage_observed_available stages it
    (``numpy_stage`` of the rows' values and presence) plus ``sensitivity_seeds``."""
    row = (first + np.arange(g)) // num_targets
    x, mask = numpy_stage(values[row], n, observed, None if present is None else present[row])
    return x, mask, bits(pkg.sensitivity_seeds(first, g, n, num_targets, targets)).reshape(-1)


def assert_staged3(got, want, what=""):
    for name, a, b in zip(("x", "mask", "g_out"), got, want):
        wrong = np.nonzero(a != b)[0]
        assert wrong.size == 0, f"{what}: {name}: {wrong.size} elements differ, the first at flat index {int(wrong[0])}"


@pytest.mark.parametrize("tcase", ["T1", "T5", "TN"])
@pytest.mark.parametrize("n", [37, 40])
def test_staging_with_targets_bitwise(pkg, lib, n, tcase):
    S, bs = 3, 4
    targets = {"T1": [n - 1], "T5": [7, n - 1, 0, 7, 20], "TN": None}[tcase]          # (a target may be named twice)
    num_targets = n if targets is None else len(targets)
    src = T.pressures(S, n, seed=n)
    av = T.availability(S, len(OBS), 0.3, seed=2)
    av[1, 1] = 0
    readings = np.ascontiguousarray(src[:, OBS])
    offset, factor = float(readings.astype(np.float64).mean()), float(readings.astype(np.float64).std()) + 1e-8
    holes = np.zeros(readings.shape, dtype=bool)
    holes[0, 1] = holes[2, 2] = True
    holed = np.where(holes, np.float32("nan"), readings).astype(np.float32)
    pairs = S * num_targets
    firsts = list(range(0, pairs, bs)) if num_targets <= 5 else [0, 36, pairs - 3]
    if tcase == "T5":
        assert any((f // 5) != ((f + bs - 1) // 5) for f in firsts)                  # a batch straddles two snapshots
    for first in firsts:
        g = min(bs, pairs - first)
        for gshift in (0, 1):                                                        # (g_out aligned and one float past)
            what = f"first {first} gshift {gshift}"
            # full rows of a store with gaps
            got = launch_targets(pkg, lib, src, 0, n, g, OBS, first, num_targets, targets, available=av, gshift=gshift)
            assert_staged3(got, expect_targets(pkg, src[:, OBS], n, OBS, av, first, g, num_targets, targets), "full rows " + what)
            # readings of a znorm estimator with gaps and NaN readings
            got = launch_targets(pkg, lib, holed, 1, n, g, OBS, first, num_targets, targets, norm=(2, offset, factor),
                                 available=av, nan=1, gshift=gshift)
            want = expect_targets(pkg, numpy_normalise(readings, 2, offset, factor), n, OBS, (av != 0) & ~holes, first, g,
                                  num_targets, targets)
            assert_staged3(got, want, "znorm readings " + what)
        # readings of an `unused` estimator, every reading there, everything one float past a 16-byte boundary
        got = launch_targets(pkg, lib, readings, 1, n, g, OBS, first, num_targets, targets, shift=1, gshift=1)
        assert_staged3(got, expect_targets(pkg, readings, n, OBS, None, first, g, num_targets, targets), f"unused first {first}")
        got = launch_targets(pkg, lib, readings, 1, n, g, OBS, first, num_targets, targets, norm=(1, offset, factor))
        assert_staged3(got, expect_targets(pkg, numpy_normalise(readings, 1, offset, factor), n, OBS, None, first, g,
                                           num_targets, targets), f"divide first {first}")


def test_staging_with_targets_more_graphs_than_grid_rows(pkg, lib):
    c = T.STAGE_MANY_GRAPHS
    N, G, S, observed = c["N"], c["G"], c["S"], c["observed"]
    num_targets, first = 7, 11
    targets = [36, 0, 5, 12, 36, 20, 1]
    src = T.pressures(S, N, seed=1)
    av = T.availability(S, len(observed), 0.2, seed=2)
    assert (first + G - 1) // num_targets < S
    for shift, gshift in ((0, 0), (0, 1), (1, 0)):
        got = launch_targets(pkg, lib, src, 0, N, G, observed, first, num_targets, targets, available=av, shift=shift, gshift=gshift)
        assert_staged3(got, expect_targets(pkg, src[:, observed], N, observed, av, first, G, num_targets, targets), f"{shift} {gshift}")


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "one_float_past"])
def test_staging_with_targets_around_the_second_tile_column(pkg, lib, shift):
    c = T.STAGE_SECOND_TILE
    N, S, observed = c["N"], c["S"], c["observed"]
    targets = [1019, 1029, 0, 1020, 1023, 1024]                                      # seeds on both sides of the tile boundary
    num_targets, first, G = len(targets), 5, 7                                       # pairs 5 .. 11: rows 0 and 1
    src = T.pressures(S, N, seed=5)
    av = T.availability(S, len(observed), 0.2, seed=6)
    for gshift in (0, 1):
        got = launch_targets(pkg, lib, src, 0, N, G, observed, first, num_targets, targets, available=av, shift=shift, gshift=gshift)
        assert_staged3(got, expect_targets(pkg, src[:, observed], N, observed, av, first, G, num_targets, targets), f"gshift {gshift}")
    got = launch_targets(pkg, lib, src, 0, N, 3, observed, 1028, N, None, shift=shift)   # all N targets, unnamed: nodes 1028, 1029, 0
    assert_staged3(got, expect_targets(pkg, src[:, observed], N, observed, None, 1028, 3, N, None), "unnamed targets")


def test_staging_with_targets_more_sensors_than_threads(pkg, lib):
    c, p = T.STAGE_MANY_SENSORS, T.STAGE_PAIRS
    N, S = c["N"], c["S"]
    observed = T.many_sensors()
    src = T.pressures(S, N, seed=7)
    av = T.availability(S, c["K"], 0.2, seed=8)
    num_targets, first, G = p["layouts"], p["first_pair"], p["G"]
    targets = [1029, 0, 1022]
    for available in (av, None):
        got = launch_targets(pkg, lib, src, 0, N, G, observed, first, num_targets, targets, available=available)
        assert_staged3(got, expect_targets(pkg, src[:, observed], N, observed, available, first, G, num_targets, targets))


# ---- 2. gather, fold, spread ----------------------------------------------------------------------------------------------------
def gather_case(pkg, lib, N, K, G, observed, fault=None, stride=None, rows=None, first=0, plant=True):
    rng = np.random.default_rng(1000 * N + 10 * K + G)
    g_x = rng.standard_normal((G, N)).astype(np.float32)
    mask = (rng.random((G, N)) < 0.3).astype(np.uint8)
    if plant:                                                   # a masked sensor whose g_x is a NaN, an unmasked one beside it
        mask[0, observed[0]] = 1
        g_x[0, observed[0]] = np.float32("nan")
        if G > 1 or K > 1:
            mask[G - 1, observed[K - 1]] = 0
    unit = 12.81 / (12.81 + 1e-8)
    stride = K if stride is None else stride
    rows = G if rows is None else rows
    J = torch.full((rows * stride + 2 * PAD,), FILL, dtype=torch.float32, device=DEV)
    d_gx, d_mask, d_obs = dev(g_x), dev(mask), dev(np.asarray(observed, dtype=np.int32))
    d_fault = None if fault is None else dev(np.asarray([fault], dtype=np.float32))
    pkg._native.check(lib.gatres_sensitivity_gather(d_gx.data_ptr(), d_mask.data_ptr(), pkg._native.ptr(d_fault), N, G,
                                                    d_obs.data_ptr(), K, unit, J.data_ptr() + 4 * PAD, rows, stride, first,
                                                    stream()), "gatres_sensitivity_gather")
    want = np.full(rows * stride + 2 * PAD, FILL, dtype=np.float32)
    body = want[PAD:PAD + rows * stride].reshape(rows, stride)
    body[first:first + G, :K] = pkg.sensitivity_rows_from_gx(g_x, mask, observed, unit, fault)
    return bits(J.cpu().numpy()), bits(want), body[first:first + G, :K]


@pytest.mark.parametrize("G", [1, 3, 32, 33])
@pytest.mark.parametrize("K", [1, 7, 8])
def test_gather_bitwise(pkg, lib, K, G):
    N = 37
    observed = [int(v) for v in np.random.default_rng(K).permutation(N)[:K]]
    got, want, rows = gather_case(pkg, lib, N, K, G, observed)
    np.testing.assert_array_equal(got, want)
    assert rows[0, 0] == 0.0 and not np.isnan(rows).any()       # the planted NaN lies under the mask
    # into the middle of a wider matrix: nothing but the batch's rows and K columns is written
    got, want, _ = gather_case(pkg, lib, N, K, G, observed, stride=K + 3, rows=G + 5, first=2)
    np.testing.assert_array_equal(got, want)
    got, want, _ = gather_case(pkg, lib, N, K, G, observed, fault=0.5)
    np.testing.assert_array_equal(got, want)
    got, want, rows = gather_case(pkg, lib, N, K, G, observed, fault=float("nan"))
    assert np.isnan(rows).all() and rows.shape == (G, K)
    assert np.isnan(got.view(np.float32)[PAD:-PAD]).all() and (got[:PAD] == want[:PAD]).all() and (got[-PAD:] == want[-PAD:]).all()


def test_gather_above_the_grid_cap(pkg, lib):
    c = R.GATHER_CAPPED
    observed = [int(v) for v in np.random.default_rng(5).permutation(c["N"])[:c["K"]]]
    assert c["G"] * c["K"] > R.grid_cap("gatres_sensitivity_gather") * R.constants()["SG_T"]
    got, want, _ = gather_case(pkg, lib, c["N"], c["K"], c["G"], observed)
    np.testing.assert_array_equal(got, want)


def fold_launch(pkg, lib, J, table, accumulate, stride=None):
    S, T_, K = J.shape
    stride = K if stride is None else stride
    wide = np.full((S * T_, stride), np.float32(FILL))
    wide[:, :K] = J.reshape(S * T_, K)
    d_J = dev(wide)
    pkg._native.check(lib.gatres_sensitivity_fold(d_J.data_ptr(), S, T_, K, stride, table.data_ptr(), accumulate, stream()),
                      "gatres_sensitivity_fold")
    return table


def fold_input(S, T_, K):
    J = np.random.default_rng(100 * S + K).standard_normal((S, T_, K)).astype(np.float32)
    J[:, 0, K - 1] = 0.0                                        # a sensor that never reaches a junction
    J[S // 2, T_ - 1, 0] = 0.0
    return J


@pytest.mark.parametrize("S,T_,K", R.FOLD_TRIPS + [(1, 1, 1), (3, 2, 8)])
def test_fold_bitwise(pkg, lib, S, T_, K):
    J = fold_input(S, T_, K)
    table = torch.full((T_, K, 5), FILL, dtype=torch.float64, device=DEV)
    got = fold_launch(pkg, lib, J, table, 0, stride=K + 2).cpu().numpy()
    want = pkg.sensitivity_fold_ref(J)
    np.testing.assert_array_equal(got.view(np.int64), want.view(np.int64))
    assert want[0, K - 1, 0] == 0 and (want[0, K - 1] == 0).all()


def test_fold_in_chunks_equals_one_launch(pkg, lib):
    S, T_, K, cut = R.FOLD_CUT
    J = fold_input(S, T_, K)
    one = fold_launch(pkg, lib, J, torch.full((T_, K, 5), FILL, dtype=torch.float64, device=DEV), 0)
    two = torch.full((T_, K, 5), FILL, dtype=torch.float64, device=DEV)
    fold_launch(pkg, lib, J[:cut], two, 0)
    fold_launch(pkg, lib, J[cut:], two, 1)
    assert torch.equal(one, two)
    np.testing.assert_array_equal(one.cpu().numpy().view(np.int64), pkg.sensitivity_fold_ref(J).view(np.int64))
    np.testing.assert_array_equal(two.cpu().numpy(), pkg.sensitivity_fold_ref(J[cut:], table=pkg.sensitivity_fold_ref(J[:cut])))


@pytest.mark.parametrize("rows", [1, 3, 300])
@pytest.mark.parametrize("K", [1, 7, 8])
def test_spread_bitwise(pkg, lib, K, rows):
    rng = np.random.default_rng(10 * K + rows)
    J = rng.standard_normal((rows, K)).astype(np.float32)
    sigma = (rng.random(K) * 0.7).astype(np.float32)
    sigma[K // 2] = 0.0
    stride = K + 1
    wide = np.full((rows, stride), np.float32("nan"))
    wide[:, :K] = J
    d_J, d_sigma = dev(wide), dev(sigma)
    out = torch.full((rows + 2 * PAD,), FILL, dtype=torch.float32, device=DEV)
    pkg._native.check(lib.gatres_sensitivity_spread(d_J.data_ptr(), rows, K, stride, d_sigma.data_ptr(), out.data_ptr() + 4 * PAD,
                                                    stream()), "gatres_sensitivity_spread")
    want = np.full(rows + 2 * PAD, FILL, dtype=np.float32)
    want[PAD:PAD + rows] = pkg.linear_spread_ref(J, sigma)
    np.testing.assert_array_equal(bits(out.cpu().numpy()), bits(want))


# ---- 3. the pass against its hand-written loop ------------------------------------------------------------------------------------
def hand_loop(pkg, model, est, store, observed, bs, targets, available=None, count=None):
    """The loop the pass replaces, on the same plan and the same batches: staging with torch, ``x1.requires_grad_()``,
    ``model(x1, ei, None, None)``, ``out.backward(seed)``, ``x1.grad`` at the sensors times the unit, zero where missing.
    ``count``: the first snapshots of the store only."""
    n, S = store.nodes_per_graph, len(store) if count is None else count
    nodes = list(range(n)) if targets is None else list(targets)
    num_targets, K = len(nodes), len(observed)
    factor = est.std + est.eps if est.norm_type == "znorm" else 1.0
    unit = torch.tensor(np.float32(est.scale / factor), device=DEV)
    node_of = torch.tensor(nodes, dtype=torch.int64, device=DEV)
    J = torch.empty((S * num_targets, K), dtype=torch.float32, device=DEV)
    sizes = []
    for first in range(0, S * num_targets, bs):
        g = min(bs, S * num_targets - first)
        pair = torch.arange(first, first + g, device=DEV)
        row, t = pair // num_targets, pair % num_targets
        values = store.data[row][:, observed]
        if available is None:
            x1, mask = torch_stage(values, n, observed)
        else:
            x1, mask = torch_stage_available(values, n, observed, available[row])
        seed = torch.zeros((g, n), dtype=torch.float32, device=DEV)
        seed[torch.arange(g, device=DEV), node_of[t]] = 1.0
        x1 = x1.view(-1, 1).clone().requires_grad_()
        out = model(x1, store.edge_index(g), None, None)
        out.backward(seed.view(-1, 1))
        gx = x1.grad.view(g, n)[:, observed]
        J[first:first + g] = torch.where(mask.view(g, n)[:, observed].bool(), torch.zeros_like(gx), gx * unit)
        sizes.append(g)
    return J.view(S, num_targets, K), sizes


@pytest.mark.parametrize("n,pipes,nc", [(37, 43, 8), (40, 47, 16)])
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "per_op"])
def test_pass_equals_the_hand_written_loop_fp32(pkg, oracle, fused, n, pipes, nc):
    S, bs, targets = 3, 4, [7, n - 1, 0, 36, 20]
    store = make_store(pkg, S, n, pipes)
    model, _ = build(pkg, oracle, 2, nc, seed=3, fused=fused)
    est = pkg.PressureEstimator.for_store(model, store, OBS8, batch_size=bs)
    av = dev(T.availability(S, len(OBS8), 0.3, seed=4))
    for available in (None, av):
        got = est.sensitivity_store(store, targets=targets, available=available)
        want, sizes = hand_loop(pkg, model, est, store, OBS8, bs, targets, available)
        assert sizes == [4, 4, 4, 3] and got.shape == (S, 5, len(OBS8))
        assert torch.equal(got, want)
        assert float(got.abs().max()) > 0
    assert (got[:, :, 0] == 0).all()                            # sensor 0 never delivers in T.availability
    # the readings entry point stages the same values (the store's normalisation, bit for bit) and gives the same rows
    raw = pkg.wdn_synth.make_snapshots(S, n, seed=1) * 12.5 + 50.0
    readings = raw.to(DEV)[:, OBS8].contiguous()
    assert torch.equal(est.sensitivity(readings, targets=targets, available=av), got)
    # every junction: the default
    full = est.sensitivity_store(store, count=1)
    want, sizes = hand_loop(pkg, model, est, store, OBS8, bs, None, count=1)
    assert full.shape == (1, n, len(OBS8)) and sum(sizes) == n
    assert torch.equal(full, want)


def test_pass_equals_the_hand_written_loop_bf16(pkg, oracle):
    S, bs, targets, n, pipes = 3, 4, [7, 36, 0, 36, 20], 37, 43
    store = make_store(pkg, S, n, pipes)
    model, _ = build(pkg, oracle, 2, 32, seed=3, fused=False)
    model.set_compute_dtype("bf16")
    est = pkg.PressureEstimator.for_store(model, store, OBS8, batch_size=bs)
    got = est.sensitivity_store(store, targets=targets)
    want, sizes = hand_loop(pkg, model, est, store, OBS8, bs, targets)
    assert sizes == [4, 4, 4, 3]
    assert torch.equal(got, want) and float(got.abs().max()) > 0


SENSORS388 = [3, 17, 100, 101, 250, 387, 42, 9, 300, 77, 211, 5, 64, 128, 199, 350, 1, 260, 333, 150]


def small_on_the_window_kernel(pkg, oracle):
    if "small" not in _CACHE:
        n, pipes = 388, 430
        store = make_store(pkg, 2, n, pipes, seed=4)
        model, p = build(pkg, oracle, 15, 32, seed=11)
        plan = model.plan_for(store.edge_index(32), 32 * n)
        assert model._call_state(plan)["window"], "gatres_small at bs 32 should take the window kernel"
        est = pkg.PressureEstimator.for_store(model, store, SENSORS388, batch_size=32)
        targets = [int(v) for v in np.random.default_rng(388).permutation(n)[:32]] + SENSORS388[:8]
        _CACHE["small"] = (store, model, p, est, targets, est.sensitivity_store(store, count=1, targets=targets))
    return _CACHE["small"]


def test_gatres_small_at_batch_32_takes_the_window_kernel(pkg, oracle):
    store, model, _, est, targets, got = small_on_the_window_kernel(pkg, oracle)
    assert len(targets) == 40
    want, sizes = hand_loop(pkg, model, est, store, SENSORS388, 32, targets, count=1)
    assert sizes == [32, 8]                                     # one full batch on the window kernel, one ragged
    assert torch.equal(got, want) and float(got.abs().max()) > 0


# ---- 4. against the fp64 oracle's Jacobian --------------------------------------------------------------------------------------
def judge_rows(oracle, p, nb, store, est, observed, targets, got, key):
    """Every target row of snapshot 0 as one "tensor" of the project's gradient yardstick: the row's error against the fp64
    oracle's Jacobian at most the larger of twice the fp32 oracle's own error and max(1e-5 |row|max, 2e-6 |J|max), with the
    helpers' ReLU-kink fallback (the fp64 parameters perturbed by 1e-7)."""
    n = store.nodes_per_graph
    ei = store.edge_index(1).cpu()
    x1, _ = torch_stage(store.data[:1][:, observed], n, observed)
    x1 = x1.cpu()
    factor = est.std + est.eps if est.norm_type == "znorm" else 1.0
    unit = est.scale / factor

    def rows_of(params, dtype):
        pd = {k: v.to(dtype) for k, v in params.items()}
        xin = x1.to(dtype).reshape(-1, 1).clone().requires_grad_(True)
        out = oracle.gatres_forward(pd, xin, ei, num_blocks=nb).reshape(-1)
        return {j: torch.autograd.grad(out[j], xin, retain_graph=True)[0].reshape(-1)[observed] * unit for j in targets}

    p64 = {k: v.double() for k, v in p.items()}
    hip = {j: got[0, t] for t, j in enumerate(targets)}
    ref32 = rows_of(p, torch.float32)
    return check_gradients_vs_fp64(hip, ref32, lambda params: rows_of(params, torch.float64), p64, _J64_CACHE, key)


@pytest.mark.parametrize("n,pipes,nc", [(37, 43, 8), (40, 47, 16)])
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "per_op"])
def test_rows_against_the_fp64_oracles_jacobian(pkg, oracle, fused, n, pipes, nc):
    store = make_store(pkg, 2, n, pipes)
    model, p = build(pkg, oracle, 2, nc, seed=3, fused=fused)
    est = pkg.PressureEstimator.for_store(model, store, OBS8, batch_size=4)
    got = est.sensitivity_store(store, count=1)                 # every junction
    worst_rel, worst_ratio, branch = judge_rows(oracle, p, 2, store, est, OBS8, list(range(n)), got, ("J", n, nc))
    note(f"sensitivity n{n} nb2 nc{nc} {'fused' if fused else 'per-op'}: worst row err over |J|max vs fp64 / worst (hip err)/"
         f"(oracle32 err) / fp64 kink branch used", [worst_rel, worst_ratio, branch])


def test_gatres_small_rows_against_the_fp64_oracles_jacobian(pkg, oracle):
    store, _, p, est, targets, got = small_on_the_window_kernel(pkg, oracle)
    rows = [0, 5, 13, 21, 31, 32, 36, 39]                       # 8 target rows: six from the full batch, two sensors' own nodes
    sub = [targets[t] for t in rows]
    worst_rel, worst_ratio, branch = judge_rows(oracle, p, 15, store, est, SENSORS388, sub, got[:, rows], ("J", 388, 32))
    note("sensitivity n388 nb15 nc32 window: worst row err over |J|max vs fp64 / worst (hip err)/(oracle32 err) / fp64 kink "
         "branch used", [worst_rel, worst_ratio, branch])


# ---- 5. locality, exactly -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb,n,pipes", R.LOCALITY_CASES)
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "per_op"])
def test_sensitivity_is_exactly_zero_beyond_three_hops_per_block(pkg, oracle, fused, nb, n, pipes):
    observed = [int(v) for v in np.random.default_rng(n).permutation(n)]      # every node carries a sensor, in no order
    store = make_store(pkg, 2, n, pipes)
    model, _ = build(pkg, oracle, nb, 16 if nb == 0 else 8, seed=3, fused=fused)
    est = pkg.PressureEstimator.for_store(model, store, observed, batch_size=5)
    J = est.sensitivity_store(store).cpu().numpy()                            # [2, n, n]
    assert not np.isnan(J).any()
    dist = R.graph_distances(topology(pkg, n, pipes).numpy(), n)[:, observed]   # junction j to the node of sensor k
    far = dist > 3 * nb
    assert int(far.sum()) == {(0, 12): 132, (1, 40): 1044, (2, 40): 172, (2, 37): 120}[(nb, n)]
    assert (J[:, far] == 0.0).all()
    if nb == 0:                                                 # a junction follows its own sensor and nothing else
        assert (J[:, ~far] != 0.0).all() and (dist[~far] == 0).all()
    else:
        assert (J[:, ~far] != 0.0).mean() > 0.5


# ---- 6. the other public methods ------------------------------------------------------------------------------------------------
def public_case(pkg, oracle):
    if "public" not in _CACHE:
        n, pipes, S = 37, 43, 6
        store = make_store(pkg, S, n, pipes)
        model, _ = build(pkg, oracle, 2, 8, seed=3)
        est = pkg.PressureEstimator.for_store(model, store, OBS8, batch_size=4)
        av = T.availability(S, len(OBS8), 0.3, seed=4)
        _CACHE["public"] = (store, model, est, dev(av), av)
    return _CACHE["public"]


def test_sensitivity_map_equals_the_fold_of_sensitivity_store(pkg, oracle):
    store, _, est, d_av, _ = public_case(pkg, oracle)
    targets = [7, 36, 0, 36, 20, 11]
    J = est.sensitivity_store(store, first=1, count=5, targets=targets, available=d_av[1:].contiguous())
    want = pkg.sensitivity_fold_ref(J.cpu().numpy())
    K = len(OBS8)
    unit = 2 * 6 * K * 4                                        # ensemble_chunk's unit: lcm(4, 6) / 6 = 2 snapshots
    assert pkg.estimation.ensemble_chunk(5, 6, 4, 4 * K, unit) == 2       # three chunks: 2, 2 and 1 snapshots
    for budget in (unit, 64 << 20):
        m = est.sensitivity_map(store, first=1, count=5, targets=targets, available=d_av[1:].contiguous(), max_scratch_bytes=budget)
        assert isinstance(m, pkg.SensitivityMap) and m.num_snapshots == 5 and m.targets == targets and m.observed_idx == OBS8
        assert m.table.device == torch.device(DEV) and m.table.dtype == torch.float64
        np.testing.assert_array_equal(m.table.cpu().numpy().view(np.int64), want.view(np.int64))
    back = pkg.SensitivityMap.from_state_dict(m.state_dict(), device=DEV)
    assert torch.equal(back.table, m.table) and back.targets == targets
    # the report, from the map and from the store
    ref = pkg.influence_from_table(want, targets, OBS8, 5)
    for r in (est.influence_report(m), est.influence_report(store, first=1, count=5, targets=targets,
                                                             available=d_av[1:].contiguous(), max_scratch_bytes=unit)):
        assert sorted(r) == sorted(ref)
        for key, v in ref.items():
            np.testing.assert_array_equal(r[key], v, err_msg=key)
    assert (ref["mean_abs"][:, 0] == 0).all() and ref["sensor_dominates"][0] == 0      # sensor 0 never delivers
    t36 = targets.index(36)
    assert ref["self_entry"][OBS8.index(36)] == ref["mean"][t36, OBS8.index(36)] and np.isnan(ref["self_entry"][OBS8.index(5)])


def test_linear_spread_equals_its_statement_and_a_missing_sensor_adds_nothing(pkg, oracle):
    store, _, est, d_av, av = public_case(pkg, oracle)
    n, S = store.nodes_per_graph, len(store)
    raw = pkg.wdn_synth.make_snapshots(S, n, seed=1) * 12.5 + 50.0
    readings = raw.to(DEV)[:, OBS8].contiguous()
    noise = [0.1, 0.2, 0.05, 0.3, 0.0, 0.15, 0.25, 0.1]
    sigma = np.asarray(noise, dtype=np.float64).astype(np.float32)
    J = est.sensitivity(readings).cpu().numpy()
    got = est.linear_spread(readings, noise)
    assert got.shape == (S, n) and got.dtype == torch.float32
    np.testing.assert_array_equal(bits(got.cpu().numpy()), bits(pkg.linear_spread_ref(J, sigma)))
    assert torch.equal(est.linear_spread_store(store, noise), got)
    assert float(got.min()) >= 0 and float(got.max()) > 0
    # with gaps: the missing readings' columns are exactly 0, so they add nothing whatever their sigma
    Ja = est.sensitivity(readings, available=d_av).cpu().numpy()
    assert (np.transpose(Ja, (0, 2, 1))[av == 0] == 0).all()                 # [S, K, N] at the missing (s, k)
    out = torch.empty((S, n), dtype=torch.float32, device=DEV)
    assert est.linear_spread(readings, noise, available=d_av, out=out) is out
    np.testing.assert_array_equal(bits(out.cpu().numpy()), bits(pkg.linear_spread_ref(Ja, sigma)))
    loud = list(noise)
    loud[0] = 50.0                                              # sensor 0 never delivers in T.availability
    assert torch.equal(est.linear_spread(readings, loud, available=d_av), out)
    one = est.linear_spread(readings, 0.2)                      # one value for every sensor
    np.testing.assert_array_equal(bits(one.cpu().numpy()), bits(pkg.linear_spread_ref(J, np.full(len(OBS8), 0.2, dtype=np.float32))))


def test_refusals_on_the_device(pkg, oracle):
    store, model, est, d_av, _ = public_case(pkg, oracle)
    S, K, n = len(store), len(OBS8), store.nodes_per_graph
    good = torch.zeros((S, K), dtype=torch.float32, device=DEV)
    for bad in (good.cpu(), good.double(), good[:, :2], good.reshape(-1), good[:0]):
        with pytest.raises(ValueError, match="readings"):
            est.sensitivity(bad)
        with pytest.raises(ValueError, match="readings"):
            est.linear_spread(bad, 0.1)
    for bad in ([], [n], [-1]):
        with pytest.raises(ValueError, match="targets"):
            est.sensitivity(good, targets=bad)
        with pytest.raises(ValueError, match="targets"):
            est.sensitivity_map(store, targets=bad)
    with pytest.raises(ValueError, match="out must"):
        est.sensitivity(good, targets=[1, 2], out=torch.empty((S, 3, K), device=DEV))
    with pytest.raises(ValueError, match="out must"):
        est.sensitivity(good, out=torch.empty((S, n, K), dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError, match="out must"):
        est.linear_spread(good, 0.1, out=torch.empty((S, n + 1), device=DEV))
    with pytest.raises(ValueError, match="available"):
        est.sensitivity(good, available=d_av[:2])
    with pytest.raises(ValueError, match="available"):
        est.sensitivity_store(store, first=1, available=d_av)   # [count, K] is what it takes
    for kw in (dict(first=-1), dict(first=S), dict(count=0), dict(first=2, count=S - 1), dict(first=1.5)):
        for method in (est.sensitivity_store, est.sensitivity_map):
            with pytest.raises(ValueError, match="first|count"):
                method(store, **kw)
        with pytest.raises(ValueError, match="first|count"):
            est.linear_spread_store(store, 0.1, **kw)
    with pytest.raises(ValueError, match="max_scratch_bytes"):
        est.sensitivity_map(store, max_scratch_bytes=0)
    with pytest.raises(ValueError, match="noise_std"):
        est.linear_spread(good, [0.1, 0.2])
    with pytest.raises(ValueError, match="noise_std"):
        est.linear_spread(good, -1.0)
    with pytest.raises(ValueError, match="nodes per graph"):
        est.sensitivity_store(make_store(pkg, 2, 40, 47))
    raw = pkg.wdn_synth.make_snapshots(3, n, seed=1) * 12.5 + 50.0
    multi = pkg.MultiSnapshotStore([(raw, topology(pkg, n, 43))] * 2, device="cpu")
    for method in (est.sensitivity_store, est.sensitivity_map, est.influence_report):
        with pytest.raises(ValueError, match="MultiSnapshotStore"):
            method(multi)
    with pytest.raises(ValueError, match="MultiSnapshotStore"):
        est.linear_spread_store(multi, 0.1)


def test_no_read_back_no_allocation_and_one_read_back_in_the_report(pkg, oracle, monkeypatch):
    store, _, est, d_av, _ = public_case(pkg, oracle)
    n, S, K = store.nodes_per_graph, len(store), len(OBS8)
    raw = pkg.wdn_synth.make_snapshots(S, n, seed=1) * 12.5 + 50.0
    readings = raw.to(DEV)[:, OBS8].contiguous()
    targets = [7, 36, 0, 20, 11]
    out_j = torch.empty((S, len(targets), K), dtype=torch.float32, device=DEV)
    out_s = torch.empty((S, n), dtype=torch.float32, device=DEV)

    def passes():
        a = est.sensitivity(readings, targets=targets, available=d_av, out=out_j)
        b = est.linear_spread(readings, 0.2, out=out_s)
        return a, b, est.sensitivity_map(store, targets=targets, max_scratch_bytes=2 * len(targets) * K * 4 * 4)

    first = passes()                                            # plans, buffers and scratch exist from here on
    first = (first[0].clone(), first[1].clone(), first[2].table.clone())
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
    before = torch.cuda.memory_stats(DEV)["allocation.all.allocated"]
    a, b, m = passes()
    allocated = torch.cuda.memory_stats(DEV)["allocation.all.allocated"] - before
    assert all(v == 0 for v in calls.values()), calls
    assert allocated == 1, allocated                            # the map's table, its result; the passes allocate nothing
    r = est.influence_report(m)
    assert calls == {"synchronize": 0, "item": 0, "cpu": 1, "tolist": 0, "float": 0, "stream_sync": 0, "event_sync": 0}
    monkeypatch.undo()
    assert torch.equal(a, first[0]) and torch.equal(b, first[1]) and torch.equal(m.table, first[2])
    assert np.isfinite(r["mean_abs"]).all()
