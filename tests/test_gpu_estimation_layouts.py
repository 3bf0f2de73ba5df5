"""Scoring sensor layouts and placing sensors on the device (``layout_errors`` / ``place_sensors`` of
estimation.PressureEstimator; gatres_stage_observed_layouts, gatres_layout_pair_errors and gatres_layout_error_reduce of
k_estimate.hip): the staging bit for bit against torch, the pair errors and the reduce against numpy restatements, the pass
against itself written out and against the existing public calls, the placement against greedy selection written out with
those calls, and the read-backs.

Shapes: 37 nodes (no multiple of 4) and 40 nodes (whole chunks, the vector paths) with K = 5 candidate sensors and L = 6 layouts
over S = 5 snapshots at batch size 4 -- the 30 pairs fall as seven batches of 4 and one of 2, and batches straddle snapshots --;
one launch of two graphs of 1 030 nodes with sensors on both sides of the staging kernel's tile boundary at node 1 024; 388 nodes
once, for gatres_small at batch size 32 on the window kernel."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from estimation_refs import check_records, numpy_fold, numpy_pair_errors      # noqa: E402
from test_gpu_estimation import DEV, N37, garbage, make_store, raw_snapshots, small_model, stream, topology      # noqa: E402
from test_gpu_estimation_noise import OBS40, avail, torch_stage_available      # noqa: E402

S5, L6, BS4 = 5, 6, 4
OBS37 = [36, 0, 5, 17, 20]                        # unsorted: column k of the layouts is node OBS37[k]
# [L6, 5]: no sensor, every sensor, three mixed rows and a copy of the first of them
LAYOUTS = [[0, 0, 0, 0, 0], [1, 1, 1, 1, 1], [1, 0, 1, 0, 0], [0, 1, 0, 0, 1], [0, 0, 1, 1, 0], [1, 0, 1, 0, 0]]
# [S5, 5]: a snapshot with every reading, one with none, mixed rows
AVAIL = [[1, 1, 1, 1, 1], [0, 0, 0, 0, 0], [1, 0, 1, 1, 0], [0, 1, 1, 0, 1], [1, 1, 0, 1, 1]]


def observed_of(n):
    return OBS37 if n == N37 else OBS40


def effective(layouts, available, S):
    """[S * L, K]: what pair p = s * L + l may read -- layouts[l] & available[s] (``available`` None: everything)."""
    lay = torch.as_tensor(layouts, dtype=torch.uint8, device=DEV)
    L = lay.shape[0]
    av = torch.ones((S, lay.shape[1]), dtype=torch.uint8, device=DEV) if available is None else available.to(torch.uint8)
    return (lay.unsqueeze(0) & (av != 0).to(torch.uint8).unsqueeze(1)).reshape(S * L, -1)


def stage_layouts(pkg, lib, src, layout, first_pair, layouts, n, g, observed, available=None, nan_is_missing=0, normalise=0,
                  offset=0.0, factor=1.0, target=None):
    """One gatres_stage_observed_layouts launch into a garbage-filled target (``target``: the two addresses to write to
    instead).  Returns the target."""
    x, mask = garbage(g * n)
    xp, mp = (x.data_ptr(), mask.data_ptr()) if target is None else target
    obs = torch.tensor(observed, dtype=torch.int32, device=DEV)
    lay = torch.as_tensor(layouts, dtype=torch.uint8, device=DEV).contiguous()
    assert lay.shape[1] == len(observed)
    pkg._native.check(lib.gatres_stage_observed_layouts(
        src.data_ptr(), layout, src.shape[0], first_pair, lay.shape[0], n, g, obs.data_ptr(), len(observed), normalise, offset,
        factor, xp, mp, pkg._native.ptr(available), nan_is_missing, lay.data_ptr(), stream()), "gatres_stage_observed_layouts")
    return x, mask


# ---- 1. staging -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [N37, 40], ids=["n37", "n40"])
@pytest.mark.parametrize("normalize", [True, False], ids=["znorm", "unused"])
def test_layout_staging_bitwise_in_both_layouts(pkg, lib, oracle, n, normalize):
    observed = observed_of(n)
    raw = raw_snapshots(pkg, S5, n)
    store = pkg.SnapshotStore(raw, topology(pkg, n, 41 if n == N37 else 45), device=DEV, normalize=normalize)
    model, _ = small_model(pkg, oracle)
    est = pkg.PressureEstimator.for_store(model, store, observed, batch_size=BS4)
    readings = raw.to(DEV)[:, observed].contiguous()
    norm = (est._normalise, store.mean if normalize else 0.0, store.std + 1e-8 if normalize else 1.0)
    av = avail(AVAIL)
    row_of = torch.arange(S5 * L6, device=DEV) // L6
    values = store.data[:, observed][row_of]                        # [S * L, K]: the pair's staged sensor values
    batches = [(first, min(BS4, S5 * L6 - first)) for first in range(0, S5 * L6, BS4)]
    assert [g for _, g in batches] == [4] * 7 + [2]
    for available in (av, None):
        eff = effective(LAYOUTS, available, S5)
        for first, g in batches:
            sl = slice(first, first + g)
            ex, em = torch_stage_available(values[sl], n, observed, eff[sl])
            x, mask = stage_layouts(pkg, lib, store.data, 0, first, LAYOUTS, n, g, observed, available)
            assert torch.equal(x, ex) and torch.equal(mask, em), first
            x, mask = stage_layouts(pkg, lib, readings, 1, first, LAYOUTS, n, g, observed, available, 0, *norm)
            assert torch.equal(x, ex) and torch.equal(mask, em), first
    # the whole pass in one launch; the empty layout hides everything, the full one is gatres_stage_observed_available's
    x, mask = stage_layouts(pkg, lib, store.data, 0, 0, LAYOUTS, n, S5 * L6, observed, av)
    ex, em = torch_stage_available(values, n, observed, effective(LAYOUTS, av, S5))
    assert torch.equal(x, ex) and torch.equal(mask, em)
    x, mask = x.view(S5, L6, n), mask.view(S5, L6, n)
    assert (x[:, 0] == 0).all() and (mask[:, 0] == 1).all() and torch.equal(x[:, 2], x[:, 5]) and torch.equal(mask[:, 2], mask[:, 5])
    ax, am = garbage(S5 * n)
    obs = torch.tensor(observed, dtype=torch.int32, device=DEV)
    pkg._native.check(lib.gatres_stage_observed_available(store.data.data_ptr(), 0, S5, None, 0, n, S5, obs.data_ptr(), len(observed),
                                                          0, 0.0, 1.0, ax.data_ptr(), am.data_ptr(), av.data_ptr(), 0, stream()),
                      "gatres_stage_observed_available")
    assert torch.equal(x[:, 1].reshape(-1), ax) and torch.equal(mask[:, 1].reshape(-1), am)
    # gaps told by NaN readings: the same staging as with available
    nan_readings = torch.where(av.bool(), readings, torch.full_like(readings, float("nan")))
    eff = effective(LAYOUTS, av, S5)
    for first, g in ((8, 4), (28, 2)):
        ex, em = torch_stage_available(values[first:first + g], n, observed, eff[first:first + g])
        x, mask = stage_layouts(pkg, lib, nan_readings, 1, first, LAYOUTS, n, g, observed, None, 1, *norm)
        assert torch.equal(x, ex) and torch.equal(mask, em) and torch.isfinite(x).all(), first


def test_layout_staging_on_an_unaligned_target(pkg, lib):
    """A target one float past a 16-byte boundary takes the element-by-element stores; nothing is written outside the batch."""
    g, first = 3, 5
    store = make_store(pkg, S5)
    av = avail(AVAIL)
    xb, mb = garbage(g * N37 + 4)
    stage_layouts(pkg, lib, store.data, 0, first, LAYOUTS, N37, g, OBS37, av, target=(xb.data_ptr() + 4, mb.data_ptr() + 1))
    row_of = torch.arange(S5 * L6, device=DEV) // L6
    ex, em = torch_stage_available(store.data[:, OBS37][row_of][first:first + g], N37, OBS37,
                                   effective(LAYOUTS, av, S5)[first:first + g])
    assert torch.equal(xb[1:1 + g * N37], ex) and torch.equal(mb[1:1 + g * N37], em)
    assert torch.isnan(xb[0]) and torch.isnan(xb[1 + g * N37:]).all() and int(mb[0]) == 0xAB and (mb[1 + g * N37:] == 0xAB).all()


def test_layout_staging_across_the_tile_boundary(pkg, lib):
    """Two graphs of 1 030 nodes: the staging kernel's second workgroup column starts at node 1 020 + shift."""
    n, observed = 1030, [1023, 1024, 1029]
    layouts = [[1, 0, 1], [0, 1, 1], [1, 1, 0]]
    src = torch.randn((2, n), generator=torch.Generator().manual_seed(5)).to(DEV)
    row_of = torch.arange(2 * 3, device=DEV) // 3
    values, eff = src[:, observed][row_of], effective(layouts, None, 2)
    for first, g in ((2, 2), (0, 2), (4, 2)):                       # (pairs 2, 3 straddle the two source rows)
        x, mask = stage_layouts(pkg, lib, src, 0, first, layouts, n, g, observed)
        ex, em = torch_stage_available(values[first:first + g], n, observed, eff[first:first + g])
        assert torch.equal(x, ex) and torch.equal(mask, em), first
        assert int((mask == 0).sum()) == 2 * g                      # two installed sensors in every layout


# ---- 2. pair errors ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [N37, 40], ids=["odd", "vector"])
@pytest.mark.parametrize("scored", [False, True], ids=["every_node", "score"])
def test_pair_errors_against_numpy(pkg, lib, n, scored):
    G, rows, L, first_pair, rec_rows, rec_first = 5, 5, 3, 7, 9, 2   # five graphs: two workgroups; truth rows 2, 2, 3, 3, 3
    scale, offset = 12.81, 51.37
    gen = torch.Generator().manual_seed(10 * n + scored)
    out = torch.randn((G, n), generator=gen).to(DEV)
    truth = torch.randn((rows, n), generator=gen).to(DEV)
    mask = (torch.rand((G, n), generator=gen) < 0.7).to(torch.uint8)
    mask[3] = 0                                                     # a graph with nothing counted
    mask = mask.to(DEV)
    score = None
    if scored:
        score = (torch.rand(n, generator=gen) < 0.5).to(torch.uint8)
        score[n - 1] = 1
        score = score.to(DEV)

    def launch(o=out, m=mask):
        rec = torch.full((rec_rows, 4), -777.25, dtype=torch.float64, device=DEV)
        pkg._native.check(lib.gatres_layout_pair_errors(
            o.data_ptr(), m.data_ptr(), truth.data_ptr(), rows, n, G, first_pair, L, scale, offset, pkg._native.ptr(score),
            rec.data_ptr(), rec_rows, rec_first, stream()), "gatres_layout_pair_errors")
        return rec.cpu().numpy()

    rec = launch()
    assert rec.tobytes() == launch().tobytes()                     # the same bits every run
    s = (first_pair + np.arange(G)) // L
    want = numpy_pair_errors(out.cpu().numpy(), mask.cpu().numpy(), truth.cpu().numpy()[s], scale, offset,
                             None if score is None else score.cpu().numpy())
    got = rec[rec_first:rec_first + G]
    check_records(got, want, n)
    assert got[3].tolist() == [0.0, 0.0, 0.0, 0.0] and (got[[0, 1, 2, 4], 0] > 0).all()
    assert (np.delete(rec, np.s_[rec_first:rec_first + G], axis=0) == -777.25).all()       # the neighbouring records
    # buffers one element past a 16-byte boundary take the element loads: the same additions in the same order
    ob = torch.empty(G * n + 1, dtype=torch.float32, device=DEV)
    mb = torch.empty(G * n + 1, dtype=torch.uint8, device=DEV)
    ob[1:] = out.reshape(-1)
    mb[1:] = mask.reshape(-1)
    assert launch(ob[1:], mb[1:]).tobytes() == rec.tobytes()


# ---- 3. the reduce ----------------------------------------------------------------------------------------------------------------
def synthetic_records(S, L, seed):
    gen = torch.Generator().manual_seed(seed)
    rec = torch.rand((S * L, 4), generator=gen, dtype=torch.float64) * 3.0 + 0.1
    rec[:, 0] = torch.randint(0, 40, (S * L,), generator=gen).double()
    rec[L + 1] = 0.0                                                # a pair with nothing counted
    return rec.to(DEV)


def fold(pkg, lib, rec, S, L, table, accumulate):
    pkg._native.check(lib.gatres_layout_error_reduce(rec.data_ptr(), S, L, table.data_ptr(), accumulate, stream()),
                      "gatres_layout_error_reduce")


@pytest.mark.parametrize("S,L", [(S5, L6), (3, 130)], ids=["S5_L6", "more_than_two_waves"])
def test_layout_error_reduce_bitwise(pkg, lib, S, L):
    rec = synthetic_records(S, L, 100 * S + L)
    want = numpy_fold(rec.cpu().numpy(), S, L)
    table = torch.full((L + 1, 4), float("nan"), dtype=torch.float64, device=DEV)      # (garbage: accumulate = 0 starts from zero)
    fold(pkg, lib, rec, S, L, table, 0)
    assert table[:L].cpu().numpy().tobytes() == want.tobytes()
    assert torch.isnan(table[L]).all()                              # nothing past the table
    if S < 5:
        return
    # the same pass cut into 3 + 2 snapshots: the same bits
    two = torch.full((L, 4), float("nan"), dtype=torch.float64, device=DEV)
    fold(pkg, lib, rec[:3 * L], 3, L, two, 0)
    assert two.cpu().numpy().tobytes() == numpy_fold(rec[:3 * L].cpu().numpy(), 3, L).tobytes()
    fold(pkg, lib, rec[3 * L:], 2, L, two, 1)
    assert two.cpu().numpy().tobytes() == want.tobytes()


# ---- 4. the pass --------------------------------------------------------------------------------------------------------------------
def layouts_hand_loop(pkg, model, store, observed, bs, layouts, available=None, score=None):
    """``layout_errors`` written out: the pairs staged by torch, the forward through the estimator's plan and entry at the
    batch's size, the errors and the fold in numpy.  Returns (table [L, 4], batch sizes)."""
    E = pkg.evaluation
    lib = pkg._native.load()
    n, S = store.nodes_per_graph, len(store)
    L = len(layouts)
    pairs = S * L
    eff = effective(layouts, available, S)
    row_of = torch.arange(pairs, device=DEV) // L
    values = store.data[:, observed][row_of]
    truth = store.data.cpu().numpy()
    scale, offset = (store.std, store.mean) if store.norm_type == "znorm" else (1.0, 0.0)
    rec, sizes = np.zeros((pairs, 4), dtype=np.float64), []
    for first in range(0, pairs, bs):
        g = min(bs, pairs - first)
        P = E._eval_plan(model, store, g)
        x1, mask = torch_stage_available(values[first:first + g], n, observed, eff[first:first + g])
        P.x.copy_(x1)
        P.mask.copy_(mask)
        E._enqueue_forward(lib, model.flat_parameters, P, stream())
        pred = P.out.clone().reshape(g, n).cpu().numpy()
        rec[first:first + g] = numpy_pair_errors(pred, mask.view(g, n).cpu().numpy(), truth[(first + np.arange(g)) // L], scale,
                                                 offset, score)
        sizes.append(g)
    return numpy_fold(rec, S, L), sizes


@pytest.mark.parametrize("kind", ["fused", "per_op", "bf16"])
def test_layout_errors_equal_the_pass_written_out(pkg, oracle, kind):
    store = make_store(pkg, S5)
    model, _ = small_model(pkg, oracle, fused=kind != "per_op") if kind != "bf16" else small_model(pkg, oracle, nb=2, nc=32, dtype="bf16")
    est = pkg.PressureEstimator.for_store(model, store, OBS37, batch_size=BS4)
    lay, av = avail(LAYOUTS), avail(AVAIL)
    want, sizes = layouts_hand_loop(pkg, model, store, OBS37, BS4, LAYOUTS, av)
    assert sizes == [4] * 7 + [2]
    table = est.layout_errors(store, lay, available=av)
    assert table.shape == (L6, pkg.estimation.LAYOUT_ERROR_RECORD) and table.dtype == torch.float64 and table.device.type == "cuda"
    got = table.cpu().numpy()
    check_records(got, want, N37 + S5)
    # what is scored: the hidden entries.  Per snapshot N37 - (installed sensors with a reading)
    hidden = S5 * N37 - (np.asarray(LAYOUTS)[:, None, :] & np.asarray(AVAIL)[None, :, :]).sum(axis=(1, 2))
    np.testing.assert_array_equal(got[:, 0], hidden)
    assert got[2].tobytes() == got[5].tobytes() and (got[:, 3] > 0).all()           # the duplicate layout: the same bits
    # the budget changes the chunks (2, 2 and 1 snapshots; everything), not the batches: the same bits
    assert pkg.estimation.ensemble_chunk(S5, L6, BS4, 32, 1) == 2
    assert torch.equal(est.layout_errors(store, lay, available=av, max_scratch_bytes=1), table)
    assert torch.equal(est.layout_errors(store, lay, available=av), table)          # a second run
    assert torch.equal(est.layout_errors(store, lay.bool(), available=av.bool()), table)
    out = torch.full((L6, 4), float("nan"), dtype=torch.float64, device=DEV)
    assert est.layout_errors(store, lay, available=av, out=out) is out and torch.equal(out, table)
    # without available, and with a pool
    want, _ = layouts_hand_loop(pkg, model, store, OBS37, BS4, LAYOUTS)
    check_records(est.layout_errors(store, lay).cpu().numpy(), want, N37 + S5)
    pool = [1, 2, 36, 17, 30]                                       # two candidates among them: scored where hidden
    score = np.zeros(N37, dtype=np.uint8)
    score[pool] = 1
    want, _ = layouts_hand_loop(pkg, model, store, OBS37, BS4, LAYOUTS, score=score)
    got = est.layout_errors(store, lay, score_nodes=pool).cpu().numpy()
    check_records(got, want, N37 + S5)
    assert got[:, 0].tolist() == [S5 * 5, S5 * 3, S5 * 4, S5 * 5, S5 * 4, S5 * 4]


def test_layout_errors_refusals(pkg, oracle):
    store = make_store(pkg, S5)
    model, _ = small_model(pkg, oracle)
    est = pkg.PressureEstimator.for_store(model, store, OBS37, batch_size=BS4)
    good = avail(LAYOUTS)
    for bad in (good.cpu(), good.float(), good[:, :4], good.reshape(-1), good[:0], torch.zeros((6, 10), dtype=torch.uint8, device=DEV)[:, ::2]):
        with pytest.raises(ValueError, match="layouts must"):
            est.layout_errors(store, bad)
    multi = pkg.MultiSnapshotStore.__new__(pkg.MultiSnapshotStore)
    with pytest.raises(ValueError, match="MultiSnapshotStore"):
        est.layout_errors(multi, good)
    for bad in ([37], [-1], [3, 3], []):
        with pytest.raises(ValueError, match="score_nodes"):
            est.layout_errors(store, good, score_nodes=bad)
    for bad in (torch.empty((L6, 5), dtype=torch.float64, device=DEV), torch.empty((L6, 4), device=DEV), torch.empty((L6, 4), dtype=torch.float64)):
        with pytest.raises(ValueError, match="out must"):
            est.layout_errors(store, good, out=bad)
    with pytest.raises(ValueError, match="available must"):
        est.layout_errors(store, good, available=good)
    with pytest.raises(ValueError, match="max_scratch_bytes"):
        est.layout_errors(store, good, max_scratch_bytes=0)


# ---- 5. against the existing public calls -----------------------------------------------------------------------------------------
def test_layout_errors_against_estimate_store_and_error_map(pkg, oracle):
    """Row l of the table against ``error_map(store, available=layouts[l] in every snapshot)`` pooled over the hidden entries.
    The two passes batch differently (pairs of several layouts against snapshots of one), so the predictions agree as fp32
    passes of different batch composition do here: 1e-5 of the largest estimate (check_against_module's bound), and the MAE,
    a mean of such differences, within the same."""
    store = make_store(pkg, S5)
    model, _ = small_model(pkg, oracle)
    est = pkg.PressureEstimator.for_store(model, store, OBS37, batch_size=BS4)
    scores = pkg.estimation.layout_scores_from_table(est.layout_errors(store, avail(LAYOUTS)).cpu().numpy())
    for l, row in enumerate(LAYOUTS):
        av = avail([row] * S5)
        estimate = est.estimate_store(store, available=av)
        m = est.error_map(store, estimates=estimate, available=av)
        bound = 1e-5 * float(estimate.abs().max())
        assert scores["count"][l] == m["hidden_count"].sum() == S5 * (N37 - sum(row))
        d = abs(scores["mae"][l] - m["hidden_mae"])
        print(f"layout {l}: mae {scores['mae'][l]:.6f}, error_map's {m['hidden_mae']:.6f}, |d| = {d:.3e} (bound {bound:.3e})")
        assert d <= bound
        assert abs(scores["rmse"][l] - m["hidden_rmse"]) <= bound and abs(scores["max_abs"][l] - np.nanmax(m["max_abs"])) <= bound


# ---- 6. gatres_small --------------------------------------------------------------------------------------------------------------
def test_gatres_small_at_batch_32_takes_the_window_kernel(pkg, oracle):
    n, pipes, S, L = 388, 430, 2, 16
    store = make_store(pkg, S, n=n, pipes=pipes, seed=4)
    model, _ = small_model(pkg, oracle, nb=15, nc=32, seed=11)
    plan = model.plan_for(store.edge_index(32), 32 * n)
    assert model._call_state(plan)["window"], "gatres_small at bs 32 should take the window kernel"
    sensors = [3, 17, 100, 101, 250, 387, 42, 9, 300, 77, 211, 5, 64, 128, 199, 350, 1, 260, 333, 150]
    layouts = (torch.rand((L, len(sensors)), generator=torch.Generator().manual_seed(6)) < 0.5).to(torch.uint8)
    layouts[3] = 1
    est = pkg.PressureEstimator.for_store(model, store, sensors, batch_size=32)
    want, sizes = layouts_hand_loop(pkg, model, store, sensors, 32, layouts.tolist())
    assert sizes == [32]
    got = est.layout_errors(store, layouts.to(DEV)).cpu().numpy()
    check_records(got, want, n + S)
    assert got[3, 0] == S * (n - len(sensors)) and (got[:, 3] > 0).all()


# ---- 7. placement -------------------------------------------------------------------------------------------------------------------
FIXED, CANDIDATES, PLACE = [36], [0, 5, 9, 14, 20, 23, 28, 33], 3
MODEL_SEED = 5      # (with this model and the store of seed 1 the fp32 oracle on the host separates the best candidate of every
                    #  round from the runner-up by 0.027 and more: ten times the bound below)


def written_out(est, store, installed, cache):
    """``estimate_store`` + ``error_map`` with exactly the sensors ``installed`` (positions in est.observed_idx) available."""
    key = tuple(sorted(installed))
    if key not in cache:
        row = [1 if k in installed else 0 for k in range(len(est.observed_idx))]
        av = avail([row] * len(store))
        estimate = est.estimate_store(store, available=av)
        cache[key] = (est.error_map(store, estimates=estimate, available=av), float(estimate.abs().max()))
    return cache[key]


def test_place_sensors_against_greedy_written_out(pkg, oracle):
    store = make_store(pkg, S5)
    model, _ = small_model(pkg, oracle, seed=MODEL_SEED)
    everything = FIXED + CANDIDATES
    est = pkg.PressureEstimator.for_store(model, store, everything, batch_size=BS4)
    column = {c: everything.index(c) for c in everything}
    cache, largest = {}, 0.0
    chosen, want_scores, want_rounds, remaining = [], [], [], list(CANDIDATES)
    for _ in range(PLACE):
        sc = []
        for c in remaining:
            m, top = written_out(est, store, [column[v] for v in FIXED + chosen + [c]], cache)
            sc.append(float(m["hidden_mae"]))
            largest = max(largest, top)
        want_rounds.append((list(remaining), sc))
        best = int(np.argmin(sc))                                   # (the first of equal scores)
        want_scores.append(sc[best])
        chosen.append(remaining.pop(best))
    bound = 1e-5 * largest
    for r, (_, sc) in enumerate(want_rounds):                       # the written-out loop alone: every round is decided
        first, second = sorted(sc)[:2]
        print(f"round {r}: best {first:.6f}, runner-up {second:.6f}, gap {second - first:.3e} (4 x bound = {4 * bound:.3e})")
        assert second - first > 4 * bound, r
    res = pkg.PressureEstimator.place_sensors(model, store, PLACE, candidates=CANDIDATES, fixed=FIXED, batch_size=BS4)
    assert sorted(res) == ["chosen", "observed_idx", "rounds", "scores"]
    assert res["chosen"] == chosen and res["observed_idx"] == FIXED + chosen
    print("chosen", res["chosen"], "scores", res["scores"], "written out", want_scores)
    assert len(res["scores"]) == PLACE and np.abs(np.asarray(res["scores"]) - np.asarray(want_scores)).max() <= bound
    assert len(res["rounds"]) == PLACE
    for r, (rem, sc) in enumerate(want_rounds):
        got = res["rounds"][r]
        assert got["candidates"] == rem and sorted(got) == ["candidates", "count", "mae", "max_abs", "rmse"]
        assert np.abs(got["mae"] - np.asarray(sc)).max() <= bound
        assert (got["count"] == S5 * (N37 - len(FIXED) - r - 1)).all()
        assert res["scores"][r] == got["mae"].min()
    # the result is ready for for_store
    assert pkg.PressureEstimator.for_store(model, store, res["observed_idx"]).observed_idx == FIXED + chosen
    # another criterion ranks by its own entry
    rm = pkg.PressureEstimator.place_sensors(model, store, 1, candidates=CANDIDATES, fixed=FIXED, criterion="rmse", batch_size=BS4)
    assert rm["scores"][0] == rm["rounds"][0]["rmse"].min() and rm["chosen"][0] == CANDIDATES[int(np.argmin(rm["rounds"][0]["rmse"]))]
    # an empty `fixed`: the first round scores single-sensor layouts
    one = pkg.PressureEstimator.place_sensors(model, store, 1, candidates=CANDIDATES, batch_size=BS4)
    assert one["observed_idx"] == one["chosen"] and (one["rounds"][0]["count"] == S5 * (N37 - 1)).all()
    # score_nodes: a pool disjoint from the sensors is every layout's pool.  Along the path the call took, every candidate's
    # score against the written-out pass pooled over the same nodes (each of them hidden in every snapshot)
    pool = [v for v in range(N37) if v not in everything]
    res = pkg.PressureEstimator.place_sensors(model, store, PLACE, candidates=CANDIDATES, fixed=FIXED, score_nodes=pool, batch_size=BS4)
    for r, got in enumerate(res["rounds"]):
        assert (got["count"] == S5 * len(pool)).all()
        for i, c in enumerate(got["candidates"]):
            m, _ = written_out(est, store, [column[v] for v in FIXED + res["chosen"][:r] + [c]], cache)
            assert (m["hidden_count"][pool] == S5).all()
            assert abs(got["mae"][i] - m["mae"][pool].mean()) <= bound, (r, c)
    assert res["observed_idx"] == FIXED + res["chosen"] and len(set(res["chosen"])) == PLACE


# ---- 8. read-backs ------------------------------------------------------------------------------------------------------------------
def test_no_read_back_in_layout_errors_and_one_per_round_in_place_sensors(pkg, oracle, monkeypatch):
    store = make_store(pkg, S5)
    model, _ = small_model(pkg, oracle, seed=MODEL_SEED)
    est = pkg.PressureEstimator.for_store(model, store, OBS37, batch_size=BS4)
    lay, av = avail(LAYOUTS), avail(AVAIL)

    def place():
        return pkg.PressureEstimator.place_sensors(model, store, PLACE, candidates=CANDIDATES, fixed=FIXED, batch_size=BS4)

    first = est.layout_errors(store, lay, available=av, score_nodes=[1, 2, 3])      # plans (4, 3 and 2 graphs) and buffers exist
    want = place()                                                                  # from here on
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
    a = est.layout_errors(store, lay, available=av, score_nodes=[1, 2, 3])
    b = est.layout_errors(store, lay, available=av, score_nodes=[1, 2, 3], max_scratch_bytes=1)
    c = est.layout_errors(store, lay)
    assert all(v == 0 for v in calls.values()), calls
    got = place()
    assert calls == {"synchronize": 0, "item": 0, "cpu": PLACE, "tolist": 0, "float": 0, "stream_sync": 0, "event_sync": 0}
    monkeypatch.undo()
    assert torch.equal(a, first) and torch.equal(a, b) and torch.isfinite(c).all()
    assert got["chosen"] == want["chosen"] and got["scores"] == want["scores"]
