"""What PressureEstimator's screening of sensor readings costs (not collected; writes profiles/screening_cost.txt).

gatres_small (15 x 32), 388 nodes, bs 32, 20 sensors, ``--snapshots`` snapshots (2 048).  The paths take turns in one process,
``--reps`` times each, every repetition ending in one synchronise; medians and ranges:
  (a) ``PressureEstimator.loo_residuals_store``: the S * K (snapshot, left-out sensor) pairs as one pass, three launches per batch;
  (b) ``reading_residuals`` on the same data: K passes of S snapshots, each writing an [S, N] estimate matrix of which one column
      is read, and torch element passes per column.  Both run the same S * K forwards;
  (c) the two new launches alone, back to back: one ``gatres_loo_residuals`` per batch of (a), one ``gatres_screen_reject``;
  (d) ``estimate_screened`` with ``max_reject`` 1 and 2 beside plain ``estimate``, for one snapshot and for all of them.
The one condition: (a) is not slower than (b) by more than (b)'s own range over its repetitions."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import gnn_pressure_estimation_amd as G      # noqa: E402

NODES, PIPES, BS, K = 388, 430, 32, 20


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--snapshots", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "screening_cost.txt"))
    args = ap.parse_args()
    S = args.snapshots
    dev = torch.device("cuda:0")
    ei = G.wdn_synth.make_wdn_topology(NODES, PIPES, seed=0)
    raw = G.wdn_synth.make_snapshots(S, NODES, seed=1) * 12.5 + 50.0
    store = G.SnapshotStore(raw, ei, device=dev)
    torch.manual_seed(0)
    model = G.GATResMeanConv(num_blocks=15, nc=32).to(dev).eval()
    sensors = sorted(int(i) for i in torch.randperm(NODES, generator=torch.Generator().manual_seed(2))[:K])
    est = G.PressureEstimator.for_store(model, store, sensors, batch_size=BS)
    readings = store.descale(store.data[:, sensors]).contiguous()
    pairs = S * K
    batches = (pairs + BS - 1) // BS
    never = G.ErrorBounds((0.9,), torch.full((1, NODES), float("inf"), device=dev),
                          torch.ones(NODES, dtype=torch.float64, device=dev), sensors)
    sb = est.calibrate_screening(store, (0.99,))
    sb.inverse                                                      # (the one read-back of the bounds, before anything is timed)
    out = torch.empty((S, NODES), dtype=torch.float32, device=dev)
    out1 = torch.empty((1, NODES), dtype=torch.float32, device=dev)
    pred, resid = (torch.empty((S, K), dtype=torch.float32, device=dev) for _ in range(2))
    avail = torch.ones((S, K), dtype=torch.uint8, device=dev)
    rejected = torch.empty((S, 1), dtype=torch.int32, device=dev)
    lib = G._native.load()
    stream = G._native.current_stream(dev)
    bound, inv = sb.bounds[0], sb.inverse[0]

    def a():
        est.loo_residuals_store(store)

    def b():
        est.reading_residuals(readings, never)

    def c():
        for first in range(0, pairs, BS):
            g = min(BS, pairs - first)
            P = G.evaluation._eval_plan(model, store, g)
            G._native.check(lib.gatres_loo_residuals(
                P.out.data_ptr(), P.mask.data_ptr(), store.data.data_ptr(), 0, S, first, NODES, g, est._observed.data_ptr(), K,
                est.scale, est.offset, None, 0, pred.data_ptr(), resid.data_ptr(), stream), "gatres_loo_residuals")
        G._native.check(lib.gatres_screen_reject(resid.data_ptr(), bound.data_ptr(), inv.data_ptr(), avail.data_ptr(), S, K, 1, 0, 1,
                                                 rejected.data_ptr(), None, stream), "gatres_screen_reject")

    paths = {"a loo_residuals_store": a, "b reading_residuals": b, "c the two new launches alone": c,
             "d estimate, all snapshots": lambda: est.estimate(readings, out),
             "d estimate_screened max_reject 1, all snapshots": lambda: est.estimate_screened(readings, sb, out=out, max_reject=1),
             "d estimate_screened max_reject 2, all snapshots": lambda: est.estimate_screened(readings, sb, out=out, max_reject=2),
             "d estimate, one snapshot": lambda: est.estimate(readings[:1], out1),
             "d estimate_screened max_reject 1, one snapshot": lambda: est.estimate_screened(readings[:1], sb, out=out1, max_reject=1),
             "d estimate_screened max_reject 2, one snapshot": lambda: est.estimate_screened(readings[:1], sb, out=out1, max_reject=2)}
    times = {k: [] for k in paths}
    for fn in paths.values():                                       # warm-up: plans, scratch, code objects
        fn(); fn()
    torch.cuda.synchronize()
    for _ in range(args.reps):
        for name, fn in paths.items():
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    want, _ = est.reading_residuals(readings, never)
    got, _ = est.loo_residuals(readings)
    same = torch.equal(got, want)
    lines = ["Cost of PressureEstimator's screening of sensor readings (tests/micro/screening_cost.py)",
             "=" * 96,
             f"MEASURED on {torch.cuda.get_device_name(0)}, torch {torch.__version__}; gatres_small (15 x 32), {NODES} nodes, bs {BS}, "
             f"{K} sensors,",
             f"{S} snapshots = {pairs} (snapshot, left-out sensor) pairs = {batches} batches; {args.reps} repetitions per path, the paths",
             "taking turns in one process, one synchronise per repetition.", ""]
    med = {}
    for name, ts in times.items():
        med[name] = statistics.median(ts)
        lines.append(f"  ({name}): median {med[name] * 1e3:9.3f} ms  (min {min(ts) * 1e3:.3f} / max {max(ts) * 1e3:.3f} ms)")
    ma, mb, mc = (med[k] for k in list(paths)[:3])
    tb = times["b reading_residuals"]
    spread_b = max(tb) - min(tb)
    holds = ma - mb <= spread_b
    lines += ["",
              f"  (a) the pass:  {ma * 1e6 / pairs:7.2f} us per pair, {ma * 1e3 / batches:.4f} ms per batch",
              f"  (b) K passes:  {mb * 1e6 / pairs:7.2f} us per pair, {mb * 1e3 / batches:.4f} ms per forward",
              f"  (a) - (b) = {(ma - mb) * 1e3:+.3f} ms ({(ma / mb - 1) * 100:+.2f} %); (b)'s range over its repetitions: {spread_b * 1e3:.3f} ms "
              f"({min(tb) * 1e3:.3f} .. {max(tb) * 1e3:.3f} ms)",
              f"  CONDITION (a) is not slower than (b) by more than (b)'s own range: {'HOLDS' if holds else 'VIOLATED'}",
              f"  residuals of loo_residuals and reading_residuals bit-identical: {same}",
              f"  (c) the two new launches: {mc * 1e3:.3f} ms for {batches} + 1 launches, {mc / ma * 100:.1f} % of the pass"]
    for scope in ("all snapshots", "one snapshot"):
        e0 = med[f"d estimate, {scope}"]
        e1, e2 = med[f"d estimate_screened max_reject 1, {scope}"], med[f"d estimate_screened max_reject 2, {scope}"]
        lines.append(f"  (d) {scope}: estimate {e0 * 1e3:.3f} ms; screened with max_reject 1 {e1 * 1e3:.3f} ms ({e1 / e0:.1f} x), with "
                     f"max_reject 2 {e2 * 1e3:.3f} ms ({e2 / e0:.1f} x)")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
