"""What calibrated error bounds cost (not collected; writes profiles/bounds_cost.txt).

gatres_small (15 x 32), 388 nodes, bs 32, 20 sensors, Q = 3 levels, S = 2 048 and 8 192 snapshots.  The paths take turns in one
process (a rotating order inside each group), ``--reps`` times each, every repetition ending in one synchronise; medians and the
range of the repetitions:
  (a) ``gatres_node_error_quantiles`` on the estimate and truth matrices, ``--launches`` launches back to back;
  (b) the torch statement of the same result on the same device matrices: ``(est - D(truth)).abs().sort(dim=0)`` and a gather of
      the ranks -- what a user writes without the launch; as many times back to back;
  (c) ``calibrate_bounds(store, levels)`` end to end beside the ``estimate_store(store)`` pass it contains;
  (d) ``gatres_node_bound_coverage`` beside ``gatres_node_error_moments`` on the same matrices.
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import gnn_pressure_estimation_amd as G      # noqa: E402

NODES, PIPES, BS, K = 388, 430, 32, 20
LEVELS = (0.5, 0.9, 0.95)
SIZES = (2048, 8192)


def measure(paths, groups, reps):
    times = {k: [] for k in paths}
    for fn in paths.values():                                       # warm-up: plans, buffers, code objects
        fn(); fn()
    torch.cuda.synchronize()
    for group in groups:
        for rep in range(reps):
            for i in range(len(group)):                             # (the order rotates: no path always follows the same one)
                name = group[(i + rep) % len(group)]
                t0 = time.perf_counter()
                paths[name]()
                torch.cuda.synchronize()
                times[name].append(time.perf_counter() - t0)
    return times


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bounds_cost.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ei = G.wdn_synth.make_wdn_topology(NODES, PIPES, seed=0)
    torch.manual_seed(0)
    model = G.GATResMeanConv(num_blocks=15, nc=32).to(dev).eval()
    sensors = sorted(int(i) for i in torch.randperm(NODES, generator=torch.Generator().manual_seed(2))[:K])
    lib = G._native.load()
    stream = G._native.current_stream(dev)
    Q, L = len(LEVELS), args.launches
    lv = (ctypes.c_double * Q)(*LEVELS)
    lines = ["Cost of calibrated error bounds (tests/micro/bounds_cost.py)",
             "=" * 96,
             f"MEASURED on {torch.cuda.get_device_name(0)}, torch {torch.__version__}; gatres_small (15 x 32), {NODES} nodes, bs {BS}, "
             f"{K} sensors, levels {LEVELS};",
             f"{args.reps} repetitions per path, the paths taking turns in one process, one synchronise per repetition; (a), (b) and "
             f"(d) as {L} launches back to back.", ""]
    for S in SIZES:
        raw = G.wdn_synth.make_snapshots(S, NODES, seed=1) * 12.5 + 50.0
        store = G.SnapshotStore(raw, ei, device=dev)
        est = G.PressureEstimator.for_store(model, store, sensors, batch_size=BS)
        p = est.estimate_store(store)
        truth = store.data
        bounds = torch.empty((Q, NODES), dtype=torch.float32, device=dev)
        counts = torch.empty((NODES,), dtype=torch.float64, device=dev)
        table9 = torch.empty((NODES, G.estimation.NODE_COVERAGE_RECORD), dtype=torch.float64, device=dev)
        table8 = torch.empty((NODES, 8), dtype=torch.float64, device=dev)
        out = torch.empty_like(p)
        ranks = torch.from_numpy(np.array([G.conformal_rank(S, q) for q in LEVELS]).astype(np.int64) - 1).to(dev)
        torch_bounds = [None]

        def a():
            for _ in range(L):
                lib.gatres_node_error_quantiles(p.data_ptr(), truth.data_ptr(), S, NODES, est.scale, est.offset, None, 0, None, lv, Q,
                                                bounds.data_ptr(), counts.data_ptr(), stream)

        def b():
            for _ in range(L):
                torch_bounds[0] = (p - store.descale(truth)).abs().sort(dim=0).values.index_select(0, ranks)

        def c():
            est.calibrate_bounds(store, LEVELS)

        def c0():
            est.estimate_store(store, out=out)

        def d():
            for _ in range(L):
                lib.gatres_node_bound_coverage(p.data_ptr(), truth.data_ptr(), S, NODES, est.scale, est.offset, None, 0, None,
                                               bounds.data_ptr(), Q, table9.data_ptr(), stream)

        def d0():
            for _ in range(L):
                lib.gatres_node_error_moments(p.data_ptr(), truth.data_ptr(), S, NODES, est.scale, est.offset,
                                              est._observed.data_ptr(), K, table8.data_ptr(), stream)

        paths = {"a quantiles launch": a, "b torch sort + gather": b, "c calibrate_bounds": c, "c0 estimate_store": c0,
                 "d coverage launch": d, "d0 moments launch": d0}
        names = list(paths)
        times = measure(paths, (names[:2], names[2:4], names[4:]), args.reps)
        a(); b()
        torch.cuda.synchronize()
        same = torch.equal(bounds.view(torch.int32), torch_bounds[0].view(torch.int32))
        lines.append(f"S = {S}  (est and truth together {2 * 4 * S * NODES / 1e6:.2f} MB; the select reads them in each of its 4 passes: "
                     f"{4 * 2 * 4 * S * NODES / 1e6:.1f} MB per launch)")
        us = {}
        for name in names:
            per = 1 if name.startswith("c") else L
            ts = [t / per * 1e6 for t in times[name]]
            us[name] = (statistics.median(ts), min(ts), max(ts))
            unit = "us per call" if per == 1 else "us per launch"
            lines.append(f"  ({name}): median {us[name][0]:10.2f} {unit}  (min {us[name][1]:.2f} / max {us[name][2]:.2f})")
        (ma, _, _), (mb, lo_b, hi_b) = us[names[0]], us[names[1]]
        verdict = "holds" if ma <= mb + (hi_b - lo_b) else "FAILS"
        lines += [f"  (a) / (b) = {ma / mb:.3f}  ((b) / (a) = {mb / ma:.2f} x); range of (b) over its repetitions {hi_b - lo_b:.2f} us: "
                  f"the condition '(a) no slower than (b) beyond (b)'s own range' {verdict}",
                  f"  bounds of (a) and (b) bit-identical: {same}",
                  f"  (c) - (c0) = {us[names[2]][0] - us[names[3]][0]:+.1f} us per call, {us[names[2]][0] / us[names[3]][0] - 1.0:+.2%} of "
                  f"the pass",
                  f"  (d) / (d0) = {us[names[4]][0] / us[names[5]][0]:.3f}", ""]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
