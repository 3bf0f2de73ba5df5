"""What availability costs PressureEstimator (not collected; writes profiles/estimate_available_cost.txt).

gatres_small (15 x 32), 388 nodes, bs 32, 2 048 snapshots, 20 sensors, 30 % of the readings missing.  The paths take turns in
one process (the passes among themselves in a rotating order, then the two moments kernels), ``--reps`` times each, every
repetition ending in one synchronise; medians, and the spread of the repetitions:
  (a) ``estimate_store(store)``: the launch sequence without availability (gatres_stage_observed);
  (b) ``estimate_store(store, available=...)``: gatres_stage_observed_available, S * K more bytes read per pass;
  (c) ``estimate(readings, nan_is_missing=True)``: the same launch told by NaN readings, no ``available`` array;
  (d) ``gatres_node_error_moments`` and (e) ``gatres_node_error_moments_available`` on the same two [S, N] matrices,
      ``--moment-launches`` launches back to back per repetition.
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import gnn_pressure_estimation_amd as G      # noqa: E402

NODES, PIPES, BS, S, K, MISSING = 388, 430, 32, 2048, 20, 0.3


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--moment-launches", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "estimate_available_cost.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ei = G.wdn_synth.make_wdn_topology(NODES, PIPES, seed=0)
    raw = G.wdn_synth.make_snapshots(S, NODES, seed=1) * 12.5 + 50.0
    store = G.SnapshotStore(raw, ei, device=dev)
    torch.manual_seed(0)
    model = G.GATResMeanConv(num_blocks=15, nc=32).to(dev).eval()
    sensors = sorted(int(i) for i in torch.randperm(NODES, generator=torch.Generator().manual_seed(2))[:K])
    est = G.PressureEstimator.for_store(model, store, sensors, batch_size=BS)
    available = (torch.rand((S, K), generator=torch.Generator().manual_seed(3)) >= MISSING).to(torch.uint8).to(dev)
    readings = raw.to(dev)[:, sensors].contiguous()
    readings[available == 0] = float("nan")
    out = torch.empty((S, NODES), dtype=torch.float32, device=dev)
    lib = G._native.load()
    stream = G._native.current_stream(dev)
    tables = [torch.empty((NODES, 8), dtype=torch.float64, device=dev) for _ in range(2)]
    estimates = est.estimate_store(store, available=available)

    def a():
        est.estimate_store(store, out=out)

    def b():
        est.estimate_store(store, out=out, available=available)

    def c():
        est.estimate(readings, out=out, nan_is_missing=True)

    def d():
        for _ in range(args.moment_launches):
            lib.gatres_node_error_moments(estimates.data_ptr(), store.data.data_ptr(), S, NODES, est.scale, est.offset,
                                          est._observed.data_ptr(), K, tables[0].data_ptr(), stream)

    def e():
        for _ in range(args.moment_launches):
            lib.gatres_node_error_moments_available(estimates.data_ptr(), store.data.data_ptr(), S, NODES, est.scale, est.offset,
                                                    est._observed.data_ptr(), K, available.data_ptr(), tables[1].data_ptr(),
                                                    stream)

    paths = {"a estimate_store": a, "b estimate_store, available": b, "c estimate, nan_is_missing": c,
             "d moments": d, "e moments, available": e}
    times = {k: [] for k in paths}
    for fn in paths.values():                                       # warm-up: plans, buffers, code objects
        fn(); fn()
    torch.cuda.synchronize()
    names = list(paths)
    for group in (names[:3], names[3:]):                            # the passes among themselves, then the moments kernels
        for rep in range(args.reps):
            for i in range(len(group)):                             # (the order rotates: no path always follows the same one)
                name = group[(i + rep) % len(group)]
                t0 = time.perf_counter()
                paths[name]()
                torch.cuda.synchronize()
                times[name].append(time.perf_counter() - t0)
    b()
    with_available = out.clone()
    c()
    same = torch.equal(out, with_available)
    batches = (S + BS - 1) // BS
    med = {k: statistics.median(v) for k, v in times.items()}
    lines = ["Cost of availability in PressureEstimator (tests/micro/estimate_available_cost.py)",
             "=" * 96,
             f"MEASURED on {torch.cuda.get_device_name(0)}, torch {torch.__version__}; gatres_small (15 x 32), {NODES} nodes, bs {BS}, "
             f"{S} snapshots, {K} sensors,",
             f"{1.0 - float(available.float().mean()):.1%} of the readings missing; {args.reps} repetitions per path, the paths "
             "taking turns in one process, one synchronise per repetition.", ""]
    for name in list(paths)[:3]:
        ts = times[name]
        lines.append(f"  ({name}): median {S / med[name] / 1e3:8.1f} k graphs/s  ({med[name] * 1e3 / batches:.4f} ms per batch; "
                     f"min {min(ts) * 1e3:.3f} / max {max(ts) * 1e3:.3f} ms per pass)")
    for name in list(paths)[3:]:
        ts = [t / args.moment_launches * 1e6 for t in times[name]]
        lines.append(f"  ({name}): median {statistics.median(ts):8.2f} us per launch, {args.moment_launches} launches back to back "
                     f"(min {min(ts):.2f} / max {max(ts):.2f})")
    ka, kb, kc, kd, ke = list(paths)
    spread_a = (max(times[ka]) - min(times[ka])) * 1e6 / batches
    lines.append("")
    for name, base, unit, per in ((kb, ka, "us per batch", batches), (kc, ka, "us per batch", batches),
                                  (ke, kd, "us per launch", args.moment_launches)):
        paired = sorted((x - y) * 1e6 / per for x, y in zip(times[name], times[base]))      # (repetition by repetition)
        lines.append(f"  ({name}) - ({base}): median {statistics.median(paired):+.3f} {unit} "
                     f"(repetitions: {paired[0]:+.3f} .. {paired[-1]:+.3f})")
    lines += [f"  spread of (a) itself over its repetitions (max - min): {spread_a:.3f} us per batch",
              f"  estimates of (b) and (c) bit-identical: {same}",
              f"  bytes the staging launch reads more per pass: {S * K} (available) of {S * NODES * 4} the pass writes"]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
