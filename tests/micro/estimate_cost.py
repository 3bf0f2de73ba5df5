"""What PressureEstimator's two launches per batch cost (not collected; writes profiles/estimate_cost.txt).

gatres_small (15 x 32), 388 nodes, bs 32, 2 048 snapshots, 20 sensors.  Three paths take turns in one process, ``--reps``
times each, every repetition ending in one synchronise; medians in graphs/s:
  (a) ``PressureEstimator.estimate_store``: staging + forward + write-back, three launches per batch;
  (b) the hand-written torch loop through the module: zeros, index_put, ``model(x1, edge_index)``, ``torch.where``, ``descale``;
  (c) the bare forward on a staged batch, 64 times over (what ``bench.py --eval`` times).
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

NODES, PIPES, BS, S, K = 388, 430, 32, 2048, 20


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "estimate_cost.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ei = G.wdn_synth.make_wdn_topology(NODES, PIPES, seed=0)
    store = G.SnapshotStore(G.wdn_synth.make_snapshots(S, NODES, seed=1) * 12.5 + 50.0, ei, device=dev)
    torch.manual_seed(0)
    model = G.GATResMeanConv(num_blocks=15, nc=32).to(dev).eval()
    sensors = sorted(int(i) for i in torch.randperm(NODES, generator=torch.Generator().manual_seed(2))[:K])
    est = G.PressureEstimator.for_store(model, store, sensors, batch_size=BS)
    obs = torch.tensor(sensors, device=dev)
    out = torch.empty((S, NODES), dtype=torch.float32, device=dev)
    lib = G._native.load()
    P = G.evaluation._eval_plan(model, store, BS)
    stream = G._native.current_stream(dev)

    def a():
        est.estimate_store(store, out=out)

    def b():
        with torch.no_grad():
            for first in range(0, S, BS):
                rows = store.data[first:first + BS]
                x1 = torch.zeros_like(rows)
                x1[:, obs] = rows[:, obs]
                pred = model(x1.view(-1, 1), store.edge_index(BS)).view(BS, NODES)
                mask = torch.ones_like(rows, dtype=torch.bool)
                mask[:, obs] = False
                out[first:first + BS] = torch.where(mask, store.descale(pred), store.descale(x1))

    def c():
        for _ in range(S // BS):
            G.evaluation._enqueue_forward(lib, model.flat_parameters, P, stream)

    paths = {"a estimate_store": a, "b torch loop through the module": b, "c bare forward": c}
    times = {k: [] for k in paths}
    for fn in paths.values():                                       # warm-up: plans, buffers, code objects
        fn(); fn()
    torch.cuda.synchronize()
    for _ in range(args.reps):
        for name, fn in paths.items():
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    b()
    ref = out.clone()
    a()
    same = torch.equal(out, ref)
    lines = ["Cost of PressureEstimator.estimate_store (tests/micro/estimate_cost.py)",
             "=" * 96,
             f"MEASURED on {torch.cuda.get_device_name(0)}, torch {torch.__version__}; gatres_small (15 x 32), {NODES} nodes, bs {BS}, "
             f"{S} snapshots, {K} sensors;",
             f"{args.reps} repetitions per path, the paths taking turns in one process, one synchronise per repetition.", ""]
    med = {}
    for name, ts in times.items():
        med[name] = statistics.median(ts)
        lines.append(f"  ({name}): median {S / med[name] / 1e3:8.1f} k graphs/s  ({med[name] * 1e3 / (S // BS):.4f} ms per batch; "
                     f"min {min(ts) * 1e3:.2f} / max {max(ts) * 1e3:.2f} ms per pass)")
    ma, mb, mc = (med[k] for k in paths)
    lines += ["", f"  the two new launches over the bare forward: {(ma - mc) * 1e3 / (S // BS):+.4f} ms per batch ({ma / mc:.3f} x)",
              f"  estimate_store against the torch loop:      {mb / ma:.2f} x the graphs/s",
              f"  estimates of (a) and (b) bit-identical:     {same}",
              f"  torch's fp32 tensor / Python float here:    {'product with the fp32 reciprocal' if G.estimation._divides_by_reciprocal(dev) else 'true division'}"]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
