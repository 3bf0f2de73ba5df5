"""Cost of the training criterion (GATResTrainer(criterion=...)), not collected by pytest: ms per training step with mse, mae
and sce, bench.py's bound-batch loop (gatres_small 15 x 32, C-Town-sized snapshots, bs 32, fp32 fused, resident batches,
hipGraph sequences of --graph-steps steps), the three trainers' timed blocks alternating in one process.  One JSON line.
    python tests/micro/criterion_cost.py [--steps 400] [--warmup 60] [--repeats 5]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

import gnn_pressure_estimation_amd as G

NODES, PIPES, NBATCHES, BS = 388, 430, 8, 32
CRITERIA = ("mse", "mae", "sce")


def make(criterion, graph_steps, steps, warmup):
    dev = torch.device("cuda", 0)
    torch.manual_seed(3)
    model = G.GATResMeanConv(name="gatres_small", num_blocks=15, nc=32).to(dev)
    topo = G.wdn_synth.make_wdn_topology(NODES, PIPES, seed=0)
    ei = G.wdn_synth.collate_edge_index(topo, NODES, BS).to(dev)
    tr = G.GATResTrainer(model, ei, NODES * BS, nodes_per_graph=[NODES] * BS, seed=1000, targets_are_inputs=True,
                         criterion=criterion)
    snaps = G.wdn_synth.make_snapshots(NBATCHES * BS, NODES, seed=100).to(dev)
    batches = [snaps[i * BS:(i + 1) * BS].reshape(-1).contiguous() for i in range(NBATCHES)]

    def chunks(k):
        return [tuple((i0 + j) % NBATCHES for j in range(min(graph_steps, k - i0))) for i0 in range(0, k, graph_steps)]
    seqs = sorted({c for c in chunks(steps) + chunks(warmup) if len(c) > 1})
    tr.bind_batches(batches, sequences=seqs)

    def run(k):
        for c in chunks(k):
            tr.steps_bound(c) if len(c) > 1 else tr.step_bound(c[0])
    return tr, run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=60)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--graph-steps", type=int, default=20)
    args = ap.parse_args()
    made = {c: make(c, args.graph_steps, args.steps, args.warmup) for c in CRITERIA}
    for _, run in made.values():
        run(args.warmup)
    torch.cuda.synchronize()
    g0 = {c: tr.num_captured_graphs for c, (tr, _) in made.items()}
    times = {c: [] for c in CRITERIA}
    for _ in range(args.repeats):
        for c in CRITERIA:
            run = made[c][1]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(args.steps)
            torch.cuda.synchronize()
            times[c].append((time.perf_counter() - t0) / args.steps * 1e3)
    assert {c: tr.num_captured_graphs for c, (tr, _) in made.items()} == g0, "a capture happened inside the timed region"
    for tr, _ in made.values():
        tr.check_no_dropped_steps()
    med = {c: statistics.median(times[c]) for c in CRITERIA}
    res = dict(model="gatres_small", batch_size=BS, path="fused", steps_per_block=args.steps, repeats=args.repeats,
               ms_per_step={c: round(med[c], 5) for c in CRITERIA},
               extra_us_per_step_vs_mse={c: round((med[c] - med["mse"]) * 1e3, 2) for c in CRITERIA if c != "mse"},
               blocks={c: [round(t, 5) for t in times[c]] for c in CRITERIA},
               last_loss={c: float(tr.loss) for c, (tr, _) in made.items()})
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
