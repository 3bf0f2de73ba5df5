"""Cost of AutoClip (GATResTrainer(use_gradient_clipping=True)), not collected by pytest: ms per training step with clipping
off and on, bench.py's bound-batch loop (resident batches, hipGraph sequences of --graph-steps steps), the two trainers'
timed blocks alternating in one process.  One JSON line per configuration.
    python tests/micro/autoclip_cost.py [--config small|large|both] [--steps 400] [--warmup 60] [--repeats 5]
small: gatres_small 15 x 32, C-Town-sized snapshots, bs 32, fp32 fused (bench.py's headline).  large: gatres_large 25 x 128,
bs 128, bf16 per-op."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

import gnn_pressure_estimation_amd as G

CONFIGS = {"small": dict(model="gatres_small", nb=15, nc=32, bs=32, dtype="fp32", per_op=False),
           "large": dict(model="gatres_large", nb=25, nc=128, bs=128, dtype="bf16", per_op=True)}
NODES, PIPES, NBATCHES = 388, 430, 8


def make(cfg, clip, graph_steps, steps, warmup):
    dev = torch.device("cuda", 0)
    torch.manual_seed(3)
    model = G.GATResMeanConv(name=cfg["model"], num_blocks=cfg["nb"], nc=cfg["nc"]).to(dev)
    if cfg["dtype"] == "bf16":
        model.set_compute_dtype("bf16")
    bs = cfg["bs"]
    topo = G.wdn_synth.make_wdn_topology(NODES, PIPES, seed=0)
    ei = G.wdn_synth.collate_edge_index(topo, NODES, bs).to(dev)
    tr = G.GATResTrainer(model, ei, NODES * bs, nodes_per_graph=[NODES] * bs, seed=1000, fused=not cfg["per_op"],
                         targets_are_inputs=True, use_gradient_clipping=clip, percentile=10.0)
    snaps = G.wdn_synth.make_snapshots(NBATCHES * bs, NODES, seed=100).to(dev)
    batches = [snaps[i * bs:(i + 1) * bs].reshape(-1).contiguous() for i in range(NBATCHES)]

    def chunks(k):
        return [tuple((i0 + j) % NBATCHES for j in range(min(graph_steps, k - i0))) for i0 in range(0, k, graph_steps)]
    seqs = sorted({c for c in chunks(steps) + chunks(warmup) if len(c) > 1})
    tr.bind_batches(batches, sequences=seqs)

    def run(k):
        for c in chunks(k):
            tr.steps_bound(c) if len(c) > 1 else tr.step_bound(c[0])
    return tr, run


def measure(name, args):
    cfg = CONFIGS[name]
    tr_off, run_off = make(cfg, False, args.graph_steps, args.steps, args.warmup)
    tr_on, run_on = make(cfg, True, args.graph_steps, args.steps, args.warmup)
    run_off(args.warmup)
    run_on(args.warmup)
    torch.cuda.synchronize()
    g0 = (tr_off.num_captured_graphs, tr_on.num_captured_graphs)
    times = {"off": [], "on": []}
    for _ in range(args.repeats):
        for key, run in (("off", run_off), ("on", run_on)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(args.steps)
            torch.cuda.synchronize()
            times[key].append((time.perf_counter() - t0) / args.steps * 1e3)
    assert (tr_off.num_captured_graphs, tr_on.num_captured_graphs) == g0, "a capture happened inside the timed region"
    tr_off.check_no_dropped_steps()
    tr_on.check_no_dropped_steps()
    hist = tr_on.grad_norm_history()
    off, on = statistics.median(times["off"]), statistics.median(times["on"])
    return dict(config=name, model=cfg["model"], batch_size=cfg["bs"], dtype=cfg["dtype"], path="per_op" if cfg["per_op"] else "fused",
                steps_per_block=args.steps, repeats=args.repeats, ms_per_step_off=round(off, 5), ms_per_step_on=round(on, 5),
                extra_us_per_step=round((on - off) * 1e3, 2), blocks_off=[round(t, 5) for t in times["off"]],
                blocks_on=[round(t, 5) for t in times["on"]], history_len=len(hist),
                last_clip_coef=float(tr_on.last_clip_coef))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="both", choices=["small", "large", "both"])
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=60)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--graph-steps", type=int, default=20)
    args = ap.parse_args()
    for name in (["small", "large"] if args.config == "both" else [args.config]):
        print(json.dumps(measure(name, args)), flush=True)


if __name__ == "__main__":
    main()
