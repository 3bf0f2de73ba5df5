"""Epoch-level cost of evaluation and of training metrics (not collected by pytest).

Graphs per second, wall clock around whole epochs (one synchronisation before and after each), for
  * the validation pass: evaluation.test_one_epoch (the host loop: numpy masks, an H2D copy, one timed forward, boolean
    gathers and seven metric syncs per batch) against evaluation.evaluate_store (three launches per batch, one sync per epoch);
  * a training epoch: GATResTrainer.fit_epoch without metrics, with the host metrics (metric_fn_dict=...) and with the
    device metrics (metric_fn_dict=..., device_metrics=True).
Configurations: gatres_small fp32 at batch 32 and gatres_large bf16 at batch 128, on a C-Town-sized synthetic store.

    python tests/micro/eval_epoch_cost.py [--snapshots 2000] [--epochs 3] [--only eval_small]

``--only eval_small`` runs evaluate_store alone (gatres_small, bs 32), for a kernel trace of the evaluation epoch:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tests/micro/eval_epoch_cost.py --only eval_small
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import numpy as np
import torch

import gnn_pressure_estimation_amd as G

NODES, PIPES = 388, 430


def timed(fn, epochs):
    fn()                                   # warm-up epoch: plans, buffers, captured sequences
    torch.cuda.synchronize()
    best = []
    for _ in range(epochs):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best.append(time.perf_counter() - t)
    return float(np.median(best))


def run(name, nb, nc, dtype, bs, S, epochs, only=None):
    torch.manual_seed(0)
    ei = G.wdn_synth.make_wdn_topology(NODES, PIPES, seed=0)
    store = G.SnapshotStore(G.wdn_synth.make_snapshots(S, NODES, seed=1) * 12.5 + 50.0, ei, device="cuda:0")
    model = G.GATResMeanConv(num_blocks=nb, nc=nc).cuda()
    if dtype != "fp32":
        model.set_compute_dtype(dtype)
    E = G.evaluation
    res = {"config": name, "dtype": dtype, "batch_size": bs, "snapshots": S}

    def dev_eval():
        return E.evaluate_store(model, store, bs, 0.95, gpu_warmup_times=10)

    if only == "eval_small":
        for _ in range(epochs + 1):
            dev_eval()
        torch.cuda.synchronize()
        return res
    res["evaluate_store_graphs_per_s"] = S / timed(dev_eval, epochs)
    rng = np.random.RandomState(0)

    def host_eval():
        return E.test_one_epoch(model, store.batches(bs, shuffle=False), 0.95, mean=store.mean, std=store.std,
                                norm_type="znorm", nodes_per_graph=NODES, gpu_warmup_times=10, rng=rng)

    res["test_one_epoch_graphs_per_s"] = S / timed(host_eval, epochs)
    res["eval_speedup"] = res["evaluate_store_graphs_per_s"] / res["test_one_epoch_graphs_per_s"]
    _, m_dev = dev_eval()
    _, m_host = host_eval()
    res["evaluate_store_test_throughput"] = m_dev["test_throughput"]
    res["test_one_epoch_test_throughput"] = m_host["test_throughput"]

    trainer = G.GATResTrainer(model, store.edge_index(bs), bs * NODES, nodes_per_graph=[NODES] * bs)
    gen = torch.Generator().manual_seed(0)
    fns = E.get_metric_fn_collection("train")
    res["fit_epoch_graphs_per_s"] = S / timed(lambda: trainer.fit_epoch(store, bs, generator=gen), epochs)
    res["fit_epoch_host_metrics_graphs_per_s"] = S / timed(lambda: trainer.fit_epoch(store, bs, generator=gen,
                                                                                     metric_fn_dict=fns), epochs)
    res["host_metrics_slowdown"] = res["fit_epoch_graphs_per_s"] / res["fit_epoch_host_metrics_graphs_per_s"]
    res["fit_epoch_device_metrics_graphs_per_s"] = S / timed(lambda: trainer.fit_epoch(store, bs, generator=gen, metric_fn_dict=fns,
                                                                                       device_metrics=True), epochs)
    res["device_metrics_slowdown"] = res["fit_epoch_graphs_per_s"] / res["fit_epoch_device_metrics_graphs_per_s"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--snapshots", type=int, default=2000)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--only", default=None, choices=[None, "eval_small"])
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    print(torch.cuda.get_device_name(0), file=sys.stderr)
    if a.only:
        run("gatres_small", 15, 32, "fp32", 32, a.snapshots, a.epochs, only=a.only)
        return
    for cfg in (("gatres_small", 15, 32, "fp32", 32), ("gatres_large", 25, 128, "bf16", 128)):
        print(json.dumps(run(*cfg, a.snapshots, a.epochs)), flush=True)


if __name__ == "__main__":
    main()
