"""Cost of training from a ``MultiSnapshotStore``: ``fit_epoch`` on gatres_small, bs 32, synthetic networks, as
  single   a ``SnapshotStore`` of the C-Town-sized network (the single-store path, which this script can also run on a
           commit without ``MultiSnapshotStore``: ``--only single``),
  k1       the same data as a one-network ``MultiSnapshotStore``,
  net0..2  every network of the mixed store by itself (``SnapshotStore``),
  mixed    three networks (388, 150 and 501 nodes) in one ``MultiSnapshotStore``.
Each configuration: two untimed epochs (plans, captures, buffers), then ``--reps`` timed epochs, wall clock around a final
synchronisation; the configurations take turns repetition by repetition, so drift hits all of them alike.  Prints one JSON line
per configuration -- raw repetitions, median and range in microseconds per graph and per node -- and the ratios the README
quotes.  ``rows_ms_median``: the host's share of an epoch's start -- drawing the permutation(s), laying the rows out batch by
batch and uploading them -- timed by itself.  ``--label`` names the commit the package was built from (the script may be run
against another checkout's package: it imports the package that lies two directories above it).  Not collected by pytest.

    python tests/micro/multi_store_cost.py [--snapshots 4096] [--reps 5] [--only single] [--label "parent ff42831"]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
NETS = [(388, 430), (150, 163), (501, 560)]
BS = 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--snapshots", type=int, default=4096, help="snapshots of the C-Town-sized network (the others: 1/2, 1/4)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="")
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    import gnn_pressure_estimation_amd as G
    assert torch.cuda.is_available(), "needs the MI355X"
    S = [args.snapshots, args.snapshots // 2, args.snapshots // 4]
    nets = []
    for k, ((n, p), s) in enumerate(zip(NETS, S)):
        nets.append((G.wdn_synth.make_snapshots(s, n, seed=3 + k) * 12.5 + 50.0, G.wdn_synth.make_wdn_topology(n, p, seed=k)))
    stores = {"single": G.SnapshotStore(*nets[0], device="cuda:0")}
    if hasattr(G, "MultiSnapshotStore"):
        stores["k1"] = G.MultiSnapshotStore(nets[:1], device="cuda:0")
        for k in range(3):
            stores[f"net{k}"] = G.SnapshotStore(*nets[k], device="cuda:0")
        stores["mixed"] = G.MultiSnapshotStore(nets, device="cuda:0")
    if args.only:
        stores = {k: v for k, v in stores.items() if k in args.only.split(",")}
    runs = {}
    for name, store in stores.items():
        torch.manual_seed(21)
        model = G.GATResMeanConv(num_blocks=15, nc=32).cuda()
        if hasattr(G.GATResTrainer, "for_store"):
            tr = G.GATResTrainer.for_store(model, store, BS)
        else:
            tr = G.GATResTrainer(model, store.edge_index(BS), BS * store.nodes_per_graph,
                                 nodes_per_graph=[store.nodes_per_graph] * BS, targets_are_inputs=True)
        gen = torch.Generator().manual_seed(7)
        tr.fit_epoch(store, BS, generator=gen)                         # untimed epoch
        tr.fit_epoch(store, BS, generator=gen)
        graphs = len(store)
        nodes = graphs * store.nodes_per_graph if not hasattr(store, "num_networks") else \
            sum(store.lengths[k] * store.nodes_per_graph_of(k) for k in range(store.num_networks))
        runs[name] = dict(tr=tr, store=store, gen=gen, graphs=graphs, nodes=nodes, times=[],
                          recipe=getattr(tr, "_recipe", None))
    for rep in range(args.reps):
        for name, r in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r["tr"].fit_epoch(r["store"], BS, generator=r["gen"])
            torch.cuda.synchronize()
            r["times"].append(time.perf_counter() - t0)
    import socket
    commit = args.label
    if not commit:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
        except OSError:
            commit = ""
    for name, r in runs.items():                       # the host side of an epoch's start, by itself
        store, ts = r["store"], []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if hasattr(store, "num_networks"):
                store.epoch_rows(store.schedule(BS, r["recipe"]), shuffle=True, generator=r["gen"])
            else:
                store.epoch_order(shuffle=True, generator=r["gen"])
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        r["rows_ms"] = 1e3 * statistics.median(ts)
    out = {}
    for name, r in runs.items():
        med = statistics.median(r["times"])
        out[name] = dict(us_per_graph=1e6 * med / r["graphs"], ns_per_node=1e9 * med / r["nodes"])
        print(json.dumps({"config": name, "graphs": r["graphs"], "nodes": r["nodes"], "recipe": r["recipe"], "reps": args.reps,
                          "epoch_s": [round(t, 5) for t in r["times"]], "median_s": round(med, 5),
                          "range_s": [round(min(r["times"]), 5), round(max(r["times"]), 5)],
                          "us_per_graph_median": round(out[name]["us_per_graph"], 3),
                          "ns_per_node_median": round(out[name]["ns_per_node"], 3),
                          "rows_ms_median": round(r["rows_ms"], 4), "commit": commit or "(working tree)",
                          "host": socket.gethostname(), "device": torch.cuda.get_device_name(0)}), flush=True)
    if "single" in out and "k1" in out:
        print(json.dumps({"ratio": "k1 / single (epoch time)", "value": round(out["k1"]["us_per_graph"] / out["single"]["us_per_graph"], 4)}))
    if "mixed" in out and all(f"net{k}" in out for k in range(3)):
        # the three single-network costs per node, weighted by the nodes each network contributes to the mixed epoch
        w = [runs[f"net{k}"]["nodes"] for k in range(3)]
        mean = sum(out[f"net{k}"]["ns_per_node"] * w[k] for k in range(3)) / sum(w)
        print(json.dumps({"ratio": "mixed / node-weighted mean of the three single-network runs (time per node)",
                          "value": round(out["mixed"]["ns_per_node"] / mean, 4), "weighted_ns_per_node": round(mean, 3)}))


if __name__ == "__main__":
    main()
