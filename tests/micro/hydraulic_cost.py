"""Cost of the hydraulic snapshot generator (csrc/k_hydraulics.hip), one JSON line per mode.  Not collected by pytest.

    python tests/micro/hydraulic_cost.py --mode solve [--scenarios 2048] [--reps 5]     scenarios / s of gatres_hydraulic_solve at
                                                                                         388 nodes / 430 pipes / 3 reservoirs
    python tests/micro/hydraulic_cost.py --mode host [--host-scenarios 64]              solve_ref(solver="banded") on the same
                                                                                         scenarios, in a pool of 16 processes
    python tests/micro/hydraulic_cost.py --mode store [--scenarios 2048]                generate_store end to end (draw, solve,
                                                                                         valid, read-back, select)
    python tests/micro/hydraulic_cost.py --mode fit [--epochs 30]                       OBSERVATION, not a condition: fit of
                                                                                         gatres_small on a generated 388-node
                                                                                         store; validation MAE in metres against
                                                                                         the MAE of predicting the store mean

The kernel's registers, LDS and scratch are the compiler's (-Rpass-analysis=kernel-resource-usage on k_hydraulics.hip; the LDS
is dynamic: hydraulics.lds_bytes).  ``python bench.py`` at the parent and at the change, taking turns in one job, shows that the
headline did not move: no existing kernel changed."""
import argparse
import json
import os
import statistics
import sys
import time

NODES, PIPES, RESERVOIRS = 388, 430, 3
DEMAND_RANGE = (1e-5, 1e-4)


def network(G, device=None):
    return G.wdn_synth.make_hydraulic_network(NODES, PIPES, RESERVOIRS, seed=6, elevation_range=(0.0, 40.0), device=device)


def scenarios(G, net, S, seed=1):
    return G.hydraulics.hydraulic_draws(seed, 0, S, *net.draw_ranges(DEMAND_RANGE, G.hydraulics.ROUGHNESS_RANGE))


def _host_chunk(args):
    first, n = args
    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, root)
    import gnn_pressure_estimation_amd as G
    net = network(G)
    demand, roughness = G.hydraulics.hydraulic_draws(1, first, n, *net.draw_ranges(DEMAND_RANGE, G.hydraulics.ROUGHNESS_RANGE))
    ref = G.hydraulics.solve_ref(net, demand, roughness, solver="banded")
    return int(ref.converged.sum()), int(ref.iterations.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["solve", "host", "store", "fit"], default="solve")
    ap.add_argument("--scenarios", type=int, default=2048)
    ap.add_argument("--host-scenarios", type=int, default=64)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=30)
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    if args.mode == "host":                            # (no GPU in this mode: the pool's processes never open it)
        import multiprocessing as mp
        per = -(-args.host_scenarios // args.threads)
        jobs = [(f, min(per, args.host_scenarios - f)) for f in range(0, args.host_scenarios, per)]
        with mp.get_context("spawn").Pool(args.threads) as pool:
            pool.map(_host_chunk, jobs[:1])            # untimed: imports
            t0 = time.perf_counter()
            done = pool.map(_host_chunk, jobs)
            dt = time.perf_counter() - t0
        print(json.dumps({"mode": "host", "solver": "banded", "processes": args.threads, "scenarios": args.host_scenarios,
                          "converged": sum(d[0] for d in done), "mean_iterations": sum(d[1] for d in done) / args.host_scenarios,
                          "seconds": round(dt, 4), "scenarios_per_s": round(args.host_scenarios / dt, 1)}), flush=True)
        return
    import torch
    import gnn_pressure_estimation_amd as G
    assert torch.cuda.is_available(), "needs the MI355X"
    H = G.hydraulics
    net = network(G, "cuda:0")
    base = {"mode": args.mode, "nodes": NODES, "pipes": PIPES, "half_bandwidth": net.half_bandwidth,
            "lds_bytes": H.lds_bytes(NODES, PIPES, net.half_bandwidth), "build": G._native.load().gatres_version().decode(),
            "device": torch.cuda.get_device_name(0)}
    if args.mode == "solve":
        S = args.scenarios
        demand, roughness = (torch.from_numpy(a).cuda() for a in scenarios(G, net, S))
        res = net.simulate(demand, roughness)          # untimed: upload of the static arrays, the LDS attribute
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            res = net.simulate(demand, roughness, want_head=False, want_flow=False)
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        it = res.iterations.double()
        print(json.dumps({**base, "scenarios": S, "ms": [round(m, 3) for m in ms], "ms_median": round(statistics.median(ms), 3),
                          "scenarios_per_s": round(1e3 * S / statistics.median(ms), 1), "converged": int(res.converged.sum()),
                          "failed": int(res.failed.sum()), "mean_iterations": float(it.mean()), "max_iterations": int(it.max())}),
              flush=True)
    elif args.mode == "store":
        net.generate_store(64, 3, demand_range=DEMAND_RANGE, pressure_range=(-1e4, 1e4))      # untimed
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        store, report = net.generate_store(args.scenarios, 3, demand_range=DEMAND_RANGE, pressure_range=(0.0, 150.0))
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print(json.dumps({**base, "seconds": round(dt, 4), "scenarios_per_s": round(args.scenarios / dt, 1), "report": report,
                          "mean_m": store.mean, "std_m": store.std}), flush=True)
    else:
        train, rep_t = net.generate_store(2048, 11, demand_range=DEMAND_RANGE, pressure_range=(0.0, 150.0))
        val_raw, rep_v = net.generate_store(512, 12, demand_range=DEMAND_RANGE, pressure_range=(0.0, 150.0), normalize=False)
        val = G.SnapshotStore(val_raw.data, net.junction_edge_index, device="cuda:0", mean=train.mean, std=train.std)
        torch.manual_seed(21)
        model = G.GATResMeanConv(num_blocks=15, nc=32).cuda()
        tr = G.GATResTrainer.for_store(model, train, batch_size=32)
        t0 = time.perf_counter()
        h = tr.fit(train, val, args.epochs, batch_size=32, generator=torch.Generator().manual_seed(7), save_best="end")
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        # what predicting the training store's mean everywhere would score on the validation store, in metres
        mean_mae = float((val_raw.data - train.mean).abs().mean())
        # and what predicting every junction's own training mean would score (the elevations are static: a harder yardstick)
        node_mae = float((val_raw.data - train.descale(train.data).mean(dim=0, keepdim=True)).abs().mean())
        # the model's: the hidden 95 % of every validation snapshot, de-normalised (evaluation.evaluate_store's test_mae)
        loss, metrics = G.evaluation.evaluate_store(model, val, 32, 0.95, seed=0)
        print(json.dumps({**base, "epochs": len(h.tr_loss), "seconds": round(dt, 2), "train": rep_t, "val": rep_v,
                          "train_mean_m": train.mean, "train_std_m": train.std, "val_loss_first": h.val_loss[0],
                          "val_loss_last": h.val_loss[-1], "val_loss_best": min(h.val_loss), "evaluate_store_loss": float(loss),
                          "evaluate_store_metrics": {k: float(v) for k, v in metrics.items()},
                          "mae_of_predicting_the_mean_m": mean_mae,
                          "mae_of_predicting_each_junctions_mean_m": node_mae}), flush=True)


if __name__ == "__main__":
    main()
