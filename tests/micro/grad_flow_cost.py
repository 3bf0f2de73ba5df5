"""Cost of ``fit(log_gradient=True)``: E epochs of training + validation on gatres_small, bs 32, synthetic C-Town snapshots
through ``GATResTrainer.fit(save_best="end")`` -- the set-up of ``fit_overhead.py --mode fit`` -- with the option off or on.
Each after one untimed epoch (captures, plans, buffers), wall clock around a final synchronisation, ``--reps`` repetitions;
prints one JSON line per store size with the raw repetitions, the median and the range.  Not collected by pytest.

    python tests/micro/grad_flow_cost.py --log-gradient 1 [--sizes 512,2048] [--epochs 20] [--reps 3] [--label change_on]

``--root DIR`` imports the package from another checkout (with its own built library), e.g. the parent commit, whose ``fit`` has
no such option: run it there with ``--log-gradient -1`` (the keyword is then not passed at all).  For a comparison, let the
sides take turns as processes of one job on one machine."""
import argparse
import json
import math
import os
import statistics
import sys
import time

NODES, PIPES, BS = 388, 430, 32


def kernels(G, torch):
    """us per launch of gatres_grad_flow (gatres_small, gatres_large) and gatres_mean_abs_diff (bs 32 / 128 of 388 nodes)."""
    import ctypes as C
    lib, dev, n_launch = G._native.load(), "cuda:0", 200

    def timed(fn):
        for _ in range(10):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(n_launch):
            fn()
        b.record()
        torch.cuda.synchronize()
        return round(1e3 * a.elapsed_time(b) / n_launch, 3)

    res = {}
    for name, nb, nc in (("gatres_small", 15, 32), ("gatres_large", 25, 128)):
        m = G._native.GatresModel(nb, nc, 0, 0)
        g = torch.randn(int(lib.gatres_param_count(nb, nc)), device=dev)
        out = torch.zeros(1 + 8 * nb, dtype=torch.float64, device=dev)
        res[f"grad_flow_us_{name}"] = [timed(lambda: lib.gatres_grad_flow(C.byref(m), g.data_ptr(), 1.0, None, out.data_ptr(), None))
                                       for _ in range(3)]
    for bs in (32, 128):
        a, b = torch.randn(bs * NODES, device=dev), torch.randn(bs * NODES, device=dev)
        out = torch.zeros(1, dtype=torch.float64, device=dev)
        res[f"mean_abs_diff_us_{bs * NODES}_nodes"] = [timed(lambda: lib.gatres_mean_abs_diff(a.data_ptr(), b.data_ptr(), a.numel(),
                                                                                            out.data_ptr(), None)) for _ in range(3)]
    res["note"] = "back-to-back launches on one stream: launch-rate bound where the kernel is shorter than a launch"
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-gradient", type=int, choices=[-1, 0, 1], default=0)
    ap.add_argument("--kernels", action="store_true", help="time the two kernels alone (HIP events around 200 launches)")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    ap.add_argument("--label", default="")
    ap.add_argument("--sizes", default="512,2048")
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    import gnn_pressure_estimation_amd as G
    assert torch.cuda.is_available(), "needs the MI355X"
    if args.kernels:
        return kernels(G, torch)
    kw = {} if args.log_gradient < 0 else {"log_gradient": bool(args.log_gradient)}
    ei = G.wdn_synth.make_wdn_topology(NODES, PIPES, seed=0)
    for S in (int(s) for s in args.sizes.split(",")):
        train = G.SnapshotStore(G.wdn_synth.make_snapshots(S, NODES, seed=3) * 12.5 + 50.0, ei, device="cuda:0")
        val = G.SnapshotStore(G.wdn_synth.make_snapshots(S // 4, NODES, seed=4) * 12.5 + 50.0, ei, device="cuda:0",
                              mean=train.mean, std=train.std)
        times = []
        for rep in range(args.reps):
            torch.manual_seed(21)
            model = G.GATResMeanConv(num_blocks=15, nc=32).cuda()
            tr = G.GATResTrainer(model, train.edge_index(BS), BS * NODES, nodes_per_graph=[NODES] * BS, targets_are_inputs=True)
            gen = torch.Generator().manual_seed(7)
            tr.fit(train, val, 1, batch_size=BS, generator=gen, save_best="end", **kw)                   # untimed epoch
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h = tr.fit(train, val, args.epochs, batch_size=BS, generator=gen, val_seed=1, save_best="end", **kw)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert len(h.tr_loss) == args.epochs and math.isfinite(h.val_loss[-1])
            if args.log_gradient > 0:
                assert len(h.total_grad_norm) == args.epochs and h.model_update[0] == 0.0
            times.append(dt)
            del tr, model
        ms = [1e3 * t / args.epochs for t in times]
        print(json.dumps({"label": args.label, "log_gradient": args.log_gradient, "train_snapshots": S, "val_snapshots": S // 4,
                          "epochs": args.epochs, "ms_per_epoch": [round(m, 4) for m in ms],
                          "ms_per_epoch_median": round(statistics.median(ms), 4),
                          "ms_per_epoch_range": [round(min(ms), 4), round(max(ms), 4)],
                          "build": G._native.load().gatres_version().decode(), "device": torch.cuda.get_device_name(0)}),
              flush=True)


if __name__ == "__main__":
    main()
