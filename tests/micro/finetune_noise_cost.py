"""Cost of fine-tuning under sensor noise (``GATResTrainer.set_sensor_layout(noise_std=...)``): gatres_small, bs 32, 2 048
synthetic C-Town-sized snapshots, 20 sensors, on one device.

  default     one ``fit_epoch`` on the row-gather path (``epoch_copy_limit_bytes = 0``: the path a layout epoch takes by design,
              so the comparison is like for like) as
                none       no layout (this configuration also runs on a commit without the feature: ``--root <checkout>``),
                mixed      ``set_sensor_layout(obs, sensor_dropout=0.1, layout_share=0.7)`` (the parent has it too),
                noisy      the same with ``noise_std=0.5``.
              Two untimed epochs each (plans, captures), then ``--reps`` timed epochs, wall clock around a final
              synchronisation; the configurations take turns repetition by repetition.  One JSON line per configuration: raw
              repetitions, median and range.
  --kernels   ``--launches`` trips of four launches on one batch -- ``gatres_stage_rows_mask_sensors`` at (0, 1) and (0.1, 0.7),
              then ``gatres_stage_rows_mask_sensors_noisy`` at the same two -- for a kernel trace of the process.
  --summarize DIR   the per-case figures from that trace's ``*kernel_trace.csv``: the two instantiations differ by name
              (``stage_rows_mask_sensors_kernel<false>`` / ``<true>``), the two settings of each by their place in the trip.
  --spread    an observation on synthetic data, not a claim: ``noise_report``'s ``nonsensor_spread`` before and after ``--epochs``
              epochs of ``PressureEstimator.fine_tune(noise_std=...)``.

``--root``: import the package of another checkout (the parent commit) instead of the one this file lies in.  Not collected by
pytest.

    python tests/micro/finetune_noise_cost.py [--reps 7] [--root <parent checkout> --label parent]
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o kt -- python tests/micro/finetune_noise_cost.py --kernels
    python tests/micro/finetune_noise_cost.py --summarize <dir>
    python tests/micro/finetune_noise_cost.py --spread [--epochs 3]
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
NODES, PIPES, BS, SENSORS, NOISE_STD = 388, 430, 32, 20, 0.5
KERNEL_CASES = ["plain (0, 1)", "plain (0.1, 0.7)", "noisy (0, 1)", "noisy (0.1, 0.7)"]


def observed(torch):
    g = torch.Generator().manual_seed(11)
    return sorted(torch.randperm(NODES, generator=g)[:SENSORS].tolist())


def stores(G, S, Sv=0):
    ei = G.wdn_synth.make_wdn_topology(NODES, PIPES, seed=0)
    tr = G.SnapshotStore(G.wdn_synth.make_snapshots(S, NODES, seed=3) * 12.5 + 50.0, ei, device="cuda:0")
    if not Sv:
        return tr, None
    va = G.SnapshotStore(G.wdn_synth.make_snapshots(Sv, NODES, seed=4) * 12.5 + 50.0, ei, device="cuda:0", mean=tr.mean, std=tr.std)
    return tr, va


def epochs(G, torch, args):
    store, _ = stores(G, args.snapshots)
    obs = observed(torch)
    has = hasattr(G, "sensor_layout_noise")
    configs = {"none": None, "mixed": {}}
    if has:
        configs["noisy"] = dict(noise_std=NOISE_STD)
    runs = {}
    for name, kw in configs.items():
        torch.manual_seed(21)
        model = G.GATResMeanConv(num_blocks=15, nc=32).cuda()
        tr = G.GATResTrainer.for_store(model, store, BS)
        tr.epoch_copy_limit_bytes = 0
        if kw is not None:
            tr.set_sensor_layout(obs, sensor_dropout=0.1, layout_share=0.7, **kw)
        gen = torch.Generator().manual_seed(7)
        for _ in range(2):
            tr.fit_epoch(store, BS, generator=gen)
        runs[name] = dict(tr=tr, gen=gen, times=[])
    for _ in range(args.reps):
        for name, r in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r["tr"].fit_epoch(store, BS, generator=r["gen"])
            torch.cuda.synchronize()
            r["times"].append(time.perf_counter() - t0)
    import socket
    for name, r in runs.items():
        med = statistics.median(r["times"])
        taken = sorted({k[0] for k in r["tr"]._graphs if isinstance(k[0], str)})
        print(json.dumps({"config": name, "label": args.label, "snapshots": args.snapshots, "reps": args.reps,
                          "epoch_ms": [round(1e3 * t, 3) for t in r["times"]], "median_ms": round(1e3 * med, 3),
                          "range_ms": [round(1e3 * min(r["times"]), 3), round(1e3 * max(r["times"]), 3)],
                          "us_per_step_median": round(1e6 * med / (args.snapshots // BS), 3), "sequences": taken,
                          "host": socket.gethostname(), "device": torch.cuda.get_device_name(0)}), flush=True)


def spread(G, torch, args):
    train, val = stores(G, args.snapshots, args.snapshots // 8)
    obs = observed(torch)
    torch.manual_seed(21)
    model = G.GATResMeanConv(num_blocks=15, nc=32).cuda()
    # a model trained the reference's way first (random 95 % masks), then fine-tuned to the layout under noise
    pre = G.GATResTrainer.for_store(model, train, BS, lr=5e-4)
    pre.fit(train, val, args.pretrain, batch_size=BS, generator=torch.Generator().manual_seed(7))
    est = G.PressureEstimator.for_store(model, train, obs, batch_size=BS)

    def report():
        rep = est.noise_report(val, NOISE_STD, args.members, seed=5)
        return round(float(rep["nonsensor_spread"]), 6)

    before = report()
    hist = est.fine_tune(train, val, args.epochs, lr=5e-4, sensor_dropout=0.1, layout_share=0.7, noise_std=NOISE_STD,
                         generator=torch.Generator().manual_seed(8))
    after = report()
    print(json.dumps({"spread": "noise_report nonsensor_spread (physical units) on the validation store", "noise_std": NOISE_STD,
                      "members": args.members, "pretrain_epochs": args.pretrain, "finetune_epochs": args.epochs, "before": before,
                      "after": after, "finetune_val_loss": [round(v, 6) for v in hist.val_loss]}), flush=True)


def kernels(G, torch, args):
    store, _ = stores(G, 256)
    lib = G._native.load()
    obs = torch.tensor(observed(torch), dtype=torch.int32, device="cuda:0")
    sigma = torch.full((SENSORS,), NOISE_STD / (store.std + 1e-8), dtype=torch.float32, device="cuda:0")
    x = torch.empty(BS * NODES, device="cuda:0")
    mask = torch.empty(BS * NODES, dtype=torch.uint8, device="cuda:0")
    node_ptr = torch.arange(0, (BS + 1) * NODES, NODES, dtype=torch.int32, device="cuda:0")
    ctr = torch.zeros(2, dtype=torch.int64, device="cuda:0")
    rows = torch.randperm(256, generator=torch.Generator().manual_seed(1))[:BS].to("cuda:0")
    head = (store.data.data_ptr(), rows.data_ptr(), NODES, x.data_ptr(), None, node_ptr.data_ptr(), BS, obs.data_ptr(), SENSORS)
    for i in range(args.launches):
        ctr[0] = i
        for drop, share in ((0.0, 1.0), (0.1, 0.7)):
            assert lib.gatres_stage_rows_mask_sensors(*head, drop, share, 0.95, 9, ctr.data_ptr(), mask.data_ptr(), None) == 0
        for drop, share in ((0.0, 1.0), (0.1, 0.7)):
            assert lib.gatres_stage_rows_mask_sensors_noisy(*head, drop, share, 0.95, 9, ctr.data_ptr(), mask.data_ptr(),
                                                            sigma.data_ptr(), 20260, None) == 0
    torch.cuda.synchronize()
    print(json.dumps({"kernels": "launched", "trips": args.launches, "per_trip": KERNEL_CASES}), flush=True)


def summarize(args):
    files = sorted(glob.glob(os.path.join(args.summarize, "**", "*kernel_trace.csv"), recursive=True))
    if len(files) != 1:
        raise SystemExit(f"want one *kernel_trace.csv under {args.summarize}, found {files}")
    rows = [r for r in csv.DictReader(open(files[0])) if "stage_rows_mask_sensors_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    if len(rows) != len(KERNEL_CASES) * args.launches:
        raise SystemExit(f"{len(rows)} staging kernels in the trace, want {len(KERNEL_CASES)} x {args.launches}")
    for i, name in enumerate(KERNEL_CASES):
        part = rows[i::len(KERNEL_CASES)]
        names = sorted({r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0] for r in part})
        if len(names) != 1 or ("<true>" in names[0]) != name.startswith("noisy"):
            raise SystemExit(f"{name}: its launches are not the one kernel expected: {names}")
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in part[args.skip:]]     # (the first ones load code)
        print(json.dumps({"case": name, "kernel": names[0], "launches": len(us), "avg_us": round(statistics.fmean(us), 3),
                          "median_us": round(statistics.median(us), 3), "min_us": round(min(us), 3),
                          "p90_us": round(sorted(us)[int(0.9 * len(us))], 3), "max_us": round(max(us), 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--snapshots", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--pretrain", type=int, default=3)
    ap.add_argument("--members", type=int, default=16)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--skip", type=int, default=20, help="--summarize: launches of each case left out of its figures (warm-up)")
    ap.add_argument("--spread", action="store_true")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--summarize", metavar="DIR")
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--label", default="change")
    args = ap.parse_args()
    if args.summarize:
        return summarize(args)
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    import gnn_pressure_estimation_amd as G
    assert torch.cuda.is_available(), "needs the MI355X"
    (spread if args.spread else kernels if args.kernels else epochs)(G, torch, args)


if __name__ == "__main__":
    main()
