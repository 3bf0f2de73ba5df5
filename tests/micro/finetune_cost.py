"""Cost of fine-tuning to a fixed sensor layout (``GATResTrainer.set_sensor_layout``): gatres_small, bs 32, 2 048 synthetic
C-Town-sized snapshots, 20 sensors, on one device.

  default     one ``fit_epoch`` on the row-gather path (``epoch_copy_limit_bytes = 0``: the path a layout epoch takes by design,
              so the comparison is like for like) as
                none       no layout (this configuration also runs on a commit without the feature: ``--root <checkout>``),
                layout     ``set_sensor_layout(obs)``                      -- dropout 0, share 1,
                mixed      ``set_sensor_layout(obs, sensor_dropout=0.1, layout_share=0.7)``,
              and, for orientation, ``inplace``: no layout on the default (in-place) epoch path.  Two untimed epochs each (plans,
              captures), then ``--reps`` timed epochs, wall clock around a final synchronisation; the configurations take turns
              repetition by repetition.  One JSON line per configuration: raw repetitions, median and range.
  --accuracy  an observation on synthetic data, not a claim: the validation MAE under the layout mask and under random 95 %
              masks, before and after ``--epochs`` epochs of ``PressureEstimator.fine_tune`` (dropout 0.1, share 0.7).
  --kernels   ``--launches`` launches each of ``gatres_stage_rows_mask`` (``stage_rows_mask_kernel<false>``) and
              ``gatres_stage_rows_mask_sensors`` at (0, 1) and (0.1, 0.7) on one batch, for a kernel trace of the process.

``--root``: import the package of another checkout (the parent commit) instead of the one this file lies in.  Not collected by
pytest.

    python tests/micro/finetune_cost.py [--reps 7] [--root <parent checkout> --label parent]
    python tests/micro/finetune_cost.py --accuracy [--epochs 3]
    python tests/micro/finetune_cost.py --kernels [--launches 200]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
NODES, PIPES, BS, SENSORS = 388, 430, 32, 20


def observed(G):
    g = torch.Generator().manual_seed(11)
    return sorted(torch.randperm(NODES, generator=g)[:SENSORS].tolist())


def stores(G, S, Sv=0):
    ei = G.wdn_synth.make_wdn_topology(NODES, PIPES, seed=0)
    tr = G.SnapshotStore(G.wdn_synth.make_snapshots(S, NODES, seed=3) * 12.5 + 50.0, ei, device="cuda:0")
    if not Sv:
        return tr, None
    va = G.SnapshotStore(G.wdn_synth.make_snapshots(Sv, NODES, seed=4) * 12.5 + 50.0, ei, device="cuda:0", mean=tr.mean, std=tr.std)
    return tr, va


def epochs(G, args):
    store, _ = stores(G, args.snapshots)
    obs = observed(G)
    has = hasattr(G.GATResTrainer, "set_sensor_layout")
    configs = {"none": None, "inplace": None}
    if has:
        configs.update(layout=(0.0, 1.0), mixed=(0.1, 0.7))
    runs = {}
    for name, lay in configs.items():
        torch.manual_seed(21)
        model = G.GATResMeanConv(num_blocks=15, nc=32).cuda()
        tr = G.GATResTrainer.for_store(model, store, BS)
        if name != "inplace":
            tr.epoch_copy_limit_bytes = 0
        if lay is not None:
            tr.set_sensor_layout(obs, sensor_dropout=lay[0], layout_share=lay[1])
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


def accuracy(G, args):
    train, val = stores(G, args.snapshots, args.snapshots // 4)
    obs = observed(G)
    torch.manual_seed(21)
    model = G.GATResMeanConv(num_blocks=15, nc=32).cuda()
    E = G.evaluation

    def maes():
        lay = E.evaluate_store(model, val, BS, 0.95, gpu_warmup_times=0, observed_idx=obs)[1]["test_mae"]
        rnd = E.evaluate_store(model, val, BS, 0.95, gpu_warmup_times=0, seed=1)[1]["test_mae"]
        return round(lay, 5), round(rnd, 5)

    # a model trained the reference's way first (random 95 % masks), then fine-tuned to the layout
    pre = G.GATResTrainer.for_store(model, train, BS, lr=5e-4)
    pre.fit(train, val, args.pretrain, batch_size=BS, generator=torch.Generator().manual_seed(7))
    before = maes()
    est = G.PressureEstimator.for_store(model, train, obs, batch_size=BS)
    hist = est.fine_tune(train, val, args.epochs, lr=5e-4, sensor_dropout=0.1, layout_share=0.7,
                         generator=torch.Generator().manual_seed(8))
    after = maes()
    print(json.dumps({"accuracy": "validation MAE (physical units): [layout mask, random 95 % masks]", "pretrain_epochs": args.pretrain,
                      "finetune_epochs": args.epochs, "before": before, "after": after,
                      "finetune_val_loss": [round(v, 6) for v in hist.val_loss]}), flush=True)


def kernels(G, args):
    store, _ = stores(G, 256)
    lib = G._native.load()
    obs = torch.tensor(observed(G), dtype=torch.int32, device="cuda:0")
    x = torch.empty(BS * NODES, device="cuda:0")
    mask = torch.empty(BS * NODES, dtype=torch.uint8, device="cuda:0")
    node_ptr = torch.arange(0, (BS + 1) * NODES, NODES, dtype=torch.int32, device="cuda:0")
    ctr = torch.zeros(2, dtype=torch.int64, device="cuda:0")
    rows = torch.randperm(256, generator=torch.Generator().manual_seed(1))[:BS].to("cuda:0")
    for i in range(args.launches):
        ctr[0] = i
        assert lib.gatres_stage_rows_mask(store.data.data_ptr(), rows.data_ptr(), NODES, x.data_ptr(), None, node_ptr.data_ptr(), BS,
                                          0.95, 9, ctr.data_ptr(), mask.data_ptr(), None) == 0
        for drop, share in ((0.0, 1.0), (0.1, 0.7)):
            assert lib.gatres_stage_rows_mask_sensors(store.data.data_ptr(), rows.data_ptr(), NODES, x.data_ptr(), None,
                                                      node_ptr.data_ptr(), BS, obs.data_ptr(), SENSORS, drop, share, 0.95, 9,
                                                      ctr.data_ptr(), mask.data_ptr(), None) == 0
    torch.cuda.synchronize()
    print(json.dumps({"kernels": "launched", "launches_each": args.launches,
                      "note": "the sensors kernel ran twice per trip: (0, 1) then (0.1, 0.7)"}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--snapshots", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--pretrain", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--accuracy", action="store_true")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--label", default="change")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import gnn_pressure_estimation_amd as G
    assert torch.cuda.is_available(), "needs the MI355X"
    (accuracy if args.accuracy else kernels if args.kernels else epochs)(G, args)


if __name__ == "__main__":
    main()
