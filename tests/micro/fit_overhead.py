"""Cost of the epoch boundary: E epochs of training + validation on gatres_small, bs 32, synthetic C-Town snapshots, as
(a) ``--mode hand``: the hand-written loop -- ``fit_epoch`` + ``evaluation.evaluate_store`` + the controller on the host +
    ``set_lr`` -- which uses only interfaces that exist without ``fit`` (run it on the parent commit for the comparison), and
(b) ``--mode fit``: ``GATResTrainer.fit(save_best="end")`` without files.
Each after one untimed epoch (captures, plans, buffers), wall clock around a final synchronisation, ``--reps`` repetitions;
prints one JSON line per store size with the raw repetitions, the median and the range.  Not collected by pytest.

    python tests/micro/fit_overhead.py --mode fit [--sizes 512,2048,8192] [--epochs 20] [--reps 3]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
NODES, PIPES, BS = 388, 430, 32


class _HostController:
    """Best bookkeeping + EarlyStopping (fp32) + ReduceLROnPlateau (torch's own class on a dummy optimizer): what a user of the
    reference writes around fit_epoch / evaluate_store."""

    def __init__(self, lr, patience, min_delta, scheduler_patience):
        import numpy as np
        self.np = np
        self.opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=lr)
        self.sched = torch.optim.lr_scheduler.ReduceLROnPlateau(self.opt, mode="min", patience=scheduler_patience)
        self.patience, self.min_delta = patience, np.float32(min_delta)
        self.best, self.bad, self.best_loss, self.best_epoch, self.epoch = None, 0, math.inf, 0, 0

    def step(self, val_loss):
        np = self.np
        self.epoch += 1
        improved = val_loss < self.best_loss
        if improved:
            self.best_loss, self.best_epoch = val_loss, self.epoch
        m, stop = np.float32(val_loss), False
        if self.best is None:
            self.best = m
        elif np.isnan(m):
            stop = True
        else:
            if m < np.float32(self.best - self.min_delta):
                self.bad, self.best = 0, m
            else:
                self.bad += 1
            stop = self.bad >= self.patience
        if not stop:
            self.sched.step(val_loss)
        return improved, stop, self.opt.param_groups[0]["lr"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["hand", "fit"], required=True)
    ap.add_argument("--sizes", default="512,2048,8192")
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    import gnn_pressure_estimation_amd as G
    assert torch.cuda.is_available(), "needs the MI355X"
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
            # patience 100 / min_delta 1e-4 / scheduler_patience 2: train.py's defaults; no run stops within the timed epochs
            if args.mode == "fit":
                tr.fit(train, val, 1, batch_size=BS, generator=gen, save_best="end")                    # untimed epoch
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                h = tr.fit(train, val, args.epochs, batch_size=BS, generator=gen, val_seed=1, save_best="end")
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                done, last = len(h.tr_loss), h.val_loss[-1]
            else:
                ctl = _HostController(tr.hparams["lr"], 100, 1e-4, 2)
                best = None

                def epoch(e):
                    nonlocal best
                    tr.fit_epoch(train, BS, generator=gen)
                    v, _ = G.evaluation.evaluate_store(model, val, BS, tr.mask_rate, seed=e, prefix="val", gpu_warmup_times=0)
                    improved, stop, lr = ctl.step(v)
                    if improved:           # the reference saves best_*.pth here; the cheapest honest stand-in keeps it on the device
                        best = (model.flat_parameters.detach().clone(), tr.exp_avg.clone(), tr.exp_avg_sq.clone(),
                                tr.step_counter.clone())
                    tr.set_lr(lr)
                    return v, stop

                epoch(0)                                                                                 # untimed epoch
                ctl = _HostController(tr.hparams["lr"], 100, 1e-4, 2)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                done = 0
                for e in range(1, args.epochs + 1):
                    last, stop = epoch(1 + e)
                    done += 1
                    if stop:
                        break
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
            assert done == args.epochs and math.isfinite(last)
            times.append(dt)
            del tr, model
        print(json.dumps({"mode": args.mode, "train_snapshots": S, "val_snapshots": S // 4, "epochs": args.epochs,
                          "seconds": [round(t, 5) for t in times], "median_s": round(statistics.median(times), 5),
                          "range_s": [round(min(times), 5), round(max(times), 5)],
                          "ms_per_epoch_median": round(1e3 * statistics.median(times) / args.epochs, 4),
                          "device": torch.cuda.get_device_name(0)}), flush=True)


if __name__ == "__main__":
    main()
