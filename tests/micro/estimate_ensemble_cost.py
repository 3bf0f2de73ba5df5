"""What a noise ensemble costs PressureEstimator (not collected; writes profiles/estimate_ensemble_cost.txt).

gatres_small (15 x 32), 388 nodes, bs 32, 20 sensors.  The paths take turns in one process (a rotating order inside each group),
``--reps`` times each, every repetition ending in one synchronise; medians, and the spread of the repetitions:
  (i)   ``estimate_store_ensemble``, S = 2 048, M = 8 (16 384 pairs, 512 batches, one reduce launch) against 8 plain
        ``estimate_store`` passes (the same 512 batches without noise and without the reduce), per pair;
  (ii)  the online case: ``estimate_ensemble`` of ONE snapshot with M = 32 (one batch of 32 graphs and the reduce) against
        ``estimate`` of 32 snapshots (the same batch), ``--online-calls`` calls back to back per repetition;
  (iii) the three new launches alone, ``--launches`` back to back per repetition: gatres_stage_observed_noisy against
        gatres_stage_observed on the same batch, gatres_ensemble_reduce on (i)'s scratch, gatres_node_spread_moments on [S, N];
and the largest deviation of the device's draws from ``reading_noise`` over 64 x 16 x 16 draws.  (iv), ``python bench.py --steps 20
--warmup 5`` at the parent commit and at the change, three turns each in the same job, is run by the job that runs this script;
``--bench-lines FILE`` appends that job's lines to the report.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import gnn_pressure_estimation_amd as G      # noqa: E402

NODES, PIPES, BS, S, K, M, M_ONLINE, SIGMA = 388, 430, 32, 2048, 20, 8, 32, 0.5


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--online-calls", type=int, default=50)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--bench-lines", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "estimate_ensemble_cost.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ei = G.wdn_synth.make_wdn_topology(NODES, PIPES, seed=0)
    raw = G.wdn_synth.make_snapshots(S, NODES, seed=1) * 12.5 + 50.0
    store = G.SnapshotStore(raw, ei, device=dev)
    torch.manual_seed(0)
    model = G.GATResMeanConv(num_blocks=15, nc=32).to(dev).eval()
    sensors = sorted(int(i) for i in torch.randperm(NODES, generator=torch.Generator().manual_seed(2))[:K])
    est = G.PressureEstimator.for_store(model, store, sensors, batch_size=BS)
    readings = raw.to(dev)[:, sensors].contiguous()
    one, batch = readings[:1].contiguous(), readings[:BS].contiguous()
    out = torch.empty((S, NODES), dtype=torch.float32, device=dev)
    mean, std = torch.empty_like(out), torch.empty_like(out)
    m1, s1 = mean[:1], std[:1]
    o32 = out[:BS]
    lib = G._native.load()
    stream = G._native.current_stream(dev)
    scratch = torch.randn((S * M, NODES), device=dev) * 0.1 + 50.0
    table = torch.empty((NODES, G._native.NODE_SPREAD_RECORD), dtype=torch.float64, device=dev)
    sigma = torch.full((K,), SIGMA, dtype=torch.float32, device=dev)
    x = torch.empty(BS * NODES, dtype=torch.float32, device=dev)
    mask = torch.empty(BS * NODES, dtype=torch.uint8, device=dev)
    obs = est._observed

    def ensemble():
        est.estimate_store_ensemble(store, SIGMA, M, seed=1, mean_out=mean, std_out=std)

    def plain():
        for _ in range(M):
            est.estimate_store(store, out=out)

    def online():
        for _ in range(args.online_calls):
            est.estimate_ensemble(one, SIGMA, M_ONLINE, seed=1, mean_out=m1, std_out=s1)

    def online_plain():
        for _ in range(args.online_calls):
            est.estimate(batch, out=o32)

    def stage_noisy():
        for _ in range(args.launches):
            lib.gatres_stage_observed_noisy(store.data.data_ptr(), 0, S, 64, M, 0, NODES, BS, obs.data_ptr(), K, 0, 0.0, 1.0,
                                            x.data_ptr(), mask.data_ptr(), None, 0, sigma.data_ptr(), 1, stream)

    def stage_plain():
        for _ in range(args.launches):
            lib.gatres_stage_observed(store.data.data_ptr(), 0, S, None, 64, NODES, BS, obs.data_ptr(), K, 0, 0.0, 1.0,
                                      x.data_ptr(), mask.data_ptr(), stream)

    def reduce():
        for _ in range(args.launches):
            lib.gatres_ensemble_reduce(scratch.data_ptr(), S, M, NODES, NODES, mean.data_ptr(), std.data_ptr(), S, NODES, 0, stream)

    def spread():
        for _ in range(args.launches):
            lib.gatres_node_spread_moments(std.data_ptr(), S, NODES, table.data_ptr(), stream)

    groups = [{"i ensemble S=2048 M=8": ensemble, "i 8 plain passes": plain},
              {"ii estimate_ensemble S=1 M=32": online, "ii estimate of 32 snapshots": online_plain},
              {"iii stage_observed_noisy": stage_noisy, "iii stage_observed": stage_plain, "iii ensemble_reduce": reduce,
               "iii node_spread_moments": spread}]
    times = {}
    for group in groups:
        for fn in group.values():                                   # warm-up: plans, buffers, code objects
            fn(); fn()
    torch.cuda.synchronize()
    for group in groups:
        names = list(group)
        for name in names:
            times[name] = []
        for rep in range(args.reps):
            for i in range(len(names)):                             # (the order rotates: no path always follows the same one)
                name = names[(i + rep) % len(names)]
                t0 = time.perf_counter()
                group[name]()
                torch.cuda.synchronize()
                times[name].append(time.perf_counter() - t0)

    # the draws against the host restatement
    zsrc = torch.zeros((64, NODES), dtype=torch.float32, device=dev)
    zx = torch.empty(64 * 16 * NODES, dtype=torch.float32, device=dev)
    zm = torch.empty(64 * 16 * NODES, dtype=torch.uint8, device=dev)
    zobs = torch.tensor(sensors[:16], dtype=torch.int32, device=dev)
    G._native.check(lib.gatres_stage_observed_noisy(zsrc.data_ptr(), 0, 64, 0, 16, 0, NODES, 64 * 16, zobs.data_ptr(), 16, 0, 0.0, 1.0,
                                                    zx.data_ptr(), zm.data_ptr(), None, 0, torch.ones(16, device=dev).data_ptr(),
                                                    20260, stream), "gatres_stage_observed_noisy")
    z = zx.view(64, 16, NODES)[:, :, sensors[:16]].double().cpu().numpy()
    dz = float(np.abs(z - G.estimation.reading_noise(20260, 16, 64, 16)).max())

    def us(name, per):
        ts = sorted(t * 1e6 / per for t in times[name])
        return statistics.median(ts), ts[0], ts[-1]

    pairs, batches = S * M, S * M // BS
    lines = ["Cost of a noise ensemble in PressureEstimator (tests/micro/estimate_ensemble_cost.py)",
             "=" * 96,
             f"MEASURED on {torch.cuda.get_device_name(0)}, torch {torch.__version__}; gatres_small (15 x 32), {NODES} nodes, bs {BS}, "
             f"{K} sensors, noise_std {SIGMA};",
             f"{args.reps} repetitions per path, the paths of a group taking turns in one process, one synchronise per repetition.", ""]
    a, b = "i ensemble S=2048 M=8", "i 8 plain passes"
    for name in (a, b):
        med, lo, hi = us(name, pairs)
        lines.append(f"  ({name}): median {med:.4f} us per pair ({med * BS:.2f} us per batch; {1e3 / med:.1f} k graphs/s; "
                     f"repetitions {lo:.4f} .. {hi:.4f})")
    paired = sorted((p - q) * 1e6 / batches for p, q in zip(times[a], times[b]))
    spread_b = (max(times[b]) - min(times[b])) * 1e6 / batches
    red = us("iii ensemble_reduce", args.launches)[0]
    d = statistics.median(paired)
    lines += [f"  (i) ensemble - plain: median {d:+.3f} us per batch = {d / BS:+.4f} us per pair (repetitions {paired[0]:+.3f} .. "
              f"{paired[-1]:+.3f} us per batch); spread of the plain passes (max - min): {spread_b:.3f} us per batch; the one reduce "
              f"launch of the pass: {red:.1f} us = {red / batches:.3f} us per batch",
              "  The ensemble enqueues the plain passes' launches with gatres_stage_observed_noisy as the staging launch, and one "
              "gatres_ensemble_reduce: the difference sits in the staging launch (iii) and the reduce.",
              ("  The difference is inside the spread of the repetitions plus the reduce launch's own time."
               if abs(d) <= spread_b + red / batches else
               "  The difference EXCEEDS the spread plus the reduce: see the staging launches under (iii) -- the noisy launch "
               "evaluates logf / sqrtf / cosf and two 64-bit hashes per present reading and divides the pair index."), ""]
    a, b = "ii estimate_ensemble S=1 M=32", "ii estimate of 32 snapshots"
    for name in (a, b):
        med, lo, hi = us(name, args.online_calls)
        lines.append(f"  ({name}): median {med:.2f} us per call of {BS} graphs ({med / BS:.3f} us per pair; repetitions {lo:.2f} .. {hi:.2f})")
    paired = sorted((p - q) * 1e6 / args.online_calls for p, q in zip(times[a], times[b]))
    lines += [f"  (ii) ensemble - plain: median {statistics.median(paired):+.2f} us per call (repetitions {paired[0]:+.2f} .. "
              f"{paired[-1]:+.2f}): four launches (staging, forward, write-back, reduce) against three", ""]
    for name in list(groups[2]):
        med, lo, hi = us(name, args.launches)
        lines.append(f"  ({name}): median {med:.2f} us per launch, {args.launches} back to back (repetitions {lo:.2f} .. {hi:.2f})")
    lines += [f"  the reduce reads {S * M * NODES * 4 / 1e6:.1f} MB twice (the second pass from L2 where it fits) and writes "
              f"{2 * S * NODES * 4 / 1e6:.1f} MB; the spread moments read {S * NODES * 4 / 1e6:.1f} MB", "",
              f"  device draws against reading_noise (fp64), 64 x 16 x 16 draws, seed 20260: max |dz| = {dz:.3e} (the test's bound: 1e-5)"]
    if args.bench_lines and os.path.exists(args.bench_lines):
        with open(args.bench_lines) as f:
            lines += ["", "  (iv) python bench.py --steps 20 --warmup 5, parent and change taking turns in the same job:"]
            lines += ["    " + ln.rstrip() for ln in f if ln.strip()]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
