"""What PressureEstimator's drift monitor costs (not collected; writes profiles/monitor_cost.txt).

gatres_small (15 x 32), 388 nodes, bs 32, 20 sensors, ``--snapshots`` snapshots (2 048) read as one series.  The paths take turns
in one process, ``--reps`` times each, every repetition ending in one synchronise; medians and ranges:
  (a) ``PressureEstimator.monitor_store``, one round, one series: the leave-one-out pass, ``gatres_cusum_scan`` and
      ``gatres_monitor_latch``;
  (b) ``loo_residuals_store`` alone on the same data; (b2) the same under an all-ones availability, the pass that every round
      but round 0 of complete readings runs;
  (c) the two new launches alone, back to back, at T = ``--snapshots`` and at T = 105 120 (a year of 5-minute readings), K = 20.
The one condition: (a) - (b) lies inside (b)'s own range over its repetitions, or is explained by (c).  The benchmark comparison
(d) is a separate job: ``python bench.py --steps 20 --warmup 5`` at the parent and at the change, three turns each."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import gnn_pressure_estimation_amd as G      # noqa: E402

NODES, PIPES, BS, K, YEAR = 388, 430, 32, 20, 105120


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--snapshots", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "monitor_cost.txt"))
    args = ap.parse_args()
    S = args.snapshots
    dev = torch.device("cuda:0")
    ei = G.wdn_synth.make_wdn_topology(NODES, PIPES, seed=0)
    raw = G.wdn_synth.make_snapshots(S, NODES, seed=1) * 12.5 + 50.0
    store = G.SnapshotStore(raw, ei, device=dev)
    torch.manual_seed(0)
    model = G.GATResMeanConv(num_blocks=15, nc=32).to(dev).eval()
    sensors = sorted(int(i) for i in torch.randperm(NODES, generator=torch.Generator().manual_seed(2))[:K])
    est = G.PressureEstimator.for_store(model, store, sensors, batch_size=BS)
    mb = est.calibrate_monitor(store)
    lib = G._native.load()
    stream = G._native.current_stream(dev)
    kq, hq = G.cusum_fixed(0.5), G.cusum_fixed(5.0)

    def launches(T):
        g = torch.Generator().manual_seed(3)
        resid = torch.randn((T, K), generator=g).to(dev)
        avail = torch.ones((T, K), dtype=torch.uint8, device=dev)
        state = torch.empty((1, K, 4), dtype=torch.int64, device=dev)
        records = torch.empty((1, K, 6), dtype=torch.int64, device=dev)
        latched = torch.empty((1, 1), dtype=torch.int32, device=dev)
        latched_rec = torch.empty((1, 1, 6), dtype=torch.int64, device=dev)
        mu, inv = torch.zeros(K, device=dev), torch.ones(K, device=dev)

        def run():
            G._native.check(lib.gatres_cusum_scan(resid.data_ptr(), mu.data_ptr(), inv.data_ptr(), avail.data_ptr(), T, K, T, 0, kq, hq,
                                                  None, state.data_ptr(), records.data_ptr(), None, None, stream), "gatres_cusum_scan")
            G._native.check(lib.gatres_monitor_latch(records.data_ptr(), avail.data_ptr(), T, K, T, 0, 0, 1, 0, 1, latched.data_ptr(),
                                                     latched_rec.data_ptr(), stream), "gatres_monitor_latch")
        return run

    ones = torch.ones((S, K), dtype=torch.uint8, device=dev)
    paths = {"a monitor_store": lambda: est.monitor_store(store, mb),
             "b loo_residuals_store": lambda: est.loo_residuals_store(store),
             "b2 loo_residuals_store, all-ones availability": lambda: est.loo_residuals_store(store, available=ones),
             f"c the two new launches alone, T = {S}": launches(S),
             f"c the two new launches alone, T = {YEAR}": launches(YEAR)}
    times = {k: [] for k in paths}
    for fn in paths.values():                                       # warm-up: plans, scratch, code objects
        fn(); fn()
    torch.cuda.synchronize()
    for _ in range(args.reps):
        for name, fn in paths.items():
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    lines = ["Cost of PressureEstimator's drift monitor (tests/micro/monitor_cost.py)",
             "=" * 96,
             f"MEASURED on {torch.cuda.get_device_name(0)}, torch {torch.__version__}; gatres_small (15 x 32), {NODES} nodes, bs {BS}, "
             f"{K} sensors,",
             f"{S} snapshots as one series; {args.reps} repetitions per path, the paths taking turns in one process, one synchronise",
             "per repetition.", ""]
    med = {}
    for name, ts in times.items():
        med[name] = statistics.median(ts)
        lines.append(f"  ({name}): median {med[name] * 1e3:9.3f} ms  (min {min(ts) * 1e3:.3f} / max {max(ts) * 1e3:.3f} ms)")
    ma, mb_, mb2, mc, _ = (med[k] for k in paths)
    tb = times["b loo_residuals_store"]
    spread_b = max(tb) - min(tb)
    inside, explained = abs(ma - mb_) <= spread_b, abs(ma - mb_ - mc) <= spread_b
    lines += ["",
              f"  (a) - (b) = {(ma - mb_) * 1e3:+.3f} ms ({(ma / mb_ - 1) * 100:+.2f} %); (b)'s range over its repetitions: "
              f"{spread_b * 1e3:.3f} ms ({min(tb) * 1e3:.3f} .. {max(tb) * 1e3:.3f} ms); (c) at T = {S}: {mc * 1e3:.3f} ms",
              f"  CONDITION (a) - (b) lies inside (b)'s own range, or is explained by (c): "
              f"{'HOLDS' if inside or explained else 'VIOLATED'} (inside the range: {inside}; within the range of (c): {explained})"]
    lines.append(f"  (b2) - (b) = {(mb2 - mb_) * 1e3:+.3f} ms: what an availability costs the pass; (a) - (b) - (c) = "
                 f"{(ma - mb_ - mc) * 1e3:+.3f} ms: the host side of monitor_store (checks, one fill, two ctypes calls) and noise")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
