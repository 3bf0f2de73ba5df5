"""What scoring sensor layouts costs PressureEstimator (not collected; writes profiles/layout_sweep_cost.txt).

gatres_small (15 x 32), 388 nodes, bs 32, S = 2 048 snapshots, 20 candidate sensors, L = 16 layouts.  The paths take turns in one
process (a rotating order inside each group), ``--reps`` times each, every repetition ending in one synchronise; medians, and the
range of the repetitions:
  (i)   ``layout_errors`` over the 16 layouts (32 768 pairs, 1 024 batches, one reduce launch, no read-back) against the same 16
        layouts through the existing calls: per layout ``estimate_store(available=...)`` + ``error_map(available=...)`` (64
        batches, one moments launch and one read-back each);
  (ii)  the three new launches alone, ``--launches`` back to back per repetition: gatres_stage_observed_layouts against
        gatres_stage_observed_available on the same batch, gatres_layout_pair_errors on one batch, gatres_layout_error_reduce on
        (i)'s records;
and the largest difference between the two paths' MAE per layout.  (iii), ``python bench.py --steps 20 --warmup 5`` at the parent
commit and at the change, three turns each in the same job, is run by the job that runs this script; ``--bench-lines FILE``
appends that job's lines to the report.
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

NODES, PIPES, BS, S, K, L = 388, 430, 32, 2048, 20, 16


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--bench-lines", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "layout_sweep_cost.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ei = G.wdn_synth.make_wdn_topology(NODES, PIPES, seed=0)
    raw = G.wdn_synth.make_snapshots(S, NODES, seed=1) * 12.5 + 50.0
    store = G.SnapshotStore(raw, ei, device=dev)
    torch.manual_seed(0)
    model = G.GATResMeanConv(num_blocks=15, nc=32).to(dev).eval()
    sensors = sorted(int(i) for i in torch.randperm(NODES, generator=torch.Generator().manual_seed(2))[:K])
    est = G.PressureEstimator.for_store(model, store, sensors, batch_size=BS)
    layouts = (torch.rand((L, K), generator=torch.Generator().manual_seed(3)) < 0.5).to(torch.uint8).to(dev)
    per_layout = [layouts[l].expand(S, K).contiguous() for l in range(L)]
    table = torch.empty((L, G._native.LAYOUT_ERROR_RECORD), dtype=torch.float64, device=dev)
    out = torch.empty((S, NODES), dtype=torch.float32, device=dev)
    lib = G._native.load()
    stream = G._native.current_stream(dev)
    x = torch.empty(BS * NODES, dtype=torch.float32, device=dev)
    mask = (torch.rand(BS * NODES, device=dev) < 0.95).to(torch.uint8)
    pred = torch.randn(BS * NODES, device=dev)
    rec = torch.rand((S * L, G._native.LAYOUT_PAIR_RECORD), dtype=torch.float64, device=dev)
    obs = est._observed
    maes = {}

    def sweep():
        est.layout_errors(store, layouts, out=table)

    def existing():
        got = []
        for l in range(L):
            est.estimate_store(store, out=out, available=per_layout[l])
            got.append(est.error_map(store, estimates=out, available=per_layout[l])["hidden_mae"])
        maes["existing"] = np.asarray(got)

    def stage_layouts():
        for _ in range(args.launches):
            lib.gatres_stage_observed_layouts(store.data.data_ptr(), 0, S, 64, L, NODES, BS, obs.data_ptr(), K, 0, 0.0, 1.0,
                                              x.data_ptr(), mask.data_ptr(), None, 0, layouts.data_ptr(), stream)

    def stage_available():
        for _ in range(args.launches):
            lib.gatres_stage_observed_available(store.data.data_ptr(), 0, S, None, 64, NODES, BS, obs.data_ptr(), K, 0, 0.0, 1.0,
                                                x.data_ptr(), mask.data_ptr(), per_layout[0].data_ptr(), 0, stream)

    def pair_errors():
        for _ in range(args.launches):
            lib.gatres_layout_pair_errors(pred.data_ptr(), mask.data_ptr(), store.data.data_ptr(), S, NODES, BS, 64, L, est.scale,
                                          est.offset, None, rec.data_ptr(), S * L, 64, stream)

    def reduce():
        for _ in range(args.launches):
            lib.gatres_layout_error_reduce(rec.data_ptr(), S, L, table.data_ptr(), 0, stream)

    groups = [{"i layout_errors L=16": sweep, "i 16 x (estimate_store + error_map)": existing},
              {"ii stage_observed_layouts": stage_layouts, "ii stage_observed_available": stage_available,
               "ii layout_pair_errors": pair_errors, "ii layout_error_reduce S=2048": reduce}]
    times = {}
    for group in groups[::-1]:                                      # warm-up: plans, buffers, code objects; (i) last: its table
        for fn in group.values():
            fn(); fn()
    torch.cuda.synchronize()
    maes["sweep"] = G.layout_scores_from_table(table.cpu().numpy())["mae"]
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

    def us(name, per):
        ts = sorted(t * 1e6 / per for t in times[name])
        return statistics.median(ts), ts[0], ts[-1]

    pairs, batches = S * L, S * L // BS
    lines = ["Cost of scoring sensor layouts in PressureEstimator (tests/micro/layout_sweep_cost.py)",
             "=" * 96,
             f"MEASURED on {torch.cuda.get_device_name(0)}, torch {torch.__version__}; gatres_small (15 x 32), {NODES} nodes, bs {BS}, "
             f"{S} snapshots, {K} candidate sensors, {L} layouts;",
             f"{args.reps} repetitions per path, the paths of a group taking turns in one process, one synchronise per repetition.", ""]
    a, b = "i layout_errors L=16", "i 16 x (estimate_store + error_map)"
    for name in (a, b):
        med, lo, hi = us(name, pairs)
        lines.append(f"  ({name}): median {med:.4f} us per pair ({med * BS:.2f} us per batch; {med * pairs / 1e3:.2f} ms per sweep; "
                     f"repetitions {lo:.4f} .. {hi:.4f})")
    paired = sorted((p - q) * 1e6 / batches for p, q in zip(times[a], times[b]))
    range_b = (max(times[b]) - min(times[b])) * 1e6 / batches
    d = statistics.median(paired)
    lines += [f"  (i) layout_errors - existing calls: median {d:+.3f} us per batch (repetitions {paired[0]:+.3f} .. {paired[-1]:+.3f}); "
              f"range of the existing-calls path (max - min): {range_b:.3f} us per batch",
              ("  layout_errors is not slower than the existing calls by more than the repetitions' range."
               if d <= range_b else
               "  layout_errors is SLOWER than the existing calls by more than the repetitions' range."),
              f"  largest |MAE(layout_errors) - MAE(existing calls)| over the {L} layouts: "
              f"{float(np.abs(maes['sweep'] - maes['existing']).max()):.3e} (MAE {float(maes['existing'].min()):.4f} .. "
              f"{float(maes['existing'].max()):.4f})", ""]
    for name in list(groups[1]):
        med, lo, hi = us(name, args.launches)
        lines.append(f"  ({name}): median {med:.2f} us per launch, {args.launches} back to back (repetitions {lo:.2f} .. {hi:.2f})")
    lines += [f"  the pair errors read {BS * NODES * 9 / 1e3:.1f} KB of the batch and {BS // L * NODES * 4 / 1e3:.1f} KB of truth rows "
              f"and write {BS * 32} bytes; the reduce reads {S * L * 32 / 1e6:.2f} MB of records, one lane per layout"]
    if args.bench_lines and os.path.exists(args.bench_lines):
        with open(args.bench_lines) as f:
            lines += ["", "  (iii) python bench.py --steps 20 --warmup 5, parent and change taking turns in the same job:"]
            lines += ["    " + ln.rstrip() for ln in f if ln.strip()]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
