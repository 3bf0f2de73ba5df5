"""What PressureEstimator's sensitivity pass costs (not collected; writes profiles/sensitivity_cost.txt).

gatres_small (15 x 32), 388 nodes, bs 32, 20 sensors: the full Jacobian (388 target junctions) of ``--snapshots`` snapshots, that
is ceil(388 S / 32) batches of staging, forward, backward and gather.  The paths take turns in one process, ``--reps`` times each,
every repetition ending in one synchronise; medians and ranges:
  (a) ``PressureEstimator.sensitivity_store``: four launches per batch, buffers kept on the estimator;
  (b) the hand-written torch loop through the module on the same batches: zeros, index_put, a seed, ``x1.requires_grad_()``,
      ``model(x1, edge_index)``, ``out.backward(seed)``, ``x1.grad`` at the sensors;
  (c) the two new launches of a batch back to back, without the model;
  (d) ``linear_spread`` of ONE snapshot beside (e) ``estimate_ensemble`` of 32 members of it.
The one condition: (a) is not slower than (b), judged against (b)'s own repetition range.  Last, as an observation, the linearised
spread beside the Monte-Carlo standard deviation of 1 024 members."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import gnn_pressure_estimation_amd as G      # noqa: E402

NODES, PIPES, BS, K, MEMBERS, NOISE = 388, 430, 32, 20, 32, 0.1


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--snapshots", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sensitivity_cost.txt"))
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
    obs = torch.tensor(sensors, device=dev)
    readings = raw.to(dev)[:, sensors].contiguous()
    pairs = S * NODES
    batches = (pairs + BS - 1) // BS
    J = torch.empty((S, NODES, K), dtype=torch.float32, device=dev)
    Jb = torch.empty((pairs, K), dtype=torch.float32, device=dev)
    spread = torch.empty((1, NODES), dtype=torch.float32, device=dev)
    mean, std = (torch.empty((1, NODES), dtype=torch.float32, device=dev) for _ in range(2))
    unit = torch.tensor(est.scale / (est.std + est.eps), dtype=torch.float32, device=dev)
    lib = G._native.load()
    stream = G._native.current_stream(dev)

    def a():
        est.sensitivity_store(store, out=J)

    def b():
        for first in range(0, pairs, BS):
            g = min(BS, pairs - first)
            pair = torch.arange(first, first + g, device=dev)
            row, t = pair // NODES, pair % NODES
            rows = store.data[row]
            x1 = torch.zeros_like(rows)
            x1[:, obs] = rows[:, obs]
            seed = torch.zeros_like(rows)
            seed[torch.arange(g, device=dev), t] = 1.0
            x1 = x1.view(-1, 1).requires_grad_()
            out = model(x1, store.edge_index(g), None, None)
            out.backward(seed.view(-1, 1))
            Jb[first:first + g] = x1.grad.view(g, NODES)[:, obs] * unit

    def c():
        for first in range(0, pairs, BS):
            g = min(BS, pairs - first)
            P = G.evaluation._eval_plan(model, store, g)
            _, g_out, g_x, _ = est._sensitivity_buffers(P)
            lib.gatres_stage_observed_targets(store.data.data_ptr(), 0, S, first, NODES, None, NODES, g, est._observed.data_ptr(),
                                              K, 0, 0.0, 1.0, P.x.data_ptr(), P.mask.data_ptr(), g_out.data_ptr(), None, 0, stream)
            lib.gatres_sensitivity_gather(g_x.data_ptr(), P.mask.data_ptr(), None, NODES, g, est._observed.data_ptr(), K, 1.0,
                                          J.data_ptr(), pairs, K, first, stream)

    def d():
        est.linear_spread(readings[:1], NOISE, out=spread)

    def e():
        est.estimate_ensemble(readings[:1], NOISE, MEMBERS, seed=7, mean_out=mean, std_out=std)

    paths = {"a sensitivity_store": a, "b torch loop through the module": b, "c the two new launches alone": c,
             "d linear_spread, one snapshot": d, "e estimate_ensemble, 32 members, one snapshot": e}
    times = {k: [] for k in paths}
    for fn in paths.values():                                       # warm-up: plans, buffers, code objects
        fn(); fn()
    torch.cuda.synchronize()
    for _ in range(args.reps):
        for name, fn in paths.items():
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    b()
    a()
    same = torch.equal(J.view(pairs, K), Jb)
    lines = ["Cost of PressureEstimator's sensitivity pass (tests/micro/sensitivity_cost.py)",
             "=" * 96,
             f"MEASURED on {torch.cuda.get_device_name(0)}, torch {torch.__version__}; gatres_small (15 x 32), {NODES} nodes, bs {BS}, "
             f"{K} sensors;",
             f"the full Jacobian ({NODES} targets) of {S} snapshots = {pairs} pairs = {batches} batches; {args.reps} repetitions per "
             "path,", "the paths taking turns in one process, one synchronise per repetition.", ""]
    med = {}
    for name, ts in times.items():
        med[name] = statistics.median(ts)
        lines.append(f"  ({name}): median {med[name] * 1e3:9.3f} ms  (min {min(ts) * 1e3:.3f} / max {max(ts) * 1e3:.3f} ms)")
    ma, mb, mc, md, me = (med[k] for k in paths)
    tb = times["b torch loop through the module"]
    holds = ma <= max(tb)
    lines += ["",
              f"  the pass:  {ma * 1e3 / S:8.3f} ms per snapshot, {ma * 1e6 / pairs:7.2f} us per pair, {ma * 1e3 / batches:.4f} ms per batch",
              f"  the loop:  {mb * 1e3 / S:8.3f} ms per snapshot, {mb * 1e6 / pairs:7.2f} us per pair, {mb * 1e3 / batches:.4f} ms per batch",
              f"  the pass against the loop: {mb / ma:.2f} x the pairs/s  (loop range {min(tb) * 1e3:.3f} .. {max(tb) * 1e3:.3f} ms)",
              f"  CONDITION the pass is not slower than the loop (median {ma * 1e3:.3f} ms <= the loop's slowest {max(tb) * 1e3:.3f} ms"
              f" and its median {mb * 1e3:.3f} ms): {'HOLDS' if holds and ma <= mb else 'holds against the range only' if holds else 'VIOLATED'}",
              f"  rows of (a) and (b) bit-identical: {same}",
              f"  the two new launches: {mc * 1e3 / batches:.4f} ms per batch, {mc / ma * 100:.1f} % of the pass",
              f"  linear_spread of one snapshot ({(NODES + BS - 1) // BS} batches, forward and backward): {md * 1e3:.3f} ms; estimate_ensemble "
              f"of {MEMBERS} members (1 batch, forward): {me * 1e3:.3f} ms; ratio {md / me:.1f} x"]
    # observation: first order against Monte Carlo
    M = 1024
    _, mc_std = est.estimate_ensemble(readings[:1], NOISE, M, seed=11)
    lin = est.linear_spread(readings[:1], NOISE)
    hidden = torch.ones(NODES, dtype=torch.bool, device=dev)
    hidden[obs] = False                                             # (keep_observed: the ensemble's sensor nodes carry the noisy reading)
    ratio = (lin[0, hidden] / mc_std[0, hidden].clamp_min(1e-12)).cpu()
    lines += ["",
              f"OBSERVATION (not asserted): noise_std {NOISE} m at every sensor, snapshot 0, the {int(hidden.sum())} junctions without a sensor:",
              f"  linear_spread / std of {M} Monte-Carlo members: median {float(ratio.median()):.4f}, min {float(ratio.min()):.4f}, max "
              f"{float(ratio.max()):.4f}  (sampling error of the Monte-Carlo std: about {1 / (2 * (M - 1)) ** 0.5:.3f} relative)",
              f"  largest linear spread {float(lin[0, hidden].max()):.5f} m, largest Monte-Carlo std {float(mc_std[0, hidden].max()):.5f} m"]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
