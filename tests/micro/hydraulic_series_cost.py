"""Cost of the hydraulic series (csrc/k_hydraulics.hip: gatres_hydraulic_series), one JSON line.  Not collected by pytest.

    python tests/micro/hydraulic_series_cost.py [--series 2048] [--steps 24] [--reps 5]

388 nodes / 430 pipes / 3 reservoirs + 2 tanks; three ways to the same day of ``--steps`` steps of 300 s, taking turns in one
process:
  (a) warm    one series launch, every step started from the flows of the step before;
  (b) cold    one series launch, every step started from the starting flows;
  (c) steps   what the steady kernel alone can do: one ``simulate`` launch per step, with demand * multiplier, the tank heads and
              the level update written in torch between the launches (cold starts: ``simulate`` takes no starting flows).
The kernels' registers and scratch are the compiler's (-Rpass-analysis=kernel-resource-usage on k_hydraulics.hip)."""
import argparse
import json
import os
import statistics
import sys

NODES, PIPES, FIXED, TANKS = 388, 430, 5, 2
DEMAND_RANGE = (1e-5, 1e-4)
DT = 300.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--series", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    import numpy as np
    import torch
    import gnn_pressure_estimation_amd as G
    assert torch.cuda.is_available(), "needs the MI355X"
    H = G.hydraulics
    S, T = args.series, args.steps
    net = G.wdn_synth.make_hydraulic_network(NODES, PIPES, FIXED, seed=6, elevation_range=(0.0, 40.0), num_tanks=TANKS, device="cuda:0")
    demand, roughness = (torch.from_numpy(a).cuda() for a in H.hydraulic_draws(1, 0, S, *net.draw_ranges(DEMAND_RANGE, H.ROUGHNESS_RANGE)))
    mult = torch.from_numpy(G.wdn_synth.make_demand_patterns(3, T, DT, 2)).cuda()
    pattern = torch.from_numpy((np.arange(NODES) % 3).astype(np.int32)).cuda()
    st = net.static()
    tanks = st["tank_node"].long()
    elev_t, area = st["elevation"][tanks], st["tank_area"]
    level0 = (st["fixed_head"][tanks] - elev_t)[None, :].expand(S, TANKS).contiguous()
    into = torch.stack([(st["pipe_b"].long() == n).double() - (st["pipe_a"].long() == n).double() for n in tanks.tolist()], dim=1)   # [P, K]

    def series(warm):
        return net.simulate_series(demand, roughness, mult, step_seconds=DT, initial_level=level0, pattern_of_node=pattern,
                                   warm_start=warm, want_head=False)

    def step_by_step():
        level, heads, iters = level0, st["fixed_head"][None, :].repeat(S, 1), 0
        for t in range(T):
            heads[:, tanks] = elev_t[None, :] + level
            res = net.simulate(demand * mult[:, t][pattern.long()][None, :], roughness, heads, want_head=False)
            level = torch.minimum(torch.maximum(level + (res.flow @ into) * DT / area[None, :], st["tank_min"][None, :]), st["tank_max"][None, :])
            iters = iters + res.iterations.sum()
        return level, iters

    for f in (lambda: series(True), lambda: series(False), step_by_step):      # untimed: uploads, the LDS attribute, allocations
        f()
    torch.cuda.synchronize()
    ms = {"warm": [], "cold": [], "steps": []}
    for _ in range(args.reps):                                                  # taking turns
        for key, f in (("warm", lambda: series(True)), ("cold", lambda: series(False)), ("steps", step_by_step)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = f()
            b.record()
            torch.cuda.synchronize()
            ms[key].append(a.elapsed_time(b))
    warm, cold = series(True), series(False)
    level_c, iters_c = step_by_step()
    line = {"nodes": NODES, "pipes": PIPES, "reservoirs": FIXED - TANKS, "tanks": TANKS, "half_bandwidth": net.half_bandwidth,
            "series": S, "steps": T, "lds_bytes": H.series_lds_bytes(NODES, PIPES, net.half_bandwidth, TANKS),
            "build": G._native.load().gatres_version().decode(), "device": torch.cuda.get_device_name(0)}
    for key in ms:
        line[f"{key}_ms"] = [round(m, 2) for m in ms[key]]
        line[f"{key}_ms_median"] = round(statistics.median(ms[key]), 2)
        line[f"{key}_ms_range"] = [round(min(ms[key]), 2), round(max(ms[key]), 2)]
    line.update({"warm_mean_iterations_per_step": float(warm.iterations.double().mean()),
                 "cold_mean_iterations_per_step": float(cold.iterations.double().mean()),
                 "steps_mean_iterations_per_step": float(iters_c) / (S * T),
                 "warm_converged_steps": int(warm.converged.sum()), "cold_converged_steps": int(cold.converged.sum()),
                 "limited_steps": int(warm.limited.sum()), "failed_steps": int(warm.failed.sum()),
                 "cold_level_equals_step_by_step": bool(torch.equal(cold.level[:, -1], level_c)),
                 "steps_over_warm": round(statistics.median(ms["steps"]) / statistics.median(ms["warm"]), 3),
                 "cold_over_warm": round(statistics.median(ms["cold"]) / statistics.median(ms["warm"]), 3)})
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
