"""Cost of the emitters launches (csrc/k_hydraulic_network.hip, LV 1), one JSON line per mode.  Not collected by pytest.

    python tests/micro/hydraulic_emitters_cost.py [--scenarios 2048] [--steps 24] [--repeats 5] [--emitters 8] [--valves-only]

On make_hydraulic_network(388, 430, 3): (a) gatres_hydraulic_solve_valves on pipe-only inputs; (b) gatres_hydraulic_solve_emitters on
the same inputs, with no emitter (the same bits: the price of the emitters' empty loops); (c) the emitters launch on the same
network with --emitters emitters, every one leaking, with the mean iterations and the mean leaked share of the inflow; (d) (a),
(b) and (c) for the series at --steps steps, the leaks beginning at --steps / 2.  The sides take turns in one process; medians of
--repeats with their ranges, timed with device events around one launch each.  ``--valves-only`` times (a) and its series alone:
that is what a checkout of the parent commit can run, for the comparison across the change."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import gnn_pressure_estimation_amd as G  # noqa: E402

H = G.hydraulics


def timed(fn, repeats):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": float(np.median(ms)), "min_ms": min(ms), "max_ms": max(ms)}, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenarios", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--emitters", type=int, default=8)
    ap.add_argument("--valves-only", action="store_true")
    a = ap.parse_args()
    net = G.wdn_synth.make_hydraulic_network(388, 430, 3, seed=6, device="cuda:0")
    ranges = [torch.from_numpy(r).to("cuda:0") for r in net.draw_ranges((1e-5, 1e-3), H.ROUGHNESS_RANGE)]
    demand, roughness = net.draw(a.scenarios, 1, 0, *ranges)
    mult = torch.ones((1, a.steps), dtype=torch.float64, device="cuda:0")
    kw = dict(want_head=False, want_flow=False)
    series = dict(step_seconds=300.0, **kw)
    modes = {"solve_valves_no_valve": lambda: net.simulate(demand, roughness, valves=True, **kw),
             "series_valves_no_valve": lambda: net.simulate_series(demand, roughness, mult, valves=True, **series)}
    if not a.valves_only:
        leaky = G.wdn_synth.make_hydraulic_network(388, 430, 3, seed=6, device="cuda:0", num_emitters=a.emitters)
        coef = torch.full((a.emitters,), 1e-4, dtype=torch.float64, device="cuda:0")
        onset = torch.full((a.emitters,), a.steps // 2, dtype=torch.int32, device="cuda:0")
        modes = {"solve_valves_no_valve": modes["solve_valves_no_valve"],
                 "solve_emitters_no_emitter": lambda: net.simulate(demand, roughness, emitters=True, **kw),
                 f"solve_emitters_{a.emitters}": lambda: leaky.simulate(demand, roughness, emitter_coefficient=coef, **kw),
                 "series_valves_no_valve": modes["series_valves_no_valve"],
                 "series_emitters_no_emitter": lambda: net.simulate_series(demand, roughness, mult, emitters=True, **series),
                 f"series_emitters_{a.emitters}": lambda: leaky.simulate_series(demand, roughness, mult, emitter_coefficient=coef,
                                                                               emitter_onset=onset, **series)}
    for name, fn in modes.items():
        t, out = timed(fn, a.repeats)
        t.update({"mode": name, "scenarios": a.scenarios, "mean_iterations": float(out.iterations.double().mean()),
                  "converged": float(out.converged.double().mean())})
        if hasattr(out, "emitter_flow") and out.emitter_flow.numel():
            t["mean_leak_m3s"] = float(out.emitter_flow.sum(dim=-1).mean())
        print(json.dumps(t), flush=True)


if __name__ == "__main__":
    main()
