"""Cost of the valves launches (csrc/k_hydraulic_network.hip, LV 0), one JSON line per mode.  Not collected by pytest.

    python tests/micro/hydraulic_valves_cost.py [--scenarios 1024] [--steps 24] [--repeats 5]

On make_hydraulic_network(388, 430, 3): (a) gatres_hydraulic_solve_links on pipe-only inputs; (b) gatres_hydraulic_solve_valves on
the same inputs, with no valve (the same bits: the price of the status machine's barriers and loops); (c) the valves launch on
the same network with num_prvs=2 and num_psvs=1, at the settings the network was built with, with the mean iterations and status
changes per scenario; (d) (a) and (b) for the series at --steps steps.  The sides take turns in one process; medians of --repeats
with their ranges, timed with device events around one launch each."""
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
    ap.add_argument("--scenarios", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    net = G.wdn_synth.make_hydraulic_network(388, 430, 3, seed=6, device="cuda:0")
    valved = G.wdn_synth.make_hydraulic_network(388, 430, 3, seed=6, device="cuda:0", num_prvs=2, num_psvs=1, valve_seed=2)
    ranges = [torch.from_numpy(r).to("cuda:0") for r in net.draw_ranges((1e-5, 1e-3), H.ROUGHNESS_RANGE)]
    demand, roughness = net.draw(a.scenarios, 1, 0, *ranges)
    mult = torch.ones((1, a.steps), dtype=torch.float64, device="cuda:0")
    kw = dict(want_head=False, want_flow=False)
    modes = {"solve_links_pipe_only": lambda: net.simulate(demand, roughness, links=True, **kw),
             "solve_valves_no_valve": lambda: net.simulate(demand, roughness, valves=True, **kw),
             "solve_valves_2_prv_1_psv": lambda: valved.simulate(demand, roughness, **kw),
             "series_links_pipe_only": lambda: net.simulate_series(demand, roughness, mult, step_seconds=300.0, links=True, **kw),
             "series_valves_no_valve": lambda: net.simulate_series(demand, roughness, mult, step_seconds=300.0, valves=True, **kw),
             "series_valves_2_prv_1_psv": lambda: valved.simulate_series(demand, roughness, mult, step_seconds=300.0, **kw)}
    for name, fn in modes.items():
        t, out = timed(fn, a.repeats)
        t.update({"mode": name, "scenarios": a.scenarios, "mean_iterations": float(out.iterations.double().mean()),
                  "converged": float(out.converged.double().mean())})
        if hasattr(out, "valve_changes"):
            t["mean_valve_changes"] = float(out.valve_changes.double().mean())
        print(json.dumps(t))


if __name__ == "__main__":
    main()
