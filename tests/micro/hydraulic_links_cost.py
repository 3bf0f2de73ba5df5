"""Cost of the links launches (csrc/k_hydraulic_links.hip), one JSON line per mode.  Not collected by pytest.

    python tests/micro/hydraulic_links_cost.py [--scenarios 2048] [--steps 24] [--repeats 5] [--modes solve,series]

On make_hydraulic_network(388, 430, 3): (a) gatres_hydraulic_solve; (b) gatres_hydraulic_solve_links on the same pipe-only inputs
(the same bits: the price of generality); (c) the links launch on the same network with num_pumps=4 and num_check_valves=20,
with the mean iterations per scenario; (d) (a) and (b) for the series at --steps steps.  The sides take turns in one process;
medians of --repeats with their ranges, timed with device events around one launch each.  ``--modes solve,series`` runs the
pipe-only launches alone and touches nothing that an older tree lacks: copied into a checkout of the parent commit, it gives the
parent's side of (a)."""
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
    ap.add_argument("--modes", default="")
    a = ap.parse_args()
    net = G.wdn_synth.make_hydraulic_network(388, 430, 3, seed=6, device="cuda:0")
    ranges = [torch.from_numpy(r).to("cuda:0") for r in net.draw_ranges((1e-5, 1e-3), H.ROUGHNESS_RANGE)]
    demand, roughness = net.draw(a.scenarios, 1, 0, *ranges)
    want = [m for m in a.modes.split(",") if m]
    links = None
    if not want or "solve_links_4_pumps_20_cv" in want:
        links = G.wdn_synth.make_hydraulic_network(388, 430, 3, seed=6, device="cuda:0", num_pumps=4, num_check_valves=20)
    mult = torch.ones((1, a.steps), dtype=torch.float64, device="cuda:0")
    modes = {"solve": lambda: net.simulate(demand, roughness, want_head=False, want_flow=False),
             "solve_links_pipe_only": lambda: net.simulate(demand, roughness, want_head=False, want_flow=False, links=True),
             "solve_links_4_pumps_20_cv": lambda: links.simulate(demand, roughness, want_head=False, want_flow=False),
             "series": lambda: net.simulate_series(demand, roughness, mult, step_seconds=300.0, want_head=False, want_flow=False),
             "series_links_pipe_only": lambda: net.simulate_series(demand, roughness, mult, step_seconds=300.0, want_head=False,
                                                                   want_flow=False, links=True)}
    for name, fn in modes.items():
        if want and name not in want:
            continue
        t, out = timed(fn, a.repeats)
        t.update({"mode": name, "scenarios": a.scenarios, "mean_iterations": float(out.iterations.double().mean()),
                  "converged": float(out.converged.double().mean())})
        print(json.dumps(t))


if __name__ == "__main__":
    main()
