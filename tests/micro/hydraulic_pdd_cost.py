"""Cost of the pressure-driven demand launches (csrc/k_hydraulic_network.hip, LV 2), one JSON line per mode.  Not collected by pytest.

    python tests/micro/hydraulic_pdd_cost.py [--scenarios 2048] [--steps 24] [--repeats 5] [--required 20] [--emitters-only]

On make_hydraulic_network(388, 430, 3): (a) gatres_hydraulic_solve_emitters on pipe-only inputs, no emitter; (b)
gatres_hydraulic_solve_pdd on the same inputs with demand_model 0 (the same bits: the price of the launch itself); (c) the same
launch pressure-driven (Pmin 0, Preq --required metres, exponent 0.5), with the mean iterations and the delivered share of the
demand beside it, since pressure-driven demand costs iterations as well as time per iteration; (d) (a), (b) and (c) for the warm
series at --steps steps.  The sides take turns in one process; medians of --repeats with their ranges, timed with device events
around one launch each.  ``--emitters-only`` times (a) and its series alone: that is what a checkout of the parent commit can
run, for the comparison across the change."""
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
    ap.add_argument("--required", type=float, default=20.0)
    ap.add_argument("--emitters-only", action="store_true")
    a = ap.parse_args()
    net = G.wdn_synth.make_hydraulic_network(388, 430, 3, seed=6, device="cuda:0")
    ranges = [torch.from_numpy(r).to("cuda:0") for r in net.draw_ranges((1e-5, 1e-3), H.ROUGHNESS_RANGE)]
    demand, roughness = net.draw(a.scenarios, 1, 0, *ranges)
    mult = torch.ones((1, a.steps), dtype=torch.float64, device="cuda:0")
    kw = dict(want_head=False, want_flow=False)
    series = dict(step_seconds=300.0, **kw)
    modes = {"solve_emitters_no_emitter": lambda: net.simulate(demand, roughness, emitters=True, **kw),
             "series_emitters_no_emitter": lambda: net.simulate_series(demand, roughness, mult, emitters=True, **series)}
    if not a.emitters_only:
        pda = dict(demand_model="pda", required_pressure=a.required)
        modes = {"solve_emitters_no_emitter": modes["solve_emitters_no_emitter"],
                 "solve_pdd_demand_driven": lambda: net.simulate(demand, roughness, demand_model="dda", **kw),
                 "solve_pdd_pressure_driven": lambda: net.simulate(demand, roughness, **pda, **kw),
                 "series_emitters_no_emitter": modes["series_emitters_no_emitter"],
                 "series_pdd_demand_driven": lambda: net.simulate_series(demand, roughness, mult, demand_model="dda", **series),
                 "series_pdd_pressure_driven": lambda: net.simulate_series(demand, roughness, mult, **pda, **series)}
    for name, fn in modes.items():
        t, out = timed(fn, a.repeats)
        t.update({"mode": name, "scenarios": a.scenarios, "mean_iterations": float(out.iterations.double().mean()),
                  "max_iterations": int(out.iterations.max()), "converged": float(out.converged.double().mean())})
        if hasattr(out, "demand_delivered"):
            full = demand if out.demand_delivered.dim() == 2 else demand[:, None, :]
            t["delivered_share"] = float(out.demand_delivered.nansum() / (full.sum() * (out.demand_delivered.numel() // demand.numel())))
        print(json.dumps(t), flush=True)


if __name__ == "__main__":
    main()
