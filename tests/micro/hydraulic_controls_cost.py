"""Cost of the series launch with THE CONTROLS (csrc/k_hydraulic_network.hip, hydraulic_series_network_kernel<LV, true>), one JSON line
per mode.  Not collected by pytest.

    python tests/micro/hydraulic_controls_cost.py [--series 2048] [--steps 24] [--repeats 7] [--pdd-only] [--library PATH]

On make_hydraulic_network(388, 430, 3) with two pumps and two tanks, as a warm series: (a) gatres_hydraulic_series_pdd,
demand-driven; (b) gatres_hydraulic_series_controls with an empty table on the same inputs (the same bits: the price of the launch
itself -- the control pass over no control and its barrier, the state words); (c) the same launch with a pump / tank table (every pump
CLOSED above a level of every tank and OPEN below another), with the mean iterations and the control changes beside it, since
switching costs iterations as well as time per iteration.  The sides take turns in one process, round after round; medians of
--repeats with their ranges, timed with device events around one launch each.  ``--pdd-only`` times (a) alone: that is what a
checkout of the parent commit can run, for the comparison across the change; ``--library`` takes another build of the library
(the parent's) in place of the tree's own, through ``_native.load_unchecked``."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import gnn_pressure_estimation_amd as G  # noqa: E402

H = G.hydraulics


def one(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--series", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--pdd-only", action="store_true")
    ap.add_argument("--library", default=None)
    a = ap.parse_args()
    if a.library:
        G._native.load_unchecked(a.library)
    net = G.wdn_synth.make_hydraulic_network(388, 430, 3, seed=6, num_pumps=2, num_tanks=2, device="cuda:0")
    ranges = [torch.from_numpy(r).to("cuda:0") for r in net.draw_ranges((1e-5, 1e-3), H.ROUGHNESS_RANGE)]
    demand, roughness = net.draw(a.series, 1, 0, *ranges)
    mult = torch.from_numpy(G.wdn_synth.make_demand_patterns(1, a.steps, 300.0, 6)).to("cuda:0")
    kw = dict(step_seconds=300.0, want_head=False, want_flow=False, demand_model="dda")
    modes = {"series_pdd": lambda: net.simulate_series(demand, roughness, mult, **kw)}
    if not a.pdd_only:
        level = net.fixed_head[net.tank_nodes] - net.elevation[net.tank_nodes]
        rows = []
        for p in net.pump_links:
            for k in range(net.num_tanks):
                rows += [(int(p), "closed", "tank_above", k, float(level[k]) + 0.02), (int(p), "open", "tank_below", k, float(level[k]) - 0.02)]
        empty, table = H.control_table(net, []), H.control_table(net, rows)
        modes["series_controls_empty_table"] = lambda: net.simulate_series(demand, roughness, mult, controls=empty, **kw)
        modes["series_controls_pump_tank_table"] = lambda: net.simulate_series(demand, roughness, mult, controls=table, **kw)
    ms, last = {m: [] for m in modes}, {}
    for fn in modes.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(a.repeats):                              # the sides take turns
        for name, fn in modes.items():
            t, last[name] = one(fn)
            ms[name].append(t)
    for name, out in last.items():
        alive = ~out.failed
        t = {"mode": name, "series": a.series, "steps": a.steps, "median_ms": float(np.median(ms[name])), "min_ms": min(ms[name]),
             "max_ms": max(ms[name]), "mean_iterations": float(out.iterations[alive].double().mean()),
             "max_iterations": int(out.iterations.max()), "converged": float(out.converged.double().mean()),
             "limited": float(out.limited.double().mean())}
        if hasattr(out, "control_changes"):
            t["control_changes_per_series"] = float(out.control_changes.double().sum(dim=1).mean())
        print(json.dumps(t), flush=True)


if __name__ == "__main__":
    main()
