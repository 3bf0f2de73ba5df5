"""Cost of the sensitivity launch (csrc/k_hydraulic_sensitivity.hip), one JSON line per mode and sensor count.  Not collected by
pytest.

    python tests/micro/hydraulic_sensitivity_cost.py [--scenarios 2048] [--sensors 20,42] [--repeats 5]

On make_hydraulic_network(388, 430, 3): (a) ``sensitivity`` with every output (dh_ddemand and dh_droughness); (b) ``localize_leaks``
without dh_ddemand (the fused path: no [S, K, N] in memory); (c) ``simulate(links=True)`` on the same inputs, the launch both
contain; (d) the finite-difference alternative, priced as (N + 1) x (c).  K = 20 is one chunk on this network, K = 42 two.  The modes
take turns in one process, --repeats turns; medians with their ranges, timed with device events around one launch each."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import gnn_pressure_estimation_amd as G  # noqa: E402

H = G.hydraulics


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenarios", type=int, default=2048)
    ap.add_argument("--sensors", default="20,42")
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    net = G.wdn_synth.make_hydraulic_network(388, 430, 3, seed=6, device="cuda:0")
    ranges = [torch.from_numpy(r).to("cuda:0") for r in net.draw_ranges((1e-5, 1e-3), H.ROUGHNESS_RANGE)]
    demand, roughness = net.draw(a.scenarios, 1, 0, *ranges)
    N, P, W = net.num_nodes, net.num_pipes, net.half_bandwidth
    for K in (int(k) for k in a.sensors.split(",")):
        sensors = np.sort(np.random.RandomState(K).permutation(net.junctions)[:K])
        readings = torch.full((a.scenarios, K), 30.0, dtype=torch.float64, device="cuda:0")
        modes = {"sensitivity_all_outputs": lambda: net.sensitivity(demand, roughness, sensors, want_roughness=True),
                 "localize_leaks_fused": lambda: net.localize_leaks(readings, demand, roughness, sensors),
                 "simulate_links": lambda: net.simulate(demand, roughness, links=True)}
        ms = {m: [] for m in modes}
        for fn in modes.values():                             # (first launches: LDS attribute, allocator)
            fn()
        torch.cuda.synchronize()
        for _ in range(a.repeats):                            # the modes take turns
            for m, fn in modes.items():
                t, out = once(fn)
                ms[m].append(t)
        chunk = H.sensitivity_chunk(N, P, W, 0, K)
        for m, v in ms.items():
            print(json.dumps({"mode": m, "sensors": K, "chunk": chunk, "chunks": -(-K // chunk), "scenarios": a.scenarios,
                              "median_ms": float(np.median(v)), "min_ms": min(v), "max_ms": max(v),
                              "lds_bytes": H.sensitivity_lds_bytes(N, P, W, 0, chunk) if m != "simulate_links" else H.links_lds_bytes(N, P, W, 0)}))
        solve = float(np.median(ms["simulate_links"]))
        print(json.dumps({"mode": "finite_differences_priced", "sensors": K, "solves": N + 1, "ms": (N + 1) * solve}))


if __name__ == "__main__":
    main()
