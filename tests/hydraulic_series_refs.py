"""The cases of the hydraulic series' tests, shared by test_hydraulic_series_host.py and test_gpu_hydraulic_series.py: each case is a
network with tanks, its series (base demands, roughness, multipliers, patterns, initial levels) and its host reference
(``simulate_series_ref`` dense and banded, warm and cold), built once and never changed.  ``check_series`` is THE CHECKER: the
device's outputs and the planted wrong answers of the host tests go through the same function.  Its bounds are formed here from the
reference's own error and the precision of fp64 -- never from a device result -- with the factors and floors of hydraulics_refs.py."""
import functools

import numpy as np

import hydraulics_refs as HR

G, H = HR.G, HR.H
EPS, FLOOR_ULPS = HR.EPS, HR.FLOOR_ULPS
PHYSICS_FACTOR, AGREEMENT_FACTOR = HR.PHYSICS_FACTOR, HR.AGREEMENT_FACTOR
DT = 300.0


def _case(net, S, T, seed, demand_hi, M=1, per_series_mult=False, per_series_heads=False, level0=None, dt=DT, demand_lo=None):
    d_lo, d_hi, c_lo, c_hi = net.draw_ranges((0.1 * demand_hi if demand_lo is None else demand_lo, demand_hi), H.ROUGHNESS_RANGE)
    demand, roughness = H.hydraulic_draws(seed, 0, S, d_lo, d_hi, c_lo, c_hi)
    mult = G.wdn_synth.make_demand_patterns(M, T, dt, seed)
    if per_series_mult:                  # [S, M, T]: every series its own day
        mult = np.stack([G.wdn_synth.make_demand_patterns(M, T, dt, seed + 1 + s) for s in range(S)])
    pattern = (np.arange(net.num_nodes) % M).astype(np.int32)
    heads = None
    if per_series_heads:                 # [S, N]: the reservoirs move per series (a tank's entry is replaced by its level)
        heads = np.tile(net.fixed_head, (S, 1))
        heads[:, net.fixed] += np.random.RandomState(seed).uniform(-2.0, 2.0, (S, int(net.fixed.sum())))
    if level0 is None:
        level0 = np.tile(net.fixed_head[net.tank_nodes] - net.elevation[net.tank_nodes], (S, 1))
    level0 = np.ascontiguousarray(np.broadcast_to(np.asarray(level0, dtype=np.float64), (S, net.num_tanks)))
    return {"net": net, "demand": demand, "roughness": roughness, "mult": mult, "pattern": pattern, "heads": heads,
            "level0": level0, "dt": dt, "T": T, "S": S, "M": M}


def _small(pairs, N, fixed, head, tanks, tank_diameter, S, T, seed, demand_hi=2e-3, tank_min=None, tank_max=None, level0=None,
           elevation=None, **kw):
    P = len(pairs)
    rng = np.random.RandomState(seed)
    length, diameter = rng.uniform(50.0, 500.0, P), rng.uniform(0.1, 0.3, P)
    elev = rng.uniform(0.0, 20.0, N) if elevation is None else np.asarray(elevation, dtype=np.float64)
    net = H.HydraulicNetwork(HR._edge_index(pairs), length, diameter, elev, fixed, head, tank_nodes=tanks,
                             tank_diameter=tank_diameter, tank_min_level=tank_min, tank_max_level=tank_max)
    return _case(net, S, T, seed, demand_hi, level0=level0, **kw)


def _synthetic(N, P, R, K, S, T, seed, demand_hi, **kw):
    net = G.wdn_synth.make_hydraulic_network(N, P, R, seed=seed, num_tanks=K)
    return _case(net, S, T, seed, demand_hi, **kw)


def _zero_junction(case):                # (b): the junction between the reservoir and the tank draws nothing
    case["demand"] = np.zeros_like(case["demand"])
    return case


BUILDERS = {
    # (a) one tank (node 0), one pipe, one junction: no reservoir
    "two_t1": lambda: _small([(0, 1)], 2, [0], [30.0], [0], [6.0], 3, 1, 21, elevation=[25.0, 3.0]),
    "two_t2": lambda: _small([(0, 1)], 2, [0], [30.0], [0], [6.0], 3, 2, 22, elevation=[25.0, 3.0]),
    "two_t12": lambda: _small([(0, 1)], 2, [0], [30.0], [0], [6.0], 3, 12, 23, elevation=[25.0, 3.0]),
    # the same tank, small and nearly empty: it drains to its minimum and is clamped from then on
    "two_drain_t12": lambda: _small([(0, 1)], 2, [0], [30.0], [0], [2.0], 3, 12, 24, elevation=[25.0, 3.0], tank_min=[4.5],
                                    tank_max=[9.0]),
    # (b) reservoir 0 -- pipe -- tank 1, directly
    "fill_direct_t12": lambda: _zero_junction(_small([(0, 1)], 2, [0, 1], [40.0, 22.0], [1], [5.0], 2, 12, 25,
                                                     elevation=[0.0, 20.0])),
    # (b) reservoir 0 -- junction 1 (no demand) -- tank 2, and the same with a maximum that is reached
    "fill_t12": lambda: _zero_junction(_small([(0, 1), (1, 2)], 3, [0, 2], [40.0, 22.0], [2], [5.0], 2, 12, 26,
                                              elevation=[0.0, 5.0, 20.0])),
    "fill_clamp_t12": lambda: _zero_junction(_small([(0, 1), (1, 2)], 3, [0, 2], [40.0, 22.0], [2], [12.0], 2, 12, 27,
                                                    elevation=[0.0, 5.0, 20.0], tank_max=[2.5])),
    # (c) two tanks and no reservoir
    "two_tanks_t12": lambda: _small([(0, 1), (1, 2)], 3, [0, 2], [32.0, 30.0], [0, 2], [8.0, 5.0], 3, 12, 28,
                                    elevation=[27.0, 2.0, 26.0]),
    "net37_t1": lambda: _synthetic(37, 41, 2, 1, 3, 1, 31, 1e-3),
    "net37_t12": lambda: _synthetic(37, 41, 2, 1, 3, 12, 32, 1e-3, M=3),
    "net40_t24": lambda: _synthetic(40, 44, 3, 1, 3, 24, 33, 1e-3, M=3, per_series_mult=True, per_series_heads=True),
    "net40_k0_t12": lambda: _synthetic(40, 44, 2, 0, 3, 12, 34, 1e-3, M=3),
    "net388_t4": lambda: _synthetic(388, 430, 5, 2, 3, 4, 35, 1e-4, M=3),
}
NAMES = tuple(BUILDERS)
CLAMPED = ("two_drain_t12", "fill_clamp_t12")


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()


def run_ref(c, **kw):
    return H.simulate_series_ref(c["net"], c["demand"], c["roughness"], c["mult"], c["dt"], initial_level=c["level0"],
                                 pattern_of_node=c["pattern"], fixed_head=c["heads"], **kw)


def step_inputs(c, level):
    """The steady scenario that step (s, t) solves, flattened to [S * T, .]: demand * multiplier (one product), roughness, and the
    fixed heads with elevation + level at the tanks."""
    net, S, T = c["net"], c["S"], c["T"]
    mult = c["mult"] if c["mult"].ndim == 3 else np.broadcast_to(c["mult"], (S,) + c["mult"].shape)
    demand = c["demand"][:, None, :] * np.swapaxes(mult, 1, 2)[:, :, c["pattern"]]                    # [S, T, N]
    heads = np.broadcast_to(net.fixed_head if c["heads"] is None else c["heads"], (S, net.num_nodes))
    heads = np.repeat(heads[:, None, :], T, axis=1).copy()
    heads[:, :, net.tank_nodes] = net.elevation[net.tank_nodes][None, None, :] + np.asarray(level)[:, :T, :]
    rough = np.repeat(c["roughness"][:, None, :], T, axis=1)
    return demand.reshape(S * T, -1), rough.reshape(S * T, -1), heads.reshape(S * T, -1)


def residuals(c, head, flow, level):
    """(mass, energy) [S, T] of a series' steps, each against the steady model it solves."""
    net, S, T = c["net"], c["S"], c["T"]
    d, r, h = step_inputs(c, level)
    with np.errstate(all="ignore"):
        mass, energy = H.hydraulic_residuals(net, head.reshape(S * T, -1), flow.reshape(S * T, -1), d, r, h)
    return mass.reshape(S, T), energy.reshape(S, T)


class Out:
    """What the checker looks at: numpy arrays named as the fields of a series result."""

    def __init__(self, head, flow, level, status, final_dq, pressure=None):
        self.head, self.flow, self.level, self.status, self.final_dq, self.pressure = head, flow, level, status, final_dq, pressure


def out_of_ref(c, r):
    status = np.stack([r.iterations, r.converged.astype(np.int32), r.failed.astype(np.int32), r.limited.astype(np.int32)],
                      axis=2).astype(np.int32)
    return Out(r.head, r.flow, r.level, status, r.final_dq, (r.head - c["net"].elevation[None, None, :]).astype(np.float32))


def _own_error(c, runs):
    """The reference's own error per step [S, T]: the larger of the given runs' (mass, energy, |volume balance|)."""
    res = [residuals(c, r.head, r.flow, r.level) for r in runs]
    bal = [np.abs(H.series_volume_balance(c["net"], r, c["demand"], c["mult"], c["dt"], c["pattern"])) for r in runs]
    return {"mass": np.maximum.reduce([r[0] for r in res]), "energy": np.maximum.reduce([r[1] for r in res]),
            "balance": np.maximum.reduce(bal), "limited": np.logical_or.reduce([r.limited for r in runs])}


@functools.lru_cache(maxsize=None)
def reference(name):
    """The warm series (dense, banded) and the cold ones, each pair's own error PER STEP ("warm", "cold"), the dense-to-banded
    distances of the warm pair and the floors.

    THE FLOORS are those of hydraulics_refs.py (64 ulp of the scale) and two that a series adds, both derived from fp64 and the
    step's conditioning at the reference's flows, none from a device result:
      mass     a solved head carries at least one rounding, EPS * max |H|, and reaches the balance of junction j through the
               gradients of its pipes: EPS * max |H| * sum_{p at j} 1 / g_p, over sum |q|, at the worst junction.  This is the
               scale of the reference's own residuals (their median over the steps is 0.5 .. 1 of it on the 37-, 40- and
               388-node cases and 0.2 .. 0.3 of it on the two-node ones); a step's residual is one draw of that noise and
               may come out a hundred times below it, which is what the floor is for.
      balance  64 ulp of the stored volume and of dt * sum |q| (it is their difference), plus dt * sum |q| times the mass floor:
               the balance is dt times the sum of the junctions' imbalances.
      level    a level inherits, step after step, dt / A_k times what the flows of the tank's pipes are uncertain by."""
    c = case(name)
    net, S, T, dt = c["net"], c["S"], c["T"], c["dt"]
    dense, banded = run_ref(c, solver="dense"), run_ref(c, solver="banded")
    cold, cold_banded = run_ref(c, solver="dense", warm_start=False), run_ref(c, solver="banded", warm_start=False)
    span = dense.head.max(axis=2) - dense.head.min(axis=2)                                            # [S, T]
    hmax = np.abs(dense.head).max(axis=2)
    qmax = np.abs(dense.flow).max(axis=2)
    qsum = np.abs(dense.flow).sum(axis=2)
    d, rough, _ = step_inputs(c, dense.level)
    _, g = H.pipe_headloss(dense.flow.reshape(S * T, -1), net.coef[None, :] / np.power(rough, 1.852))
    g = g.reshape(S, T, -1)
    flow_floor = np.minimum(FLOOR_ULPS * EPS * hmax[:, :, None] / g, H.ACCURACY * qmax[:, :, None])                      # [S, T, P]
    at_node = np.zeros((S, T, net.num_nodes))                                                         # sum of 1 / g_p over a node's pipes
    for p, (a, b) in enumerate(net.pipes):
        at_node[:, :, a] += 1.0 / g[:, :, p]
        at_node[:, :, b] += 1.0 / g[:, :, p]
    mass_floor = np.maximum(FLOOR_ULPS * EPS, EPS * hmax * at_node[:, :, ~net.fixed].max(axis=2, initial=0.0) / qsum)
    at_tank = np.stack([(net.pipes[:, 0] == n) | (net.pipes[:, 1] == n) for n in net.tank_nodes]) if net.num_tanks else np.zeros((0, net.num_pipes), bool)
    per_step = np.stack([flow_floor[:, :, at_tank[k]].sum(axis=2) * dt / net.tank_area[k] for k in range(net.num_tanks)], axis=2) \
        if net.num_tanks else np.zeros((S, T, 0))
    level_floor = np.concatenate([np.zeros((S, 1, net.num_tanks)), np.cumsum(per_step, axis=1)], axis=1)                 # [S, T + 1, K]
    stored = (np.abs(dense.level) * net.tank_area[None, None, :]).sum(axis=2).max(axis=1) if net.num_tanks else np.zeros(S)
    balance_floor = FLOOR_ULPS * EPS * (stored[:, None] + dt * qsum) + dt * qsum * mass_floor
    with np.errstate(all="ignore"):
        dh = np.nanmax(np.abs(banded.head - dense.head).max(axis=2) / span)
        dq = np.nanmax(np.abs(banded.flow - dense.flow).max(axis=2) / qmax)
        dl = np.nanmax(np.abs(banded.level - dense.level)) if net.num_tanks else 0.0
    out = {"dense": dense, "banded": banded, "cold": cold, "cold_banded": cold_banded, "warm_error": _own_error(c, (dense, banded)),
           "cold_error": _own_error(c, (cold, cold_banded)), "dh": dh, "dq": dq, "dl": dl,
           "floors": {"mass": mass_floor, "energy": FLOOR_ULPS * EPS * hmax, "dh": FLOOR_ULPS * EPS * hmax / span,
                      "flow": flow_floor, "level": level_floor, "balance": balance_floor}}
    for r in (dense, banded, cold, cold_banded):
        for v in (r.head, r.flow, r.level):
            v.setflags(write=False)
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_series(name, out, agreement=True, start="warm", log=None):
    """THE CHECKER.  Returns the names of the checks that ``out`` (an ``Out``) misses on the case, [] for a right answer; ``log``
    (a list) receives one line of figures per check.  What is bit for bit: level[0] is the input; every later level and the
    clamp flag are ``level_update_ref`` of the SAME step's flows and levels; a tank's head is elevation + level and a
    reservoir's the fixed head; the pressure is fp32(head - elevation).  What is bounded by the reference's own error, step by
    step: the mass and energy residuals of step (s, t) and, where no level was clamped, its volume balance, each <=
    PHYSICS_FACTOR x max(the same quantity of the reference ON THAT STEP, the floor), the reference being the larger of its
    dense and banded runs of the same ``start`` ("warm" or "cold": a warm result is never held to a cold run or the other way
    round).  And with ``agreement``: heads, flows and levels against the dense warm reference (AGREEMENT_FACTOR x the
    dense-to-banded distance of the case, as test_gpu_hydraulics.py takes it) and the iteration counts."""
    c, ref = case(name), reference(name)
    net, S, T, dt = c["net"], c["S"], c["T"], c["dt"]
    note = (lambda s: log.append(f"[{name}] {s}")) if log is not None else (lambda s: None)
    missed = []

    def hold(what, ok, figures=""):
        note(f"{what}: {'ok' if ok else 'MISSED'} {figures}")
        if not ok:
            missed.append(what)

    alive = out.status[:, :, 2] == 0
    hold("level0", same_bits(out.level[:, 0], c["level0"]))
    nxt, clamped = H.level_update_ref(net, out.level[:, :-1], out.flow, dt)
    hold("level_update", all(same_bits(out.level[:, t + 1][alive[:, t]], nxt[:, t][alive[:, t]]) for t in range(T)))
    hold("limited_flag", np.array_equal(out.status[:, :, 3][alive] != 0, clamped.any(axis=2)[alive]))
    fixed_heads = step_inputs(c, out.level)[2].reshape(S, T, -1)
    hold("fixed_heads", same_bits(out.head[:, :, net.fixed][alive], fixed_heads[:, :, net.fixed][alive]))
    if out.pressure is not None:
        hold("pressure", same_bits(out.pressure, (out.head - net.elevation[None, None, :]).astype(np.float32)))
    mass, energy = residuals(c, out.head, out.flow, out.level)
    own = ref[start + "_error"]
    b_mass = HR.bound(own["mass"], ref["floors"]["mass"], PHYSICS_FACTOR)
    b_energy = HR.bound(own["energy"], ref["floors"]["energy"], PHYSICS_FACTOR)
    with np.errstate(all="ignore"):
        hold("mass", bool((mass <= b_mass)[alive].all()), f"worst dev/bound {np.nanmax(mass / b_mass):.3e}")
        hold("energy", bool((energy <= b_energy)[alive].all()), f"worst dev/bound {np.nanmax(energy / b_energy):.3e}")
    free = alive & ~clamped.any(axis=2) & ~own["limited"]               # (by the statement on out's own flows, not by out's flag)
    balance = np.abs(H.series_volume_balance(net, out, c["demand"], c["mult"], dt, c["pattern"]))
    b_bal = HR.bound(own["balance"], ref["floors"]["balance"], PHYSICS_FACTOR)
    with np.errstate(all="ignore"):
        hold("volume_balance", bool((balance <= b_bal)[free].all()),
             f"worst dev/bound {np.max((balance / b_bal)[free], initial=0.0):.3e} (m3: {np.max(balance[free], initial=0.0):.3e})")
    if agreement:
        dense = ref["dense"]
        span = dense.head.max(axis=2) - dense.head.min(axis=2)
        qmax = np.abs(dense.flow).max(axis=2)
        dh = np.abs(out.head - dense.head).max(axis=2) / span
        b_h = HR.bound(ref["dh"], ref["floors"]["dh"], AGREEMENT_FACTOR)
        dq = np.abs(out.flow - dense.flow) / qmax[:, :, None]
        b_q = HR.bound(ref["dq"], ref["floors"]["flow"] / qmax[:, :, None], AGREEMENT_FACTOR)
        dl = np.abs(out.level - dense.level)
        b_l = HR.bound(ref["dl"], ref["floors"]["level"], AGREEMENT_FACTOR)
        with np.errstate(all="ignore"):
            hold("head_agreement", bool((dh <= b_h).all()), f"worst dev/bound {np.nanmax(dh / b_h):.3e}")
            hold("flow_agreement", bool((dq <= b_q).all()), f"worst dev/bound {np.nanmax(dq / b_q):.3e}")
            hold("level_agreement", bool((dl <= b_l).all()),
                 f"worst dev/bound {np.max(dl / np.where(b_l > 0, b_l, 1.0), initial=0.0):.3e}" if dl.size else "")
        hold("iterations", np.array_equal(out.status[:, :, 0], dense.iterations),
             f"dev {out.status[:, :, 0].sum()} ref {dense.iterations.sum()}")
        hold("status", np.array_equal(out.status[:, :, 1] != 0, dense.converged) and np.array_equal(out.status[:, :, 2] != 0, dense.failed))
    return missed


# ---- planted wrong answers: the series loop written out with one mistake -------------------------------------------------------------
BUGS = ("next_flows", "flipped_inflow", "dt_twice", "no_elevation", "pattern_shift")


def buggy_series(name, bug):
    """A cold-start series by ``solve_ref``, step by step, with one planted mistake; returns an ``Out``."""
    c = case(name)
    net, S, T, dt, tanks = c["net"], c["S"], c["T"], c["dt"], c["net"].tank_nodes
    mult = c["mult"] if c["mult"].ndim == 3 else np.broadcast_to(c["mult"], (S,) + c["mult"].shape)
    pattern = (c["pattern"] + 1) % c["M"] if bug == "pattern_shift" else c["pattern"]
    heads = np.broadcast_to(net.fixed_head if c["heads"] is None else c["heads"], (S, net.num_nodes)).copy()
    level = np.empty((S, T + 1, net.num_tanks))
    level[:, 0] = c["level0"]
    head, flow = np.empty((S, T, net.num_nodes)), np.empty((S, T, net.num_pipes))
    status, final_dq = np.zeros((S, T, 4), dtype=np.int32), np.empty((S, T))
    for t in range(T):
        heads[:, tanks] = (0.0 if bug == "no_elevation" else net.elevation[tanks][None, :]) + level[:, t]
        r = H.solve_ref(net, c["demand"] * mult[:, pattern, t], c["roughness"], heads)
        head[:, t], flow[:, t], final_dq[:, t] = r.head, r.flow, r.final_dq
        status[:, t, 0], status[:, t, 1] = r.iterations, r.converged
        q = -r.flow if bug == "flipped_inflow" else r.flow
        nxt, clamped = H.level_update_ref(net, level[:, t], q, dt * dt if bug == "dt_twice" else dt)
        level[:, t + 1], status[:, t, 3] = nxt, clamped.any(axis=1)
    if bug == "next_flows":              # every level moved by the flows of the step AFTER it (the last by its own)
        for t in range(T):
            level[:, t + 1] = H.level_update_ref(net, level[:, t], flow[:, min(t + 1, T - 1)], dt)[0]
    return Out(head, flow, level, status, final_dq, (head - net.elevation[None, None, :]).astype(np.float32))
