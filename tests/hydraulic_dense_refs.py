"""The cases that hold the hydraulic network kernels (k_hydraulic_network.hip on hy_newton_valves, k_hydraulics_dev.h) with every
feature on at once and every per-record loop on its second trip, shared by test_hydraulic_dense_host.py and
test_gpu_hydraulic_dense.py: one 300-node layout with pumps, check valves, minor losses, two PRVs, a PSV and an emitter on 280
junctions (N, P and Ke all above HY_T = 256) -- ``dense_steady`` at the three levels of the kernel template (LV 0 the layout
without emitters, LV 1 demand-driven, LV 2 pressure-driven), ``dense_series`` on the same layout with two tanks, three demand
patterns, a pump speed pattern and per-series emitter onsets (warm and cold, demand-driven and pressure-driven), and
``dense_budget``, the largest pressure-driven series the LDS budget admits.  Each case and its host reference (``solve_ref`` /
``simulate_series_ref`` dense and banded, their residuals, their mutual distances, the floors, ``decisive``) is built once and never
changed.  The factors, the floors and ``bound`` are those of hydraulics_refs.py, DECISIVE is what hydraulic_emitters_refs.py says
it is; every bound is formed from the reference's own error, never from a device result.  The comparisons of the GPU test are
stated HERE (``comparisons``, ``series_comparisons``, ``same_statuses``), so that the host test can hold planted wrong answers to the
very same bounds.  The layout, the seeds and the three scalars of the demand model were searched on the CPU until both host
solvers converge in every scenario and step, all of them decisively, with the three valve statuses, a status change in a warm
step and the three regimes of the demand model in every scenario (``steady_reference`` and ``series_reference`` assert it), and
until every case is ROBUST (``moved_answers``; test_hydraulic_dense_host.py asserts it)."""
import contextlib
import functools
import types

import numpy as np

import hydraulic_emitters_refs as ER
import hydraulic_valves_refs as VR
import hydraulics_refs as HR

H, G = HR.H, HR.G
EPS = HR.EPS
HY_T = 256                              # threads of a solve workgroup (test_hydraulic_dense_host.py reads it from k_hydraulics_dev.h)
LEVELS = (0, 1, 2)                      # LV of hydraulic_solve_network_kernel: valves / + emitters / + pressure-driven demand
# make_hydraulic_network(N, P, R, ...): the layout, with every kind of special link.  What the search took: valve_seed 0 with a demand
# ceiling of 3e-4 is the one of the valve seeds 0 .. 11 and the ceilings 3e-4 and 1e-3 that is decisive at LV 0 and LV 1 with all
# three statuses (the others bring a valve's flow within 100 QTOL of a status rule in some scenario); Preq 40 m makes LV 2 decisive too
# (with 30 m the third scenario is not).  The series needed a seed (147 of 17 .. 200), setting factors and scalars of its own.
N_NODES, N_PIPES, N_FIXED, SEED = 300, 330, 3, 6
LAYOUT = dict(num_pumps=2, num_check_valves=6, minor_loss_range=(0.0, 2.0), num_prvs=2, num_psvs=1, valve_seed=0)
KE = 280                                # emitters: background leakage on nearly every junction
SCENARIOS, DEMAND_HI = 3, 3e-4
COEF_RANGE = (1e-6, 1e-5)               # m3/s per m^0.5
COEF_OFF = (3, 100, 255, 256, 257, 279)     # emitters that are off (coefficient exactly 0) in scenario s: these, shifted by s
PUMP_SPEED = ((1.0, 0.9), (1.1, 1.0), (0.95, 1.05))        # [S, Kp]
SETTING_FACTOR = (0.6, 1.4)             # valve k of scenario s: factor[(s + k) % 2] x the pressure of its node without valves
CAP_BASE = (1, 2, 1)                    # the scenarios 1024, 1025, 1026 of cap_case repeat these: other valve statuses than 0, 1, 2
PDD = (0.0, 40.0, 0.5)                  # (Pmin, Preq, exponent) of LV 2
# the series
SERIES, STEPS, STEP_SECONDS, PATTERNS = 2, 6, 600.0, 3
MULT_RANGE, SPEED_MULT_RANGE = (0.7, 1.3), (0.8, 1.1)
SERIES_SEED = 147
SERIES_DEMAND_HI = 1e-3                 # larger draws than the steady case's: the valves' flows stay clear of the status rules' QTOL
SERIES_SETTING_FACTOR = (0.93, 1.07)    # nearer the pressures without valves: the patterns move the valves across their rules
SERIES_PDD = (5.0, 30.0, 1.0)            # the series' own scalars, searched with the seed (see ROBUST)
SERIES_VARIANTS = tuple((warm, pda) for warm in (True, False) for pda in (False, True))
# the budget case
BUDGET_SERIES, BUDGET_STEPS, BUDGET_DEMAND, BUDGET_COEF, BUDGET_PDD = 2, 2, 2e-5, 1e-6, (0.0, 60.0, 0.5)


def _network(num_emitters, num_tanks=0):
    return G.wdn_synth.make_hydraulic_network(N_NODES, N_PIPES, N_FIXED, seed=SEED, num_tanks=num_tanks, num_emitters=num_emitters,
                                              **LAYOUT)


def _coefficients(S, Ke, seed):
    coef = np.random.RandomState(seed + 101).uniform(COEF_RANGE[0], COEF_RANGE[1], (S, Ke))
    for s in range(S):
        coef[s, (np.asarray(COEF_OFF) + s) % Ke] = 0.0
    return coef


def _settings(net, num_tanks, demand, roughness, speed, factor=SETTING_FACTOR):
    """factor x the pressure that a valve's controlled node has in the same scenario of the layout without valves."""
    free = G.wdn_synth.make_hydraulic_network(N_NODES, N_PIPES, N_FIXED, seed=SEED, num_tanks=num_tanks,
                                              **dict(LAYOUT, num_prvs=0, num_psvs=0))
    sol = H.solve_ref(free, demand, roughness, solver="banded", pump_speed=speed)
    assert sol.converged.all()
    pressure = sol.head[:, net.valve_node] - net.elevation[net.valve_node][None, :]
    S = demand.shape[0]
    return np.where((np.arange(S)[:, None] + np.arange(net.num_valves)[None, :]) % 2 == 0, *factor) * pressure


# ---- rows: what one steady launch is given -------------------------------------------------------------------------------------------
def rows(net, demand, roughness, fixed_head=None, speed=None, setting=None, coef=None, pdd=None):
    """One scenario per row: every per-scenario input of ``simulate``, ``solve_ref`` and ``hydraulic_residuals`` alike."""
    return {"net": net, "demand": demand, "roughness": roughness, "fixed_head": fixed_head, "speed": speed, "setting": setting,
            "coef": coef, "pdd": pdd}


def pdd_kw(pdd):
    return {} if pdd is None else dict(demand_model="pda", minimum_pressure=pdd[0], required_pressure=pdd[1], pressure_exponent=pdd[2])


def model_kw(c):
    """The keywords that ``simulate``, ``solve_ref`` and ``hydraulic_residuals`` share."""
    kw = dict(fixed_head=c["fixed_head"], pump_speed=c["speed"], valve_setting=c["setting"], **pdd_kw(c["pdd"]))
    if c["net"].num_emitters:
        kw["emitter_coefficient"] = c["coef"]
    return kw


def solution(src, fields=("head", "flow", "link_state", "iterations", "valve_changes", "emitter_flow", "demand_delivered", "level")):
    """head, flow, link_state, iterations, valve_changes, emitter_flow, demand_delivered (None where the launch has none) of a host
    reference or of a device result brought to numpy (a dict: its iterations are status[..., 0])."""
    if isinstance(src, dict):
        src = types.SimpleNamespace(iterations=src["status"][..., 0], **src)
    return types.SimpleNamespace(**{k: getattr(src, k, None) for k in fields})


def flat(sol):
    """A series solution [S, T, ...] as rows [S T, ...]."""
    f = lambda v: None if v is None else v.reshape((-1,) + v.shape[2:])
    return types.SimpleNamespace(head=f(sol.head), flow=f(sol.flow), link_state=f(sol.link_state), iterations=f(sol.iterations),
                                 valve_changes=f(sol.valve_changes), emitter_flow=f(sol.emitter_flow),
                                 demand_delivered=f(sol.demand_delivered), level=None)


def solve(c, solver="dense", **kw):
    return H.solve_ref(c["net"], c["demand"], c["roughness"], solver=solver, **dict(model_kw(c), **kw))


def residuals(c, sol):
    return H.hydraulic_residuals(c["net"], sol.head, sol.flow, c["demand"], c["roughness"], link_state=sol.link_state,
                                 emitter_flow=sol.emitter_flow, demand_delivered=sol.demand_delivered, **model_kw(c))


def regimes(c, delivered):
    """Per row the numbers of junctions with q_d <= 0, partial and full (hydraulic_pdd_refs.regimes)."""
    j = ~c["net"].fixed[None, :] & (c["demand"] > 0)
    zero, full = (delivered <= 0) & j, (delivered >= c["demand"]) & j
    return zero.sum(axis=1), (j & ~zero & ~full).sum(axis=1), full.sum(axis=1)


def rows_reference(c, dense, banded, c_banded=None):
    """The residuals of two host solutions of the rows ``c`` (the larger of the two), their mutual distances and the floors of
    hydraulic_pdd_refs.reference: a flow takes 64 ulp of the largest head over its link's gradient, capped at the stop rule's
    accuracy x the largest flow; an emitter's flow and a delivered flow take the same with their own gradients."""
    net = c["net"]
    res_d, res_b = residuals(c, dense), residuals(c_banded or c, banded)
    hmax = np.abs(dense.head).max(axis=1)
    span = dense.head.max(axis=1) - dense.head.min(axis=1)
    qmax = np.abs(dense.flow).max(axis=1)[:, None]
    g = np.empty_like(dense.flow)
    for s in range(dense.flow.shape[0]):
        own = np.zeros(net.num_pipes, dtype=bool)
        own[net.valve_links] = dense.link_state[s, net.valve_links] == H.VALVE_CLOSED
        law = H.link_law(net, None if c["speed"] is None else c["speed"][s])
        g[s] = H.link_headloss(dense.flow[s], H._link_resistance(net, c["roughness"][s]), **dict(law, shut=law["shut"] | own))[1]
    floors = {"mass": np.full(hmax.shape, HR.FLOOR_ULPS * EPS), "energy": HR.FLOOR_ULPS * EPS * hmax,
              "dh": HR.FLOOR_ULPS * EPS * hmax / span,
              "flow": np.minimum(HR.FLOOR_ULPS * EPS * hmax[:, None] / g, H.ACCURACY * qmax)}
    out = {"mass": np.maximum(res_d[0], res_b[0]), "energy": np.maximum(res_d[1], res_b[1]),
           "dh": np.abs(banded.head - dense.head).max(axis=1) / span, "dq": np.abs(banded.flow - dense.flow).max(axis=1) / qmax[:, 0],
           "floors": floors, "qmax": qmax, "span": span}
    if net.num_emitters:
        ge = H.emitter_headloss(dense.emitter_flow, c["coef"], net.emitter_exponent)[1]
        floors["emitter_flow"] = np.minimum(HR.FLOOR_ULPS * EPS * hmax[:, None] / ge, H.ACCURACY * qmax)
        out["de"] = np.abs(banded.emitter_flow - dense.emitter_flow) / qmax
    if c["pdd"] is not None:
        pmin, preq, e = c["pdd"]
        on = ~net.fixed[None, :] & (c["demand"] > 0)
        gd = np.where(on, H.demand_headloss(dense.demand_delivered, np.where(on, c["demand"], 1.0), preq - pmin, e)[1], np.inf)
        floors["delivered"] = np.minimum(HR.FLOOR_ULPS * EPS * hmax[:, None] / gd, H.ACCURACY * qmax)
        out["dd"] = np.abs(banded.demand_delivered - dense.demand_delivered) / qmax
    return out


def comparisons(c, ref, dense, got, c_got=None):
    """THE COMPARISONS of a launch with its reference, per row: {name: (value, bound, the reference's own largest value)}.  Mass and energy residuals within
    PHYSICS_FACTOR x the reference's own; heads, flows, emitter flows and delivered flows within AGREEMENT_FACTOR x the
    dense-to-banded distance of the case, with the floors.  ``c_got``: the rows that the result itself was given, where they are
    not the reference's (the steps of a series stand on the result's own levels)."""
    fl, qmax = ref["floors"], ref["qmax"]
    mass, energy = residuals(c_got or c, got)
    out = {"mass": (mass, HR.bound(ref["mass"], fl["mass"], HR.PHYSICS_FACTOR), ref["mass"].max()),
           "energy": (energy, HR.bound(ref["energy"], fl["energy"], HR.PHYSICS_FACTOR), ref["energy"].max()),
           "head": (np.abs(got.head - dense.head).max(axis=1) / ref["span"], HR.bound(ref["dh"].max(), fl["dh"], HR.AGREEMENT_FACTOR),
                    ref["dh"].max()),
           "flow": (np.abs(got.flow - dense.flow) / qmax, HR.bound(ref["dq"].max(), fl["flow"] / qmax, HR.AGREEMENT_FACTOR),
                    ref["dq"].max())}
    if c["net"].num_emitters:
        out["emitter_flow"] = (np.abs(got.emitter_flow - dense.emitter_flow) / qmax,
                               HR.bound(ref["de"].max(), fl["emitter_flow"] / qmax, HR.AGREEMENT_FACTOR), ref["de"].max())
    if c["pdd"] is not None:
        out["delivered"] = (np.abs(got.demand_delivered - dense.demand_delivered) / qmax,
                            HR.bound(ref["dd"].max(), fl["delivered"] / qmax, HR.AGREEMENT_FACTOR), ref["dd"].max())
    return out


def same_statuses(dense, got):
    """Iterations, link_state and valve_changes EQUAL to the reference's (every row of these cases is decisive)."""
    return np.array_equal(got.iterations, dense.iterations) and np.array_equal(got.link_state, dense.link_state) and \
        np.array_equal(got.valve_changes, dense.valve_changes)


def exceeded(cmp):
    """The names of the comparisons that a result misses."""
    return tuple(k for k, (value, bound, _) in cmp.items() if not (value <= bound).all())


def report(cmp):
    """device value / bound / reference value of every comparison: the first two at the entry nearest its bound, the third the
    reference's own largest value of that quantity (its residual, or the dense-to-banded distance)."""
    parts = []
    for k, (value, bound, own) in cmp.items():
        ratio = value / np.broadcast_to(bound, value.shape)
        i = np.unravel_index(np.nanargmax(ratio), ratio.shape)
        parts.append(f"{k} {value[i]:.3e} / {np.broadcast_to(bound, value.shape)[i]:.3e} / {own:.3e}")
    return "  ".join(parts)


# ---- dense_steady -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def steady_case(level):
    """LV 0: the layout without emitters; LV 1: with them, demand-driven; LV 2: pressure-driven."""
    net = _network(KE if level else 0)
    base = G.wdn_synth.make_hydraulic_network(N_NODES, N_PIPES, N_FIXED, seed=SEED)
    demand, roughness = HR._draws(base, SCENARIOS, SEED, DEMAND_HI)
    speed = np.array(PUMP_SPEED, dtype=np.float64)
    return rows(net, demand, roughness, None, speed, _settings(net, 0, demand, roughness, speed),
                _coefficients(SCENARIOS, KE, SEED) if level else None, PDD if level == 2 else None)


def _decisive(dense, banded, solve_dense):
    d = (dense.iterations == banded.iterations) & (dense.valve_changes == banded.valve_changes)
    for ref in (dense, banded):
        d &= (ref.margin[..., 0] >= VR.DECISIVE_H) & (ref.margin[..., 1] >= VR.DECISIVE_Q)
    return d & ER.stop_rule_decisive(solve_dense, dense.iterations)


def _freeze(*refs):
    for ref in refs:
        for v in ref:
            if isinstance(v, np.ndarray):
                v.setflags(write=False)


@functools.lru_cache(maxsize=None)
def steady_reference(level):
    """dense, banded and ``rows_reference`` of them, and ``decisive`` [S]; asserts that both converge in every scenario with the
    same statuses, that every scenario is decisive and, pressure-driven, has the three regimes."""
    c = steady_case(level)
    dense, banded = solve(c, "dense"), solve(c, "banded")
    for ref in (dense, banded):
        assert ref.converged.all() and not ref.failed.any(), (level, ref.iterations, ref.converged)
    assert np.array_equal(dense.link_state, banded.link_state), level
    decisive = _decisive(dense, banded, lambda **kw: solve(c, "dense", **kw))
    assert decisive.all(), (level, decisive, dense.iterations, banded.iterations, dense.margin, banded.margin)
    if level == 2:
        assert all((n > 0).all() for n in regimes(c, dense.demand_delivered)), regimes(c, dense.demand_delivered)
    _freeze(dense, banded)
    return dict(rows_reference(c, solution(dense), solution(banded)), dense=dense, banded=banded, decisive=decisive)


@functools.lru_cache(maxsize=None)
def cap_case():
    """(rows, pairs): ABOVE_CAP scenarios on the dense_steady layout at LV 2, one more trip for the first workgroups of the capped
    grid, and the pairs (s, s + GRID_CAP) that one workgroup solves one after the other.  The bulk repeats the three scenarios
    with the demands scaled by 0.9 .. 1.1; a scenario past the cap repeats the one of CAP_BASE, whose valves end in other
    statuses than those of the scenario its workgroup solved before, with other emitters off and with junctions without demand
    below and above node 256, so that what the workgroup left in LDS -- the fixed rows of the controlled nodes, the valve bits,
    ce of an emitter that was off, D of a junction that was not pressure-driven -- is wrong for it."""
    c = steady_case(2)
    net, S = c["net"], HR.ABOVE_CAP
    idx = np.arange(S) % SCENARIOS
    idx[H.GRID_CAP:] = CAP_BASE
    demand = c["demand"][idx] * np.linspace(0.9, 1.1, S)[:, None]
    roughness, speed, setting, coef = c["roughness"][idx].copy(), c["speed"][idx].copy(), c["setting"][idx].copy(), c["coef"][idx].copy()
    junctions = np.flatnonzero(~net.fixed)
    low, high = junctions[junctions < HY_T], junctions[junctions >= HY_T]
    pairs = tuple((s, s + H.GRID_CAP) for s in range(S - H.GRID_CAP))
    for s, t in pairs:
        coef[t, [10 + s, 200 + s, HY_T + 4 + s, KE - 5 - s]] = 0.0
        demand[t, [low[5 + s], high[3 + s]]] = 0.0
    return rows(net, demand, roughness, None, speed, setting, coef, c["pdd"]), pairs


# ---- dense_series -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def series_case(pda):
    """The layout with two tanks and all its emitters: S series of T steps, three demand patterns assigned per node, one pump
    speed pattern, an onset per series and emitter."""
    net = _network(KE, num_tanks=2)
    base = G.wdn_synth.make_hydraulic_network(N_NODES, N_PIPES, N_FIXED, seed=SEED)
    demand, roughness = HR._draws(base, SERIES, SEED, SERIES_DEMAND_HI)
    rng = np.random.RandomState(SERIES_SEED)
    mult = rng.uniform(MULT_RANGE[0], MULT_RANGE[1], (PATTERNS, STEPS))
    pattern = rng.randint(0, PATTERNS, N_NODES)
    smult = rng.uniform(SPEED_MULT_RANGE[0], SPEED_MULT_RANGE[1], (1, STEPS))
    onset = rng.randint(0, STEPS, (SERIES, KE))
    speed = np.array(PUMP_SPEED[:SERIES], dtype=np.float64)
    return {"net": net, "demand": demand, "roughness": roughness, "mult": mult, "pattern": pattern, "dt": STEP_SECONDS, "speed": speed,
            "smult": smult, "spat": np.zeros(net.num_pumps, dtype=np.int64), "setting": _settings(net, 2, demand, roughness, speed, SERIES_SETTING_FACTOR),
            "coef": _coefficients(SERIES, KE, SEED + 1), "onset": onset, "pdd": SERIES_PDD if pda else None}


def series_kw(c):
    """The keywords that ``simulate_series`` and ``simulate_series_ref`` share."""
    kw = dict(pattern_of_node=c["pattern"], pump_speed=c["speed"], speed_multipliers=c["smult"], speed_pattern_of_pump=c["spat"],
              valve_setting=c["setting"], emitter_coefficient=c["coef"], emitter_onset=c["onset"], **pdd_kw(c["pdd"]))
    if c.get("level0") is not None:
        kw["initial_level"] = c["level0"]
    return kw


def simulate_ref(c, solver="dense", warm=True, **kw):
    return H.simulate_series_ref(c["net"], c["demand"], c["roughness"], c["mult"], c["dt"], solver=solver, warm_start=warm,
                                 **dict(series_kw(c), **kw))


def step_rows(c, level):
    """The S T steps of a series as rows of a steady launch, in the order [s, t]: the rounded product demand x multiplier of the
    node's pattern, the tank heads elevation + level [S, T + 1, K] of the step, the pump speeds speed x the speed pattern, and
    the coefficients of the emitters whose onset has come."""
    net, S, T = c["net"], c["demand"].shape[0], c["mult"].shape[1]
    demand = np.where(net.fixed[None, None, :], 0.0, c["demand"][:, None, :] * c["mult"][c["pattern"], :].T[None, :, :])
    heads = np.tile(net.fixed_head, (S, T, 1))
    heads[:, :, net.tank_nodes] = net.elevation[net.tank_nodes][None, None, :] + level[:, :T]
    speed = None if c["speed"] is None else c["speed"][:, None, :] * c["smult"][c["spat"], :].T[None, :, :]
    live = np.where(np.arange(T)[None, :, None] < c["onset"][:, None, :], 0.0, c["coef"][:, None, :])
    rep = lambda v: np.repeat(v[:, None], T, axis=1)
    f = lambda v: None if v is None else np.ascontiguousarray(v.reshape((S * T,) + v.shape[2:]))
    return rows(net, f(demand), f(rep(c["roughness"])), f(heads), f(speed), None if c["setting"] is None else f(rep(c["setting"])),
                f(live), c["pdd"])


def levels_and_balance(c, dense, banded, got):
    """The level and volume-balance comparisons of test_a_warm_series_against_the_reference_and_its_volume_balance, per tank: a flow
    is determined to ACCURACY x the largest flow, which moves a level by dt / A in every step; the balance within
    PHYSICS_FACTOR x the reference's own, floored by dt x that flow accuracy."""
    net, T, dt = c["net"], c["mult"].shape[1], c["dt"]
    qmax = np.abs(dense.flow).max()
    l_floor = T * dt / net.tank_area * H.ACCURACY * qmax
    l_own = np.abs(dense.level - banded.level).max()
    l_bound = HR.bound(l_own, l_floor, HR.AGREEMENT_FACTOR)
    balance = lambda r: np.abs(H.series_volume_balance(net, r, c["demand"], c["mult"], dt, pattern_of_node=c["pattern"]))
    b_own = balance(dense).max()
    b_bound = HR.bound(b_own, dt * H.ACCURACY * qmax, HR.PHYSICS_FACTOR)
    return {"level": (np.abs(got.level - dense.level).max(axis=(0, 1)), l_bound, l_own),
            "volume": (balance(got).max(axis=1), np.full(c["demand"].shape[0], b_bound), b_own)}


@functools.lru_cache(maxsize=None)
def series_reference(warm, pda):
    """dense, banded, ``rows_reference`` of their steps and ``decisive`` [S, T]; asserts convergence in every step, equal
    statuses, that every step is decisive and, pressure-driven, has the three regimes."""
    c = series_case(pda)
    dense, banded = simulate_ref(c, "dense", warm), simulate_ref(c, "banded", warm)
    for ref in (dense, banded):
        assert ref.converged.all() and not ref.failed.any(), (warm, pda, ref.iterations, ref.converged)
    assert np.array_equal(dense.link_state, banded.link_state), (warm, pda)
    decisive = _decisive(dense, banded, lambda **kw: simulate_ref(c, "dense", warm, **kw))
    assert decisive.all(), (warm, pda, decisive, dense.iterations, banded.iterations)
    steps = step_rows(c, dense.level)
    if pda:
        assert all((n > 0).all() for n in regimes(steps, flat(solution(dense)).demand_delivered)), (warm, pda)
    _freeze(dense, banded)
    return dict(rows_reference(steps, flat(solution(dense)), flat(solution(banded)), step_rows(c, banded.level)), dense=dense,
                banded=banded, decisive=decisive, steps=steps)


def series_comparisons(c, ref, got):
    """``comparisons`` of every step, and ``levels_and_balance``."""
    out = comparisons(ref["steps"], ref, flat(solution(ref["dense"])), flat(got), step_rows(c, got.level))
    out.update(levels_and_balance(c, ref["dense"], ref["banded"], got))
    return out


# ---- dense_budget -------------------------------------------------------------------------------------------------------------------
def budget_nodes():
    """The largest N for which a path reservoir -- N - 2 junctions with an emitter each -- tank, given the full band, fits a
    pressure-driven series launch."""
    need = lambda n: H.series_pdd_lds_bytes(n, n - 1, n - 1, 1, 0, 0, n - 2)
    n = 3
    while need(n + 1) <= H.LDS_BUDGET:
        n += 1
    return n


def budget_network(N):
    """reservoir 0 (80 m) -- junctions 1 .. N - 2, every one with an emitter -- tank N - 1 (bottom at 60 m, 3 m of water), in the
    given order with the full band, as hydraulics_refs._small builds path139_full_s3."""
    rng = np.random.RandomState(18)
    P = N - 1
    elevation = rng.uniform(0.0, 20.0, N)
    elevation[N - 1] = 60.0
    net = H.HydraulicNetwork(HR._edge_index([(i, i + 1) for i in range(P)]), rng.uniform(50.0, 500.0, P), rng.uniform(0.1, 0.3, P),
                             elevation, [0, N - 1], [80.0, 63.0], tank_nodes=[N - 1], tank_diameter=[8.0],
                             emitter_nodes=np.arange(1, N - 1))
    net.order = np.arange(N, dtype=np.int32)
    net.position = net.order.copy()
    net.half_bandwidth = N - 1
    return net


def _budget_case(N):
    net = budget_network(N)
    rng = np.random.RandomState(19)
    demand = np.where(net.fixed[None, :], 0.0, rng.uniform(0.1 * BUDGET_DEMAND, BUDGET_DEMAND, (BUDGET_SERIES, N)))
    coef = np.full((BUDGET_SERIES, N - 2), BUDGET_COEF)
    coef[:, ::7] = 0.0
    return {"net": net, "demand": demand, "roughness": rng.uniform(80.0, 130.0, (BUDGET_SERIES, N - 1)),
            "mult": np.array([[1.0, 1.2][:BUDGET_STEPS]]), "pattern": np.zeros(N, dtype=np.int64), "dt": STEP_SECONDS, "speed": None,
            "smult": None, "spat": None, "setting": None, "coef": coef, "onset": np.zeros((BUDGET_SERIES, N - 2), dtype=np.int64),
            "pdd": BUDGET_PDD}


@functools.lru_cache(maxsize=None)
def budget_case(extra=0):
    return _budget_case(budget_nodes() + extra)


@functools.lru_cache(maxsize=None)
def budget_reference():
    c = budget_case()
    dense, banded = simulate_ref(c, "dense"), simulate_ref(c, "banded")
    for ref in (dense, banded):
        assert ref.converged.all() and not ref.failed.any(), (ref.iterations, ref.converged)
    decisive = _decisive(dense, banded, lambda **kw: simulate_ref(c, "dense", **kw))
    steps = step_rows(c, dense.level)
    _freeze(dense, banded)
    return dict(rows_reference(steps, flat(solution(dense)), flat(solution(banded)), step_rows(c, banded.level)), dense=dense,
                banded=banded, decisive=decisive, steps=steps)


# ---- ROBUST: right answers with other roundings must pass -----------------------------------------------------------------------------
def moved_answers(kind, *key):
    """ROBUST, a condition on the inputs like DECISIVE: the host solutions of the case with every roughness moved by ONE ULP, up
    and down, dense and banded, as (name, the comparisons with the case's reference, same statuses).  They are right answers
    that differ from the reference by rounding alone, as a device result does; a case on which one of them takes other
    iterations or misses a bound checks the luck of the roundings and not the kernel.  (The pressure-driven series with exponent
    0.5 that the search met on this layout were such cases: a junction 18 cm above Pmin delivers D sqrt(p / dp), whose slope in
    p has no bound, and the heads of a cold step differ between right solvers by what the stop rule leaves open; moved by one
    ulp, ``simulate_series_ref`` itself then took other iterations.  SERIES_PDD has the exponent 1.)"""
    out = []
    for way in (np.inf, 0.0):
        for solver in ("banded", "dense"):
            name = f"{'up' if way else 'down'}-{solver}"
            if kind == "steady":
                c, ref = steady_case(*key), steady_reference(*key)
                sol = solution(solve(dict(c, roughness=np.nextafter(c["roughness"], way)), solver))
                out.append((name, comparisons(c, ref, solution(ref["dense"]), sol), same_statuses(ref["dense"], sol)))
            else:
                warm, pda = key
                c, ref = series_case(pda), series_reference(warm, pda)
                sol = solution(simulate_ref(dict(c, roughness=np.nextafter(c["roughness"], way)), solver, warm))
                out.append((name, series_comparisons(c, ref, sol), same_statuses(flat(solution(ref["dense"])), flat(sol))))
    return out


# ---- planted wrong answers: the comparisons above must catch each ---------------------------------------------------------------------
@contextlib.contextmanager
def _patched(name, wrong):
    right = getattr(H, name)
    setattr(H, name, wrong(right))
    try:
        yield
    finally:
        setattr(H, name, right)


def wrong_answer(kind):
    """(the comparisons of, the reference's solution, the wrong solution): each wrong solution is the converged host solution of
    a WRONG model -- the mistakes a kernel makes whose loops stop at HY_T records, or whose series forgets what it carries."""
    if kind == "emitters_past_the_first_trip_left_out":         # `k < Ke` taken for `tid < Ke`: the emitters 256.. never leak
        c, ref = steady_case(1), steady_reference(1)
        coef = c["coef"].copy()
        coef[:, HY_T:] = 0.0
        sol = solve(dict(c, coef=coef), "banded")
        assert sol.converged.all()
        return comparisons(c, ref, solution(ref["dense"]), solution(sol)), solution(ref["dense"]), solution(sol)
    if kind == "junctions_past_the_first_trip_demand_driven":   # the junctions 256.. never become pressure-driven
        c, ref = steady_case(2), steady_reference(2)

        def wrong(record):
            def first_trip_only(network, d, pdd, q=None, keep=None):
                rec = record(network, d, pdd, q, keep)
                if rec is not None:
                    rec["on"][HY_T:] = False
                    rec["D"][HY_T:], rec["q"][HY_T:] = 0.0, 0.0
                return rec
            return first_trip_only
        with _patched("demand_record", wrong):
            sol = solve(c, "banded")
        assert sol.converged.all()
        return comparisons(c, ref, solution(ref["dense"]), solution(sol)), solution(ref["dense"]), solution(sol)
    c = series_case(False)
    ref = series_reference(True, False)
    if kind == "valve_statuses_reset_at_every_step":            # a warm series that starts every valve ACTIVE at every step
        def wrong(record):
            return lambda network, valve_setting=None, shut=None, status=None: record(network, valve_setting, shut, None)
        with _patched("valve_record", wrong):
            sol = simulate_ref(c, "banded", True)
    elif kind == "every_onset_taken_as_zero":                   # every emitter of the last series leaks from step 0 on (with those
        onset = c["onset"].copy()                               # of the first as well, the wrong model has no solution)
        onset[-1] = 0
        sol = simulate_ref(dict(c, onset=onset), "banded", True)
    else:
        raise KeyError(kind)
    assert sol.converged.all()
    return series_comparisons(c, ref, solution(sol)), flat(solution(ref["dense"])), flat(solution(sol))


WRONG = ("emitters_past_the_first_trip_left_out", "junctions_past_the_first_trip_demand_driven",
         "valve_statuses_reset_at_every_step", "every_onset_taken_as_zero")
WRONG_STATUS = ("valve_statuses_reset_at_every_step",)

CACHED = (steady_case, steady_reference, cap_case, series_case, series_reference, budget_case, budget_reference)
