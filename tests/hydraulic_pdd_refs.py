"""The cases of the pressure-driven demand tests, shared by test_hydraulic_pdd_host.py and test_gpu_hydraulic_pdd.py: each case is a
network, its scenarios, the three scalars of the demand model and its host reference (``solve_ref`` dense and banded with the
demand's node term), built once and never changed.  The factors, the floors and ``bound`` are those of hydraulics_refs.py; every
bound is formed from the reference's own error, never from a device result.  DECISIVE is what hydraulic_emitters_refs.py says it
is: the status-rule margins of hydraulic_valves_refs.py, equal iterations in both host solvers, and a stop rule that keeps its
iteration count with the accuracy moved by ``STOP_MARGIN`` either way.  The synthetic cases were chosen on the CPU so that both
host solvers converge in every scenario, every scenario has a junction in each regime (q_d <= 0, partial, full) and every
scenario is decisive; ``reference`` asserts all three."""
import functools

import numpy as np

import hydraulic_emitters_refs as ER
import hydraulic_valves_refs as VR
import hydraulics_refs as HR

H, G = HR.H, HR.G
EPS = HR.EPS
H0 = 50.0                               # the reservoir of the chains
E_HW = 1.0 / 1.852                      # the exponent at which demand and pipe add up in closed form
STOP_MARGIN = ER.STOP_MARGIN


def _case(net, demand, roughness, pdd, coef=None, setting=None):
    return {"net": net, "demand": demand, "roughness": roughness, "pdd": pdd, "coef": coef, "setting": setting}


def pdd_kw(c):
    pmin, preq, e = c["pdd"]
    return dict(demand_model="pda", minimum_pressure=pmin, required_pressure=preq, pressure_exponent=e)


def _chain(lengths, minor, elevation, demands, pdd):
    """reservoir 0 (H0) -- link 0 -- 1 -- link 1 -- 2 ...: a chain of pipes; ``demands`` {node: [S]}."""
    P = len(lengths)
    S = len(next(iter(demands.values())))
    net = H.HydraulicNetwork(HR._edge_index([(i, i + 1) for i in range(P)]), lengths, np.full(P, 0.2), elevation, [0], [H0],
                             minor_loss=minor)
    demand = np.zeros((S, P + 1))
    for node, d in demands.items():
        demand[:, node] = d
    return _case(net, demand, np.full((S, P), 100.0), pdd)


CHAINS = {
    # one pipe, e = 1 / 1.852: q = ((H0 - z - Pmin) / (r + dp / D^1.852))^(1 / 1.852)
    "chain_hw": lambda: _chain([100.0], [0.0], [0.0, 30.0], {1: [0.004, 0.01, 0.03]}, (5.0, 30.0, E_HW)),
    # a throttle link (r = 0, m > 0), e = 0.5: q = sqrt((H0 - z - Pmin) / (m + dp / D^2))
    "chain_throttle": lambda: _chain([0.0], [3.0], [0.0, 30.0], {1: [0.004, 0.01, 0.03]}, (5.0, 30.0, 0.5)),
    # the junction lies above the required pressure: it delivers D + (p - Preq) / 1e8
    "chain_full": lambda: _chain([100.0], [0.0], [0.0, 10.0], {1: [0.004, 0.01, 0.02]}, (0.0, 20.0, 0.5)),
    # the junction lies above the source head: it carries -|p - Pmin| / 1e8
    "chain_above": lambda: _chain([100.0], [0.0], [0.0, 60.0], {1: [0.004, 0.01, 0.02]}, (5.0, 30.0, 0.5)),
    # three junctions, all partial: against the shooting root on the first pipe's flow
    "chain3_e05": lambda: _chain([100.0, 150.0, 80.0], [0.0, 0.0, 1.5], [0.0, 25.0, 32.0, 28.0],
                                 {1: [0.004, 0.008, 0.02], 2: [0.006, 0.003, 0.01], 3: [0.002, 0.009, 0.015]}, (0.0, 30.0, 0.5)),
    "chain3_e1": lambda: _chain([100.0, 150.0, 80.0], [0.0, 0.0, 1.5], [0.0, 25.0, 32.0, 28.0],
                                {1: [0.004, 0.008, 0.02], 2: [0.006, 0.003, 0.01], 3: [0.002, 0.009, 0.015]}, (2.0, 40.0, 1.0)),
}
CLOSED_FORMS = ("chain_hw", "chain_throttle", "chain3_e05", "chain3_e1")


def _r(c, p):
    return c["net"].coef[p] / c["roughness"][:, p] ** 1.852


def chain_exact(name):
    """The delivered flows [S, junctions] of a chain of partial junctions without Newton: the closed form, or the shooting root
    on the first pipe's flow q_0 -- down the chain H_i = H_{i-1} - h_{i-1}(q_{i-1}), q_d,i = D_i ((H_i - z_i - Pmin) / dp)^e,
    q_i = q_{i-1} - q_d,i; the last pipe must end with nothing left -- taken to adjacent doubles by bisection."""
    c = case(name)
    net, (pmin, preq, e) = c["net"], c["pdd"]
    dp, z, D = preq - pmin, net.elevation, c["demand"]
    if name == "chain_hw":
        return (((H0 - z[1] - pmin) / (_r(c, 0) + dp / D[:, 1] ** 1.852)) ** (1.0 / 1.852))[:, None]
    if name == "chain_throttle":
        return np.sqrt((H0 - z[1] - pmin) / (net.minor[0] + dp / D[:, 1] ** 2))[:, None]
    J = net.num_nodes - 1

    def shoot(q0):
        head, q, out = np.full_like(q0, H0), q0.copy(), []
        for i in range(1, J + 1):
            head = head - _r(c, i - 1) * np.abs(q) ** 0.852 * q - net.minor[i - 1] * np.abs(q) * q
            x = np.clip((head - z[i] - pmin) / dp, 0.0, 1.0)
            out.append(D[:, i] * x ** e)
            q = q - out[-1]
        return q, np.stack(out, axis=1)
    q0 = ER._bisect(lambda q: -shoot(q)[0], np.zeros(D.shape[0]), D.sum(axis=1))
    delivered = shoot(q0)[1]
    assert ((delivered > 0) & (delivered < D[:, 1:])).all(), name           # every junction partial: the law above is the whole law
    return delivered


# ---- the synthetic networks ------------------------------------------------------------------------------------------------------
def _synthetic(N, P, R, S, seed, demand_hi, pdd, num_prvs=0, valve_seed=0, num_emitters=0, emitter_seed=0, coef_range=(2e-5, 2e-4)):
    """``make_hydraulic_network`` and the draws of hydraulics_refs.py (every junction draws a positive demand, so every junction
    is pressure-driven); with a PRV its setting is 0.6 x the pressure that its controlled node has pressure-driven without the
    valve, so that the valve regulates; the emitter coefficients are seeded uniform draws."""
    base = G.wdn_synth.make_hydraulic_network(N, P, R, seed=seed)
    net = base if not (num_prvs or num_emitters) else \
        G.wdn_synth.make_hydraulic_network(N, P, R, seed=seed, num_prvs=num_prvs, valve_seed=valve_seed, num_emitters=num_emitters,
                                           emitter_seed=emitter_seed)
    demand, roughness = HR._draws(base, S, seed, demand_hi)
    setting, coef = None, None
    if net.num_valves:
        free = H.solve_ref(base, demand, roughness, solver="banded", demand_model="pda", minimum_pressure=pdd[0],
                           required_pressure=pdd[1], pressure_exponent=pdd[2])
        setting = 0.6 * (free.head[:, net.valve_node] - net.elevation[net.valve_node][None, :])
    if net.num_emitters:
        coef = np.random.RandomState(seed + 101).uniform(coef_range[0], coef_range[1], (S, num_emitters))
    return _case(net, demand, roughness, pdd, coef, setting)


# (N, P, R, S, seed, demand ceiling, (Pmin, Preq, e), PRVs, valve_seed, emitters, emitter_seed): the layouts, the draws and the
# settings at which a pipes-only Newton loop with this law was seen to converge before the kernels were written
SYNTHETIC = {
    "net37": (37, 41, 1, 4, 3, 1e-3, (0.0, 20.0, 0.5)),                       # N < 64: most threads idle
    # a PRV and an emitter on pressure-driven junctions.  valve_seed 6 and emitter_seed 1 were taken: the valve is ACTIVE in two
    # scenarios and CLOSED in two, its controlled node gets 88 % of its demand where it is ACTIVE, and the emitter leaks beside
    # a partial demand (emitter_seed 0 puts it on a junction under negative pressure; valve seeds 1 and 3 are not decisive)
    "net40_prv_e1": (40, 44, 2, 4, 5, 3e-3, (5.0, 30.0, 0.5), 1, 6, 1, 1),
    "net388": (388, 430, 3, 4, 6, 1e-4, (0.0, 40.0, E_HW)),                   # N > HY_T: the node loops take a second trip
}
BUILDERS = dict(CHAINS)
BUILDERS.update({name: (lambda a=args: _synthetic(*a)) for name, args in SYNTHETIC.items()})
NAMES = tuple(BUILDERS)
# The generated store: the 388-node layout with every elevation below the lowest reservoir head the generator draws (60 m), so
# that no junction is under negative pressure at rest, and a demand range for which ``solve_ref`` demand-driven converges on all
# 32 drawn scenarios but leaves 3 of them with a negative junction pressure (down to -14.2 m): the demand-driven store drops
# those 3 as out_of_range at (0, 150), and pressure-driven ``solve_ref`` converges and keeps all 32 (the lowest pressure 1.4 m).
STORE_NET, STORE_ELEVATION, STORE_SCENARIOS, STORE_SEED, STORE_DEMAND, STORE_PRESSURE, STORE_PDD, STORE_DDA_DROPPED = \
    (388, 430, 3, 6), (3.48, 55.0), 32, 11, (3e-5, 3e-4), (0.0, 150.0), (0.0, 20.0, 0.5), 3


@functools.lru_cache(maxsize=None)
def store_network():
    N, P, R, seed = STORE_NET
    return G.wdn_synth.make_hydraulic_network(N, P, R, seed=seed, elevation_range=STORE_ELEVATION)


@functools.lru_cache(maxsize=None)
def store_reference():
    """The drawn scenarios of the store and what ``solve_ref`` keeps of them: (demand, roughness, kept demand-driven [S], kept
    pressure-driven [S], the pressure-driven reference).  Kept: converged, and every junction pressure, rounded to fp32 as the
    kernel stores it, inside STORE_PRESSURE."""
    net = store_network()
    d, r = H.hydraulic_draws(STORE_SEED, 0, STORE_SCENARIOS, *net.draw_ranges(STORE_DEMAND, H.ROUGHNESS_RANGE))
    pmin, preq, e = STORE_PDD
    dda = H.solve_ref(net, d, r, solver="banded")
    pda = H.solve_ref(net, d, r, solver="banded", demand_model="pda", minimum_pressure=pmin, required_pressure=preq, pressure_exponent=e)

    def kept(ref):
        p = (ref.head - net.elevation[None, :]).astype(np.float32)[:, ~net.fixed].astype(np.float64)
        with np.errstate(invalid="ignore"):
            return ref.converged & ~ref.failed & ((p >= STORE_PRESSURE[0]) & (p <= STORE_PRESSURE[1])).all(axis=1)
    return d, r, kept(dda), kept(pda), pda


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()


def solve(c, solver="dense", **kw):
    return H.solve_ref(c["net"], c["demand"], c["roughness"], solver=solver, valve_setting=c["setting"],
                       emitter_coefficient=c["coef"], **pdd_kw(c), **kw)


def residuals(c, head, flow, link_state, emitter_flow, delivered, **kw):
    return H.hydraulic_residuals(c["net"], head, flow, c["demand"], c["roughness"], valve_setting=c["setting"], link_state=link_state,
                                 emitter_flow=emitter_flow, emitter_coefficient=c["coef"], demand_delivered=delivered,
                                 **dict(pdd_kw(c), **kw))


def regimes(c, delivered):
    """Per scenario the numbers of junctions with q_d <= 0, partial and full."""
    j = ~c["net"].fixed & (c["demand"] > 0)
    zero, full = (delivered <= 0) & j, (delivered >= c["demand"]) & j
    return zero.sum(axis=1), (j & ~zero & ~full).sum(axis=1), full.sum(axis=1)


@functools.lru_cache(maxsize=None)
def reference(name):
    """dense, banded, their residuals, their mutual distance, the floors of the case (hydraulic_emitters_refs.reference; a
    delivered flow takes the floor of a link with its gradient) and ``decisive`` [S]; asserts that both converge in every
    scenario with the same statuses and, on a synthetic case, that every scenario has the three regimes and is decisive."""
    c = case(name)
    net = c["net"]
    pmin, preq, e = c["pdd"]
    dense, banded = solve(c, "dense"), solve(c, "banded")
    for ref in (dense, banded):
        assert ref.converged.all() and not ref.failed.any(), (name, ref.iterations, ref.converged)
    assert np.array_equal(dense.link_state, banded.link_state), name
    decisive = (dense.iterations == banded.iterations) & (dense.valve_changes == banded.valve_changes)
    for ref in (dense, banded):
        decisive &= (ref.margin[:, 0] >= VR.DECISIVE_H) & (ref.margin[:, 1] >= VR.DECISIVE_Q)
    decisive &= ER.stop_rule_decisive(lambda **kw: solve(c, "dense", **kw), dense.iterations)
    if name in SYNTHETIC:
        assert all((n > 0).all() for n in regimes(c, dense.demand_delivered)), (name, regimes(c, dense.demand_delivered))
        assert decisive.all(), (name, decisive, dense.iterations, banded.iterations)
    res_d = residuals(c, dense.head, dense.flow, dense.link_state, dense.emitter_flow, dense.demand_delivered)
    res_b = residuals(c, banded.head, banded.flow, banded.link_state, banded.emitter_flow, banded.demand_delivered)
    dh, dq = HR.distances(net, banded.head, banded.flow, dense)
    hmax = np.abs(dense.head).max(axis=1)
    span = dense.head.max(axis=1) - dense.head.min(axis=1)
    g = np.empty_like(dense.flow)
    for s in range(dense.flow.shape[0]):
        own = np.zeros(net.num_pipes, dtype=bool)
        own[net.valve_links] = dense.link_state[s, net.valve_links] == H.VALVE_CLOSED
        law = H.link_law(net)
        g[s] = H.link_headloss(dense.flow[s], H._link_resistance(net, c["roughness"][s]), **dict(law, shut=law["shut"] | own))[1]
    on = ~net.fixed[None, :] & (c["demand"] > 0)
    gd = np.where(on, H.demand_headloss(dense.demand_delivered, np.where(on, c["demand"], 1.0), preq - pmin, e)[1], np.inf)
    qmax = np.abs(dense.flow).max(axis=1)[:, None]
    floors = {"mass": np.full(hmax.shape, HR.FLOOR_ULPS * EPS), "energy": HR.FLOOR_ULPS * EPS * hmax,
              "dh": HR.FLOOR_ULPS * EPS * hmax / span,
              "flow": np.minimum(HR.FLOOR_ULPS * EPS * hmax[:, None] / g, H.ACCURACY * qmax),
              "delivered": np.minimum(HR.FLOOR_ULPS * EPS * hmax[:, None] / gd, H.ACCURACY * qmax)}
    if net.num_emitters:
        ge = H.emitter_headloss(dense.emitter_flow, c["coef"], net.emitter_exponent)[1]
        floors["emitter_flow"] = np.minimum(HR.FLOOR_ULPS * EPS * hmax[:, None] / ge, H.ACCURACY * qmax)
    for ref in (dense, banded):
        for v in (ref.head, ref.flow, ref.emitter_flow, ref.demand_delivered):
            v.setflags(write=False)
    return {"dense": dense, "banded": banded, "mass": np.maximum(res_d[0], res_b[0]), "energy": np.maximum(res_d[1], res_b[1]),
            "dh": dh, "dq": dq, "dd": np.abs(banded.demand_delivered - dense.demand_delivered) / qmax,
            "de": np.abs(banded.emitter_flow - dense.emitter_flow) / qmax, "floors": floors, "decisive": decisive}


# ---- the series -----------------------------------------------------------------------------------------------------------------------
def short_series():
    """reservoir 0 (60 m) -- 1 -- 2 -- tank 3 (bottom at 30 m, 3 m of water), Pmin 10 m and Preq 70 m: both junctions are below
    the required pressure whenever they draw.  Junction 2 follows a pattern of its own that is 0 at steps 1 and 2."""
    net = H.HydraulicNetwork(HR._edge_index([(0, 1), (1, 2), (2, 3)]), [400.0, 100.0, 200.0], np.full(3, 0.2), [0.0, 0.0, 5.0, 30.0],
                             [0, 3], [60.0, 33.0], tank_nodes=[3], tank_diameter=[8.0])
    demand = np.zeros((2, 4))
    demand[:, 1], demand[:, 2] = [0.01, 0.015], [0.012, 0.008]
    mult = np.array([[0.8, 1.0, 1.2, 1.0, 0.9, 1.1], [1.0, 0.0, 0.0, 1.0, 1.2, 0.5]])
    kw = dict(pattern_of_node=[0, 0, 1, 0], demand_model="pda", minimum_pressure=10.0, required_pressure=70.0)
    return net, demand, np.full((2, 3), 100.0), mult, 600.0, kw


# ---- planted wrong answers: hydraulic_residuals must catch each ------------------------------------------------------------------------
def wrong_residuals(kind, c):
    """(mass, energy) under the case's model of a solution that made one mistake about the demand: each is the converged host
    solution of a WRONG model, held to the right one."""
    net, (pmin, preq, e) = c["net"], c["pdd"]
    kw = dict(solver="banded", valve_setting=c["setting"], emitter_coefficient=c["coef"])
    if kind == "demand_in_full":                # the demand-driven solution, every demand delivered
        sol = H.solve_ref(net, c["demand"], c["roughness"], demand_model="dda", **kw)
    elif kind == "pmin_left_out":               # the virtual links end at the elevation, not at elevation + Pmin
        sol = H.solve_ref(net, c["demand"], c["roughness"], demand_model="pda", minimum_pressure=0.0, required_pressure=preq - pmin,
                          pressure_exponent=e, **kw)
    elif kind == "wrong_exponent":
        sol = H.solve_ref(net, c["demand"], c["roughness"], demand_model="pda", minimum_pressure=pmin, required_pressure=preq,
                          pressure_exponent=1.0 if e != 1.0 else 0.5, **kw)
    elif kind == "elevation_left_out":          # the demand held to the head, not the pressure
        flat = H.HydraulicNetwork.__new__(H.HydraulicNetwork)
        flat.__dict__.update(net.__dict__)
        flat.elevation = np.zeros_like(net.elevation)
        if net.num_valves:                      # (the valve keeps its target head)
            kw["valve_setting"] = c["setting"] + net.elevation[net.valve_node][None, :]
        sol = H.solve_ref(flat, c["demand"], c["roughness"], **pdd_kw(c), **kw)
    else:
        raise KeyError(kind)
    assert sol.converged.all(), kind
    return residuals(c, sol.head, sol.flow, sol.link_state, sol.emitter_flow, sol.demand_delivered)


WRONG = ("demand_in_full", "pmin_left_out", "wrong_exponent", "elevation_left_out")
