"""The cases of the emitter (leak) tests, shared by test_hydraulic_emitters_host.py and test_gpu_hydraulic_emitters.py: each case is a
network with emitters, its scenarios and its host reference (``solve_ref`` dense and banded with the emitters' node term), built
once and never changed.  The factors, the floors and ``bound`` are those of hydraulics_refs.py; every bound is formed from the
reference's own error, never from a device result.  A scenario's reference is DECISIVE where, in both host solvers, every
comparison of the valves' status rules was at least ``hydraulic_valves_refs.DECISIVE_H`` / ``DECISIVE_Q`` from its threshold, both
took the same iterations, and the stop rule was nowhere near its threshold: the iterations stay the same with the accuracy
moved by ``STOP_MARGIN`` either way (rounding moves sum |dq| / sum |q| by some 1e-12 of itself).  A device result that differs by
rounding then takes the same iterations and statuses, which are held EQUAL."""
import functools

import numpy as np

import hydraulic_valves_refs as VR
import hydraulics_refs as HR

H, G = HR.H, HR.G
EPS = HR.EPS
H0 = 50.0                               # the reservoir of the chains
GAMMA_HW = 1.0 / 1.852                  # the exponent at which emitter and pipe add up in closed form
STOP_MARGIN = 1e-3                      # relative: the stop rule is decisive where the accuracy x (1 +- this) changes no iteration count


def stop_rule_decisive(solve, iterations):
    """Where ``solve(accuracy=)`` takes ``iterations`` at the accuracy moved by STOP_MARGIN either way."""
    out = np.ones(np.shape(iterations), dtype=bool)
    for factor in (1.0 - STOP_MARGIN, 1.0 + STOP_MARGIN):
        out &= solve(accuracy=H.ACCURACY * factor).iterations == iterations
    return out


def _case(net, demand, roughness, coef, setting=None):
    return {"net": net, "demand": demand, "roughness": roughness, "coef": coef, "setting": setting}


def _chain(lengths, minor, elevation, emitter, gamma, coefs, demands=None):
    """reservoir 0 (H0) -- link 0 -- 1 -- link 1 -- 2 ...: a chain with one emitter at the node ``emitter``; ``coefs`` [S] are the
    scenarios' coefficients, ``demands`` {node: [S]}."""
    P, S = len(lengths), len(coefs)
    N = P + 1
    net = H.HydraulicNetwork(HR._edge_index([(i, i + 1) for i in range(P)]), lengths, np.full(P, 0.2), elevation, [0], [H0],
                             minor_loss=minor, emitter_nodes=[emitter], emitter_exponent=gamma)
    demand = np.zeros((S, N))
    for node, d in (demands or {}).items():
        demand[:, node] = d
    return _case(net, demand, np.full((S, P), 100.0), np.asarray(coefs, dtype=np.float64)[:, None])


CHAINS = {
    # one pipe, gamma = 1 / 1.852: q = ((H0 - z) / (r + C^-1.852))^(1 / 1.852)
    "chain_hw": lambda: _chain([100.0], [0.0], [0.0, 10.0], 1, GAMMA_HW, [1e-3, 2e-3, 5e-3]),
    # a throttle link (r = 0, m > 0), gamma = 0.5: q = sqrt((H0 - z) / (m + 1 / C^2))
    "chain_throttle": lambda: _chain([0.0], [3.0], [0.0, 10.0], 1, 0.5, [1e-4, 1e-3, 4e-3]),
    # the junction lies above the source head: the emitter is shut, |q_e| <= |p| / 1e8
    "chain_shut": lambda: _chain([100.0], [0.0], [0.0, 60.0], 1, 0.5, [1e-3, 2e-3, 5e-3]),
    # three and four nodes, a demand on the way: against the bisection root
    "chain3_g118": lambda: _chain([100.0, 150.0], [0.0, 0.0], [0.0, 5.0, 12.0], 2, 1.18, [2e-5, 1e-4, 3e-4],
                                  {1: [0.004, 0.008, 0.002]}),
    "chain4_g1_tiny": lambda: _chain([100.0, 150.0, 80.0], [0.0, 0.0, 1.5], [0.0, 5.0, 12.0, 8.0], 3, 1.0, [1e-6, 1e-5, 1e-4],
                                     {1: [0.004, 0.008, 0.002], 2: [0.001, 0.001, 0.003]}),
}


def _r(c, p):
    return c["net"].coef[p] / c["roughness"][:, p] ** 1.852


def _bisect(f, lo, hi):
    """The root of the decreasing f on [lo, hi], per scenario, taken to adjacent doubles."""
    lo, hi = np.array(lo, dtype=np.float64), np.array(hi, dtype=np.float64)
    for _ in range(1100):
        mid = 0.5 * (lo + hi)
        up = f(mid) > 0
        lo, hi = np.where(up, mid, lo), np.where(up, hi, mid)
    assert (np.nextafter(lo, np.inf) >= hi).all()
    return lo


def chain_exact(name):
    """The emitter's flow [S] of a chain without Newton: the closed form, or the bisection root of the head balance along the
    chain H0 - sum_p h_p(q + demand downstream of p) - z - (q / C)^(1 / gamma) = 0."""
    c = case(name)
    net, C = c["net"], c["coef"][:, 0]
    z = net.elevation[net.emitter_nodes[0]]
    if name == "chain_hw":
        return ((H0 - z) / (_r(c, 0) + C ** -1.852)) ** (1.0 / 1.852)
    if name == "chain_throttle":
        return np.sqrt((H0 - z) / (net.minor[0] + 1.0 / C ** 2))
    n = 1.0 / net.emitter_exponent
    e = int(net.emitter_nodes[0])
    below = [c["demand"][:, p + 1:e + 1].sum(axis=1) for p in range(e)]         # the demand downstream of link p, up to the emitter

    def f(q):
        h = H0 - z - (q / C) ** n
        for p in range(e):
            x = q + below[p]
            h = h - _r(c, p) * x ** 1.852 - net.minor[p] * x * x
        return h
    return _bisect(f, np.zeros_like(C), np.ones_like(C))


# ---- the synthetic networks ------------------------------------------------------------------------------------------------------
def _synthetic(N, P, R, S, seed, demand_hi, num_prvs, num_psvs, valve_seed, num_emitters, gamma, coef_range):
    """``make_hydraulic_network`` with valves and emitters; the settings as in hydraulic_valves_refs.py (0.6 x or 1.4 x the
    pressure the controlled node has without valves), the coefficients seeded uniform draws per scenario and emitter."""
    base = G.wdn_synth.make_hydraulic_network(N, P, R, seed=seed)
    net = G.wdn_synth.make_hydraulic_network(N, P, R, seed=seed, num_prvs=num_prvs, num_psvs=num_psvs, valve_seed=valve_seed,
                                             num_emitters=num_emitters, emitter_exponent=gamma)
    demand, roughness = HR._draws(base, S, seed, demand_hi)
    setting = None
    if net.num_valves:
        pipe_only = H.solve_ref(base, demand, roughness, solver="banded")
        pressure = pipe_only.head[:, net.valve_node] - net.elevation[net.valve_node][None, :]
        setting = np.where((np.arange(S)[:, None] + np.arange(net.num_valves)[None, :]) % 2 == 0, 0.6, 1.4) * pressure
    coef = np.random.RandomState(seed + 101).uniform(coef_range[0], coef_range[1], (S, num_emitters))
    return _case(net, demand, roughness, coef, setting)


# (N, P, R, S, seed, demand_hi, PRVs, PSVs, valve_seed, emitters, gamma, coefficient range): layouts for which both host solvers
# converge in every scenario (checked when the reference is built)
SYNTHETIC = {
    "net37_e1_g05": (37, 41, 1, 4, 3, 1e-3, 1, 0, 6, 1, 0.5, (2e-5, 2e-4)),
    "net37_e2_g1": (37, 41, 1, 4, 3, 1e-3, 1, 1, 6, 2, 1.0, (2e-6, 2e-5)),
    "net40_e2_g05": (40, 44, 2, 4, 5, 1e-3, 0, 0, 0, 2, 0.5, (2e-5, 2e-4)),
    "net40_e3_g118": (40, 44, 2, 4, 5, 1e-3, 2, 1, 3, 3, 1.18, (1e-6, 1e-5)),
}
BUILDERS = dict(CHAINS)
BUILDERS.update({name: (lambda a=args: _synthetic(*a)) for name, args in SYNTHETIC.items()})
NAMES = tuple(BUILDERS)
# the generated store: the 388-node network with three emitters
STORE_NET, STORE_SCENARIOS, STORE_SEED, STORE_DEMAND, STORE_COEF, STORE_LEAK_P, STORE_PRESSURE = \
    (388, 430, 3, 6, 3, 0.5), 64, 11, (1e-5, 1e-4), (1e-5, 1e-4), 0.5, (-1e3, 1e3)


@functools.lru_cache(maxsize=None)
def store_network():
    N, P, R, seed, Ke, gamma = STORE_NET
    return G.wdn_synth.make_hydraulic_network(N, P, R, seed=seed, num_emitters=Ke, emitter_exponent=gamma)


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()


def solve(c, solver="dense", **kw):
    return H.solve_ref(c["net"], c["demand"], c["roughness"], solver=solver, valve_setting=c["setting"],
                       emitter_coefficient=c["coef"], **kw)


def residuals(c, head, flow, link_state, emitter_flow, **kw):
    return H.hydraulic_residuals(c["net"], head, flow, c["demand"], c["roughness"], valve_setting=c["setting"], link_state=link_state,
                                 emitter_flow=emitter_flow, **dict({"emitter_coefficient": c["coef"]}, **kw))


@functools.lru_cache(maxsize=None)
def reference(name):
    """dense, banded, their residuals, their mutual distance, the floors of the case (hydraulic_valves_refs.reference, with the
    emitters: an emitter's flow takes the floor of a link with its gradient) and ``decisive`` [S]; asserts that both converge in
    every scenario and take the same statuses."""
    c = case(name)
    net = c["net"]
    dense, banded = solve(c, "dense"), solve(c, "banded")
    for ref in (dense, banded):
        assert ref.converged.all() and not ref.failed.any(), (name, ref.iterations, ref.converged)
    assert np.array_equal(dense.link_state, banded.link_state), name
    decisive = (dense.iterations == banded.iterations) & (dense.valve_changes == banded.valve_changes)
    for ref in (dense, banded):
        decisive &= (ref.margin[:, 0] >= VR.DECISIVE_H) & (ref.margin[:, 1] >= VR.DECISIVE_Q)
    decisive &= stop_rule_decisive(lambda **kw: solve(c, "dense", **kw), dense.iterations)
    res_d = residuals(c, dense.head, dense.flow, dense.link_state, dense.emitter_flow)
    res_b = residuals(c, banded.head, banded.flow, banded.link_state, banded.emitter_flow)
    dh, dq = HR.distances(net, banded.head, banded.flow, dense)
    hmax = np.abs(dense.head).max(axis=1)
    span = dense.head.max(axis=1) - dense.head.min(axis=1)
    g = np.empty_like(dense.flow)
    for s in range(dense.flow.shape[0]):
        own = np.zeros(net.num_pipes, dtype=bool)
        own[net.valve_links] = dense.link_state[s, net.valve_links] == H.VALVE_CLOSED
        law = H.link_law(net)
        g[s] = H.link_headloss(dense.flow[s], H._link_resistance(net, c["roughness"][s]), **dict(law, shut=law["shut"] | own))[1]
    ge = H.emitter_headloss(dense.emitter_flow, c["coef"], net.emitter_exponent)[1]
    qmax = np.abs(dense.flow).max(axis=1)[:, None]
    floors = {"mass": np.full(hmax.shape, HR.FLOOR_ULPS * EPS), "energy": HR.FLOOR_ULPS * EPS * hmax,
              "dh": HR.FLOOR_ULPS * EPS * hmax / span,
              "flow": np.minimum(HR.FLOOR_ULPS * EPS * hmax[:, None] / g, H.ACCURACY * qmax),
              "emitter_flow": np.minimum(HR.FLOOR_ULPS * EPS * hmax[:, None] / ge, H.ACCURACY * qmax)}
    for v in (dense.head, dense.flow, dense.emitter_flow, banded.head, banded.flow, banded.emitter_flow):
        v.setflags(write=False)
    return {"dense": dense, "banded": banded, "mass": np.maximum(res_d[0], res_b[0]), "energy": np.maximum(res_d[1], res_b[1]),
            "dh": dh, "dq": dq, "de": np.abs(banded.emitter_flow - dense.emitter_flow) / qmax, "floors": floors, "decisive": decisive}


# ---- planted wrong answers: hydraulic_residuals must catch each ------------------------------------------------------------------------
def wrong_residuals(kind, c, ref):
    """(mass, energy) of the reference's own solution under one mistake about the emitters."""
    if kind == "leak_forgotten":                # the mass balance without q_e
        return residuals(c, ref.head, ref.flow, ref.link_state, np.zeros_like(ref.emitter_flow))
    if kind == "wrong_exponent":                # gamma = 1 where the network has another, and the reverse
        other = H.HydraulicNetwork.__new__(H.HydraulicNetwork)
        other.__dict__.update(c["net"].__dict__)
        other.emitter_exponent = 1.0 if c["net"].emitter_exponent != 1.0 else 0.5
        return H.hydraulic_residuals(other, ref.head, ref.flow, c["demand"], c["roughness"], valve_setting=c["setting"],
                                     link_state=ref.link_state, emitter_flow=ref.emitter_flow, emitter_coefficient=c["coef"])
    if kind == "pressure_as_head":              # the emitter held to the head, not the pressure: the elevation left out
        law = lambda q, C, gamma: (H.emitter_headloss(q, C, gamma)[0] + 1.0, None)
        return residuals(c, ref.head, ref.flow, ref.link_state, ref.emitter_flow, emitter_law=law)
    if kind == "coefficient_doubled":
        return residuals(c, ref.head, ref.flow, ref.link_state, ref.emitter_flow, emitter_coefficient=2.0 * c["coef"])
    raise KeyError(kind)


WRONG = ("leak_forgotten", "wrong_exponent", "pressure_as_head", "coefficient_doubled")
