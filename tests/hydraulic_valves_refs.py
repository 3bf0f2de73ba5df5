"""The cases of the regulating-valve tests (PRV and PSV), shared by test_hydraulic_valves_host.py and test_gpu_hydraulic_valves.py:
each case is a network with its scenarios and its host reference (``solve_ref`` dense and banded with the valves' status machine),
built once and never changed.  The factors and the floors are those of hydraulics_refs.py; every bound is formed from the
reference's own error, never from a device result.  When a reference is built it is held to be DECISIVE: at every iteration every
comparison of the status rules was at least ``DECISIVE_H`` metres (``DECISIVE_Q`` m3/s for flows) from its threshold, in both host
solvers, so that a device result that differs from the reference by rounding takes the same statuses at every iteration and its
iterations, ``link_state`` and ``valve_changes`` can be held EQUAL to the reference's."""
import functools

import numpy as np

import hydraulics_refs as HR

H, G = HR.H, HR.G
EPS = HR.EPS
DECISIVE_H = 1e-3                       # metres
DECISIVE_Q = 100.0 * H.VALVE_QTOL       # m3/s
H0, LOW = 60.0, 20.0                    # the reservoirs of the chains


def _case(net, demand, roughness, setting=None):
    return {"net": net, "demand": demand, "roughness": roughness, "setting": setting}


def _chain(kind, setting, far_head=None, K=2.0, demands=(0.01, 0.02, 0.03), far_pipe=None):
    """PRV: reservoir 0 (H0) -- pipe 0 -- a = 1 -- valve -- b = 2 -- pipe 2 -- node 3 with the demand [-- pipe 3 -- reservoir 4 at
    ``far_head``].  PSV: reservoir 0 (H0) -- pipe 0 -- a = 1 with the demand -- valve -- b = 2 -- pipe 2 -- reservoir 3 at
    ``far_head``.  Elevations 0, so a setting is a head."""
    S = len(demands)
    if kind == "PRV":
        pairs, fixed, heads, N = [(0, 1), (1, 2), (2, 3)], [0], [H0], 4
        length = [100.0, 0.0, 100.0]
        if far_head is not None:
            pairs, fixed, heads, N, length = pairs + [(3, 4)], [0, 4], [H0, far_head], 5, length + [far_pipe or 100.0]
        node = 3
    else:
        pairs, fixed, heads, N, length, node = [(0, 1), (1, 2), (2, 3)], [0, 3], [H0, far_head], 4, [100.0, 0.0, 100.0], 1
    P = len(pairs)
    minor = np.zeros(P)
    minor[1] = K
    net = H.HydraulicNetwork(HR._edge_index(pairs), length, np.full(P, 0.2), np.zeros(N), fixed, heads, minor_loss=minor,
                             valve_links=[1], valve_kind=kind, valve_setting=[setting])
    demand = np.zeros((S, N))
    demand[:, node] = demands
    return _case(net, demand, np.full((S, P), 100.0))


CHAINS = {
    "prv_active": lambda: _chain("PRV", 40.0),
    "prv_open": lambda: _chain("PRV", 70.0),                        # the setting above what arrives
    "prv_closed_reverse": lambda: _chain("PRV", 40.0, far_head=80.0),      # a higher reservoir downstream
    "prv_closed_held": lambda: _chain("PRV", 40.0, far_head=50.0),  # a second reservoir holds H_b above hset
    "psv_active": lambda: _chain("PSV", 50.0, far_head=LOW),
    "psv_open": lambda: _chain("PSV", 10.0, far_head=LOW),          # the setting below what arrives
    "psv_closed_reverse": lambda: _chain("PSV", 50.0, far_head=80.0),
    "psv_closed_held": lambda: _chain("PSV", 70.0, far_head=LOW),   # the upstream reservoir cannot hold H_a at hset
}
CHAIN_STATE = {"prv_active": H.VALVE_ACTIVE, "prv_open": H.VALVE_OPEN, "prv_closed_reverse": H.VALVE_CLOSED,
               "prv_closed_held": H.VALVE_CLOSED, "psv_active": H.VALVE_ACTIVE, "psv_open": H.VALVE_OPEN,
               "psv_closed_reverse": H.VALVE_CLOSED, "psv_closed_held": H.VALVE_CLOSED}
# what a CLOSED valve still passes, dh / 1e8 <= 60 m / 1e8 = 6e-7 m3/s, moves the heads of the closed forms below by g times
# that, with g = 1.852 r q^0.852 <= 50 s/m2 in these pipes (r = 535, q <= 0.03): 3e-5 m
CLOSED_LEAK_FLOW = 6e-7
CLOSED_LEAK_HEAD = 3e-5


def _r(c, p):
    return c["net"].coef[p] / c["roughness"][:, p] ** 1.852


def _bisect(f, lo, hi):
    """The root of the decreasing f on [lo, hi], per scenario."""
    lo, hi = np.array(lo, dtype=np.float64), np.array(hi, dtype=np.float64)
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        up = f(mid) > 0
        lo, hi = np.where(up, mid, lo), np.where(up, hi, mid)
    return 0.5 * (lo + hi)


def chain_exact(name):
    """The closed form of a chain: {node: head [S]} and {link: flow [S]} for the entries it determines (a CLOSED valve's own
    leak is left out: ``CLOSED_LEAK_HEAD`` covers it)."""
    c = case(name)
    net, m = c["net"], c["net"].minor[1]
    if name.startswith("prv"):
        d = c["demand"][:, 3]
        if name == "prv_active":
            return {1: H0 - _r(c, 0) * d ** 1.852, 2: np.full_like(d, 40.0), 3: 40.0 - _r(c, 2) * d ** 1.852}, {0: d, 1: d, 2: d}
        if name == "prv_open":
            ha = H0 - _r(c, 0) * d ** 1.852
            return {1: ha, 2: ha - m * d * d, 3: ha - m * d * d - _r(c, 2) * d ** 1.852}, {0: d, 1: d, 2: d}
        far = net.fixed_head[4]
        h3 = far - _r(c, 3) * d ** 1.852                    # the demand comes from the far reservoir alone
        return {1: np.full_like(d, H0), 2: h3, 3: h3}, {3: -d}
    d = c["demand"][:, 1]
    far = net.fixed_head[3]
    if name == "psv_active":
        q0 = ((H0 - 50.0) / _r(c, 0)) ** (1.0 / 1.852)
        return {1: np.full_like(d, 50.0), 2: far + _r(c, 2) * (q0 - d) ** 1.852}, {0: q0, 1: q0 - d, 2: q0 - d}
    if name == "psv_open":                                  # q through the valve: H0 - r0 (q + d)^1.852 - m q^2 - r2 q^1.852 = far
        q = _bisect(lambda x: H0 - _r(c, 0) * (x + d) ** 1.852 - m * x * x - _r(c, 2) * x ** 1.852 - far, np.zeros_like(d), np.ones_like(d))
        ha = H0 - _r(c, 0) * (q + d) ** 1.852
        return {1: ha, 2: ha - m * q * q}, {0: q + d, 1: q, 2: q}
    return {1: H0 - _r(c, 0) * d ** 1.852, 2: np.full_like(d, far)}, {0: d}      # CLOSED: a is fed from reservoir 0 alone


# ---- the synthetic networks ------------------------------------------------------------------------------------------------------
def _synthetic_valves(N, P, R, S, seed, demand_hi, num_prvs, num_psvs, valve_seed):
    """``make_hydraulic_network`` with regulating valves; valve k of scenario s is set to 0.6 x or 1.4 x the pressure that its
    controlled node has in the same scenario of the network without valves, alternating over s + k."""
    base = G.wdn_synth.make_hydraulic_network(N, P, R, seed=seed)
    net = G.wdn_synth.make_hydraulic_network(N, P, R, seed=seed, num_prvs=num_prvs, num_psvs=num_psvs, valve_seed=valve_seed)
    demand, roughness = HR._draws(base, S, seed, demand_hi)
    pipe_only = H.solve_ref(base, demand, roughness, solver="banded")
    pressure = pipe_only.head[:, net.valve_node] - net.elevation[net.valve_node][None, :]
    factor = np.where((np.arange(S)[:, None] + np.arange(net.num_valves)[None, :]) % 2 == 0, 0.6, 1.4)
    return _case(net, demand, roughness, factor * pressure)


# (N, P, R, S, seed, demand_hi, PRVs, PSVs, valve_seed): layouts for which both host solvers converge in every scenario, decisively
SYNTHETIC = {
    "net37_v1": (37, 41, 1, 4, 3, 1e-3, 1, 0, 6),
    "net37_v2": (37, 41, 1, 4, 3, 1e-3, 1, 1, 6),
    "net37_v3": (37, 41, 1, 4, 3, 1e-3, 2, 1, 6),
    "net40_v1": (40, 44, 2, 4, 5, 1e-3, 1, 0, 6),
    "net40_v2": (40, 44, 2, 4, 5, 1e-3, 1, 1, 1),
    "net40_v3": (40, 44, 2, 4, 5, 1e-3, 2, 1, 3),
    "net388_v1": (388, 430, 3, 4, 6, 1e-3, 0, 1, 3),
    "net388_v2": (388, 430, 3, 4, 6, 1e-3, 1, 1, 2),
    "net388_v3": (388, 430, 3, 4, 6, 1e-3, 2, 1, 2),
}
BUILDERS = dict(CHAINS)
BUILDERS.update({name: (lambda a=args: _synthetic_valves(*a)) for name, args in SYNTHETIC.items()})
NAMES = tuple(BUILDERS)
# the generated store of the 40-node case: settings drawn per scenario and valve; a pressure range that no solved scenario leaves
STORE_CASE, STORE_SCENARIOS, STORE_SEED, STORE_DEMAND, STORE_SETTING, STORE_PRESSURE, STORE_MIN_KEPT = \
    "net40_v3", 64, 11, (1e-4, 1e-3), (20.0, 60.0), (-1e3, 1e3), 48


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()


def solve(c, solver="dense", **kw):
    return H.solve_ref(c["net"], c["demand"], c["roughness"], solver=solver, valve_setting=c["setting"], **kw)


def residuals(c, head, flow, link_state, **kw):
    return H.hydraulic_residuals(c["net"], head, flow, c["demand"], c["roughness"], valve_setting=c["setting"],
                                 link_state=link_state, **kw)


@functools.lru_cache(maxsize=None)
def reference(name):
    """dense, banded, their residuals, their mutual distance and the floors of the case (hydraulics_refs.reference, with the
    valves); asserts that both converge in every scenario, take the same statuses, and are decisive."""
    c = case(name)
    net = c["net"]
    dense, banded = solve(c, "dense"), solve(c, "banded")
    for ref in (dense, banded):
        assert ref.converged.all() and not ref.failed.any(), (name, ref.iterations, ref.converged)
        assert ref.margin[:, 0].min() >= DECISIVE_H and ref.margin[:, 1].min() >= DECISIVE_Q, (name, ref.margin)
    assert np.array_equal(dense.iterations, banded.iterations) and np.array_equal(dense.link_state, banded.link_state)
    assert np.array_equal(dense.valve_changes, banded.valve_changes)
    res_d = residuals(c, dense.head, dense.flow, dense.link_state)
    res_b = residuals(c, banded.head, banded.flow, banded.link_state)
    dh, dq = HR.distances(net, banded.head, banded.flow, dense)
    hmax = np.abs(dense.head).max(axis=1)
    span = dense.head.max(axis=1) - dense.head.min(axis=1)
    g = np.empty_like(dense.flow)
    for s in range(dense.flow.shape[0]):
        own = np.zeros(net.num_pipes, dtype=bool)
        own[net.valve_links] = dense.link_state[s, net.valve_links] == H.VALVE_CLOSED
        law = H.link_law(net)
        g[s] = H.link_headloss(dense.flow[s], H._link_resistance(net, c["roughness"][s]), **dict(law, shut=law["shut"] | own))[1]
    floors = {"mass": np.full(hmax.shape, HR.FLOOR_ULPS * EPS), "energy": HR.FLOOR_ULPS * EPS * hmax,
              "dh": HR.FLOOR_ULPS * EPS * hmax / span,
              "flow": np.minimum(HR.FLOOR_ULPS * EPS * hmax[:, None] / g, H.ACCURACY * np.abs(dense.flow).max(axis=1)[:, None])}
    for v in (dense.head, dense.flow, banded.head, banded.flow):
        v.setflags(write=False)
    return {"dense": dense, "banded": banded, "mass": np.maximum(res_d[0], res_b[0]), "energy": np.maximum(res_d[1], res_b[1]),
            "dh": dh, "dq": dq, "floors": floors}


# ---- planted wrong laws: hydraulic_residuals with one mistake about the valve -------------------------------------------------------
def wrong_residuals(kind, c, ref):
    """(mass, energy) of the reference's own solution under a wrong statement of the valve."""
    net = c["net"]
    if kind == "wrong_node":                    # the target head held at the valve's other end
        other = G.hydraulics.HydraulicNetwork.__new__(G.hydraulics.HydraulicNetwork)
        other.__dict__.update(net.__dict__)
        a, b = net.pipes[net.valve_links, 0], net.pipes[net.valve_links, 1]
        other.valve_node = np.where(net.valve_node == a, b, a)
        return H.hydraulic_residuals(other, ref.head, ref.flow, c["demand"], c["roughness"], valve_setting=c["setting"],
                                     link_state=ref.link_state)
    if kind == "active_as_open":                # an ACTIVE valve held to the open law: no loss but m q^2
        state = np.where(ref.link_state == H.VALVE_ACTIVE, H.VALVE_OPEN, ref.link_state)
        return residuals(c, ref.head, ref.flow, state)
    if kind == "setting_as_head":               # the setting taken for a head: the elevation left out (chains: 0; use an offset)
        return H.hydraulic_residuals(net, ref.head, ref.flow, c["demand"], c["roughness"],
                                     valve_setting=(net.valve_setting if c["setting"] is None else c["setting"]) + 1.0,
                                     link_state=ref.link_state)
    raise KeyError(kind)


WRONG_LAWS = ("wrong_node", "active_as_open", "setting_as_head")
