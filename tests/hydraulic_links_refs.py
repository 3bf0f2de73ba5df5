"""The cases of the link-law tests (pumps, check valves, closed links, minor losses), shared by test_hydraulic_links_host.py and
test_gpu_hydraulic_links.py: each case is a network with its scenarios and its host reference (``solve_ref`` dense and banded
under THE LINK LAW), built once and never changed.  The factors and the floors are those of hydraulics_refs.py; every bound is
formed from the reference's own error, never from a device result."""
import functools

import numpy as np

import hydraulics_refs as HR

H, G = HR.H, HR.G
EPS = HR.EPS
# the generated store of net40_links: the demand range of the case's own scenarios, speeds as the issue sets them, and a pressure
# range that no solved scenario leaves (the elevations are drawn over 110 m), so that what is dropped is what does not converge
STORE_SCENARIOS, STORE_SEED, STORE_DEMAND, STORE_SPEED, STORE_PRESSURE = 64, 11, (1e-4, 1e-3), (0.8, 1.2), (-1e3, 1e3)
DECISIVE = 1e-3                      # metres: a checked link's |dh - h(0)| in the reference is above this in every chosen case


def _net(pairs, length, diameter, elevation, fixed, head, **kw):
    return H.HydraulicNetwork(HR._edge_index(pairs), length, diameter, elevation, fixed, head, **kw)


def _const(net, S, demand, roughness=100.0):
    d = np.zeros((S, net.num_nodes))
    d[:, ~net.fixed] = np.asarray(demand, dtype=np.float64).reshape(S, -1)
    return d, np.full((S, net.num_pipes), float(roughness))


def _case(net, demand, roughness, speed=None, closed=None):
    return {"net": net, "demand": demand, "roughness": roughness, "speed": speed, "closed": closed}


def pump_two():
    """reservoir 0 -- pump -- junction 1 with demand d: H = H0 + w^2 h0 - w^(2-n) rp d^n.  Three speeds, n = 2 and n = 1.5."""
    out = {}
    for n in (2.0, 1.5):
        net = _net([(0, 1)], [10.0], [0.2], [0.0, 5.0], [0], [20.0], pump_links=[0], pump_h0=[40.0], pump_r=[2000.0], pump_n=[n])
        demand, roughness = _const(net, 3, [0.05, 0.02, 0.08])
        out[n] = _case(net, demand, roughness, np.array([[1.0], [0.8], [1.2]]))
    return out


def pump_two_exact(c):
    net, d, w = c["net"], c["demand"][:, 1], c["speed"][:, 0]
    n = net.pump_n[0]
    return 20.0 + w * w * 40.0 - w ** (2.0 - n) * 2000.0 * d ** n


def pump_shut():
    """low reservoir 0 -- pump -- junction 1 -- pipe -- high reservoir 2 (80 m), no demand.  At speeds 0.8, 1 and 1.2 the pump
    (h0 = 40) is held shut: both links carry -(H2 - H0 - w^2 h0) / 1e8 (the pipe's own loss at such a flow, 1e-9 m, is part of
    the reference's distance from this form); at 1.5 it runs."""
    net = _net([(0, 1), (1, 2)], [10.0, 100.0], [0.2, 0.2], [0.0, 5.0, 0.0], [0, 2], [20.0, 80.0], pump_links=[0], pump_h0=[40.0],
               pump_r=[2000.0])
    demand, roughness = _const(net, 4, [0.0, 0.0, 0.0, 0.0])
    return _case(net, demand, roughness, np.array([[0.8], [1.0], [1.2], [1.5]]))


def pump_shut_exact(c):
    """Flow of both links per scenario: the closed form where shut; where it runs, a bisection of
    w^2 h0 - rp q^2 - r q^1.852 = H2 - H0 on q."""
    net, w = c["net"], c["speed"][:, 0]
    r = net.coef[1] / c["roughness"][0, 1] ** 1.852
    out = np.empty(w.size)
    for s, ws in enumerate(w):
        lift = ws * ws * 40.0
        if lift <= 60.0:
            out[s] = -(60.0 - lift) / 1e8
            continue
        lo, hi = 0.0, 1.0
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if lift - 2000.0 * mid * mid - r * mid ** 1.852 > 60.0 else (lo, mid)
        out[s] = 0.5 * (lo + hi)
    return out


def cv_reverse():
    """reservoir 0 (50 m) -- pipe -- junction 1 -- CV pipe 1 -> 2 -- reservoir 2 (70 m): the CV points uphill, from the junction
    to the higher reservoir, so nothing may pass from 2 to 1 and the junction is fed from 0 alone; the CV carries -dh / 1e8."""
    net = _net([(0, 1), (1, 2)], [100.0, 100.0], [0.2, 0.2], [0.0, 5.0, 0.0], [0, 2], [50.0, 70.0], check_valve=[False, True])
    demand, roughness = _const(net, 2, [0.01, 0.03])
    return _case(net, demand, roughness)


def closed_loop():
    """A triangle 0-1-2 with reservoir 0 and pipe (1, 2) closed: the tree 0-1, 0-2."""
    rng = np.random.RandomState(5)
    length, diameter, elev = rng.uniform(50, 500, 3), rng.uniform(0.1, 0.3, 3), rng.uniform(0, 20, 3)
    net = _net([(0, 1), (0, 2), (1, 2)], length, diameter, elev, [0], [60.0], closed=[False, False, True])
    tree = _net([(0, 1), (0, 2)], length[:2], diameter[:2], elev, [0], [60.0])
    demand, roughness = HR._draws(net, 3, 5, 2e-3)
    c = _case(net, demand, roughness)
    c["tree"] = tree
    return c


def minor_and_tcv():
    """reservoir 0 -- link -- junction 1: a pipe with a minor loss (both terms) and a throttle valve (length 0: m only)."""
    both = _net([(0, 1)], [200.0], [0.15], [0.0, 3.0], [0], [45.0], minor_loss=[7.5])
    tcv = _net([(0, 1)], [0.0], [0.15], [0.0, 3.0], [0], [45.0], minor_loss=[120.0])
    return {"minor": _case(both, *_const(both, 3, [0.01, 0.02, 0.04], 110.0)), "tcv": _case(tcv, *_const(tcv, 3, [0.01, 0.02, 0.04], 110.0))}


def single_link_exact(c):
    net, d = c["net"], c["demand"][:, 1]
    r = net.coef[0] / c["roughness"][:, 0] ** 1.852
    return 45.0 - r * d ** 1.852 - net.minor[0] * d * d


def _synthetic_links(N, P, R, S, seed, demand_hi, num_pumps, num_cv, minor_hi=0.0, speeds=(1.0,), pick=1):
    """``make_hydraulic_network`` with special links put on it: pumps on links that leave a reservoir, pointing away from it,
    sized to add about 10 m at the pipe-only flow; check valves on random pipes, every second one against the pipe-only flow
    (it engages), the others along it, and only on pipes that lose more than 0.05 m one way in every pipe-only scenario; minor losses on every pipe.  A choice the constructor refuses (a zone cut off) is
    skipped."""
    base = G.wdn_synth.make_hydraulic_network(N, P, R, seed=seed)
    demand, roughness = HR._draws(base, S, seed, demand_hi)
    pipe_only = H.solve_ref(base, demand, roughness)
    flow = pipe_only.flow[0]
    drop = pipe_only.head[:, base.pipes[:, 0]] - pipe_only.head[:, base.pipes[:, 1]]
    steady = (np.abs(drop).min(axis=0) > 50.0 * DECISIVE) & (np.sign(drop) == np.sign(drop[0])).all(axis=0)      # decisive pipes only
    rng = np.random.RandomState(seed + pick)
    a, b = base.pipes[:, 0], base.pipes[:, 1]
    at_res = np.flatnonzero(base.fixed[a] ^ base.fixed[b])
    pumps = list(rng.permutation(at_res)[:num_pumps])
    flip = np.zeros(P, dtype=bool)
    flip[pumps] = base.fixed[b[pumps]]                              # from the reservoir to the junction
    rest = [p for p in rng.permutation(P) if p not in pumps and steady[p] and not (base.fixed[a[p]] or base.fixed[b[p]])]
    check = np.zeros(P, dtype=bool)
    kw = dict(pump_links=pumps, pump_h0=np.full(len(pumps), 30.0),
              pump_r=[20.0 / max(abs(flow[p]), 1e-4) ** 2 for p in pumps], pump_n=np.full(len(pumps), 2.0))
    minor = rng.uniform(0.0, minor_hi, P) if minor_hi > 0 else np.zeros(P)
    minor[pumps] = 0.0
    build = lambda: H.HydraulicNetwork(base.edge_index, base.length, base.diameter, base.elevation, base.fixed_nodes,
                                       base.fixed_head[base.fixed_nodes], minor_loss=minor, check_valve=check, link_reversed=flip, **kw)
    placed = 0
    for p in rest:
        if placed == num_cv:
            break
        against = placed % 2 == 1
        check[p], old = True, flip[p]
        flip[p] = (flow[p] < 0) ^ against
        try:
            build()
            placed += 1
        except ValueError:
            check[p], flip[p] = False, old
    assert placed == num_cv
    net = build()
    speed = np.asarray(speeds, dtype=np.float64)[rng.randint(0, len(speeds), (S, len(pumps)))]
    return _case(net, demand, roughness, speed)


BUILDERS = {
    "net37_links": lambda: _synthetic_links(37, 41, 1, 3, 3, 1e-3, 2, 5),
    "net40_links": lambda: _synthetic_links(40, 44, 2, 3, 5, 1e-3, 2, 4, speeds=(0.8, 1.0, 1.2), pick=3),
    "net388_links": lambda: _synthetic_links(388, 430, 3, 3, 6, 1e-3, 4, 20, minor_hi=5.0, speeds=(0.0, 0.8, 1.0, 1.2), pick=8),
}
NAMES = tuple(BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()


def solve(c, solver="dense", **kw):
    return H.solve_ref(c["net"], c["demand"], c["roughness"], solver=solver, pump_speed=c["speed"], link_closed=c["closed"], **kw)


def residuals(c, head, flow, **kw):
    return H.hydraulic_residuals(c["net"], head, flow, c["demand"], c["roughness"], pump_speed=c["speed"], link_closed=c["closed"], **kw)


@functools.lru_cache(maxsize=None)
def reference(name):
    """dense, banded, their residuals, their mutual distance, the floors of the case (hydraulics_refs.reference, under the link
    law) and how far the checked links sit from the switch."""
    c = case(name)
    net = c["net"]
    dense, banded = solve(c, "dense"), solve(c, "banded")
    res_d, res_b = residuals(c, dense.head, dense.flow), residuals(c, banded.head, banded.flow)
    dh, dq = HR.distances(net, banded.head, banded.flow, dense)
    hmax = np.abs(dense.head).max(axis=1)
    span = dense.head.max(axis=1) - dense.head.min(axis=1)
    g = np.stack([H.link_headloss(dense.flow[s], np.where(net.is_pump, 0.0, net.coef / c["roughness"][s] ** 1.852),
                                  **H.link_law(net, c["speed"][s]))[1] for s in range(dense.flow.shape[0])])
    floors = {"mass": np.full(hmax.shape, HR.FLOOR_ULPS * EPS), "energy": HR.FLOOR_ULPS * EPS * hmax,
              "dh": HR.FLOOR_ULPS * EPS * hmax / span,
              "flow": np.minimum(HR.FLOOR_ULPS * EPS * hmax[:, None] / g, H.ACCURACY * np.abs(dense.flow).max(axis=1)[:, None])}
    # a checked link's distance from its switch: dh - h(0), with h(0) = -w^2 h0 for a pump
    a, b = net.pipes[:, 0], net.pipes[:, 1]
    lift = np.zeros_like(dense.flow)
    if net.num_pumps:
        lift[:, net.pump_links] = c["speed"] ** 2 * net.pump_h0[None, :]
    margin = np.abs(dense.head[:, a] - dense.head[:, b] + lift)
    margin = margin[(dense.link_state != 2) & (net.check_valve & ~net.closed)[None, :]]         # (a shut link is not checked)
    return {"dense": dense, "banded": banded, "mass": np.maximum(res_d[0], res_b[0]), "energy": np.maximum(res_d[1], res_b[1]),
            "dh": dh, "dq": dq, "floors": floors, "margin": margin}


# ---- planted wrong laws: each is link_headloss with one mistake ------------------------------------------------------------------
def _wrong(kind):
    def law(q, r, minor=0.0, pump=False, check=False, shut=False, h0=0.0, rp=1.0, n=1.0, speed=1.0):
        q = np.asarray(q, dtype=np.float64)
        h, g = H.link_headloss(q, r, minor, pump, check, shut, h0, rp, n, speed)
        pump, w = np.asarray(pump, dtype=bool), np.asarray(speed, dtype=np.float64)
        if kind == "pump_sign":                     # the shut-off head added to the loss
            return np.where(pump, h + 2.0 * w * w * h0, h), g
        if kind == "w2_for_w2n":                    # w^2 in place of w^(2-n)
            fwd = pump & (q >= 0)
            return np.where(fwd, -w * w * h0 + w * w * rp * np.maximum(q, 0.0) ** n, h), g
        if kind == "no_reverse":                    # a CHECK pipe that lets the water back: the odd extension of its forward law
            back = -H.link_headloss(-q, r, minor, shut=shut)[0]
            return np.where(np.asarray(check, dtype=bool) & ~pump & (q < 0), back, h), g
        raise KeyError(kind)
    return law


WRONG_LAWS = ("pump_sign", "w2_for_w2n", "no_reverse")
wrong_law = _wrong
