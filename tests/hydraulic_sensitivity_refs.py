"""The cases of the sensitivity and leak-localisation tests (gatres.h: THE SENSITIVITIES), shared by
test_hydraulic_sensitivity_host.py and test_gpu_hydraulic_sensitivity.py.  The networks are those of hydraulics_refs.py and
hydraulic_links_refs.py; what is added here is the sensor sets, the comparisons the GPU tests use (so that the host tests can hold
planted wrong answers against the very same functions), the planted leaks and the recorded figures of the reference.  Every bound
is formed from the reference's own error and the precision of fp64, never from a device result."""
import functools

import numpy as np

import hydraulic_links_refs as LR
import hydraulics_refs as HR

H, G, EPS = HR.H, HR.G, HR.EPS
TIGHT = 1e-10                         # the accuracy at which the finite differences and the planted leaks are solved
LEAK_FRACTION = 1e-3                  # a planted leak: 0.1 % of the scenario's total demand
# THE RECORDED FIGURES of the reference (test_hydraulic_sensitivity_host.py measures them and holds them;
# profiles/hydraulic_sensitivity_margins.txt lists what was measured): over net37_s3 and net40_s3, 4 and 8 sensors, scenario 0,
# every junction in turn leaking LEAK_FRACTION of the total demand, readings and model solved by ``solve_ref`` at TIGHT --
# the true node's score deficit to the top score, and the relative error of ``leak_flow`` at the true node.  They are properties of
# the first-order model (what the linearisation leaves out at a leak of this size), not of any device result; each is the
# measured maximum rounded up to the next power of ten.  A junction that no sensor sees (a column of zeros: net40_s3 has one, a
# dead end hanging off a reservoir) has no score and takes no part.
DEFICIT_RECORDED = 1e-6               # measured: 1.44e-10, 1.66e-10 (net37_s3, K = 4, 8), 1.05e-7, 8.7e-8 (net40_s3)
LEAK_FLOW_RECORDED = 1e-2             # measured: 2.4e-3, 5.8e-4 (net37_s3), 1.6e-3, 1.5e-3 (net40_s3)
FD_MAX_SKIPPED = 0.25                 # at most a quarter of the finite differences may have a leg that does not converge


def sensors_of(net, K, seed=0):
    """K distinct junctions (fewer where the network has fewer), drawn once per (network size, K, seed)."""
    j = net.junctions
    return np.sort(np.random.RandomState(1000 * seed + K).permutation(j)[:min(K, j.size)]).astype(np.int32)


def links_case(name):
    """A case of either refs file in one shape: (net, demand, roughness, heads, speed, closed)."""
    if name in HR.BUILDERS:
        net, demand, roughness, heads = HR.case(name)
        return net, demand, roughness, heads, None, None
    c = LR.case(name)
    return c["net"], c["demand"], c["roughness"], None, c["speed"], c["closed"]


# ---- the comparisons of the GPU tests -------------------------------------------------------------------------------------------------
def distance(got, ref):
    """Per scenario: max |got - ref| / max |ref| over the scenario's [K, *] block (0 where the reference is all zero and equal)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    S = ref.shape[0]
    diff = np.abs(got - ref).reshape(S, -1).max(axis=1)
    scale = np.abs(ref).reshape(S, -1).max(axis=1)
    with np.errstate(all="ignore"):
        return np.where(scale > 0, diff / scale, np.where(diff > 0, np.inf, 0.0))


def agreement_bound(dense, banded):
    """The project's rule for device against reference: AGREEMENT_FACTOR x the dense-to-banded distance of the two host solvers on
    the same matrix, the largest over the case's scenarios, with the floor of 64 ulp that ``HR.bound`` takes."""
    return float(HR.bound(np.nanmax(distance(banded, dense)), HR.FLOOR_ULPS * EPS, HR.AGREEMENT_FACTOR))


def compare(got_dd, got_dc, net, demand, roughness, sensors, flow, heads=None, speed=None, closed=None):
    """THE comparison of the GPU tests: a result's ``dh_ddemand`` and ``dh_droughness`` against ``sensitivity_ref`` at ``flow`` (the
    result's own returned flows: this isolates the linear algebra).  Returns {name: (figure per scenario, bound)}; a NaN
    anywhere in what is compared makes the figure inf."""
    kw = dict(fixed_head=heads, pump_speed=speed, link_closed=closed, flow=flow)
    dense = H.sensitivity_ref(net, demand, roughness, sensors, solver="dense", **kw)
    banded = H.sensitivity_ref(net, demand, roughness, sensors, solver="banded", **kw)
    out = {}
    for name, got, d, b in (("dh_ddemand", got_dd, dense.dh_ddemand, banded.dh_ddemand),
                            ("dh_droughness", got_dc, dense.dh_droughness, banded.dh_droughness)):
        if got is None:
            continue
        fig = distance(got, d)
        out[name] = (np.where(np.isnan(fig), np.inf, fig), agreement_bound(d, b))
    return out


def accepted(result):
    return all(bool((fig <= bound).all()) for fig, bound in result.values())


# ---- the fused localisation ---------------------------------------------------------------------------------------------------------------
def score_bound(K):
    """|score - leak_scores_ref's score| at most, for K sensors.  Each of <z, rho>, <z, z>, <rho, rho> is a sum of K rounded
    products, off by at most (K + 1) eps x the sum of the products' magnitudes, whether or not a compiler contracts product and
    sum into one rounding (contraction only drops roundings); by Cauchy-Schwarz sum |z_k rho_k| <= |z| |rho|, so the numerator
    is off by (K + 1) eps of the scale of the quotient, each of the two roots by (K + 1) eps / 2 relative, and the product and
    the quotient by one eps each plus one per root: (2 K + 6) eps for one evaluation with |score| <= 1, twice that between two."""
    return 2.0 * (2.0 * K + 6.0) * EPS


def leak_flow_bound(K, dh_ddemand, residual):
    """The same for ``leak_flow`` [S, N]: <z, rho> / <z, z> has the scale |rho| / |z|, so ``score_bound`` x that, per node."""
    Z, rho = np.asarray(dh_ddemand, dtype=np.float64), np.asarray(residual, dtype=np.float64)
    on = ~np.isnan(rho)
    r2 = np.where(on, rho * rho, 0.0).sum(axis=-1)
    z2 = np.where(on[..., None], Z * Z, 0.0).sum(axis=-2)
    with np.errstate(all="ignore"):
        return score_bound(Z.shape[-2]) * np.sqrt(r2)[..., None] / np.sqrt(z2)


# ---- the planted leaks ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def leak_case(name, K, scenario=0):
    """Every junction of the case's network in turn leaking LEAK_FRACTION of the scenario's total demand: the nominal scenario
    repeated once per junction (demand, roughness [J, *]), the leaks [J], and the reference's readings [J, K] (pressures at the
    sensors with the leak as an extra demand, ``solve_ref`` at TIGHT), nominal pressures, residuals and ``sensitivity_ref``."""
    net, demand, roughness, heads = HR.case(name)
    assert heads is None
    sens, J = sensors_of(net, K), net.junctions.size
    d0, c0 = demand[scenario], roughness[scenario]
    leak = LEAK_FRACTION * d0[~net.fixed].sum()
    d_leak = np.tile(d0, (J, 1))
    d_leak[np.arange(J), net.junctions] += leak
    nominal = H.solve_ref(net, d0[None], c0[None], accuracy=TIGHT, links=True)
    leaking = H.solve_ref(net, d_leak, np.tile(c0, (J, 1)), accuracy=TIGHT, links=True)
    assert nominal.converged.all() and leaking.converged.all(), (name, K)
    readings = leaking.head[:, sens] - net.elevation[sens]
    model = nominal.head[0, sens] - net.elevation[sens]
    Z = H.sensitivity_ref(net, d0[None], c0[None], sens, flow=nominal.flow).dh_ddemand[0]
    out = {"net": net, "sensors": sens, "demand": np.tile(d0, (J, 1)), "roughness": np.tile(c0, (J, 1)), "leak": leak,
           "readings": readings, "residual": readings - model[None, :], "dh_ddemand": Z, "nominal": nominal}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def leak_figures(score, leak_flow, true_nodes, leak):
    """(deficit [J], relative error of leak_flow at the true node [J]) of a localisation with one true node per row; NaN in a row
    without a score (a true node that no sensor sees)."""
    score, leak_flow, leak = np.asarray(score), np.asarray(leak_flow), np.asarray(leak, dtype=np.float64)
    rows = np.arange(score.shape[0])
    live = ~np.isnan(score)
    top = np.where(live.any(axis=1), np.where(live, score, -np.inf).max(axis=1), np.nan)
    return top - score[rows, true_nodes], np.abs(leak_flow[rows, true_nodes] - leak) / np.abs(leak)
