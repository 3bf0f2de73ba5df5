"""Hydraulic sensitivities and leak localisation, on the host (gatres.h: THE SENSITIVITIES): the new symbol is declared, exported
and bound without an ABI change and refuses its bad arguments before any launch; ``sensitivity_ref`` against central differences
of ``solve_ref``, against the closed form on trees, symmetric and zero at fixed nodes; ``leak_scores_ref`` on hand-computed cases;
the localisation condition of a small planted leak, held to the recorded figures; planted wrong answers are rejected by the
comparisons the GPU tests use; the LDS sum and the chunk rule against the literals of the kernel source.  No GPU, no kernel
launches.  Every figure is printed before it is asserted (profiles/hydraulic_sensitivity_margins.txt holds them)."""
import os
import re

import numpy as np
import pytest

import hydraulic_sensitivity_refs as SR

HR, LR, H, G = SR.HR, SR.LR, SR.H, SR.G
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gnn-pressure-estimation_amd", "csrc")
Q = 1 << 24                    # (any non-null addresses, far apart: a refused call never reads them)
NAME = "gatres_hydraulic_sensitivity"
ARGS = ("pipe_a", "pipe_b", "coef", "q_start", "fixed", "elevation", "order", "position", "W", "demand", "roughness",
        "fixed_head", "stride", "S", "N", "P", "accuracy", "max_iter", "pressure", "head", "flow", "status", "final_dq",
        "link_kind", "link_flags", "minor", "pump_link", "pump_h0", "pump_r", "pump_n", "Kp", "speed", "speed_stride",
        "closed", "closed_stride", "link_state", "sensor_node", "K", "chunk", "readings", "dh_ddemand", "dh_droughness",
        "residual", "leak_flow", "score", "best")
SCALARS = dict(W=2, stride=0, S=3, N=5, P=6, accuracy=1e-6, max_iter=40, Kp=2, speed_stride=0, closed_stride=0, K=4, chunk=0)
OUTPUTS = ("pressure", "head", "flow", "status", "final_dq", "link_state", "dh_ddemand", "dh_droughness", "residual", "leak_flow",
           "score", "best")


# ---- 1. symbols and refusals ----------------------------------------------------------------------------------------------------------
def test_sensitivity_symbol_is_declared_exported_and_bound_and_the_abi_stays(pkg, lib):
    with open(os.path.join(ROOT, "include", "gatres.h")) as f:
        text = f.read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\b%s\s*\(" % NAME, hdr) and "THE SENSITIVITIES" in text
    assert hasattr(lib, NAME), f"{NAME} is not exported"
    assert len(pkg._native.SIGNATURES[NAME][1]) == len(ARGS) + 1 == 47
    links = pkg._native.SIGNATURES["gatres_hydraulic_solve_links"][1]
    assert pkg._native.SIGNATURES[NAME][1][:36] == links[:36]                # the links arguments, unchanged and in the same order
    assert "#define GATRES_ABI_VERSION 9" in hdr and pkg._native.ABI_VERSION == 9 and b"abi9" in lib.gatres_version()
    assert pkg._build.SOURCES.count("k_hydraulic_sensitivity.hip") == 1
    for name in ("HydraulicSensitivityResult", "LeakLocalization", "sensitivity_ref", "leak_scores_ref", "localization_report",
                 "sensitivity_lds_bytes", "sensitivity_chunk"):
        assert name in pkg.__all__ and hasattr(pkg, name), name
    with open(os.path.join(CSRC, "k_hydraulic_sensitivity.hip")) as f:
        src = f.read()
    assert src.count("hy_newton<true>(") == 1 and "for (int it = 1;" not in src         # the Newton loop stays stated once
    with open(os.path.join(ROOT, "tests", "golden", "hydraulic_launches.json")) as f:
        assert NAME not in f.read()                                           # the launch record has no row for it


def call(lib, **kw):
    """S = 3, N = 5, P = 6, Kp = 2, K = 4: every array at its own address, 2^24 bytes apart."""
    a = dict(SCALARS)
    a.update({n: (i + 1) * Q for i, n in enumerate([n for n in ARGS if n not in SCALARS])})
    a.update(kw)
    return lib.gatres_hydraulic_sensitivity(*[a[n] for n in ARGS], None)


def test_sensitivity_checks_its_arguments_before_any_launch(lib):
    addr = {n: (i + 1) * Q for i, n in enumerate([n for n in ARGS if n not in SCALARS])}
    optional = OUTPUTS + ("closed", "readings")
    for name in addr:                                                     # everything the links entry point refuses ...
        if name not in optional:
            assert call(lib, **{name: None}) == -1, name
    for name in ("S", "N", "P"):
        assert call(lib, **{name: 0}) == -1 and call(lib, **{name: -1}) == -1, name
    assert call(lib, Kp=-1) == -1 and call(lib, Kp=7) == -1
    assert call(lib, speed_stride=1) == -1 and call(lib, closed_stride=5) == -1 and call(lib, closed=None, closed_stride=6) == -1
    assert call(lib, W=0) == -1 and call(lib, W=5) == -1 and call(lib, stride=1) == -1 and call(lib, max_iter=0) == -1
    for acc in (0.0, -1e-6, float("inf"), float("nan")):
        assert call(lib, accuracy=acc) == -1, acc
    assert call(lib, K=0) == -1 and call(lib, K=-1) == -1 and call(lib, chunk=-1) == -1       # ... K < 1, a negative chunk,
    assert call(lib, sensor_node=None) == -1                                                  # sensor_node NULL,
    assert call(lib, N=139, P=138, W=138, Kp=0) == -1                                         # the links arrays alone past the budget,
    # a band that fits the links launch and leaves no room for one right-hand side: Kc < 1
    N, P, W = 138, 137, 137
    assert H.links_lds_bytes(N, P, W, 0) <= H.LDS_BUDGET and H.sensitivity_chunk(N, P, W, 0, 4) == 0
    assert call(lib, N=N, P=P, W=W, Kp=0) == -1
    loc = dict(residual=None, leak_flow=None, score=None, best=None)
    assert call(lib, **loc) == -1                                                             # readings with no localisation output,
    for name in loc:                                                                          # one of those without readings,
        assert call(lib, **{**loc, name: addr[name], "readings": None}) == -1, name
    sizes = dict(pressure=4 * 3 * 5, head=8 * 3 * 5, flow=8 * 3 * 6, status=16 * 3, final_dq=8 * 3, link_state=18,
                 dh_ddemand=8 * 3 * 4 * 5, dh_droughness=8 * 3 * 4 * 6, residual=8 * 3 * 4, leak_flow=8 * 3 * 5, score=8 * 3 * 5, best=12)
    for name in OUTPUTS:                                                                      # and outputs that overlap
        assert call(lib, **{name: addr["minor"] + 47}) == -1, name                            # the last byte of minor
        assert call(lib, **{name: addr["sensor_node"] + 15}) == -1, name                      # the last byte of sensor_node
        assert call(lib, **{name: addr["readings"] + 8 * 3 * 4 - 1}) == -1, name
        for other in OUTPUTS:
            if other != name:
                assert call(lib, **{name: addr[other] + sizes[other] - 1}) == -1, (name, other)


# ---- 2. sensitivity_ref against finite differences ------------------------------------------------------------------------------------
def _central(net, demand, roughness, sens, what, index, step):
    """(central difference of the sensor heads [S, K], converged [S]) for a step of ``what`` at ``index`` in every scenario."""
    legs = []
    for sign in (1.0, -1.0):
        d, c = demand.copy(), roughness.copy()
        (d if what == "demand" else c)[:, index] += sign * step
        legs.append(H.solve_ref(net, d, c, accuracy=SR.TIGHT, links=True))
    ok = legs[0].converged & legs[1].converged
    return (legs[0].head[:, sens] - legs[1].head[:, sens]) / (2.0 * step), ok


@pytest.mark.parametrize("name", ("net37_s3", "net40_s3"))
def test_sensitivity_ref_equals_central_differences_of_solve_ref(name, capsys):
    """Eight junctions drawn at random, and the twelve pipes whose roughness moves the sensor heads most (in the scenario where it
    moves them least); a difference with a leg that does not converge at the tight accuracy is skipped and counted.
    TOLERANCES, from the two errors a central difference has.  NOISE: at accuracy 1e-10 the heads of two solves differ by about
    1e-9 m for reasons other than the step, and the steps here move the sensor heads by 1e-6 m or more (asserted), so noise is
    of the order of 1e-3 of the difference at worst.  TRUNCATION: the step is 1e-3 of the quantity (of the mean demand; of C),
    and the law is a power law, so the third-order term is of the order of 1e-6.  Bound: 2e-3 of the column's largest entry."""
    net, demand, roughness, _ = HR.case(name)
    sens = SR.sensors_of(net, 8)
    base = H.solve_ref(net, demand, roughness, accuracy=SR.TIGHT, links=True)
    assert base.converged.all()
    ref = H.sensitivity_ref(net, demand, roughness, sens, flow=base.flow)
    rng = np.random.RandomState(7)
    done, skipped, worst = 0, 0, {"demand": 0.0, "roughness": 0.0}
    with capsys.disabled():
        for what, picks, step, table in (("demand", rng.permutation(net.junctions)[:8], 1e-3 * demand[:, ~net.fixed].mean(), ref.dh_ddemand),
                                         ("roughness", np.argsort(-np.abs(ref.dh_droughness).max(axis=1).min(axis=0), kind="stable")[:12], 0.1,
                                          ref.dh_droughness)):
            for i in picks:
                fd, ok = _central(net, demand, roughness, sens, what, i, step)
                col = table[:, :, i]
                assert (np.abs(col).max(axis=1) * step >= 1e-6).all(), (what, i)
                held = ok
                skipped += int((~held).sum())
                done += int(held.sum())
                if held.any():
                    err = (np.abs(fd - col).max(axis=1) / np.abs(col).max(axis=1))[held].max()
                    worst[what] = max(worst[what], float(err))
        print(f"\n{name}: sensitivity_ref against central differences: dH/dd {worst['demand']:.3e}  dH/dC {worst['roughness']:.3e}  "
              f"(bound 2e-3); held {done}, skipped {skipped}")
    assert worst["demand"] <= 2e-3 and worst["roughness"] <= 2e-3
    assert skipped <= SR.FD_MAX_SKIPPED * (done + skipped)


# ---- 3. the closed form on trees --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("path12_s3", "tree37_s3"))
def test_on_a_tree_dh_ddemand_is_minus_the_gradients_on_the_common_path(name, capsys):
    """On a tree every pipe's flow is the demand behind it, so dH_k / dd_n = -sum of g_p over the pipes common to the two paths
    from the reservoir.  Both host solvers are held to it, within the reference's own error: AGREEMENT_FACTOR x their distance
    from one another on the same matrix (``SR.agreement_bound``: the gradients of tree37_s3 span five decades, and the dense
    solve loses 1e-11 to that)."""
    net, demand, roughness, heads = HR.case(name)
    N, P = net.num_nodes, net.num_pipes
    assert P == N - 1 and net.fixed.sum() == 1
    sens = net.junctions.astype(np.int32)
    flow = H.solve_ref(net, demand, roughness, heads).flow
    refs = {solver: H.sensitivity_ref(net, demand, roughness, sens, heads, flow=flow, solver=solver).dh_ddemand for solver in ("dense", "banded")}
    parent, via = np.full(N, -1), np.full(N, -1)
    queue, seen = [int(net.fixed_nodes[0])], {int(net.fixed_nodes[0])}
    for v in queue:
        for p, (a, b) in enumerate(net.pipes):
            w = int(b) if a == v else (int(a) if b == v else -1)
            if w >= 0 and w not in seen:
                seen.add(w)
                parent[w], via[w] = v, p
                queue.append(w)
    path = {}
    for n in range(N):
        path[n], v = set(), n
        while parent[v] >= 0:
            path[n].add(int(via[v]))
            v = parent[v]
    want = np.empty_like(refs["dense"])
    for s in range(demand.shape[0]):
        g = H.pipe_headloss(flow[s], net.coef / roughness[s] ** 1.852)[1]
        want[s] = [[-sum(g[p] for p in path[int(k)] & path[n]) for n in range(N)] for k in sens]
    bound = SR.agreement_bound(refs["dense"], refs["banded"])
    for solver, got in refs.items():
        worst = float(SR.distance(got, want).max())
        with capsys.disabled():
            print(f"\n{name}: {solver} against the closed form on the tree {worst:.3e} (bound {bound:.3e})")
        assert worst <= bound, solver


# ---- 4. properties ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("net37_s3", "net40_heads_s3", "net37_links"))
def test_sensitivity_ref_is_symmetric_and_zero_at_fixed_nodes(name, capsys):
    net, demand, roughness, heads, speed, closed = SR.links_case(name)
    sens = np.arange(net.num_nodes, dtype=np.int32)                      # every node a sensor, the fixed ones included
    ref = H.sensitivity_ref(net, demand, roughness, sens, heads, speed, closed)
    Z = ref.dh_ddemand
    assert np.isfinite(Z).all() and (Z[:, net.fixed, :] == 0).all() and (Z[:, :, net.fixed] == 0).all()
    assert not np.signbit(Z[:, net.fixed, :]).any() and not np.signbit(Z[:, :, net.fixed]).any()       # exactly +0.0
    J = ~net.fixed
    ZJ = Z[:, J][:, :, J]                                                # an outflow lowers every head it reaches, its own always
    assert (ZJ <= 0).all() and (ZJ[:, np.arange(J.sum()), np.arange(J.sum())] < 0).all()
    asym = float(np.abs(Z - Z.transpose(0, 2, 1)).max() / np.abs(Z).max())
    bound = HR.FLOOR_ULPS * HR.EPS * net.num_nodes
    with capsys.disabled():
        print(f"\n{name}: asymmetry of dh_ddemand {asym:.3e} (bound {bound:.3e})")
    assert asym <= bound
    assert (ref.dh_droughness[:, :, net.is_pump] == 0).all() and (ref.dh_droughness[:, net.fixed, :] == 0).all()


def test_sensitivity_ref_refuses_what_it_does_not_model():
    import hydraulic_valves_refs as VR
    valves = next(c["net"] for c in (VR.case(n) for n in VR.NAMES) if c["net"].has_valves)
    with pytest.raises(ValueError, match="regulating valves"):
        H.sensitivity_ref(valves, np.zeros((1, valves.num_nodes)), np.full((1, valves.num_pipes), 100.0), [int(valves.junctions[0])])
    net, demand, roughness, _ = HR.case("net37_s3")
    for bad in ([], [-1], [net.num_nodes]):
        with pytest.raises(ValueError, match="sensor_nodes"):
            H.sensitivity_ref(net, demand, roughness, bad)
    with pytest.raises(ValueError, match="solver"):
        H.sensitivity_ref(net, demand, roughness, [1], solver="sparse")


# ---- 5. leak_scores_ref on hand-computed cases ----------------------------------------------------------------------------------------------
def test_leak_scores_ref_on_hand_computed_cases():
    nan = np.nan
    # K = 2 sensors, N = 4 nodes: columns (3, 4), (1, 0), (0, 0) a zero column, (6, 8) twice the first
    Z = np.array([[3.0, 1.0, 0.0, 6.0], [4.0, 0.0, 0.0, 8.0]])
    score, leak, best = H.leak_scores_ref(Z, np.array([3.0, 4.0]))
    assert score.tolist()[:2] == [1.0, 0.6] and np.isnan(score[2]) and score[3] == 1.0
    assert leak.tolist()[:2] == [1.0, 3.0] and np.isnan(leak[2]) and leak[3] == 0.5
    assert best == 0 and best.dtype == np.int32                          # the planted exact tie (nodes 0 and 3) goes to the lower index
    score, leak, best = H.leak_scores_ref(Z[:, ::-1], np.array([3.0, 4.0]))
    assert best == 0 and score[0] == score[3] == 1.0                     # ... whichever of the two comes first
    # a missing reading: the sums run over the other sensor alone
    score, leak, best = H.leak_scores_ref(Z, np.array([nan, 2.0]))
    assert score[0] == 1.0 and np.isnan(score[1]) and np.isnan(score[2]) and leak[0] == 0.5 and np.isnan(leak[1]) and best == 0
    score, leak, best = H.leak_scores_ref(Z, np.array([-3.0, nan]))
    assert score.tolist()[:2] == [-1.0, -1.0] and leak.tolist()[:2] == [-1.0, -3.0] and score[3] == -1.0 and best == 0
    # a zero residual: no score, the least-squares flow is 0 where the column is not; no sensor at all: the same, and 0 / 0
    score, leak, best = H.leak_scores_ref(Z, np.zeros(2))
    assert np.isnan(score).all() and best == -1 and leak.tolist()[:2] == [0.0, 0.0] and np.isnan(leak[2])
    score, leak, best = H.leak_scores_ref(Z, np.array([nan, nan]))
    assert np.isnan(score).all() and best == -1 and np.isnan(leak).all()
    # batched, and a NaN matrix (a failed scenario)
    score, leak, best = H.leak_scores_ref(np.stack([Z, np.full_like(Z, nan)]), np.array([[3.0, 4.0], [3.0, 4.0]]))
    assert best.tolist() == [0, -1] and np.isnan(score[1]).all() and np.isnan(leak[1]).all() and score[0, 1] == 0.6


# ---- 6. the localisation condition ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,K", (("net37_s3", 4), ("net37_s3", 8), ("net40_s3", 4), ("net40_s3", 8)))
def test_a_small_leak_at_any_junction_scores_within_the_recorded_deficit_of_the_top(name, K, capsys):
    """An exact argmax hit is not identifiable (junctions behind the same sensor cut have proportional columns), so what is held
    is the true node's deficit to the top score and its least-squares flow, against THE RECORDED FIGURES."""
    c = SR.leak_case(name, K)
    net, Z, rho = c["net"], c["dh_ddemand"], c["residual"]
    score, leak, best = H.leak_scores_ref(np.broadcast_to(Z, (rho.shape[0],) + Z.shape), rho)
    deficit, rel = SR.leak_figures(score, leak, net.junctions, c["leak"])
    unseen = ~(Z[:, net.junctions] != 0).any(axis=0)
    assert np.array_equal(np.isnan(deficit), unseen) and unseen.sum() <= 1
    hits = float((best == net.junctions)[~unseen].mean())
    with capsys.disabled():
        print(f"\n{name} K={K}: leak {c['leak']:.3e} m3/s; deficit of the true node {np.nanmax(deficit):.3e} (recorded "
              f"{SR.DEFICIT_RECORDED:.0e}); leak_flow error {np.nanmax(rel):.3e} (recorded {SR.LEAK_FLOW_RECORDED:.0e}); exact hits "
              f"{hits:.2f}; junctions no sensor sees {int(unseen.sum())}")
    assert np.nanmax(deficit) <= SR.DEFICIT_RECORDED and (deficit[~unseen] >= 0).all()
    assert np.nanmax(rel) <= SR.LEAK_FLOW_RECORDED


# ---- 7. planted wrong answers -----------------------------------------------------------------------------------------------------------
def test_planted_wrong_answers_are_rejected_by_the_comparisons_of_the_gpu_tests(capsys):
    """The stand-in for a right device result is the banded host solve at the flows ``solve_ref`` returned; each wrong answer is
    that with one mistake, and ``SR.compare`` -- what test_gpu_hydraulic_sensitivity.py asserts with -- must refuse it."""
    net, demand, roughness, _ = HR.case("net37_s3")
    assert not np.array_equal(net.order, np.arange(net.num_nodes))       # (solver order and node order differ on this case)
    sens = SR.sensors_of(net, 6)
    assert not np.array_equal(net.order[sens], sens)
    sol = H.solve_ref(net, demand, roughness, links=True)
    assert sol.converged.all() and (sol.iterations > 2).all()
    good = H.sensitivity_ref(net, demand, roughness, sens, flow=sol.flow, solver="banded")
    stale_flow = np.stack([H.solve_ref(net, demand[s:s + 1], roughness[s:s + 1], links=True, max_iter=int(sol.iterations[s]) - 1).flow[0]
                           for s in range(demand.shape[0])])            # the flows before the last update
    stale = H.sensitivity_ref(net, demand, roughness, sens, flow=stale_flow, solver="banded")
    node_order = H.sensitivity_ref(net, demand, roughness, net.order[sens], flow=sol.flow, solver="banded")
    check = lambda dd, dc: SR.compare(dd, dc, net, demand, roughness, sens, sol.flow)
    cases = {"right": (good.dh_ddemand, good.dh_droughness), "sign flip": (-good.dh_ddemand, good.dh_droughness),
             "g before the last flow update": (stale.dh_ddemand, stale.dh_droughness),
             "pipe direction transposed": (good.dh_ddemand, -good.dh_droughness),
             "sensor row in node order": (node_order.dh_ddemand, node_order.dh_droughness)}
    with capsys.disabled():
        print()
        for what, (dd, dc) in cases.items():
            res = check(dd, dc)
            print(f"{what}: " + "  ".join(f"{k} {fig.max():.3e} (bound {b:.3e})" for k, (fig, b) in res.items()))
            assert SR.accepted(res) == (what == "right"), what
    # the localisation comparisons: a score off by more than its bound, and a best that is not the lowest index of the maximum
    Z, rho = good.dh_ddemand, np.random.RandomState(3).normal(size=(demand.shape[0], sens.size))
    score, leak, best = H.leak_scores_ref(Z, rho)
    assert np.array_equal(H.best_score_ref(score), best)
    bumped = score.copy()
    bumped[0, best[0]] = np.nextafter(bumped[0, best[0]], 2.0) + 4 * SR.score_bound(sens.size)
    assert np.nanmax(np.abs(bumped - score)) > SR.score_bound(sens.size)
    tie = score.copy()
    tie[0, net.junctions[-1]] = tie[0, best[0]] = np.nanmax(score[0])
    assert H.best_score_ref(tie)[0] == min(best[0], net.junctions[-1])


# ---- 8. the LDS sum and the chunk rule ----------------------------------------------------------------------------------------------------
def test_sensitivity_lds_bytes_and_chunk_are_the_literals_of_the_kernel_source():
    with open(os.path.join(CSRC, "k_hydraulic_sensitivity.hip")) as f:
        src = f.read()
    m = re.search(r"hy_sens_lds_bytes\([^)]*\)\s*\{\s*return hy_links_lds_bytes\(N, P, W, Kp\) \+ (\d+) \* N \+ (\d+) \* Kc \* \(N \+ (\d+)\);", src)
    assert m, "the LDS sum of the kernel source is not where this test reads it"
    per_row, per_rhs, extra = (int(v) for v in m.groups())
    m2 = re.search(r"\+ (\d+) \* N;\s*if \(base >= HY_LDS_BUDGET\) return 0;\s*const uint64_t fit = \(HY_LDS_BUDGET - base\) / \((\d+) \* \(N \+ (\d+)\)\);", src)
    assert m2 and tuple(int(v) for v in m2.groups()) == (per_row, per_rhs, extra)
    for N, P, W, Kp, K in ((388, 430, 19, 0, 100), (388, 430, 19, 0, 20), (388, 430, 26, 4, 42), (37, 41, 8, 2, 8), (2, 1, 1, 0, 1),
                           (138, 137, 137, 0, 3), (139, 138, 138, 0, 3)):
        links = H.links_lds_bytes(N, P, W, Kp)
        room = H.LDS_BUDGET - links - per_row * N
        want = max(0, min(K, room // (per_rhs * (N + extra))))
        assert H.sensitivity_chunk(N, P, W, Kp, K) == want, (N, P, W, Kp, K)
        for kc in (1, want, want + 1):
            assert H.sensitivity_lds_bytes(N, P, W, Kp, kc) == links + per_row * N + per_rhs * kc * (N + extra)
        if want:
            assert H.sensitivity_lds_bytes(N, P, W, Kp, want) <= H.LDS_BUDGET
            assert want == K or H.sensitivity_lds_bytes(N, P, W, Kp, want + 1) > H.LDS_BUDGET
    # the figures gatres.h gives: 388 / 430 / W = 19 without pumps
    assert H.links_lds_bytes(388, 430, 19, 0) == 92264 and H.sensitivity_chunk(388, 430, 19, 0, 100) == 21
    assert H.sensitivity_chunk(138, 137, 137, 0, 3) == 0 and H.sensitivity_chunk(139, 138, 138, 0, 3) == 0
