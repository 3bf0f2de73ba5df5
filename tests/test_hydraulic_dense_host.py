"""The cases of hydraulic_dense_refs.py are what they claim to be: every size above HY_T, emitters on and off on both sides of index
256, both host solvers converged, equal and decisive in every scenario and step, the three valve statuses, a status change in a
warm step, the three regimes of the demand model, onsets inside the series, every LDS need inside the budget and the budget case
one node below its end -- and the comparisons that test_gpu_hydraulic_dense.py makes reject four planted wrong answers, each the
converged host solution of a wrong model.  No GPU.  Every figure is printed before it is asserted."""
import os
import re

import numpy as np
import pytest

import hydraulic_dense_refs as DR
import hydraulics_refs as HR

H, G = HR.H, HR.G
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_sizes_lie_above_the_workgroup_and_emitters_are_on_and_off_on_both_sides_of_it():
    source = open(os.path.join(ROOT, "gnn-pressure-estimation_amd", "csrc", "k_hydraulics_dev.h")).read()
    assert int(re.search(r"constexpr int HY_T = (\d+);", source).group(1)) == DR.HY_T == 256
    for c in (DR.steady_case(1), DR.steady_case(2), DR.series_case(False), DR.series_case(True)):
        net, coef = c["net"], c["coef"]
        assert net.num_nodes > DR.HY_T and net.num_pipes > DR.HY_T and net.num_emitters > DR.HY_T
        assert net.num_pumps >= 1 and net.check_valve.any() and (net.minor > 0).any()
        assert (net.valve_kind == H.LINK_PRV).any() and (net.valve_kind == H.LINK_PSV).any()
        for side in (slice(0, DR.HY_T), slice(DR.HY_T, None)):
            assert ((coef[:, side] == 0).any(axis=1) & (coef[:, side] > 0).any(axis=1)).all()
        assert np.unique(net.emitter_nodes).size == net.num_emitters and not net.fixed[net.emitter_nodes].any()
        assert (np.sort(net.emitter_nodes)[-1] >= DR.HY_T) and (c["speed"] != 1.0).any()
    c0 = DR.steady_case(0)                                  # LV 0: the same layout without emitters
    assert c0["net"].num_emitters == 0 and np.array_equal(c0["net"].pipes, DR.steady_case(1)["net"].pipes)
    assert np.array_equal(c0["net"].valve_links, DR.steady_case(1)["net"].valve_links) and 3 <= c0["demand"].shape[0] <= 4
    s = DR.series_case(True)
    assert s["net"].num_tanks == 2 and s["mult"].shape == (DR.PATTERNS, DR.STEPS) and DR.PATTERNS >= 3 and DR.SERIES >= 2
    assert set(s["pattern"].tolist()) == set(range(DR.PATTERNS)) and (s["smult"] != 1.0).any() and (s["smult"] >= 0.8).all()
    assert (s["mult"] > 0).all() and ((s["onset"] > 0) & (s["onset"] < DR.STEPS) & (s["coef"] > 0)).any(axis=1).all()
    assert not np.array_equal(s["onset"][0], s["onset"][1])


@pytest.mark.parametrize("level", DR.LEVELS)
def test_dense_steady_converges_decisively_in_both_solvers(level, capsys):
    c, ref = DR.steady_case(level), DR.steady_reference(level)
    dense, banded, net = ref["dense"], ref["banded"], c["net"]
    states = dense.link_state[:, net.valve_links]
    with capsys.disabled():
        print(f"dense_steady LV {level}: W {net.half_bandwidth}  iterations {dense.iterations.tolist()}  changes {dense.valve_changes.tolist()}  "
              f"valve states {states.tolist()}  margins {dense.margin.min(axis=0).tolist()}  mass {ref['mass'].max():.3e}  "
              f"energy {ref['energy'].max():.3e}  dh {ref['dh'].max():.3e}  dq {ref['dq'].max():.3e}")
    for r in (dense, banded):
        assert r.converged.all() and not r.failed.any() and (r.iterations < H.MAX_ITER).all()
    assert np.array_equal(dense.iterations, banded.iterations) and np.array_equal(dense.link_state, banded.link_state)
    assert np.array_equal(dense.valve_changes, banded.valve_changes) and ref["decisive"].all()
    if level:
        on = c["coef"] > 0
        assert (dense.emitter_flow[~on] == 0).all() and not np.signbit(dense.emitter_flow[~on]).any() and (dense.emitter_flow[on] > 0).any()
    if level == 2:
        zero, part, full = DR.regimes(c, dense.demand_delivered)
        with capsys.disabled():
            print(f"dense_steady LV 2: q_d <= 0 / partial / full {zero.tolist()} / {part.tolist()} / {full.tolist()}")
        assert (zero > 0).all() and (part > 0).all() and (full > 0).all()


def test_the_three_valve_statuses_occur_over_dense_steady():
    seen = set()
    for level in DR.LEVELS:
        net = DR.steady_case(level)["net"]
        seen |= set(DR.steady_reference(level)["dense"].link_state[:, net.valve_links].ravel().tolist())
    assert seen >= {H.VALVE_OPEN, H.VALVE_ACTIVE, H.VALVE_CLOSED}


@pytest.mark.parametrize("warm,pda", DR.SERIES_VARIANTS)
def test_dense_series_converges_decisively_in_both_solvers(warm, pda, capsys):
    c, ref = DR.series_case(pda), DR.series_reference(warm, pda)
    dense, banded = ref["dense"], ref["banded"]
    with capsys.disabled():
        print(f"dense_series warm={warm} pda={pda}: iterations {dense.iterations.tolist()}  changes {dense.valve_changes.tolist()}  "
              f"levels {dense.level[:, [0, -1]].round(3).tolist()}  mass {ref['mass'].max():.3e}  energy {ref['energy'].max():.3e}")
    for r in (dense, banded):
        assert r.converged.all() and not r.failed.any() and not r.limited.any() and (r.iterations < H.MAX_ITER).all()
    assert np.array_equal(dense.iterations, banded.iterations) and np.array_equal(dense.link_state, banded.link_state)
    assert np.array_equal(dense.valve_changes, banded.valve_changes) and ref["decisive"].all()
    if warm:                                                # a status that a warm series carried changes in a later step
        assert (dense.valve_changes[:, 1:] > 0).any()
        cold = DR.series_reference(False, pda)["dense"]
        assert not np.array_equal(dense.iterations, cold.iterations)
    T = DR.STEPS
    live = (np.arange(T)[None, :, None] >= c["onset"][:, None, :]) & (c["coef"][:, None, :] > 0)
    assert ((dense.emitter_flow != 0) == live).all() and not np.signbit(dense.emitter_flow[~live]).any()
    if pda:
        zero, part, full = DR.regimes(ref["steps"], DR.flat(DR.solution(dense)).demand_delivered)
        assert (zero > 0).all() and (part > 0).all() and (full > 0).all()


def test_every_lds_need_is_inside_the_budget_and_the_budget_case_ends_one_node_below_it(capsys):
    net = DR.steady_case(2)["net"]
    steady = H.pdd_lds_bytes(net.num_nodes, net.num_pipes, net.half_bandwidth, net.num_pumps, net.num_valves, net.num_emitters)
    net = DR.series_case(True)["net"]
    series = H.series_pdd_lds_bytes(net.num_nodes, net.num_pipes, net.half_bandwidth, net.num_tanks, net.num_pumps, net.num_valves,
                                    net.num_emitters)
    N = DR.budget_nodes()
    need = lambda n: H.series_pdd_lds_bytes(n, n - 1, n - 1, 1, 0, 0, n - 2)
    with capsys.disabled():
        print(f"LDS: dense_steady {steady}  dense_series {series}  dense_budget N = {N}: {need(N)}, N + 1: {need(N + 1)}  of {H.LDS_BUDGET}")
    assert steady <= H.LDS_BUDGET and series <= H.LDS_BUDGET and need(N) <= H.LDS_BUDGET < need(N + 1)
    b = DR.budget_case()["net"]
    assert (b.num_nodes, b.num_pipes, b.half_bandwidth, b.num_tanks, b.num_emitters) == (N, N - 1, N - 1, 1, N - 2)
    ref = DR.budget_reference()
    assert ref["dense"].converged.all() and ref["banded"].converged.all() and (ref["dense"].emitter_flow > 0).any()
    assert np.array_equal(ref["dense"].iterations, ref["banded"].iterations)


def test_the_scenarios_on_either_side_of_the_capped_grid_differ_in_regime(capsys):
    c, pairs = DR.cap_case()
    rows = np.array([s for pair in pairs for s in pair])
    sub = DR.rows(c["net"], c["demand"][rows], c["roughness"][rows], None, c["speed"][rows], c["setting"][rows], c["coef"][rows], c["pdd"])
    ref = DR.solve(sub, "banded")
    states = ref.link_state[:, c["net"].valve_links]
    with capsys.disabled():
        print(f"cap_case S = {c['demand'].shape[0]}: scenarios {rows.tolist()}  iterations {ref.iterations.tolist()}  valve states {states.tolist()}")
    assert c["demand"].shape[0] == HR.ABOVE_CAP and ref.converged.all() and c["net"].num_emitters > DR.HY_T
    for i, (s, t) in enumerate(pairs):
        assert t == s + H.GRID_CAP and not np.array_equal(states[2 * i], states[2 * i + 1])
        assert not np.array_equal(c["coef"][s] == 0, c["coef"][t] == 0) and not np.array_equal(c["demand"][s] == 0, c["demand"][t] == 0)
        assert (c["demand"][t][~c["net"].fixed] == 0).any()


@pytest.mark.parametrize("key", tuple(("steady", lv) for lv in DR.LEVELS) + tuple(("series",) + v for v in DR.SERIES_VARIANTS))
def test_right_answers_with_other_roundings_meet_the_comparisons(key, capsys):
    """ROBUST: the host solutions with every roughness moved by one ulp take the reference's iterations and statuses and meet
    every bound that the GPU test holds the device to."""
    for name, cmp, same in DR.moved_answers(*key):
        with capsys.disabled():
            print(f"{key} {name}: same statuses {same}  {DR.report(cmp)}")
        assert same and not DR.exceeded(cmp), (name, DR.exceeded(cmp))


@pytest.mark.parametrize("kind", DR.WRONG)
def test_the_comparisons_reject_planted_wrong_answers(kind, capsys):
    """Each wrong answer converged under its wrong model; held to the GPU test's own comparisons it exceeds a bound, and a wrong
    answer about the carried statuses differs from the reference in iterations or ``link_state``."""
    cmp, right, wrong = DR.wrong_answer(kind)
    missed = DR.exceeded(cmp)
    with capsys.disabled():
        print(f"{kind}: exceeds {missed}  {DR.report(cmp)}  same statuses {DR.same_statuses(right, wrong)}")
    assert missed
    if kind in DR.WRONG_STATUS:
        assert not DR.same_statuses(right, wrong)
    assert not DR.exceeded({k: (v * 0.0, b, own) for k, (v, b, own) in cmp.items()})     # (a result without error meets every bound)
