"""The hydraulic network kernels (k_hydraulic_network.hip on hy_newton_valves) with every feature on at once and every per-record loop
on its second trip, against the host references of hydraulic_dense_refs.py: a 300-node layout with pumps, check valves, minor
losses, two PRVs, a PSV and 280 emitters -- steady at LV 0, 1 and 2 against ``solve_ref``; series with two tanks, three demand
patterns, a speed pattern and emitter onsets, warm and cold, demand-driven and pressure-driven, against ``simulate_series_ref``;
every bit of a cold series against steady launches of its steps; every bit of scenarios on either side of the capped grid against
launches of their own, where the two scenarios of one workgroup differ in every regime that it keeps in LDS; the largest
pressure-driven series the LDS budget admits; a duplicate emitter node whose pair straddles the first trip.  The comparisons are
``hydraulic_dense_refs.comparisons``: every bound comes from the reference.  Every figure is printed before it is asserted
(profiles/hydraulic_dense_margins.txt holds them: device value / bound / the reference's own value per comparison)."""
import gc

import numpy as np
import pytest
import torch

import hydraulic_dense_refs as DR
import hydraulics_refs as HR

pytestmark = pytest.mark.gpu
H, G = HR.H, HR.G
STEADY = ("pressure", "head", "flow", "status", "final_dq", "link_state", "valve_changes")
SERIES = ("pressure", "head", "flow", "level", "status", "final_dq", "link_state", "valve_changes")
FIELDS = {0: (), 1: ("emitter_flow",), 2: ("emitter_flow", "demand_delivered")}


@pytest.fixture(scope="module", autouse=True)
def own_memory_pool():
    """This module's device memory comes from a pool of its own and goes back when the module ends, with the cached cases: the
    caching allocator then hands the tests that run after it the blocks it would hand them without this module."""
    pool = torch.cuda.MemPool()
    routed = torch.cuda.use_mem_pool(pool)
    routed.__enter__()
    yield
    for cached in DR.CACHED:
        cached.cache_clear()
    gc.collect()
    torch.cuda.synchronize()
    routed.__exit__(None, None, None)


def host(result, fields):
    torch.cuda.synchronize()
    return {k: getattr(result, k).cpu().numpy() for k in fields}


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def level_of(c):
    return 0 if not c["net"].num_emitters else (2 if c["pdd"] is not None else 1)


def run(c):
    """The rows ``c`` in one steady launch."""
    return host(c["net"].simulate(c["demand"], c["roughness"], **DR.model_kw(c)), STEADY + FIELDS[level_of(c)])


def run_series(c, warm):
    fields = SERIES + FIELDS[2 if c["pdd"] is not None else 1]
    return host(c["net"].simulate_series(c["demand"], c["roughness"], c["mult"], step_seconds=c["dt"], warm_start=warm, **DR.series_kw(c)),
                fields)


# ---- 1. steady, per level ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", DR.LEVELS)
def test_dense_steady_against_the_reference(level, capsys):
    """``comparisons``; iterations, link_state and valve_changes EQUAL to the reference's (every scenario is decisive); an emitter
    with coefficient 0 returns +0.0 below and above index 256."""
    c, ref = DR.steady_case(level), DR.steady_reference(level)
    dense = ref["dense"]
    raw = run(c)
    got = DR.solution(raw)
    cmp = DR.comparisons(c, ref, DR.solution(dense), got)
    with capsys.disabled():
        print(f"dense_steady LV {level}: iterations {got.iterations.tolist()} (reference {dense.iterations.tolist()})  changes "
              f"{got.valve_changes.tolist()}  valve states {got.link_state[:, c['net'].valve_links].tolist()}  {DR.report(cmp)}")
    assert raw["status"][:, 1].all() and not raw["status"][:, 2:].any()
    assert ref["decisive"].all() and DR.same_statuses(dense, got), (got.iterations, dense.iterations)
    assert not DR.exceeded(cmp), DR.exceeded(cmp)
    if level:
        off = c["coef"] == 0
        for side in (slice(0, DR.HY_T), slice(DR.HY_T, None)):
            assert off[:, side].any() and (got.emitter_flow[:, side][off[:, side]] == 0).all()
            assert not np.signbit(got.emitter_flow[:, side][off[:, side]]).any() and (got.emitter_flow[:, side][~off[:, side]] > 0).any()
    else:
        assert "emitter_flow" not in raw
    if level == 2:
        zero, part, full = DR.regimes(c, got.demand_delivered)
        assert (zero > 0).all() and (part > 0).all() and (full > 0).all()


# ---- 2. the series ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("warm,pda", DR.SERIES_VARIANTS)
def test_dense_series_against_the_reference(warm, pda, capsys):
    """``series_comparisons``: the steady comparisons at every step, the levels and the volume balance; iterations, link_state and
    valve_changes EQUAL per step; an emitter's flow is +0.0 before its onset."""
    c, ref = DR.series_case(pda), DR.series_reference(warm, pda)
    dense = ref["dense"]
    raw = run_series(c, warm)
    got = DR.solution(raw)
    cmp = DR.series_comparisons(c, ref, got)
    with capsys.disabled():
        print(f"dense_series warm={warm} pda={pda}: iterations {got.iterations.tolist()} (reference {dense.iterations.tolist()})  changes "
              f"{got.valve_changes.tolist()}  {DR.report(cmp)}")
    assert raw["status"][..., 1].all() and not raw["status"][..., 2:].any()
    assert ref["decisive"].all() and DR.same_statuses(dense, got), (got.iterations, dense.iterations)
    assert not DR.exceeded(cmp), DR.exceeded(cmp)
    live = (np.arange(DR.STEPS)[None, :, None] >= c["onset"][:, None, :]) & (c["coef"][:, None, :] > 0)
    assert ((got.emitter_flow != 0) == live).all() and not np.signbit(got.emitter_flow[~live]).any() and (got.emitter_flow > 0).any()
    assert (live[:, :, DR.HY_T:].any(axis=(1, 2)) & (~live)[:, :, DR.HY_T:].any(axis=(1, 2))).all()
    if warm:
        assert (got.valve_changes[:, 1:] > 0).any()


# ---- 3. bits: a cold series against steady launches ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pda", (False, True))
def test_every_step_of_a_cold_series_has_every_bit_of_a_steady_launch(pda):
    """One steady launch of S T scenarios with each step's demands, tank heads, pump speeds and live emitters (``step_rows``)."""
    c = DR.series_case(pda)
    ser = run_series(c, False)
    assert ser["status"][..., 1].all()
    steps = run(DR.step_rows(c, ser["level"]))
    S, T = ser["status"].shape[:2]
    for k in steps:
        assert same_bits(steps[k].reshape((S, T) + steps[k].shape[1:]), ser[k]), k


# ---- 4. bits: one scenario per workgroup trip -------------------------------------------------------------------------------------------------
def test_scenarios_on_either_side_of_the_capped_grid_have_the_bits_of_launches_of_their_own():
    c, pairs = DR.cap_case()
    S = c["demand"].shape[0]
    whole = run(c)
    valves = c["net"].valve_links
    for s, t in pairs:                                      # the two scenarios of one workgroup: other regimes, both solved
        assert whole["status"][[s, t], 1].all() and not np.array_equal(whole["link_state"][s, valves], whole["link_state"][t, valves])
        assert not whole["emitter_flow"][t][c["coef"][t] == 0].any() and whole["emitter_flow"][t][c["coef"][s] == 0].any()
        none = (c["demand"][t] == 0) & ~c["net"].fixed
        assert none.any() and not whole["demand_delivered"][t][none].any() and not np.signbit(whole["demand_delivered"][t][none]).any()
    assert S == HR.ABOVE_CAP and not whole["status"][:, 2].any()
    for rows in (slice(0, 4), slice(S - 7, S)):
        sub = DR.rows(c["net"], *(c[k][rows] for k in ("demand", "roughness")), None, *(c[k][rows] for k in ("speed", "setting", "coef")),
                      c["pdd"])
        part = run(sub)
        for k in part:
            assert same_bits(part[k], whole[k][rows]), (rows, k)


# ---- 5. the budget ----------------------------------------------------------------------------------------------------------------------------
def test_the_largest_pressure_driven_series_the_budget_admits_and_one_node_more(capsys):
    c, ref = DR.budget_case(), DR.budget_reference()
    net, dense = c["net"], ref["dense"]
    raw = run_series(c, True)
    got = DR.solution(raw)
    cmp = DR.series_comparisons(c, ref, got)
    need = H.series_pdd_lds_bytes(net.num_nodes, net.num_pipes, net.half_bandwidth, 1, 0, 0, net.num_emitters)
    with capsys.disabled():
        print(f"dense_budget N = {net.num_nodes}, {need} of {H.LDS_BUDGET} bytes: iterations {got.iterations.tolist()} (reference "
              f"{dense.iterations.tolist()})  {DR.report(cmp)}")
    assert raw["status"][..., 1].all() and not raw["status"][..., 2:].any() and need <= H.LDS_BUDGET
    assert np.array_equal(got.iterations[ref["decisive"]], dense.iterations[ref["decisive"]])
    assert not DR.exceeded(cmp), DR.exceeded(cmp)
    assert ((got.emitter_flow != 0) == (c["coef"][:, None, :] > 0)).all() and not np.signbit(got.emitter_flow[got.emitter_flow == 0]).any()
    more = DR.budget_case(1)
    with pytest.raises(ValueError, match="bytes of LDS"):
        run_series(more, True)
    again = run_series(c, True)                             # nothing was launched, nothing is broken
    for k in raw:
        assert same_bits(raw[k], again[k]), k


# ---- 6. refusal -------------------------------------------------------------------------------------------------------------------------------
def test_a_duplicate_emitter_node_whose_pair_straddles_the_first_trip_fails_every_scenario():
    """hy_check_emitters scans the emitters before each one: the thread of emitter 270, on its second trip, must find emitter 10."""
    good = DR.steady_case(1)
    c = dict(good, net=DR._network(DR.KE))                  # (a network of its own: the test overwrites its uploaded array)
    net = c["net"]
    net._emitter_args(1, (1,), c["coef"][0])                # uploads the emitter array
    st = net.static()
    node = st["emitter_node"].clone()
    node[DR.HY_T + 14] = node[10]                           # an in-range junction, twice
    st["emitter_node"] = node
    got = run(c)
    assert (got["status"] == [0, 0, 1, 0]).all() and np.isnan(got["head"]).all() and np.isnan(got["flow"]).all()
    assert np.isnan(got["pressure"]).all() and np.isnan(got["emitter_flow"]).all() and not got["link_state"].any()
    again = run(good)                                       # the device is as it was
    assert again["status"][:, 1].all()
