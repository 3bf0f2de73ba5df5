"""THE CONTROLS on the host (hydraulics.py: ``control_table``, ``control_step_ref``, ``simulate_series_ref(controls=)``): the pass as a
plain loop, every refusal, the identities of the series reference, the operating case, the DECISIVE, CLEAR and ROBUST conditions of
every case the GPU test uses (hydraulic_controls_refs.py), the planted wrong answers held to the very comparisons of the GPU test,
and the new entry point's place in gatres.h, in the library and in ``_native``.  No GPU."""
import os
import re

import numpy as np
import pytest

import hydraulic_controls_refs as CR
import hydraulic_dense_refs as DR

H, G = CR.H, CR.G
same_bits = CR.same_bits
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = [("operating", False), ("kinds", False), ("kinds", True), ("dense", False), ("dense", True)]


# ---- control_step_ref ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net():
    return CR.case("kinds")["net"]


def step(net, rows, state=None, level=(3.0,), pressure=None, t=1):
    table = H.control_table(net, rows)
    pressure = np.full(net.num_nodes, 30.0) if pressure is None else pressure
    return H.control_step_ref(table, table.threshold, H.control_state(net.num_pipes) if state is None else state, np.asarray(level), pressure, t)


def test_the_later_control_wins(net):
    st, n = step(net, [(6, "closed", "at_step", 1), (6, "open", "at_step", 1)])
    assert st["ctl"][6] == H.CTL_OPEN and n == 2 and st["changed"][6]
    st, n = step(net, [(6, "open", "at_step", 1), (6, "closed", "at_step", 1)])
    assert st["ctl"][6] == H.CTL_CLOSED and n == 2


def test_controls_are_level_triggered_and_the_state_persists(net):
    rows = [(6, "closed", "tank_above", 0, 2.5)]
    st, total = H.control_state(net.num_pipes), []
    for t in range(5):                                      # true for five steps: one change
        st, n = step(net, rows, st, level=(3.0,), t=t)
        total.append(n)
        assert st["ctl"][6] == H.CTL_CLOSED and st["changed"][6] == (t == 0)
    assert total == [1, 0, 0, 0, 0]
    st, n = step(net, rows, st, level=(2.0,), t=5)          # the condition turns false: the state stays
    assert st["ctl"][6] == H.CTL_CLOSED and n == 0 and not st["changed"].any()
    st, n = step(net, [(6, "closed", "tank_below", 0, 2.0)], level=(2.0,), t=0)     # <= and >= include the threshold, at t = 0 too
    assert st["ctl"][6] == H.CTL_CLOSED and n == 1


def test_a_setting_opens_the_link_and_its_bits_count(net):
    st, n = step(net, [(0, "closed", "at_step", 1), (0, ("setting", 0.8), "at_step", 1)])
    assert st["ctl"][0] == H.CTL_OPEN and st["has_value"][0] and st["value"][0] == 0.8 and n == 2
    again, n = step(net, [(0, ("setting", 0.8), "at_step", 1)], st)
    assert n == 0
    moved, n = step(net, [(0, ("setting", np.nextafter(0.8, 1.0)), "at_step", 1)], st)
    assert n == 1 and moved["value"][0] != 0.8
    opened, n = step(net, [(0, "open", "at_step", 1)], st)   # OPEN keeps the override
    assert n == 0 and opened["has_value"][0] and opened["value"][0] == 0.8


def test_node_conditions_are_skipped_at_step_zero_and_a_late_step_never_fires(net):
    rows = [(6, "closed", "node_below", 5, 40.0), (8, "closed", "node_above", 5, 20.0), (2, "closed", "at_step", 7)]
    st, n = step(net, rows, t=0)
    assert n == 0 and not st["ctl"].any()
    st, n = step(net, rows, t=1)
    assert n == 2 and st["ctl"][[6, 8, 2]].tolist() == [H.CTL_CLOSED, H.CTL_CLOSED, H.CTL_NONE]
    for t in range(7):                                      # T = 7: a target of T or more never fires
        assert step(net, [(2, "closed", "at_step", 7), (2, "closed", "at_step", CR.NEVER)], t=t)[1] == 0


def test_open_overrides_a_static_closed_flag_and_a_closed_byte():
    c = CR.case("kinds")
    net, S = c["net"], 2
    shut = np.zeros(net.num_pipes, dtype=bool)
    shut[6] = True
    flagged = H.HydraulicNetwork(CR.HR._edge_index([tuple(p) for p in net.pipes]), net.length, net.diameter, net.elevation, [0, 7], [5.0, 43.0],
                                 tank_nodes=[7], tank_diameter=[10.0], tank_min_level=[0.0], tank_max_level=[8.0], pump_links=[0],
                                 pump_h0=[70.0], pump_r=[3000.0], pump_n=[2.0], valve_links=[4], valve_kind=["PRV"], valve_setting=[25.0],
                                 closed=shut)
    table = H.control_table(flagged, [(6, "open", "at_step", 2), (2, "open", "at_step", 2)])
    r = H.simulate_series_ref(flagged, c["demand"], c["roughness"], c["mult"][:, :4], c["dt"], pattern_of_node=c["pattern"],
                              initial_level=c["level0"], link_closed=c["closed"], controls=table)
    assert not r.failed.any()
    assert r.link_state[:, :, 6].tolist() == [[2, 2, 0, 0]] * S                     # the static flag
    assert r.link_state[1, :, 2].tolist() == [2, 2, 0, 0] and not (r.link_state[0, :, 2] == 2).any()       # the byte of series 1
    assert r.control_changes.tolist() == [[0, 0, 2, 0]] * S


# ---- control_table: every refusal names its offender ------------------------------------------------------------------------------------------
def _check_net(net):
    check = np.zeros(net.num_pipes, dtype=bool)
    check[1] = True
    return H.HydraulicNetwork(CR.HR._edge_index([tuple(p) for p in net.pipes]), net.length, net.diameter, net.elevation, [0, 7], [5.0, 43.0],
                              tank_nodes=[7], tank_diameter=[10.0], pump_links=[0], pump_h0=[70.0], pump_r=[3000.0], pump_n=[2.0],
                              valve_links=[4], valve_kind=["PRV"], valve_setting=[25.0], check_valve=check)


REFUSED = [((9, "closed", "at_step", 1), "link 9 is outside"), ((-1, "closed", "at_step", 1), "link -1 is outside"),
           ((6, "shut", "at_step", 1), "unknown action 'shut'"), ((6, "closed", "when", 1), "unknown kind 'when'"),
           ((1, "closed", "at_step", 1), "link 1 is a CHECK pipe"), ((6, ("setting", 1.0), "at_step", 1), "link 6 is neither a pump nor"),
           ((4, ("setting", np.inf), "at_step", 1), "setting inf of link 4"), ((0, ("setting", -0.1), "at_step", 1), "setting -0.1 of link 0"),
           ((6, "closed", "tank_above", 1, 2.0), "tank 1 is outside"), ((6, "closed", "tank_below", -1, 2.0), "target -1 is negative"),
           ((6, "closed", "node_above", 8, 2.0), "node 8 is outside"), ((6, "closed", "node_below", 7, 2.0), "node 7 is a fixed-head node"),
           ((6, "closed", "node_below", 0, 2.0), "node 0 is a fixed-head node"), ((6, "closed", "at_step", -1), "target -1 is negative"),
           ((6, "closed", "tank_above", 0), "needs a threshold"), ((6, "closed", "at_time", 450.0), "no whole number of steps")]


@pytest.mark.parametrize("row,what", REFUSED)
def test_control_table_refuses_by_name(net, row, what):
    good = (6, "closed", "at_step", 3)
    with pytest.raises(ValueError, match="control 1: .*" + re.escape(what)):
        H.control_table(_check_net(net), [good, row, good], step_seconds=300.0)


def test_control_table_takes_the_forms_the_issue_names(net):
    t = H.control_table(net, [(6, "closed", "tank_above", 0, 4.5), (0, ("setting", 0.8), "at_step", 12), (8, "open", "node_below", 5, 20.0),
                              (4, ("setting", -3.0), "at_time", 900.0)], step_seconds=300.0)
    assert len(t) == 4 and t.link.dtype == np.int32 and t.action.dtype == np.uint8 and t.kind.dtype == np.uint8 and t.target.dtype == np.int32
    assert t.action.tolist() == [1, 2, 0, 2] and t.kind.tolist() == [1, 4, 2, 4] and t.target.tolist() == [0, 12, 5, 3]
    assert t.value.tolist() == [0.0, 0.8, 0.0, -3.0] and t.threshold.tolist() == [4.5, 0.0, 20.0, 0.0]
    assert H.ControlTable.ACTIONS == {"open": 0, "closed": 1, "setting": 2} and H.ControlTable.KINDS["at_step"] == 4
    assert len(H.control_table(net, [])) == 0 and len(H.control_table(net, t)) == 4


# ---- the identities of simulate_series_ref ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("warm", (True, False))
@pytest.mark.parametrize("pda", (False, True))
def test_an_empty_table_is_no_table_and_closed_at_step_zero_is_the_closed_byte(pda, warm):
    c = CR.case("kinds", pda)
    model = {} if pda else {"demand_model": "dda"}
    plain = CR.simulate_ref(c, "banded", warm, controls=False, **model)
    empty = CR.simulate_ref(c, "banded", warm, controls=H.ControlTable([], [], [], [], [], []))
    for k in plain._fields:
        assert same_bits(getattr(plain, k), getattr(empty, k)), k
    assert not empty.control_changes.any()
    links = (6, 0, 4)
    closed = c["closed"].copy()
    closed[:, links] = 1
    by_byte = CR.simulate_ref(dict(c, closed=closed), "banded", warm, controls=False, **model)
    by_control = CR.simulate_ref(c, "banded", warm, controls=H.control_table(c["net"], [(p, "closed", "at_step", 0) for p in links]))
    for k in by_byte._fields:
        assert same_bits(getattr(by_byte, k), getattr(by_control, k)), k
    assert (by_control.link_state[:, :, links] == 2).all() and by_control.control_changes[:, 0].tolist() == [3, 3]


def test_a_threshold_that_is_not_finite_fails_its_series_from_step_zero():
    c = CR.case("kinds")
    thr = CR.thresholds(c).copy()
    thr[1, 2] = np.nan
    r, right = CR.simulate_ref(c, "banded", control_threshold=thr), CR.simulate_ref(c, "banded")
    assert r.failed[1].all() and np.isnan(r.head[1]).all() and not r.control_changes[1].any()
    assert same_bits(r.head[0], right.head[0]) and same_bits(r.control_changes[0], right.control_changes[0])
    with pytest.raises(ValueError, match="control_threshold needs controls"):
        CR.simulate_ref(c, "banded", controls=False, control_threshold=thr)


# ---- the operating case -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("warm", (True, False))
def test_the_operating_case_stays_unlimited_with_controls_and_is_limited_without(warm, capsys):
    c, ref = CR.case("operating"), CR.reference("operating", warm)
    net, dt, dense = c["net"], c["dt"], ref["dense"]
    free = CR.simulate_ref(c, "dense", warm, controls=False)
    assert free.limited.any(axis=1).all()                   # the condition on the case
    assert dense.converged.all() and not dense.failed.any() and not dense.limited.any()
    shut = (dense.link_state[:, :, 0] == 2).astype(int)
    off, on = (np.diff(shut, axis=1) == 1).sum(axis=1), (np.diff(shut, axis=1) == -1).sum(axis=1)
    inflow = np.abs(np.diff(dense.level[:, :, 0], axis=1)).max(axis=1)              # max |inflow| dt / A, from the run itself
    lo, hi = np.array(CR.OP_BAND).T
    with capsys.disabled():
        print(f"operating warm={warm}: levels {dense.level[:, :, 0].min(axis=1)} .. {dense.level[:, :, 0].max(axis=1)}, bands {CR.OP_BAND}, "
              f"d {inflow}, off {off} on {on}")
    assert (off >= 2).all() and (on >= 2).all()
    assert (dense.level[:, :, 0] >= (lo - inflow)[:, None]).all() and (dense.level[:, :, 0] <= (hi + inflow)[:, None]).all()
    assert (hi + inflow < net.tank_max_level[0]).all() and (lo - inflow > net.tank_min_level[0]).all()


# ---- DECISIVE, CLEAR, ROBUST ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("warm", (True, False))
@pytest.mark.parametrize("name,pda", VARIANTS)
def test_every_case_is_decisive_clear_and_robust(name, pda, warm, capsys):
    c, ref = CR.case(name, pda), CR.reference(name, warm, pda)              # (asserts convergence, no clamp, DECISIVE)
    clear = CR.clearance(c, ref)
    with capsys.disabled():
        print(f"controls {name} pda={pda} warm={warm}: clearance {clear.tolist()}  control_changes {ref['dense'].control_changes.tolist()}")
    assert ref["decisive"].all() and (clear >= CR.CLEARANCE).all()
    assert ref["dense"].control_changes.any()
    for moved, cmp, same in CR.moved_answers(name, warm, pda):
        assert same and not DR.exceeded(cmp), (moved, DR.exceeded(cmp), DR.report(cmp))


def test_the_kinds_case_has_every_kind_and_action_and_the_dense_table_turns_its_loops_over():
    c = CR.case("kinds")
    t = c["controls"]
    assert set(t.kind.tolist()) == {0, 1, 2, 3, 4} and set(t.action.tolist()) == {0, 1, 2}
    assert c["net"].is_pump[t.link[t.action == 2]].any() and c["net"].is_valve[t.link[t.action == 2]].any()
    dense = CR.reference("kinds")["dense"]
    assert (dense.link_state[:, 1, 0] == 0).all() and (dense.link_state[:, :, 0] == 2).any()       # the pump runs on its setting, then stops
    assert all((dense.link_state[:, :, 4] == v).any() for v in (2, 3, 4)) and (dense.link_state[:, :, 8] == 2).any()
    d = CR.case("dense")
    hi, lo, pump, prv = d["links"]
    first, last = d["live"]
    assert len(d["controls"]) > DR.HY_T and first > 0 and last < len(d["controls"]) and hi >= DR.HY_T > lo
    assert (d["controls"].link[:first] == hi).any() and (d["controls"].link[last:] == hi).any()


# ---- planted wrong answers ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", CR.WRONG)
def test_a_planted_wrong_answer_misses_the_comparisons_of_the_gpu_test(kind, capsys):
    sol = CR.wrong_answer(kind, "kinds", True, False)
    missed = CR.misses("kinds", True, False, sol)
    with capsys.disabled():
        print(f"{kind}: misses {missed}")
    assert missed
    right = CR.solution(CR.simulate_ref(CR.case("kinds"), "banded", True))
    assert CR.misses("kinds", True, False, right) == []


# ---- the entry point and the LDS sum -----------------------------------------------------------------------------------------------------------
def test_the_lds_sum_and_the_entry_point():
    for args in ((300, 330, 40, 2, 2, 3, 280), (8, 9, 3, 1, 1, 1, 0), (133, 132, 132, 1, 0, 0, 131)):
        for model in (0, 1):
            assert H.series_controls_lds_bytes(*args, model) == H.series_pdd_lds_bytes(*args, model) + 12 * args[1] + 16
    name, count = "gatres_hydraulic_series_controls", 73 + 9
    header = open(os.path.join(ROOT, "include", "gatres.h")).read()
    m = re.search(r"\bint " + name + r"\(([^;]*?)\);", header, re.S)
    assert m and m.group(1).count(",") + 1 == count and "THE CONTROLS" in header and "12 P + 16" in header
    assert len(G._native.SIGNATURES[name][1]) == count
    sources = {f: open(os.path.join(G._build.CSRC, f)).read() for f in os.listdir(G._build.CSRC) if f.endswith((".hip", ".h"))}
    assert sum(len(re.findall(r'extern "C" int ' + name + r"\(", text)) for text in sources.values()) == 1
    assert "return 12 * P + 16;" in sources["k_hydraulic_network.hip"]
    assert len(getattr(G._native.load(), name).argtypes) == count
    assert "#define GATRES_ABI_VERSION 9" in header and G._native.ABI_VERSION == 9
    for word, value in (("OPEN", 0), ("CLOSED", 1), ("SETTING", 2), ("TANK_BELOW", 0), ("TANK_ABOVE", 1), ("NODE_BELOW", 2), ("NODE_ABOVE", 3),
                        ("AT_STEP", 4)):
        assert f"#define GATRES_HYD_CTL_{word} {value}\n" in header
