"""THE CONTROLS on the device (gatres_hydraulic_series_controls, hydraulic_series_network_kernel<LV, true>) against the host
references of hydraulic_controls_refs.py: an empty table and a table that never fires give every bit of the pdd launch; CLOSED at
step 0 gives every bit of the closed bytes; a cold series that closes a link at step t0 is, from t0 on, every bit of a launch that
starts there; the operating case, the case with every kind and action and the 300-node case with a table of 275 controls agree
with ``simulate_series_ref`` (``hydraulic_controls_refs.misses``: the comparisons of hydraulic_dense_refs.py, and control_changes,
link_state, iterations, valve_changes and limited EQUAL); series on either side of the capped grid; every refusal; the LDS budget.
Every figure is printed before it is asserted."""
import gc

import numpy as np
import pytest
import torch

import hydraulic_controls_refs as CR
import hydraulic_dense_refs as DR

pytestmark = pytest.mark.gpu
H, G = CR.H, CR.G
same_bits = CR.same_bits
PDD_FIELDS = ("pressure", "head", "flow", "level", "status", "final_dq", "link_state", "valve_changes", "emitter_flow", "demand_delivered")
FIELDS = PDD_FIELDS + ("control_changes", "limited")
BADARG = "GATRES_E_BADARG"


@pytest.fixture(scope="module", autouse=True)
def own_memory_pool():
    """As in test_gpu_hydraulic_dense.py: this module's device memory goes back when the module ends, with the cached cases."""
    pool = torch.cuda.MemPool()
    routed = torch.cuda.use_mem_pool(pool)
    routed.__enter__()
    yield
    for cached in DR.CACHED + (CR.reference, CR.operating_case, CR.kinds_case, CR.dense_case):
        cached.cache_clear()
    gc.collect()
    torch.cuda.synchronize()
    routed.__exit__(None, None, None)


def host(result, fields):
    torch.cuda.synchronize()
    return {k: getattr(result, k).cpu().numpy() for k in fields}


def launch(c, warm, controls=True, fields=None, **over):
    """The case in one series launch; ``controls=False``: the pdd launch of the same series (demand-driven unless the case is not)."""
    kw = dict(CR.series_kw(c, controls), **over)
    if c["pdd"] is None and "controls" not in kw:
        kw["demand_model"] = "dda"
    res = c["net"].simulate_series(c["demand"], c["roughness"], c["mult"], step_seconds=c["dt"], warm_start=warm, **kw)
    return host(res, fields or (FIELDS if "controls" in kw else PDD_FIELDS))


def empty_table():
    return H.ControlTable([], [], [], [], [], [])


VARIANTS = [("operating", False), ("kinds", False), ("kinds", True), ("dense", False), ("dense", True)]


# ---- 1. a table that does nothing ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("warm", (True, False))
@pytest.mark.parametrize("name,pda", VARIANTS)
def test_an_empty_table_and_one_that_never_fires_give_every_bit_of_the_pdd_launch(name, pda, warm):
    """LV 1 (demand-driven) and LV 2 (pressure-driven), warm and cold, on the small cases and on the 300-node one."""
    c = CR.case(name, pda)
    net = c["net"]
    plain = launch(c, warm, controls=False)
    assert not plain["status"][..., 2].any()
    empty = launch(c, warm, controls=empty_table())
    never = H.control_table(net, [(int(c["controls"].link[0]), "closed", "at_step", CR.NEVER), (int(c["controls"].link[0]), "closed", "tank_above", 0, 1e9),
                                  (int(c["controls"].link[0]), "closed", "node_below", int(np.flatnonzero(~net.fixed)[0]), -1e9)])
    quiet = launch(c, warm, controls=never)
    for k in PDD_FIELDS:
        assert same_bits(plain[k], empty[k]), ("empty", k)
        assert same_bits(plain[k], quiet[k]), ("never", k)
    assert not empty["control_changes"].any() and not quiet["control_changes"].any()


# ---- 2. CLOSED at step 0 is the closed byte --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("warm", (True, False))
@pytest.mark.parametrize("pda", (False, True))
def test_closed_at_step_zero_on_a_pipe_a_pump_and_a_prv_gives_every_bit_of_the_closed_bytes(pda, warm):
    c = CR.case("kinds", pda)
    net, links = c["net"], (6, 0, 4)                        # pipe 3 -- 6, the pump, the PRV
    assert not net.is_pump[6] and not net.is_valve[6] and net.is_pump[0] and net.is_valve[4]
    table = H.control_table(net, [(p, "closed", "at_step", 0) for p in links])
    closed = c["closed"].copy()
    closed[:, links] = 1
    by_control = launch(c, warm, controls=table)
    by_byte = launch(c, warm, controls=False, link_closed=closed)
    for k in PDD_FIELDS:
        assert same_bits(by_control[k], by_byte[k]), k
    assert (by_control["link_state"][:, :, links] == 2).all()
    assert (by_control["control_changes"][:, 0] == 3).all() and not by_control["control_changes"][:, 1:].any()


# ---- 3. a switch in the middle of a cold series ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pda", (False, True))
def test_a_cold_series_that_closes_a_link_at_t0_is_from_there_on_a_launch_that_starts_there(pda):
    c = CR.case("kinds", pda)
    net, p, t0, T = c["net"], 6, 4, CR.KINDS_STEPS
    a = launch(c, False, controls=H.control_table(net, [(p, "closed", "at_step", t0)]))
    b = launch(c, False, controls=False)
    assert not a["status"][..., 2].any() and (a["link_state"][:, t0:, p] == 2).all() and (a["link_state"][:, :t0, p] != 2).all()
    for k in PDD_FIELDS:
        steps = t0 + 1 if k == "level" else t0
        assert same_bits(np.ascontiguousarray(a[k][:, :steps]), np.ascontiguousarray(b[k][:, :steps])), ("before", k)
    closed = c["closed"].copy()
    closed[:, p] = 1
    tail = dict(c, mult=np.ascontiguousarray(c["mult"][:, t0:]), smult=np.ascontiguousarray(c["smult"][:, t0:]),
                level0=np.ascontiguousarray(a["level"][:, t0]), closed=closed)
    rest = launch(tail, False, controls=False)
    for k in PDD_FIELDS:
        assert same_bits(np.ascontiguousarray(a[k][:, t0:]), rest[k]), ("after", k)
    assert T - t0 >= 2 and not np.array_equal(a["flow"][:, t0:], b["flow"][:, t0:])


# ---- 4. and 5. against the host reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("warm", (True, False))
@pytest.mark.parametrize("name,pda", VARIANTS)
def test_a_series_with_controls_against_the_reference(name, pda, warm, capsys):
    """``hydraulic_controls_refs.misses``: mass, energy, heads, flows, emitter flows, delivered demand, levels and the volume balance
    within the bounds of hydraulic_dense_refs.py; control_changes, link_state, iterations, valve_changes and limited EQUAL at every
    step (every case is DECISIVE and CLEAR).  ``dense``: controls on links below and above 256 in a table of 275."""
    c, ref = CR.case(name, pda), CR.reference(name, warm, pda)
    dense = ref["dense"]
    raw = launch(c, warm)
    got = CR.solution(raw)
    cmp = CR.series_comparisons(c, ref, got)
    with capsys.disabled():
        print(f"controls {name} pda={pda} warm={warm}: iterations {got.iterations.tolist()} (reference {dense.iterations.tolist()})  "
              f"control_changes {got.control_changes.tolist()}  clearance {CR.clearance(c, ref).tolist()}  {DR.report(cmp)}")
    assert raw["status"][..., 1].all() and not raw["status"][..., 2:].any()
    assert ref["decisive"].all() and (CR.clearance(c, ref) >= CR.CLEARANCE).all()
    assert np.array_equal(got.control_changes, dense.control_changes), (got.control_changes, dense.control_changes)
    assert CR.same_statuses(dense, got), (got.iterations, dense.iterations)
    assert not DR.exceeded(cmp), DR.exceeded(cmp)
    assert CR.misses(name, warm, pda, got) == []
    assert got.control_changes.any()
    if name == "operating":                                 # the pump is operated: never limited, switched off and on twice
        shut = (got.link_state[:, :, 0] == 2).astype(int)
        assert ((np.diff(shut, axis=1) == 1).sum(axis=1) >= 2).all() and ((np.diff(shut, axis=1) == -1).sum(axis=1) >= 2).all()
        free = launch(c, warm, controls=False, links=True)
        assert free["status"][..., 3].any(axis=1).all() and not raw["status"][..., 3].any()
    if name == "dense":
        hi, lo, pump, prv = c["links"]
        assert hi >= DR.HY_T > lo and len(c["controls"]) > DR.HY_T
        assert (got.link_state[:, 1:4, hi] == 2).all() and (got.link_state[:, 4:, hi] != 2).all() and (got.link_state[:, 2:, lo] == 2).all()


# ---- 6. the capped grid -----------------------------------------------------------------------------------------------------------------------
def test_series_on_either_side_of_the_capped_grid_have_the_bits_of_launches_of_their_own():
    """S = 1026 on the kinds network with T = 6.  Series 0 and 1 fire a CLOSED control at step 1 (a pressure condition with their own
    threshold); series 1024 and 1025, which the same workgroups run afterwards, fire nothing and must find no state left over."""
    base = CR.case("kinds", False)
    net, S, T = base["net"], H.GRID_CAP + 2, 6
    idx = np.arange(S) % 2
    scale = np.linspace(0.9, 1.1, S)[:, None]
    c = dict(base, demand=base["demand"][idx] * scale, roughness=base["roughness"][idx].copy(), closed=None,
             mult=np.ascontiguousarray(base["mult"][:, :T]), smult=np.ascontiguousarray(base["smult"][:, :T]),
             level0=np.full((S, 1), 3.0), speed=base["speed"][idx].copy(), setting=base["setting"][idx].copy(),
             coef=np.zeros((S, 0)), onset=np.zeros((S, 0), dtype=np.int64))
    node = 5
    table = H.control_table(net, [(6, "closed", "node_above", node, 0.0), (0, ("setting", 0.95), "node_above", node, 0.0)])
    thr = np.full((S, 2), 1e9)
    thr[:2] = 0.0
    whole = launch(c, True, controls=table, control_threshold=thr)
    assert not whole["status"][..., 2].any()
    assert (whole["control_changes"][:2, 1] == 2).all() and whole["control_changes"][:2].sum() == 4 and not whole["control_changes"][2:].any()
    assert (whole["link_state"][:2, 1:, 6] == 2).all() and not (whole["link_state"][2:, :, 6] == 2).any()
    for rows in (slice(0, 2), slice(S - 2, S), slice(500, 502), slice(H.GRID_CAP - 1, H.GRID_CAP + 1)):
        sub = dict(c, **{k: np.ascontiguousarray(c[k][rows]) for k in ("demand", "roughness", "level0", "speed", "setting", "coef", "onset")})
        part = launch(sub, True, controls=table, control_threshold=np.ascontiguousarray(thr[rows]))
        for k in FIELDS:
            assert same_bits(part[k], whole[k][rows]), (rows, k)
    quiet = launch(dict(c, **{k: np.ascontiguousarray(c[k][-2:]) for k in ("demand", "roughness", "level0", "speed", "setting", "coef", "onset")}),
                   True, controls=False)
    for k in PDD_FIELDS:                                    # and the two past the cap are the pdd launch's, as nothing fired
        assert same_bits(quiet[k], whole[k][-2:]), k


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------
def _check_net():
    """The kinds network with a check valve on pipe 1 -- 2."""
    c = CR.case("kinds", False)
    net = c["net"]
    check = np.zeros(net.num_pipes, dtype=bool)
    check[1] = True
    pairs = [tuple(p) for p in net.pipes]
    return H.HydraulicNetwork(CR.HR._edge_index(pairs), np.full(9, 200.0), np.full(9, 0.2), net.elevation, [0, 7], [5.0, 43.0], tank_nodes=[7],
                              tank_diameter=[10.0], tank_min_level=[0.0], tank_max_level=[8.0], pump_links=[0], pump_h0=[70.0],
                              pump_r=[3000.0], pump_n=[2.0], valve_links=[4], valve_kind=["PRV"], valve_setting=[25.0], check_valve=check)


REFUSED = {"a link outside the network": (9, 1, 0.0, 4, 0, 0.0), "a negative link": (-1, 1, 0.0, 4, 0, 0.0),
           "an unknown action": (6, 3, 0.0, 4, 0, 0.0), "an unknown kind": (6, 1, 0.0, 5, 0, 0.0),
           "a control on a CHECK pipe": (1, 1, 0.0, 4, 0, 0.0), "a setting on a pipe": (6, 2, 1.0, 4, 0, 0.0),
           "a setting that is not finite": (4, 2, np.nan, 4, 0, 0.0), "a negative setting on a pump": (0, 2, -0.5, 4, 0, 0.0),
           "a tank outside the network": (6, 1, 0.0, 1, 1, 1.0), "a node outside the network": (6, 1, 0.0, 2, 8, 1.0),
           "a fixed-head node": (6, 1, 0.0, 3, 7, 1.0), "a negative step": (6, 1, 0.0, 4, -1, 0.0)}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_a_table_that_control_table_refuses_fails_every_series_on_the_device(what):
    c = dict(CR.case("kinds", False), net=_check_net())
    row = REFUSED[what]
    good = (6, 1, 0.0, 4, CR.NEVER, 0.0)
    table = H.ControlTable(*zip(good, row, good))           # (unchecked: the arrays go to the entry point as they are)
    with pytest.raises(ValueError, match="control 1"):
        H.control_table(c["net"], table)
    got = launch(c, True, controls=table)
    assert (got["status"] == [0, 0, 1, 0]).all() and not got["link_state"].any() and not got["control_changes"].any()
    for k in ("head", "flow", "pressure", "final_dq", "demand_delivered"):
        assert np.isnan(got[k]).all(), k
    assert np.isnan(got["level"][:, 1:]).all()
    again = launch(c, True, controls=H.ControlTable(*zip(good, good)))      # the device is as it was
    assert not again["status"][..., 2].any()


def test_a_threshold_that_is_not_finite_fails_its_series_alone():
    c = CR.case("kinds", False)
    thr = CR.thresholds(c).copy()
    thr[1, 1] = np.inf
    got, right = launch(c, True, control_threshold=thr), launch(c, True)
    assert (got["status"][1] == [0, 0, 1, 0]).all() and np.isnan(got["head"][1]).all() and not got["control_changes"][1].any()
    for k in FIELDS:
        assert same_bits(got[k][0], right[k][0]), k
    thr[1, 1], thr[1, 0] = CR.thresholds(c)[1, 1], np.nan   # an AT_STEP control's threshold is not read
    assert c["controls"].kind[0] == H.CONTROL_KINDS["at_step"]
    got = launch(c, True, control_threshold=thr)
    for k in FIELDS:
        assert same_bits(got[k], right[k]), k


def test_a_null_argument_or_an_overlapping_output_is_refused_before_any_launch(monkeypatch):
    """The entry point through ctypes with the arguments of a good call, one of them replaced."""
    c = CR.case("kinds", False)
    lib = G._native.load()
    real = lib.gatres_hydraulic_series_controls
    names = ("control_link", "control_action", "control_value", "control_kind", "control_target", "control_threshold")
    seen = {}

    def probe(*args):
        args = list(args)
        first = len(args) - 10                              # the table, its stride and count, control_changes, the stream
        changes, valve_changes = first + 8, first - 14      # (valve_changes: before the 8 emitter and the 5 demand-model arguments)
        for i, name in enumerate(names):
            seen[name] = real(*(args[:first + i] + [None] + args[first + i + 1:]))
        seen["control_changes"] = real(*(args[:changes] + [None] + args[changes + 1:]))
        seen["num_controls < 0"] = real(*(args[:first + 7] + [-1] + args[first + 8:]))
        seen["a stride that is not Kc"] = real(*(args[:first + 6] + [3] + args[first + 7:]))
        seen["control_changes on valve_changes"] = real(*(args[:changes] + [args[valve_changes]] + args[changes + 1:]))
        seen["control_changes on the table"] = real(*(args[:changes] + [args[first + 4]] + args[changes + 1:]))
        seen["no table at all"] = real(*(args[:first] + [None] * 6 + [0, 0] + args[first + 8:]))
        return real(*args)

    monkeypatch.setattr(lib, "gatres_hydraulic_series_controls", probe, raising=False)
    got = launch(c, True)
    monkeypatch.undo()
    assert got["status"][..., 1].all()
    allowed = seen.pop("no table at all")
    assert allowed == 0 and len(seen) == 11 and all(rc == -1 for rc in seen.values()), (allowed, seen)
    assert G._native.ERRORS[-1].startswith(BADARG)


# ---- 8. the LDS budget ----------------------------------------------------------------------------------------------------------------------
def _budget_nodes():
    need = lambda n: H.series_controls_lds_bytes(n, n - 1, n - 1, 1, 0, 0, n - 2)
    n = 3
    while need(n + 1) <= H.LDS_BUDGET:
        n += 1
    return n


def _budget_case(N):
    c = DR._budget_case(N)
    net, S, T = c["net"], DR.BUDGET_SERIES, DR.BUDGET_STEPS
    table = H.control_table(net, [(N // 2, "closed", "at_step", CR.NEVER), (N // 2, "open", "at_step", 1), (3, "open", "tank_above", 0, 0.5)])
    return dict(c, speed=np.ones((S, 0)), smult=np.ones((1, T)), spat=np.zeros(0, dtype=np.int64), setting=np.zeros((S, 0)), closed=None,
                controls=table)


def test_the_largest_path_the_controls_launch_admits_and_one_node_more(capsys, monkeypatch):
    N = _budget_nodes()
    c = _budget_case(N)
    net = c["net"]
    need = H.series_controls_lds_bytes(N, N - 1, N - 1, 1, 0, 0, N - 2)
    assert need <= H.LDS_BUDGET < H.series_controls_lds_bytes(N + 1, N, N, 1, 0, 0, N - 1) and N < DR.budget_nodes() + 1
    ref = CR._reference(c, True, all_decisive=False)
    raw = launch(c, True)
    got = CR.solution(raw)
    cmp = CR.series_comparisons(c, ref, got)
    with capsys.disabled():
        print(f"controls budget N = {N}, {need} of {H.LDS_BUDGET} bytes: iterations {got.iterations.tolist()} (reference "
              f"{ref['dense'].iterations.tolist()})  control_changes {got.control_changes.tolist()}  {DR.report(cmp)}")
    assert raw["status"][..., 1].all() and not raw["status"][..., 2].any()
    assert np.array_equal(got.iterations[ref["decisive"]], ref["dense"].iterations[ref["decisive"]])
    assert np.array_equal(got.control_changes, ref["dense"].control_changes) and got.control_changes.any()
    assert not DR.exceeded(cmp), DR.exceeded(cmp)
    more = _budget_case(N + 1)
    with pytest.raises(ValueError, match="bytes of LDS"):
        launch(more, True)
    monkeypatch.setattr(H, "LDS_BUDGET", 1 << 30)           # past the Python check, the entry point refuses the same launch
    with pytest.raises(RuntimeError, match=BADARG):
        launch(more, True)
    monkeypatch.undo()
    again = launch(c, True)                                 # nothing was launched, nothing is broken
    for k in raw:
        assert same_bits(raw[k], again[k]), k
