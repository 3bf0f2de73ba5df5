"""The cases of THE CONTROLS (gatres.h; hydraulics.py: ``control_table``, ``simulate_series(controls=)``), shared by
test_hydraulic_controls_host.py and test_gpu_hydraulic_controls.py: ``operating`` (reservoir -> pump -> junctions -> tank, the pump
switched by the tank's level), ``kinds`` (a looped network with a pump, a PRV, a tank, all five kinds of condition and all three
actions, a speed setting on the pump and a setting change on the PRV) and ``dense`` (the 300-node, 330-link, two-tank series of
hydraulic_dense_refs.py with a table of 275 controls, most of them fillers that never fire, on links below and above 256).  Each
case and its host reference (``simulate_series_ref`` dense and banded) is built once and never changed.

The comparisons are those of hydraulic_dense_refs.py, as they are (``series_comparisons``, ``same_statuses``): a step of a series
with controls is the steady scenario of ``step_rows`` with the pump speeds, valve settings and closed bytes that the control state
of the step gives, which is all that ``controlled_rows`` adds.  No new tolerance.

Every case is DECISIVE and CLEAR: besides the DECISIVE condition of hydraulic_dense_refs.py, every level and pressure condition that
the reference evaluates is at least CLEARANCE (1000) times further from its threshold than the difference the level and head
comparisons would still accept (``clearance``), so a device result inside those bounds fires the same controls at the same steps.
ROBUST (``moved_answers``) as in hydraulic_dense_refs.py: the reference with every roughness moved by one ulp fires the same
controls and takes the same iterations.  The layouts and seeds were searched on the CPU until all of that holds."""
import contextlib
import functools
import types

import numpy as np

import hydraulic_dense_refs as DR
import hydraulic_series_refs as SR
import hydraulics_refs as HR

H, G = HR.H, HR.G
same_bits = SR.same_bits
CLEARANCE = 1000.0
NEVER = 1 << 30                         # an AT_STEP target no series reaches
FIELDS = ("head", "flow", "link_state", "iterations", "valve_changes", "emitter_flow", "demand_delivered", "level", "control_changes",
          "limited")


# ---- the keywords and rows of a case ------------------------------------------------------------------------------------------------
def series_kw(c, controls=True):
    """The keywords that ``simulate_series`` and ``simulate_series_ref`` share; ``controls=False``: the same series without its
    table; a ``ControlTable``: with that one in place of the case's (and with its own thresholds)."""
    kw = DR.series_kw(c)
    if c.get("closed") is not None:
        kw["link_closed"] = c["closed"]
    if controls is True:
        kw["controls"] = c["controls"]
        if c.get("threshold") is not None:
            kw["control_threshold"] = c["threshold"]
    elif controls is not False:
        kw["controls"] = controls
    return kw


def thresholds(c):
    """[S, Kc]: the case's own thresholds per series, or the table's for every series."""
    S = c["demand"].shape[0]
    return np.broadcast_to(c["controls"].threshold if c.get("threshold") is None else c["threshold"], (S, len(c["controls"])))


def simulate_ref(c, solver="dense", warm=True, controls=True, **kw):
    return H.simulate_series_ref(c["net"], c["demand"], c["roughness"], c["mult"], c["dt"], solver=solver, warm_start=warm,
                                 **dict(series_kw(c, controls), **kw))


def solution(src):
    return DR.solution(src, FIELDS)


def flat(sol):
    """``hydraulic_dense_refs.flat`` (a series solution [S, T, ...] as rows [S T, ...]) that also takes a network without emitters."""
    f = lambda v: None if v is None else v.reshape((v.shape[0] * v.shape[1],) + v.shape[2:])
    return types.SimpleNamespace(head=f(sol.head), flow=f(sol.flow), link_state=f(sol.link_state), iterations=f(sol.iterations),
                                 valve_changes=f(sol.valve_changes), emitter_flow=f(sol.emitter_flow),
                                 demand_delivered=f(sol.demand_delivered), level=None)


def replay(c, sol):
    """The control state that every step of a solution starts with, from its OWN levels and heads: a list [S][T] of states, and
    control_changes [S, T]."""
    net, S, T = c["net"], c["demand"].shape[0], c["mult"].shape[1]
    table = c["controls"]
    states, changes = [], np.zeros((S, T), dtype=np.int32)
    for s in range(S):
        st, row = H.control_state(net.num_pipes), []
        for t in range(T):
            prev = None if t == 0 else sol.head[s, t - 1] - net.elevation
            st, changes[s, t] = H.control_step_ref(table, thresholds(c)[s], st, sol.level[s, t], prev, t)
            row.append(st)
        states.append(row)
    return states, changes


def controlled_rows(c, sol):
    """``hydraulic_dense_refs.step_rows`` of a series with controls: the steps as rows of a steady launch, with the speed, the setting
    and the closed byte that the control state of the step gives each pump, valve and link."""
    net, S, T = c["net"], c["demand"].shape[0], c["mult"].shape[1]
    rows = DR.step_rows(c, sol.level)
    states, _ = replay(c, sol)
    closed0 = np.zeros((S, net.num_pipes), dtype=np.uint8) if c.get("closed") is None else np.broadcast_to(c["closed"], (S, net.num_pipes))
    speed, setting = rows["speed"].copy(), rows["setting"].copy()
    closed = np.zeros((S * T, net.num_pipes), dtype=np.uint8)
    for s in range(S):
        for t in range(T):
            st, i = states[s][t], s * T + t
            pl, vl = net.pump_links, net.valve_links
            speed[i] = np.where(st["has_value"][pl], st["value"][pl], c["speed"][s]) * c["smult"][c["spat"], t]
            setting[i] = np.where(st["has_value"][vl], st["value"][vl], c["setting"][s])
            closed[i] = np.where(st["ctl"] == H.CTL_NONE, closed0[s], st["ctl"] == H.CTL_CLOSED)
            assert not (net.closed & (st["ctl"] == H.CTL_OPEN)).any(), "open a link through its byte, not its static flag, in a case"
    return dict(rows, speed=speed, setting=setting, closed=closed)


@contextlib.contextmanager
def closed_rows():
    """hydraulic_dense_refs.model_kw hands a row's closed bytes on as well, while its comparisons run on controlled rows."""
    right = DR.model_kw
    DR.model_kw = lambda c: dict(right(c), **({} if c.get("closed") is None else {"link_closed": c["closed"]}))
    try:
        yield
    finally:
        DR.model_kw = right


def series_comparisons(c, ref, got):
    """``hydraulic_dense_refs.series_comparisons`` as it is, on controlled rows."""
    with closed_rows():
        out = DR.comparisons(ref["steps"], ref, flat(DR.solution(ref["dense"])), flat(got), controlled_rows(c, got))
        out.update(DR.levels_and_balance(c, ref["dense"], ref["banded"], got))
    return out


def same_statuses(dense, got):
    """``hydraulic_dense_refs.same_statuses``, and control_changes and limited EQUAL too."""
    return DR.same_statuses(flat(solution(dense)), flat(got)) and np.array_equal(got.control_changes, dense.control_changes) and \
        np.array_equal(np.asarray(got.limited) != 0, dense.limited)


# ---- CLEAR: the conditions the reference evaluates, and how far each is from its threshold ----------------------------------------
def clearance(c, ref):
    """Per series [S] the smallest ratio, over every level and pressure condition that the dense and the banded reference evaluate
    at any step, of |value - threshold| to the difference that the comparisons accept for that value: ``levels_and_balance``'s
    level bound for a tank, the head bound of ``comparisons`` times the step's head span for a junction."""
    net, table = c["net"], c["controls"]
    S, T = c["demand"].shape[0], c["mult"].shape[1]
    dense, banded = ref["dense"], ref["banded"]
    l_accept = DR.levels_and_balance(c, dense, banded, dense)["level"][1]                         # [K]
    h_accept = (HR.bound(ref["dh"].max(), ref["floors"]["dh"], HR.AGREEMENT_FACTOR) * ref["span"]).reshape(S, T)
    worst = np.full(S, np.inf)
    for r in (dense, banded):
        for k in range(len(table)):
            kind, target, thr = int(table.kind[k]), int(table.target[k]), thresholds(c)[:, k, None]
            if kind <= 1:
                worst = np.minimum(worst, (np.abs(r.level[:, :T, target] - thr) / l_accept[target]).min(axis=1))
            elif kind <= 3 and T > 1:
                pr = r.head[:, :-1, target] - net.elevation[target]
                worst = np.minimum(worst, (np.abs(pr - thr) / h_accept[:, :-1]).min(axis=1))
    return worst


def _reference(c, warm, all_decisive=True):
    dense, banded = simulate_ref(c, "dense", warm), simulate_ref(c, "banded", warm)
    for r in (dense, banded):
        assert r.converged.all() and not r.failed.any() and not r.limited.any(), (warm, r.iterations, r.converged, r.limited)
    assert np.array_equal(dense.link_state, banded.link_state) and np.array_equal(dense.control_changes, banded.control_changes), warm
    decisive = DR._decisive(dense, banded, lambda **kw: simulate_ref(c, "dense", warm, **kw))
    assert decisive.all() or not all_decisive, (warm, decisive, dense.iterations, banded.iterations)
    with closed_rows():
        steps = controlled_rows(c, dense)
        ref = dict(DR.rows_reference(steps, flat(DR.solution(dense)), flat(DR.solution(banded)), controlled_rows(c, banded)),
                   dense=dense, banded=banded, decisive=decisive, steps=steps)
    assert np.array_equal(replay(c, dense)[1], dense.control_changes)
    DR._freeze(dense, banded)
    return ref


# ---- operating: reservoir -> pump -> junctions -> tank ----------------------------------------------------------------------------------
OP_STEPS, OP_DT = 14, 600.0
OP_BAND = ((2.0, 2.85), (1.9, 2.7))      # (lo, hi) of the tank's level per series: searched, see the module's header
OP_SEED, OP_DEMAND = 5, (0.006, 0.010)              # searched: see the module's header


def _full(net, S, T, **kw):
    """The keys of a ``hydraulic_dense_refs`` series case that a network may lack, filled with what changes nothing."""
    c = {"net": net, "speed": np.ones((S, net.num_pumps)), "smult": np.ones((1, T)), "spat": np.zeros(net.num_pumps, dtype=np.int64),
         "setting": np.tile(net.valve_setting, (S, 1)), "coef": np.zeros((S, net.num_emitters)),
         "onset": np.zeros((S, net.num_emitters), dtype=np.int64), "pdd": None, "closed": None}
    c.update(kw)
    return c


@functools.lru_cache(maxsize=None)
def operating_case():
    """Node 0 a reservoir below the network, link 0 the pump, three junctions that draw on a daily pattern, node 4 the tank.  With
    the pump on the tank gains up to 0.7 m a step and without it loses 0.2 .. 0.4 m, so without controls it is full after a few
    steps and clamped; with the pump CLOSED above the series' hi and OPEN below its lo (OP_BAND, as ``control_threshold`` [S, Kc]) it stays between its limits."""
    pairs = [(0, 1), (1, 2), (2, 3), (3, 4)]
    net = H.HydraulicNetwork(HR._edge_index(pairs), [10.0, 300.0, 250.0, 200.0], [0.3, 0.25, 0.25, 0.25], [0.0, 0.0, 5.0, 8.0, 30.0],
                             [0, 4], [5.0, 32.0], tank_nodes=[4], tank_diameter=[8.0], tank_min_level=[0.0], tank_max_level=[6.0],
                             pump_links=[0], pump_h0=[60.0], pump_r=[4000.0], pump_n=[2.0])
    S, T = 2, OP_STEPS
    rng = np.random.RandomState(OP_SEED)
    demand = np.zeros((S, 5))
    demand[:, 1:4] = rng.uniform(OP_DEMAND[0], OP_DEMAND[1], (S, 3))
    mult = 1.0 + 0.3 * np.sin(np.arange(T) * 2 * np.pi / 12)[None, :]
    controls = H.control_table(net, [(0, "closed", "tank_above", 0, OP_BAND[0][1]), (0, "open", "tank_below", 0, OP_BAND[0][0])])
    threshold = np.array([[hi, lo] for lo, hi in OP_BAND])
    return _full(net, S, T, demand=demand, roughness=rng.uniform(90.0, 130.0, (S, 4)), mult=mult, pattern=np.zeros(5, dtype=np.int64),
                 dt=OP_DT, level0=np.array([[2.6], [3.1]]), controls=controls, threshold=threshold)


# ---- kinds: every kind of condition and every action -----------------------------------------------------------------------------------
KINDS_PDD = (5.0, 30.0, 1.0)
KINDS_STEPS = 10
KINDS_SEED, KINDS_ROUGHNESS_SEED = 11, 2
# (lo, hi) of the tank's level per series, demand-driven and pressure-driven: searched, see the module's header
KINDS_BAND = {False: ((3.46, 4.21), (3.3, 3.85)), True: ((3.3, 3.97), (3.38, 4.01))}


@functools.lru_cache(maxsize=None)
def kinds_case(pda):
    """Reservoir 0 -- pump (link 0) -- 1 -- 2 -- 3 -- tank 7; 2 -- PRV -- 4 -- 5 -- 6; 3 -- 6 and 1 -- 6 close the loops, so that no
    control cuts a junction off.  Links in the order of ``pairs``.  The pump gets a speed setting at step 1 and is switched by the
    tank's level; the PRV gets a new setting by the pressure at node 5, is CLOSED at step 5 and OPEN again at step 7; pipe 5 -- 6 is
    CLOSED when node 5 has pressure to spare (after step 0 only) and OPEN from step 4 on, before the PRV closes, so that nodes 4 and
    5 are never cut off; pipe 1 -- 6 starts closed by its byte in series 1; at step 3 one
    control closes it and the next one opens it, so it is OPEN from step 3 on because the last control wins."""
    pairs = [(0, 1), (1, 2), (1, 6), (2, 3), (2, 4), (3, 7), (3, 6), (4, 5), (5, 6)]      # link 0 .. 8
    P, N = len(pairs), 8
    rng = np.random.RandomState(KINDS_SEED)
    length, diameter = rng.uniform(100.0, 400.0, P), rng.uniform(0.15, 0.3, P)
    elevation = np.array([0.0, 2.0, 4.0, 6.0, 3.0, 2.0, 5.0, 40.0])
    net = H.HydraulicNetwork(HR._edge_index(pairs), length, diameter, elevation, [0, 7], [5.0, 43.0], tank_nodes=[7], tank_diameter=[10.0],
                             tank_min_level=[0.0], tank_max_level=[8.0], pump_links=[0], pump_h0=[70.0], pump_r=[3000.0], pump_n=[2.0],
                             valve_links=[4], valve_kind=["PRV"], valve_setting=[25.0])
    assert [tuple(p) for p in net.pipes] == pairs
    S, T = 2, KINDS_STEPS
    demand = np.zeros((S, N))
    demand[:, 1:7] = rng.uniform(0.002, 0.005, (S, 6))
    mult = rng.uniform(0.7, 1.3, (2, T))
    closed = np.zeros((S, P), dtype=np.uint8)
    closed[1, 2] = 1
    controls = H.control_table(net, [
        (0, ("setting", 0.9), "at_step", 1),
        (0, "closed", "tank_above", 0, KINDS_BAND[pda][0][1]),
        (0, "open", "tank_below", 0, KINDS_BAND[pda][0][0]),
        (4, ("setting", 20.0), "node_below", 5, 27.0),
        (4, ("setting", 28.0), "node_above", 5, 1000.0),
        (4, "closed", "at_step", 5),
        (4, "open", "at_step", 7),
        (8, "closed", "node_above", 5, 55.0),
        (8, "open", "at_step", 4),
        (2, "closed", "at_step", 3),
        (2, "open", "at_step", 3),
    ])
    threshold = np.tile(controls.threshold, (S, 1))
    threshold[:, 1], threshold[:, 2] = [hi for _, hi in KINDS_BAND[pda]], [lo for lo, _ in KINDS_BAND[pda]]
    roughness = rng.uniform(90.0, 130.0, (S, P))
    if KINDS_ROUGHNESS_SEED:
        roughness = np.random.RandomState(KINDS_ROUGHNESS_SEED).uniform(90.0, 130.0, (S, P))
    return _full(net, S, T, threshold=threshold, demand=demand, roughness=roughness, mult=mult,
                 pattern=(np.arange(N) % 2).astype(np.int64), dt=600.0, level0=np.array([[3.4], [3.0]]), controls=controls,
                 closed=closed, speed=np.array([[1.0], [1.05]]), smult=rng.uniform(0.9, 1.1, (1, T)),
                 pdd=KINDS_PDD if pda else None)


# ---- dense: where the loops turn over ------------------------------------------------------------------------------------------------
DENSE_FILLERS = (130, 140)              # fillers before and after the live controls: Kc = 130 + 5 + 140 = 275 > 256


@functools.lru_cache(maxsize=None)
def dense_case(pda):
    """``hydraulic_dense_refs.series_case`` with a table of more than 256 controls.  The fillers never fire (AT_STEP ``NEVER``, a
    tank level of 1e9 m) but sit on the live controls' links with the opposite action, before and after them, so that a pass that
    took a filler for live, or stopped at 256 controls, gives another answer.  The live ones: a pipe with index >= 256 is CLOSED at
    step 1 and OPEN at step 4, a pipe below 256 is CLOSED at step 2, pump 0 gets a speed setting at step 3 and a PRV a new setting by
    the level of tank 0."""
    c = dict(DR.series_case(pda))
    net = c["net"]
    special = net.is_pump | net.is_valve | net.check_valve | net.closed
    tank_or_res = np.isin(net.pipes[:, 0], np.flatnonzero(net.fixed)) | np.isin(net.pipes[:, 1], np.flatnonzero(net.fixed))
    plain = np.flatnonzero(~special & ~tank_or_res)
    hi, lo = int(plain[plain >= DR.HY_T][3]), int(plain[plain < DR.HY_T][40])
    pump, prv = int(net.pump_links[0]), int(net.valve_links[net.valve_kind == H.LINK_PRV][0])
    k_prv = int(np.flatnonzero(net.valve_links == prv)[0])
    live = [(hi, "closed", "at_step", 1), (hi, "open", "at_step", 4), (lo, "closed", "at_step", 2),
            (pump, ("setting", 0.97), "at_step", 3),
            (prv, ("setting", float(c["setting"][:, k_prv].mean())), "tank_above", 0, 0.0)]
    links = (hi, lo, pump, prv)
    filler = lambda i: (links[i % 4], "open" if i % 2 else "closed", "at_step", NEVER) if i % 3 else \
        (links[i % 4], "closed", "tank_above", i % 2, 1e9)
    rows = [filler(i) for i in range(DENSE_FILLERS[0])] + live + [filler(i + 1) for i in range(DENSE_FILLERS[1])]
    c.update(controls=H.control_table(net, rows), closed=None, live=(DENSE_FILLERS[0], DENSE_FILLERS[0] + len(live)), links=links)
    assert len(c["controls"]) > DR.HY_T and hi >= DR.HY_T > lo
    return c


CASES = {"operating": lambda pda: operating_case(), "kinds": kinds_case, "dense": dense_case}


def case(name, pda=False):
    return CASES[name](pda)


@functools.lru_cache(maxsize=None)
def reference(name, warm=True, pda=False):
    return _reference(case(name, pda), warm)


def moved_answers(name, warm, pda):
    """ROBUST, as hydraulic_dense_refs.moved_answers: the case with every roughness moved by one ulp, up and down, dense and banded,
    as (name, the comparisons with the case's reference, same statuses and control_changes)."""
    c, ref = case(name, pda), reference(name, warm, pda)
    out = []
    for way in (np.inf, 0.0):
        for solver in ("banded", "dense"):
            sol = solution(simulate_ref(dict(c, roughness=np.nextafter(c["roughness"], way)), solver, warm))
            out.append((f"{'up' if way else 'down'}-{solver}", series_comparisons(c, ref, sol), same_statuses(ref["dense"], sol)))
    return out


def misses(name, warm, pda, got):
    """What a solution misses of the comparisons the GPU test makes: the names of the bounds it exceeds, and "statuses"."""
    c, ref = case(name, pda), reference(name, warm, pda)
    out = list(DR.exceeded(series_comparisons(c, ref, got)))
    if not same_statuses(ref["dense"], got):
        out.append("statuses")
    return out


# ---- planted wrong answers: the host solution of a WRONG model of the controls ----------------------------------------------------------
WRONG = ("state_not_reset_between_series", "controls_applied_a_step_late", "first_control_wins", "reopened_link_not_restarted",
         "valve_not_restarted_active")


def wrong_answer(kind, name="kinds", warm=True, pda=False):
    """The banded host solution of the case under one planted mistake of a kernel."""
    c = case(name, pda)
    right_step, right_state, right_start = H.control_step_ref, H.control_state, H.control_start_ref
    last = {}

    def keep_step(table, threshold, state, level, pressure_prev, t):
        st, n = right_step(table, threshold, state, level, pressure_prev, t)
        last["state"] = st
        return st, n

    def stale_state(num_links):          # the state the series before left behind
        return {k: v.copy() for k, v in last["state"].items()} if last else right_state(num_links)

    def late_step(table, threshold, state, level, pressure_prev, t):
        # the pass runs behind the step's inputs: what it decides at step t acts from step t + 1 on
        pending = state.get("pending", state)
        new, n = right_step(table, threshold, {k: v for k, v in pending.items() if k != "pending"}, level, pressure_prev, t)
        acting = {k: v.copy() for k, v in pending.items() if k != "pending"}
        acting["pending"] = new
        return acting, n

    def first_wins(table, threshold, state, level, pressure_prev, t):
        back = H.ControlTable(*(getattr(table, f)[::-1] for f in ("link", "action", "value", "kind", "target", "threshold")))
        return right_step(back, np.asarray(threshold)[::-1], state, level, pressure_prev, t)

    patches = {"state_not_reset_between_series": [("control_step_ref", keep_step), ("control_state", stale_state)],
               "controls_applied_a_step_late": [("control_step_ref", late_step)],
               "first_control_wins": [("control_step_ref", first_wins)],
               "reopened_link_not_restarted": [("control_start_ref", lambda st, ws, t: (np.zeros_like(ws), right_start(st, ws, t)[1]))],
               "valve_not_restarted_active": [("control_start_ref", lambda st, ws, t: (right_start(st, ws, t)[0], np.zeros_like(ws)))]}
    with contextlib.ExitStack() as stack:
        for attr, fn in patches[kind]:
            stack.enter_context(DR._patched(attr, lambda right, fn=fn: fn))
        sol = simulate_ref(c, "banded", warm)
    return solution(sol)
