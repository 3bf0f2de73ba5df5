"""THE REGULATING VALVES on the host (hydraulics.py): the restatement ``solve_ref`` against closed forms on chains with a PRV or a
PSV in each of its statuses, the six status rules, the constructor's refusals, the two singular layouts, the draw restatement,
``make_hydraulic_network``'s valves, and ``hydraulic_residuals`` catching wrong statements of the valve.  No GPU."""
import numpy as np
import pytest

import hydraulic_valves_refs as VR
import hydraulics_refs as HR

H, G = HR.H, HR.G
ROUNDING = HR.FLOOR_ULPS * HR.EPS * VR.H0 * 16      # metres: 64 ulp of the heads, through the few operations of a closed form


def chain(name):
    c, ref = VR.case(name), VR.reference(name)["dense"]
    heads, flows = VR.chain_exact(name)
    print(name, "iterations", ref.iterations.tolist(), "state", ref.link_state[:, 1].tolist(), "changes", ref.valve_changes.tolist())
    for i, e in heads.items():
        print(f"  head[{i}] error {np.abs(ref.head[:, i] - e).max():.3e}")
    for i, e in flows.items():
        print(f"  flow[{i}] error {np.abs(ref.flow[:, i] - e).max():.3e}")
    assert (ref.link_state[:, 1] == VR.CHAIN_STATE[name]).all()
    return c, ref, heads, flows


@pytest.mark.parametrize("name", ("prv_active", "psv_active"))
def test_active_valve_holds_the_target_head_to_rounding(name):
    c, ref, heads, flows = chain(name)
    node = int(c["net"].valve_node[0])
    assert (ref.head[:, node] == heads[node]).all()         # H_c = hset: an identity row
    for i, e in heads.items():
        assert np.abs(ref.head[:, i] - e).max() <= ROUNDING
    for i, e in flows.items():                               # the flows to the stop rule's accuracy
        assert np.abs(ref.flow[:, i] - e).max() <= H.ACCURACY * np.abs(e).max()
    if name == "prv_active":                                 # q = the downstream demand, H_a = H0 - r q^1.852
        assert np.abs(ref.flow[:, 1] - c["demand"][:, 3]).max() <= ROUNDING


@pytest.mark.parametrize("name", ("prv_open", "psv_open"))
def test_open_valve_loses_its_minor_loss(name):
    c, ref, heads, flows = chain(name)
    q, m = ref.flow[:, 1], c["net"].minor[1]
    assert np.abs(ref.head[:, 1] - ref.head[:, 2] - m * q * q).max() <= ROUNDING       # H_b = H_a - m q^2
    for i, e in heads.items():                               # a head moves by g <= 50 s/m2 times the flow's accuracy
        assert np.abs(ref.head[:, i] - e).max() <= 50.0 * H.ACCURACY * 0.2
    for i, e in flows.items():
        assert np.abs(ref.flow[:, i] - e).max() <= H.ACCURACY * 0.2


@pytest.mark.parametrize("name", ("prv_closed_reverse", "prv_closed_held", "psv_closed_reverse", "psv_closed_held"))
def test_closed_valve_passes_nothing(name):
    c, ref, heads, flows = chain(name)
    dh = ref.head[:, 1] - ref.head[:, 2]
    assert np.abs(ref.flow[:, 1] - dh / 1e8).max() <= 1e-12 and np.abs(ref.flow[:, 1]).max() <= VR.CLOSED_LEAK_FLOW
    for i, e in heads.items():
        assert np.abs(ref.head[:, i] - e).max() <= VR.CLOSED_LEAK_HEAD
    for i, e in flows.items():
        assert np.abs(ref.flow[:, i] - e).max() <= VR.CLOSED_LEAK_FLOW
    if name.endswith("reverse"):                             # the higher reservoir is downstream: H_b > H_a
        assert (dh < 0).all()
    else:                                                    # closed although the water would run forward
        assert (dh > 0).all()


@pytest.mark.parametrize("name", VR.NAMES)
def test_references_converge_decisively_and_satisfy_the_model(name):
    ref = VR.reference(name)                                 # (asserts convergence, decisiveness and dense = banded statuses)
    print(name, ref["dense"].iterations.tolist(), ref["dense"].margin.min(axis=0).tolist(), ref["mass"].max(), ref["energy"].max())
    assert ref["mass"].max() <= 1e-8 and ref["energy"].max() <= 1e-6


# ---- the six rules ----------------------------------------------------------------------------------------------------------------------
O, A, C = H.VALVE_OPEN, H.VALVE_ACTIVE, H.VALVE_CLOSED
RULES = [   # kind, from, H_a, H_b, q, m, hset -> to
    ("PRV", A, 50.0, 40.0, -1e-3, 0.0, 40.0, C), ("PRV", A, 39.0, 40.0, 1e-3, 0.0, 40.0, O), ("PRV", A, 50.0, 40.0, 1e-3, 0.0, 40.0, A),
    ("PRV", A, 40.5, 40.0, 1.0, 1.0, 40.0, O),                # the minor loss counts: H_a - m q^2 < hset
    ("PRV", O, 50.0, 45.0, -1e-3, 0.0, 40.0, C), ("PRV", O, 50.0, 41.0, 1e-3, 0.0, 40.0, A), ("PRV", O, 39.0, 38.0, 1e-3, 0.0, 40.0, O),
    ("PRV", C, 50.0, 30.0, 0.0, 0.0, 40.0, A), ("PRV", C, 39.0, 30.0, 0.0, 0.0, 40.0, O), ("PRV", C, 50.0, 45.0, 0.0, 0.0, 40.0, C),
    ("PRV", C, 30.0, 35.0, 0.0, 0.0, 40.0, C),
    ("PSV", A, 50.0, 40.0, -1e-3, 0.0, 50.0, C), ("PSV", A, 50.0, 51.0, 1e-3, 0.0, 50.0, O), ("PSV", A, 50.0, 40.0, 1e-3, 0.0, 50.0, A),
    ("PSV", A, 50.0, 49.5, 1.0, 1.0, 50.0, O),
    ("PSV", O, 60.0, 40.0, -1e-3, 0.0, 50.0, C), ("PSV", O, 49.0, 40.0, 1e-3, 0.0, 50.0, A), ("PSV", O, 60.0, 40.0, 1e-3, 0.0, 50.0, O),
    ("PSV", C, 60.0, 55.0, 0.0, 0.0, 50.0, O), ("PSV", C, 60.0, 40.0, 0.0, 0.0, 50.0, A), ("PSV", C, 45.0, 40.0, 0.0, 0.0, 50.0, C),
    ("PSV", C, 60.0, 70.0, 0.0, 0.0, 50.0, C),
]


def test_the_six_status_rules():
    cols = list(zip(*RULES))
    got = H.valve_status_ref(list(cols[0]), cols[1], cols[2], cols[3], cols[4], cols[5], cols[6])
    assert got.tolist() == list(cols[7])
    # the tolerances: inside HTOL and QTOL nothing moves
    assert H.valve_status_ref("PRV", A, 40.0 - 0.5 * H.VALVE_HTOL, 40.0, 1e-3, 0.0, 40.0)[0] == A
    assert H.valve_status_ref("PRV", A, 50.0, 40.0, -0.5 * H.VALVE_QTOL, 0.0, 40.0)[0] == A
    assert H.valve_status_ref("PSV", O, 50.0 - 0.5 * H.VALVE_HTOL, 40.0, 1e-3, 0.0, 50.0)[0] == O
    with pytest.raises(ValueError):
        H.valve_status_ref("FCV", A, 1.0, 1.0, 1.0, 0.0, 1.0)


# ---- the constructor --------------------------------------------------------------------------------------------------------------------
def build(pairs, fixed, heads, N, **kw):
    P = len(pairs)
    return H.HydraulicNetwork(HR._edge_index(pairs), np.full(P, 100.0), np.full(P, 0.2), np.zeros(N), fixed, heads, **kw)


CHAIN4 = [(0, 1), (1, 2), (2, 3)]


def test_constructor_takes_a_valve_and_reads_neither_its_length_nor_a_roughness():
    net = H.HydraulicNetwork(HR._edge_index(CHAIN4), [100.0, np.nan, 100.0], np.full(3, 0.2), np.zeros(4), [0], [60.0],
                             valve_links=[1], valve_kind="PRV", valve_setting=[40.0])
    assert net.has_valves and net.coef[1] == 0 and net.link_kind.tolist() == [0, H.LINK_PRV, 0] and net.valve_node.tolist() == [2]
    d = np.zeros((1, 4))
    d[0, 3] = 0.01
    rough = np.array([[100.0, np.nan, 100.0]])
    ref = H.solve_ref(net, d, rough)
    assert ref.converged.all() and ref.head[0, 2] == 40.0
    psv = build(CHAIN4, [0, 3], [60.0, 20.0], 4, valve_links=[1], valve_kind=["PSV"], valve_setting=[50.0])
    assert psv.valve_node.tolist() == [1] and psv.link_kind[1] == H.LINK_PSV


def test_refused_a_valve_that_is_a_pump():
    with pytest.raises(ValueError, match="neither a pump nor a CHECK"):
        build(CHAIN4, [0], [60.0], 4, valve_links=[0], valve_kind="PRV", valve_setting=[40.0], pump_links=[0], pump_h0=[10.0], pump_r=[1.0])


def test_refused_a_valve_that_is_a_check_link():
    with pytest.raises(ValueError, match="neither a pump nor a CHECK"):
        build(CHAIN4, [0], [60.0], 4, valve_links=[1], valve_kind="PRV", valve_setting=[40.0], check_valve=[False, True, False])


def test_refused_a_controlled_node_that_is_fixed():
    with pytest.raises(ValueError, match="controlled node"):
        build(CHAIN4, [0, 3], [60.0, 20.0], 4, valve_links=[2], valve_kind="PRV", valve_setting=[40.0])      # PRV 2 -> 3, 3 fixed
    with pytest.raises(ValueError, match="controlled node"):
        build(CHAIN4, [0], [60.0], 4, valve_links=[0], valve_kind="PSV", valve_setting=[40.0])               # PSV 0 -> 1, 0 fixed


def test_refused_two_valves_that_share_a_node():
    with pytest.raises(ValueError, match="share a node"):
        build(CHAIN4 + [(3, 4)], [0], [60.0], 5, valve_links=[1, 2], valve_kind=["PRV", "PRV"], valve_setting=[40.0, 30.0])


def test_refused_a_setting_that_is_not_finite():
    for s in (np.nan, np.inf):
        with pytest.raises(ValueError, match="finite"):
            build(CHAIN4, [0], [60.0], 4, valve_links=[1], valve_kind="PRV", valve_setting=[s])


def test_refused_bad_valve_arguments():
    with pytest.raises(ValueError, match="distinct links"):
        build(CHAIN4, [0], [60.0], 4, valve_links=[3], valve_kind="PRV", valve_setting=[40.0])
    with pytest.raises(ValueError, match="PRV"):
        build(CHAIN4, [0], [60.0], 4, valve_links=[1], valve_kind="FCV", valve_setting=[40.0])


def test_refused_singular_an_uncontrolled_end_that_reaches_no_fixed_head():
    """reservoir 0 -- 1 -- PSV 1 -> 2 -- 2 -- 3: the PSV's downstream end hangs on the valve alone, and an ACTIVE valve is not in
    the matrix."""
    with pytest.raises(ValueError, match="uncontrolled end"):
        build(CHAIN4, [0], [60.0], 4, valve_links=[1], valve_kind="PSV", valve_setting=[50.0])


def test_refused_singular_a_junction_that_reaches_neither_a_fixed_head_nor_a_controlled_node():
    """reservoir 0 -- 1 -- PRV 1 -> 2, and 2 -- CHECK 3 -> 2 -- 3: node 3 lies upstream of a check valve towards the controlled
    node, so nothing holds its head."""
    with pytest.raises(ValueError, match="controlled node of a regulating valve"):
        build(CHAIN4, [0], [60.0], 4, valve_links=[1], valve_kind="PRV", valve_setting=[40.0], check_valve=[False, False, True],
              link_reversed=[False, False, True])
    with pytest.raises(ValueError, match="not connected"):   # without the valve the old words, as ever
        build(CHAIN4, [0], [60.0], 4, closed=[False, True, False])


def test_shut_valve_is_a_shut_link_without_a_status():
    c = VR.case("prv_closed_held")
    net = c["net"]
    shut = np.zeros(net.num_pipes, dtype=np.uint8)
    shut[1] = 1
    ref = H.solve_ref(net, c["demand"], c["roughness"], link_closed=shut)
    assert (ref.link_state[:, 1] == 2).all() and not ref.valve_changes.any() and ref.converged.all()


def test_a_setting_of_nan_fails_its_scenario_alone_on_the_host():
    c = VR.case("prv_active")
    s = np.array([[40.0], [np.nan], [40.0]])
    ref = H.solve_ref(c["net"], c["demand"], c["roughness"], valve_setting=s)
    assert ref.failed.tolist() == [False, True, False] and np.isnan(ref.head[1]).all()


def test_lds_need_is_the_links_need_and_24_bytes_per_valve():
    assert H.valves_lds_bytes(40, 44, 9, 2, 3) == H.links_lds_bytes(40, 44, 9, 2) + 72
    assert H.series_valves_lds_bytes(40, 44, 9, 2, 1, 3) == H.series_links_lds_bytes(40, 44, 9, 2, 1) + 72
    net = VR.case("net40_v3")["net"]                        # the constructor holds the network to the sum of its own launch
    assert H.valves_lds_bytes(40, 44, net.half_bandwidth, 0, 3) <= H.LDS_BUDGET


# ---- the draws --------------------------------------------------------------------------------------------------------------------------
def test_valve_cells_leave_every_existing_cell_as_it_was():
    net = VR.case("net40_v3")["net"]
    r = net.draw_ranges((1e-4, 1e-3), H.ROUGHNESS_RANGE)
    old = H.hydraulic_link_draws(7, 5, 9, *r, 0, (0.8, 1.2), 0.1)
    new = H.hydraulic_valve_draws(7, 5, 9, *r, 0, net.num_valves, (20.0, 60.0), (0.8, 1.2), 0.1)
    for a, b in zip(old, new[:4]):
        assert a.tobytes() == b.tobytes() and a.shape == b.shape
    plain = H.hydraulic_draws(7, 5, 9, *r)
    assert plain[0].tobytes() == new[0].tobytes() and plain[1].tobytes() == new[1].tobytes()
    s = new[4]
    assert s.shape == (9, 3) and (s >= 20.0).all() and (s < 60.0).all() and np.unique(s).size == 27
    # chunks give the bits of one call
    part = H.hydraulic_valve_draws(7, 8, 3, *r, 0, net.num_valves, (20.0, 60.0), (0.8, 1.2), 0.1)
    assert part[4].tobytes() == s[3:6].tobytes()


def test_make_hydraulic_network_places_valves_after_everything_else():
    base = G.wdn_synth.make_hydraulic_network(40, 44, 2, seed=5)
    net = G.wdn_synth.make_hydraulic_network(40, 44, 2, seed=5, num_prvs=2, num_psvs=1)
    for k in ("diameter", "elevation", "fixed_head"):
        assert np.array_equal(getattr(base, k), getattr(net, k)), k
    keep = ~net.is_valve
    assert np.array_equal(base.length[keep], net.length[keep]) and net.valve_kind_names == ("PRV", "PRV", "PSV")
    assert np.array_equal(np.sort(base.pipes, axis=1), np.sort(net.pipes, axis=1))
    # oriented along the flow of the network without valves in the nominal scenario
    demand = np.where(base.fixed, 0.0, 0.5 * (H.DEMAND_RANGE[0] + H.DEMAND_RANGE[1]))[None, :]
    flow = H.solve_ref(base, demand, np.full((1, 44), 0.5 * sum(H.ROUGHNESS_RANGE)), solver="banded").flow[0]
    for p in net.valve_links:
        along = 1.0 if tuple(net.pipes[p]) == tuple(base.pipes[p]) else -1.0
        assert along * flow[p] >= 0
    other = G.wdn_synth.make_hydraulic_network(40, 44, 2, seed=5, num_prvs=2, num_psvs=1, valve_seed=3)
    assert not np.array_equal(other.valve_links, net.valve_links)
    with pytest.raises(ValueError):
        G.wdn_synth.make_hydraulic_network(40, 44, 2, seed=5, num_prvs=-1)


# ---- residuals catch a wrong statement of the valve -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", VR.WRONG_LAWS)
def test_wrong_statements_of_the_valve_are_caught(kind):
    """Under the right statement the reference's own solution leaves an energy residual below 1e-6 m; under each wrong one, on a
    case whose valves are ACTIVE somewhere, at least 1e-2 m."""
    c, ref = VR.case("net40_v2"), VR.reference("net40_v2")
    assert (ref["dense"].link_state == H.VALVE_ACTIVE).any() and ref["energy"].max() <= 1e-6
    _, energy = VR.wrong_residuals(kind, c, ref["dense"])
    print(kind, energy.tolist(), "right:", ref["energy"].tolist())
    assert energy.max() >= 1e-2


def test_residuals_need_the_statuses():
    c, ref = VR.case("prv_active"), VR.reference("prv_active")["dense"]
    with pytest.raises(ValueError, match="link_state"):
        H.hydraulic_residuals(c["net"], ref.head, ref.flow, c["demand"], c["roughness"])


def test_series_reference_carries_statuses_only_when_warm():
    """Two steps of prv_closed_held's chain: the demand of step 1 would leave an ACTIVE start ACTIVE -- but warm, the valve starts
    CLOSED and the CLOSED rule keeps it so only if H_b stays above hset; cold, it starts ACTIVE again and counts its changes."""
    c = VR.case("prv_closed_held")
    mult = np.array([[1.0, 1.0]])
    warm = H.simulate_series_ref(c["net"], c["demand"], c["roughness"], mult, 300.0, warm_start=True)
    cold = H.simulate_series_ref(c["net"], c["demand"], c["roughness"], mult, 300.0, warm_start=False)
    print(warm.valve_changes.tolist(), cold.valve_changes.tolist())
    assert (warm.link_state[:, :, 1] == C).all() and (cold.link_state[:, :, 1] == C).all()
    assert (warm.valve_changes[:, 1] == 0).all() and (cold.valve_changes[:, 1] == cold.valve_changes[:, 0]).all()
    assert (cold.valve_changes[:, 0] >= 1).all()
