"""The generator side of the link law, on the host: ``make_hydraulic_network`` with pumps, check valves and minor losses draws them
after everything else; ``hydraulic_link_draws`` puts its cells after the existing ones; and ``solve_ref`` alone keeps at least
seven eighths of the 64 scenarios that tests/test_gpu_hydraulic_links.py generates a store from.  No GPU."""
import numpy as np
import pytest

import hydraulic_links_refs as LR

HR, H, G = LR.HR, LR.H, LR.G


def test_make_hydraulic_network_draws_the_special_links_after_everything_else():
    mk = G.wdn_synth.make_hydraulic_network
    for kw in (dict(), dict(num_tanks=1)):
        plain = mk(40, 44, 2, seed=5, **kw)
        same = mk(40, 44, 2, seed=5, num_pumps=0, num_check_valves=0, minor_loss_range=None, **kw)
        links = mk(40, 44, 2, seed=5, num_pumps=2, num_check_valves=6, minor_loss_range=(0.5, 5.0), **kw)
        again = mk(40, 44, 2, seed=5, num_pumps=2, num_check_valves=6, minor_loss_range=(0.5, 5.0), **kw)
        assert not plain.has_links and not same.has_links and links.has_links
        for k in ("length", "diameter", "elevation", "fixed_head", "fixed_nodes", "tank_diameter", "coef", "pipes"):
            assert np.array_equal(getattr(plain, k), getattr(same, k)), k
        for k in ("length", "diameter", "elevation", "fixed_head", "fixed_nodes", "tank_diameter"):
            assert np.array_equal(getattr(plain, k), getattr(links, k)), k
        for k in ("pipes", "pump_links", "pump_h0", "pump_r", "minor_loss", "check_valve"):
            assert np.array_equal(getattr(links, k), getattr(again, k)), k
        assert links.num_pumps == 2 and int((links.check_valve & ~links.is_pump).sum()) == 6
        a, b = links.pipes[links.pump_links, 0], links.pipes[links.pump_links, 1]
        assert links.fixed[a].all() and not links.fixed[b].any()             # a pump runs from its source to the junction
        lo, hi = G.wdn_synth.PUMP_SHUTOFF_RANGE
        assert ((links.pump_h0 >= lo) & (links.pump_h0 <= hi)).all() and (links.pump_n == 2).all()
        # half the shut-off head at the design velocity in the pump's link
        q = G.wdn_synth.PUMP_DESIGN_VELOCITY * np.pi * links.diameter[links.pump_links] ** 2 / 4
        assert np.allclose(links.pump_h0 - links.pump_r * q ** 2, 0.5 * links.pump_h0, rtol=1e-12)
        k = links.minor_loss[~links.is_pump]
        assert ((k >= 0.5) & (k <= 5.0)).all() and (links.minor_loss[links.is_pump] == 0).all()
    with pytest.raises(ValueError, match="num_pumps"):
        mk(40, 44, 1, seed=5, num_pumps=30)
    with pytest.raises(ValueError, match="check valves"):
        mk(12, 11, 1, seed=5, num_check_valves=11, num_pumps=1)             # a tree: some link must point away from its leaves


def test_link_draws_come_after_the_existing_cells():
    net = LR.case("net40_links")["net"]
    ranges = net.draw_ranges((1e-4, 1e-3), H.ROUGHNESS_RANGE)
    old_d, old_c = H.hydraulic_draws(7, 3, 64, *ranges)
    d, c, speed, closed = H.hydraulic_link_draws(7, 3, 64, *ranges, net.num_pumps, (0.8, 1.2), 0.25)
    assert d.tobytes() == old_d.tobytes() and c.tobytes() == old_c.tobytes()
    assert speed.shape == (64, net.num_pumps) and ((speed >= 0.8) & (speed < 1.2)).all() and np.unique(speed).size == speed.size
    assert closed.shape == (64, net.num_pipes) and closed.dtype == np.uint8 and closed.max() == 1
    assert abs(closed.mean() - 0.25) < 4 * np.sqrt(0.25 * 0.75 / closed.size)      # four standard deviations of the mean
    _, _, one, none = H.hydraulic_link_draws(7, 3, 64, *ranges, net.num_pumps, None, 0.0)
    assert (one == 1.0).all() and not none.any()
    # a scenario's draws do not depend on the chunk it is drawn in
    _, _, s2, c2 = H.hydraulic_link_draws(7, 13, 5, *ranges, net.num_pumps, (0.8, 1.2), 0.25)
    assert s2.tobytes() == speed[10:15].tobytes() and c2.tobytes() == closed[10:15].tobytes()
    with pytest.raises(ValueError):
        H.link_draw_ranges(ranges[2], ranges[3], net.num_pumps, (1.2, 0.8))


def test_solve_ref_alone_keeps_seven_eighths_of_the_store_scenarios():
    """The condition of the generated-store test on the device (at most a quarter dropped) is set with this margin."""
    net = LR.case("net40_links")["net"]
    d, c, speed, closed = H.hydraulic_link_draws(LR.STORE_SEED, 0, LR.STORE_SCENARIOS, *net.draw_ranges(LR.STORE_DEMAND, H.ROUGHNESS_RANGE),
                                                 net.num_pumps, LR.STORE_SPEED, 0.0)
    ref = H.solve_ref(net, d, c, pump_speed=speed, link_closed=closed)
    pressure = (ref.head - net.elevation[None, :])[:, ~net.fixed]
    lo, hi = LR.STORE_PRESSURE
    kept = ref.converged & ~ref.failed & ((pressure >= lo) & (pressure <= hi)).all(axis=1)
    print(f"solve_ref keeps {int(kept.sum())} of {LR.STORE_SCENARIOS}; pressures {pressure.min():.1f} .. {pressure.max():.1f} m")
    assert kept.sum() >= LR.STORE_SCENARIOS - LR.STORE_SCENARIOS // 8
