"""``wdn_io.parse_inp_hydraulics(controls="model")`` on the host: a small input text with both forms of control line, in SI and in US
units, gives the tuples written out below by hand; every refusal names its offender; the default and ``ignore_controls=True``
behave as they always did; [RULES] is still refused.  No GPU."""
import numpy as np
import pytest

import hydraulics_refs as HR

H, G = HR.H, HR.G
io = G.wdn_io

TEXT = """
[JUNCTIONS]
 J1 10 1.0
 J2 12 2.0
 J3 15 1.5
[RESERVOIRS]
 R1 20
[TANKS]
 T1 55 3 0.5 6 10
[PIPES]
 P1 J1 J2 300 300 120 0 Open
 P2 J2 J3 250 250 110 0 Open
 P3 J3 T1 200 200 100 0 {p3}
[PUMPS]
 PU1 R1 J1 HEAD C1
[VALVES]
 V1 J2 J3 200 PRV 30 {vk}
[CURVES]
 C1 40 50
[OPTIONS]
 UNITS {units}
 HEADLOSS H-W
[CONTROLS]
{controls}
{extra}
"""
CONTROLS = """ LINK PU1 CLOSED IF NODE T1 ABOVE 5
 LINK PU1 OPEN IF NODE T1 BELOW 1.5
 link PU1 0.8 at time 2
 LINK V1 25 IF NODE J3 BELOW 18
 LINK P2 CLOSED AT TIME 1:30
 LINK P2 OPEN AT TIME 0:45:30
"""
# links in file order: P1 0, P2 1, P3 2, PU1 3, V1 4; nodes J1 0, J2 1, J3 2, R1 3, T1 4; one tank


def parse(lines=CONTROLS, units="LPS", p3="Open", extra="", mode="model", **kw):
    return io.parse_inp_hydraulics(text=TEXT.format(controls=lines, units=units, p3=p3, extra=extra, vk=0), regulating="model", controls=mode,
                                   **kw)


def test_both_forms_of_control_line_in_si_units():
    r = parse()
    assert r.controls == ((3, "closed", "tank_above", 0, 5.0), (3, "open", "tank_below", 0, 1.5), (3, ("setting", 0.8), "at_time", 7200.0),
                          (4, ("setting", 25.0), "node_below", 2, 18.0), (1, "closed", "at_time", 5400.0), (1, "open", "at_time", 2730.0))
    with pytest.raises(ValueError, match="control 5.*whole number of steps"):
        H.control_table(r.network, r.controls, 300.0)
    table = H.control_table(r.network, r.controls, 30.0)
    assert table.link.tolist() == [3, 3, 3, 4, 1, 1] and table.action.tolist() == [1, 0, 2, 2, 1, 0]
    assert table.kind.tolist() == [1, 0, 4, 2, 4, 4] and table.target.tolist() == [0, 0, 240, 2, 180, 91]
    assert table.value.tolist() == [0.0, 0.0, 0.8, 25.0, 0.0, 0.0] and table.threshold.tolist() == [5.0, 1.5, 0.0, 18.0, 0.0, 0.0]
    with pytest.raises(ValueError, match="needs step_seconds"):
        H.control_table(r.network, r.controls)


def test_the_same_lines_in_us_units_are_converted():
    """A tank's level in feet, a junction's pressure and a PRV's setting in psi (EPANET's 0.4333 psi per foot), a speed as it is."""
    r = parse(units="GPM")
    foot, psi = 0.3048, 0.3048 / 0.4333
    got = r.controls
    assert got[0] == (3, "closed", "tank_above", 0, 5 * foot) and got[1] == (3, "open", "tank_below", 0, 1.5 * foot)
    assert got[2] == (3, ("setting", 0.8), "at_time", 7200.0)
    assert got[3][:4] == (4, ("setting", pytest.approx(25 * psi, rel=1e-15)), "node_below", 2) and got[3][4] == pytest.approx(18 * psi, rel=1e-15)
    assert got[4:] == ((1, "closed", "at_time", 5400.0), (1, "open", "at_time", 2730.0))


def test_what_was_read_operates_the_series():
    r = parse(lines=" LINK PU1 CLOSED AT TIME 0:10\n LINK PU1 OPEN AT TIME 0:20\n")
    ser = H.simulate_series_ref(r.network, r.demand[None], r.roughness[None], np.ones((1, 4)), 300.0, pump_speed=r.pump_speed[None],
                                controls=H.control_table(r.network, r.controls, 300.0))
    assert not ser.failed.any()
    assert ser.link_state[0, :, 3].tolist() == [0, 0, 2, 2] and ser.control_changes[0].tolist() == [0, 0, 1, 0]


REFUSED = [
    (" LINK PU1 CLOSED AT CLOCKTIME 6 AM\n", "AT CLOCKTIME"),
    (" LINK PX CLOSED AT TIME 2\n", "no link PX"),
    (" LINK P1 CLOSED IF NODE JX ABOVE 3\n", "no node JX"),
    (" LINK P1 0.5 AT TIME 2\n", "link P1 takes no setting"),
    (" LINK P1 HALF AT TIME 2\n", "neither OPEN, CLOSED nor a number"),
    (" LINK P1 CLOSED AT TIME soon\n", "soon is no number"),
    (" LINK P1 CLOSED IF NODE J1 ABOVE high\n", "high is no number"),
    (" PUMP PU1 CLOSED AT TIME 2\n", "not of the form"),
    (" LINK P1 CLOSED IF NODE J1 NEAR 3\n", "not of the form"),
    (" LINK P1 CLOSED IF NODE R1 ABOVE 3\n", "fixed-head node"),
    (" LINK PU1 -0.5 AT TIME 2\n", "negative on a pump"),
]


@pytest.mark.parametrize("line,what", REFUSED)
def test_a_refusal_names_its_offender(line, what):
    with pytest.raises(ValueError, match=r"\[CONTROLS\] line 2.*" + what):
        parse(lines=" LINK P2 OPEN AT TIME 1\n" + line)


def test_a_control_on_a_cv_pipe_is_refused_by_name():
    with pytest.raises(ValueError, match=r"\[CONTROLS\] line 1.*CHECK pipe"):
        parse(lines=" LINK P3 CLOSED AT TIME 1\n", p3="CV")


def test_a_valve_takes_a_setting_only_as_a_regulating_valve():
    with pytest.raises(ValueError, match="link V1 takes no setting"):
        io.parse_inp_hydraulics(text=TEXT.format(controls=" LINK V1 25 AT TIME 1\n", units="LPS", p3="Open", extra="", vk=2.5), controls="model",
                                unsupported_valves="open")
    with pytest.raises(ValueError, match='controls must be None or "model"'):
        parse(lines="", mode="all")


def test_the_default_and_ignore_controls_are_as_they_were():
    with pytest.raises(ValueError, match=r"\[CONTROLS\] has 6 lines: controls and rules are not modelled"):
        parse(lines=CONTROLS, mode=None)
    dropped = parse(lines=CONTROLS, ignore_controls=True, mode=None)
    assert dropped.controls == ()
    assert parse(lines=CONTROLS, ignore_controls=True).controls == ()            # told to drop them, it drops them
    assert parse(lines="").controls == () and io.InpHydraulics._field_defaults["controls"] == ()
    plain = io.parse_inp_hydraulics(text=TEXT.format(controls="", units="LPS", p3="Open", extra="", vk=0), regulating="model")
    assert plain.controls == () and len(plain) == 15


def test_rules_are_still_refused():
    rules = "[RULES]\n RULE 1\n IF TANK T1 LEVEL ABOVE 5\n THEN PUMP PU1 STATUS IS CLOSED\n"
    with pytest.raises(ValueError, match=r"\[RULES\] has 3 lines"):
        parse(extra=rules)
    assert parse(extra=rules, ignore_controls=True, mode=None).controls == ()
