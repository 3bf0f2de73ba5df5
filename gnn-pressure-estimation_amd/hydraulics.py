"""Hydraulically consistent pressure snapshots, generated on the device (csrc/k_hydraulics.hip).

The reference gets its training data from a hydraulic solver (EPANET through its scene generator) run over random scenarios of
demand, roughness and so on; ``wdn_synth.make_snapshots`` is N(0, 1) noise.  This module is the steady-state solver in between:
``HydraulicNetwork.simulate`` solves S independent scenarios, one workgroup each, and ``generate_store`` draws, solves and
filters scenarios straight into a ``SnapshotStore``.

THE MODEL (include/gatres.h states it for the kernel; this is the host statement).  Pipes, junctions and fixed-head nodes
(reservoirs, or tanks held at a level); demand-driven, steady, Hazen-Williams in SI units.  Pipe p from a to b carries q_p
(m3/s, positive from a to b):

    H_a - H_b = h_p(q_p),    h_p(q) = r_p |q|^0.852 q,    r_p = 10.667 L_p / (C_p^1.852 D_p^4.871)

and at every junction inflow - outflow = demand.  At low flow the law is EPANET's (``pipe_headloss``): where the gradient
g = 1.852 r |q|^0.852 falls below 1e-7, g = 1e-7 and h = 1e-7 q.  The solver is Newton's method in the global-gradient form of
Todini & Pilati, as in EPANET: per iteration one symmetric positive definite solve ``A H = F`` over the junctions
(A_ii = sum 1/g_p, A_ij = -1/g_p), then q <- q - (h - (H_a - H_b)) / g; flows start at 1 ft/s; it stops once
sum |dq| <= accuracy * sum |q|, or after ``max_iter`` iterations.

THE LINK LAW (gatres.h: THE LINK LAW; csrc/k_hydraulic_links.hip; ``link_headloss``).  A network built with ``minor_loss``,
``check_valve``, ``closed`` or ``pump_links`` takes the two links launches, which differ from the pipe launches in the law alone.
Every link has a kind, PIPE = 0 or PUMP = 1, and flags CHECK (flow only from a to b) and CLOSED; a pump is always CHECK.
PIPE, forward branch: h = r |q|^0.852 q + m |q| q, g = 1.852 r |q|^0.852 + 2 m |q|, with m = 8 K / (pi^2 * 9.80665 * D^4) from the
minor-loss coefficient K; m = 0 is the pipe above in every bit; r = 0 (length 0) with m > 0 is a throttle valve (EPANET's TCV);
where g < 1e-7: g = 1e-7, h = 1e-7 q.  PUMP, forward branch (q >= 0), at speed w with shut-off head h0 >= 0, coefficient rp > 0 and
exponent n >= 1: the gain is w^2 h0 - w^(2-n) rp q^n (the affinity laws), so h = -w^2 h0 + w^(2-n) rp q^n and
g = n w^(2-n) rp q^(n-1); where g < 1e-7: g = 1e-7, h = -w^2 h0 + 1e-7 q.  REVERSE BRANCH of a CHECK link (q < 0): g = 1e8,
h = h(0) + 1e8 q, h(0) = 0 for a pipe and -w^2 h0 for a pump.  A CLOSED link (by its flag or by ``link_closed``) or a pump with
w == 0: g = 1e8, h = 1e8 q at every q, and it starts at q = 0.  The law is continuous and monotone up to the jump at the low-flow
floor, so the system stays symmetric positive definite.  There is no status machine: a link that holds shut carries -dh / 1e8.
``link_state`` (uint8, at the returned flows): 0 forward, 1 a CHECK link on its reverse branch, 2 shut by input or by w == 0.
A link runs from the lower-numbered node to the higher one unless ``link_reversed`` says otherwise.  WHAT DOES NOT HOLD: a zone
that CHECK or shut links cut off from every fixed-head node gets heads near -1e8 x demand and usually does not meet the stop
rule; the constructor refuses a network in which that is so statically, and a scenario in which ``link_closed`` or a speed of 0
causes it is not converged and is dropped by ``valid``, never repaired.  PRV and PSV valves are the matter of THE REGULATING
VALVES below; PBV, FCV and GPV valves, power-rated pumps, controls and rules stay out of scope.  Parity with EPANET is not
claimed and has not been checked.

THE REGULATING VALVES (gatres.h: THE REGULATING VALVES; csrc/k_hydraulic_network.hip; ``_NewtonRef.run_valves``).  A network built
with ``valve_links`` takes the two valves launches: the links launches with a status machine for pressure-reducing (PRV) and
pressure-sustaining (PSV) valves.  A regulating valve is a link from a to b without pipe resistance (r = 0; its length and its
roughness are not read, as for a pump) and with the minor-loss term m of any link (K = 0 is allowed).  It has a kind and a
setting s, a pressure in metres, and one controlled node c: PRV c = b, the downstream end; PSV c = a, the upstream end.  The
target head is hset = elevation[c] + s.  During the Newton loop it carries a status, OPEN, ACTIVE or CLOSED, and starts ACTIVE.
Law by status -- OPEN: the PIPE branch of THE LINK LAW with r = 0 (with the linear floor where g < 1e-7, so K = 0 is a valve
that loses nothing); CLOSED: g = 1e8, h = 1e8 q; ACTIVE: the link is not in the matrix at all.  Assembly: the controlled node of
an ACTIVE valve is a fixed-head row at hset for that iteration -- the identity row that a reservoir's is, its neighbours take
pi * hset on their right-hand side, no off-diagonal is written for it, so the band never widens -- and the valve's present flow
q_v is a fixed draw, -q_v on the right-hand side of row a and +q_v on that of row b wherever that row is not fixed and not
effectively fixed; every sum stays in pipe order.  Flows: after the head solve every link that is not ACTIVE updates as ever;
each ACTIVE valve then takes the flow that closes the mass balance at c over the other links' new flows, added up in pipe order:
PRV q_v = d_c - inflow, PSV q_v = inflow - d_c.  Status: every valve reads the new heads H_a, H_b and its own new q, all valves
from the old statuses at once, with HTOL = 1.524e-4 m and QTOL = 2.8316846592e-6 m3/s (EPANET's 0.0005 ft and 0.0001 cfs) and
hml = m |q| q (``valve_status_ref``):

    PRV ACTIVE   q < -QTOL -> CLOSED; else H_a - hml < hset - HTOL -> OPEN; else ACTIVE
    PRV OPEN     q < -QTOL -> CLOSED; else H_b >= hset + HTOL -> ACTIVE; else OPEN
    PRV CLOSED   H_a >= hset + HTOL and H_b < hset - HTOL -> ACTIVE; else H_a < hset - HTOL and H_a > H_b + HTOL -> OPEN; else CLOSED
    PSV ACTIVE   q < -QTOL -> CLOSED; else H_b + hml > hset + HTOL -> OPEN; else ACTIVE
    PSV OPEN     q < -QTOL -> CLOSED; else H_a < hset - HTOL -> ACTIVE; else OPEN
    PSV CLOSED   H_b > hset + HTOL and H_a > H_b + HTOL -> OPEN; else H_a >= hset + HTOL and H_a > H_b + HTOL -> ACTIVE; else CLOSED

A valve that turns CLOSED gets q = 0.  Stop rule: sum |dq| <= accuracy * sum |q| AND no status changed in this iteration; the dq
of a valve that has just closed is the one from before it was zeroed, the q in the sum the one after.  A valve shut by its
static flag or by ``link_closed`` is a shut link as ever (state 2), and its status machine does not run.  ``link_state`` of a
regulating valve: 0 OPEN, 3 ACTIVE, 4 CLOSED by its own status, 2 shut by input; ``valve_changes`` counts the status changes of
a scenario or step.  In a series with ``warm_start`` the statuses carry over from step to step along with the flows; without it
they start ACTIVE at every step; settings do not follow patterns.  Refused by the constructor (``ValueError``): a valve that is
also a pump or a CHECK link, a controlled node that is a fixed-head node, two regulating valves that share any node, a setting
that is not finite, and the two layouts in which the ACTIVE system is singular -- with all regulating valves removed, the
uncontrolled end of every valve must still reach a fixed-head node (under the walk rules for CHECK and closed links), and every
junction must reach a fixed-head node or the controlled node of some valve.  A scenario that still produces a bad pivot fails.
WHAT DOES NOT HOLD: the valve's flow lags one iteration behind the heads, as in EPANET, so convergence across a valve is linear,
not quadratic.  Statuses can cycle: such a scenario uses all its iterations, is not converged, and is dropped by ``valid``,
never repaired.  An OPEN valve with K = 0 sits on the linear branch, where its flow jitters by 1e-7 m3/s per ulp of the heads
(WHAT DOES NOT HOLD, below) and the stop rule is met by chance: give a valve a loss coefficient where that matters
(``make_hydraulic_network`` does).  Parity with EPANET is not claimed.  FCV, PBV and GPV valves stay out of scope.

THE EMITTERS (gatres.h: THE EMITTERS; csrc/k_hydraulic_network.hip; ``emitter_headloss``, ``_NewtonRef.run_valves(emit=)``).  A
network built with ``emitter_nodes`` takes the two emitters launches: the valves launches with a node term for pressure-dependent
outflow, EPANET's emitter q = C p^gamma -- a leak.  An emitter sits on a junction i; its coefficient C >= 0 (m3/s per m^gamma)
belongs to the scenario (``simulate(emitter_coefficient=)``), the exponent gamma to the network, as in EPANET.  It is a virtual
link from i to the fixed head z_i = elevation[i] with a flow q_e of its own, positive out of the network.  With n = 1 / gamma and
ce = C^(-n) -- forward branch (q_e >= 0): ca = ce q_e^(n-1), g = n ca, h = ca q_e; where g < 1e-7 the linear floor; where g > 1e8
or g is not finite (q_e -> 0 with gamma > 1): g = 1e8, h = 1e8 q_e.  Reverse branch (q_e < 0): a leak takes no water in: g = 1e8,
h = 1e8 q_e, so a junction under negative pressure p carries -|p| / 1e8, as every shut link does.  C == 0 means no emitter in that
scenario or step: its row gets nothing, q_e is +0.0 and it adds nothing to the sums of the stop rule, so a network whose
coefficients are all 0 has every bit of the network without emitters.  Assembly, on the row of i after its links in pipe order:
diag += 1/g, f -= q_e - h/g, f += z_i (1/g); no off-diagonal, so the band never widens.  Flow update after the links':
dq = h/g - (H_i - z_i) (1/g), q_e -= dq; |dq| and |q_e| join the sums of the stop rule after the links, in emitter order.  Start:
q_e = C, the flow at one metre of pressure.  In a series ``emitter_onset`` [Ke] / [S, Ke] keeps emitter k off (C = 0) at the steps
t < onset -- a leak that begins mid-series; with ``warm_start`` an emitter that was on in the step before keeps its q_e, one that
has just switched on starts at C.  Refused by the constructor (``ValueError``; the kernels fail every scenario): gamma that is not
finite and positive, an emitter node outside the network, listed twice, fixed-head, or the controlled node of a regulating valve.
A coefficient that is negative or not finite fails its scenario (a series: from step 0 on, whatever the onset).  WHAT DOES NOT
HOLD: an emitter on a valve's controlled node is refused, not modelled (an ACTIVE valve closes that node's mass balance over the
links alone, and that rule stays as it stands).  Parity with EPANET is not claimed.

THE PRESSURE-DRIVEN DEMAND (gatres.h: THE PRESSURE-DRIVEN DEMAND; csrc/k_hydraulic_network.hip; ``demand_headloss``,
``_NewtonRef.run_valves(pdd=)``).  ``simulate(demand_model="pda", minimum_pressure=, required_pressure=, pressure_exponent=)``
takes the two pdd launches: the emitters launches with EPANET 2.2's PDA as a node term at every junction that draws.  With
dp = Preq - Pmin and n = 1 / exponent, a junction i whose full demand D (in a series: demand x the step's multiplier) is positive
is a virtual link from i to the fixed head z_i = elevation[i] + Pmin with a flow q_d of its own, positive out of the network:
q_d < 0: g = 1e8, h = 1e8 q_d (no demand node feeds the network); 0 <= q_d <= D: g = n dp (q_d / D)^(n-1) / D, h = g q_d / n =
dp (q_d / D)^n, with the linear floor where g < 1e-7 and g = 1e8, h = 1e8 q_d where g > 1e8 or g is not finite; q_d > D: g = 1e8,
h = dp + 1e8 (q_d - D), so a junction above Preq delivers D + (p - Preq) / 1e8, as every shut link leaks.  Junctions with D <= 0
(an inflow included) and fixed-head nodes keep the fixed draw -demand.  Assembly: a pressure-driven row gets no -demand; after its
links in pipe order and after an emitter's term, diag += 1/g, f -= q_d - h/g, f += z_i (1/g); no off-diagonal.  Flow update after
the links' and the emitters': dq = h/g - (H_i - z_i) (1/g), q_d -= dq; |dq| and |q_d| join the sums of the stop rule after the
links and emitters, in node order.  Start: q_d = D; in a series with ``warm_start`` a junction that was pressure-driven in the
step before keeps its q_d.  The controlled node of a regulating valve may be pressure-driven: while the valve is ACTIVE the row
is the identity row, q_d is still updated from the row's head, and the valve's mass balance draws the new q_d.  An emitter and
pressure-driven demand may share a junction.  The result's ``demand_delivered`` holds q_d at pressure-driven junctions, the demand
itself at the others, 0 at fixed-head nodes.  ``demand_model="dda"`` takes the same launch demand-driven: every bit of the
emitters launch.  Refused (``ValueError``; the kernels fail every scenario): pressures that are not finite, dp < 0.1 m (EPANET's
MINPDIFF), an exponent that is not finite and positive with a finite inverse.  Parity with EPANET is not claimed.

THE SERIES (``simulate_series``, ``generate_series_store``; gatres.h: THE SERIES): extended-period simulation, T steps of
``step_seconds`` of one scenario in one launch, one workgroup per series.  Tanks are a subset of the fixed-head nodes: tank k
has its bottom at the node's elevation, a diameter D_k, the area A_k = pi D_k^2 / 4 and level limits min_level[k] <=
max_level[k]; during step t its head is elevation + level[t][k], one fp64 add.  Reservoirs, the other fixed-head nodes, keep
their heads.  Junction n of series s draws demand[s][n] * mult[pattern_of_node[n]][t] at step t (one rounded product).  A step
is the steady solve above; step 0 starts from the starting flows, step t > 0 from the final flows of step t - 1 (``warm_start``,
EPANET's way) or from the starting flows again.  After step t the levels move by explicit Euler, as in EPANET:
inflow_k = the sum over the pipes in pipe order of +q_p where the pipe ends at the tank and -q_p where it starts there, and
level[t + 1][k] = clamp(level[t][k] + (inflow_k * dt) / A_k, min_level[k], max_level[k]), every operation rounded on its own.
A multiplier that is negative or not finite, a non-finite product or tank head, a bad pivot or non-finite sums fail the step and
every later step of the series (NaN outputs, status failed; earlier steps keep theirs); a step that merely does not converge is
no failure and the series goes on from its flows.

WHAT DOES NOT HOLD IN A SERIES: EPANET shortens a time step at the moment a tank becomes full or empty and closes the pipes of
such a tank; this model clamps the level and does neither.  A step after which any level was clamped has status[s][t][3] = 1
(``limited``), and volume is not conserved across such a step; ``series_valid`` and ``generate_series_store`` drop such series
unless told otherwise.  Simple controls are THE CONTROLS below; rule-based controls ([RULES]) stay out of scope.  The limit on
flows that should be zero (below) carries over unchanged: a step with a zero multiplier will not meet the stop rule.

THE CONTROLS (``control_table``, ``simulate_series(controls=)``, ``generate_series_store(controls=)``; gatres.h: THE CONTROLS):
EPANET's simple controls in a series, ``gatres_hydraulic_series_controls`` -- the pdd launch with a table of Kc >= 0 controls whose
order matters.  Control k holds link[k]; action[k] (OPEN 0, CLOSED 1, SETTING 2); value[k], read for SETTING only (on a pump the
base speed in place of pump_speed[s][k'], still multiplied by the step's speed multiplier; on a PRV or PSV the setting in metres
in place of valve_setting[s][k']); kind[k] (TANK_BELOW 0, TANK_ABOVE 1, NODE_BELOW 2, NODE_ABOVE 3, AT_STEP 4); target[k] (a tank
index, a junction's node index, a step index); threshold [Kc] or [S, Kc] (a level in metres above the tank's bottom, a pressure
in metres; not read for AT_STEP).  EVALUATION at the start of step t, before the step's inputs are formed: TANK_BELOW
level[t][target] <= threshold, TANK_ABOVE >= (the level the step starts with, so at t = 0 too); NODE_BELOW / NODE_ABOVE
H - elevation of the solution of step t - 1 <= / >= threshold, not at t = 0, whether or not step t - 1 converged; AT_STEP
t == target (a target of T or more never fires).  Every control whose condition holds applies its action, in table order: the
last one wins.  Controls are level-triggered, as in EPANET.  STATE per link, reset at the start of every series and kept until a
control changes it: ctl in {none, open, closed} and an override with a presence flag; OPEN sets ctl = open, CLOSED ctl = closed,
SETTING stores the override and sets ctl = open.  A control that fires has changed its link when ctl, the flag or the bits of the
override differ from what they were; ``control_changes`` [S, T] counts these per step.  EFFECT: a link is shut by input when
ctl == closed, or when ctl == none and the static CLOSED flag or the ``link_closed`` byte says so; ctl == open overrides both.  A
pump with w == 0 is still shut: a SETTING of 0 switches it off, OPEN gives a pump with base speed 0 no speed.  ``link_state`` 2
reads "shut by input, by w == 0 or by a control".  A link a control has touched (ctl != none) that was shut in step t - 1 and is
not in step t starts step t at q_start, warm or cold; its regulating valve starts the step ACTIVE, even warm, when a control
changed the link at step t or it was shut in step t - 1 (``control_start_ref``).  A link no control has touched behaves as in the
pdd launch, which an empty table gives bit for bit.  REFUSED (``control_table`` raises ``ValueError``; the kernel fails every
series): a link outside [0, P), an unknown action or kind, a control on a CHECK pipe that is no pump, SETTING on a link that is
neither a pump nor a PRV / PSV, a SETTING that is not finite or negative on a pump, a tank index outside [0, K), a node outside
the network or with a fixed head, a negative step.  A threshold that is not finite fails its series from step 0 on.  WHAT DOES
NOT HOLD: EPANET shortens a time step so that a level control fires when the level is reached; here levels are read at step
starts, so a level overshoots its threshold by up to |inflow| dt / A.  EPANET's volume tolerance on level controls is not
modelled.  A control that cuts a zone off from every fixed-head node gives a step that does not converge (``series_valid`` drops
it, as with ``link_closed``).  [RULES] and controls on pipe settings (TCV loss, FCV and the like) stay out.  Parity with EPANET
is not claimed.

WHAT DOES NOT HOLD: flows that should be zero do not come to rest on the linear branch.  A head of 100 m resolves 1.4e-14 m
in fp64, and on the linear branch a head difference becomes a flow with 1 / g = 1e7: one ulp between two neighbours is
1e-7 m3/s, which is off the linear branch again (it ends near 1e-12 m3/s).  Such flows jitter at 1e-7 .. 1e-6 m3/s from one
iteration to the next, and each adds its jitter to sum |dq|.  A scenario with zero demand everywhere never meets the stop
rule (all iterations used, ``converged`` False, heads right to 1e-7 m), and one in which many pipes carry next to nothing --
dead ends without demand -- may not meet it either once their jitter exceeds accuracy * sum |q|: measured, the 388-node
network with three reservoirs and zero demand (0.04 m3/s between the reservoirs) does not converge in 40 iterations.
``generate_store`` counts such scenarios as not_converged and drops them; give every junction a demand range above zero, as
the default does not (``DEMAND_RANGE`` starts at 0: its draws are positive with probability 1 - 2^-53 per junction, and of
the order of the upper end).

Host restatements in numpy fp64 (the yardsticks of the tests): ``pipe_headloss``, ``solve_ref``, ``hydraulic_residuals``,
``hydraulic_draws``, ``tree_solution``, ``simulate_series_ref``, ``level_update_ref``, ``series_valid_ref``,
``series_volume_balance``, ``link_headloss``, ``link_state_ref``, ``hydraulic_link_draws``, ``pump_curve_from_points``,
``valve_status_ref``, ``hydraulic_valve_draws``, ``emitter_headloss``, ``hydraulic_emitter_draws``, ``demand_headloss``,
``control_step_ref`` and ``control_start_ref``.
"""
from __future__ import annotations

from collections import namedtuple
from typing import Dict, Sequence, Tuple

import numpy as np
import torch

from . import _native
from .snapshot_store import SnapshotStore

HW_EXPONENT = 1.852
HW_FACTOR = 10.667
HW_DIAMETER_EXPONENT = 4.871
LINEAR_GRADIENT = 1e-7                  # the law at low flow
SHUT_GRADIENT = 1e8                     # the gradient of a shut link and of a CHECK link's reverse branch
GRAVITY = 9.80665                       # m/s2, in m = 8 K / (pi^2 g D^4)
LINK_PIPE, LINK_PUMP = 0, 1             # GATRES_HYD_PIPE, GATRES_HYD_PUMP
LINK_CHECK, LINK_CLOSED = 1, 2          # GATRES_HYD_LINK_CHECK, GATRES_HYD_LINK_CLOSED
START_VELOCITY = 0.3048                 # m/s: 1 ft/s, EPANET's starting flows
ACCURACY = 1e-6
MAX_ITER = 40
HYD_STATUS = _native.HYD_STATUS         # GATRES_HYD_STATUS: iterations, converged, failed, 0
LDS_BUDGET = _native.HYD_LDS_BUDGET     # GATRES_HYD_LDS_BUDGET
GRID_CAP = _native.HYD_GRID_CAP         # GATRES_HYD_GRID_CAP

# the ranges of the reference's scenario generator for C-Town (configs/v7.1: pipe, junction and reservoir sections), SI units
ROUGHNESS_RANGE = (60.128711911111104, 139.0834768)
DIAMETER_RANGE = (0.051, 0.61)
LENGTH_RANGE = (4.3, 1280.3)
ELEVATION_RANGE = (3.48, 113.08)
HEAD_RANGE = (60.0, 126.21526763089759)
DEMAND_RANGE = (0.0, 1e-4)
TANK_DIAMETER_RANGE = (7.140000000000001, 31.3)       # (the tank section of the same file)
TANK_LEVEL_RANGE = (0.0, 4.940000000000007)
LEVEL_SEED_OFFSET = 0x74616E6B          # generate_series_store draws the initial levels with seed + this, mod 2^64

HydraulicResult = namedtuple("HydraulicResult", "pressure head flow iterations converged failed status final_dq")
HydraulicReference = namedtuple("HydraulicReference", "head flow iterations converged failed final_dq")
HydraulicSeriesResult = namedtuple("HydraulicSeriesResult", "pressure head flow level iterations converged failed limited status final_dq")
HydraulicSeriesReference = namedtuple("HydraulicSeriesReference", "head flow level iterations converged failed limited final_dq")
# what a network with special links returns: the fields above, and link_state
HydraulicLinksResult = namedtuple("HydraulicLinksResult", HydraulicResult._fields + ("link_state",))
HydraulicLinksReference = namedtuple("HydraulicLinksReference", HydraulicReference._fields + ("link_state",))
HydraulicSeriesLinksResult = namedtuple("HydraulicSeriesLinksResult", HydraulicSeriesResult._fields + ("link_state",))
HydraulicSeriesLinksReference = namedtuple("HydraulicSeriesLinksReference", HydraulicSeriesReference._fields + ("link_state",))
# what a network with regulating valves returns: the fields above, and valve_changes (status changes per scenario or step)
HydraulicValvesResult = namedtuple("HydraulicValvesResult", HydraulicLinksResult._fields + ("valve_changes",))
HydraulicValvesReference = namedtuple("HydraulicValvesReference", HydraulicLinksReference._fields + ("valve_changes", "margin"))
HydraulicSeriesValvesResult = namedtuple("HydraulicSeriesValvesResult", HydraulicSeriesLinksResult._fields + ("valve_changes",))
HydraulicSeriesValvesReference = namedtuple("HydraulicSeriesValvesReference",
                                            HydraulicSeriesLinksReference._fields + ("valve_changes", "margin"))
# what ``HydraulicNetwork.sensitivity`` and ``localize_leaks`` return (gatres.h: THE SENSITIVITIES); every field a device tensor
HydraulicSensitivityResult = namedtuple("HydraulicSensitivityResult", HydraulicLinksResult._fields + ("dh_ddemand", "dh_droughness"))
LeakLocalization = namedtuple("LeakLocalization", "score leak_flow best residual pressure status dh_ddemand")
HydraulicSensitivityReference = namedtuple("HydraulicSensitivityReference", "dh_ddemand dh_droughness")
LINK_PRV, LINK_PSV = 2, 3               # GATRES_HYD_PRV, GATRES_HYD_PSV
VALVE_OPEN, VALVE_ACTIVE, VALVE_CLOSED = 0, 3, 4      # link_state of a regulating valve (2: shut by input)
VALVE_HTOL, VALVE_QTOL = 1.524e-4, 2.8316846592e-6    # EPANET's 0.0005 ft and 0.0001 cfs
VALVE_KINDS = {"PRV": LINK_PRV, "PSV": LINK_PSV}
# what a network with emitters returns: the fields above, and emitter_flow (m3/s out of the network, per scenario or step and emitter)
HydraulicEmittersResult = namedtuple("HydraulicEmittersResult", HydraulicValvesResult._fields + ("emitter_flow",))
HydraulicEmittersReference = namedtuple("HydraulicEmittersReference", HydraulicValvesReference._fields + ("emitter_flow",))
HydraulicSeriesEmittersResult = namedtuple("HydraulicSeriesEmittersResult", HydraulicSeriesValvesResult._fields + ("emitter_flow",))
HydraulicSeriesEmittersReference = namedtuple("HydraulicSeriesEmittersReference",
                                              HydraulicSeriesValvesReference._fields + ("emitter_flow",))
EMITTER_EXPONENT = 0.5                  # EPANET's default


def emitter_headloss(q, coefficient, exponent=EMITTER_EXPONENT) -> Tuple[np.ndarray, np.ndarray]:
    """THE EMITTERS, elementwise with the kernel's operations: head loss h and gradient g of an emitter with coefficient C > 0 and
    exponent gamma at its flow q (positive out of the network).  n = 1 / gamma, ce = C^(-n).  Forward (q >= 0): ca = ce q^(n - 1),
    g = n ca, h = ca q; the linear floor where g < 1e-7; g = 1e8, h = 1e8 q where g > 1e8 or g is not finite.  Reverse (q < 0):
    g = 1e8, h = 1e8 q.  (C == 0 is no emitter and has no law: the callers leave such an emitter out.)"""
    q, C = np.asarray(q, dtype=np.float64), np.asarray(coefficient, dtype=np.float64)
    n = 1.0 / np.float64(exponent)
    with np.errstate(all="ignore"):
        ce = np.power(C, -n)
        ca = ce * np.power(np.maximum(q, 0.0), n - 1.0)
        g, h = n * ca, ca * q
        low = g < LINEAR_GRADIENT
        high = ~low & ~(g <= SHUT_GRADIENT)
        g = np.where(low, LINEAR_GRADIENT, np.where(high, SHUT_GRADIENT, g))
        h = np.where(low, LINEAR_GRADIENT * q, np.where(high, SHUT_GRADIENT * q, h))
        reverse = q < 0
        g = np.where(reverse, SHUT_GRADIENT, g)
        h = np.where(reverse, SHUT_GRADIENT * q, h)
    return h, g


# what a launch with a demand model returns: the fields above, and demand_delivered (m3/s out of the network, per scenario or step
# and node: q_d at a pressure-driven junction, the demand itself at another junction, 0 at a fixed-head node)
HydraulicPddResult = namedtuple("HydraulicPddResult", HydraulicEmittersResult._fields + ("demand_delivered",))
HydraulicPddReference = namedtuple("HydraulicPddReference", HydraulicEmittersReference._fields + ("demand_delivered",))
HydraulicSeriesPddResult = namedtuple("HydraulicSeriesPddResult", HydraulicSeriesEmittersResult._fields + ("demand_delivered",))
HydraulicSeriesPddReference = namedtuple("HydraulicSeriesPddReference",
                                         HydraulicSeriesEmittersReference._fields + ("demand_delivered",))
PRESSURE_EXPONENT = 0.5                 # EPANET's default
MIN_PRESSURE_DIFFERENCE = 0.1           # EPANET's MINPDIFF, in metres here
DEMAND_MODELS = {"dda": 0, "pda": 1}    # demand_model of the two pdd launches


def demand_headloss(q, D, dp, exponent=PRESSURE_EXPONENT) -> Tuple[np.ndarray, np.ndarray]:
    """THE PRESSURE-DRIVEN DEMAND, elementwise with the kernel's operations: head loss h and gradient g of the virtual link of a
    junction with full demand D > 0 at its delivered flow q (positive out of the network), dp = Preq - Pmin, n = 1 / exponent.
    q < 0: g = 1e8, h = 1e8 q.  0 <= q <= D: g = n dp (q / D)^(n - 1) / D, h = g q / n; the linear floor where g < 1e-7;
    g = 1e8, h = 1e8 q where g > 1e8 or g is not finite.  q > D: g = 1e8, h = dp + 1e8 (q - D)."""
    q, D = np.asarray(q, dtype=np.float64), np.asarray(D, dtype=np.float64)
    dp, n = np.float64(dp), 1.0 / np.float64(exponent)
    with np.errstate(all="ignore"):
        g = ((n * dp) * np.power(np.maximum(q, 0.0) / D, n - 1.0)) / D
        h = (g * q) / n
        low = g < LINEAR_GRADIENT
        high = ~low & ~(g <= SHUT_GRADIENT)
        g = np.where(low, LINEAR_GRADIENT, np.where(high, SHUT_GRADIENT, g))
        h = np.where(low, LINEAR_GRADIENT * q, np.where(high, SHUT_GRADIENT * q, h))
        above, reverse = q > D, q < 0
        g = np.where(above | reverse, SHUT_GRADIENT, g)
        h = np.where(above, dp + SHUT_GRADIENT * (q - D), np.where(reverse, SHUT_GRADIENT * q, h))
    return h, g


def pdd_arguments(demand_model, minimum_pressure=0.0, required_pressure=None, pressure_exponent=PRESSURE_EXPONENT):
    """None without a demand model, else the four scalars of the pdd launches: (demand_model, Pmin, Preq, exponent).  Refused with
    ``ValueError``: a model other than "pda" / "dda", "pda" without ``required_pressure``, pressures that are not finite,
    Preq - Pmin below 0.1 m, an exponent that is not finite and positive with a finite inverse; and, without a model, any of the
    three scalars set.  With "dda" the three scalars are not read (an input file's may be handed on as they are)."""
    given = required_pressure is not None or float(minimum_pressure) != 0.0 or float(pressure_exponent) != PRESSURE_EXPONENT
    if demand_model is None:
        if given:
            raise ValueError("minimum_pressure, required_pressure and pressure_exponent need demand_model='pda'")
        return None
    if demand_model not in DEMAND_MODELS:
        raise ValueError("demand_model must be None, 'pda' or 'dda'")
    if demand_model == "dda":
        return (0, 0.0, 0.0, PRESSURE_EXPONENT)
    if required_pressure is None:
        raise ValueError("demand_model='pda' needs required_pressure")
    pmin, preq, e = float(minimum_pressure), float(required_pressure), float(pressure_exponent)
    if not (np.isfinite(pmin) and np.isfinite(preq)):
        raise ValueError("minimum_pressure and required_pressure must be finite")
    if not preq - pmin >= MIN_PRESSURE_DIFFERENCE:
        raise ValueError(f"required_pressure must exceed minimum_pressure by at least {MIN_PRESSURE_DIFFERENCE} m")
    with np.errstate(all="ignore"):
        if not (np.isfinite(e) and e > 0 and np.isfinite(np.float64(1.0) / np.float64(e))):
            raise ValueError("pressure_exponent must be finite and positive")
    return (1, pmin, preq, e)


def _pdd_keywords(demand_model, minimum_pressure, required_pressure, pressure_exponent) -> dict:
    """What the store generators hand to ``simulate``: nothing without a demand model (the call it always was)."""
    if pdd_arguments(demand_model, minimum_pressure, required_pressure, pressure_exponent) is None:
        return {}
    return dict(demand_model=demand_model, minimum_pressure=minimum_pressure, required_pressure=required_pressure,
                pressure_exponent=pressure_exponent)


def pdd_lds_bytes(num_nodes: int, num_pipes: int, half_bandwidth: int, num_pumps: int, num_valves: int, num_emitters: int,
                  demand_model: int = 1) -> int:
    """What a workgroup of ``gatres_hydraulic_solve_pdd`` takes of the LDS (gatres.h states the same sum): the arrays of the
    emitters launch and, with demand_model 1, per node D, q_d, 1 / g and h / g."""
    return emitters_lds_bytes(num_nodes, num_pipes, half_bandwidth, num_pumps, num_valves, num_emitters) + \
        (32 * num_nodes if demand_model else 0)


def series_pdd_lds_bytes(num_nodes: int, num_pipes: int, half_bandwidth: int, num_tanks: int, num_pumps: int, num_valves: int,
                         num_emitters: int, demand_model: int = 1) -> int:
    """What a workgroup of ``gatres_hydraulic_series_pdd`` takes of the LDS (gatres.h states the same sum)."""
    return series_emitters_lds_bytes(num_nodes, num_pipes, half_bandwidth, num_tanks, num_pumps, num_valves, num_emitters) + \
        (32 * num_nodes if demand_model else 0)


def emitters_lds_bytes(num_nodes: int, num_pipes: int, half_bandwidth: int, num_pumps: int, num_valves: int, num_emitters: int) -> int:
    """What a workgroup of ``gatres_hydraulic_solve_emitters`` takes of the LDS (gatres.h states the same sum): the arrays of the
    valves launch, and per emitter ce, z, q_e, 1 / g, h / g, its row and its node."""
    return valves_lds_bytes(num_nodes, num_pipes, half_bandwidth, num_pumps, num_valves) + 48 * num_emitters


def series_emitters_lds_bytes(num_nodes: int, num_pipes: int, half_bandwidth: int, num_tanks: int, num_pumps: int, num_valves: int,
                              num_emitters: int) -> int:
    """What a workgroup of ``gatres_hydraulic_series_emitters`` takes of the LDS (gatres.h states the same sum)."""
    return series_valves_lds_bytes(num_nodes, num_pipes, half_bandwidth, num_tanks, num_pumps, num_valves) + 48 * num_emitters


# ---- THE CONTROLS (gatres.h): EPANET's simple controls in a series ---------------------------------------------------------------
CONTROL_ACTIONS = {"open": 0, "closed": 1, "setting": 2}            # GATRES_HYD_CTL_OPEN, _CLOSED, _SETTING
CONTROL_KINDS = {"tank_below": 0, "tank_above": 1, "node_below": 2, "node_above": 3, "at_step": 4}      # GATRES_HYD_CTL_TANK_BELOW ..
CTL_NONE, CTL_OPEN, CTL_CLOSED = 0, 1, 2                            # a link's control state
# what a series with controls returns: the fields of the pdd launch, and control_changes (int32 [S, T])
HydraulicSeriesControlsResult = namedtuple("HydraulicSeriesControlsResult", HydraulicSeriesPddResult._fields + ("control_changes",))
HydraulicSeriesControlsReference = namedtuple("HydraulicSeriesControlsReference",
                                              HydraulicSeriesPddReference._fields + ("control_changes",))


class ControlTable:
    """THE TABLE of THE CONTROLS: ``link`` int32, ``action`` uint8 (``CONTROL_ACTIONS``), ``value`` fp64 (read for a setting),
    ``kind`` uint8 (``CONTROL_KINDS``), ``target`` int32 and ``threshold`` fp64, each [Kc], in the order that decides which control
    wins.  A plain record: ``control_table`` is what checks one against a network."""
    ACTIONS, KINDS = CONTROL_ACTIONS, CONTROL_KINDS

    def __init__(self, link, action, value, kind, target, threshold):
        self.link = np.ascontiguousarray(link, dtype=np.int32).reshape(-1)
        Kc = self.link.size
        self.action = np.ascontiguousarray(action, dtype=np.uint8).reshape(Kc)
        self.value = np.ascontiguousarray(value, dtype=np.float64).reshape(Kc)
        self.kind = np.ascontiguousarray(kind, dtype=np.uint8).reshape(Kc)
        self.target = np.ascontiguousarray(target, dtype=np.int32).reshape(Kc)
        self.threshold = np.ascontiguousarray(threshold, dtype=np.float64).reshape(Kc)

    def __len__(self) -> int:
        return int(self.link.size)

    @property
    def num_controls(self) -> int:
        return int(self.link.size)


def control_table(network: "HydraulicNetwork", controls, step_seconds=None) -> ControlTable:
    """The ``ControlTable`` of ``controls`` on ``network``: a sequence of tuples (link, action, kind, target[, threshold]) such as
    ``(link, "closed", "tank_above", tank, 4.5)``, ``(link, ("setting", 0.8), "at_step", 12)`` and
    ``(link, "open", "node_below", node, 20.0)``.  ``action`` is "open", "closed" or ("setting", value); ``kind`` one of
    ``CONTROL_KINDS``, or "at_time" with a target in seconds, which ``step_seconds`` turns into a step (a time that is no whole
    number of steps is refused).  A ``ControlTable`` is checked as it is.  ``ValueError``, naming the control, for everything THE
    CONTROLS refuse: a link outside [0, P), an unknown action or kind, a control on a CHECK pipe that is no pump, a setting on a link
    that is neither a pump nor a PRV / PSV, a setting that is not finite or is negative on a pump, a tank index outside [0, K), a
    node outside the network or with a fixed head, a negative step."""
    P, N, K = network.num_pipes, network.num_nodes, network.num_tanks
    if isinstance(controls, ControlTable):
        rows = [(int(controls.link[k]), int(controls.action[k]), float(controls.value[k]), int(controls.kind[k]),
                 int(controls.target[k]), float(controls.threshold[k])) for k in range(len(controls))]
    else:
        rows = []
        for k, c in enumerate(controls):
            if len(c) not in (4, 5):
                raise ValueError(f"control {k}: expected (link, action, kind, target[, threshold]), got {c!r}")
            link, action, kind, target = c[:4]
            value = 0.0
            if isinstance(action, (tuple, list)):
                if len(action) != 2:
                    raise ValueError(f"control {k}: a setting is ('setting', value), got {action!r}")
                action, value = action[0], float(action[1])
            if action not in CONTROL_ACTIONS:
                raise ValueError(f"control {k}: unknown action {action!r}")
            if kind == "at_time":
                if step_seconds is None:
                    raise ValueError(f"control {k}: 'at_time' needs step_seconds")
                steps = float(target) / float(step_seconds)
                if not (np.isfinite(steps) and steps == np.floor(steps)):
                    raise ValueError(f"control {k}: the time {target} s is no whole number of steps of {step_seconds} s")
                kind, target = "at_step", int(steps)
            if kind not in CONTROL_KINDS:
                raise ValueError(f"control {k}: unknown kind {kind!r}")
            if CONTROL_KINDS[kind] != CONTROL_KINDS["at_step"] and len(c) != 5:
                raise ValueError(f"control {k}: a {kind} control needs a threshold")
            if int(target) != target:
                raise ValueError(f"control {k}: the target {target!r} is no index")
            rows.append((int(link), CONTROL_ACTIONS[action], value, CONTROL_KINDS[kind], int(target),
                         float(c[4]) if len(c) == 5 else 0.0))
    for k, (link, action, value, kind, target, _thr) in enumerate(rows):
        if not 0 <= link < P:
            raise ValueError(f"control {k}: link {link} is outside [0, {P})")
        if action not in CONTROL_ACTIONS.values():
            raise ValueError(f"control {k}: unknown action {action}")
        if kind not in CONTROL_KINDS.values():
            raise ValueError(f"control {k}: unknown kind {kind}")
        pump, valve = bool(network.is_pump[link]), bool(network.is_valve[link])
        if network.check_valve[link] and not pump:
            raise ValueError(f"control {k}: link {link} is a CHECK pipe, which takes no control")
        if action == CONTROL_ACTIONS["setting"]:
            if not (pump or valve):
                raise ValueError(f"control {k}: link {link} is neither a pump nor a PRV / PSV and takes no setting")
            if not np.isfinite(value) or (pump and value < 0):
                raise ValueError(f"control {k}: the setting {value} of link {link} is not finite or is negative on a pump")
        if target < 0:
            raise ValueError(f"control {k}: the target {target} is negative")
        if kind <= CONTROL_KINDS["tank_above"]:
            if target >= K:
                raise ValueError(f"control {k}: tank {target} is outside [0, {K})")
        elif kind <= CONTROL_KINDS["node_above"]:
            if target >= N:
                raise ValueError(f"control {k}: node {target} is outside the network")
            if network.fixed[target]:
                raise ValueError(f"control {k}: node {target} is a fixed-head node")
    cols = list(zip(*rows)) if rows else [[]] * 6
    return ControlTable(*cols)


def series_controls_lds_bytes(num_nodes: int, num_pipes: int, half_bandwidth: int, num_tanks: int, num_pumps: int, num_valves: int,
                              num_emitters: int, demand_model: int = 1) -> int:
    """What a workgroup of ``gatres_hydraulic_series_controls`` takes of the LDS (gatres.h states the same sum): the bytes of
    ``gatres_hydraulic_series_pdd`` and 12 P + 16, per link the override and the state word and the four waves' change counts."""
    return series_pdd_lds_bytes(num_nodes, num_pipes, half_bandwidth, num_tanks, num_pumps, num_valves, num_emitters,
                                demand_model) + 12 * num_pipes + 16


def control_state(num_links: int) -> dict:
    """The control state of the links at the start of a series: ``ctl`` [P] (``CTL_NONE``), ``has_value`` [P] False, ``value``
    [P] 0, and ``changed`` [P], whether a control changed the link in the step last evaluated."""
    return {"ctl": np.zeros(num_links, dtype=np.int8), "has_value": np.zeros(num_links, dtype=bool),
            "value": np.zeros(num_links, dtype=np.float64), "changed": np.zeros(num_links, dtype=bool)}


def control_step_ref(table: ControlTable, threshold, state: dict, level, pressure_prev, t: int) -> Tuple[dict, int]:
    """THE CONTROLS at the start of step ``t``, as a plain loop over the table in its order: ``threshold`` [Kc], ``state`` as
    ``control_state`` leaves it or as the step before returned it, ``level`` [K] the levels the step starts with,
    ``pressure_prev`` [N] head - elevation of step t - 1 (not read at t = 0).  Returns (the new state, the number of controls that
    changed their link: its ctl, the presence of an override or the bits of the override)."""
    thr = np.asarray(threshold, dtype=np.float64)
    st = {k: v.copy() for k, v in state.items()}
    st["changed"][:] = False
    changes = 0
    for k in range(len(table)):
        kind, target, p = int(table.kind[k]), int(table.target[k]), int(table.link[k])
        if kind == CONTROL_KINDS["at_step"]:
            fire = t == target
        elif kind == CONTROL_KINDS["tank_below"]:
            fire = bool(level[target] <= thr[k])
        elif kind == CONTROL_KINDS["tank_above"]:
            fire = bool(level[target] >= thr[k])
        elif t == 0:
            fire = False
        elif kind == CONTROL_KINDS["node_below"]:
            fire = bool(pressure_prev[target] <= thr[k])
        else:
            fire = bool(pressure_prev[target] >= thr[k])
        if not fire:
            continue
        action = int(table.action[k])
        ctl = CTL_CLOSED if action == CONTROL_ACTIONS["closed"] else CTL_OPEN
        has, val = bool(st["has_value"][p]), st["value"][p]
        if action == CONTROL_ACTIONS["setting"]:
            has, val = True, table.value[k]
        if ctl != st["ctl"][p] or has != st["has_value"][p] or np.float64(val).tobytes() != np.float64(st["value"][p]).tobytes():
            st["ctl"][p], st["has_value"][p], st["value"][p] = ctl, has, val
            st["changed"][p] = True
            changes += 1
    return st, changes


def control_start_ref(state: dict, was_shut, t: int) -> Tuple[np.ndarray, np.ndarray]:
    """The start rules of THE CONTROLS at step ``t``, per link [P]: (starts at q_start -- a link a control has touched that was shut
    in step t - 1; it starts at 0 instead where it is still shut --, its regulating valve starts ACTIVE -- such a link that a
    control changed at step t or that was shut in step t - 1).  Nothing at t = 0."""
    touched = (state["ctl"] != CTL_NONE) & (t > 0)
    was_shut = np.asarray(was_shut, dtype=bool)
    return touched & was_shut, touched & (state["changed"] | was_shut)


def _control_inputs(network, controls, control_threshold, S: int, step_seconds=None):
    """(table, thresholds [S, Kc]) of a call with ``controls``."""
    table = controls if isinstance(controls, ControlTable) else control_table(network, controls, step_seconds)
    Kc = len(table)
    thr = table.threshold if control_threshold is None else np.asarray(control_threshold, dtype=np.float64)
    if thr.shape not in ((Kc,), (S, Kc)):
        raise ValueError(f"control_threshold must be [{Kc}] or [{S}, {Kc}]")
    return table, np.broadcast_to(thr, (S, Kc))


def _valve_rule(psv: bool, status: int, Ha: float, Hb: float, q: float, hml: float, hset: float):
    """One valve's next status by the six rules, and how far the comparisons it made were from their thresholds: (status,
    margin in metres, margin in m3/s); a margin is +inf where no comparison of its kind was made."""
    mh, mq = [np.inf], [np.inf]

    def lt(x, y, m=mh):                                     # x < y, recorded
        m[0] = min(m[0], abs(x - y))
        return x < y

    ge = lambda x, y: not lt(x, y)
    gt = lambda x, y: lt(y, x)
    lo, hi = hset - VALVE_HTOL, hset + VALVE_HTOL
    if status != VALVE_CLOSED:
        if lt(q, -VALVE_QTOL, mq):
            return VALVE_CLOSED, mh[0], mq[0]
        if not psv:
            if status == VALVE_ACTIVE:
                ns = VALVE_OPEN if lt(Ha - hml, lo) else VALVE_ACTIVE
            else:
                ns = VALVE_ACTIVE if ge(Hb, hi) else VALVE_OPEN
        elif status == VALVE_ACTIVE:
            ns = VALVE_OPEN if gt(Hb + hml, hi) else VALVE_ACTIVE
        else:
            ns = VALVE_ACTIVE if lt(Ha, lo) else VALVE_OPEN
    elif not psv:
        if ge(Ha, hi) and lt(Hb, lo):
            ns = VALVE_ACTIVE
        elif lt(Ha, lo) and gt(Ha, Hb + VALVE_HTOL):
            ns = VALVE_OPEN
        else:
            ns = VALVE_CLOSED
    else:
        if gt(Hb, hi) and gt(Ha, Hb + VALVE_HTOL):
            ns = VALVE_OPEN
        elif ge(Ha, hi) and gt(Ha, Hb + VALVE_HTOL):
            ns = VALVE_ACTIVE
        else:
            ns = VALVE_CLOSED
    return ns, mh[0], mq[0]


def valve_status_ref(kind, status, head_a, head_b, q, minor, hset) -> np.ndarray:
    """THE REGULATING VALVES, the six status rules, elementwise: the next status (``VALVE_OPEN``, ``VALVE_ACTIVE``,
    ``VALVE_CLOSED``) of valves of ``kind`` ("PRV" / "PSV" or ``LINK_PRV`` / ``LINK_PSV``) at ``status`` from the new heads at their
    ends, their own new flow, their minor-loss term m (hml = (m |q|) q) and their target head."""
    kinds = np.array([VALVE_KINDS.get(k, k) for k in np.atleast_1d(kind)])
    args = np.broadcast_arrays(kinds, *[np.asarray(v, dtype=np.float64) for v in (status, head_a, head_b, q, minor, hset)])
    out = np.empty(args[0].shape, dtype=np.uint8)
    for i in np.ndindex(out.shape):
        k, st, ha, hb, qv, m, hs = (a[i] for a in args)
        if k not in (LINK_PRV, LINK_PSV) or int(st) not in (VALVE_OPEN, VALVE_ACTIVE, VALVE_CLOSED):
            raise ValueError("valve_status_ref takes kinds PRV / PSV and statuses OPEN, ACTIVE, CLOSED")
        out[i] = _valve_rule(k == LINK_PSV, int(st), float(ha), float(hb), float(qv), (float(m) * abs(float(qv))) * float(qv), float(hs))[0]
    return out


def valves_lds_bytes(num_nodes: int, num_pipes: int, half_bandwidth: int, num_pumps: int, num_valves: int) -> int:
    """What a workgroup of ``gatres_hydraulic_solve_valves`` takes of the LDS (gatres.h states the same sum): the arrays of the
    links launch, and per valve hset, its link, the row and the node of c and a change flag."""
    return links_lds_bytes(num_nodes, num_pipes, half_bandwidth, num_pumps) + 24 * num_valves


def series_valves_lds_bytes(num_nodes: int, num_pipes: int, half_bandwidth: int, num_tanks: int, num_pumps: int, num_valves: int) -> int:
    """What a workgroup of ``gatres_hydraulic_series_valves`` takes of the LDS (gatres.h states the same sum)."""
    return series_links_lds_bytes(num_nodes, num_pipes, half_bandwidth, num_tanks, num_pumps) + 24 * num_valves


def pipe_headloss(q, r) -> Tuple[np.ndarray, np.ndarray]:
    """THE LAW: head loss h and its gradient g at the flow q for the resistance r, with EPANET's rule at low flow."""
    q = np.asarray(q, dtype=np.float64)
    r = np.asarray(r, dtype=np.float64)
    ra = r * np.power(np.abs(q), 0.852)
    g = 1.852 * ra
    h = ra * q
    low = g < LINEAR_GRADIENT
    g = np.where(low, LINEAR_GRADIENT, g)
    h = np.where(low, LINEAR_GRADIENT * q, h)
    return h, g


def link_headloss(q, r, minor=0.0, pump=False, check=False, shut=False, h0=0.0, rp=1.0, n=1.0, speed=1.0) -> Tuple[np.ndarray, np.ndarray]:
    """THE LINK LAW, elementwise with the kernel's operations: head loss h and gradient g at the flow q of a link with resistance
    r and minor-loss term ``minor`` (m, not K); ``pump`` links have (h0, rp, n) and run at ``speed``; ``check`` links (every pump
    is one) take the reverse branch at q < 0; ``shut`` links, and pumps at speed 0, are closed.  With the defaults it is
    ``pipe_headloss`` in every bit."""
    q, r, minor = np.asarray(q, dtype=np.float64), np.asarray(r, dtype=np.float64), np.asarray(minor, dtype=np.float64)
    pump, check, shut = np.asarray(pump, dtype=bool), np.asarray(check, dtype=bool), np.asarray(shut, dtype=bool)
    h0, rp, n, w = (np.asarray(v, dtype=np.float64) for v in (h0, rp, n, speed))
    with np.errstate(all="ignore"):
        aq = np.abs(q)
        ra, ma = r * np.power(aq, 0.852), minor * aq
        g = 1.852 * ra + 2.0 * ma
        h = (ra + ma) * q
        w2, w2n = w * w, np.where(w > 0, np.power(np.where(w > 0, w, 1.0), 2.0 - n), 0.0)
        ca = (w2n * rp) * np.power(np.maximum(q, 0.0), n - 1.0)
        g = np.where(pump, n * ca, g)
        h = np.where(pump, ca * q, h)
        low = g < LINEAR_GRADIENT
        g = np.where(low, LINEAR_GRADIENT, g)
        h = np.where(low, LINEAR_GRADIENT * q, h)
        lift = np.where(pump, w2 * h0, 0.0)
        h = h - lift
        reverse = (check | pump) & (q < 0)
        g = np.where(reverse, SHUT_GRADIENT, g)
        h = np.where(reverse, SHUT_GRADIENT * q - lift, h)
        closed = shut | (pump & (w == 0))
        g = np.where(closed, SHUT_GRADIENT, g)
        h = np.where(closed, SHUT_GRADIENT * q, h)
    return h, g


def link_state_ref(q, pump=False, check=False, shut=False, speed=1.0, valve_status=None) -> np.ndarray:
    """``link_state`` of gatres.h at the flows q: 0 forward, 1 a CHECK link on its reverse branch, 2 shut.  ``valve_status``: per
    link, the status of a regulating valve (0 OPEN, 3 ACTIVE, 4 CLOSED) and -1 where the link is none; a valve that its input
    shuts is 2 like any link."""
    q, pump = np.asarray(q, dtype=np.float64), np.asarray(pump, dtype=bool)
    closed = np.asarray(shut, dtype=bool) | (pump & (np.asarray(speed, dtype=np.float64) == 0))
    reverse = (np.asarray(check, dtype=bool) | pump) & (q < 0)
    state = np.where(reverse, 1, 0)
    if valve_status is not None:
        vs = np.asarray(valve_status)
        state = np.where(vs >= 0, vs, state)
    return np.where(closed, 2, state).astype(np.uint8)


def pump_curve_from_points(flows, heads) -> Tuple[float, float, float]:
    """(h0, rp, n) of the head curve gain = h0 - rp q^n, EPANET's way.  One point (q_d, h_d): the shut-off head is 1.33 h_d and
    the head is zero at 2 q_d, with n = 2 fitted through the three.  Three points (0, h0), (q1, h1), (q2, h2) with
    h0 > h1 > h2 >= 0 and 0 < q1 < q2: the power fit n = ln((h0 - h2) / (h0 - h1)) / ln(q2 / q1), rp = (h0 - h1) / q1^n."""
    q, h = np.asarray(flows, dtype=np.float64).reshape(-1), np.asarray(heads, dtype=np.float64).reshape(-1)
    if q.shape != h.shape or q.size not in (1, 3) or not (np.isfinite(q).all() and np.isfinite(h).all()):
        raise ValueError("a pump curve has one point or three, all finite")
    if q.size == 1:
        if not (q[0] > 0 and h[0] > 0):
            raise ValueError("a single-point pump curve needs q > 0 and h > 0")
        q, h = np.array([0.0, q[0], 2.0 * q[0]]), np.array([1.33 * h[0], h[0], 0.0])
    if not (q[0] == 0 and 0 < q[1] < q[2] and h[0] > h[1] > h[2] >= 0):
        raise ValueError("a three-point pump curve needs q = 0 < q1 < q2 and h0 > h1 > h2 >= 0")
    n = float(np.log((h[0] - h[2]) / (h[0] - h[1])) / np.log(q[2] / q[1]))
    if not (np.isfinite(n) and n >= 1.0):
        raise ValueError(f"the pump curve's exponent {n} is below 1")
    return float(h[0]), float((h[0] - h[1]) / q[1] ** n), n


def links_lds_bytes(num_nodes: int, num_pipes: int, half_bandwidth: int, num_pumps: int) -> int:
    """What a workgroup of ``gatres_hydraulic_solve_links`` takes of the LDS (gatres.h states the same sum): a solve workgroup's
    arrays, per link m and its code, per pump h0, rp, n, w^2, w^(2-n) and w."""
    return lds_bytes(num_nodes, num_pipes, half_bandwidth) + 12 * num_pipes + 48 * num_pumps


def sensitivity_chunk(num_nodes: int, num_pipes: int, half_bandwidth: int, num_pumps: int, num_sensors: int) -> int:
    """Kc of ``gatres_hydraulic_sensitivity`` (gatres.h: THE SENSITIVITIES): how many of the K right-hand sides a workgroup takes at
    once -- as many as fit beside the links arrays and the two score accumulators, 0 where not even one does (the launch is
    refused)."""
    room = LDS_BUDGET - links_lds_bytes(num_nodes, num_pipes, half_bandwidth, num_pumps) - 16 * num_nodes
    return max(0, min(int(num_sensors), room // (8 * (num_nodes + 1))))


def sensitivity_lds_bytes(num_nodes: int, num_pipes: int, half_bandwidth: int, num_pumps: int, chunk: int) -> int:
    """What a workgroup of ``gatres_hydraulic_sensitivity`` takes of the LDS with ``chunk`` right-hand sides at once (gatres.h states
    the same sum): the links arrays, <z, rho> and <z, z> per row, and per right-hand side its column and its residual."""
    return links_lds_bytes(num_nodes, num_pipes, half_bandwidth, num_pumps) + 16 * num_nodes + 8 * chunk * (num_nodes + 1)


def series_links_lds_bytes(num_nodes: int, num_pipes: int, half_bandwidth: int, num_tanks: int, num_pumps: int) -> int:
    """What a workgroup of ``gatres_hydraulic_series_links`` takes of the LDS (gatres.h states the same sum)."""
    return series_lds_bytes(num_nodes, num_pipes, half_bandwidth, num_tanks) + 12 * num_pipes + 48 * num_pumps


def lds_bytes(num_nodes: int, num_pipes: int, half_bandwidth: int) -> int:
    """What a solve workgroup takes of the LDS (gatres.h states the same sum)."""
    return 8 * (num_nodes * (half_bandwidth + 1) + 2 * num_nodes + 4 * num_pipes) + 4 * (2 * num_pipes + num_nodes) + 64


def series_lds_bytes(num_nodes: int, num_pipes: int, half_bandwidth: int, num_tanks: int) -> int:
    """What a series workgroup takes of the LDS (gatres.h states the same sum): a solve workgroup's arrays, the step's demand
    and per tank the level, the area, two limits, the node and its row."""
    return lds_bytes(num_nodes, num_pipes, half_bandwidth) + 8 * num_nodes + 40 * num_tanks


def _mix64(z: np.ndarray) -> np.ndarray:
    z = z.astype(np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def hydraulic_draws(seed: int, first_scenario: int, num_scenarios: int, d_lo, d_hi, c_lo, c_hi) -> Tuple[np.ndarray, np.ndarray]:
    """``gatres_hydraulic_draw`` in numpy, bit for bit: (demand [S, N], roughness [S, P]) of the global scenarios
    ``first_scenario .. first_scenario + num_scenarios``."""
    d_lo, d_hi = np.asarray(d_lo, dtype=np.float64), np.asarray(d_hi, dtype=np.float64)
    c_lo, c_hi = np.asarray(c_lo, dtype=np.float64), np.asarray(c_hi, dtype=np.float64)
    N, P = d_lo.shape[0], c_lo.shape[0]
    with np.errstate(over="ignore"):
        g = np.arange(num_scenarios, dtype=np.uint64) + np.uint64(first_scenario % (1 << 64)) + np.uint64(1)
        stream = _mix64(np.uint64(seed % (1 << 64)) + np.uint64(0x9E3779B97F4A7C15) * g)
        cell = np.arange(N + P, dtype=np.uint64) + np.uint64(1)
        h = _mix64(stream[:, None] + np.uint64(0xBF58476D1CE4E5B9) * cell[None, :])
    u = (h >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    demand = d_lo[None, :] + (d_hi - d_lo)[None, :] * u[:, :N]
    roughness = c_lo[None, :] + (c_hi - c_lo)[None, :] * u[:, N:]
    return demand, roughness


def link_draw_ranges(c_lo, c_hi, num_pumps: int, pump_speed_range=None) -> Tuple[np.ndarray, np.ndarray]:
    """The roughness ranges [P] extended by the cells of the link draws, which come AFTER the N + P cells of a scenario (so the
    demands and the roughness of a scenario are what they are without them): Kp cells for the pump speeds, uniform in
    ``pump_speed_range`` (None: (1, 1)), then P cells uniform in [0, 1) that decide the closures."""
    c_lo, c_hi = np.asarray(c_lo, dtype=np.float64), np.asarray(c_hi, dtype=np.float64)
    w_lo, w_hi = (1.0, 1.0) if pump_speed_range is None else (float(pump_speed_range[0]), float(pump_speed_range[1]))
    if not (np.isfinite(w_lo) and np.isfinite(w_hi) and 0 <= w_lo <= w_hi):
        raise ValueError("pump_speed_range must be 0 <= lo <= hi, finite")
    P = c_lo.shape[0]
    return (np.concatenate([c_lo, np.full(num_pumps, w_lo), np.zeros(P)]), np.concatenate([c_hi, np.full(num_pumps, w_hi), np.ones(P)]))


def hydraulic_link_draws(seed: int, first_scenario: int, num_scenarios: int, d_lo, d_hi, c_lo, c_hi, num_pumps: int,
                         pump_speed_range=None, closed_probability: float = 0.0):
    """What ``generate_store(pump_speed_range=, closed_probability=)`` draws, in numpy, bit for bit: (demand [S, N], roughness
    [S, P], pump_speed [S, Kp], link_closed uint8 [S, P]); link p of a scenario is closed where its cell's uniform number is
    below ``closed_probability``."""
    P = np.asarray(c_lo).shape[0]
    lo, hi = link_draw_ranges(c_lo, c_hi, num_pumps, pump_speed_range)
    demand, cells = hydraulic_draws(seed, first_scenario, num_scenarios, d_lo, d_hi, lo, hi)
    closed = (cells[:, P + num_pumps:] < float(closed_probability)).astype(np.uint8)
    return demand, np.ascontiguousarray(cells[:, :P]), np.ascontiguousarray(cells[:, P:P + num_pumps]), closed


def hydraulic_valve_draws(seed: int, first_scenario: int, num_scenarios: int, d_lo, d_hi, c_lo, c_hi, num_pumps: int,
                          num_valves: int, valve_setting_range, pump_speed_range=None, closed_probability: float = 0.0):
    """What ``generate_store(valve_setting_range=)`` draws, in numpy, bit for bit: the four arrays of ``hydraulic_link_draws``,
    unchanged by the Kv cells that come AFTER all of theirs, and valve_setting [S, Kv], uniform in ``valve_setting_range``."""
    P = np.asarray(c_lo).shape[0]
    lo, hi = link_draw_ranges(c_lo, c_hi, num_pumps, pump_speed_range)
    v_lo, v_hi = float(valve_setting_range[0]), float(valve_setting_range[1])
    if not (np.isfinite(v_lo) and np.isfinite(v_hi) and v_lo <= v_hi):
        raise ValueError("valve_setting_range must be lo <= hi, finite")
    lo, hi = np.concatenate([lo, np.full(num_valves, v_lo)]), np.concatenate([hi, np.full(num_valves, v_hi)])
    demand, cells = hydraulic_draws(seed, first_scenario, num_scenarios, d_lo, d_hi, lo, hi)
    closed = (cells[:, P + num_pumps:2 * P + num_pumps] < float(closed_probability)).astype(np.uint8)
    return (demand, np.ascontiguousarray(cells[:, :P]), np.ascontiguousarray(cells[:, P:P + num_pumps]), closed,
            np.ascontiguousarray(cells[:, 2 * P + num_pumps:]))


def emitter_draw_ranges(c_lo, c_hi, num_pumps: int, num_valves: int, num_emitters: int, emitter_coefficient_range,
                        leak_onset_range=None, pump_speed_range=None, valve_setting_range=None) -> Tuple[np.ndarray, np.ndarray]:
    """The ranges of ``link_draw_ranges`` extended by the Kv valve cells (``valve_setting_range``, None: (0, 0), not used) and,
    AFTER all of those, by the cells of the emitter draws: Ke cells for the coefficients, uniform in
    ``emitter_coefficient_range``, Ke cells uniform in [0, 1) that decide whether the emitter leaks at all, and with
    ``leak_onset_range`` (lo, hi) Ke cells uniform in [lo, hi) whose floor is the onset step."""
    lo, hi = link_draw_ranges(c_lo, c_hi, num_pumps, pump_speed_range)
    v_lo, v_hi = (0.0, 0.0) if valve_setting_range is None else (float(valve_setting_range[0]), float(valve_setting_range[1]))
    e_lo, e_hi = float(emitter_coefficient_range[0]), float(emitter_coefficient_range[1])
    if not (np.isfinite(v_lo) and np.isfinite(v_hi) and v_lo <= v_hi):
        raise ValueError("valve_setting_range must be lo <= hi, finite")
    if not (np.isfinite(e_lo) and np.isfinite(e_hi) and 0 <= e_lo <= e_hi):
        raise ValueError("emitter_coefficient_range must be 0 <= lo <= hi, finite")
    parts_lo = [lo, np.full(num_valves, v_lo), np.full(num_emitters, e_lo), np.zeros(num_emitters)]
    parts_hi = [hi, np.full(num_valves, v_hi), np.full(num_emitters, e_hi), np.ones(num_emitters)]
    if leak_onset_range is not None:
        o_lo, o_hi = float(leak_onset_range[0]), float(leak_onset_range[1])
        if not (np.isfinite(o_lo) and np.isfinite(o_hi) and 0 <= o_lo <= o_hi < 2 ** 31):
            raise ValueError("leak_onset_range must be 0 <= lo <= hi, in steps")
        parts_lo.append(np.full(num_emitters, o_lo))
        parts_hi.append(np.full(num_emitters, o_hi))
    return np.concatenate(parts_lo), np.concatenate(parts_hi)


def hydraulic_emitter_draws(seed: int, first_scenario: int, num_scenarios: int, d_lo, d_hi, c_lo, c_hi, num_pumps: int,
                            num_valves: int, num_emitters: int, emitter_coefficient_range, leak_probability: float = 1.0,
                            leak_onset_range=None, pump_speed_range=None, closed_probability: float = 0.0,
                            valve_setting_range=None):
    """What ``generate_store(emitter_coefficient_range=, leak_probability=)`` and ``generate_series_store(..., leak_onset_range=)``
    draw, in numpy, bit for bit: the five arrays of ``hydraulic_valve_draws`` (the settings all 0 without
    ``valve_setting_range``), unchanged by the cells that come AFTER all of theirs, then emitter_coefficient [S, Ke] (0 where the
    emitter's second cell is not below ``leak_probability``) and emitter_onset int32 [S, Ke] (None without ``leak_onset_range``)."""
    P, Kp, Kv, Ke = np.asarray(c_lo).shape[0], num_pumps, num_valves, num_emitters
    lo, hi = emitter_draw_ranges(c_lo, c_hi, Kp, Kv, Ke, emitter_coefficient_range, leak_onset_range, pump_speed_range,
                                 valve_setting_range)
    demand, cells = hydraulic_draws(seed, first_scenario, num_scenarios, d_lo, d_hi, lo, hi)
    base = 2 * P + Kp + Kv
    closed = (cells[:, P + Kp:2 * P + Kp] < float(closed_probability)).astype(np.uint8)
    coef = np.where(cells[:, base + Ke:base + 2 * Ke] < float(leak_probability), cells[:, base:base + Ke], 0.0)
    onset = None if leak_onset_range is None else np.floor(cells[:, base + 2 * Ke:base + 3 * Ke]).astype(np.int32)
    return (demand, np.ascontiguousarray(cells[:, :P]), np.ascontiguousarray(cells[:, P:P + Kp]), closed,
            np.ascontiguousarray(cells[:, 2 * P + Kp:base]), np.ascontiguousarray(coef), onset)


def _half_bandwidth(pipes: np.ndarray, fixed: np.ndarray, position: np.ndarray) -> int:
    both = ~fixed[pipes[:, 0]] & ~fixed[pipes[:, 1]]
    if not both.any():
        return 0
    return int(np.abs(position[pipes[both, 0]] - position[pipes[both, 1]]).max())


def _reverse_cuthill_mckee(num_nodes: int, pipes: np.ndarray, fixed: np.ndarray) -> np.ndarray:
    """Reverse Cuthill-McKee over the junction-to-junction pipes (a fixed-head node is an identity row: it couples nothing and
    goes last).  Returns order: solver row -> node."""
    adj = [[] for _ in range(num_nodes)]
    for a, b in pipes:
        if not fixed[a] and not fixed[b]:
            adj[a].append(int(b))
            adj[b].append(int(a))
    deg = np.array([len(set(x)) for x in adj])
    seen = fixed.copy()
    out = []
    for start in sorted(np.flatnonzero(~fixed), key=lambda v: (deg[v], v)):
        if seen[start]:
            continue
        seen[start] = True
        queue, head = [int(start)], 0
        while head < len(queue):
            v = queue[head]
            head += 1
            for w in sorted(set(adj[v]), key=lambda x: (deg[x], x)):
                if not seen[w]:
                    seen[w] = True
                    queue.append(w)
        out.extend(queue)
    return np.array(out[::-1] + [int(v) for v in np.flatnonzero(fixed)], dtype=np.int32)


# ---- THE LAUNCH TABLES: a level's entry point and result class.  A level's arguments are those of the level below and one group
# more, in the order of the C signature: the prefix | the link group (in a series: and the speed-pattern group), link_state | the valve
# group, valve_changes | the emitter group with emitter_flow | the pdd scalars, demand_delivered | in a series: the control group
# with control_changes.  The result gains one field per level in the same way.
PIPES, LINKS, VALVES, EMITTERS, PDD, CONTROLS = range(6)
STEADY_LAUNCHES = (("gatres_hydraulic_solve", HydraulicResult), ("gatres_hydraulic_solve_links", HydraulicLinksResult),
                   ("gatres_hydraulic_solve_valves", HydraulicValvesResult), ("gatres_hydraulic_solve_emitters", HydraulicEmittersResult),
                   ("gatres_hydraulic_solve_pdd", HydraulicPddResult))
SERIES_LAUNCHES = (("gatres_hydraulic_series", HydraulicSeriesResult), ("gatres_hydraulic_series_links", HydraulicSeriesLinksResult),
                   ("gatres_hydraulic_series_valves", HydraulicSeriesValvesResult),
                   ("gatres_hydraulic_series_emitters", HydraulicSeriesEmittersResult),
                   ("gatres_hydraulic_series_pdd", HydraulicSeriesPddResult),
                   ("gatres_hydraulic_series_controls", HydraulicSeriesControlsResult))


def _launch_level(network, pdd, controls, emitters, valves, links, emitter_arrays, valve_arrays, link_arrays) -> int:
    """The level of a ``simulate`` / ``simulate_series`` call.  Controls take the controls launch and a demand model the pdd launch;
    below them ``emitters`` / ``valves`` / ``links`` decide where given, else the network's ``has_*`` flag or one of the level's
    arrays (``*_arrays``: the call's arguments, None where not given).  A level takes every level below it, and a network with
    emitters or regulating valves is refused below its own level."""
    if controls is not None:
        return CONTROLS
    if pdd is not None:
        return PDD
    given = lambda arrays: any(a is not None for a in arrays)
    if bool(emitters) if emitters is not None else (network.has_emitters or given(emitter_arrays)):
        return EMITTERS
    if network.has_emitters:
        raise ValueError("a network with emitters takes the emitters launch")
    if bool(valves) if valves is not None else (network.has_valves or given(valve_arrays)):
        return VALVES
    if network.has_valves:
        raise ValueError("a network with regulating valves takes the valves launch")
    return LINKS if (bool(links) if links is not None else (network.has_links or given(link_arrays))) else PIPES


def _add_level(call, group) -> None:
    """One level more on ``call`` = (arguments, result extras, held tensors), from ``group`` = (the group's arguments, its output,
    what the arguments point into): the arguments and the output's pointer (null for an empty one), the output as the result's next
    field, and the tensors to keep until the launch is queued."""
    out = group[1]
    call[0].extend(group[0])
    call[0].append(out.data_ptr() if out.numel() else None)
    call[1].append(out)
    call[2].append(group[2])


class HydraulicNetwork:
    """One water network for the steady-state solver.

    ``edge_index``: int64 [2, 2 P], both directions of every pipe (``wdn_synth.make_wdn_topology``'s layout); pipe p is the p-th
    column with source < destination, and runs from its source to its destination.  ``length``, ``diameter``: [P] metres;
    ``elevation``: [N] metres; ``fixed_nodes``: the fixed-head nodes, ``fixed_head``: their heads in metres (the default of
    ``simulate``).  Refused with ``ValueError``: a graph that is not symmetric or has a pipe from a node to itself, a junction
    that no path connects to a fixed-head node, a length or diameter that is not positive and finite, a band that does not fit
    the LDS budget of the kernel.  The solver order is the narrower of the given node order and reverse Cuthill-McKee.

    TANKS (``simulate_series``): ``tank_nodes`` are a subset of ``fixed_nodes``; ``tank_diameter`` [K] metres; ``tank_min_level``,
    ``tank_max_level`` [K] metres above the node's elevation, default (0, +inf).  An infinite maximum IS allowed: a tank that
    is never full.  Refused with ``ValueError``: a tank that is not a fixed node, duplicate tanks, a diameter that is not
    positive and finite, a minimum that is not finite, a maximum that is NaN or -inf, min > max.  ``simulate`` ignores the tanks:
    there every fixed-head node is held at its head.

    ``junctions`` are the nodes of a generated store and ``junction_edge_index`` its graph: the pipes between two junctions,
    renumbered.  A junction whose every pipe leads to a fixed-head node keeps no edge there; such nodes are listed in
    ``isolated_junctions`` (a model sees them without neighbours -- drop them from the sensor set, or model the reservoir's
    neighbour as the fixed node).

    REGULATING VALVES (the module's docstring: THE REGULATING VALVES): ``valve_links`` [Kv] links, ``valve_kind`` "PRV" / "PSV" (one
    for all, or one per valve), ``valve_setting`` [Kv] pressures in metres; a valve runs from a to b as its link does
    (``link_reversed``), its ``minor_loss`` K may be 0, its length is not read.  ``valve_node`` holds the controlled nodes.

    EMITTERS (the module's docstring: THE EMITTERS): ``emitter_nodes`` [Ke] junctions on which a leak can be, ``emitter_exponent``
    gamma (one for the network, default 0.5).  The coefficients are a scenario's: ``simulate(emitter_coefficient=)``."""

    def __init__(self, edge_index, length, diameter, elevation, fixed_nodes: Sequence[int], fixed_head,
                 start_velocity: float = START_VELOCITY, device=None, tank_nodes=None, tank_diameter=None, tank_min_level=None,
                 tank_max_level=None, minor_loss=None, check_valve=None, closed=None, pump_links=None, pump_h0=None, pump_r=None,
                 pump_n=None, pump_q_start=None, link_reversed=None, valve_links=None, valve_kind=None, valve_setting=None,
                 emitter_nodes=None, emitter_exponent: float = EMITTER_EXPONENT):
        ei = torch.as_tensor(edge_index).detach().cpu()
        if ei.dim() != 2 or ei.shape[0] != 2 or ei.dtype != torch.int64:
            raise ValueError("edge_index must be int64 [2, E]")
        e = ei.numpy()
        elevation = np.asarray(elevation, dtype=np.float64).reshape(-1)
        N = int(elevation.shape[0])
        if N < 2:
            raise ValueError("a network has at least two nodes")
        if e.size == 0 or e.min() < 0 or e.max() >= N:
            raise ValueError("edge_index refers to nodes outside the network")
        if (e[0] == e[1]).any():
            raise ValueError("a pipe from a node to itself")
        fwd = np.sort(e[0] * N + e[1])
        if not np.array_equal(fwd, np.sort(e[1] * N + e[0])):
            raise ValueError("edge_index is not symmetric: every pipe needs both directions")
        pipes = e[:, e[0] < e[1]].T.astype(np.int32)
        P = int(pipes.shape[0])
        length = np.asarray(length, dtype=np.float64).reshape(-1)
        diameter = np.asarray(diameter, dtype=np.float64).reshape(-1)
        if length.shape[0] != P or diameter.shape[0] != P:
            raise ValueError(f"length and diameter must have one entry per pipe ({P})")
        # the special links (THE LINK LAW): all absent by default, and then nothing below differs from a network of pipes
        per_link = lambda v, dt: np.zeros(P, dtype=dt) if v is None else np.asarray(v, dtype=dt).reshape(-1)
        minor_k = per_link(minor_loss, np.float64)
        check = per_link(check_valve, bool)
        shut = per_link(closed, bool)
        flip = per_link(link_reversed, bool)
        if not (minor_k.shape[0] == check.shape[0] == shut.shape[0] == flip.shape[0] == P):
            raise ValueError(f"minor_loss, check_valve, closed and link_reversed must have one entry per link ({P})")
        if not (np.isfinite(minor_k).all() and (minor_k >= 0).all()):
            raise ValueError("minor-loss coefficients must be finite and not negative")
        pumps = np.asarray([] if pump_links is None else pump_links, dtype=np.int64).reshape(-1)
        Kp = int(pumps.size)
        if Kp and (pumps.min() < 0 or pumps.max() >= P or np.unique(pumps).size != Kp):
            raise ValueError("pump_links must be distinct links of the network")
        p_h0 = np.asarray([] if pump_h0 is None else pump_h0, dtype=np.float64).reshape(-1)
        p_r = np.asarray([] if pump_r is None else pump_r, dtype=np.float64).reshape(-1)
        p_n = np.full(Kp, 2.0) if pump_n is None else np.asarray(pump_n, dtype=np.float64).reshape(-1)
        if p_h0.shape[0] != Kp or p_r.shape[0] != Kp or p_n.shape[0] != Kp:
            raise ValueError(f"pump_h0, pump_r and pump_n must have one entry per pump ({Kp})")
        if not (np.isfinite(p_h0).all() and (p_h0 >= 0).all() and np.isfinite(p_r).all() and (p_r > 0).all()
                and np.isfinite(p_n).all() and (p_n >= 1).all()):
            raise ValueError("a pump needs h0 >= 0, r > 0 and n >= 1, all finite")
        is_pump = np.zeros(P, dtype=bool)
        is_pump[pumps] = True
        if (minor_k[is_pump] != 0).any():
            raise ValueError("a pump has no minor loss")
        pipes[flip] = pipes[flip][:, ::-1]                  # a reversed link runs from its higher node to its lower one
        # the regulating valves (THE REGULATING VALVES): none by default
        valves = np.asarray([] if valve_links is None else valve_links, dtype=np.int64).reshape(-1)
        Kv = int(valves.size)
        if Kv and (valves.min() < 0 or valves.max() >= P or np.unique(valves).size != Kv):
            raise ValueError("valve_links must be distinct links of the network")
        v_names = [] if valve_kind is None else ([valve_kind] * Kv if isinstance(valve_kind, str) else list(valve_kind))
        if len(v_names) != Kv or any(k not in VALVE_KINDS for k in v_names):
            raise ValueError(f"valve_kind must be 'PRV' or 'PSV', one per valve ({Kv})")
        v_kind = np.array([VALVE_KINDS[k] for k in v_names], dtype=np.uint8)
        v_set = np.asarray([] if valve_setting is None else valve_setting, dtype=np.float64).reshape(-1)
        if v_set.shape[0] != Kv or not np.isfinite(v_set).all():
            raise ValueError(f"valve_setting must have one finite pressure per valve ({Kv})")
        is_valve = np.zeros(P, dtype=bool)
        is_valve[valves] = True
        if (is_valve & (is_pump | check)).any():
            raise ValueError("a regulating valve is neither a pump nor a CHECK link")
        v_ctrl = np.where(v_kind == LINK_PRV, pipes[valves, 1], pipes[valves, 0]).astype(np.int64)      # c: PRV b, PSV a
        v_free = np.where(v_kind == LINK_PRV, pipes[valves, 0], pipes[valves, 1]).astype(np.int64)      # the uncontrolled end
        if np.unique(pipes[valves].reshape(-1)).size != 2 * Kv:
            raise ValueError("two regulating valves share a node")
        length = np.where(is_valve, 0.0, length)            # (a valve's length is not read)
        throttle = (length == 0) & (minor_k > 0)            # r = 0 with m > 0: a throttle valve
        if not (np.isfinite(length).all() and ((length > 0) | throttle | is_pump | is_valve).all()
                and np.isfinite(diameter).all() and (diameter > 0).all()):
            raise ValueError("lengths and diameters must be positive and finite")
        if not np.isfinite(elevation).all():
            raise ValueError("elevations must be finite")
        fixed_nodes = np.asarray(fixed_nodes, dtype=np.int64).reshape(-1)
        heads = np.asarray(fixed_head, dtype=np.float64).reshape(-1)
        if fixed_nodes.size == 0 or fixed_nodes.min() < 0 or fixed_nodes.max() >= N or np.unique(fixed_nodes).size != fixed_nodes.size:
            raise ValueError("fixed_nodes must be distinct nodes of the network, at least one")
        if heads.shape[0] != fixed_nodes.size or not np.isfinite(heads).all():
            raise ValueError("fixed_head must have one finite head per fixed node")
        fixed = np.zeros(N, dtype=bool)
        fixed[fixed_nodes] = True
        if Kv and fixed[v_ctrl].any():
            raise ValueError("the controlled node of a regulating valve is a fixed-head node")
        # the emitters (THE EMITTERS): none by default
        emitters = np.asarray([] if emitter_nodes is None else emitter_nodes, dtype=np.int64).reshape(-1)
        Ke = int(emitters.size)
        gamma = float(emitter_exponent)
        with np.errstate(all="ignore"):
            if not (np.isfinite(gamma) and gamma > 0 and np.isfinite(np.float64(1.0) / np.float64(gamma))):
                raise ValueError("emitter_exponent must be finite and positive")
        if Ke and (emitters.min() < 0 or emitters.max() >= N or np.unique(emitters).size != Ke):
            raise ValueError("emitter_nodes must be distinct nodes of the network")
        if Ke and fixed[emitters].any():
            raise ValueError("an emitter sits on a junction, not on a fixed-head node")
        if Ke and Kv and np.isin(emitters, v_ctrl).any():
            raise ValueError("an emitter on the controlled node of a regulating valve is not modelled")
        adj = [[] for _ in range(N)]
        for p, (a, b) in enumerate(pipes):                  # a CHECK link is walked from a to b only, a closed one not at all,
            if shut[p] or is_valve[p]:                      # and a regulating valve not at all: ACTIVE, it is not in the matrix
                continue
            adj[a].append(int(b))
            if not (check[p] or is_pump[p]):
                adj[b].append(int(a))

        def walk(sources):
            reach = np.zeros(N, dtype=bool)
            reach[sources] = True
            stack = [int(v) for v in sources]
            while stack:
                v = stack.pop()
                for w in adj[v]:
                    if not reach[w]:
                        reach[w] = True
                        stack.append(w)
            return reach

        reach = walk(fixed_nodes)                           # every junction is fed from a fixed-head node
        if Kv:                                              # the two rules without which the ACTIVE system is singular
            if not reach[v_free].all():
                raise ValueError(f"the uncontrolled end of the regulating valves {valves[~reach[v_free]][:8].tolist()} does not "
                                 "reach a fixed-head node with all regulating valves removed")
            reach = walk(np.concatenate([fixed_nodes, v_ctrl]))
            if not reach.all():
                raise ValueError(f"junctions {np.flatnonzero(~reach)[:8].tolist()} reach neither a fixed-head node nor the "
                                 "controlled node of a regulating valve with all regulating valves removed")
        if not reach.all():
            raise ValueError(f"junctions {np.flatnonzero(~reach)[:8].tolist()} are not connected to a fixed-head node")

        self.num_nodes, self.num_pipes = N, P
        self.edge_index = ei
        self.pipes = pipes
        self.length, self.diameter, self.elevation = length, diameter, elevation
        self.fixed = fixed
        self.fixed_nodes = fixed_nodes
        self.fixed_head = np.zeros(N, dtype=np.float64)    # [N]: the heads at the fixed nodes, 0 elsewhere
        self.fixed_head[fixed_nodes] = heads
        self.junctions = np.flatnonzero(~fixed)
        # the tanks of a series (simulate_series): a subset of the fixed-head nodes
        tanks = np.asarray([] if tank_nodes is None else tank_nodes, dtype=np.int64).reshape(-1)
        K = int(tanks.size)
        if K and (tanks.min() < 0 or tanks.max() >= N or not fixed[tanks].all()):
            raise ValueError("tank_nodes must be fixed-head nodes of the network")
        if np.unique(tanks).size != K:
            raise ValueError("tank_nodes must be distinct")
        if K == 0 and any(v is not None and np.asarray(v).size for v in (tank_diameter, tank_min_level, tank_max_level)):
            raise ValueError("tank_diameter and the level limits need tank_nodes")
        t_dia = np.asarray([] if tank_diameter is None else tank_diameter, dtype=np.float64).reshape(-1)
        t_min = np.zeros(K) if tank_min_level is None else np.asarray(tank_min_level, dtype=np.float64).reshape(-1)
        t_max = np.full(K, np.inf) if tank_max_level is None else np.asarray(tank_max_level, dtype=np.float64).reshape(-1)
        if t_dia.shape[0] != K or t_min.shape[0] != K or t_max.shape[0] != K:
            raise ValueError(f"tank_diameter and the level limits must have one entry per tank ({K})")
        if not (np.isfinite(t_dia).all() and (t_dia > 0).all()):
            raise ValueError("tank diameters must be positive and finite")
        # the maximum may be +inf (the default: a tank that is never full); a minimum is finite, and nothing is NaN
        if not np.isfinite(t_min).all() or np.isnan(t_max).any() or (t_max == -np.inf).any() or (t_min > t_max).any():
            raise ValueError("tank level limits must be finite (the maximum may be +inf) with min <= max")
        self.tank_nodes, self.tank_diameter, self.tank_min_level, self.tank_max_level = tanks, t_dia, t_min, t_max
        self.num_tanks = K
        self.tank_area = np.pi * t_dia * t_dia / 4.0
        self.coef = HW_FACTOR * length / np.power(diameter, HW_DIAMETER_EXPONENT)
        self.q_start = float(start_velocity) * (np.pi * diameter * diameter / 4.0)
        # the link arrays of gatres_hydraulic_solve_links
        self.num_pumps, self.pump_links, self.pump_h0, self.pump_r, self.pump_n = Kp, pumps, p_h0, p_r, p_n
        self.is_pump, self.check_valve, self.closed, self.minor_loss = is_pump, check | is_pump, shut, minor_k
        self.link_kind = is_pump.astype(np.uint8) * LINK_PUMP
        self.link_kind[valves] = v_kind
        # the valve arrays of gatres_hydraulic_solve_valves
        self.num_valves, self.valve_links, self.valve_kind, self.valve_setting = Kv, valves, v_kind, v_set
        self.valve_kind_names = tuple(v_names)
        self.is_valve, self.valve_node, self.has_valves = is_valve, v_ctrl, Kv > 0
        self.coef[valves] = 0.0                             # (a valve has no resistance; its coef is not read)
        self.link_flags = (check.astype(np.uint8) * LINK_CHECK) | (shut.astype(np.uint8) * LINK_CLOSED)
        self.minor = 8.0 * minor_k / (np.pi ** 2 * GRAVITY * np.power(diameter, 4))
        self.has_links = bool(Kp or check.any() or shut.any() or (minor_k > 0).any())
        if Kp:
            self.coef[pumps] = 0.0                          # (a pump has no resistance; its coef is not read)
            if pump_q_start is None:                        # the flow at which the gain is 3/4 of the shut-off head
                q0 = np.power(p_h0 / (4.0 * p_r), 1.0 / p_n)
            else:
                q0 = np.asarray(pump_q_start, dtype=np.float64).reshape(-1)
                if q0.shape[0] != Kp or not (np.isfinite(q0).all() and (q0 >= 0).all()):
                    raise ValueError(f"pump_q_start must have one finite flow >= 0 per pump ({Kp})")
            self.q_start[pumps] = q0
        elif pump_q_start is not None and np.asarray(pump_q_start).size:
            raise ValueError("pump_q_start needs pump_links")
        self.pump_of_link = np.full(P, -1, dtype=np.int64)
        self.pump_of_link[pumps] = np.arange(Kp)
        identity = np.arange(N, dtype=np.int32)
        rcm = _reverse_cuthill_mckee(N, pipes, fixed)
        rcm_pos = np.empty(N, dtype=np.int32)
        rcm_pos[rcm] = identity
        if _half_bandwidth(pipes, fixed, rcm_pos) < _half_bandwidth(pipes, fixed, identity):
            self.order, self.position = rcm, rcm_pos
        else:                                               # (the given order is already as narrow: keep it)
            self.order, self.position = identity, identity.copy()
        self.half_bandwidth = max(1, _half_bandwidth(pipes, fixed, self.position))
        need = links_lds_bytes(N, P, self.half_bandwidth, Kp) if self.has_links else lds_bytes(N, P, self.half_bandwidth)
        if Kv:
            need = series_valves_lds_bytes(N, P, self.half_bandwidth, K, Kp, Kv) if K else valves_lds_bytes(N, P, self.half_bandwidth, Kp, Kv)
        # the emitter arrays of gatres_hydraulic_solve_emitters
        self.num_emitters, self.emitter_nodes, self.emitter_exponent, self.has_emitters = Ke, emitters, gamma, Ke > 0
        if Ke:
            need = series_emitters_lds_bytes(N, P, self.half_bandwidth, K, Kp, Kv, Ke) if K else \
                emitters_lds_bytes(N, P, self.half_bandwidth, Kp, Kv, Ke)
        if need > LDS_BUDGET:
            raise ValueError(f"the band of {N} rows with half-bandwidth {self.half_bandwidth} needs "
                             f"{need} bytes of LDS, the kernel has {LDS_BUDGET}")
        # the junction subgraph, renumbered: what a SnapshotStore over the junctions takes
        renum = np.full(N, -1, dtype=np.int64)
        renum[self.junctions] = np.arange(self.junctions.size)
        keep = ~fixed[e[0]] & ~fixed[e[1]]
        self.junction_edge_index = torch.from_numpy(renum[e[:, keep]])
        has_edge = np.zeros(N, dtype=bool)
        has_edge[e[0, keep]] = True
        self.isolated_junctions = renum[np.flatnonzero(~fixed & ~has_edge)]      # indices INSIDE the junction graph
        self.device = torch.device(device) if device is not None else None
        self._static: Dict[str, torch.Tensor] = {}

    @classmethod
    def from_inp(cls, source=None, **kw) -> "HydraulicNetwork":
        """The network of an EPANET input file: ``wdn_io.parse_inp_hydraulics(source, **kw).network`` (that function also returns
        the base demands, the roughness, the patterns and the pump speeds of the file, and says what it reads and refuses)."""
        from . import wdn_io
        return wdn_io.parse_inp_hydraulics(source, **kw).network

    # ---- the device side ----------------------------------------------------------------------------------------------------------
    def _dev(self) -> torch.device:
        if self.device is None:
            if not torch.cuda.is_available():
                raise RuntimeError("the hydraulic solver runs on a ROCm device; this engine has no CPU path (solve_ref is the "
                                   "host restatement)")
            self.device = torch.device("cuda", torch.cuda.current_device())
        return self.device

    def static(self) -> Dict[str, torch.Tensor]:
        """The static arrays of every launch, uploaded once: the network's pipes, fixed heads and tanks, its link, pump, valve and
        emitter arrays, the default pump speed ``speed1`` and the default pattern ``pattern0``.  A launch reads them from here."""
        if not self._static:
            dev, Kp = self._dev(), self.num_pumps
            up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
            self._static = {"pipe_a": up(self.pipes[:, 0], np.int32), "pipe_b": up(self.pipes[:, 1], np.int32),
                            "coef": up(self.coef, np.float64), "q_start": up(self.q_start, np.float64),
                            "fixed": up(self.fixed, np.uint8), "elevation": up(self.elevation, np.float64),
                            "order": up(self.order, np.int32), "position": up(self.position, np.int32),
                            "fixed_head": up(self.fixed_head, np.float64),
                            "junctions": up(self.junctions, np.int64),
                            "tank_node": up(self.tank_nodes, np.int32), "tank_area": up(self.tank_area, np.float64),
                            "tank_min": up(self.tank_min_level, np.float64), "tank_max": up(self.tank_max_level, np.float64),
                            "pattern0": torch.zeros(self.num_nodes, dtype=torch.int32, device=dev),
                            "link_kind": up(self.link_kind, np.uint8), "link_flags": up(self.link_flags, np.uint8),
                            "minor": up(self.minor, np.float64), "pump_link": up(self.pump_links, np.int32),
                            "pump_h0": up(self.pump_h0, np.float64), "pump_r": up(self.pump_r, np.float64),
                            "pump_n": up(self.pump_n, np.float64), "speed1": torch.ones(max(Kp, 1), dtype=torch.float64, device=dev),
                            "valve_link": up(self.valve_links, np.int32), "valve_kind": up(self.valve_kind, np.uint8),
                            "valve_setting": up(self.valve_setting, np.float64), "emitter_node": up(self.emitter_nodes, np.int32)}
        return self._static

    def _per_scenario(self, a, S: int, K: int, name: str, dtype=torch.float64):
        """An array that is [K] for the whole launch or [S, K] per scenario: the contiguous device tensor and its stride (0 or K),
        or (None, 0) without one."""
        if a is None:
            return None, 0
        if isinstance(a, np.ndarray) and not a.flags.writeable:
            a = a.copy()                                    # (torch does not take a read-only array as it is)
        t = torch.as_tensor(a, dtype=dtype).to(self._dev()).contiguous()
        if tuple(t.shape) == (K,):
            return t, 0
        if tuple(t.shape) == (S, K):
            return t, K
        raise ValueError(f"{name} must be [{K}] or [{S}, {K}]")

    # The three argument groups: each returns (the group's arguments before its output, the output tensor to fill, the tensors of
    # this call that the arguments point into, which the caller holds until the launch is queued) -- what ``_add_level`` takes.
    def _link_args(self, S: int, state_shape, pump_speed, link_closed):
        """The twelve link arguments of the links launches (no pump pointer without pumps) and ``link_state``."""
        st, dev, P, Kp = self.static(), self._dev(), self.num_pipes, self.num_pumps
        speed, speed_stride = self._per_scenario(pump_speed, S, Kp, "pump_speed")
        closed, closed_stride = self._per_scenario(link_closed, S, P, "link_closed", torch.uint8)
        speed = st["speed1"] if speed is None else speed
        pumps = [t.data_ptr() if Kp else None for t in (st["pump_link"], st["pump_h0"], st["pump_r"], st["pump_n"], speed)]
        return [st["link_kind"].data_ptr(), st["link_flags"].data_ptr(), st["minor"].data_ptr(), *pumps[:4], Kp, pumps[4],
                speed_stride, _native.ptr(closed), closed_stride], torch.empty(state_shape, dtype=torch.uint8, device=dev), (speed, closed)

    def _valve_args(self, S: int, changes_shape, valve_setting):
        """The five valve arguments of the valves launches (default: the network's settings) and ``valve_changes``."""
        st, Kv = self.static(), self.num_valves
        setting, stride = self._per_scenario(valve_setting, S, Kv, "valve_setting")
        setting = st["valve_setting"] if setting is None else setting
        return [t.data_ptr() if Kv else None for t in (st["valve_link"], st["valve_kind"], setting)] + [stride, Kv], \
            torch.empty(changes_shape, dtype=torch.int32, device=self._dev()), setting

    def _emitter_args(self, S: int, flow_shape, emitter_coefficient, emitter_onset=None, series: bool = False):
        """The emitter arguments of the emitters launches (in a series: with the onsets) and ``emitter_flow`` [*flow_shape, Ke]."""
        Ke = self.num_emitters
        if Ke and emitter_coefficient is None:
            raise ValueError("a network with emitters needs emitter_coefficient")
        if not Ke and emitter_coefficient is not None and torch.as_tensor(emitter_coefficient).numel():
            raise ValueError("emitter_coefficient needs a network with emitters")
        coef, stride = self._per_scenario(emitter_coefficient if Ke else None, S, Ke, "emitter_coefficient")
        if emitter_onset is not None and not series:
            raise ValueError("emitter_onset belongs to a series")
        onset, onset_stride = self._per_scenario(emitter_onset, S, Ke, "emitter_onset", torch.int32)
        if Ke == 0:
            onset, onset_stride = None, 0
        args = [self.static()["emitter_node"].data_ptr() if Ke else None, _native.ptr(coef), stride, Ke, float(self.emitter_exponent)]
        return args + ([_native.ptr(onset), onset_stride] if series else []), \
            torch.empty(tuple(flow_shape) + (Ke,), dtype=torch.float64, device=self._dev()), (coef, onset)

    def _launch(self, launches, level: int, args, lead, flags: int, status, final_dq, extras):
        """THE call of a launch table's row: the entry point with ``args`` and the stream, checked, and the row's result -- ``lead``,
        the iterations and ``flags`` flag columns of ``status`` (read after the launch, in stream order), ``status``, ``final_dq``
        and the level's ``extras``."""
        name, cls = launches[level]
        rc = getattr(_native.load(), name)(*args, _native.current_stream(self._dev()))
        _native.check(rc, name)
        return cls(*lead, status[..., 0], *[status[..., k] != 0 for k in range(1, flags + 1)], status, final_dq, *extras)


    def _f64(self, a, shape, name) -> torch.Tensor:
        t = torch.as_tensor(a, dtype=torch.float64).to(self._dev()).contiguous()
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name} must be {list(shape)}, got {list(t.shape)}")
        return t

    def _scenarios(self, demand, roughness, none: str):
        """(demand [S, N], roughness [S, P], S) of a call, on the device; ``none`` is what it says to S = 0."""
        demand = torch.as_tensor(demand)
        if demand.dim() != 2:
            raise ValueError("demand must be [S, N]")
        S = int(demand.shape[0])
        if S < 1:
            raise ValueError(none)
        return self._f64(demand, (S, self.num_nodes), "demand"), self._f64(roughness, (S, self.num_pipes), "roughness"), S

    def _draw(self, num_scenarios: int, seed: int, first_scenario: int, d_lo, d_hi, x_lo, x_hi, N: int, C: int):
        """THE ``gatres_hydraulic_draw`` launch: (demand [S, N], cells [S, C]) from the ranges of the N demand and the C other cells."""
        dev = self._dev()
        demand = torch.empty((num_scenarios, N), dtype=torch.float64, device=dev)
        cells = torch.empty((num_scenarios, C), dtype=torch.float64, device=dev)
        rc = _native.load().gatres_hydraulic_draw(d_lo.data_ptr(), d_hi.data_ptr(), x_lo.data_ptr(), x_hi.data_ptr(), num_scenarios,
                                                  N, C, seed % (1 << 64), first_scenario, demand.data_ptr(), cells.data_ptr(),
                                                  _native.current_stream(dev))
        _native.check(rc, "gatres_hydraulic_draw")
        return demand, cells

    def _draw_cells(self, cells: torch.Tensor, closed_probability: float):
        """The cells of a scenario after its demands, split where the blocks begin: (roughness [S, P], pump_speed [S, Kp],
        link_closed uint8 [S, P], valve_setting [S, Kv]) and the views of the three emitter blocks (coefficient, leak, onset:
        [S, Ke] each).  A block that was not drawn is empty."""
        at = np.cumsum([0, self.num_pipes, self.num_pumps, self.num_pipes, self.num_valves] + 3 * [self.num_emitters]).tolist()
        block = [cells[:, a:b] for a, b in zip(at, at[1:])]
        closed = (block[2] < float(closed_probability)).to(torch.uint8).contiguous()
        return (block[0].contiguous(), block[1].contiguous(), closed, block[3].contiguous()), block[4:]

    def draw(self, num_scenarios: int, seed: int, first_scenario: int, d_lo: torch.Tensor, d_hi: torch.Tensor, c_lo: torch.Tensor,
             c_hi: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """``gatres_hydraulic_draw``: (demand [S, N], roughness [S, P]) on the device."""
        return self._draw(num_scenarios, seed, first_scenario, d_lo, d_hi, c_lo, c_hi, self.num_nodes, self.num_pipes)

    def draw_links(self, num_scenarios: int, seed: int, first_scenario: int, d_lo: torch.Tensor, d_hi: torch.Tensor,
                   x_lo: torch.Tensor, x_hi: torch.Tensor, closed_probability: float):
        """``gatres_hydraulic_draw`` over the N + P cells of a scenario and the Kp + P link cells after them (``x_lo``, ``x_hi``:
        ``link_draw_ranges`` on the device): (demand [S, N], roughness [S, P], pump_speed [S, Kp], link_closed uint8 [S, P]).
        ``hydraulic_link_draws`` restates it."""
        return self.draw_valves(num_scenarios, seed, first_scenario, d_lo, d_hi, x_lo, x_hi, closed_probability)[:4]

    def draw_valves(self, num_scenarios: int, seed: int, first_scenario: int, d_lo: torch.Tensor, d_hi: torch.Tensor,
                    x_lo: torch.Tensor, x_hi: torch.Tensor, closed_probability: float):
        """``draw_links`` with the valve cells behind the link cells where ``x_lo``, ``x_hi`` hold their ranges (Kv more entries,
        or none): the four arrays of ``draw_links`` and valve_setting [S, Kv] or [S, 0].  ``hydraulic_valve_draws`` restates it."""
        C, base = int(x_lo.shape[0]), 2 * self.num_pipes + self.num_pumps
        if C not in (base, base + self.num_valves):
            raise ValueError("the ranges of the link cells do not fit the network")
        demand, cells = self._draw(num_scenarios, seed, first_scenario, d_lo, d_hi, x_lo, x_hi, self.num_nodes, C)
        return (demand, *self._draw_cells(cells, closed_probability)[0])

    def draw_emitters(self, num_scenarios: int, seed: int, first_scenario: int, d_lo: torch.Tensor, d_hi: torch.Tensor,
                      x_lo: torch.Tensor, x_hi: torch.Tensor, closed_probability: float, leak_probability: float):
        """``draw_valves`` with the emitter cells behind the Kv valve cells (``x_lo``, ``x_hi``: ``emitter_draw_ranges`` on the
        device, 2 Ke or 3 Ke entries more): the five arrays of ``draw_valves``, emitter_coefficient [S, Ke] and emitter_onset
        int32 [S, Ke] or None.  ``hydraulic_emitter_draws`` restates it."""
        Ke = self.num_emitters
        C, base = int(x_lo.shape[0]), 2 * self.num_pipes + self.num_pumps + self.num_valves
        if C not in (base + 2 * Ke, base + 3 * Ke):
            raise ValueError("the ranges of the emitter cells do not fit the network")
        demand, cells = self._draw(num_scenarios, seed, first_scenario, d_lo, d_hi, x_lo, x_hi, self.num_nodes, C)
        links, (coef, leak, onset) = self._draw_cells(cells, closed_probability)
        coef = torch.where(leak < float(leak_probability), coef, torch.zeros((), dtype=torch.float64, device=cells.device)).contiguous()
        return (demand, *links, coef, onset.floor().to(torch.int32).contiguous() if C == base + 3 * Ke and Ke else None)

    def _emitter_draw_setup(self, ranges, pump_speed_range, closed_probability, valve_setting_range, emitter_coefficient_range,
                            leak_probability, leak_onset_range=None):
        """None where a store is generated without emitter draws (the call it always was), else the device ranges of
        ``draw_emitters``."""
        if emitter_coefficient_range is None:
            if float(leak_probability) != 1.0 or leak_onset_range is not None:
                raise ValueError("leak_probability and leak_onset_range need emitter_coefficient_range")
            return None
        if self.num_emitters == 0:
            raise ValueError("emitter_coefficient_range needs a network with emitters")
        if not 0.0 <= float(leak_probability) <= 1.0:
            raise ValueError("leak_probability must lie in [0, 1]")
        self._check_link_draws(pump_speed_range, closed_probability, valve_setting_range)
        lo, hi = emitter_draw_ranges(ranges[2], ranges[3], self.num_pumps, self.num_valves, self.num_emitters,
                                     emitter_coefficient_range, leak_onset_range, pump_speed_range, valve_setting_range)
        return torch.from_numpy(lo).to(self._dev()), torch.from_numpy(hi).to(self._dev())

    def _check_link_draws(self, pump_speed_range, closed_probability, valve_setting_range) -> None:
        """What both draw setups refuse of the link and valve draws."""
        if valve_setting_range is not None and self.num_valves == 0:
            raise ValueError("valve_setting_range needs a network with regulating valves")
        if not 0.0 <= float(closed_probability) < 1.0:
            raise ValueError("closed_probability must lie in [0, 1)")
        if pump_speed_range is not None and self.num_pumps == 0:
            raise ValueError("pump_speed_range needs a network with pumps")

    def _link_draw_setup(self, ranges, pump_speed_range, closed_probability, valve_setting_range=None):
        """None where a store is generated without link draws (the call it always was), else the device ranges of ``draw_links``
        (of ``draw_valves``: with ``valve_setting_range`` the Kv valve cells come after all the others)."""
        if pump_speed_range is None and not closed_probability and valve_setting_range is None:
            return None
        self._check_link_draws(pump_speed_range, closed_probability, valve_setting_range)
        lo, hi = link_draw_ranges(ranges[2], ranges[3], self.num_pumps, pump_speed_range)
        if valve_setting_range is not None:
            v_lo, v_hi = float(valve_setting_range[0]), float(valve_setting_range[1])
            if not (np.isfinite(v_lo) and np.isfinite(v_hi) and v_lo <= v_hi):
                raise ValueError("valve_setting_range must be lo <= hi, finite")
            lo, hi = np.concatenate([lo, np.full(self.num_valves, v_lo)]), np.concatenate([hi, np.full(self.num_valves, v_hi)])
        return torch.from_numpy(lo).to(self._dev()), torch.from_numpy(hi).to(self._dev())

    def simulate(self, demand, roughness, fixed_head=None, accuracy: float = ACCURACY, max_iter: int = MAX_ITER,
                 want_head: bool = True, want_flow: bool = True, pump_speed=None, link_closed=None, links=None,
                 valve_setting=None, valves=None, emitter_coefficient=None, emitters=None, demand_model=None,
                 minimum_pressure: float = 0.0, required_pressure=None,
                 pressure_exponent: float = PRESSURE_EXPONENT) -> HydraulicResult:
        """Solve S scenarios on the device.  ``demand`` [S, N] m3/s (ignored at fixed nodes), ``roughness`` [S, P]
        Hazen-Williams coefficients, ``fixed_head`` None (the network's), [N] or [S, N] (read at fixed nodes).  Every field
        of the result is a device tensor; nothing is read back.  A network with a special link or a minor loss (or
        ``pump_speed`` [Kp] / [S, Kp], default 1; ``link_closed`` bytes [P] / [S, P]; or ``links=True``) takes
        ``gatres_hydraulic_solve_links`` and returns a ``HydraulicLinksResult``: the same fields and ``link_state`` uint8 [S, P].
        A network of pipes takes ``gatres_hydraulic_solve`` as it always did.  A network with a regulating valve (or
        ``valve_setting`` [Kv] / [S, Kv] metres of pressure, default the network's; or ``valves=True``) takes
        ``gatres_hydraulic_solve_valves`` and returns a ``HydraulicValvesResult``: the links fields and ``valve_changes`` int32 [S].
        A network with emitters (or ``emitters=True``) takes ``gatres_hydraulic_solve_emitters`` with ``emitter_coefficient`` [Ke] /
        [S, Ke] (m3/s per m^gamma, required; 0 is no leak there) and returns a ``HydraulicEmittersResult``: the valves fields and
        ``emitter_flow`` fp64 [S, Ke], the leaked flows.  ``demand_model="pda"`` (THE PRESSURE-DRIVEN DEMAND) takes
        ``gatres_hydraulic_solve_pdd`` on any network, with ``minimum_pressure``, ``required_pressure`` (required) in metres and
        ``pressure_exponent``, and returns a ``HydraulicPddResult``: the emitters fields and ``demand_delivered`` fp64 [S, N];
        ``demand_model="dda"`` takes the same launch demand-driven (every bit of the emitters launch, and the demand itself as
        ``demand_delivered``).  Without ``demand_model`` the call takes exactly the launches it always took."""
        st, dev, N, P = self.static(), self._dev(), self.num_nodes, self.num_pipes
        pdd = pdd_arguments(demand_model, minimum_pressure, required_pressure, pressure_exponent)
        level = _launch_level(self, pdd, None, emitters, valves, links, (emitter_coefficient,), (valve_setting,),
                              (pump_speed, link_closed))
        demand, roughness, S = self._scenarios(demand, roughness, "no scenarios")
        fh, stride = self._per_scenario(fixed_head, S, N, "fixed_head")
        fh = st["fixed_head"] if fh is None else fh
        new = lambda shape, dtype=torch.float64: torch.empty(shape, dtype=dtype, device=dev)
        pressure, status, final_dq = new((S, N), torch.float32), new((S, HYD_STATUS), torch.int32), new((S,))
        head, flow = new((S, N)) if want_head else None, new((S, P)) if want_flow else None
        # the 23 arguments every steady entry point begins with
        args = [st["pipe_a"].data_ptr(), st["pipe_b"].data_ptr(), st["coef"].data_ptr(), st["q_start"].data_ptr(),
                st["fixed"].data_ptr(), st["elevation"].data_ptr(), st["order"].data_ptr(), st["position"].data_ptr(),
                self.half_bandwidth, demand.data_ptr(), roughness.data_ptr(), fh.data_ptr(), stride, S, N, P, float(accuracy),
                int(max_iter), pressure.data_ptr(), _native.ptr(head), _native.ptr(flow), status.data_ptr(), final_dq.data_ptr()]
        call = (args, [], [])
        if level >= LINKS:
            _add_level(call, self._link_args(S, (S, P), pump_speed, link_closed))
        if level >= VALVES:
            _add_level(call, self._valve_args(S, (S,), valve_setting))
        if level >= EMITTERS:
            _add_level(call, self._emitter_args(S, (S,), emitter_coefficient))
        if level >= PDD:
            need = pdd_lds_bytes(N, P, self.half_bandwidth, self.num_pumps, self.num_valves, self.num_emitters, pdd[0])
            if need > LDS_BUDGET:
                raise ValueError(f"the band of {N} rows with half-bandwidth {self.half_bandwidth} needs {need} bytes of LDS "
                                 f"with this demand model, the kernel has {LDS_BUDGET}")
            _add_level(call, (pdd, new((S, N)), None))
        return self._launch(STEADY_LAUNCHES, level, args, (pressure, head, flow), 2, status, final_dq, call[1])

    def _sensitivity_launch(self, demand, roughness, sensor_nodes, fixed_head, pump_speed, link_closed, accuracy, max_iter, chunk,
                            readings, want):
        """THE ``gatres_hydraulic_sensitivity`` launch (gatres.h: THE SENSITIVITIES): the shared outputs and those named in ``want``
        (a subset of dh_ddemand, dh_droughness, residual, leak_flow, score, best), as a dict of device tensors."""
        if self.has_valves:
            raise ValueError("a network with regulating valves has no sensitivities here: an ACTIVE valve's flow is lagged outside "
                             "the matrix, so the matrix is not the Jacobian")
        st, dev, N, P = self.static(), self._dev(), self.num_nodes, self.num_pipes
        demand, roughness, S = self._scenarios(demand, roughness, "no scenarios")
        sensors = torch.as_tensor(np.array(sensor_nodes) if isinstance(sensor_nodes, np.ndarray) else sensor_nodes)
        if sensors.dim() != 1 or sensors.numel() < 1 or sensors.dtype.is_floating_point or sensors.dtype == torch.bool:
            raise ValueError("sensor_nodes must be a list of at least one node index")
        K = int(sensors.numel())
        sensors = sensors.to(device=dev, dtype=torch.int32).contiguous()
        if sensitivity_chunk(N, P, self.half_bandwidth, self.num_pumps, K) < 1:
            raise ValueError(f"the band of {N} rows with half-bandwidth {self.half_bandwidth} leaves no room in the LDS for one "
                             f"right-hand side ({LDS_BUDGET} bytes)")
        if chunk is not None and int(chunk) < 1:
            raise ValueError("chunk must be at least 1")
        fh, stride = self._per_scenario(fixed_head, S, N, "fixed_head")
        fh = st["fixed_head"] if fh is None else fh
        readings = None if readings is None else self._f64(readings, (S, K), "readings")
        new = lambda shape, dtype=torch.float64: torch.empty(shape, dtype=dtype, device=dev)
        out = {"pressure": new((S, N), torch.float32), "head": new((S, N)), "flow": new((S, P)),
               "status": new((S, HYD_STATUS), torch.int32), "final_dq": new((S,))}
        shapes = {"dh_ddemand": (S, K, N), "dh_droughness": (S, K, P), "residual": (S, K), "leak_flow": (S, N), "score": (S, N)}
        for name in want:
            out[name] = new((S,), torch.int32) if name == "best" else new(shapes[name])
        args = [st["pipe_a"].data_ptr(), st["pipe_b"].data_ptr(), st["coef"].data_ptr(), st["q_start"].data_ptr(),
                st["fixed"].data_ptr(), st["elevation"].data_ptr(), st["order"].data_ptr(), st["position"].data_ptr(),
                self.half_bandwidth, demand.data_ptr(), roughness.data_ptr(), fh.data_ptr(), stride, S, N, P, float(accuracy),
                int(max_iter), out["pressure"].data_ptr(), out["head"].data_ptr(), out["flow"].data_ptr(), out["status"].data_ptr(),
                out["final_dq"].data_ptr()]
        link_args, out["link_state"], held = self._link_args(S, (S, P), pump_speed, link_closed)
        args += link_args + [out["link_state"].data_ptr(), sensors.data_ptr(), K, 0 if chunk is None else int(chunk),
                             _native.ptr(readings)]
        args += [_native.ptr(out.get(name)) for name in ("dh_ddemand", "dh_droughness", "residual", "leak_flow", "score", "best")]
        rc = _native.load().gatres_hydraulic_sensitivity(*args, _native.current_stream(dev))
        _native.check(rc, "gatres_hydraulic_sensitivity")
        return out

    def sensitivity(self, demand, roughness, sensor_nodes, fixed_head=None, pump_speed=None, link_closed=None,
                    want_roughness: bool = False, accuracy: float = ACCURACY, max_iter: int = MAX_ITER,
                    chunk=None) -> HydraulicSensitivityResult:
        """Solve S scenarios as ``simulate(links=True)`` does and, in the same launch, the first-order sensitivities of the heads at
        ``sensor_nodes`` [K] (gatres.h: THE SENSITIVITIES): ``dh_ddemand`` fp64 [S, K, N], dH_sensor / dd_node = -(A^-1) in metres
        per m3/s (negative: an outflow lowers heads; 0 where the node or the sensor has a fixed head), and with ``want_roughness``
        ``dh_droughness`` fp64 [S, K, P], dH_sensor / dC_pipe (else None).  The other fields are those of a
        ``HydraulicLinksResult``, bit for bit.  A failed scenario has NaN.  A network with emitters is taken with its emitters not
        leaking: the nominal model a leak is measured against.  A network with regulating valves is refused (``ValueError``), and
        there is no ``demand_model``: neither system has ``A`` for its Jacobian.  ``chunk`` caps the right-hand sides a workgroup
        takes at once (default: as many as fit, ``sensitivity_chunk``); no output depends on it.  Nothing is read back."""
        o = self._sensitivity_launch(demand, roughness, sensor_nodes, fixed_head, pump_speed, link_closed, accuracy, max_iter, chunk,
                                     None, ("dh_ddemand", "dh_droughness") if want_roughness else ("dh_ddemand",))
        st = o["status"]
        return HydraulicSensitivityResult(o["pressure"], o["head"], o["flow"], st[:, 0], st[:, 1] != 0, st[:, 2] != 0, st,
                                          o["final_dq"], o["link_state"], o["dh_ddemand"], o.get("dh_droughness"))

    def localize_leaks(self, readings, demand, roughness, sensor_nodes, fixed_head=None, pump_speed=None, link_closed=None,
                       want_sensitivity: bool = False, accuracy: float = ACCURACY, max_iter: int = MAX_ITER,
                       chunk=None) -> LeakLocalization:
        """Where is the water lost?  ``readings`` fp64 [S, K]: measured pressures in metres at ``sensor_nodes`` (NaN: the sensor is
        missing in that scenario); ``demand``, ``roughness`` and the rest: the NOMINAL model, without the leak.  One launch solves
        the model, forms ``residual`` [S, K] = reading - model pressure (fp64 head - elevation) and matches it against every
        column z_n of ``dh_ddemand`` without writing that matrix: ``score`` [S, N] the cosine <z_n, rho> / (|z_n| |rho|) (+1: the
        residual is what an outflow at n would cause), ``leak_flow`` [S, N] the least-squares outflow <z_n, rho> / <z_n, z_n> in
        m3/s, ``best`` int32 [S] the lowest node among those holding the top score (-1 where every score is NaN: a failed scenario,
        no sensor, a zero residual).  Junctions behind the same sensor cut have proportional columns and scores that differ by
        rounding alone: ``best`` names one of them (``localization_report`` measures what that means).  ``pressure`` and
        ``status`` are the model's; ``dh_ddemand`` is None unless ``want_sensitivity``.  Refusals as ``sensitivity``.  Nothing is
        read back."""
        if readings is None:
            raise ValueError("localize_leaks needs readings")
        want = ("residual", "leak_flow", "score", "best") + (("dh_ddemand",) if want_sensitivity else ())
        o = self._sensitivity_launch(demand, roughness, sensor_nodes, fixed_head, pump_speed, link_closed, accuracy, max_iter, chunk,
                                     readings, want)
        return LeakLocalization(o["score"], o["leak_flow"], o["best"], o["residual"], o["pressure"], o["status"], o.get("dh_ddemand"))

    def valid(self, result: HydraulicResult, pressure_range: Tuple[float, float]) -> torch.Tensor:
        """``gatres_hydraulic_valid``: uint8 [S], 1 where the scenario converged, did not fail and every junction pressure lies
        in the range."""
        st, dev, lib = self.static(), self._dev(), _native.load()
        S = int(result.pressure.shape[0])
        out = torch.empty((S,), dtype=torch.uint8, device=dev)
        rc = lib.gatres_hydraulic_valid(result.pressure.data_ptr(), result.status.data_ptr(), st["fixed"].data_ptr(), S,
                                        self.num_nodes, float(pressure_range[0]), float(pressure_range[1]), out.data_ptr(),
                                        _native.current_stream(dev))
        _native.check(rc, "gatres_hydraulic_valid")
        return out

    # ---- the series ---------------------------------------------------------------------------------------------------------------
    def simulate_series(self, demand, roughness, multipliers, *, step_seconds: float, initial_level=None, pattern_of_node=None,
                        fixed_head=None, warm_start: bool = True, accuracy: float = ACCURACY, max_iter: int = MAX_ITER,
                        want_head: bool = True, want_flow: bool = True, pump_speed=None, link_closed=None, speed_multipliers=None,
                        speed_pattern_of_pump=None, links=None, valve_setting=None, valves=None, emitter_coefficient=None,
                        emitter_onset=None, emitters=None, demand_model=None, minimum_pressure: float = 0.0,
                        required_pressure=None, pressure_exponent: float = PRESSURE_EXPONENT, controls=None,
                        control_threshold=None) -> HydraulicSeriesResult:
        """``gatres_hydraulic_series``: S series of T steps on the device, one launch.  ``demand`` [S, N] base demands,
        ``roughness`` [S, P], ``multipliers`` [M, T] (for every series) or [S, M, T], ``pattern_of_node`` int [N] with values in
        [0, M) (default: pattern 0 everywhere; host data outside the range raises ``ValueError``, a DEVICE tensor is not read back
        and a value outside the range makes the kernel fail every series of the launch), ``initial_level`` [S, K] or [K] (default: fixed_head - elevation at the tank
        nodes), ``fixed_head`` as in ``simulate``.  Every field of the result is a device tensor; nothing is read back:
        pressure [S, T, N] fp32, head [S, T, N], flow [S, T, P], level [S, T + 1, K], iterations / converged / failed / limited
        [S, T], status [S, T, 4], final_dq [S, T].  A network without tanks works (K = 0: patterns only).  A network with a
        special link or a minor loss (or one of the link arguments, or ``links=True``) takes ``gatres_hydraulic_series_links`` and
        returns a ``HydraulicSeriesLinksResult`` with ``link_state`` uint8 [S, T, P]: ``pump_speed`` and ``link_closed`` as in
        ``simulate``, ``speed_multipliers`` [Ms, T] (default ones) and ``speed_pattern_of_pump`` int [Kp] (default 0); pump k
        runs at pump_speed[s][k] * speed_multipliers[pattern][t] in step t, and 0 switches it off for that step.  A network with
        a regulating valve (or ``valve_setting`` [Kv] / [S, Kv], or ``valves=True``) takes ``gatres_hydraulic_series_valves`` and
        returns a ``HydraulicSeriesValvesResult`` with ``valve_changes`` int32 [S, T]; with ``warm_start`` the statuses carry over
        from step to step, without it they start ACTIVE at every step.  The series launch takes 8 N bytes of LDS more than the
        steady one; a network with valves and without tanks that the constructor accepted for ``simulate`` but whose series does
        not fit is refused here with ``ValueError``.  A network with emitters (or ``emitters=True``) takes
        ``gatres_hydraulic_series_emitters`` with ``emitter_coefficient`` [Ke] / [S, Ke] and ``emitter_onset`` int [Ke] / [S, Ke]
        (default 0: emitter k leaks nothing at the steps t < onset) and returns a ``HydraulicSeriesEmittersResult`` with
        ``emitter_flow`` fp64 [S, T, Ke]; with ``warm_start`` an emitter's flow carries over while it stays on.  ``demand_model``,
        ``minimum_pressure``, ``required_pressure`` and ``pressure_exponent`` as in ``simulate``: ``gatres_hydraulic_series_pdd`` and a
        ``HydraulicSeriesPddResult`` with ``demand_delivered`` fp64 [S, T, N]; a junction is pressure-driven at the steps where
        its demand times the multiplier is positive, and with ``warm_start`` keeps its delivered flow while it stays so.
        ``controls`` (a ``ControlTable``, or what ``control_table`` takes) gives THE CONTROLS: ``gatres_hydraulic_series_controls``,
        the pdd launch (demand-driven unless ``demand_model="pda"``) with the table evaluated at the start of every step, and a
        ``HydraulicSeriesControlsResult`` with ``control_changes`` int32 [S, T]; ``control_threshold`` [Kc] or [S, Kc] overrides the
        table's thresholds.  With ``controls=None`` nothing changes."""
        st, dev, N, P, K, Kp = self.static(), self._dev(), self.num_nodes, self.num_pipes, self.num_tanks, self.num_pumps
        pdd = pdd_arguments(demand_model, minimum_pressure, required_pressure, pressure_exponent)
        if controls is None and control_threshold is not None:
            raise ValueError("control_threshold needs controls")
        if controls is not None and pdd is None:
            pdd = (0, 0.0, 0.0, PRESSURE_EXPONENT)
        level = _launch_level(self, pdd, controls, emitters, valves, links, (emitter_coefficient, emitter_onset), (valve_setting,),
                              (pump_speed, link_closed, speed_multipliers, speed_pattern_of_pump))
        demand, roughness, S = self._scenarios(demand, roughness, "no series")
        mult = torch.as_tensor(multipliers, dtype=torch.float64).to(dev).contiguous()
        if mult.dim() == 2 and mult.shape[0] >= 1 and mult.shape[1] >= 1:
            M, T, mult_stride = int(mult.shape[0]), int(mult.shape[1]), 0
        elif mult.dim() == 3 and mult.shape[0] == S and mult.shape[1] >= 1 and mult.shape[2] >= 1:
            M, T = int(mult.shape[1]), int(mult.shape[2])
            mult_stride = M * T
        else:
            raise ValueError(f"multipliers must be [M, T] or [{S}, M, T]")
        pattern = st["pattern0"]
        if pattern_of_node is not None:
            on_device = isinstance(pattern_of_node, torch.Tensor) and pattern_of_node.is_cuda
            pattern = torch.as_tensor(pattern_of_node)
            if tuple(pattern.shape) != (N,):
                raise ValueError(f"pattern_of_node must be [{N}]")
            if not on_device and (int(pattern.min()) < 0 or int(pattern.max()) >= M):      # (host data: no read-back)
                raise ValueError(f"pattern_of_node must hold values in [0, {M})")
            pattern = pattern.to(device=dev, dtype=torch.int32).contiguous()
        fh, stride = self._per_scenario(fixed_head, S, N, "fixed_head")
        fh = st["fixed_head"] if fh is None else fh
        level0, _ = self._per_scenario(initial_level, S, K, "initial_level")
        if level0 is None:
            tanks = st["tank_node"].to(torch.int64)
            level0 = fh.reshape(-1, N).index_select(1, tanks) - st["elevation"].index_select(0, tanks)[None, :]
        level0 = (level0[None, :] if level0.dim() == 1 else level0).expand(S, K).contiguous()      # (the launch takes [S, K])
        if not (float(step_seconds) > 0.0 and np.isfinite(float(step_seconds))):
            raise ValueError("step_seconds must be positive and finite")
        new = lambda shape, dtype=torch.float64: torch.empty(shape, dtype=dtype, device=dev)
        pressure, status, final_dq = new((S, T, N), torch.float32), new((S, T, HYD_STATUS), torch.int32), new((S, T))
        head, flow, tank_level = new((S, T, N)) if want_head else None, new((S, T, P)) if want_flow else None, new((S, T + 1, K))
        tp = (lambda t: t.data_ptr()) if K else (lambda t: None)
        # the 37 arguments every series entry point begins with
        args = [st["pipe_a"].data_ptr(), st["pipe_b"].data_ptr(), st["coef"].data_ptr(), st["q_start"].data_ptr(),
                st["fixed"].data_ptr(), st["elevation"].data_ptr(), st["order"].data_ptr(), st["position"].data_ptr(),
                self.half_bandwidth, tp(st["tank_node"]), tp(st["tank_area"]), tp(st["tank_min"]), tp(st["tank_max"]), K,
                pattern.data_ptr(), mult.data_ptr(), mult_stride, M, demand.data_ptr(), roughness.data_ptr(), fh.data_ptr(), stride,
                tp(level0), S, T, N, P, float(step_seconds), 1 if warm_start else 0, float(accuracy), int(max_iter),
                pressure.data_ptr(), _native.ptr(head), _native.ptr(flow), tp(tank_level), status.data_ptr(), final_dq.data_ptr()]
        call = (args, [], [])
        if level >= LINKS:
            link_args, link_state, held = self._link_args(S, (S, T, P), pump_speed, link_closed)
            smult = torch.ones((1, T), dtype=torch.float64, device=dev) if speed_multipliers is None else \
                torch.as_tensor(speed_multipliers, dtype=torch.float64).to(dev).contiguous()
            if smult.dim() != 2 or smult.shape[0] < 1 or smult.shape[1] != T:
                raise ValueError(f"speed_multipliers must be [Ms, {T}]")
            spat = np.zeros(Kp, dtype=np.int64) if speed_pattern_of_pump is None else np.asarray(speed_pattern_of_pump, dtype=np.int64)
            if spat.shape != (Kp,) or (Kp and (spat.min() < 0 or spat.max() >= smult.shape[0])):
                raise ValueError(f"speed_pattern_of_pump must be [{Kp}] with values in [0, {int(smult.shape[0])})")
            spat = torch.from_numpy(spat.astype(np.int32)).to(dev)
            speed_args = [smult.data_ptr(), spat.data_ptr(), int(smult.shape[0])] if Kp else [None, None, 0]
            _add_level(call, (link_args + speed_args, link_state, (held, smult, spat)))
        if level >= VALVES:
            need = series_pdd_lds_bytes(N, P, self.half_bandwidth, K, Kp, self.num_valves, self.num_emitters,
                                        0 if pdd is None else pdd[0]) + (0 if controls is None else 12 * P + 16)
            if need > LDS_BUDGET:                           # (the constructor held a network without tanks to the steady launch's sum)
                raise ValueError(f"a series on the band of {N} rows with half-bandwidth {self.half_bandwidth} needs {need} bytes "
                                 f"of LDS, the kernel has {LDS_BUDGET}")
            _add_level(call, self._valve_args(S, (S, T), valve_setting))
        if level >= EMITTERS:
            _add_level(call, self._emitter_args(S, (S, T), emitter_coefficient, emitter_onset, True))
        if level >= PDD:
            _add_level(call, (pdd, new((S, T, N)), None))
        if level >= CONTROLS:
            table = controls if isinstance(controls, ControlTable) else control_table(self, controls, step_seconds)
            Kc = len(table)
            thr, thr_stride = self._per_scenario(table.threshold if control_threshold is None else control_threshold, S, Kc,
                                                 "control_threshold")
            up = lambda a: torch.from_numpy(np.array(a)).to(dev)
            held = [up(a) for a in (table.link, table.action, table.value, table.kind, table.target)] + [thr]
            _add_level(call, ([t.data_ptr() if Kc else None for t in held] + [thr_stride, Kc], new((S, T), torch.int32), held))
        return self._launch(SERIES_LAUNCHES, level, args, (pressure, head, flow, tank_level), 3, status, final_dq, call[1])

    def series_valid(self, result: HydraulicSeriesResult, pressure_range: Tuple[float, float], allow_limited: bool = False) -> torch.Tensor:
        """``gatres_hydraulic_series_valid``: uint8 [S], 1 where every step of the series converged and none failed, no level
        was clamped (unless ``allow_limited``) and every junction pressure of every step lies in the range."""
        st, dev, lib = self.static(), self._dev(), _native.load()
        S, T = int(result.pressure.shape[0]), int(result.pressure.shape[1])
        out = torch.empty((S,), dtype=torch.uint8, device=dev)
        rc = lib.gatres_hydraulic_series_valid(result.pressure.data_ptr(), result.status.data_ptr(), st["fixed"].data_ptr(), S, T,
                                               self.num_nodes, float(pressure_range[0]), float(pressure_range[1]),
                                               1 if allow_limited else 0, out.data_ptr(), _native.current_stream(dev))
        _native.check(rc, "gatres_hydraulic_series_valid")
        return out

    def level_ranges(self, level_range=None) -> Tuple[np.ndarray, np.ndarray]:
        """(lo, hi) [K] of the initial-level draw: ``level_range`` (default ``TANK_LEVEL_RANGE``), clipped to the tanks' limits."""
        lo, hi = TANK_LEVEL_RANGE if level_range is None else level_range
        lo = np.maximum(np.broadcast_to(np.asarray(lo, dtype=np.float64), (self.num_tanks,)), self.tank_min_level)
        hi = np.minimum(np.broadcast_to(np.asarray(hi, dtype=np.float64), (self.num_tanks,)), self.tank_max_level)
        if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (lo <= hi).all()):
            raise ValueError("level_range does not meet the tanks' level limits")
        return lo, hi

    def draw_levels(self, num_series: int, seed: int, first_series: int, lo: torch.Tensor, hi: torch.Tensor) -> torch.Tensor:
        """Initial levels [S, K]: ``gatres_hydraulic_draw`` once more, with N := K and P := 1 and the seed
        ``seed + LEVEL_SEED_OFFSET`` (mod 2^64); ``hydraulic_draws`` restates it."""
        if self.num_tanks == 0:
            return torch.empty((num_series, 0), dtype=torch.float64, device=self._dev())
        unit = torch.zeros(2, dtype=torch.float64, device=self._dev())
        return self._draw(num_series, seed + LEVEL_SEED_OFFSET, first_series, lo, hi, unit[:1], unit[1:], self.num_tanks, 1)[0]

    def _chunk_draws(self, seed: int, demand_range, roughness_range, pump_speed_range, closed_probability, valve_setting_range,
                     emitter_coefficient_range, leak_probability, leak_onset_range=None):
        """The draw of a store generator's chunk: ``draw(n, first)`` -> (demand, roughness, the keyword arguments that hand the
        drawn link, valve and emitter arrays to ``simulate`` / ``simulate_series``, the leak labels (coefficient, onset) or None).
        With emitter draws ``draw_emitters``, with link or valve draws ``draw_valves``, else ``draw``: the cells a call always drew."""
        host_ranges = self.draw_ranges(demand_range, roughness_range)
        ranges = [torch.from_numpy(a).to(self._dev()) for a in host_ranges]
        leak_ranges = self._emitter_draw_setup(host_ranges, pump_speed_range, closed_probability, valve_setting_range,
                                               emitter_coefficient_range, leak_probability, leak_onset_range)
        if leak_ranges is None and self.has_emitters:
            raise ValueError("a network with emitters needs emitter_coefficient_range")
        link_ranges = None if leak_ranges is not None else \
            self._link_draw_setup(host_ranges, pump_speed_range, closed_probability, valve_setting_range)

        def draw(n: int, first: int):
            if leak_ranges is None and link_ranges is None:
                return (*self.draw(n, seed, first, *ranges), {}, None)
            kw, labels = {}, None
            if leak_ranges is not None:
                demand, roughness, speed, closed, setting, coef, onset = self.draw_emitters(
                    n, seed, first, ranges[0], ranges[1], *leak_ranges, closed_probability, leak_probability)
                kw, labels = {"emitter_coefficient": coef, **({} if onset is None else {"emitter_onset": onset})}, (coef, onset)
            else:
                demand, roughness, speed, closed, setting = self.draw_valves(n, seed, first, ranges[0], ranges[1], *link_ranges,
                                                                             closed_probability)
            kw.update(pump_speed=speed if self.num_pumps else None, link_closed=closed)
            if valve_setting_range is not None:
                kw["valve_setting"] = setting
            return demand, roughness, kw, labels
        return draw

    def _finish_store(self, kept_rows, leak_rows, supply_rows, report, normalize: bool):
        """(store, report) of a generator: the kept rows as a ``SnapshotStore`` over the junctions, and the labels of the kept rows
        as ``report["leak"]`` (coefficient, flow, and onset where it was drawn) and ``report["supply"]`` (delivered, full)."""
        if leak_rows:
            coef, flow, onset = [None if rows[0] is None else torch.cat(rows, dim=0) for rows in zip(*leak_rows)]
            report["leak"] = {"coefficient": coef, "flow": flow, **({} if onset is None else {"onset": onset})}
        if supply_rows:
            delivered, full = [torch.cat(rows, dim=0) for rows in zip(*supply_rows)]
            report["supply"] = {"delivered": delivered, "full": full}
        return SnapshotStore(torch.cat(kept_rows, dim=0), self.junction_edge_index, device=self._dev(), normalize=normalize), report

    @staticmethod
    def _keep_labels(idx, res, labels, full, leak_rows, supply_rows) -> None:
        """The labels of a chunk's kept rows ``idx``: the drawn leaks and their flows, the delivered and the ``full`` demand."""
        if labels is not None:
            leak_rows.append((labels[0].index_select(0, idx), res.emitter_flow.index_select(0, idx),
                              None if labels[1] is None else labels[1].index_select(0, idx)))
        if full is not None:
            supply_rows.append((res.demand_delivered.index_select(0, idx), full))

    def generate_series_store(self, num_series: int, steps: int, seed: int, *, step_seconds: float = 300.0, multipliers=None,
                              pattern_of_node=None, level_range=None, demand_range=DEMAND_RANGE, roughness_range=ROUGHNESS_RANGE,
                              pressure_range: Tuple[float, float] = (0.0, 150.0), chunk: int = 256, normalize: bool = True,
                              allow_limited: bool = False, warm_start: bool = True, accuracy: float = ACCURACY,
                              max_iter: int = MAX_ITER, pump_speed_range=None, closed_probability: float = 0.0,
                              speed_multipliers=None, speed_pattern_of_pump=None, valve_setting_range=None,
                              emitter_coefficient_range=None, leak_probability: float = 1.0, leak_onset_range=None,
                              demand_model=None, minimum_pressure: float = 0.0, required_pressure=None,
                              pressure_exponent: float = PRESSURE_EXPONENT, controls=None):
        """Draw, simulate and filter ``num_series`` series of ``steps`` steps into a ``SnapshotStore`` over the junctions whose
        rows are series-major (E * steps rows for E kept series: what ``monitor_store(series_length=steps)`` expects).  Base
        demands and roughness per series come from ``draw``, the initial levels from ``draw_levels``; ``multipliers`` default to
        ``wdn_synth.make_demand_patterns(1, steps, step_seconds, seed)``.  Per chunk: draws -> series -> series_valid, ONE
        read-back (status and the valid bytes as one tensor), a device ``index_select`` of whole series.  Returns
        ``(store, report)``; the report counts series: drawn = kept + failed + not_converged + limited + out_of_range, each dropped
        series counted once by the first cause in that order (``series_report``), and gives max_iterations, mean_iterations
        (over the steps that did not fail), mean_iterations_first_step and series_length.  ``RuntimeError`` when nothing is
        kept.  ``pump_speed_range`` and ``closed_probability`` as in ``generate_store``, per series (a closure holds for the whole
        series); ``speed_multipliers`` and ``speed_pattern_of_pump`` go to ``simulate_series``; ``valve_setting_range`` as in
        ``generate_store``, per series and valve; ``emitter_coefficient_range`` and ``leak_probability`` as in ``generate_store``,
        per series and emitter, and ``leak_onset_range`` (lo, hi) draws the step at which each leak begins, the floor of a uniform
        number in [lo, hi), on Ke cells after those.  The report then has ``report["leak"]``: device tensors ``coefficient``
        [kept, Ke], ``flow`` [kept, steps, Ke] and, with ``leak_onset_range``, ``onset`` int32 [kept, Ke] -- the labels.
        ``demand_model`` and its three scalars as in ``generate_store``: ``report["supply"]`` then holds ``delivered`` and ``full``
        [kept, steps, N].  ``controls`` (as in ``simulate_series``: THE CONTROLS) goes to every chunk's launch as it is, so a
        pump that feeds a tank can be operated and its series kept."""
        pdd_kw = _pdd_keywords(demand_model, minimum_pressure, required_pressure, pressure_exponent)
        ctl_kw = {} if controls is None else {"controls": controls if isinstance(controls, ControlTable) else
                                              control_table(self, controls, step_seconds)}
        supply_rows = []
        if num_series < 1 or chunk < 1 or steps < 1:
            raise ValueError("num_series, steps and chunk must be positive")
        st, dev = self.static(), self._dev()
        if multipliers is None:
            from . import wdn_synth
            multipliers = wdn_synth.make_demand_patterns(1, steps, step_seconds, seed)
        mult = torch.as_tensor(multipliers, dtype=torch.float64).to(dev).contiguous()
        if mult.dim() != 2 or mult.shape[1] != steps:
            raise ValueError(f"multipliers must be [M, {steps}]")
        draw = self._chunk_draws(seed, demand_range, roughness_range, pump_speed_range, closed_probability, valve_setting_range,
                                 emitter_coefficient_range, leak_probability, leak_onset_range)
        link_kw = {k: v for k, v in (("speed_multipliers", speed_multipliers), ("speed_pattern_of_pump", speed_pattern_of_pump))
                   if v is not None}
        lv = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in self.level_ranges(level_range)]
        kept_rows, leak_rows, tables = [], [], []
        for first in range(0, num_series, chunk):
            n = min(chunk, num_series - first)
            demand, roughness, drawn_kw, labels = draw(n, first)
            level0 = self.draw_levels(n, seed, first, *lv)
            res = self.simulate_series(demand, roughness, mult, step_seconds=step_seconds, initial_level=level0,
                                       pattern_of_node=pattern_of_node, warm_start=warm_start, accuracy=accuracy,
                                       max_iter=max_iter, want_head=False, want_flow=False, **link_kw, **drawn_kw, **pdd_kw, **ctl_kw)
            ok = self.series_valid(res, pressure_range, allow_limited)
            table = torch.cat([res.status.reshape(n, -1), ok.to(torch.int32)[:, None]], dim=1).cpu().numpy()     # the read-back
            tables.append(table)
            rows = np.flatnonzero(table[:, -1])
            if rows.size:
                idx = torch.from_numpy(rows).to(dev)
                kept = res.pressure.index_select(0, idx).index_select(2, st["junctions"])
                kept_rows.append(kept.reshape(rows.size * steps, -1))
                full = None
                if pdd_kw:                                  # the full demand of a step: the kernel's one rounded product
                    pat = torch.zeros(self.num_nodes, dtype=torch.int64, device=dev) if pattern_of_node is None else \
                        torch.as_tensor(pattern_of_node).to(device=dev, dtype=torch.int64)
                    full = demand.index_select(0, idx)[:, None, :] * mult.t().index_select(1, pat)[None, :, :]
                self._keep_labels(idx, res, labels, full, leak_rows, supply_rows)
        table = np.concatenate(tables, axis=0)
        report = series_report(table[:, :-1].reshape(-1, steps, HYD_STATUS), table[:, -1], allow_limited)
        if not kept_rows:
            raise RuntimeError(f"no series of {num_series} was kept with every junction pressure in {tuple(pressure_range)}: {report}")
        return self._finish_store(kept_rows, leak_rows, supply_rows, report, normalize)

    def draw_ranges(self, demand_range=DEMAND_RANGE, roughness_range=ROUGHNESS_RANGE):
        """(d_lo, d_hi, c_lo, c_hi) as host fp64 arrays: a (lo, hi) pair of scalars for every junction / pipe, or of arrays
        [N] / [P]; fixed-head nodes get d_lo = d_hi = 0."""
        d_lo = np.broadcast_to(np.asarray(demand_range[0], dtype=np.float64), (self.num_nodes,)).copy()
        d_hi = np.broadcast_to(np.asarray(demand_range[1], dtype=np.float64), (self.num_nodes,)).copy()
        d_lo[self.fixed] = 0.0
        d_hi[self.fixed] = 0.0
        c_lo = np.broadcast_to(np.asarray(roughness_range[0], dtype=np.float64), (self.num_pipes,)).copy()
        c_hi = np.broadcast_to(np.asarray(roughness_range[1], dtype=np.float64), (self.num_pipes,)).copy()
        return d_lo, d_hi, c_lo, c_hi

    def generate_store(self, num_scenarios: int, seed: int, demand_range=DEMAND_RANGE, roughness_range=ROUGHNESS_RANGE,
                       pressure_range: Tuple[float, float] = (0.0, 150.0), chunk: int = 1024, normalize: bool = True,
                       accuracy: float = ACCURACY, max_iter: int = MAX_ITER, pump_speed_range=None, closed_probability: float = 0.0,
                       valve_setting_range=None, emitter_coefficient_range=None, leak_probability: float = 1.0,
                       demand_model=None, minimum_pressure: float = 0.0, required_pressure=None,
                       pressure_exponent: float = PRESSURE_EXPONENT):
        """Draw, solve and filter ``num_scenarios`` scenarios into a ``SnapshotStore`` over the junctions (pressures in metres
        before the store's normalisation).  Per chunk: draw -> solve -> valid, ONE read-back (status and the valid bytes as one
        tensor), a device ``index_select`` of the kept rows.  Returns ``(store, report)``; the report counts drawn, converged,
        failed, not_converged, out_of_range and kept scenarios (drawn = kept + out_of_range + not_converged + failed) and gives
        the maximum and the mean of the iterations over the scenarios that did not fail.  ``RuntimeError`` when nothing is
        kept.  Rows of all-zero or mostly-zero demand do not meet the ratio stop rule (the module's docstring says why) and
        are counted as not_converged, not kept: watch that count when the demand range reaches down to zero.
        ``pump_speed_range`` (lo, hi) draws a speed per scenario and pump, ``closed_probability`` closes every link of a scenario
        with that probability (``draw_links``: new cells after the existing ones, so a call without the two gives the store it
        always gave).  A scenario whose closures or check valves cut a zone off does not converge: it is counted as
        not_converged, apart from out_of_range, and dropped, never repaired.  ``valve_setting_range`` (lo, hi) draws a setting per
        scenario and regulating valve, on Kv cells after all the others (``draw_valves``); a scenario whose statuses cycle is
        counted as not_converged and dropped in the same way.  ``emitter_coefficient_range`` (lo, hi) draws a coefficient per
        scenario and emitter on Ke cells after all the others, and ``leak_probability`` decides on Ke further cells whether the
        emitter leaks at all (C = 0 where its cell is not below the probability; ``draw_emitters``).  The report then has
        ``report["leak"]``: device tensors ``coefficient`` and ``flow`` [kept, Ke] of the kept rows -- the labels.
        ``demand_model="pda"`` with ``minimum_pressure``, ``required_pressure`` and ``pressure_exponent`` (as in ``simulate``)
        solves every scenario pressure-driven; no cell is drawn for it, so the draws are those of the call without it.  The report
        then has ``report["supply"]``: device tensors ``delivered`` (``demand_delivered``) and ``full`` (the full demand, 0 at
        fixed-head nodes), fp64 [kept, N] of the kept rows -- the labels of deficient supply: a junction is short by
        full - delivered."""
        pdd_kw = _pdd_keywords(demand_model, minimum_pressure, required_pressure, pressure_exponent)
        supply_rows = []
        if num_scenarios < 1 or chunk < 1:
            raise ValueError("num_scenarios and chunk must be positive")
        st, dev = self.static(), self._dev()
        draw = self._chunk_draws(seed, demand_range, roughness_range, pump_speed_range, closed_probability, valve_setting_range,
                                 emitter_coefficient_range, leak_probability)
        kept_rows, leak_rows = [], []
        report = {"drawn": 0, "converged": 0, "failed": 0, "not_converged": 0, "out_of_range": 0, "kept": 0, "max_iterations": 0,
                  "mean_iterations": 0.0}
        iter_sum = 0
        for first in range(0, num_scenarios, chunk):
            n = min(chunk, num_scenarios - first)
            demand, roughness, drawn_kw, labels = draw(n, first)
            res = self.simulate(demand, roughness, accuracy=accuracy, max_iter=max_iter, want_head=False, want_flow=False,
                                **drawn_kw, **pdd_kw)
            ok = self.valid(res, pressure_range)
            table = torch.cat([res.status[:, :3], ok.to(torch.int32)[:, None]], dim=1).cpu().numpy()     # the read-back
            rows = np.flatnonzero(table[:, 3])
            alive = table[:, 2] == 0
            report["drawn"] += n
            report["converged"] += int(table[:, 1].sum())
            report["failed"] += int(table[:, 2].sum())
            report["kept"] += int(rows.size)
            if alive.any():
                report["max_iterations"] = max(report["max_iterations"], int(table[alive, 0].max()))
                iter_sum += int(table[alive, 0].sum())
            if rows.size:
                idx = torch.from_numpy(rows).to(dev)
                kept_rows.append(res.pressure.index_select(0, idx).index_select(1, st["junctions"]))
                self._keep_labels(idx, res, labels, demand.index_select(0, idx) if pdd_kw else None, leak_rows, supply_rows)
        report["not_converged"] = report["drawn"] - report["converged"] - report["failed"]
        report["out_of_range"] = report["converged"] - report["kept"]
        alive_n = report["drawn"] - report["failed"]
        report["mean_iterations"] = iter_sum / alive_n if alive_n else 0.0
        if not kept_rows:
            raise RuntimeError(f"no scenario of {num_scenarios} converged with every junction pressure in {tuple(pressure_range)}: "
                               f"{report}")
        return self._finish_store(kept_rows, leak_rows, supply_rows, report, normalize)


# ---- host restatements ----------------------------------------------------------------------------------------------------------------
def _resistance(network: HydraulicNetwork, roughness: np.ndarray) -> np.ndarray:
    return network.coef / np.power(roughness, HW_EXPONENT)


def _fixed_heads(network: HydraulicNetwork, fixed_head, S: int) -> np.ndarray:
    fh = network.fixed_head if fixed_head is None else np.asarray(fixed_head, dtype=np.float64)
    return np.broadcast_to(fh, (S, network.num_nodes))


class _NewtonRef:
    """The per-scenario Newton loop of ``solve_ref`` and ``simulate_series_ref``: the algorithm and the stop rule of the kernel in
    numpy fp64, with the kernel's order in every sum of the assembly and of the stop rule; the linear solve is the library's."""

    def __init__(self, network: "HydraulicNetwork", solver: str, accuracy: float, max_iter: int):
        if solver not in ("dense", "banded"):
            raise ValueError("solver must be 'dense' or 'banded'")
        self.net, self.solver, self.accuracy, self.max_iter = network, solver, accuracy, max_iter
        self.a, self.b = network.pipes[:, 0].astype(np.int64), network.pipes[:, 1].astype(np.int64)
        self.fixed = network.fixed
        self.ja, self.jb = ~self.fixed[self.a], ~self.fixed[self.b]
        self.jj = self.ja & self.jb
        if solver == "banded":
            from scipy.linalg import solveh_banded
            self.solveh_banded = solveh_banded
            self.pos, self.W = network.position.astype(np.int64), network.half_bandwidth

    def inputs_ok(self, d, hf, c, r) -> bool:
        return bool(np.isfinite(d).all() and np.isfinite(hf).all() and np.isfinite(c).all() and (c > 0).all()
                    and np.isfinite(r).all() and (r > 0).all())

    def link_inputs_ok(self, d, hf, c, r, law) -> bool:
        """``inputs_ok`` under THE LINK LAW: a pump's roughness is not read, r = 0 is allowed where m > 0, speeds are finite and
        not negative (``law`` is None where a speed or a closed byte was refused)."""
        if law is None:
            return False
        pipe = ~law["pump"] & ~self.net.is_valve           # (a valve's roughness is not read either)
        w = law["speed"]
        with np.errstate(all="ignore"):
            w_ok = np.isfinite(w * w).all() and np.isfinite(np.power(np.where(w > 0, w, 1.0), 2.0 - law["n"])).all()
        return bool(np.isfinite(d).all() and np.isfinite(hf).all() and np.isfinite(c[pipe]).all() and (c[pipe] > 0).all()
                    and np.isfinite(r[pipe]).all() and (r[pipe] >= 0).all() and (law["minor"][pipe & (r == 0)] > 0).all() and w_ok)

    def run(self, d, hf, r, q_start, law=None):
        """(H, q, iterations, converged, ok, rel) from the flows ``q_start``; d: demands (0 at fixed nodes), hf: fixed heads (0 at
        junctions), r: resistances; ``law``: None for pipes, or the per-link arrays of ``link_headloss`` (a shut link then
        starts at rest)."""
        N, P = self.net.num_nodes, self.net.num_pipes
        a, b, fixed, ja, jb, jj = self.a, self.b, self.fixed, self.ja, self.jb, self.jj
        q = q_start.copy()
        if law is not None:
            q[law["shut"] | (law["pump"] & (law["speed"] == 0))] = 0.0
        H = hf.copy()
        rel, ok, iterations, converged = 0.0, True, 0, False
        for it in range(1, self.max_iter + 1):
            iterations = it
            h, g = pipe_headloss(q, r) if law is None else link_headloss(q, r, **law)
            pinv, y = 1.0 / g, h / g
            t = q - y
            diag = np.zeros(N)
            F = -d.copy()
            for p in range(P):                              # a row's sums run over its pipes in pipe order, as in the kernel
                ap, bp, pi, tp = a[p], b[p], pinv[p], t[p]
                if ja[p]:
                    diag[ap] += pi
                    F[ap] -= tp
                    if not jb[p]:
                        F[ap] += pi * hf[bp]
                if jb[p]:
                    diag[bp] += pi
                    F[bp] += tp
                    if not ja[p]:
                        F[bp] += pi * hf[ap]
            diag[fixed] = 1.0
            F[fixed] = hf[fixed]
            try:
                if self.solver == "dense":
                    A = np.zeros((N, N))
                    A[np.arange(N), np.arange(N)] = diag
                    np.add.at(A, (a[jj], b[jj]), -pinv[jj])
                    np.add.at(A, (b[jj], a[jj]), -pinv[jj])
                    H = np.linalg.solve(A, F)
                else:
                    pos, W = self.pos, self.W
                    ab = np.zeros((W + 1, N))
                    ab[0, pos] = diag
                    hi, lo = np.maximum(pos[a[jj]], pos[b[jj]]), np.minimum(pos[a[jj]], pos[b[jj]])
                    np.add.at(ab, (hi - lo, lo), -pinv[jj])
                    Fb = np.empty(N)
                    Fb[pos] = F
                    H = self.solveh_banded(ab, Fb, lower=True)[pos]
            except (np.linalg.LinAlgError, ValueError):
                ok = False
                break
            dq = y - (H[a] - H[b]) * pinv
            q = q - dq
            dqs, qs = float(np.cumsum(np.abs(dq))[-1]), float(np.cumsum(np.abs(q))[-1])      # (added up in pipe order)
            if not (np.isfinite(dqs) and np.isfinite(qs)):
                ok = False
                break
            rel = dqs / qs if qs > 0 else (np.inf if dqs > 0 else 0.0)
            if dqs <= self.accuracy * qs:
                converged = True
                break
        return H, q, iterations, converged, ok, rel

    def run_valves(self, d, hf, r, q_start, law, valves, emit=None, pdd=None):
        """``run`` with THE REGULATING VALVES, the loop of ``hy_newton_valves``: ``valves`` is the record of ``valve_record``; its
        ``status`` [Kv] is the start and is replaced by the end, ``changes`` counts the status changes, ``margin_h`` and
        ``margin_q`` keep the smallest distance of a comparison of the status rules from its threshold (metres, m3/s).  With no
        valve it is ``run`` in every bit.  ``emit``: None, or the record of ``emitter_record`` (THE EMITTERS, the loop of
        ``hy_newton_valves<true>``); its ``q`` [Ke] is the start and is replaced by the end; with no emitter that is on, every
        bit is the one without the record.  ``pdd``: None, or the record of ``demand_record`` (THE PRESSURE-DRIVEN DEMAND, the
        loop of ``hy_newton_valves<true, true>``); its ``q`` [N] is the start and is replaced by the end."""
        N, P = self.net.num_nodes, self.net.num_pipes
        a, b, fixed = self.a, self.b, self.fixed
        link, psv, node, hset, live = valves["link"], valves["psv"], valves["node"], valves["hset"], valves["live"]
        status = valves["status"]
        status[~live] = VALVE_OPEN
        Kv = link.size
        shut0 = law["shut"] | (law["pump"] & (law["speed"] == 0))
        q = q_start.copy()
        q[shut0] = 0.0
        H = hf.copy()
        rel, ok, iterations, converged = 0.0, True, 0, False
        for it in range(1, self.max_iter + 1):
            iterations = it
            active = np.zeros(P, dtype=bool)
            active[link[live & (status == VALVE_ACTIVE)]] = True
            closed = np.zeros(P, dtype=bool)
            closed[link[live & (status == VALVE_CLOSED)]] = True
            h, g = link_headloss(q, r, **dict(law, shut=law["shut"] | closed))
            pinv, y = np.where(active, 0.0, 1.0 / g), np.where(active, 0.0, h / g)
            on = live & (status == VALVE_ACTIVE)
            fx, hfe = fixed.copy(), hf.copy()               # the controlled node of an ACTIVE valve is a fixed row at hset
            fx[node[on]] = True
            hfe[node[on]] = hset[on]
            ja, jb = ~fx[a], ~fx[b]
            jj = ja & jb & ~active
            t = q - y
            diag = np.zeros(N)
            F = -d.copy()
            if emit is not None:
                e_on, qe = emit["C"] > 0, emit["q"]
                with np.errstate(all="ignore"):
                    he, ge = emitter_headloss(qe, np.where(e_on, emit["C"], 1.0), emit["gamma"])
                    einv, ey = np.where(e_on, 1.0 / ge, 0.0), np.where(e_on, he / ge, 0.0)
            if pdd is not None:
                d_on, qd = pdd["on"], pdd["q"]
                with np.errstate(all="ignore"):
                    hd, gd = demand_headloss(qd, np.where(d_on, pdd["D"], 1.0), pdd["dp"], pdd["exponent"])
                    dinv, dy = np.where(d_on, 1.0 / gd, 0.0), np.where(d_on, hd / gd, 0.0)
                F[d_on] = 0.0                               # a pressure-driven row has no fixed draw
            for p in range(P):                              # a row's sums run over its pipes in pipe order, as in the kernel
                ap, bp, pi, tp = a[p], b[p], pinv[p], t[p]
                if active[p]:                               # a fixed draw at both ends
                    if ja[p]:
                        F[ap] -= q[p]
                    if jb[p]:
                        F[bp] += q[p]
                    continue
                if ja[p]:
                    diag[ap] += pi
                    F[ap] -= tp
                    if not jb[p]:
                        F[ap] += pi * hfe[bp]
                if jb[p]:
                    diag[bp] += pi
                    F[bp] += tp
                    if not ja[p]:
                        F[bp] += pi * hfe[ap]
            if emit is not None:                            # the emitter's term, after the row's links
                for k in np.flatnonzero(e_on):
                    i = emit["node"][k]
                    diag[i] += einv[k]
                    F[i] -= qe[k] - ey[k]
                    F[i] += emit["z"][k] * einv[k]
            if pdd is not None:                             # then the junction's own demand term
                for i in np.flatnonzero(d_on):
                    diag[i] += dinv[i]
                    F[i] -= qd[i] - dy[i]
                    F[i] += pdd["z"][i] * dinv[i]
            diag[fx] = 1.0
            F[fx] = hfe[fx]
            try:
                if self.solver == "dense":
                    A = np.zeros((N, N))
                    A[np.arange(N), np.arange(N)] = diag
                    np.add.at(A, (a[jj], b[jj]), -pinv[jj])
                    np.add.at(A, (b[jj], a[jj]), -pinv[jj])
                    H = np.linalg.solve(A, F)
                else:
                    pos, W = self.pos, self.W
                    ab = np.zeros((W + 1, N))
                    ab[0, pos] = diag
                    hi, lo = np.maximum(pos[a[jj]], pos[b[jj]]), np.minimum(pos[a[jj]], pos[b[jj]])
                    np.add.at(ab, (hi - lo, lo), -pinv[jj])
                    Fb = np.empty(N)
                    Fb[pos] = F
                    H = self.solveh_banded(ab, Fb, lower=True)[pos]
            except (np.linalg.LinAlgError, ValueError):
                ok = False
                break
            H[node[on]] = hset[on]                          # (an identity row: the kernel's y / 1)
            dq = y - (H[a] - H[b]) * pinv
            q_new = q - dq
            if emit is not None:                            # the emitters' flows, after the links'
                dqe = np.where(e_on, ey - (H[emit["node"]] - emit["z"]) * einv, 0.0)
                emit["q"] = qe = np.where(e_on, qe - dqe, 0.0)
            if pdd is not None:                             # the delivered flows, after the emitters'
                with np.errstate(all="ignore"):
                    dqd = np.where(d_on, dy - (H - pdd["z"]) * dinv, 0.0)
                pdd["q"] = qd = np.where(d_on, qd - dqd, 0.0)
            d_valve = d if pdd is None else np.where(d_on, qd, d)      # what an ACTIVE valve's mass balance draws at its node
            changed = 0
            for k in range(Kv):                             # every valve from the old statuses, the new heads and its own new flow
                if not live[k]:
                    continue
                p, st = link[k], int(status[k])
                if st == VALVE_ACTIVE:
                    inflow = 0.0
                    for o in range(P):
                        if o == p:
                            continue
                        if b[o] == node[k]:
                            inflow += q_new[o]
                        if a[o] == node[k]:
                            inflow -= q_new[o]
                    qn = inflow - d_valve[node[k]] if psv[k] else d_valve[node[k]] - inflow
                    dq[p], q_new[p] = q[p] - qn, qn
                qv = q_new[p]
                ns, mh, mq = _valve_rule(bool(psv[k]), st, H[a[p]], H[b[p]], qv, (law["minor"][p] * abs(qv)) * qv, hset[k])
                valves["margin_h"], valves["margin_q"] = min(valves["margin_h"], mh), min(valves["margin_q"], mq)
                if ns != st:
                    changed += 1
                    status[k] = ns
                    if ns == VALVE_CLOSED:
                        q_new[p] = 0.0
            valves["changes"] += changed
            q = q_new
            adq, aq = np.abs(dq), np.abs(q)
            if emit is not None:                            # the emitters that are on join the sums after the links
                adq, aq = np.concatenate([adq, np.abs(dqe[e_on])]), np.concatenate([aq, np.abs(qe[e_on])])
            if pdd is not None:                             # then the pressure-driven junctions, in node order
                adq, aq = np.concatenate([adq, np.abs(dqd[d_on])]), np.concatenate([aq, np.abs(qd[d_on])])
            dqs, qs = float(np.cumsum(adq)[-1]), float(np.cumsum(aq)[-1])      # (added up in pipe order)
            if not (np.isfinite(dqs) and np.isfinite(qs)):
                ok = False
                break
            rel = dqs / qs if qs > 0 else (np.inf if dqs > 0 else 0.0)
            if dqs <= self.accuracy * qs and changed == 0:
                converged = True
                break
        return H, q, iterations, converged, ok, rel


def valve_record(network: "HydraulicNetwork", valve_setting=None, shut=None, status=None):
    """The valves of one scenario for ``_NewtonRef.run_valves``: target heads from ``valve_setting`` [Kv] (default the network's),
    ``live`` where the scenario's ``shut`` [P] leaves the valve its status machine, ``status`` (default: ACTIVE).  None where a
    setting or a target head is not finite: the scenario fails."""
    Kv = network.num_valves
    s = network.valve_setting if valve_setting is None else np.asarray(valve_setting, dtype=np.float64).reshape(Kv)
    with np.errstate(all="ignore"):
        hset = network.elevation[network.valve_node] + s
    if not np.isfinite(hset).all():
        return None
    live = np.ones(Kv, dtype=bool) if shut is None else ~np.asarray(shut, dtype=bool)[network.valve_links]
    st = np.full(Kv, VALVE_ACTIVE, dtype=np.int64) if status is None else np.asarray(status, dtype=np.int64).copy()
    return {"link": network.valve_links, "psv": network.valve_kind == LINK_PSV, "node": network.valve_node, "hset": hset,
            "live": live, "status": st, "changes": 0, "margin_h": np.inf, "margin_q": np.inf}


def emitter_record(network: "HydraulicNetwork", emitter_coefficient, q=None, keep=None):
    """The emitters of one scenario or step for ``_NewtonRef.run_valves``: ``emitter_coefficient`` [Ke] (0: off); the flows start
    at the coefficient itself, the flow at one metre of pressure, but where ``keep`` [Ke] (a warm series: the emitter was on in
    the step before) at ``q``.  None where a coefficient is negative or not finite: the scenario fails."""
    Ke = network.num_emitters
    C = np.zeros(0) if Ke == 0 else np.asarray(emitter_coefficient, dtype=np.float64).reshape(Ke).copy()
    if not (np.isfinite(C).all() and (C >= 0).all()):
        return None
    start = C.copy() if q is None or keep is None else np.where(keep, q, C)
    return {"node": network.emitter_nodes, "z": network.elevation[network.emitter_nodes], "C": C,
            "gamma": network.emitter_exponent, "q": np.where(C > 0, start, 0.0)}


def demand_record(network: "HydraulicNetwork", d, pdd, q=None, keep=None):
    """The pressure-driven junctions of one scenario or step for ``_NewtonRef.run_valves``: ``d`` [N] the full demands (0 at fixed
    nodes), ``pdd`` the tuple of ``pdd_arguments`` with model 1.  A junction is pressure-driven where d > 0; its flow starts at d,
    but where ``keep`` [N] (a warm series: it was pressure-driven in the step before) at ``q``.  None where the head
    elevation + Pmin of such a junction is not finite: the scenario fails."""
    d = np.asarray(d, dtype=np.float64)
    on = ~network.fixed & (d > 0)
    with np.errstate(all="ignore"):
        z = network.elevation + np.float64(pdd[1])
    if not np.isfinite(z[on]).all():
        return None
    start = d.copy() if q is None or keep is None else np.where(keep, q, d)
    return {"on": on, "D": np.where(on, d, 0.0), "z": z, "dp": np.float64(pdd[2]) - np.float64(pdd[1]), "exponent": pdd[3],
            "q": np.where(on, start, 0.0)}


def _delivered(record, d, fixed):
    """demand_delivered of one scenario or step: q_d where pressure-driven, the demand itself at other junctions, 0 at fixed nodes."""
    out = np.where(fixed, 0.0, d)
    return out if record is None else np.where(record["on"], record["q"], out)


def _valve_link_status(network, record) -> np.ndarray:
    """Per link: the status of a live valve, -1 elsewhere (what ``link_state_ref`` takes)."""
    vs = np.full(network.num_pipes, -1, dtype=np.int64)
    vs[record["link"][record["live"]]] = record["status"][record["live"]]
    return vs


def _link_resistance(network, roughness):
    """r per link under THE LINK LAW: a pump and a regulating valve have none, and their roughness is not read."""
    with np.errstate(all="ignore"):
        return np.where(network.is_pump | network.is_valve, 0.0, _resistance(network, roughness))


def link_law(network: HydraulicNetwork, pump_speed=None, link_closed=None):
    """The per-link arrays of ``link_headloss`` for one scenario: ``pump_speed`` [Kp] (default 1), ``link_closed`` [P] bytes
    (default none).  None where a speed is negative or not finite or a byte is above 1: the scenario fails."""
    P, Kp = network.num_pipes, network.num_pumps
    w = np.ones(Kp) if pump_speed is None else np.asarray(pump_speed, dtype=np.float64).reshape(Kp)
    cl = np.zeros(P, dtype=np.uint8) if link_closed is None else np.asarray(link_closed).reshape(P)
    if not (np.isfinite(w).all() and (w >= 0).all() and (cl <= 1).all() and (cl >= 0).all()):
        return None
    k = np.maximum(network.pump_of_link, 0)
    pick = lambda v, fill: np.where(network.is_pump, v[k], fill) if Kp else np.full(P, fill)
    return {"minor": network.minor, "pump": network.is_pump, "check": network.check_valve, "shut": network.closed | (cl != 0),
            "h0": pick(network.pump_h0, 0.0), "rp": pick(network.pump_r, 1.0), "n": pick(network.pump_n, 1.0), "speed": pick(w, 1.0)}


def _link_rows(network, S, pump_speed, link_closed):
    """[S, Kp] speeds and [S, P] bytes (or None) from what ``simulate`` takes."""
    w = None if pump_speed is None else np.broadcast_to(np.asarray(pump_speed, dtype=np.float64), (S, network.num_pumps))
    cl = None if link_closed is None else np.broadcast_to(np.asarray(link_closed), (S, network.num_pipes))
    return w, cl


def _solve_links_ref(network, demand, roughness, fixed_head, solver, accuracy, max_iter, pump_speed, link_closed,
                     with_valves=False, valve_setting=None, with_emitters=False, emitter_coefficient=None, pdd=None):
    newton = _NewtonRef(network, solver, accuracy, max_iter)
    demand, roughness = np.asarray(demand, dtype=np.float64), np.asarray(roughness, dtype=np.float64)
    S, N, P = demand.shape[0], network.num_nodes, network.num_pipes
    fh, fixed = _fixed_heads(network, fixed_head, S), network.fixed
    speeds, closed = _link_rows(network, S, pump_speed, link_closed)
    settings = None if valve_setting is None else np.broadcast_to(np.asarray(valve_setting, dtype=np.float64), (S, network.num_valves))
    head, flow = np.full((S, N), np.nan), np.full((S, P), np.nan)
    iterations, converged, failed = np.zeros(S, dtype=np.int32), np.zeros(S, dtype=bool), np.zeros(S, dtype=bool)
    final_dq, state = np.full(S, np.nan), np.zeros((S, P), dtype=np.uint8)
    changes, margin = np.zeros(S, dtype=np.int32), np.full((S, 2), np.inf)
    if with_emitters:
        if network.num_emitters and emitter_coefficient is None:
            raise ValueError("a network with emitters needs emitter_coefficient")
        e_coef = np.broadcast_to(np.zeros(0) if network.num_emitters == 0 else np.asarray(emitter_coefficient, dtype=np.float64),
                                 (S, network.num_emitters))
        e_flow = np.full((S, network.num_emitters), np.nan)
    delivered = np.full((S, N), np.nan)
    for s in range(S):
        c = roughness[s]
        r = _link_resistance(network, c)
        d, hf = np.where(fixed, 0.0, demand[s]), np.where(fixed, fh[s], 0.0)
        law = link_law(network, None if speeds is None else speeds[s], None if closed is None else closed[s])
        if not newton.link_inputs_ok(d, hf, c, r, law):
            failed[s] = True
            continue
        vs = None
        if with_valves:
            rec = valve_record(network, None if settings is None else settings[s], law["shut"])
            emit = emitter_record(network, e_coef[s]) if with_emitters else None
            dem = demand_record(network, d, pdd) if pdd is not None and pdd[0] else None
            if rec is None or (with_emitters and emit is None) or (pdd is not None and pdd[0] and dem is None):
                failed[s] = True
                continue
            H, q, iterations[s], converged[s], ok, rel = newton.run_valves(d, hf, r, network.q_start, law, rec, emit, dem)
            vs = _valve_link_status(network, rec)
        else:
            H, q, iterations[s], converged[s], ok, rel = newton.run(d, hf, r, network.q_start, law)
        if not ok:
            failed[s] = True
            continue
        head[s], flow[s], final_dq[s] = H, q, rel
        state[s] = link_state_ref(q, law["pump"], law["check"], law["shut"], law["speed"], vs)
        if with_valves:
            changes[s], margin[s] = rec["changes"], (rec["margin_h"], rec["margin_q"])
        if with_emitters:
            e_flow[s] = emit["q"]
        if pdd is not None:
            delivered[s] = _delivered(dem, d, fixed)
    if pdd is not None:
        return HydraulicPddReference(head, flow, iterations, converged, failed, final_dq, state, changes, margin, e_flow, delivered)
    if with_emitters:
        return HydraulicEmittersReference(head, flow, iterations, converged, failed, final_dq, state, changes, margin, e_flow)
    if with_valves:
        return HydraulicValvesReference(head, flow, iterations, converged, failed, final_dq, state, changes, margin)
    return HydraulicLinksReference(head, flow, iterations, converged, failed, final_dq, state)


def solve_ref(network: HydraulicNetwork, demand, roughness, fixed_head=None, solver: str = "dense", accuracy: float = ACCURACY,
              max_iter: int = MAX_ITER, pump_speed=None, link_closed=None, links=None, valve_setting=None,
              valves=None, emitter_coefficient=None, emitters=None, demand_model=None, minimum_pressure: float = 0.0,
              required_pressure=None, pressure_exponent: float = PRESSURE_EXPONENT) -> HydraulicReference:
    """The algorithm and the stop rule of the kernel in numpy fp64, scenario by scenario, with the kernel's order in every
    sum of the assembly and of the stop rule; the linear solve is the library's.  ``solver``: "dense"
    (``numpy.linalg.solve`` on the N x N system in the given node order) or "banded" (``scipy.linalg.solveh_banded`` in the
    solver order).  A network with special links (or ``pump_speed`` [Kp] / [S, Kp], ``link_closed`` [P] / [S, P], or
    ``links=True``) is solved under THE LINK LAW and returns a ``HydraulicLinksReference``.  A network with regulating valves (or
    ``valve_setting`` [Kv] / [S, Kv], or ``valves=True``) is solved with their status machine (``_NewtonRef.run_valves``) and
    returns a ``HydraulicValvesReference``: the links fields, ``valve_changes`` [S] and ``margin`` [S, 2], the smallest distance
    of a comparison of the status rules from its threshold over all iterations, in metres and in m3/s.  A network with emitters
    (or ``emitters=True``) is solved with their node term from ``emitter_coefficient`` [Ke] / [S, Ke] and returns a
    ``HydraulicEmittersReference``: the valves fields and ``emitter_flow`` [S, Ke].  ``demand_model`` and its three scalars as in
    ``simulate``: ``gatres_hydraulic_solve_pdd`` and a ``HydraulicPddReference`` with ``demand_delivered`` [S, N]."""
    pdd = pdd_arguments(demand_model, minimum_pressure, required_pressure, pressure_exponent)
    if pdd is not None:
        return _solve_links_ref(network, demand, roughness, fixed_head, solver, accuracy, max_iter, pump_speed, link_closed,
                                True, valve_setting, True, emitter_coefficient, pdd)
    if emitters or (emitters is None and (network.has_emitters or emitter_coefficient is not None)):
        return _solve_links_ref(network, demand, roughness, fixed_head, solver, accuracy, max_iter, pump_speed, link_closed,
                                True, valve_setting, True, emitter_coefficient)
    if valves or (valves is None and (network.has_valves or valve_setting is not None)):
        return _solve_links_ref(network, demand, roughness, fixed_head, solver, accuracy, max_iter, pump_speed, link_closed,
                                True, valve_setting)
    if links or (links is None and (network.has_links or pump_speed is not None or link_closed is not None)):
        return _solve_links_ref(network, demand, roughness, fixed_head, solver, accuracy, max_iter, pump_speed, link_closed)
    newton = _NewtonRef(network, solver, accuracy, max_iter)
    demand = np.asarray(demand, dtype=np.float64)
    roughness = np.asarray(roughness, dtype=np.float64)
    S, N, P = demand.shape[0], network.num_nodes, network.num_pipes
    fh = _fixed_heads(network, fixed_head, S)
    fixed = network.fixed
    head = np.full((S, N), np.nan)
    flow = np.full((S, P), np.nan)
    iterations = np.zeros(S, dtype=np.int32)
    converged = np.zeros(S, dtype=bool)
    failed = np.zeros(S, dtype=bool)
    final_dq = np.full(S, np.nan)
    for s in range(S):
        c = roughness[s]
        with np.errstate(all="ignore"):
            r = _resistance(network, c)
        d = np.where(fixed, 0.0, demand[s])
        hf = np.where(fixed, fh[s], 0.0)
        if not newton.inputs_ok(d, hf, c, r):
            failed[s] = True
            continue
        H, q, iterations[s], converged[s], ok, rel = newton.run(d, hf, r, network.q_start)
        if not ok:
            failed[s] = True
            continue
        head[s], flow[s], final_dq[s] = H, q, rel
    return HydraulicReference(head, flow, iterations, converged, failed, final_dq)


def level_update_ref(network: HydraulicNetwork, level, flow, step_seconds: float) -> Tuple[np.ndarray, np.ndarray]:
    """THE LEVEL UPDATE of the kernel in numpy, bit for bit: ``level`` [..., K] and ``flow`` [..., P] of one step give
    (level of the next step [..., K], clamped [..., K] bool).  Per tank the pipes are added up in pipe order (+q where the pipe
    ends at the tank, -q where it starts there), then level + (inflow * dt) / A, then the clamp; every operation is rounded on
    its own.  A NaN stays a NaN and is not clamped."""
    level, flow = np.asarray(level, dtype=np.float64), np.asarray(flow, dtype=np.float64)
    dt = np.float64(step_seconds)
    nxt, clamped = np.empty_like(level), np.zeros(level.shape, dtype=bool)
    a, b = network.pipes[:, 0], network.pipes[:, 1]
    with np.errstate(all="ignore"):
        for k, node in enumerate(network.tank_nodes):
            inflow = np.zeros(level.shape[:-1])
            for p in range(network.num_pipes):
                if b[p] == node:
                    inflow = inflow + flow[..., p]
                if a[p] == node:
                    inflow = inflow - flow[..., p]
            vol = inflow * dt
            nl = level[..., k] + vol / network.tank_area[k]
            low, high = nl < network.tank_min_level[k], nl > network.tank_max_level[k]
            nl = np.where(low, network.tank_min_level[k], np.where(high, network.tank_max_level[k], nl))
            nxt[..., k], clamped[..., k] = nl, low | high
    return nxt, clamped


def _series_inputs(network, demand, multipliers, pattern_of_node):
    demand = np.asarray(demand, dtype=np.float64)
    S, N = demand.shape[0], network.num_nodes
    mult = np.asarray(multipliers, dtype=np.float64)
    if mult.ndim == 2:
        mult = np.broadcast_to(mult, (S,) + mult.shape)
    if mult.ndim != 3 or mult.shape[0] != S:
        raise ValueError("multipliers must be [M, T] or [S, M, T]")
    pattern = np.zeros(N, dtype=np.int64) if pattern_of_node is None else np.asarray(pattern_of_node, dtype=np.int64)
    if pattern.shape != (N,) or pattern.min() < 0 or pattern.max() >= mult.shape[1]:
        raise ValueError("pattern_of_node must be [N] with values in [0, M)")
    return demand, mult, pattern


def simulate_series_ref(network: HydraulicNetwork, demand, roughness, multipliers, step_seconds: float, initial_level=None,
                        pattern_of_node=None, fixed_head=None, solver: str = "dense", warm_start: bool = True,
                        accuracy: float = ACCURACY, max_iter: int = MAX_ITER, pump_speed=None, link_closed=None,
                        speed_multipliers=None, speed_pattern_of_pump=None, links=None, valve_setting=None,
                        valves=None, emitter_coefficient=None, emitter_onset=None, emitters=None, demand_model=None,
                        minimum_pressure: float = 0.0, required_pressure=None,
                        pressure_exponent: float = PRESSURE_EXPONENT, controls=None,
                        control_threshold=None) -> HydraulicSeriesReference:
    """``gatres_hydraulic_series`` in numpy fp64, series by series and step by step, on the Newton loop of ``solve_ref``: the
    rounded product demand * multiplier, the tank heads elevation + level, the warm or cold start, ``level_update_ref`` and
    the kernel's failure rules.  head [S, T, N], flow [S, T, P], level [S, T + 1, K], the rest [S, T].  With special links (as
    in ``simulate_series``) it is ``gatres_hydraulic_series_links`` and returns a ``HydraulicSeriesLinksReference``; with
    regulating valves (as in ``simulate_series``) it is ``gatres_hydraulic_series_valves`` and returns a
    ``HydraulicSeriesValvesReference`` (``valve_changes`` [S, T]; ``margin`` [S, T, 2] as in ``solve_ref``); with emitters (as in
    ``simulate_series``) it is ``gatres_hydraulic_series_emitters`` and returns a ``HydraulicSeriesEmittersReference``
    (``emitter_flow`` [S, T, Ke]); with ``demand_model`` (as in ``simulate_series``) it is ``gatres_hydraulic_series_pdd`` and returns
    a ``HydraulicSeriesPddReference`` (``demand_delivered`` [S, T, N]); with ``controls`` (as in ``simulate_series``) it is
    ``gatres_hydraulic_series_controls``: ``control_step_ref`` at the start of every step, the start rules of THE CONTROLS, and a
    ``HydraulicSeriesControlsReference`` (``control_changes`` [S, T], 0 where the step failed)."""
    newton = _NewtonRef(network, solver, accuracy, max_iter)
    demand, mult, pattern = _series_inputs(network, demand, multipliers, pattern_of_node)
    pdd = pdd_arguments(demand_model, minimum_pressure, required_pressure, pressure_exponent)
    table = None
    if controls is not None:
        table, c_thr = _control_inputs(network, controls, control_threshold, demand.shape[0], step_seconds)
        control_changes = np.zeros((demand.shape[0], mult.shape[2]), dtype=np.int32)
        evaluated = table.kind != CONTROL_KINDS["at_step"]
        if pdd is None:
            pdd = (0, 0.0, 0.0, PRESSURE_EXPONENT)
    elif control_threshold is not None:
        raise ValueError("control_threshold needs controls")
    if pdd is not None:
        emitters = True
        delivered = np.full((demand.shape[0], mult.shape[2], network.num_nodes), np.nan)
    with_emitters = bool(emitters) if emitters is not None else (
        network.has_emitters or emitter_coefficient is not None or emitter_onset is not None)
    if with_emitters:
        valves, Ke = True, network.num_emitters
        if Ke and emitter_coefficient is None:
            raise ValueError("a network with emitters needs emitter_coefficient")
        e_coef = np.broadcast_to(np.zeros(0) if Ke == 0 else np.asarray(emitter_coefficient, dtype=np.float64), (demand.shape[0], Ke))
        e_onset = np.broadcast_to(np.zeros(Ke, dtype=np.int64) if emitter_onset is None or Ke == 0 else
                                  np.asarray(emitter_onset, dtype=np.int64), (demand.shape[0], Ke))
        e_flow = np.full((demand.shape[0], mult.shape[2], Ke), np.nan)
    with_valves = bool(valves) if valves is not None else (network.has_valves or valve_setting is not None)
    with_links = with_valves or (bool(links) if links is not None else (
        network.has_links or any(v is not None for v in (pump_speed, link_closed, speed_multipliers, speed_pattern_of_pump))))
    if with_valves:
        settings = None if valve_setting is None else np.broadcast_to(np.asarray(valve_setting, dtype=np.float64),
                                                                      (demand.shape[0], network.num_valves))
        changes = np.zeros(demand.shape[:1] + (mult.shape[2],), dtype=np.int32)
        margin = np.full(changes.shape + (2,), np.inf)
    if with_links:
        speeds, closed = _link_rows(network, demand.shape[0], pump_speed, link_closed)
        smult = np.ones((1, mult.shape[2])) if speed_multipliers is None else np.asarray(speed_multipliers, dtype=np.float64)
        spat = np.zeros(network.num_pumps, dtype=np.int64) if speed_pattern_of_pump is None else \
            np.asarray(speed_pattern_of_pump, dtype=np.int64)
        state = np.zeros(demand.shape[:1] + (mult.shape[2], network.num_pipes), dtype=np.uint8)
    roughness = np.asarray(roughness, dtype=np.float64)
    S, N, P, K, T = demand.shape[0], network.num_nodes, network.num_pipes, network.num_tanks, mult.shape[2]
    fh = _fixed_heads(network, fixed_head, S)
    fixed, tanks = network.fixed, network.tank_nodes
    if initial_level is None:
        level0 = fh[:, tanks] - network.elevation[tanks][None, :]
    else:
        level0 = np.broadcast_to(np.asarray(initial_level, dtype=np.float64), (S, K))
    head, flow, level = np.full((S, T, N), np.nan), np.full((S, T, P), np.nan), np.full((S, T + 1, K), np.nan)
    iterations = np.zeros((S, T), dtype=np.int32)
    converged, limited = np.zeros((S, T), dtype=bool), np.zeros((S, T), dtype=bool)
    failed = np.ones((S, T), dtype=bool)
    final_dq = np.full((S, T), np.nan)
    level[:, 0] = level0
    for s in range(S):
        c = roughness[s]
        with np.errstate(all="ignore"):
            r = _resistance(network, c)
        hf = np.where(fixed, fh[s], 0.0)
        if with_links:
            r = _link_resistance(network, c)
            if not newton.link_inputs_ok(np.zeros(N), hf, c, r, link_law(network)):
                continue
        elif not newton.inputs_ok(np.zeros(N), hf, c, r):
            continue
        q, lev, valve_status = network.q_start, level0[s].copy(), None
        if with_emitters:                                   # a bad coefficient fails the series from step 0 on, whatever its onset
            if emitter_record(network, e_coef[s]) is None:
                continue
            e_q, e_was_on = np.zeros(Ke), np.zeros(Ke, dtype=bool)
        d_q, d_was_on = np.zeros(N), np.zeros(N, dtype=bool)
        if table is not None:                               # a threshold that is not finite fails the series from step 0 on
            if not np.isfinite(c_thr[s][evaluated]).all():
                continue
            cstate, was_shut = control_state(P), np.zeros(P, dtype=bool)
        for t in range(T):
            m = mult[s, :, t]
            with np.errstate(all="ignore"):
                d = np.where(fixed, 0.0, demand[s] * m[pattern])
                hf[tanks] = network.elevation[tanks] + lev
            if not (np.isfinite(m).all() and (m >= 0).all() and np.isfinite(d).all() and np.isfinite(hf[tanks]).all()):
                break
            law = None
            if with_links:
                sm = smult[:, t]
                if not (np.isfinite(sm).all() and (sm >= 0).all()):
                    break
                base = np.ones(network.num_pumps) if speeds is None else speeds[s]
                if table is not None:                       # THE CONTROLS: before the step's inputs are formed
                    cstate, n_changed = control_step_ref(table, c_thr[s], cstate, lev,
                                                         None if t == 0 else head[s, t - 1] - network.elevation, t)
                    pl = network.pump_links
                    base = np.where(cstate["has_value"][pl], cstate["value"][pl], base)
                with np.errstate(all="ignore"):
                    w = base * sm[spat]
                law = link_law(network, w, None if closed is None else closed[s])
                if law is not None and table is not None:   # a control state stands in place of the static flag and the byte
                    law["shut"] = np.where(cstate["ctl"] == CTL_NONE, law["shut"], cstate["ctl"] == CTL_CLOSED)
                if not newton.link_inputs_ok(d, hf, c, r, law):
                    break
            q_from = q if warm_start else network.q_start
            if with_valves:                                 # a warm series carries the statuses along with the flows
                v_set = None if settings is None else settings[s]
                v_status = valve_status if warm_start else None
                if table is not None:
                    reopened, again = control_start_ref(cstate, was_shut, t)
                    q_from = np.where(reopened, network.q_start, q_from)
                    vl = network.valve_links
                    v_set = np.where(cstate["has_value"][vl], cstate["value"][vl], network.valve_setting if v_set is None else v_set)
                    if v_status is not None and t > 0:      # such a valve starts ACTIVE, even in a warm series
                        v_status = np.where(again[vl], VALVE_ACTIVE, v_status)
                    was_shut = law["shut"] | (law["pump"] & (law["speed"] == 0))
                rec = valve_record(network, v_set, law["shut"], v_status)
                if rec is None:
                    break
                emit = None
                if with_emitters:                           # off before its onset; kept while it stays on in a warm series
                    emit = emitter_record(network, np.where(t < e_onset[s], 0.0, e_coef[s]), e_q, e_was_on & bool(warm_start))
                dem = None
                if pdd is not None and pdd[0]:              # kept while the junction stays pressure-driven in a warm series
                    dem = demand_record(network, d, pdd, d_q, d_was_on & bool(warm_start))
                    if dem is None:
                        break
                H, q_new, iterations[s, t], converged[s, t], ok, rel = newton.run_valves(d, hf, r, q_from, law, rec, emit, dem)
            else:
                H, q_new, iterations[s, t], converged[s, t], ok, rel = newton.run(d, hf, r, q if warm_start else network.q_start, law)
            if not ok:
                break
            q = q_new
            failed[s, t] = False
            head[s, t], flow[s, t], final_dq[s, t] = H, q, rel
            if with_valves:
                valve_status = rec["status"]
                changes[s, t], margin[s, t] = rec["changes"], (rec["margin_h"], rec["margin_q"])
            if with_emitters:
                e_flow[s, t] = e_q = emit["q"]
                e_was_on = emit["C"] > 0
            if pdd is not None:
                delivered[s, t] = _delivered(dem, d, fixed)
                if dem is not None:
                    d_q, d_was_on = dem["q"], dem["on"]
            if table is not None:
                control_changes[s, t] = n_changed
            if with_links:
                state[s, t] = link_state_ref(q, law["pump"], law["check"], law["shut"], law["speed"],
                                             _valve_link_status(network, rec) if with_valves else None)
            lev, clamped = level_update_ref(network, lev, q, step_seconds)
            level[s, t + 1], limited[s, t] = lev, clamped.any()
        converged[s] &= ~failed[s]
    if table is not None:
        return HydraulicSeriesControlsReference(head, flow, level, iterations, converged, failed, limited, final_dq, state, changes,
                                                margin, e_flow, delivered, control_changes)
    if pdd is not None:
        return HydraulicSeriesPddReference(head, flow, level, iterations, converged, failed, limited, final_dq, state, changes,
                                           margin, e_flow, delivered)
    if with_emitters:
        return HydraulicSeriesEmittersReference(head, flow, level, iterations, converged, failed, limited, final_dq, state, changes,
                                                margin, e_flow)
    if with_valves:
        return HydraulicSeriesValvesReference(head, flow, level, iterations, converged, failed, limited, final_dq, state, changes,
                                              margin)
    if with_links:
        return HydraulicSeriesLinksReference(head, flow, level, iterations, converged, failed, limited, final_dq, state)
    return HydraulicSeriesReference(head, flow, level, iterations, converged, failed, limited, final_dq)


def series_valid_ref(network: HydraulicNetwork, pressure, status, pressure_range, allow_limited: bool = False) -> np.ndarray:
    """``gatres_hydraulic_series_valid`` in numpy: uint8 [S] from pressure [S, T, N] fp32 and status [S, T, 4]."""
    pressure, status = np.asarray(pressure), np.asarray(status)
    p64 = pressure.astype(np.float64)[:, :, ~network.fixed]
    inside = ((p64 >= pressure_range[0]) & (p64 <= pressure_range[1])).all(axis=(1, 2))
    ok = (status[:, :, 1] != 0).all(axis=1) & (status[:, :, 2] == 0).all(axis=1) & inside
    if not allow_limited:
        ok &= (status[:, :, 3] == 0).all(axis=1)
    return ok.astype(np.uint8)


def series_report(status, valid, allow_limited: bool = False) -> Dict[str, float]:
    """The report of ``generate_series_store`` from the read-back tables: status [S, T, 4] and valid [S].  Counts are per
    series; a dropped series is counted once, by the first cause in the order failed, not_converged, limited, out_of_range, so
    drawn = kept + failed + not_converged + limited + out_of_range."""
    status, valid = np.asarray(status), np.asarray(valid) != 0
    S, T = status.shape[0], status.shape[1]
    failed = (status[:, :, 2] != 0).any(axis=1)
    not_conv = ~failed & (status[:, :, 1] == 0).any(axis=1)
    limited = ~failed & ~not_conv & (status[:, :, 3] != 0).any(axis=1) & (not allow_limited)
    out = ~failed & ~not_conv & ~limited & ~valid
    alive = status[:, :, 2] == 0
    first = alive[:, 0]
    return {"drawn": int(S), "kept": int((valid & ~failed & ~not_conv & ~limited).sum()), "failed": int(failed.sum()),
            "not_converged": int(not_conv.sum()), "limited": int(limited.sum()), "out_of_range": int(out.sum()),
            "max_iterations": int(status[:, :, 0][alive].max()) if alive.any() else 0,
            "mean_iterations": float(status[:, :, 0][alive].mean()) if alive.any() else 0.0,
            "mean_iterations_first_step": float(status[first, 0, 0].mean()) if first.any() else 0.0,
            "series_length": int(T)}


def series_volume_balance(network: HydraulicNetwork, result, demand, multipliers, step_seconds: float,
                          pattern_of_node=None, count_leaks: bool = True) -> np.ndarray:
    """THE INVARIANT of a series, per series and step, in m3 [S, T]: the change of the stored volume sum_k A_k level_k across the
    step minus dt times the net inflow to the tanks, the latter taken from the OTHER side of the network -- the net outflow of
    the reservoirs (from ``result.flow``) minus the step's total demand (from ``demand`` and ``multipliers``).  It is zero up
    to the mass residual of the step's solution, except across a step whose level was clamped.  ``result`` has ``flow``
    [S, T, P] and ``level`` [S, T + 1, K] (a ``HydraulicSeriesReference``, or a device result brought to numpy).  On a network with
    emitters ``result.emitter_flow`` [S, T, Ke] is an outflow like the demand: the leaked volume dt * sum q_e leaves the network;
    ``count_leaks=False`` leaves it out, and the balance is then off by exactly that volume.  A result with ``demand_delivered``
    [S, T, N] (a launch with a demand model) is balanced with the delivered volume in place of the demanded one."""
    demand, mult, pattern = _series_inputs(network, demand, multipliers, pattern_of_node)
    flow, level = np.asarray(result.flow, dtype=np.float64), np.asarray(result.level, dtype=np.float64)
    a, b = network.pipes[:, 0], network.pipes[:, 1]
    tank = np.zeros(network.num_nodes, dtype=bool)
    tank[network.tank_nodes] = True
    reservoir = network.fixed & ~tank
    out_of_reservoirs = flow[:, :, reservoir[a]].sum(axis=2) - flow[:, :, reservoir[b]].sum(axis=2)
    per_node = demand[:, None, :] * np.swapaxes(mult, 1, 2)[:, :, pattern]              # [S, T, N]
    if getattr(result, "demand_delivered", None) is not None:
        per_node = np.asarray(result.demand_delivered, dtype=np.float64)
    total_demand = per_node[:, :, ~network.fixed].sum(axis=2)
    if network.num_emitters and count_leaks:
        total_demand = total_demand + np.asarray(result.emitter_flow, dtype=np.float64).sum(axis=2)
    stored = (level * network.tank_area[None, None, :]).sum(axis=2)                     # [S, T + 1]
    return (stored[:, 1:] - stored[:, :-1]) - float(step_seconds) * (out_of_reservoirs - total_demand)


def hydraulic_residuals(network: HydraulicNetwork, head, flow, demand, roughness, fixed_head=None, pump_speed=None,
                        link_closed=None, law=link_headloss, valve_setting=None, link_state=None, emitter_flow=None,
                        emitter_coefficient=None, emitter_law=emitter_headloss, demand_delivered=None, demand_model=None,
                        minimum_pressure: float = 0.0, required_pressure=None, pressure_exponent: float = PRESSURE_EXPONENT,
                        demand_law=demand_headloss) -> Tuple[np.ndarray, np.ndarray]:
    """How well (head, flow) satisfy the model, per scenario: (mass, energy).  mass: the largest junction imbalance
    |inflow - outflow - demand| divided by sum |q| (not divided where that sum is 0); energy: the largest
    |H_a - H_b - h_p(q_p)| over the pipes and |H_f - fixed head| over the fixed nodes, in metres.  NaN where an input is.
    A network with special links (or ``pump_speed`` / ``link_closed``) is held to THE LINK LAW, ``law`` (``link_headloss``; the
    tests plant wrong ones).  A network with regulating valves needs ``link_state`` [S, P], the statuses the solution was
    returned with (and takes ``valve_setting`` [Kv] / [S, Kv], default the network's): an OPEN valve is held to the PIPE branch
    with r = 0, a CLOSED one to h = 1e8 q, and the energy check of an ACTIVE valve is |H_c - hset|.  A network with emitters
    needs ``emitter_flow`` [S, Ke] and ``emitter_coefficient`` [Ke] / [S, Ke]: the mass balance of an emitter's junction counts
    q_e as an outflow and sum |q| includes |q_e|; the emitter's energy residual is |H_i - z_i - h(q_e)| under ``emitter_law``
    (``emitter_headloss``), on either branch; an emitter with C = 0 is held to q_e = 0 (its |q_e| joins the mass residual).
    With ``demand_model="pda"`` (and its scalars, as in ``simulate``) ``demand_delivered`` [S, N] is needed: a junction with a
    positive demand draws its delivered flow q_d in the mass balance, sum |q| includes |q_d|, and its virtual link's energy
    residual is |H_i - elevation_i - Pmin - h(q_d)| under ``demand_law`` (``demand_headloss``), on every branch; at the other
    junctions |delivered - demand| joins the mass residual."""
    pdd = pdd_arguments(demand_model, minimum_pressure, required_pressure, pressure_exponent)
    pdd = pdd if pdd is not None and pdd[0] else None
    if pdd is not None:
        if demand_delivered is None:
            raise ValueError("demand_model='pda' needs demand_delivered")
        d_q = np.asarray(demand_delivered, dtype=np.float64).reshape(np.asarray(head).shape[0], network.num_nodes)
    head, flow = np.asarray(head, dtype=np.float64), np.asarray(flow, dtype=np.float64)
    demand, roughness = np.asarray(demand, dtype=np.float64), np.asarray(roughness, dtype=np.float64)
    S, N = head.shape[0], network.num_nodes
    with_links = network.has_links or network.has_valves or pump_speed is not None or link_closed is not None
    speeds, closed = _link_rows(network, S, pump_speed, link_closed)
    if network.has_valves:
        if link_state is None:
            raise ValueError("a network with regulating valves needs link_state")
        vstate = np.asarray(link_state)[:, network.valve_links]
        settings = np.broadcast_to(network.valve_setting if valve_setting is None else np.asarray(valve_setting, dtype=np.float64),
                                   (S, network.num_valves))
    fh = _fixed_heads(network, fixed_head, S)
    a, b, fixed = network.pipes[:, 0].astype(np.int64), network.pipes[:, 1].astype(np.int64), network.fixed
    mass, energy = np.empty(S), np.empty(S)
    Ke = network.num_emitters
    if Ke:
        if emitter_flow is None or emitter_coefficient is None:
            raise ValueError("a network with emitters needs emitter_flow and emitter_coefficient")
        e_q = np.asarray(emitter_flow, dtype=np.float64).reshape(S, Ke)
        e_c = np.broadcast_to(np.asarray(emitter_coefficient, dtype=np.float64), (S, Ke))
    for s in range(S):
        net = np.zeros(N)
        np.add.at(net, b, flow[s])
        np.add.at(net, a, -flow[s])
        if Ke:                                              # a leak is an outflow of its junction; none where C = 0
            np.add.at(net, network.emitter_nodes, -np.where(e_c[s] > 0, e_q[s], 0.0))
        draw = demand[s]
        if pdd is not None:                                 # a pressure-driven junction draws what it is delivered
            d_on = ~fixed & (demand[s] > 0)
            draw = np.where(d_on, d_q[s], demand[s])
        imbalance = np.abs(net - draw)[~fixed]
        if Ke:
            imbalance = np.concatenate([imbalance, np.abs(e_q[s])[~(e_c[s] > 0)]])
        total = np.abs(flow[s]).sum() + (np.abs(e_q[s]).sum() if Ke else 0.0)
        if pdd is not None:
            imbalance = np.concatenate([imbalance, np.abs(d_q[s] - demand[s])[~fixed & ~d_on]])
            total += np.abs(d_q[s][d_on]).sum()
        worst = imbalance.max() if imbalance.size else 0.0
        mass[s] = worst / total if total > 0 else worst
        if with_links:
            arrays = link_law(network, None if speeds is None else speeds[s], None if closed is None else closed[s])
            if arrays is not None and network.has_valves:   # a valve CLOSED by its status obeys the shut law
                own = np.zeros(network.num_pipes, dtype=bool)
                own[network.valve_links[vstate[s] == VALVE_CLOSED]] = True
                arrays = dict(arrays, shut=arrays["shut"] | own)
            h = np.full(network.num_pipes, np.nan) if arrays is None else law(flow[s], _link_resistance(network, roughness[s]), **arrays)[0]
        else:
            h, _ = pipe_headloss(flow[s], _resistance(network, roughness[s]))
        e_link = np.abs(head[s][a] - head[s][b] - h)
        if network.has_valves:
            on = vstate[s] == VALVE_ACTIVE
            e_link[network.valve_links[on]] = np.abs(head[s][network.valve_node[on]] - (network.elevation[network.valve_node[on]] + settings[s][on]))
        if Ke and (e_c[s] > 0).any():
            on, i = e_c[s] > 0, network.emitter_nodes
            he = emitter_law(e_q[s][on], e_c[s][on], network.emitter_exponent)[0]
            e_link = np.concatenate([e_link, np.abs(head[s][i[on]] - network.elevation[i[on]] - he)])
        if pdd is not None and d_on.any():
            hd = demand_law(d_q[s][d_on], demand[s][d_on], pdd[2] - pdd[1], pdd[3])[0]
            e_link = np.concatenate([e_link, np.abs(head[s][d_on] - network.elevation[d_on] - pdd[1] - hd)])
        e_pipe = e_link.max()
        e_fixed = np.abs(head[s] - fh[s])[fixed].max()
        energy[s] = max(e_pipe, e_fixed) if not (np.isnan(e_pipe) or np.isnan(e_fixed)) else np.nan
    return mass, energy


def tree_solution(network: HydraulicNetwork, demand, roughness, fixed_head=None) -> Tuple[np.ndarray, np.ndarray]:
    """The exact answer on a tree with one fixed-head node, without Newton: a pipe's flow is the demand downstream of it, and the
    heads follow by path sums of ``pipe_headloss`` from the fixed node.  Returns (head [S, N], flow [S, P])."""
    N, P = network.num_nodes, network.num_pipes
    if P != N - 1 or network.fixed_nodes.size != 1:
        raise ValueError("tree_solution needs a tree (num_pipes == num_nodes - 1) with one fixed-head node")
    demand, roughness = np.asarray(demand, dtype=np.float64), np.asarray(roughness, dtype=np.float64)
    S = demand.shape[0]
    fh = _fixed_heads(network, fixed_head, S)
    root = int(network.fixed_nodes[0])
    adj = [[] for _ in range(N)]
    for p, (a, b) in enumerate(network.pipes):
        adj[a].append((int(b), p))
        adj[b].append((int(a), p))
    parent, parent_pipe, bfs = np.full(N, -1), np.full(N, -1), [root]
    seen = np.zeros(N, dtype=bool)
    seen[root] = True
    for v in bfs:
        for w, p in adj[v]:
            if not seen[w]:
                seen[w] = True
                parent[w], parent_pipe[w] = v, p
                bfs.append(w)
    head, flow = np.empty((S, N)), np.empty((S, P))
    for s in range(S):
        below = np.where(network.fixed, 0.0, demand[s]).copy()
        for v in reversed(bfs[1:]):
            below[parent[v]] += below[v]
        r = _resistance(network, roughness[s])
        head[s, root] = fh[s, root]
        for v in bfs[1:]:
            p = parent_pipe[v]
            sign = 1.0 if network.pipes[p, 1] == v else -1.0          # the pipe runs towards v: its flow is positive
            flow[s, p] = sign * below[v]
            h, _ = pipe_headloss(flow[s, p], r[p])
            head[s, v] = head[s, parent[v]] - sign * float(h)
    return head, flow


# ---- THE SENSITIVITIES on the host (gatres.h: THE SENSITIVITIES) --------------------------------------------------------------------
def roughness_gain(network: HydraulicNetwork, q, roughness, law) -> np.ndarray:
    """-h_C / g per link at the flows q under ``law`` (``link_law``): what a unit of Hazen-Williams coefficient moves the link's
    flow at fixed heads, ((1.852 ra) q) / (C g) with ra = r |q|^0.852; 0 for a pump, on a 1e8 branch and on the low-flow floor."""
    q, c = np.asarray(q, dtype=np.float64), np.asarray(roughness, dtype=np.float64)
    r = _link_resistance(network, c)
    _, g = link_headloss(q, r, **law)
    aq = np.abs(q)
    ra = r * np.power(aq, 0.852)
    live = ~(law["pump"] | law["shut"] | (law["check"] & (q < 0))) & ~(1.852 * ra + 2.0 * (law["minor"] * aq) < LINEAR_GRADIENT)
    with np.errstate(all="ignore"):
        return np.where(live, ((1.852 * ra) * q) / (c * g), 0.0)


def sensitivity_ref(network: HydraulicNetwork, demand, roughness, sensor_nodes, fixed_head=None, pump_speed=None, link_closed=None,
                    flow=None, solver: str = "dense", accuracy: float = ACCURACY,
                    max_iter: int = MAX_ITER) -> HydraulicSensitivityReference:
    """THE SENSITIVITIES in numpy fp64: (``dh_ddemand`` [S, K, N], ``dh_droughness`` [S, K, P]).  Per scenario the matrix A of the
    solver is built from THE LINK LAW's g at ``solve_ref``'s flows under the link law -- or at ``flow`` [S, P] where given (a
    device result's own flows isolate the linear algebra) -- with unit rows for the fixed-head nodes; dh_ddemand[k][n] =
    -(A^-1)[sensor k][n], 0 where either has a fixed head; dh_droughness[k][p] = (Z[k][a] - Z[k][b]) * ``roughness_gain``[p].
    ``solver``: "dense" (``numpy.linalg.solve`` in node order) or "banded" (``scipy.linalg.solveh_banded`` in solver order).  A
    failed scenario is NaN.  Emitters are taken as not leaking; regulating valves are refused."""
    if network.has_valves:
        raise ValueError("a network with regulating valves has no sensitivities here")
    if solver not in ("dense", "banded"):
        raise ValueError("solver must be 'dense' or 'banded'")
    demand, roughness = np.asarray(demand, dtype=np.float64), np.asarray(roughness, dtype=np.float64)
    sensors = np.asarray(sensor_nodes, dtype=np.int64).reshape(-1)
    S, N, P, K = demand.shape[0], network.num_nodes, network.num_pipes, sensors.size
    if K < 1 or sensors.min() < 0 or sensors.max() >= N:
        raise ValueError("sensor_nodes must be nodes of the network, at least one")
    if flow is None:
        flow = _solve_links_ref(network, demand, roughness, fixed_head, solver, accuracy, max_iter, pump_speed, link_closed).flow
    flow = np.asarray(flow, dtype=np.float64)
    speeds, closed = _link_rows(network, S, pump_speed, link_closed)
    a, b, fixed = network.pipes[:, 0].astype(np.int64), network.pipes[:, 1].astype(np.int64), network.fixed
    jj = ~fixed[a] & ~fixed[b]
    pos, W = network.position.astype(np.int64), network.half_bandwidth
    Z, dC = np.full((S, K, N), np.nan), np.full((S, K, P), np.nan)
    rhs = np.zeros((N, K))
    rhs[sensors, np.arange(K)] = np.where(fixed[sensors], 0.0, 1.0)
    for s in range(S):
        law = link_law(network, None if speeds is None else speeds[s], None if closed is None else closed[s])
        if law is None or not np.isfinite(flow[s]).all():
            continue
        _, g = link_headloss(flow[s], _link_resistance(network, roughness[s]), **law)
        pinv = 1.0 / g
        diag = np.zeros(N)
        for p in range(P):                                  # a row's sum runs over its pipes in pipe order, as in the kernel
            diag[a[p]] += pinv[p]
            diag[b[p]] += pinv[p]
        diag[fixed] = 1.0
        try:
            if solver == "dense":
                A = np.zeros((N, N))
                A[np.arange(N), np.arange(N)] = diag
                np.add.at(A, (a[jj], b[jj]), -pinv[jj])
                np.add.at(A, (b[jj], a[jj]), -pinv[jj])
                X = np.linalg.solve(A, rhs)
            else:
                from scipy.linalg import solveh_banded
                ab = np.zeros((W + 1, N))
                ab[0, pos] = diag
                hi, lo = np.maximum(pos[a[jj]], pos[b[jj]]), np.minimum(pos[a[jj]], pos[b[jj]])
                np.add.at(ab, (hi - lo, lo), -pinv[jj])
                Xb = np.empty((N, K))
                Xb[pos] = rhs
                X = solveh_banded(ab, Xb, lower=True)[pos]
        except (np.linalg.LinAlgError, ValueError):
            continue
        z = np.where(fixed[None, :] | fixed[sensors][:, None], 0.0, 0.0 - X.T)          # (0.0 - x: a zero stays +0.0)
        Z[s] = z
        dC[s] = (z[:, a] - z[:, b]) * roughness_gain(network, flow[s], roughness[s], law)[None, :]
    return HydraulicSensitivityReference(Z, dC)


def leak_scores_ref(dh_ddemand, residual) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The fused localisation of ``gatres_hydraulic_sensitivity`` in numpy, with the kernel's operations in the kernel's order:
    ``dh_ddemand`` [..., K, N] and ``residual`` [..., K] (NaN: the sensor is missing) give (score [..., N], leak_flow [..., N],
    best int32 [...]).  <z_n, rho>, <z_n, z_n> and <rho, rho> run over the available k ascending, product and sum rounded on their
    own; leak_flow = <z, rho> / <z, z>, score = <z, rho> / (sqrt(<z, z>) * sqrt(<rho, rho>)); both NaN where <z, z> == 0 (a
    fixed-head node has a column of zeros) or the matrix is NaN; every score NaN where <rho, rho> == 0 or no sensor is available;
    best: the lowest index among those holding the largest score, -1 where there is none."""
    Z, rho = np.asarray(dh_ddemand, dtype=np.float64), np.asarray(residual, dtype=np.float64)
    K, N = Z.shape[-2:]
    lead = Z.shape[:-2]
    Z, rho = Z.reshape(-1, K, N), rho.reshape(-1, K)
    num, den, r2, cnt = np.zeros((Z.shape[0], N)), np.zeros((Z.shape[0], N)), np.zeros(Z.shape[0]), np.zeros(Z.shape[0])
    with np.errstate(all="ignore"):
        for k in range(K):
            on = ~np.isnan(rho[:, k])
            rk = np.where(on, rho[:, k], 0.0)
            num = np.where(on[:, None], num + Z[:, k, :] * rk[:, None], num)
            den = np.where(on[:, None], den + Z[:, k, :] * Z[:, k, :], den)
            r2 = np.where(on, r2 + rk * rk, r2)
            cnt += on
        off = (den == 0.0) | np.isnan(den)
        leak = np.where(off, np.nan, num / den)
        none = (cnt == 0) | (r2 == 0.0)
        score = np.where(off | none[:, None], np.nan, num / (np.sqrt(den) * np.sqrt(r2)[:, None]))
    return score.reshape(lead + (N,)), leak.reshape(lead + (N,)), best_score_ref(score).reshape(lead)


def best_score_ref(score) -> np.ndarray:
    """THE TIE RULE of ``best``: per row of ``score`` [..., N] the lowest index among those holding the maximum, NaN taking no part;
    -1 where every score is NaN."""
    score = np.asarray(score, dtype=np.float64)
    live = ~np.isnan(score)
    best = np.argmax(np.where(live, score, -np.inf), axis=-1).astype(np.int32)        # (argmax takes the first of equals)
    return np.where(live.any(axis=-1), best, np.int32(-1)).astype(np.int32)


def hop_distances(network: HydraulicNetwork, source: int) -> np.ndarray:
    """Links between ``source`` and every node of the network's graph (every link counts, whatever its state); -1 where no path is."""
    N = network.num_nodes
    adj = [[] for _ in range(N)]
    for a, b in network.pipes:
        adj[int(a)].append(int(b))
        adj[int(b)].append(int(a))
    dist = np.full(N, -1, dtype=np.int64)
    dist[int(source)] = 0
    queue = [int(source)]
    for v in queue:
        for w in adj[v]:
            if dist[w] < 0:
                dist[w] = dist[v] + 1
                queue.append(w)
    return dist


def localization_report(network: HydraulicNetwork, localization: LeakLocalization, true_node, tolerance: float = 1e-9) -> Dict[str, np.ndarray]:
    """How a ``LeakLocalization`` did against the labels, with ONE read-back (scores and best together).  ``true_node``: the leaking
    node, one for all scenarios or [S].  Per scenario: ``hops`` the links between ``best`` and the true node (-1 where best is -1);
    ``deficit`` the top score minus the true node's score (0: the true node is among the best; NaN where there is no score);
    ``above`` how many candidates score more than ``tolerance`` above the true node; and ``best`` itself.  Columns of junctions
    behind the same sensor cut are proportional, so a deficit at rounding level with hops > 0 is all that the sensors can tell."""
    score, best = localization.score, localization.best
    S, N = int(score.shape[0]), network.num_nodes
    back = torch.cat([score, best.to(torch.float64)[:, None]], dim=1).cpu().numpy()            # the one read-back
    score, best = back[:, :N], back[:, N].astype(np.int64)
    true = np.broadcast_to(np.asarray(true_node, dtype=np.int64), (S,))
    if true.min() < 0 or true.max() >= N:
        raise ValueError("true_node must be a node of the network")
    hops = np.full(S, -1, dtype=np.int64)
    for t in np.unique(true):
        rows = (true == t) & (best >= 0)
        hops[rows] = hop_distances(network, int(t))[best[rows]]
    mine = score[np.arange(S), true]
    live = ~np.isnan(score)
    with np.errstate(all="ignore"):
        top = np.where(live.any(axis=1), np.where(live, score, -np.inf).max(axis=1), np.nan)
        above = (live & (score > (mine + float(tolerance))[:, None])).sum(axis=1)
    return {"hops": hops, "deficit": top - mine, "above": above, "best": best}
