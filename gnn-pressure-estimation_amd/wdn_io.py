"""On-disk formats on either side of the hot path: what the reference's ``WDNDataset.collect``
(gnn_pressure_estimation/utils/DataLoader.py:206-258) reads and what its checkpoints hold, without wntr / zarr /
numcodecs / torch_geometric -- none of them is installable here.

* ``parse_inp`` / ``inp_edge_index``: the topology of an EPANET ``.inp`` file as the ``edge_index`` the reference feeds its
  models.  The reference builds it as ``pgu.from_networkx(nx.Graph(wn.to_graph()).to_undirected().subgraph(keep).copy())``
  (DataLoader.py:28-37, :236-254); the node and edge ORDER that pipeline produces is restated here step by step (it
  decides the order of every neighbour sum, hence the last bits of every fp32 result).  The networkx part is checked
  against networkx itself in tests/test_wdn_io.py; the wntr part (registry order: junctions, reservoirs, tanks; pipes,
  pumps, valves; ``to_graph`` adding one edge per link from start node to end node) is from the author's knowledge of
  wntr >= 0.4 and cannot be verified in this container.
* ``ZarrZip``: reader for the zarr-v2 ``ZipStore`` the scenario generator writes (scenegenv7.py:701-725):
  ``root[feature][split]`` arrays, C order, chunked, compressor ``null`` / ``zlib`` / ``blosc`` (Blosc-1 container with the
  lz4, lz4hc, zlib or memcpy codecs and the byte-shuffle filter; zarr's default is Blosc(lz4, shuffle)).  The container
  and the LZ4 block format are implemented from their published specifications; no real zarr output exists in this
  container to read back, so the committed fixture is written by this module's own (test-side) encoder.
* ``save_checkpoint`` / ``load_checkpoint``: the ``.pth`` dict of train.py:433-451 / utils/auxil.py:206-233, plus the
  conversion between ``GATResTrainer``'s flat Adam moments and ``torch.optim.Adam.state_dict()`` so a run can move
  between the reference loop and the native trainer.
* ``load_wdn``: the three together -> ``(SnapshotStore, node_names)``.
"""
from __future__ import annotations

import io
import json
import struct
import zipfile
import zlib
from collections import OrderedDict, namedtuple
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import os
import warnings

import numpy as np
import torch

from . import _native

# ---------------------------------------------------------------------------------------------------------------- .inp
_NODE_SECTIONS = ("JUNCTIONS", "RESERVOIRS", "TANKS")
_LINK_SECTIONS = ("PIPES", "PUMPS", "VALVES")


def parse_inp(source=None, *, text: Optional[str] = None) -> Dict[str, list]:
    """Topology sections of an EPANET input file.  ``source``: a path (``str`` / ``os.PathLike``); ``text=``: the file's
    text instead.  (A ``str`` that is not an existing path but contains a newline is still taken as text, as before; a path
    with brackets in it -- ``/data/run[1]/ctown.inp`` -- is a path.)  Returns
    ``{"JUNCTIONS": [id, ...], "RESERVOIRS": [...], "TANKS": [...], "PIPES": [(id, node1, node2), ...], "PUMPS": [...],
    "VALVES": [...]}`` in file order.  ``;`` starts a comment, section names are case-insensitive, ids are the first
    whitespace-separated tokens of a line (EPANET 2.2 users manual, appendix C).  Raises if the text has no
    ``[JUNCTIONS]`` section (not an EPANET input file)."""
    if (source is None) == (text is None):
        raise ValueError("parse_inp: give a path OR text=")
    if text is None:
        if isinstance(source, os.PathLike) or os.path.exists(str(source)) or "\n" not in str(source):
            with open(source, "r", encoding="latin-1") as f:       # (a missing file raises FileNotFoundError here)
                text = f.read()
        else:
            text = str(source)
    out: Dict[str, list] = {k: [] for k in _NODE_SECTIONS + _LINK_SECTIONS}
    section = None
    seen_sections = set()
    for raw in str(text).splitlines():
        line = raw.split(";", 1)[0].strip()
        if not line:
            continue
        if line.startswith("["):
            section = line.strip("[]").strip().upper()
            seen_sections.add(section)
            continue
        tok = line.split()
        if section in _NODE_SECTIONS:
            out[section].append(tok[0])
        elif section in _LINK_SECTIONS:
            if len(tok) < 3:
                raise ValueError(f"[{section}] line needs an id and two node ids: {raw!r}")
            out[section].append((tok[0], tok[1], tok[2]))
        if section is not None:
            seen_sections.add(section)
    if "JUNCTIONS" not in seen_sections:
        raise ValueError("no [JUNCTIONS] section: not an EPANET .inp file")
    return out


def _readd(nodes: Sequence[str], adj: "OrderedDict[str, list]") -> "OrderedDict[str, list]":
    """What ``Graph.copy()`` / ``to_undirected()`` / ``subgraph().copy()`` do to the adjacency ORDER: nodes are re-inserted in
    order, then every (u, v) of ``for u in adj: for v in adj[u]`` is re-added, which appends v to u's list AND u to v's
    list if not there yet -- so a node's neighbours that come earlier in the node order end up first."""
    new = OrderedDict((n, []) for n in nodes)
    seen = {n: set() for n in nodes}
    for u in nodes:
        for v in adj[u]:
            if v not in seen[u]:
                seen[u].add(v); new[u].append(v)
            if u not in seen[v]:
                seen[v].add(u); new[v].append(u)
    return new


def inp_edge_index(inp: Dict[str, list], removal: str = "keep_junction") -> Tuple[torch.Tensor, List[str]]:
    """``edge_index`` int64 [2, E] (both directions of every link, grouped by source node) and the kept node names, in the
    order ``get_graph_template(nx.Graph(wn.to_graph()).to_undirected().subgraph(keep_list).copy())`` yields
    (DataLoader.py:28-37, :230-254).  ``removal``: ``keep_junction`` (train.py's default, :597-603), ``keep_all``,
    ``reservoir`` (drop reservoirs) or ``tank`` (drop tanks)."""
    nodes = list(inp["JUNCTIONS"]) + list(inp["RESERVOIRS"]) + list(inp["TANKS"])        # wntr node registry order
    links = list(inp["PIPES"]) + list(inp["PUMPS"]) + list(inp["VALVES"])                 # wntr link registry order
    index = {n: i for i, n in enumerate(nodes)}
    if len(index) != len(nodes):
        raise ValueError("duplicate node id in the .inp file")
    # wn.to_graph(): MultiDiGraph, one edge start -> end per link in registry order => successor lists in link order
    succ = OrderedDict((n, []) for n in nodes)
    for _, a, b in links:
        if a not in index or b not in index:
            raise ValueError(f"link endpoint {a!r} / {b!r} is not a node")
        succ[a].append(b)
    # nx.Graph(multidigraph): add_edge(u, v) for u in node order, v in successor order (parallel links collapse)
    adj = OrderedDict((n, []) for n in nodes)
    seen = {n: set() for n in nodes}
    for u in nodes:
        for v in succ[u]:
            if v not in seen[u]:
                seen[u].add(v); adj[u].append(v)
            if u not in seen[v]:
                seen[v].add(u); adj[v].append(u)
    adj = _readd(nodes, adj)                                                               # .to_undirected()
    subgraph = True
    if removal == "keep_junction":
        keep = set(inp["JUNCTIONS"])
    elif removal == "keep_all":
        keep, subgraph = set(nodes), False
    elif removal == "reservoir":           # (get_keep_list: no reservoirs / tanks = no keep list = the graph itself)
        keep, subgraph = set(nodes) - set(inp["RESERVOIRS"]), bool(inp["RESERVOIRS"])
    elif removal == "tank":
        keep, subgraph = set(nodes) - set(inp["TANKS"]), bool(inp["TANKS"])
    else:
        raise ValueError(f"removal {removal!r}: use keep_junction / keep_all / reservoir / tank")
    kept = [n for n in nodes if n in keep]
    if subgraph and 2 * len(keep) < len(nodes):
        # networkx walks the KEEP SET (hash order of the names) instead of the graph when it is the smaller one
        # (FilterAtlas.__iter__): the reference's node order is then arbitrary from run to run
        warnings.warn("fewer than half of the nodes are kept: the reference's node order is undefined here (networkx "
                      "iterates the keep set); using the .inp registry order", stacklevel=2)
    sub = OrderedDict((n, [v for v in adj[n] if v in keep]) for n in kept)
    if subgraph:
        sub = _readd(kept, sub)                                                            # .subgraph(keep).copy()
    # from_networkx: to_directed() keeps adjacency order; edges() = for u in nodes: for v in succ[u]
    new_id = {n: i for i, n in enumerate(kept)}
    src = [new_id[u] for u in kept for _ in sub[u]]
    dst = [new_id[v] for u in kept for v in sub[u]]
    return torch.tensor([src, dst], dtype=torch.int64).reshape(2, -1), kept


def inp_node_order(inp: Dict[str, list]) -> List[str]:
    """``wn.node_name_list``: the column order of the zarr arrays (DataLoader.py:243-249)."""
    return list(inp["JUNCTIONS"]) + list(inp["RESERVOIRS"]) + list(inp["TANKS"])


# ------------------------------------------------------------------------------------------------- .inp: hydraulics
# flow units -> m3/s (EPANET 2.2 users manual, appendix A); the first five are SI (metres, millimetres), the others US customary
# (feet for lengths, elevations and heads, inches for diameters)
_GALLON, _FOOT = 3.785411784e-3, 0.3048
FLOW_UNITS = {"LPS": 1e-3, "LPM": 1e-3 / 60.0, "MLD": 1e3 / 86400.0, "CMH": 1.0 / 3600.0, "CMD": 1.0 / 86400.0,
              "GPM": _GALLON / 60.0, "CFS": _FOOT ** 3, "MGD": 1e6 * _GALLON / 86400.0}
_SI_UNITS = ("LPS", "LPM", "MLD", "CMH", "CMD")
_REGULATING = ("PRV", "PSV", "PBV", "FCV", "GPV")
_PSI_PER_FOOT, _KPA_PER_PSI = 0.4333, 6.895     # EPANET's own constants for a pressure in psi or kPa
NOMINAL_ROUGHNESS = 100.0               # what a pump or a valve gets in the roughness row: it has no resistance and it is not read
NOMINAL_PUMP_DIAMETER = 1.0             # metres: a pump has no diameter; HydraulicNetwork asks for one and reads it nowhere

InpHydraulics = namedtuple("InpHydraulics", "network demand roughness multipliers pattern_of_node pump_speed node_names link_names "
                                            "pattern_names emitter_coefficient demand_model minimum_pressure required_pressure "
                                            "pressure_exponent controls", defaults=(None,) * 5 + ((),))


def _inp_sections(source, text) -> "OrderedDict[str, list]":
    """Every section of an EPANET input file as its token lists, comments stripped, in file order."""
    if (source is None) == (text is None):
        raise ValueError("give a path OR text=")
    if text is None:
        if isinstance(source, os.PathLike) or os.path.exists(str(source)) or "\n" not in str(source):
            with open(source, "r", encoding="latin-1") as f:
                text = f.read()
        else:
            text = str(source)
    out: "OrderedDict[str, list]" = OrderedDict()
    section = None
    for raw in str(text).splitlines():
        line = raw.split(";", 1)[0].strip()
        if not line:
            continue
        if line.startswith("["):
            section = line.strip("[]").strip().upper()
            out.setdefault(section, [])
        elif section is not None:
            out[section].append(line.split())
    if "JUNCTIONS" not in out:
        raise ValueError("no [JUNCTIONS] section: not an EPANET .inp file")
    return out


def parse_inp_hydraulics(source=None, *, text: Optional[str] = None, unsupported_valves: str = "refuse", ignore_controls: bool = False,
                         device=None, regulating: Optional[str] = None, emitters: Optional[str] = None,
                         demand_model: Optional[str] = None, controls: Optional[str] = None) -> "InpHydraulics":
    """The hydraulic attributes of an EPANET input file as a ``hydraulics.HydraulicNetwork`` and the arrays ``simulate`` and
    ``simulate_series`` take, in SI units.  Read: [JUNCTIONS] (elevation, base demand, pattern), [RESERVOIRS] (head), [TANKS]
    (elevation, initial, minimum and maximum level, diameter), [PIPES] (length, diameter, roughness, minor loss, Open / Closed /
    CV), [PUMPS] (``HEAD`` curve, ``SPEED``), [CURVES], [VALVES] (TCV: the setting is its loss coefficient), [STATUS] (Open,
    Closed, or a pump's speed), [PATTERNS] and of [OPTIONS] ``UNITS``, ``HEADLOSS`` and ``PATTERN``.  Nodes come in the order
    junctions, reservoirs, tanks, links in the order pipes, pumps, valves, each in file order; a link runs from its first node
    to its second.  Returns ``InpHydraulics``: network; demand [N] m3/s; roughness [P] (``NOMINAL_ROUGHNESS`` for pumps and
    valves); multipliers [M, T], row 0 the constant pattern 1 and then the file's patterns, the shorter ones repeated up to the
    longest, as EPANET wraps them; pattern_of_node int32 [N] (a junction without a pattern takes the default pattern of
    [OPTIONS], "1" if there is one, else row 0); pump_speed [Kp] (0 for a pump that [STATUS] closes); the names.

    Refused with a ``ValueError`` that names the offender: flow units other than ``FLOW_UNITS``, a head-loss formula other than
    H-W, a ``POWER`` pump or one without a ``HEAD`` curve, a regulating valve (PRV, PSV, PBV, FCV, GPV) unless
    ``unsupported_valves="open"``, which makes it an open link with its minor loss, [CONTROLS] or [RULES] with content unless
    ``ignore_controls=True``.  What EPANET does with the rest of the file (demand multiplier, emitters unless ``emitters="model"``,
    the demand model unless ``demand_model="model"``, quality, energy, times) is not read.

    ``regulating="model"`` (default ``None``: everything above, as it always was) makes PRV and PSV valves the regulating valves
    of ``hydraulics`` (THE REGULATING VALVES): the valve runs from its first node to its second, its setting is a pressure in the
    file's pressure unit, converted to metres (SI flow units: metres, or kPa with ``PRESSURE KPA``; US units: psi), and its loss
    coefficient may be 0.  [STATUS] may close such a valve (a shut link); a fixed OPEN status is refused by name.  FCV, PBV and
    GPV still go by ``unsupported_valves``.

    ``emitters="model"`` (default ``None``: [EMITTERS] is not read, as it always was -- a leaky file is then simulated as tight)
    makes the lines of [EMITTERS] the emitters of ``hydraulics`` (THE EMITTERS), in file order, with the exponent of [OPTIONS]
    ``EMITTER EXPONENT`` (default 0.5).  A coefficient is a flow in the file's flow unit at one pressure unit (metres, kPa or psi,
    as for ``regulating``); the result's ``emitter_coefficient`` [Ke] holds C * flow unit / (metres per pressure unit)^exponent,
    m3/s per m^exponent.  Refused by name: an emitter on a reservoir or a tank, on no node, or listed twice, and a coefficient
    that is negative or not finite.

    ``demand_model="model"`` (default ``None``: the four options are not read, as they never were -- a file that asks for PDA is
    then simulated demand-driven) takes from [OPTIONS] ``DEMAND MODEL`` (``DDA``, the default, or ``PDA``), ``MINIMUM PRESSURE``
    (default 0), ``REQUIRED PRESSURE`` (default 0.1) and ``PRESSURE EXPONENT`` (default 0.5), the pressures converted to metres
    as for ``regulating``.  The result's ``demand_model`` is "dda" or "pda" and its ``minimum_pressure``, ``required_pressure`` and
    ``pressure_exponent`` are what ``simulate(demand_model=...)`` takes (THE PRESSURE-DRIVEN DEMAND).  Refused by name: a
    ``DEMAND MODEL`` word other than DDA or PDA, a value that is not finite, an exponent that is not positive and, with PDA, a
    required pressure less than 0.1 m above the minimum pressure.  What is still not read: the demand multiplier, quality,
    energy, times.

    ``controls="model"`` (default ``None``: [CONTROLS] with content is refused, as it always was, and ``ignore_controls=True`` still
    drops it) reads the simple controls of [CONTROLS] for ``hydraulics`` (THE CONTROLS): lines of the forms
    ``LINK id OPEN|CLOSED|<number> IF NODE id ABOVE|BELOW <number>`` and ``LINK id OPEN|CLOSED|<number> AT TIME <hours | H:MM>``,
    in file order.  A number is a pump's speed or, with ``regulating="model"``, a PRV's or PSV's setting in the file's pressure
    unit.  The value of a tank is a level in the file's length unit, that of a junction a pressure in the file's pressure unit,
    converted as for ``regulating``.  The result's ``controls`` is a tuple of what ``hydraulics.control_table`` takes; AT TIME is
    kept in seconds, as ``(link, action, "at_time", seconds)``, and ``control_table(network, controls, step_seconds)`` turns it into
    a step, refusing a time that is no whole number of steps.  Refused by name: ``AT CLOCKTIME``, a line of another form, an
    unknown link or node, a number on a link that takes no setting, and everything ``control_table`` refuses (a control on a CV
    pipe, a reservoir as the node).  [RULES] with content is still refused."""
    from . import hydraulics as H
    if demand_model not in (None, "model"):
        raise ValueError('demand_model must be None or "model"')
    if emitters not in (None, "model"):
        raise ValueError('emitters must be None or "model"')
    if unsupported_valves not in ("refuse", "open"):
        raise ValueError('unsupported_valves must be "refuse" or "open"')
    if regulating not in (None, "model"):
        raise ValueError('regulating must be None or "model"')
    if controls not in (None, "model"):
        raise ValueError('controls must be None or "model"')
    sec = _inp_sections(source, text)
    options = {" ".join(t[:-1]).upper(): t[-1] for t in sec.get("OPTIONS", []) if len(t) >= 2}
    units = options.get("UNITS", "GPM").upper()
    if units not in FLOW_UNITS:
        raise ValueError(f"[OPTIONS] UNITS {units}: flow units must be one of {sorted(FLOW_UNITS)}")
    formula = options.get("HEADLOSS", "H-W").upper()
    if formula != "H-W":
        raise ValueError(f"[OPTIONS] HEADLOSS {formula}: only the Hazen-Williams formula (H-W) is modelled")
    for name in ("CONTROLS", "RULES"):
        if sec.get(name) and not ignore_controls and not (name == "CONTROLS" and controls == "model"):
            raise ValueError(f"[{name}] has {len(sec[name])} lines: controls and rules are not modelled (ignore_controls=True drops them)")
    flow = FLOW_UNITS[units]
    metre, dia = (1.0, 1e-3) if units in _SI_UNITS else (_FOOT, _FOOT / 12.0)
    num = lambda tok, i, default=0.0: float(tok[i]) if len(tok) > i else default
    pressure_unit = options.get("PRESSURE", "METERS" if units in _SI_UNITS else "PSI").upper()
    if (regulating or emitters or demand_model or controls) and pressure_unit not in (("METERS", "KPA") if units in _SI_UNITS else ("PSI",)):
        raise ValueError(f"[OPTIONS] PRESSURE {pressure_unit} does not go with UNITS {units}")
    pressure = {"METERS": 1.0, "PSI": _FOOT / _PSI_PER_FOOT, "KPA": _FOOT / _PSI_PER_FOOT / _KPA_PER_PSI}[pressure_unit] if (regulating or emitters or demand_model or controls) else 1.0

    # nodes
    names, elevation, demand, pattern_id = [], [], [], []
    for t in sec["JUNCTIONS"]:
        names.append(t[0]); elevation.append(num(t, 1) * metre); demand.append(num(t, 2) * flow); pattern_id.append(t[3] if len(t) > 3 else None)
    fixed_nodes, fixed_head, tanks, t_dia, t_min, t_max = [], [], [], [], [], []
    for t in sec.get("RESERVOIRS", []):
        fixed_nodes.append(len(names)); fixed_head.append(num(t, 1) * metre)
        names.append(t[0]); elevation.append(num(t, 1) * metre); demand.append(0.0); pattern_id.append(None)
    for t in sec.get("TANKS", []):
        if len(t) < 6:
            raise ValueError(f"[TANKS] {t[0]}: needs elevation, initial, minimum and maximum level and diameter")
        fixed_nodes.append(len(names)); fixed_head.append((num(t, 1) + num(t, 2)) * metre)
        tanks.append(len(names)); t_min.append(num(t, 3) * metre); t_max.append(num(t, 4) * metre); t_dia.append(num(t, 5) * metre)
        names.append(t[0]); elevation.append(num(t, 1) * metre); demand.append(0.0); pattern_id.append(None)
    index = {n: i for i, n in enumerate(names)}
    if len(index) != len(names):
        raise ValueError("a node id appears twice")

    # links: pipes, pumps, valves
    links, ends, length, diameter, rough, minor, check, closed = [], [], [], [], [], [], [], []

    def add(section, t, L, D, C, K, cv=False, shut=False):
        for n in t[1:3]:
            if n not in index:
                raise ValueError(f"[{section}] {t[0]}: no node {n}")
        links.append(t[0]); ends.append((index[t[1]], index[t[2]])); length.append(L); diameter.append(D); rough.append(C)
        minor.append(K); check.append(cv); closed.append(shut)

    for t in sec.get("PIPES", []):
        if len(t) < 6:
            raise ValueError(f"[PIPES] {t[0]}: needs two nodes, length, diameter and roughness")
        status = t[7].upper() if len(t) > 7 else "OPEN"
        if status not in ("OPEN", "CLOSED", "CV"):
            raise ValueError(f"[PIPES] {t[0]}: status {t[7]}")
        add("PIPES", t, num(t, 3) * metre, num(t, 4) * dia, num(t, 5), num(t, 6), status == "CV", status == "CLOSED")
    curves: Dict[str, list] = {}
    for t in sec.get("CURVES", []):
        if len(t) < 3:
            raise ValueError(f"[CURVES] {t[0]}: needs an x and a y")
        curves.setdefault(t[0], []).append((float(t[1]), float(t[2])))
    pump_links, pump_curve, pump_speed = [], [], []
    for t in sec.get("PUMPS", []):
        if len(t) < 5 or len(t) % 2 == 0:
            raise ValueError(f"[PUMPS] {t[0]}: needs two nodes and keyword-value pairs")
        props = {t[i].upper(): t[i + 1] for i in range(3, len(t), 2)}
        if "POWER" in props:
            raise ValueError(f"[PUMPS] {t[0]}: a POWER pump is not modelled, give it a HEAD curve")
        if "HEAD" not in props or props["HEAD"] not in curves:
            raise ValueError(f"[PUMPS] {t[0]}: needs a HEAD curve that [CURVES] defines")
        pts = curves[props["HEAD"]]
        try:
            pump_curve.append(H.pump_curve_from_points([q * flow for q, _ in pts], [h * metre for _, h in pts]))
        except ValueError as err:
            raise ValueError(f"[PUMPS] {t[0]}, curve {props['HEAD']}: {err}") from None
        pump_links.append(len(links)); pump_speed.append(float(props.get("SPEED", 1.0)))
        add("PUMPS", t, 0.0, NOMINAL_PUMP_DIAMETER, NOMINAL_ROUGHNESS, 0.0)
    valve_links, valve_kind, valve_setting = [], [], []
    for t in sec.get("VALVES", []):
        if len(t) < 6:
            raise ValueError(f"[VALVES] {t[0]}: needs two nodes, diameter, type and setting")
        kind, K = t[4].upper(), num(t, 6)
        if kind == "TCV":
            K = max(K, float(t[5]))
        elif regulating == "model" and kind in ("PRV", "PSV"):
            valve_links.append(len(links)); valve_kind.append(kind); valve_setting.append(float(t[5]) * pressure)
            add("VALVES", t, 0.0, num(t, 3) * dia, NOMINAL_ROUGHNESS, K)
            continue
        elif kind in _REGULATING and unsupported_valves == "open":
            pass
        else:
            raise ValueError(f'[VALVES] {t[0]}: a {kind} valve is not modelled (unsupported_valves="open" makes it an open link)')
        if not K > 0:
            raise ValueError(f"[VALVES] {t[0]}: an open valve without a loss coefficient has no head-loss law")
        add("VALVES", t, 0.0, num(t, 3) * dia, NOMINAL_ROUGHNESS, K)
    link_index = {n: i for i, n in enumerate(links)}
    if len(link_index) != len(links):
        raise ValueError("a link id appears twice")
    for t in sec.get("STATUS", []):
        if len(t) < 2 or t[0] not in link_index:
            raise ValueError(f"[STATUS] {t[0]}: no such link")
        p, word = link_index[t[0]], t[1].upper()
        k = pump_links.index(p) if p in pump_links else None
        if word in ("OPEN", "CLOSED"):
            if word == "OPEN" and p in valve_links:        # (EPANET: fixed open, the setting overridden; not modelled)
                raise ValueError(f"[STATUS] {t[0]}: a fixed OPEN status of a regulating valve is not modelled")
            if k is None:
                closed[p] = word == "CLOSED"
            elif word == "CLOSED":
                pump_speed[k] = 0.0
        elif k is not None:
            pump_speed[k] = float(t[1])
        else:
            raise ValueError(f"[STATUS] {t[0]}: a setting for a link that is no pump")

    # patterns: row 0 is the constant 1
    pats: "OrderedDict[str, list]" = OrderedDict()
    for t in sec.get("PATTERNS", []):
        pats.setdefault(t[0], []).extend(float(x) for x in t[1:])
    T = max([len(v) for v in pats.values()] + [1])
    mult = np.ones((1 + len(pats), T))
    for i, v in enumerate(pats.values()):
        if not v:
            raise ValueError(f"[PATTERNS] {list(pats)[i]}: no multipliers")
        mult[1 + i] = np.resize(np.asarray(v), T)
    row = {n: 1 + i for i, n in enumerate(pats)}
    default = row.get(options.get("PATTERN", "1"), 0)
    pattern_of_node = np.zeros(len(names), dtype=np.int32)
    for i, pid in enumerate(pattern_id):
        if pid is not None and pid not in row:
            raise ValueError(f"[JUNCTIONS] {names[i]}: no pattern {pid}")
        pattern_of_node[i] = default if pid is None else row[pid]
    pattern_of_node[fixed_nodes] = 0

    ends_a = np.asarray(ends, dtype=np.int64).reshape(-1, 2)
    if (ends_a[:, 0] == ends_a[:, 1]).any():
        raise ValueError(f"link {links[int(np.flatnonzero(ends_a[:, 0] == ends_a[:, 1])[0])]} joins a node to itself")
    lo, hi = ends_a.min(axis=1), ends_a.max(axis=1)
    edge_index = torch.from_numpy(np.stack([np.concatenate([lo, hi]), np.concatenate([hi, lo])]))
    kw = {}
    if tanks:
        kw.update(tank_nodes=tanks, tank_diameter=t_dia, tank_min_level=t_min, tank_max_level=t_max)
    if pump_links:
        h0, rp, n = (np.asarray(v) for v in zip(*pump_curve))
        kw.update(pump_links=pump_links, pump_h0=h0, pump_r=rp, pump_n=n)
    if valve_links:
        kw.update(valve_links=valve_links, valve_kind=valve_kind, valve_setting=valve_setting)
    emitter_coefficient = None
    if emitters == "model":
        gamma = float(options.get("EMITTER EXPONENT", 0.5))
        e_nodes, e_coef = [], []
        for t in sec.get("EMITTERS", []):
            if len(t) < 2:
                raise ValueError(f"[EMITTERS] {t[0]}: needs a junction and a coefficient")
            if t[0] not in index:
                raise ValueError(f"[EMITTERS] {t[0]}: no such node")
            if index[t[0]] in fixed_nodes:
                raise ValueError(f"[EMITTERS] {t[0]}: an emitter sits on a junction, not on a reservoir or a tank")
            if index[t[0]] in e_nodes:
                raise ValueError(f"[EMITTERS] {t[0]}: listed twice")
            c = float(t[1])
            if not (np.isfinite(c) and c >= 0):
                raise ValueError(f"[EMITTERS] {t[0]}: the coefficient {t[1]} must be finite and not negative")
            e_nodes.append(index[t[0]]); e_coef.append(c * flow / pressure ** gamma)
        kw.update(emitter_nodes=e_nodes, emitter_exponent=gamma)
        emitter_coefficient = np.asarray(e_coef, dtype=np.float64)
    pdd = (None,) * 4
    if demand_model == "model":
        word = options.get("DEMAND MODEL", "DDA").upper()
        if word not in ("DDA", "PDA"):
            raise ValueError(f"[OPTIONS] DEMAND MODEL {word}: the demand model must be DDA or PDA")
        values = {}
        for key, default in (("MINIMUM PRESSURE", 0.0), ("REQUIRED PRESSURE", 0.1), ("PRESSURE EXPONENT", 0.5)):
            try:
                values[key] = float(options.get(key, default))
            except ValueError:
                values[key] = float("nan")
            if not np.isfinite(values[key]):
                raise ValueError(f"[OPTIONS] {key} {options.get(key)}: must be a finite number")
        p_min, p_req, e = values["MINIMUM PRESSURE"] * pressure, values["REQUIRED PRESSURE"] * pressure, values["PRESSURE EXPONENT"]
        if not (e > 0 and np.isfinite(1.0 / e)):
            raise ValueError(f"[OPTIONS] PRESSURE EXPONENT {options.get('PRESSURE EXPONENT')}: must be positive")
        if word == "PDA" and not p_req - p_min >= H.MIN_PRESSURE_DIFFERENCE:
            raise ValueError(f"[OPTIONS] REQUIRED PRESSURE {options.get('REQUIRED PRESSURE', 0.1)}: must lie at least "
                             f"{H.MIN_PRESSURE_DIFFERENCE} m above MINIMUM PRESSURE {options.get('MINIMUM PRESSURE', 0)} "
                             f"({p_req:.6g} m against {p_min:.6g} m)")
        pdd = (word.lower(), p_min, p_req, e)
    network = H.HydraulicNetwork(edge_index, length, diameter, elevation, fixed_nodes, fixed_head, device=device, minor_loss=minor,
                                 check_valve=check, closed=closed, link_reversed=ends_a[:, 0] > ends_a[:, 1], **kw)
    rows = []
    if controls == "model" and not ignore_controls:
        for i, t in enumerate(sec.get("CONTROLS", [])):
            where = f"[CONTROLS] line {i + 1} ({' '.join(t)})"
            w = [x.upper() for x in t]
            if "CLOCKTIME" in w:
                raise ValueError(f"{where}: AT CLOCKTIME is not modelled")
            timed = len(w) == 6 and w[3] == "AT" and w[4] == "TIME"
            if not (w and w[0] == "LINK" and (timed or (len(w) == 8 and w[3] == "IF" and w[4] == "NODE" and w[6] in ("ABOVE", "BELOW")))):
                raise ValueError(f"{where}: not of the form LINK id status IF NODE id ABOVE|BELOW value or LINK id status AT TIME t")
            if t[1] not in link_index:
                raise ValueError(f"{where}: no link {t[1]}")
            p = link_index[t[1]]
            if w[2] in ("OPEN", "CLOSED"):
                action = w[2].lower()
            else:
                try:
                    value = float(t[2])
                except ValueError:
                    raise ValueError(f"{where}: the status {t[2]} is neither OPEN, CLOSED nor a number") from None
                if p in pump_links:
                    action = ("setting", value)
                elif p in valve_links:
                    action = ("setting", value * pressure)
                else:
                    raise ValueError(f"{where}: link {t[1]} takes no setting")
            try:
                if timed:
                    hms = [float(x) for x in t[5].split(":")]
                    if len(hms) > 3 or not all(np.isfinite(x) and x >= 0 for x in hms):
                        raise ValueError
                    seconds = sum(x * f for x, f in zip(hms, (3600.0, 60.0, 1.0)))
                    rows.append((p, action, "at_time", seconds))
                    continue
                level = float(t[7])
            except ValueError:
                raise ValueError(f"{where}: {t[-1]} is no number") from None
            if t[5] not in index:
                raise ValueError(f"{where}: no node {t[5]}")
            n, side = index[t[5]], w[6].lower()
            if n in tanks:
                rows.append((p, action, "tank_" + side, tanks.index(n), level * metre))
            else:
                rows.append((p, action, "node_" + side, n, level * pressure))
        for i, row in enumerate(rows):                      # everything control_table refuses, named by the file's line
            try:
                H.control_table(network, [row if row[2] != "at_time" else (row[0], row[1], "at_step", 0)])
            except ValueError as err:
                raise ValueError(f"[CONTROLS] line {i + 1} ({' '.join(sec['CONTROLS'][i])}): {str(err).split(': ', 1)[-1]}") from None
    return InpHydraulics(network, np.asarray(demand), np.asarray(rough), mult, pattern_of_node, np.asarray(pump_speed, dtype=np.float64),
                         names, links, ["1 (constant)"] + list(pats), emitter_coefficient, *pdd, tuple(rows))


# ------------------------------------------------------------------------------------------------------------- blosc
_BLOSC_CODECS = {0: "blosclz", 1: "lz4", 2: "snappy", 3: "zlib", 4: "zstd"}


def _lz4_block(src: bytes, out_len: int) -> bytes:
    lib = _native.load()
    dst = np.empty(out_len, dtype=np.uint8)
    s = np.frombuffer(src, dtype=np.uint8)
    n = lib.gatres_lz4_decompress_host(s.ctypes.data, len(src), dst.ctypes.data, out_len)
    if n != out_len:
        raise ValueError(f"LZ4 block: expected {out_len} bytes, decoder returned {n}")
    return dst.tobytes()


def blosc_decompress(buf: bytes) -> bytes:
    """One Blosc-1 frame (what ``numcodecs.Blosc`` writes per chunk).  Header: version, versionlz, flags, typesize, nbytes,
    blocksize, cbytes (16 bytes, little endian); flags: 0x1 byte shuffle, 0x2 memcpy, 0x4 bit shuffle, 0x10 blocks not
    split, bits 5-7 codec.  Then one int32 start offset per block; a block is ``typesize`` separately compressed streams
    when it was split (each prefixed by its int32 compressed size; a stream stored raw has size == its uncompressed
    length), else one."""
    if len(buf) < 16:
        raise ValueError("Blosc frame shorter than its header")
    _ver, _verlz, flags, typesize = buf[0], buf[1], buf[2], buf[3]
    nbytes, blocksize, cbytes = struct.unpack_from("<III", buf, 4)
    if cbytes > len(buf):
        raise ValueError("Blosc frame truncated")
    if flags & 0x4:
        raise ValueError("Blosc bit-shuffle is not supported (the reference's stores use the default byte shuffle)")
    if flags & 0x2:
        return bytes(buf[16:16 + nbytes])
    codec = _BLOSC_CODECS.get(flags >> 5)
    if codec not in ("lz4", "zlib"):
        raise ValueError(f"Blosc codec {codec!r} is not supported (lz4 / lz4hc / zlib / memcpy are)")
    if nbytes == 0:
        return b""
    nblocks = (nbytes + blocksize - 1) // blocksize
    bstarts = struct.unpack_from(f"<{nblocks}i", buf, 16)
    dont_split = bool(flags & 0x10)
    out = bytearray(nbytes)
    for b in range(nblocks):
        bsize = min(blocksize, nbytes - b * blocksize)
        leftover = bsize != blocksize
        nsplits = typesize if (not dont_split and not leftover and typesize <= 16 and bsize // typesize >= 128) else 1
        neblock = bsize // nsplits
        pos = bstarts[b]
        block = bytearray()
        for _ in range(nsplits):
            (csize,) = struct.unpack_from("<i", buf, pos)
            pos += 4
            chunk = bytes(buf[pos:pos + csize])
            pos += csize
            if csize == neblock:
                block += chunk
            elif codec == "lz4":
                block += _lz4_block(chunk, neblock)
            else:
                block += zlib.decompress(chunk)
        if len(block) != bsize:
            raise ValueError("Blosc block decoded to the wrong length")
        if (flags & 0x1) and typesize > 1:
            n_el = bsize // typesize
            body = np.frombuffer(bytes(block[:n_el * typesize]), dtype=np.uint8).reshape(typesize, n_el).T.reshape(-1)
            block = bytearray(body.tobytes()) + block[n_el * typesize:]
        out[b * blocksize:b * blocksize + bsize] = block
    return bytes(out)


# -------------------------------------------------------------------------------------------------------------- zarr
class ZarrZip:
    """Read-only view of a zarr-v2 group hierarchy inside a zip file (``zarr.ZipStore``)."""

    def __init__(self, path: str):
        self.path = path
        self._zip = zipfile.ZipFile(path, "r")
        self._names = set(self._zip.namelist())
        if ".zgroup" not in self._names and not any(n.endswith(".zarray") for n in self._names):
            raise ValueError(f"{path}: no zarr metadata (.zgroup / .zarray) inside")
        self.attrs = self._json(".zattrs") or {}

    def _json(self, name: str):
        return json.loads(self._zip.read(name).decode("utf-8")) if name in self._names else None

    def close(self) -> None:
        self._zip.close()

    def group_keys(self, prefix: str = "") -> List[str]:
        """Sub-groups directly under ``prefix`` (``root.group_keys()``, DataLoader.py:213)."""
        pre = prefix.strip("/") + "/" if prefix.strip("/") else ""
        keys = set()
        for n in self._names:
            if n.startswith(pre) and n.endswith("/.zgroup"):
                rest = n[len(pre):-len("/.zgroup")]
                if rest and "/" not in rest:
                    keys.add(rest)
        return sorted(keys)

    def array_keys(self, prefix: str = "") -> List[str]:
        pre = prefix.strip("/") + "/" if prefix.strip("/") else ""
        keys = set()
        for n in self._names:
            if n.startswith(pre) and n.endswith("/.zarray"):
                rest = n[len(pre):-len("/.zarray")]
                if rest and "/" not in rest:
                    keys.add(rest)
        return sorted(keys)

    def array(self, key: str) -> np.ndarray:
        """``np.array(root[feature][split])`` for ``key = "feature/split"`` (DataLoader.py:239)."""
        key = key.strip("/")
        meta = self._json(key + "/.zarray")
        if meta is None:
            raise KeyError(f"{self.path}: no array {key!r}")
        if meta.get("zarr_format") != 2:
            raise ValueError("only zarr format 2 is supported")
        if meta.get("order", "C") != "C":
            raise ValueError("only C-order arrays are supported")
        if meta.get("filters"):
            raise ValueError("zarr filters are not supported")
        shape, chunks = tuple(meta["shape"]), tuple(meta["chunks"])
        dtype = np.dtype(meta["dtype"])
        comp = meta.get("compressor")
        sep = meta.get("dimension_separator", ".")
        fill = meta.get("fill_value")
        fillv = {None: 0, "NaN": np.nan, "Infinity": np.inf, "-Infinity": -np.inf}.get(fill, fill) if not isinstance(
            fill, (int, float)) else fill
        out = np.full(shape, fillv, dtype=dtype)
        grid = [max(1, -(-s // c)) for s, c in zip(shape, chunks)]
        for idx in np.ndindex(*grid):
            name = key + "/" + sep.join(str(i) for i in idx) if shape else key + "/0"
            if name not in self._names:
                continue                                  # an unwritten chunk holds the fill value
            raw = self._zip.read(name)
            if comp is None:
                data = raw
            elif comp.get("id") == "blosc":
                data = blosc_decompress(raw)
            elif comp.get("id") == "zlib" or comp.get("id") == "gzip":
                data = zlib.decompress(raw, 15 + 32)
            else:
                raise ValueError(f"zarr compressor {comp.get('id')!r} is not supported")
            chunk = np.frombuffer(data, dtype=dtype).reshape(chunks)
            sel = tuple(slice(i * c, min((i + 1) * c, s)) for i, c, s in zip(idx, chunks, shape))
            out[sel] = chunk[tuple(slice(0, sl.stop - sl.start) for sl in sel)]
        return out


# -------------------------------------------------------------------------------------------------------- checkpoints
def save_checkpoint(path: str, **kwargs) -> str:
    """utils/auxil.py:224-233: ``torch.save(kwargs, path)``.  train.py:433-451 stores ``model_state_dict``,
    ``optimizer_state_dict``, ``epoch``, ``loss``, the metric dicts, ``mean`` / ``std`` / ``min`` / ``max``, the edge statistics
    and ``norm_type``."""
    if not str(path).endswith(".pth"):
        raise ValueError("checkpoint paths end in .pth (utils/auxil.py:216)")
    torch.save(kwargs, path)
    return path


def load_checkpoint(path: str, model: torch.nn.Module, map_location=None):
    """utils/auxil.py:206-221.  The model's loader accepts PyG's ``lin_src`` / ``lin_dst`` pair as well as the single
    ``lin.weight`` of PyG >= 2.5."""
    if not str(path).endswith(".pth"):
        raise ValueError("checkpoint paths end in .pth (utils/auxil.py:216)")
    if model is None:
        raise ValueError("a model to load the weights into is required")
    cp = torch.load(path, map_location=map_location, weights_only=False)
    model.load_state_dict(cp["model_state_dict"])
    return model, cp


def adam_state_dict(trainer, *, exp_avg: Optional[torch.Tensor] = None, exp_avg_sq: Optional[torch.Tensor] = None,
                    step: Optional[int] = None, lr: Optional[float] = None) -> dict:
    """``torch.optim.Adam(model.parameters(), ...).state_dict()`` equivalent of a ``GATResTrainer``'s flat moments: one
    state entry per parameter in ``model.parameters()`` order (train.py:348, :436).  The keyword arguments put other flat
    moments, another step count or another learning rate in place of the trainer's current ones (``GATResTrainer.fit``: the
    best epoch's state kept on the device)."""
    params = trainer.model._param_list
    exp_avg = trainer.exp_avg if exp_avg is None else exp_avg
    exp_avg_sq = trainer.exp_avg_sq if exp_avg_sq is None else exp_avg_sq
    step = int(trainer.step_counter[0].item()) if step is None else int(step)
    state, off = {}, 0
    for i, p in enumerate(params):
        n = p.numel()
        state[i] = {"step": torch.tensor(float(step)),
                    "exp_avg": exp_avg[off:off + n].view(p.shape).clone(),
                    "exp_avg_sq": exp_avg_sq[off:off + n].view(p.shape).clone()}
        off += n
    h = trainer.hparams
    group = {"lr": h["lr"] if lr is None else float(lr), "betas": (h["beta1"], h["beta2"]), "eps": h["eps"], "weight_decay": h["weight_decay"],
             "amsgrad": False, "maximize": False, "foreach": None, "capturable": False, "differentiable": False,
             "fused": None, "params": list(range(len(params)))}
    return {"state": state, "param_groups": [group]}


def load_adam_state_dict(trainer, state_dict: dict) -> None:
    """The reverse: continue a reference run (``optimizer_state_dict`` of a train.py checkpoint) on the native trainer."""
    params = trainer.model._param_list
    st = state_dict["state"]
    if len(st) not in (0, len(params)):
        raise ValueError(f"optimizer state has {len(st)} entries, the model {len(params)} parameters")
    off, step = 0, 0
    with torch.no_grad():
        for i, p in enumerate(params):
            n = p.numel()
            if st:
                e = st[i]
                trainer.exp_avg[off:off + n].copy_(e["exp_avg"].reshape(-1))
                trainer.exp_avg_sq[off:off + n].copy_(e["exp_avg_sq"].reshape(-1))
                step = int(float(e["step"]))
            off += n
        trainer.step_counter[0] = step
    g = state_dict["param_groups"][0]
    trainer.set_hparams(lr=g["lr"], beta1=g["betas"][0], beta2=g["betas"][1], eps=g["eps"], weight_decay=g["weight_decay"])


# --------------------------------------------------------------------------------------------------------- all of it
def _load_wdn_arrays(inp_path: str, zip_path: str, feature: str, split: str, removal: str, num_records: Optional[int]):
    """One file pair's ``(snapshots fp32 [S, N_kept], edge_index, kept node names)`` on the host."""
    inp = parse_inp(inp_path)
    edge_index, kept = inp_edge_index(inp, removal)
    root = ZarrZip(zip_path)
    try:
        if feature not in root.group_keys():
            raise KeyError(f"feature {feature} is unavailable in zarr file {zip_path}")
        arr = root.array(f"{feature}/{split}")
    finally:
        root.close()
    if num_records is not None:
        arr = arr[:num_records]
    order = inp_node_order(inp)
    keep = set(kept)
    cols = [i for i, n in enumerate(order) if n in keep]
    if arr.shape[-1] < len(order):
        raise ValueError(f"the store has {arr.shape[-1]} columns, the network {len(order)} nodes")
    arr = np.take(arr, cols, axis=-1)
    return torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float32)), edge_index, kept


def load_wdn(inp_path: str, zip_path: str, feature: str = "pressure", split: str = "train",
             removal: str = "keep_junction", num_records: Optional[int] = None, device=None, **store_kw):
    """``WDNDataset.collect`` + ``compute_stats`` for one file pair (DataLoader.py:206-258, :120-147): the ``feature`` array
    of ``split``, its columns restricted to the kept nodes (``np.take(array, taken_indices, axis=-1)`` over
    ``wn.node_name_list``), on the device as a ``SnapshotStore`` together with the junction-subgraph ``edge_index``."""
    from .snapshot_store import SnapshotStore
    snaps, edge_index, kept = _load_wdn_arrays(inp_path, zip_path, feature, split, removal, num_records)
    store = SnapshotStore(snaps, edge_index, device=device, **store_kw)
    return store, kept


def load_wdns(input_paths, zip_paths, feature: str = "pressure", split: str = "train", removal: str = "keep_junction",
              num_records=None, mean: Optional[float] = None, std: Optional[float] = None, device=None, **store_kw):
    """The list form of ``load_wdn`` (``WDNDataset`` takes lists of ``.inp`` / ``.zip`` paths, DataLoader.py:61-183; train.py's
    ``--input_paths`` / ``--dataset_paths``): one network per file pair, all on the device as ONE ``MultiSnapshotStore``
    whose statistics are taken over all networks' arrays together -- or are ``mean`` / ``std`` (a validation or test split
    takes the training store's, train.py:67-86).  ``num_records``: an int for every network or one value per network.
    Returns ``(store, kept)``, ``kept`` the kept node names per network."""
    from .multi_snapshot_store import MultiSnapshotStore
    input_paths, zip_paths = list(input_paths), list(zip_paths)
    if not input_paths or len(input_paths) != len(zip_paths):
        raise ValueError(f"{len(input_paths)} input paths for {len(zip_paths)} dataset paths")
    records = list(num_records) if isinstance(num_records, (list, tuple)) else [num_records] * len(input_paths)
    if len(records) != len(input_paths):
        raise ValueError(f"num_records holds {len(records)} values for {len(input_paths)} networks")
    networks, kept = [], []
    for inp_path, zip_path, n in zip(input_paths, zip_paths, records):
        snaps, edge_index, names = _load_wdn_arrays(inp_path, zip_path, feature, split, removal, n)
        networks.append((snaps, edge_index))
        kept.append(names)
    return MultiSnapshotStore(networks, device=device, mean=mean, std=std, **store_kw), kept
