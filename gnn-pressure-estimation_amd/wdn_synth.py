"""Synthetic water-distribution-network (WDN) snapshots with C-Town's shape.

The reference's C-Town inputs are not shipped (inputs/ctown.inp is a Git-LFS pointer and
datasets/ctown.zip is a generated artefact), so benchmarks and tests use a seeded
stand-in with the same sizes: 388 junction nodes, 430 pipes -> 860 directed edges, emitted in the
order ``torch_geometric.utils.from_networkx`` produces for an undirected ``nx.Graph``
(reference: utils/DataLoader.py:28-37, :236 -- grouped by source node, neighbours in insertion order).

Also here: the block-diagonal batch collation the reference gets from
``torch_geometric.loader.DataLoader`` (train.py:302-303) and the reference's host-side mask
sampler (utils/auxil.py:143-182) for callers that want bit-identical host masks.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np
import torch

CTOWN_NODES = 388
CTOWN_PIPES = 430


def make_wdn_topology(num_nodes: int = CTOWN_NODES, num_pipes: int = CTOWN_PIPES, seed: int = 0,
                      max_degree: int = 5, locality: int = 24) -> torch.Tensor:
    """Random near-planar WDN: a spanning tree plus ``num_pipes - (num_nodes-1)`` loop-closing chords.

    Returns ``edge_index`` int64 [2, 2*num_pipes]: both directions of every pipe, grouped by source node
    in ascending order, neighbours in the order the pipes were inserted (``from_networkx`` order).
    """
    assert num_pipes >= num_nodes - 1
    rng = np.random.RandomState(seed)
    adj: List[List[int]] = [[] for _ in range(num_nodes)]
    deg = np.zeros(num_nodes, dtype=np.int64)
    have = set()

    def add(u: int, v: int) -> None:
        adj[u].append(v)
        adj[v].append(u)
        deg[u] += 1
        deg[v] += 1
        have.add((min(u, v), max(u, v)))

    for v in range(1, num_nodes):                      # spanning tree, attach to a nearby earlier node
        lo = max(0, v - locality)
        cand = [u for u in range(lo, v) if deg[u] < max_degree - 1]
        if not cand:
            cand = [u for u in range(0, v) if deg[u] < max_degree]
        add(int(rng.choice(cand)), v)
    chords = num_pipes - (num_nodes - 1)
    tries = 0
    while chords > 0:
        tries += 1
        assert tries < 1000000, "could not place chords under the degree cap"
        u = int(rng.randint(0, num_nodes))
        v = u + int(rng.randint(2, locality + 1)) * (1 if rng.rand() < 0.5 else -1)
        if v < 0 or v >= num_nodes or u == v:
            continue
        if (min(u, v), max(u, v)) in have or deg[u] >= max_degree or deg[v] >= max_degree:
            continue
        add(u, v)
        chords -= 1
    src = [u for u in range(num_nodes) for _ in adj[u]]
    dst = [v for u in range(num_nodes) for v in adj[u]]
    return torch.tensor([src, dst], dtype=torch.int64)


def make_hydraulic_network(num_nodes: int = CTOWN_NODES, num_pipes: int = CTOWN_PIPES, num_reservoirs: int = 1, seed: int = 0,
                           length_range=None, diameter_range=None, elevation_range=None, head_range=None, device=None,
                           num_tanks: int = 0, num_pumps: int = 0, num_check_valves: int = 0, minor_loss_range=None,
                           num_prvs: int = 0, num_psvs: int = 0, valve_seed: int = 0,
                           valve_minor_loss: float = 2.5, num_emitters: int = 0, emitter_exponent: float = 0.5,
                           emitter_seed: int = 0):
    """A ``hydraulics.HydraulicNetwork`` on ``make_wdn_topology(num_nodes, num_pipes, seed)``: ``num_reservoirs`` of the nodes
    are fixed-head nodes, and lengths, diameters, elevations and reservoir heads are seeded uniform numpy draws from the ranges
    of the reference's scenario generator for C-Town (``hydraulics.LENGTH_RANGE`` and so on) unless given.  The last
    ``num_tanks`` of the fixed-head nodes are tanks: a diameter from ``hydraulics.TANK_DIAMETER_RANGE`` and a starting level from
    ``hydraulics.TANK_LEVEL_RANGE`` each, drawn AFTER everything else (``num_tanks=0`` returns what it always did); a tank's
    elevation is set to its head minus that level, so the network's ``fixed_head`` is the tank's starting head (a drawn elevation
    and a drawn head would put the level anywhere).  Level limits: the constructor's default, (0, +inf).

    SPECIAL LINKS (hydraulics.py: THE LINK LAW), drawn after the tanks, so the defaults return what they always did:
    ``num_pumps`` of the links that leave a fixed-head node become pumps that run from that node to the junction, with a shut-off
    head from ``PUMP_SHUTOFF_RANGE`` and a quadratic curve that gives half of it at ``PUMP_DESIGN_VELOCITY`` in the link;
    ``minor_loss_range`` (lo, hi) draws a minor-loss coefficient K for every link but the pumps; ``num_check_valves`` of the
    other links, in a drawn order and a drawn direction each, become check valves -- one that would leave a junction without
    a directed path from a fixed-head node is passed over.  ``ValueError`` where that many cannot be placed.

    REGULATING VALVES (hydraulics.py: THE REGULATING VALVES), drawn after everything else with a generator of their own, so the
    defaults return what they always did: ``num_prvs`` + ``num_psvs`` of the links that are neither pumps nor check valves, in a
    drawn order, become valves (the PRVs first) wherever the constructor accepts them, oriented along the flow of the network
    without valves in one nominal scenario (mid-range demand and roughness, ``solve_ref``); a valve's setting is the pressure
    of its controlled node in that scenario; ``valve_seed`` picks another layout of the valves on the same network.  A valve
    gets the minor-loss coefficient ``valve_minor_loss``: with K = 0 an OPEN valve sits on the linear floor of the law, where
    its flow jitters by 1e-7 m3/s per ulp of the heads and the stop rule is met by chance (hydraulics.py: WHAT DOES NOT HOLD).
    ``ValueError`` where that many cannot be placed.

    EMITTERS (hydraulics.py: THE EMITTERS), drawn after everything else with a generator of their own, so the defaults return what
    they always did: ``num_emitters`` junctions, in a drawn order, never a fixed-head node nor the controlled node of a
    regulating valve, get an emitter with the exponent ``emitter_exponent``; ``emitter_seed`` picks other junctions.  The
    coefficients are a scenario's (``simulate(emitter_coefficient=)``), not the network's."""
    from . import hydraulics as H
    if not 1 <= num_reservoirs < num_nodes:
        raise ValueError("num_reservoirs must lie in [1, num_nodes)")
    if not 0 <= num_tanks <= num_reservoirs:
        raise ValueError("num_tanks must lie in [0, num_reservoirs]: the tanks are the last of the fixed-head nodes")
    ei = make_wdn_topology(num_nodes, num_pipes, seed=seed)
    rng = np.random.RandomState(seed + 7919)
    fixed_nodes = np.sort(rng.choice(num_nodes, num_reservoirs, replace=False))
    draw = lambda rg, n: rng.uniform(rg[0], rg[1], n)
    length = draw(length_range or H.LENGTH_RANGE, num_pipes)
    diameter = draw(diameter_range or H.DIAMETER_RANGE, num_pipes)
    elevation = draw(elevation_range or H.ELEVATION_RANGE, num_nodes)
    head = draw(head_range or H.HEAD_RANGE, num_reservoirs)
    kw = {}
    if num_tanks:
        tanks = fixed_nodes[num_reservoirs - num_tanks:]
        tank_diameter = draw(H.TANK_DIAMETER_RANGE, num_tanks)
        level = draw(H.TANK_LEVEL_RANGE, num_tanks)
        elevation[tanks] = head[num_reservoirs - num_tanks:] - level
        kw.update(tank_nodes=tanks, tank_diameter=tank_diameter)
    if num_pumps < 0 or num_check_valves < 0:
        raise ValueError("num_pumps and num_check_valves must not be negative")
    if not (num_pumps or num_check_valves or minor_loss_range is not None):
        return _with_valves(H, num_prvs, num_psvs, seed, valve_seed, valve_minor_loss, (ei, length, diameter, elevation, fixed_nodes, head), dict(device=device, **kw),
                            (num_emitters, emitter_exponent, emitter_seed))
    # the special links, drawn after everything else
    e = ei.numpy()
    pipes = e[:, e[0] < e[1]].T
    fixed = np.zeros(num_nodes, dtype=bool)
    fixed[fixed_nodes] = True
    a, b = pipes[:, 0], pipes[:, 1]
    at_source = np.flatnonzero(fixed[a] ^ fixed[b])
    if num_pumps > at_source.size:
        raise ValueError(f"num_pumps = {num_pumps}, but only {at_source.size} links leave a fixed-head node")
    pumps = rng.permutation(at_source)[:num_pumps]
    flip = np.zeros(num_pipes, dtype=bool)
    flip[pumps] = fixed[b[pumps]]                                   # a pump runs from the fixed-head node to the junction
    h0 = draw(PUMP_SHUTOFF_RANGE, num_pumps)
    q_design = PUMP_DESIGN_VELOCITY * np.pi * diameter[pumps] ** 2 / 4.0
    kw.update(pump_links=pumps, pump_h0=h0, pump_r=0.5 * h0 / q_design ** 2, pump_n=np.full(num_pumps, 2.0))
    minor = np.zeros(num_pipes)
    if minor_loss_range is not None:
        minor = draw(minor_loss_range, num_pipes)
        minor[pumps] = 0.0
    check = np.zeros(num_pipes, dtype=bool)
    is_pump = np.zeros(num_pipes, dtype=bool)
    is_pump[pumps] = True
    placed = 0
    for p, way in zip(rng.permutation(num_pipes), rng.randint(0, 2, num_pipes).astype(bool)):
        if placed == num_check_valves:
            break
        if is_pump[p]:
            continue
        check[p], flip[p] = True, way
        if _all_fed(num_nodes, pipes, flip, check | is_pump, fixed):
            placed += 1
        else:                                                       # (it would cut a zone off from every source: not this one)
            check[p], flip[p] = False, False
    if placed < num_check_valves:
        raise ValueError(f"only {placed} of {num_check_valves} check valves can be placed without cutting a zone off")
    return _with_valves(H, num_prvs, num_psvs, seed, valve_seed, valve_minor_loss, (ei, length, diameter, elevation, fixed_nodes, head),
                        dict(device=device, minor_loss=minor, check_valve=check, link_reversed=flip, **kw),
                        (num_emitters, emitter_exponent, emitter_seed))


def _with_emitters(net, rebuild, seed: int, emitters):
    """``net`` with its emitters placed (none: ``net`` itself); ``rebuild(emitter_nodes=, emitter_exponent=)`` builds it again."""
    num_emitters, exponent, emitter_seed = emitters
    if num_emitters < 0:
        raise ValueError("num_emitters must not be negative")
    if num_emitters == 0:
        return net
    free = ~net.fixed
    free[net.valve_node] = False
    nodes = np.flatnonzero(free)
    if num_emitters > nodes.size:
        raise ValueError(f"num_emitters = {num_emitters}, but only {nodes.size} junctions can take an emitter")
    rng = np.random.RandomState(seed + 32452843 + emitter_seed)
    return rebuild(emitter_nodes=rng.permutation(nodes)[:num_emitters], emitter_exponent=exponent)


def _with_valves(H, num_prvs: int, num_psvs: int, seed: int, valve_seed: int, valve_minor_loss: float, args, kw, emitters=(0, 0.5, 0)):
    """The network of ``make_hydraulic_network`` with its regulating valves placed (none: the constructor's call as it was), and
    then its emitters."""
    if num_prvs < 0 or num_psvs < 0:
        raise ValueError("num_prvs and num_psvs must not be negative")
    net = H.HydraulicNetwork(*args, **kw)
    want = ["PRV"] * num_prvs + ["PSV"] * num_psvs
    if not want:
        return _with_emitters(net, lambda **e: H.HydraulicNetwork(*args, **dict(kw, **e)), seed, emitters)
    demand = np.where(net.fixed, 0.0, 0.5 * (H.DEMAND_RANGE[0] + H.DEMAND_RANGE[1]))[None, :]
    roughness = np.full((1, net.num_pipes), 0.5 * (H.ROUGHNESS_RANGE[0] + H.ROUGHNESS_RANGE[1]))
    nominal = H.solve_ref(net, demand, roughness, solver="banded")
    if nominal.failed[0]:
        raise ValueError("the nominal scenario of the network without valves fails: no flow to orient the valves along")
    flow, pressure = nominal.flow[0], nominal.head[0] - net.elevation
    rng = np.random.RandomState(seed + 15485863 + valve_seed)
    flip = net.pipes[:, 0] > net.pipes[:, 1]                        # the orientation the network has
    links, kinds, settings = [], [], []
    minor = net.minor_loss.copy()

    def build(flip, links, kinds, settings, **e):
        k = minor.copy()
        k[links] = valve_minor_loss
        return H.HydraulicNetwork(*args, **dict(kw, link_reversed=flip, minor_loss=k, valve_links=links, valve_kind=kinds,
                                                valve_setting=settings, **e))
    for p in rng.permutation(net.num_pipes):
        if len(links) == len(want):
            break
        if net.is_pump[p] or net.check_valve[p] or net.closed[p]:
            continue
        kind = want[len(links)]
        trial = flip.copy()
        trial[p] = flip[p] ^ (flow[p] < 0)                          # along the flow
        a, b = (net.pipes[p, 1], net.pipes[p, 0]) if flow[p] < 0 else (net.pipes[p, 0], net.pipes[p, 1])
        c = b if kind == "PRV" else a
        try:
            build(trial, links + [int(p)], kinds + [kind], settings + [float(pressure[c])])
        except ValueError:
            continue
        flip = trial
        links, kinds, settings = links + [int(p)], kinds + [kind], settings + [float(pressure[c])]
    if len(links) < len(want):
        raise ValueError(f"only {len(links)} of {len(want)} regulating valves can be placed")
    return _with_emitters(build(flip, links, kinds, settings), lambda **e: build(flip, links, kinds, settings, **e), seed, emitters)


PUMP_SHUTOFF_RANGE = (20.0, 40.0)       # metres: the shut-off heads make_hydraulic_network draws
PUMP_DESIGN_VELOCITY = 1.0              # m/s in the pump's link at the design flow, where the gain is half the shut-off head


def _all_fed(num_nodes: int, pipes: np.ndarray, flip: np.ndarray, one_way: np.ndarray, fixed: np.ndarray) -> bool:
    """Does a directed path reach every junction from a fixed-head node, one-way links walked from a to b only?  (What the
    constructor of ``HydraulicNetwork`` refuses otherwise.)"""
    adj = [[] for _ in range(num_nodes)]
    for (lo, hi), f, ow in zip(pipes, flip, one_way):
        u, v = (hi, lo) if f else (lo, hi)
        adj[u].append(int(v))
        if not ow:
            adj[v].append(int(u))
    seen = fixed.copy()
    stack = [int(v) for v in np.flatnonzero(fixed)]
    while stack:
        u = stack.pop()
        for v in adj[u]:
            if not seen[v]:
                seen[v] = True
                stack.append(v)
    return bool(seen.all())


def make_demand_patterns(num_patterns: int, steps: int, step_seconds: float, seed: int) -> np.ndarray:
    """Demand multipliers fp64 [num_patterns, steps]: seeded, smooth (a constant plus the first three harmonics of a day),
    strictly positive, with a period of 24 h in time and a mean of 1 over the ``steps`` given.  Host numpy."""
    if num_patterns < 1 or steps < 1 or not step_seconds > 0:
        raise ValueError("num_patterns, steps and step_seconds must be positive")
    rng = np.random.RandomState(seed + 104729)
    day = 2.0 * np.pi * (np.arange(steps, dtype=np.float64) * float(step_seconds)) / 86400.0
    amplitude = rng.uniform(0.0, 1.0, (num_patterns, 3)) * np.array([0.35, 0.2, 0.1])       # (their sum stays below 0.65 < 1)
    phase = rng.uniform(0.0, 2.0 * np.pi, (num_patterns, 3))
    wave = sum(amplitude[:, k, None] * np.cos((k + 1) * day[None, :] + phase[:, k, None]) for k in range(3))
    mult = 1.0 + wave
    return mult / mult.mean(axis=1, keepdims=True)


def collate_edge_index(edge_index: torch.Tensor, num_nodes: int, batch_size: int) -> torch.Tensor:
    """Block-diagonal batch of ``batch_size`` copies of one topology (PyG ``Batch`` edge_index:
    per-graph edge lists concatenated, node ids offset by ``k * num_nodes``)."""
    E = edge_index.shape[1]
    off = (torch.arange(batch_size, dtype=torch.int64) * num_nodes).repeat_interleave(E)
    return edge_index.repeat(1, batch_size) + off.unsqueeze(0)


def make_snapshots(num_snapshots: int, num_nodes: int = CTOWN_NODES, seed: int = 1) -> torch.Tensor:
    """z-normalised pressures: fp32 [S, num_nodes] ~ N(0, 1) (reference stores ``[S, N_nodes]`` per split,
    utils/DataLoader.py:212-242, then z-norms with scalar mean/std, :142-147)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn((num_snapshots, num_nodes), generator=g, dtype=torch.float32)


def collate_snapshots(snapshots: torch.Tensor, rows: Sequence[int]) -> torch.Tensor:
    """x = y = [B*N_g, 1] for the chosen snapshot rows (nx_to_pyg, utils/auxil.py:84-98)."""
    return snapshots[list(rows)].reshape(-1, 1).contiguous()


def mask_nodes(num_nodes: int, masking_rate: float, rng: np.random.RandomState,
               required_idx: Sequence[int] = ()) -> np.ndarray:
    """Reference host sampler, utils/auxil.py:143-163: exactly ``int(num_nodes * rate)`` nodes are masked -- the
    ``required_idx`` ones (the sensor nodes of evaluation.py's second pass) always, the rest chosen without replacement
    among the others."""
    required = sorted(set(int(i) for i in required_idx))
    mask_length = int(num_nodes * masking_rate) - len(required)
    if mask_length <= 0:
        raise ValueError("mask length must be positive")
    if required:
        selected = np.setdiff1d(np.arange(num_nodes), np.asarray(required))
        idx = rng.choice(selected, mask_length, replace=False)
    else:
        idx = rng.choice(num_nodes, mask_length, replace=False)
    mask = np.zeros(num_nodes, dtype=bool)
    mask[idx] = True
    mask[required] = True
    return mask


def generate_batch_mask(num_nodes_per_graph: Sequence[int], mask_rate: float, rng: np.random.RandomState,
                        required_idx: Sequence[int] = ()) -> np.ndarray:
    """utils/auxil.py:166-182 (``required_idx`` are node indices INSIDE a graph, the same for every graph of the batch)."""
    return np.hstack([mask_nodes(int(n), mask_rate, rng, required_idx) for n in num_nodes_per_graph])


def make_batch(batch_size: int, num_nodes: int = CTOWN_NODES, num_pipes: int = CTOWN_PIPES,
               topo_seed: int = 0, data_seed: int = 1, mask_seed: int = 2,
               mask_rate: float = 0.95) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """One training batch: (x, y, edge_index, mask) on CPU; x == y before masking (train.py:162-174)."""
    ei = make_wdn_topology(num_nodes, num_pipes, seed=topo_seed)
    edge_index = collate_edge_index(ei, num_nodes, batch_size)
    snaps = make_snapshots(batch_size, num_nodes, seed=data_seed)
    y = collate_snapshots(snaps, range(batch_size))
    mask = torch.from_numpy(generate_batch_mask([num_nodes] * batch_size, mask_rate,
                                                np.random.RandomState(mask_seed)))
    return y.clone(), y, edge_index, mask
