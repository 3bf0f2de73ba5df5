"""Fine-tuning to a FIXED sensor layout: the host side of ``gatres_stage_rows_mask_sensors`` and of its noisy sibling
``gatres_stage_rows_mask_sensors_noisy`` (csrc/k_stage.hip).

``sensor_layout_draws`` restates the launch's draws in numpy ``uint64`` arithmetic (no device use): which graphs of a batch take
the layout mask and which sensors keep their reading; ``sensor_layout_noise`` names the standard normal draw of each (graph,
sensor) of the noisy launch.  ``SensorLayout`` is what ``GATResTrainer.set_sensor_layout`` holds: the checked indices, their
device copy (uploaded once), the two probabilities and, under measurement noise, the device ``sigma[K]`` (uploaded once) and
the noise seed."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

_GOLDEN, _NODE, _GRAPH = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB


def _mix64(z: np.ndarray) -> np.ndarray:
    """``mix64`` of csrc/gatres_common.h on uint64 arrays (numpy's unsigned array arithmetic is modulo 2^64)."""
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _base(seed: int, step: int) -> np.ndarray:
    with np.errstate(over="ignore"):
        return np.asarray([int(seed) & 0xFFFFFFFFFFFFFFFF], dtype=np.uint64) + np.uint64(_GOLDEN) * np.asarray(
            [(int(step) + 1) & 0xFFFFFFFFFFFFFFFF], dtype=np.uint64)


def mode_hashes(seed: int, step: int, graphs) -> np.ndarray:
    """The 24-bit hash that decides the mode of graph ``g`` (layout mask iff it is below ``threshold(layout_share)``)."""
    g = np.asarray(graphs, dtype=np.uint64).reshape(-1)
    with np.errstate(over="ignore"):
        return (_mix64(_base(seed, step) + np.uint64(_GRAPH) * (g + np.uint64(1))) >> np.uint64(40)).astype(np.int64)


def node_hashes(seed: int, step: int, positions) -> np.ndarray:
    """The 24-bit hash of the node at batch position ``node_ptr[g] + v`` (a sensor keeps its reading iff it is at least
    ``threshold(sensor_dropout)``): the upper bits of the device sampler's key of that node."""
    p = np.asarray(positions, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return (_mix64(_base(seed, step) + np.uint64(_NODE) * (p + np.uint64(1))) >> np.uint64(40)).astype(np.int64)


def threshold(probability: float) -> int:
    """``(uint32_t)(probability * 16777216.0)``: the launch's 24-bit threshold of a probability."""
    return int(float(probability) * 16777216.0)


def check_probabilities(sensor_dropout: float, layout_share: float) -> Tuple[float, float]:
    d, s = float(sensor_dropout), float(layout_share)
    if not 0.0 <= d < 1.0:
        raise ValueError(f"sensor_dropout must lie in [0, 1) (got {sensor_dropout})")
    if not 0.0 <= s <= 1.0:
        raise ValueError(f"layout_share must lie in [0, 1] (got {layout_share})")
    return d, s


def sensor_layout_draws(seed: int, step: int, num_graphs: int, nodes_per_graph: int, observed_idx: Sequence[int],
                        sensor_dropout: float, layout_share: float) -> Tuple[np.ndarray, np.ndarray]:
    """The draws of ``gatres_stage_rows_mask_sensors`` for a batch of ``num_graphs`` graphs of ``nodes_per_graph`` nodes at
    sampler step ``step``: ``(layout_mode bool [G], keep bool [G, K])``.  ``layout_mode[g]``: graph g takes the layout mask (else
    the sampler's random one); ``keep[g, k]``: sensor ``observed_idx[k]`` of graph g keeps its reading (it is dropped otherwise;
    the value matters in layout mode only).  ``seed`` is the trainer's effective seed, ``step`` the optimizer's step count."""
    d, s = check_probabilities(sensor_dropout, layout_share)
    G, N = int(num_graphs), int(nodes_per_graph)
    obs = np.asarray([int(i) for i in observed_idx], dtype=np.int64)
    if G < 1 or N < 1 or obs.size < 1 or obs.min() < 0 or obs.max() >= N:
        raise ValueError("sensor_layout_draws needs num_graphs, nodes_per_graph >= 1 and observed_idx inside a graph")
    mode = mode_hashes(seed, step, np.arange(G)) < threshold(s)
    pos = np.arange(G, dtype=np.int64).reshape(G, 1) * N + obs.reshape(1, -1)
    keep = node_hashes(seed, step, pos) >= threshold(d)
    return mode, keep


def sensor_layout_noise(noise_seed: int, step: int, rows, num_sensors: int) -> np.ndarray:
    """The standard normal draws of ``gatres_stage_rows_mask_sensors_noisy`` for a batch whose graphs are the source rows
    ``rows`` at sampler step ``step``: float64 ``[G, K]``, entry ``[g, k]`` the ``z`` that sensor ``k`` of graph ``g`` gets if it
    keeps its reading in a layout-mode graph.  The generator is ``gatres_stage_observed_noisy``'s with the step as the member:
    ``reading_noise(noise_seed, 1, S, K, member0=step)[rows[g], 0, k]`` -- the graph's place in the batch does not enter."""
    from .estimation import reading_noise
    r = np.asarray([int(i) for i in rows], dtype=np.int64).reshape(-1)
    if r.size < 1 or r.min() < 0:
        raise ValueError("sensor_layout_noise needs at least one row, none of them negative")
    return reading_noise(noise_seed, 1, int(r.max()) + 1, num_sensors, member0=int(step))[r, 0, :]


class SensorLayout:
    """A trainer's sensor layout: ``observed_idx`` (checked), its int32 device copy, ``sensor_dropout`` and ``layout_share``.
    One object serves a trainer and its siblings.

    ``noise_std`` (``None``: no noise; one non-negative finite number or K of them, physical units): the measurement noise the
    kept readings are staged under.  ``norm = (norm_type, std, eps)`` of the store converts it to the device ``sigma[K]`` in
    store units (``estimation.noise_sigma``, the statement ``PressureEstimator`` uses for full rows), uploaded once, here.  A
    ``noise_std`` of zeros is no noise: ``sigma`` stays None and every launch is the noise-free one."""

    def __init__(self, observed_idx: Sequence[int], nodes_per_graph: int, sensor_dropout: float, layout_share: float, device,
                 noise_std=None, noise_seed: Optional[int] = None, norm: Optional[Tuple[str, Optional[float], float]] = None):
        import torch
        from .estimation import _check_observed, _check_seed, noise_sigma, noise_std_vector
        self.sensor_dropout, self.layout_share = check_probabilities(sensor_dropout, layout_share)
        self.observed_idx: List[int] = _check_observed(observed_idx, int(nodes_per_graph))
        self.nodes_per_graph = int(nodes_per_graph)
        self.noise_std: Optional[List[float]] = None
        self.noise_seed: Optional[int] = None
        self.sigma = None
        if noise_std is not None:
            std = noise_std_vector(noise_std, len(self.observed_idx))
            seed = _check_seed(noise_seed)
            if std.any():
                if norm is None:
                    raise ValueError("noise_std is in physical units and the store's normalisation is unknown to this trainer: "
                                     "build it with GATResTrainer.for_store(model, store, ...), or set trainer.store_norm = "
                                     "(norm_type, std, eps) -- ('unused', None, 0.0) for a store that is not normalised")
                self.noise_std, self.noise_seed = [float(v) for v in std], seed
                self.sigma = torch.from_numpy(noise_sigma(std, len(self.observed_idx), norm[0], norm[1], norm[2],
                                                          full_rows=True)).to(device)
        self.observed = torch.tensor(self.observed_idx, dtype=torch.int32).to(device)

    def key(self) -> tuple:
        """What a captured launch sequence that stages under this layout depends on."""
        key = ("layout", self.observed.data_ptr(), len(self.observed_idx), self.sensor_dropout, self.layout_share)
        return key if self.sigma is None else key + (self.sigma.data_ptr(), self.noise_seed)

    def describe(self) -> dict:
        d = {"observed_idx": list(self.observed_idx), "sensor_dropout": self.sensor_dropout, "layout_share": self.layout_share}
        if self.sigma is not None:
            d["noise_std"], d["noise_seed"] = list(self.noise_std), self.noise_seed
        return d


def refuse_layout_data_parallel(world: int) -> None:
    """A sensor layout trains on one device: the ranks' draws and the layout validation are not sharded."""
    if world > 1:
        raise NotImplementedError(f"fine-tuning to a sensor layout under data parallelism (world size {world}) is not "
                                  f"implemented: set the layout on a single-device trainer")


def refuse_layout_multi_store(store) -> None:
    """Sensor sets belong to one network: a ``MultiSnapshotStore`` has no single layout."""
    from .multi_snapshot_store import MultiSnapshotStore
    if isinstance(store, MultiSnapshotStore):
        raise NotImplementedError("a sensor layout with a MultiSnapshotStore is not implemented (a layout per network would be "
                                  "needed): fine-tune on one network's SnapshotStore")


def stage_rows(lib, data, rows_ptr: int, nodes_per_graph: int, x, y: Optional[object], node_ptr, num_graphs: int,
               layout_observed, num_observed: int, sensor_dropout: float, layout_share: float, mask_rate: float, seed: int,
               step_ptr: Optional[int], mask, stream, sigma=None, noise_seed: int = 0) -> None:
    """Enqueue ``gatres_stage_rows_mask_sensors`` -- with ``sigma`` (device fp32 ``[K]``, store units)
    ``gatres_stage_rows_mask_sensors_noisy`` -- (tensors in, addresses out)."""
    from . import _native
    if sigma is not None:
        _native.check(lib.gatres_stage_rows_mask_sensors_noisy(
            data.data_ptr(), rows_ptr, int(nodes_per_graph), x.data_ptr(), None if y is None else y.data_ptr(),
            node_ptr.data_ptr(), int(num_graphs), layout_observed.data_ptr(), int(num_observed), float(sensor_dropout),
            float(layout_share), float(mask_rate), int(seed) & 0xFFFFFFFFFFFFFFFF, step_ptr, mask.data_ptr(), sigma.data_ptr(),
            int(noise_seed) & 0xFFFFFFFFFFFFFFFF, stream), "gatres_stage_rows_mask_sensors_noisy")
        return
    _native.check(lib.gatres_stage_rows_mask_sensors(
        data.data_ptr(), rows_ptr, int(nodes_per_graph), x.data_ptr(), None if y is None else y.data_ptr(), node_ptr.data_ptr(),
        int(num_graphs), layout_observed.data_ptr(), int(num_observed), float(sensor_dropout), float(layout_share),
        float(mask_rate), int(seed) & 0xFFFFFFFFFFFFFFFF, step_ptr, mask.data_ptr(), stream), "gatres_stage_rows_mask_sensors")
