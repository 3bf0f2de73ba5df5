"""Shared by the monitoring test modules: the constants of csrc/k_monitor.hip read from its text (the ``constants`` / ``grid_cap``
idiom of screening_refs.py), the shapes that lie past them, the inputs of the scan's bitwise cases and the slice-wise evaluation
of the CUSUM that the kernel's decomposition rests on.  Everything here runs on the host."""
import numpy as np

import sensitivity_refs as R
from screening_refs import FAR_SENSORS, same_floats      # noqa: F401

FILE = "k_monitor.hip"


def constants():
    return R.constants(FILE)


def grid_cap(entry):
    return R.grid_cap(entry, FILE)


def source():
    return R.source(FILE)


def scan_lengths(W):
    """The series lengths of the bitwise test for a workgroup of W threads: slices of length 0, 1 and 2, ragged slices, and
    one long series (slices of 274 rows)."""
    return [1, 2, W - 1, W, W + 1, 3 * W + 5, 70001]


SCAN_K = [1, 2, 7]
SCAN_E = [1, 3]
SCAN_LONG = 70001
SCAN_CAPPED = dict(E=1100, K=1, T=2)           # pairs > the grid cap of gatres_cusum_scan
LATCH_CAPPED = dict(E=1030, K=3, T=2)          # series > the grid cap of gatres_monitor_latch


def slice_bounds(T, W):
    """The kernel's slices: thread i owns rows [min(i * per, T), min(i * per + per, T)) with per = ceil(T / W)."""
    per = (T + W - 1) // W
    return [(min(i * per, T), min(i * per + per, T)) for i in range(W)]


def scan_inputs(E, T, K, seed, gaps, specials):
    """Residuals as small multiples of 2^-4 plus a little noise (with sigma = 1 and kappa = 0.5 the statistics return to zero
    again and again), ``mu``, ``inv_sigma`` and an availability.  ``specials`` plants NaN residuals, a residual of 1e30 and one of
    +inf, a column that is never counted (K >= 2), ``inv_sigma = +inf`` and a NaN ``mu`` on one sensor each (K >= 7)."""
    rng = np.random.default_rng(seed)
    S = E * T
    resid = (rng.integers(-12, 13, size=(S, K)) / 16.0).astype(np.float32)
    noisy = rng.random((S, K)) < 0.3
    resid[noisy] += (rng.standard_normal(int(noisy.sum())) * 1e-3).astype(np.float32)
    mu = (rng.integers(-2, 3, size=K) / 16.0).astype(np.float32)
    inv_sigma = rng.choice(np.float32([1.0, 2.0, 0.5]), size=K).astype(np.float32)
    inv_sigma[0] = 1.0
    if specials and S >= 8:
        holes = rng.random((S, K)) < 0.03
        resid[holes] = np.nan
        resid[rng.integers(0, S), 0] = 1e30
        resid[rng.integers(0, S), K - 1] = np.inf
        resid[rng.integers(0, S), 0] = -np.inf
        if K >= 2:
            resid[:, 1] = np.nan                                   # a column that is never counted
        if K >= 7:
            inv_sigma[4] = np.inf                                  # z = +-inf, or NaN where resid == mu
            resid[::5, 4] = mu[4]
            mu[5] = np.nan
            inv_sigma[6] = 0.0                                     # z = 0, or NaN at an infinite residual
            resid[S // 2, 6] = np.inf
    available = None
    if gaps:
        available = (rng.random((S, K)) < 0.85).astype(np.uint8)
        available[:, 0] |= (np.arange(S) % 3 != 0).astype(np.uint8)
    return resid, mu, inv_sigma, available


def slicewise_cusum(pkg, a, g0, cuts):
    """One side of the CUSUM, ``g = max(0, g + a[t])`` from ``g0``, evaluated the way the kernel does: every slice of ``cuts``
    (a list of (lo, hi)) composes its steps to one map, an exclusive scan of the maps gives the slice its carry-in, the slice is
    then walked with the true values.  Returns the path."""
    ops = []
    for lo, hi in cuts:
        op = pkg.monitoring.CUSUM_IDENTITY
        for t in range(lo, hi):
            op = pkg.cusum_compose(op, (int(a[t]), 0))
        ops.append(op)
    path, before = [0] * len(a), pkg.monitoring.CUSUM_IDENTITY
    for (lo, hi), op in zip(cuts, ops):
        g = max(before[1], int(g0) + before[0])
        for t in range(lo, hi):
            g = max(0, g + int(a[t]))
            path[t] = g
        before = pkg.cusum_compose(before, op)
    return path
