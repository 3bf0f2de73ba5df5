"""Host statements of the estimation kernels (k_estimate.hip), shared by the estimation test modules.

Two kinds.  The torch statements (``torch_stage``, ``torch_stage_available``) restate the reference's collation with torch on
the device; the tests of the passes feed them to the forward, so they stay where the buffers are.  The numpy statements restate
a kernel on the host, away from the device under test: fp32 with separately rounded multiply and add wherever the kernel forms
fp32 values (numpy rounds every fp32 operation once), fp64 sums of exact terms elsewhere.  They are vectorised over the elements;
the only Python loops run over members (``numpy_reduce``), snapshots (``numpy_fold``) and graphs (``numpy_pair_errors``), where
the kernels fix the order of the additions."""
import numpy as np
import torch

DEV = "cuda:0"
U = 2.0 ** -53


# ---- targets ------------------------------------------------------------------------------------------------------------------------
def garbage(n):
    """A staging target that shows any element the launch leaves unwritten: NaN inputs and mask bytes of 0xAB."""
    return (torch.full((n,), float("nan"), dtype=torch.float32, device=DEV),
            torch.full((n,), 0xAB, dtype=torch.uint8, device=DEV))


# ---- staging, with torch on the device ----------------------------------------------------------------------------------------------
def torch_stage(values, n, observed):
    """The reference's collation for a fixed sensor set: zeros, the sensors' values put at their nodes, a mask of ones with
    zeros there.  ``values``: [g, K]."""
    g = values.shape[0]
    obs = torch.tensor(observed, dtype=torch.int64, device=DEV)
    x = torch.zeros((g, n), dtype=torch.float32, device=DEV)
    x.index_put_((torch.arange(g, device=DEV).unsqueeze(1), obs.unsqueeze(0)), values)
    mask = torch.ones((g, n), dtype=torch.uint8, device=DEV)
    mask[:, obs] = 0
    return x.reshape(-1), mask.reshape(-1)


def torch_stage_available(values, n, observed, available):
    """The reference's collation with gaps: zeros, ``index_put_`` of the PRESENT values at their nodes, a mask of ones with
    zeros where present.  ``values``, ``available``: [g, K]."""
    g = values.shape[0]
    obs = torch.tensor(observed, dtype=torch.int64, device=DEV)
    gi, ki = available.bool().nonzero(as_tuple=True)
    x = torch.zeros((g, n), dtype=torch.float32, device=DEV)
    x.index_put_((gi, obs[ki]), values[gi, ki])
    mask = torch.ones((g, n), dtype=torch.uint8, device=DEV)
    mask[gi, obs[ki]] = 0
    return x.reshape(-1), mask.reshape(-1)


# ---- staging, in numpy on the host --------------------------------------------------------------------------------------------------
def numpy_normalise(v, mode, offset, factor):
    """(v - offset) / factor as the staging kernel forms it on fp32 values: the subtraction rounded to fp32, then a division by
    (float)factor (mode 1) or the product with the fp32 reciprocal 1.0f / (float)factor (mode 2); mode 0: ``v`` itself."""
    v = np.asarray(v, dtype=np.float32)
    if mode == 0:
        return v
    c = (v - np.float32(offset)).astype(np.float32)
    f = np.float32(factor)
    return (c / f).astype(np.float32) if mode == 1 else (c * (np.float32(1.0) / f)).astype(np.float32)


def numpy_stage(values, n, observed, present=None):
    """gatres_stage_observed[_available] restated: ``values`` fp32 [g, K] (the staged value of sensor k in graph g), ``present``
    [g, K] (None: everything).  x = 0 and mask = 1 everywhere but at the present sensors, which carry their value and mask = 0.
    The sensors are distinct, so the assignment order does not matter.  Returns (x as int32 bits [g * n], mask uint8 [g * n])."""
    values = np.ascontiguousarray(values, dtype=np.float32)
    g, K = values.shape
    obs = np.asarray(observed, dtype=np.int64)
    assert obs.shape == (K,) and len(set(obs.tolist())) == K
    here = np.ones((g, K), dtype=bool) if present is None else np.asarray(present) != 0
    gi, ki = np.nonzero(here)
    x = np.zeros((g, n), dtype=np.float32)
    mask = np.ones((g, n), dtype=np.uint8)
    x[gi, obs[ki]] = values[gi, ki]
    mask[gi, obs[ki]] = 0
    return x.reshape(-1).view(np.int32), mask.reshape(-1)


# ---- write-back ---------------------------------------------------------------------------------------------------------------------
def numpy_descale(v, scale, offset):
    """D(v) = v * (float)scale + (float)offset in fp32, the product and the sum each rounded."""
    v = np.asarray(v, dtype=np.float32)
    return ((v * np.float32(scale)).astype(np.float32) + np.float32(offset)).astype(np.float32)


def numpy_write_back(out, x, mask, n, scale, offset, keep, dst, first_row):
    """gatres_estimate_write restated: graph g's n values, D(out) -- with ``keep`` D(x) where mask == 0 --, into the columns
    [0, n) of row first_row + g of a copy of ``dst`` [rows, stride]; everything else stays."""
    g = out.size // n
    v = np.where(np.asarray(mask) != 0, out, x) if keep else out
    res = np.array(dst, dtype=np.float32, copy=True)
    res[first_row:first_row + g, :n] = numpy_descale(v, scale, offset).reshape(g, n)
    return res


# ---- ensemble reduce ----------------------------------------------------------------------------------------------------------------
def numpy_reduce(x):
    """Mean and sample standard deviation over axis 1 of fp32 ``x`` [C, M, N] as include/gatres.h states them: fp64 sums in
    member order, written as loops (np.mean / np.std associate pairwise)."""
    x = np.asarray(x, dtype=np.float32)
    C, M, N = x.shape
    acc = np.zeros((C, N), dtype=np.float64)
    for m in range(M):
        acc = acc + x[:, m].astype(np.float64)
    mean64 = acc / np.float64(M)
    sq = np.zeros((C, N), dtype=np.float64)
    for m in range(M):
        d = x[:, m].astype(np.float64) - mean64
        sq = sq + d * d
    sd = np.sqrt(sq / np.float64(M - 1)).astype(np.float32) if M > 1 else np.zeros((C, N), dtype=np.float32)
    return mean64.astype(np.float32), sd


# ---- per-node moments ---------------------------------------------------------------------------------------------------------------
def numpy_node_moments(est, truth, scale, offset, observed, available=None):
    """gatres_node_error_moments[_available] restated, [N, 8] fp64: t = D(truth) and e = est - t in fp32 with separate roundings,
    every sum in fp64 over the snapshots (numpy's order, not the kernel's: ``check_moments`` bounds the difference).  Without
    ``available``: [S, sum e, sum |e|, sum e^2, max |e|, #kept, sum |e| / |t| over the kept, observed flag], kept: |t| > 0.01.
    With ``available`` [S, K]: the same over the HIDDEN entries -- every entry of a node outside ``observed``, the entries of
    sensor k where available[s, k] == 0 --, [0] their number and [7] S minus it."""
    est = np.asarray(est, dtype=np.float32)
    S, N = est.shape
    obs = np.asarray(observed, dtype=np.int64)
    t32 = numpy_descale(truth, scale, offset)
    e32 = (est - t32).astype(np.float32)
    assert t32.dtype == np.float32 and e32.dtype == np.float32
    H = np.ones((S, N), dtype=bool)
    if available is not None:
        H[:, obs] = np.asarray(available) == 0
    e, ae, at = e32.astype(np.float64), np.abs(e32).astype(np.float64), np.abs(t32).astype(np.float64)
    keep = (np.abs(t32) > np.float32(0.01)) & H
    T = np.zeros((N, 8), dtype=np.float64)
    T[:, 1] = np.where(H, e, 0.0).sum(0)
    T[:, 2] = np.where(H, ae, 0.0).sum(0)
    T[:, 3] = np.where(H, e * e, 0.0).sum(0)
    T[:, 4] = np.where(H, ae, 0.0).max(0)
    T[:, 5] = keep.sum(0)
    T[:, 6] = np.where(keep, ae / np.where(keep, at, 1.0), 0.0).sum(0)
    if available is None:
        T[:, 0] = S
        T[obs, 7] = 1.0
    else:
        T[:, 0] = H.sum(0)
        T[:, 7] = S - H.sum(0)
    return T


def numpy_spread_moments(sd):
    """gatres_node_spread_moments restated, [N, 4] fp64: [S, sum (double)sd^2, max sd, sum sd] over the snapshots."""
    sd = np.asarray(sd, dtype=np.float32)
    x = sd.astype(np.float64)
    T = np.empty((sd.shape[1], 4), dtype=np.float64)
    T[:, 0] = sd.shape[0]
    T[:, 1] = (x * x).sum(0)
    T[:, 2] = x.max(0)
    T[:, 3] = x.sum(0)
    return T


def check_sums(got, want, terms, what, against=None):
    """Sums of ``terms`` fp64 terms that both sides form exactly: only the order of the additions can differ, and either order
    is within (terms - 1) * 2^-53 of the exact sum of the absolute terms.  Non-negative terms: that sum is ``want`` itself; a
    signed sum cancels and is bounded against the sum of its absolute terms, ``against``."""
    ref = np.abs(want) if against is None else against
    d = np.abs(got - want)
    print(f"{what}: max difference / reference {float((d / np.maximum(ref, 1e-300)).max()):.3e} (bound {2 * terms * U:.3e})")
    assert (d <= 2 * terms * U * ref).all(), what


def check_moments(got, want, S):
    """A moments table against ``numpy_node_moments``: the counts, the maximum and the flag exact, the sums by ``check_sums``."""
    for f, name in ((0, "count"), (4, "max |e|"), (5, "kept"), (7, "flag")):
        np.testing.assert_array_equal(got[:, f], want[:, f], err_msg=name)
    check_sums(got[:, 2], want[:, 2], S, "sum |e|")
    check_sums(got[:, 3], want[:, 3], S, "sum e^2")
    check_sums(got[:, 6], want[:, 6], S, "sum |e| / |t|")
    check_sums(got[:, 1], want[:, 1], S, "sum e", against=want[:, 2])


# ---- layout errors ------------------------------------------------------------------------------------------------------------------
def numpy_pair_errors(out, mask, truth, scale, offset, score=None):
    """gatres_layout_pair_errors restated: ``out``, ``truth`` fp32 [G, N] (truth: the row of each graph), ``mask`` uint8 [G, N],
    ``score`` uint8 [N] or None.  D() and the difference in fp32 with separate roundings, the sums in fp64."""
    out, truth = np.asarray(out, dtype=np.float32), np.asarray(truth, dtype=np.float32)
    sc, of = np.float32(scale), np.float32(offset)
    e = ((out * sc).astype(np.float32) + of).astype(np.float32) - ((truth * sc).astype(np.float32) + of).astype(np.float32)
    assert e.dtype == np.float32
    counted = np.asarray(mask) != 0
    if score is not None:
        counted = counted & (np.asarray(score) != 0)[None, :]
    rec = np.zeros((out.shape[0], 4), dtype=np.float64)
    for g in range(out.shape[0]):
        eg = e[g][counted[g]].astype(np.float64)
        if eg.size:
            rec[g] = [eg.size, np.abs(eg).sum(), (eg * eg).sum(), np.abs(eg).max()]
    return rec


def check_records(got, want, terms):
    """Count and max exact; the two sums within 2 * terms * 2^-53 relative (non-negative terms that are exact in fp64: only the
    order of the additions can differ, and either order is within (terms - 1) * 2^-53 of the exact sum)."""
    np.testing.assert_array_equal(got[:, 0], want[:, 0])
    np.testing.assert_array_equal(got[:, 3], want[:, 3])
    for f in (1, 2):
        d = np.abs(got[:, f] - want[:, f])
        print(f"field {f}: max relative difference {float((d / np.maximum(want[:, f], 1e-300)).max()):.3e} "
              f"(bound {2 * terms * U:.3e})")
        assert (d <= 2 * terms * U * want[:, f]).all(), f


def numpy_fold(rec, S, L, table=None):
    """gatres_layout_error_reduce restated: per layout in snapshot order."""
    t = np.zeros((L, 4), dtype=np.float64) if table is None else table.copy()
    r = rec.reshape(S, L, 4)
    for s in range(S):
        t[:, :3] = t[:, :3] + r[s, :, :3]
        t[:, 3] = np.maximum(t[:, 3], r[s, :, 3])
    return t
