"""Shared by the screening test modules: the constants of csrc/k_screen.hip read from its text (the ``constants`` / ``grid_cap``
idiom of sensitivity_refs.py), the shapes that lie past them, and ``gatres_loo_residuals`` restated from the launch's raw
buffers.  Everything here runs on the host."""
import numpy as np

import sensitivity_refs as R
from estimation_refs import numpy_descale

FILE = "k_screen.hip"
NAN_BITS = 0x7FC00000

# gatres_loo_residuals: the batches of the bitwise test, and one launch past the grid cap (graphs > cap * LR_T)
LOO_K = [2, 7, 8]
LOO_G = [1, 3, 32, 33]
LOO_CAPPED = dict(N=3, K=2, G=65600)
# gatres_screen_reject: one wave per snapshot, the lanes stride over k; one launch past the grid cap (snapshots > cap * SR_WAVES)
REJECT_S = [1, 3, 300]
REJECT_K = [2, 7, 64, 65, 600]
REJECT_CAPPED = dict(S=4100, K=2)
# the sensors of the end-to-end case on make_wdn_topology(40, 47, seed=0): pairwise more than 3 hops apart
FAR_SENSORS = [0, 10, 12, 14, 22, 33, 37]


def constants():
    return R.constants(FILE)


def grid_cap(entry):
    return R.grid_cap(entry, FILE)


def source():
    return R.source(FILE)


def numpy_loo_residuals(pkg, out, mask, src, full_rows, N, K, first_pair, observed, scale, offset, available, nan_is_missing,
                        pred, resid):
    """``gatres_loo_residuals`` from the launch's buffers: ``out`` fp32 and ``mask`` uint8 ``[G, N]``, ``src`` ``[S, N]`` scaled
    (``full_rows``) or ``[S, K]`` physical, ``available`` ``[S, K]`` or None.  Returns copies of ``pred`` / ``resid`` (``[S, K]``)
    with the batch's G entries from pair ``first_pair`` on replaced."""
    G = out.shape[0]
    obs = np.asarray(observed, dtype=np.int64)
    p = first_pair + np.arange(G)
    s, k = p // K, p % K
    v = obs[k]
    r = numpy_descale(src[s, v], scale, offset) if full_rows else np.asarray(src, dtype=np.float32)[s, k]
    here = np.ones(G, dtype=bool) if available is None else np.asarray(available)[s, k] != 0
    if nan_is_missing:
        here = here & ~np.isnan(r)
    here = here & (mask[np.arange(G), v] != 0)
    res, pr = pkg.loo_residuals_from_estimates(r[None, :], numpy_descale(out[np.arange(G), v], scale, offset)[None, :], here[None, :])
    pred, resid = np.array(pred, dtype=np.float32, copy=True), np.array(resid, dtype=np.float32, copy=True)
    pred.reshape(-1)[p] = pr[0]
    resid.reshape(-1)[p] = res[0]
    return pred, resid


def same_floats(got, want, what=""):
    """Bit for bit, but for the payload of a NaN that an arithmetic operation produced (the two machines may differ there): the
    NaNs sit at the same places, everything else has the same bits."""
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, what
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=what)
    ok = ~np.isnan(want)
    np.testing.assert_array_equal(got.view(np.int32)[ok], want.view(np.int32)[ok], err_msg=what)
