"""fp64 host reference of the moment record ``gatres_masked_metrics`` writes (a test helper, not collected)."""
import numpy as np


def masked_metric_moments(out, y, mask, scale: float = 1.0, offset: float = 0.0) -> np.ndarray:
    """Host fp64 counterpart of one record of ``gatres_masked_metrics`` (include/gatres.h gives the layout): ``out`` / ``y``
    scaled fp32 values, ``mask`` bool; descaled as torch rounds ``scaled * scale + offset`` on fp32 tensors."""
    m = np.asarray(mask, dtype=bool).reshape(-1)
    so = np.asarray(out, dtype=np.float32).reshape(-1)[m]
    st = np.asarray(y, dtype=np.float32).reshape(-1)[m]
    sc, of = np.float32(scale), np.float32(offset)
    p = ((so * sc).astype(np.float32) + of).astype(np.float32)
    t = ((st * sc).astype(np.float32) + of).astype(np.float32)
    pd, td = p.astype(np.float64), t.astype(np.float64)
    r = np.zeros(16, dtype=np.float64)
    M = so.size
    r[0] = M
    r[1] = float(np.sum((so.astype(np.float64) - st.astype(np.float64)) ** 2))
    d = pd - td
    r[2], r[3], r[4], r[5] = np.sum(np.abs(d)), np.sum(d * d), np.sum(pd), np.sum(td)
    with np.errstate(invalid="ignore", divide="ignore"):
        dp, dt = pd - r[4] / M, td - r[5] / M
    r[6], r[7], r[8] = np.sum(dp * dp), np.sum(dt * dt), np.sum(dp * dt)
    keep = np.abs(t) > np.float32(0.01)
    r[9] = keep.sum()
    r[10] = np.sum(np.abs(np.abs(td[keep] - pd[keep]) / td[keep]))
    r[11] = np.sum(np.abs(t - p) <= t * np.float32(0.1))
    return r
