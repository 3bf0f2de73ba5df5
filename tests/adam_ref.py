"""The Adam update the four update kernels each write out (adam_kernel, k_misc.hip; autoclip_adam_kernel, k_autoclip.hip;
reduce_adam_kernel and param_grads_finish_kernel, k_fused_host.hip), stated once on the host: in float64 with a bound per
element on what fp32 rounding may do to it (``adam_step_fp64``), and operation by operation in numpy float32
(``adam_step_fp32``: the kernel lines, used on the host only).  Also here: the constructed input vector and the
hyper-parameter grid that the host tests (test_adam_ref_host.py) and the device tests (test_gpu_adam_elementwise.py) share.

The statement is ``torch.optim.Adam``'s single-tensor form with L2 weight decay, which the reference's train.py uses:

    gv = g * scale * coef + wd * p            (scale, coef: fp32 values -- the kernels multiply by a ``float``)
    m' = m + (1 - b1) (gv - m)
    v' = b2 v + (1 - b2) gv^2
    D  = -(lr / (1 - b1^t)) m' / (sqrt(v') / sqrt(1 - b2^t) + eps)
    p' = p + D

numpy only: nothing here needs a device."""
import math

import numpy as np

U = 2.0 ** -24                 # unit round-off of fp32
TINY = 2.0 ** -126             # the smallest normal fp32: covers a result below the normal range, flushed or not
# K is the ceiling the bounds were specified with (16), not a count that happens to reach it.  Counted along the longest chain
# of the kernel lines (k_misc.hip, adam_kernel's loop body), one rounding per operation or (float) conversion:
#   gv : g*scale [1], *coef [2], + (float)wd*pv [3]   (beside the chain: (float)wd, the product wd*pv)              -> 3
#   m' : gv [3], gv-mv [4], * (float)(1-b1) [5], mv + ... [6]                                                      -> 6
#   v' : gv [3], (float)(1-b2)*gv [4], *gv [5], + (float)b2*v [6]                                                  -> 6
#   D  : sqrtf [1], /s_bc2_sqrt [2], + (float)eps [3], the division [4], pv + ... belongs to E_p                   -> 4
# A first-order tally of EVERY rounding that reaches a result -- side operands included, gv's error counted twice in gv*gv --
# gives 9 for m', 16 for v' and 8 for D: K = 16 holds all three, with room to spare for m' and D.  Every rounding is
# relative to a partial result no larger than the sum of magnitudes the bound multiplies.
K = 16

# (lr, beta1, beta2, eps, weight_decay, grad_scale)
CONFIGS = [
    (5e-4, 0.9, 0.999, 1e-8, 6e-6, 1.0),
    (1e-2, 0.0, 0.9, 1e-3, 1e-2, 1.0 / 64),
    (3e-5, 0.5, 0.99, 1e-15, 0.0, 3.0),
    (1e-3, 0.9, 0.9999999, 1e-8, 0.3, 0.7),
]
STEPS = [1, 2, 10, 1000, 10 ** 5, 10 ** 7, 2 ** 33 + 1]         # t: reached by writing t - 1 into step_counter[0]
UPDATE_THREADS = 256
ADAM_MAX_BLOCKS = 512                  # k_misc.hip
AC_UPDATE_MAX_BLOCKS = 512             # k_autoclip.hip
N_GRID = 4096                          # the grid x t runs on this many elements
# one element, one short of a workgroup, a workgroup, one more, and 77 past what the capped grid covers in one trip
SIZES = [1, 255, 256, 257, ADAM_MAX_BLOCKS * UPDATE_THREADS + 77]
SIZE_CONFIG, SIZE_T = 3, 10            # the configuration and t that the sizes run at (every term is live in CONFIGS[3])
GUARD = 64                             # floats behind each array that a launch must leave alone

# Elements that are checked by CLASS (zero, finite, +inf, -inf, NaN) against adam_step_fp32 instead of by bound:
# name -> (g, p, m, v).  The subnormal gradients meet a state of ordinary size, so their results are normal numbers whether
# or not the device flushes subnormals.
SPECIALS = [
    ("g_square_overflows", (1e30, 0.5, 1e-3, 1e-6)),
    ("g_square_overflows_negative", (-1e30, 0.5, 1e-3, 1e-6)),
    ("g_square_overflows_zero_state", (1e30, 0.0, 0.0, 0.0)),
    ("g_plus_inf", (float("inf"), 0.5, 1e-3, 1e-6)),
    ("g_minus_inf", (float("-inf"), 0.5, 1e-3, 1e-6)),
    ("g_nan", (float("nan"), 0.5, 1e-3, 1e-6)),
    ("g_subnormal", (1e-40, 0.5, 1e-3, 1e-6)),
    ("g_subnormal_negative", (-1e-40, -0.5, 1e-3, 1e-6)),
    ("g_smallest_subnormal", (2.0 ** -149, 0.5, -1e-3, 1e-6)),
]
NONFINITE_SPECIALS = ("g_plus_inf", "g_minus_inf", "g_nan")
SPECIAL_FIRST, SPECIAL_STRIDE = 5, 16  # special k sits at index 5 + 16 k (where the vector is that long)
# what an ordinary element is, by index % 8
KINDS = ("generic", "g_zero", "p_zero", "mv_zero", "g_equals_m", "g_cancels_decay", "generic", "generic")


def f32(x):
    return np.float32(x)


def bias_corrections(t, b1, b2):
    """1 - beta^t as Python floats (torch.optim.Adam's own expression)."""
    return 1.0 - float(b1) ** int(t), 1.0 - float(b2) ** int(t)


def adam_step_fp64(p, g, m, v, t, lr, b1, b2, eps, wd, scale, coef=1.0):
    """One update in float64 from the fp32 values, and what fp32 rounding of the kernel lines may move each result by:
    returns p', m', v' and (E_p, E_m, E_v), arrays like p.  First-order propagation with u = 2^-24 and
    G = |g scale coef| + |wd p|, sums of magnitudes, so the bounds hold where g ~ -wd p or g ~ m cancel:

        E_m = K u (|m| + G) + tiny
        E_v = K u (b2 v + (1 - b2) G^2) + tiny
        E_D = s E_m / denom + |D| (E_sqrt / sqrt(bc2) / denom + K u),   E_sqrt = E_v / (2 sqrt(v'))
        E_p = E_D + u |p + D| + tiny

    Where v' is zero or below E_v the first-order E_sqrt has no meaning; |sqrt(a) - sqrt(b)| <= sqrt(|a - b|) always holds,
    and E_sqrt is the smaller of the two: never looser than the first-order term alone.  Where v' is only a few times E_v
    the first-order term understates the true change a little (0.35 against 0.41 of sqrt(E_v) at v' = 2 E_v): that can fail
    a correct kernel, never pass a wrong one."""
    p, g, m, v = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (p, g, m, v))
    sc, cf = float(np.float32(scale)), float(np.float32(coef))
    bc1, bc2 = bias_corrections(t, b1, b2)
    s = lr / bc1
    with np.errstate(all="ignore"):
        gs = g * sc * cf
        gv = gs + wd * p
        m1 = m + (1.0 - b1) * (gv - m)
        v1 = b2 * v + (1.0 - b2) * gv * gv
        root = np.sqrt(v1)
        denom = root / math.sqrt(bc2) + eps
        d = -s * m1 / denom
        p1 = p + d
        G = np.abs(gs) + np.abs(wd * p)
        e_m = K * U * (np.abs(m) + G) + TINY
        e_v = K * U * (b2 * v + (1.0 - b2) * G * G) + TINY
        e_sqrt = np.minimum(np.where(root > 0, e_v / (2.0 * np.where(root > 0, root, 1.0)), np.inf), np.sqrt(e_v))
        e_d = s * e_m / denom + np.abs(d) * (e_sqrt / math.sqrt(bc2) / denom + K * U)
        e_p = e_d + U * np.abs(p1) + TINY
    return p1, m1, v1, (e_p, e_m, e_v)


MUTANTS = ("decay_dropped", "decoupled_decay", "scale_after_decay", "t_off_by_one", "bc2_without_sqrt",
           "eps_over_sqrt_bc2", "eps_inside_sqrt")


def adam_step_fp32(p, g, m, v, t, lr, b1, b2, eps, wd, scale, coef=1.0, mutant=None):
    """The kernel lines in numpy float32, one operation per rounding (host only; returns p', m', v' as float32).
    ``mutant``: one of MUTANTS -- the update written wrongly in that one way (what the bounds must reject)."""
    assert mutant is None or mutant in MUTANTS, mutant
    p, g, m, v = (np.asarray(a, dtype=np.float32) for a in (p, g, m, v))
    bc1, bc2 = bias_corrections(t + 1 if mutant == "t_off_by_one" else t, b1, b2)
    step_size = f32(lr / bc1)                                            # s_step_size = (float)(lr / bc1)
    bc2_sqrt = f32(bc2) if mutant == "bc2_without_sqrt" else f32(math.sqrt(bc2))      # s_bc2_sqrt = (float)sqrt(bc2)
    with np.errstate(all="ignore"):
        pv = p
        if mutant == "scale_after_decay":
            gv = (g + f32(wd) * pv) * f32(scale)
            gv = gv * f32(coef)
        else:
            gv = g * f32(scale)                                          # float gv = a.g[idx] * a.grad_scale;
            gv = gv * f32(coef)                                          # gv = gv * coef;       (autoclip_adam_kernel only)
            if mutant == "decoupled_decay":
                pv = p - f32(lr * wd) * p
            elif mutant != "decay_dropped":
                gv = gv + f32(wd) * pv                                   # gv = gv + (float)wd * pv;
        mv = m + f32(1.0 - b1) * (gv - m)                                # mv = mv + (float)(1.0 - b1) * (gv - mv);
        vv = f32(b2) * v + f32(1.0 - b2) * gv * gv                       # vv = (float)b2 * v + (float)(1.0 - b2) * gv * gv;
        if mutant == "eps_over_sqrt_bc2":
            denom = (np.sqrt(vv) + f32(eps)) / bc2_sqrt
        elif mutant == "eps_inside_sqrt":
            denom = np.sqrt(vv + f32(eps)) / bc2_sqrt
        else:
            denom = np.sqrt(vv) / bc2_sqrt + f32(eps)                    # denom = sqrtf(vv) / s_bc2_sqrt + (float)eps;
        pn = pv + (-step_size * mv) / denom                              # pn = pv + (-s_step_size * mv) / denom;
    for a in (pn, mv, vv):
        assert a.dtype == np.float32
    return pn, mv, vv


def special_indices(n, nonfinite=True):
    """[(index, name)] of the special elements of a vector of n elements."""
    out = []
    for k, (name, _) in enumerate(SPECIALS):
        i = SPECIAL_FIRST + SPECIAL_STRIDE * k
        if i < n and (nonfinite or name not in NONFINITE_SPECIALS):
            out.append((i, name))
    return out


def make_inputs(n, config, coef=1.0, nonfinite=True, seed=0):
    """The constructed vector: dict of float32 arrays p, g, m, v of n elements, ``special`` = [(index, name)] and ``regular``,
    the boolean mask of everything else.  Gradient magnitudes run from 1e-18 to 1e12, v from 0 to (30 |g|)^2, m around g;
    by index % 8 an element has g = 0, p = 0, m = v = 0, g = m, or g = -wd p / (scale coef) to one part in 1e5 (KINDS).
    ``nonfinite=False`` leaves the +-inf / NaN gradients out (their places hold ordinary elements): AutoClip's norm of a
    vector that holds them is not finite, its coefficient NaN, so no coefficient below 1 can be had with them in place."""
    lr, b1, b2, eps, wd, scale = config
    r = np.random.RandomState(1000 + seed)
    sign = lambda: np.where(r.rand(n) < 0.5, -1.0, 1.0)
    g = sign() * 10.0 ** r.uniform(-18.0, 12.0, n)
    p = sign() * 10.0 ** r.uniform(-2.0, 0.5, n)
    m = g * sign() * 10.0 ** r.uniform(-2.0, 1.0, n)
    v = (np.abs(g) * 30.0 * r.rand(n) ** 2) ** 2
    idx = np.arange(n)
    kind = idx % 8
    v[idx % 64 == 6] = 0.0                                                # v = 0 beside an ordinary g and m
    g[kind == 1] = 0.0
    p[kind == 2] = 0.0
    m[kind == 3] = 0.0
    v[kind == 3] = 0.0
    p, g, m, v = (a.astype(np.float32) for a in (p, g, m, v))
    g[kind == 4] = m[kind == 4]
    c = kind == 5
    denom = float(np.float32(scale)) * float(np.float32(coef))
    g[c] = (-(wd * p[c].astype(np.float64)) / denom * (1.0 + 1e-5)).astype(np.float32)
    special = special_indices(n, nonfinite)
    table = dict(SPECIALS)
    regular = np.ones(n, dtype=bool)
    for i, name in special:
        g[i], p[i], m[i], v[i] = (np.float32(x) for x in table[name])
        regular[i] = False
    return dict(p=p, g=g, m=m, v=v, special=special, regular=regular)


def classify(x):
    """0 zero, 1 finite and not zero, 2 +inf, 3 -inf, 4 NaN."""
    x = np.asarray(x, dtype=np.float64)
    out = np.ones(x.shape, dtype=np.int8)
    out[x == 0] = 0
    out[np.isposinf(x)] = 2
    out[np.isneginf(x)] = 3
    out[np.isnan(x)] = 4
    return out


def bound_ratios(got, ref, bound, regular):
    """max over the regular elements of |got - ref| / bound, per array (got, ref, bound: triples for p, m, v).  A result
    or a ratio that is not finite counts as infinitely far off."""
    out = []
    for a, b, e in zip(got, ref, bound):
        a = np.asarray(a, dtype=np.float64)[regular]
        with np.errstate(all="ignore"):
            ratio = np.abs(a - b[regular]) / e[regular]
        ratio[~np.isfinite(a) | ~np.isfinite(ratio)] = np.inf
        out.append(float(ratio.max()) if ratio.size else 0.0)
    return out


def check_against_reference(got, inputs, t, config, coef=1.0):
    """What every comparison of a launch with the statement does: returns the worst ratio to each bound over the regular
    elements (p, m, v) and the list of special elements whose class differs from adam_step_fp32's."""
    lr, b1, b2, eps, wd, scale = config
    args = (inputs["p"], inputs["g"], inputs["m"], inputs["v"], t, lr, b1, b2, eps, wd, scale, coef)
    p1, m1, v1, bounds = adam_step_fp64(*args)
    ratios = bound_ratios(got, (p1, m1, v1), bounds, inputs["regular"])
    want = adam_step_fp32(*args)
    wrong = []
    for i, name in inputs["special"]:
        for what, a, b in zip("pmv", got, want):
            ca, cb = int(classify(np.asarray(a)[i])), int(classify(b[i]))
            if ca != cb:
                wrong.append((name, what, ca, cb))
    return ratios, wrong


def predicted_clip_coef(g_first, g_second, scale, percentile):
    """AutoClip's coefficient for the second of two updates (history: the two norms), from its definition in float64."""
    n = [math.sqrt(float(np.sum((np.asarray(g, dtype=np.float32) * np.float32(scale)).astype(np.float64) ** 2)))
         for g in (g_first, g_second)]
    c = float(np.percentile(np.asarray(n), percentile))
    return min(1.0, c / (n[1] + 1e-6))


def class_mismatches(got, want):
    """[(array, index, class got, class wanted)] over ALL elements of p, m, v (the first few per array)."""
    out = []
    for what, a, b in zip("pmv", got, want):
        ca, cb = classify(a), classify(b)
        for i in np.nonzero(ca != cb)[0][:4]:
            out.append((what, int(i), int(ca[i]), int(cb[i])))
    return out
