"""References for the epoch-side kernels, written from the definitions (a test helper, not collected; numpy only).

tests/epoch_kernel_cases.py says at which sizes they run, tests/test_gpu_epoch_kernels.py compares the kernels with them through
the ``*_failures`` functions below, and tests/test_epoch_kernels_host.py shows on the host that the same functions reject planted
wrong answers (the ``mutant`` arguments: what a wrong kernel would have written)."""
import math

import numpy as np

import epoch_kernel_cases as EC

U = 2.0 ** -53                     # unit round-off of fp64
F32 = np.float32
MOMENT_MUTANTS = ("fma_descale", "keep_ge", "drops_last_partial_trip")
PLAIN_FIELDS = (1, 2, 3, 4, 5, 10)
CENTRED_FIELDS = (6, 7, 8)
COUNT_FIELDS = (0, 9, 11)


# ---- 1. moments ---------------------------------------------------------------------------------------------------------------------
def descale32(s, scale, offset, fma=False):
    """``s * scale + offset`` as torch rounds it on fp32 tensors: a multiply, then an add, each rounded to fp32.
    ``fma``: the wrong one -- one rounding (the fp64 product of two fp32 values is exact, and so is its sum with an fp32 offset
    of similar size; the conversion is then the only rounding)."""
    s = np.asarray(s, dtype=F32)
    if fma:
        return (s.astype(np.float64) * float(F32(scale)) + float(F32(offset))).astype(F32)
    return ((s * F32(scale)).astype(F32) + F32(offset)).astype(F32)


def _gamma(k):
    return k * U / (1.0 - k * U)


def moments(out, y, mask, scale=1.0, offset=0.0, mutant=None):
    """The record ``gatres_masked_metrics`` writes, from its definition (include/gatres.h gives the layout), and how far a
    correct kernel may be from it.  Returns ``dict(record, terms, abs, bound)``.

    Counts (fields 0, 9, 11): M, the number of kept elements; ``|t| > 0.01`` and ``|t - p| <= t * 0.1`` evaluated in numpy
    float32 on the descaled values, as the reference's metric functions evaluate them on float32 tensors.  EQUAL or wrong.

    Plain sums (1 loss, 2 |d|, 3 d^2, 4 p, 5 t, 10 relative error): every term is formed in float64 from the fp32 values by
    the operations of the definition (a difference, a product, a quotient: each one IEEE operation on operands that are exact,
    so a term has the same bits in any implementation that does not contract them) and the terms are summed with
    ``math.fsum``: the record holds the exact sum, rounded once.  ``abs[f]`` is sum |term|, ``terms[f]`` the terms themselves, so that a comparison can
    take ``fsum(terms + [-got])``, the exact distance, rounded once.  Any order of adding n fp64 numbers is within
    (n - 1) u sum |term| of their exact sum, u = 2^-53 (Jeannerod and Rump, "Improved error bounds for inner products in
    floating-point arithmetic", SIAM J. Matrix Anal. Appl. 34 (2013): the first-order constant holds without a higher-order
    term): ``bound[f] = (n - 1) u abs[f]`` with n = M (field 10: n = the keep count, the number of its terms).

    Centred sums (6 sum (p - pm)^2, 7 sum (t - tm)^2, 8 sum (p - pm)(t - tm)), around the exact means pm = S_p / M,
    tm = S_t / M rounded once.  A kernel has a mean pm^ = fl(S_p^ / M) from its own sum S_p^, so with A_p = sum |p|

        |pm^ - pm| <= e_p := (1 + 4 u) ((M - 1) u A_p / M + u |pm|)            (the bound on S_p^, then one division)

    and it adds the M terms fl(fl(p_i - pm^)^2).  With x_i = p_i - pm (exact, sum x_i = 0) and eps = pm - pm^:
    sum (x_i + eps)^2 = C + M eps^2 exactly -- the mean's error enters in second order only -- and every term carries at most
    M + 2 roundings (the difference, squared: 2; the product: 1; at most M - 1 additions), so

        |C^ - C| <= M e_p^2 + g(M + 2) (C + M e_p^2),        g(k) = k u / (1 - k u)                        (fields 6, 7)
        |C^ - C| <= M e_p e_t + g(M + 2) sqrt((C_p + M e_p^2) (C_t + M e_t^2))                             (field 8)

    the second by sum (x_i + eps_p)(z_i + eps_t) = C_pt + M eps_p eps_t and Cauchy-Schwarz on sum |x_i + eps_p| |z_i + eps_t|.
    The reference forms its terms the same way around its own mean, rounded twice (the sum, the division:
    |rho| <= 2 u (1 + u) |pm|), and sums them with fsum: four roundings per term, so it obeys the same two expressions with rho for e and g(4) for g(M + 2).  ``bound[f]`` is the SUM of
    the kernel's allowance and the reference's own error, with C_p, C_t replaced by upper bounds got from the reference's
    values through its own error.  Nothing in it is fitted to a kernel's output; it is evaluated in fp64 (relative 1e-15).
    At M = 0 every sum is 0.0 and every bound 0."""
    assert mutant is None or mutant in MOMENT_MUTANTS, mutant
    m = np.asarray(mask, dtype=bool).reshape(-1).copy()
    so_all, st_all = np.asarray(out, dtype=F32).reshape(-1), np.asarray(y, dtype=F32).reshape(-1)
    if mutant == "drops_last_partial_trip":
        m[(m.size // EC.MET_TRIP) * EC.MET_TRIP:] = False
    so, st = so_all[m], st_all[m]
    p, t = (descale32(a, scale, offset, fma=mutant == "fma_descale") for a in (so, st))
    pd, td = p.astype(np.float64), t.astype(np.float64)
    M = int(so.size)
    with np.errstate(all="ignore"):
        keep = np.abs(t) >= F32(0.01) if mutant == "keep_ge" else np.abs(t) > F32(0.01)
        acc = np.abs(t - p) <= t * F32(0.1)
        d = pd - td
        ds = so.astype(np.float64) - st.astype(np.float64)
        terms = {1: ds * ds, 2: np.abs(d), 3: d * d, 4: pd, 5: td, 10: np.abs(np.abs(td[keep] - pd[keep]) / td[keep])}
    r = np.zeros(EC.METRICS_RECORD, dtype=np.float64)
    r[0], r[9], r[11] = M, int(keep.sum()), int(acc.sum())
    absum, bound = {}, {}
    for f, v in terms.items():
        r[f] = math.fsum(v)
        absum[f] = math.fsum(np.abs(v))
        bound[f] = max(v.size - 1, 0) * U * absum[f]
    if M:
        pm, tm = r[4] / M, r[5] / M
        x, z = pd - pm, td - tm
        terms.update({6: x * x, 7: z * z, 8: x * z})
        for f in CENTRED_FIELDS:
            r[f] = math.fsum(terms[f])
            absum[f] = math.fsum(np.abs(terms[f]))
        e = {4: (1 + 4 * U) * ((M - 1) * U * absum[4] / M + U * abs(pm)), 5: (1 + 4 * U) * ((M - 1) * U * absum[5] / M + U * abs(tm))}
        rho = {4: 2 * U * abs(pm) * (1 + U), 5: 2 * U * abs(tm) * (1 + U)}
        gk, gr = _gamma(M + 2), _gamma(4)
        up = {f: (r[f] + M * rho[s] ** 2 * (1 + gr)) / (1 - gr) for f, s in ((6, 4), (7, 5))}     # C <= this
        for f, s in ((6, 4), (7, 5)):
            bound[f] = (M * e[s] ** 2 + gk * (up[f] + M * e[s] ** 2)) + (M * rho[s] ** 2 + gr * (up[f] + M * rho[s] ** 2))
        bound[8] = (M * e[4] * e[5] + gk * math.sqrt((up[6] + M * e[4] ** 2) * (up[7] + M * e[5] ** 2))) + \
                   (M * rho[4] * rho[5] + gr * math.sqrt((up[6] + M * rho[4] ** 2) * (up[7] + M * rho[5] ** 2)))
    else:
        for f in CENTRED_FIELDS:
            terms[f], absum[f], bound[f] = np.zeros(0), 0.0, 0.0
    return dict(record=r, terms=terms, abs=absum, bound=bound)


def moment_failures(got, ref):
    """Every comparison of one record ``got`` (16 doubles) with ``moments(...)``: returns (failures, worst error / bound).
    Counts equal; plain sums by their exact distance; centred sums against the reference's value; words 12 .. 15 zero.  A sum
    whose bound is 0 (no term, one term, M = 0) must be the reference's bits (+0.0 where there is no term)."""
    got = np.asarray(got, dtype=np.float64)
    fails, worst = [], 0.0
    for f in COUNT_FIELDS:
        if got[f] != ref["record"][f]:
            fails.append(f"field {f}: count {got[f]!r}, reference {ref['record'][f]!r}")
    for f in PLAIN_FIELDS + CENTRED_FIELDS:
        g, b = float(got[f]), ref["bound"][f]
        if not math.isfinite(g):
            fails.append(f"field {f}: {g!r}")
            continue
        err = abs(math.fsum(ref["terms"][f].tolist() + [-g])) if f in PLAIN_FIELDS else abs(g - ref["record"][f])
        if b == 0.0:
            if err != 0.0 or (ref["terms"][f].size == 0 and math.copysign(1.0, g) < 0):
                fails.append(f"field {f}: {g!r} where the reference has {ref['record'][f]!r} and the bound is 0")
            continue
        worst = max(worst, err / b)
        if err > b:
            fails.append(f"field {f}: {g!r}, reference {ref['record'][f]!r}, error {err:.3e} > bound {b:.3e}")
    for f in range(12, EC.METRICS_RECORD):
        if got[f] != 0.0 or math.copysign(1.0, got[f]) < 0:
            fails.append(f"word {f}: {got[f]!r}, not +0.0")
    return fails, worst


def _neighbours(x):
    x = np.asarray(x, dtype=F32)
    return np.nextafter(x, F32(-np.inf)), x, np.nextafter(x, F32(np.inf))


def designed_unit():
    """(out, y) at scale 1, offset 0 (descaling is exact): every element sits at a value where one of the two fp32 predicates
    turns.  ``|t| > 0.01``: t = +-float32(0.01) and its two neighbours.  ``|t - p| <= t * 0.1``: for 48 positive t,
    p = fl(t - fl(0.1f t)) and fl(t + fl(0.1f t)), each with its two neighbours; the same construction on negative t, for which
    the predicate is never true (also at p = t)."""
    r = np.random.RandomState(11)
    ts, ps = [], []
    c = F32(0.01)
    for sign in (F32(1), F32(-1)):
        for v in _neighbours(c):
            ts.append(sign * v)
            ps.append(sign * v * F32(1.05))
    tpos = np.concatenate([(10.0 ** r.uniform(-1.5, 2.0, 44)).astype(F32), np.array([0.5, 1.0, 3.0, 1e-3], dtype=F32)])
    for t in np.concatenate([tpos, -tpos]):
        h = F32(t * F32(0.1))
        for base in (F32(t - h), F32(t + h)):
            for p in _neighbours(base):
                ts.append(t)
                ps.append(p)
        ts.append(t)
        ps.append(t)
    return np.array(ps, dtype=F32), np.array(ts, dtype=F32)


def designed_fma(count=48):
    """(out, y) at EC.FMA_SCALE: targets s_t whose product with float32(12.81) needs rounding before the add, so that the
    twice-rounded t differs from the once-rounded one, each paired with a prediction s_p for which ``|t - p| <= t * 0.1`` is
    TRUE with the rounding of the definition and FALSE with an fma's (found by scanning 513 consecutive fp32 values of s_p
    around the value where p = 0.9 t): the accuracy count of a kernel that descales with an fma is lower by ``count``."""
    sc, of = EC.FMA_SCALE
    r = np.random.RandomState(12)
    outs, ys = [], []
    while len(ys) < count:
        s_t = r.randn(4096).astype(F32)
        s_t = s_t[descale32(s_t, sc, of) != descale32(s_t, sc, of, fma=True)]
        for st in s_t:
            t2 = descale32(st, sc, of)
            base = F32((0.9 * float(t2) - float(F32(of))) / float(F32(sc)))
            if abs(base) < 1e-3:
                continue
            cand = (np.full(513, base, dtype=F32).view(np.int32) + np.arange(-256, 257, dtype=np.int32)).view(F32)
            tt = np.full(cand.shape, st, dtype=F32)
            ok = []
            for fma in (False, True):
                p, t = descale32(cand, sc, of, fma), descale32(tt, sc, of, fma)
                ok.append(np.abs(t - p) <= t * F32(0.1))
            hit = np.nonzero(ok[0] & ~ok[1])[0]
            if hit.size:
                outs.append(cand[hit[0]])
                ys.append(st)
                if len(ys) == count:
                    break
    return np.array(outs, dtype=F32), np.array(ys, dtype=F32)


# ---- 2. snapshot --------------------------------------------------------------------------------------------------------------------
SNAP_MUTANTS = ("head_one_too_long",)


def snapshot_expected(dst_raw, src, dst_shift, copies):
    """What a destination buffer holds after ``gatres_snapshot_if``: the copy as slices.  dst_raw: guard floats, the shift, P
    floats, guard floats; src: the P source floats."""
    want = np.array(dst_raw, copy=True)
    if copies:
        lo = EC.SNAP_GUARD + dst_shift
        want[lo:lo + src.size] = src
    return want


def snapshot_failures(dst_after, dst_before, src, dst_shift, copies):
    """Bit for bit: the P floats are the source's (or untouched where nothing is to be copied), every guard float intact."""
    want = snapshot_expected(dst_before, src, dst_shift, copies)
    a, b = np.asarray(dst_after, dtype=F32).view(np.uint32), want.view(np.uint32)
    lo, hi = EC.SNAP_GUARD + dst_shift, EC.SNAP_GUARD + dst_shift + src.size
    fails = []
    if not np.array_equal(a[lo:hi], b[lo:hi]):
        bad = np.nonzero(a[lo:hi] != b[lo:hi])[0]
        fails.append(f"{bad.size} of {src.size} floats differ, the first at {int(bad[0])}")
    if not (np.array_equal(a[:lo], b[:lo]) and np.array_equal(a[hi:], b[hi:])):
        fails.append("a guard float changed")
    return fails


def snapshot_emulate(dst_raw, src_padded, src_shift, dst_shift, P, mutant=None):
    """snapshot_if_kernel's three loops on the host, by EC.snapshot_geometry (src_padded: the source with floats behind it,
    as device memory has).  ``mutant``: the head loop runs one float further than the head the body starts at."""
    assert mutant is None or mutant in SNAP_MUTANTS
    g = EC.snapshot_geometry(P, src_shift, dst_shift)
    out = np.array(dst_raw, copy=True)
    lo = EC.SNAP_GUARD + dst_shift
    head = g["head"] + (1 if mutant == "head_one_too_long" and g["head"] else 0)
    out[lo:lo + head] = src_padded[:head]
    body0, body1 = g["head"], g["head"] + (4 * g["nvec"] if g["vec"] else g["scalar"])
    out[lo + body0:lo + body1] = src_padded[body0:body1]
    out[lo + body1:lo + P] = src_padded[body1:P]
    return out


# ---- 3. AutoClip --------------------------------------------------------------------------------------------------------------------
AC_MUTANTS = ("rank_before_a_tie", "lerp_one_form")


def percentile_linear(sorted_hist, q, one_form=False):
    """numpy's ``percentile(..., method="linear")`` written out: virtual index h = (t - 1) (q / 100), its two neighbours, and
    numpy's ``_lerp``: ``a + (b - a) g``, replaced by ``b - (b - a) (1 - g)`` where g >= 0.5.  ``one_form``: the wrong one,
    the first expression for every g (equal in exact arithmetic, not in its last bits)."""
    a = np.asarray(sorted_hist, dtype=np.float64)
    t = a.size
    h = np.float64(t - 1) * (np.float64(q) / np.float64(100.0))
    i0 = min(max(int(math.floor(h)), 0), t - 1)
    i1 = min(i0 + 1, t - 1)
    g = h - np.float64(i0)
    va, vb = a[i0], a[i1]
    diff = vb - va
    if g >= 0.5 and not one_form:
        return float(vb - diff * (np.float64(1.0) - g))
    return float(va + diff * g)


def autoclip_reference(log, percentile):
    """After an update whose norm is log[-1]: the sorted history, the clip value and the coefficient, by numpy."""
    h = np.asarray(log, dtype=np.float64)
    c = float(np.percentile(h, percentile))
    return np.sort(h), c, min(1.0, c / (float(h[-1]) + 1e-6))


def autoclip_emulate(sorted_hist, n, percentile, mutant=None):
    """The update's bookkeeping on the host: the rank of n (entries that sort before it), the next sorted copy, the clip
    value, the coefficient.  Mutants: a search that, where n equals an entry, returns the index in front of the last smaller
    entry; the one-expression lerp."""
    assert mutant is None or mutant in AC_MUTANTS
    a = np.asarray(sorted_hist, dtype=np.float64)
    r = int(np.searchsorted(a, n, side="left"))
    if mutant == "rank_before_a_tie" and r < a.size and a[r] == n and r > 0:
        r -= 1
    nxt = np.concatenate([a[:r], [n], a[r:]])
    c = percentile_linear(nxt, percentile, one_form=mutant == "lerp_one_form")
    return nxt, c, min(1.0, c / (n + 1e-6))


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


def autoclip_failures(sorted_live, log, outs, percentile, norm):
    """One update against numpy.  sorted_live / log: the live sorted buffer and the log, both of the new count; outs: the
    launch's {norm, clip, coef}.  The sorted buffer is np.sort(log) bit for bit, the log's new entry and the norm output are
    ``norm`` (exact where the gradient has one non-zero element; 1e-12 relative otherwise), clip and coefficient within 1e-12
    relative of np.percentile / min(1, c / (n + 1e-6)), and the clip value the bits of ``percentile_linear`` -- numpy's own
    expression, which tests/test_epoch_kernels_host.py holds to np.percentile bit for bit on these histories."""
    want_sorted, c, coef = autoclip_reference(log, percentile)
    fails = []
    if not np.array_equal(np.asarray(sorted_live).view(np.uint64), want_sorted.view(np.uint64)):
        fails.append("the live sorted buffer is not np.sort(log)")
    if float(log[-1]) != float(outs[0]) or rel(outs[0], norm) > 1e-12:
        fails.append(f"norm {outs[0]!r}, log {log[-1]!r}, wanted {norm!r}")
    if rel(outs[1], c) > 1e-12 or rel(outs[2], coef) > 1e-12:
        fails.append(f"clip {outs[1]!r} / coef {outs[2]!r}, numpy {c!r} / {coef!r}")
    if float(outs[1]) != percentile_linear(want_sorted, percentile):
        fails.append(f"clip {float(outs[1]).hex()} is not numpy's lerp {percentile_linear(want_sorted, percentile).hex()}")
    return fails


# ---- 4. validation sums -------------------------------------------------------------------------------------------------------------
def val_sums(losses, graphs):
    """The host loop: ``acc += loss_b * g_b`` batch by batch in fp64 (a product and a sum, each rounded), and the graph count."""
    acc, n = 0.0, 0
    for l, g in zip(np.asarray(losses, dtype=F32), graphs):
        acc += float(l) * int(g)
        n += int(g)
    return acc, float(n)


def val_inputs(B, nan_at=None):
    r = np.random.RandomState(900 + B)
    losses = (r.rand(B) * 10.0 ** r.uniform(-6, 2, B)).astype(F32)
    if nan_at is not None:
        losses[nan_at] = np.nan
    return losses, r.randint(1, 33, size=B).astype(np.int32)
