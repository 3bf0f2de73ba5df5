"""Where the epoch-side kernels turn over: the masked-metric moments (csrc/k_metrics.hip), the checkpoint copy and the validation
sums (csrc/k_epoch.hip) and AutoClip's update (csrc/k_autoclip.hip).  Plain Python, no device (a test helper, not collected).

The constants restate literals of the sources; tests/test_epoch_kernels_host.py reads them back from there and holds every case
below to the branch it is named for, with the small restatements of the launch geometry at the end of this file.
tests/epoch_kernel_refs.py states the references, tests/test_gpu_epoch_kernels.py runs the cases."""
import numpy as np

# ---- the literals -------------------------------------------------------------------------------------------------------------------
GATRES_WAVE = 64
MET_T = 1024                       # k_metrics.hip: one workgroup of MET_T threads ...
MET_U = 8                          # ... MET_U strides per trip of the element loops
MET_WAVES = MET_T // GATRES_WAVE   # 16 wave partials, added in wave order
MET_TRIP = MET_T * MET_U           # 8192 elements per trip of the workgroup
METRICS_RECORD = 16                # doubles per record; words 12 .. 15 are written as 0.0
SNAP_T = 256                       # k_epoch.hip, snapshot_if_kernel
SNAP_U = 4                         # 16-byte vectors per thread and trip
SNAP_WG_FLOATS = SNAP_T * SNAP_U * 4      # 4096 floats per workgroup and trip
SNAP_MAX_WGS = 2048
AC_THREADS = 256                   # k_autoclip.hip: both launches
AC_NORM_MAX_BLOCKS = 256
AC_UPDATE_MAX_BLOCKS = 512
AC_SEARCH_WAYS = 256               # entries sampled per round of the rank search
AC_COUNT, AC_SNAP_COUNT, AC_SNAP_STEP, AC_SNAP_DROP, AC_OVERFLOW = 0, 1, 2, 3, 4      # k_autoclip.h: ctl words

# ---- 1. moments ---------------------------------------------------------------------------------------------------------------------
# N -> the branch: thread tid takes elements tid + 1024 u + 8192 k; a wave is 64 consecutive tids
MOMENT_N = {
    1: "one element: thread 0 alone, every other lane of every wave adds 0.0",
    63: "one short of a wave",
    64: "exactly one wave",
    65: "the second wave holds one element",
    1023: "one short of the first stride",
    1024: "the first stride exactly: every thread one element",
    1025: "thread 0 takes a second stride (u = 1) within the first trip",
    8191: "one short of a trip: the last thread's eighth stride is out of range",
    8192: "one trip exactly, all eight strides of every thread",
    8193: "thread 0 alone makes a second trip",
    16384: "two whole trips",
    16385: "thread 0 alone makes a third trip",
}
MOMENT_MASKS = {
    "all": "every element kept",
    "most": "about 95 % kept (the training and evaluation mask rate)",
    "last": "only element N - 1",
    "second_trip": "only elements at index >= 8192: nothing kept in the first trip (empty at N <= 8192)",
    "one_per_wave": "one kept element per wave that holds an element: every wave partial is one term or zero",
    "none": "no element kept: M = 0",
}
# (scale, offset): identity; the C-Town-like pressures; offset 0 (|t| <= 0.01 happens); a spread of 0.01 around 1e4, where raw
# second moments cancel (sum p^2 ~ 1e8 M against sum (p - pm)^2 ~ 1e-4 M)
MOMENT_SCALES = [(1.0, 0.0), (12.81, 51.37), (12.81, 0.0), (1e-2, 1e4)]
FMA_SCALE = (12.81, 51.37)         # the designed fma inputs: a product that needs rounding before the add
GUARD_RECORDS = 2                  # records in front of and behind the table that a launch must leave alone
SENTINEL_F64 = -7.0625e77          # the garbage every table word holds before a launch (no sum of the cases comes near it)


def moment_mask(kind, N, seed=0):
    """The boolean mask of a case."""
    i = np.arange(N)
    if kind == "all":
        return np.ones(N, dtype=bool)
    if kind == "most":
        return np.random.RandomState(7000 + N + seed).rand(N) < 0.95
    if kind == "last":
        return i == N - 1
    if kind == "second_trip":
        return i >= MET_TRIP
    if kind == "one_per_wave":
        m = np.zeros(N, dtype=bool)
        for w in range(MET_WAVES):
            if N <= w * GATRES_WAVE:
                break
            tid = w * GATRES_WAVE + (7 * w + 3) % min(GATRES_WAVE, N - w * GATRES_WAVE)      # a lane that holds an element
            mine = np.arange(tid, N, MET_T)                 # the elements thread `tid` takes, in its order
            if mine.size:
                m[mine[0] if w % 2 == 0 else mine[-1]] = True      # even waves: the first stride; odd waves: the last one
        return m
    if kind == "none":
        return np.zeros(N, dtype=bool)
    raise KeyError(kind)


def moment_inputs(N, seed=0):
    """(out, y): scaled fp32 predictions and targets of unit spread, predictions 8 % off; the first elements' targets are 0
    (with offset 0 they descale to |t| <= 0.01 and are not kept by the relative error)."""
    r = np.random.RandomState(100 + N + seed)
    y = r.randn(N).astype(np.float32)
    out = (y + np.float32(0.08) * r.randn(N).astype(np.float32)).astype(np.float32)
    y[: min(50, N // 4)] = 0.0
    return out, y


# ---- 2. snapshot --------------------------------------------------------------------------------------------------------------------
# (source shift, destination shift) in floats off a 16-byte boundary -> the branch
SNAP_SHIFTS = {
    (0, 0): "no head, float4 body, scalar tail",
    (1, 1): "head of 3 floats, float4 body, scalar tail",
    (3, 3): "head of 1 float, float4 body, scalar tail",
    (0, 1): "head of 3 floats, then the source is misaligned: scalar loop",
    (1, 0): "no head, the source is misaligned: scalar loop",
    (2, 1): "head of 3 floats, then the source is misaligned: scalar loop",
}
SNAP_P = {
    1: "count below the head of 3 and equal to the head of 1",
    2: "count below the head of 3",
    3: "count equal to the head of 3: nothing behind it",
    4: "one vector where there is no head; one float behind a head of 3",
    5: "a head and a tail with no vector between them (head 3); one vector (head 1, head 0)",
    7: "one vector behind a head: head 3 + 4, head 1 + 4 + tail 2",
    4095: "one short of a workgroup trip",
    4096: "a workgroup trip of the body exactly where there is no head",
    4097: "one past: a second workgroup",
    4096 + 3: "a workgroup trip of the body exactly behind a head of 3",
    SNAP_MAX_WGS * SNAP_WG_FLOATS + 5: "behind the grid cap: 2048 workgroups; block 0 makes a second trip of the body",
}
SNAP_GUARD = 8                     # guard floats on either side of every destination
SNAP_SENTINEL = -7.25


def snapshot_geometry(count, src_shift, dst_shift):
    """snapshot_if_kernel's split of one array whose allocations start on 16-byte boundaries: head / nvec / tail floats, whether
    the body is the float4 one, the grid, and the trips block 0 makes through its body loop."""
    head = min(((16 - (4 * dst_shift) % 16) % 16) // 4, count)
    vec = (4 * (src_shift + head)) % 16 == 0
    nvec = (count - head) // 4 if vec else 0
    tail = count - head - 4 * nvec if vec else 0
    wgs = min(-(-count // SNAP_WG_FLOATS), SNAP_MAX_WGS)
    if vec:
        per_trip = wgs * SNAP_T * SNAP_U
        trips = -(-nvec // per_trip)
    else:
        per_trip = wgs * SNAP_T
        trips = -(-(count - head) // per_trip)
    return dict(head=head, vec=vec, nvec=nvec, tail=tail, scalar=0 if vec else count - head, wgs=wgs, trips=trips)


# ---- 3. AutoClip --------------------------------------------------------------------------------------------------------------------
AC_P = 3001                        # 12 update workgroups: the history copy strides by 3072 entries
# entries in the history before the first update -> the branch of the rank search (cnt = n0, n0 + 1, n0 + 2, n0 + 3)
AC_PRESET_N0 = {
    255: "no round (hi - lo <= 256), then one at the fourth update",
    256: "no round at the first update, one round from the second on",
    257: "one round with stride 2",
    65535: "one round with stride 256, gap 255",
    65536: "one round with stride 256 / 257, gap 255 / 256",
    65537: "one round with stride 257, gap 256: the last size that needs no second round",
    70000: "two rounds (stride 274, then 2)",
}
AC_PERCENTILES = [0.0, 10.0, 100.0]
AC_UPDATES = ("rank_0", "rank_n0", "in_ties", "inside")         # where the four norms land
AC_CAP_P = {
    65536: "256 norm workgroups: the cap exactly, one trip",
    65537: "257 wanted, 256 run: block 0 of the norm launch makes a second trip",
    131072: "512 update workgroups: the cap exactly",
    131073: "513 wanted, 512 run: block 0 of the update makes a second trip",
}
AC_CAP_UPDATES = 3
AC_OVERFLOW_CAPACITY, AC_OVERFLOW_UPDATES = 4, 6


def ac_search_rounds(cnt):
    """[(stride, gap)] of the rounds the rank search makes over a history of cnt entries when the answer lies in the longest
    gap (any gap but a clipped last one has stride - 1 entries)."""
    lo, hi, out = 0, cnt, []
    while hi - lo > AC_SEARCH_WAYS:
        stride = (hi - lo + AC_SEARCH_WAYS - 1) // AC_SEARCH_WAYS
        lo, hi = lo + 1, lo + stride              # k = 1: the gap behind the first sample
        out.append((stride, hi - lo))
    return out


def ac_blocks(P):
    """(norm workgroups, update workgroups) of gatres_autoclip_adam_step on P parameters."""
    need = -(-P // AC_THREADS)
    return min(need, AC_NORM_MAX_BLOCKS), min(need, AC_UPDATE_MAX_BLOCKS)


def ac_copy_trips(P, t):
    """Trips block 0 makes through the copy of the next sorted history (t entries) in the update launch."""
    return -(-t // (ac_blocks(P)[1] * AC_THREADS))


def ac_preset_history(n0, seed=0):
    """(sorted history, log): n0 norms.  The lowest fifth are float64 values with all their bits; the eight around index
    n0 / 10 lie far apart (0.61 .. 0.95) and are drawn until, at one of the four updates of the case or more, the 10th
    percentile's two neighbours make the two expressions of numpy's lerp differ in their last bit (one pair in twenty to fifty does, none at a weight of 0.5;
    at n0 = 70000 the weight stays below 0.5 and there is one expression only).  The rest are fp32-representable values drawn from at most 300 levels (n0 / 16 of them), so that they form
    runs of exact ties a norm can be made to land in.  The log is the history in a shuffled (step) order."""
    r = np.random.RandomState(4000 + n0 + seed)
    low = n0 // 5
    a, k = np.sort(r.uniform(0.5, 0.6, low)), n0 // 10
    for _ in range(5000):
        a[k - 3:k + 5] = 0.61 + np.sort(r.uniform(0.0, 0.34, 8))
        differ = 0
        for j in range(4):                       # update j + 1 sees t = n0 + j + 1 entries, the first update's 0.25 in front
            h = np.float64(n0 + j) * (np.float64(10.0) / np.float64(100.0))
            i0 = int(np.floor(h))
            g, va, vb = h - np.float64(i0), a[i0 - 1], a[i0]
            differ += bool(g >= 0.5 and va + (vb - va) * g != vb - (vb - va) * (np.float64(1.0) - g))
        if differ or n0 == 70000:
            break
    else:
        raise AssertionError(n0)
    a[k + 5:] = np.sort(r.uniform(0.96, 1.0, low - k - 5))
    nlev = min(300, max(8, n0 // 16))
    levels = np.float32(1.0) + np.arange(1, nlev + 1, dtype=np.float32) * np.float32(1.0 / 256)
    b = levels[r.randint(0, levels.size, n0 - low)].astype(np.float64)
    hist = np.sort(np.concatenate([a, b]))
    return hist, hist[r.permutation(n0)]


def ac_preset_norms(hist):
    """The four norms of a preset case, each an fp32 value (the gradient is that value in one element, zero elsewhere, so
    its fp64 norm is the value itself): below every entry, above every entry, equal to an entry of a run of ties, and strictly
    between two distinct neighbours in the upper part."""
    tie = float(hist[(7 * hist.size) // 10])
    assert np.float32(tie) == tie and (hist == tie).sum() >= 2
    upper = np.unique(hist[hist > 1.0])
    between = float(np.float32(0.5 * (upper[3] + upper[4])))
    assert upper[3] < between < upper[4]
    return {"rank_0": 0.25, "rank_n0": 4.0, "in_ties": tie, "inside": between}


# ---- 4. validation sums -------------------------------------------------------------------------------------------------------------
VAL_B = {
    1: "one batch",
    63: "one short of a wave",
    64: "one wave exactly",
    65: "a second load of one batch",
    128: "two waves exactly",
    129: "a third load",
}
VAL_NAN_B = 65                     # also run with a NaN loss in the middle (batch 32)
