"""tests/epoch_kernel_cases.py and tests/epoch_kernel_refs.py against the kernel sources, on the host.

tests/test_gpu_epoch_kernels.py runs the masked-metric moments, the checkpoint copy, the validation sums and AutoClip's update at
sizes chosen to lie just past a wave, a stride, a trip, a capped grid, a round of the rank search.  Those sizes are only as good as
the constants they were chosen against: this module reads the literals from the sources, asserts that epoch_kernel_cases.py
restates them and that every case still reaches the branch it is named for, holds the references to independent statements (the
older moment reference, np.percentile, the kernel's own order of summation restated in numpy) and shows that the comparisons the
GPU module makes reject six planted wrong answers.  No GPU, no kernel launches."""
import math
import os
import re

import numpy as np
import pytest

import epoch_kernel_cases as EC
import epoch_kernel_refs as R
import metric_moments_ref as MR
from test_proj_turnover_host import body_of, one

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gnn-pressure-estimation_amd", "csrc")


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


MET, EPO, ACL, ACH, COMMON = (_read(n) for n in ("k_metrics.hip", "k_epoch.hip", "k_autoclip.hip", "k_autoclip.h", "gatres_common.h"))


# ---- 1. the literals ----------------------------------------------------------------------------------------------------------------
def test_cases_restate_the_literals_of_the_sources():
    assert int(one(r"#define GATRES_WAVE (\d+)", COMMON)) == EC.GATRES_WAVE
    assert "return __fadd_rn(__fmul_rn(s, scale), offset);" in body_of(COMMON, "float gatres_descale(", "\n}\n")
    # moments
    assert int(one(r"constexpr int MET_T = (\d+);", MET)) == EC.MET_T
    assert int(one(r"constexpr int MET_U = (\d+);", MET)) == EC.MET_U
    assert "constexpr int MET_WAVES = MET_T / GATRES_WAVE;" in MET and EC.MET_WAVES == EC.MET_T // EC.GATRES_WAVE == 16
    k = body_of(MET, "void masked_metrics_kernel(", "\n}\n")
    assert k.count("for (long long i0 = tid; i0 < N; i0 += MET_U * MET_T) {") == 2        # 64-bit: i0 + u * MET_T cannot wrap
    assert k.count("const long long i = i0 + u * MET_T;") == 2 and "int i0" not in k.replace("long long i0", "")
    assert "if (fabsf(t) > 0.01f) {" in k and "if (fabsf(__fsub_rn(t, p)) <= __fmul_rn(t, 0.1f)) a[8] += 1.0;" in k
    assert "for (int f = 12; f < GATRES_METRICS_RECORD; ++f) r[f] = 0.0;" in k
    assert "dim3(1), dim3(MET_T)" in body_of(MET, 'extern "C" int gatres_masked_metrics(', "\n}\n")
    assert int(one(r"#define GATRES_METRICS_RECORD (\d+)", _read(os.path.join("..", "..", "include", "gatres.h")))) == EC.METRICS_RECORD
    # snapshot
    assert int(one(r"constexpr int SNAP_T = (\d+);", EPO)) == EC.SNAP_T
    assert int(one(r"constexpr int SNAP_U = (\d+);", EPO)) == EC.SNAP_U
    assert "constexpr int SNAP_WG_FLOATS = SNAP_T * SNAP_U * 4;" in EPO and EC.SNAP_WG_FLOATS == 4096
    assert int(one(r"constexpr int SNAP_MAX_WGS = (\d+);", EPO)) == EC.SNAP_MAX_WGS
    k = body_of(EPO, "void snapshot_if_kernel(", "\n}\n")
    assert "(((16u - (unsigned)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u) / 4u)" in k and "if (head > count) head = count;" in k
    assert "const bool vec = (reinterpret_cast<uintptr_t>(src + head) & 15u) == 0;" in k
    assert "if (flag && !(flag[0] != 0.0)) return;" in k
    ln = body_of(EPO, 'extern "C" int gatres_snapshot_if(', "\n}\n")
    assert "((long long)count + SNAP_WG_FLOATS - 1) / SNAP_WG_FLOATS" in ln and "if (wgs > SNAP_MAX_WGS) wgs = SNAP_MAX_WGS;" in ln
    # validation sums
    k = body_of(EPO, "void epoch_val_sums(", "\n}\n")
    assert "for (int b0 = 0; b0 < B; b0 += GATRES_WAVE) {" in k and "acc = __dadd_rn(acc, __shfl(prod, i));" in k
    # AutoClip
    assert int(one(r"constexpr int AC_NORM_MAX_BLOCKS = (\d+);", ACL)) == EC.AC_NORM_MAX_BLOCKS
    assert int(one(r"constexpr int AC_UPDATE_MAX_BLOCKS = (\d+);", ACL)) == EC.AC_UPDATE_MAX_BLOCKS
    for name in ("AC_COUNT", "AC_SNAP_COUNT", "AC_SNAP_STEP", "AC_SNAP_DROP", "AC_OVERFLOW"):
        assert int(one(r"constexpr int %s = (\d+);" % name, ACH)) == getattr(EC, name)
    k = body_of(ACL, "void autoclip_adam_kernel(", "\n}\n")
    w = str(EC.AC_SEARCH_WAYS)
    assert "while (hi - lo > %s) {" % w in k and "stride = (hi - lo + %d) / %s" % (EC.AC_SEARCH_WAYS - 1, w) in k
    assert "const long long gstride = (long long)a.update_blocks * %d;" % EC.AC_THREADS in k
    assert "for (long long i = (long long)blockIdx.x * %d + tid; i < t; i += gstride) B[i] = sorted_at(i);" % EC.AC_THREADS in k
    assert "const bool overflow = cnt >= (unsigned long long)a.capacity;" in k and "if (overflow) a.ctl[AC_OVERFLOW] = 1ULL;" in k
    assert "const double c = gam >= 0.5 ? vb - diff * (1.0 - gam) : va + diff * gam;" in k
    assert set(re.findall(r"__launch_bounds__\((\d+)\)", ACL)) == {str(EC.AC_THREADS)}
    assert "(count + 255) / 256" in body_of(ACL, 'extern "C" int32_t gatres_autoclip_partials(', "\n}\n")


# ---- 2. every case reaches its branch -----------------------------------------------------------------------------------------------
def _thread_elements(tid, N):
    """(trips, strides taken in the last trip) of thread tid of the moments kernel."""
    trips = len(range(tid, N, EC.MET_TRIP))
    if not trips:
        return 0, 0
    last = tid + (trips - 1) * EC.MET_TRIP
    return trips, len(range(last, N, EC.MET_T)[:EC.MET_U])


def test_moment_sizes_reach_the_turnovers_they_name():
    T = _thread_elements
    assert T(0, 1) == (1, 1) and T(1, 1) == (0, 0)
    assert T(62, 63)[0] == 1 and T(63, 63)[0] == 0 and T(63, 64)[0] == 1 and T(64, 64)[0] == 0 and T(64, 65) == (1, 1)
    assert T(1022, 1023) == (1, 1) and T(1023, 1023)[0] == 0 and T(1023, 1024) == (1, 1) and T(0, 1024) == (1, 1)
    assert T(0, 1025) == (1, 2) and T(1, 1025) == (1, 1)
    assert T(1023, 8191) == (1, 7) and T(1022, 8191) == (1, 8) and T(1023, 8192) == (1, 8)
    assert T(0, 8193) == (2, 1) and T(1, 8193) == (1, 8)
    assert T(0, 16384) == (2, 8) and T(1023, 16384) == (2, 8) and T(0, 16385) == (3, 1) and T(1, 16385) == (2, 8)
    assert sorted(EC.MOMENT_N) == [1, 63, 64, 65, 1023, 1024, 1025, 8191, 8192, 8193, 16384, 16385]
    assert EC.MOMENT_SCALES == [(1.0, 0.0), (12.81, 51.37), (12.81, 0.0), (1e-2, 1e4)]


def test_moment_masks_are_what_their_names_say():
    assert list(EC.MOMENT_MASKS) == ["all", "most", "last", "second_trip", "one_per_wave", "none"]
    for N in EC.MOMENT_N:
        m = {k: EC.moment_mask(k, N) for k in EC.MOMENT_MASKS}
        assert all(v.dtype == bool and v.shape == (N,) for v in m.values())
        assert m["all"].all() and not m["none"].any() and m["last"].sum() == 1 and m["last"][N - 1]
        assert m["second_trip"].sum() == max(N - EC.MET_TRIP, 0) and not m["second_trip"][:EC.MET_TRIP].any()
        if N >= 1024:
            assert 0.9 < m["most"].mean() < 0.99
        kept = np.nonzero(m["one_per_wave"])[0]
        waves = (kept % EC.MET_T) // EC.GATRES_WAVE
        assert len(set(waves)) == len(waves) == min(EC.MET_WAVES, -(-N // EC.GATRES_WAVE))       # one per wave that has elements
    m = EC.moment_mask("one_per_wave", 16385)
    assert (np.nonzero(m)[0] >= EC.MET_TRIP).sum() == EC.MET_WAVES // 2                          # odd waves: in the last trip
    out, y = EC.moment_inputs(16385)
    assert (y[:50] == 0).all() and out.dtype == y.dtype == np.float32


def test_snapshot_cases_reach_the_paths_they_name():
    G = EC.snapshot_geometry
    assert sorted(EC.SNAP_P) == [1, 2, 3, 4, 5, 7, 4095, 4096, 4097, 4099, 2048 * 4096 + 5]
    assert list(EC.SNAP_SHIFTS) == [(0, 0), (1, 1), (3, 3), (0, 1), (1, 0), (2, 1)]
    big = EC.SNAP_MAX_WGS * EC.SNAP_WG_FLOATS + 5
    for (s, d), heads in (((1, 1), 3), ((3, 3), 1)):
        # head, float4 body and tail in one launch -- the path no other test runs
        full = [P for P in EC.SNAP_P if (lambda g: g["head"] == heads and g["vec"] and g["nvec"] > 0 and g["tail"] > 0)(G(P, s, d))]
        assert any(4000 < P < 5000 for P in full) and (heads == 3 or any(P < 16 for P in full)), (s, d, full)
        assert G(1, s, d)["head"] == 1 and G(1, s, d)["nvec"] == 0 and G(1, s, d)["tail"] == 0
    assert [G(P, 1, 1)["head"] for P in (1, 2, 3, 4)] == [1, 2, 3, 3]                             # count < head, == head, past it
    assert G(5, 1, 1) == dict(head=3, vec=True, nvec=0, tail=2, scalar=0, wgs=1, trips=0)
    assert G(7, 1, 1)["nvec"] == 1 and G(7, 1, 1)["tail"] == 0 and G(7, 3, 3)["tail"] == 2
    assert G(4096, 0, 0) == dict(head=0, vec=True, nvec=1024, tail=0, scalar=0, wgs=1, trips=1)
    assert G(4095, 0, 0)["nvec"] == 1023 and G(4095, 0, 0)["tail"] == 3 and G(4097, 0, 0)["wgs"] == 2
    assert G(4099, 1, 1)["nvec"] == 1024 and G(4099, 1, 1)["tail"] == 0 and G(4099, 3, 3)["nvec"] == 1024 and G(4099, 3, 3)["tail"] == 2
    for s, d in ((0, 1), (1, 0), (2, 1)):
        assert not G(4097, s, d)["vec"] and G(4097, s, d)["nvec"] == 0 and G(4097, s, d)["scalar"] == 4097 - G(4097, s, d)["head"]
    assert G(4097, 1, 0)["head"] == 0 and G(4097, 0, 1)["head"] == 3 and G(4097, 2, 1)["head"] == 3
    # behind the grid cap: 2048 workgroups, and block 0 comes round again
    assert G(big, 0, 0)["wgs"] == EC.SNAP_MAX_WGS and G(big - 5, 0, 0)["wgs"] == EC.SNAP_MAX_WGS and G(big - 5, 0, 0)["trips"] == 1
    assert G(big, 0, 0)["trips"] == 2 and G(big, 3, 3)["trips"] == 2 and G(big, 1, 1)["trips"] == 1
    assert G(big, 1, 0)["trips"] == 17 and G(big, 0, 1)["trips"] == 17
    assert 6 * 4 * (big + 2 * EC.SNAP_GUARD + 3) < 210e6                                           # "about 200 MB"


def test_autoclip_cases_reach_the_rounds_trips_and_caps_they_name():
    S = EC.ac_search_rounds
    assert sorted(EC.AC_PRESET_N0) == [255, 256, 257, 65535, 65536, 65537, 70000] and EC.AC_PERCENTILES == [0.0, 10.0, 100.0]
    assert S(255) == [] and S(256) == [] and S(257) == [(2, 1)] and S(258) == [(2, 1)]
    assert S(65535) == [(256, 255)] and S(65536) == [(256, 255)] and S(65537) == [(257, 256)] and S(65540) == [(257, 256)]
    assert len(S(65792)) == 1 and len(S(65793)) == 2               # the first history that needs two rounds: 257 * 256 + 1
    assert all(len(S(70000 + i)) == 2 for i in range(4)) and S(70000) == [(274, 273), (2, 1)]
    assert EC.ac_blocks(EC.AC_P) == (12, 12) and EC.ac_copy_trips(EC.AC_P, 256) == 1 and EC.ac_copy_trips(EC.AC_P, 70001) == 23
    assert all(EC.ac_copy_trips(EC.AC_P, n0 + 1) >= 22 for n0 in EC.AC_PRESET_N0 if n0 >= 65535)
    assert sorted(EC.AC_CAP_P) == [65536, 65537, 131072, 131073]
    assert EC.ac_blocks(65536) == (256, 256) and EC.ac_blocks(65537) == (256, 257)
    assert EC.ac_blocks(131072) == (256, 512) and EC.ac_blocks(131073) == (256, 512)
    assert -(-131073 // EC.AC_THREADS) == EC.AC_UPDATE_MAX_BLOCKS + 1 and -(-65537 // EC.AC_THREADS) == EC.AC_NORM_MAX_BLOCKS + 1
    assert EC.AC_OVERFLOW_CAPACITY == 4 and EC.AC_OVERFLOW_UPDATES == 6


@pytest.mark.parametrize("n0", list(EC.AC_PRESET_N0))
def test_preset_histories_have_ties_and_the_four_norms_land_where_they_should(n0):
    hist, log = EC.ac_preset_history(n0)
    assert hist.size == log.size == n0 and np.array_equal(np.sort(log), hist) and not np.array_equal(log, hist)
    norms = EC.ac_preset_norms(hist)
    assert list(norms) == list(EC.AC_UPDATES)
    assert all(float(np.float32(v)) == v for v in norms.values())         # a one-element fp32 gradient has exactly this norm
    left = {k: int(np.searchsorted(hist, v, side="left")) for k, v in norms.items()}
    right = {k: int(np.searchsorted(hist, v, side="right")) for k, v in norms.items()}
    assert left["rank_0"] == right["rank_0"] == 0 and left["rank_n0"] == right["rank_n0"] == n0
    assert right["in_ties"] - left["in_ties"] >= 2 and left["in_ties"] > 0
    assert 0 < left["inside"] == right["inside"] < n0
    # the search of the tie and of the inner norm goes through whole gaps: the rounds of ac_search_rounds
    if n0 >= 65535:
        assert n0 // 2 < left["in_ties"] < n0 - 300 and n0 // 5 < left["inside"] < n0 - 300


def test_validation_sum_sizes():
    assert sorted(EC.VAL_B) == [1, 63, 64, 65, 128, 129] and EC.VAL_NAN_B in EC.VAL_B
    for B in EC.VAL_B:
        losses, graphs = R.val_inputs(B)
        assert losses.dtype == np.float32 and graphs.dtype == np.int32 and losses.size == graphs.size == B
        acc, n = R.val_sums(losses, graphs)
        assert n == float(graphs.sum()) and abs(acc - float(np.dot(losses.astype(np.float64), graphs))) <= 1e-12 * acc
    acc, n = R.val_sums(*R.val_inputs(EC.VAL_NAN_B, nan_at=32))
    assert math.isnan(acc) and n == float(R.val_inputs(EC.VAL_NAN_B)[1].sum())


# ---- 3. the references against independent statements -------------------------------------------------------------------------------
def _kernel_order_record(out, y, mask, scale, offset, mutant=None):
    """The moments kernel's own order of operations in numpy float64: every thread adds its elements in index order, the waves
    reduce by the xor butterfly, thread 0 adds the 16 wave partials in wave order; the second pass is centred on the first
    pass's means.  (Masked-out elements add 0.0 here; the kernel skips them.)  ``mutant``: R.MOMENT_MUTANTS."""
    N = len(y)
    m = np.asarray(mask, dtype=bool).copy()
    if mutant == "drops_last_partial_trip":
        m[(N // EC.MET_TRIP) * EC.MET_TRIP:] = False
    p, t = (R.descale32(a, scale, offset, fma=mutant == "fma_descale").astype(np.float64) for a in (out, y))
    p32, t32 = p.astype(np.float32), t.astype(np.float32)
    keep = (np.abs(t32) >= np.float32(0.01)) if mutant == "keep_ge" else (np.abs(t32) > np.float32(0.01))
    acc = np.abs(t32 - p32) <= t32 * np.float32(0.1)

    def block_sum(terms):
        rows = -(-N // EC.MET_T)
        pad = np.zeros(rows * EC.MET_T)
        pad[:N] = np.where(m, terms, 0.0)
        a = np.zeros(EC.MET_T)
        for row in pad.reshape(rows, EC.MET_T):
            a = a + row
        lane = np.arange(EC.MET_T)
        off = EC.GATRES_WAVE // 2
        while off:
            a = a + a[lane ^ off]
            off >>= 1
        s = 0.0
        for w in range(EC.MET_WAVES):
            s = s + a[w * EC.GATRES_WAVE]
        return s

    with np.errstate(all="ignore"):
        ds = np.asarray(out, dtype=np.float64) - np.asarray(y, dtype=np.float64)
        d = p - t
        r = np.zeros(EC.METRICS_RECORD)
        r[0] = block_sum(np.ones(N))
        r[1], r[2], r[3], r[4], r[5] = (block_sum(v) for v in (ds * ds, np.abs(d), d * d, p, t))
        r[9], r[11] = block_sum(keep.astype(np.float64)), block_sum(acc.astype(np.float64))
        r[10] = block_sum(np.where(keep, np.abs(np.abs(t - p) / np.where(keep, t, 1.0)), 0.0))
        pm, tm = r[4] / r[0], r[5] / r[0]
        dp, dt = p - pm, t - tm
        if r[0]:
            r[6], r[7], r[8] = block_sum(dp * dp), block_sum(dt * dt), block_sum(dp * dt)
    return r


@pytest.mark.parametrize("N", list(EC.MOMENT_N))
def test_the_kernels_order_of_summation_lies_within_the_bounds(N):
    """A right answer passes: the kernel's association, restated in numpy, against the exact sums -- at every size, mask and
    scale the GPU module runs.  Also: the record agrees with the older reference of tests/metric_moments_ref.py."""
    out, y = EC.moment_inputs(N)
    worst = 0.0
    for kind in EC.MOMENT_MASKS:
        mask = EC.moment_mask(kind, N)
        for scale, offset in EC.MOMENT_SCALES:
            ref = R.moments(out, y, mask, scale, offset)
            fails, w = R.moment_failures(_kernel_order_record(out, y, mask, scale, offset), ref)
            assert not fails, (N, kind, scale, offset, fails)
            worst = max(worst, w)
            if mask.any():
                old = MR.masked_metric_moments(out, y, mask, scale, offset)
                assert np.array_equal(old[[0, 9, 11]], ref["record"][[0, 9, 11]])
                np.testing.assert_allclose(old, ref["record"], rtol=1e-9, atol=1e-9)
            else:
                assert not ref["record"].any() and not any(ref["bound"].values())
    assert worst <= 1.0
    print(f"N={N}: worst error / bound of the kernel's order on the host {worst:.3f}")


def test_the_centred_sums_do_not_cancel_where_raw_moments_would():
    """(1e-2, 1e4): sum (p - pm)^2 ~ 1e-4 M under p ~ 1e4.  The bound is relative to the centred sum, so a kernel that forms
    sum p^2 - M pm^2 in fp64 (relative 1e-16 of 1e8 M: an absolute 1e-8 M) is far outside it."""
    N = 16385
    out, y = EC.moment_inputs(N)
    mask = EC.moment_mask("all", N)
    ref = R.moments(out, y, mask, 1e-2, 1e4)
    assert ref["bound"][6] < 1e-10 * ref["record"][6] and ref["bound"][8] < 1e-10 * abs(ref["record"][8])
    p = R.descale32(out, 1e-2, 1e4).astype(np.float64)
    raw = ref["record"].copy()
    raw[6] = float(np.sum(p * p)) - N * (float(np.sum(p)) / N) ** 2
    fails, _ = R.moment_failures(raw, ref)
    assert any(f.startswith("field 6") for f in fails), fails


@pytest.mark.parametrize("n0", list(EC.AC_PRESET_N0))
def test_the_restated_lerp_is_numpys_percentile_bit_for_bit(n0):
    hist, _ = EC.ac_preset_history(n0)
    norms = EC.ac_preset_norms(hist)
    differ = 0
    for q in EC.AC_PERCENTILES + [37.5, 50.0, 99.9]:
        a = hist
        for k in EC.AC_UPDATES:
            a = np.sort(np.append(a, norms[k]))
            assert R.percentile_linear(a, q) == float(np.percentile(a, q)), (n0, q, k)
            differ += R.percentile_linear(a, q) != R.percentile_linear(a, q, one_form=True)
    assert differ or n0 == 70000, n0                 # the two expressions of the lerp are told apart on this history


# ---- 4. planted wrong answers -------------------------------------------------------------------------------------------------------
def _designed(which):
    out, y = R.designed_unit() if which == "unit" else R.designed_fma()
    return out, y, np.ones(len(y), dtype=bool), ((1.0, 0.0) if which == "unit" else EC.FMA_SCALE)


def test_designed_inputs_sit_on_the_predicates():
    out, y, mask, (sc, of) = _designed("unit")
    assert np.array_equal(R.descale32(y, sc, of), y) and np.array_equal(R.descale32(out, sc, of), out)       # exact at (1, 0)
    c = np.float32(0.01)
    for v in (c, np.nextafter(c, np.float32(0)), np.nextafter(c, np.float32(1))):
        assert (y == v).any() and (y == -v).any()
    ref = R.moments(out, y, mask, sc, of)["record"]
    assert 0 < ref[11] < (y > 0).sum() and ref[9] == len(y) - 4 - 14       # not kept: +-0.01f, +-its lower neighbour, the rows of t = +-1e-3
    neg = y < 0
    assert R.moments(out[neg], y[neg], mask[neg], sc, of)["record"][11] == 0 and (out[neg] == y[neg]).any()
    # each of the three p around t - fl(0.1f t) decides differently for some t: the boundary is really between them
    pos = R.moments(out[~neg], y[~neg], mask[~neg], sc, of)["record"]
    assert 0.2 * (~neg).sum() < pos[11] < 0.8 * (~neg).sum()
    out, y, mask, (sc, of) = _designed("fma")
    t2, tf = R.descale32(y, sc, of), R.descale32(y, sc, of, fma=True)
    assert (t2 != tf).all() and len(y) == 48


def test_planted_descale_as_one_fma_changes_a_count_on_the_designed_inputs():
    out, y, mask, (sc, of) = _designed("fma")
    ref = R.moments(out, y, mask, sc, of)
    bad = R.moments(out, y, mask, sc, of, mutant="fma_descale")["record"]
    assert ref["record"][11] == len(y) and bad[11] == 0
    fails, _ = R.moment_failures(bad, ref)
    assert any(f.startswith("field 11") for f in fails), fails
    fails, _ = R.moment_failures(_kernel_order_record(out, y, mask, sc, of, mutant="fma_descale"), ref)
    assert any(f.startswith("field 11") for f in fails), fails
    assert R.moment_failures(_kernel_order_record(out, y, mask, sc, of), ref)[0] == []


def test_planted_keep_predicate_with_ge_fails_the_count_on_the_designed_inputs():
    out, y, mask, (sc, of) = _designed("unit")
    ref = R.moments(out, y, mask, sc, of)
    fails, _ = R.moment_failures(_kernel_order_record(out, y, mask, sc, of, mutant="keep_ge"), ref)
    assert any(f.startswith("field 9") for f in fails), fails
    assert R.moment_failures(_kernel_order_record(out, y, mask, sc, of), ref)[0] == []
    # on the random inputs of the size cases nothing sits at 0.01f: they cannot tell the two apart
    o2, y2 = EC.moment_inputs(8193)
    m2 = EC.moment_mask("all", 8193)
    assert R.moment_failures(_kernel_order_record(o2, y2, m2, 12.81, 0.0, mutant="keep_ge"), R.moments(o2, y2, m2, 12.81, 0.0))[0] == []


@pytest.mark.parametrize("N", [1, 1025, 8191, 8193, 16385])
def test_planted_sum_that_drops_the_last_partial_trip_fails(N):
    out, y = EC.moment_inputs(N)
    for kind in ("all", "most", "last"):
        mask = EC.moment_mask(kind, N)
        ref = R.moments(out, y, mask, 12.81, 51.37)
        fails, _ = R.moment_failures(_kernel_order_record(out, y, mask, 12.81, 51.37, mutant="drops_last_partial_trip"), ref)
        assert any(f.startswith("field 0") for f in fails) and any(f.startswith("field 4") for f in fails), (N, kind, fails)


def _snap_buffers(P, s, d, seed):
    r = np.random.RandomState(seed)
    src_padded = r.randn(P + 8).astype(np.float32)
    raw = np.full(EC.SNAP_GUARD + d + P + EC.SNAP_GUARD, EC.SNAP_SENTINEL, dtype=np.float32)
    return src_padded, raw


def test_planted_head_one_float_too_long_breaks_a_guard():
    caught = []
    for (s, d) in EC.SNAP_SHIFTS:
        for P in [p for p in EC.SNAP_P if p < 5000]:
            src_padded, raw = _snap_buffers(P, s, d, P)
            right = R.snapshot_emulate(raw, src_padded, s, d, P)
            assert R.snapshot_failures(right, raw, src_padded[:P], d, True) == [], (s, d, P)
            assert R.snapshot_failures(raw, raw, src_padded[:P], d, False) == []
            wrong = R.snapshot_emulate(raw, src_padded, s, d, P, mutant="head_one_too_long")
            if R.snapshot_failures(wrong, raw, src_padded[:P], d, True):
                caught.append(((s, d), P))
    # seen exactly where the count does not reach past the head: the extra float lands on the guard behind the array
    assert caught == [((s, d), P) for (s, d) in EC.SNAP_SHIFTS for P in sorted(EC.SNAP_P)
                      if P < 5000 and 0 < EC.snapshot_geometry(P, s, d)["head"] == P], caught
    assert ((1, 1), 1) in caught and ((1, 1), 3) in caught and ((3, 3), 1) in caught
    # and a copy that was not made, or one float short, is seen
    src_padded, raw = _snap_buffers(7, 1, 1, 3)
    short = R.snapshot_emulate(raw, src_padded, 1, 1, 6)
    assert R.snapshot_failures(short, raw, src_padded[:7], 1, True) and R.snapshot_failures(raw, raw, src_padded[:7], 1, True)


def _updates(n0, percentile, mutant=None):
    """The four updates of a preset case on the host: [(failures of the GPU module's comparison, rank, tie)]."""
    hist, log = EC.ac_preset_history(n0)
    out = []
    for k, n in EC.ac_preset_norms(hist).items():
        nxt, c, coef = R.autoclip_emulate(hist, n, percentile, mutant=mutant)
        log = np.append(log, n)
        out.append((k, R.autoclip_failures(nxt, log, (n, c, coef), percentile, n)))
        hist = np.sort(log)
    return out


@pytest.mark.parametrize("n0", [255, 65537, 70000])
def test_planted_rank_off_by_one_among_ties_fails_the_sorted_buffer(n0):
    for q in EC.AC_PERCENTILES:
        assert all(f == [] for _, f in _updates(n0, q)), (n0, q)
        bad = dict(_updates(n0, q, mutant="rank_before_a_tie"))
        assert any("np.sort" in f for f in bad["in_ties"]), bad
        assert bad["rank_0"] == [] and bad["rank_n0"] == []             # only a norm that ties an entry shows it


def test_planted_percentile_without_numpys_second_form_fails_the_clip_bits():
    seen = 0
    for n0 in EC.AC_PRESET_N0:
        assert all(f == [] for _, f in _updates(n0, 10.0))
        bad = _updates(n0, 10.0, mutant="lerp_one_form")
        assert all(all("lerp" in line for line in f) for _, f in bad)          # nothing but the bits of the clip value
        seen += sum(bool(f) for _, f in bad)
        for q in (0.0, 100.0):                                                   # g = 0: the two forms are the same expression
            assert all(f == [] for _, f in _updates(n0, q, mutant="lerp_one_form"))
    assert seen >= 3, seen
