"""The kernels that run once per epoch or once per update, beside the training step, where their loops, lanes and capped grids
turn over: the masked-metric moments (csrc/k_metrics.hip), the checkpoint copy and the validation sums (csrc/k_epoch.hip) and
AutoClip's update (csrc/k_autoclip.hip), each through the C ABI on buffers this module owns.

tests/epoch_kernel_cases.py says which sizes and why, tests/epoch_kernel_refs.py states the references, the bounds and the
comparisons (its ``*_failures`` functions; tests/test_epoch_kernels_host.py shows on the host what they reject):

  * moments: counts EQUAL to numpy float32's, every plain sum within (n - 1) 2^-53 sum |term| of the exact sum, the centred sums
    within the bound derived in epoch_kernel_refs.moments -- no margin anywhere; the worst error / bound per case is printed and
    noted into the parity report (profiles/epoch_kernels_margins.txt holds the measured table); designed inputs on the two
    fp32 predicates; the record bit for bit under shifted pointers, NaN in everything it must not read, cursor against slot;
  * snapshot: every destination bit-equal to its source and every guard float intact for equal and unequal misalignment of
    source and destination, counts below the head, around a workgroup trip and behind the grid cap; the flag as +0.0 / -0.0 / 1.0;
  * AutoClip: the live sorted buffer is np.sort(log) bit for bit over preset histories that need no, one and two rounds of the
    256-way search, norms at rank 0, rank n0, inside ties and strictly inside; parameters and moments at the block caps against
    tests/adam_ref.py element by element; the overflow branch;
  * validation sums in their ``losses`` form against the sequential loop, bit for bit."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import adam_ref as A
import epoch_kernel_cases as EC
import epoch_kernel_refs as R
from test_gpu_model import note

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGINS = {}
G = EC.GUARD_RECORDS
REC = EC.METRICS_RECORD


@pytest.fixture(scope="module", autouse=True)
def _note_margins():
    """One entry of the parity report for the module: the worst error / bound of every case, by name."""
    yield
    if MARGINS:
        note("epoch kernels: worst error / bound per moment case and per update of AutoClip's Adam at the block caps", dict(MARGINS))


# ---- 1. moments ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _inputs(N):
    return EC.moment_inputs(N)


def _table(capacity):
    """A garbage-filled table of ``capacity`` records with G guard records on either side: (whole buffer, pointer to record 0)."""
    raw = torch.full(((capacity + 2 * G) * REC,), EC.SENTINEL_F64, dtype=torch.float64, device=DEV)
    return raw, raw[G * REC:].data_ptr()


def _records(raw):
    return raw.cpu().numpy().reshape(-1, REC)


def _untouched(rows):
    return bool((rows.view(np.uint64) == np.float64(EC.SENTINEL_F64).view(np.uint64)).all())


def _metrics(pkg, lib, out, y, mask, N, scale, offset, table_ptr, slot, capacity, cursor=None):
    pkg._native.check(lib.gatres_masked_metrics(out.data_ptr(), y.data_ptr(), mask.data_ptr(), N, scale, offset, table_ptr, slot,
                                                capacity, pkg._native.ptr(cursor), pkg._native.current_stream(out.device)),
                      "gatres_masked_metrics")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize("scale,offset", EC.MOMENT_SCALES)
@pytest.mark.parametrize("N", list(EC.MOMENT_N))
def test_moments_against_exact_sums_at_every_turnover(pkg, lib, N, scale, offset):
    out, y = _inputs(N)
    d_out, d_y = _dev(out), _dev(y)
    kinds = list(EC.MOMENT_MASKS)
    raw, tp = _table(len(kinds))
    for slot, kind in enumerate(kinds):
        _metrics(pkg, lib, d_out, d_y, _dev(EC.moment_mask(kind, N).astype(np.uint8)), N, scale, offset, tp, slot, len(kinds))
    T = _records(raw)
    assert _untouched(T[:G]) and _untouched(T[G + len(kinds):]), "a guard record changed"
    bad = []
    for slot, kind in enumerate(kinds):
        mask = EC.moment_mask(kind, N)
        ref = R.moments(out, y, mask, scale, offset)
        fails, worst = R.moment_failures(T[G + slot], ref)
        name = f"moments N={N} scale={scale:g} offset={offset:g} mask={kind}"
        MARGINS[name] = worst
        print(f"{name}: M={int(ref['record'][0])} worst error / bound {worst:.4f}")
        bad += [f"{kind}: {f}" for f in fails]
        if not mask.any():
            rec = T[G + slot]
            assert not rec.any() and not np.signbit(rec).any(), f"{kind}: an empty mask leaves {rec!r}"
            loss, met = pkg.evaluation.metrics_from_moments(rec[None], [3])
            empty = torch.empty(0)
            # (of the reference's seven functions only its NSE has a value on empty tensors: 1 - 0 / (0 + 1e-12))
            assert math.isnan(loss) and met.pop("test_mynse") == float(pkg.evaluation.calculate_nse(empty, empty)) == 1.0
            assert len(met) == 6 and all(math.isnan(v) for v in met.values()), met
    assert not bad, bad


@pytest.mark.parametrize("which", ["unit", "fma"])
def test_moments_counts_on_inputs_designed_to_sit_on_the_predicates(pkg, lib, which):
    """|t| at float32(0.01) and its neighbours, p one ulp to either side of t -+ fl(0.1f t), negative t (scale 1, offset 0: exact
    descaling); and (12.81, 51.37) targets whose product needs rounding before the add, paired with predictions for which an
    fma-descaled kernel decides the accuracy predicate the other way (tests/test_epoch_kernels_host.py: all 48 of them)."""
    out, y = R.designed_unit() if which == "unit" else R.designed_fma()
    scale, offset = (1.0, 0.0) if which == "unit" else EC.FMA_SCALE
    N = len(y)
    mask = np.ones(N, dtype=bool)
    raw, tp = _table(1)
    _metrics(pkg, lib, _dev(out), _dev(y), _dev(mask.astype(np.uint8)), N, scale, offset, tp, 0, 1)
    T = _records(raw)
    ref = R.moments(out, y, mask, scale, offset)
    fails, worst = R.moment_failures(T[G], ref)
    MARGINS[f"moments designed {which} N={N}"] = worst
    print(f"designed {which}: counts {T[G][[0, 9, 11]]}, reference {ref['record'][[0, 9, 11]]}, worst error / bound {worst:.4f}")
    assert not fails, fails
    assert _untouched(T[:G]) and _untouched(T[G + 1:])


@pytest.mark.parametrize("N", [65, 1025, 8193, 16385])
def test_moments_record_keeps_its_bits(pkg, lib, N):
    """The same record, bit for bit: from pointers one element further into their allocations; with NaN behind element N - 1
    and under every masked-out entry (mask bytes behind N - 1 set); through the cursor as through ``slot``.  A cursor at or past
    ``capacity`` writes nothing and still advances.  No launch touches another slot."""
    scale, offset = 12.81, 51.37
    out, y = _inputs(N)
    mask = EC.moment_mask("most", N)
    cap = 4
    raw, tp = _table(cap)
    _metrics(pkg, lib, _dev(out), _dev(y), _dev(mask.astype(np.uint8)), N, scale, offset, tp, 1, cap)
    base = _records(raw)[G + 1].copy()
    assert R.moment_failures(base, R.moments(out, y, mask, scale, offset))[0] == []

    def only(raw, slot):
        T = _records(raw)
        others = np.delete(T, G + slot, axis=0) if slot is not None else T
        assert _untouched(others), "a launch wrote outside its slot"
        return T[G + slot] if slot is not None else None

    # (a) every pointer one element on: out / y 4 bytes, the mask 1 byte off their allocations' alignment
    pad = 64
    s_out, s_y = (_dev(np.concatenate([[np.nan], a, np.full(pad, np.nan)]).astype(np.float32)) for a in (out, y))
    s_m = _dev(np.concatenate([[1], mask.astype(np.uint8), np.ones(pad, dtype=np.uint8)]).astype(np.uint8))
    raw, tp = _table(cap)
    _metrics(pkg, lib, s_out[1:], s_y[1:], s_m[1:], N, scale, offset, tp, 2, cap)
    assert s_out[1:].data_ptr() % 16 == 4 and s_m[1:].data_ptr() % 16 == 1
    assert only(raw, 2).tobytes() == base.tobytes(), "shifted pointers change the record"
    # (b) NaN wherever the kernel must not look
    n_out, n_y = out.copy(), y.copy()
    n_out[~mask] = np.nan
    n_y[~mask] = np.nan
    n_out, n_y = (_dev(np.concatenate([a, np.full(pad, np.nan)]).astype(np.float32)) for a in (n_out, n_y))
    n_m = _dev(np.concatenate([mask.astype(np.uint8), np.ones(pad, dtype=np.uint8)]))
    raw, tp = _table(cap)
    _metrics(pkg, lib, n_out, n_y, n_m, N, scale, offset, tp, 0, cap)
    assert only(raw, 0).tobytes() == base.tobytes(), "values outside the mask or behind N - 1 reach the record"
    # (c) the cursor: slot + cursor[0] names the record, the cursor advances by one
    d_out, d_y, d_m = _dev(out), _dev(y), _dev(mask.astype(np.uint8))
    raw, tp = _table(cap)
    cursor = torch.tensor([3, -9], dtype=torch.int64, device=DEV)
    _metrics(pkg, lib, d_out, d_y, d_m, N, scale, offset, tp, 0, cap, cursor)
    assert only(raw, 3).tobytes() == base.tobytes() and cursor.tolist() == [4, -9]
    # (d) at and past the capacity: nothing written, still advanced
    _metrics(pkg, lib, d_out, d_y, d_m, N, scale, offset, tp, 0, cap, cursor)
    cursor[0] = cap + 5
    _metrics(pkg, lib, d_out, d_y, d_m, N, scale, offset, tp, 0, cap, cursor)
    assert only(raw, 3).tobytes() == base.tobytes() and cursor.tolist() == [cap + 6, -9]
    raw, tp = _table(cap)
    cursor = torch.tensor([cap, -9], dtype=torch.int64, device=DEV)
    _metrics(pkg, lib, d_out, d_y, d_m, N, scale, offset, tp, 0, cap, cursor)
    only(raw, None)
    assert cursor.tolist() == [cap + 1, -9]


# ---- 2. snapshot --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def snap_pool():
    """Three sources of different contents and three destinations, sized for the largest count and shift (about 200 MB)."""
    P = max(EC.SNAP_P)
    g = torch.Generator(device=DEV).manual_seed(5)
    src = [torch.randn(P + 8, device=DEV, generator=g) * (10.0 ** k) for k in (0, -3, 3)]
    dst = [torch.empty(2 * EC.SNAP_GUARD + 3 + P, device=DEV) for _ in range(3)]
    assert all(t.data_ptr() % 16 == 0 for t in src + dst)
    yield src, dst
    del src, dst
    torch.cuda.empty_cache()


@pytest.mark.parametrize("P", list(EC.SNAP_P))
@pytest.mark.parametrize("shifts", list(EC.SNAP_SHIFTS), ids=lambda s: f"src{s[0]}-dst{s[1]}")
def test_snapshot_copies_bit_for_bit_at_every_alignment_and_size(lib, snap_pool, shifts, P):
    s, d = shifts
    geo = EC.snapshot_geometry(P, s, d)
    src_raw, dst_raw = snap_pool
    lo = EC.SNAP_GUARD + d
    raw = [t[:lo + P + EC.SNAP_GUARD] for t in dst_raw]
    for r in raw:
        r.fill_(EC.SNAP_SENTINEL)
    src = [t[s:s + P] for t in src_raw]
    dst = [r[lo:lo + P] for r in raw]
    assert all(t.data_ptr() % 16 == 4 * s for t in src) and all(t.data_ptr() % 16 == 4 * d for t in dst)
    step = torch.tensor([41, 7], dtype=torch.int64, device=DEV)
    dstep = torch.tensor([-1, -2, -3], dtype=torch.int64, device=DEV)
    flag = torch.zeros(1, dtype=torch.float64, device=DEV)

    def call():
        assert lib.gatres_snapshot_if(flag.data_ptr(), src[0].data_ptr(), src[1].data_ptr(), src[2].data_ptr(), step.data_ptr(),
                                      dst[0].data_ptr(), dst[1].data_ptr(), dst[2].data_ptr(), dstep[1:].data_ptr(), P, None) == 0
        torch.cuda.synchronize()

    for f in (0.0, -0.0):                                   # not set: no float and no step word moves
        flag.fill_(f)
        call()
        assert all(bool((r == EC.SNAP_SENTINEL).all()) for r in raw) and dstep.tolist() == [-1, -2, -3], (f, geo)
    before = [np.full(r.numel(), EC.SNAP_SENTINEL, dtype=np.float32) for r in raw]
    flag.fill_(1.0)
    call()
    assert dstep.tolist() == [-1, 41, -3] and step.tolist() == [41, 7]
    for k in range(3):
        fails = R.snapshot_failures(raw[k].cpu().numpy(), before[k], src[k].cpu().numpy(), d, True)
        assert not fails, (k, geo, fails)


# ---- 3. AutoClip --------------------------------------------------------------------------------------------------------------------
CFG = (5e-4, 0.9, 0.999, 1e-8, 6e-6, 1.0)
GARBAGE = -3.0e300


def _ac_state(percentile, P, capacity):
    from gnn_pressure_estimation_amd import train_step as TS
    return TS._AutoClipState(percentile, P, torch.device(DEV), capacity)


def _ac_step(pkg, st, d, step, P, cfg=CFG):
    lr, b1, b2, eps, wd, scale = cfg
    N_ = pkg._native
    N_.check(N_.load().gatres_autoclip_adam_step(d["p"].data_ptr(), d["g"].data_ptr(), d["m"].data_ptr(), d["v"].data_ptr(),
                                                 step.data_ptr(), P, lr, b1, b2, eps, wd, scale, C.byref(st.c),
                                                 N_.current_stream(d["p"].device)), "gatres_autoclip_adam_step")
    torch.cuda.synchronize()


def _live(st, cnt):
    return (st.sorted1 if cnt & 1 else st.sorted0), (st.sorted0 if cnt & 1 else st.sorted1)


@pytest.mark.parametrize("percentile", EC.AC_PERCENTILES)
@pytest.mark.parametrize("n0", list(EC.AC_PRESET_N0))
def test_autoclip_update_on_a_preset_history(pkg, n0, percentile):
    """A sorted history of n0 entries with runs of exact ties is written into the buffer the count's parity selects, the log
    and the count beside it; four updates then land at rank 0, rank n0, inside a run of ties and strictly inside.  Every norm
    is an fp32 value carried by one gradient element, so the fp64 norm is that value exactly."""
    P = EC.AC_P
    hist, log = EC.ac_preset_history(n0)
    norms = EC.ac_preset_norms(hist)
    cap = n0 + 8
    st = _ac_state(percentile, P, cap)
    for t in (st.sorted0, st.sorted1, st.log):
        t.fill_(GARBAGE)
    _live(st, n0)[0][:n0] = _dev(hist)
    st.log[:n0] = _dev(log)
    st.ctl[EC.AC_COUNT] = n0
    g = torch.Generator().manual_seed(n0)
    d = {k: (torch.randn(P, generator=g) * 0.1).to(DEV) for k in "pm"}
    d["v"] = (torch.rand(P, generator=g) * 1e-3).to(DEV)
    d["g"] = torch.zeros(P, device=DEV)
    step = torch.tensor([10, 77], dtype=torch.int64, device=DEV)
    host_log = list(log)
    for j, kind in enumerate(EC.AC_UPDATES):
        n = norms[kind]
        cnt = n0 + j + 1
        assert len(EC.ac_search_rounds(cnt - 1)) == (0 if cnt - 1 <= 256 else 2 if cnt - 1 > 65792 else 1)
        d["g"].zero_()
        d["g"][(997 * (j + 1)) % P] = -n if j % 2 else n
        p_before = d["p"].clone()
        _ac_step(pkg, st, d, step, P)
        host_log.append(n)
        ctl = st.ctl.tolist()
        assert ctl[EC.AC_COUNT] == cnt and ctl[EC.AC_OVERFLOW] == 0 and step.tolist() == [11 + j, 77], (kind, ctl)
        live, other = _live(st, cnt)
        live, dlog = live.cpu().numpy(), st.log.cpu().numpy()
        fails = R.autoclip_failures(live[:cnt], dlog[:cnt], st.out.tolist(), percentile, n)
        assert not fails, (n0, percentile, kind, fails)
        assert np.array_equal(dlog[:cnt], np.array(host_log))                                   # the log before it: untouched
        assert (live[cnt:] == GARBAGE).all() and (dlog[cnt:] == GARBAGE).all(), "written behind the count"
        assert np.array_equal(other.cpu().numpy()[:cnt - 1], np.sort(np.array(host_log[:-1]))) # the copy it read: untouched
        assert not torch.equal(d["p"], p_before)                                                # and Adam ran


def _guarded(arr):
    buf = torch.empty(len(arr) + A.GUARD, dtype=torch.float32, device=DEV)
    buf[:len(arr)] = torch.from_numpy(np.ascontiguousarray(arr))
    buf[len(arr):] = 1234.25
    return buf


@pytest.mark.parametrize("P", list(EC.AC_CAP_P))
def test_autoclip_adam_at_the_block_caps_element_by_element(pkg, P):
    """256 norm workgroups and 512 update workgroups exactly, and one element more (block 0 makes a second trip): parameters and
    both moments against tests/adam_ref.py on the clipped gradient at that module's bounds, the norm against fp64, clip value
    and coefficient against numpy.  Three updates, gradients of 1, 4 and 2 times a vector: coefficients ~1, 0.325, 0.6."""
    cfg = A.CONFIGS[A.SIZE_CONFIG]
    scale = cfg[5]
    x = A.make_inputs(P, cfg, nonfinite=False)
    st = _ac_state(10.0, P, 8)
    assert st.partials.numel() >= EC.ac_blocks(P)[0]
    bufs = {k: _guarded(x[k]) for k in "pgmv"}
    d = {k: b[:P] for k, b in bufs.items()}
    step = torch.tensor([0, 5], dtype=torch.int64, device=DEV)
    norms = []
    for j, factor in enumerate((1.0, 4.0, 2.0)[:EC.AC_CAP_UPDATES]):
        gj = (x["g"] * np.float32(factor)).astype(np.float32)               # (powers of two: the norms are 1 : 4 : 2 exactly)
        state = {k: d[k].cpu().numpy() for k in "pmv"}
        d["g"].copy_(torch.from_numpy(gj))
        _ac_step(pkg, st, d, step, P, cfg)
        norm, clip, coef = st.out.tolist()
        n_ref = math.sqrt(math.fsum(((gj * np.float32(scale)).astype(np.float64) ** 2).tolist()))
        norms.append(n_ref)
        c_ref = float(np.percentile(np.array(norms), 10.0))
        assert R.rel(norm, n_ref) < 1e-12 and R.rel(clip, c_ref) < 1e-12 and R.rel(coef, min(1.0, c_ref / (n_ref + 1e-6))) < 1e-12
        assert step.tolist() == [j + 1, 5] and st.ctl.tolist()[EC.AC_COUNT] == j + 1
        inputs = dict(state, g=gj, special=x["special"], regular=x["regular"])
        got = [d[k].cpu().numpy() for k in "pmv"]
        ratios, wrong = A.check_against_reference(got, inputs, j + 1, cfg, coef)
        print(f"autoclip at P={P}, update {j + 1}: coef {coef:.4f}, worst ratio to the bound p {ratios[0]:.3f} "
              f"exp_avg {ratios[1]:.3f} exp_avg_sq {ratios[2]:.3f}")
        MARGINS[f"autoclip adam P={P} update {j + 1}: p, exp_avg, exp_avg_sq"] = max(ratios)
        assert all(r <= 1.0 for r in ratios), ratios
        assert not wrong, wrong
        for k, b in bufs.items():
            assert bool((b[P:] == 1234.25).all()), f"the launch wrote behind {k}"
        assert np.array_equal(d["g"].cpu().numpy().view(np.uint32), gj.view(np.uint32))
    assert st.out.tolist()[2] < 0.7 and np.array_equal(st.log[:3].cpu().numpy(), _live(st, 3)[0][:3].cpu().numpy()[[0, 2, 1]])


def test_autoclip_overflow_skips_the_step_and_sets_the_flag(pkg):
    """Capacity 4 and nobody grows it: updates 5 and 6 find the history full."""
    P = EC.AC_P
    st = _ac_state(10.0, P, EC.AC_OVERFLOW_CAPACITY)
    g = torch.Generator().manual_seed(9)
    d = {k: (torch.randn(P, generator=g) * 0.1).to(DEV) for k in "pm"}
    d["v"] = (torch.rand(P, generator=g) * 1e-3).to(DEV)
    step = torch.tensor([0, 3], dtype=torch.int64, device=DEV)
    kept = None
    for j in range(EC.AC_OVERFLOW_UPDATES):
        d["g"] = torch.randn(P, generator=g).to(DEV) * (j + 1.0)
        _ac_step(pkg, st, d, step, P)
        everything = [d["p"], d["m"], d["v"], step, st.log, st.sorted0, st.sorted1, st.out]
        ctl = st.ctl.tolist()
        if j < EC.AC_OVERFLOW_CAPACITY:
            assert ctl[EC.AC_COUNT] == j + 1 and ctl[EC.AC_OVERFLOW] == 0 and step.tolist() == [j + 1, 3]
            kept = [t.clone() for t in everything]
        else:
            assert ctl[EC.AC_COUNT] == EC.AC_OVERFLOW_CAPACITY and ctl[EC.AC_OVERFLOW] == 1
            for name, a, b in zip(("p", "exp_avg", "exp_avg_sq", "step", "log", "sorted0", "sorted1", "out"), everything, kept):
                assert torch.equal(a.view(torch.int64) if a.dtype != torch.float32 else a.view(torch.int32),
                                   b.view(torch.int64) if b.dtype != torch.float32 else b.view(torch.int32)), (j + 1, name)
    assert np.array_equal(_live(st, 4)[0].cpu().numpy(), np.sort(st.log.cpu().numpy()))


# ---- 4. validation sums -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,nan_at", [(B, None) for B in EC.VAL_B] + [(EC.VAL_NAN_B, 32)])
def test_val_sums_of_losses_are_the_sequential_loop(lib, B, nan_at):
    losses, graphs = R.val_inputs(B, nan_at)
    pad = np.full(64, np.nan, dtype=np.float32)                       # behind batch B - 1: NaN losses with huge graph counts
    d_l = _dev(np.concatenate([losses, pad]))
    d_g = _dev(np.concatenate([graphs, np.full(64, 1 << 20, dtype=np.int32)]))
    out = torch.full((4,), EC.SENTINEL_F64, dtype=torch.float64, device=DEV)
    assert lib.gatres_epoch_val_sums(None, d_l.data_ptr(), d_g.data_ptr(), B, out[1:].data_ptr(), None) == 0
    torch.cuda.synchronize()
    acc, n = R.val_sums(losses, graphs)
    got = out.tolist()
    assert got[0] == got[3] == EC.SENTINEL_F64 and got[2] == n
    if nan_at is None:
        assert got[1] == acc and math.isfinite(acc), (got, acc)
    else:
        assert math.isnan(got[1]) and math.isnan(acc)
