"""The four kernels that each write out the Adam update -- adam_kernel (k_misc.hip), autoclip_adam_kernel (k_autoclip.hip),
reduce_adam_kernel and param_grads_finish_kernel<16 / 32> (k_fused_host.hip) -- held element by element to the float64
statement of tests/adam_ref.py (bounds derived from fp32 rounding, not from kernel output; test_adam_ref_host.py anchors
the statement to torch.optim.Adam and shows what the bounds reject) and, bit for bit, to one another: every other kernel's
p, exp_avg and exp_avg_sq must be the bytes ``gatres_adam_step`` leaves from the same state and gradient.  That identity
rests on the kernels stating the same operations and on the build's -ffp-contract=off, not on a host rounding model.

Hyper-parameters: the four tuples of adam_ref.CONFIGS (weight decay from 0 to 0.3, eps from 1e-15 to 1e-3, beta1 = 0,
beta2 = 1 - 1e-7, grad_scale from 1/64 to 3) at t from 1 to 2^33 + 1, reached by writing t - 1 into the step count."""
import ctypes as C

import numpy as np
import pytest
import torch

import adam_ref as A
from test_gpu_model import build, note

pytestmark = pytest.mark.gpu
GRID = [(ci, t) for ci in range(len(A.CONFIGS)) for t in A.STEPS]
PERCENTILE = 10.0
WORST = {}


@pytest.fixture(scope="module")
def ops():
    from tests import hipops
    return hipops


def _record(kernel, ratios):
    """The worst ratio to each bound seen so far for this kernel, into parity_report.json."""
    w = WORST.setdefault(kernel, [0.0, 0.0, 0.0])
    WORST[kernel] = [max(a, float(b)) for a, b in zip(w, ratios)]
    note(f"adam element-wise, {kernel}: worst |kernel - fp64| / bound for p, exp_avg, exp_avg_sq", WORST[kernel])


def _guard_pattern():
    return (torch.arange(A.GUARD, dtype=torch.float32) * 0.5 + 1234.25).cuda()


def _guarded(arr):
    """arr on the device with GUARD floats behind it; returns (whole buffer, view of arr's elements)."""
    n = len(arr)
    buf = torch.empty(n + A.GUARD, dtype=torch.float32, device="cuda")
    buf[:n] = torch.from_numpy(np.ascontiguousarray(arr))
    buf[n:] = _guard_pattern()
    return buf, buf[:n]


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same_bytes(a, b):
    return torch.equal(_bits(a), _bits(b))


def _state_on_device(x):
    bufs = {k: _guarded(x[k]) for k in "pgmv"}
    return bufs, {k: v[1] for k, v in bufs.items()}


def _assert_guards(bufs, inputs, n):
    for k, (whole, _) in bufs.items():
        assert torch.equal(whole[n:], _guard_pattern()), f"the launch wrote behind {k}"
    assert _same_bytes(bufs["g"][1], torch.from_numpy(inputs["g"]).cuda()), "the launch wrote to the gradient"


def _judge(kernel, got, inputs, t, cfg, coef=1.0):
    """got: device tensors p, m, v after the launch.  Every regular element within its bound, every special one of the class
    adam_step_fp32 gives; the ratios are printed and recorded before anything is asserted."""
    got = [a.detach().cpu().numpy() for a in got]
    ratios, wrong = A.check_against_reference(got, inputs, t, cfg, coef)
    print(f"{kernel} n={len(inputs['p'])} config={cfg} t={t} coef={coef!r}: worst ratio to the bound p {ratios[0]:.3f} "
          f"exp_avg {ratios[1]:.3f} exp_avg_sq {ratios[2]:.3f}")
    _record(kernel, ratios)
    assert all(r <= 1.0 for r in ratios), (kernel, ratios, _worst_element(got, inputs, t, cfg, coef))
    assert not wrong, wrong


def _worst_element(got, inputs, t, cfg, coef):
    """Index, kind and values of the element furthest outside its bound (for the failure message)."""
    lr, b1, b2, eps, wd, scale = cfg
    ref = A.adam_step_fp64(inputs["p"], inputs["g"], inputs["m"], inputs["v"], t, lr, b1, b2, eps, wd, scale, coef)
    out = []
    for what, a, r, e in zip("pmv", got, ref[:3], ref[3]):
        with np.errstate(all="ignore"):
            ratio = np.where(inputs["regular"], np.abs(a.astype(np.float64) - r) / e, 0.0)
        ratio[~np.isfinite(ratio)] = np.inf
        i = int(np.argmax(ratio))
        out.append((what, i, A.KINDS[i % 8], float(ratio[i]), float(a[i]), float(r[i]),
                    {k: float(inputs[k][i]) for k in "pgmv"}))
    return out


def _cases():
    return [pytest.param(A.N_GRID, ci, t, id=f"cfg{ci}-t{t}") for ci, t in GRID] + \
           [pytest.param(n, A.SIZE_CONFIG, A.SIZE_T, id=f"n{n}") for n in A.SIZES if n != A.N_GRID]


# ------------------------------------------------------------------------------------------------- (a) gatres_adam_step
@pytest.mark.parametrize("n,ci,t", _cases())
def test_adam_step_element_by_element(ops, n, ci, t):
    cfg = A.CONFIGS[ci]
    lr, b1, b2, eps, wd, scale = cfg
    x = A.make_inputs(n, cfg)
    bufs, d = _state_on_device(x)
    step = torch.tensor([t - 1, 0], dtype=torch.int64, device="cuda")
    ops.adam_step(d["p"], d["g"], d["m"], d["v"], step, lr, b1, b2, eps, wd, scale)
    torch.cuda.synchronize()
    assert step.tolist() == [t, 0]
    _assert_guards(bufs, x, n)
    _judge("adam_kernel", (d["p"], d["m"], d["v"]), x, t, cfg)


# ---------------------------------------------------------------------------------------- (b) gatres_autoclip_adam_step
def _autoclip_launch(pkg, st, d, step, n, cfg):
    lr, b1, b2, eps, wd, scale = cfg
    N_ = pkg._native
    st.reserve(1)
    N_.check(N_.load().gatres_autoclip_adam_step(d["p"].data_ptr(), d["g"].data_ptr(), d["m"].data_ptr(), d["v"].data_ptr(),
                                                 step.data_ptr(), n, lr, b1, b2, eps, wd, scale, C.byref(st.c),
                                                 N_.current_stream(d["p"].device)), "gatres_autoclip_adam_step")


@pytest.mark.parametrize("n,ci,t", _cases())
def test_autoclip_adam_step_element_by_element_and_bitwise_equal_to_adam_step(pkg, ops, n, ci, t):
    """Two launches: the first, on a quarter of the gradient and a state of its own, puts a norm n/4 into the history; the
    second is the case -- clipped to the 10th percentile of {n/4, n}, a coefficient of about 0.325 (less where the 1e-6 of
    the rule counts).  The vector leaves the +-inf / NaN gradients out: with them the norm is not finite and the
    coefficient NaN, never below 1; the full vector runs in the test after this one.  The cancelling block is built for the coefficient the rule predicts; the reference takes the one the
    launch reports."""
    from gnn_pressure_estimation_amd import train_step as TS
    cfg = A.CONFIGS[ci]
    lr, b1, b2, eps, wd, scale = cfg
    x = A.make_inputs(n, cfg, nonfinite=False)
    coef_pred = A.predicted_clip_coef(x["g"] * np.float32(0.25), x["g"], scale, PERCENTILE)
    x = A.make_inputs(n, cfg, coef=coef_pred, nonfinite=False)
    st = TS._AutoClipState(PERCENTILE, n, torch.device("cuda", 0), 8)
    first = dict(x, g=x["g"] * np.float32(0.25))
    _, d1 = _state_on_device(first)
    _autoclip_launch(pkg, st, d1, torch.tensor([t - 1, 0], dtype=torch.int64, device="cuda"), n, cfg)
    bufs, d = _state_on_device(x)
    before = {k: d[k].clone() for k in "pmv"}
    step = torch.tensor([t - 1, 0], dtype=torch.int64, device="cuda")
    _autoclip_launch(pkg, st, d, step, n, cfg)
    torch.cuda.synchronize()
    coef = float(st.out[2])
    assert step.tolist() == [t, 0] and int(st.ctl[0]) == 2
    assert 0.0 < coef < 0.5 and abs(coef / coef_pred - 1.0) < 1e-6, (coef, coef_pred)
    _assert_guards(bufs, x, n)
    # device to device: plain Adam on g' = (g * scale) * float32(coef), formed in torch fp32, scale 1
    g2 = (d["g"] * torch.tensor(scale, dtype=torch.float32, device="cuda")) * torch.tensor(coef, dtype=torch.float32, device="cuda")
    step2 = torch.tensor([t - 1, 0], dtype=torch.int64, device="cuda")
    ops.adam_step(before["p"], g2, before["m"], before["v"], step2, lr, b1, b2, eps, wd, 1.0)
    torch.cuda.synchronize()
    for k in "pmv":
        assert _same_bytes(d[k], before[k]), (k, int((_bits(d[k]) != _bits(before[k])).sum()))
    _judge("autoclip_adam_kernel", (d["p"], d["m"], d["v"]), x, t, cfg, coef)


def _same_bytes_or_both_nan(a, b):
    """Bit for bit, except that a NaN may be any NaN (its sign and payload are not part of the arithmetic)."""
    return bool(((_bits(a) == _bits(b)) | (torch.isnan(a) & torch.isnan(b))).all())


@pytest.mark.parametrize("norm_kind", ["nan", "inf"])
@pytest.mark.parametrize("ci", range(len(A.CONFIGS)))
def test_autoclip_adam_step_on_the_full_vector_with_nonfinite_gradients(pkg, ops, ci, norm_kind):
    """The vector of (a) with all nine special elements through ONE gatres_autoclip_adam_step launch.  Its +-inf / NaN
    gradients make the norm NaN ("nan"; "inf": the NaN gradient replaced by 1, the norm is +inf).  The reference's rule is
    np.percentile over the history followed by torch.nn.utils.clip_grad_norm_, whose clamp(max=1) lets the NaN quotient
    c / (n + 1e-6) through: every gradient entry, and so every element of p, exp_avg and exp_avg_sq, becomes NaN
    (test_adam_ref_host.py shows torch doing it).  Observed on the device with the kernel as it was before this test: clip
    value NaN, coefficient 1.0 in all eight cases -- fmin(1, NaN) = 1 -- so the finite elements got an ordinary unclipped
    update; the kernel now lets the NaN through as clamp does.  Checked: the three outputs, every
    element's class against adam_step_fp32 at the coefficient the launch reports -- the nine specials among them -- the
    bounds on the regular elements should a coefficient ever be finite, and the identity with gatres_adam_step on
    g' = (g * scale) * float32(coef)."""
    from gnn_pressure_estimation_amd import train_step as TS
    import math
    cfg = A.CONFIGS[ci]
    lr, b1, b2, eps, wd, scale = cfg
    t, n = A.STEPS[ci + 1], A.N_GRID
    x = A.make_inputs(n, cfg)
    assert len(x["special"]) == len(A.SPECIALS)
    if norm_kind == "inf":
        x["g"][dict((name, i) for i, name in x["special"])["g_nan"]] = 1.0
    st = TS._AutoClipState(PERCENTILE, n, torch.device("cuda", 0), 8)
    bufs, d = _state_on_device(x)
    before = {k: d[k].clone() for k in "pmv"}
    step = torch.tensor([t - 1, 0], dtype=torch.int64, device="cuda")
    _autoclip_launch(pkg, st, d, step, n, cfg)
    torch.cuda.synchronize()
    norm, clip, coef = (float(v) for v in st.out)
    print(f"autoclip_adam_kernel, full vector, config {ci}, t {t}: norm {norm!r} clip value {clip!r} coefficient {coef!r}")
    assert step.tolist() == [t, 0] and int(st.ctl[0]) == 1 and int(st.ctl[4]) == 0
    _assert_guards(bufs, x, n)
    assert math.isnan(norm) if norm_kind == "nan" else norm == math.inf
    assert math.isnan(clip) and math.isnan(coef), (clip, coef)            # np.percentile([n]) and clip_grad_norm_'s clamp
    got = tuple(d[k].detach().cpu().numpy() for k in "pmv")
    want = A.adam_step_fp32(x["p"], x["g"], x["m"], x["v"], t, lr, b1, b2, eps, wd, scale, coef)
    assert not A.class_mismatches(got, want)
    for a in got:
        assert np.isnan(a).all()
    if math.isfinite(coef):
        _judge("autoclip_adam_kernel", (d["p"], d["m"], d["v"]), x, t, cfg, coef)
    g2 = (d["g"] * torch.tensor(scale, dtype=torch.float32, device="cuda")) * torch.tensor(coef, dtype=torch.float32, device="cuda")
    want_dev, count = _adam_step_from(ops, before, g2, t, (lr, b1, b2, eps, wd), 1.0)
    assert count == [t, 0]
    for k, b in zip("pmv", want_dev):
        assert _same_bytes_or_both_nan(d[k], b), k


# ------------------------------------------------------- (c) gatres_fused_finish / _hp, gatres_fused_param_grads_finish
SMALL_NB = 2
SMALL_GRAPHS = [(40, 45), (60, 68)]
_TRAINERS = {}


def _small_batch(pkg):
    tops = [pkg.wdn_synth.make_wdn_topology(n, e, seed=11 + i) for i, (n, e) in enumerate(SMALL_GRAPHS)]
    offs = np.cumsum([0] + [n for n, _ in SMALL_GRAPHS])
    ei = torch.cat([t + int(o) for t, o in zip(tops, offs[:-1])], dim=1)
    npg = [n for n, _ in SMALL_GRAPHS]
    N = int(offs[-1])
    y = torch.randn(N, generator=torch.Generator().manual_seed(4)).cuda()
    mask = torch.from_numpy(pkg.wdn_synth.generate_batch_mask(npg, 0.95, np.random.RandomState(2))).cuda()
    return ei.cuda(), N, npg, y, mask


def _small_trainer(pkg, oracle, nc, **kw):
    model, _ = build(pkg, oracle, SMALL_NB, nc, seed=17 + nc, fused=kw.get("fused", True))
    ei, N, npg, y, mask = _small_batch(pkg)
    tr = pkg.GATResTrainer(model, ei, N, nodes_per_graph=npg, **kw)
    return model, tr, y, mask


def _adam_step_from(ops, before, g, t, hp, scale):
    """gatres_adam_step on clones of a before-state: returns p, m, v and the step count it leaves."""
    p, m, v = (before[k].clone() for k in "pmv")
    step = torch.tensor([t - 1, 0], dtype=torch.int64, device="cuda")
    ops.adam_step(p, g.contiguous(), m, v, step, *hp, scale)
    torch.cuda.synchronize()
    return (p, m, v), step.tolist()


def _all_regular(before, g):
    x = {k: before[k].detach().cpu().numpy() for k in "pmv"}
    x["g"] = g.detach().cpu().numpy()
    x["special"], x["regular"] = [], np.ones(len(x["p"]), dtype=bool)
    return x


@pytest.mark.parametrize("ci", range(len(A.CONFIGS)))
@pytest.mark.parametrize("nc", [8, 16, 32])
def test_fused_update_launches_element_by_element_and_bitwise_equal_to_adam_step(pkg, oracle, lib, ops, nc, ci):
    """The slab sum + Adam launch (reduce_adam_kernel: gatres_fused_finish, gatres_fused_finish_hp) and, where the parameter
    gradients fold (nc 16, 32), parameter gradients + slab sum + Adam in one launch (param_grads_finish_kernel), driven as
    test_folded_update_equals_the_two_launch_form does.  Moments filled, t poked, grad_scale 0.5; with a hparams buffer the
    by-value arguments are other numbers, so only the buffer's can give the expected bytes.  After the launch ``grads``
    holds the summed gradient: from the before-state and that gradient gatres_adam_step must leave the same bytes, the
    float64 statement must hold them within bounds, and scratch's transposed conv weights must be those of the new p."""
    if nc not in _TRAINERS:
        _TRAINERS[nc] = _small_trainer(pkg, oracle, nc, use_graph=False)
    model, tr, y, mask = _TRAINERS[nc]
    p0 = model.flat_parameters.detach().clone()
    try:
        _fused_update_case(pkg, lib, ops, nc, ci, model, tr, y, mask, p0)
    finally:                                 # the trainer is shared: a failing case hands no shifted parameters to the next
        with torch.no_grad():
            model.flat_parameters.copy_(p0)
        tr.invalidate_weights()


def _fused_update_case(pkg, lib, ops, nc, ci, model, tr, y, mask, p0):
    from gnn_pressure_estimation_amd import train_step as TS
    assert tr.fused
    folds = lib.gatres_fused_finish_folds(model._cmodel_ref(), tr.plan.ref()) == 1
    assert folds == (nc != 8)
    lr, b1, b2, eps, wd, _ = A.CONFIGS[ci]
    hp, scale = (lr, b1, b2, eps, wd), 0.5
    cfg = hp + (scale,)
    other = (1.0, 0.1, 0.2, 1.0, 1.0)                                    # by-value arguments beside a hparams buffer
    hp_dev = torch.tensor(hp, dtype=torch.float64, device="cuda")
    P = tr.P
    gen = torch.Generator().manual_seed(100 * nc + ci)
    m0 = (torch.randn(P, generator=gen) * 1e-3).cuda()
    v0 = (torch.rand(P, generator=gen) * 1e-5).cuda()
    st = pkg._native.current_stream(tr.device)
    m, g = model._cmodel_ref(), tr.plan.ref(model._cmodel_ref())
    entries = ["finish", "finish_hp"] + (["folded", "folded_hp"] if folds else [])
    grads_seen = []
    for k, entry in enumerate(entries):
        t = A.STEPS[(ci + 2 * k + nc // 8) % len(A.STEPS)]
        with torch.no_grad():
            model.flat_parameters.copy_(p0)
        tr.invalidate_weights()
        tr.exp_avg.copy_(m0); tr.exp_avg_sq.copy_(v0)
        tr.step_counter.copy_(torch.tensor([t - 1, 0], dtype=torch.int64))
        before = dict(p=p0.clone(), m=m0.clone(), v=v0.clone())
        tr.grads.fill_(float("nan"))
        tr.load_batch(y, y, mask)
        tr._enqueue(TS.PHASE_FORWARD | TS.PHASE_BACKWARD, False, flags=TS.FLAG_GRADS_DEFERRED)
        state = (1, model.flat_parameters.data_ptr(), tr.exp_avg.data_ptr(), tr.exp_avg_sq.data_ptr(), tr.step_counter.data_ptr())
        by_value = other if entry.endswith("_hp") else hp
        hparams = hp_dev.data_ptr() if entry.endswith("_hp") else None
        if entry.startswith("folded"):
            pkg._native.check(lib.gatres_fused_param_grads_finish(m, g, tr.saved.data_ptr(), tr.scratch.data_ptr(),
                                                                  tr.grads.data_ptr(), None, None, *state, *by_value, hparams,
                                                                  scale, 0, SMALL_NB, st), entry)
        else:
            pkg._native.check(lib.gatres_fused_param_grads(m, g, tr.saved.data_ptr(), tr.scratch.data_ptr(), st), "param_grads")
            if entry == "finish":
                pkg._native.check(lib.gatres_fused_finish(m, g, tr.scratch.data_ptr(), tr.grads.data_ptr(), None, None, *state,
                                                          *by_value, scale, st), entry)
            else:
                pkg._native.check(lib.gatres_fused_finish_hp(m, g, tr.scratch.data_ptr(), tr.grads.data_ptr(), None, None, *state,
                                                             *by_value, hparams, scale, None, 0, 0.0, 0, None, st), entry)
        torch.cuda.synchronize()
        assert tr.step_counter.tolist() == [t, 0], entry
        grads = tr.grads.clone()
        assert torch.isfinite(grads).all() and float(grads.abs().max()) > 0
        grads_seen.append(grads)
        got = (model.flat_parameters.detach().clone(), tr.exp_avg.clone(), tr.exp_avg_sq.clone())
        want, count = _adam_step_from(ops, before, grads, t, hp, scale)
        assert count == [t, 0]
        for what, a, b in zip(("p", "exp_avg", "exp_avg_sq"), got, want):
            assert _same_bytes(a, b), (entry, what, int((_bits(a) != _bits(b)).sum()), float((a - b).abs().max()))
        assert not _same_bytes(got[0], p0)
        kernel = f"param_grads_finish_kernel<{nc}>" if entry.startswith("folded") else "reduce_adam_kernel"
        _judge(kernel, got, _all_regular(before, grads), t, cfg)
        # scratch's transposed conv weights: deriving them again from the new p must change no byte of scratch ...
        scratch = tr.scratch.clone()
        tr._prepare_backward()
        torch.cuda.synchronize()
        assert _same_bytes(tr.scratch, scratch), (entry, "transposed weights are not those of the new parameters")
        with torch.no_grad():                                              # ... and from other parameters it does
            model.flat_parameters.add_(1.0)
        tr._prepare_backward()
        torch.cuda.synchronize()
        assert not _same_bytes(tr.scratch, scratch)
    for gk in grads_seen[1:]:                                             # the same chain, the same gradient, whoever sums it
        assert _same_bytes(gk, grads_seen[0])


# ------------------------------------------------------------------------------------------------------ (d) trainer routes
ROUTES = {
    "fused-eager": dict(fused=True, use_graph=False),
    "fused-graph": dict(fused=True, use_graph=True),
    "fused-graph-device-mask": dict(fused=True, use_graph=True, device_mask=True),
    "per-op-eager": dict(fused=False, use_graph=False),
    "per-op-graph": dict(fused=False, use_graph=True),
    "collective-one-bucket": dict(fused=True, use_graph=True, force_collective_path=True, buckets=1),
    "collective-one-bucket-device-mask": dict(fused=True, use_graph=True, force_collective_path=True, buckets=1,
                                              device_mask=True),
    "collective-two-buckets": dict(fused=True, use_graph=True, force_collective_path=True, buckets=2),
    "collective-per-op": dict(fused=False, use_graph=False, force_collective_path=True, buckets=1),
    "clipping-fused-graph": dict(fused=True, use_graph=True, use_gradient_clipping=True),
    "clipping-fused-graph-device-mask": dict(fused=True, use_graph=True, use_gradient_clipping=True, device_mask=True),
    "clipping-per-op-eager": dict(fused=False, use_graph=False, use_gradient_clipping=True),
}
# the hyper-parameters of the three steps: the constructor's, then two changes through set_hparams
ROUTE_HPARAMS = [A.CONFIGS[0][:5], A.CONFIGS[1][:5], A.CONFIGS[3][:5]]


@pytest.mark.parametrize("nc", [8, 32])
@pytest.mark.parametrize("route", list(ROUTES))
def test_trainer_steps_element_by_element_and_bitwise_equal_to_adam_step(pkg, oracle, ops, route, nc):
    """GATResTrainer.step through every route to an update kernel, three steps, the hyper-parameters changed between them
    with set_hparams (a captured step must read the device buffer).  Each step is judged on its own from the kernel's own
    prior state -- p, exp_avg, exp_avg_sq and the step count cloned before it, ``tr.grads`` (and under clipping
    ``last_clip_coef``) read after it -- so the bounds stay as tight as for a single launch."""
    kw = dict(ROUTES[route])
    buckets, device_mask = kw.pop("buckets", None), kw.pop("device_mask", False)
    lr, b1, b2, eps, wd = ROUTE_HPARAMS[0]
    model, tr, y, mask = _small_trainer(pkg, oracle, nc, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd,
                                        percentile=PERCENTILE, **kw)
    assert tr.fused == kw["fused"] and tr.use_graph == kw["use_graph"] and tr.world == 1
    if buckets is not None:
        tr.fused_buckets = buckets
        assert tr.split
    clipped = []
    for it, hp in enumerate(ROUTE_HPARAMS):
        if it:
            tr.set_hparams(lr=hp[0], beta1=hp[1], beta2=hp[2], eps=hp[3], weight_decay=hp[4])
        torch.cuda.synchronize()
        before = dict(p=model.flat_parameters.detach().clone(), m=tr.exp_avg.clone(), v=tr.exp_avg_sq.clone())
        t = int(tr.step_counter[0]) + 1
        assert t == it + 1
        # (targets 16 and 256 times as large: the gradient norm hardly moves below a factor of 16 -- 95 % of the inputs are
        #  masked to zero -- and grows several times with each of these, so AutoClip clips the second and third step for real)
        yk = y * float(16 ** it)
        if device_mask:
            tr.load_batch(yk, yk)
            tr.run_step(device_mask=True)
        else:
            tr.step(yk, yk, mask)
        torch.cuda.synchronize()
        assert tr.step_counter.tolist() == [t, 0] and tr.fault_count == 0 and tr.dropped_steps == 0
        g = tr.grads.clone()
        assert torch.isfinite(g).all() and float(g.abs().max()) > 0
        coef = 1.0
        if tr._clip is not None:
            coef = float(tr.last_clip_coef)
            assert 0.0 < coef <= 1.0
            clipped.append(coef)
            g_used = (g * torch.tensor(1.0, dtype=torch.float32, device="cuda")) * torch.tensor(coef, dtype=torch.float32, device="cuda")
        else:
            g_used = g
        got = (model.flat_parameters.detach().clone(), tr.exp_avg.clone(), tr.exp_avg_sq.clone())
        want, count = _adam_step_from(ops, before, g_used, t, hp, 1.0)
        assert count == [t, 0]
        for what, a, b in zip(("p", "exp_avg", "exp_avg_sq"), got, want):
            assert _same_bytes(a, b), (route, it, what, int((_bits(a) != _bits(b)).sum()), float((a - b).abs().max()))
        assert not _same_bytes(got[0], before["p"])
        _judge(f"GATResTrainer.step ({route})", got, _all_regular(before, g), t, tuple(hp) + (1.0,), coef)
    if tr._clip is not None:
        assert min(clipped) < 0.9, clipped                               # clipped for real at least once
