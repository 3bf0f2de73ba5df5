"""The fused kernels on either side of every segment size at which their LDS plan turns over (tests/fused_plan_cases.py: found
by search with the restatement tests/fused_plan_refs.py, never written down): the training launch of the window kernel where
keep-in-LDS stops fitting and where parts pass 64 own rows (up to 352), the uncached whole-segment kernel unsplit, split and in
forward-only inference, the cached kernel with its borrowed W slot, and the hand-over to the per-op path.

Every test first asks ``gatres_fused_plan`` -- the decision function the launch itself calls -- what this device will launch for
the plan it really built, and FAILS if that is not the kind the case is named for: no test passes on another kernel.

Order of sums.  The whole-segment kernel runs the same stage functions cached or not (k_fused_whole.hip: seg_softmax, seg_gather,
seg_mean_fwd, seg_proj); uncached they read their operands from the segment's saved tables in global memory instead of the LDS
copies, row by row over the same CSR in the same order, and the projections take the same MFMA tiles.  They are the functions the
existing split tests hold bit-identical to the per-op kernels on WDN graphs, so the predictions are held to ``torch.equal`` with
the per-op model here too, next to the project's 2e-5 against the fp32 oracle.  Gradients: per tensor, the fp64 oracle as arbiter
(test_gpu_model.check_gradients_vs_fp64, unchanged)."""
import ctypes as C

import numpy as np
import pytest
import torch

import fused_plan_cases as FC
import fused_plan_refs as FR
from test_gpu_irregular import _split
from test_gpu_model import build, check_gradients_vs_fp64, note, relerr

pytestmark = pytest.mark.gpu

CASES = FC.cases()
FUSED = [c for c in CASES if c["rc"] == 0]
PER_OP = [c for c in CASES if c["rc"] != 0]
_G64 = {}
_REF = {}
PH_MASK_WITHOUT_OW64 = str(0xffff & ~FR.FACT_OW64)


@pytest.fixture(autouse=True)
def stop_at_a_gpu_fault():
    """A launch that faulted leaves the device in error for whatever follows: end the run there, not test by test."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the GPU reported an error after this test, nothing more is launched: {e}", returncode=3)


def _ids(cases):
    return [c["id"] for c in cases]


def _graph_cases():
    """One hipGraph case per kind of launch: the smallest case of each kind."""
    first = {}
    for c in sorted(FUSED, key=lambda c: c["n"]):
        first.setdefault(c["kind"], c)
    return list(first.values())


def record(case, what, got, errors):
    """note(...) for the parity report: the size found, the kind launched, the errors (the record of one run, as a table:
    profiles/fused_plan_turnover.txt)."""
    note(f"fused plan turnover {case['id']} {what}", {"nb": case["nb"], "split": case["split"], "launched": got, "errors": errors})


def asked(lib, model, plan, phases, inference=False):
    """(rc, words) of gatres_fused_plan for the CURRENT device (num_cus = 0) and the plan as bound for this model."""
    import gnn_pressure_estimation_amd as G
    m = G._native.GatresModel(model.num_blocks, model.nc, G._native.DTYPE_F32, FR.MODEL_INFERENCE if inference else 0)
    out = (C.c_int32 * len(FR.WORDS))()
    rc = lib.gatres_fused_plan(C.byref(m), plan.ref(model._cmodel_ref()), phases, 0, out)
    return rc, dict(zip(FR.WORDS, list(out)))


def require_kind(lib, case, model, plan, phases=FR.TRAIN, inference=False):
    """The device launches what the case is named for: the restatement's words for this plan, the probed-dispatch fact apart
    (it is the device's).  Returns the kind."""
    f = FR.figures_of(plan)
    assert f == FC.figures(case["n"]), "the GPU process built another plan than the search did"
    rc, got = asked(lib, model, plan, phases, inference)
    want_rc, want = FR.fused_plan(case["nb"], case["nc"], f, phases=phases, cus=got["cus"] or 256, inference=inference,
                                  split=case["split"], probed=bool(got["facts"] & FR.FACT_PROBED))
    assert (rc, got) == (want_rc, want), (case["id"], rc, got, want_rc, want)
    assert FC.check_side(case) and (rc != 0 or got["cus"] == 256), (case["id"], got)
    if phases == FR.TRAIN:
        assert dict(got, facts=got["facts"] & ~FR.FACT_PROBED) == case["plan"], (case["id"], got, case["plan"])
    return FR.kind(got, rc)


def reference(pkg, oracle, case):
    """Per case, computed once and left unchanged: the batch, two targets and masks, the parameters, the fp32 oracle's
    prediction and gradient for the module's loss, the fp64 gradient function, and OracleTrainer's two steps."""
    if case["id"] in _REF:
        return _REF[case["id"]]
    nb, nc, seed = case["nb"], case["nc"], 900 + case["nc"] + case["n"] % 97
    ei, npg = FC.batch(case["n"])
    N = sum(npg)
    g = torch.Generator().manual_seed(seed)
    ys = [torch.randn(N, 1, generator=g) for _ in range(2)]
    masks = [torch.from_numpy(pkg.wdn_synth.generate_batch_mask(npg, 0.95, np.random.RandomState(seed + k))) for k in range(2)]
    p = oracle.init_params(nb, nc, seed=seed)
    xin = ys[0].clone()
    xin[masks[0]] = 0
    leaves = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    o32 = oracle.gatres_forward(leaves, xin, ei, num_blocks=nb)
    torch.nn.functional.mse_loss(o32[masks[0]], ys[0][masks[0]]).backward()

    def grads64(params64):
        lv = {k: v.clone().requires_grad_(True) for k, v in params64.items()}
        o = oracle.gatres_forward(lv, xin.double(), ei, num_blocks=nb)
        torch.nn.functional.mse_loss(o[masks[0]], ys[0].double()[masks[0]]).backward()
        return {k: v.grad for k, v in lv.items()}

    steps = 2 if case["plan"]["parts"] > 1 or case["rc"] != 0 else 1       # (a second step where hand-off epochs persist)
    tr = oracle.OracleTrainer(p)
    ref_steps = []
    for it in range(steps):
        l_ref, o_ref = tr.step(ys[it].clone(), ys[it], ei, masks[it])
        ref_steps.append((l_ref.detach().clone(), o_ref.detach().clone(), {k: v.clone() for k, v in tr.grads().items()}))
    _REF[case["id"]] = dict(ei=ei, npg=npg, N=N, ys=ys, masks=masks, p=p, xin=xin, o32=o32.detach(), seed=seed,
                            ref32={k: v.grad for k, v in leaves.items()}, grads64=grads64,
                            p64={k: v.double() for k, v in p.items()}, steps=ref_steps)
    return _REF[case["id"]]


def models(pkg, oracle, case, ref, per_op=True):
    mf, _ = build(pkg, oracle, case["nb"], case["nc"], seed=ref["seed"], fused=True)       # (init_params(seed): ref["p"])
    mp = build(pkg, oracle, case["nb"], case["nc"], seed=ref["seed"], fused=False)[0] if per_op else None
    return mf, mp


def training(pkg, oracle, lib, case, use_graph, expect_fused=True):
    """The module's forward and backward, then GATResTrainer steps on one scratch buffer.  Returns (kind, errors)."""
    ref = reference(pkg, oracle, case)
    mf, mp = models(pkg, oracle, case, ref)
    dx, dei, dm = ref["xin"].cuda(), ref["ei"].cuda(), ref["masks"][0].cuda()
    plan = mf.plan_for(dei, ref["N"])
    kind = require_kind(lib, case, mf, plan)
    assert bool(lib.gatres_fused_supported(mf._cmodel_ref(), plan.ref())) == expect_fused
    out = mf(dx, dei)
    with torch.no_grad():
        out_per_op = mp(dx, dei)
    e_mod = relerr(out, ref["o32"])
    same = torch.equal(out.detach(), out_per_op)
    torch.nn.functional.mse_loss(out[dm], ref["ys"][0].cuda()[dm]).backward()
    hip = {k: prm.grad for k, prm in zip(ref["p"], mf.parameters())}
    key = ("turnover", case["id"])
    m_grad = check_gradients_vs_fp64(hip, ref["ref32"], ref["grads64"], ref["p64"], _G64, key)
    tr = pkg.GATResTrainer(mf, dei, ref["N"], nodes_per_graph=ref["npg"], use_graph=use_graph)
    assert tr.fused == expect_fused
    errs = []
    for it, (l_ref, o_ref, g_ref) in enumerate(ref["steps"]):
        loss = tr.step(ref["ys"][it].cuda(), ref["ys"][it].cuda(), ref["masks"][it].cuda())
        e_o, e_l = relerr(tr.out, o_ref), relerr(loss, l_ref)
        errs += [e_o, e_l]
        if it == 0:
            t_hip = _split(tr.grads.detach().cpu(), oracle.param_shapes(case["nb"], case["nc"]))
            t_grad = check_gradients_vs_fp64(t_hip, g_ref, ref["grads64"], ref["p64"], _G64, key)
    errors = dict(module_out=e_mod, module_grad=list(m_grad), steps_out_loss=errs, step_grad=list(t_grad), graph=use_graph,
                  equals_per_op=same)
    record(case, "training" + (" graph" if use_graph else ""), kind, errors)
    assert same, "predictions differ from the per-op model's bits"
    assert e_mod < 2e-5, e_mod
    assert all(e < 2e-5 for e in errs), errs
    assert tr.fault_count == 0 and tr.dropped_steps == 0
    return kind, errors


@pytest.mark.parametrize("case", FUSED, ids=_ids(FUSED))
def test_training_launches(pkg, oracle, lib, case, monkeypatch):
    if case["split"]:
        monkeypatch.setenv("GATRES_FUSED_SPLIT", str(case["split"]))
    kind, _ = training(pkg, oracle, lib, case, use_graph=False)
    assert kind == case["kind"]


@pytest.mark.parametrize("case", _graph_cases(), ids=_ids(_graph_cases()))
def test_training_launches_in_a_captured_graph(pkg, oracle, lib, case, monkeypatch):
    if case["split"]:
        monkeypatch.setenv("GATRES_FUSED_SPLIT", str(case["split"]))
    kind, _ = training(pkg, oracle, lib, case, use_graph=True)
    assert kind == case["kind"]


@pytest.mark.parametrize("case", FUSED, ids=_ids(FUSED))
def test_inference_launch(pkg, oracle, lib, case, monkeypatch):
    """The forward-only launch under torch.no_grad() -- where the window kernel does not fit, every such launch takes the
    whole-segment kernel without a saved buffer -- equals the training forward and the per-op model bit for bit, twice on one
    scratch buffer, and meets the fp32 oracle."""
    if case["split"]:
        monkeypatch.setenv("GATRES_FUSED_SPLIT", str(case["split"]))
    ref = reference(pkg, oracle, case)
    mf, mp = models(pkg, oracle, case, ref)
    dx, dei = ref["xin"].cuda(), ref["ei"].cuda()
    plan = mf.plan_for(dei, ref["N"])
    kind = require_kind(lib, case, mf, plan, phases=FR.PHASE_FORWARD, inference=True)
    with torch.no_grad():
        o1 = mf(dx, dei).clone()
        o2 = mf(dx, dei).clone()
        op = mp(dx, dei)
    e = relerr(o1, ref["o32"])
    same = torch.equal(o1, op)
    record(case, "inference", kind, dict(out=e, equals_per_op=same))
    assert torch.equal(o1, o2) and same and e < 2e-5, (same, e)
    assert torch.equal(mf(dx, dei).detach(), o1)                      # the training forward (a saved buffer, a grad node)
    assert kind == case["kind"].replace(" keep", "")                  # (keep-in-LDS is the training launch's alone)


SWITCHED = [c for c in FUSED if c["side"] == "low" and c["turnover"] in ("keep", "rows64")]


@pytest.mark.parametrize("case", SWITCHED, ids=_ids(SWITCHED))
def test_switch_gives_same_bytes(pkg, oracle, lib, case, monkeypatch):
    """The low side of `keep` differs from its neighbour in keep-in-LDS only, the low side of `rows64` in launch fact 0x1000
    only: the same batch with that one thing switched off (GATRES_FUSED_NO_KEEP=1, GATRES_WINDOW_PH_MASK without the bit) takes
    the neighbour's code on this side's operands and must give the same bytes -- predictions, loss, gradient, parameters."""
    ref = reference(pkg, oracle, case)
    env = {"GATRES_FUSED_NO_KEEP": "1"} if case["turnover"] == "keep" else {"GATRES_WINDOW_PH_MASK": PH_MASK_WITHOUT_OW64}
    res = []
    for switched in (False, True):
        for k, v in env.items():
            if switched:
                monkeypatch.setenv(k, v)
        mf, _ = models(pkg, oracle, case, ref, per_op=False)
        dei = ref["ei"].cuda()
        tr = pkg.GATResTrainer(mf, dei, ref["N"], nodes_per_graph=ref["npg"], use_graph=False)
        rc, got = asked(lib, mf, tr.plan, FR.TRAIN)
        assert rc == 0 and got["window"] == 1 and got["parts"] == case["plan"]["parts"]
        if case["turnover"] == "keep":
            assert got["keep"] == (0 if switched else 1)
        else:
            assert got["facts"] & FR.FACT_OW64          # (the mask is applied in the launch: the plan still has the fact)
        outs = []
        for it in range(2):
            loss = tr.step(ref["ys"][it].cuda(), ref["ys"][it].cuda(), ref["masks"][it].cuda())
            outs += [tr.out.clone(), loss.clone(), tr.grads.clone()]
        outs.append(mf.flat_parameters.clone())
        assert tr.fault_count == 0 and tr.dropped_steps == 0
        res.append(outs)
    for u, v in zip(*res):
        assert torch.isfinite(u).all() and torch.equal(u, v)
    record(case, "switched off", "same bytes", env)


@pytest.mark.parametrize("case", PER_OP, ids=_ids(PER_OP))
def test_unsupported_side_takes_the_per_op_path(pkg, oracle, lib, case):
    """One node past what the uncached kernel's LDS (or the 4096-node cap) takes: the library says so, model and trainer take
    the per-op kernels, and they still meet the oracle."""
    ref = reference(pkg, oracle, case)
    mf, _ = models(pkg, oracle, case, ref, per_op=False)
    dx, dei, dm = ref["xin"].cuda(), ref["ei"].cuda(), ref["masks"][0].cuda()
    plan = mf.plan_for(dei, ref["N"])
    assert require_kind(lib, case, mf, plan) == "per-op"
    assert lib.gatres_fused_supported(mf._cmodel_ref(), plan.ref()) == 0
    assert lib.gatres_fused_cus_per_segment(mf._cmodel_ref(), plan.ref()) == 0
    out = mf(dx, dei)
    e_mod = relerr(out, ref["o32"])
    with torch.no_grad():
        assert torch.equal(mf(dx, dei), out.detach())
    torch.nn.functional.mse_loss(out[dm], ref["ys"][0].cuda()[dm]).backward()
    hip = {k: prm.grad for k, prm in zip(ref["p"], mf.parameters())}
    key = ("turnover", case["id"])
    m_grad = check_gradients_vs_fp64(hip, ref["ref32"], ref["grads64"], ref["p64"], _G64, key)
    tr = pkg.GATResTrainer(mf, dei, ref["N"], nodes_per_graph=ref["npg"], use_graph=False)
    assert not tr.fused
    errs = []
    for it, (l_ref, o_ref, g_ref) in enumerate(ref["steps"]):
        loss = tr.step(ref["ys"][it].cuda(), ref["ys"][it].cuda(), ref["masks"][it].cuda())
        errs += [relerr(tr.out, o_ref), relerr(loss, l_ref)]
        if it == 0:
            t_hip = _split(tr.grads.detach().cpu(), oracle.param_shapes(case["nb"], case["nc"]))
            t_grad = check_gradients_vs_fp64(t_hip, g_ref, ref["grads64"], ref["p64"], _G64, key)
    record(case, "training", "per-op", dict(module_out=e_mod, module_grad=list(m_grad), steps_out_loss=errs, step_grad=list(t_grad)))
    assert e_mod < 2e-5 and all(e < 2e-5 for e in errs), (e_mod, errs)
    assert tr.fault_count == 0 and tr.dropped_steps == 0
