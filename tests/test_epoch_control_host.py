"""The epoch-boundary controller of ``GATResTrainer.fit`` on the host: ``epoch_control.EpochController`` (the plain-Python
statement of what ``gatres_epoch_control`` computes) against recorded results of the reference's ``EarlyStopping`` and of
torch's ``ReduceLROnPlateau`` (tests/golden/epoch_control_traces.json), against torch's scheduler run live, and the
header / ctypes agreement of the new C-ABI entries."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gatres.h")


def dec(s):
    if s is None:
        return None
    return {"nan": math.nan, "inf": math.inf, "-inf": -math.inf}.get(s) if s in ("nan", "inf", "-inf") else float.fromhex(s)


def same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def traces():
    with open(os.path.join(ROOT, "tests", "golden", "epoch_control_traces.json")) as f:
        return json.load(f)["cases"]


def controller(pkg, case):
    return pkg.epoch_control.EpochController(dec(case["lr"]), patience=case["patience"], min_delta=dec(case["min_delta"]),
                                             scheduler_patience=case["scheduler_patience"])


def test_the_traces_hold_the_cases_the_controller_must_get_right():
    cases = {c["name"]: c for c in traces()}
    vals = lambda n: [dec(v) for v in cases[n]["val_losses"]]
    assert {c["patience"] for c in cases.values()} >= {0, 1, 3} and {c["scheduler_patience"] for c in cases.values()} >= {0, 2}
    assert math.isnan(vals("nan_first")[0]) and math.isnan(vals("nan_in_the_middle")[2])
    a, b = vals("fp32_equal_fp64_different")[:2]
    assert a != b and np.float32(a) == np.float32(b)
    assert len(set(vals("exact_tie")[:3])) == 1 and len(set(vals("plateau")[1:])) == 1
    d = np.diff(vals("small_improvement"))
    assert (d < 0).all() and (-d < dec(cases["small_improvement"]["min_delta"])).all()
    lrs = [dec(e["lr"]) for e in cases["eps_floor"]["epochs"]]
    assert lrs[-1] == lrs[-5] and 0 < lrs[-1] * 0.9 <= 1e-8 and lrs[-1] < lrs[0]              # stuck at the eps floor
    stop, free = cases["stop_preempts_scheduler"]["epochs"], cases["no_preempt_for_comparison"]["epochs"]
    assert stop[-1]["stop"] and dec(stop[-1]["lr"]) == dec(stop[0]["lr"]) and dec(free[3]["lr"]) < dec(free[2]["lr"])
    assert not any(e["stop"] for e in cases["patience_0"]["epochs"]) and len(cases["patience_0"]["epochs"]) == 8


@pytest.mark.parametrize("case", traces(), ids=lambda c: c["name"])
def test_mirror_reproduces_the_recorded_results(pkg, case):
    ctl = controller(pkg, case)
    vals = [dec(v) for v in case["val_losses"]]
    for k, want in enumerate(case["epochs"]):
        rec = ctl.step(0.0, vals[k])
        assert bool(rec["stop"]) == want["stop"] == ctl.stopped, k
        assert rec["es_bad"] == want["es_bad"], k
        if want["es_best"] is None:
            assert ctl.es_best is None
        else:
            assert same(float(ctl.es_best), dec(want["es_best"])), k
        assert ctl.lr == dec(want["lr"]) == rec["lr_after"], k
        assert rec["sched_bad"] == want["sched_bad"] and same(rec["sched_best"], dec(want["sched_best"])), k
    assert ctl.stopped == case["epochs"][-1]["stop"]
    if ctl.stopped:
        assert len(case["epochs"]) <= len(vals)


def test_mirror_equals_torch_scheduler_on_random_sequences(pkg):
    rng = np.random.RandomState(11)
    drops = 0
    for trial in range(300):
        n = int(rng.randint(5, 40))
        kind = trial % 4
        if kind == 0:
            seq = np.abs(1.0 + np.cumsum(rng.randn(n) * 0.02))
        elif kind == 1:
            seq = np.round(rng.rand(n), 1)                                    # many exact ties
        elif kind == 2:
            seq = np.exp(-np.arange(n) * rng.rand()) * (1 + 1e-4 * rng.randn(n))
        else:
            seq = rng.rand(n)
            seq[rng.randint(n)] = np.nan
        lr = float(10.0 ** rng.uniform(-8, -2))
        sp = int(rng.randint(0, 4))
        opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=lr)
        sch = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="min", patience=sp)
        ctl = pkg.epoch_control.EpochController(lr, patience=0, scheduler_patience=sp)
        for v in seq:
            sch.step(float(v))
            rec = ctl.step(0.0, float(v))
            assert ctl.lr == opt.param_groups[0]["lr"]
            assert rec["sched_bad"] == sch.num_bad_epochs and same(rec["sched_best"], sch.best)
        drops += ctl.lr < lr
    assert drops > 100


def test_best_bookkeeping_and_scheduler_off(pkg):
    ctl = pkg.epoch_control.EpochController(1e-3, patience=0, scheduler=False)
    seen = [ctl.step(1.0, v) for v in (0.5, 0.5, 0.4, math.nan, 0.45, 0.4)]
    assert [r["improved"] for r in seen] == [1.0, 0.0, 1.0, 0.0, 0.0, 0.0]                # strict, fp64
    assert ctl.best_loss == 0.4 and ctl.best_epoch == 3 and ctl.lr == 1e-3 and not ctl.stopped
    assert pkg.epoch_control.weighted_mean([0.5, 0.25], [32, 5]) == (0.5 * 32 + 0.25 * 5) / 37


# ---- header / ctypes -------------------------------------------------------------------------------------------------------
def _define(name):
    m = re.search(rf"#define\s+{name}\s+(\S+)", open(HEADER).read())
    assert m, name
    return int(m.group(1))


def test_epoch_constants_of_the_header_and_the_python_side(pkg):
    N, M = pkg._native, pkg.epoch_control
    assert _define("GATRES_EPOCH_RECORD") == N.EPOCH_RECORD == M.RECORD
    assert _define("GATRES_EPOCH_STATE") == N.EPOCH_STATE == M.STATE == len(M.STATE_FIELDS)
    for k, name in enumerate(M.STATE_FIELDS):
        assert _define("GATRES_EPOCH_S_" + name.upper()) == k
    for k, name in enumerate(M.RECORD_FIELDS):
        assert _define("GATRES_EPOCH_R_" + name.upper()) == k
    assert len(M.RECORD_FIELDS) <= M.RECORD
    assert _define("GATRES_ABI_VERSION") == N.ABI_VERSION == 9
    for name in ("gatres_epoch_control", "gatres_epoch_val_sums", "gatres_snapshot_if"):
        assert name in N.SIGNATURES


def test_epoch_config_struct_layout_matches_the_header(pkg):
    """Field order, types, offsets and size of gatres_epoch_config_t as a C compiler lays the header's declaration out."""
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct gatres_epoch_config \{(.*?)\} gatres_epoch_config_t;", hdr, flags=re.S).group(1)
    fields = re.findall(r"(double|int32_t)\s+(\w+);", body)
    size = {"double": 8, "int32_t": 4}
    ctype = {"double": C.c_double, "int32_t": C.c_int32}
    cls = pkg._native.GatresEpochConfig
    assert [n for n, _ in cls._fields_] == [n for _, n in fields]
    off = 0
    for t, n in fields:
        off = (off + size[t] - 1) // size[t] * size[t]
        assert getattr(cls, n).offset == off and dict(cls._fields_)[n] is ctype[t], n
        off += size[t]
    assert C.sizeof(cls) == (off + 7) // 8 * 8 == 56


def test_library_exports_the_epoch_entry_points(lib):
    for name in ("gatres_epoch_control", "gatres_epoch_val_sums", "gatres_snapshot_if"):
        assert hasattr(lib, name)
    # argument errors are refused before anything is launched (no device needed)
    assert lib.gatres_snapshot_if(None, None, None, None, None, None, None, None, None, 4, None) == -1
    assert lib.gatres_epoch_control(None, None, None, None, 0, None, None, None, None, None, 1, None) == -1
