"""``gatres_fused_plan`` -- the decision function a fused launch itself calls -- held word for word to the plain-Python
restatement (tests/fused_plan_refs.py), asked for 256 CUs on a machine without a GPU:

  * every case of tests/fused_plan_cases.py lands on the side of its turnover it is named for, in the restatement and in the
    library, on the plan ``GraphPlan`` really builds for the batch, for the training launch and the two forward-only launches;
  * the two agree on a sweep over segment sizes, widths, depths, segment counts, CU counts and phases on synthetic figures
    (the decision reads nothing but figures);
  * a restatement with ONE formula off by one 16-row tile is caught by that sweep.

Host only: integers, equality, no tolerance."""
import ctypes as C
import os
import re

import pytest
import torch

import fused_plan_cases as FC
import fused_plan_refs as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWEEP_N = range(16, 4113, 16)
SWEEP_SEGMENTS = (1, 8, 33, 56, 72, 96, 130)
SWEEP_PHASES = (FR.TRAIN, FR.PHASE_FORWARD)
CASES = FC.cases()
_KEEPALIVE = torch.zeros(4, dtype=torch.int32)          # (gatres_graph_t.seg_ptr: non-null, never read by the decision)


def lib_plan(pkg, lib, nb, nc, gref, phases, cus=256, inference=False):
    m = pkg._native.GatresModel(nb, nc, pkg._native.DTYPE_F32, FR.MODEL_INFERENCE if inference else 0)
    out = (C.c_int32 * len(FR.WORDS))(*([-7] * len(FR.WORDS)))
    rc = lib.gatres_fused_plan(C.byref(m), gref, phases, cus, out)
    return rc, dict(zip(FR.WORDS, list(out)))


def graph_of(pkg, f):
    """A gatres_graph_t that holds the figures ``f`` and nothing else."""
    n_all = f.nodes * f.num_segments
    return pkg._native.GatresGraph(n_all, f.edges_gat * f.num_segments, f.edges_mean * f.num_segments, f.num_segments,
                                   *([None] * 9), _KEEPALIVE.data_ptr(), f.nodes, f.edges_gat, f.edges_mean, f.flags,
                                   (C.c_int32 * 21)(*f.windows[:21]), 0, None, (C.c_int32 * 7)(*f.windows[21:28]), 0, None, 0, 0)


def synthetic_figures(n, segments, spread):
    """Figures of ``segments`` WDN-like snapshots of n nodes (11 n / 10 pipes): a part's window is its own rows and ``spread``
    rows on either side, with the edges of that many rows; a tenth of the window's edges cross to another part."""
    pipes = (11 * n) // 10
    win, halo = [], []
    for M in range(2, 9):
        wr = min(n, FR.own_rows(n, M) + 2 * spread)
        gm = (2 * pipes * wr + n - 1) // n
        win += [wr, gm + wr, gm]
        halo.append(gm // 10 + 3)
    return FR.Figures(segments, n, 2 * pipes + n, 2 * pipes, tuple(win + halo), FR.GRAPH_DEG_LE6 | 1)


def test_the_symbol_is_declared_exported_and_bound_and_the_abi_stays(pkg, lib):
    with open(os.path.join(ROOT, "include", "gatres.h")) as f:
        hdr = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert re.search(r"\bgatres_fused_plan\s*\(", hdr) and hasattr(lib, "gatres_fused_plan")
    assert len(pkg._native.SIGNATURES["gatres_fused_plan"][1]) == 5
    assert "#define GATRES_ABI_VERSION 9" in hdr and pkg._native.ABI_VERSION == 9
    assert b"abi9" in lib.gatres_version()
    for k, word in enumerate(FR.WORDS[:-1]):
        assert f"#define GATRES_FUSED_PLAN_{word.upper()} {k}\n" in hdr, word
    assert f"#define GATRES_FUSED_PLAN_WORDS {len(FR.WORDS)}\n" in hdr
    f = synthetic_figures(388, 2, 24)
    g = graph_of(pkg, f)
    m = pkg._native.GatresModel(2, 32, 0, 0)
    out = (C.c_int32 * 12)()
    assert lib.gatres_fused_plan(None, C.byref(g), FR.TRAIN, 256, out) == -1
    assert lib.gatres_fused_plan(C.byref(m), None, FR.TRAIN, 256, out) == -1
    assert lib.gatres_fused_plan(C.byref(m), C.byref(g), FR.TRAIN, 256, None) == -1


def test_the_search_reaches_every_turnover_it_can(pkg):
    """Each width has both sides of every turnover but the ones the module names as unreachable, and those are the ones a WDN
    batch cannot reach: the plan never CHOOSES the cached whole-segment kernel once a segment has two tiles (the window kernel
    fits there), and at nc 8 / 16 the cached kernel's tables stop fitting before its private W slot does."""
    got = {(c["nc"], c["turnover"], c["side"]) for c in CASES}
    missing = {(nc, name) for nc, name, _ in FC.unreachable()}
    assert missing == ({(nc, "cache_chosen") for nc in FC.NCS}
                       | {(nc, name) for nc in (8, 16) for name in ("wslot_unsplit", "wslot_split")})
    for nc in FC.NCS:
        for name in FC.TURNOVERS:
            if (nc, name) not in missing:
                assert {(nc, name, "low"), (nc, name, "high")} <= got, (nc, name)
    by = {c["id"]: c for c in CASES}
    assert any(c["turnover"] == "supported" and c["nc"] == 8 and c["n"] == 4096 and c["side"] == "low" for c in CASES)
    assert any(c["turnover"] == "rows64" and c["plan"]["part_rows"] == 80 for c in CASES)
    assert max(c["plan"]["part_rows"] for c in CASES if c["plan"]["window"]) >= 320
    assert len(by) == len(CASES)


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_case_lands_on_its_side_in_restatement_and_library(pkg, lib, case, monkeypatch):
    if case["split"]:
        monkeypatch.setenv("GATRES_FUSED_SPLIT", str(case["split"]))
    ei, npg = FC.batch(case["n"])
    plan = pkg.GraphPlan(ei, sum(npg), device="cpu")
    f = FR.figures_of(plan)
    assert f == FC.figures(case["n"])
    assert FC.check_side(case)
    # the neighbour is on the OTHER side, one node away
    other = dict(case, n=case["neighbour"], side="high" if case["side"] == "low" else "low")
    assert abs(case["n"] - case["neighbour"]) == 1 and FC.check_side(other) and not FC.check_side(dict(other, side=case["side"]))
    for phases, inference in ((FR.TRAIN, False), (FR.PHASE_FORWARD, False), (FR.PHASE_FORWARD, True), (FR.PHASE_BACKWARD, False)):
        want = FR.fused_plan(case["nb"], case["nc"], f, phases=phases, cus=256, inference=inference, split=case["split"])
        got = lib_plan(pkg, lib, case["nb"], case["nc"], plan.ref(), phases, 256, inference)
        assert got == want, (phases, inference, got, want)
        if phases == FR.TRAIN:
            assert want == (case["rc"], case["plan"])
    m = pkg._native.GatresModel(case["nb"], case["nc"], 0, 0)
    assert lib.gatres_fused_supported(C.byref(m), plan.ref()) == (1 if case["rc"] == 0 else 0)


def _sweep(pkg, lib, ncs, **planted):
    """(comparisons, [(what, library's answer, restatement's answer) that differ])."""
    bad, count, kinds = [], 0, set()
    for spread in (24, 160):
        for segments in SWEEP_SEGMENTS:
            for n in SWEEP_N:
                f = synthetic_figures(n, segments, spread)
                g = graph_of(pkg, f)
                for nc in ncs:
                    for nb, cus in ((2, 256), (1, 104)):
                        for phases in SWEEP_PHASES:
                            got = lib_plan(pkg, lib, nb, nc, C.byref(g), phases, cus)
                            want = FR.fused_plan(nb, nc, f, phases=phases, cus=cus, **planted)
                            count += 1
                            kinds.add((FR.kind(got[1], got[0]), got[1]["launches"]))
                            if got != want:
                                bad.append(((spread, segments, n, nc, nb, cus, phases), got, want))
    return count, bad, kinds


def test_library_and_restatement_agree_on_the_sweep(pkg, lib):
    """n = 16, 32 .. 4112 x nc 8 / 16 / 32 x 1 .. 130 segments x training / forward-only (x two depths and CU counts, two
    window spreads): 43 k decisions, every word.  The sweep crosses every kind of plan, launches in rounds included."""
    count, bad, kinds = _sweep(pkg, lib, FC.NCS)
    assert count == 2 * len(SWEEP_SEGMENTS) * len(SWEEP_N) * 3 * 2 * 2
    assert not bad, (len(bad), bad[:3])
    names = {k for k, _ in kinds}
    assert {"per-op", "whole x1 cached", "whole x1 uncached", "whole x4 uncached", "window x8 keep"} <= names, names
    assert any("rows>64" in k and "keep" in k for k in names) and any("rows>64" in k and "keep" not in k for k in names)
    assert any(launches == 2 for _, launches in kinds) and any(k.startswith("window x6") for k in names)


def test_a_formula_off_by_one_tile_is_caught_by_the_sweep(pkg, lib):
    """The restatement with the window kernel's own rows one 16-row tile too many (window_kernel_fits only): the sweep must
    disagree with the library somewhere -- at the least where keep-in-LDS stops fitting, which no other word follows."""
    _, bad, _ = _sweep(pkg, lib, (32,), ow_tiles_off=1)
    assert bad
    assert any(got[1]["window"] == want[1]["window"] and got[1]["keep"] != want[1]["keep"] for _, got, want in bad)
