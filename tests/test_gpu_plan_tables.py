"""The window kernel on the plan's part tables (gatres_graph_part_tables_host, copied into LDS verbatim) against the same
kernel deriving its tables from the CSR arrays in every launch (GATRES_NO_PART_TABLES=1), beyond the 388-node network of
test_gpu_model.py::test_part_tables_equal_in_kernel_derivation: irregular snapshots with rows of 7 .. 33+ entries, a
directed plan with heartbeat hand-offs, the nc = 16 instantiation, and a ragged batch whose smallest segment has fewer
16-row tiles than parts.  Two training steps each way; out, loss, gradients and parameters must be the same bits."""
import numpy as np
import pytest
import torch

import irregular_graphs as IG
import plan_cases as PC
from test_gpu_model import build      # noqa: E402

pytestmark = pytest.mark.gpu


def _snap(name, bs=3):
    g = IG.named(name)
    return IG.collate(g, bs), [g.num_nodes] * bs


CASES = {
    # name: (graph, nc, GATRES_FUSED_SPLIT or None, workgroups per segment expected, GATRES_GRAPH_SYMMETRIC expected)
    "snap_sym_nc32_split4": (lambda: _snap("snap_sym"), 32, 4, 4, True),
    "snap_sym_nc32_split8": (lambda: _snap("snap_sym"), 32, 8, 8, True),
    "snap_dir_hub_nc32": (lambda: _snap("snap_dir_hub"), 32, None, 8, False),
    "snap_sym_nc16": (lambda: _snap("snap_sym"), 16, None, 8, True),
    "ragged_17_130_389_nc32": (PC.ragged_batch, 32, None, 8, True),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_window_kernel_on_part_tables_equals_in_kernel_derivation(pkg, oracle, case, monkeypatch):
    graph, nc, split, parts, symmetric = CASES[case]
    nb = 2
    ei, npg = graph()
    N = int(sum(npg))
    if split is not None:
        monkeypatch.setenv("GATRES_FUSED_SPLIT", str(split))
    gen = torch.Generator().manual_seed(len(case))
    ys = [torch.randn(N, 1, generator=gen) for _ in range(2)]
    masks = [torch.from_numpy(pkg.wdn_synth.generate_batch_mask(npg, 0.95, np.random.RandomState(9 + k))) for k in range(2)]
    lib = pkg._native.load()
    res = []
    for no_tables in (False, True):
        if no_tables:
            monkeypatch.setenv("GATRES_NO_PART_TABLES", "1")
        model, _ = build(pkg, oracle, nb, nc, seed=5, fused=True)
        tr = pkg.GATResTrainer(model, ei.cuda(), N, nodes_per_graph=npg, use_graph=False)
        assert tr.fused and bool(tr.plan.flags & 1) == symmetric
        # which split and which kernel: the window kernel, `parts` workgroups per segment, with and without the tables
        assert int(lib.gatres_fused_cus_per_segment(model._cmodel_ref(), tr.plan.ref())) == parts
        assert int(lib.gatres_fused_window_kernel(model._cmodel_ref(), tr.plan.ref())) == 1
        assert bool(tr._gstruct.part_tables) == (not no_tables) and not tr.plan.c.part_tables
        if not no_tables:
            assert tr._gstruct.part_tables_m == parts and tr._gstruct.part_tables_stride % 4 == 0
        out = []
        for it in range(2):
            loss = tr.step(ys[it].cuda(), ys[it].cuda(), masks[it].cuda())
            out.append((tr.out.clone(), loss.clone(), tr.grads.clone(), model.flat_parameters.clone()))
        assert tr.fault_count == 0
        res.append(out)
    for a, b in zip(res[0], res[1]):
        for u, v in zip(a, b):
            assert torch.isfinite(u).all() and torch.equal(u, v)
    if case.startswith("ragged"):
        assert (min(npg) + 15) // 16 < parts          # (a segment with fewer 16-row tiles than parts: empty parts in the launch)
