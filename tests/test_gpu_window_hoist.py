"""The window kernel's per-row edge descriptors in registers (k_window.hip: HOIST; k_window_stages.h: the REG forms).

Instantiations that know "rows of at most six entries" (0x400), "part tables present" (0x800) and "parts of at most 64
rows" (0x1000) read a lane's descriptors once per phase and keep them in registers across the block loop; a lane's row is
lo + tid / 16 at conv1's width and lo + tid / 8 at conv2's, clamped to hi - 1.  Only where a descriptor comes from
changes, so every output must equal, BIT FOR BIT, what the same launch computes with the descriptors read from LDS in
every stage: GATRES_WINDOW_PH_MASK=4095 (the instantiation without 0x1000) and GATRES_WINDOW_RUNTIME_PHASES=1 (the
run-time-phases kernel).  As test_window_kernel_instantiations_are_bit_identical (test_gpu_headline.py), on topologies
where the lane-to-row map can go wrong:

  * 130 nodes: 9 row tiles over 8 parts -- seven parts of 16 rows and one of 18 (two tiles, the second holding 2 rows):
    at either width most waves hold no row, and the last wave that does holds clamped lanes;
  * 388 nodes, the headline shape: parts of 48 rows and one of 52, whose last tile holds 4 rows;
  * 512 nodes: every part owns exactly 64 rows, the edge of fact 0x1000 -- all 16 waves hold rows at conv1's width, waves
    0 .. 7 at conv2's.  (Found on the host side of an MI355X when this test was written: with 8 workgroups per snapshot
    every topology of 497 .. 512 nodes takes the window kernel and has 64-row parts; 512 is the largest.)
  * the 388-node topology with its edge list edited: one node is given a fifth pipe (with the self loop its GATConv row
    uses all six slots) and one node loses all of its pipes (its SimpleConv row is empty: the descriptor lists the row
    itself, and the mean divides by max(0, 1)).

Every case asserts that the window kernel was taken and that the plan carries the three facts."""
import numpy as np
import pytest
import torch

from test_gpu_model import build

pytestmark = pytest.mark.gpu
NB, NC = 2, 32


def _topology(pkg, nodes):
    return pkg.wdn_synth.make_wdn_topology(nodes, int(round(nodes * 430 / 388)), seed=0)


def _edited(pkg, nodes):
    """The topology with one node of degree 5 (made so if there is none) and one node without any pipe."""
    ei = _topology(pkg, nodes)
    pairs = {(int(u), int(v)) for u, v in ei.t().tolist()}
    deg = np.bincount(ei[0].numpy(), minlength=nodes)
    full = int(np.argmax(deg))
    while deg[full] < 5:                                   # a near-by node that can take one more pipe
        v = next(v for v in range(max(0, full - 24), min(nodes, full + 25))
                 if v != full and deg[v] < 5 and (full, v) not in pairs)
        pairs |= {(full, v), (v, full)}
        deg[full] += 1
        deg[v] += 1
    nbrs_of_full = {v for u, v in pairs if u == full}
    lone = min((v for v in range(16, nodes - 16) if v != full and v not in nbrs_of_full), key=lambda v: deg[v])
    pairs = {(u, v) for u, v in pairs if u != lone and v != lone}
    order = sorted(pairs)                                  # grouped by source node, as make_wdn_topology's lists are
    out = torch.tensor(order, dtype=torch.int64).t().contiguous()
    d = np.bincount(out[0].numpy(), minlength=nodes)
    assert d.max() == 5 and d[full] == 5 and d[lone] == 0
    return out


CASES = [("130", 130, False, 3), ("388", 388, False, 2), ("512", 512, False, 2), ("388-edited", 388, True, 4)]


@pytest.mark.parametrize("name,nodes,edited,bs", CASES, ids=[c[0] for c in CASES])
def test_register_descriptors_are_bit_identical(pkg, oracle, lib, monkeypatch, name, nodes, edited, bs):
    ei1 = _edited(pkg, nodes) if edited else _topology(pkg, nodes)
    ei = pkg.wdn_synth.collate_edge_index(ei1, nodes, bs).cuda()
    y = pkg.wdn_synth.collate_snapshots(pkg.wdn_synth.make_snapshots(bs, nodes, seed=9), range(bs)).cuda()
    mask = torch.from_numpy(pkg.wdn_synth.generate_batch_mask([nodes] * bs, 0.95, np.random.RandomState(4))).cuda()
    parts = None

    def run(env):
        nonlocal parts
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        model, _ = build(pkg, oracle, NB, NC, seed=13)
        tr = pkg.GATResTrainer(model, ei, nodes * bs, nodes_per_graph=[nodes] * bs, use_graph=False)
        cm, plan = model._cmodel_ref(), tr.plan
        # the window kernel, and the three facts its launches will carry (k_fused_host.hip: a.facts, a.ptab)
        assert lib.gatres_fused_window_kernel(cm, plan.ref()) == 1
        m = lib.gatres_fused_cus_per_segment(cm, plan.ref())
        assert plan.num_segments == bs and plan.max_segment_nodes == nodes
        assert plan.flags & 1 and plan.flags & 4, "a symmetric plan with rows of at most six entries (0x200, 0x400)"
        bound = plan.bound(cm)
        assert bound.part_tables and bound.part_tables_m == m, "part tables of this split (0x800)"
        tiles = (nodes + 15) // 16
        assert 16 * ((tiles + m - 1) // m) <= 64, "parts of at most 64 rows (0x1000)"
        parts = [min(nodes, 16 * (tiles * (p + 1) // m)) - 16 * (tiles * p // m) for p in range(m)]
        out = {}
        tr.step(y, y, mask)
        out["pred"], out["loss"], out["grads"] = tr.out.clone(), tr.loss.clone(), tr.grads.clone()
        tr.step(y, y, mask)
        out["params"] = model.flat_parameters.clone()
        with torch.no_grad():
            out["eval"] = model(y.reshape(-1, 1), ei).clone()                      # forward-only launch
        model.zero_grad()
        o = model(y.reshape(-1, 1), ei)                                            # the module's forward + backward launches
        (o * o).mean().backward()
        out["module_out"], out["module_grads"] = o.detach().clone(), model.flat_grad().clone()
        assert tr.fault_count == 0
        for k in env:
            monkeypatch.delenv(k)
        return out

    got = run({})                                          # the default instantiations: descriptors in registers
    if nodes == 130:
        assert sorted(set(parts)) == [16, 18], parts
    elif nodes == 388:
        assert max(parts) == 52 and 52 % 16 == 4, parts
    else:
        assert max(parts) == 64, parts
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), k
    for env in ({"GATRES_WINDOW_PH_MASK": "4095"}, {"GATRES_WINDOW_RUNTIME_PHASES": "1"}):
        ref = run(env)
        for k, v in ref.items():
            assert torch.equal(v, got[k]), (name, env, k)
