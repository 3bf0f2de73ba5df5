"""The window kernel's hand-off sweep slots in registers (k_window.hip: sF1 / sF2 / sF3; k_window_stages.h: xch_slot and
xch_import2_reg).

In the instantiations that know 0x400, 0x800 and 0x1000 (test_gpu_window_hoist.py) a lane takes the same access of the
part's import list in the first trip of every sweep of a phase.  What the generic sweep derives from the list for that trip
-- valid, first, the LDS index, the granule's byte offset -- is formed once per phase and kept in registers; trips beyond
the first run the generic body.  Nothing but where those values come from changes, so every output must equal, BIT FOR
BIT, what the same launch computes with the generic sweeps in every block: GATRES_WINDOW_PH_MASK=4095 (the instantiation
without 0x1000) and GATRES_WINDOW_RUNTIME_PHASES=1 (the run-time-phases kernel).  The forward's three sweeps carry slots;
the backward's were measured slower with them (profiles/window_sweep_hoist.txt) and keep the generic form, whose lists the
cases below pin all the same.

Accesses of one part's sweeps, from its record (plan_refs.part_record_ref, M = 8, the single-snapshot topology):
F1 33 F_HCNT, F2 17 F_HCNT, F3 16 F_HCNT, B1 16 B_HRCNT, B2 16 B_HRCNT + B_HECNT, B3 32 B_HRCNT + B_HECNT.  A trip is
1024 lanes (B2, swept by waves 8 .. 15 during the stage before it: 512).  Every case asserts the list lengths it is there for:

  * 130 nodes: F2 / F3 / B1 lists of 160 .. 459 accesses -- most waves hold no slot, the last one that does is partly filled;
  * 388 nodes, the headline shape: every list is one trip (F1 <= 858, B2 <= 444, B3 <= 860);
  * 512 nodes: parts of 64 rows, F1 <= 924, B3 <= 926;
  * 336 nodes, seed 4: the longest B2 list is exactly 512 accesses, the edge of the early sweep's trip;
  * 388 nodes with 21 pipes added between the own rows of parts 3 and 4 (24 rows of part 4 x the last 24 of part 3, node
    degree kept below 5): F_HCNT of the two parts becomes 35 and 32, so F1 (1155), B3 (1169) and B2 (609) need a second
    trip while the largest window stays at 92 rows;
  * 388 nodes relabelled at random (bench.py --shuffle-nodes): the plan is relabelled by RCM and its lists are others."""
import numpy as np
import pytest
import torch

from plan_refs import part_record_ref, part_rows, ref_plan
from test_gpu_model import build

pytestmark = pytest.mark.gpu
NB, NC, M = 2, 32, 8
SWEEPS = ("F1", "F2", "F3", "B1", "B2", "B3")


def _topology(pkg, nodes, seed=0):
    return pkg.wdn_synth.make_wdn_topology(nodes, int(round(nodes * 430 / 388)), seed=seed)


def _long_lists(pkg, nodes, rows=24):
    """The topology with pipes added across the border of parts 3 and 4: for a in the first ``rows`` own rows of part 4, one
    pipe to the first b among the last ``rows`` own rows of part 3 (from the border down) with both degrees below 4."""
    ei = _topology(pkg, nodes)
    pairs = {(int(u), int(v)) for u, v in ei.t().tolist()}
    deg = np.bincount(ei[0].numpy(), minlength=nodes)
    (_, hi3), (lo4, _) = part_rows(nodes, 3, M), part_rows(nodes, 4, M)
    added = 0
    for a in range(lo4, lo4 + rows):
        b = next((b for b in range(hi3 - 1, hi3 - 1 - rows, -1) if deg[a] < 4 and deg[b] < 4 and (a, b) not in pairs), None)
        if b is not None:
            pairs |= {(a, b), (b, a)}
            deg[a] += 1
            deg[b] += 1
            added += 1
    out = torch.tensor(sorted(pairs), dtype=torch.int64).t().contiguous()      # grouped by source node
    assert added == 21 and np.bincount(out[0].numpy(), minlength=nodes).max() == 5
    return out


def _sweep_lengths(ei1, nodes):
    """Per part: accesses of the six sweeps, and the rows of its window."""
    plan = ref_plan(ei1, nodes)
    out = []
    for p in range(M):
        r = part_record_ref(ei1, nodes, [0, nodes], 0, p, M, plan=plan)
        h, hr, he = r["F_HCNT"], r["B_HRCNT"], r["B_HECNT"]
        out.append(dict(F1=33 * h, F2=17 * h, F3=16 * h, B1=16 * hr, B2=16 * hr + he, B3=32 * hr + he,
                        window=r["WHI"] - r["WLO"], own=r["HI"] - r["LO"]))
    return out


def _most(lengths, key):
    return max(p[key] for p in lengths)


def _check_130(L):
    assert sorted({p["own"] for p in L}) == [16, 18]
    assert _most(L, "F1") <= 1024 and min(p["F3"] for p in L) < 192
    assert all(160 <= p[k] <= 459 for p in L for k in ("F2", "F3", "B1"))


def _check_388(L):
    assert (_most(L, "F1"), _most(L, "B2"), _most(L, "B3")) == (858, 444, 860)
    assert all(p[k] <= (512 if k == "B2" else 1024) for p in L for k in SWEEPS), "every list is one trip"


def _check_512(L):
    assert all(p["own"] == 64 for p in L)
    assert (_most(L, "F1"), _most(L, "B3")) == (924, 926) and _most(L, "B2") <= 512


def _check_336(L):
    assert _most(L, "B2") == 512 and _most(L, "F1") == 990 and _most(L, "B3") <= 1024


def _check_long(L):
    assert (_most(L, "F1"), _most(L, "B3"), _most(L, "B2")) == (1155, 1169, 609)
    assert _most(L, "F1") > 1024 and _most(L, "B3") > 1024 and _most(L, "B2") > 512 and _most(L, "window") <= 92


CASES = [("130", 130, 0, None, 3, _check_130), ("388", 388, 0, None, 2, _check_388), ("512", 512, 0, None, 2, _check_512),
         ("336-seed4", 336, 4, None, 2, _check_336), ("388-two-trips", 388, 0, "long", 2, _check_long),
         ("388-relabelled", 388, 0, "shuffle", 2, None)]


@pytest.mark.parametrize("name,nodes,seed,edit,bs,check", CASES, ids=[c[0] for c in CASES])
def test_sweep_slots_are_bit_identical(pkg, oracle, lib, monkeypatch, name, nodes, seed, edit, bs, check):
    if edit == "long":
        ei1 = _long_lists(pkg, nodes)
    else:
        ei1 = _topology(pkg, nodes, seed)
    if check is not None:
        check(_sweep_lengths(ei1, nodes))
    if edit == "shuffle":
        ei1 = torch.randperm(nodes, generator=torch.Generator().manual_seed(12345))[ei1]
    ei = pkg.wdn_synth.collate_edge_index(ei1, nodes, bs).cuda()
    y = pkg.wdn_synth.collate_snapshots(pkg.wdn_synth.make_snapshots(bs, nodes, seed=9), range(bs)).cuda()
    mask = torch.from_numpy(pkg.wdn_synth.generate_batch_mask([nodes] * bs, 0.95, np.random.RandomState(4))).cuda()
    plan_perm = None

    def run(env):
        nonlocal plan_perm
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        model, _ = build(pkg, oracle, NB, NC, seed=13)
        tr = pkg.GATResTrainer(model, ei, nodes * bs, nodes_per_graph=[nodes] * bs, use_graph=False)
        cm, plan = model._cmodel_ref(), tr.plan
        # the window kernel, and the facts its launches will carry (k_fused_host.hip: a.facts, a.ptab)
        assert lib.gatres_fused_window_kernel(cm, plan.ref()) == 1
        m = lib.gatres_fused_cus_per_segment(cm, plan.ref())
        assert m == M and plan.num_segments == bs and plan.max_segment_nodes == nodes
        assert plan.flags & 1 and plan.flags & 4, "a symmetric plan with rows of at most six entries (0x200, 0x400)"
        bound = plan.bound(cm)
        assert bound.part_tables and bound.part_tables_m == m, "part tables of this split (0x800)"
        tiles = (nodes + 15) // 16
        assert 16 * ((tiles + m - 1) // m) <= 64, "parts of at most 64 rows (0x1000)"
        plan_perm = plan.perm_host
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

    got = run({})                                          # the default instantiations: sweep slots in registers
    if plan_perm is not None:
        # the lists the kernel swept are those of the plan's own labelling (RCM) of a snapshot
        old2new = torch.empty(nodes, dtype=torch.int64)
        old2new[plan_perm[:nodes].long()] = torch.arange(nodes, dtype=torch.int64)
        L = _sweep_lengths(old2new[ei1], nodes)
        if edit == "shuffle":                              # other lists and windows than the unshuffled topology's
            L0 = _sweep_lengths(_topology(pkg, nodes, seed), nodes)
            assert [p["F1"] for p in L] != [p["F1"] for p in L0] and [p["window"] for p in L] != [p["window"] for p in L0]
        else:      # (130 nodes: the plan adopts RCM's labelling -- F1 165 .. 825, F3 80 .. 400 -- and the case's conditions hold there too)
            assert name == "130" and _most(L, "F1") <= 1024 and min(p["F3"] for p in L) < 192
        assert all(p[k] <= (512 if k == "B2" else 1024) for p in L for k in SWEEPS)
    else:
        assert edit != "shuffle", "the shuffled topology's plan is relabelled (RCM)"
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), k
    for env in ({"GATRES_WINDOW_PH_MASK": "4095"}, {"GATRES_WINDOW_RUNTIME_PHASES": "1"}):
        ref = run(env)
        for k, v in ref.items():
            assert torch.equal(v, got[k]), (name, env, k)
