"""Diagnostic fuzzer (not collected by pytest): random batches of random graphs -- directed / undirected edges, degrees
beyond the slot paths' 6, isolated nodes, self loops, ragged sizes, local and shuffled node orders -- through the fused
kernels (whichever of window / whole-segment / split the plan selects) against the per-op kernels.
    python tests/micro/fuzz_fused.py [cases] [seed] [max segments + 1 = 9] [min segments = 1]     (GATRES_FUSED_SPLIT etc. apply;
    49 .. 96 segments exercise the two-round launches)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch
import gnn_pressure_estimation_amd as G
from tests import irregular_graphs as IG

cases = int(sys.argv[1]) if len(sys.argv) > 1 else 30
rng = np.random.RandomState(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
seg_hi = int(sys.argv[3]) if len(sys.argv) > 3 else 9
seg_lo = int(sys.argv[4]) if len(sys.argv) > 4 else 1


def random_graph(n):
    return IG.random_graph(rng, n, G.wdn_synth.make_wdn_topology)


def relerr(a, b):
    return float((a.double() - b.double()).abs().max() / max(float(b.double().abs().max()), 1e-30))


bad = 0
for case in range(cases):
    nb, nc = int(rng.choice([1, 2, 3])), int(rng.choice([8, 16, 32, 32, 32]))
    sizes = [int(rng.choice([17, 33, 60, 120, 200, 388, 388, 450])) for _ in range(rng.randint(seg_lo, seg_hi))]
    tops = [random_graph(n) for n in sizes]
    offs = np.cumsum([0] + sizes)
    ei = torch.cat([t + int(o) for t, o in zip(tops, offs[:-1])], dim=1)
    N = int(offs[-1])
    torch.manual_seed(case)
    mf = G.GATResMeanConv(num_blocks=nb, nc=nc, fused=True).cuda()
    mp = G.GATResMeanConv(num_blocks=nb, nc=nc, fused=False).cuda()
    with torch.no_grad():
        mp.flat_parameters.copy_(mf.flat_parameters)
    x = torch.randn(N, 1).cuda()
    dei = ei.cuda()
    hubs = int(torch.bincount(ei[1][ei[0] != ei[1]], minlength=N).max()) + 1 > 32
    ok = True
    for rep in range(2):
        of, op = mf(x, dei), mp(x, dei)
        # bit-identical predictions, except on batches with hub rows (more than 32 in-edges): the per-op kernels reduce those
        # by the whole wave with staged partial sums, the fused kernels edge after edge (fp32 reassociation only)
        if not (torch.equal(of, op) or (hubs and relerr(of, op) < 1e-6)):
            ok = False; print("case", case, "rep", rep, "FORWARD differs", relerr(of, op))
        g = torch.randn_like(of)
        mf.zero_grad(); mp.zero_grad()
        of.backward(g); op.backward(g)
        gf = torch.cat([q.grad.reshape(-1) for q in mf.parameters()])
        gp = torch.cat([q.grad.reshape(-1) for q in mp.parameters()])
        e = relerr(gf, gp)
        if not (e < 5e-5) or not torch.isfinite(gf).all():
            ok = False; print("case", case, "rep", rep, "GRADS differ", e)
    plan = mf._plans.get(dei, N)
    lib = G._native.load()
    cus = lib.gatres_fused_cus_per_segment(mf._cmodel_ref(), plan.ref())
    print(f"case {case:3d} nb {nb} nc {nc:2d} sizes {sizes if len(sizes) < 10 else str(sizes[:6])[:-1] + ', ...]'} segments {plan.num_segments} CUs/segment {cus} windows {plan.windows[3:6]}"
          f" -> {'ok' if ok else 'FAIL'}{' (hub rows: last-bit forward differences allowed)' if hubs else ''}")
    bad += 0 if ok else 1
print("failures:", bad, "of", cases)
sys.exit(1 if bad else 0)
