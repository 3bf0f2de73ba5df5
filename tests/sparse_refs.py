"""Plain fp64 statements of the sparse kernels (torch CPU, no autograd), each with its `abs` twin -- the same operation on
absolute values, which bounds fp32 summation error under cancellation -- and the element-wise judge the bf16 kernel tests
use.  Row conventions of the graph plan (include/gatres.h): GATConv edges = the edges without self loops plus one self loop
per node, alpha / g_e stored in destination-sorted (stable) order; SimpleConv edges = edge_index as it is."""
import torch

from oracle import gatres_oracle as O


def gat_edges(ei, n):
    """(src, dst) of GATConv's edge list in the plan's destination-sorted order."""
    eg = O.add_self_loops(O.remove_self_loops(ei), n)
    order = torch.sort(eg[1], stable=True).indices
    return eg[0][order], eg[1][order]


def _sum_to(idx, vals, n):
    return torch.zeros((n,) + vals.shape[1:], dtype=vals.dtype).index_add_(0, idx, vals)


def gat_aggregate_fwd(src, dst, h, a_s, a_d, bias, n, H, relu):
    """out = [relu](sum_e alpha_e h[src_e] + bias), alpha = softmax over each destination's edges of leaky(a_s + a_d)."""
    h, a_s, a_d, bias = (t.double() for t in (h, a_s, a_d, bias))
    C = h.shape[1] // H
    s = torch.nn.functional.leaky_relu(a_s[src] + a_d[dst], O.NEG_SLOPE)
    alpha = O.segment_softmax(s, dst, n)                                        # [E', H]
    hv = h.view(n, H, C)
    pre = _sum_to(dst, alpha[..., None] * hv[src], n).reshape(n, H * C) + bias
    pre_abs = _sum_to(dst, alpha[..., None] * hv[src].abs(), n).reshape(n, H * C) + bias.abs()
    return (pre.relu() if relu else pre), pre_abs, alpha


def gat_aggregate_bwd_dst(src, dst, g_out, h, alpha, a_s, a_d, n, H):
    """g_e = d loss / d (a_s[src] + a_d[dst]) through the softmax and LeakyReLU, g_a_dst = its sum per destination."""
    g_out, h, alpha, a_s, a_d = (t.double() for t in (g_out, h, alpha, a_s, a_d))
    C = h.shape[1] // H
    go, hv = g_out.view(n, H, C)[dst], h.view(n, H, C)[src]
    ga, ga_abs = (go * hv).sum(-1), (go * hv).abs().sum(-1)                      # d loss / d alpha  [E', H]
    dot = _sum_to(dst, alpha * ga, n)[dst]
    dot_abs = _sum_to(dst, alpha * ga_abs, n)[dst]
    slope = torch.where(a_s[src] + a_d[dst] > 0, torch.ones((), dtype=torch.float64),
                        torch.full((), O.NEG_SLOPE, dtype=torch.float64))
    g_e = alpha * (ga - dot) * slope
    g_e_abs = alpha * (ga_abs + dot_abs) * slope
    return g_e, g_e_abs, _sum_to(dst, g_e, n), _sum_to(dst, g_e_abs, n)


def gat_aggregate_bwd_src(src, dst, g_out, alpha, g_e, g_a_dst, att_s, att_d, n, H):
    """g_a_src[j] = sum of g_e over j's out-edges; g_h[j] = sum alpha_e g_out[dst_e] + g_a_src[j] att_s + g_a_dst[j] att_d."""
    g_out, alpha, g_e, g_a_dst, att_s, att_d = (t.double() for t in (g_out, alpha, g_e, g_a_dst, att_s, att_d))
    C = g_out.shape[1] // H
    g_as, g_as_abs = _sum_to(src, g_e, n), _sum_to(src, g_e.abs(), n)
    go = g_out.view(n, H, C)[dst]
    msg, msg_abs = _sum_to(src, alpha[..., None] * go, n), _sum_to(src, alpha[..., None] * go.abs(), n)
    A, D = att_s.view(1, H, C), att_d.view(1, H, C)
    g_h = msg + g_as[..., None] * A + g_a_dst[..., None] * D
    g_h_abs = msg_abs + g_as_abs[..., None] * A.abs() + g_a_dst.abs()[..., None] * D.abs()
    return g_h.reshape(n, H * C), g_h_abs.reshape(n, H * C), g_as, g_as_abs


def mean_residual_relu(ei, y, x0, n):
    y, x0 = y.double(), x0.double()
    pre = O.simple_conv_mean(y, ei) + x0
    return pre.relu(), O.simple_conv_mean(y.abs(), ei) + x0.abs()


def mean_bwd(ei, g_pre, n):
    """g_y[j] = sum over j's out-edges (j -> i) of g_pre[i] / max(indeg(i), 1)."""
    g_pre = g_pre.double()
    src, dst = ei[0], ei[1]
    cnt = torch.bincount(dst, minlength=n).clamp(min=1).double()[:, None]
    return _sum_to(src, (g_pre / cnt)[dst], n), _sum_to(src, (g_pre.abs() / cnt)[dst], n)


def excess(got, ref, ref_abs, rel):
    """The c a comparison needs: max over elements of (|got - ref| - rel |ref|) / ref_abs, floored at 0 (the judge
    below passes iff this is <= c)."""
    got, ref, ref_abs = got.detach().double().cpu(), ref.double(), ref_abs.double()
    e = ((got - ref).abs() - rel * ref.abs()).clamp(min=0) / ref_abs.clamp(min=1e-300)
    return float(e.max()) if e.numel() else 0.0


def assert_within(what, got, ref, ref_abs, rel, c):
    """|got - ref| <= rel |ref| + c ref_abs, element by element (rel = 2^-8 for bf16 stores, 0 for fp32 results)."""
    got, ref, ref_abs = got.detach().double().cpu(), ref.double(), ref_abs.double()
    bad = (got - ref).abs() > rel * ref.abs() + c * ref_abs
    assert torch.isfinite(got).all(), what
    if bad.any():
        i = int(bad.reshape(-1).nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements off, first at flat index {i}: "
                             f"got {float(got.reshape(-1)[i])} ref {float(ref.reshape(-1)[i])} "
                             f"(|ref| sum {float(ref_abs.reshape(-1)[i])}); needs c = {excess(got, ref, ref_abs, rel):.3g}")
