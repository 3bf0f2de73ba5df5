"""The device mask sampler (csrc/k_mask.h: ``mask_sample_graph``) restated on the host in plain Python integers.

The sampler is integer arithmetic modulo 2^64 and one double product, so this restatement is exact: the GPU tests
(test_gpu_mask_sampler.py) demand equal bytes from every launch that instantiates the sampler, and the properties of the
distribution are tested on this file alone (test_sampler_ref_host.py).  Nothing here is shared with the package:
``sensor_layout._mix64`` is a second, independent statement of the hash, and the two are compared in the host test.

The contract (the comment block of k_mask.h and the sampler section of include/gatres.h): node ``v`` of graph ``g`` has the key
``hash32(seed, step, node_ptr[g] + v) << 32 | v`` -- unique inside a graph --, a required node has the bare key ``v``, and the
``k = int(n * rate)`` smallest keys of a graph are masked."""
import numpy as np

M64 = (1 << 64) - 1
GOLDEN, NODE = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9


def mix64(z):
    """The finaliser of splitmix64 (csrc/gatres_common.h: mix64)."""
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return (z ^ (z >> 31)) & M64


def mask_key(seed, step, gnode, local):
    """The key of the node at batch position ``gnode`` that is node ``local`` of its graph."""
    z = mix64(((seed & M64) + GOLDEN * (((step & M64) + 1) & M64) + NODE * ((gnode + 1) & M64)) & M64)
    return (((z >> 32) << 32) | (local & 0xFFFFFFFF)) & M64


def graph_keys(seed, step, n0, n, required=()):
    """The ``n`` keys of a graph whose first node is at batch position ``n0``."""
    keys = [mask_key(seed, step, n0 + v, v) for v in range(n)]
    for v in required:
        if 0 <= v < n:
            keys[v] = v
    return keys


def mask_count(n, rate):
    """``int(n * rate)``: the kernel's ``(int)((double)n * rate)``, the same double product and truncation."""
    return int(n * rate)


def sampler_mask(seed, step, sizes, rate, required=None):
    """The mask bytes of a batch of graphs of ``sizes`` nodes at sampler step ``step``.  ``required``: None, one list of local
    indices for every graph, or one list per graph (the multi-network launch)."""
    sizes = [int(n) for n in sizes]
    if required is None:
        per_graph = [()] * len(sizes)
    elif len(required) and isinstance(required[0], (list, tuple)):
        assert len(required) == len(sizes)
        per_graph = [tuple(r) for r in required]
    else:
        per_graph = [tuple(required)] * len(sizes)
    out = np.zeros(sum(sizes), dtype=np.uint8)
    n0 = 0
    for n, req in zip(sizes, per_graph):
        k = mask_count(n, rate)
        if k > 0:
            keys = graph_keys(seed, step, n0, n, req)
            for v in sorted(range(n), key=keys.__getitem__)[:k]:
                out[n0 + v] = 1
        n0 += n
    return out


def rate_for_count(n, k):
    """A rate with ``int(n * rate) == k`` (the middle of the interval of such rates), checked."""
    rate = (k + 0.5) / n
    assert 0.0 <= rate <= 1.0 and mask_count(n, rate) == k, (n, k, rate)
    return rate


# ---- graphs in which two nodes share the upper 32 key bits ---------------------------------------------------------------------
# The low 32 bits of a key are the node's local index, so the four low radix passes and the tie order of the all-pairs rank do
# real work only where two nodes of one graph share their upper 32 bits.  COLLISION_SEED and the table below name such graphs
# at batch position 0: {nodes: (step, the lower sorted rank of the pair, the pair's local indices in key order)}; the pair sits
# at ranks r and r + 1.  test_sampler_ref_host.py finds them again by search (collision_search) and asserts this table.
COLLISION_SEED = 4321
COLLISIONS = {
    16397: (2, 6251, (11622, 12849)),
    2048: (1640, 1313, (60, 1421)),
    2049: (1640, 1313, (60, 1421)),
}


def upper_halves(seed, step, n0, n):
    """numpy restatement of the keys' upper 32 bits for the nodes of one graph (the search only; uint64 arithmetic wraps)."""
    with np.errstate(over="ignore"):
        base = np.uint64(seed & M64) + np.uint64(GOLDEN) * np.uint64((step + 1) & M64)
        z = base + np.uint64(NODE) * (np.arange(n0 + 1, n0 + n + 1, dtype=np.uint64))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return z >> np.uint64(32)


def collision_search(seed, n, max_steps):
    """The first step in [0, max_steps) at which a graph of ``n`` nodes at batch position 0 holds two nodes with equal upper key
    halves: (step, lower sorted rank of the pair, (node of rank r, node of rank r + 1)); None if there is none."""
    for step in range(max_steps):
        hi = upper_halves(seed, step, 0, n)
        if np.unique(hi).size == n:
            continue
        order = np.argsort((hi << np.uint64(32)) | np.arange(n, dtype=np.uint64), kind="stable")
        s = hi[order]
        r = int(np.flatnonzero(s[1:] == s[:-1])[0])
        return step, r, (int(order[r]), int(order[r + 1]))
    return None


COLLISION_REQUIRED = [2048, 7, 2047, 1000, 0]      # for the 2049-node graph: unsorted, astride index 2048, neither node of the pair


def collision_required_rate(n, req):
    """(rate, rank) with the k-th key of the n-node collision graph under the required list ``req`` being the lower node of the
    colliding pair: the required nodes whose random keys lay above the pair now rank below it."""
    step, _, (a, b) = COLLISIONS[n]
    keys = graph_keys(COLLISION_SEED, step, 0, n, req)
    order = sorted(range(n), key=keys.__getitem__)
    r = order.index(a)
    assert order[r + 1] == b and a not in req and b not in req
    return rate_for_count(n, r + 1), r


# ---- the batch of the GPU tests --------------------------------------------------------------------------------------------------
# 64 -> 65: Q 1 -> 2; 960 -> 961: Q reaches its cap of 16; sizes below MASK_WGS (4) and MASK_WGS_UPDATE (16) and not divisible by
# them leave node ranges empty or ragged; 2048 -> 2049: the all-pairs rank hands over to the radix select; 16397 gives the
# radix histogram real counts.  One batch in a mixed order: node_ptr[g] is non-zero and unaligned for most graphs.
GPU_SIZES = [388, 1, 16397, 64, 2, 2049, 65, 3, 1025, 960, 4, 129, 2048, 5, 961, 15, 4097, 16, 1023, 17, 128, 63, 2047, 1024]
GPU_RATES = [0.0, 1.0, 0.95, 0.5, 0.29, 0.34, 1e-4]
GPU_SEED_STEPS = [(0, None), (4321, 6), (2 ** 64 - 1, 2 ** 63), (77, 2 ** 32 + 5)]      # None: a null step counter (step 0)
