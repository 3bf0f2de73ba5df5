"""The row copy of the staging launches (csrc/k_stage.hip), pinned where a scalar-head / ``float4``-body / scalar-tail copy can
go wrong: graphs shorter than the head, an empty vector body, no tail, odd graph sizes (source row and destination graph on
another 16-byte phase from graph to graph), every phase of source, destination and second destination, one graph long enough
for the vector loop to stride more than once (and for the sampler's radix path to run beside the copy).  The payload holds a
NaN with a payload, -0.0, a denormal and +-inf, and everything is compared as ``int32``: a copy is a copy.  Canaries directly
around every destination and around the mask must survive.

The mask is compared only where it is ``gatres_mask_generate``'s by contract (no required nodes, layout share 0); the required
and layout masks have their own tests (test_gpu_eval_device.py, test_gpu_sensor_layout.py); what the sampler itself must output is
restated on the host in tests/sampler_ref.py, and test_gpu_mask_sampler.py holds every launch of it to that, byte for byte."""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S, SEED, STEP = 5, 4321, 6
SMALL_N = (1, 2, 3, 4, 5, 7, 8, 13)
BIG_N = 16397                                   # > 4 * MASK_WGS * 1024 floats: a second trip of the vector loop; > 2048: radix path
ROWS = {1: [3], 2: [3, 3], 3: [4, 1, 4]}        # permuted, one row named twice
SPECIAL = (0x7FC12345, -0x80000000, 0x00000001, 0x7F800000, -0x00800000)    # NaN + payload, -0.0, denormal, +inf, -inf
CANARY_F, CANARY_B, GUARD = 0x5A5AA5A5, 0xC3, 8
Y_MODES = ("none", "same", "other", "apart")    # no y; y_dst is x_dst; its own buffer on another phase; ... on x_dst's phase
VARIANTS = ("rows", "required0", "required1", "sensors1", "sensors0")


def _i32(v):
    return v - (1 << 32) if v >= (1 << 31) else v


def _source(N, phase, seed=0):
    """A contiguous [S, N] matrix that starts `phase` floats into a flat buffer, as int32 bits; every row holds the specials."""
    rng = np.random.default_rng(1000 * N + seed)
    flat = rng.standard_normal(3 + S * N + 3).astype(np.float32).view(np.int32).copy()
    m = flat[phase:phase + S * N].reshape(S, N)
    for r in range(S):
        for j in range(min(N, len(SPECIAL))):
            m[r, (3 * r + j) % N] = SPECIAL[(r + j) % len(SPECIAL)]
    flat = torch.from_numpy(flat).to(DEV)
    return flat, flat.data_ptr() + 4 * phase, flat[phase:phase + S * N].view(S, N)


_SOURCES = {}


def source(N, phase, seed=0):
    key = (N, phase, seed)
    if key not in _SOURCES:
        _SOURCES[key] = _source(N, phase, seed)
    return _SOURCES[key]


class Dest:
    """n elements that start `phase` elements behind GUARD canaries in a fresh buffer, with GUARD canaries behind them."""

    def __init__(self, n, phase, dtype=torch.int32, canary=_i32(CANARY_F)):
        self.n, self.lo, self.canary = n, GUARD + phase, canary
        self.buf = torch.full((GUARD + phase + n + GUARD,), canary, dtype=dtype, device=DEV)
        self.ptr = self.buf.data_ptr() + self.lo * self.buf.element_size()

    @property
    def body(self):
        return self.buf[self.lo:self.lo + self.n]

    def intact(self):
        return bool(self.buf[:self.lo].eq(self.canary).all()) and bool(self.buf[self.lo + self.n:].eq(self.canary).all())


def dests(n, xphase, ymode):
    x = Dest(n, xphase)
    y = {"none": None, "same": x, "other": Dest(n, (xphase + 1) % 4), "apart": Dest(n, xphase)}[ymode]
    return x, y


def node_ptr_of(sizes):
    return torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32, device=DEV)


_MASKS = {}


def sampler_mask(lib, sizes, rate):
    """gatres_mask_generate's mask for these graphs at (rate, SEED, STEP): computed once, never written again."""
    key = (tuple(sizes), rate)
    if key not in _MASKS:
        m = torch.empty(sum(sizes), dtype=torch.uint8, device=DEV)
        ctr = torch.tensor([STEP], dtype=torch.int64, device=DEV)
        assert lib.gatres_mask_generate(node_ptr_of(sizes).data_ptr(), len(sizes), rate, SEED, ctr.data_ptr(), m.data_ptr(), None) == 0
        torch.cuda.synchronize()
        _MASKS[key] = m
    return _MASKS[key]


def launch_single(lib, variant, N, G, rate, data_ptr, rows, x, y, mask, node_ptr, ctr, aux):
    yp = None if y is None else y.ptr
    head = (data_ptr, rows.data_ptr(), N, x.ptr, yp, node_ptr.data_ptr(), G)
    if variant == "rows":
        return lib.gatres_stage_rows_mask(*head, rate, SEED, ctr.data_ptr(), mask.ptr, None)
    if variant.startswith("required"):
        r = int(variant[-1])
        return lib.gatres_stage_rows_mask_required(*head, rate, SEED, ctr.data_ptr(), aux.data_ptr() if r else None, r, mask.ptr, None)
    share = float(variant[-1])
    return lib.gatres_stage_rows_mask_sensors(*head, aux.data_ptr(), aux.numel(), 0.0, share, rate, SEED, ctr.data_ptr(), mask.ptr, None)


def single_cases():
    for variant in VARIANTS:
        for N in SMALL_N + (BIG_N,):
            if variant == "required1" and N == 1:
                continue            # (one node: int(N * rate) - 1 <= 0 at every rate, the wrapper refuses; test_return_codes)
            for G in ((2,) if N == BIG_N else (1, 3)):
                yield pytest.param(variant, N, G, id=f"{variant}-{N}x{G}")


@pytest.mark.parametrize("variant,N,G", list(single_cases()))
def test_single_matrix_collation_is_a_copy(lib, variant, N, G):
    # required1: the last node of every graph is required; the wrapper wants int(N * rate) - 1 > 0, which 0.75 gives from N = 3 on
    rate = 1.0 if variant == "required1" and N < 3 else 0.75
    rows = torch.tensor(ROWS[G], dtype=torch.int64, device=DEV)
    node_ptr = node_ptr_of([N] * G)
    ctr = torch.tensor([STEP], dtype=torch.int64, device=DEV)
    if variant.startswith("sensors"):
        aux = torch.tensor(sorted({0, N - 1}), dtype=torch.int32, device=DEV)
    else:
        aux = torch.tensor([N - 1], dtype=torch.int32, device=DEV)
    mask_is_the_samplers = variant in ("rows", "required0", "sensors0")
    for sphase, xphase, ymode in itertools.product(range(4), range(4), Y_MODES):
        _, data_ptr, data = source(N, sphase)
        want = data[rows].reshape(-1)
        x, y = dests(G * N, xphase, ymode)
        mask = Dest(G * N, 0, torch.uint8, CANARY_B)
        assert launch_single(lib, variant, N, G, rate, data_ptr, rows, x, y, mask, node_ptr, ctr, aux) == 0
        torch.cuda.synchronize()
        where = (sphase, xphase, ymode)
        assert torch.equal(x.body, want), where
        assert x.intact(), where
        if y is not None:
            assert torch.equal(y.body, want) and y.intact(), where
        assert mask.intact(), where
        if mask_is_the_samplers:
            assert torch.equal(mask.body, sampler_mask(lib, [N] * G, rate)), where
        else:
            assert bool(mask.body.le(1).all()), where                  # (written everywhere: no canary byte left)


# ---- several snapshot matrices: two networks of 5 and 8 nodes in one batch of 3 graphs -----------------------------------------
NET_N, NET_OF_GRAPH, MULTI_ROWS = (5, 8), (0, 1, 0), (4, 1, 4)
MULTI_SIZES = [NET_N[k] for k in NET_OF_GRAPH]


def multi_sources(sphase):
    srcs = [source(n, (sphase + k) % 4, seed=7 + k) for k, n in enumerate(NET_N)]
    table = torch.tensor([s[1] for s in srcs], dtype=torch.int64, device=DEV)
    return table, [s[2] for s in srcs]


@pytest.mark.parametrize("required", [False, True])
def test_multi_network_collation_is_a_copy(lib, required):
    rate, n = 0.75, sum(MULTI_SIZES)
    nog = torch.tensor(NET_OF_GRAPH, dtype=torch.int32, device=DEV)
    rows = torch.tensor(MULTI_ROWS, dtype=torch.int64, device=DEV)
    node_ptr = node_ptr_of(MULTI_SIZES)
    ctr = torch.tensor([STEP], dtype=torch.int64, device=DEV)
    req_ptr = torch.tensor([0, 1, 2], dtype=torch.int32, device=DEV) if required else None        # one sensor per network:
    req_idx = torch.tensor([4, 7], dtype=torch.int32, device=DEV) if required else None            # its last node
    for sphase, xphase, ymode in itertools.product(range(4), range(4), Y_MODES):
        table, mats = multi_sources(sphase)
        want = torch.cat([mats[k][r] for k, r in zip(NET_OF_GRAPH, MULTI_ROWS)])
        x, y = dests(n, xphase, ymode)
        mask = Dest(n, 0, torch.uint8, CANARY_B)
        assert lib.gatres_stage_multi_rows_mask_required(
            table.data_ptr(), len(NET_N), nog.data_ptr(), rows.data_ptr(), node_ptr.data_ptr(), len(MULTI_SIZES), x.ptr,
            None if y is None else y.ptr, rate, SEED, ctr.data_ptr(), None if req_ptr is None else req_ptr.data_ptr(),
            None if req_idx is None else req_idx.data_ptr(), mask.ptr, None) == 0
        torch.cuda.synchronize()
        where = (sphase, xphase, ymode)
        assert torch.equal(x.body, want) and x.intact(), where
        if y is not None:
            assert torch.equal(y.body, want) and y.intact(), where
        assert mask.intact(), where
        if required:
            assert bool(mask.body.le(1).all()), where
        else:
            assert torch.equal(mask.body, sampler_mask(lib, MULTI_SIZES, rate)), where


def test_multi_network_gather_is_a_copy(lib):
    n, batches, gap = sum(MULTI_SIZES), 2, 3
    stride = n + gap                                   # (not a multiple of four: the second batch lies on another phase)
    nog = torch.tensor(NET_OF_GRAPH, dtype=torch.int32, device=DEV)
    rows_host = [MULTI_ROWS, (0, 3, 2)]
    rows = torch.tensor(rows_host, dtype=torch.int64, device=DEV).reshape(-1)
    node_ptr = node_ptr_of(MULTI_SIZES)
    for sphase, xphase in itertools.product(range(4), range(4)):
        table, mats = multi_sources(sphase)
        dst = Dest(batches * stride - gap, xphase)
        assert lib.gatres_gather_multi_rows(table.data_ptr(), len(NET_N), nog.data_ptr(), rows.data_ptr(), node_ptr.data_ptr(),
                                            len(MULTI_SIZES), batches, dst.ptr, stride, None) == 0
        torch.cuda.synchronize()
        where = (sphase, xphase)
        for b in range(batches):
            want = torch.cat([mats[k][r] for k, r in zip(NET_OF_GRAPH, rows_host[b])])
            assert torch.equal(dst.body[b * stride:b * stride + n], want), where
        assert bool(dst.body[n:stride].eq(dst.canary).all()) and dst.intact(), where           # the gap between the batches too


# ---- what the wrappers refuse ----------------------------------------------------------------------------------------------------
def refused(fn, ok, bad):
    assert fn(*ok) == 0
    for i, v in bad:
        args = list(ok)
        args[i] = v
        assert fn(*args) == -1, (fn.__name__, i, v)


def test_return_codes(lib):
    N, G, n = 8, 3, 24
    _, data_ptr, _ = source(N, 0)
    rows = torch.tensor(ROWS[G], dtype=torch.int64, device=DEV)
    x, y, x2 = (torch.zeros(n + 4, device=DEV) for _ in range(3))
    mask = torch.zeros(n, dtype=torch.uint8, device=DEV)
    ptr = node_ptr_of([N] * G)
    ctr = torch.tensor([STEP], dtype=torch.int64, device=DEV)
    idx = torch.tensor([0, 7], dtype=torch.int32, device=DEV)
    nan = float("nan")
    X, Y, R, P, M, C, I = x.data_ptr(), y.data_ptr(), rows.data_ptr(), ptr.data_ptr(), mask.data_ptr(), ctr.data_ptr(), idx.data_ptr()

    refused(lib.gatres_mask_generate, (P, G, 0.75, SEED, C, M, None),
            [(0, None), (5, None), (1, 0), (1, -1), (2, 1.5), (2, -0.1), (2, nan)])
    refused(lib.gatres_stage_batch_mask, (x2.data_ptr(), None, X, None, n, P, G, 0.75, SEED, C, M, None),
            [(5, None), (10, None), (6, 0), (7, 1.5), (7, -0.1), (7, nan), (0, None), (2, None), (4, 0), (1, Y), (3, Y)])
    common = [(5, None), (6, 0), (6, -1), (0, None), (1, None), (3, None), (2, 0), (0, X)]        # (0, X): data == x_dst
    refused(lib.gatres_stage_rows_mask, (data_ptr, R, N, X, Y, P, G, 0.75, SEED, C, M, None),
            common + [(10, None), (7, 1.5), (7, -0.1), (7, nan)])
    refused(lib.gatres_stage_rows_mask_required, (data_ptr, R, N, X, Y, P, G, 0.75, SEED, C, I, 2, M, None),
            common + [(12, None), (7, 1.5), (7, -0.1), (7, nan), (11, -1), (10, None), (11, 6), (7, 0.25)])   # int(N * rate) - r <= 0
    assert lib.gatres_stage_rows_mask_required(data_ptr, R, N, X, X, P, G, 0.75, SEED, C, None, 0, M, None) == 0
    refused(lib.gatres_stage_rows_mask_sensors, (data_ptr, R, N, X, Y, P, G, I, 2, 0.1, 0.7, 0.75, SEED, C, M, None),
            common + [(14, None), (11, 1.5), (11, -0.1), (11, nan), (7, None), (8, 0), (8, N + 1), (9, 1.0), (9, -0.1), (9, nan),
                      (10, 1.5), (10, -0.1), (10, nan)])

    table, _ = multi_sources(0)
    nog = torch.tensor(NET_OF_GRAPH, dtype=torch.int32, device=DEV)
    mptr = node_ptr_of(MULTI_SIZES)
    T, NG, MP = table.data_ptr(), nog.data_ptr(), mptr.data_ptr()
    refused(lib.gatres_stage_multi_rows_mask_required, (T, 2, NG, R, MP, 3, X, Y, 0.75, SEED, C, None, None, M, None),
            [(0, None), (1, 0), (2, None), (3, None), (4, None), (5, 0), (6, None), (13, None), (8, 1.5), (8, -0.1), (8, nan),
             (11, I), (12, I), (6, X + 2), (7, Y + 2)])            # (one of req_ptr / req_idx alone; a destination off 4 bytes)
    refused(lib.gatres_gather_multi_rows, (T, 2, NG, R, MP, 3, 1, X, sum(MULTI_SIZES), None),
            [(0, None), (1, 0), (2, None), (3, None), (4, None), (5, 0), (6, 0), (7, None), (8, 0), (7, X + 2)])
    # num_graphs * num_batches > 2^31 - 1
    assert lib.gatres_gather_multi_rows(T, 2, NG, R, MP, 1 << 16, 1 << 16, X, sum(MULTI_SIZES), None) == -1
    torch.cuda.synchronize()
