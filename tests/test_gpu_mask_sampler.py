"""Every launch that instantiates the device mask sampler (csrc/k_mask.h: ``mask_sample_graph``) against its host restatement
(tests/sampler_ref.py), byte for byte: the sampler's own launch and the staging launches (``<1024, 4>``, with and without
required nodes, single- and multi-network, under a sensor layout's random mode) and the sampling tails of the three update
launches (``<256, 16>``: ``reduce_adam_kernel``, ``autoclip_adam_kernel`` and -- through the one-rank collective path --
``adam_kernel``).  The sampler is integer arithmetic, so every comparison is ``np.array_equal``; every mask the test owns lies
between guard bytes that must survive.  What the restatement itself must satisfy (exactly k, uniformity, the collision
constants) is tested on the CPU in test_sampler_ref_host.py, which also names the case here that each of six plausible edits
of the kernel's selection fails.

All sizes at which the sampler changes its plan go into ONE batch per launch (sampler_ref.GPU_SIZES, where they are
explained), so most graphs start at a non-zero, unaligned batch position and a test is a handful of launches."""
import numpy as np
import pytest
import torch

import sampler_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, CANARY = 16, 0xC3
SEED, STEP = 4321, 6


class Mask:
    """n mask bytes that start `phase` bytes behind GUARD canaries in a fresh buffer, with GUARD canaries behind them."""

    def __init__(self, n, phase=0):
        self.n, self.lo = n, GUARD + phase
        self.buf = torch.full((self.lo + n + GUARD,), CANARY, dtype=torch.uint8, device=DEV)
        self.ptr = self.buf.data_ptr() + self.lo

    def read(self):
        """The mask bytes on the host, after the guards were found intact."""
        torch.cuda.synchronize()
        b = self.buf.cpu().numpy()
        assert (b[:self.lo] == CANARY).all() and (b[self.lo + self.n:] == CANARY).all(), "guard bytes around the mask"
        return b[self.lo:self.lo + self.n]


def node_ptr_of(sizes):
    return torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32, device=DEV)


def counter(step):
    """A device step counter holding ``step`` as an unsigned 64-bit value (None: no counter, the launch reads step 0)."""
    if step is None:
        return None
    return torch.from_numpy(np.array([step, 0], dtype=np.uint64).view(np.int64)).to(DEV)


def cptr(ctr):
    return None if ctr is None else ctr.data_ptr()


def differing(got, want, sizes):
    """Which graphs differ (for the assertion message)."""
    off = np.concatenate([[0], np.cumsum(sizes)])
    return [(g, int(n)) for g, n in enumerate(sizes) if not np.array_equal(got[off[g]:off[g + 1]], want[off[g]:off[g + 1]])][:8]


_WANT = {}


def want_mask(seed, step, sizes, rate, required=None):
    """The restatement's mask, computed once per case and never written again."""
    key = (seed, step, tuple(sizes), rate, repr(required))
    if key not in _WANT:
        m = R.sampler_mask(seed, step or 0, sizes, rate, required)
        m.setflags(write=False)
        _WANT[key] = m
    return _WANT[key]


# ---- the sampler's own launch ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,step", R.GPU_SEED_STEPS, ids=lambda v: "null" if v is None else hex(v))
def test_mask_generate_equals_the_restatement(lib, seed, step):
    sizes = R.GPU_SIZES
    node_ptr, ctr = node_ptr_of(sizes), counter(step)
    for phase, rate in enumerate(R.GPU_RATES):
        mask = Mask(sum(sizes), phase % 4)
        assert lib.gatres_mask_generate(node_ptr.data_ptr(), len(sizes), rate, seed, cptr(ctr), mask.ptr, None) == 0
        got, want = mask.read(), want_mask(seed, step, sizes, rate)
        assert np.array_equal(got, want), (rate, differing(got, want, sizes))
    # 1e-4: no node of the small graphs and at least one of the large ones, in the same launch
    ks = [int(n * 1e-4) for n in sizes]
    assert min(ks) == 0 and max(ks) >= 1


@pytest.mark.parametrize("n", sorted(R.COLLISIONS))
def test_mask_generate_where_two_nodes_share_the_upper_key_half(lib, n):
    """The k-th key is the lower one of two keys that differ in their low 32 bits only: the four low radix passes (16397,
    2049 nodes) and the all-pairs rank's full-width comparison (2048 nodes) decide which of the two is masked."""
    step, r, (a, b) = R.COLLISIONS[n]
    sizes = [n, 5]                                           # the colliding graph first: its batch position is 0
    rate = R.rate_for_count(n, r + 1)
    mask, ctr = Mask(sum(sizes)), counter(step)
    assert lib.gatres_mask_generate(node_ptr_of(sizes).data_ptr(), 2, rate, R.COLLISION_SEED, ctr.data_ptr(), mask.ptr, None) == 0
    got, want = mask.read(), want_mask(R.COLLISION_SEED, step, sizes, rate)
    assert want[a] == 1 and want[b] == 0
    assert (got[a], got[b]) == (1, 0), (got[a], got[b])
    assert np.array_equal(got, want), differing(got, want, sizes)


# ---- the staging launches without a list -----------------------------------------------------------------------------------------
def test_stage_batch_mask_equals_the_restatement(lib):
    sizes = R.GPU_SIZES
    n = sum(sizes)
    src = torch.arange(n, dtype=torch.float32, device=DEV)
    node_ptr, ctr = node_ptr_of(sizes), counter(STEP)
    for rate in (0.95, 0.29):
        dst = torch.zeros(n, dtype=torch.float32, device=DEV)
        mask = Mask(n, 1)
        assert lib.gatres_stage_batch_mask(src.data_ptr(), None, dst.data_ptr(), None, n, node_ptr.data_ptr(), len(sizes), rate,
                                           SEED, ctr.data_ptr(), mask.ptr, None) == 0
        got, want = mask.read(), want_mask(SEED, STEP, sizes, rate)
        assert np.array_equal(got, want), (rate, differing(got, want, sizes))
        assert torch.equal(dst, src)


ROW_LAUNCHES = ("rows", "required_none", "sensors_share0")


def stage_rows(lib, launch, N, G, rate, seed, ctr, mask, required=None, observed=None, drop=0.0, share=0.0):
    """One collation of G rows of a [G + 2, N] matrix with the sampler behind it; returns nothing (the mask is the subject)."""
    data = torch.arange((G + 2) * N, dtype=torch.float32, device=DEV).reshape(G + 2, N)
    rows = torch.tensor([(g + 1) % (G + 2) for g in range(G)], dtype=torch.int64, device=DEV)
    x = torch.zeros(G * N, dtype=torch.float32, device=DEV)
    node_ptr = node_ptr_of([N] * G)
    head = (data.data_ptr(), rows.data_ptr(), N, x.data_ptr(), None, node_ptr.data_ptr(), G)
    if launch == "rows":
        rc = lib.gatres_stage_rows_mask(*head, rate, seed, cptr(ctr), mask.ptr, None)
    elif launch.startswith("required"):
        req = torch.tensor(required, dtype=torch.int32, device=DEV) if required else None
        rc = lib.gatres_stage_rows_mask_required(*head, rate, seed, cptr(ctr), None if req is None else req.data_ptr(),
                                                 len(required or ()), mask.ptr, None)
    else:
        obs = torch.tensor(observed, dtype=torch.int32, device=DEV)
        rc = lib.gatres_stage_rows_mask_sensors(*head, obs.data_ptr(), len(observed), drop, share, rate, seed, cptr(ctr), mask.ptr,
                                                None)
    assert rc == 0, (launch, N, rc)
    torch.cuda.synchronize()
    assert torch.equal(x, data[rows].reshape(-1))


@pytest.mark.parametrize("N", [5, 388, 2049])
@pytest.mark.parametrize("launch", ROW_LAUNCHES)
def test_row_staging_launches_equal_the_restatement(lib, launch, N):
    G, ctr = 3, counter(STEP)
    for rate in (0.95, 0.29):
        mask = Mask(G * N, 3)
        stage_rows(lib, launch, N, G, rate, SEED, ctr, mask, observed=[0, N - 1])
        got, want = mask.read(), want_mask(SEED, STEP, [N] * G, rate)
        assert np.array_equal(got, want), (rate, differing(got, want, [N] * G))


# ---- required nodes ----------------------------------------------------------------------------------------------------------------
def required_cases():
    for N in (388, 2049, 3000):
        yield pytest.param(N, [N // 3], 0.5, id=f"{N}-one")
        yield pytest.param(N, [0, N - 1], 0.5, id=f"{N}-ends")
        yield pytest.param(N, [N - 1, 3, N // 2, 0, 77, N - 2, 5], 0.29, id=f"{N}-unsorted")
        if N > 2048:
            yield pytest.param(N, [2046, 2048, 2047] + ([2049, 2050] if N > 2050 else []), 0.5, id=f"{N}-astride2048")
        # all but one of the masked nodes are required: exactly one random draw is left
        rate = 0.05 if N == 388 else 0.01
        k = int(N * rate)
        picks = [int(v) for v in np.random.RandomState(N).permutation(N)[:k - 1]]
        yield pytest.param(N, picks, rate, id=f"{N}-one-draw-left")


@pytest.mark.parametrize("N,required,rate", list(required_cases()))
def test_required_nodes_equal_the_restatement(lib, N, required, rate):
    G = 3
    assert len(set(required)) == len(required) < int(N * rate)
    mask = Mask(G * N, 2)
    stage_rows(lib, "required", N, G, rate, SEED, counter(STEP), mask, required=required)
    got, want = mask.read(), want_mask(SEED, STEP, [N] * G, rate, required)
    assert all(want[g * N + v] == 1 for g in range(G) for v in required)
    assert np.array_equal(got, want), differing(got, want, [N] * G)


def test_required_nodes_beside_a_colliding_pair(lib):
    """The 2049-node graph whose nodes 60 and 1421 share the upper key half, under a required list that holds neither: the
    required nodes whose random keys lay above the pair rank below it now, and the rate is derived for the shifted rank."""
    N, G = 2049, 2
    step, r, (a, b) = R.COLLISIONS[N]
    rate, r2 = R.collision_required_rate(N, R.COLLISION_REQUIRED)
    assert r2 > r
    mask = Mask(G * N)
    stage_rows(lib, "required", N, G, rate, R.COLLISION_SEED, counter(step), mask, required=R.COLLISION_REQUIRED)
    got, want = mask.read(), want_mask(R.COLLISION_SEED, step, [N] * G, rate, R.COLLISION_REQUIRED)
    assert want[a] == 1 and want[b] == 0 and (got[a], got[b]) == (1, 0)
    assert np.array_equal(got, want), differing(got, want, [N] * G)


# ---- several networks in one batch -------------------------------------------------------------------------------------------------
NET_N = (37, 388, 2100)
NET_OF_GRAPH = (2, 0, 1, 0, 2, 1, 0)                                   # interleaved
NET_REQUIRED = ([36, 0, 9], [], [2099, 5, 2048, 2047, 1000])           # per network; one of them empty


@pytest.mark.parametrize("with_lists", [True, False])
def test_multi_network_staging_equals_the_restatement(lib, with_lists):
    sizes = [NET_N[k] for k in NET_OF_GRAPH]
    n, rate = sum(sizes), 0.5
    mats = [torch.arange(3 * m, dtype=torch.float32, device=DEV).reshape(3, m) + 1000.0 * k for k, m in enumerate(NET_N)]
    table = torch.tensor([m.data_ptr() for m in mats], dtype=torch.int64, device=DEV)
    nog = torch.tensor(NET_OF_GRAPH, dtype=torch.int32, device=DEV)
    rows_host = [g % 3 for g in range(len(sizes))]
    rows = torch.tensor(rows_host, dtype=torch.int64, device=DEV)
    node_ptr, ctr = node_ptr_of(sizes), counter(STEP)
    x = torch.zeros(n, dtype=torch.float32, device=DEV)
    req_ptr = torch.tensor(np.concatenate([[0], np.cumsum([len(r) for r in NET_REQUIRED])]), dtype=torch.int32, device=DEV)
    req_idx = torch.tensor([v for r in NET_REQUIRED for v in r], dtype=torch.int32, device=DEV)
    mask = Mask(n, 1)
    assert lib.gatres_stage_multi_rows_mask_required(
        table.data_ptr(), len(NET_N), nog.data_ptr(), rows.data_ptr(), node_ptr.data_ptr(), len(sizes), x.data_ptr(), None, rate,
        SEED, ctr.data_ptr(), req_ptr.data_ptr() if with_lists else None, req_idx.data_ptr() if with_lists else None, mask.ptr,
        None) == 0
    required = [list(NET_REQUIRED[k]) for k in NET_OF_GRAPH] if with_lists else None
    got, want = mask.read(), want_mask(SEED, STEP, sizes, rate, required)
    assert np.array_equal(got, want), differing(got, want, sizes)
    assert torch.equal(x, torch.cat([mats[k][r] for k, r in zip(NET_OF_GRAPH, rows_host)]))
    if with_lists:
        assert not np.array_equal(want, want_mask(SEED, STEP, sizes, rate))


# ---- a sensor layout's random-mode graphs ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [388, 2049])
def test_random_mode_graphs_under_a_sensor_layout_equal_the_restatement(pkg, lib, N):
    """(the layout-mode graphs are test_gpu_sensor_layout.py's)"""
    G, rate, drop, share = 8, 0.95, 0.3, 0.5
    obs = [0, N // 2, N - 1]
    mode, _ = pkg.sensor_layout_draws(SEED, STEP, G, N, obs, drop, share)
    assert mode.any() and not mode.all()
    mask = Mask(G * N, 1)
    stage_rows(lib, "sensors", N, G, rate, SEED, counter(STEP), mask, observed=obs, drop=drop, share=share)
    got, want = mask.read().reshape(G, N), want_mask(SEED, STEP, [N] * G, rate).reshape(G, N)
    for g in range(G):
        if not mode[g]:
            assert np.array_equal(got[g], want[g]), g
        else:
            assert not np.array_equal(got[g], want[g]), g        # (a layout mask: every node but the kept sensors)


# ---- the update launches' sampling tails -------------------------------------------------------------------------------------------
# Uniform graphs of 9 nodes (fewer than MASK_WGS_UPDATE: most of a graph's 16 workgroups own no node), 388 (the workload's) and
# 2100 (the radix path), the smallest model whose parameter gradients fold into the update launch (nc 16, one block).
TAIL_GRAPHS = {9: (10, 3), 388: (430, 3), 2100: (2330, 2)}            # nodes: (pipes, graphs)
TAIL_VARIANTS = {"reduce_adam": {}, "autoclip_adam": dict(use_gradient_clipping=True, percentile=10.0),
                 "adam": dict(force_collective_path=True)}


@pytest.mark.parametrize("N", list(TAIL_GRAPHS))
@pytest.mark.parametrize("variant", list(TAIL_VARIANTS))
def test_update_launch_tails_equal_the_restatement(pkg, variant, N):
    """After every step ``tr.mask`` is the restatement's mask at the optimizer step count that step started from.  Step 0 and
    the step after the change of the mask rate are sampled by the sampler's own launch, the others by the tail of the update
    launch in front of them (asserted: the mask sampled ahead is current when the step begins)."""
    pipes, G = TAIL_GRAPHS[N]
    torch.manual_seed(3)
    model = pkg.GATResMeanConv(num_blocks=1, nc=16).to(DEV)
    ei = pkg.wdn_synth.collate_edge_index(pkg.wdn_synth.make_wdn_topology(N, pipes, seed=0), N, G).to(DEV)
    tr = pkg.GATResTrainer(model, ei, N * G, nodes_per_graph=[N] * G, seed=SEED, **TAIL_VARIANTS[variant])
    assert tr.fused and tr._mask_next and tr.seed == SEED
    assert tr.split == (variant == "adam") and (tr._clip is not None) == (variant == "autoclip_adam")
    x = pkg.wdn_synth.make_snapshots(G, N, seed=5).reshape(-1).to(DEV)
    tr.load_batch(x, x)              # (run_step: step(x, y) would stage the batch with the sampler's own launch at every step)
    ahead = []
    for i in range(5):
        if i == 3:
            tr.set_hparams(mask_rate=0.5)
        before = tr.optimizer_step
        assert before == i
        ahead.append(tr._mask_current())
        tr.run_step()
        torch.cuda.synchronize()
        got, want = tr.mask.cpu().numpy(), want_mask(SEED, before, [N] * G, tr.mask_rate)
        assert np.array_equal(got, want), (i, differing(got, want, [N] * G))
    assert ahead == [False, True, True, False, True]
    assert tr.optimizer_step == 5 and tr.fault_count == 0 and tr.dropped_steps == 0
