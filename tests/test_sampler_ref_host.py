"""The host restatement of the device mask sampler (tests/sampler_ref.py), tested on the CPU: known answers of the hash,
agreement with the package's own (independent) statement of it, the sampler's contract, the truncation of ``int(n * rate)``, the
distribution -- the device is shown equal to the restatement byte for byte in test_gpu_mask_sampler.py, so uniformity is
tested here at no GPU cost --, the graphs in which two nodes share the upper key half, and which of the GPU cases each of six
plausible edits of the kernel's selection would fail (on a numpy model of the kernel's algorithm, slices and radix passes)."""
import math

import numpy as np
import pytest

import sampler_ref as R

M64 = (1 << 64) - 1


# ---- known answers and the package's own statement --------------------------------------------------------------------------
def test_mix64_known_answers():
    # splitmix64's first two outputs for seed 0
    assert R.mix64(0x9E3779B97F4A7C15) == 0xE220A8397B1DCDAF
    assert R.mix64((2 * 0x9E3779B97F4A7C15) & M64) == 0x6E789E6AA1B965F4
    assert R.mix64(0) == 0


def test_key_layout():
    k = R.mask_key(4321, 6, 1000, 17)
    assert k & 0xFFFFFFFF == 17 and k >> 32 == R.mix64(4321 + R.GOLDEN * 7 + R.NODE * 1001) >> 32
    assert R.mask_key(4321, 6, 1000, 17) >> 32 == R.mask_key(4321, 6, 1000, 99) >> 32       # the hash is the batch position's
    assert R.mask_key(4321, 6, 1000, 17) >> 32 != R.mask_key(4321, 6, 1001, 17) >> 32
    assert R.mask_key(4321, 6, 1000, 17) >> 32 != R.mask_key(4321, 7, 1000, 17) >> 32
    assert R.mask_key(4321 + (1 << 64), 6, 1000, 17) == k                                   # modulo 2^64


@pytest.mark.parametrize("seed,step", [(0, 0), (4321, 6), (2 ** 64 - 1, 2 ** 63), (77, 2 ** 32 + 5), (9, 2 ** 64 - 1)])
def test_upper_key_bits_equal_the_packages_node_hashes(pkg, seed, step):
    pos = list(range(150)) + [387, 388, 1023, 1024, 2047, 2048, 16396, 16397, 65535, 65536, 10 ** 6, 2 ** 31 - 2]
    pos += [int(p) for p in np.random.RandomState(3).randint(0, 2 ** 31 - 1, size=200)]
    want = pkg.sensor_layout.node_hashes(seed, step, pos)
    got = [R.mask_key(seed, step, p, 0) >> 40 for p in pos]
    assert got == [int(w) for w in want]
    # ... and the search's numpy statement of the upper half is the restatement's
    assert [int(h) for h in R.upper_halves(seed, step, 5, 300)] == [R.mask_key(seed, step, 5 + v, v) >> 32 for v in range(300)]


# ---- the contract ----------------------------------------------------------------------------------------------------------------
SIZES = [5, 388, 1, 64, 2049, 3, 388]


@pytest.mark.parametrize("rate", [0.0, 1.0, 0.95, 0.5, 0.29, 0.34, 1e-4])
def test_exactly_k_per_graph(rate):
    m = R.sampler_mask(4321, 6, SIZES, rate)
    assert m.dtype == np.uint8 and m.shape == (sum(SIZES),) and set(np.unique(m)) <= {0, 1}
    off = np.concatenate([[0], np.cumsum(SIZES)])
    for g, n in enumerate(SIZES):
        assert int(m[off[g]:off[g + 1]].sum()) == int(n * rate), (g, n)
    if rate == 1.0:
        assert m.all()
    if rate == 0.0:
        assert not m.any()


def test_the_k_smallest_keys_are_masked():
    n0, n, rate = 393, 388, 0.5
    m = R.sampler_mask(7, 3, [5, 388, 388], rate)[n0:n0 + n]
    keys = R.graph_keys(7, 3, n0, n)
    assert len(set(keys)) == n
    assert max(k for k, b in zip(keys, m) if b) < min(k for k, b in zip(keys, m) if not b)


def test_required_nodes():
    sizes, rate = [388, 37, 388], 0.5
    req = [387, 0, 20, 5]                                         # unsorted
    m = R.sampler_mask(11, 2, sizes, rate, req)
    off = np.concatenate([[0], np.cumsum(sizes)])
    for g, n in enumerate(sizes):
        part = m[off[g]:off[g + 1]]
        assert int(part.sum()) == int(n * rate)
        assert all(part[v] == 1 for v in req if v < n)            # (387 is outside the 37-node graph: ignored there)
    assert np.array_equal(m, R.sampler_mask(11, 2, sizes, rate, sorted(req)))
    # the others are the smallest keys among the non-required nodes: a required node displaces the largest masked keys only
    free = R.sampler_mask(11, 2, sizes, rate)
    part, fpart = m[:388], free[:388]
    keys = R.graph_keys(11, 2, 0, 388)
    dropped = [v for v in range(388) if fpart[v] and not part[v]]
    kept = [v for v in range(388) if fpart[v] and part[v] and v not in req]
    assert dropped and max(keys[v] for v in kept) < min(keys[v] for v in dropped)
    # no list, an empty list and empty per-graph lists: the same bytes
    assert R.sampler_mask(11, 2, sizes, rate, []).tobytes() == free.tobytes()
    assert R.sampler_mask(11, 2, sizes, rate, [[], [], []]).tobytes() == free.tobytes()
    # per-graph lists
    per = R.sampler_mask(11, 2, sizes, rate, [[3], [], [0, 387]])
    assert per[3] == 1 and per[off[2]] == 1 and per[off[2] + 387] == 1
    assert np.array_equal(per[off[1]:off[2]], free[off[1]:off[2]])
    assert np.array_equal(per[:388], R.sampler_mask(11, 2, [388], rate, [3]))


def test_mask_depends_on_the_batch_position():
    a = R.sampler_mask(4321, 6, [388, 388], 0.5)
    assert not np.array_equal(a[:388], a[388:])
    b = R.sampler_mask(4321, 6, [1, 388], 0.5)
    assert not np.array_equal(a[:388], b[1:]) and not np.array_equal(a[388:], b[1:])
    assert not np.array_equal(a, R.sampler_mask(4321, 7, [388, 388], 0.5))
    assert not np.array_equal(a, R.sampler_mask(4322, 6, [388, 388], 0.5))


@pytest.mark.parametrize("n,rate,k", [(100, 0.29, 28), (20, 0.95, 19), (3, 0.34, 1), (388, 0.95, 368)])
def test_truncation(n, rate, k):
    # (100 * 0.29 = 28.999999999999996 and 20 * 0.95 = 19.0 exactly in doubles: what int() sees is the double product)
    assert R.mask_count(n, rate) == k
    assert int(R.sampler_mask(1, 1, [n], rate).sum()) == k


def test_rate_for_count():
    for n, k in ((388, 0), (388, 1), (388, 387), (388, 388 - 1), (2049, 1314), (16397, 6252), (5, 5 - 1)):
        assert int(n * R.rate_for_count(n, k)) == k


# ---- the distribution ------------------------------------------------------------------------------------------------------------
# Per-node counts of falling into the RARER of the two classes over D draws (consecutive steps, one seed), and how often two
# fixed nodes are open together.  With k of n nodes drawn without replacement a node's count is Binomial(D, p), p = k/n, so the
# chi-square statistic sum (c - Dp)^2 / (Dp) has mean n(1 - p): for the rarer class close to its n - 1 degrees of freedom (388
# nodes, 20 open: 368 of 387), for the other class a twentieth of them -- which is why the rarer class is counted.  The bound is
# the one test_gpu_eval_device.py uses, df + 6 sqrt(2 df).
# D: 2000 draws give an expected count of 103 per node at 388 nodes (the chi-square approximation is good from ~5 on), and a
# sampler whose per-node probabilities are off by 7 % rms adds D * 20 * 0.07^2 = 196 > 6 sqrt(2 * 387) = 167 to the statistic.
# At 2100 nodes (the radix path's size class; rate 0.3: 630 masked, the rarer class) 200 draws give 60 per node.
# Both D were checked against the reference's own sampler (numpy's choice without replacement through
# wdn_synth.generate_batch_mask) with the same bounds: test_the_reference_sampler_stays_inside_the_same_bounds.
DIST_CASES = {"388": (388, 0.95, 2000), "2100": (2100, 0.3, 200)}
PAIRS = {"388": [(0, 1), (193, 194), (0, 387), (100, 300)], "2100": [(0, 1), (2047, 2048), (0, 2099), (700, 1400)]}
PAIR_SIGMAS = 5.0    # two-sided margin of a pair count in binomial standard deviations: 8 pairs x 2 samplers, P(> 5 sd) ~ 1e-5 each


def _judge(name, masks):
    """masks: [D, n] uint8.  Asserts the chi-square bound and the pair margins; returns the figures."""
    n, rate, D = DIST_CASES[name]
    assert masks.shape == (D, n)
    k = int(n * rate)
    assert (masks.sum(axis=1) == k).all()
    rare = masks if k <= n - k else 1 - masks
    kr = min(k, n - k)
    counts = rare.sum(axis=0).astype(np.float64)
    expect = D * kr / n
    chi2 = float(((counts - expect) ** 2 / expect).sum())
    df = n - 1
    bound = df + 6 * math.sqrt(2 * df)
    assert chi2 < bound, (name, chi2, bound)
    assert chi2 > n * (1 - kr / n) - 6 * math.sqrt(2 * df), (name, chi2)          # (not too regular either: the mean less 6 sd)
    ko = n - k                                                                      # open together: k'(k'-1) / (n(n-1))
    p2 = ko * (ko - 1) / (n * (n - 1))
    sd = math.sqrt(D * p2 * (1 - p2))
    both = []
    for a, b in PAIRS[name]:
        c = int(((masks[:, a] == 0) & (masks[:, b] == 0)).sum())
        assert abs(c - D * p2) <= PAIR_SIGMAS * sd, (name, (a, b), c, D * p2, sd)
        both.append(c)
    return chi2, bound, both, D * p2, sd


@pytest.mark.parametrize("name", list(DIST_CASES))
def test_the_restatement_is_uniform(name):
    n, rate, D = DIST_CASES[name]
    masks = np.stack([R.sampler_mask(99, step, [n], rate) for step in range(D)])
    print(name, _judge(name, masks))


@pytest.mark.parametrize("name", list(DIST_CASES))
def test_the_reference_sampler_stays_inside_the_same_bounds(pkg, name):
    n, rate, D = DIST_CASES[name]
    rng = np.random.RandomState(99)
    masks = np.stack([pkg.wdn_synth.generate_batch_mask([n], rate, rng).astype(np.uint8) for _ in range(D)])
    print(name, _judge(name, masks))


def test_a_biased_sampler_leaves_the_bounds():
    """The judge has teeth: masking the k smallest of keys whose hash is multiplied by (1 + 0.3 v / n) -- a mild preference
    for low indices that keeps exactly k per graph -- fails the chi-square bound on the same D."""
    n, rate, D = DIST_CASES["388"]
    k = int(n * rate)
    tilt = 1.0 + 0.3 * np.arange(n) / n
    masks = np.zeros((D, n), dtype=np.uint8)
    for step in range(D):
        h = R.upper_halves(99, step, 0, n).astype(np.float64) * tilt
        masks[step, np.argsort(h, kind="stable")[:k]] = 1
    with pytest.raises(AssertionError):
        _judge("388", masks)


# ---- graphs in which two nodes share the upper key half ------------------------------------------------------------------------
@pytest.mark.parametrize("n,max_steps", [(16397, 8), (2048, 2000), (2049, 2000)])
def test_collision_constants_are_what_the_search_finds(n, max_steps):
    found = R.collision_search(R.COLLISION_SEED, n, max_steps)
    assert found == R.COLLISIONS[n]
    step, r, (a, b) = found
    # the same in plain Python: the pair shares the upper half, sits at sorted ranks r and r + 1, the lower index first
    keys = R.graph_keys(R.COLLISION_SEED, step, 0, n)
    assert keys[a] >> 32 == keys[b] >> 32 and a < b
    order = sorted(range(n), key=keys.__getitem__)
    assert order[r] == a and order[r + 1] == b
    # a rate whose k-th key is the lower one of the pair: exactly one of the two is masked
    rate = R.rate_for_count(n, r + 1)
    m = R.sampler_mask(R.COLLISION_SEED, step, [n, 5], rate)
    assert m[a] == 1 and m[b] == 0 and int(m[:n].sum()) == r + 1


def test_collision_under_a_required_list():
    """The 2049-node pair with required nodes outside it: every required node whose random key lay above the pair's moves below
    it, so the pair's rank shifts by that count; the rate is derived for the shifted rank."""
    n = 2049
    step, r, (a, b) = R.COLLISIONS[n]
    req = R.COLLISION_REQUIRED
    assert a not in req and b not in req
    rate, r2 = R.collision_required_rate(n, req)
    keys = R.graph_keys(R.COLLISION_SEED, step, 0, n)
    assert r2 == r + sum(1 for v in req if keys[v] > keys[b]) and r2 > r
    m = R.sampler_mask(R.COLLISION_SEED, step, [n, 5], rate, req)
    assert m[a] == 1 and m[b] == 0 and all(m[v] == 1 for v in req) and int(m[:n].sum()) == r2 + 1


# ---- which GPU case fails under which edit of the selection ----------------------------------------------------------------------
def kernel_model(seed, step, sizes, rate, wgs, required=None, edit=None):
    """numpy model of mask_sample_graph's ALGORITHM (not of its contract): Q slices of the all-pairs rank, the WGS node ranges,
    the 8-pass radix select with its histogram walk.  ``edit`` applies one of the mutations below."""
    out = np.full(sum(sizes), 0xC3, dtype=np.uint8)              # (a byte nobody writes stays 0xC3)
    n0 = 0
    for n in sizes:
        k = int(n * rate)
        gn0 = 0 if edit == "gnode_local" else n0
        keys = np.array(R.graph_keys(seed, step, gn0, n, required or ()), dtype=np.uint64)
        if k <= 0:
            out[n0:n0 + n] = 0
        elif n <= 2048:
            Q = min(16, max(1, (n + 63) // 64))
            sl = n // Q if edit == "slice_floor" else (n + Q - 1) // Q
            per = (n + wgs - 1) // wgs
            for wq in range(wgs):
                vlo = min(n, wq * per)
                vhi = min(n, vlo + per)
                rank = np.zeros(vhi - vlo, dtype=np.int64)
                for q in range(Q):
                    ub, ue = q * sl, min(n, q * sl + sl)
                    rank += (keys[None, ub:ue] < keys[vlo:vhi, None]).sum(axis=1)
                out[n0 + vlo:n0 + vhi] = (rank <= k) if edit == "rank_le" else (rank < k)
        else:
            prefix, kk = 0, k
            passes = range(7, 3, -1) if edit == "low_passes_skipped" else range(7, -1, -1)
            for p in passes:
                match = np.ones(n, dtype=bool) if p == 7 else (keys >> np.uint64(8 * (p + 1))) == np.uint64(prefix)
                hist = np.bincount(((keys[match] >> np.uint64(8 * p)) & np.uint64(255)).astype(np.int64), minlength=256)
                b = 0
                while b < 255 and kk > hist[b]:
                    kk -= hist[b]
                    b += 1
                prefix = (prefix << 8) | b
            if edit == "low_passes_skipped":
                prefix = (prefix << 32) | 0xFFFFFFFF             # (every key of the selected upper half)
            kth = np.uint64(prefix)
            out[n0:n0 + n] = (keys < kth) if edit == "radix_lt" else (keys <= kth)
        n0 += n
    return out


GPU_SIZES = R.GPU_SIZES


@pytest.mark.parametrize("wgs", [4, 16])
@pytest.mark.parametrize("rate", [0.95, 0.29, 1e-4])
def test_the_kernels_algorithm_equals_the_contract_on_the_gpu_cases(wgs, rate):
    assert np.array_equal(kernel_model(4321, 6, GPU_SIZES, rate, wgs), R.sampler_mask(4321, 6, GPU_SIZES, rate))


def _graph(mask, sizes, g):
    off = np.concatenate([[0], np.cumsum(sizes)])
    return mask[off[g]:off[g + 1]]


def test_each_edit_of_the_selection_fails_a_named_gpu_case():
    """The edits the sampler's tests must notice, each on cases of test_gpu_mask_sampler.py (sizes, seed 4321, step 6)."""
    sizes, rate = GPU_SIZES, 0.5
    true = R.sampler_mask(4321, 6, sizes, rate)
    differs = {}
    for edit in ("rank_le", "slice_floor", "radix_lt", "low_passes_skipped", "gnode_local"):
        got = kernel_model(4321, 6, sizes, rate, 4, edit=edit)
        differs[edit] = [n for g, n in enumerate(sizes) if not np.array_equal(_graph(got, sizes, g), _graph(true, sizes, g))]
    # `<= k`: every all-pairs graph with 0 < k < n (k + 1 nodes masked); not the radix graphs
    assert set(differs["rank_le"]) == {n for n in sizes if n <= 2048 and 0 < int(n * rate) < n}
    # floor: the keys behind Q * (n // Q) are never counted: graphs whose size Q does not divide, here among others
    assert {65, 388, 961, 1023, 2047} <= set(differs["slice_floor"])
    assert not {64, 128, 129, 960, 1024, 2048} & set(differs["slice_floor"])          # (129 = 3 * 43)
    # `< kth`: every radix graph (k - 1 nodes masked); not the all-pairs graphs
    assert set(differs["radix_lt"]) == {n for n in sizes if n > 2048}
    # the batch position: every graph but the first (a graph of a few nodes can draw the same subset by chance)
    assert set(differs["gnode_local"]) >= {n for n in sizes[1:] if n >= 15} and sizes[0] not in differs["gnode_local"]
    # the low passes: nothing in this batch -- only the collision graphs notice, where both nodes of the pair get masked
    assert differs["low_passes_skipped"] == []
    for n in (16397, 2049):
        step, r, (a, b) = R.COLLISIONS[n]
        crate = R.rate_for_count(n, r + 1)
        true_c = R.sampler_mask(R.COLLISION_SEED, step, [n, 5], crate)
        assert np.array_equal(kernel_model(R.COLLISION_SEED, step, [n, 5], crate, 4), true_c)
        got = kernel_model(R.COLLISION_SEED, step, [n, 5], crate, 4, edit="low_passes_skipped")
        assert got[a] == 1 and got[b] == 1 and true_c[b] == 0
    # (the all-pairs tie order, at 2048 nodes: ranking by the upper half alone puts both nodes of the pair at the same rank)
    step, r, (a, b) = R.COLLISIONS[2048]
    keys = R.graph_keys(R.COLLISION_SEED, step, 0, 2048)
    hi = [key >> 32 for key in keys]
    assert sum(h < hi[a] for h in hi) == sum(h < hi[b] for h in hi) == r
    # `step` for `step + 1` in an update tail's key: the mask of optimizer step s + 1 would be the mask of step s, which the
    # trainer test compares with the restatement at s + 1
    assert not np.array_equal(R.sampler_mask(9, 1, [388, 388], 0.95), R.sampler_mask(9, 0, [388, 388], 0.95))
