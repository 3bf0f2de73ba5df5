"""Host logic of ``MultiSnapshotStore``: the batch recipe, the epoch schedule, the shared statistics, the cached block-diagonal
``edge_index`` -- and the C-ABI symbols of the multi-matrix collation, declared in include/gatres.h and bound in _native.py."""
import os
import re
from collections import Counter

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def largest_remainder(lengths, B):
    """The rule restated: quotas B * S_k / sum(S), floors, the leftover graphs to the largest fractional parts (ties: the
    lower index); then every non-empty network that holds none takes one from the network that holds the most (ties: the
    lower index)."""
    total = sum(lengths)
    quota = [B * s / total for s in lengths]            # (small integers: exact enough to order the fractions below)
    b = [int(np.floor(q)) for q in quota]
    frac = [(B * s) % total for s in lengths]           # the fractional parts, as exact integers over `total`
    order = sorted(range(len(lengths)), key=lambda k: (-frac[k], k))
    for k in order[:B - sum(b)]:
        b[k] += 1
    for k, s in enumerate(lengths):
        if s >= 1 and b[k] == 0:
            top = max(b)
            j = b.index(top)
            b[j] -= 1
            b[k] = 1
    return tuple(b)


RECIPE_CASES = [
    ([100, 100, 100], 32),          # equal lengths
    ([100, 100, 100], 3),           # B == K
    ([1000, 10, 5], 8),             # one dominant network: the small ones would get none
    ([1000, 10, 5], 32),
    ([7, 1, 50], 16),               # a length of 1
    ([1, 1, 1], 3),
    ([640, 388, 97], 32),
    ([500], 32),                    # one network
    ([33, 17], 2),
]


# Worked by hand: quotas B * S_k / sum(S), floors, leftover graphs to the largest fractions, then one graph for every network
# that has none, taken from the largest share.
#   [1000, 10, 5] at 8: quotas 7.88 / 0.08 / 0.04 -> floors 7, 0, 0, the one leftover to network 0 -> (8, 0, 0) -> (6, 1, 1)
#   [100, 100, 100] at 32: quotas 10.67 each, two leftovers to the two lowest indices -> (11, 11, 10)
#   [7, 1, 50] at 16: quotas 1.93 / 0.28 / 13.79 -> floors 1, 0, 13, leftovers to 0.93 and 0.79 -> (2, 0, 14) -> (2, 1, 13)
#   [640, 388, 97] at 32: quotas 18.20 / 11.04 / 2.76 -> floors 18, 11, 2, the leftover to 0.76 -> (18, 11, 3)
#   [33, 17] at 2: quotas 1.32 / 0.68 -> floors 1, 0, the leftover to 0.68 -> (1, 1)
HAND_WORKED = [([1000, 10, 5], 8, (6, 1, 1)), ([100, 100, 100], 32, (11, 11, 10)), ([7, 1, 50], 16, (2, 1, 13)),
               ([640, 388, 97], 32, (18, 11, 3)), ([33, 17], 2, (1, 1)), ([100, 100, 100], 3, (1, 1, 1)), ([500], 32, (32,))]


@pytest.mark.parametrize("lengths,B,want", HAND_WORKED)
def test_recipe_equals_the_hand_worked_answers(pkg, lengths, B, want):
    from gnn_pressure_estimation_amd.multi_snapshot_store import batch_recipe
    assert batch_recipe(lengths, B) == want


@pytest.mark.parametrize("lengths,B", RECIPE_CASES)
def test_recipe_is_the_largest_remainder_answer_with_every_network_present(pkg, lengths, B):
    from gnn_pressure_estimation_amd.multi_snapshot_store import batch_recipe
    b = batch_recipe(lengths, B)
    assert sum(b) == B and all(x >= 1 for x in b)
    assert b == largest_remainder(lengths, B)


def test_recipe_refuses_fewer_graphs_than_networks(pkg):
    from gnn_pressure_estimation_amd.multi_snapshot_store import batch_recipe, epoch_schedule
    with pytest.raises(ValueError):
        batch_recipe([10, 10, 10], 2)
    with pytest.raises(ValueError):
        epoch_schedule([10, 10, 10], 2)
    with pytest.raises(ValueError):
        epoch_schedule([10, 10, 10], 8, recipe=(4, 4))           # not a recipe of three networks
    with pytest.raises(ValueError):
        epoch_schedule([10, 10, 10], 8, recipe=(4, 4, 4))        # not 8 graphs


def _nets(pkg, shapes, scale=6.0, shift=35.0):
    out = []
    for i, (S, n) in enumerate(shapes):
        ei = pkg.wdn_synth.make_wdn_topology(n, n + n // 10, seed=i)
        out.append((pkg.wdn_synth.make_snapshots(S, n, seed=10 + i) * scale * (i + 1) + shift, ei))
    return out


SCHEDULE_CASES = [
    ([100, 37, 11], 16, None),
    ([23, 23, 23], 6, None),
    ([40, 9, 3], 8, None),           # tails of two different recipes
    ([50, 20], 8, (4, 4)),           # the caller's recipe: network 1 runs out first, the rest of network 0 goes to tails
    ([31], 4, None),
    ([5, 1, 1], 32, None),           # fewer snapshots than one batch: no full batch at all
]


@pytest.mark.parametrize("lengths,B,recipe", SCHEDULE_CASES)
def test_schedule_visits_every_snapshot_exactly_once(pkg, lengths, B, recipe):
    from gnn_pressure_estimation_amd.multi_snapshot_store import epoch_schedule
    store = pkg.MultiSnapshotStore(_nets(pkg, [(S, 7 + 3 * k) for k, S in enumerate(lengths)]))
    sched = store.schedule(B, recipe, drop_last=False)
    assert sched == epoch_schedule(lengths, B, recipe, False)                   # a pure function of these arguments
    main = sched.recipe
    if sum(lengths) >= B:
        assert sum(main) == B
    assert sched.nfull == min(s // b for s, b in zip(lengths, main) if b)
    assert all(0 < sum(t) <= B for t in sched.tails)
    epochs = []
    for ep in range(2):
        rows = store.epoch_rows_host(sched, shuffle=True, generator=torch.Generator().manual_seed(5 + ep))
        assert rows.dtype == torch.int64 and rows.numel() == sum(lengths)
        at, visited = 0, []
        for r in [main] * sched.nfull + list(sched.tails):
            for k, b in enumerate(r):
                for row in rows[at:at + b].tolist():
                    assert 0 <= row < lengths[k]
                    visited.append((k, row))
                at += b
        assert Counter(visited) == Counter((k, s) for k, S in enumerate(lengths) for s in range(S))
        epochs.append(visited)
    assert epochs[0] != epochs[1] or sum(lengths) < 4                            # ... in another order every epoch
    assert [k for k, _ in epochs[0]] == [k for k, _ in epochs[1]]              # the same schedule apart from the permutations
    # without shuffle every network is taken in order
    rows = store.epoch_rows_host(sched, shuffle=False)
    at, nxt = 0, [0] * len(lengths)
    for r in [main] * sched.nfull + list(sched.tails):
        for k, b in enumerate(r):
            assert rows[at:at + b].tolist() == list(range(nxt[k], nxt[k] + b))
            nxt[k] += b
            at += b


def test_a_tail_that_needs_two_different_recipes(pkg):
    from gnn_pressure_estimation_amd.multi_snapshot_store import epoch_schedule
    sched = epoch_schedule([40, 9, 3], 8)
    assert len(set(sched.tails)) >= 2 and all(t != sched.recipe for t in sched.tails), sched
    again = epoch_schedule([40, 9, 3], 8)
    assert again == sched


@pytest.mark.parametrize("lengths,B,recipe", SCHEDULE_CASES)
def test_drop_last_yields_exactly_the_full_batches(pkg, lengths, B, recipe):
    from gnn_pressure_estimation_amd.multi_snapshot_store import epoch_schedule
    full = epoch_schedule(lengths, B, recipe, drop_last=True)
    both = epoch_schedule(lengths, B, recipe, drop_last=False)
    assert full.tails == () and full.nfull == both.nfull and full.recipe == both.recipe
    assert full.sizes == [sum(full.recipe)] * full.nfull


def test_shared_statistics_are_numpys_over_all_values(pkg):
    nets = _nets(pkg, [(20, 30), (7, 13), (5, 50)])
    store = pkg.MultiSnapshotStore(nets)
    allv = np.concatenate([a.numpy().ravel() for a, _ in nets])
    # the store's statistics are formed in double; numpy's own fp32 reductions (pairwise, fp32 accumulators) are within a few
    # fp32 ulps of that
    assert store.mean == pytest.approx(float(np.mean(allv.astype(np.float64))), rel=1e-12)
    assert store.std == pytest.approx(float(np.std(allv.astype(np.float64))), rel=1e-12)
    assert store.mean == pytest.approx(float(np.mean(allv)), rel=1e-5)
    assert store.std == pytest.approx(float(np.std(allv)), rel=1e-5)
    assert store.min == float(allv.min()) and store.max == float(allv.max())
    assert store.norm_type == "znorm" and len(store) == 32 and store.num_networks == 3 and store.lengths == (20, 7, 5)
    assert [store.nodes_per_graph_of(k) for k in range(3)] == [30, 13, 50]
    for k, (a, _) in enumerate(nets):
        assert torch.equal(store.data_of(k), (a - store.mean) / (store.std + 1e-8))
    x = torch.randn(11)
    assert torch.equal(store.descale(x), x * store.std + store.mean)
    # passed-in statistics (a validation store takes the training store's) are used unchanged
    val = pkg.MultiSnapshotStore(_nets(pkg, [(3, 30), (2, 13), (4, 50)], scale=2.0), mean=store.mean, std=store.std,
                                 min=store.min, max=store.max)
    assert (val.mean, val.std, val.min, val.max) == (store.mean, store.std, store.min, store.max)
    assert pkg.evaluation._store_descale(val, None) == (store.std, store.mean)


def test_one_network_is_the_snapshot_store_of_that_network(pkg):
    (snaps, ei), = _nets(pkg, [(19, 41)])
    multi, single = pkg.MultiSnapshotStore([(snaps, ei)]), pkg.SnapshotStore(snaps, ei)
    assert multi.mean == single.mean and multi.std == single.std
    assert torch.equal(multi.data_of(0), single.data)                          # bit for bit
    assert torch.equal(multi.edge_index((4,)), single.edge_index(4))
    assert multi.recipe(4) == (4,) and multi.nodes_per_graph((4,)) == [41] * 4
    sched = multi.schedule(4)
    assert (sched.nfull, sched.tails) == (4, ((3,),))
    rows = multi.epoch_rows_host(sched, generator=torch.Generator().manual_seed(3))
    assert torch.equal(rows, single.epoch_order(generator=torch.Generator().manual_seed(3)))


def test_edge_index_of_a_recipe_is_the_networks_blocks_side_by_side(pkg):
    nets = _nets(pkg, [(4, 30), (4, 13), (4, 50)])
    store = pkg.MultiSnapshotStore(nets)
    singles = [pkg.SnapshotStore(a, ei, normalize=False) for a, ei in nets]
    for recipe in [(2, 1, 3), (1, 1, 1), (0, 2, 1)]:
        ei = store.edge_index(recipe)
        blocks, off = [], 0
        for k, b in enumerate(recipe):
            if b:
                blocks.append(singles[k].edge_index(b) + off)
            off += b * singles[k].nodes_per_graph
        assert torch.equal(ei, torch.cat(blocks, dim=1))
        assert store.edge_index(recipe) is ei and store.edge_index(list(recipe)) is ei     # the same object: the plan cache's identity path
        assert store.num_nodes(recipe) == off and sum(store.nodes_per_graph(recipe)) == off
        assert store.net_of_graph(recipe).tolist() == [k for k, b in enumerate(recipe) for _ in range(b)]
        assert store.node_ranges(recipe)[-1][1] == off
    with pytest.raises(ValueError):
        store.recipe(2)                                                        # B < K
    with pytest.raises(ValueError):
        store.recipe(8, (4, 4))
    assert store.recipe(8, (1, 1, 6)) == (1, 1, 6)


def test_required_idx_of_several_networks_is_one_sequence_per_network(pkg):
    store = pkg.MultiSnapshotStore(_nets(pkg, [(4, 30), (4, 13), (4, 50)]))
    E = pkg.evaluation
    assert E.required_csr(store, [[3, 1], [], [7, 49, 7]], 0.9) == ([0, 2, 2, 4], [1, 3, 7, 49])
    with pytest.raises(ValueError, match="flat"):
        E.required_csr(store, [1, 2, 3], 0.9)
    with pytest.raises(ValueError):
        E.required_csr(store, [[1], [2]], 0.9)                                 # two sequences for three networks
    with pytest.raises(ValueError):
        E.required_csr(store, [[1], [13], []], 0.9)                            # outside network 1
    with pytest.raises(ValueError):
        E.required_csr(store, [[], list(range(11)), []], 0.9)                  # int(13 * 0.9) = 11 required: nothing left to sample


def test_data_parallel_training_from_several_networks_is_refused(pkg):
    from gnn_pressure_estimation_amd.epoch_loop import refuse_multi_store_data_parallel
    refuse_multi_store_data_parallel(1)
    with pytest.raises(NotImplementedError, match="MultiSnapshotStore"):
        refuse_multi_store_data_parallel(2)


def test_load_wdns_is_the_list_form_of_load_wdn(pkg):
    io = pkg.wdn_io
    inp, zp = os.path.join(ROOT, "tests", "golden", "wdn_tiny.inp"), os.path.join(ROOT, "tests", "golden", "wdn_tiny.zip")
    one, kept = io.load_wdn(inp, zp, num_records=40)
    multi, kepts = io.load_wdns([inp, inp], [zp, zp], num_records=[40, 25])
    assert isinstance(multi, pkg.MultiSnapshotStore) and multi.lengths == (40, 25) and kepts == [kept, kept]
    assert torch.equal(multi.edge_index((1, 0)), one.edge_index(1))
    raw = one.data * (one.std + 1e-8) + one.mean
    allv = np.concatenate([raw.numpy().ravel(), raw[:25].numpy().ravel()]).astype(np.float64)
    assert multi.mean == pytest.approx(float(allv.mean()), rel=1e-6) and multi.std == pytest.approx(float(allv.std()), rel=1e-5)
    val, _ = io.load_wdns([inp, inp], [zp, zp], split="valid", mean=multi.mean, std=multi.std)
    assert (val.mean, val.std) == (multi.mean, multi.std)
    with pytest.raises(ValueError):
        io.load_wdns([inp, inp], [zp])


def test_the_multi_matrix_collation_is_declared_and_bound(pkg):
    with open(os.path.join(ROOT, "include", "gatres.h")) as f:
        header = f.read()
    for name in ("gatres_stage_multi_rows_mask_required", "gatres_gather_multi_rows"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in pkg._native.SIGNATURES
    assert "MultiSnapshotStore" in pkg.__all__
