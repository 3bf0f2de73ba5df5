"""The cut of an estimation pass (``pass_schedule`` / ``pass_batch_sizes`` of estimation.py, the loops of
``PressureEstimator._pair_pass``) against the three loops the passes used to write out themselves, restated here literally: the
plain pass's loop over S snapshots, the flat loop over the S * W pairs and the chunked loop over ``ensemble_chunk``'s chunks.
No device."""
import itertools

SNAPSHOTS, WIDTHS, BATCH_SIZES = range(1, 12), range(1, 8), range(1, 7)
BUDGETS = (1, 64, 200, 1000, 10 ** 9)
ROW_BYTES = 12                                                 # (of a pair in the scratch: any; with the budgets it moves the chunk)


def plain_loop(S, bs):
    """The plain pass: ``(plan size, first, g, dst_first)`` per batch and the sizes the plans were fetched for."""
    sizes = [min(bs, S - first) for first in range(0, S, bs)]
    return [(g, b * bs, g, b * bs) for b, g in enumerate(sizes)], sorted(set(sizes))


def flat_loop(S, W, bs):
    """The unchunked pass over pairs: ``(plan size, first, g, dst_first)`` per batch and the sizes the plans were fetched for."""
    out = []
    for first in range(0, S * W, bs):
        g = min(bs, S * W - first)
        out.append((g, first, g, first))
    return out, sorted({min(bs, S * W - first) for first in (0, (S * W - 1) // bs * bs)})


def chunked_loop(S, W, bs, C):
    """The chunked pass: per chunk ``(s0, c)`` and its batches ``(plan size, first, g, dst_first)``."""
    chunks = []
    for s0 in range(0, S, C):
        c = min(C, S - s0)
        batches = []
        for off in range(0, c * W, bs):
            g = min(bs, c * W - off)
            batches.append((g, s0 * W + off, g, off))
        chunks.append(((s0, c), batches))
    return chunks


def schedule(E, S, W, bs, chunk=None):
    """``pass_schedule`` with every chunk's batches as a list."""
    return [(s0, c, list(batches)) for s0, c, batches in E.pass_schedule(S, W, bs, chunk)]


def driven(E, S, W, bs, chunk):
    """What ``_pair_pass`` does with the schedule: per chunk ``(s0, c)`` and the ``(plan size, first, g, off)`` of its batches."""
    return [((s0, c), [(g, first, g, off) for first, g, off in batches]) for s0, c, batches in E.pass_schedule(S, W, bs, chunk)]


def test_the_schedule_is_the_three_loops(pkg):
    E = pkg.estimation
    for S, W, bs in itertools.product(SNAPSHOTS, WIDTHS, BATCH_SIZES):
        flat, flat_sizes = flat_loop(S, W, bs)
        one = driven(E, S, W, bs, None)
        # one chunk of all S snapshots: the flat loop, row for row (off == first: the result is the chunk)
        assert one == [((0, S), flat)], (S, W, bs)
        occurring = {g for g, _, _, _ in flat}
        assert E.pass_batch_sizes(S, W, bs) == occurring == set(flat_sizes), (S, W, bs)
        if W == 1:
            plain, plain_sizes = plain_loop(S, bs)
            assert one == [((0, S), plain)] and sorted(occurring) == plain_sizes, (S, bs)
        for budget in BUDGETS:
            C = E.ensemble_chunk(S, W, bs, ROW_BYTES, budget)
            got = driven(E, S, W, bs, C)
            assert got == chunked_loop(S, W, bs, C), (S, W, bs, budget)
            # the chunks are consecutive and cover the S snapshots
            assert [s0 for (s0, _), _ in got] == list(range(0, S, C)) and sum(c for (_, c), _ in got) == S
            # the batch partition does not depend on the budget: (first, g) of the flat loop
            assert [(first, g) for _, batches in got for _, first, g, _ in batches] == [(first, g) for _, first, g, _ in flat]
            # every chunk but the last ends on a batch boundary, and its batches tile it from row 0 of the scratch
            for (s0, c), batches in got:
                assert [off for _, _, _, off in batches] == [first - s0 * W for _, first, _, _ in batches]
                assert sum(g for g, _, _, _ in batches) == c * W
                if s0 + c < S:
                    assert (c * W) % bs == 0 and all(g == bs for g, _, _, _ in batches), (S, W, bs, budget)
    assert [E.ensemble_chunk(11, 4, 2, ROW_BYTES, b) for b in BUDGETS] == [1, 1, 4, 11, 11]        # (the budgets do move the chunk)


def test_the_quoted_cases_by_hand(pkg):
    """The chunkings the device tests quote, with their schedules written out."""
    E = pkg.estimation
    # 5 snapshots x 3 members at batch size 4, 37 nodes: a unit of lcm(4, 3) / 3 = 4 snapshots, then 1
    assert E.ensemble_chunk(5, 3, 4, 4 * 37, 1) == 4
    assert schedule(E, 5, 3, 4, 4) == [(0, 4, [(0, 4, 0), (4, 4, 4), (8, 4, 8)]), (4, 1, [(12, 3, 0)])]
    assert E.pass_batch_sizes(5, 3, 4) == {4, 3}
    # 5 snapshots x 6 layouts / targets at batch size 4: units of lcm(4, 6) / 6 = 2 snapshots -- chunks of 2, 2 and 1
    three = [(0, 2, [(0, 4, 0), (4, 4, 4), (8, 4, 8)]), (2, 2, [(12, 4, 0), (16, 4, 4), (20, 4, 8)]), (4, 1, [(24, 4, 0), (28, 2, 4)])]
    assert E.ensemble_chunk(5, 6, 4, 32, 1) == 2
    for K in (3, 8):
        assert E.ensemble_chunk(5, 6, 4, 4 * K, 2 * 6 * K * 4) == 2
    assert schedule(E, 5, 6, 4, 2) == three
    assert E.pass_batch_sizes(5, 6, 4) == {4, 2}
    # the same pairs as one chunk: the same (first, g), off == first
    assert schedule(E, 5, 6, 4) == [(0, 5, [(f, g, f) for f, g in ((0, 4), (4, 4), (8, 4), (12, 4), (16, 4), (20, 4),
                                                                              (24, 4), (28, 2))])]
    # a chunk's batches do not depend on when they are taken: after the whole schedule, in any order
    late = list(E.pass_schedule(5, 6, 4, 2))
    assert [(s0, c, list(b)) for s0, c, b in reversed(late)] == three[::-1]
    # one batch holds everything: one plan size
    assert schedule(E, 2, 3, 32) == [(0, 2, [(0, 6, 0)])] and E.pass_batch_sizes(2, 3, 32) == {6}
