"""Scoring sensor layouts and placing sensors, on the host: the three new symbols of k_estimate.hip are declared, exported and
bound without an ABI change and refuse their bad arguments before any launch; ``layout_scores_from_table`` holds on
hand-computed records; ``greedy_selection`` follows its rule on a fake scorer; ``place_sensors`` refuses what it can refuse
without a device.  No GPU, no kernel launches."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gatres_stage_observed_layouts", "gatres_layout_pair_errors", "gatres_layout_error_reduce")
P = 4096                       # (any non-null address: a refused call never reads it)
Q = 8192


def header():
    with open(os.path.join(ROOT, "include", "gatres.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


# ---- 1. symbols and refusals ----------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound_and_the_abi_stays(pkg, lib):
    hdr = header()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in pkg._native.SIGNATURES
    S = pkg._native.SIGNATURES
    # the arguments of gatres_stage_observed_available without rows, plus first_pair's partner num_layouts, and layouts
    assert len(S["gatres_stage_observed_layouts"][1]) == len(S["gatres_stage_observed_available"][1]) - 1 + 2
    assert len(S["gatres_layout_pair_errors"][1]) == 15 and len(S["gatres_layout_error_reduce"][1]) == 6
    assert "#define GATRES_ABI_VERSION 9" in hdr and pkg._native.ABI_VERSION == 9
    assert b"abi9" in lib.gatres_version()


def test_the_record_macros_equal_the_python_constants(pkg):
    N = pkg._native
    assert re.search(r"#define GATRES_LAYOUT_PAIR_RECORD\s+%d\b" % N.LAYOUT_PAIR_RECORD, header())
    assert re.search(r"#define GATRES_LAYOUT_ERROR_RECORD\s+%d\b" % N.LAYOUT_ERROR_RECORD, header())
    assert N.LAYOUT_PAIR_RECORD == 4 == pkg.estimation.LAYOUT_PAIR_RECORD
    assert N.LAYOUT_ERROR_RECORD == 4 == pkg.estimation.LAYOUT_ERROR_RECORD
    assert pkg.layout_scores_from_table is pkg.estimation.layout_scores_from_table
    assert pkg.greedy_selection is pkg.estimation.greedy_selection


def stage(lib, src=P, layout=0, src_rows=8, first_pair=0, num_layouts=6, n=37, graphs=3, observed=P, k=3, normalise=0, offset=0.0,
          factor=1.0, x=Q, mask=Q + 4096, available=3 * Q, nan_is_missing=0, layouts=5 * Q):
    return lib.gatres_stage_observed_layouts(src, layout, src_rows, first_pair, num_layouts, n, graphs, observed, k, normalise,
                                             offset, factor, x, mask, available, nan_is_missing, layouts, None)


def test_stage_observed_layouts_checks_its_arguments_before_any_launch(lib):
    # the pair range: 8 rows x 6 layouts = 48 pairs
    assert stage(lib, first_pair=-1) == -1
    assert stage(lib, first_pair=46) == -1                     # pairs 46, 47, 48 of 48
    assert stage(lib, first_pair=8, num_layouts=1) == -1       # as a plain pass: row 8 of 8
    assert stage(lib, first_pair=6, num_layouts=1) == -1       # rows 6, 7, 8 of 8
    assert stage(lib, src_rows=0) == -1
    assert stage(lib, src_rows=2 ** 62, num_layouts=4) == -1   # (src_rows * num_layouts does not fit)
    assert stage(lib, num_layouts=0) == -1
    assert stage(lib, num_layouts=-3) == -1
    assert stage(lib, layouts=None) == -1
    assert stage(lib, layouts=Q) == -1                         # layouts is x_dst
    assert stage(lib, layouts=Q + 4 * 3 * 37 - 1) == -1        # the last byte of x_dst
    assert stage(lib, layouts=Q + 4096 + 3 * 37 - 1) == -1     # the last byte of mask
    assert stage(lib, layouts=Q - 6 * 3 + 1) == -1             # its last byte is the first of x_dst
    # those of gatres_stage_observed_available
    assert stage(lib, k=0) == -1
    assert stage(lib, k=38) == -1
    assert stage(lib, graphs=0) == -1
    assert stage(lib, n=0) == -1
    for name in ("src", "observed", "x", "mask"):
        assert stage(lib, **{name: None}) == -1, name
    assert stage(lib, layout=2) == -1
    assert stage(lib, normalise=3) == -1
    assert stage(lib, layout=1, normalise=1, factor=0.0) == -1
    assert stage(lib, x=P) == -1                               # in place
    assert stage(lib, available=Q) == -1                       # available is x_dst
    assert stage(lib, available=Q + 4096 + 3 * 37 - 1) == -1   # the last byte of mask
    assert stage(lib, available=None, nan_is_missing=0, k=0) == -1      # (NULL is legal here: k is what is refused)


def pair_errors(lib, out=P, mask=Q, truth=4 * Q, truth_rows=8, n=37, graphs=3, first_pair=0, num_layouts=6, scale=12.5, offset=50.0,
                score=None, rec=64 * Q, rec_rows=9, rec_first=2):
    return lib.gatres_layout_pair_errors(out, mask, truth, truth_rows, n, graphs, first_pair, num_layouts, scale, offset, score, rec,
                                         rec_rows, rec_first, None)


def test_layout_pair_errors_checks_its_arguments_before_any_launch(lib):
    for name in ("out", "mask", "truth", "rec"):
        assert pair_errors(lib, **{name: None}) == -1, name
    assert pair_errors(lib, n=0) == -1
    assert pair_errors(lib, graphs=0) == -1
    assert pair_errors(lib, num_layouts=0) == -1
    assert pair_errors(lib, truth_rows=0) == -1
    assert pair_errors(lib, truth_rows=2 ** 62, num_layouts=4) == -1
    # the pair range: 8 rows x 6 layouts = 48 pairs
    assert pair_errors(lib, first_pair=-1) == -1
    assert pair_errors(lib, first_pair=46) == -1
    # the records: 3 of them from rec_first, 9 rows
    assert pair_errors(lib, rec_first=-1) == -1
    assert pair_errors(lib, rec_first=7) == -1                 # records 7, 8, 9 of 9
    assert pair_errors(lib, rec_rows=0) == -1
    assert pair_errors(lib, rec_rows=2, rec_first=0) == -1
    # overlaps: rec is 9 records of 32 bytes = 288 bytes; out 3 * 37 floats = 444 bytes from P, mask 111 bytes from Q, truth
    # 8 * 37 floats = 1184 bytes from 4 Q, score 37 bytes
    assert pair_errors(lib, rec=P) == -1
    assert pair_errors(lib, rec=P + 444 - 8) == -1             # starts on the last bytes of out
    assert pair_errors(lib, rec=P - 288 + 8) == -1             # ends on the first bytes of out
    assert pair_errors(lib, rec=Q + 104) == -1                 # inside mask
    assert pair_errors(lib, rec=4 * Q + 1184 - 8) == -1        # the last float of truth
    assert pair_errors(lib, score=64 * Q + 280) == -1          # score starts inside the last record


def reduce(lib, rec=P, S=5, L=6, table=64 * Q, accumulate=0):
    return lib.gatres_layout_error_reduce(rec, S, L, table, accumulate, None)


def test_layout_error_reduce_checks_its_arguments_before_any_launch(lib):
    assert reduce(lib, rec=None) == -1
    assert reduce(lib, table=None) == -1
    assert reduce(lib, S=0) == -1
    assert reduce(lib, S=-2) == -1
    assert reduce(lib, L=0) == -1
    assert reduce(lib, S=2 ** 60, L=64) == -1                  # (the records' bytes do not fit)
    # rec is 5 * 6 records of 32 bytes = 960 bytes from P, table 6 records = 192 bytes
    assert reduce(lib, table=P) == -1
    assert reduce(lib, table=P + 960 - 8, accumulate=1) == -1
    assert reduce(lib, table=P - 192 + 8) == -1


# ---- 2. the scores ----------------------------------------------------------------------------------------------------------------
def test_layout_scores_on_hand_computed_records(pkg):
    """Layout 0: errors 1, -2, 2 over three entries; layout 1: one entry of -0.5; layout 2: nothing scored."""
    table = np.array([[3.0, 5.0, 9.0, 2.0], [1.0, 0.5, 0.25, 0.5], [0.0, 0.0, 0.0, 0.0]])
    assert table.shape[1] == pkg.estimation.LAYOUT_ERROR_RECORD
    m = pkg.estimation.layout_scores_from_table(table)
    assert sorted(m) == ["count", "mae", "max_abs", "rmse"]
    np.testing.assert_array_equal(m["count"], [3.0, 1.0, 0.0])
    np.testing.assert_array_equal(m["mae"][:2], [5.0 / 3.0, 0.5])
    np.testing.assert_array_equal(m["rmse"][:2], [np.sqrt(3.0), 0.5])
    np.testing.assert_array_equal(m["max_abs"][:2], [2.0, 0.5])
    for key in ("mae", "rmse", "max_abs"):
        assert np.isnan(m[key][2]) and m[key].dtype == np.float64 and m[key].shape == (3,)
    # a flat list of one record is one layout
    assert pkg.estimation.layout_scores_from_table([2.0, 1.0, 1.0, 0.75])["mae"].tolist() == [0.5]


# ---- 3. the selection rule --------------------------------------------------------------------------------------------------------
def test_greedy_selection_with_a_fake_scorer(pkg):
    greedy = pkg.estimation.greedy_selection
    nan = float("nan")
    calls = []

    def table_scorer(table):
        def score_round(chosen, remaining):
            calls.append((list(chosen), list(remaining)))
            return [table[len(chosen)][c] for c in remaining]
        return score_round

    cands = [30, 10, 20, 40]
    # round 1: 20 is the smallest; round 2: 10 and 40 tie, 10 is earlier in `cands`; round 3: NaN loses to any number
    rounds = [{30: 3.0, 10: 2.0, 20: 1.0, 40: 5.0}, {30: 4.0, 10: 0.5, 40: 0.5}, {30: nan, 40: 7.0}, {30: nan}]
    chosen, scores = greedy(table_scorer(rounds), cands, 4)
    assert chosen == [20, 10, 40, 30]
    assert scores[:3] == [1.0, 0.5, 7.0] and np.isnan(scores[3])           # a round of NaNs: the earliest candidate
    assert calls == [([], [30, 10, 20, 40]), ([20], [30, 10, 40]), ([20, 10], [30, 40]), ([20, 10, 40], [30])]
    # num is respected: the scorer is not asked for more rounds
    del calls[:]
    assert greedy(table_scorer(rounds), cands, 2) == ([20, 10], [1.0, 0.5]) and len(calls) == 2
    assert greedy(table_scorer(rounds), cands, 0) == ([], [])
    # every score NaN but a later one: NaN counts as worst wherever it stands; all NaN: the first
    assert greedy(lambda ch, rem: [nan, nan, 2.0, nan][:len(rem)], cands, 1) == ([20], [2.0])
    assert greedy(lambda ch, rem: [nan] * len(rem), cands, 2)[0] == [30, 10]
    # ties over the whole round: `candidates` order
    assert greedy(lambda ch, rem: [1.0] * len(rem), cands, 3)[0] == [30, 10, 20]
    # an infinite score is a number: it beats NaN
    assert greedy(lambda ch, rem: [nan, float("inf")][:len(rem)], [1, 2], 1) == ([2], [float("inf")])
    for bad in (5, -1, 1.5, None, True):
        with pytest.raises(ValueError, match="num"):
            greedy(table_scorer(rounds), cands, bad)
    with pytest.raises(ValueError, match="duplicates"):
        greedy(table_scorer(rounds), [1, 2, 1], 1)
    with pytest.raises(ValueError, match="scores"):
        greedy(lambda ch, rem: [1.0], cands, 1)


# ---- 4. refusals in Python ----------------------------------------------------------------------------------------------------------
def test_place_sensors_refusals_that_need_no_device(pkg):
    class Store:                                                 # (what place_sensors reads of a store before it builds anything)
        nodes_per_graph = 37

    place = pkg.PressureEstimator.place_sensors
    model = object()
    for bad in (0, -1, 9, 2.5, None, True):
        with pytest.raises(ValueError, match="num_sensors"):
            place(model, Store(), bad, candidates=[1, 2, 3, 4, 5, 6, 7, 8], fixed=[0])
    with pytest.raises(ValueError, match="num_sensors"):
        place(model, Store(), 37, fixed=[0])                     # candidates=None: the 36 other nodes
    with pytest.raises(ValueError, match="num_sensors"):
        place(model, Store(), 1, candidates=[])
    with pytest.raises(ValueError, match="overlap"):
        place(model, Store(), 1, candidates=[1, 2, 3], fixed=[3])
    for bad in ("mse", "MAE", None, 1):
        with pytest.raises(ValueError, match="criterion"):
            place(model, Store(), 1, candidates=[1, 2, 3], criterion=bad)
    with pytest.raises(ValueError, match="observed_idx"):
        place(model, Store(), 1, candidates=[1, 2, 37])          # outside [0, 37)
    with pytest.raises(ValueError, match="duplicates"):
        place(model, Store(), 1, candidates=[1, 2, 2])
    with pytest.raises(ValueError, match="duplicates"):
        place(model, Store(), 1, candidates=[1, 2], fixed=[5, 5])
    multi = pkg.MultiSnapshotStore.__new__(pkg.MultiSnapshotStore)
    with pytest.raises(ValueError, match="MultiSnapshotStore"):
        place(model, multi, 1, candidates=[1, 2])
