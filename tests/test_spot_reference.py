"""CPU tests of the subsequence-alignment checker (tests/_spot_reference.py) and of apd_spot_hits, which is host only.

The checker is what tests/test_gpu_spot.py compares the kernels with bit for bit, so it is pinned here first: the two hand-worked
cases of the contract, the prefix property (column j depends on columns <= j only) and, for a one-frame stream, the plain
recurrence.  apd_spot_hits runs without a GPU and is compared with the checker's own peak picking."""
import ctypes as C

import numpy as np
import pytest

import _spot_reference as ref

F = np.float32


def col(values):
    return np.array(values, dtype=F).reshape(-1, 1)


def test_hand_cases():
    cost, start, best = ref.spot(col([1, 2]), col([5, 1, 2, 5]))
    assert cost.tolist() == [7.0, 1.0, 0.0, 3.0] and start.tolist() == [1, 2, 2, 2]
    assert np.array_equal(ref.scores(cost, start, 2), np.array([F(7) / F(3), F(1) / F(3), F(0), F(3) / F(5)], dtype=F))
    assert (int(best["end"]), int(best["start"]), float(best["cost"]), float(best["score"])) == (3, 2, 0.0, 0.0)
    # the tie quirk: cell (2, 3) has del == ins == 0 < match == 1 and takes MATCH: 2, where the minimum rule would give 1
    cost, start, _ = ref.spot(col([0, 1]), col([0, 1, 0]))
    assert cost.tolist() == [1.0, 0.0, 2.0] and start.tolist() == [1, 1, 2]


def test_one_frame_query_and_one_frame_stream():
    x, y = col([3]), col([1, 3, 7])
    cost, start, best = ref.spot(x, y)
    assert cost.tolist() == [2.0, 0.0, 4.0] and start.tolist() == [1, 2, 3]         # row 1: every column starts its own window
    assert (int(best["end"]), int(best["start"])) == (2, 2) and best["score"] == 0.0
    cost, start, best = ref.spot(col([1, 2, 4]), col([2]))                           # m < n: one column, INSERT down from (1, 1)
    assert cost.tolist() == [1.0 + 0.0 + 2.0] and start.tolist() == [1]
    assert best["score"] == F(3.0) / F(3 + 1)


def test_nothing_kept_and_nan():
    x, y = col([1, 2]), col([np.nan, np.nan])
    cost, start, best = ref.spot(x, y)
    assert np.isnan(cost).all()
    assert (int(best["end"]), int(best["start"])) == (0, 0) and np.isposinf(best["cost"]) and np.isposinf(best["score"])
    y = col([np.nan, 1, 2, 9])
    cost, start, best = ref.spot(x, y)
    assert np.isnan(cost[0]) and np.isfinite(cost[2]) and int(best["end"]) == 3     # the NaN column is never kept


@pytest.mark.parametrize("dim,integer", [(1, True), (13, False)])
def test_prefix_property(dim, integer):
    rng = np.random.default_rng(5 + dim)
    make = (lambda n: rng.integers(0, 3, (n, dim)).astype(F)) if integer else (lambda n: rng.standard_normal((n, dim)).astype(F))
    x, y = make(9), make(40)
    for pen in ((1.0, 1.0, 1.0), (1.0, 2.0, 0.5)):
        cost, start = ref.curves(x, y, *pen)
        for k in (1, 2, 17, 39):
            c, s = ref.curves(x, y[:k], *pen)
            assert np.array_equal(ref.bits(c), ref.bits(cost[:k])) and np.array_equal(s, start[:k])
        assert np.all(start >= 1) and np.all(start <= np.arange(1, 41))


def raw_hits(apd, cost, start, n, threshold, capacity):
    cost, start = np.ascontiguousarray(cost, dtype=F), np.ascontiguousarray(start, dtype=np.uint32)
    hits = np.full((capacity + 1) * 16, 0x55, dtype=np.uint8).view(ref.BEST)        # one record more than asked: a canary
    count = C.c_uint64(99)
    rc = apd.lib().apd_spot_hits(cost.ctypes.data_as(C.POINTER(C.c_float)), start.ctypes.data_as(C.POINTER(C.c_uint32)), len(cost), n,
                                 threshold, hits.ctypes.data_as(C.POINTER(apd.SpotBest)), capacity, C.byref(count))
    assert hits[-1]["end"] == 0x55555555
    return rc, hits[:min(capacity, count.value)].copy(), count.value


def test_spot_hits_strict_threshold_tie_order_and_overlap(apd):
    # n = 1, start == end: score = cost / 2.  Columns 2 and 5 tie at 0.5, column 4 scores exactly the threshold.
    cost = np.array([4.0, 1.0, 3.0, 2.0, 1.0, np.nan], dtype=F)
    start = np.arange(1, 7, dtype=np.uint32)
    rc, hits, count = raw_hits(apd, cost, start, 1, 1.0, 8)
    assert rc == apd.APD_OK and count == 2
    assert [(int(h["end"]), int(h["start"]), float(h["cost"]), float(h["score"])) for h in hits] == [(2, 2, 1.0, 0.5), (5, 5, 1.0, 0.5)]
    # overlap: [2, 4] (score 0) is accepted first; [4, 5] and [1, 2] touch it, [5, 6] does not
    cost = np.array([1.0, 9.0, 9.0, 0.0, 1.0, 2.0], dtype=F)
    start = np.array([1, 1, 3, 2, 4, 5], dtype=np.uint32)
    rc, hits, count = raw_hits(apd, cost, start, 3, 100.0, 8)
    assert rc == apd.APD_OK
    assert [(int(h["end"]), int(h["start"])) for h in hits] == [(4, 2), (1, 1), (6, 5)]
    assert ref.same_best(hits, ref.hits(cost, start, 3, 100.0))


def test_spot_hits_capacity_overflow_count_and_nan(apd):
    rng = np.random.default_rng(9)
    cost = rng.integers(0, 6, 200).astype(F)
    cost[::17] = np.nan
    end = np.arange(1, 201)
    start = (end - rng.integers(0, 4, 200)).clip(1).astype(np.uint32)
    want = ref.hits(cost, start, 5, 0.4)
    assert len(want) > 6 and not np.isnan(want["score"]).any()
    rc, hits, count = raw_hits(apd, cost, start, 5, 0.4, 256)
    assert rc == apd.APD_OK and count == len(want) and ref.same_best(hits, want)
    rc, hits, count = raw_hits(apd, cost, start, 5, 0.4, 3)                         # *n_hits may exceed capacity
    assert rc == apd.APD_OK and count == len(want) and ref.same_best(hits, want[:3])
    rc, _, count = raw_hits(apd, cost, start, 5, -1.0, 4)
    assert rc == apd.APD_OK and count == 0
    rc, _, count = raw_hits(apd, cost, start, 5, float("nan"), 4)                   # nothing is below NaN
    assert rc == apd.APD_OK and count == 0
    from audio_pattern_discovery_amd.alignments import SPOT_BEST, spot_hits
    mine = spot_hits(cost, start, 5, 0.4)
    assert mine.dtype == SPOT_BEST and ref.same_best(mine, want)
    assert len(spot_hits(cost[:0], start[:0], 5, 0.4)) == 0


def test_spot_entry_points_refuse_bad_arguments(apd):
    L = apd.lib()
    assert C.sizeof(apd.SpotBest) == 16
    cost, start = (C.c_float * 2)(0.0, 1.0), (C.c_uint32 * 2)(1, 2)
    count = C.c_uint64(0)
    one = (apd.SpotBest * 1)()
    assert L.apd_spot_hits(cost, start, 2, 0, 1.0, one, 1, C.byref(count)) == apd.APD_ERR_INVALID_ARG      # n == 0
    assert L.apd_spot_hits(cost, start, 2, 1, 1.0, one, 1, None) == apd.APD_ERR_INVALID_ARG
    assert L.apd_spot_hits(None, start, 2, 1, 1.0, one, 1, C.byref(count)) == apd.APD_ERR_INVALID_ARG
    assert L.apd_spot_hits(cost, start, 2, 1, 1.0, None, 1, C.byref(count)) == apd.APD_ERR_INVALID_ARG
    bad = (C.c_uint32 * 2)(1, 3)                                                                           # a window that begins after its end
    assert L.apd_spot_hits(cost, bad, 2, 1, 9.0, one, 1, C.byref(count)) == apd.APD_ERR_INVALID_ARG
    cfg = apd.AlignConfig(1.0, 1.0, 1.0, 1.0)
    pairs, off = (C.c_uint32 * 2)(0, 1), (C.c_uint64 * 2)()
    assert L.apd_spot(None, None, C.byref(cfg), pairs, 1, None, None, 0, off, one) == apd.APD_ERR_INVALID_ARG
