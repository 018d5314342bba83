"""The chunked checker (tests/_spot_stream_reference.py) against the whole-stream checker (tests/_spot_reference.py), without a GPU:
sequential chunks that carry the last column are the very same table, bit for bit, whatever the cuts -- the claim the streaming
session (include/apd.h, "streaming spotting") rests on, and the reason the GPU tests may compare a session with either checker."""
import numpy as np
import pytest

import _spot_reference as ref
import _spot_stream_reference as sref

F = np.float32
UNIT = (1.0, 1.0, 1.0)
SKEWED = (1.0, 2.0, 0.5)                        # (insertion, deletion, match)
M = 12


def integer_pair(seed, n=5, m=M, dim=2):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 3, (n, dim)).astype(F), rng.integers(0, 3, (m, dim)).astype(F)      # tie-rich


def gauss_pair(seed, n=7, m=M, dim=3):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, dim)).astype(F), rng.standard_normal((m, dim)).astype(F)


PAIRS = {"integer": integer_pair(11), "integer-long-query": integer_pair(12, n=9), "gauss": gauss_pair(13)}
CUTS = [(k, M - k) for k in range(1, M)] + [(1,) * M, (0, 5, 0, 0, 7, 0), (M, 0), (0, M)]


def assert_chunked_equals_whole(x, y, pen, sizes, first_column=0):
    want_cost, want_start, _ = ref.spot(x, y, *pen)
    want_start = np.where(want_start > 0, want_start + first_column, 0).astype(np.uint32)
    prefix = sref.prefix_bests(want_cost, want_start, len(x), first_column)
    pushes = sref.run(x, sref.split(y, sizes), *pen, first_column=first_column)
    cost = np.concatenate([p[0] for p in pushes])
    start = np.concatenate([p[1] for p in pushes])
    assert np.array_equal(sref.bits(cost), sref.bits(want_cost)), sizes
    assert np.array_equal(start, want_start), sizes
    done = 0
    for size, (_, _, best) in zip(sizes, pushes):
        done += size
        assert ref.same_best(best, prefix[done]), (sizes, done, best, prefix[done])
    return pushes


@pytest.mark.parametrize("pen", [UNIT, SKEWED], ids=["unit", "skewed"])
@pytest.mark.parametrize("name", sorted(PAIRS))
def test_any_cut_gives_the_whole_streams_bits(name, pen):
    x, y = PAIRS[name]
    for sizes in CUTS:
        assert_chunked_equals_whole(x, y, pen, sizes)


def test_the_last_prefix_best_is_the_whole_streams_best():
    for name in sorted(PAIRS):
        x, y = PAIRS[name]
        cost, start, best = ref.spot(x, y)
        assert ref.same_best(sref.prefix_bests(cost, start, len(x))[-1], best)
        assert ref.same_best(sref.run(x, [y])[0][2], best)


def test_hand_case_the_tie_that_independent_pieces_get_wrong():
    x, y = np.array([[0], [1]], dtype=F), np.array([[0], [1], [0]], dtype=F)
    (c0, s0, _), (c1, s1, best) = sref.run(x, [y[:1], y[1:]])
    assert c0.tolist() == [1.0] and s0.tolist() == [1]
    assert c1.tolist() == [0.0, 2.0] and s1.tolist() == [1, 2]
    assert (best["end"], best["start"], best["cost"]) == (2, 1, 0.0)
    alone = ref.curves(x, y[1:])                                   # columns 2..3 spotted on their own: another table
    assert alone[0].tolist()[-1] == 1.0


def test_a_zero_length_push_changes_nothing():
    x, y = PAIRS["integer"]
    s = sref.Session(x)
    s.push(y[:4])
    before = (list(s.col_t), list(s.col_s), s.column, s.best.copy())
    cost, start, best = s.push(y[:0])
    assert len(cost) == 0 and len(start) == 0 and ref.same_best(best, before[3])
    assert (list(s.col_t), list(s.col_s), s.column) == before[:3]


@pytest.mark.parametrize("name", sorted(PAIRS))
def test_first_column_shifts_starts_and_ends_and_no_cost_bit(name):
    x, y = PAIRS[name]
    for sizes in ((M,), (5, 7), (1,) * M):
        plain = assert_chunked_equals_whole(x, y, SKEWED, sizes)
        moved = assert_chunked_equals_whole(x, y, SKEWED, sizes, first_column=1000)
        for (c0, s0, b0), (c1, s1, b1) in zip(plain, moved):
            assert np.array_equal(sref.bits(c0), sref.bits(c1))
            assert np.array_equal(np.where(s0 > 0, s0 + 1000, 0), s1)
            assert sref.bits(b0["cost"]) == sref.bits(b1["cost"]) and sref.bits(b0["score"]) == sref.bits(b1["score"])
            if b0["end"]:
                assert (b1["end"], b1["start"]) == (b0["end"] + 1000, b0["start"] + 1000)


def test_reset_starts_a_fresh_table():
    x, y = PAIRS["gauss"]
    s = sref.Session(x)
    s.push(y)
    s.reset()
    cost, start, best = s.push(y)
    want = ref.spot(x, y)
    assert np.array_equal(sref.bits(cost), sref.bits(want[0])) and np.array_equal(start, want[1]) and ref.same_best(best, want[2])
