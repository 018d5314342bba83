"""CPU tests of the contract of apd_spot_paths (include/apd.h, "warping paths of spotted windows") as tests/_spot_path_reference.py
restates it: the hand cases, the tie quirk that makes a table of the window alone a different table, the invariants of the walk over
seeded random small cases, and apd_spot_path_bound -- host only -- through the loaded library.  No GPU."""
import numpy as np
import pytest

import _spot_path_reference as ref
import _spot_reference as spot_ref

F = np.float32
M, I, D, S = ref.MATCH, ref.INSERT, ref.DELETE, ref.START
UNIT = (1.0, 1.0, 1.0)
SKEWED = (1.0, 2.0, 0.5)                        # (insertion, deletion, match)


def col(values):
    return np.array(values, dtype=F).reshape(-1, 1)


def as_tuples(steps):
    return [(int(s["i"]), int(s["j"]), float(s["cost"]), int(s["op"])) for s in steps]


HAND_X, HAND_Y = col([1, 2]), col([5, 1, 2, 5])
HAND = {1: [(0, 0, 0.0, S), (1, 1, 4.0, M), (2, 1, 7.0, I)],
        2: [(0, 1, 0.0, S), (1, 2, 0.0, M), (2, 2, 1.0, I)],
        3: [(0, 1, 0.0, S), (1, 2, 0.0, M), (2, 3, 0.0, M)],
        4: [(0, 1, 0.0, S), (1, 2, 0.0, M), (2, 3, 0.0, M), (2, 4, 3.0, D)]}
QUIRK_X, QUIRK_Y = col([0, 1]), col([0, 1, 0])
QUIRK = [(0, 1, 0.0, S), (1, 2, 1.0, M), (2, 3, 2.0, M)]


def test_hand_cases():
    tab = ref.table(HAND_X, HAND_Y)
    cost, start = spot_ref.curves(HAND_X, HAND_Y)
    for end, want in HAND.items():
        steps, found, score = ref.answer(tab, 2, end, int(start[end - 1]))
        assert as_tuples(steps) == want
        assert found == start[end - 1] and steps["cost"][-1] == cost[end - 1]
        assert score == spot_ref.scores(cost, start, 2)[end - 1]


def test_the_tie_quirk_makes_the_window_alone_another_table():
    cost, start = spot_ref.curves(QUIRK_X, QUIRK_Y)
    assert (int(start[2]), float(cost[2])) == (2, 2.0)
    tab = ref.table(QUIRK_X, QUIRK_Y)
    steps, found, _ = ref.answer(tab, 2, 3, 2)
    assert as_tuples(steps) == QUIRK and found == 2
    alone = ref.table(QUIRK_X, QUIRK_Y, first=2)                                # the same recurrence on columns 2..3 only
    assert float(alone[0][2][3]) == 1.0
    other, _ = ref.walk(alone, 2, 3)
    assert as_tuples(other) != QUIRK
    # the window cut out and aligned on its own: the same other table
    cut = ref.table(QUIRK_X, QUIRK_Y[1:])
    assert float(cut[0][2][2]) == 1.0


def test_a_wrong_or_absent_start_gets_no_path():
    tab = ref.table(HAND_X, HAND_Y)
    steps, found, score = ref.answer(tab, 2, 3, 3)                              # the table's start is 2
    assert len(steps) == 0 and found == 2 and score == 0.0
    steps, found, score = ref.answer(tab, 2, 0, 0)
    assert len(steps) == 0 and found == 0 and np.isposinf(score)


def random_cases():
    rng = np.random.default_rng(2024)
    for k in range(240):
        n, m, dim = int(rng.integers(1, 7)), int(rng.integers(1, 12)), int(rng.integers(1, 4))
        kind = k % 3
        if kind == 0:
            x, y = rng.integers(0, 3, (n, dim)).astype(F), rng.integers(0, 3, (m, dim)).astype(F)
        else:
            x, y = rng.standard_normal((n, dim)).astype(F), rng.standard_normal((m, dim)).astype(F)
        if kind == 2:
            y[int(rng.integers(0, m)), :] = (np.nan, np.inf)[k % 2]
        yield x, y, (UNIT, SKEWED)[(k // 3) % 2]


def test_walk_invariants_over_random_small_cases():
    windows = longest = 0
    for x, y, pen in random_cases():
        n, m = len(x), len(y)
        tab = ref.table(x, y, *pen)
        cost, start = spot_ref.curves(x, y, *pen)
        assert np.array_equal([tab[1][n][j] for j in range(1, m + 1)], start)    # the same table as the spotting checker's
        assert np.array_equal(ref.bits([tab[0][n][j] for j in range(1, m + 1)]), ref.bits(cost))
        for end in range(1, m + 1):
            first = int(start[end - 1])
            steps, entered = ref.walk(tab, n, end)
            assert entered == (first == 0)                                      # S = 0 exactly when the walk would enter column 0
            if first == 0:
                continue
            windows += 1
            length = end - first + 1
            assert max(n, length) + 1 <= len(steps) <= n + length == ref.bound(n, end, first)
            longest += len(steps) == n + length
            assert steps[0]["op"] == S and steps[0]["i"] == 0 and steps[0]["j"] in (first - 1, first) and steps[0]["cost"] == 0.0
            assert (int(steps[1]["i"]), int(steps[1]["j"])) == (1, first) and steps[1]["op"] in (M, I)
            assert steps[0]["j"] == (first - 1 if steps[1]["op"] == M else first)
            assert (int(steps[-1]["i"]), int(steps[-1]["j"])) == (n, end)
            assert np.all(steps["j"][1:] >= first) and np.all(steps["j"] <= end) and np.all(steps["j"][1:] >= 1)
            assert ref.bits(steps["cost"][-1:])[0] == ref.bits(cost[end - 1:end])[0]
            assert np.array_equal(ref.bits(ref.replay(x, y, steps, *pen)), ref.bits(steps["cost"]))
            for a, b in zip(steps[:-1], steps[1:]):
                assert (int(b["i"]) - int(a["i"]), int(b["j"]) - int(a["j"])) == {M: (1, 1), I: (1, 0), D: (0, 1)}[int(b["op"])]
            got, found, score = ref.answer(tab, n, end, first)
            assert ref.same_steps(got, steps) and found == first
            assert ref.bits([score])[0] == ref.bits(spot_ref.scores(cost, start, n)[end - 1:end])[0]
    assert windows > 1000 and longest > 0                                       # the upper bound n + L is reached


@pytest.mark.parametrize("n, end, start, want", [(1, 1, 1, 2), (5, 9, 3, 12), (5, 9, 0, 0), (5, 0, 3, 0), (5, 3, 9, 0), (0, 9, 3, 0)])
def test_bound_through_the_library(apd, n, end, start, want):
    assert ref.bound(n, end, start) == want
    assert apd.lib().apd_spot_path_bound(n, end, start) == want
