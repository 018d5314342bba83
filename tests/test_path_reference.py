"""CPU tests of the warping-path checker (tests/_path_reference.py) and of the host side of the path entry points.

The checker is what tests/test_gpu_paths.py compares the kernels with bit for bit, so it is pinned here first: its score equals the
C oracle's and the second-opinion numpy oracle's on 60 random cases, its paths have the shape the contract states, and its costs
are what a forward replay of the path gives."""
import ctypes as C

import numpy as np
import pytest

import _path_reference as ref
from oracle import np_reference

PENALTIES = ((1.0, 1.0, 1.0), (1.5, 0.75, 1.25))          # (insertion, deletion, match)


def random_cases():
    """60 cases: n, m <= 90 (lengths 1 and 2 among them), D in {1, 3, 13}, integer and Gaussian features, bands {0, 2, 5, 200},
    unit and non-unit penalties."""
    rng = np.random.default_rng(20260)
    cases = []
    for t in range(60):
        dim = (1, 3, 13)[t % 3]
        n, m = int(rng.integers(1, 91)), int(rng.integers(1, 91))
        if t % 10 == 0:
            n = 1 + (t // 10) % 2                           # lengths 1 and 2 against anything
        if t == 30:
            n = m = 1
        if t % 4 < 2:
            x, y = rng.integers(-2, 3, (n, dim)), rng.integers(-2, 3, (m, dim))
        else:
            x, y = rng.standard_normal((n, dim)), rng.standard_normal((m, dim))
        cases.append((x.astype(np.float32), y.astype(np.float32), (0, 2, 5, 200)[(t // 3) % 4], PENALTIES[(t // 2) % 2]))
    return cases


@pytest.fixture(scope="module")
def cases():
    return [(x, y, band, pen, ref.path(x, y, band, *pen)) for x, y, band, pen in random_cases()]


def test_checker_score_equals_both_oracles(oracle, cases):
    for x, y, band, (ins, dele, match), (steps, score) in cases:
        want = np.float32(oracle.dtw_pair(x, y, band, ins, dele, match))
        second = np.float32(np_reference.dtw_pair(x, y, band, ins, dele, match))
        assert np.float32(score).view(np.uint32) == want.view(np.uint32) == second.view(np.uint32), (len(x), len(y), band)


def test_checker_path_shape_and_replay(cases):
    seen_empty = seen_single = 0
    for x, y, band, pen, (steps, score) in cases:
        n, m = len(x), len(y)
        assert (len(steps) == 0) == ((n == 1) != (m == 1))                  # empty iff exactly one length is 1
        if len(steps) == 0:
            assert np.isposinf(score)
            seen_empty += 1
            continue
        assert np.isfinite(score)                                           # finite features: every present cell is finite
        assert tuple(steps[0]) == (0, 0, 0.0, ref.START)
        assert (int(steps[-1]["i"]), int(steps[-1]["j"])) == (n - 1, m - 1)
        assert len(steps) <= n + m - 1
        assert not np.any(steps["op"][1:] == ref.START)
        for a, b in zip(steps[:-1], steps[1:]):                             # every step leaves its predecessor by its own branch
            di, dj = ref.PRED[int(b["op"])]
            assert (int(b["i"]) + di, int(b["j"]) + dj) == (int(a["i"]), int(a["j"]))
        assert np.array_equal(ref.replay(x, y, steps, *pen).view(np.uint32), steps["cost"].view(np.uint32))
        seen_single += n == 1 and m == 1
    assert seen_empty >= 3 and seen_single == 1


def as_tuples(steps):
    return [(int(s["i"]), int(s["j"]), float(s["cost"]), int(s["op"])) for s in steps]


def test_hand_cases():
    M, I, S = ref.MATCH, ref.INSERT, ref.START
    x, y = np.array([[0], [1], [0], [0]], np.float32), np.array([[1], [0], [1], [0]], np.float32)
    steps, score = ref.path(x, y, 4)
    # the tie quirk: at (1,1) .. (3,3) DELETE and INSERT tie exactly and MATCH is taken although it is larger
    assert as_tuples(steps) == [(0, 0, 0.0, S), (1, 1, 1.0, M), (2, 2, 2.0, M), (3, 3, 3.0, M)]
    assert score == np.float32(0.375)
    x, y = np.array([[0], [1], [5]], np.float32), np.array([[0], [9]], np.float32)
    steps, score = ref.path(x, y, 3)
    assert as_tuples(steps) == [(0, 0, 0.0, S), (1, 1, 0.0, M), (2, 1, 1.0, I)]
    assert score == np.float32(0.2)
    steps, score = ref.path(np.zeros((1, 2), np.float32), np.ones((1, 2), np.float32), 0)
    assert as_tuples(steps) == [(0, 0, 0.0, S)] and score == 0.0
    steps, score = ref.path(np.zeros((1, 2), np.float32), np.ones((5, 2), np.float32), 9)
    assert len(steps) == 0 and np.isposinf(score)


def test_checker_walk_ends_early_on_a_nan_table():
    """A NaN frame poisons every cell after it; NaN compares false, so those cells take MATCH, and a walk that runs along the
    diagonal into row 0 or column 0 away from the origin stops there: the path does not start with START."""
    x, y = np.ones((6, 2), np.float32), np.ones((9, 2), np.float32)
    x[0, 0] = np.nan
    steps, score = ref.path(x, y, 20)
    assert len(steps) and steps[0]["op"] != ref.START and np.isnan(score)
    assert (int(steps[-1]["i"]), int(steps[-1]["j"])) == (5, 8) and np.all(steps["op"] == ref.MATCH)
    assert np.array_equal(ref.bits(ref.replay(x, y, steps)), ref.bits(steps["cost"]))


def test_path_bound(apd):
    L = apd.lib()
    for n, m, want in ((0, 0, 0), (0, 7, 0), (7, 0, 0), (1, 1, 1), (1, 9, 9), (4, 4, 7), (520, 530, 1049), (1 << 40, 3, (1 << 40) + 2)):
        assert L.apd_path_bound(n, m) == want
    assert C.sizeof(apd.PathStep) == 16
    assert (apd.APD_PATH_MATCH, apd.APD_PATH_INSERT, apd.APD_PATH_DELETE, apd.APD_PATH_START) == (0, 1, 2, 3)


def test_path_entry_points_refuse_a_null_context(apd):
    L = apd.lib()
    cfg = apd.AlignConfig(1.0, 1.0, 1.0, 1.0)
    pairs = (C.c_uint32 * 2)(0, 1)
    off = (C.c_uint64 * 2)()
    assert L.apd_align_paths(None, None, C.byref(cfg), pairs, 1, None, 0, off, None, None) == apd.APD_ERR_INVALID_ARG
    x = (C.c_float * 2)(0.0, 1.0)
    p = apd.AlignmentParamsC(2, 1.0, 1.0, 1.0)
    used, score = C.c_uint64(0), C.c_float(0)
    steps = (apd.PathStep * 3)()
    assert L.apd_align_pair_path(None, x, 2, x, 2, 1, C.byref(p), steps, 3, C.byref(used), C.byref(score)) == apd.APD_ERR_INVALID_ARG
