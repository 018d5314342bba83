"""The checker of apd_neighbors against hand-written cases and against an independent formulation, no GPU: what
tests/test_gpu_neighbors.py compares the kernels with is itself pinned here."""
import numpy as np
import pytest

from _neighbors_reference import F, KINDS, PAD_BITS, PAD_INDEX, Ranked, assert_same, reference, reference_lexsort, values

NAN, INF = np.nan, np.inf


def bits(row):
    return np.array(row, F).view(np.uint32).tolist()


def test_ties_go_to_the_smaller_index():
    d = np.array([[3, 1, 2, 1, 1, 0]], F)
    index, distance, count, nans = reference(d, 4)
    assert index.tolist() == [[5, 1, 3, 4]] and distance.tolist() == [[0, 1, 1, 1]] and count.tolist() == [4] and nans.tolist() == [0]
    index, _, _, _ = reference(d, 2)
    assert index.tolist() == [[5, 1]]                                  # the cut falls inside the run of ties: the lowest index


def test_the_two_zeros_tie_and_keep_their_own_bits():
    d = np.array([[0.0, -0.0, 1.0, -0.0, 0.0, -1.0]], F)
    index, distance, count, _ = reference(d, 5)
    assert index.tolist() == [[5, 0, 1, 3, 4]] and count.tolist() == [5]
    assert distance.view(np.uint32).tolist() == [bits([-1.0, 0.0, -0.0, -0.0, 0.0])]   # index order among the zeros, signs as stored


def test_inf_is_a_candidate_behind_every_finite_value():
    d = np.array([[INF, 3e38, INF, -INF, 1.0]], F)
    index, distance, count, _ = reference(d, 5)
    assert index.tolist() == [[3, 4, 1, 0, 2]] and count.tolist() == [5]
    assert distance.view(np.uint32).tolist() == [bits([-INF, 1.0, 3e38, INF, INF])]


def test_nan_is_dropped_and_counted_and_an_all_nan_row_is_empty():
    d = np.array([[NAN, 2.0, NAN, 1.0], [NAN, NAN, NAN, NAN]], F)
    index, distance, count, nans = reference(d, 3)
    assert index.tolist() == [[3, 1, PAD_INDEX], [PAD_INDEX] * 3] and count.tolist() == [2, 0] and nans.tolist() == [2, 4]
    assert distance.view(np.uint32).tolist() == [bits([1.0, 2.0]) + [PAD_BITS], [PAD_BITS] * 3]
    assert reference(d, 3, skip_self=True)[3].tolist() == [1, 3]         # a skipped self entry is not counted, NaN or not


def test_k_beyond_the_row_pads_the_tail():
    d = np.array([[2.0, 1.0]], F)
    index, distance, count, _ = reference(d, 4)
    assert index.tolist() == [[1, 0, PAD_INDEX, PAD_INDEX]] and count.tolist() == [2]
    assert distance.view(np.uint32).tolist() == [bits([1.0, 2.0]) + [PAD_BITS] * 2]


def test_skip_self_is_a_plain_index_comparison_on_a_rectangular_matrix():
    d = np.array([[0, 5, 6], [5, 0, 6], [5, 6, 0], [1, 2, 3]], F)      # 4 x 3
    index, _, count, _ = reference(d, 3, skip_self=True)
    assert index.tolist() == [[1, 2, PAD_INDEX], [0, 2, PAD_INDEX], [0, 1, PAD_INDEX], [0, 1, 2]]   # row 3 has no entry 3
    assert count.tolist() == [2, 2, 2, 3]
    index, _, count, _ = reference(d, 4, axis=1, skip_self=True)         # column q ranks d[:, q] without entry q
    assert index.tolist() == [[3, 1, 2, PAD_INDEX], [3, 0, 2, PAD_INDEX], [3, 0, 1, PAD_INDEX]] and count.tolist() == [3, 3, 3]


def test_query_lists_answer_each_entry_on_its_own():
    d = values("ties", 9, 11, seed=1)
    full = reference(d, 4, skip_self=True)
    got = reference(d, 4, skip_self=True, queries=[7, 2, 7, 0])
    for part, whole in zip(got, full):
        assert np.array_equal(part, whole[[7, 2, 7, 0]])
    assert_same(Ranked(d.T.copy(), 0).take(5), reference(d, 5, axis=1), "columns are the rows of the transpose")


@pytest.mark.parametrize("kind", KINDS)
def test_the_sorted_loop_equals_a_lexsort(kind):
    for seed, (rows, cols) in enumerate(((7, 1), (9, 9), (5, 64), (6, 131))):
        d = values(kind, rows, cols, seed=100 + seed, k=8)
        for axis in (0, 1):
            for skip_self in (False, True):
                ranked = Ranked(d, axis, skip_self)
                for k in (1, 8, d.shape[1 - axis], d.shape[1 - axis] + 3):
                    assert_same(ranked.take(k), reference_lexsort(d, k, axis, skip_self), "%s %dx%d axis %d k %d" % (kind, rows, cols, axis, k))
