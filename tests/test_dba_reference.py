"""Pins the prototype checker (tests/_dba_reference.py) with answers worked by hand: it is what tests/test_gpu_prototypes.py
compares the GPU against, so it has to be right on its own.  No GPU, no library."""
import numpy as np

import _dba_reference as dba
import _path_reference as ref

F = np.float32


def col(*values):
    return np.array(values, dtype=F).reshape(-1, 1)


def test_barycenter_known_answer():
    """D = 1, a = [0,2,9], b = [0,4,9], init a, full band, unit penalties.  (c = a, y = a): the diagonal, score 0; (c = a, y = b):
    (1,1) = 0, (2,2) = 0 + |2 - 4| = 2 by MATCH (DELETE would come from (2,1) = 2, INSERT from (1,2) = 4), score 2 / 6.  Row 1
    averages 0 and 0, row 2 averages 2 and 4; row 3 is never on a path that ends at (n-1, m-1) and keeps 9."""
    a, b = col(0, 2, 9), col(0, 4, 9)
    out, inertia, used = dba.barycenters([a, b], [[0, 1]], [0], 1.0, iterations=1)
    assert out[0].tolist() == [[0.0], [3.0], [9.0]]
    assert used.tolist() == [[2]]
    assert inertia[0, 0] == F(F(F(2.0) / F(6.0)) / F(2.0)) == F(1.0 / 6.0)
    # the member order inside a set does not matter
    again, inertia2, _ = dba.barycenters([a, b], [[1, 0]], [0], 1.0, iterations=1)
    assert again[0].tobytes() == out[0].tobytes() and inertia2.tobytes() == inertia.tobytes()


def test_zero_iterations_is_the_identity():
    a, b = col(0.5, -2, 9, 4), col(0, 4, 9)
    out, inertia, used = dba.barycenters([a, b], [[0, 1], [1]], [0, 1], 1.0, iterations=0)
    assert out[0].tobytes() == a.tobytes() and out[1].tobytes() == b.tobytes()
    assert inertia.shape == (0, 2) and used.shape == (0, 2)


def test_one_frame_member_is_skipped():
    a, b, one = col(0, 2, 9), col(0, 4, 9), col(7)
    with_one, inertia, used = dba.barycenters([a, b, one], [[0, 1, 2]], [0], 1.0, iterations=1)
    without, inertia0, used0 = dba.barycenters([a, b, one], [[0, 1]], [0], 1.0, iterations=1)
    assert used.tolist() == [[2]] and used0.tolist() == [[2]]                   # three members, two contribute
    assert np.isfinite(inertia[0, 0]) and inertia.tobytes() == inertia0.tobytes()
    assert with_one[0].tobytes() == without[0].tobytes()
    # nothing contributes: the barycenter stays, the inertia is +INF
    alone, inertia1, used1 = dba.barycenters([a, b, one], [[2]], [0], 1.0, iterations=2)
    assert alone[0].tobytes() == a.tobytes() and used1.tolist() == [[0], [0]] and np.all(np.isposinf(inertia1))


def test_one_frame_barycenter_keeps_its_frame():
    a, b, one, other = col(0, 2, 9), col(0, 4, 9), col(7), col(5)
    out, inertia, used = dba.barycenters([a, b, one, other], [[0, 1, 3]], [2], 1.0, iterations=3)
    assert out[0].tolist() == [[7.0]]
    # only the one-frame member gives a path (the single START step, score 0); it averages nothing: row 1 is the score cell's row
    assert used.tolist() == [[1], [1], [1]] and inertia.tolist() == [[0.0], [0.0], [0.0]]


def test_empty_set():
    a = col(0, 2, 9)
    out, inertia, used = dba.barycenters([a], [[], [0]], [0, 0], 1.0, iterations=1)
    assert out[0].shape == (0, 1) and np.isposinf(inertia[0, 0]) and used[0, 0] == 0
    assert out[1].tobytes() == a.tobytes() and inertia[0, 1] == 0.0 and used[0, 1] == 1


def test_medoid_by_hand():
    """cost(0) = 0+0 + 1+2 + 4+8 = 15, cost(1) = 2+1 + 0+0 + 1+3 = 7, cost(2) = 8+4 + 3+1 + 0+0 = 16."""
    d = np.array([[0, 1, 4], [2, 0, 1], [8, 3, 0]], dtype=F)
    medoid, cost = dba.medoids(d, [[0, 1, 2], [2, 0], [1], []])
    assert medoid.tolist() == [1, 0, 1, dba.NONE]                               # {0, 2}: 12 and 12, the smaller index
    assert cost.tolist()[:3] == [7.0, 12.0, 0.0] and np.isposinf(cost[3])


def test_medoid_adds_one_term_at_a_time():
    """cost(0) over {0,1,2} = (((2^24 + 1) + 1) + 0: each + 1 is lost to rounding; any other association gives 2^24 + 2."""
    d = np.zeros((3, 3), dtype=F)
    d[0, 1], d[1, 0], d[0, 2] = 2.0 ** 24, 1.0, 1.0
    d[1, 2] = d[2, 1] = 2.0 ** 25                                               # keeps the others away
    medoid, cost = dba.medoids(d, [[2, 1, 0]])
    assert medoid[0] == 0 and cost[0] == F(2.0 ** 24)


def test_medoid_never_keeps_a_nan():
    d = np.array([[0, 5, 5], [1, np.nan, 1], [5, 5, 0]], dtype=F)              # member 1 would win with a zero diagonal
    medoid, cost = dba.medoids(d, [[0, 1, 2]])
    assert medoid[0] == 0 and cost[0] == 16.0                                   # 0+0 + 5+1 + 5+5; member 2 ties and loses
    d[1, :] = np.nan                                                            # a NaN row poisons every cost of a set that holds it
    medoid, cost = dba.medoids(d, [[0, 1, 2], [0, 2]])
    assert medoid.tolist() == [dba.NONE, 0] and np.isposinf(cost[0]) and cost[1] == 10.0
    assert ref.bits(cost)[0] == 0x7F800000
