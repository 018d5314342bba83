"""The checker of apd_cross_linkage against itself, no GPU: the loop with the first-set sequences as an array axis
(_linkage_reference.reference_over_q) gives the bits of the scalar loop."""
import numpy as np

from _linkage_reference import F, NONE, assert_equal, reference, reference_over_q, six_set_case


def test_the_loop_over_q_as_an_array_equals_the_scalar_loop():
    fs, sf, sets = six_set_case()
    want = reference(fs, sf, sets)
    assert_equal(reference_over_q(fs, sf, sets), want, "six sets")
    listed = reference(fs, sf, sets, ascending=False)
    assert (want[0].view(np.uint32) != listed[0].view(np.uint32)).sum() > 0              # the order of the chain shows in the bits
    # an empty set (NaN, never chosen), +INF members, exact ties, no set at all
    with_empty = [sets[2], [], sets[0]]
    assert_equal(reference_over_q(fs, sf, with_empty), reference(fs, sf, with_empty), "an empty set")
    fs_inf, sf_inf = fs.copy(), sf.copy()
    fs_inf[:, sets[2][3]] = np.inf
    sf_inf[sets[3][7], :] = np.inf
    assert_equal(reference_over_q(fs_inf, sf_inf, sets), reference(fs_inf, sf_inf, sets), "+INF members")
    fs_t, sf_t = np.full(fs.shape, 2.0, F), np.full(sf.shape, 2.0, F)
    sf_t[2, :] = 1.0
    tie_sets = [[5, 9, 1], [7, 3], [2]]
    got = reference_over_q(fs_t, sf_t, tie_sets)
    assert_equal(got, reference(fs_t, sf_t, tie_sets), "ties")
    assert np.all(got[2] == 2) and np.all(got[3] == 1.0)
    none = reference_over_q(fs, sf, [])
    assert none[0].shape == (fs.shape[0], 0) and np.all(none[2] == NONE) and np.all(np.isposinf(none[3]))
