"""CPU side of density clustering: the numpy restatement of apd_density_clusters' contract (tests/_density_reference.py) pinned by
hand-worked cases and, where scikit-learn is installed, against DBSCAN(metric="precomputed"); density_sets against its definition;
and the library's export of the entry point."""
import numpy as np
import pytest

from _density_reference import (BORDER, BOTH, CORE, EITHER, F, NOISE, adjacency, blob_matrix, border_tie_matrix, density_reference,
                                density_sets_reference)

INF, NAN = F(np.inf), F(np.nan)


def line(*xs):
    x = np.array(xs, F)
    return np.abs(x[:, None] - x[None, :]).astype(F)


def test_three_points_on_a_line():
    d = line(0, 1, 2)                                                         # 0 - 1 - 2 with eps 1: degrees 1, 2, 1
    labels, kind, degree, counts, nans = density_reference(d, 1.0, 2)
    assert degree.tolist() == [1, 2, 1] and kind.tolist() == [CORE] * 3 and labels.tolist() == [0, 0, 0]
    assert counts.tolist() == [1, 3, 0, 0] and nans == 0
    labels, kind, degree, counts, _ = density_reference(d, 1.0, 3)            # only the middle point has two neighbours
    assert kind.tolist() == [BORDER, CORE, BORDER] and labels.tolist() == [1, 1, 1] and counts.tolist() == [1, 1, 2, 0]
    labels, kind, _, counts, _ = density_reference(d, 0.5, 2)
    assert kind.tolist() == [NOISE] * 3 and labels.tolist() == [0, 1, 2] and counts.tolist() == [0, 0, 0, 3]


def test_a_border_point_between_two_clusters_takes_the_smaller_label():
    labels, kind, degree, counts, _ = density_reference(border_tie_matrix(), 0.5, 3)
    assert degree.tolist() == [2, 2, 3, 2, 2, 2, 3]
    assert kind.tolist() == [CORE] * 7 and len(set(labels.tolist())) == 1    # min_pts 3: 0 is core and joins the two
    labels, kind, degree, counts, _ = density_reference(border_tie_matrix(), 0.5, 4)
    assert kind.tolist() == [BORDER, BORDER, CORE, BORDER, BORDER, BORDER, CORE]
    assert labels.tolist() == [2, 2, 2, 2, 6, 6, 6] and counts.tolist() == [2, 2, 5, 0]   # 0 sees cores 2 and 6: label 2


def test_an_asymmetric_pair():
    d = np.array([[0, 1], [5, 0]], F)
    labels, kind, degree, counts, _ = density_reference(d, 2.0, 2, EITHER)
    assert labels.tolist() == [0, 0] and degree.tolist() == [1, 1] and counts.tolist() == [1, 2, 0, 0]
    labels, kind, degree, counts, _ = density_reference(d, 2.0, 2, BOTH)
    assert labels.tolist() == [0, 1] and degree.tolist() == [0, 0] and counts.tolist() == [0, 0, 0, 2]


def test_special_values():
    d = np.array([[0, -0.0, 3], [1, 0, 3], [3, 3, 0]], F)                     # eps = 0: the -0.0 entry is near, 1 is not
    labels, _, degree, counts, _ = density_reference(d, 0.0, 2, EITHER)
    assert degree.tolist() == [1, 1, 0] and labels.tolist() == [0, 0, 2] and counts.tolist() == [1, 2, 0, 1]
    assert density_reference(d, 0.0, 2, BOTH)[2].tolist() == [0, 0, 0]
    assert density_reference(d, -0.0, 2, EITHER)[2].tolist() == [1, 1, 0]     # and a -0.0 eps equals a +0.0 entry's
    d = np.array([[0, NAN, 1], [1, 0, NAN], [INF, 1, NAN]], F)                # a NaN entry is never near, and is counted off the diagonal
    labels, _, degree, counts, nans = density_reference(d, 1.0, 2, EITHER)
    assert nans == 2 and degree.tolist() == [2, 2, 2] and labels.tolist() == [0, 0, 0]
    assert density_reference(d, 1.0, 2, BOTH)[2].tolist() == [0, 0, 0]
    labels, _, degree, counts, nans = density_reference(d, INF, 3, BOTH)      # eps = +INF: every non-NaN entry, +INF included
    assert adjacency(d, INF, BOTH).tolist() == [[False, False, True], [False, False, False], [True, False, False]]
    assert degree.tolist() == [1, 0, 1] and counts.tolist() == [0, 0, 0, 3] and nans == 2
    assert density_reference(d, INF, 3, EITHER)[3].tolist() == [1, 3, 0, 0]
    labels, kind, degree, counts, nans = density_reference(line(0, 1, 2), NAN, 1)   # a NaN eps: nothing is near
    assert degree.tolist() == [0, 0, 0] and kind.tolist() == [CORE] * 3 and counts.tolist() == [3, 3, 0, 0] and nans == 0


def test_min_pts_one_and_min_pts_beyond_n():
    d = line(0, 1, 5)
    labels, kind, _, counts, _ = density_reference(d, 1.0, 1)                 # every point is core; the lone one is its own cluster
    assert kind.tolist() == [CORE] * 3 and labels.tolist() == [0, 0, 2] and counts.tolist() == [2, 3, 0, 0]
    labels, kind, _, counts, _ = density_reference(d, INF, 4)                 # n + 1: nobody can be core
    assert kind.tolist() == [NOISE] * 3 and labels.tolist() == [0, 1, 2] and counts.tolist() == [0, 0, 0, 3]
    labels, kind, _, counts, _ = density_reference(d, INF, 3)
    assert kind.tolist() == [CORE] * 3 and counts.tolist() == [1, 3, 0, 0]
    labels, kind, degree, counts, nans = density_reference(np.zeros((0, 0), F), 1.0, 1)
    assert len(labels) == len(kind) == len(degree) == 0 and counts.tolist() == [0, 0, 0, 0] and nans == 0
    labels, kind, degree, counts, nans = density_reference(np.array([[NAN]], F), 1.0, 1)   # the diagonal is not counted
    assert labels.tolist() == [0] and kind.tolist() == [CORE] and counts.tolist() == [1, 1, 0, 0] and nans == 0


SETTINGS = ((0.3, 4), (0.5, 6), (0.2, 3))


@pytest.mark.parametrize("n", (193, 321))
def test_against_scikit_learn(n):
    cluster = pytest.importorskip("sklearn.cluster")
    d = blob_matrix(n, seed=n)
    assert np.array_equal(d, d.T)
    for eps, min_pts in SETTINGS:
        labels, kind, degree, counts, nans = density_reference(d, eps, min_pts)
        assert counts[0] >= 2 and counts[1] and counts[2] and counts[3], "a degenerate input: %r" % (counts,)
        model = cluster.DBSCAN(eps=float(F(eps)), min_samples=min_pts, metric="precomputed").fit(d.astype(np.float64))
        theirs = model.labels_
        core = np.zeros(n, bool)
        core[model.core_sample_indices_] = True
        assert np.array_equal(core, kind == CORE)
        assert np.array_equal(theirs == -1, kind == NOISE)
        pairs = set(zip(labels[core].tolist(), theirs[core].tolist()))        # the same partition of the core points: a bijection
        assert len(pairs) == len({p for p, _ in pairs}) == len({q for _, q in pairs}) == counts[0]
        adj = adjacency(d, eps, EITHER)
        for i in np.flatnonzero(kind == BORDER):                              # theirs depends on the visiting order: any core neighbour's
            assert theirs[i] in set(theirs[np.flatnonzero(adj[i] & core)].tolist())
            assert labels[i] == labels[np.flatnonzero(adj[i] & core)].min()


def test_the_generator_gives_all_three_kinds_in_both_links():
    for n in (127, 129, 193):
        d = blob_matrix(n, seed=n, asymmetric=True)
        assert not np.array_equal(d, d.T)
        for link in (EITHER, BOTH):
            counts = density_reference(d, 0.3, 4, link)[3]
            assert counts[0] >= 2 and counts[1] and counts[2] and counts[3], (n, link, counts)


def test_density_sets():
    from audio_pattern_discovery_amd.clustering import density_sets
    for n, eps, min_pts in ((193, 0.3, 4), (65, 0.5, 6), (7, 0.01, 2)):
        labels, kind, *_ = density_reference(blob_matrix(n, seed=3), eps, min_pts)
        members, set_off = density_sets(labels, kind)
        want_members, want_off = density_sets_reference(labels, kind)
        assert members.dtype == set_off.dtype == np.uint32
        assert np.array_equal(members, want_members) and np.array_equal(set_off, want_off)
        assert len(members) == (kind != NOISE).sum() and len(set_off) == len(np.unique(labels[kind != NOISE])) + 1
    members, set_off = density_sets([2, 2, 2, 2, 6, 6, 6], [1, 1, 2, 1, 1, 1, 2])
    assert members.tolist() == [0, 1, 2, 3, 4, 5, 6] and set_off.tolist() == [0, 4, 7]
    members, set_off = density_sets([6, 1, 6, 3, 0], [2, 0, 1, 0, 2])         # sets ascend by label, noise is left out
    assert members.tolist() == [4, 0, 2] and set_off.tolist() == [0, 1, 3]
    members, set_off = density_sets([], [])
    assert len(members) == 0 and set_off.tolist() == [0]


def test_the_library_exports_the_entry_point(apd):
    L = apd.lib()
    assert L.apd_density_clusters is not None
    assert (apd.APD_DENSITY_EITHER, apd.APD_DENSITY_BOTH, apd.APD_DENSITY_MAX_SETTINGS) == (0, 1, 8)
    assert (apd.APD_DENSITY_NOISE, apd.APD_DENSITY_BORDER, apd.APD_DENSITY_CORE) == (NOISE, BORDER, CORE) == (0, 1, 2)
    # argument errors are answered before the device is touched
    import ctypes as C
    eps, min_pts = (C.c_float * 1)(1.0), (C.c_uint32 * 1)(2)
    assert L.apd_density_clusters(None, None, 0, 0, 0, eps, min_pts, 1, None, None, None, None, None) == apd.APD_ERR_INVALID_ARG
