"""The density hierarchy without a GPU: the numpy restatement of its contract (tests/_density_tree_reference.py) against hand cases,
against the DBSCAN restatement of tests/_density_reference.py (the pinned property: a cut of the tree IS apd_density_clusters on the
core points) and against scipy's minimum spanning tree; and the library's host-only entry points apd_density_tree_cut and
apd_density_tree_operations against the restatement."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from _density_reference import BOTH, CORE, EITHER, F, blob_matrix, border_tie_matrix, density_reference
from _density_tree_reference import (cut_reference, keys, operations_reference, rounded_matrix, same_partition, special_matrix,
                                     tree_reference, values)

INF, NAN = F(np.inf), F(np.nan)
SIZES = (1, 2, 3, 7, 40, 65, 130)
KINDS = {"blobs": lambda n: blob_matrix(n, seed=n, asymmetric=True), "ties": lambda n: rounded_matrix(n, seed=n + 1),
         "special": lambda n: special_matrix(n, seed=n + 2)}


@functools.lru_cache(maxsize=None)
def tree_case(kind, n, link, min_pts):
    d = KINDS[kind](n)
    d.setflags(write=False)
    return d, tree_reference(d, min_pts, link)


def eps_of(tree):
    """Every distinct edge weight, and +-INF."""
    return [-INF] + np.unique(tree[3]).tolist() + [INF]


def test_keys_follow_the_order_and_come_back_canonical():
    v = np.array([-np.inf, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, np.inf, np.nan], F)
    k = keys(v)
    assert k[3] == k[4] and (np.diff(np.delete(k, 3).astype(np.int64)) > 0).all() and k[-1] == 0xFFFFFFFF
    back = values(k)
    assert np.array_equal(back.view(np.uint32)[:-1], np.where(v[:-1] == 0, F(0.0), v[:-1]).view(np.uint32))
    assert back.view(np.uint32)[-1] == 0x7FC00000
    assert values(keys(np.array([-np.nan], F))).view(np.uint32)[0] == 0x7FC00000


def test_hand_cases():
    # three collinear points at 0, 1 and 3
    x = np.array([0.0, 1.0, 3.0])
    d = np.abs(x[:, None] - x[None, :]).astype(F)
    core, ei, ej, w, nans = tree_reference(d, 1)
    assert (core == -INF).all() and (ei.tolist(), ej.tolist(), w.tolist(), nans) == ([0, 1], [1, 2], [1.0, 2.0], 0)
    core, ei, ej, w, _ = tree_reference(d, 2)
    assert core.tolist() == [1.0, 1.0, 2.0] and (ei.tolist(), ej.tolist(), w.tolist()) == ([0, 1], [1, 2], [1.0, 2.0])
    core, ei, ej, w, _ = tree_reference(d, 3)                                  # every mr is 3: the order (i, j) decides
    assert core.tolist() == [3.0, 2.0, 3.0] and (ei.tolist(), ej.tolist(), w.tolist()) == ([0, 0], [1, 2], [3.0, 3.0])
    core, ei, ej, w, _ = tree_reference(d, 4)                                  # m - 1 > n - 1: every core distance is missing
    assert np.isnan(core).all() and len(ei) == 0
    labels, kind, counts = cut_reference(tree_reference(d, 2), 1.0)
    assert labels.tolist() == [0, 0, 2] and kind.tolist() == [CORE, CORE, 0] and counts.tolist() == [1, 2, 0, 1]
    # an all-equal matrix: every pair ties, the order (i, j) decides: the star around 0
    for link in (EITHER, BOTH):
        for min_pts in (1, 3, 9):
            core, ei, ej, w, _ = tree_reference(np.full((9, 9), 2.5, F), min_pts, link)
            assert ei.tolist() == [0] * 8 and ej.tolist() == list(range(1, 9)) and (w == 2.5).all()
    # two triangles and a point that sees one vertex of each
    d = border_tie_matrix()
    core, ei, ej, w, _ = tree_reference(d, 4)
    assert core.tolist() == [9.0, 9.0, 0.5, 9.0, 9.0, 9.0, 0.5]               # 2 and 6 have three neighbours at 0.5
    assert (ei.tolist(), ej.tolist(), w.tolist()) == ([0, 0, 0, 0, 0, 0], [1, 2, 3, 4, 5, 6], [9.0] * 6)
    labels, kind, counts = cut_reference((core, ei, ej, w), 0.5)
    assert labels.tolist() == [0, 1, 2, 3, 4, 5, 6] and counts.tolist() == [2, 2, 0, 5]   # DBSCAN*: the border points are noise
    want = density_reference(d, 0.5, 4)
    assert (kind == CORE).tolist() == (want[1] == CORE).tolist() and labels[[2, 6]].tolist() == want[0][[2, 6]].tolist()


@pytest.mark.parametrize("link", (EITHER, BOTH))
@pytest.mark.parametrize("n", SIZES)
def test_a_cut_is_density_clustering_on_the_core_points(n, link):
    """The pinned property, restatement against restatement."""
    cases = 0
    for kind in KINDS:
        for min_pts in sorted({1, 2, 4, n, n + 1}):
            d, tree = tree_case(kind, n, link, min_pts)
            assert len(tree[1]) <= max(n - 1, 0) and (tree[1] < tree[2]).all() and not np.isnan(tree[3]).any()
            assert (np.diff(keys(tree[3]).astype(np.int64)) >= 0).all()
            for eps in eps_of(tree):
                labels, kind_cut, counts = cut_reference(tree, eps)
                want_labels, want_kind, _, want_counts, want_nans = density_reference(d, eps, min_pts, link)
                core = want_kind == CORE
                what = "%s n %d link %d min_pts %d eps %r" % (kind, n, link, min_pts, eps)
                assert np.array_equal(kind_cut == CORE, core), what
                assert np.array_equal(labels[core], want_labels[core]) and np.array_equal(labels[~core], np.flatnonzero(~core)), what
                assert counts[0] == want_counts[0] and counts[1] == want_counts[1] and tree[4] == want_nans, what
                cases += 1
    assert cases >= 3 * 3 * 2


def test_weights_equal_scipys_minimum_spanning_tree():
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    d32 = blob_matrix(200, 1)
    d32 = np.minimum(d32, d32.T)
    for min_pts in (1, 5):
        core, ei, ej, w, _ = tree_reference(d32, min_pts)
        d = d32.astype(np.float64)
        c = core.astype(np.float64)
        mr = np.maximum(d, np.maximum(c[:, None], c[None, :])) if min_pts > 1 else d
        np.fill_diagonal(mr, 0.0)                                             # (no edge)
        mst = csgraph.minimum_spanning_tree(mr)
        assert len(w) == 199 and mst.nnz == 199
        assert np.array_equal(np.sort(mst.data), np.sort(w.astype(np.float64)))


def library_cut(tree, eps):
    from audio_pattern_discovery_amd.clustering import density_cut
    return density_cut(tree, eps, details=True)


@pytest.mark.parametrize("link", (EITHER, BOTH))
@pytest.mark.parametrize("n", SIZES)
def test_library_cut_and_operations_equal_the_restatement(apd, n, link):
    from audio_pattern_discovery_amd.clustering import AgglomerativeClustering, ClusteringOperation, Merge, density_operations
    for kind in KINDS:
        for min_pts in sorted({1, 2, 4, n, n + 1}):
            d, tree = tree_case(kind, n, link, min_pts)
            eps = np.array(eps_of(tree), F)
            labels, counts, kinds = library_cut(tree, eps)
            assert labels.dtype == np.uint32 and kinds.dtype == np.uint8 and counts.dtype == np.uint32
            for s, e in enumerate(eps):
                want = cut_reference(tree, e)
                what = "%s n %d link %d min_pts %d eps %r" % (kind, n, link, min_pts, e)
                assert np.array_equal(labels[s], want[0]) and np.array_equal(kinds[s], want[1]) and np.array_equal(counts[s], want[2]), what
            one = library_cut(tree, float(eps[len(eps) // 2]))                 # a scalar eps
            assert np.array_equal(one[0], labels[len(eps) // 2]) and np.array_equal(one[1], counts[len(eps) // 2])
            ops = density_operations(tree)
            want_ops = operations_reference(tree)
            assert [(o.merge_i, o.merge_j, o.into, int(o.operation)) for o in ops] == [(p, q, k, m) for p, q, k, _, m in want_ops]
            assert np.array_equal(np.array([o.distance for o in ops], F).view(np.uint32), np.array([w for _, _, _, w, _ in want_ops], F).view(np.uint32))
            # the merge list is a dendrogram to the library's other readers
            if min_pts == 1:
                assigned = AgglomerativeClustering.assignment(ops, n)
                assert same_partition(assigned, labels[-1]), "apd_cut_labels against the cut at +INF"
                half = len(ops) // 2
                if half and tree[3][half - 1] < tree[3][half]:                # a prefix of the list is the cut at its last weight
                    assert same_partition(AgglomerativeClustering.assignment(ops[:half], n), library_cut(tree, float(tree[3][half - 1]))[0])
                roots = set(int(v) for v in assigned if v >= n)
                sets = AgglomerativeClustering.cluster_sets(ops, roots, n)
                assert sorted(map(sorted, sets)) == sorted(sorted(np.flatnonzero(assigned == r).tolist()) for r in roots)


def test_operations_draw_as_a_dendrogram(apd):
    from audio_pattern_discovery_amd.clustering import dendrograms, density_operations
    x = np.array([0.0, 1.0, 3.0, 3.5])
    tree = tree_reference(np.abs(x[:, None] - x[None, :]).astype(F), 1)
    ops = density_operations(tree)                                             # (2, 3) at 0.5, (0, 1) at 1, then the two clusters at 2
    assert [(o.merge_i, o.merge_j, o.into, o.distance, o.operation.name) for o in ops] == [
        (2, 3, 4, 0.5, "Sequence2Sequence"), (0, 1, 5, 1.0, "Sequence2Sequence"), (5, 4, 6, 2.0, "Cluster2Cluster")]
    assert dendrograms(ops, {6}, list("ABCD")) == {6: "[.6 [[.5 [A B ] ] [.4 [C D ] ] ] ]"}


def raw_cut(apd, n, core, ei, ej, w, n_edges, eps, n_eps, labels, kind, counts):
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    return apd.lib().apd_density_tree_cut(n, p(core), p(ei), p(ej), p(w), n_edges, p(eps), n_eps, p(labels), p(kind), p(counts))


def test_host_entry_points_refuse_what_is_not_a_forest(apd):
    d, tree = tree_case("blobs", 7, EITHER, 2)
    core, ei, ej, w = tree[:4]
    eps = np.array([0.5, INF], F)
    labels, kind, counts = np.full((2, 7), 0x5A5A5A5A, np.uint32), np.full((2, 7), 0x5A, np.uint8), np.full((2, 4), 0x5A5A5A5A, np.uint32)
    untouched = lambda: (labels == 0x5A5A5A5A).all() and (kind == 0x5A).all() and (counts == 0x5A5A5A5A).all()
    swapped, beyond, cycle_i, cycle_j = ei.copy(), ej.copy(), ei.copy(), ej.copy()
    swapped[2] = ej[2]
    beyond[1] = 7
    cycle_i[5], cycle_j[5] = ei[0], ej[0]                                      # an edge twice: a cycle
    nan_eps = np.array([0.5, NAN], F)
    calls = {"edge_i >= edge_j": (7, core, swapped, ej, w, 6, eps, 2, labels, kind, counts),
             "a vertex >= n": (7, core, ei, beyond, w, 6, eps, 2, labels, kind, counts),
             "a cycle": (7, core, cycle_i, cycle_j, w, 6, eps, 2, labels, kind, counts),
             "more than n - 1 edges": (6, core, ei, ej, w, 6, eps, 2, labels, kind, counts),
             "a NaN eps": (7, core, ei, ej, w, 6, nan_eps, 2, labels, kind, counts),
             "no core": (7, None, ei, ej, w, 6, eps, 2, labels, kind, counts), "no eps": (7, core, ei, ej, w, 6, None, 2, labels, kind, counts),
             "no labels": (7, core, ei, ej, w, 6, eps, 2, None, kind, counts), "no counts": (7, core, ei, ej, w, 6, eps, 2, labels, kind, None),
             "no edge_i": (7, core, None, ej, w, 6, eps, 2, labels, kind, counts), "no weight": (7, core, ei, ej, None, 6, eps, 2, labels, kind, counts)}
    for what, args in calls.items():
        assert raw_cut(apd, *args) == apd.APD_ERR_INVALID_ARG, what
        assert untouched(), what
    assert raw_cut(apd, 7, core, ei, ej, w, 6, eps, 0, labels, kind, counts) == apd.APD_OK and untouched()   # no eps: nothing to do
    assert raw_cut(apd, 7, core, ei, ej, w, 6, eps, 2, labels, None, counts) == apd.APD_OK                  # kind may be NULL
    assert (kind == 0x5A).all() and np.array_equal(labels[0], cut_reference(tree, 0.5)[0]) and counts[1].tolist() == [1, 7, 0, 0]
    assert raw_cut(apd, 0, None, None, None, None, 0, eps, 2, None, None, counts) == apd.APD_OK and not counts.any()   # no instances
    ops = (apd.ClusterOp * 8)()
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    f = apd.lib().apd_density_tree_operations
    for what, args in {"edge_i >= edge_j": (7, swapped, ej, w, 6), "a vertex >= n": (7, ei, beyond, w, 6), "a cycle": (7, cycle_i, cycle_j, w, 6),
                       "no weight": (7, ei, ej, None, 6), "no edge_j": (7, ei, None, w, 6)}.items():
        assert f(args[0], p(args[1]), p(args[2]), p(args[3]), args[4], ops) == apd.APD_ERR_INVALID_ARG, what
        assert all(o.into == 0 for o in ops), what
    assert f(7, p(ei), p(ej), p(w), 6, None) == apd.APD_ERR_INVALID_ARG
    assert f(7, p(ei), p(ej), p(w), 6, ops) == apd.APD_OK and [o.into for o in ops[:6]] == list(range(7, 13))
    from audio_pattern_discovery_amd.clustering import density_cut
    with pytest.raises(apd.ApdError) as e:
        density_cut(tree, [0.5, NAN])
    assert e.value.status == apd.APD_ERR_INVALID_ARG
    assert math.isnan(NAN)
