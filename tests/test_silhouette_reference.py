"""CPU side of the silhouette: the numpy restatement of apd_silhouette's contract (tests/_silhouette_reference.py) against hand
cases, its own fast form and float64, and the two host-only entry points apd_dendrogram_cut / apd_cut_labels through the library."""
import ctypes as C

import numpy as np
import pytest

from audio_pattern_discovery_amd import synth
from _silhouette_reference import (F, KINDS, NO_LABEL, assert_same, bits, matrix, silhouette_float64, silhouette_literal,
                                   silhouette_rows)

HAND = np.array([[0, 1, 4, 6], [2, 0, 5, 7], [8, 3, 0, 1], [9, 9, 2, 0]], F)
HAND_LABELS = np.array([7, 7, 9, 9], np.uint32)


def f32_div(p, q):
    return F(F(p) / F(q))


@pytest.mark.parametrize("fn", (silhouette_literal, silhouette_rows))
def test_hand_case(fn):
    score, clusters, nans, s, a, b, nearest = fn(HAND, HAND_LABELS, 0)
    assert a.tolist() == [1, 2, 1, 2] and b.tolist() == [5, 6, 5.5, 9] and nearest.tolist() == [9, 9, 7, 7]
    want = [f32_div(4, 5), f32_div(4, 6), f32_div(4.5, 5.5), f32_div(7, 9)]
    assert np.array_equal(bits(s), bits(np.array(want, F)))
    assert clusters == 2 and nans == 0
    assert bits(np.array([score], F))[0] == bits(np.array([F(F(F(F(want[0] + want[1]) + want[2]) + want[3]) / F(4))], F))[0]
    _, _, _, s, a, b, _ = fn(HAND, HAND_LABELS, 1)
    assert a[0] == 2 and b[0] == 8.5 and s[0] == f32_div(6.5, 8.5)


@pytest.mark.parametrize("fn", (silhouette_literal, silhouette_rows))
def test_singletons_one_cluster_and_a_single_instance(fn):
    d = matrix(5, 1)
    score, clusters, nans, s, a, b, nearest = fn(d, np.arange(5), 0)          # all singletons: a = s = 0, b the nearest other entry
    assert clusters == 5 and nans == 0 and score == 0 and not a.any() and not s.any()
    for i in range(5):
        others = [d[i, y] for y in range(5) if y != i]
        assert b[i] == min(others) and nearest[i] == [y for y in range(5) if y != i][int(np.argmin(others))]
    score, clusters, nans, s, a, b, nearest = fn(d, np.full(5, 3), 0)         # one cluster: b = +INF, s = (INF - a) / INF = NaN
    assert clusters == 1 and nans == 5 and np.isnan(score) and np.isposinf(b).all() and (nearest == NO_LABEL).all() and np.isnan(s).all()
    assert bits(np.array([score], F))[0] == 0x7FC00000
    score, clusters, nans, s, a, b, nearest = fn(np.array([[np.nan]], F), np.array([4]), 0)   # n = 1: a singleton, nothing else
    assert (clusters, nans, score, s[0], a[0], nearest[0]) == (1, 0, 0, 0, 0, NO_LABEL) and np.isposinf(b[0])
    score, clusters, nans, s, *_ = fn(np.zeros((0, 0), F), np.zeros(0, np.uint32), 0)
    assert clusters == 0 and nans == 0 and np.isnan(score) and len(s) == 0


@pytest.mark.parametrize("fn", (silhouette_literal, silhouette_rows))
def test_special_values(fn):
    # a tie of two means goes to the smaller label, whichever comes first by index
    d = np.array([[0, 3, 3, 9], [1, 0, 1, 1], [1, 1, 0, 1], [1, 1, 1, 0]], F)
    for labels, want in (([5, 8, 2, 5], 2), ([5, 2, 8, 5], 2)):
        *_, b, nearest = fn(d, np.array(labels, np.uint32), 0)
        assert nearest[0] == want and b[0] == 3
    # a NaN diagonal is skipped, not added: instance 0's own chain is d[0][1] alone
    d = np.array([[np.nan, 2, 5], [4, np.nan, 7], [1, 1, np.nan]], F)
    _, _, nans, s, a, b, _ = fn(d, np.array([1, 1, 6], np.uint32), 0)
    assert nans == 0 and a.tolist() == [2, 4, 0] and b.tolist() == [5, 7, 1] and s[2] == 0
    # a NaN row: its a, b and s are NaN, it is counted and left out of the score; NaN means are never kept
    d = matrix(6, 3)
    d[2, :] = np.nan
    score, _, nans, s, a, b, nearest = fn(d, np.array([0, 0, 0, 1, 1, 1], np.uint32), 0)
    assert nans == 1 and np.isnan(s[2]) and np.isnan(a[2]) and np.isposinf(b[2]) and nearest[2] == NO_LABEL and not np.isnan(score)
    # +INF entries: a mean of +INF is not below +INF, so it is not kept
    d = np.array([[0, np.inf, np.inf], [1, 0, 2], [np.inf, 1, 0]], F)
    _, _, nans, s, a, b, nearest = fn(d, np.array([0, 1, 2], np.uint32), 0)
    assert np.isposinf(b[0]) and nearest[0] == NO_LABEL and b[2] == 1 and nearest[2] == 1
    d = np.array([[0, np.inf, 1], [1, 0, 2], [3, 1, 0]], F)
    _, _, nans, s, a, b, _ = fn(d, np.array([0, 0, 2], np.uint32), 0)
    assert np.isposinf(a[0]) and b[0] == 1 and np.isnan(s[0]) and nans == 1   # (1 - INF) / INF: not patched
    # negative entries whose mean rounds to -0.0: it ties with +0.0 (the smaller label keeps it), and b carries its sign
    t = F(-1e-45)
    d = np.array([[0, t, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]], F)
    *_, b, nearest = fn(d, np.array([9, 3, 3, 4, 4], np.uint32), 0)
    assert bits(b)[0] == 0x80000000 and nearest[0] == 3
    *_, b, nearest = fn(d, np.array([9, 4, 4, 3, 3], np.uint32), 0)
    assert bits(b)[0] == 0 and nearest[0] == 3


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("axis", (0, 1))
def test_the_fast_form_is_the_literal_one_bitwise(kind, axis):
    rng = np.random.default_rng(7)
    for n in (1, 2, 3, 17, 29):
        d = matrix(n, 100 + n, kind)
        for labels in (np.arange(n), np.zeros(n), rng.integers(0, 4, n), rng.integers(0, 2, n) * 0xFFFFFF00 + 3):
            labels = labels.astype(np.uint32)
            assert_same(silhouette_rows(d, labels, axis), silhouette_literal(d, labels, axis), "%s n %d axis %d" % (kind, n, axis))


@pytest.mark.parametrize("n", (40, 300))
def test_agreement_with_float64(n):
    """Nonnegative finite matrices: each mean carries at most n roundings of 2^-24 (relative), s = +-(1 - min / max) the two means'
    errors plus two more roundings, (2n + 3) 2^-24 < n 2^-22.  a/b ties are excluded by construction: the own cluster's entries are
    drawn from [0.05, 1), the others' from [2, 4)."""
    rng = np.random.default_rng(n)
    labels = rng.integers(0, 5, n).astype(np.uint32)
    inside = labels[:, None] == labels[None, :]
    d = np.where(inside, rng.uniform(0.05, 1.0, (n, n)), rng.uniform(2.0, 4.0, (n, n))).astype(F)
    for axis in (0, 1):
        s = silhouette_rows(d, labels, axis)[3]
        assert np.abs(s.astype(np.float64) - silhouette_float64(d, labels, axis)).max() <= n * 2.0 ** -22


# ---- the host-only entry points, through the library

def c_ops(apd, ops):
    arr = (apd.ClusterOp * max(len(ops), 1))()
    for t, (i, j, into, distance) in enumerate(ops):
        arr[t] = apd.ClusterOp(i, j, into, distance, 0)
    return arr


def oracle_runs(oracle):
    runs = []
    for n, seed, perc in ((12, 5, 0.4), (20, 6, 0.9), (9, 7, 1.0 - 1e-6)):
        frames, offsets = synth.make_sequences(n, 16, 4, seed=seed)
        d = oracle.align_all(frames, offsets, 1.0, workers=4)
        ops, _, _ = oracle.clustering(d, n, perc)
        runs.append((n, [(o["merge_i"], o["merge_j"], o["into"], o["distance"]) for o in ops]))
    return runs


def test_dendrogram_cut_replays_the_loop_condition(oracle, apd):
    """clustering.rs:104-108 on recorded operation lists: thresholds below the first distance, equal to a distance (the operation
    that reaches it is kept), between two, above all, zero, negative and NaN."""
    L = apd.lib()
    for n, ops in oracle_runs(oracle) + [(4, [(0, 1, 4, 0.5), (2, 3, 5, 0.5), (4, 5, 6, 2.0)]), (3, [])]:
        dist = [F(o[3]) for o in ops]
        thresholds = [0.0, -1.0, float("nan"), float("inf"), 1e-30]
        for k, v in enumerate(dist):
            thresholds += [float(v), float(np.nextafter(v, F(np.inf))), float(np.nextafter(v, F(-np.inf)))]
        for threshold in thresholds:
            kept, distance = 0, F(0.0)
            while kept < len(ops) and distance < F(threshold):
                distance = dist[kept]
                kept += 1
            got = C.c_uint32(77)
            assert L.apd_dendrogram_cut(c_ops(apd, ops), len(ops), float(F(threshold)), C.byref(got)) == apd.APD_OK
            assert got.value == kept, (n, threshold)
    assert L.apd_dendrogram_cut(c_ops(apd, []), 0, 1.0, None) == apd.APD_ERR_INVALID_ARG
    assert L.apd_dendrogram_cut(None, 2, 1.0, C.byref(C.c_uint32(0))) == apd.APD_ERR_INVALID_ARG


def test_cut_labels_replays_the_parent_pointers(oracle, apd):
    """assignment() (clustering.rs:115-128) over the parents merge_clusters (clustering.rs:134-141) leaves, for every prefix of
    oracle dendrograms; singletons keep their own number."""
    from audio_pattern_discovery_amd.clustering import AgglomerativeClustering, ClusteringOperation, Merge
    L = apd.lib()
    for n, ops in oracle_runs(oracle):
        assert ops
        for kept in range(len(ops) + 1):
            parents = list(range(n))
            for p, q, _, _ in ops[:kept]:
                k = len(parents)
                parents[p] = k
                parents[q] = k
                parents.append(k)

            def cluster(i):
                p = i
                while p != parents[p]:
                    p = parents[p]
                return p
            want = [cluster(i) for i in range(n)]
            labels = np.full(n, 0xDEAD, np.uint32)
            assert L.apd_cut_labels(c_ops(apd, ops), kept, n, labels.ctypes.data_as(C.POINTER(C.c_uint32))) == apd.APD_OK
            assert labels.tolist() == want
            mine = [ClusteringOperation(i, j, into, dist, Merge.Sequence2Sequence) for i, j, into, dist in ops[:kept]]
            assert AgglomerativeClustering.assignment(mine, n).tolist() == want
        assert want != list(range(n))
    assert AgglomerativeClustering.assignment([], 3).tolist() == [0, 1, 2]
    assert AgglomerativeClustering.assignment([], 0).tolist() == []


def test_cut_labels_rejects_every_malformed_operation(apd):
    L = apd.lib()
    good = [(0, 1, 5, 0.1), (2, 5, 6, 0.2), (3, 4, 7, 0.3), (6, 7, 8, 0.4)]
    bad = {
        "into is not n + t": [(0, 1, 6, 0.1)],
        "into of a later operation": good[:1] + [(2, 5, 7, 0.2)],
        "merge_i == merge_j": [(2, 2, 5, 0.1)],
        "merge_i merged before": good[:1] + [(0, 2, 6, 0.2)],
        "merge_j merged before": good[:1] + [(2, 1, 6, 0.2)],
        "merge_i is a node merged before": good[:2] + [(5, 3, 7, 0.3)],
        "merge_j is its own into": [(0, 5, 5, 0.1)],
        "merge_i is a node that does not exist yet": [(6, 0, 5, 0.1)],
        "merge_j beyond every id": [(0, 0xFFFFFFFF, 5, 0.1)],
        "the last operation": good[:3] + [(6, 6, 8, 0.4)],
    }
    labels = np.full(5, 0xDEAD, np.uint32)
    ptr = labels.ctypes.data_as(C.POINTER(C.c_uint32))
    assert L.apd_cut_labels(c_ops(apd, good), len(good), 5, ptr) == apd.APD_OK and labels.tolist() == [8] * 5
    for what, ops in bad.items():
        labels[:] = 0xDEAD
        assert L.apd_cut_labels(c_ops(apd, ops), len(ops), 5, ptr) == apd.APD_ERR_INVALID_ARG, what
        assert (labels == 0xDEAD).all(), what + ": labels were written"
    assert L.apd_cut_labels(None, 1, 5, ptr) == apd.APD_ERR_INVALID_ARG
    assert L.apd_cut_labels(c_ops(apd, good), 1, 5, None) == apd.APD_ERR_INVALID_ARG
    assert L.apd_cut_labels(c_ops(apd, good), 0, 0, None) == apd.APD_OK


def test_cut_is_the_prefix_clustering_returns(apd):
    from audio_pattern_discovery_amd.clustering import AgglomerativeClustering, ClusteringOperation, Merge
    ops = [ClusteringOperation(0, 1, 4, 0.5, Merge.Sequence2Sequence), ClusteringOperation(2, 3, 5, 1.5, Merge.Sequence2Sequence),
           ClusteringOperation(4, 5, 6, 2.5, Merge.Cluster2Cluster)]
    assert AgglomerativeClustering.cut(ops, 0.0) == [] and AgglomerativeClustering.cut(ops, float("nan")) == []
    assert AgglomerativeClustering.cut(ops, 0.25) == ops[:1] and AgglomerativeClustering.cut(ops, 0.5) == ops[:1]
    assert AgglomerativeClustering.cut(ops, 0.75) == ops[:2] and AgglomerativeClustering.cut(ops, 9.0) == ops
