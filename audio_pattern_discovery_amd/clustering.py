"""Host mirror of src/clustering.rs over the C ABI of include/apd.h."""
import ctypes as C
import enum
from dataclasses import dataclass

import numpy as np

from . import _lib


class Merge(enum.IntEnum):
    """clustering.rs:8-13"""
    Sequence2Sequence = 0
    Sequence2Cluster = 1
    Cluster2Sequence = 2
    Cluster2Cluster = 3


@dataclass
class ClusteringOperation:
    """clustering.rs:19-25 (`distance` is private in the reference; kept readable here for tests)."""
    merge_i: int
    merge_j: int
    into: int
    distance: float
    operation: Merge


class AgglomerativeClustering:
    """clustering.rs:27-210: the two associated functions the pipeline calls (main.rs:196-203)."""

    @staticmethod
    def clustering(distances, n_instances, perc, ctx=None, return_threshold=False):
        """clustering.rs:81-110 -> (Vec<ClusteringOperation>, set of root ids)."""
        ctx = ctx or _lib.default_context()
        d = np.ascontiguousarray(distances, dtype=np.float32).ravel()
        if d.size != n_instances * n_instances:
            raise ValueError("distances must hold n_instances^2 values")
        ops = (_lib.ClusterOp * max(n_instances, 1))()
        roots = np.zeros(max(n_instances, 1), dtype=np.uint32)
        n_ops, n_roots, thr = C.c_uint32(0), C.c_uint32(0), C.c_float(0)
        _lib.check(_lib.lib().apd_clustering(ctx.handle, C.c_void_p(d.ctypes.data), 0, n_instances, float(perc), ops,
                                             C.byref(n_ops), roots.ctypes.data_as(C.POINTER(C.c_uint32)),
                                             C.byref(n_roots), C.byref(thr)), ctx.handle)
        out = [ClusteringOperation(o.merge_i, o.merge_j, o.into, o.distance, Merge(o.operation))
               for o in ops[:n_ops.value]]
        ids = set(int(r) for r in roots[:n_roots.value])
        return (out, ids, float(thr.value)) if return_threshold else (out, ids)

    @staticmethod
    def cluster_sets(operations, cluster_ids, n_instances):
        """clustering.rs:40-76.  Roots are visited in ascending order (the reference iterates a HashSet)."""
        ops = (_lib.ClusterOp * max(len(operations), 1))()
        for t, o in enumerate(operations):
            ops[t] = _lib.ClusterOp(o.merge_i, o.merge_j, o.into, o.distance, int(o.operation))
        roots = np.array(sorted(cluster_ids), dtype=np.uint32)
        members = np.zeros(n_instances + len(operations) + 2, dtype=np.uint32)
        set_off = np.zeros(len(roots) + 2, dtype=np.uint32)
        n_sets = C.c_uint32(0)
        _lib.check(_lib.lib().apd_cluster_sets(ops, len(operations), roots.ctypes.data_as(C.POINTER(C.c_uint32)),
                                               len(roots), n_instances, members.ctypes.data_as(C.POINTER(C.c_uint32)),
                                               set_off.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(n_sets)))
        return [members[set_off[s]:set_off[s + 1]].tolist() for s in range(n_sets.value)]

    @staticmethod
    def cut(operations, threshold):
        """apd_dendrogram_cut: the prefix of `operations` a run at `threshold` performs -- the loop condition of clustering.rs:104-108
        replayed, so the operation that reaches the threshold is kept; a NaN threshold or one <= 0 keeps nothing."""
        n_kept = C.c_uint32(0)
        _lib.check(_lib.lib().apd_dendrogram_cut(_c_ops(operations), len(operations), float(threshold), C.byref(n_kept)))
        return list(operations[:n_kept.value])

    @staticmethod
    def assignment(operations, n_instances):
        """clustering.rs:115-128 after the merges of `operations` (apd_cut_labels): uint32[n], every instance's root -- its own
        number for an instance never merged.  A list that is not a dendrogram over n_instances raises ApdError(APD_ERR_INVALID_ARG)."""
        labels = np.zeros(n_instances, dtype=np.uint32)
        keep = np.zeros(max(n_instances, 1), dtype=np.uint32)                  # (a pointer that is never NULL)
        _lib.check(_lib.lib().apd_cut_labels(_c_ops(operations), len(operations), n_instances, keep.ctypes.data_as(C.POINTER(C.c_uint32))))
        labels[:] = keep[:n_instances]
        return labels

    @staticmethod
    def sweep(distances, n_instances, percs, axis=0, ctx=None, return_operations=False):
        """One UPGMA run, every percentile of `percs` as a cut of its dendrogram, the silhouette of all cuts in one apd_silhouette:
        the matrix is uploaded once, apd_clustering runs at max(percs), each threshold is apd_percentile on the resident matrix.
        Returns per percentile, in the order given, (perc, threshold, n_ops, n_clusters, score, nans); the first n_ops operations
        of the run are what clustering() returns at that percentile.  With return_operations: (rows, the run's operations)."""
        ctx = ctx or _lib.default_context()
        d = np.ascontiguousarray(distances, dtype=np.float32).ravel()
        n = int(n_instances)
        if d.size != n * n:
            raise ValueError("distances must hold n_instances^2 values")
        percs = [float(p) for p in percs]
        if not percs:
            return ([], []) if return_operations else []
        L = _lib.lib()
        buf = ctx.upload(d) if d.size else ctx.alloc(16)
        try:
            ops = (_lib.ClusterOp * max(n, 1))()
            roots = np.zeros(max(n, 1), dtype=np.uint32)
            n_ops, n_roots, thr = C.c_uint32(0), C.c_uint32(0), C.c_float(0)
            _lib.check(L.apd_clustering(ctx.handle, buf.at(), 1, n, max(percs), ops, C.byref(n_ops), roots.ctypes.data_as(C.POINTER(C.c_uint32)),
                                        C.byref(n_roots), C.byref(thr)), ctx.handle)
            operations = [ClusteringOperation(o.merge_i, o.merge_j, o.into, o.distance, Merge(o.operation)) for o in ops[:n_ops.value]]
            thresholds, kept = [], []
            labels = np.zeros((len(percs), n), dtype=np.uint32)
            for c, p in enumerate(percs):
                v = C.c_float(0)
                _lib.check(L.apd_percentile(ctx.handle, buf.at(), d.size, p, 1, C.byref(v)), ctx.handle)
                thresholds.append(float(v.value))
                kept.append(len(AgglomerativeClustering.cut(operations, v.value)))
                labels[c] = AgglomerativeClustering.assignment(operations[:kept[c]], n)
            score, clusters, nans = silhouette((buf.at(), n), labels, axis=axis, ctx=ctx, on_device=True)
        finally:
            buf.free()
        rows = [(percs[c], thresholds[c], kept[c], int(clusters[c]), float(score[c]), int(nans[c])) for c in range(len(percs))]
        return (rows, operations) if return_operations else rows


def _c_ops(operations):
    ops = (_lib.ClusterOp * max(len(operations), 1))()
    for t, o in enumerate(operations):
        ops[t] = _lib.ClusterOp(o.merge_i, o.merge_j, o.into, o.distance, int(o.operation))
    return ops


def silhouette(distances, labels, axis=0, samples=False, ctx=None, on_device=False):
    """apd_silhouette: the silhouette of cluster assignments over the [n][n] matrix of AlignmentWorkers.align_all.  labels: [n], or
    [L][n] for L assignments scored in one pass over the matrix; arbitrary uint32 values.  axis=0: dist(i, y) = distances[i][y],
    axis=1: distances[y][i] (the matrix is directed).  Per assignment a(i) is the mean distance to the other members of i's cluster
    (ascending f32 chain, the diagonal skipped), b(i) the smallest such mean over the other clusters (the smaller label among equals,
    NaN never), s(i) = (b - a) / max(a, b), 0 for a singleton, NaN where the arithmetic gives one; score is the sequential mean of
    the non-NaN s(i).  With on_device the matrix is (device pointer, n) and stays in HBM, as do the results until they are read here.
    Returns (score float32, clusters uint32, nans uint32) -- scalars for an [n] labels, [L] arrays otherwise -- and with samples also
    (s, a, b, nearest): float32 / uint32 [n] or [L][n]; nearest[i] is the label b(i) came from, 0xFFFFFFFF if none."""
    ctx = ctx or _lib.default_context()
    lab = np.ascontiguousarray(labels, dtype=np.uint32)
    single = lab.ndim == 1
    lab = lab.reshape(1, -1) if single else lab
    if lab.ndim != 2:
        raise ValueError("labels must be [n] or [L][n]")
    if on_device:
        ptr, n = distances
        ptr = ptr if isinstance(ptr, C.c_void_p) else C.c_void_p(int(ptr))
    else:
        d = np.ascontiguousarray(distances, dtype=np.float32)
        n = int(round(d.size ** 0.5))
        if d.size != n * n:
            raise ValueError("distances must hold n^2 values")
        ptr = C.c_void_p(d.ctypes.data)
    if lab.shape[1] != n:
        raise ValueError("labels must hold n values per assignment")
    cuts = lab.shape[0]
    per_cut = [np.zeros(cuts, np.float32), np.zeros(cuts, np.uint32), np.zeros(cuts, np.uint32)]
    per_sample = [np.zeros((cuts, n), t) for t in (np.float32, np.float32, np.float32, np.uint32)] if samples else []
    outs = per_cut + per_sample
    head = (ctx.handle, ptr, int(bool(on_device)), n, int(axis), lab.ctypes.data_as(C.POINTER(C.c_uint32)), cuts)
    none = [None] * (4 - len(per_sample))
    if not on_device:
        _lib.check(_lib.lib().apd_silhouette(*head, *[C.c_void_p(o.ctypes.data) for o in outs], *none), ctx.handle)
    else:
        bufs = [ctx.alloc(max(o.nbytes, 16)) for o in outs]
        try:
            _lib.check(_lib.lib().apd_silhouette(*head, *[b.at() for b in bufs], *none), ctx.handle)
            for o, b in zip(outs, bufs):
                if o.size:
                    o[...] = b.to_numpy(o.dtype, o.size).reshape(o.shape)     # the copy waits for the context's stream
        finally:
            for b in bufs:
                b.free()
    if single:
        outs = [o[0] for o in outs]
    return (tuple(outs[:3]), tuple(outs[3:])) if samples else tuple(outs)


def density(distances, eps, min_pts, link="either", ctx=None, on_device=False, details=False):
    """apd_density_clusters: DBSCAN over the [n][n] matrix of AlignmentWorkers.align_all.  near(i, j) is distances[i][j] <= eps (a NaN
    is never near); the matrix is directed, so link="either" joins i and j when one direction is near, "both" when both are.  A point
    with at least min_pts - 1 such neighbours is a core point (it counts itself, scikit-learn's convention: the k-th distance of
    neighbors(..., k, skip_self=True) as eps with min_pts = k + 1 makes the point core); clusters are the connected components of the
    core points, labelled by their smallest member; a non-core neighbour of core points is a border point and takes the smallest
    label among them; everything else is noise and keeps its own number, so the labels go straight into silhouette().
    eps, min_pts: scalars, or sequences of S settings (a scalar beside a sequence is repeated) answered from one pass over the matrix.
    With on_device the matrix is (device pointer, n) and stays in HBM.  Returns (labels uint32, counts uint32): [n] and [4] for
    scalars, [S][n] and [S][4] otherwise; counts = clusters, core, border, noise points.  With details also (kind uint8, degree
    uint32, nans int): kind 0 noise, 1 border, 2 core; nans the NaN entries off the diagonal."""
    ctx = ctx or _lib.default_context()
    single = np.ndim(eps) == 0 and np.ndim(min_pts) == 0
    e = np.atleast_1d(np.asarray(eps, dtype=np.float32)).ravel()
    m = np.atleast_1d(np.asarray(min_pts, dtype=np.int64)).ravel()
    if len(e) != len(m):
        if 1 not in (len(e), len(m)):
            raise ValueError("eps and min_pts must hold the same number of settings")
        e, m = np.repeat(e, len(m)) if len(e) == 1 else e, np.repeat(m, len(e)) if len(m) == 1 else m
    if len(e) == 0 or (m < 0).any() or (m > 0xFFFFFFFF).any():
        raise ValueError("at least one setting, and min_pts within 32 bits")
    e, m = np.ascontiguousarray(e), np.ascontiguousarray(m.astype(np.uint32))
    link = {"either": _lib.APD_DENSITY_EITHER, "both": _lib.APD_DENSITY_BOTH}.get(link, link)
    if on_device:
        ptr, n = distances
        ptr = ptr if isinstance(ptr, C.c_void_p) else C.c_void_p(int(ptr))
    else:
        d = np.ascontiguousarray(distances, dtype=np.float32)
        n = int(round(d.size ** 0.5))
        if d.size != n * n:
            raise ValueError("distances must hold n^2 values")
        ptr = C.c_void_p(d.ctypes.data)
    S = len(e)
    labels, counts = np.zeros((S, n), np.uint32), np.zeros((S, 4), np.uint32)
    kind, degree, nans = np.zeros((S, n), np.uint8), np.zeros((S, n), np.uint32), np.zeros(1, np.uint64)
    L, f32p, u32p = _lib.lib(), C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    for s0 in range(0, S, _lib.APD_DENSITY_MAX_SETTINGS):                     # a call with S settings equals S calls with one
        s1 = min(s0 + _lib.APD_DENSITY_MAX_SETTINGS, S)
        head = (ctx.handle, ptr, int(bool(on_device)), n, int(link), e[s0:s1].ctypes.data_as(f32p), m[s0:s1].ctypes.data_as(u32p), s1 - s0)
        outs = [labels[s0:s1], kind[s0:s1] if details else None, degree[s0:s1] if details else None, counts[s0:s1], nans if details else None]
        if not on_device:
            _lib.check(L.apd_density_clusters(*head, *[None if o is None else C.c_void_p(o.ctypes.data) for o in outs]), ctx.handle)
            continue
        bufs = [None if o is None else ctx.alloc(max(o.nbytes, 16)) for o in outs]
        try:
            _lib.check(L.apd_density_clusters(*head, *[None if b is None else b.at() for b in bufs]), ctx.handle)
            for o, b in zip(outs, bufs):
                if o is not None and o.size:
                    o[...] = b.to_numpy(o.dtype, o.size).reshape(o.shape)
        finally:
            for b in bufs:
                if b is not None:
                    b.free()
    if single:
        labels, counts, kind, degree = labels[0], counts[0], kind[0], degree[0]
    return ((labels, counts), (kind, degree, int(nans[0]))) if details else (labels, counts)


def density_sets(labels, kind):
    """The clusters of one density() assignment in apd_cluster_sets' layout, for medoids, barycenters and cross_linkage: (members,
    set_off) with set k = members[set_off[k]:set_off[k + 1]].  Host only.  Noise is left out; the sets ascend by label and the
    members inside a set ascend."""
    lab, kd = np.asarray(labels, dtype=np.uint32).ravel(), np.asarray(kind, dtype=np.uint8).ravel()
    if lab.shape != kd.shape:
        raise ValueError("labels and kind must hold one value per instance")
    kept = np.flatnonzero(kd != _lib.APD_DENSITY_NOISE)
    order = kept[np.argsort(lab[kept], kind="stable")]                        # by (label, index)
    sizes = np.unique(lab[kept], return_counts=True)[1]
    set_off = np.zeros(len(sizes) + 1, np.uint32)
    set_off[1:] = np.cumsum(sizes)
    return order.astype(np.uint32), set_off


def density_tree(distances, min_pts, link="either", ctx=None, on_device=False):
    """apd_density_tree: the density hierarchy of the [n][n] matrix of AlignmentWorkers.align_all at one min_pts -- every eps of
    density() at once.  Values are ordered with NaN as missing and last, -0.0 equal to +0.0; sym(i, j) is the smaller ("either") or
    larger ("both") of distances[i][j] and distances[j][i]; core[i] the (min_pts - 1)-th smallest sym(i, j) over j != i (-INF for
    min_pts = 1, NaN when there are not that many or the entry is missing), so core[i] <= eps exactly when density(eps, min_pts) calls
    i core; the tree is the minimum spanning forest of the mutual reachability max(core[i], core[j], sym(i, j)), its edges ordered
    by (weight, i, j).  With min_pts = 1 it is the single-linkage dendrogram.  With on_device the matrix is (device pointer, n) and
    stays in HBM.  Returns (core float32 [n], edge_i uint32, edge_j uint32, weight float32, nans int): the edge arrays trimmed to
    the edges found (at most n - 1), edge_i < edge_j, ascending; nans the NaN entries off the diagonal."""
    ctx = ctx or _lib.default_context()
    link = {"either": _lib.APD_DENSITY_EITHER, "both": _lib.APD_DENSITY_BOTH}.get(link, link)
    m = int(min_pts)
    if not 0 <= m <= 0xFFFFFFFF:
        raise ValueError("min_pts within 32 bits")
    if on_device:
        ptr, n = distances
        ptr = ptr if isinstance(ptr, C.c_void_p) else C.c_void_p(int(ptr))
    else:
        d = np.ascontiguousarray(distances, dtype=np.float32)
        n = int(round(d.size ** 0.5))
        if d.size != n * n:
            raise ValueError("distances must hold n^2 values")
        ptr = C.c_void_p(d.ctypes.data)
    slots = max(n - 1, 0)
    outs = [np.zeros(n, np.float32), np.zeros(slots, np.uint32), np.zeros(slots, np.uint32), np.zeros(slots, np.float32)]
    n_edges, nans = C.c_uint32(0), C.c_uint64(0)
    head = (ctx.handle, ptr, int(bool(on_device)), n, int(link), m)
    if not on_device:
        keep = [o if o.size else np.zeros(1, o.dtype) for o in outs]              # (pointers that are never NULL)
        _lib.check(_lib.lib().apd_density_tree(*head, *[C.c_void_p(o.ctypes.data) for o in keep], C.byref(n_edges), C.byref(nans)), ctx.handle)
    else:
        bufs = [ctx.alloc(max(o.nbytes, 16)) for o in outs]
        try:
            _lib.check(_lib.lib().apd_density_tree(*head, *[b.at() for b in bufs], C.byref(n_edges), C.byref(nans)), ctx.handle)
            for o, b in zip(outs, bufs):
                if o.size:
                    o[...] = b.to_numpy(o.dtype, o.size)
        finally:
            for b in bufs:
                b.free()
    core, edge_i, edge_j, weight = outs
    e = n_edges.value
    return core, edge_i[:e].copy(), edge_j[:e].copy(), weight[:e].copy(), int(nans.value)


_NOTHING = np.zeros(2, np.uint64)


def _ptr(array):
    """The array's address; an empty array gives a pointer that is not NULL and is never read."""
    return C.c_void_p(array.ctypes.data if array.size else _NOTHING.ctypes.data)


def _tree_arrays(tree):
    core, edge_i, edge_j, weight = (np.ascontiguousarray(a, dtype=t).ravel()
                                    for a, t in zip(tree[:4], (np.float32, np.uint32, np.uint32, np.float32)))
    if not len(edge_i) == len(edge_j) == len(weight):
        raise ValueError("edge_i, edge_j and weight must hold one value per edge")
    return core, edge_i, edge_j, weight


def density_cut(tree, eps, details=False):
    """apd_density_tree_cut: density clustering at eps read off a density_tree() result, on the host.  Edges with weight <= eps are
    joined; a point with core <= eps is core and takes the smallest number of its component, every other point is noise and keeps its
    own number (DBSCAN*: no border points).  On the core points the labels are density()'s at the same eps, min_pts and link.  eps: a
    scalar or a sequence of any length; NaN is refused.  Returns (labels uint32, counts uint32): [n] and [4] for a scalar, [S][n] and
    [S][4] otherwise; counts = clusters, core, 0, noise points.  With details also kind (uint8: 0 noise, 2 core)."""
    core, edge_i, edge_j, weight = _tree_arrays(tree)
    single = np.ndim(eps) == 0
    e = np.ascontiguousarray(np.atleast_1d(np.asarray(eps, dtype=np.float32)).ravel())
    n, S = len(core), len(e)
    labels, kind, counts = np.zeros((S, n), np.uint32), np.zeros((S, n), np.uint8), np.zeros((S, 4), np.uint32)
    _lib.check(_lib.lib().apd_density_tree_cut(n, _ptr(core), _ptr(edge_i), _ptr(edge_j), _ptr(weight), len(edge_i), _ptr(e), S, _ptr(labels),
                                               _ptr(kind), _ptr(counts)))
    if single:
        labels, kind, counts = labels[0], kind[0], counts[0]
    return (labels, counts, kind) if details else (labels, counts)


def density_operations(tree):
    """apd_density_tree_operations: the edges of a density_tree() result as a merge list in ClusteringOperation form -- edge t merges
    the current roots of its endpoints into n + t at distance weight[t] -- for AgglomerativeClustering.assignment / cluster_sets and
    dendrograms().  With min_pts = 1 this is the single-linkage dendrogram."""
    core, edge_i, edge_j, weight = _tree_arrays(tree)
    ops = (_lib.ClusterOp * max(len(edge_i), 1))()
    _lib.check(_lib.lib().apd_density_tree_operations(len(core), _ptr(edge_i), _ptr(edge_j), _ptr(weight), len(edge_i), ops))
    return [ClusteringOperation(o.merge_i, o.merge_j, o.into, o.distance, Merge(o.operation)) for o in ops[:len(edge_i)]]


def density_sweep(distances, min_pts, eps=None, link="either", axis=0, ctx=None):
    """One density_tree(), every eps as a cut of it, the silhouette of all cuts in one apd_silhouette: the matrix is uploaded once and
    read by the tree's rounds and by the silhouette only.  eps: the values to try; None: the distinct edge weights, thinned to at
    most 64 evenly by rank.  Returns per eps, in the order given, (eps, clusters, core, noise, score, nans): the counts of
    density_cut and the silhouette of its labels, noise as singletons.  AgglomerativeClustering.sweep's counterpart."""
    ctx = ctx or _lib.default_context()
    d = np.ascontiguousarray(distances, dtype=np.float32)
    n = int(round(d.size ** 0.5))
    if d.size != n * n:
        raise ValueError("distances must hold n^2 values")
    buf = ctx.upload(d.ravel()) if d.size else ctx.alloc(16)
    try:
        tree = density_tree((buf.at(), n), min_pts, link=link, ctx=ctx, on_device=True)
        if eps is None:
            eps = np.unique(tree[3])
            if len(eps) > 64:
                eps = eps[np.round(np.linspace(0, len(eps) - 1, 64)).astype(np.int64)]
        eps = np.atleast_1d(np.asarray(eps, dtype=np.float32)).ravel()
        if len(eps) == 0:
            return []
        labels, counts = density_cut(tree, eps)
        score, _, nans = silhouette((buf.at(), n), labels, axis=axis, ctx=ctx, on_device=True)
    finally:
        buf.free()
    return [(float(eps[c]), int(counts[c][0]), int(counts[c][1]), int(counts[c][3]), float(score[c]), int(nans[c])) for c in range(len(eps))]


def cross_linkage(fs, sf, sets, ctx=None):
    """apd_cross_linkage: the reference's average linkage (clustering.rs:153-170) between every first-set sequence q and every
    set of second-set sequence numbers in `sets` (as cluster_sets returns them; any order inside a set), from the cross matrices
    fs [n1][n2] and sf [n2][n1] of AlignmentWorkers.cross.  Returns (link_fs [n1][len(sets)], link_sf, nearest, nearest_linkage):
    nearest[q] is the set merge() would pick for q (0xFFFFFFFF if none has a linkage below +INF)."""
    ctx = ctx or _lib.default_context()
    fs = np.ascontiguousarray(fs, dtype=np.float32)
    sf = np.ascontiguousarray(sf, dtype=np.float32)
    if fs.ndim != 2 or sf.shape != fs.shape[::-1]:
        raise ValueError("fs must be [n1][n2] and sf [n2][n1]")
    n1, n2 = fs.shape
    members = np.array([m for s in sets for m in s], dtype=np.uint32)
    set_off = np.zeros(len(sets) + 1, dtype=np.uint32)
    set_off[1:] = np.cumsum([len(s) for s in sets])
    link_fs, link_sf = np.zeros((n1, len(sets)), np.float32), np.zeros((n1, len(sets)), np.float32)
    nearest, nearest_linkage = np.zeros(n1, np.uint32), np.zeros(n1, np.float32)
    u32p, vp = C.POINTER(C.c_uint32), C.c_void_p
    _lib.check(_lib.lib().apd_cross_linkage(ctx.handle, vp(fs.ctypes.data), vp(sf.ctypes.data), 0, n1, n2, members.ctypes.data_as(u32p),
                                            set_off.ctypes.data_as(u32p), len(sets), vp(link_fs.ctypes.data), vp(link_sf.ctypes.data),
                                            vp(nearest.ctypes.data), vp(nearest_linkage.ctypes.data)), ctx.handle)
    return link_fs, link_sf, nearest, nearest_linkage


def medoids(distances, sets, ctx=None):
    """apd_cluster_medoids: per set of sequence numbers in `sets` (as cluster_sets returns them; any order inside a set) the member
    whose distances to and from the set's members -- summed ascending in f32, one rounded add per term -- are smallest, from the
    [n][n] matrix of AlignmentWorkers.align_all.  Returns (medoid, cost): uint32 sequence numbers (the smallest among equal costs;
    0xFFFFFFFF for an empty set or one whose costs are all +INF / NaN) and float32 costs (+INF there)."""
    ctx = ctx or _lib.default_context()
    d = np.ascontiguousarray(distances, dtype=np.float32)
    n = int(round(d.size ** 0.5))
    if d.size != n * n:
        raise ValueError("distances must hold n^2 values")
    members = np.array([m for s in sets for m in s], dtype=np.uint32)
    set_off = np.zeros(len(sets) + 1, dtype=np.uint32)
    set_off[1:] = np.cumsum([len(s) for s in sets])
    medoid, cost = np.zeros(len(sets), np.uint32), np.zeros(len(sets), np.float32)
    u32p, vp = C.POINTER(C.c_uint32), C.c_void_p
    _lib.check(_lib.lib().apd_cluster_medoids(ctx.handle, vp(d.ctypes.data), 0, n, members.ctypes.data_as(u32p),
                                              set_off.ctypes.data_as(u32p), len(sets), vp(medoid.ctypes.data), vp(cost.ctypes.data)),
               ctx.handle)
    return medoid, cost


def neighbors(distances, k, axis=0, skip_self=False, queries=None, ctx=None, on_device=False):
    """apd_neighbors: the k nearest entries of rows (axis=0: query q ranks distances[q][:]) or columns (axis=1: distances[:][q]) of
    a 2-D matrix -- the [n][n] one of AlignmentWorkers.align_all, or a cross matrix of cross() -- ascending by (value, index), NaN
    entries dropped, the query's own number too with skip_self.  queries: row / column numbers in any order, repeats allowed; None:
    all of them, ascending.  With on_device the matrix is (device pointer, rows, cols) and stays in HBM, as do the results until
    they are read here.  Returns (index uint32 [Q][k], distance float32 [Q][k], count uint32 [Q], nans uint32 [Q]): count[q]
    candidates were found (at most k), the slots behind them hold 0xFFFFFFFF and NaN; nans[q] NaN entries were met."""
    ctx = ctx or _lib.default_context()
    if on_device:
        ptr, rows, cols = distances
        ptr = ptr if isinstance(ptr, C.c_void_p) else C.c_void_p(int(ptr))
    else:
        d = np.ascontiguousarray(distances, dtype=np.float32)
        if d.ndim != 2:
            raise ValueError("distances must be a 2-D array")
        (rows, cols), ptr = d.shape, C.c_void_p(d.ctypes.data)
    q = None if queries is None else np.ascontiguousarray(queries, dtype=np.uint32).ravel()
    n_q = (rows, cols)[int(axis)] if q is None and axis in (0, 1) else (0 if q is None else len(q))
    k = int(k)
    shape = (n_q, max(k, 0))
    index, distance = np.zeros(shape, np.uint32), np.zeros(shape, np.float32)
    count, nans = np.zeros(n_q, np.uint32), np.zeros(n_q, np.uint32)
    q_ptr = None if q is None else q.ctypes.data_as(C.POINTER(C.c_uint32))
    head = (ctx.handle, ptr, int(bool(on_device)), int(rows), int(cols), int(axis), q_ptr, 0 if q is None else len(q), k, int(bool(skip_self)))
    outs = (index, distance, count, nans)
    if not on_device:
        _lib.check(_lib.lib().apd_neighbors(*head, *[C.c_void_p(a.ctypes.data) for a in outs]), ctx.handle)
        return outs
    bufs = [ctx.alloc(max(a.nbytes, 16)) for a in outs]
    try:
        _lib.check(_lib.lib().apd_neighbors(*head, *[b.at() for b in bufs]), ctx.handle)
        for a, b in zip(outs, bufs):
            if a.size:
                a[...] = b.to_numpy(a.dtype, a.size).reshape(a.shape)     # the copy waits for the context's stream
    finally:
        for b in bufs:
            b.free()
    return outs


def percentile(x, perc, ctx=None):
    """numerics.rs:125-133 on the GPU (apd_percentile)."""
    ctx = ctx or _lib.default_context()
    a = np.ascontiguousarray(x, dtype=np.float32).ravel()
    v = C.c_float(0)
    _lib.check(_lib.lib().apd_percentile(ctx.handle, C.c_void_p(a.ctypes.data), a.size, float(perc), 0, C.byref(v)),
               ctx.handle)
    return float(v.value)


def dendrograms(operations, clusters, labels):
    """The bracket strings reporting.rs:135-169 builds for TikZ-qtree (apd_dendrograms), one per root that was merged at
    least once: leaf i is rendered as labels[i] (the reference puts an \\includegraphics reference there, reporting.rs:211-221),
    node k as "[.k [<left> <right> ] ]".  Roots never merged are skipped, as the reference does (reporting.rs:200).
    Lets a run be diffed against the reference's output/ (SURVEY.md 8(f) item 4)."""
    ops = (_lib.ClusterOp * max(len(operations), 1))()
    for t, o in enumerate(operations):
        ops[t] = _lib.ClusterOp(o.merge_i, o.merge_j, o.into, o.distance, int(o.operation))
    roots = np.array(sorted(clusters), dtype=np.uint32)
    lab = (C.c_char_p * max(len(labels), 1))(*[str(v).encode() for v in labels])
    which = np.zeros(len(roots) + 1, dtype=np.uint32)
    n_bytes, n_strings = C.c_uint64(0), C.c_uint32(0)
    u32p = C.POINTER(C.c_uint32)
    L = _lib.lib()
    _lib.check(L.apd_dendrograms(ops, len(operations), roots.ctypes.data_as(u32p), len(roots), lab, len(labels), None, 0,
                                 C.byref(n_bytes), which.ctypes.data_as(u32p), C.byref(n_strings)))
    buf = C.create_string_buffer(n_bytes.value + 1)
    _lib.check(L.apd_dendrograms(ops, len(operations), roots.ctypes.data_as(u32p), len(roots), lab, len(labels), buf, n_bytes.value,
                                 C.byref(n_bytes), which.ctypes.data_as(u32p), C.byref(n_strings)))
    parts = buf.raw[:n_bytes.value].split(b"\0")[:n_strings.value]
    return {int(roots[which[i]]): parts[i].decode() for i in range(n_strings.value)}
