"""The contract of apd_density_tree, apd_density_tree_cut and apd_density_tree_operations (include/apd.h) restated in numpy: test
infrastructure, shares no code with the library.

    tree_reference(d, min_pts, link)        ->  core, edge_i, edge_j, weight, nans
    cut_reference(tree, eps)                ->  labels, kind, counts                  for ONE eps
    operations_reference(tree)              ->  [(merge_i, merge_j, into, distance, operation)]

Values are ordered through uint32 keys (NaN last, the zeros equal), the core distance is read off a sorted row, the tree is Kruskal's
over ALL pairs sorted by (key, i, j) with a union-find, and the cut is another union-find.  Also the matrices the tree tests share."""
import numpy as np

from _density_reference import BOTH, CORE, EITHER, F, NOISE, blob_matrix

U = np.uint32
MISSING = U(0xFFFFFFFF)
QUIET = 0x7FC00000


def keys(values):
    """Order keys of float32 values: ascending key == the contract's order."""
    v = np.ascontiguousarray(values, F)
    u = v.view(U).copy()
    u[v == 0] = 0                                                             # -0.0 is +0.0
    k = np.where(u & U(0x80000000), ~u, u | U(0x80000000)).astype(U)
    k[np.isnan(v)] = MISSING
    return k


def values(k):
    """The canonical float32 of keys: +0.0 for the zeros, the quiet NaN for missing."""
    k = np.ascontiguousarray(k, U)
    u = np.where(k & U(0x80000000), k & U(0x7FFFFFFF), ~k).astype(U)
    u[k == MISSING] = QUIET
    return u.view(F)


def sym_keys(d, link):
    k = keys(d)
    return np.minimum(k, k.T) if link == EITHER else np.maximum(k, k.T)


def core_keys(sym, min_pts):
    n = sym.shape[0]
    if min_pts == 1:
        return np.full(n, keys(np.array([-np.inf], F))[0], U)
    core = np.full(n, MISSING, U)
    if min_pts - 1 <= n - 1:
        for i in range(n):
            core[i] = np.sort(np.delete(sym[i], i))[min_pts - 2]
    return core


class _Sets:
    def __init__(self, n):
        self.up = list(range(n))

    def find(self, v):
        up = self.up
        while up[v] != v:
            up[v] = up[up[v]]
            v = up[v]
        return v

    def join(self, a, b):
        a, b = self.find(a), self.find(b)
        if a == b:
            return False
        self.up[max(a, b)] = min(a, b)
        return True


def tree_reference(d, min_pts, link=EITHER):
    d = np.ascontiguousarray(d, F)
    n = d.shape[0]
    assert d.shape == (n, n) and int(min_pts) >= 1 and link in (EITHER, BOTH)
    off = ~np.eye(n, dtype=bool)
    nans = int(np.isnan(d[off]).sum()) if n else 0
    sym = sym_keys(d, link)
    core = core_keys(sym, int(min_pts))
    mr = np.maximum(sym, np.maximum(core[:, None], core[None, :]))
    i, j = np.triu_indices(n, 1)
    w = mr[i, j]
    keep = w != MISSING
    i, j, w = i[keep], j[keep], w[keep]
    order = np.lexsort((j, i, w))                                             # by (key, i, j)
    sets, chosen = _Sets(n), []
    for t in order.tolist():
        if sets.join(int(i[t]), int(j[t])):
            chosen.append(t)
            if len(chosen) == n - 1:
                break
    chosen = np.array(chosen, np.int64)
    return values(core), i[chosen].astype(U), j[chosen].astype(U), values(w[chosen]), nans


def cut_reference(tree, eps):
    core, edge_i, edge_j, weight = tree[:4]
    n, eps = len(core), F(eps)
    assert not np.isnan(eps)
    sets = _Sets(n)
    with np.errstate(invalid="ignore"):
        for t in np.flatnonzero(weight <= eps).tolist():
            sets.join(int(edge_i[t]), int(edge_j[t]))
        is_core = core <= eps
    labels = np.array([sets.find(v) if is_core[v] else v for v in range(n)], U)
    kind = np.where(is_core, CORE, NOISE).astype(np.uint8)
    clusters = len(np.unique(labels[is_core]))
    return labels, kind, np.array([clusters, is_core.sum(), 0, n - is_core.sum()], U)


def operations_reference(tree):
    core, edge_i, edge_j, weight = tree[:4]
    n = len(core)
    sets, name, ops = _Sets(n), list(range(n)), []                            # name[root]: the cluster the root stands for
    for t in range(len(edge_i)):
        p, q = name[sets.find(int(edge_i[t]))], name[sets.find(int(edge_j[t]))]
        sets.join(int(edge_i[t]), int(edge_j[t]))
        name[sets.find(int(edge_i[t]))] = n + t
        kind = 0 if (p < n and q < n) else 3 if (p >= n and q >= n) else 2 if p >= n else 1   # clustering.rs:193-201
        ops.append((p, q, n + t, weight[t], kind))
    return ops


def same_partition(a, b):
    """Two label arrays name the same sets."""
    a, b = np.asarray(a), np.asarray(b)
    return len(a) == len(b) and len({(int(x), int(y)) for x, y in zip(a, b)}) == len(set(a.tolist())) == len(set(b.tolist()))


def rounded_matrix(n, seed):
    """blob_matrix with its distances rounded to integers: heavy ties, asymmetric."""
    d = np.rint(blob_matrix(n, seed, asymmetric=True) * 2).astype(F)
    np.fill_diagonal(d, 0.0)
    return d


def special_matrix(n, seed):
    """An asymmetric matrix with NaN rows, NaN blocks that split it into a forest, NaN entries on one side only, -0.0 against +0.0, a
    negative entry and +-INF; the diagonal holds a NaN and an INF that enter nothing."""
    d = (np.rint(blob_matrix(n, seed, asymmetric=True) * 4) / 4).astype(F)
    if n >= 2:
        rng = np.random.default_rng(seed + 7)
        half = n // 2
        d[:half, half:] = np.nan                                              # two blocks with nothing between them ...
        d[half:, :half] = np.nan
        if n >= 7:
            d[half - 1, half], d[2, n - 1] = 1.5, np.nan                      # ... but one entry (one direction only) and a lone NaN
            lone = int(rng.integers(0, n))
            d[lone, :] = np.nan                                               # a NaN row: its column still links it under EITHER
            d[3, 4], d[4, 3], d[0, 1], d[1, 0] = -0.0, 0.0, -1.0, -0.0
            d[5, 6], d[6, 5], d[0, 2], d[2, 0] = np.inf, np.inf, -np.inf, np.inf
        d[0, 0], d[n - 1, n - 1] = np.nan, np.inf
    return d
