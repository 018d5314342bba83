"""The contract of apd_silhouette (include/apd.h) restated in numpy float32: loops, one rounded add per term.

silhouette_literal is the contract word for word in f32 scalars.  silhouette_rows is the same arithmetic with every instance's chain
advanced at once (one float32 vector add per member: still one rounded add per term and instance), fast enough for the GPU tests;
tests/test_silhouette_reference.py holds the two bitwise equal.  Both take one assignment; axis 0: dist(i, y) = d[i][y], 1: d[y][i].

Results are (score, clusters, nans, s, a, b, nearest); compare with `same` / `assert_same`, which look at bits (`comparable`)."""
import numpy as np

F = np.float32
NO_LABEL = 0xFFFFFFFF
QUIET_NAN = np.array([0x7FC00000], np.uint32).view(np.float32)[0]


def _score(s):
    total, kept, nans = F(0.0), 0, 0
    with np.errstate(all="ignore"):
        for v in s:
            if v != v:
                nans += 1
            else:
                total = F(total + v)
                kept += 1
        return (F(total / F(kept)) if kept else QUIET_NAN), nans


def silhouette_literal(d, labels, axis=0):
    d = np.asarray(d, np.float32)
    labels = np.asarray(labels, np.uint32)
    n = len(labels)
    dist = d if axis == 0 else d.T
    present = sorted(set(int(v) for v in labels))
    s, a, b = np.zeros(n, F), np.zeros(n, F), np.zeros(n, F)
    nearest = np.zeros(n, np.uint32)
    with np.errstate(all="ignore"):
        for i in range(n):
            total, cnt = {}, {}
            for L in present:
                acc, terms = F(0.0), 0
                for y in range(n):
                    if int(labels[y]) == L and y != i:
                        acc = F(acc + dist[i, y])
                        terms += 1
                total[L], cnt[L] = acc, terms
            own = int(labels[i])
            single = cnt[own] == 0
            a[i] = F(0.0) if single else F(total[own] / F(cnt[own]))
            best, arg = F(np.inf), NO_LABEL
            for L in present:
                if L == own:
                    continue
                mean = F(total[L] / F(cnt[L]))
                if mean < best:
                    best, arg = mean, L
            b[i], nearest[i] = best, arg
            if single:
                s[i] = F(0.0)
            else:
                m = b[i] if a[i] < b[i] else a[i]
                s[i] = F(F(b[i] - a[i]) / m)
    score, nans = _score(s)
    return score, np.uint32(len(present)), np.uint32(nans), s, a, b, nearest


def cluster_means(d, labels, axis=0):
    """(present labels ascending, sum [K][n], cnt [K][n]): the chains of every instance against every label, diagonal skipped."""
    d = np.asarray(d, np.float32)
    labels = np.asarray(labels, np.uint32)
    n = len(labels)
    dist = d if axis == 0 else d.T
    present = np.unique(labels)
    me = np.arange(n)
    total = np.zeros((len(present), n), F)
    cnt = np.zeros((len(present), n), np.int64)
    with np.errstate(all="ignore"):
        for k, L in enumerate(present):
            for y in np.flatnonzero(labels == L):
                other = me != y
                total[k] = np.where(other, total[k] + dist[:, y], total[k])
                cnt[k] += other
    return present, total, cnt


def silhouette_rows(d, labels, axis=0):
    labels = np.asarray(labels, np.uint32)
    n = len(labels)
    present, total, cnt = cluster_means(d, labels, axis)
    rank = np.searchsorted(present, labels)
    me = np.arange(n)
    with np.errstate(all="ignore"):
        mean = total / cnt.astype(F) if n else total
        own_cnt = cnt[rank, me] if n else np.zeros(0, np.int64)
        single = own_cnt == 0
        a = np.where(single, F(0.0), mean[rank, me]).astype(F) if n else np.zeros(0, F)
        best = np.full(n, np.inf, F)
        arg = np.full(n, NO_LABEL, np.uint32)
        for k, L in enumerate(present):                                     # ascending label, strict <
            take = (mean[k] < best) & (rank != k)
            best = np.where(take, mean[k], best)
            arg = np.where(take, L, arg).astype(np.uint32)
        m = np.where(a < best, best, a)
        s = np.where(single, F(0.0), (best - a) / m).astype(F)
    score, nans = _score(s)
    return score, np.uint32(len(present)), np.uint32(nans), s, a, best, arg


def silhouette_float64(d, labels, axis=0):
    """s(i) in float64 with numpy's own sums: what the f32 chains approximate (finite non-negative matrices)."""
    d = np.asarray(d, np.float64)
    labels = np.asarray(labels)
    n = len(labels)
    dist = d if axis == 0 else d.T
    s = np.zeros(n)
    for i in range(n):
        others = np.arange(n) != i
        own = (labels == labels[i]) & others
        if not own.any():
            continue
        a = dist[i, own].mean()
        b = min((dist[i, labels == L].mean() for L in np.unique(labels) if L != labels[i]), default=np.inf)
        s[i] = (b - a) / max(a, b)
    return s


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x


def comparable(x):
    """bits(x) with every NaN as 0x7FC00000.  Which NaN an operation makes is the hardware's choice, not IEEE's and not the contract's:
    x86 gives INF - INF the sign bit (0xFFC00000) and passes an operand's payload on, the GPU makes 0x7FC00000.  The one NaN the
    contract spells out -- the score of a cut without a non-NaN s(i) -- is checked as raw bits where it occurs."""
    x = np.ascontiguousarray(x)
    if x.dtype != np.float32:
        return x
    return np.where(np.isnan(x), np.uint32(0x7FC00000), x.view(np.uint32))


def same(got, want):
    return all(np.array_equal(comparable(np.asarray(g)), comparable(np.asarray(w))) for g, w in zip(got, want)) and len(got) == len(want)


def assert_same(got, want, what=""):
    names = ("score", "clusters", "nans", "s", "a", "b", "nearest")
    assert len(got) == len(want), what
    for name, g, w in zip(names, got, want):
        g, w = np.atleast_1d(np.asarray(g)), np.atleast_1d(np.asarray(w))
        assert g.dtype == w.dtype and g.shape == w.shape, "%s: %s is %s %s, expected %s %s" % (what, name, g.dtype, g.shape, w.dtype, w.shape)
        bad = np.flatnonzero(comparable(g).ravel() != comparable(w).ravel())
        assert bad.size == 0, "%s: %s differs at %d places, first %d: got %r, expected %r" % (what, name, bad.size, bad[0], g.ravel()[bad[0]], w.ravel()[bad[0]])


def matrix(n, seed, kind="random"):
    """Asymmetric random matrices with a nonzero, partly NaN diagonal; `kind` adds the special values of the contract."""
    rng = np.random.default_rng(seed)
    d = rng.uniform(0.05, 4.0, (n, n)).astype(F)
    diag = rng.uniform(1.0, 9.0, n).astype(F)
    diag[::3] = np.nan
    d[np.arange(n), np.arange(n)] = diag
    if kind == "nan_row" and n > 1:
        d[n // 2, :] = np.nan
        d[:, n // 3] = np.nan
    elif kind == "inf" and n > 1:
        d[rng.integers(0, n, n), rng.integers(0, n, n)] = np.inf
    elif kind == "negative":
        d = (d - F(2.0)).astype(F)
    elif kind == "tiny":                                                     # sums of -1.4e-45 whose means round to -0.0
        d = np.where(rng.random((n, n)) < 0.5, F(-1e-45), F(0.0)).astype(F)
    elif kind == "ties":                                                     # small integers: equal means, a = b
        d = rng.integers(0, 3, (n, n)).astype(F)
    return d


KINDS = ("random", "nan_row", "inf", "negative", "tiny", "ties")
