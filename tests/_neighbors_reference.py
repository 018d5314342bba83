"""Checker for apd_neighbors (include/apd.h): TEST INFRASTRUCTURE, no GPU, no code shared with the product.

The contract restated in plain Python over a numpy float32 matrix.  Per query: its row (axis 0) or column (axis 1), NaN entries
dropped, entry `q` dropped with skip_self, the rest sorted by (float(v), j) -- Python compares -0.0 == 0.0, so the two zeros tie and
the smaller j goes first, and +INF sorts behind every finite value -- the first k kept, the rest of the k slots padded."""
import numpy as np

F = np.float32
PAD_INDEX = 0xFFFFFFFF
PAD_BITS = 0x7FC00000


class Ranked:
    """Every row (axis 0) or column (axis 1) of d with its candidates in the contract's order: computed once, shared by the tests
    that take different k or different queries from it, never changed."""

    def __init__(self, d, axis=0, skip_self=False):
        self.d = np.array(d, dtype=F)
        assert self.d.ndim == 2 and axis in (0, 1)
        self.axis = axis
        self.order, self.nans = [], []
        for q in range(self.d.shape[axis]):
            line = self.d[q, :] if axis == 0 else self.d[:, q]
            candidates, nans = [], 0
            for j, v in enumerate(line.tolist()):                        # Python floats: exactly float(v)
                if skip_self and j == q:
                    continue
                if v != v:
                    nans += 1
                    continue
                candidates.append((j, v))
            self.order.append([j for j, v in sorted(candidates, key=lambda c: (c[1], c[0]))])   # -0.0 == 0.0: the smaller j first
            self.nans.append(nans)

    def take(self, k, queries=None):
        """(index uint32 [Q][k], distance float32 [Q][k], count uint32 [Q], nans uint32 [Q])."""
        assert k >= 1
        queries = range(len(self.order)) if queries is None else [int(q) for q in queries]
        index = np.full((len(queries), k), PAD_INDEX, np.uint32)
        bits = np.full((len(queries), k), PAD_BITS, np.uint32)
        count, nans = np.zeros(len(queries), np.uint32), np.zeros(len(queries), np.uint32)
        for s, q in enumerate(queries):
            line = (self.d[q, :] if self.axis == 0 else self.d[:, q]).view(np.uint32)
            kept = np.asarray(self.order[q][:k], np.intp)
            count[s], nans[s] = len(kept), self.nans[q]
            index[s, :len(kept)] = kept
            bits[s, :len(kept)] = line[kept]                             # the matrix's own bits
        return index, bits.view(F), count, nans


def reference(d, k, axis=0, skip_self=False, queries=None):
    return Ranked(d, axis, skip_self).take(k, queries)


def reference_lexsort(d, k, axis=0, skip_self=False):
    """The same answer for every row / column by one np.lexsort per query: an independent formulation (keys: value with the zeros
    merged, then index; NaN and self pushed behind everything and cut off by the count)."""
    d = np.asarray(d, dtype=F)
    lines = d if axis == 0 else d.T
    n_q, n = lines.shape
    index = np.full((n_q, k), PAD_INDEX, np.uint32)
    bits = np.full((n_q, k), PAD_BITS, np.uint32)
    count, nans = np.zeros(n_q, np.uint32), np.zeros(n_q, np.uint32)
    for q in range(n_q):
        v = lines[q]
        drop = np.isnan(v)
        if skip_self and q < n:
            nans[q] = int(drop.sum()) - int(drop[q])
            drop = drop.copy()
            drop[q] = True
        else:
            nans[q] = int(drop.sum())
        value = np.where(drop, F(0), v) + F(0)                            # -0.0 + 0.0 = +0.0: one zero
        order = np.lexsort((np.arange(n), value.astype(np.float64), drop))   # last key first: kept entries, then value, then index
        c = min(k, n - int(drop.sum()))
        count[q] = c
        index[q, :c] = order[:c]
        bits[q, :c] = v[order[:c]].view(np.uint32)
    return index, bits.view(F), count, nans


def same(got, want):
    """Bitwise: index, the bits of distance, count, nans."""
    return (np.array_equal(np.asarray(got[0], np.uint32), want[0]) and
            np.array_equal(np.ascontiguousarray(got[1], F).view(np.uint32), np.ascontiguousarray(want[1], F).view(np.uint32)) and
            np.array_equal(np.asarray(got[2], np.uint32), want[2]) and np.array_equal(np.asarray(got[3], np.uint32), want[3]))


def assert_same(got, want, what):
    names = ("index", "distance bits", "count", "nans")
    for name, g, w in zip(names, got, want):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        if g.dtype == F:
            g, w = g.view(np.uint32), w.view(np.uint32)
        assert g.shape == w.shape, "%s: %s has shape %s, expected %s" % (what, name, g.shape, w.shape)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, "%s: %s differs at %d places, first %s: got %s, expected %s" % (
            what, name, len(bad), tuple(bad[0]), g[tuple(bad[0])], w[tuple(bad[0])])


def values(kind, rows, cols, seed, k=16):
    """The value families of the GPU tests, seeded (k: only "inf" reads it)."""
    rng = np.random.default_rng(seed)
    if kind == "ties":                       # integer-valued: ties dominate every digit pass, the tie compaction decides most slots
        return rng.integers(0, 3, (rows, cols)).astype(F)
    if kind == "equal":
        return np.full((rows, cols), 2.5, F)
    if kind == "zeros":                      # +-0.0 mixed, a few other values
        d = np.where(rng.random((rows, cols)) < 0.5, F(-0.0), F(0.0)).astype(F)
        d[rng.random((rows, cols)) < 0.2] = F(1.0)
        d[rng.random((rows, cols)) < 0.1] = F(-1.0)
        return d
    if kind == "inf":                        # min(k, cols) // 2 finite entries per row: more +INF than cols - k, INF reaches the output
        d = np.full((rows, cols), np.inf, F)
        for r in range(rows):
            at = rng.choice(cols, size=min(k, cols) // 2, replace=False)
            d[r, at] = rng.random(len(at), dtype=F)
        return d
    if kind == "nan":                        # 10 % NaN and one row of nothing else
        d = rng.standard_normal((rows, cols)).astype(F)
        d[rng.random((rows, cols)) < 0.1] = np.nan
        d[rows // 2, :] = np.nan
        return d
    if kind == "subnormal":                  # negative values, subnormals of both signs, zeros
        d = (rng.standard_normal((rows, cols)) * 3).astype(F)
        tiny = rng.integers(1, 1 << 22, (rows, cols)).astype(np.uint32) | (rng.integers(0, 2, (rows, cols)).astype(np.uint32) << 31)
        pick = rng.random((rows, cols)) < 0.4
        d[pick] = tiny.view(F)[pick]
        d[rng.random((rows, cols)) < 0.05] = 0.0
        return d
    if kind == "bits":                       # the whole of f32: random bit patterns, NaNs and infinities among them
        return rng.integers(0, 1 << 32, (rows, cols), dtype=np.uint64).astype(np.uint32).view(F)
    raise ValueError(kind)


KINDS = ("ties", "equal", "zeros", "inf", "nan", "subnormal", "bits")
