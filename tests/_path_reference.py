"""Checker for the warping paths (include/apd.h, "warping paths"): TEST INFRASTRUCTURE, no GPU, no code shared with the product.

A restatement of the reference's table as a dict keyed (i, j) like its HashMap (alignments.rs:99-111,165-180), with the branch
every cell took (alignments.rs:153-159) recorded beside it, and the walk back from the score cell (n-1, m-1).  Every scalar is an
np.float32, so each operation rounds once as in the Rust build; the frame distances come from one f32 array operation per
reference operation (numerics.rs:114-120: difference, square, partial sum, square root -- numpy's f32 sqrt is correctly rounded),
in the style of oracle/np_reference.py::variance.
"""
import numpy as np

F = np.float32
INF = F(np.inf)
MATCH, INSERT, DELETE, START = 0, 1, 2, 3
STEP = np.dtype([("i", np.uint32), ("j", np.uint32), ("cost", np.float32), ("op", np.uint32)])


U64_MAX = (1 << 64) - 1


def band_from_pct(pct, length):
    """discovery.rs:38-45: f32 product, saturating truncation (Rust `as usize`): NaN and negatives give 0, a product at or beyond
    2^64 (+INF included) gives usize::MAX.  Never raises."""
    with np.errstate(all="ignore"):
        v = F(pct) * F(length)
    if np.isnan(v) or v <= 0:
        return 0
    if v >= F(2.0 ** 64):
        return U64_MAX
    return int(v)


def window(n, m, band):
    """alignments.rs:173, the band clamped to max(n, m) first (oracle/apd_oracle.h, "the band's domain"): where the reference's
    usize arithmetic overflows, the band is the full matrix."""
    return max(min(int(band), max(n, m)), abs(n - m)) + 2


def sq_distances(x, y):
    """numerics.rs:114-120 up to the square root: every difference, square and partial sum an f32 array operation that rounds once."""
    x, y = np.asarray(x, dtype=F), np.asarray(y, dtype=F)
    acc = np.zeros((len(x), len(y)), dtype=F)
    with np.errstate(all="ignore"):
        for k in range(x.shape[1]):
            t = x[:, None, k] - y[None, :, k]
            acc = acc + t * t
    return acc


def distances(x, y):
    """d[a][b] = euclidean(x[a], y[b]) (numerics.rs:114-120), every operation an f32 array operation that rounds once."""
    with np.errstate(all="ignore"):
        return np.sqrt(sq_distances(x, y))


def table(x, y, band, ins=1.0, dele=1.0, match=1.0):
    """construct_alignment (alignments.rs:165-180): (sparse, branch), both keyed (i, j) with 1-based table indices."""
    x, y = np.asarray(x, dtype=F), np.asarray(y, dtype=F)
    n, m = len(x), len(y)
    sparse, branch = {(0, 0): F(0.0)}, {}
    if n == 0 or m == 0:
        return sparse, branch
    d = distances(x, y)
    with np.errstate(all="ignore"):
        weighted = {MATCH: F(match) * d, INSERT: F(ins) * d, DELETE: F(dele) * d}      # pen * d, rounded on its own
    w = window(n, m, band)                                                             # :173
    with np.errstate(all="ignore"):                                                    # comparisons with NaN included
        for i in range(1, n + 1):                                                      # :174
            for j in range(max(i - w, 1), min(i + w, m + 1)):                          # :175
                ms = sparse.get((i - 1, j - 1), INF)                                   # :139
                is_ = sparse.get((i - 1, j), INF)                                      # :144
                ds = sparse.get((i, j - 1), INF)                                       # :149
                if ds < ms and ds < is_:                                               # :153
                    op, pred = DELETE, ds
                elif is_ < ms and is_ < ds:                                            # :155
                    op, pred = INSERT, is_
                else:
                    op, pred = MATCH, ms                                               # :158
                sparse[(i, j)] = F(pred + weighted[op][i - 1, j - 1])                  # :177
                branch[(i, j)] = op
    return sparse, branch


PRED = {MATCH: (-1, -1), INSERT: (-1, 0), DELETE: (0, -1)}


def path(x, y, band, ins=1.0, dele=1.0, match=1.0):
    """(steps as a STEP array, origin first; score as np.float32): the walk back from (n-1, m-1) through the table's branches."""
    n, m = len(x), len(y)
    if n == 0 and m == 0:
        return np.zeros(0, dtype=STEP), INF                                            # :117-118
    sparse, branch = table(x, y, band, ins, dele, match)
    cell = (n - 1, m - 1)                                                              # :120
    if cell not in sparse:
        return np.zeros(0, dtype=STEP), INF
    walked = []
    while True:
        if cell == (0, 0):
            walked.append((0, 0, sparse[cell], START))
            break
        op = branch[cell]
        walked.append((cell[0], cell[1], sparse[cell], op))
        cell = (cell[0] + PRED[op][0], cell[1] + PRED[op][1])
        if cell not in sparse:
            break
    steps = np.array(walked[::-1], dtype=STEP)
    with np.errstate(all="ignore"):
        score = F(steps["cost"][-1] / F(n + m))                                        # :121
    return steps, score


def replay(x, y, steps, ins=1.0, dele=1.0, match=1.0):
    """The costs of `steps` recomputed forward: an absent predecessor reads +INF, sparse[(0,0)] = 0, then pred + pen * d."""
    x, y = np.asarray(x, dtype=F), np.asarray(y, dtype=F)
    pen = {MATCH: F(match), INSERT: F(ins), DELETE: F(dele)}
    d = distances(x, y)
    out, prev = [], INF
    with np.errstate(all="ignore"):
        for s in steps:
            prev = F(0.0) if s["op"] == START else F(prev + F(pen[int(s["op"])] * d[int(s["i"]) - 1, int(s["j"]) - 1]))
            out.append(prev)
    return np.array(out, dtype=F)


def bits(a):
    """f32 values as uint32, every NaN mapped to one pattern.  IEEE 754 leaves the sign and payload of a NaN an operation makes
    (INF - INF, 0 * INF) to the implementation: x86 makes 0xFFC00000, gfx950 0x7FC00000.  Which cells are NaN is compared, and
    every other value bit for bit."""
    a = np.ascontiguousarray(a, dtype=F)
    b = a.view(np.uint32).copy()
    b[np.isnan(a)] = 0x7FC00000
    return b
