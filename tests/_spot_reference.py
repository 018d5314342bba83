"""Checker for the subsequence alignment (include/apd.h, "subsequence alignment"): TEST INFRASTRUCTURE, no GPU, no code shared with
the product.

A restatement of the contract in the style of tests/_path_reference.py: the table T with a free start (row 0 is 0 in every column,
column 0 is +INF below it), the select of alignments.rs:153-159 in every cell, the start column S carried with the value, the
curves of row n, the score with the matched window's length in place of m, and the scan for the best column.  Every scalar is an
np.float32, so each operation rounds once; the frame distances are _path_reference.distances (numerics.rs:114-120).
"""
import numpy as np

from _path_reference import F, INF, bits, distances  # noqa: F401  (bits: re-exported for the tests)

BEST = np.dtype([("end", np.uint32), ("start", np.uint32), ("cost", np.float32), ("score", np.float32)])


def curves(x, y, ins=1.0, dele=1.0, match=1.0):
    """(cost, start): cost[j-1] = T[n][j] as float32, start[j-1] = S[n][j] as uint32, for j = 1 .. m."""
    x, y = np.asarray(x, dtype=F), np.asarray(y, dtype=F)
    n, m = len(x), len(y)
    assert n >= 1 and m >= 1
    d = distances(x, y)
    with np.errstate(all="ignore"):
        w_match, w_ins, w_del = F(match) * d, F(ins) * d, F(dele) * d          # pen * d, rounded on its own
    prev_t, prev_s = [F(0.0)] * (m + 1), [0] * (m + 1)                         # row 0: free start
    for i in range(1, n + 1):
        row_t, row_s = [INF] * (m + 1), [0] * (m + 1)                          # T[i][0] = +INF, nothing starts there
        for j in range(1, m + 1):
            ms, is_, ds = prev_t[j - 1], prev_t[j], row_t[j - 1]
            with np.errstate(all="ignore"):
                if ds < ms and ds < is_:                                       # alignments.rs:153
                    row_t[j], row_s[j] = F(ds + w_del[i - 1, j - 1]), row_s[j - 1]
                elif is_ < ms and is_ < ds:                                    # :155
                    row_t[j], row_s[j] = F(is_ + w_ins[i - 1, j - 1]), (j if i == 1 else prev_s[j])
                else:                                                          # :158
                    row_t[j], row_s[j] = F(ms + w_match[i - 1, j - 1]), (j if i == 1 else prev_s[j - 1])
        prev_t, prev_s = row_t, row_s
    return np.array(prev_t[1:], dtype=F), np.array(prev_s[1:], dtype=np.uint32)


def scores(cost, start, n):
    """score(j) = cost / (float)(n + L), L = j - start + 1: one f32 division."""
    cost = np.asarray(cost, dtype=F)
    j = np.arange(1, len(cost) + 1, dtype=np.int64)
    length = j - np.asarray(start, dtype=np.int64) + 1
    with np.errstate(all="ignore"):
        return (cost / (n + length).astype(F)).astype(F)


def best(cost, start, n):
    """The scan of j ascending: a column is kept only if its score is strictly below the best so far, starting from +INF."""
    out = np.zeros((), dtype=BEST)
    out["cost"], out["score"] = INF, INF
    for j, s in enumerate(scores(cost, start, n), start=1):
        if s < out["score"]:
            out["end"], out["start"], out["cost"], out["score"] = j, start[j - 1], cost[j - 1], s
    return out


def spot(x, y, ins=1.0, dele=1.0, match=1.0):
    """(cost, start, best) of the query x against the stream y."""
    cost, start = curves(x, y, ins, dele, match)
    return cost, start, best(cost, start, len(x))


def hits(cost, start, n, threshold):
    """Greedy non-overlapping peak picking: candidates with score < threshold in ascending score, the smaller end first among equal
    scores; accepted if [start, end] shares no column with an accepted window.  A BEST array in acceptance order."""
    sc = scores(cost, start, n)
    cand = [j for j in range(1, len(sc) + 1) if sc[j - 1] < F(threshold)]
    cand.sort(key=lambda j: (sc[j - 1], j))
    taken, out = [], []
    for j in cand:
        lo, hi = int(start[j - 1]), j
        if all(hi < a or lo > b for a, b in taken):
            taken.append((lo, hi))
            out.append((hi, lo, cost[j - 1], sc[j - 1]))
    return np.array(out, dtype=BEST)


def same_best(got, want):
    """Every field of two BEST records (or arrays) equal, floats by their bits."""
    got, want = np.atleast_1d(got), np.atleast_1d(want)
    return (np.array_equal(got["end"], want["end"]) and np.array_equal(got["start"], want["start"])
            and np.array_equal(bits(got["cost"]), bits(want["cost"])) and np.array_equal(bits(got["score"]), bits(want["score"])))
