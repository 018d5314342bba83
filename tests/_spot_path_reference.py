"""Checker for the warping paths of spotted windows (include/apd.h, "warping paths of spotted windows"): TEST INFRASTRUCTURE, no GPU,
no code shared with the product.

A restatement of the contract on top of tests/_spot_reference.py and tests/_path_reference.py: the whole free-start table T with the
start column S and the branch of every cell (alignments.rs:153-159), the walk back from (n, end) to row 0, the slots a window owns,
and what the call reports for a window: the start it found, the score, and the path or nothing.  Every scalar is an np.float32, so
each operation rounds once.
"""
import numpy as np

from _path_reference import DELETE, F, INF, INSERT, MATCH, PRED, START, STEP, bits, distances, replay  # noqa: F401  (re-exported)

WINDOW = np.dtype([("x", np.uint32), ("y", np.uint32), ("end", np.uint32), ("start", np.uint32)])


def table(x, y, ins=1.0, dele=1.0, match=1.0, first=1):
    """(T, S, B), each [n + 1][m + 1]: T[0][j] = 0, T[i][0] = +INF, S[i][0] = 0; B[i][j] the branch of cell (i, j), i, j >= 1.
    first > 1: the same recurrence on columns first .. m ALONE -- column first - 1 plays column 0, the columns before it stay
    unswept -- which is NOT the table."""
    x, y = np.asarray(x, dtype=F), np.asarray(y, dtype=F)
    n, m = len(x), len(y)
    assert n >= 1 and m >= 1
    d = distances(x, y)
    with np.errstate(all="ignore"):
        weighted = {MATCH: F(match) * d, INSERT: F(ins) * d, DELETE: F(dele) * d}      # pen * d, rounded on its own
    T = [[F(0.0)] * (m + 1)] + [[INF] * (m + 1) for _ in range(n)]
    S = [[0] * (m + 1) for _ in range(n + 1)]
    B = [[None] * (m + 1) for _ in range(n + 1)]
    for i in range(1, n + 1):
        for j in range(first, m + 1):
            ms, is_, ds = T[i - 1][j - 1], T[i - 1][j], T[i][j - 1]
            with np.errstate(all="ignore"):
                if ds < ms and ds < is_:                                               # alignments.rs:153
                    op, pred, s = DELETE, ds, S[i][j - 1]
                elif is_ < ms and is_ < ds:                                            # :155
                    op, pred, s = INSERT, is_, (j if i == 1 else S[i - 1][j])
                else:                                                                  # :158
                    op, pred, s = MATCH, ms, (j if i == 1 else S[i - 1][j - 1])
                T[i][j] = F(pred + weighted[op][i - 1, j - 1])
            S[i][j], B[i][j] = s, op
    return T, S, B


def walk(tab, n, end):
    """The walk back from (n, end): (steps as a STEP array, origin first; entered_column_0).  A cell of column 0 ends the walk
    without a START (the contract never walks there: S is 0 then)."""
    T, _, B = tab
    i, j, walked = n, end, []
    while True:
        if i == 0:
            walked.append((0, j, F(0.0), START))
            break
        if j == 0:
            return np.array(walked[::-1], dtype=STEP), True
        op = B[i][j]
        walked.append((i, j, T[i][j], op))
        i, j = i + PRED[op][0], j + PRED[op][1]
    return np.array(walked[::-1], dtype=STEP), False


def bound(n, end, start):
    """apd_spot_path_bound."""
    return n + (end - start + 1) if n >= 1 and 1 <= start <= end else 0


def answer(tab, n, end, start):
    """What apd_spot_paths reports for the window (end, start) of a pair whose table is `tab`:
    (steps, found_start, score as np.float32).  No window, or a start that is not the table's: no steps."""
    T, S, _ = tab
    if end == 0 or start == 0:
        return np.zeros(0, dtype=STEP), 0, INF
    found = S[n][end]
    with np.errstate(all="ignore"):
        score = F(T[n][end] / F(n + end - found + 1))
    if found != start:
        return np.zeros(0, dtype=STEP), found, score
    steps, entered = walk(tab, n, end)
    assert not entered
    return steps, found, score


def same_steps(got, want):
    """Two STEP arrays equal field by field, costs by their bits."""
    return (len(got) == len(want) and np.array_equal(got["i"], want["i"]) and np.array_equal(got["j"], want["j"])
            and np.array_equal(got["op"], want["op"]) and np.array_equal(bits(got["cost"]), bits(want["cost"])))
