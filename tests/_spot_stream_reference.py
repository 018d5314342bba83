"""Checker for the streaming spotting session (include/apd.h, "streaming spotting"): TEST INFRASTRUCTURE, no GPU, no code shared with
the product.

A chunked restatement of the contract in the style of tests/_spot_reference.py, column by column instead of row by row: a session
keeps T[i][c] and S[i][c], i = 1 .. n, of the last pushed column c (column 0: +INF and 0), the absolute number of that column and
the running best; a push walks the chunk's columns from there.  Row 0 of the table is 0 in every column, and an alignment that leaves
it in column J (a MATCH or an INSERT in row 1) starts at J, absolute.  Every scalar is an np.float32, so each operation rounds once;
the frame distances are _path_reference.distances (numerics.rs:114-120)."""
import numpy as np

from _path_reference import F, INF, bits, distances  # noqa: F401  (bits: re-exported for the tests)
from _spot_reference import BEST


def none_best():
    out = np.zeros((), dtype=BEST)
    out["cost"], out["score"] = INF, INF
    return out


class Session:
    """One (query, channel) pair of a session."""

    def __init__(self, x, ins=1.0, dele=1.0, match=1.0, first_column=0):
        self.x = np.asarray(x, dtype=F)
        self.n = len(self.x)
        assert self.n >= 1
        self.pen = (F(ins), F(dele), F(match))
        self.reset(first_column)

    def reset(self, first_column=0):
        self.col_t = [INF] * (self.n + 1)                  # [i] = T[i][c]; [0] is row 0 and is not read
        self.col_s = [0] * (self.n + 1)
        self.column = int(first_column)                    # absolute number of column c
        self.best = none_best()

    def push(self, y):
        """(cost, start, best): T[n][J] and S[n][J] of the chunk's columns, and the running best after it (a copy)."""
        y = np.asarray(y, dtype=F).reshape(-1, self.x.shape[1])
        m, n = len(y), self.n
        cost, start = np.zeros(m, dtype=F), np.zeros(m, dtype=np.uint32)
        if m == 0:
            return cost, start, self.best.copy()
        ins, dele, match = self.pen
        d = distances(self.x, y)
        with np.errstate(all="ignore"):
            w_match, w_ins, w_del = match * d, ins * d, dele * d               # pen * d, rounded on its own
        for k in range(m):
            J = self.column + 1
            old_t, old_s = self.col_t, self.col_s
            new_t, new_s = [F(0.0)] * (n + 1), [J] * (n + 1)                   # row 0: value 0; leaving it in column J starts at J
            for i in range(1, n + 1):
                ms = F(0.0) if i == 1 else old_t[i - 1]                        # (i-1, J-1)
                is_, ds = new_t[i - 1], old_t[i]                               # (i-1, J), (i, J-1)
                with np.errstate(all="ignore"):
                    if ds < ms and ds < is_:                                   # alignments.rs:153
                        new_t[i], new_s[i] = F(ds + w_del[i - 1, k]), old_s[i]
                    elif is_ < ms and is_ < ds:                                # :155
                        new_t[i], new_s[i] = F(is_ + w_ins[i - 1, k]), (J if i == 1 else new_s[i - 1])
                    else:                                                      # :158
                        new_t[i], new_s[i] = F(ms + w_match[i - 1, k]), (J if i == 1 else old_s[i - 1])
            self.col_t, self.col_s, self.column = new_t, new_s, J
            cost[k], start[k] = new_t[n], new_s[n]
            with np.errstate(all="ignore"):
                score = F(new_t[n] / F(n + (J - new_s[n] + 1)))                # one f32 division
            if score < self.best["score"]:                                     # strict: the smallest end wins, a NaN is never kept
                self.best["end"], self.best["start"], self.best["cost"], self.best["score"] = J, new_s[n], new_t[n], score
        return cost, start, self.best.copy()


def run(x, chunks, ins=1.0, dele=1.0, match=1.0, first_column=0):
    """[(cost, start, best)] of the pushes `chunks` of one stream, in order."""
    s = Session(x, ins, dele, match, first_column)
    return [s.push(c) for c in chunks]


def split(y, sizes):
    """The stream y cut into consecutive chunks of `sizes` frames (they must add up)."""
    y = np.asarray(y, dtype=F)
    assert sum(sizes) == len(y)
    cuts = np.cumsum((0,) + tuple(sizes))
    return [y[cuts[k]:cuts[k + 1]] for k in range(len(sizes))]


def prefix_bests(cost, start, n, first_column=0):
    """out[J]: the best of the first J columns of a whole stream's curves (out[0]: none), as one scan; columns absolute."""
    out = np.zeros(len(cost) + 1, dtype=BEST)
    out[0] = none_best()
    for j in range(1, len(cost) + 1):
        out[j] = out[j - 1]
        with np.errstate(all="ignore"):
            score = F(F(cost[j - 1]) / F(n + (first_column + j - int(start[j - 1]) + 1)))
        if score < out[j]["score"]:
            out[j] = (first_column + j, start[j - 1], cost[j - 1], score)
    return out
