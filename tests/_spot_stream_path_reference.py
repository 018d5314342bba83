"""Checker for the warping paths of a streaming session (include/apd.h, "a kept history of columns"): TEST INFRASTRUCTURE, no GPU, no
code shared with the product.

A chunk-by-chunk restatement of the contract in f32 scalars, on top of tests/_spot_stream_reference.py: a session that REALLY keeps
only H columns -- the branch of every cell, row n's value and start, the stream frame -- in rings indexed by the absolute column
modulo H, overwrites them as the chunks arrive, and answers a window from the rings alone: S[n][end] and T[n][end] from the curve
ring, the walk back through the branch ring, the costs by the forward replay (a table value IS predecessor + pen * d in these
operations) over the query and the frame ring.  What a window outside the rings gets is decided from `kept()` before a ring is read.
"""
import numpy as np

import _spot_stream_reference as sref
from _path_reference import DELETE, F, INF, INSERT, MATCH, PRED, START, STEP, distances

NONE = (np.zeros(0, dtype=STEP), 0, INF)


class Session(sref.Session):
    """One (query, channel) pair of a session with a history of `history` columns (0: none)."""

    def __init__(self, x, ins=1.0, dele=1.0, match=1.0, first_column=0, history=0):
        self.H = 0
        super().__init__(x, ins, dele, match, first_column)
        self.keep(history)

    def reset(self, first_column=0):
        super().reset(first_column)
        self.origin = self.column                              # the history is empty, behind the new first column

    def keep(self, history):
        self.H = int(history)
        self.origin = self.column                              # whatever was kept before is gone
        self.ring_b = [None] * self.H                          # [J % H][i]: branch of cell (i, J)
        self.ring_c = [None] * self.H                          # [J % H]: (T[n][J], S[n][J])
        self.ring_y = [None] * self.H                          # [J % H]: frame of column J

    def kept(self):
        """(first, last) of the kept columns; first == last + 1: none."""
        last = self.column
        return (max(self.origin + 1, last - self.H + 1) if self.H else last + 1), last

    def push(self, y):
        """As the parent's, column by column, and every column goes to the rings."""
        y = np.asarray(y, dtype=F).reshape(-1, self.x.shape[1])
        m, n = len(y), self.n
        cost, start = np.zeros(m, dtype=F), np.zeros(m, dtype=np.uint32)
        if m == 0:
            return cost, start, self.best.copy()
        ins, dele, match = self.pen
        d = distances(self.x, y)
        with np.errstate(all="ignore"):
            weighted = {MATCH: match * d, INSERT: ins * d, DELETE: dele * d}   # pen * d, rounded on its own
        for k in range(m):
            J = self.column + 1
            old_t, old_s = self.col_t, self.col_s
            new_t, new_s, ops = [F(0.0)] * (n + 1), [J] * (n + 1), [START] * (n + 1)
            for i in range(1, n + 1):
                ms = F(0.0) if i == 1 else old_t[i - 1]                        # (i-1, J-1)
                is_, ds = new_t[i - 1], old_t[i]                               # (i-1, J), (i, J-1)
                with np.errstate(all="ignore"):
                    if ds < ms and ds < is_:                                   # alignments.rs:153
                        op, pred, s = DELETE, ds, old_s[i]
                    elif is_ < ms and is_ < ds:                                # :155
                        op, pred, s = INSERT, is_, (J if i == 1 else new_s[i - 1])
                    else:                                                      # :158
                        op, pred, s = MATCH, ms, (J if i == 1 else old_s[i - 1])
                    new_t[i] = F(pred + weighted[op][i - 1, k])
                new_s[i], ops[i] = s, op
            self.col_t, self.col_s, self.column = new_t, new_s, J
            cost[k], start[k] = new_t[n], new_s[n]
            if self.H:
                self.ring_b[J % self.H], self.ring_c[J % self.H], self.ring_y[J % self.H] = ops, (new_t[n], new_s[n]), y[k].copy()
            with np.errstate(all="ignore"):
                score = F(new_t[n] / F(n + (J - new_s[n] + 1)))                # one f32 division
            if score < self.best["score"]:                                     # strict: the smallest end wins, a NaN is never kept
                self.best["end"], self.best["start"], self.best["cost"], self.best["score"] = J, new_s[n], new_t[n], score
        return cost, start, self.best.copy()

    def answer(self, end, start):
        """What apd_spot_stream_paths reports for the window (end, start), absolute columns: (steps, found_start, score)."""
        n, H = self.n, self.H
        first, last = self.kept()
        assert end <= last and (end == 0 or start <= end)
        if end == 0 or start == 0 or end < first:              # no window, or its end has aged out
            return NONE
        t_end, found = self.ring_c[end % H]
        with np.errstate(all="ignore"):
            score = F(t_end / F(n + end - found + 1))
        if found != start or found < first:                    # a wrong start, or a start that has aged out
            return np.zeros(0, dtype=STEP), found, score
        i, j, walked = n, end, []
        while i >= 1:
            assert first <= j <= end                           # the walk stays inside columns S .. end
            op = self.ring_b[j % H][i]
            walked.append((i, j, op))
            i, j = i + PRED[op][0], j + PRED[op][1]
        pen = {MATCH: self.pen[2], INSERT: self.pen[0], DELETE: self.pen[1]}
        steps, value = [(0, j, F(0.0), START)], F(0.0)
        for i, j, op in walked[::-1]:                          # the replay: predecessor + pen * d, each rounded on its own
            d = distances(self.x[i - 1:i], self.ring_y[j % H][None, :])[0, 0]
            with np.errstate(all="ignore"):
                value = F(value + F(pen[op] * d))
            steps.append((i, j, value, op))
        return np.array(steps, dtype=STEP), found, score


def expected(whole, n, first_column, kept, end, start):
    """The contract from the WHOLE stream's answer: `whole` = _spot_path_reference.answer(table, n, end - first_column, start -
    first_column) of the stream since the reset, kept = (first, last).  Shifts it, and applies the aged-out rules."""
    first, _ = kept
    steps, found, score = whole
    if end == 0 or start == 0 or end < first:
        return NONE
    found = found + first_column if found > 0 else 0
    if found != start or found < first:
        return np.zeros(0, dtype=STEP), found, score
    steps = steps.copy()
    steps["j"] += np.uint32(first_column)
    return steps, found, score
