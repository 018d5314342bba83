"""Checker for the online detector of a streaming session (include/apd.h, "streaming spotting, online detection"): TEST
INFRASTRUCTURE, no GPU, no code shared with the product.

The hold-off machine restated in plain Python over WHOLE-STREAM curves of one channel (those of _spot_stream_reference or, with
first_column = 0, of _spot_reference): one loop over the absolute columns, the six steps in the header's order and in its per-column
wording -- the timer is looked at in every column, not only where a candidate stands.  Every score is one np.float32 division.

channel_hits() is one channel from one origin on; `upto` stops it after an absolute column ("what has been emitted once column L
was pushed"), `flush_at` flushes after given columns.  A reset is two runs: the old table up to the reset column, whose pending
windows are dropped by stopping there, then the fresh table's curves from the new first_column with the ranks carried over --
with_reset() does that.  ordered() gives the order a drain promises: ascending group, then ascending rank."""
import numpy as np

from _path_reference import F, bits

HIT = np.dtype([("pair", np.uint32), ("end", np.uint32), ("start", np.uint32), ("cost", np.float32), ("score", np.float32),
                ("rank", np.uint32)])
NEVER = 0xFFFFFFFF
EVENTS = ("replace", "equal_discard", "floor_discard", "timer", "displace", "tie")


def score_at(cost, start, n, j):
    """score(j) = cost / (float)(n + (j - start + 1)): one f32 division."""
    with np.errstate(all="ignore"):
        return F(F(cost) / F(n + (j - int(start) + 1)))


def new_stats():
    return {e: 0 for e in EVENTS + ("flush", "candidates")}


def channel_hits(channel, curves, lengths, thresholds, per_stream, holdoff, first_column=0, origin=None, upto=None, flush_at=(),
                 ranks=None, stats=None):
    """curves[q] = (cost, start) of query q on this channel, entry i being absolute column first_column + 1 + i, starts absolute;
    lengths[q], thresholds[q] per query.  The detector was armed at column `origin` (default: first_column).  Returns (hits, when):
    a HIT array, group-major and in emission order inside a group, and for every hit the absolute column at which it was emitted
    (the flushed column for a flush).  ranks: {group: next rank}, read and updated in place.  stats: event counts, updated."""
    n_q = len(curves)
    m = len(curves[0][0])
    origin = first_column if origin is None else int(origin)
    last = first_column + m if upto is None else min(int(upto), first_column + m)
    ranks = {} if ranks is None else ranks
    stats = new_stats() if stats is None else stats
    flush_at = set(int(c) for c in flush_at)
    thresholds = np.broadcast_to(np.asarray(thresholds, dtype=F), (n_q,))
    groups = [list(range(n_q))] if per_stream else [[q] for q in range(n_q)]
    out, when = [], []
    for members in groups:
        g = channel if per_stream else channel * n_q + members[0]
        pending, floor = None, origin                                        # pending: (pair, end, start, cost, score)

        def emit(column, why):
            nonlocal pending, floor
            out.append(pending + (ranks.get(g, 0),))
            when.append(column)
            ranks[g] = ranks.get(g, 0) + 1
            floor, pending = pending[1], None
            stats[why] += 1

        for j in range(origin + 1, last + 1):
            i = j - first_column - 1
            if pending is not None and j - pending[1] > holdoff:            # 1: the timer (0xFFFFFFFF: never)
                emit(j, "timer")
            c = None
            for q in members:                                                # the group's one candidate: smallest score, then smallest pair
                cost, start = curves[q][0][i], int(curves[q][1][i])
                score = score_at(cost, start, lengths[q], j)
                with np.errstate(invalid="ignore"):
                    below = bool(score < thresholds[q])                      # strict; NaN on either side: False
                if start == 0 or not below:
                    continue
                stats["candidates"] += 1
                if c is None or score < c[4]:
                    c = (channel * n_q + q, j, start, F(cost), score)
                elif score == c[4]:                                          # -0.0 == +0.0: a tie, the smaller pair stays
                    stats["tie"] += 1
            if c is not None:                                                # 2
                if c[2] <= floor:                                            # 3
                    stats["floor_discard"] += 1
                elif pending is None:                                        # 4
                    pending = c
                elif c[2] <= pending[1]:                                     # 5
                    if c[4] < pending[4]:
                        pending = c
                        stats["replace"] += 1
                    elif c[4] == pending[4]:
                        stats["equal_discard"] += 1
                else:                                                        # 6
                    emit(j, "displace")
                    pending = c
            if j in flush_at and pending is not None:
                emit(j, "flush")
    return np.array(out, dtype=HIT), np.array(when, dtype=np.int64)


def with_reset(channel, before, after, reset_at, first_column, lengths, thresholds, per_stream, holdoff, origin=0, upto=None, stats=None):
    """A channel that is reset after absolute column reset_at to `first_column`: `before` are the old table's curves (first column
    1), `after` the fresh table's (first column first_column + 1).  Pending windows die with the reset, the ranks go on."""
    ranks = {}
    a, wa = channel_hits(channel, before, lengths, thresholds, per_stream, holdoff, 0, origin, reset_at, ranks=ranks, stats=stats)
    b, wb = channel_hits(channel, after, lengths, thresholds, per_stream, holdoff, first_column, first_column, upto, ranks=ranks, stats=stats)
    return np.concatenate([a, b]), np.concatenate([wa, wb])


def group_of(hits, n_queries, per_stream):
    return hits["pair"] // n_queries if per_stream else hits["pair"]


def ordered(hits, n_queries, per_stream):
    """Ascending group, then ascending rank: the order of a drain."""
    hits = np.asarray(hits, dtype=HIT)
    return hits[np.lexsort((hits["rank"], group_of(hits, n_queries, per_stream)))]


def same_hits(got, want):
    """Every field of two HIT arrays equal, floats by their bits."""
    got, want = np.atleast_1d(got), np.atleast_1d(want)
    return (len(got) == len(want) and all(np.array_equal(got[f], want[f]) for f in ("pair", "end", "start", "rank"))
            and np.array_equal(bits(got["cost"]), bits(want["cost"])) and np.array_equal(bits(got["score"]), bits(want["score"])))
