"""The seeded cases of the online detector's tests: TEST INFRASTRUCTURE, shared by tests/test_spot_online_reference.py (which asserts,
on the checker alone, that every case shows every event of the machine) and tests/test_gpu_spot_online.py (which runs them).

A case: a few queries, one stream per channel, penalties, a threshold per (channel, query), a hold-off and the grouping.  Streams
are words over a small alphabet of small-integer frames with the queries' own frames pasted in here and there, so exact matches
(cost 0), equal scores in overlapping windows and equal scores of two queries at one column all occur; per channel the last query
is a copy of the first, which ties with it wherever either is a candidate.  The thresholds are a quantile of each pair's own finite
scores, so they differ from pair to pair."""
import functools

import numpy as np

import _spot_online_reference as online
import _spot_reference as ref
from _path_reference import F

UNIT = (1.0, 1.0, 1.0)
SKEWED = (1.0, 2.0, 0.5)                        # (insertion, deletion, match)
# match = minus the smallest subnormal: an exact match costs +0.0, one with a mismatch or two a few subnormals below zero, and the
# division by n + window rounds those to -0.0 -- both zeros occur as scores, and f32 < says they tie
TINY = (1.0, 1.0, -1e-45)

# name: (seed, dim, stream frames per channel, query frames, per_stream, holdoff, penalties, threshold quantile -- None: a few 1e-30, above every score that is not positive)
SPECS = {
    "pairs_d13": (11, 13, (230, 171), (3, 5, 70, 130, 3), False, 4, UNIT, 0.30),
    "channels_d5": (12, 5, (150, 333, 201), (4, 3, 6, 4), True, 3, SKEWED, 0.35),
    "channels_d13": (13, 13, (400,), (5, 3, 5), True, 6, UNIT, 0.30),
    "channels_q65": (34, 13, (150,), tuple(3 + i % 3 for i in range(64)) + (3,), True, 3, UNIT, 0.30),
    "zeros_d2": (35, 2, (160, 150), (2, 3, 2), True, 2, TINY, None),
}


def build(seed, dim, stream_lengths, query_lengths, per_stream, holdoff, pen, quantile):
    rng = np.random.default_rng(seed)
    alphabet = rng.integers(0, 3, (3, dim)).astype(F)
    queries = [alphabet[rng.integers(0, 3, n)] for n in query_lengths[:-1]]
    queries.append(queries[0].copy())                                       # a copy: ties with query 0 on every channel
    assert len(queries[-1]) == query_lengths[-1]
    streams = []
    for m in stream_lengths:
        y = alphabet[rng.integers(0, 3, m)]
        for _ in range(max(2, m // 25)):                                    # paste queries in: exact matches, some of them cut short
            q = queries[int(rng.integers(0, len(queries)))]
            at = int(rng.integers(0, m))
            piece = q[:m - at]
            y[at:at + len(piece)] = piece
        streams.append(np.ascontiguousarray(y))
    lengths = [len(q) for q in queries]
    curves = [[ref.curves(q, y, *pen) for q in queries] for y in streams]
    thresholds = (1e-30 * (1 + np.arange(len(streams) * len(queries)))).astype(F).reshape(len(streams), len(queries))
    for k, per_query in enumerate(curves):
        for q, (cost, start) in enumerate(per_query):
            sc = ref.scores(cost, start, lengths[q])
            if quantile is not None:
                thresholds[k, q] = np.quantile(sc[np.isfinite(sc)], quantile).astype(F)
    return {"queries": queries, "streams": streams, "lengths": lengths, "curves": curves, "thresholds": thresholds, "pen": pen,
            "per_stream": per_stream, "holdoff": holdoff, "dim": dim}


@functools.lru_cache(maxsize=None)
def case(name):
    return build(*SPECS[name])


def subset(c, queries):
    """The case with only the listed queries (the thresholds and curves of the others dropped)."""
    out = dict(c)
    out["queries"] = [c["queries"][q] for q in queries]
    out["lengths"] = [c["lengths"][q] for q in queries]
    out["curves"] = [[per_query[q] for q in queries] for per_query in c["curves"]]
    out["thresholds"] = np.ascontiguousarray(c["thresholds"][:, queries])
    return out


def expected(c, upto=None, flush=False, stats=None, holdoff=None, per_stream=None, thresholds=None, origin=None, parts=False):
    """The checker on every channel of a case; `upto` and `origin`: one absolute column for all channels, or one per channel;
    flush: every channel is flushed after its last column (`upto`, or the stream's end).  Returns the hits in drain order (parts:
    (hits, when) per channel instead)."""
    n_ch = len(c["streams"])
    spread = lambda v: [v] * n_ch if v is None or np.isscalar(v) else list(v)       # noqa: E731
    upto, origin = spread(upto), spread(origin)
    per_stream = c["per_stream"] if per_stream is None else per_stream
    thresholds = c["thresholds"] if thresholds is None else np.broadcast_to(np.asarray(thresholds, dtype=F), c["thresholds"].shape)
    out = []
    for k in range(n_ch):
        m = len(c["streams"][k])
        last = m if upto[k] is None else min(int(upto[k]), m)
        out.append(online.channel_hits(k, c["curves"][k], c["lengths"], thresholds[k], per_stream, c["holdoff"] if holdoff is None else holdoff,
                                       origin=origin[k], upto=last, flush_at=[last] if flush else (), stats=stats))
    if parts:
        return out
    return online.ordered(np.concatenate([h for h, _ in out]), len(c["queries"]), per_stream)


def zero_sign_ties(c):
    """Columns of a per-channel case at which the candidates of one group hold a -0.0 and a +0.0 score."""
    count = 0
    for k, per_query in enumerate(c["curves"]):
        sc = np.array([ref.scores(cost, start, n) for (cost, start), n in zip(per_query, c["lengths"])])
        with np.errstate(invalid="ignore"):
            cand = (sc < c["thresholds"][k][:, None]) & (np.array([s for _, s in per_query]) != 0)
        neg = np.any(cand & (sc.view(np.uint32) == 0x80000000), axis=0)
        pos = np.any(cand & (sc.view(np.uint32) == 0), axis=0)
        count += int(np.sum(neg & pos))
    return count


def pending_at(c, k, b):
    """The windows pending on channel k once column b has been pushed: what a flush there would emit."""
    args = (k, c["curves"][k], c["lengths"], c["thresholds"][k], c["per_stream"], c["holdoff"])
    plain, _ = online.channel_hits(*args, upto=b)
    flushed, _ = online.channel_hits(*args, upto=b, flush_at=[b])
    known = {(int(h["pair"]), int(h["end"])) for h in plain}
    return [h for h in flushed if (int(h["pair"]), int(h["end"])) not in known]


def carried_across(c, size):
    """(windows pending at a multiple of `size` columns, those of them a later overlapping candidate replaced): a pending window
    carried from one push to the next, and a run of candidates that crosses the boundary."""
    carried = replaced = 0
    for k, y in enumerate(c["streams"]):
        final, _ = online.channel_hits(k, c["curves"][k], c["lengths"], c["thresholds"][k], c["per_stream"], c["holdoff"], flush_at=[len(y)])
        kept = {(int(h["pair"]), int(h["end"])) for h in final}
        for b in range(size, len(y), size):
            for h in pending_at(c, k, b):
                carried += 1
                replaced += (int(h["pair"]), int(h["end"])) not in kept
    return carried, replaced
