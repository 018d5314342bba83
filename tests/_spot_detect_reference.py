"""Checker for spot detection (include/apd.h, "spot detection"): TEST INFRASTRUCTURE, no GPU, no code shared with the product.

Built on _spot_reference.curves / scores: the groups as the contract states them, the candidates (score < threshold, strictly, by
f32 comparison), the key (score, end, pair) and the greedy with the interval test `lo <= hi' and lo' <= hi`.  A candidate whose
start is 0 would contradict the contract (such a column costs +INF or NaN): asserted, not filtered.
"""
import numpy as np

import _spot_reference as ref
from _path_reference import F, bits

HIT = np.dtype([("pair", np.uint32), ("end", np.uint32), ("start", np.uint32), ("cost", np.float32), ("score", np.float32),
                ("rank", np.uint32)])


def groups_of(pairs, per_stream):
    """(group of every pair, label of every group): pair index per pair, else the distinct streams in order of first appearance."""
    if not per_stream:
        return list(range(len(pairs))), list(range(len(pairs)))
    labels, group = [], []
    for _, y in pairs:
        if int(y) not in labels:
            labels.append(int(y))
        group.append(labels.index(int(y)))
    return group, labels


def detect_curves(curves, lengths, pairs, thresholds, per_stream):
    """curves[p] = (cost, start) of pair p, lengths[p] = frames of its query.  Returns (hits, hit_off, labels, stats); stats counts, per
    group, the candidates, the rejected ones and the exact (score, end) ties between candidates of different pairs."""
    thresholds = np.broadcast_to(np.asarray(thresholds, dtype=F), (len(pairs),))
    group, labels = groups_of(pairs, per_stream)
    cands = [[] for _ in labels]
    for p, (cost, start) in enumerate(curves):
        sc = ref.scores(cost, start, lengths[p])
        for j in range(1, len(sc) + 1):
            with np.errstate(invalid="ignore"):
                below = bool(sc[j - 1] < thresholds[p])                     # NaN on either side: False
            if below:
                assert start[j - 1] != 0, "a candidate whose alignment ran through column 0"
                cands[group[p]].append((sc[j - 1], j, p, int(start[j - 1]), cost[j - 1]))
    out, hit_off, stats = [], [0], []
    for members in cands:
        members.sort(key=lambda c: (c[0], c[1], c[2]))                      # f32 <: -0.0 == 0.0 tie, then end, then pair
        taken, rejected = [], 0
        for score, end, p, lo, cost in members:
            if any(lo <= b and a <= end for a, b in taken):
                rejected += 1
                continue
            out.append((p, end, lo, cost, score, len(taken)))
            taken.append((lo, end))
        ties = sum(1 for a, b in zip(members[:-1], members[1:]) if a[0] == b[0] and a[1] == b[1] and a[2] != b[2])
        stats.append({"candidates": len(members), "hits": len(taken), "rejected": rejected, "ties": ties,
                      "pairs_hit": len({h[0] for h in out[hit_off[-1]:]})})
        hit_off.append(len(out))
    return np.array(out, dtype=HIT), np.array(hit_off, dtype=np.uint64), labels, stats


def detect(seqs, pairs, thresholds, per_stream, pen=(1.0, 1.0, 1.0), cache=None):
    """The whole contract from the sequences.  cache: a dict that keeps the curves of (x, y) between calls."""
    cache = {} if cache is None else cache
    curves = []
    for x, y in pairs:
        k = (int(x), int(y), tuple(pen))
        if k not in cache:
            cache[k] = ref.curves(seqs[int(x)], seqs[int(y)], *pen)
        curves.append(cache[k])
    return detect_curves(curves, [len(seqs[int(x)]) for x, _ in pairs], pairs, thresholds, per_stream)


def same_hits(got, want):
    """Every field of two HIT arrays equal, floats by their bits."""
    got, want = np.atleast_1d(got), np.atleast_1d(want)
    return (len(got) == len(want) and all(np.array_equal(got[f], want[f]) for f in ("pair", "end", "start", "rank"))
            and np.array_equal(bits(got["cost"]), bits(want["cost"])) and np.array_equal(bits(got["score"]), bits(want["score"])))


def median_threshold(curves, lengths):
    """The median finite score over the curves of a case: about half of the finite columns become candidates."""
    sc = np.concatenate([ref.scores(c, s, n) for (c, s), n in zip(curves, lengths)])
    return F(np.median(sc[np.isfinite(sc)]))


def seeded_cases(count=40, seed=7):
    """The per-stream sweep's case list: integer features in {0, 1, 2}, D in {1, 2}, m in [40, 140), three queries of 2 .. 6 frames cut
    from the stream, the third a copy of the first; threshold = the median finite score.  Each case: (seqs, pairs, threshold, the pairs' curves)."""
    rng = np.random.default_rng(seed)
    cases = []
    for _ in range(count):
        dim = int(rng.integers(1, 3))
        m = int(rng.integers(40, 140))
        stream = rng.integers(0, 3, (m, dim)).astype(F)
        queries = []
        for _ in range(2):
            n = int(rng.integers(2, 7))
            at = int(rng.integers(0, m - n + 1))
            queries.append(stream[at:at + n].copy())
        queries.append(queries[0].copy())
        seqs = queries + [stream]
        pairs = [(0, 3), (1, 3), (2, 3)]
        curves = [ref.curves(seqs[x], seqs[y]) for x, y in pairs]
        cases.append((seqs, pairs, median_threshold(curves, [len(seqs[x]) for x, _ in pairs]), curves))
    return cases
