"""Checker for spot score quantiles (include/apd.h, "spot score quantiles"): TEST INFRASTRUCTURE, no GPU, no code shared with the
product.

Built on _spot_reference.curves / scores: the groups as the contract states them, the population of a group (one score per stream
column of every pair of the group, a repeated pair as often as listed), and numerics.rs:125-133 on it -- NaN dropped, np.sort after
-0.0 was made +0.0, the element at trunc(f32(entries) * f32(perc)) of the UNFILTERED length, APD_ERR_INDEX beyond the non-NaN scores.
Also the two sources of cases the GPU tests run: a seeded generator over the shapes the select's paths turn on, and multisets
dictated through one-frame queries.
"""
import numpy as np

import _spot_reference as ref
from _path_reference import F, bits  # noqa: F401  (bits: re-exported for the tests)

OK, ERR_INDEX = 0, -7
NAN_BITS = 0x7FC00000                           # the value of a rank beyond the population
BYS = ("pair", "query", "all")
UNIT = (1.0, 1.0, 1.0)


def groups_of(pairs, by):
    """(group of every pair, label of every group): the pair index per pair, the distinct queries in order of first appearance, or
    one group (none for an empty list)."""
    pairs = [(int(x), int(y)) for x, y in pairs]
    if by == "pair":
        return list(range(len(pairs))), list(range(len(pairs)))
    if by == "all":
        return [0] * len(pairs), ([0] if pairs else [])
    assert by == "query"
    labels, group = [], []
    for x, _ in pairs:
        if x not in labels:
            labels.append(x)
        group.append(labels.index(x))
    return group, labels


def percentile_index(entries, perc):
    """(entries as f32 * perc) as usize: an f32 product, truncated, saturating (NaN and negatives give 0)."""
    with np.errstate(all="ignore"):
        nf = F(entries) * F(perc)
    if not nf > 0:
        return 0
    return int(nf) if nf < F(2.0 ** 64) else 2 ** 64 - 1


def populations(curves, lengths, pairs, by):
    """The scores of every group, unsorted: curves[p] = (cost, start) of pair p, lengths[p] = frames of its query."""
    group, labels = groups_of(pairs, by)
    parts = [[] for _ in labels]
    for p, (cost, start) in enumerate(curves):
        parts[group[p]].append(ref.scores(cost, start, lengths[p]))
    return [np.concatenate(s) for s in parts], group


def quantiles(curves, lengths, pairs, by, perc):
    """(values [n_groups, n_perc] f32, status [n_groups, n_perc] i32, group_of, entries, nans, k [n_groups, n_perc] as Python ints)."""
    perc = np.atleast_1d(np.asarray(perc, dtype=F))
    pops, group = populations(curves, lengths, pairs, by)
    values = np.zeros((len(pops), len(perc)), dtype=F)
    status = np.zeros((len(pops), len(perc)), dtype=np.int32)
    entries, nans, ks = [], [], []
    for g, pop in enumerate(pops):
        kept = pop[~np.isnan(pop)]
        kept = np.sort(np.where(kept == 0, F(0.0), kept))                  # -0.0 and +0.0 tie and come back as +0.0
        entries.append(len(pop))
        nans.append(len(pop) - len(kept))
        ks.append([percentile_index(len(pop), q) for q in perc])
        for q, k in enumerate(ks[-1]):
            if k >= len(kept):
                values[g, q], status[g, q] = np.array([NAN_BITS], dtype=np.uint32).view(F)[0], ERR_INDEX
            else:
                values[g, q] = kept[k]
    return values, status, np.array(group, dtype=np.uint64), np.array(entries, dtype=np.uint64), np.array(nans, dtype=np.uint64), ks


def perc_for_rank(entries, k):
    """A perc whose index into a population of `entries` is exactly k (1 <= k < 2^23: the product is then exact enough to search)."""
    p = F((k + 0.5) / float(F(entries)))
    for _ in range(64):
        got = percentile_index(entries, p)
        if got == k:
            return p
        p = np.nextafter(p, F(np.inf) if got < k else F(-np.inf))
    raise AssertionError("no perc reaches rank %d of %d" % (k, entries))


# ---- seeded cases

def _corpus(rng, dim, query_lens, stream_lens, integer, nan_in=None, inf_in=None):
    draw = (lambda n: rng.integers(0, 3, (n, dim)).astype(F)) if integer else (lambda n: rng.standard_normal((n, dim)).astype(F))
    seqs = [draw(n) for n in query_lens] + [draw(m) for m in stream_lens]
    if nan_in is not None:
        s = seqs[len(query_lens) + nan_in]
        s[rng.choice(len(s), 3, replace=False), 0] = np.nan
    if inf_in is not None:
        s = seqs[len(query_lens) + inf_in]
        s[rng.choice(len(s), 2, replace=False), 1] = np.inf
    return seqs


def seeded_cases(columns=256, seed=20261):
    """The GPU sweep's case list.  Three corpora -- D = 8 gaussian under unit penalties; D = 13 gaussian under skewed ones, one stream
    with NaN frames, one with infinite frames; D = 8 with features in {0, 1, 2} under penalties <= 0 (ties, negative scores) --, queries
    of 1, 7 and 65 frames against streams of 1, 2, 63, 64, 65 and columns - 1, columns, columns + 1, 2 columns + 3 frames (`columns`:
    what a workgroup of the select takes per step), a pair with x == y, repeated pairs, the list shuffled.  Every corpus runs under all
    three groupings with one perc and with eight, two of the eight aimed at the last non-NaN rank of the corpus' by="all" group and
    at the one beyond.  Each case: dict(seqs, pairs, pen, by, perc, curves, lengths); the curves are computed once per corpus."""
    rng = np.random.default_rng(seed)
    stream_lens = [1, 2, 63, 64, 65, columns - 1, columns, columns + 1, 2 * columns + 3]
    corpora = [
        (_corpus(rng, 8, [1, 7, 65], stream_lens, False), 3, UNIT),
        (_corpus(rng, 13, [1, 7, 65], stream_lens, False, nan_in=4, inf_in=7), 3, (1.0, 2.0, 0.5)),
        (_corpus(rng, 8, [1, 7], [63, 65, 130], True), 2, (-1.0, -0.5, -1.0)),
    ]
    cases = []
    for seqs, n_queries, pen in corpora:
        pairs = [(x, y) for x in range(n_queries) for y in range(n_queries, len(seqs))]
        pairs += [(n_queries - 1, n_queries - 1), (1, 1), pairs[3], pairs[3], pairs[-1]]       # x == y twice, repeats
        pairs = [pairs[i] for i in rng.permutation(len(pairs))]
        cache = {}
        for x, y in pairs:
            if (x, y) not in cache:
                cache[(x, y)] = ref.curves(seqs[x], seqs[y], *pen)
        curves = [cache[p] for p in pairs]
        lengths = [len(seqs[x]) for x, _ in pairs]
        _, _, _, entries, nans, _ = quantiles(curves, lengths, pairs, "all", [0.0])
        live = int(entries[0]) - int(nans[0])
        eight = np.array([0.0, 0.001, 0.05, 0.5, 0.95, 1.0, perc_for_rank(int(entries[0]), live - 1), perc_for_rank(int(entries[0]), live)], dtype=F)
        for by in BYS:
            for perc in (np.array([0.5], dtype=F), eight):
                cases.append(dict(seqs=seqs, pairs=pairs, pen=pen, by=by, perc=perc, curves=curves, lengths=lengths))
    return cases


# ---- dictated multisets

def dictated(scores, dim=8):
    """(query, stream): a one-frame query of zeros and a stream whose frame j differs from it in coordinate 0 only, by 2 scores[j].
    Under unit penalties row 1 takes MATCH from row 0 in every column (0 < 0 is false twice), so start = j, cost = |2 s_j| and
    score(j) = |2 s_j| / (float)(1 + 1) = s_j bit for bit, for s_j >= 0, NaN or +INF with 4 s_j^2 neither overflowing nor subnormal."""
    scores = np.asarray(scores, dtype=F)
    y = np.zeros((len(scores), dim), dtype=F)
    with np.errstate(all="ignore"):
        y[:, 0] = F(2.0) * scores
    return np.zeros((1, dim), dtype=F), y


def sorted_scores(scores):
    """What quantiles() orders: the non-NaN scores ascending, zeros as +0.0; and the NaN count."""
    scores = np.asarray(scores, dtype=F)
    kept = scores[~np.isnan(scores)]
    return np.sort(np.where(kept == 0, F(0.0), kept)), len(scores) - len(kept)
