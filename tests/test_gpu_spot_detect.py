"""GPU tests of spot detection (apd_spot_detect) against the checker tests/_spot_detect_reference.py and against the route it
replaces, apd_spot with curves followed by apd_spot_hits.

Every comparison is bitwise: pair, end, start and rank equal, cost and score equal as uint32.  Shapes are the smallest that reach
each path of csrc/dtw_spot_detect.hip and of the host's planner: streams around one wavefront and one marking block (63 / 64 / 65,
200, 1000), groups with fewer candidates than one pass of the picking workgroup, exactly one pass (1024), one more (1025) and
several, groups whose pairs lie apart in the list, lists cut into chunks of whole groups, a group that alone exceeds the cap."""
import ctypes as C
import os

import numpy as np
import pytest

import _spot_detect_reference as det
import _spot_reference as ref

pytestmark = pytest.mark.gpu
UNIT = (1.0, 1.0, 1.0)
SKEWED = (1.0, 2.0, 0.5)                        # (insertion, deletion, match)
F = np.float32
INF = F(np.inf)
CANARY = 0x55555555


@pytest.fixture(scope="module")
def ctx(apd):
    c = apd.Context(0)
    yield c
    c.close()


def make_batch(ctx, seqs):
    from audio_pattern_discovery_amd.alignments import Batch
    seqs = [np.ascontiguousarray(s, dtype=F) for s in seqs]
    offsets = np.zeros(len(seqs) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(s) for s in seqs])
    return Batch(ctx, np.concatenate(seqs, axis=0), offsets, seqs[0].shape[1])


def config(apd, pen):
    return apd.AlignConfig(float("nan"), pen[0], pen[1], pen[2])                 # the band percentage is not read


def bound(seqs, pairs, per_stream):
    """The capacity that always suffices: frames of the stream of every group."""
    streams = list(dict.fromkeys(int(y) for _, y in pairs)) if per_stream else [int(y) for _, y in pairs]
    return sum(len(seqs[y]) for y in streams)


def raw_detect(apd, ctx, batch, pen, pairs, thresholds, per_stream, capacity, counts_only=False):
    """apd_spot_detect through ctypes: (hits written, hit_off, n_hits).  One record more than `capacity` is allocated and must stay
    untouched, and so must the hit_off slots behind the groups."""
    L = apd.lib()
    cfg = config(apd, pen)
    pr = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
    n_pairs = len(pr)
    thr = np.ascontiguousarray(np.broadcast_to(np.asarray(thresholds, dtype=F), (n_pairs,)))
    hits = np.full((capacity + 1) * 6, CANARY, dtype=np.uint32).view(det.HIT)
    off = np.full(n_pairs + 2, 77, dtype=np.uint64)
    n_groups, n_hits = C.c_uint64(99), C.c_uint64(99)
    apd.check(L.apd_spot_detect(ctx.handle, batch.handle, C.byref(cfg), pr.ctypes.data_as(C.POINTER(C.c_uint32)), n_pairs,
                                thr.ctypes.data_as(C.POINTER(C.c_float)), int(per_stream),
                                None if counts_only else hits.ctypes.data_as(C.POINTER(apd.SpotHit)), 0 if counts_only else capacity,
                                off.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(n_groups), C.byref(n_hits)), ctx.handle)
    ng = int(n_groups.value)
    assert ng <= n_pairs and np.all(off[ng + 1:] == 77) and int(off[ng]) == int(n_hits.value) and off[0] == 0
    written = 0 if counts_only else min(int(n_hits.value), capacity)
    assert np.all(hits[written:].view(np.uint32) == CANARY)                      # nothing past the hits, nothing past the capacity
    return hits[:written].copy(), off[:ng + 1].copy(), int(n_hits.value)


def raw_curves(apd, ctx, batch, pen, pairs):
    """apd_spot with curves through ctypes: (list of (cost, start), best)."""
    L = apd.lib()
    cfg = config(apd, pen)
    pr = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
    n_pairs = len(pr)
    u32p, u64p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_float)
    head = (ctx.handle, batch.handle, C.byref(cfg), pr.ctypes.data_as(u32p), n_pairs)
    off = np.zeros(n_pairs + 1, dtype=np.uint64)
    best = np.zeros(n_pairs, dtype=ref.BEST)
    apd.check(L.apd_spot(*head, None, None, 0, off.ctypes.data_as(u64p), None), ctx.handle)
    cost, start = np.zeros(int(off[-1]), dtype=F), np.zeros(int(off[-1]), dtype=np.uint32)
    apd.check(L.apd_spot(*head, cost.ctypes.data_as(f32p), start.ctypes.data_as(u32p), len(cost), off.ctypes.data_as(u64p),
                         best.ctypes.data_as(C.POINTER(apd.SpotBest))), ctx.handle)
    return [(cost[int(off[p]):int(off[p + 1])].copy(), start[int(off[p]):int(off[p + 1])].copy()) for p in range(n_pairs)], best


def check_case(apd, ctx, seqs, pairs, thresholds, per_stream, pen=UNIT, batch=None, cache=None):
    """One call at the bound, compared with the checker; returns the checker's (hits, hit_off, labels, stats)."""
    own = batch is None
    batch = batch or make_batch(ctx, seqs)
    try:
        got, off, n_hits = raw_detect(apd, ctx, batch, pen, pairs, thresholds, per_stream, bound(seqs, pairs, per_stream))
    finally:
        if own:
            batch.close()
    want = det.detect(seqs, pairs, thresholds, per_stream, pen, cache)
    assert np.array_equal(off, want[1]) and n_hits == len(want[0]), (off, want[1])
    assert det.same_hits(got, want[0]), (got, want[0])
    return want


def gauss_seqs(lengths, dim, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((n, dim)).astype(F) for n in lengths]


def integer_seqs(lengths, dim, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 3, (n, dim)).astype(F) for n in lengths]


def col(values):
    return np.array(values, dtype=F).reshape(-1, 1)


def test_hand_worked_example_through_both_entry_points(apd, ctx):
    """The example tests/test_spot_detect_reference.py works out on paper, through the C ABI and through AlignmentWorkers.detect."""
    from audio_pattern_discovery_amd.alignments import SPOT_HIT, AlignmentWorkers, NDSequence
    from audio_pattern_discovery_amd.discovery import Discovery
    y, a, b = col([5, 1, 2, 5, 1, 3, 5, 2, 4, 3]), col([1, 2]), col([2, 4, 1])
    seqs, pairs, thr = [a, b, a.copy(), y], [(0, 3), (1, 3), (2, 3)], [0.3, 0.4, 0.3]
    want = check_case(apd, ctx, seqs, pairs, thr, True)
    assert [(int(h["pair"]), int(h["end"]), int(h["start"])) for h in want[0]] == [(0, 3, 2), (0, 6, 5), (1, 10, 8)]
    alone = check_case(apd, ctx, seqs, pairs, thr, False)
    workers = AlignmentWorkers.new([NDSequence(s) for s in seqs], ctx)
    try:
        hits, off, groups = workers.detect(pairs, Discovery(), thr, per_stream=True)
        assert hits.dtype == SPOT_HIT and det.same_hits(hits, want[0]) and off.tolist() == [0, 3] and groups.tolist() == [3]
        hits, off, groups = workers.detect(pairs, Discovery(), thr)
        assert det.same_hits(hits, alone[0]) and off.tolist() == [0, 2, 4, 6] and groups.tolist() == [0, 1, 2]
        hits, off, groups = workers.detect(pairs, Discovery(), 0.3, per_stream=True, capacity=2)       # a scalar threshold, a short buffer
        assert off.tolist() == [0, 2] and det.same_hits(hits, want[0][:2])
    finally:
        workers.close()


QUERY_LENGTHS = (1, 2, 5, 64, 65, 130)
STREAM_LENGTHS = (1, 63, 64, 65, 200, 1000)


@pytest.fixture(scope="module")
def edges(apd, ctx):
    """Every query length against every stream length, and the existing route's results on them, computed once."""
    seqs = gauss_seqs(QUERY_LENGTHS + STREAM_LENGTHS, 13, 301)
    nq = len(QUERY_LENGTHS)
    pairs = [(q, nq + s) for q in range(nq) for s in range(len(STREAM_LENGTHS))]
    batch = make_batch(ctx, seqs)
    route = {pen: raw_curves(apd, ctx, batch, pen, pairs) for pen in (UNIT, SKEWED)}
    yield seqs, pairs, batch, route
    batch.close()


@pytest.mark.parametrize("pen", [UNIT, SKEWED])
def test_per_pair_equals_spot_followed_by_spot_hits(apd, ctx, edges, pen):
    """Through the library itself: apd_spot's curves, apd_spot_hits on each pair with the pair's own threshold (its median score)."""
    from audio_pattern_discovery_amd.alignments import spot_hits
    seqs, pairs, batch, route = edges
    curves, _ = route[pen]
    lengths = [len(seqs[x]) for x, _ in pairs]
    thr = np.array([det.median_threshold([c], [n]) for c, n in zip(curves, lengths)], dtype=F)
    assert len(set(thr.tolist())) > len(pairs) // 2
    got, off, n_hits = raw_detect(apd, ctx, batch, pen, pairs, thr, False, bound(seqs, pairs, False))
    assert len(off) == len(pairs) + 1 and n_hits >= len(pairs)
    for p, (cost, start) in enumerate(curves):
        host = spot_hits(cost, start, lengths[p], thr[p])
        mine = got[int(off[p]):int(off[p + 1])]
        assert len(mine) == len(host), (p, pairs[p])
        assert np.all(mine["pair"] == p) and mine["rank"].tolist() == list(range(len(mine)))
        assert ref.same_best(mine[["end", "start", "cost", "score"]].astype(ref.BEST), host), (p, pairs[p])
    want = det.detect_curves(curves, lengths, pairs, thr, False)                 # and the checker on the same curves
    assert np.array_equal(off, want[1]) and det.same_hits(got, want[0])


def test_infinite_threshold_starts_with_the_best_window(apd, ctx, edges):
    seqs, pairs, batch, route = edges
    curves, best = route[UNIT]
    got, off, _ = raw_detect(apd, ctx, batch, UNIT, pairs, INF, False, bound(seqs, pairs, False))
    for p in range(len(pairs)):
        assert int(off[p + 1]) > int(off[p])
        first = got[int(off[p]):int(off[p]) + 1]
        assert first["rank"][0] == 0 and first["pair"][0] == p
        assert ref.same_best(first[["end", "start", "cost", "score"]].astype(ref.BEST), best[p])
    want = det.detect_curves(curves, [len(seqs[x]) for x, _ in pairs], pairs, INF, False)
    assert np.array_equal(off, want[1]) and det.same_hits(got, want[0])
    # a query with a NaN frame: every column of its curve is +INF or NaN, apd_spot keeps nothing, and neither does the detection
    poisoned = gauss_seqs((4, 50, 3), 13, 302)
    poisoned[0][2, :] = np.nan
    b = make_batch(ctx, poisoned)
    try:
        curves, best = raw_curves(apd, ctx, b, UNIT, [(0, 1), (2, 1)])
        assert not np.any(np.isfinite(curves[0][0])) and np.any(np.isnan(curves[0][0])) and int(best[0]["end"]) == 0
        got, off, n_hits = raw_detect(apd, ctx, b, UNIT, [(0, 1), (2, 1)], INF, False, 100)
        assert int(off[1]) == 0 and n_hits == int(off[2]) >= 1 and np.all(got["pair"] == 1)
        got, off, _ = raw_detect(apd, ctx, b, UNIT, [(0, 1), (2, 1)], INF, True, 50)
        assert len(off) == 2 and np.all(got["pair"] == 1)
    finally:
        b.close()


def test_per_stream_seeded_cases(apd, ctx):
    """The 40 cases tests/test_spot_detect_reference.py proves non-vacuous, one call each."""
    cases = det.seeded_cases()
    assert len(cases) == 40
    for seqs, pairs, thr, curves in cases:
        batch = make_batch(ctx, seqs)
        try:
            got, off, n_hits = raw_detect(apd, ctx, batch, UNIT, pairs, thr, True, len(seqs[3]))
        finally:
            batch.close()
        want = det.detect_curves(curves, [len(seqs[x]) for x, _ in pairs], pairs, thr, True)
        assert np.array_equal(off, want[1]) and n_hits == len(want[0]) and det.same_hits(got, want[0])


@pytest.fixture(scope="module")
def interleaved():
    """Templates of different lengths cut from three streams, the pairs of the streams interleaved, one pair repeated, every pair
    with a threshold of its own.  Shared by the per-stream, chunking, capacity and refill tests with one cache of checker curves."""
    rng = np.random.default_rng(310)
    streams = [rng.integers(0, 3, (m, 2)).astype(F) for m in (90, 150, 61)]
    templates = [streams[0][10:13].copy(), streams[1][40:47].copy(), streams[2][5:7].copy(), streams[1][100:105].copy(), streams[0][10:13].copy()]
    seqs = templates + streams                                                   # streams are 5, 6, 7
    pairs = [(0, 6), (1, 5), (2, 7), (3, 6), (0, 5), (1, 6), (4, 5), (0, 6), (2, 5), (3, 7), (4, 6), (1, 7), (2, 6)]
    cache = {}
    curves = [cache.setdefault((x, y, UNIT), ref.curves(seqs[x], seqs[y])) for x, y in pairs]
    base = det.median_threshold(curves, [len(seqs[x]) for x, _ in pairs])
    thr = np.array([base * F(0.6 + 0.1 * (p % 5)) for p in range(len(pairs))], dtype=F)
    thr[7] = thr[0]                                                              # the repeated pair (0, 6), with the threshold of the first
    return seqs, pairs, thr, cache


def test_per_stream_interleaved_pairs_repeats_and_own_thresholds(apd, ctx, interleaved):
    seqs, pairs, thr, cache = interleaved
    hits, off, labels, stats = check_case(apd, ctx, seqs, pairs, thr, True, cache=cache)
    assert labels == [6, 5, 7] and len(off) == 4
    assert all(s["hits"] >= 2 and s["rejected"] >= 1 for s in stats) and stats[0]["ties"] >= 1 and stats[0]["pairs_hit"] >= 2
    assert 7 not in hits["pair"]                                                 # the repeated pair (0, 6) loses every tie to pair 0
    check_case(apd, ctx, seqs, pairs, thr, False, cache=cache)
    check_case(apd, ctx, seqs, pairs, thr, True, pen=SKEWED, cache=cache)


def test_thresholds(apd, ctx, interleaved):
    seqs, pairs, _, cache = interleaved
    batch = make_batch(ctx, seqs)
    try:
        for per_stream in (False, True):
            groups = 3 if per_stream else len(pairs)
            for none in (np.nan, -1.0, 0.0):                                     # 0: the templates occur exactly, score 0, and 0 < 0 is false
                got, off, n_hits = raw_detect(apd, ctx, batch, UNIT, pairs, none, per_stream, 8)
                assert len(got) == 0 and n_hits == 0 and off.tolist() == [0] * (groups + 1)
            hits, _, _, stats = check_case(apd, ctx, seqs, pairs, INF, per_stream, batch=batch, cache=cache)
            assert sum(s["candidates"] for s in stats) == sum(len(seqs[y]) for _, y in pairs)      # every column is finite here
            for g in set(hits["pair"].tolist()) if not per_stream else ():
                spans = sorted((int(h["start"]), int(h["end"])) for h in hits[hits["pair"] == g])
                assert all(a[1] < b[0] for a, b in zip(spans[:-1], spans[1:]))
        mixed = np.where(np.arange(len(pairs)) % 2 == 0, INF, F(np.nan)).astype(F)                # a NaN threshold silences its pair only
        hits, _, _, _ = check_case(apd, ctx, seqs, pairs, mixed, True, batch=batch, cache=cache)
        assert len(hits) and np.all(hits["pair"] % 2 == 0)
    finally:
        batch.close()
    assert np.any(ref.curves(seqs[0], seqs[5])[0] == 0.0)


def test_keys_cover_negative_scores_nan_columns_and_infinite_penalties(apd, ctx):
    rng = np.random.default_rng(320)
    stream = rng.integers(0, 3, (120, 2)).astype(F)
    other = rng.integers(0, 3, (70, 2)).astype(F)
    other[30, :] = np.nan                                                        # column 31 is NaN in every row: never a hit
    seqs = [stream[20:24].copy(), stream[60:62].copy(), stream[20:24].copy(), stream, other]
    pairs = [(0, 3), (1, 4), (1, 3), (2, 3), (0, 4), (2, 4)]
    cache = {}
    # match = -1: costs and scores go negative, and the most negative score is the first hit
    negative = (1.0, 1.0, -1.0)
    hits, off, _, stats = check_case(apd, ctx, seqs, pairs, -0.05, True, pen=negative, cache=cache)
    assert np.all(hits["score"] < 0) and stats[0]["hits"] >= 2 and stats[0]["rejected"] >= 1
    for g in range(2):
        scores = hits["score"][int(off[g]):int(off[g + 1])]
        assert len(scores) >= 2 and np.all(np.diff(scores) >= 0) and scores[0] < scores[-1]
    check_case(apd, ctx, seqs, pairs, INF, False, pen=negative, cache=cache)     # negative and positive scores in one list
    # the NaN frame
    hits, off, labels, _ = check_case(apd, ctx, seqs, pairs, INF, True, cache=cache)
    assert labels == [3, 4]
    on_other = hits[int(off[1]):]
    assert len(on_other) >= 2 and 31 not in on_other["end"] and np.all(np.isfinite(on_other["score"]))
    assert all(np.isnan(cache[(x, 4, UNIT)][0][30]) for x in (0, 1, 2))          # the NaN frame's own column, in every curve on it
    # an infinite penalty: INF * d is NaN where d = 0 and INF elsewhere
    for pen in ((np.inf, 1.0, 1.0), (1.0, 1.0, np.inf), (1.0, np.inf, 1.0)):
        check_case(apd, ctx, seqs, pairs, INF, True, pen=pen, cache=cache)
        check_case(apd, ctx, seqs, pairs, 0.5, False, pen=pen, cache=cache)


def test_groups_around_one_pass_of_the_picking_workgroup(apd, ctx):
    """The picking workgroup scans 1024 candidates per pass: one pass exactly, one candidate more, and several passes with four
    templates competing.  With threshold +INF every finite column is a candidate, so the counts are the streams' lengths."""
    rng = np.random.default_rng(330)
    streams = [rng.integers(0, 3, (m, 1)).astype(F) for m in (1024, 1025, 700)]
    templates = [streams[2][100:103].copy(), streams[2][300:306].copy(), streams[2][500:502].copy(), streams[2][100:103].copy()]
    seqs = templates + streams                                                   # streams are 4, 5, 6
    pairs = [(2, 4), (2, 5)] + [(t, 6) for t in range(4)]
    hits, off, _, stats = check_case(apd, ctx, seqs, pairs, INF, True)
    assert [s["candidates"] for s in stats] == [1024, 1025, 2800]
    assert stats[2]["hits"] >= 64 and stats[2]["ties"] >= 1 and stats[2]["pairs_hit"] >= 3


def test_chunked_equals_unchunked(apd, ctx, interleaved):
    """Chunks hold whole groups: caps that cut the three groups 2 + 1 and 1 + 2, and a cap every group alone exceeds (1 + 1 + 1)."""
    seqs, pairs, thr, cache = interleaved
    batch = make_batch(ctx, seqs)
    cap_all = bound(seqs, pairs, True)
    per_group = {}
    for _, y in pairs:
        per_group[y] = per_group.get(y, 0) + 24 * len(seqs[y])
    per_group = {y: b + 8 * len(seqs[y]) for y, b in per_group.items()}          # 24 bytes per entry, 8 per stream column (include/apd.h)
    try:
        whole = raw_detect(apd, ctx, batch, UNIT, pairs, thr, True, cap_all)
        whole_pairs = raw_detect(apd, ctx, batch, UNIT, pairs, thr, False, bound(seqs, pairs, False))
        try:
            for cap in (per_group[6] + per_group[5], max(per_group.values()), 1):
                os.environ["APD_SPOT_WORKSPACE_BYTES"] = str(cap)
                for per_stream, want in ((True, whole), (False, whole_pairs)):
                    got = raw_detect(apd, ctx, batch, UNIT, pairs, thr, per_stream, bound(seqs, pairs, per_stream))
                    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1], want[1]) and got[2] == want[2]
        finally:
            del os.environ["APD_SPOT_WORKSPACE_BYTES"]
    finally:
        batch.close()
    assert det.same_hits(whole[0], det.detect(seqs, pairs, thr, True, UNIT, cache)[0])
    assert per_group[6] + per_group[5] < sum(per_group.values()) and min(per_group.values()) > 1


def test_capacity_below_the_total_and_counts_only(apd, ctx, interleaved):
    seqs, pairs, thr, cache = interleaved
    want_hits, want_off, _, _ = det.detect(seqs, pairs, thr, True, UNIT, cache)
    total = len(want_hits)
    assert total >= 6 and int(want_off[1]) >= 2
    batch = make_batch(ctx, seqs)
    try:
        for capacity in (1, int(want_off[1]) - 1, int(want_off[1]) + 1, total - 1, total):      # inside the first group, across a group edge
            got, off, n_hits = raw_detect(apd, ctx, batch, UNIT, pairs, thr, True, capacity)      # (the canary behind `capacity` is checked there)
            assert n_hits == total and np.array_equal(off, want_off) and det.same_hits(got, want_hits[:capacity])
        got, off, n_hits = raw_detect(apd, ctx, batch, UNIT, pairs, thr, True, 0, counts_only=True)
        assert len(got) == 0 and n_hits == total and np.array_equal(off, want_off)
        os.environ["APD_SPOT_WORKSPACE_BYTES"] = "1"                             # the capacity ends inside the second chunk
        try:
            got, off, n_hits = raw_detect(apd, ctx, batch, UNIT, pairs, thr, True, int(want_off[1]) + 1)
        finally:
            del os.environ["APD_SPOT_WORKSPACE_BYTES"]
        assert n_hits == total and np.array_equal(off, want_off) and det.same_hits(got, want_hits[:int(want_off[1]) + 1])
    finally:
        batch.close()


def test_detect_follows_a_refill_and_runs_on_a_joined_batch(apd, ctx, interleaved):
    from audio_pattern_discovery_amd.alignments import AlignmentWorkers, NDSequence
    from audio_pattern_discovery_amd.discovery import Discovery
    seqs, pairs, thr, cache = interleaved
    fresh = integer_seqs([len(s) for s in seqs], 2, 340)
    batch = make_batch(ctx, seqs)
    try:
        before = check_case(apd, ctx, seqs, pairs, thr, True, batch=batch, cache=cache)
        frames = np.ascontiguousarray(np.concatenate(fresh, axis=0))
        apd.check(apd.lib().apd_batch_refill(ctx.handle, batch.handle, C.c_void_p(frames.ctypes.data), 0), ctx.handle)
        after = check_case(apd, ctx, fresh, pairs, INF, True, batch=batch)
    finally:
        batch.close()
    assert not det.same_hits(before[0], after[0])
    templates, streams = seqs[:5], seqs[5:]
    wa, wb = AlignmentWorkers.new([NDSequence(s) for s in templates], ctx), AlignmentWorkers.new([NDSequence(s) for s in streams], ctx)
    try:
        hits, off, groups = wa.detect(pairs, Discovery(), thr, per_stream=True, streams=wb)
        alone = wa.detect(pairs, Discovery(), thr, streams=wb)
        empty = wa.detect(np.zeros((0, 2), np.uint32), Discovery(), 1.0, per_stream=True, streams=wb)
    finally:
        wa.close()
        wb.close()
    assert det.same_hits(hits, before[0]) and np.array_equal(off, before[1]) and groups.tolist() == [6, 5, 7]
    want = det.detect(seqs, pairs, thr, False, UNIT, cache)
    assert det.same_hits(alone[0], want[0]) and np.array_equal(alone[1], want[1]) and alone[2].tolist() == list(range(len(pairs)))
    assert len(empty[0]) == 0 and empty[1].tolist() == [0] and len(empty[2]) == 0


def test_argument_errors_launch_nothing(apd, ctx):
    L = apd.lib()
    seqs = gauss_seqs((12, 40, 25), 13, 350)
    batch = make_batch(ctx, seqs)
    other = apd.Context(0)
    cfg = apd.AlignConfig(1.0, 1.0, 1.0, 1.0)
    u32p, u64p, f32p, hitp = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_float), C.POINTER(apd.SpotHit)
    pairs = np.array([(0, 1), (2, 2), (0, 2)], dtype=np.uint32)
    thr = np.full(3, np.inf, dtype=F)
    hits = np.full(100 * 6, CANARY, dtype=np.uint32).view(det.HIT)
    off = np.full(5, 77, dtype=np.uint64)
    ng, nh = C.c_uint64(99), C.c_uint64(99)
    prp, thrp, hp, offp = pairs.ctypes.data_as(u32p), thr.ctypes.data_as(f32p), hits.ctypes.data_as(hitp), off.ctypes.data_as(u64p)

    def call(ctx_=None, batch_=None, pairs_=prp, n=3, thr_=thrp, compete=0, hits_=hp, capacity=100, off_=offp, ng_=C.byref(ng), nh_=C.byref(nh)):
        return L.apd_spot_detect((ctx_ or ctx).handle, (batch_ or batch).handle, C.byref(cfg), pairs_, n, thr_, compete, hits_, capacity, off_, ng_, nh_)

    def untouched():
        return not ctx.stream_busy() and np.all(hits.view(np.uint32) == CANARY)

    try:
        ctx.synchronize()
        for bad in (dict(compete=2), dict(compete=-1), dict(thr_=None), dict(off_=None), dict(ng_=None), dict(nh_=None), dict(hits_=None),
                    dict(pairs_=None), dict(ctx_=other)):
            assert call(**bad) == apd.APD_ERR_INVALID_ARG and untouched(), bad
        wrong = np.array([(0, 1), (3, 0)], dtype=np.uint32)                                                       # index = n_seq
        assert call(pairs_=wrong.ctypes.data_as(u32p), n=2) == apd.APD_ERR_INVALID_ARG and untouched()
        assert off.tolist() == [77] * 5 and (ng.value, nh.value) == (99, 99)                                      # nor the outputs
        assert call(pairs_=None, n=0, thr_=None, hits_=None, capacity=0) == apd.APD_OK                            # an empty list
        assert (ng.value, nh.value, int(off[0]), int(off[1])) == (0, 0, 0, 77) and untouched()
        assert call(hits_=None, capacity=0) == apd.APD_OK and ng.value == 3 and nh.value == int(off[3]) >= 3 and untouched()   # counts only
        assert call() == apd.APD_OK and np.all(hits[nh.value:].view(np.uint32) == CANARY) and np.all(hits["rank"][:nh.value] < 40)
    finally:
        batch.close()
        other.close()
    # an empty sequence in the batch, a query beyond the documented limit: apd_spot's codes, before anything is launched
    from audio_pattern_discovery_amd.alignments import Batch
    frames = np.zeros((16385 + 5, 1), dtype=F)
    empty = Batch(ctx, frames[:9], np.array([0, 4, 4, 9], dtype=np.uint64), 1)
    long_ = Batch(ctx, frames, np.array([0, 16385, 16390], dtype=np.uint64), 1)
    one = np.array([(0, 2)], dtype=np.uint32)
    hits[:] = np.full(6, CANARY, dtype=np.uint32).view(det.HIT)[0]
    try:
        ctx.synchronize()
        assert call(batch_=empty, pairs_=one.ctypes.data_as(u32p), n=1) == apd.APD_ERR_EMPTY_SEQUENCE and untouched()
        one[0] = (0, 1)
        assert call(batch_=long_, pairs_=one.ctypes.data_as(u32p), n=1) == apd.APD_ERR_UNSUPPORTED and untouched()
        one[0] = (1, 0)                                                                                           # the other way round runs
        thr[0] = 1.0
        assert call(batch_=long_, pairs_=one.ctypes.data_as(u32p), n=1, compete=1) == apd.APD_OK and ng.value == 1 and nh.value >= 1
        assert (int(hits[0]["pair"]), int(hits[0]["end"]), int(hits[0]["rank"]), float(hits[0]["score"])) == (0, 1, 0, 0.0)   # all-zero frames
    finally:
        empty.close()
        long_.close()


def test_timing_covers_the_sweep_and_the_detection(apd, ctx, edges):
    seqs, pairs, batch, _ = edges
    L = apd.lib()
    cfg = config(apd, UNIT)
    pr = np.ascontiguousarray(pairs, dtype=np.uint32)
    off = np.zeros(len(pairs) + 1, dtype=np.uint64)
    best = np.zeros(len(pairs), dtype=ref.BEST)

    def best_only():
        apd.check(L.apd_spot(ctx.handle, batch.handle, C.byref(cfg), pr.ctypes.data_as(C.POINTER(C.c_uint32)), len(pairs), None, None, 0,
                             off.ctypes.data_as(C.POINTER(C.c_uint64)), best.ctypes.data_as(C.POINTER(apd.SpotBest))), ctx.handle)
        return ctx.last_kernel_ms()

    ctx.set_timing(True)
    try:
        best_only()                                                              # both routes once before either is timed
        raw_detect(apd, ctx, batch, UNIT, pairs, INF, True, bound(seqs, pairs, True))
        sweep_ms = min(best_only() for _ in range(3))
        raw_detect(apd, ctx, batch, UNIT, pairs, INF, True, bound(seqs, pairs, True))
        detect_ms = ctx.last_kernel_ms()
    finally:
        ctx.set_timing(False)
    assert sweep_ms > 0.0 and detect_ms >= sweep_ms, (sweep_ms, detect_ms)
