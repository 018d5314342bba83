"""GPU tests of spot score quantiles (apd_spot_quantiles) against the checker tests/_spot_quantile_reference.py.

Every value is compared by its bits, and so are the statuses, groups, entry and NaN counts.  Shapes are the smallest that reach each
path of csrc/dtw_spot_quantile.hip and of the host's planner: streams around one wavefront (63 / 64 / 65) and around one step of a
pass workgroup (columns - 1, columns, columns + 1, 2 columns + 3), groups of one pair, of a query's pairs lying apart in the list
and of the whole list, one quantile and eight, multisets that make all four digit passes decide, ranks on and beyond the last
non-NaN score, lists cut into chunks of whole groups, a group that alone exceeds the cap, and one group of more than 2^24 entries,
where the f32 index is no longer the integer one."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _spot_detect_reference as det
import _spot_quantile_reference as qref
import _spot_reference as ref
from _path_reference import F, bits

pytestmark = pytest.mark.gpu
UNIT = (1.0, 1.0, 1.0)
INF = F(np.inf)
CANARY = 0x55555555
BY = {"pair": 0, "query": 1, "all": 2}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx(apd):
    c = apd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cases(apd):
    return qref.seeded_cases(columns=apd.APD_SPOT_QUANTILES_COLUMNS)


def make_batch(ctx, seqs):
    from audio_pattern_discovery_amd.alignments import Batch
    seqs = [np.ascontiguousarray(s, dtype=F) for s in seqs]
    offsets = np.zeros(len(seqs) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(s) for s in seqs])
    return Batch(ctx, np.concatenate(seqs, axis=0), offsets, seqs[0].shape[1])


def config(apd, pen):
    return apd.AlignConfig(float("nan"), pen[0], pen[1], pen[2])                 # the band percentage is not read


def raw_quantiles(apd, ctx, batch, pen, pairs, by, perc):
    """apd_spot_quantiles through ctypes: (values, status, group_of, entries, nans), cut to the groups.  One slot more than the
    contract's bound is allocated everywhere and must stay untouched, and so must the slots behind the groups."""
    cfg = config(apd, pen)
    pr = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
    n_pairs = len(pr)
    pc = np.ascontiguousarray(np.atleast_1d(np.asarray(perc, dtype=F)))
    nq = len(pc)
    values = np.full((n_pairs + 1) * nq, CANARY, dtype=np.uint32)
    status = np.full((n_pairs + 1) * nq, CANARY, dtype=np.uint32)
    group_of, entries, nans = (np.full(n_pairs + 1, 77, dtype=np.uint64) for _ in range(3))
    n_groups = C.c_uint64(99)
    u32p, u64p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_float)
    apd.check(apd.lib().apd_spot_quantiles(ctx.handle, batch.handle, C.byref(cfg), pr.ctypes.data_as(u32p), n_pairs, BY[by],
                                           pc.ctypes.data_as(f32p), nq, values.ctypes.data_as(f32p), status.ctypes.data_as(C.POINTER(C.c_int32)),
                                           group_of.ctypes.data_as(u64p), entries.ctypes.data_as(u64p), nans.ctypes.data_as(u64p),
                                           C.byref(n_groups)), ctx.handle)
    ng = int(n_groups.value)
    assert ng <= n_pairs and np.all(values[ng * nq:] == CANARY) and np.all(status[ng * nq:] == CANARY)
    assert group_of[n_pairs] == 77 and np.all(entries[ng:] == 77) and np.all(nans[ng:] == 77)
    return (values[:ng * nq].view(F).reshape(ng, nq).copy(), status[:ng * nq].view(np.int32).reshape(ng, nq).copy(), group_of[:n_pairs].copy(),
            entries[:ng].copy(), nans[:ng].copy())


def same(got, want):
    """Two results of raw_quantiles / the first five of qref.quantiles equal, values by their bits."""
    return (got[0].shape == want[0].shape and np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1])
            and all(np.array_equal(a, b) for a, b in zip(got[2:5], want[2:5])))


def expect(multisets, by, perc):
    """The checker's arithmetic on dictated score multisets, one per pair, every pair a query of its own (by="query" == by="pair")."""
    perc = np.atleast_1d(np.asarray(perc, dtype=F))
    pops = [np.concatenate(multisets)] if by == "all" else multisets
    values = np.zeros((len(pops), len(perc)), dtype=F)
    status = np.zeros((len(pops), len(perc)), dtype=np.int32)
    nans = []
    for g, pop in enumerate(pops):
        kept, n_nan = qref.sorted_scores(pop)
        nans.append(n_nan)
        for q, p in enumerate(perc):
            k = qref.percentile_index(len(pop), p)
            if k >= len(kept):
                values[g, q], status[g, q] = np.array([qref.NAN_BITS], dtype=np.uint32).view(F)[0], qref.ERR_INDEX
            else:
                values[g, q] = kept[k]
    group = np.zeros(len(multisets), dtype=np.uint64) if by == "all" else np.arange(len(multisets), dtype=np.uint64)
    return values, status, group, np.array([len(p) for p in pops], dtype=np.uint64), np.array(nans, dtype=np.uint64)


def test_the_header_and_the_binding_name_the_same_columns(apd):
    text = open(os.path.join(ROOT, "include", "apd.h")).read()
    assert int(re.search(r"#define APD_SPOT_QUANTILES_COLUMNS\s+(\d+)", text).group(1)) == apd.APD_SPOT_QUANTILES_COLUMNS
    assert int(re.search(r"#define APD_SPOT_QUANTILES_MAX\s+(\d+)", text).group(1)) == apd.APD_SPOT_QUANTILES_MAX == 8


def test_seeded_cases_against_the_checker(apd, ctx, cases):
    batches = {}
    try:
        for c in cases:
            if id(c["seqs"]) not in batches:
                batches[id(c["seqs"])] = make_batch(ctx, c["seqs"])
            got = raw_quantiles(apd, ctx, batches[id(c["seqs"])], c["pen"], c["pairs"], c["by"], c["perc"])
            want = qref.quantiles(c["curves"], c["lengths"], c["pairs"], c["by"], c["perc"])
            assert same(got, want), (c["by"], c["perc"], got, want[:5])
    finally:
        for b in batches.values():
            b.close()


def dictated_batch(ctx, multisets):
    """One one-frame query and one stream per multiset: sequences 2 i and 2 i + 1; the pairs."""
    seqs = []
    for s in multisets:
        seqs.extend(qref.dictated(s))
    return make_batch(ctx, seqs), [(2 * i, 2 * i + 1) for i in range(len(multisets))]


def test_dictated_multisets(apd, ctx):
    """Scores dictated through one-frame queries (tests/test_spot_quantile_reference.py checks the construction on the CPU): what the
    select must return follows from the multiset alone."""
    rng = np.random.default_rng(410)
    near = (np.uint32(0x3F5A3C00) + rng.permutation(256).astype(np.uint32)).view(F)       # the top 24 key bits agree: pass 3 decides
    equal = np.full(300, 0.7, dtype=F)
    wide = np.array([2.0 ** e for e in range(-40, 41, 3)] + [1.5 * 2.0 ** e for e in range(-39, 40, 5)] + [0.0, 0.0], dtype=F)
    rng.shuffle(wide)
    holes = rng.random(130).astype(F)
    holes[[3, 64, 65, 129]] = np.nan
    holes[[0, 63, 100]] = np.inf
    all_nan = np.full(5, np.nan, dtype=F)
    multisets = [near, equal, wide, holes, all_nan]
    batch, pairs = dictated_batch(ctx, multisets)
    live = len(holes) - 4
    try:
        for perc in ([0.0, -1.0, np.nan, 1.0, qref.perc_for_rank(len(holes), live - 1), qref.perc_for_rank(len(holes), live), 0.5, 0.25],
                     np.linspace(0.0, 0.999, 8), [0.37]):
            for by in qref.BYS:
                got = raw_quantiles(apd, ctx, batch, UNIT, pairs, by, perc)
                assert same(got, expect(multisets, by, perc)), (by, perc, got)
        got = raw_quantiles(apd, ctx, batch, UNIT, pairs, "pair", [qref.perc_for_rank(len(holes), live - 1), qref.perc_for_rank(len(holes), live)])
        assert got[1][3].tolist() == [qref.OK, qref.ERR_INDEX] and got[0][3, 0] == INF and got[4][3] == 4      # the last rank, the next one up
        assert got[1][4].tolist() == [qref.ERR_INDEX] * 2 and got[4][4] == 5                                     # nothing but NaN
        every = raw_quantiles(apd, ctx, batch, UNIT, pairs[:1], "pair", np.arange(8) / 256.0 * 32)               # 8 of the 256 neighbours
        assert np.array_equal(bits(every[0][0]), np.uint32(0x3F5A3C00) + np.arange(8, dtype=np.uint32) * 32)
    finally:
        batch.close()


@pytest.fixture(scope="module")
def big(ctx):
    """2^24 + 3 entries through one-frame queries: 2^20 distinct scores in 256 streams of 4096 frames listed 16 times each, two scores
    below them all and one above in a stream of three, the list shuffled.  (workers, pairs, the distinct scores, the three)."""
    from audio_pattern_discovery_amd.alignments import AlignmentWorkers, NDSequence
    rng = np.random.default_rng(411)
    distinct = (np.uint32(0x38000000) + rng.permutation(1 << 20).astype(np.uint32) * 16).view(F)
    edge = np.array([1e-9, 100.0, 2e-9], dtype=F)
    seqs = [np.zeros((1, 8), dtype=F)] + [qref.dictated(distinct[s * 4096:(s + 1) * 4096])[1] for s in range(256)] + [qref.dictated(edge)[1]]
    pairs = np.array([(0, 1 + s) for s in range(256)] * 16 + [(0, 257)], dtype=np.uint32)
    pairs = pairs[rng.permutation(len(pairs))]
    workers = AlignmentWorkers.new([NDSequence(s) for s in seqs], ctx)
    yield workers, pairs, distinct, edge
    workers.close()


def test_more_than_2_24_entries_take_the_f32_index(apd, ctx, big):
    """entries = 2^24 + 3 under by="all": (f32)entries = 2^24 + 4, so perc 0.5 asks for rank 8 388 610 where the integer formula gives
    8 388 609.  Rank r >= 2 holds distinct score (r - 2) // 16, and the two ranks straddle a boundary.  Expected: numpy on the curves
    AlignmentWorkers.spot returns."""
    from audio_pattern_discovery_amd.discovery import Discovery
    workers, pairs, distinct, edge = big
    entries = (1 << 24) + 3
    k32, k64 = qref.percentile_index(entries, 0.5), entries // 2
    assert (k32, k64) == (8388610, 8388609)
    curves, _ = workers.spot(pairs, Discovery())
    values, group_of, got_entries, nans = workers.score_quantiles(pairs, Discovery(), [0.5, 0.0], by="all")
    scores = np.concatenate([ref.scores(cost, start, 1) for cost, start in curves])
    assert len(scores) == entries
    scores.sort()
    assert scores[k32] != scores[k64] and scores[k32] == np.sort(distinct)[(k32 - 2) // 16]
    assert values.shape == (1, 2) and bits(values[0]).tolist() == [bits(scores[k32:k32 + 1])[0], bits(edge[:1])[0]]
    assert got_entries.tolist() == [entries] and nans.tolist() == [0] and not group_of.any()


def chunks_of(sizes, cap):
    """The greedy cut of the contract: a chunk takes its first group whatever it weighs, then every further one that fits the cap."""
    count, used = 0, None
    for s in sizes:
        if used is None or used + s > cap:
            count, used = count + 1, 0
        used += s
    return count


def test_chunked_equals_unchunked(apd, ctx, cases, capfd):
    """Chunks hold whole groups: a cap every group alone exceeds, caps that hold a few groups; results bit for bit those of one chunk.
    How many chunks were cut is read off APD_DEBUG_PLAN's lines (one "spot quantile select" line per chunk) and held to the greedy
    cut of the sizes include/apd.h states: 8 bytes per entry, 64 per pair, a 257-bin histogram and 32 bytes per (group, quantile)."""
    c = next(c for c in cases if c["seqs"][0].shape[1] == 13 and len(c["perc"]) == 8)
    batch = make_batch(ctx, c["seqs"])

    def run(by):
        capfd.readouterr()
        os.environ["APD_DEBUG_PLAN"] = "1"
        try:
            got = raw_quantiles(apd, ctx, batch, c["pen"], c["pairs"], by, c["perc"])
        finally:
            del os.environ["APD_DEBUG_PLAN"]
        return got, capfd.readouterr().err.count("spot quantile select")

    try:
        whole, sizes = {}, {}
        for by in qref.BYS:
            whole[by], n_chunks = run(by)
            assert n_chunks == 1
            members = np.bincount(whole[by][2].astype(np.int64))
            sizes[by] = [int(e) * 8 + int(k) * 64 + 8 * (257 * 8 + 32) for e, k in zip(whole[by][3], members)]
        assert same(whole["query"], qref.quantiles(c["curves"], c["lengths"], c["pairs"], "query", c["perc"]))
        assert len(sizes["query"]) == 3 and len(sizes["all"]) == 1
        two = sizes["query"][0] + sizes["query"][1]
        seen = {}
        try:
            for cap in (1, two, max(sizes["query"][1] + sizes["query"][2], two) - 1, 60000):
                os.environ["APD_SPOT_WORKSPACE_BYTES"] = str(cap)
                for by in qref.BYS:
                    got, n_chunks = run(by)
                    assert same(got, whole[by]), (cap, by)
                    assert n_chunks == chunks_of(sizes[by], cap), (cap, by, n_chunks)
                    seen[(cap, by)] = n_chunks
        finally:
            del os.environ["APD_SPOT_WORKSPACE_BYTES"]
        assert seen[(1, "query")] == 3 and seen[(1, "pair")] == len(c["pairs"]) and seen[(1, "all")] == 1    # a group above the cap: its own chunk
        assert seen[(two, "query")] == 2 and 1 < seen[(60000, "pair")] < len(c["pairs"])
    finally:
        batch.close()


def test_the_result_does_not_depend_on_the_column_blocks(apd, ctx, cases):
    """One workgroup per pair, and as many as its columns allow: the histograms are integer sums."""
    c = next(c for c in cases if c["seqs"][0].shape[1] == 8 and len(c["perc"]) == 8 and c["by"] == "query")
    batch = make_batch(ctx, c["seqs"])
    try:
        want = raw_quantiles(apd, ctx, batch, c["pen"], c["pairs"], "query", c["perc"])
        try:
            for target in (1, 1 << 20):
                os.environ["APD_SPOT_QUANTILE_WORKGROUPS"] = str(target)
                assert same(raw_quantiles(apd, ctx, batch, c["pen"], c["pairs"], "query", c["perc"]), want), target
        finally:
            del os.environ["APD_SPOT_QUANTILE_WORKGROUPS"]
    finally:
        batch.close()


def test_thresholds_agree_with_detection(apd, ctx, cases):
    """detect() under spot_thresholds() finds what the detection checker finds under the quantile checker's values; the minimum of a
    group (perc = 0) is a threshold under which nothing lies: the comparison is strict."""
    from audio_pattern_discovery_amd.alignments import AlignmentWorkers, NDSequence
    from audio_pattern_discovery_amd.discovery import Discovery
    c = next(c for c in cases if c["seqs"][0].shape[1] == 8 and c["pen"] == UNIT)
    seqs, pairs, curves, lengths = c["seqs"], c["pairs"], c["curves"], c["lengths"]
    workers = AlignmentWorkers.new([NDSequence(s) for s in seqs], ctx)
    try:
        for by, rate in (("pair", 0.05), ("query", 0.01), ("all", 0.002)):
            thr = workers.spot_thresholds(pairs, Discovery(), rate, by=by)
            values, _, group, _, _, _ = qref.quantiles(curves, lengths, pairs, by, [rate])
            want_thr = values[group.astype(np.int64), 0]
            assert thr.dtype == F and np.array_equal(bits(thr), bits(want_thr))
            hits, off, _ = workers.detect(pairs, Discovery(), thr)
            want = det.detect_curves(curves, lengths, pairs, want_thr, False)
            assert det.same_hits(hits, want[0]) and np.array_equal(off, want[1])
            if by == "pair":
                assert len(hits) >= 10
        lowest = workers.spot_thresholds(pairs, Discovery(), 0.0, by="pair")
        assert np.array_equal(bits(lowest), bits(np.array([ref.scores(c_, s_, n).min() for (c_, s_), n in zip(curves, lengths)], dtype=F)))
        assert len(workers.detect(pairs, Discovery(), lowest)[0]) == 0
        per_query = workers.spot_thresholds(pairs, Discovery(), 0.01, by="query", per_query=True)
        values, _, group, _, _, _ = qref.quantiles(curves, lengths, pairs, "query", [0.01])
        assert np.array_equal(bits(per_query), bits(values[:, 0])) and len(per_query) == 3
        with pytest.raises(ValueError):
            workers.spot_thresholds(pairs, Discovery(), 0.01, by="pair", per_query=True)
        # strict: a rank beyond the scores raises; strict=False hands the statuses back
        with pytest.raises(apd.ApdError) as e:
            workers.score_quantiles(pairs, Discovery(), [0.5, 1.0], by="query")
        assert e.value.status == apd.APD_ERR_INDEX
        out = workers.score_quantiles(pairs, Discovery(), [0.5, 1.0], by="query", strict=False)
        assert len(out) == 5 and out[4].tolist() == [[apd.APD_OK, apd.APD_ERR_INDEX]] * 3 and np.all(np.isnan(out[0][:, 1]))
        assert same((out[0], out[4]) + out[1:4], qref.quantiles(curves, lengths, pairs, "query", [0.5, 1.0]))
        scalar = workers.score_quantiles(pairs, Discovery(), 0.5, by="all")
        assert scalar[0].shape == (1, 1) and bits(scalar[0])[0, 0] == bits(qref.quantiles(curves, lengths, pairs, "all", [0.5])[0])[0, 0]
    finally:
        workers.close()


def test_quantiles_follow_a_refill_and_run_on_a_joined_batch(apd, ctx, cases):
    from audio_pattern_discovery_amd.alignments import AlignmentWorkers, NDSequence
    from audio_pattern_discovery_amd.discovery import Discovery
    c = next(c for c in cases if c["pen"][0] < 0 and len(c["perc"]) == 8 and c["by"] == "query")
    seqs, pairs, pen, perc = c["seqs"], c["pairs"], c["pen"], c["perc"]
    rng = np.random.default_rng(412)
    fresh = [rng.integers(0, 3, s.shape).astype(F) for s in seqs]
    batch = make_batch(ctx, seqs)
    try:
        before = raw_quantiles(apd, ctx, batch, pen, pairs, "query", perc)
        assert same(before, qref.quantiles(c["curves"], c["lengths"], pairs, "query", perc))
        frames = np.ascontiguousarray(np.concatenate(fresh, axis=0))
        apd.check(apd.lib().apd_batch_refill(ctx.handle, batch.handle, C.c_void_p(frames.ctypes.data), 0), ctx.handle)
        after = raw_quantiles(apd, ctx, batch, pen, pairs, "query", perc)
    finally:
        batch.close()
    cache = {(x, y): ref.curves(fresh[x], fresh[y], *pen) for x, y in set(pairs)}
    fresh_curves = [cache[p] for p in pairs]
    assert same(after, qref.quantiles(fresh_curves, c["lengths"], pairs, "query", perc)) and not np.array_equal(bits(after[0]), bits(before[0]))
    # joined: the queries in one AlignmentWorkers, the streams in another; numbers of the two joined
    wa, wb = AlignmentWorkers.new([NDSequence(s) for s in seqs[:2]], ctx), AlignmentWorkers.new([NDSequence(s) for s in seqs[2:]], ctx)
    params = Discovery(insertion_penalty=pen[0], deletion_penalty=pen[1], match_penalty=pen[2])
    try:
        out = wa.score_quantiles(pairs, params, perc, by="query", streams=wb, strict=False)
        empty = wa.score_quantiles(np.zeros((0, 2), np.uint32), params, perc, by="all", streams=wb)
    finally:
        wa.close()
        wb.close()
    assert same((out[0], out[4]) + out[1:4], before)
    assert empty[0].shape == (0, 8) and all(len(a) == 0 for a in empty[1:])


def test_argument_errors_launch_nothing(apd, ctx):
    L = apd.lib()
    rng = np.random.default_rng(413)
    seqs = [rng.standard_normal((n, 13)).astype(F) for n in (12, 40, 25)]
    batch = make_batch(ctx, seqs)
    other = apd.Context(0)
    cfg = apd.AlignConfig(1.0, 1.0, 1.0, 1.0)
    u32p, u64p, f32p, i32p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_float), C.POINTER(C.c_int32)
    pairs = np.array([(0, 1), (2, 2), (0, 2)], dtype=np.uint32)
    perc = np.array([0.1, 0.5, 0.9, 0.2, 0.3, 0.4, 0.6, 0.7, 0.8], dtype=F)
    values, status = np.full(40, CANARY, dtype=np.uint32), np.full(40, CANARY, dtype=np.uint32)
    group_of, entries, nans = (np.full(5, 77, dtype=np.uint64) for _ in range(3))
    ng = C.c_uint64(99)
    prp, pcp, vp, sp = pairs.ctypes.data_as(u32p), perc.ctypes.data_as(f32p), values.ctypes.data_as(f32p), status.ctypes.data_as(i32p)
    gp, ep, np_ = group_of.ctypes.data_as(u64p), entries.ctypes.data_as(u64p), nans.ctypes.data_as(u64p)

    def call(ctx_=None, batch_=None, pairs_=prp, n=3, grouping=0, perc_=pcp, n_perc=2, values_=vp, status_=sp, group_=gp, entries_=ep, nans_=np_,
             ng_=C.byref(ng)):
        return L.apd_spot_quantiles((ctx_ or ctx).handle, (batch_ or batch).handle, C.byref(cfg), pairs_, n, grouping, perc_, n_perc, values_, status_,
                                    group_, entries_, nans_, ng_)

    def untouched():
        return (not ctx.stream_busy() and np.all(values == CANARY) and np.all(status == CANARY) and ng.value == 99
                and all(np.all(a == 77) for a in (group_of, entries, nans)))

    try:
        ctx.synchronize()
        for bad in (dict(grouping=3), dict(grouping=-1), dict(n_perc=0), dict(n_perc=9), dict(perc_=None), dict(values_=None), dict(ng_=None),
                    dict(pairs_=None), dict(ctx_=other)):
            assert call(**bad) == apd.APD_ERR_INVALID_ARG and untouched(), bad
        wrong = np.array([(0, 1), (3, 0)], dtype=np.uint32)                                                       # index = n_seq
        assert call(pairs_=wrong.ctypes.data_as(u32p), n=2) == apd.APD_ERR_INVALID_ARG and untouched()
        for grouping in (0, 1, 2):                                                                                # an empty list: zero groups
            ng.value = 99
            assert call(pairs_=None, n=0, grouping=grouping) == apd.APD_OK and ng.value == 0
            ng.value = 99
            assert untouched()
        # every optional output absent; eight quantiles
        assert call(grouping=1, n_perc=8, status_=None, group_=None, entries_=None, nans_=None) == apd.APD_OK and ng.value == 2
        assert np.all(values[16:] == CANARY) and not np.any(values[:16] == CANARY) and np.all(status == CANARY)
        assert all(np.all(a == 77) for a in (group_of, entries, nans))
        assert call(grouping=2) == apd.APD_OK and ng.value == 1 and entries[0] == 40 + 25 + 25 and group_of[:3].tolist() == [0, 0, 0] and nans[0] == 0
        assert status[:2].view(np.int32).tolist() == [0, 0] and np.all(status[2:] == CANARY)
    finally:
        batch.close()
        other.close()
    # an empty sequence in the batch, a query beyond the documented limit: apd_spot's codes, before anything is launched
    from audio_pattern_discovery_amd.alignments import Batch
    frames = np.zeros((16385 + 5, 1), dtype=F)
    empty = Batch(ctx, frames[:9], np.array([0, 4, 4, 9], dtype=np.uint64), 1)
    long_ = Batch(ctx, frames, np.array([0, 16385, 16390], dtype=np.uint64), 1)
    one = np.array([(0, 2)], dtype=np.uint32)
    values[:], status[:], ng.value = CANARY, CANARY, 99
    for a in (group_of, entries, nans):
        a[:] = 77
    try:
        ctx.synchronize()
        assert call(batch_=empty, pairs_=one.ctypes.data_as(u32p), n=1) == apd.APD_ERR_EMPTY_SEQUENCE and untouched()
        one[0] = (0, 1)
        assert call(batch_=long_, pairs_=one.ctypes.data_as(u32p), n=1) == apd.APD_ERR_UNSUPPORTED and untouched()
        one[0] = (1, 0)                                                                                           # the other way round runs
        assert call(batch_=long_, pairs_=one.ctypes.data_as(u32p), n=1, n_perc=1) == apd.APD_OK and ng.value == 1 and entries[0] == 16385
        assert values[0] == 0 and status[0] == 0                                                                  # all-zero frames: +0.0
        # one group of 2^24 + 1 pairs, pooled by query or over the list: refused before anything is launched or written
        values[:], status[:], ng.value = CANARY, CANARY, 99
        for a in (group_of, entries, nans):
            a[:] = 77
        many = np.tile(np.array([(1, 0)], dtype=np.uint32), ((1 << 24) + 1, 1))
        ctx.synchronize()
        for grouping in (1, 2):
            assert call(batch_=long_, pairs_=many.ctypes.data_as(u32p), n=len(many), grouping=grouping, n_perc=1) == apd.APD_ERR_UNSUPPORTED
            assert untouched() and b"2^24" in L.apd_last_error(ctx.handle)
    finally:
        empty.close()
        long_.close()


def test_timing_covers_the_sweep_and_the_select(apd, ctx, big):
    """apd_last_kernel_ms of the call against that of apd_spot with curves on the same list, on 2^24 + 3 entries with eight quantiles,
    where the select is no rounding error of the sweep.  The bound: the four passes read both curves of every entry, 4 x 8 bytes x
    entries = 537 MB, and nothing on the chip delivers that at more than 16 TB/s (twice the HBM peak, to allow for the curves sitting
    in the last-level cache), so a span that holds the select exceeds the sweep's by 0.033 ms at the very least; a span that ended
    before the select would exceed it by nothing.  Best of three on either side."""
    workers, pairs, _, _ = big
    L = apd.lib()
    cfg = config(apd, UNIT)
    entries = (1 << 24) + 3
    pr = np.ascontiguousarray(pairs, dtype=np.uint32)
    off = np.zeros(len(pr) + 1, dtype=np.uint64)
    cost, start = np.zeros(entries, dtype=F), np.zeros(entries, dtype=np.uint32)
    perc = np.linspace(0.05, 0.95, 8)

    def sweep():
        apd.check(L.apd_spot(ctx.handle, workers._batch.handle, C.byref(cfg), pr.ctypes.data_as(C.POINTER(C.c_uint32)), len(pr),
                             cost.ctypes.data_as(C.POINTER(C.c_float)), start.ctypes.data_as(C.POINTER(C.c_uint32)), entries,
                             off.ctypes.data_as(C.POINTER(C.c_uint64)), None), ctx.handle)
        return ctx.last_kernel_ms()

    def select():
        got = raw_quantiles(apd, ctx, workers._batch, UNIT, pairs, "all", perc)
        assert int(got[3][0]) == entries and not got[1].any()
        return ctx.last_kernel_ms()

    ctx.set_timing(True)
    try:
        sweep()                                                                  # both routes once before either is timed
        select()
        sweep_ms = min(sweep() for _ in range(3))
        quantile_ms = min(select() for _ in range(3))
    finally:
        ctx.set_timing(False)
    floor_ms = 4 * 8 * entries / 16e12 * 1e3
    print("sweep %.4f ms, sweep + select %.4f ms, floor of the select %.4f ms" % (sweep_ms, quantile_ms, floor_ms))
    assert sweep_ms > 0.0 and quantile_ms >= sweep_ms + floor_ms, (sweep_ms, quantile_ms, floor_ms)
