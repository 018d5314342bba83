"""GPU tests of the online detector of a streaming session (apd_spot_stream_detect / _flush / _hits, kernels of
csrc/dtw_spot_online.hip) against the checker tests/_spot_online_reference.py, through the C ABI and through SpotStream.

Every record is compared bit for bit: pair, end, start and rank equal, cost and score equal as uint32.  The seeded cases are those of
tests/_spot_online_cases.py; tests/test_spot_online_reference.py asserts on the checker alone that each of them shows every event of
the machine (replacement, discard at equal scores, discard by the floor, emission by the timer and by displacement, a cross-pair tie
per channel), so no comparison here passes vacuously.  Shapes: queries of 3 to 70 frames and one of 130 (a one-row and a three-row
lane class), D = 13, 5 and 2, one to three channels, streams of 150 to 400 columns, 1, 2, 3, 4 and 65 queries per channel."""
import ctypes as C

import numpy as np
import pytest

import _spot_online_cases as cases
import _spot_online_reference as online
import _spot_stream_reference as sref
from _path_reference import bits
from test_gpu_spot import make_batch
from test_gpu_spot_stream import RawStream, rounds_of

pytestmark = pytest.mark.gpu
F = np.float32
INF = F(np.inf)
ALL = 0xFFFFFFFF
NEVER = online.NEVER
CANARY = 0x55555555


@pytest.fixture(scope="module")
def ctx(apd):
    c = apd.Context(0)
    yield c
    c.close()


class OnlineStream(RawStream):
    """RawStream with the three calls of the detector, canaries behind the drained records."""

    def detect_status(self, thresholds, per_stream, holdoff):
        if thresholds is None:
            return self.apd.lib().apd_spot_stream_detect(self.ctx.handle, self.handle, None, int(per_stream), holdoff)
        thr = np.ascontiguousarray(np.broadcast_to(np.asarray(thresholds, dtype=F), (self.channels, self.n_queries)))
        return self.apd.lib().apd_spot_stream_detect(self.ctx.handle, self.handle, thr.ctypes.data_as(C.POINTER(C.c_float)), int(per_stream), holdoff)

    def detect(self, thresholds, per_stream=False, holdoff=0):
        self.apd.check(self.detect_status(thresholds, per_stream, holdoff), self.ctx.handle)

    def flush_status(self, channel=ALL):
        return self.apd.lib().apd_spot_stream_flush(self.ctx.handle, self.handle, channel)

    def flush(self, channel=ALL):
        self.apd.check(self.flush_status(channel), self.ctx.handle)

    def queued(self):
        n = C.c_uint64(99)
        self.apd.check(self.apd.lib().apd_spot_stream_hits(self.ctx.handle, self.handle, None, 0, C.byref(n)), self.ctx.handle)
        return int(n.value)

    def hits(self, short=0):
        """The drained hits; with short > 0 the capacity is that much below the queued count: nothing may be written or consumed."""
        n = self.queued()
        buf = np.full((n + 1) * 6, CANARY, dtype=np.uint32).view(online.HIT)
        m = C.c_uint64(99)
        self.apd.check(self.apd.lib().apd_spot_stream_hits(self.ctx.handle, self.handle, buf.ctypes.data_as(C.POINTER(self.apd.SpotHit)), n - short,
                                                           C.byref(m)), self.ctx.handle)
        assert int(m.value) == n
        if short and n:
            assert np.all(buf.view(np.uint32) == CANARY) and self.queued() == n
            return None
        assert np.all(buf[n:].view(np.uint32) == CANARY) and self.queued() == 0
        return buf[:n].copy()


def open_session(apd, ctx, c, arm=True, **kw):
    """(batch, armed session) of a case."""
    batch = make_batch(ctx, c["queries"])
    s = OnlineStream(apd, ctx, batch, list(range(len(c["queries"]))), c["pen"], len(c["streams"]))
    assert s.status == apd.APD_OK
    if arm:
        s.detect(kw.get("thresholds", c["thresholds"]), kw.get("per_stream", c["per_stream"]), kw.get("holdoff", c["holdoff"]))
    return batch, s


def drain_order(parts, c, per_stream=None):
    per_stream = c["per_stream"] if per_stream is None else per_stream
    parts = [p for p in parts if len(p)]
    return online.ordered(np.concatenate(parts) if parts else np.zeros(0, online.HIT), len(c["queries"]), per_stream)


def even(c, size):
    """Every channel cut into chunks of `size` columns."""
    return [(size,) * (len(y) // size) + ((len(y) % size,) if len(y) % size else ()) for y in c["streams"]]


def cycle(c, sizes):
    out = []
    for y in c["streams"]:
        left, cut, i = len(y), [], 0
        while left:
            cut.append(min(sizes[i % len(sizes)], left))
            left -= cut[-1]
            i += 1
        out.append(tuple(cut))
    return out


def chunkings(c):
    lengths = [len(y) for y in c["streams"]]
    out = {"one push": [(m,) for m in lengths], "64": even(c, 64), "63, 64, 65": cycle(c, (63, 64, 65)),
           "zero-length chunks": [(0, 40, 0, 0, m - 41, 0, 1) for m in lengths], "1, 5, 130": cycle(c, (1, 5, 130))}
    if len(lengths) > 1:                       # channels of different chunk lengths in one push, one of them empty in most rounds
        out["unequal"] = [(m,) if k == 0 else cycle(c, (17 + 30 * k, 0, 64))[k] for k, m in enumerate(lengths)]
    return out


def run(apd, ctx, c, cuts, drain_every=False, check_prefix=False, **kw):
    """The case pushed as `cuts` says (best only on the host), then flushed.  Returns the drained hits in drain order."""
    batch, s = open_session(apd, ctx, c, **kw)
    drained = []
    try:
        for chunks in rounds_of(c["streams"], cuts):
            s.push(chunks, curves=False)
            if drain_every:
                drained.append(s.hits())
                if check_prefix:               # the promise: what is out now is what the machine emits up to each channel's column
                    now = [s.columns(k) for k in range(s.channels)]
                    want = cases.expected(c, upto=now, holdoff=kw.get("holdoff"), per_stream=kw.get("per_stream"), thresholds=kw.get("thresholds"))
                    assert online.same_hits(drain_order(drained, c, kw.get("per_stream")), want), now
        s.flush()
        drained.append(s.hits())
    finally:
        s.close()
        batch.close()
    return drain_order(drained, c, kw.get("per_stream"))


@pytest.mark.parametrize("name", sorted(cases.SPECS))
def test_every_chunking_gives_the_checkers_hits(apd, ctx, name):
    c = cases.case(name)
    want = cases.expected(c, flush=True)
    assert len(want) >= 10
    for label, cuts in chunkings(c).items():
        assert [sum(x) for x in cuts] == [len(y) for y in c["streams"]], label
        got = run(apd, ctx, c, cuts)           # several pushes without a drain, one drain at the end
        assert online.same_hits(got, want), label


@pytest.mark.parametrize("name", ["pairs_d13", "channels_d5", "zeros_d2"])
def test_draining_after_every_push_gives_the_same_sequence(apd, ctx, name):
    c = cases.case(name)
    want = cases.expected(c, flush=True)
    if name == "channels_d5":                  # 64-column pushes carry a pending window across and see it replaced behind the boundary
        assert min(cases.carried_across(c, 64)) >= 1
    if name == "zeros_d2":
        assert cases.zero_sign_ties(c) >= 1 and np.any(bits(want["score"]) == 0x80000000)
    for cuts in (even(c, 64), chunkings(c).get("unequal", cycle(c, (63, 64, 65)))):
        assert online.same_hits(run(apd, ctx, c, cuts, drain_every=True, check_prefix=True), want)


def test_columns_one_by_one(apd, ctx):
    c = cases.case("channels_d5")
    want = cases.expected(c, flush=True)
    assert online.same_hits(run(apd, ctx, c, [(1,) * len(y) for y in c["streams"]]), want)
    assert online.same_hits(run(apd, ctx, c, [(1,) * len(y) for y in c["streams"]], drain_every=True), want)


def test_the_timer_edge_inside_a_stretch_without_candidates(apd, ctx):
    """A push that ends exactly at P.end + holdoff emits nothing, one column more emits -- at a column where the group has no
    candidate, so it is the look at the chunk's last column that fires."""
    c = cases.case("channels_d13")
    (hits, when), = cases.expected(c, parts=True)
    per_query = c["curves"][0]
    sc = np.array([[online.score_at(cost[i], start[i], n, i + 1) for i in range(len(cost))] for (cost, start), n in zip(per_query, c["lengths"])])
    with np.errstate(invalid="ignore"):
        cand = np.any((sc < c["thresholds"][0][:, None]) & (np.array([s for _, s in per_query]) != 0), axis=0)
    edge = [i for i in range(len(hits)) if when[i] == int(hits["end"][i]) + c["holdoff"] + 1 and not cand[when[i] - 1]]
    assert edge
    i = edge[0]
    w = int(when[i])
    batch, s = open_session(apd, ctx, c)
    try:
        y = c["streams"][0]
        s.push([y[:w - 1]], curves=False)
        first = s.hits()
        assert online.same_hits(first, cases.expected(c, upto=w - 1)) and len(first) == i
        s.push([y[w - 1:w]], curves=False)
        second = s.hits()
        assert online.same_hits(second, hits[i:i + 1])
    finally:
        s.close()
        batch.close()


@pytest.mark.parametrize("holdoff", [0, 4, 6, NEVER])
def test_holdoffs_around_the_template_length(apd, ctx, holdoff):
    """0, one less and one more than the 5 frames of the template, and the timer that never fires."""
    c = cases.case("channels_d13")
    assert c["lengths"][0] == 5
    stats = online.new_stats()
    want = cases.expected(c, holdoff=holdoff, stats=stats)
    assert len(want) >= 5 and (stats["timer"] == 0 and stats["displace"] >= 5 if holdoff == NEVER else stats["timer"] >= 1)
    batch, s = open_session(apd, ctx, c, holdoff=holdoff)
    try:
        for chunks in rounds_of(c["streams"], cycle(c, (65, 63))):
            s.push(chunks, curves=False)
        assert online.same_hits(s.hits(), want)                              # without a flush: the timer and displacement alone
        s.flush()
        last = s.hits()
        flushed = cases.expected(c, holdoff=holdoff, flush=True)
        assert len(last) == len(flushed) - len(want) == (0 if holdoff == 0 else 1) and online.same_hits(drain_order([want, last], c), flushed)
    finally:
        s.close()
        batch.close()


@pytest.mark.parametrize("n_queries", [1, 2])
def test_one_and_two_queries_per_channel(apd, ctx, n_queries):
    """Per channel with one query is per pair; with two -- a query and its copy -- every candidate column is a tie that goes to the
    smaller pair.  (65 queries: the case channels_q65 above.)"""
    whole = cases.case("channels_d13")
    c = cases.subset(whole, [0, 2][:n_queries])
    stats = online.new_stats()
    want = cases.expected(c, flush=True, stats=stats)
    if n_queries == 1:
        assert online.same_hits(want, cases.expected(c, flush=True, per_stream=False))
    else:
        assert stats["tie"] >= 10 and np.all(want["pair"] == 0)
    assert online.same_hits(run(apd, ctx, c, cycle(c, (63, 64, 65))), want)
    assert online.same_hits(run(apd, ctx, c, cycle(c, (63, 64, 65)), per_stream=False), cases.expected(c, flush=True, per_stream=False))


def special_session(apd, ctx, queries, stream, pen, thresholds, per_stream, holdoff, cuts):
    """A case of one channel made on the spot: (drained hits after a flush, the checker's, the curves)."""
    curves = [sref.Session(q, *pen).push(stream)[:2] for q in queries]
    c = {"queries": queries, "streams": [stream], "lengths": [len(q) for q in queries], "curves": [curves], "pen": pen,
         "thresholds": np.broadcast_to(np.asarray(thresholds, dtype=F), (1, len(queries))), "per_stream": per_stream, "holdoff": holdoff}
    return run(apd, ctx, c, [cuts]), cases.expected(c, flush=True), curves


def test_negative_scores_nan_columns_and_start_zero_columns(apd, ctx):
    rng = np.random.default_rng(41)
    stream = rng.integers(0, 3, (150, 13)).astype(F)
    queries = [stream[20:24].copy(), stream[60:63].copy(), stream[20:24].copy()]
    cuts = (64, 1, 85)
    # match = -1: costs and scores go negative; the most negative windows win their overlaps
    got, want, curves = special_session(apd, ctx, queries, stream, (1.0, 1.0, -1.0), -0.05, True, 3, cuts)
    assert online.same_hits(got, want) and len(want) >= 3 and np.all(want["score"] < 0)
    got, want, _ = special_session(apd, ctx, queries, stream, (1.0, 1.0, -1.0), [-0.05, INF, -0.2], False, 3, cuts)
    assert online.same_hits(got, want) and len(set(want["pair"].tolist())) == 3 and np.all(want["score"] < 0)
    # an infinite insertion penalty: where no branch is strictly smallest the cell takes MATCH out of column 0 -- start 0, cost +INF
    # -- and INF * 0 is NaN; both stand next to finite columns.  +INF as threshold takes every finite score and nothing else
    got, want, curves = special_session(apd, ctx, queries, stream, (float("inf"), 1.0, -1.0), INF, False, 3, cuts)
    cost, start = np.concatenate([cv[0] for cv in curves]), np.concatenate([cv[1] for cv in curves])
    assert np.any(np.isnan(cost)) and np.any(np.isfinite(cost)) and np.any(start == 0) and np.all(np.isfinite(want["score"]))
    assert online.same_hits(got, want) and len(want) >= 3
    # a NaN frame in the stream: the columns whose alignments touch it are NaN (the start is free, so the table recovers behind
    # them), and none of them is a candidate even under +INF
    poisoned = stream.copy()
    poisoned[100, 3] = np.nan
    got, want, curves = special_session(apd, ctx, queries, poisoned, cases.UNIT, INF, True, 3, cuts)
    dead = np.flatnonzero(np.all([np.isnan(cv[0]) for cv in curves], axis=0)) + 1
    assert len(dead) >= 3 and not np.any(np.isin(want["end"], dead)) and np.any(want["end"] > dead.max())
    assert online.same_hits(got, want) and len(want) >= 3


def test_threshold_edges(apd, ctx):
    """-INF and NaN give no candidate, +INF every finite score; a threshold that IS the pair's smallest score rejects it (strict),
    the next float above accepts it."""
    c = cases.subset(cases.case("pairs_d13"), [0, 1, 2, 4])
    n_q = 4
    thr = c["thresholds"].copy()
    lowest = []
    for k in range(2):
        cost, start = c["curves"][k][3]
        sc = np.array([online.score_at(cost[i], start[i], c["lengths"][3], i + 1) for i in range(len(cost)) if start[i] != 0])
        lowest.append(F(np.nanmin(sc)))
    thr[0] = [-INF, INF, F(np.nan), lowest[0]]
    thr[1] = [INF, F(np.nan), -INF, np.nextafter(lowest[1], INF)]
    want = cases.expected(c, flush=True, thresholds=thr)
    by_pair = np.bincount(want["pair"], minlength=2 * n_q)
    assert by_pair[[0, 2, 3, n_q + 1, n_q + 2]].tolist() == [0] * 5 and np.all(by_pair[[1, n_q, n_q + 3]] >= 1)
    assert np.all(bits(want["score"][want["pair"] == n_q + 3]) == bits(lowest[1]))
    assert online.same_hits(run(apd, ctx, c, cycle(c, (64, 65)), thresholds=thr), want)


def test_reset_flush_and_ranks(apd, ctx):
    """A reset of one channel in mid-stream, with a first_column shift, clears that channel's pending windows only and the ranks go
    on; then a flush of one channel and a flush of all."""
    c = cases.case("channels_d5")
    R, B = 102, 1000
    pend = [cases.pending_at(c, k, R) for k in range(3)]
    assert all(len(p) == 1 for p in pend)                                       # every channel has a window pending at the reset
    after = [sref.Session(q, *c["pen"], first_column=B).push(c["streams"][1][R:])[:2] for q in c["queries"]]
    args = (c["lengths"], c["thresholds"][1], True, c["holdoff"])
    reset_plain = online.with_reset(1, c["curves"][1], after, R, B, *args)[0]
    ranks = {}
    head, _ = online.channel_hits(1, c["curves"][1], *args, upto=R, ranks=ranks)
    tail, _ = online.channel_hits(1, after, *args, first_column=B, flush_at=[B + len(c["streams"][1]) - R], ranks=ranks)
    reset_flushed = np.concatenate([head, tail])
    assert len(tail) >= 2 and tail["rank"][0] == len(head) >= 1 and np.all(tail["start"] > B)
    plain, flushed = cases.expected(c, parts=True), cases.expected(c, flush=True, parts=True)
    batch, s = open_session(apd, ctx, c)
    try:
        s.push([y[:R] for y in c["streams"]], curves=False)
        assert s.reset(1, B) == apd.APD_OK and [s.columns(k) for k in range(3)] == [R, B, R]
        s.push([y[R:] for y in c["streams"]], curves=False)
        s.flush(0)
        first = s.hits()
        assert online.same_hits(first, drain_order([flushed[0][0], reset_plain, plain[2][0]], c))
        s.flush()                                                            # channel 0 has nothing pending any more
        second = s.hits()
        assert len(second) == 2 and second["pair"].tolist()[0] // 4 == 1 and second["pair"].tolist()[1] // 4 == 2
        assert online.same_hits(drain_order([first, second], c), drain_order([flushed[0][0], reset_flushed, flushed[2][0]], c))
        assert s.queued() == 0
        s.flush()                                                            # nothing pending: nothing emitted
        assert s.queued() == 0
    finally:
        s.close()
        batch.close()


def test_arming_again_in_mid_stream_and_disarming(apd, ctx):
    c = cases.case("channels_d13")
    y = c["streams"][0]
    batch, s = open_session(apd, ctx, c)
    try:
        s.push([y[:150]], curves=False)
        assert s.queued() >= 1
        s.detect(c["thresholds"], True, 2)                                   # a new origin at column 150, the queue discarded
        assert s.queued() == 0
        s.flush()
        assert s.queued() == 0                                               # and so is what was pending
        s.push([y[150:300]], curves=False)
        s.flush()
        want = cases.expected(c, origin=150, upto=300, holdoff=2, flush=True)
        assert len(want) >= 3 and np.all(want["start"] > 150) and want["rank"][0] == 0
        assert online.same_hits(s.hits(), want)
        s.detect(c["thresholds"], False, 2)                                  # the other grouping, from column 300 on
        s.push([y[300:]], curves=False)
        s.flush()
        assert online.same_hits(s.hits(), cases.expected(c, origin=300, holdoff=2, flush=True, per_stream=False))
        s.push([y[:10]], curves=False)
        assert s.queued() >= 0
        s.detect(None, False, 0)                                             # disarmed
        assert s.queued() == 0 and s.flush_status() == apd.APD_ERR_UNSUPPORTED
        assert "not armed" in apd.lib().apd_last_error(ctx.handle).decode()
        s.push([y[10:20]], curves=False)
        assert s.queued() == 0
    finally:
        s.close()
        batch.close()


def test_the_queue_keeps_everything_until_a_full_drain(apd, ctx):
    c = cases.case("pairs_d13")
    want = cases.expected(c, flush=True)
    batch, s = open_session(apd, ctx, c)
    try:
        counts = []
        for chunks in rounds_of(c["streams"], even(c, 32)):                  # several pushes without a drain: the queue grows
            s.push(chunks, curves=False)
            counts.append(s.queued())
        assert counts == sorted(counts) and counts[-1] > 64 and len(set(counts)) > 3
        assert s.hits(short=1) is None                                       # one short: nothing written, nothing consumed
        s.flush()
        assert s.queued() == len(want) and s.hits(short=1) is None
        assert online.same_hits(s.hits(), want)
    finally:
        s.close()
        batch.close()


def test_an_unarmed_session_returns_the_same_curves_and_bests(apd, ctx):
    c = cases.case("pairs_d13")
    batch, armed = open_session(apd, ctx, c)
    plain = OnlineStream(apd, ctx, batch, list(range(len(c["queries"]))), c["pen"], len(c["streams"]))
    try:
        assert plain.status == apd.APD_OK and plain.queued() == 0
        for r, chunks in enumerate(rounds_of(c["streams"], cycle(c, (65, 1, 64)))):
            a, b = armed.push(chunks, curves=r % 2 == 0), plain.push(chunks, curves=r % 2 == 0)
            assert len(a[0]) == len(b[0]) and a[1].tobytes() == b[1].tobytes()
            for (ca, sa), (cb, sb) in zip(a[0], b[0]):
                assert ca.tobytes() == cb.tobytes() and sa.tobytes() == sb.tobytes()
        armed.flush()
        assert online.same_hits(armed.hits(), cases.expected(c, flush=True)) and plain.queued() == 0
    finally:
        armed.close()
        plain.close()
        batch.close()


def test_errors_leave_the_state_untouched(apd, ctx):
    c = cases.case("channels_d13")
    y = c["streams"][0]
    L = apd.lib()
    other = apd.Context(0)
    batch, s = open_session(apd, ctx, c)
    try:
        s.push([y[:200]], curves=False)
        queued = s.queued()
        assert queued >= 1
        thr = np.ascontiguousarray(c["thresholds"])
        thrp = thr.ctypes.data_as(C.POINTER(C.c_float))
        n = C.c_uint64(99)
        for compete in (2, -1):
            assert L.apd_spot_stream_detect(ctx.handle, s.handle, thrp, compete, 3) == apd.APD_ERR_INVALID_ARG
        assert L.apd_spot_stream_detect(other.handle, s.handle, thrp, 1, 3) == apd.APD_ERR_INVALID_ARG
        assert L.apd_spot_stream_detect(None, s.handle, thrp, 1, 3) == apd.APD_ERR_INVALID_ARG
        assert L.apd_spot_stream_detect(ctx.handle, None, thrp, 1, 3) == apd.APD_ERR_INVALID_ARG
        assert L.apd_spot_stream_flush(other.handle, s.handle, ALL) == apd.APD_ERR_INVALID_ARG
        assert L.apd_spot_stream_flush(ctx.handle, s.handle, 1) == apd.APD_ERR_INVALID_ARG                    # channel >= n_channels
        assert L.apd_spot_stream_hits(other.handle, s.handle, None, 0, C.byref(n)) == apd.APD_ERR_INVALID_ARG
        assert L.apd_spot_stream_hits(ctx.handle, s.handle, None, 0, None) == apd.APD_ERR_INVALID_ARG
        assert L.apd_spot_stream_hits(ctx.handle, s.handle, None, queued, C.byref(n)) == apd.APD_ERR_INVALID_ARG   # room, but nowhere to write
        assert n.value == queued and s.queued() == queued
        status, _, _, _ = s.push_status([y[200:210]], dim=c["dim"] + 1)                                        # a refused push moves nothing
        assert status == apd.APD_ERR_INVALID_ARG and s.columns(0) == 200 and s.queued() == queued
        s.push([y[200:]], curves=False)
        s.flush()
        assert online.same_hits(s.hits(), cases.expected(c, flush=True))                                       # as if none of it had happened
    finally:
        s.close()
        batch.close()
        other.close()
    plain = OnlineStream(apd, ctx, make_batch(ctx, c["queries"]), [0], c["pen"], 1)
    try:
        assert plain.flush_status() == apd.APD_ERR_UNSUPPORTED and plain.queued() == 0
    finally:
        plain.close()


def test_hits_of_a_session_with_a_history_trace_through_python(apd, ctx):
    """SpotStream.detect / flush / hits, a history and a detector together: every drained hit goes to SpotStream.paths, the start
    found is the hit's and the last step's cost is the hit's cost, bit for bit."""
    from audio_pattern_discovery_amd.alignments import SPOT_HIT, SPOT_WINDOW, AlignmentWorkers, NDSequence
    from audio_pattern_discovery_amd.discovery import Discovery
    c = cases.case("channels_d5")
    n_q = len(c["queries"])
    workers = AlignmentWorkers.new([NDSequence(q) for q in c["queries"]], ctx)
    params = Discovery(insertion_penalty=c["pen"][0], deletion_penalty=c["pen"][1], match_penalty=c["pen"][2])
    stream = workers.spot_stream(list(range(n_q)), params, channels=3, history=512)
    try:
        assert len(stream.hits()) == 0                                       # not armed: empty
        stream.detect(c["thresholds"], per_stream=True, holdoff=c["holdoff"])
        got = []
        for chunks in rounds_of(c["streams"], cycle(c, (70, 33))):
            stream.push(chunks, curves=False)
            hits = stream.hits()
            assert hits.dtype == SPOT_HIT
            got.append(hits)
        stream.flush()
        got.append(stream.hits())
        got = drain_order([g.astype(online.HIT) for g in got], c)
        assert online.same_hits(got, cases.expected(c, flush=True))
        win = np.zeros(len(got), dtype=SPOT_WINDOW)
        win["x"], win["y"], win["end"], win["start"] = got["pair"] % n_q, got["pair"] // n_q, got["end"], got["start"]
        paths, found, scores = stream.paths(win)
        assert np.array_equal(found, got["start"]) and np.array_equal(bits(scores), bits(got["score"]))
        for steps, h in zip(paths, got):
            assert len(steps) >= 2 and bits(steps["cost"][-1:])[0] == bits(h["cost"]) and int(steps["j"][-1]) == int(h["end"])
        # a scalar and a per-query vector are broadcast; None disarms
        stream.detect(0.5, per_stream=False, holdoff=stream.NEVER)
        stream.detect(c["thresholds"][0], per_stream=True)
        stream.flush(channel=1)
        stream.detect(None)
        with pytest.raises(Exception):
            stream.flush()
    finally:
        stream.close()
        workers.close()
