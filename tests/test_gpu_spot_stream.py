"""GPU tests of the streaming spotting session (apd_spot_stream_*, kernels spot_kernel<SpotStreamSweep, RT, D> of csrc/dtw_spot_stream.hip) against
the checkers tests/_spot_reference.py (the whole stream) and tests/_spot_stream_reference.py (chunk by chunk).

The promise under test takes no tolerance: whatever the chunking, the curves of the pushes, one after the other, are the bits of the
whole stream's curves (start equal, cost equal as uint32, NaN matched as NaN: _path_reference.bits), and `best` after every push is
the checker's best of the prefix pushed so far.  The first group runs EVERY instantiation <RT, D> on the case tests/_spot_matrix.py
builds for it -- query lengths that put row n on every row of a lane, R = 1 .. 4 and the LDS class, a 40- and a 91-frame stream as
two channels of one session -- under the chunkings of CHUNKINGS: a chunk of one column, both parities of m + lane_n, a chunk just
below, at and above a wavefront, and no-op pushes (a zero-length chunk in the list, and every push after one channel has finished
while the other has not).  The case's gate pairs (both square-root branches) and tie pairs (small integers) run as sessions of their
own on their own streams; the gate streams have 37 frames, so they take the 40-frame chunkings with the last chunk three shorter.
Every push runs under APD_DEBUG_PLAN and must name exactly the intended kernel with every pair of the session."""
import ctypes as C
import re

import numpy as np
import pytest

import _kernel_table as kt
import _spot_matrix as sm
import _spot_reference as ref
import _spot_stream_reference as sref
from test_gpu_spot import make_batch, raw_spot, reference

pytestmark = pytest.mark.gpu
F = np.float32
UNIT, SKEWED = sm.UNIT, sm.SKEWED
ALL = 0xFFFFFFFF

CHUNKINGS = {40: [(40,), (1,) * 40, (39, 1), (2, 38)],
             91: [(91,), (64, 27), (27, 64), (1, 63, 2, 25), (65, 1, 25), (45, 0, 46)]}
CHUNKINGS[sm.GATE_STREAM] = [c[:-1] + (c[-1] - (40 - sm.GATE_STREAM),) for c in CHUNKINGS[40]]

REGISTER_KERNELS = [k for k in kt.spot_kernels() if k[1] > 0]           # every <RT, D> with a kernel dimension, the LDS class included
ANY_DIMENSIONS = sm.any_dimensions(kt.parse_dims(kt.header_text()))
_seen = set()                                   # (kind, RT, D) of every spotting-kernel line read in this module


def kernel_id(kernel):
    return "<%d, %d>" % kernel


def spot_limit(name):
    m = re.search(r"constexpr\s+uint32_t\s+%s\s*=\s*(0x[0-9A-Fa-f]+|\d+)u?\s*;" % name, kt.header_text())
    return int(m.group(1), 0)


@pytest.fixture(scope="module")
def ctx(apd):
    c = apd.Context(0)
    yield c
    c.close()


class RawStream:
    """An apd_spot_stream through ctypes, with canaries behind every output."""

    def __init__(self, apd, ctx, batch, queries, pen, channels):
        self.apd, self.ctx, self.dim = apd, ctx, batch.dim
        self.n_queries, self.channels = len(queries), channels
        self.n_pairs = len(queries) * channels
        self.handle = C.c_void_p()
        cfg = apd.AlignConfig(float("nan"), pen[0], pen[1], pen[2])              # the band percentage is not read
        q = np.ascontiguousarray(queries, dtype=np.uint32)
        self.status = apd.lib().apd_spot_stream_create(ctx.handle, batch.handle, C.byref(cfg), q.ctypes.data_as(C.POINTER(C.c_uint32)), len(q),
                                                       channels, C.byref(self.handle))

    def close(self):
        if self.handle:
            assert self.apd.lib().apd_spot_stream_destroy(self.handle) == self.apd.APD_OK
            self.handle = C.c_void_p()

    def __enter__(self):
        assert self.status == self.apd.APD_OK, self.status
        return self

    def __exit__(self, *exc):
        self.close()

    def columns(self, channel):
        out = C.c_uint64(0)
        assert self.apd.lib().apd_spot_stream_columns(self.handle, channel, C.byref(out)) == self.apd.APD_OK
        return int(out.value)

    def reset(self, channel=ALL, first_column=0):
        return self.apd.lib().apd_spot_stream_reset(self.ctx.handle, self.handle, channel, first_column)

    def push_status(self, chunks, curves=True, device=None, short=0, dim=None):
        """(status, list of (cost, start) per pair, best, curve_off).  device: a DeviceBuffer that already holds the packed frames;
        short: entries the capacity is short of what the push needs."""
        apd, L = self.apd, self.apd.lib()
        u32p, u64p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_float)
        arrays = [np.ascontiguousarray(c, dtype=F) for c in chunks]
        assert len(arrays) == self.channels and all(a.ndim == 2 for a in arrays)
        chunk_off = np.zeros(self.channels + 1, dtype=np.uint64)
        chunk_off[1:] = np.cumsum([len(a) for a in arrays])
        host = np.ascontiguousarray(np.concatenate(arrays, axis=0))
        frames = C.c_void_p(device.ptr) if device is not None else C.c_void_p(host.ctypes.data)
        head = (self.ctx.handle, self.handle, frames, chunk_off.ctypes.data_as(u64p), self.dim if dim is None else dim, int(device is not None))
        off = np.full(self.n_pairs + 1, 77, dtype=np.uint64)
        before = [self.columns(k) for k in range(self.channels)]
        status = L.apd_spot_stream_push(*head, None, None, 0, off.ctypes.data_as(u64p), None)          # sizes only: nothing moves
        if status != apd.APD_OK:
            return status, None, None, None
        assert [self.columns(k) for k in range(self.channels)] == before
        want_off = np.concatenate([[0], np.cumsum(np.repeat(np.diff(chunk_off), self.n_queries))]).astype(np.uint64)
        assert np.array_equal(off, want_off)
        best = np.full((self.n_pairs + 1) * 16, 0x55, dtype=np.uint8).view(ref.BEST)                  # one record more than asked: a canary
        bestp = best.ctypes.data_as(C.POINTER(apd.SpotBest))
        off2 = np.zeros(self.n_pairs + 1, dtype=np.uint64)
        if not curves:
            status = L.apd_spot_stream_push(*head, None, None, 0, off2.ctypes.data_as(u64p), bestp)
            assert best[-1]["end"] == 0x55555555
            return status, [], best[:self.n_pairs].copy(), off
        total = int(off[-1])
        cost = np.full((total + 1) * 4, 0x55, dtype=np.uint8).view(F)
        start = np.full(total + 1, 0x55555555, dtype=np.uint32)
        status = L.apd_spot_stream_push(*head, cost.ctypes.data_as(f32p), start.ctypes.data_as(u32p), total - short, off2.ctypes.data_as(u64p), bestp)
        assert best[-1]["end"] == 0x55555555 and start[-1] == 0x55555555 and cost.view(np.uint32)[-1] == 0x55555555
        if status != apd.APD_OK:
            assert [self.columns(k) for k in range(self.channels)] == before
            return status, None, None, off
        assert np.array_equal(off, off2)
        assert [self.columns(k) for k in range(self.channels)] == [b + len(a) for b, a in zip(before, arrays)]
        out = [(cost[int(off[p]):int(off[p + 1])].copy(), start[int(off[p]):int(off[p + 1])].copy()) for p in range(self.n_pairs)]
        return status, out, best[:self.n_pairs].copy(), off

    def push(self, chunks, **kw):
        status, out, best, _ = self.push_status(chunks, **kw)
        self.apd.check(status, self.ctx.handle)
        return out, best


def rounds_of(streams, chunkings):
    """The pushes of channels whose streams are cut as chunkings[k]: round r holds channel k's r-th chunk, or none of its frames
    once the channel has finished."""
    cuts = [sref.split(y, sizes) for y, sizes in zip(streams, chunkings)]
    return [[c[r] if r < len(c) else y[:0] for c, y in zip(cuts, streams)] for r in range(max(len(c) for c in cuts))]


def run_session(stream, streams, chunkings, first_column=0):
    """Pushes the rounds; returns per pair the concatenated (cost, start), and per round (best records, columns pushed per channel)."""
    parts = [([], []) for _ in range(stream.n_pairs)]
    after = []
    done = [0] * len(streams)
    for chunks in rounds_of(streams, chunkings):
        out, best = stream.push(chunks)
        for k, c in enumerate(chunks):
            done[k] += len(c)
        for p, (cost, start) in enumerate(out):
            assert len(cost) == len(start) == len(chunks[p // stream.n_queries])
            parts[p][0].append(cost)
            parts[p][1].append(start)
        after.append((best, tuple(done)))
    return [(np.concatenate(c), np.concatenate(s)) for c, s in parts], after


def assert_session(got, after, wants, n_queries, lens, what, first_column=0):
    """got / after of run_session against wants[p] = the whole stream's (cost, start, best) of pair p = channel n_queries + q."""
    for p, (cost, start) in enumerate(got):
        want_cost, want_start, _ = wants[p]
        want_start = np.where(want_start > 0, want_start + first_column, 0).astype(np.uint32)
        assert np.array_equal(start, want_start), (what, p, "start")
        assert np.array_equal(ref.bits(cost), ref.bits(want_cost)), (what, p, "cost")
        prefix = sref.prefix_bests(want_cost, want_start, lens[p % n_queries], first_column)
        for best, done in after:
            assert ref.same_best(best[p], prefix[done[p // n_queries]]), (what, p, done, best[p])


def assert_stream_plan(err, kernel, n_pairs, pushes, r_max=None):
    rt, d = kernel
    launches = kt.read_spot_launches(err)
    plan = kt.read_spot_plan(err)
    _seen.update(plan)
    assert set(plan) == {("stream", rt, d)}, "%s: the spotting kernels that ran are %r" % (kernel_id(kernel), plan)
    assert len(launches) == pushes and all(launch["pairs"] == n_pairs for launch in launches), launches
    if rt == 0:
        assert all((launch["r_max"], launch["lds"]) == (r_max, r_max * 64 * 8) for launch in launches), launches
    else:
        assert all(launch["r_max"] is None and launch["lds"] is None for launch in launches)


def stream_case(apd, ctx, capfd, case):
    key = ("matrix", case.kernel, case.dim)                  # the references of tests/test_gpu_spot_matrix.py, computed once
    batch = make_batch(ctx, case.seqs)
    try:
        nq = len({x for x, _ in case.unit_pairs})
        channels = [nq + s for s in range(len(sm.STREAMS))]
        assert [case.lengths[y] for y in channels] == list(sm.STREAMS) and sorted(case.unit_pairs) == [(q, y) for q in range(nq) for y in channels]
        sessions = [(UNIT, list(range(nq)), channels), (SKEWED, sorted({x for x, _ in case.skewed_pairs}), channels)]
        sessions += [(UNIT, [x], [y]) for x, y in case.gate_pairs + case.tie_pairs]
        for pen, queries, ys in sessions:
            pairs = [(x, y) for y in ys for x in queries]                                    # p = channel n_queries + q
            wants = [reference(key, case.seqs, pen, x, y) for x, y in pairs]
            whole, _, _ = raw_spot(apd, ctx, batch, pen, pairs)                               # apd_spot on the very batch
            lens = [case.lengths[x] for x in queries]
            r_max = max(kt.spot_rows_per_lane(n) for n in lens)
            streams = [case.seqs[y] for y in ys]
            per_channel = [CHUNKINGS[len(s)] for s in streams]
            with RawStream(apd, ctx, batch, queries, pen, len(ys)) as stream:
                for k in range(max(len(c) for c in per_channel)):
                    chunkings = [c[k % len(c)] for c in per_channel]
                    assert stream.reset() == apd.APD_OK
                    with kt.debug_plan(capfd) as err:
                        got, after = run_session(stream, streams, chunkings)
                    what = "%s %s %s" % (kernel_id(case.kernel), pen, chunkings)
                    rounds = rounds_of(streams, chunkings)
                    assert_stream_plan(err[0], case.kernel, len(pairs), sum(1 for r in rounds if sum(len(c) for c in r)), r_max)
                    assert_session(got, after, wants, len(queries), lens, what)
                    for p in range(len(pairs)):
                        assert np.array_equal(got[p][1], whole[p][1]) and np.array_equal(ref.bits(got[p][0]), ref.bits(whole[p][0])), (what, p)
    finally:
        batch.close()


@pytest.mark.parametrize("kernel", REGISTER_KERNELS, ids=kernel_id)
def test_stream_kernel_runs_and_matches_the_checker_under_every_chunking(apd, ctx, capfd, kernel):
    stream_case(apd, ctx, capfd, sm.register_case(*kernel))


@pytest.mark.parametrize("dim", ANY_DIMENSIONS)
def test_stream_of_a_dimension_without_kernels_of_its_own(apd, ctx, capfd, dim):
    case = sm.any_case(dim)
    assert case.kernel == (0, 0) and len(case.tie_pairs) == 1
    stream_case(apd, ctx, capfd, case)


def test_every_stream_kernel_was_dispatched():
    """The union of the kernels' own lines over this module: every <RT, D> the header implies, as a streaming sweep and as nothing
    else.  A case that silently stopped reaching its kernel fails here (and so does a run of this test without the cases above)."""
    want = {("stream",) + kernel for kernel in kt.spot_kernels()}
    assert _seen == want, "never dispatched: %r; not in the header: %r" % (sorted(want - _seen), sorted(_seen - want))


def col(values):
    return np.array(values, dtype=F).reshape(-1, 1)


HAND_X, HAND_Y = col([0, 1]), col([0, 1, 0])


def test_hand_case_and_first_column_through_both_entry_points(apd, ctx):
    from audio_pattern_discovery_amd.alignments import AlignmentWorkers, NDSequence
    from audio_pattern_discovery_amd.discovery import Discovery
    batch = make_batch(ctx, [HAND_X])
    try:
        with RawStream(apd, ctx, batch, [0], UNIT, 1) as stream:
            for shift in (0, 1000):
                assert stream.reset(ALL, shift) == apd.APD_OK and stream.columns(0) == shift
                (first,), best = stream.push([HAND_Y[:1]])
                assert first[0].tolist() == [1.0] and first[1].tolist() == [1 + shift]
                (second,), best = stream.push([HAND_Y[1:]])
                assert second[0].tolist() == [0.0, 2.0] and second[1].tolist() == [1 + shift, 2 + shift]
                assert (best[0]["end"], best[0]["start"], best[0]["cost"], best[0]["score"]) == (2 + shift, 1 + shift, 0.0, 0.0)
                assert stream.columns(0) == 3 + shift
    finally:
        batch.close()
    workers = AlignmentWorkers.new([NDSequence(HAND_X)], ctx)
    session = workers.spot_stream([0], Discovery(), channels=1)
    try:
        for shift in (0, 1000):
            session.reset(first_column=shift)
            curves, best = session.push([HAND_Y[:1]])
            assert curves[0][0].tolist() == [1.0] and curves[0][1].tolist() == [1 + shift]
            curves, best = session.push([HAND_Y[1:]])
            assert curves[0][0].tolist() == [0.0, 2.0] and curves[0][1].tolist() == [1 + shift, 2 + shift]
            assert (best[0]["end"], best[0]["start"]) == (2 + shift, 1 + shift) and session.columns(0) == 3 + shift
            none, alone = session.push([HAND_Y[:0]], curves=False)
            assert none == [] and np.array_equal(alone.view(np.uint32), best.view(np.uint32))
    finally:
        session.close()
        workers.close()


def small_case(seed=31, dim=13, n=(70, 9), m=(50, 33)):
    rng = np.random.default_rng(seed)
    queries = [rng.standard_normal((k, dim)).astype(F) for k in n]
    streams = [rng.standard_normal((k, dim)).astype(F) for k in m]
    return queries, streams


def wants_of(queries, streams, pen):
    return [ref.spot(x, y, *pen) for y in streams for x in queries]


def test_first_column_shifts_a_two_class_session(apd, ctx):
    queries, streams = small_case()
    wants = wants_of(queries, streams, SKEWED)
    lens = [len(q) for q in queries]
    batch = make_batch(ctx, queries)
    try:
        with RawStream(apd, ctx, batch, [0, 1], SKEWED, 2) as stream:
            for shift in (0, 1000):
                assert stream.reset(ALL, shift) == apd.APD_OK
                got, after = run_session(stream, streams, [(20, 1, 29), (33,)])
                assert_session(got, after, wants, 2, lens, "shift %d" % shift, first_column=shift)
    finally:
        batch.close()


def test_reset_of_one_channel_leaves_the_other_running(apd, ctx):
    queries, streams = small_case(seed=32)
    wants = wants_of(queries, streams, UNIT)
    lens = [len(q) for q in queries]
    batch = make_batch(ctx, queries)
    try:
        with RawStream(apd, ctx, batch, [0, 1], UNIT, 2) as stream:
            first, _ = stream.push([streams[0][:30], streams[1][:10]])
            assert stream.reset(1, 0) == apd.APD_OK and (stream.columns(0), stream.columns(1)) == (30, 0)
            second, best = stream.push([streams[0][30:], streams[1]])          # channel 0 goes on, channel 1 starts over with its whole stream
            for q in range(2):
                cost = np.concatenate([first[q][0], second[q][0]])
                start = np.concatenate([first[q][1], second[q][1]])
                assert np.array_equal(ref.bits(cost), ref.bits(wants[q][0])) and np.array_equal(start, wants[q][1])
                assert ref.same_best(best[q], wants[q][2])
                cost, start = second[2 + q]
                assert np.array_equal(ref.bits(cost), ref.bits(wants[2 + q][0])) and np.array_equal(start, wants[2 + q][1])
                assert ref.same_best(best[2 + q], wants[2 + q][2])
            assert stream.reset(2, 0) == apd.APD_ERR_INVALID_ARG
    finally:
        batch.close()
    assert lens == [70, 9]


def test_a_refused_push_leaves_the_state_untouched(apd, ctx):
    queries, streams = small_case(seed=33)
    wants = wants_of(queries, streams, UNIT)
    batch = make_batch(ctx, queries)
    try:
        with RawStream(apd, ctx, batch, [0, 1], UNIT, 2) as stream:
            first, _ = stream.push([streams[0][:17], streams[1][:5]])
            rest = [streams[0][17:], streams[1][5:]]
            status, _, _, _ = stream.push_status(rest, short=1)
            assert status == apd.APD_ERR_INVALID_ARG
            second, best = stream.push(rest)
            for p in range(4):
                cost = np.concatenate([first[p][0], second[p][0]])
                start = np.concatenate([first[p][1], second[p][1]])
                assert np.array_equal(ref.bits(cost), ref.bits(wants[p][0])) and np.array_equal(start, wants[p][1]), p
                assert ref.same_best(best[p], wants[p][2])
    finally:
        batch.close()


def test_column_limit(apd, ctx):
    limit = spot_limit("kSpotMaxStream")
    rng = np.random.default_rng(34)
    x, y = rng.standard_normal((3, 5)).astype(F), rng.standard_normal((10, 5)).astype(F)
    batch = make_batch(ctx, [x])
    try:
        with RawStream(apd, ctx, batch, [0], UNIT, 1) as stream:
            assert stream.reset(0, limit) == apd.APD_ERR_UNSUPPORTED and stream.columns(0) == 0
            assert stream.reset(0, limit - 10) == apd.APD_OK and stream.columns(0) == limit - 10
            (got,), best = stream.push([y[:9]])
            (want,) = sref.run(x, [y[:9]], first_column=limit - 10)
            assert np.array_equal(ref.bits(got[0]), ref.bits(want[0])) and np.array_equal(got[1], want[1]) and ref.same_best(best[0], want[2])
            assert got[1].min() > limit - 10 and stream.columns(0) == limit - 1
            status, _, _, _ = stream.push_status([y[9:]])
            assert status == apd.APD_ERR_UNSUPPORTED and stream.columns(0) == limit - 1
    finally:
        batch.close()


def test_query_length_and_dimension(apd, ctx):
    longest = spot_limit("kSpotMaxQuery")
    rng = np.random.default_rng(35)
    too_long = make_batch(ctx, [np.zeros((longest + 1, 1), dtype=F)])
    try:
        stream = RawStream(apd, ctx, too_long, [0], UNIT, 1)
        assert stream.status == apd.APD_ERR_UNSUPPORTED and not stream.handle
        assert RawStream(apd, ctx, too_long, [1], UNIT, 1).status == apd.APD_ERR_INVALID_ARG     # no such sequence
        assert RawStream(apd, ctx, too_long, [0], UNIT, 0).status == apd.APD_ERR_INVALID_ARG     # no channel
    finally:
        too_long.close()
    x, y = rng.standard_normal((1, 13)).astype(F), rng.standard_normal((7, 13)).astype(F)
    batch = make_batch(ctx, [x])
    try:
        with RawStream(apd, ctx, batch, [0], UNIT, 1) as stream:
            status, _, _, _ = stream.push_status([y[:1, :12]], dim=12)
            assert status == apd.APD_ERR_INVALID_ARG and stream.columns(0) == 0
            sizes = (1, 5, 1)                                                # a one-frame query: only lane 0 is ever live
            got, after = run_session(stream, [y], [sizes])
            assert_session(got, after, [ref.spot(x, y)], 1, [1], "one-frame query")
    finally:
        batch.close()


def test_device_frames_and_best_only(apd, ctx):
    queries, streams = small_case(seed=36)
    batch = make_batch(ctx, queries)
    try:
        with RawStream(apd, ctx, batch, [0, 1], SKEWED, 2) as stream:
            records = {}
            for mode in ("host", "device", "best only"):
                assert stream.reset() == apd.APD_OK
                records[mode] = []
                for lo, hi in ((0, 12), (12, 13), (13, 33)):
                    chunks = [s[lo:hi] for s in streams]
                    buf = ctx.upload(np.ascontiguousarray(np.concatenate(chunks, axis=0))) if mode == "device" else None
                    out, best = stream.push(chunks, curves=mode != "best only", device=buf)
                    if buf is not None:
                        buf.free()
                    records[mode].append((out, best))
            for (h_out, h_best), (d_out, d_best), (b_out, b_best) in zip(records["host"], records["device"], records["best only"]):
                assert b_out == [] and np.array_equal(h_best.view(np.uint32), d_best.view(np.uint32))
                assert np.array_equal(h_best.view(np.uint32), b_best.view(np.uint32))
                for (hc, hs), (dc, ds) in zip(h_out, d_out):
                    assert np.array_equal(hc.view(np.uint32), dc.view(np.uint32)) and np.array_equal(hs, ds)
            wants = wants_of(queries, [s[:33] for s in streams], SKEWED)
            for p in range(4):
                assert ref.same_best(records["host"][-1][1][p], wants[p][2])
    finally:
        batch.close()


def test_non_finite_frames_in_the_middle_chunk(apd, ctx):
    queries, streams = small_case(seed=37, n=(70, 130), m=(45, 45))
    streams[0][20, 3] = np.nan
    streams[1][22, 0] = np.inf
    wants = wants_of(queries, streams, UNIT)
    batch = make_batch(ctx, queries)
    try:
        with RawStream(apd, ctx, batch, [0, 1], UNIT, 2) as stream:
            got, after = run_session(stream, streams, [(15, 10, 20), (15, 10, 20)])
            assert_session(got, after, wants, 2, [70, 130], "non-finite")
            assert np.isnan(got[0][0]).any() or np.isinf(got[0][0]).any()
    finally:
        batch.close()
