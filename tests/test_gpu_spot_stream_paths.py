"""GPU tests of the history of a streaming session (apd_spot_stream_keep / _history / _paths; kernels spot_kernel<SpotStreamRecordSweep, RT, D>,
spot_stream_frames_kernel and dtw_spot_stream_trace of csrc/dtw_spot_stream_rec.hip) against the checker tests/_spot_path_reference.py
on the whole stream, shifted and aged out as tests/_spot_stream_path_reference.expected says (that module's ring session is shown
equal to it, on the CPU, by tests/test_spot_stream_path_reference.py).

The promise takes no tolerance: a window whose columns all lie in the kept [first, last] of its channel gets the steps (i, j, the bits
of cost, op), found start and score of apd_spot_paths on the whole stream, whatever the chunking; the others get the aged-out form.
The first group runs EVERY instantiation <RT, D> on the case tests/_spot_matrix.py builds for it (query lengths that put row n on
every row of a lane, a 40- and a 91-frame stream as two channels, unit and skewed penalties), with H = 24 (a push that wraps the
rings, and pushes of one column), H = 50 (a zero-length chunk) and H = 128 (nothing ages out: also compared with apd_spot_paths on
the same GPU).  After every push every pair is asked the windows (end, S[n][end]) of its last H + 3 pushed columns, one window with a
wrong start and one "no window" record; the curves and bests of the pushes must still be apd_spot's, and every push must name
exactly the `streamrec` kernel of the case with every pair.  Before the GPU is touched the windows of a case are counted on the
checker's numbers: for H = 24 and H = 50 at least 10 are traced, at least 10 have aged out and one traced window spans H / 2 columns
or more -- a history that traced nothing, or never let go of anything, would pass no test here."""
import ctypes as C
import os

import numpy as np
import pytest

import _kernel_table as kt
import _spot_matrix as sm
import _spot_path_reference as ref
import _spot_stream_path_reference as hist
import _spot_stream_reference as sref
from test_gpu_spot import make_batch, reference
from test_gpu_spot_paths import raw_paths, table
from test_gpu_spot_stream import ALL, ANY_DIMENSIONS, REGISTER_KERNELS, RawStream, assert_session, kernel_id, rounds_of, spot_limit

pytestmark = pytest.mark.gpu
F = np.float32
UNIT, SKEWED = sm.UNIT, sm.SKEWED
CANARY = 0x55555555
# (H, the chunking of the 40-frame channel, of the 91-frame channel)
CONFIGS = ((24, (40,), (91,)), (24, (1,) * 40, (1, 63, 2, 25)), (50, (39, 1), (45, 0, 46)), (128, (2, 38), (64, 27)))
_seen = set()                                   # (kind, RT, D) of every spotting-kernel line read in this module
_ANSWERS = {}


@pytest.fixture(scope="module")
def ctx(apd):
    c = apd.Context(0)
    yield c
    c.close()


class HistoryStream(RawStream):
    """RawStream with the three entry points of the history, canaries behind every output of apd_spot_stream_paths."""

    def keep(self, history):
        return self.apd.lib().apd_spot_stream_keep(self.ctx.handle, self.handle, history)

    def history(self, channel):
        first, last = C.c_uint64(0), C.c_uint64(0)
        assert self.apd.lib().apd_spot_stream_history(self.handle, channel, C.byref(first), C.byref(last)) == self.apd.APD_OK
        return int(first.value), int(last.value)

    def paths_status(self, records, n_of):
        """(status, list of STEP arrays, found_start, scores) for records [(q, channel, end, start)]; n_of[q]: frames of query q.
        Checks the size query against the bound, that unused slots are zero and that nothing is written past what was asked."""
        apd, L = self.apd, self.apd.lib()
        win = np.array([tuple(int(v) for v in r) for r in records], dtype=ref.WINDOW).reshape(-1)
        k = len(win)
        u32p, u64p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_float)
        head = (self.ctx.handle, self.handle, win.ctypes.data_as(C.POINTER(apd.SpotWindow)), k)
        off = np.full(k + 1, 77, dtype=np.uint64)
        status = L.apd_spot_stream_paths(*head, None, 0, off.ctypes.data_as(u64p), None, None, None)           # sizes only
        if status != apd.APD_OK:
            return status, None, None, None
        assert [int(off[p + 1] - off[p]) for p in range(k)] == [ref.bound(n_of[int(r[0])], int(r[2]), int(r[3])) for r in records]
        total = int(off[-1])
        steps = np.full((total + 1) * 16, 0x55, dtype=np.uint8).view(ref.STEP)                                  # one slot more: a canary
        lens, found = np.full(k + 1, CANARY, dtype=np.uint32), np.full(k + 1, CANARY, dtype=np.uint32)
        scores = np.full(k + 1, CANARY, dtype=np.uint32).view(F)
        off2 = np.zeros(k + 1, dtype=np.uint64)
        status = L.apd_spot_stream_paths(*head, steps.ctypes.data_as(C.POINTER(apd.PathStep)), total, off2.ctypes.data_as(u64p),
                                         lens.ctypes.data_as(u32p), found.ctypes.data_as(u32p), scores.ctypes.data_as(f32p))
        assert steps[-1]["op"] == CANARY and lens[-1] == CANARY and found[-1] == CANARY and scores.view(np.uint32)[-1] == CANARY
        if status != apd.APD_OK:
            return status, None, None, None
        assert np.array_equal(off, off2)
        paths = []
        for p in range(k):
            lo, hi = int(off[p]), int(off[p + 1])
            assert lens[p] <= hi - lo and not steps[lo + int(lens[p]):hi].view(np.uint32).any()                 # unused slots are zeroed
            paths.append(steps[lo:lo + int(lens[p])].copy())
        return status, paths, found[:k].copy(), scores[:k].copy()

    def paths(self, records, n_of):
        status, paths, found, scores = self.paths_status(records, n_of)
        self.apd.check(status, self.ctx.handle)
        return paths, found, scores


def whole_answer(key, seqs, pen, x, y, end, start):
    """The checker's answer on the whole stream (columns counted from the reset), computed once per window."""
    k = (key, pen, x, y, end, start)
    if k not in _ANSWERS:
        _ANSWERS[k] = ref.answer(table(key, seqs, pen, x, y), len(seqs[x]), end, start)
    return _ANSWERS[k]


def kept_of(history, origin, last):
    return (max(origin + 1, last - history + 1) if history else last + 1), last


def recent_records(tab_start, q, channel, history, last, first_column=0, pushed_from=0):
    """The windows asked of one pair after a push: (end, S[n][end]) for every end of the last H + 3 pushed columns, one window with
    a wrong start and one "no window" record.  tab_start[j]: S[n][j] of the whole stream, j counted from the reset."""
    lo = max(first_column + pushed_from + 1, last - history - 2)
    out = []
    for end in range(lo, last + 1):
        s = int(tab_start[end - first_column])
        out.append((q, channel, end, s + first_column if s else 0))
    if last > first_column + pushed_from:
        s = int(tab_start[last - first_column]) + first_column
        wrong = [w for w in (s - 1, s + 1) if first_column + 1 <= w <= last]
        if wrong:
            out.append((q, channel, last, wrong[0]))
    out.append((q, channel, 0, 0))
    return out


def same_window(got, want):
    return ref.same_steps(got[0], want[0]) and int(got[1]) == int(want[1]) and ref.bits([got[2]])[0] == ref.bits([want[2]])[0]


def plan_of(case, key, pen, queries, ys, history, chunkings):
    """Without a GPU: per round (the chunks, the records asked after it, what the contract says of each)."""
    streams = [case.seqs[y] for y in ys]
    done = [0] * len(ys)
    plan = []
    for chunks in rounds_of(streams, chunkings):
        for k, c in enumerate(chunks):
            done[k] += len(c)
        records, wants = [], []
        for k, y in enumerate(ys):
            kept = kept_of(history, 0, done[k])
            for q, x in enumerate(queries):
                tab_start = table(key, case.seqs, pen, x, y)[1][len(case.seqs[x])]
                for r in recent_records(tab_start, q, k, history, done[k]):
                    records.append(r)
                    wants.append(hist.expected(whole_answer(key, case.seqs, pen, x, y, r[2], r[3]), len(case.seqs[x]), 0, kept, r[2], r[3]))
        plan.append((chunks, records, wants, tuple(done)))
    return plan


def sessions_of(case):
    nq = len({x for x, _ in case.unit_pairs})
    channels = [nq + s for s in range(len(sm.STREAMS))]
    assert [case.lengths[y] for y in channels] == list(sm.STREAMS)
    return [(UNIT, list(range(nq)), channels), (SKEWED, sorted({x for x, _ in case.skewed_pairs}), channels)]


def populations(plans):
    """(traced, aged out, longest traced span in columns) among the windows with the table's start, over [(history, plan)]."""
    traced = aged = span = 0
    for _, plan in plans:
        for _, records, wants, _ in plan:
            for r, w in zip(records, wants):
                if r[2] and r[3] and (int(w[1]) == r[3] or int(w[1]) == 0):
                    if len(w[0]):
                        traced, span = traced + 1, max(span, r[2] - r[3] + 1)
                    else:
                        aged += 1
    return traced, aged, span


def history_case(apd, ctx, capfd, case):
    key = ("matrix", case.kernel, case.dim)                  # the references of tests/test_gpu_spot_matrix.py, computed once
    sessions = sessions_of(case)
    plans = {}
    for s, (pen, queries, ys) in enumerate(sessions):
        for c, (history, short, long_) in enumerate(CONFIGS):
            plans[(s, c)] = (history, plan_of(case, key, pen, queries, ys, history, [short, long_]))
    for history in (24, 50):                                 # the condition of the module's docstring, before the GPU is touched
        traced, aged, span = populations([v for v in plans.values() if v[0] == history])
        assert traced >= 10 and aged >= 10 and 2 * span >= history, (kernel_id(case.kernel), history, traced, aged, span)
    batch = make_batch(ctx, case.seqs)
    try:
        for s, (pen, queries, ys) in enumerate(sessions):
            pairs = [(x, y) for y in ys for x in queries]                                    # p = channel n_queries + q
            curve_wants = [reference(key, case.seqs, pen, x, y) for x, y in pairs]
            lens = [case.lengths[x] for x in queries]
            r_max = max(kt.spot_rows_per_lane(n) for n in lens)
            with HistoryStream(apd, ctx, batch, queries, pen, len(ys)) as stream:
                for c, (history, short, long_) in enumerate(CONFIGS):
                    what = "%s %s H %d %s" % (kernel_id(case.kernel), pen, history, (short, long_))
                    assert stream.reset() == apd.APD_OK and stream.keep(history) == apd.APD_OK
                    parts = [([], []) for _ in pairs]
                    after, pushes = [], 0
                    with kt.debug_plan(capfd) as err:
                        for chunks, records, wants, done in plans[(s, c)][1]:
                            out, best = stream.push(chunks)
                            pushes += any(len(ch) for ch in chunks)
                            for p, (cost, start) in enumerate(out):
                                parts[p][0].append(cost)
                                parts[p][1].append(start)
                            after.append((best, done))
                            for k in range(len(ys)):
                                assert stream.history(k) == kept_of(history, 0, done[k]), (what, done)
                            paths, found, scores = stream.paths(records, lens)
                            for t, (r, w) in enumerate(zip(records, wants)):
                                assert same_window((paths[t], found[t], scores[t]), w), (what, done, r)
                    launches = kt.read_spot_launches(err[0])
                    plan = kt.read_spot_plan(err[0])
                    _seen.update(plan)
                    assert set(plan) == {("streamrec",) + case.kernel}, "%s: the spotting kernels that ran are %r" % (what, plan)
                    assert len(launches) == pushes and all(launch["pairs"] == len(pairs) for launch in launches), launches
                    if case.kernel[0] == 0:
                        assert all((launch["r_max"], launch["lds"]) == (r_max, r_max * 64 * 8) for launch in launches), launches
                    got = [(np.concatenate(cs), np.concatenate(ss)) for cs, ss in parts]
                    assert_session(got, after, curve_wants, len(queries), lens, what)          # the table is not touched
                    if history >= max(sm.STREAMS):                                           # nothing has aged out: apd_spot_paths itself
                        records = [(q, k, end, int(curve_wants[k * len(queries) + q][1][end - 1]))
                                   for k in range(len(ys)) for q in range(len(queries)) for end in range(1, case.lengths[ys[k]] + 1)]
                        paths, found, scores = stream.paths(records, lens)
                        whole = raw_paths(apd, ctx, batch, pen, [(queries[q], ys[k], end, start) for q, k, end, start in records])
                        for t, r in enumerate(records):
                            assert same_window((paths[t], found[t], scores[t]), (whole[0][t], whole[1][t], whole[2][t])), (what, r)
                            assert r[3] == 0 or len(paths[t]) > 0, (what, r)
    finally:
        batch.close()


@pytest.mark.parametrize("kernel", REGISTER_KERNELS, ids=kernel_id)
def test_history_kernel_runs_and_matches_the_checker(apd, ctx, capfd, kernel):
    history_case(apd, ctx, capfd, sm.register_case(*kernel))


@pytest.mark.parametrize("dim", ANY_DIMENSIONS)
def test_history_of_a_dimension_without_kernels_of_its_own(apd, ctx, capfd, dim):
    case = sm.any_case(dim)
    assert case.kernel == (0, 0)
    history_case(apd, ctx, capfd, case)


def test_every_history_kernel_was_dispatched():
    """The union of the kernels' own lines over this module: every <RT, D> the header implies, as a recording streaming sweep and
    as nothing else (and so does a run of this test without the cases above fail)."""
    want = {("streamrec",) + kernel for kernel in kt.spot_kernels()}
    assert _seen == want, "never dispatched: %r; not in the header: %r" % (sorted(want - _seen), sorted(_seen - want))


# ---- edges, on one small case: D = 13, queries of 70 and 9 frames, streams of 50 and 33

def small_case(seed=41, dim=13, n=(70, 9), m=(50, 33)):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((k, dim)).astype(F) for k in n], [rng.standard_normal((k, dim)).astype(F) for k in m]


class Model:
    """What the contract says of a session on small_case: the whole-stream tables, per channel the first column and the origin."""

    def __init__(self, queries, streams, pen, first_column=0):
        self.queries, self.pen = queries, pen
        self.lens = [len(q) for q in queries]
        self.set_streams(streams, [first_column] * len(streams))
        self.history = 0

    def set_streams(self, streams, first_columns):
        self.streams, self.first = list(streams), list(first_columns)
        self.tabs = [[ref.table(x, y, *self.pen) for x in self.queries] for y in streams]
        self.origin = list(first_columns)
        self.pushed = [0] * len(streams)                       # frames pushed since the reset
        self.kept_from = [0] * len(streams)                    # frames pushed when the history began

    def keep(self, history):
        self.history = history
        self.origin = [f + p for f, p in zip(self.first, self.pushed)]
        self.kept_from = list(self.pushed)

    def last(self, k):
        return self.first[k] + self.pushed[k]

    def kept(self, k):
        return kept_of(self.history, self.origin[k], self.last(k))

    def records(self):
        out = []
        for k in range(len(self.streams)):
            for q in range(len(self.queries)):
                out += recent_records(self.tabs[k][q][1][self.lens[q]], q, k, self.history, self.last(k), self.first[k])
        return out

    def want(self, r):
        q, k, end, start = r
        fc = self.first[k]
        whole = ref.answer(self.tabs[k][q], self.lens[q], end - fc if end else 0, start - fc if start else 0)
        return hist.expected(whole, self.lens[q], fc, self.kept(k), end, start)


def push_and_check(stream, model, sizes, what, device=None):
    chunks = [y[p:p + s] for y, p, s in zip(model.streams, model.pushed, sizes)]
    stream.push(chunks, device=device)
    model.pushed = [p + s for p, s in zip(model.pushed, sizes)]
    check(stream, model, what)


def check(stream, model, what):
    for k in range(len(model.streams)):
        assert stream.history(k) == model.kept(k), (what, k)
    records = model.records()
    paths, found, scores = stream.paths(records, model.lens)
    traced = 0
    for t, r in enumerate(records):
        assert same_window((paths[t], found[t], scores[t]), model.want(r)), (what, r)
        traced += len(paths[t]) > 0
    return traced, (paths, found, scores)


def test_one_column_of_history(apd, ctx):
    queries, streams = small_case()
    queries = queries + [streams[0][7:8].copy()]               # a one-frame query equal to a stream frame: windows of one column
    model = Model(queries, streams, UNIT)
    batch = make_batch(ctx, queries)
    try:
        with HistoryStream(apd, ctx, batch, [0, 1, 2], UNIT, 2) as stream:
            assert stream.keep(1) == apd.APD_OK
            model.keep(1)
            traced = 0
            for sizes in ((7, 5), (1, 1), (1, 0), (20, 27)):
                push_and_check(stream, model, sizes, "H = 1 %s" % (sizes,))
                traced += check(stream, model, "again")[0]
            assert traced >= 1 and model.kept(0) == (29, 29)
    finally:
        batch.close()


def test_keep_in_mid_stream_again_and_none(apd, ctx):
    queries, streams = small_case(seed=42)
    model = Model(queries, streams, SKEWED)
    batch = make_batch(ctx, queries)
    try:
        with HistoryStream(apd, ctx, batch, [0, 1], SKEWED, 2) as stream:
            assert stream.history(0) == (1, 0)
            stream.push([streams[0][:12], streams[1][:3]])
            model.pushed = [12, 3]
            assert stream.keep(16) == apd.APD_OK                 # in mid-stream: the history starts behind columns 12 and 3
            model.keep(16)
            check(stream, model, "kept, nothing pushed")
            push_and_check(stream, model, (9, 9), "origin")
            assert model.kept(0) == (13, 21) and model.kept(1) == (4, 12)
            push_and_check(stream, model, (20, 0), "wrapped")
            assert stream.keep(40) == apd.APD_OK                 # again, with another H: empty again
            model.keep(40)
            check(stream, model, "kept again")
            push_and_check(stream, model, (9, 21), "second history")
            assert model.kept(0) == (42, 50) and model.kept(1) == (13, 33)
            records = model.records()
            assert stream.keep(0) == apd.APD_OK and stream.history(0) == (51, 50)
            status, _, _, _ = stream.paths_status(records, model.lens)            # the size query is legal, the paths are not
            assert status == apd.APD_ERR_UNSUPPORTED and b"history" in apd.lib().apd_last_error(ctx.handle)
            assert stream.paths_status([], model.lens)[0] == apd.APD_ERR_UNSUPPORTED
    finally:
        batch.close()


def test_reset_of_one_channel_empties_only_its_history(apd, ctx):
    queries, streams = small_case(seed=43)
    model = Model(queries, streams, UNIT)
    batch = make_batch(ctx, queries)
    try:
        with HistoryStream(apd, ctx, batch, [0, 1], UNIT, 2) as stream:
            assert stream.keep(24) == apd.APD_OK
            model.keep(24)
            push_and_check(stream, model, (30, 20), "before the reset")
            assert stream.reset(1, 500) == apd.APD_OK
            model.first[1], model.origin[1], model.pushed[1] = 500, 500, 0
            assert stream.history(0) == (7, 30) and stream.history(1) == (501, 500)
            check(stream, model, "after the reset")
            push_and_check(stream, model, (20, 33), "channel 1 from its first frame")
            assert model.kept(1) == (510, 533)
    finally:
        batch.close()


def test_columns_near_the_limit_and_device_chunks(apd, ctx):
    limit = spot_limit("kSpotMaxStream")
    queries, streams = small_case(seed=44)
    model = Model(queries, streams, SKEWED)
    batch = make_batch(ctx, queries)
    try:
        with HistoryStream(apd, ctx, batch, [0, 1], SKEWED, 2) as stream:
            assert stream.reset(ALL, limit - 101) == apd.APD_OK and stream.keep(24) == apd.APD_OK     # column + lane sits near 2^32
            model.set_streams(streams, [limit - 101] * 2)
            model.keep(24)
            for sizes in ((30, 10), (1, 0), (19, 23)):
                chunks = [y[p:p + s] for y, p, s in zip(model.streams, model.pushed, sizes)]
                buf = ctx.upload(np.ascontiguousarray(np.concatenate(chunks, axis=0)))
                push_and_check(stream, model, sizes, "near the limit %s" % (sizes,), device=buf)
                buf.free()
            assert stream.history(0) == (limit - 101 + 27, limit - 101 + 50)
    finally:
        batch.close()


def test_refused_calls_leave_state_and_history_untouched(apd, ctx):
    queries, streams = small_case(seed=45)
    model = Model(queries, streams, UNIT)
    batch = make_batch(ctx, queries)
    other = apd.Context(0)
    try:
        with HistoryStream(apd, ctx, batch, [0, 1], UNIT, 2) as stream:
            assert stream.keep(24) == apd.APD_OK
            model.keep(24)
            push_and_check(stream, model, (30, 20), "before")
            L, bad = apd.lib(), apd.APD_ERR_INVALID_ARG
            assert L.apd_spot_stream_keep(other.handle, stream.handle, 5) == bad                     # a foreign context
            for r in ((2, 0, 30, 30), (0, 2, 30, 30), (0, 0, 31, 31), (0, 0, 20, 21), (0, 1, 21, 21)):
                assert stream.paths_status([(0, 0, 30, 29), r], model.lens)[0] == bad, r
            status, _, _, _ = stream.push_status([streams[0][30:], streams[1][20:]], short=1)
            assert status == bad
            win = np.zeros(1, dtype=ref.WINDOW)
            off = np.zeros(2, dtype=np.uint64)
            assert L.apd_spot_stream_paths(other.handle, stream.handle, win.ctypes.data_as(C.POINTER(apd.SpotWindow)), 1, None, 0,
                                           off.ctypes.data_as(C.POINTER(C.c_uint64)), None, None, None) == bad
            check(stream, model, "after the refusals")
            push_and_check(stream, model, (20, 13), "and on")
    finally:
        other.close()
        batch.close()


def test_a_small_workspace_cap_gives_identical_results(apd, ctx):
    queries, streams = small_case(seed=46)
    model = Model(queries, streams, SKEWED)
    batch = make_batch(ctx, queries)
    try:
        with HistoryStream(apd, ctx, batch, [0, 1], SKEWED, 2) as stream:
            assert stream.keep(24) == apd.APD_OK
            model.keep(24)
            push_and_check(stream, model, (50, 33), "whole")
            _, (paths, found, scores) = check(stream, model, "default cap")
            os.environ["APD_SPOT_WORKSPACE_BYTES"] = "4096"                                           # a few windows per chunk
            try:
                _, (paths2, found2, scores2) = check(stream, model, "small cap")
            finally:
                os.environ.pop("APD_SPOT_WORKSPACE_BYTES", None)
            assert all(ref.same_steps(a, b) for a, b in zip(paths, paths2))
            assert np.array_equal(found, found2) and np.array_equal(scores.view(np.uint32), scores2.view(np.uint32))
    finally:
        batch.close()


def test_two_branch_words_per_lane(apd, ctx, capfd):
    rng = np.random.default_rng(47)
    queries = [rng.standard_normal((1030, 13)).astype(F)]      # R = 17 rows per lane: two words per lane and macro-step
    streams = [rng.standard_normal((70, 13)).astype(F)]
    model = Model(queries, streams, UNIT)
    batch = make_batch(ctx, queries)
    try:
        with HistoryStream(apd, ctx, batch, [0], UNIT, 1) as stream:
            assert stream.keep(24) == apd.APD_OK
            model.keep(24)
            with kt.debug_plan(capfd) as err:
                traced = sum(push_and_check_count(stream, model, sizes) for sizes in ((30,), (1,), (39,)))
            assert set(kt.read_spot_plan(err[0])) == {("streamrec", 0, 13)}
            assert traced >= 1
    finally:
        batch.close()


def push_and_check_count(stream, model, sizes):
    chunks = [y[p:p + s] for y, p, s in zip(model.streams, model.pushed, sizes)]
    stream.push(chunks)
    model.pushed = [p + s for p, s in zip(model.pushed, sizes)]
    return check(stream, model, "R = 17 %s" % (sizes,))[0]


def test_hand_case_one_column_at_a_time(apd, ctx):
    """include/apd.h: x = [0, 1], y = [0, 1, 0]: window (3, 2) costs 2.0 in the table (columns 2 .. 3 alone would give 1.0); with
    H = 2 it is traced, and one more column later it has aged out.  Through the Python session as well."""
    from audio_pattern_discovery_amd.alignments import AlignmentWorkers, NDSequence, SPOT_WINDOW
    from audio_pattern_discovery_amd.discovery import Discovery
    x, y = np.array([[0], [1]], dtype=F), np.array([[0], [1], [0]], dtype=F)
    batch = make_batch(ctx, [x])
    try:
        with HistoryStream(apd, ctx, batch, [0], UNIT, 1) as stream:
            assert stream.keep(2) == apd.APD_OK
            for k in range(3):
                stream.push([y[k:k + 1]])
            (steps,), found, scores = stream.paths([(0, 0, 3, 2)], [2])
            assert [(int(s["i"]), int(s["j"]), float(s["cost"]), int(s["op"])) for s in steps][-1][:3] == (2, 3, 2.0)
            assert int(steps[0]["op"]) == ref.START and found[0] == 2 and scores[0] == F(2.0) / F(4.0)
            stream.push([y[:1]])
            (steps,), found, scores = stream.paths([(0, 0, 3, 2)], [2])
            assert len(steps) == 0 and found[0] == 2 and scores[0] == F(2.0) / F(4.0) and stream.history(0) == (3, 4)
    finally:
        batch.close()
    workers = AlignmentWorkers.new([NDSequence(x)], ctx)
    session = workers.spot_stream([0], Discovery(), channels=1, history=2)
    try:
        for k in range(3):
            session.push([y[k:k + 1]])
        assert session.history(0) == (2, 3)
        win = np.array([(0, 0, 3, 2)], dtype=SPOT_WINDOW)
        (steps,), found, scores = session.paths(win)
        assert float(steps[-1]["cost"]) == 2.0 and found[0] == 2
        session.keep(0)
        assert session.history(0) == (4, 3)
    finally:
        session.close()
        workers.close()
