"""GPU tests of the warping paths of spotted windows (apd_spot_paths) against the checker tests/_spot_path_reference.py.

Every comparison is bitwise: i, j and op equal, the costs and scores equal as uint32 (NaN payloads aside: _path_reference.bits says
why).  Shapes are the smallest that reach each path of the kernels (csrc/dtw_spot_path.hip, csrc/dtw_spot_sweep.h): R = 1 .. 3 rows
per lane in registers with the last lane full, one row over and one lane over, R = 5 in LDS, R = 18 with two branch words per
lane, streams shorter than one wavefront, every kind of frame dimension, window lists that merge into one interval or stay apart,
and a list cut into one chunk per window."""
import ctypes as C
import os

import numpy as np
import pytest

import _kernel_table as kt
import _spot_path_reference as ref
import _spot_reference as spot_ref

pytestmark = pytest.mark.gpu
UNIT = (1.0, 1.0, 1.0)
SKEWED = (1.0, 2.0, 0.5)                        # (insertion, deletion, match)
F = np.float32
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
    return apd.AlignConfig(float("nan"), pen[0], pen[1], pen[2])                  # the band percentage is not read


def windows_of(records):
    """[(x, y, end, start), ...] as a WINDOW array."""
    return np.array([tuple(int(v) for v in r) for r in records], dtype=ref.WINDOW).reshape(-1)


def raw_paths(apd, ctx, batch, pen, records):
    """apd_spot_paths through ctypes: (list of STEP arrays, found_start, scores).  Checks the size query against the bound, that
    the unused slots are zero and that nothing is written past the capacity."""
    L = apd.lib()
    cfg = config(apd, pen)
    win = windows_of(records)
    k = len(win)
    u32p, u64p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_float)
    head = (ctx.handle, batch.handle, C.byref(cfg), win.ctypes.data_as(C.POINTER(apd.SpotWindow)), k)
    off = np.full(k + 1, 77, dtype=np.uint64)
    apd.check(L.apd_spot_paths(*head, None, 0, off.ctypes.data_as(u64p), None, None, None), ctx.handle)          # sizes only
    total = int(off[-1])
    steps = np.full((total + 1) * 16, 0x55, dtype=np.uint8).view(ref.STEP)                                       # one slot more: a canary
    lens, found = np.full(k + 1, CANARY, dtype=np.uint32), np.full(k + 1, CANARY, dtype=np.uint32)
    scores = np.full(k + 1, CANARY, dtype=np.uint32).view(F)
    off2 = np.zeros(k + 1, dtype=np.uint64)
    apd.check(L.apd_spot_paths(*head, steps.ctypes.data_as(C.POINTER(apd.PathStep)), total, off2.ctypes.data_as(u64p),
                               lens.ctypes.data_as(u32p), found.ctypes.data_as(u32p), scores.ctypes.data_as(f32p)), ctx.handle)
    assert np.array_equal(off, off2)
    assert steps[-1]["op"] == CANARY and lens[-1] == CANARY and found[-1] == CANARY and scores.view(np.uint32)[-1] == CANARY
    paths = []
    for p in range(k):
        lo, hi = int(off[p]), int(off[p + 1])
        assert lens[p] <= hi - lo and not steps[lo + int(lens[p]):hi].view(np.uint32).any()                      # unused slots are zeroed
        paths.append(steps[lo:lo + int(lens[p])].copy())
    return paths, found[:k].copy(), scores[:k].copy()


def raw_curves(apd, ctx, batch, pen, pairs):
    """apd_spot's (cost, start) per pair."""
    L = apd.lib()
    cfg = config(apd, pen)
    pr = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
    u32p, u64p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_float)
    head = (ctx.handle, batch.handle, C.byref(cfg), pr.ctypes.data_as(u32p), len(pr))
    off = np.zeros(len(pr) + 1, dtype=np.uint64)
    apd.check(L.apd_spot(*head, None, None, 0, off.ctypes.data_as(u64p), None), ctx.handle)
    cost, start = np.zeros(int(off[-1]), dtype=F), np.zeros(int(off[-1]), dtype=np.uint32)
    apd.check(L.apd_spot(*head, cost.ctypes.data_as(f32p), start.ctypes.data_as(u32p), len(cost), off.ctypes.data_as(u64p), None), ctx.handle)
    return [(cost[int(off[p]):int(off[p + 1])], start[int(off[p]):int(off[p + 1])]) for p in range(len(pr))]


_TABLES = {}


def table(key, seqs, pen, x, y):
    """The checker's table of query x against stream y of `seqs`, computed once per (key, penalties, pair)."""
    k = (key, pen, x, y)
    if k not in _TABLES:
        _TABLES[k] = ref.table(seqs[x], seqs[y], *pen)
    return _TABLES[k]


def assert_window(got, key, seqs, pen, record, what=""):
    """One window's (steps, found_start, score) against the checker's answer."""
    x, y, end, start = (int(v) for v in record)
    steps, found, score = got
    want_steps, want_found, want_score = ref.answer(table(key, seqs, pen, x, y), len(seqs[x]), end, start)
    what = "%s %s window %s" % (key, what, (x, y, end, start))
    assert int(found) == want_found, what
    assert ref.bits([score])[0] == ref.bits([want_score])[0], what
    assert ref.same_steps(steps, want_steps), what


def check_windows(apd, ctx, key, seqs, pen, records, batch=None):
    own = batch is None
    batch = batch or make_batch(ctx, seqs)
    try:
        paths, found, scores = raw_paths(apd, ctx, batch, pen, records)
    finally:
        if own:
            batch.close()
    for p, record in enumerate(records):
        assert_window((paths[p], found[p], scores[p]), key, seqs, pen, record)
    return paths, found, scores


def curve_windows(apd, ctx, seqs, pen, pairs, ends_of, batch=None):
    """[(x, y, end, S[n][end])] for the ends ends_of(m) of every pair, the starts from apd_spot's curves."""
    own = batch is None
    batch = batch or make_batch(ctx, seqs)
    try:
        curves = raw_curves(apd, ctx, batch, pen, pairs)
    finally:
        if own:
            batch.close()
    return [(x, y, end, int(start[end - 1])) for (x, y), (_, start) in zip(pairs, curves) for end in ends_of(len(seqs[y]))]


def gauss_seqs(lengths, dim, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((n, dim)).astype(F) for n in lengths]


def integer_seqs(lengths, dim, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 3, (n, dim)).astype(F) for n in lengths]


def col(values):
    return np.array(values, dtype=F).reshape(-1, 1)


def as_tuples(steps):
    return [(int(s["i"]), int(s["j"]), float(s["cost"]), int(s["op"])) for s in steps]


M, I, D, S = ref.MATCH, ref.INSERT, ref.DELETE, ref.START
HAND = ((col([1, 2]), col([5, 1, 2, 5]), [1, 2, 2, 2],
         [[(0, 0, 0.0, S), (1, 1, 4.0, M), (2, 1, 7.0, I)], [(0, 1, 0.0, S), (1, 2, 0.0, M), (2, 2, 1.0, I)],
          [(0, 1, 0.0, S), (1, 2, 0.0, M), (2, 3, 0.0, M)], [(0, 1, 0.0, S), (1, 2, 0.0, M), (2, 3, 0.0, M), (2, 4, 3.0, D)]]),
        (col([0, 1]), col([0, 1, 0]), [1, 1, 2],                                   # the tie quirk: (2, 3) takes MATCH although larger
         [[(0, 0, 0.0, S), (1, 1, 0.0, M), (2, 1, 1.0, I)], [(0, 0, 0.0, S), (1, 1, 0.0, M), (2, 2, 0.0, M)],
          [(0, 1, 0.0, S), (1, 2, 1.0, M), (2, 3, 2.0, M)]]))


def test_hand_cases_through_both_entry_points(apd, ctx):
    from audio_pattern_discovery_amd.alignments import SPOT_BEST, AlignmentWorkers, NDSequence
    from audio_pattern_discovery_amd.discovery import Discovery
    for x, y, starts, want in HAND:
        records = [(0, 1, end, starts[end - 1]) for end in range(1, len(y) + 1)]
        paths, found, scores = check_windows(apd, ctx, "hand%d" % len(y), [x, y], UNIT, records)
        assert [as_tuples(p) for p in paths] == want and found.tolist() == starts
        workers = AlignmentWorkers.new([NDSequence(x), NDSequence(y)], ctx)
        try:
            curves, _ = workers.spot([(0, 1)], Discovery())
            cost, start = curves[0]
            asked = np.zeros(len(y), dtype=SPOT_BEST)
            asked["end"], asked["start"] = np.arange(1, len(y) + 1), start
            mine, mine_found, mine_scores = workers.spot_paths([(0, 1)] * len(y), asked, Discovery())
        finally:
            workers.close()
        assert [as_tuples(p) for p in mine] == want and mine_found.tolist() == starts
        assert np.array_equal(mine_scores.view(np.uint32), scores.view(np.uint32))
        assert [float(p["cost"][-1]) for p in mine] == cost.tolist()                 # the last step's cost is the curve's


QUERY_LENGTHS = (1, 2, 63, 64, 65, 128, 130)      # R = 1, 2, 3 rows per lane; last lane full, one row over, one lane over
LDS_QUERY_LENGTHS = (257, 300)                    # R = 5: the lane columns in LDS
STREAM_LENGTHS = (1, 2, 63, 64, 65, 200)


def edge_ends(m):
    return range(1, m + 1) if m <= 65 else (1, 2, 63, 64, 65, 128, m)


def check_edges(apd, ctx, key, queries, dim, seed):
    seqs = gauss_seqs(tuple(queries) + STREAM_LENGTHS, dim, seed)
    nq = len(queries)
    pairs = [(q, nq + s) for q in range(nq) for s in range(len(STREAM_LENGTHS))]
    batch = make_batch(ctx, seqs)
    try:
        records = curve_windows(apd, ctx, seqs, UNIT, pairs, edge_ends, batch=batch)
        assert len(records) == nq * sum(len(edge_ends(m)) for m in STREAM_LENGTHS) and all(r[3] >= 1 for r in records)
        check_windows(apd, ctx, key, seqs, UNIT, records, batch=batch)
    finally:
        batch.close()


def test_lane_and_row_block_edges_in_registers(apd, ctx, capfd):
    with kt.debug_plan(capfd) as err:
        check_edges(apd, ctx, "edges", QUERY_LENGTHS, 13, 301)
    assert set(kt.read_spot_plan(err[0])) == {(kind, rt, 13) for kind in kt.SPOT_KINDS for rt in (1, 2, 3)}, err[0]


def test_lane_and_row_block_edges_in_lds(apd, ctx, capfd):
    with kt.debug_plan(capfd) as err:
        check_edges(apd, ctx, "edges-lds", LDS_QUERY_LENGTHS, 13, 302)
    assert set(kt.read_spot_plan(err[0])) == {("sweep", 0, 13), ("record", 0, 13)}, err[0]


def test_two_branch_words_per_lane(apd, ctx, capfd):
    with kt.debug_plan(capfd) as err:
        check_edges(apd, ctx, "edges-wpl2", (1100,), 13, 303)                       # R = 18 in LDS: WPL = 2
    assert {(v["kind"], v["rt"], v["d"], v["r_max"]) for v in kt.read_spot_launches(err[0])} == {("sweep", 0, 13, 18), ("record", 0, 13, 18)}


def test_dimension_without_kernels_of_its_own(apd, ctx, capfd):
    """A dimension above the largest kernel dimension runs <0, 0>: frames re-read per cell, R = 3 rows per lane in LDS.  A small one
    does not: dim = 5 is made resident as kernel_dim(5) = 8 and runs <3, 8>, everything in registers."""
    top = max(kt.parse_dims(kt.header_text()))
    for dim, kernel, seed in ((top + 5, (0, 0), 305), (5, (3, kt.kernel_dim(5)), 304)):
        assert kt.spot_row_class(kt.kernel_dim(dim), 130) == kernel[0]
        seqs = gauss_seqs((130, 100), dim, seed)
        with kt.debug_plan(capfd) as err:
            records = curve_windows(apd, ctx, seqs, SKEWED, [(0, 1)], lambda m: range(1, m + 1))
            paths, _, _ = check_windows(apd, ctx, "dim%d" % dim, seqs, SKEWED, records)
        assert kt.read_spot_plan(err[0]) == {("sweep",) + kernel: 1, ("record",) + kernel: 1}, err[0]
        if kernel == (0, 0):
            assert {(v["r_max"], v["lds"]) for v in kt.read_spot_launches(err[0])} == {(3, 3 * 64 * 8)}
        assert len(paths) == 100 and all(len(p) > 130 for p in paths)


@pytest.mark.parametrize("dim", [3, 8, 13, 16, 40])
@pytest.mark.parametrize("pen", [UNIT, SKEWED])
def test_dimensions(apd, ctx, dim, pen):
    seqs = gauss_seqs((65, 100), dim, 310 + dim)
    records = curve_windows(apd, ctx, seqs, pen, [(0, 1)], lambda m: range(1, m + 1))
    paths, _, _ = check_windows(apd, ctx, "dim%d" % dim, seqs, pen, records)
    assert len(paths) == 100 and all(len(p) > 65 for p in paths)


@pytest.mark.parametrize("dim", [1, 13])
@pytest.mark.parametrize("pen", [UNIT, SKEWED])
def test_integer_ties(apd, ctx, dim, pen):
    seqs = integer_seqs((65, 100), dim, 320 + dim)
    records = curve_windows(apd, ctx, seqs, pen, [(0, 1)], lambda m: range(1, m + 1))
    paths, _, _ = check_windows(apd, ctx, "ties%d" % dim, seqs, pen, records)
    assert len(paths) == 100 and len({len(p) for p in paths}) > 1


def test_consistency_with_spot_at_a_size_the_checker_cannot_afford(apd, ctx):
    from audio_pattern_discovery_amd import synth
    from audio_pattern_discovery_amd.alignments import SPOT_BEST, AlignmentWorkers, NDSequence, spot_hits
    from audio_pattern_discovery_amd.discovery import Discovery
    n, m, dim = 1100, 3000, 13
    rng = np.random.default_rng(330)
    frames, offsets = synth.make_sequences(1, n, dim, seed=330, jitter=0)
    query = np.ascontiguousarray(synth.split(frames, offsets)[0])
    assert len(query) == n
    warped = synth._warp_copy(rng, query, 900)
    noise = [rng.standard_normal((k, dim)).astype(F) for k in (200, 300, m - n - 900 - 500)]
    stream = np.concatenate([noise[0], query, noise[1], warped, noise[2]], axis=0).astype(F)
    assert len(stream) == m
    pen = Discovery()
    penalties = (pen.insertion_penalty, pen.deletion_penalty, pen.match_penalty)
    workers = AlignmentWorkers.new([NDSequence(query), NDSequence(stream)], ctx)
    try:
        curves, best = workers.spot([(0, 1)], pen)
        cost, start = curves[0]
        all_scores = spot_ref.scores(cost, start, n)
        hits = spot_hits(cost, start, n, float(np.median(all_scores[np.isfinite(all_scores)])))
        asked = np.concatenate([hits, best]).astype(SPOT_BEST)
        assert len(hits) >= 2 and best[0]["score"] == 0.0 and int(best[0]["end"]) == 200 + n      # the embedded copy itself
        paths, found, scores = workers.spot_paths([(0, 1)] * len(asked), asked, pen)
    finally:
        workers.close()
    assert np.array_equal(found, asked["start"])
    assert np.array_equal(scores.view(np.uint32), asked["score"].view(np.uint32))
    moves = {M: (1, 1), I: (1, 0), D: (0, 1)}
    for steps, w in zip(paths, asked):
        end, first = int(w["end"]), int(w["start"])
        assert steps[0]["op"] == S and steps[0]["i"] == 0 and steps[0]["cost"] == 0.0
        assert (int(steps[1]["i"]), int(steps[1]["j"])) == (1, first) and steps[1]["op"] in (M, I)
        assert (int(steps[-1]["i"]), int(steps[-1]["j"])) == (n, end)
        assert max(n, end - first + 1) + 1 <= len(steps) <= n + end - first + 1
        di = np.diff(steps["i"].astype(np.int64))
        dj = np.diff(steps["j"].astype(np.int64))
        assert all((a, b) == moves[int(op)] for a, b, op in zip(di, dj, steps["op"][1:]))
        assert steps["cost"][-1:].view(np.uint32)[0] == cost[end - 1:end].view(np.uint32)[0]
        assert np.array_equal(ref.bits(ref.replay(query, stream, steps, *penalties)), ref.bits(steps["cost"]))
    exact = paths[-1]                                                                # the copy: the diagonal, cost 0 all along
    assert len(exact) == n + 1 and not exact["cost"].any() and np.all(exact["op"][1:] == M)


@pytest.fixture(scope="module")
def listed(apd, ctx):
    """Two templates and two recordings, the curves of two pairs, and a window list with every relation between windows."""
    templates, streams = gauss_seqs((20, 66), 13, 340), gauss_seqs((90, 130), 13, 341)
    seqs = templates + streams
    batch = make_batch(ctx, seqs)
    try:
        (_, s_a), (_, s_b) = raw_curves(apd, ctx, batch, UNIT, [(1, 3), (0, 2)])
    finally:
        batch.close()
    m = len(seqs[3])

    def at(end):
        return (1, 3, end, int(s_a[end - 1]))

    c = 100
    b = int(s_a[c - 1]) - 1                                                        # [S(b), b] touches [b + 1, c]
    assert b >= 2
    records = [at(m), at(c), at(c), at(c - 1), at(b), at(c + 9), (0, 2, 90, int(s_b[89])), at(1), (0, 2, 45, int(s_b[44])),
               at(c - 3), (0, 0, 0, 0), at(30), at(2)]
    records.sort(key=lambda r: -r[2])                                              # descending end
    assert records[0][2] == m and at(1)[3] == 1 and at(c - 1)[3] < c - 3                # windows of neighbouring ends overlap
    return templates, streams, seqs, records


def test_window_list_semantics_in_a_joined_batch(apd, ctx, listed):
    from audio_pattern_discovery_amd.alignments import Batch
    templates, streams, seqs, records = listed
    a, b = make_batch(ctx, templates), make_batch(ctx, streams)
    joined = Batch.join(a, b)
    try:
        paths, found, scores = check_windows(apd, ctx, "listed", seqs, UNIT, records, batch=joined)
        for p, record in enumerate(records):                                       # the same windows asked one per call
            one, one_found, one_score = raw_paths(apd, ctx, joined, UNIT, [record])
            assert ref.same_steps(one[0], paths[p]) and one_found[0] == found[p]
            assert one_score.view(np.uint32)[0] == scores.view(np.uint32)[p]
    finally:
        joined.close()
        a.close()
        b.close()
    twice = [p for p, r in enumerate(records) if r == records[[r[2] for r in records].index(100)]]
    assert len(twice) == 2 and ref.same_steps(paths[twice[0]], paths[twice[1]])


def test_chunked_equals_unchunked(apd, ctx, listed):
    _, _, seqs, records = listed
    batch = make_batch(ctx, seqs)
    try:
        whole = raw_paths(apd, ctx, batch, UNIT, records)
        os.environ["APD_SPOT_WORKSPACE_BYTES"] = "1"                               # every window a chunk of its own
        try:
            ones = raw_paths(apd, ctx, batch, UNIT, records)
            os.environ["APD_SPOT_WORKSPACE_BYTES"] = str(40 * 1024)               # a few windows per chunk
            some = raw_paths(apd, ctx, batch, UNIT, records)
        finally:
            del os.environ["APD_SPOT_WORKSPACE_BYTES"]
    finally:
        batch.close()
    for other in (ones, some):
        assert all(ref.same_steps(p, q) for p, q in zip(other[0], whole[0]))
        assert np.array_equal(other[1], whole[1]) and np.array_equal(other[2].view(np.uint32), whole[2].view(np.uint32))
    for p, record in enumerate(records):
        assert_window((ones[0][p], ones[1][p], ones[2][p]), "listed", seqs, UNIT, record)


def test_wrong_and_absent_starts(apd, ctx):
    seqs = gauss_seqs((70, 150), 13, 350)
    batch = make_batch(ctx, seqs)
    try:
        (cost, start), = raw_curves(apd, ctx, batch, UNIT, [(0, 1)])
        scores = spot_ref.scores(cost, start, 70)
        ends = [e for e in (40, 100, 150) if start[e - 1] > 1]
        assert ends
        wrong = [(0, 1, e, int(start[e - 1]) + 1) for e in ends] + [(0, 1, e, int(start[e - 1]) - 1) for e in ends] + [(0, 0, 0, 0), (0, 1, 0, 5), (0, 1, 7, 0)]
        paths, found, got_scores = check_windows(apd, ctx, "wrong", seqs, UNIT, wrong, batch=batch)
        assert all(len(p) == 0 for p in paths)
        k = 2 * len(ends)
        assert found[:k].tolist() == [int(start[e - 1]) for e in ends] * 2 and not found[k:].any()
        assert np.array_equal(got_scores[:k].view(np.uint32), np.array([scores[e - 1] for e in ends] * 2, dtype=F).view(np.uint32))
        assert np.all(np.isposinf(got_scores[k:]))
        again = [(0, 1, e, int(f)) for e, f in zip(ends, found)]                   # asked again with found_start, the path comes
        paths, _, _ = check_windows(apd, ctx, "wrong", seqs, UNIT, again, batch=batch)
        assert all(len(p) > 70 for p in paths)
    finally:
        batch.close()


def test_nan_tables(apd, ctx):
    seqs = gauss_seqs((6, 40), 13, 351)
    seqs[1][0, :] = np.nan                                                         # column 1: rows >= 2 take MATCH from column 0, S = 0
    seqs[1][25, 2] = np.nan
    cost, start = spot_ref.curves(seqs[0], seqs[1])
    through_0 = [e for e in range(1, 41) if start[e - 1] == 0]
    nan_with_start = [e for e in range(1, 41) if start[e - 1] >= 1 and np.isnan(cost[e - 1])]
    assert 1 in through_0 and nan_with_start
    batch = make_batch(ctx, seqs)
    try:
        (got_cost, got_start), = raw_curves(apd, ctx, batch, UNIT, [(0, 1)])
        assert np.array_equal(got_start, start) and np.array_equal(ref.bits(got_cost), ref.bits(cost))
        records = [(0, 1, e, 1) for e in through_0] + [(0, 1, e, 0) for e in through_0] + [(0, 1, e, int(start[e - 1])) for e in range(1, 41)]
        paths, found, _ = check_windows(apd, ctx, "nan", seqs, UNIT, records, batch=batch)
    finally:
        batch.close()
    k = len(through_0)
    assert all(len(p) == 0 for p in paths[:2 * k]) and not found[:2 * k].any()
    for e in nan_with_start:
        steps = paths[2 * k + e - 1]
        assert len(steps) > 6 and steps[0]["op"] == S and np.isnan(steps["cost"][-1])   # a complete path with NaN costs


def test_modes_refill_and_timing(apd, ctx):
    lengths = (30, 150, 300, 120, 95)
    seqs, fresh = gauss_seqs(lengths, 13, 360), gauss_seqs(lengths, 13, 361)
    pairs = [(0, 3), (1, 4), (2, 3)]

    def ends(m):
        return (1, m // 2, m)

    batch = make_batch(ctx, seqs)
    try:
        records = curve_windows(apd, ctx, seqs, UNIT, pairs, ends, batch=batch)
        results = []
        try:
            for mode in (0, 1, 2):
                ctx.set_distance_mode(mode)
                results.append(raw_paths(apd, ctx, batch, UNIT, records))
        finally:
            ctx.set_distance_mode("hybrid")
        for p, record in enumerate(records):
            assert_window((results[0][0][p], results[0][1][p], results[0][2][p]), "modes", seqs, UNIT, record)
        for other in results[1:]:
            assert all(ref.same_steps(p, q) for p, q in zip(other[0], results[0][0]))
            assert np.array_equal(other[1], results[0][1]) and np.array_equal(other[2].view(np.uint32), results[0][2].view(np.uint32))
        ctx.set_timing(True)
        try:
            raw_paths(apd, ctx, batch, UNIT, records)
            assert ctx.last_kernel_ms() > 0.0
        finally:
            ctx.set_timing(False)
        frames = np.ascontiguousarray(np.concatenate(fresh, axis=0))
        apd.check(apd.lib().apd_batch_refill(ctx.handle, batch.handle, C.c_void_p(frames.ctypes.data), 0), ctx.handle)
        after = curve_windows(apd, ctx, fresh, UNIT, pairs, ends, batch=batch)
        paths, _, _ = check_windows(apd, ctx, "refilled", fresh, UNIT, after, batch=batch)
        assert paths[-1].tobytes() != results[0][0][-1].tobytes()
    finally:
        batch.close()


def test_size_query_and_argument_errors(apd, ctx):
    from audio_pattern_discovery_amd.alignments import Batch
    L = apd.lib()
    seqs = gauss_seqs((12, 40, 25), 13, 370)
    batch = make_batch(ctx, seqs)
    cfg = config(apd, UNIT)
    u32p, u64p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_float)
    winp, stepp = C.POINTER(apd.SpotWindow), C.POINTER(apd.PathStep)
    (_, s_a), (_, s_b) = raw_curves(apd, ctx, batch, UNIT, [(0, 1), (0, 2)])
    win = windows_of([(0, 1, 40, s_a[39]), (0, 0, 0, 0), (0, 2, 9, s_b[8]), (0, 1, 5, 0)])
    sizes = [0, 12 + 40 - int(s_a[39]) + 1, 0, 12 + 9 - int(s_b[8]) + 1, 0]
    want_off = np.cumsum(sizes).tolist()
    total = want_off[-1]
    off = np.zeros(5, dtype=np.uint64)
    steps = np.full(total * 16, 0x55, dtype=np.uint8).view(ref.STEP)
    lens, found = np.full(4, CANARY, dtype=np.uint32), np.full(4, CANARY, dtype=np.uint32)
    scores = np.full(4, CANARY, dtype=np.uint32).view(F)
    offp, lenp, foundp, scorep, stepsp = (off.ctypes.data_as(u64p), lens.ctypes.data_as(u32p), found.ctypes.data_as(u32p),
                                          scores.ctypes.data_as(f32p), steps.ctypes.data_as(stepp))
    head = (ctx.handle, batch.handle, C.byref(cfg))

    def call(w, *rest):
        return L.apd_spot_paths(*head, w.ctypes.data_as(winp), len(w), *rest)

    def untouched():
        return (not ctx.stream_busy() and np.all(steps.view(np.uint32) == CANARY) and np.all(lens == CANARY) and np.all(found == CANARY)
                and np.all(scores.view(np.uint32) == CANARY))

    try:
        ctx.synchronize()
        assert call(win, None, 0, offp, None, None, None) == apd.APD_OK and off.tolist() == want_off and untouched()   # the size query
        assert call(win, stepsp, total - 1, offp, lenp, foundp, scorep) == apd.APD_ERR_INVALID_ARG and untouched()    # capacity one short
        assert call(win, stepsp, total, None, lenp, foundp, scorep) == apd.APD_ERR_INVALID_ARG and untouched()
        assert call(win, stepsp, total, offp, None, foundp, scorep) == apd.APD_ERR_INVALID_ARG and untouched()
        assert L.apd_spot_paths(*head, None, 4, stepsp, total, offp, lenp, foundp, scorep) == apd.APD_ERR_INVALID_ARG and untouched()
        for bad in ((3, 1, 5, 1), (0, 3, 5, 1), (0, 1, 5, 6), (0, 1, 41, 3), (0, 2, 26, 26)):                           # index = n_seq, start > end, end > m
            w = win.copy()
            w[2] = bad
            assert call(w, stepsp, total, offp, lenp, foundp, scorep) == apd.APD_ERR_INVALID_ARG and untouched(), bad
        assert L.apd_spot_paths(*head, None, 0, stepsp, 0, offp, lenp, foundp, scorep) == apd.APD_OK and off[0] == 0 and untouched()
        assert call(win, stepsp, total, offp, lenp, None, None) == apd.APD_OK                                           # found_start and scores may be NULL
        assert lens[1] == 0 and lens[3] == 0 and lens[0] > 12 and lens[2] > 12
        assert np.all(found == CANARY) and np.all(scores.view(np.uint32) == CANARY)
        assert call(win, stepsp, total, offp, lenp, foundp, scorep) == apd.APD_OK
        assert found.tolist() == [int(s_a[39]), 0, int(s_b[8]), 0] and np.isposinf(scores[1]) and np.isposinf(scores[3])
    finally:
        batch.close()
    # an empty sequence in the batch, a query beyond the documented limit: refused before anything is launched
    frames = np.zeros((16385 + 5, 1), dtype=F)
    empty = Batch(ctx, frames[:9], np.array([0, 4, 4, 9], dtype=np.uint64), 1)
    long_ = Batch(ctx, frames, np.array([0, 16385, 16390], dtype=np.uint64), 1)
    steps = np.full(16400 * 16, 0x55, dtype=np.uint8).view(ref.STEP)
    stepsp = steps.ctypes.data_as(stepp)
    try:
        ctx.synchronize()
        one = windows_of([(0, 2, 3, 1)])
        rest = (stepsp, len(steps), offp, lenp, foundp, scorep)
        lens[:], found[:] = CANARY, CANARY
        scores.view(np.uint32)[:] = CANARY
        assert L.apd_spot_paths(ctx.handle, empty.handle, C.byref(cfg), one.ctypes.data_as(winp), 1, *rest) == apd.APD_ERR_EMPTY_SEQUENCE and untouched()
        one = windows_of([(0, 1, 3, 1)])
        assert L.apd_spot_paths(ctx.handle, long_.handle, C.byref(cfg), one.ctypes.data_as(winp), 1, *rest) == apd.APD_ERR_UNSUPPORTED and untouched()
        one = windows_of([(1, 0, 16385, 16381)])                                                                        # the other way round runs
        assert L.apd_spot_paths(ctx.handle, long_.handle, C.byref(cfg), one.ctypes.data_as(winp), 1, *rest) == apd.APD_OK
        assert lens[0] == 6 and found[0] == 16381 and scores[0] == 0.0                                                  # all-zero frames: exact ties, MATCH all along
    finally:
        empty.close()
        long_.close()
