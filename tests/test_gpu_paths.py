"""GPU tests of the warping paths (apd_align_paths, apd_align_pair_path) against the checker tests/_path_reference.py.

Every comparison is bitwise: i, j and op equal, cost and score equal as uint32 (NaN payloads aside: _path_reference.bits says why).
Shapes are the smallest that reach each code path of the two kernels (csrc/dtw_path.hip): C = 2 cells per lane with one direction
word, C >= 3, more than one direction word per lane (2w+1 > 1024), a DP row beyond 64 KB of LDS (2w+1 > 16384), bands that bind,
widen (|n-m| > band) and vanish (band 0), lengths 1 and 2, and a pair list cut into several workspace chunks."""
import ctypes as C
import os

import numpy as np
import pytest

import _path_reference as ref

pytestmark = pytest.mark.gpu
UNIT = (1.0, 1.0, 1.0)
SKEWED = (1.5, 0.75, 1.25)                      # (insertion, deletion, match)


@pytest.fixture(scope="module")
def ctx(apd):
    c = apd.Context(0)
    yield c
    c.close()


def make_batch(ctx, seqs):
    from audio_pattern_discovery_amd.alignments import Batch
    seqs = [np.ascontiguousarray(s, dtype=np.float32) for s in seqs]
    offsets = np.zeros(len(seqs) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(s) for s in seqs])
    return Batch(ctx, np.concatenate(seqs, axis=0), offsets, seqs[0].shape[1])


def raw_paths(apd, ctx, batch, pct, pen, pairs):
    """apd_align_paths through ctypes: (list of step arrays, scores, step_off)."""
    L = apd.lib()
    cfg = apd.AlignConfig(pct, pen[0], pen[1], pen[2])
    pr = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
    n_pairs = len(pr)
    u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    off = np.full(n_pairs + 1, 77, dtype=np.uint64)
    apd.check(L.apd_align_paths(ctx.handle, batch.handle, C.byref(cfg), pr.ctypes.data_as(u32p), n_pairs, None, 0,
                                off.ctypes.data_as(u64p), None, None), ctx.handle)
    steps = np.full((int(off[-1]) + 1) * 16, 0x55, dtype=np.uint8).view(ref.STEP)          # one slot more than asked: a canary
    lens = np.zeros(n_pairs, dtype=np.uint32)
    scores = np.zeros(n_pairs, dtype=np.float32)
    off2 = np.zeros(n_pairs + 1, dtype=np.uint64)
    apd.check(L.apd_align_paths(ctx.handle, batch.handle, C.byref(cfg), pr.ctypes.data_as(u32p), n_pairs,
                                steps.ctypes.data_as(C.POINTER(apd.PathStep)), int(off[-1]), off2.ctypes.data_as(u64p),
                                lens.ctypes.data_as(u32p), scores.ctypes.data_as(C.POINTER(C.c_float))), ctx.handle)
    assert np.array_equal(off, off2)
    assert steps[-1]["i"] == 0x55555555 and steps[-1]["op"] == 0x55555555                      # nothing written past the capacity
    out = []
    for p in range(n_pairs):
        lo, hi = int(off[p]), int(off[p + 1])
        assert lens[p] <= hi - lo
        assert not steps[lo + int(lens[p]):hi].view(np.uint32).any()                           # unused slots are zeroed
        out.append(steps[lo:lo + int(lens[p])].copy())
    return out, scores, off


_REFERENCE = {}


def reference(key, seqs, pct, pen, x, y):
    """The checker's (steps, score) of the ordered pair (x, y) of `seqs`, computed once per (key, band, penalties, pair)."""
    k = (key, pct, pen, x, y)
    if k not in _REFERENCE:
        band = ref.band_from_pct(pct, max(len(seqs[x]), len(seqs[y])))
        _REFERENCE[k] = ref.path(seqs[x], seqs[y], band, *pen)
    return _REFERENCE[k]


def assert_same_path(got_steps, got_score, want_steps, want_score, what=""):
    assert len(got_steps) == len(want_steps), what
    for f in ("i", "j", "op"):
        assert np.array_equal(got_steps[f], want_steps[f]), (what, f)
    assert np.array_equal(ref.bits(got_steps["cost"]), ref.bits(want_steps["cost"])), what
    assert ref.bits([got_score])[0] == ref.bits([want_score])[0], what


def check_batch(apd, ctx, key, seqs, pct, pen, pairs, batch=None):
    own = batch is None
    batch = batch or make_batch(ctx, seqs)
    try:
        got, scores, off = raw_paths(apd, ctx, batch, pct, pen, pairs)
    finally:
        if own:
            batch.close()
    for p, (x, y) in enumerate(pairs):
        want_steps, want_score = reference(key, seqs, pct, pen, x, y)
        assert int(off[p + 1] - off[p]) == len(seqs[x]) + len(seqs[y]) - 1
        assert_same_path(got[p], scores[p], want_steps, want_score, "%s pair (%d, %d)" % (key, x, y))
    return got, scores


def all_ordered(n):
    return [(a, b) for a in range(n) for b in range(n) if a != b]


def gauss_seqs(lengths, dim, seed, integer=False):
    rng = np.random.default_rng(seed)
    if integer:
        return [rng.integers(-2, 3, (n, dim)).astype(np.float32) for n in lengths]
    return [rng.standard_normal((n, dim)).astype(np.float32) for n in lengths]


BIND_LENGTHS = (40, 43, 37, 41, 38, 42, 40, 39, 43, 37, 41, 40)


@pytest.fixture(scope="module")
def bind_seqs():
    return gauss_seqs(BIND_LENGTHS, 13, 11)


def bind_pairs():
    return all_ordered(12) + [(s, s) for s in range(12)] + [(3, 7), (3, 7), (0, 11)]


def pair_path(apd, ctx, x, y, band, pen=UNIT):
    """apd_align_pair_path through ctypes."""
    L = apd.lib()
    x, y = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(y, np.float32)
    p = apd.AlignmentParamsC(band, *pen)
    bound = int(L.apd_path_bound(len(x), len(y)))
    steps = np.zeros(bound, dtype=ref.STEP)
    used, score = C.c_uint64(99), C.c_float(0)
    f32p = C.POINTER(C.c_float)
    apd.check(L.apd_align_pair_path(ctx.handle, x.ctypes.data_as(f32p), len(x), y.ctypes.data_as(f32p), len(y), x.shape[1], C.byref(p),
                                    steps.ctypes.data_as(C.POINTER(apd.PathStep)), bound, C.byref(used), C.byref(score)), ctx.handle)
    return steps[:used.value].copy(), np.float32(score.value)


def test_hand_cases_through_both_entry_points(apd, ctx):
    M, I, S = ref.MATCH, ref.INSERT, ref.START
    hand = ((np.array([[0], [1], [0], [0]], np.float32), np.array([[1], [0], [1], [0]], np.float32), 4,
             [(0, 0, 0.0, S), (1, 1, 1.0, M), (2, 2, 2.0, M), (3, 3, 3.0, M)], 0.375),          # the tie quirk: MATCH although larger
            (np.array([[0], [1], [5]], np.float32), np.array([[0], [9]], np.float32), 3,
             [(0, 0, 0.0, S), (1, 1, 0.0, M), (2, 1, 1.0, I)], 0.2))
    for x, y, band, want, want_score in hand:
        steps, score = pair_path(apd, ctx, x, y, band)
        assert [(int(s["i"]), int(s["j"]), float(s["cost"]), int(s["op"])) for s in steps] == want
        assert score == np.float32(want_score)
        batch = make_batch(ctx, [x, y])
        got, scores, _ = raw_paths(apd, ctx, batch, 1.0, UNIT, [(0, 1)])       # pct 1.0: band = max(n, m) = the hand case's band
        batch.close()
        assert [(int(s["i"]), int(s["j"]), float(s["cost"]), int(s["op"])) for s in got[0]] == want
        assert scores[0] == np.float32(want_score)


def test_band_binds_every_ordered_pair_in_input_order(apd, ctx, bind_seqs):
    """C = 2, one direction word: all 132 ordered pairs, the 12 (s, s) pairs, a repeated pair; results in input order."""
    got, scores = check_batch(apd, ctx, "bind", bind_seqs, 0.0625, UNIT, bind_pairs())
    for s in range(12):                                                        # x == y: the diagonal, cost 0 all the way
        steps = got[132 + s]
        assert np.all(steps["op"][1:] == ref.MATCH) and not steps["cost"].any() and scores[132 + s] == 0.0
    assert np.array_equal(got[144].view(np.uint32), got[145].view(np.uint32)) and scores[144].view(np.uint32) == scores[145].view(np.uint32)


def test_band_widens_with_the_length_gap(apd, ctx):
    lengths = (30, 46, 62, 78, 94, 110)
    seqs = gauss_seqs(lengths, 13, 12)
    pairs = [(0, 5), (5, 0), (1, 4), (4, 1), (2, 3), (3, 2), (0, 1), (5, 4), (2, 5), (4, 0)]
    assert all(abs(lengths[a] - lengths[b]) > ref.band_from_pct(0.0625, max(lengths[a], lengths[b])) for a, b in pairs)
    check_batch(apd, ctx, "widen", seqs, 0.0625, UNIT, pairs)


def test_band_zero(apd, ctx, bind_seqs):
    check_batch(apd, ctx, "bind", bind_seqs, 0.0, UNIT, all_ordered(12)[::5] + [(4, 4)])


def test_full_band_three_cells_per_lane(apd, ctx):
    seqs = gauss_seqs((80, 77, 83, 80), 13, 13)                                # w = 82 .. 85: 2w+1 >= 165, C = 3
    check_batch(apd, ctx, "full", seqs, 1.0, UNIT, all_ordered(4))
    check_batch(apd, ctx, "full", seqs, 1.0, SKEWED, [(0, 2), (2, 0), (1, 3)])


def test_more_than_one_direction_word_per_lane(apd, ctx):
    seqs = gauss_seqs((520, 530), 3, 14)                                       # w = 532: 2w+1 = 1065, C = 17, two words per lane
    check_batch(apd, ctx, "words", seqs, 1.0, UNIT, [(0, 1), (1, 0)])


def test_dp_row_beyond_64_kib_of_lds(apd, ctx):
    """3 x 8200 frames: w = 8199, 2w+1 = 16399 offsets, C = 257 cells per lane -- the sweep's row takes 65.8 KB of dynamic LDS (the
    launch has to ask for it) and 17 direction words per lane; the walk runs along a row across every lane."""
    seqs = gauss_seqs((3, 8200), 1, 15)
    check_batch(apd, ctx, "lds", seqs, 0.0, UNIT, [(0, 1), (1, 0)])


@pytest.mark.parametrize("dim", [1, 5])
@pytest.mark.parametrize("pen", [UNIT, SKEWED])
def test_integer_ties(apd, ctx, dim, pen):
    seqs = gauss_seqs((25, 28, 22, 25, 31, 24), dim, 16 + dim, integer=True)
    got, _ = check_batch(apd, ctx, "ties%d" % dim, seqs, 0.25, pen, all_ordered(6))
    assert any(np.any(s["op"] == ref.INSERT) for s in got) and any(np.any(s["op"] == ref.DELETE) for s in got)


@pytest.mark.parametrize("dim", [1, 3, 8, 13, 26, 40])
def test_dimensions(apd, ctx, dim):
    seqs = gauss_seqs((21, 26, 19), dim, 20 + dim)
    check_batch(apd, ctx, "dim%d" % dim, seqs, 0.2, UNIT, [(0, 1), (1, 2), (2, 0)])


def test_degenerate_lengths(apd, ctx):
    lengths = (1, 1, 2, 2, 7, 30)
    seqs = gauss_seqs(lengths, 3, 30)
    pairs = all_ordered(6) + [(0, 0), (2, 2)]
    got, scores = check_batch(apd, ctx, "degenerate", seqs, 0.5, UNIT, pairs)
    for p, (x, y) in enumerate(pairs):
        n, m = lengths[x], lengths[y]
        if (n == 1) != (m == 1):
            assert len(got[p]) == 0 and np.isposinf(scores[p])                 # the score cell is absent
        if n == 1 and m == 1:
            assert [tuple(s) for s in got[p]] == [(0, 0, 0.0, ref.START)] and scores[p] == 0.0


def test_outside_the_feature_range(apd, ctx):
    """NaN, infinite and 2^-45 features need no routing: the arithmetic is the literal one anyway.  Walks through NaN cells take
    MATCH and may run into row 0 / column 0 away from the origin, where they end without a START step."""
    lengths = (20, 23, 18, 21, 25, 20)
    base = gauss_seqs(lengths, 13, 40)
    poisoned = {"nan": [s.copy() for s in base], "inf": [s.copy() for s in base], "tiny": [(s * np.float32(2.0 ** -45)) for s in base]}
    poisoned["nan"][1][0, 4] = np.nan                                          # first frame: every cell of (1, *) after it is NaN
    poisoned["nan"][3][9, :] = np.nan
    poisoned["inf"][2][5, 0] = np.inf
    poisoned["inf"][4][3, 7] = -np.inf
    for name, seqs in poisoned.items():
        batch = make_batch(ctx, seqs)
        flag = C.c_int(0)
        apd.check(apd.lib().apd_batch_nonfinite(ctx.handle, batch.handle, C.byref(flag)), ctx.handle)
        assert flag.value == 1
        got, scores = check_batch(apd, ctx, name, seqs, 0.25, UNIT, all_ordered(6), batch=batch)
        batch.close()
        if name == "nan":
            early = [s for s in got if len(s) and s[0]["op"] != ref.START]
            assert early and np.isnan(scores).any() and np.isfinite(scores).any()
        if name == "tiny":
            assert np.all(np.isfinite(scores)) and np.any(scores > 0)


def test_chunked_equals_unchunked(apd, ctx, bind_seqs):
    pairs = bind_pairs()
    batch = make_batch(ctx, bind_seqs)
    whole, whole_scores, _ = raw_paths(apd, ctx, batch, 0.0625, UNIT, pairs)
    # direction words of a pair (include/apd.h): (len x + 63) * ceil(C / 16) * 256 bytes, C = 2 here
    need = sum((len(bind_seqs[x]) + 63) * 256 for x, _ in pairs)
    cap = need // 4
    assert need / cap >= 3
    os.environ["APD_PATH_WORKSPACE_BYTES"] = str(cap)
    try:
        parts, part_scores, _ = raw_paths(apd, ctx, batch, 0.0625, UNIT, pairs)
    finally:
        del os.environ["APD_PATH_WORKSPACE_BYTES"]
        batch.close()
    assert len(parts) == len(whole)
    for a, b in zip(parts, whole):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(part_scores.view(np.uint32), whole_scores.view(np.uint32))
    for p, (x, y) in enumerate(pairs):
        assert_same_path(parts[p], part_scores[p], *reference("bind", bind_seqs, 0.0625, UNIT, x, y))


def test_scores_equal_the_strict_matrix_in_every_mode(apd, ctx, oracle, bind_seqs):
    L = apd.lib()
    n = len(bind_seqs)
    pairs = all_ordered(n)
    batch = make_batch(ctx, bind_seqs)
    cfg = apd.AlignConfig(0.0625, 1.0, 1.0, 1.0)
    matrix = np.zeros((n, n), dtype=np.float32)
    try:
        ctx.set_distance_mode("strict")
        apd.check(L.apd_align_all(ctx.handle, batch.handle, C.byref(cfg), matrix.ctypes.data_as(C.POINTER(C.c_float))), ctx.handle)
        strict, strict_scores, _ = raw_paths(apd, ctx, batch, 0.0625, UNIT, pairs)
        ctx.set_distance_mode("hybrid")
        hybrid, hybrid_scores, _ = raw_paths(apd, ctx, batch, 0.0625, UNIT, pairs)
    finally:
        ctx.set_distance_mode("hybrid")
        batch.close()
    for p, (x, y) in enumerate(pairs):
        want = np.float32(oracle.dtw_pair(bind_seqs[x], bind_seqs[y], ref.band_from_pct(0.0625, max(len(bind_seqs[x]), len(bind_seqs[y])))))
        assert strict_scores[p].view(np.uint32) == matrix[x, y].view(np.uint32) == want.view(np.uint32), (x, y)
        assert np.array_equal(strict[p].view(np.uint32), hybrid[p].view(np.uint32))
    assert np.array_equal(strict_scores.view(np.uint32), hybrid_scores.view(np.uint32))


def test_paths_follow_a_refill(apd, ctx, bind_seqs):
    lengths = [len(s) for s in bind_seqs]
    fresh = gauss_seqs(lengths, 13, 50)
    pairs = [(0, 1), (5, 2), (11, 4), (7, 7)]
    batch = make_batch(ctx, bind_seqs)
    try:
        check_batch(apd, ctx, "bind", bind_seqs, 0.0625, UNIT, pairs, batch=batch)
        frames = np.ascontiguousarray(np.concatenate(fresh, axis=0))
        apd.check(apd.lib().apd_batch_refill(ctx.handle, batch.handle, C.c_void_p(frames.ctypes.data), 0), ctx.handle)
        got, _ = check_batch(apd, ctx, "refilled", fresh, 0.0625, UNIT, pairs, batch=batch)
    finally:
        batch.close()
    assert got[0]["cost"].tobytes() != reference("bind", bind_seqs, 0.0625, UNIT, 0, 1)[0]["cost"].tobytes()


def test_size_query_and_argument_errors(apd, ctx, bind_seqs):
    L = apd.lib()
    batch = make_batch(ctx, bind_seqs)
    cfg = apd.AlignConfig(0.0625, 1.0, 1.0, 1.0)
    u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    pairs = np.array([(0, 1), (2, 2), (11, 3)], dtype=np.uint32)
    off = np.zeros(4, dtype=np.uint64)
    try:
        assert L.apd_align_paths(ctx.handle, batch.handle, C.byref(cfg), pairs.ctypes.data_as(u32p), 3, None, 0, off.ctypes.data_as(u64p), None, None) == apd.APD_OK
        bounds = [int(L.apd_path_bound(len(bind_seqs[x]), len(bind_seqs[y]))) for x, y in pairs]
        assert off.tolist() == [0] + np.cumsum(bounds).tolist()
        steps = np.zeros(int(off[-1]), dtype=ref.STEP)
        lens, scores = np.zeros(3, np.uint32), np.zeros(3, np.float32)
        args = (steps.ctypes.data_as(C.POINTER(apd.PathStep)),)
        tail = (off.ctypes.data_as(u64p), lens.ctypes.data_as(u32p), scores.ctypes.data_as(C.POINTER(C.c_float)))
        assert L.apd_align_paths(ctx.handle, batch.handle, C.byref(cfg), pairs.ctypes.data_as(u32p), 3, *args, int(off[-1]) - 1, *tail) == apd.APD_ERR_INVALID_ARG
        bad = np.array([(0, 1), (12, 0)], dtype=np.uint32)                     # index = n_seq
        assert L.apd_align_paths(ctx.handle, batch.handle, C.byref(cfg), bad.ctypes.data_as(u32p), 2, *args, int(off[-1]), *tail) == apd.APD_ERR_INVALID_ARG
        assert L.apd_align_paths(ctx.handle, batch.handle, C.byref(cfg), None, 0, *args, 0, *tail) == apd.APD_OK and off[0] == 0
        # scores may be NULL
        assert L.apd_align_paths(ctx.handle, batch.handle, C.byref(cfg), pairs.ctypes.data_as(u32p), 3, *args, int(off[-1]), tail[0], tail[1], None) == apd.APD_OK
        assert lens[1] == len(bind_seqs[2])                                     # (2, 2): START + the diagonal to (n-1, n-1)
    finally:
        batch.close()
    # the single pair: sizes, empty sequences, a band the sweep cannot hold in LDS (2w+1 > 20480) refused before any launch
    f32p = C.POINTER(C.c_float)
    x = np.zeros((10300, 1), np.float32)
    p = apd.AlignmentParamsC(10300, 1.0, 1.0, 1.0)
    used, score = C.c_uint64(0), C.c_float(0)
    assert L.apd_align_pair_path(ctx.handle, x.ctypes.data_as(f32p), 5, x.ctypes.data_as(f32p), 9, 1, C.byref(p), None, 0, C.byref(used), C.byref(score)) == apd.APD_OK
    assert used.value == 13
    one = (apd.PathStep * 1)()
    assert L.apd_align_pair_path(ctx.handle, x.ctypes.data_as(f32p), 0, x.ctypes.data_as(f32p), 0, 1, C.byref(p), one, 1, C.byref(used), C.byref(score)) == apd.APD_OK
    assert used.value == 0 and np.isposinf(score.value)
    assert L.apd_align_pair_path(ctx.handle, x.ctypes.data_as(f32p), 0, x.ctypes.data_as(f32p), 4, 1, C.byref(p), one, 1, C.byref(used), C.byref(score)) == apd.APD_ERR_EMPTY_SEQUENCE
    assert L.apd_align_pair_path(ctx.handle, x.ctypes.data_as(f32p), 5, x.ctypes.data_as(f32p), 9, 1, C.byref(p), one, 1, C.byref(used), C.byref(score)) == apd.APD_ERR_INVALID_ARG
    big = np.zeros(2 * 10300 - 1, dtype=ref.STEP)
    assert L.apd_align_pair_path(ctx.handle, x.ctypes.data_as(f32p), 10300, x.ctypes.data_as(f32p), 10300, 1, C.byref(p),
                                 big.ctypes.data_as(C.POINTER(apd.PathStep)), len(big), C.byref(used), C.byref(score)) == apd.APD_ERR_BAND_TOO_WIDE


def test_python_mirror_agrees_with_the_raw_abi(apd, ctx, bind_seqs):
    from audio_pattern_discovery_amd.alignments import Alignment, AlignmentParams, AlignmentWorkers, NDSequence
    from audio_pattern_discovery_amd.discovery import Discovery
    pairs = [(0, 1), (6, 6), (9, 2), (9, 2)]
    workers = AlignmentWorkers.new([NDSequence(s) for s in bind_seqs], ctx)
    try:
        got, scores = workers.paths(pairs, Discovery(warping_band_percentage=0.0625))
    finally:
        workers.close()
    assert scores.dtype == np.float32 and len(got) == len(pairs)
    for p, (x, y) in enumerate(pairs):
        assert_same_path(got[p], scores[p], *reference("bind", bind_seqs, 0.0625, UNIT, x, y))
    a = Alignment(ctx)
    x, y = bind_seqs[0], bind_seqs[1]
    band = ref.band_from_pct(0.0625, max(len(x), len(y)))
    a.construct_alignment(NDSequence(x), NDSequence(y), AlignmentParams(band), path=True)
    assert_same_path(a.path(), np.float32(a.score()), *reference("bind", bind_seqs, 0.0625, UNIT, 0, 1))
    raw_steps, raw_score = pair_path(apd, ctx, x, y, band)
    assert np.array_equal(a.path().view(np.uint32), raw_steps.view(np.uint32)) and np.float32(a.score()) == raw_score
    a.construct_alignment(NDSequence(x), NDSequence(y), AlignmentParams(band))                  # without path=True: the score alone, as before
    with pytest.raises(ValueError):
        a.path()
