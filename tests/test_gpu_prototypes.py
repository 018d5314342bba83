"""GPU tests of the cluster prototypes (apd_cluster_medoids, apd_barycenters) against the checker tests/_dba_reference.py.

Every comparison is bitwise: medoids and counts equal, cost, inertia and frames equal as uint32 (NaN payloads aside:
_path_reference.bits says why).  Shapes are the smallest that reach each code path: barycenters longer than a wavefront, bands that
bind and widen, structural ties, barycenters of 1 and 2 frames, singleton and empty sets, frame dimensions with and without padding
slots, a NaN member, sets that straddle workspace chunks, joined batches, the device-resident result, 70 sets in one call; medoid
sets within one, two and three wavefronts, and 130 sets with runs of empty ones."""
import ctypes as C
import os

import numpy as np
import pytest

import _dba_reference as dba
import _path_reference as ref

pytestmark = pytest.mark.gpu
UNIT = (1.0, 1.0, 1.0)
SKEWED = (1.5, 0.75, 1.25)                      # (insertion, deletion, match)
U32P, U64P, F32P = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_float)


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


def flat_sets(sets):
    members = np.array([m for s in sets for m in s], dtype=np.uint32)
    set_off = np.zeros(len(sets) + 1, dtype=np.uint32)
    set_off[1:] = np.cumsum([len(s) for s in sets])
    return members, set_off


def raw_barycenters(apd, ctx, batch, dim, pct, pen, sets, init, iterations):
    """apd_barycenters through ctypes, host result: (list of frame arrays, inertia, used, frame_off).  The sizes-only call first;
    the frame after `capacity` is a canary."""
    L = apd.lib()
    cfg = apd.AlignConfig(pct, *pen)
    members, set_off = flat_sets(sets)
    init = np.ascontiguousarray(init, dtype=np.uint32)
    head = (ctx.handle, batch.handle, C.byref(cfg), members.ctypes.data_as(U32P), set_off.ctypes.data_as(U32P), len(sets),
            init.ctypes.data_as(U32P), iterations)
    off = np.full(len(sets) + 1, 77, dtype=np.uint64)
    ctx.synchronize()                                                                        # whatever made the batch is done
    apd.check(L.apd_barycenters(*head, None, 0, 0, off.ctypes.data_as(U64P), None, None), ctx.handle)
    assert not ctx.stream_busy()                                                             # sizes need no GPU work
    total = int(off[-1])
    frames = np.full((total + 1, dim), 0x55555555, dtype=np.uint32).view(np.float32)
    inertia = np.full((iterations, len(sets)), -1.0, dtype=np.float32)
    used = np.full((iterations, len(sets)), 99, dtype=np.uint32)
    off2 = np.zeros(len(sets) + 1, dtype=np.uint64)
    apd.check(L.apd_barycenters(*head, C.c_void_p(frames.ctypes.data), 0, total, off2.ctypes.data_as(U64P), inertia.ctypes.data_as(F32P),
                                used.ctypes.data_as(U32P)), ctx.handle)
    assert np.array_equal(off, off2)
    assert np.all(frames[total].view(np.uint32) == 0x55555555)                               # nothing written past the capacity
    return [frames[int(off[k]):int(off[k + 1])].copy() for k in range(len(sets))], inertia, used, off


def assert_same(got, want, what=""):
    (g_frames, g_inertia, g_used), (w_frames, w_inertia, w_used) = got, want
    assert len(g_frames) == len(w_frames), what
    for k, (g, w) in enumerate(zip(g_frames, w_frames)):
        assert g.shape == w.shape, (what, k)
        assert np.array_equal(ref.bits(g), ref.bits(w)), (what, "frames of set %d" % k)
    assert np.array_equal(g_used, w_used), (what, "used")
    assert np.array_equal(ref.bits(g_inertia), ref.bits(w_inertia)), (what, "inertia")


def check(apd, ctx, seqs, pct, pen, sets, init, iterations, what="", batch=None):
    own = batch is None
    batch = batch or make_batch(ctx, seqs)
    try:
        frames, inertia, used, off = raw_barycenters(apd, ctx, batch, seqs[0].shape[1], pct, pen, sets, init, iterations)
    finally:
        if own:
            batch.close()
    want = dba.barycenters(seqs, sets, init, pct, pen, iterations)
    assert np.diff(off).tolist() == [len(w) for w in want[0]]
    assert_same((frames, inertia, used), want, what)
    return (frames, inertia, used), want


def gauss_seqs(lengths, dim, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((n, dim)).astype(np.float32) for n in lengths]


def col(*values):
    return np.array(values, dtype=np.float32).reshape(-1, 1)


def test_known_answer_through_the_abi_and_the_mirror(apd, ctx):
    from audio_pattern_discovery_amd.alignments import AlignmentWorkers, NDSequence
    from audio_pattern_discovery_amd.discovery import Discovery
    seqs = [col(0, 2, 9), col(0, 4, 9)]
    (frames, inertia, used), _ = check(apd, ctx, seqs, 1.0, UNIT, [[0, 1]], [0], 1, "known answer")
    assert frames[0].tolist() == [[0.0], [3.0], [9.0]] and used.tolist() == [[2]] and inertia[0, 0] == np.float32(1.0 / 6.0)
    workers = AlignmentWorkers.new([NDSequence(s) for s in seqs], ctx)
    try:
        with pytest.raises(ValueError):
            workers.barycenters([[0, 1]], Discovery(warping_band_percentage=1.0))            # init=None before any align_all
        out, inertia, used = workers.barycenters([[1, 0]], Discovery(warping_band_percentage=1.0), init=[0], iterations=1)
        assert out[0].tolist() == [[0.0], [3.0], [9.0]] and used.tolist() == [[2]] and inertia[0, 0] == np.float32(1.0 / 6.0)
        workers.align_all(Discovery(warping_band_percentage=1.0))
        # medoids of the matrix: d(a, b) = d(b, a), a tie: sequence 0, the known answer again
        out, inertia, used = workers.barycenters([[0, 1]], Discovery(warping_band_percentage=1.0), iterations=1)
        assert out[0].tolist() == [[0.0], [3.0], [9.0]] and inertia.dtype == np.float32 and used.dtype == np.uint32
    finally:
        workers.close()


def test_rows_beyond_a_wavefront_band_binds_and_widens(apd, ctx):
    lengths = (55, 61, 67, 73, 79, 85, 1)
    seqs = gauss_seqs(lengths, 13, 71)
    band = ref.band_from_pct(0.0625, 85)
    assert abs(67 - 85) > band and abs(67 - 61) > ref.band_from_pct(0.0625, 67) and ref.band_from_pct(0.0625, 67) > 0
    (frames, inertia, used), _ = check(apd, ctx, seqs, 0.0625, UNIT, [list(range(7))], [2], 3, "one set")
    assert used.tolist() == [[6], [6], [6]]                                                  # the one-frame member never contributes
    assert np.array_equal(frames[0][-1], seqs[2][-1]) and not np.array_equal(frames[0][:-1], seqs[2][:-1])
    assert np.all(np.isfinite(inertia))


def test_integer_features_structural_ties(apd, ctx):
    rng = np.random.default_rng(72)
    seqs = [rng.integers(0, 3, (n, 2)).astype(np.float32) for n in (9, 12, 10, 2, 17)]
    for init in (0, 3):
        check(apd, ctx, seqs, 0.25, SKEWED, [[4, 2, 0, 3, 1]], [init], 2, "ties, init %d" % init)


SEVERAL_LENGTHS = (1, 2, 9, 70, 8, 11, 64, 75, 3, 1)
SEVERAL_SETS = [[4, 5, 9], [1, 4, 8], [5, 2, 4], [3, 6, 7], [5], [], [9, 0]]
SEVERAL_INIT = [0, 1, 2, 3, 5, 0, 9]                                                         # set 0: its init is no member


@pytest.fixture(scope="module")
def several():
    seqs = gauss_seqs(SEVERAL_LENGTHS, 3, 73)
    return seqs, dba.barycenters(seqs, SEVERAL_SETS, SEVERAL_INIT, 0.25, UNIT, 2)


def test_several_sets_in_one_call(apd, ctx, several):
    seqs, want = several
    batch = make_batch(ctx, seqs)
    try:
        frames, inertia, used, off = raw_barycenters(apd, ctx, batch, 3, 0.25, UNIT, SEVERAL_SETS, SEVERAL_INIT, 2)
    finally:
        batch.close()
    assert_same((frames, inertia, used), want, "several sets")
    assert np.diff(off).tolist() == [1, 2, 9, 70, 11, 0, 1]
    assert used[0].tolist() == [1, 3, 3, 3, 1, 0, 2] and np.isposinf(inertia[:, 5]).all()
    assert frames[0].tobytes() == seqs[0].tobytes()                                          # T = 1 keeps its frame


def test_chunked_equals_unchunked(apd, ctx, several):
    """A cap of one byte: every pair is a chunk of its own, every set with two members straddles chunks."""
    seqs, want = several
    batch = make_batch(ctx, seqs)
    os.environ["APD_PATH_WORKSPACE_BYTES"] = "1"
    try:
        frames, inertia, used, _ = raw_barycenters(apd, ctx, batch, 3, 0.25, UNIT, SEVERAL_SETS, SEVERAL_INIT, 2)
    finally:
        del os.environ["APD_PATH_WORKSPACE_BYTES"]
        batch.close()
    assert_same((frames, inertia, used), want, "one pair per chunk")


def test_seventy_sets_of_short_sequences(apd, ctx):
    """bary_set_of (csrc/dtw_path.hip) finds the set of a pair, and of a barycenter frame, by the same search over set_off: 70 sets
    of 0 to 4 sequences of 1 to 12 frames, empty ones at the front, at the end and in runs in between."""
    rng = np.random.default_rng(82)
    lengths = [1 + (5 * s) % 12 for s in range(40)]
    seqs = gauss_seqs(lengths, 3, 82)
    sizes = [int(v) for v in rng.integers(1, 5, 70)]
    for k in (0, 1, 17, 33, 34, 35, 51, 68, 69):
        sizes[k] = 0
    sets = [[int(v) for v in rng.choice(len(seqs), size=sz, replace=False)] for sz in sizes]
    init = [int(rng.integers(0, len(seqs))) for _ in sets]                                   # usually no member of its set
    (frames, inertia, used), _ = check(apd, ctx, seqs, 0.25, UNIT, sets, init, 2, "70 sets")
    assert [len(f) for f in frames] == [lengths[i] if s else 0 for i, s in zip(init, sets)]
    assert (used[0] > 0).sum() >= 30 and np.all(used[:, [sz == 0 for sz in sizes]] == 0)


@pytest.mark.parametrize("dim", [1, 5, 13, 26, 32])
def test_dimensions(apd, ctx, dim):
    seqs = gauss_seqs((20, 23, 18, 21), dim, 80 + dim)
    check(apd, ctx, seqs, 0.2, UNIT, [[0, 1, 2, 3]], [3], 2, "dim %d" % dim)


def test_a_nan_member_of_the_inits_length(apd, ctx):
    seqs = gauss_seqs((20, 20, 22, 19), 13, 74)
    seqs[1][7, :] = np.nan
    (frames, inertia, used), (w_frames, _, w_used) = check(apd, ctx, seqs, 0.25, UNIT, [[0, 1, 2, 3]], [0], 2, "nan")
    assert w_used[0, 0] == 4                                                                 # the NaN path is complete: it contributes
    assert np.isnan(frames[0]).any() and np.isfinite(frames[0]).any()
    assert np.array_equal(np.isnan(frames[0]), np.isnan(w_frames[0]))


def test_joined_batch(apd, ctx):
    from audio_pattern_discovery_amd.alignments import Batch
    seqs = gauss_seqs((18, 25, 21, 30, 17, 22), 5, 75)
    first, second = make_batch(ctx, seqs[:3]), make_batch(ctx, seqs[3:])
    joined = Batch.join(first, second)
    try:
        check(apd, ctx, seqs, 0.2, UNIT, [[0, 4, 5], [3, 1], [2, 3, 4, 0]], [4, 1, 0], 2, "joined", batch=joined)
    finally:
        joined.close()
        second.close()
        first.close()


def test_result_on_the_device_makes_a_batch(apd, ctx):
    from audio_pattern_discovery_amd.alignments import AlignmentWorkers, Batch, NDSequence, PATH_STEP
    from audio_pattern_discovery_amd.discovery import Discovery
    seqs = gauss_seqs((24, 29, 21, 26, 23), 13, 76)
    sets, init = [[0, 1, 2], [3, 4, 1]], [1, 3]
    params = Discovery(warping_band_percentage=0.2)
    workers = AlignmentWorkers.new([NDSequence(s) for s in seqs], ctx)
    try:
        host, inertia, used = workers.barycenters(sets, params, init=init, iterations=2)
        buf, off, d_inertia, d_used = workers.barycenters(sets, params, init=init, iterations=2, on_device=True)
        assert_same((host, inertia, used), dba.barycenters(seqs, sets, init, 0.2, UNIT, 2), "host result")
        assert off.tolist() == [0, 29, 55] and inertia.tobytes() == d_inertia.tobytes() and used.tobytes() == d_used.tobytes()
        assert buf.to_numpy(np.float32, 55 * 13).tobytes() == np.concatenate(host).tobytes()
        # the device result as a batch, joined with the members: the path of (barycenter 1, member 4)
        protos = Batch(ctx, buf.ptr, off, 13, on_device=True)
        joined = Batch.join(protos, workers._batch)
        try:
            L = apd.lib()
            cfg = params.align_config()
            pair = np.array([1, 2 + 4], dtype=np.uint32)
            step_off, n_steps, score = np.zeros(2, np.uint64), np.zeros(1, np.uint32), np.zeros(1, np.float32)
            steps = np.zeros(int(L.apd_path_bound(26, 23)), dtype=PATH_STEP)
            apd.check(L.apd_align_paths(ctx.handle, joined.handle, C.byref(cfg), pair.ctypes.data_as(U32P), 1,
                                        steps.ctypes.data_as(C.POINTER(apd.PathStep)), len(steps), step_off.ctypes.data_as(U64P),
                                        n_steps.ctypes.data_as(U32P), score.ctypes.data_as(F32P)), ctx.handle)
        finally:
            joined.close()
            protos.close()
            buf.free()
    finally:
        workers.close()
    want_steps, want_score = ref.path(host[1], seqs[4], ref.band_from_pct(0.2, 26))
    got = steps[:int(n_steps[0])]
    assert len(got) == len(want_steps) and all(np.array_equal(got[f], want_steps[f]) for f in ("i", "j", "op"))
    assert np.array_equal(ref.bits(got["cost"]), ref.bits(want_steps["cost"])) and ref.bits(score)[0] == ref.bits([want_score])[0]


def test_errors_return_before_any_launch(apd, ctx):
    L = apd.lib()
    seqs = gauss_seqs((12, 15, 10), 3, 77)
    cfg = apd.AlignConfig(0.25, 1.0, 1.0, 1.0)
    frames = np.full((64, 3), 0x55555555, dtype=np.uint32).view(np.float32)
    inertia, used = np.full((1, 2), -1.0, dtype=np.float32), np.full((1, 2), 99, dtype=np.uint32)
    off = np.zeros(3, dtype=np.uint64)

    def call(batch, sets, init, capacity=64, config=cfg):
        members, set_off = flat_sets(sets)
        init = np.array(init, dtype=np.uint32)
        rc = L.apd_barycenters(ctx.handle, batch.handle, C.byref(config), members.ctypes.data_as(U32P), set_off.ctypes.data_as(U32P), len(sets),
                               init.ctypes.data_as(U32P), 1, C.c_void_p(frames.ctypes.data), 0, capacity, off.ctypes.data_as(U64P),
                               inertia.ctypes.data_as(F32P), used.ctypes.data_as(U32P))
        assert not ctx.stream_busy()
        assert np.all(frames.view(np.uint32) == 0x55555555) and np.all(inertia == -1.0) and np.all(used == 99)
        return rc

    batch = make_batch(ctx, seqs)
    try:
        assert call(batch, [[0, 1], [3]], [0, 1]) == apd.APD_ERR_INVALID_ARG                 # a member = the sequence count
        assert call(batch, [[0, 1], [2]], [0, 3]) == apd.APD_ERR_INVALID_ARG                 # an init sequence past the end
        assert call(batch, [[0, 1, 0], [2]], [0, 1]) == apd.APD_ERR_INVALID_ARG              # listed twice in one set
        assert call(batch, [[0, 1], [2]], [1, 0], capacity=26) == apd.APD_ERR_INVALID_ARG    # 15 + 12 frames do not fit
        assert off.tolist() == [0, 15, 27]
    finally:
        batch.close()
    batch = make_batch(ctx, seqs + [np.zeros((0, 3), np.float32)])
    try:
        assert call(batch, [[0, 1], [2]], [0, 1]) == apd.APD_ERR_EMPTY_SEQUENCE
    finally:
        batch.close()
    batch = make_batch(ctx, [np.zeros((3, 1), np.float32), np.zeros((10300, 1), np.float32)])
    wide = np.full((64, 1), 0x55555555, dtype=np.uint32).view(np.float32)
    try:                                                                                     # w = 10297 + 2: 2w+1 > 20480
        members, set_off, init = np.array([1], np.uint32), np.array([0, 1], np.uint32), np.array([0], np.uint32)
        rc = L.apd_barycenters(ctx.handle, batch.handle, C.byref(cfg), members.ctypes.data_as(U32P), set_off.ctypes.data_as(U32P), 1,
                               init.ctypes.data_as(U32P), 1, C.c_void_p(wide.ctypes.data), 0, 64, off.ctypes.data_as(U64P), None, None)
        assert rc == apd.APD_ERR_BAND_TOO_WIDE and not ctx.stream_busy() and np.all(wide.view(np.uint32) == 0x55555555)
    finally:
        batch.close()


# ------------------------------------------------------------------------------------------ medoids

def raw_medoids(apd, ctx, d, sets, want_cost=True):
    L = apd.lib()
    d = np.ascontiguousarray(d, dtype=np.float32)
    members, set_off = flat_sets(sets)
    medoid, cost = np.full(len(sets) + 1, 0x55555555, dtype=np.uint32), np.full(len(sets) + 1, -1.0, dtype=np.float32)
    apd.check(L.apd_cluster_medoids(ctx.handle, C.c_void_p(d.ctypes.data), 0, len(d), members.ctypes.data_as(U32P), set_off.ctypes.data_as(U32P),
                                    len(sets), C.c_void_p(medoid.ctypes.data), C.c_void_p(cost.ctypes.data) if want_cost else None), ctx.handle)
    assert medoid[-1] == 0x55555555 and cost[-1] == -1.0
    return medoid[:-1], cost[:-1]


def test_medoids_of_sets_beyond_one_and_two_wavefronts(apd, ctx):
    from audio_pattern_discovery_amd import clustering
    rng = np.random.default_rng(78)
    d = rng.random((200, 200), dtype=np.float32)
    order = rng.permutation(200)
    sets = [order[:1].tolist(), order[1:3].tolist(), order[3:68].tolist(), order[68:198].tolist(), []]
    want_m, want_c = dba.medoids(d, sets)
    got_m, got_c = raw_medoids(apd, ctx, d, sets)
    assert np.array_equal(got_m, want_m) and np.array_equal(ref.bits(got_c), ref.bits(want_c))
    assert got_m[4] == dba.NONE and np.isposinf(got_c[4]) and got_c[0] == np.float32(d[order[0], order[0]] + d[order[0], order[0]])
    m2, c2 = clustering.medoids(d, sets, ctx)
    assert np.array_equal(m2, want_m) and np.array_equal(ref.bits(c2), ref.bits(want_c))
    m3, _ = raw_medoids(apd, ctx, d, sets, want_cost=False)                                  # cost may be NULL
    assert np.array_equal(m3, want_m)


def test_medoids_of_130_sets_with_runs_of_empty_ones(apd, ctx):
    """medoid_pick_kernel's third, partial block (sets 128 and 129), and medoid_cost_kernel's search for `the largest k with
    set_off[k] <= e` among runs of equal offsets: three empty sets at the front, four in the middle, three at the end, and single
    empty sets in between."""
    rng = np.random.default_rng(83)
    n, n_sets = 200, 130
    d = rng.random((n, n), dtype=np.float32)
    sizes = [int(v) for v in rng.integers(1, 9, n_sets)]
    for k in (0, 1, 2, 40, 63, 64, 65, 66, 97, 127, 128, 129):
        sizes[k] = 0
    sizes[126], sizes[3] = 70, 1                                                             # beyond a wavefront; a singleton
    sets = [[int(v) for v in rng.choice(n, size=sz, replace=False)] for sz in sizes]        # unsorted, sequences shared between sets
    assert sum(sizes) > 3 * 64 and any(s != sorted(s) for s in sets)
    want_m, want_c = dba.medoids(d, sets)
    got_m, got_c = raw_medoids(apd, ctx, d, sets)
    assert np.array_equal(got_m, want_m) and np.array_equal(ref.bits(got_c), ref.bits(want_c))
    empty = np.array([sz == 0 for sz in sizes])
    assert np.all(got_m[empty] == dba.NONE) and np.isposinf(got_c[empty]).all() and np.all(got_m[~empty] != dba.NONE)


def test_medoid_ties_and_nan(apd, ctx):
    rng = np.random.default_rng(79)
    n = 70
    d = rng.integers(5, 40, (n, n)).astype(np.float32)                                       # integers: every sum is exact
    np.fill_diagonal(d, 0)
    d[3, :], d[:, 3] = 1, 1                                                                  # 3 and 10 are twins, and the closest to all
    d[10, :], d[:, 10] = d[3, :], d[:, 3]
    d[3, 3] = d[10, 10] = 0
    d[20, :] = np.nan
    d[30, 30] = np.nan
    everyone = [i for i in range(n) if i != 20]
    sets = [everyone[::-1], list(range(15, 26)), [30, 31, 32], [20]]
    want_m, want_c = dba.medoids(d, sets)
    assert want_m.tolist()[:2] == [3, dba.NONE] and want_m[2] in (31, 32) and want_m[3] == dba.NONE
    got_m, got_c = raw_medoids(apd, ctx, d, sets)
    assert np.array_equal(got_m, want_m) and np.array_equal(ref.bits(got_c), ref.bits(want_c))


def test_medoids_on_the_resident_matrix_of_align_all(apd, ctx):
    L = apd.lib()
    n = 40
    seqs = gauss_seqs([30 + (7 * s) % 11 for s in range(n)], 13, 81)
    batch = make_batch(ctx, seqs)
    cfg = apd.AlignConfig(0.0625, 1.0, 1.0, 1.0)
    sets = [list(range(0, 40, 3)), list(range(1, 40, 3)), [38, 2, 5, 8], []]
    members, set_off = flat_sets(sets)
    d_matrix, d_medoid, d_cost = ctx.alloc(n * n * 4), ctx.alloc(4 * 4), ctx.alloc(4 * 4)
    try:
        apd.check(L.apd_align_all_device_async(ctx.handle, batch.handle, C.byref(cfg), d_matrix.at(0)), ctx.handle)
        apd.check(L.apd_cluster_medoids(ctx.handle, d_matrix.at(0), 1, n, members.ctypes.data_as(U32P), set_off.ctypes.data_as(U32P), 4,
                                        d_medoid.at(0), d_cost.at(0)), ctx.handle)
        ctx.synchronize()
        matrix = d_matrix.to_numpy(np.float32).reshape(n, n)
        got_m, got_c = d_medoid.to_numpy(np.uint32), d_cost.to_numpy(np.float32)
        # n_sets = 0: nothing is written, nothing is read
        apd.check(L.apd_cluster_medoids(ctx.handle, d_matrix.at(0), 1, n, None, None, 0, d_medoid.at(0), d_cost.at(0)), ctx.handle)
        assert not ctx.stream_busy()
        assert np.array_equal(d_medoid.to_numpy(np.uint32), got_m)
        bad = np.array([0, 40], dtype=np.uint32)
        twice = np.array([7, 7], dtype=np.uint32)
        two = np.array([0, 2], dtype=np.uint32)
        for m in (bad, twice):
            assert L.apd_cluster_medoids(ctx.handle, d_matrix.at(0), 1, n, m.ctypes.data_as(U32P), two.ctypes.data_as(U32P), 1,
                                         d_medoid.at(0), d_cost.at(0)) == apd.APD_ERR_INVALID_ARG
        assert not ctx.stream_busy() and np.array_equal(d_medoid.to_numpy(np.uint32), got_m)
    finally:
        for b in (d_matrix, d_medoid, d_cost):
            b.free()
        batch.close()
    want_m, want_c = dba.medoids(matrix, sets)
    assert np.array_equal(got_m, want_m) and np.array_equal(ref.bits(got_c), ref.bits(want_c))
    assert np.all(np.isfinite(want_c[:3])) and want_m[3] == dba.NONE
