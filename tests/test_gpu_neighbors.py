"""apd_neighbors: the k nearest entries of rows and columns of a distance matrix, against the plain-Python contract of
tests/_neighbors_reference.py.  Every comparison is bitwise: index, the bits of distance, count, nans.

The three environment knobs (APD_NEIGHBORS_LDS_COLUMNS, APD_NEIGHBORS_WORKSPACE_BYTES, APD_NEIGHBORS_WORKGROUP) are read by the
library at every call, so the tests set them in this process around the calls they concern."""
import contextlib
import ctypes as C
import functools
import os

import numpy as np
import pytest

from audio_pattern_discovery_amd import synth
from _neighbors_reference import F, KINDS, PAD_INDEX, Ranked, assert_same, same, values

pytestmark = pytest.mark.gpu

COLS = (1, 63, 64, 65, 1000, 1025, 4097)
MAX_K = 1024


def rows_for(cols):
    return 70 if cols <= 65 else (12 if cols <= 1025 else 5)


def ks_for(cols):
    """(k, skip_self): the fixed ks, k == cols (where the API allows it: k <= 1024), k == cols - 1 with skip_self, k > cols."""
    ks = [(k, False) for k in (1, 2, 63, 64, 65, 1024)]
    if cols <= MAX_K:
        ks.append((cols, False))
    if 1 <= cols - 1 <= MAX_K:
        ks.append((cols - 1, True))
    if cols + 3 <= MAX_K:
        ks.append((cols + 3, False))
    return ks


@pytest.fixture(scope="module")
def ctx(apd):
    c = apd.Context(0)
    yield c
    c.close()


@contextlib.contextmanager
def environment(**values_):
    old = {name: os.environ.get(name) for name in values_}
    os.environ.update({name: str(v) for name, v in values_.items()})
    try:
        yield
    finally:
        for name, v in old.items():
            if v is None:
                del os.environ[name]
            else:
                os.environ[name] = v


@functools.lru_cache(maxsize=None)
def case(kind, cols, seed=0, k=16):
    """The matrix of a (kind, cols) and its candidates in order, with and without the self entry: made once, read by every test."""
    d = values(kind, rows_for(cols), cols, seed=1000 * KINDS.index(kind) + cols + seed, k=k)
    d.setflags(write=False)
    return d, {skip: Ranked(d, 0, skip) for skip in (False, True)}


@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("kind", KINDS)
def test_rows_match_the_contract_bitwise(ctx, kind, cols):
    from audio_pattern_discovery_amd.clustering import neighbors
    for k, skip in ks_for(cols):
        d, ranked = case(kind, cols, k=k) if kind == "inf" else case(kind, cols)
        want = ranked[skip].take(k)
        if kind == "inf" and cols > 1:
            assert np.isposinf(want[1]).any()                             # +INF really reaches the output
        assert_same(neighbors(d, k, 0, skip, ctx=ctx), want, "%s %dx%d k %d skip_self %d" % (kind, d.shape[0], cols, k, skip))


@pytest.mark.parametrize("kind", KINDS)
def test_the_streaming_row_path_gives_the_same_bits(ctx, kind):
    """Rows longer than the residency limit are re-read per pass instead of kept in LDS.  With the limit lowered to 64 entries the
    rows of 65, 1000 and 4097 entries take that path (and those of 63 and 64 do not)."""
    from audio_pattern_discovery_amd.clustering import neighbors
    for cols in (63, 64, 65, 1000, 4097):
        d, ranked = case(kind, cols)
        for k, skip in ((1, False), (64, False), (65, True), (1024, False)):
            resident = neighbors(d, k, 0, skip, ctx=ctx)
            with environment(APD_NEIGHBORS_LDS_COLUMNS=64):
                streamed = neighbors(d, k, 0, skip, ctx=ctx)
            what = "%s cols %d k %d skip_self %d" % (kind, cols, k, skip)
            assert_same(streamed, ranked[skip].take(k), "streamed, " + what)
            assert_same(streamed, resident, "streamed against resident, " + what)
    with environment(APD_NEIGHBORS_LDS_COLUMNS=0):                        # nothing resident at all
        d, ranked = case(kind, 63)
        assert_same(neighbors(d, 5, 0, True, ctx=ctx), ranked[True].take(5), "limit 0")


@pytest.mark.parametrize("cols", (8192, 8193, 16384, 32768, 32769))
def test_the_sizes_at_which_the_launch_changes(ctx, cols):
    """Rows of up to 8192 entries run in workgroups of 256, longer ones of 512 while two resident rows fit a compute unit's LDS
    (16384) and of 1024 beyond (32768); from about 14000 entries on the resident row needs more than 64 KB of LDS (asked for
    explicitly); 32768 entries is the last resident size, 32769 the first that streams by itself.  Three rows each (one of them the
    query's own for skip_self), both axes, and the streaming path at 1024 work-items."""
    from audio_pattern_discovery_amd.clustering import neighbors
    for kind in ("ties", "bits"):
        d = values(kind, 3, cols, seed=cols)
        for skip in (False, True):
            ranked = Ranked(d, 0, skip)
            for k in (1, 16, 1024):
                what = "%s cols %d k %d skip_self %d" % (kind, cols, k, skip)
                got = neighbors(d, k, 0, skip, ctx=ctx)
                assert_same(got, ranked.take(k), what)
                if k == 16:
                    assert_same(neighbors(np.ascontiguousarray(d.T), k, 1, skip, ctx=ctx), got, "columns, " + what)
                    with environment(APD_NEIGHBORS_LDS_COLUMNS=8192):
                        assert_same(neighbors(d, k, 0, skip, ctx=ctx), got, "residency limit 8192, " + what)


def test_the_workgroup_size_does_not_change_a_bit(ctx):
    """One wavefront, 256, 512 and 1024 work-items on rows of 65, 1000 and 4097 entries, resident and streamed."""
    from audio_pattern_discovery_amd.clustering import neighbors
    for kind in ("ties", "nan", "bits"):
        for cols in (65, 1000, 4097):
            d, ranked = case(kind, cols)
            for k, skip in ((2, False), (65, True), (1024, False)):
                want = ranked[skip].take(k)
                for wg in (64, 256, 512, 1024):
                    for limit in (32768, 64):
                        with environment(APD_NEIGHBORS_WORKGROUP=wg, APD_NEIGHBORS_LDS_COLUMNS=limit):
                            assert_same(neighbors(d, k, 0, skip, ctx=ctx), want, "%s cols %d k %d workgroup %d limit %d" % (kind, cols, k, wg, limit))


@pytest.mark.parametrize("kind", KINDS)
def test_columns_equal_rows_of_the_transpose(ctx, kind):
    from audio_pattern_discovery_amd.clustering import neighbors
    for cols in (1, 63, 65, 1025):
        d, _ = case(kind, cols)
        t = np.ascontiguousarray(d.T)                                     # [cols][rows]: its columns are d's rows
        for skip in (False, True):
            ranked = Ranked(t, 1, skip)
            for k in (1, 7, 64, 70, 71):
                by_columns = neighbors(t, k, 1, skip, ctx=ctx)
                what = "%s %dx%d k %d skip_self %d" % (kind, t.shape[0], t.shape[1], k, skip)
                assert_same(by_columns, ranked.take(k), "columns, " + what)
                assert_same(by_columns, neighbors(d, k, 0, skip, ctx=ctx), "columns against rows of the transpose, " + what)


def test_column_panels_do_not_change_a_bit(ctx):
    """The 1025 columns of a 70 x 1025 matrix: a panel row is 72 floats, so a workspace of 400 of them takes 384 columns at a time
    (whole tiles of 64) -- three panels, the last of 257 -- and one of a single byte takes one column at a time on a small matrix."""
    from audio_pattern_discovery_amd.clustering import neighbors
    for kind in ("ties", "nan", "bits"):
        d = values(kind, 70, 1025, seed=77)
        ranked = Ranked(d, 1, True)
        whole = neighbors(d, 33, 1, True, ctx=ctx)
        assert_same(whole, ranked.take(33), kind + ", one panel")
        with environment(APD_NEIGHBORS_WORKSPACE_BYTES=400 * 72 * 4):
            assert_same(neighbors(d, 33, 1, True, ctx=ctx), whole, kind + ", three panels")
            picked = [1024, 3, 3, 700, 0] + list(range(100, 500))          # a gathered list over two panels
            assert_same(neighbors(d, 33, 1, True, queries=picked, ctx=ctx), ranked.take(33, picked), kind + ", a list in two panels")
        small = values(kind, 9, 13, seed=78)
        with environment(APD_NEIGHBORS_WORKSPACE_BYTES=1, APD_NEIGHBORS_LDS_COLUMNS=4):
            assert_same(neighbors(small, 4, 1, False, ctx=ctx), Ranked(small, 1, False).take(4), kind + ", a column per panel")


def test_query_lists_on_both_axes(ctx):
    from audio_pattern_discovery_amd.clustering import neighbors
    d = values("ties", 70, 65, seed=5)
    rng = np.random.default_rng(6)
    for axis in (0, 1):
        n = d.shape[axis]
        picked = rng.permutation(n)[:n // 2].tolist()
        picked.insert(3, picked[0])                                       # a duplicate, answered again
        full = neighbors(d, 9, axis, True, ctx=ctx)
        got = neighbors(d, 9, axis, True, queries=picked, ctx=ctx)
        assert_same(got, tuple(part[picked] for part in full), "axis %d, the rows of the full answer" % axis)
        assert_same(got, Ranked(d, axis, True).take(9, picked), "axis %d, the contract" % axis)
    empty = neighbors(d, 9, 0, queries=[], ctx=ctx)
    assert empty[0].shape == (0, 9) and empty[2].shape == (0,)


def test_the_device_route_equals_the_host_route(ctx):
    from audio_pattern_discovery_amd.clustering import neighbors
    for kind, cols in (("bits", 1000), ("nan", 65), ("ties", 4097)):
        d, ranked = case(kind, cols)
        buf = ctx.upload(d)
        try:
            for axis in (0, 1):
                host = neighbors(d, 17, axis, True, ctx=ctx)
                device = neighbors((buf.ptr, d.shape[0], d.shape[1]), 17, axis, True, ctx=ctx, on_device=True)
                assert_same(device, host, "%s cols %d axis %d" % (kind, cols, axis))
                picked = [d.shape[axis] - 1, 0, 0]
                assert_same(neighbors((buf.ptr, d.shape[0], d.shape[1]), 17, axis, False, queries=picked, ctx=ctx, on_device=True),
                            Ranked(d, axis, False).take(17, picked), "%s cols %d axis %d, a list" % (kind, cols, axis))
        finally:
            buf.free()


def real_batch():
    """24 sequences of 93 .. 99 frames, number 11 cut to a single frame.  At 6.25 % the band (6) is wider than any length gap, so
    it is the band itself, [-w, w-1], that binds: the CPU oracle's matrix of this batch differs from its transpose in 44 entries."""
    frames, offsets = synth.make_sequences(24, 96, 13, seed=31, jitter=3)
    seqs = synth.split(frames, offsets)
    seqs[11] = seqs[11][:1]
    return seqs


def test_a_real_asymmetric_matrix_on_both_axes(ctx):
    from audio_pattern_discovery_amd.alignments import AlignmentWorkers, NDSequence
    from audio_pattern_discovery_amd.clustering import neighbors
    from audio_pattern_discovery_amd.discovery import Discovery
    workers = AlignmentWorkers.new([NDSequence(s) for s in real_batch()], ctx)
    try:
        d = workers.align_all(Discovery(warping_band_percentage=0.0625)).reshape(24, 24).copy()
    finally:
        workers.close()
    off = ~np.eye(24, dtype=bool)
    assert np.isposinf(d[11][off[11]]).all() and np.isposinf(d[:, 11][off[11]]).all()      # the one-frame sequence
    assert (d != d.T).any()
    by_rows, by_columns = neighbors(d, 5, 0, True, ctx=ctx), neighbors(d, 5, 1, True, ctx=ctx)
    assert_same(by_rows, Ranked(d, 0, True).take(5), "rows")
    assert_same(by_columns, Ranked(d, 1, True).take(5), "columns")
    all_of_them, all_by_columns = neighbors(d, 23, 0, True, ctx=ctx), neighbors(d, 23, 1, True, ctx=ctx)
    assert_same(all_of_them, Ranked(d, 0, True).take(23), "rows, everything")
    assert_same(all_by_columns, Ranked(d, 1, True).take(23), "columns, everything")
    assert not same(all_of_them, all_by_columns)                          # the two axes are different questions
    assert np.all(all_of_them[2] == 23) and np.all(np.isposinf(all_of_them[1][np.arange(24) != 11, -1]))   # +INF comes last


def test_nearest_equals_neighbors_on_the_cross_matrices(ctx):
    from audio_pattern_discovery_amd.alignments import AlignmentWorkers, NDSequence
    from audio_pattern_discovery_amd.clustering import neighbors
    from audio_pattern_discovery_amd.discovery import Discovery
    seqs = real_batch()
    params = Discovery(warping_band_percentage=0.0625)
    first, second = AlignmentWorkers.new([NDSequence(s) for s in seqs[:7]], ctx), AlignmentWorkers.new([NDSequence(s) for s in seqs[7:]], ctx)
    try:
        fs, sf = first.cross(second, params)
        assert fs.shape == (7, 17) and sf.shape == (17, 7)
        for k in (1, 4, 17, 20):
            assert_same(first.nearest(second, params, k, as_x=True), neighbors(fs, k, 0, ctx=ctx), "as x, k %d" % k)
            assert_same(first.nearest(second, params, k, as_x=False), neighbors(sf, k, 1, ctx=ctx), "as y, k %d" % k)
        assert_same(first.nearest(second, params, 4), Ranked(fs, 0).take(4), "as x against the contract")
        assert_same(first.nearest(second, params, 4, as_x=False), Ranked(sf, 1).take(4), "as y against the contract")
    finally:
        first.close()
        second.close()


def test_errors_leave_the_outputs_untouched(ctx, apd):
    d = values("ties", 6, 9, seed=3)
    u32p, vp = C.POINTER(C.c_uint32), C.c_void_p

    def call(k, axis, queries):
        index, distance = np.full((16, max(k, 1)), 0xABABABAB, np.uint32), np.full((16, max(k, 1)), 0xABABABAB, np.uint32)
        count, nans = np.full(16, 0xABABABAB, np.uint32), np.full(16, 0xABABABAB, np.uint32)
        q = None if queries is None else np.array(queries, np.uint32)
        rc = apd.lib().apd_neighbors(ctx.handle, vp(d.ctypes.data), 0, 6, 9, axis, None if q is None else q.ctypes.data_as(u32p),
                                     0 if q is None else len(q), k, 0, vp(index.ctypes.data), vp(distance.ctypes.data), vp(count.ctypes.data),
                                     vp(nans.ctypes.data))
        untouched = all(np.all(a == 0xABABABAB) for a in (index, distance, count, nans))
        return rc, untouched

    bad = apd.APD_ERR_INVALID_ARG
    assert call(0, 0, None) == (bad, True)
    assert call(1025, 0, None) == (bad, True)
    assert call(3, 2, None) == (bad, True)
    assert call(3, -1, None) == (bad, True)
    assert call(3, 0, [0, 5, 6]) == (bad, True)                           # rows: 0 .. 5
    assert call(3, 1, [8, 9, 0]) == (bad, True)                           # columns: 0 .. 8
    assert call(3, 0, [5, 0]) == (apd.APD_OK, False)
    assert call(3, 1, [8, 6]) == (apd.APD_OK, False)
    assert call(1024, 0, None) == (apd.APD_OK, False)


def test_empty_sides(ctx):
    from audio_pattern_discovery_amd.clustering import neighbors
    index, distance, count, nans = neighbors(np.zeros((5, 0), F), 3, 0, ctx=ctx)       # five rows of nothing: padding only
    assert np.all(index == PAD_INDEX) and np.isnan(distance).all() and count.tolist() == [0] * 5 and nans.tolist() == [0] * 5
    index, distance, count, nans = neighbors(np.zeros((0, 5), F), 3, 1, ctx=ctx)
    assert np.all(index == PAD_INDEX) and np.isnan(distance).all() and count.tolist() == [0] * 5
    assert neighbors(np.zeros((0, 5), F), 3, 0, ctx=ctx)[0].shape == (0, 3)            # no rows: no queries
