"""apd_silhouette against the numpy contract of tests/_silhouette_reference.py.  Every comparison is bitwise: score, clusters, nans,
s, a, b, nearest.  A NaN equals a NaN (which NaN an operation makes is the hardware's choice: x86 gives INF - INF the sign bit, the GPU
does not; `comparable` in the reference file); the one NaN the contract states, the score of a cut with nothing kept, is checked raw.

The three environment knobs (APD_SILHOUETTE_WORKGROUP, APD_SILHOUETTE_LDS_COLUMNS, APD_SILHOUETTE_WORKSPACE_BYTES) are read by the
library at every call, so the tests set them in this process around the calls they concern."""
import contextlib
import ctypes as C
import functools
import os

import numpy as np
import pytest

from audio_pattern_discovery_amd import synth
from _silhouette_reference import F, KINDS, assert_same, bits, cluster_means, comparable, matrix, silhouette_rows

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 63, 64, 65, 130, 300)


@pytest.fixture(scope="module")
def ctx(apd):
    c = apd.Context(0)
    yield c
    c.close()


@contextlib.contextmanager
def environment(**values):
    old = {name: os.environ.get(name) for name in values}
    os.environ.update({name: str(v) for name, v in values.items()})
    try:
        yield
    finally:
        for name, v in old.items():
            if v is None:
                del os.environ[name]
            else:
                os.environ[name] = v


def label_sets(n):
    """[L][n]: all singletons, one cluster, two clusters, clusters of 1, 64, 65 and 129 members (as many of them as n holds, the
    rest one more cluster), sparse large label values, and enough singleton cuts that the (cut, cluster) items outnumber the 256
    work-items of a workgroup at every n above 64."""
    rng = np.random.default_rng(n)
    me = np.arange(n, dtype=np.uint32)
    sized = np.full(n, 4, np.uint32)
    at = 0
    for label, size in enumerate((1, 64, 65, 129)):
        sized[at:at + size] = label
        at += size
    sets = [me, np.full(n, 11, np.uint32), (me % 2 == 0).astype(np.uint32), rng.permutation(sized).astype(np.uint32),
            np.array([0xFFFFFFFF, 0x80000000, 0x7FFFFFFF, 5, 0xFFFFFFFE], np.uint32)[rng.integers(0, 5, n)],
            me[::-1] * np.uint32(3), (me // 3).astype(np.uint32), rng.integers(0, max(n // 4, 1), n).astype(np.uint32)]
    return np.ascontiguousarray(np.stack(sets))


@functools.lru_cache(maxsize=None)
def case(n, kind="random"):
    """A matrix, its label table and the contract's answer on both axes: made once, read by every test."""
    d = matrix(n, 7 * n + KINDS.index(kind), kind)
    labels = label_sets(n)
    d.setflags(write=False)
    labels.setflags(write=False)
    return d, labels, {axis: stacked(d, labels, axis) for axis in (0, 1)}


def stacked(d, labels, axis):
    per_cut = [silhouette_rows(d, lab, axis) for lab in labels]
    return tuple(np.stack([np.asarray(cut[k]) for cut in per_cut]) for k in range(7))


def run(d, labels, axis, ctx, on_device=False):
    from audio_pattern_discovery_amd.clustering import silhouette
    if on_device:
        buf = ctx.upload(np.ascontiguousarray(d)) if d.size else ctx.alloc(16)
        try:
            head, samples = silhouette((buf.at(), d.shape[0]), labels, axis, samples=True, ctx=ctx, on_device=True)
        finally:
            buf.free()
    else:
        head, samples = silhouette(d, labels, axis, samples=True, ctx=ctx)
    return tuple(head) + tuple(samples)


@pytest.mark.parametrize("axis", (0, 1))
@pytest.mark.parametrize("n", SIZES)
def test_every_output_matches_the_contract_bitwise(ctx, n, axis):
    d, labels, want = case(n)
    got = run(d, labels, axis, ctx)
    assert_same(got, want[axis], "n %d axis %d" % (n, axis))
    if n > 1:                                                                 # one cluster: no s(i) is kept, the score is THE quiet NaN
        assert got[2][1] == n and bits(got[0])[1] == 0x7FC00000
    if n in (3, 65, 300):
        assert_same(run(d, labels, axis, ctx, on_device=True), want[axis], "on_device, n %d axis %d" % (n, axis))


@pytest.mark.parametrize("kind", KINDS[1:])
def test_special_values(ctx, kind):
    """A NaN row and column, +INF entries, negative entries, sums of the smallest subnormal whose means are -0.0, small integers whose
    means tie."""
    for n in (5, 65):
        d, labels, want = case(n, kind)
        for axis in (0, 1):
            assert_same(run(d, labels, axis, ctx), want[axis], "%s n %d axis %d" % (kind, n, axis))
    if kind == "tiny":
        assert (bits(case(65, kind)[2][0][5]) == 0x80000000).any()            # a b of -0.0 really reaches the output


def test_hand_cases(ctx):
    from audio_pattern_discovery_amd.clustering import silhouette
    d = np.array([[0, 1, 4, 6], [2, 0, 5, 7], [8, 3, 0, 1], [9, 9, 2, 0]], F)
    (score, clusters, nans), (s, a, b, nearest) = silhouette(d, [7, 7, 9, 9], samples=True, ctx=ctx)
    assert a.tolist() == [1, 2, 1, 2] and b.tolist() == [5, 6, 5.5, 9] and nearest.tolist() == [9, 9, 7, 7] and clusters == 2 and nans == 0
    assert np.array_equal(s, np.array([F(4) / F(5), F(4) / F(6), F(4.5) / F(5.5), F(7) / F(9)], F)) and score.dtype == np.float32
    _, (s, a, b, _) = silhouette(d, [7, 7, 9, 9], axis=1, samples=True, ctx=ctx)
    assert a[0] == 2 and b[0] == 8.5 and s[0] == F(6.5) / F(8.5)
    score, clusters, nans = silhouette(np.zeros((0, 0), F), np.zeros((3, 0), np.uint32), ctx=ctx)   # n = 0: NaN scores, zero counts
    assert bits(score).tolist() == [0x7FC00000] * 3 and not clusters.any() and not nans.any()


def raw_call(apd, ctx, d_ptr, on_device, n, axis, labels, cuts, outs):
    """apd_silhouette itself; outs: seven pointers or None."""
    ptr = None if labels is None else labels.ctypes.data_as(C.POINTER(C.c_uint32))
    return apd.lib().apd_silhouette(ctx.handle, d_ptr, on_device, n, axis, ptr, cuts, *outs)


def test_optional_outputs_may_be_null_on_the_device_and_on_the_host(ctx, apd):
    d, labels, want = case(65)
    cuts, n = labels.shape
    shapes = [(cuts,)] * 3 + [(cuts, n)] * 4
    dtypes = [np.float32, np.uint32, np.uint32, np.float32, np.float32, np.float32, np.uint32]
    d_buf = ctx.upload(np.ascontiguousarray(d))
    bufs = [ctx.alloc(int(np.prod(s)) * 4) for s in shapes]
    try:
        for axis in (0, 1):
            for absent in (None, 3, 4, 5, 6, (3, 4, 5, 6)):
                gone = () if absent is None else (absent if isinstance(absent, tuple) else (absent,))
                for b in bufs:
                    b.fill(0xA5)
                outs = [None if k in gone else bufs[k].at() for k in range(7)]
                assert raw_call(apd, ctx, d_buf.at(), 1, n, axis, labels, cuts, outs) == apd.APD_OK
                host = [np.full(s, 0x5A5A5A5A, np.uint32).view(t) for s, t in zip(shapes, dtypes)]
                outs = [None if k in gone else C.c_void_p(host[k].ctypes.data) for k in range(7)]
                assert raw_call(apd, ctx, C.c_void_p(d.ctypes.data), 0, n, axis, labels, cuts, outs) == apd.APD_OK
                for k in range(7):
                    got = bufs[k].to_numpy(dtypes[k], int(np.prod(shapes[k]))).reshape(shapes[k])
                    what = "axis %d, absent %r, output %d" % (axis, absent, k)
                    if k in gone:
                        assert (bits(got) == 0xA5A5A5A5).all() and (bits(host[k]) == 0x5A5A5A5A).all(), what
                    else:
                        assert np.array_equal(comparable(got), comparable(want[axis][k])), "device, " + what
                        assert np.array_equal(comparable(host[k]), comparable(want[axis][k])), "host, " + what
    finally:
        for b in bufs + [d_buf]:
            b.free()


def test_invalid_arguments_leave_the_outputs_untouched(ctx, apd):
    d, labels, _ = case(5)
    cuts, n = labels.shape
    host = [np.full((cuts, n), 0x5A5A5A5A, np.uint32) for _ in range(7)]
    ptrs = [C.c_void_p(h.ctypes.data) for h in host]
    d_ptr = C.c_void_p(d.ctypes.data)
    without = lambda k: [None if j == k else p for j, p in enumerate(ptrs)]
    calls = {"axis 2": (d_ptr, 0, n, 2, labels, cuts, ptrs), "axis -1": (d_ptr, 0, n, -1, labels, cuts, ptrs),
             "no cuts": (d_ptr, 0, n, 0, labels, 0, ptrs), "no labels": (d_ptr, 0, n, 0, None, cuts, ptrs),
             "no score": (d_ptr, 0, n, 0, labels, cuts, without(0)), "no clusters": (d_ptr, 0, n, 1, labels, cuts, without(1)),
             "no nans": (d_ptr, 0, n, 0, labels, cuts, without(2))}
    for what, args in calls.items():
        assert raw_call(apd, ctx, *args) == apd.APD_ERR_INVALID_ARG, what
        assert all((h == 0x5A5A5A5A).all() for h in host), what
    assert apd.lib().apd_silhouette(None, d_ptr, 0, n, 0, labels.ctypes.data_as(C.POINTER(C.c_uint32)), cuts, *ptrs) == apd.APD_ERR_INVALID_ARG


def test_the_knobs_do_not_change_a_bit(ctx):
    """Workgroups of 64 and 1024 work-items (the items are dealt anew), an LDS limit below n (the row is read from HBM), a panel
    workspace of one column (n gathers and launches on the column axis)."""
    for n in (65, 300):
        d, labels, want = case(n)
        for axis in (0, 1):
            for knobs in (dict(APD_SILHOUETTE_WORKGROUP=64), dict(APD_SILHOUETTE_WORKGROUP=1024), dict(APD_SILHOUETTE_LDS_COLUMNS=64),
                          dict(APD_SILHOUETTE_LDS_COLUMNS=0, APD_SILHOUETTE_WORKGROUP=128), dict(APD_SILHOUETTE_WORKSPACE_BYTES=1),
                          dict(APD_SILHOUETTE_WORKSPACE_BYTES=4 * 304 * 70, APD_SILHOUETTE_LDS_COLUMNS=64, APD_SILHOUETTE_WORKGROUP=64)):
                if "APD_SILHOUETTE_WORKSPACE_BYTES" in knobs and axis == 0:
                    continue
                with environment(**knobs):
                    assert_same(run(d, labels, axis, ctx), want[axis], "n %d axis %d %r" % (n, axis, knobs))


def test_means_are_cross_linkage_bits(ctx):
    """ROWS: for L != C(i), mean(i, L) is apd_cross_linkage's link_fs[i][L] with fs = the matrix.  b(i) is the mean of nearest(i), and
    with two clusters it is the mean of the only other one."""
    from audio_pattern_discovery_amd.clustering import cross_linkage, silhouette
    for n in (65, 300):
        d, labels, _ = case(n)
        for lab in (labels[2], labels[3], labels[7]):
            present = np.unique(lab)
            sets = [np.flatnonzero(lab == L).tolist() for L in present]
            link_fs = cross_linkage(d, np.ascontiguousarray(d.T), sets, ctx=ctx)[0]
            _, (s, a, b, nearest) = silhouette(d, lab, samples=True, ctx=ctx)
            assert (nearest != 0xFFFFFFFF).all()
            k = np.searchsorted(present, nearest)
            assert np.array_equal(bits(b), bits(np.ascontiguousarray(link_fs[np.arange(n), k])))
            _, total, cnt = cluster_means(d, lab, 0)                          # and every other mean, through the reference's chains
            other = np.searchsorted(present, lab)[None, :] != np.arange(len(present))[:, None]
            with np.errstate(all="ignore"):
                mean = (total / cnt.astype(F)).astype(F)
            assert np.array_equal(bits(np.ascontiguousarray(mean[other])), bits(np.ascontiguousarray(link_fs.T[other])))


@functools.lru_cache(maxsize=None)
def real_run():
    """200 synthetic sequences, their matrix from the GPU, one UPGMA run high up the dendrogram."""
    from audio_pattern_discovery_amd import _lib
    from audio_pattern_discovery_amd.alignments import AlignmentWorkers, NDSequence
    from audio_pattern_discovery_amd.clustering import AgglomerativeClustering
    from audio_pattern_discovery_amd.discovery import Discovery
    ctx = _lib.default_context()
    frames, offsets = synth.make_sequences(200, 24, 13, seed=11)
    workers = AlignmentWorkers.new([NDSequence(s) for s in synth.split(frames, offsets)], ctx)
    d = np.ascontiguousarray(workers.align_all(Discovery(warping_band_percentage=0.25)).reshape(200, 200))
    ops, _ = AgglomerativeClustering.clustering(d, 200, 0.9, ctx)
    d.setflags(write=False)
    return d, ops


def test_forty_cuts_in_one_call_equal_forty_calls(ctx):
    from audio_pattern_discovery_amd.clustering import AgglomerativeClustering
    d, ops = real_run()
    assert len(ops) >= 80
    labels = np.stack([AgglomerativeClustering.assignment(ops[:kept], 200) for kept in np.linspace(0, len(ops), 40).astype(int)])
    assert len({tuple(lab) for lab in labels}) == 40
    for axis in (0, 1):
        together = run(d, labels, axis, ctx)
        for c in (0, 1, 20, 39):                                              # against the contract as well
            assert_same(tuple(x[c] for x in together), silhouette_rows(d, labels[c], axis), "cut %d axis %d" % (c, axis))
        alone = [run(d, labels[c:c + 1], axis, ctx) for c in range(40)]
        assert_same(together, tuple(np.concatenate([one[k] for one in alone]) for k in range(7)), "axis %d" % axis)


def test_sweep_end_to_end(ctx):
    """The kept prefix of every percentile is what a fresh apd_clustering returns at that percentile -- operations, the bits of their
    distances, the threshold -- and the scores are those of separate calls."""
    from audio_pattern_discovery_amd.clustering import AgglomerativeClustering, silhouette
    d, _ = real_run()
    percs = (0.2, 0.02, 0.6)
    for axis in (0, 1):
        rows, ops = AgglomerativeClustering.sweep(d, 200, percs, axis=axis, ctx=ctx, return_operations=True)
        assert [r[0] for r in rows] == list(percs) and rows == AgglomerativeClustering.sweep(d, 200, percs, axis=axis, ctx=ctx)
        assert len({r[2] for r in rows}) == 3 and max(r[2] for r in rows) == len(ops)
        for perc, threshold, n_ops, n_clusters, score, nans in rows:
            fresh, roots, fresh_threshold = AgglomerativeClustering.clustering(d, 200, perc, ctx, return_threshold=True)
            assert bits(np.array([threshold], F))[0] == bits(np.array([fresh_threshold], F))[0]
            assert [(o.merge_i, o.merge_j, o.into, o.operation) for o in fresh] == [(o.merge_i, o.merge_j, o.into, o.operation) for o in ops[:n_ops]]
            assert np.array_equal(bits(np.array([o.distance for o in fresh], F)), bits(np.array([o.distance for o in ops[:n_ops]], F)))
            assert n_clusters == len(roots) == 200 - n_ops
            want = silhouette(d, AgglomerativeClustering.assignment(fresh, 200), axis=axis, ctx=ctx)
            assert (bits(np.array([score], F))[0], n_clusters, nans) == (bits(np.array([want[0]], F))[0], want[1], want[2])
