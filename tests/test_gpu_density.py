"""apd_density_clusters against the numpy contract of tests/_density_reference.py.  Every output is an integer and every comparison
is bitwise: labels, kind, degree, counts, nans.

The three environment knobs (APD_DENSITY_WORKSPACE_BYTES, APD_DENSITY_ROUNDS_PER_SYNC, APD_DENSITY_WORKGROUP) are read by the library
at every call, so the tests set them in this process around the calls they concern."""
import contextlib
import ctypes as C
import functools
import os

import numpy as np
import pytest

from audio_pattern_discovery_amd import synth
from _density_reference import (BORDER, BOTH, CORE, EITHER, F, NOISE, blob_matrix, border_tie_matrix, chain_matrix, density_reference)

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 2, 63, 64, 65, 127, 129, 193)
SETTINGS = ((0.3, 4), (0.5, 6), (0.2, 3), (0.3, 1))                           # the last: every point is core
INF, NAN = F(np.inf), F(np.nan)


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


def reference(d, settings, link):
    """(labels [S][n], counts [S][4], kind [S][n], degree [S][n], nans) of the contract."""
    per = [density_reference(d, eps, min_pts, link) for eps, min_pts in settings]
    return (np.stack([p[0] for p in per]), np.stack([p[3] for p in per]), np.stack([p[1] for p in per]), np.stack([p[2] for p in per]),
            per[0][4])


def run(d, settings, link, ctx, details=True, on_device=False):
    from audio_pattern_discovery_amd.clustering import density
    eps, min_pts = [s[0] for s in settings], [s[1] for s in settings]
    where = d
    buf = None
    if on_device:
        buf = ctx.upload(np.ascontiguousarray(d))
        where = (buf.at(), d.shape[0])
    try:
        out = density(where, eps, min_pts, link=link, ctx=ctx, on_device=on_device, details=details)
    finally:
        if buf is not None:
            buf.free()
    return (out[0] + out[1]) if details else out


def assert_same(got, want, what):
    names = ("labels", "counts", "kind", "degree", "nans")
    for name, g, w in zip(names, got, want):
        if name == "nans":
            assert g == w, "%s: nans %r, expected %r" % (what, g, w)
        else:
            assert g.dtype == w.dtype and g.shape == w.shape, "%s: %s %s %s, expected %s %s" % (what, name, g.dtype, g.shape, w.dtype, w.shape)
            assert np.array_equal(g, w), "%s: %s differs at %r" % (what, name, np.argwhere(g != w)[:5].tolist())


@functools.lru_cache(maxsize=None)
def case(n, link):
    """An asymmetric matrix and the contract's answer for SETTINGS: made once, read by every test."""
    d = blob_matrix(n, seed=n, asymmetric=True)
    d.setflags(write=False)
    return d, reference(d, SETTINGS, link)


@pytest.mark.parametrize("link", (EITHER, BOTH))
@pytest.mark.parametrize("n", SIZES)
def test_tile_edges(ctx, n, link):
    d, want = case(n, link)
    if n >= 127:                                                              # the input is not a degenerate one
        assert all(c[0] >= 2 and c[1] and c[2] and c[3] for c in want[1][:3]), want[1]
    assert_same(run(d, SETTINGS, link, ctx), want, "n %d link %d" % (n, link))
    assert_same(run(d, SETTINGS, link, ctx, details=False), want[:2], "kind, degree, nans NULL, n %d link %d" % (n, link))
    if n in (1, 65, 193):
        assert_same(run(d, SETTINGS, link, ctx, on_device=True), want, "on_device, n %d link %d" % (n, link))
        assert_same(run(d, SETTINGS, link, ctx, details=False, on_device=True), want[:2], "on_device, NULL, n %d link %d" % (n, link))


def test_special_values(ctx):
    """NaN, +-INF and -0.0 planted off the diagonal on both sides of a tile edge, a NaN and an INF on the diagonal (not counted, never
    near), against eps = 0, -0, +INF, NaN and an ordinary one."""
    for n in (70, 128):                                                       # the scalar and the 16-byte load path
        d = blob_matrix(n, seed=5 * n, asymmetric=True).copy()
        d[3, 66], d[66, 3], d[1, 2], d[65, 64] = NAN, 0.0, NAN, NAN
        d[5, 6], d[6, 5], d[7, 69], d[69, 7] = INF, INF, -INF, INF
        d[10, 11], d[11, 10], d[12, 67], d[67, 12] = -0.0, 0.0, -0.0, 5.0
        d[64, 64], d[0, 0], d[1, 1] = NAN, INF, -INF
        settings = ((0.0, 2), (-0.0, 1), (INF, 3), (INF, n), (INF, n + 1), (NAN, 1), (NAN, 2), (0.3, 4))
        for link in (EITHER, BOTH):
            want = reference(d, settings, link)
            assert want[4] == 3 and want[3][0].max() >= 1
            assert_same(run(d, settings, link, ctx), want, "n %d link %d" % (n, link))


@functools.lru_cache(maxsize=None)
def chains(count):
    """`count` path graphs of 1500 points each whose numbers are a seeded permutation, interleaved in one matrix, and 63 points that
    belong to none: components of diameter 1499."""
    n = 1500 * count + 63
    order = np.random.default_rng(17 + count).permutation(np.arange(20, n))[:1500 * count]
    paths = [order[c::count] for c in range(count)]
    d = chain_matrix(paths[0], n)
    for path in paths[1:]:
        d = np.minimum(d, chain_matrix(path, n))
    np.fill_diagonal(d, 0.0)
    d.setflags(write=False)
    return d, paths, reference(d, ((1.0, 2),), EITHER)


@pytest.mark.parametrize("count", (1, 2))
def test_long_chains(ctx, count):
    d, paths, want = chains(count)
    labels, counts = want[0][0], want[1][0]
    assert counts.tolist() == [count, 1500 * count, 0, 63]
    for path in paths:
        assert (labels[path] == path.min()).all()
    assert_same(run(d, ((1.0, 2),), EITHER, ctx), want, "%d chains" % count)
    if count == 1:
        with environment(APD_DENSITY_ROUNDS_PER_SYNC=1):
            assert_same(run(d, ((1.0, 2),), EITHER, ctx), want, "one round per sync")
        with environment(APD_DENSITY_ROUNDS_PER_SYNC=7, APD_DENSITY_WORKGROUP=1024):
            assert_same(run(d, ((1.0, 2),), EITHER, ctx), want, "seven rounds per sync")
        both = reference(d, ((1.0, 2),), BOTH)                                # the chain's links are one-directional
        assert both[1][0].tolist() == [0, 0, 0, len(d)]
        assert_same(run(d, ((1.0, 2),), BOTH, ctx), both, "BOTH")


def test_border_tie(ctx):
    d = border_tie_matrix()
    labels, counts, kind, degree, nans = run(d, ((0.5, 4),), EITHER, ctx)
    assert labels[0].tolist() == [2, 2, 2, 2, 6, 6, 6] and counts[0].tolist() == [2, 2, 5, 0] and nans == 0
    assert kind[0].tolist() == [BORDER, BORDER, CORE, BORDER, BORDER, BORDER, CORE] and degree[0].tolist() == [2, 2, 3, 2, 2, 2, 3]
    # the same graph spread over three tiles: the border point's two clusters are named by core points of other tiles
    n, at = 150, np.array([140, 3, 70, 5, 6, 130, 66])
    big = np.full((n, n), 9.0, F)
    big[np.ix_(at, at)] = d
    np.fill_diagonal(big, 0.0)
    want = reference(big, ((0.5, 4),), EITHER)
    assert want[0][0][140] == 66 and want[2][0][140] == BORDER and want[1][0].tolist() == [2, 2, 5, n - 7]
    assert_same(run(big, ((0.5, 4),), EITHER, ctx), want, "spread")


def test_eight_settings_in_one_call_equal_eight_calls(ctx):
    d = blob_matrix(193, seed=193, asymmetric=True).copy()
    d[7, 100] = d[191, 0] = NAN
    settings = ((0.3, 4), (0.5, 6), (0.2, 3), (0.3, 1), (0.25, 5), (1.0, 40), (0.05, 2), (INF, 194))
    for link in (EITHER, BOTH):
        want = reference(d, settings, link)
        assert want[4] == 2 and len({tuple(lab) for lab in want[0]}) >= 6
        together = run(d, settings, link, ctx)
        assert_same(together, want, "link %d" % link)
        alone = [run(d, (s,), link, ctx) for s in settings]
        assert_same(together, tuple(np.concatenate([one[k] for one in alone]) for k in range(4)) + (alone[0][4],), "alone, link %d" % link)
        for knobs in (dict(APD_DENSITY_WORKSPACE_BYTES=1), dict(APD_DENSITY_WORKSPACE_BYTES=3 * 193 * 4 * 8 + 8),
                      dict(APD_DENSITY_WORKGROUP=64), dict(APD_DENSITY_WORKGROUP=1024),
                      dict(APD_DENSITY_WORKSPACE_BYTES=1, APD_DENSITY_WORKGROUP=128, APD_DENSITY_ROUNDS_PER_SYNC=1)):
            with environment(**knobs):
                assert_same(run(d, settings, link, ctx), want, "link %d %r" % (link, knobs))
                assert_same(run(d, settings, link, ctx, on_device=True), want, "on_device, link %d %r" % (link, knobs))


@functools.lru_cache(maxsize=None)
def real_matrix():
    """200 synthetic sequences and their matrix from the GPU (the corpus of tests/test_gpu_silhouette.py)."""
    from audio_pattern_discovery_amd import _lib
    from audio_pattern_discovery_amd.alignments import AlignmentWorkers, NDSequence
    from audio_pattern_discovery_amd.discovery import Discovery
    frames, offsets = synth.make_sequences(200, 24, 13, seed=11)
    workers = AlignmentWorkers.new([NDSequence(s) for s in synth.split(frames, offsets)], _lib.default_context())
    d = np.ascontiguousarray(workers.align_all(Discovery(warping_band_percentage=0.25)).reshape(200, 200))
    d.setflags(write=False)
    return d


def test_on_device_form_on_an_alignment_matrix(ctx):
    from audio_pattern_discovery_amd.clustering import density, neighbors, silhouette
    d = real_matrix()
    n, k = 200, 4
    _, kth, count, _ = neighbors(d, k, skip_self=True, ctx=ctx)
    assert (count == k).all()
    eps = [float(np.quantile(kth[:, k - 1], q)) for q in (0.25, 0.5, 0.9)]
    settings = tuple((e, k + 1) for e in eps)
    for link in (EITHER, BOTH):
        want = reference(d, settings, link)
        host = run(d, settings, link, ctx)
        assert_same(host, want, "host, link %d" % link)
        assert_same(run(d, settings, link, ctx, on_device=True), host, "on_device, link %d" % link)
        score, clusters, nans = silhouette(d, host[0], ctx=ctx)               # noise as singletons: a valid assignment
        assert clusters.tolist() == [len(np.unique(lab)) for lab in host[0]]
        assert clusters.tolist() == [int(c[0] + c[3]) for c in host[1]]
    # the k-th neighbour distance of i as eps with min_pts = k + 1 makes i core
    for i in (0, 57, 199):
        (_, _), (kind, degree, _) = density(d, float(kth[i, k - 1]), k + 1, ctx=ctx, details=True)
        assert kind[i] == CORE and degree[i] >= k


def raw_call(apd, ctx, d_ptr, n, link, eps, min_pts, n_settings, outs):
    f32p, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    e = None if eps is None else eps.ctypes.data_as(f32p)
    m = None if min_pts is None else min_pts.ctypes.data_as(u32p)
    return apd.lib().apd_density_clusters(None if ctx is None else ctx.handle, d_ptr, 0, n, link, e, m, n_settings, *outs)


def test_invalid_arguments_leave_the_outputs_untouched(ctx, apd):
    d, _ = case(65, EITHER)
    n = 65
    eps, min_pts = np.full(9, 0.3, F), np.full(9, 4, np.uint32)
    zero = min_pts.copy()
    zero[2] = 0
    host = [np.full((9, n), 0x5A5A5A5A, np.uint32) for _ in range(5)]
    ptrs = [C.c_void_p(h.ctypes.data) for h in host]
    d_ptr = C.c_void_p(d.ctypes.data)
    without = lambda k: [None if j == k else p for j, p in enumerate(ptrs)]
    calls = {"link 2": (ctx, d_ptr, n, 2, eps, min_pts, 3, ptrs), "link -1": (ctx, d_ptr, n, -1, eps, min_pts, 3, ptrs),
             "no settings": (ctx, d_ptr, n, 0, eps, min_pts, 0, ptrs), "nine settings": (ctx, d_ptr, n, 0, eps, min_pts, 9, ptrs),
             "a min_pts of 0": (ctx, d_ptr, n, 1, eps, zero, 3, ptrs), "no eps": (ctx, d_ptr, n, 0, None, min_pts, 3, ptrs),
             "no min_pts": (ctx, d_ptr, n, 0, eps, None, 3, ptrs), "no labels": (ctx, d_ptr, n, 0, eps, min_pts, 3, without(0)),
             "no counts": (ctx, d_ptr, n, 1, eps, min_pts, 3, without(3)), "no context": (None, d_ptr, n, 0, eps, min_pts, 3, ptrs)}
    for what, args in calls.items():
        assert raw_call(apd, *args) == apd.APD_ERR_INVALID_ARG, what
        assert all((h == 0x5A5A5A5A).all() for h in host), what
    assert raw_call(apd, ctx, d_ptr, n, 0, eps, min_pts, 8, ptrs) == apd.APD_OK   # and the largest number of settings is taken
    assert not (host[0][:8] == 0x5A5A5A5A).any() and (host[0][8] == 0x5A5A5A5A).all()
    counts = np.full((2, 4), 0x5A5A5A5A, np.uint32)                            # n = 0: zero counts, nothing else
    nans = np.full(1, 77, np.uint64)
    outs = [ptrs[0], None, None, C.c_void_p(counts.ctypes.data), C.c_void_p(nans.ctypes.data)]
    assert raw_call(apd, ctx, None, 0, 0, eps, min_pts, 2, outs) == apd.APD_OK
    assert not counts.any() and nans[0] == 0
