"""apd_density_tree against the numpy contract of tests/_density_tree_reference.py.  Every output is compared bitwise: core, edge_i,
edge_j, weight (as uint32 words), the number of edges, the padding behind them and nans.

The two environment knobs (APD_DENSITY_TREE_WORKSPACE_BYTES, APD_DENSITY_TREE_WORKGROUP) are read by the library at every call, so
the tests set them in this process around the calls they concern."""
import contextlib
import ctypes as C
import functools
import os

import numpy as np
import pytest

from _density_reference import BOTH, CORE, EITHER, F, blob_matrix, chain_matrix
from _density_tree_reference import rounded_matrix, special_matrix, tree_reference

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 2, 3, 63, 64, 65, 129, 130, 200, 1021, 1024)
INF, NAN = F(np.inf), F(np.nan)


def chain_over_random_order(n, seed):
    return chain_matrix(np.random.default_rng(seed).permutation(n), n) if n else np.zeros((0, 0), F)


KINDS = {"blobs": lambda n: blob_matrix(n, seed=n, asymmetric=True), "ties": lambda n: rounded_matrix(n, seed=n + 1),
         "equal": lambda n: np.full((n, n), 2.5, F), "chain": lambda n: chain_over_random_order(n, seed=n + 3),
         "special": lambda n: special_matrix(n, seed=n + 2)}


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


def min_pts_of(n):
    return sorted({1, 2, 9, max(n, 1), n + 1})


@functools.lru_cache(maxsize=None)
def case(kind, n, link, min_pts):
    """A matrix and the contract's answer: made once, read by every test."""
    d = KINDS[kind](n)
    d.setflags(write=False)
    return d, tree_reference(d, min_pts, link)


def most_rounds(n):
    return (max(n, 1) - 1).bit_length() + 1                                   # ceil(log2 n) + 1


def rounds_of(apd, ctx):
    phase, rounds = (C.c_float * 3)(), C.c_uint32(77)
    assert apd.lib().apd_density_tree_last_profile(ctx.handle, phase, C.byref(rounds)) == apd.APD_OK
    return rounds.value, list(phase)


def run(d, min_pts, link, ctx, on_device=False):
    from audio_pattern_discovery_amd.clustering import density_tree
    where, buf = d, None
    if on_device:
        buf = ctx.upload(np.ascontiguousarray(d)) if d.size else ctx.alloc(16)
        where = (buf.at(), d.shape[0])
    try:
        return density_tree(where, min_pts, link=link, ctx=ctx, on_device=on_device)
    finally:
        if buf is not None:
            buf.free()


def assert_same(got, want, what):
    for name, g, w in zip(("core", "edge_i", "edge_j", "weight"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, "%s: %s %s %s, expected %s %s" % (what, name, g.dtype, g.shape, w.dtype, w.shape)
        gw, ww = g.view(np.uint32), w.view(np.uint32)
        assert np.array_equal(gw, ww), "%s: %s differs at %r" % (what, name, np.flatnonzero(gw != ww)[:5].tolist())
    assert got[4] == want[4], "%s: nans %r, expected %r" % (what, got[4], want[4])


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("n", SIZES)
def test_tree_equals_the_contract(apd, ctx, n, kind):
    for link in (EITHER, BOTH):
        for min_pts in min_pts_of(n):
            d, want = case(kind, n, link, min_pts)
            what = "%s n %d link %d min_pts %d" % (kind, n, link, min_pts)
            assert_same(run(d, min_pts, link, ctx), want, what)
            rounds, _ = rounds_of(apd, ctx)
            assert rounds <= most_rounds(n) and (rounds >= 1 or n < 2), "%s: %d rounds" % (what, rounds)
            if min_pts in (1, 9):
                assert_same(run(d, min_pts, link, ctx, on_device=True), want, "on_device, " + what)
                assert rounds_of(apd, ctx)[0] <= most_rounds(n)
    if n >= 129 and kind == "blobs":                                          # the inputs are not degenerate ones
        assert len(case(kind, n, EITHER, 9)[1][1]) == n - 1 and len(np.unique(case(kind, n, EITHER, 9)[1][0])) > n // 4
    if n >= 129 and kind == "special":
        assert 0 < len(case(kind, n, BOTH, 2)[1][1]) < n - 2 and case(kind, n, BOTH, 2)[1][4] > n


@pytest.mark.parametrize("n", (65, 130, 1021))
def test_knobs_change_nothing(apd, ctx, n):
    for kind in ("ties", "special"):
        for link in (EITHER, BOTH):
            for min_pts in (2, 9):
                d, want = case(kind, n, link, min_pts)
                for knobs in (dict(APD_DENSITY_TREE_WORKSPACE_BYTES=1), dict(APD_DENSITY_TREE_WORKSPACE_BYTES=3 * 4 * ((n + 3) & ~3)),
                              dict(APD_DENSITY_TREE_WORKGROUP=64), dict(APD_DENSITY_TREE_WORKGROUP=1024),
                              dict(APD_DENSITY_TREE_WORKSPACE_BYTES=70 * 4 * ((n + 3) & ~3), APD_DENSITY_TREE_WORKGROUP=128)):
                    if n > 200 and knobs.get("APD_DENSITY_TREE_WORKSPACE_BYTES") == 1 and (kind, link) != ("ties", EITHER):
                        continue                                              # a launch per row: once is enough at this size
                    with environment(**knobs):
                        what = "%s n %d link %d min_pts %d %r" % (kind, n, link, min_pts, knobs)
                        assert_same(run(d, min_pts, link, ctx), want, what)
                        assert_same(run(d, min_pts, link, ctx, on_device=True), want, "on_device, " + what)


def test_padding_and_raw_outputs(apd, ctx):
    """The C entry point itself: the slots behind n_edges, the host words, n = 0 and n = 1."""
    d, want = case("special", 130, BOTH, 2)
    n = 130
    core, ei, ej, w = np.zeros(n, F), np.zeros(n - 1, np.uint32), np.zeros(n - 1, np.uint32), np.zeros(n - 1, F)
    n_edges, nans = C.c_uint32(77), C.c_uint64(77)
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    f = apd.lib().apd_density_tree
    assert f(ctx.handle, p(d), 0, n, BOTH, 2, p(core), p(ei), p(ej), p(w), C.byref(n_edges), C.byref(nans)) == apd.APD_OK
    e = n_edges.value
    assert e == len(want[1]) < n - 1 and nans.value == want[4]
    assert_same((core, ei[:e], ej[:e], w[:e], nans.value), want, "raw")
    assert (ei[e:] == 0xFFFFFFFF).all() and (ej[e:] == 0xFFFFFFFF).all() and (w[e:].view(np.uint32) == 0x7FC00000).all()
    assert (core.view(np.uint32)[np.isnan(core)] == 0x7FC00000).all() and np.isnan(core).any()
    one, alone = np.full(1, 5.0, F), np.zeros((1, 1), F)
    for min_pts, bits in ((1, 0xFF800000), (2, 0x7FC00000)):
        n_edges.value, nans.value = 77, 77
        assert f(ctx.handle, p(alone), 0, 1, EITHER, min_pts, p(one), None, None, None, C.byref(n_edges), C.byref(nans)) == apd.APD_OK
        assert one.view(np.uint32)[0] == bits and n_edges.value == 0 and nans.value == 0
    n_edges.value, nans.value = 77, 77
    assert f(ctx.handle, None, 0, 0, EITHER, 3, None, None, None, None, C.byref(n_edges), C.byref(nans)) == apd.APD_OK
    assert n_edges.value == 0 and nans.value == 0 and rounds_of(apd, ctx)[0] == 0


def test_invalid_arguments_leave_the_outputs_untouched(apd, ctx):
    d, _ = case("blobs", 65, EITHER, 2)
    n = 65
    outs = [np.full(n, 0x5A5A5A5A, np.uint32) for _ in range(4)]
    n_edges, nans = C.c_uint32(77), C.c_uint64(77)
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    ptrs = [p(o) for o in outs]
    without = lambda k: [None if j == k else q for j, q in enumerate(ptrs)]
    f = apd.lib().apd_density_tree
    words = (C.byref(n_edges), C.byref(nans))
    calls = {"link 2": (ctx.handle, p(d), 0, n, 2, 2, *ptrs, *words), "link -1": (ctx.handle, p(d), 0, n, -1, 2, *ptrs, *words),
             "a min_pts of 0": (ctx.handle, p(d), 0, n, 0, 0, *ptrs, *words), "no context": (None, p(d), 0, n, 0, 2, *ptrs, *words),
             "no matrix": (ctx.handle, None, 0, n, 0, 2, *ptrs, *words), "no core": (ctx.handle, p(d), 0, n, 0, 2, *without(0), *words),
             "no edge_i": (ctx.handle, p(d), 0, n, 1, 2, *without(1), *words), "no edge_j": (ctx.handle, p(d), 0, n, 0, 2, *without(2), *words),
             "no weight": (ctx.handle, p(d), 0, n, 0, 1, *without(3), *words), "no n_edges": (ctx.handle, p(d), 0, n, 0, 2, *ptrs, None, words[1]),
             "no nans": (ctx.handle, p(d), 0, n, 0, 2, *ptrs, words[0], None)}
    for what, args in calls.items():
        assert f(*args) == apd.APD_ERR_INVALID_ARG, what
        assert all((o == 0x5A5A5A5A).all() for o in outs) and n_edges.value == 77 and nans.value == 77, what
    assert f(ctx.handle, p(d), 0, (1 << 21) + 1, 0, 2, *ptrs, *words) == apd.APD_ERR_UNSUPPORTED
    assert all((o == 0x5A5A5A5A).all() for o in outs) and n_edges.value == 77
    phase, rounds = (C.c_float * 3)(), C.c_uint32(0)
    assert apd.lib().apd_density_tree_last_profile(None, phase, C.byref(rounds)) == apd.APD_ERR_INVALID_ARG
    assert apd.lib().apd_density_tree_last_profile(ctx.handle, None, C.byref(rounds)) == apd.APD_ERR_INVALID_ARG


def test_profile_under_timing(apd, ctx):
    d, want = case("blobs", 200, EITHER, 9)
    ctx.set_timing(True)
    try:
        assert_same(run(d, 9, EITHER, ctx), want, "timing on")
        rounds, phase = rounds_of(apd, ctx)
        assert 1 <= rounds <= most_rounds(200) and all(ms > 0.0 for ms in phase) and ctx.last_kernel_ms() >= max(phase)
    finally:
        ctx.set_timing(False)


@pytest.mark.parametrize("link", ("either", "both"))
def test_cuts_equal_the_density_kernel_on_core_points(ctx, link):
    """The pinned property against the existing kernel, on the device: 16 eps values in two calls of eight settings."""
    from audio_pattern_discovery_amd.clustering import density, density_cut, density_tree
    d = blob_matrix(200, seed=200, asymmetric=True).copy()
    d[7, 100] = d[191, 0] = NAN
    for min_pts in (1, 5):
        tree = density_tree(d, min_pts, link=link, ctx=ctx)
        assert tree[4] == 2
        weights = np.unique(tree[3])
        eps = np.concatenate([weights[np.round(np.linspace(0, len(weights) - 1, 12)).astype(int)], F([-INF, 0.0, 0.31, INF])])
        labels, counts, kind = density_cut(tree, eps, details=True)
        (want_labels, want_counts), (want_kind, _, nans) = density(d, eps, min_pts, link=link, ctx=ctx, details=True)
        assert nans == 2 and len({tuple(lab) for lab in labels}) >= 8
        for s in range(16):
            core = want_kind[s] == CORE
            assert np.array_equal(kind[s] == CORE, core), (min_pts, eps[s])
            assert np.array_equal(labels[s][core], want_labels[s][core]), (min_pts, eps[s])
            assert counts[s][0] == want_counts[s][0] and counts[s][1] == want_counts[s][1]


def test_sweep_equals_its_parts(ctx):
    from audio_pattern_discovery_amd.clustering import density_cut, density_sweep, density_tree, silhouette
    d = blob_matrix(130, seed=130, asymmetric=True)
    tree = density_tree(d, 4, ctx=ctx)
    rows = density_sweep(d, 4, ctx=ctx)
    eps = np.unique(tree[3])
    assert len(eps) > 64 and len(rows) == 64 and rows[0][0] == eps[0] and rows[-1][0] == eps[-1]
    assert all(a[0] < b[0] and a[0] in eps for a, b in zip(rows, rows[1:]))
    for chosen, got in ((np.array([r[0] for r in rows], F), rows), (F([0.3, 0.1, INF]), density_sweep(d, 4, eps=[0.3, 0.1, INF], axis=1, ctx=ctx))):
        labels, counts = density_cut(tree, chosen)
        score, _, nans = silhouette(d, labels, axis=0 if got is rows else 1, ctx=ctx)
        for c, row in enumerate(got):
            assert row[:4] == (float(chosen[c]), int(counts[c][0]), int(counts[c][1]), int(counts[c][3])) and row[5] == int(nans[c])
            assert np.array_equal(F(row[4]).view(np.uint32), score[c].view(np.uint32)), (c, row, score[c])
    assert density_sweep(np.zeros((0, 0), F), 2, ctx=ctx) == []
    both = density_sweep(d, 4, eps=[0.3], link="both", ctx=ctx)
    assert both[0][1:4] == tuple(int(v) for v in density_cut(density_tree(d, 4, link="both", ctx=ctx), 0.3)[1][[0, 1, 3]])
