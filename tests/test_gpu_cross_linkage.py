"""apd_cross_linkage: the reference's average linkage (clustering.rs:153-170) of every first-set sequence to sets of the second, and
merge()'s choice among them (clustering.rs:178-187), bit for bit against the sequential numpy-f32 loop of tests/_linkage_reference.py."""
import ctypes as C

import numpy as np
import pytest

from audio_pattern_discovery_amd import synth
from _linkage_reference import F, NONE, assert_equal, reference, reference_over_q, same_bits, six_set_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(apd):
    c = apd.Context(0)
    yield c
    c.close()


def test_linkage_matches_the_sequential_loop_bitwise(ctx, apd):
    from audio_pattern_discovery_amd.clustering import cross_linkage
    fs, sf, sets = six_set_case()
    n1, n2 = fs.shape
    want = reference(fs, sf, sets)
    listed = reference(fs, sf, sets, ascending=False)
    n_link = n1 * len(sets)                                           # 222 linkages per direction
    moved = [int((want[d].view(np.uint32) != listed[d].view(np.uint32)).sum()) for d in (0, 1)]
    pairwise = sum(int(F(np.sum(fs[q, sorted(s)])) / F(len(s)) != want[0][q, k]) for k, s in enumerate(sets) for q in range(n1))
    print("of %d linkages, summing in listed order changes %d (fs) and %d (sf), a pairwise np.sum %d (fs)" % (n_link, moved[0], moved[1], pairwise))
    assert min(moved) >= n_link // 4                                  # so a kernel that sums in any other order fails below
    assert_equal(cross_linkage(fs, sf, sets, ctx), want, "six sets")

    # an empty set: 0 / 0 = NaN, never chosen
    with_empty = [sets[2], [], sets[0]]
    got = cross_linkage(fs, sf, with_empty, ctx)
    assert np.isnan(got[0][:, 1]).all() and np.isnan(got[1][:, 1]).all() and not np.any(got[2] == 1)
    assert_equal(got, reference(fs, sf, with_empty), "an empty set")

    # a set holding a +INF entry; every entry +INF
    fs_inf, sf_inf = fs.copy(), sf.copy()
    fs_inf[:, sets[2][3]] = np.inf
    sf_inf[sets[3][7], :] = np.inf
    assert_equal(cross_linkage(fs_inf, sf_inf, sets, ctx), reference(fs_inf, sf_inf, sets), "+INF members")
    all_inf = cross_linkage(np.full_like(fs, np.inf), np.full_like(sf, np.inf), sets, ctx)
    assert np.all(all_inf[2] == NONE) and np.all(np.isposinf(all_inf[3]))

    # exact ties: link_fs[q][k] == link_sf[q][k] and two equal sets -- the first scanned wins (k ascending, fs before sf)
    fs_t, sf_t = np.full((n1, n2), 2.0, F), np.full((n2, n1), 2.0, F)
    tie_sets = [[5, 9, 1], [7, 3], [2]]
    got = cross_linkage(fs_t, sf_t, tie_sets, ctx)
    assert np.all(got[0] == 2.0) and np.all(got[1] == 2.0) and np.all(got[2] == 0) and np.all(got[3] == 2.0)
    sf_t[2, :] = 1.0                                                  # only (S_2, {q}) is lower: the later, lower value wins
    got = cross_linkage(fs_t, sf_t, tie_sets, ctx)
    assert np.all(got[2] == 2) and np.all(got[3] == 1.0)
    assert_equal(got, reference(fs_t, sf_t, tie_sets), "ties")

    # n_sets = 0
    got = cross_linkage(fs, sf, [], ctx)
    assert got[0].shape == (n1, 0) and np.all(got[2] == NONE) and np.all(np.isposinf(got[3]))

    # a member >= n_second
    with pytest.raises(apd.ApdError) as e:
        cross_linkage(fs, sf, [[1, n2]], ctx)
    assert e.value.status == apd.APD_ERR_INVALID_ARG

    # the device form: matrices and results in HBM, the same bits
    members = np.array([m for s in sets for m in s], np.uint32)
    set_off = np.zeros(len(sets) + 1, np.uint32)
    set_off[1:] = np.cumsum([len(s) for s in sets])
    d_fs, d_sf = ctx.upload(fs), ctx.upload(sf)
    d_lf, d_ls, d_near, d_best = (ctx.alloc(4 * n1 * len(sets)), ctx.alloc(4 * n1 * len(sets)), ctx.alloc(4 * n1), ctx.alloc(4 * n1))
    u32p = C.POINTER(C.c_uint32)
    apd.check(apd.lib().apd_cross_linkage(ctx.handle, d_fs.at(), d_sf.at(), 1, n1, n2, members.ctypes.data_as(u32p), set_off.ctypes.data_as(u32p),
                                          len(sets), d_lf.at(), d_ls.at(), d_near.at(), d_best.at()), ctx.handle)
    ctx.synchronize()
    dev = (d_lf.to_numpy(F).reshape(n1, -1), d_ls.to_numpy(F).reshape(n1, -1), d_near.to_numpy(np.uint32), d_best.to_numpy(F))
    assert_equal(dev, want, "device form")
    for b in (d_fs, d_sf, d_lf, d_ls, d_near, d_best):
        b.free()


def test_three_query_blocks_and_more_sets_than_the_grid_has_rows(ctx, apd):
    """cross_linkage_kernel / cross_nearest_kernel run one lane per first-set sequence q, 64 to a block, and stride the sets by
    gridDim.y = min(n_sets, 16384).  n_first = 130: three blocks, the last with two lanes, rows of `link` at q >= 64;
    n_sets = 16384 + 3: sets 16384 .. 16386 are a block's second trip.  Sets of 0, 1, 2 and 3 members in turn, drawn with repeats
    across sets and listed unsorted; the host form and the device form, against the loop with q as the array axis."""
    from audio_pattern_discovery_amd.clustering import cross_linkage
    six = six_set_case()
    assert_equal(reference_over_q(*six), reference(*six), "the loop over q as an array, on the six sets")
    rng = np.random.default_rng(20240608)
    n1, n2, n_sets = 130, 50, 16384 + 3
    fs = (rng.random((n1, n2), dtype=F) * F(9.0) + F(0.01)).astype(F)
    sf = (rng.random((n2, n1), dtype=F) * F(9.0) + F(0.01)).astype(F)
    sets = [[int(v) for v in rng.choice(n2, size=k % 4, replace=False)] for k in range(n_sets)]
    assert any(s != sorted(s) for s in sets) and [len(s) for s in sets[-3:]] == [0, 1, 2]
    want = reference_over_q(fs, sf, sets)
    assert len(set(want[2].tolist())) > 20 and NONE not in want[2]               # the scan's choice differs from lane to lane
    assert_equal(cross_linkage(fs, sf, sets, ctx), want, "130 x 16387, host form")

    members = np.array([m for s in sets for m in s], np.uint32)
    set_off = np.zeros(n_sets + 1, np.uint32)
    set_off[1:] = np.cumsum([len(s) for s in sets])
    d_fs, d_sf = ctx.upload(fs), ctx.upload(sf)
    d_lf, d_ls, d_near, d_best = (ctx.alloc(4 * n1 * n_sets), ctx.alloc(4 * n1 * n_sets), ctx.alloc(4 * n1), ctx.alloc(4 * n1))
    u32p = C.POINTER(C.c_uint32)
    try:
        apd.check(apd.lib().apd_cross_linkage(ctx.handle, d_fs.at(), d_sf.at(), 1, n1, n2, members.ctypes.data_as(u32p),
                                              set_off.ctypes.data_as(u32p), n_sets, d_lf.at(), d_ls.at(), d_near.at(), d_best.at()), ctx.handle)
        ctx.synchronize()
        dev = (d_lf.to_numpy(F).reshape(n1, -1), d_ls.to_numpy(F).reshape(n1, -1), d_near.to_numpy(np.uint32), d_best.to_numpy(F))
    finally:
        for b in (d_fs, d_sf, d_lf, d_ls, d_near, d_best):
            b.free()
    assert_equal(dev, want, "130 x 16387, device form")


def test_queries_find_their_clusters_end_to_end(ctx, oracle, apd):
    """corpus -> align_all -> clustering -> cluster_sets, then queries -> cross -> cross_linkage, strict mode: the linkages are those of
    the numpy loop over the ORACLE's cross matrices, bit for bit, and nearest is identical."""
    from audio_pattern_discovery_amd.alignments import AlignmentWorkers, NDSequence
    from audio_pattern_discovery_amd.clustering import AgglomerativeClustering, cross_linkage
    from audio_pattern_discovery_amd.discovery import Discovery
    n2, nq, dim, pct = 40, 10, 13, 0.0625
    frames, offsets = synth.make_sequences(n2, 64, dim, seed=11, copies=0.5)
    corpus = synth.split(frames, offsets)
    rng = np.random.default_rng(5)
    queries = [synth._warp_copy(rng, corpus[int(rng.integers(0, n2))], int(rng.integers(62, 67))) for _ in range(nq)]
    params = Discovery(warping_band_percentage=pct)
    ctx.set_distance_mode("strict")
    try:
        wc, wq = AlignmentWorkers.new([NDSequence(s) for s in corpus], ctx), AlignmentWorkers.new([NDSequence(s) for s in queries], ctx)
        dist = wc.align_all(params).reshape(n2, n2).copy()
        ops, roots = AgglomerativeClustering.clustering(dist, n2, 0.3, ctx)
        sets = AgglomerativeClustering.cluster_sets(ops, roots, n2)
        assert len(sets) >= 2 and all(len(s) >= 2 for s in sets)
        fs, sf = wq.cross(wc, params)
    finally:
        ctx.set_distance_mode("hybrid")
    allf = np.concatenate(queries + corpus, axis=0)
    alloff = np.zeros(nq + n2 + 1, np.uint64)
    alloff[1:] = np.cumsum([len(s) for s in queries + corpus])
    q, c = np.meshgrid(np.arange(nq), np.arange(n2), indexing="ij")
    want_fs = oracle.align_sample(allf, alloff, q.ravel(), nq + c.ravel(), pct, workers=8)[0].reshape(nq, n2)
    want_sf = oracle.align_sample(allf, alloff, nq + c.T.ravel(), q.T.ravel(), pct, workers=8)[0].reshape(n2, nq)
    assert same_bits(fs, want_fs) and same_bits(sf, want_sf)
    assert_equal(cross_linkage(fs, sf, sets, ctx), reference(want_fs, want_sf, sets), "end to end")
    wc.close()
    wq.close()
