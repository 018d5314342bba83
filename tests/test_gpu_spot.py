"""GPU tests of the subsequence alignment (apd_spot, apd_spot_hits) against the checker tests/_spot_reference.py.

Every comparison is bitwise: start equal, cost and every field of `best` equal as uint32 (NaN payloads aside: _path_reference.bits
says why).  Shapes are the smallest that reach each code path of the kernels (csrc/dtw_spot.hip): R = 1 .. 4 query rows per lane
in registers, R >= 5 in LDS, lane and row-block edges of the query (63 / 64 / 65, 128 / 130, 256 / 257), streams shorter than one
wavefront and shorter than the query, every instantiated frame dimension and one without kernels of its own, lane columns beyond
64 KB of LDS, and a pair list cut into several workspace chunks."""
import ctypes as C
import os

import numpy as np
import pytest

import _kernel_table as kt
import _spot_reference as ref

pytestmark = pytest.mark.gpu
UNIT = (1.0, 1.0, 1.0)
SKEWED = (1.0, 2.0, 0.5)                        # (insertion, deletion, match)
F = np.float32


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


def raw_spot(apd, ctx, batch, pen, pairs, curves=True):
    """apd_spot through ctypes: (list of (cost, start) per pair -- empty without curves --, best records, curve_off)."""
    L = apd.lib()
    cfg = apd.AlignConfig(float("nan"), pen[0], pen[1], pen[2])                 # the band percentage is not read
    pr = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
    n_pairs = len(pr)
    u32p, u64p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_float)
    head = (ctx.handle, batch.handle, C.byref(cfg), pr.ctypes.data_as(u32p), n_pairs)
    off = np.full(n_pairs + 1, 77, dtype=np.uint64)
    apd.check(L.apd_spot(*head, None, None, 0, off.ctypes.data_as(u64p), None), ctx.handle)      # sizes only
    best = np.full((n_pairs + 1) * 16, 0x55, dtype=np.uint8).view(ref.BEST)                       # one record more than asked: a canary
    bestp = best.ctypes.data_as(C.POINTER(apd.SpotBest))
    off2 = np.zeros(n_pairs + 1, dtype=np.uint64)
    if not curves:
        apd.check(L.apd_spot(*head, None, None, 0, off2.ctypes.data_as(u64p), bestp), ctx.handle)
        assert np.array_equal(off, off2) and best[-1]["end"] == 0x55555555
        return [], best[:n_pairs].copy(), off
    total = int(off[-1])
    cost = np.full((total + 1) * 4, 0x55, dtype=np.uint8).view(F)
    start = np.full(total + 1, 0x55555555, dtype=np.uint32)
    apd.check(L.apd_spot(*head, cost.ctypes.data_as(f32p), start.ctypes.data_as(u32p), total, off2.ctypes.data_as(u64p), bestp), ctx.handle)
    assert np.array_equal(off, off2)
    assert best[-1]["end"] == 0x55555555 and start[-1] == 0x55555555 and cost.view(np.uint32)[-1] == 0x55555555   # nothing past the capacity
    out = [(cost[int(off[p]):int(off[p + 1])].copy(), start[int(off[p]):int(off[p + 1])].copy()) for p in range(n_pairs)]
    return out, best[:n_pairs].copy(), off


_REFERENCE = {}


def reference(key, seqs, pen, x, y):
    """The checker's (cost, start, best) of query x against stream y of `seqs`, computed once per (key, penalties, pair)."""
    k = (key, pen, x, y)
    if k not in _REFERENCE:
        _REFERENCE[k] = ref.spot(seqs[x], seqs[y], *pen)
    return _REFERENCE[k]


def assert_same(got_curves, got_best, want, what=""):
    want_cost, want_start, want_best = want
    if got_curves is not None:
        cost, start = got_curves
        assert len(cost) == len(want_cost) and len(start) == len(want_start), what
        assert np.array_equal(start, want_start), (what, "start")
        assert np.array_equal(ref.bits(cost), ref.bits(want_cost)), (what, "cost")
    assert ref.same_best(got_best, want_best), (what, got_best, want_best)


def check_batch(apd, ctx, key, seqs, pen, pairs, batch=None):
    own = batch is None
    batch = batch or make_batch(ctx, seqs)
    try:
        got, best, off = raw_spot(apd, ctx, batch, pen, pairs)
    finally:
        if own:
            batch.close()
    for p, (x, y) in enumerate(pairs):
        assert int(off[p + 1] - off[p]) == len(seqs[y])
        assert_same(got[p], best[p], reference(key, seqs, pen, x, y), "%s pair (%d, %d)" % (key, x, y))
    return got, best


def gauss_seqs(lengths, dim, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((n, dim)).astype(F) for n in lengths]


def integer_seqs(lengths, dim, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 3, (n, dim)).astype(F) for n in lengths]


def col(values):
    return np.array(values, dtype=F).reshape(-1, 1)


HAND = ((col([1, 2]), col([5, 1, 2, 5]), [7.0, 1.0, 0.0, 3.0], [1, 2, 2, 2]),
        (col([0, 1]), col([0, 1, 0]), [1.0, 0.0, 2.0], [1, 1, 2]))                # the tie quirk: (2, 3) takes MATCH although larger


def test_hand_cases_through_both_entry_points(apd, ctx):
    from audio_pattern_discovery_amd.alignments import SPOT_BEST, AlignmentWorkers, NDSequence
    from audio_pattern_discovery_amd.discovery import Discovery
    for x, y, want_cost, want_start in HAND:
        batch = make_batch(ctx, [x, y])
        got, best, _ = raw_spot(apd, ctx, batch, UNIT, [(0, 1)])
        batch.close()
        assert got[0][0].tolist() == want_cost and got[0][1].tolist() == want_start
        workers = AlignmentWorkers.new([NDSequence(x), NDSequence(y)], ctx)
        try:
            curves, mine = workers.spot([(0, 1)], Discovery())
            _, alone = workers.spot([(0, 1)], Discovery(), curves=False)
        finally:
            workers.close()
        assert curves[0][0].tolist() == want_cost and curves[0][1].tolist() == want_start
        assert mine.dtype == SPOT_BEST and ref.same_best(mine, best) and ref.same_best(alone, best)
    batch = make_batch(ctx, [HAND[0][0], HAND[0][1]])
    _, best, _ = raw_spot(apd, ctx, batch, UNIT, [(0, 1)])
    batch.close()
    assert (int(best[0]["end"]), int(best[0]["start"]), float(best[0]["cost"]), float(best[0]["score"])) == (3, 2, 0.0, 0.0)


QUERY_LENGTHS = (1, 2, 63, 64, 65, 128, 130)      # R = 1, 2, 3 rows per lane in registers (D = 13); last lane full, one row over, one lane over
STREAM_LENGTHS = (1, 2, 63, 64, 65, 200)


def test_lane_and_row_block_edges(apd, ctx):
    seqs = gauss_seqs(QUERY_LENGTHS + STREAM_LENGTHS, 13, 101)
    nq = len(QUERY_LENGTHS)
    pairs = [(q, nq + s) for q in range(nq) for s in range(len(STREAM_LENGTHS))]
    assert any(len(seqs[y]) < len(seqs[x]) for x, y in pairs)
    got, best = check_batch(apd, ctx, "edges", seqs, UNIT, pairs)
    assert all(np.all(s >= 1) and np.all(s <= np.arange(1, len(s) + 1)) for _, s in got)
    assert np.all(best["end"] >= 1) and np.all(np.isfinite(best["score"]))


def test_rows_in_registers_and_in_lds(apd, ctx, capfd):
    """R = 3, 4 (registers), R = 5 (the first query length whose lane columns live in LDS), and the row-block edges around them."""
    seqs = gauss_seqs((192, 256, 257, 320, 70, 33), 13, 102)
    with kt.debug_plan(capfd) as err:
        check_batch(apd, ctx, "classes", seqs, UNIT, [(q, s) for q in range(4) for s in (4, 5)])
    assert kt.read_spot_plan(err[0]) == {("sweep", 3, 13): 2, ("sweep", 4, 13): 2, ("sweep", 0, 13): 4}, err[0]
    with kt.debug_plan(capfd) as err:
        check_batch(apd, ctx, "classes", seqs, SKEWED, [(1, 4), (2, 5)])
    assert kt.read_spot_plan(err[0]) == {("sweep", 4, 13): 1, ("sweep", 0, 13): 1}, err[0]


@pytest.mark.parametrize("dim", [1, 13])
@pytest.mark.parametrize("pen", [UNIT, SKEWED])
def test_integer_ties(apd, ctx, dim, pen):
    seqs = integer_seqs((5, 66, 130, 40, 100), dim, 110 + dim)
    check_batch(apd, ctx, "ties%d" % dim, seqs, pen, [(q, s) for q in range(3) for s in (3, 4)])


@pytest.mark.parametrize("dim", [3, 8, 10, 13, 16, 20, 26, 40])
def test_dimensions(apd, ctx, dim):
    seqs = gauss_seqs((70, 150), dim, 120 + dim)
    check_batch(apd, ctx, "dim%d" % dim, seqs, UNIT, [(0, 1)])


def test_dimension_without_kernels_of_its_own_with_a_long_query(apd, ctx, capfd):
    seqs = gauss_seqs((330, 20), 40, 125)                                      # D = 40: frames re-read per cell, R = 6 in LDS
    with kt.debug_plan(capfd) as err:
        check_batch(apd, ctx, "dim40long", seqs, SKEWED, [(0, 1), (1, 0)])     # the 20-frame query too: one launch, LDS for R = 6
    assert kt.read_spot_plan(err[0]) == {("sweep", 0, 0): 2}, err[0]
    assert [(v["r_max"], v["lds"]) for v in kt.read_spot_launches(err[0])] == [(6, 6 * 64 * 8)]


def test_embedded_copies(apd, ctx):
    from audio_pattern_discovery_amd.alignments import spot_hits
    rng = np.random.default_rng(130)
    query = rng.standard_normal((40, 13)).astype(F)
    noise = [rng.standard_normal((k, 13)).astype(F) for k in (30, 25, 20)]
    stream = np.concatenate([noise[0], query, noise[1], query, noise[2]], axis=0)
    got, best = check_batch(apd, ctx, "copies", [query, stream], UNIT, [(0, 1)])
    cost, start = got[0]
    for end, first in ((70, 31), (135, 96)):
        assert cost[end - 1].view(np.uint32) == 0 and start[end - 1] == first  # exactly +0.0 at the copy's end, its exact start
    assert (int(best[0]["end"]), int(best[0]["start"])) == (70, 31) and best[0]["score"] == 0.0
    hits = spot_hits(cost, start, len(query), 1e-6)
    assert [(int(h["end"]), int(h["start"])) for h in hits] == [(70, 31), (135, 96)] and not hits["score"].any()
    assert ref.same_best(hits, ref.hits(cost, start, len(query), 1e-6))
    loose = spot_hits(cost, start, len(query), 1e9)                             # every column a candidate: a cover of disjoint windows
    assert ref.same_best(loose, ref.hits(cost, start, len(query), 1e9)) and ref.same_best(loose[:2], hits)
    spans = sorted((int(h["start"]), int(h["end"])) for h in loose)
    assert all(a[1] < b[0] for a, b in zip(spans[:-1], spans[1:]))


def test_prefix_property(apd, ctx):
    """Column j depends on columns <= j only: the curves of y[:k] are the first k entries of the curves of y, bit for bit."""
    x, y = gauss_seqs((70, 150), 13, 140)
    cuts = (1, 63, 64, 65)
    seqs = [x, y] + [y[:k] for k in cuts]
    got, _ = check_batch(apd, ctx, "prefix", seqs, UNIT, [(0, 1)])
    batch = make_batch(ctx, seqs)
    parts, _, _ = raw_spot(apd, ctx, batch, UNIT, [(0, 2 + t) for t in range(len(cuts))])
    batch.close()
    for k, (cost, start) in zip(cuts, parts):
        assert np.array_equal(cost.view(np.uint32), got[0][0][:k].view(np.uint32)) and np.array_equal(start, got[0][1][:k])


def test_pair_list_order_repeats_and_a_joined_batch(apd, ctx):
    from audio_pattern_discovery_amd.alignments import AlignmentWorkers, Batch, NDSequence
    from audio_pattern_discovery_amd.discovery import Discovery
    templates = gauss_seqs((20, 66, 9), 13, 150)
    streams = gauss_seqs((90, 45, 130, 70), 13, 151)
    seqs = templates + streams
    pairs = [(1, 5), (0, 3), (2, 6), (1, 5), (4, 4), (0, 0), (3, 1), (2, 3), (1, 4), (0, 6)]     # repeats, x == y, a stream as query
    got, best = check_batch(apd, ctx, "list", seqs, UNIT, pairs)                                  # a plain batch of all seven
    assert np.array_equal(got[0][0].view(np.uint32), got[3][0].view(np.uint32)) and ref.same_best(best[0], best[3])
    assert not got[4][0][-1] and best[4]["score"] == 0.0 and int(best[4]["start"]) == 1          # x == y: the diagonal, cost 0 at the end
    a, b = make_batch(ctx, templates), make_batch(ctx, streams)
    joined = Batch.join(a, b)
    try:
        got_j, best_j = check_batch(apd, ctx, "list", seqs, UNIT, pairs, batch=joined)
    finally:
        joined.close()
        a.close()
        b.close()
    assert ref.same_best(best_j, best)
    wa, wb = AlignmentWorkers.new([NDSequence(s) for s in templates], ctx), AlignmentWorkers.new([NDSequence(s) for s in streams], ctx)
    try:
        mine, mine_best = wa.spot(pairs, Discovery(), streams=wb)
    finally:
        wa.close()
        wb.close()
    assert ref.same_best(mine_best, best)
    for p in range(len(pairs)):
        assert np.array_equal(mine[p][0].view(np.uint32), got[p][0].view(np.uint32)) and np.array_equal(mine[p][1], got[p][1])


@pytest.fixture(scope="module")
def mixed():
    """Queries of every kernel class against three streams: the list the mode / chunk / best-only / refill tests share."""
    lengths = (30, 100, 150, 250, 300, 120, 61, 95)
    seqs = gauss_seqs(lengths, 13, 160)
    pairs = [(q, s) for q in range(5) for s in (5, 6, 7)] + [(5, 6), (2, 2)]
    return lengths, seqs, pairs


def test_best_only_equals_best_with_curves(apd, ctx, mixed):
    _, seqs, pairs = mixed
    batch = make_batch(ctx, seqs)
    try:
        _, with_curves = check_batch(apd, ctx, "mixed", seqs, UNIT, pairs, batch=batch)
        none, alone, _ = raw_spot(apd, ctx, batch, UNIT, pairs, curves=False)
    finally:
        batch.close()
    assert none == [] and ref.same_best(alone, with_curves)
    assert np.array_equal(alone.view(np.uint32), with_curves.view(np.uint32))


def test_bits_do_not_depend_on_the_distance_mode(apd, ctx, mixed):
    _, seqs, pairs = mixed
    batch = make_batch(ctx, seqs)
    results = []
    try:
        for mode in (0, 1, 2):
            ctx.set_distance_mode(mode)
            results.append(raw_spot(apd, ctx, batch, UNIT, pairs))
    finally:
        ctx.set_distance_mode("hybrid")
        batch.close()
    for p, (x, y) in enumerate(pairs):
        assert_same(results[0][0][p], results[0][1][p], reference("mixed", seqs, UNIT, x, y))
    for got, best, _ in results[1:]:
        assert np.array_equal(best.view(np.uint32), results[0][1].view(np.uint32))
        for (c, s), (c0, s0) in zip(got, results[0][0]):
            assert np.array_equal(c.view(np.uint32), c0.view(np.uint32)) and np.array_equal(s, s0)


def test_outside_the_feature_range(apd, ctx):
    """A NaN frame, an infinite one and a 2^-60 one inside a stream: no routing needed, the arithmetic is the literal one anyway."""
    base = gauss_seqs((20, 70, 90, 90, 90), 13, 170)
    seqs = [s.copy() for s in base]
    seqs[2][40, :] = np.nan
    seqs[2][41, 3] = np.nan
    seqs[3][17, 5] = np.inf
    seqs[3][60, :] = -np.inf
    seqs[4][30, :] *= F(2.0 ** -60)
    seqs[4][31:34, :] = F(2.0 ** -60)
    batch = make_batch(ctx, seqs)
    flag = C.c_int(0)
    apd.check(apd.lib().apd_batch_nonfinite(ctx.handle, batch.handle, C.byref(flag)), ctx.handle)
    assert flag.value == 1
    try:
        got, best = check_batch(apd, ctx, "range", seqs, UNIT, [(q, s) for q in (0, 1) for s in (2, 3, 4)], batch=batch)
        check_batch(apd, ctx, "range", seqs, SKEWED, [(0, 2), (1, 3)], batch=batch)
    finally:
        batch.close()
    assert np.isnan(got[0][0]).any() and np.isfinite(got[0][0]).any()          # the NaN frame poisons columns, not the whole curve
    assert np.all(np.isfinite(best["score"]))                                  # a NaN column is never the best
    assert np.isinf(got[1][0]).any() or np.isnan(got[1][0]).any()


def test_chunked_equals_unchunked(apd, ctx, mixed):
    _, seqs, pairs = mixed
    batch = make_batch(ctx, seqs)
    whole, whole_best, _ = raw_spot(apd, ctx, batch, UNIT, pairs)
    need = 8 * sum(len(seqs[y]) for _, y in pairs)                             # 8 bytes per curve entry (include/apd.h)
    cap = need // 4
    assert need / cap >= 3
    os.environ["APD_SPOT_WORKSPACE_BYTES"] = str(cap)
    try:
        parts, part_best, _ = raw_spot(apd, ctx, batch, UNIT, pairs)
        os.environ["APD_SPOT_WORKSPACE_BYTES"] = "1"                           # one pair per chunk
        ones, one_best, _ = raw_spot(apd, ctx, batch, UNIT, pairs)
    finally:
        del os.environ["APD_SPOT_WORKSPACE_BYTES"]
        batch.close()
    for other, other_best in ((parts, part_best), (ones, one_best)):
        assert np.array_equal(other_best.view(np.uint32), whole_best.view(np.uint32))
        for (c, s), (c0, s0) in zip(other, whole):
            assert np.array_equal(c.view(np.uint32), c0.view(np.uint32)) and np.array_equal(s, s0)
    for p, (x, y) in enumerate(pairs):
        assert_same(parts[p], part_best[p], reference("mixed", seqs, UNIT, x, y))


def test_spot_follows_a_refill(apd, ctx, mixed):
    lengths, seqs, _ = mixed
    fresh = gauss_seqs(lengths, 13, 180)
    pairs = [(0, 5), (3, 6), (4, 7)]
    batch = make_batch(ctx, seqs)
    try:
        before, _ = check_batch(apd, ctx, "mixed", seqs, UNIT, pairs, batch=batch)
        frames = np.ascontiguousarray(np.concatenate(fresh, axis=0))
        apd.check(apd.lib().apd_batch_refill(ctx.handle, batch.handle, C.c_void_p(frames.ctypes.data), 0), ctx.handle)
        after, _ = check_batch(apd, ctx, "refilled", fresh, UNIT, pairs, batch=batch)
    finally:
        batch.close()
    assert before[0][0].tobytes() != after[0][0].tobytes()


def test_a_long_query(apd, ctx, capfd):
    seqs = gauss_seqs((4096, 96), 13, 190)                                     # R = 64 rows per lane, 32 KB of LDS
    with kt.debug_plan(capfd) as err:
        check_batch(apd, ctx, "long", seqs, UNIT, [(0, 1)])
    assert [(v["kind"], v["rt"], v["d"], v["r_max"], v["lds"]) for v in kt.read_spot_launches(err[0])] == [("sweep", 0, 13, 64, 32 * 1024)]


def test_lane_columns_beyond_64_kib_of_lds_and_the_longest_query(apd, ctx, capfd):
    """dim = 1 is resident as D = 8: kernel <0, 8>.  R = 256 is the limit; both pairs go in ONE launch, sized for the longer query
    (128 KB), so the R = 129 pair is also run alone: 64.5 KB, the smallest size the launch has to ask for."""
    seqs = gauss_seqs((8200, 16384, 3, 2), 1, 191)
    with kt.debug_plan(capfd) as err:
        check_batch(apd, ctx, "lds", seqs, UNIT, [(0, 2), (1, 3)])
    d = kt.kernel_dim(1)
    assert [(v["kind"], v["rt"], v["d"], v["pairs"], v["r_max"], v["lds"]) for v in kt.read_spot_launches(err[0])] == [("sweep", 0, d, 2, 256, 128 * 1024)]
    with kt.debug_plan(capfd) as err:
        check_batch(apd, ctx, "lds", seqs, UNIT, [(0, 2)])
    assert [(v["kind"], v["rt"], v["d"], v["pairs"], v["r_max"], v["lds"]) for v in kt.read_spot_launches(err[0])] == [("sweep", 0, d, 1, 129, 129 * 512)]


def test_timing_covers_the_call(apd, ctx, mixed):
    _, seqs, pairs = mixed
    batch = make_batch(ctx, seqs)
    ctx.set_timing(True)
    try:
        raw_spot(apd, ctx, batch, UNIT, pairs, curves=False)
        assert ctx.last_kernel_ms() > 0.0
    finally:
        ctx.set_timing(False)
        batch.close()


def test_size_query_and_argument_errors(apd, ctx):
    L = apd.lib()
    seqs = gauss_seqs((12, 40, 25), 13, 195)
    batch = make_batch(ctx, seqs)
    cfg = apd.AlignConfig(1.0, 1.0, 1.0, 1.0)
    u32p, u64p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_float)
    pairs = np.array([(0, 1), (2, 2), (0, 2)], dtype=np.uint32)
    off = np.zeros(4, dtype=np.uint64)
    cost, start = np.zeros(90, dtype=F), np.zeros(90, dtype=np.uint32)
    best = np.zeros(3, dtype=ref.BEST)
    head = (ctx.handle, batch.handle, C.byref(cfg), pairs.ctypes.data_as(u32p), 3)
    costp, startp, offp, bestp = cost.ctypes.data_as(f32p), start.ctypes.data_as(u32p), off.ctypes.data_as(u64p), best.ctypes.data_as(C.POINTER(apd.SpotBest))

    def idle():
        return not ctx.stream_busy()

    try:
        ctx.synchronize()
        assert L.apd_spot(*head, None, None, 0, offp, None) == apd.APD_OK and off.tolist() == [0, 40, 65, 90]     # the size query
        assert L.apd_spot(*head, costp, startp, 89, offp, bestp) == apd.APD_ERR_INVALID_ARG and idle()            # capacity one short
        assert L.apd_spot(*head, costp, None, 90, offp, bestp) == apd.APD_ERR_INVALID_ARG and idle()              # exactly one curve NULL
        assert L.apd_spot(*head, None, startp, 90, offp, bestp) == apd.APD_ERR_INVALID_ARG and idle()
        assert L.apd_spot(*head, costp, startp, 90, None, bestp) == apd.APD_ERR_INVALID_ARG and idle()
        bad = np.array([(0, 1), (3, 0)], dtype=np.uint32)                                                         # index = n_seq
        assert L.apd_spot(ctx.handle, batch.handle, C.byref(cfg), bad.ctypes.data_as(u32p), 2, costp, startp, 90, offp, bestp) == apd.APD_ERR_INVALID_ARG
        assert idle()
        assert L.apd_spot(ctx.handle, batch.handle, C.byref(cfg), None, 0, costp, startp, 0, offp, bestp) == apd.APD_OK and off[0] == 0
        assert L.apd_spot(*head, costp, startp, 90, offp, None) == apd.APD_OK                                     # best may be NULL with curves
        assert L.apd_spot(*head, None, None, 0, offp, bestp) == apd.APD_OK                                        # best only
        want = [reference("errors", seqs, UNIT, int(x), int(y)) for x, y in pairs]
        for p in range(3):
            assert_same((cost[int(off[p]):int(off[p + 1])], start[int(off[p]):int(off[p + 1])]), best[p], want[p])
    finally:
        batch.close()
    # an empty sequence in the batch, a query beyond the documented limit: refused before anything is launched
    from audio_pattern_discovery_amd.alignments import Batch
    frames = np.zeros((16385 + 5, 1), dtype=F)
    empty = Batch(ctx, frames[:9], np.array([0, 4, 4, 9], dtype=np.uint64), 1)
    long_ = Batch(ctx, frames, np.array([0, 16385, 16390], dtype=np.uint64), 1)
    one = np.array([(0, 2)], dtype=np.uint32)
    try:
        ctx.synchronize()
        assert L.apd_spot(ctx.handle, empty.handle, C.byref(cfg), one.ctypes.data_as(u32p), 1, None, None, 0, offp, bestp) == apd.APD_ERR_EMPTY_SEQUENCE
        assert idle()
        one[0] = (0, 1)
        assert L.apd_spot(ctx.handle, long_.handle, C.byref(cfg), one.ctypes.data_as(u32p), 1, None, None, 0, offp, bestp) == apd.APD_ERR_UNSUPPORTED
        assert idle()
        one[0] = (1, 0)                                                                                           # the other way round runs: m is not limited
        assert L.apd_spot(ctx.handle, long_.handle, C.byref(cfg), one.ctypes.data_as(u32p), 1, None, None, 0, offp, bestp) == apd.APD_OK
        assert best[0]["score"] == 0.0 and int(best[0]["end"]) == 1                                               # all-zero frames: cost 0 in every column
    finally:
        empty.close()
        long_.close()
