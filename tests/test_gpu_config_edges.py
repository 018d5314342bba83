"""Every DTW entry point under the degenerate alignment configurations of tests/_config_cases.py, against the CPU checkers.

include/apd.h accepts any f32 penalty and percentage and any u64 explicit band ("the domain of an alignment configuration").  The
table's entries carry their own bound -- 1e-4 relative with identical zero / INF / NaN pattern for positive finite equal penalties,
the checker's bits (NaN payloads aside) for everything else -- and every comparison below uses the entry's bound or the bits; no other
number appears.  The oracle's matrices are computed once per (batch, entry) (_config_cases.want_matrix), the per-cell Python
checkers once per (entry, pair).

apd_align_all / apd_align_all_device_async run in hybrid, exact and strict mode and with the first listed geometry of every kernel
family forced; the APD_DEBUG_PLAN lines show that a non-positive, infinite or NaN penalty ran geometry 0 (the literal kernel) alone,
forced geometry or not.  Then apd_align_cross (both planes, a joined batch resident in swapped order and one that is not),
apd_align_pair with explicit bands up to UINT64_MAX, the one-call apd_dtw_all_pairs, one pass through sharding.Multi([0]),
the warping paths, spotting, its paths, a streaming session with a kept history, the barycenters, the literal kernel's band limit and
the plan cache."""
import ctypes as C

import numpy as np
import pytest

import _config_cases as cc
import _dba_reference as dba
import _kernel_table as kt
import _path_reference as ref
import _spot_path_reference as spref
import _spot_reference as sref

pytestmark = pytest.mark.gpu
F32P, U64P = C.POINTER(C.c_float), C.POINTER(C.c_uint64)
ALL = cc.ENTRIES + [cc.ROUNDING_ENTRY]
IDS = [e.name for e in ALL]
PEN_IDS = [e.name for e in cc.PENALTY_ENTRIES]
MODES = ("hybrid", "exact", "strict")
# the first listed geometry of each family (csrc/apd_internal.h, read by tests/_kernel_table.py)
FORCED = [kt.encode(fam, *geoms[0]) for fam, geoms in kt.parse_table()[0].items()]


@pytest.fixture(scope="module")
def ctx(apd):
    c = apd.Context(0)
    yield c
    c.set_variant(0)
    c.set_distance_mode("hybrid")
    c.close()


def discovery(entry):
    from audio_pattern_discovery_amd.discovery import Discovery
    return Discovery(warping_band_percentage=entry.pct, insertion_penalty=entry.pens[0], deletion_penalty=entry.pens[1],
                     match_penalty=entry.pens[2])


def workers_of(ctx, seqs):
    from audio_pattern_discovery_amd.alignments import AlignmentWorkers, NDSequence
    return AlignmentWorkers.new([NDSequence(s) for s in seqs], ctx)


def batches_of(entry):
    return ("R",) if entry is cc.ROUNDING_ENTRY else ("A", "B")


def n_tiles(n_seq):
    side = (n_seq + 15) // 16
    return side * (side + 1) // 2


def align(ctx, capfd, key, entry, mode, variant, device=False):
    """(matrix, {geometry code: tiles}) of one apd_align_all (or apd_align_all_device_async) of a fresh resident batch."""
    from audio_pattern_discovery_amd import _lib
    b = cc.batch(key)
    n = len(b.seqs)
    ctx.set_distance_mode(mode)
    ctx.set_variant(variant)
    w = workers_of(ctx, b.seqs)
    try:
        with kt.debug_plan(capfd) as captured:
            if device:
                cfg = discovery(entry).align_config()
                d_out = ctx.alloc(4 * n * n)
                d_out.fill(0x55)
                _lib.check(_lib.lib().apd_align_all_device_async(ctx.handle, w._batch.handle, C.byref(cfg), d_out.at()), ctx.handle)
                ctx.synchronize()
                got = d_out.to_numpy(np.float32).reshape(n, n).copy()
                d_out.free()
            else:
                got = w.align_all(discovery(entry)).reshape(n, n).copy()
    finally:
        w.close()
        ctx.set_variant(0)
        ctx.set_distance_mode("hybrid")
    return got, kt.read_plan(captured[0])


# ---- apd_align_all, apd_align_all_device_async

@pytest.mark.parametrize("entry", ALL, ids=IDS)
def test_align_all_in_every_mode_and_under_forced_geometries(ctx, oracle, capfd, entry):
    """Hybrid, exact and strict mode, the device form, and the first geometry of every family forced.  A bitwise entry gives the
    oracle's bits every time (hence the same bits in all modes and under every forced code); strict mode is bitwise for every entry.
    A penalty that is <= 0, infinite or NaN runs geometry 0 alone: a forced geometry does not override the literal routing."""
    for key in batches_of(entry):
        want = cc.want_matrix(oracle, key, entry)
        tiles = n_tiles(len(cc.batch(key).seqs))
        runs = [(mode, 0, False) for mode in MODES] + [("hybrid", 0, True), ("strict", 0, True)] + [("hybrid", code, False) for code in FORCED]
        if cc.literal(entry.pens):
            runs += [("strict", FORCED[0], False), ("exact", FORCED[-1], True)]
        for mode, variant, device in runs:
            got, plan = align(ctx, capfd, key, entry, mode, variant, device)
            what = "%s batch %s %s variant %d%s" % (entry.name, key, mode, variant, " device" if device else "")
            cc.check(got, want, cc.BITWISE if mode == "strict" else entry.bound, what)
            assert sum(plan.values()) == tiles, (what, plan)
            if cc.literal(entry.pens):
                assert plan == {0: tiles}, "%s: the plan is %r, not the literal kernel alone" % (what, plan)


def test_positive_finite_penalties_do_take_the_fast_kernels(ctx, oracle, capfd):
    """The other side of the routing assertion: the plan lines of a positive finite entry name fast geometries, so `plan == {0: ..}`
    above is not what every plan says."""
    for name in ("unit/pct0.0625", "extremes/pct0.0625", "subnormal/pct0.0625", "p2^60/pct0.0625"):
        _, plan = align(ctx, capfd, "A", cc.BY_NAME[name], "hybrid", 0)
        assert plan and 0 not in plan, (name, plan)


def test_a_nan_score_is_a_result_and_a_dropped_tile_is_still_reported(apd, ctx, oracle):
    """A NaN penalty whose payload is the very pattern of the poison (0xFFFFFFFF): the matrix is the canonical NaN entry's, not
    APD_ERR_INCOMPLETE.  And the poison still works under the same configuration: with a tile dropped (apd_set_fault_injection)
    the call reports APD_ERR_INCOMPLETE."""
    b = cc.batch("A")
    n = len(b.seqs)
    entry = cc.BY_NAME["mat-nan/pct0.0625"]
    cfg = discovery(entry).align_config()
    C.memmove(C.addressof(cfg) + 12, (C.c_uint32 * 1)(0xFFFFFFFF), 4)               # match_penalty: a NaN of all ones
    assert cfg.match_penalty != cfg.match_penalty
    w = workers_of(ctx, b.seqs)
    try:
        out = np.zeros((n, n), dtype=np.float32)
        apd.check(apd.lib().apd_align_all(ctx.handle, w._batch.handle, C.byref(cfg), out.ctypes.data_as(F32P)), ctx.handle)
        cc.check(out, cc.want_matrix(oracle, "A", entry), cc.BITWISE, "NaN penalty with the poison's payload")
        assert np.isnan(out).sum() > 300
        ctx.set_fault_injection(1)
        try:
            rc = apd.lib().apd_align_all(ctx.handle, w._batch.handle, C.byref(cfg), out.ctypes.data_as(F32P))
        finally:
            ctx.set_fault_injection(0)
        assert rc == apd.APD_ERR_INCOMPLETE
    finally:
        w.close()


# ---- apd_align_cross

@pytest.mark.parametrize("entry", cc.ENTRIES, ids=[e.name for e in cc.ENTRIES])
def test_cross_both_planes_in_both_resident_orders(ctx, oracle, capfd, entry):
    """Batch A split 8 / 12: the second set is the longer one on average, so the joined batch is resident in swapped order; joined
    the other way round it is not.  fs[q][c] = score(x = first q, y = second c), sf[c][q] = score(x = second c, y = first q): the
    entries of the all-pairs matrix."""
    b = cc.batch("A")
    want = cc.want_matrix(oracle, "A", entry)
    cut = 8
    la, lb = b.lens[:cut], b.lens[cut:]
    assert sum(la) * len(lb) < sum(lb) * len(la)                     # apd_batch_join: swapped resident order for (first, second)
    first, second = workers_of(ctx, b.seqs[:cut]), workers_of(ctx, b.seqs[cut:])
    try:
        for mode in ("hybrid", "strict"):
            ctx.set_distance_mode(mode)
            bound = cc.BITWISE if mode == "strict" else entry.bound
            with kt.debug_plan(capfd) as captured:
                fs, sf = first.cross(second, discovery(entry))
                fs2, sf2 = second.cross(first, discovery(entry))
            plan = kt.read_plan(captured[0])
            cc.check(fs, want[:cut, cut:], bound, entry.name + " fs " + mode)
            cc.check(sf, want[cut:, :cut], bound, entry.name + " sf " + mode)
            cc.check(fs2, want[cut:, :cut], bound, entry.name + " fs, joined the other way " + mode)
            cc.check(sf2, want[:cut, cut:], bound, entry.name + " sf, joined the other way " + mode)
            if cc.literal(entry.pens):
                assert set(plan) == {0}, (entry.name, plan)
    finally:
        ctx.set_distance_mode("hybrid")
        first.close()
        second.close()


# ---- apd_align_pair with explicit bands

PAIR_PENS = ("unit", "ins0", "extremes", "all-inf", "mat-nan", "all-1")
PAIRS_OF_A = [(13, 14), (3, 5), (0, 1), (2, 4), (18, 15), (15, 18), cc.DUP_A, cc.INTEGER_A, (1, 0)]


@pytest.mark.parametrize("pname", PAIR_PENS)
def test_align_pair_with_explicit_bands(apd, ctx, oracle, pname):
    """warping_band 0, max(n, m), 2^32 - 1, 2^32, 0xFFFFFFF0 and UINT64_MAX.  band_from_params clamps to 0xFFFFFFF0 instead of
    truncating to 32 bits: 2^32 must be the full matrix, not band 0 -- and the two differ for these pairs."""
    from audio_pattern_discovery_amd.alignments import Alignment, AlignmentParams
    b = cc.batch("A")
    pens = cc.PENS[pname]
    bound = cc.bound_of(pens)
    told_apart = 0
    for x, y in PAIRS_OF_A:
        n, m = b.lens[x], b.lens[y]
        got, want = [], []
        for band in cc.EXPLICIT_BANDS:
            band = max(n, m) if band is None else band
            a = Alignment(ctx)
            a.construct_alignment(b.seqs[x], b.seqs[y], AlignmentParams(band, *pens))
            got.append(a.score())
            want.append(oracle.dtw_pair(b.seqs[x], b.seqs[y], band, *pens))
        cc.check(np.array(got, np.float32), np.array(want, np.float32), bound, "%s pair (%d, %d)" % (pname, x, y))
        assert cc.same_bits(want[1:], [want[1]] * 5)                 # every band from max(n, m) up is the full matrix
        told_apart += int(not cc.same_bits([want[0]], [want[3]]))
    assert told_apart >= 1 or pname in ("all-inf", "mat-nan")


# ---- the one-call form and the multi-device handle

@pytest.mark.parametrize("entry", ALL, ids=IDS)
def test_dtw_all_pairs_in_one_call(apd, oracle, entry):
    key = batches_of(entry)[0]
    b = cc.batch(key)
    n = len(b.seqs)
    out = np.full((n, n), -1.0, dtype=np.float32)
    apd.check(apd.lib().apd_dtw_all_pairs(b.frames.ctypes.data_as(F32P), b.offsets.ctypes.data_as(U64P), n, b.dim, entry.pct, entry.pens[0],
                                          entry.pens[1], entry.pens[2], 1, out.ctypes.data_as(F32P)))
    cc.check(out, cc.want_matrix(oracle, key, entry), entry.bound, entry.name)


def test_one_pass_through_the_multi_device_handle(apd, oracle):
    from audio_pattern_discovery_amd import sharding
    multi = sharding.Multi([0])
    try:
        for key in ("A", "B", "R"):
            b = cc.batch(key)
            mb = multi.batch(b.offsets, b.dim, frames=b.frames)
            try:
                for entry in ([cc.ROUNDING_ENTRY] if key == "R" else cc.ENTRIES):
                    got = multi.align_all(mb, discovery(entry).align_config())
                    cc.check(got, cc.want_matrix(oracle, key, entry), entry.bound, "%s batch %s" % (entry.name, key))
            finally:
                mb.close()
    finally:
        multi.close()


# ---- warping paths

_PATHS = {}


def want_path(key, x, y, band, pens):
    k = (key, x, y, min(int(band), 2 ** 64), pens if not any(p != p for p in pens) else repr(pens))
    if k not in _PATHS:
        b = cc.batch(key)
        _PATHS[k] = ref.path(b.seqs[x], b.seqs[y], band, *pens)
    return _PATHS[k]


def assert_same_path(got_steps, got_score, want, x, y, pens, what):
    want_steps, want_score = want
    assert spref.same_steps(got_steps, want_steps), what
    assert cc.same_bits([got_score], [want_score]), what
    # the costs replayed forward from the steps the GPU returned
    if len(got_steps) and got_steps[0]["op"] == ref.START:
        assert cc.same_bits(ref.replay(x, y, got_steps, *pens), got_steps["cost"]), what + ": replayed costs"


@pytest.mark.parametrize("entry", ALL, ids=IDS)
def test_align_paths(ctx, oracle, entry):
    """apd_align_paths over the pairs the per-cell checker walks: steps, lengths, costs and scores, NaN tables included (a score
    cell that was never visited gives no steps; a walk that leaves the table ends without a START)."""
    key = batches_of(entry)[0]
    b = cc.batch(key)
    pairs = cc.SLOW_PAIRS if key == "A" else [(0, 1), (1, 0), (0, 3), (3, 0), (2, 4), (4, 5), (5, 1)]
    w = workers_of(ctx, b.seqs)
    try:
        got, scores = w.paths(pairs, discovery(entry))
    finally:
        w.close()
    empty = partial = 0
    for p, (x, y) in enumerate(pairs):
        band = ref.band_from_pct(entry.pct, max(b.lens[x], b.lens[y]))
        want = want_path(key, x, y, band, entry.pens)
        assert_same_path(got[p], scores[p], want, b.seqs[x], b.seqs[y], entry.pens, "%s pair (%d, %d)" % (entry.name, x, y))
        assert cc.same_bits([scores[p]], [cc.want_matrix(oracle, key, entry)[x, y]])
        empty += int(len(want[0]) == 0)
        partial += int(len(want[0]) > 0 and want[0][0]["op"] != ref.START)
    if key == "A":
        assert empty >= 4                                            # the one-frame sequence against longer ones: no score cell


@pytest.mark.parametrize("entry", cc.PENALTY_ENTRIES, ids=PEN_IDS)
def test_align_pair_path_with_explicit_bands(apd, ctx, entry):
    from test_gpu_paths import pair_path
    b = cc.batch("A")
    for x, y in [(3, 5), (2, 4), (0, 1), cc.DUP_A, (19, 3)]:
        for band in (0, None, 2 ** 32, 2 ** 64 - 1):
            band = max(b.lens[x], b.lens[y]) if band is None else band
            steps, score = pair_path(apd, ctx, b.seqs[x], b.seqs[y], band, entry.pens)
            assert_same_path(steps, score, want_path("A", x, y, band, entry.pens), b.seqs[x], b.seqs[y], entry.pens,
                             "%s pair (%d, %d) band %d" % (entry.name, x, y, band))


# ---- spotting: apd_spot, apd_spot_paths, the streaming session

# (query, stream) of batch A: the 130-frame query (three rows per lane), the three-, two- and one-frame ones, the duplicate and the
# integer pair (zero distances, exact ties); the percentage is not read: NaN is passed
SPOT_PAIRS = [(cc.LONG_A, 15), (2, 15), (1, 3), (0, 3), cc.DUP_A, cc.INTEGER_A, (5, 15)]
_SPOTS, _SPOT_TABLES = {}, {}


def spot_entry(entry):
    return cc.Entry(entry.name, entry.pens, float("nan"), cc.BITWISE)


def want_spot(x, y, pens):
    k = (x, y, repr(pens))
    if k not in _SPOTS:
        b = cc.batch("A")
        _SPOTS[k] = sref.spot(b.seqs[x], b.seqs[y], *pens)
    return _SPOTS[k]


def want_spot_table(x, y, pens):
    k = (x, y, repr(pens))
    if k not in _SPOT_TABLES:
        b = cc.batch("A")
        _SPOT_TABLES[k] = spref.table(b.seqs[x], b.seqs[y], *pens)
    return _SPOT_TABLES[k]


def windows_of(x, y, pens):
    """The windows asked of one pair: the best one, the last column's, one in the middle, one with a wrong start, no window."""
    b = cc.batch("A")
    cost, start, best = want_spot(x, y, pens)
    m = b.lens[y]
    mid = max(m // 2, 1)
    out = [(int(best["end"]), int(best["start"])), (m, int(start[m - 1])), (mid, int(start[mid - 1])), (0, 0)]
    if int(start[m - 1]) > 1:
        out.append((m, int(start[m - 1]) - 1))
    return [(e, s) for e, s in out if (e == 0 and s == 0) or 1 <= s <= e]


@pytest.mark.parametrize("entry", cc.PENALTY_ENTRIES, ids=PEN_IDS)
def test_spot_and_spot_paths(ctx, entry):
    from audio_pattern_discovery_amd.alignments import SPOT_BEST
    b = cc.batch("A")
    e = spot_entry(entry)
    w = workers_of(ctx, b.seqs)
    try:
        curves, best = w.spot(SPOT_PAIRS, discovery(e))
        _, best_only = w.spot(SPOT_PAIRS, discovery(e), curves=False)
        records, asked = [], []
        for x, y in SPOT_PAIRS:
            for end, start in windows_of(x, y, entry.pens):
                records.append((x, y))
                asked.append((end, start))
        win = np.zeros(len(asked), dtype=SPOT_BEST)
        win["end"], win["start"] = [a[0] for a in asked], [a[1] for a in asked]
        paths, found, scores = w.spot_paths(records, win, discovery(e))
    finally:
        w.close()
    for p, (x, y) in enumerate(SPOT_PAIRS):
        cost, start, want_best = want_spot(x, y, entry.pens)
        what = "%s pair (%d, %d)" % (entry.name, x, y)
        assert cc.same_bits(curves[p][0], cost), what + " cost"
        assert np.array_equal(curves[p][1], start), what + " start"
        assert sref.same_best(best[p], want_best) and sref.same_best(best_only[p], want_best), what + " best"
    for k, ((x, y), (end, start)) in enumerate(zip(records, asked)):
        what = "%s pair (%d, %d) window (%d, %d)" % (entry.name, x, y, end, start)
        steps, want_found, want_score = spref.answer(want_spot_table(x, y, entry.pens), b.lens[x], end, start)
        assert spref.same_steps(paths[k], steps), what
        assert int(found[k]) == want_found and cc.same_bits([scores[k]], [want_score]), what


STREAM_QUERIES = [cc.LONG_A, 2, 5, 0]
STREAM_OF = 15
CHUNKINGS = ((70,), (1, 30, 0, 39), (33, 37))


@pytest.mark.parametrize("entry", cc.PENALTY_ENTRIES, ids=PEN_IDS)
def test_streaming_session_equals_spot_on_the_whole_stream(ctx, entry):
    """Three chunkings of the 70-frame stream: the curves of the pushes, one after the other, and the last best are apd_spot's bits on
    the whole stream (and the checker's); with the whole stream kept, apd_spot_stream_paths gives apd_spot_paths' answers."""
    from audio_pattern_discovery_amd.alignments import SPOT_BEST, SPOT_WINDOW
    b = cc.batch("A")
    e = spot_entry(entry)
    stream = b.seqs[STREAM_OF]
    pairs = [(q, STREAM_OF) for q in STREAM_QUERIES]
    w = workers_of(ctx, b.seqs)
    try:
        curves, best = w.spot(pairs, discovery(e))
        for p, (x, y) in enumerate(pairs):
            cost, start, want_best = want_spot(x, y, entry.pens)
            assert cc.same_bits(curves[p][0], cost) and np.array_equal(curves[p][1], start) and sref.same_best(best[p], want_best)
        asked = [(q, 0) + win for q, (x, y) in enumerate(pairs) for win in windows_of(x, y, entry.pens)]
        win = np.zeros(len(asked), dtype=SPOT_BEST)
        win["end"], win["start"] = [a[2] for a in asked], [a[3] for a in asked]
        whole_paths, whole_found, whole_scores = w.spot_paths([pairs[a[0]] for a in asked], win, discovery(e))
        for chunking in CHUNKINGS:
            assert sum(chunking) == len(stream)
            session = w.spot_stream(STREAM_QUERIES, discovery(e), channels=1, history=len(stream))
            try:
                cost = [[] for _ in pairs]
                start = [[] for _ in pairs]
                at = 0
                for size in chunking:
                    pushed, running = session.push([stream[at:at + size]])
                    at += size
                    for p in range(len(pairs)):
                        cost[p].append(pushed[p][0])
                        start[p].append(pushed[p][1])
                for p in range(len(pairs)):
                    what = "%s query %d chunking %r" % (entry.name, STREAM_QUERIES[p], chunking)
                    assert cc.same_bits(np.concatenate(cost[p]), curves[p][0]), what
                    assert np.array_equal(np.concatenate(start[p]), curves[p][1]), what
                    assert sref.same_best(running[p], best[p]), what
                records = np.array(asked, dtype=SPOT_WINDOW)
                paths, found, scores = session.paths(records)
                for k in range(len(asked)):
                    what = "%s window %r chunking %r" % (entry.name, asked[k], chunking)
                    assert spref.same_steps(paths[k], whole_paths[k]), what
                    assert found[k] == whole_found[k] and cc.same_bits([scores[k]], [whole_scores[k]]), what
            finally:
                session.close()
    finally:
        w.close()


# ---- apd_barycenters

DBA_ENTRIES = cc.PENALTY_ENTRIES + [cc.BY_NAME["unit/" + n] for n, _ in cc.PCT_SATURATED] + \
    [cc.BY_NAME["unit/" + n] for n in ("pct-nan", "pct-0.5", "pct-inf")] + [cc.BY_NAME["ins0/pct+inf"], cc.BY_NAME["ins0/pct-nan"]]
# a barycenter of 130 frames (longer than a wavefront) over members of 30, 37, 35 and 1 frames; the duplicates and an integer
# sequence from one of the duplicates; a singleton
DBA_SETS = [[3, 5, 19, 0], [9, 10, 16], [2]]
DBA_INIT = [cc.LONG_A, 9, 2]


@pytest.mark.parametrize("entry", DBA_ENTRIES, ids=[e.name for e in DBA_ENTRIES])
def test_barycenters_two_iterations(apd, ctx, entry):
    from test_gpu_prototypes import assert_same, make_batch, raw_barycenters
    b = cc.batch("A")
    batch = make_batch(ctx, b.seqs)
    try:
        frames, inertia, used, off = raw_barycenters(apd, ctx, batch, b.dim, entry.pct, entry.pens, DBA_SETS, DBA_INIT, 2)
    finally:
        batch.close()
    want = dba.barycenters(b.seqs, DBA_SETS, DBA_INIT, entry.pct, entry.pens, 2)
    assert np.diff(off).tolist() == [len(f) for f in want[0]]
    assert_same((frames, inertia, used), want, entry.name)


# ---- the literal kernel's band limit, from apd_align_all

def literal_band_limit():
    """The largest 2w + 1 the literal kernel holds, from generic_lds_bytes and the 160 KiB test of launch_align (csrc/dtw_generic.hip):
    c_max = ceil((2w + 1) / 64) cells per lane, two DP rows of 64 * c_max floats, c_max * 64 * 2 * 4 <= 160 * 1024."""
    c_max = (160 * 1024) // (64 * 2 * 4)
    return 64 * c_max


def test_literal_band_limit_is_refused_before_anything_is_enqueued(apd, ctx, oracle, capfd):
    """2w + 1 <= 20480 = 64 * floor(160 KiB / (64 lanes * 2 rows * 4 bytes)).  Two dim-1 sequences of 10238 frames under a zero
    penalty (the literal kernel) and a full band have w = 10240, 2w + 1 = 20481: APD_ERR_BAND_TOO_WIDE, nothing enqueued, the output
    untouched, the context usable.  With 10237 frames 2w + 1 = 20479: the literal kernel at its largest LDS row, bit for bit the
    oracle's."""
    from audio_pattern_discovery_amd.alignments import Batch
    assert literal_band_limit() == 20480
    over, under = (literal_band_limit() - 5) // 2 + 1, (literal_band_limit() - 5) // 2      # 2 (n + 2) + 1 <= limit
    assert (over, under) == (10238, 10237) and 2 * (over + 2) + 1 > literal_band_limit() >= 2 * (under + 2) + 1
    entry = cc.Entry("ins0/pct1", cc.PENS["ins0"], 1.0, cc.BITWISE)
    rng = np.random.default_rng(10237)
    walk = np.cumsum(rng.standard_normal((2, over, 1)), axis=1).astype(np.float32)
    L = apd.lib()
    for n, fits in ((over, False), (under, True)):
        frames = np.concatenate([walk[0, :n], walk[1, :n]], axis=0)
        offsets = np.array([0, n, 2 * n], dtype=np.uint64)
        batch = Batch(ctx, frames, offsets, 1)
        try:
            ctx.synchronize()
            out = np.full((2, 2), -7.0, dtype=np.float32)
            cfg = discovery(entry).align_config()
            with kt.debug_plan(capfd) as captured:
                rc = L.apd_align_all(ctx.handle, batch.handle, C.byref(cfg), out.ctypes.data_as(F32P))
                busy = ctx.stream_busy()
            assert kt.read_plan(captured[0]) == {0: 1}
            if not fits:
                assert rc == apd.APD_ERR_BAND_TOO_WIDE and not busy
                assert np.all(out == -7.0)
                d_out = ctx.alloc(16)
                d_out.fill(0x55)
                ctx.synchronize()
                assert L.apd_align_all_device_async(ctx.handle, batch.handle, C.byref(cfg), d_out.at()) == apd.APD_ERR_BAND_TOO_WIDE
                assert not ctx.stream_busy()
                assert np.all(d_out.to_numpy(np.uint32) == 0x55555555)
                d_out.free()
            else:
                apd.check(rc, ctx.handle)
                cc.check(out, oracle.align_all(frames, offsets, 1.0, *entry.pens, workers=2), cc.BITWISE, "literal kernel at its widest band")
        finally:
            batch.close()
    # the context is usable after the refusal
    got, _ = align(ctx, capfd, "A", cc.BY_NAME["ins0/pct0.0625"], "hybrid", 0)
    cc.check(got, cc.want_matrix(oracle, "A", cc.BY_NAME["ins0/pct0.0625"]), cc.BITWISE, "after the refusal")


# ---- the plan cache

def test_plan_cache_keeps_fast_and_literal_plans_apart(ctx, oracle):
    """One resident batch under a positive config, a zero-penalty config of the same band, and the positive one again: the cached
    plans are keyed by what chose the kernels, so the first and third matrices are bit-identical and the second is the oracle's."""
    b = cc.batch("A")
    n = len(b.seqs)
    w = workers_of(ctx, b.seqs)
    try:
        unit, zero = cc.BY_NAME["unit/pct0.0625"], cc.BY_NAME["ins0/pct0.0625"]
        first = w.align_all(discovery(unit)).reshape(n, n).copy()
        second = w.align_all(discovery(zero)).reshape(n, n).copy()
        third = w.align_all(discovery(unit)).reshape(n, n).copy()
        fourth = w.align_all(discovery(cc.BY_NAME["all-inf/pct0.0625"])).reshape(n, n).copy()
        fifth = w.align_all(discovery(zero)).reshape(n, n).copy()
    finally:
        w.close()
    assert cc.same_bits(first, third)
    cc.check(first, cc.want_matrix(oracle, "A", unit), unit.bound, "positive config")
    cc.check(second, cc.want_matrix(oracle, "A", zero), cc.BITWISE, "zero-penalty config between two positive ones")
    cc.check(fourth, cc.want_matrix(oracle, "A", cc.BY_NAME["all-inf/pct0.0625"]), cc.BITWISE, "infinite penalties on the cached literal plan")
    assert cc.same_bits(second, fifth)
