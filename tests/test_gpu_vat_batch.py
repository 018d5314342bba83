"""Stage 1 for a whole corpus (csrc/vat.hip): apd_interesting_ranges_batch against the C oracle, its numpy twin and -- where the
arithmetic is exact -- plain integers (_companion_cases.py); apd_slice_samples against numpy slicing; `segment` against the
reference's order of operations done with the single-recording calls and the oracle.

A recording's answer must not depend on the batch around it: every comparison below is per recording, and the same recordings are
run in several batches (in order, reversed, alone, and alone through apd_interesting_ranges, which is a batch of one: the same
kernels, so no witness of its own -- every such comparison stands beside one with the oracle or the integers)."""
import ctypes as C

import numpy as np
import pytest

import _companion_cases as cc
from _vat_batch_calls import SENTINEL, U64P, batch_call, batch_result, gather, ramps, single_result
from audio_pattern_discovery_amd import synth
from oracle import np_reference as npr

pytestmark = pytest.mark.gpu
TILE = 256            # kVatTile (csrc/vat.hip): frames per workgroup of the variance kernel; windows up to it keep their halo in LDS
FORMS = ["host", "device", "device+4"]


@pytest.fixture(scope="module")
def ctx(apd):
    c = apd.Context(0)
    yield c
    c.close()


def reference_result(fn, *args):
    try:
        return fn(*args)
    except IndexError:
        return "panic"


def index_of(t, perc):
    return int(np.float32(t) * np.float32(perc))


# ------------------------------------------------------------------------------------------------ known answers

def kat_batch(n_bins=4):
    moved = list(cc.KAT_A)
    moved[30], moved[44] = 1, 7                                     # the lone burst of frame 30 now sits at frame 44
    return [list(cc.KAT_A), list(cc.random_integer_a()), moved], n_bins


@pytest.mark.parametrize("form", FORMS)
def test_known_answers_in_a_batch(ctx, apd, form):
    """Ties with the threshold and runs of min_len and min_len + 1, decided by integer arithmetic, for three recordings at once."""
    a_list, n_bins = kat_batch()
    recs = [cc.alternating(a, n_bins) for a in a_list]
    k, perc = cc.KAT_K, cc.KAT_PERC
    for min_len in (cc.KAT_MIN_LEN - 1, cc.KAT_MIN_LEN, cc.KAT_MIN_LEN + 1):
        want = [cc.integer_ranges(a, k, index_of(len(a), perc), min_len)[0] for a in a_list]
        if min_len == cc.KAT_MIN_LEN:
            assert want[0] == cc.KAT_RANGES and want[2] != want[0] and all(want)
        assert batch_result(apd, ctx, recs, k, perc, min_len, form) == want
        assert batch_result(apd, ctx, recs[::-1], k, perc, min_len, form) == want[::-1]


# -------------------------------------------------------------- among neighbours == alone (a batch of one) == oracle

def planted(rng, t, n_bins):
    """Random f32 frames with louder stretches, so that runs open and close at every length."""
    f = rng.standard_normal((t, n_bins)).astype(np.float32)
    for lo, hi, g in ((t // 10, t // 4, 5.0), (t // 3, t // 3 + max(t // 40, 1), 9.0), (t // 2, (9 * t) // 10, 3.0)):
        f[lo:hi] *= np.float32(g)
    return f


# 64 bins: wider than the variance kernel stages through LDS (48), its rows are read from global memory directly
@pytest.mark.parametrize("n_bins", [1, 2, 13, 26, 40, 64])
def test_batch_equals_the_single_call_and_the_oracle(ctx, apd, oracle, n_bins):
    rng = np.random.default_rng(900 + n_bins)
    nonempty = compared = 0
    for k in (1, 3, 15, 64, TILE, TILE + 1, 5000):
        lengths = [1, k, k + 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 2500]
        recs = [planted(rng, t, n_bins) for t in lengths]
        for perc in (0.0, 0.05, 0.5, 0.95):
            for min_len in (0, 5, 30):
                want = [reference_result(oracle.interesting_ranges, f, k, perc, min_len) for f in recs]
                got = batch_result(apd, ctx, recs, k, perc, min_len, "device" if min_len == 5 else "host")
                assert got == want, (k, perc, min_len)
                assert batch_result(apd, ctx, recs[::-1], k, perc, min_len) == want[::-1], (k, perc, min_len)   # other neighbours, first <-> last
                if min_len == 5:
                    assert [single_result(apd, ctx, f, k, perc, min_len) for f in recs] == want
                if min_len == 30 and perc == 0.5:
                    for s in (0, 2, 7, 10):
                        assert batch_result(apd, ctx, [recs[s]], k, perc, min_len) == [want[s]]                  # alone
                compared += len(recs)
                nonempty += sum(1 for w in want if w and w != "panic")
    if n_bins == 1:
        assert nonempty == 0                                        # every std is 0, the threshold is 0 and nothing is below it
    else:
        assert nonempty >= 40, (nonempty, compared)


# ------------------------------------------------------------------------------------------------ panics

def test_panics_per_recording(ctx, apd, oracle):
    rng = np.random.default_rng(31)
    a, b = planted(rng, 300, 7), planted(rng, 700, 7)
    recs = [a, np.zeros((0, 7), np.float32), np.full((90, 7), np.nan, np.float32), b]
    want = [reference_result(oracle.interesting_ranges, f, 4, 0.5, 3) for f in recs]
    assert want[1] == "panic" and want[2] == "panic" and len(want[0]) > 1 and len(want[3]) > 1
    assert [reference_result(npr.interesting_ranges, f, 4, 0.5, 3) for f in recs] == want
    for form in ("host", "device"):
        assert batch_result(apd, ctx, recs, 4, 0.5, 3, form) == want
    # without a status array: APD_ERR_INDEX, the first such recording named, nothing reported
    rc, range_off, ranges, _ = batch_call(apd, ctx, recs, 4, 0.5, 3, with_status=False)
    assert rc == apd.APD_ERR_INDEX and np.all(range_off == 0) and np.all(ranges == SENTINEL)
    assert b"recording 1" in apd.lib().apd_last_error(ctx.handle)
    rc, range_off, _, _ = batch_call(apd, ctx, [a, b], 4, 0.5, 3, with_status=False)
    assert rc == apd.APD_OK and int(range_off[-1]) == len(want[0]) + len(want[3])
    # perc = 1: index == length; moving_average = 0: every variance is 0 / 0
    for k, perc in ((4, 1.0), (0, 0.5), (0, 0.0)):
        assert reference_result(oracle.interesting_ranges, a, k, perc, 3) == "panic"
        assert batch_result(apd, ctx, recs, k, perc, 3) == ["panic"] * 4
        rc, range_off, _, _ = batch_call(apd, ctx, recs, k, perc, 3, with_status=False)
        assert rc == apd.APD_ERR_INDEX and np.all(range_off == 0)
        assert b"recording 0" in apd.lib().apd_last_error(ctx.handle)


def test_argument_errors_and_empty_batches(ctx, apd):
    L = apd.lib()
    f = cc.kat_frames()
    range_off = np.full(3, SENTINEL, np.uint64)
    one = np.zeros(1, np.uint64)
    # n_seq == 0
    assert L.apd_interesting_ranges_batch(ctx.handle, None, one.ctypes.data_as(U64P), 0, 4, 4, 0.5, 3, 0, range_off.ctypes.data_as(U64P), None, 0, None) == apd.APD_OK
    assert range_off[0] == 0 and range_off[1] == SENTINEL
    # descending offsets
    bad = np.array([0, 64, 10], np.uint64)
    ranges = np.zeros(64, np.uint64)
    assert L.apd_interesting_ranges_batch(ctx.handle, C.c_void_p(f.ctypes.data), bad.ctypes.data_as(U64P), 2, 4, 4, 0.5, 3, 0, range_off.ctypes.data_as(U64P),
                                          ranges.ctypes.data_as(U64P), 32, None) == apd.APD_ERR_INVALID_ARG
    # a recording of 2^32 frames: refused before anything is read
    huge = np.array([0, 2 ** 32], np.uint64)
    assert L.apd_interesting_ranges_batch(ctx.handle, C.c_void_p(f.ctypes.data), huge.ctypes.data_as(U64P), 1, 4, 4, 0.5, 3, 0, range_off.ctypes.data_as(U64P),
                                          ranges.ctypes.data_as(U64P), 32, None) == apd.APD_ERR_UNSUPPORTED
    # the same through the single call, device form: the limit comes before any launch or allocation, so the pointer is never read
    # (it is no device address), *n_ranges is 0 and the caller's array is untouched
    ranges[:] = SENTINEL
    n = C.c_uint64(12345)
    assert L.apd_interesting_ranges(ctx.handle, C.c_void_p(f.ctypes.data), 2 ** 32, 4, 4, 0.5, 3, 1, ranges.ctypes.data_as(U64P), 32,
                                    C.byref(n)) == apd.APD_ERR_UNSUPPORTED
    assert n.value == 0 and np.all(ranges == SENTINEL)
    assert b"apd_interesting_ranges:" in L.apd_last_error(ctx.handle)
    ranges[:] = 0
    # n_bins == 0, no range_off
    ok = np.array([0, 64], np.uint64)
    assert L.apd_interesting_ranges_batch(ctx.handle, C.c_void_p(f.ctypes.data), ok.ctypes.data_as(U64P), 1, 0, 4, 0.5, 3, 0, range_off.ctypes.data_as(U64P),
                                          ranges.ctypes.data_as(U64P), 32, None) == apd.APD_ERR_INVALID_ARG
    assert L.apd_interesting_ranges_batch(ctx.handle, C.c_void_p(f.ctypes.data), ok.ctypes.data_as(U64P), 1, 4, 4, 0.5, 3, 0, None,
                                          ranges.ctypes.data_as(U64P), 32, None) == apd.APD_ERR_INVALID_ARG


# ------------------------------------------------------------------------------------------------ non-finite frames

@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_nonfinite_frames_stay_in_their_recording(ctx, apd, oracle, bad):
    rng = np.random.default_rng(78)
    k, perc, min_len = 4, 0.5, 2
    left, base, right = planted(rng, 333, 6), planted(rng, 400, 6), planted(rng, 129, 6)
    clean = batch_result(apd, ctx, [left, base, right], k, perc, min_len)
    want_clean = oracle.interesting_ranges(base, k, perc, min_len)
    assert clean[1] == want_clean and len(want_clean) > 2
    inside = (want_clean[1][0] + want_clean[1][1]) // 2
    edge = want_clean[1][1] - 1
    for where in (inside, edge, 1):                                # inside a run, the last frame of a run, among the first k frames
        f = base.copy()
        f[where, 2] = bad
        want = reference_result(oracle.interesting_ranges, f, k, perc, min_len)
        assert reference_result(npr.interesting_ranges, f, k, perc, min_len) == want and want != "panic"
        for form in ("host", "device"):
            got = batch_result(apd, ctx, [left, f, right], k, perc, min_len, form)
            assert got[1] == want, (where, form)
            assert got[0] == clean[0] and got[2] == clean[2]


# ------------------------------------------------------------------------------------------------ capacity

@pytest.mark.parametrize("form", ["host", "device+4"])
def test_capacity(ctx, apd, form):
    a_list, n_bins = kat_batch()
    recs = [cc.alternating(a, n_bins) for a in a_list]
    k, perc, min_len = cc.KAT_K, cc.KAT_PERC, cc.KAT_MIN_LEN
    want = [cc.integer_ranges(a, k, index_of(len(a), perc), min_len)[0] for a in a_list]
    flat = np.array([v for rec in want for pair in rec for v in pair], dtype=np.uint64)
    want_off = np.concatenate([[0], np.cumsum([len(w) for w in want])]).astype(np.uint64)
    total = int(want_off[-1])
    assert total > len(want[0]) + 1                                 # the cuts below fall inside the second recording
    for cap in (0, 1, len(want[0]) + 1, total - 1, total, total + 3):
        rc, range_off, ranges, status = batch_call(apd, ctx, recs, k, perc, min_len, form, capacity=cap)
        assert rc == apd.APD_OK and np.array_equal(range_off, want_off) and np.all(status == apd.APD_OK)
        w = 2 * min(cap, total)
        assert np.array_equal(ranges[:w], flat[:w]) and np.all(ranges[w:] == SENTINEL)
    rc, range_off, _, _ = batch_call(apd, ctx, recs, k, perc, min_len, form, capacity=0, null_ranges=True)
    assert rc == apd.APD_OK and np.array_equal(range_off, want_off)
    rc, _, _, _ = batch_call(apd, ctx, recs, k, perc, min_len, form, capacity=2, null_ranges=True)
    assert rc == apd.APD_ERR_INVALID_ARG


# ------------------------------------------------------------------------------------------------ one long recording

def test_one_long_recording_among_short_ones(ctx, apd, oracle):
    """300 000 frames [a, -a] with a constant over 256 frames, window 8: exact arithmetic, a few hundred runs, the scan's state carried
    over hundreds of steps; the short neighbours keep their answers."""
    a_long = cc.wrap_a(300000, seed=6)
    a_list = [list(cc.KAT_A), a_long, list(cc.random_integer_a())]
    recs = [cc.alternating(a, 2) for a in a_list]
    k, perc, min_len = 8, 0.5, 100
    want_long = oracle.interesting_ranges(recs[1], k, perc, min_len)
    assert 100 < len(want_long) < 2000 and want_long[-1][1] > 290000
    assert cc.integer_ranges(a_long, k, index_of(300000, perc), min_len)[0] == want_long
    for min_len_short, form in ((100, "device"), (3, "host")):
        want = [cc.integer_ranges(a, k, index_of(len(a), perc), min_len_short)[0] for a in a_list[::2]]
        got = batch_result(apd, ctx, recs, k, perc, min_len_short, form)
        assert [got[0], got[2]] == want
        if min_len_short == min_len:
            assert got[1] == want_long
        else:
            assert got[1] == oracle.interesting_ranges(recs[1], k, perc, min_len_short) and len(got[1]) >= len(want_long)
    assert any(want)


# ------------------------------------------------------------------------------------------------ slices

def random_ranges(rng, lengths, fft_step):
    out = []
    for n in lengths:
        frames = n // fft_step
        cuts = np.sort(rng.choice(frames + 1, size=2 * int(rng.integers(0, min(5, (frames + 1) // 2) + 1)), replace=False)) if frames else []
        out.append([(int(cuts[2 * i]), int(cuts[2 * i + 1])) for i in range(len(cuts) // 2)])
    return out


@pytest.mark.parametrize("fft_step", [127, 128])
@pytest.mark.parametrize("form", ["host", "device", "device+2"])
def test_slices_equal_numpy_slicing(ctx, apd, fft_step, form):
    rng = np.random.default_rng(5 + fft_step)
    lengths = [5003, 12345, 801, 0, 60, 40001, 1279]               # none a multiple of either step
    assert all(n % fft_step for n in lengths if n)
    recs = ramps(lengths)
    seen = 0
    for _ in range(4):
        ranges = random_ranges(rng, lengths, fft_step)
        ranges[1] = ranges[1] or [(3, 90)]
        want = np.concatenate([recs[s][a * fft_step:b * fft_step] for s in range(len(recs)) for a, b in ranges[s]] + [np.zeros(0, np.int16)])
        rc, out, total = gather(apd, ctx, recs, ranges, fft_step, form)
        assert rc == apd.APD_OK and total == len(want)
        assert np.array_equal(out[:total], want)
        assert np.all(out[total:] == 0x5A5A)                         # nothing written past the slices
        seen += sum(len(r) for r in ranges)
    assert seen > 10


def test_slices_edge_cases(ctx, apd):
    recs = ramps([1000, 700])
    # no ranges: nothing written, APD_OK
    for form in ("host", "device"):
        rc, out, total = gather(apd, ctx, recs, [[], []], 128, form)
        assert rc == apd.APD_OK and total == 0 and np.all(out == 0x5A5A)
    # slices shorter than a 16-byte group, touching, empty, and the very end of a recording
    ranges = [[(0, 1), (1, 1), (1, 3), (3, 7)], [(2, 2), (4, 5)]]
    for step in (1, 3, 100):
        want = np.concatenate([recs[s][a * step:b * step] for s in range(2) for a, b in ranges[s]])
        for form in ("host", "device+2"):
            rc, out, total = gather(apd, ctx, recs, ranges, step, form)
            assert rc == apd.APD_OK and np.array_equal(out[:total], want) and np.all(out[total:] == 0x5A5A)
    # a range past its recording, a capacity below the total
    L = apd.lib()
    sample_off, range_off = np.array([0, 1000, 1700], np.uint64), np.array([0, 1, 1], np.uint64)
    flat, out = np.array([2, 8], np.uint64), np.zeros(2000, np.int16)
    samples = np.concatenate(recs)
    call = lambda step, cap: L.apd_slice_samples(ctx.handle, C.c_void_p(samples.ctypes.data), sample_off.ctypes.data_as(U64P), 2, range_off.ctypes.data_as(U64P),
                                                 flat.ctypes.data_as(U64P), step, 0, C.c_void_p(out.ctypes.data), cap)
    assert call(125, 750) == apd.APD_OK and np.array_equal(out[:750], recs[0][250:1000])
    assert call(126, 2000) == apd.APD_ERR_INVALID_ARG and call(125, 749) == apd.APD_ERR_INVALID_ARG


def test_slices_refuse_bad_range_offsets_before_sizing_anything(ctx, apd):
    """range_off is checked as a whole before range_off[n_seq] sizes the call's own arrays: a descent behind a long recording, a
    first entry that is not 0 and an absurd last entry are APD_ERR_INVALID_ARG (the last one APD_ERR_OOM at worst), never a write."""
    L = apd.lib()
    recs = ramps([1000, 700])
    samples, out = np.concatenate(recs), np.full(2000, 0x5A5A, np.int16)
    sample_off = np.array([0, 1000, 1700], np.uint64)
    flat = np.array([(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)], np.uint64).ravel()
    call = lambda ro: L.apd_slice_samples(ctx.handle, C.c_void_p(samples.ctypes.data), sample_off.ctypes.data_as(U64P), 2,
                                          np.array(ro, np.uint64).ctypes.data_as(U64P), flat.ctypes.data_as(U64P), 100, 0, C.c_void_p(out.ctypes.data), 2000)
    assert call([0, 5, 5]) == apd.APD_OK and np.array_equal(out[:500], recs[0][:500])
    out[:] = 0x5A5A
    assert call([0, 5, 2]) == apd.APD_ERR_INVALID_ARG
    assert call([1, 3, 5]) == apd.APD_ERR_INVALID_ARG
    assert call([0, 2 ** 62, 2 ** 62 - 1]) == apd.APD_ERR_INVALID_ARG
    assert np.all(out == 0x5A5A)


def test_offsets_that_do_not_start_at_zero(ctx, apd, oracle):
    """frame_offsets[0] != 0 and sample_offsets[0] != 0: the batch is a part of a larger packed array, addressed from its start."""
    L = apd.lib()
    rng = np.random.default_rng(12)
    lead, recs = planted(rng, 77, 13), [planted(rng, t, 13) for t in (300, 513, 90)]
    k, perc, min_len = 15, 0.5, 5
    want = [oracle.interesting_ranges(f, k, perc, min_len) for f in recs]
    assert all(want[:2])
    flat = np.ascontiguousarray(np.concatenate([lead] + recs), dtype=np.float32)
    offsets = (77 + np.concatenate([[0], np.cumsum([len(r) for r in recs])])).astype(np.uint64)
    d_flat = ctx.upload(flat)
    for ptr, on_device in ((C.c_void_p(flat.ctypes.data), 0), (d_flat.at(), 1)):
        range_off, ranges, status = np.zeros(4, np.uint64), np.zeros(2 * 500, np.uint64), np.zeros(3, np.int32)
        apd.check(L.apd_interesting_ranges_batch(ctx.handle, ptr, offsets.ctypes.data_as(U64P), 3, 13, k, perc, min_len, on_device,
                                                 range_off.ctypes.data_as(U64P), ranges.ctypes.data_as(U64P), 500,
                                                 status.ctypes.data_as(C.POINTER(C.c_int32))), ctx.handle)
        got = [[(int(ranges[2 * r]), int(ranges[2 * r + 1])) for r in range(int(range_off[s]), int(range_off[s + 1]))] for s in range(3)]
        assert got == want and np.all(status == apd.APD_OK)
    # the same for samples: 333 samples of another recording in front
    audio = ramps([333, 5003, 12345])
    samples = np.concatenate(audio)
    sample_off = np.array([333, 333 + 5003, 333 + 5003 + 12345], np.uint64)
    slices = [[(0, 3), (7, 39)], [(2, 50), (50, 96)]]
    want_s = np.concatenate([audio[s + 1][a * 127:b * 127] for s in range(2) for a, b in slices[s]])
    from audio_pattern_discovery_amd.alignments import slice_samples
    assert np.array_equal(slice_samples(samples, sample_off, slices, 127, ctx), want_s)
    d_out = slice_samples(ctx.upload(samples), sample_off, slices, 127, ctx, on_device=True)
    assert np.array_equal(d_out.to_numpy(np.int16, len(want_s)), want_s)


def test_cepstra_of_gathered_slices_are_the_cepstra_of_host_slices(ctx, apd):
    from audio_pattern_discovery_amd.alignments import NDSequence, slice_offsets, slice_samples
    recs = [synth.make_audio(n, seed=40 + s) for s, n in enumerate((9000, 20011, 4999))]
    fft, step, filt = 256, 128, 18
    ranges = [[(0, 9), (20, 61)], [(5, 6), (30, 150)], [(1, 30)]]
    sample_off = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.uint64)
    d_samples = ctx.upload(np.concatenate(recs).astype(np.int16))
    d_slices = slice_samples(d_samples, sample_off, ranges, step, ctx, on_device=True)
    offs, seq = slice_offsets(sample_off, ranges, step)
    assert seq.tolist() == [0, 0, 1, 1, 2]
    L = apd.lib()
    f_off, nb = np.zeros(len(offs), np.uint64), C.c_uint32(0)
    head = (ctx.handle, d_slices.at(), offs.ctypes.data_as(U64P), len(offs) - 1, fft, step, filt, 1)
    apd.check(L.apd_cepstrum_batch(*head, None, f_off.ctypes.data_as(U64P), C.byref(nb)), ctx.handle)
    d_ceps = ctx.alloc(int(f_off[-1]) * nb.value * 4)
    apd.check(L.apd_cepstrum_batch(*head, d_ceps.at(), f_off.ctypes.data_as(U64P), C.byref(nb)), ctx.handle)
    got = d_ceps.to_numpy(np.float32).reshape(-1, nb.value)
    r = 0
    for s, rec in enumerate(recs):
        for a, b in ranges[s]:
            want = NDSequence.new(fft, step, filt, rec[a * step:b * step], ctx).frames
            mine = got[int(f_off[r]):int(f_off[r + 1])]
            assert mine.shape == want.shape and np.array_equal(mine.view(np.uint32), want.view(np.uint32)), (s, a, b)
            r += 1
    assert int(f_off[-1]) > 100


def test_segment_equals_the_single_recording_calls(ctx, apd, oracle):
    """`segment` over the corpus against main.rs:58-92 done per recording; the ranges of a recording also against the oracle on the
    GPU's own cepstrum frames of it, since the single call runs the batch's kernels."""
    from audio_pattern_discovery_amd.alignments import NDSequence, segment
    from audio_pattern_discovery_amd.discovery import Discovery
    cfg = Discovery(dft_win=256, dft_step=128, ceps_filter=18, vat_moving=15, vat_percentile=0.6, vat_min_len=10)
    recs = []
    for s, n in enumerate((30000, 52013, 18000, 41111)):
        audio = synth.make_audio(n, seed=70 + s).astype(np.int32)
        audio[n // 3:n // 2] //= 8                                  # a quiet stretch: the variance of the cepstrum moves
        recs.append(audio.astype(np.int16))
    sample_off = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.uint64)
    d_slices, slice_off, slice_seq, ranges = segment(np.concatenate(recs), sample_off, cfg, ctx)
    want_ranges, want_slices, want_seq = [], [], []
    for s, rec in enumerate(recs):                                  # main.rs:58-92 per recording
        seq = NDSequence.new(cfg.dft_win, cfg.dft_step, cfg.ceps_filter, rec, ctx)
        found = [(sl.start, sl.stop) for sl in seq.interesting_ranges(cfg.vat_moving, cfg.vat_percentile, cfg.vat_min_len, ctx)]
        assert found == oracle.interesting_ranges(seq.frames, cfg.vat_moving, cfg.vat_percentile, cfg.vat_min_len)
        want_ranges.append(found)
        want_slices += [rec[a * cfg.dft_step:b * cfg.dft_step] for a, b in found]
        want_seq += [s] * len(found)
    assert ranges == want_ranges and sum(len(r) for r in ranges) >= 4
    assert slice_seq.tolist() == want_seq
    assert slice_off.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want_slices])]).tolist()
    assert np.array_equal(d_slices.to_numpy(np.int16, int(slice_off[-1])), np.concatenate(want_slices))


def test_python_wrapper_strict_and_lenient(ctx, apd):
    from audio_pattern_discovery_amd.alignments import interesting_ranges_batch
    a_list, n_bins = kat_batch()
    recs = [cc.alternating(a, n_bins) for a in a_list]
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in recs])])
    want = [cc.integer_ranges(a, cc.KAT_K, index_of(len(a), cc.KAT_PERC), cc.KAT_MIN_LEN)[0] for a in a_list]
    assert interesting_ranges_batch(np.concatenate(recs), offsets, cc.KAT_K, cc.KAT_PERC, cc.KAT_MIN_LEN, ctx) == want
    with_empty = np.concatenate([offsets, offsets[-1:]])
    got, status = interesting_ranges_batch(np.concatenate(recs), with_empty, cc.KAT_K, cc.KAT_PERC, cc.KAT_MIN_LEN, ctx, strict=False)
    assert got == want + [[]] and status == [apd.APD_OK] * 3 + [apd.APD_ERR_INDEX]
    with pytest.raises(apd.ApdError) as e:
        interesting_ranges_batch(np.concatenate(recs), with_empty, cc.KAT_K, cc.KAT_PERC, cc.KAT_MIN_LEN, ctx)
    assert e.value.status == apd.APD_ERR_INDEX
