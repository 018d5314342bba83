"""GPU tests of the audio feed (apd_feed_*, apd_spot_stream_push_audio; kernel feed_frames_kernel of csrc/companions.hip).

The promise under test takes no tolerance: the frames of the pushes, one after the other, are the bits of apd_cepstrum (+ apd_encode)
on the whole recording through the same library, whatever the chunking (uint32 views, np.array_equal).  Which frames a push must
return comes from the checker tests/_feed_reference.py.  The one comparison with a tolerance is the cross-check against the oracle's
cepstrum, at tests/test_gpu_cepstrum.py's own bound.

A window of 8 samples has no legal filter size (K is at most 2), so apd_feed_create refuses it as apd_cepstrum does; the step-1 shape
fed sample by sample is (16, 1) with filter 8, the smallest power-of-two window that runs."""
import ctypes as C

import numpy as np
import pytest

import _feed_reference as ref
from audio_pattern_discovery_amd.alignments import SPOT_WINDOW, AlignmentWorkers, AudioFeed, NDSequence
from audio_pattern_discovery_amd.discovery import Discovery
from test_gpu_cepstrum import ATOL

pytestmark = pytest.mark.gpu
u64p = C.POINTER(C.c_uint64)
f32p = C.POINTER(C.c_float)
SHAPES = [(64, 16, 16), (48, 20, 12), (32, 40, 8), (16, 1, 8)]        # (fft, step, filter)
SAMPLE_BY_SAMPLE = [(32, 40, 8), (16, 1, 8)]


@pytest.fixture(scope="module")
def ctx(apd):
    c = apd.Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(got, want):
    return got.shape == want.shape and np.array_equal(bits(got), bits(want))


def noise(n, seed):
    return np.random.default_rng(seed).integers(-32768, 32768, size=n).astype(np.int16)


_whole = {}


def whole(apd, ctx, audio, fft, step, filt):
    """apd_cepstrum of a whole recording (host arrays): [T][n_bins]; computed once per recording and shape."""
    key = (audio.tobytes(), fft, step, filt)
    if key not in _whole:
        L = apd.lib()
        t, nb = C.c_uint64(0), C.c_uint32(0)
        apd.check(L.apd_cepstrum(ctx.handle, audio.ctypes.data, audio.size, fft, step, filt, 0, None, C.byref(t), C.byref(nb)), ctx.handle)
        out = np.full((int(t.value), nb.value), np.nan, np.float32)
        if out.size:
            apd.check(L.apd_cepstrum(ctx.handle, audio.ctypes.data, audio.size, fft, step, filt, 0, out.ctypes.data, C.byref(t), C.byref(nb)),
                      ctx.handle)
        out.setflags(write=False)
        _whole[key] = out
    return _whole[key]


def encode(apd, ctx, x, w, b):
    out = np.full((len(x), w.shape[1]), np.nan, np.float32)
    x = np.ascontiguousarray(x, np.float32)
    apd.check(apd.lib().apd_encode(ctx.handle, x.ctypes.data, len(x), x.shape[1], w.ctypes.data_as(f32p), b.ctypes.data_as(f32p), w.shape[1], 0,
                                   out.ctypes.data), ctx.handle)
    return out


def recordings(fft, step, seed):
    """3 channels of different lengths, about 40 frames each; the last ends exactly at a window's end (its last frame absent)."""
    return [noise(fft + step * 37 + 1, seed), noise(fft + step * 40 + 3, seed + 1), noise(fft + step * 42, seed + 2)]


def feed_split(feed, recs, splits, fft, step):
    """Feeds channel k its recording in pieces of splits[k] (lists of equal length); checks every push's row counts against the
    checker and returns the concatenated rows per channel."""
    n_push = len(splits[0])
    assert all(len(s) == n_push for s in splits) and all(sum(s) == len(r) for s, r in zip(splits, recs))
    want = [ref.pushes(fft, step, s)[0] for s in splits]
    pos = [0] * len(recs)
    got = [[] for _ in recs]
    for i in range(n_push):
        chunks = [r[p:p + s[i]] for r, p, s in zip(recs, pos, splits)]
        rows = feed.push(chunks)
        for k, r in enumerate(rows):
            assert len(r) == want[k][i][1] - want[k][i][0], "push %d, channel %d" % (i, k)
            got[k].append(r)
            pos[k] += splits[k][i]
    return [np.concatenate(g) for g in got]


def check_split(apd, ctx, recs, splits, fft, step, filt):
    feed = AudioFeed(ctx, len(recs), fft, step, filt)
    try:
        got = feed_split(feed, recs, splits, fft, step)
        for k, r in enumerate(recs):
            want = whole(apd, ctx, r, fft, step, filt)
            assert feed.dim == want.shape[1]
            assert same(got[k], want), "channel %d" % k
            assert feed.totals(k) == (len(r), len(want))
    finally:
        feed.close()


def padded(splits):
    n = max(len(s) for s in splits)
    return [list(s) + [0] * (n - len(s)) for s in splits]


# ------------------------------------------------------------------------------------------------ chunking invariance

@pytest.mark.parametrize("fft,step,filt", SHAPES)
def test_one_piece(apd, ctx, fft, step, filt):
    recs = recordings(fft, step, 10 * fft)
    check_split(apd, ctx, recs, [[len(r)] for r in recs], fft, step, filt)


@pytest.mark.parametrize("fft,step,filt", SAMPLE_BY_SAMPLE)
def test_single_samples(apd, ctx, fft, step, filt):
    recs = recordings(fft, step, 11 * fft)
    check_split(apd, ctx, recs, padded([[1] * len(r) for r in recs]), fft, step, filt)


@pytest.mark.parametrize("fft,step,filt", SHAPES)
def test_cut_at_a_windows_end_and_one_sample_later(apd, ctx, fft, step, filt):
    """A push that ends exactly at fft + k step does not emit frame k; the one-sample push behind it emits exactly that frame."""
    recs = recordings(fft, step, 12 * fft)
    splits = []
    for k, r in zip(((0, 1, 5), (2, 3), (7, 30)), recs):
        cuts = sorted({fft + q * step for q in k} | {fft + q * step + 1 for q in k})
        splits.append(np.diff([0] + cuts + [len(r)]).tolist())
        ranges = ref.pushes(fft, step, splits[-1])[0]
        for q in k:
            i = cuts.index(fft + q * step)
            assert ranges[i][1] == q and ranges[i + 1] == (q, q + 1)
    check_split(apd, ctx, recs, padded(splits), fft, step, filt)


@pytest.mark.parametrize("fft,step,filt", SHAPES)
def test_random_pieces(apd, ctx, fft, step, filt):
    """Seeded random pieces, empty ones among them, and a channel that idles for several pushes in mid-recording."""
    rng = np.random.default_rng(13 * fft + step)
    for trial in range(3):
        recs = recordings(fft, step, 14 * fft + trial)
        splits = [ref.random_split(rng, len(r), 9, empty=0.3) for r in recs]
        splits[trial] = splits[trial][:4] + [0, 0, 0, 0] + splits[trial][4:]         # this channel idles while the others go on
        check_split(apd, ctx, recs, padded(splits), fft, step, filt)


# ------------------------------------------------------------------------------------------------ every frame-body variant

VARIANTS = {
    # two frames per wavefront; pushes of 7, 0, 1 and 3 frames (odd counts leave a half-wave idle)
    "two frames per wavefront": (64, 16, 16, [64 + 16 * 6 + 1, 5, 11, 16 * 3]),
    # one frame per wavefront; the tail grows to the full 2048 samples, then windows straddle tail and chunk
    "one frame per wavefront": (2048, 512, 64, [1000, 1048, 1, 700, 2048 + 512 * 3 + 1 - 2749]),
    "direct sum": (48, 20, 12, [30, 48, 20 * 4 + 1, 7]),
    # K = 510: the DCT table read from global memory; 3 frames
    "dct in global memory": (4096, 1024, 512, [3000, 2000, 4096 + 2 * 1024 + 1 - 5000]),
    # step > fft: the first chunk ends inside the gap behind window 0 (5 samples to skip), the second still inside it (2 left)
    "skipped samples": (32, 40, 8, [35, 3, 40 * 5, 1, 33]),
}


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_frame_body_variants(apd, ctx, name):
    fft, step, filt, split = VARIANTS[name]
    assert all(s >= 0 for s in split)
    rec = noise(sum(split), len(name))
    assert len(whole(apd, ctx, rec, fft, step, filt)) >= 3
    check_split(apd, ctx, [rec], [split], fft, step, filt)
    if name == "skipped samples":
        _, states = ref.pushes(fft, step, split)
        assert states[0] == (0, 5) and states[1] == (0, 2)
    if name == "one frame per wavefront":
        assert ref.pushes(fft, step, split)[1][1] == (2048, 0)


def test_silence_and_full_scale_across_a_boundary(apd, ctx):
    fft, step, filt = 64, 16, 16
    loud = np.where(np.arange(200) % 2 == 0, 32767, -32768).astype(np.int16)
    rec = np.concatenate([np.zeros(150, np.int16), loud, np.zeros(150, np.int16), np.full(100, -32768, np.int16)])
    check_split(apd, ctx, [rec, rec[::-1].copy()], [[150, 100, 130, 220], [170, 180, 1, 249]], fft, step, filt)


def test_a_window_without_a_legal_filter_is_refused(apd, ctx):
    with pytest.raises(apd.ApdError) as e:
        AudioFeed(ctx, 1, 8, 1, 8)
    assert e.value.status == apd.APD_ERR_INVALID_ARG
    with pytest.raises(apd.ApdError) as e:
        AudioFeed(ctx, 0, 64, 16, 16)
    assert e.value.status == apd.APD_ERR_INVALID_ARG
    with pytest.raises(apd.ApdError) as e:
        AudioFeed(ctx, 1, 8192, 16, 16)
    assert e.value.status == apd.APD_ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------------ encoder fused

def weights(d_in, latent, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(0, 0.3, size=(d_in, latent)).astype(np.float32), rng.normal(0, 0.5, size=latent).astype(np.float32)


@pytest.mark.parametrize("fft,step,filt,latent", [(64, 16, 16, 4), (48, 20, 12, 3), (2048, 512, 64, 5)])
def test_encoder_fused(apd, ctx, fft, step, filt, latent):
    frames = 41 if fft < 2048 else 5
    recs = [noise(fft + step * (frames - 1) + 1, 20 + fft), noise(fft + step * (frames - 2) + 9, 21 + fft)]
    cep = [whole(apd, ctx, r, fft, step, filt) for r in recs]
    if fft == 64:
        assert cep[0].shape[1] == 10
    w, b = weights(cep[0].shape[1], latent, fft)
    rng = np.random.default_rng(fft)
    feed = AudioFeed(ctx, 2, fft, step, filt, encoder=(w, b))
    try:
        assert feed.dim == latent
        got = feed_split(feed, recs, [ref.random_split(rng, len(r), 6) for r in recs], fft, step)
        for g, c in zip(got, cep):
            assert same(g, encode(apd, ctx, c, w, b))
    finally:
        feed.close()


def test_encoder_misfits_are_refused(apd, ctx):
    L = apd.lib()
    other = apd.Context(0)
    try:
        for d_in, owner in ((9, ctx), (10, other)):
            w, b = weights(d_in, 4, 5)
            enc = C.c_void_p()
            apd.check(L.apd_encoder_create(owner.handle, w.ctypes.data_as(f32p), b.ctypes.data_as(f32p), d_in, 4, C.byref(enc)), owner.handle)
            with pytest.raises(apd.ApdError) as e:
                AudioFeed(ctx, 1, 64, 16, 16, encoder=enc)
            assert e.value.status == apd.APD_ERR_INVALID_ARG
            assert L.apd_encoder_destroy(enc) == apd.APD_OK
    finally:
        other.close()


# ------------------------------------------------------------------------------------------------ state

def raw_push(apd, ctx, feed, samples, sample_off, on_device, frames, frames_on_device, capacity):
    off = np.full(len(sample_off), 77, dtype=np.uint64)
    sample_off = np.ascontiguousarray(sample_off, dtype=np.uint64)
    status = apd.lib().apd_feed_push(ctx.handle, feed.handle, samples, sample_off.ctypes.data_as(u64p), int(on_device), frames,
                                     int(frames_on_device), capacity, off.ctypes.data_as(u64p))
    return status, off


def test_queries_and_refused_pushes_do_not_move_the_state(apd, ctx):
    fft, step, filt = 64, 16, 16
    recs = [noise(400, 30), noise(300, 31)]
    want = [whole(apd, ctx, r, fft, step, filt) for r in recs]
    feed = AudioFeed(ctx, 2, fft, step, filt)
    try:
        first = feed.push([recs[0][:100], recs[1][:90]])
        rest = np.concatenate([recs[0][100:], recs[1][90:]])
        off = [0, 300, 510]
        rows = np.full((64, feed.dim), np.nan, np.float32)
        before = [feed.totals(k) for k in range(2)]
        status, f_off = raw_push(apd, ctx, feed, rest.ctypes.data, off, 0, None, 0, 0)                      # sizes only
        assert status == apd.APD_OK and f_off.tolist() == [0, len(want[0]) - len(first[0]), len(want[0]) - len(first[0]) + len(want[1]) - len(first[1])]
        total = int(f_off[-1])
        status, f_off2 = raw_push(apd, ctx, feed, rest.ctypes.data, off, 0, rows.ctypes.data, 0, total - 1)   # capacity too small
        assert status == apd.APD_ERR_INVALID_ARG and np.array_equal(f_off, f_off2) and np.isnan(rows).all()
        status, f_off3 = raw_push(apd, ctx, feed, rest.ctypes.data, [0, 300, 299], 0, rows.ctypes.data, 0, 64)  # descending offsets
        assert status == apd.APD_ERR_INVALID_ARG and f_off3[0] == 0 and f_off3[1] == f_off[1] and np.isnan(rows).all()
        status, _ = raw_push(apd, ctx, feed, None, off, 0, rows.ctypes.data, 0, 64)                          # samples missing
        assert status == apd.APD_ERR_INVALID_ARG
        assert [feed.totals(k) for k in range(2)] == before
        second = feed.push([recs[0][100:], recs[1][90:]])
        for k in range(2):
            assert same(np.concatenate([first[k], second[k]]), want[k])
    finally:
        feed.close()


def test_reset_restarts_one_channel(apd, ctx):
    fft, step, filt = 48, 20, 12
    recs = [noise(500, 40), noise(500, 41)]
    again = noise(300, 42)
    feed = AudioFeed(ctx, 2, fft, step, filt)
    try:
        a = feed.push([recs[0][:250], recs[1][:260]])
        feed.reset(0)
        assert feed.totals(0) == (0, 0) and feed.totals(1)[0] == 260
        b = feed.push([again[:100], recs[1][260:]])
        c = feed.push([again[100:], recs[1][:0]])
        assert same(np.concatenate([b[0], c[0]]), whole(apd, ctx, again, fft, step, filt))
        assert same(np.concatenate([a[1], b[1], c[1]]), whole(apd, ctx, recs[1], fft, step, filt))
        feed.reset()
        assert feed.totals(1) == (0, 0)
        assert same(feed.push([recs[0], recs[1]])[1], whole(apd, ctx, recs[1], fft, step, filt))
    finally:
        feed.close()


def test_host_and_device_arrays_give_the_same_bits(apd, ctx):
    fft, step, filt = 64, 16, 16
    recs = [noise(700, 50), noise(650, 51)]
    want = [whole(apd, ctx, r, fft, step, filt) for r in recs]
    host, dev_in, dev_out = (AudioFeed(ctx, 2, fft, step, filt) for _ in range(3))
    try:
        pos = [0, 0]
        got = [[[], []] for _ in range(3)]
        for lens in ((300, 10), (0, 400), (400, 240)):
            chunks = [r[p:p + n] for r, p, n in zip(recs, pos, lens)]
            pos = [p + n for p, n in zip(pos, lens)]
            packed = np.concatenate(chunks)
            off = np.array([0, lens[0], lens[0] + lens[1]], np.uint64)
            rows_host = host.push(chunks)
            d_samples = ctx.upload(np.concatenate([np.zeros(3, np.int16), packed]))                 # an odd sample offset into the buffer
            rows_dev = dev_in.push((d_samples.ptr, off + 3), on_device=True)
            total = sum(len(r) for r in rows_host)
            d_rows = ctx.alloc(max(total, 1) * host.dim * 4)
            status, f_off = raw_push(apd, ctx, dev_out, packed.ctypes.data, off, 0, d_rows.at(0), 1, total)
            assert status == apd.APD_OK and int(f_off[-1]) == total
            flat = d_rows.to_numpy(np.float32, total * host.dim).reshape(total, host.dim)
            for k in range(2):
                got[0][k].append(rows_host[k])
                got[1][k].append(rows_dev[k])
                got[2][k].append(flat[int(f_off[k]):int(f_off[k + 1])])
            d_samples.free()
            d_rows.free()
        for route in got:
            for k in range(2):
                assert same(np.concatenate(route[k]), want[k])
    finally:
        for f in (host, dev_in, dev_out):
            f.close()


# ------------------------------------------------------------------------------------------------ with a session

FFT, STEP, FILT = 64, 16, 16
PARAMS = Discovery(warping_band_percentage=0.0, insertion_penalty=1.0, deletion_penalty=1.0, match_penalty=0.5)


@pytest.fixture(scope="module")
def session_case(apd, ctx):
    """2 templates of 8 and 12 frames (the first cut out of channel 0, so that something matches), 2 channels of about 40 columns."""
    recs = [noise(FFT + STEP * 39 + 1, 60), noise(FFT + STEP * 42 + 5, 61)]
    frames = [np.array(whole(apd, ctx, r, FFT, STEP, FILT)) for r in recs]
    templates = [frames[0][10:18].copy(), np.array(whole(apd, ctx, noise(FFT + STEP * 11 + 1, 62), FFT, STEP, FILT))]
    assert [len(t) for t in templates] == [8, 12]
    rng = np.random.default_rng(63)
    splits = padded([ref.random_split(rng, len(r), 7) for r in recs])
    workers = AlignmentWorkers.new([NDSequence(t) for t in templates], ctx)
    yield {"recs": recs, "frames": frames, "splits": splits, "workers": workers}
    workers.close()


def chunk_list(recs, splits):
    pos = [0] * len(recs)
    for i in range(len(splits[0])):
        yield [r[p:p + s[i]] for r, p, s in zip(recs, pos, splits)]
        pos = [p + s[i] for p, s in zip(pos, splits)]


def frame_chunks(case):
    """The frames each push of the case's chunking carries, per channel."""
    ranges = [ref.pushes(FFT, STEP, s)[0] for s in case["splits"]]
    for i in range(len(case["splits"][0])):
        yield [f[r[i][0]:r[i][1]] for f, r in zip(case["frames"], ranges)]


def test_push_audio_equals_spot_on_the_whole_recording(apd, ctx, session_case):
    case = session_case
    streams = AlignmentWorkers.new([NDSequence(f) for f in case["frames"]], ctx)
    pairs = [(q, 2 + k) for k in range(2) for q in range(2)]                    # session pair p = channel * 2 + q
    want_curves, want_best = case["workers"].spot(pairs, PARAMS, streams=streams)
    streams.close()
    session = case["workers"].spot_stream([0, 1], PARAMS, channels=2)
    feed = AudioFeed(ctx, 2, FFT, STEP, FILT)
    try:
        cost, start = [[] for _ in pairs], [[] for _ in pairs]
        for chunks in chunk_list(case["recs"], case["splits"]):
            curves, best = session.push_audio(feed, chunks)
            for p, (c, s) in enumerate(curves):
                cost[p].append(c)
                start[p].append(s)
        for p in range(4):
            assert np.array_equal(bits(np.concatenate(cost[p])), bits(want_curves[p][0]))
            assert np.array_equal(np.concatenate(start[p]), want_curves[p][1])
        assert best.tobytes() == want_best.tobytes()
        assert [session.columns(k) for k in range(2)] == [len(f) for f in case["frames"]]
        _, best2 = session.push_audio(feed, [case["recs"][0][:0]] * 2, curves=False)   # nothing new: bests only
        assert best2.tobytes() == want_best.tobytes()
    finally:
        feed.close()
        session.close()


def test_push_audio_hits_and_paths_equal_the_frame_route(apd, ctx, session_case):
    """Armed with holdoff 4 and keeping 16 columns: the drained hits and the paths of the hits still inside the history are those of
    the same session fed the same frames by push()."""
    case = session_case
    streams = AlignmentWorkers.new([NDSequence(f) for f in case["frames"]], ctx)
    _, whole_best = case["workers"].spot([(q, 2 + k) for k in range(2) for q in range(2)], PARAMS, streams=streams)
    streams.close()
    threshold = float(np.median(whole_best["score"])) + 1.0
    results = []
    for route in ("audio", "frames"):
        session = case["workers"].spot_stream([0, 1], PARAMS, channels=2, history=16)
        session.detect(threshold, holdoff=4)
        feed = AudioFeed(ctx, 2, FFT, STEP, FILT)
        try:
            if route == "audio":
                for chunks in chunk_list(case["recs"], case["splits"]):
                    session.push_audio(feed, chunks, curves=False)
            else:
                for chunks in frame_chunks(case):
                    session.push(chunks, curves=False)
            session.flush()
            hits = session.hits()
            windows = np.zeros(len(hits), dtype=SPOT_WINDOW)
            windows["x"], windows["y"], windows["end"], windows["start"] = hits["pair"] % 2, hits["pair"] // 2, hits["end"], hits["start"]
            results.append((hits, session.paths(windows), [session.history(k) for k in range(2)]))
        finally:
            feed.close()
            session.close()
    (hits_a, paths_a, hist_a), (hits_f, paths_f, hist_f) = results
    assert len(hits_f) > 0 and hits_a.tobytes() == hits_f.tobytes()
    assert hist_a == hist_f
    assert any(len(s) for s in paths_f[0])                                      # a hit inside the kept columns was traced
    assert len(paths_a[0]) == len(paths_f[0]) and all(a.tobytes() == f.tobytes() for a, f in zip(paths_a[0], paths_f[0]))
    assert np.array_equal(paths_a[1], paths_f[1]) and np.array_equal(bits(paths_a[2]), bits(paths_f[2]))


def test_a_feed_that_does_not_fit_the_session_is_refused(apd, ctx, session_case):
    case = session_case
    session = case["workers"].spot_stream([0, 1], PARAMS, channels=2)
    other = apd.Context(0)
    misfits = [AudioFeed(ctx, 2, 48, 20, 12), AudioFeed(ctx, 3, FFT, STEP, FILT), AudioFeed(other, 2, FFT, STEP, FILT)]
    try:
        assert misfits[0].dim == 6
        for feed in misfits:
            chunks = [noise(500, 70 + k) for k in range(feed.channels)]
            with pytest.raises(apd.ApdError) as e:
                session.push_audio(feed, chunks)
            assert e.value.status == apd.APD_ERR_INVALID_ARG
            assert [feed.totals(k) for k in range(feed.channels)] == [(0, 0)] * feed.channels
            assert [session.columns(k) for k in range(2)] == [0, 0]
    finally:
        for feed in misfits:
            feed.close()
        other.close()
        session.close()


# ------------------------------------------------------------------------------------------------ against the oracle

def test_chunked_feed_against_the_oracle(apd, ctx, oracle):
    fft, step, filt = 64, 16, 16
    rec = noise(fft + step * 20 + 1, 80)
    feed = AudioFeed(ctx, 1, fft, step, filt)
    try:
        got = feed_split(feed, [rec], [[50, 15, 0, 200, len(rec) - 265]], fft, step)[0]
    finally:
        feed.close()
    want = oracle.cepstrum(rec, fft, step, filt)
    assert got.shape == want.shape == (21, 10)
    np.testing.assert_allclose(got, want, rtol=0, atol=ATOL)
