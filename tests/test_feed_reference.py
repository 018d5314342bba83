"""CPU tests of the framing contract of an apd_feed: apd_cepstrum_frames (host only) against the oracle's cepstrum frame count, and
the numpy checker of tests/_feed_reference.py against itself -- per-push counts sum to the whole recording's, the carried tail
never exceeds the window, samples are skipped only when the step is longer than the window."""
import numpy as np
import pytest

import _feed_reference as ref

# (fft, step, filter): every filter size passes apd_cepstrum's K >= 5 check, which reads the window and filter size only.  No
# filter size does for a window of 8 (K is at most 2 there: the smallest window with K >= 5 is 14), so the oracle refuses (8, 1)
# whatever the filter: that shape is counted against the reference's loop alone, and (16, 1) stands beside it with the oracle.
SHAPES = [(64, 16, 16), (48, 20, 12), (32, 40, 8), (8, 1, None), (16, 1, 8)]


@pytest.mark.parametrize("fft,step,filt", SHAPES)
def test_frame_count_equals_the_oracles(apd, oracle, fft, step, filt):
    """Every n in 0 .. fft + 3 step + 2: below a window 0 frames, frame k absent at n = fft + k step and present one sample later."""
    L = apd.lib()
    audio = np.arange(fft + 3 * step + 2, dtype=np.int16)
    for n in range(len(audio) + 1):
        want = len(oracle.cepstrum(audio[:n], fft, step, filt)) if filt else len(range(fft, n, step))   # spectrogram.rs:51
        assert int(L.apd_cepstrum_frames(n, fft, step)) == want == ref.frames_of(n, fft, step), n
    for k in range(4):
        assert int(L.apd_cepstrum_frames(fft + k * step, fft, step)) == k
        assert int(L.apd_cepstrum_frames(fft + k * step + 1, fft, step)) == k + 1
    assert int(L.apd_cepstrum_frames(10 * fft, fft, 0)) == 0
    if filt is None:
        assert all(len(oracle.cepstrum(audio, fft, step, f)) == 0 for f in range(1, fft + 1))   # no filter size makes the window legal


@pytest.mark.parametrize("fft,step,filt", SHAPES)
def test_push_counts_sum_to_the_recording(fft, step, filt):
    rng = np.random.default_rng(1000 * fft + step)
    for trial in range(50):
        n = int(rng.integers(0, fft + 40 * step))
        lengths = ref.random_split(rng, n, int(rng.integers(1, 12)))
        assert sum(lengths) == n
        ranges, states = ref.pushes(fft, step, lengths)
        assert ranges[0][0] == 0 and ranges[-1][1] == ref.frames_of(n, fft, step)
        assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:])) and all(a <= b for a, b in ranges)
        whole = np.arange(ref.frames_of(n, fft, step) * 3).reshape(-1, 3)
        got = ref.rows(whole, fft, step, lengths)
        assert np.array_equal(np.concatenate(got) if got else whole[:0], whole)


@pytest.mark.parametrize("fft,step,filt", SHAPES)
def test_carried_state_is_bounded(fft, step, filt):
    rng = np.random.default_rng(7 * fft + step)
    for trial in range(50):
        lengths = [int(v) for v in rng.integers(0, 2 * max(fft, step), size=10)] + [1] * 5
        _, states = ref.pushes(fft, step, lengths)
        for tail, skip in states:
            assert 0 <= tail <= fft
            assert skip == 0 or (step > fft and tail == 0 and skip <= step - fft)
