"""apd_slice_offsets (host only, no GPU): the sample offsets of the sliced corpus -- slice r of recording s is
samples[sample_offsets[s] + start * fft_step .. sample_offsets[s] + stop * fft_step) (main.rs:81-88) -- against a three-line numpy
definition over random ranges, slice_seq, and the argument errors include/apd.h lists."""
import ctypes as C

import numpy as np

U64P, U32P = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
SENTINEL = np.uint64(0xDEADBEEFDEADBEEF)


def call(apd, sample_off, range_off, ranges, fft_step, with_seq=True):
    sample_off, range_off = np.asarray(sample_off, np.uint64), np.asarray(range_off, np.uint64)
    ranges = np.asarray(ranges, np.uint64).ravel()
    n_slices = int(range_off[-1])
    out = np.full(n_slices + 2, SENTINEL, np.uint64)
    seq = np.full(n_slices + 1, 0xABCDABCD, np.uint32)
    rc = apd.lib().apd_slice_offsets(sample_off.ctypes.data_as(U64P), range_off.ctypes.data_as(U64P),
                                     ranges.ctypes.data_as(U64P) if ranges.size else None, len(range_off) - 1, fft_step,
                                     out.ctypes.data_as(U64P), seq.ctypes.data_as(U32P) if with_seq else None)
    return rc, out, seq


def random_case(rng, n_seq, fft_step):
    """Recordings of random lengths (some shorter than a step), each with 0 .. 6 ascending disjoint ranges inside it."""
    lens = rng.integers(0, 40 * fft_step, n_seq)
    lens[rng.random(n_seq) < 0.2] = 0                                       # a few empty recordings
    sample_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    ranges, range_off = [], [0]
    for s in range(n_seq):
        frames = int(lens[s]) // fft_step
        cuts = np.sort(rng.choice(frames + 1, size=min(2 * int(rng.integers(0, 7)), frames + 1) // 2 * 2, replace=False)) if frames else []
        ranges += [(int(cuts[2 * i]), int(cuts[2 * i + 1])) for i in range(len(cuts) // 2)]
        range_off.append(len(ranges))
    return sample_off, np.array(range_off, np.uint64), np.array(ranges, np.uint64).reshape(-1, 2)


def test_offsets_and_slice_seq_against_the_numpy_definition(apd):
    rng = np.random.default_rng(20261020)
    seen = 0
    for fft_step in (1, 127, 128):
        for n_seq in (1, 2, 9, 40):
            sample_off, range_off, ranges = random_case(rng, n_seq, fft_step)
            # the definition
            lengths = (ranges[:, 1] - ranges[:, 0]) * np.uint64(fft_step)
            want = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
            want_seq = np.repeat(np.arange(n_seq), np.diff(range_off).astype(np.int64)).astype(np.uint32)
            for with_seq in (True, False):
                rc, out, seq = call(apd, sample_off, range_off, ranges, fft_step, with_seq)
                assert rc == apd.APD_OK
                assert np.array_equal(out[:len(want)], want) and out[len(want)] == SENTINEL
                if with_seq:
                    assert np.array_equal(seq[:len(want_seq)], want_seq) and seq[len(want_seq)] == 0xABCDABCD
                else:
                    assert np.all(seq == 0xABCDABCD)
            seen += len(ranges)
    assert seen > 100


def test_a_range_may_end_exactly_at_its_recording_and_touch_its_neighbour(apd):
    # 1000 samples, step 100: frames 0 .. 10; [0, 3) [3, 3) [3, 10) are ascending (a start may equal the previous stop), 10 * 100 == 1000
    rc, out, seq = call(apd, [5, 1005], [0, 3], [(0, 3), (3, 3), (3, 10)], 100)
    assert rc == apd.APD_OK and out[:4].tolist() == [0, 300, 300, 1000] and seq[:3].tolist() == [0, 0, 0]


def test_invalid_ranges_are_refused(apd):
    ok = ([0, 1000, 1500], [0, 2, 3], [(1, 3), (5, 8), (0, 2)], 100)
    assert call(apd, *ok)[0] == apd.APD_OK
    # a range that runs past its recording: stop * fft_step > length (the second recording has 500 samples: 5 frames)
    assert call(apd, [0, 1000, 1500], [0, 2, 3], [(1, 3), (5, 8), (0, 6)], 100)[0] == apd.APD_ERR_INVALID_ARG
    assert call(apd, [0, 1000, 1500], [0, 2, 3], [(1, 3), (5, 11), (0, 2)], 100)[0] == apd.APD_ERR_INVALID_ARG
    assert call(apd, [0, 1000, 1500], [0, 2, 3], [(1, 3), (5, 2 ** 63), (0, 2)], 100)[0] == apd.APD_ERR_INVALID_ARG    # no overflow
    # stop < start
    assert call(apd, [0, 1000, 1500], [0, 2, 3], [(3, 1), (5, 8), (0, 2)], 100)[0] == apd.APD_ERR_INVALID_ARG
    # the ranges of a recording not ascending; the same pairs in ascending order pass, and so do equal ranges of DIFFERENT recordings
    assert call(apd, [0, 1000, 1500], [0, 2, 3], [(5, 8), (1, 3), (0, 2)], 100)[0] == apd.APD_ERR_INVALID_ARG
    assert call(apd, [0, 1000, 1500], [0, 2, 3], [(1, 6), (5, 8), (0, 2)], 100)[0] == apd.APD_ERR_INVALID_ARG
    assert call(apd, [0, 1000, 2000], [0, 1, 2], [(1, 6), (1, 6)], 100)[0] == apd.APD_OK
    # descending offsets of either kind
    assert call(apd, [0, 1000, 900], [0, 2, 3], [(1, 3), (5, 8), (0, 2)], 100)[0] == apd.APD_ERR_INVALID_ARG
    assert call(apd, [0, 1000, 1500], [0, 3, 2], [(1, 3), (5, 8), (9, 10)], 100)[0] == apd.APD_ERR_INVALID_ARG
    # a descent LATER in range_off is found before anything is written: the outputs are sized from range_off[n_seq] = 2, recording
    # 0 alone names five slices, and the guarded arrays stay untouched
    sample_off, range_off = np.array([0, 1000, 1500], np.uint64), np.array([0, 5, 2], np.uint64)
    ranges = np.array([(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)], np.uint64).ravel()
    out, seq = np.full(3 + 8, SENTINEL, np.uint64), np.full(2 + 8, 0xABCDABCD, np.uint32)
    rc = apd.lib().apd_slice_offsets(sample_off.ctypes.data_as(U64P), range_off.ctypes.data_as(U64P), ranges.ctypes.data_as(U64P), 2, 100,
                                     out.ctypes.data_as(U64P), seq.ctypes.data_as(U32P))
    assert rc == apd.APD_ERR_INVALID_ARG and np.all(out == SENTINEL) and np.all(seq == 0xABCDABCD)
    # range_off that does not start at 0, and descending sample offsets behind valid ranges: nothing written either
    for so, ro in (([0, 1000, 1500], [1, 3, 5]), ([0, 1000, 900], [0, 3, 5])):
        out[:] = SENTINEL
        rc = apd.lib().apd_slice_offsets(np.array(so, np.uint64).ctypes.data_as(U64P), np.array(ro, np.uint64).ctypes.data_as(U64P),
                                         ranges.ctypes.data_as(U64P), 2, 100, out.ctypes.data_as(U64P), None)
        assert rc == apd.APD_ERR_INVALID_ARG and np.all(out == SENTINEL)
    # NULL where data is due
    L = apd.lib()
    off = np.array([0, 10], np.uint64)
    assert L.apd_slice_offsets(off.ctypes.data_as(U64P), off.ctypes.data_as(U64P), None, 1, 1, None, None) == apd.APD_ERR_INVALID_ARG
    out = np.zeros(12, np.uint64)
    assert L.apd_slice_offsets(off.ctypes.data_as(U64P), np.array([0, 1], np.uint64).ctypes.data_as(U64P), None, 1, 1,
                               out.ctypes.data_as(U64P), None) == apd.APD_ERR_INVALID_ARG


def test_no_recordings_and_no_ranges(apd):
    rc, out, seq = call(apd, [0], [0], [], 128)
    assert rc == apd.APD_OK and out[0] == 0 and out[1] == SENTINEL
    rc, out, seq = call(apd, [0, 500, 500, 900], [0, 0, 0, 0], [], 128)
    assert rc == apd.APD_OK and out[0] == 0 and out[1] == SENTINEL and np.all(seq == 0xABCDABCD)


def test_python_wrapper(apd):
    from audio_pattern_discovery_amd.alignments import slice_offsets
    offs, seq = slice_offsets([0, 1000, 1500], [[(1, 3), (5, 8)], [(0, 2)]], 100)
    assert offs.tolist() == [0, 200, 500, 700] and seq.tolist() == [0, 0, 1]
    offs, seq = slice_offsets([0, 1000], [[]], 100)
    assert offs.tolist() == [0] and seq.tolist() == []
