"""CPU tests of the audio feed's entry points (include/apd.h, "raw audio in chunks"): the library exports them, the ctypes table binds
them, and arguments that can be refused without a device are, with their outputs untouched."""
import ctypes as C

import numpy as np

SYMBOLS = ("apd_cepstrum_frames", "apd_feed_create", "apd_feed_destroy", "apd_feed_reset", "apd_feed_totals", "apd_feed_push",
           "apd_spot_stream_push_audio")


def test_library_exports_the_seven_entry_points(apd):
    L = apd.lib()
    bound = {n for n, _, _ in apd.SYMBOLS}
    for name in SYMBOLS:
        assert hasattr(L, name), "libapd_hip.so does not export %s" % name
        assert name in bound, "the ctypes table does not bind %s" % name


def test_null_arguments_are_refused_without_a_device(apd):
    L = apd.lib()
    bad = apd.APD_ERR_INVALID_ARG
    u64p = C.POINTER(C.c_uint64)
    handle, dim = C.c_void_p(), C.c_uint32(77)
    assert L.apd_feed_create(None, 1, 64, 16, 16, None, C.byref(dim), C.byref(handle)) == bad
    assert L.apd_feed_create(None, 0, 0, 0, 0, None, None, None) == bad
    assert not handle.value and dim.value == 77
    assert L.apd_feed_destroy(None) == bad
    assert L.apd_feed_reset(None, None, 0) == bad
    samples, frames = C.c_uint64(5), C.c_uint64(6)
    assert L.apd_feed_totals(None, 0, C.byref(samples), C.byref(frames)) == bad
    assert (samples.value, frames.value) == (5, 6)
    sample_off = np.zeros(2, dtype=np.uint64)
    frame_off = np.full(2, 9, dtype=np.uint64)
    audio = np.zeros(4, dtype=np.int16)
    assert L.apd_feed_push(None, None, audio.ctypes.data, sample_off.ctypes.data_as(u64p), 0, None, 0, 0, frame_off.ctypes.data_as(u64p)) == bad
    assert frame_off.tolist() == [9, 9]
    curve_off = np.full(2, 9, dtype=np.uint64)
    assert L.apd_spot_stream_push_audio(None, None, None, audio.ctypes.data, sample_off.ctypes.data_as(u64p), 0, None, None, 0,
                                        curve_off.ctypes.data_as(u64p), None) == bad
    assert curve_off.tolist() == [9, 9]


def test_frame_count_needs_no_context(apd):
    """apd_cepstrum_frames is pure host arithmetic: n > fft ? ceil((n - fft) / step) : 0."""
    L = apd.lib()
    assert [int(L.apd_cepstrum_frames(n, 256, 128)) for n in (0, 256, 257, 384, 385, 2 ** 40)] == [0, 0, 1, 1, 2, (2 ** 40 - 256 + 127) // 128]
