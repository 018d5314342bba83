"""CPU tests of the entry points of a streaming session's history (include/apd.h, "a kept history of columns"): the library exports
them, the ctypes table binds them, and arguments that can be refused without a device are."""
import ctypes as C

import numpy as np

SYMBOLS = ("apd_spot_stream_keep", "apd_spot_stream_history", "apd_spot_stream_paths")


def test_library_exports_the_three_entry_points(apd):
    L = apd.lib()
    bound = {n for n, _, _ in apd.SYMBOLS}
    for name in SYMBOLS:
        assert hasattr(L, name), "libapd_hip.so does not export %s" % name
        assert name in bound, "the ctypes table does not bind %s" % name


def test_null_arguments_are_refused_without_a_device(apd):
    L = apd.lib()
    bad = apd.APD_ERR_INVALID_ARG
    assert L.apd_spot_stream_keep(None, None, 16) == bad
    first, last = C.c_uint64(7), C.c_uint64(9)
    assert L.apd_spot_stream_history(None, 0, C.byref(first), C.byref(last)) == bad and (first.value, last.value) == (7, 9)
    windows = np.zeros(1, dtype=np.dtype([("x", np.uint32), ("y", np.uint32), ("end", np.uint32), ("start", np.uint32)]))
    step_off = np.full(2, 9, dtype=np.uint64)
    u64p = C.POINTER(C.c_uint64)
    assert L.apd_spot_stream_paths(None, None, windows.ctypes.data_as(C.POINTER(apd.SpotWindow)), 1, None, 0, step_off.ctypes.data_as(u64p),
                                   None, None, None) == bad
    assert step_off.tolist() == [9, 9]


def test_python_session_has_the_history_methods():
    from audio_pattern_discovery_amd.alignments import AlignmentWorkers, SpotStream
    import inspect
    assert "history" in inspect.signature(AlignmentWorkers.spot_stream).parameters
    for name in ("keep", "history", "paths"):
        assert callable(getattr(SpotStream, name))
