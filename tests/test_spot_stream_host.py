"""CPU tests of the streaming spotting entry points (include/apd.h, "streaming spotting"): the library exports them, the ctypes table
binds them, and arguments that can be refused without a device are."""
import ctypes as C

import numpy as np

SYMBOLS = ("apd_spot_stream_create", "apd_spot_stream_destroy", "apd_spot_stream_reset", "apd_spot_stream_columns", "apd_spot_stream_push")


def test_library_exports_the_five_entry_points(apd):
    L = apd.lib()
    bound = {n for n, _, _ in apd.SYMBOLS}
    for name in SYMBOLS:
        assert hasattr(L, name), "libapd_hip.so does not export %s" % name
        assert name in bound, "the ctypes table does not bind %s" % name


def test_null_arguments_are_refused_without_a_device(apd):
    L = apd.lib()
    bad = apd.APD_ERR_INVALID_ARG
    cfg = apd.AlignConfig(0.0, 1.0, 1.0, 1.0)
    queries = np.zeros(1, dtype=np.uint32)
    qp = queries.ctypes.data_as(C.POINTER(C.c_uint32))
    handle = C.c_void_p()
    assert L.apd_spot_stream_create(None, None, C.byref(cfg), qp, 1, 1, C.byref(handle)) == bad
    assert L.apd_spot_stream_create(None, None, None, None, 0, 0, None) == bad
    assert not handle.value
    assert L.apd_spot_stream_destroy(None) == bad
    assert L.apd_spot_stream_reset(None, None, 0, 0) == bad
    columns = C.c_uint64(7)
    assert L.apd_spot_stream_columns(None, 0, C.byref(columns)) == bad and columns.value == 7
    chunk_off = np.zeros(2, dtype=np.uint64)
    curve_off = np.full(2, 9, dtype=np.uint64)
    u64p = C.POINTER(C.c_uint64)
    assert L.apd_spot_stream_push(None, None, None, chunk_off.ctypes.data_as(u64p), 1, 0, None, None, 0, curve_off.ctypes.data_as(u64p), None) == bad
    assert curve_off.tolist() == [9, 9]
