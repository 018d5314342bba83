"""CPU tests of the cross-alignment entry points: without a device there is no context, and every call refuses its NULL or
mismatched arguments with APD_ERR_INVALID_ARG before it touches the GPU."""
import ctypes as C

import numpy as np


def test_cross_calls_refuse_null_arguments_without_a_device(apd):
    L = apd.lib()
    bad = apd.APD_ERR_INVALID_ARG
    h = C.c_void_p(0x1234)                                          # never dereferenced: a NULL beside it decides first
    out = C.c_void_p(7)
    assert L.apd_batch_join(None, None, None, C.byref(out)) == bad
    assert L.apd_batch_join(None, h, h, C.byref(out)) == bad
    assert L.apd_batch_join(None, None, None, None) == bad
    assert L.apd_batch_first_len(None) == 0 and L.apd_batch_len(None) == 0
    cfg = apd.AlignConfig(0.0625, 1, 1, 1)
    buf = np.zeros(4, np.float32)
    f32p = buf.ctypes.data_as(C.POINTER(C.c_float))
    assert L.apd_align_cross(None, None, C.byref(cfg), f32p, f32p) == bad
    assert L.apd_align_cross(None, h, C.byref(cfg), f32p, f32p) == bad
    assert L.apd_align_cross(None, None, None, None, None) == bad
    assert L.apd_align_cross_device_async(None, None, C.byref(cfg), C.c_void_p(buf.ctypes.data), None) == bad
    assert L.apd_align_cross_device_async(None, h, None, None, None) == bad
    members, set_off = np.array([0, 1], np.uint32), np.array([0, 2], np.uint32)
    u32p = C.POINTER(C.c_uint32)
    v = C.c_void_p(buf.ctypes.data)
    assert L.apd_cross_linkage(None, v, v, 0, 2, 2, members.ctypes.data_as(u32p), set_off.ctypes.data_as(u32p), 1, v, v, v, v) == bad
    assert L.apd_cross_linkage(None, None, None, 0, 0, 0, None, None, 0, None, None, None, None) == bad


def test_python_mirrors_refuse_mismatched_shapes():
    import pytest
    from audio_pattern_discovery_amd.clustering import cross_linkage
    with pytest.raises(ValueError):
        cross_linkage(np.zeros((3, 4), np.float32), np.zeros((3, 4), np.float32), [[0]], ctx=object())
