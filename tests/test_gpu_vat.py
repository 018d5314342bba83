"""The VAT pre-segmentation on the GPU through its single call (apd_interesting_ranges, a batch of one recording through
vat_variance_kernel, vat_select_kernel and vat_scan_kernel of csrc/vat.hip; reference spectrogram.rs:174-216) against the C
oracle, its numpy twin (oracle/np_reference.py) and, where the arithmetic is exact, plain integers.

The call returns integer ranges only.  Random frames rarely put a boundary where an off-by-one window or comparison would
move it, so the known answers use frames [a, -a, a, -a] with small integers a and a power-of-two window: every mean, std
and moving mean is then exact in f32 and the expected ranges are computed here in integer Python (_companion_cases.py).

One property of the reference cannot be observed through ranges: whether the scan starts "recording" (spectrogram.rs:202).
variance[0] is the literal 0.0 for every window k >= 1 (k = 0 panics), and no variance is negative.  With a threshold > 0 the
initial run closes at frame 0 with length 0, which `0 > min_len` never emits; with a threshold of 0 nothing is ever below it and
a scan that starts idle opens its run at frame 0 as well.  Both scans are in the same state after frame 0."""
import ctypes as C

import numpy as np
import pytest

import _companion_cases as cc
from oracle import np_reference as npr

pytestmark = pytest.mark.gpu
SENTINEL = np.uint64(0xDEADBEEFDEADBEEF)


@pytest.fixture(scope="module")
def ctx(apd):
    c = apd.Context(0)
    yield c
    c.close()


def gpu_ranges(apd, ctx, frames, k, perc, min_len, form="host", capacity=None, null_ranges=False):
    """apd_interesting_ranges in one of its forms -> (status, *n_ranges, the whole ranges array as passed).
    form: "host", "host+4" (frames one float past a 16-byte boundary), "device", "device+4"."""
    f = np.ascontiguousarray(frames, dtype=np.float32)
    t, n_bins = f.shape
    keep = None
    if form.startswith("host"):
        raw = np.empty(f.size + 8, dtype=np.float32)
        first = ((-raw.ctypes.data) % 16) // 4 + (1 if form.endswith("+4") else 0)
        host = raw[first:first + f.size]
        host[:] = f.ravel()
        assert host.ctypes.data % 16 == (4 if form.endswith("+4") else 0)
        ptr, on_device, keep = C.c_void_p(host.ctypes.data if t else None), 0, raw
    else:
        off = 4 if form.endswith("+4") else 0
        keep = ctx.alloc(f.nbytes + 16)
        keep.copy_from(f.ravel(), byte_offset=off)
        assert keep.ptr % 16 == 0
        ptr, on_device = keep.at(off), 1
    capacity = t if capacity is None else capacity
    ranges = np.full(2 * max(t, capacity, 1), SENTINEL, dtype=np.uint64)
    n = C.c_uint64(12345)
    rc = apd.lib().apd_interesting_ranges(ctx.handle, ptr, t, n_bins, int(k), float(perc), int(min_len), on_device,
                                          None if null_ranges else ranges.ctypes.data_as(C.POINTER(C.c_uint64)),
                                          capacity, C.byref(n))
    del keep
    return rc, int(n.value), ranges


def gpu_result(apd, ctx, frames, k, perc, min_len, form="host"):
    """The ranges as a list, or "panic" for APD_ERR_INDEX (where the reference panics, numerics.rs:132)."""
    rc, n, ranges = gpu_ranges(apd, ctx, frames, k, perc, min_len, form)
    if rc == apd.APD_ERR_INDEX:
        assert n == 0
        return "panic"
    apd.check(rc, ctx.handle)
    assert np.all(ranges[2 * n:] == SENTINEL)
    return [(int(ranges[2 * i]), int(ranges[2 * i + 1])) for i in range(n)]


def reference_result(fn, *args):
    try:
        return fn(*args)
    except IndexError:
        return "panic"


FORMS = ["host", "host+4", "device", "device+4"]


@pytest.mark.parametrize("form", FORMS)
def test_known_answer_in_integers(ctx, apd, oracle, form):
    """KAT_A (see _companion_cases.py): an off-by-one window, ties with the threshold, runs of min_len and min_len + 1, the
    initial run and the open last run, each decided by integer arithmetic; through every form of the entry point."""
    f, k, perc, min_len = cc.kat_frames(), cc.KAT_K, cc.KAT_PERC, cc.KAT_MIN_LEN
    want = cc.integer_ranges(cc.KAT_A, k, len(cc.KAT_A) // 2, min_len)[0]
    assert want == cc.KAT_RANGES
    assert oracle.interesting_ranges(f, k, perc, min_len) == want and npr.interesting_ranges(f, k, perc, min_len) == want
    assert gpu_result(apd, ctx, f, k, perc, min_len, form) == want
    # one less / one more in min_len moves exactly the runs of length min_len and min_len + 1
    assert gpu_result(apd, ctx, f, k, perc, min_len - 1, form) == sorted(want + [(39, 42)])
    assert gpu_result(apd, ctx, f, k, perc, min_len + 1, form) == [r for r in want if r != (31, 35)]


@pytest.mark.parametrize("k,n_bins", [(4, 4), (8, 2), (1, 4), (16, 6)])
def test_random_integers_against_integer_arithmetic(ctx, apd, oracle, k, n_bins):
    a = cc.random_integer_a()
    f = cc.alternating(a, n_bins)
    for perc, idx in ((0.5, 250), (0.25, 125), (0.0, 0)):
        for min_len in (0, 2, 7):
            want = cc.integer_ranges(a, k, idx, min_len)[0]
            assert oracle.interesting_ranges(f, k, perc, min_len) == want
            assert gpu_result(apd, ctx, f, k, perc, min_len, "device" if min_len == 2 else "host") == want


@pytest.mark.parametrize("form", ["host", "device+4"])
def test_capacity_smaller_than_the_count(ctx, apd, form):
    """The prefix is written, *n_ranges holds the full count, nothing past the capacity is touched; capacity 0 with a NULL
    array only counts."""
    f, k, perc, min_len = cc.kat_frames(), cc.KAT_K, cc.KAT_PERC, cc.KAT_MIN_LEN
    flat = np.array(cc.KAT_RANGES, dtype=np.uint64).ravel()
    for cap in (0, 1, 3, 4, 5):
        rc, n, ranges = gpu_ranges(apd, ctx, f, k, perc, min_len, form, capacity=cap)
        assert rc == apd.APD_OK and n == 4
        w = 2 * min(cap, 4)
        assert np.array_equal(ranges[:w], flat[:w]) and np.all(ranges[w:] == SENTINEL)
    rc, n, _ = gpu_ranges(apd, ctx, f, k, perc, min_len, form, capacity=0, null_ranges=True)
    assert rc == apd.APD_OK and n == 4
    rc, n, _ = gpu_ranges(apd, ctx, f, k, perc, min_len, form, capacity=2, null_ranges=True)
    assert rc == apd.APD_ERR_INVALID_ARG


def test_degenerate_shapes(ctx, apd, oracle):
    rng = np.random.default_rng(77)
    k = 4
    for t in (1, k, k + 1, 2 * k + 1):
        f = rng.standard_normal((t, 5)).astype(np.float32)
        for perc in (0.0, 0.5, 0.95):
            want = oracle.interesting_ranges(f, k, perc, 0)
            assert npr.interesting_ranges(f, k, perc, 0) == want
            for form in ("host", "device"):
                assert gpu_result(apd, ctx, f, k, perc, 0, form) == want
    f = rng.standard_normal((300, 7)).astype(np.float32)
    f[100:180] *= 4.0
    # t = 0 and moving_average = 0: the reference panics (percentile of an empty / all-NaN vector)
    empty = np.zeros((0, 7), np.float32)
    assert reference_result(oracle.interesting_ranges, empty, k, 0.5, 0) == "panic"
    assert reference_result(npr.interesting_ranges, empty, k, 0.5, 0) == "panic"
    assert gpu_result(apd, ctx, empty, k, 0.5, 0) == "panic" and gpu_result(apd, ctx, empty, k, 0.0, 0) == "panic"
    for perc in (0.0, 0.5):
        assert reference_result(oracle.interesting_ranges, f, 0, perc, 0) == "panic"
        assert reference_result(npr.interesting_ranges, f, 0, perc, 0) == "panic"
        assert gpu_result(apd, ctx, f, 0, perc, 0) == "panic"
    # moving_average >= t: all zeros, threshold 0, the initial run never closes
    for moving in (300, 301, 5000):
        assert oracle.interesting_ranges(f, moving, 0.5, 0) == [] and npr.interesting_ranges(f, moving, 0.5, 0) == []
        assert gpu_result(apd, ctx, f, moving, 0.5, 0) == []
    # n_bins = 1: every std is 0
    one = rng.standard_normal((300, 1)).astype(np.float32) * 50
    assert oracle.interesting_ranges(one, k, 0.5, 0) == [] and gpu_result(apd, ctx, one, k, 0.5, 0) == []
    # perc = 0: the threshold is the minimum (the k leading zeros): again nothing is below it
    assert oracle.interesting_ranges(f, k, 0.0, 0) == [] and gpu_result(apd, ctx, f, k, 0.0, 0) == []
    # perc = 1: index == len
    assert reference_result(oracle.interesting_ranges, f, k, 1.0, 0) == "panic" and gpu_result(apd, ctx, f, k, 1.0, 0) == "panic"
    # and a plain case on the same frames, so that the empty answers above are not all this input can give
    want = oracle.interesting_ranges(f, k, 0.5, 3)
    assert len(want) > 3 and gpu_result(apd, ctx, f, k, 0.5, 3) == want


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_nonfinite_frames(ctx, apd, oracle, bad):
    """A NaN or infinite bin makes its frame's std NaN (inf - inf), and that the k moving means after it.  NaN variances are
    dropped before the percentile while its index is taken from the full length (numerics.rs:126-132), and they neither open
    nor close a run."""
    rng = np.random.default_rng(78)
    k = 4
    base = rng.standard_normal((200, 6)).astype(np.float32)
    base[60:120] *= 6.0
    for where in (slice(70, 71), slice(70, 70 + k), slice(118, 121), slice(0, 200)):
        f = base.copy()
        f[where, 2] = bad
        for perc in (0.1, 0.5, 0.9):
            want = reference_result(oracle.interesting_ranges, f, k, perc, 2)
            assert reference_result(npr.interesting_ranges, f, k, perc, 2) == want
            assert (want == "panic") == (where == slice(0, 200))
            assert gpu_result(apd, ctx, f, k, perc, 2, "device" if perc == 0.5 else "host") == want, (where, perc)


@pytest.mark.parametrize("n_bins", [2, 13, 26, 40])
def test_random_sweep(ctx, apd, oracle, n_bins):
    rng = np.random.default_rng(200 + n_bins)
    f = rng.standard_normal((401, n_bins)).astype(np.float32)
    for lo, hi, g in ((30, 90, 5.0), (150, 158, 9.0), (220, 380, 3.0)):
        f[lo:hi] *= g
    nonempty = 0
    for moving in (1, 3, 15, 40):
        for perc in (0.05, 0.3, 0.5, 0.8, 0.95):
            for min_len in (0, 5, 30):
                want = oracle.interesting_ranges(f, moving, perc, min_len)
                assert gpu_result(apd, ctx, f, moving, perc, min_len) == want, (moving, perc, min_len)
                nonempty += bool(want)
    assert nonempty >= 40


def test_grid_wrap(ctx, apd, oracle):
    """One recording of 8192 * 256 + 300 frames: 8193 tiles of vat_variance_kernel, the last one partial, and 2049 steps of
    the 1024-wide vat_select_kernel and vat_scan_kernel.  Exact arithmetic: frames [a, -a], a constant over 256 frames,
    window 8."""
    a = cc.wrap_a()
    f = cc.alternating(a, 2)
    assert f.shape == (cc.GRID_WRAP_FRAMES, 2) and cc.GRID_WRAP_FRAMES > 8192 * 256 > 4096 * 256
    want = oracle.interesting_ranges(f, 8, 0.5, 100)
    assert 1000 < len(want) < 10000 and want[-1][1] > 8192 * 256
    assert npr.interesting_ranges(f, 8, 0.5, 100) == want
    assert gpu_result(apd, ctx, f, 8, 0.5, 100) == want
    del f
