"""The ctypes calls shared by tests/test_gpu_vat_batch.py and tests/test_gpu_vat_batch_edges.py: apd_interesting_ranges_batch,
apd_interesting_ranges and apd_slice_samples with sentinels around everything the library may write.  No assertion of a test lives
here but the ones every caller wants (range_off ascends, nothing is written past the reported ranges)."""
import ctypes as C

import numpy as np

SENTINEL = np.uint64(0xDEADBEEFDEADBEEF)
U64P = C.POINTER(C.c_uint64)


def batch_call(apd, ctx, recs, k, perc, min_len, form="host", capacity=None, with_status=True, null_ranges=False):
    """apd_interesting_ranges_batch on the recordings packed back to back -> (rc, range_off, the whole ranges array as passed, status).
    form: "host", "device", "device+4" (frames one float past a 16-byte boundary)."""
    n_bins = recs[0].shape[1]
    lens = [r.shape[0] for r in recs]
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    flat = np.ascontiguousarray(np.concatenate([np.asarray(r, np.float32).reshape(-1, n_bins) for r in recs]), dtype=np.float32)
    keep = None
    if form == "host":
        ptr, on_device = C.c_void_p(flat.ctypes.data if flat.size else None), 0
    else:
        off = 4 if form.endswith("+4") else 0
        keep = ctx.alloc(flat.nbytes + 16)
        keep.copy_from(flat.ravel(), byte_offset=off)
        assert keep.ptr % 16 == 0
        ptr, on_device = keep.at(off), 1
    bound = sum(lens) // 2 + 1
    capacity = bound if capacity is None else capacity
    ranges = np.full(2 * max(bound, capacity, 1), SENTINEL, dtype=np.uint64)
    range_off = np.full(len(recs) + 1, SENTINEL, dtype=np.uint64)
    status = np.full(len(recs), 12345, dtype=np.int32)
    rc = apd.lib().apd_interesting_ranges_batch(ctx.handle, ptr, offsets.ctypes.data_as(U64P), len(recs), n_bins, int(k), float(perc), int(min_len),
                                                on_device, range_off.ctypes.data_as(U64P), None if null_ranges else ranges.ctypes.data_as(U64P),
                                                capacity, status.ctypes.data_as(C.POINTER(C.c_int32)) if with_status else None)
    del keep
    return rc, range_off, ranges, status


def batch_result(apd, ctx, recs, k, perc, min_len, form="host"):
    """Per recording: the list of ranges, or "panic" for APD_ERR_INDEX in its status."""
    rc, range_off, ranges, status = batch_call(apd, ctx, recs, k, perc, min_len, form)
    apd.check(rc, ctx.handle)
    assert range_off[0] == 0 and np.all(np.diff(range_off.astype(np.int64)) >= 0)
    assert np.all(ranges[2 * int(range_off[-1]):] == SENTINEL)
    out = []
    for s in range(len(recs)):
        lo, hi = int(range_off[s]), int(range_off[s + 1])
        assert status[s] in (apd.APD_OK, apd.APD_ERR_INDEX)
        if status[s] == apd.APD_ERR_INDEX:
            assert lo == hi
            out.append("panic")
        else:
            out.append([(int(ranges[2 * r]), int(ranges[2 * r + 1])) for r in range(lo, hi)])
    return out


def single_result(apd, ctx, frames, k, perc, min_len):
    """apd_interesting_ranges on one recording (host form)."""
    f = np.ascontiguousarray(frames, dtype=np.float32)
    t, n_bins = f.shape
    ranges = np.zeros(2 * max(t, 1), dtype=np.uint64)
    n = C.c_uint64(0)
    rc = apd.lib().apd_interesting_ranges(ctx.handle, C.c_void_p(f.ctypes.data if t else None), t, n_bins, int(k), float(perc), int(min_len), 0,
                                          ranges.ctypes.data_as(U64P), t, C.byref(n))
    if rc == apd.APD_ERR_INDEX:
        return "panic"
    apd.check(rc, ctx.handle)
    return [(int(ranges[2 * i]), int(ranges[2 * i + 1])) for i in range(n.value)]


def ramps(lengths):
    """int16 recordings whose every sample encodes its recording and its position."""
    return [((np.arange(n, dtype=np.int64) * 31 + 7919 * (s + 1)) % 65536).astype(np.uint16).view(np.int16) for s, n in enumerate(lengths)]


def gather(apd, ctx, recs, ranges, fft_step, form):
    """apd_slice_samples -> (rc, the whole output array as passed, total).  form: "host", "device", "device+2" (output two bytes past a
    16-byte boundary, input one sample past one)."""
    from audio_pattern_discovery_amd.alignments import _flat_ranges, slice_offsets
    sample_off = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.uint64)
    samples = np.concatenate(recs).astype(np.int16) if recs else np.zeros(0, np.int16)
    range_off, flat = _flat_ranges(ranges)
    total = int(slice_offsets(sample_off, ranges, fft_step)[0][-1])
    L = apd.lib()
    args = (sample_off.ctypes.data_as(U64P), len(recs), range_off.ctypes.data_as(U64P), flat.ctypes.data_as(U64P) if flat.size else None, fft_step)
    if form == "host":
        out = np.full(total + 9, 0x5A5A, np.int16)
        rc = L.apd_slice_samples(ctx.handle, C.c_void_p(samples.ctypes.data), *args, 0, C.c_void_p(out.ctypes.data), total)
        return rc, out, total
    shift = 2 if form.endswith("+2") else 0
    d_in, d_out = ctx.alloc(samples.nbytes + 16), ctx.alloc(2 * total + 64)
    d_in.copy_from(samples, byte_offset=shift)
    d_out.fill(0x5A)
    rc = L.apd_slice_samples(ctx.handle, d_in.at(shift), *args, 1, d_out.at(shift), total)
    return rc, d_out.to_numpy(np.int16, total + 9, byte_offset=shift), total


def gather_shifted(apd, ctx, recs, ranges, fft_step, out_shift, in_shift):
    """apd_slice_samples, device form, the output `out_shift` bytes and the samples `in_shift` bytes past a 16-byte boundary (both
    even) -> (rc, the WHOLE output buffer from that boundary on as int16, total): [out_shift / 2, out_shift / 2 + total) is what the
    call may write, the rest is 0x5A5A."""
    from audio_pattern_discovery_amd.alignments import _flat_ranges, slice_offsets
    assert out_shift % 2 == 0 and in_shift % 2 == 0 and 0 <= out_shift < 16 and 0 <= in_shift < 16
    sample_off = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.uint64)
    samples = np.concatenate(recs).astype(np.int16)
    range_off, flat = _flat_ranges(ranges)
    total = int(slice_offsets(sample_off, ranges, fft_step)[0][-1])
    d_in, d_out = ctx.alloc(samples.nbytes + 16), ctx.alloc(2 * total + 64)
    assert d_in.ptr % 16 == 0 and d_out.ptr % 16 == 0
    d_in.copy_from(samples, byte_offset=in_shift)
    d_out.fill(0x5A)
    rc = apd.lib().apd_slice_samples(ctx.handle, d_in.at(in_shift), sample_off.ctypes.data_as(U64P), len(recs), range_off.ctypes.data_as(U64P),
                                     flat.ctypes.data_as(U64P) if flat.size else None, fft_step, 1, d_out.at(out_shift), total)
    return rc, d_out.to_numpy(np.int16, total + 32), total
