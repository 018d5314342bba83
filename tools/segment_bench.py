#!/usr/bin/env python3
"""Stage 1 on a whole corpus: the VAT ranges of every recording and the gather of the audio they name, on
frames and samples that are already resident, D = 13, vat_moving = 15, vat_percentile = 0.95, vat_min_len = 150, dft_step = 128.
Two corpora: many short recordings (4096 x 1024 frames) and few long ones (16 x 2^20 frames).  Two routes, taking turns in one
process, wall clock around the blocking calls, best of --repeats with the spread:
  (a) the single call per recording: apd_interesting_ranges(on_device=1), a batch of one each time, the slices cut on the host and
      uploaded;
  (b) apd_interesting_ranges_batch + apd_slice_samples(on_device=1).
Both must give the same ranges and the same slices before anything is timed.

The frames are noise with planted bursts of IDENTICAL loud frames: at the 95th percentile only ties let a run exceed 150 frames
(5 % of 1024 frames are 51), and the moving mean of 15 equal stds is the same number wherever the window lies inside a burst.
usage: python tools/segment_bench.py [--repeats R] [--corpus short,long] [--scale S]      one JSON line per corpus; --scale divides
the number of recordings (short) or their length (long), for a quick look."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D, MOVING, PERC, MIN_LEN, STEP, FFT = 13, 15, 0.95, 150, 128, 256
U64P = C.POINTER(C.c_uint64)


def recording(rng, noise, t, s):
    """Noise with a burst of 250 identical loud frames in every stretch of 2048 frames (12 % of the frames: the threshold is the
    bursts' common variance), placed differently in every recording."""
    f = noise[:t].copy()
    loud = (rng.standard_normal(D) * 40.0).astype(np.float32)
    for lo in range((97 * s) % 512 + 64, t - 260, 2048):
        f[lo:lo + 250] = loud
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--corpus", default="short,long")
    ap.add_argument("--scale", type=int, default=1)
    args = ap.parse_args()
    from audio_pattern_discovery_amd import _lib
    L = _lib.lib()
    ctx = _lib.Context(0)
    shapes = {"short": (4096 // args.scale, 1024), "long": (16, (1 << 20) // args.scale)}
    for name in args.corpus.split(","):
        n, t = shapes[name]
        rng = np.random.default_rng(len(name))
        noise = rng.standard_normal((t, D)).astype(np.float32)
        frame_off = (np.arange(n + 1, dtype=np.uint64) * np.uint64(t))
        per_rec = t * STEP + FFT                                    # samples of a recording with t frames
        sample_off = (np.arange(n + 1, dtype=np.uint64) * np.uint64(per_rec))
        d_frames = ctx.alloc(n * t * D * 4)
        for s in range(n):
            d_frames.copy_from(recording(rng, noise, t, s), byte_offset=s * t * D * 4)
        block = (np.arange(1 << 20, dtype=np.int64) * 7919 % 65521 - 32760).astype(np.int16)
        samples = np.resize(block, n * per_rec)
        d_samples = ctx.upload(samples)

        cap = n * (t // (MIN_LEN + 2) + 1)
        ranges_a, ranges_b = np.zeros(2 * cap, np.uint64), np.zeros(2 * cap, np.uint64)
        off_a, off_b = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)
        state = {}

        def route_a(d_out):
            count = C.c_uint64(0)
            total = 0
            for s in range(n):
                _lib.check(L.apd_interesting_ranges(ctx.handle, d_frames.at(s * t * D * 4), t, D, MOVING, PERC, MIN_LEN, 1,
                                                    ranges_a[2 * total:].ctypes.data_as(U64P), cap - total, C.byref(count)), ctx.handle)
                total += count.value
                off_a[s + 1] = total
            pieces = [samples[int(sample_off[s]) + int(ranges_a[2 * r]) * STEP:int(sample_off[s]) + int(ranges_a[2 * r + 1]) * STEP]
                      for s in range(n) for r in range(int(off_a[s]), int(off_a[s + 1]))]
            packed = np.concatenate(pieces) if pieces else np.zeros(0, np.int16)
            if d_out is not None and packed.size:
                d_out.copy_from(packed)
            state["packed"] = packed

        def route_b(d_out):
            t0 = time.perf_counter()
            _lib.check(L.apd_interesting_ranges_batch(ctx.handle, d_frames.at(), frame_off.ctypes.data_as(U64P), n, D, MOVING, PERC, MIN_LEN, 1,
                                                      off_b.ctypes.data_as(U64P), ranges_b.ctypes.data_as(U64P), cap, None), ctx.handle)
            state["ranges_ms"] = (time.perf_counter() - t0) * 1e3
            if d_out is not None:
                _lib.check(L.apd_slice_samples(ctx.handle, d_samples.at(), sample_off.ctypes.data_as(U64P), n, off_b.ctypes.data_as(U64P),
                                               ranges_b.ctypes.data_as(U64P), STEP, 1, d_out.at(), d_out.nbytes // 2), ctx.handle)

        # both routes agree, before anything is timed (this also loads the code objects)
        route_a(None)
        route_b(None)
        total = int(off_a[-1])
        assert total > 0 and np.array_equal(off_a, off_b) and np.array_equal(ranges_a[:2 * total], ranges_b[:2 * total]), "the routes disagree"
        n_out = int(state["packed"].size)
        d_out_a, d_out_b = ctx.alloc(max(2 * n_out, 16)), ctx.alloc(max(2 * n_out, 16))
        route_a(d_out_a)
        route_b(d_out_b)
        assert np.array_equal(d_out_a.to_numpy(np.int16, n_out), d_out_b.to_numpy(np.int16, n_out)), "the slices disagree"

        ms = {"a": [], "b": [], "b_ranges": []}
        for _ in range(args.repeats):
            for key, route, out in (("a", route_a, d_out_a), ("b", route_b, d_out_b)):
                t0 = time.perf_counter()
                route(out)
                ms[key].append((time.perf_counter() - t0) * 1e3)
            ms["b_ranges"].append(state["ranges_ms"])
        print(json.dumps({"corpus": name, "recordings": n, "frames_each": t, "ranges": total, "slice_samples": n_out,
                          "a_per_recording_ms_best": round(min(ms["a"]), 3), "a_per_recording_ms_worst": round(max(ms["a"]), 3),
                          "b_batch_ms_best": round(min(ms["b"]), 3), "b_batch_ms_worst": round(max(ms["b"]), 3),
                          "b_ranges_only_ms_best": round(min(ms["b_ranges"]), 3),
                          "ratio_a_over_b": round(min(ms["a"]) / min(ms["b"]), 2)}), flush=True)
        for buf in (d_frames, d_samples, d_out_a, d_out_b):
            buf.free()
        del samples
    ctx.close()


if __name__ == "__main__":
    main()
