#!/usr/bin/env python3
"""Streaming spotting against apd_spot on the same pairs, in one process.

  64 templates of 128 frames against 16 streams of 16 384 frames, D = 13, curves on: 1024 pairs of 128 x 16 384 cells each --
  apd_spot's documented shape at sixteen streams.

  spot:     apd_spot on the joined batch, curves on;
  one push: a session of 64 queries x 16 channels fed every stream in one push of 16 384 columns;
  1024:     the same session fed in chunks of 1024 columns (16 pushes);
  128:      ... in chunks of 128 columns (128 pushes).

All are timed with the library's own events (apd_set_timing / apd_last_kernel_ms; a session's figure is the sum over its pushes:
the repack of each chunk and its sweep), the best of `--repeats` runs after one warm-up run counts.  The chunks are packed on the
device beforehand (frames_on_device), as apd_spot's frames are resident, and pushed back to back: host copies and bookkeeping between
pushes of a few hundred microseconds each would be part of what the events see.  The wall time of the pushes (kernels, copy-out of the curves, one
synchronisation each) is reported beside it.  The session's concatenated curves and final best are compared with apd_spot's, bit
for bit, before anything is printed.  `model` is the macro-step count of the chunking relative to apd_spot's: every chunk of m
columns costs m + lane_n macro-steps, rounded up to even (lane_n = 63 for these queries).  Prints ONE JSON line.

    python tools/spot_stream_bench.py [--repeats 3] [--small]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DIM = 13


def macro_steps(m, lane_n):
    return (m + lane_n + 1) // 2 * 2


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="streams of 2048 frames (a quick look, not the recorded figure)")
    args = ap.parse_args()

    import numpy as np

    from audio_pattern_discovery_amd import _lib
    from audio_pattern_discovery_amd.alignments import AlignmentWorkers, NDSequence
    from audio_pattern_discovery_amd.discovery import Discovery

    n_templates, template_len, n_streams, stream_len = 64, 128, 16, (2048 if args.small else 16384)
    ctx = _lib.Context(0)
    ctx.set_timing(True)
    rng = np.random.default_rng(0x5B07)
    templates = [NDSequence(rng.standard_normal((template_len, DIM)).astype(np.float32)) for _ in range(n_templates)]
    streams = []
    for r in range(n_streams):
        y = rng.standard_normal((stream_len, DIM)).astype(np.float32)
        at = int(rng.integers(0, stream_len - template_len))
        y[at:at + template_len] = templates[r % n_templates].frames           # one exact occurrence of one template per stream
        streams.append(NDSequence(y))
    wt, ws = AlignmentWorkers.new(templates, ctx), AlignmentWorkers.new(streams, ctx)
    # the session's pair order: p = channel * n_templates + q
    pairs = [(t, n_templates + r) for r in range(n_streams) for t in range(n_templates)]
    cells = len(pairs) * template_len * stream_len
    out = dict(pairs=len(pairs), cells=cells)

    spot_ms = []
    for _ in range(args.repeats):
        curves, best = wt.spot(pairs, Discovery(), curves=True, streams=ws)
        spot_ms.append(ctx.last_kernel_ms())
    want_cost = np.stack([c for c, _ in curves]).view(np.uint32)
    want_start = np.stack([s for _, s in curves])
    del curves
    out["spot"] = dict(kernel_ms=spot_ms)

    lane_n = (template_len - 1) // ((template_len + 63) // 64)
    whole = macro_steps(stream_len, lane_n)
    session = wt.spot_stream(list(range(n_templates)), Discovery(), channels=n_streams)
    # The pushes go through the C ABI with every chunk already packed on the device and the outputs preallocated, so that -- as for
    # apd_spot, whose frames are resident -- no host copy and no Python bookkeeping leaves the GPU idle ahead of a timed kernel.
    L = _lib.lib()
    u32p, u64p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_float)
    n_pairs = len(pairs)
    for name, m in (("one_push", stream_len), ("chunks_1024", 1024), ("chunks_128", 128)):
        m = min(m, stream_len)
        pushes = stream_len // m
        chunk_off = np.arange(n_streams + 1, dtype=np.uint64) * m
        device = [ctx.upload(np.ascontiguousarray(np.concatenate([s.frames[k * m:(k + 1) * m] for s in streams], axis=0))) for k in range(pushes)]
        cost = np.zeros((pushes, n_pairs, m), dtype=np.float32)
        start = np.zeros((pushes, n_pairs, m), dtype=np.uint32)
        curve_off = np.zeros(n_pairs + 1, dtype=np.uint64)
        got_best = np.zeros(n_pairs, dtype=best.dtype)
        kernel_ms, wall_ms = [], []
        for rep in range(args.repeats + 1):                                    # the first repeat is the warm-up
            session.reset()
            k_ms = 0.0
            t0 = time.perf_counter()
            for k in range(pushes):
                _lib.check(L.apd_spot_stream_push(ctx.handle, session.handle, C.c_void_p(device[k].ptr), chunk_off.ctypes.data_as(u64p), DIM, 1,
                                                  cost[k].ctypes.data_as(f32p), start[k].ctypes.data_as(u32p), n_pairs * m,
                                                  curve_off.ctypes.data_as(u64p), got_best.ctypes.data_as(C.POINTER(_lib.SpotBest))), ctx.handle)
                k_ms += ctx.last_kernel_ms()
            if rep:
                wall_ms.append((time.perf_counter() - t0) * 1e3)
                kernel_ms.append(k_ms)
        assert np.array_equal(np.concatenate(list(cost), axis=1).view(np.uint32), want_cost), "%s: cost bits differ from apd_spot" % name
        assert np.array_equal(np.concatenate(list(start), axis=1), want_start), "%s: starts differ from apd_spot" % name
        assert np.array_equal(got_best.view(np.uint32), best.view(np.uint32)), "%s: best differs from apd_spot" % name
        for buf in device:
            buf.free()
        out[name] = dict(pushes=pushes, kernel_ms=kernel_ms, wall_ms=wall_ms, ratio_to_spot=min(kernel_ms) / min(spot_ms),
                         model=pushes * macro_steps(m, lane_n) / whole)
    session.close()
    wt.close()
    ws.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
