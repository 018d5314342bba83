#!/usr/bin/env python3
"""What a kept history costs a streaming session, and what tracing from it costs.

  tools/spot_stream_bench.py's workload: 64 templates of 128 frames against 16 channels of 16 384 frames, D = 13, curves on, fed
  in chunks of 1024 columns packed on the device beforehand and pushed back to back through the C ABI.

  off:    the session without a history (the kernels of the kind SpotStreamSweep);
  on:     the same session after apd_spot_stream_keep(H) (the kind SpotStreamRecordSweep and the frame-ring copy); its curves and bests are
          compared with `off`'s, bit for bit;
  trace:  after the last push of `on`, apd_spot_stream_paths for one window per pair -- the best-scoring end of the last chunk whose
          start is still kept -- beside apd_spot (curves, (a)) and apd_spot_paths ((b)) for the same 1024 windows on the joined
          batch; the steps of the two are compared bit for bit before anything is printed.

Library events (apd_set_timing / apd_last_kernel_ms; a session's figure is the sum over its pushes), `--repeats` runs after one
warm-up run; every repeat is printed, the best counts.  `--modes off` uses nothing this tool's library must have beyond the streaming
session itself, so the same script times an older build through APD_LIB.  Prints ONE JSON line.

    python tools/spot_stream_path_bench.py [--repeats 5] [--history 4096] [--modes off,on,trace] [--small]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DIM, CHUNK = 13, 1024


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--history", type=int, default=4096)
    ap.add_argument("--modes", default="off,on,trace")
    ap.add_argument("--small", action="store_true", help="channels of 4096 frames and H = 2048 (a quick look, not the recorded figure)")
    args = ap.parse_args()
    modes = args.modes.split(",")

    import numpy as np

    from audio_pattern_discovery_amd import _lib
    from audio_pattern_discovery_amd.alignments import SPOT_WINDOW, AlignmentWorkers, NDSequence
    from audio_pattern_discovery_amd.discovery import Discovery

    n_templates, template_len, n_streams, stream_len = 64, 128, 16, (4096 if args.small else 16384)
    history = min(args.history, stream_len // 2)
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
    n_pairs = n_templates * n_streams
    out = dict(pairs=n_pairs, cells=n_pairs * template_len * stream_len, chunk=CHUNK, history=history)

    session = wt.spot_stream(list(range(n_templates)), Discovery(), channels=n_streams)
    L = _lib.lib()
    u32p, u64p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_float)
    pushes = stream_len // CHUNK
    chunk_off = np.arange(n_streams + 1, dtype=np.uint64) * CHUNK
    device = [ctx.upload(np.ascontiguousarray(np.concatenate([s.frames[k * CHUNK:(k + 1) * CHUNK] for s in streams], axis=0))) for k in range(pushes)]
    curve_off = np.zeros(n_pairs + 1, dtype=np.uint64)
    results = {}
    for mode in ("off", "on"):
        if mode not in modes and not (mode == "on" and "trace" in modes):
            continue
        if mode == "on":
            session.keep(history)
        cost = np.zeros((pushes, n_pairs, CHUNK), dtype=np.float32)
        start = np.zeros((pushes, n_pairs, CHUNK), dtype=np.uint32)
        best = np.zeros(n_pairs, dtype=np.dtype([("end", np.uint32), ("start", np.uint32), ("cost", np.float32), ("score", np.float32)]))
        kernel_ms = []
        for rep in range(args.repeats + 1):                                    # the first repeat is the warm-up
            session.reset()
            k_ms = 0.0
            for k in range(pushes):
                _lib.check(L.apd_spot_stream_push(ctx.handle, session.handle, C.c_void_p(device[k].ptr), chunk_off.ctypes.data_as(u64p), DIM, 1,
                                                  cost[k].ctypes.data_as(f32p), start[k].ctypes.data_as(u32p), n_pairs * CHUNK,
                                                  curve_off.ctypes.data_as(u64p), best.ctypes.data_as(C.POINTER(_lib.SpotBest))), ctx.handle)
                k_ms += ctx.last_kernel_ms()
            if rep:
                kernel_ms.append(k_ms)
        results[mode] = (cost, start, best)
        out[mode] = dict(pushes=pushes, kernel_ms=kernel_ms)
    if "off" in results and "on" in results:
        for a, b in zip(results["off"], results["on"]):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "a history changed the curves or the bests"
        out["on_over_off"] = min(out["on"]["kernel_ms"]) / min(out["off"]["kernel_ms"])

    if "trace" in modes:
        cost, start, _ = results["on"]
        first, last = session.history(0)
        assert (first, last) == (stream_len - history + 1, stream_len)
        with np.errstate(all="ignore"):
            ends = np.arange(last - CHUNK + 1, last + 1, dtype=np.int64)[None, :]
            score = cost[-1] / (template_len + ends - start[-1] + 1).astype(np.float32)
        score[start[-1] < first] = np.inf
        pick = np.argmin(score, axis=1)
        windows = np.zeros(n_pairs, dtype=SPOT_WINDOW)
        for p in range(n_pairs):
            windows[p] = (p % n_templates, p // n_templates, last - CHUNK + 1 + pick[p], start[-1][p, pick[p]])
        trace_ms = []
        for _ in range(args.repeats + 1):
            paths, found, scores = session.paths(windows)
            trace_ms.append(ctx.last_kernel_ms())
        assert all(len(p) > 0 for p in paths) and np.array_equal(found, windows["start"])
        pairs = [(int(w["x"]), n_templates + int(w["y"])) for w in windows]
        spot_ms, paths_ms = [], []
        for _ in range(args.repeats + 1):
            wt.spot(pairs, Discovery(), curves=True, streams=ws)
            spot_ms.append(ctx.last_kernel_ms())
            whole, w_found, w_scores = wt.spot_paths(pairs, windows, Discovery(), streams=ws)
            paths_ms.append(ctx.last_kernel_ms())
        assert np.array_equal(found, w_found) and np.array_equal(scores.view(np.uint32), w_scores.view(np.uint32))
        for a, b in zip(paths, whole):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "the session's steps differ from apd_spot_paths'"
        out["trace"] = dict(windows=n_pairs, steps=int(sum(len(p) for p in paths)), stream_paths_ms=trace_ms[1:], spot_ms=spot_ms[1:],
                            spot_paths_ms=paths_ms[1:], b_minus_a=min(paths_ms[1:]) - min(spot_ms[1:]))
    for buf in device:
        buf.free()
    session.close()
    wt.close()
    ws.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
