#!/usr/bin/env python3
"""Spot detection on the device against the route it replaces, in one process.

64 templates of 128 frames against 16 streams of 16 384 frames, D = 13, from synth.py: 1024 pairs, 16.8 M curve entries.  Every
stream holds 32 planted occurrences of templates, half of them exact and half noisy, so that real windows exist.  One threshold for
all pairs, the 1 % quantile of all scores: about one column in a hundred is a candidate.

  host_route:  apd_spot with curves (134 MB to the host) followed by apd_spot_hits on each of the 1024 pairs -- wall time;
  per_pair:    apd_spot_detect, every pair its own group -- wall time and kernel time;
  per_stream:  apd_spot_detect, the 64 templates of a stream competing -- wall time and kernel time;
  sweep:       apd_spot, best windows only -- kernel time, the floor of the sweep alone.  The sweep WITH curves, which is what the
               detection launches, is timed inside host_route too (curves_sweep): the detection kernels are reported over both.

Before anything is timed the per-pair hits are compared bit for bit with the host route's.  Then the four run alternately,
`--repeats` times; the best of each counts.  Kernel time: the library's own events (apd_set_timing / apd_last_kernel_ms).  Wall time:
a host clock around the blocking calls, buffers allocated beforehand, straight through the C ABI on one joined batch.  Prints ONE
JSON line: the threshold, the candidates and hits it produced, every time in milliseconds, the detection kernels over the sweep
floor, and the model next to them (the marking pass reads 8 bytes per entry once; picking costs, per group, hits x ceil(candidates /
1024) passes of the workgroup, and the slowest group is the critical path).

    python tools/spot_detect_bench.py [--repeats 5]
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()

    import numpy as np

    from audio_pattern_discovery_amd import _lib, synth
    from audio_pattern_discovery_amd.alignments import SPOT_BEST, SPOT_HIT, Batch

    n_templates, template_len, n_streams, stream_len, planted = 64, 128, 16, 16384, 32
    frames, offsets = synth.make_sequences(n_templates, template_len, DIM, seed=0xD7EC, copies=0.0, jitter=0)
    templates = synth.split(frames, offsets)
    frames, offsets = synth.make_sequences(n_streams, stream_len, DIM, seed=0xD7ED, copies=0.0, jitter=0)
    streams = [s.copy() for s in synth.split(frames, offsets)]
    rng = np.random.default_rng(0xD7EE)
    slot = stream_len // planted
    for r, y in enumerate(streams):
        for k in range(planted):
            at = k * slot + int(rng.integers(0, slot - template_len))
            t = templates[(r * planted + k) % n_templates]
            y[at:at + template_len] = t if k % 2 == 0 else t + 0.25 * rng.standard_normal(t.shape).astype(np.float32)

    def resident(seqs):
        off = np.zeros(len(seqs) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(s) for s in seqs])
        return Batch(ctx, np.ascontiguousarray(np.concatenate(seqs, axis=0), dtype=np.float32), off, DIM)

    ctx = _lib.Context(0)
    ctx.set_timing(True)
    L = _lib.lib()
    bt, bs = resident(templates), resident(streams)
    joined = Batch.join(bt, bs)
    cfg = _lib.AlignConfig(1.0, 1.0, 1.0, 1.0)
    pairs = np.array([(t, n_templates + r) for t in range(n_templates) for r in range(n_streams)], dtype=np.uint32)
    n_pairs = len(pairs)
    entries = n_pairs * stream_len
    u32p, u64p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_float)
    head = (ctx.handle, joined.handle, C.byref(cfg), pairs.ctypes.data_as(u32p), n_pairs)
    cost, start = np.zeros(entries, dtype=np.float32), np.zeros(entries, dtype=np.uint32)
    curve_off = np.zeros(n_pairs + 1, dtype=np.uint64)
    best = np.zeros(n_pairs, dtype=SPOT_BEST)
    host_hits = np.zeros((n_pairs, stream_len // 8), dtype=SPOT_BEST)             # far more than a pair can hold at a 1 % threshold
    host_count = np.zeros(n_pairs, dtype=np.uint64)
    hits = np.zeros(n_pairs * stream_len // 8, dtype=SPOT_HIT)
    hit_off = np.zeros(n_pairs + 1, dtype=np.uint64)
    n_groups, n_hits = C.c_uint64(0), C.c_uint64(0)

    def host_route(threshold):
        t0 = time.perf_counter()
        _lib.check(L.apd_spot(*head, cost.ctypes.data_as(f32p), start.ctypes.data_as(u32p), entries, curve_off.ctypes.data_as(u64p),
                              best.ctypes.data_as(C.POINTER(_lib.SpotBest))), ctx.handle)
        sweep_ms = ctx.last_kernel_ms()
        count = C.c_uint64(0)
        for p in range(n_pairs):
            a = p * stream_len
            _lib.check(L.apd_spot_hits(cost[a:a + stream_len].ctypes.data_as(f32p), start[a:a + stream_len].ctypes.data_as(u32p), stream_len,
                                       template_len, threshold, host_hits[p].ctypes.data_as(C.POINTER(_lib.SpotBest)), host_hits.shape[1],
                                       C.byref(count)))
            host_count[p] = count.value
        return (time.perf_counter() - t0) * 1e3, sweep_ms

    def detect(threshold, per_stream):
        thr = np.full(n_pairs, threshold, dtype=np.float32)
        t0 = time.perf_counter()
        _lib.check(L.apd_spot_detect(*head, thr.ctypes.data_as(f32p), int(per_stream), hits.ctypes.data_as(C.POINTER(_lib.SpotHit)), len(hits),
                                     hit_off.ctypes.data_as(u64p), C.byref(n_groups), C.byref(n_hits)), ctx.handle)
        return (time.perf_counter() - t0) * 1e3, ctx.last_kernel_ms()

    def sweep():
        _lib.check(L.apd_spot(*head, None, None, 0, curve_off.ctypes.data_as(u64p), best.ctypes.data_as(C.POINTER(_lib.SpotBest))), ctx.handle)
        return ctx.last_kernel_ms()

    # the threshold, from the curves themselves; then the comparison that comes before any timing
    host_route(0.0)
    window = np.tile(np.arange(1, stream_len + 1, dtype=np.int64), n_pairs) - start + 1
    with np.errstate(all="ignore"):
        scores = cost / (template_len + window).astype(np.float32)
    threshold = float(np.partition(scores[np.isfinite(scores)], entries // 100)[entries // 100])
    with np.errstate(invalid="ignore"):
        candidates = int(np.count_nonzero(scores < np.float32(threshold)))
    per_pair_candidates = np.count_nonzero((scores < np.float32(threshold)).reshape(n_pairs, stream_len), axis=1)
    del scores, window
    host_route(threshold)
    assert int(host_count.max()) <= host_hits.shape[1]
    detect(threshold, False)
    assert n_groups.value == n_pairs and n_hits.value == int(host_count.sum()) <= len(hits), (n_hits.value, int(host_count.sum()))
    for p in range(n_pairs):
        mine, want = hits[int(hit_off[p]):int(hit_off[p + 1])], host_hits[p, :int(host_count[p])]
        assert len(mine) == len(want) and np.all(mine["pair"] == p) and np.array_equal(mine["rank"], np.arange(len(mine)))
        for f in ("end", "start", "cost", "score"):
            assert np.array_equal(mine[f].view(np.uint32), want[f].view(np.uint32)), (p, f)
    pair_hits = np.diff(hit_off[:n_pairs + 1]).astype(np.int64)
    detect(threshold, True)
    assert n_groups.value == n_streams
    stream_hits = np.diff(hit_off[:n_streams + 1]).astype(np.int64)
    stream_candidates = per_pair_candidates.reshape(n_templates, n_streams).sum(axis=0)

    def passes(h, c):
        return ((h + 1) * -(-c // 1024)).astype(np.int64)                        # hits + 1 rounds, each ceil(candidates / 1024) passes

    runs = dict(host_route=[], curves_sweep_kernel=[], per_pair_wall=[], per_pair_kernel=[], per_stream_wall=[], per_stream_kernel=[], sweep_kernel=[])
    for _ in range(args.repeats):
        wall, kernel = host_route(threshold)
        runs["host_route"].append(wall)
        runs["curves_sweep_kernel"].append(kernel)
        wall, kernel = detect(threshold, False)
        runs["per_pair_wall"].append(wall)
        runs["per_pair_kernel"].append(kernel)
        wall, kernel = detect(threshold, True)
        runs["per_stream_wall"].append(wall)
        runs["per_stream_kernel"].append(kernel)
        runs["sweep_kernel"].append(sweep())
    joined.close()
    bt.close()
    bs.close()
    ctx.close()
    floor, with_curves = min(runs["sweep_kernel"]), min(runs["curves_sweep_kernel"])
    out = dict(pairs=n_pairs, entries=entries, planted_per_stream=planted, threshold=threshold, candidates=candidates,
               per_pair_hits=int(pair_hits.sum()), per_stream_hits=int(stream_hits.sum()), verified_bitwise_against_host_route=True,
               host_route_copy_bytes=8 * entries, ms=runs,
               host_route_wall_ms=min(runs["host_route"]), host_route_spread_ms=max(runs["host_route"]) - min(runs["host_route"]),
               per_pair_wall_ms=min(runs["per_pair_wall"]), per_stream_wall_ms=min(runs["per_stream_wall"]),
               per_pair_detection_over_sweep_ms=min(runs["per_pair_kernel"]) - floor,
               per_stream_detection_over_sweep_ms=min(runs["per_stream_kernel"]) - floor, sweep_floor_ms=floor,
               per_pair_detection_over_curves_sweep_ms=min(runs["per_pair_kernel"]) - with_curves,
               per_stream_detection_over_curves_sweep_ms=min(runs["per_stream_kernel"]) - with_curves, curves_sweep_ms=with_curves,
               model=dict(mark_bytes=8 * entries,
                          per_pair_passes_slowest_group=int(passes(pair_hits, per_pair_candidates).max()),
                          per_pair_passes_all_groups=int(passes(pair_hits, per_pair_candidates).sum()),
                          per_stream_passes_slowest_group=int(passes(stream_hits, stream_candidates).max()),
                          per_stream_passes_all_groups=int(passes(stream_hits, stream_candidates).sum())))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
