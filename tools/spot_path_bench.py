#!/usr/bin/env python3
"""Warping paths of spotted windows against the spotting sweep itself, in one process.

64 templates of 128 frames against 16 streams of 16 384 frames, D = 13 (tools/spot_bench.py --small's shapes): 1024 pairs.

  spot:        apd_spot with curves on the 1024 pairs;
  paths_best:  apd_spot_paths with one window per pair, the best window;
  paths_eight: apd_spot_paths with eight windows per pair, the curve's start at the ends k m / 8 (a start of 0 skipped).

All timed with the library's own events (apd_set_timing / apd_last_kernel_ms); the best of `--repeats` runs counts.  Prints ONE JSON
line: milliseconds of each, best_over_spot = paths_best / spot (a sweep plus stores and a short trace) and eight_over_best =
paths_eight / paths_best (a pair is swept once however many windows it has: near 1, not near 8).

    python tools/spot_path_bench.py [--repeats 3]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DIM = 13


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()

    import numpy as np

    from audio_pattern_discovery_amd import _lib
    from audio_pattern_discovery_amd.alignments import SPOT_BEST, AlignmentWorkers, NDSequence
    from audio_pattern_discovery_amd.discovery import Discovery

    n_templates, template_len, n_streams, stream_len = 64, 128, 16, 16384
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
    pairs = [(t, n_templates + r) for t in range(n_templates) for r in range(n_streams)]
    params = Discovery()

    spot_ms = []
    for _ in range(args.repeats):
        curves, best = wt.spot(pairs, params, streams=ws)
        spot_ms.append(ctx.last_kernel_ms())

    def timed(asked_pairs, asked):
        ms, steps = [], 0
        for _ in range(args.repeats):
            paths, found, _ = wt.spot_paths(asked_pairs, asked, params, streams=ws)
            ms.append(ctx.last_kernel_ms())
            assert np.array_equal(found, asked["start"]) and all(len(p) > template_len for p in paths)
            steps = sum(len(p) for p in paths)
        return ms, steps

    best_ms, best_steps = timed(pairs, best)
    eight_pairs, eight = [], []
    for pair, (cost, start) in zip(pairs, curves):
        for k in range(1, 9):
            end = k * stream_len // 8
            if start[end - 1]:
                eight_pairs.append(pair)
                eight.append((end, start[end - 1], cost[end - 1], 0.0))
    eight_ms, eight_steps = timed(eight_pairs, np.array(eight, dtype=SPOT_BEST))
    wt.close()
    ws.close()
    ctx.close()
    out = dict(pairs=len(pairs), cells=len(pairs) * template_len * stream_len,
               spot=dict(kernel_ms=spot_ms),
               paths_best=dict(windows=len(pairs), steps=best_steps, kernel_ms=best_ms),
               paths_eight=dict(windows=len(eight), steps=eight_steps, kernel_ms=eight_ms),
               best_over_spot=min(best_ms) / min(spot_ms), eight_over_best=min(eight_ms) / min(best_ms))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
