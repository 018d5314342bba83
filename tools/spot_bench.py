#!/usr/bin/env python3
"""Subsequence alignment against the strict-mode band kernels, per DP cell, in one process.

  spot:    64 templates of 128 frames against 256 streams of 16 384 frames, D = 13: 16 384 pairs of 128 x 16 384 cells each, best
           windows only (apd_spot without curve buffers);
  strict:  apd_align_all in apd_set_distance_mode(2) on a cfg-3-shaped batch (1024 sequences of ~1024 frames, D = 13, band 6.25 %),
           cells as apd_align_work counts them.

Both are timed with the library's own events (apd_set_timing / apd_last_kernel_ms); the best of `--repeats` runs counts.  Prints
ONE JSON line: milliseconds, cells and cells per second of each, and ratio = spot rate / strict rate.  The strict kernels share
every literal distance between the two orders of a pair and carry no start column, so a ratio of one half is the allowance.

    python tools/spot_bench.py [--repeats 3] [--small]
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
    ap.add_argument("--small", action="store_true", help="a sixteenth of both workloads (a quick look, not the recorded figure)")
    args = ap.parse_args()

    import numpy as np

    from audio_pattern_discovery_amd import _lib, synth
    from audio_pattern_discovery_amd.alignments import AlignmentWorkers, NDSequence, align_work
    from audio_pattern_discovery_amd.discovery import Discovery

    n_templates, template_len, n_streams, stream_len = (64, 128, 16, 16384) if args.small else (64, 128, 256, 16384)
    n_seq, length, pct = (256 if args.small else 1024), 1024, 0.0625

    ctx = _lib.Context(0)
    ctx.set_timing(True)
    out = {}

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
    spot_ms = []
    for _ in range(args.repeats):
        _, best = wt.spot(pairs, Discovery(), curves=False, streams=ws)
        spot_ms.append(ctx.last_kernel_ms())
    found = sum(1 for r in range(n_streams) if best[(r % n_templates) * n_streams + r]["score"] == 0.0)
    wt.close()
    ws.close()
    spot_cells = len(pairs) * template_len * stream_len
    out["spot"] = dict(pairs=len(pairs), cells=spot_cells, kernel_ms=spot_ms, cells_per_s=spot_cells / (min(spot_ms) * 1e-3),
                       planted_found=found, planted=n_streams)

    frames, offsets = synth.make_sequences(n_seq, length, DIM, seed=0xA9D0)
    cfg = Discovery(warping_band_percentage=pct)
    workers = AlignmentWorkers.new([NDSequence(s) for s in synth.split(frames, offsets)], ctx)
    ctx.set_distance_mode("strict")
    strict_ms = []
    for _ in range(args.repeats + 1):                                          # the first call builds the tile plan
        workers.align_all(cfg)
        strict_ms.append(ctx.last_kernel_ms())
    strict_ms = strict_ms[1:]
    workers.close()
    _, strict_cells, _ = align_work(offsets, DIM, cfg.align_config())
    out["strict"] = dict(n_seq=n_seq, cells=strict_cells, kernel_ms=strict_ms, cells_per_s=strict_cells / (min(strict_ms) * 1e-3))
    out["ratio"] = out["spot"]["cells_per_s"] / out["strict"]["cells_per_s"]
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
