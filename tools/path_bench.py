#!/usr/bin/env python3
"""Warping paths against the literal kernel on one batch: 91 cfg-3-shaped sequences (length ~1024, D = 13, band 6.25 %), all 8190
ordered pairs -- apd_align_paths (sweep + trace) and apd_align_all on the literal kernel (apd_set_variant 1), which produces the
same 8190 ordered scores.  Prints ONE JSON line: kernel milliseconds of each, split per kernel from one
`rocprofv3 --kernel-trace --stats` run of a child process, and their ratio.

    python tools/path_bench.py              # the measurement (starts the profiled child)
    python tools/path_bench.py --worker     # the child: the two calls, timed with the library's own events
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_SEQ, LENGTH, DIM, PCT, REPEATS = 91, 1024, 13, 0.0625, 2


def worker():
    import ctypes as C

    import numpy as np

    from audio_pattern_discovery_amd import _lib, synth
    from audio_pattern_discovery_amd.alignments import AlignmentWorkers, NDSequence
    from audio_pattern_discovery_amd.discovery import Discovery

    ctx = _lib.Context(0)
    ctx.set_timing(True)
    frames, offsets = synth.make_sequences(N_SEQ, LENGTH, DIM, seed=0xA9D0)
    workers = AlignmentWorkers.new([NDSequence(s) for s in synth.split(frames, offsets)], ctx)
    cfg = Discovery(warping_band_percentage=PCT)
    pairs = [(a, b) for a in range(N_SEQ) for b in range(N_SEQ) if a != b]
    out = dict(pairs=len(pairs), path_ms=[], literal_ms=[])
    for _ in range(REPEATS):
        steps, scores = workers.paths(pairs, cfg)
        out["path_ms"].append(ctx.last_kernel_ms())
    ctx.set_variant(1)
    ctx.set_distance_mode("strict")
    for _ in range(REPEATS):
        matrix = workers.align_all(cfg).reshape(N_SEQ, N_SEQ).copy()
        out["literal_ms"].append(ctx.last_kernel_ms())
    want = np.array([matrix[a, b] for a, b in pairs], dtype=np.float32)
    out["scores_bit_equal_literal"] = bool(np.array_equal(want.view(np.uint32), scores.view(np.uint32)))
    out["mean_path_len"] = float(np.mean([len(s) for s in steps]))
    workers.close()
    ctx.close()
    print("PATH_BENCH " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--worker", action="store_true")
    args = ap.parse_args()
    if args.worker:
        return worker()
    with tempfile.TemporaryDirectory() as d:
        run = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
                              sys.executable, os.path.abspath(__file__), "--worker"], capture_output=True, text=True, timeout=900)
        if run.returncode != 0:
            sys.exit("profiled child failed (%d):\n%s" % (run.returncode, (run.stdout + run.stderr)[-3000:]))
        line = [l for l in run.stdout.splitlines() if l.startswith("PATH_BENCH ")][-1]
        result = json.loads(line[len("PATH_BENCH "):])
        kernels = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as fp:
                for row in csv.DictReader(fp):
                    for key in ("dtw_path_sweep", "dtw_path_trace", "dtw_fused_generic"):
                        if key + "(" in row["Name"]:
                            kernels[key] = kernels.get(key, 0.0) + float(row["TotalDurationNs"]) / 1e6 / REPEATS
    result["sweep_ms"] = kernels.get("dtw_path_sweep")
    result["trace_ms"] = kernels.get("dtw_path_trace")
    result["literal_kernel_ms"] = kernels.get("dtw_fused_generic")
    if result["sweep_ms"] and result["trace_ms"] and result["literal_kernel_ms"]:
        result["ratio"] = (result["sweep_ms"] + result["trace_ms"]) / result["literal_kernel_ms"]
    print(json.dumps(result))


if __name__ == "__main__":
    main()
