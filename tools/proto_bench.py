#!/usr/bin/env python3
"""Cluster prototypes on one cfg-3-shaped batch: 4096 sequences (length ~1024, D = 13, band 6.25 %) as 64 sets of 64 members, the
first member of every set as init.  Measured in one process, with the library's own events (apd_last_kernel_ms):

  * one apd_barycenters iteration (init, sweep, trace, accumulate, finalize, pack: all kernels of the call);
  * apd_align_paths on the identical (init, member) pair list -- the same sweeps and traces, plus the download of every step;
  * apd_cluster_medoids of the 64 sets on the batch's own apd_align_all matrix (DESIGN.md section 4.11 puts it next to UPGMA's time).

Prints ONE JSON line.  The expectation section 4.11 states: barycenter_ms / paths_ms <= 1.

    python tools/proto_bench.py              # the measurement
    python tools/proto_bench.py --profile    # the same under `rocprofv3 --kernel-trace --stats`: adds milliseconds per kernel
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_SETS, SET_SIZE, LENGTH, DIM, PCT, REPEATS = 64, 64, 1024, 13, 0.0625, 2
KERNELS = ("dtw_path_sweep", "dtw_path_trace", "bary_init_kernel", "bary_scores_kernel", "bary_accumulate_kernel",
           "bary_finalize_kernel", "bary_pack_kernel", "medoid_cost_kernel", "medoid_pick_kernel")


def measure(n_sets, set_size, length):
    import numpy as np

    from audio_pattern_discovery_amd import _lib, clustering, synth
    from audio_pattern_discovery_amd.alignments import AlignmentWorkers, NDSequence
    from audio_pattern_discovery_amd.discovery import Discovery

    ctx = _lib.Context(0)
    ctx.set_timing(True)
    n_seq = n_sets * set_size
    frames, offsets = synth.make_sequences(n_seq, length, DIM, seed=0xDBA)
    workers = AlignmentWorkers.new([NDSequence(s) for s in synth.split(frames, offsets)], ctx)
    cfg = Discovery(warping_band_percentage=PCT)
    sets = [list(range(k * set_size, (k + 1) * set_size)) for k in range(n_sets)]
    init = [s[0] for s in sets]
    pairs = [(init[k], m) for k in range(n_sets) for m in sets[k]]
    out = dict(sets=n_sets, members=set_size, pairs=len(pairs), barycenter_ms=[], barycenter_wall_ms=[], paths_ms=[], paths_wall_ms=[])
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        protos, inertia, used = workers.barycenters(sets, cfg, init=init, iterations=1)
        out["barycenter_wall_ms"].append((time.perf_counter() - t0) * 1e3)
        out["barycenter_ms"].append(ctx.last_kernel_ms())
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        steps, scores = workers.paths(pairs, cfg)
        out["paths_wall_ms"].append((time.perf_counter() - t0) * 1e3)
        out["paths_ms"].append(ctx.last_kernel_ms())
    # the iteration's inertia is the mean of the very scores apd_align_paths returns (the barycenter before the update IS the init)
    want = []
    for k in range(n_sets):
        total = np.float32(0.0)
        for s in scores[k * set_size:(k + 1) * set_size]:
            total = np.float32(total + s)
        want.append(np.float32(total / np.float32(set_size)))
    out["inertia_bit_equal_paths"] = bool(np.array_equal(np.array(want, np.float32).view(np.uint32), inertia[0].view(np.uint32)))
    out["used_all"] = bool(np.all(used == set_size))
    out["ratio"] = min(out["barycenter_ms"]) / min(out["paths_ms"])
    matrix = workers.align_all(cfg)
    out["align_all_ms"] = ctx.last_kernel_ms()
    out["medoid_ms"] = []
    for _ in range(REPEATS):
        medoid, cost = clustering.medoids(matrix, sets, ctx)
        out["medoid_ms"].append(ctx.last_kernel_ms())
    workers.close()
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--profile", action="store_true", help="run the measurement as a child under rocprofv3 and add the time per kernel")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--sets", type=int, default=N_SETS)
    ap.add_argument("--members", type=int, default=SET_SIZE)
    ap.add_argument("--length", type=int, default=LENGTH)
    args = ap.parse_args()
    shape = ["--sets", str(args.sets), "--members", str(args.members), "--length", str(args.length)]
    if not args.profile:
        result = measure(args.sets, args.members, args.length)
        print(("PROTO_BENCH " if args.worker else "") + json.dumps(result), flush=True)
        return
    with tempfile.TemporaryDirectory() as d:
        run = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
                              sys.executable, os.path.abspath(__file__), "--worker"] + shape, capture_output=True, text=True, timeout=900)
        if run.returncode != 0:
            sys.exit("profiled child failed (%d):\n%s" % (run.returncode, (run.stdout + run.stderr)[-3000:]))
        line = [l for l in run.stdout.splitlines() if l.startswith("PROTO_BENCH ")][-1]
        result = json.loads(line[len("PROTO_BENCH "):])
        kernels = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as fp:
                for row in csv.DictReader(fp):
                    for key in KERNELS:
                        if key + "(" in row["Name"]:
                            kernels[key] = kernels.get(key, 0.0) + float(row["TotalDurationNs"]) / 1e6
    result["kernel_total_ms"] = kernels        # over the whole run: REPEATS barycenter calls and REPEATS path calls share sweep and trace
    print(json.dumps(result))


if __name__ == "__main__":
    main()
