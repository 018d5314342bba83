#!/usr/bin/env python3
"""apd_neighbors on seeded N x N matrices that are uploaded once: k in {1, 16, 64, 1024}, both axes,
skip_self, the library's own events (apd_last_kernel_ms), best of 5 with the spread after a warm-up of every shape.

    N = 4096    67 MB: resident in the 256 MiB Infinity Cache -- its rates are cache rates
    N = 16384   1.07 GB: HBM

Against the route a caller has without it, in the same process and taking turns with the new call:
  * apd_copy_to_host of the whole matrix (wall clock), and
  * numpy argpartition plus the sort of the k kept, per query, on a seeded sample of the queries, scaled to all of them; COLUMNS
    reads a strided column view, as a host caller has to.
And against the model: one read of rows * cols * 4 bytes at 6.3 TB/s (MI355X, measured streaming rate) for ROWS, three times the
bytes for the column form (the panel is written and read back).  Prints ONE JSON line.

    python tools/neighbors_bench.py                  # the measurement
    python tools/neighbors_bench.py --sizes 4096     # one size
    python tools/neighbors_bench.py --profile        # the same under `rocprofv3 --kernel-trace --stats`: adds milliseconds per kernel
"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES, KS, REPEATS, STREAM_RATE, HOST_SAMPLE = (4096, 16384), (1, 16, 64, 1024), 5, 6.3e12, 256
KERNELS = ("neighbors_select_kernel<true>", "neighbors_select_kernel<false>", "neighbors_gather_kernel")


def host_route(d, queries, k, axis):
    """What a caller does today with the downloaded matrix: (index [Q][k], seconds)."""
    import numpy as np
    t0 = time.perf_counter()
    out = np.empty((len(queries), k), np.int64)
    for s, q in enumerate(queries):
        line = d[q, :] if axis == 0 else d[:, q]                            # axis 1: a strided view of the whole matrix
        keep = np.flatnonzero(np.arange(len(line)) != q)
        v = line[keep]
        part = np.argpartition(v, k - 1)[:k] if k < len(v) else np.arange(len(v))
        part = np.flatnonzero(v <= v[part].max())                           # ties at the cut: all of them, the lowest indices win
        out[s] = keep[part[np.lexsort((keep[part], v[part]))][:k]]          # the k kept, by (value, index)
    return out, time.perf_counter() - t0


def measure(sizes):
    import numpy as np

    from audio_pattern_discovery_amd import _lib

    ctx = _lib.Context(0)
    ctx.set_timing(True)
    L = _lib.lib()
    out = dict(stream_rate=STREAM_RATE, repeats=REPEATS, sizes={})
    for n in sizes:
        rng = np.random.default_rng(n)
        d = rng.random((n, n), dtype=np.float32)
        np.fill_diagonal(d, 0.0)
        d_mat = ctx.upload(d)
        k_max = max(KS)
        bufs = [ctx.alloc(4 * n * k_max), ctx.alloc(4 * n * k_max), ctx.alloc(4 * n), ctx.alloc(4 * n)]
        sample = np.sort(rng.choice(n, size=min(HOST_SAMPLE, n), replace=False)).astype(np.uint32)
        back = np.empty_like(d)
        entry = dict(matrix_bytes=int(d.nbytes), in_infinity_cache=bool(d.nbytes < (256 << 20)), copy_to_host_ms=[], runs=[])

        def call(k, axis):
            _lib.check(L.apd_neighbors(ctx.handle, d_mat.at(), 1, n, n, axis, None, 0, k, 1, *[b.at() for b in bufs]), ctx.handle)
            return ctx.last_kernel_ms()                                     # waits for the call's last event

        for k in KS:                                                        # every shape once before anything is timed
            for axis in (0, 1):
                call(k, axis)
        for k in KS:
            for axis in (0, 1):
                ms, host_s = [], None
                for r in range(REPEATS):                                    # the new call and today's route take turns
                    ms.append(call(k, axis))
                    if r == 0:
                        t0 = time.perf_counter()
                        _lib.check(L.apd_copy_to_host(ctx.handle, C.c_void_p(back.ctypes.data), d_mat.at(), d.nbytes), ctx.handle)
                        entry["copy_to_host_ms"].append((time.perf_counter() - t0) * 1e3)
                        want, host_s = host_route(back, sample, k, axis)
                call(k, axis)
                got = bufs[0].to_numpy(np.uint32, n * k).reshape(n, k)[sample.astype(np.int64)]
                model_bytes = d.nbytes * (1 if axis == 0 else 3)
                best = min(ms)
                entry["runs"].append(dict(k=k, axis=("rows", "columns")[axis], ms_best=best, ms_all=ms, model_bytes=model_bytes,
                                          model_ms=model_bytes / STREAM_RATE * 1e3, achieved_bytes_per_s=model_bytes / (best * 1e-3),
                                          time_over_model=best * 1e-3 / (model_bytes / STREAM_RATE),
                                          numpy_ms_scaled=host_s * 1e3 * n / len(sample), numpy_sampled_queries=int(len(sample)),
                                          agrees_with_numpy=bool(np.array_equal(got.astype(np.int64), want))))
        entry["workgroup_sweep_rows_k16_ms"] = {}                           # APD_NEIGHBORS_WORKGROUP: the same bits, another launch
        for wg in (256, 512, 1024):
            os.environ["APD_NEIGHBORS_WORKGROUP"] = str(wg)
            try:
                call(16, 0)
                entry["workgroup_sweep_rows_k16_ms"][str(wg)] = min(call(16, 0) for _ in range(REPEATS))
            finally:
                del os.environ["APD_NEIGHBORS_WORKGROUP"]
        out["sizes"][str(n)] = entry
        for b in bufs + [d_mat]:
            b.free()
        del d, back
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--profile", action="store_true", help="run the measurement as a child under rocprofv3 and add the time per kernel")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--sizes", type=int, nargs="+", default=list(SIZES))
    args = ap.parse_args()
    if not args.profile:
        result = measure(args.sizes)
        print(("NEIGHBORS_BENCH " if args.worker else "") + json.dumps(result), flush=True)
        return
    with tempfile.TemporaryDirectory() as d:
        run = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
                              os.path.abspath(__file__), "--worker", "--sizes"] + [str(s) for s in args.sizes],
                             capture_output=True, text=True, timeout=1500)
        if run.returncode != 0:
            sys.exit("profiled child failed (%d):\n%s" % (run.returncode, (run.stdout + run.stderr)[-3000:]))
        line = [l for l in run.stdout.splitlines() if l.startswith("NEIGHBORS_BENCH ")][-1]
        result = json.loads(line[len("NEIGHBORS_BENCH "):])
        kernels = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as fp:
                for row in csv.DictReader(fp):
                    for key in KERNELS:
                        if key + "(" in row["Name"]:
                            kernels[key] = dict(calls=int(row.get("Calls", 0)), total_ms=float(row["TotalDurationNs"]) / 1e6)
    result["kernels"] = kernels                  # over the whole run: every k, both axes, warm-up included
    print(json.dumps(result))


if __name__ == "__main__":
    main()
