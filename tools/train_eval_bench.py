#!/usr/bin/env python3
"""Evaluation of resident models on held-out frames.  Section 4.18's workload: 2^20 resident frames ~
N(0, 2^2), identity order, 13 -> 8 and 26 -> 10, with 1, 64 and 1024 models.  The routes take turns in one process, --repeats turns,
best and worst of each, timed with the library's events (apd_set_timing / apd_last_kernel_ms) and with the wall clock around the call:
  (a) what a caller had before apd_trainer_evaluate: a second trainer's run(alpha = 0) + totals() (1 and 64 models only: seconds a run);
  (b) evaluate, totals only;
  (c) evaluate, totals and the per-frame errors left on the device;
  (f) the forward pass alone (errors left on the device, no totals): (b) - (f) is the sequential chain of the totals;
  (d) tools/train_eval_cpu.cpp at -O2 on one host thread, one model.
usage: python tools/train_eval_bench.py [--frames N] [--repeats R] [--models 1,64,1024] [--no-cpu]      one JSON line per figure."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def cpu_baseline(d, l, frames, repeats):
    exe = os.path.join(ROOT, "build", "train_eval_cpu")
    src = os.path.join(ROOT, "tools", "train_eval_cpu.cpp")
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", src, "-o", exe])
    out = subprocess.run([exe, "bench", str(d), str(l), str(frames), str(repeats)], capture_output=True, text=True, check=True)
    return json.loads(out.stdout)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--models", default="1,64,1024")
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    from audio_pattern_discovery_amd import _lib
    from audio_pattern_discovery_amd.neural import AutoEncoder, Trainer
    ctx = _lib.Context(0)
    ctx.set_timing(True)
    L = _lib.lib()
    n = args.frames
    identity = np.arange(n, dtype=np.uint32)
    for d, l in ((13, 8), (26, 10)):
        frames = (np.random.default_rng(d).standard_normal((n, d)) * 2.0).astype(np.float32)
        d_x = ctx.upload(frames)
        for n_models in (int(c) for c in args.models.split(",")):
            models = [AutoEncoder.new(d, l, np.random.default_rng(100 + m)) for m in range(n_models)]
            d_err = ctx.alloc(n_models * n * 4)
            times = {}
            with Trainer(ctx, models) as t, Trainer(ctx, models) as clone:
                total, first = np.empty(n_models, np.float32), np.empty(n_models, np.uint64)

                def forward_only():
                    _lib.check(L.apd_trainer_evaluate(ctx.handle, t.handle, d_x.at(), n, 1, None, n, 0, d_err.at(), 1, None, None), ctx.handle)

                def parents_route():
                    clone.run((d_x.at(), n), identity, 0.0, on_device=True)
                    ms = ctx.last_kernel_ms()
                    return ms, np.array([e for e, _, _ in clone.totals(reset=True)], np.float32)

                routes = {"b evaluate, totals": lambda: t.evaluate((d_x.at(), n), on_device=True)[0],
                          "c evaluate, totals and device errors": lambda: t.evaluate((d_x.at(), n), on_device=True, errors=d_err.at())[1],
                          "f forward pass alone": forward_only}
                t.evaluate((d_x.at(), min(n, 4096)), on_device=True)                   # code objects loaded
                clone.run((d_x.at(), n), identity[:64], 0.0, on_device=True)
                clone.totals(reset=True)
                results = {}
                for _ in range(args.repeats):
                    if n_models <= 64:
                        t0 = time.perf_counter()
                        ms, results["a"] = parents_route()
                        times.setdefault("a run(alpha = 0) + totals on a second trainer", []).append((ms, (time.perf_counter() - t0) * 1e3))
                    for name, call in routes.items():
                        t0 = time.perf_counter()
                        results[name[0]] = call()
                        wall = (time.perf_counter() - t0) * 1e3
                        times.setdefault(name, []).append((ctx.last_kernel_ms(), wall))
                same = "a" not in results or bool(np.array_equal(results["a"].view(np.uint32), results["b"].view(np.uint32)))
                finite = int(np.isfinite(results["b"]).sum())
            d_err.free()
            for name, ts in times.items():
                k, w = [x[0] for x in ts], [x[1] for x in ts]
                print(json.dumps({"what": "gpu", "route": name, "d_in": d, "latent": l, "models": n_models, "positions": n, "kernel_ms_best": round(min(k), 3),
                                  "kernel_ms_worst": round(max(k), 3), "wall_ms_best": round(min(w), 3), "wall_ms_worst": round(max(w), 3),
                                  "ns_per_model_position": round(min(k) * 1e6 / (n * n_models), 4), "totals_equal_route_a": same, "finite_totals": finite}),
                      flush=True)
        d_x.free()
        if not args.no_cpu:
            print(json.dumps(dict(what="cpu single thread (C++ restatement, not the Rust reference)", route="d", **cpu_baseline(d, l, n, min(args.repeats, 3)))),
                  flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
