#!/usr/bin/env python3
"""Step time of the autoencoder trainer.  13 -> 8 and 26 -> 10 on 2^20 resident frames ~ N(0, 2^2), one
epoch (every frame once, the order of apd_train_order) per measurement, timed with the library's events (apd_set_timing /
apd_last_kernel_ms: the training kernel alone), best of --repeats with the spread:
  * nanoseconds per step for ONE model;
  * model-steps per second with 1, 64, 256 and 1024 models side by side (shared order, own inits): up to one model per SIMD
    (1024 on an MI355X) the kernel time should not grow;
  * the single-thread C++ restatement of the same step (tools/train_cpu.cpp, g++ -O2) on this machine's CPU: the baseline a user of
    this library had before -- NOT the Rust reference, which is not built here.
usage: python tools/train_bench.py [--frames N] [--repeats R] [--models 1,64,256,1024] [--no-cpu]     one JSON line per figure."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def cpu_baseline(d, l, frames, repeats):
    exe = os.path.join(ROOT, "build", "train_cpu")
    src = os.path.join(ROOT, "tools", "train_cpu.cpp")
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-x", "c++", src, "-o", exe])
    out = subprocess.run([exe, "bench", str(d), str(l), str(frames), str(repeats)], capture_output=True, text=True, check=True)
    return json.loads(out.stdout)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--models", default="1,64,256,1024")
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    from audio_pattern_discovery_amd import _lib
    from audio_pattern_discovery_amd.neural import AutoEncoder, Trainer, train_order
    ctx = _lib.Context(0)
    ctx.set_timing(True)
    counts = [int(c) for c in args.models.split(",")]
    for d, l in ((13, 8), (26, 10)):
        rng = np.random.default_rng(d)
        frames = (rng.standard_normal((args.frames, d)) * 2.0).astype(np.float32)
        d_x = ctx.upload(frames)
        offsets = np.array([0, args.frames], np.uint64)
        for n_models in counts:
            models = [AutoEncoder.new(d, l, np.random.default_rng(100 + m)) for m in range(n_models)]
            ms = []
            with Trainer(ctx, models) as t:
                t.run((d_x.at(), args.frames), train_order(0, 99, offsets)[:4096], 0.1, on_device=True)      # code object loaded
                for r in range(args.repeats if n_models == 1 else min(args.repeats, 3)):
                    t.run((d_x.at(), args.frames), train_order(0, r, offsets), 0.1, on_device=True)
                    ms.append(ctx.last_kernel_ms())
                finite = sum(first is None for _, _, first in t.totals())
            best = min(ms)
            print(json.dumps({"what": "gpu", "d_in": d, "latent": l, "models": n_models, "steps": args.frames, "kernel_ms_best": round(best, 3),
                              "kernel_ms_worst": round(max(ms), 3), "ns_per_step": round(best * 1e6 / args.frames, 2),
                              "model_steps_per_s": round(n_models * args.frames / (best * 1e-3)), "models_still_finite": finite}), flush=True)
        d_x.free()
        if not args.no_cpu:
            print(json.dumps(dict(what="cpu single thread (C++ restatement, not the Rust reference)", **cpu_baseline(d, l, args.frames, min(args.repeats, 3)))),
                  flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
