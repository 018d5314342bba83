#!/usr/bin/env python3
"""Spot score quantiles on the device against the route the benches took before, in one process.

Section 4.15's workload: 64 templates of 128 frames against 16 streams of 16 384 frames, D = 13, from synth.py: 1024 pairs, 16.8 M
curve entries, 32 planted occurrences per stream.

  host_pair / host_all:  (A) apd_spot with curves (134 MB to the host), the scores and np.partition on the host -- per pair, and
                         over all scores at once -- wall time; the sweep's kernel time is taken from the same calls;
  pair / query / all:    (B) apd_spot_quantiles by="pair", by="query", by="all", with one perc and with eight -- wall and kernel time.

Before anything is timed B's values are compared bit for bit with A's (by="query" against a host partition of each template's 16
curves).  Then the routes take turns, `--repeats` times; the best of each counts and the spread (max - min) is reported next to it.
Kernel time: the library's own events (apd_set_timing / apd_last_kernel_ms).  Wall time: a host clock around the blocking calls,
buffers allocated beforehand, straight through the C ABI on one joined batch.  Prints ONE JSON line: every time in milliseconds, the
select kernels alone (the call's kernel time minus that of apd_spot with curves), the model next to them (four reads of 8 bytes per
entry at --hbm-gbs), and whether by="all" -- one group of 16.8 M entries -- is the slow one.  `--workgroups` (a list) repeats the B
routes under APD_SPOT_QUANTILE_WORKGROUPS = each value: the measurement the library's bound of workgroups per pass was picked from.

    python tools/spot_quantile_bench.py [--repeats 7] [--workgroups 256,1024,2048,4096,16384]
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
PERC1 = [0.001]
PERC8 = [0.0001, 0.001, 0.01, 0.05, 0.25, 0.5, 0.75, 0.99]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--hbm-gbs", type=float, default=4000.0, help="HBM rate of the model, GB/s")
    ap.add_argument("--workgroups", type=str, default="", help="comma-separated values of APD_SPOT_QUANTILE_WORKGROUPS to repeat route B under")
    args = ap.parse_args()

    import numpy as np

    from audio_pattern_discovery_amd import _lib, synth
    from audio_pattern_discovery_amd.alignments import Batch

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
    pairs = np.array([(t, n_templates + r) for t in range(n_templates) for r in range(n_streams)], dtype=np.uint32)   # a template's pairs adjacent
    n_pairs = len(pairs)
    entries = n_pairs * stream_len
    u32p, u64p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_float)
    head = (ctx.handle, joined.handle, C.byref(cfg), pairs.ctypes.data_as(u32p), n_pairs)
    cost, start = np.zeros(entries, dtype=np.float32), np.zeros(entries, dtype=np.uint32)
    curve_off = np.zeros(n_pairs + 1, dtype=np.uint64)
    column = np.tile(np.arange(1, stream_len + 1, dtype=np.int64), n_pairs) + (template_len + 1)
    values = np.zeros((n_pairs, 8), dtype=np.float32)
    status = np.zeros((n_pairs, 8), dtype=np.int32)
    n_groups = C.c_uint64(0)
    groupings = {"pair": (_lib.APD_QUANTILES_PER_PAIR, n_pairs), "query": (_lib.APD_QUANTILES_PER_QUERY, n_templates), "all": (_lib.APD_QUANTILES_ALL, 1)}

    def index(length, perc):
        nf = np.float32(length) * np.float32(perc)
        return int(nf) if nf > 0 else 0

    def host(by, perc):
        """Route A: (values [groups, len(perc)], wall ms, the sweep's kernel ms).  No NaN on this workload: the partition takes all."""
        groups = groupings[by][1]
        t0 = time.perf_counter()
        _lib.check(L.apd_spot(*head, cost.ctypes.data_as(f32p), start.ctypes.data_as(u32p), entries, curve_off.ctypes.data_as(u64p), None), ctx.handle)
        sweep_ms = ctx.last_kernel_ms()
        with np.errstate(all="ignore"):
            scores = (cost / (column - start).astype(np.float32)).reshape(groups, entries // groups)
        ks = sorted({index(scores.shape[1], p) for p in perc})
        part = np.partition(scores, ks, axis=1)
        out = np.stack([part[:, index(scores.shape[1], p)] for p in perc], axis=1)
        return out, (time.perf_counter() - t0) * 1e3, sweep_ms

    def device(by, perc):
        """Route B: (values, wall ms, kernel ms)."""
        pc = np.asarray(perc, dtype=np.float32)
        t0 = time.perf_counter()
        _lib.check(L.apd_spot_quantiles(*head, groupings[by][0], pc.ctypes.data_as(f32p), len(pc), values.ctypes.data_as(f32p),
                                        status.ctypes.data_as(C.POINTER(C.c_int32)), None, None, None, C.byref(n_groups)), ctx.handle)
        wall = (time.perf_counter() - t0) * 1e3
        ng = int(n_groups.value)
        assert ng == groupings[by][1] and not status.ravel()[:ng * len(pc)].any()
        return values.ravel()[:ng * len(pc)].reshape(ng, len(pc)).copy(), wall, ctx.last_kernel_ms()

    # the comparison that comes before any timing
    for by in groupings:
        for perc in (PERC1, PERC8):
            want, got = host(by, perc)[0], device(by, perc)[0]
            assert not np.isnan(want).any() and np.array_equal(np.where(want == 0, np.float32(0), want).view(np.uint32), got.view(np.uint32)), (by, perc)

    def measure(repeats, with_host):
        runs = {}
        for _ in range(repeats):
            if with_host:
                for by in ("pair", "all"):
                    _, wall, sweep_ms = host(by, PERC1)
                    runs.setdefault("host_%s_wall" % by, []).append(wall)
                    runs.setdefault("curves_sweep_kernel", []).append(sweep_ms)
            for by in groupings:
                for name, perc in (("1", PERC1), ("8", PERC8)):
                    _, wall, kernel = device(by, perc)
                    runs.setdefault("%s_%s_wall" % (by, name), []).append(wall)
                    runs.setdefault("%s_%s_kernel" % (by, name), []).append(kernel)
        return runs

    runs = measure(args.repeats, True)
    sweeps = {}
    for target in [t for t in args.workgroups.split(",") if t]:
        os.environ["APD_SPOT_QUANTILE_WORKGROUPS"] = target
        sweeps[target] = {k: min(v) for k, v in measure(3, False).items() if k.endswith("_kernel")}
    os.environ.pop("APD_SPOT_QUANTILE_WORKGROUPS", None)
    joined.close()
    bt.close()
    bs.close()
    ctx.close()
    best = {k: min(v) for k, v in runs.items()}
    spread = {k: max(v) - min(v) for k, v in runs.items()}
    sweep_ms = best["curves_sweep_kernel"]
    select = {k[:-7]: best[k] - sweep_ms for k in best if k.endswith("_kernel") and k != "curves_sweep_kernel"}
    model_ms = 4 * 8 * entries / (args.hbm_gbs * 1e9) * 1e3
    accepted = all(best["%s_%s_wall" % (by, n)] <= best["host_%s_wall" % ("all" if by == "all" else "pair")] for by in groupings for n in ("1", "8"))
    out = dict(pairs=n_pairs, entries=entries, perc_one=PERC1, perc_eight=PERC8, verified_bitwise_against_host_route=True,
               host_route_copy_bytes=8 * entries, repeats=args.repeats, ms=runs, best_ms=best, spread_ms=spread,
               curves_sweep_kernel_ms=sweep_ms, select_kernels_ms=select, model_select_ms=model_ms, model_hbm_gbs=args.hbm_gbs,
               all_over_pair_select=select["all_1"] / select["pair_1"] if select["pair_1"] > 0 else None,
               slowest_select=max(select, key=select.get), device_wall_not_above_host=accepted, workgroup_bound_sweep_kernel_ms=sweeps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
