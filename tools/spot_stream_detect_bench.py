#!/usr/bin/env python3
"""Online detection on a streaming session against the route it replaces, in one process.

  Section 4.13's workload: 64 templates of 128 frames, 16 channels of 16 384 frames, D = 13, fed in chunks of 1024 columns that are
  already packed on the device (16 pushes).  Thresholds: the 1 % quantile of every pair's own scores.

  curves:   the route a caller had before: an unarmed session, every push copies both curves to the host (8 bytes per template,
            channel and column); the host's peak picking is NOT timed, which favours this route;
  best:     an unarmed session, best only (nothing but 16 bytes per pair leaves the device);
  pair:     an armed session per pair, holdoff = the template length, best only on the host, the queue drained after every push;
  channel:  the same with the templates of a channel competing.

Wall time of the 16 pushes (and drains), every repeat printed, the best of `--repeats` after one warm-up run counts; the library's
own events (apd_set_timing / apd_last_kernel_ms, summed over the pushes) beside it.  `scan_ms_per_push` is the armed session's kernel time
minus that of `curves` -- the same sweeps, storing the same curves -- per push: the hold-off scan, whose model is 8 bytes per curve
entry read once.  Before anything is printed the armed sessions' bests are compared with the unarmed ones' bit for bit, and the
drained hits with a plain restatement of the machine on the curves of `curves`.  `--modes curves,best` uses nothing beyond the
streaming session itself, so the same script times an older build through APD_LIB.  Prints ONE JSON line.

    python tools/spot_stream_detect_bench.py [--repeats 5] [--modes curves,best,pair,channel] [--small]
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
CHUNK = 1024


def machine(np, cost, start, n, thresholds, n_queries, per_stream, holdoff):
    """The contract of include/apd.h on whole-stream curves [pairs][columns]: the hits of every group, then a flush; a list of
    (pair, end, start, cost bits, score bits, rank) in drain order."""
    pairs, m = cost.shape
    with np.errstate(all="ignore"):
        score = cost / (n + np.arange(1, m + 1, dtype=np.int64)[None, :] - start.astype(np.int64) + 1).astype(np.float32)
        cand = (score < thresholds[:, None]) & (start != 0)
    out = []
    size = n_queries if per_stream else 1
    for g in range(pairs // size):
        mine = slice(g * size, (g + 1) * size)
        columns = np.flatnonzero(np.any(cand[mine], axis=0))
        # the group's one candidate per column: the smallest score, the smaller pair among equal ones (argmin takes the first)
        winner = g * size + np.argmin(np.where(cand[mine][:, columns], score[mine][:, columns], np.inf), axis=0)
        pending, floor, rank = None, 0, 0
        for i, p in zip(columns, winner):
            j = int(i) + 1
            if pending is not None and j - pending[1] > holdoff:
                out.append(pending + (rank,)); rank += 1; floor = pending[1]; pending = None
            c = (int(p), j, int(start[p, i]), cost[p, i], score[p, i])
            if c[2] <= floor:
                continue
            if pending is None:
                pending = c
            elif c[2] <= pending[1]:
                if c[4] < pending[4]:
                    pending = c
            else:
                out.append(pending + (rank,)); rank += 1; floor = pending[1]; pending = c
        if pending is not None:                                              # the timer at the stream's end, or the flush
            out.append(pending + (rank,))
    return [(p, e, s, np.float32(c).view(np.uint32), np.float32(sc).view(np.uint32), r) for p, e, s, c, sc, r in out]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--modes", default="curves,best,pair,channel")
    ap.add_argument("--small", action="store_true", help="channels of 4096 frames (a quick look, not the recorded figure)")
    args = ap.parse_args()
    modes = args.modes.split(",")

    import numpy as np

    from audio_pattern_discovery_amd import _lib
    if os.environ.get("APD_LIB"):                                            # an older build: bind what it exports
        probe = C.CDLL(_lib.LIB_PATH)
        _lib.SYMBOLS = [s for s in _lib.SYMBOLS if hasattr(probe, s[0])]
    from audio_pattern_discovery_amd.alignments import SPOT_HIT, AlignmentWorkers, NDSequence
    from audio_pattern_discovery_amd.discovery import Discovery

    n_templates, template_len, n_streams, stream_len = 64, 128, 16, (4096 if args.small else 16384)
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
    wt = AlignmentWorkers.new(templates, ctx)
    n_pairs = n_templates * n_streams
    pushes = stream_len // CHUNK
    out = dict(pairs=n_pairs, cells=n_pairs * template_len * stream_len, chunk=CHUNK, pushes=pushes, curve_bytes_per_push=8 * n_pairs * CHUNK)

    session = wt.spot_stream(list(range(n_templates)), Discovery(), channels=n_streams)
    L = _lib.lib()
    u64p, f32p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    chunk_off = np.arange(n_streams + 1, dtype=np.uint64) * CHUNK
    device = [ctx.upload(np.ascontiguousarray(np.concatenate([s.frames[k * CHUNK:(k + 1) * CHUNK] for s in streams], axis=0))) for k in range(pushes)]
    curve_off = np.zeros(n_pairs + 1, dtype=np.uint64)
    best = np.zeros(n_pairs, dtype=np.dtype([("end", np.uint32), ("start", np.uint32), ("cost", np.float32), ("score", np.float32)]))
    bestp = best.ctypes.data_as(C.POINTER(_lib.SpotBest))
    cost = np.zeros((pushes, n_pairs, CHUNK), dtype=np.float32)
    start = np.zeros((pushes, n_pairs, CHUNK), dtype=np.uint32)

    def feed(with_curves, drain, arm=None):
        """One pass over the streams: (wall ms, kernel ms, drained hits).  arm: (thresholds, per_stream) -- armed afresh before
        the clock starts, since a reset keeps the ranks going."""
        session.reset()
        if arm is not None:
            session.detect(arm[0], per_stream=arm[1], holdoff=template_len)
        hits, k_ms = [], 0.0
        t0 = time.perf_counter()
        for k in range(pushes):
            head = (ctx.handle, session.handle, C.c_void_p(device[k].ptr), chunk_off.ctypes.data_as(u64p), DIM, 1)
            if with_curves:
                rc = L.apd_spot_stream_push(*head, cost[k].ctypes.data_as(f32p), start[k].ctypes.data_as(u32p), n_pairs * CHUNK,
                                            curve_off.ctypes.data_as(u64p), bestp)
            else:
                rc = L.apd_spot_stream_push(*head, None, None, 0, curve_off.ctypes.data_as(u64p), bestp)
            _lib.check(rc, ctx.handle)
            k_ms += ctx.last_kernel_ms()
            if drain:
                hits.append(session.hits())
        if drain:
            session.flush()
            hits.append(session.hits())
        return (time.perf_counter() - t0) * 1e3, k_ms, hits

    def timed(with_curves, drain, arm=None):
        wall, kernel, hits = [], [], None
        for rep in range(args.repeats + 1):                                  # the first repeat is the warm-up
            w, k, hits = feed(with_curves, drain, arm)
            if rep:
                wall.append(w)
                kernel.append(k)
        return dict(wall_ms=wall, kernel_ms=kernel), hits

    thresholds = whole_cost = whole_start = None
    if "curves" in modes:
        out["curves"], _ = timed(True, False)
        whole_cost, whole_start = np.concatenate(list(cost), axis=1), np.concatenate(list(start), axis=1)
        with np.errstate(all="ignore"):
            score = whole_cost / (template_len + np.arange(1, stream_len + 1, dtype=np.int64)[None, :] - whole_start.astype(np.int64) + 1).astype(np.float32)
        score[~np.isfinite(score)] = np.inf
        thresholds = np.quantile(score, 0.01, axis=1).astype(np.float32)
        plain_best = best.copy()
    if "best" in modes:
        out["best"], _ = timed(False, False)
    for mode in ("pair", "channel"):
        if mode not in modes:
            continue
        assert thresholds is not None, "the armed modes take their thresholds from the curves of `curves`"
        per_stream = mode == "channel"
        out[mode], hits = timed(False, True, (thresholds.reshape(n_streams, n_templates), per_stream))
        session.detect(None)
        assert np.array_equal(best.view(np.uint32), plain_best.view(np.uint32)), "arming changed the bests"
        got = np.concatenate(hits).astype(SPOT_HIT)
        got = got[np.lexsort((got["rank"], got["pair"] // (n_templates if per_stream else 1)))]
        want = machine(np, whole_cost, whole_start, template_len, thresholds, n_templates, per_stream, template_len)
        have = [(int(h["pair"]), int(h["end"]), int(h["start"]), h["cost"].view(np.uint32), h["score"].view(np.uint32), int(h["rank"])) for h in got]
        if have != want:
            bad = next((k for k, (a, b) in enumerate(zip(have, want)) if a != b), min(len(have), len(want)))
            print("%s: %d drained, %d expected, first difference at %d: %s / %s" % (mode, len(have), len(want), bad, have[bad:bad + 2], want[bad:bad + 2]),
                  file=sys.stderr)
        assert have == want, "%s: the drained hits differ from the machine on the host's curves" % mode
        out[mode]["hits"] = len(got)
        out[mode]["wall_over_curves"] = min(out[mode]["wall_ms"]) / min(out["curves"]["wall_ms"])
        out[mode]["scan_ms_per_push"] = (min(out[mode]["kernel_ms"]) - min(out["curves"]["kernel_ms"])) / pushes
    for buf in device:
        buf.free()
    session.close()
    wt.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
