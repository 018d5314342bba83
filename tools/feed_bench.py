#!/usr/bin/env python3
"""Raw audio into a streaming session: the audio feed against the route it replaces, in one process.

  README's streaming workload with audio in front of it: 64 templates of 128 frames, 16 channels, 16 384 columns per channel, fed in
  chunks of 1024 and of 128 columns' worth of int16 samples; window 256, step 128, filter 18 (13 bins), once as they are (D = 13) and
  once through a 13 -> 10 encoder (templates of 10 dimensions).  Bests only: nothing but 16 bytes per pair leaves the device.

  (a) today:   the caller keeps every channel's tail on the host, packs [tail | chunk] per channel, uploads it, and calls
               apd_cepstrum_batch(on_device) (a plan built, five tables uploaded, one synchronisation, per push), apd_encode_async,
               apd_spot_stream_push(frames_on_device);
  (b) audio:   apd_spot_stream_push_audio with the samples resident on the device; `audio_host`: the same from host samples (the
               bytes route (a) uploads, minus the tails);
  (c) front:   the front end alone, every call blocking: apd_feed_push into a device buffer against apd_cepstrum_batch_async (+
               apd_encode_async) + apd_synchronize with a plan made in advance over the same number of frames per channel.  Beside
               the wall time of a call, `event_ms`: the time between two events on the stream -- the library's own around the feed's
               launch (apd_last_kernel_ms), this script's around the one or two enqueue-only calls.  Pushes of full size only (the
               first and last differ by a frame);
  (d) frames:  apd_spot_stream_push on feature frames resident on the device, this build against `--parent-lib` (an older
               libapd_hip.so), taking turns; and `plan_async_event_ms`, the two kernels whose bodies the feed shares
               (apd_cepstrum_batch_async + apd_encode_async, 16 x 1024 frames) on both builds: there the figures under `wall_ms`
               are the event time of one pair of calls, not wall time.

Every figure is the wall time of one pass (all pushes of all channels), in ms; the routes take turns inside every repeat, the first
repeat is a warm-up, and each route reports every repeat: the best counts, the spread is max - min.  Before anything is timed the
bests of (a) and (b) are compared bit for bit.  Prints ONE JSON line.

    python tools/feed_bench.py [--repeats 5] [--parent-lib PATH] [--small]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FFT, STEP, FILT, BINS, LATENT = 256, 128, 18, 13, 10
N_TEMPLATES, TEMPLATE_LEN, N_CHANNELS = 64, 128, 16


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="an older libapd_hip.so for (d)")
    ap.add_argument("--small", action="store_true", help="channels of 2048 columns (a quick look, not the recorded figure)")
    args = ap.parse_args()

    import numpy as np

    from audio_pattern_discovery_amd import _lib

    u64p, f32p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    vp = C.c_void_p
    columns = 2048 if args.small else 16384
    rng = np.random.default_rng(0xFEED)
    audio = [rng.integers(-32768, 32768, size=STEP * columns + FFT).astype(np.int16) for _ in range(N_CHANNELS)]
    w = rng.normal(0, 0.3, size=(BINS, LATENT)).astype(np.float32)
    b = rng.normal(0, 0.5, size=LATENT).astype(np.float32)
    templates = {d: rng.standard_normal((N_TEMPLATES * TEMPLATE_LEN, d)).astype(np.float32) for d in (BINS, LATENT)}
    t_off = (np.arange(N_TEMPLATES + 1, dtype=np.uint64) * TEMPLATE_LEN)
    queries = np.arange(N_TEMPLATES, dtype=np.uint32)
    n_pairs = N_TEMPLATES * N_CHANNELS

    def bind(path):
        lib = C.CDLL(path)
        for name, res, argtypes in _lib.SYMBOLS:
            if hasattr(lib, name):
                fn = getattr(lib, name)
                fn.restype, fn.argtypes = res, argtypes
        return lib

    class Side:
        """One library: a context, and sessions on it."""

        def __init__(self, lib):
            self.L = lib
            self.ctx = vp()
            self.ok(lib.apd_create(0, C.byref(self.ctx)))
            self.ok(lib.apd_set_timing(self.ctx, 1))
            self.cfg = _lib.AlignConfig(0.0, 1.0, 1.0, 1.0)

        def ok(self, rc):
            if rc != 0:
                raise RuntimeError("apd status %d: %s" % (rc, self.L.apd_last_error(self.ctx).decode() if self.ctx else ""))

        def session(self, dim):
            batch, s = vp(), vp()
            self.ok(self.L.apd_batch_create(self.ctx, templates[dim].ctypes.data, t_off.ctypes.data_as(u64p), N_TEMPLATES, dim, 0, C.byref(batch)))
            self.ok(self.L.apd_spot_stream_create(self.ctx, batch, C.byref(self.cfg), queries.ctypes.data_as(u32p), N_TEMPLATES, N_CHANNELS, C.byref(s)))
            return batch, s

        def alloc(self, nbytes):
            p = vp()
            self.ok(self.L.apd_device_alloc(self.ctx, max(int(nbytes), 16), C.byref(p)))
            return p

        def upload(self, array):
            a = np.ascontiguousarray(array)
            p = self.alloc(a.nbytes)
            self.ok(self.L.apd_copy_to_device(self.ctx, p, a.ctypes.data, a.nbytes))
            return p

    here = Side(_lib.lib())
    L, ctx = here.L, here.ctx
    # the HIP runtime the library is bound to, for events around the enqueue-only calls of (c): they record none of their own
    hip = C.CDLL(next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line))
    stream, ev0, ev1 = vp(), vp(), vp()
    for rc in (hip.hipStreamCreate(C.byref(stream)), hip.hipEventCreate(C.byref(ev0)), hip.hipEventCreate(C.byref(ev1))):
        assert rc == 0, "HIP status %d" % rc
    here.ok(L.apd_set_stream(ctx, stream))
    out = dict(fft=FFT, step=STEP, filter=FILT, bins=BINS, latent=LATENT, templates=N_TEMPLATES, template_len=TEMPLATE_LEN,
               channels=N_CHANNELS, columns=columns, repeats=args.repeats)
    curve_off = np.zeros(n_pairs + 1, dtype=np.uint64)
    best = np.zeros(n_pairs, dtype=np.dtype([("end", np.uint32), ("start", np.uint32), ("cost", np.float32), ("score", np.float32)]))
    bestp = best.ctypes.data_as(C.POINTER(_lib.SpotBest))

    def turns(routes):
        """routes: name -> function returning the wall ms of one pass.  Every repeat runs every route once, in order."""
        wall = {name: [] for name in routes}
        for rep in range(args.repeats + 1):
            for name, fn in routes.items():
                ms = fn()
                if rep:
                    wall[name].append(ms)
        return {name: dict(wall_ms=[round(v, 4) for v in ms], best_ms=round(min(ms), 4), spread_ms=round(max(ms) - min(ms), 4)) for name, ms in wall.items()}

    enc = vp()
    here.ok(L.apd_encoder_create(ctx, w.ctypes.data_as(f32p), b.ctypes.data_as(f32p), BINS, LATENT, C.byref(enc)))

    for chunk_cols in (1024, 128):
        pushes = columns // chunk_cols
        bounds = [k * chunk_cols * STEP for k in range(pushes)] + [len(audio[0])]        # the last chunk carries the closing window
        chunks = [[a[bounds[k]:bounds[k + 1]] for a in audio] for k in range(pushes)]
        packed = [np.concatenate(c) for c in chunks]
        s_off = [np.concatenate([[0], np.cumsum([len(x) for x in c])]).astype(np.uint64) for c in chunks]
        d_packed = [here.upload(p) for p in packed]
        room = max(len(p) for p in packed) + N_CHANNELS * FFT
        d_stage = here.alloc(room * 2)
        d_cep = here.alloc((room // STEP + N_CHANNELS) * BINS * 4)
        d_enc = here.alloc((room // STEP + N_CHANNELS) * LATENT * 4)
        result = {}
        for dim in (BINS, LATENT):
            batch, session = here.session(dim)
            feed, fdim = vp(), C.c_uint32(0)
            here.ok(L.apd_feed_create(ctx, N_CHANNELS, FFT, STEP, FILT, enc if dim == LATENT else None, C.byref(fdim), C.byref(feed)))
            assert fdim.value == dim

            def today():
                here.ok(L.apd_spot_stream_reset(ctx, session, 0xFFFFFFFF, 0))
                tails = [a[:0] for a in audio]
                f_off, nb = np.zeros(N_CHANNELS + 1, dtype=np.uint64), C.c_uint32(0)
                t0 = time.perf_counter()
                for k in range(pushes):
                    parts = [np.concatenate([t, c]) for t, c in zip(tails, chunks[k])]
                    host = np.concatenate(parts)
                    off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.uint64)
                    here.ok(L.apd_copy_to_device(ctx, d_stage, host.ctypes.data, host.nbytes))
                    here.ok(L.apd_cepstrum_batch(ctx, d_stage, off.ctypes.data_as(u64p), N_CHANNELS, FFT, STEP, FILT, 1, d_cep, f_off.ctypes.data_as(u64p), C.byref(nb)))
                    rows = d_cep
                    if dim == LATENT:
                        here.ok(L.apd_encode_async(ctx, enc, d_cep, int(f_off[-1]), d_enc))
                        rows = d_enc
                    here.ok(L.apd_spot_stream_push(ctx, session, rows, f_off.ctypes.data_as(u64p), dim, 1, None, None, 0, curve_off.ctypes.data_as(u64p), bestp))
                    made = np.diff(f_off).astype(np.int64)
                    tails = [p[int(m) * STEP:] for p, m in zip(parts, made)]                # from the next window's first sample on
                return (time.perf_counter() - t0) * 1e3

            def audio_route(on_device):
                def run():
                    here.ok(L.apd_spot_stream_reset(ctx, session, 0xFFFFFFFF, 0))
                    here.ok(L.apd_feed_reset(ctx, feed, 0xFFFFFFFF))
                    t0 = time.perf_counter()
                    for k in range(pushes):
                        samples = d_packed[k] if on_device else packed[k].ctypes.data
                        here.ok(L.apd_spot_stream_push_audio(ctx, session, feed, samples, s_off[k].ctypes.data_as(u64p), int(on_device), None, None, 0,
                                                             curve_off.ctypes.data_as(u64p), bestp))
                    return (time.perf_counter() - t0) * 1e3
                return run

            today()
            want = best.copy()
            audio_route(True)()
            assert best.tobytes() == want.tobytes(), "the audio route's bests differ from today's route"
            audio_route(False)()
            assert best.tobytes() == want.tobytes(), "the host-sample audio route's bests differ from today's route"
            r = turns({"today": today, "audio": audio_route(True), "audio_host": audio_route(False)})
            r["audio_over_today"] = round(r["audio"]["best_ms"] / r["today"]["best_ms"], 4)

            # (c) the front end alone, pushes of full size, every call blocking
            full = list(range(1, pushes - 1))
            frames_full = chunk_cols
            plan_off = (np.arange(N_CHANNELS + 1, dtype=np.uint64) * (FFT + STEP * (frames_full - 1) + 1))
            p_off, nb, plan = np.zeros(N_CHANNELS + 1, dtype=np.uint64), C.c_uint32(0), vp()
            here.ok(L.apd_cepstrum_plan_create(ctx, plan_off.ctypes.data_as(u64p), N_CHANNELS, FFT, STEP, FILT, p_off.ctypes.data_as(u64p), C.byref(nb), C.byref(plan)))
            assert int(p_off[-1]) == N_CHANNELS * frames_full
            d_plan_samples = here.upload(np.concatenate([a[:int(plan_off[1])] for a in audio]))
            f_off = np.zeros(N_CHANNELS + 1, dtype=np.uint64)
            events = []

            def front_feed():
                here.ok(L.apd_feed_reset(ctx, feed, 0xFFFFFFFF))
                here.ok(L.apd_feed_push(ctx, feed, d_packed[0], s_off[0].ctypes.data_as(u64p), 1, d_cep if dim == BINS else d_enc, 1, room, f_off.ctypes.data_as(u64p)))
                total, ev = 0.0, 0.0
                for k in full:
                    t0 = time.perf_counter()
                    here.ok(L.apd_feed_push(ctx, feed, d_packed[k], s_off[k].ctypes.data_as(u64p), 1, d_cep if dim == BINS else d_enc, 1, room, f_off.ctypes.data_as(u64p)))
                    total += time.perf_counter() - t0
                    assert int(f_off[-1]) == N_CHANNELS * frames_full
                    ev += L.apd_last_kernel_ms(ctx)
                events.append(ev / len(full))
                return total * 1e3 / len(full)

            plan_events = []

            def front_two():
                total, ev, ms = 0.0, 0.0, C.c_float(0)
                for k in full:
                    t0 = time.perf_counter()
                    hip.hipEventRecord(ev0, stream)
                    here.ok(L.apd_cepstrum_batch_async(ctx, plan, d_plan_samples, d_cep))
                    if dim == LATENT:
                        here.ok(L.apd_encode_async(ctx, enc, d_cep, N_CHANNELS * frames_full, d_enc))
                    hip.hipEventRecord(ev1, stream)
                    here.ok(L.apd_synchronize(ctx))
                    total += time.perf_counter() - t0
                    assert hip.hipEventElapsedTime(C.byref(ms), ev0, ev1) == 0
                    ev += ms.value
                plan_events.append(ev / len(full))
                return total * 1e3 / len(full)

            if full:
                c = turns({"feed_push": front_feed, "plan_async": front_two})
                c["feed_push"]["event_ms"] = [round(v, 4) for v in events[1:]]
                c["plan_async"]["event_ms"] = [round(v, 4) for v in plan_events[1:]]
                c["frames_per_call"] = N_CHANNELS * frames_full
                r["front_ms_per_push"] = c
            here.ok(L.apd_cepstrum_plan_destroy(plan))
            L.apd_device_free(ctx, d_plan_samples)
            here.ok(L.apd_feed_destroy(feed))
            here.ok(L.apd_spot_stream_destroy(session))
            here.ok(L.apd_batch_destroy(batch))
            result["D%d" % dim] = r
        for p in d_packed + [d_stage, d_cep, d_enc]:
            L.apd_device_free(ctx, p)
        out["chunk_%d" % chunk_cols] = result

    # (d) the existing path on feature frames, this build and the parent's taking turns
    if args.parent_lib:
        sides = {"this": here, "parent": Side(bind(args.parent_lib))}
        frames = rng.standard_normal((N_CHANNELS, columns, BINS)).astype(np.float32)
        d = {}
        for chunk_cols in (1024, 128):
            pushes = columns // chunk_cols
            chunk_off = np.arange(N_CHANNELS + 1, dtype=np.uint64) * chunk_cols
            routes, keep, bests = {}, [], {}
            for name, side in sides.items():
                batch, session = side.session(BINS)
                dev = [side.upload(frames[:, k * chunk_cols:(k + 1) * chunk_cols].reshape(-1, BINS)) for k in range(pushes)]
                keep.append((side, batch, session, dev))

                def run(side=side, session=session, dev=dev, name=name):
                    side.ok(side.L.apd_spot_stream_reset(side.ctx, session, 0xFFFFFFFF, 0))
                    t0 = time.perf_counter()
                    for k in range(pushes):
                        side.ok(side.L.apd_spot_stream_push(side.ctx, session, dev[k], chunk_off.ctypes.data_as(u64p), BINS, 1, None, None, 0,
                                                            curve_off.ctypes.data_as(u64p), bestp))
                    ms = (time.perf_counter() - t0) * 1e3
                    bests[name] = best.tobytes()
                    return ms
                routes[name] = run
            d["chunk_%d" % chunk_cols] = turns(routes)
            assert bests["this"] == bests["parent"], "the existing path's bests differ from the parent's"
            for side, batch, session, dev in keep:
                side.ok(side.L.apd_spot_stream_destroy(session))
                side.ok(side.L.apd_batch_destroy(batch))
                for p in dev:
                    side.L.apd_device_free(side.ctx, p)
        out["frames_push"] = d
        # ... and the two kernels whose bodies were factored: cepstrum_kernel and the staged encoder, 16 x 1024 frames, event ms
        here.ok(sides["parent"].L.apd_set_stream(sides["parent"].ctx, stream))
        frames_full = 1024
        plan_off = (np.arange(N_CHANNELS + 1, dtype=np.uint64) * (FFT + STEP * (frames_full - 1) + 1))
        packed = np.concatenate([a[:int(plan_off[1])] for a in audio])
        routes, keep = {}, []
        for name, side in sides.items():
            p_off, nb, plan, e = np.zeros(N_CHANNELS + 1, dtype=np.uint64), C.c_uint32(0), vp(), vp()
            side.ok(side.L.apd_cepstrum_plan_create(side.ctx, plan_off.ctypes.data_as(u64p), N_CHANNELS, FFT, STEP, FILT, p_off.ctypes.data_as(u64p),
                                                    C.byref(nb), C.byref(plan)))
            side.ok(side.L.apd_encoder_create(side.ctx, w.ctypes.data_as(f32p), b.ctypes.data_as(f32p), BINS, LATENT, C.byref(e)))
            bufs = (side.upload(packed), side.alloc(int(p_off[-1]) * BINS * 4), side.alloc(int(p_off[-1]) * LATENT * 4))
            keep.append((side, plan, e, bufs))

            def run(side=side, plan=plan, e=e, bufs=bufs, total=int(p_off[-1])):
                ev, ms = 0.0, C.c_float(0)
                for _ in range(14):
                    hip.hipEventRecord(ev0, stream)
                    side.ok(side.L.apd_cepstrum_batch_async(side.ctx, plan, bufs[0], bufs[1]))
                    side.ok(side.L.apd_encode_async(side.ctx, e, bufs[1], total, bufs[2]))
                    hip.hipEventRecord(ev1, stream)
                    side.ok(side.L.apd_synchronize(side.ctx))
                    assert hip.hipEventElapsedTime(C.byref(ms), ev0, ev1) == 0
                    ev += ms.value
                return ev / 14
            routes[name] = run
        out["plan_async_event_ms"] = turns(routes)
        for side, plan, e, bufs in keep:
            side.ok(side.L.apd_cepstrum_plan_destroy(plan))
            side.ok(side.L.apd_encoder_destroy(e))
            for p in bufs:
                side.L.apd_device_free(side.ctx, p)
        sides["parent"].L.apd_destroy(sides["parent"].ctx)
    L.apd_encoder_destroy(enc)
    L.apd_destroy(ctx)
    hip.hipStreamDestroy(stream)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
