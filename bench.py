#!/usr/bin/env python3
"""Benchmark of the hot path: all-pairs Sakoe-Chiba-banded DTW distance matrix (reference
src/alignments.rs:31-67) on synthetic MFCC-like sequences.  NO torch anywhere: device buffers, streams,
the RCCL communicators and the timing fences all come from libapd_hip.so through its C ABI (include/apd.h).

    python bench.py --gpus N --steps K --warmup W [--full] [--dump-outputs DIR]

How N GPUs are driven:
  * WORLD_SIZE unset (how the driver starts it):  ONE process drives the N devices through the library's
    persistent multi-device handle (apd_multi_create: one context + worker thread per device, ncclCommInitAll,
    resident batches and gather buffers made once; a step = apd_multi_batch_refill + apd_multi_align_all_async).
  * under a launcher that sets RANK / LOCAL_RANK / WORLD_SIZE (python -m torch.distributed.run --nproc-per-node N
    bench.py --gpus N ..., or `--launcher spawn`, which starts the N ranks itself BEFORE any GPU call):  one process per
    GPU, apd_comm_create (ncclCommInitRank) on an id handed over through a rendezvous directory in /tmp, a step =
    apd_batch_refill + apd_align_all_sharded_async; barriers and the max of the elapsed time go through the library's
    own all-gather.  Only if the library's communicator cannot be made does this mode fall back to torch.distributed
    (gloo control plane + nccl all_gather_into_tensor) -- the line then carries "collective_fallback": true and the error.

A step = one full pass of the path over the resident corpus: (features on-device for cfg4 / cfg5,) repack of the
[sum len][D] frames into the kernels' padded layout, fused-pair DTW over each device's pair tiles, ONE all-gather of
the packed tile slabs, unpack into the N x N matrix on rank 0's device.  The pair set is fixed as GPUs are added
(strong scaling).  Timed region: K steps between two fences (every device synchronised, all ranks at a barrier), wall
clock of the slowest rank.

Prints ONE JSON line (rank 0): metric DTW cell-updates/s (whole job), value, unit, ms_per_step, dtype, ... with
  roofline      -- algorithmic bytes (4*D*(n+m)+4 per ordered pair) / kernel time of the timed steps vs 8 TB/s
A plain run does nothing else: set up, warm up, time the K steps, write --dump-outputs if given, print the line.
--full adds the checks and the other measurements, all outside the timed region:
  max_rel_err_vs_oracle, parity_ok -- sampled entries of the matrix against the CPU oracle (--verify)
  cpu_baseline  -- the CPU oracle (a port of the reference's algorithm) timed on a bounded sample (--cpu-seconds)
  parity_census -- default distance form vs the bit-exact strict mode over EVERY matrix entry (--census)
  pcie_inclusive -- the host-buffer entry point (H2D + align + D2H) on the same workload, one call
  secondary     -- measured in the same run on the same context (N = 1, default workload only, --secondary): cfg3_strict (the tolerance-
                   compliant mode on the headline workload: kernel time, roofline fraction, bits against the oracle), cfg4 (through
                   apd_encode) and cfg5s (cfg 5's per-pair shape), each with its own census, and cfg2, cfg1
  clustering    -- percentile + UPGMA on the resident matrix (cfg3 at N = 1 by default, or --cluster): seconds, merges, us / merge,
                   algorithmic bytes / merge and the bandwidth they amount to

--dump-outputs DIR: after the timed steps, the N x N matrix the last step left on rank 0's device, as float32 .npy files
(see dump_outputs); the inputs are seeded, so two builds run with the same arguments can be compared entry for entry.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# BASELINE.json configs: name -> (n_seq, nominal_len, dim, band_pct)
WORKLOADS = {
    "cfg1": dict(n_seq=64, length=256, dim=13, pct=1.0,
                 desc="64 seq len~256 D=13 full DTW (reference CPU-runnable case)"),
    "cfg2": dict(n_seq=1024, length=512, dim=13, pct=0.0625,
                 desc="1024 seq len~512 D=13 MFCC, Sakoe-Chiba band=32"),
    "cfg3": dict(n_seq=4096, length=1024, dim=13, pct=0.0625,
                 desc="4096 seq len~1024 D=13 MFCC, band=64, all-pairs distance matrix"),
    "cfg4": dict(n_seq=4096, length=1024, dim=8, pct=0.0625, encode_from=13,
                 desc="4096 seq len~1024, 13-dim frames -> 8-dim autoencoder embeddings on-device (neural.rs:55-71) -> DTW, band=64"),
}
WORKLOADS["cfg5s"] = dict(n_seq=512, length=2048, dim=13, pct=0.0625,
                          desc="512 seq len~2048 D=13, band=128 (cfg 5's per-pair shape at 1/32 of its sequence count; not a BASELINE config)")
WORKLOADS["cfg5m"] = dict(n_seq=2048, length=2048, dim=13, pct=0.0625,
                          desc="2048 seq len~2048 D=13, band=128 (cfg 5's per-pair shape at 1/8 of its sequence count: 1000 waves per SIMD slot instead of cfg5s' 33; not a BASELINE config)")
WORKLOADS["cfg5e"] = dict(n_seq=256, length=2048, dim=13, pct=0.0625, audio=True,
                          desc="cfg 5's end-to-end data path at 1/64 of its sequence count: 256 recordings x 262400 i16 samples -> on-device "
                               "cepstrum (spectrogram.rs:31-80, dft_win 256, step 128, ceps_filter 18 -> 13 bins) -> DTW band=128 (not a BASELINE config)")
WORKLOADS["cfg5"] = dict(n_seq=16384, length=2048, dim=13, pct=0.0625, audio=True,
                         desc="cfg5: 16384 recordings x 262400 i16 samples -> on-device cepstrum (13 bins) -> DTW band=128 "
                              "(add --full --cluster for the UPGMA leg); ~1 min per step on one GPU")
WORKLOADS["ship"] = dict(n_seq=512, length=525, jitter=375, dim=10, pct=1.0, encode_from=26,
                         desc="the reference's shipped Discovery.toml shape: 512 ragged VAT slices of 150..900 frames, 26-bin cepstra -> "
                              "10-dim autoencoder embeddings on-device -> full DTW (warping_band_percentage = 1.0); not a BASELINE config")
WORKLOADS["wide7"] = dict(n_seq=128, length=4000, dim=13, pct=0.1,
                          desc="128 seq len~4000 D=13, band=400: a binding band wider than one wavefront (dtw_fused_wide; not a BASELINE config)")
WORKLOADS["wide11"] = dict(n_seq=128, length=3000, dim=13, pct=0.4,
                           desc="128 seq len~3000 D=13, band=1200: a binding band of 2400 offsets, 80 % of the sequence (banded strips vs 8-wave band form; not a BASELINE config)")
WORKLOADS["short12"] = dict(n_seq=2048, length=220, jitter=70, dim=10, pct=0.1,
                            desc="2048 short slices of 150..290 frames, D=10, band 10 % (w follows |n-m|): band-form kernels and banded strips mixed (not a BASELINE config)")
WORKLOADS["rag10"] = dict(n_seq=512, length=525, jitter=375, dim=10, pct=0.1,
                          desc="512 ragged slices of 150..900 frames, D=10, band 10 %: w = max(band, |n-m|) + 2 spans every kernel family (not a BASELINE config)")
WORKLOADS["short9"] = dict(n_seq=2048, length=220, jitter=70, dim=10, pct=1.0,
                           desc="2048 short slices of 150..290 frames, D=10, full DTW (the shipped vat_min_len = 150 end of the range; not a BASELINE config)")
WORKLOADS["full8"] = dict(n_seq=96, length=3000, jitter=1000, dim=10, pct=1.0,
                          desc="96 long slices of 2000..4000 frames, D=10, full DTW: several 64*CW-column passes per pair (not a BASELINE config)")
WORKLOADS["full6"] = dict(n_seq=256, length=600, dim=13, pct=1.0,
                          desc="256 seq len~600 D=13, full DTW (the reference's shipped warping_band_percentage = 1.0 on long slices; not a BASELINE config)")
KERNEL_SOURCES = ["dtw_systolic.h", "dtw_common.h", "dtw_full.h", "dtw_wide.h", "dtw_generic.hip", "apd_internal.h", "Makefile"]


def kernel_source_sha():
    """sha256 over the alignment kernels' sources: profiles/hbm_traffic.json records the value its counters were taken at, and
    the bench line carries them only while it still matches (a changed kernel makes them stale, silently otherwise)."""
    import hashlib
    h = hashlib.sha256()
    for name in KERNEL_SOURCES:
        with open(os.path.join(ROOT, "audio_pattern_discovery_amd", "csrc", name), "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def recorded_counters(workload, world):
    """(traffic_bytes, sq_insts_valu, reason-if-absent) from profiles/hbm_traffic.json."""
    try:
        rec = json.load(open(os.path.join(ROOT, "profiles", "hbm_traffic.json"))).get(workload)
    except (OSError, ValueError) as exc:
        return None, None, "profiles/hbm_traffic.json unreadable: %s" % exc
    if not rec:
        return None, None, "no recorded counters for this workload"
    if rec.get("n_gpus") != world:
        return None, None, "the committed PMC passes were taken at %s GPU(s); this run drives %d (rocprofv3 counters of one device do not add up to a launch of another size)" % (rec.get("n_gpus"), world)
    if rec.get("kernel_source_sha") != kernel_source_sha():
        return None, None, "the kernel sources changed since the recorded profile (%s): counters withheld until re-profiled" % rec.get("source", "?")
    return rec["traffic_bytes"], rec.get("sq_insts_valu"), None


HBM_PEAK_GBS = 8000.0      # MI355X_MICROARCH.md: 8.0 TB/s spec
VALU_PEAK = 1024 * 32 * 2.4e9   # lane-instr/s: 1024 SIMDs x 32 lanes x 2.4 GHz (gfx950 SIMDs are 32 lanes wide: 157.3 TFLOP/s f32 / 2)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workload", default=os.environ.get("APD_WORKLOAD", "cfg3"), choices=sorted(WORKLOADS))
    ap.add_argument("--variant", type=int, default=0, help="kernel variant (0 = auto)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also run the checks and other measurements (oracle parity, census, CPU baseline, "
                         "host-buffer path, secondary workloads, clustering); a plain run times the headline only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the distance matrix of the last timed step to DIR/*.npy (float32; a fixed, seeded sample of rows when large)")
    ap.add_argument("--cpu-seconds", type=float, default=12.0, help="--full: CPU baseline budget per leg (0 = skip)")
    ap.add_argument("--verify", type=int, default=64, help="--full: entries re-checked against the oracle after timing")
    ap.add_argument("--distance", default="hybrid", choices=["hybrid", "exact", "strict"], help="local-distance form (apd_set_distance_mode); strict = the reference's arithmetic, bit-identical")
    ap.add_argument("--tau", type=float, default=0.0, help="hybrid recomputation threshold (0 = library default 1/64)")
    ap.add_argument("--cluster", action="store_true", help="--full: also time percentile + UPGMA (rank 0, outside the timed region)")
    ap.add_argument("--launcher", default="auto", choices=["auto", "inprocess", "spawn", "torchrun"],
                    help="auto: one process per GPU if RANK / WORLD_SIZE are set (torchrun), else ONE process driving --gpus devices "
                         "through apd_multi; spawn: start the --gpus ranks from here (before any GPU call)")
    ap.add_argument("--backend", default="apd", choices=["apd", "nccl", "gloo"],
                    help="process-per-GPU mode only.  apd = the library's own RCCL communicator (default); nccl = force the torch.distributed "
                         "fallback; gloo (staged through host memory) only to rehearse N>1 on a box with fewer GPUs")
    ap.add_argument("--census", default="auto", choices=["auto", "on", "off"],
                    help="--full: full-matrix parity census against the bit-exact strict mode after timing (auto: when it costs < ~10 s)")
    ap.add_argument("--secondary", default="auto", choices=["auto", "on", "off"],
                    help="--full: also measure cfg2 and cfg1 in this run (auto: N = 1 and the default cfg3 workload)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if not args.full and (args.cluster or args.census == "on" or args.secondary == "on"):
        ap.error("--cluster, --census on and --secondary on are legs of a --full run")
    return args


def host_threads():
    """CPU threads for the oracle legs: the GPU box grants 16 cores per GPU."""
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    return max(1, min(avail, 16))


def cpu_baseline(frames, offsets, wl, seconds, note=""):
    """Times the CPU oracle (oracle/apd_oracle.c, kind = "port") on a bounded random sample of
    ordered pairs with every host core; returns the JSON object."""
    from oracle import binding as oracle
    cores = host_threads()
    rng = np.random.default_rng(1234)
    n = len(offsets) - 1

    def sample(k):
        pi = rng.integers(0, n, k).astype(np.uint32)
        pj = (pi + 1 + rng.integers(0, n - 1, k)).astype(np.uint32) % n
        return pi, pj

    out = {}
    for name, hm in (("dense", False), ("hashmap", True)):
        pi, pj = sample(cores * 4)
        t0 = time.perf_counter()
        _, cells = oracle.align_sample(frames, offsets, pi, pj, wl["pct"], workers=cores, hashmap=hm)
        dt = max(time.perf_counter() - t0, 1e-6)
        k = int(max(cores * 4, min(seconds / dt * len(pi) * 0.8, 2_000_000)))
        pi, pj = sample(k)
        t0 = time.perf_counter()
        _, cells = oracle.align_sample(frames, offsets, pi, pj, wl["pct"], workers=cores, hashmap=hm)
        dt = time.perf_counter() - t0
        out[name] = (cells / dt, k, dt)
    return {
        "value": out["dense"][0], "unit": "cell-updates/s", "cores": cores, "kind": "port",
        "sample": "%d random ordered pairs of the same workload%s, dense rolling-row oracle, %.1f s"
                  % (out["dense"][1], note, out["dense"][2]),
        "reference_like_value": out["hashmap"][0],
        "reference_like_sample": "%d pairs with the reference's per-pair hash-map cost structure, %.1f s"
                                 % (out["hashmap"][1], out["hashmap"][2]),
    }


# ------------------------------------------------------------------------------------------------- synthetic inputs

def make_inputs(name):
    """Host-side synthetic inputs of a workload: frames or audio, offsets, encoder weights."""
    from audio_pattern_discovery_amd import synth
    wl = WORKLOADS[name]
    n, dim = wl["n_seq"], wl["dim"]
    src_dim = wl.get("encode_from", dim)
    inp = dict(wl=wl, name=name, n=n, dim=dim, src_dim=src_dim, audio=None, frames=None, enc_w=None, enc_b=None, s_off=None)
    if wl.get("audio"):
        rng_a = np.random.default_rng(0xA0D10)
        n_samp = 256 + 128 * wl["length"]
        base = [synth.make_audio(n_samp, seed=1000 + k) for k in range(16)]
        inp["audio"] = [np.clip(base[k % 16].astype(np.int32) + rng_a.integers(-200 * min(k // 16, 40), 200 * min(k // 16, 40) + 1, n_samp, dtype=np.int16),
                                -32768, 32767).astype(np.int16) for k in range(n)]
        inp["s_off"] = np.concatenate([[0], np.cumsum([len(a) for a in inp["audio"]])]).astype(np.uint64)
        offsets = np.zeros(n + 1, dtype=np.uint64)
        offsets[1:] = np.cumsum([(len(a) - 256 + 127) // 128 for a in inp["audio"]])
    else:
        inp["frames"], offsets = synth.make_sequences(n, wl["length"], src_dim, seed=0xA9D0 + sum(map(ord, name)) % 97, jitter=wl.get("jitter"))
    inp["offsets"] = np.ascontiguousarray(offsets, dtype=np.uint64)
    if src_dim != dim:                                               # Mat::seeded-scale random encoder (numerics.rs:178-186)
        rng = np.random.default_rng(0xE1C)
        inp["enc_w"] = ((rng.random((src_dim, dim)) - 0.5) / dim).astype(np.float32)
        inp["enc_b"] = ((rng.random(dim) - 0.5) / dim).astype(np.float32)
    return inp


class DeviceInputs:
    """One device's resident inputs (HBM, through apd_device_alloc) and its feature stage: audio -> cepstra (cfg5),
    13-dim frames -> embeddings (cfg4), or the frames as they are."""

    def __init__(self, ctx, inp):
        from audio_pattern_discovery_amd import _lib
        self._lib, self.L = _lib, _lib.lib()
        self.ctx, self.inp = ctx, inp
        total = int(inp["offsets"][-1])
        self.total = total
        if inp["audio"] is not None:
            self.d_audio = ctx.upload(np.concatenate(inp["audio"]))
            self.d_src = ctx.alloc(total * inp["src_dim"] * 4)
            self.f_off = np.zeros(inp["n"] + 1, dtype=np.uint64)
            self.nb = C.c_uint32(0)
        else:
            self.d_audio = None
            self.d_src = ctx.upload(inp["frames"])
        self.d_frames = self.d_src if inp["enc_w"] is None else ctx.alloc(total * inp["dim"] * 4)
        # the feature stage's resident objects, made once (setup, like AlignmentWorkers::new): a step only enqueues the kernels
        f32p, u64p = C.POINTER(C.c_float), C.POINTER(C.c_uint64)
        self.plan, self.encoder = C.c_void_p(), C.c_void_p()
        if self.d_audio is not None:
            _lib.check(self.L.apd_cepstrum_plan_create(ctx.handle, inp["s_off"].ctypes.data_as(u64p), inp["n"], 256, 128, 18,
                                                       self.f_off.ctypes.data_as(u64p), C.byref(self.nb), C.byref(self.plan)), ctx.handle)
        if inp["enc_w"] is not None:
            _lib.check(self.L.apd_encoder_create(ctx.handle, inp["enc_w"].ctypes.data_as(f32p), inp["enc_b"].ctypes.data_as(f32p),
                                                 inp["src_dim"], inp["dim"], C.byref(self.encoder)), ctx.handle)

    def features(self):
        """Enqueue-only (apd_cepstrum_batch_async / apd_encode_async): called for device after device from one host thread, the
        devices' feature kernels still run concurrently."""
        inp, L, ctx = self.inp, self.L, self.ctx
        if self.d_audio is not None:                                 # NDSequence::new on the whole corpus, in HBM
            self._lib.check(L.apd_cepstrum_batch_async(ctx.handle, self.plan, self.d_audio.at(), self.d_src.at()), ctx.handle)
        if inp["enc_w"] is not None:                                 # NDSequence::encoded on the whole corpus, in HBM
            self._lib.check(L.apd_encode_async(ctx.handle, self.encoder, self.d_src.at(), self.total, self.d_frames.at()), ctx.handle)

    def close(self):
        if self.plan:
            self.L.apd_cepstrum_plan_destroy(self.plan)
            self.plan = C.c_void_p()
        if self.encoder:
            self.L.apd_encoder_destroy(self.encoder)
            self.encoder = C.c_void_p()


def oracle_features(inp, seqs=None):
    """Host frames the CPU legs align: the oracle's encoder output for cfg4-like workloads; for audio workloads the oracle's
    cepstra of the recordings in `seqs` only (returns (frames, offsets, remap))."""
    from oracle import binding as oracle
    if inp["audio"] is not None:
        need = sorted(set(seqs))
        remap = {s_: k for k, s_ in enumerate(need)}
        feats = [oracle.cepstrum(inp["audio"][s_], 256, 128, 18) for s_ in need]
        return np.concatenate(feats), np.concatenate([[0], np.cumsum([len(f) for f in feats])]).astype(np.uint64), remap
    frames = inp["frames"] if inp["enc_w"] is None else oracle.encode(inp["frames"], inp["enc_w"], inp["enc_b"])
    return frames, inp["offsets"], None


def verify_sample(inp, result, k, seed=7):
    """max relative error of k random entries of `result` against the CPU oracle."""
    from oracle import binding as oracle
    n = inp["n"]
    rng = np.random.default_rng(seed)
    pi = rng.integers(0, n, k).astype(np.uint32)
    pj = (pi + 1 + rng.integers(0, n - 1, k)).astype(np.uint32) % n
    frames, offsets, remap = oracle_features(inp, pi.tolist() + pj.tolist())
    qi, qj = (pi, pj) if remap is None else (np.array([remap[v] for v in pi.tolist()], np.uint32), np.array([remap[v] for v in pj.tolist()], np.uint32))
    want, _ = oracle.align_sample(frames, offsets, qi, qj, inp["wl"]["pct"], workers=host_threads())
    return float(np.max(np.abs(result[pi, pj] - want) / np.maximum(np.abs(want), 1e-30)))


def census(default, strict):
    """Default-mode matrix against the strict-mode matrix (bit-identical to the CPU arithmetic) over EVERY entry."""
    fin_d, fin_s = np.isfinite(default), np.isfinite(strict)
    both = fin_d & fin_s & (strict != 0)
    rel = np.abs(default[both] - strict[both]) / np.abs(strict[both])
    over = rel > 1e-4
    out = {"entries": int(default.size), "max_rel": float(rel.max()) if rel.size else 0.0, "over_1e-4": int(over.sum()),
           "nonfinite_pattern_equal": bool(np.array_equal(fin_d, fin_s) and np.array_equal(np.isnan(default), np.isnan(strict))
                                           and np.array_equal(default[~fin_d & ~np.isnan(default)], strict[~fin_s & ~np.isnan(strict)])),
           "zero_pattern_equal": bool(np.array_equal(default == 0, strict == 0)),
           "bitwise_equal": int((default.view(np.uint32) == strict.view(np.uint32)).sum()),
           "reference": "apd_set_distance_mode(2): operation-for-operation arithmetic of numerics.rs:114-120 / alignments.rs:129-160, "
                        "bit-identical to the CPU oracle (tests/test_gpu_fuzz.py); oracle-anchored by max_rel_err_vs_oracle on the sampled entries"}
    if over.any():
        flat = int(np.flatnonzero(both)[int(np.argmax(rel))])
        out["worst_entry"] = [flat // default.shape[1], flat % default.shape[1]]
    return out


DUMP_MATRIX_BYTES = 32 << 20      # --dump-outputs: whole rows of the matrix up to this size (the limit is 64 MB in all)
DUMP_SEED = 0xD0A1


def dump_outputs(out_dir, result):
    """--dump-outputs: what a caller of the timed path receives, the N x N distance matrix, as
      distances.npy      float32 [k][N]  -- the whole matrix (k = N) while it fits in DUMP_MATRIX_BYTES, else k whole rows
      distance_rows.npy  float64 [k]     -- the row numbers, ascending; drawn with a fixed seed, so the same rows in every run."""
    os.makedirs(out_dir, exist_ok=True)
    n = result.shape[0]
    k = max(1, min(n, DUMP_MATRIX_BYTES // (4 * n)))
    rows = np.arange(n) if k == n else np.sort(np.random.default_rng(DUMP_SEED).choice(n, k, replace=False))
    np.save(os.path.join(out_dir, "distances.npy"), np.ascontiguousarray(result[rows], dtype=np.float32))
    np.save(os.path.join(out_dir, "distance_rows.npy"), rows.astype(np.float64))


# ------------------------------------------------------------------------------------------------- control planes

class FileRendezvous:
    """Hands small blobs between the ranks of one node through a directory in /tmp (no torch, no sockets): named by the
    launcher's port and the identity of the common parent process, so concurrent or stale runs cannot meet."""

    def __init__(self, rank, world):
        ppid = os.getppid()
        try:
            start = open("/proc/%d/stat" % ppid).read().rsplit(")", 1)[1].split()[19]
        except (OSError, IndexError):
            start = "0"
        tag = "%s_%s_%d_%s" % (os.environ.get("MASTER_PORT", "0"), os.environ.get("TORCHELASTIC_RUN_ID", "none"), ppid, start)
        self.dir = os.path.join(os.environ.get("APD_RDZV_DIR", "/tmp"), "apd_bench_rdzv_" + "".join(c if c.isalnum() or c in "_-" else "_" for c in tag))
        self.rank, self.world = rank, world
        os.makedirs(self.dir, exist_ok=True)

    def put(self, name, blob):
        tmp = os.path.join(self.dir, ".%s.%d" % (name, self.rank))
        with open(tmp, "wb") as f:
            f.write(blob)
        os.replace(tmp, os.path.join(self.dir, name))

    def get(self, name, timeout=300.0):
        path, t0 = os.path.join(self.dir, name), time.time()
        while not os.path.exists(path):
            if time.time() - t0 > timeout:
                raise TimeoutError("rendezvous: %s never appeared in %s" % (name, self.dir))
            time.sleep(0.01)
        return open(path, "rb").read()

    def gather_status(self, text, tag="status", timeout=300.0):
        """Every rank posts a line; returns all of them in rank order (a barrier on the host side)."""
        self.put("%s.%d" % (tag, self.rank), text.encode())
        return [self.get("%s.%d" % (tag, r), timeout).decode() for r in range(self.world)]

    def finish(self):
        """Every rank has passed its last use of the directory: rank 0 waits for all of them, then removes it."""
        self.put("done.%d" % self.rank, b"")
        if self.rank == 0:
            import shutil
            for r in range(self.world):
                self.get("done.%d" % r)
            shutil.rmtree(self.dir, ignore_errors=True)


class DeviceView:
    """A library-owned device buffer seen through __cuda_array_interface__ (torch fallback path only)."""

    def __init__(self, ptr, count):
        self.__cuda_array_interface__ = {"shape": (int(count),), "typestr": "<f4", "data": (int(ptr), False), "version": 2}


# ------------------------------------------------------------------------------------------------- secondary workloads

def strict_bits_vs_oracle(inp, strict, k=32, seed=11, device_frames=None):
    """How many of k sampled entries of the strict-mode matrix carry exactly the CPU oracle's bits (all of them must).
    device_frames: the features the GPU aligned, read back -- for workloads whose features are made on the device (cfg4: the
    encoder's expf is within an ulp of the CPU's, not equal to it), so that the alignment is compared on identical inputs."""
    from oracle import binding as oracle
    n = inp["n"]
    rng = np.random.default_rng(seed)
    pi = rng.integers(0, n, k).astype(np.uint32)
    pj = (pi + 1 + rng.integers(0, n - 1, k)).astype(np.uint32) % n
    frames, offsets, remap = (device_frames, inp["offsets"], None) if device_frames is not None else oracle_features(inp, pi.tolist() + pj.tolist())
    qi, qj = (pi, pj) if remap is None else (np.array([remap[v] for v in pi.tolist()], np.uint32), np.array([remap[v] for v in pj.tolist()], np.uint32))
    want, _ = oracle.align_sample(frames, offsets, qi, qj, inp["wl"]["pct"], workers=host_threads())
    return int((strict[pi, pj].view(np.uint32) == want.view(np.uint32)).sum()), int(k)


def measure_secondary(ctx, name, steps=5, with_census=False):
    """Another BASELINE configuration measured on the same context in the same run: resident inputs, `steps` timed
    steps ((features +) repack + alignment + unpack), kernel time from HIP events, parity against the oracle on sampled entries;
    with_census: one more pass in strict mode (bit-identical to the CPU arithmetic) and the default matrix against it, entry by entry."""
    from audio_pattern_discovery_amd import _lib
    from audio_pattern_discovery_amd.alignments import align_work
    L = _lib.lib()
    inp = make_inputs(name)
    wl, n, dim = inp["wl"], inp["n"], inp["dim"]
    cfg = _lib.AlignConfig(wl["pct"], 1.0, 1.0, 1.0)
    pairs, cells, alg_bytes = align_work(inp["offsets"], dim, cfg, 0, 1)
    dev = DeviceInputs(ctx, inp)
    d_out = ctx.alloc(n * n * 4)
    batch = C.c_void_p()
    u64p = C.POINTER(C.c_uint64)
    dev.features()
    _lib.check(L.apd_batch_create(ctx.handle, dev.d_frames.at(), inp["offsets"].ctypes.data_as(u64p), n, dim, 1, C.byref(batch)), ctx.handle)

    def step():
        dev.features()
        _lib.check(L.apd_batch_refill(ctx.handle, batch, dev.d_frames.at(), 1), ctx.handle)
        _lib.check(L.apd_align_all_device_async(ctx.handle, batch, C.byref(cfg), d_out.at()), ctx.handle)

    step()
    ctx.synchronize()
    kernel_ms = []
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
        kernel_ms.append(ctx.last_kernel_ms())
    ctx.synchronize()
    elapsed = time.perf_counter() - t0
    result = d_out.to_numpy(np.float32).reshape(n, n)
    k_ms = float(np.mean(kernel_ms))
    err = verify_sample(inp, result, 64 if inp["audio"] is None else 16)
    tol = 1e-3 if inp["audio"] is not None else 1e-4                # audio: the cepstra themselves are f32 FFTs against an f64 oracle
    achieved = alg_bytes / (k_ms * 1e-3) / 1e9
    out = {"workload": "%s: %s" % (name, wl["desc"]), "steps": steps, "ms_per_step": elapsed / steps * 1e3, "value": cells * steps / elapsed,
           "unit": "cell-updates/s", "kernel_ms": k_ms, "kernel_cells_per_s": cells / (k_ms * 1e-3), "alg_bytes_per_launch": alg_bytes,
           "roofline_achieved_GBs": achieved, "roofline_frac": achieved / HBM_PEAK_GBS, "max_rel_err_vs_oracle": err, "parity_ok": bool(err <= tol)}
    if with_census:
        ctx.set_distance_mode("strict")
        _lib.check(L.apd_align_all_device_async(ctx.handle, batch, C.byref(cfg), d_out.at()), ctx.handle)
        s_ms = ctx.last_kernel_ms()
        ctx.synchronize()
        ctx.set_distance_mode("hybrid")
        strict = d_out.to_numpy(np.float32).reshape(n, n)
        out["parity_census"] = census(result, strict)
        dev_frames = dev.d_frames.to_numpy(np.float32).reshape(-1, dim) if (inp["enc_w"] is not None or inp["audio"] is not None) else None
        same, of = strict_bits_vs_oracle(inp, strict, device_frames=dev_frames)
        out["strict"] = {"kernel_ms": s_ms, "roofline_frac": alg_bytes / (s_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                         "bitwise_equal_to_oracle_sample": "%d of %d" % (same, of),
                         "oracle_inputs": "the device's own features, read back" if dev_frames is not None else "the host frames"}
        out["parity_ok"] = bool(out["parity_ok"] and out["parity_census"]["nonfinite_pattern_equal"] and out["parity_census"]["zero_pattern_equal"]
                                and same == of)
    L.apd_batch_destroy(batch)
    dev.close()
    return out


def clustering_leg(ctx, d_out, n, perc=0.05):
    """percentile + UPGMA on the resident matrix (clustering.rs:81-110), outside the timed region.  bytes_per_merge is the
    ALGORITHMIC traffic of the merges made: re-summing the new cluster's row and column of the cluster-sum matrix reads every
    raw distance between its |Ck| members and the other n - |Ck| instances once per direction (2 |Ck| (n - |Ck|) floats), writes
    the 2 (live - 1) sums, and the arg-min streams the live row minima once."""
    from audio_pattern_discovery_amd import _lib
    L = _lib.lib()
    ops = (_lib.ClusterOp * n)()
    roots = np.zeros(n, dtype=np.uint32)
    n_ops, n_roots, thr = C.c_uint32(0), C.c_uint32(0), C.c_float(0)
    t0 = time.perf_counter()
    _lib.check(L.apd_clustering(ctx.handle, d_out.at(), 1, n, perc, ops, C.byref(n_ops),
                                roots.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(n_roots), C.byref(thr)), ctx.handle)
    dt = time.perf_counter() - t0
    m = int(n_ops.value)
    size = {}
    total_bytes = 0
    for t in range(m):
        k = size.get(ops[t].merge_i, 1) + size.get(ops[t].merge_j, 1)
        size[ops[t].into] = k
        live = n - t - 1
        total_bytes += 4 * (2 * k * (n - k) + 2 * max(live - 1, 0) + live)
    return {"seconds": dt, "merges": m, "roots": int(n_roots.value), "threshold": float(thr.value), "percentile": perc,
            "us_per_merge": dt / max(m, 1) * 1e6, "bytes_per_merge": total_bytes / max(m, 1),
            "achieved_GBs": total_bytes / dt / 1e9, "hbm_frac": total_bytes / dt / 1e9 / HBM_PEAK_GBS,
            "note": "apd_clustering on the resident matrix: radix-select threshold (4 passes over n^2 floats, included in `seconds`) + UPGMA, two or three "
                    "launches per merge (the segment launches are left out of the replayed graph while no merge needs them); bound by launch boundaries "
                    "and dependent gathers, not by bandwidth: see DESIGN.md section 4.3"}


# ------------------------------------------------------------------------------------------------- launch modes

def spawn_ranks(args):
    """--launcher spawn: start the N ranks from here, BEFORE this process makes any GPU call; forward rank 0's line."""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    argv = [a for a in sys.argv[1:]]
    for k, a in enumerate(argv):
        if a == "--launcher":
            argv[k + 1] = "auto"
        elif a.startswith("--launcher="):
            argv[k] = "--launcher=auto"
    procs = []
    for r in range(args.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(args.gpus), LOCAL_WORLD_SIZE=str(args.gpus),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv, env=env))
    rc = 0
    for p in procs:
        rc = p.wait() or rc
    raise SystemExit(rc)


def main():
    args = parse()
    env_world = int(os.environ.get("WORLD_SIZE", "0") or 0)
    under_launcher = "RANK" in os.environ and env_world >= 1
    if args.launcher == "spawn" and not under_launcher and args.gpus > 1:
        spawn_ranks(args)
    if args.launcher == "torchrun" and not under_launcher and args.gpus > 1:
        raise SystemExit("--launcher torchrun: start me with `python -m torch.distributed.run --nproc-per-node %d bench.py ...`" % args.gpus)
    ranks_mode = under_launcher and env_world > 1 and args.launcher != "inprocess"
    rank = int(os.environ.get("RANK", "0")) if ranks_mode else 0
    local_rank = int(os.environ.get("LOCAL_RANK", "0")) if ranks_mode else 0
    world = env_world if ranks_mode else max(args.gpus, 1)
    multi_mode = (not ranks_mode) and (world > 1 or os.environ.get("APD_BENCH_FORCE_MULTI") == "1")   # the env: the handle's path at one device (1-GPU boxes)
    args.gpus = world

    from audio_pattern_discovery_amd import _lib, sharding
    from audio_pattern_discovery_amd.alignments import align_work
    L = _lib.lib()
    f32p, u64p = C.POINTER(C.c_float), C.POINTER(C.c_uint64)

    inp = make_inputs(args.workload)
    wl, n, dim = inp["wl"], inp["n"], inp["dim"]
    offsets = inp["offsets"]
    cfg = _lib.AlignConfig(wl["pct"], 1.0, 1.0, 1.0)
    pairs_all, cells_all, bytes_all = align_work(offsets, dim, cfg, 0, 1)
    pairs_r, cells_r, bytes_r = align_work(offsets, dim, cfg, rank, world)

    # ---- devices, contexts, communicator --------------------------------------------------------------------------
    multi = comm = rdzv = None
    collective, collective_fallback, collective_error, ranks_seen = "none (1 rank)", False, None, 1
    dist = torch = nccl_group = None
    if multi_mode:
        # APD_BENCH_DEVICES=0,0,0,0 (with APD_MULTI_COLLECTIVE=peer): rehearse N ranks of the handle on ONE GPU; not a measurement
        dev_list = [int(v) for v in os.environ["APD_BENCH_DEVICES"].split(",")] if os.environ.get("APD_BENCH_DEVICES") else list(range(world))
        if len(dev_list) != world:
            raise SystemExit("APD_BENCH_DEVICES must name --gpus devices")
        multi = sharding.Multi(dev_list)
        ctxs = multi.contexts
        collective, ranks_seen = "apd_multi: " + multi.collective(), multi.ranks_seen()
        collective_fallback = multi.collective().startswith("peer-copy")
        if collective_fallback:
            collective_error = multi.collective()
            sys.stderr.write("[bench] %s\n" % collective_error)
    else:
        dev_index = int(os.environ.get("APD_FORCE_DEVICE", local_rank))  # rehearsal: several ranks on one GPU
        ctxs = [_lib.Context(dev_index)]
    ctx = ctxs[0]
    for c in ctxs:
        c.selftest()
        c.set_variant(args.variant)
        c.set_distance_mode(args.distance, args.tau)
        c.set_timing(True)
    devs = [DeviceInputs(c, inp) for c in ctxs]                      # inputs resident in HBM (every device holds the corpus)
    d_out = ctx.alloc(n * n * 4)
    slab_floats = int(L.apd_slab_floats(n, world))

    if ranks_mode:
        rdzv = FileRendezvous(rank, world)
        err = ""
        if args.backend == "apd":
            try:
                if rank == 0:
                    rdzv.put("id", sharding.Comm.unique_id())
                comm = sharding.Comm(ctx, rdzv.get("id"), rank, world)   # ncclCommInitRank: collective over the ranks
                ranks_seen = comm.count()
                # one small all-gather now: RCCL sets its channels up on first use, which must not land in a timed step (--warmup 0)
                warm_src, warm_dst = ctx.upload(np.full(256, float(rank), np.float32)), ctx.alloc(256 * world * 4)
                _lib.check(L.apd_all_gather_async(ctx.handle, comm.handle, warm_src.at(), warm_dst.at(), 256), ctx.handle)
                ctx.synchronize()
                if not np.array_equal(warm_dst.to_numpy(np.float32).reshape(world, 256)[:, 0], np.arange(world, dtype=np.float32)):
                    raise RuntimeError("all-gather returned the slabs out of rank order")
            except Exception as exc:                                     # noqa: BLE001 -- any failure: agree on the fallback
                err = "rank %d: %s: %s" % (rank, type(exc).__name__, exc)
                sys.stderr.write("[bench] library communicator failed (%s); falling back to torch.distributed\n" % err)
        else:
            err = "forced by --backend %s" % args.backend
        status = rdzv.gather_status(err)
        if any(status):
            collective_fallback = args.backend == "apd"
            collective_error = "; ".join(s for s in status if s)
            if comm is not None:
                comm.close()
                comm = None
            import torch                                                 # fallback only: control plane + collective from torch
            import torch.distributed as dist
            dist.init_process_group("gloo", rank=rank, world_size=world)
            if args.backend != "gloo":
                torch.cuda.set_device(dev_index)
                nccl_group = dist.new_group(backend="nccl", device_id=torch.device("cuda", dev_index))
                collective, ranks_seen = "torch.distributed all_gather_into_tensor (nccl = RCCL)", dist.get_world_size(nccl_group)
            else:
                collective = "gloo through host memory (rehearsal only)"
            d_slab, d_gathered = ctx.alloc(slab_floats * 4), ctx.alloc(slab_floats * world * 4)
            if nccl_group is not None:
                t_slab = torch.as_tensor(DeviceView(d_slab.ptr, slab_floats), device="cuda")
                t_gathered = torch.as_tensor(DeviceView(d_gathered.ptr, slab_floats * world), device="cuda")
        else:
            collective = "apd_comm: library-owned RCCL communicator (ncclCommInitRank), ncclAllGather inside apd_align_all_sharded_async"
        gather_one, gather_src = (ctx.alloc(4 * world), ctx.alloc(4)) if comm is not None else (None, None)

    def all_ranks(value):
        """Every rank's float, in rank order (also a barrier).  Library all-gather; torch only in the fallback."""
        if not ranks_mode:
            return [value]
        if comm is not None:
            gather_src.copy_from(np.array([value], np.float32))
            _lib.check(L.apd_all_gather_async(ctx.handle, comm.handle, gather_src.at(), gather_one.at(), 1), ctx.handle)
            ctx.synchronize()
            return gather_one.to_numpy(np.float32).astype(np.float64).tolist()
        t = torch.zeros(world, dtype=torch.float64)
        t[rank] = value
        dist.all_reduce(t)
        return t.tolist()

    # ---- prime: code objects loaded on every device, RCCL channels set up -- none of that may land in a timed step when the
    # driver passes --warmup 0 (a 32-sequence toy batch through the same entry points; part of setup, like AlignmentWorkers::new)
    from audio_pattern_discovery_amd import synth as _synth
    toy_n = 64
    toy_frames, toy_off = _synth.make_sequences(toy_n, 48, dim, seed=1)
    toy_cfg = _lib.AlignConfig(wl["pct"], 1.0, 1.0, 1.0)
    toy_off64 = np.ascontiguousarray(toy_off, np.uint64)
    multi_selfcheck = None                                           # N > 1: the same batch on N devices and on device 0 alone, compared bitwise

    def single_device_toy(c):
        h, out = C.c_void_p(), np.empty(toy_n * toy_n, dtype=np.float32)
        _lib.check(L.apd_batch_create(c.handle, toy_frames.ctypes.data_as(f32p), toy_off64.ctypes.data_as(u64p), toy_n, dim, 0, C.byref(h)), c.handle)
        _lib.check(L.apd_align_all(c.handle, h, C.byref(toy_cfg), out.ctypes.data_as(f32p)), c.handle)
        L.apd_batch_destroy(h)
        return out.reshape(toy_n, toy_n)

    if multi_mode:
        toy = multi.batch(toy_off, dim, frames=toy_frames)
        toy_multi = multi.align_all(toy, toy_cfg)
        toy.close()
        if world > 1:
            multi_selfcheck = "bitwise" if np.array_equal(toy_multi.view(np.uint32), single_device_toy(ctx).view(np.uint32)) else "MISMATCH"
    else:
        toy = C.c_void_p()
        toy_out = ctx.alloc(toy_n * toy_n * 4)
        _lib.check(L.apd_batch_create(ctx.handle, toy_frames.ctypes.data_as(f32p), toy_off64.ctypes.data_as(u64p), toy_n, dim, 0,
                                      C.byref(toy)), ctx.handle)
        if comm is not None or world == 1:
            _lib.check(L.apd_align_all_sharded_async(ctx.handle, comm.handle if comm is not None else None, toy, C.byref(toy_cfg), toy_out.at()), ctx.handle)
        else:
            _lib.check(L.apd_align_tiles_async(ctx.handle, toy, C.byref(toy_cfg), rank, world, d_slab.at()), ctx.handle)
        ctx.synchronize()
        L.apd_batch_destroy(toy)
        if comm is not None and world > 1 and rank == 0:
            multi_selfcheck = "bitwise" if np.array_equal(toy_out.to_numpy(np.float32).view(np.uint32), single_device_toy(ctx).ravel().view(np.uint32)) else "MISMATCH"
    if multi_selfcheck == "MISMATCH":
        sys.stderr.write("[bench] multi-GPU self-check FAILED: %d devices and device 0 alone disagree on a %d-sequence batch\n" % (world, toy_n))
        raise SystemExit(3)

    # ---- the step ---------------------------------------------------------------------------------------------------
    batch = C.c_void_p()
    mbatch = None

    def make_batch():
        nonlocal mbatch
        if multi_mode:
            mbatch = multi.batch(offsets, dim, d_frames=[d.d_frames.ptr for d in devs])
        else:
            _lib.check(L.apd_batch_create(ctx.handle, devs[0].d_frames.at(), offsets.ctypes.data_as(u64p), n, dim, 1, C.byref(batch)), ctx.handle)

    def step():
        for d in devs:
            d.features()
        if multi_mode:
            if mbatch is None:
                make_batch()
            else:
                mbatch.refill(d_frames=[d.d_frames.ptr for d in devs])
            multi.align_all_async(mbatch, cfg, d_out.ptr)
            return
        if not batch:                                                # AlignmentWorkers::new once; later steps refill the resident copy
            make_batch()
        else:
            _lib.check(L.apd_batch_refill(ctx.handle, batch, devs[0].d_frames.at(), 1), ctx.handle)
        if comm is not None or world == 1:
            # tiles of this rank + the one ncclAllGather (RCCL over xGMI) + unpack, all inside the library
            _lib.check(L.apd_align_all_sharded_async(ctx.handle, comm.handle if comm is not None else None, batch, C.byref(cfg), d_out.at()), ctx.handle)
            return
        _lib.check(L.apd_align_tiles_async(ctx.handle, batch, C.byref(cfg), rank, world, d_slab.at()), ctx.handle)   # torch fallback
        ctx.synchronize()
        if nccl_group is not None:
            dist.all_gather_into_tensor(t_gathered, t_slab, group=nccl_group)
            torch.cuda.synchronize()
        else:
            host = torch.empty(slab_floats * world, dtype=torch.float32)
            dist.all_gather_into_tensor(host, torch.from_numpy(d_slab.to_numpy(np.float32)))
            d_gathered.copy_from(host.numpy())
        _lib.check(L.apd_unpack_tiles_async(ctx.handle, batch, world, d_gathered.at(), d_out.at()), ctx.handle)

    def fence():
        if multi_mode:
            multi.synchronize()                                      # every device; raises APD_ERR_INCOMPLETE if an unpack met an unwritten score
            return
        ctx.synchronize()
        if ranks_mode:
            all_ranks(0.0)                                           # barrier
            ctx.synchronize()

    for _ in range(max(args.warmup, 0)):
        step()
    if not batch and mbatch is None:                                 # --warmup 0: AlignmentWorkers::new is not part of a step
        for d in devs:
            d.features()
        make_batch()
    kernel_ms = []
    fence()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
        kernel_ms.append(ctx.last_kernel_ms())                       # syncs on the kernel's end event only
    fence()
    elapsed = time.perf_counter() - t0
    elapsed = max(all_ranks(elapsed))

    result = d_out.to_numpy(np.float32).reshape(n, n) if rank == 0 and (args.full or args.dump_outputs) else None
    if result is not None and args.dump_outputs:
        dump_outputs(args.dump_outputs, result)
    # ---- --full from here on.  Parity census: the default distance form against strict mode (bit-identical to the CPU arithmetic)
    # over EVERY entry, on the same resident batch, after the timed region; every rank takes part (the strict run is sharded like a step)
    strict, census_seconds, strict_kernel_ms = None, 0.0, None
    want_census = args.full and (args.census == "on" or (args.census == "auto" and args.distance != "strict" and cells_all <= 3e12))
    if want_census and (multi_mode or comm is not None or world == 1):
        t0 = time.perf_counter()
        for c in ctxs:
            c.set_distance_mode("strict")
        if multi_mode:
            multi.align_all_async(mbatch, cfg, d_out.ptr)
        else:
            _lib.check(L.apd_align_all_sharded_async(ctx.handle, comm.handle if comm is not None else None, batch, C.byref(cfg), d_out.at()), ctx.handle)
        strict_kernel_ms = ctx.last_kernel_ms()
        fence()
        for c in ctxs:
            c.set_distance_mode(args.distance, args.tau)
        if rank == 0:
            strict = d_out.to_numpy(np.float32).reshape(n, n)
            d_out.copy_from(result.ravel())                          # leave the default-mode matrix resident (the UPGMA leg reads it)
        census_seconds = time.perf_counter() - t0

    if rank == 0:
        traffic, valu_insts, counters_withheld = recorded_counters(args.workload, world) if args.distance == "hybrid" else (None, None, "recorded for the default distance form only")
        k_ms = float(np.mean(kernel_ms))
        achieved = bytes_r / (k_ms * 1e-3) / 1e9
        mode = ("one process driving %d devices (apd_multi)" % world if multi_mode else
                "one process per GPU (%s)" % ("torchrun / env ranks" if ranks_mode else "single device"))
        line = {
            "metric": "DTW cell-updates/sec (whole node)", "value": cells_all * args.steps / elapsed,
            "unit": "cell-updates/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "strong",
            "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": "%s: %s" % (args.workload, wl["desc"]), "n_seq": n, "nominal_len": wl["length"],
                       "dim": dim, "warping_band_percentage": wl["pct"], "ordered_pairs": pairs_all,
                       "cells_per_step": cells_all, "sharding": "pair tiles 16x16, cyclic over %d ranks, 1 all-gather" % world,
                       "launch": mode, "collective": collective, "collective_fallback": collective_fallback,
                       "collective_error": collective_error, "ranks_seen": ranks_seen, "multi_selfcheck": multi_selfcheck,
                       "runtime": _lib.runtime_info(), "torch_imported": "torch" in sys.modules,
                       "kernel_variant": args.variant, "distance_form": args.distance, "full": args.full},
            "wall_clock_matrix_s": elapsed / args.steps,
            "pairs_per_s": pairs_all * args.steps / elapsed,
            "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBS, "traffic": traffic,
                         "traffic_withheld": counters_withheld,
                         "traffic_source": None if traffic is None else
                         "profiles/hbm_traffic.json: rocprofv3 --pmc FETCH_SIZE (x2, gfx950) + WRITE_SIZE of this command, committed; "
                         "a recorded constant, not re-measured in this run",
                         "note": "rows n / columns m of every pair are not swept (score() reads cell (n-1, m-1), alignments.rs:120): "
                                 "the kernel touches ~0.2 % fewer cells than `value` counts; `value` counts the reference's cells",
                         "kernel": "dtw_fused (rank 0 share: %d ordered pairs)" % pairs_r,
                         "kernel_ms": k_ms, "alg_bytes_per_launch": bytes_r,
                         "kernel_cells_per_s": cells_r / (k_ms * 1e-3)},
            # the kernel is VALU-bound, so the HBM fraction above is reported next to the vector-issue figure:
            # lane-instructions per cell from the SQ_INSTS_VALU counter of this workload, times the live cell rate, over VALU_PEAK
            "valu": None if not valu_insts else {
                "lane_instr_per_cell": valu_insts * 64.0 / cells_r,
                "lane_instr_per_s": valu_insts * 64.0 / (k_ms * 1e-3),
                "peak_lane_instr_per_s": VALU_PEAK,
                "frac": valu_insts * 64.0 / (k_ms * 1e-3) / VALU_PEAK,
                "source": "profiles/hbm_traffic.json (rocprofv3 --pmc SQ_INSTS_VALU of this command, committed; not re-measured in this run)"},
        }
        if args.full:
            verify = verify_sample(inp, result, args.verify) if args.verify > 0 else None
            line["max_rel_err_vs_oracle"] = verify
            line["parity_ok"] = (verify is None) or bool(verify <= (1e-3 if inp["audio"] is not None else 1e-4))
        if strict is not None:                                       # --full only
            line["parity_census"] = census(result, strict)
            line["parity_census"]["seconds"] = census_seconds
            line["parity_census"]["strict_max_rel_err_vs_oracle"] = verify_sample(inp, strict, min(args.verify, 32), seed=11) if args.verify > 0 else None
            line["parity_ok"] = bool(line["parity_ok"] and line["parity_census"]["over_1e-4"] == 0 and
                                     line["parity_census"]["nonfinite_pattern_equal"] and line["parity_census"]["zero_pattern_equal"])
            if line["parity_census"]["over_1e-4"]:
                line["parity_note"] = ("%d of %d entries beyond 1e-4 in the default distance form: the coincidental-tie deviation (DESIGN.md section 6, "
                                       "1-6 entries in 1e8 on the BASELINE shapes); --distance strict computes the reference's bits at 1.9x the time (secondary.cfg3_strict)"
                                       % (line["parity_census"]["over_1e-4"], line["parity_census"]["entries"]))
        if args.full and inp["frames"] is not None and inp["enc_w"] is None and world == 1:
            # the host-buffer entry of the boundary (AlignmentWorkers::new + align_all on host Vec<f32>s): H2D of the frames,
            # repack, kernel, unpack, D2H of the matrix -- reported beside `value`, never as it
            host_out = np.empty(n * n, dtype=np.float32)
            hb = C.c_void_p()
            t0 = time.perf_counter()
            _lib.check(L.apd_batch_create(ctx.handle, inp["frames"].ctypes.data_as(f32p), offsets.ctypes.data_as(u64p), n, dim, 0, C.byref(hb)), ctx.handle)
            _lib.check(L.apd_align_all(ctx.handle, hb, C.byref(cfg), host_out.ctypes.data_as(f32p)), ctx.handle)
            dt = time.perf_counter() - t0
            L.apd_batch_destroy(hb)
            line["pcie_inclusive"] = {"seconds": dt, "value": cells_all / dt, "unit": "cell-updates/s",
                                      "h2d_bytes": int(inp["frames"].nbytes), "d2h_bytes": int(host_out.nbytes),
                                      "bitwise_equal_to_resident_path": bool(np.array_equal(host_out.reshape(n, n), result)),
                                      "note": "apd_batch_create(host frames) + apd_align_all(host out), pageable host memory, one call"}
        want_cluster = args.full and (args.cluster or (world == 1 and args.workload == "cfg3" and args.secondary != "off"))
        if want_cluster:
            line["clustering"] = clustering_leg(ctx, d_out, n)
        if args.full and world == 1 and (args.secondary == "on" or (args.secondary == "auto" and args.workload == "cfg3")):
            sec = {}
            if strict is not None and args.workload == "cfg3":
                # the tolerance-compliant mode on the headline workload: the census pass above IS a full strict-mode alignment
                same, of = strict_bits_vs_oracle(inp, strict)
                sec["cfg3_strict"] = {"workload": "cfg3 in apd_set_distance_mode(2): the reference's arithmetic operation for operation", "kernel_ms": strict_kernel_ms,
                                      "kernel_cells_per_s": cells_r / (strict_kernel_ms * 1e-3), "roofline_achieved_GBs": bytes_r / (strict_kernel_ms * 1e-3) / 1e9,
                                      "roofline_frac": bytes_r / (strict_kernel_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, "x_default_kernel": strict_kernel_ms / k_ms,
                                      "bitwise_equal_to_oracle_sample": "%d of %d" % (same, of), "parity_ok": bool(same == of)}
            sec["cfg4"] = measure_secondary(ctx, "cfg4", steps=3, with_census=True)
            sec["cfg5s"] = measure_secondary(ctx, "cfg5s", steps=5, with_census=True)
            sec["cfg2"] = measure_secondary(ctx, "cfg2")
            sec["cfg1"] = measure_secondary(ctx, "cfg1")
            line["secondary"] = sec
        if args.full and args.cpu_seconds > 0:
            if inp["audio"] is None:
                line["cpu_baseline"] = cpu_baseline(oracle_features(inp)[0], offsets, wl, args.cpu_seconds)
            else:
                # audio workloads: the CPU legs align the oracle's own cepstra of a subset of the recordings (the whole corpus' would take minutes)
                subset = list(range(0, n, max(n // 48, 1)))[:48]
                fr, off, _ = oracle_features(inp, subset)
                line["cpu_baseline"] = cpu_baseline(fr, off, wl, args.cpu_seconds, note=" among %d of the %d recordings (oracle cepstra)" % (len(subset), n))
        elif args.full:
            line["cpu_baseline"] = None
        print(json.dumps(line), flush=True)
    if ranks_mode:
        all_ranks(0.0)                                               # nobody tears the communicator down while rank 0 still works
    if batch:
        L.apd_batch_destroy(batch)
    if mbatch is not None:
        mbatch.close()
    for d in devs:
        d.close()
    if comm is not None:
        comm.close()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    if rdzv is not None:
        rdzv.finish()
    if multi is not None:
        multi.close()


if __name__ == "__main__":
    main()
