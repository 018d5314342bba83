"""Host mirror of src/alignments.rs (+ the NDSequence container of src/spectrogram.rs:13-24,99-101,
152-154) over the C ABI of include/apd.h.  Names, argument meaning and error behaviour follow the
Rust items; the compute is the HIP library, never Python."""
import contextlib
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib


class NDSequence:
    """spectrogram.rs:13-24: flat row-major frames `[T][n_bins]` plus n_bins."""

    def __init__(self, frames, n_bins=None, audio_id=0):
        a = np.ascontiguousarray(frames, dtype=np.float32)
        if a.ndim == 1:
            if not n_bins:
                raise ValueError("n_bins required for flat frames")
            a = a.reshape(-1, n_bins)
        self.frames = a
        self.n_bins = int(a.shape[1])
        self.audio_id = audio_id

    @staticmethod
    def new(fft_size, fft_step, filter_size, raw_audio, ctx=None):
        """NDSequence::new (spectrogram.rs:31-94), cepstrum branch: `raw_audio` is the i16 sample vector
        (AudioData.data, audio.rs:10-14).  The plotting-only z-scored spectrogram is not produced."""
        ctx = ctx or _lib.default_context()
        s = np.ascontiguousarray(getattr(raw_audio, "data", raw_audio), dtype=np.int16)
        nf, nb = C.c_uint64(0), C.c_uint32(0)
        L = _lib.lib()
        _lib.check(L.apd_cepstrum(ctx.handle, C.c_void_p(s.ctypes.data), s.size, fft_size, fft_step, filter_size, 0, None,
                                  C.byref(nf), C.byref(nb)), ctx.handle)
        out = np.empty((nf.value, nb.value), dtype=np.float32)
        if nf.value:
            _lib.check(L.apd_cepstrum(ctx.handle, C.c_void_p(s.ctypes.data), s.size, fft_size, fft_step, filter_size, 0,
                                      C.c_void_p(out.ctypes.data), C.byref(nf), C.byref(nb)), ctx.handle)
        return NDSequence(out, nb.value, getattr(raw_audio, "id", 0))

    def encoded(self, nn, ctx=None):        # spectrogram.rs:103-121
        return NDSequence(nn.predict_frames(self.frames, ctx), nn.n_latent(), self.audio_id)

    def interesting_ranges(self, moving_average, perc, min_len, ctx=None):
        """spectrogram.rs:192-216 -> list of Slice(start, stop)."""
        ctx = ctx or _lib.default_context()
        t = self.len()
        ranges = np.zeros(2 * max(t, 1), dtype=np.uint64)
        n = C.c_uint64(0)
        _lib.check(_lib.lib().apd_interesting_ranges(ctx.handle, C.c_void_p(self.frames.ctypes.data), t, self.n_bins,
                                                     int(moving_average), float(perc), int(min_len), 0,
                                                     ranges.ctypes.data_as(C.POINTER(C.c_uint64)), t, C.byref(n)), ctx.handle)
        return [Slice(int(ranges[2 * i]), int(ranges[2 * i + 1]), self) for i in range(n.value)]

    def vec(self, t):                       # spectrogram.rs:99-101
        return self.frames[t]

    def len(self):                          # spectrogram.rs:152-154
        return int(self.frames.shape[0])

    __len__ = len


@dataclass
class Slice:
    """spectrogram.rs:222-243: a frame range of a sequence."""
    start: int
    stop: int
    sequence: "NDSequence" = None

    def len(self):
        return self.stop - self.start

    def extract(self):                      # spectrogram.rs:245-262
        return NDSequence(self.sequence.frames[self.start:self.stop], self.sequence.n_bins, self.sequence.audio_id)


_U64P = C.POINTER(C.c_uint64)


def _ptr(x):
    """The address of a numpy array, or of a DeviceBuffer's first byte."""
    return x.at() if isinstance(x, _lib.DeviceBuffer) else C.c_void_p(x.ctypes.data if x.size else None)


def interesting_ranges_batch(frames, offsets, moving_average, perc, min_len, ctx=None, on_device=False, strict=True, n_bins=None):
    """NDSequence.interesting_ranges for every recording of a packed corpus (apd_interesting_ranges_batch): `frames` [offsets[-1]][n_bins]
    and `offsets` as apd_cepstrum_batch leaves them; frames a DeviceBuffer (n_bins given) with on_device.  Returns a list, per
    recording, of (start, stop) frame pairs.  strict: a recording for which the reference panics raises ApdError(APD_ERR_INDEX);
    strict=False: (ranges, status), that recording's status APD_ERR_INDEX and its list empty."""
    ctx = ctx or _lib.default_context()
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = len(offsets) - 1
    if not on_device:
        frames = np.ascontiguousarray(frames, dtype=np.float32)
        n_bins = int(frames.shape[1]) if frames.ndim == 2 else int(n_bins)
    L = _lib.lib()
    range_off = np.zeros(n + 1, dtype=np.uint64)
    status = np.zeros(max(n, 1), dtype=np.int32)
    st = None if strict else status.ctypes.data_as(C.POINTER(C.c_int32))
    head = (ctx.handle, _ptr(frames), offsets.ctypes.data_as(_U64P), n, int(n_bins), int(moving_average), float(perc), int(min_len), int(bool(on_device)))
    # the bound of a recording's ranges: each takes more than min_len frames and the frame that closes it
    capacity = int(sum(int(offsets[s + 1] - offsets[s]) // (int(min_len) + 2) for s in range(n)))
    ranges = np.zeros(2 * max(capacity, 1), dtype=np.uint64)
    _lib.check(L.apd_interesting_ranges_batch(*head, range_off.ctypes.data_as(_U64P), ranges.ctypes.data_as(_U64P), capacity, st), ctx.handle)
    out = [[(int(ranges[2 * r]), int(ranges[2 * r + 1])) for r in range(int(range_off[s]), int(range_off[s + 1]))] for s in range(n)]
    return out if strict else (out, [int(v) for v in status[:n]])


def _flat_ranges(ranges):
    """A list of lists of (start, stop) -> (range_off [n + 1], flat pairs), both uint64."""
    range_off = np.zeros(len(ranges) + 1, dtype=np.uint64)
    range_off[1:] = np.cumsum([len(r) for r in ranges], dtype=np.uint64)
    flat = np.array([v for rec in ranges for pair in rec for v in pair], dtype=np.uint64)
    return range_off, flat


def slice_offsets(sample_offsets, ranges, fft_step):
    """apd_slice_offsets: (slice_offsets [n_slices + 1], slice_seq [n_slices]) of the ranges a list per recording holds -- the sample
    offsets of the sliced corpus (main.rs:81-88) and, per slice, the recording it came from."""
    sample_offsets = np.ascontiguousarray(sample_offsets, dtype=np.uint64)
    range_off, flat = _flat_ranges(ranges)
    n_slices = int(range_off[-1])
    out, seq = np.zeros(n_slices + 1, dtype=np.uint64), np.zeros(max(n_slices, 1), dtype=np.uint32)
    _lib.check(_lib.lib().apd_slice_offsets(sample_offsets.ctypes.data_as(_U64P), range_off.ctypes.data_as(_U64P),
                                            flat.ctypes.data_as(_U64P) if n_slices else None, len(ranges), int(fft_step),
                                            out.ctypes.data_as(_U64P), seq.ctypes.data_as(C.POINTER(C.c_uint32))))
    return out, seq[:n_slices]


def slice_samples(samples, sample_offsets, ranges, fft_step, ctx=None, on_device=False):
    """apd_slice_samples: the slices packed back to back -- an int16 array, or with on_device (samples a DeviceBuffer) a DeviceBuffer
    of slice_offsets[-1] samples."""
    ctx = ctx or _lib.default_context()
    sample_offsets = np.ascontiguousarray(sample_offsets, dtype=np.uint64)
    range_off, flat = _flat_ranges(ranges)
    total = int(slice_offsets(sample_offsets, ranges, fft_step)[0][-1])
    if on_device:
        out = ctx.alloc(max(2 * total, 16))
    else:
        samples = np.ascontiguousarray(samples, dtype=np.int16)
        out = np.zeros(total, dtype=np.int16)
    _lib.check(_lib.lib().apd_slice_samples(ctx.handle, _ptr(samples), sample_offsets.ctypes.data_as(_U64P), len(ranges),
                                            range_off.ctypes.data_as(_U64P), flat.ctypes.data_as(_U64P) if len(flat) else None,
                                            int(fft_step), int(bool(on_device)), _ptr(out), total), ctx.handle)
    return out


def segment(samples, sample_offsets, discovery, ctx=None):
    """Stage 1 of the reference (main.rs:58-92) for a whole corpus, resident: apd_cepstrum_batch on the device, the batched VAT
    ranges with discovery.vat_*, the gather of the raw audio.  samples: int16 array or DeviceBuffer.  Returns (d_slices, slice_offsets,
    slice_seq, ranges): a DeviceBuffer holding the sliced corpus, ready for apd_cepstrum_batch with slice_offsets."""
    ctx = ctx or _lib.default_context()
    L = _lib.lib()
    sample_offsets = np.ascontiguousarray(sample_offsets, dtype=np.uint64)
    n = len(sample_offsets) - 1
    d_samples = samples if isinstance(samples, _lib.DeviceBuffer) else ctx.upload(np.ascontiguousarray(samples, dtype=np.int16))
    frame_off, nb = np.zeros(n + 1, dtype=np.uint64), C.c_uint32(0)
    head = (ctx.handle, d_samples.at(), sample_offsets.ctypes.data_as(_U64P), n, int(discovery.dft_win), int(discovery.dft_step),
            int(discovery.ceps_filter), 1)
    _lib.check(L.apd_cepstrum_batch(*head, None, frame_off.ctypes.data_as(_U64P), C.byref(nb)), ctx.handle)
    d_frames = ctx.alloc(max(int(frame_off[-1]) * nb.value * 4, 16))
    _lib.check(L.apd_cepstrum_batch(*head, d_frames.at(), frame_off.ctypes.data_as(_U64P), C.byref(nb)), ctx.handle)
    ranges = interesting_ranges_batch(d_frames, frame_off, discovery.vat_moving, discovery.vat_percentile, discovery.vat_min_len, ctx,
                                      on_device=True, n_bins=nb.value)
    offs, seq = slice_offsets(sample_offsets, ranges, discovery.dft_step)
    return slice_samples(d_samples, sample_offsets, ranges, discovery.dft_step, ctx, on_device=True), offs, seq, ranges


@dataclass
class AlignmentParams:
    """alignments.rs:77-83"""
    warping_band: int
    insertion_penalty: float = 1.0
    deletion_penalty: float = 1.0
    match_penalty: float = 1.0

    @staticmethod
    def default(length):                    # alignments.rs:86-93
        return AlignmentParams(int(length), 1.0, 1.0, 1.0)


# apd_path_step as a numpy record: what Alignment.path() and AlignmentWorkers.paths() return
PATH_STEP = np.dtype([("i", np.uint32), ("j", np.uint32), ("cost", np.float32), ("op", np.uint32)])
# apd_spot_best as a numpy record: what AlignmentWorkers.spot() and spot_hits() return
SPOT_BEST = np.dtype([("end", np.uint32), ("start", np.uint32), ("cost", np.float32), ("score", np.float32)])
# apd_spot_window as a numpy record: what AlignmentWorkers.spot_paths() hands to the library
SPOT_WINDOW = np.dtype([("x", np.uint32), ("y", np.uint32), ("end", np.uint32), ("start", np.uint32)])

# apd_spot_hit as a numpy record: what AlignmentWorkers.detect() returns
SPOT_HIT = np.dtype([("pair", np.uint32), ("end", np.uint32), ("start", np.uint32), ("cost", np.float32), ("score", np.float32),
                     ("rank", np.uint32)])


class Alignment:
    """alignments.rs:99-181.  construct_alignment runs the HIP kernel.  The DP table `sparse` is not materialised as a whole; with
    `path=True` the cells a reader of `sparse` walks back through from the score cell (n-1, m-1) are kept, with their table
    values and branches: path() (include/apd.h, "warping paths")."""

    def __init__(self, ctx=None):           # Alignment::new, :107-111
        self.n = 0
        self.m = 0
        self._score = float("inf")
        self._ctx = ctx
        self._path = None

    def construct_alignment(self, x, y, params, path=False):     # :165-180
        ctx = self._ctx or _lib.default_context()
        xs = np.ascontiguousarray(x.frames if isinstance(x, NDSequence) else x, dtype=np.float32)
        ys = np.ascontiguousarray(y.frames if isinstance(y, NDSequence) else y, dtype=np.float32)
        dim = xs.shape[1] if xs.ndim == 2 and xs.shape[1] else ys.shape[1]
        self.n, self.m = int(xs.shape[0]), int(ys.shape[0])
        p = _lib.AlignmentParamsC(int(params.warping_band), params.insertion_penalty,
                                  params.deletion_penalty, params.match_penalty)
        out = C.c_float(0)
        self._path = None
        if path:
            L = _lib.lib()
            steps = np.zeros(int(L.apd_path_bound(self.n, self.m)), dtype=PATH_STEP)
            used = C.c_uint64(0)
            _lib.check(L.apd_align_pair_path(ctx.handle, xs.ctypes.data_as(C.POINTER(C.c_float)), self.n,
                                             ys.ctypes.data_as(C.POINTER(C.c_float)), self.m, int(dim), C.byref(p),
                                             steps.ctypes.data_as(C.POINTER(_lib.PathStep)), len(steps), C.byref(used),
                                             C.byref(out)), ctx.handle)
            self._path = steps[:used.value].copy()
        else:
            _lib.check(_lib.lib().apd_align_pair(ctx.handle, xs.ctypes.data_as(C.POINTER(C.c_float)), self.n,
                                                 ys.ctypes.data_as(C.POINTER(C.c_float)), self.m, int(dim),
                                                 C.byref(p), C.byref(out)), ctx.handle)
        self._score = float(out.value)

    def score(self):                        # :116-125
        if self.n == 0 and self.m == 0:
            return float("inf")
        return self._score

    def path(self):
        """The warping path of the last construct_alignment(..., path=True): a PATH_STEP array, origin first, end cell
        (n-1, m-1) last; empty when the score cell is absent."""
        if self._path is None:
            raise ValueError("construct_alignment(..., path=True) has not run")
        return self._path


class Batch:
    """apd_batch: Arc<Vec<NDSequence>> resident in HBM."""

    def __init__(self, ctx, frames, offsets, dim, on_device=False):
        self.ctx = ctx
        self.offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        self.n_seq = len(self.offsets) - 1
        self.dim = int(dim)
        self.handle = C.c_void_p()
        if on_device:
            ptr = C.c_void_p(int(frames))
        else:
            self._host = np.ascontiguousarray(frames, dtype=np.float32)
            ptr = C.c_void_p(self._host.ctypes.data)
        _lib.check(_lib.lib().apd_batch_create(ctx.handle, ptr, self.offsets.ctypes.data_as(C.POINTER(C.c_uint64)),
                                               self.n_seq, self.dim, int(bool(on_device)), C.byref(self.handle)),
                   ctx.handle)

    @staticmethod
    def join(first, second):
        """apd_batch_join: a resident batch holding `first`'s sequences followed by `second`'s (numbers n_first + c), made from the
        two batches' resident frames on the device.  An ordinary batch for align_all / paths, and what cross() aligns."""
        if first.ctx is not second.ctx:
            raise ValueError("join() needs two batches of one context")
        b = Batch.__new__(Batch)
        b.ctx, b.dim = first.ctx, first.dim
        b.handle = C.c_void_p()
        _lib.check(_lib.lib().apd_batch_join(first.ctx.handle, first.handle, second.handle, C.byref(b.handle)), first.ctx.handle)
        b.n_seq = first.n_seq + second.n_seq
        b.n_first = first.n_seq
        b.offsets = np.concatenate([first.offsets, second.offsets[1:] + first.offsets[-1]]).astype(np.uint64)
        return b

    def first_len(self):
        """apd_batch_first_len: sequences of the first set of a joined batch; all of them for a plain one."""
        return int(_lib.lib().apd_batch_first_len(self.handle))

    def close(self):
        if getattr(self, "handle", None):
            _lib.lib().apd_batch_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class AlignmentWorkers:
    """alignments.rs:11-68.  `new(data)` takes the sequences, `align_all(params)` blocks until
    `result` (n*n, row-major, diagonal 0.0) is filled.  `alignment_workers` is accepted and ignored:
    the GPU grid replaces the OS threads of :35-41."""

    def __init__(self, data, ctx=None, devices=None):     # AlignmentWorkers::new, :17-26
        """`devices`: HIP device ordinals -- the workers of :33-41 become these GPUs, driven through the library's persistent
        multi-device handle (made here once; every align_all then pays kernels + one all-gather + unpack)."""
        self._multi = None
        self._aligned = False                             # align_all has filled `result`
        if devices is not None:
            from . import sharding
            self._multi = sharding.Multi(devices)
            ctx = self._multi.contexts[0]
        self.ctx = ctx or _lib.default_context()
        self.data = list(data)
        n = len(self.data)
        self.result = np.zeros(n * n, dtype=np.float32)
        dims = {s.n_bins for s in self.data}
        if len(dims) > 1:
            raise ValueError("all sequences must share n_bins")
        self._dim = dims.pop() if dims else 1
        lens = [s.len() for s in self.data]
        offsets = np.zeros(n + 1, dtype=np.uint64)
        offsets[1:] = np.cumsum(lens)
        frames = (np.concatenate([s.frames for s in self.data], axis=0) if n
                  else np.zeros((0, self._dim), np.float32))
        self._batch = (self._multi.batch(offsets, self._dim, frames=frames) if self._multi is not None
                       else Batch(self.ctx, frames, offsets, self._dim))

    @staticmethod
    def new(data, ctx=None, devices=None):
        return AlignmentWorkers(data, ctx, devices)

    def align_all(self, params):            # :31-67, params: Discovery
        cfg = params.align_config()
        if self._multi is not None:
            self.result[:] = self._multi.align_all(self._batch, cfg).ravel()
            self._aligned = True
            return self.result
        _lib.check(_lib.lib().apd_align_all(self.ctx.handle, self._batch.handle, C.byref(cfg),
                                            self.result.ctypes.data_as(C.POINTER(C.c_float))), self.ctx.handle)
        self._aligned = True
        return self.result

    def paths(self, pairs, params):
        """Warping paths of the ordered pairs `pairs` ([(x, y), ...] in this object's sequence numbers; repeats and x == y
        allowed), params: Discovery.  Returns (list of PATH_STEP arrays in input order, float32 scores): apd_align_paths."""
        if self._multi is not None:
            raise ValueError("paths() runs on one context: make the AlignmentWorkers without `devices`")
        cfg = params.align_config()
        pr = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
        n_pairs = len(pr)
        L = _lib.lib()
        off = np.zeros(n_pairs + 1, dtype=np.uint64)
        lens = np.zeros(n_pairs, dtype=np.uint32)
        scores = np.zeros(n_pairs, dtype=np.float32)
        u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
        _lib.check(L.apd_align_paths(self.ctx.handle, self._batch.handle, C.byref(cfg), pr.ctypes.data_as(u32p), n_pairs, None, 0,
                                     off.ctypes.data_as(u64p), None, None), self.ctx.handle)
        steps = np.zeros(max(int(off[-1]), 1), dtype=PATH_STEP)
        _lib.check(L.apd_align_paths(self.ctx.handle, self._batch.handle, C.byref(cfg), pr.ctypes.data_as(u32p), n_pairs,
                                     steps.ctypes.data_as(C.POINTER(_lib.PathStep)), len(steps), off.ctypes.data_as(u64p),
                                     lens.ctypes.data_as(u32p), scores.ctypes.data_as(C.POINTER(C.c_float))), self.ctx.handle)
        return [steps[int(off[p]):int(off[p]) + int(lens[p])].copy() for p in range(n_pairs)], scores

    @contextlib.contextmanager
    def _pair_call(self, method, pairs, params, streams):
        """What spot(), detect(), score_quantiles() and spot_paths() begin and end with: one context only; yields (cfg, pairs as
        an (n, 2) uint32 array, the batch the pair numbers index -- this object's, or the two joined, closed on the way out)."""
        if self._multi is not None or (streams is not None and streams._multi is not None):
            raise ValueError("%s() runs on one context: make the AlignmentWorkers without `devices`" % method)
        cfg = params.align_config()
        pr = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
        batch = self._batch if streams is None else Batch.join(self._batch, streams._batch)
        try:
            yield cfg, pr, batch
        finally:
            if streams is not None:
                batch.close()

    def spot(self, pairs, params, curves=True, streams=None):
        """Subsequence alignment (include/apd.h, "subsequence alignment"): every (query, stream) pair of `pairs` -- this object's
        sequence numbers, or, with `streams` (an AlignmentWorkers of the same context), numbers of the two joined: below len(self.data)
        this object's, the others `streams`' -- params: Discovery (penalties only: there is no band).  Returns (list of (cost, start)
        arrays in input order, `best` as a SPOT_BEST array); the list is empty with curves=False: apd_spot."""
        with self._pair_call("spot", pairs, params, streams) as (cfg, pr, batch):
            n_pairs = len(pr)
            L = _lib.lib()
            off = np.zeros(n_pairs + 1, dtype=np.uint64)
            best = np.zeros(n_pairs, dtype=SPOT_BEST)
            u32p, u64p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_float)
            head = (self.ctx.handle, batch.handle, C.byref(cfg), pr.ctypes.data_as(u32p), n_pairs)
            tail = (off.ctypes.data_as(u64p), best.ctypes.data_as(C.POINTER(_lib.SpotBest)))
            if not curves:
                _lib.check(L.apd_spot(*head, None, None, 0, *tail), self.ctx.handle)
                return [], best
            _lib.check(L.apd_spot(*head, None, None, 0, tail[0], None), self.ctx.handle)          # sizes
            cost = np.zeros(max(int(off[-1]), 1), dtype=np.float32)
            start = np.zeros(len(cost), dtype=np.uint32)
            _lib.check(L.apd_spot(*head, cost.ctypes.data_as(f32p), start.ctypes.data_as(u32p), len(cost), *tail), self.ctx.handle)
        return [(cost[int(off[p]):int(off[p + 1])].copy(), start[int(off[p]):int(off[p + 1])].copy()) for p in range(n_pairs)], best

    def detect(self, pairs, params, thresholds, per_stream=False, streams=None, capacity=None):
        """Spot detection (include/apd.h, "spot detection"): spot() and spot_hits() in one call on the device.  pairs, params and
        `streams` as for spot(); thresholds: one value for all pairs or one per pair.  per_stream=False: every pair picks its own
        non-overlapping windows; True: the pairs of the list that share a stream compete for its columns.  capacity: hits to hold
        (None: a bound that always suffices).  Returns (hits as a SPOT_HIT array, group-major; hit_off, groups + 1 entries; groups:
        the stream number of every group with per_stream, else its pair index): apd_spot_detect.  With a capacity below the total
        only the first `capacity` hits are returned; hit_off stays exact."""
        with self._pair_call("detect", pairs, params, streams) as (cfg, pr, batch):
            n_pairs = len(pr)
            thr = np.ascontiguousarray(np.broadcast_to(np.asarray(thresholds, dtype=np.float32), (n_pairs,)))
            if per_stream:
                _, first = np.unique(pr[:, 1], return_index=True)
                groups = pr[np.sort(first), 1].astype(np.uint32)          # distinct streams in order of first appearance
            else:
                groups = np.arange(n_pairs, dtype=np.uint32)
            lens = [len(s.frames) for s in self.data] + ([len(s.frames) for s in streams.data] if streams is not None else [])
            if capacity is None:
                known = not n_pairs or int(pr.max()) < len(lens)         # a wrong index is the library's to refuse
                capacity = int(sum(lens[int(y)] for y in (groups if per_stream else pr[:, 1]))) if known else 0
            hits = np.zeros(max(int(capacity), 1), dtype=SPOT_HIT)
            off = np.zeros(n_pairs + 1, dtype=np.uint64)
            n_groups, n_hits = C.c_uint64(0), C.c_uint64(0)
            u32p, u64p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_float)
            _lib.check(_lib.lib().apd_spot_detect(self.ctx.handle, batch.handle, C.byref(cfg), pr.ctypes.data_as(u32p), n_pairs,
                                                  thr.ctypes.data_as(f32p), int(bool(per_stream)), hits.ctypes.data_as(C.POINTER(_lib.SpotHit)),
                                                  int(capacity), off.ctypes.data_as(u64p), C.byref(n_groups), C.byref(n_hits)), self.ctx.handle)
        return hits[:min(int(n_hits.value), int(capacity))].copy(), off[:n_groups.value + 1].copy(), groups

    def score_quantiles(self, pairs, params, perc, by="pair", streams=None, strict=True):
        """Spot score quantiles (include/apd.h, "spot score quantiles"): numerics::percentile over the scores of groups of spotting
        curves, on the device.  pairs, params and `streams` as for spot(); perc: a scalar or a sequence of at most 8; by: "pair" (a
        group per pair), "query" (the pairs of a query pooled, groups in order of first appearance) or "all" (one group).  Returns
        (values [n_groups, n_perc] float32, group_of [n_pairs], entries [n_groups], nans [n_groups]): apd_spot_quantiles.  A rank
        beyond a group's non-NaN scores (every perc = 1.0) raises ApdError(APD_ERR_INDEX) with strict=True; with strict=False its value
        is NaN and the int32 status array [n_groups, n_perc] is returned as a fifth item."""
        with self._pair_call("score_quantiles", pairs, params, streams) as (cfg, pr, batch):
            grouping = {"pair": _lib.APD_QUANTILES_PER_PAIR, "query": _lib.APD_QUANTILES_PER_QUERY, "all": _lib.APD_QUANTILES_ALL}[by]
            n_pairs = len(pr)
            pc = np.ascontiguousarray(np.atleast_1d(np.asarray(perc, dtype=np.float32)))
            slots = max(n_pairs, 1)
            values = np.zeros((slots, len(pc)), dtype=np.float32)
            status = np.zeros((slots, len(pc)), dtype=np.int32)
            group_of, entries, nans = (np.zeros(slots, dtype=np.uint64) for _ in range(3))
            n_groups = C.c_uint64(0)
            u32p, u64p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_float)
            _lib.check(_lib.lib().apd_spot_quantiles(self.ctx.handle, batch.handle, C.byref(cfg), pr.ctypes.data_as(u32p), n_pairs, grouping,
                                                     pc.ctypes.data_as(f32p), len(pc), values.ctypes.data_as(f32p),
                                                     status.ctypes.data_as(C.POINTER(C.c_int32)), group_of.ctypes.data_as(u64p),
                                                     entries.ctypes.data_as(u64p), nans.ctypes.data_as(u64p), C.byref(n_groups)), self.ctx.handle)
        ng = int(n_groups.value)
        out = (values[:ng].copy(), group_of[:n_pairs].copy(), entries[:ng].copy(), nans[:ng].copy())
        if not strict:
            return out + (status[:ng].copy(),)
        bad = np.argwhere(status[:ng] != _lib.APD_OK)
        if len(bad):
            g, q = (int(v) for v in bad[0])
            raise _lib.ApdError(int(status[g, q]), "score_quantiles: perc %r of group %d (%d entries, %d NaN) lies beyond its scores"
                                % (float(pc[q]), g, int(entries[g]), int(nans[g])))
        return out

    def spot_thresholds(self, pairs, params, rate, by="pair", streams=None, per_query=False):
        """Detection thresholds from the data: the `rate` quantile of the scores of every pair's group (score_quantiles, strict).
        Returns one float32 per pair, values[group_of[p], 0] -- what detect(pairs, params, thresholds) takes.  With by="query" and
        per_query=True: one value per distinct query in order of first appearance -- the vector SpotStream.detect takes when the
        queries are listed in that order."""
        if per_query and by != "query":
            raise ValueError("per_query=True needs by=\"query\"")
        values, group_of, _, _ = self.score_quantiles(pairs, params, float(rate), by=by, streams=streams)
        return values[:, 0].copy() if per_query else values[group_of.astype(np.int64), 0]

    def spot_paths(self, pairs, windows, params, streams=None):
        """Warping paths of spotted windows (include/apd.h, "warping paths of spotted windows"): window k is columns windows[k]["start"]
        .. windows[k]["end"] of the stream of pairs[k] = (query, stream) -- `windows` a SPOT_BEST array of len(pairs) records, as
        spot()'s best or spot_hits() return them (a pair may appear many times, once per hit); numbering and `streams` as for spot().
        Returns (list of PATH_STEP arrays in input order -- empty for a {0, 0} record and for a start that is not the table's --,
        found_start, scores): apd_spot_paths."""
        with self._pair_call("spot_paths", pairs, params, streams) as (cfg, pr, batch):
            n_windows = len(pr)
            if len(windows) != n_windows:
                raise ValueError("one window per pair")
            win = np.zeros(n_windows, dtype=SPOT_WINDOW)
            win["x"], win["y"] = pr[:, 0], pr[:, 1]
            win["end"], win["start"] = windows["end"], windows["start"]
            L = _lib.lib()
            off = np.zeros(n_windows + 1, dtype=np.uint64)
            lens = np.zeros(n_windows, dtype=np.uint32)
            found = np.zeros(n_windows, dtype=np.uint32)
            scores = np.zeros(n_windows, dtype=np.float32)
            u32p, u64p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_float)
            head = (self.ctx.handle, batch.handle, C.byref(cfg), win.ctypes.data_as(C.POINTER(_lib.SpotWindow)), n_windows)
            _lib.check(L.apd_spot_paths(*head, None, 0, off.ctypes.data_as(u64p), None, None, None), self.ctx.handle)       # sizes
            steps = np.zeros(max(int(off[-1]), 1), dtype=PATH_STEP)
            _lib.check(L.apd_spot_paths(*head, steps.ctypes.data_as(C.POINTER(_lib.PathStep)), len(steps), off.ctypes.data_as(u64p),
                                        lens.ctypes.data_as(u32p), found.ctypes.data_as(u32p), scores.ctypes.data_as(f32p)), self.ctx.handle)
        return [steps[int(off[p]):int(off[p]) + int(lens[p])].copy() for p in range(n_windows)], found, scores

    def spot_stream(self, queries, params, channels=1, history=0):
        """A streaming spotting session (include/apd.h, "streaming spotting"): the sequences `queries` of this object (repeats allowed)
        as templates against `channels` independent streams that arrive in chunks; params: Discovery (penalties only).  history: the
        columns the session keeps for SpotStream.paths() (0: none, SpotStream.keep() changes it).  This object must stay open as
        long as the session: SpotStream."""
        if self._multi is not None:
            raise ValueError("spot_stream() runs on one context: make the AlignmentWorkers without `devices`")
        return SpotStream(self, queries, params, channels, history)

    def barycenters(self, sets, params, init=None, iterations=10, on_device=False):
        """DTW barycenter averaging (include/apd.h, "cluster prototypes") of the sets of this object's sequence numbers in `sets`
        (as cluster_sets returns them), params: Discovery.  init[k]: the sequence whose frames start set k's barycenter; None: the
        medoids (clustering.medoids) of the last align_all's result -- an empty set then starts from sequence 0, which nothing
        reads.  Returns (list of [T_k][dim] float32 arrays, inertia [iterations][len(sets)], used [iterations][len(sets)]):
        apd_barycenters.  on_device=True: (DeviceBuffer holding the packed frames, frame_off, inertia, used) instead -- what
        Batch(ctx, buf.ptr, frame_off, dim, on_device=True) takes."""
        if self._multi is not None:
            raise ValueError("barycenters() runs on one context: make the AlignmentWorkers without `devices`")
        n_sets = len(sets)
        if init is None:
            if not self._aligned:
                raise ValueError("barycenters(init=None) takes the medoids of the last align_all: call align_all first, or pass init")
            from . import clustering
            init = clustering.medoids(self.result, sets, self.ctx)[0].copy()
            init[init == 0xFFFFFFFF] = 0
        init = np.ascontiguousarray(init, dtype=np.uint32)
        if len(init) != n_sets:
            raise ValueError("one init sequence per set")
        cfg = params.align_config()
        members = np.array([m for s in sets for m in s], dtype=np.uint32)
        set_off = np.zeros(n_sets + 1, dtype=np.uint32)
        set_off[1:] = np.cumsum([len(s) for s in sets])
        off = np.zeros(n_sets + 1, dtype=np.uint64)
        inertia = np.zeros((int(iterations), n_sets), dtype=np.float32)
        used = np.zeros((int(iterations), n_sets), dtype=np.uint32)
        u32p, u64p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_float)
        L = _lib.lib()
        head = (self.ctx.handle, self._batch.handle, C.byref(cfg), members.ctypes.data_as(u32p), set_off.ctypes.data_as(u32p), n_sets,
                init.ctypes.data_as(u32p), int(iterations))
        _lib.check(L.apd_barycenters(*head, None, 0, 0, off.ctypes.data_as(u64p), None, None), self.ctx.handle)          # sizes
        total = int(off[-1])
        tail = (total, off.ctypes.data_as(u64p), inertia.ctypes.data_as(f32p), used.ctypes.data_as(u32p))
        if on_device:
            buf = self.ctx.alloc(max(total * self._dim * 4, 16))
            _lib.check(L.apd_barycenters(*head, buf.at(0), 1, *tail), self.ctx.handle)
            return buf, off, inertia, used
        frames = np.zeros((max(total, 1), self._dim), dtype=np.float32)
        _lib.check(L.apd_barycenters(*head, C.c_void_p(frames.ctypes.data), 0, *tail), self.ctx.handle)
        return [frames[int(off[k]):int(off[k + 1])].copy() for k in range(n_sets)], inertia, used

    def cross(self, other, params):
        """Aligns this object's sequences against `other`'s (an AlignmentWorkers of the same context), params: Discovery.  Returns
        (fs [n1][n2], sf [n2][n1]): fs[q][c] = score(x = self q, y = other c), sf[c][q] = score(x = other c, y = self q):
        apd_batch_join + apd_align_cross."""
        if self._multi is not None or other._multi is not None:
            raise ValueError("cross() runs on one context: make the AlignmentWorkers without `devices`")
        cfg = params.align_config()
        n1, n2 = len(self.data), len(other.data)
        fs, sf = np.zeros((n1, n2), dtype=np.float32), np.zeros((n2, n1), dtype=np.float32)
        joined = Batch.join(self._batch, other._batch)
        try:
            _lib.check(_lib.lib().apd_align_cross(self.ctx.handle, joined.handle, C.byref(cfg), fs.ctypes.data_as(C.POINTER(C.c_float)),
                                                  sf.ctypes.data_as(C.POINTER(C.c_float))), self.ctx.handle)
        finally:
            joined.close()
        return fs, sf

    def nearest(self, other, params, k, as_x=True):
        """For every sequence of this object its k nearest sequences of `other` (an AlignmentWorkers of the same context), params:
        Discovery.  as_x=True ranks score(x = self q, y = other c) over c -- the rows of cross()'s fs; as_x=False ranks
        score(x = other c, y = self q) -- the columns of sf.  apd_batch_join + apd_align_cross_device_async + apd_neighbors: the
        cross matrix is made, ranked and freed in HBM.  Returns what clustering.neighbors returns, indices numbering `other`."""
        from .clustering import neighbors
        if self._multi is not None or other._multi is not None:
            raise ValueError("nearest() runs on one context: make the AlignmentWorkers without `devices`")
        cfg = params.align_config()
        n1, n2 = len(self.data), len(other.data)
        if n1 == 0 or n2 == 0:                                       # an empty set: nothing to align (apd_align_cross writes nothing)
            return neighbors(np.zeros((n1, n2) if as_x else (n2, n1), np.float32), k, 0 if as_x else 1, ctx=self.ctx)
        joined = Batch.join(self._batch, other._batch)
        matrix = self.ctx.alloc(4 * n1 * n2)
        try:
            fs, sf = (matrix.at(), None) if as_x else (None, matrix.at())
            _lib.check(_lib.lib().apd_align_cross_device_async(self.ctx.handle, joined.handle, C.byref(cfg), fs, sf), self.ctx.handle)
            shape = (matrix.ptr, n1, n2) if as_x else (matrix.ptr, n2, n1)
            return neighbors(shape, k, 0 if as_x else 1, ctx=self.ctx, on_device=True)
        finally:
            joined.close()
            matrix.free()

    def close(self):
        """Releases the GPU side (the reference's Drop of the Arcs)."""
        if self._batch is not None:
            self._batch.close()
            self._batch = None
        if self._multi is not None:
            self._multi.close()
            self._multi = None


class SpotStream:
    """apd_spot_stream: AlignmentWorkers.spot_stream() makes it.  Pair p = channel * len(queries) + q; the curves of the pushes, one
    after the other, are spot()'s curves of the whole stream, bit for bit, whatever the chunking."""

    ALL = 0xFFFFFFFF

    def __init__(self, workers, queries, params, channels=1, history=0):
        self._workers = workers                                   # keeps the templates' batch alive
        self.ctx = workers.ctx
        self.dim = int(workers._dim)
        self.queries = np.ascontiguousarray(queries, dtype=np.uint32).ravel()
        self.channels = int(channels)
        self.n_pairs = len(self.queries) * self.channels
        self.handle = C.c_void_p()
        cfg = params.align_config()
        _lib.check(_lib.lib().apd_spot_stream_create(self.ctx.handle, workers._batch.handle, C.byref(cfg),
                                                     self.queries.ctypes.data_as(C.POINTER(C.c_uint32)), len(self.queries), self.channels,
                                                     C.byref(self.handle)), self.ctx.handle)
        if history:
            self.keep(history)

    def keep(self, history):
        """From now on the session keeps its last `history` pushed columns of every channel (0: none): apd_spot_stream_keep.  The
        history starts empty behind each channel's current column; the table, the curves and the bests are not touched."""
        _lib.check(_lib.lib().apd_spot_stream_keep(self.ctx.handle, self.handle, int(history)), self.ctx.handle)

    def history(self, channel):
        """(first, last): the absolute columns of `channel` whose cells are kept; first == last + 1: none."""
        first, last = C.c_uint64(0), C.c_uint64(0)
        _lib.check(_lib.lib().apd_spot_stream_history(self.handle, int(channel), C.byref(first), C.byref(last)))
        return int(first.value), int(last.value)

    def paths(self, windows):
        """Warping paths of windows found while streaming (include/apd.h, "a kept history of columns"): `windows` a SPOT_WINDOW array
        -- x an index into the session's queries, y a channel, end and start absolute columns as push() reports them.  Returns what
        AlignmentWorkers.spot_paths returns: (list of PATH_STEP arrays in input order -- empty for a window that has aged out of the
        history, for a {0, 0} record and for a start that is not the table's --, found_start, scores): apd_spot_stream_paths."""
        win = np.ascontiguousarray(windows, dtype=SPOT_WINDOW)
        n_windows = len(win)
        L = _lib.lib()
        off = np.zeros(n_windows + 1, dtype=np.uint64)
        lens = np.zeros(n_windows, dtype=np.uint32)
        found = np.zeros(n_windows, dtype=np.uint32)
        scores = np.zeros(n_windows, dtype=np.float32)
        u32p, u64p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_float)
        head = (self.ctx.handle, self.handle, win.ctypes.data_as(C.POINTER(_lib.SpotWindow)), n_windows)
        _lib.check(L.apd_spot_stream_paths(*head, None, 0, off.ctypes.data_as(u64p), None, None, None), self.ctx.handle)       # sizes
        steps = np.zeros(max(int(off[-1]), 1), dtype=PATH_STEP)
        _lib.check(L.apd_spot_stream_paths(*head, steps.ctypes.data_as(C.POINTER(_lib.PathStep)), len(steps), off.ctypes.data_as(u64p),
                                           lens.ctypes.data_as(u32p), found.ctypes.data_as(u32p), scores.ctypes.data_as(f32p)), self.ctx.handle)
        return [steps[int(off[p]):int(off[p]) + int(lens[p])].copy() for p in range(n_windows)], found, scores

    def push(self, chunks, curves=True, on_device=False):
        """One chunk per channel: a list of (frames, dim) float32 arrays, zero frames allowed; with on_device=True the pair
        (device pointer of the packed frames, chunk_off array of channels + 1 entries).  Returns (list of (cost, start) arrays per pair
        -- empty with curves=False --, the running `best` as a SPOT_BEST array)."""
        L = _lib.lib()
        u32p, u64p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_float)
        if on_device:
            ptr, chunk_off = chunks
            chunk_off = np.ascontiguousarray(chunk_off, dtype=np.uint64)
            frames = C.c_void_p(int(ptr))
        else:
            if len(chunks) != self.channels:
                raise ValueError("one chunk per channel")
            arrays = [np.ascontiguousarray(c, dtype=np.float32).reshape(-1, self.dim) for c in chunks]
            chunk_off = np.zeros(self.channels + 1, dtype=np.uint64)
            chunk_off[1:] = np.cumsum([len(a) for a in arrays])
            host = np.ascontiguousarray(np.concatenate(arrays, axis=0)) if arrays else np.zeros((0, self.dim), np.float32)
            frames = C.c_void_p(host.ctypes.data)
        if len(chunk_off) != self.channels + 1:
            raise ValueError("chunk_off needs channels + 1 entries")
        off = np.zeros(self.n_pairs + 1, dtype=np.uint64)
        best = np.zeros(self.n_pairs, dtype=SPOT_BEST)
        head = (self.ctx.handle, self.handle, frames, chunk_off.ctypes.data_as(u64p), self.dim, int(bool(on_device)))
        tail = (off.ctypes.data_as(u64p), best.ctypes.data_as(C.POINTER(_lib.SpotBest)))
        if not curves:
            _lib.check(L.apd_spot_stream_push(*head, None, None, 0, *tail), self.ctx.handle)
            return [], best
        entries = int(chunk_off[-1]) * len(self.queries)
        cost = np.zeros(max(entries, 1), dtype=np.float32)
        start = np.zeros(len(cost), dtype=np.uint32)
        _lib.check(L.apd_spot_stream_push(*head, cost.ctypes.data_as(f32p), start.ctypes.data_as(u32p), len(cost), *tail), self.ctx.handle)
        return [(cost[int(off[p]):int(off[p + 1])].copy(), start[int(off[p]):int(off[p + 1])].copy()) for p in range(self.n_pairs)], best

    def push_audio(self, feed, chunks, curves=True, on_device=False):
        """push() with an AudioFeed in front: `chunks` is what AudioFeed.push takes (int16 samples per channel), the result what
        push() returns for the frames the feed makes of them; the frames never leave the device: apd_spot_stream_push_audio."""
        L = _lib.lib()
        u32p, u64p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_float)
        samples, sample_off, _keep = feed._samples(chunks, on_device)
        off = np.zeros(self.n_pairs + 1, dtype=np.uint64)
        best = np.zeros(self.n_pairs, dtype=SPOT_BEST)
        head = (self.ctx.handle, self.handle, feed.handle, samples, sample_off.ctypes.data_as(u64p), int(bool(on_device)))
        tail = (off.ctypes.data_as(u64p), best.ctypes.data_as(C.POINTER(_lib.SpotBest)))
        if not curves:
            _lib.check(L.apd_spot_stream_push_audio(*head, None, None, 0, *tail), self.ctx.handle)
            return [], best
        _lib.check(L.apd_spot_stream_push_audio(*head, None, None, 0, off.ctypes.data_as(u64p), None), self.ctx.handle)      # sizes
        cost = np.zeros(max(int(off[-1]), 1), dtype=np.float32)
        start = np.zeros(len(cost), dtype=np.uint32)
        _lib.check(L.apd_spot_stream_push_audio(*head, cost.ctypes.data_as(f32p), start.ctypes.data_as(u32p), len(cost), *tail), self.ctx.handle)
        return [(cost[int(off[p]):int(off[p + 1])].copy(), start[int(off[p]):int(off[p + 1])].copy()) for p in range(self.n_pairs)], best

    NEVER = 0xFFFFFFFF                                            # a holdoff whose timer never fires

    def detect(self, thresholds, per_stream=False, holdoff=0):
        """Arms the online detector (include/apd.h, "streaming spotting, online detection"), or arms it again: from the channels'
        current columns on, every push also runs the hold-off machine on the device and queues its hits.  thresholds: one value, one
        per query or the full (channels, queries) matrix; None disarms.  per_stream=False: every pair is its own group; True: the
        queries of a channel compete for its columns.  holdoff: columns after a pending window's end at which it is final (NEVER:
        only a later disjoint candidate or flush() emits it).  Arming again and disarming discard pending windows and hits not yet
        drained: flush() and hits() first.  apd_spot_stream_detect."""
        if thresholds is None:
            _lib.check(_lib.lib().apd_spot_stream_detect(self.ctx.handle, self.handle, None, 0, 0), self.ctx.handle)
            return
        thr = np.ascontiguousarray(np.broadcast_to(np.asarray(thresholds, dtype=np.float32), (self.channels, len(self.queries))))
        _lib.check(_lib.lib().apd_spot_stream_detect(self.ctx.handle, self.handle, thr.ctypes.data_as(C.POINTER(C.c_float)),
                                                     int(bool(per_stream)), int(holdoff)), self.ctx.handle)

    def flush(self, channel=None):
        """Emits the pending windows of `channel` (None: every channel) as if their timers had fired; the stream may go on:
        apd_spot_stream_flush."""
        _lib.check(_lib.lib().apd_spot_stream_flush(self.ctx.handle, self.handle, self.ALL if channel is None else int(channel)),
                   self.ctx.handle)

    def hits(self):
        """Drains the queue: every hit emitted since the last drain as a SPOT_HIT array (what AlignmentWorkers.detect returns),
        ascending group, then ascending rank, whatever the chunking of the pushes; empty on a session that is not armed:
        apd_spot_stream_hits.  hits[k] as a window for paths(): x = pair % len(queries), y = pair // len(queries), end, start."""
        L = _lib.lib()
        n = C.c_uint64(0)
        _lib.check(L.apd_spot_stream_hits(self.ctx.handle, self.handle, None, 0, C.byref(n)), self.ctx.handle)
        out = np.zeros(int(n.value), dtype=SPOT_HIT)
        if len(out):
            _lib.check(L.apd_spot_stream_hits(self.ctx.handle, self.handle, out.ctypes.data_as(C.POINTER(_lib.SpotHit)), len(out), C.byref(n)),
                       self.ctx.handle)
        return out

    def reset(self, channel=None, first_column=0):
        """A fresh table for `channel` (None: every channel); its next frame is absolute column first_column + 1."""
        _lib.check(_lib.lib().apd_spot_stream_reset(self.ctx.handle, self.handle, self.ALL if channel is None else int(channel),
                                                    int(first_column)), self.ctx.handle)

    def columns(self, channel):
        """Absolute column of the channel's last pushed frame."""
        out = C.c_uint64(0)
        _lib.check(_lib.lib().apd_spot_stream_columns(self.handle, int(channel), C.byref(out)))
        return int(out.value)

    def close(self):
        if getattr(self, "handle", None):
            _lib.lib().apd_spot_stream_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def cepstrum_frames(n_samples, fft_size, fft_step):
    """apd_cepstrum_frames: the frames NDSequence::new yields for a recording of n_samples (spectrogram.rs:51).  Host only."""
    return int(_lib.lib().apd_cepstrum_frames(int(n_samples), int(fft_size), int(fft_step)))


class AudioFeed:
    """apd_feed: int16 samples of `channels` live recordings in, in chunks of any length; cepstrum frames (or, with an encoder,
    their encodings) out.  The frames of the pushes, one after the other, are the bits of apd_cepstrum (+ apd_encode) on the whole
    recording, whatever the chunking.  encoder: None, a (w_encode [n_bins][latent], b_encode [latent]) pair, or the handle of an
    apd_encoder of the same context (its weights are copied: it may be destroyed afterwards)."""

    ALL = 0xFFFFFFFF

    def __init__(self, ctx, channels, fft_size, fft_step, filter_size, encoder=None):
        self.ctx = ctx
        self.channels = int(channels)
        self.handle = C.c_void_p()
        L = _lib.lib()
        dim = C.c_uint32(0)
        made = None
        if isinstance(encoder, tuple):
            w = np.ascontiguousarray(encoder[0], dtype=np.float32)
            b = np.ascontiguousarray(encoder[1], dtype=np.float32).ravel()
            made = C.c_void_p()
            f32p = C.POINTER(C.c_float)
            _lib.check(L.apd_encoder_create(ctx.handle, w.ctypes.data_as(f32p), b.ctypes.data_as(f32p), w.shape[0], w.shape[1], C.byref(made)),
                       ctx.handle)
            encoder = made
        try:
            _lib.check(L.apd_feed_create(ctx.handle, self.channels, int(fft_size), int(fft_step), int(filter_size), encoder, C.byref(dim),
                                         C.byref(self.handle)), ctx.handle)
        finally:
            if made is not None:
                L.apd_encoder_destroy(made)
        self.dim = int(dim.value)

    def _samples(self, chunks, on_device):
        """(samples pointer, sample_off, what must stay alive during the call) of a push."""
        if on_device:
            ptr, sample_off = chunks
            sample_off = np.ascontiguousarray(sample_off, dtype=np.uint64)
            if len(sample_off) != self.channels + 1:
                raise ValueError("sample_off needs channels + 1 entries")
            return C.c_void_p(int(ptr)), sample_off, None
        if len(chunks) != self.channels:
            raise ValueError("one chunk per channel")
        arrays = [np.ascontiguousarray(c, dtype=np.int16).ravel() for c in chunks]
        sample_off = np.zeros(self.channels + 1, dtype=np.uint64)
        sample_off[1:] = np.cumsum([len(a) for a in arrays])
        host = np.ascontiguousarray(np.concatenate(arrays)) if arrays else np.zeros(0, np.int16)
        return C.c_void_p(host.ctypes.data), sample_off, host

    def push(self, chunks, on_device=False):
        """One chunk per channel: a list of int16 arrays, any lengths, empty ones allowed; with on_device=True the pair (device
        pointer of the packed samples, sample_off array of channels + 1 entries).  Returns the new frames, one (frames, dim) float32
        array per channel: apd_feed_push."""
        L = _lib.lib()
        u64p = C.POINTER(C.c_uint64)
        samples, sample_off, _keep = self._samples(chunks, on_device)
        off = np.zeros(self.channels + 1, dtype=np.uint64)
        head = (self.ctx.handle, self.handle, samples, sample_off.ctypes.data_as(u64p), int(bool(on_device)))
        _lib.check(L.apd_feed_push(*head, None, 0, 0, off.ctypes.data_as(u64p)), self.ctx.handle)                         # sizes
        rows = np.zeros((max(int(off[-1]), 1), self.dim), dtype=np.float32)
        _lib.check(L.apd_feed_push(*head, C.c_void_p(rows.ctypes.data), 0, len(rows), off.ctypes.data_as(u64p)), self.ctx.handle)
        return [rows[int(off[k]):int(off[k + 1])].copy() for k in range(self.channels)]

    def reset(self, channel=None):
        """The channel (None: every channel) starts a new recording: apd_feed_reset."""
        _lib.check(_lib.lib().apd_feed_reset(self.ctx.handle, self.handle, self.ALL if channel is None else int(channel)), self.ctx.handle)

    def totals(self, channel):
        """(samples received, frames emitted) of the channel since its reset: apd_feed_totals."""
        s, f = C.c_uint64(0), C.c_uint64(0)
        _lib.check(_lib.lib().apd_feed_totals(self.handle, int(channel), C.byref(s), C.byref(f)))
        return int(s.value), int(f.value)

    def close(self):
        if getattr(self, "handle", None):
            _lib.lib().apd_feed_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def spot_hits(cost, start, n, threshold):
    """apd_spot_hits: greedy non-overlapping peak picking on one pair's curves (query of n frames): the windows whose score is
    strictly below `threshold`, best first, as a SPOT_BEST array.  Host only."""
    cost = np.ascontiguousarray(cost, dtype=np.float32)
    start = np.ascontiguousarray(start, dtype=np.uint32)
    if cost.shape != start.shape or cost.ndim != 1:
        raise ValueError("cost and start are the two curves of one pair")
    L = _lib.lib()
    args = (cost.ctypes.data_as(C.POINTER(C.c_float)), start.ctypes.data_as(C.POINTER(C.c_uint32)), len(cost), int(n), float(threshold))
    count = C.c_uint64(0)
    _lib.check(L.apd_spot_hits(*args, None, 0, C.byref(count)))
    hits = np.zeros(count.value, dtype=SPOT_BEST)
    _lib.check(L.apd_spot_hits(*args, hits.ctypes.data_as(C.POINTER(_lib.SpotBest)), len(hits), C.byref(count)))
    return hits


def align_work(offsets, dim, cfg, rank=0, world=1):
    """apd_align_work: (ordered pairs, reference-loop cells, algorithmic bytes) of a rank's share."""
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    p, c, b = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    _lib.check(_lib.lib().apd_align_work(offsets.ctypes.data_as(C.POINTER(C.c_uint64)), len(offsets) - 1, int(dim),
                                         C.byref(cfg), rank, world, C.byref(p), C.byref(c), C.byref(b)))
    return int(p.value), int(c.value), int(b.value)
