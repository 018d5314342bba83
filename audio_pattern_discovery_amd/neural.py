"""Host mirror of src/neural.rs: AutoEncoder::{new, n_latent, step_decay, predict, take_step, from_file, save_file}, and the training
loop of main.rs:115-135 (train).  Training runs on the GPU through apd_trainer: the reference's sequential SGD, one
wavefront per model, bit-defined -- take_step is the drop-in form (one launch per step, slow by nature), Trainer / train the resident
ones.  from_file / save_file read and write the
reference's `output/encoder/auto_encoder.bin` (bincode 1.x default configuration: little-endian, usize and Vec
lengths as u64, f32 as 4 bytes; struct fields in declaration order -- neural.rs:13-19, numerics.rs:171-174), so the
weights of a real reference run can be fed to apd_encode."""
import ctypes as C

import numpy as np

from . import _lib


class Mat:
    """numerics.rs:171-174: flat row-major matrix + column count."""

    def __init__(self, flat, cols):
        self.flat = np.ascontiguousarray(flat, dtype=np.float32).ravel()
        self.cols = int(cols)

    def rows(self):
        return self.flat.size // self.cols


class AutoEncoder:
    """neural.rs:12-19.  predict() uses the encoder half; take_step() and to_bytes() need all four matrices."""

    def __init__(self, w_encode, b_encode, w_decode=None, b_decode=None):
        self.w_encode = w_encode if isinstance(w_encode, Mat) else Mat(w_encode, np.asarray(w_encode).shape[1])
        self.b_encode = b_encode if isinstance(b_encode, Mat) else Mat(b_encode, np.asarray(b_encode).size)
        self.w_decode, self.b_decode = w_decode, b_decode

    @staticmethod
    def new(input_dim, latent, rng=None):
        """neural.rs:46-53: four Mat::seeded (numerics.rs:178-186), (u - 0.5) / cols in f32 with u uniform on [0, 1), drawn in the
        reference's order: w_encode, w_decode, b_encode, b_decode.  rng: a numpy Generator (the reference uses thread_rng)."""
        rng = rng if rng is not None else np.random.default_rng()

        def seeded(rows, cols):
            return Mat((rng.random(rows * cols, dtype=np.float32) - np.float32(0.5)) / np.float32(cols), cols)

        w_encode, w_decode = seeded(input_dim, latent), seeded(latent, input_dim)
        return AutoEncoder(w_encode, seeded(1, latent), w_decode, seeded(1, input_dim))

    @staticmethod
    def step_decay(epoch, discovery):         # neural.rs:26-28, every operation in f32
        return float(_lib.lib().apd_step_decay(discovery.learning_rate, discovery.drop, discovery.epoch_drop, float(epoch)))

    def take_step(self, x, alpha, ctx=None):
        """neural.rs:74-94: one SGD step on the frame x (a Mat 1 x D or D values), the four matrices updated in place; returns the
        step's error.  A one-model trainer made, run for one step and dropped: the drop-in form.  Use Trainer / train for more."""
        flat = x.flat if isinstance(x, Mat) else np.asarray(x, np.float32)
        with Trainer(ctx or _lib.default_context(), [self]) as t:
            t.run(np.asarray(flat, np.float32).reshape(1, -1), np.zeros(1, np.uint32), alpha)
            err = t.totals()[0][0]
            got = t.weights(0)
        for name in ("w_encode", "w_decode", "b_encode", "b_decode"):
            getattr(self, name).flat[:] = getattr(got, name).flat
        return float(err)

    @staticmethod
    def from_bytes(buf):
        """bincode::deserialize::<AutoEncoder> (neural.rs:30-36) through apd_autoencoder_parse / apd_autoencoder_copy:
        w_encode, w_decode, b_encode, b_decode, each a Mat { flat: Vec<f32>, cols: usize }."""
        buf = bytes(buf)
        view = _lib.AutoEncoderView()
        raw = C.create_string_buffer(buf, len(buf))
        if _lib.lib().apd_autoencoder_parse(raw, len(buf), C.byref(view)) != _lib.APD_OK:
            raise ValueError("not a bincode AutoEncoder (truncated, trailing bytes or inconsistent Mat shapes)")
        mats = []
        for mv in (view.w_encode, view.w_decode, view.b_encode, view.b_decode):
            flat = np.empty(mv.len, dtype=np.float32)
            _lib.check(_lib.lib().apd_autoencoder_copy(raw, C.byref(mv), flat.ctypes.data_as(C.POINTER(C.c_float))))
            mats.append(Mat(flat, mv.cols))
        return AutoEncoder(mats[0], mats[2], mats[1], mats[3])

    @staticmethod
    def from_file(file):                      # neural.rs:30-36
        with open(file, "rb") as fp:
            return AutoEncoder.from_bytes(fp.read())

    def to_bytes(self):                       # bincode::serialize (neural.rs:39-44) through apd_autoencoder_serialize
        mats = []
        for m in (self.w_encode, self.w_decode, self.b_encode, self.b_decode):
            if m is None:
                raise ValueError("decoder half missing: cannot serialise")
            mats.append(m if isinstance(m, Mat) else Mat(m, np.asarray(m).shape[-1]))
        latent, d_in = mats[0].cols, mats[0].rows()
        f32p = C.POINTER(C.c_float)
        ptrs = [m.flat.ctypes.data_as(f32p) for m in mats]
        n = C.c_uint64(0)
        _lib.check(_lib.lib().apd_autoencoder_serialize(None, None, None, None, d_in, latent, None, 0, C.byref(n)))
        out = C.create_string_buffer(n.value)
        if (mats[1].flat.size, mats[2].flat.size, mats[3].flat.size) != (d_in * latent, latent, d_in):
            raise ValueError("AutoEncoder matrices have inconsistent shapes")
        _lib.check(_lib.lib().apd_autoencoder_serialize(ptrs[0], ptrs[1], ptrs[2], ptrs[3], d_in, latent, out, n.value, C.byref(n)))
        return out.raw

    def save_file(self, file):                # neural.rs:39-44
        with open(file, "wb") as fp:
            fp.write(self.to_bytes())

    def n_latent(self):                       # neural.rs:22-24
        return self.b_encode.cols

    def predict_frames(self, frames, ctx=None):
        """AutoEncoder::predict applied to every row of `frames` ([t][d_in]) -> [t][latent] (neural.rs:55-71)."""
        ctx = ctx or _lib.default_context()
        x = np.ascontiguousarray(frames, dtype=np.float32)
        d_in, latent = self.w_encode.rows(), self.n_latent()
        if x.ndim != 2 or x.shape[1] != d_in:
            raise AssertionError("self.cols == other.rows()")     # the reference's only assert (numerics.rs:306)
        out = np.empty((x.shape[0], latent), dtype=np.float32)
        f32p = C.POINTER(C.c_float)
        _lib.check(_lib.lib().apd_encode(ctx.handle, C.c_void_p(x.ctypes.data), x.shape[0], d_in,
                                         self.w_encode.flat.ctypes.data_as(f32p), self.b_encode.flat.ctypes.data_as(f32p),
                                         latent, 0, C.c_void_p(out.ctypes.data)), ctx.handle)
        return out

    def reconstruction_errors(self, frames, ctx=None):
        """The error take_step would return for every row of `frames` under these weights (0.5 * euclidean(activation, x.norm())),
        nothing updated: Trainer.evaluate over a one-model trainer made and dropped.  A novelty curve of the frames under this model."""
        with Trainer(ctx or _lib.default_context(), [self]) as t:
            return t.evaluate(frames, errors=True)[0][0]

    def predict(self, x, ctx=None):           # neural.rs:55-71, x: Mat 1 x D
        flat = x.flat if isinstance(x, Mat) else np.asarray(x, np.float32)
        return Mat(self.predict_frames(np.asarray(flat, np.float32).reshape(1, -1), ctx).ravel(), self.n_latent())


class Encoder:
    """An apd_encoder handle (what apd_encode_async and apd_feed_create take), here one made by Trainer.encoder()."""

    def __init__(self, ctx, handle, d_in, latent):
        self.ctx, self.handle, self.d_in, self.latent = ctx, handle, d_in, latent

    def encode_async(self, d_x, t, d_out):
        """apd_encode_async on device pointers ([t][d_in] -> [t][latent]); enqueues only."""
        _lib.check(_lib.lib().apd_encode_async(self.ctx.handle, self.handle, d_x, int(t), d_out), self.ctx.handle)

    def close(self):
        if self.handle:
            _lib.lib().apd_encoder_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Trainer:
    """apd_trainer: `models` (AutoEncoders of one shape, all four matrices) resident on ctx's GPU, advanced side by side."""

    def __init__(self, ctx, models):
        models = list(models)
        if not models:
            raise _lib.ApdError(_lib.APD_ERR_INVALID_ARG)
        self.ctx, self.n_models = ctx, len(models)
        self.d_in, self.latent = models[0].w_encode.rows(), models[0].n_latent()
        packed = []
        for name, size in (("w_encode", self.d_in * self.latent), ("w_decode", self.d_in * self.latent), ("b_encode", self.latent),
                           ("b_decode", self.d_in)):
            mats = [getattr(m, name) for m in models]
            if any(x is None or x.flat.size != size for x in mats):
                raise ValueError("every model needs the four matrices of one shape")
            packed.append(np.ascontiguousarray(np.concatenate([x.flat for x in mats]), dtype=np.float32))
        f32p = C.POINTER(C.c_float)
        self.handle = C.c_void_p()
        _lib.check(_lib.lib().apd_trainer_create(ctx.handle, self.d_in, self.latent, self.n_models, *[a.ctypes.data_as(f32p) for a in packed],
                                                 C.byref(self.handle)), ctx.handle)

    def run(self, frames, order, alpha, on_device=False):
        """apd_trainer_run.  frames: [n][d_in] array, or with on_device a (device pointer, n) pair.  order: [steps] frame numbers
        shared by all models, or [n_models][steps].  alpha: one value or one per model."""
        order = np.ascontiguousarray(order, dtype=np.uint32)
        per_model = order.ndim == 2
        if per_model and order.shape[0] != self.n_models:
            raise ValueError("a per-model order has one row per model")
        alpha = np.ascontiguousarray(np.broadcast_to(np.asarray(alpha, np.float32), (self.n_models,)))
        if on_device:
            ptr, n_frames = frames
            ptr = ptr if isinstance(ptr, C.c_void_p) else C.c_void_p(int(ptr))
        else:
            x = np.ascontiguousarray(frames, dtype=np.float32).reshape(-1, self.d_in)
            ptr, n_frames = C.c_void_p(x.ctypes.data), x.shape[0]
        _lib.check(_lib.lib().apd_trainer_run(self.ctx.handle, self.handle, ptr, int(n_frames), int(bool(on_device)),
                                              order.ctypes.data_as(C.POINTER(C.c_uint32)), order.shape[-1], int(per_model),
                                              alpha.ctypes.data_as(C.POINTER(C.c_float))), self.ctx.handle)

    def totals(self, reset=False):
        """(total_err [f32], steps since the last reset, first non-finite step or None) per model; reset: an epoch boundary."""
        err, steps, first = np.empty(self.n_models, np.float32), np.empty(self.n_models, np.uint64), np.empty(self.n_models, np.uint64)
        _lib.check(_lib.lib().apd_trainer_totals(self.handle, err.ctypes.data_as(C.POINTER(C.c_float)), steps.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                 first.ctypes.data_as(C.POINTER(C.c_uint64)), int(bool(reset))), self.ctx.handle)
        none = np.uint64(0xFFFFFFFFFFFFFFFF)
        return [(err[m], int(steps[m]), None if first[m] == none else int(first[m])) for m in range(self.n_models)]

    def evaluate(self, frames, order=None, on_device=False, errors=False):
        """apd_trainer_evaluate: every model's current weights on frames[order[e]], nothing updated.  frames as in run(); order: None
        (every frame, in order), [n_eval] shared by all models, or [n_models][n_eval].  Returns (total_err [n_models] f32,
        first_nonfinite [n_models]: a position or None); with errors=True (errors [n_models][n_eval] f32, total_err, first_nonfinite).
        errors may also be a device pointer (a DeviceBuffer.at()): the per-frame errors are left there and the pointer is returned."""
        if on_device:
            ptr, n_frames = frames
            ptr = ptr if isinstance(ptr, C.c_void_p) else C.c_void_p(int(ptr))
        else:
            x = np.ascontiguousarray(frames, dtype=np.float32).reshape(-1, self.d_in)
            ptr, n_frames = C.c_void_p(x.ctypes.data), x.shape[0]
        per_model, order_ptr, n_eval = False, None, int(n_frames)
        if order is not None:
            order = np.ascontiguousarray(order, dtype=np.uint32)
            per_model = order.ndim == 2
            if per_model and order.shape[0] != self.n_models:
                raise ValueError("a per-model order has one row per model")
            order_ptr, n_eval = order.ctypes.data_as(C.POINTER(C.c_uint32)), order.shape[-1]
        out, out_ptr, out_on_device = None, None, 0
        if errors is True:
            out = np.empty((self.n_models, n_eval), np.float32)
            out_ptr = C.c_void_p(out.ctypes.data)
        elif errors is not False and errors is not None:
            out, out_on_device = errors, 1
            out_ptr = errors if isinstance(errors, C.c_void_p) else C.c_void_p(int(errors))
        total, first = np.empty(self.n_models, np.float32), np.empty(self.n_models, np.uint64)
        _lib.check(_lib.lib().apd_trainer_evaluate(self.ctx.handle, self.handle, ptr, int(n_frames), int(bool(on_device)), order_ptr, n_eval,
                                                   int(per_model), out_ptr, out_on_device, total.ctypes.data_as(C.POINTER(C.c_float)),
                                                   first.ctypes.data_as(C.POINTER(C.c_uint64))), self.ctx.handle)
        none = np.uint64(0xFFFFFFFFFFFFFFFF)
        first = [None if f == none else int(f) for f in first]
        return (total, first) if out is None else (out, total, first)

    def best(self, frames, order=None, on_device=False):
        """The model evaluate() scores lowest on these frames (a NaN total never wins), and the totals: (index or None, total_err)."""
        total, _ = self.evaluate(frames, order, on_device)
        return (None if np.isnan(total).all() else int(np.nanargmin(total))), total

    def weights(self, model):
        d, l = self.d_in, self.latent
        we, wd, be, bd = (np.empty(n, np.float32) for n in (d * l, d * l, l, d))
        f32p = C.POINTER(C.c_float)
        _lib.check(_lib.lib().apd_trainer_weights(self.handle, int(model), we.ctypes.data_as(f32p), wd.ctypes.data_as(f32p),
                                                  be.ctypes.data_as(f32p), bd.ctypes.data_as(f32p)), self.ctx.handle)
        return AutoEncoder(Mat(we, l), Mat(be, l), Mat(wd, d), Mat(bd, d))

    def encoder(self, model):
        """apd_trainer_encoder: the model's current encoder half as a resident apd_encoder (a copy, device to device)."""
        h = C.c_void_p()
        _lib.check(_lib.lib().apd_trainer_encoder(self.ctx.handle, self.handle, int(model), C.byref(h)), self.ctx.handle)
        return Encoder(self.ctx, h, self.d_in, self.latent)

    def close(self):
        if getattr(self, "handle", None):
            _lib.lib().apd_trainer_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def train_order(seed, epoch, offsets):
    """apd_train_order: the frame numbers of one epoch -- signals in order, each signal's frames freshly shuffled (main.rs:120-124)."""
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    n_seq = max(len(offsets) - 1, 0)
    order = np.empty(int(offsets[-1] - offsets[0]) if n_seq else 0, np.uint32)
    _lib.check(_lib.lib().apd_train_order(int(seed), int(epoch), offsets.ctypes.data_as(C.POINTER(C.c_uint64)), n_seq,
                                          order.ctypes.data_as(C.POINTER(C.c_uint32))))
    return order


def epoch_count(n):
    """The reference's `total` after n steps (main.rs:117,131): an f32 that grows by 1.0 per step and so stops at 2^24, where
    16777216 + 1 rounds back.  In closed form: min(n, 2^24)."""
    return np.float32(min(int(n), 1 << 24))


def train(frames, offsets, discovery, models=1, seed=0, ctx=None):
    """The loop of main.rs:115-135 on the GPU.  Per epoch: the learning rate of step_decay, the order of apd_train_order(seed, epoch)
    (one order, shared by the models), one run over it, and the mean error total_err / total with `total` the reference's f32 count
    (epoch_count).  models: a number (AutoEncoder.new(D, discovery.auto_encoder) from default_rng(seed + m) each) or the AutoEncoders
    to start from (left unchanged).  Returns (trained AutoEncoders, means [epochs][models] f32)."""
    ctx = ctx or _lib.default_context()
    x = np.ascontiguousarray(frames, dtype=np.float32)
    if isinstance(models, int):
        models = [AutoEncoder.new(x.shape[1], discovery.auto_encoder, np.random.default_rng(seed + m)) for m in range(models)]
    means = np.empty((discovery.epochs, len(models)), np.float32)
    with Trainer(ctx, models) as t:
        d_x = ctx.upload(x) if x.size else None
        for epoch in range(discovery.epochs):
            lr = AutoEncoder.step_decay(epoch, discovery)
            order = train_order(seed, epoch, offsets)
            if order.size:
                t.run((d_x.at(), x.shape[0]), order, lr, on_device=True)
            total = epoch_count(order.size)
            with np.errstate(invalid="ignore", divide="ignore"):
                means[epoch] = [err / total for err, _, _ in t.totals(reset=True)]
        out = [t.weights(m) for m in range(len(models))]
        if d_x is not None:
            d_x.free()
    return out, means
