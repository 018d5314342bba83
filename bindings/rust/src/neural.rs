//! Drop-in for the path-facing part of src/neural.rs of dkohlsdorf/audio_pattern_discovery: `AutoEncoder` with the same public
//! fields (neural.rs:13-18) and `n_latent`, `step_decay`, `from_file`, `save_file`, `new`, `predict`, `take_step` (neural.rs:21-94),
//! plus `train`, the loop of main.rs:115-135.  UNCOMPILED (no Rust toolchain in the build image).
//!
//! `from_file` / `save_file` keep the reference's bincode calls when the crate still depends on bincode; the variants below go through
//! the library's own reader / writer of the same byte layout (apd_autoencoder_parse / _copy / _serialize: bincode 1.x defaults,
//! field order w_encode, w_decode, b_encode, b_decode, each {flat: Vec<f32>, cols: usize}), so that the weights a reference run saved
//! load without bincode.  Training runs on the GPU through apd_trainer: the reference's sequential SGD
//! with a defined sigmoid, bit-reproducible.  `take_step` is the drop-in form (a one-model trainer per call: slow by nature); `train`
//! keeps the model resident and launches once per epoch.
use crate::apd_sys::*;
use crate::discovery::Discovery;
use crate::error::*;
use crate::numerics::Mat;
use crate::spectrogram::{check, feature_context};
use std::fs::File;
use std::io::prelude::*;

#[derive(Clone)]
pub struct AutoEncoder {
    pub w_encode: Mat,
    pub w_decode: Mat,
    pub b_encode: Mat,
    pub b_decode: Mat,
}

impl AutoEncoder {
    /// neural.rs:21-23
    pub fn n_latent(&self) -> usize {
        self.b_encode.cols
    }

    /// neural.rs:26-28, in f32 like the reference
    pub fn step_decay(epoch: f32, params: &Discovery) -> f32 {
        unsafe { apd_step_decay(params.learning_rate, params.drop, params.epoch_drop, epoch) }
    }

    /// neural.rs:46-53: four Mat::seeded (the reference's own thread_rng draws)
    pub fn new(input_dim: usize, latent: usize) -> AutoEncoder {
        AutoEncoder {
            w_encode: Mat::seeded(input_dim, latent),
            w_decode: Mat::seeded(latent, input_dim),
            b_encode: Mat::seeded(1, latent),
            b_decode: Mat::seeded(1, input_dim),
        }
    }

    fn trainer(models: &[AutoEncoder]) -> *mut apd_trainer {
        let (d_in, latent) = (models[0].b_decode.cols as u32, models[0].b_encode.cols as u32);
        let pack = |f: &dyn Fn(&AutoEncoder) -> &Mat| -> Vec<f32> { models.iter().flat_map(|m| f(m).flat.iter().cloned()).collect() };
        let (we, wd, be, bd) = (pack(&|m| &m.w_encode), pack(&|m| &m.w_decode), pack(&|m| &m.b_encode), pack(&|m| &m.b_decode));
        let mut t: *mut apd_trainer = std::ptr::null_mut();
        unsafe { check(apd_trainer_create(feature_context(), d_in, latent, models.len() as u32, we.as_ptr(), wd.as_ptr(), be.as_ptr(), bd.as_ptr(), &mut t)); }
        t
    }

    fn download(&mut self, t: *mut apd_trainer, model: u32) {
        unsafe {
            check(apd_trainer_weights(t, model, self.w_encode.flat.as_mut_ptr(), self.w_decode.flat.as_mut_ptr(), self.b_encode.flat.as_mut_ptr(),
                                      self.b_decode.flat.as_mut_ptr()));
        }
    }

    /// neural.rs:73-94: one SGD step on x (1 x D) at learning rate alpha; returns 0.5 * euclidean(activation, y).
    pub fn take_step(&mut self, x: &Mat, alpha: f32) -> f32 {
        let t = AutoEncoder::trainer(std::slice::from_ref(self));
        let (order, mut err) = ([0u32], 0f32);
        unsafe {
            check(apd_trainer_run(feature_context(), t, x.flat.as_ptr(), 1, 0, order.as_ptr(), 1, 0, &alpha));
            check(apd_trainer_totals(t, &mut err, std::ptr::null_mut(), std::ptr::null_mut(), 0));
        }
        self.download(t, 0);
        unsafe { check(apd_trainer_destroy(t)); }
        err
    }

    /// The loop of main.rs:115-135 over `frames` ([offsets[n]][n_bins], the signals back to back): per epoch the decayed rate, the
    /// order of apd_train_order(seed, epoch), one run, and the mean error total_err / total, returned per epoch.  `total` is the
    /// reference's f32 count of ones, which stops at 2^24: min(steps, 2^24) in closed form.
    pub fn train(&mut self, frames: &[f32], offsets: &[u64], params: &Discovery, seed: u64) -> Vec<f32> {
        let t = AutoEncoder::trainer(std::slice::from_ref(self));
        let n_seq = offsets.len().saturating_sub(1) as u32;
        let n_frames = if n_seq > 0 { offsets[n_seq as usize] - offsets[0] } else { 0 };
        let mut order = vec![0u32; n_frames as usize];
        let mut means = vec![];
        for epoch in 0..params.epochs {
            let lr = AutoEncoder::step_decay(epoch as f32, params);
            let mut total_err = 0f32;
            unsafe {
                check(apd_train_order(seed, epoch as u64, offsets.as_ptr(), n_seq, order.as_mut_ptr()));
                check(apd_trainer_run(feature_context(), t, frames.as_ptr(), (frames.len() / self.b_decode.cols) as u64, 0, order.as_ptr(), n_frames, 0, &lr));
                check(apd_trainer_totals(t, &mut total_err, std::ptr::null_mut(), std::ptr::null_mut(), 1));
            }
            means.push(total_err / (n_frames.min(1 << 24) as f32));
        }
        self.download(t, 0);
        unsafe { check(apd_trainer_destroy(t)); }
        means
    }

    /// neural.rs:30-36.  The reference `unwrap`s a malformed file (panic); so does this.
    pub fn from_file(file: &str) -> Result<AutoEncoder> {
        let mut fp = File::open(file)?;
        let mut buf: Vec<u8> = vec![];
        let _ = fp.read_to_end(&mut buf)?;
        let mut view = apd_autoencoder_view::default();
        unsafe { check(apd_autoencoder_parse(buf.as_ptr() as *const _, buf.len() as u64, &mut view)); }
        let mat = |m: &apd_mat_view| -> Mat {
            let mut flat = vec![0f32; m.len as usize];
            unsafe { check(apd_autoencoder_copy(buf.as_ptr() as *const _, m, flat.as_mut_ptr())); }
            Mat { flat, cols: m.cols as usize }
        };
        Ok(AutoEncoder { w_encode: mat(&view.w_encode), w_decode: mat(&view.w_decode), b_encode: mat(&view.b_encode), b_decode: mat(&view.b_decode) })
    }

    /// neural.rs:39-44
    pub fn save_file(&self, file: &str) -> Result<()> {
        let (d_in, latent) = ((self.w_encode.flat.len() / self.w_encode.cols) as u32, self.w_encode.cols as u32);
        let mut n_bytes = 0u64;
        unsafe {
            check(apd_autoencoder_serialize(self.w_encode.flat.as_ptr(), self.w_decode.flat.as_ptr(), self.b_encode.flat.as_ptr(),
                                            self.b_decode.flat.as_ptr(), d_in, latent, std::ptr::null_mut(), 0, &mut n_bytes));
        }
        let mut encoded = vec![0u8; n_bytes as usize];
        unsafe {
            check(apd_autoencoder_serialize(self.w_encode.flat.as_ptr(), self.w_decode.flat.as_ptr(), self.b_encode.flat.as_ptr(),
                                            self.b_decode.flat.as_ptr(), d_in, latent, encoded.as_mut_ptr() as *mut _, n_bytes, &mut n_bytes));
        }
        let mut fp = File::create(file)?;
        fp.write_all(&encoded)?;
        Ok(())
    }

    /// neural.rs:55-71: z-score (sigma >= 1) of 255 * sigmoid(x W + b), one row.  The pipeline never calls this per frame any more
    /// (NDSequence::encoded hands the whole sequence to apd_encode); kept for callers that do.
    pub fn predict(&self, x: &Mat) -> Mat {
        let latent = self.n_latent();
        let rows = x.flat.len() / x.cols;
        let mut flat = vec![0f32; rows * latent];
        unsafe {
            check(apd_encode(feature_context(), x.flat.as_ptr(), rows as u64, x.cols as u32, self.w_encode.flat.as_ptr(),
                             self.b_encode.flat.as_ptr(), latent as u32, 0, flat.as_mut_ptr()));
        }
        Mat { flat, cols: latent }
    }
}

/// apd_trainer: models of one shape resident on the GPU, side by side.  The reference has no such item (it trains one model); this
/// is what restarts and learning-rate sweeps are made of, and `evaluate` is what picks one of them.
pub struct Trainer {
    handle: *mut apd_trainer,
    n_models: usize,
    d_in: usize,
}

impl Trainer {
    pub fn new(models: &[AutoEncoder]) -> Trainer {
        Trainer { handle: AutoEncoder::trainer(models), n_models: models.len(), d_in: models[0].b_decode.cols }
    }

    /// The error of every model's current weights on `frames[order[e]]` (order: one list shared by the models; None: every frame in
    /// order), nothing updated: (total_err per model -- one f32 add per position in position order, first position whose error is not
    /// finite per model).  Bit for bit what take_step would return for each frame under frozen weights.
    pub fn evaluate(&self, frames: &[f32], order: Option<&[u32]>) -> (Vec<f32>, Vec<Option<u64>>) {
        let n_frames = (frames.len() / self.d_in) as u64;
        let (order_ptr, n_eval) = match order { Some(o) => (o.as_ptr(), o.len() as u64), None => (std::ptr::null(), n_frames) };
        let (mut total, mut first) = (vec![0f32; self.n_models], vec![0u64; self.n_models]);
        unsafe {
            check(apd_trainer_evaluate(feature_context(), self.handle, frames.as_ptr(), n_frames, 0, order_ptr, n_eval, 0, std::ptr::null_mut(), 0,
                                       total.as_mut_ptr(), first.as_mut_ptr()));
        }
        (total, first.into_iter().map(|f| if f == u64::MAX { None } else { Some(f) }).collect())
    }
}

impl Drop for Trainer {
    fn drop(&mut self) {
        unsafe { apd_trainer_destroy(self.handle); }
    }
}
