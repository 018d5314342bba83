//! Drop-in for src/alignments.rs of dkohlsdorf/audio_pattern_discovery: the same public items (alignments.rs:11-14, 17, 31,
//! 77-93, 99-125, 165), bodies on the MI355X through libapd_hip.so.  UNCOMPILED (no Rust toolchain in the build image).
use crate::apd_sys::*;
use crate::discovery::Discovery;
use crate::neural::AutoEncoder;
use crate::spectrogram::{AudioFeed, NDSequence};
use std::collections::HashMap;
use std::os::raw::c_int;
use std::sync::{Arc, Mutex};

/// HIP device ordinals from APD_DEVICES ("0,1,2,3"), default device 0.
fn devices() -> Vec<c_int> {
    std::env::var("APD_DEVICES").ok()
        .map(|s| s.split(',').filter_map(|t| t.trim().parse().ok()).collect::<Vec<c_int>>())
        .filter(|v| !v.is_empty())
        .unwrap_or_else(|| vec![0])
}

/// The GPU side of an AlignmentWorkers: made by the first align_all, kept for the next ones (create once, align many).
struct Resident {
    multi: *mut apd_multi,              // contexts, RCCL communicators, worker threads: one per device
    batch: *mut apd_multi_batch,        // the corpus resident on every device
}
unsafe impl Send for Resident {}
impl Drop for Resident {
    fn drop(&mut self) { unsafe { apd_multi_destroy(self.multi); } }   // also destroys the batch
}

/// alignments.rs:11-14 -- field names and types as in the reference, so main.rs:189-195 compiles unchanged.
pub struct AlignmentWorkers {
    pub data: Arc<Vec<NDSequence>>,
    pub result: Arc<Mutex<Vec<f32>>>,
    resident: Option<Resident>,
}

impl AlignmentWorkers {
    /// alignments.rs:17-26: takes the sequences, allocates the n*n zero matrix.
    pub fn new(data: Vec<NDSequence>) -> AlignmentWorkers {
        let n = data.len();
        AlignmentWorkers { data: Arc::from(data), result: Arc::from(Mutex::from(vec![0.0f32; n * n])), resident: None }
    }

    /// alignments.rs:31-67: blocks until result[i*n+j] = score(x = data[i], y = data[j]) for every i != j; diagonal 0.0.
    /// `alignment_workers` is not read: the workers are the GPUs of APD_DEVICES.
    pub fn align_all(&mut self, params: &Discovery) {
        let n = self.data.len();
        if n == 0 { return; }
        let cfg = apd_align_config {
            warping_band_percentage: params.warping_band_percentage, insertion_penalty: params.insertion_penalty,
            deletion_penalty: params.deletion_penalty, match_penalty: params.match_penalty,
        };
        if self.resident.is_none() {
            let dim = self.data[0].n_bins as u32;
            let mut offsets = vec![0u64; n + 1];
            let mut frames: Vec<f32> = Vec::new();
            for (s, seq) in self.data.iter().enumerate() {
                offsets[s + 1] = offsets[s] + seq.len() as u64;
                frames.extend_from_slice(&seq.frames);                    // NDSequence.frames: [T][n_bins] row-major (spectrogram.rs:16-17)
            }
            let devs = devices();
            let mut multi = std::ptr::null_mut();
            let mut batch = std::ptr::null_mut();
            unsafe {
                check(apd_multi_create(devs.as_ptr(), devs.len() as u32, &mut multi));
                let rc = apd_multi_batch_create(multi, frames.as_ptr(), std::ptr::null(), offsets.as_ptr(), n as u32, dim, &mut batch);
                if rc != APD_OK { let why = last_error(multi); apd_multi_destroy(multi); panic!("libapd_hip: {} ({})", why, rc); }
            }
            self.resident = Some(Resident { multi, batch });
        }
        let r = self.resident.as_ref().unwrap();
        let mut result = self.result.lock().unwrap();                     // the reference panics on a poisoned mutex too (:56)
        let rc = unsafe { apd_multi_align_all(r.multi, r.batch, &cfg, result.as_mut_ptr()) };
        if rc != APD_OK { panic!("libapd_hip: {} ({})", last_error(r.multi), rc); }   // APD_ERR_INCOMPLETE: NaN left where no score was written
    }
}

/// Not in the reference: its align_all only knows one set.  Aligns every sequence of `queries` against every sequence of `corpus`
/// on the first device of APD_DEVICES (apd_batch_join + apd_align_cross) and returns (fs, sf), row-major:
/// fs[q * n2 + c] = score(x = queries[q], y = corpus[c]), sf[c * n1 + q] = score(x = corpus[c], y = queries[q]).
pub fn align_cross(queries: &[NDSequence], corpus: &[NDSequence], params: &Discovery) -> (Vec<f32>, Vec<f32>) {
    let (n1, n2) = (queries.len(), corpus.len());
    let (mut fs, mut sf) = (vec![0.0f32; n1 * n2], vec![0.0f32; n1 * n2]);
    if n1 == 0 || n2 == 0 { return (fs, sf); }
    let cfg = apd_align_config {
        warping_band_percentage: params.warping_band_percentage, insertion_penalty: params.insertion_penalty,
        deletion_penalty: params.deletion_penalty, match_penalty: params.match_penalty,
    };
    let pack = |set: &[NDSequence]| {
        let mut offsets = vec![0u64; set.len() + 1];
        let mut frames: Vec<f32> = Vec::new();
        for (s, seq) in set.iter().enumerate() {
            offsets[s + 1] = offsets[s] + seq.len() as u64;
            frames.extend_from_slice(&seq.frames);
        }
        (frames, offsets)
    };
    let dim = queries[0].n_bins as u32;
    let ((fa, oa), (fb, ob)) = (pack(queries), pack(corpus));
    unsafe {
        let mut ctx = std::ptr::null_mut();
        check(apd_create(devices()[0], &mut ctx));
        let (mut a, mut b, mut j) = (std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut());
        check(apd_batch_create(ctx, fa.as_ptr(), oa.as_ptr(), n1 as u32, dim, 0, &mut a));
        check(apd_batch_create(ctx, fb.as_ptr(), ob.as_ptr(), n2 as u32, dim, 0, &mut b));
        check(apd_batch_join(ctx, a, b, &mut j));
        debug_assert_eq!(apd_batch_first_len(j) as usize, n1);
        let rc = apd_align_cross(ctx, j, &cfg, fs.as_mut_ptr(), sf.as_mut_ptr());
        apd_destroy(ctx);                                                 // releases the device side of the three batches
        for h in [j, b, a] { apd_batch_destroy(h); }
        check(rc);
    }
    (fs, sf)
}

/// Not in the reference: subsequence alignment.  Every template against every stream on the first device of APD_DEVICES
/// (apd_batch_join + apd_spot, best only): out[t * streams.len() + r] = the best window of templates[t] in streams[r]; end and
/// start are 1-based stream columns, (0, 0) with an infinite score when nothing was kept.  Penalties from `params`; no band.
pub fn spot(templates: &[NDSequence], streams: &[NDSequence], params: &Discovery) -> Vec<apd_spot_best> {
    let (n1, n2) = (templates.len(), streams.len());
    let mut best = vec![apd_spot_best::default(); n1 * n2];
    if n1 == 0 || n2 == 0 { return best; }
    let cfg = apd_align_config {
        warping_band_percentage: params.warping_band_percentage, insertion_penalty: params.insertion_penalty,
        deletion_penalty: params.deletion_penalty, match_penalty: params.match_penalty,
    };
    let pack = |set: &[NDSequence]| {
        let mut offsets = vec![0u64; set.len() + 1];
        let mut frames: Vec<f32> = Vec::new();
        for (s, seq) in set.iter().enumerate() {
            offsets[s + 1] = offsets[s] + seq.len() as u64;
            frames.extend_from_slice(&seq.frames);
        }
        (frames, offsets)
    };
    let dim = templates[0].n_bins as u32;
    let ((fa, oa), (fb, ob)) = (pack(templates), pack(streams));
    let mut pairs: Vec<u32> = Vec::with_capacity(2 * n1 * n2);
    for t in 0..n1 { for r in 0..n2 { pairs.push(t as u32); pairs.push((n1 + r) as u32); } }
    let mut curve_off = vec![0u64; n1 * n2 + 1];
    unsafe {
        let mut ctx = std::ptr::null_mut();
        check(apd_create(devices()[0], &mut ctx));
        let (mut a, mut b, mut j) = (std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut());
        check(apd_batch_create(ctx, fa.as_ptr(), oa.as_ptr(), n1 as u32, dim, 0, &mut a));
        check(apd_batch_create(ctx, fb.as_ptr(), ob.as_ptr(), n2 as u32, dim, 0, &mut b));
        check(apd_batch_join(ctx, a, b, &mut j));
        let rc = apd_spot(ctx, j, &cfg, pairs.as_ptr(), (n1 * n2) as u64, std::ptr::null_mut(), std::ptr::null_mut(), 0, curve_off.as_mut_ptr(), best.as_mut_ptr());
        apd_destroy(ctx);                                                 // releases the device side of the three batches
        for h in [j, b, a] { apd_batch_destroy(h); }
        check(rc);
    }
    best
}

/// Not in the reference: spot detection.  Every template against every stream on the first device of APD_DEVICES (apd_batch_join +
/// apd_spot_detect), pair p = t * streams.len() + r as for spot(); thresholds: one per pair.  per_stream = false: every pair picks its
/// own non-overlapping windows, group g = pair g; true: the templates compete for the columns of each stream, group g = stream g.
/// Returns (hits, group-major and in acceptance order inside a group; hit_off, groups + 1 entries).
pub fn detect(templates: &[NDSequence], streams: &[NDSequence], params: &Discovery, thresholds: &[f32], per_stream: bool) -> (Vec<apd_spot_hit>, Vec<u64>) {
    let (n1, n2) = (templates.len(), streams.len());
    if n1 == 0 || n2 == 0 { return (Vec::new(), vec![0u64]); }
    assert_eq!(thresholds.len(), n1 * n2, "one threshold per pair");
    let cfg = apd_align_config {
        warping_band_percentage: params.warping_band_percentage, insertion_penalty: params.insertion_penalty,
        deletion_penalty: params.deletion_penalty, match_penalty: params.match_penalty,
    };
    let pack = |set: &[NDSequence]| {
        let mut offsets = vec![0u64; set.len() + 1];
        let mut frames: Vec<f32> = Vec::new();
        for (s, seq) in set.iter().enumerate() {
            offsets[s + 1] = offsets[s] + seq.len() as u64;
            frames.extend_from_slice(&seq.frames);
        }
        (frames, offsets)
    };
    let dim = templates[0].n_bins as u32;
    let ((fa, oa), (fb, ob)) = (pack(templates), pack(streams));
    let mut pairs: Vec<u32> = Vec::with_capacity(2 * n1 * n2);
    for t in 0..n1 { for r in 0..n2 { pairs.push(t as u32); pairs.push((n1 + r) as u32); } }
    // a group has no more hits than its stream has frames
    let frames_of = |r: usize| (ob[r + 1] - ob[r]) as usize;
    let capacity: usize = if per_stream { (0..n2).map(frames_of).sum() } else { n1 * (0..n2).map(frames_of).sum::<usize>() };
    let mut hits = vec![apd_spot_hit::default(); capacity.max(1)];
    let mut hit_off = vec![0u64; n1 * n2 + 1];
    let (mut n_groups, mut n_hits) = (0u64, 0u64);
    let compete = if per_stream { APD_DETECT_PER_STREAM } else { APD_DETECT_PER_PAIR };
    unsafe {
        let mut ctx = std::ptr::null_mut();
        check(apd_create(devices()[0], &mut ctx));
        let (mut a, mut b, mut j) = (std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut());
        check(apd_batch_create(ctx, fa.as_ptr(), oa.as_ptr(), n1 as u32, dim, 0, &mut a));
        check(apd_batch_create(ctx, fb.as_ptr(), ob.as_ptr(), n2 as u32, dim, 0, &mut b));
        check(apd_batch_join(ctx, a, b, &mut j));
        let rc = apd_spot_detect(ctx, j, &cfg, pairs.as_ptr(), (n1 * n2) as u64, thresholds.as_ptr(), compete, hits.as_mut_ptr(), capacity as u64, hit_off.as_mut_ptr(), &mut n_groups, &mut n_hits);
        apd_destroy(ctx);                                                 // releases the device side of the three batches
        for h in [j, b, a] { apd_batch_destroy(h); }
        check(rc);
    }
    hits.truncate(n_hits as usize);
    hit_off.truncate(n_groups as usize + 1);
    (hits, hit_off)
}

/// Not in the reference: spot score quantiles, the thresholds of detect() from the data.  Every template against every stream on the
/// first device of APD_DEVICES (apd_batch_join + apd_spot_quantiles), pair p = t * streams.len() + r as for spot().  grouping:
/// APD_QUANTILES_PER_PAIR (group g = pair g), APD_QUANTILES_PER_QUERY (group g = template g, its scores pooled over every stream) or
/// APD_QUANTILES_ALL (one group).  perc: 1 .. APD_SPOT_QUANTILES_MAX values.  Returns (values [groups][perc.len()]: numerics::percentile
/// of the group's scores, NaN where the index lies beyond its non-NaN scores; status [groups][perc.len()]: 0 or APD_ERR_INDEX there;
/// entries and NaN scores of every group).
pub fn score_quantiles(templates: &[NDSequence], streams: &[NDSequence], params: &Discovery, perc: &[f32], grouping: c_int)
                       -> (Vec<f32>, Vec<i32>, Vec<u64>, Vec<u64>) {
    let (n1, n2) = (templates.len(), streams.len());
    if n1 == 0 || n2 == 0 { return (Vec::new(), Vec::new(), Vec::new(), Vec::new()); }
    assert!(!perc.is_empty() && perc.len() <= APD_SPOT_QUANTILES_MAX, "1 .. APD_SPOT_QUANTILES_MAX quantiles");
    let cfg = apd_align_config {
        warping_band_percentage: params.warping_band_percentage, insertion_penalty: params.insertion_penalty,
        deletion_penalty: params.deletion_penalty, match_penalty: params.match_penalty,
    };
    let pack = |set: &[NDSequence]| {
        let mut offsets = vec![0u64; set.len() + 1];
        let mut frames: Vec<f32> = Vec::new();
        for (s, seq) in set.iter().enumerate() {
            offsets[s + 1] = offsets[s] + seq.len() as u64;
            frames.extend_from_slice(&seq.frames);
        }
        (frames, offsets)
    };
    let dim = templates[0].n_bins as u32;
    let ((fa, oa), (fb, ob)) = (pack(templates), pack(streams));
    let mut pairs: Vec<u32> = Vec::with_capacity(2 * n1 * n2);
    for t in 0..n1 { for r in 0..n2 { pairs.push(t as u32); pairs.push((n1 + r) as u32); } }
    let mut values = vec![0f32; n1 * n2 * perc.len()];
    let mut status = vec![0i32; n1 * n2 * perc.len()];
    let (mut entries, mut nans) = (vec![0u64; n1 * n2], vec![0u64; n1 * n2]);
    let mut n_groups = 0u64;
    unsafe {
        let mut ctx = std::ptr::null_mut();
        check(apd_create(devices()[0], &mut ctx));
        let (mut a, mut b, mut j) = (std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut());
        check(apd_batch_create(ctx, fa.as_ptr(), oa.as_ptr(), n1 as u32, dim, 0, &mut a));
        check(apd_batch_create(ctx, fb.as_ptr(), ob.as_ptr(), n2 as u32, dim, 0, &mut b));
        check(apd_batch_join(ctx, a, b, &mut j));
        let rc = apd_spot_quantiles(ctx, j, &cfg, pairs.as_ptr(), (n1 * n2) as u64, grouping, perc.as_ptr(), perc.len() as u32, values.as_mut_ptr(), status.as_mut_ptr(), std::ptr::null_mut(), entries.as_mut_ptr(), nans.as_mut_ptr(), &mut n_groups);
        apd_destroy(ctx);                                                 // releases the device side of the three batches
        for h in [j, b, a] { apd_batch_destroy(h); }
        check(rc);
    }
    let ng = n_groups as usize;
    values.truncate(ng * perc.len());
    status.truncate(ng * perc.len());
    entries.truncate(ng);
    nans.truncate(ng);
    (values, status, entries, nans)
}

/// Not in the reference: a streaming spotting session on the first device of APD_DEVICES (apd_spot_stream_*): every template against
/// `channels` streams that arrive in chunks.  Pair p = channel * templates.len() + t; the curves of the pushes, one after the other,
/// are apd_spot's curves of the whole stream, bit for bit, whatever the chunking.  Owns its context and the templates' batch.
pub struct SpotStream {
    ctx: *mut apd_context,
    batch: *mut apd_batch,
    handle: *mut apd_spot_stream,
    dim: u32,
    n_pairs: usize,
    channels: usize,
}

impl SpotStream {
    pub fn new(templates: &[NDSequence], params: &Discovery, channels: usize) -> SpotStream {
        assert!(!templates.is_empty() && channels > 0);
        let cfg = apd_align_config {
            warping_band_percentage: params.warping_band_percentage, insertion_penalty: params.insertion_penalty,
            deletion_penalty: params.deletion_penalty, match_penalty: params.match_penalty,
        };
        let mut offsets = vec![0u64; templates.len() + 1];
        let mut frames: Vec<f32> = Vec::new();
        for (s, seq) in templates.iter().enumerate() {
            offsets[s + 1] = offsets[s] + seq.len() as u64;
            frames.extend_from_slice(&seq.frames);
        }
        let dim = templates[0].n_bins as u32;
        let queries: Vec<u32> = (0..templates.len() as u32).collect();
        let mut s = SpotStream { ctx: std::ptr::null_mut(), batch: std::ptr::null_mut(), handle: std::ptr::null_mut(), dim,
                                 n_pairs: templates.len() * channels, channels };
        unsafe {
            check(apd_create(devices()[0], &mut s.ctx));
            check(apd_batch_create(s.ctx, frames.as_ptr(), offsets.as_ptr(), templates.len() as u32, dim, 0, &mut s.batch));
            check(apd_spot_stream_create(s.ctx, s.batch, &cfg, queries.as_ptr(), queries.len() as u32, channels as u32, &mut s.handle));
        }
        s
    }
    /// chunks[k]: channel k's frames, [m_k][dim] packed, m_k = 0 allowed.  Returns (cost, start, curve_off, best): pair p owns
    /// cost / start [curve_off[p] .. curve_off[p + 1]); best is the running best per pair, columns absolute.
    pub fn push(&mut self, chunks: &[&[f32]]) -> (Vec<f32>, Vec<u32>, Vec<u64>, Vec<apd_spot_best>) {
        assert_eq!(chunks.len(), self.channels);
        let mut chunk_off = vec![0u64; self.channels + 1];
        let mut frames: Vec<f32> = Vec::new();
        for (k, c) in chunks.iter().enumerate() {
            chunk_off[k + 1] = chunk_off[k] + (c.len() / self.dim as usize) as u64;
            frames.extend_from_slice(c);
        }
        let entries = (chunk_off[self.channels] as usize * (self.n_pairs / self.channels)).max(1);
        let (mut cost, mut start) = (vec![0f32; entries], vec![0u32; entries]);
        let mut curve_off = vec![0u64; self.n_pairs + 1];
        let mut best = vec![apd_spot_best::default(); self.n_pairs];
        unsafe {
            check(apd_spot_stream_push(self.ctx, self.handle, frames.as_ptr(), chunk_off.as_ptr(), self.dim, 0, cost.as_mut_ptr(), start.as_mut_ptr(), entries as u64, curve_off.as_mut_ptr(), best.as_mut_ptr()));
        }
        (cost, start, curve_off, best)
    }
    /// An AudioFeed on this session's context, one channel per channel of the session; its rows must have the templates' dimension.
    pub fn audio_feed(&self, fft_size: usize, fft_step: usize, filter_size: usize, nn: Option<&AutoEncoder>) -> AudioFeed {
        AudioFeed::on(self.ctx, self.channels, fft_size, fft_step, filter_size, nn)
    }
    /// push() with the feed in front: chunks[k] is channel k's new int16 samples; the frames never leave the device.
    pub fn push_audio(&mut self, feed: &mut AudioFeed, chunks: &[&[i16]]) -> (Vec<f32>, Vec<u32>, Vec<u64>, Vec<apd_spot_best>) {
        assert_eq!(chunks.len(), self.channels);
        let mut sample_off = vec![0u64; self.channels + 1];
        let mut samples: Vec<i16> = Vec::new();
        for (k, c) in chunks.iter().enumerate() {
            sample_off[k + 1] = sample_off[k] + c.len() as u64;
            samples.extend_from_slice(c);
        }
        let mut curve_off = vec![0u64; self.n_pairs + 1];
        let mut best = vec![apd_spot_best::default(); self.n_pairs];
        unsafe {
            check(apd_spot_stream_push_audio(self.ctx, self.handle, feed.handle, samples.as_ptr(), sample_off.as_ptr(), 0, std::ptr::null_mut(), std::ptr::null_mut(), 0, curve_off.as_mut_ptr(), std::ptr::null_mut()));   // sizes first
        }
        let entries = (curve_off[self.n_pairs] as usize).max(1);
        let (mut cost, mut start) = (vec![0f32; entries], vec![0u32; entries]);
        unsafe {
            check(apd_spot_stream_push_audio(self.ctx, self.handle, feed.handle, samples.as_ptr(), sample_off.as_ptr(), 0, cost.as_mut_ptr(), start.as_mut_ptr(), entries as u64, curve_off.as_mut_ptr(), best.as_mut_ptr()));
        }
        (cost, start, curve_off, best)
    }
    /// channel None: every channel.  The channel's next frame is absolute column first_column + 1.
    pub fn reset(&mut self, channel: Option<u32>, first_column: u64) {
        unsafe { check(apd_spot_stream_reset(self.ctx, self.handle, channel.unwrap_or(0xFFFF_FFFF), first_column)); }
    }
    pub fn columns(&self, channel: u32) -> u64 {
        let mut c: u64 = 0;
        unsafe { check(apd_spot_stream_columns(self.handle, channel, &mut c)); }
        c
    }
    /// From now on the session keeps its last `history_columns` columns (0: none); windows inside them can be traced: paths().
    pub fn keep(&mut self, history_columns: u32) {
        unsafe { check(apd_spot_stream_keep(self.ctx, self.handle, history_columns)); }
    }
    /// (first, last) of the channel's kept columns; first == last + 1: none.
    pub fn history(&self, channel: u32) -> (u64, u64) {
        let (mut first, mut last) = (0u64, 0u64);
        unsafe { check(apd_spot_stream_history(self.handle, channel, &mut first, &mut last)); }
        (first, last)
    }
    /// windows[k]: x a template number, y a channel, end and start absolute columns as push() reported them.  Returns per window
    /// (steps origin first, found_start, score); the steps are empty for a window that has aged out of the history, for a (0, 0)
    /// window and for a start that is not the table's.
    pub fn paths(&mut self, windows: &[apd_spot_window]) -> Vec<(Vec<apd_path_step>, u32, f32)> {
        let k = windows.len();
        let mut off = vec![0u64; k + 1];
        let (mut len, mut found, mut scores) = (vec![0u32; k], vec![0u32; k], vec![0f32; k]);
        unsafe {
            check(apd_spot_stream_paths(self.ctx, self.handle, windows.as_ptr(), k as u64, std::ptr::null_mut(), 0, off.as_mut_ptr(), std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut()));
        }
        let mut steps = vec![apd_path_step::default(); (off[k] as usize).max(1)];
        unsafe {
            check(apd_spot_stream_paths(self.ctx, self.handle, windows.as_ptr(), k as u64, steps.as_mut_ptr(), steps.len() as u64, off.as_mut_ptr(), len.as_mut_ptr(), found.as_mut_ptr(), scores.as_mut_ptr()));
        }
        (0..k).map(|p| (steps[off[p] as usize..off[p] as usize + len[p] as usize].to_vec(), found[p], scores[p])).collect()
    }
    /// Arms the online detector, or arms it again (pending windows and undrained hits are discarded: flush() and hits() first).
    /// thresholds: [channels][templates], None disarms.  per_stream = false: every pair is its own group; true: the templates of a
    /// channel compete.  holdoff: columns after a pending window's end at which it is final; u32::MAX: the timer never fires.
    pub fn detect(&mut self, thresholds: Option<&[f32]>, per_stream: bool, holdoff: u32) {
        let compete = if per_stream { APD_DETECT_PER_STREAM } else { APD_DETECT_PER_PAIR };
        let ptr = match thresholds {
            Some(t) => { assert_eq!(t.len(), self.n_pairs); t.as_ptr() }
            None => std::ptr::null(),
        };
        unsafe { check(apd_spot_stream_detect(self.ctx, self.handle, ptr, compete, holdoff)); }
    }
    /// Emits the pending windows of `channel` (None: every channel) as if their timers had fired; the stream may go on.
    pub fn flush(&mut self, channel: Option<u32>) {
        unsafe { check(apd_spot_stream_flush(self.ctx, self.handle, channel.unwrap_or(0xFFFF_FFFF))); }
    }
    /// Drains the queue: the hits emitted since the last drain, ascending group, then ascending rank.
    pub fn hits(&mut self) -> Vec<apd_spot_hit> {
        let mut n: u64 = 0;
        unsafe { check(apd_spot_stream_hits(self.ctx, self.handle, std::ptr::null_mut(), 0, &mut n)); }
        let mut hits = vec![apd_spot_hit::default(); n as usize];
        if n > 0 {
            unsafe { check(apd_spot_stream_hits(self.ctx, self.handle, hits.as_mut_ptr(), n, &mut n)); }
        }
        hits
    }
}

impl Drop for SpotStream {
    fn drop(&mut self) {
        unsafe {
            if !self.handle.is_null() { apd_spot_stream_destroy(self.handle); }
            if !self.batch.is_null() { apd_batch_destroy(self.batch); }
            if !self.ctx.is_null() { apd_destroy(self.ctx); }
        }
    }
}

/// Not in the reference: the warping paths of spotted windows (apd_batch_join + apd_spot_paths) on the first device of APD_DEVICES.
/// windows[k]: x a template number, y a stream number (NOT offset by templates.len(): that is done here), end and start as spot()
/// or spot_hits() reported them.  Returns per window (steps origin first with (n, end) last, found_start, score); the steps are
/// empty for a (0, 0) window and for a start that is not the table's -- found_start then says which start to ask again with.
pub fn spot_paths(templates: &[NDSequence], streams: &[NDSequence], windows: &[apd_spot_window], params: &Discovery)
                  -> Vec<(Vec<apd_path_step>, u32, f32)> {
    let (n1, n2, k) = (templates.len(), streams.len(), windows.len());
    if n1 == 0 || n2 == 0 || k == 0 { return Vec::new(); }
    let cfg = apd_align_config {
        warping_band_percentage: params.warping_band_percentage, insertion_penalty: params.insertion_penalty,
        deletion_penalty: params.deletion_penalty, match_penalty: params.match_penalty,
    };
    let pack = |set: &[NDSequence]| {
        let mut offsets = vec![0u64; set.len() + 1];
        let mut frames: Vec<f32> = Vec::new();
        for (s, seq) in set.iter().enumerate() {
            offsets[s + 1] = offsets[s] + seq.len() as u64;
            frames.extend_from_slice(&seq.frames);
        }
        (frames, offsets)
    };
    let dim = templates[0].n_bins as u32;
    let ((fa, oa), (fb, ob)) = (pack(templates), pack(streams));
    let joined: Vec<apd_spot_window> = windows.iter().map(|w| apd_spot_window { x: w.x, y: w.y + n1 as u32, end: w.end, start: w.start }).collect();
    let mut step_off = vec![0u64; k + 1];
    let (mut len, mut found, mut scores) = (vec![0u32; k], vec![0u32; k], vec![0f32; k]);
    let mut steps: Vec<apd_path_step>;
    unsafe {
        let mut ctx = std::ptr::null_mut();
        check(apd_create(devices()[0], &mut ctx));
        let (mut a, mut b, mut j) = (std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut());
        check(apd_batch_create(ctx, fa.as_ptr(), oa.as_ptr(), n1 as u32, dim, 0, &mut a));
        check(apd_batch_create(ctx, fb.as_ptr(), ob.as_ptr(), n2 as u32, dim, 0, &mut b));
        check(apd_batch_join(ctx, a, b, &mut j));
        let mut rc = apd_spot_paths(ctx, j, &cfg, joined.as_ptr(), k as u64, std::ptr::null_mut(), 0, step_off.as_mut_ptr(), std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut());
        steps = vec![apd_path_step::default(); (step_off[k] as usize).max(1)];
        if rc == APD_OK {
            rc = apd_spot_paths(ctx, j, &cfg, joined.as_ptr(), k as u64, steps.as_mut_ptr(), steps.len() as u64, step_off.as_mut_ptr(), len.as_mut_ptr(), found.as_mut_ptr(), scores.as_mut_ptr());
        }
        apd_destroy(ctx);                                                 // releases the device side of the three batches
        for h in [j, b, a] { apd_batch_destroy(h); }
        check(rc);
    }
    (0..k).map(|p| (steps[step_off[p] as usize..step_off[p] as usize + len[p] as usize].to_vec(), found[p], scores[p])).collect()
}

/// Not in the reference: DTW barycenter averaging (apd_barycenters) of the sets of sequence numbers in `sets` (as cluster_sets
/// returns them) on the first device of APD_DEVICES.  init[k]: the sequence whose frames start set k's barycenter (usually
/// clustering::medoids' choice).  Returns one NDSequence per set, as long as its init sequence (empty for an empty set; the last
/// frame keeps the init's last frame: the paths end at the reference's score cell), and inertia[it * sets.len() + k].
pub fn barycenters(data: &[NDSequence], sets: &[Vec<usize>], init: &[usize], iterations: usize, params: &Discovery) -> (Vec<NDSequence>, Vec<f32>) {
    assert_eq!(sets.len(), init.len());
    let n = data.len();
    if n == 0 || sets.is_empty() { return (Vec::new(), Vec::new()); }
    let cfg = apd_align_config {
        warping_band_percentage: params.warping_band_percentage, insertion_penalty: params.insertion_penalty,
        deletion_penalty: params.deletion_penalty, match_penalty: params.match_penalty,
    };
    let dim = data[0].n_bins;
    let mut offsets = vec![0u64; n + 1];
    let mut all: Vec<f32> = Vec::new();
    for (s, seq) in data.iter().enumerate() {
        offsets[s + 1] = offsets[s] + seq.len() as u64;
        all.extend_from_slice(&seq.frames);
    }
    let members: Vec<u32> = sets.iter().flat_map(|s| s.iter().map(|v| *v as u32)).collect();
    let mut set_off = vec![0u32; sets.len() + 1];
    for (k, s) in sets.iter().enumerate() { set_off[k + 1] = set_off[k] + s.len() as u32; }
    let init: Vec<u32> = init.iter().map(|v| *v as u32).collect();
    let mut frame_off = vec![0u64; sets.len() + 1];
    let mut inertia = vec![0f32; (iterations * sets.len()).max(1)];
    let mut frames: Vec<f32>;
    unsafe {
        let mut ctx = std::ptr::null_mut();
        check(apd_create(devices()[0], &mut ctx));
        let mut b = std::ptr::null_mut();
        check(apd_batch_create(ctx, all.as_ptr(), offsets.as_ptr(), n as u32, dim as u32, 0, &mut b));
        let mut rc = apd_barycenters(ctx, b, &cfg, members.as_ptr(), set_off.as_ptr(), sets.len() as u32, init.as_ptr(), iterations as u32, std::ptr::null_mut(), 0, 0, frame_off.as_mut_ptr(), std::ptr::null_mut(), std::ptr::null_mut());
        let total = frame_off[sets.len()];
        frames = vec![0f32; (total as usize * dim).max(1)];
        if rc == APD_OK {
            rc = apd_barycenters(ctx, b, &cfg, members.as_ptr(), set_off.as_ptr(), sets.len() as u32, init.as_ptr(), iterations as u32, frames.as_mut_ptr(), 0, total, frame_off.as_mut_ptr(), inertia.as_mut_ptr(), std::ptr::null_mut());
        }
        apd_destroy(ctx);                                                 // releases the device side of the batch
        apd_batch_destroy(b);
        check(rc);
    }
    inertia.truncate(iterations * sets.len());
    let out = (0..sets.len()).map(|k| NDSequence {
        frames: frames[frame_off[k] as usize * dim..frame_off[k + 1] as usize * dim].to_vec(), n_bins: dim,
        dft_win: data[init[k] as usize].dft_win, spectrogram: Vec::new(), audio_id: data[init[k] as usize].audio_id,
    }).collect();
    (out, inertia)
}

/// apd_spot_hits: the non-overlapping windows of one pair's curves whose score is strictly below `threshold`, best first.
pub fn spot_hits(cost: &[f32], start: &[u32], n: usize, threshold: f32) -> Vec<apd_spot_best> {
    assert_eq!(cost.len(), start.len());
    let mut count: u64 = 0;
    unsafe { check(apd_spot_hits(cost.as_ptr(), start.as_ptr(), cost.len() as u64, n as u64, threshold, std::ptr::null_mut(), 0, &mut count)); }
    let mut hits = vec![apd_spot_best::default(); count as usize];
    unsafe { check(apd_spot_hits(cost.as_ptr(), start.as_ptr(), cost.len() as u64, n as u64, threshold, hits.as_mut_ptr(), count, &mut count)); }
    hits
}

fn last_error(multi: *mut apd_multi) -> String {
    unsafe { std::ffi::CStr::from_ptr(apd_multi_last_error(multi)) }.to_string_lossy().into_owned()
}

/// alignments.rs:77-83
#[derive(Clone, Debug)]
pub struct AlignmentParams {
    pub warping_band: usize,
    pub insertion_penalty: f32,
    pub deletion_penalty: f32,
    pub match_penalty: f32,
}

impl AlignmentParams {
    /// alignments.rs:86-93
    pub fn default(len: usize) -> AlignmentParams {
        AlignmentParams { warping_band: len, insertion_penalty: 1.0, deletion_penalty: 1.0, match_penalty: 1.0 }
    }
}

thread_local! {
    /// One context per thread for the single-pair entry point (contexts are cheap; streams are not shared between threads).
    static PAIR_CTX: *mut apd_context = {
        let mut ctx = std::ptr::null_mut();
        unsafe { check(apd_create(devices()[0], &mut ctx)); }
        ctx
    };
}

/// One cell of a warping path (apd_path_step): the reference's 1-based table indices, sparse[(i, j)], the branch taken.
#[derive(Clone, Copy, Debug, PartialEq)]
pub struct PathStep {
    pub i: usize,
    pub j: usize,
    pub cost: f32,
    pub op: PathOp,
}
#[derive(Clone, Copy, Debug, PartialEq)]
pub enum PathOp { Match, Insert, Delete, Start }

/// alignments.rs:99-104.  `sparse` holds (0, 0) -> 0.0 from new() on, as in the reference, and after construct_alignment the
/// cells of the warping path -- the cells a reader of the reference's table meets walking back from the score cell (n-1, m-1) --
/// keyed as the reference keys them, with the table's values.  The cells off the path never leave the GPU.
#[derive(Debug)]
pub struct Alignment {
    pub n: usize,
    pub m: usize,
    pub sparse: HashMap<(usize, usize), f32>,
    score: f32,
    path: Vec<PathStep>,
}

impl Alignment {
    /// alignments.rs:107-111
    pub fn new() -> Alignment {
        let mut sparse = HashMap::new();
        sparse.insert((0, 0), 0.0);
        Alignment { n: 0, m: 0, sparse, score: std::f32::INFINITY, path: Vec::new() }
    }

    /// alignments.rs:116-125: INF for two empty sequences, else D[n-1][m-1] / (n + m) (INF if that cell was never visited).
    pub fn score(&self) -> f32 {
        if self.n == 0 && self.m == 0 { std::f32::INFINITY } else { self.score }
    }

    /// The warping path of the last construct_alignment, origin first, end cell (n-1, m-1) last; empty if that cell is absent.
    pub fn path(&self) -> &[PathStep] {
        &self.path
    }

    /// alignments.rs:165-180
    pub fn construct_alignment(&mut self, x: &NDSequence, y: &NDSequence, params: &AlignmentParams) {
        self.n = x.len();
        self.m = y.len();
        let p = apd_alignment_params { warping_band: params.warping_band as u64, insertion_penalty: params.insertion_penalty,
                                       deletion_penalty: params.deletion_penalty, match_penalty: params.match_penalty };
        let bound = unsafe { apd_path_bound(self.n as u64, self.m as u64) } as usize;
        let mut steps = vec![apd_path_step { i: 0, j: 0, cost: 0.0, op: 0 }; bound.max(1)];
        let mut used: u64 = 0;
        PAIR_CTX.with(|ctx| unsafe {
            check(apd_align_pair_path(*ctx, x.frames.as_ptr(), self.n as u64, y.frames.as_ptr(), self.m as u64, x.n_bins as u32, &p, steps.as_mut_ptr(), steps.len() as u64, &mut used, &mut self.score));
        });
        self.path = steps[..used as usize].iter().map(|s| PathStep {
            i: s.i as usize, j: s.j as usize, cost: s.cost,
            op: match s.op { APD_PATH_INSERT => PathOp::Insert, APD_PATH_DELETE => PathOp::Delete, APD_PATH_START => PathOp::Start, _ => PathOp::Match },
        }).collect();
        self.sparse.clear();
        self.sparse.insert((0, 0), 0.0);
        for s in &self.path { self.sparse.insert((s.i, s.j), s.cost); }
    }
}
