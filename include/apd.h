/*
 * apd.h -- C ABI of the MI355X-native alignment + clustering path.
 *
 * Drop-in boundary for the one hot path of dkohlsdorf/audio_pattern_discovery:
 * AlignmentWorkers::align_all (src/alignments.rs:31-67) feeding
 * AgglomerativeClustering::clustering (src/clustering.rs:81-110), plus the two feature
 * companions NDSequence::new (src/spectrogram.rs:31-94) and AutoEncoder::predict
 * (src/neural.rs:55-71).  The reference has no FFI of its own (one Rust crate, plain `pub`
 * items called from src/main.rs:187-203); each entry point below names the Rust item a
 * binding crate would route to it -- INTEGRATION.md shows that binding.
 *
 * Conventions: plain pointers and sizes only; every function returns an apd_status
 * (0 = OK, negative = error), never throws or aborts across the boundary; the caller owns
 * host buffers, the library owns device buffers behind the opaque handles; functions taking
 * a context are synchronous unless their name ends in _async.  Pointers named d_* are
 * DEVICE pointers (HBM of the context's GPU), everything else is host memory.
 *
 * There is no CPU fallback: without a gfx950 device apd_create fails with
 * APD_ERR_NO_DEVICE and nothing else can be called.
 */
#ifndef APD_H
#define APD_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum apd_status {
    APD_OK = 0,
    APD_ERR_INVALID_ARG = -1,
    APD_ERR_NO_DEVICE = -2,      /* no HIP device / not gfx950 */
    APD_ERR_HIP = -3,            /* a HIP runtime call failed: apd_last_error() has the text */
    APD_ERR_OOM = -4,
    APD_ERR_EMPTY_SEQUENCE = -5, /* a zero-length sequence: the reference underflows usize at alignments.rs:120 */
    APD_ERR_BAND_TOO_WIDE = -6,  /* 2*w+1 exceeds what one wavefront's LDS state can hold */
    APD_ERR_INDEX = -7,          /* percentile index past the data: the reference panics at numerics.rs:132 */
    APD_ERR_UNSUPPORTED = -8,
    APD_ERR_INCOMPLETE = -9,     /* a pair score was never written (a launch was cut short or skipped): the output holds NaN
                                    there.  The reference swallows a failed worker and leaves silent zeros
                                    (alignments.rs:64-66); this library poisons and reports instead */
    APD_ERR_COMM = -10           /* an RCCL call failed: apd_last_error() has the text */
} apd_status;

typedef struct apd_context apd_context;   /* one GPU + one HIP stream + workspaces */
typedef struct apd_batch apd_batch;       /* Arc<Vec<NDSequence>> resident in HBM (alignments.rs:12) */
typedef struct apd_comm apd_comm;         /* this rank's end of an RCCL communicator over the GPUs that share the pair tiles */
typedef struct apd_encoder apd_encoder;   /* AutoEncoder's w_encode / b_encode resident on a context's GPU (neural.rs:13-17) */
typedef struct apd_cepstrum_plan apd_cepstrum_plan;   /* window, filterbank, DCT and twiddle tables + the offsets of a corpus, resident */

/* THE DOMAIN OF AN ALIGNMENT CONFIGURATION (apd_align_config and apd_alignment_params; every entry point that takes one).
 *
 * Penalties.  Any f32 is accepted: zero, negative, +-INF, NaN, subnormal.  The arithmetic is the reference's, IEEE operation for
 * operation (node = predecessor + (penalty * d), the product rounded on its own; a comparison with a NaN is false and takes the
 * MATCH branch, alignments.rs:153-159), so 0 * d, INF * 0 = NaN on a duplicated frame and a NaN penalty come out as on the CPU,
 * NaN payloads aside: a NaN penalty is read as the canonical quiet NaN, and a NaN score is a result, not APD_ERR_INCOMPLETE.
 *   apd_align_all / _device_async, apd_align_tiles_async and what is built on them (apd_align_cross, apd_align_pair, the sharded,
 *   multi-device and one-call forms): a call in which ANY penalty is <= 0 (-0.0 included), +INF or NaN runs the literal kernel
 *   alone (the fast kernels need pen * INF = INF); apd_set_variant does not override that.  Positive finite penalties run the
 *   fast kernels: equal ones within 1e-4 relative of the CPU code (bit-identical in distance mode 2), unequal ones bit-identical.
 *   apd_align_paths, apd_align_pair_path, apd_spot, apd_spot_detect, apd_spot_paths, the streaming session and apd_barycenters have
 *   one kernel family each and route nothing: bit-identical for every penalty.
 *
 * The band.  warping_band_percentage: the band of a pair is (pct * (float)max(n, m)) as usize, ONE f32 product truncated with
 * Rust's saturating cast (discovery.rs:40): NaN, negatives, -0.0 and products below 1 give 0; float32(0.7) * 10 is 7, not 6.
 * warping_band: any u64.  Either way the window is w = max(min(band, max(n, m)), |n - m|) + 2 (alignments.rs:173 with the band
 * clamped first): a band >= max(n, m) already spans the whole matrix, so 1.5, 1e10, 1e30, +INF, 2^32 - 1, 2^32 and UINT64_MAX
 * all equal the full band.  DEVIATION, deliberate: for a band within 2 of usize::MAX the reference's `+ 2` overflows (a panic in
 * a debug build, w = 1 in a release build); here, and in the checkers (oracle/apd_oracle.h), the band is the full matrix.
 * apd_discovery_alignment_params saturates to UINT64_MAX as the cast does; an explicit band beyond 0xFFFFFFF0 is held as
 * 0xFFFFFFF0 internally, which the clamp makes indistinguishable.  apd_spot and its family read no band.
 *
 * APD_ERR_BAND_TOO_WIDE.  The literal kernel keeps two DP rows of 2w + 1 offsets in LDS: 2w + 1 <= 20 480.  A call that must run
 * it -- a non-positive, infinite or NaN penalty, or frames outside the fast kernels' feature range -- over a pair with a wider
 * window (lengths beyond 10 237 under a full band) returns APD_ERR_BAND_TOO_WIDE before anything is enqueued or written.  The
 * path and barycenter calls have the same limit for every penalty (below). */

/* The four Discovery fields the path reads (src/discovery.rs:17-20, project/config/Discovery.toml:17-20). */
typedef struct apd_align_config {
    float warping_band_percentage;
    float insertion_penalty;
    float deletion_penalty;
    float match_penalty;
} apd_align_config;

/* AlignmentParams (src/alignments.rs:77-83). */
typedef struct apd_alignment_params {
    uint64_t warping_band;
    float insertion_penalty;
    float deletion_penalty;
    float match_penalty;
} apd_alignment_params;

/* Merge (src/clustering.rs:8-13) and ClusteringOperation (src/clustering.rs:19-25). */
enum { APD_SEQUENCE2SEQUENCE = 0, APD_SEQUENCE2CLUSTER = 1, APD_CLUSTER2SEQUENCE = 2, APD_CLUSTER2CLUSTER = 3 };
typedef struct apd_cluster_op {
    uint32_t merge_i;
    uint32_t merge_j;
    uint32_t into;
    float distance;
    uint32_t operation;
} apd_cluster_op;

/* ---- context ------------------------------------------------------------------------- */
/* Environment: APD_DEBUG_AFFINITY=1 makes every allocation, event record and launch inside the library check that the calling
 * thread is bound to THIS context (not merely to the same device number) and fail with APD_ERR_HIP otherwise -- how the
 * several-ranks-on-one-GPU rehearsals catch a worker thread that forgot hipSetDevice (tests/test_gpu_multi.py). */
int apd_create(int device, apd_context **ctx);
/* Also releases the device memory of every batch, and the RCCL side of every communicator, still alive on the context; such
 * a batch / communicator may (and must, for its host part) still be passed to apd_batch_destroy / apd_comm_destroy
 * afterwards, in any order, and is refused by every other call. */
int apd_destroy(apd_context *ctx);
/* Run on the caller's hipStream_t (e.g. torch's current stream) instead of the context's own. */
int apd_set_stream(apd_context *ctx, void *hip_stream);
/* Waits for the context's stream.  Also reports (once) what asynchronous calls found since the last report:
 * APD_ERR_INCOMPLETE if an unpack met a pair score that no kernel wrote. */
int apd_synchronize(apd_context *ctx);
const char *apd_status_string(int status);
const char *apd_last_error(apd_context *ctx);
/* Record HIP events around every alignment kernel launch; apd_last_kernel_ms returns the
 * duration of the most recent one (ms, on the launch stream), < 0 if none was timed. */
int apd_set_timing(apd_context *ctx, int enabled);
float apd_last_kernel_ms(apd_context *ctx);
/* Tuning knob for experiments: 0 = pick automatically.  See DESIGN.md "Kernel variants". */
int apd_set_variant(apd_context *ctx, int variant);
/* Local-distance form of the fast kernels with UNIT penalties (1.0, 1.0, 1.0 -- the shipped Discovery.toml).
 * mode 1 (default; D >= 8 in the band kernels, D >= 10 in the strip kernels): |x|^2 + |y|^2 - 2 x.y from precomputed frame
 * norms, recomputed in the difference form wherever the result is below tau * (|x|^2 + |y|^2) (cancellation region; default
 * tau 1/64): ~3e-7 relative measured (tolerance asked: 1e-4); exact copies score exactly 0.  tau = 0 (or -0.0) keeps the context's
 * current value; a value > 0 is stored in the context whatever the mode and stays until the next value > 0 -- it survives mode
 * changes, and modes 0 and 2 do not read it; tau < 0 or NaN is APD_ERR_INVALID_ARG and changes neither the mode nor the value.
 * Since |x - y|^2 <= 2 (|x|^2 + |y|^2), tau = 4 recomputes every cell with a non-zero norm sum (tests/test_gpu_tau_gate.py).
 * mode 0: the difference form sqrt(sum (x_k-y_k)^2).  In the band-form kernels it is computed operation for operation as
 * numerics.rs:114-120 does (every difference, square and partial sum rounded on its own, correctly rounded sqrt), and with
 * unit penalties the fast select picks the reference's predecessor for every non-NaN input: scores are bit-identical to the CPU
 * code, about 1.9x the time of mode 1.  (The strip kernels of full-band batches keep an fma chain in mode 0: ~2e-7.)
 * mode 2 (strict): the reference's arithmetic in EVERY kernel family -- band kernels as mode 0, strip kernels through their
 * literal-select path: every score bit-identical to the CPU code -- the mode that meets 1e-4 on EVERY entry.  cfg 3: 1.44 s instead
 * of 0.75 s (the square root is v_sqrt_f32 + an exact two-sided fix-up, checked for every f32 input by apd_selftest_sqrt).
 * With any other penalties the recurrence is discontinuous in its inputs (the penalty added depends on which predecessor wins
 * a strict comparison), so the library ignores the mode and computes operation for operation as numerics.rs:114-120 /
 * alignments.rs:129-160 do: bit-identical to the CPU arithmetic.
 * What modes 0 / 2 buy over mode 1: the reference resolves an EXACT tie between the DELETE and INSERT predecessors by taking
 * MATCH even when MATCH is larger; when such a tie arises by coincidence of two rounded f32 sums (real-valued features),
 * mode 1 -- whose distances differ in the last bit -- does not see a tie and keeps the smaller predecessor, and that entry can
 * differ by a few 1e-4 relative.  Counted over every entry of the BASELINE shapes (tests/test_gpu_census.py): none on cfg 2,
 * cfg 3 and cfg 5's shape, one pair of 8.4 million on cfg 4; over 60 corpora per shape 1-6 entries in 1e8, worst seen 2.2e-3
 * (tools/census_sweep.py).  Ties that are structural (identical frames, integer features,
 * +INF) are reproduced in every mode.
 * Feature range: all of the above holds for batches whose features are 0 or have 2^-40 <= |v| < 2^60 -- there every non-zero
 * squared distance and frame norm is a normal, finite f32.  A batch with any other value (apd_batch_nonfinite) is aligned by the
 * literal kernel whatever the mode: bit-identical to the CPU code, subnormal and overflowing distances included.  (Without that
 * routing modes 0 and 1 lose the tolerance once squared distances go subnormal: DESIGN.md section 6 has the measured table.) */
int apd_set_distance_mode(apd_context *ctx, int mode, float tau);
/* Device self-test of the cross-lane primitives the kernels rely on (DPP wave shifts). */
int apd_selftest(apd_context *ctx);
/* TEST HOOK: strict mode's square root (v_sqrt_f32 + an exact two-sided fix-up, csrc/dtw_common.h sqrt_rn_finite) against the
 * compiler's correctly rounded sqrtf (= Rust's f32::sqrt, numerics.rs:119) for the `count` (<= 2^32) consecutive f32 bit patterns
 * from first_bits, restricted to its domain 2^-96 <= x < +INF: *mismatches = how many differ (must be 0), *first_mismatch the
 * first such pattern, raw_ulp_hist[5] (may be NULL) = how often the bare v_sqrt_f32 is off by <= -2, -1, 0, +1, >= +2 ulps.
 * The whole f32 range takes about a second (tests/test_gpu_sqrt.py). */
int apd_selftest_sqrt(apd_context *ctx, uint32_t first_bits, uint64_t count, uint64_t *mismatches, uint32_t *first_mismatch,
                      uint64_t *raw_ulp_hist);
/* TEST HOOK: binds the calling thread to `bound`, then runs the library's affinity check for `checked` (see APD_DEBUG_AFFINITY
 * above): APD_OK if the check is off (*enabled = 0) or the two are the same context, APD_ERR_HIP with the text in
 * apd_last_error(checked) otherwise -- also when both contexts sit on the same device, which is the point. */
int apd_debug_affinity_probe(apd_context *bound, apd_context *checked, int *enabled);
/* TEST HOOK: *busy = 1 while work enqueued on the context's stream has not finished (hipStreamQuery), 0 once it is idle.  What the
 * "_async only enqueues" tests assert on, instead of wall-clock ratios. */
int apd_stream_busy(apd_context *ctx, int *busy);
/* TEST HOOK (fault injection): the next alignment launches leave the last `drop_tiles` tiles of every kernel class
 * unprocessed, as a launch that is cut short would.  0 = off.  Exists so that the poison / APD_ERR_INCOMPLETE path can
 * be tested (tests/test_gpu_dtw.py); never set it in production. */
int apd_set_fault_injection(apd_context *ctx, uint32_t drop_tiles);

/* ---- Discovery::alignment_params (src/discovery.rs:38-45) ----------------------------- */
int apd_discovery_alignment_params(const apd_align_config *cfg, uint64_t n_size, apd_alignment_params *out);

/* ---- AlignmentWorkers::new (src/alignments.rs:17-26) ---------------------------------- */
/* frames: packed [offsets[n_seq]][dim] f32 row-major (NDSequence.frames of every sequence,
 * spectrogram.rs:16-17, back to back); offsets: n_seq+1 frame offsets.  If frames_on_device
 * != 0, `frames` is a device pointer and stays owned by the caller (it is only read during
 * this call).  The batch keeps its own HBM copy in the kernels' padded layout. */
int apd_batch_create(apd_context *ctx, const float *frames, const uint64_t *offsets, uint32_t n_seq,
                     uint32_t dim, int frames_on_device, apd_batch **batch);
int apd_batch_destroy(apd_batch *batch);
uint32_t apd_batch_len(const apd_batch *batch);
/* New frame VALUES for the same sequence lengths (the same `offsets` and `dim` the batch was created with): re-runs only
 * the repack kernel, asynchronously on the context's stream; the batch keeps its device buffers and its cached tile
 * plans.  For pipelines that call align_all repeatedly on features recomputed in HBM (bench.py's step). */
int apd_batch_refill(apd_context *ctx, apd_batch *batch, const float *frames, int frames_on_device);
/* 1 if the resident frames hold a value outside the fast kernels' feature range: a NaN, an infinity, a magnitude of 2^60 or
 * more, or a NON-ZERO magnitude below 2^-40 (exact zeros are inside the range).  Then every pair goes through the literal kernel,
 * which computes operation for operation as the CPU code does: NaN compares false and takes the MATCH branch
 * (alignments.rs:153-159), an overflowing distance is +INF, an underflowing one the subnormal or 0 it is on the CPU -- scores
 * bit-identical to the CPU code in every distance mode, at the literal kernel's speed.  0 if every feature is 0 or has
 * 2^-40 <= |v| < 2^60.  Follows apd_batch_refill.  Synchronises. */
int apd_batch_nonfinite(apd_context *ctx, const apd_batch *batch, int *nonfinite);

/* ---- two sets in one batch: the cross alignment (the `cdist` next to align_all's `pdist`) ------------------------------
 * A resident batch holding the sequences of `first` followed by those of `second` (same context, same caller frame dimension,
 * else APD_ERR_INVALID_ARG).  Caller's sequence numbers: s < apd_batch_len(first) is first's sequence s, the others second's
 * s - apd_batch_len(first).  A snapshot: made from the two batches' resident frames by device-to-device copies on the context's
 * stream (no host round trip of frames, no synchronisation: the out-of-range flag of apd_batch_nonfinite is the OR of the two
 * inputs' flags, formed on the device); later refills of first / second are not followed.  Both inputs stay usable.
 * Resident order: two segments, each in its own length order; which set lies first is the library's choice (the one with the
 * larger mean length) and no result depends on it.  total frames + 2 * sequences >= 2^32 is APD_ERR_INVALID_ARG.
 * A joined batch is an ordinary batch for apd_batch_len / apd_batch_destroy / apd_destroy, apd_batch_nonfinite, apd_align_all*,
 * apd_align_tiles_async / apd_unpack_tiles_async (which use the batch's own order), apd_align_paths (the warping path between
 * a sequence of one set and one of the other) and apd_spot (templates of one set spotted in recordings of the other).
 * apd_batch_refill on it is APD_ERR_INVALID_ARG.  The host-only views that take raw offsets (apd_length_order, apd_rank_tile_list, apd_unpack_tiles_host, apd_align_work) describe LENGTH-ORDERED batches
 * only, not joined ones.  The multi-GPU entry points (apd_multi_*, apd_comm_*, apd_align_all_sharded_async) do not take the
 * cross alignment: out of scope. */
int apd_batch_join(apd_context *ctx, const apd_batch *first, const apd_batch *second, apd_batch **joined);
uint32_t apd_batch_first_len(const apd_batch *batch);   /* sequences of the first set; apd_batch_len for a plain batch */
/* out_fs: [n_first][n_second], out_fs[q][c] = Alignment::score(x = first q, y = second c);
 * out_sf: [n_second][n_first], out_sf[c][q] = score(x = second c, y = first q).  Either may be NULL.  Blocking / asynchronous
 * exactly as apd_align_all / apd_align_all_device_async; band per pair from max(len) as everywhere; distance modes, feature-range
 * routing to the literal kernel, poison + APD_ERR_INCOMPLETE, apd_set_variant, apd_set_timing / apd_last_kernel_ms and
 * apd_set_fault_injection all as for apd_align_all.  An empty set: APD_OK, nothing written.  A plain (not joined) batch:
 * APD_ERR_INVALID_ARG.  Only the tiles of the pair matrix that hold a first-second pair are swept. */
int apd_align_cross(apd_context *ctx, const apd_batch *joined, const apd_align_config *cfg, float *out_fs, float *out_sf);
int apd_align_cross_device_async(apd_context *ctx, const apd_batch *joined, const apd_align_config *cfg, float *d_out_fs,
                                 float *d_out_sf);

/* ---- AlignmentWorkers::align_all (src/alignments.rs:31-67) ---------------------------- */
/* out: n_seq*n_seq f32 row-major, out[i*n+j] = Alignment::score of (x = seq i, y = seq j),
 * diagonal 0.0 (alignments.rs:21-23,51,57).  Blocking. */
int apd_align_all(apd_context *ctx, const apd_batch *batch, const apd_align_config *cfg, float *out);
/* Same, result left in HBM (d_out: n_seq*n_seq floats); asynchronous on the context's stream. */
int apd_align_all_device_async(apd_context *ctx, const apd_batch *batch, const apd_align_config *cfg,
                               float *d_out);

/* Sharded form (the reference's static row blocks, alignments.rs:33-37, become pair tiles):
 * the sequences are taken in LENGTH ORDER (apd_length_order: longest first, equal lengths by
 * ascending index -- a batch keeps them resident in that order), and the upper triangle of the
 * n x n pair matrix over those positions is cut into apd_tile_size() x apd_tile_size() tiles, so
 * that the sequences of a tile have like lengths; rank r of `world` owns tiles r, r+world, ...
 * Each rank fills one packed slab of apd_slab_floats() floats; after an all-gather of the `world`
 * slabs (rank order) into d_gathered, apd_unpack_tiles_async scatters them into the n x n matrix
 * indexed by the caller's sequence numbers. */
uint32_t apd_tile_size(void);
uint64_t apd_num_tiles(uint32_t n_seq);
uint64_t apd_rank_tiles(uint32_t n_seq, uint32_t rank, uint32_t world);
uint64_t apd_slab_floats(uint32_t n_seq, uint32_t world);
/* "_async" for the alignment entry points (this one, apd_align_all_device_async, apd_align_all_sharded_async,
 * apd_multi_align_all_async) means what it says: the kernels, the collective and the unpack are only ENQUEUED when the call
 * returns, also right after apd_batch_create / apd_batch_refill.  The choice between the fast kernels and the literal,
 * CPU-faithful one (a batch with a NaN, an infinite feature or a non-zero one outside 2^-40 <= |v| < 2^60 must take the
 * latter: apd_batch_nonfinite) is made ON THE DEVICE: the repack kernel
 * leaves its verdict in a flag word, the fast kernels return at once when it is raised, and a small persistent launch of the
 * literal kernel behind them returns at once when it is not.  One exception: a band so wide that the literal kernel cannot
 * hold it in LDS (2w+1 > 20 480 offsets) -- then the first alignment after a fill reads the flag back on the host (4 bytes,
 * one synchronisation of the context's stream).  The first call on a new batch / band also builds the tile plan on the host
 * (a small upload and a stream synchronisation); later calls reuse it. */
int apd_align_tiles_async(apd_context *ctx, const apd_batch *batch, const apd_align_config *cfg,
                          uint32_t rank, uint32_t world, float *d_slab);
int apd_unpack_tiles_async(apd_context *ctx, const apd_batch *batch, uint32_t world, const float *d_gathered,
                           float *d_out);
/* ---- the same over several GPUs, collective included (RCCL over xGMI; no torch, no MPI) --------------------------
 * The reference runs `alignment_workers` threads over row blocks (alignments.rs:33-41); here a worker is a GPU.  Two ways
 * to bring the GPUs together:
 *
 * (1) one PROCESS PER GPU (how bench.py is launched): rank 0 calls apd_comm_unique_id and hands the 128 bytes to every
 *     rank over whatever channel the host has (a file, a socket, MPI, torch.distributed's store); every rank then calls
 *     apd_comm_create on its own context.  apd_align_all_sharded_async = this rank's tiles (apd_align_tiles_async) +
 *     ONE ncclAllGather of the equal-sized slabs on the context's stream + apd_unpack_tiles_async: afterwards EVERY
 *     rank holds the full n x n matrix in d_out (rank 0 is the consumer: UPGMA runs there).
 * (2) ONE process driving n_devices GPUs: apd_align_all_multi (ncclCommInitAll, one context + one resident copy of the
 *     batch per device, per-device streams, the same all-gather inside one ncclGroup, unpack on devices[0], copy to the
 *     host).  n_devices == 1 degenerates to apd_align_all and returns the identical bits. */
#define APD_COMM_ID_BYTES 128
int apd_comm_unique_id(void *id_bytes /* APD_COMM_ID_BYTES */);
int apd_comm_create(apd_context *ctx, const void *id_bytes, uint32_t rank, uint32_t world, apd_comm **comm);
int apd_comm_destroy(apd_comm *comm);
int apd_comm_count(const apd_comm *comm, uint32_t *world);   /* ncclCommCount: the ranks RCCL actually sees */
int apd_comm_rank(const apd_comm *comm, uint32_t *rank);     /* ncclCommUserRank */
/* d_out: n_seq*n_seq floats in this rank's HBM; the batch must hold the same sequences on every rank.  Asynchronous on
 * the context's stream.  With comm == NULL the call is apd_align_all_device_async (world 1). */
int apd_align_all_sharded_async(apd_context *ctx, apd_comm *comm, const apd_batch *batch, const apd_align_config *cfg,
                                float *d_out);
/* The same with the slab gathered by the caller's own transport between the two halves is apd_align_tiles_async +
 * apd_unpack_tiles_async below.  apd_all_gather_async is the library's collective on its own: d_send (count floats) of
 * every rank, concatenated in rank order into d_recv (count * world floats), on the context's stream. */
int apd_all_gather_async(apd_context *ctx, apd_comm *comm, const float *d_send, float *d_recv, uint64_t count);
/* frames / offsets / out: host memory, as apd_batch_create + apd_align_all take them.  devices: HIP device ordinals.
 * Blocking.  ONE-SHOT convenience over the persistent handle below (apd_multi_create + apd_multi_batch_create +
 * apd_multi_align_all + destroy): it pays communicator setup on every call -- a host that aligns more than once
 * (main.rs:187-195 in a loop) keeps an apd_multi instead. */
int apd_align_all_multi(const int *devices, uint32_t n_devices, const float *frames, const uint64_t *offsets, uint32_t n_seq,
                        uint32_t dim, const apd_align_config *cfg, float *out, uint32_t *ranks_seen);

/* The two one-call entry points SURVEY.md section 8(b) spells out for the Rust shim and the C++ harness -- the whole alignment leg
 * (AlignmentWorkers::new + align_all, src/alignments.rs:17-67, main.rs:187-195) and the whole clustering leg
 * (AgglomerativeClustering::clustering, src/clustering.rs:81-110) with host buffers in and out, the library owning contexts,
 * device buffers and communicators for the duration of the call.  Synchronous, thread-compatible, 0 = OK, nothing unwinds.
 * apd_dtw_all_pairs: frames [sum len][dim], offsets [n_seq + 1] in frames, out [n_seq][n_seq] caller-owned; devices 0 ..
 *   n_devices - 1 (n_devices <= 1: device 0 alone); default distance mode.  = apd_align_all_multi over those devices.
 * apd_upgma: dist [n][n] host, ops capacity >= n, roots capacity >= n; on device 0.  = apd_create + apd_clustering + apd_destroy.
 * A host that calls them more than once keeps an apd_multi / apd_context instead and saves the set-up. */
int apd_dtw_all_pairs(const float *frames, const uint64_t *offsets, uint32_t n_seq, uint32_t dim, float band_pct,
                      float ins_pen, float del_pen, float match_pen, int n_devices, float *out);
int apd_upgma(const float *dist, uint32_t n, float perc, apd_cluster_op *ops, uint32_t *n_ops, uint32_t *roots, uint32_t *n_roots);

/* ---- (2) as a persistent handle: AlignmentWorkers { data, result } (alignments.rs:11-14) over n_devices GPUs ---------
 * apd_multi owns, for its whole life: one apd_context per device (own stream), the RCCL communicators of
 * ncclCommInitAll, one host worker thread per device (the reference's `alignment_workers` threads, alignments.rs:35-41:
 * here a worker feeds a GPU), the gather workspaces and -- per apd_multi_batch -- one resident copy of the corpus and the
 * cached tile plans on every device.  Create once, align many: a second apd_multi_align_all pays kernels + one
 * all-gather + unpack only.
 * If RCCL cannot make the communicators (or APD_MULTI_COLLECTIVE=peer is set), the handle falls back to gathering the slabs
 * onto devices[0] with hipMemcpyPeerAsync; apd_multi_collective() says which and carries RCCL's error text.  Results are
 * the same bits either way (the collective only moves the slabs).  With the peer-copy collective forced a device may be named
 * several times in `devices` (several ranks on one GPU): a rehearsal aid for single-GPU boxes, nothing else. */
/* A handle is driven by ONE host thread at a time (its own worker threads are internal); different handles and contexts
 * may be used from different threads concurrently. */
typedef struct apd_multi apd_multi;
typedef struct apd_multi_batch apd_multi_batch;
int apd_multi_create(const int *devices, uint32_t n_devices, apd_multi **multi);
int apd_multi_destroy(apd_multi *multi);                     /* also destroys the batches still alive on it */
uint32_t apd_multi_size(const apd_multi *multi);             /* n_devices */
int apd_multi_ranks_seen(const apd_multi *multi, uint32_t *ranks);   /* ncclCommCount (n_devices in the peer-copy fallback) */
const char *apd_multi_collective(const apd_multi *multi);    /* "rccl: ..." or "peer-copy fallback: <why>" */
const char *apd_multi_last_error(const apd_multi *multi);    /* "device k: <text>" of the last failing call */
/* Device i's context, owned by the handle (never apd_destroy it): for the per-device settings (apd_set_distance_mode,
 * apd_set_timing, apd_set_variant), the feature kernels (apd_encode, apd_cepstrum_batch) and buffers on that device. */
apd_context *apd_multi_context(apd_multi *multi, uint32_t i);
/* AlignmentWorkers::new (alignments.rs:17-26) on every device.  Either `frames` (host, packed as for apd_batch_create,
 * uploaded to every device by its worker thread) or `d_frames` (n_devices device pointers, d_frames[i] in device i's
 * HBM, only read during the call) must be given. */
int apd_multi_batch_create(apd_multi *multi, const float *frames, const float *const *d_frames, const uint64_t *offsets,
                           uint32_t n_seq, uint32_t dim, apd_multi_batch **batch);
int apd_multi_batch_refill(apd_multi *multi, apd_multi_batch *batch, const float *frames, const float *const *d_frames);
int apd_multi_batch_destroy(apd_multi_batch *batch);
/* AlignmentWorkers::align_all (alignments.rs:31-67): every device aligns its pair tiles (g = i mod n_devices), ONE grouped
 * ncclAllGather, unpack on devices[0].  d_out: n_seq*n_seq floats in devices[0]'s HBM (NULL: a buffer owned by the handle,
 * see apd_multi_result).  Returns when every device's work is ENQUEUED; apd_multi_synchronize waits for all devices and
 * reports APD_ERR_INCOMPLETE like apd_synchronize. */
int apd_multi_align_all_async(apd_multi *multi, const apd_multi_batch *batch, const apd_align_config *cfg, float *d_out);
int apd_multi_synchronize(apd_multi *multi);
/* Device address (devices[0]) of the matrix the last apd_multi_align_all_async(.., d_out = NULL) wrote; NULL if none. */
const float *apd_multi_result(const apd_multi *multi);
/* Blocking form: out = n_seq*n_seq floats, host. */
int apd_multi_align_all(apd_multi *multi, const apd_multi_batch *batch, const apd_align_config *cfg, float *out);

/* ---- device buffers -------------------------------------------------------------------------------------------------
 * For hosts that keep features or the matrix resident between calls (what a Rust binding wraps in a Drop-ing DeviceVec):
 * plain hipMalloc / hipFree / hipMemcpy on the context's device, the copies ordered on the context's stream and
 * complete when the call returns.  apd_destroy releases the buffers of a context that were never freed (after which they
 * must not be passed to apd_device_free); freeing a pointer the context did not hand out is APD_ERR_INVALID_ARG. */
int apd_device_alloc(apd_context *ctx, uint64_t bytes, void **d_ptr);
int apd_device_free(apd_context *ctx, void *d_ptr);
int apd_copy_to_device(apd_context *ctx, void *d_dst, const void *src, uint64_t bytes);
int apd_copy_to_host(apd_context *ctx, void *dst, const void *d_src, uint64_t bytes);
int apd_device_fill(apd_context *ctx, void *d_dst, int byte_value, uint64_t bytes);   /* hipMemsetAsync on the stream */
/* Which HIP and RCCL libraries this process actually mapped for the library's calls (dladdr of hipMalloc /
 * ncclAllGather) and their versions, as one line of text; returns the length needed (incl. NUL). */
uint64_t apd_runtime_info(char *out, uint64_t capacity);

/* Host-side views of the same sharding (no GPU needed): the length order (order[p] = sequence at position p), the
 * (tile_a, tile_b) list of a rank over those positions, 2 uint32 per tile, and the scatter of gathered slabs held in
 * HOST memory (for a host that gathers over its own transport). */
int apd_length_order(const uint64_t *offsets, uint32_t n_seq, uint32_t *order);
int apd_rank_tile_list(uint32_t n_seq, uint32_t rank, uint32_t world, uint32_t *tile_ab, uint64_t capacity,
                       uint64_t *n_tiles);
int apd_unpack_tiles_host(const uint64_t *offsets, uint32_t n_seq, uint32_t world, const float *gathered, float *out);

/* Work accounting for the metric: cells = sum over ordered pairs of the
 * cells alignments.rs:174-175 visits; alg_bytes = sum of 4*dim*(n+m)+4. */
int apd_align_work(const uint64_t *offsets, uint32_t n_seq, uint32_t dim, const apd_align_config *cfg,
                   uint32_t rank, uint32_t world, uint64_t *pairs, uint64_t *cells, uint64_t *alg_bytes);

/* ---- Alignment::new + construct_alignment + score (src/alignments.rs:107-180) --------- */
/* x: [n][dim], y: [m][dim] host.  *score = Alignment::score() after construct_alignment(x, y, params). */
int apd_align_pair(apd_context *ctx, const float *x, uint64_t n, const float *y, uint64_t m, uint32_t dim,
                   const apd_alignment_params *params, float *score);

/* ---- warping paths: the alignment information of Alignment.sparse (src/alignments.rs:99-111,165-180) ----------------
 * The reference's one public result besides the score is its DP table; what a caller does with it is walk back from the score
 * cell (n-1, m-1) (alignments.rs:120) to see which frames were matched to which.  These two calls return that walk for a
 * caller-chosen list of ORDERED pairs of a resident batch, and for a single pair, backtracked on the GPU.
 * Table: sparse[(0,0)] = 0; cells (i, j), 1 <= i <= n, max(i-w, 1) <= j < min(i+w, m+1), w = max(band, |n-m|) + 2; every other
 * cell is absent and reads as +INF.  Each cell remembers the branch alignments.rs:153-159 took: DELETE (from (i, j-1)) if
 * del < match && del < ins, INSERT (from (i-1, j)) if ins < match && ins < del, MATCH (from (i-1, j-1)) otherwise -- so an exact
 * DELETE / INSERT tie takes MATCH even when MATCH is larger, and so does a NaN (compares false) and an all-INF node.
 * Walk: from (n-1, m-1); if that cell is absent (exactly one of n, m is 1) the path is empty and the score +INF; at (0,0) emit
 * START and stop; else emit the cell with its branch and move to that branch's predecessor, stopping if it is absent (row 0 /
 * column 0 other than the origin, outside the band).  A finite end cell always leads back to (0,0); only NaN / INF tables end
 * early.  The path is reported origin first, end cell last, at most n + m - 1 steps; n = m = 1 gives the single step
 * (0, 0, 0.0, START) and score 0.  i, j are the reference's 1-based table indices (the cell compares x[i-1] with y[j-1]); cost
 * holds the bits of sparse[(i,j)]; score = cost of the last step / (n + m) as f32 (alignments.rs:121).
 * Arithmetic: ALWAYS the literal one (numerics.rs:114-120, alignments.rs:153-159 operation for operation: every difference,
 * square and partial sum rounded on its own, correctly rounded square root, pen * d rounded, then added), whatever
 * apd_set_distance_mode says -- a path that disagrees with its own costs by an ulp is useless.  The score is therefore
 * bit-identical to the strict-mode (mode 2) matrix entry and to the CPU code; a default-mode (mode 1) matrix entry may differ
 * from it within that mode's documented 1e-4.  A batch outside the fast feature range (apd_batch_nonfinite) needs no special
 * routing here: NaN, infinite, overflowing and subnormal distances come out as on the CPU (NaN payloads aside). */
enum { APD_PATH_MATCH = 0, APD_PATH_INSERT = 1, APD_PATH_DELETE = 2, APD_PATH_START = 3 };
typedef struct apd_path_step {
    uint32_t i, j;
    float cost;
    uint32_t op;
} apd_path_step;   /* 16 bytes */
/* Step slots a pair of n x m frames owns: n + m - 1, 0 if either is 0.  Host only. */
uint64_t apd_path_bound(uint64_t n, uint64_t m);
/* pairs: [n_pairs][2] = (x, y) in the CALLER's sequence numbers; any order, repeats and x == y allowed; results in input order.
 * step_off (n_pairs + 1, always written, no GPU work needed for it): path p owns steps[step_off[p] .. step_off[p+1]),
 *   step_off[p+1] - step_off[p] = apd_path_bound(len x, len y); path_len[p] of those slots are used, the others are zeroed.
 * steps == NULL: sizes only.  capacity (in steps) < step_off[n_pairs]: APD_ERR_INVALID_ARG.  scores may be NULL.  A pair index
 * >= the batch's sequence count is APD_ERR_INVALID_ARG, an empty sequence in the batch APD_ERR_EMPTY_SEQUENCE, a pair whose band
 * needs 2w+1 > 20 480 offsets APD_ERR_BAND_TOO_WIDE (the literal kernel's limit), each before anything is launched.  Follows
 * apd_batch_refill.  Blocking.  With apd_set_timing on, apd_last_kernel_ms covers the two kernels of the call (all chunks).
 * Workspace: 2 bits per swept cell in words of 16 cells per lane, (len x + 63) * ceil(C / 16) * 256 bytes per pair with
 * C = max(ceil((2w+1) / 64), 2); a long list is cut into chunks that keep it under 1 GiB (APD_PATH_WORKSPACE_BYTES overrides
 * the cap: tests only), results identical. */
int apd_align_paths(apd_context *ctx, const apd_batch *batch, const apd_align_config *cfg, const uint32_t *pairs,
                    uint64_t n_pairs, apd_path_step *steps, uint64_t capacity, uint64_t *step_off, uint32_t *path_len,
                    float *scores);
/* Alignment::construct_alignment with its alignment information: explicit band, host frames, as apd_align_pair (whose
 * two-sequence batch it shares).  *n_steps = steps used (steps == NULL: apd_path_bound(n, m), nothing computed); capacity <
 * apd_path_bound(n, m) is APD_ERR_INVALID_ARG.  n = m = 0: *n_steps = 0, *score = +INF; one of them 0: APD_ERR_EMPTY_SEQUENCE. */
int apd_align_pair_path(apd_context *ctx, const float *x, uint64_t n, const float *y, uint64_t m, uint32_t dim,
                        const apd_alignment_params *params, apd_path_step *steps, uint64_t capacity, uint64_t *n_steps,
                        float *score);

/* ---- subsequence alignment ("spotting"): where does a template occur in a recording nobody has segmented? -------------------
 * Open-begin, open-end DTW of a query x (n >= 1 frames) against a stream y (m >= 1 frames): the recurrence above, with another
 * boundary.  Table T, 0 <= i <= n, 0 <= j <= m, cell (i, j) comparing x[i-1] with y[j-1]; T[0][j] = 0 for every j (an alignment may
 * start anywhere in the stream), T[i][0] = +INF for i >= 1; for i, j >= 1 alignments.rs:153-159 verbatim: DELETE from (i, j-1) if
 * del < match && del < ins, INSERT from (i-1, j) if ins < match && ins < del, MATCH from (i-1, j-1) otherwise (an exact DELETE /
 * INSERT tie takes MATCH even when MATCH is larger, and so does a NaN); value = predecessor + (pen * d rounded on its own), d the
 * euclidean distance of numerics.rs:114-120.  There is NO band (a band relative to an unknown start is not a DP): the table is
 * n x m cells and cfg->warping_band_percentage is not read.
 * Start column S[i][j], 1-based: in row 1 a MATCH or INSERT starts the alignment, S = j; everywhere else S is the S of the
 * predecessor the select chose (S[i][0] = 0: nothing starts there).
 * Curves, for j = 1 .. m at index j - 1: cost = T[n][j] (the table's bits), start = S[n][j]; the matched window is y[start-1 .. j-1],
 * L = j - start + 1 frames, and score(j) = cost / (float)(n + L), one f32 division: alignments.rs:121 with the window in place of y.
 * The reference reads its score one row and one column short, at (n-1, m-1) (alignments.rs:120); that is NOT carried over: the
 * reference has no spotting to stay identical to, and row n - 1 would leave a one-frame query without a row.
 * best: a scan of j ascending that keeps a column only if its score is strictly below the best so far, starting from +INF: the
 * smallest end wins ties, a NaN is never kept, nothing kept gives {0, 0, +INF, +INF}.
 * Arithmetic: ALWAYS the literal one, whatever apd_set_distance_mode says, as for the warping paths; a batch outside the fast
 * feature range needs no routing.
 * The warping path of a hit: apd_spot_paths below, which walks back through this very table.  (apd_align_pair_path on x and the
 * matched window fills another table, banded and anchored at both ends: its costs need not equal the curve's.) */
typedef struct apd_spot_best {
    uint32_t end, start;   /* 1-based stream columns of the window's last and first frame; 0, 0: none */
    float cost, score;
} apd_spot_best;   /* 16 bytes */
/* pairs: [n_pairs][2] = (query x, stream y) in the CALLER's sequence numbers of any resident batch -- usually a joined one,
 * templates joined with recordings; any order, repeats and x == y allowed; results in input order.
 * curve_off (n_pairs + 1, always written, no GPU work needed for it): pair p owns cost / start [curve_off[p] .. curve_off[p+1]),
 *   curve_off[p+1] - curve_off[p] = frames of y.  cost and start both NULL: best only (capacity is not read, no curve is stored
 *   anywhere); exactly one of them NULL, or capacity (in entries) < curve_off[n_pairs]: APD_ERR_INVALID_ARG.  best (n_pairs) may
 *   be NULL only if the curves are given; all three NULL: sizes only.
 * A pair index >= the batch's sequence count is APD_ERR_INVALID_ARG, an empty sequence in the batch APD_ERR_EMPTY_SEQUENCE, a query
 * of more than 16 384 frames (or a stream of 2^32 - 65 536 or more) APD_ERR_UNSUPPORTED, each before anything is launched.  Follows
 * apd_batch_refill.  Blocking.  With apd_set_timing on, apd_last_kernel_ms covers the kernels of the call (all chunks).
 * One wavefront sweeps one pair, whatever its size: the parallelism is pairs (templates x recordings).  A single long pair runs
 * on one wavefront; cutting a free-start DP along the stream into independent pieces is not exact and is not attempted
 * (sequential chunks that carry the last column are: "streaming spotting" below).
 * Workspace: 8 bytes per curve entry on the device; a long list is cut into chunks that keep it under 1 GiB
 * (APD_SPOT_WORKSPACE_BYTES overrides the cap: tests only), results identical. */
int apd_spot(apd_context *ctx, const apd_batch *batch, const apd_align_config *cfg, const uint32_t *pairs, uint64_t n_pairs,
             float *cost, uint32_t *start, uint64_t capacity, uint64_t *curve_off, apd_spot_best *best);
/* Greedy non-overlapping peak picking on ONE pair's curves (m entries, query of n >= 1 frames).  Host only, no context.
 * Candidates: the columns j with score(j) < threshold (strict, as merge()'s test is; a NaN score is no candidate), taken in
 * ascending score, the smaller end first among equal scores; a candidate is accepted if its window [start, end] shares no column
 * with an accepted one.  hits: the accepted windows in acceptance order, at most `capacity` written; *n_hits counts all of them and
 * may exceed capacity.  n == 0: APD_ERR_INVALID_ARG. */
int apd_spot_hits(const float *cost, const uint32_t *start, uint64_t m, uint64_t n, float threshold, apd_spot_best *hits,
                  uint64_t capacity, uint64_t *n_hits);

/* ---- spot detection: apd_spot and apd_spot_hits in one call on the device, per pair or with the templates of a stream competing --
 * Table, curves, score: exactly apd_spot's -- free start, no band, ALWAYS the literal arithmetic (apd_set_distance_mode is not
 * read); score(j) = cost / (float)(n + (j - start + 1)), one f32 division.  The curves never leave the device; only hits come back.
 * Candidates: column j of pair p is a candidate if score(j) < thresholds[p] (strict, as apd_spot_hits; a NaN score is never a
 * candidate, a NaN threshold gives none).  A column whose start is 0 is never a candidate: its alignment ran through column 0, so
 * its cost is +INF or NaN whatever the penalties (T[i][0] = +INF, and +INF plus any pen * d is +INF or NaN).
 * Groups.  APD_DETECT_PER_PAIR: group g is pair g -- apd_spot + apd_spot_hits, pair by pair.  APD_DETECT_PER_STREAM: group g is the
 * g-th distinct stream number y in order of first appearance in `pairs`, and all pairs of the list with that y belong to it, adjacent
 * in the list or not; a repeated pair is a member like any other.
 * Order inside a group: ascending score by f32 < (so -0.0 and +0.0 tie), then the smaller end, then the smaller pair index.  A group
 * holds one candidate per (pair, end), so this is a strict total order and the result depends on nothing else -- not on the
 * workspace cap, not on scheduling.
 * Greedy: candidates are taken in that order; one is accepted iff its window [start, end] shares no column with an accepted window
 * of its group.
 * Output: hits group-major, in acceptance order inside a group (rank 0, 1, ...); group g owns hits[hit_off[g] .. hit_off[g+1]).
 * hit_off (*n_groups + 1 entries; n_pairs + 1 slots always suffice), *n_groups and *n_hits are exact whatever `capacity`; only hits
 * whose global index is below `capacity` are written, nothing past it; hits == NULL with capacity == 0: counts only.  Disjoint windows
 * cover one column each at least, so a group has no more hits than its stream has frames: the sum over the groups of the frames of
 * the group's stream is a capacity that always suffices.
 * Errors, each before anything is launched: whatever apd_spot refuses, with its code (a pair index >= the batch's sequence count or
 * a batch of another context APD_ERR_INVALID_ARG, an empty sequence in the batch APD_ERR_EMPTY_SEQUENCE, a query of more than 16 384
 * frames or a stream at apd_spot's limit APD_ERR_UNSUPPORTED); compete other than 0 or 1, thresholds == NULL with n_pairs > 0,
 * hit_off, n_groups or n_hits NULL, capacity > 0 with hits == NULL: APD_ERR_INVALID_ARG; a group of more than 2^24 pairs:
 * APD_ERR_UNSUPPORTED.  n_pairs == 0: zero groups, hit_off[0] = 0, APD_OK.
 * Follows apd_batch_refill.  Blocking.  With apd_set_timing on, apd_last_kernel_ms covers the sweep and the detection kernels of the
 * call (all chunks).
 * Workspace: per curve entry 8 bytes of curves and a 16-byte candidate slot, plus 8 bytes per group and frame of its stream (the
 * accepted windows) -- 24 to 32 bytes per entry -- and 24 bytes per hit written.  A long list is cut into chunks of WHOLE groups
 * that keep this under 1 GiB (APD_SPOT_WORKSPACE_BYTES overrides the cap: tests only); a chunk holds at least one group even if
 * that group alone exceeds the cap; results identical whatever the cap. */
typedef struct apd_spot_hit {
    uint32_t pair;         /* index into `pairs` */
    uint32_t end, start;   /* 1-based stream columns, as apd_spot_best */
    float    cost, score;  /* the bits of apd_spot's curve at `end` and of its score there */
    uint32_t rank;         /* acceptance rank inside the hit's group, 0 = first accepted */
} apd_spot_hit;            /* 24 bytes */
#define APD_DETECT_PER_PAIR   0   /* every pair is its own group: apd_spot + apd_spot_hits, pair by pair */
#define APD_DETECT_PER_STREAM 1   /* all pairs of the list that share a stream y compete for its columns */
int apd_spot_detect(apd_context *ctx, const apd_batch *batch, const apd_align_config *cfg, const uint32_t *pairs, uint64_t n_pairs,
                    const float *thresholds, int compete, apd_spot_hit *hits, uint64_t capacity, uint64_t *hit_off,
                    uint64_t *n_groups, uint64_t *n_hits);

/* ---- spot score quantiles: the thresholds of apd_spot_detect from the data, without the curves leaving the device ---------------
 * "Each template fires on at most one column in a thousand of this background corpus": the 0.001 quantile of the template's scores
 * over that corpus, which is numerics::percentile (numerics.rs:125-133) over a group of score curves.
 * Table, curves, score: exactly apd_spot's -- free start, no band, ALWAYS the literal arithmetic (apd_set_distance_mode is not
 * read); score(j) = cost / (float)(n + (j - start + 1)), one f32 division.
 * Groups.  APD_QUANTILES_PER_PAIR: group g is pair g.  APD_QUANTILES_PER_QUERY: group g is the g-th distinct query number x in order
 * of first appearance in `pairs`, and all pairs of the list with that x belong to it, adjacent in the list or not -- a template's
 * scores pooled over every stream it is paired with.  APD_QUANTILES_ALL: one group, every pair of the list.
 * Population of a group: one entry per stream column j = 1 .. m of every pair of the group (a column whose start is 0 included: its
 * score is +INF or NaN); a repeated pair counts as often as it is listed.  entries[g] = sum of m over the group's pairs.
 * Value (numerics.rs:125-133 on that population): NaN scores are dropped, nans[g] is their count; the others are ordered ascending
 * by f32 <, +INF kept; the value is the element at k = (usize)((f32)entries[g] * perc[q]), an f32 product of the UNFILTERED length,
 * truncated and saturating (a negative or NaN perc gives 0), as apd_percentile computes it.  -0.0 and +0.0 tie and come back as
 * +0.0; otherwise the value is the bits of an element of the population.  It depends on nothing else -- not on the workspace cap,
 * not on scheduling.
 * A rank beyond the population, k >= entries[g] - nans[g] (the reference's numbers[n] panics, numerics.rs:132; every perc = 1.0
 * ends so): status[g * n_perc + q] = APD_ERR_INDEX and values[g * n_perc + q] = NaN (0x7FC00000) -- a NaN threshold makes
 * apd_spot_detect find nothing -- and the call still returns APD_OK, as apd_interesting_ranges_batch does for a recording that fails
 * on its own.  Every other status is APD_OK.
 * Output: values and status ([n_groups][n_perc]; n_pairs * n_perc slots always suffice; status may be NULL), group_of ([n_pairs]: the
 * group of every pair; may be NULL), entries and nans ([n_groups], n_pairs slots suffice; either may be NULL), *n_groups.
 * Errors, each before anything is launched or written: whatever apd_spot refuses, with its code (a pair index >= the batch's sequence
 * count or a batch of another context APD_ERR_INVALID_ARG, an empty sequence in the batch APD_ERR_EMPTY_SEQUENCE, a query of more than
 * 16 384 frames or a stream at apd_spot's limit APD_ERR_UNSUPPORTED); grouping other than 0, 1 or 2, n_perc == 0 or above
 * APD_SPOT_QUANTILES_MAX, perc, values or n_groups NULL: APD_ERR_INVALID_ARG; a group of more than 2^24 pairs: APD_ERR_UNSUPPORTED.
 * n_pairs == 0: zero groups, APD_OK.
 * Follows apd_batch_refill.  Blocking.  With apd_set_timing on, apd_last_kernel_ms covers the sweep and the select kernels of the
 * call (all chunks).
 * Workspace: per curve entry 8 bytes of curves; per pair 64 bytes; per (group, quantile) a 257-bin 64-bit histogram and 32 bytes.  A
 * long list is cut into chunks of WHOLE groups that keep this under 1 GiB (APD_SPOT_WORKSPACE_BYTES overrides the cap: tests
 * only); a chunk holds at least one group even if that group alone exceeds the cap; results identical whatever the cap.
 * APD_SPOT_QUANTILES_COLUMNS: the columns a workgroup of the select takes per step -- for tests that place stream lengths around it. */
#define APD_QUANTILES_PER_PAIR  0   /* group g is pair g */
#define APD_QUANTILES_PER_QUERY 1   /* group g: the g-th distinct query x in order of first appearance; all pairs with that x */
#define APD_QUANTILES_ALL       2   /* one group: every pair of the list (zero groups if n_pairs == 0) */
#define APD_SPOT_QUANTILES_MAX  8
#define APD_SPOT_QUANTILES_COLUMNS 256
int apd_spot_quantiles(apd_context *ctx, const apd_batch *batch, const apd_align_config *cfg, const uint32_t *pairs, uint64_t n_pairs,
                       int grouping, const float *perc, uint32_t n_perc, float *values, int32_t *status, uint64_t *group_of,
                       uint64_t *entries, uint64_t *nans, uint64_t *n_groups);

/* ---- warping paths of spotted windows: which query frame was matched to which stream frame inside a window ----------------------
 * Table: exactly apd_spot's T and S -- free start, no band, always the literal arithmetic -- with every cell also remembering the
 * branch alignments.rs:153-159 took: DELETE from (i, j-1), INSERT from (i-1, j), MATCH from (i-1, j-1) otherwise.  Not a table of
 * the window alone: an exact DELETE / INSERT tie takes MATCH even when MATCH is larger, so the cells inside a window depend on the
 * columns before it (x = [0, 1], y = [0, 1, 0], end 3: the curve says start 2, cost 2.0; columns 2..3 alone give cost 1.0).
 * Window: query x, stream y in the CALLER's sequence numbers of any resident batch, plain or joined; end and start are 1-based
 * stream columns as apd_spot's curves, best and apd_spot_hits report them.  end == 0 or start == 0 is "no window" (apd_spot's none
 * record, or a column whose alignment ran through column 0): 0 slots, path length 0, found_start 0, score +INF; not an error.
 * Walk: from (n, end) back; each cell is emitted with its branch and its table value and the walk moves to the branch's
 * predecessor; on reaching row 0 at column j0 it emits (0, j0, 0.0, APD_PATH_START) and stops.  j0 = S - 1 after a MATCH in row 1,
 * S after an INSERT in row 1; it may be 0.  The path is reported origin first, (n, end) last.  i, j are 1-based table indices, j
 * the absolute stream column; cost holds the bits of T[i][j], so the last step's cost is bit-identical to apd_spot's cost curve at
 * `end`.  With S >= 1 the walk never enters column 0 and stays inside columns S .. end; its first cell after START is (1, S) with
 * MATCH or INSERT; it has between max(n, L) + 1 and n + L steps, L = end - S + 1.
 * The caller's start is checked, not trusted: found_start[p] = S[n][end] as the sweep carried it, scores[p] = T[n][end] /
 * (float)(n + end - S + 1), the bits of apd_spot's score at that column -- both written whether or not the start matches, either
 * may be NULL.  found_start[p] != start (S = 0 with a start >= 1 included): path_len[p] = 0, the window's slots zeroed, the call
 * still APD_OK; ask again with the start found. */
typedef struct apd_spot_window {
    uint32_t x, y;         /* query and stream */
    uint32_t end, start;   /* 1-based stream columns of the window's last and first frame, as in apd_spot_best */
} apd_spot_window;   /* 16 bytes */
/* Step slots a window owns: n + (end - start + 1) for n >= 1 and 1 <= start <= end, else 0.  Host only. */
uint64_t apd_spot_path_bound(uint64_t n, uint64_t end, uint64_t start);
/* windows: any order, repeats, overlaps and windows of one pair allowed; results in input order.
 * step_off (n_windows + 1, always written, no GPU work needed for it): window p owns steps[step_off[p] .. step_off[p+1]),
 *   step_off[p+1] - step_off[p] = apd_spot_path_bound(len x, end, start); path_len[p] of those slots are used, the others zeroed.
 * steps == NULL: sizes only.  capacity (in steps) < step_off[n_windows]: APD_ERR_INVALID_ARG.
 * x or y >= the batch's sequence count, start > end, or end > frames of y: APD_ERR_INVALID_ARG; an empty sequence in the batch
 * APD_ERR_EMPTY_SEQUENCE; a query of more than 16 384 frames or a stream at apd_spot's limit APD_ERR_UNSUPPORTED; each before
 * anything is launched.  Follows apd_batch_refill.  Blocking.  With apd_set_timing on, apd_last_kernel_ms covers all kernels of the
 * call.  apd_set_distance_mode is not read; a batch outside the fast feature range needs no routing.
 * A (query, stream) pair is swept ONCE per chunk however many of its windows the chunk holds, from column 1 to the largest end
 * asked for; the branches are kept only for the columns the windows cover (merged into disjoint intervals).  Workspace: 2 bits per
 * kept cell in words of 16 rows per lane, (L + 63) * ceil(ceil(n / 64) / 16) * 256 bytes per interval of L columns, plus the
 * steps; a long list is cut into chunks that keep each under 1 GiB (APD_SPOT_WORKSPACE_BYTES overrides the cap: tests only); a
 * chunk holds at least one window; results identical whatever the cap. */
int apd_spot_paths(apd_context *ctx, const apd_batch *batch, const apd_align_config *cfg, const apd_spot_window *windows,
                   uint64_t n_windows, apd_path_step *steps, uint64_t capacity, uint64_t *step_off, uint32_t *path_len,
                   uint32_t *found_start, float *scores);

/* ---- streaming spotting: a recording that arrives in chunks, the table's last column kept on the device --------------------------
 * apd_spot needs the whole recording resident.  Spotting each piece on its own is wrong, not merely approximate (the tie rule makes
 * the cells of a window depend on the columns before it, see above), but SEQUENTIAL chunks are exact: column j of T and S depends
 * on column j - 1 and on nothing else.  A session keeps, for every pair, rows 1 .. n of the last pushed column (value and start)
 * and the running best on the device, and a push continues that very table.
 * The promise: take any split of a stream y into chunks, zero-length ones included, and concatenate the curves of the pushes in
 * order: the result is bit-identical to apd_spot of (x, y) in a joined batch; best after any push is apd_spot's best of the prefix
 * pushed so far, bit for bit.  With first_column = b every start and end is shifted by b; costs and scores keep their bits.
 * templates: any resident batch, plain or joined; it must outlive the session.  queries (n_queries of them, repeats allowed): the
 *   caller's sequence numbers.  The session reads the batch's resident frames at every push: it follows apd_batch_refill, and a
 *   refill in mid-stream continues the OLD table with the NEW rows (call apd_spot_stream_reset for a fresh one).  Of cfg only the
 *   three penalties are read; there is no band.
 * n_channels independent streams (microphones, files); pair p = channel * n_queries + q.  Device state per pair: 8 bytes per row
 *   (rounded up to whole rows per lane) twice -- a push reads one copy and writes the other -- plus a 16-byte best.  A fresh or
 *   reset channel holds column 0 of the table (+INF / 0) and best {0, 0, +INF, +INF}.
 * Arithmetic: the literal one, always; apd_set_distance_mode is not read, no feature-range routing.  One wavefront per pair, as for
 * apd_spot: the parallelism is templates x channels.  A chunk of m columns costs m + (lane of row n) macro-steps, so chunks much
 * shorter than 64 columns pay mostly for filling the wavefront.
 * Warping paths of windows found while streaming: a session that keeps a history of its last columns traces them itself
 * ("a kept history of columns" below).  apd_spot_paths needs the table from column 1, so it serves only a recording that was kept. */
typedef struct apd_spot_stream apd_spot_stream;
/* A query index >= the batch's sequence count, n_queries * n_channels == 0 or >= 2^24, or a batch of another context:
 * APD_ERR_INVALID_ARG; an empty query APD_ERR_EMPTY_SEQUENCE; one of more than 16 384 frames APD_ERR_UNSUPPORTED.  Blocking. */
int apd_spot_stream_create(apd_context *ctx, const apd_batch *templates, const apd_align_config *cfg, const uint32_t *queries,
                           uint32_t n_queries, uint32_t n_channels, apd_spot_stream **stream);
/* As for batches: apd_destroy releases the device side of a session still alive, and afterwards only this call is legal on it. */
int apd_spot_stream_destroy(apd_spot_stream *stream);
/* channel (0xFFFFFFFF: every channel) starts over: column 0, no best, and its next frame is absolute column first_column + 1.
 * channel >= n_channels: APD_ERR_INVALID_ARG; first_column >= 2^32 - 65 536: APD_ERR_UNSUPPORTED.  Blocking. */
int apd_spot_stream_reset(apd_context *ctx, apd_spot_stream *stream, uint32_t channel, uint64_t first_column);
/* *columns = absolute column of the channel's last pushed frame: first_column + frames pushed since the reset.  Host only. */
int apd_spot_stream_columns(const apd_spot_stream *stream, uint32_t channel, uint64_t *columns);
/* frames: packed [chunk_off[n_channels]][dim] f32, host or (frames_on_device != 0) device -- device frames never visit the host;
 *   channel k's chunk is frames[chunk_off[k] .. chunk_off[k+1]), chunk_off[0] = 0.  dim must be the frame dimension the templates
 *   were created with.  Lengths may differ per channel and may be 0: a no-op for that channel.
 * curve_off (n_pairs + 1, always written, no GPU work needed for it): pair p owns as many entries as its channel's chunk has frames.
 * cost[e], start[e]: T[n][J] and S[n][J] of the chunk's columns, J and S absolute (J = apd_spot_stream_columns before the push + 1,
 *   + 2, ...).  best[p]: apd_spot's scan (strict <: the smallest end wins, a NaN is never kept) continued over everything pushed
 *   since the reset, end and start absolute.
 * cost and start both NULL: best only, no curve is stored anywhere; exactly one of them NULL, or capacity (in entries) <
 * curve_off[n_pairs]: APD_ERR_INVALID_ARG; best may be NULL only if the curves are given; all three NULL: sizes only, the state is
 * not advanced.
 * Errors, each before anything is launched and with the state untouched: a dim mismatch, a foreign context, descending chunk_off or
 * 2^32 - 2 frames or more in one push: APD_ERR_INVALID_ARG; a push that would take a channel's absolute column to 2^32 - 65 536 or
 * beyond: APD_ERR_UNSUPPORTED.  After APD_ERR_HIP / APD_ERR_OOM the state is undefined until apd_spot_stream_reset.
 * Blocking; one synchronisation per push, no allocation once the session's buffers have grown to the largest push seen.  With
 * apd_set_timing on, apd_last_kernel_ms covers the push's kernels: the repack of the chunk and one sweep per kernel class. */
int apd_spot_stream_push(apd_context *ctx, apd_spot_stream *stream, const float *frames, const uint64_t *chunk_off, uint32_t dim,
                         int frames_on_device, float *cost, uint32_t *start, uint64_t capacity, uint64_t *curve_off,
                         apd_spot_best *best);

/* ---- streaming spotting, a kept history of columns: warping paths of windows found while streaming ------------------------------
 * A window [S, end] is walked back only through cells of columns S .. end, and the session sweeps those very cells of the very
 * table once, as the chunks arrive.  A session that keeps, for its last H columns, the branch of every cell, row n's value and
 * start and the stream's frames can trace every window that still lies inside those columns -- with the results of apd_spot_paths
 * on the whole stream, at a cost that does not grow with the age of the stream and without the recording.
 *
 * apd_spot_stream_keep: from now on the session keeps the last history_columns pushed columns of every channel; 0 releases the
 * history.  Legal at any time, in mid-stream and repeatedly.  The table is not touched: curves and bests of later pushes keep their
 * bits.  The history starts EMPTY behind each channel's current column (its "origin"): windows that start at or before
 * apd_spot_stream_columns at the time of the call are not traceable, whatever was kept before.  Blocking.  APD_ERR_OOM leaves the
 * session exactly as before the call, its previous history included.  A foreign context: APD_ERR_INVALID_ARG.
 * Device memory, H = history_columns, R = ceil(n / 64) rows per lane of a query of n frames:
 *     per pair:     H * (ceil(R / 16) * 256 + 8) bytes    2 bits per cell in words of 16 rows per lane, 64 lanes; row n's value and start
 *     per channel:  H * 4 * ceil4(dim + 1) bytes          one resident frame per column
 * While a history is kept a push runs recording kernels (the same sweep, one more coalesced 256-byte store per macro-step and
 * word); a session without one runs the kernels it always ran. */
int apd_spot_stream_keep(apd_context *ctx, apd_spot_stream *stream, uint32_t history_columns);
/* The absolute columns [*first, *last] of `channel` whose cells are kept: last = apd_spot_stream_columns, first = max(origin + 1,
 * last - H + 1); nothing kept (no history, or nothing pushed since the origin): first = last + 1.  apd_spot_stream_reset of a
 * channel empties its history, with the origin at the new first_column.  Host only. */
int apd_spot_stream_history(const apd_spot_stream *stream, uint32_t channel, uint64_t *first, uint64_t *last);
/* apd_spot_paths for the windows of a session.  windows[p]: x = index into the session's `queries`, y = channel, end and start
 * absolute columns as a push reports them (a record of `best` can be handed over as it is).  Slots, step_off, sizes only (steps ==
 * NULL, legal with or without a history), zeroed unused slots, results in input order, path_len / found_start / scores and the
 * workspace cap (APD_SPOT_WORKSPACE_BYTES) exactly as for apd_spot_paths; a window owns apd_spot_path_bound(n, end, start) slots.
 * The promise: for a window whose columns start .. end all lie in [first, last] of its channel (apd_spot_stream_history), steps (i,
 * j, the bits of cost, op), path_len, found_start and scores are those of apd_spot_paths on the whole stream since the reset, in a
 * joined batch -- j, found_start (unless 0) and the START step's column shifted by the channel's first_column -- and no bit of a
 * cost or score differs, whatever the chunking of the pushes, zero-length chunks and pushes longer than H included.
 * The caller's start is checked against the kept S[n][end], not trusted, as there.
 *   end inside the history, start (or the start found) before `first`: found_start and scores as above, path_len = 0, the slots
 *     zeroed, APD_OK: the window has aged out; found_start == start tells it from a wrong start.
 *   end before `first`: path_len = 0, found_start = 0, score +INF, the slots zeroed, APD_OK.
 *   end == 0 or start == 0: "no window", as for apd_spot_paths.
 * Before anything is launched: x >= n_queries, y >= n_channels, start > end (with end >= 1) or end beyond the channel's pushed
 * column: APD_ERR_INVALID_ARG; a foreign context: APD_ERR_INVALID_ARG; steps != NULL on a session that keeps no history:
 * APD_ERR_UNSUPPORTED, with a text in apd_last_error.  Blocking.  With apd_set_timing on, apd_last_kernel_ms covers the traces.
 * The replay reads the templates' resident rows: after an apd_batch_refill the kept branches belong to the OLD rows; reset the
 * channel, as for the table.  Workspace: the steps of a chunk of windows; nothing else is allocated. */
int apd_spot_stream_paths(apd_context *ctx, apd_spot_stream *stream, const apd_spot_window *windows, uint64_t n_windows,
                          apd_path_step *steps, uint64_t capacity, uint64_t *step_off, uint32_t *path_len, uint32_t *found_start,
                          float *scores);

/* ---- streaming spotting, online detection: hold-off hits from a session, the curves never leaving the device ---------------------
 * apd_spot_detect takes candidates in global score order, so on a stream a hit would be final only when the stream ends.  An armed
 * session runs another contract: a causal machine per group, a function of the curves alone -- so the chunking of the pushes
 * changes nothing -- that reports a hit at most holdoff + 1 columns after the hit's end.
 * Candidates: column j (absolute, as a push reports it) of session pair p = channel * n_queries + q is a candidate iff
 * score(j) < thresholds[p] and start(j) != 0, with score(j) = cost / (float)(n + (j - start + 1)) on the bits a push would put in
 * its curves: the sweep's own expression, one f32 division.  The test is strict; a NaN on either side gives no candidate, a NaN
 * threshold none at all (apd_spot_detect's rules).
 * Groups.  APD_DETECT_PER_PAIR: group g is pair g.  APD_DETECT_PER_STREAM: group g is channel g and its n_queries pairs compete: at
 * column j the group has at most ONE candidate, the one among its pairs with the smallest score by f32 < (-0.0 and +0.0 tie), the
 * smaller p among equal scores.  This reduction is part of the definition: the column's other candidates do not exist below.
 * The machine, per group, over the columns in ascending order.  State: a pending window P or none; a floor F, the end of the
 * group's last emitted hit; a rank counter.  With c the group's candidate at column j, in this order:
 *   1. timer: if P exists and j - P.end > holdoff: emit P, F = P.end, no P.
 *   2. no c: the column is done.
 *   3. c.start <= F: discard c (it shares a column with an emitted hit).
 *   4. else no P: P = c.
 *   5. else c.start <= P.end (overlap; c.end = j > P.end): P = c if c.score < P.score by f32 <, else discard c -- an equal score
 *      keeps the earlier end.
 *   6. else (disjoint): emit P, F = P.end, P = c.
 * Emitting writes an apd_spot_hit: pair = p; end and start absolute; cost and score the curve's bits (a zero score keeps its
 * sign); rank = the group's emissions since arming, from 0.  holdoff == 0xFFFFFFFF never fires the timer.
 * Consequences: a group's emitted windows are pairwise disjoint and their ends ascend; a hit is emitted by the push that contains
 * column end + holdoff + 1, or earlier.
 * The promise: after any sequence of pushes the hits emitted so far are exactly what the machine emits up to each channel's current
 * column, the records bit for bit, whatever the chunking -- zero-length chunks and pushes longer or shorter than holdoff included.
 * A session that is not armed runs the kernels it always ran and returns the bits it always returned.
 *
 * apd_spot_stream_detect arms the session, or arms it again; thresholds ([n_channels][n_queries], host) == NULL disarms it and
 * releases the detector's device memory.  Legal at any time; the table, the curves and the bests of later pushes keep their bits.
 * Every group starts with no pending window, rank 0 and F = its channel's current column (apd_spot_stream_columns), the detector's
 * origin as apd_spot_stream_keep's: a window that starts at or before the origin is never reported.  Arming again and disarming
 * DISCARD pending windows and hits not yet drained: drain first (apd_spot_stream_flush, apd_spot_stream_hits).  compete other than
 * 0 or 1 (read even when disarming) or a foreign context: APD_ERR_INVALID_ARG.  APD_ERR_OOM leaves the session as it was.
 * Blocking.  Device memory: 8 bytes per pair, 32 bytes per group, 24 bytes per slot of the hit queue.
 *
 * apd_spot_stream_push on an armed session keeps its signature and every rule above ("all three NULL: sizes only, the state is not
 * advanced" included).  Any other push also runs the machine over the chunk's columns of every group: the sweeps write their
 * curves to the session's device buffer whether or not the caller asked for them on the host (8 bytes per curve entry of the
 * largest push seen), one more kernel on the same stream reads them, and emitted hits are appended to a queue on the device.  Still
 * one synchronisation per push; the count of queued hits comes back with it.  No hit is ever dropped: a group emits at most
 * (chunk columns + 1) hits per push, and the queue is grown to the queued count plus that bound BEFORE anything is launched; if it
 * cannot grow: APD_ERR_OOM with nothing enqueued and the state untouched. */
int apd_spot_stream_detect(apd_context *ctx, apd_spot_stream *stream, const float *thresholds, int compete, uint32_t holdoff);
/* Emits every pending window of the groups of `channel` (0xFFFFFFFF: every channel) as if its timer had fired, F = the emitted
 * window's end.  The stream may go on afterwards.  Not armed: APD_ERR_UNSUPPORTED, with a text in apd_last_error; channel >=
 * n_channels or a foreign context: APD_ERR_INVALID_ARG.  Blocking. */
int apd_spot_stream_flush(apd_context *ctx, apd_spot_stream *stream, uint32_t channel);
/* *n_hits = the hits queued.  capacity >= *n_hits: all are written and the queue is emptied.  Otherwise (hits == NULL with
 * capacity 0 included): nothing is written, nothing is consumed, APD_OK.  Order: ascending group, then ascending rank -- so it does
 * not depend on how the pushes were cut; a hit's group is its pair (per pair) or pair / n_queries (per stream).  Not armed: *n_hits
 * = 0, APD_OK.  n_hits == NULL, hits == NULL with hits to write, or a foreign context: APD_ERR_INVALID_ARG.  Blocking.
 * apd_spot_stream_reset of a channel also clears the pending windows of the channel's groups and sets their F to the new
 * first_column; the rank is NOT restarted, so (group, rank) stays unique in the queue, and hits already emitted stay queued.
 * A hit can be handed to apd_spot_stream_paths as the window {x = pair % n_queries, y = pair / n_queries, end, start}. */
int apd_spot_stream_hits(apd_context *ctx, apd_spot_stream *stream, apd_spot_hit *hits, uint64_t capacity, uint64_t *n_hits);

/* ---- numerics::percentile (src/numerics.rs:125-133) ----------------------------------- */
/* x: len floats, host or (x_on_device != 0) device. */
int apd_percentile(apd_context *ctx, const float *x, uint64_t len, float perc, int x_on_device, float *value);

/* ---- AgglomerativeClustering::clustering (src/clustering.rs:81-110) ------------------- */
/* distances: n*n host (or device if distances_on_device).  ops capacity >= n, roots capacity >= n.
 * roots = dendrogram.clusters() in ascending id order (the reference returns a HashSet).
 * Workspace: about 6 n^2 floats of device memory for the duration of the call (cluster sums, row-sum predictions, the two working
 * copies of the matrix and the buffers they are re-laid out into, member lists); APD_ERR_OOM if it does not fit.
 * Environment (tests / measurement only; results are bit-identical whatever they say): APD_UPGMA_TWO_LAUNCH=0|2 (always / never
 * replay the segment launches), APD_UPGMA_DEFRAG=<merges> (least number of merges between two re-layouts, 0 = never; default 128
 * from n = 2048 on), APD_UPGMA_SEGMENT_BLOCKS=<workgroups> (grid of the segment launch: a multiple of 64, at least 64),
 * APD_UPGMA_SHORT_CHAIN=<elements> (longest chain one wavefront sums whole: at least 64, default 8192).  Set to anything:
 * APD_UPGMA_DEFRAG_ALWAYS (re-lay out every <merges> merges, whatever they gathered), APD_UPGMA_NO_GRAPH (plain launches instead
 * of graph replay, for profilers), APD_DEBUG_UPGMA (progress of every batch on stderr), APD_DEBUG_UPGMA_TIMING (phase stamps on
 * stderr). */
int apd_clustering(apd_context *ctx, const float *distances, int distances_on_device, uint32_t n,
                   float perc, apd_cluster_op *ops, uint32_t *n_ops, uint32_t *roots, uint32_t *n_roots,
                   float *threshold);
/* AgglomerativeClustering::cluster_sets (src/clustering.rs:40-76); host-only bookkeeping.
 * members capacity >= n + n_ops + 2, set_off capacity >= n_roots+1. */
int apd_cluster_sets(const apd_cluster_op *ops, uint32_t n_ops, const uint32_t *roots, uint32_t n_roots,
                     uint32_t n, uint32_t *members, uint32_t *set_off, uint32_t *n_sets);
/* Cuts of a dendrogram; host-only bookkeeping.  The merge sequence does not depend on the threshold, so a run of apd_clustering at a
 * lower threshold is a prefix of a run at a higher one.  apd_dendrogram_cut replays the loop condition of clustering.rs:104-108:
 *   kept = 0; distance = 0.0f; while (kept < n_ops && distance < threshold) { distance = ops[kept].distance; ++kept; }
 * so the operation that reaches the threshold is kept, as the reference keeps it, and a NaN threshold or one <= 0 keeps nothing.  If
 * ops came from apd_clustering at threshold T, then for t <= T the first *n_kept of them are exactly what apd_clustering returns at t.
 * apd_cut_labels is assignment() (clustering.rs:115-128) after the first n_kept merges: labels[i] = i for an instance never merged,
 * otherwise the `into` of the last kept operation whose subtree holds i -- singletons keep a label, which apd_cluster_sets cannot
 * give.  labels: [n].  APD_ERR_INVALID_ARG, with nothing written, unless for every operation t < n_kept: into == n + t, and merge_i
 * and merge_j are distinct and each a current root (an instance < n or an earlier `into`, not merged since). */
int apd_dendrogram_cut(const apd_cluster_op *ops, uint32_t n_ops, float threshold, uint32_t *n_kept);
int apd_cut_labels(const apd_cluster_op *ops, uint32_t n_kept, uint32_t n, uint32_t *labels);

/* Average linkage of every first-set sequence to clusters of the second set, from the two cross matrices of apd_align_cross:
 * clustering.rs:153-170 with each first-set sequence q as a cluster of its own and set k of the second set as the other:
 *   link_fs[q][k] = (((0 + fs[q][y1]) + fs[q][y2]) + ...) / (1.0f * (float)|S_k|)     y ascending over S_k
 *   link_sf[q][k] = (((0 + sf[x1][q]) + sf[x2][q]) + ...) / ((float)|S_k| * 1.0f)     x ascending over S_k
 * f32, one rounded add per member in ASCENDING sequence number whatever order `members` lists them (the reference loops x, y
 * over 0..n); an empty set gives 0/0 = NaN as the reference would.  members / set_off / n_sets: as apd_cluster_sets returns them
 * (sequence numbers of the second set; >= n_second is APD_ERR_INVALID_ARG); singletons the caller wants considered are sets of one.
 * nearest[q]: merge()'s choice (clustering.rs:178-187) among the ordered pairs that involve q: scan k ascending, link_fs[q][k]
 * then link_sf[q][k], keep a value only if it is strictly below the best so far, starting from +INF; nearest_linkage[q] that
 * value; none kept (all +INF / NaN, or n_sets = 0): 0xFFFFFFFF and +INF.
 * fs: [n_first][n_second], sf: [n_second][n_first]; fs / sf / outputs: host, or all device pointers if on_device (matrices and
 * results stay in HBM; the call waits once for the upload of the member lists, the kernels are only enqueued on the context's
 * stream).  link_fs, link_sf: [n_first][n_sets], may be NULL.  members / set_off: always host. */
int apd_cross_linkage(apd_context *ctx, const float *fs, const float *sf, int on_device, uint32_t n_first, uint32_t n_second,
                      const uint32_t *members, const uint32_t *set_off, uint32_t n_sets,
                      float *link_fs, float *link_sf, uint32_t *nearest, float *nearest_linkage);

/* ---- nearest neighbours: the k smallest entries of rows or columns of a distance matrix ---------------------------------------
 * distances: row-major [rows][cols], square or not: the matrix of apd_align_all, or a cross matrix of apd_align_cross.  Query q
 * ranks the entries d[q][j], j < cols (APD_NEIGHBORS_ROWS) or d[j][q], j < rows (APD_NEIGHBORS_COLUMNS); the matrices are not
 * symmetric (the band is [-w, w-1]), so the two are different questions.
 * queries: HOST array of n_queries row (ROWS) or column (COLUMNS) numbers, in any order, repeats allowed, each answered on its own;
 * NULL: every row / column ascending, n_queries is not read.  Q is the number of queries.
 * The candidates of query q are its entries (j, v) with v not NaN and, if skip_self, j != q (a plain comparison of numbers, for
 * rectangular matrices too: pass 0 for cross matrices).  They are ordered ascending by (v, j): v under IEEE `<` -- -0.0 and +0.0
 * tie, +INF is a candidate behind every finite value -- and equal values by the smaller j.  Then
 *   count[q] = min(k, candidates); index[q][s], distance[q][s] for s < count[q]: j and the matrix's own bits of v (a -0.0 comes
 *   back as -0.0); the slots behind them hold 0xFFFFFFFF and a quiet NaN (0x7FC00000); nans[q] (nans may be NULL) = NaN entries of
 *   the row / column, not counting a skipped self entry.
 * A function of the matrix alone, bit for bit: no workgroup size, schedule or workspace size enters it.
 * index, distance: [Q][k]; count, nans: [Q]; host, or all device pointers if on_device (the matrix and the results stay in HBM; the
 * call waits once for the upload of the query list -- not at all without one -- and the kernels are only enqueued on the context's
 * stream, as apd_cross_linkage does).  Otherwise the call blocks.
 * APD_ERR_INVALID_ARG, before anything is launched or written: k == 0, k > APD_NEIGHBORS_MAX_K, another axis, a query >= rows (ROWS)
 * or >= cols (COLUMNS).  Q == 0: APD_OK, nothing written; rows == 0 or cols == 0 with Q > 0: counts of 0 and padding.  k larger
 * than a row is fine: the tail is padding.
 * Rows of up to 32768 entries are read from HBM once and kept in LDS; longer ones are re-read per digit pass.  COLUMNS gathers the
 * queried columns into a [panel][rows] workspace of the context (256 MiB) and ranks its rows, in as many panels as it takes.
 * Environment (tests only; read at every call; results are bit-identical whatever they say): APD_NEIGHBORS_LDS_COLUMNS=<entries>
 * lowers the LDS residency limit, APD_NEIGHBORS_WORKSPACE_BYTES=<bytes> sets the panel workspace (at least one column is taken),
 * APD_NEIGHBORS_WORKGROUP=<64 .. 1024, a multiple of 64> sets the work-items of a select workgroup (default 256 for rows of up to
 * 8192 entries, 512 or 1024 beyond). */
#define APD_NEIGHBORS_ROWS    0
#define APD_NEIGHBORS_COLUMNS 1
#define APD_NEIGHBORS_MAX_K   1024
int apd_neighbors(apd_context *ctx, const float *distances, int on_device, uint32_t rows, uint32_t cols, int axis,
                  const uint32_t *queries, uint32_t n_queries, uint32_t k, int skip_self,
                  uint32_t *index, float *distance, uint32_t *count, uint32_t *nans);

/* ---- silhouette: how well n_cuts cluster assignments ("cuts") fit the distance matrix, in one pass over it ---------------------
 * distances: the [n][n] matrix of apd_align_all.  labels: HOST [n_cuts][n], arbitrary uint32 values per cut (they need not be dense;
 * apd_cut_labels gives them for cuts of a dendrogram).  The matrix is directed, so axis chooses as for apd_neighbors:
 * APD_NEIGHBORS_ROWS: dist(i, y) = d[i][y] ({i} is the x cluster of clustering.rs:153-170); APD_NEIGHBORS_COLUMNS: dist(i, y) = d[y][i].
 * Bit for bit, for cut c and instance i, with C(y) the label of y in that cut:
 *   sum(i, L) = ((0.0f + dist(i, y1)) + dist(i, y2)) + ... over the y with C(y) == L and y != i, ascending: f32, one rounded add per
 *     term; the diagonal entry is skipped, not added.  cnt(i, L): the number of terms.
 *   a(i) = sum(i, C(i)) / (float)cnt(i, C(i)); a singleton (cnt(i, C(i)) == 0) has a(i) = 0.0f and s(i) = 0.0f.
 *   b(i), nearest(i): scan the labels L != C(i) in ascending label value, mean = sum(i, L) / (float)cnt(i, L); keep a mean only if it is
 *     strictly below the best so far under IEEE `<`, starting from +INF -- the smaller label wins ties, -0.0 and +0.0 tie, NaN is
 *     never kept.  nearest(i) is the kept label; nothing kept: b = +INF, nearest = 0xFFFFFFFF.
 *   a non-singleton: m = (a < b) ? b : a; s(i) = (b - a) / m, one subtraction and one division.  NaN falls out of the arithmetic
 *     and is not patched (a single cluster, a = b = 0, a NaN in the row); which NaN an operation makes (sign, payload) is the
 *     hardware's choice, not this contract's.
 *   clusters[c]: the distinct labels of the cut; nans[c]: the i with NaN s(i);
 *   score[c] = (((0.0f + s(i1)) + s(i2)) + ...) / (float)kept over the non-NaN s(i), i ascending; kept == 0: a quiet NaN (0x7FC00000).
 * For L != C(i) and ROWS, mean(i, L) is the bits of apd_cross_linkage's link_fs[i][L] with fs = the matrix.
 * A function of the matrix and the labels alone: no workgroup size, schedule, LDS limit, panel cut or number of cuts per call enters
 * it; a call with L cuts equals L calls with one cut.
 * score, clusters, nans: [n_cuts]; s, a, b, nearest: [n_cuts][n], each may be NULL.  distances and the outputs: host, or all device
 * pointers if on_device (the call waits once for the upload of the label tables -- once per 1024 cuts -- and the kernels are only
 * enqueued on the context's stream, as apd_cross_linkage does).  Otherwise the call blocks.
 * APD_ERR_INVALID_ARG, before anything is launched or written: another axis, n_cuts == 0, a NULL labels, score, clusters or nans.
 * n == 0: APD_OK with NaN scores and zero counts.  A workspace that does not fit: APD_ERR_OOM.  Workspace: 8 n bytes per cut and 16
 * bytes per (cut, cluster), n floats per cut more when s is NULL; the host form also holds the matrix and the results.
 * Rows of up to 32768 entries are staged in LDS once; longer ones are read from HBM.  COLUMNS gathers the columns into a [panel][n]
 * workspace of the context (256 MiB, shared with apd_neighbors) and walks its rows, in as many panels as it takes.
 * Environment (tests only; read at every call; results are bit-identical whatever they say): APD_SILHOUETTE_WORKGROUP=<64 .. 1024, a
 * multiple of 64> sets the work-items of a row's workgroup, APD_SILHOUETTE_LDS_COLUMNS=<entries> lowers the LDS residency limit,
 * APD_SILHOUETTE_WORKSPACE_BYTES=<bytes> sets the panel workspace (at least one column is taken). */
int apd_silhouette(apd_context *ctx, const float *distances, int on_device, uint32_t n, int axis,
                   const uint32_t *labels, uint32_t n_cuts, float *score, uint32_t *clusters, uint32_t *nans,
                   float *s, float *a, float *b, uint32_t *nearest);

/* ---- density clustering: which instances recur at least min_pts times within eps, and which are alone (DBSCAN) -----------------
 * distances: the [n][n] matrix of apd_align_all.  eps, min_pts: HOST arrays of n_settings (<= APD_DENSITY_MAX_SETTINGS) settings, all
 * answered from one pass over the matrix.  The matrix is directed and components need a symmetric relation, so for setting s:
 *   near(i, j) := d[i][j] <= eps[s] under IEEE comparison: a NaN entry or a NaN eps is never near, -0.0 and +0.0 are equal, eps = +INF
 *     makes every non-NaN entry near, +INF included.
 *   for i != j: adj(i, j) := near(i, j) || near(j, i) (APD_DENSITY_EITHER), near(i, j) && near(j, i) (APD_DENSITY_BOTH).  The value on
 *     the diagonal enters nothing.
 *   degree[i] = the number of j != i with adj(i, j).  i is a core point iff (uint64)degree[i] + 1 >= min_pts[s]: the point counts
 *     itself and the comparison is <=, scikit-learn's DBSCAN convention -- the k-th neighbour distance of i from apd_neighbors
 *     (skip_self) as eps with min_pts = k + 1 makes i core.
 *   labels: clusters are the connected components of adj restricted to core points; a core point's label is the smallest core point
 *     of its component.  A non-core point with at least one core neighbour is a border point, its label the smallest label among its
 *     core neighbours (a fixed rule where the textbook algorithm depends on the visiting order).  Every other point is noise with
 *     labels[i] = i, apd_cut_labels' idiom for an instance never merged; it cannot collide with a cluster, whose label is a core
 *     point's number.  So labels[s] is always a valid assignment for apd_silhouette, noise as singletons.
 *   kind[i]: APD_DENSITY_NOISE, _BORDER or _CORE.  counts[s] = {distinct cluster labels, core, border, noise points}; the last three
 *     sum to n.  nans: the NaN entries off the diagonal.
 * Every bit of the result is decided by one comparison per entry; everything behind it is integer (ballots, popcounts, minima of
 * numbers).  A function of the matrix and the settings alone: no workgroup size, schedule, round count, workspace size or number of
 * settings per call enters it; a call with S settings equals S calls with one.
 * labels, degree: [n_settings][n] uint32, kind: [n_settings][n] bytes, counts: [n_settings][4], nans: one value; kind, degree and nans
 * may be NULL.  distances and the outputs: host, or all device pointers if on_device.  BLOCKING IN BOTH FORMS, unlike apd_neighbors
 * (whose kernels are only enqueued): the component search converges on the device -- minimum-label propagation with hooking and
 * pointer jumping, with no bound on its rounds other than n -- and the host reads a "changed" word between batches of rounds.  With
 * apd_set_timing on, apd_last_kernel_ms covers the call's kernels and apd_density_last_profile splits them: phase_ms[4] = adjacency,
 * degree, propagation, border (summed over the groups below), rounds = propagation rounds enqueued.
 * APD_ERR_INVALID_ARG, before anything is launched or written: another link, n_settings == 0 or above the maximum, a min_pts[s] == 0,
 * a NULL eps, min_pts, labels or counts.  n == 0: APD_OK with zero counts.  A workspace that does not fit: APD_ERR_OOM.  More than
 * 2^21 instances: APD_ERR_UNSUPPORTED.
 * Workspace: a bit matrix of n * ceil(n / 64) * 8 bytes per setting (32 MiB at n = 16384), bounded by 256 MiB; when the planes of all
 * settings do not fit, the settings are processed in groups and every group reads the matrix again -- the only case in which it is
 * read more than once.  The host form also holds the matrix and the results.
 * Environment (tests only; read at every call; results are bit-identical whatever they say): APD_DENSITY_WORKSPACE_BYTES=<bytes> sets
 * the bound on the planes (at least one setting's plane is taken), APD_DENSITY_ROUNDS_PER_SYNC=<r> the rounds enqueued between two
 * reads of the changed words (default 4), APD_DENSITY_WORKGROUP=<64 .. 1024, a multiple of 64> the work-items of a workgroup of the
 * propagation and border kernels (default 256). */
#define APD_DENSITY_EITHER 0
#define APD_DENSITY_BOTH   1
#define APD_DENSITY_MAX_SETTINGS 8
#define APD_DENSITY_NOISE  0
#define APD_DENSITY_BORDER 1
#define APD_DENSITY_CORE   2
int apd_density_clusters(apd_context *ctx, const float *distances, int on_device, uint32_t n, int link,
                         const float *eps, const uint32_t *min_pts, uint32_t n_settings,
                         uint32_t *labels, uint8_t *kind, uint32_t *degree, uint32_t *counts, uint64_t *nans);
int apd_density_last_profile(apd_context *ctx, float *phase_ms, uint32_t *rounds);

/* ---- density hierarchy: every eps of apd_density_clusters at one min_pts, from one tree (HDBSCAN's hierarchy) ------------------
 * distances: the [n][n] matrix of apd_align_all.  A function of the matrix, link and min_pts alone, bit for bit.
 * Order.  Every value is compared through a key: NaN is MISSING and ranks behind everything, +INF included; -0.0 and +0.0 are equal;
 *   everything else follows IEEE order -- negative values and +-INF are ordinary values.  Values come back in canonical form: either
 *   zero as +0.0, missing as the quiet NaN 0x7FC00000, so nothing depends on which of two equal entries was "chosen".
 * Symmetrised distance, i != j (the diagonal enters nothing): sym(i, j) = the smaller of d[i][j] and d[j][i] under the order
 *   (APD_DENSITY_EITHER: a NaN loses to any number, two NaNs give missing), the larger (APD_DENSITY_BOTH: a NaN wins).  For every
 *   non-NaN eps, sym(i, j) <= eps is exactly apd_density_clusters' adj(i, j).
 * Core distance.  min_pts = 1: core[i] = -INF.  min_pts = m >= 2: the (m - 1)-th smallest sym(i, j) over j != i under the order;
 *   missing when m - 1 > n - 1 or when that entry is missing.  Only the one value is selected, so there is no cap on min_pts such as
 *   APD_NEIGHBORS_MAX_K.  core[i] <= eps holds exactly when i is a core point of apd_density_clusters(eps, m, link).
 * Mutual reachability: mr(i, j) = the largest of core[i], core[j] and sym(i, j) under the order.
 * Tree: the minimum spanning forest of the graph on n vertices whose edges are the pairs i < j with non-missing mr(i, j), the edges
 *   ordered by the strict total order (key(mr), i, j) -- under which the forest is unique.  *n_edges <= n - 1 edges come back with
 *   edge_i[t] < edge_j[t] and weight[t] = mr, t ascending in that order; the slots behind them hold 0xFFFFFFFF, 0xFFFFFFFF and the
 *   quiet NaN.  *nans: the NaN entries off the diagonal, as apd_density_clusters counts them.
 * core: [n] floats; edge_i, edge_j, weight: [n - 1] (none for n <= 1, and then they may be NULL); host, or all device pointers if
 * on_device.  n_edges and nans are HOST words in both forms.  BLOCKING IN BOTH FORMS, like apd_density_clusters: the forest is built in
 * Boruvka rounds on the device (every component takes its smallest edge that leaves it; a round is one pass over the matrix) and the
 * host reads the number of edges between rounds.  At most ceil(log2 n) + 1 rounds; more is an internal error (APD_ERR_HIP), not a
 * longer loop.  With apd_set_timing on, apd_last_kernel_ms covers the call's kernels and apd_density_tree_last_profile splits them:
 * phase_ms[3] = core distances, rounds, final ordering; rounds = the rounds run.
 * APD_ERR_INVALID_ARG, before anything is launched or written: another link, min_pts == 0, a NULL n_edges, nans, core (n >= 1) or
 * edge array (n >= 2).  n == 0: APD_OK with no edges; n == 1: core[0] and no edges.  More than 2^21 instances: APD_ERR_UNSUPPORTED.
 * A workspace that does not fit: APD_ERR_OOM.
 * Workspace: at most 56 bytes per instance, and for min_pts in 2 .. n the [panel][n] gather of mirror columns shared with apd_neighbors (256
 * MiB at most); no n^2 workspace -- every round reads the matrix.  The host form also holds the matrix and the results.
 * Environment (tests only; read at every call; results are bit-identical whatever they say): APD_DENSITY_TREE_WORKSPACE_BYTES=<bytes>
 * sets the bound on the panel (at least one column is taken), APD_DENSITY_TREE_WORKGROUP=<64 .. 1024, a multiple of 64> the work-items
 * of a workgroup of the core-distance select and of the per-instance kernels (default 256).
 *
 * apd_density_tree_cut: host only, no context.  For each of n_eps values of eps (any number of them): join the endpoints of every
 *   edge with weight <= eps; a vertex with core[i] <= eps is core (kind APD_DENSITY_CORE) and its label is the smallest vertex of its
 *   component -- such a component holds core points only, because mr >= core; every other vertex is noise (APD_DENSITY_NOISE) with
 *   labels[i] = i.  counts[s] = {clusters, core, 0, noise}.  This is DBSCAN* (no border points: assigning them needs the adjacency and
 *   stays with apd_density_clusters): the core mask equals kind == CORE of apd_density_clusters(eps, min_pts, link) and the labels
 *   agree on those points, for every non-NaN eps.  labels: [n_eps][n], kind: [n_eps][n] bytes or NULL, counts: [n_eps][4].
 *   APD_ERR_INVALID_ARG with nothing written: a NaN eps (the one setting where the two calls cannot agree: with min_pts = 1
 *   apd_density_clusters calls every point core under a NaN eps), a NULL core, eps, labels or counts, or an edge list that is not a
 *   forest over n (a vertex >= n, edge_i >= edge_j, or a cycle).
 * apd_density_tree_operations: host only.  The single-linkage merge list (min_pts = 1; for larger min_pts the same over mr) in
 *   apd_cluster_op format: edge t merges the current roots of its endpoints, merge_i the root on edge_i's side, merge_j the root on
 *   edge_j's side, into = n + t, distance = weight[t], operation by the rule of clustering.rs:193-201.  ops: [n_edges].
 *   apd_cut_labels, apd_cluster_sets and apd_dendrograms take the list as they take apd_clustering's.  The same refusals. */
int apd_density_tree(apd_context *ctx, const float *distances, int on_device, uint32_t n, int link, uint32_t min_pts,
                     float *core, uint32_t *edge_i, uint32_t *edge_j, float *weight, uint32_t *n_edges, uint64_t *nans);
int apd_density_tree_last_profile(apd_context *ctx, float *phase_ms, uint32_t *rounds);
int apd_density_tree_cut(uint32_t n, const float *core, const uint32_t *edge_i, const uint32_t *edge_j, const float *weight,
                         uint32_t n_edges, const float *eps, uint32_t n_eps, uint32_t *labels, uint8_t *kind, uint32_t *counts);
int apd_density_tree_operations(uint32_t n, const uint32_t *edge_i, const uint32_t *edge_j, const float *weight, uint32_t n_edges,
                                apd_cluster_op *ops);

/* ---- cluster prototypes: which member stands for a cluster, and the cluster's average shape ---------------------------------
 * The medoid of every set: the member closest to all the others, from the [n][n] matrix of apd_align_all.  For set k with its
 * members sorted ascending j1 < j2 < ..., whatever order `members` lists them in, the cost of member i is
 *   cost(i) = ((((0 + d[i][j1]) + d[j1][i]) + d[i][j2]) + d[j2][i]) + ...
 * f32, one rounded add per term; j = i is included (its diagonal entry is 0 in a matrix of apd_align_all).  medoid[k]: scan i
 * ascending and keep a member only if its cost is strictly below the best so far, starting from +INF -- the smallest sequence
 * number wins ties, a NaN cost is never kept; cost[k] that value (cost may be NULL).  Nothing kept (all +INF / NaN, or an empty set):
 * 0xFFFFFFFF and +INF.
 * members / set_off / n_sets: host arrays, as apd_cluster_sets returns them and apd_cross_linkage takes them; a member >= n or a
 * sequence listed twice in one set is APD_ERR_INVALID_ARG.  n_sets == 0: APD_OK, nothing written.
 * distances / medoid / cost: host, or all device pointers if on_device (the matrix and the results stay in HBM; the call waits once
 * for the upload of the member lists, the kernels are only enqueued on the context's stream, as apd_cross_linkage does). */
int apd_cluster_medoids(apd_context *ctx, const float *distances, int on_device, uint32_t n,
                        const uint32_t *members, const uint32_t *set_off, uint32_t n_sets,
                        uint32_t *medoid, float *cost);

/* DTW barycenter averaging (DBA, Petitjean et al. 2011) of every set: a sequence whose frames are the means of the member frames
 * that warp onto them.  batch: any resident batch, plain or joined; sequence numbers are the caller's.  members / set_off / n_sets:
 * as for apd_cluster_medoids.  init[k]: the sequence whose frames start set k's barycenter -- usually the medoid; it need not be a
 * member.  The barycenter of set k keeps the length of init[k]: T_k frames, 0 for an empty set.
 * One iteration for set k, current barycenter c (T frames), members s1 < s2 < ... ascending whatever order `members` lists them in:
 *   for every member s the warping path of the ordered pair (x = c, y = s) exactly as apd_align_paths defines it: band from
 *     max(T, len s) through cfg, the literal arithmetic whatever apd_set_distance_mode says, the walk from (n-1, m-1);
 *   a path CONTRIBUTES iff it is non-empty and its first step is START (it reached the origin).  The test is structural: a complete
 *     path with NaN costs contributes; a member of one frame gives an empty path and is skipped unless T = 1 as well;
 *   for table rows t = 1 .. T: sum[t][.] = 0, cnt[t] = 0; then over the contributing members ascending, and over each path's steps
 *     in path order with i == t and op != START: sum[t][d] = sum[t][d] + y_s[j-1][d] (one rounded f32 add per dimension), cnt[t] += 1;
 *   new c[t-1][d] = sum[t][d] / (float)cnt[t] (one f32 division) where cnt[t] > 0, otherwise c[t-1] keeps its value.
 * The paths end at the reference's score cell (n-1, m-1) (alignments.rs:120), so row T is never on a path: THE LAST FRAME OF A
 * BARYCENTER KEEPS THE LAST FRAME OF init[k].  That is the project's alignment, not an accident.  Rows 1 .. T-1 are all visited by a
 * complete path, so they average at least one frame per contributing member.
 *   used[it][k] = contributing members; inertia[it][k] = ((0 + score_s1) + score_s2 + ...) / (float)used over the contributing
 *   members ascending, scores (apd_align_paths' score) measured against the barycenter BEFORE this iteration's update; +INF if
 *   used == 0.  No monotonicity is promised: the reference's tie rule (alignments.rs:153-159) does not take a minimum.
 * iterations == 0 returns the init frames unchanged, bit for bit.
 * frame_off (n_sets + 1 entries, always written, no GPU work needed for it): set k owns frames[frame_off[k] .. frame_off[k+1]), each
 *   entry one frame of the caller's dim floats.  frames == NULL: sizes only.  capacity (in frames) < frame_off[n_sets]:
 *   APD_ERR_INVALID_ARG.  frames_on_device: frames is a device pointer and the result stays in HBM, packed exactly as
 *   apd_batch_create(..., frames_on_device = 1) takes it with frame_off as offsets.  inertia / used: [iterations][n_sets], host,
 *   either may be NULL.
 * An index (member or init) >= apd_batch_len or a sequence listed twice in one set is APD_ERR_INVALID_ARG, an empty sequence in the
 * batch APD_ERR_EMPTY_SEQUENCE, any (T_k, len s) whose band needs 2w+1 > 20 480 offsets APD_ERR_BAND_TOO_WIDE, each before anything is
 * launched.  Follows apd_batch_refill.  Blocking.  With apd_set_timing on, apd_last_kernel_ms covers all kernels of the call.
 * The barycenters never visit the host between iterations and no step is downloaded; the pairs run in chunks under
 * apd_align_paths' workspace cap (APD_PATH_WORKSPACE_BYTES), a set may straddle chunks, results identical whatever the cap. */
int apd_barycenters(apd_context *ctx, const apd_batch *batch, const apd_align_config *cfg,
                    const uint32_t *members, const uint32_t *set_off, uint32_t n_sets,
                    const uint32_t *init, uint32_t iterations,
                    float *frames, int frames_on_device, uint64_t capacity, uint64_t *frame_off,
                    float *inertia, uint32_t *used);

/* ---- companions ---------------------------------------------------------------------- */
/* AutoEncoder::predict over every frame = NDSequence::encoded (src/neural.rs:55-71,
 * src/spectrogram.rs:103-121).  x: [t][d_in]; w_encode: [d_in][latent] (Mat{flat, cols=latent},
 * numerics.rs:171-174); b_encode: [latent]; out: [t][latent].  *_on_device selects HBM pointers
 * for x and out. */
int apd_encode(apd_context *ctx, const float *x, uint64_t t, uint32_t d_in, const float *w_encode,
               const float *b_encode, uint32_t latent, int on_device, float *out);
/* Cepstrum frames of NDSequence::new (src/spectrogram.rs:31-80).  Returns the frame count in
 * *n_frames and bins per frame in *n_bins; out may be NULL to query sizes.
 * Limits, the same for every cepstrum call (size queries and plans included): K = *n_bins + 4, the filterbank outputs, must be at
 * least 5 (else APD_ERR_INVALID_ARG, as the reference's cepstrum[4..] would be empty); fft_size <= 4096 and K <= 512 run (any
 * window length: powers of two by FFT, the others by the defining sum); fft_size > 4096 or K > 512 is APD_ERR_UNSUPPORTED. */
int apd_cepstrum(apd_context *ctx, const int16_t *samples, uint64_t n_samples, uint32_t fft_size,
                 uint32_t fft_step, uint32_t filter_size, int on_device, float *out, uint64_t *n_frames,
                 uint32_t *n_bins);

/* apd_cepstrum for n_seq recordings stored back to back (sample_offsets: n_seq+1): one launch for the whole corpus.
 * frame_offsets (n_seq+1, host, always written) and out ([frame_offsets[n_seq]][*n_bins], packed) are exactly the
 * `offsets` / `frames` arguments of apd_batch_create, so with on_device != 0 features go from audio to the
 * alignment without leaving HBM.  out may be NULL to query sizes. */
int apd_cepstrum_batch(apd_context *ctx, const int16_t *samples, const uint64_t *sample_offsets, uint32_t n_seq,
                       uint32_t fft_size, uint32_t fft_step, uint32_t filter_size, int on_device, float *out,
                       uint64_t *frame_offsets, uint32_t *n_bins);

/* The same two as RESIDENT objects + enqueue-only calls, for hosts that build features repeatedly or on several GPUs (the
 * reference does it per recording with par_iter, src/main.rs:150-161).  apd_encoder_create / apd_cepstrum_plan_create upload the
 * weights / build and upload the tables and the corpus' offsets ONCE (blocking; the host arrays are free on return; frame_offsets
 * and *n_bins are written as apd_cepstrum_batch writes them); apd_encode_async / apd_cepstrum_batch_async then only ENQUEUE the
 * kernel on the context's stream: device pointers only, no allocation, no table building, no synchronisation
 * (tests/test_gpu_companions.py::test_async_feature_stage_only_enqueues).  A plan serves every corpus with the same sample offsets.
 * Objects die with apd_*_destroy, or device-side with their context (apd_destroy), after which only the destroy call is legal.
 * With several GPUs each context runs the whole corpus' kernel concurrently -- replicated on purpose: the kernels (0.15 ms for cfg 4,
 * 19 ms for cfg 5, whole corpus) cost less than an all-gather of their output would. */
int apd_encoder_create(apd_context *ctx, const float *w_encode, const float *b_encode, uint32_t d_in, uint32_t latent,
                       apd_encoder **encoder);
int apd_encoder_destroy(apd_encoder *encoder);
int apd_encode_async(apd_context *ctx, const apd_encoder *encoder, const float *d_x, uint64_t t, float *d_out);
int apd_cepstrum_plan_create(apd_context *ctx, const uint64_t *sample_offsets, uint32_t n_seq, uint32_t fft_size, uint32_t fft_step,
                             uint32_t filter_size, uint64_t *frame_offsets, uint32_t *n_bins, apd_cepstrum_plan **plan);
int apd_cepstrum_plan_destroy(apd_cepstrum_plan *plan);
int apd_cepstrum_batch_async(apd_context *ctx, const apd_cepstrum_plan *plan, const int16_t *d_samples, float *d_out);

/* ---- raw audio in chunks: a resident front end for a live feed -------------------------- */
/* The frames NDSequence::new yields for a recording of n_samples: n > fft ? ceil((n - fft) / step) : 0.  The loop is
 * `for i in (fft_size..n).step_by(fft_step)` (spectrogram.rs:51): the window that ends exactly at sample n is not produced, a frame
 * appears one sample after its window is complete.  Host only; 0 for fft_step == 0. */
uint64_t apd_cepstrum_frames(uint64_t n_samples, uint32_t fft_size, uint32_t fft_step);

/* An apd_feed turns the int16 samples of n_channels live recordings, delivered in chunks of any length, into the rows a streaming
 * session takes: cepstrum frames, or with an encoder (NULL: cepstra as they are) their encodings.  THE FRAMES OF THE PUSHES, ONE
 * AFTER THE OTHER, ARE THE BITS OF apd_cepstrum (+ apd_encode) ON THE WHOLE RECORDING, WHATEVER THE CHUNKING: a frame depends on its
 * own fft_size samples and nothing else, and the encoder is per frame.  The feed carries what a push leaves for the next: per
 * channel the samples from the start of the next window on (at most fft_size, in HBM), or how many samples are still to be skipped
 * when fft_step > fft_size.  A push is one kernel launch; buffers grow to the largest push seen and are then reused.
 *   create: limits and error codes are apd_cepstrum's; *dim is the row width -- the cepstrum's n_bins, or the encoder's latent.
 *     n_channels == 0, an encoder of another context or one whose d_in is not n_bins: APD_ERR_INVALID_ARG; a plan with the encoder's
 *     weights that does not fit the 160 KiB of LDS: APD_ERR_UNSUPPORTED.  The encoder's weights are copied: it may be destroyed.
 *     The feed is a child of its context, like plans and sessions.
 *   reset: the channel (0xFFFFFFFF: all) starts a new recording; totals: samples received and frames emitted since (host only).
 *   push: channel k's chunk is samples[sample_off[k] .. sample_off[k+1]) (0, 1 or any number of samples).  A push that takes a channel
 *     from N0 to N1 samples emits frames apd_cepstrum_frames(N0) .. apd_cepstrum_frames(N1) - 1 of its recording; the output is packed
 *     [frame_off[n_channels]][dim] -- the `frames` / `chunk_off` pair of apd_spot_stream_push.  frame_off (n_channels + 1, host) is
 *     always written.  frames == NULL: sizes only, the state does not move.  Descending sample_off or capacity (in frames) below
 *     frame_off[n_channels]: APD_ERR_INVALID_ARG, the state untouched; every error is raised before anything is launched.  Blocking. */
typedef struct apd_feed apd_feed;
int apd_feed_create(apd_context *ctx, uint32_t n_channels, uint32_t fft_size, uint32_t fft_step, uint32_t filter_size,
                    const apd_encoder *encoder, uint32_t *dim, apd_feed **feed);
int apd_feed_destroy(apd_feed *feed);
int apd_feed_reset(apd_context *ctx, apd_feed *feed, uint32_t channel);
int apd_feed_totals(const apd_feed *feed, uint32_t channel, uint64_t *samples, uint64_t *frames);
int apd_feed_push(apd_context *ctx, apd_feed *feed, const int16_t *samples, const uint64_t *sample_off, int samples_on_device,
                  float *frames, int frames_on_device, uint64_t capacity, uint64_t *frame_off);
/* apd_feed_push into a device buffer the feed owns, then apd_spot_stream_push on those rows: raw audio in, curves, bests, queued hits
 * and kept history out, exactly what apd_spot_stream_push produces for the same frames (it is that code).  The feed's dim must be
 * the templates' dimension and its channel count the session's (else APD_ERR_INVALID_ARG before anything runs); the remaining
 * arguments and the sizes-only form (cost, start and best all NULL: neither state moves) are apd_spot_stream_push's.  The session
 * and the feed are reset separately. */
int apd_spot_stream_push_audio(apd_context *ctx, apd_spot_stream *stream, apd_feed *feed, const int16_t *samples,
                               const uint64_t *sample_off, int samples_on_device, float *cost, uint32_t *start,
                               uint64_t capacity, uint64_t *curve_off, apd_spot_best *best);

/* NDSequence::interesting_ranges (src/spectrogram.rs:174-216), the "VAT" pre-segmentation that precedes the path:
 * per-frame std, mean of the `moving_average` previous values, percentile threshold, runs longer than min_len.
 * frames: [t][n_bins] (device if on_device).  ranges: (start, stop) frame pairs, host; *n_ranges may exceed capacity; ranges == NULL
 * with capacity == 0 only counts, with capacity > 0 it is APD_ERR_INVALID_ARG.
 * This is apd_interesting_ranges_batch (below) for a batch of one: frame_offsets = {0, t}, no status array, *n_ranges = range_off[1].
 * So where the reference panics (t == 0, moving_average == 0, a percentile index at or beyond the non-NaN variances) the call returns
 * APD_ERR_INDEX with *n_ranges == 0, and apd_last_error carries the batch's text under this call's name; t >= 2^32 is
 * APD_ERR_UNSUPPORTED before anything is launched (*n_ranges == 0, nothing read or written); the host form's input and the variances
 * live in the context's grow-only workspace, nothing is allocated per call once it has grown.  Kernels: csrc/vat.hip. */
int apd_interesting_ranges(apd_context *ctx, const float *frames, uint64_t t, uint32_t n_bins, uint32_t moving_average,
                           float perc, uint64_t min_len, int on_device, uint64_t *ranges, uint64_t capacity,
                           uint64_t *n_ranges);

/* ---- stage 1 for a whole corpus: batched VAT ranges and the slices they name (src/main.rs:58-92) ------------------------------
 * NDSequence::interesting_ranges (src/spectrogram.rs:174-216) for n_seq recordings in a number of launches and synchronisations that
 * depends on neither n_seq nor any length: frames / frame_offsets are what apd_cepstrum_batch writes and apd_batch_create takes (packed [frame_offsets[n_seq]][n_bins],
 * the offsets a HOST array; frames in HBM with on_device).  RECORDING s GETS, IN ORDER, EXACTLY THE RANGES spectrogram.rs:174-216
 * GIVES FOR ITS FRAMES, whatever its neighbours are: ranges[range_off[s] .. range_off[s + 1]) as (start, stop) frame pairs counted
 * within the recording.  range_off (n_seq + 1, host) is always written and exact whatever the capacity (in ranges); ranges past the
 * capacity are not written; ranges == NULL with capacity == 0 only counts, with capacity > 0 it is APD_ERR_INVALID_ARG.
 * Where the reference panics for one recording (no frames, moving_average == 0, a percentile index at or beyond its non-NaN
 * variances): with status (n_seq, host) that recording gets APD_ERR_INDEX there and no ranges, the others APD_OK, and the call returns
 * APD_OK; with status == NULL the call returns APD_ERR_INDEX, apd_last_error names the first such recording and range_off is all zero.
 * n_seq == 0: APD_OK, range_off[0] = 0.  Descending offsets: APD_ERR_INVALID_ARG; a recording of 2^32 frames or more:
 * APD_ERR_UNSUPPORTED; both before anything is launched.  Blocking: one read-back of verdicts and counts, one of the ranges; no
 * variance leaves the device.  Kernels: csrc/vat.hip, DESIGN.md section 4.19. */
int apd_interesting_ranges_batch(apd_context *ctx, const float *frames, const uint64_t *frame_offsets, uint32_t n_seq,
                                 uint32_t n_bins, uint32_t moving_average, float perc, uint64_t min_len, int on_device,
                                 uint64_t *range_off, uint64_t *ranges, uint64_t capacity, int32_t *status);
/* The slices of the raw audio (main.rs:76-89, audio.rs:54-60) as a new packed corpus: slice r of recording s is
 * samples[sample_offsets[s] + start * fft_step .. sample_offsets[s] + stop * fft_step), the slices back to back in range order.
 * apd_slice_offsets (host only): slice_offsets (range_off[n_seq] + 1) is the sample_offsets argument of apd_cepstrum_batch /
 * apd_cepstrum_plan_create for the sliced corpus; slice_seq[r] (or NULL) is the recording slice r came from, the reference's
 * audio_id.  apd_slice_samples: the gather, one launch; on_device covers both samples and out; capacity (in samples) below
 * slice_offsets[range_off[n_seq]] is APD_ERR_INVALID_ARG.  From both calls APD_ERR_INVALID_ARG for descending offsets, a range with
 * stop < start, ranges of a recording that are not ascending (a start before the previous stop), and a range whose stop * fft_step
 * runs past its recording (ranges of a cepstrum with the same fft_step never do); range_off must start at 0, and both offset arrays
 * are checked as a whole before anything is sized from them or written.  No ranges: APD_OK, nothing written. */
int apd_slice_offsets(const uint64_t *sample_offsets, const uint64_t *range_off, const uint64_t *ranges, uint32_t n_seq,
                      uint32_t fft_step, uint64_t *slice_offsets, uint32_t *slice_seq);
int apd_slice_samples(apd_context *ctx, const int16_t *samples, const uint64_t *sample_offsets, uint32_t n_seq,
                      const uint64_t *range_off, const uint64_t *ranges, uint32_t fft_step, int on_device, int16_t *out,
                      uint64_t capacity);

/* ---- formats either side of the path (host only, no context needed) ------------------------------------------------ */
/* AutoEncoder::from_file / save_file (src/neural.rs:30-44): the bincode 1.x image of
 *   struct AutoEncoder { w_encode, w_decode, b_encode, b_decode: Mat }  (neural.rs:13-19)
 *   struct Mat { flat: Vec<f32>, cols: usize }                             (numerics.rs:171-174)
 * i.e. four times { u64 length, length x f32, u64 cols }, little-endian.  apd_autoencoder_parse checks the image (sizes,
 * shapes D x L / L x D / 1 x L / 1 x D, no trailing bytes) and says where each matrix lies; apd_autoencoder_copy reads one
 * out (byte order handled); w_encode and b_encode are what apd_encode takes. */
typedef struct apd_mat_view { uint64_t offset /* byte offset of flat[0] */, len /* values */, cols; } apd_mat_view;
typedef struct apd_autoencoder_view { apd_mat_view w_encode, w_decode, b_encode, b_decode; } apd_autoencoder_view;
int apd_autoencoder_parse(const void *bytes, uint64_t n_bytes, apd_autoencoder_view *view);
int apd_autoencoder_copy(const void *bytes, const apd_mat_view *mat, float *out /* mat->len floats */);
/* out == NULL: *n_bytes = size of the image.  w_encode: [d_in][latent], w_decode: [latent][d_in], b_*: [latent], [d_in]. */
int apd_autoencoder_serialize(const float *w_encode, const float *w_decode, const float *b_encode, const float *b_decode,
                              uint32_t d_in, uint32_t latent, void *out, uint64_t capacity, uint64_t *n_bytes);

/* Discovery (src/discovery.rs:7-26) and Discovery::from_toml (:28-36) on the text of project/config/Discovery.toml: flat
 * `key = value  # comment` lines; every field exactly once, integers for the usize fields; keys the struct does not have
 * (and anything under a [table] header) are ignored, as serde does without deny_unknown_fields. */
typedef struct apd_discovery {
    uint64_t dft_win, dft_step, ceps_filter, vat_moving;
    float vat_percentile;
    uint64_t vat_min_len, alignment_workers;
    float clustering_percentile, warping_band_percentage, insertion_penalty, deletion_penalty, match_penalty;
    uint64_t auto_encoder;
    float learning_rate;
    uint64_t epochs;
    float epoch_drop, drop;
} apd_discovery;
int apd_discovery_parse_toml(const char *text, apd_discovery *out);

/* Templates::dendrograms (src/reporting.rs:135-169), the strings only: for every root that some op made, the TikZ-qtree
 * bracket string "[.k [<left> <right> ] ]" with leaves rendered as labels[leaf] (the reference puts its image_ref there,
 * reporting.rs:211-221) -- NUL-terminated, concatenated in the order of `roots`; which_root[i] = index into roots of
 * string i (roots never merged have none, reporting.rs:200).  out == NULL: sizes only.  The LaTeX / file output of :171-203
 * is presentation and stays with the caller.  Replay semantics are the reference's HashMap's for ANY ids (a repeated `into`
 * overwrites, an op may name its own `into` as an operand: the string built earlier is embedded); a string beyond 1 GiB or an
 * allocation failure is APD_ERR_OOM, never an abort. */
int apd_dendrograms(const apd_cluster_op *ops, uint32_t n_ops, const uint32_t *roots, uint32_t n_roots,
                    const char *const *labels, uint32_t n_labels, char *out, uint64_t capacity, uint64_t *n_bytes,
                    uint32_t *which_root, uint32_t *n_strings);

/* ---- autoencoder training (src/neural.rs:74-94, src/main.rs:115-135) ----------------------------------------------------------
 * The reference's SGD: batch size 1, one AutoEncoder::take_step per frame, in the order given.  A trainer holds n_models
 * independent models of one shape on the context's GPU; apd_trainer_run advances every one of them by n_steps steps in ONE launch,
 * one wavefront per model, the model on chip throughout.  A step is neural.rs:74-94 operation for operation in f32 (Mat::norm's
 * inverted condition, the decoder fed the pre-activation latent, Mat::mul from 0.0 with k ascending and no fused multiply-add),
 * with ONE stated deviation: the sigmoid's exponential is the defined sequence of f32 operations of DESIGN.md section 4.18 instead
 * of the platform's expf (at most 2 ulp from it).  WHAT A RUN LEAVES IS THEREFORE DEFINED BIT FOR BIT, whatever n_models and however
 * an order is split into runs; tests/_train_reference.py is the literal restatement.
 *   apd_trainer_create: host arrays [n_models][...] in the reference's Mat layouts: w_encode [d_in][latent], w_decode
 *     [latent][d_in], b_encode [latent], b_decode [d_in].  d_in or latent above 64: APD_ERR_UNSUPPORTED; 0, n_models == 0 or a NULL:
 *     APD_ERR_INVALID_ARG.
 *   apd_trainer_run: frames [n_frames][d_in] (host, or device with frames_on_device); order: HOST array of frame numbers, [n_steps]
 *     shared by all models or [n_models][n_steps] with order_per_model; alpha [n_models] (host).  Continues from the state the
 *     previous run left.  An index >= n_frames: APD_ERR_INVALID_ARG before anything is enqueued, the state untouched.  n_steps == 0
 *     changes nothing.  Blocking.  With apd_set_timing on, apd_last_kernel_ms covers the training kernel.
 *   apd_trainer_totals: per model, the running total_err (main.rs:130: one f32 add of 0.5 * euclidean per step), the steps since the
 *     last reset, and the step -- counted from the trainer's creation, resets notwithstanding -- at which a weight first became
 *     non-finite (UINT64_MAX while the model is finite; non-finite weights never recover).  Any of the three may be NULL.  reset:
 *     total_err and steps go back to 0 afterwards (an epoch boundary); the weights and first_nonfinite stay.
 *   apd_trainer_weights: one model's four matrices, downloaded.
 *   apd_trainer_encoder: an apd_encoder made from the model's CURRENT w_encode / b_encode, device to device: what apd_encode_async
 *     and apd_feed_create take.  It owns a copy: later runs do not change it, and the trainer may be destroyed before it.
 * A trainer or context of another context, a NULL where data is due, model >= n_models: APD_ERR_INVALID_ARG.  After APD_ERR_HIP the
 * trainer's state is undefined. */
typedef struct apd_trainer apd_trainer;
int apd_trainer_create(apd_context *ctx, uint32_t d_in, uint32_t latent, uint32_t n_models, const float *w_encode,
                       const float *w_decode, const float *b_encode, const float *b_decode, apd_trainer **trainer);
int apd_trainer_destroy(apd_trainer *trainer);
int apd_trainer_run(apd_context *ctx, apd_trainer *trainer, const float *frames, uint64_t n_frames, int frames_on_device,
                    const uint32_t *order, uint64_t n_steps, int order_per_model, const float *alpha);
int apd_trainer_totals(apd_trainer *trainer, float *total_err, uint64_t *steps, uint64_t *first_nonfinite, int reset);
int apd_trainer_weights(apd_trainer *trainer, uint32_t model, float *w_encode, float *w_decode, float *b_encode, float *b_decode);
int apd_trainer_encoder(apd_context *ctx, apd_trainer *trainer, uint32_t model, apd_encoder **encoder);
/* Evaluation: the error of every model's CURRENT weights on chosen frames, and no update -- what picks one of many trained models
 * on held-out frames.  For model m and position e < n_eval, with x = frames[order[e]] (order [n_eval] shared by the models, or
 * [n_models][n_eval] with order_per_model; HOST array), error[m][e] is what AutoEncoder::take_step (neural.rs:74-94) would return for
 * x: the arithmetic of apd_trainer_run operation for operation (x.norm() with its inverted condition, Mat::mul from 0.0 with k
 * ascending and no fused multiply-add, the decoder fed the pre-activation latent, the defined sigmoid, 0.5 * sqrt of the squares
 * added in ascending i).  Every (model, position) is independent: DEFINED BIT FOR BIT whatever n_models, the grid or the chunking.
 *   errors: [n_models][n_eval] f32, host, or device with errors_on_device; may be NULL.
 *   total_err [n_models] (host, may be NULL): main.rs:130 with the weights frozen -- from +0.0, one f32 add per position in position
 *     order (no tree, no f64): the bits of apd_trainer_run with alpha = 0 wherever that route is defined.
 *   first_nonfinite [n_models] (host, may be NULL): the first position whose error is not finite, UINT64_MAX if there is none.
 * The trainer is not changed: weights, total_err, steps, the lifetime count and its own first_nonfinite keep their bits, also after
 * APD_ERR_HIP.  A constant, NaN or infinite frame gives a NaN or inf error at its own position (and from there on in the sequential
 * total) and touches nothing else -- apd_trainer_run with alpha = 0 turns every weight NaN on the first constant frame.
 * order == NULL: positions 0 .. n_frames - 1; n_eval must equal n_frames and order_per_model be 0.  An index >= n_frames, n_frames
 * >= 2^32, all three outputs NULL, a trainer of another context, a NULL where data is due: APD_ERR_INVALID_ARG before anything is
 * enqueued, apd_last_error naming the call.  n_eval == 0 launches nothing: totals +0.0, first_nonfinite UINT64_MAX.  Blocking.  A call
 * whose n_models * n_eval * 4 bytes exceed 1 GiB (APD_EVAL_WORKSPACE_BYTES overrides, for tests) is cut into chunks of positions, the
 * results identical whatever the cut.  With apd_set_timing on, apd_last_kernel_ms covers the evaluation's kernels. */
int apd_trainer_evaluate(apd_context *ctx, apd_trainer *trainer, const float *frames, uint64_t n_frames, int frames_on_device,
                         const uint32_t *order, uint64_t n_eval, int order_per_model, float *errors, int errors_on_device,
                         float *total_err, uint64_t *first_nonfinite);
/* AutoEncoder::step_decay (neural.rs:26-28): learning_rate * drop ^ floor((1 + epoch) / epoch_drop) in f32.  Host only. */
float apd_step_decay(float learning_rate, float drop, float epoch_drop, float epoch);
/* The order of one epoch (main.rs:120-124): the signals in order (signal s owns frames offsets[s] .. offsets[s + 1]), each signal's
 * frames in a fresh Fisher-Yates shuffle.  order: offsets[n_seq] - offsets[0] frame numbers.  The reference draws from thread_rng;
 * here the draws come from a counter-based generator (SplitMix64's finaliser over a key of (seed, epoch, signal) and the position:
 * csrc/train_math.h), so (seed, epoch) fixes the order on every machine.  Descending offsets or 2^32 frames or more:
 * APD_ERR_INVALID_ARG.  n_seq == 0: nothing written.  Host only. */
int apd_train_order(uint64_t seed, uint64_t epoch, const uint64_t *offsets, uint32_t n_seq, uint32_t *order);

#ifdef __cplusplus
}
#endif
#endif
