// The VAT pre-segmentation, NDSequence::interesting_ranges (spectrogram.rs:174-216), and stage 1 of the reference (main.rs:58-92,
// dump_interesting) built on it: the ranges of every recording of a corpus in a number of launches that does not depend on the
// corpus, and the gather of the raw audio the ranges name (main.rs:76-89, audio.rs:54-60) into a new packed corpus.  DESIGN.md
// section 4.19.
//
//   vat_variance_kernel   per-frame std + moving mean, a tile of one recording per workgroup, the halo's stds in LDS
//   vat_select_kernel     numerics.rs:125-133 per recording: four 8-bit digit passes, histogram, prefix and rank on chip
//   vat_scan_kernel       the run scan, 64 columns per wavefront step through ballots; counts, then the ranges in order
//   slice_gather_kernel   one work-item per 16 bytes of output
//
// This is the library's one implementation: apd_interesting_ranges is apd_interesting_ranges_batch for a batch of one.
#include <algorithm>
#include <cstring>
#include <exception>
#include <string>
#include <vector>

#include "apd_internal.h"

using namespace apd;

namespace {

constexpr uint32_t kVatTile = 256;        // frames per workgroup of the variance kernel, and its work-items
constexpr uint32_t kVatHaloMax = kVatTile; // windows up to this keep the halo's stds in LDS (at most twice the stds per output)
// Steps of the select whose loads are issued together.  A step is short (a ballot, a shuffle, LDS atomics) and a workgroup owns a
// whole recording, so one load per step leaves it waiting on HBM: 16 recordings of 2^20 frames select in 2.01 ms with one load in
// flight per work-item and in 1.05 ms with eight (kernel trace, MI355X).  The scan's steps hold a barrier and gain nothing from it.
constexpr uint32_t kSelectAhead = 8;
constexpr uint32_t kVatStageBins = 48;    // frames up to this width are staged through LDS (4 wavefronts x 64 rows x 49 floats)

struct VatSeq {
    uint64_t off;       // first frame of the recording, counted from the batch's first frame
    uint32_t t;         // its frames
    uint32_t kidx;      // (t as f32 * perc) as usize, saturated: the percentile's index into the NaN-filtered variances
};
struct VatResult {
    float th;           // the selected variance
    int32_t status;     // APD_OK, or APD_ERR_INDEX where the reference panics
    uint32_t nan;       // NaN variances
    uint32_t count;     // ranges longer than min_len (vat_scan_kernel<false>)
};

struct VatParams {
    const float *frames;           // the batch's first frame
    const VatSeq *seq;
    const uint32_t *tile_first;    // [n_seq + 1] first tile (= workgroup) of every recording
    uint32_t n_seq, n_bins, k;
    float *stds;                   // [T] modes 1 and 2
    float *var;                    // [T]
};

// NDSequence::variance (spectrogram.rs:174-187): per-frame population std (numerics.rs:12-29), then the mean of the k PREVIOUS
// values, summed in order.
__device__ __forceinline__ float frame_std(const float *v, uint32_t n_bins)
{
    float mean = 0.0f;
    for (uint32_t b = 0; b < n_bins; ++b) mean = mean + v[b];
    mean = mean / (float)n_bins;
    float sd = 0.0f;
    for (uint32_t b = 0; b < n_bins; ++b) { const float d = v[b] - mean; sd = sd + d * d; }
    return sqrtf(sd / (float)n_bins);
}
__device__ __forceinline__ float moving_mean(const float *prev /* the k stds in front of the frame */, uint32_t k)
{
    float acc = 0.0f;
    for (uint32_t q = 0; q < k; ++q) acc = acc + prev[q];
    return acc / (float)k;
}

#define VAT_WAVE_LDS_FENCE() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")

// MODE 0: stds of the tile and of the k frames in front of it into LDS, then the tile's moving means (k <= kVatHaloMax).
// MODE 1: the tile's stds to P.stds.  MODE 2: the tile's moving means from P.stds (any k).
// A workgroup's frames all belong to one recording; a wavefront reads 64 rows as one contiguous stretch of floats.
template <int MODE>
__global__ __launch_bounds__(kVatTile) void vat_variance_kernel(const VatParams P)
{
    extern __shared__ float lds[];
    uint32_t s = 0;
    for (uint32_t hi = P.n_seq; hi - s > 1;) { const uint32_t mid = (s + hi) >> 1; if (P.tile_first[mid] <= blockIdx.x) s = mid; else hi = mid; }
    const VatSeq q = P.seq[s];
    const uint32_t k = P.k, a = (blockIdx.x - P.tile_first[s]) * kVatTile, b = min(q.t - a, kVatTile) + a;   // the tile: frames [a, b)
    const uint32_t i = a + threadIdx.x;
    if (MODE == 2) {
        if (i < b) P.var[q.off + i] = i >= k ? moving_mean(P.stds + q.off + (i - k), k) : 0.0f;
        return;
    }
    if (MODE == 0 && b <= k) {                                      // the first k outputs of a recording are the literal 0.0
        if (i < b) P.var[q.off + i] = 0.0f;
        return;
    }
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t row_lo = MODE == 0 && a > k ? a - k : (MODE == 0 ? 0u : a), n_rows = b - row_lo;   // <= kVatTile + kVatHaloMax
    float *sstd = lds;                                              // MODE 0: stds of rows row_lo ..
    const bool staged = P.n_bins <= kVatStageBins;
    const uint32_t stride = P.n_bins | 1;                           // odd: lanes reading a column of 64 rows hit 64 banks
    float *stage = lds + (MODE == 0 ? kVatTile + kVatHaloMax : 0) + (size_t)wave * 64 * stride;
    const uint32_t dq = 64 / P.n_bins, dr = 64 % P.n_bins;
    for (uint32_t c = wave * 64; c < n_rows; c += kVatTile) {
        const uint32_t r0 = row_lo + c, nr = min(64u, b - r0);
        float sd = 0.0f;
        if (staged) {
            const float *src = P.frames + (q.off + r0) * P.n_bins;
            const uint32_t count = nr * P.n_bins;
            uint32_t row = lane / P.n_bins, col = lane % P.n_bins;
            for (uint32_t e = lane; e < count; e += 64) {
                stage[row * stride + col] = src[e];
                row += dq; col += dr;
                if (col >= P.n_bins) { col -= P.n_bins; ++row; }
            }
            VAT_WAVE_LDS_FENCE();
            if (lane < nr) sd = frame_std(stage + lane * stride, P.n_bins);
            VAT_WAVE_LDS_FENCE();
        } else if (lane < nr) {
            sd = frame_std(P.frames + (q.off + r0 + lane) * P.n_bins, P.n_bins);
        }
        if (lane < nr) {
            if (MODE == 1) P.stds[q.off + r0 + lane] = sd; else sstd[c + lane] = sd;
        }
    }
    if (MODE == 1) return;
    __syncthreads();
    if (i < b) P.var[q.off + i] = i >= k ? moving_mean(sstd + (i - k - row_lo), k) : 0.0f;
}

// One workgroup per recording: the k-th smallest non-NaN variance, by four passes over the digits of order_key.  The histogram
// lives in LDS, the prefix found so far and the remaining rank in registers: nothing visits the host between passes.  The answer
// is an element of the input, so it does not depend on the workgroup's size.
__global__ __launch_bounds__(1024) void vat_select_kernel(const float *__restrict__ var, const VatSeq *__restrict__ seq, VatResult *__restrict__ res)
{
    __shared__ uint32_t hist[257];
    __shared__ uint32_t s_next[4];                                  // the digit in place, the rank left, the verdict, the NaN count
    const VatSeq q = seq[blockIdx.x];
    const float *x = var + q.off;
    const uint32_t lane = threadIdx.x & 63;
    uint32_t prefix = 0, mask = 0, rank = q.kidx, nan = 0;
    bool bad = false;
    for (int pass = 0; pass < 4 && !bad; ++pass) {
        const int shift = 24 - 8 * pass;
        for (uint32_t h = threadIdx.x; h < 257; h += blockDim.x) hist[h] = 0;
        __syncthreads();
        for (uint64_t g0 = 0; g0 < q.t; g0 += (uint64_t)kSelectAhead * blockDim.x) {
            float ahead[kSelectAhead];                               // the loads of kSelectAhead steps are in flight together
            for (uint32_t u = 0; u < kSelectAhead; ++u) { const uint64_t e = g0 + u * blockDim.x + threadIdx.x; ahead[u] = e < q.t ? x[e] : 0.0f; }
            for (uint32_t u = 0; u < kSelectAhead; ++u) {
                const uint64_t e0 = g0 + u * blockDim.x, e = e0 + threadIdx.x;
                if (e0 >= q.t) break;                                // uniform: the ballots below see whole wavefronts
                const float v = ahead[u];
                const bool live = e < q.t, is_nan = v != v;
                const uint32_t key = order_key(v);
                const bool want = live && (is_nan ? pass == 0 : (key & mask) == prefix);
                const uint32_t d = is_nan ? 256u : (key >> shift) & 0xFFu;
                // equal variances are the rule (the leading zeros, silence): the first wanted lane's digit is added once per wavefront
                const unsigned long long m = __ballot(want);
                if (m) {
                    const int leader = __ffsll((long long)m) - 1;
                    const uint32_t ld = __shfl(d, leader);
                    const unsigned long long same = __ballot(want && d == ld);
                    if ((int)lane == leader) atomicAdd(&hist[ld], (uint32_t)__popcll(same));
                    else if (want && d != ld) atomicAdd(&hist[d], 1u);
                }
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t verdict = 0, acc = 0, d = 0;
            if (pass == 0) { s_next[3] = hist[256]; if (q.kidx >= q.t - hist[256]) verdict = 1; }   // numbers[n] panics (numerics.rs:132)
            if (!verdict) {
                for (; d < 256; ++d) { if (rank - acc < hist[d]) break; acc += hist[d]; }
                if (d == 256) verdict = 1;
            }
            s_next[0] = (d & 0xFFu) << shift; s_next[1] = rank - acc; s_next[2] = verdict;
        }
        __syncthreads();
        if (pass == 0) nan = s_next[3];
        prefix |= s_next[0]; rank = s_next[1]; bad = s_next[2] != 0;
        mask |= 0xFFu << shift;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const uint32_t u = (prefix & 0x80000000u) ? (prefix & 0x7FFFFFFFu) : ~prefix;   // invert order_key
        VatResult r;
        r.th = bad ? 0.0f : __builtin_bit_cast(float, u);
        r.status = bad ? APD_ERR_INDEX : APD_OK;
        r.nan = nan; r.count = 0;
        res[blockIdx.x] = r;
    }
}

// The scan of spectrogram.rs:202-214 for one recording per workgroup, blockDim columns per step.  A column is above (v >= th),
// below (v < th) or neither (NaN); with A, B the ballots of a wavefront, N = ~(A | B) and c = "not recording" on entry,
//   an above column opens a run  iff the nearest classified column before it is below:  opens  = A & ((B << 1) + N + c) & (A | B)
//   a below column closes a run  iff the nearest classified column before it is above:  closes = B & ((A << 1) + N + !c) & (A | B)
// (a carry entered behind a below column ripples through the unclassified ones and stops on the next classified one).  The
// state carried from step to step and from wavefront to wavefront is "recording?" and the current start; every wavefront
// derives its entry state from the ballots of all wavefronts (LDS), one wavefront per lane, without a loop.  WRITE: the ranges
// go to ranges[range_off[s] ..) in ascending order, below `capacity` only; otherwise the count goes to res[s].count.
struct ScanState { bool recording; uint32_t start; };
__device__ __forceinline__ void scan_masks(unsigned long long A, unsigned long long B, bool recording, unsigned long long &opens, unsigned long long &closes)
{
    const unsigned long long nn = A | B;
    opens = A & ((B << 1) + ~nn + (recording ? 0ull : 1ull)) & nn;
    closes = B & ((A << 1) + ~nn + (recording ? 1ull : 0ull)) & nn;
}
template <bool WRITE>
__global__ __launch_bounds__(1024) void vat_scan_kernel(const float *__restrict__ var, const VatSeq *__restrict__ seq, VatResult *__restrict__ res,
                                                        uint64_t min_len, const uint64_t *__restrict__ range_off, ulonglong2 *__restrict__ ranges,
                                                        uint64_t capacity)
{
    __shared__ unsigned long long s_a[2][16], s_b[2][16];
    __shared__ uint32_t s_cnt[2][16];
    const VatSeq q = seq[blockIdx.x];
    const VatResult r = res[blockIdx.x];
    if (r.status != APD_OK) return;                                  // no ranges; the count stays 0
    const float *x = var + q.off, th = r.th;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63, n_waves = blockDim.x >> 6;
    const unsigned long long below_me = (1ull << lane) - 1;
    ScanState st{true, 0};                                           // :202, the scan starts "recording"
    uint64_t emitted = 0;                                            // WRITE: ranges of the steps before; else: of this wavefront alone
    const uint64_t out0 = WRITE ? range_off[blockIdx.x] : 0;
    uint32_t parity = 0;
    for (uint64_t e0 = 0; e0 < q.t; e0 += blockDim.x, parity ^= 1) {
        const uint64_t e = e0 + threadIdx.x;
        const bool live = e < q.t;
        const float v = live ? x[e] : 0.0f;
        const unsigned long long A = __ballot(live && v >= th), B = __ballot(live && v < th);
        if (lane == 0) { s_a[parity][wave] = A; s_b[parity][wave] = B; }
        __syncthreads();
        // The same carry rule one level up, by every wavefront for itself: lane l takes wavefront l's ballots (lane n_waves: none,
        // its entry state is the state after the step).  Wavefront l is entered "recording" iff the last classified column of the
        // nearest wavefront before it that has one is above, and with the start of the nearest wavefront before it that opens a run.
        const unsigned long long a_l = lane < n_waves ? s_a[parity][lane] : 0ull, b_l = lane < n_waves ? s_b[parity][lane] : 0ull, nn_l = a_l | b_l;
        const bool last_above = nn_l && ((a_l >> (63 - __clzll((long long)nn_l))) & 1ull);
        const unsigned long long ends_above = __ballot(last_above), ends_any = __ballot(nn_l != 0) & below_me;
        const bool rec_l = ends_any ? (ends_above >> (63 - __clzll((long long)ends_any))) & 1ull : st.recording;
        unsigned long long opens_l, closes_l;
        scan_masks(a_l, b_l, rec_l, opens_l, closes_l);
        const uint32_t open_l = (uint32_t)e0 + lane * 64 + (opens_l ? 63 - __clzll((long long)opens_l) : 0);
        const unsigned long long opened = __ballot(opens_l != 0) & below_me;
        const uint32_t open_before = __shfl(open_l, opened ? 63 - __clzll((long long)opened) : 0);
        const uint32_t start_l = opened ? open_before : st.start;
        const ScanState in{__shfl((int)rec_l, (int)wave) != 0, (uint32_t)__shfl(start_l, (int)wave)};
        st = ScanState{__shfl((int)rec_l, (int)n_waves) != 0, (uint32_t)__shfl(start_l, (int)n_waves)};
        unsigned long long opens, closes;
        scan_masks(A, B, in.recording, opens, closes);
        const unsigned long long before = opens & below_me;
        const uint32_t start = before ? (uint32_t)e0 + wave * 64 + (63 - __clzll((long long)before)) : in.start;
        const bool emit = ((closes >> lane) & 1ull) && e - start > min_len;          // :211
        const unsigned long long emits = __ballot(emit);
        if (WRITE) {
            if (lane == 0) s_cnt[parity][wave] = (uint32_t)__popcll(emits);
            __syncthreads();
            uint64_t slot = emitted + __popcll(emits & below_me);
            for (uint32_t w = 0; w < n_waves; ++w) { const uint32_t c = s_cnt[parity][w]; if (w < wave) slot += c; emitted += c; }
            if (emit && out0 + slot < capacity) ranges[out0 + slot] = make_ulonglong2(start, e);
        } else {
            emitted += __popcll(emits);
        }
    }
    if (!WRITE && lane == 0 && emitted) atomicAdd(&res[blockIdx.x].count, (uint32_t)emitted);
}

// ---- slices -------------------------------------------------------------------------------------------------------------------------
// out[slice_off[r] .. slice_off[r + 1]) = samples[src[r] ..): a work-item owns one 16-byte-aligned group of eight output samples
// (the first owns what lies in front of the first aligned address).  A whole group inside one slice is one 16-byte store, fed by
// one 16-byte load when the source is aligned as well and by eight 2-byte loads when it is not; a group that straddles slices, or
// the last one, goes sample by sample.
struct GatherParams {
    const int16_t *samples;
    const uint64_t *slice_off;     // [n_slices + 1]
    const uint64_t *src;           // [n_slices] first sample of every slice in `samples`
    uint64_t n_slices, total;
    int16_t *out;
    uint32_t head;                 // samples in front of the first 16-byte-aligned output address
};
__global__ __launch_bounds__(256) void slice_gather_kernel(const GatherParams P)
{
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t lo = g == 0 ? 0 : P.head + (g - 1) * 8;
    if (lo >= P.total) return;
    const uint64_t hi = min(g == 0 ? (uint64_t)P.head : lo + 8, P.total);
    uint64_t r = 0;                                                  // the slice of sample lo: the last one that starts at or before it
    for (uint64_t top = P.n_slices; top - r > 1;) { const uint64_t mid = (r + top) >> 1; if (P.slice_off[mid] <= lo) r = mid; else top = mid; }
    uint64_t r_end = P.slice_off[r + 1];
    if (hi - lo == 8 && hi <= r_end) {
        const int16_t *sp = P.samples + P.src[r] + (lo - P.slice_off[r]);
        uint4 w;
        if (((uintptr_t)sp & 15) == 0) {
            w = *reinterpret_cast<const uint4 *>(sp);
        } else {
            auto pair = [sp](int j) { return (uint32_t)(uint16_t)sp[j] | ((uint32_t)(uint16_t)sp[j + 1] << 16); };
            w = make_uint4(pair(0), pair(2), pair(4), pair(6));
        }
        *reinterpret_cast<uint4 *>(P.out + lo) = w;
        return;
    }
    for (uint64_t o = lo; o < hi; ++o) {
        while (o >= r_end) { ++r; r_end = P.slice_off[r + 1]; }      // empty slices are stepped over; o < total = slice_off[n_slices]
        P.out[o] = P.samples[P.src[r] + (o - P.slice_off[r])];
    }
}

// Both offset arrays ascend, range_off starts at 0 (so every entry is at most range_off[n_seq], which sizes the outputs), and
// ranges are there when any are named: checked as a whole before slice_plan writes, or a caller sizes, anything.
int slice_offsets_ok(const uint64_t *sample_offsets, const uint64_t *range_off, const uint64_t *ranges, uint32_t n_seq)
{
    if (!range_off || (n_seq && !sample_offsets) || range_off[0] != 0) return APD_ERR_INVALID_ARG;
    for (uint32_t s = 0; s < n_seq; ++s)
        if (sample_offsets[s + 1] < sample_offsets[s] || range_off[s + 1] < range_off[s]) return APD_ERR_INVALID_ARG;
    if (range_off[n_seq] && !ranges) return APD_ERR_INVALID_ARG;
    return APD_OK;
}

// The host side of both slice calls: checks every range against its recording, fills slice_offsets / slice_seq / src (any may be
// null).  APD_ERR_INVALID_ARG for descending offsets, stop < start, ranges of a recording that are not ascending, and a range
// that runs past its recording.
int slice_plan(const uint64_t *sample_offsets, const uint64_t *range_off, const uint64_t *ranges, uint32_t n_seq, uint32_t fft_step,
               uint64_t *slice_offsets, uint32_t *slice_seq, uint64_t *src, uint64_t *total)
{
    if (const int rc = slice_offsets_ok(sample_offsets, range_off, ranges, n_seq)) return rc;
    uint64_t acc = 0;
    if (slice_offsets) slice_offsets[0] = 0;
    for (uint32_t s = 0; s < n_seq; ++s) {
        const uint64_t len = sample_offsets[s + 1] - sample_offsets[s];
        uint64_t prev_stop = 0;
        for (uint64_t r = range_off[s]; r < range_off[s + 1]; ++r) {
            const uint64_t start = ranges[2 * r], stop = ranges[2 * r + 1];
            if (stop < start || start < prev_stop) return APD_ERR_INVALID_ARG;
            if (fft_step && stop > len / fft_step) return APD_ERR_INVALID_ARG;          // stop * fft_step > len, without the overflow
            prev_stop = stop;
            if (src) src[r] = sample_offsets[s] + start * fft_step;
            if (slice_seq) slice_seq[r] = s;
            acc += (stop - start) * fft_step;
            if (slice_offsets) slice_offsets[r + 1] = acc;
        }
    }
    if (total) *total = acc;
    return APD_OK;
}

// Both entry points; `who` is the one called, for the texts of apd_last_error.
int interesting_ranges(const char *who, apd_context *ctx, const float *frames, const uint64_t *frame_offsets, uint32_t n_seq,
                       uint32_t n_bins, uint32_t moving_average, float perc, uint64_t min_len, int on_device, uint64_t *range_off,
                       uint64_t *ranges, uint64_t capacity, int32_t *status)
{
    if (!ctx || !range_off || n_bins == 0 || (n_seq && !frame_offsets) || (capacity && !ranges)) return APD_ERR_INVALID_ARG;
    for (uint32_t s = 0; s < n_seq; ++s)
        if (frame_offsets[s + 1] < frame_offsets[s]) return APD_ERR_INVALID_ARG;
    for (uint32_t s = 0; s <= n_seq; ++s) range_off[s] = 0;
    if (n_seq == 0) return APD_OK;
    const uint64_t base = frame_offsets[0], T = frame_offsets[n_seq] - base;
    if (T && !frames) return APD_ERR_INVALID_ARG;
    // what the kernels read: the recordings, their tiles, and a place for the second pass' range offsets -- one upload
    const size_t seq_bytes = (size_t)n_seq * sizeof(VatSeq), tile_bytes = (((size_t)n_seq + 1) * sizeof(uint32_t) + 15) & ~(size_t)15;
    std::vector<uint64_t> h_meta((seq_bytes + tile_bytes) / sizeof(uint64_t));
    VatSeq *h_seq = reinterpret_cast<VatSeq *>(h_meta.data());
    uint32_t *h_tile = reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(h_meta.data()) + seq_bytes);
    uint64_t tiles = 0;
    uint32_t t_max = 0;
    for (uint32_t s = 0; s < n_seq; ++s) {
        const uint64_t t = frame_offsets[s + 1] - frame_offsets[s];
        if (t > 0xFFFFFFFFull) { ctx->last_error = std::string(who) + ": a recording of 2^32 frames or more"; return APD_ERR_UNSUPPORTED; }
        const uint64_t kidx = percentile_index(t, perc);
        h_seq[s] = VatSeq{frame_offsets[s] - base, (uint32_t)t, (uint32_t)std::min<uint64_t>(kidx, 0xFFFFFFFFull)};   // >= t either way: a panic
        h_tile[s] = (uint32_t)tiles;
        tiles += (t + kVatTile - 1) / kVatTile;
        t_max = std::max(t_max, (uint32_t)t);
        if (tiles >= (1ull << 31)) { ctx->last_error = std::string(who) + ": 2^39 frames or more"; return APD_ERR_UNSUPPORTED; }
    }
    h_tile[n_seq] = (uint32_t)tiles;
    HIP_TRY(ctx, bind_device(ctx));
    const bool halo_in_lds = moving_average <= kVatHaloMax;
    auto round = [](size_t n) { return (n + 255) & ~(size_t)255; };
    const size_t o_meta = 0, o_res = round(seq_bytes + tile_bytes), o_roff = o_res + round((size_t)n_seq * sizeof(VatResult));
    const size_t o_var = o_roff + round(((size_t)n_seq + 1) * sizeof(uint64_t)), o_std = o_var + round(T * sizeof(float));
    // the ranges the second pass may write: no more than the capacity, and a recording holds at most t / (min_len + 2) of them
    // (each takes more than min_len frames and the frame that closes it) -- known before the counts are, so nothing is allocated
    // between the two passes
    uint64_t range_bound = 0;
    for (uint32_t s = 0; s < n_seq; ++s) range_bound += h_seq[s].t / (std::min<uint64_t>(min_len, 0xFFFFFFFFull) + 2);
    range_bound = std::min(range_bound, capacity);
    const size_t o_rng = o_std + (halo_in_lds ? 0 : round(T * sizeof(float))), o_in = o_rng + round(range_bound * sizeof(ulonglong2));
    const size_t in_bytes = on_device ? 0 : (size_t)T * n_bins * sizeof(float);
    if (const int rc = reserve_ws(ctx, ctx->ws_misc, o_in + round(in_bytes) + 256)) return rc;
    char *ws = ctx->ws_misc.as<char>();
    VatParams P{};
    P.seq = reinterpret_cast<const VatSeq *>(ws + o_meta);
    P.tile_first = reinterpret_cast<const uint32_t *>(ws + o_meta + seq_bytes);
    P.n_seq = n_seq; P.n_bins = n_bins; P.k = moving_average;
    P.var = reinterpret_cast<float *>(ws + o_var);
    P.stds = reinterpret_cast<float *>(ws + o_std);
    P.frames = on_device ? frames + base * n_bins : reinterpret_cast<const float *>(ws + o_in);
    VatResult *d_res = reinterpret_cast<VatResult *>(ws + o_res);
    uint64_t *d_roff = reinterpret_cast<uint64_t *>(ws + o_roff);
    APD_AFFINITY(ctx, "VAT batch launch");
    HIP_TRY(ctx, hipMemcpyAsync(ws + o_meta, h_meta.data(), seq_bytes + tile_bytes, hipMemcpyHostToDevice, ctx->stream));
    if (in_bytes) HIP_TRY(ctx, hipMemcpyAsync(ws + o_in, frames + base * n_bins, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    if (tiles) {
        const bool staged = n_bins <= kVatStageBins;
        const size_t stage_bytes = staged ? (size_t)(kVatTile / 64) * 64 * (n_bins | 1) * sizeof(float) : 0;
        if (halo_in_lds) {
            hipLaunchKernelGGL(vat_variance_kernel<0>, dim3((unsigned)tiles), dim3(kVatTile), (kVatTile + kVatHaloMax) * sizeof(float) + stage_bytes,
                               ctx->stream, P);
        } else {
            hipLaunchKernelGGL(vat_variance_kernel<1>, dim3((unsigned)tiles), dim3(kVatTile), stage_bytes, ctx->stream, P);
            hipLaunchKernelGGL(vat_variance_kernel<2>, dim3((unsigned)tiles), dim3(kVatTile), 0, ctx->stream, P);
        }
    }
    // a workgroup per recording: 256 work-items where none is long (more recordings per compute unit), 1024 otherwise
    const unsigned wg = t_max <= 8192 ? 256 : 1024;
    hipLaunchKernelGGL(vat_select_kernel, dim3(n_seq), dim3(wg), 0, ctx->stream, P.var, P.seq, d_res);
    hipLaunchKernelGGL(vat_scan_kernel<false>, dim3(n_seq), dim3(wg), 0, ctx->stream, P.var, P.seq, d_res, min_len, nullptr, nullptr, 0);
    HIP_TRY(ctx, hipGetLastError());
    std::vector<VatResult> h_res(n_seq);
    HIP_TRY(ctx, hipMemcpyAsync(h_res.data(), d_res, (size_t)n_seq * sizeof(VatResult), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));                 // the one read-back of verdicts and counts
    std::vector<uint64_t> h_roff((size_t)n_seq + 1, 0);
    for (uint32_t s = 0; s < n_seq; ++s) {
        if (h_res[s].status != APD_OK && !status) {
            ctx->last_error = std::string(who) + ": recording " + std::to_string(s) + ": the percentile's index is beyond its " +
                              std::to_string((uint64_t)h_seq[s].t - h_res[s].nan) + " non-NaN variances (numerics.rs:132)";
            return APD_ERR_INDEX;                                    // range_off is all zero
        }
        if (status) status[s] = h_res[s].status;
        h_roff[s + 1] = h_roff[s] + (h_res[s].status == APD_OK ? h_res[s].count : 0);
    }
    std::memcpy(range_off, h_roff.data(), h_roff.size() * sizeof(uint64_t));
    const uint64_t n_write = std::min(h_roff[n_seq], capacity);
    if (n_write == 0) return APD_OK;
    ulonglong2 *d_ranges = reinterpret_cast<ulonglong2 *>(ws + o_rng);   // n_write <= range_bound
    HIP_TRY(ctx, hipMemcpyAsync(d_roff, h_roff.data(), h_roff.size() * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(vat_scan_kernel<true>, dim3(n_seq), dim3(wg), 0, ctx->stream, P.var, P.seq, d_res, min_len, d_roff, d_ranges, n_write);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(ranges, d_ranges, n_write * sizeof(ulonglong2), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return APD_OK;
}

}  // namespace

extern "C" int apd_interesting_ranges_batch(apd_context *ctx, const float *frames, const uint64_t *frame_offsets, uint32_t n_seq,
                                            uint32_t n_bins, uint32_t moving_average, float perc, uint64_t min_len, int on_device,
                                            uint64_t *range_off, uint64_t *ranges, uint64_t capacity, int32_t *status)
{
    return interesting_ranges("apd_interesting_ranges_batch", ctx, frames, frame_offsets, n_seq, n_bins, moving_average, perc, min_len,
                              on_device, range_off, ranges, capacity, status);
}

// A batch of one.  Where the reference panics, APD_ERR_INDEX is the batch's verdict for its only recording.
extern "C" int apd_interesting_ranges(apd_context *ctx, const float *frames, uint64_t t, uint32_t n_bins, uint32_t moving_average,
                                      float perc, uint64_t min_len, int on_device, uint64_t *ranges, uint64_t capacity,
                                      uint64_t *n_ranges)
{
    if (!ctx || !n_ranges || n_bins == 0 || (t && !frames) || (capacity && !ranges)) return APD_ERR_INVALID_ARG;
    *n_ranges = 0;
    const uint64_t frame_offsets[2] = {0, t};
    uint64_t range_off[2] = {0, 0};
    const int rc = interesting_ranges("apd_interesting_ranges", ctx, frames, frame_offsets, 1, n_bins, moving_average, perc, min_len,
                                      on_device, range_off, ranges, capacity, nullptr);
    *n_ranges = range_off[1];
    return rc;
}

extern "C" int apd_slice_offsets(const uint64_t *sample_offsets, const uint64_t *range_off, const uint64_t *ranges, uint32_t n_seq,
                                 uint32_t fft_step, uint64_t *slice_offsets, uint32_t *slice_seq)
{
    if (!slice_offsets) return APD_ERR_INVALID_ARG;
    return slice_plan(sample_offsets, range_off, ranges, n_seq, fft_step, slice_offsets, slice_seq, nullptr, nullptr);
}

extern "C" int apd_slice_samples(apd_context *ctx, const int16_t *samples, const uint64_t *sample_offsets, uint32_t n_seq,
                                 const uint64_t *range_off, const uint64_t *ranges, uint32_t fft_step, int on_device, int16_t *out,
                                 uint64_t capacity)
{
    if (!ctx) return APD_ERR_INVALID_ARG;
    if (const int rc = slice_offsets_ok(sample_offsets, range_off, ranges, n_seq)) return rc;   // before range_off[n_seq] sizes anything
    const uint64_t n_slices = range_off[n_seq];
    std::vector<uint64_t> h;                                         // slice offsets, then the slices' first source samples
    try { h.resize((size_t)2 * n_slices + 1); } catch (const std::exception &) { return APD_ERR_OOM; }
    uint64_t total = 0;
    if (const int rc = slice_plan(sample_offsets, range_off, ranges, n_seq, fft_step, h.data(), nullptr, h.data() + n_slices + 1, &total)) return rc;
    if (total > capacity || (total && (!samples || !out))) return APD_ERR_INVALID_ARG;
    if (total == 0) return APD_OK;
    const uint64_t n_samples = sample_offsets[n_seq], groups = 1 + (total + 7) / 8;
    if ((groups + 255) / 256 >= (1ull << 31)) { ctx->last_error = "apd_slice_samples: 2^42 samples or more"; return APD_ERR_UNSUPPORTED; }
    HIP_TRY(ctx, bind_device(ctx));
    auto round = [](size_t n) { return (n + 255) & ~(size_t)255; };
    const size_t o_in = round(h.size() * sizeof(uint64_t)), o_out = o_in + (on_device ? 0 : round(n_samples * sizeof(int16_t)));
    if (const int rc = reserve_ws(ctx, ctx->ws_misc, o_out + (on_device ? 0 : round(total * sizeof(int16_t))) + 256)) return rc;
    char *ws = ctx->ws_misc.as<char>();
    APD_AFFINITY(ctx, "slice gather launch");
    HIP_TRY(ctx, hipMemcpyAsync(ws, h.data(), h.size() * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    if (!on_device) HIP_TRY(ctx, hipMemcpyAsync(ws + o_in, samples, n_samples * sizeof(int16_t), hipMemcpyHostToDevice, ctx->stream));
    GatherParams G{};
    G.samples = on_device ? samples : reinterpret_cast<const int16_t *>(ws + o_in);
    G.slice_off = reinterpret_cast<const uint64_t *>(ws);
    G.src = G.slice_off + n_slices + 1;
    G.n_slices = n_slices; G.total = total;
    G.out = on_device ? out : reinterpret_cast<int16_t *>(ws + o_out);
    G.head = (uint32_t)std::min<uint64_t>(((16 - ((uintptr_t)G.out & 15)) & 15) / sizeof(int16_t), total);
    hipLaunchKernelGGL(slice_gather_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, ctx->stream, G);
    HIP_TRY(ctx, hipGetLastError());
    if (!on_device) HIP_TRY(ctx, hipMemcpyAsync(out, G.out, total * sizeof(int16_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return APD_OK;
}
