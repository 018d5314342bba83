// Generic fused-pair banded DTW + layout/unpack helpers + kernel dispatch (gfx950).
//
// Replaces the per-pair body of AlignmentWorkers::align_all (reference src/alignments.rs:50-58):
// Alignment::new + construct_alignment (:165-180) + alignment_score (:129-160) + score (:116-125).
//
// Work unit: one UNORDERED pair (a, b), a < b.  One sweep computes BOTH ordered scores
//   DP1 = score(x = a, y = b)  and  DP2 = score(x = b, y = a),
// because the two recurrences visit (almost) the same cells and share every local distance
// euclidean(A[i], B[j]) (numerics.rs:114-120).  In A-row / B-column coordinates (i over A, j over B, band
// offset o = j - i, u = o + w):
//   DP1: u in [0, 2w-1], left neighbour (i, j-1) is the DELETE branch, up (i-1, j) the INSERT branch;
//   DP2: u in [1, 2w],   up   neighbour is the DELETE branch, left the INSERT branch
// (DP2's cell (j, i) of the swapped problem is our cell (i, j); the reference band j'-i' in [-w, w-1] of
// alignments.rs:175 becomes o in [-w+1, w]).  Each DP is exactly the reference recurrence for its ordered pair.
//
// Lane mapping: a lane owns C consecutive offsets u = C*l + c.  Macro-step tau: every lane processes row
// i = tau - l, its C cells left to right.  Dependences across lanes:
//   (i, u-1) of the first cell  = last cell of lane l-1 from the PREVIOUS macro-step  -> DPP shift up
//   (i-1, u+1) of the last cell = first cell of lane l+1 from THIS macro-step          -> DPP shift down
// so C >= 2 and the min(INS, DEL, MATCH) dependency never goes through memory.
// Only rows 1..n-1 and columns 1..m-1 are swept: score() reads cell (n-1, m-1) (alignments.rs:120); row n and
// column m never influence it.
//
// The kernel in this file is the slow, fully general one: any frame dimension, any band up to what 160 KB of LDS
// holds (C chosen at run time, per-lane DP rows in LDS, every boundary tested per cell, any penalty values).
// dtw_systolic.h holds the production kernel.
#include <algorithm>
#include <cmath>
#include <type_traits>
#include "dtw_common.h"

namespace apd {

__device__ __forceinline__ void generic_pair(const AlignLaunch &L, int c_max, uint32_t wave, float *lds)
{
    const int lane = threadIdx.x;
    const uint32_t tile = wave / kSlotsPerTile, slot = wave % kSlotsPerTile;
    const PairInfo P = decode_pair(L, tile, slot);
    if (!P.valid) return;
    const int n = P.n, m = P.m, w = P.w;
    if (n == 1 || m == 1) {                                   // alignments.rs:116-125 with an absent cell
        if (lane == 0) { const float s = (n == 1 && m == 1) ? 0.0f : APD_INF; store_pair(L, tile, P, s, s); }
        return;
    }
    const float ins = L.band.ins, del = L.band.del, mat = L.band.mat;
    const int two_w = 2 * w;
    int C = (two_w + 1 + 63) / 64;
    C = max(C, 2);
    float *p1 = lds, *p2 = lds + c_max * 64;               // [c][lane]
    for (int c = 0; c < C; ++c) { p1[c * 64 + lane] = APD_INF; p2[c * 64 + lane] = APD_INF; }
    const int dp4 = (int)L.dpad / 4, dim = (int)L.dim;
    const int u0 = C * lane;
    const int g_act = (two_w + 1 + C - 1) / C;
    const int total = (n - 1) + g_act;
    float res1 = 0.0f, res2 = 0.0f;
    float last1 = APD_INF, last2 = APD_INF;
    for (int tau = 0; tau < total; ++tau) {
        const int i = tau - lane;
        const int jb = i + u0 - w;
        const float4 *xa = reinterpret_cast<const float4 *>(P.A + (uint64_t)(min(max(i, 1), n) - 1) * L.dpad);
        float left1 = from_lower_lane(last1, APD_INF);
        float left2 = from_lower_lane(last2, APD_INF);
        float upr1 = APD_INF, upr2 = APD_INF;
        float nxt1 = p1[lane], nxt2 = p2[lane];             // prev[c] for c = 0
        for (int c = 0; c < C; ++c) {
            const int j = jb + c, u = u0 + c;
            const float4 *yb = reinterpret_cast<const float4 *>(P.B + (uint64_t)(min(max(j, 1), m) - 1) * L.dpad);
            // numerics.rs:114-120 operation for operation (difference, square, sum each rounded; correctly rounded sqrt):
            // this kernel serves every penalty setting, and with unequal penalties near-ties must resolve as on the CPU
            float acc = 0.0f;
            for (int q = 0; q < dp4; ++q) {                  // slots >= dim hold the squared norm / padding: skipped
                const float4 xv = xa[q], yv = yb[q];
                const int k0 = 4 * q;
                float t = xv.x - yv.x, sq = t * t;
                acc = (k0 < dim) ? acc + sq : acc;
                t = xv.y - yv.y; sq = t * t; acc = (k0 + 1 < dim) ? acc + sq : acc;
                t = xv.z - yv.z; sq = t * t; acc = (k0 + 2 < dim) ? acc + sq : acc;
                t = xv.w - yv.w; sq = t * t; acc = (k0 + 3 < dim) ? acc + sq : acc;
            }
            const float d = __builtin_sqrtf(acc);
            const float m1 = nxt1, m2 = nxt2;
            float up1, up2;
            if (c < C - 1) { up1 = p1[(c + 1) * 64 + lane]; up2 = p2[(c + 1) * 64 + lane]; }
            else { up1 = upr1; up2 = upr2; }
            nxt1 = up1; nxt2 = up2;                          // prev[c+1] is the next cell's MATCH predecessor
            float r1 = select_node<false>(left1, up1, m1, d, del, ins, mat);   // DP1: left = DELETE, up = INSERT
            float r2 = select_node<false>(up2, left2, m2, d, del, ins, mat);   // DP2: up = DELETE, left = INSERT
            const bool inside = (i >= 1) & (j >= 1);
            const float inv = ((i == 0) & (j == 0)) ? 0.0f : APD_INF;          // D[0][0] = 0 (alignments.rs:109)
            r1 = (inside & (u <= two_w - 1)) ? r1 : inv;
            r2 = (inside & (u >= 1) & (u <= two_w)) ? r2 : inv;
            if ((i == n - 1) & (j == m - 1)) { res1 = r1; res2 = r2; }
            p1[c * 64 + lane] = r1; p2[c * 64 + lane] = r2;
            left1 = r1; left2 = r2;
            if (c == 0) { upr1 = from_upper_lane(r1, APD_INF); upr2 = from_upper_lane(r2, APD_INF); }
        }
        last1 = left1; last2 = left2;
    }
    const int ustar = (m - 1) - (n - 1) + w;
    if (lane == ustar / C) {
        const float denom = (float)(n + m);                  // alignments.rs:121
        store_pair(L, tile, P, res1 / denom, res2 / denom);
    }
}

// one wavefront per pair slot
__global__ __launch_bounds__(64) void dtw_fused_generic(const AlignLaunch L, int c_max)
{
    extern __shared__ float lds[];
    generic_pair(L, c_max, blockIdx.x, lds);
}

// The same as the fallback behind the fast kernels: a small persistent grid over all pair slots of the launch that returns at
// once unless the batch's non-finite flag is raised (then the fast kernels have returned at once, and this one does the work).
__global__ __launch_bounds__(64) void dtw_fused_generic_fallback(const AlignLaunch L, int c_max, uint32_t total_waves)
{
    extern __shared__ float lds[];
    if (*L.d_nonfinite == 0u) return;
    for (uint32_t wave = blockIdx.x; wave < total_waves; wave += gridDim.x) {
        generic_pair(L, c_max, wave, lds);
        __syncthreads();                                     // the DP rows in LDS are reused by the next pair
    }
}

// ------------------------------------------------------------------------------------------------
// Resident layout: sequences in length order (apd_length_order), per sequence [frames | sentinel H | sentinel E],
// seq_off[p] = resident_offsets[p] + 2 p; src_off[p] = first frame of that sequence in the caller's array.  A frame is dpad =
// ceil4(dim + 1) floats: the dim components, then the squared norm sum_k x_k^2 (slot dim), then zeros.  Sentinel H has
// zero components and norm +INF (hybrid distances), sentinel E has +INF components (difference-form distances).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pad_frames_kernel(const float *__restrict__ src, float *__restrict__ dst, const uint32_t *__restrict__ seq_off,
                                  const uint32_t *__restrict__ src_off, uint32_t n_seq, uint64_t n_frames_padded, uint32_t src_dim,
                                  uint32_t dim, uint32_t dpad, uint32_t *__restrict__ flags, float *__restrict__ seq_nmax)
{
    // One thread per 16-byte piece of a resident frame (dpad / 4 pieces per frame, dpad / 4 consecutive lanes -- a power of
    // two up to 8 for the instantiated dimensions, any count otherwise): one search for the frame's sequence per piece,
    // contiguous reads of the source frame, one aligned 16-byte store; the squared norm is summed in f64 over the lanes of
    // the frame.  (The first version ran one thread, one search and one 4-byte store per FLOAT: 0.48 TB/s.)
    const uint32_t ppf = dpad / 4;                                // pieces per frame
    const uint64_t total = n_frames_padded * ppf;
    bool nonfinite = false;
    const bool shuffle_ok = (ppf & (ppf - 1)) == 0 && ppf <= 64;  // the lanes of a frame sit in one wavefront, aligned
    for (uint64_t e0 = (uint64_t)blockIdx.x * blockDim.x; e0 < total; e0 += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t e = e0 + threadIdx.x;
        const bool live = e < total;
        const uint32_t f = live ? (uint32_t)(e / ppf) : 0u, q = live ? (uint32_t)(e - (uint64_t)f * ppf) : 0u;
        // largest s with seq_off[s] <= f: one search per wavefront (for its first frame), then a step or two forward per lane
        const uint32_t f_first = (uint32_t)__builtin_amdgcn_readfirstlane((int)f);
        uint32_t lo = 0, hi = n_seq;
        while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (seq_off[mid] <= f_first) lo = mid; else hi = mid; }
        while (live && lo + 1 < n_seq && seq_off[lo + 1] <= f) ++lo;
        const bool sent_e = live && (f + 1 == seq_off[lo + 1]), sent_h = live && (f + 2 == seq_off[lo + 1]);
        const bool real = live && !sent_e && !sent_h;
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        double part = 0.0;                                        // this piece's share of sum_k x_k^2
        if (real) {
            const float *fr = src + (uint64_t)(src_off[lo] + (f - seq_off[lo])) * src_dim;
#pragma unroll
            for (uint32_t i = 0; i < 4; ++i) {
                const uint32_t k = 4 * q + i;
                if (k < src_dim) {                                // components src_dim .. dim - 1 stay zero
                    v[i] = fr[k];
                    // outside [kFeatureFloor, kFeatureBound) and not 0: NaN, +-INF, so large that a squared distance could overflow, or
                    // so small that one could be subnormal.  On the bits of |v| (they order like the magnitudes, NaN above +INF): a
                    // subnormal feature is seen as what it is whatever the denormal mode of the float compare.
                    const uint32_t mag = __builtin_bit_cast(uint32_t, v[i]) & 0x7FFFFFFFu;
                    nonfinite |= mag != 0u && (mag < __builtin_bit_cast(uint32_t, kFeatureFloor) || mag >= __builtin_bit_cast(uint32_t, kFeatureBound));
                    part += (double)v[i] * (double)v[i];
                }
            }
        }
        double norm = part;
        if (ppf == 4) {                                           // D <= 14: the four pieces of a frame are one DPP quad
            auto quad_swap = [](double x, auto ctrl) __attribute__((always_inline)) {
                constexpr int CTRL = decltype(ctrl)::value;
                const unsigned long long b = __builtin_bit_cast(unsigned long long, x);
                const unsigned int lo32 = (unsigned int)__builtin_amdgcn_update_dpp(0, (int)(unsigned int)b, CTRL, 0xf, 0xf, false);
                const unsigned int hi32 = (unsigned int)__builtin_amdgcn_update_dpp(0, (int)(unsigned int)(b >> 32), CTRL, 0xf, 0xf, false);
                return __builtin_bit_cast(double, ((unsigned long long)hi32 << 32) | lo32);
            };
            norm += quad_swap(norm, std::integral_constant<int, 0xB1>{});   // quad_perm [1,0,3,2]
            norm += quad_swap(norm, std::integral_constant<int, 0x4E>{});   // quad_perm [2,3,0,1]
        } else if (shuffle_ok) {
            for (uint32_t o = 1; o < ppf; o <<= 1) norm += __shfl_xor(norm, (int)o);
        } else if (real) {                                        // generic dimension: the piece holding slot `dim` re-reads the frame
            norm = 0.0;
            if (dim / 4 == q) {
                const float *fr = src + (uint64_t)(src_off[lo] + (f - seq_off[lo])) * src_dim;
                for (uint32_t t = 0; t < src_dim; ++t) norm += (double)fr[t] * (double)fr[t];
            }
        }
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) {
            const uint32_t k = 4 * q + i;
            if (sent_e) v[i] = (k <= dim) ? APD_INF : 0.0f;
            else if (sent_h) v[i] = (k == dim) ? APD_INF : 0.0f;
            else if (real && k == dim) v[i] = (float)norm;
        }
        {
            // largest norm of the sequence: non-negative floats order like their bit patterns (a NaN norm flags the batch anyway).
            // The frames of a wavefront almost always belong to one sequence: one atomic per wavefront then, not one per frame.
            const float mine = (real && dim / 4 == q && norm == norm) ? (float)norm : 0.0f;
            const bool has = real && dim / 4 == q;
            const uint32_t lo_first = (uint32_t)__builtin_amdgcn_readfirstlane((int)lo);
            const unsigned long long any_has = __ballot(has);
            if (__ballot(has && lo != lo_first) == 0ull) {
                float m = mine;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) m = fmaxf(m, __shfl_xor(m, o));
                if ((threadIdx.x & 63) == 0 && any_has != 0ull) atomicMax(reinterpret_cast<unsigned int *>(&seq_nmax[lo_first]), __builtin_bit_cast(unsigned int, m));
            } else if (has) atomicMax(reinterpret_cast<unsigned int *>(&seq_nmax[lo]), __builtin_bit_cast(unsigned int, mine));
        }
        if (live) *reinterpret_cast<float4 *>(dst + e * 4) = make_float4(v[0], v[1], v[2], v[3]);
    }
    // the fast kernels assume finite features (fminf-based select, +INF sentinels, norm expansion) and finite, normal squared
    // distances (sqrt_rn_finite, v_sqrt_f32): a batch with a NaN, an infinity, a feature of magnitude >= 2^60 or a non-zero one below
    // 2^-40 anywhere is routed to the literal kernel, where NaN compares false and takes MATCH as in alignments.rs:153-159, an
    // overflowing distance is +INF and an underflowing one is the subnormal or 0 that it is on the CPU
    if (__ballot(nonfinite) != 0ull && (threadIdx.x & 63) == 0) atomicOr(flags, 1u);
}

// The poison of a score slot no kernel wrote: the 0xFF bytes the slabs are filled with before the alignment launches, compared by
// its bits.  A score may be NaN in its own right -- an infinite penalty on a zero distance (INF * 0), a NaN penalty -- and is then
// the NaN the arithmetic makes (0x7FC00000 on gfx950) or the canonical one the host puts in place of a NaN penalty
// (canonical_penalty, apd_api.hip): never this pattern.
__device__ __forceinline__ bool is_poison(float s) { return __builtin_bit_cast(uint32_t, s) == 0xFFFFFFFFu; }

// gathered: `world` slabs of slab_floats each; slab r holds tiles r, r+world, ... in order.
__global__ void unpack_tiles_kernel(const float *__restrict__ gathered, float *__restrict__ out,
                                    const uint32_t *__restrict__ order, uint32_t n_seq, uint32_t world, uint64_t slab_floats, uint32_t n_tiles_side,
                                    const uint32_t *__restrict__ flags, uint32_t *__restrict__ status)
{
    const uint32_t g = blockIdx.x;                            // (ta, tb), ta <= tb, row-major over the upper triangle
    uint32_t ta = 0, rem = g, row = n_tiles_side;
    while (rem >= row) { rem -= row; ++ta; --row; }
    const uint32_t tb = ta + rem;
    const uint32_t rank = g % world, local = g / world;
    const float *slab = gathered + (uint64_t)rank * slab_floats + (uint64_t)local * 2 * kSlotsPerTile;
    const int sa = threadIdx.x / kTile, sb = threadIdx.x % kTile;
    const uint32_t pa = ta * kTile + sa, pb = tb * kTile + sb;   // positions in the resident (length) order
    bool poisoned = false;
    if (pa < pb && pb < n_seq) {
        const uint32_t a = order[pa], b = order[pb];
        const float s1 = slab[sa * kTile + sb], s2 = slab[kSlotsPerTile + sa * kTile + sb];
        out[(uint64_t)a * n_seq + b] = s1;
        out[(uint64_t)b * n_seq + a] = s2;
        poisoned = is_poison(s1) | is_poison(s2);
    } else if (pa == pb && pb < n_seq) {
        const uint32_t a = order[pa];
        out[(uint64_t)a * n_seq + a] = 0.0f;                  // the diagonal is never aligned (alignments.rs:21-23, 51)
    }
    // every slab is filled with the poison NaN before the alignment launches: a slot that still holds it is a pair no kernel
    // wrote (a launch cut short or skipped).  It stays NaN in the matrix and is reported, never a silent 0.
    if (__ballot(poisoned) != 0ull && (threadIdx.x & 63) == 0 && flags[0] == 0u) atomicOr(status, 1u);
}

// The rectangular unpack of apd_align_cross: one work-item per (position pa of the first resident segment, position pb of the
// second).  slab: [tiles][2][kTile][kTile] over the tile rectangle ta in [0, ceil(n0 / kTile)) x tb in [tb0, tb0 + tiles_b), row-major.
// order[] holds joined caller numbers (first set below n_first, second set from n_first on); `swapped`: the first resident segment
// is the caller's second set.  Same-set pairs that the straddling tiles swept are never read.
__global__ __launch_bounds__(256) void unpack_cross_kernel(const float *__restrict__ slab, float *__restrict__ out_fs, float *__restrict__ out_sf,
                                                           const uint32_t *__restrict__ order, uint32_t n_seq, uint32_t n0, uint32_t n_first,
                                                           uint32_t swapped, uint32_t tb0, uint32_t tiles_b,
                                                           const uint32_t *__restrict__ flags, uint32_t *__restrict__ status)
{
    const uint32_t n1 = n_seq - n0, n_second = n_seq - n_first;
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool poisoned = false;
    if (e < (uint64_t)n0 * n1) {
        const uint32_t pa = (uint32_t)(e / n1), pb = n0 + (uint32_t)(e % n1);   // consecutive lanes: consecutive pb
        const uint32_t ta = pa / kTile, tb = pb / kTile, sa = pa % kTile, sb = pb % kTile;
        const float *t = slab + ((uint64_t)ta * tiles_b + (tb - tb0)) * 2 * kSlotsPerTile;
        const float s1 = t[sa * kTile + sb], s2 = t[kSlotsPerTile + sa * kTile + sb];   // score(x = pa, y = pb), score(x = pb, y = pa)
        const uint32_t a = order[pa], b = order[pb];
        if (!swapped) {                                            // a: first set, b: second set
            if (out_fs) out_fs[(uint64_t)a * n_second + (b - n_first)] = s1;
            if (out_sf) out_sf[(uint64_t)(b - n_first) * n_first + a] = s2;
        } else {                                                   // a: second set, b: first set
            if (out_sf) out_sf[(uint64_t)(a - n_first) * n_first + b] = s1;
            if (out_fs) out_fs[(uint64_t)b * n_second + (a - n_first)] = s2;
        }
        poisoned = is_poison(s1) | is_poison(s2);
    }
    // as in unpack_tiles_kernel: a slot that still holds the poison pattern is a pair no kernel wrote
    if (__ballot(poisoned) != 0ull && (threadIdx.x & 63) == 0 && flags[0] == 0u) atomicOr(status, 1u);
}

// apd_batch_join: the joined batch is out of the fast kernels' feature range if either input is
__global__ void join_flags_kernel(uint32_t *__restrict__ out, const uint32_t *__restrict__ a, const uint32_t *__restrict__ b)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) out[0] = a[0] | b[0];
}

__global__ void selftest_kernel(int *result)
{
    const int lane = threadIdx.x;
    const float v = (float)lane;
    bool ok = true;
    ok &= from_lower_lane(v, -1.0f) == (lane == 0 ? -1.0f : (float)(lane - 1));
    ok &= from_upper_lane(v, -2.0f) == (lane == 63 ? -2.0f : (float)(lane + 1));
    ok &= group_from_lower<16>(v, -3.0f, lane % 16) == (lane % 16 == 0 ? -3.0f : (float)(lane - 1));
    ok &= group_from_upper<16>(v, -4.0f, lane % 16) == (lane % 16 == 15 ? -4.0f : (float)(lane + 1));
    ok &= group_from_lower<32>(v, -5.0f, lane % 32) == (lane % 32 == 0 ? -5.0f : (float)(lane - 1));
    ok &= group_from_upper<32>(v, -7.0f, lane % 32) == (lane % 32 == 31 ? -7.0f : (float)(lane + 1));
    ok &= group_from_upper<32>(v, (float)(100 + lane), lane % 32) == (lane % 32 == 31 ? (float)(100 + lane) : (float)(lane + 1));   // per-lane keep value
    ok &= group_from_upper<8>(v, -6.0f, lane % 8) == (lane % 8 == 7 ? -6.0f : (float)(lane + 1));
    const unsigned long long all = __ballot(ok);
    if (lane == 0) *result = (all == ~0ull) ? 1 : 0;
}

// Exhaustive check of sqrt_rn_finite (dtw_common.h) against the compiler's correctly rounded sqrtf over the bit patterns
// [first, first + count): out[0] = patterns inside the domain (2^-96 <= x < +INF) where the two differ, out[1] = the first such
// pattern + 1, out[2..6] = how often the raw v_sqrt_f32 is off by -2 or less, -1, 0, +1, +2 or more ulps there.
__global__ __launch_bounds__(256) void sqrt_sweep_kernel(uint32_t first, uint64_t count, unsigned long long *out)
{
    unsigned long long bad = 0, hist[5] = {0, 0, 0, 0, 0};
    uint32_t first_bad = 0xFFFFFFFFu;
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < count; e += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t bits = first + (uint32_t)e;
        const float x = __builtin_bit_cast(float, bits);
        if (!(x >= 0x1p-96f && x < APD_INF)) continue;
        const float want = __builtin_sqrtf(x), got = sqrt_rn_finite(x), raw = __builtin_amdgcn_sqrtf(x);
        if (__builtin_bit_cast(uint32_t, want) != __builtin_bit_cast(uint32_t, got)) { ++bad; first_bad = min(first_bad, bits); }
        const int off = __builtin_bit_cast(int, raw) - __builtin_bit_cast(int, want);
        ++hist[off <= -2 ? 0 : off >= 2 ? 4 : off + 2];
    }
    if (bad) { atomicAdd(&out[0], bad); atomicMin(&out[1], (unsigned long long)first_bad + 1ull); }
#pragma unroll
    for (int k = 0; k < 5; ++k) if (hist[k]) atomicAdd(&out[2 + k], hist[k]);
}

hipError_t launch_sqrt_sweep(uint32_t first, uint64_t count, unsigned long long *d_out, hipStream_t stream)
{
    hipLaunchKernelGGL(sqrt_sweep_kernel, dim3(4096), dim3(256), 0, stream, first, count, d_out);
    return hipGetLastError();
}

hipError_t launch_selftest(int *d_result, hipStream_t stream)
{
    hipLaunchKernelGGL(selftest_kernel, dim3(1), dim3(64), 0, stream, d_result);
    return hipGetLastError();
}

hipError_t launch_pad(const float *d_src, float *d_dst, const uint32_t *d_seq_off, const uint32_t *d_src_off, uint32_t n_seq,
                      uint64_t n_frames_padded, uint32_t src_dim, uint32_t dim, uint32_t dpad, uint32_t *d_flags, float *d_seq_nmax,
                      hipStream_t stream)
{
    if (n_frames_padded == 0) return hipSuccess;
    const uint64_t total = n_frames_padded * (dpad / 4);
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((total + 255) / 256, 16384);
    hipLaunchKernelGGL(pad_frames_kernel, dim3(blocks), dim3(256), 0, stream, d_src, d_dst, d_seq_off, d_src_off, n_seq, n_frames_padded,
                       src_dim, dim, dpad, d_flags, d_seq_nmax);
    return hipGetLastError();
}

hipError_t launch_unpack(const float *d_gathered, float *d_out, const uint32_t *d_order, uint32_t n_seq, uint32_t world,
                         uint64_t slab_floats, const uint32_t *d_flags, uint32_t *d_status, hipStream_t stream)
{
    const uint32_t side = (n_seq + kTile - 1) / kTile;
    const uint64_t n_tiles = (uint64_t)side * (side + 1) / 2;
    if (n_tiles == 0) return hipSuccess;
    hipLaunchKernelGGL(unpack_tiles_kernel, dim3((uint32_t)n_tiles), dim3(kSlotsPerTile), 0, stream, d_gathered, d_out,
                       d_order, n_seq, world, slab_floats, side, d_flags, d_status);
    return hipGetLastError();
}

hipError_t launch_join_flags(uint32_t *d_flags_out, const uint32_t *d_flags_a, const uint32_t *d_flags_b, hipStream_t stream)
{
    hipLaunchKernelGGL(join_flags_kernel, dim3(1), dim3(64), 0, stream, d_flags_out, d_flags_a, d_flags_b);
    return hipGetLastError();
}

hipError_t launch_unpack_cross(const float *d_slab, float *d_fs, float *d_sf, const uint32_t *d_order, uint32_t n_seq, uint32_t n0,
                               uint32_t n_first, bool swapped, const uint32_t *d_flags, uint32_t *d_status, hipStream_t stream)
{
    const uint64_t pairs = (uint64_t)n0 * (n_seq - n0);
    if (pairs == 0) return hipSuccess;
    const uint32_t tb0 = n0 / kTile, tiles_b = (n_seq + kTile - 1) / kTile - tb0;
    hipLaunchKernelGGL(unpack_cross_kernel, dim3((uint32_t)((pairs + 255) / 256)), dim3(256), 0, stream, d_slab, d_fs, d_sf, d_order, n_seq,
                       n0, n_first, swapped ? 1u : 0u, tb0, tiles_b, d_flags, d_status);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// dispatch: which kernel sweeps which tile, with which geometry (the lists of what exists: apd_internal.h)
// ------------------------------------------------------------------------------------------------

// apd_set_variant, decoded once per tile plan: 0 lets every family be searched, 1 forces the generic kernel, a geometry's code
// forces that geometry (tuning); any other code keeps the band-form search and turns the column strips off.
struct VariantRequest {
    bool automatic;   // variant 0: strips searched, small strip classes consolidated
    bool generic;     // variant 1
    KernelGeom geom;  // the forced geometry as decoded (it may name one that is not instantiated); Generic: none
    explicit VariantRequest(int variant) : automatic(variant == 0), generic(variant == 1), geom(KernelGeom::decode(variant)) {}
};

// Band form: the (lanes per pair, offsets per lane) that wastes the fewest lanes for a band of `need` offsets; Generic if none.
static KernelGeom pick_band_geom(uint32_t need, uint32_t dim, const VariantRequest &req, bool uniform_pen, bool fast_shift)
{
    if (req.generic || !is_kernel_dim(dim)) return {};
    KernelGeom f = req.geom;
    if (f.family == KernelGeom::SharedColumns) f.family = KernelGeom::Systolic;   // forced shared columns: its DPP twin here, promoted by the plan
    if (f.family == KernelGeom::Systolic || f.family == KernelGeom::Wide)   // forced; too narrow (or not instantiated): generic
        return (f.family == KernelGeom::Systolic || uniform_pen) && f.capacity() >= need && geom_instantiated(f, dim) ? f : KernelGeom{};
    // score = lanes busy x how cheap a cell is at this C.  A macro-step costs about 116 SIMD cycles (window moves, exchanges,
    // threshold test) plus 76 per cell pair, so relative to C = 9 a cell costs 1.04 / 1.11 / 1.29 / 1.50
    // at C = 7 / 5 / 3 / 2.  G = 8 and G = 32 span half / two DPP rows: one-instruction moves only in the hybrid form with unit
    // penalties (`fast_shift`: masked column fetch), two instructions or a select per move otherwise.
    auto cell_eff = [](int c) { return c >= 9 ? 1.0 : c >= 7 ? 0.96 : c >= 5 ? 0.90 : c >= 3 ? 0.78 : 0.67; };
    KernelGeom best{};
    double best_util = 0.0;
    for (KernelGeom q : kSystolicGeoms) {
        if (q.capacity() < need || !geom_instantiated(q, dim)) continue;
        const bool split_rows = q.lanes_or_waves == 8 || q.lanes_or_waves == 32;
        const double util = (double)need / (double)q.capacity() * cell_eff(q.cells) * (split_rows ? (fast_shift ? 0.99 : 0.90) : 1.0);
        if (util > best_util) { best_util = util; best = q; }
    }
    if (best.family != KernelGeom::Generic) return best;
    // beyond one wavefront: NW waves per pair (dtw_wide.h), uniform penalties only; the smallest that holds the band
    if (uniform_pen)
        for (KernelGeom q : kWideGeoms)
            if (q.capacity() >= need && geom_instantiated(q, dim)) return q;
    return {};
}

struct GeomList {
    const KernelGeom *first, *last;
    const KernelGeom *begin() const { return first; }
    const KernelGeom *end() const { return last; }
};
static GeomList strip_geoms(KernelGeom::Family family)
{
    if (family == KernelGeom::Strip) return {std::begin(kStripGeoms), std::end(kStripGeoms)};
    return {std::begin(kBandedStripGeoms), std::end(kBandedStripGeoms)};
}

// Column strips (dtw_full.h), one pair of `rows` x `cols`: with G = 64 / ppw lanes per pair it takes ceil(cols / (G CW))
// passes of rows + G macro-steps, each serving ppw pairs.  The cost of a macro-step was fitted on MI355X
// (tools/debug/strip_grid.sh: every forced geometry on bench.py's short9 / full6 / ship / full8): proportional to CW (+0.5 /
// +1.5 for the two-DPP moves and per-lane bookkeeping of 32- / 16-lane groups), 8 % more once CW frames of D + 1 floats push
// the kernel to two waves per SIMD, and inversely to the wavefronts per CU that the LDS boundary columns (ppw * rows floats
// per wavefront) leave room for.  +inf for a geometry that is not instantiated or does not fit.
static double strip_cost(uint32_t cols, uint32_t rows, uint32_t dim, KernelGeom key)
{
    const bool banded = key.family == KernelGeom::BandedStrip;
    if ((key.family != KernelGeom::Strip && !banded) || !geom_instantiated(key, dim)) return INFINITY;
    const int ppw = key.lanes_or_waves, cw = key.cells;
    const uint32_t g = 64u / ppw;
    const double lds_bytes = (double)strip_lds_bytes(dim, ppw, banded, rows);
    if (lds_bytes > 160.0 * 1024) return INFINITY;
    const double waves_per_cu = std::floor(160.0 * 1024 / lds_bytes);
    const double lds_factor = waves_per_cu >= 8.0 ? 1.0 : 8.0 / waves_per_cu;
    const double group_steps = ppw == 1 ? 0.0 : (ppw == 2 ? 0.5 : 1.5);
    const double occupancy_factor = (uint32_t)cw * (dim + 3) > 150 ? 1.08 : 1.0;
    const double passes = (double)((cols + g * cw - 1) / (g * cw));
    return passes * ((double)rows + g) * (cw + group_steps) * occupancy_factor * lds_factor / ppw;
}

// The cheapest strip geometry of `family` for pairs of at most `rows` x `cols` frames; Generic if none applies.
static KernelGeom pick_strip_geom(uint32_t cols, uint32_t rows, uint32_t dim, const VariantRequest &req, KernelGeom::Family family)
{
    if (!is_kernel_dim(dim)) return {};
    if (!req.automatic) return req.geom.family == family && std::isfinite(strip_cost(cols, rows, dim, req.geom)) ? req.geom : KernelGeom{};
    KernelGeom best{};
    double best_cost = INFINITY;
    for (KernelGeom g : strip_geoms(family)) {
        if (g.cells < 5) continue;                                     // 3-column strips only on request: measured slower than the model says
        const double cost = strip_cost(cols, rows, dim, g);
        if (cost < best_cost) { best = g; best_cost = cost; }
    }
    return best;
}

// Which kernel sweeps which tile.  Tiles are grouped by the kernel geometry their widest pair needs (w is bounded per tile
// from the lengths of its 32 sequences), one launch per group: a few long or unequal sequences do not force every pair
// onto a wide kernel.
void plan_tile_classes(const std::vector<uint64_t> &offsets, uint32_t n_seq, const std::vector<uint2> &tiles, const BandSpec &band,
                       uint32_t dim, int variant, bool fast_ok, bool uniform_pen, bool fast_shift, std::vector<TileClass> &classes,
                       std::vector<uint4> &flat)
{
    const VariantRequest req(variant);
    // per tile-row (16 sequences) min / max length
    const uint32_t side = (n_seq + kTile - 1) / kTile;
    std::vector<uint32_t> lo(side, 0xFFFFFFFFu), hi(side, 0);
    for (uint32_t s = 0; s < n_seq; ++s) {
        const uint32_t len = (uint32_t)(offsets[s + 1] - offsets[s]);
        lo[s / kTile] = std::min(lo[s / kTile], len);
        hi[s / kTile] = std::max(hi[s / kTile], len);
    }
    struct Group { std::vector<uint4> tiles; uint32_t w_max = 0, n_max = 0; };
    std::map<KernelGeom, Group> groups;
    // Shared column rings (dtw_systolic.h): the hybrid form with unit penalties (`fast_shift`), for the tiles whose workgroups
    // sweep bands of nearly one width.  A forced systolic code keeps naming the DPP window; a forced shared-column code takes
    // the tiles that qualify and leaves the others to its DPP twin.
    const bool shared_ok = fast_shift && req.geom.family != KernelGeom::Systolic;
    std::vector<uint32_t> lens;
    if (shared_ok) {
        lens.resize(n_seq);
        for (uint32_t s = 0; s < n_seq; ++s) lens[s] = (uint32_t)(offsets[s + 1] - offsets[s]);
    }
    for (uint32_t t = 0; t < tiles.size(); ++t) {
        const uint32_t mx = std::max(hi[tiles[t].x], hi[tiles[t].y]), mn = std::min(lo[tiles[t].x], lo[tiles[t].y]);
        const uint32_t band_ub = band.use_explicit ? band.explicit_band : host_band_from_pct(band.pct, mx);
        const uint32_t w = std::max(std::min(band_ub, mx), mx - mn) + 2;   // >= w of every pair of the tile
        KernelGeom key = fast_ok ? pick_band_geom(2 * w + 1, dim, req, uniform_pen, fast_shift) : KernelGeom{};
        if (shared_ok && key.family == KernelGeom::Systolic) {
            const KernelGeom shared{KernelGeom::SharedColumns, key.lanes_or_waves, key.cells};
            // every pair of the tile has its w between these bounds: within the slack, no need to look at the pairs
            const uint32_t lx = lo[tiles[t].x], ly = lo[tiles[t].y], hx = hi[tiles[t].x], hy = hi[tiles[t].y];
            const uint32_t mx_lo = std::max(lx, ly), gap_lo = lx > hy ? lx - hy : ly > hx ? ly - hx : 0u;
            const uint32_t band_lb = band.use_explicit ? band.explicit_band : host_band_from_pct(band.pct, mx_lo);
            const uint32_t w_lb = std::max(std::min(band_lb, mx_lo), gap_lo) + 2;
            const uint32_t slack = shared_column_slack(shared);
            if (geom_instantiated(shared, dim) && (w - w_lb <= slack || shared_columns_qualify(lens, tiles[t].x, tiles[t].y, band, slack)))
                key = shared;
        }
        // the band binds nowhere in this tile (band >= longest - 3 for its longest sequence, hence for all) and the penalties
        // are equal: both ordered scores are one number, swept over column strips (dtw_full.h).  Not for very short columns,
        // where four pairs per wavefront in band form keep more lanes busy.
        const uint32_t cols = std::min(hi[tiles[t].x], hi[tiles[t].y]);
        const bool never_binds = mx >= 3 && std::min(band_ub, mx) >= mx - 3;
        if (fast_ok && uniform_pen && never_binds && (cols >= 49 || req.geom.family == KernelGeom::Strip)) {
            const KernelGeom fk = pick_strip_geom(cols > 0 ? cols - 1 : 0, mx, dim, req, KernelGeom::Strip);
            if (fk.family != KernelGeom::Generic) key = fk;
        } else if (fast_ok && mx >= 3 && cols >= 49 &&                          // (any penalties: unequal ones take the literal select)
                   (2ull * w + 1 >= cols ||                                   // band at least as wide as the short side
                    key.family == KernelGeom::Generic ||                      // no band-form kernel fits: anything beats the generic one
                    req.geom.family == KernelGeom::BandedStrip)) {
            // the band binds, but is wider than the short side of the tile's pairs (w grows with |n - m|, alignments.rs:173):
            // in band coordinates most offsets of such a pair lie outside it; column strips with masked band edges fit
            const KernelGeom bk = pick_strip_geom(cols - 1, mx, dim, req, KernelGeom::BandedStrip);
            if (bk.family != KernelGeom::Generic) key = bk;
        }
        Group &g = groups[key];
        g.tiles.push_back(make_uint4(tiles[t].x, tiles[t].y, t, 0));
        g.w_max = std::max(g.w_max, w);
        g.n_max = std::max(g.n_max, mx);
    }
    // Every class is a launch of its own, and launches of one stream do not overlap: a full-matrix class of a few dozen
    // tiles would run at a fraction of the machine.  Small classes (all of them, in a small batch) move to the geometry
    // that is best for the full-matrix tiles as a whole.
    if (req.automatic) {
        for (KernelGeom::Family family : {KernelGeom::Strip, KernelGeom::BandedStrip}) {   // one DP (band never binds) / two DPs (banded)
            size_t n_fam = 0;
            for (auto &g : groups) if (g.first.family == family) n_fam += g.second.tiles.size();
            if (n_fam == 0) continue;
            const int max_ppw = n_fam * kSlotsPerTile < 8192 ? 1 : 4;    // too few pairs to fill the GPU: one wavefront each
            KernelGeom global{};
            double global_cost = INFINITY;
            for (KernelGeom k : strip_geoms(family)) {
                if (k.cells < 5 || k.lanes_or_waves > max_ppw) continue;
                double total = 0.0;
                for (auto &g : groups) {
                    if (g.first.family != family) continue;
                    for (const uint4 &t : g.second.tiles) {
                        const uint32_t c = std::min(hi[t.x], hi[t.y]);
                        total += strip_cost(c > 0 ? c - 1 : 0, std::max(hi[t.x], hi[t.y]), dim, k);
                    }
                }
                if (total < global_cost) { global_cost = total; global = k; }
            }
            const size_t min_class = n_fam < 2048 ? n_fam + 1 : 256;
            if (global.family == KernelGeom::Generic) continue;
            std::vector<KernelGeom> small;
            for (auto &g : groups) if (g.first.family == family && !(g.first == global) && g.second.tiles.size() < min_class) small.push_back(g.first);
            for (KernelGeom k : small) {
                Group &from = groups[k], &to = groups[global];
                to.tiles.insert(to.tiles.end(), from.tiles.begin(), from.tiles.end());
                to.w_max = std::max(to.w_max, from.w_max);
                to.n_max = std::max(to.n_max, from.n_max);
                groups.erase(k);
            }
            std::vector<uint4> &merged = groups[global].tiles;
            std::sort(merged.begin(), merged.end(), [](const uint4 &a, const uint4 &b) { return a.z < b.z; });
        }
    }
    classes.clear();
    flat.clear();
    for (auto &g : groups) {
        classes.push_back(TileClass{g.first, (uint32_t)flat.size(), (uint32_t)g.second.tiles.size(), g.second.w_max, g.second.n_max});
        flat.insert(flat.end(), g.second.tiles.begin(), g.second.tiles.end());
    }
}

// the generic kernel's LDS: two DP rows of c_max cells per lane
static size_t generic_lds_bytes(uint32_t w_max, int *c_max_out)
{
    int c_max = (int)((2 * (uint64_t)w_max + 1 + 63) / 64);
    if (c_max < 2) c_max = 2;
    if (c_max_out) *c_max_out = c_max;
    return (size_t)c_max * 64 * 2 * sizeof(float);
}

static hipError_t launch_align_chunk(const AlignLaunch &L, KernelGeom g, hipStream_t stream, std::string &err, int *status)
{
    if (L.n_tiles == 0) return hipSuccess;
    if (g.family == KernelGeom::Generic) {
        int c_max = 2;
        const size_t lds_bytes = generic_lds_bytes(L.w_max, &c_max);
        if (lds_bytes > 160 * 1024) { *status = APD_ERR_BAND_TOO_WIDE; err = "band too wide for the generic kernel"; return hipSuccess; }
        if (lds_bytes > 64 * 1024) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(dtw_fused_generic),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
            if (e != hipSuccess) return e;
        }
        const uint64_t waves = (uint64_t)L.n_tiles * kSlotsPerTile;
        hipLaunchKernelGGL(dtw_fused_generic, dim3((uint32_t)waves), dim3(64), lds_bytes, stream, L, c_max);
        return hipGetLastError();
    }
    hipError_t e = hipSuccess;
    bool found = false;
    with_kernel_dim(L.dim, [&](auto d) {
        constexpr int D = decltype(d)::value;
        found = g.family == KernelGeom::Systolic || g.family == KernelGeom::SharedColumns ? launch_systolic<D>(L, g, stream)
              : g.family == KernelGeom::Wide     ? launch_wide<D>(L, g, stream, &e)
                                                 : launch_full<D>(L, g, stream, &e);
    });
    if (!found) {                                                      // the plan only names listed geometries
        *status = APD_ERR_UNSUPPORTED;
        err = "no kernel for geometry " + std::to_string(g.encode()) + " at dimension " + std::to_string(L.dim);
        return hipSuccess;
    }
    return e != hipSuccess ? e : hipGetLastError();
}

// A launch may not exceed 2^32 work-items (beyond, the grid is silently cut short on this runtime): launches are cut
// into runs of tiles that stay below 2^31.  Work-items per tile: 256 pairs x lanes per pair.
hipError_t launch_align(const AlignLaunch &L, KernelGeom g, hipStream_t stream, std::string &err, int *status)
{
    *status = APD_OK;
    const uint32_t kTilesPerLaunch = (1u << 31) / (kSlotsPerTile * std::max(g.lanes_per_pair(), 64u));
    // The distance form (the kernels never read L.hybrid; their launchers pick the instantiation by it).  The norm expansion
    // trades D - 1 vector ops per cell (systolic kernel, pre-scaled rows; D - 4 in the strip kernels) for a branch per
    // macro-step: measured worth it from D = 8 in the systolic kernel (cfg 4: -2.6 %), from D = 10 in the wide and strip
    // kernels, which have it with unit penalties only.  Strict mode keeps the systolic kernel's UNIFORM_PEN path with unit
    // penalties (its fast select on the difference form is the reference's arithmetic operation for operation, see
    // dtw_systolic.h) and switches only the hybrid form off.
    AlignLaunch part = L;
    part.hybrid = L.hybrid && (g.family == KernelGeom::Systolic || g.family == KernelGeom::SharedColumns ? L.dim >= 8 && !L.strict : L.dim >= 10 && L.band.mat == 1.0f);
    for (uint32_t first = 0; first < L.n_tiles; first += kTilesPerLaunch) {
        part.d_tiles = L.d_tiles + first;
        part.n_tiles = std::min(kTilesPerLaunch, L.n_tiles - first);
        const hipError_t e = launch_align_chunk(part, g, stream, err, status);
        if (e != hipSuccess || *status != APD_OK) return e;
    }
    return hipSuccess;
}

bool generic_band_fits(uint32_t w_max) { return generic_lds_bytes(w_max, nullptr) <= 160 * 1024; }

bool generic_fallback_fits(uint32_t w_max)
{
    const size_t lds_bytes = generic_lds_bytes(w_max, nullptr);
    if (lds_bytes > 160 * 1024) return false;                             // gfx950: 160 KB of LDS per workgroup
    if (lds_bytes > 64 * 1024 &&                                          // beyond the default limit: ask now, not after the fast kernels are enqueued
        hipFuncSetAttribute(reinterpret_cast<const void *>(dtw_fused_generic_fallback), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds_bytes) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return true;
}

hipError_t launch_generic_fallback(const AlignLaunch &L, hipStream_t stream, bool *fits)
{
    *fits = true;
    if (L.n_tiles == 0 || L.d_nonfinite == nullptr) return hipSuccess;
    int c_max = 2;
    const size_t lds_bytes = generic_lds_bytes(L.w_max, &c_max);
    if (lds_bytes > 160 * 1024) { *fits = false; return hipSuccess; }
    if (lds_bytes > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(dtw_fused_generic_fallback),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e != hipSuccess) return e;
    }
    const uint64_t waves = (uint64_t)L.n_tiles * kSlotsPerTile;
    if (waves > 0xFFFFFFFFull) { *fits = false; return hipSuccess; }
    const uint32_t grid = (uint32_t)std::min<uint64_t>(waves, 256u * 32u);   // 32 single-wave workgroups per CU when it has to work
    hipLaunchKernelGGL(dtw_fused_generic_fallback, dim3(grid), dim3(64), lds_bytes, stream, L, c_max, (uint32_t)waves);
    return hipGetLastError();
}

}  // namespace apd
