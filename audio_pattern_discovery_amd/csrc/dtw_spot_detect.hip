// Spot detection (gfx950): apd_spot_detect.  What stands between the curves of apd_spot and the windows a caller wants -- score every
// column, keep those below the pair's threshold, pick non-overlapping windows greedily in ascending (score, end, pair) -- done where
// the curves already are.  The sweep is spot_kernel<SpotSweep, RT, D> (dtw_spot.hip), launched by the host exactly as apd_spot
// launches it with curves on; the kernels here read its curves and never touch the table (include/apd.h, "spot detection").
//
// Four kernels on the call's stream, per chunk of whole groups:
//   spot_detect_mark     over the chunk's curve entries, coalesced: the score (spot_score, the sweep's own: one IEEE division), the
//                        threshold test, and for every candidate a 16-byte key in its GROUP's list.  A wavefront compacts with one
//                        ballot and one atomic on the group's counter; the order of a list therefore depends on scheduling, and
//                        nothing downstream reads it: every choice below is a minimum over the full key.
//   spot_detect_pick     one workgroup per group: rounds of "smallest live key of the list, accept it, kill what overlaps it".  The
//                        kill of round r rides on the scan of round r + 1, so a hit costs one pass over the list.
//   spot_detect_offsets  one workgroup: the exclusive prefix of the groups' hit counts.
//   spot_detect_emit     after the host has sized the packed buffer: the apd_spot_hit records, group-major, acceptance order inside.
//
// The key.  hi = spot_score_key(score) << 32 | end, lo = pair << 32 | start, compared (hi, lo): ascending score by f32 <, then the
// smaller end, then the smaller pair (a group holds one candidate per (pair, end), so `start` below the pair never decides).
// spot_score_key() (apd_internal.h): the sign bit flipped for a non-negative score, every bit for a negative one -- the usual monotone
// map of f32 onto u32 -- after both zeros were made +0.0, so that -0.0 and +0.0 tie as f32 < says they do.  A candidate's score is
// below its threshold and so below +INF: its key is below 0xFF800000, and hi = 2^64 - 1 is free to mean "dead".  The record's score
// is computed again from the curves at emit (spot_score again: the same bits, and the sign of a zero survives).
#include "dtw_spot_curves.h"

namespace apd {

namespace {

constexpr unsigned long long kDead = ~0ull;
constexpr int kPickThreads = 1024;             // 16 wavefronts per group
constexpr int kMarkThreads = 256;

__device__ __forceinline__ bool key_less(unsigned long long ah, unsigned long long al, unsigned long long bh, unsigned long long bl)
{
    return ah < bh || (ah == bh && al < bl);
}

// grid and walk: spot_curve_walk (dtw_spot_curves.h), kMarkThreads columns a step
__global__ __launch_bounds__(kMarkThreads) void spot_detect_mark(const SpotDetectLaunch L)
{
    const uint32_t p = blockIdx.x;
    const SpotDetectPair P = L.d_pairs[p];
    const SpotDetectGroup G = L.d_groups[P.curve.group];
    ulonglong2 *list = L.d_cand + G.cand_off;
    unsigned long long *counter = L.d_cand_count + P.curve.group;
    const uint32_t lane = threadIdx.x & 63u;
    spot_curve_walk<kMarkThreads>(P.curve, L.d_cost, L.d_start, [&](uint64_t j, bool live, float, uint32_t s, float score) {
        const bool cand = live && s != 0u && score < P.threshold;         // strict; a NaN on either side compares false
        const unsigned long long vote = __ballot(cand);
        if (vote == 0) return;
        const int leader = __ffsll((long long)vote) - 1;
        unsigned long long base = 0;
        if ((int)lane == leader) base = atomicAdd(counter, (unsigned long long)__popcll(vote));
        base = shfl_u64(base, leader);
        if (cand) {
            const uint64_t slot = base + (uint64_t)__popcll(vote & ((1ull << lane) - 1ull));
            ulonglong2 k;
            k.x = ((unsigned long long)spot_score_key(score) << 32) | (uint32_t)(j + 1u);
            k.y = ((unsigned long long)p << 32) | s;
            if (slot < G.cand_cap) list[slot] = k;                        // one candidate per entry at most: always true
        }
    });
}

// grid: the chunk's groups
__global__ __launch_bounds__(kPickThreads) void spot_detect_pick(const SpotDetectLaunch L)
{
    __shared__ unsigned long long red_hi[kPickThreads / 64], red_lo[kPickThreads / 64];
    __shared__ unsigned long long win_hi, win_lo;
    const uint32_t g = blockIdx.x;
    const SpotDetectGroup G = L.d_groups[g];
    ulonglong2 *list = L.d_cand + G.cand_off;
    uint2 *stage = L.d_stage + G.stage_off;
    unsigned long long count = L.d_cand_count[g];
    if (count > G.cand_cap) count = G.cand_cap;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    bool have = false;
    uint32_t w_end = 0, w_start = 0, rank = 0;
    for (;;) {
        unsigned long long bh = kDead, bl = kDead;
        for (unsigned long long i = tid; i < count; i += kPickThreads) {
            const ulonglong2 k = list[i];
            if (k.x == kDead) continue;
            const uint32_t end = (uint32_t)k.x, st = (uint32_t)k.y;
            if (have && st <= w_end && w_start <= end) {                  // shares a column with the window just accepted (itself too)
                list[i].x = kDead;
                continue;
            }
            if (key_less(k.x, k.y, bh, bl)) { bh = k.x; bl = k.y; }
        }
#pragma unroll
        for (int mask = 32; mask >= 1; mask >>= 1) {
            const unsigned long long oh = shfl_xor_u64(bh, mask), ol = shfl_xor_u64(bl, mask);
            if (key_less(oh, ol, bh, bl)) { bh = oh; bl = ol; }
        }
        if (lane == 0) { red_hi[wave] = bh; red_lo[wave] = bl; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < kPickThreads / 64; ++w)
                if (key_less(red_hi[w], red_lo[w], bh, bl)) { bh = red_hi[w]; bl = red_lo[w]; }
            win_hi = bh; win_lo = bl;
            if (bh != kDead && rank < G.stage_cap) stage[rank] = make_uint2((uint32_t)(bl >> 32), (uint32_t)bh);   // (pair, end)
        }
        __syncthreads();
        bh = win_hi; bl = win_lo;
        if (bh == kDead) break;
        have = true;
        w_end = (uint32_t)bh; w_start = (uint32_t)bl;
        ++rank;
    }
    if (tid == 0) L.d_hit_count[g] = rank < G.stage_cap ? rank : G.stage_cap;
}

// one workgroup: d_hit_base[g] = hits of the chunk's groups before g, d_hit_base[n_groups] = all of them
__global__ __launch_bounds__(1024) void spot_detect_offsets(const SpotDetectLaunch L)
{
    __shared__ unsigned long long part[1024];
    const uint32_t tid = threadIdx.x, n = L.n_groups;
    const uint32_t per = (n + 1023u) / 1024u;
    const uint64_t lo = (uint64_t)tid * per, hi = lo + per < n ? lo + per : n;
    unsigned long long sum = 0;
    for (uint64_t g = lo; g < hi; ++g) sum += L.d_hit_count[g];
    part[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        unsigned long long run = 0;
        for (int t = 0; t < 1024; ++t) { const unsigned long long v = part[t]; part[t] = run; run += v; }
        L.d_hit_base[n] = run;
    }
    __syncthreads();
    unsigned long long run = part[tid];
    for (uint64_t g = lo; g < hi; ++g) { L.d_hit_base[g] = run; run += L.d_hit_count[g]; }
}

// grid: the chunk's groups, one wavefront each; d_hits holds the chunk's first n_write hits
__global__ __launch_bounds__(64) void spot_detect_emit(const SpotDetectLaunch L, apd_spot_hit *d_hits, uint64_t n_write)
{
    const uint32_t g = blockIdx.x;
    const SpotDetectGroup G = L.d_groups[g];
    const uint2 *stage = L.d_stage + G.stage_off;
    const uint32_t count = L.d_hit_count[g];
    const unsigned long long base = L.d_hit_base[g];
    for (uint32_t r = threadIdx.x; r < count; r += 64u) {
        const unsigned long long at = base + r;
        if (at >= n_write) break;
        const uint2 w = stage[r];                                         // (pair of the chunk, end)
        const SpotCurve P = L.d_pairs[w.x].curve;
        apd_spot_hit h;
        h.pair = P.pair;
        h.end = w.y;
        h.start = L.d_start[P.curve_off + w.y - 1u];
        h.cost = L.d_cost[P.curve_off + w.y - 1u];
        h.score = spot_score(h.cost, h.end, h.start, P.n);
        h.rank = r;
        d_hits[at] = h;
    }
}

}  // namespace

hipError_t launch_spot_detect(const SpotDetectLaunch &L, uint32_t m_max, hipStream_t stream)
{
    if (L.n_pairs == 0 || L.n_groups == 0) return hipSuccess;
    const uint64_t blocks = ((uint64_t)m_max + kMarkThreads - 1) / kMarkThreads;
    const uint32_t by = (uint32_t)(blocks < 1 ? 1 : blocks > 65535 ? 65535 : blocks);
    hipLaunchKernelGGL(spot_detect_mark, dim3(L.n_pairs, by), dim3(kMarkThreads), 0, stream, L);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(spot_detect_pick, dim3(L.n_groups), dim3(kPickThreads), 0, stream, L);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(spot_detect_offsets, dim3(1), dim3(1024), 0, stream, L);
    return hipGetLastError();
}

hipError_t launch_spot_detect_emit(const SpotDetectLaunch &L, apd_spot_hit *d_hits, uint64_t n_write, hipStream_t stream)
{
    if (L.n_groups == 0 || n_write == 0) return hipSuccess;
    hipLaunchKernelGGL(spot_detect_emit, dim3(L.n_groups), dim3(64), 0, stream, L, d_hits, n_write);
    return hipGetLastError();
}

}  // namespace apd
