// Spot score quantiles (gfx950): apd_spot_quantiles.  numerics.rs:125-133 over the scores of whole groups of spotting curves -- per
// pair, per query, or all of a list -- done where the curves already are.  The sweep is spot_kernel<SpotSweep, RT, D> (dtw_spot.hip),
// launched by the host exactly as apd_spot launches it with curves on; the kernels here read its curves and never touch the table
// (include/apd.h, "spot score quantiles").
//
// An 8-bit radix select over spot_score_key, most significant digit first: four passes, two kernels each, all on the call's stream
// with no visit of the host between them.
//   spot_quantile_pass   grid (pairs of the chunk, column blocks): the score (spot_score, the sweep's own: one IEEE division) and its
//                        key of every column, coalesced over the pair's two curves.  Per requested quantile a 257-bin histogram in
//                        LDS of the digit of this pass, over the columns whose key matches the quantile's prefix so far (bin 256:
//                        NaN, counted in pass 0 only).  At the end the non-zero bins are added to the histogram of the pair's GROUP,
//                        one 64-bit atomicAdd each.
//   spot_quantile_step   one wavefront per (group, quantile): a prefix sum over the 256 bins finds the digit that holds the rank,
//                        the state record takes the digit and the rank left inside it, the histogram is cleared for the next pass.
//                        Pass 0 also compares the rank with the non-NaN count (beyond it: APD_ERR_INDEX, NaN); pass 3 decodes the key.
// Inside a launch nothing goes from one workgroup to another but those integer adds, and they are read by the next launch only: no
// fence, no last arriver, no waiting.  Integer counts make every histogram, and so the value, independent of scheduling.
//
// Two sources of contention, both kept off the atomics:
//   * scores of one detector share their exponent, so in pass 0 nearly every lane of a wavefront has the same digit: the digit of
//     the first counted lane is added once per wavefront (a ballot and one LDS add, as vat_select_kernel), the others one by one;
//   * the groups of APD_QUANTILES_ALL and _PER_QUERY receive the flushes of all their pairs' workgroups: a pair gets a bounded number
//     of workgroups (spot_quantile_blocks), each walking its columns with a grid stride, so a group sees a few thousand flushes of
//     at most 257 adds per pass, not one per kSpotQuantileColumns columns.
// Quantiles that share their prefix (all of them in pass 0) share one LDS histogram: the later one is flushed from the earlier one's.
#include <cstdio>
#include <cstdlib>

#include "dtw_spot_curves.h"

namespace apd {

static_assert(kSpotQuantileColumns == APD_SPOT_QUANTILES_COLUMNS, "include/apd.h tells the tests the columns of a workgroup step");

namespace {

constexpr uint32_t kBins = kSpotQuantileBins;
constexpr uint32_t kMaxQ = APD_SPOT_QUANTILES_MAX;

// grid and walk: spot_curve_walk (dtw_spot_curves.h), kSpotQuantileColumns columns a step
__global__ __launch_bounds__(kSpotQuantileColumns) void spot_quantile_pass(const SpotQuantileLaunch L, const int pass)
{
    __shared__ uint32_t hist[kMaxQ][kBins];
    __shared__ uint32_t s_prefix[kMaxQ], s_mask[kMaxQ], s_rep[kMaxQ];   // s_rep[q]: the quantile whose histogram q reads; kMaxQ: q is settled
    const SpotCurve P = L.d_pairs[blockIdx.x];
    const uint32_t nq = L.n_perc, tid = threadIdx.x, lane = tid & 63u;
    const int shift = 24 - 8 * pass;
    for (uint32_t h = tid; h < nq * kBins; h += kSpotQuantileColumns) (&hist[0][0])[h] = 0;
    if (tid == 0) {
        for (uint32_t q = 0; q < nq; ++q) {
            const SpotQuantileState st = L.d_state[(uint64_t)P.group * nq + q];
            s_prefix[q] = st.prefix; s_mask[q] = st.mask;
            uint32_t rep = st.verdict != 0 ? kMaxQ : q;
            for (uint32_t e = 0; e < q && rep == q; ++e)
                if (s_rep[e] == e && s_prefix[e] == st.prefix) rep = e;   // the mask is the pass's, the same for all
            s_rep[q] = rep;
        }
    }
    __syncthreads();
    spot_curve_walk<kSpotQuantileColumns>(P, L.d_cost, L.d_start, [&](uint64_t, bool live, float, uint32_t, float score) {
        const bool is_nan = score != score;
        const uint32_t key = spot_score_key(score);
        const uint32_t d = is_nan ? 256u : (key >> shift) & 0xFFu;
        for (uint32_t q = 0; q < nq; ++q) {
            if (s_rep[q] != q) continue;                                   // uniform: settled, or counted with an earlier quantile
            const bool want = live && (is_nan ? pass == 0 : (key & s_mask[q]) == s_prefix[q]);
            const unsigned long long vote = __ballot(want);
            if (vote == 0) continue;
            const int leader = __ffsll((long long)vote) - 1;
            const uint32_t ld = (uint32_t)__shfl((int)d, leader, 64);
            const unsigned long long same = __ballot(want && d == ld);
            if ((int)lane == leader) atomicAdd(&hist[q][ld], (uint32_t)__popcll(same));
            else if (want && d != ld) atomicAdd(&hist[q][d], 1u);
        }
    });
    __syncthreads();
    for (uint32_t q = 0; q < nq; ++q) {
        const uint32_t rep = s_rep[q];
        if (rep == kMaxQ) continue;
        unsigned long long *out = L.d_hist + ((uint64_t)P.group * nq + q) * kBins;
        for (uint32_t b = tid; b < kBins; b += kSpotQuantileColumns) {
            const uint32_t c = hist[rep][b];
            if (c) atomicAdd(out + b, (unsigned long long)c);
        }
    }
}

// grid: (groups of the chunk) x (quantiles), one wavefront each; lane l owns bins 4 l .. 4 l + 3
__global__ __launch_bounds__(64) void spot_quantile_step(const SpotQuantileLaunch L, const int pass)
{
    const uint64_t gq = blockIdx.x;
    const uint32_t lane = threadIdx.x;
    unsigned long long *h = L.d_hist + gq * kBins;
    unsigned long long c[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { c[i] = h[4 * lane + i]; h[4 * lane + i] = 0; }
    const unsigned long long nans = h[256];                               // pass 0 only: zero afterwards
    SpotQuantileState st = L.d_state[gq];
    if (st.verdict != 0) return;                                          // settled in pass 0: nothing was added since
    if (lane == 0) h[256] = 0;
    const int shift = 24 - 8 * pass;
    const unsigned long long mine = c[0] + c[1] + c[2] + c[3];
    unsigned long long incl = mine;
#pragma unroll
    for (uint32_t delta = 1; delta < 64; delta <<= 1) {
        const unsigned long long up = shfl_up_u64(incl, delta);
        if (lane >= delta) incl += up;
    }
    const unsigned long long before = incl - mine;
    // the lane whose four bins hold the rank; none: the rank lies beyond the counted keys (pass 0: k >= entries - nans, numerics.rs:132)
    const bool owner = st.rank >= before && st.rank - before < mine;
    if (pass == 0 && lane == 0 && gq % L.n_perc == 0 && L.d_nans) L.d_nans[gq / L.n_perc] = nans;
    if (__ballot(owner) == 0) {
        if (lane == 0) {
            st.verdict = APD_ERR_INDEX;
            L.d_state[gq] = st;
            L.d_values[gq] = __builtin_nanf("");
            L.d_status[gq] = APD_ERR_INDEX;
        }
        return;
    }
    if (!owner) return;
    unsigned long long rank = st.rank - before;
    uint32_t d = 4 * lane;
#pragma unroll
    for (int i = 0; i < 3; ++i)
        if (d == 4 * lane + i && rank >= c[i]) { rank -= c[i]; ++d; }
    st.prefix |= d << shift;
    st.mask |= 0xFFu << shift;
    st.rank = rank;
    L.d_state[gq] = st;
    if (pass == 3) {
        const uint32_t u = (st.prefix & 0x80000000u) ? (st.prefix & 0x7FFFFFFFu) : ~st.prefix;   // invert spot_score_key
        L.d_values[gq] = __uint_as_float(u);
        L.d_status[gq] = APD_OK;
    }
}

}  // namespace

// Column blocks per pair: enough workgroups to fill the chip when the pairs alone do not, no more than a pair's columns need.
// kSpotQuantileWorkgroups is the measured bound; APD_SPOT_QUANTILE_WORKGROUPS overrides it (measurements
// and tests only: the values do not depend on it).
uint32_t spot_quantile_blocks(uint32_t n_pairs, uint32_t m_max)
{
    uint64_t target = kSpotQuantileWorkgroups;
    if (const char *v = std::getenv("APD_SPOT_QUANTILE_WORKGROUPS")) {
        const unsigned long long t = std::strtoull(v, nullptr, 10);
        if (t > 0) target = t;
    }
    const uint64_t need = ((uint64_t)m_max + kSpotQuantileColumns - 1) / kSpotQuantileColumns;
    const uint64_t share = (target + n_pairs - 1) / (n_pairs ? n_pairs : 1);
    const uint64_t by = need < share ? need : share;
    return (uint32_t)(by < 1 ? 1 : by > 65535 ? 65535 : by);
}

hipError_t launch_spot_quantiles(const SpotQuantileLaunch &L, uint32_t m_max, hipStream_t stream)
{
    if (L.n_pairs == 0 || L.n_groups == 0 || L.n_perc == 0) return hipSuccess;
    const uint32_t by = spot_quantile_blocks(L.n_pairs, m_max);
    if (std::getenv("APD_DEBUG_PLAN"))
        std::fprintf(stderr, "[apd] spot quantile select: %u pairs, %u groups x %u quantiles, %u column blocks of %u columns per pair\n",
                     L.n_pairs, L.n_groups, L.n_perc, by, kSpotQuantileColumns);
    for (int pass = 0; pass < 4; ++pass) {
        hipLaunchKernelGGL(spot_quantile_pass, dim3(L.n_pairs, by), dim3(kSpotQuantileColumns), 0, stream, L, pass);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
        hipLaunchKernelGGL(spot_quantile_step, dim3(L.n_groups * L.n_perc), dim3(64), 0, stream, L, pass);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace apd
