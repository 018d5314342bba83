// Subsequence alignment ("spotting", gfx950): apd_spot.  A query x of n frames against every window of a stream y of m frames in ONE
// DP: the recurrence of alignments.rs:153-159 with a free start (row 0 of the table is 0 in every column, column 0 is +INF below
// it), no band, and the column in which each cell's alignment left row 0 carried along with the value.  The results are the last
// row's value and start per stream column (include/apd.h, "subsequence alignment").
//
// The reference has no spotting, so nothing of it is mirrored beyond the recurrence and the arithmetic -- in particular NOT its habit
// of reading the score one row and one column short, at (n-1, m-1) (alignments.rs:120): the curves are row n's, or a one-frame query
// would have no row at all.
//
// The sweep itself -- lane mapping, macro-step, arithmetic -- is spot_sweep (dtw_spot_sweep.h), which apd_spot_paths' recording
// sweep shares; here it runs with REC = false: the lane that owns row n stores the curves (when the caller asked for them) and keeps
// the running best -- the scan over j is serial there already, no atomics, no reduction.
#include <cstdio>
#include <cstdlib>

#include "dtw_spot_sweep.h"

namespace apd {

template <int RT, int D>
__global__ __launch_bounds__(64) void dtw_spot(const SpotLaunch L)
{
    const SpotPair P = L.d_pairs[blockIdx.x];
    spot_sweep<RT, D, false>(L, P, SpotRecord{});
}

size_t spot_lds_bytes(uint32_t rows_per_lane) { return (size_t)rows_per_lane * 64 * (sizeof(float) + sizeof(uint32_t)); }

void spot_debug_line(const char *kind, int rt, int d, uint32_t n_pairs, uint32_t r_max, size_t lds_bytes)
{
    if (!std::getenv("APD_DEBUG_PLAN")) return;
    if (rt > 0)
        std::fprintf(stderr, "[apd] spot %s kernel <%d, %d>: %u pairs\n", kind, rt, d, n_pairs);
    else
        std::fprintf(stderr, "[apd] spot %s kernel <0, %d>: %u pairs, r_max %u, lds %zu bytes\n", kind, d, n_pairs, r_max, lds_bytes);
}

namespace {

template <int RT, int D>
hipError_t launch_spot_as(const SpotLaunch &L, uint32_t r_max, hipStream_t stream)
{
    const size_t lds_bytes = RT > 0 ? 0 : spot_lds_bytes(r_max);
    spot_debug_line("sweep", RT, D, L.n_pairs, r_max, lds_bytes);
    if (lds_bytes > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(dtw_spot<RT, D>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)lds_bytes);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((dtw_spot<RT, D>), dim3(L.n_pairs), dim3(64), lds_bytes, stream, L);
    return hipGetLastError();
}

template <int D>
hipError_t launch_spot_rows(const SpotLaunch &L, uint32_t rt, uint32_t r_max, hipStream_t stream)
{
    switch (rt) {
        case 1: return launch_spot_as<1, D>(L, r_max, stream);
        case 2: return launch_spot_as<2, D>(L, r_max, stream);
        case 3: return launch_spot_as<3, D>(L, r_max, stream);
        case 4: return launch_spot_as<4, D>(L, r_max, stream);
        default: return launch_spot_as<0, D>(L, r_max, stream);
    }
}

}  // namespace

// The pairs of L all belong to one class (spot_row_class): rt = 1 .. 4 rows per lane in registers, or 0 with at most r_max rows in LDS.
hipError_t launch_spot(const SpotLaunch &L, uint32_t rt, uint32_t r_max, hipStream_t stream)
{
    if (L.n_pairs == 0) return hipSuccess;
    hipError_t e = hipSuccess;
    const bool typed = with_kernel_dim(L.dim, [&](auto d) { e = launch_spot_rows<decltype(d)::value>(L, rt, r_max, stream); });
    if (!typed) e = launch_spot_as<0, 0>(L, r_max, stream);              // any other dimension: frames re-read per cell, column in LDS
    return e;
}

}  // namespace apd
