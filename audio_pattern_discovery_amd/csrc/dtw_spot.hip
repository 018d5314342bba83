// Subsequence alignment ("spotting", gfx950): apd_spot.  A query x of n frames against every window of a stream y of m frames in ONE
// DP: the recurrence of alignments.rs:153-159 with a free start (row 0 of the table is 0 in every column, column 0 is +INF below
// it), no band, and the column in which each cell's alignment left row 0 carried along with the value.  The results are the last
// row's value and start per stream column (include/apd.h, "subsequence alignment").
//
// The reference has no spotting, so nothing of it is mirrored beyond the recurrence and the arithmetic -- in particular NOT its habit
// of reading the score one row and one column short, at (n-1, m-1) (alignments.rs:120): the curves are row n's, or a one-frame query
// would have no row at all.
//
// The sweep itself -- lane mapping, macro-step, arithmetic -- is spot_sweep (dtw_spot_sweep.h), which the other three sweep kinds
// share, as they share the kernel template and the launcher; the kind SpotSweep runs it with REC = false: the lane that owns row n
// stores the curves (when the caller asked for them) and keeps the running best -- the scan over j is serial there already, no
// atomics, no reduction.  spot_lds_bytes and spot_debug_line, which the launcher calls for every kind, live here.
#include <cstdio>
#include <cstdlib>

#include "dtw_spot_sweep.h"

namespace apd {

struct SpotSweep {
    using Launch = SpotLaunch;
    static constexpr const char *word = "sweep";
    template <int RT, int D>
    static __device__ __forceinline__ void pair(const Launch &L)
    {
        spot_sweep<RT, D, false>(L.src, SpotOut{L.d_cost, L.d_start, L.d_best}, L.d_pairs[blockIdx.x], SpotRecord{});
    }
};

size_t spot_lds_bytes(uint32_t rows_per_lane) { return (size_t)rows_per_lane * 64 * (sizeof(float) + sizeof(uint32_t)); }

void spot_debug_line(const char *kind, int rt, int d, uint32_t n_pairs, uint32_t r_max, size_t lds_bytes)
{
    if (!std::getenv("APD_DEBUG_PLAN")) return;
    if (rt > 0)
        std::fprintf(stderr, "[apd] spot %s kernel <%d, %d>: %u pairs\n", kind, rt, d, n_pairs);
    else
        std::fprintf(stderr, "[apd] spot %s kernel <0, %d>: %u pairs, r_max %u, lds %zu bytes\n", kind, d, n_pairs, r_max, lds_bytes);
}

hipError_t launch_spot(const SpotLaunch &L, uint32_t rt, uint32_t r_max, hipStream_t stream)
{
    return spot_launch<SpotSweep>(L, L.n_pairs, L.src.dim, rt, r_max, stream);
}

}  // namespace apd
