// What the host drivers of the pair-list entry points share (apd_path_api.hip, apd_spot_api.hip, apd_spot_stream_api.hip): the
// planning arithmetic of apd_plan.h and the few pieces that need the project's types.
#pragma once
#include <algorithm>
#include <cmath>

#include "apd_internal.h"
#include "apd_plan.h"

#pragma GCC visibility push(hidden)   // internal to libapd_hip.so, as apd_plan.h
namespace apd {

// 64 work-items per pair or window: a launch of so many stays below 2^31 work-items
constexpr uint64_t kMaxPairsPerLaunch = 1ull << 24;

// Caller's sequence number -> resident position, and the sequence's frames.
struct ResidentIndex {
    const apd_batch *batch;
    std::vector<uint32_t> pos;
    explicit ResidentIndex(const apd_batch *b) : batch(b), pos(b->n_seq) { for (uint32_t p = 0; p < b->n_seq; ++p) pos[b->order[p]] = p; }
    uint32_t len(uint32_t s) const { return (uint32_t)(batch->offsets[pos[s] + 1] - batch->offsets[pos[s]]); }
};

// The head every spotting launch struct begins with: the batch the query rows come from, and the penalties.
inline SpotSource spot_source(const apd_batch *b, float ins, float del, float mat)
{
    return {b->d_frames.as<float>(), b->d_seq_off, b->dim, b->dpad, ins, del, mat};
}

// A query of n frames against a stream of m: APD_ERR_UNSUPPORTED beyond what the spotting kernels hold, in `entry`'s name.
inline int spot_check_lengths(apd_context *ctx, const char *entry, uint32_t n, uint64_t m)
{
    if (n <= kSpotMaxQuery && m < kSpotMaxStream) return APD_OK;
    ctx->last_error = std::string(entry) + ": a query of more than " + std::to_string(kSpotMaxQuery) + " frames";
    return APD_ERR_UNSUPPORTED;
}

// The descriptors of a spotting launch, grouped by kernel class (spot_row_class): one launch per class.
struct SpotClasses : ClassBuckets<kSpotClasses> {
    uint32_t r_max = 1;             // the most rows per lane among the queries of class 0: it sizes their LDS
    uint32_t add(uint32_t dim, uint32_t n, uint64_t items = 1)   // counts `items` descriptors of a query of n frames; its class
    {
        const uint32_t c = spot_row_class(dim, n);
        count(c, items);
        if (c == 0) r_max = std::max(r_max, spot_rows_per_lane(n));
        return c;
    }
};

// The per-window results of a chunk of window paths (apd_spot_paths, apd_spot_stream_paths).  live: the chunk's windows that reach
// the trace, in input order; the device holds [lengths | found | scores] of those, the caller's arrays are indexed by window.
struct WindowResults {
    uint32_t *path_len, *found_start;   // found_start and scores may be null
    float *scores;
    std::vector<uint64_t> live;
    std::vector<uint32_t> h_len, h_found;
    std::vector<float> h_scores;
    size_t o_len = 0, o_found = 0, o_scores = 0;
    void set(uint64_t p, uint32_t len, uint32_t found, float score) const
    {
        path_len[p] = len;
        if (found_start) found_start[p] = found;
        if (scores) scores[p] = score;
    }
    void dead(uint64_t p) const { set(p, 0, 0, INFINITY); }   // a window that reaches no trace: no path
    void carve(Carve &ws)
    {
        o_len = ws.take<uint32_t>(live.size()); o_found = ws.take<uint32_t>(live.size()); o_scores = ws.take<float>(live.size());
    }
    template <class L> void bind(L &l, char *base) const
    {
        l.n_windows = (uint32_t)live.size();
        l.d_len = (uint32_t *)(base + o_len); l.d_found = (uint32_t *)(base + o_found); l.d_scores = (float *)(base + o_scores);
    }
    // the three copies to the host, enqueued; scatter() after the synchronisation
    template <class L> int read_back(apd_context *ctx, const L &l)
    {
        const size_t nt = live.size();
        h_len.resize(nt); h_found.resize(nt); h_scores.resize(nt);
        HIP_TRY(ctx, hipMemcpyAsync(h_len.data(), l.d_len, nt * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(h_found.data(), l.d_found, nt * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(h_scores.data(), l.d_scores, nt * 4, hipMemcpyDeviceToHost, ctx->stream));
        return APD_OK;
    }
    void scatter() const { for (size_t t = 0; t < live.size(); ++t) set(live[t], h_len[t], h_found[t], h_scores[t]); }
};

}  // namespace apd
#pragma GCC visibility pop
