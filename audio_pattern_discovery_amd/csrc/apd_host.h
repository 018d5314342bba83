// What the host drivers of the pair-list entry points share (apd_path_api.hip, apd_spot_api.hip, apd_spot_stream_api.hip): the
// planning arithmetic of apd_plan.h and the pieces that need the project's types -- among them CurveSweep, the one sweep of a chunk of
// curves under apd_spot, apd_spot_detect and apd_spot_quantiles.
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

// What apd_spot, apd_spot_detect and apd_spot_quantiles check of their list: the pairs name sequences of the batch, and its lengths
// are sane; then, once the entry has answered what needs no launch, every pair's lengths in the entry's name.
inline int check_pair_list(const apd_batch *batch, const uint32_t *pairs, uint64_t n_pairs)
{
    for (uint64_t p = 0; p < n_pairs; ++p)
        if (pairs[2 * p] >= batch->n_seq || pairs[2 * p + 1] >= batch->n_seq) return APD_ERR_INVALID_ARG;
    return check_lengths(batch);
}
inline int spot_check_pairs(apd_context *ctx, const char *entry, const ResidentIndex &idx, const uint32_t *pairs, uint64_t n_pairs)
{
    for (uint64_t p = 0; p < n_pairs; ++p)
        if (int rc = spot_check_lengths(ctx, entry, idx.len(pairs[2 * p]), idx.len(pairs[2 * p + 1]))) return rc;
    return APD_OK;
}

// The first stage of apd_spot, apd_spot_detect and apd_spot_quantiles on one chunk of a GroupChunkPlan whose items are the
// caller's pairs and whose lengths are their streams' frames: launch_spot once per kernel class, the curves of slot k at the plan's
// offset, its best at L.d_best[k].  Per chunk, after next() has moved the plan to it, in this order:
//   carve()   opens `ws`, the layout of ws_spot, with the sweep's regions: curves (none: best only), bests, and the descriptors
//             last -- the records the caller takes next follow them in one host image, uploaded with one copy;
//   place()   once those are taken: sizes the image up to the end of `ws` and puts the descriptors at its head, by class;
//             record<T>(off) is where the caller's region at `off` lies in the image;
//   run()     once the whole workspace is taken: reserves it, uploads the image, zeroes the stretch the caller names, opens the
//             timing window at the list's first chunk and launches the sweep.  device<T>(off): a region on the device.
// The caller's own stage follows, then the end of the timing window at the list's last chunk; a synchronisation ends the chunk (the
// next one reuses the workspace and the image).
struct CurveSweep {
    apd_context *ctx;
    const apd_batch *batch;
    const apd_align_config *cfg;
    const ResidentIndex &idx;
    const uint32_t *pairs;
    Carve ws{};
    SpotClasses classes;
    SpotLaunch L{};                   // d_cost, d_start (null: best only) and d_best: the chunk's, once run() has returned
    std::vector<char> image;
    bool curves = true;
    size_t o_cost = 0, o_start = 0, o_best = 0, o_desc = 0;

    uint32_t query_len(uint64_t p) const { return idx.len(pairs[2 * p]); }
    uint32_t stream_len(uint64_t p) const { return idx.len(pairs[2 * p + 1]); }
    // the record a second stage reads the slot's curves by
    SpotCurve curve(const GroupChunkPlan::Slot &s) const { return {s.off, s.len, query_len(s.item), s.group, (uint32_t)s.item}; }
    template <class Weight> bool next(GroupChunkPlan &plan, Weight group_bytes) const
    {
        return plan.next(group_bytes, [this](uint64_t p) { return stream_len(p); });
    }
    void carve(const GroupChunkPlan &plan, bool with_curves = true)
    {
        curves = with_curves;
        ws = Carve();
        o_cost = ws.take<float>(curves ? plan.entries : 0); o_start = ws.take<uint32_t>(curves ? plan.entries : 0);
        o_best = ws.take<apd_spot_best>(plan.np()); o_desc = ws.take<SpotPair>(plan.np());
    }
    void place(const GroupChunkPlan &plan)
    {
        image.assign(ws.size - o_desc, 0);
        classes = SpotClasses();
        for (const auto &s : plan.slots) classes.add(batch->dim, query_len(s.item));
        classes.close();
        for (uint64_t k = 0; k < plan.np(); ++k) {
            const auto &s = plan.slots[k];
            record<SpotPair>(o_desc)[classes.slot(spot_row_class(batch->dim, query_len(s.item)))] =
                SpotPair{idx.pos[pairs[2 * s.item]], idx.pos[pairs[2 * s.item + 1]], (uint32_t)k, 0, s.off};
        }
    }
    template <class T> T *record(size_t off) { return (T *)(image.data() + (off - o_desc)); }
    template <class T> T *device(size_t off) const { return (T *)(ctx->ws_spot.as<char>() + off); }
    int run(const GroupChunkPlan &plan, size_t zero_off = 0, size_t zero_bytes = 0)
    {
        if (int rc = reserve_ws(ctx, ctx->ws_spot, ws.size)) return rc;
        L = SpotLaunch{};
        L.src = spot_source(batch, cfg->insertion_penalty, cfg->deletion_penalty, cfg->match_penalty);
        L.d_cost = curves ? device<float>(o_cost) : nullptr;
        L.d_start = curves ? device<uint32_t>(o_start) : nullptr;
        L.d_best = device<apd_spot_best>(o_best);
        HIP_TRY(ctx, hipMemcpyAsync(device<char>(o_desc), image.data(), image.size(), hipMemcpyHostToDevice, ctx->stream));
        if (zero_bytes) HIP_TRY(ctx, hipMemsetAsync(device<char>(zero_off), 0, zero_bytes, ctx->stream));
        if (ctx->timing && plan.g0 == 0) HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
        for (uint32_t c = 0; c < kSpotClasses; ++c) {
            L.d_pairs = device<SpotPair>(o_desc) + classes.first[c];
            L.n_pairs = (uint32_t)classes.n[c];
            HIP_TRY(ctx, launch_spot(L, c, classes.r_max, ctx->stream));
        }
        return APD_OK;
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
