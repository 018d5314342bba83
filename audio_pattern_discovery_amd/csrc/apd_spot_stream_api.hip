// C ABI of libapd_hip.so (include/apd.h): streaming spotting -- sessions, pushes of frames and of raw audio, the online detector and
// the history of a session.  The host side around dtw_spot_stream.hip, dtw_spot_stream_rec.hip and dtw_spot_online.hip.
#include <cstring>
#include <new>

#include "apd_host.h"

using namespace apd;

// A resident spotting session (include/apd.h, "streaming spotting"; kernels: dtw_spot_stream.hip).  Everything a push needs lives
// here and grows only: the pair descriptors (grouped by kernel class once, at create), the two halves of the carried columns, the
// running bests, the words a push uploads, the staged chunk and the curves.
struct apd_spot_stream : apd::ContextChild {
    const apd_batch *templates = nullptr;
    uint32_t n_queries = 0, n_channels = 0, n_pairs = 0;
    float ins = 0.0f, del = 0.0f, mat = 0.0f;
    std::vector<uint64_t> columns;      // per channel: absolute column of the last frame pushed (first_column after a reset)
    std::vector<uint32_t> parity;       // per channel: the half of d_state that holds its column
    std::vector<SpotStreamPair> h_pairs;
    std::vector<uint32_t> h_push;       // host image of d_push, alive as long as the session (the upload is asynchronous)
    SpotClasses classes;                // of d_pairs
    uint64_t state_half = 0;            // floats
    apd::DeviceBuf d_pairs, d_state, d_best;
    apd::DeviceBuf d_push;              // [chunk first n_channels + 1 | base n_channels | parity n_channels | the repack's words, kPadWords]
    apd::DeviceBuf d_raw;               // host chunks on their way to the repack kernel
    apd::DeviceBuf d_stage;             // the chunks in the resident layout, two sentinel frames behind them
    apd::DeviceBuf d_curves;            // [cost | start]
    // the history (apd_spot_stream_keep; kernels: dtw_spot_stream_rec.hip): the last `history` columns of every pair's branches and
    // row-n curve and of every channel's frames, in rings; 0: none kept, and a push runs the kernels it ran before there was one
    uint32_t history = 0;
    std::vector<uint64_t> origin;       // per channel: the column behind which the history starts (cells of columns > origin are kept)
    std::vector<uint32_t> q_len, q_pos; // per query: frames, resident position
    std::vector<uint32_t> wpl_before;   // per pair p: the sum of ceil(R / 16) over the pairs before it (and the total behind the last)
    apd::DeviceBuf d_hist_dirs, d_hist_curves, d_hist_frames, d_hist_wpl;
    // the online detector (apd_spot_stream_detect; kernels: dtw_spot_online.hip); a session that is not armed holds none of it and
    // a push runs the kernels it ran before there was one
    bool armed = false;
    uint32_t det_per_stream = 0, det_holdoff = 0, det_groups = 0;
    apd::DeviceBuf d_det_pairs, d_det_state, d_det_count;
    apd::DeviceBuf d_det_queue;         // det_cap records, the first det_queued of them queued, in arrival order
    uint64_t det_cap = 0, det_queued = 0;
    unsigned long long h_det_count = 0; // where a push's copy of *d_det_count lands (alive as long as the session)
    SpotOnlineLaunch online() const
    {
        SpotOnlineLaunch L{};
        L.d_push = d_push.as<uint32_t>();
        L.n_channels = n_channels; L.n_queries = n_queries;
        L.per_stream = det_per_stream; L.holdoff = det_holdoff; L.n_groups = det_groups;
        L.d_pairs = d_det_pairs.as<SpotOnlinePair>(); L.d_state = d_det_state.as<SpotOnlineState>();
        L.d_queue = d_det_queue.as<apd_spot_hit>(); L.d_count = d_det_count.as<unsigned long long>(); L.queue_cap = det_cap;
        return L;
    }
    SpotHistory rings() const
    {
        SpotHistory H{};
        H.rows = history;
        H.d_dirs = d_hist_dirs.as<uint32_t>(); H.d_wpl_before = d_hist_wpl.as<uint32_t>();
        H.d_curve_v = d_hist_curves.as<float>();
        H.d_curve_s = d_hist_curves.as<uint32_t>() + (size_t)n_pairs * history;
        H.d_frames = d_hist_frames.as<float>();
        return H;
    }
    // [first, last] of the channel's kept columns; first = last + 1: none
    void kept(uint32_t channel, uint64_t *first, uint64_t *last) const
    {
        const uint64_t end = columns[channel], from_ring = end + 1 > history ? end + 1 - history : 0;
        *last = end;
        *first = history ? std::max(origin[channel] + 1, from_ring) : end + 1;
    }
    // the staged chunks are ONE sequence to the repack kernel: [seq_off 2 | src_off 1 | unused 1 | flags 4 | norm maximum 1 | unused 3]
    static constexpr uint32_t kPadWords = 12;
    size_t push_words() const { return 3 * (size_t)n_channels + 1 + kPadWords; }
    SpotStreamLaunch launch() const
    {
        SpotStreamLaunch S{};
        S.src = spot_source(templates, ins, del, mat);
        S.d_stage = d_stage.as<float>(); S.d_push = d_push.as<uint32_t>();
        S.n_channels = n_channels; S.n_queries = n_queries;
        S.d_pairs = d_pairs.as<SpotStreamPair>(); S.n_pairs = n_pairs;
        S.d_state = d_state.as<float>(); S.state_half = state_half;
        S.d_best = d_best.as<apd_spot_best>();
        return S;
    }
    void release_device() override
    {
        d_pairs.reset(); d_state.reset(); d_best.reset(); d_push.reset(); d_raw.reset(); d_stage.reset(); d_curves.reset();
        d_hist_dirs.reset(); d_hist_curves.reset(); d_hist_frames.reset(); d_hist_wpl.reset();
        d_det_pairs.reset(); d_det_state.reset(); d_det_count.reset(); d_det_queue.reset();
    }
};

// Room for `extra` more hits behind the queued ones, made before the launch that may emit them: no hit is ever dropped.  Growth
// allocates first -- a refusal is APD_ERR_OOM with nothing enqueued and the session untouched -- then moves the queued records over.
static int spot_online_reserve(apd_context *ctx, apd_spot_stream *s, uint64_t extra)
{
    const uint64_t need = s->det_queued + extra;
    if (need <= s->det_cap) return APD_OK;
    const uint64_t cap = std::max(need, 2 * s->det_cap);
    apd::DeviceBuf grown;
    if (grown.alloc((size_t)cap * sizeof(apd_spot_hit)) != hipSuccess) {
        (void)hipGetLastError();
        ctx->last_error = "apd_spot_stream: no device memory for a queue of " + std::to_string(cap) + " hits";
        return APD_ERR_OOM;
    }
    if (s->det_queued) {
        HIP_TRY(ctx, hipMemcpyAsync(grown.ptr, s->d_det_queue.ptr, (size_t)s->det_queued * sizeof(apd_spot_hit), hipMemcpyDeviceToDevice, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));                  // the old queue is released below
    }
    s->d_det_queue = std::move(grown);
    s->det_cap = cap;
    return APD_OK;
}

extern "C" int apd_spot_stream_create(apd_context *ctx, const apd_batch *templates, const apd_align_config *cfg, const uint32_t *queries,
                                      uint32_t n_queries, uint32_t n_channels, apd_spot_stream **stream)
{
    if (!ctx || !templates || !cfg || !stream || !queries || templates->ctx != ctx) return APD_ERR_INVALID_ARG;
    *stream = nullptr;
    const uint64_t n_pairs = (uint64_t)n_queries * n_channels;
    if (n_pairs == 0 || n_pairs >= (1ull << 24)) return APD_ERR_INVALID_ARG;   // 64 work-items per pair: a launch stays below 2^31
    const uint32_t n_seq = templates->n_seq;
    for (uint32_t q = 0; q < n_queries; ++q)
        if (queries[q] >= n_seq) return APD_ERR_INVALID_ARG;
    const ResidentIndex idx(templates);
    for (uint32_t q = 0; q < n_queries; ++q)
        if (idx.len(queries[q]) == 0) return APD_ERR_EMPTY_SEQUENCE;
    for (uint32_t q = 0; q < n_queries; ++q)
        if (const int rc = spot_check_lengths(ctx, "apd_spot_stream_create", idx.len(queries[q]), 0)) return rc;
    HIP_TRY(ctx, bind_device(ctx));
    APD_AFFINITY(ctx, "spot stream allocation");
    apd_spot_stream *s = new (std::nothrow) apd_spot_stream();
    if (!s) return APD_ERR_OOM;
    s->templates = templates; s->n_queries = n_queries; s->n_channels = n_channels; s->n_pairs = (uint32_t)n_pairs;
    s->ins = cfg->insertion_penalty; s->del = cfg->deletion_penalty; s->mat = cfg->match_penalty;
    s->columns.assign(n_channels, 0);
    s->parity.assign(n_channels, 0u);
    s->origin.assign(n_channels, 0);
    s->h_push.assign(s->push_words(), 0u);
    for (uint32_t q = 0; q < n_queries; ++q) { s->q_len.push_back(idx.len(queries[q])); s->q_pos.push_back(idx.pos[queries[q]]); }
    s->wpl_before.assign(n_pairs + 1, 0u);
    for (uint64_t p = 0; p < n_pairs; ++p) s->wpl_before[p + 1] = s->wpl_before[p] + (spot_rows_per_lane(s->q_len[p % n_queries]) + 15) / 16;
    // the descriptors, grouped by kernel class (one launch each per push); `out` keeps p = channel n_queries + q
    for (uint32_t q = 0; q < n_queries; ++q) s->classes.add(templates->dim, s->q_len[q], n_channels);
    s->classes.close();
    s->h_pairs.resize(n_pairs);
    uint64_t state_floats = 0;
    for (uint32_t k = 0; k < n_channels; ++k)
        for (uint32_t q = 0; q < n_queries; ++q) {
            const uint32_t n = s->q_len[q], rows = spot_rows_per_lane(n);
            s->h_pairs[s->classes.slot(spot_row_class(templates->dim, n))] = SpotStreamPair{s->q_pos[q], k, k * n_queries + q, rows, state_floats};
            state_floats += 2ull * rows * 64;                             // values, then starts
        }
    s->state_half = state_floats;
    s->ctx = ctx;
    ctx->children.insert(s);                                              // from here on apd_spot_stream_destroy undoes everything
    auto fail = [&](int rc) { apd_spot_stream_destroy(s); return rc; };
    const size_t pair_bytes = (size_t)n_pairs * sizeof(SpotStreamPair);
    if (s->d_pairs.alloc(pair_bytes) != hipSuccess || s->d_state.alloc((size_t)state_floats * 2 * sizeof(float)) != hipSuccess ||
        s->d_best.alloc((size_t)n_pairs * sizeof(apd_spot_best)) != hipSuccess ||
        s->d_push.alloc(s->push_words() * sizeof(uint32_t)) != hipSuccess)
        return fail(APD_ERR_OOM);
    hipError_t e = hipMemcpyAsync(s->d_pairs.ptr, s->h_pairs.data(), pair_bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = launch_spot_stream_reset(s->launch(), 0xFFFFFFFFu, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { ctx->last_error = std::string("apd_spot_stream_create: ") + hipGetErrorString(e); return fail(APD_ERR_HIP); }
    *stream = s;
    return APD_OK;
}

extern "C" int apd_spot_stream_destroy(apd_spot_stream *stream) { return destroy_child(stream); }

extern "C" int apd_spot_stream_reset(apd_context *ctx, apd_spot_stream *stream, uint32_t channel, uint64_t first_column)
{
    if (!ctx || !stream || stream->ctx != ctx) return APD_ERR_INVALID_ARG;
    const bool all = channel == 0xFFFFFFFFu;
    if (!all && channel >= stream->n_channels) return APD_ERR_INVALID_ARG;
    if (first_column >= kSpotMaxStream) {
        ctx->last_error = "apd_spot_stream_reset: first_column at or beyond " + std::to_string(kSpotMaxStream);
        return APD_ERR_UNSUPPORTED;
    }
    HIP_TRY(ctx, bind_device(ctx));
    APD_AFFINITY(ctx, "spot stream reset");
    HIP_TRY(ctx, launch_spot_stream_reset(stream->launch(), channel, ctx->stream));
    // an armed session: the channel's pending windows go, its floors move to the new origin; ranks and queued hits stay
    if (stream->armed) HIP_TRY(ctx, launch_spot_online_touch(stream->online(), channel, false, (uint32_t)first_column, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (uint32_t k = 0; k < stream->n_channels; ++k)
        if (all || k == channel) stream->columns[k] = stream->origin[k] = first_column;   // either half holds column 0 now: the parity stays; the history is empty
    return APD_OK;
}

extern "C" int apd_spot_stream_columns(const apd_spot_stream *stream, uint32_t channel, uint64_t *columns)
{
    if (!stream || !columns || channel >= stream->n_channels) return APD_ERR_INVALID_ARG;
    *columns = stream->columns[channel];
    return APD_OK;
}

extern "C" int apd_spot_stream_push(apd_context *ctx, apd_spot_stream *stream, const float *frames, const uint64_t *chunk_off, uint32_t dim,
                                    int frames_on_device, float *cost, uint32_t *start, uint64_t capacity, uint64_t *curve_off,
                                    apd_spot_best *best)
{
    if (!ctx || !stream || stream->ctx != ctx || !chunk_off || !curve_off) return APD_ERR_INVALID_ARG;
    if ((cost == nullptr) != (start == nullptr)) return APD_ERR_INVALID_ARG;
    apd_spot_stream *s = stream;
    const apd_batch *t = s->templates;
    if (t->ctx != ctx || dim != t->src_dim) return APD_ERR_INVALID_ARG;
    const uint32_t n_ch = s->n_channels, n_q = s->n_queries;
    if (chunk_off[0] != 0) return APD_ERR_INVALID_ARG;
    for (uint32_t k = 0; k < n_ch; ++k)
        if (chunk_off[k + 1] < chunk_off[k]) return APD_ERR_INVALID_ARG;
    const uint64_t total = chunk_off[n_ch];
    if (total + 2 >= (1ull << 32) || (total > 0 && !frames)) return APD_ERR_INVALID_ARG;   // one resident "sequence", as a batch's limit
    for (uint32_t k = 0; k < n_ch; ++k)
        if (s->columns[k] + (chunk_off[k + 1] - chunk_off[k]) >= kSpotMaxStream) {
            ctx->last_error = "apd_spot_stream_push: channel " + std::to_string(k) + " would reach column " + std::to_string(kSpotMaxStream);
            return APD_ERR_UNSUPPORTED;
        }
    curve_off[0] = 0;
    for (uint32_t k = 0; k < n_ch; ++k)
        for (uint32_t q = 0; q < n_q; ++q) {
            const uint64_t p = (uint64_t)k * n_q + q;
            curve_off[p + 1] = curve_off[p] + (chunk_off[k + 1] - chunk_off[k]);
        }
    const bool curves = cost != nullptr;
    if (!curves && !best) return APD_OK;                                  // sizes only: the state is not advanced
    const uint64_t entries = curve_off[s->n_pairs];
    if (curves && capacity < entries) return APD_ERR_INVALID_ARG;
    HIP_TRY(ctx, bind_device(ctx));
    APD_AFFINITY(ctx, "spot stream launch");
    SpotStreamLaunch S = s->launch();
    const size_t best_bytes = (size_t)s->n_pairs * sizeof(apd_spot_best);
    if (total > 0) {
        // buffers: grown to the largest push seen, then reused
        // an armed session: the detector reads the curves on the device whether or not the caller asked for them on the host
        const bool stored = curves || s->armed;
        const size_t curve_bytes = stored ? ((size_t)entries * 4 + 15) / 16 * 16 : 0;
        HIP_TRY(ctx, s->d_stage.reserve((size_t)(total + 2) * t->dpad * sizeof(float)));
        if (stored) HIP_TRY(ctx, s->d_curves.reserve(2 * curve_bytes));
        const size_t raw_bytes = (size_t)total * dim * sizeof(float);
        if (!frames_on_device) HIP_TRY(ctx, s->d_raw.reserve(raw_bytes));
        if (s->armed) {
            // a group emits at most (chunk columns + 1) hits per push, and none on a channel without columns
            uint64_t bound = 0;
            for (uint32_t k = 0; k < n_ch; ++k)
                if (chunk_off[k + 1] > chunk_off[k]) bound += (chunk_off[k + 1] - chunk_off[k] + 1) * (s->det_per_stream ? 1u : n_q);
            if (const int rc = spot_online_reserve(ctx, s, bound)) return rc;
        }
        S = s->launch();
        S.d_cost = stored ? s->d_curves.as<float>() : nullptr;
        S.d_start = stored ? (uint32_t *)(s->d_curves.as<char>() + curve_bytes) : nullptr;
        // the words of this push
        uint32_t *w = s->h_push.data(), *pad = w + 3 * (size_t)n_ch + 1;
        for (uint32_t k = 0; k <= n_ch; ++k) w[k] = (uint32_t)chunk_off[k];
        for (uint32_t k = 0; k < n_ch; ++k) {
            w[n_ch + 1 + k] = (uint32_t)s->columns[k];
            w[2 * n_ch + 1 + k] = s->parity[k];
        }
        std::fill(pad, pad + apd_spot_stream::kPadWords, 0u);
        pad[1] = (uint32_t)total + 2;                                     // seq_off = {0, total + 2}, src_off = {0}, flags and norm maximum zeroed
        uint32_t *d_w = s->d_push.as<uint32_t>(), *d_pad = d_w + 3 * (size_t)n_ch + 1;
        HIP_TRY(ctx, hipMemcpyAsync(d_w, w, s->push_words() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        const float *d_src = frames;
        if (!frames_on_device) {
            HIP_TRY(ctx, hipMemcpyAsync(s->d_raw.ptr, frames, raw_bytes, hipMemcpyHostToDevice, ctx->stream));
            d_src = s->d_raw.as<float>();
        }
        if (ctx->timing) HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
        HIP_TRY(ctx, launch_pad(d_src, s->d_stage.as<float>(), d_pad, d_pad + 2, 1, total + 2, dim, t->dim, t->dpad, d_pad + 4,
                                reinterpret_cast<float *>(d_pad + 8), ctx->stream));
        SpotStreamRecLaunch A{S, s->rings()};
        if (s->history) HIP_TRY(ctx, launch_spot_stream_frames(A, (uint32_t)total, ctx->stream));
        for (uint32_t c = 0; c < kSpotClasses; ++c) {
            A.S.d_pairs = S.d_pairs = s->d_pairs.as<SpotStreamPair>() + s->classes.first[c];
            A.S.n_pairs = S.n_pairs = (uint32_t)s->classes.n[c];
            if (s->history) HIP_TRY(ctx, launch_spot_stream_record(A, c, s->classes.r_max, ctx->stream));
            else HIP_TRY(ctx, launch_spot_stream(S, c, s->classes.r_max, ctx->stream));
        }
        if (s->armed) {
            SpotOnlineLaunch O = s->online();
            O.d_cost = S.d_cost; O.d_start = S.d_start;
            uint64_t m_max = 0;
            for (uint32_t k = 0; k < n_ch; ++k) m_max = std::max(m_max, chunk_off[k + 1] - chunk_off[k]);
            HIP_TRY(ctx, launch_spot_online_scan(O, m_max, ctx->stream));
            HIP_TRY(ctx, hipMemcpyAsync(&s->h_det_count, O.d_count, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
        }
        if (ctx->timing) { HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream)); ctx->timed = true; }
        // the table has moved on, whatever the copies below do
        for (uint32_t k = 0; k < n_ch; ++k) {
            const uint64_t m = chunk_off[k + 1] - chunk_off[k];
            if (m) { s->columns[k] += m; s->parity[k] ^= 1u; }
        }
        if (curves) {
            HIP_TRY(ctx, hipMemcpyAsync(cost, S.d_cost, (size_t)entries * 4, hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipMemcpyAsync(start, S.d_start, (size_t)entries * 4, hipMemcpyDeviceToHost, ctx->stream));
        }
    }
    if (best) HIP_TRY(ctx, hipMemcpyAsync(best, S.d_best, best_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));                      // blocking: the results are the caller's, `frames` is free again
    if (s->armed && total > 0) s->det_queued = s->h_det_count;            // the queued count came back with that synchronisation
    return APD_OK;
}

// Raw audio into a session: the feed's push into its own device buffer, then the push above on those rows.  Everything either
// would refuse is refused before the feed moves on.
extern "C" int apd_spot_stream_push_audio(apd_context *ctx, apd_spot_stream *stream, apd_feed *feed, const int16_t *samples,
                                          const uint64_t *sample_off, int samples_on_device, float *cost, uint32_t *start,
                                          uint64_t capacity, uint64_t *curve_off, apd_spot_best *best)
{
    if (!ctx || !stream || stream->ctx != ctx || !feed || !sample_off || !curve_off) return APD_ERR_INVALID_ARG;
    const apd_context *feed_ctx = nullptr;
    uint32_t feed_channels = 0, dim = 0;
    feed_info(feed, &feed_ctx, &feed_channels, &dim);
    if (feed_ctx != ctx || feed_channels != stream->n_channels || dim != stream->templates->src_dim) return APD_ERR_INVALID_ARG;
    std::vector<uint64_t> chunk_off((size_t)feed_channels + 1);
    if (const int rc = feed_sizes(feed, sample_off, chunk_off.data())) return rc;
    // the session's own checks and curve_off: its sizes-only form
    if ((cost == nullptr) != (start == nullptr)) return APD_ERR_INVALID_ARG;
    static const float unread = 0.0f;                                     // the sizes-only form wants a frame pointer and does not follow it
    if (const int rc = apd_spot_stream_push(ctx, stream, &unread, chunk_off.data(), dim, 1, nullptr, nullptr, 0, curve_off, nullptr)) return rc;
    if (!cost && !best) return APD_OK;                                    // sizes only: neither state is advanced
    if (cost && capacity < curve_off[stream->n_pairs]) return APD_ERR_INVALID_ARG;
    if (sample_off[feed_channels] > sample_off[0] && !samples) return APD_ERR_INVALID_ARG;
    HIP_TRY(ctx, bind_device(ctx));
    const float *d_rows = nullptr;
    if (const int rc = feed_enqueue(ctx, feed, samples, sample_off, samples_on_device, chunk_off.data(), &d_rows)) return rc;
    return apd_spot_stream_push(ctx, stream, d_rows, chunk_off.data(), dim, 1, cost, start, capacity, curve_off, best);
}

// ---- the online detector of a session: apd_spot_stream_detect / _flush / _hits (include/apd.h; kernels: dtw_spot_online.hip)

extern "C" int apd_spot_stream_detect(apd_context *ctx, apd_spot_stream *stream, const float *thresholds, int compete, uint32_t holdoff)
{
    if (!ctx || !stream || stream->ctx != ctx) return APD_ERR_INVALID_ARG;
    if (compete != APD_DETECT_PER_PAIR && compete != APD_DETECT_PER_STREAM) return APD_ERR_INVALID_ARG;
    apd_spot_stream *s = stream;
    HIP_TRY(ctx, bind_device(ctx));
    APD_AFFINITY(ctx, "spot stream detector");
    if (!thresholds) {
        s->d_det_pairs.reset(); s->d_det_state.reset(); s->d_det_count.reset(); s->d_det_queue.reset();
        s->armed = false;
        s->det_groups = 0; s->det_cap = s->det_queued = 0;
        return APD_OK;
    }
    const uint32_t n_q = s->n_queries, groups = compete == APD_DETECT_PER_STREAM ? s->n_channels : s->n_pairs;
    std::vector<SpotOnlinePair> pairs(s->n_pairs);
    for (uint32_t p = 0; p < s->n_pairs; ++p) { pairs[p].n = s->q_len[p % n_q]; pairs[p].threshold = thresholds[p]; }
    // every group: no pending window, rank 0, the floor at its channel's current column (the detector's origin)
    std::vector<SpotOnlineState> state(groups, SpotOnlineState{});
    for (uint32_t g = 0; g < groups; ++g) state[g].floor = (uint32_t)s->columns[compete == APD_DETECT_PER_STREAM ? g : g / n_q];
    // the new buffers first: a refusal leaves the session as it was, armed or not
    apd::DeviceBuf d_pairs, d_state, d_count, d_queue;
    const uint64_t cap = s->d_det_queue ? s->det_cap : std::max<uint64_t>(groups, 64);
    if (d_pairs.alloc(pairs.size() * sizeof(SpotOnlinePair)) != hipSuccess || d_state.alloc(state.size() * sizeof(SpotOnlineState)) != hipSuccess ||
        d_count.alloc(sizeof(unsigned long long)) != hipSuccess ||
        (!s->d_det_queue && d_queue.alloc((size_t)cap * sizeof(apd_spot_hit)) != hipSuccess)) {
        (void)hipGetLastError();
        ctx->last_error = "apd_spot_stream_detect: no device memory for " + std::to_string(groups) + " groups";
        return APD_ERR_OOM;
    }
    HIP_TRY(ctx, hipMemcpyAsync(d_pairs.ptr, pairs.data(), pairs.size() * sizeof(SpotOnlinePair), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d_state.ptr, state.data(), state.size() * sizeof(SpotOnlineState), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(d_count.ptr, 0, sizeof(unsigned long long), ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    s->d_det_pairs = std::move(d_pairs); s->d_det_state = std::move(d_state); s->d_det_count = std::move(d_count);
    if (!s->d_det_queue) s->d_det_queue = std::move(d_queue);             // arming again keeps the queue's memory and discards its hits
    s->det_cap = cap; s->det_queued = 0;
    s->det_per_stream = (uint32_t)compete; s->det_holdoff = holdoff; s->det_groups = groups;
    s->armed = true;
    return APD_OK;
}

extern "C" int apd_spot_stream_flush(apd_context *ctx, apd_spot_stream *stream, uint32_t channel)
{
    if (!ctx || !stream || stream->ctx != ctx) return APD_ERR_INVALID_ARG;
    apd_spot_stream *s = stream;
    if (channel != 0xFFFFFFFFu && channel >= s->n_channels) return APD_ERR_INVALID_ARG;
    if (!s->armed) {
        ctx->last_error = "apd_spot_stream_flush: the session is not armed (apd_spot_stream_detect)";
        return APD_ERR_UNSUPPORTED;
    }
    HIP_TRY(ctx, bind_device(ctx));
    APD_AFFINITY(ctx, "spot stream flush");
    if (const int rc = spot_online_reserve(ctx, s, s->det_groups)) return rc;   // one pending window per group at most
    const SpotOnlineLaunch O = s->online();
    HIP_TRY(ctx, launch_spot_online_touch(O, channel, true, 0u, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&s->h_det_count, O.d_count, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    s->det_queued = s->h_det_count;
    return APD_OK;
}

extern "C" int apd_spot_stream_hits(apd_context *ctx, apd_spot_stream *stream, apd_spot_hit *hits, uint64_t capacity, uint64_t *n_hits)
{
    if (!ctx || !stream || stream->ctx != ctx || !n_hits) return APD_ERR_INVALID_ARG;
    apd_spot_stream *s = stream;
    *n_hits = s->armed ? s->det_queued : 0;
    if (*n_hits == 0 || capacity < *n_hits) return APD_OK;                // too small: nothing written, nothing consumed
    if (!hits) return APD_ERR_INVALID_ARG;
    HIP_TRY(ctx, bind_device(ctx));
    APD_AFFINITY(ctx, "spot stream hits");
    std::vector<apd_spot_hit> h((size_t)*n_hits);
    HIP_TRY(ctx, hipMemcpyAsync(h.data(), s->d_det_queue.ptr, h.size() * sizeof(apd_spot_hit), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(s->d_det_count.ptr, 0, sizeof(unsigned long long), ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    s->det_queued = 0;
    // the queue holds arrival order, which depends on scheduling; (group, rank) is unique and does not
    const uint32_t per_group = s->det_per_stream ? s->n_queries : 1u;
    std::sort(h.begin(), h.end(), [&](const apd_spot_hit &a, const apd_spot_hit &b) {
        const uint32_t ga = a.pair / per_group, gb = b.pair / per_group;
        return ga != gb ? ga < gb : a.rank < b.rank;
    });
    std::copy(h.begin(), h.end(), hits);
    return APD_OK;
}

// ---- the history of a session: apd_spot_stream_keep / _history / _paths (include/apd.h; kernels: dtw_spot_stream_rec.hip)

extern "C" int apd_spot_stream_keep(apd_context *ctx, apd_spot_stream *stream, uint32_t history_columns)
{
    if (!ctx || !stream || stream->ctx != ctx) return APD_ERR_INVALID_ARG;
    apd_spot_stream *s = stream;
    HIP_TRY(ctx, bind_device(ctx));
    APD_AFFINITY(ctx, "spot stream history");
    const uint64_t H = history_columns;
    apd::DeviceBuf dirs, curves, frames;
    if (H) {
        // the new rings first: a refusal leaves the session with the ones it has
        const uint64_t dir_bytes = (uint64_t)s->wpl_before[s->n_pairs] * H * 64 * sizeof(uint32_t);
        const uint64_t curve_bytes = (uint64_t)s->n_pairs * H * 8, frame_bytes = (uint64_t)s->n_channels * H * s->templates->dpad * sizeof(float);
        if (dirs.alloc((size_t)dir_bytes) != hipSuccess || curves.alloc((size_t)curve_bytes) != hipSuccess ||
            frames.alloc((size_t)frame_bytes) != hipSuccess || (!s->d_hist_wpl.ptr && s->d_hist_wpl.alloc((size_t)s->n_pairs * sizeof(uint32_t)) != hipSuccess)) {
            (void)hipGetLastError();
            ctx->last_error = "apd_spot_stream_keep: no device memory for " + std::to_string(H) + " columns of history";
            return APD_ERR_OOM;
        }
        // nothing reads a row before a push has written it; zeros all the same, so that no run depends on what the memory held
        HIP_TRY(ctx, hipMemsetAsync(dirs.ptr, 0, (size_t)dir_bytes, ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(curves.ptr, 0, (size_t)curve_bytes, ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(frames.ptr, 0, (size_t)frame_bytes, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(s->d_hist_wpl.ptr, s->wpl_before.data(), (size_t)s->n_pairs * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    s->d_hist_dirs = std::move(dirs); s->d_hist_curves = std::move(curves); s->d_hist_frames = std::move(frames);
    s->history = history_columns;
    s->origin = s->columns;                                               // the history starts empty, behind every channel's current column
    return APD_OK;
}

extern "C" int apd_spot_stream_history(const apd_spot_stream *stream, uint32_t channel, uint64_t *first, uint64_t *last)
{
    if (!stream || !first || !last || channel >= stream->n_channels) return APD_ERR_INVALID_ARG;
    stream->kept(channel, first, last);
    return APD_OK;
}

// The windows are taken in input order, a chunk at a time: as many as keep the steps under the workspace cap, at least one.  What
// the rings no longer hold is decided here: a window whose end lies before the channel's first kept column never reaches the
// device; one whose end is kept is given to the trace, which reads S[n][end] and walks only if that start is kept as well.
extern "C" int apd_spot_stream_paths(apd_context *ctx, apd_spot_stream *stream, const apd_spot_window *windows, uint64_t n_windows,
                                     apd_path_step *steps, uint64_t capacity, uint64_t *step_off, uint32_t *path_len,
                                     uint32_t *found_start, float *scores)
{
    if (!ctx || !stream || stream->ctx != ctx || !step_off || (n_windows && !windows)) return APD_ERR_INVALID_ARG;
    const apd_spot_stream *s = stream;
    const apd_batch *t = s->templates;
    if (t->ctx != ctx) return APD_ERR_INVALID_ARG;
    for (uint64_t p = 0; p < n_windows; ++p) {
        const apd_spot_window &w = windows[p];
        if (w.x >= s->n_queries || w.y >= s->n_channels) return APD_ERR_INVALID_ARG;
        if (w.end > s->columns[w.y] || (w.end && w.start > w.end)) return APD_ERR_INVALID_ARG;
    }
    step_off[0] = 0;
    for (uint64_t p = 0; p < n_windows; ++p)
        step_off[p + 1] = step_off[p] + apd_spot_path_bound(s->q_len[windows[p].x], windows[p].end, windows[p].start);
    if (!steps) return APD_OK;                                            // sizes only
    if (capacity < step_off[n_windows] || (n_windows && !path_len)) return APD_ERR_INVALID_ARG;
    if (!s->history) {
        ctx->last_error = "apd_spot_stream_paths: the session keeps no history (apd_spot_stream_keep)";
        return APD_ERR_UNSUPPORTED;
    }
    if (n_windows == 0) return APD_OK;
    HIP_TRY(ctx, bind_device(ctx));
    APD_AFFINITY(ctx, "spot stream path launch");
    ChunkBudget budget{workspace_cap("APD_SPOT_WORKSPACE_BYTES"), kMaxPairsPerLaunch};
    WindowResults results{path_len, found_start, scores};
    std::vector<uint64_t> &live = results.live;
    std::vector<SpotRingWindow> trace;
    bool first_launch = true;
    for (uint64_t first = 0; first < n_windows;) {
        uint64_t last = first;
        budget.reset();
        while (last < n_windows && budget.admit((step_off[last + 1] - step_off[last]) * sizeof(apd_path_step))) ++last;
        live.clear(); trace.clear();
        for (uint64_t p = first; p < last; ++p) {
            const apd_spot_window &w = windows[p];
            uint64_t kept_first, kept_last;
            s->kept(w.y, &kept_first, &kept_last);
            if (step_off[p + 1] > step_off[p] && w.end >= kept_first) {
                SpotRingWindow r{};
                r.px = s->q_pos[w.x]; r.channel = w.y; r.pair = w.y * s->n_queries + w.x;
                r.end = w.end; r.start = w.start; r.first = (uint32_t)kept_first;
                r.step_off = step_off[p] - step_off[first];
                live.push_back(p); trace.push_back(r);
                continue;
            }
            results.dead(p);                                              // no window, or its end has aged out: nothing to read
            std::memset(steps + step_off[p], 0, (size_t)(step_off[p + 1] - step_off[p]) * sizeof(apd_path_step));
        }
        if (live.empty()) { first = last; continue; }
        const size_t steps_bytes = (size_t)(step_off[last] - step_off[first]) * sizeof(apd_path_step);
        Carve ws;                                                         // ws_spot_steps: the steps, the windows (uploaded), their results
        const size_t o_steps = ws.take<apd_path_step>(step_off[last] - step_off[first]), o_win = ws.take<SpotRingWindow>(trace.size());
        results.carve(ws);
        int rc = reserve_ws(ctx, ctx->ws_spot_steps, ws.size);
        if (rc) return rc;
        char *base = ctx->ws_spot_steps.as<char>();
        SpotRingTraceLaunch L{};
        L.src = spot_source(t, s->ins, s->del, s->mat);
        L.H = s->rings();
        L.d_windows = (const SpotRingWindow *)(base + o_win);
        L.d_steps = (apd_path_step *)(base + o_steps);
        results.bind(L, base);
        HIP_TRY(ctx, hipMemcpyAsync(base + o_win, trace.data(), trace.size() * sizeof(SpotRingWindow), hipMemcpyHostToDevice, ctx->stream));
        // an aged-out window between two traced ones leaves slots of the chunk no trace owns: the device copy is zeroed whole
        HIP_TRY(ctx, hipMemsetAsync(L.d_steps, 0, steps_bytes, ctx->stream));
        if (ctx->timing && first_launch) HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
        first_launch = false;
        HIP_TRY(ctx, launch_spot_stream_trace(L, ctx->stream));
        if (ctx->timing) { HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream)); ctx->timed = true; }   // the last chunk's record stands
        HIP_TRY(ctx, hipMemcpyAsync(steps + step_off[first], L.d_steps, steps_bytes, hipMemcpyDeviceToHost, ctx->stream));
        if ((rc = results.read_back(ctx, L))) return rc;
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));                  // the next chunk reuses the workspace (and `trace`)
        results.scatter();
        first = last;
    }
    return APD_OK;
}
