// C ABI of libapd_hip.so (include/apd.h): warping paths of selected pairs and DTW barycenters, the host side around dtw_path.hip.
#include <cstring>

#include "apd_host.h"

using namespace apd;

extern "C" uint64_t apd_path_bound(uint64_t n, uint64_t m) { return (n == 0 || m == 0) ? 0 : n + m - 1; }

namespace {

// Pairs [first, last) of a plan, swept and traced by one launch each: `words` direction words, `slots` step slots, c_max the most
// band offsets per lane among them.
struct PathChunk { uint64_t first, last, words, slots; uint32_t c_max; };

// A pair list cut into chunks whose direction words and steps each stay under APD_PATH_WORKSPACE_BYTES, one pair at least.
// apd_align_paths and apd_barycenters cut the same list the same way.
struct PathPlan {
    std::vector<PathPair> desc;           // dir_off, step_off: relative to the pair's chunk
    uint64_t n = 0;                       // pairs added
    std::vector<PathChunk> chunks;
    ChunkBudget budget{workspace_cap("APD_PATH_WORKSPACE_BYTES"), kMaxPairsPerLaunch};
    explicit PathPlan(uint64_t n_pairs) : desc(n_pairs) {}
    // the pair of x (nx frames, position px of its side) and y (my frames, resident position py); false: its band is too wide
    bool add(const BandSpec &band, uint32_t nx, uint32_t my, uint32_t px, uint32_t py)
    {
        const uint32_t w = host_w(band, nx, my);
        if (2ull * w + 1 > kPathMaxOffsets) return false;
        const uint64_t words = path_dir_words(nx, my, w), slots = apd_path_bound(nx, my);
        if (chunks.empty() || !budget.admit(words * sizeof(uint32_t), slots * sizeof(apd_path_step))) {
            budget.reset();
            budget.admit(words * sizeof(uint32_t), slots * sizeof(apd_path_step));
            chunks.push_back(PathChunk{n, n, 0, 0, 2});
        }
        PathChunk &c = chunks.back();
        desc[n++] = PathPair{px, py, c.words, c.slots};
        c.last = n; c.words += words; c.slots += slots;
        c.c_max = std::max(c.c_max, path_cells_per_lane(w));
        return true;
    }
};

constexpr const char *kBandTooWide = "band too wide for the path sweep";

// The sweep and the trace (dtw_path.hip) over `pairs`, a chunk at a time.
int align_paths_impl(apd_context *ctx, const apd_batch *batch, const BandSpec &band, const uint32_t *pairs, uint64_t n_pairs,
                     apd_path_step *steps, uint64_t capacity, uint64_t *step_off, uint32_t *path_len, float *scores)
{
    if (!ctx || !batch || batch->ctx != ctx || !step_off || (n_pairs && !pairs)) return APD_ERR_INVALID_ARG;
    const uint32_t n_seq = batch->n_seq;
    const ResidentIndex idx(batch);
    for (uint64_t p = 0; p < n_pairs; ++p)
        if (pairs[2 * p] >= n_seq || pairs[2 * p + 1] >= n_seq) return APD_ERR_INVALID_ARG;
    int rc = check_lengths(batch);
    if (rc) return rc;
    step_off[0] = 0;
    for (uint64_t p = 0; p < n_pairs; ++p) step_off[p + 1] = step_off[p] + apd_path_bound(idx.len(pairs[2 * p]), idx.len(pairs[2 * p + 1]));
    if (!steps) return APD_OK;                                            // sizes only
    if (capacity < step_off[n_pairs] || (n_pairs && !path_len)) return APD_ERR_INVALID_ARG;
    if (n_pairs == 0) return APD_OK;
    PathPlan plan(n_pairs);
    for (uint64_t p = 0; p < n_pairs; ++p) {
        const uint32_t x = pairs[2 * p], y = pairs[2 * p + 1];
        if (!plan.add(band, idx.len(x), idx.len(y), idx.pos[x], idx.pos[y])) { ctx->last_error = kBandTooWide; return APD_ERR_BAND_TOO_WIDE; }
    }
    HIP_TRY(ctx, bind_device(ctx));
    APD_AFFINITY(ctx, "path launch");
    std::vector<float> score_sink;
    if (!scores) score_sink.resize(n_pairs);
    float *h_scores = scores ? scores : score_sink.data();
    for (const PathChunk &c : plan.chunks) {
        const uint64_t np = c.last - c.first;
        Carve ws;
        const size_t o_steps = ws.take<apd_path_step>(c.slots), o_desc = ws.take<PathPair>(np);
        const size_t o_len = ws.take<uint32_t>(np), o_scores = ws.take<float>(np);
        rc = reserve_ws(ctx, ctx->ws_path_dirs, std::max<size_t>((size_t)c.words * sizeof(uint32_t), 16));
        if (rc) return rc;
        rc = reserve_ws(ctx, ctx->ws_path_steps, ws.size);
        if (rc) return rc;
        char *base = ctx->ws_path_steps.as<char>();
        PathLaunch L{};
        L.d_frames = batch->d_frames.as<float>(); L.d_seq_off = batch->d_seq_off; L.dim = batch->dim; L.dpad = batch->dpad; L.band = band;
        L.d_pairs = (const PathPair *)(base + o_desc);
        L.n_pairs = (uint32_t)np;
        L.d_dirs = ctx->ws_path_dirs.as<uint32_t>();
        L.d_steps = (apd_path_step *)(base + o_steps);
        L.d_len = (uint32_t *)(base + o_len);
        L.d_scores = (float *)(base + o_scores);
        HIP_TRY(ctx, hipMemcpyAsync((void *)L.d_pairs, plan.desc.data() + c.first, (size_t)np * sizeof(PathPair), hipMemcpyHostToDevice, ctx->stream));
        if (ctx->timing && c.first == 0) HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
        HIP_TRY(ctx, launch_path_sweep(L, c.c_max, ctx->stream));
        HIP_TRY(ctx, launch_path_trace(L, ctx->stream));
        if (ctx->timing && c.last == n_pairs) { HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream)); ctx->timed = true; }
        if (c.slots) HIP_TRY(ctx, hipMemcpyAsync(steps + step_off[c.first], L.d_steps, (size_t)c.slots * sizeof(apd_path_step), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(path_len + c.first, L.d_len, (size_t)np * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(h_scores + c.first, L.d_scores, (size_t)np * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));                  // the next chunk reuses the workspaces
    }
    return APD_OK;
}

}  // namespace

extern "C" int apd_align_paths(apd_context *ctx, const apd_batch *batch, const apd_align_config *cfg, const uint32_t *pairs,
                               uint64_t n_pairs, apd_path_step *steps, uint64_t capacity, uint64_t *step_off, uint32_t *path_len,
                               float *scores)
{
    if (!ctx || !batch || !cfg) return APD_ERR_INVALID_ARG;
    return align_paths_impl(ctx, batch, band_from_cfg(cfg), pairs, n_pairs, steps, capacity, step_off, path_len, scores);
}

extern "C" int apd_align_pair_path(apd_context *ctx, const float *x, uint64_t n, const float *y, uint64_t m, uint32_t dim,
                                   const apd_alignment_params *params, apd_path_step *steps, uint64_t capacity, uint64_t *n_steps,
                                   float *score)
{
    if (!ctx || !params || !n_steps || !score || dim == 0) return APD_ERR_INVALID_ARG;
    if (n == 0 && m == 0) { *n_steps = 0; *score = INFINITY; return APD_OK; }   // alignments.rs:117-118
    if (n == 0 || m == 0) return APD_ERR_EMPTY_SEQUENCE;                  // usize underflow at :120
    if (!x || !y) return APD_ERR_INVALID_ARG;
    if (!steps) { *n_steps = apd_path_bound(n, m); return APD_OK; }
    if (capacity < apd_path_bound(n, m)) return APD_ERR_INVALID_ARG;
    int rc = prepare_pair_batch(ctx, x, n, y, m, dim);
    if (rc) return rc;
    const uint32_t pair[2] = {0, 1};
    uint64_t off[2] = {0, 0};
    uint32_t len = 0;
    rc = align_paths_impl(ctx, ctx->pair_batch, band_from_params(params), pair, 1, steps, capacity, off, &len, score);
    if (rc == APD_OK) *n_steps = len;
    return rc;
}

// ------------------------------------------------------------------------------ DTW barycenters

// DBA over sets of a resident batch (kernels: dtw_path.hip).  The pairs (set, member ascending) are cut into chunks once; every
// iteration runs sweep, trace and accumulate per chunk, then one finalize.
extern "C" int apd_barycenters(apd_context *ctx, const apd_batch *batch, const apd_align_config *cfg, const uint32_t *members,
                               const uint32_t *set_off, uint32_t n_sets, const uint32_t *init, uint32_t iterations, float *frames,
                               int frames_on_device, uint64_t capacity, uint64_t *frame_off, float *inertia, uint32_t *used)
{
    if (!ctx || !batch || !cfg || batch->ctx != ctx || !frame_off || (n_sets && (!set_off || !init))) return APD_ERR_INVALID_ARG;
    if (n_sets && set_off[0] != 0) return APD_ERR_INVALID_ARG;
    for (uint32_t k = 0; k < n_sets; ++k) if (set_off[k + 1] < set_off[k]) return APD_ERR_INVALID_ARG;
    const uint32_t n_pairs = n_sets ? set_off[n_sets] : 0u, n_seq = batch->n_seq;
    if (n_pairs && !members) return APD_ERR_INVALID_ARG;
    // ascending sequence number inside every set: the order of the contract's sums
    std::vector<uint32_t> sorted(members, members + n_pairs);
    for (uint32_t k = 0; k < n_sets; ++k) {
        if (init[k] >= n_seq) return APD_ERR_INVALID_ARG;
        std::sort(sorted.begin() + set_off[k], sorted.begin() + set_off[k + 1]);
        for (uint32_t t = set_off[k]; t < set_off[k + 1]; ++t)
            if (sorted[t] >= n_seq || (t > set_off[k] && sorted[t] == sorted[t - 1])) return APD_ERR_INVALID_ARG;
    }
    int rc = check_lengths(batch);
    if (rc) return rc;
    const ResidentIndex idx(batch);
    auto frames_of = [&](uint32_t k) { return set_off[k + 1] > set_off[k] ? idx.len(init[k]) : 0u; };   // an empty set has no barycenter
    frame_off[0] = 0;
    for (uint32_t k = 0; k < n_sets; ++k) frame_off[k + 1] = frame_off[k] + frames_of(k);
    if (!frames) return APD_OK;                                           // sizes only
    if (capacity < frame_off[n_sets]) return APD_ERR_INVALID_ARG;
    const BandSpec band = band_from_cfg(cfg);
    const uint64_t n_padded = frame_off[n_sets] + 2ull * n_sets;
    if (n_padded >= (1ull << 32) || n_padded * batch->dpad >= (1ull << 39)) return APD_ERR_INVALID_ARG;   // one work-item per float, below 2^31 workgroups

    // ---- the plan: pair descriptors (px: the set, whose barycenter is x), chunks, and per chunk the pairs of every set
    PathPlan plan(n_pairs);
    for (uint32_t k = 0; k < n_sets; ++k)
        for (uint32_t t = set_off[k]; t < set_off[k + 1]; ++t)
            if (!plan.add(band, frames_of(k), idx.len(sorted[t]), k, idx.pos[sorted[t]])) { ctx->last_error = kBandTooWide; return APD_ERR_BAND_TOO_WIDE; }
    const std::vector<PathChunk> &chunks = plan.chunks;
    std::vector<uint2> set_pairs(chunks.size() * n_sets);                 // per chunk and set: its pairs [x, y), relative to the chunk
    uint64_t max_words = 0, max_slots = 0, max_np = 0;
    for (size_t ci = 0; ci < chunks.size(); ++ci) {
        const PathChunk &c = chunks[ci];
        for (uint32_t k = 0; k < n_sets; ++k) {
            const uint64_t lo = std::min(std::max<uint64_t>(set_off[k], c.first), c.last), hi = std::min(std::max<uint64_t>(set_off[k + 1], c.first), c.last);
            set_pairs[ci * n_sets + k] = make_uint2((uint32_t)(lo - c.first), (uint32_t)(hi - c.first));
        }
        max_words = std::max(max_words, c.words); max_slots = std::max(max_slots, c.slots); max_np = std::max(max_np, c.last - c.first);
    }
    if (n_sets == 0) return APD_OK;

    // ---- device state
    HIP_TRY(ctx, bind_device(ctx));
    APD_AFFINITY(ctx, "barycenter launch");
    // ws_bary: what an iteration zeroes is [sums | counts | score sums | used], what is uploaded once [bary_off .. contributes)
    Carve ws(256);
    const size_t bary_floats = (size_t)n_padded * batch->dpad, results = (size_t)iterations * n_sets;
    const size_t o_bary = ws.take<float>(bary_floats), o_sum = ws.take<float>(bary_floats), o_cnt = ws.take<uint32_t>(n_padded);
    const size_t o_score = ws.take<float>(n_sets), o_used = ws.take<uint32_t>(n_sets);
    const size_t o_off = ws.take<uint32_t>((size_t)n_sets + 1), o_init = ws.take<uint32_t>(n_sets);
    const size_t o_desc = ws.take<PathPair>(plan.desc.size()), o_ranges = ws.take<uint2>(set_pairs.size());
    const size_t o_contrib = ws.take<uint32_t>(max_np), o_inertia = ws.take<float>(results), o_usedout = ws.take<uint32_t>(results);
    rc = reserve_ws(ctx, ctx->ws_bary, ws.size);
    if (rc) return rc;
    rc = reserve_ws(ctx, ctx->ws_path_dirs, std::max<size_t>((size_t)max_words * sizeof(uint32_t), 16));
    if (rc) return rc;
    Carve steps_ws;                                                       // as apd_align_paths lays it out, the descriptors apart (ws_bary)
    const size_t o_steps = steps_ws.take<apd_path_step>(max_slots), o_len = steps_ws.take<uint32_t>(max_np), o_scores = steps_ws.take<float>(max_np);
    rc = reserve_ws(ctx, ctx->ws_path_steps, std::max<size_t>(steps_ws.size, 16));   // sets without members: nothing to trace
    if (rc) return rc;
    DeviceBuf d_packed;                                                   // the host form's result on its way out
    const size_t out_bytes = (size_t)frame_off[n_sets] * batch->src_dim * sizeof(float);
    if (!frames_on_device && out_bytes) HIP_TRY(ctx, d_packed.alloc(out_bytes));
    char *base = ctx->ws_bary.as<char>();
    std::vector<char> upload(o_contrib - o_off, 0);
    {
        uint32_t *h_off = (uint32_t *)upload.data(), *h_init = (uint32_t *)(upload.data() + (o_init - o_off));
        for (uint32_t k = 0; k <= n_sets; ++k) h_off[k] = (uint32_t)(frame_off[k] + 2ull * k);
        for (uint32_t k = 0; k < n_sets; ++k) h_init[k] = idx.pos[init[k]];
        if (!plan.desc.empty()) std::memcpy(upload.data() + (o_desc - o_off), plan.desc.data(), plan.desc.size() * sizeof(PathPair));
        if (!set_pairs.empty()) std::memcpy(upload.data() + (o_ranges - o_off), set_pairs.data(), set_pairs.size() * sizeof(uint2));
    }
    HIP_TRY(ctx, hipMemcpyAsync(base + o_off, upload.data(), upload.size(), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));                      // `upload` is a local: it must have left the host
    BaryLaunch B{};
    B.d_frames = batch->d_frames.as<float>(); B.d_seq_off = batch->d_seq_off;
    B.d_bary = (float *)(base + o_bary); B.d_bary_off = (const uint32_t *)(base + o_off);
    B.n_sets = n_sets; B.n_padded = (uint32_t)n_padded;
    B.dim = batch->dim; B.src_dim = batch->src_dim; B.dpad = batch->dpad;
    B.d_sum = (float *)(base + o_sum); B.d_cnt = (uint32_t *)(base + o_cnt);
    B.d_score_sum = (float *)(base + o_score); B.d_used = (uint32_t *)(base + o_used);
    B.d_contrib = (uint32_t *)(base + o_contrib);
    float *d_inertia = (float *)(base + o_inertia);
    uint32_t *d_used_out = (uint32_t *)(base + o_usedout);
    char *steps_base = ctx->ws_path_steps.as<char>();
    if (ctx->timing) HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    HIP_TRY(ctx, launch_bary_init(B, (const uint32_t *)(base + o_init), ctx->stream));
    for (uint32_t it = 0; it < iterations; ++it) {
        HIP_TRY(ctx, hipMemsetAsync(base + o_sum, 0, o_off - o_sum, ctx->stream));   // sums, counts, score sums, used
        for (size_t ci = 0; ci < chunks.size(); ++ci) {
            const PathChunk &c = chunks[ci];
            PathLaunch L{};
            L.d_frames = B.d_frames; L.d_seq_off = B.d_seq_off; L.dim = batch->dim; L.dpad = batch->dpad; L.band = band;
            L.d_x_frames = B.d_bary; L.d_x_seq_off = B.d_bary_off;
            L.d_pairs = (const PathPair *)(base + o_desc) + c.first;
            L.n_pairs = (uint32_t)(c.last - c.first);
            L.d_dirs = ctx->ws_path_dirs.as<uint32_t>();
            L.d_steps = (apd_path_step *)(steps_base + o_steps);
            L.d_len = (uint32_t *)(steps_base + o_len);
            L.d_scores = (float *)(steps_base + o_scores);
            HIP_TRY(ctx, launch_path_sweep(L, c.c_max, ctx->stream));
            HIP_TRY(ctx, launch_path_trace(L, ctx->stream));
            B.d_pairs = L.d_pairs; B.d_set_pairs = (const uint2 *)(base + o_ranges) + ci * n_sets;
            B.d_steps = L.d_steps; B.d_len = L.d_len; B.d_scores = L.d_scores;
            HIP_TRY(ctx, launch_bary_accumulate(B, ctx->stream));
        }
        HIP_TRY(ctx, launch_bary_finalize(B, d_inertia + (size_t)it * n_sets, d_used_out + (size_t)it * n_sets, ctx->stream));
    }
    float *d_out = frames_on_device ? frames : d_packed.as<float>();
    if (out_bytes) HIP_TRY(ctx, launch_bary_pack(B, d_out, ctx->stream));
    if (ctx->timing) { HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream)); ctx->timed = true; }
    if (!frames_on_device && out_bytes) HIP_TRY(ctx, hipMemcpyAsync(frames, d_out, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (inertia && results) HIP_TRY(ctx, hipMemcpyAsync(inertia, d_inertia, results * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (used && results) HIP_TRY(ctx, hipMemcpyAsync(used, d_used_out, results * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));                      // blocking: the results are the caller's now
    return APD_OK;
}
