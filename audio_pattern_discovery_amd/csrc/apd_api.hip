// C ABI of libapd_hip.so (include/apd.h): context, resident batches, tile sharding and the
// host-side plumbing around the alignment kernels.  No torch, no CPU fallback.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <new>

#include "apd_internal.h"

using namespace apd;

namespace {

uint32_t tiles_side(uint32_t n_seq) { return (n_seq + kTile - 1) / kTile; }

void rank_tile_list(uint32_t n_seq, uint32_t rank, uint32_t world, std::vector<uint2> &out)
{
    out.clear();
    const uint32_t side = tiles_side(n_seq);
    uint64_t g = 0;
    for (uint32_t ta = 0; ta < side; ++ta)
        for (uint32_t tb = ta; tb < side; ++tb, ++g)
            if (g % world == rank) out.push_back(make_uint2(ta, tb));
}

// apd_align_cross: the tiles of the pair matrix that hold a pair of the first resident segment (positions below seg0) with one of
// the second: the full rectangle ta in [0, ceil(seg0 / kTile)) x tb in [seg0 / kTile, ceil(n_seq / kTile)), row-major -- a tile's
// place in this list is its place in the slab.  ta <= tb throughout, so the kernels' a < b rule holds for every cross pair.
void cross_tile_list(uint32_t n_seq, uint32_t seg0, std::vector<uint2> &out)
{
    out.clear();
    if (seg0 == 0 || seg0 >= n_seq) return;
    const uint32_t side = tiles_side(n_seq), rows = tiles_side(seg0), tb0 = seg0 / kTile;
    for (uint32_t ta = 0; ta < rows; ++ta)
        for (uint32_t tb = tb0; tb < side; ++tb) out.push_back(make_uint2(ta, tb));
}

// Resident / tiling order: position p holds sequence order[p]; longest first, equal lengths by ascending index.  Pure
// function of the lengths, so every rank derives the same order.
void length_order(const uint64_t *offsets, uint32_t n_seq, std::vector<uint32_t> &order)
{
    order.resize(n_seq);
    for (uint32_t s = 0; s < n_seq; ++s) order[s] = s;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
        return offsets[a + 1] - offsets[a] > offsets[b + 1] - offsets[b];
    });
}

// cells visited by alignments.rs:174-175 for lengths (n, m) and half-width w:
// #{(i,j) in [1,n]x[1,m] : -w <= j-i <= w-1}
uint64_t tri_count(uint64_t n, uint64_t m, uint64_t k)   // #{(i,j): j - i >= k}, k >= 0
{
    if (m <= k) return 0;
    const uint64_t q = m - k, l = std::min(n, q);
    return l * q - l * (l - 1) / 2;
}
uint64_t band_cells(uint64_t n, uint64_t m, uint64_t w)
{
    return n * m - tri_count(n, m, w) - tri_count(m, n, w + 1);
}

}  // namespace

namespace apd {
thread_local const apd_context *tl_bound_context = nullptr;
bool affinity_debug()
{
    static const bool on = [] { const char *v = std::getenv("APD_DEBUG_AFFINITY"); return v && v[0] && v[0] != '0'; }();
    return on;
}
hipError_t bind_device(const apd_context *ctx)
{
    tl_bound_context = ctx;
    return hipSetDevice(ctx->device);
}
bool affinity_ok(const apd_context *ctx, const char *where)
{
    int dev = -1;
    const bool ok = tl_bound_context == ctx && hipGetDevice(&dev) == hipSuccess && dev == ctx->device;
    if (!ok) {
        const_cast<apd_context *>(ctx)->last_error = std::string("APD_DEBUG_AFFINITY: ") + where + " on a thread bound to " +
            (tl_bound_context == ctx ? "this context but HIP device " + std::to_string(dev) :
             tl_bound_context ? "another context (device " + std::to_string(tl_bound_context->device) + ")" : "no context") +
            ", expected device " + std::to_string(ctx->device);
        std::fprintf(stderr, "[apd] %s\n", ctx->last_error.c_str());
    }
    return ok;
}
}  // namespace apd

// ------------------------------------------------------------------------------------ context

extern "C" const char *apd_status_string(int s)
{
    switch (s) {
        case APD_OK: return "ok";
        case APD_ERR_INVALID_ARG: return "invalid argument";
        case APD_ERR_NO_DEVICE: return "no gfx950 HIP device";
        case APD_ERR_HIP: return "HIP runtime error";
        case APD_ERR_OOM: return "out of device memory";
        case APD_ERR_EMPTY_SEQUENCE: return "zero-length sequence (undefined in the reference, alignments.rs:120)";
        case APD_ERR_BAND_TOO_WIDE: return "warping band too wide for one wavefront";
        case APD_ERR_INDEX: return "percentile index out of range (the reference panics, numerics.rs:132)";
        case APD_ERR_UNSUPPORTED: return "unsupported";
        case APD_ERR_INCOMPLETE: return "a pair score was never written (launch cut short or skipped): NaN left in the output";
        case APD_ERR_COMM: return "RCCL error";
        default: return "unknown status";
    }
}

extern "C" int apd_create(int device, apd_context **out)
{
    if (!out) return APD_ERR_INVALID_ARG;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count) return APD_ERR_NO_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return APD_ERR_NO_DEVICE;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return APD_ERR_NO_DEVICE;   // kernels are built for gfx950 only
    apd_context *ctx = new (std::nothrow) apd_context();
    if (!ctx) return APD_ERR_OOM;
    ctx->device = device;
    if (bind_device(ctx) != hipSuccess || hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
        delete ctx;
        return APD_ERR_HIP;
    }
    ctx->own_stream = true;
    if (hipMalloc((void **)&ctx->d_status, 64) != hipSuccess || hipMemset(ctx->d_status, 0, 64) != hipSuccess) {
        hipStreamDestroy(ctx->stream);
        delete ctx;
        return APD_ERR_OOM;
    }
    hipEventCreate(&ctx->ev0);
    hipEventCreate(&ctx->ev1);
    hipEventCreateWithFlags(&ctx->fork, hipEventDisableTiming);
    for (int k = 0; k < apd_context::kSideStreams; ++k) {
        hipStreamCreateWithFlags(&ctx->side[k], hipStreamNonBlocking);
        hipEventCreateWithFlags(&ctx->side_done[k], hipEventDisableTiming);
    }
    *out = ctx;
    return APD_OK;
}

extern "C" int apd_destroy(apd_context *ctx)
{
    if (!ctx) return APD_ERR_INVALID_ARG;
    bind_device(ctx);
    hipStreamSynchronize(ctx->stream);
    if (ctx->pair_batch) { apd_batch_destroy(ctx->pair_batch); ctx->pair_batch = nullptr; }   // apd_align_pair's own (nobody else holds it)
    for (ContextChild *c : ctx->children) { c->release_device(); c->ctx = nullptr; }   // orphans: see destroy_child
    ctx->children.clear();
    for (void *p : ctx->buffers) hipFree(p);                              // apd_device_alloc'ed and never freed
    ctx->buffers.clear();
    if (ctx->d_status) hipFree(ctx->d_status);
    if (ctx->ev0) hipEventDestroy(ctx->ev0);
    if (ctx->ev1) hipEventDestroy(ctx->ev1);
    if (ctx->fork) hipEventDestroy(ctx->fork);
    for (int k = 0; k < apd_context::kSideStreams; ++k) {
        if (ctx->side[k]) { hipStreamSynchronize(ctx->side[k]); hipStreamDestroy(ctx->side[k]); }
        if (ctx->side_done[k]) hipEventDestroy(ctx->side_done[k]);
    }
    if (ctx->own_stream && ctx->stream) hipStreamDestroy(ctx->stream);
    delete ctx;                                                          // frees the workspaces: the device is still bound
    return APD_OK;
}

// The shared body of the children's destroy entry points (apd::ContextChild).
int apd::destroy_child(ContextChild *child)
{
    if (!child) return APD_ERR_INVALID_ARG;
    if (apd_context *ctx = child->ctx) {                                 // else: orphaned by apd_destroy, device side already released
        bind_device(ctx);
        hipStreamSynchronize(ctx->stream);
        child->release_device();
        ctx->children.erase(child);
    }
    delete child;
    return APD_OK;
}

extern "C" int apd_set_stream(apd_context *ctx, void *hip_stream)
{
    if (!ctx) return APD_ERR_INVALID_ARG;
    if (ctx->own_stream && ctx->stream) { hipStreamSynchronize(ctx->stream); hipStreamDestroy(ctx->stream); }
    ctx->stream = (hipStream_t)hip_stream;
    ctx->own_stream = false;
    return APD_OK;
}

// Waits for the stream and reads the sticky device status word back; a raised bit is reported once and cleared.
static int sync_and_report(apd_context *ctx)
{
    uint32_t st = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&st, ctx->d_status, sizeof(st), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (st & 1u) {
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_status, 0, sizeof(st), ctx->stream));
        ctx->last_error = "unpack met a pair score that no alignment kernel wrote (NaN poison survived): launch cut short or skipped";
        return APD_ERR_INCOMPLETE;
    }
    return APD_OK;
}

extern "C" int apd_synchronize(apd_context *ctx)
{
    if (!ctx) return APD_ERR_INVALID_ARG;
    HIP_TRY(ctx, bind_device(ctx));
    return sync_and_report(ctx);
}

extern "C" int apd_debug_affinity_probe(apd_context *bound, apd_context *checked, int *enabled)
{
    if (!bound || !checked) return APD_ERR_INVALID_ARG;
    if (enabled) *enabled = apd::affinity_debug() ? 1 : 0;
    HIP_TRY(bound, bind_device(bound));
    APD_AFFINITY(checked, "affinity probe");                              // what every allocation / event / launch in the library does
    return APD_OK;
}

extern "C" int apd_stream_busy(apd_context *ctx, int *busy)
{
    if (!ctx || !busy) return APD_ERR_INVALID_ARG;
    HIP_TRY(ctx, bind_device(ctx));
    const hipError_t e = hipStreamQuery(ctx->stream);
    if (e != hipSuccess && e != hipErrorNotReady) { ctx->last_error = std::string("hipStreamQuery: ") + hipGetErrorString(e); return APD_ERR_HIP; }
    *busy = e == hipErrorNotReady ? 1 : 0;
    return APD_OK;
}

extern "C" int apd_set_fault_injection(apd_context *ctx, uint32_t drop_tiles)
{
    if (!ctx) return APD_ERR_INVALID_ARG;
    ctx->drop_tiles = drop_tiles;
    return APD_OK;
}

extern "C" const char *apd_last_error(apd_context *ctx) { return ctx ? ctx->last_error.c_str() : "null context"; }

extern "C" int apd_set_timing(apd_context *ctx, int enabled)
{
    if (!ctx) return APD_ERR_INVALID_ARG;
    ctx->timing = enabled != 0;
    ctx->timed = false;
    return APD_OK;
}

extern "C" float apd_last_kernel_ms(apd_context *ctx)
{
    if (!ctx || !ctx->timed) return -1.0f;
    float ms = -1.0f;
    if (hipEventSynchronize(ctx->ev1) != hipSuccess) return -1.0f;
    if (hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1) != hipSuccess) return -1.0f;
    return ms;
}

extern "C" int apd_set_variant(apd_context *ctx, int variant)
{
    if (!ctx) return APD_ERR_INVALID_ARG;
    ctx->variant = variant;
    return APD_OK;
}

extern "C" int apd_set_distance_mode(apd_context *ctx, int mode, float tau)
{
    if (!ctx || mode < 0 || mode > 2 || !(tau >= 0.0f)) return APD_ERR_INVALID_ARG;
    ctx->distance_mode = mode;
    if (tau > 0.0f) ctx->tau = tau;
    return APD_OK;
}

extern "C" int apd_selftest(apd_context *ctx)
{
    if (!ctx) return APD_ERR_INVALID_ARG;
    HIP_TRY(ctx, bind_device(ctx));
    int rc = reserve_ws(ctx, ctx->ws_misc, 256);
    if (rc) return rc;
    int *d_ok = ctx->ws_misc.as<int>();
    HIP_TRY(ctx, hipMemsetAsync(d_ok, 0, sizeof(int), ctx->stream));
    HIP_TRY(ctx, launch_selftest(d_ok, ctx->stream));
    int ok = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&ok, d_ok, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (!ok) { ctx->last_error = "DPP wave_shr/wave_shl self-test failed"; return APD_ERR_HIP; }
    return APD_OK;
}

extern "C" int apd_selftest_sqrt(apd_context *ctx, uint32_t first_bits, uint64_t count, uint64_t *mismatches, uint32_t *first_mismatch,
                                 uint64_t *raw_ulp_hist)
{
    if (!ctx || !mismatches || count > (1ull << 32)) return APD_ERR_INVALID_ARG;
    HIP_TRY(ctx, bind_device(ctx));
    int rc = reserve_ws(ctx, ctx->ws_misc, 256);
    if (rc) return rc;
    unsigned long long h[7] = {0, ~0ull, 0, 0, 0, 0, 0}, *d_h = ctx->ws_misc.as<unsigned long long>();
    HIP_TRY(ctx, hipMemcpyAsync(d_h, h, sizeof(h), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));                       // h is a stack buffer
    if (count) HIP_TRY(ctx, launch_sqrt_sweep(first_bits, count, d_h, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(h, d_h, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *mismatches = h[0];
    if (first_mismatch) *first_mismatch = h[0] ? (uint32_t)(h[1] - 1ull) : 0u;
    if (raw_ulp_hist) for (int k = 0; k < 5; ++k) raw_ulp_hist[k] = h[2 + k];
    return APD_OK;
}

// --------------------------------------------------------------------- Discovery::alignment_params

extern "C" int apd_discovery_alignment_params(const apd_align_config *cfg, uint64_t n_size, apd_alignment_params *out)
{
    if (!cfg || !out) return APD_ERR_INVALID_ARG;
    const float p = cfg->warping_band_percentage * (float)n_size;        // discovery.rs:40
    uint64_t band;
    if (!(p > 0.0f)) band = 0;
    else if (p >= 18446744073709551616.0f) band = UINT64_MAX;
    else band = (uint64_t)p;
    out->warping_band = band;
    out->insertion_penalty = cfg->insertion_penalty;                     // :41
    out->match_penalty = cfg->match_penalty;                             // :42
    out->deletion_penalty = cfg->deletion_penalty;                       // :43
    return APD_OK;
}

// ------------------------------------------------------------------------------------- batch

// The resident form of a batch, described HERE and nowhere else.  Expects n_seq, dim, dpad, total_frames, order and offsets (of the
// resident order) filled in.
//   d_frames: total_frames + 2 n_seq frames of dpad floats, two sentinel frames behind every sequence (dtw_generic.hip);
//   d_meta:   one allocation filled by one copy of h_meta, [seq_off m1 | src_off m1 | order m1 | flags 4 | nmax m1] with m1 = n_seq + 1:
//             padded frame offsets; first frame of every resident sequence in the caller's frame array (`caller_offsets`; zeros without
//             one: a joined batch is never refilled); resident position -> caller's index; then what the device writes (repack
//             kernel, join): the flag words and the per-sequence norm maxima, meta_tail_words from d_flags to the end.
// The batch is registered with the context before anything is allocated: on any failure apd_batch_destroy undoes everything.
static constexpr size_t meta_tail_words(uint32_t n_seq) { return 4 + (size_t)n_seq + 1; }

static int batch_make_resident(apd_context *ctx, apd_batch *b, const uint64_t *caller_offsets)
{
    const uint32_t n_seq = b->n_seq;
    const size_t m1 = (size_t)n_seq + 1;
    b->h_meta.assign(3 * m1 + meta_tail_words(n_seq), 0u);
    uint32_t *off32 = b->h_meta.data(), *src32 = off32 + m1, *ord32 = src32 + m1;
    for (uint32_t p = 0; p < n_seq; ++p) {
        if (caller_offsets) src32[p] = (uint32_t)caller_offsets[b->order[p]];
        ord32[p] = b->order[p];
    }
    for (uint32_t p = 0; p <= n_seq; ++p) off32[p] = (uint32_t)b->offsets[p] + 2 * p;   // two sentinel frames behind every sequence
    const uint64_t padded_frames = b->total_frames + 2ull * n_seq;
    const size_t padded_bytes = std::max<size_t>((size_t)padded_frames * b->dpad * sizeof(float), 16);
    b->frames_bytes = padded_bytes < 0xFFFFFE00ull ? (uint32_t)padded_bytes : 0u;   // 4 GiB and beyond: no buffer addressing
    b->ctx = ctx;
    ctx->children.insert(b);
    const size_t meta_bytes = b->h_meta.size() * sizeof(uint32_t);
    if (b->d_frames.alloc(padded_bytes) != hipSuccess || b->d_meta.alloc(meta_bytes) != hipSuccess) return APD_ERR_OOM;
    uint32_t *d_meta = b->d_meta.as<uint32_t>();
    b->d_seq_off = d_meta; b->d_src_off = d_meta + m1; b->d_order = d_meta + 2 * m1; b->d_flags = d_meta + 3 * m1;
    b->d_seq_nmax = reinterpret_cast<float *>(b->d_flags + 4);
    if (hipMemcpyAsync(d_meta, b->h_meta.data(), meta_bytes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
        return APD_ERR_HIP;                                               // h_meta lives as long as the batch: no sync needed
    return APD_OK;
}

extern "C" int apd_batch_create(apd_context *ctx, const float *frames, const uint64_t *offsets, uint32_t n_seq,
                                uint32_t dim, int frames_on_device, apd_batch **out)
{
    if (!ctx || !offsets || !out || dim == 0 || dim > 1024) return APD_ERR_INVALID_ARG;
    *out = nullptr;
    HIP_TRY(ctx, bind_device(ctx));
    const uint64_t total = offsets[n_seq];
    if (total > 0 && !frames) return APD_ERR_INVALID_ARG;
    if (total + 2ull * n_seq >= (1ull << 32) || offsets[0] != 0) return APD_ERR_INVALID_ARG;
    apd_batch *b = new (std::nothrow) apd_batch();
    if (!b) return APD_ERR_OOM;
    // resident frames carry kernel_dim(dim) >= dim components (zero fill: distances unchanged, dtw_common.h), then the squared norm
    b->n_seq = n_seq; b->src_dim = dim; b->dim = kernel_dim(dim); b->dpad = (b->dim + 4) & ~3u; b->total_frames = total;
    b->min_len = 0xFFFFFFFFu; b->max_len = 0;
    for (uint32_t s = 0; s < n_seq; ++s) {
        if (offsets[s + 1] < offsets[s]) { delete b; return APD_ERR_INVALID_ARG; }
        const uint32_t len = (uint32_t)(offsets[s + 1] - offsets[s]);
        b->min_len = std::min(b->min_len, len);
        b->max_len = std::max(b->max_len, len);
    }
    if (n_seq == 0) b->min_len = 0;
    // Resident order: longest sequence first (length_order), so that the 16 sequences of a tile row have like lengths --
    // one kernel geometry fits the whole tile -- and the most expensive tiles of a launch start first.
    length_order(offsets, n_seq, b->order);
    b->offsets.assign(n_seq + 1, 0);                                     // offsets of the RESIDENT order
    for (uint32_t p = 0; p < n_seq; ++p) b->offsets[p + 1] = b->offsets[p] + (offsets[b->order[p] + 1] - offsets[b->order[p]]);
    int rc = batch_make_resident(ctx, b, offsets);
    if (rc == APD_OK) rc = apd_batch_refill(ctx, b, frames, frames_on_device);
    if (rc != APD_OK) { apd_batch_destroy(b); return rc; }
    *out = b;
    return APD_OK;
}

extern "C" int apd_batch_refill(apd_context *ctx, apd_batch *b, const float *frames, int frames_on_device)
{
    if (!ctx || !b || b->ctx != ctx || b->joined) return APD_ERR_INVALID_ARG;   // a joined batch is a snapshot of two others
    const uint64_t total = b->total_frames, padded_frames = total + 2ull * b->n_seq;
    if (total > 0 && !frames) return APD_ERR_INVALID_ARG;
    HIP_TRY(ctx, bind_device(ctx));
    b->nonfinite = -1;
    HIP_TRY(ctx, hipMemsetAsync(b->d_flags, 0, meta_tail_words(b->n_seq) * sizeof(uint32_t), ctx->stream));   // flags and the per-sequence norm maxima
    if (padded_frames > 0) {
        const float *d_src = frames;
        DeviceBuf tmp;                                                    // the caller's host frames on their way to the repack kernel
        const uint32_t dim = b->src_dim;
        if (!frames_on_device && total > 0) {
            const size_t bytes = (size_t)total * dim * sizeof(float);
            if (tmp.alloc(bytes) != hipSuccess) return APD_ERR_OOM;
            if (hipMemcpyAsync(tmp.ptr, frames, bytes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) return APD_ERR_HIP;
            d_src = tmp.as<float>();
        }
        hipError_t e = launch_pad(d_src, b->d_frames.as<float>(), b->d_seq_off, b->d_src_off, b->n_seq, padded_frames, dim, b->dim, b->dpad, b->d_flags, b->d_seq_nmax, ctx->stream);
        if (tmp) hipStreamSynchronize(ctx->stream);                       // the host frames and `tmp` are read until the repack is done
        if (e != hipSuccess) { ctx->last_error = hipGetErrorString(e); return APD_ERR_HIP; }
    }
    return APD_OK;
}

// The repack kernel's verdict on the frames, read back once per fill (4 bytes, one stream sync).
static int batch_nonfinite(apd_context *ctx, const apd_batch *b, bool *out)
{
    if (b->nonfinite < 0) {
        uint32_t f = 0;
        HIP_TRY(ctx, hipMemcpyAsync(&f, b->d_flags, sizeof(f), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        b->nonfinite = f ? 1 : 0;
    }
    *out = b->nonfinite == 1;
    return APD_OK;
}

extern "C" int apd_batch_nonfinite(apd_context *ctx, const apd_batch *b, int *nonfinite)
{
    if (!ctx || !b || !nonfinite || b->ctx != ctx) return APD_ERR_INVALID_ARG;
    HIP_TRY(ctx, bind_device(ctx));
    bool nf = false;
    const int rc = batch_nonfinite(ctx, b, &nf);
    *nonfinite = nf ? 1 : 0;
    return rc;
}

void apd_batch::release_device()
{
    tile_cache.clear();
    d_frames.reset();
    d_meta.reset();
    d_seq_off = nullptr; d_src_off = nullptr; d_order = nullptr; d_flags = nullptr; d_seq_nmax = nullptr;
}

extern "C" int apd_batch_destroy(apd_batch *b) { return destroy_child(b); }

extern "C" uint32_t apd_batch_len(const apd_batch *b) { return b ? b->n_seq : 0; }
extern "C" uint32_t apd_batch_first_len(const apd_batch *b) { return !b ? 0 : b->joined ? b->first_len : b->n_seq; }

extern "C" int apd_batch_join(apd_context *ctx, const apd_batch *first, const apd_batch *second, apd_batch **out)
{
    if (!ctx || !first || !second || !out) return APD_ERR_INVALID_ARG;
    *out = nullptr;
    if (first->ctx != ctx || second->ctx != ctx || first->src_dim != second->src_dim) return APD_ERR_INVALID_ARG;
    const uint64_t n_seq64 = (uint64_t)first->n_seq + second->n_seq, total = first->total_frames + second->total_frames;
    if (n_seq64 > 0xFFFFFFFFull || total + 2ull * n_seq64 >= (1ull << 32)) return APD_ERR_INVALID_ARG;
    HIP_TRY(ctx, bind_device(ctx));
    apd_batch *b = new (std::nothrow) apd_batch();
    if (!b) return APD_ERR_OOM;
    // The first resident segment: the set with the larger mean length (the first set on a tie), so that -- as in a plain batch -- the
    // column sequence a of most pairs is the longer one.  mean(first) < mean(second) without a division:
    const bool swapped = first->n_seq && second->n_seq &&
                         first->total_frames * second->n_seq < second->total_frames * first->n_seq;   // both factors below 2^32
    const apd_batch *seg[2] = {swapped ? second : first, swapped ? first : second};
    const uint32_t n_seq = (uint32_t)n_seq64, n0 = seg[0]->n_seq;
    b->n_seq = n_seq; b->src_dim = first->src_dim; b->dim = first->dim; b->dpad = first->dpad; b->total_frames = total;
    b->joined = true; b->swapped = swapped; b->first_len = first->n_seq; b->seg0 = n0;
    b->min_len = n_seq ? 0xFFFFFFFFu : 0u; b->max_len = 0;
    for (const apd_batch *s : seg)
        if (s->n_seq) { b->min_len = std::min(b->min_len, s->min_len); b->max_len = std::max(b->max_len, s->max_len); }
    // each segment keeps its own resident (length) order; the second one is rebased behind the first
    b->order.resize(n_seq);
    b->offsets.assign((size_t)n_seq + 1, 0);
    for (uint32_t p = 0; p < n_seq; ++p) {
        const int k = p < n0 ? 0 : 1;
        const uint32_t q = p - (k ? n0 : 0u);                             // position inside its segment
        const bool is_second = (k == 1) != swapped;                       // does this segment hold the caller's second set?
        b->order[p] = seg[k]->order[q] + (is_second ? first->n_seq : 0u);
        b->offsets[p + 1] = b->offsets[p] + (seg[k]->offsets[q + 1] - seg[k]->offsets[q]);
    }
    auto fail = [&](int rc) { apd_batch_destroy(b); return rc; };
    if (const int rc = batch_make_resident(ctx, b, nullptr); rc != APD_OK) return fail(rc);   // no caller array to refill from
    // frames (sentinels included) and per-sequence norm maxima: device to device, segment by segment, behind the metadata copy
    const size_t frame_bytes = (size_t)b->dpad * sizeof(float);
    const uint64_t padded0 = seg[0]->total_frames + 2ull * n0, padded_frames = total + 2ull * n_seq;
    const size_t bytes0 = (size_t)padded0 * frame_bytes, bytes1 = (size_t)(padded_frames - padded0) * frame_bytes;
    char *d_dst = b->d_frames.as<char>();
    hipError_t e = hipSuccess;
    if (bytes0) e = hipMemcpyAsync(d_dst, seg[0]->d_frames.ptr, bytes0, hipMemcpyDeviceToDevice, ctx->stream);
    if (e == hipSuccess && bytes1) e = hipMemcpyAsync(d_dst + bytes0, seg[1]->d_frames.ptr, bytes1, hipMemcpyDeviceToDevice, ctx->stream);
    if (e == hipSuccess && n0) e = hipMemcpyAsync(b->d_seq_nmax, seg[0]->d_seq_nmax, (size_t)n0 * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream);
    if (e == hipSuccess && n_seq > n0)
        e = hipMemcpyAsync(b->d_seq_nmax + n0, seg[1]->d_seq_nmax, (size_t)(n_seq - n0) * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream);
    if (e == hipSuccess) e = launch_join_flags(b->d_flags, first->d_flags, second->d_flags, ctx->stream);   // no host synchronisation
    if (e != hipSuccess) { ctx->last_error = std::string("apd_batch_join: ") + hipGetErrorString(e); return fail(APD_ERR_HIP); }
    if (first->nonfinite >= 0 && second->nonfinite >= 0) b->nonfinite = (first->nonfinite | second->nonfinite) ? 1 : 0;   // both already read back
    *out = b;
    return APD_OK;
}

// ------------------------------------------------------------------------------------- tiles

extern "C" uint32_t apd_tile_size(void) { return kTile; }

extern "C" uint64_t apd_num_tiles(uint32_t n_seq)
{
    const uint64_t side = tiles_side(n_seq);
    return side * (side + 1) / 2;
}

extern "C" uint64_t apd_rank_tiles(uint32_t n_seq, uint32_t rank, uint32_t world)
{
    if (world == 0 || rank >= world) return 0;
    const uint64_t t = apd_num_tiles(n_seq);
    return t / world + (rank < t % world ? 1 : 0);
}

extern "C" uint64_t apd_slab_floats(uint32_t n_seq, uint32_t world)
{
    if (world == 0) return 0;
    const uint64_t t = apd_num_tiles(n_seq);
    return ((t + world - 1) / world) * 2 * kSlotsPerTile;
}

extern "C" int apd_rank_tile_list(uint32_t n_seq, uint32_t rank, uint32_t world, uint32_t *tile_ab, uint64_t capacity,
                                  uint64_t *n_tiles)
{
    if (world == 0 || rank >= world || !n_tiles) return APD_ERR_INVALID_ARG;
    std::vector<uint2> tiles;
    rank_tile_list(n_seq, rank, world, tiles);
    *n_tiles = tiles.size();
    if (tile_ab) {
        if (capacity < tiles.size()) return APD_ERR_INVALID_ARG;
        for (size_t t = 0; t < tiles.size(); ++t) { tile_ab[2 * t] = tiles[t].x; tile_ab[2 * t + 1] = tiles[t].y; }
    }
    return APD_OK;
}

extern "C" int apd_length_order(const uint64_t *offsets, uint32_t n_seq, uint32_t *order)
{
    if (!offsets || (n_seq && !order)) return APD_ERR_INVALID_ARG;
    std::vector<uint32_t> o;
    length_order(offsets, n_seq, o);
    std::copy(o.begin(), o.end(), order);
    return APD_OK;
}

extern "C" int apd_unpack_tiles_host(const uint64_t *offsets, uint32_t n_seq, uint32_t world, const float *gathered, float *out)
{
    if (!offsets || world == 0 || (n_seq && (!gathered || !out))) return APD_ERR_INVALID_ARG;
    std::vector<uint32_t> order;
    length_order(offsets, n_seq, order);
    const uint64_t slab = apd_slab_floats(n_seq, world);
    std::memset(out, 0, (size_t)n_seq * n_seq * sizeof(float));                 // alignments.rs:21-23
    const uint32_t side = tiles_side(n_seq);
    uint64_t g = 0;
    for (uint32_t ta = 0; ta < side; ++ta)
        for (uint32_t tb = ta; tb < side; ++tb, ++g) {
            const float *t = gathered + (g % world) * slab + (g / world) * 2 * kSlotsPerTile;
            for (uint32_t sa = 0; sa < kTile; ++sa)
                for (uint32_t sb = 0; sb < kTile; ++sb) {
                    const uint32_t pa = ta * kTile + sa, pb = tb * kTile + sb;   // positions in the resident order
                    if (pa < pb && pb < n_seq) {
                        const uint32_t a = order[pa], b = order[pb];
                        out[(uint64_t)a * n_seq + b] = t[sa * kTile + sb];
                        out[(uint64_t)b * n_seq + a] = t[kSlotsPerTile + sa * kTile + sb];
                    }
                }
        }
    return APD_OK;
}

int check_lengths(const apd_batch *b)
{
    if (b->n_seq > 0 && b->min_len == 0) return APD_ERR_EMPTY_SEQUENCE;
    return APD_OK;
}

// Which tiles of a batch's pair matrix a call aligns, and what follows from that choice: the slab they fill and the prefix of the
// tile plan's cache key.  Kernel choice, poison, fan-out, fallback and timing are one code path for both cases.
struct TileSource {
    bool cross;             // false: rank's share (every world-th tile) of the upper triangle; true: apd_align_cross's rectangle
    uint32_t rank, world;   // cross: 0 of 1
    static TileSource triangle(uint32_t rank, uint32_t world) { return {false, rank, world}; }
    static TileSource cross_rectangle() { return {true, 0, 1}; }
    void tiles(const apd_batch &b, std::vector<uint2> &out) const
    {
        if (cross) cross_tile_list(b.n_seq, b.seg0, out);
        else rank_tile_list(b.n_seq, rank, world, out);
    }
    uint64_t num_tiles(const apd_batch &b) const                          // over all ranks
    {
        if (!cross) return apd_num_tiles(b.n_seq);
        if (b.seg0 == 0 || b.seg0 >= b.n_seq) return 0;
        return (uint64_t)tiles_side(b.seg0) * (tiles_side(b.n_seq) - b.seg0 / kTile);
    }
    uint64_t slab_floats(const apd_batch &b) const { return cross ? num_tiles(b) * 2 * kSlotsPerTile : apd_slab_floats(b.n_seq, world); }
    std::string key_prefix() const { return (cross ? "cross/" : "") + std::to_string(rank) + "/" + std::to_string(world); }
};

// The tile plan (device tile list + classes, plan_tile_classes) of one tile source.
static int build_tile_plan(apd_context *ctx, const apd_batch *batch, const BandSpec &band, const TileSource &src, bool fast_ok,
                           bool uniform_pen, bool fast_shift, apd_batch::TilePlan &plan_out)
{
    apd_batch::TilePlan plan;                                             // built locally, published only when complete
    std::vector<uint2> tiles;
    src.tiles(*batch, tiles);
    std::vector<uint4> flat;
    plan_tile_classes(batch->offsets, batch->n_seq, tiles, band, batch->dim, ctx->variant, fast_ok, uniform_pen, fast_shift,
                      plan.classes, flat);
    if (std::getenv("APD_DEBUG_PLAN"))                                  // tuning aid: which kernel geometry got how many tiles
        for (const TileClass &tc : plan.classes)
            std::fprintf(stderr, "[apd] rank %u/%u: geometry %d: %u tiles, w_max %u, n_max %u\n", src.rank, src.world, tc.geom.encode(),
                         tc.count, tc.w_max, tc.n_max);
    HIP_TRY(ctx, plan.d_tiles.alloc(std::max<size_t>(flat.size(), 1) * sizeof(uint4)));
    if (!flat.empty()) {
        hipError_t e = hipMemcpyAsync(plan.d_tiles.ptr, flat.data(), flat.size() * sizeof(uint4), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) { ctx->last_error = std::string("tile plan upload: ") + hipGetErrorString(e); return APD_ERR_HIP; }
    }
    plan_out = std::move(plan);
    return APD_OK;
}

// How one call chooses between the fast kernels and the literal one.  fast_ok: the plan may use the fast kernels; device_select:
// ... and the batch's flag decides ON THE DEVICE whether they or the literal fallback behind them run.
static int choose_align_mode(apd_context *ctx, const apd_batch *batch, const BandSpec &band, uint64_t n_tiles_all, bool &fast_ok,
                             bool &device_select)
{
    const bool pens_ok = (band.ins > 0.0f) && (band.del > 0.0f) && (band.mat > 0.0f) && (band.ins < INFINITY) &&
                         (band.del < INFINITY) && (band.mat < INFINITY);   // the systolic kernel needs pen * INF = INF
    // A feature outside the fast range anywhere in the batch (NaN, infinite, |v| >= kFeatureBound, or non-zero below kFeatureFloor)
    // means: literal kernel only (the fast kernels' selects and sentinels assume finite features, their distance forms normal
    // squared distances).  The repack kernel leaves that verdict in batch->d_flags[0]; it is consumed ON THE DEVICE: the fast
    // kernels return at once when it is set, and a fallback launch of the generic kernel over the same tiles returns at once when
    // it is clear (`device_select`).  No host round trip, nothing blocks: the call only enqueues.  The one exception: a band so
    // wide that the generic kernel cannot hold it in LDS -- then the host reads the flag (a stream synchronisation), as the fast
    // kernels are the only ones that can run.
    const bool static_fast = pens_ok && batch->frames_bytes != 0;
    bool nonfinite = false;
    device_select = false;
    if (static_fast) {
        const uint32_t band_ub = band.use_explicit ? band.explicit_band : host_band_from_pct(band.pct, batch->max_len);
        const uint32_t w_all = std::max(std::min(band_ub, batch->max_len), batch->max_len - batch->min_len) + 2;   // >= w of every pair
        device_select = generic_fallback_fits(w_all) && n_tiles_all * kSlotsPerTile <= 0xFFFFFFFFull;
        if (!device_select)
            if (const int rc = batch_nonfinite(ctx, batch, &nonfinite)) return rc;
    }
    fast_ok = static_fast && !nonfinite;
    return APD_OK;
}

// The cached plan of (tile source, band, everything the choice of kernels depends on); built on first use.
static int tile_plan(apd_context *ctx, const apd_batch *batch, const BandSpec &band, const TileSource &src, bool fast_ok,
                     const apd_batch::TilePlan **plan)
{
    // strict mode: distances computed operation for operation as numerics.rs:114-120 in every kernel family.  The band kernels
    // keep the fast select with unit penalties (it picks the reference's predecessor for every non-NaN input: dtw_systolic.h, <.., true,
    // false>) and take the literal comparison chain with any others; the strip kernels go through their literal-select path, which
    // is why `uniform_pen` is cleared here -- it steers the strip / wide families only (plan_tile_classes, dtw_generic.hip).
    const bool strict = ctx->distance_mode == 2;
    const bool uniform_pen = (band.ins == band.del) && (band.del == band.mat) && !strict;
    // the band kernel's hybrid form with unit penalties moves its column window with one DPP instruction per register at any
    // group size (dtw_systolic.h, MASKED_FETCH): 8- and 32-lane groups cost no more than 16- and 64-lane ones there
    const bool fast_shift = band.ins == 1.0f && band.del == 1.0f && band.mat == 1.0f && ctx->distance_mode == 1 && batch->dim >= 8;
    char keybuf[160];
    uint32_t pct_bits;
    std::memcpy(&pct_bits, &band.pct, sizeof(pct_bits));
    std::snprintf(keybuf, sizeof(keybuf), "%s/%08x/%u/%d/%d/%d/%d/%d", src.key_prefix().c_str(), pct_bits, band.explicit_band, band.use_explicit,
                  ctx->variant, (int)fast_ok, (int)uniform_pen, (int)fast_shift);   // everything the choice of kernels depends on
    auto cached = batch->tile_cache.find(keybuf);
    if (cached == batch->tile_cache.end()) {
        apd_batch::TilePlan fresh;
        if (const int rc = build_tile_plan(ctx, batch, band, src, fast_ok, uniform_pen, fast_shift, fresh)) return rc;
        cached = batch->tile_cache.emplace(keybuf, std::move(fresh)).first;
    }
    *plan = &cached->second;
    return APD_OK;
}

// One launch per class of the plan.  Classes are independent (disjoint tiles, disjoint slab regions): with more than one, their
// launches are spread over side streams forked from and joined back into the context's stream, so that a class of a few tiles
// does not hold the GPU alone (a ragged banded corpus splits into a dozen geometries).
static int launch_classes(apd_context *ctx, const apd_batch::TilePlan &plan, AlignLaunch L)
{
    const bool fan_out = plan.classes.size() > 1 && ctx->side[0] != nullptr;
    if (fan_out) {
        HIP_TRY(ctx, hipEventRecord(ctx->fork, ctx->stream));
        for (int k = 0; k < apd_context::kSideStreams; ++k) HIP_TRY(ctx, hipStreamWaitEvent(ctx->side[k], ctx->fork, 0));
    }
    int rc_launch = APD_OK;
    size_t ci = 0;
    for (const TileClass &tc : plan.classes) {
        L.d_tiles = plan.d_tiles.as<uint4>() + tc.first; L.n_tiles = tc.count; L.w_max = tc.w_max; L.n_max = tc.n_max;
        if (ctx->drop_tiles) L.n_tiles -= std::min(L.n_tiles, ctx->drop_tiles);   // fault injection (apd_set_fault_injection)
        int status = APD_OK;
        hipStream_t s = fan_out ? ctx->side[ci++ % apd_context::kSideStreams] : ctx->stream;
        hipError_t e = launch_align(L, tc.geom, s, ctx->last_error, &status);
        if (e != hipSuccess) { ctx->last_error = std::string("launch_align: ") + hipGetErrorString(e); rc_launch = APD_ERR_HIP; break; }
        if (status != APD_OK) { rc_launch = status; break; }
    }
    if (fan_out)                                                        // always join, also after a failed launch
        for (int k = 0; k < apd_context::kSideStreams; ++k) {
            HIP_TRY(ctx, hipEventRecord(ctx->side_done[k], ctx->side[k]));
            HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->side_done[k], 0));
        }
    return rc_launch;
}

// The literal kernel behind the fast ones (device_select), idle unless the flag is raised -- over the classes a FAST kernel took (a
// class that already runs the literal kernel, geometry 0, ignores the flag and must not be aligned twice); neighbouring classes
// are contiguous in the tile list and share a launch.
static int launch_literal_fallback(apd_context *ctx, const apd_batch::TilePlan &plan, AlignLaunch L)
{
    size_t k = 0;
    while (k < plan.classes.size()) {
        if (plan.classes[k].geom.family == KernelGeom::Generic) { ++k; continue; }
        uint32_t first = plan.classes[k].first, total = 0, w_max = 0, n_max = 0;
        for (; k < plan.classes.size() && plan.classes[k].geom.family != KernelGeom::Generic && plan.classes[k].first == first + total; ++k) {
            total += plan.classes[k].count; w_max = std::max(w_max, plan.classes[k].w_max); n_max = std::max(n_max, plan.classes[k].n_max);
        }
        L.d_tiles = plan.d_tiles.as<uint4>() + first; L.n_tiles = total; L.w_max = w_max; L.n_max = n_max;
        if (ctx->drop_tiles) L.n_tiles -= std::min(L.n_tiles, ctx->drop_tiles);
        bool fits = true;
        const hipError_t e = launch_generic_fallback(L, ctx->stream, &fits);
        if (e != hipSuccess || !fits) { ctx->last_error = std::string("launch_generic_fallback: ") + (fits ? hipGetErrorString(e) : "band too wide"); return APD_ERR_HIP; }
    }
    return APD_OK;
}

static int align_tiles_impl(apd_context *ctx, const apd_batch *batch, const BandSpec &band, const TileSource &src, float *d_slab)
{
    if (!ctx || !batch || !d_slab || src.world == 0 || src.rank >= src.world || batch->ctx != ctx) return APD_ERR_INVALID_ARG;
    if (src.cross && !batch->joined) return APD_ERR_INVALID_ARG;
    int rc = check_lengths(batch);
    if (rc) return rc;
    HIP_TRY(ctx, bind_device(ctx));
    bool fast_ok = false, device_select = false;
    rc = choose_align_mode(ctx, batch, band, src.num_tiles(*batch), fast_ok, device_select);
    if (rc) return rc;
    const apd_batch::TilePlan *plan = nullptr;
    rc = tile_plan(ctx, batch, band, src, fast_ok, &plan);
    if (rc) return rc;
    // A class of the literal kernel whose band does not fit its LDS rows: refused here, before the poison memset -- the call has
    // enqueued nothing and written nothing when APD_ERR_BAND_TOO_WIDE comes back (launch_align keeps the same test)
    for (const TileClass &tc : plan->classes)
        if (tc.geom.family == KernelGeom::Generic && tc.count != 0 && !generic_band_fits(tc.w_max)) {
            ctx->last_error = "band too wide for the generic kernel";
            return APD_ERR_BAND_TOO_WIDE;
        }
    // Poison: every score slot of the rank's slab starts as NaN, so a pair that no kernel writes (a launch cut short, a
    // skipped class) reaches the matrix as NaN and raises APD_ERR_INCOMPLETE in the unpack -- never a stale or zero distance.
    APD_AFFINITY(ctx, "alignment launches");
    HIP_TRY(ctx, hipMemsetAsync(d_slab, 0xFF, src.slab_floats(*batch) * sizeof(float), ctx->stream));
    AlignLaunch L{};
    L.d_frames = batch->d_frames.as<float>(); L.frames_bytes = batch->frames_bytes; L.d_seq_off = batch->d_seq_off; L.d_seq_nmax = batch->d_seq_nmax;
    L.n_seq = batch->n_seq; L.dim = batch->dim; L.dpad = batch->dpad; L.band = band; L.d_slab = d_slab;
    L.variant = ctx->variant;
    L.hybrid = ctx->distance_mode == 1; L.strict = ctx->distance_mode == 2; L.tau = ctx->tau;
    L.d_nonfinite = device_select ? batch->d_flags : nullptr;
    if (ctx->timing) HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    rc = launch_classes(ctx, *plan, L);
    if (rc == APD_OK && device_select) rc = launch_literal_fallback(ctx, *plan, L);
    if (rc) return rc;
    if (ctx->timing) { HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream)); ctx->timed = true; }
    return APD_OK;
}

// Any f32 penalty is accepted (include/apd.h, "the domain of an alignment configuration").  A NaN penalty reaches the kernels as
// THE canonical quiet NaN: its payload would otherwise travel into the scores, where the pattern 0xFFFFFFFF means "never written"
// (is_poison, dtw_generic.hip).  Which scores are NaN does not depend on the payload.
static float canonical_penalty(float p) { return p != p ? std::numeric_limits<float>::quiet_NaN() : p; }

BandSpec band_from_cfg(const apd_align_config *cfg)
{
    BandSpec b{};
    b.pct = cfg->warping_band_percentage; b.use_explicit = 0; b.explicit_band = 0;
    b.ins = canonical_penalty(cfg->insertion_penalty); b.del = canonical_penalty(cfg->deletion_penalty);
    b.mat = canonical_penalty(cfg->match_penalty);
    return b;
}

extern "C" int apd_align_tiles_async(apd_context *ctx, const apd_batch *batch, const apd_align_config *cfg,
                                     uint32_t rank, uint32_t world, float *d_slab)
{
    if (!cfg) return APD_ERR_INVALID_ARG;
    return align_tiles_impl(ctx, batch, band_from_cfg(cfg), TileSource::triangle(rank, world), d_slab);
}

extern "C" int apd_unpack_tiles_async(apd_context *ctx, const apd_batch *batch, uint32_t world, const float *d_gathered,
                                      float *d_out)
{
    if (!ctx || !batch || batch->ctx != ctx || !d_gathered || !d_out || world == 0) return APD_ERR_INVALID_ARG;
    const uint32_t n_seq = batch->n_seq;
    HIP_TRY(ctx, bind_device(ctx));
    APD_AFFINITY(ctx, "unpack launch");
    // the unpack writes every entry, the zero diagonal (alignments.rs:21-23) included; anything it fails to write stays NaN
    HIP_TRY(ctx, hipMemsetAsync(d_out, 0xFF, (size_t)n_seq * n_seq * sizeof(float), ctx->stream));
    HIP_TRY(ctx, launch_unpack(d_gathered, d_out, batch->d_order, n_seq, world, apd_slab_floats(n_seq, world), batch->d_flags,
                               ctx->d_status, ctx->stream));
    return APD_OK;
}

static int align_all_device_impl(apd_context *ctx, const apd_batch *batch, const BandSpec &band, float *d_out)
{
    if (!ctx || !batch || !d_out) return APD_ERR_INVALID_ARG;
    const size_t slab_bytes = std::max<size_t>(apd_slab_floats(batch->n_seq, 1) * sizeof(float), 16);
    int rc = reserve_ws(ctx, ctx->ws_slab, slab_bytes);
    if (rc) return rc;
    rc = align_tiles_impl(ctx, batch, band, TileSource::triangle(0, 1), ctx->ws_slab.as<float>());
    if (rc) return rc;
    return apd_unpack_tiles_async(ctx, batch, 1, ctx->ws_slab.as<float>(), d_out);
}

// The end of a blocking entry point: given the status of what was enqueued so far, the copies of the results to the host (entries
// without a destination are skipped), then the wait and the device's verdict (sync_and_report).
struct ReadBack { void *dst; const void *d_src; size_t bytes; };
static int read_back(apd_context *ctx, int rc, std::initializer_list<ReadBack> copies)
{
    if (rc != APD_OK) return rc;
    for (const ReadBack &c : copies) {
        if (!c.dst) continue;
        const hipError_t e = hipMemcpyAsync(c.dst, c.d_src, c.bytes, hipMemcpyDeviceToHost, ctx->stream);
        if (e != hipSuccess) { ctx->last_error = hipGetErrorString(e); return APD_ERR_HIP; }
    }
    return sync_and_report(ctx);                                          // APD_ERR_INCOMPLETE: the outputs hold NaN where no score was written
}

extern "C" int apd_align_all_device_async(apd_context *ctx, const apd_batch *batch, const apd_align_config *cfg,
                                          float *d_out)
{
    if (!cfg) return APD_ERR_INVALID_ARG;
    return align_all_device_impl(ctx, batch, band_from_cfg(cfg), d_out);
}

extern "C" int apd_align_all(apd_context *ctx, const apd_batch *batch, const apd_align_config *cfg, float *out)
{
    if (!ctx || !batch || !cfg || (!out && batch->n_seq)) return APD_ERR_INVALID_ARG;
    if (batch->n_seq == 0) return APD_OK;
    HIP_TRY(ctx, bind_device(ctx));
    const size_t bytes = (size_t)batch->n_seq * batch->n_seq * sizeof(float);
    DeviceBuf d_out;
    HIP_TRY(ctx, d_out.alloc(bytes));
    const int rc = align_all_device_impl(ctx, batch, band_from_cfg(cfg), d_out.as<float>());
    return read_back(ctx, rc, {{out, d_out.ptr, bytes}});
}

// ------------------------------------------------------------------------------ cross alignment

static int align_cross_device_impl(apd_context *ctx, const apd_batch *batch, const BandSpec &band, float *d_fs, float *d_sf)
{
    const uint32_t n_first = batch->first_len, n_second = batch->n_seq - n_first;
    const TileSource src = TileSource::cross_rectangle();
    int rc = reserve_ws(ctx, ctx->ws_slab, std::max<size_t>(src.slab_floats(*batch) * sizeof(float), 16));
    if (rc) return rc;
    rc = align_tiles_impl(ctx, batch, band, src, ctx->ws_slab.as<float>());
    if (rc) return rc;
    APD_AFFINITY(ctx, "unpack launch");
    // the unpack writes every entry; anything it fails to write stays NaN
    const size_t out_bytes = (size_t)n_first * n_second * sizeof(float);
    if (d_fs) HIP_TRY(ctx, hipMemsetAsync(d_fs, 0xFF, out_bytes, ctx->stream));
    if (d_sf) HIP_TRY(ctx, hipMemsetAsync(d_sf, 0xFF, out_bytes, ctx->stream));
    HIP_TRY(ctx, launch_unpack_cross(ctx->ws_slab.as<float>(), d_fs, d_sf, batch->d_order, batch->n_seq, batch->seg0, n_first,
                                     batch->swapped, batch->d_flags, ctx->d_status, ctx->stream));
    return APD_OK;
}

extern "C" int apd_align_cross_device_async(apd_context *ctx, const apd_batch *batch, const apd_align_config *cfg, float *d_out_fs,
                                            float *d_out_sf)
{
    if (!ctx || !batch || !cfg || batch->ctx != ctx || !batch->joined) return APD_ERR_INVALID_ARG;
    if (batch->first_len == 0 || batch->first_len == batch->n_seq) return APD_OK;   // an empty set: nothing to write
    if (!d_out_fs && !d_out_sf) return APD_ERR_INVALID_ARG;
    HIP_TRY(ctx, bind_device(ctx));
    return align_cross_device_impl(ctx, batch, band_from_cfg(cfg), d_out_fs, d_out_sf);
}

extern "C" int apd_align_cross(apd_context *ctx, const apd_batch *batch, const apd_align_config *cfg, float *out_fs, float *out_sf)
{
    if (!ctx || !batch || !cfg || batch->ctx != ctx || !batch->joined) return APD_ERR_INVALID_ARG;
    if (batch->first_len == 0 || batch->first_len == batch->n_seq) return APD_OK;
    if (!out_fs && !out_sf) return APD_ERR_INVALID_ARG;
    HIP_TRY(ctx, bind_device(ctx));
    const size_t bytes = (size_t)batch->first_len * (batch->n_seq - batch->first_len) * sizeof(float);
    DeviceBuf d_out;                                                      // [fs | sf]
    HIP_TRY(ctx, d_out.alloc(2 * bytes));
    float *d_fs = out_fs ? d_out.as<float>() : nullptr, *d_sf = out_sf ? d_out.as<float>() + bytes / sizeof(float) : nullptr;
    const int rc = align_cross_device_impl(ctx, batch, band_from_cfg(cfg), d_fs, d_sf);
    return read_back(ctx, rc, {{out_fs, d_fs, bytes}, {out_sf, d_sf, bytes}});
}

// Linkage of the first set to clusters of the second (kernels: clustering.hip).  Workspace (ws_linkage, owned by the context so that
// the device form only enqueues): [members | set_off | link fs, sf].
extern "C" int apd_cross_linkage(apd_context *ctx, const float *fs, const float *sf, int on_device, uint32_t n_first, uint32_t n_second,
                                 const uint32_t *members, const uint32_t *set_off, uint32_t n_sets, float *link_fs, float *link_sf,
                                 uint32_t *nearest, float *nearest_linkage)
{
    if (!ctx || (n_sets && !set_off)) return APD_ERR_INVALID_ARG;
    const uint32_t n_members = n_sets ? set_off[n_sets] : 0u;
    if (n_sets && set_off[0] != 0) return APD_ERR_INVALID_ARG;
    for (uint32_t k = 0; k < n_sets; ++k) if (set_off[k + 1] < set_off[k]) return APD_ERR_INVALID_ARG;
    if (n_members && !members) return APD_ERR_INVALID_ARG;
    for (uint32_t t = 0; t < n_members; ++t) if (members[t] >= n_second) return APD_ERR_INVALID_ARG;
    if (n_first && (!nearest || !nearest_linkage || (n_members && (!fs || !sf)))) return APD_ERR_INVALID_ARG;
    if (n_first == 0) return APD_OK;
    HIP_TRY(ctx, bind_device(ctx));
    // ascending sequence number inside every set: the order the reference's loops over 0..n visit the members in
    std::vector<uint32_t> stage(members, members + n_members);
    for (uint32_t k = 0; k < n_sets; ++k) std::sort(stage.begin() + set_off[k], stage.begin() + set_off[k + 1]);
    stage.insert(stage.end(), set_off, set_off + (n_sets ? n_sets + 1 : 0));
    if (n_sets == 0) stage.push_back(0u);
    const size_t meta_bytes = (stage.size() * sizeof(uint32_t) + 255) & ~(size_t)255;
    const size_t link_floats = (size_t)n_first * n_sets, mat_bytes = (size_t)n_first * n_second * sizeof(float);
    const size_t res_bytes = (size_t)n_first * 8;                          // host form: [nearest | nearest_linkage]
    size_t need = meta_bytes + 2 * link_floats * sizeof(float);
    const size_t in_off = (need + 255) & ~(size_t)255;
    if (!on_device) need = in_off + 2 * mat_bytes + res_bytes;
    int rc = reserve_ws(ctx, ctx->ws_linkage, std::max<size_t>(need, 256));
    if (rc) return rc;
    char *base = ctx->ws_linkage.as<char>();
    uint32_t *d_members = (uint32_t *)base, *d_set_off = d_members + n_members;
    float *d_link = (float *)(base + meta_bytes);
    HIP_TRY(ctx, hipMemcpyAsync(d_members, stage.data(), stage.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    const float *d_fs = fs, *d_sf = sf;
    uint32_t *d_nearest = nearest;
    float *d_nl = nearest_linkage;
    if (!on_device) {
        float *in = (float *)(base + in_off);
        if (mat_bytes && fs) HIP_TRY(ctx, hipMemcpyAsync(in, fs, mat_bytes, hipMemcpyHostToDevice, ctx->stream));
        if (mat_bytes && sf) HIP_TRY(ctx, hipMemcpyAsync(in + mat_bytes / sizeof(float), sf, mat_bytes, hipMemcpyHostToDevice, ctx->stream));
        d_fs = in; d_sf = in + mat_bytes / sizeof(float);
        d_nearest = (uint32_t *)(base + in_off + 2 * mat_bytes);
        d_nl = (float *)(d_nearest + n_first);
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));                      // `stage` is a local: its upload must have left the host
    APD_AFFINITY(ctx, "linkage launch");
    HIP_TRY(ctx, launch_cross_linkage(d_fs, d_sf, n_first, n_second, d_members, d_set_off, n_sets, d_link, d_nearest, d_nl, ctx->stream));
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (link_fs && link_floats) HIP_TRY(ctx, hipMemcpyAsync(link_fs, d_link, link_floats * sizeof(float), kind, ctx->stream));
    if (link_sf && link_floats) HIP_TRY(ctx, hipMemcpyAsync(link_sf, d_link + link_floats, link_floats * sizeof(float), kind, ctx->stream));
    if (!on_device) {
        HIP_TRY(ctx, hipMemcpyAsync(nearest, d_nearest, (size_t)n_first * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(nearest_linkage, d_nl, (size_t)n_first * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    return APD_OK;
}

int prepare_pair_batch(apd_context *ctx, const float *x, uint64_t n, const float *y, uint64_t m, uint32_t dim)
{
    std::vector<float> frames((n + m) * (size_t)dim);
    std::memcpy(frames.data(), x, n * (size_t)dim * sizeof(float));
    std::memcpy(frames.data() + n * (size_t)dim, y, m * (size_t)dim * sizeof(float));
    const uint64_t offsets[3] = {0, n, n + m};
    // A host that loops over Alignment::construct_alignment (alignments.rs:165) mostly aligns pairs of the SAME lengths (fixed
    // windows): the context keeps the last pair's two-sequence batch and refills it (no allocation, no plan rebuild) when the next
    // pair has the same (n, m, dim); any other shape replaces it.
    int rc = APD_OK;
    if (ctx->pair_batch && (ctx->pair_n != n || ctx->pair_m != m || ctx->pair_dim != dim)) { apd_batch_destroy(ctx->pair_batch); ctx->pair_batch = nullptr; }
    if (!ctx->pair_batch) {
        rc = apd_batch_create(ctx, frames.data(), offsets, 2, dim, 0, &ctx->pair_batch);
        if (rc) { ctx->pair_batch = nullptr; return rc; }
        ctx->pair_n = n; ctx->pair_m = m; ctx->pair_dim = dim;
    } else {
        rc = apd_batch_refill(ctx, ctx->pair_batch, frames.data(), 0);   // host frames: the refill has consumed them when it returns
        if (rc) return rc;
    }
    return APD_OK;
}

BandSpec band_from_params(const apd_alignment_params *params)
{
    BandSpec band{};
    band.use_explicit = 1;
    band.explicit_band = params->warping_band > 0xFFFFFFF0ull ? 0xFFFFFFF0u : (uint32_t)params->warping_band;
    band.ins = canonical_penalty(params->insertion_penalty); band.del = canonical_penalty(params->deletion_penalty);
    band.mat = canonical_penalty(params->match_penalty);
    return band;
}

extern "C" int apd_align_pair(apd_context *ctx, const float *x, uint64_t n, const float *y, uint64_t m, uint32_t dim,
                              const apd_alignment_params *params, float *score)
{
    if (!ctx || !params || !score || dim == 0) return APD_ERR_INVALID_ARG;
    if (n == 0 && m == 0) { *score = INFINITY; return APD_OK; }           // alignments.rs:117-118
    if (n == 0 || m == 0) return APD_ERR_EMPTY_SEQUENCE;                  // usize underflow at :120
    if (!x || !y) return APD_ERR_INVALID_ARG;
    int rc = prepare_pair_batch(ctx, x, n, y, m, dim);
    if (rc) return rc;
    apd_batch *b = ctx->pair_batch;
    const BandSpec band = band_from_params(params);
    rc = reserve_ws(ctx, ctx->ws_misc, 256);
    if (rc) return rc;
    float *d_out = ctx->ws_misc.as<float>();
    float host[4] = {0, 0, 0, 0};
    rc = read_back(ctx, align_all_device_impl(ctx, b, band, d_out), {{host, d_out, sizeof(host)}});
    if (rc == APD_OK) *score = host[1];                                   // out[0*2+1] = score(x, y)
    return rc;
}

// ------------------------------------------------------------------------------- work accounting

extern "C" int apd_align_work(const uint64_t *offsets, uint32_t n_seq, uint32_t dim, const apd_align_config *cfg,
                              uint32_t rank, uint32_t world, uint64_t *pairs, uint64_t *cells, uint64_t *alg_bytes)
{
    if (!offsets || !cfg || world == 0 || rank >= world) return APD_ERR_INVALID_ARG;
    const BandSpec band = band_from_cfg(cfg);
    std::vector<uint2> tiles;
    rank_tile_list(n_seq, rank, world, tiles);
    std::vector<uint32_t> order;
    length_order(offsets, n_seq, order);                                  // tiles are cut from the resident order
    uint64_t np = 0, nc = 0, nb = 0;
    for (const uint2 &t : tiles)
        for (uint32_t sa = 0; sa < kTile; ++sa)
            for (uint32_t sb = 0; sb < kTile; ++sb) {
                const uint32_t pa = t.x * kTile + sa, pb = t.y * kTile + sb;
                if (!(pa < pb && pb < n_seq)) continue;
                const uint32_t a = order[pa], b = order[pb];
                const uint64_t n = offsets[a + 1] - offsets[a], m = offsets[b + 1] - offsets[b];
                if (n == 0 || m == 0) return APD_ERR_EMPTY_SEQUENCE;
                const uint64_t mx = std::max(n, m), gap = mx - std::min(n, m);
                uint64_t bnd = host_band_from_pct(band.pct, (uint32_t)mx);
                const uint64_t w = std::max(bnd, gap) + 2;                // alignments.rs:173 (unclamped: same cell set)
                np += 2;                                                  // both ordered pairs (alignments.rs:50-51)
                nc += band_cells(n, m, w) + band_cells(m, n, w);
                nb += 2 * (4ull * dim * (n + m) + 4);
            }
    if (pairs) *pairs = np;
    if (cells) *cells = nc;
    if (alg_bytes) *alg_bytes = nb;
    return APD_OK;
}

// ------------------------------------------------------------------------------- device buffers

extern "C" int apd_device_alloc(apd_context *ctx, uint64_t bytes, void **d_ptr)
{
    if (!ctx || !d_ptr) return APD_ERR_INVALID_ARG;
    *d_ptr = nullptr;
    HIP_TRY(ctx, bind_device(ctx));
    HIP_TRY(ctx, hipMalloc(d_ptr, std::max<size_t>((size_t)bytes, 16)));
    ctx->buffers.insert(*d_ptr);
    return APD_OK;
}

extern "C" int apd_device_free(apd_context *ctx, void *d_ptr)
{
    if (!ctx) return APD_ERR_INVALID_ARG;
    if (!d_ptr) return APD_OK;
    HIP_TRY(ctx, bind_device(ctx));
    if (ctx->buffers.erase(d_ptr) == 0) return APD_ERR_INVALID_ARG;       // not a buffer of this context (or freed twice)
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));                      // nothing queued may still use it
    HIP_TRY(ctx, hipFree(d_ptr));
    return APD_OK;
}

extern "C" int apd_copy_to_device(apd_context *ctx, void *d_dst, const void *src, uint64_t bytes)
{
    if (!ctx || (bytes && (!d_dst || !src))) return APD_ERR_INVALID_ARG;
    if (bytes == 0) return APD_OK;
    HIP_TRY(ctx, bind_device(ctx));
    HIP_TRY(ctx, hipMemcpyAsync(d_dst, src, (size_t)bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return APD_OK;
}

extern "C" int apd_copy_to_host(apd_context *ctx, void *dst, const void *d_src, uint64_t bytes)
{
    if (!ctx || (bytes && (!dst || !d_src))) return APD_ERR_INVALID_ARG;
    if (bytes == 0) return APD_OK;
    HIP_TRY(ctx, bind_device(ctx));
    HIP_TRY(ctx, hipMemcpyAsync(dst, d_src, (size_t)bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return APD_OK;
}

extern "C" int apd_device_fill(apd_context *ctx, void *d_dst, int byte_value, uint64_t bytes)
{
    if (!ctx || (bytes && !d_dst)) return APD_ERR_INVALID_ARG;
    if (bytes == 0) return APD_OK;
    HIP_TRY(ctx, bind_device(ctx));
    HIP_TRY(ctx, hipMemsetAsync(d_dst, byte_value, (size_t)bytes, ctx->stream));
    return APD_OK;
}
