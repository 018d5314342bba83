// C ABI of libapd_hip.so (include/apd.h): context, resident batches, tile sharding and the
// host-side plumbing around the alignment kernels.  No torch, no CPU fallback.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <new>
#include <tuple>

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

static int check_lengths(const apd_batch *b)
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

static BandSpec band_from_cfg(const apd_align_config *cfg)
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

// The context's two-sequence batch holding (x, y): sequence 0 = x, sequence 1 = y.
static int prepare_pair_batch(apd_context *ctx, const float *x, uint64_t n, const float *y, uint64_t m, uint32_t dim)
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

static BandSpec band_from_params(const apd_alignment_params *params)
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

// --------------------------------------------------------------------------------- warping paths

extern "C" uint64_t apd_path_bound(uint64_t n, uint64_t m) { return (n == 0 || m == 0) ? 0 : n + m - 1; }

// Cap of the direction workspace of one chunk of pairs (bytes); also bounds the chunk's step buffer.
static uint64_t path_workspace_cap()
{
    if (const char *v = std::getenv("APD_PATH_WORKSPACE_BYTES")) {
        const unsigned long long b = std::strtoull(v, nullptr, 10);
        if (b > 0) return b;
    }
    return 1ull << 30;
}

// The sweep and the trace (dtw_path.hip) over `pairs`, in chunks whose direction words stay under the cap.
static int align_paths_impl(apd_context *ctx, const apd_batch *batch, const BandSpec &band, const uint32_t *pairs, uint64_t n_pairs,
                            apd_path_step *steps, uint64_t capacity, uint64_t *step_off, uint32_t *path_len, float *scores)
{
    if (!ctx || !batch || batch->ctx != ctx || !step_off || (n_pairs && !pairs)) return APD_ERR_INVALID_ARG;
    const uint32_t n_seq = batch->n_seq;
    std::vector<uint32_t> pos(n_seq);                                     // caller's sequence number -> resident position
    for (uint32_t p = 0; p < n_seq; ++p) pos[batch->order[p]] = p;
    auto len_of = [&](uint32_t s) { return (uint32_t)(batch->offsets[pos[s] + 1] - batch->offsets[pos[s]]); };
    for (uint64_t p = 0; p < n_pairs; ++p)
        if (pairs[2 * p] >= n_seq || pairs[2 * p + 1] >= n_seq) return APD_ERR_INVALID_ARG;
    int rc = check_lengths(batch);
    if (rc) return rc;
    step_off[0] = 0;
    for (uint64_t p = 0; p < n_pairs; ++p) step_off[p + 1] = step_off[p] + apd_path_bound(len_of(pairs[2 * p]), len_of(pairs[2 * p + 1]));
    if (!steps) return APD_OK;                                            // sizes only
    if (capacity < step_off[n_pairs] || (n_pairs && !path_len)) return APD_ERR_INVALID_ARG;
    if (n_pairs == 0) return APD_OK;
    std::vector<PathPair> desc(n_pairs);
    std::vector<uint64_t> dir_words(n_pairs);
    std::vector<uint32_t> cells(n_pairs);
    for (uint64_t p = 0; p < n_pairs; ++p) {
        const uint32_t n = len_of(pairs[2 * p]), m = len_of(pairs[2 * p + 1]);
        const uint32_t w = host_w(band, n, m);
        if (2ull * w + 1 > kPathMaxOffsets) { ctx->last_error = "band too wide for the path sweep"; return APD_ERR_BAND_TOO_WIDE; }
        desc[p].px = pos[pairs[2 * p]];
        desc[p].py = pos[pairs[2 * p + 1]];
        dir_words[p] = path_dir_words(n, m, w);
        cells[p] = path_cells_per_lane(w);
    }
    HIP_TRY(ctx, bind_device(ctx));
    APD_AFFINITY(ctx, "path launch");
    const uint64_t cap = path_workspace_cap();
    constexpr uint64_t kMaxPairsPerLaunch = 1ull << 24;                   // 64 work-items per pair, launches stay below 2^31
    std::vector<float> score_sink;
    if (!scores) score_sink.resize(n_pairs);
    float *h_scores = scores ? scores : score_sink.data();
    bool first_chunk = true;
    for (uint64_t first = 0; first < n_pairs;) {
        // the chunk [first, last): at least one pair, then as many as keep the direction words and the steps under the cap
        uint64_t last = first, words = 0, slots = 0;
        uint32_t c_max = 2;
        while (last < n_pairs && last - first < kMaxPairsPerLaunch) {
            const uint64_t nw = words + dir_words[last], ns = slots + (step_off[last + 1] - step_off[last]);
            if (last > first && (nw * sizeof(uint32_t) > cap || ns * sizeof(apd_path_step) > cap)) break;
            desc[last].dir_off = words;
            desc[last].step_off = slots;
            words = nw; slots = ns;
            c_max = std::max(c_max, cells[last]);
            ++last;
        }
        const uint64_t np = last - first;
        // steps workspace: [steps | pair descriptors | lengths | scores]
        const size_t steps_bytes = (size_t)slots * sizeof(apd_path_step), desc_bytes = (size_t)np * sizeof(PathPair);
        rc = reserve_ws(ctx, ctx->ws_path_dirs, std::max<size_t>((size_t)words * sizeof(uint32_t), 16));
        if (rc) return rc;
        rc = reserve_ws(ctx, ctx->ws_path_steps, steps_bytes + desc_bytes + (size_t)np * 8 + 16);
        if (rc) return rc;
        char *base = ctx->ws_path_steps.as<char>();
        PathLaunch L{};
        L.d_frames = batch->d_frames.as<float>(); L.d_seq_off = batch->d_seq_off; L.dim = batch->dim; L.dpad = batch->dpad; L.band = band;
        L.d_pairs = (const PathPair *)(base + steps_bytes);
        L.n_pairs = (uint32_t)np;
        L.d_dirs = ctx->ws_path_dirs.as<uint32_t>();
        L.d_steps = (apd_path_step *)base;
        L.d_len = (uint32_t *)(base + steps_bytes + desc_bytes);
        L.d_scores = (float *)(base + steps_bytes + desc_bytes + (size_t)np * 4);
        HIP_TRY(ctx, hipMemcpyAsync((void *)L.d_pairs, desc.data() + first, desc_bytes, hipMemcpyHostToDevice, ctx->stream));
        if (ctx->timing && first_chunk) HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
        HIP_TRY(ctx, launch_path_sweep(L, c_max, ctx->stream));
        HIP_TRY(ctx, launch_path_trace(L, ctx->stream));
        if (ctx->timing && last == n_pairs) { HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream)); ctx->timed = true; }
        if (slots) HIP_TRY(ctx, hipMemcpyAsync(steps + step_off[first], L.d_steps, steps_bytes, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(path_len + first, L.d_len, (size_t)np * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(h_scores + first, L.d_scores, (size_t)np * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));                  // the next chunk reuses the workspaces
        first = last;
        first_chunk = false;
    }
    return APD_OK;
}

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

// DBA over sets of a resident batch (kernels: dtw_path.hip).  The pairs (set, member ascending) are cut into chunks under the path
// workspace cap once; every iteration runs sweep, trace and accumulate per chunk, then one finalize.  ws_bary, uploaded once:
// [barycenters | sums | counts | score sums | used | bary_off | init positions | pair descriptors | per chunk: pairs of every set |
//  contributes | inertia, used of every iteration].
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
    std::vector<uint32_t> pos(n_seq);                                     // caller's sequence number -> resident position
    for (uint32_t p = 0; p < n_seq; ++p) pos[batch->order[p]] = p;
    auto len_of = [&](uint32_t s) { return (uint32_t)(batch->offsets[pos[s] + 1] - batch->offsets[pos[s]]); };
    auto frames_of = [&](uint32_t k) { return set_off[k + 1] > set_off[k] ? len_of(init[k]) : 0u; };   // an empty set has no barycenter
    frame_off[0] = 0;
    for (uint32_t k = 0; k < n_sets; ++k) frame_off[k + 1] = frame_off[k] + frames_of(k);
    if (!frames) return APD_OK;                                           // sizes only
    if (capacity < frame_off[n_sets]) return APD_ERR_INVALID_ARG;
    const BandSpec band = band_from_cfg(cfg);
    const uint64_t n_padded = frame_off[n_sets] + 2ull * n_sets;
    if (n_padded >= (1ull << 32) || n_padded * batch->dpad >= (1ull << 39)) return APD_ERR_INVALID_ARG;   // one work-item per float, below 2^31 workgroups

    // ---- the plan: pair descriptors, chunks, and per chunk the pairs of every set
    struct Chunk { uint32_t first, last, c_max; uint64_t words, slots; };
    std::vector<PathPair> desc(n_pairs);
    std::vector<Chunk> chunks;
    const uint64_t cap = path_workspace_cap();
    constexpr uint32_t kMaxPairsPerLaunch = 1u << 24;                     // 64 work-items per pair, launches stay below 2^31
    {
        std::vector<uint32_t> set_of(n_pairs);
        for (uint32_t k = 0; k < n_sets; ++k) for (uint32_t t = set_off[k]; t < set_off[k + 1]; ++t) set_of[t] = k;
        Chunk c{0, 0, 2, 0, 0};
        for (uint32_t p = 0; p < n_pairs; ++p) {
            const uint32_t n = frames_of(set_of[p]), m = len_of(sorted[p]);
            const uint32_t w = host_w(band, n, m);
            if (2ull * w + 1 > kPathMaxOffsets) { ctx->last_error = "band too wide for the path sweep"; return APD_ERR_BAND_TOO_WIDE; }
            const uint64_t words = path_dir_words(n, m, w), slots = apd_path_bound(n, m);
            if (p > c.first && ((c.words + words) * sizeof(uint32_t) > cap || (c.slots + slots) * sizeof(apd_path_step) > cap ||
                                p - c.first >= kMaxPairsPerLaunch)) {
                c.last = p;
                chunks.push_back(c);
                c = Chunk{p, 0, 2, 0, 0};
            }
            desc[p] = PathPair{set_of[p], pos[sorted[p]], c.words, c.slots};   // px: the set, whose barycenter is x
            c.words += words; c.slots += slots;
            c.c_max = std::max(c.c_max, path_cells_per_lane(w));
        }
        if (n_pairs) { c.last = n_pairs; chunks.push_back(c); }
    }
    std::vector<uint2> set_pairs(chunks.size() * n_sets);                 // per chunk and set: its pairs [x, y), relative to the chunk
    uint64_t max_words = 0, max_slots = 0;
    uint32_t max_np = 0;
    for (size_t ci = 0; ci < chunks.size(); ++ci) {
        const Chunk &c = chunks[ci];
        for (uint32_t k = 0; k < n_sets; ++k) {
            const uint32_t lo = std::min(std::max(set_off[k], c.first), c.last), hi = std::min(std::max(set_off[k + 1], c.first), c.last);
            set_pairs[ci * n_sets + k] = make_uint2(lo - c.first, hi - c.first);
        }
        max_words = std::max(max_words, c.words); max_slots = std::max(max_slots, c.slots); max_np = std::max(max_np, c.last - c.first);
    }
    if (n_sets == 0) return APD_OK;

    // ---- device state
    HIP_TRY(ctx, bind_device(ctx));
    APD_AFFINITY(ctx, "barycenter launch");
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t bary_bytes = up((size_t)n_padded * batch->dpad * sizeof(float)), cnt_bytes = up((size_t)n_padded * 4);
    const size_t set_bytes = up((size_t)n_sets * 4), off_bytes = up(((size_t)n_sets + 1) * 4);
    const size_t desc_bytes = up(desc.size() * sizeof(PathPair)), ranges_bytes = up(set_pairs.size() * sizeof(uint2));
    const size_t contrib_bytes = up((size_t)max_np * 4), result_bytes = up((size_t)iterations * n_sets * 4);
    // [bary | sum | cnt | score_sum | used] then the uploaded block [bary_off | init_pos | desc | ranges] then [contrib | inertia | used_out]
    const size_t o_sum = bary_bytes, o_cnt = o_sum + bary_bytes, o_score = o_cnt + cnt_bytes, o_used = o_score + set_bytes;
    const size_t o_off = o_used + set_bytes, o_init = o_off + off_bytes, o_desc = o_init + set_bytes, o_ranges = o_desc + desc_bytes;
    const size_t o_contrib = o_ranges + ranges_bytes, o_inertia = o_contrib + contrib_bytes, o_usedout = o_inertia + result_bytes;
    rc = reserve_ws(ctx, ctx->ws_bary, o_usedout + result_bytes);
    if (rc) return rc;
    rc = reserve_ws(ctx, ctx->ws_path_dirs, std::max<size_t>((size_t)max_words * sizeof(uint32_t), 16));
    if (rc) return rc;
    // steps workspace, as apd_align_paths lays it out: [steps | lengths | scores] (the descriptors live in ws_bary)
    const size_t steps_bytes = (size_t)max_slots * sizeof(apd_path_step);
    rc = reserve_ws(ctx, ctx->ws_path_steps, steps_bytes + (size_t)max_np * 8 + 16);
    if (rc) return rc;
    DeviceBuf d_packed;                                                   // the host form's result on its way out
    const size_t out_bytes = (size_t)frame_off[n_sets] * batch->src_dim * sizeof(float);
    if (!frames_on_device && out_bytes) HIP_TRY(ctx, d_packed.alloc(out_bytes));
    char *base = ctx->ws_bary.as<char>();
    std::vector<char> upload(o_contrib - o_off, 0);
    {
        uint32_t *h_off = (uint32_t *)upload.data(), *h_init = (uint32_t *)(upload.data() + (o_init - o_off));
        for (uint32_t k = 0; k <= n_sets; ++k) h_off[k] = (uint32_t)(frame_off[k] + 2ull * k);
        for (uint32_t k = 0; k < n_sets; ++k) h_init[k] = pos[init[k]];
        if (!desc.empty()) std::memcpy(upload.data() + (o_desc - o_off), desc.data(), desc.size() * sizeof(PathPair));
        if (!set_pairs.empty()) std::memcpy(upload.data() + (o_ranges - o_off), set_pairs.data(), set_pairs.size() * sizeof(uint2));
    }
    HIP_TRY(ctx, hipMemcpyAsync(base + o_off, upload.data(), upload.size(), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));                      // `upload` is a local: it must have left the host
    BaryLaunch B{};
    B.d_frames = batch->d_frames.as<float>(); B.d_seq_off = batch->d_seq_off;
    B.d_bary = (float *)base; B.d_bary_off = (const uint32_t *)(base + o_off);
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
            const Chunk &c = chunks[ci];
            const uint32_t np = c.last - c.first;
            PathLaunch L{};
            L.d_frames = B.d_frames; L.d_seq_off = B.d_seq_off; L.dim = batch->dim; L.dpad = batch->dpad; L.band = band;
            L.d_x_frames = B.d_bary; L.d_x_seq_off = B.d_bary_off;
            L.d_pairs = (const PathPair *)(base + o_desc) + c.first;
            L.n_pairs = np;
            L.d_dirs = ctx->ws_path_dirs.as<uint32_t>();
            L.d_steps = (apd_path_step *)steps_base;
            L.d_len = (uint32_t *)(steps_base + steps_bytes);
            L.d_scores = (float *)(steps_base + steps_bytes + (size_t)max_np * 4);
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
    const size_t res = (size_t)iterations * n_sets * 4;
    if (!frames_on_device && out_bytes) HIP_TRY(ctx, hipMemcpyAsync(frames, d_out, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (inertia && res) HIP_TRY(ctx, hipMemcpyAsync(inertia, d_inertia, res, hipMemcpyDeviceToHost, ctx->stream));
    if (used && res) HIP_TRY(ctx, hipMemcpyAsync(used, d_used_out, res, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));                      // blocking: the results are the caller's now
    return APD_OK;
}

// ------------------------------------------------------------------------- subsequence alignment

// Cap of the device curves of one chunk of pairs (bytes).
static uint64_t spot_workspace_cap()
{
    if (const char *v = std::getenv("APD_SPOT_WORKSPACE_BYTES")) {
        const unsigned long long b = std::strtoull(v, nullptr, 10);
        if (b > 0) return b;
    }
    return 1ull << 30;
}

extern "C" int apd_spot(apd_context *ctx, const apd_batch *batch, const apd_align_config *cfg, const uint32_t *pairs, uint64_t n_pairs,
                        float *cost, uint32_t *start, uint64_t capacity, uint64_t *curve_off, apd_spot_best *best)
{
    if (!ctx || !batch || !cfg || batch->ctx != ctx || !curve_off || (n_pairs && !pairs)) return APD_ERR_INVALID_ARG;
    if ((cost == nullptr) != (start == nullptr)) return APD_ERR_INVALID_ARG;
    const uint32_t n_seq = batch->n_seq;
    std::vector<uint32_t> pos(n_seq);                                     // caller's sequence number -> resident position
    for (uint32_t p = 0; p < n_seq; ++p) pos[batch->order[p]] = p;
    auto len_of = [&](uint32_t s) { return (uint32_t)(batch->offsets[pos[s] + 1] - batch->offsets[pos[s]]); };
    for (uint64_t p = 0; p < n_pairs; ++p)
        if (pairs[2 * p] >= n_seq || pairs[2 * p + 1] >= n_seq) return APD_ERR_INVALID_ARG;
    int rc = check_lengths(batch);
    if (rc) return rc;
    curve_off[0] = 0;
    for (uint64_t p = 0; p < n_pairs; ++p) curve_off[p + 1] = curve_off[p] + len_of(pairs[2 * p + 1]);
    const bool curves = cost != nullptr;
    if (!curves && !best) return APD_OK;                                  // sizes only
    if (curves && capacity < curve_off[n_pairs]) return APD_ERR_INVALID_ARG;
    if (n_pairs == 0) return APD_OK;
    for (uint64_t p = 0; p < n_pairs; ++p)
        if (len_of(pairs[2 * p]) > kSpotMaxQuery || len_of(pairs[2 * p + 1]) >= kSpotMaxStream) {
            ctx->last_error = "apd_spot: a query of more than " + std::to_string(kSpotMaxQuery) + " frames";
            return APD_ERR_UNSUPPORTED;
        }
    HIP_TRY(ctx, bind_device(ctx));
    APD_AFFINITY(ctx, "spot launch");
    const uint64_t cap = spot_workspace_cap();
    constexpr uint64_t kMaxPairsPerLaunch = 1ull << 24;                   // 64 work-items per pair, launches stay below 2^31
    constexpr uint32_t kClasses = kSpotRegisterRows + 1;                  // spot_row_class
    std::vector<apd_spot_best> best_sink;
    if (!best) best_sink.resize(n_pairs);
    apd_spot_best *h_best = best ? best : best_sink.data();
    std::vector<SpotPair> desc;
    bool first_chunk = true;
    for (uint64_t first = 0; first < n_pairs;) {
        // the chunk [first, last): at least one pair, then as many as keep the curves under the cap
        uint64_t last = first, entries = 0;
        while (last < n_pairs && last - first < kMaxPairsPerLaunch) {
            const uint64_t ne = entries + (curve_off[last + 1] - curve_off[last]);
            if (curves && last > first && ne * (sizeof(float) + sizeof(uint32_t)) > cap) break;
            entries = ne;
            ++last;
        }
        const uint64_t np = last - first;
        // the chunk's descriptors, grouped by kernel class (one launch each); `out` keeps the input order
        uint64_t class_count[kClasses] = {}, class_first[kClasses] = {};
        uint32_t r_max = 1;
        for (uint64_t p = first; p < last; ++p) {
            const uint32_t n = len_of(pairs[2 * p]);
            const uint32_t c = spot_row_class(batch->dim, n);
            ++class_count[c];
            if (c == 0) r_max = std::max(r_max, spot_rows_per_lane(n));
        }
        for (uint32_t c = 1; c < kClasses; ++c) class_first[c] = class_first[c - 1] + class_count[c - 1];
        desc.resize(np);
        uint64_t fill[kClasses];
        std::copy(class_first, class_first + kClasses, fill);
        for (uint64_t p = first; p < last; ++p) {
            SpotPair &d = desc[fill[spot_row_class(batch->dim, len_of(pairs[2 * p]))]++];
            d.px = pos[pairs[2 * p]];
            d.py = pos[pairs[2 * p + 1]];
            d.out = (uint32_t)(p - first);
            d.pad = 0;
            d.curve_off = curve_off[p] - curve_off[first];
        }
        // workspace: [cost | start | pair descriptors | best]
        const size_t curve_floats = curves ? (size_t)entries : 0;
        const size_t curve_bytes = (curve_floats * 4 + 15) / 16 * 16;
        const size_t desc_bytes = (size_t)np * sizeof(SpotPair), best_bytes = (size_t)np * sizeof(apd_spot_best);
        rc = reserve_ws(ctx, ctx->ws_spot, 2 * curve_bytes + desc_bytes + best_bytes + 16);
        if (rc) return rc;
        char *base = ctx->ws_spot.as<char>();
        SpotLaunch L{};
        L.d_frames = batch->d_frames.as<float>(); L.d_seq_off = batch->d_seq_off; L.dim = batch->dim; L.dpad = batch->dpad;
        L.ins = cfg->insertion_penalty; L.del = cfg->deletion_penalty; L.mat = cfg->match_penalty;
        L.d_cost = curves ? (float *)base : nullptr;
        L.d_start = curves ? (uint32_t *)(base + curve_bytes) : nullptr;
        const SpotPair *d_desc = (const SpotPair *)(base + 2 * curve_bytes);
        L.d_best = (apd_spot_best *)(base + 2 * curve_bytes + desc_bytes);
        HIP_TRY(ctx, hipMemcpyAsync((void *)d_desc, desc.data(), desc_bytes, hipMemcpyHostToDevice, ctx->stream));
        if (ctx->timing && first_chunk) HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
        for (uint32_t c = 0; c < kClasses; ++c) {
            L.d_pairs = d_desc + class_first[c];
            L.n_pairs = (uint32_t)class_count[c];
            HIP_TRY(ctx, launch_spot(L, c, r_max, ctx->stream));
        }
        if (ctx->timing && last == n_pairs) { HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream)); ctx->timed = true; }
        if (curve_floats) {
            HIP_TRY(ctx, hipMemcpyAsync(cost + curve_off[first], L.d_cost, curve_floats * 4, hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipMemcpyAsync(start + curve_off[first], L.d_start, curve_floats * 4, hipMemcpyDeviceToHost, ctx->stream));
        }
        HIP_TRY(ctx, hipMemcpyAsync(h_best + first, L.d_best, best_bytes, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));                  // the next chunk reuses the workspace (and `desc`)
        first = last;
        first_chunk = false;
    }
    return APD_OK;
}

// score(j) of the spotting contract: one f32 division, the window's length in place of m (alignments.rs:121)
static float spot_score(float cost, uint64_t j, uint32_t start, uint64_t n)
{
    return cost / (float)(n + (j - start + 1));
}

extern "C" int apd_spot_hits(const float *cost, const uint32_t *start, uint64_t m, uint64_t n, float threshold, apd_spot_best *hits,
                             uint64_t capacity, uint64_t *n_hits)
{
    if (!n_hits || n == 0 || (m && (!cost || !start)) || (capacity && !hits)) return APD_ERR_INVALID_ARG;
    *n_hits = 0;
    try {
        std::vector<std::pair<float, uint64_t>> cand;                     // (score, end), ends ascending
        for (uint64_t j = 1; j <= m; ++j) {
            if (start[j - 1] > j) return APD_ERR_INVALID_ARG;             // not a curve of apd_spot
            const float s = spot_score(cost[j - 1], j, start[j - 1], n);
            if (s < threshold) cand.emplace_back(s, j);                   // strict; NaN compares false
        }
        std::stable_sort(cand.begin(), cand.end(), [](const auto &a, const auto &b) { return a.first < b.first; });
        std::map<uint64_t, uint64_t> taken;                               // accepted windows, first column -> last column (disjoint)
        for (const auto &c : cand) {
            const uint64_t hi = c.second, lo = start[hi - 1];
            auto next = taken.upper_bound(hi);                            // the first accepted window that begins after `hi`
            if (next != taken.begin() && std::prev(next)->second >= lo) continue;   // the one before it reaches into [lo, hi]
            taken.emplace(lo, hi);
            if (*n_hits < capacity) {
                apd_spot_best &h = hits[*n_hits];
                h.end = (uint32_t)hi; h.start = (uint32_t)lo; h.cost = cost[hi - 1]; h.score = c.first;
            }
            ++*n_hits;
        }
    } catch (const std::bad_alloc &) {
        return APD_ERR_OOM;
    }
    return APD_OK;
}

// ----------------------------------------------------------------------------------------- spot detection

// apd_spot's sweep into the workspace, then candidates, greedy picking and the packed hits on the device (kernels:
// dtw_spot_detect.hip).  A chunk is a run of whole groups; its pairs are numbered group by group.
// ws_spot: [cost | start | candidates | accepted windows | sweep pairs, detect pairs, groups (uploaded) | best | candidate counts,
// hit counts (zeroed) | hit bases]; ws_spot_hits: the chunk's packed hits, sized once its hit counts are known.
extern "C" int apd_spot_detect(apd_context *ctx, const apd_batch *batch, const apd_align_config *cfg, const uint32_t *pairs, uint64_t n_pairs,
                               const float *thresholds, int compete, apd_spot_hit *hits, uint64_t capacity, uint64_t *hit_off,
                               uint64_t *n_groups, uint64_t *n_hits)
{
    if (!ctx || !batch || !cfg || batch->ctx != ctx || (n_pairs && !pairs)) return APD_ERR_INVALID_ARG;
    if ((compete != APD_DETECT_PER_PAIR && compete != APD_DETECT_PER_STREAM) || (n_pairs && !thresholds) || !hit_off || !n_groups || !n_hits ||
        (capacity && !hits))
        return APD_ERR_INVALID_ARG;
    const uint32_t n_seq = batch->n_seq;
    std::vector<uint32_t> pos(n_seq);                                     // caller's sequence number -> resident position
    for (uint32_t p = 0; p < n_seq; ++p) pos[batch->order[p]] = p;
    auto len_of = [&](uint32_t s) { return (uint32_t)(batch->offsets[pos[s] + 1] - batch->offsets[pos[s]]); };
    for (uint64_t p = 0; p < n_pairs; ++p)
        if (pairs[2 * p] >= n_seq || pairs[2 * p + 1] >= n_seq) return APD_ERR_INVALID_ARG;
    int rc = check_lengths(batch);
    if (rc) return rc;
    *n_groups = 0;
    *n_hits = 0;
    hit_off[0] = 0;
    if (n_pairs == 0) return APD_OK;
    for (uint64_t p = 0; p < n_pairs; ++p)
        if (len_of(pairs[2 * p]) > kSpotMaxQuery || len_of(pairs[2 * p + 1]) >= kSpotMaxStream) {
            ctx->last_error = "apd_spot_detect: a query of more than " + std::to_string(kSpotMaxQuery) + " frames";
            return APD_ERR_UNSUPPORTED;
        }
    constexpr uint64_t kMaxPairsPerLaunch = 1ull << 24;                   // as apd_spot
    // groups in order of first appearance; members[member_first[g] .. member_first[g + 1]): the group's pairs, ascending
    std::vector<uint64_t> group_of(n_pairs), member_first, members(n_pairs);
    uint64_t ng = 0;
    if (compete == APD_DETECT_PER_PAIR) {
        ng = n_pairs;
        for (uint64_t p = 0; p < n_pairs; ++p) group_of[p] = p;
    } else {
        std::vector<uint64_t> group_of_stream(n_seq, ~0ull);
        for (uint64_t p = 0; p < n_pairs; ++p) {
            uint64_t &g = group_of_stream[pairs[2 * p + 1]];
            if (g == ~0ull) g = ng++;
            group_of[p] = g;
        }
    }
    member_first.assign(ng + 1, 0);
    for (uint64_t p = 0; p < n_pairs; ++p) ++member_first[group_of[p] + 1];
    for (uint64_t g = 0; g < ng; ++g) {
        if (member_first[g + 1] > kMaxPairsPerLaunch) {
            ctx->last_error = "apd_spot_detect: a group of more than 2^24 pairs";
            return APD_ERR_UNSUPPORTED;
        }
        member_first[g + 1] += member_first[g];
    }
    {
        std::vector<uint64_t> fill(member_first.begin(), member_first.end() - 1);
        for (uint64_t p = 0; p < n_pairs; ++p) members[fill[group_of[p]]++] = p;
    }
    auto stream_len = [&](uint64_t g) { return (uint64_t)len_of(pairs[2 * members[member_first[g]] + 1]); };
    auto group_pairs = [&](uint64_t g) { return member_first[g + 1] - member_first[g]; };
    *n_groups = ng;
    HIP_TRY(ctx, bind_device(ctx));
    APD_AFFINITY(ctx, "spot detect launch");
    const uint64_t cap = spot_workspace_cap();
    constexpr uint32_t kClasses = kSpotRegisterRows + 1;                  // spot_row_class
    constexpr uint64_t kEntryBytes = sizeof(float) + sizeof(uint32_t) + sizeof(ulonglong2), kStageBytes = sizeof(uint2);
    auto pad16 = [](size_t b) { return (b + 15) / 16 * 16; };
    std::vector<char> upload;
    std::vector<uint32_t> counts;
    bool first_chunk = true;
    for (uint64_t g0 = 0; g0 < ng;) {
        // the chunk of groups [g0, g1): at least one, then as many as keep the curves, the candidates and the windows under the cap
        uint64_t g1 = g0, entries = 0, stage_slots = 0, np = 0;
        while (g1 < ng) {
            const uint64_t ne = entries + group_pairs(g1) * stream_len(g1), ns = stage_slots + stream_len(g1);
            if (g1 > g0 && (ne * kEntryBytes + ns * kStageBytes > cap || np + group_pairs(g1) > kMaxPairsPerLaunch)) break;
            entries = ne; stage_slots = ns; np += group_pairs(g1);
            ++g1;
        }
        const uint64_t ngc = g1 - g0;
        // what is uploaded: [sweep pairs by kernel class | detect pairs | groups]
        const size_t desc_bytes = pad16((size_t)np * sizeof(SpotPair)), dp_bytes = (size_t)np * sizeof(SpotDetectPair);
        const size_t grp_bytes = (size_t)ngc * sizeof(SpotDetectGroup);
        upload.assign(desc_bytes + dp_bytes + grp_bytes, 0);
        SpotPair *desc = (SpotPair *)upload.data();
        SpotDetectPair *dp = (SpotDetectPair *)(upload.data() + desc_bytes);
        SpotDetectGroup *grp = (SpotDetectGroup *)(upload.data() + desc_bytes + dp_bytes);
        uint64_t class_count[kClasses] = {}, class_first[kClasses] = {};
        uint32_t r_max = 1, m_max = 1;
        uint64_t k = 0, off = 0, stage_off = 0;
        for (uint64_t g = g0; g < g1; ++g) {
            SpotDetectGroup &G = grp[g - g0];
            const uint32_t m = (uint32_t)stream_len(g);
            G.cand_off = off; G.cand_cap = group_pairs(g) * m; G.stage_off = stage_off; G.stage_cap = m;
            stage_off += m;
            m_max = std::max(m_max, m);
            for (uint64_t t = member_first[g]; t < member_first[g + 1]; ++t, ++k) {
                const uint64_t p = members[t];
                SpotDetectPair &d = dp[k];
                d.curve_off = off; d.m = m; d.n = len_of(pairs[2 * p]); d.threshold = thresholds[p];
                d.group = (uint32_t)(g - g0); d.pair = (uint32_t)p;
                off += m;
                const uint32_t c = spot_row_class(batch->dim, d.n);
                ++class_count[c];
                if (c == 0) r_max = std::max(r_max, spot_rows_per_lane(d.n));
            }
        }
        for (uint32_t c = 1; c < kClasses; ++c) class_first[c] = class_first[c - 1] + class_count[c - 1];
        uint64_t fill[kClasses];
        std::copy(class_first, class_first + kClasses, fill);
        for (k = 0; k < np; ++k) {
            const uint64_t p = dp[k].pair;
            SpotPair &d = desc[fill[spot_row_class(batch->dim, dp[k].n)]++];
            d.px = pos[pairs[2 * p]];
            d.py = pos[pairs[2 * p + 1]];
            d.out = (uint32_t)k;
            d.pad = 0;
            d.curve_off = dp[k].curve_off;
        }
        const size_t curve_bytes = pad16((size_t)entries * 4), cand_bytes = (size_t)entries * sizeof(ulonglong2);
        const size_t stage_bytes = pad16((size_t)stage_slots * sizeof(uint2)), best_bytes = (size_t)np * sizeof(apd_spot_best);
        const size_t cc_bytes = (size_t)ngc * sizeof(unsigned long long), hc_bytes = pad16((size_t)ngc * sizeof(uint32_t));
        const size_t hb_bytes = (size_t)(ngc + 1) * sizeof(unsigned long long);
        rc = reserve_ws(ctx, ctx->ws_spot, 2 * curve_bytes + cand_bytes + stage_bytes + upload.size() + best_bytes + cc_bytes + hc_bytes + hb_bytes + 16);
        if (rc) return rc;
        char *base = ctx->ws_spot.as<char>();
        char *d_upload = base + 2 * curve_bytes + cand_bytes + stage_bytes, *d_counts = d_upload + upload.size() + best_bytes;
        SpotLaunch L{};
        L.d_frames = batch->d_frames.as<float>(); L.d_seq_off = batch->d_seq_off; L.dim = batch->dim; L.dpad = batch->dpad;
        L.ins = cfg->insertion_penalty; L.del = cfg->deletion_penalty; L.mat = cfg->match_penalty;
        L.d_cost = (float *)base;
        L.d_start = (uint32_t *)(base + curve_bytes);
        const SpotPair *d_desc = (const SpotPair *)d_upload;
        L.d_best = (apd_spot_best *)(d_upload + upload.size());
        SpotDetectLaunch D{};
        D.d_cost = L.d_cost; D.d_start = L.d_start;
        D.d_pairs = (const SpotDetectPair *)(d_upload + desc_bytes); D.n_pairs = (uint32_t)np;
        D.d_groups = (const SpotDetectGroup *)(d_upload + desc_bytes + dp_bytes); D.n_groups = (uint32_t)ngc;
        D.d_cand = (ulonglong2 *)(base + 2 * curve_bytes);
        D.d_stage = (uint2 *)(base + 2 * curve_bytes + cand_bytes);
        D.d_cand_count = (unsigned long long *)d_counts;
        D.d_hit_count = (uint32_t *)(d_counts + cc_bytes);
        D.d_hit_base = (unsigned long long *)(d_counts + cc_bytes + hc_bytes);
        HIP_TRY(ctx, hipMemcpyAsync(d_upload, upload.data(), upload.size(), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(d_counts, 0, cc_bytes + hc_bytes, ctx->stream));
        if (ctx->timing && first_chunk) HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
        for (uint32_t c = 0; c < kClasses; ++c) {
            L.d_pairs = d_desc + class_first[c];
            L.n_pairs = (uint32_t)class_count[c];
            HIP_TRY(ctx, launch_spot(L, c, r_max, ctx->stream));
        }
        HIP_TRY(ctx, launch_spot_detect(D, m_max, ctx->stream));
        counts.resize(ngc);
        HIP_TRY(ctx, hipMemcpyAsync(counts.data(), D.d_hit_count, (size_t)ngc * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));                  // the packed buffer is sized by the counts
        const uint64_t chunk_first = hit_off[g0];
        for (uint64_t g = g0; g < g1; ++g) hit_off[g + 1] = hit_off[g] + counts[g - g0];
        const uint64_t chunk_hits = hit_off[g1] - chunk_first;
        const uint64_t n_write = capacity > chunk_first ? std::min(chunk_hits, capacity - chunk_first) : 0;
        if (n_write) {
            rc = reserve_ws(ctx, ctx->ws_spot_hits, (size_t)n_write * sizeof(apd_spot_hit));
            if (rc) return rc;
            HIP_TRY(ctx, launch_spot_detect_emit(D, ctx->ws_spot_hits.as<apd_spot_hit>(), n_write, ctx->stream));
        }
        if (ctx->timing && g1 == ng) { HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream)); ctx->timed = true; }
        if (n_write) {
            HIP_TRY(ctx, hipMemcpyAsync(hits + chunk_first, ctx->ws_spot_hits.ptr, (size_t)n_write * sizeof(apd_spot_hit), hipMemcpyDeviceToHost,
                                        ctx->stream));
        }
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));                  // the next chunk reuses the workspace (and `upload`)
        g0 = g1;
        first_chunk = false;
    }
    *n_hits = hit_off[ng];
    return APD_OK;
}

// ------------------------------------------------------------------- warping paths of spotted windows

extern "C" uint64_t apd_spot_path_bound(uint64_t n, uint64_t end, uint64_t start)
{
    return (n == 0 || start == 0 || start > end) ? 0 : n + (end - start + 1);
}

// The windows are taken in input order, a chunk at a time: as many as keep the direction words (counted per window, before the
// merge makes them fewer) and the steps under the workspace cap, at least one.  Inside a chunk the windows are grouped by (query,
// stream) pair: one sweep per pair over the union of its windows' columns, one trace per window (kernels: dtw_spot_path.hip).
// ws_spot_steps: [steps | pairs | intervals | windows | ends] (all but the steps uploaded), then [end cost | end start | lengths |
// found | scores]; ws_spot_dirs: the intervals' words.
extern "C" int apd_spot_paths(apd_context *ctx, const apd_batch *batch, const apd_align_config *cfg, const apd_spot_window *windows,
                              uint64_t n_windows, apd_path_step *steps, uint64_t capacity, uint64_t *step_off, uint32_t *path_len,
                              uint32_t *found_start, float *scores)
{
    if (!ctx || !batch || !cfg || batch->ctx != ctx || !step_off || (n_windows && !windows)) return APD_ERR_INVALID_ARG;
    const uint32_t n_seq = batch->n_seq;
    std::vector<uint32_t> pos(n_seq);                                     // caller's sequence number -> resident position
    for (uint32_t p = 0; p < n_seq; ++p) pos[batch->order[p]] = p;
    auto len_of = [&](uint32_t s) { return (uint32_t)(batch->offsets[pos[s] + 1] - batch->offsets[pos[s]]); };
    for (uint64_t p = 0; p < n_windows; ++p)
        if (windows[p].x >= n_seq || windows[p].y >= n_seq) return APD_ERR_INVALID_ARG;
    int rc = check_lengths(batch);
    if (rc) return rc;
    for (uint64_t p = 0; p < n_windows; ++p) {
        const apd_spot_window &w = windows[p];
        if (w.end > len_of(w.y) || (w.end && w.start > w.end)) return APD_ERR_INVALID_ARG;
    }
    auto slots_of = [&](uint64_t p) { return apd_spot_path_bound(len_of(windows[p].x), windows[p].end, windows[p].start); };
    step_off[0] = 0;
    for (uint64_t p = 0; p < n_windows; ++p) step_off[p + 1] = step_off[p] + slots_of(p);
    if (!steps) return APD_OK;                                            // sizes only
    if (capacity < step_off[n_windows] || (n_windows && !path_len)) return APD_ERR_INVALID_ARG;
    if (n_windows == 0) return APD_OK;
    for (uint64_t p = 0; p < n_windows; ++p)
        if (len_of(windows[p].x) > kSpotMaxQuery || len_of(windows[p].y) >= kSpotMaxStream) {
            ctx->last_error = "apd_spot_paths: a query of more than " + std::to_string(kSpotMaxQuery) + " frames";
            return APD_ERR_UNSUPPORTED;
        }
    HIP_TRY(ctx, bind_device(ctx));
    APD_AFFINITY(ctx, "spot path launch");
    const uint64_t cap = spot_workspace_cap();
    constexpr uint64_t kMaxWindowsPerLaunch = 1ull << 24;                 // 64 work-items per window, launches stay below 2^31
    constexpr uint32_t kClasses = kSpotRegisterRows + 1;                  // spot_row_class
    auto up16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
    std::vector<uint64_t> live;                                           // the chunk's windows that own slots, input order
    std::vector<uint64_t> by_pair;                                        // the same, grouped by pair, starts ascending
    std::vector<SpotRecPair> rec_pairs[kClasses];
    std::vector<SpotInterval> intervals;
    std::vector<uint32_t> ends;
    std::vector<SpotTraceWindow> trace;
    std::vector<char> upload;
    std::vector<uint32_t> h_len, h_found;
    std::vector<float> h_scores;
    bool first_launch = true;
    for (uint64_t first = 0; first < n_windows;) {
        uint64_t last = first, est_words = 0;
        while (last < n_windows && last - first < kMaxWindowsPerLaunch) {
            const apd_spot_window &w = windows[last];
            const uint64_t slots = step_off[last + 1] - step_off[last];
            const uint64_t nw = est_words + (slots ? spot_dir_words(len_of(w.x), (uint64_t)w.end - w.start + 1) : 0);
            if (last > first && (nw * sizeof(uint32_t) > cap || (step_off[last + 1] - step_off[first]) * sizeof(apd_path_step) > cap)) break;
            est_words = nw;
            ++last;
        }
        live.clear();
        for (uint64_t p = first; p < last; ++p) {
            if (step_off[p + 1] > step_off[p]) { live.push_back(p); continue; }
            path_len[p] = 0;                                              // no window: nothing to sweep
            if (found_start) found_start[p] = 0;
            if (scores) scores[p] = INFINITY;
        }
        if (live.empty()) { first = last; continue; }
        // ---- the plan: per pair its merged intervals and its distinct ends; per window its interval and its end's slot
        by_pair = live;
        std::sort(by_pair.begin(), by_pair.end(), [&](uint64_t a, uint64_t b) {
            const apd_spot_window &u = windows[a], &v = windows[b];
            return std::make_tuple(u.x, u.y, u.start, u.end, a) < std::make_tuple(v.x, v.y, v.start, v.end, b);
        });
        for (auto &v : rec_pairs) v.clear();
        intervals.clear(); ends.clear();
        trace.assign(live.size(), SpotTraceWindow{});
        uint64_t words = 0;
        uint32_t r_max = 1;
        for (size_t g = 0; g < by_pair.size();) {
            size_t g_end = g;
            const apd_spot_window &head = windows[by_pair[g]];
            while (g_end < by_pair.size() && windows[by_pair[g_end]].x == head.x && windows[by_pair[g_end]].y == head.y) ++g_end;
            const uint32_t n = len_of(head.x), c = spot_row_class(batch->dim, n);
            if (c == 0) r_max = std::max(r_max, spot_rows_per_lane(n));
            SpotRecPair rp{};
            rp.px = pos[head.x]; rp.py = pos[head.y];
            rp.iv_first = (uint32_t)intervals.size(); rp.end_first = (uint32_t)ends.size();
            for (size_t t = g; t < g_end; ++t) {
                const apd_spot_window &w = windows[by_pair[t]];
                if (intervals.size() > rp.iv_first && (uint64_t)w.start <= (uint64_t)intervals.back().b + 1)
                    intervals.back().b = std::max(intervals.back().b, w.end);   // overlapping or touching: one interval
                else
                    intervals.push_back(SpotInterval{w.start, w.end, 0});
                ends.push_back(w.end);
                rp.max_end = std::max(rp.max_end, w.end);
            }
            std::sort(ends.begin() + rp.end_first, ends.end());
            ends.erase(std::unique(ends.begin() + rp.end_first, ends.end()), ends.end());
            rp.n_iv = (uint32_t)intervals.size() - rp.iv_first; rp.n_ends = (uint32_t)ends.size() - rp.end_first;
            for (uint32_t k = rp.iv_first; k < intervals.size(); ++k) {
                intervals[k].off = words;
                words += spot_dir_words(n, (uint64_t)intervals[k].b - intervals[k].a + 1);
            }
            for (size_t t = g; t < g_end; ++t) {
                const uint64_t p = by_pair[t];
                const apd_spot_window &w = windows[p];
                SpotTraceWindow &tw = trace[std::lower_bound(live.begin(), live.end(), p) - live.begin()];
                uint32_t k = rp.iv_first;
                while (intervals[k].b < w.end) ++k;                       // the interval that holds [start, end]
                tw.px = rp.px; tw.py = rp.py; tw.end = w.end; tw.start = w.start;
                tw.a = intervals[k].a; tw.dir_off = intervals[k].off;
                tw.end_slot = (uint32_t)(std::lower_bound(ends.begin() + rp.end_first, ends.end(), w.end) - ends.begin());
                tw.step_off = step_off[p] - step_off[first];
            }
            rec_pairs[c].push_back(rp);
            g = g_end;
        }
        // ---- workspaces
        const size_t nt = trace.size(), ne = ends.size();
        size_t np = 0;
        for (auto &v : rec_pairs) np += v.size();
        const size_t steps_bytes = (size_t)(step_off[last] - step_off[first]) * sizeof(apd_path_step);
        const size_t o_pairs = 0, o_iv = o_pairs + np * sizeof(SpotRecPair), o_win = o_iv + intervals.size() * sizeof(SpotInterval);
        const size_t o_ends = o_win + nt * sizeof(SpotTraceWindow), upload_bytes = up16(o_ends + ne * 4);
        const size_t o_end_cost = upload_bytes, o_end_start = o_end_cost + up16(ne * 4), o_len = o_end_start + up16(ne * 4);
        const size_t o_found = o_len + up16(nt * 4), o_scores = o_found + up16(nt * 4), side_bytes = o_scores + up16(nt * 4);
        rc = reserve_ws(ctx, ctx->ws_spot_dirs, std::max<size_t>((size_t)words * sizeof(uint32_t), 16));
        if (rc) return rc;
        rc = reserve_ws(ctx, ctx->ws_spot_steps, steps_bytes + side_bytes + 16);
        if (rc) return rc;
        upload.assign(upload_bytes, 0);
        size_t class_first[kClasses], at = 0;
        for (uint32_t c = 0; c < kClasses; ++c) {
            class_first[c] = at;
            if (!rec_pairs[c].empty()) std::memcpy(upload.data() + o_pairs + at * sizeof(SpotRecPair), rec_pairs[c].data(), rec_pairs[c].size() * sizeof(SpotRecPair));
            at += rec_pairs[c].size();
        }
        std::memcpy(upload.data() + o_iv, intervals.data(), intervals.size() * sizeof(SpotInterval));
        std::memcpy(upload.data() + o_win, trace.data(), nt * sizeof(SpotTraceWindow));
        std::memcpy(upload.data() + o_ends, ends.data(), ne * 4);
        char *base = ctx->ws_spot_steps.as<char>(), *side = base + steps_bytes;
        SpotPathLaunch L{};
        L.d_frames = batch->d_frames.as<float>(); L.d_seq_off = batch->d_seq_off; L.dim = batch->dim; L.dpad = batch->dpad;
        L.ins = cfg->insertion_penalty; L.del = cfg->deletion_penalty; L.mat = cfg->match_penalty;
        L.d_intervals = (const SpotInterval *)(side + o_iv);
        L.d_ends = (const uint32_t *)(side + o_ends);
        L.d_end_cost = (float *)(side + o_end_cost); L.d_end_start = (uint32_t *)(side + o_end_start);
        L.d_dirs = ctx->ws_spot_dirs.as<uint32_t>();
        L.d_windows = (const SpotTraceWindow *)(side + o_win); L.n_windows = (uint32_t)nt;
        L.d_steps = (apd_path_step *)base;
        L.d_len = (uint32_t *)(side + o_len); L.d_found = (uint32_t *)(side + o_found); L.d_scores = (float *)(side + o_scores);
        HIP_TRY(ctx, hipMemcpyAsync(side, upload.data(), upload_bytes, hipMemcpyHostToDevice, ctx->stream));
        if (ctx->timing && first_launch) HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
        first_launch = false;
        for (uint32_t c = 0; c < kClasses; ++c) {
            L.d_pairs = (const SpotRecPair *)(side + o_pairs) + class_first[c];
            L.n_pairs = (uint32_t)rec_pairs[c].size();
            HIP_TRY(ctx, launch_spot_record(L, c, r_max, ctx->stream));
        }
        HIP_TRY(ctx, launch_spot_trace(L, ctx->stream));
        if (ctx->timing) { HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream)); ctx->timed = true; }   // the last chunk's record stands
        h_len.resize(nt); h_found.resize(nt); h_scores.resize(nt);
        HIP_TRY(ctx, hipMemcpyAsync(steps + step_off[first], L.d_steps, steps_bytes, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(h_len.data(), L.d_len, nt * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(h_found.data(), L.d_found, nt * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(h_scores.data(), L.d_scores, nt * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));                  // the next chunk reuses the workspaces (and `upload`)
        for (size_t t = 0; t < nt; ++t) {
            const uint64_t p = live[t];
            path_len[p] = h_len[t];
            if (found_start) found_start[p] = h_found[t];
            if (scores) scores[p] = h_scores[t];
        }
        first = last;
    }
    return APD_OK;
}

// ------------------------------------------------------------------------------------ streaming spotting

// A resident spotting session (include/apd.h, "streaming spotting"; kernels: dtw_spot_stream.hip).  Everything a push needs lives
// here and grows only: the pair descriptors (grouped by kernel class once, at create), the two halves of the carried columns, the
// running bests, the words a push uploads, the staged chunk and the curves.
struct apd_spot_stream : apd::ContextChild {
    static constexpr uint32_t kClasses = kSpotRegisterRows + 1;             // spot_row_class
    const apd_batch *templates = nullptr;
    uint32_t n_queries = 0, n_channels = 0, n_pairs = 0;
    float ins = 0.0f, del = 0.0f, mat = 0.0f;
    std::vector<uint64_t> columns;      // per channel: absolute column of the last frame pushed (first_column after a reset)
    std::vector<uint32_t> parity;       // per channel: the half of d_state that holds its column
    std::vector<SpotStreamPair> h_pairs;
    std::vector<uint32_t> h_push;       // host image of d_push, alive as long as the session (the upload is asynchronous)
    uint32_t class_first[kClasses] = {}, class_count[kClasses] = {};
    uint32_t r_max = 1;
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
        S.d_frames = templates->d_frames.as<float>(); S.d_seq_off = templates->d_seq_off;
        S.d_stage = d_stage.as<float>(); S.d_push = d_push.as<uint32_t>();
        S.n_channels = n_channels; S.n_queries = n_queries; S.dim = templates->dim; S.dpad = templates->dpad;
        S.ins = ins; S.del = del; S.mat = mat;
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
    std::vector<uint32_t> pos(n_seq);                                     // caller's sequence number -> resident position
    for (uint32_t p = 0; p < n_seq; ++p) pos[templates->order[p]] = p;
    auto len_of = [&](uint32_t s) { return (uint32_t)(templates->offsets[pos[s] + 1] - templates->offsets[pos[s]]); };
    for (uint32_t q = 0; q < n_queries; ++q)
        if (len_of(queries[q]) == 0) return APD_ERR_EMPTY_SEQUENCE;
    for (uint32_t q = 0; q < n_queries; ++q)
        if (len_of(queries[q]) > kSpotMaxQuery) {
            ctx->last_error = "apd_spot_stream_create: a query of more than " + std::to_string(kSpotMaxQuery) + " frames";
            return APD_ERR_UNSUPPORTED;
        }
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
    for (uint32_t q = 0; q < n_queries; ++q) { s->q_len.push_back(len_of(queries[q])); s->q_pos.push_back(pos[queries[q]]); }
    s->wpl_before.assign(n_pairs + 1, 0u);
    for (uint64_t p = 0; p < n_pairs; ++p) s->wpl_before[p + 1] = s->wpl_before[p] + (spot_rows_per_lane(s->q_len[p % n_queries]) + 15) / 16;
    // the descriptors, grouped by kernel class (one launch each per push); `out` keeps p = channel n_queries + q
    constexpr uint32_t kClasses = apd_spot_stream::kClasses;
    for (uint32_t q = 0; q < n_queries; ++q) {
        const uint32_t n = len_of(queries[q]), c = spot_row_class(templates->dim, n);
        s->class_count[c] += n_channels;
        if (c == 0) s->r_max = std::max(s->r_max, spot_rows_per_lane(n));
    }
    for (uint32_t c = 1; c < kClasses; ++c) s->class_first[c] = s->class_first[c - 1] + s->class_count[c - 1];
    uint32_t fill[kClasses];
    std::copy(s->class_first, s->class_first + kClasses, fill);
    s->h_pairs.resize(n_pairs);
    uint64_t state_floats = 0;
    for (uint32_t k = 0; k < n_channels; ++k)
        for (uint32_t q = 0; q < n_queries; ++q) {
            const uint32_t n = len_of(queries[q]);
            SpotStreamPair &d = s->h_pairs[fill[spot_row_class(templates->dim, n)]++];
            d.px = pos[queries[q]];
            d.channel = k;
            d.out = k * n_queries + q;
            d.rows = spot_rows_per_lane(n);
            d.state_off = state_floats;
            state_floats += 2ull * d.rows * 64;                           // values, then starts
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
        for (uint32_t c = 0; c < apd_spot_stream::kClasses; ++c) {
            A.S.d_pairs = S.d_pairs = s->d_pairs.as<SpotStreamPair>() + s->class_first[c];
            A.S.n_pairs = S.n_pairs = s->class_count[c];
            if (s->history) HIP_TRY(ctx, launch_spot_stream_record(A, c, s->r_max, ctx->stream));
            else HIP_TRY(ctx, launch_spot_stream(S, c, s->r_max, ctx->stream));
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
// ws_spot_steps: [steps | windows (uploaded) | lengths | found | scores].
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
    const uint64_t cap = spot_workspace_cap();
    constexpr uint64_t kMaxWindowsPerLaunch = 1ull << 24;                 // 64 work-items per window, launches stay below 2^31
    auto up16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
    std::vector<uint64_t> live;                                           // the chunk's windows that reach the trace, input order
    std::vector<SpotRingWindow> trace;
    std::vector<uint32_t> h_len, h_found;
    std::vector<float> h_scores;
    bool first_launch = true;
    for (uint64_t first = 0; first < n_windows;) {
        uint64_t last = first;
        while (last < n_windows && last - first < kMaxWindowsPerLaunch) {
            if (last > first && (step_off[last + 1] - step_off[first]) * sizeof(apd_path_step) > cap) break;
            ++last;
        }
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
            path_len[p] = 0;                                              // no window, or its end has aged out: nothing to read
            if (found_start) found_start[p] = 0;
            if (scores) scores[p] = INFINITY;
            std::memset(steps + step_off[p], 0, (size_t)(step_off[p + 1] - step_off[p]) * sizeof(apd_path_step));
        }
        if (live.empty()) { first = last; continue; }
        const size_t nt = trace.size();
        const size_t steps_bytes = (size_t)(step_off[last] - step_off[first]) * sizeof(apd_path_step);
        const size_t upload_bytes = up16(nt * sizeof(SpotRingWindow));
        const size_t o_len = upload_bytes, o_found = o_len + up16(nt * 4), o_scores = o_found + up16(nt * 4), side_bytes = o_scores + up16(nt * 4);
        int rc = reserve_ws(ctx, ctx->ws_spot_steps, steps_bytes + side_bytes + 16);
        if (rc) return rc;
        char *base = ctx->ws_spot_steps.as<char>(), *side = base + steps_bytes;
        SpotRingTraceLaunch L{};
        L.d_frames = t->d_frames.as<float>(); L.d_seq_off = t->d_seq_off; L.dim = t->dim; L.dpad = t->dpad;
        L.ins = s->ins; L.del = s->del; L.mat = s->mat;
        L.H = s->rings();
        L.d_windows = (const SpotRingWindow *)side; L.n_windows = (uint32_t)nt;
        L.d_steps = (apd_path_step *)base;
        L.d_len = (uint32_t *)(side + o_len); L.d_found = (uint32_t *)(side + o_found); L.d_scores = (float *)(side + o_scores);
        HIP_TRY(ctx, hipMemcpyAsync(side, trace.data(), nt * sizeof(SpotRingWindow), hipMemcpyHostToDevice, ctx->stream));
        // an aged-out window between two traced ones leaves slots of the chunk no trace owns: the device copy is zeroed whole
        HIP_TRY(ctx, hipMemsetAsync(base, 0, steps_bytes, ctx->stream));
        if (ctx->timing && first_launch) HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
        first_launch = false;
        HIP_TRY(ctx, launch_spot_stream_trace(L, ctx->stream));
        if (ctx->timing) { HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream)); ctx->timed = true; }   // the last chunk's record stands
        h_len.resize(nt); h_found.resize(nt); h_scores.resize(nt);
        HIP_TRY(ctx, hipMemcpyAsync(steps + step_off[first], L.d_steps, steps_bytes, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(h_len.data(), L.d_len, nt * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(h_found.data(), L.d_found, nt * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(h_scores.data(), L.d_scores, nt * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));                  // the next chunk reuses the workspace (and `trace`)
        for (size_t k = 0; k < nt; ++k) {
            const uint64_t p = live[k];
            path_len[p] = h_len[k];
            if (found_start) found_start[p] = h_found[k];
            if (scores) scores[p] = h_scores[k];
        }
        first = last;
    }
    return APD_OK;
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
