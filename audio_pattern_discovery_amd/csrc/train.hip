// Autoencoder training (neural.rs:74-94, main.rs:115-135) on the GPU: the reference's batch-size-1 SGD, one wavefront per model,
// the model in LDS for the whole launch.  DESIGN.md section 4.18 has the layout, the dependent chain and the measured step time;
// train_math.h the defined sigmoid.  Host side: the apd_trainer object of include/apd.h.
#include <algorithm>
#include <cstring>
#include <limits>
#include <new>

#include "apd_internal.h"
#include "apd_plan.h"
#include "train_math.h"

namespace {

constexpr uint32_t kTrainMaxDim = 64;     // one lane per unit
constexpr int kTrainBlock = 8;            // steps whose frames are fetched together, one block ahead of their use
constexpr uint32_t kNonFiniteBits = 0x7F800000u;

struct TrainTotals {
    float total_err;                 // main.rs:130, one add per step
    uint32_t pad;
    unsigned long long steps;        // since the last reset
    unsigned long long lifetime;     // steps since creation: what first_nonfinite counts in
    unsigned long long first_nonfinite;
};

struct TrainLaunch {
    const float *d_frames;           // [n_frames][d_in]
    const uint32_t *d_order;         // [rows][n_steps], rows = 1 or n_models
    const float2 *d_norm;            // [rows][n_steps]: (min, max - min) of the step's frame if Mat::norm rescales it, else (NaN, 0)
    const float *d_alpha;            // [n_models]
    float *d_weights;                // model m: w_enc | w_dec | b_enc | b_dec from float m * model_floats
    TrainTotals *d_totals;           // [n_models]
    uint64_t n_steps;
    uint32_t d_in, latent, n_models, per_model;
    uint64_t model_floats;
};

// Mat::norm's decision per step (numerics.rs:192-208), literally and in the frame's own order: min and max skip non-finite values and
// keep the FIRST of equal candidates (the sign of a zero), and only |min - max| < 1e-8 rescales.  One work-item per (order row, step);
// nothing here is on the trainer's dependent chain.
__global__ void train_norm_kernel(const float *__restrict__ frames, const uint32_t *__restrict__ order, uint64_t n_entries, uint32_t d_in,
                                  float2 *__restrict__ norm)
{
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_entries; e += (uint64_t)gridDim.x * blockDim.x) {
        const float *x = frames + (uint64_t)order[e] * d_in;
        float mn = INFINITY, mx = -INFINITY;
        for (uint32_t k = 0; k < d_in; ++k) {
            const float v = x[k];
            const bool finite = (__float_as_uint(v) & kNonFiniteBits) != kNonFiniteBits;
            if (v < mn && finite) mn = v;
            if (v > mx && finite) mx = v;
        }
        const bool rescale = fabsf(mn - mx) < 1e-8f;
        norm[e] = rescale ? make_float2(mn, mx - mn) : make_float2(__uint_as_float(0x7FC00000u), 0.0f);
    }
}

__device__ __forceinline__ float lane_value(float v, uint32_t lane)   // v of lane `lane` (wave-uniform), through an SGPR
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), (int)lane));
}

// Runs body(k, a[k], b[k]) for k = 0 .. n-1 in ascending order.  The LDS reads of eight k are issued together and waited for once (a
// single wavefront has nothing else to hide their latency behind); beyond the last row, row n - 1 is read again and not used.
template <class A, class B, class F>
__device__ __forceinline__ void for_rows(uint32_t n, A a, B b, F body)
{
    for (uint32_t k0 = 0; k0 < n; k0 += 8) {
        float va[8], vb[8];
#pragma unroll
        for (uint32_t u = 0; u < 8; ++u) {
            const uint32_t k = min(k0 + u, n - 1);
            va[u] = a(k);
            vb[u] = b(k);
        }
#pragma unroll
        for (uint32_t u = 0; u < 8; ++u)
            if (k0 + u < n) body(k0 + u, va[u], vb[u]);
    }
}

// blockIdx.x: the model; one wavefront.  Lane j < latent is latent unit j, lane i < d_in output unit i.
// LDS (floats, every row 64 wide so that lane l's accesses fall into bank l):
//   wenc[k][j] = W_enc[k][j]            d_in rows     lane j walks its column for the latent
//   wdc [j][i] = W_dec[j][i]            latent rows   lane i walks its column for the output
//   wdr [i][j] = W_dec[j][i]            d_in rows     lane j walks its row for delta_decode; updated with the expression that
//                                                     updates wdc, so the two copies stay bit-equal
//   xs  [t][i]                          kTrainBlock rows: the frames of the current block of steps
__global__ void __launch_bounds__(64) train_kernel(TrainLaunch T)
{
    extern __shared__ float lds[];
    const uint32_t lane = threadIdx.x, m = blockIdx.x;
    const uint32_t D = T.d_in, L = T.latent;
    float *wenc = lds, *wdc = wenc + D * 64, *wdr = wdc + L * 64, *xs = wdr + D * 64;
    float *g_wenc = T.d_weights + m * T.model_floats, *g_wdec = g_wenc + D * L, *g_benc = g_wdec + L * D, *g_bdec = g_benc + L;
    const bool on_l = lane < L, on_d = lane < D;

    for (uint32_t k = 0; k < D; ++k) wenc[k * 64 + lane] = on_l ? g_wenc[k * L + lane] : 0.0f;
    for (uint32_t j = 0; j < L; ++j) wdc[j * 64 + lane] = on_d ? g_wdec[j * D + lane] : 0.0f;
    for (uint32_t i = 0; i < D; ++i) wdr[i * 64 + lane] = on_l ? g_wdec[lane * D + i] : 0.0f;
    float benc = on_l ? g_benc[lane] : 0.0f, bdec = on_d ? g_bdec[lane] : 0.0f;
    TrainTotals tot = T.d_totals[m];
    const float alpha = T.d_alpha[m];
    const uint64_t n_steps = T.n_steps;
    const uint32_t *order = T.d_order + (T.per_model ? (uint64_t)m * n_steps : 0);
    const float2 *norm = T.d_norm + (T.per_model ? (uint64_t)m * n_steps : 0);
    const float *frames = T.d_frames;
    const uint32_t l8 = lane & (kTrainBlock - 1);
    uint32_t seen_l = 0, seen_d = 0;       // the largest |weight| bit pattern this lane has stored: >= kNonFiniteBits once non-finite

    // Prefetch: the frames of a block are in flight during the block before it, their order indices one block earlier still.
    float xn[kTrainBlock];
    uint32_t ord_next = 0;
    float2 nrm_next = make_float2(0.0f, 0.0f);
    {
        const uint32_t o = l8 < n_steps ? order[l8] : 0;
#pragma unroll
        for (int t = 0; t < kTrainBlock; ++t) {
            xn[t] = 0.0f;
            if ((uint64_t)t < n_steps) {
                const uint64_t f = (uint32_t)__builtin_amdgcn_readlane((int)o, t);
                if (on_d) xn[t] = frames[f * D + lane];
            }
        }
        if (l8 < n_steps) nrm_next = norm[l8];
        if ((uint64_t)kTrainBlock + l8 < n_steps) ord_next = order[kTrainBlock + l8];
    }

    for (uint64_t s0 = 0; s0 < n_steps; s0 += kTrainBlock) {
#pragma unroll
        for (int t = 0; t < kTrainBlock; ++t) xs[t * 64 + lane] = xn[t];
        const float2 nrm = nrm_next;
        {   // the next block's frames, and the order of the one after
            const uint64_t s1 = s0 + kTrainBlock;
            const uint32_t o = ord_next;
#pragma unroll
            for (int t = 0; t < kTrainBlock; ++t) {
                xn[t] = 0.0f;
                if (s1 + t < n_steps) {
                    const uint64_t f = (uint32_t)__builtin_amdgcn_readlane((int)o, t);
                    if (on_d) xn[t] = frames[f * D + lane];
                }
            }
            nrm_next = make_float2(0.0f, 0.0f);
            if (s1 + l8 < n_steps) nrm_next = norm[s1 + l8];
            ord_next = 0;
            if (s1 + kTrainBlock + l8 < n_steps) ord_next = order[s1 + kTrainBlock + l8];
        }
        const uint32_t nb = (uint32_t)min((uint64_t)kTrainBlock, n_steps - s0);
        for (uint32_t t = 0; t < nb; ++t) {
            const float *xt = xs + t * 64;
            const float x = xt[lane];
            // y = x.norm(): the rescale is rare (a frame whose finite values all coincide) and wave-uniform
            const float mn = lane_value(nrm.x, t), scaler = lane_value(nrm.y, t);
            float y = x;
            if (mn == mn) y = (x - mn) / scaler;
            // latent = x . W_enc + b_enc (numerics.rs:305-319: from 0.0, k ascending, multiply then add)
            float acc = 0.0f;
            for_rows(D, [&](uint32_t k) { return xt[k]; }, [&](uint32_t k) { return wenc[k * 64 + lane]; },
                     [&](uint32_t, float xk, float w) { acc = acc + xk * w; });
            const float latent = acc + benc;
            const float la = apd::train_sigmoid(latent);
            // output = latent . W_dec + b_dec, from the pre-activation latent (neural.rs:78)
            acc = 0.0f;
            for_rows(L, [&](uint32_t) { return 0.0f; }, [&](uint32_t j) { return wdc[j * 64 + lane]; },
                     [&](uint32_t j, float, float w) { acc = acc + lane_value(latent, j) * w; });
            const float act = apd::train_sigmoid(acc + bdec);
            const float dout = ((y - act) * -1.0f) * (act * (1.0f - act));
            // delta_decode = (delta_out . W_dec^T) (.) la (1 - la)
            acc = 0.0f;
            for_rows(D, [&](uint32_t) { return 0.0f; }, [&](uint32_t i) { return wdr[i * 64 + lane]; },
                     [&](uint32_t i, float, float w) { acc = acc + lane_value(dout, i) * w; });
            const float ddec = acc * (la * (1.0f - la));
            // the updates; a gradient entry is Mat::mul over one term, 0.0 + a * b, then scaled by alpha (neural.rs:87-92)
            for_rows(L, [&](uint32_t) { return 0.0f; }, [&](uint32_t j) { return wdc[j * 64 + lane]; },
                     [&](uint32_t j, float, float w) {
                         const float nw = w - (0.0f + lane_value(latent, j) * dout) * alpha;
                         wdc[j * 64 + lane] = nw;
                         seen_d = max(seen_d, __float_as_uint(nw) & 0x7FFFFFFFu);
                     });
            for_rows(D, [&](uint32_t) { return 0.0f; }, [&](uint32_t i) { return wdr[i * 64 + lane]; },
                     [&](uint32_t i, float, float w) { wdr[i * 64 + lane] = w - (0.0f + latent * lane_value(dout, i)) * alpha; });
            for_rows(D, [&](uint32_t k) { return xt[k]; }, [&](uint32_t k) { return wenc[k * 64 + lane]; },
                     [&](uint32_t k, float xk, float w) {
                         const float nw = w - (0.0f + xk * ddec) * alpha;
                         wenc[k * 64 + lane] = nw;
                         seen_l = max(seen_l, __float_as_uint(nw) & 0x7FFFFFFFu);
                     });
            benc = benc - ddec * alpha;
            bdec = bdec - dout * alpha;
            seen_l = max(seen_l, __float_as_uint(benc) & 0x7FFFFFFFu);
            seen_d = max(seen_d, __float_as_uint(bdec) & 0x7FFFFFFFu);
            // 0.5 * euclidean(activation, y) (numerics.rs:114-120), i ascending
            const float diff = act - y, sq = diff * diff;
            float dist = 0.0f;
            for (uint32_t i = 0; i < D; ++i) dist = dist + lane_value(sq, i);
            tot.total_err = tot.total_err + 0.5f * __builtin_sqrtf(dist);
            const bool bad = (on_l && seen_l >= kNonFiniteBits) || (on_d && seen_d >= kNonFiniteBits);
            if (tot.first_nonfinite == ~0ull && __ballot(bad) != 0) tot.first_nonfinite = tot.lifetime;
            ++tot.steps;
            ++tot.lifetime;
        }
    }

    if (on_l) {
        for (uint32_t k = 0; k < D; ++k) g_wenc[k * L + lane] = wenc[k * 64 + lane];
        g_benc[lane] = benc;
    }
    if (on_d) {
        for (uint32_t j = 0; j < L; ++j) g_wdec[j * D + lane] = wdc[j * 64 + lane];
        g_bdec[lane] = bdec;
    }
    if (lane == 0) T.d_totals[m] = tot;
}

size_t train_lds_bytes(uint32_t d_in, uint32_t latent) { return ((size_t)(2 * d_in + latent) * 64 + kTrainBlock * 64) * sizeof(float); }

// ---- evaluation (apd_trainer_evaluate): the forward half of the step above under frozen weights, one lane
// per position.  Nothing below writes the trainer.
struct EvalCarry {
    float total_err;                 // main.rs:130 with the weights frozen: one add per position, in position order
    uint32_t pad;
    unsigned long long first_nonfinite;   // the first position whose error is not finite
};

struct EvalLaunch {
    const float *d_frames;           // [n_frames][d_in]
    const uint32_t *d_order;         // the chunk's first entry of row 0; nullptr: position p names frame first + p
    const float *d_weights;          // the trainer's
    float *d_err;                    // model m, position p of the chunk: d_err[m * err_stride + p]
    EvalCarry *d_carry;              // [n_models]
    uint64_t first;                  // the chunk's first position
    uint64_t n_pos;                  // positions of the chunk
    uint64_t order_stride;           // 0: one order for all models
    uint64_t err_stride;
    uint64_t model_floats;
    uint32_t d_in, latent, n_models;
    uint32_t groups;                 // workgroups per model
};

constexpr uint32_t kEvalBlockOutputs = 4;   // units whose sums run side by side: one read of x[k] (latent[j]) feeds four of them
constexpr size_t kEvalLdsTarget = 64 * 1024;

// A workgroup owns model blockIdx.x / groups and every `groups`-th tile of blockDim.x positions; the model is staged once.
// LDS (floats): wenc [D][L] | wdec [L][D] | benc [L] | bdec [D] in the reference's flat layouts (every lane reads the same word: a
// broadcast) | xs [D][T] the tile's frames | lat [L][T] its pre-activation latents (lane t's accesses fall into bank t mod 64).
// Every (model, position) chain is private to a lane, in the order of train_kernel: the bits do not depend on T, groups or the grid.
__global__ void __launch_bounds__(256) train_eval_kernel(EvalLaunch E)
{
    extern __shared__ float lds[];
    const uint32_t D = E.d_in, L = E.latent, T = blockDim.x, t = threadIdx.x;
    const uint32_t m = blockIdx.x / E.groups, g = blockIdx.x % E.groups;
    float *wenc = lds, *wdec = wenc + D * L, *benc = wdec + L * D, *bdec = benc + L, *xs = bdec + D, *lat = xs + D * T;
    const float *gw = E.d_weights + m * E.model_floats;
    for (uint32_t i = t; i < (uint32_t)E.model_floats; i += T) lds[i] = gw[i];
    const uint32_t *order = E.d_order ? E.d_order + m * E.order_stride : nullptr;
    float *err = E.d_err + m * E.err_stride;
    const uint64_t n_tiles = (E.n_pos + T - 1) / T;
    __syncthreads();

    for (uint64_t tile = g; tile < n_tiles; tile += E.groups) {
        const uint64_t p = tile * T + t;
        if (p >= E.n_pos) continue;                 // no barrier below: xs and lat columns are the lane's own
        const float *x = E.d_frames + (order ? (uint64_t)order[p] : E.first + p) * D;
        // the frame, and Mat::norm's decision as train_norm_kernel takes it
        float mn = INFINITY, mx = -INFINITY;
        for (uint32_t k = 0; k < D; ++k) {
            const float v = x[k];
            xs[k * T + t] = v;
            const bool finite = (__float_as_uint(v) & kNonFiniteBits) != kNonFiniteBits;
            if (v < mn && finite) mn = v;
            if (v > mx && finite) mx = v;
        }
        const bool rescale = fabsf(mn - mx) < 1e-8f;
        const float scaler = mx - mn;
        // latent = x . W_enc + b_enc (from 0.0, k ascending, multiply then add)
        for (uint32_t j0 = 0; j0 < L; j0 += kEvalBlockOutputs) {
            float acc[kEvalBlockOutputs];
            uint32_t col[kEvalBlockOutputs];
#pragma unroll
            for (uint32_t u = 0; u < kEvalBlockOutputs; ++u) { acc[u] = 0.0f; col[u] = min(j0 + u, L - 1); }
            for (uint32_t k = 0; k < D; ++k) {
                const float xk = xs[k * T + t];
#pragma unroll
                for (uint32_t u = 0; u < kEvalBlockOutputs; ++u) acc[u] = acc[u] + xk * wenc[k * L + col[u]];
            }
#pragma unroll
            for (uint32_t u = 0; u < kEvalBlockOutputs; ++u)
                if (j0 + u < L) lat[(j0 + u) * T + t] = acc[u] + benc[j0 + u];
        }
        // output = latent . W_dec + b_dec from the pre-activation latent; the output units are streamed into the distance, i ascending
        float dist = 0.0f;
        for (uint32_t i0 = 0; i0 < D; i0 += kEvalBlockOutputs) {
            float acc[kEvalBlockOutputs];
            uint32_t col[kEvalBlockOutputs];
#pragma unroll
            for (uint32_t u = 0; u < kEvalBlockOutputs; ++u) { acc[u] = 0.0f; col[u] = min(i0 + u, D - 1); }
            for (uint32_t j = 0; j < L; ++j) {
                const float lj = lat[j * T + t];
#pragma unroll
                for (uint32_t u = 0; u < kEvalBlockOutputs; ++u) acc[u] = acc[u] + lj * wdec[j * D + col[u]];
            }
#pragma unroll
            for (uint32_t u = 0; u < kEvalBlockOutputs; ++u) {
                if (i0 + u < D) {
                    const float act = apd::train_sigmoid(acc[u] + bdec[i0 + u]);
                    const float xi = xs[(i0 + u) * T + t];
                    float y = xi;
                    if (rescale) y = (xi - mn) / scaler;
                    const float diff = act - y, sq = diff * diff;
                    dist = dist + sq;
                }
            }
        }
        err[p] = 0.5f * __builtin_sqrtf(dist);
    }
}

// blockIdx.x: the model; one wavefront.  The chunk's errors 64 per load, added in position order on one chain.
__global__ void __launch_bounds__(64) train_eval_total_kernel(EvalLaunch E)
{
    const uint32_t lane = threadIdx.x, m = blockIdx.x;
    const float *err = E.d_err + m * E.err_stride;
    EvalCarry c = E.d_carry[m];
    float next = lane < E.n_pos ? err[lane] : 0.0f;
    for (uint64_t s = 0; s < E.n_pos; s += 64) {
        const float v = next;
        if (s + 64 + lane < E.n_pos) next = err[s + 64 + lane];
        const uint32_t n = (uint32_t)min((uint64_t)64, E.n_pos - s);
        const bool bad = lane < n && (__float_as_uint(v) & kNonFiniteBits) == kNonFiniteBits;
        const unsigned long long b = __ballot(bad);
        if (b != 0 && c.first_nonfinite == ~0ull) c.first_nonfinite = E.first + s + (uint64_t)__builtin_ctzll(b);
        if (n == 64) {
#pragma unroll
            for (uint32_t l = 0; l < 64; ++l) c.total_err = c.total_err + lane_value(v, l);
        } else {
            for (uint32_t l = 0; l < n; ++l) c.total_err = c.total_err + lane_value(v, l);
        }
    }
    if (lane == 0) E.d_carry[m] = c;
}

// positions per workgroup of train_eval_kernel: the most of 256, 128, 64 whose tile keeps the workgroup's LDS within kEvalLdsTarget
uint32_t eval_tile(uint32_t d_in, uint32_t latent, uint64_t model_floats)
{
    for (uint32_t tile : {256u, 128u})
        if ((model_floats + (size_t)(d_in + latent) * tile) * sizeof(float) <= kEvalLdsTarget) return tile;
    return 64;
}

}  // namespace

struct apd_trainer : apd::ContextChild {
    apd::DeviceBuf d_weights;         // n_models x (w_enc | w_dec | b_enc | b_dec)
    apd::DeviceBuf d_totals;          // n_models TrainTotals
    uint32_t d_in = 0, latent = 0, n_models = 0;
    uint64_t model_floats = 0;
    void release_device() override { d_weights.reset(); d_totals.reset(); }
};

extern "C" int apd_trainer_create(apd_context *ctx, uint32_t d_in, uint32_t latent, uint32_t n_models, const float *w_encode,
                                  const float *w_decode, const float *b_encode, const float *b_decode, apd_trainer **out)
{
    if (!ctx || !out || !w_encode || !w_decode || !b_encode || !b_decode || n_models == 0 || d_in == 0 || latent == 0)
        return APD_ERR_INVALID_ARG;
    *out = nullptr;
    if (d_in > kTrainMaxDim || latent > kTrainMaxDim) return APD_ERR_UNSUPPORTED;
    HIP_TRY(ctx, apd::bind_device(ctx));
    apd_trainer *t = new (std::nothrow) apd_trainer();
    if (!t) return APD_ERR_OOM;
    t->ctx = ctx; t->d_in = d_in; t->latent = latent; t->n_models = n_models;
    const uint64_t wf = (uint64_t)d_in * latent;
    t->model_floats = 2 * wf + latent + d_in;
    std::vector<float> image;
    std::vector<TrainTotals> totals;
    try {
        image.resize(t->model_floats * n_models);
        totals.assign(n_models, TrainTotals{0.0f, 0u, 0ull, 0ull, ~0ull});
    } catch (const std::bad_alloc &) {
        delete t;
        return APD_ERR_OOM;
    }
    for (uint32_t m = 0; m < n_models; ++m) {
        float *p = image.data() + m * t->model_floats;
        std::memcpy(p, w_encode + m * wf, wf * sizeof(float));
        std::memcpy(p + wf, w_decode + m * wf, wf * sizeof(float));
        std::memcpy(p + 2 * wf, b_encode + (uint64_t)m * latent, latent * sizeof(float));
        std::memcpy(p + 2 * wf + latent, b_decode + (uint64_t)m * d_in, d_in * sizeof(float));
    }
    hipError_t err = t->d_weights.alloc(image.size() * sizeof(float));
    if (err == hipSuccess) err = t->d_totals.alloc(totals.size() * sizeof(TrainTotals));
    if (err == hipSuccess) err = hipMemcpyAsync(t->d_weights.ptr, image.data(), image.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream);
    if (err == hipSuccess) err = hipMemcpyAsync(t->d_totals.ptr, totals.data(), totals.size() * sizeof(TrainTotals), hipMemcpyHostToDevice, ctx->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(ctx->stream);
    if (err != hipSuccess) {
        ctx->last_error = std::string("apd_trainer_create: ") + hipGetErrorString(err);
        delete t;
        return err == hipErrorOutOfMemory ? APD_ERR_OOM : APD_ERR_HIP;
    }
    ctx->children.insert(t);
    *out = t;
    return APD_OK;
}

extern "C" int apd_trainer_destroy(apd_trainer *trainer) { return apd::destroy_child(trainer); }

extern "C" int apd_trainer_run(apd_context *ctx, apd_trainer *t, const float *frames, uint64_t n_frames, int frames_on_device,
                               const uint32_t *order, uint64_t n_steps, int order_per_model, const float *alpha)
{
    if (!ctx || !t || t->ctx != ctx || !alpha || (n_steps && (!order || !frames))) return APD_ERR_INVALID_ARG;
    const uint64_t rows = order_per_model ? t->n_models : 1;
    if (n_steps >= (1ull << 40) / rows) return APD_ERR_INVALID_ARG;
    const uint64_t n_entries = rows * n_steps;
    for (uint64_t e = 0; e < n_entries; ++e)
        if (order[e] >= n_frames) return APD_ERR_INVALID_ARG;          // before anything is enqueued
    if (n_steps == 0) return APD_OK;                                    // nothing runs: every bit of the state stays
    HIP_TRY(ctx, apd::bind_device(ctx));
    APD_AFFINITY(ctx, "trainer launch");
    apd::DeviceBuf pool, d_host_frames;                                 // pool: [norm | order | alpha]
    const size_t norm_bytes = n_entries * sizeof(float2), order_bytes = (n_entries * sizeof(uint32_t) + 15) & ~(size_t)15;
    HIP_TRY(ctx, pool.alloc(norm_bytes + order_bytes + t->n_models * sizeof(float)));
    float2 *d_norm = pool.as<float2>();
    uint32_t *d_order = (uint32_t *)(pool.as<char>() + norm_bytes);
    float *d_alpha = (float *)(pool.as<char>() + norm_bytes + order_bytes);
    HIP_TRY(ctx, hipMemcpyAsync(d_order, order, n_entries * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d_alpha, alpha, t->n_models * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    const float *d_frames = frames;
    if (!frames_on_device) {
        const size_t bytes = (size_t)n_frames * t->d_in * sizeof(float);
        HIP_TRY(ctx, d_host_frames.alloc(bytes));
        HIP_TRY(ctx, hipMemcpyAsync(d_host_frames.ptr, frames, bytes, hipMemcpyHostToDevice, ctx->stream));
        d_frames = d_host_frames.as<float>();
    }
    const unsigned norm_blocks = (unsigned)std::min<uint64_t>((n_entries + 255) / 256, 8192);
    hipLaunchKernelGGL(train_norm_kernel, dim3(norm_blocks), dim3(256), 0, ctx->stream, d_frames, d_order, n_entries, t->d_in, d_norm);
    TrainLaunch T{};
    T.d_frames = d_frames; T.d_order = d_order; T.d_norm = d_norm; T.d_alpha = d_alpha;
    T.d_weights = t->d_weights.as<float>(); T.d_totals = t->d_totals.as<TrainTotals>();
    T.n_steps = n_steps; T.d_in = t->d_in; T.latent = t->latent; T.n_models = t->n_models; T.per_model = order_per_model ? 1u : 0u;
    T.model_floats = t->model_floats;
    if (ctx->timing) HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    hipLaunchKernelGGL(train_kernel, dim3(t->n_models), dim3(64), train_lds_bytes(t->d_in, t->latent), ctx->stream, T);
    HIP_TRY(ctx, hipGetLastError());
    if (ctx->timing) { HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream)); ctx->timed = true; }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return APD_OK;
}

extern "C" int apd_trainer_totals(apd_trainer *t, float *total_err, uint64_t *steps, uint64_t *first_nonfinite, int reset)
{
    if (!t || !t->ctx) return APD_ERR_INVALID_ARG;
    apd_context *ctx = t->ctx;
    HIP_TRY(ctx, apd::bind_device(ctx));
    std::vector<TrainTotals> h(t->n_models);
    HIP_TRY(ctx, hipMemcpyAsync(h.data(), t->d_totals.ptr, h.size() * sizeof(TrainTotals), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (uint32_t m = 0; m < t->n_models; ++m) {
        if (total_err) total_err[m] = h[m].total_err;
        if (steps) steps[m] = h[m].steps;
        if (first_nonfinite) first_nonfinite[m] = h[m].first_nonfinite;
        h[m].total_err = 0.0f;
        h[m].steps = 0;
    }
    if (reset) {                                                        // an epoch boundary (main.rs:117-118); the weights stay
        HIP_TRY(ctx, hipMemcpyAsync(t->d_totals.ptr, h.data(), h.size() * sizeof(TrainTotals), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    return APD_OK;
}

extern "C" int apd_trainer_weights(apd_trainer *t, uint32_t model, float *w_encode, float *w_decode, float *b_encode, float *b_decode)
{
    if (!t || !t->ctx || model >= t->n_models || !w_encode || !w_decode || !b_encode || !b_decode) return APD_ERR_INVALID_ARG;
    apd_context *ctx = t->ctx;
    HIP_TRY(ctx, apd::bind_device(ctx));
    const uint64_t wf = (uint64_t)t->d_in * t->latent;
    const float *p = t->d_weights.as<float>() + model * t->model_floats;
    HIP_TRY(ctx, hipMemcpyAsync(w_encode, p, wf * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(w_decode, p + wf, wf * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(b_encode, p + 2 * wf, t->latent * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(b_decode, p + 2 * wf + t->latent, t->d_in * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return APD_OK;
}

extern "C" int apd_trainer_encoder(apd_context *ctx, apd_trainer *t, uint32_t model, apd_encoder **encoder)
{
    if (!ctx || !t || t->ctx != ctx || model >= t->n_models || !encoder) return APD_ERR_INVALID_ARG;
    const float *p = t->d_weights.as<float>() + model * t->model_floats;
    return apd::encoder_from_device(ctx, p, p + 2 * (uint64_t)t->d_in * t->latent, t->d_in, t->latent, encoder);
}

// Evaluation: every model's current weights on frames[order[e]], no update.  Nothing here writes t->d_weights or t->d_totals, so the
// trainer keeps its bits whatever this call returns.  The positions are cut into chunks whose per-frame errors stay within the cap
// (APD_EVAL_WORKSPACE_BYTES, 1 GiB); the running total and the first non-finite position travel between chunks in d_carry.
extern "C" int apd_trainer_evaluate(apd_context *ctx, apd_trainer *t, const float *frames, uint64_t n_frames, int frames_on_device,
                                    const uint32_t *order, uint64_t n_eval, int order_per_model, float *errors, int errors_on_device,
                                    float *total_err, uint64_t *first_nonfinite)
{
    if (!ctx) return APD_ERR_INVALID_ARG;
    auto refuse = [ctx](const char *why) { ctx->last_error = std::string("apd_trainer_evaluate: ") + why; return APD_ERR_INVALID_ARG; };
    if (!t || t->ctx != ctx) return refuse("the trainer is not one of this context");
    if (!errors && !total_err && !first_nonfinite) return refuse("errors, total_err and first_nonfinite are all NULL");
    if (n_frames >= (1ull << 32)) return refuse("2^32 frames or more");
    if (!order && order_per_model) return refuse("order_per_model without an order");
    if (!order && n_eval != n_frames) return refuse("order == NULL needs n_eval == n_frames");
    if (n_eval && !frames) return refuse("frames is NULL");
    const uint64_t rows = order_per_model ? t->n_models : 1;
    if (n_eval >= (1ull << 40) / t->n_models) return refuse("n_models * n_eval is 2^40 or more");
    const uint64_t n_entries = order ? rows * n_eval : 0;
    for (uint64_t e = 0; e < n_entries; ++e)
        if (order[e] >= n_frames) return refuse("an order entry is not below n_frames");      // before anything is enqueued
    const uint32_t n_models = t->n_models;
    if (n_eval == 0) {
        for (uint32_t m = 0; m < n_models; ++m) {
            if (total_err) total_err[m] = 0.0f;
            if (first_nonfinite) first_nonfinite[m] = ~0ull;
        }
        return APD_OK;
    }
    HIP_TRY(ctx, apd::bind_device(ctx));
    APD_AFFINITY(ctx, "trainer evaluation");
    const bool want_totals = total_err || first_nonfinite;
    const uint64_t cap = apd::workspace_cap("APD_EVAL_WORKSPACE_BYTES");
    const uint64_t chunk = std::min<uint64_t>(n_eval, std::max<uint64_t>(cap / ((uint64_t)n_models * sizeof(float)), 1));
    apd::DeviceBuf d_order, d_host_frames;
    std::vector<EvalCarry> carry;
    try {
        carry.assign(n_models, EvalCarry{0.0f, 0u, ~0ull});
    } catch (const std::bad_alloc &) {
        return APD_ERR_OOM;
    }
    // the context's workspace: [carry | the chunk's errors, unless they go to the caller's device buffer]
    apd::Carve ws;
    const size_t o_carry = ws.take<EvalCarry>(n_models);
    const size_t o_err = ws.take<float>(errors_on_device && errors ? 0 : (size_t)n_models * chunk);
    if (const int rc = reserve_ws(ctx, ctx->ws_misc, ws.size)) return rc;
    EvalCarry *d_carry = (EvalCarry *)(ctx->ws_misc.as<char>() + o_carry);
    float *d_ws_err = (float *)(ctx->ws_misc.as<char>() + o_err);
    HIP_TRY(ctx, hipMemcpyAsync(d_carry, carry.data(), n_models * sizeof(EvalCarry), hipMemcpyHostToDevice, ctx->stream));
    if (order) {
        HIP_TRY(ctx, d_order.alloc(n_entries * sizeof(uint32_t)));
        HIP_TRY(ctx, hipMemcpyAsync(d_order.ptr, order, n_entries * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    }
    const float *d_frames = frames;
    if (!frames_on_device) {
        const size_t bytes = (size_t)n_frames * t->d_in * sizeof(float);
        HIP_TRY(ctx, d_host_frames.alloc(bytes));
        HIP_TRY(ctx, hipMemcpyAsync(d_host_frames.ptr, frames, bytes, hipMemcpyHostToDevice, ctx->stream));
        d_frames = d_host_frames.as<float>();
    }
    const uint32_t tile = eval_tile(t->d_in, t->latent, t->model_floats);
    const size_t lds_bytes = (t->model_floats + (size_t)(t->d_in + t->latent) * tile) * sizeof(float);
    if (lds_bytes > 64 * 1024)
        HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(train_eval_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    EvalLaunch E{};
    E.d_frames = d_frames; E.d_weights = t->d_weights.as<float>(); E.d_carry = d_carry;
    E.order_stride = order_per_model ? n_eval : 0; E.model_floats = t->model_floats;
    E.d_in = t->d_in; E.latent = t->latent; E.n_models = n_models;
    if (ctx->timing) HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    for (uint64_t first = 0; first < n_eval; first += chunk) {
        const uint64_t n_pos = std::min(chunk, n_eval - first);
        E.first = first; E.n_pos = n_pos;
        E.d_order = order ? d_order.as<uint32_t>() + first : nullptr;
        if (errors_on_device && errors) { E.d_err = errors + first; E.err_stride = n_eval; }
        else { E.d_err = d_ws_err; E.err_stride = n_pos; }
        // workgroups per model: enough to fill the chip a few times over, and several tiles per staged model beyond that
        const uint64_t n_tiles = (n_pos + tile - 1) / tile;
        E.groups = (uint32_t)std::min<uint64_t>(n_tiles, std::max<uint32_t>(2048 / n_models, 1));
        hipLaunchKernelGGL(train_eval_kernel, dim3(n_models * E.groups), dim3(tile), lds_bytes, ctx->stream, E);
        HIP_TRY(ctx, hipGetLastError());
        if (want_totals) {
            hipLaunchKernelGGL(train_eval_total_kernel, dim3(n_models), dim3(64), 0, ctx->stream, E);
            HIP_TRY(ctx, hipGetLastError());
        }
        if (ctx->timing && first + n_pos == n_eval) { HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream)); ctx->timed = true; }
        if (errors && !errors_on_device)
            HIP_TRY(ctx, hipMemcpy2DAsync(errors + first, n_eval * sizeof(float), d_ws_err, n_pos * sizeof(float), n_pos * sizeof(float), n_models,
                                          hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));                  // the next chunk reuses the workspace
    }
    if (want_totals) {
        HIP_TRY(ctx, hipMemcpyAsync(carry.data(), d_carry, n_models * sizeof(EvalCarry), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        for (uint32_t m = 0; m < n_models; ++m) {
            if (total_err) total_err[m] = carry[m].total_err;
            if (first_nonfinite) first_nonfinite[m] = carry[m].first_nonfinite;
        }
    }
    return APD_OK;
}
