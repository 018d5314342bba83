// Feature companions on the GPU: AutoEncoder::predict (reference src/neural.rs:55-71) and the cepstrum branch of
// NDSequence::new (src/spectrogram.rs:31-80).  Both are streaming kernels far off the hot path's critical time
// (cfg 4: 4.2 M frames x 21 floats; cfg 5: 33.5 M frames of 256 samples); they exist so that the feature sequences
// the alignment consumes are produced in HBM and never cross PCIe.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "apd_internal.h"

using namespace apd;

namespace {

// --------------------------------------------------------------------------------------- encoder
// One thread per frame.  Arithmetic order follows the reference: Mat::mul accumulates k ascending with a separate
// multiply and add (numerics.rs:310-316; this unit is built with -ffp-contract=off), add_col, sigmoid, scale(255),
// population mean / std over the latent values (numerics.rs:12-29), sigma floored at 1 (neural.rs:62), z-score.
//
// The kernel is a stream (cfg 4: 218 MB in, 134 MB out, ~300 flops per frame), so what matters is how the bytes move: a
// wavefront takes 64 consecutive frames = one contiguous run of 64 * d_in floats, brings it into LDS with 16-byte coalesced
// loads, lets every lane read ITS frame from LDS (row stride padded to an odd number of floats: conflict-free), computes, and
// sends the 64 * latent results back through LDS as one contiguous run of 16-byte stores.  (The first version read frame
// rows straight from global memory, 52 bytes apart per lane: 13 load instructions touching 52 cache lines each, 4.8 % of
// the HBM rate.)
struct EncodeFrame {
    // latent value j before the z-score: 255 * sigmoid(x . w[:, j] + b[j])
    template <typename GetX>
    __device__ static __forceinline__ float unit(uint32_t d_in, uint32_t latent, const float *__restrict__ wb, GetX x, uint32_t j)
    {
        const float *bs = wb + d_in * latent;
        float acc = 0.0f;
        for (uint32_t k = 0; k < d_in; ++k) acc = acc + x(k) * wb[k * latent + j];
        acc = acc + bs[j];
        const float s = 1.0f / (1.0f + expf(-acc));            // numerics.rs:233
        return s * 255.0f;
    }
    // sigma of the values in pred around their mean mu, floored at 1
    __device__ static __forceinline__ float sigma(uint32_t latent, const float *pred, float mu)
    {
        float sd = 0.0f;
        for (uint32_t j = 0; j < latent; ++j) { const float dv = pred[j] - mu; sd = sd + dv * dv; }
        return fmaxf(sqrtf(sd / (float)latent), 1.0f);
    }
    template <typename GetX, typename PutZ>
    __device__ static __forceinline__ void run(uint32_t d_in, uint32_t latent, const float *__restrict__ wb, GetX x, PutZ put, float *__restrict__ pred)
    {
        float mean = 0.0f;
        for (uint32_t j = 0; j < latent; ++j) {
            const float v = unit(d_in, latent, wb, x, j);
            pred[j] = v;
            mean = mean + v;
        }
        const float mu = mean / (float)latent;
        const float sg = sigma(latent, pred, mu);
        for (uint32_t j = 0; j < latent; ++j) put(j, (pred[j] - mu) / sg);
    }
    // The same frame by `gsize` consecutive lanes of one wavefront (gl: lane within the group), pred in LDS: the lanes share the
    // latent values out, every lane sums the moments in run()'s order, so the bits are run()'s.
    template <typename GetX, typename PutZ>
    __device__ static __forceinline__ void run_lanes(uint32_t d_in, uint32_t latent, const float *wb, GetX x, PutZ put, float *pred,
                                                     uint32_t gl, uint32_t gsize)
    {
        for (uint32_t j = gl; j < latent; j += gsize) pred[j] = unit(d_in, latent, wb, x, j);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       // one wavefront: LDS runs in order, only the compiler must not reorder
        float mean = 0.0f;
        for (uint32_t j = 0; j < latent; ++j) mean = mean + pred[j];
        const float mu = mean / (float)latent;
        const float sg = sigma(latent, pred, mu);
        for (uint32_t j = gl; j < latent; j += gsize) put(j, (pred[j] - mu) / sg);
    }
};

__global__ __launch_bounds__(256) void encode_kernel(const float *__restrict__ x, uint64_t t, uint32_t d_in,
                                                     const float *__restrict__ w, const float *__restrict__ b,
                                                     uint32_t latent, float *__restrict__ out)
{
    extern __shared__ float wb[];                               // w[d_in][latent] then b[latent]
    for (uint32_t e = threadIdx.x; e < d_in * latent + latent; e += blockDim.x) wb[e] = e < d_in * latent ? w[e] : b[e - d_in * latent];
    __syncthreads();
    for (uint64_t f = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; f < t; f += (uint64_t)gridDim.x * blockDim.x) {
        const float *xf = x + f * d_in;
        float *pred = out + f * latent;                         // the un-normalised values are parked in the output row
        EncodeFrame::run(d_in, latent, wb, [&](uint32_t k) { return xf[k]; }, [&](uint32_t j, float v) { pred[j] = v; }, pred);
    }
}

// The staged form.  LDS: [w | b] then, per wavefront, 64 input rows of stride_in floats and 64 output rows of stride_out.
__global__ __launch_bounds__(256) void encode_staged_kernel(const float *__restrict__ x, uint64_t t, uint32_t d_in,
                                                            const float *__restrict__ w, const float *__restrict__ b,
                                                            uint32_t latent, float *__restrict__ out)
{
    extern __shared__ float lds[];
    const uint32_t n_wb = d_in * latent + latent, stride_in = d_in | 1u, stride_out = latent | 1u;
    float *wb = lds;
    for (uint32_t e = threadIdx.x; e < n_wb; e += blockDim.x) wb[e] = e < d_in * latent ? w[e] : b[e - d_in * latent];
    __syncthreads();
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float *xin = lds + ((n_wb + 3u) & ~3u) + wave * 64u * (stride_in + stride_out), *zout = xin + 64u * stride_in;
    const uint64_t n_chunks = (t + 63) / 64, waves = (uint64_t)gridDim.x * 4u;
    for (uint64_t chunk = (uint64_t)blockIdx.x * 4u + wave; chunk < n_chunks; chunk += waves) {
        const uint64_t f0 = chunk * 64;
        const uint32_t frames = (uint32_t)min<uint64_t>(64, t - f0), n_in = frames * d_in, n_out = frames * latent;
        const float *src = x + f0 * d_in;                       // 64 * d_in * 4 bytes per chunk: a multiple of 16, and hipMalloc aligns the base
        const bool vec_in = ((uintptr_t)src & 15u) == 0;
        for (uint32_t e = lane * 4u; e < n_in; e += 256u) {     // coalesced: 1 KB per wave instruction
            float v[4];
            if (vec_in && e + 4u <= n_in) { const float4 q = *reinterpret_cast<const float4 *>(src + e); v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; }
            else for (uint32_t i = 0; i < 4; ++i) v[i] = e + i < n_in ? src[e + i] : 0.0f;
            uint32_t fr = e / d_in, k = e - fr * d_in;
            for (uint32_t i = 0; i < 4 && e + i < n_in; ++i) { xin[fr * stride_in + k] = v[i]; if (++k == d_in) { k = 0; ++fr; } }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       // one wavefront: LDS runs in order, only the compiler must not reorder
        if (lane < frames) {
            const float *mine = xin + lane * stride_in;
            float *pred = zout + lane * stride_out;
            EncodeFrame::run(d_in, latent, wb, [&](uint32_t k) { return mine[k]; }, [&](uint32_t j, float v) { pred[j] = v; }, pred);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        float *dst = out + f0 * latent;
        const bool vec_out = ((uintptr_t)dst & 15u) == 0;
        for (uint32_t e = lane * 4u; e < n_out; e += 256u) {
            float v[4];
            uint32_t fr = e / latent, j = e - fr * latent;
            for (uint32_t i = 0; i < 4; ++i) { v[i] = e + i < n_out ? zout[fr * stride_out + j] : 0.0f; if (++j == latent) { j = 0; ++fr; } }
            if (vec_out && e + 4u <= n_out) *reinterpret_cast<float4 *>(dst + e) = make_float4(v[0], v[1], v[2], v[3]);
            else for (uint32_t i = 0; i < 4 && e + i < n_out; ++i) dst[e + i] = v[i];
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       // the rows are reused by the next chunk
    }
}

// -------------------------------------------------------------------------------------- cepstrum
// One wavefront per frame, wavefronts loop over frames.  Hamming window, DFT of the N real samples, magnitudes of the
// first N/2 bins, triangular filterbank with stride L/2, ln(. + 1e-6), DCT-I as a K x K table product, drop 4, subtract
// the mean of what is left (spectrogram.rs:51-79).  The DFT is an autosort (Stockham) FFT in LDS, radix-4 passes, when N is a power of two and
// the defining sum X_k = sum_s x_s e^(-2 pi i k s / N) otherwise (rustfft plans any length, spectrogram.rs:44-48; the
// reference's shipped window is 256).  The tables live in LDS, loaded once per workgroup; the wavefronts of a workgroup
// never exchange data, so the stages are ordered by the wavefront's own in-order LDS queue, not by barriers.
// Power-of-two windows: radix-4 passes, and each HALF of a wavefront (32 lanes) transforms a frame of its own.
// A workgroup has 1 - 4 wavefronts, as many as the plan fits into 160 KiB of LDS; when the K x K DCT table does not fit
// beside one frame slot (large K), it stays in global memory (L2) and only the other tables are copied.
// What a cepstrum frame needs whatever its samples come from: the geometry, the LDS layout of a workgroup and the tables.
struct CepsGeom {
    uint32_t fft, step, L, fstep, K, log2n;   // log2n == 0: N is not a power of two, direct DFT
    uint32_t frames_per_wave;  // 2: each half of a wavefront transforms a frame of its own (power-of-two windows whose slots fit in LDS); else 1
    uint32_t waves;            // wavefronts per workgroup, 1 .. 4 (blockDim.x / 64)
    uint32_t dct_lds;          // 1: the DCT table is copied to LDS; 0: it is read from global memory
    uint32_t tw_lds;           // float offset of the twiddle table in LDS (even: 8-byte aligned)
    uint32_t slot_floats;      // floats per frame slot (even)
    const float *hamming;      // [fft]
    const float *triag;        // [L]
    const float2 *twiddle;     // power of two: [fft/2] exp(-2 pi i k / fft); else [fft] exp(-2 pi i t / fft)
    const float *dct;          // [K][K]   DCT-I table incl. the 1/2 weights of the end points
};

struct CepsParams : CepsGeom {
    const int16_t *samples;
    const uint64_t *sample_off;   // [n_seq+1] first sample of every recording
    const uint64_t *frame_off;    // [n_seq+1] first output frame of every recording
    uint32_t n_seq;
    uint64_t n_frames;
    float *out;                // [n_frames][K-4]
};

#define APD_WAVE_LDS_FENCE() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")

__device__ __forceinline__ float2 cmul(const float2 a, const float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

// The tables of a workgroup in LDS: hamming[N], triag[L], dct[K][K] (when the plan keeps it in LDS), twiddles at G.tw_lds; the
// frame slots follow the twiddles.  Copied by the whole workgroup, which meets at the barrier at the end.
struct CepsTables {
    float *ham, *tri, *dct;
    float2 *tw;
    float *slots;
};
__device__ __forceinline__ CepsTables load_ceps_tables(const CepsGeom &G, float *lds)
{
    const uint32_t N = G.fft, K = G.K, n_tw = G.log2n ? N / 2 : N;
    CepsTables T;
    T.ham = lds; T.tri = T.ham + N; T.dct = T.tri + G.L;
    T.tw = reinterpret_cast<float2 *>(lds + G.tw_lds);
    T.slots = reinterpret_cast<float *>(T.tw + n_tw);
    for (uint32_t e = threadIdx.x; e < N; e += blockDim.x) T.ham[e] = G.hamming[e];
    for (uint32_t e = threadIdx.x; e < G.L; e += blockDim.x) T.tri[e] = G.triag[e];
    if (G.dct_lds)
        for (uint32_t e = threadIdx.x; e < K * K; e += blockDim.x) T.dct[e] = G.dct[e];
    for (uint32_t e = threadIdx.x; e < n_tw; e += blockDim.x) T.tw[e] = G.twiddle[e];
    __syncthreads();
    return T;
}

// A frame slot: FFT -- two complex buffers of N/2 (ping-pong), mag[half], conv[K], ceps[K]; direct sum -- N real samples,
// mag[half], conv[K], ceps[K].  Power-of-two windows: TWO slots per wavefront when they fit -- each half of the wave (32 lanes)
// transforms a frame of its own; else one.  `gsize` consecutive lanes own a slot, `gl` = lane within that group.
struct CepsSlot {
    float *base, *mag, *conv, *ceps;
    uint32_t gsize, gl, fs;
};
__device__ __forceinline__ CepsSlot ceps_slot(const CepsGeom &G, float *slots, int wave, int lane)
{
    CepsSlot S;
    S.gsize = 64u / G.frames_per_wave; S.gl = (uint32_t)lane % S.gsize; S.fs = (uint32_t)lane / S.gsize;   // lane group = frame slot
    S.base = slots + ((size_t)wave * G.frames_per_wave + S.fs) * G.slot_floats;
    S.mag = S.base + (G.log2n ? 2 * G.fft : G.fft); S.conv = S.mag + G.fft / 2; S.ceps = S.conv + G.K;
    return S;
}

// From the samples of one window to the magnitudes of its first N/2 bins in S.mag: Hamming window, then the real-packed Stockham
// FFT or the defining sum (spectrogram.rs:55-63).  fetch.one(s): sample s of the window, s in [0, N); fetch.two(s, a, b): samples s
// and s + 1, s even -- the FFT packs them into one complex value, and a source that holds them side by side loads them at once.
// Executed by the slot's lane group; the caller fences behind it.  A group without a frame (`live` false) transforms zeros and
// fetches nothing.
template <typename Fetch>
__device__ __forceinline__ void frame_magnitudes(const CepsGeom &G, const CepsTables &T, const CepsSlot &S, int lane, bool live, Fetch fetch)
{
    const uint32_t N = G.fft, half = N / 2, gl = S.gl, gsize = S.gsize;
    const float *t_ham = T.ham;
    const float2 *t_tw = T.tw;
    float *mag = S.mag;
    if (G.log2n) {
        // real input: the N samples are packed as M = N/2 complex values z[s] = x[2s] + i x[2s+1], one M-point FFT is
        // run (half the butterflies and half the LDS traffic of an N-point transform of zero-imaginary data), and the
        // N-point spectrum of the real signal follows from Z[k] and conj(Z[M-k]).  The M-point transform is an autosort
        // (Stockham) FFT in radix-4 passes with one radix-2 pass at the end when log2(M) is odd: M = 128 takes 4 LDS round
        // trips instead of 7, and a radix-4 pass of 32 butterflies is exactly one half-wave.
        float2 *bufa = reinterpret_cast<float2 *>(S.base), *bufb = bufa + half;
        const uint32_t M = half, m = G.log2n - 1u, n4 = m / 2u;
        for (uint32_t s = gl; s < M; s += gsize) {
            float2 z = make_float2(0.0f, 0.0f);
            if (live) {
                int16_t a, b;
                fetch.two(2 * s, a, b);
                z = make_float2((float)a * t_ham[2 * s], (float)b * t_ham[2 * s + 1]);   // :55-59
            }
            bufa[s] = z;
        }
        APD_WAVE_LDS_FENCE();
        float2 *src = bufa, *dst = bufb;
        uint32_t Ns = 1;
        for (uint32_t st = 0; st < n4; ++st) {
            const uint32_t q = M / 4u;
            for (uint32_t j = gl; j < q; j += gsize) {
                const uint32_t k = j & (Ns - 1u);
                const float2 w1 = t_tw[k * (half / 2u / Ns)];   // exp(-2 pi i k / (4 Ns))
                const float2 w2 = t_tw[k * (half / Ns)];        // its square
                const float2 w3 = cmul(w1, w2);
                const float2 v0 = src[j], v1 = cmul(src[j + q], w1), v2 = cmul(src[j + 2u * q], w2), v3 = cmul(src[j + 3u * q], w3);
                const float2 a0 = make_float2(v0.x + v2.x, v0.y + v2.y), a1 = make_float2(v0.x - v2.x, v0.y - v2.y);
                const float2 a2 = make_float2(v1.x + v3.x, v1.y + v3.y), a3 = make_float2(v1.y - v3.y, v3.x - v1.x);   // -i (v1 - v3)
                const uint32_t idx = ((j - k) << 2) + k;
                dst[idx] = make_float2(a0.x + a2.x, a0.y + a2.y);
                dst[idx + Ns] = make_float2(a1.x + a3.x, a1.y + a3.y);
                dst[idx + 2u * Ns] = make_float2(a0.x - a2.x, a0.y - a2.y);
                dst[idx + 3u * Ns] = make_float2(a1.x - a3.x, a1.y - a3.y);
            }
            APD_WAVE_LDS_FENCE();
            float2 *tmp = src; src = dst; dst = tmp;
            Ns <<= 2;
        }
        if (m & 1u) {                                           // the last, radix-2 pass: Ns = M / 2
            const uint32_t hm = M / 2u;
            for (uint32_t j = gl; j < hm; j += gsize) {
                const uint32_t k = j & (Ns - 1u);
                const float2 p = src[j], qv = cmul(src[j + hm], t_tw[k * (half / Ns)]);   // exp(-2 pi i k / (2 Ns))
                const uint32_t idx = ((j - k) << 1) + k;
                dst[idx] = make_float2(p.x + qv.x, p.y + qv.y);
                dst[idx + Ns] = make_float2(p.x - qv.x, p.y - qv.y);
            }
            APD_WAVE_LDS_FENCE();
            float2 *tmp = src; src = dst; dst = tmp;
        }
        for (uint32_t k = gl; k < M; k += gsize) {
            const float2 zk = src[k], zm = src[(M - k) & (M - 1)], w = t_tw[k];   // w = exp(-2 pi i k / N)
            const float ax = 0.5f * (zk.x + zm.x), ay = 0.5f * (zk.y - zm.y);     // (Z[k] + conj Z[M-k]) / 2
            const float bx = zk.x - zm.x, by = zk.y + zm.y;                       //  Z[k] - conj Z[M-k]
            const float xr = ax + 0.5f * (w.x * by + w.y * bx), xi = ay - 0.5f * (w.x * bx - w.y * by);
            mag[k] = sqrtf(xr * xr + xi * xi);                                    // norm_sqr().sqrt() (:63)
        }
    } else {
        float *win = S.base;                                   // N windowed samples; one frame per wavefront, always live
        for (uint32_t s = lane; s < N; s += 64) win[s] = (float)fetch.one(s) * t_ham[s];
        APD_WAVE_LDS_FENCE();
        for (uint32_t k = lane; k < half; k += 64) {           // X_k = sum_s x_s (cos - i sin)(2 pi k s / N)
            float re = 0.0f, im = 0.0f;
            uint32_t idx = 0;                                  // (k * s) mod N
            for (uint32_t s = 0; s < N; ++s) {
                const float2 w = t_tw[idx];
                const float x = win[s];
                re = fmaf(x, w.x, re);
                im = fmaf(x, w.y, im);
                idx += k;
                if (idx >= N) idx -= N;
            }
            mag[k] = sqrtf(re * re + im * im);
        }
    }
}

// From the magnitudes of one frame (mag[0 .. N/2) in LDS) to its output row: triangular filterbank with stride L/2, ln(. + 1e-6),
// DCT-I as a K x K table product, drop 4, subtract the mean of what is left (spectrogram.rs:66-79).  Executed by `gsize`
// consecutive lanes (a whole wavefront, or one half of it), `gl` = lane within that group; the caller fences before and after.
// sink(b, v): bin b of the row, called by the lane that owns it, live groups only.
template <typename Sink>
__device__ __forceinline__ void finish_frame(const CepsGeom &P, const float *t_tri, const float *t_dct, const float *mag, float *conv,
                                             float *ceps, uint32_t gl, uint32_t gsize, bool live, Sink sink)
{
    const uint32_t K = P.K;
    for (uint32_t c = gl; c < K; c += gsize) {                 // convolve (numerics.rs:102-109)
        const uint32_t p = P.L + c * P.fstep;
        float dot = 0.0f;
#pragma unroll 4
        for (uint32_t q = 0; q < P.L; ++q) dot = dot + t_tri[q] * mag[p - P.L + q];
        conv[c] = logf(dot + 1e-6f);                           // :69
    }
    APD_WAVE_LDS_FENCE();
    for (uint32_t k = gl; k < K; k += gsize) {                 // DCT-I (:71-73)
        float acc = 0.0f;
#pragma unroll 4
        for (uint32_t q = 0; q < K; ++q) acc = acc + t_dct[k * K + q] * conv[q];
        ceps[k] = acc;
    }
    APD_WAVE_LDS_FENCE();
    float mu = 0.0f;
#pragma unroll 4
    for (uint32_t k = 4; k < K; ++k) mu = mu + ceps[k];        // mean of cepstrum[4..] (:74, numerics.rs:12-18)
    mu = mu / (float)(K - 4);
    if (live)
        for (uint32_t k = 4 + gl; k < K; k += gsize) sink(k - 4, ceps[k] - mu);   // :75-79
}

// One frame, from its samples to its row; the body both kernels below run.
template <typename Fetch, typename Sink>
__device__ __forceinline__ void cepstrum_frame(const CepsGeom &G, const CepsTables &T, const CepsSlot &S, int lane, bool live, Fetch fetch, Sink sink)
{
    frame_magnitudes(G, T, S, lane, live, fetch);
    APD_WAVE_LDS_FENCE();
    if (G.dct_lds) finish_frame(G, T.tri, T.dct, S.mag, S.conv, S.ceps, S.gl, S.gsize, live, sink);   // two copies, so that each reads
    else finish_frame(G, T.tri, G.dct, S.mag, S.conv, S.ceps, S.gl, S.gsize, live, sink);            // its table through one address space
    APD_WAVE_LDS_FENCE();                                      // the buffers are reused by this lane group's next frame
}

// A window that lies in one array.
struct ArrayFetch {
    const int16_t *window;
    __device__ __forceinline__ int16_t one(uint32_t s) const { return window[s]; }
    __device__ __forceinline__ void two(uint32_t s, int16_t &a, int16_t &b) const { a = window[s]; b = window[s + 1]; }
};

__global__ __launch_bounds__(256) void cepstrum_kernel(const CepsParams P)
{
    extern __shared__ float lds[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const CepsTables T = load_ceps_tables(P, lds);
    const CepsSlot S = ceps_slot(P, T.slots, wave, lane);
    const uint32_t slots = P.frames_per_wave, fs = S.fs, K = P.K;
    // A wavefront takes a CONTIGUOUS run of frames: consecutive frames of a recording overlap (dft_step < dft_win: their samples
    // come from L2 the second time) and the recording index only ever steps forward (one binary search per run, not per frame).
    const uint64_t n_waves = (uint64_t)gridDim.x * P.waves, per_wave = (P.n_frames + n_waves - 1) / n_waves;
    const uint64_t f_begin = ((uint64_t)blockIdx.x * P.waves + wave) * per_wave, f_end = min(f_begin + per_wave, P.n_frames);
    // recording holding this group's first frame: largest s with frame_off[s] <= frame
    uint32_t lo = 0;
    const uint64_t f_first = f_begin + fs;
    if (f_first < f_end) {
        uint32_t hi = P.n_seq;
        while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (P.frame_off[mid] <= f_first) lo = mid; else hi = mid; }
    }
    uint64_t next_off = f_first < f_end ? P.frame_off[lo + 1] : 0, this_off = f_first < f_end ? P.frame_off[lo] : 0, samp0 = f_first < f_end ? P.sample_off[lo] : 0;
    for (uint64_t f0 = f_begin; f0 < f_end; f0 += slots) {
        const uint64_t frame = f0 + fs;
        const bool live = frame < f_end;                           // an odd run leaves the second half of the wave without a frame
        if (live)
            while (frame >= next_off) { ++lo; this_off = next_off; next_off = P.frame_off[lo + 1]; samp0 = P.sample_off[lo]; }   // recordings without frames are skipped
        const uint64_t start = live ? samp0 + (frame - this_off) * P.step : 0;   // i - fft_size, i = fft + t * step (:51-53)
        cepstrum_frame(P, T, S, lane, live, ArrayFetch{P.samples + start}, [&](uint32_t b, float v) { P.out[frame * (K - 4) + b] = v; });
    }
}

// The front end of an apd_feed: the new frames of one push, every channel's in one launch.  A channel's samples are a stream whose
// first `tail_len` come from the tail the last push left in HBM (tail_in) and whose rest is this push's chunk; the first new
// window starts `skip` samples into it (non-zero only when step > fft and the last push ended between two windows), and
// [keep_from, keep_from + keep_len) of it is what the next push will need: every workgroup copies its share of that into the
// OTHER tail buffer, which nothing in this launch reads.  A lane group takes a frame exactly as in cepstrum_kernel; with an
// encoder the finished row stays in the slot and the group runs AutoEncoder::predict on it (EncodeFrame::run_lanes).
struct FeedChan {
    uint64_t chunk_off, skip, keep_from;
    uint32_t tail_len, keep_len;
};
struct FeedParams : CepsGeom {
    const uint64_t *frame_off;    // [n_channels+1] first output row of every channel
    const FeedChan *chan;         // [n_channels]
    uint32_t n_channels;
    uint64_t n_frames;
    const int16_t *chunk;
    const int16_t *tail_in;       // [n_channels][fft]
    int16_t *tail_out;
    const float *wb;              // encoder: w[K-4][latent] then b[latent]; null: the rows are the cepstra
    uint32_t latent;
    uint32_t wb_lds;              // float offset of the encoder's weights in LDS (behind the frame slots)
    float *out;                   // [n_frames][latent or K-4]
};

__device__ __forceinline__ int16_t feed_sample(const FeedParams &P, const FeedChan &c, uint32_t channel, uint64_t p)
{
    return p < c.tail_len ? P.tail_in[(size_t)channel * P.fft + p] : P.chunk[c.chunk_off + (p - c.tail_len)];
}

// A window of a channel's stream [tail | chunk] that starts at its sample `start`.  A pair comes from one of the two in one load,
// except the one pair that straddles them.
struct FeedFetch {
    const int16_t *tail, *chunk;
    uint64_t start;
    uint32_t tail_len;
    __device__ __forceinline__ int16_t one(uint32_t s) const
    {
        const uint64_t p = start + s;
        return p < tail_len ? tail[p] : chunk[p - tail_len];
    }
    __device__ __forceinline__ void two(uint32_t s, int16_t &a, int16_t &b) const
    {
        const uint64_t p = start + s;
        if (p + 1 == tail_len) { a = tail[p]; b = chunk[0]; return; }
        const int16_t *pair = p < tail_len ? tail + p : chunk + (p - tail_len);
        a = pair[0]; b = pair[1];
    }
};

__global__ __launch_bounds__(256) void feed_frames_kernel(const FeedParams P)
{
    extern __shared__ float lds[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t d_in = P.K - 4, n_wb = P.wb ? d_in * P.latent + P.latent : 0;
    float *wb = lds + P.wb_lds;
    for (uint32_t e = threadIdx.x; e < n_wb; e += blockDim.x) wb[e] = P.wb[e];
    const CepsTables T = load_ceps_tables(P, lds);                 // ends in the workgroup's barrier
    const CepsSlot S = ceps_slot(P, T.slots, wave, lane);
    float *row = S.ceps + P.K, *pred = row + d_in;                  // the encoder's part of a slot
    const uint32_t slots = P.frames_per_wave, fs = S.fs, width = P.wb ? P.latent : d_in;
    const uint64_t n_waves = (uint64_t)gridDim.x * P.waves, per_wave = (P.n_frames + n_waves - 1) / n_waves;
    const uint64_t f_begin = ((uint64_t)blockIdx.x * P.waves + wave) * per_wave, f_end = min(f_begin + per_wave, P.n_frames);
    uint32_t lo = 0;                                               // channel holding this group's first frame
    const uint64_t f_first = f_begin + fs;
    if (f_first < f_end) {
        uint32_t hi = P.n_channels;
        while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (P.frame_off[mid] <= f_first) lo = mid; else hi = mid; }
    }
    uint64_t next_off = f_first < f_end ? P.frame_off[lo + 1] : 0, this_off = f_first < f_end ? P.frame_off[lo] : 0;
    FeedChan c = P.chan[f_first < f_end ? lo : 0];
    for (uint64_t f0 = f_begin; f0 < f_end; f0 += slots) {
        const uint64_t frame = f0 + fs;
        const bool live = frame < f_end;
        if (live)
            while (frame >= next_off) { ++lo; this_off = next_off; next_off = P.frame_off[lo + 1]; c = P.chan[lo]; }   // channels without new frames are skipped
        const uint64_t start = live ? c.skip + (frame - this_off) * P.step : 0;
        const FeedFetch fetch{P.tail_in + (size_t)lo * P.fft, P.chunk + c.chunk_off, start, c.tail_len};
        if (!P.wb) {
            cepstrum_frame(P, T, S, lane, live, fetch, [&](uint32_t b, float v) { P.out[frame * width + b] = v; });
        } else {
            cepstrum_frame(P, T, S, lane, live, fetch, [&](uint32_t b, float v) { row[b] = v; });   // fenced behind the row
            if (live)
                EncodeFrame::run_lanes(d_in, P.latent, wb, [&](uint32_t k) { return row[k]; }, [&](uint32_t j, float v) { P.out[frame * width + j] = v; },
                                       pred, S.gl, S.gsize);
            APD_WAVE_LDS_FENCE();
        }
    }
    // the tails of the next push, behind the frames: the first workgroups take them, and finish while later ones still transform
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < (uint64_t)P.n_channels * P.fft; e += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t channel = (uint32_t)(e / P.fft), i = (uint32_t)(e % P.fft);
        const FeedChan k = P.chan[channel];
        if (i < k.keep_len) P.tail_out[e] = feed_sample(P, k, channel, k.keep_from + i);
    }
}

}  // namespace

// ---- the feature stage as RESIDENT objects + enqueue-only calls -----------------------------------------------------------------
// The reference builds its features once per recording with par_iter (main.rs:150-161); a host that recomputes them per step (the
// benchmark's cfg 4 / cfg 5 step, or a pipeline over many corpora) calls these: the encoder weights / the cepstrum tables and
// offsets are uploaded ONCE into an object that lives on the context's GPU, and apd_encode_async / apd_cepstrum_batch_async only
// enqueue the kernel on the context's stream -- no allocation, no table building, no synchronisation.  With several GPUs every
// device runs the whole corpus' feature kernel concurrently (replicated, not sharded: the kernels take 0.15 ms (cfg 4) and 19 ms
// (cfg 5) for the WHOLE corpus, less than an all-gather of their 134 MB / 1.74 GB output over xGMI would).

struct apd_encoder : apd::ContextChild {
    apd::DeviceBuf d_w;               // floats: [d_in][latent] weights, then [latent] bias
    uint32_t d_in = 0, latent = 0;
    void release_device() override { d_w.reset(); }
};

struct apd_cepstrum_plan : apd::ContextChild {
    apd::DeviceBuf pool;              // tables | sample offsets | frame offsets
    CepsParams P{};                   // samples / out filled per call
    size_t lds_bytes = 0;
    unsigned blocks = 0;
    uint64_t n_samples = 0;
    void release_device() override { pool.reset(); }
};

extern "C" int apd_encoder_create(apd_context *ctx, const float *w_encode, const float *b_encode, uint32_t d_in, uint32_t latent, apd_encoder **out)
{
    if (!ctx || !w_encode || !b_encode || d_in == 0 || latent == 0 || !out) return APD_ERR_INVALID_ARG;
    *out = nullptr;
    const size_t wb_bytes = ((size_t)d_in * latent + latent) * sizeof(float);
    if (wb_bytes > 64 * 1024) return APD_ERR_UNSUPPORTED;
    HIP_TRY(ctx, apd::bind_device(ctx));
    apd_encoder *e = new (std::nothrow) apd_encoder();
    if (!e) return APD_ERR_OOM;
    e->ctx = ctx; e->d_in = d_in; e->latent = latent;
    hipError_t err = e->d_w.alloc(wb_bytes);
    float *d_w = e->d_w.as<float>();
    if (err == hipSuccess) err = hipMemcpyAsync(d_w, w_encode, (size_t)d_in * latent * sizeof(float), hipMemcpyHostToDevice, ctx->stream);
    if (err == hipSuccess) err = hipMemcpyAsync(d_w + (size_t)d_in * latent, b_encode, latent * sizeof(float), hipMemcpyHostToDevice, ctx->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(ctx->stream);      // the host arrays are the caller's: done with them on return
    if (err != hipSuccess) {
        ctx->last_error = std::string("apd_encoder_create: ") + hipGetErrorString(err);
        delete e;
        return err == hipErrorOutOfMemory ? APD_ERR_OOM : APD_ERR_HIP;
    }
    ctx->children.insert(e);
    *out = e;
    return APD_OK;
}

extern "C" int apd_encoder_destroy(apd_encoder *e) { return apd::destroy_child(e); }

// An encoder whose weights already lie in this context's HBM (apd_trainer_encoder, train.hip): copied device to device, so the
// source may change or go afterwards.
int apd::encoder_from_device(apd_context *ctx, const float *d_w_encode, const float *d_b_encode, uint32_t d_in, uint32_t latent, apd_encoder **out)
{
    *out = nullptr;
    const size_t w_bytes = (size_t)d_in * latent * sizeof(float), b_bytes = latent * sizeof(float);
    if (w_bytes + b_bytes > 64 * 1024) return APD_ERR_UNSUPPORTED;
    HIP_TRY(ctx, apd::bind_device(ctx));
    apd_encoder *e = new (std::nothrow) apd_encoder();
    if (!e) return APD_ERR_OOM;
    e->ctx = ctx; e->d_in = d_in; e->latent = latent;
    hipError_t err = e->d_w.alloc(w_bytes + b_bytes);
    if (err == hipSuccess) err = hipMemcpyAsync(e->d_w.ptr, d_w_encode, w_bytes, hipMemcpyDeviceToDevice, ctx->stream);
    if (err == hipSuccess) err = hipMemcpyAsync(e->d_w.as<char>() + w_bytes, d_b_encode, b_bytes, hipMemcpyDeviceToDevice, ctx->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(ctx->stream);
    if (err != hipSuccess) {
        ctx->last_error = std::string("apd_trainer_encoder: ") + hipGetErrorString(err);
        delete e;
        return err == hipErrorOutOfMemory ? APD_ERR_OOM : APD_ERR_HIP;
    }
    ctx->children.insert(e);
    *out = e;
    return APD_OK;
}

extern "C" int apd_encode_async(apd_context *ctx, const apd_encoder *e, const float *d_x, uint64_t t, float *d_out)
{
    if (!ctx || !e || e->ctx != ctx || (t && (!d_x || !d_out))) return APD_ERR_INVALID_ARG;
    if (t == 0) return APD_OK;
    HIP_TRY(ctx, apd::bind_device(ctx));
    APD_AFFINITY(ctx, "encoder launch");
    const uint32_t d_in = e->d_in, latent = e->latent;
    const float *d_w = e->d_w.as<float>();
    const unsigned blocks = (unsigned)std::min<uint64_t>((t + 255) / 256, 8192);
    // staged through LDS when the 4 x 64 staged rows fit next to the weights (they do for every shape the reference produces)
    const size_t staged_bytes = (((size_t)d_in * latent + latent + 3) & ~(size_t)3) * sizeof(float) +
                                4 * 64 * (size_t)((d_in | 1u) + (latent | 1u)) * sizeof(float);
    if (std::getenv("APD_DEBUG_PLAN"))                                  // as for the tile plans: the only report of which kernel ran
        std::fprintf(stderr, "[apd] encoder %u -> %u: %s, %zu bytes of LDS\n", d_in, latent, staged_bytes <= 64 * 1024 ? "staged" : "direct",
                     staged_bytes <= 64 * 1024 ? staged_bytes : ((size_t)d_in * latent + latent) * sizeof(float));
    if (staged_bytes <= 64 * 1024)
        hipLaunchKernelGGL(encode_staged_kernel, dim3(blocks), dim3(256), staged_bytes, ctx->stream, d_x, t, d_in, d_w,
                           d_w + (size_t)d_in * latent, latent, d_out);
    else
        hipLaunchKernelGGL(encode_kernel, dim3(blocks), dim3(256), ((size_t)d_in * latent + latent) * sizeof(float), ctx->stream, d_x, t, d_in, d_w,
                           d_w + (size_t)d_in * latent, latent, d_out);
    HIP_TRY(ctx, hipGetLastError());
    return APD_OK;
}

// The encoder over host arrays (through temporary device buffers) or device arrays (as they are); blocking either way.
static int encode_blocking(apd_context *ctx, const apd_encoder *e, const float *x, uint64_t t, int on_device, float *out)
{
    apd::DeviceBuf d_x, d_out;
    const size_t in_bytes = t * e->d_in * sizeof(float), out_bytes = t * e->latent * sizeof(float);
    if (!on_device) {
        HIP_TRY(ctx, d_x.alloc(in_bytes));
        HIP_TRY(ctx, d_out.alloc(out_bytes));
        HIP_TRY(ctx, hipMemcpyAsync(d_x.ptr, x, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    }
    if (const int rc = apd_encode_async(ctx, e, on_device ? x : d_x.as<float>(), t, on_device ? out : d_out.as<float>())) return rc;
    if (!on_device) HIP_TRY(ctx, hipMemcpyAsync(out, d_out.ptr, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return APD_OK;
}

// The one-call form (host or device arrays): an encoder object made, used and dropped inside the call; blocking.
extern "C" int apd_encode(apd_context *ctx, const float *x, uint64_t t, uint32_t d_in, const float *w_encode,
                          const float *b_encode, uint32_t latent, int on_device, float *out)
{
    if (!ctx || !w_encode || !b_encode || d_in == 0 || latent == 0 || (t && (!x || !out))) return APD_ERR_INVALID_ARG;
    if (((size_t)d_in * latent + latent) * sizeof(float) > 64 * 1024) return APD_ERR_UNSUPPORTED;
    if (t == 0) return APD_OK;
    apd_encoder *e = nullptr;
    int rc = apd_encoder_create(ctx, w_encode, b_encode, d_in, latent, &e);
    if (rc != APD_OK) return rc;
    rc = encode_blocking(ctx, e, x, t, on_device, out);
    apd_encoder_destroy(e);                                               // waits for the stream, also after a failure
    return rc;
}

// i in (fft_size..n).step_by(step), spectrogram.rs:51: the window that ends exactly at sample n is not produced.
extern "C" uint64_t apd_cepstrum_frames(uint64_t n_samples, uint32_t fft_size, uint32_t fft_step)
{
    return fft_step && n_samples > fft_size ? (n_samples - fft_size + fft_step - 1) / fft_step : 0;
}

// The filterbank outputs K of a window (numerics.rs:105) and the limits every cepstrum call shares: pure host arithmetic.
static int cepstrum_bins(uint32_t fft_size, uint32_t fft_step, uint32_t filter_size, uint32_t *K_out)
{
    if (fft_size < 2 || fft_step == 0 || filter_size == 0) return APD_ERR_INVALID_ARG;
    const uint32_t L = fft_size / filter_size, half = fft_size / 2, fstep = L / 2;      // spectrogram.rs:38,64,67
    if (L == 0 || fstep == 0) return APD_ERR_INVALID_ARG;                               // step_by(0) panics in the reference
    uint32_t K = 0;
    for (uint32_t i = L; i < half; i += fstep) ++K;                                     // numerics.rs:105
    if (K < 5) return APD_ERR_INVALID_ARG;                                              // cepstrum[4..] of an empty tail
    if (fft_size > 4096 || K > 512) return APD_ERR_UNSUPPORTED;                         // the limits of include/apd.h, apd_cepstrum
    *K_out = K;
    return APD_OK;
}

// Frame offsets and bin count of a corpus (spectrogram.rs:51, numerics.rs:105): pure host arithmetic.
static int cepstrum_geometry(const uint64_t *sample_off, uint32_t n_seq, uint32_t fft_size, uint32_t fft_step, uint32_t filter_size,
                             uint64_t *frame_off, uint32_t *n_bins, uint32_t *K_out)
{
    if (!sample_off || !frame_off || !n_bins) return APD_ERR_INVALID_ARG;
    uint32_t K = 0;
    if (const int rc = cepstrum_bins(fft_size, fft_step, filter_size, &K)) return rc;
    frame_off[0] = 0;
    for (uint32_t s = 0; s < n_seq; ++s) {
        if (sample_off[s + 1] < sample_off[s]) return APD_ERR_INVALID_ARG;
        frame_off[s + 1] = frame_off[s] + apd_cepstrum_frames(sample_off[s + 1] - sample_off[s], fft_size, fft_step);
    }
    *n_bins = K - 4;
    *K_out = K;
    return APD_OK;
}

// The tables of a window as the reference computes them, in one host array: hamming[fft] | triag[L] | dct[K][K] | pad to 8 bytes |
// twiddles; and where they lie in it.
struct CepsHostTables {
    std::vector<float> tab;
    size_t tw_off = 0;            // floats
    uint32_t L = 0, fstep = 0, log2n = 0, n_tw = 0;
};
static CepsHostTables cepstrum_tables(uint32_t fft_size, uint32_t filter_size, uint32_t K)
{
    CepsHostTables H;
    const uint32_t L = fft_size / filter_size, half = fft_size / 2;
    uint32_t log2n = 0;
    while ((1u << log2n) < fft_size) ++log2n;
    if ((1u << log2n) != fft_size) log2n = 0;                                           // not a power of two: the defining sum
    const uint32_t n_tw = log2n ? half : fft_size;
    H.L = L; H.fstep = L / 2; H.log2n = log2n; H.n_tw = n_tw;
    H.tw_off = ((size_t)fft_size + L + (size_t)K * K + 1) & ~(size_t)1;                 // float2 table: 8-byte aligned
    H.tab.assign(H.tw_off + 2 * (size_t)n_tw, 0.0f);
    float *hamming = H.tab.data(), *triag = hamming + fft_size, *dct = triag + L;
    float2 *tw = reinterpret_cast<float2 *>(H.tab.data() + H.tw_off);
    for (uint32_t i = 0; i < fft_size; ++i) {                                           // numerics.rs:60-66
        const float arg = (2.0f * 3.14159265358979323846f * (float)i) / (float)fft_size;
        hamming[i] = 0.54f + 0.46f * cosf(arg);
    }
    for (uint32_t i = 0; i < L; ++i) triag[i] = 0.0f;                                   // numerics.rs:78-86
    for (uint32_t i = 0; i <= (L - 1) / 2; ++i) { triag[i] = (float)i / (float)L; triag[L - 1 - i] = (float)i / (float)L; }
    for (uint32_t k = 0; k < K; ++k)                                                    // rustdct DCT-I definition
        for (uint32_t q = 0; q < K; ++q) {
            double c;
            if (q == 0) c = 0.5;
            else if (q == K - 1) c = (k & 1) ? -0.5 : 0.5;
            else c = std::cos(M_PI * (double)q * (double)k / (double)(K - 1));
            dct[(size_t)k * K + q] = (float)c;
        }
    for (uint32_t k = 0; k < n_tw; ++k) {
        const double a = -2.0 * M_PI * (double)k / (double)fft_size;
        tw[k] = make_float2((float)std::cos(a), (float)std::sin(a));
    }
    return H;
}

// The geometry of a plan over tables resident at d_tab, and the LDS of a workgroup laid out as the kernels read it: hamming | triag |
// dct (if kept in LDS) | twiddles, then waves x frames_per_wave frame slots, then `behind` floats (a feed's encoder).  The FFT slot
// holds two complex ping-pong buffers of N/2, the direct sum's N real samples; `slot_extra` floats follow either.  Returns the
// bytes of LDS; more than 160 KiB: the plan does not run.
static size_t cepstrum_layout(CepsGeom &G, const CepsHostTables &H, const float *d_tab, uint32_t fft_size, uint32_t fft_step, uint32_t K,
                              size_t slot_extra, size_t behind)
{
    const uint32_t L = H.L, half = fft_size / 2, log2n = H.log2n, n_tw = H.n_tw;
    G.fft = fft_size; G.step = fft_step; G.L = L; G.fstep = H.fstep; G.K = K; G.log2n = log2n;
    G.hamming = d_tab; G.triag = d_tab + fft_size; G.dct = d_tab + fft_size + L;
    G.twiddle = reinterpret_cast<const float2 *>(d_tab + H.tw_off);
    const size_t lds_cap = 160 * 1024 / sizeof(float);
    auto table_floats = [&](bool dct) { return (((size_t)fft_size + L + (dct ? (size_t)K * K : 0) + 1) & ~(size_t)1) + 2 * (size_t)n_tw + behind; };
    const size_t slot_floats = ((log2n ? 2 : 1) * (size_t)fft_size + half + 2 * K + slot_extra + 1) & ~(size_t)1;
    // two frames per wavefront for power-of-two windows, if eight slots fit beside the tables (windows up to 1024 do)
    G.frames_per_wave = (log2n && (table_floats(true) + 8 * slot_floats) * sizeof(float) <= 96 * 1024) ? 2u : 1u;
    // the DCT table in LDS if it fits beside one wavefront's slots, else read from global memory; then as many wavefronts (up
    // to 4) as fit.  fft_size <= 4096 and K <= 512 always fit one wavefront: under 77 KiB without the DCT table.
    G.dct_lds = table_floats(true) + G.frames_per_wave * slot_floats <= lds_cap ? 1u : 0u;
    const size_t tables = table_floats(G.dct_lds != 0);
    G.waves = 4;
    while (G.waves > 1 && tables + (size_t)G.waves * G.frames_per_wave * slot_floats > lds_cap) --G.waves;
    G.tw_lds = (uint32_t)(tables - behind - 2 * (size_t)n_tw);
    G.slot_floats = (uint32_t)slot_floats;
    return (tables + (size_t)G.waves * G.frames_per_wave * slot_floats) * sizeof(float);
}

// the attribute belongs to the kernel, not to the plan: raised to the most any plan asks for, so plans of any size may alternate
static bool cepstrum_lds_granted(const void *kernel, size_t lds_bytes)
{
    return lds_bytes <= 64 * 1024 || hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess;
}

extern "C" int apd_cepstrum_plan_create(apd_context *ctx, const uint64_t *sample_off, uint32_t n_seq, uint32_t fft_size, uint32_t fft_step,
                                        uint32_t filter_size, uint64_t *frame_off, uint32_t *n_bins, apd_cepstrum_plan **out)
{
    if (!ctx || !out) return APD_ERR_INVALID_ARG;
    *out = nullptr;
    uint32_t K = 0;
    int rc = cepstrum_geometry(sample_off, n_seq, fft_size, fft_step, filter_size, frame_off, n_bins, &K);
    if (rc != APD_OK) return rc;
    const uint64_t T = frame_off[n_seq];
    HIP_TRY(ctx, apd::bind_device(ctx));
    const CepsHostTables H = cepstrum_tables(fft_size, filter_size, K);
    apd_cepstrum_plan *plan = new (std::nothrow) apd_cepstrum_plan();
    if (!plan) return APD_ERR_OOM;
    plan->ctx = ctx;
    plan->n_samples = sample_off[n_seq];
    const size_t tab_bytes = H.tab.size() * sizeof(float), off_bytes = 2 * ((size_t)n_seq + 1) * sizeof(uint64_t);
    const size_t offs_off = (tab_bytes + 255) & ~(size_t)255;
    hipError_t err = plan->pool.alloc(offs_off + off_bytes + 256);
    char *pool = plan->pool.as<char>();
    if (err == hipSuccess) err = hipMemcpyAsync(pool, H.tab.data(), tab_bytes, hipMemcpyHostToDevice, ctx->stream);
    if (err == hipSuccess) err = hipMemcpyAsync(pool + offs_off, sample_off, off_bytes / 2, hipMemcpyHostToDevice, ctx->stream);
    if (err == hipSuccess) err = hipMemcpyAsync(pool + offs_off + off_bytes / 2, frame_off, off_bytes / 2, hipMemcpyHostToDevice, ctx->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(ctx->stream);                     // the tables and the caller's offsets are free after this
    CepsParams &P = plan->P;
    P.sample_off = reinterpret_cast<const uint64_t *>(pool + offs_off);
    P.frame_off = P.sample_off + n_seq + 1;
    P.n_seq = n_seq; P.n_frames = T;
    plan->lds_bytes = cepstrum_layout(P, H, reinterpret_cast<const float *>(pool), fft_size, fft_step, K, 0, 0);
    // wavefronts loop over frames: enough workgroups to fill the GPU several times over, tables loaded once per workgroup
    const uint32_t per_block = P.waves * P.frames_per_wave;
    plan->blocks = (unsigned)std::min<uint64_t>((T + per_block - 1) / per_block, 256 * 16);
    int status = APD_OK;
    if (err != hipSuccess) { ctx->last_error = std::string("apd_cepstrum_plan_create: ") + hipGetErrorString(err); status = err == hipErrorOutOfMemory ? APD_ERR_OOM : APD_ERR_HIP; }
    else if (plan->lds_bytes > 160 * 1024) status = APD_ERR_UNSUPPORTED;
    else if (!cepstrum_lds_granted(reinterpret_cast<const void *>(cepstrum_kernel), plan->lds_bytes)) {
        ctx->last_error = "apd_cepstrum_plan_create: the runtime refused the kernel its LDS";
        status = APD_ERR_HIP;
    }
    if (status != APD_OK) { delete plan; return status; }
    ctx->children.insert(plan);
    *out = plan;
    return APD_OK;
}

extern "C" int apd_cepstrum_plan_destroy(apd_cepstrum_plan *plan) { return apd::destroy_child(plan); }

extern "C" int apd_cepstrum_batch_async(apd_context *ctx, const apd_cepstrum_plan *plan, const int16_t *d_samples, float *d_out)
{
    if (!ctx || !plan || plan->ctx != ctx) return APD_ERR_INVALID_ARG;
    if (plan->P.n_frames == 0) return APD_OK;
    if (!d_samples || !d_out) return APD_ERR_INVALID_ARG;
    HIP_TRY(ctx, apd::bind_device(ctx));
    APD_AFFINITY(ctx, "cepstrum launch");
    CepsParams P = plan->P;
    P.samples = d_samples; P.out = d_out;
    hipLaunchKernelGGL(cepstrum_kernel, dim3(plan->blocks), dim3(64 * P.waves), plan->lds_bytes, ctx->stream, P);
    HIP_TRY(ctx, hipGetLastError());
    return APD_OK;
}

// The plan over host arrays (through temporary device buffers) or device arrays (as they are); blocking either way.
static int cepstrum_blocking(apd_context *ctx, const apd_cepstrum_plan *plan, const int16_t *samples, size_t in_bytes, int on_device,
                             float *out, size_t out_bytes)
{
    apd::DeviceBuf d_in, d_o;
    if (!on_device) {
        HIP_TRY(ctx, d_in.alloc(in_bytes));
        HIP_TRY(ctx, d_o.alloc(out_bytes));
        HIP_TRY(ctx, hipMemcpyAsync(d_in.ptr, samples, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    }
    if (const int rc = apd_cepstrum_batch_async(ctx, plan, on_device ? samples : d_in.as<int16_t>(), on_device ? out : d_o.as<float>())) return rc;
    if (!on_device) HIP_TRY(ctx, hipMemcpyAsync(out, d_o.ptr, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return APD_OK;
}

// The one-call forms: a plan made, used and dropped inside the call; host or device arrays; blocking.
static int cepstrum_impl(apd_context *ctx, const int16_t *samples, const uint64_t *sample_off, uint32_t n_seq, uint32_t fft_size,
                         uint32_t fft_step, uint32_t filter_size, int on_device, float *out, uint64_t *frame_off, uint32_t *n_bins)
{
    if (!ctx) return APD_ERR_INVALID_ARG;
    uint32_t K = 0;
    int rc = cepstrum_geometry(sample_off, n_seq, fft_size, fft_step, filter_size, frame_off, n_bins, &K);
    if (rc != APD_OK) return rc;
    const uint64_t T = frame_off[n_seq], n_samples = sample_off[n_seq];
    if (!out || T == 0) return APD_OK;
    if (!samples) return APD_ERR_INVALID_ARG;
    apd_cepstrum_plan *plan = nullptr;
    rc = apd_cepstrum_plan_create(ctx, sample_off, n_seq, fft_size, fft_step, filter_size, frame_off, n_bins, &plan);
    if (rc != APD_OK) return rc;
    rc = cepstrum_blocking(ctx, plan, samples, n_samples * sizeof(int16_t), on_device, out, T * (K - 4) * sizeof(float));
    apd_cepstrum_plan_destroy(plan);                                      // waits for the stream, also after a failure
    return rc;
}

extern "C" int apd_cepstrum(apd_context *ctx, const int16_t *samples, uint64_t n_samples, uint32_t fft_size,
                            uint32_t fft_step, uint32_t filter_size, int on_device, float *out, uint64_t *n_frames,
                            uint32_t *n_bins)
{
    if (!n_frames) return APD_ERR_INVALID_ARG;
    const uint64_t sample_off[2] = {0, n_samples};
    uint64_t frame_off[2] = {0, 0};
    const int rc = cepstrum_impl(ctx, samples, sample_off, 1, fft_size, fft_step, filter_size, on_device, out, frame_off, n_bins);
    *n_frames = frame_off[1];
    return rc;
}

extern "C" int apd_cepstrum_batch(apd_context *ctx, const int16_t *samples, const uint64_t *sample_offsets, uint32_t n_seq,
                                  uint32_t fft_size, uint32_t fft_step, uint32_t filter_size, int on_device, float *out,
                                  uint64_t *frame_offsets, uint32_t *n_bins)
{
    return cepstrum_impl(ctx, samples, sample_offsets, n_seq, fft_size, fft_step, filter_size, on_device, out, frame_offsets, n_bins);
}

// ---- the resident front end of a live feed: apd_feed (include/apd.h, "raw audio in chunks"; kernel: feed_frames_kernel) -----------
// The tables of a cepstrum plan without a corpus' offsets, a copy of the encoder's weights, and per channel what a push carries to
// the next: the samples from the start of the next window on (at most fft_size of them, in one of two tail buffers in HBM) or, when
// fft_step > fft_size, how many samples are still to be skipped.  All of it is worked out on the host, which sees every length.
struct apd_feed : apd::ContextChild {
    apd::DeviceBuf pool;              // tables | encoder weights | tails [2][n_channels][fft] | frame_off [n_channels+1] | FeedChan [n_channels]
    apd::DeviceBuf d_in;              // host samples on their way to the kernel
    apd::DeviceBuf d_out;             // rows on their way to the host, or to a session (apd_spot_stream_push_audio)
    FeedParams P{};                   // per-push fields filled per call
    size_t lds_bytes = 0;
    uint32_t n_channels = 0, dim = 0;
    int16_t *d_tail[2] = {nullptr, nullptr};
    uint32_t current = 0;             // the tail buffer the next push reads
    struct Channel { uint64_t samples = 0, frames = 0, skip = 0; uint32_t tail = 0; };
    std::vector<Channel> chan, next;  // since the reset; `next`: a push's result until it is launched
    std::vector<uint64_t> h_words;    // host image of frame_off | FeedChan, alive as long as the feed (the upload is asynchronous)
    size_t words_bytes() const { return ((size_t)n_channels + 1) * sizeof(uint64_t) + (size_t)n_channels * sizeof(FeedChan); }
    void release_device() override { pool.reset(); d_in.reset(); d_out.reset(); }
};

extern "C" int apd_feed_create(apd_context *ctx, uint32_t n_channels, uint32_t fft_size, uint32_t fft_step, uint32_t filter_size,
                               const apd_encoder *encoder, uint32_t *dim, apd_feed **out)
{
    if (!ctx || !dim || !out) return APD_ERR_INVALID_ARG;
    *out = nullptr;
    uint32_t K = 0;
    if (const int rc = cepstrum_bins(fft_size, fft_step, filter_size, &K)) return rc;
    if (n_channels == 0 || (encoder && (encoder->ctx != ctx || encoder->d_in != K - 4))) return APD_ERR_INVALID_ARG;
    HIP_TRY(ctx, apd::bind_device(ctx));
    APD_AFFINITY(ctx, "feed allocation");
    const CepsHostTables H = cepstrum_tables(fft_size, filter_size, K);
    apd_feed *f = new (std::nothrow) apd_feed();
    if (!f) return APD_ERR_OOM;
    f->ctx = ctx; f->n_channels = n_channels;
    const uint32_t latent = encoder ? encoder->latent : 0, n_wb = encoder ? (K - 4) * latent + latent : 0;
    f->dim = encoder ? latent : K - 4;
    f->chan.assign(n_channels, apd_feed::Channel());
    f->next = f->chan;
    f->h_words.assign(f->words_bytes() / sizeof(uint64_t), 0);
    auto round = [](size_t n) { return (n + 255) & ~(size_t)255; };
    const size_t tab_bytes = H.tab.size() * sizeof(float), wb_off = round(tab_bytes), tail_off = wb_off + round(n_wb * sizeof(float));
    const size_t tail_bytes = round((size_t)n_channels * fft_size * sizeof(int16_t)), words_off = tail_off + 2 * tail_bytes;
    hipError_t err = f->pool.alloc(words_off + round(f->words_bytes()));
    char *pool = f->pool.as<char>();
    if (err == hipSuccess) err = hipMemcpyAsync(pool, H.tab.data(), tab_bytes, hipMemcpyHostToDevice, ctx->stream);
    if (err == hipSuccess && encoder) err = hipMemcpyAsync(pool + wb_off, encoder->d_w.ptr, n_wb * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(ctx->stream);                     // the tables are free after this, and so is the encoder
    FeedParams &P = f->P;
    // a slot carries the finished row and the encoder's un-normalised values behind the cepstrum's own buffers; the weights lie behind the slots
    f->lds_bytes = cepstrum_layout(P, H, reinterpret_cast<const float *>(pool), fft_size, fft_step, K, encoder ? (K - 4) + latent : 0, n_wb);
    P.wb_lds = (uint32_t)(f->lds_bytes / sizeof(float) - n_wb);
    P.wb = encoder ? reinterpret_cast<const float *>(pool + wb_off) : nullptr;
    P.latent = latent;
    P.n_channels = n_channels;
    f->d_tail[0] = reinterpret_cast<int16_t *>(pool + tail_off);
    f->d_tail[1] = reinterpret_cast<int16_t *>(pool + tail_off + tail_bytes);
    P.frame_off = reinterpret_cast<const uint64_t *>(pool + words_off);
    P.chan = reinterpret_cast<const FeedChan *>(P.frame_off + n_channels + 1);
    int status = APD_OK;
    if (err != hipSuccess) { ctx->last_error = std::string("apd_feed_create: ") + hipGetErrorString(err); status = err == hipErrorOutOfMemory ? APD_ERR_OOM : APD_ERR_HIP; }
    else if (f->lds_bytes > 160 * 1024) status = APD_ERR_UNSUPPORTED;
    else if (!cepstrum_lds_granted(reinterpret_cast<const void *>(feed_frames_kernel), f->lds_bytes)) {
        ctx->last_error = "apd_feed_create: the runtime refused the kernel its LDS";
        status = APD_ERR_HIP;
    }
    if (status != APD_OK) { delete f; return status; }
    ctx->children.insert(f);
    *dim = f->dim;
    *out = f;
    return APD_OK;
}

extern "C" int apd_feed_destroy(apd_feed *feed) { return apd::destroy_child(feed); }

extern "C" int apd_feed_reset(apd_context *ctx, apd_feed *feed, uint32_t channel)
{
    if (!ctx || !feed || feed->ctx != ctx) return APD_ERR_INVALID_ARG;
    const bool all = channel == 0xFFFFFFFFu;
    if (!all && channel >= feed->n_channels) return APD_ERR_INVALID_ARG;
    for (uint32_t k = 0; k < feed->n_channels; ++k)
        if (all || k == channel) feed->chan[k] = apd_feed::Channel();                   // no tail, nothing to skip: the buffers are not read
    return APD_OK;
}

extern "C" int apd_feed_totals(const apd_feed *feed, uint32_t channel, uint64_t *samples, uint64_t *frames)
{
    if (!feed || !samples || !frames || channel >= feed->n_channels) return APD_ERR_INVALID_ARG;
    *samples = feed->chan[channel].samples;
    *frames = feed->chan[channel].frames;
    return APD_OK;
}

// The rows a push adds per channel (frame_off, always written) and its argument checks: host only, the state is not touched.
static int feed_rows(const apd_feed *f, const uint64_t *sample_off, uint64_t *frame_off)
{
    bool ascending = true;
    frame_off[0] = 0;
    for (uint32_t k = 0; k < f->n_channels; ++k) {
        const bool ok = sample_off[k + 1] >= sample_off[k];
        const apd_feed::Channel &c = f->chan[k];
        const uint64_t n1 = c.samples + (ok ? sample_off[k + 1] - sample_off[k] : 0);
        frame_off[k + 1] = frame_off[k] + (apd_cepstrum_frames(n1, f->P.fft, f->P.step) - c.frames);
        ascending = ascending && ok;
    }
    return ascending ? APD_OK : APD_ERR_INVALID_ARG;
}

// The launch of a push whose arguments feed_rows accepted: d_samples and d_rows on the device; the state moves on; no
// synchronisation.  A push without a sample changes nothing and launches nothing.
static int feed_launch(apd_context *ctx, apd_feed *f, const int16_t *d_samples, const uint64_t *sample_off, const uint64_t *frame_off, float *d_rows)
{
    const uint32_t n_ch = f->n_channels, step = f->P.step;
    if (sample_off[n_ch] == sample_off[0]) return APD_OK;
    uint64_t *h_frame_off = f->h_words.data();
    FeedChan *h_chan = reinterpret_cast<FeedChan *>(h_frame_off + n_ch + 1);
    for (uint32_t k = 0; k < n_ch; ++k) {
        const apd_feed::Channel &c = f->chan[k];
        apd_feed::Channel &n = f->next[k];
        const uint64_t len = sample_off[k + 1] - sample_off[k];
        n.samples = c.samples + len;
        n.frames = c.frames + (frame_off[k + 1] - frame_off[k]);
        // the channel's stream of this push: [tail | chunk], its first sample the recording's sample `origin`
        const uint64_t origin = c.samples - c.tail, window = n.frames * step;           // window: where the next push's first window starts
        FeedChan &d = h_chan[k];
        d.chunk_off = sample_off[k];
        d.skip = c.skip;
        d.tail_len = c.tail;
        if (window >= n.samples) { n.tail = 0; n.skip = window - n.samples; d.keep_from = 0; d.keep_len = 0; }
        else { n.tail = (uint32_t)(n.samples - window); n.skip = 0; d.keep_from = window - origin; d.keep_len = n.tail; }   // n.tail <= fft: apd_cepstrum_frames rounds up
        h_frame_off[k] = frame_off[k];
    }
    h_frame_off[n_ch] = frame_off[n_ch];
    APD_AFFINITY(ctx, "feed launch");
    HIP_TRY(ctx, hipMemcpyAsync(const_cast<uint64_t *>(f->P.frame_off), f->h_words.data(), f->words_bytes(), hipMemcpyHostToDevice, ctx->stream));
    FeedParams P = f->P;
    P.n_frames = frame_off[n_ch];
    P.chunk = d_samples;
    P.tail_in = f->d_tail[f->current];
    P.tail_out = f->d_tail[f->current ^ 1u];
    P.out = d_rows;
    const uint32_t per_block = P.waves * P.frames_per_wave;
    const unsigned blocks = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((P.n_frames + per_block - 1) / per_block, 256 * 16));
    if (ctx->timing) HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    hipLaunchKernelGGL(feed_frames_kernel, dim3(blocks), dim3(64 * P.waves), f->lds_bytes, ctx->stream, P);
    HIP_TRY(ctx, hipGetLastError());
    if (ctx->timing) { HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream)); ctx->timed = true; }
    f->chan.swap(f->next);
    f->current ^= 1u;
    return APD_OK;
}

// Samples from the host go through the feed's staging buffer; grown to the largest push seen, then reused.
static int feed_stage(apd_context *ctx, apd_feed *f, const int16_t *samples, const uint64_t *sample_off, int samples_on_device,
                      const int16_t **d_samples, std::vector<uint64_t> &rebased)
{
    const uint32_t n_ch = f->n_channels;
    *d_samples = samples;
    if (samples_on_device || sample_off[n_ch] == sample_off[0]) return APD_OK;
    const size_t bytes = (size_t)(sample_off[n_ch] - sample_off[0]) * sizeof(int16_t);
    HIP_TRY(ctx, f->d_in.reserve(bytes));
    HIP_TRY(ctx, hipMemcpyAsync(f->d_in.ptr, samples + sample_off[0], bytes, hipMemcpyHostToDevice, ctx->stream));
    rebased.resize(n_ch + 1);
    for (uint32_t k = 0; k <= n_ch; ++k) rebased[k] = sample_off[k] - sample_off[0];
    *d_samples = f->d_in.as<int16_t>();
    return APD_OK;
}

extern "C" int apd_feed_push(apd_context *ctx, apd_feed *feed, const int16_t *samples, const uint64_t *sample_off, int samples_on_device,
                             float *frames, int frames_on_device, uint64_t capacity, uint64_t *frame_off)
{
    if (!ctx || !feed || feed->ctx != ctx || !sample_off || !frame_off) return APD_ERR_INVALID_ARG;
    apd_feed *f = feed;
    const uint32_t n_ch = f->n_channels;
    if (const int rc = feed_rows(f, sample_off, frame_off)) return rc;
    if (!frames) return APD_OK;                                            // sizes only: the state is not advanced
    const uint64_t total = frame_off[n_ch];
    if (capacity < total || (sample_off[n_ch] > sample_off[0] && !samples)) return APD_ERR_INVALID_ARG;
    HIP_TRY(ctx, apd::bind_device(ctx));
    APD_AFFINITY(ctx, "feed push");
    const size_t out_bytes = (size_t)total * f->dim * sizeof(float);
    if (!frames_on_device && total) HIP_TRY(ctx, f->d_out.reserve(out_bytes));
    const int16_t *d_samples = nullptr;
    std::vector<uint64_t> rebased;
    if (const int rc = feed_stage(ctx, f, samples, sample_off, samples_on_device, &d_samples, rebased)) return rc;
    float *d_rows = frames_on_device ? frames : f->d_out.as<float>();
    if (const int rc = feed_launch(ctx, f, d_samples, rebased.empty() ? sample_off : rebased.data(), frame_off, d_rows)) return rc;
    if (!frames_on_device && total) HIP_TRY(ctx, hipMemcpyAsync(frames, d_rows, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));                       // blocking: the rows are the caller's, `samples` is free again
    return APD_OK;
}

// What apd_spot_stream_push_audio (apd_api.hip) needs of a feed.
void apd::feed_info(const apd_feed *feed, const apd_context **ctx, uint32_t *n_channels, uint32_t *dim)
{
    *ctx = feed->ctx; *n_channels = feed->n_channels; *dim = feed->dim;
}
int apd::feed_sizes(const apd_feed *feed, const uint64_t *sample_off, uint64_t *frame_off) { return feed_rows(feed, sample_off, frame_off); }
int apd::feed_enqueue(apd_context *ctx, apd_feed *feed, const int16_t *samples, const uint64_t *sample_off, int samples_on_device,
                      const uint64_t *frame_off, const float **d_rows)
{
    apd_feed *f = feed;
    const uint32_t n_ch = f->n_channels;
    if (sample_off[n_ch] > sample_off[0] && !samples) return APD_ERR_INVALID_ARG;
    // two rows of slack: the session's repack reads the chunk as one sequence with two sentinel frames behind it
    HIP_TRY(ctx, f->d_out.reserve((size_t)(frame_off[n_ch] + 2) * f->dim * sizeof(float)));
    const int16_t *d_samples = nullptr;
    std::vector<uint64_t> rebased;
    if (const int rc = feed_stage(ctx, f, samples, sample_off, samples_on_device, &d_samples, rebased)) return rc;
    *d_rows = f->d_out.as<float>();
    return feed_launch(ctx, f, d_samples, rebased.empty() ? sample_off : rebased.data(), frame_off, f->d_out.as<float>());
}
