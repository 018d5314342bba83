// The defined arithmetic of the autoencoder trainer, shared by the device kernel (train.hip), the host
// entry points (train_host.hip) and the single-thread restatement (tools/train_cpu.cpp).  Plain C++: no HIP type appears here.
// Every unit that includes it is built with -ffp-contract=off: each operation below is one IEEE f32 operation, round to nearest.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define APD_TRAIN_HD __host__ __device__
#else
#define APD_TRAIN_HD
#endif

namespace apd {

APD_TRAIN_HD inline float train_pow2(int k)   // 2^k for -126 <= k <= 127, from the exponent field
{
    const uint32_t bits = (uint32_t)(k + 127) << 23;
    float f;
    memcpy(&f, &bits, 4);
    return f;
}

// e ~ exp(t), within 2 ulp (measured: 0.97) wherever exp(t) is a normal f32.  Adds, subtractions, multiplications, comparisons, one
// float -> int conversion and two scalings by exact powers of two; no transcendental instruction, no libm.
//   t is clamped to [-104, 100] (a NaN passes the comparisons);
//   k  = round-to-nearest-even(t * log2 e), by adding and subtracting 1.5 * 2^23;
//   r  = (t - k * 0.693359375) - k * (-2.12194440e-4): the first product is exact (9 x 8 bits), |r| <= 0.35;
//   p  = 1 + (r + r^2 * P(r)), P the degree-5 polynomial of Cephes' expf, Horner, each step a multiply then an add;
//   e  = (p * 2^(k >> 1)) * 2^(k - (k >> 1)): one rounding at most (in the subnormal range), +inf above the f32 range.
APD_TRAIN_HD inline float train_exp(float t)
{
    float tc = t > 100.0f ? 100.0f : t;
    tc = tc < -104.0f ? -104.0f : tc;
    const float z = tc * 1.44269504f;
    const float kf = (z + 12582912.0f) - 12582912.0f;
    const float r = (tc - kf * 0.693359375f) - kf * -2.12194440e-4f;
    float p = 1.9875691500e-4f;
    p = p * r + 1.3981999507e-3f;
    p = p * r + 8.3334519073e-3f;
    p = p * r + 4.1665795894e-2f;
    p = p * r + 1.6666665459e-1f;
    p = p * r + 5.0000001201e-1f;
    const float rr = r * r;
    p = p * rr;
    p = p + r;
    p = p + 1.0f;
    const int k = (int)(tc == tc ? kf : 0.0f);
    const int k1 = k >> 1, k2 = k - k1;
    p = p * train_pow2(k1) * train_pow2(k2);
    return tc == tc ? p : t;
}

// numerics.rs:233 with the exponential above: 1 / (1 + exp(-v)), an IEEE division.  NaN -> NaN, +inf -> 1, -inf -> 0.
APD_TRAIN_HD inline float train_sigmoid(float v) { return 1.0f / (1.0f + train_exp(-v)); }

// The counter-based generator of apd_train_order: SplitMix64's finaliser over a key made of (seed, epoch, signal) and a counter.
APD_TRAIN_HD inline uint64_t train_mix64(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
inline uint64_t train_order_key(uint64_t seed, uint64_t epoch, uint64_t signal)
{
    uint64_t key = train_mix64(seed + 0x9E3779B97F4A7C15ull);
    key = train_mix64(key ^ (epoch + 1) * 0xD1B54A32D192ED03ull);
    return train_mix64(key ^ (signal + 1) * 0x8CB92BA72F3D8DD7ull);
}
// the draw for position i of a shuffle: uniform on [0, bound) up to 2^-32 (the high word of a 64 x 64-bit product; bound < 2^32)
inline uint64_t train_order_draw(uint64_t key, uint64_t i, uint64_t bound)
{
    const uint64_t u = train_mix64(key + i * 0x9E3779B97F4A7C15ull);
    return ((u >> 32) * bound) >> 32;
}

}  // namespace apd
