// Systolic fused-pair banded DTW (the production kernel), gfx950.
//
// See dtw_generic.hip for the recurrence and the DP1/DP2 fusion.  This kernel adds:
//  * G lanes per unordered pair (64/G pairs per wavefront), lane gl owns C band offsets u = C*gl + c, so that a
//    band of 2w+1 offsets fills the wave instead of leaving lanes idle (w = 66 -> G = 16, C = 9: 133/144 busy);
//  * column frames y[j] enter at lane G-1 of a group and move one lane down per macro-step (DPP row/wave shifts),
//    each lane keeping its C-column window in registers; row frames x[i] (shared by every group of the wave: the
//    pairs of a wave have the same b) are staged once per wave in a small LDS ring, filled by coalesced 16-byte
//    loads U rows ahead, and read back by every lane (row tau + 1 - gl).  Each frame is fetched from memory once
//    per wave: the algorithmic minimum 4*D*(n+m) bytes per ordered pair is an upper bound of what the kernel reads;
//  * the rows are sequence b of the pair (a < b), the columns sequence a (decode_pair_rows_b): sequences are resident longest
//    first, so b is the shorter one, and a sweep takes as many macro-steps as it has rows, plus the lane of the result cell.
//    The kernel computes score(x = rows, y = cols) and score(x = cols, y = rows) whichever sequence the rows are, bit for bit
//    (dtw_common.h), so this is a relabelling; store_pair_rows_b puts each score into its plane;
//  * the sweep ends with the capture of the result cell, in lane u* / C at macro-step (rows - 1) + u* / C (sweep_steps_needed,
//    apd_internal.h; the largest of the wave, of the workgroup in the shared-column kernel): the lanes above it would only run
//    cells of the last rows through that nothing reads;
//  * no per-cell boundary tests: rows <= 0 use an x frame of -INF, columns <= 0 the +INF sentinel frame stored
//    behind every sequence, so those cells evaluate to +INF by arithmetic (penalties must be > 0; otherwise the
//    dispatcher takes the generic kernel); D[0][0] = 0 (alignments.rs:109) is injected and the result cell
//    (n-1, m-1) (alignments.rs:120) captured only in the first G and the last macro-steps, from the shortest pair's last row on
//    ("slow" phases);
//  * the static band edges (DP1 stops at u = 2w-1, DP2 spans u = 1..2w) are two per-lane scalar masks per offset
//    OR-ed into the select (see select_node): no vector instruction;
//  * hybrid distance form (unit penalties): |x|^2 + |y|^2 - 2 x.y with the row frames pre-scaled by -2 when they are staged
//    (one add + D fmac per cell), ONE superset threshold test per macro-step in front of a rarely taken recompute branch, the
//    window moves issued between that test and its branch, the entering column fetched a macro-step ahead;
//  * steady-state macro-steps carry no address arithmetic (running column offset, contiguous LDS row window) and the DP rows'
//    edge exchanges are rotations (what wraps around is +INF or feeds a guarded node).
// DESIGN.md section 4.1 has the instruction budget, the measurements and what was tried and dropped.
#pragma once
#include <type_traits>

// Timing-only ablations for kernel tuning (results become wrong): build one unit with -DAPD_ABLATE=<bits>.
//   1 no sqrt   2 no DP rows   4 no frame shifts   8 no edge fetches   16 no band guards   32 software-pipelined distances (valid results)
//   64 select = min3 + d (no tie rule, no guards: what a deferred tie check could save at most)   128 no hybrid threshold test
//   512 G = 32 without the one-instruction wave shift + masked column fetch (valid results)
#ifndef APD_ABLATE
#define APD_ABLATE 0
#endif

#include "dtw_common.h"

namespace apd {

typedef float apd_f32x4 __attribute__((ext_vector_type(4)));
constexpr uint32_t kNoFrame = 0xFFFFFF00u;   // beyond every descriptor (frames_bytes < kNoFrame), +imm offsets cannot wrap

// One padded frame through a buffer descriptor.  A lane whose byte offset is out of range (kNoFrame) gets
// zeros from the range check without touching memory: the edge-lane fetches need no branch and no select.
template <int D>
__device__ __forceinline__ void load_frame(float (&dst)[D], __amdgpu_buffer_rsrc_t rsrc, uint32_t byte_off)
{
    constexpr int DP4 = (D + 3) / 4;
#pragma unroll
    for (int q = 0; q < DP4; ++q) {
        const apd_f32x4 t = __builtin_bit_cast(apd_f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, byte_off + 16u * q, 0, 0));
        if (4 * q + 0 < D) dst[4 * q + 0] = t.x;
        if (4 * q + 1 < D) dst[4 * q + 1] = t.y;
        if (4 * q + 2 < D) dst[4 * q + 2] = t.z;
        if (4 * q + 3 < D) dst[4 * q + 3] = t.w;
    }
}

// Same, one dword per instruction: no register-tuple constraint on the destination, so a frame can be fetched in
// place into registers that the DPP shifts also write (the allocator then needs no copies on the loop back-edge).
template <int D>
__device__ __forceinline__ void load_frame_dwords(float (&dst)[D], __amdgpu_buffer_rsrc_t rsrc, uint32_t byte_off)
{
#pragma unroll
    for (int k = 0; k < D; ++k)
        dst[k] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, byte_off + 4u * k, 0, 0));
}

// numerics.rs:114-120 as an fma chain, k ascending; v_sqrt_f32 (<= 1 ulp).
template <int D, int DN>
__device__ __forceinline__ float frame_dist(const float (&x)[DN], const float (&y)[DN])
{
    float t = x[0] - y[0];
    float acc = t * t;
#pragma unroll
    for (int k = 1; k < D; ++k) {
        t = x[k] - y[k];
        acc = __builtin_fmaf(t, t, acc);
    }
    if (APD_ABLATE & 1) return acc;
    return __builtin_amdgcn_sqrtf(acc);
}

// numerics.rs:114-120 operation for operation: every difference, square and partial sum rounded on its own, then the
// correctly rounded square root -- the bits the CPU code produces.  Used with non-unit penalties, where the node update
// adds a penalty that depends on WHICH predecessor won: a near-tie resolved the other way moves the score by percents,
// so the comparison inputs must be the reference's to the last bit.
template <int D, int DN>
__device__ __forceinline__ float frame_sq_strict(const float (&x)[DN], const float (&y)[DN])
{
    float t = x[0] - y[0];
    float acc = t * t;                                            // 0.0 + t*t == t*t
#pragma unroll
    for (int k = 1; k < D; ++k) {
        t = x[k] - y[k];
        const float sq = t * t;
        acc = acc + sq;
    }
    return acc;
}
template <int D, int DN>
__device__ __forceinline__ float frame_dist_strict(const float (&x)[DN], const float (&y)[DN])
{
    return __builtin_sqrtf(frame_sq_strict<D, DN>(x, y));         // correctly rounded (hipcc default: -fhip-fp32-correctly-rounded-divide-sqrt)
}

// Squared distance by norm expansion, |x|^2 + |y|^2 - 2 x.y: x[D], y[D] hold the squared norms, and the row frame comes
// pre-scaled: xm[k] = -2 x[k] (done once per row when the wave stages it in LDS), xm[D] = |x|^2.
// |x|^2 + |y|^2 + sum xm_k y_k: one add and D v_fmac -- the multiply that opens the dot product and the closing fma(-2, ., .) are gone.
template <int D>
__device__ __forceinline__ float frame_sq_expanded_pre(const float (&xm)[D + 1], const float (&y)[D + 1])
{
    float acc = xm[D] + y[D];
#pragma unroll
    for (int k = 0; k < D; ++k) acc = __builtin_fmaf(xm[k], y[k], acc);
    return acc;
}
// One 16-byte piece (components 4 piece .. 4 piece + 3) of a row frame on its way into the LDS ring: times -2, the norm kept.
template <int D>
__device__ __forceinline__ void prescale_row_piece(apd_f32x4 &v, int piece)
{
    const bool np = piece == D / 4;                              // the piece that holds the norm
    v.x = (np && D % 4 == 0) ? v.x : -2.0f * v.x;
    v.y = (np && D % 4 == 1) ? v.y : -2.0f * v.y;
    v.z = (np && D % 4 == 2) ? v.z : -2.0f * v.z;
    v.w = (np && D % 4 == 3) ? v.w : -2.0f * v.w;
}
// Difference form from the pre-scaled row frame: fma(-0.5, xm_k, -y_k) is x_k - y_k with its one rounding (the scaling is exact).
template <int D>
__device__ __forceinline__ float frame_sq_exact_pre(const float (&xm)[D + 1], const float (&y)[D + 1])
{
    float t = __builtin_fmaf(-0.5f, xm[0], -y[0]);
    float acc = t * t;
#pragma unroll
    for (int k = 1; k < D; ++k) {
        t = __builtin_fmaf(-0.5f, xm[k], -y[k]);
        acc = __builtin_fmaf(t, t, acc);
    }
    return acc;
}
// The two DP rows of one macro-step, shared by the systolic kernels: DP1 = score(a, b) (left = DELETE), DP2 = score(b, a) (up = DELETE).
// Exchanges across lanes wrap around the group (rotations: no +INF fill to materialise).  What the edge lanes
// receive is either +INF already or never looked at: lane 0's DELETE/INSERT neighbour comes from offset
// G*C - 1 >= 2w, outside DP1's band and therefore +INF (guarded nodes sit on their +INF MATCH predecessor), and
// its DP2 node (u = 0) is guarded itself; lane G-1's last node is guarded in DP1, and in DP2 either guarded
// (G*C - 1 > 2w) or handed lane 0's guarded u = 0 node, +INF.  (G = 8, 32: the rotation spans two groups / the wave; the nodes
// that wrap in come from the neighbouring group's edges, which meet the same conditions -- G*C >= 2w + 1 holds
// for every pair of the tile, and idle groups sweep a 1 x 1 dummy with w = 2.)
template <int C, int G, bool UNIFORM_PEN>
__device__ __forceinline__ void dp_rows_step(float (&prev1)[C], float (&prev2)[C], const float (&d)[C], const bool (&g1)[C],
                                             const bool (&g2)[C], float del, float ins, float mat, int gl)
{
    float left1 = group_from_lower_wrap<G>(prev1[C - 1], APD_INF, gl);
    float left2 = group_from_lower_wrap<G>(prev2[C - 1], APD_INF, gl);
    float upr1 = APD_INF, upr2 = APD_INF;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        if (APD_ABLATE & 2) { prev1[c] += d[c]; prev2[c] -= d[c]; continue; }
        const float up1 = (c < C - 1) ? prev1[(c + 1) % C] : upr1;
        const float up2 = (c < C - 1) ? prev2[(c + 1) % C] : upr2;
        // guards: outside a DP's band the node is forced onto its MATCH predecessor, which is +INF
        const float r1 = select_node<UNIFORM_PEN>(left1, up1, prev1[c], d[c], del, ins, mat, (APD_ABLATE & 16) ? false : g1[c]);   // left = DELETE
        const float r2 = select_node<UNIFORM_PEN>(up2, left2, prev2[c], d[c], del, ins, mat, (APD_ABLATE & 16) ? false : g2[c]);   // up   = DELETE
        prev1[c] = r1; prev2[c] = r2;
        left1 = r1; left2 = r2;
        if (c == 0) {
            upr1 = group_from_upper_wrap<G>(r1, APD_INF, gl);
            upr2 = group_from_upper_wrap<G>(r2, APD_INF, gl);
        }
    }
}
// Slow-phase bookkeeping of one macro-step: D[0][0] = 0 once the lane has swept row 0, and the result cell (n-1, m-1) kept.
template <int C>
__device__ __forceinline__ void slow_phase_captures(float (&prev1)[C], float (&prev2)[C], float &res1, float &res2, int tau, int gl,
                                                    int tau_cap, int cw, int cstar)
{
    if (tau == gl) {                              // this lane just swept row 0: D[0][0] = 0
#pragma unroll
        for (int c = 0; c < C; ++c) if (c == cw) { prev1[c] = 0.0f; prev2[c] = 0.0f; }
    }
    if (tau == tau_cap) {                         // row n-1 done: keep cell (n-1, m-1)
#pragma unroll
        for (int c = 0; c < C; ++c) if (c == cstar) { res1 = prev1[c]; res2 = prev2[c]; }
    }
}
template <int D, int C, int G, bool UNIFORM_PEN, bool HYBRID>
__global__ __launch_bounds__(256) void dtw_fused_systolic(const AlignLaunch L)
{
    static_assert(C >= 2 && (64 % G) == 0, "bad geometry");
    if (L.d_nonfinite != nullptr && *L.d_nonfinite != 0u) return;   // a NaN / infinite feature in the batch: the literal kernel's job
    constexpr int DN = D + 1;                                  // frame components + squared norm
    constexpr int DP = (DN + 3) & ~3;                          // floats per resident frame
    constexpr int PPW = 64 / G;                                // pairs per wave
    constexpr int WPT = kSlotsPerTile / (4 * PPW);             // workgroups per tile
    const int lane = threadIdx.x & 63;
    const int gl = lane % G;
    // XCD-aware placement: blocks b and b+8 share an XCD (and its L2); keep a tile's workgroups on one XCD.
    const uint32_t xcd = blockIdx.x & 7u, q = blockIdx.x >> 3;
    const uint32_t tile = (q / WPT) * 8u + xcd;
    const uint32_t slot = ((q % WPT) * 4u + (threadIdx.x >> 6)) * PPW + lane / G;   // transposed: one b, consecutive a
    const PairInfo P = decode_pair_rows_b(L, tile, slot);         // rows (A, n): sequence b, the shorter; columns (B, m): a
    const bool special = P.valid && (P.n == 1 || P.m == 1);   // absent result cell (alignments.rs:120-123)
    const bool sweep = P.valid && !special;
    if (__ballot(sweep) == 0ull) {
        if (special && gl == 0) { const float s = (P.n == 1 && P.m == 1) ? 0.0f : APD_INF; store_pair(L, tile, P, s, s); }
        return;
    }
    const int n = sweep ? P.n : 1, m = sweep ? P.m : 1, w = sweep ? P.w : 2;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)L.d_frames, 0, L.frames_bytes, 0x00020000);
    const uint32_t a_off = (uint32_t)(P.A - L.d_frames) * 4u, b_off = (uint32_t)(P.B - L.d_frames) * 4u;   // bytes
    constexpr uint32_t FB = DP * 4u;                             // bytes per padded frame
    float ins = L.band.ins, del = L.band.del, mat = L.band.mat;
    float tau_thr = L.tau, nmax_b = P.nmax_b;
    asm volatile("" : "+v"(ins), "+v"(del), "+v"(mat), "+v"(tau_thr), "+v"(nmax_b));   // keep them in VGPRs: an SGPR operand doubles a VOP2's issue cost
    // row-frame ring of this wave: slot = row & (R - 1); rows <= 0 hold -INF.  R > 2U + G - 2 keeps a refill from
    // overwriting a row some lane still needs.
    constexpr int R = (G == 64) ? 128 : 64;                      // G = 32, U <= 10: 2U + G - 2 = 50 < 64
    constexpr int LPF = DP / 4;                                  // lanes (16-byte pieces) per frame
    constexpr int FPF = 64 / LPF;                                // frames per wave-wide fill
    // ring rows are RS = DP + 4 floats apart: the 16 lanes of a ds_read_b128 group read 16 consecutive rows, and a stride of
    // 16 floats would put every fourth of them on the same banks (4-way conflict); 20 floats spreads them over all 64
    constexpr int RS = DP + 4;
    // S = C + 1 and U (rows per refill) are fixed further down; the ring carries a copy of its first U rows behind row R - 1, so
    // that the U consecutive rows a lane reads during one unrolled block are contiguous: one address per block, the rest are
    // immediate offsets of the ds_read
    constexpr int U_ROWS = ((C + 1) % 2 == 0) ? (C + 1) : 2 * (C + 1);
    __shared__ float xring_all[4][(R + U_ROWS) * RS];
    float *const xring = xring_all[threadIdx.x >> 6];
    // the row sequence b (and its length) is the same for every sweeping group of the wave
    const int lead = __builtin_ctzll(__ballot(sweep));
    const uint32_t a_off_w = __builtin_amdgcn_readlane(a_off, lead);
    const int n_w = __builtin_amdgcn_readlane(n, lead);
    const int u0 = C * gl;
    const int two_w = 2 * w;

    // static band guards
    bool g1[C], g2[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int u = u0 + c;
        g1[c] = u >= two_w;                       // DP1 spans u in [0, 2w-1]
        g2[c] = (u == 0) | (u > two_w);           // DP2 spans u in [1, 2w]
    }
    const int cw = w - u0;                        // offset index holding u == w (cell (0,0)) if 0 <= cw < C
    const int ustar = sweep_result_offset(n, m, w);   // band offset of the result cell (n-1, m-1)
    const int cstar = ustar - u0;
    const int tau_cap = (n - 1) + gl;             // macro-step in which this lane sweeps row n-1

    // wave-uniform loop bounds: the sweep ends with the last capture of the wave (lane ustar / C at its tau_cap)
    // (the bound goes through a copy of w the compiler cannot see through: it would otherwise keep this u* / C in a register for
    // the store at the kernel's end instead of dividing again there, which costs some instantiations a wave per SIMD)
    int w_bound = w;
    asm volatile("" : "+v"(w_bound));
    int my_total = sweep ? sweep_steps_needed(n, m, w_bound, C) : 0;
    int my_min = sweep ? (n - 1) : 0x7fffffff;
    int total = 0, min_rows = 0x7fffffff;
#pragma unroll
    for (int g = 0; g < PPW; ++g) {
        total = max(total, __builtin_amdgcn_readlane(my_total, g * G));
        min_rows = min(min_rows, __builtin_amdgcn_readlane(my_min, g * G));
    }
    // Column window: S = C + 1 register slots used as a ring (slot = column mod S): C live columns plus the one
    // entering at the next macro-step.  Row frames: two sets, ping-pong.  With the loop unrolled U = lcm(S, 2)
    // macro-steps every slot keeps its physical registers (no copies on the back-edge).
    constexpr int S = C + 1;
    constexpr int U = (S % 2 == 0) ? S : 2 * S;
    static_assert(U == U_ROWS, "ring copy sized for another unroll");
    // G = 32 (two DPP rows per group), hybrid form: a shift inside the group takes two DPP instructions per register (the rows
    // that read across a row boundary, and the rows that end a group and must keep the fetched frame).  Instead the whole wave
    // shifts by one lane with ONE instruction -- the two group-top lanes receive a frame of the neighbouring pair or keep a
    // stale one -- and only those lanes then fetch their entering column, under EXEC, on top of it.
    // G = 8 (two groups per DPP row) is the same case one level down: row_shl instead of wave_shl.
    constexpr bool MASKED_FETCH = HYBRID && (G == 32 || G == 8) && !(APD_ABLATE & 512);
    const int total_r = ((total + U - 1) / U) * U;
    // Strict mode (unit penalties, difference form): the steady-state loop takes square roots with sqrt_rn_finite, whose domain
    // excludes +INF, so every macro-step in which some lane still holds a sentinel column (j <= 0: tau <= w - (C-1) gl, at most w)
    // or a row <= 0 (tau < G) stays in the slow phase, whose square root is the compiler's general sequence.
    int a_steps = G;
    if (UNIFORM_PEN && !HYBRID) {
        int w_max = 0;
#pragma unroll
        for (int g = 0; g < PPW; ++g) w_max = max(w_max, __builtin_amdgcn_readlane(w, g * G));
        a_steps = max(G, w_max + 1);
    }
    const int a_end = min(((a_steps + U - 1) / U) * U, total_r);
    const int b_end = min(max((min_rows / U) * U, a_end), total_r);

    float prev1[C], prev2[C];
#pragma unroll
    for (int c = 0; c < C; ++c) { prev1[c] = APD_INF; prev2[c] = APD_INF; }
    float res1 = 0.0f, res2 = 0.0f;

    // window at macro-step 0: column j = -gl + u0 + c - w in slot c; columns <= 0 read the +INF sentinel (index m)
    float yf[S][DN];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int j = u0 - gl + c - w;
        const int idx = (j >= 1) ? (min(j, m) - 1) : (HYBRID ? m : m + 1);   // sentinel H / sentinel E
        load_frame<DN>(yf[c], rsrc, b_off + (uint32_t)idx * FB);
    }
#pragma unroll
    for (int k = 0; k < DN; ++k) yf[C][k] = 0.0f;
    if (HYBRID && !MASKED_FETCH && !(APD_ABLATE & 8)) {          // hybrid form: columns are fetched one macro-step ahead (fetch_column)
        const int jt = 1 + (C - 1) * G - w;
        const uint32_t yo = b_off + (uint32_t)((jt >= 1) ? (min(jt, m) - 1) : m) * FB;
        load_frame<DN>(yf[C], rsrc, gl == G - 1 ? yo : kNoFrame);
    }
    // ring prologue: rows -(G-1)..0 are -INF, rows 1..U come from memory
    constexpr int NFILL = (U + FPF - 1) / FPF;
    const int fill_f = lane / LPF, fill_q = lane % LPF;          // this lane's frame and 16-byte piece inside a fill
    auto fill_load = [&](int first_row, apd_f32x4 (&regs)[NFILL]) __attribute__((always_inline)) {
#pragma unroll
        for (int f = 0; f < NFILL; ++f) {
            const int fi = f * FPF + fill_f;
            const bool act = (fill_f < FPF) & (fi < U);
            const uint32_t off = a_off_w + (uint32_t)(min(first_row + fi, n_w) - 1) * FB + 16u * fill_q;
            regs[f] = __builtin_bit_cast(apd_f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, act ? off : kNoFrame, 0, 0));
        }
    };
    auto fill_store = [&](int first_row, const apd_f32x4 (&regs)[NFILL]) __attribute__((always_inline)) {
#pragma unroll
        for (int f = 0; f < NFILL; ++f) {
            const int fi = f * FPF + fill_f;
            if ((fill_f < FPF) & (fi < U)) {
                apd_f32x4 v = regs[f];
                if (HYBRID) prescale_row_piece<D>(v, fill_q);    // stage -2 x (the norm slot stays): see frame_sq_expanded_pre
                const int slot = (first_row + fi) & (R - 1);
                *reinterpret_cast<apd_f32x4 *>(&xring[slot * RS + 4 * fill_q]) = v;
                if (slot < U) *reinterpret_cast<apd_f32x4 *>(&xring[(slot + R) * RS + 4 * fill_q]) = v;   // the copy behind the ring
            }
        }
    };
    for (int e = lane; e < G * DP; e += 64) {                    // rows <= 0: -INF components, or (hybrid) zeros with norm +INF
        const int slot = (-(e / DP)) & (R - 1);
        const float v = HYBRID ? ((e % DP) == D ? APD_INF : 0.0f) : -APD_INF;
        xring[slot * RS + (e % DP)] = v;
        if (slot < U) xring[(slot + R) * RS + (e % DP)] = v;
    }
    {
        apd_f32x4 regs[NFILL];
        fill_load(1, regs);
        fill_store(1, regs);
    }
    asm volatile("" ::: "memory");
    auto read_row = [&](float (&dst)[DN], int row) __attribute__((always_inline)) {
        const float *p = &xring[(row & (R - 1)) * RS];
#pragma unroll
        for (int q = 0; q < LPF; ++q) {
            const apd_f32x4 t = *reinterpret_cast<const apd_f32x4 *>(p + 4 * q);
            if (4 * q + 0 < DN) dst[4 * q + 0] = t.x;
            if (4 * q + 1 < DN) dst[4 * q + 1] = t.y;
            if (4 * q + 2 < DN) dst[4 * q + 2] = t.z;
            if (4 * q + 3 < DN) dst[4 * q + 3] = t.w;
        }
    };
    auto read_row_at = [&](float (&dst)[DN], const float *p) __attribute__((always_inline)) {
#pragma unroll
        for (int q = 0; q < LPF; ++q) {
            const apd_f32x4 t = *reinterpret_cast<const apd_f32x4 *>(p + 4 * q);
            if (4 * q + 0 < DN) dst[4 * q + 0] = t.x;
            if (4 * q + 1 < DN) dst[4 * q + 1] = t.y;
            if (4 * q + 2 < DN) dst[4 * q + 2] = t.z;
            if (4 * q + 3 < DN) dst[4 * q + 3] = t.w;
        }
    };
    constexpr int NX = HYBRID ? 1 : 2;                           // hybrid: one row-frame set (registers are the limit)
    float xs[NX][DN];
    read_row(xs[0], 0 - gl);                                     // macro-step 0: row -gl (all -INF)
#pragma unroll
    for (int k = 0; k < DN; ++k) xs[NX - 1][k] = (NX == 1) ? xs[0][k] : 0.0f;
    // Software pipeline: the first C-1 distances of macro-step tau+1 only need columns the lane already holds, so they
    // are computed during macro-step tau, next to the serial DP chain; only the last column waits for the shift.
    constexpr bool PIPE = (APD_ABLATE & 32) != 0;                  // measured: no gain on MI355X (cfg 3: -2 %), kept as a tuning switch
    float dn[C];
#pragma unroll
    for (int c = 0; c < C; ++c) dn[c] = (PIPE && !HYBRID && c < C - 1) ? frame_dist_strict<D, DN>(xs[0], yf[c]) : 0.0f;

    // advance the column window: every column moves one lane down (q: position inside the unrolled block)
    auto advance_window = [&](int q) __attribute__((always_inline)) {
        const int r = q % S, e = (r + C) % S;
#pragma unroll
        for (int k = 0; k < (HYBRID ? DN : D); ++k) {
            if (APD_ABLATE & 4) { yf[e][k] = yf[(r + 1) % S][k] + yf[e][k]; continue; }
            yf[e][k] = MASKED_FETCH ? dpp_move<(G == 8) ? 0x101 : 0x130>(yf[(r + 1) % S][k], yf[e][k])   // row_shl:1 / wave_shl:1, every row
                                    : group_from_upper<G>(yf[(r + 1) % S][k], yf[e][k], gl);
        }
    };
    auto macro_steps = [&](int tau_begin, int tau_end, auto slow_tag) __attribute__((always_inline)) {
        constexpr bool SLOW = decltype(slow_tag)::value;
        // Steady state (tau >= G, so the entering column jt = tau + 1 + (C-1) G - w is >= 1: G C >= 2w + 1): the top lane's fetch
        // offset advances by one frame per macro-step, clamped at column m; the other lanes stay out of range.
        uint32_t yo_cur = kNoFrame, yo_cap = kNoFrame, yo_step = 0u;
        if (!SLOW && gl == G - 1) {                              // (hybrid form: fetched one macro-step ahead, see below)
            yo_cap = b_off + (uint32_t)(m - 1) * FB;
            yo_cur = min(b_off + (uint32_t)(tau_begin + ((HYBRID && !MASKED_FETCH) ? 1 : 0) + (C - 1) * G - w) * FB, yo_cap);
            yo_step = FB;
        }
        // the column entering the group at step t + 1, fetched by the top lane
        auto fetch_column = [&](float (&dst)[DN], int t) __attribute__((always_inline)) {
            if (APD_ABLATE & 8) return;
            if (SLOW) {
                const int jt = t + 1 + (C - 1) * G - w;
                const uint32_t yo = b_off + (uint32_t)((jt >= 1) ? (min(jt, m) - 1) : (HYBRID ? m : m + 1)) * FB;
                load_frame<DN>(dst, rsrc, gl == G - 1 ? yo : kNoFrame);
            } else {
                load_frame<DN>(dst, rsrc, yo_cur);
                yo_cur = min(yo_cur + yo_step, yo_cap);
            }
        };
        for (int tau0 = tau_begin; tau0 < tau_end; tau0 += U) {
            apd_f32x4 fill_regs[NFILL];
            fill_load(tau0 + U + 1, fill_regs);                  // rows of the NEXT block, stored at this block's end
            const float *const xrows = &xring[((tau0 + 1 - gl) & (R - 1)) * RS];   // rows tau0 + 1 - gl ... + U - 1, contiguous
#pragma unroll
            for (int q = 0; q < U; ++q) {
                const int tau = tau0 + q;
                const int r = q % S;               // slot of this step's first column
                const int xa = HYBRID ? 0 : (q & 1), xb = HYBRID ? 0 : (xa ^ 1);   // current / next row-frame set
                const int e = (r + C) % S;         // slot of the column entering at tau + 1 (dead during this step)
                // column frame entering the group at tau + 1: fetched by the top lane straight into the dead slot
                // (other lanes' offsets are out of range: no memory access, and the DPP below overwrites them)
                // (hybrid form: the window moves in the middle of the step, so the frame is fetched a step ahead, see fetch_column)
                if (!HYBRID) {
                    fetch_column(yf[e], tau);
                    read_row_at(xs[xb], xrows + q * RS);         // next row frame from the wave's LDS ring
                }
                // the C local distances of this row
                float d[C];
                if (HYBRID) {
                    // |x|^2 + |y|^2 - 2 x.y; where that is below tau (|x|^2 + |y|^2) cancellation has eaten the digits:
                    // such cells are recomputed in the difference form (wave-uniform branch, rare for unrelated frames)
                    // One test per macro-step instead of one per cell: if some cell has d2_c < tau (|x|^2 + |y_c|^2) then the
                    // smallest d2 of the lane is below tau (|x|^2 + N_b), N_b the largest frame norm of sequence b -- a superset
                    // of the per-cell condition (never misses a cell; on a hit the exact per-cell test below decides).
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        d[c] = frame_sq_expanded_pre<D>(xs[xa], yf[(r + c) % S]);
                    }
                    float dmin = d[0];
#pragma unroll
                    for (int c = 1; c + 1 < C; c += 2) dmin = __builtin_fminf(__builtin_fminf(dmin, d[c]), d[c + 1]);
                    if (C % 2 == 0) dmin = __builtin_fminf(dmin, d[C - 1]);
                    const bool any = (APD_ABLATE & 128) ? false : dmin < (xs[xa][D] + nmax_b) * tau_thr;
                    // The window moves here, between the test and the branch on it: the slot it writes is dead, nothing below
                    // reads the one it vacates before the next step, and the 14 moves cover the latency of compare -> branch.
                    advance_window(q);
                    if (MASKED_FETCH) {
                        if (gl == G - 1) fetch_column(yf[e], tau);   // the column entering at tau + 1, on top of what the shift left there
                    }
                    if (__builtin_expect(__ballot(any) != 0ull, 0)) {   // rare: placed out of the hot instruction stream
                        float nx = xs[xa][D];
                        asm volatile("" : "+v"(nx));              // a norm sum of its own: reusing the hot path's would keep nine of them
                                                                 // alive across the branch and turn their v_fmac into 3-operand v_fma
#pragma unroll
                        for (int c = 0; c < C; ++c) {
                            const float sc = nx + yf[(r + c) % S][D];
                            const float ex = frame_sq_exact_pre<D>(xs[xa], yf[(r + c) % S]);
                            d[c] = (d[c] < sc * tau_thr) ? ex : d[c];
                        }
                    }
                    // slot r (this step's first column) is dead from here on, and it is the slot the NEXT step's window move fills:
                    // fetch that step's entering column now, a whole macro-step before it is needed
                    if (!MASKED_FETCH) fetch_column(yf[r], tau + 1);
#pragma unroll
                    for (int c = 0; c < C; ++c) d[c] = (APD_ABLATE & 1) ? d[c] : __builtin_amdgcn_sqrtf(d[c]);
                    read_row_at(xs[0], xrows + q * RS);           // the row frame is dead now: fetch the next one under the DP rows
                } else if (UNIFORM_PEN && !SLOW && !PIPE) {
                    // Strict mode, steady state.  The difference form of the band kernels IS the reference's arithmetic
                    // (numerics.rs:114-120 operation for operation); the square root is sqrt_rn_finite (dtw_common.h): v_sqrt_f32 and
                    // an exact two-sided fix-up, 7 vector ops instead of the 16 of the compiler's general sequence.  Its domain is
                    // 2^-96 <= d2 < +INF: the steady state sees no sentinel frame (strict_a_end below keeps those macro-steps in the
                    // slow phase) and no overflow (features >= 2^60 flag the batch for the literal kernel), and a macro-step in
                    // which some cell's d2 is below 2^-96 (zero included: identical frames) takes the general sequence instead,
                    // behind one wave-uniform branch.
                    float d2[C];
#pragma unroll
                    for (int c = 0; c < C; ++c) d2[c] = frame_sq_strict<D, DN>(xs[xa], yf[(r + c) % S]);
                    float dmin = d2[0];
#pragma unroll
                    for (int c = 1; c + 1 < C; c += 2) dmin = __builtin_fminf(__builtin_fminf(dmin, d2[c]), d2[c + 1]);
                    if (C % 2 == 0) dmin = __builtin_fminf(dmin, d2[C - 1]);
                    if (__builtin_expect(__ballot(!(dmin >= 0x1p-96f)) != 0ull, 0)) {
#pragma unroll
                        for (int c = 0; c < C; ++c) d[c] = __builtin_sqrtf(d2[c]);
                    } else {
#pragma unroll
                        for (int c = 0; c < C; ++c) d[c] = sqrt_rn_finite(d2[c]);
                    }
                } else {
#pragma unroll
                    for (int c = 0; c < C; ++c)
                        // The difference form of the band kernels IS the reference's arithmetic (numerics.rs:114-120 operation for
                        // operation), with either select: with unit penalties `base + 1.0 * d` is `base + d` and the fast select
                        // picks the reference's predecessor for every non-NaN input, so <.., UNIFORM_PEN = true, HYBRID = false> is
                        // bit-identical to the CPU code at 4 instead of ~12 vector ops per node (strict mode, apd_set_distance_mode 2).
                        d[c] = (UNIFORM_PEN && PIPE && c < C - 1) ? dn[c] : frame_dist_strict<D, DN>(xs[xa], yf[(r + c) % S]);
                    if (PIPE) {
#pragma unroll
                        for (int c = 0; c < C - 1; ++c) dn[c] = frame_dist_strict<D, DN>(xs[xb], yf[(r + 1 + c) % S]);
                    }
                }
                dp_rows_step<C, G, UNIFORM_PEN>(prev1, prev2, d, g1, g2, del, ins, mat, gl);
                if (SLOW) slow_phase_captures<C>(prev1, prev2, res1, res2, tau, gl, tau_cap, cw, cstar);
                if (!HYBRID) advance_window(q);
            }
            fill_store(tau0 + U + 1, fill_regs);
            asm volatile("" ::: "memory");                       // rows written by other lanes are read in the next block: no
                                                                 // barrier needed inside one wave (LDS runs in order), but the
                                                                 // compiler must not move the reads up
        }
    };
    macro_steps(0, a_end, std::true_type{});
    macro_steps(a_end, b_end, std::false_type{});
    macro_steps(b_end, total_r, std::true_type{});

    if (P.valid && gl == (sweep ? ustar / C : 0)) {
        if (sweep) {
            const float denom = (float)(n + m);                  // alignments.rs:121
            store_pair_rows_b(L, tile, P, res1 / denom, res2 / denom);
        } else {
            const float s = (P.n == 1 && P.m == 1) ? 0.0f : APD_INF;
            store_pair(L, tile, P, s, s);
        }
    }
}

// One resident frame (DN floats, 16-byte aligned) out of LDS: whole 16-byte pieces, and a last read of exactly the floats that are
// left.  A fourth ds_read_b128 for a tail of two floats would need a register quad of its own (or one that overlaps the
// neighbouring piece's, with a wait for the LDS in between): the shared-column kernel reads two frames per macro-step this way.
typedef float apd_f32x2 __attribute__((ext_vector_type(2)));
// 16-byte piece `piece` of that frame (floats 4 piece .. 4 piece + 3, as far as the frame goes) on its own
template <int DN>
__device__ __forceinline__ void read_frame_piece_lds(float (&dst)[DN], const float *p, int piece)
{
    constexpr int FULL = DN / 4, TAIL = DN % 4;
    if (piece < FULL) {
        const apd_f32x4 t = *reinterpret_cast<const apd_f32x4 *>(p + 4 * piece);
        dst[4 * piece + 0] = t.x; dst[4 * piece + 1] = t.y; dst[4 * piece + 2] = t.z; dst[4 * piece + 3] = t.w;
        return;
    }
    if (TAIL >= 2) {
        const apd_f32x2 t = *reinterpret_cast<const apd_f32x2 *>(p + 4 * FULL);
        dst[4 * FULL + 0] = t.x; dst[4 * FULL + 1] = t.y;
    }
    if (TAIL == 1) dst[4 * FULL] = p[4 * FULL];
    if (TAIL == 3) dst[4 * FULL + 2] = p[4 * FULL + 2];
}
template <int DN>
__device__ __forceinline__ void read_frame_lds(float (&dst)[DN], const float *p)
{
#pragma unroll
    for (int piece = 0; piece < (DN + 3) / 4; ++piece) read_frame_piece_lds<DN>(dst, p, piece);
}

// A pointer into LDS as the 32-bit address the ds instructions take, and back: a block's base kept as such an address needs no
// add of the LDS segment's own base in front of every read.
typedef __attribute__((address_space(3))) const char apd_lds_cchar;
__device__ __forceinline__ uint32_t lds_address(const void *p) { return (uint32_t)(uintptr_t)(apd_lds_cchar *)p; }
__device__ __forceinline__ const float *lds_floats_at(uint32_t a) { return (const float *)(apd_lds_cchar *)(uintptr_t)a; }

// Floats of one column ring: RC frames and a copy of the first U behind them (as the row ring has: the U consecutive slots a lane
// reads during one unrolled block are contiguous), 16 bytes of padding per 8 frames, rounded to whole 256-byte bank rows so
// that the four rings start on the same banks.
constexpr int shared_column_ring_floats(int rc, int u, int dp) { return (((rc + u) * dp + ((rc + u + 7) / 8) * 4) * 4 + 255) / 256 * 64; }

// ---- Shared column rings: the hybrid, unit-penalty kernel with the column window fed from LDS instead of moved by DPP.
// A workgroup sweeps a 4 x 4 sub-block of its tile instead of a 16 x 1 column: wavefront k the row sequence b_k (one b per wavefront,
// as above: the row ring and everything that rests on it stay), its four lane groups the columns a_0 .. a_3.  The four
// wavefronts need the same four column sequences, so the workgroup keeps one ring of RC column frames per a in LDS:
//  * wavefront k fills ring k, U columns per unrolled block, with coalesced 16-byte loads (sentinel frame for columns <= 0,
//    clamped beyond m), stored at the block's end; one barrier per block orders the fills against the reads;
//  * in each macro-step every lane reads the column entering its window, j = tau + 1 + (C-1)(gl+1) - w, into the dead register
//    slot: LPF ds_read_b128 in place of the DN DPP moves and of the top lane's fetch.  The same frames reach the same fmac
//    chains in the same order: results are bit-identical to dtw_fused_systolic<D, C, G, true, true>;
//  * the 16 lanes of a group read columns C - 1 = 8 apart.  Ring slot p = j mod RC lives at p * FB + (p / 8) * 16 bytes: the
//    16 bytes behind every eighth frame make the lane stride an odd number of 16-byte bank slots, conflict-free except where
//    the ring wraps inside the group.  A copy of the first U frames sits behind the ring, so the U consecutive slots a lane
//    reads during one unrolled block are contiguous: one base per block, the frame offsets are immediates of the ds_read and
//    only the padding term is computed per macro-step (2 integer operations: slot p is at (ring + p (FB + 2)) & ~15).  The
//    fetch offsets of the fills run along, clamped, as the DPP kernel's column offset does;
//  * the row frame of macro-step tau + 1 is read into the registers of macro-step tau's, one 16-byte piece at a time, as soon as
//    the nine distance chains are through with that piece: the reads are issued in front of the threshold test and its branch
//    instead of behind them, where their first use followed at once.  The rare recompute branch, which needs the frame of its own
//    step, reads it a second time from the ring and asks for the next one again;
//  * with the fill of block b + 1 written while other wavefronts still read block b, the ring spans the lanes' window,
//    2 U columns and the spread of w inside the workgroup (apd_internal.h, shared_column_ring_frames); the tile plan sends
//    only tiles within that spread here (shared_columns_qualify);
//  * the block count is the workgroup's maximum, and a wavefront without a swept pair still walks the barriers and fills its ring.
//    The phase boundaries (slow / steady / slow) stay per wavefront, so the four wavefronts may sit at DIFFERENT barrier
//    instructions in the same block (the loop body is instantiated once per phase).  That is correct because s_barrier counts
//    arrivals of the workgroup's wavefronts and does not match program locations, and every wavefront executes exactly
//    total_r / U of them; it is a property of this hardware, beyond what the HIP model promises for __syncthreads().
template <int D, int C, int G>
__global__ __launch_bounds__(256) void dtw_fused_systolic_shared(const AlignLaunch L)
{
    static_assert(C >= 2 && G == 16, "one ring per wavefront: four lane groups");
    if (L.d_nonfinite != nullptr && *L.d_nonfinite != 0u) return;   // a NaN / infinite feature in the batch: the literal kernel's job
    constexpr int DN = D + 1;
    constexpr int DP = (DN + 3) & ~3;
    constexpr int PPW = 64 / G;                                // pairs per wave = wavefronts per workgroup = rings
    constexpr int WPT = kSlotsPerTile / (4 * PPW);
    constexpr int S = C + 1;
    constexpr int U = shared_column_unroll(C);
    constexpr int RC = shared_column_ring_frames(G, C);
    constexpr int R = 64;                                      // row ring, as in dtw_fused_systolic
    constexpr int LPF = DP / 4;
    constexpr int FPF = 64 / LPF;
    constexpr int RS = DP + 4;
    constexpr uint32_t FB = DP * 4u;
    constexpr int XRING = (R + U) * RS;                         // floats of one row ring
    constexpr int CRING = shared_column_ring_floats(RC, U, DP);   // floats of one column ring
    static_assert(FPF >= U && RC % 8 == 0, "one wave-wide load per fill");
    // While some wavefront reads block tau0 (lowest column tau0 + C - w_hi) another may already store the fill of the next block
    // (columns up to tau0 + 2U + (C-1)G - w_lo, which land on the slots of the columns RC below them): nothing still read is
    // overwritten as long as RC >= (G-1)(C-1) + 2U + (w_hi - w_lo).  The plan's slack is what the host admits for w_hi - w_lo.
    static_assert(RC >= (G - 1) * (C - 1) + 2 * U + (int)shared_column_slack(KernelGeom{KernelGeom::SharedColumns, G, C}),
                  "ring too short for the spread of w the tile plan admits");
    extern __shared__ __attribute__((aligned(16))) float apd_shared_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int gl = lane % G;
    float *const xring = apd_shared_lds + wave * XRING;
    float *const crings = apd_shared_lds + 4 * XRING;
    int *const wg_words = reinterpret_cast<int *>(crings + PPW * CRING);   // [wave][total, smallest w]
    const uint32_t xcd = blockIdx.x & 7u, q = blockIdx.x >> 3;
    const uint32_t tile = (q / WPT) * 8u + xcd;
    const uint32_t sub = q % WPT;                                // 4 x 4 sub-block of the tile
    const uint32_t slot = ((sub % 4u) * 4u + wave) * kTile + (sub / 4u) * 4u + lane / G;   // transposed: b of the wavefront, a of the group
    const PairInfo P = decode_pair_rows_b(L, tile, slot);         // rows (A, n): sequence b, the shorter; columns (B, m): a
    const bool special = P.valid && (P.n == 1 || P.m == 1);
    const bool sweep = P.valid && !special;
    const int n = sweep ? P.n : 1, m = sweep ? P.m : 1, w = sweep ? P.w : 2;
    const int u0 = C * gl;
    const int two_w = 2 * w;
    int w_bound = w;                                             // opaque copy, as in dtw_fused_systolic
    asm volatile("" : "+v"(w_bound));
    int my_total = sweep ? sweep_steps_needed(n, m, w_bound, C) : 0;   // up to this pair's capture
    int my_min = sweep ? (n - 1) : 0x7fffffff;
    int my_w = sweep ? w : 0x7fffffff;
    int total = 0, min_rows = 0x7fffffff, w_lo = 0x7fffffff;
#pragma unroll
    for (int g = 0; g < PPW; ++g) {
        total = max(total, __builtin_amdgcn_readlane(my_total, g * G));
        min_rows = min(min_rows, __builtin_amdgcn_readlane(my_min, g * G));
        w_lo = min(w_lo, __builtin_amdgcn_readlane(my_w, g * G));
    }
    if (lane == 0) { wg_words[2 * wave] = total; wg_words[2 * wave + 1] = w_lo; }
    __syncthreads();
    total = 0; w_lo = 0x7fffffff;
#pragma unroll
    for (int k = 0; k < 4; ++k) { total = max(total, wg_words[2 * k]); w_lo = min(w_lo, wg_words[2 * k + 1]); }
    if (total == 0) {                                            // workgroup-uniform: nothing to sweep (diagonal tiles, the batch's edge)
        if (special && gl == 0) { const float s = (P.n == 1 && P.m == 1) ? 0.0f : APD_INF; store_pair(L, tile, P, s, s); }
        return;
    }
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)L.d_frames, 0, L.frames_bytes, 0x00020000);
    const uint32_t a_off = (uint32_t)(P.A - L.d_frames) * 4u, b_off = (uint32_t)(P.B - L.d_frames) * 4u;
    float ins = L.band.ins, del = L.band.del, mat = L.band.mat;
    float tau_thr = L.tau, nmax_b = P.nmax_b;
    asm volatile("" : "+v"(ins), "+v"(del), "+v"(mat), "+v"(tau_thr), "+v"(nmax_b));
    // row sequence b of this wavefront (none: a wavefront that only walks the barriers sweeps the first frame of the batch)
    const unsigned long long sweeping = __ballot(sweep);
    const int lead = sweeping ? __builtin_ctzll(sweeping) : 0;
    const uint32_t a_off_w = sweeping ? __builtin_amdgcn_readlane(a_off, lead) : 0u;
    const int n_w = sweeping ? __builtin_amdgcn_readlane(n, lead) : 1;
    // the column sequence of this wavefront's ring: a_wave of the sub-block, whether or not this wavefront's own pair with it is valid
    uint32_t cb_off = 0u;
    int cm = 0;
    bool cvalid = false;
    {
        const uint4 t = L.d_tiles[tile];                         // total > 0: the tile exists
        const uint32_t a = t.x * kTile + (sub / 4u) * 4u + wave;
        if (a < L.n_seq) {
            const uint32_t oa = L.d_seq_off[a];
            cm = (int)(L.d_seq_off[a + 1] - oa) - 2;
            cb_off = oa * L.dpad * 4u;
            cvalid = true;
        }
    }

    bool g1[C], g2[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int u = u0 + c;
        g1[c] = u >= two_w;
        g2[c] = (u == 0) | (u > two_w);
    }
    const int cw = w - u0;
    const int ustar = sweep_result_offset(n, m, w);
    const int cstar = ustar - u0;
    const int tau_cap = (n - 1) + gl;
    // block counts: the workgroup's (every block has one barrier); the phase boundaries stay this wavefront's own
    const int total_r = ((total + U - 1) / U) * U;
    const int a_end = min(((G + U - 1) / U) * U, total_r);
    const int b_end = min(max((min_rows / U) * U, a_end), total_r);

    float prev1[C], prev2[C];
#pragma unroll
    for (int c = 0; c < C; ++c) { prev1[c] = APD_INF; prev2[c] = APD_INF; }
    float res1 = 0.0f, res2 = 0.0f;

    // window at macro-step 0, from memory; the slot of the entering column is read from the ring in macro-step 0
    float yf[S][DN];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int j = u0 - gl + c - w;
        const int idx = (j >= 1) ? (min(j, m) - 1) : m;
        load_frame<DN>(yf[c], rsrc, b_off + (uint32_t)idx * FB);
    }
#pragma unroll
    for (int k = 0; k < DN; ++k) yf[C][k] = 0.0f;

    // ---- row ring (as in dtw_fused_systolic)
    constexpr int NFILL = (U + FPF - 1) / FPF;
    const int fill_f = lane / LPF, fill_q = lane % LPF;
    const bool fill_act = (fill_f < FPF) & (fill_f < U);
    auto fill_load = [&](int first_row, apd_f32x4 (&regs)[NFILL]) __attribute__((always_inline)) {
        const uint32_t off = a_off_w + (uint32_t)(min(first_row + fill_f, n_w) - 1) * FB + 16u * fill_q;
        regs[0] = __builtin_bit_cast(apd_f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, fill_act ? off : kNoFrame, 0, 0));
    };
    auto fill_store = [&](int first_row, const apd_f32x4 (&regs)[NFILL]) __attribute__((always_inline)) {
        if (fill_act) {
            apd_f32x4 v = regs[0];
            prescale_row_piece<D>(v, fill_q);
            const int rslot = (first_row + fill_f) & (R - 1);
            *reinterpret_cast<apd_f32x4 *>(&xring[rslot * RS + 4 * fill_q]) = v;
            if (rslot < U) *reinterpret_cast<apd_f32x4 *>(&xring[(rslot + R) * RS + 4 * fill_q]) = v;
        }
    };
    for (int e = lane; e < G * DP; e += 64) {
        const int rslot = (-(e / DP)) & (R - 1);
        const float v = (e % DP) == D ? APD_INF : 0.0f;
        xring[rslot * RS + (e % DP)] = v;
        if (rslot < U) xring[(rslot + R) * RS + (e % DP)] = v;
    }
    {
        apd_f32x4 regs[NFILL];
        fill_load(1, regs);
        fill_store(1, regs);
    }
    // ---- column rings.  Ring slot of column j: j mod RC (kept as running, wrapped counters: no division in the loop).
    // During block tau0 the lanes read columns tau0 + C - w .. tau0 + U + (C-1) G - w; col_hi is the last of them for the
    // smallest w of the workgroup.  The ring holds (col_hi - RC, col_hi] when the block starts.
    float *const cring_fill = crings + wave * CRING;
    const int col_hi0 = U + (C - 1) * G - w_lo;
    auto ring_slot = [](int j) { return (j + 64 * RC) % RC; };   // prologue only: columns there are above -RC - G C / 2
    auto ring_at = [](auto *ring, uint32_t p) { return ring + p * DP + ((p >> 3) << 2); };
    auto col_load = [&](int j, bool act) __attribute__((always_inline)) {
        const int idx = (j >= 1) ? (min(j, cm) - 1) : cm;        // sentinel H behind the sequence for columns <= 0
        const uint32_t off = cb_off + (uint32_t)idx * FB + 16u * fill_q;
        return __builtin_bit_cast(apd_f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, (act & cvalid) ? off : kNoFrame, 0, 0));
    };
    for (int j0 = col_hi0 - RC + 1; j0 <= col_hi0; j0 += FPF) {   // prologue: the whole ring
        const int j = j0 + fill_f;
        const bool act = (fill_f < FPF) & (j <= col_hi0);
        const apd_f32x4 v = col_load(j, act);
        const uint32_t ps = (uint32_t)ring_slot(j);
        if (act) *reinterpret_cast<apd_f32x4 *>(ring_at(cring_fill, ps) + 4 * fill_q) = v;
        if (act && ps < (uint32_t)U) *reinterpret_cast<apd_f32x4 *>(ring_at(cring_fill, ps + RC) + 4 * fill_q) = v;   // the copy behind the ring
    }
    uint32_t pf = (uint32_t)ring_slot(col_hi0 + 1 + fill_f);      // slot this lane fills at the end of the first block
    // this lane's reads: the column entering at macro-step 1 first
    const float *const cring_read = crings + (lane / G) * CRING;
    uint32_t pr = (uint32_t)ring_slot(1 + (C - 1) * (gl + 1) - w);   // slot read in the first macro-step of the coming block
    // Fetch offsets of the two fills, kept running (yo_cur / yo_cap of dtw_fused_systolic): every block fetches the U frames
    // behind the last block's, clamped at the sequence's last frame; lanes without a share stay out of range (step 0).  The
    // columns fetched here are tau0 + col_hi0 + 1 + fill_f >= U + (C-1) G + 1 - w_lo > 0 (2 w_lo + 1 <= G C): never the sentinel.
    const uint32_t ro_step = fill_act ? (uint32_t)U * FB : 0u;
    const uint32_t ro_cap = fill_act ? a_off_w + (uint32_t)(n_w - 1) * FB + 16u * fill_q : kNoFrame;
    uint32_t ro_cur = fill_act ? min(a_off_w + (uint32_t)(U + fill_f) * FB + 16u * fill_q, ro_cap) : kNoFrame;   // row U + 1 + fill_f
    const bool col_act = fill_act & cvalid;
    const uint32_t co_step = col_act ? (uint32_t)U * FB : 0u;
    const uint32_t co_cap = col_act ? cb_off + (uint32_t)(cm - 1) * FB + 16u * fill_q : kNoFrame;
    uint32_t co_cur = col_act ? min(cb_off + (uint32_t)(col_hi0 + fill_f) * FB + 16u * fill_q, co_cap) : kNoFrame;   // column col_hi0 + 1 + fill_f
    // Byte address of ring slot p of this lane's column ring: ring + p FB + (p / 8) 16 = (ring + p (FB + 2)) & ~15, the ring
    // being 16-byte aligned.  col_base holds ring + pr (FB + 2) for the block; step q adds 2 q and masks, the frames between
    // (q FB) are the immediate of the ds_read: two integer operations per macro-step.
    const uint32_t cring_read_b = lds_address(cring_read);
    uint32_t col_base = 0u;
    auto read_col = [&](float (&dst)[DN], int q) __attribute__((always_inline)) {
        const uint32_t b = (col_base + 2u * (uint32_t)q) & ~15u;
        read_frame_lds<DN>(dst, lds_floats_at(b) + q * DP);
    };
    __syncthreads();
    float xs[DN];
    read_frame_lds<DN>(xs, &xring[((0 - gl) & (R - 1)) * RS]);   // macro-step 0: row -gl
    // The hit path of a macro-step reads its row frame a second time (below).  The oldest such row in block tau0 is
    // tau0 - (G - 1) (lane G - 1, first step: fetched by the previous block), the newest row stored before the block ends is
    // tau0 + U (the previous block's fill): R > U + G - 1 keeps them in different slots.
    static_assert(R > U + G - 1, "a macro-step's row frame must survive in the ring until the block's fill_store");

    auto macro_steps = [&](int tau_begin, int tau_end, auto slow_tag) __attribute__((always_inline)) {
        constexpr bool SLOW = decltype(slow_tag)::value;
        for (int tau0 = tau_begin; tau0 < tau_end; tau0 += U) {
            apd_f32x4 fill_regs[NFILL];
            // rows and columns of the NEXT block, stored at this block's end
            fill_regs[0] = __builtin_bit_cast(apd_f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, ro_cur, 0, 0));
            const apd_f32x4 col_regs = __builtin_bit_cast(apd_f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, co_cur, 0, 0));
            ro_cur = min(ro_cur + ro_step, ro_cap);
            co_cur = min(co_cur + co_step, co_cap);
            // the two LDS bases of the block, in registers of their own (opaque: not recomputed from tau0 / pr in every macro-step)
            uint32_t xrows_b = lds_address(xring) + (uint32_t)(((tau0 + 1 - gl) & (R - 1)) * RS) * 4u;
            col_base = cring_read_b + __umul24(pr, FB + 2u);
            asm volatile("" : "+v"(xrows_b), "+v"(col_base));
            const float *const xrows = lds_floats_at(xrows_b);   // rows tau0 + 1 - gl ... + U - 1, contiguous (the copy behind the ring)
#pragma unroll
            for (int q = 0; q < U; ++q) {
                const int tau = tau0 + q;
                const int r = q % S;               // slot of this step's first column
                const int e = (r + C) % S;         // slot of the column entering at tau + 1 (dead during this step)
                float d[C];
                // the entering column first: its slot is dead since the previous macro-step's branch
                read_col(yf[e], q);
                // The row frame of the NEXT macro-step replaces this one's piece by piece, each 16-byte piece as soon as the nine
                // chains are through with it (k ascending in every chain, as frame_sq_expanded_pre has it: the same bits), so
                // that the reads have the rest of the chains, the minimum and the branch in front of their first use.  The
                // empty asm statements keep the scheduler from sinking a read to its first use or the chains past it.
                const float *const xnext = xrows + q * RS;
                const float thr = (xs[D] + nmax_b) * tau_thr;
#pragma unroll
                for (int c = 0; c < C; ++c) d[c] = xs[D] + yf[(r + c) % S][D];
#pragma unroll
                for (int piece = 0; piece < LPF; ++piece) {
#pragma unroll
                    for (int k = 4 * piece; k < 4 * piece + 4 && k < D; ++k)
#pragma unroll
                        for (int c = 0; c < C; ++c) d[c] = __builtin_fmaf(xs[k], yf[(r + c) % S][k], d[c]);
#pragma unroll
                    for (int c = 0; c < C; ++c) asm volatile("" : "+v"(d[c]) : : "memory");
                    read_frame_piece_lds<DN>(xs, xnext, piece);
                }
                float dmin = d[0];
#pragma unroll
                for (int c = 1; c + 1 < C; c += 2) dmin = __builtin_fminf(__builtin_fminf(dmin, d[c]), d[c + 1]);
                if (C % 2 == 0) dmin = __builtin_fminf(dmin, d[C - 1]);
                const bool any = dmin < thr;
                asm volatile("" : : : "memory");
                if (__builtin_expect(__ballot(any) != 0ull, 0)) {
                    // rare: this step's row frame once more (xs is on its way to the next one), the exact form where the cell's
                    // own test asks for it, then the next row's reads again -- the registers are the same on both paths
                    float xc[DN];
                    read_frame_lds<DN>(xc, &xring[((tau - gl) & (R - 1)) * RS]);
                    float nx = xc[D];
                    asm volatile("" : "+v"(nx));
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        const float sc = nx + yf[(r + c) % S][D];
                        const float ex = frame_sq_exact_pre<D>(xc, yf[(r + c) % S]);
                        d[c] = (d[c] < sc * tau_thr) ? ex : d[c];
                    }
                    asm volatile("" : : : "memory");
                    read_frame_lds<DN>(xs, xnext);
                }
#pragma unroll
                for (int c = 0; c < C; ++c) d[c] = __builtin_amdgcn_sqrtf(d[c]);
                dp_rows_step<C, G, true>(prev1, prev2, d, g1, g2, del, ins, mat, gl);
                if (SLOW) slow_phase_captures<C>(prev1, prev2, res1, res2, tau, gl, tau_cap, cw, cstar);
            }
            fill_store(tau0 + U + 1, fill_regs);
            if (fill_act) *reinterpret_cast<apd_f32x4 *>(ring_at(cring_fill, pf) + 4 * fill_q) = col_regs;
            if (fill_act && pf < (uint32_t)U) *reinterpret_cast<apd_f32x4 *>(ring_at(cring_fill, pf + RC) + 4 * fill_q) = col_regs;
            pf = min(pf + (uint32_t)U, pf + (uint32_t)U - (uint32_t)RC);   // one wrap: pf + U - RC is huge (unsigned) until pf + U reaches RC
            pr = min(pr + (uint32_t)U, pr + (uint32_t)U - (uint32_t)RC);
            __syncthreads();                                     // the next block reads what the four wavefronts just stored
        }
    };
    macro_steps(0, a_end, std::true_type{});
    macro_steps(a_end, b_end, std::false_type{});
    macro_steps(b_end, total_r, std::true_type{});

    if (P.valid && gl == (sweep ? ustar / C : 0)) {
        if (sweep) {
            const float denom = (float)(n + m);
            store_pair_rows_b(L, tile, P, res1 / denom, res2 / denom);
        } else {
            const float s = (P.n == 1 && P.m == 1) ? 0.0f : APD_INF;
            store_pair(L, tile, P, s, s);
        }
    }
}

// LDS of one workgroup of dtw_fused_systolic_shared<D, C, G>: four row rings, four column rings, the workgroup's words
template <int D, int C, int G>
constexpr size_t shared_columns_lds_bytes()
{
    constexpr int DP = (D + 1 + 3) & ~3, U = shared_column_unroll(C), RC = shared_column_ring_frames(G, C);
    constexpr int XRING = (64 + U) * (DP + 4), CRING = shared_column_ring_floats(RC, U, DP);
    return (size_t)(4 * XRING + (64 / G) * CRING + 8) * sizeof(float);
}
template <int D, int C, int G>
static hipError_t launch_shared_columns_kernel(const AlignLaunch &L, hipStream_t stream)
{
    constexpr int WPT = kSlotsPerTile / (4 * (64 / G));
    constexpr size_t lds = shared_columns_lds_bytes<D, C, G>();
    static_assert(lds <= 80 * 1024, "two workgroups per CU");
    // beyond the 64 KB default: asked for once per device (a race between two first launches asks twice, harmlessly)
    static bool granted[64] = {};
    int dev = 0;
    if (hipError_t e = hipGetDevice(&dev); e != hipSuccess) return e;
    if (dev < 0 || dev >= 64 || !granted[dev]) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(dtw_fused_systolic_shared<D, C, G>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        if (dev >= 0 && dev < 64) granted[dev] = true;
    }
    const uint32_t tiles8 = (L.n_tiles + 7u) / 8u * 8u;
    hipLaunchKernelGGL((dtw_fused_systolic_shared<D, C, G>), dim3(tiles8 * WPT), dim3(256), lds, stream, L);
    return hipSuccess;
}

// The three instantiations of one (D, C, G) live in two translation units -- dtw_sys.hip: hybrid form and the literal select
// (non-unit penalties); dtw_sysx.hip (APD_SYSTOLIC_STRICT_UNIT): strict mode's <.., true, false> -- so that each is compiled
// once per D, in parallel, with the scheduler flags measured for its own instruction mix (csrc/Makefile).
template <int D, int C, int G, bool UNIFORM_PEN, bool HYBRID>
static void launch_systolic_kernel(const AlignLaunch &L, hipStream_t stream)
{
    constexpr int PPW = 64 / G;
    constexpr int WPT = kSlotsPerTile / (4 * PPW);
    const uint32_t tiles8 = (L.n_tiles + 7u) / 8u * 8u;
    hipLaunchKernelGGL((dtw_fused_systolic<D, C, G, UNIFORM_PEN, HYBRID>), dim3(tiles8 * WPT), dim3(256), 0, stream, L);
}

#ifdef APD_SYSTOLIC_STRICT_UNIT
template <int D>
bool launch_systolic_strict(const AlignLaunch &L, KernelGeom g, hipStream_t stream)
{
#define APD_CASE(GG, CC) if constexpr (geom_instantiated(KernelGeom{KernelGeom::Systolic, GG, CC}, D)) { \
        if (g == KernelGeom{KernelGeom::Systolic, GG, CC}) { launch_systolic_kernel<D, CC, GG, true, false>(L, stream); return true; } }
    APD_SYSTOLIC_GEOMS(APD_CASE)
#undef APD_CASE
    return false;
}
#else
template <int D>
bool launch_systolic(const AlignLaunch &L, KernelGeom g, hipStream_t stream)
{
    // unit penalties: the fast select, either distance form; anything else: literal select on strict (bit-faithful) distances
    const bool unit = L.band.ins == 1.0f && L.band.del == 1.0f && L.band.mat == 1.0f;
    if (g.family == KernelGeom::SharedColumns) {                 // hybrid form, unit penalties only: the plan names it for nothing else
        if (!(unit && L.hybrid)) return false;
#define APD_CASE(GG, CC) if constexpr (geom_instantiated(KernelGeom{KernelGeom::SharedColumns, GG, CC}, D)) { \
        if (g == KernelGeom{KernelGeom::SharedColumns, GG, CC}) return launch_shared_columns_kernel<D, CC, GG>(L, stream) == hipSuccess; }
        APD_SHARED_COLUMN_GEOMS(APD_CASE)
#undef APD_CASE
        return false;
    }
    if (unit && !L.hybrid) return launch_systolic_strict<D>(L, g, stream);
#define APD_CASE(GG, CC) if constexpr (geom_instantiated(KernelGeom{KernelGeom::Systolic, GG, CC}, D)) { \
        if (g == KernelGeom{KernelGeom::Systolic, GG, CC}) { \
            if (!unit) launch_systolic_kernel<D, CC, GG, false, false>(L, stream); else launch_systolic_kernel<D, CC, GG, true, true>(L, stream); \
            return true; } }
    APD_SYSTOLIC_GEOMS(APD_CASE)
#undef APD_CASE
    return false;
}
#endif

}  // namespace apd
