// Internal declarations shared by the HIP translation units of libapd_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <iterator>
#include <map>
#include <set>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/apd.h"

struct apd_context;
namespace apd {

constexpr int kTile = 16;              // sequences per tile side -> 256 pair slots per tile
constexpr int kSlotsPerTile = kTile * kTile;
constexpr int kWave = 64;

// How the per-pair Sakoe-Chiba band is obtained.
struct BandSpec {
    float pct;                 // Discovery.warping_band_percentage (discovery.rs:40)
    uint32_t explicit_band;    // AlignmentParams.warping_band when use_explicit
    int use_explicit;
    float ins, del, mat;
};

// One launch of the fused-pair alignment over a list of tiles.
struct AlignLaunch {
    const float *d_frames;       // resident layout, see dtw_generic.hip: [frames | sentinel H | sentinel E] per sequence, dpad floats per frame
    uint32_t frames_bytes;       // size of d_frames in bytes (0 if >= 4 GiB: buffer addressing unavailable)
    const uint32_t *d_seq_off;   // [n_seq+1] padded frame offsets (sequence s owns seq_off[s+1]-seq_off[s]-2 real frames)
    const float *d_seq_nmax;     // [n_seq] largest squared frame norm of every resident sequence (bound of the hybrid form's threshold test)
    const uint4 *d_tiles;        // [n_tiles] (tile_a, tile_b, index of the tile in the slab, unused), tile_a <= tile_b
    uint32_t n_tiles;
    uint32_t n_seq;
    uint32_t dim, dpad;
    BandSpec band;
    float *d_slab;               // [tiles of the rank][2][kTile][kTile]
    // Device-side choice between the fast kernels and the literal, NaN-faithful one (no host round trip): the word the repack
    // kernel raises when a frame holds a NaN / infinity.  Fast kernels return at once when it is set; the fallback launch of
    // the generic kernel (launch_generic_fallback) returns at once when it is clear.  nullptr: no check.
    const uint32_t *d_nonfinite;
    uint32_t w_max;              // upper bound of w over the pairs of this launch
    uint32_t n_max;              // upper bound of the longer length over the pairs of this launch
    int variant;                 // 0 auto
    int hybrid;                  // 1: norm-expansion distances with exact recomputation below tau (see dtw_systolic.h)
    int strict;                  // 1: the reference's arithmetic operation for operation, whatever the penalties (apd_set_distance_mode 2)
    float tau;
};

// Frame dimensions with instantiated kernels.  A batch of another dimension <= 26 is zero-padded up to the next one when it
// is made resident (zero components change neither (x - y)^2 sums nor norms and dot products, bit for bit).
constexpr int kKernelDims[] = {8, 10, 13, 16, 20, 26};
constexpr bool is_kernel_dim(uint32_t d) { for (int k : kKernelDims) if ((uint32_t)k == d) return true; return false; }
constexpr uint32_t kernel_dim(uint32_t d) { for (int k : kKernelDims) if ((uint32_t)k >= d) return (uint32_t)k; return d; }
// Cells per lane the register file holds: (C + 2) frames of ceil4(D + 1) floats plus ~50 registers of state.
constexpr int max_cells_per_lane(uint32_t d) { return d <= 13 ? 9 : (d <= 16 ? 7 : 5); }
// Column strips of the full-matrix kernel hold CW frames per lane and one DP row: wider strips fit.
constexpr int max_strip_columns(uint32_t d) { return d <= 10 ? 13 : (d <= 13 ? 11 : max_cells_per_lane(d)); }   // 13 x 14 floats do not fit at D = 13

// ---- kernel geometry: which kernel family sweeps a tile class, and with which shape.
struct KernelGeom {
    enum Family : uint8_t { Generic, Systolic, Wide, Strip, BandedStrip, SharedColumns };
    Family family = Generic;
    uint8_t lanes_or_waves = 0;   // systolic, shared columns: lanes per pair G; wide: wavefronts per pair NW; strips: pairs per wavefront
    uint8_t cells = 0;            // offsets per lane C (band form), columns per lane CW (strips)

    // The integer form of apd_set_variant, the tile-plan cache key and the APD_DEBUG_PLAN line: 0 generic, G * 100 + C systolic,
    // 10000 + NW * 100 + C wide, 20000 + ppw * 100 + CW column strips, 30000 + ppw * 100 + CW banded column strips,
    // 40000 + G * 100 + C systolic with workgroup-shared column rings (the tiles that qualify; the others fall to G * 100 + C).
    constexpr int encode() const
    {
        constexpr int base[] = {0, 0, 10000, 20000, 30000, 40000};
        return family == Generic ? 0 : base[family] + lanes_or_waves * 100 + cells;
    }
    // any other code (1 .. 99, negative, >= 50000) decodes to Generic
    static constexpr KernelGeom decode(int key)
    {
        const Family f = key >= 100 && key < 10000 ? Systolic : key >= 10000 && key < 20000 ? Wide
                       : key >= 20000 && key < 30000 ? Strip : key >= 30000 && key < 40000 ? BandedStrip
                       : key >= 40000 && key < 50000 ? SharedColumns : Generic;
        if (f == Generic) return KernelGeom{};
        return KernelGeom{f, (uint8_t)((key % 10000) / 100), (uint8_t)(key % 100)};
    }
    // work-items per pair (the launches are cut at 2^31 work-items): the generic and strip kernels use at most one wavefront
    constexpr uint32_t lanes_per_pair() const
    {
        return family == Systolic || family == SharedColumns ? lanes_or_waves : family == Wide ? 64u * lanes_or_waves : 64u;
    }
    // offsets (band form) or columns (strips) one pair covers per pass
    constexpr uint32_t capacity() const { return (family == Wide ? 64u : 1u) * lanes_or_waves * cells; }
    constexpr bool operator==(KernelGeom o) const { return family == o.family && lanes_or_waves == o.lanes_or_waves && cells == o.cells; }
    constexpr bool operator<(KernelGeom o) const { return encode() < o.encode(); }   // tile classes run in this order
};

// The instantiated geometries, one list per family: the launchers (dtw_systolic.h, dtw_wide.h, dtw_full.h) expand them into
// their compile-time cases, the dispatcher (dtw_generic.hip) walks them in this order for its automatic choices and tests a
// forced variant against them.  max_cells_per_lane / max_strip_columns above drop the entries a frame dimension cannot hold
// (geom_instantiated), in the launchers and the dispatcher alike.
#define APD_SYSTOLIC_GEOMS(X) X(8, 5) X(8, 7) X(8, 9) X(16, 2) X(16, 3) X(16, 5) X(16, 7) X(16, 9) X(32, 5) X(32, 7) X(32, 9) \
                              X(64, 3) X(64, 5) X(64, 7) X(64, 9)
#define APD_WIDE_GEOMS(X) X(2, 5) X(2, 7) X(2, 9) X(4, 5) X(4, 7) X(4, 9) X(8, 5) X(8, 7) X(8, 9)   // ascending capacity
#define APD_STRIP_GEOMS(X) X(1, 3) X(1, 5) X(1, 7) X(1, 9) X(1, 11) X(1, 13) X(2, 3) X(2, 5) X(2, 7) X(2, 9) X(2, 11) X(2, 13) \
                           X(4, 3) X(4, 5) X(4, 7) X(4, 9) X(4, 11) X(4, 13)
#define APD_BANDED_STRIP_GEOMS(X) X(1, 5) X(1, 9) X(4, 5) X(4, 9)
// shared column rings: the hybrid form with unit penalties only, four pairs per wavefront (one ring per wavefront of the workgroup)
#define APD_SHARED_COLUMN_GEOMS(X) X(16, 9)

#define APD_SYSTOLIC_ENTRY_(A, B) KernelGeom{KernelGeom::Systolic, A, B},
#define APD_WIDE_ENTRY_(A, B) KernelGeom{KernelGeom::Wide, A, B},
#define APD_STRIP_ENTRY_(A, B) KernelGeom{KernelGeom::Strip, A, B},
#define APD_BANDED_STRIP_ENTRY_(A, B) KernelGeom{KernelGeom::BandedStrip, A, B},
#define APD_SHARED_COLUMN_ENTRY_(A, B) KernelGeom{KernelGeom::SharedColumns, A, B},
constexpr KernelGeom kSystolicGeoms[] = {APD_SYSTOLIC_GEOMS(APD_SYSTOLIC_ENTRY_)};
constexpr KernelGeom kWideGeoms[] = {APD_WIDE_GEOMS(APD_WIDE_ENTRY_)};
constexpr KernelGeom kStripGeoms[] = {APD_STRIP_GEOMS(APD_STRIP_ENTRY_)};
constexpr KernelGeom kBandedStripGeoms[] = {APD_BANDED_STRIP_GEOMS(APD_BANDED_STRIP_ENTRY_)};
constexpr KernelGeom kSharedColumnGeoms[] = {APD_SHARED_COLUMN_GEOMS(APD_SHARED_COLUMN_ENTRY_)};
#undef APD_SYSTOLIC_ENTRY_
#undef APD_WIDE_ENTRY_
#undef APD_STRIP_ENTRY_
#undef APD_BANDED_STRIP_ENTRY_
#undef APD_SHARED_COLUMN_ENTRY_

// Every frame dimension of the dispatch, as a compile-time constant: f(std::integral_constant<int, D>{}).  false: no kernels for `dim`.
template <class F, size_t... I>
bool with_kernel_dim_(uint32_t dim, F &&f, std::index_sequence<I...>)
{
    return ((dim == (uint32_t)kKernelDims[I] ? (f(std::integral_constant<int, kKernelDims[I]>{}), true) : false) || ...);
}
template <class F>
bool with_kernel_dim(uint32_t dim, F &&f) { return with_kernel_dim_(dim, f, std::make_index_sequence<std::size(kKernelDims)>{}); }

// The one test of "a kernel exists for g at frame dimension dim": on the family's list and within the dimension's clamp.
constexpr bool geom_instantiated(KernelGeom g, uint32_t dim)
{
    if (g.family == KernelGeom::Generic) return true;
    if (!is_kernel_dim(dim)) return false;
    const bool strip = g.family == KernelGeom::Strip;
    if (g.cells > (strip ? max_strip_columns(dim) : max_cells_per_lane(dim))) return false;
    auto on = [g](const auto &list) { for (KernelGeom e : list) if (e == g) return true; return false; };
    return g.family == KernelGeom::Systolic ? on(kSystolicGeoms) : g.family == KernelGeom::Wide ? on(kWideGeoms)
         : g.family == KernelGeom::SharedColumns ? on(kSharedColumnGeoms) : strip ? on(kStripGeoms) : on(kBandedStripGeoms);
}
// the lists and their integer codes are one and the same: every entry decodes back to itself
template <size_t N>
constexpr bool geoms_round_trip(const KernelGeom (&list)[N])
{
    for (KernelGeom g : list) if (!(KernelGeom::decode(g.encode()) == g)) return false;
    return true;
}
static_assert(geoms_round_trip(kSystolicGeoms) && geoms_round_trip(kWideGeoms) && geoms_round_trip(kStripGeoms) &&
                  geoms_round_trip(kBandedStripGeoms) && geoms_round_trip(kSharedColumnGeoms), "a listed geometry has no integer code of its own");

// ---- sweep bounds of the systolic kernels (dtw_systolic.h, both of them).  Lane gl of a pair owns the band offsets C gl .. C gl + C - 1
// and sweeps row tau - gl in macro-step tau.  The result cell (rows - 1, cols - 1) has band offset u* = (cols - 1) - (rows - 1) + w
// (2 <= u* <= 2w - 2: w >= |rows - cols| + 2), lives in lane u* / C and is final once that lane has swept row rows - 1: nothing a
// later macro-step computes can reach it, so a pair needs sweep_steps_needed macro-steps, not the (rows - 1) + ceil((2w + 1) / C)
// that run every lane of the band through the last row.
__host__ __device__ constexpr int sweep_result_offset(int rows, int cols, int w) { return (cols - 1) - (rows - 1) + w; }
__host__ __device__ constexpr int sweep_capture_step(int rows, int cols, int w, int c)
{
    return (rows - 1) + sweep_result_offset(rows, cols, w) / c;
}
__host__ __device__ constexpr int sweep_steps_needed(int rows, int cols, int w, int c) { return sweep_capture_step(rows, cols, w, c) + 1; }
static_assert(sweep_result_offset(1000, 1024, 66) == 90 && sweep_capture_step(1000, 1024, 66, 9) == 1009 &&
                  sweep_steps_needed(1000, 1024, 66, 9) == 1010, "cfg 3's shape, rows the shorter sequence: lane 10 ends the sweep");
static_assert(sweep_steps_needed(1024, 1000, 66, 9) == 1028, "the same pair with the longer sequence as rows: u* = 42, lane 4");
static_assert(sweep_capture_step(40, 72, 34, 9) == 39 + 7 && (2 * 34 + 1 + 8) / 9 == 8,
              "|n - m| = w - 2: u* = 2w - 2 sits in the last active lane, nothing is cut at the end");
static_assert(sweep_steps_needed(2, 2, 2, 2) == 3 && sweep_steps_needed(72, 40, 34, 9) == 72, "smallest pair; u* = 2: lane 0");

// ---- shared column rings (dtw_systolic.h, dtw_fused_systolic_shared).  A workgroup sweeps a 4 x 4 sub-block of a tile: wavefront k
// row sequence b_k, its four lane groups the columns a_0 .. a_3, which the four wavefronts read from one LDS ring per a.
// A macro-step block is U steps (the kernel's unroll); during one, the G lanes of the pairs of the workgroup read columns
// spanning (G - 1)(C - 1) + U + (largest - smallest w of the workgroup's swept pairs), and the next block's U columns are
// written meanwhile.  The ring holds what equal bands need (shared_column_ring_min) and at least 16 frames more, in whole
// groups of 8 columns; what it holds beyond the minimum is the spread of w a workgroup may have (shared_column_slack).
constexpr int shared_column_unroll(int c) { return (c + 1) % 2 == 0 ? c + 1 : 2 * (c + 1); }
constexpr int shared_column_ring_min(int g, int c) { return (g - 1) * (c - 1) + 1 + 2 * shared_column_unroll(c); }
constexpr int shared_column_ring_frames(int g, int c) { return (shared_column_ring_min(g, c) + 16 + 7) / 8 * 8; }
// the spread of w one workgroup tolerates: what the ring holds beyond the window of equal bands
constexpr uint32_t shared_column_slack(KernelGeom g)
{
    return (uint32_t)(shared_column_ring_frames(g.lanes_or_waves, g.cells) - shared_column_ring_min(g.lanes_or_waves, g.cells));
}
inline uint32_t host_w(const BandSpec &b, uint32_t n, uint32_t m);   // below
// The qualification rule of the tile plan: in every 4 x 4 sub-block of tile (tile_a, tile_b) the swept pairs (a < b < n_seq, both
// longer than one frame) have bands within `slack` of each other.  lens[s]: frames of resident sequence s.
// Which sequence of a pair is swept as rows does not enter: a lane's column in macro-step tau is tau - gl + u - w whatever the rows
// are, so the span of columns a workgroup reads (and the ring span the kernel's static_assert bounds) depends on the pairs' w
// alone, w is symmetric in (n, m), and a workgroup's pairs are the same 4 x 4 sub-block under either assignment.
inline bool shared_columns_qualify(const std::vector<uint32_t> &lens, uint32_t tile_a, uint32_t tile_b, const BandSpec &band,
                                   uint32_t slack)
{
    const uint32_t n_seq = (uint32_t)lens.size();
    for (uint32_t sa = 0; sa < (uint32_t)kTile; sa += 4)
        for (uint32_t sb = 0; sb < (uint32_t)kTile; sb += 4) {
            uint32_t lo = 0xFFFFFFFFu, hi = 0;
            for (uint32_t i = 0; i < 16; ++i) {
                const uint32_t a = tile_a * kTile + sa + i / 4, b = tile_b * kTile + sb + i % 4;
                if (!(a < b && b < n_seq) || lens[a] < 2 || lens[b] < 2) continue;
                const uint32_t w = host_w(band, lens[a], lens[b]);
                lo = w < lo ? w : lo;
                hi = w > hi ? w : hi;
            }
            if (hi > lo && hi - lo > slack) return false;
        }
    return true;
}

// LDS of the column-strip kernels (dtw_full.h): row frames of their lanes, one boundary column per pair and DP, and a few words
constexpr uint64_t strip_lds_bytes(uint32_t dim, uint32_t ppw, bool banded, uint32_t rows)
{
    const uint64_t dp = (dim + 4) & ~3u;
    return 4 * ((ppw == 1 ? 128 : 64) * dp + (uint64_t)ppw * (banded ? 2 : 1) * (rows + 4) + 16);
}

// ---- warping paths (dtw_path.hip): one ordered pair per wavefront, a sweep that records every cell's branch and a trace.
constexpr uint32_t kPathMaxOffsets = 20480;   // 2w + 1 beyond this: the sweep's DP row does not fit in LDS (the literal kernel's limit)
// band offsets per lane of the sweep, as generic_pair chooses them
__host__ __device__ constexpr uint32_t path_cells_per_lane(uint32_t w) { return (2 * w + 1 + 63) / 64 < 2 ? 2u : (2 * w + 1 + 63) / 64; }
// direction words of a pair of n x m frames with half-width w: 2 bits per cell, ceil(C / 16) words per (macro-step, lane), n + 63
// macro-steps (rows 1 .. n-1 on 64 lanes); none when either length is 1 (nothing is swept)
inline uint64_t path_dir_words(uint32_t n, uint32_t m, uint32_t w)
{
    if (n < 2 || m < 2) return 0;
    return ((uint64_t)n + 63) * ((path_cells_per_lane(w) + 15) / 16) * 64;
}
struct PathPair {
    uint32_t px, py;       // resident positions of x and y
    uint64_t dir_off;      // first direction word of the pair in d_dirs
    uint64_t step_off;     // first step slot of the pair in d_steps
};
struct PathLaunch {
    const float *d_frames;
    const uint32_t *d_seq_off;
    uint32_t dim, dpad;
    BandSpec band;
    const PathPair *d_pairs;
    uint32_t n_pairs;
    uint32_t *d_dirs;
    apd_path_step *d_steps;
    uint32_t *d_len;       // [n_pairs] steps used
    float *d_scores;       // [n_pairs]
    // an x side of its own (apd_barycenters: one "sequence" per set, in the resident frame layout); px then indexes d_x_seq_off.
    // Both null: x comes from d_frames / d_seq_off like y.
    const float *d_x_frames;
    const uint32_t *d_x_seq_off;
};
hipError_t launch_path_sweep(const PathLaunch &L, uint32_t c_max, hipStream_t stream);
hipError_t launch_path_trace(const PathLaunch &L, hipStream_t stream);

// ---- DTW barycenters (dtw_path.hip): the averaging around the sweep and the trace.  The barycenters live in the resident frame
// layout -- set k owns frames d_bary_off[k] .. d_bary_off[k + 1] - 3 of dpad floats, two padding frames behind, d_bary_off[k] =
// sum of T + 2 k -- so that the path kernels take them as their x side.  d_sum / d_cnt: the running sums and counts of one
// iteration, per padded frame; d_score_sum / d_used: per set.  The chunk fields describe the paths a trace has just left on the
// device: d_set_pairs[k] = the chunk's pairs [x, y) of set k, members ascending.
struct BaryLaunch {
    const float *d_frames;          // the batch: the y side
    const uint32_t *d_seq_off;
    float *d_bary;
    const uint32_t *d_bary_off;     // [n_sets + 1]
    uint32_t n_sets, n_padded;      // n_padded = d_bary_off[n_sets]
    uint32_t dim, src_dim, dpad;
    float *d_sum;                   // [n_padded][dpad]
    uint32_t *d_cnt;                // [n_padded]
    float *d_score_sum;             // [n_sets]
    uint32_t *d_used;               // [n_sets]
    const PathPair *d_pairs;
    const uint2 *d_set_pairs;       // [n_sets]
    const apd_path_step *d_steps;
    const uint32_t *d_len;
    const float *d_scores;
    uint32_t *d_contrib;            // [pairs of the chunk] 1: the path reached the origin
};
// d_init_pos[k]: resident position of the sequence that starts set k's barycenter; writes every float of d_bary
hipError_t launch_bary_init(const BaryLaunch &L, const uint32_t *d_init_pos, hipStream_t stream);
// the chunk's contribution to d_score_sum / d_used (and d_contrib), then to d_sum / d_cnt
hipError_t launch_bary_accumulate(const BaryLaunch &L, hipStream_t stream);
// ends an iteration: the new frames, d_inertia[k] and d_used_out[k]
hipError_t launch_bary_finalize(const BaryLaunch &L, float *d_inertia, uint32_t *d_used_out, hipStream_t stream);
// d_out: [sum of T][src_dim], the caller's packing
hipError_t launch_bary_pack(const BaryLaunch &L, float *d_out, hipStream_t stream);

// ---- subsequence alignment (dtw_spot.hip): one (query, stream) pair per wavefront, lane l owns ceil(n / 64) consecutive query rows.
constexpr uint32_t kSpotMaxQuery = 16384;     // frames of a query: 256 rows per lane, 128 KB of LDS for the lane columns
constexpr uint32_t kSpotMaxStream = 0xFFFF0000u;   // frames of a stream: query + window + 1 stays below 2^32
constexpr uint32_t kSpotRegisterRows = 4;     // rows per lane the kernels hold in registers
constexpr uint32_t kSpotClasses = kSpotRegisterRows + 1;   // kernel classes: the host's buckets and the launcher's fold (dtw_spot_sweep.h)
constexpr uint32_t spot_rows_per_lane(uint32_t n) { return (n + 63) / 64; }
// The kernel class of a query of n frames at resident dimension dim: R = 1 .. kSpotRegisterRows rows per lane in registers (frame
// dimensions with instantiated kernels only), 0: the lane columns in LDS.
constexpr uint32_t spot_row_class(uint32_t dim, uint32_t n)
{
    return is_kernel_dim(dim) && spot_rows_per_lane(n) <= kSpotRegisterRows ? spot_rows_per_lane(n) : 0u;
}
constexpr bool spot_row_classes_hold()
{
    for (int d : kKernelDims) {
        for (uint32_t r = 1; r < kSpotClasses; ++r)
            if (spot_row_class(d, 64 * (r - 1) + 1) != r || spot_row_class(d, 64 * r) != r) return false;
        if (spot_row_class(d, 64 * kSpotRegisterRows + 1) != 0 || spot_row_class(d, kSpotMaxQuery) != 0) return false;
    }
    return true;
}
static_assert(spot_row_classes_hold(), "spot_row_class names the classes 0 .. kSpotClasses - 1, r rows per lane as class r, and no other");
// Where the query rows and the penalties of a spotting launch are: the head of every spotting launch struct (spot_source, apd_host.h).
struct SpotSource {
    const float *d_frames;
    const uint32_t *d_seq_off;
    uint32_t dim, dpad;
    float ins, del, mat;
};
// The score of a spotted window [start, end] of cost `cost` under a query of n frames, for the sweep's running best, the traces,
// detection and online detection alike: the window and the sum in u32 (< 2^32: kSpotMaxStream), one conversion, one f32 division
// (alignments.rs:121 with the window for m).
__device__ __forceinline__ float spot_score(float cost, uint32_t end, uint32_t start, uint32_t n)
{
    const uint32_t window = end - start + 1u;                     // frames of the stream the alignment covers
    return cost / (float)(n + window);
}
// The sort key of a score in both detections: the usual monotone map of f32 onto u32 (the sign bit flipped for a non-negative score,
// every bit for a negative one) after both zeros were made +0.0, so that -0.0 and +0.0 tie as f32 < says they do.
__device__ __forceinline__ uint32_t spot_score_key(float score)
{
    const uint32_t b = score == 0.0f ? 0u : __float_as_uint(score);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
struct SpotPair {
    uint32_t px, py;       // resident positions of the query x and the stream y
    uint32_t out;          // the pair's record in d_best
    uint32_t pad;
    uint64_t curve_off;    // first entry of the pair's curves in d_cost / d_start
};
struct SpotLaunch {
    SpotSource src;
    const SpotPair *d_pairs;
    uint32_t n_pairs;
    float *d_cost;         // both null: best only
    uint32_t *d_start;
    apd_spot_best *d_best;
};
size_t spot_lds_bytes(uint32_t rows_per_lane);
// Under APD_DEBUG_PLAN, one stderr line per launch of a spotting kernel, printed where the template arguments are chosen:
//   [apd] spot <kind> kernel <RT, D>: <n> pairs                                  (rows in registers)
//   [apd] spot <kind> kernel <0, D>: <n> pairs, r_max <r>, lds <b> bytes         (lane columns in LDS; D = 0: any dimension)
// kind: the word of the kind type whose spot_kernel<Kind, RT, D> is launched (dtw_spot_sweep.h): "sweep" (SpotSweep), "record"
// (SpotRecordSweep), "stream" (SpotStreamSweep) or "streamrec" (SpotStreamRecordSweep).  The only report of which spotting kernel ran.
void spot_debug_line(const char *kind, int rt, int d, uint32_t n_pairs, uint32_t r_max, size_t lds_bytes);
// The pairs of L all have row class `rt`; r_max: the most rows per lane among them (class 0: sizes the LDS).
hipError_t launch_spot(const SpotLaunch &L, uint32_t rt, uint32_t r_max, hipStream_t stream);

// ---- the curves of a chunk (apd_spot_detect, apd_spot_quantiles): what launch_spot left in the workspace, read again by a second
// stage.  A chunk holds whole groups; its pairs are numbered group by group (a group's pairs adjacent, in the caller's order:
// GroupChunkPlan, apd_plan.h), so a group's curve entries are one stretch.  The column walk over a record: dtw_spot_curves.h.
struct SpotCurve {
    uint64_t curve_off;    // first entry of the pair's curves in d_cost / d_start
    uint32_t m, n;         // frames of the stream and of the query
    uint32_t group;        // of the chunk
    uint32_t pair;         // the caller's index into `pairs`
};
static_assert(sizeof(SpotCurve) == 24, "include/apd.h states the workspace weights of apd_spot_quantiles: 64 bytes per pair");

// ---- spot detection (dtw_spot_detect.hip): candidates and greedy non-overlapping picking on the curves.  A group's candidate list
// -- one 16-byte slot per entry at most -- lies at the offset of its curve entries.
struct SpotDetectPair {
    SpotCurve curve;
    float threshold;
    uint32_t pad;
};
static_assert(sizeof(SpotDetectPair) == 32, "a detection record is the curve record, the threshold and a pad");
struct SpotDetectGroup {
    uint64_t cand_off;     // first slot of the group's candidate list in d_cand = first curve entry of its first pair
    uint64_t cand_cap;     // its slots: the group's curve entries
    uint64_t stage_off;    // first slot of the group's accepted windows in d_stage
    uint32_t stage_cap;    // its slots: frames of the group's stream (disjoint windows cover one column each at least)
    uint32_t pad;
};
struct SpotDetectLaunch {
    const float *d_cost;
    const uint32_t *d_start;
    const SpotDetectPair *d_pairs;
    uint32_t n_pairs;
    const SpotDetectGroup *d_groups;
    uint32_t n_groups;
    ulonglong2 *d_cand;                  // (sortable score << 32 | end, pair of the chunk << 32 | start)
    unsigned long long *d_cand_count;    // [n_groups], zeroed by the caller
    uint2 *d_stage;                      // (pair of the chunk, end) in acceptance order
    uint32_t *d_hit_count;               // [n_groups]
    unsigned long long *d_hit_base;      // [n_groups + 1] exclusive prefix of d_hit_count
};
// marking, picking and the prefix of the hit counts; m_max: the longest stream among the pairs
hipError_t launch_spot_detect(const SpotDetectLaunch &L, uint32_t m_max, hipStream_t stream);
// d_hits[0 .. n_write): the chunk's first n_write hits, group-major
hipError_t launch_spot_detect_emit(const SpotDetectLaunch &L, apd_spot_hit *d_hits, uint64_t n_write, hipStream_t stream);

// ---- spot score quantiles (dtw_spot_quantile.hip): a radix select over spot_score_key on the curves; its pairs are SpotCurve records.
constexpr uint32_t kSpotQuantileColumns = 256;      // columns a workgroup of the pass kernel takes per step (its work-items)
constexpr uint32_t kSpotQuantileBins = 257;         // the 256 digits of a pass, and the NaN scores
constexpr uint32_t kSpotQuantileWorkgroups = 2048;  // workgroups of a pass the column blocks are chosen to reach (spot_quantile_blocks)
// One (group, quantile) of a chunk between the passes: uploaded with rank = k and zeros.
struct SpotQuantileState {
    uint64_t rank;         // the rank left among the keys that match `prefix` under `mask`
    uint32_t prefix, mask; // the digits found so far, in place
    int32_t verdict;       // APD_OK, or APD_ERR_INDEX once k proved to lie beyond the non-NaN scores
    uint32_t pad;
};
struct SpotQuantileLaunch {
    const float *d_cost;
    const uint32_t *d_start;
    const SpotCurve *d_pairs;
    uint32_t n_pairs;
    uint32_t n_groups, n_perc;
    SpotQuantileState *d_state;          // [n_groups][n_perc]
    unsigned long long *d_hist;          // [n_groups][n_perc][kSpotQuantileBins], zeroed by the caller; zero again afterwards
    float *d_values;                     // [n_groups][n_perc]
    int32_t *d_status;                   // [n_groups][n_perc]
    unsigned long long *d_nans;          // [n_groups]
};
uint32_t spot_quantile_blocks(uint32_t n_pairs, uint32_t m_max);
// the four passes; m_max: the longest stream among the pairs
hipError_t launch_spot_quantiles(const SpotQuantileLaunch &L, uint32_t m_max, hipStream_t stream);

// ---- streaming spotting (dtw_spot_stream.hip): the sweep above entered and left in mid-stream.  A session (apd_spot_stream) keeps,
// per pair p = channel n_queries + q, the last pushed column of the table and the running best on the device; a push sweeps every
// channel's chunk from there.  Query rows come from the templates' batch, stream columns from the session's staging buffer.
struct SpotStreamPair {
    uint32_t px;           // resident position of the query in the templates' batch
    uint32_t channel;
    uint32_t out;          // p: the pair's record in d_best, and its place in the curves
    uint32_t rows;         // rows per lane R = spot_rows_per_lane(n): the pair's state is [R][64] values, then [R][64] starts
    uint64_t state_off;    // first float of the pair's state in either half of d_state
};
struct SpotStreamLaunch {
    SpotSource src;                  // the templates
    const float *d_stage;            // the chunks of this push, packed, in the resident layout (dpad floats per frame)
    // what a push uploads, n_channels + 1 | n_channels | n_channels words: first staged frame of every channel's chunk (and the
    // total); absolute column of the channel's last frame before this push; which half of d_state holds the channel's column
    const uint32_t *d_push;
    uint32_t n_channels, n_queries;
    const SpotStreamPair *d_pairs;
    uint32_t n_pairs;
    float *d_state;                  // two halves of state_half floats: a sweep reads one and writes the other
    uint64_t state_half;
    float *d_cost;                   // both null: best only
    uint32_t *d_start;
    apd_spot_best *d_best;           // [n_queries n_channels], the session's: read at the start of a sweep, written at its end
};
// The pairs of S all have row class `rt`, as for launch_spot; kind "stream" on the APD_DEBUG_PLAN line.
hipError_t launch_spot_stream(const SpotStreamLaunch &S, uint32_t rt, uint32_t r_max, hipStream_t stream);
// S.d_pairs: every pair of the session; resets those of `channel` (0xFFFFFFFF: all) to column 0 and no best.
hipError_t launch_spot_stream_reset(const SpotStreamLaunch &S, uint32_t channel, hipStream_t stream);

// ---- warping paths of spotted windows (dtw_spot_path.hip): the sweep above once per distinct (query, stream) pair of a chunk,
// recording the branch of every cell whose column some window of the pair covers, then one wavefront per window walking back.
// Columns [a, b] of a stream whose branches are kept, and the first of the interval's words in d_dirs (dtw_spot_sweep.h).
struct SpotInterval {
    uint32_t a, b;
    uint64_t off;
};
// Direction words an interval of `columns` columns owns for a query of n frames: 2 bits per cell, 16 rows of a lane per word.
constexpr uint64_t spot_dir_words(uint32_t n, uint64_t columns) { return (columns + 63) * ((spot_rows_per_lane(n) + 15) / 16) * 64; }
struct SpotRecPair {
    uint32_t px, py;       // resident positions of the query x and the stream y
    uint32_t max_end;      // the last column swept: the pair's largest requested end
    uint32_t n_iv;         // the pair's intervals: d_intervals[iv_first .. iv_first + n_iv), ascending and disjoint
    uint32_t iv_first;
    uint32_t n_ends;       // the pair's requested ends: d_ends[end_first .. end_first + n_ends), ascending and distinct
    uint32_t end_first;
    uint32_t pad;
};
struct SpotTraceWindow {
    uint32_t px, py;
    uint32_t end, start;   // the caller's window
    uint32_t a;            // first column of the interval that holds the window
    uint32_t end_slot;     // where the sweep left T[n][end] and S[n][end]: d_end_cost / d_end_start
    uint64_t dir_off;      // first word of that interval in d_dirs
    uint64_t step_off;     // first step slot of the window in d_steps
};
struct SpotPathLaunch {
    SpotSource src;
    const SpotRecPair *d_pairs;        // the sweep's grid
    uint32_t n_pairs;
    const SpotInterval *d_intervals;
    const uint32_t *d_ends;
    float *d_end_cost;
    uint32_t *d_end_start;
    uint32_t *d_dirs;
    const SpotTraceWindow *d_windows;  // the trace's grid
    uint32_t n_windows;
    apd_path_step *d_steps;
    uint32_t *d_len;                   // [n_windows] steps used
    uint32_t *d_found;                 // [n_windows] S[n][end]
    float *d_scores;                   // [n_windows]
};
// The pairs of L all have row class `rt`, as for launch_spot.
hipError_t launch_spot_record(const SpotPathLaunch &L, uint32_t rt, uint32_t r_max, hipStream_t stream);
hipError_t launch_spot_trace(const SpotPathLaunch &L, hipStream_t stream);

// ---- streaming spotting with a history (dtw_spot_stream_rec.hip): a session that keeps the last `rows` = H pushed columns -- the
// branches of every pair's cells, row n's value and start, and every channel's frames -- in rings on the device, and traces windows
// that still lie inside them (include/apd.h, apd_spot_stream_keep / _paths).  The branch and curve rings are indexed by ABSOLUTE
// macro-step (dtw_spot_sweep.h, SpotRing), the frame ring by absolute column.
struct SpotHistory {
    uint32_t rows;                   // H >= 1
    uint32_t *d_dirs;                // pair p: rows x WPL_p x 64 words from word d_wpl_before[p] * rows * 64
    const uint32_t *d_wpl_before;    // [n_pairs] by p: the sum of WPL = ceil(R / 16) over the pairs before p
    float *d_curve_v;                // pair p: [p * rows ..), T[n][J] at row (J + lane of row n) mod rows
    uint32_t *d_curve_s;             //         S[n][J], absolute
    float *d_frames;                 // channel k: [k * rows * dpad ..), the resident frame of column J at row J mod rows
};
struct SpotStreamRecLaunch {
    SpotStreamLaunch S;
    SpotHistory H;
};
// As launch_spot_stream, and every live cell's branch and row n's curve go to the rings; kind "streamrec" on the APD_DEBUG_PLAN line.
hipError_t launch_spot_stream_record(const SpotStreamRecLaunch &R, uint32_t rt, uint32_t r_max, hipStream_t stream);
// The last min(m, H) staged frames of every channel's chunk go to its frame ring; total: staged frames of the push (> 0).
hipError_t launch_spot_stream_frames(const SpotStreamRecLaunch &R, uint32_t total, hipStream_t stream);
struct SpotRingWindow {
    uint32_t px;           // resident position of the query
    uint32_t channel;
    uint32_t pair;         // p = channel n_queries + q
    uint32_t end, start;   // the caller's window, absolute columns; end lies inside the kept columns
    uint32_t first;        // the channel's first kept column: a start before it has aged out (no walk)
    uint64_t step_off;     // first step slot of the window in d_steps
};
struct SpotRingTraceLaunch {
    SpotSource src;                    // the templates
    SpotHistory H;
    const SpotRingWindow *d_windows;
    uint32_t n_windows;
    apd_path_step *d_steps;
    uint32_t *d_len;                   // [n_windows] steps used
    uint32_t *d_found;                 // [n_windows] S[n][end]
    float *d_scores;                   // [n_windows]
};
hipError_t launch_spot_stream_trace(const SpotRingTraceLaunch &L, hipStream_t stream);

// ---- online spot detection (dtw_spot_online.hip): the hold-off machine of an armed session (include/apd.h, "streaming spotting,
// online detection").  It reads the curves a push's sweeps have just left in the session's buffer -- pair p = channel n_queries + q
// owns the m entries of its channel's chunk behind those of the pairs before it, so a channel's pairs are adjacent -- and keeps 32
// bytes of state per group.  Group g is pair g, or (per_stream) channel g with its n_queries pairs.
struct SpotOnlinePair {
    uint32_t n;            // frames of the pair's query
    float threshold;
};
struct SpotOnlineState {
    uint32_t pair, end, start;   // the pending window P; end == 0: none (an absolute column is >= 1)
    float cost, score;           // the curve's bits at `end` and the score taken from them
    uint32_t floor;              // F: the end of the group's last emitted hit, or its origin
    uint32_t rank;               // emissions since arming
    uint32_t pad;
};
struct SpotOnlineLaunch {
    const float *d_cost;             // the push's curves (scan only)
    const uint32_t *d_start;
    const uint32_t *d_push;          // SpotStreamLaunch::d_push of the same push (scan only)
    uint32_t n_channels, n_queries;
    uint32_t per_stream;             // 0: a group per pair, 1: a group per channel
    uint32_t holdoff;                // 0xFFFFFFFF: the timer never fires
    uint32_t n_groups;
    const SpotOnlinePair *d_pairs;   // [n_channels n_queries] by p
    SpotOnlineState *d_state;        // [n_groups]
    apd_spot_hit *d_queue;           // emitted hits in arrival order (the drain orders them); queue_cap slots
    unsigned long long *d_count;     // hits queued
    uint64_t queue_cap;
};
// One workgroup per group walks its channel's chunk; a group of a channel whose chunk is empty does nothing.  Appends at most
// (chunk columns + 1) hits per group: the caller has sized the queue for that.  m_max: the longest chunk of the push (it sizes the
// workgroup: one wavefront per 64 columns, 16 at most and no more than fill the chip once; the hits do not depend on it).
hipError_t launch_spot_online_scan(const SpotOnlineLaunch &L, uint64_t m_max, hipStream_t stream);
// The groups of `channel` (0xFFFFFFFF: all).  flush: a pending window is emitted and becomes the floor.  Otherwise (a reset): the
// pending window is dropped and the floor becomes first_column; the rank stays.  Appends at most one hit per group.
hipError_t launch_spot_online_touch(const SpotOnlineLaunch &L, uint32_t channel, bool flush, uint32_t first_column, hipStream_t stream);

// One launch of the alignment kernel that geometry g names, cut into launches below 2^31 work-items.
hipError_t launch_align(const AlignLaunch &L, KernelGeom g, hipStream_t stream, std::string &err, int *status);
// The generic kernel over ALL tiles of L as a small persistent grid that does nothing unless *L.d_nonfinite is set.
// *fits = false (and nothing launched) if the band of L.w_max needs more LDS than a workgroup can have.
hipError_t launch_generic_fallback(const AlignLaunch &L, hipStream_t stream, bool *fits);
// true if the literal kernel can hold a band of w_max in LDS AND the runtime grants it that much (the hipFuncSetAttribute is made
// here, before anything is enqueued: a refusal sends the caller down the host-side choice instead of failing mid-call)
bool generic_fallback_fits(uint32_t w_max);
// true if the literal kernel's two DP rows of a band of w_max fit the 160 KB of LDS a workgroup can have: 2 * w_max + 1 <= 20480.
// Host arithmetic only (launch_align's own test, asked before a call enqueues anything).
bool generic_band_fits(uint32_t w_max);

// One launch of the tile plan: the tiles [first, first + count) of its device tile list, all swept with geometry `geom`.
struct TileClass { KernelGeom geom; uint32_t first, count, w_max, n_max; };
// The policy of the tile plan (dtw_generic.hip): which kernel geometry sweeps which of `tiles` (tile-row pairs, see
// rank_tile_list) of a batch whose resident sequence p spans offsets[p] .. offsets[p + 1].  `variant` is apd_set_variant's
// code.  Fills `classes` in geometry order and `flat`, the tile list they index: (tile_a, tile_b, index in the slab, 0).
void plan_tile_classes(const std::vector<uint64_t> &offsets, uint32_t n_seq, const std::vector<uint2> &tiles, const BandSpec &band,
                       uint32_t dim, int variant, bool fast_ok, bool uniform_pen, bool fast_shift, std::vector<TileClass> &classes,
                       std::vector<uint4> &flat);
// d_flags[0] is raised when a frame holds a NaN, an infinity or a non-zero feature outside [kFeatureFloor, kFeatureBound) (the fast
// kernels' selects, sentinels and distance forms assume finite features and normal squared distances)
// d_seq_nmax[p] (zeroed by the caller) receives the largest squared frame norm of resident sequence p
hipError_t launch_pad(const float *d_src, float *d_dst, const uint32_t *d_seq_off, const uint32_t *d_src_off, uint32_t n_seq,
                      uint64_t n_frames_padded, uint32_t src_dim, uint32_t dim, uint32_t dpad, uint32_t *d_flags, float *d_seq_nmax,
                      hipStream_t stream);
// writes EVERY entry of d_out (diagonal included); *d_status |= 1 when a pair score of a batch with finite frames is NaN,
// i.e. still carries the poison its slab was filled with before the alignment launches
hipError_t launch_unpack(const float *d_gathered, float *d_out, const uint32_t *d_order, uint32_t n_seq, uint32_t world,
                         uint64_t slab_floats, const uint32_t *d_flags, uint32_t *d_status, hipStream_t stream);
hipError_t launch_selftest(int *d_result, hipStream_t stream);
// Joined batches (apd_batch_join): flags_out[0] = flags_a[0] | flags_b[0], on the device.
hipError_t launch_join_flags(uint32_t *d_flags_out, const uint32_t *d_flags_a, const uint32_t *d_flags_b, hipStream_t stream);
// The rectangular unpack of apd_align_cross.  d_slab: [tiles][2][kTile][kTile] over the tile rectangle ta in [0, ceil(n0 / kTile)) x
// tb in [n0 / kTile, ceil(n_seq / kTile)), row-major; n0: sequences of the first RESIDENT segment; n_first: sequences of the caller's
// first set; `swapped`: the resident first segment holds the caller's SECOND set.  One work-item per (position < n0, position >= n0);
// same-set pairs of straddling tiles are dropped.  d_fs / d_sf (either may be null) are NaN-filled by the caller; *d_status |= 1
// as in launch_unpack.
hipError_t launch_unpack_cross(const float *d_slab, float *d_fs, float *d_sf, const uint32_t *d_order, uint32_t n_seq, uint32_t n0,
                               uint32_t n_first, bool swapped, const uint32_t *d_flags, uint32_t *d_status, hipStream_t stream);
// clustering.hip: the two kernels of apd_cross_linkage.  d_members: member lists sorted ascending per set; d_link: [2][n_first][n_sets]
// workspace (plane 0 fs, plane 1 sf).
hipError_t launch_cross_linkage(const float *d_fs, const float *d_sf, uint32_t n_first, uint32_t n_second, const uint32_t *d_members,
                                const uint32_t *d_set_off, uint32_t n_sets, float *d_link, uint32_t *d_nearest, float *d_nearest_linkage,
                                hipStream_t stream);
// clustering.hip: the two kernels of apd_cluster_medoids.  d_members: sorted ascending per set; d_keys: [n_sets] workspace.
hipError_t launch_cluster_medoids(const float *d_dist, uint32_t n, const uint32_t *d_members, const uint32_t *d_set_off, uint32_t n_sets,
                                  uint32_t n_members, unsigned long long *d_keys, uint32_t *d_medoid, float *d_cost, hipStream_t stream);
// neighbors.hip: panel[s][y] = d[y][column of slot q_first + s] for s < n_slots, y < rows (d: [rows][cols]; d_queries null: slot s is
// column s), 64 x 64 tiles through LDS; `stride` floats from a panel row to the next.  The column forms of apd_neighbors and
// apd_silhouette.  n_slots, rows > 0.
hipError_t launch_column_gather(const float *d, uint32_t rows, uint32_t cols, const uint32_t *d_queries, uint32_t q_first, uint32_t n_slots,
                                float *panel, uint64_t stride, hipStream_t stream);
hipError_t launch_sqrt_sweep(uint32_t first, uint64_t count, unsigned long long *d_out, hipStream_t stream);
// The feature range of the fast kernels: a batch is theirs when every feature is 0 or has kFeatureFloor <= |v| < kFeatureBound;
// any other value (NaN and the infinities included) raises the batch's flag, and the literal kernel aligns every pair.
// Bound: below 2^60 every squared distance and every frame norm is finite (26 * (2 * 2^60)^2 < 2^127), which the fast kernels'
// square roots and norm expansion rely on.
// Floor: the fast distance forms end in the bare v_sqrt_f32, which does not take subnormal inputs (the compiler's sqrtf rescales
// them first), and the hybrid form compares against frame norms (an f64 sum cast to f32) that go subnormal from |v| ~ 2^-63 and
// are 0 from ~ 2^-75.  With every non-zero |v| >= 2^-40 the ulp of a feature is at least 2^-63, so a non-zero component
// difference is a multiple of 2^-63 and a non-zero squared distance at least 2^-126: normal; a non-zero frame norm is at least
// 2^-80.  Exact zeros (silence, padding) contribute nothing to either and stay on the fast kernels.
constexpr float kFeatureFloor = 0x1p-40f;
constexpr float kFeatureBound = 0x1p60f;

// ---- ownership of device memory.  Whatever the library allocates for itself lives in a DeviceBuf: a move-only owner of ONE hipMalloc
// allocation, released by reset() or the destructor -- so an early return (HIP_TRY) between an allocation and its release leaks
// nothing.  Frees are plain hipFree (which waits for the device); the device of the owning context must be bound when one runs.
// Buffers handed to the caller (apd_device_alloc) are not DeviceBufs: they are the caller's to free.
struct DeviceBuf {
    void *ptr = nullptr;
    size_t bytes = 0;
    DeviceBuf() = default;
    DeviceBuf(DeviceBuf &&o) noexcept : ptr(o.ptr), bytes(o.bytes) { o.ptr = nullptr; o.bytes = 0; }   // (no copies: the moves suppress them)
    DeviceBuf &operator=(DeviceBuf &&o) noexcept { std::swap(ptr, o.ptr); std::swap(bytes, o.bytes); return *this; }   // o's destructor frees the old one
    ~DeviceBuf() { reset(); }
    hipError_t reset() { const hipError_t e = ptr ? hipFree(ptr) : hipSuccess; ptr = nullptr; bytes = 0; return e; }
    // a fresh allocation of n bytes (whatever was held is released first)
    hipError_t alloc(size_t n)
    {
        if (hipError_t e = reset(); e != hipSuccess) return e;
        if (hipError_t e = hipMalloc(&ptr, n); e != hipSuccess) { ptr = nullptr; return e; }
        bytes = n;
        return hipSuccess;
    }
    // at least n bytes; grows only, and growth discards the contents
    hipError_t reserve(size_t n) { return ptr && bytes >= n ? hipSuccess : alloc(n); }
    template <class T> T *as() const { return static_cast<T *>(ptr); }
    explicit operator bool() const { return ptr != nullptr; }
};

// ---- objects made on a context that may outlive it (destruction order is the caller's, e.g. a garbage collector's): batches,
// communicators, encoders, cepstrum plans.  While the context lives, it lists them in apd_context::children and the object's
// destroy entry point (destroy_child) releases the device side and takes it off the list.  apd_destroy calls release_device() on
// every child still listed and clears its `ctx`: the later destroy call then only deletes the host part.
struct ContextChild {
    apd_context *ctx = nullptr;
    virtual void release_device() = 0;   // frees device memory / tears the RCCL handle down; host fields stay
    virtual ~ContextChild() = default;
};
int destroy_child(ContextChild *child);   // the shared body of apd_batch_destroy, apd_comm_destroy, ... (apd_api.hip)

// companions.hip: what apd_spot_stream_push_audio needs of an apd_feed.  feed_sizes: the rows a push would add per channel
// (frame_off: n_channels + 1, always written; APD_ERR_INVALID_ARG for descending offsets), host only.  feed_enqueue: that push into
// the feed's own device buffer (*d_rows), enqueued on the context's stream without a synchronisation.
void feed_info(const apd_feed *feed, const apd_context **ctx, uint32_t *n_channels, uint32_t *dim);
int feed_sizes(const apd_feed *feed, const uint64_t *sample_off, uint64_t *frame_off);
int feed_enqueue(apd_context *ctx, apd_feed *feed, const int16_t *samples, const uint64_t *sample_off, int samples_on_device,
                 const uint64_t *frame_off, const float **d_rows);

// companions.hip: an apd_encoder of this context whose weights ([d_in][latent]) and bias ([latent]) are copied from device memory
int encoder_from_device(apd_context *ctx, const float *d_w_encode, const float *d_b_encode, uint32_t d_in, uint32_t latent, apd_encoder **out);

// numerics.rs:125-133 on a device array (clustering.hip): radix select of the k-th smallest non-NaN value, a launch and a read-back
// per digit, for inputs of any size (apd_percentile, apd_clustering).  vat.hip selects per recording inside one workgroup instead.
int device_select(apd_context *ctx, const float *d_x, uint64_t len, uint64_t k, float *value);
uint64_t percentile_index(uint64_t len, float perc);
// The digits both selects (clustering.hip, vat.hip) walk: ascending key order == ascending float order.
__device__ __forceinline__ uint32_t order_key(float v)
{
    const uint32_t u = __builtin_bit_cast(uint32_t, v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// Host-side mirrors of the device band arithmetic (bit-identical f32 product).
inline uint32_t host_band_from_pct(float pct, uint32_t len)
{
    float p = pct * (float)len;                 // discovery.rs:40
    if (!(p > 0.0f)) return 0;                  // NaN / negative saturate to 0 (Rust `as usize`)
    if (p >= 4294967040.0f) return 0xFFFFFFFFu;
    return (uint32_t)p;
}
inline uint32_t host_w(const BandSpec &b, uint32_t n, uint32_t m)
{
    uint32_t mx = n > m ? n : m, gap = n > m ? n - m : m - n;
    uint32_t band = b.use_explicit ? b.explicit_band : host_band_from_pct(b.pct, mx);
    if (band > mx) band = mx;                   // any band >= max(n,m) already covers the full matrix
    return (band > gap ? band : gap) + 2;       // alignments.rs:173
}

// ---- device affinity.  Every entry point binds its context's device to the calling thread through bind_device() before it
// allocates, records an event or launches.  With APD_DEBUG_AFFINITY=1 the library also remembers, per thread, WHICH CONTEXT was
// bound last, and APD_AFFINITY(ctx) -- placed at the allocations, event records and launches inside the library -- fails the call
// unless that context is `ctx` and hipGetDevice() agrees.  Comparing contexts, not device numbers, is what lets the one-GPU
// rehearsals (several "ranks" that all name device 0, tests/test_gpu_multi.py) catch a worker thread that forgot to bind.
extern thread_local const apd_context *tl_bound_context;
bool affinity_debug();
hipError_t bind_device(const apd_context *ctx);
bool affinity_ok(const apd_context *ctx, const char *where);

}  // namespace apd

#define APD_AFFINITY(ctx, where)                                                                   \
    do { if (apd::affinity_debug() && !apd::affinity_ok((ctx), (where))) return APD_ERR_HIP; } while (0)

// A failed HIP call returns from the entry point: APD_ERR_OOM or APD_ERR_HIP, last_error naming the call and HIP's message.
#define HIP_TRY(ctx, call)                                                             \
    do {                                                                               \
        if (hipError_t e_ = (call); e_ != hipSuccess) {                                \
            (ctx)->last_error = std::string(#call) + ": " + hipGetErrorString(e_);     \
            return e_ == hipErrorOutOfMemory ? APD_ERR_OOM : APD_ERR_HIP;              \
        }                                                                              \
    } while (0)

struct apd_context {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    bool timing = false;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // side streams for the launches of different tile classes (independent work, joined back into `stream` with events)
    static constexpr int kSideStreams = 4;
    hipStream_t side[kSideStreams] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t side_done[kSideStreams] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t fork = nullptr;
    // batches, communicators, encoders and cepstrum plans made on this context and not yet destroyed (see apd::ContextChild)
    std::set<apd::ContextChild *> children;
    // buffers handed out by apd_device_alloc and not yet freed: apd_destroy releases them (a host whose destructors run in any
    // order -- a garbage collector's -- may free a buffer after its context: apd_device_free on a destroyed context is never
    // called by the mirrors, and nothing leaks)
    std::set<void *> buffers;
    bool timed = false;
    int variant = 0;
    int distance_mode = 1;            // 0 exact differences, 1 hybrid, 2 strict (bit-identical to the CPU arithmetic)
    float tau = 1.0f / 64.0f;
    std::string last_error;
    // reusable device workspaces, grown through reserve_ws
    apd::DeviceBuf ws_linkage;        // apd_cross_linkage: [members | set_off | link fs, sf], then the host form's staging;
                                      // apd_cluster_medoids: [members | set_off | keys], then the host form's [matrix | medoid | cost]
    apd::DeviceBuf ws_slab;
    apd::DeviceBuf ws_misc;
    apd::DeviceBuf ws_gather;         // gathered slabs of apd_align_all_sharded_async
    apd::DeviceBuf ws_path_dirs;      // apd_align_paths, apd_barycenters: direction words of a chunk of pairs
    apd::DeviceBuf ws_path_steps;     // ... its steps, descriptors and results
    apd::DeviceBuf ws_bary;           // apd_barycenters: the barycenters, their sums and counts, the plan of every chunk
    apd::DeviceBuf ws_spot;           // CurveSweep (apd_host.h): curves, descriptors and results of a chunk of pairs
    apd::DeviceBuf ws_spot_hits;      // apd_spot_detect: the packed hits of a chunk
    apd::DeviceBuf ws_spot_dirs;      // apd_spot_paths: direction words of the intervals of a chunk of windows
    apd::DeviceBuf ws_spot_steps;     // apd_spot_paths, apd_spot_stream_paths: steps, descriptors and results of a chunk of windows
    apd::DeviceBuf ws_neighbors;      // apd_neighbors, apd_silhouette, column form: the [panel][rows] gather of the queried columns (bounded)
    apd::DeviceBuf ws_density;        // apd_density_clusters: the bit planes of a group of settings, their core masks, the changed words (bounded)
    float density_phase_ms[4] = {0.0f, 0.0f, 0.0f, 0.0f};   // ... with timing on: adjacency, degree, propagation, border of the last call
    uint32_t density_rounds = 0;      // ... propagation rounds it enqueued, summed over its groups of settings
    apd::DeviceBuf ws_density_tree;   // apd_density_tree: core keys, components, the words of a round, the edges being sorted (O(n))
    float density_tree_phase_ms[3] = {0.0f, 0.0f, 0.0f};    // ... with timing on: core distances, rounds, final ordering of the last call
    uint32_t density_tree_rounds = 0; // ... Boruvka rounds it ran
    uint32_t *d_status = nullptr;     // sticky device word: bit 0 = an unpack met an unwritten (poisoned) pair score
    uint32_t drop_tiles = 0;          // fault injection (apd_set_fault_injection)
    apd_batch *pair_batch = nullptr;  // apd_align_pair: the last pair's two-sequence batch, refilled while (n, m, dim) repeat
    uint64_t pair_n = 0, pair_m = 0;
    uint32_t pair_dim = 0;
};

// Grows a workspace of the context to `need` bytes (contents are lost when it grows; the hipFree of the old one waits for the device).
inline int reserve_ws(apd_context *ctx, apd::DeviceBuf &ws, size_t need)
{
    APD_AFFINITY(ctx, "workspace allocation");
    HIP_TRY(ctx, ws.reserve(need));
    return APD_OK;
}

struct apd_batch : apd::ContextChild {
    uint32_t n_seq = 0, dim = 0, dpad = 0;   // dim: resident (kernel) frame dimension, >= src_dim
    uint32_t src_dim = 0;                    // the caller's frame dimension
    uint64_t total_frames = 0;
    apd::DeviceBuf d_frames;          // floats: padded layout with sentinels (see dtw_generic.hip)
    uint32_t frames_bytes = 0;
    apd::DeviceBuf d_meta;            // ONE allocation, filled by one copy of h_meta; layout: batch_make_resident (apd_api.hip)
    std::vector<uint32_t> h_meta;     // host image of d_meta, alive as long as the batch (the H2D copy is asynchronous)
    uint32_t *d_seq_off = nullptr;
    uint32_t *d_src_off = nullptr;    // first frame of resident sequence p in the caller's frame array
    uint32_t *d_order = nullptr;      // resident position p -> caller's sequence index
    uint32_t *d_flags = nullptr;      // [0] 1: some frame holds a NaN / infinity (raised by the repack kernel)
    float *d_seq_nmax = nullptr;      // [n_seq] largest squared frame norm per resident sequence (written by the repack kernel)
    mutable int nonfinite = -1;       // host copy of d_flags[0]; -1: not read back yet
    std::vector<uint32_t> order;      // host copy of d_order
    std::vector<uint64_t> offsets;    // frame offsets of the RESIDENT order (host)
    uint32_t min_len = 0, max_len = 0;
    // apd_batch_join: two resident segments, each in its own length order.  first_len: sequences of the caller's first set (n_seq for
    // a plain batch); seg0: sequences of the first resident segment; swapped: that segment holds the caller's SECOND set
    bool joined = false, swapped = false;
    uint32_t first_len = 0, seg0 = 0;
    // device-resident tile lists, grouped by the kernel geometry each tile needs
    struct TilePlan { apd::DeviceBuf d_tiles; std::vector<apd::TileClass> classes; };   // d_tiles: uint4 per tile
    mutable std::map<std::string, TilePlan> tile_cache;   // keyed by tile source/band/variant (tile_plan, apd_api.hip)
    void release_device() override;
};

// ---- what the API units share (defined in apd_api.hip; hidden: not among the exported symbols of libapd_hip.so)
#pragma GCC visibility push(hidden)
int check_lengths(const apd_batch *b);                                   // APD_ERR_EMPTY_SEQUENCE for a batch with an empty sequence
apd::BandSpec band_from_cfg(const apd_align_config *cfg);
apd::BandSpec band_from_params(const apd_alignment_params *params);
// The context's two-sequence batch (ctx->pair_batch) holding (x, y): sequence 0 = x, sequence 1 = y.
int prepare_pair_batch(apd_context *ctx, const float *x, uint64_t n, const float *y, uint64_t m, uint32_t dim);
#pragma GCC visibility pop
