// hq_internal.h -- structs shared by the HIP kernels (the hq_*.hip translation
// units) and the host runtime (hq_runtime.hip).  Not part of the public ABI
// (include/hq.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hq_cost_layout.h"

namespace hq {

constexpr int kMaxK = 256;        // u8 palette indices (K <= 256 on the tiled path)
constexpr int kMaxKWide = 1 << 24;  // K > 256: 32-bit indices (the plugin's limit, HQ:192)
constexpr int kMaxKChunked = 16384;  // 256 < K <= 16384: palettes as 256-colour chunks, 16-bit indices
#ifndef HQ_MAX_NCH_FAST
#define HQ_MAX_NCH_FAST 32
#endif
constexpr int kMaxNchFast = HQ_MAX_NCH_FAST;  // chunked palettes of up to 32 chunks run the tiled cost kernel
// chunks of a palette of K colours on the chunked path: a power of two (2 .. 64)
inline int chunk_count(int K) {
    int n = 1;
    while (256 * n < K) n <<= 1;
    return n;
}
constexpr int kMaxTaps = 255;     // generic path limit (2*half+1)
constexpr int kL1Cap = 31;        // level-1 candidate list capacity (32-B entry)
#ifndef HQ_L2B
#define HQ_L2B 8  // bytes per level-2 entry: 8 (count + 7 indices) or 16 (count + 15)
#endif
constexpr int kL2Bytes = HQ_L2B;
constexpr int kL2Cap = kL2Bytes - 1;  // level-2 candidate list capacity (stored)
constexpr int kL2Build = 15;          // list length build_grid tracks before pruning
constexpr int kL2Line = 4 * kL2Bytes;  // one cell's entries of a group of 4 palettes
constexpr uint8_t kOverflow = 255;

// The 7 separable (vertical, horizontal) filter pairs of the candidate stencil,
// CL:234-306 restated: channel 0 = k1.x (x) k1.x + k2.x (x) k2.x + |k3| (x) k3,
// channel 1 = k1.y (x) k1.y + k2.y (x) k2.y, channel 2 = k1.z (x) k1.z + k2.z (x) k2.z
// (vertical kernel first).  Filter f feeds opponent channel kFiltChan[f].
__host__ __device__ constexpr int filt_chan(int f) { return f < 3 ? 0 : (f < 5 ? 1 : 2); }

template <int T>
struct TapTable {
    float v[kNumFilt][T];  // vertical taps per filter
    float h[kNumFilt][T];  // horizontal taps per filter
};

// Geometry of one (possibly sharded) image on a device.
struct Geom {
    int W, H;        // full image
    int r0, r1;      // owned rows [r0, r1)
    int e0, e1;      // extended rows held on device [e0, e1) (owned +- half, clipped)
    int lab_pitch;   // floats per row of the planar LabRef (multiple of 4)
    int64_t n_ext;   // W * (e1 - e0)
    int64_t idx_pitch;  // bytes per palette in the index buffer (>= n_ext, multiple of 256)
};

struct PaletteArgs {
    const float4* pal_in;   // [P][K] host-uploaded palettes
    float4* pal;            // [P][256] sanitised colours (.w = 0)
    float4* opp;            // [P][256] opponent colour of each palette entry (CL:194-198)
    uint4* opp16;           // [P][256] its channels x 2^14 as (hi, lo) f16 pairs (split_f16), .w = 0
    uint8_t* dup;           // [P][256] 1 if an identical colour exists at a lower index
    int* pflags;            // [P] bit0: non-finite colour present -> exhaustive argmin
    int K;
    // option "assign_space": the table the argmin kernels read, [P][256] (.w = 0).  space 0:
    // arg == pal, nothing more is stored.  space 1: each colour's CIELAB coordinates
    // (assign_coord_lab under inv_illum); a coordinate that is not finite sets pflags too
    float4* arg;
    int space;
    float inv_illum[3];
};

// coords_kernel (hq_argspace.hip): the argmin coordinates of the extended rows' pixels,
// from the packed bytes (rgbx) or, rgbx null, the planar floats, into three planes of the
// same length and padding (quads: their floats / 4; the padding reads as zero).
struct CoordArgs {
    const uint32_t* rgbx;
    const float* R;
    const float* G;
    const float* B;
    float* oR;
    float* oG;
    float* oB;
    int64_t n_ext, quads;
    float inv_illum[3];
};

constexpr int kSaMaxP = 64;        // device-resident SWASA: largest population
constexpr int kSaMaxSub = 512;     // ... and sub-palettes (P nch; sa_step's fold: 8 P nch used words <= 4 x 1024)
// Used-colour bits are kept in kUsedSlots copies, used_stride(P) words apart
// (256-B multiples): assign's workgroups OR theirs into copy blockIdx & 7, the
// readers OR the copies.  One copy took every workgroup's atomic at the end of
// the launch (C2, P = 1: 2048 workgroups on one 32-B word set, +14 us).
constexpr int kUsedSlots = 8;
// words per used-bit copy: P palettes x 8 words, rounded up to 64 words (256 B)
inline int used_stride(int P) { return (P * 8 + 63) / 64 * 64; }
// fixed-point dE sums (hq_device.h acc_add): slot counters per palette, and two
// sets used alternately by consecutive evaluations (a set is zeroed by the
// kernel before the evaluation's cost kernel, while the previous set is read)
constexpr int kAccSlots = 16;
// palettes per slot row, a multiple of 8: each slot's counters start a 256-B
// row of their own, so the slots' atomics spread over the memory channels
// rather than queueing on one (P = 1: sixteen 32-B slots shared 512 B)
__host__ __device__ constexpr int acc_pitch(int P) { return (P + 7) & ~7; }
inline size_t acc_words(int P) { return (size_t)kAccSlots * acc_pitch(P) * 4; }

// sa_step_kernel: one accept + generate step of the device-resident SWASA search.
struct SaArgs {
    const double* out;      // [P][1+K] finalize sums + used flags of the last evaluation
    const float* colors_in; // [P][4K] accepted palettes (ping)
    float* colors_out;      // (pong)
    const float* cand_in;   // [P][4K] candidates just evaluated
    float* cand_out;        // [P][4K] next candidates (generate)
    const double* err_in;   // [P] current errors
    double* err_out;
    const uint64_t* seed_in;  // java.util.Random state
    uint64_t* seed_out;
    const double* best_err_in;  // best error so far (ping-ponged like the state: the
    double* best_err_out;       // writer updates it while other workgroups read it)
    float* best_colors;     // [4K]
    const uint64_t* jump_A; // LCG jumps: n steps = A_n s + C_n mod 2^48, n = 0 .. 3K*P
    const uint64_t* jump_C;
    PaletteArgs prep;       // outputs of the palette prep of the next candidates
    // fold (no communicator, or a row-block split): the accept step reads the
    // fixed-point sums and the used bits itself, so no finalize launch sits
    // between the cost kernel and this step.  Row-block ranks: nranks blocks,
    // each rank's own, gathered by one RCCL all-gather (integer sums and OR'ed
    // bits: the same totals in any rank order).
    const uint64_t* acc;    // [nranks][kAccSlots][P][4] (acc_total), acc_rank_words apart
    const uint32_t* used_glob;  // [nranks][kUsedSlots][used_stride]: [P][8 nch] per slot
    int used_stride;
    int fold;
    int nranks;             // rank blocks of acc and used_glob (1 without a communicator)
    int64_t acc_rank_words;
    double n_total;         // pixels of the whole image
    double keep_threshold;  // SW:59-62 -(tanh(num/den))/2 + 0.5 at the accepted iteration
    float temperature;      // SW:54-57 temperature at the accepted iteration
    float amax;             // SW:91-101 max_step_width(ite) / 256 for the generated iteration
    float delta;            // SW:74-82 penalty per unused colour
    int P, K;
    int accept;             // 1: accept the evaluated population first
    int init;               // accept as IM:490-493 (initial population) instead
    int generate;           // 1: generate the next candidates (and prep them)
    int random;             // generate SW:40-52 random colours instead of neighbours
    int convergence;
    int nch;                // chunked palettes: chunks per palette (P nch workgroups), else 1
    int nfixed;             // fixed colours (hq_set_fixed_colors): candidate colour k < nfixed is the
                            // member's colour k, its draws discarded (0: none; 0 in a random step)
};

struct GridArgs {
    const float4* pal;
    const uint8_t* dup;
    const int* pflags;
    uint8_t* lvl1;          // [P][G1^3][32]
    uint8_t* lvl2;          // [ceil(P/4)][G2^3][4][kL2Bytes]: a group's 4 entries of a cell side by side
    uint32_t* used_glob;    // [kUsedSlots][used_stride] used-colour bits, zeroed here for the assign
    int used_stride;        // that follows
    int K;
    int G1;                 // level-1 resolution (G2 / 4)
    int64_t lvl1_pitch;     // bytes per palette
    int64_t lvl2_gstride;   // bytes per group of 4 palettes (G2^3 * kL2Line)
    uint64_t* acc_zero;     // the fixed-point sums the following cost kernel adds to, zeroed here
    int P_acc;              // their palettes (P above / nch)
    int nch;                // sub-palettes per palette (chunked palettes), else 1
};

// Native 16-bit candidate lists (hq_lists16.hip) for chunked palettes of 4 to
// 32 chunks (512 < K <= 8192): one grid over all K colours, level 1 at 16^3
// cells (u16 count + 127 or 255 indices), level 2 at 64^3 (u16 count + 15
// indices, 32 B); count kN16Ovf = overflow.
constexpr int kN16G2 = 64, kN16G1 = kN16G2 / 4, kN16G0 = kN16G1 / 4;
// Level-1 entries: 128 u16 (count + 127) up to K = 4096, 256 above (lists at
// K = 8192: mean ~66, a tail past 127); the buffer is sized for the larger.
constexpr int kN16L2Cap = 15, kN16L2Words = kN16L2Cap + 1;  // u16 per entry
constexpr int kN16L1WordsMax = 256;
__host__ __device__ constexpr int n16_l1_words(int K) { return K > 4096 ? 256 : 128; }
constexpr uint16_t kN16Ovf = 0xffff;
constexpr int kN16MinNch = 4;   // chunk counts that take the native lists (option "lists16") ...
constexpr int kN16MaxNch = 32;  // ... up to K = 8192: the palette's 128 KiB table in assign16's LDS
constexpr int kN16MaxK = 256 * kN16MaxNch;

struct Lists16Args {
    const float4* pal;      // [P][kpal] colours (the prepared sub-palettes, contiguous per palette)
    const int* pflags;      // [P nch] sub-palette flags (non-finite colour: exhaustive)
    uint16_t* lvl1;         // [P][16^3][n16_l1_words(K)]
    uint16_t* lvl2;         // [P][64^3][kN16L2Words]
    uint32_t* used_glob;    // [kUsedSlots][used_stride]: [P][8 nch] used-colour bits, zeroed here
    int used_stride;
    uint64_t* acc_zero;     // the fixed-point sums of the cost kernel that follows, zeroed here
    int P_acc;
    int K, kpal, nch;
};

struct AssignArgs {
    const float* R;         // planar, n_ext floats (extended rows)
    const float* G;
    const float* B;
    const uint32_t* rgbx;   // packed 8-bit R,G,B (byte 0..2) of an image whose channels are all
                            // k/255 (exactly, IM:100's int-RGB source), else null
    const float4* pal;      // [P][256]
    const int* pflags;
    const uint8_t* lvl1;
    const uint8_t* lvl2;
    uint8_t* idx;           // [P][idx_pitch]
    uint32_t* used_glob;    // [kUsedSlots][used_stride]: [P][8] used-colour bits per slot, every
    int used_stride;        // workgroup ORs its own into slot blockIdx & 7 (atomics)
    int64_t n_ext;
    int64_t idx_pitch;
    int64_t lvl1_pitch;     // bytes per palette
    int64_t lvl2_gstride;   // bytes per group of 4 palettes (G2^3 * kL2Line)
    int K;
    int G2;                 // 0 = exhaustive
    int nblocks;            // workgroups per palette group
    // chunked palettes (256 < K <= 4096): the P above are sub-palettes, nch per
    // palette (chunk_count), combined into 16-bit indices (hq_assign.hip)
    uint16_t* idx16;        // [P / nch][idx_pitch]
    float* dist;            // [P / nch][idx_pitch] best reference distance (nch > 4 passes)
    int nch = 1, lg_nch = 0;
    int gstep = 1;          // (set by the launcher)
    // native 16-bit lists (hq_lists16.hip): palette p's colours at pal + p kpal
    const uint16_t* l1n = nullptr;
    const uint16_t* l2n = nullptr;
    int kpal = 0;
    // ordered dithering (hq_ordered_population; launch_assign_ordered): the argmin sees
    // min(max(pix_c + amp[c] * map[(y & mh_mask) << lg_mw | (x & mw_mask)], 0), 1), (x, y) the
    // pixel's position in the FULL image.  nch = 1 only.
    const float* map = nullptr;  // [mh][mw], mw and mh powers of two up to kMaxMapSide
    uint32_t mw_mask = 0, mh_mask = 0, lg_mw = 0;
    float amp[3] = {0.f, 0.f, 0.f};
    uint32_t W = 1;         // the image's width
    uint32_t y0 = 0;        // the full-image row of extended row 0 (Geom::e0)
    uint32_t dx = 0, dy = 0;  // nblocks * 256 = dy W + dx, dx < W (set by the launcher)
};
constexpr int kMaxMapSide = 64;  // threshold maps: up to 64 x 64 (hq_set_dither_map)

struct CostArgs {
    const uint8_t* idx;     // [P][idx_pitch]
    const uint4* opp16;     // [P][256] split opponent table (PaletteArgs::opp16)
    const void* taps;       // CostTaps<10> x 2 in device memory (build_fast_taps)
    const uint4* vfrag16;   // [trim][4 stacks][hi, lo][64 lanes] f16x8 A fragments of the
                            // vertical taps (build_vpass_f16_stack_fragments; cost_mfma)
    const uint4* vfrag16p;  // [trim][u][4 stacks][hi, lo][64 lanes]: the same taps in the (hi, lo)
                            // pair layout of cost16w (build_vpass_f16_pair_fragments)
    const float* labL;      // planar LabRef, owned rows, pitch lab_pitch
    const float* labA;
    const float* labB;
    uint64_t* acc;          // fixed-point dE sums [kAccSlots][acc_P][4] (acc_add); this launch's
    int acc_P, acc_p0;      // palettes are acc_p0 .. (a group of a larger population: acc_p0 > 0)
    Geom g;
    int K;
    int tiles_x;
    int ntiles;      // tiles of the shard (partial pitch per palette)
    float m_lab[9];  // Opp->XYZ rows / illuminant (CL:124-131), opp2xyz_over_illum()
    float* pix_err;  // test option "pixel_err": [P][pix_pitch] per-pixel dE of the owned rows
    int64_t pix_pitch;  // (null: not written)
    // pixel mask (hq_set_mask; read by the masked instances only, hq_cost_masked.hip): a byte per
    // owned pixel at the LabRef planes' pitch, (y - r0) lab_pitch + x, non-zero = the pixel counts.
    // Pixel weights (hq_set_weights; the weighted instances, hq_cost_weighted.hip) use the same
    // three fields: the byte is the pixel's weight, 0 = the pixel is left out
    const uint8_t* mask;
    const int32_t* live;    // their work items' tiles: item w is palette w % P over tile live[w / P]
    int nlive;              // entries of live (the launch covers nlive P items)
};

struct FinalizeArgs {
    const uint64_t* acc;    // fixed-point dE sums [kAccSlots][P][4]
    const uint32_t* used_glob;  // [kUsedSlots][used_stride] used-colour bits (assign)
    int used_stride;
    double* out;            // [P][1+K]
    int P;
    int K;
    const uint32_t* used32; // K > 4096: [P][K] used flags (assign_wide), replaces used_mask
    int wpp;                // used words per palette in used_glob (8; 8 nch for chunked palettes)
};

// Palettes of K > 256 colours (hq_wide.hip).
struct WideArgs {
    const float4* pal_in;   // [P][K] host-uploaded palettes
    float4* pal;            // [P][K] .w = 0
    float4* opp;            // [P][K] opponent colours (CL:194-198)
    int* pflags;            // [P] bit 0: non-finite colour (zeroed before prep)
    const float* R;         // planar extended rows
    const float* G;
    const float* B;
    uint32_t* idx32;        // [P][idx_pitch] 32-bit palette indices
    uint32_t* used32;       // [P][K] used flags (zeroed before assign)
    int64_t n_ext;
    int64_t idx_pitch;      // elements per palette
    int K;
};

// Per-colour pixel sums of the last evaluated population (hq_centroid.hip): the
// k-means half the argmin leaves open.  A workgroup covers at most
// cent_max_span pixels, which bounds its LDS accumulators (the bound is worked
// out there).
constexpr int kCentLdsK = kMaxK;          // K up to here (the u8 index images): accumulators in LDS;
                                          // above: global atomics straight away
constexpr int kCentBlocksPerCu = 4;       // workgroups per CU over all palette groups
// pixels per workgroup, at most: the packed form (32-bit fields of byte sums), the planar form
// (a 16-bit count above a 48-bit sum of values up to 2^32).  Under pixel weights (a pixel adds
// up to 255 times as much): the packed form's 32-bit fields hold 2^16 pixels of 255 255; the
// planar form has four whole 64-bit words per colour, 2^22 pixels of 255 2^32 < 2^40 each.
__host__ __device__ constexpr uint32_t cent_max_span(bool u8, bool weighted = false) {
    return weighted ? (u8 ? 1u << 16 : 1u << 22) : (u8 ? 1u << 22 : 1u << 15);
}
struct ClusterArgs {
    const void* idx;        // [P][idx_pitch] index images over the extended rows: u8, u16 or u32
    const float* R;         // planar, extended rows (padded to a multiple of 4 floats)
    const float* G;
    const float* B;
    const uint32_t* rgbx;   // packed 8-bit R,G,B (AssignArgs::rgbx), else null
    unsigned long long* sums;  // [P][K][4] sum R, sum G, sum B, count (zeroed before the launch)
    int* bad;               // planar form: set to 1 by an owned pixel that is not in [0, 1]
    int64_t idx_pitch;      // elements per palette
    uint32_t q0, q1;        // the owned rows: positions [q0, q1) of the extended rows
    int P, K;
    int nblocks;            // workgroups per group of 4 palettes   } set by the
    uint32_t qspan;         // quads of 4 pixels per workgroup      } launcher
    // pixel mask (hq_set_mask): a byte per position of the extended rows (padded to whole quads),
    // non-zero = the pixel is added; null: every owned pixel.  The range flag looks at every owned
    // pixel either way.
    const uint8_t* mask = nullptr;
    // pixel weights (hq_set_weights): mask holds the weights, and a pixel adds weight times its
    // channels and its weight to the count
    int weighted = 0;
    // test option "cent_span": pixels per workgroup (0: by the grid), clamped to cent_max_span
    uint32_t span = 0;
};

// Per-colour error statistics of the last evaluated population (hq_errsum.hip,
// hq_cluster_errors): ClusterArgs' view of the index images and the pixels, plus
// the error image the cost kernels stored and the prepared palettes.
struct ClusterErrArgs {
    const void* idx;        // [P][idx_pitch] index images over the extended rows: u8, u16 or u32
    const float* R;         // planar, extended rows (padded to a multiple of 4 floats)
    const float* G;
    const float* B;
    const uint32_t* rgbx;   // packed 8-bit R,G,B when the argmin read it, else null
    const float* pix_err;   // [P][err_pitch] per-pixel dE of the owned rows (CostArgs::pix_err)
    const float4* pal;      // [P][pal_pitch] the prepared palettes (.w = 0)
    unsigned long long* stats;  // [P][K][4] sum of RN(e 2^20), count, key of the worst movable pixel
                                // ((bits of e) << 32 | 2^32 - 1 - position; 0: none), 0 (zeroed before the launch)
    float4* worst;          // [P][K] (R, G, B, 0) of that pixel, zeros without one
    int* bad;               // set to 1 by an owned pixel whose dE is not a finite number in [0, 2^20)
    int64_t idx_pitch;      // elements per palette
    int64_t err_pitch;
    int64_t pal_pitch;
    uint32_t q0, q1;        // the owned rows: positions [q0, q1) of the extended rows
    uint32_t pos0;          // position y w + x in the full image of extended position 0
    int P, K;
    int nblocks;            // workgroups per group of 4 palettes   } set by the
    uint32_t qspan;         // quads of 4 pixels per workgroup      } launcher
};

// Colour histogram of the owned rows (hq_hist.hip, hq_color_histogram): per cell
// of a 2^bits grid per channel the sum of its pixels and their count, in the
// units of ClusterArgs::sums.
constexpr int kHistBlocksPerCu = 8;       // workgroups per CU: one resident round
struct HistArgs {
    const float* R;         // planar, extended rows (padded to a multiple of 4 floats)
    const float* G;
    const float* B;
    const uint32_t* rgbx;   // packed 8-bit R,G,B (AssignArgs::rgbx), else null
    unsigned long long* cells;  // [2^(3 bits)][4] sum R, sum G, sum B, count (zeroed before the launch)
    int* bad;               // planar form: set to 1 by an owned pixel that is not in [0, 1]
    uint32_t q0, q1;        // the owned rows: positions [q0, q1) of the extended rows
    int bits;               // 2 .. 6
    int nblocks;            // workgroups                           } set by the
    uint32_t qspan;         // quads of 4 pixels per workgroup      } launcher
    const uint8_t* mask = nullptr;  // pixel mask (ClusterArgs::mask), or null
    int weighted = 0;               // pixel weights (ClusterArgs::weighted)
};

// lloyd_update_kernel (hq_search.hip): the k-means move of a device-resident
// hybrid iteration.  Candidate colour k of palette p with count > 0 becomes the
// mean of its pixels (lloyd_mean, hq_lloyd.h), in place; the palette is
// prepared again (prep's outputs) and the sums it read are zeroed for the next
// hybrid iteration.
struct LloydArgs {
    unsigned long long* sums;  // [P][K][4] ClusterArgs::sums of the assign-only pass
    float* cand;               // [P][4K] the search's candidates (the next sa_step's cand_in)
    PaletteArgs prep;          // outputs of the palette prep of the updated candidates
    int K;
    int bytes;                 // sums in units of 1/255 (the packed image), else 2^-32
    int nfixed;                // fixed colours: colour k < nfixed keeps its bits whatever its count
};

// reseed_kernel (hq_search.hip): the repair move of a device-resident repair
// iteration, hq_reseed_unused's rule on the device.  Unused candidate colours of
// palette p become worst pixels of the clusters with the most error, in place;
// the palette is prepared again (prep's outputs) and the statistics it read are
// zeroed for the next repair iteration.
struct ReseedArgs {
    unsigned long long* stats;  // [P][K][4] ClusterErrArgs::stats of the error pass
    const float4* worst;       // [P][K] ClusterErrArgs::worst
    float* cand;               // [P][4K] the search's candidates (the next sa_step's cand_in)
    PaletteArgs prep;          // outputs of the palette prep of the repaired candidates
    int K;
    int max_moves;             // colours moved per palette at most (< 0: no limit)
    int nfixed;                // fixed colours (hq_reseed_unused_fixed): colour k < nfixed is no receiver
};

// Generic two-pass path (any half-width), one palette per launch.
struct GenArgs {
    const void* idx;         // palette's index image (extended rows): u8, or u32 for K > 256
    const float4* opp;       // palette's opponent table [max(K, 256)]
    const float* k1;         // [T][4]
    const float* k2;         // [T][4]
    const float* k3;         // [T]
    const float* absk3;      // [T]
    float* t;                // [7][n_ext] horizontal results (t1.xyz, t2.xyz, t3)
    const float* labL;
    const float* labA;
    const float* labB;
    uint64_t* acc;           // fixed-point dE sums [kAccSlots][P][4] (acc_add), palette p
    int p, P;
    Geom g;
    int half;
    float m_lab[9];  // Opp->XYZ rows / illuminant (CL:124-131), opp2xyz_over_illum()
    float* pix_err;  // this palette's per-pixel dE of the owned rows (test option), or null
    const float* vtaps;  // tiled path: [7][vtap_pitch] vertical taps per plane, zero-padded
    int vtap_pitch;      // (2 half + 1 rounded up to 16, + 16)
    int hrow4 = 1;       // tiled path: horizontal pass with 4 outputs per thread (gen_hrow4), else gen_hrow
    int hrow_no = 4;     // gen_hrow4's outputs per thread: 4 or 8
    int vtile2 = 1;      // tiled path: double-buffered LDS-DMA vertical pass (gen_vtile2), else gen_vtile
    int vmfma = 1;       // tiled path: the vertical pass on the matrix cores (gen_vmfma, split f16)
    const uint32_t* vtapd = nullptr;  // its duplicated split taps [7][hi, lo][16 S + 16] (build_vtile_dup_taps)
    int hmfma = 1;       // with vmfma: the horizontal pass on the matrix cores too (gen_hmfma)
    int shape = 0;       // matrix-core pair's tile shapes: 0 by grid size, 1 the short forms, 2 the tall ones
    const uint32_t* htapd = nullptr;  // its taps, the same layout (k3 signed: the horizontal t3 taps)
    const float4* htaps = nullptr;  // gen_hrow4: [T][2] (k1.xyz, k3), (k2.xyz, 0) horizontal taps
    // pixel mask or pixel weights (CostArgs::mask's layout): a pixel's dE times its byte, as
    // doubles (a mask's bytes are 0 / 1), a zero byte a select; null: every owned pixel counts
    const uint8_t* mask = nullptr;
};

// reduce_u8_kernel / reduce_planar_kernel (hq_reduce.hip): the box reduction of a whole
// image by an integer factor (hq_set_image_reduced), one context's image into another's
// planes.  Output pixel (X, Y) is the mean of source columns [f X, min(f X + f, W)) and
// the rows likewise.
struct ReduceArgs {
    const uint32_t* rgbx;  // the packed form: the source's 8-bit copy [H][W] (R | G << 8 | B << 16), or null
    const float* R;        // the planar form: the source's planes [H][W]
    const float* G;
    const float* B;
    float* oR;             // the reduced planes [rh][rw]
    float* oG;
    float* oB;
    int W, H;              // the source image
    int rw, rh;            // the reduced image: ceil(W / f), ceil(H / f)
    int factor;            // f in 1 .. kMaxReduce
};
constexpr int kMaxReduce = 16;

}  // namespace hq
