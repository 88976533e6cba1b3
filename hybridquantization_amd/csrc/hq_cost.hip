// hq_cost.hip -- the S-CIELAB stencil cost of a population (CL:234-306,
// vertical pass first), Opp->Lab (CL:124-145) and dE (CL:201-226) against the
// precomputed LabRef, one fp64 partial per (tile, palette): the fast path for
// half-widths up to 24.  Longer filters: hq_cost_generic.hip; the host-built
// tap tables and MFMA fragments of both: hq_cost_taps.cpp.
#include "hq_device.h"
#include "hq_launch.h"

#ifndef HQ_CHW
#define HQ_CHW 8  // horizontal taps per chunk at HB = 15, 24
#endif
#ifndef HQ_CH19
#define HQ_CH19 6  // horizontal taps per chunk at HB = 19 (6, 8, 13: equal since the pair layout; with the
                   // 32-row layout 8 spilled 40 B per lane at 3 waves/SIMD, 6 spilled 12)
#endif

namespace hq {

// ----------------------------------------------------------------------------
// Fast path (HALF = 10, the 21-tap filters of the default viewing set): a 1-D
// grid of (output tile, palette) work items.  One workgroup = one TW x TH output
// tile; its region = (TH + 2*HALF) rows x RW columns of palette indices.
// Vertical pass first on all RW region columns (separable filters commute),
// then the horizontal pass on the TW output columns, Opp->Lab, dE, fp64 partial.
// ----------------------------------------------------------------------------
// Tile geometry of the fast path: 8 x 108 output tiles of a 28 x 128 region
// (cost_mfma_kernel) or 16 x 128 tiles of a 36 x 148 region (cost16w_kernel).
constexpr int kFastHalf = 10, kFastRW = 128;
constexpr int kFastTW = kFastRW - 2 * kFastHalf;

// Taps are read through a constant-address-space pointer into device memory
// (uniform s_load per filter; build_fast_taps holds both scalings).
template <int HALF>
using TapsPtr = const __attribute__((address_space(4))) CostTaps<HALF>*;

// TRIM: the narrow k1.x / k1.y / k1.z filters (f = 0, 3, 5) run over their
// significant-tap windows kTrimLo..kTrimHi only (|taps| outside are below 1e-9
// of the filter's peak for the default filter set; see trim_window_ok()).
// Per-filter loops keep one filter's 21 taps live in SGPRs (interleaving a
// channel's filters needs 63 and spills to VGPR lanes).
constexpr int kTrimLo[3] = {kFastHalf - trim_w(kFastHalf, 0), kFastHalf - trim_w(kFastHalf, 1),
                            kFastHalf - trim_w(kFastHalf, 2)};
constexpr int kTrimHi[3] = {kFastHalf + trim_w(kFastHalf, 0), kFastHalf + trim_w(kFastHalf, 1),
                            kFastHalf + trim_w(kFastHalf, 2)};

// ---- vertical pass on the matrix cores --------------------------------------
// The vertical pass of a filter over a 16-column block is a banded-Toeplitz
// product with the block's TH + 2*HALF gathered input rows: one
// v_mfma_f32_16x16x32_f16 K step (rows past the region zero-weighted).  fp32
// accuracy from f16 operands: x = hi + lo (both f16, x scaled by 2^14 so lo
// stays normal down to |x| ~ 1e-5) and the products hi.hi + hi.lo + lo.hi (each
// exact in the f32 accumulator; the dropped lo.lo is ~2^-22 relative).  Taps
// are split the same way on the host, scaled by 2^16
// (build_vpass_f16_stack_fragments); the 2^30 total scale is folded into the
// horizontal taps, exactly (a power of two): kVTapScale, kVOutScale and the K
// slot maps kv_row / kv_row_s the host shares are in hq_cost_layout.h.


// One work item of the cost pass: palette p over output tile `tile`.
struct TileItem {
    int p, tile, x0, y0;
};

// MSK (the masked instances, hq_cost_masked.hip): the tile through the live-tile
// list of the launch (CostArgs::live), which covers nlive P items.  MSK is 0 (the plain
// instances), 1 (a pixel mask) or 2 (pixel weights, hq_cost_weighted.hip: the mask bytes are the
// pixels' weights, the live tiles those with a non-zero one).
template <int TW, int TH, int MSK = 0>
__device__ __forceinline__ TileItem tile_item(const CostArgs& a, int w, int P) {
    TileItem t;
    t.p = w % P;
    if constexpr (MSK != 0) t.tile = a.live[w / P];
    else t.tile = w / P;
    t.x0 = (t.tile % a.tiles_x) * TW;
    t.y0 = a.g.r0 + (t.tile / a.tiles_x) * TH;
    return t;
}

// dE2000: a shard's tile rows lie on the full image's tile grid.  The first
// one starts at fast_grid_row0 <= r0, and the kernels' `if constexpr (DE == 2)`
// statements mask its rows above r0.  So a pixel sits at the same row of its
// tile, its taps at the same K slots of the vertical pass, in every sharding:
// the shards' per-pixel dE are the full image's bit for bit, at the price of
// up to one extra, partly masked tile row per shard.  dE76 and dE94 keep their
// tiles from r0, and their kernels the parent's statements token for token
// (a shared helper that folds to `true` for them still moved their registers).
template <int DE, int TW, int TH>
__device__ __forceinline__ void tile_item_to_grid(const CostArgs& a, TileItem& t) {
    static_assert((TH & (TH - 1)) == 0, "fast_grid_row0 masks with TH - 1");
    if constexpr (DE == 2) t.y0 -= a.g.r0 & (TH - 1);
}

// The global loads that fill one item's LDS (index rows of its region, its
// palette's opponent entry), held in registers between issue and commit.
// Every load is issued before the first wait: vmcnt retires in order, so a
// load -> wait -> store loop pays one memory round trip per trip (4 for the
// interior index rows, 14 for the byte gathers of edge tiles).
// Interior rows are read as DW = RW / 4 dword pairs: the first DM = NTH / 8
// dword columns by a (row, column) = (tid / DM + 8q, tid % DM) map (shifts and
// masks, row offsets one multiply-add), the DW - DM tail columns (cost16w's
// 148-byte rows: 5 of 37; the 276-byte rows of 256-column tiles: 5 of 69) by a
// second, short pass.  NTH = threads of the workgroup.
template <int HALF, int RW, int TH, int NTH = 256>
struct TileFill {
    static constexpr int TW = RW - 2 * HALF, RH = TH + 2 * HALF, DW = RW / 4, DM = NTH / 8;
    static constexpr int DWT = DW - DM;                                   // tail dword columns
    static constexpr int DWTD = DWT > 0 ? DWT : 1;                        // its divisor (no tail: unused)
    static constexpr int NM = (RH * DM + NTH - 1) / NTH, NT = (RH * DWT + NTH - 1) / NTH;
    static constexpr int NFD = NM + NT, NFB = (RH * RW + NTH - 1) / NTH;
    static_assert(RW % 4 == 0 && DW >= DM && DWT < DM, "whole dwords per region row, DM <= DW < 2 DM");
    uint32_t lo[NFD], hi[NFD];  // interior tiles: aligned dword pairs of the index rows
    uint32_t roff[NFD];         // their rows' byte offsets (alignment for commit)
    uint4 ov;  // the palette's split opponent entry tid (zeros past K)
    TileItem t;
    bool interior;

    // Byte offset of region row i in the palette's index image (reflection at the
    // image edges, clamped to the rows held on this device).
    __device__ __forceinline__ static int row_base(const Geom& g, const TileItem& t, int i) {
        int gy = reflect_clamp(t.y0 - HALF + i, g.H);
        gy = min(max(gy, g.e0), g.e1 - 1);
        return (gy - g.e0) * g.W + (t.x0 - HALF);
    }

    // Issue the loads; interior tiles only (edge tiles -- the image's first and
    // last tile columns -- gather bytes with reflection at commit time).  Tiles
    // whose halo rows need neither reflection nor clamping (all but the image's
    // and the shard's first and last tile rows) take row offsets from one
    // multiply-add.  Loads are unconditional (rows clamped into the region) and
    // use 32-bit unsigned offsets from the palette's base (saddr form); the host
    // keeps a shard's index image below 2^31 bytes.
    __device__ __forceinline__ void issue(const CostArgs& a, const TileItem& ti, int tid) {
        static_assert(kMaxK <= NTH, "one opponent-table entry per thread");
        const Geom& g = a.g;
        t = ti;
        const uint8_t* idx = a.idx + (int64_t)t.p * g.idx_pitch;
#ifdef HQ_ABL_NOFILL  // timing ablation (wrong results): no global loads for the fill
        ov = make_uint4(tid, tid + 1, tid + 2, 0u);
        interior = true;
#pragma unroll
        for (int q = 0; q < NFD; ++q) lo[q] = hi[q] = roff[q] = (uint32_t)(tid * 7 + q);
        return;
#endif
        ov = tid < a.K ? a.opp16[(int64_t)t.p * kMaxK + tid] : make_uint4(0u, 0u, 0u, 0u);
        interior = t.x0 - HALF >= 0 && t.x0 + TW + HALF <= g.W;
        if (interior) {
            const int ytop = t.y0 - HALF;
            const bool vfast = ytop >= 0 && ytop >= g.e0 && ytop + RH <= g.H && ytop + RH <= g.e1;
            const int ubase = (ytop - g.e0) * g.W + (t.x0 - HALF);
            auto load = [&](int q, int i, int c) {
                roff[q] = (uint32_t)(vfast ? ubase + i * g.W : row_base(g, t, i));
                const uint32_t* src =
                    reinterpret_cast<const uint32_t*>(idx + ((roff[q] & ~3u) + 4u * (uint32_t)c));
                lo[q] = src[0];
                hi[q] = src[1];
            };
#pragma unroll
            for (int q = 0; q < NM; ++q) load(q, min(tid / DM + 8 * q, RH - 1), tid % DM);
#pragma unroll
            for (int q = 0; q < NT; ++q) {
                const int e = min(tid + NTH * q, RH * DWT - 1);
                load(NM + q, e / DWTD, DM + e % DWTD);
            }
        }
    }

    // index rows into s_idx (row pitch IDXP bytes); the first write waits for the loads
    template <int IDXP>
    __device__ __forceinline__ void commit_idx(const CostArgs& a, uint8_t* s_idx, int tid) const {
        const Geom& g = a.g;
        if (interior) {
            uint32_t* s32 = reinterpret_cast<uint32_t*>(s_idx);
#pragma unroll
            for (int q = 0; q < NM; ++q) {
                const int i = tid / DM + 8 * q;
                if (i < RH)
                    s32[i * (IDXP / 4) + tid % DM] = __builtin_amdgcn_alignbyte(hi[q], lo[q], roff[q] & 3u);
            }
#pragma unroll
            for (int q = 0; q < NT; ++q) {
                const int e = tid + NTH * q;
                if (e < RH * DWT)
                    s32[(e / DWTD) * (IDXP / 4) + DM + e % DWTD] =
                        __builtin_amdgcn_alignbyte(hi[NM + q], lo[NM + q], roff[NM + q] & 3u);
            }
        } else {
            const uint8_t* idx = a.idx + (int64_t)t.p * g.idx_pitch;
            uint32_t b[NFB];
#pragma unroll
            for (int q = 0; q < NFB; ++q) {  // all loads first: one round trip
                const int e = min(tid + NTH * q, RH * RW - 1);
                const int i = e / RW, j = e % RW;
                int gy = reflect_clamp(t.y0 - HALF + i, g.H);
                gy = min(max(gy, g.e0), g.e1 - 1);
                const int gx = reflect_clamp(t.x0 - HALF + j, g.W);
                b[q] = idx[(uint32_t)((gy - g.e0) * g.W + gx)];
            }
#pragma unroll
            for (int q = 0; q < NFB; ++q) {
                const int e = tid + NTH * q;
                if (e < RH * RW) s_idx[(e / RW) * IDXP + e % RW] = (uint8_t)b[q];
            }
        }
    }
};

// The 16-bit index rows of a chunked palette's tile (256 < K <= 4096): region
// row i = RWL indices from column x0 - HALF into s_idx row i (pitch RW
// elements; columns RWL .. RW - 1, read by the vertical pass's last block but
// never used, are zeroed so they index the table).  Tiles whose rows all start
// on a dword (interior tiles of an even-width image at an even HALF) load
// dwords of two indices; the others gather element by element with reflection.
template <int HALF, int RWL, int RW, int TH, int NTH = 256>
struct TileFill16 {
    static constexpr int RH = TH + 2 * HALF, DW = RWL / 2, NL = (RH * DW + NTH - 1) / NTH;
    static constexpr int NE = (RH * RW + NTH - 1) / NTH, NZ = RH * (RW - RWL) / 2;
    static_assert(RWL % 2 == 0 && RW % 2 == 0, "whole dwords");
    uint32_t v[NL];
    TileItem t;
    bool fast;

    __device__ __forceinline__ void issue(const CostArgs& a, const TileItem& ti, int tid) {
        const Geom& g = a.g;
        t = ti;
        const uint16_t* idx = reinterpret_cast<const uint16_t*>(a.idx) + (int64_t)t.p * g.idx_pitch;
        fast = t.x0 - HALF >= 0 && t.x0 + RWL - HALF <= g.W && (g.W & 1) == 0 && ((t.x0 - HALF) & 1) == 0;
        if (fast) {
#pragma unroll
            for (int q = 0; q < NL; ++q) {
                const int e = min(tid + NTH * q, RH * DW - 1), i = e / DW, c = e - i * DW;
                const int roff = TileFill<HALF, RWL, TH, NTH>::row_base(g, t, i);  // even: dword aligned
                v[q] = *reinterpret_cast<const uint32_t*>(idx + roff + 2 * c);
            }
        }
    }

    __device__ __forceinline__ void commit(const CostArgs& a, uint16_t* s_idx, int tid) const {
        const Geom& g = a.g;
        uint32_t* s32 = reinterpret_cast<uint32_t*>(s_idx);
        if (fast) {
#pragma unroll
            for (int q = 0; q < NL; ++q) {
                const int e = tid + NTH * q, i = e / DW, c = e - i * DW;
                if (e < RH * DW) s32[i * (RW / 2) + c] = v[q];
            }
            for (int e = tid; e < NZ; e += NTH) {
                const int i = e / ((RW - RWL) / 2), c = e - i * ((RW - RWL) / 2);
                s32[i * (RW / 2) + RWL / 2 + c] = 0u;
            }
        } else {
            const uint16_t* idx = reinterpret_cast<const uint16_t*>(a.idx) + (int64_t)t.p * g.idx_pitch;
            uint32_t b[NE];
#pragma unroll
            for (int q = 0; q < NE; ++q) {  // all loads first: one round trip
                const int e = min(tid + NTH * q, RH * RW - 1), i = e / RW, j = e - i * RW;
                int gy = reflect_clamp(t.y0 - HALF + i, g.H);
                gy = min(max(gy, g.e0), g.e1 - 1);
                const int gx = reflect_clamp(t.x0 - HALF + min(j, RWL - 1), g.W);
                b[q] = idx[(uint32_t)((gy - g.e0) * g.W + gx)];
            }
#pragma unroll
            for (int q = 0; q < NE; ++q) {
                const int e = tid + NTH * q, i = e / RW, j = e - i * RW;
                if (e < RH * RW) s_idx[i * RW + j] = j < RWL ? (uint16_t)b[q] : (uint16_t)0;
            }
        }
    }
};

// Horizontal pass on row pairs: s_v holds float2 (row 2m, row 2m+1) per column,
// so v_pk_fma_f32 runs across a row pair and every tap reads a naturally
// aligned register pair (a row layout's odd taps needed register-pair shuffles,
// ~29% of the pass's VALU instructions).  HR output columns per item.
template <int HALF, int TH, int RW, int HR, int TLO = 0, int THI = 2 * HALF>
__device__ __forceinline__ void hpass_pair_filters(const f32x4* src, TapsPtr<HALF> taps, int f0,
                                                   int f1, f32x2 (&acc)[HR], int fslot = 0) {
    constexpr int NIN = HR + 2 * HALF;  // window columns (float2 each)
    constexpr int NQ = (NIN + 1) / 2;   // ds_read_b128, two columns each
#pragma unroll 1
    for (int f = f0; f < f1; ++f) {
        const f32x4* row = src + (f - fslot) * (TH / 2) * RW / 2;
        f32x4 v[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) v[q] = row[q];
        f32x2 in[2 * NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            in[2 * q] = v[q].xy;
            in[2 * q + 1] = v[q].zw;
        }
#pragma unroll
        for (int t = TLO; t <= THI; ++t) {
            const float k = taps->h[f][t];
            const f32x2 kk = {k, k};
#pragma unroll
            for (int xo = 0; xo < HR; ++xo) acc[xo] = __builtin_elementwise_fma(in[xo + t], kk, acc[xo]);
        }
    }
}

// ----------------------------------------------------------------------------
// cost_mfma: 8-row tiles in two channel groups -- channel 0's three filters (V
// then H), then channels 1-2's four -- so s_v holds at most four filter planes
// (23 KiB of LDS, 6 workgroups per CU).  Both vertical passes on the matrix
// cores in split f16: per 16-column block and pair of filters
// of one channel, one v_mfma_f32_16x16x32_f16 K-step covers the 28 region rows
// (+4 zero-weight rows) as hi.hi + hi.lo + lo.hi (each product exact in the
// fp32 accumulator; lo.lo ~2^-22 relative is dropped).  A = the stacked
// Toeplitz taps (rows = filter pair x 8 output rows, x 2^16, split on the host:
// build_vpass_f16_stack_fragments), B = the gathered opponent values (x 2^14),
// read from per-channel (hi, lo) f16 dword tables (split once per palette by
// the prep, PaletteArgs::opp16), so the gathers need no conversion (one LDS
// read per value).  D (x 2^30, folded exactly into the
// horizontal taps) holds 4 consecutive output rows of one filter and column per
// lane: two row-pair stores.  Stacks (f0, f1), (f2, -), (f3, f4), (f5, f6); wave
// w takes region columns 32w .. +31: 12 MFMAs per group and wave.
// (An exact-fp32 version on v_mfma_f32_16x16x4_f32, 56 MFMAs per wave, was 9%
// slower than the VALU pass: fp32 MFMA runs at the fp32 vector rate.)
// ----------------------------------------------------------------------------
// D of one 16x16 stack block -> s_v row pairs: lane (c = l & 15, q = l >> 4)
// holds rows 4(q & 1) .. +3 of the stack's filter q >> 1 at column c.
__device__ __forceinline__ void store_vstack(float* s_v, const f32x4v& d, int plane_a, int plane_b,
                                             int lk, int col) {
    constexpr int RW = 128, PAIRS = 4;
    const int plane = lk < 2 ? plane_a : plane_b;
    if (plane < 0) return;
    const int p0 = 2 * (lk & 1);
    f32x2* v = reinterpret_cast<f32x2*>(s_v);
    v[(plane * PAIRS + p0) * RW + col] = f32x2{d[0], d[1]};
    v[(plane * PAIRS + p0 + 1) * RW + col] = f32x2{d[2], d[3]};
}

// B fragments of one 16-column block: region rows 8q .. 8q+7 (q = lane >> 4) of
// column `col`.  Table entries hold (hi, lo) f16 of a channel in one dword
// (split_f16), so one LDS read per value; v_perm packs the halves.
__device__ __forceinline__ void pack_b(const uint32_t (&w)[8], f16x8& bh, f16x8& bl) {
    u32x4 h, l;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        h[m] = __builtin_amdgcn_perm(w[2 * m + 1], w[2 * m], 0x05040100u);  // hi halves
        l[m] = __builtin_amdgcn_perm(w[2 * m + 1], w[2 * m], 0x07060302u);  // lo halves
    }
    bh = __builtin_bit_cast(f16x8, h);
    bl = __builtin_bit_cast(f16x8, l);
}

// Both halves' B operands of a 16-row tile's block: w[0..7] = half 0's slots,
// w[8], w[9] = half 1's slots 0 and 1 (kv_row).  Half 1's operand is half 0's
// with dword 0 replaced: the caller issues half 0's MFMAs, then writes nh / nl
// into dword 0 (the registers are reused in place).
__device__ __forceinline__ void pack_b_halves(const uint32_t (&w)[10], u32x4& h, u32x4& l,
                                              uint32_t& nh, uint32_t& nl) {
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        h[m] = __builtin_amdgcn_perm(w[2 * m + 1], w[2 * m], 0x05040100u);  // hi halves
        l[m] = __builtin_amdgcn_perm(w[2 * m + 1], w[2 * m], 0x07060302u);  // lo halves
    }
    nh = __builtin_amdgcn_perm(w[9], w[8], 0x05040100u);
    nl = __builtin_amdgcn_perm(w[9], w[8], 0x07060302u);
}

__device__ __forceinline__ f32x4v mfma3(const f16x8& ah, const f16x8& al, const f16x8& bh,
                                        const f16x8& bl) {
    f32x4v d = {0.f, 0.f, 0.f, 0.f};
#ifndef HQ_ABL_MFMA1  // (timing ablation, wrong results: the hi.hi product only)
    d = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh, d, 0, 0, 0);
    d = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl, d, 0, 0, 0);
#endif
    d = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh, d, 0, 0, 0);
    return d;
}

template <int DE, bool TRIM, int MSK = 0>
__global__ __launch_bounds__(256, 6) void cost_mfma_kernel(CostArgs a, int P_) {
    constexpr int HALF = 10, RW = 128, TH = 8, HR = 2, T2 = 2 * HALF;
    constexpr int TW = RW - 2 * HALF, RH = TH + 2 * HALF;
    constexpr int NRUN = TW / HR, SLOTS = 64, NITEM = (TH / 2) * SLOTS;
    constexpr int PLANE = (TH / 2) * RW / 2;  // f32x4 per filter plane (row pairs)
    static_assert(NRUN <= SLOTS && NITEM <= 256 && RH <= 32, "tile");
    __shared__ f32x4 s_vq[4 * PLANE];
    __shared__ uint32_t s_ox[kMaxK];  // opponent x 2^14 as (hi, lo) f16 pairs: channel 0
    __shared__ uint2 s_oyz[kMaxK];     // channels 1, 2
    // 32 rows: the K = 32 step reads rows 28-31 too (zero taps; any finite index)
    __shared__ __attribute__((aligned(16))) uint8_t s_idx[32 * RW];
    __shared__ double s_red[4];
    float* s_v = reinterpret_cast<float*>(s_vq);
    const int tid = threadIdx.x;
    const Geom& g = a.g;
    TileItem cur;
    if constexpr (MSK != 0) cur = tile_item<TW, TH, MSK>(a, xcd_remap(blockIdx.x, a.nlive * P_), P_);
    else cur = tile_item<TW, TH>(a, xcd_remap(blockIdx.x, a.ntiles * P_), P_);
    tile_item_to_grid<DE, TW, TH>(a, cur);
    const TapsPtr<HALF> taps = (TapsPtr<HALF>)(uintptr_t)a.taps;  // H taps x 2^-30
    const int lane = tid & 63, wv = tid >> 6, lc = lane & 15, lk = lane >> 4;
    const uint4* frag = a.vfrag16 + (TRIM ? 2 * 4 * 2 * 64 : 0) + lane;  // [trim][half 0][stack][hi,lo][lane]

    TileFill<HALF, RW, TH> fill;
    fill.issue(a, cur, tid);
    uint4 F0h = frag[(0 * 2 + 0) * 64], F0l = frag[(0 * 2 + 1) * 64];  // group 0 stacks
    uint4 F1h = frag[(1 * 2 + 0) * 64], F1l = frag[(1 * 2 + 1) * 64];
    // every entry (zeros for tid >= K): the zero-weight rows 28-31 gather arbitrary
    // indices, and 0 x NaN would be NaN
    s_ox[tid] = fill.ov.x;
    s_oyz[tid] = make_uint2(fill.ov.y, fill.ov.z);
    fill.template commit_idx<RW>(a, s_idx, tid);
    const int m = tid / SLOTS, jr = tid % SLOTS;
    const bool has_item = tid < NITEM && jr < NRUN;
    const int gy0 = cur.y0 + 2 * m, gx0 = cur.x0 + HR * jr;
    __syncthreads();

    const int col0 = 32 * wv + lc;
    const f32x4* hsrc = &s_vq[(m * RW + HR * jr) / 2];
    f32x2 acc0[HR], acc1[HR], acc2[HR];
#pragma unroll
    for (int xo = 0; xo < HR; ++xo) acc0[xo] = acc1[xo] = acc2[xo] = f32x2{0.f, 0.f};

    // ---- group 0: channel 0 -> planes 0-2 ----
    {
        const f16x8 a0h = __builtin_bit_cast(f16x8, F0h), a0l = __builtin_bit_cast(f16x8, F0l);
        const f16x8 a1h = __builtin_bit_cast(f16x8, F1h), a1l = __builtin_bit_cast(f16x8, F1l);
#pragma unroll
        for (int bb = 0; bb < 2; ++bb) {
            uint32_t w[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) w[j] = s_ox[s_idx[kv_row(0, lk, j) * RW + col0 + 16 * bb]];
            f16x8 bh, bl;
            pack_b(w, bh, bl);
            store_vstack(s_v, mfma3(a0h, a0l, bh, bl), 0, 1, lk, col0 + 16 * bb);
            store_vstack(s_v, mfma3(a1h, a1l, bh, bl), 2, -1, lk, col0 + 16 * bb);
        }
    }
    const uint4 F2h = frag[(2 * 2 + 0) * 64], F2l = frag[(2 * 2 + 1) * 64];  // group 1 stacks,
    const uint4 F3h = frag[(3 * 2 + 0) * 64], F3l = frag[(3 * 2 + 1) * 64];  // in flight during H
    __syncthreads();
    if (has_item) {
        if constexpr (TRIM) {
            hpass_pair_filters<HALF, TH, RW, HR, kTrimLo[0], kTrimHi[0]>(hsrc, taps, 0, 1, acc0);
            hpass_pair_filters<HALF, TH, RW, HR, 0, T2>(hsrc, taps, 1, 3, acc0);
        } else {
            hpass_pair_filters<HALF, TH, RW, HR, 0, T2>(hsrc, taps, 0, 3, acc0);
        }
    }
    __syncthreads();

    // ---- group 1: channels 1, 2 -> planes 0-3 ----
    {
        const f16x8 a2h = __builtin_bit_cast(f16x8, F2h), a2l = __builtin_bit_cast(f16x8, F2l);
        const f16x8 a3h = __builtin_bit_cast(f16x8, F3h), a3l = __builtin_bit_cast(f16x8, F3l);
#pragma unroll
        for (int bb = 0; bb < 2; ++bb) {
            uint32_t wy[8], wz[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const uint2 e = s_oyz[s_idx[kv_row(0, lk, j) * RW + col0 + 16 * bb]];
                wy[j] = e.x; wz[j] = e.y;
            }
            f16x8 bh, bl;
            pack_b(wy, bh, bl);
            store_vstack(s_v, mfma3(a2h, a2l, bh, bl), 0, 1, lk, col0 + 16 * bb);
            pack_b(wz, bh, bl);
            store_vstack(s_v, mfma3(a3h, a3l, bh, bl), 2, 3, lk, col0 + 16 * bb);
        }
    }
    float labv[2][3][HR];
    uint32_t mk[2];  // MSK: the mask bytes of each row's 2 pixels, one load at the LabRef offset
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        bool ok = has_item && gy0 + r < g.r1 && gx0 < g.W;
        if constexpr (DE == 2) ok = ok && gy0 + r >= g.r0;
        const uint32_t off = ok ? (uint32_t)((gy0 + r - g.r0) * g.lab_pitch + gx0) : 0u;
        if constexpr (MSK != 0) mk[r] = *reinterpret_cast<const uint16_t*>(a.mask + off);
        const float* src3[3] = {a.labL, a.labA, a.labB};
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float2 v = *reinterpret_cast<const float2*>(
                reinterpret_cast<const char*>(src3[ch]) + (off << 2));  // 32-bit byte offset
            labv[r][ch][0] = v.x; labv[r][ch][1] = v.y;
        }
    }
    __syncthreads();

    double sum = 0.0;
    if (has_item) {
        if constexpr (TRIM) {
            hpass_pair_filters<HALF, TH, RW, HR, kTrimLo[1], kTrimHi[1]>(hsrc, taps, 3, 4, acc1, 3);
            hpass_pair_filters<HALF, TH, RW, HR, 0, T2>(hsrc, taps, 4, 5, acc1, 3);
            hpass_pair_filters<HALF, TH, RW, HR, kTrimLo[2], kTrimHi[2]>(hsrc, taps, 5, 6, acc2, 3);
            hpass_pair_filters<HALF, TH, RW, HR, 0, T2>(hsrc, taps, 6, 7, acc2, 3);
        } else {
            hpass_pair_filters<HALF, TH, RW, HR, 0, T2>(hsrc, taps, 3, 5, acc1, 3);
            hpass_pair_filters<HALF, TH, RW, HR, 0, T2>(hsrc, taps, 5, 7, acc2, 3);
        }
        float part = 0.f;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
#pragma unroll
            for (int xo = 0; xo < HR; ++xo) {
                const float3 lf = opp2f_fast(acc0[xo][r], acc1[xo][r], acc2[xo][r], a.m_lab);
                const float e = delta_e_f<DE>(labv[r][0][xo], labv[r][1][xo], labv[r][2][xo], lf);
                bool in = gy0 + r < g.r1 && gx0 + xo < g.W;
                if constexpr (DE == 2) in = in && gy0 + r >= g.r0;
                if constexpr (MSK == 2) {  // one fma with the weight; weight 0 is the select
                    const uint32_t wb = (mk[r] >> (8 * xo)) & 0xffu;
                    part = in && wb != 0u ? fmaf(e, (float)wb, part) : part;
                } else
                if constexpr (MSK == 1) {  // a select: a masked-out NaN stays out of the sum
                    part += in && ((mk[r] >> (8 * xo)) & 0xffu) != 0u ? e : 0.f;
                } else
                part += in ? e : 0.f;
                if (a.pix_err && in)  // test option: the per-pixel dE (CL:201-209's error image)
                    a.pix_err[(int64_t)cur.p * a.pix_pitch + (int64_t)(gy0 + r - g.r0) * g.W + gx0 + xo] = e;
            }
        }
        sum = (double)part;
    }
    sum = wave_sum_to_lane63(sum);
    if ((tid & 63) == 63) s_red[tid >> 6] = sum;
    __syncthreads();
    if (tid == 0)
        acc_add(a.acc, a.acc_P, a.acc_p0 + cur.p, cur.tile, (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]));
}

// ----------------------------------------------------------------------------
// cost16w<HB>: 16 x 128 output tiles of a (16 + 2 HB) x (128 + 2 HB) region,
// HB = the tap bucket's half-width: the filters' own half-width H <= HB sits
// centred in 2 HB + 1 taps (zero-padded; Tile16, fast_bucket), so every viewing
// geometry of the plugin (dpi, distance: HQ:229-231, SP:80-102, IM:408) up to
// H = 24 runs this kernel.  HB = 10 is the default 21-tap set.  The random
// opponent-table gathers of the vertical pass and the horizontal windows are
// the kernel's LDS traffic; FP32 VALU issue (horizontal taps, Lab/dE) bounds it.
// - vertical pass on the matrix cores: output rows 0-7 take region rows
//   0 .. 32 S - 1 (S K steps of 32 rows), rows 8-15 take rows 8 .. 32 S + 7.
//   Lane group g holds every 4th row (kv_row: K slot (g, j) of step s = row
//   32 s + 4 j + g), so half 1's operand of step s is half 0's with dword 0
//   replaced by the next step's dword 0: each lane gathers 8 S + 2 rows (the
//   ones past the region are zero, not gathered) for 2 x 8 output rows, no
//   divergence.  At HB = 10 (S = 1): 36 gathered rows per 16 output rows.
//   Above HB = 10 the (hi, lo) pair layout instead (vblock_pair): steps of 16
//   rows, the gathered dwords used as B operands as they are, 4 S + 2 rows per
//   lane.
//   RW / 16 blocks of 16 columns (ranges of 32) cover the region columns
//   (+ unread ones): each block is the 16 columns of one parity half of a range
//   (lane n -> column 4(n >> 1) + 2 (b & 1) + (n & 1)), so its stores fill 16
//   contiguous float2 of one half: conflict free without padding.  Block sets
//   {s, s+4, s+8} go to the waves, rotated per workgroup.
// - horizontal pass: items of 4 output columns x a row pair (256 items, one per
//   thread: 8 row pairs x 32), a (4 + 2 HB)-column window = 2 + HB ds_read_b128
//   per filter for 8 outputs.  Row-pair rows store their column pairs split by
//   parity (pair p -> half p & 1, slot p >> 1), so read q of item j lands at
//   half q & 1, slot j + q / 2: lanes 16 B apart, conflict free.  (The
//   108-column tile of a 128-column region gave 27 items to 32 threads: 16% of
//   the lanes idle through the horizontal pass and Lab/dE; 0.398 vs 0.383 ms.)
// - the row-pair planes fit 4 workgroups per CU (3 for HB > 10) three filters
//   at a time, so the channels run in three phases: channel 0 (f0, f1, f2),
//   channel 1 (f3, f4), channel 2 (f5, f6).  Channels 1 and 2 share one gather
//   per region row; channel 2's vertical results wait in registers through
//   channel 1's horizontal pass.  HB = 10: 39,584 B of LDS.
// ----------------------------------------------------------------------------
constexpr int kTH16 = 16;
#ifndef HQ_LAB_SKIPLIN
#define HQ_LAB_SKIPLIN 1  // cost16w: skip the linear Lab segment when no pixel of the wave is in it
#endif
#ifndef HQ_LAB_NT
#define HQ_LAB_NT 0  // 1: LabRef read with non-temporal loads (streamed past the caches)
#endif

template <int HB, int NW = 4>
struct Tile16 {
    static constexpr int TH = kTH16, TW = 32 * NW, HR = 4;  // NW waves: 4 (16 x 128) or 8 (16 x 256)
    static constexpr int RWL = (TW + 2 * HB + 3) / 4 * 4;  // region columns read (whole dwords)
    static constexpr int RW = (RWL + 31) / 32 * 32;    // LDS pitch: whole 32-column ranges
    static constexpr int RH = TH + 2 * HB;             // region rows
    static constexpr int NBLK = RW / 16;               // vertical-pass column blocks
    static constexpr int NSET = (NBLK + NW - 1) / NW;  // blocks per wave (at most)
    static constexpr int WH = RW / 2;                  // float2 per half of a permuted row-pair row
    // vertical pass: the (hi, lo) pair layout (vblock_pair) above the 21-tap
    // bucket, the 32-row layout (vblock) at HB = 10 (same-box A/B: pair layout
    // -3% cost at HB = 19, -1.5% at 15, +4% at 10, where it needs 4 MFMAs per
    // half and stack instead of 3 and its overlapping B windows cost copies)
    static constexpr bool PAIR = HB > 10;
    static constexpr int S = PAIR ? pair_steps(HB) : bucket_steps(HB);  // MFMA K steps per half
    static constexpr int NJ = PAIR ? 4 * S + 2 : 8 * S + 2;  // rows 4 n + g a lane gathers
    static constexpr int AH = PAIR ? 1 : 2;  // fragment sets per stack and step (the pair layout's halves share)
    static constexpr int PLANE4 = (TH / 2) * RW / 2;   // f32x4 per filter plane
    static constexpr int NQ = (HR + 2 * HB) / 2;       // horizontal window reads per filter
    static_assert(RWL % 4 == 0 && RWL / 4 >= 8 * NW && RWL / 4 < 16 * NW, "TileFill: 8 NW <= dwords per row < 16 NW");
    static_assert(NSET <= 3, "three blocks per wave at most");
};

// float2 position of column `col` in a permuted row-pair row: half = bit 1 of
// col, 16-B slot col >> 2, float2 col & 1.
template <int WH>
__device__ __forceinline__ int wide_pos(int col) {
    return ((col >> 1) & 1) * WH + ((col >> 2) << 1) + (col & 1);
}

// Horizontal pass of filter f for item j (output columns 4j .. 4j+3) of a row
// pair: src = the row-pair row in plane 0; pstride = f32x4 per plane; taps
// [TLO, THI].  Item j's read q (columns 4j + 2q, +1) sits at half q & 1,
// slot j + q / 2.  Windows longer than 24 columns run in chunks of 12 taps
// (each chunk's reads issued together) to bound the live registers.
template <int HB, int TLO = 0, int THI = 2 * HB, int WH = 80>
__device__ __forceinline__ void hpass_wide(const f32x4* src, int j, TapsPtr<HB> taps, int f,
                                           int plane, int pstride, f32x2 (&acc)[4]) {
    constexpr int HR = 4;
    constexpr int CH = HB <= 10 ? 2 * HB + 1 : HB == 19 ? HQ_CH19 : HQ_CHW;  // taps per chunk
    const f32x4* row = src + plane * pstride + j;
#ifdef HQ_ABL_NOHPASS  // timing ablation (wrong results): one window read, no taps
    {
        const f32x4 v = row[0];
        acc[0] += v.xy;
        acc[1] += v.zw;
        return;
    }
#endif
#pragma unroll
    for (int t0 = TLO; t0 <= THI; t0 += CH) {
        const int t1 = t0 + CH - 1 < THI ? t0 + CH - 1 : THI;
        const int q0 = t0 / 2, q1 = (t1 + HR - 1) / 2;  // reads covering columns t0 .. t1 + 3
        f32x2 in[2 * (CH / 2 + 3)];
#pragma unroll
        for (int q = q0; q <= q1; ++q) {
            const f32x4 v = row[(q & 1) * (WH / 2) + (q >> 1)];
            in[2 * (q - q0)] = v.xy;
            in[2 * (q - q0) + 1] = v.zw;
        }
#pragma unroll
        for (int t = t0; t <= t1; ++t) {
            const float k = taps->h[f][t];
            const f32x2 kk = {k, k};
#pragma unroll
            for (int xo = 0; xo < HR; ++xo)
                acc[xo] = __builtin_elementwise_fma(in[xo + t - 2 * q0], kk, acc[xo]);
        }
    }
}

// D of one 16x16 stack block of output-row half `half` -> permuted row pairs:
// lane (c = l & 15, q = l >> 4) holds rows 8 half + 4(q & 1) .. +3 of the
// stack's filter q >> 1 at its column.  Addresses hoisted: `base` = the
// lane's float2 slot of block set i = 0, half 0 in its plane (vstack_base);
// block i and half add compile-time offsets (block b + 4 moves 64 columns =
// 32 float2 of the permuted row).
template <int WH>
__device__ __forceinline__ f32x2* vstack_base(float* s_v, int plane, int lk, int col0) {
    constexpr int PAIRS = kTH16 / 2, ROW = 2 * WH;
    return reinterpret_cast<f32x2*>(s_v) + (plane * PAIRS + 2 * (lk & 1)) * ROW + wide_pos<WH>(col0);
}
template <int WH, int NW = 4>
__device__ __forceinline__ void store_vstack_at(f32x2* base, const f32x4v& d, int i, int half) {
    constexpr int ROW = 2 * WH;
#ifdef HQ_ABL_NOVSTORE  // timing ablation (wrong results): vertical results not stored
    if (d[0] != 12345.f) return;
#endif
    f32x2* v = base + 4 * half * ROW + 8 * NW * i;  // block set i + 1: 16 NW columns on
    v[0] = f32x2{d[0], d[1]};
    v[ROW] = f32x2{d[2], d[3]};
}

__device__ __forceinline__ f32x4v mfma3_acc(const f16x8& ah, const f16x8& al, const f16x8& bh,
                                            const f16x8& bl, f32x4v d) {
    d = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh, d, 0, 0, 0);
    d = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl, d, 0, 0, 0);
    d = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh, d, 0, 0, 0);
    return d;
}

// One column block's vertical products for up to two stacks: w[NJ] = the
// gathered (hi, lo) dwords of rows 4 n + g; A[stack][half][step][hi, lo] the
// split-f16 tap fragments.  d[stack][half] = both halves' 16 x 16 blocks.
template <int S, int NST>
__device__ __forceinline__ void vblock(const uint32_t (&w)[8 * S + 2], const uint4 (&A)[NST][2][S][2],
                                       f32x4v (&d)[NST][2]) {
    auto H = [](const uint4& u) { return __builtin_bit_cast(f16x8, u); };
    auto B = [](const u32x4& u) { return __builtin_bit_cast(f16x8, u); };
#pragma unroll
    for (int st = 0; st < NST; ++st) d[st][0] = d[st][1] = f32x4v{0.f, 0.f, 0.f, 0.f};
#ifdef HQ_ABL_NOMFMA  // timing ablation (wrong results): no operand packing, no MFMA
#pragma unroll
    for (int st = 0; st < NST; ++st) {
        d[st][0] = f32x4v{__uint_as_float(w[0]), __uint_as_float(w[1]), __uint_as_float(A[st][0][0][0].x), 0.f};
        d[st][1] = f32x4v{__uint_as_float(w[2]), __uint_as_float(w[3]), __uint_as_float(A[st][1][0][1].y), 0.f};
    }
    return;
#endif
#pragma unroll
    for (int s = 0; s < S; ++s) {
        u32x4 bh, bl;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            bh[m] = __builtin_amdgcn_perm(w[8 * s + 2 * m + 1], w[8 * s + 2 * m], 0x05040100u);  // hi halves
            bl[m] = __builtin_amdgcn_perm(w[8 * s + 2 * m + 1], w[8 * s + 2 * m], 0x07060302u);  // lo halves
        }
        const uint32_t nh = __builtin_amdgcn_perm(w[8 * s + 9], w[8 * s + 8], 0x05040100u);
        const uint32_t nl = __builtin_amdgcn_perm(w[8 * s + 9], w[8 * s + 8], 0x07060302u);
#pragma unroll
        for (int st = 0; st < NST; ++st)
            d[st][0] = mfma3_acc(H(A[st][0][s][0]), H(A[st][0][s][1]), B(bh), B(bl), d[st][0]);
        bh[0] = nh;  // half 1 of step s: half 0's operand with dword 0 of step s + 1
        bl[0] = nl;
#pragma unroll
        for (int st = 0; st < NST; ++st)
            d[st][1] = mfma3_acc(H(A[st][1][s][0]), H(A[st][1][s][1]), B(bh), B(bl), d[st][1]);
    }
}

// One column block's vertical products in the (hi, lo) pair layout: w[n] =
// the gathered dword of region row 4 n + g, its (hi, lo) f16 pair, used as
// two K slots of the B operand as is (no repacking).  Step u of half 0 reads
// w[4 u .. 4 u + 3] (rows 16 u .. 16 u + 15 over the four lane groups), half 1
// the rows 8 further on, w[4 u + 2 .. 4 u + 5], with the same A fragments
// A[stack][u][hi, lo] (each K-slot pair holds one tap part twice): hi taps x
// (hi + lo) data, then lo taps x (hi + lo) data, fp32 accumulate -- the full
// split product (the lo.lo term included), two MFMAs per 16 rows and no
// v_perm (the 32-row layout needed ten per step to split hi and lo halves).
template <int N>
using u32xn = uint32_t __attribute__((ext_vector_type(N)));

// dwords O .. O + 3 of the gathered rows as one B operand: a sub-register of
// the rows' single wide register, so the overlapping windows of the two
// halves need no copies
template <int O, int N>
__device__ __forceinline__ f16x8 pair_window(const u32xn<N>& v) {
    return __builtin_bit_cast(f16x8, __builtin_shufflevector(v, v, O, O + 1, O + 2, O + 3));
}

template <int U, int S, int NST>
__device__ __forceinline__ void vblock_pair_step(const u32xn<4 * S + 2>& v, const uint4 (&A)[NST][S][2],
                                                 f32x4v (&d)[NST][2]) {
    if constexpr (U < S) {
        auto H = [](const uint4& u) { return __builtin_bit_cast(f16x8, u); };
        const f16x8 b0 = pair_window<4 * U, 4 * S + 2>(v);
        const f16x8 b1 = pair_window<4 * U + 2, 4 * S + 2>(v);
#pragma unroll
        for (int st = 0; st < NST; ++st) {
            d[st][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(H(A[st][U][0]), b0, d[st][0], 0, 0, 0);
            d[st][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(H(A[st][U][1]), b0, d[st][0], 0, 0, 0);
            d[st][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(H(A[st][U][0]), b1, d[st][1], 0, 0, 0);
            d[st][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(H(A[st][U][1]), b1, d[st][1], 0, 0, 0);
        }
        vblock_pair_step<U + 1, S, NST>(v, A, d);
    }
}

template <int S, int NST>
__device__ __forceinline__ void vblock_pair(const uint32_t (&w)[4 * S + 2], const uint4 (&A)[NST][S][2],
                                            f32x4v (&d)[NST][2]) {
    u32xn<4 * S + 2> v;
#pragma unroll
    for (int n = 0; n < 4 * S + 2; ++n) v[n] = w[n];
#pragma unroll
    for (int st = 0; st < NST; ++st) d[st][0] = d[st][1] = f32x4v{0.f, 0.f, 0.f, 0.f};
    vblock_pair_step<0, S, NST>(v, A, d);
}

// cost16w's vertical products in its bucket's layout (Tile16::PAIR)
template <bool PAIR, int S, int NST, int AH, int NJ>
__device__ __forceinline__ void vblock_any(const uint32_t (&w)[NJ], const uint4 (&A)[NST][AH][S][2],
                                           f32x4v (&d)[NST][2]) {
    if constexpr (PAIR) vblock_pair<S, NST>(w, *reinterpret_cast<const uint4(*)[NST][S][2]>(&A), d);
    else vblock<S, NST>(w, A, d);
}

#ifndef HQ_LB15
#define HQ_LB15 3  // waves per SIMD of the 15-tap bucket (4, with its (y, z) table moved into plane 2 to
                   // fit 4 workgroups' LDS: no faster, 0.476 against 0.477 ms at 150/30)
#endif
#ifndef HQ_LB24
#define HQ_LB24 2  // waves per SIMD of the 24-tap bucket (3: 92 B of spill, 0.823-0.826 against 0.820 ms)
#endif
#ifndef HQ_LB19
#define HQ_LB19 3  // waves per SIMD of the 19-tap bucket
#endif
// occupancy per bucket: LDS allows 4 workgroups per CU at HB = 10, 3 above;
// chunked palettes (NCH > 1: 16-bit indices, a table of 256 NCH entries): 3 up
// to 1,024 colours, 2 up to 4,096, 1 above (the 64 KiB table at 8,192)
template <int HB, int NCH = 1>
constexpr int cost16w_waves() {
    return NCH > 16 ? 1 : NCH > 4 ? 2 : NCH > 1 ? 3 : HB == 10 ? 4 : HB == 15 ? HQ_LB15 : HB == 19 ? HQ_LB19 : HQ_LB24;
}

// NCH > 1 (chunked palettes, 256 < K <= 256 NCH; HB = 10): the index image is
// 16-bit and the split opponent table has KT = 256 NCH entries, in dynamic LDS
// (8 KT bytes): channel 0's x words first, then -- loaded from global memory
// during channel 0's horizontal pass, once its gathers are done -- the (y, z)
// pairs in the same bytes.
template <int HB, int DE, bool TRIM, int NW, int NCH = 1, int MSK = 0>
__global__ __launch_bounds__(64 * NW, (cost16w_waves<HB, NCH>())) void cost16w_kernel(CostArgs a, int P_) {
    using Gm = Tile16<HB, NW>;
    constexpr int NTH = 64 * NW, IPR = 8 * NW;  // threads; horizontal items per row pair
    constexpr int TH = kTH16, HR = 4, T2 = 2 * HB, TW = Gm::TW, RWL = Gm::RWL, RW = Gm::RW;
    constexpr int RH = Gm::RH, WH = Gm::WH, NBLK = Gm::NBLK, NSET = Gm::NSET, S = Gm::S, NJ = Gm::NJ;
    constexpr bool PAIR = Gm::PAIR;
    constexpr int AH = Gm::AH;
    constexpr int ROW = 2 * WH, PLANE4 = Gm::PLANE4;
    constexpr int L0 = HB - trim_w(HB, 0), L1 = HB - trim_w(HB, 1), L2 = HB - trim_w(HB, 2);
    static_assert(TW / HR == IPR && 8 * IPR == NTH, "one horizontal item per thread");
    constexpr bool W16 = NCH > 1;
    constexpr int KT = kMaxK * NCH, NTE = KT / NTH;  // table entries (per thread)
    using IT = std::conditional_t<W16, uint16_t, uint8_t>;
    __shared__ f32x4 s_vq[3 * PLANE4];
    __shared__ uint32_t s_ox8[W16 ? 1 : kMaxK];  // opponent x 2^14 as (hi, lo) f16 pairs: channel 0
    __shared__ uint2 s_oyz8[W16 ? 1 : kMaxK];    // channels 1, 2
    __shared__ __attribute__((aligned(16))) IT s_idx[RH * RW];
    extern __shared__ __attribute__((aligned(16))) uint32_t s_tab[];  // W16: 8 KT bytes
    uint32_t* const s_ox = W16 ? s_tab : s_ox8;
    uint2* const s_oyz = W16 ? reinterpret_cast<uint2*>(s_tab) : s_oyz8;
    float* s_v = reinterpret_cast<float*>(s_vq);
    const int tid = threadIdx.x;
    const Geom& g = a.g;
    TileItem cur;
    if constexpr (MSK != 0) cur = tile_item<TW, TH, MSK>(a, xcd_remap(blockIdx.x, a.nlive * P_), P_);
    else cur = tile_item<TW, TH>(a, xcd_remap(blockIdx.x, a.ntiles * P_), P_);
    tile_item_to_grid<DE, TW, TH>(a, cur);
    const TapsPtr<HB> taps = (TapsPtr<HB>)(uintptr_t)a.taps;  // H taps x 2^-30
    const int lane = tid & 63, wv = tid >> 6, lc = lane & 15, lk = lane >> 4;
    // pair layout: [trim][step][stack][hi, lo][lane] (build_vpass_f16_pair_fragments);
    // else [trim][half][step][stack][hi, lo][lane] (build_vpass_f16_stack_fragments)
    const uint4* frag = (PAIR ? a.vfrag16p : a.vfrag16) + (TRIM ? AH * S * 4 * 2 * 64 : 0) + lane;
    auto F = [&](int half, int s, int st, int hl) { return frag[(((half * S + s) * 4 + st) * 2 + hl) * 64]; };

    std::conditional_t<W16, TileFill16<HB, RWL, RW, TH, NTH>, TileFill<HB, RWL, TH, NTH>> fill;
    fill.issue(a, cur, tid);
    uint32_t tx[W16 ? NTE : 1];  // W16: this thread's x words of the table (entries tid + NTH j)
    if constexpr (W16) {
#pragma unroll
        for (int j = 0; j < NTE; ++j) tx[j] = a.opp16[(int64_t)cur.p * KT + tid + NTH * j].x;
    }
    uint4 A[2][AH][S][2];  // channel 0's stacks (f0, f1), (f2, -); then channels 1-2's
#pragma unroll
    for (int st = 0; st < 2; ++st)
#pragma unroll
        for (int h = 0; h < AH; ++h)
#pragma unroll
            for (int s = 0; s < S; ++s) {
                A[st][h][s][0] = F(h, s, st, 0);
                A[st][h][s][1] = F(h, s, st, 1);
            }
    // every entry (zeros for tid >= K): zero-weight rows and the columns past
    // the region gather arbitrary indices, and 0 x NaN would be NaN
    if constexpr (W16) {
#pragma unroll
        for (int j = 0; j < NTE; ++j) s_ox[tid + NTH * j] = tx[j];
        fill.commit(a, s_idx, tid);
    } else {
        if (NTH == kMaxK || tid < kMaxK) {
            s_ox[tid] = fill.ov.x;
            s_oyz[tid] = make_uint2(fill.ov.y, fill.ov.z);
        }
        fill.template commit_idx<RW>(a, s_idx, tid);
    }
    // H item: row pair m, output columns 4j .. 4j+3 (every thread has one)
    const int m = tid / IPR, jr = tid % IPR;
    const int gy0 = cur.y0 + 2 * m, gx0 = cur.x0 + HR * jr;
    const f32x4* hsrc = &s_vq[(m * ROW) / 2];
    f32x2 acc0[HR], acc1[HR], acc2[HR];
#pragma unroll
    for (int xo = 0; xo < HR; ++xo) acc0[xo] = acc1[xo] = acc2[xo] = f32x2{0.f, 0.f};
    __syncthreads();

    // Block b = wset + NW i covers the 16 columns of parity half b & 1 of range
    // b >> 1.  With 10 blocks over 4 waves, sets 0 and 1 hold 3 blocks and sets
    // 2 and 3 hold 2 (18 over 8: sets 0, 1 hold 3): the sets rotate with the
    // workgroup, so the extra blocks do not land on the same SIMDs in every
    // workgroup.
    const int wset = (wv + (int)blockIdx.x) & (NW - 1);
    const int col0 = 32 * (wset >> 1) + 4 * (lc >> 1) + (lc & 1) + 2 * (wset & 1);
    f32x2* const st01 = vstack_base<WH>(s_v, lk < 2 ? 0 : 1, lk, col0);  // stacks -> planes 0, 1
    f32x2* const st2 = vstack_base<WH>(s_v, 2, lk, col0);                // (f2, -) -> plane 2
    // gather of K slot n (rows 4 n + lk) of column col from a table; slots past
    // the region are zero (zero taps), a partly covered slot reads a clamped row
    auto gather_row = [&](int n, int col) {
        const int row = 4 * n + lk;
        return (4 * n + 3 < RH ? row : min(row, RH - 1)) * RW + col;
    };
    // index of a gathered element (timing ablations, wrong results: HQ_ABL_NOIDX
    // skips the index read, HQ_ABL_NOTAB the table read below)
    auto gidx = [&](int n, int col) -> uint32_t {
#ifdef HQ_ABL_NOIDX
        return (uint32_t)(gather_row(n, col) & 255);
#else
        return s_idx[gather_row(n, col)];
#endif
    };

    // ---- channel 0: stacks (f0, f1) -> planes 0, 1 and (f2, -) -> plane 2 ----
#pragma unroll
    for (int i = 0; i < NSET; ++i) {
        const int b = wset + NW * i;
        if (b >= NBLK) break;
        const int col = col0 + 16 * NW * i;
        uint32_t w[NJ];
#pragma unroll
#ifdef HQ_ABL_NOTAB
        for (int n = 0; n < NJ; ++n) w[n] = 4 * n < RH ? gidx(n, col) * 0x00010001u : 0u;
#else
        for (int n = 0; n < NJ; ++n) w[n] = 4 * n < RH ? s_ox[gidx(n, col)] : 0u;
#endif
        f32x4v d[2][2];
        vblock_any<PAIR>(w, A, d);
        store_vstack_at<WH, NW>(st01, d[0][0], i, 0);
        store_vstack_at<WH, NW>(st01, d[0][1], i, 1);
        if (lk < 2) {  // the (f2, -) stack's second filter slot is empty
            store_vstack_at<WH, NW>(st2, d[1][0], i, 0);
            store_vstack_at<WH, NW>(st2, d[1][1], i, 1);
        }
    }
    // channel 1-2 stacks: in flight during channel 0's horizontal pass with one
    // K step (32 VGPRs); with two, loaded after it (64 VGPRs would spill)
    auto load_a12 = [&]() {
#pragma unroll
        for (int st = 0; st < 2; ++st)
#pragma unroll
            for (int h = 0; h < AH; ++h)
#pragma unroll
                for (int s = 0; s < S; ++s) {
                    A[st][h][s][0] = F(h, s, 2 + st, 0);
                    A[st][h][s][1] = F(h, s, 2 + st, 1);
                }
    };
    // (32 fragment VGPRs in flight at most)
    constexpr bool A12_EARLY = AH * S <= 2;
    if constexpr (A12_EARLY) load_a12();
    __syncthreads();
    uint2 tyz[W16 ? NTE : 1];  // W16: the (y, z) words, in flight through channel 0's horizontal pass
    if constexpr (W16) {
#pragma unroll
        for (int j = 0; j < NTE; ++j) {
            const uint4 e = a.opp16[(int64_t)cur.p * KT + tid + NTH * j];
            tyz[j] = make_uint2(e.y, e.z);
        }
    }
    if constexpr (TRIM) hpass_wide<HB, L0, T2 - L0, WH>(hsrc, jr, taps, 0, 0, PLANE4, acc0);
    else hpass_wide<HB, 0, T2, WH>(hsrc, jr, taps, 0, 0, PLANE4, acc0);
    hpass_wide<HB, 0, T2, WH>(hsrc, jr, taps, 1, 1, PLANE4, acc0);
    hpass_wide<HB, 0, T2, WH>(hsrc, jr, taps, 2, 2, PLANE4, acc0);
    if constexpr (W16) {  // (the x words' last reads were the gathers before the barrier)
#pragma unroll
        for (int j = 0; j < NTE; ++j) s_oyz[tid + NTH * j] = tyz[j];
    }
    __syncthreads();

    {
        // ---- channels 1, 2: one gather of (y, z) per region row; stack (f3, f4)
        // -> planes 0, 1 now, stack (f5, f6)'s results held in registers until
        // channel 1's horizontal pass has read the planes ----
        if constexpr (!A12_EARLY) load_a12();
        f32x4v d5[NSET][2];
#pragma unroll
        for (int i = 0; i < NSET; ++i) {
            const int b = wset + NW * i;
            if (b >= NBLK) break;
            const int col = col0 + 16 * NW * i;
            uint32_t wy[NJ], wz[NJ];
#pragma unroll
            for (int n = 0; n < NJ; ++n) {
                if (4 * n < RH) {
#ifdef HQ_ABL_NOTAB
                    const uint32_t ix = gidx(n, col);
                    const uint2 e = make_uint2(ix * 0x00010001u, ix * 0x00020002u);
#else
                    const uint2 e = s_oyz[gidx(n, col)];
#endif
                    wy[n] = e.x; wz[n] = e.y;
                } else {
                    wy[n] = wz[n] = 0u;
                }
            }
            {
                const uint4(&Ay)[1][AH][S][2] = *reinterpret_cast<const uint4(*)[1][AH][S][2]>(&A[0]);
                f32x4v d[1][2];
                vblock_any<PAIR>(wy, Ay, d);
                store_vstack_at<WH, NW>(st01, d[0][0], i, 0);
                store_vstack_at<WH, NW>(st01, d[0][1], i, 1);
            }
            {
                const uint4(&Az)[1][AH][S][2] = *reinterpret_cast<const uint4(*)[1][AH][S][2]>(&A[1]);
                f32x4v d[1][2];
                vblock_any<PAIR>(wz, Az, d);
                d5[i][0] = d[0][0];
                d5[i][1] = d[0][1];
            }
        }
        __syncthreads();
        if constexpr (TRIM) hpass_wide<HB, L1, T2 - L1, WH>(hsrc, jr, taps, 3, 0, PLANE4, acc1);
        else hpass_wide<HB, 0, T2, WH>(hsrc, jr, taps, 3, 0, PLANE4, acc1);
        hpass_wide<HB, 0, T2, WH>(hsrc, jr, taps, 4, 1, PLANE4, acc1);
        __syncthreads();

        // ---- channel 2: stack (f5, f6) -> planes 0, 1 ----
#pragma unroll
        for (int i = 0; i < NSET; ++i) {
            const int b = wset + NW * i;
            if (b >= NBLK) break;
            store_vstack_at<WH, NW>(st01, d5[i][0], i, 0);
            store_vstack_at<WH, NW>(st01, d5[i][1], i, 1);
        }
    }
    // LabRef of the item's 2 x 4 pixels, in flight across the barrier
    float4 lab[2][3];
    uint32_t mk[2];  // MSK: the mask bytes of each row's 4 pixels, one dword at the LabRef offset
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        bool ok = gy0 + r < g.r1 && gx0 < g.W;
        if constexpr (DE == 2) ok = ok && gy0 + r >= g.r0;
        const uint32_t off = ok ? (uint32_t)((gy0 + r - g.r0) * g.lab_pitch + gx0) : 0u;
        if constexpr (MSK != 0) mk[r] = *reinterpret_cast<const uint32_t*>(a.mask + off);
#ifdef HQ_ABL_NOLABLD  // timing ablation (wrong results): no LabRef loads
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) lab[r][ch] = make_float4(off, off + 1, off + ch, r);
#else
        const float* src3[3] = {a.labL, a.labA, a.labB};
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float4* lp =
                reinterpret_cast<const float4*>(reinterpret_cast<const char*>(src3[ch]) + (off << 2));  // 32-bit byte offset
#if HQ_LAB_NT
            const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(lp));
            lab[r][ch] = make_float4(v.x, v.y, v.z, v.w);
#else
            lab[r][ch] = *lp;
#endif
        }
#endif
    }
    __syncthreads();
    if constexpr (TRIM) hpass_wide<HB, L2, T2 - L2, WH>(hsrc, jr, taps, 5, 0, PLANE4, acc2);
    else hpass_wide<HB, 0, T2, WH>(hsrc, jr, taps, 5, 0, PLANE4, acc2);
    hpass_wide<HB, 0, T2, WH>(hsrc, jr, taps, 6, 1, PLANE4, acc2);

    float e[2][HR];
#if HQ_LAB_SKIPLIN
    // t = X/Xn, Y/Yn, Z/Zn of the item's 8 pixels; when no t of the wave is in
    // the linear Lab segment (t <= delta^3: near-black filtered colours, rare),
    // the cube roots alone (lab_f_root), else lab_f_fast's select (same values)
    float3 tf[2][HR];
    float tmin = INFINITY;
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int xo = 0; xo < HR; ++xo) {
            const float o0 = acc0[xo][r], o1 = acc1[xo][r], o2 = acc2[xo][r];
            tf[r][xo] = make_float3(dot3(o0, o1, o2, a.m_lab + 0), dot3(o0, o1, o2, a.m_lab + 3),
                                    dot3(o0, o1, o2, a.m_lab + 6));
            tmin = fminf(tmin, fminf(tf[r][xo].x, fminf(tf[r][xo].y, tf[r][xo].z)));  // (v_min3; a NaN t drops out)
        }
    if (__builtin_amdgcn_ballot_w64(!(tmin > LAB_DELTA3)) == 0) {
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int xo = 0; xo < HR; ++xo)
                tf[r][xo] = make_float3(lab_f_root(tf[r][xo].x), lab_f_root(tf[r][xo].y), lab_f_root(tf[r][xo].z));
    } else {
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int xo = 0; xo < HR; ++xo)
                tf[r][xo] = make_float3(lab_f_fast(tf[r][xo].x), lab_f_fast(tf[r][xo].y), lab_f_fast(tf[r][xo].z));
    }
#endif
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const float Ls[4] = {lab[r][0].x, lab[r][0].y, lab[r][0].z, lab[r][0].w};
        const float As[4] = {lab[r][1].x, lab[r][1].y, lab[r][1].z, lab[r][1].w};
        const float Bs[4] = {lab[r][2].x, lab[r][2].y, lab[r][2].z, lab[r][2].w};
#pragma unroll
        for (int xo = 0; xo < HR; ++xo) {
#ifdef HQ_ABL_NOLAB  // timing ablation (wrong results): no Opp->Lab / dE
            e[r][xo] = (acc0[xo][r] + acc1[xo][r]) + (acc2[xo][r] + (Ls[xo] + As[xo] + Bs[xo]));
#elif HQ_LAB_SKIPLIN
            e[r][xo] = delta_e_f<DE>(Ls[xo], As[xo], Bs[xo], tf[r][xo]);
#else
            const float3 lf = opp2f_fast(acc0[xo][r], acc1[xo][r], acc2[xo][r], a.m_lab);
            e[r][xo] = delta_e_f<DE>(Ls[xo], As[xo], Bs[xo], lf);
#endif
        }
    }
    if (a.pix_err) {  // test option: the per-pixel dE (CL:201-209's error image)
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if constexpr (DE == 2) {
                if (gy0 + r < g.r0) continue;
            }
#pragma unroll
            for (int xo = 0; xo < HR; ++xo)
                if (gy0 + r < g.r1 && gx0 + xo < g.W)
                    a.pix_err[(int64_t)cur.p * a.pix_pitch + (int64_t)(gy0 + r - g.r0) * g.W + gx0 + xo] =
                        e[r][xo];
        }
    }
    // tiles inside the image and shard (all but the last tile column and row)
    // sum without per-pixel masks
    float part = 0.f;
    if constexpr (MSK == 2) {  // pixel weights: the masked form's pixels in its order, each by one fma with its
                               // weight (w = 1: fma(e, 1, part) = part + e, the masked bits); weight 0 is the
                               // select, so a NaN of such a pixel stays out of the sum
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int xo = 0; xo < HR; ++xo) {
                const uint32_t wb = (mk[r] >> (8 * xo)) & 0xffu;
                bool in = gy0 + r < g.r1 && gx0 + xo < g.W && wb != 0u;
                if constexpr (DE == 2) in = in && gy0 + r >= g.r0;
                part = in ? fmaf(e[r][xo], (float)wb, part) : part;
            }
    } else
    if constexpr (MSK == 1) {  // every tile with per-pixel selects, in the plain forms' order of additions: an
                          // all-ones mask gives their bits, a masked-out NaN stays out of the sum
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int xo = 0; xo < HR; ++xo) {
                bool in = gy0 + r < g.r1 && gx0 + xo < g.W && ((mk[r] >> (8 * xo)) & 0xffu) != 0u;
                if constexpr (DE == 2) in = in && gy0 + r >= g.r0;
                part += in ? e[r][xo] : 0.f;
            }
    } else
    if constexpr (DE == 2) {  // the same, and a shard's first tile row masks its rows above r0
        if (cur.x0 + TW <= g.W && cur.y0 + TH <= g.r1 && cur.y0 >= g.r0) {
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int xo = 0; xo < HR; ++xo) part += e[r][xo];
        } else {
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int xo = 0; xo < HR; ++xo)
                    part += (gy0 + r >= g.r0 && gy0 + r < g.r1 && gx0 + xo < g.W) ? e[r][xo] : 0.f;
        }
    } else  // (dE76, dE94: the statement as it was, unindented on purpose)
    if (cur.x0 + TW <= g.W && cur.y0 + TH <= g.r1) {
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int xo = 0; xo < HR; ++xo) part += e[r][xo];
    } else {
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int xo = 0; xo < HR; ++xo) part += (gy0 + r < g.r1 && gx0 + xo < g.W) ? e[r][xo] : 0.f;
    }
#ifdef HQ_ABL_NORED  // timing ablation (wrong results): no reduction / accumulation
    if (part == 12345.f) a.acc[tid] = 1;
#else
    // each wave adds its own partial: the fixed-point sum is order-free, so no
    // end-of-tile barrier and LDS fold (that form: cost 0.3522 against 0.3499 ms)
    const double sum = wave_sum_to_lane63((double)part);
    if (lane == 63) acc_add(a.acc, a.acc_P, a.acc_p0 + cur.p, cur.tile * NW + wv, sum);
#endif
}

// ---- host side: the fast path's launchers (its tables: hq_cost_taps.cpp) ----
// This file is compiled three times: as it is (the plain instances and launchers),
// through hq_cost_masked.hip with HQ_COST_MASKED defined (the MSK = 1 instances and
// launch_cost_fast_masked / launch_cost_chunked_masked) and through
// hq_cost_weighted.hip with HQ_COST_WEIGHTED defined (MSK = 2,
// launch_cost_fast_weighted / launch_cost_chunked_weighted), so the sets build
// side by side and the plain set's source is what it was.
#if defined(HQ_COST_WEIGHTED)
constexpr bool kMasked = true;  // (the launch covers the live tiles)
constexpr int kMsk = 2;
#define HQ_COST_LAUNCHER(name) name##_weighted
#elif defined(HQ_COST_MASKED)
constexpr bool kMasked = true;
constexpr int kMsk = 1;
#define HQ_COST_LAUNCHER(name) name##_masked
#else
constexpr bool kMasked = false;
constexpr int kMsk = 0;
#define HQ_COST_LAUNCHER(name) name
// The two CostTaps<HB> of build_fast_taps.
size_t fast_taps_bytes(int HB) { return 2 * 2 * sizeof(float) * kNumFilt * (2 * HB + 1); }
static_assert(2 * sizeof(CostTaps<24>) == 2 * 2 * sizeof(float) * kNumFilt * 49, "CostTaps: two float [7][2 HB + 1]");

// tile_rows: 8 (cost_mfma_kernel, 8 x 108 tiles) or 16 (cost16w_kernel, 16 x
// tile_w tiles, tile_w = 128 or 256)
// First row of a shard's tile grid (tile_item): r0, or for dE2000 the image's
// tile row that holds r0.  own_rows of fast_tile_dims counts from it.
int fast_grid_row0(int de, int r0, int tile_rows) { return de == 2 ? r0 & ~(tile_rows - 1) : r0; }

int fast_tile_width(int tile_rows, int tile_w) { return tile_rows == kTH16 ? tile_w : kFastTW; }

void fast_tile_dims(int W, int own_rows, int tile_rows, int tile_w, int* tiles_x, int* ntiles) {
    const int tw = fast_tile_width(tile_rows, tile_w);
    *tiles_x = (W + tw - 1) / tw;
    *ntiles = *tiles_x * ((own_rows + tile_rows - 1) / tile_rows);
}
#endif

// a.taps = the two CostTaps<HB> of build_fast_taps; [1], which the kernels
// here read, carries the vertical pass's 2^30 scale in its horizontal taps.
// NCH > 1: chunked palettes (NCH chunks of 256 colours, 16-bit indices); the
// table takes 8 * 256 NCH bytes of dynamic LDS, above 64 KB in all at NCH 16.
template <int HB, int NW, int NCH = 1>
static void launch_cost16w(const CostArgs& a0, int P, int de, bool trim, hipStream_t s, CostTag* tag) {
    CostArgs a = a0;
    a.taps = static_cast<const char*>(a0.taps) + sizeof(CostTaps<HB>);
    const dim3 grid((unsigned)((kMasked ? a.nlive : a.ntiles) * P)), block(64 * NW);
    with_de(de, [&](auto DE) {
        with_bool(trim, [&](auto TRIM) {
            constexpr auto kern = cost16w_kernel<HB, DE.value, TRIM.value, NW, NCH, kMsk>;
            if constexpr (NCH > 1) HQ_LAUNCH_DYN_LDS(kern, grid, block, 8 * (size_t)kMaxK * NCH, s, a, P);
            else HQ_LAUNCH(kern, grid, block, 0, s, a, P);
            if (tag) *tag = CostTag{1, HB, DE.value, TRIM.value, NW, NCH, kMsk};
        });
    });
}

hipError_t HQ_COST_LAUNCHER(launch_cost_chunked)(const CostArgs& a, int P, int nch, int de, bool trim, hipStream_t s,
                                                 CostTag* tag) {
    if (!known_de(de) || (kMasked && (!a.mask || !a.live || a.nlive < 1))) return hipErrorInvalidValue;
    switch (nch) {
    case 2: launch_cost16w<10, 4, 2>(a, P, de, trim, s, tag); break;
    case 4: launch_cost16w<10, 4, 4>(a, P, de, trim, s, tag); break;
    case 8: launch_cost16w<10, 4, 8>(a, P, de, trim, s, tag); break;
    case 16: launch_cost16w<10, 4, 16>(a, P, de, trim, s, tag); break;
    case 32: launch_cost16w<10, 4, 32>(a, P, de, trim, s, tag); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// 256-column tiles (8 waves, 69 KB of LDS at HB = 10) and 8-row tiles: HB = 10 only.
hipError_t HQ_COST_LAUNCHER(launch_cost_fast)(const CostArgs& a0, int P, int de, bool trim, int tile_rows, int tile_w,
                                              int HB, hipStream_t s, CostTag* tag) {
    if (!known_de(de) || (HB != 10 && (tile_rows != kTH16 || tile_w == 256))) return hipErrorInvalidValue;
    if (kMasked && (!a0.mask || !a0.live || a0.nlive < 1)) return hipErrorInvalidValue;
    if (tile_rows == kTH16 && tile_w == 256) {
        launch_cost16w<10, 8>(a0, P, de, trim, s, tag);
    } else if (tile_rows == kTH16) {
        switch (HB) {
        case kFastBuckets[0]: launch_cost16w<kFastBuckets[0], 4>(a0, P, de, trim, s, tag); break;
        case kFastBuckets[1]: launch_cost16w<kFastBuckets[1], 4>(a0, P, de, trim, s, tag); break;
        case kFastBuckets[2]: launch_cost16w<kFastBuckets[2], 4>(a0, P, de, trim, s, tag); break;
        case kFastBuckets[3]: launch_cost16w<kFastBuckets[3], 4>(a0, P, de, trim, s, tag); break;
        default: return hipErrorInvalidValue;
        }
    } else {
        CostArgs a = a0;
        a.taps = static_cast<const char*>(a0.taps) + sizeof(CostTaps<10>);
        const dim3 grid((unsigned)((kMasked ? a.nlive : a.ntiles) * P));
        with_de(de, [&](auto DE) {
            with_bool(trim, [&](auto TRIM) {
                HQ_LAUNCH((cost_mfma_kernel<DE.value, TRIM.value, kMsk>), grid, dim3(256), 0, s, a, P);
                if (tag) *tag = CostTag{2, 10, DE.value, TRIM.value, 4, 1, kMsk};
            });
        });
    }
    return hipGetLastError();
}

}  // namespace hq
