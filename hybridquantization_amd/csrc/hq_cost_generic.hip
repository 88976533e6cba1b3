// hq_cost_generic.hip -- the S-CIELAB cost of one palette at any filter
// half-width, one launch pair per palette.  First the plain pair (option
// cost_variant 1): the reference's computeScielabKernelsTemp (CL:234-272) and
// computeScielabKernelsEnd (CL:274-306) restated per pixel through a
// [7][n_ext] fp32 scratch; it cross-checks the fast path (hq_cost.hip) in the
// tests.  Then the tiled forms that filters longer than 24 taps a side run on.
#include "hq_device.h"
#include "hq_launch.h"

namespace hq {

template <typename IT>
__global__ __launch_bounds__(256) void gen_hpass_kernel(GenArgs a) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= a.g.n_ext) return;
    const int ly = (int)(q / a.g.W), x = (int)(q % a.g.W);
    const IT* row = static_cast<const IT*>(a.idx) + (int64_t)ly * a.g.W;
    float t1x = 0, t1y = 0, t1z = 0, t2x = 0, t2y = 0, t2z = 0, t3 = 0;
    for (int i = -a.half, t = 0; i <= a.half; ++i, ++t) {  // CL:254-267
        const float4 in = a.opp[row[reflect_only(x + i, a.g.W)]];
        t1x = fmaf(in.x, a.k1[4 * t + 0], t1x);
        t1y = fmaf(in.y, a.k1[4 * t + 1], t1y);
        t1z = fmaf(in.z, a.k1[4 * t + 2], t1z);
        t2x = fmaf(in.x, a.k2[4 * t + 0], t2x);
        t2y = fmaf(in.y, a.k2[4 * t + 1], t2y);
        t2z = fmaf(in.z, a.k2[4 * t + 2], t2z);
        t3 = fmaf(in.x, a.k3[t], t3);
    }
    const int64_t n = a.g.n_ext;
    a.t[q] = t1x; a.t[n + q] = t1y; a.t[2 * n + q] = t1z;
    a.t[3 * n + q] = t2x; a.t[4 * n + q] = t2y; a.t[5 * n + q] = t2z;
    a.t[6 * n + q] = t3;
}

template <int DE>
__global__ __launch_bounds__(256) void gen_vpass_kernel(GenArgs a) {
    __shared__ double s_red[4];
    const int own_w = a.g.W;
    const int64_t n_own = (int64_t)own_w * (a.g.r1 - a.g.r0);
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double e = 0.0;
    if (q < n_own) {
        const int y = a.g.r0 + (int)(q / own_w), x = (int)(q % own_w);
        const int64_t n = a.g.n_ext;
        float ox = 0, oy = 0, oz = 0;
        for (int i = -a.half, t = 0; i <= a.half; ++i, ++t) {  // CL:292-304
            const int64_t s = (int64_t)(reflect_only(y + i, a.g.H) - a.g.e0) * a.g.W + x;
            ox = fmaf(a.t[s], a.k1[4 * t + 0], fmaf(a.t[3 * n + s], a.k2[4 * t + 0], ox));
            oy = fmaf(a.t[n + s], a.k1[4 * t + 1], fmaf(a.t[4 * n + s], a.k2[4 * t + 1], oy));
            oz = fmaf(a.t[2 * n + s], a.k1[4 * t + 2], fmaf(a.t[5 * n + s], a.k2[4 * t + 2], oz));
            ox = fmaf(a.t[6 * n + s], a.absk3[t], ox);
        }
        const float3 lf = opp2f_fast(ox, oy, oz, a.m_lab);
        const int64_t off = (int64_t)(y - a.g.r0) * a.g.lab_pitch + x;
        const float ef = delta_e_f<DE>(a.labL[off], a.labA[off], a.labB[off], lf);
        if (a.pix_err) a.pix_err[q] = ef;  // test option: the per-pixel dE
        // pixel mask or weights: dE times the byte (a mask's: 0 / 1), an exact double product; a
        // zero byte is a select, so a masked-out NaN stays out
        const double wgt = a.mask ? (double)a.mask[off] : 1.0;
        e = wgt != 0.0 ? (double)ef * wgt : 0.0;
    }
    e = wave_sum(e);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = e;
    __syncthreads();
    if (threadIdx.x == 0) acc_add(a.acc, a.P, a.p, blockIdx.x, (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]));
}

// ----------------------------------------------------------------------------
// Tiled generic path (any half-width; the default generic path since round 4,
// and the one half > 24 -- e.g. 300 dpi at 50 cm, half 51 -- takes).  The same
// two passes and the same [7][n_ext] scratch as gen_hpass / gen_vpass, staged
// through LDS so each input feeds many outputs from LDS instead of L1/L2:
// - gen_hrow: grid (ceil(W / 256), extended rows), block 256.  The opponent
//   colours of the row segment x0 - half .. x0 + 255 + half (reflected,
//   CL:256-263) land in LDS once (a float4 each); output x then reads one
//   float4 per tap for its 7 FMAs, in the reference's tap order (CL:254-267).
//   (gen_hpass gathered index and table entry per tap: 2 (2 half + 1) L1 reads.)
// - gen_vtile: grid (64 x 64 output tiles of the owned rows), block 256.  For
//   each filter (plane t1.xyz, t2.xyz, t3 with vertical taps k1.xyz, k2.xyz,
//   |k3|), rows y0 - half .. y0 + 63 + half of the tile's 64 columns land in LDS;
//   thread (column c, row block rb) owns output rows 16 rb .. 16 rb + 15 and runs
//   the taps in chunks of 16: 32 window values from LDS and 16 taps (scalar
//   loads, zero-padded to a multiple of 16) make 256 FMAs.  The filters are
//   summed one after another (the reference interleaves them per tap): the
//   fp32 rounding differs, as in the fast path (1e-6 relative on costs).  Then
//   Opp->Lab, dE and the tile's fixed-point partial.  (gen_vpass read 7 (2 half
//   + 1) floats per output from L2: 2.9 KB at half 51.)
// ----------------------------------------------------------------------------
template <typename IT>
__global__ __launch_bounds__(256) void gen_hrow_kernel(GenArgs a) {
    extern __shared__ float4 s_opp[];  // [256 + 2 half]
    const int tid = threadIdx.x, half = a.half, W = a.g.W;
    const int x0 = blockIdx.x * 256, ly = blockIdx.y;
    const IT* row = static_cast<const IT*>(a.idx) + (int64_t)ly * W;
    for (int e = tid; e < 256 + 2 * half; e += 256) {
        const int x = min(x0 - half + e, W - 1 + half);  // (past the row end: reflected, unused)
        s_opp[e] = a.opp[row[reflect_only(x, W)]];
    }
    __syncthreads();
    const int x = x0 + tid;
    if (x >= W) return;
    float t1x = 0, t1y = 0, t1z = 0, t2x = 0, t2y = 0, t2z = 0, t3 = 0;
    for (int t = 0; t <= 2 * half; ++t) {  // CL:254-267
        const float4 in = s_opp[tid + t];
        t1x = fmaf(in.x, a.k1[4 * t + 0], t1x);
        t1y = fmaf(in.y, a.k1[4 * t + 1], t1y);
        t1z = fmaf(in.z, a.k1[4 * t + 2], t1z);
        t2x = fmaf(in.x, a.k2[4 * t + 0], t2x);
        t2y = fmaf(in.y, a.k2[4 * t + 1], t2y);
        t2z = fmaf(in.z, a.k2[4 * t + 2], t2z);
        t3 = fmaf(in.x, a.k3[t], t3);
    }
    const int64_t n = a.g.n_ext, q = (int64_t)ly * W + x;
    a.t[q] = t1x; a.t[n + q] = t1y; a.t[2 * n + q] = t1z;
    a.t[3 * n + q] = t2x; a.t[4 * n + q] = t2y; a.t[5 * n + q] = t2z;
    a.t[6 * n + q] = t3;
}

// gen_hrow4: the same horizontal pass with 4 adjacent outputs per thread
// (grid (ceil(W / 1024), rows), block 256): a thread slides a window of 7
// colours over its taps in chunks of 4 -- 4 new ds_read_b128 per 4 taps and
// 112 FMAs, against 4 reads per 28 FMAs above, which left gen_hrow bound by
// the LDS reads at large half-widths.  The row segment sits in LDS permuted
// (element e at slot (e & 3) Q + e / 4), so the 64 lanes of a read hit
// consecutive slots.  Each output sums its taps in ascending order (CL:254-
// 267), so the planes equal gen_hrow's bit for bit.
// NO adjacent outputs per thread (4 or 8: option gen_hrow_outputs), a row
// segment of 256 NO outputs per workgroup; element e of the segment sits at
// slot (e % NO) Q + e / NO, so a read's 64 lanes hit consecutive slots.
template <typename IT, bool SPLIT, int NO>
__global__ __launch_bounds__(256) void gen_hrow4_kernel(GenArgs a) {
    extern __shared__ float4 s_opp[];  // [NO][Q] permuted
    constexpr int SEG = 256 * NO, NW = NO + 3;  // window: NO outputs x a chunk of 4 taps
    const int tid = threadIdx.x, half = a.half, W = a.g.W, T = 2 * half + 1;
    const int x0 = blockIdx.x * SEG, ly = blockIdx.y;
    const int Q = (SEG + 2 * half + 3 + NO - 1) / NO;
    const IT* row = static_cast<const IT*>(a.idx) + (int64_t)ly * W;
    // the segment's colours, 8 per thread and batch: every index load of a batch
    // first, then every table load, then the stores (one dependent pair of round
    // trips per batch; a load -> load -> store loop paid two per element)
    for (int e0 = 0; e0 < NO * Q; e0 += 8 * 256) {
        uint32_t ix[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int e = min(e0 + tid + 256 * u, NO * Q - 1);
            const int x = min(x0 - half + e, W - 1 + half);  // (past the row end: reflected, unused)
            ix[u] = (uint32_t)row[reflect_only(x, W)];
        }
        float4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = a.opp[ix[u]];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int e = e0 + tid + 256 * u;
            if (e < NO * Q) s_opp[(e % NO) * Q + e / NO] = v[u];
        }
    }
    __syncthreads();
    float acc[7][NO];
#pragma unroll
    for (int f = 0; f < 7; ++f)
#pragma unroll
        for (int xo = 0; xo < NO; ++xo) acc[f][xo] = 0.f;
    // window w[i] = element NO tid + t0 + i of the segment, i = 0 .. NO + 2
    auto rd = [&](int e) { return s_opp[(e % NO) * Q + e / NO]; };
    float4 w[NW];
#pragma unroll
    for (int i = 0; i < NO - 1; ++i) w[i] = rd(NO * tid + i);
    // taps t: ka = (k1.xyz, k3), kb = (k2.xyz, 0) (a.htaps, packed on the host: a
    // chunk's 4 taps are 2 wide scalar loads, not 7 per tap)
    auto taps_fma = [&](int d, float4 ka, float4 kb) {
#pragma unroll
        for (int xo = 0; xo < NO; ++xo) {
            const float4 in = w[d + xo];
            acc[0][xo] = fmaf(in.x, ka.x, acc[0][xo]);
            acc[1][xo] = fmaf(in.y, ka.y, acc[1][xo]);
            acc[2][xo] = fmaf(in.z, ka.z, acc[2][xo]);
            acc[3][xo] = fmaf(in.x, kb.x, acc[3][xo]);
            acc[4][xo] = fmaf(in.y, kb.y, acc[4][xo]);
            acc[5][xo] = fmaf(in.z, kb.z, acc[5][xo]);
            acc[6][xo] = fmaf(in.x, ka.w, acc[6][xo]);
        }
    };
    const float4* tp = a.htaps;
    int t0 = 0;
    for (; t0 + 4 <= T; t0 += 4) {  // whole chunks
#pragma unroll
        for (int i = NO - 1; i < NW; ++i) w[i] = rd(NO * tid + t0 + i);
#pragma unroll
        for (int d = 0; d < 4; ++d) taps_fma(d, tp[2 * (t0 + d)], tp[2 * (t0 + d) + 1]);
#pragma unroll
        for (int i = 0; i < NO - 1; ++i) w[i] = w[i + 4];
    }
    if (t0 < T) {  // the last taps: guarded (a tap past T is not a zero product on a non-finite colour)
#pragma unroll
        for (int i = NO - 1; i < NW; ++i) w[i] = rd(NO * tid + t0 + i);
#pragma unroll
        for (int d = 0; d < 3; ++d)
            if (t0 + d < T) taps_fma(d, tp[2 * (t0 + d)], tp[2 * (t0 + d) + 1]);
    }
    const int64_t n = a.g.n_ext, q0 = (int64_t)ly * W + x0 + NO * tid;
    const bool whole = (W & 3) == 0 && x0 + NO * tid + NO - 1 < W;  // (planes of n_ext = W rows: 16-B aligned)
    if constexpr (SPLIT) {  // planes of (hi, lo) f16 pairs of x 2^14 for the matrix-core vertical pass
        uint32_t* t = reinterpret_cast<uint32_t*>(a.t);
        if (whole) {
#pragma unroll
            for (int f = 0; f < 7; ++f)
#pragma unroll
                for (int v = 0; v < NO; v += 4)
                    *reinterpret_cast<uint4*>(t + f * n + q0 + v) =
                        make_uint4(split_f16(acc[f][v]), split_f16(acc[f][v + 1]), split_f16(acc[f][v + 2]),
                                   split_f16(acc[f][v + 3]));
        } else {
#pragma unroll
            for (int xo = 0; xo < NO; ++xo)
                if (x0 + NO * tid + xo < W)
#pragma unroll
                    for (int f = 0; f < 7; ++f) t[f * n + q0 + xo] = split_f16(acc[f][xo]);
        }
        return;
    }
    if (whole) {
#pragma unroll
        for (int f = 0; f < 7; ++f)
#pragma unroll
            for (int v = 0; v < NO; v += 4)
                *reinterpret_cast<float4*>(a.t + f * n + q0 + v) =
                    make_float4(acc[f][v], acc[f][v + 1], acc[f][v + 2], acc[f][v + 3]);
    } else {
#pragma unroll
        for (int xo = 0; xo < NO; ++xo)
            if (x0 + NO * tid + xo < W)
#pragma unroll
                for (int f = 0; f < 7; ++f) a.t[f * n + q0 + xo] = acc[f][xo];
    }
}

constexpr int kVtTile = 64, kVtRows = 16;  // gen_vtile: 64 x 64 tiles, 16 output rows per thread
template <int DE>
__global__ __launch_bounds__(256) void gen_vtile_kernel(GenArgs a, int tiles_x) {
    extern __shared__ float s_win[];  // [64 + 2 half][64]
    constexpr int TW = kVtTile, RB = kVtRows;
    __shared__ double s_red[4];
    const int tid = threadIdx.x, c = tid & (TW - 1), rb = tid >> 6;
    const Geom& g = a.g;
    const int x0 = (blockIdx.x % tiles_x) * TW, y0 = g.r0 + (blockIdx.x / tiles_x) * TW;
    const int half = a.half, RH = TW + 2 * half, T = 2 * half + 1;
    const int64_t n = g.n_ext;
    float acc[3][RB];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
#pragma unroll
        for (int j = 0; j < RB; ++j) acc[ch][j] = 0.f;
    for (int f = 0; f < kNumFilt; ++f) {
        const float* plane = a.t + (int64_t)f * n;
        const float* vt = a.vtaps + f * a.vtap_pitch;  // zero-padded to a multiple of 16
        __syncthreads();  // (the previous filter's window reads)
        // the window rows, 16 loads per thread in flight per batch (a load ->
        // store loop paid one memory round trip per element: ~42 per filter at
        // half 51, most of the kernel's time)
        const int jx = min(x0 + (tid & (TW - 1)), g.W - 1);
        for (int e0 = 0; e0 < RH * TW; e0 += 16 * 256) {
            float v[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int i = min(e0 + tid + 256 * u, RH * TW - 1) / TW;  // (clamped: loaded, not stored)
                int gy = reflect_clamp(y0 - half + i, g.H);
                gy = min(max(gy, g.e0), g.e1 - 1);
                v[u] = plane[(int64_t)(gy - g.e0) * g.W + jx];
            }
#pragma unroll
            for (int u = 0; u < 16; ++u)
                if (e0 + tid + 256 * u < RH * TW) s_win[e0 + tid + 256 * u] = v[u];
        }
        __syncthreads();
        float o[RB];
#pragma unroll
        for (int j = 0; j < RB; ++j) o[j] = 0.f;
        for (int k0 = 0; k0 < T; k0 += 16) {
            float v[RB + 16];
#pragma unroll
            for (int i = 0; i < RB + 16; ++i) v[i] = s_win[min(RB * rb + k0 + i, RH - 1) * TW + c];
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) {
                const float w = vt[k0 + kk];
#pragma unroll
                for (int j = 0; j < RB; ++j) o[j] = fmaf(v[j + kk], w, o[j]);
            }
        }
        // planes: 0 t1.x, 1 t1.y, 2 t1.z, 3 t2.x, 4 t2.y, 5 t2.z, 6 t3 -> channels x y z x y z x
        const int chp = f == 6 ? 0 : f % 3;
#pragma unroll
        for (int j = 0; j < RB; ++j) {
            if (chp == 0) acc[0][j] += o[j];
            else if (chp == 1) acc[1][j] += o[j];
            else acc[2][j] += o[j];
        }
    }
    double part = 0.0;
    const int gx = x0 + c;
#pragma unroll
    for (int j = 0; j < RB; ++j) {
        const int y = y0 + RB * rb + j;
        if (gx < g.W && y < g.r1) {
            const float3 lf = opp2f_fast(acc[0][j], acc[1][j], acc[2][j], a.m_lab);
            const int64_t off = (int64_t)(y - g.r0) * g.lab_pitch + gx;
            const float ef = delta_e_f<DE>(a.labL[off], a.labA[off], a.labB[off], lf);
            if (a.pix_err) a.pix_err[(int64_t)(y - g.r0) * g.W + gx] = ef;  // test option: the per-pixel dE
            const double wgt = a.mask ? (double)a.mask[off] : 1.0;  // pixel mask or weights (gen_vpass)
            part += wgt != 0.0 ? (double)ef * wgt : 0.0;
        }
    }
    part = wave_sum_to_lane63(part);
    if ((tid & 63) == 63) s_red[tid >> 6] = part;
    __syncthreads();
    if (tid == 0) acc_add(a.acc, a.P, a.p, blockIdx.x, (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]));
}

// gen_vtile2: the vertical pass on 32 x 64 output tiles (half <= kVt2MaxHalf)
// with the filters' windows double-buffered in LDS and filled by LDS DMA
// (global_load_lds_dword: no registers held): filter f + 1's window streams in
// while filter f's taps run, so the fill's memory round trips hide behind the
// FMAs (gen_vtile waits for each window between two barriers).  Thread
// (column c = tid % 32, row block rb = tid / 32) owns output rows 8 rb .. 8 rb
// + 7.  Element e of a window is row e / 32, column e % 32 -- a wave's DMA
// instruction writes 64 consecutive LDS dwords, two window rows.  Same sums
// in the same order as gen_vtile (filters one after another, each filter's
// taps in chunks of 16), so every pixel's dE is bit-identical (the fixed-point
// sums round per tile, and the tiles differ: 2^-20 per partial).
// One filter's window (rows y0 - half .. of the tile's 32 columns, NE = RH x 32
// dwords) from a [n_ext] plane into LDS by DMA.  An image width that is a
// multiple of 4 makes every row segment 16-B aligned: global_load_lds_dwordx4,
// 1 KiB per wave instruction (a lane's 4 dwords: row e4 / 8, columns 4 (e4 % 8)
// .. + 3; the last tile column reads up to 31 elements past its row, which stay
// inside the planes' 256-B tail pad and feed only masked output columns);
// otherwise one dword per lane, columns clamped.  (Dword DMA is 4x the
// instructions, and their issue held the vertical pass.)
template <typename T>
__device__ __forceinline__ void dma_window(const T* plane, T* dst, int NE, int tid, int wv, const Geom& g, int x0,
                                           int y0, int half, bool rows_inside, bool wide) {
    auto row_off = [&](int i) -> uint32_t {
        int gy = y0 - half + i;
        if (!rows_inside) {
            gy = reflect_clamp(gy, g.H);
            gy = min(max(gy, g.e0), g.e1 - 1);
        }
        return (uint32_t)((gy - g.e0) * g.W);
    };
    if (wide) {
        const int NE4 = NE >> 2;
        for (int e0 = 0; e0 < NE4; e0 += 256) {
            const int e = e0 + tid;
            if (e < NE4) {
                const T* src = plane + row_off(e >> 3) + (uint32_t)(x0 + 4 * (e & 7));
                __builtin_amdgcn_global_load_lds(src, (__attribute__((address_space(3))) void*)(dst + 4 * (e0 + 64 * wv)),
                                                 16, 0, 0);
            }
        }
    } else {
        const int jx = min(x0 + (tid & 31), g.W - 1);
        for (int e0 = 0; e0 < NE; e0 += 256) {
            const int e = e0 + tid;
            if (e < NE) {
                const T* src = plane + row_off(e >> 5) + (uint32_t)jx;
                __builtin_amdgcn_global_load_lds(src, (__attribute__((address_space(3))) void*)(dst + e0 + 64 * wv), 4, 0, 0);
            }
        }
    }
}

constexpr int kVt2W = 32, kVt2MaxHalf = 64;
#ifndef HQ_VT2_RB
#define HQ_VT2_RB 8  // gen_vtile2: output rows per thread, tiles of 32 x 8 RB (16: 3.677 vs 3.619 ms at 300/50)
#endif
template <int DE, int RB>
__global__ __launch_bounds__(256) void gen_vtile2_kernel(GenArgs a, int tiles_x) {
    extern __shared__ float s_w2[];  // [2][8 RB + 2 half][32]
    constexpr int TW = kVt2W, kVt2H = 8 * RB;
    __shared__ double s_red[4];
    const int tid = threadIdx.x, c = tid & (TW - 1), rb = tid >> 5;
    const Geom& g = a.g;
    const int x0 = (blockIdx.x % tiles_x) * TW, y0 = g.r0 + (blockIdx.x / tiles_x) * kVt2H;
    const int half = a.half, RH = kVt2H + 2 * half, T = 2 * half + 1, NE = RH * TW;
    const int64_t n = g.n_ext;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool rows_inside = y0 - half >= g.e0 && y0 - half >= 0 && y0 + kVt2H + half <= g.e1 && y0 + kVt2H + half <= g.H;
    const bool wide = (g.W & 3) == 0;
    auto issue = [&](int f, int b) {
        dma_window(a.t + (int64_t)f * n, s_w2 + b * NE, NE, tid, wv, g, x0, y0, half, rows_inside, wide);
    };
    float acc[3][RB];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
#pragma unroll
        for (int j = 0; j < RB; ++j) acc[ch][j] = 0.f;
    issue(0, 0);
    for (int f = 0; f < kNumFilt; ++f) {
        __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): this wave's rows of window f have landed
        __syncthreads();                     // every wave's rows; window f - 1's readers are done
        if (f + 1 < kNumFilt) issue(f + 1, (f + 1) & 1);
        const float* win = s_w2 + (f & 1) * NE;
        const float* vt = a.vtaps + f * a.vtap_pitch;  // zero-padded to a multiple of 16
        float o[RB];
#pragma unroll
        for (int j = 0; j < RB; ++j) o[j] = 0.f;
        for (int k0 = 0; k0 < T; k0 += 16) {
            float v[RB + 16];
#pragma unroll
            for (int i = 0; i < RB + 16; ++i) v[i] = win[min(RB * rb + k0 + i, RH - 1) * TW + c];
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) {
                const float w = vt[k0 + kk];
#pragma unroll
                for (int j = 0; j < RB; ++j) o[j] = fmaf(v[j + kk], w, o[j]);
            }
        }
        const int chp = f == 6 ? 0 : f % 3;  // planes t1.xyz, t2.xyz, t3 -> channels x y z x y z x
#pragma unroll
        for (int j = 0; j < RB; ++j) {
            if (chp == 0) acc[0][j] += o[j];
            else if (chp == 1) acc[1][j] += o[j];
            else acc[2][j] += o[j];
        }
    }
    double part = 0.0;
    const int gx = x0 + c;
#pragma unroll
    for (int j = 0; j < RB; ++j) {
        const int y = y0 + RB * rb + j;
        if (gx < g.W && y < g.r1) {
            const float3 lf = opp2f_fast(acc[0][j], acc[1][j], acc[2][j], a.m_lab);
            const int64_t off = (int64_t)(y - g.r0) * g.lab_pitch + gx;
            const float ef = delta_e_f<DE>(a.labL[off], a.labA[off], a.labB[off], lf);
            if (a.pix_err) a.pix_err[(int64_t)(y - g.r0) * g.W + gx] = ef;  // test option: the per-pixel dE
            const double wgt = a.mask ? (double)a.mask[off] : 1.0;  // pixel mask or weights (gen_vpass)
            part += wgt != 0.0 ? (double)ef * wgt : 0.0;
        }
    }
    part = wave_sum_to_lane63(part);
    if ((tid & 63) == 63) s_red[tid >> 6] = part;
    __syncthreads();
    if (tid == 0) acc_add(a.acc, a.P, a.p, blockIdx.x, (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]));
}

// gen_vmfma: the tiled generic path's vertical pass on the matrix cores
// (half <= kVt2MaxHalf), the split-f16 (hi, lo) pair scheme of cost16w's wide
// buckets: gen_hrow4<SPLIT> writes each plane value x as the dword (hi, lo) of
// x 2^14 (split_f16), which is two K slots of the B operand as it stands; A
// holds the vertical taps x 2^16 split on the host, each tap part in both
// slots of a row (build_vtile_dup_taps, read from LDS), the hi parts in one MFMA and
// the lo parts in the next: (t_hi + t_lo)(x_hi + x_lo), every product exact in
// the fp32 accumulator.  A 16 x 16 output block takes K steps of 16 window rows
// (S = ceil((16 + 2 half) / 16)); K slot (g, 2 j + h) of step s is window row
// 16 s + 4 g + j of the block, part h.  The windows are the 32 x (64 + 2 half)
// dword planes of gen_vtile2, double-buffered by LDS DMA.  Wave w owns output
// rows 16 w .. 16 w + 15 of the 64 x 32 tile, both 16-column blocks; a
// channel's filters accumulate into its two D blocks (x 2^30, folded into the
// Lab matrix).
// NRB = 2: wave w owns output rows 32 w .. 32 w + 31 of a 128 x 32 tile.  Block
// 1's B operand of step s is block 0's of step s + 1 (the rows 16 further
// down), so one window read feeds both blocks: D0 += A_b B_b, D1 += A_(b-1) B_b
// over b = 0 .. S; and the (128 + 2 half)-row window re-reads 1.8x the tile's
// rows at half 51 instead of 2.6x.
template <int DE, int NRB>
__global__ __launch_bounds__(256) void gen_vmfma_kernel(GenArgs a, int tiles_x) {
    // [2][TH + 2 half][32] windows, then the duplicated split taps [7][hi, lo][TP]
    extern __shared__ uint32_t s_wm[];
    constexpr int TW = kVt2W, TH = 64 * NRB;
    __shared__ double s_red[4];
    const int tid = threadIdx.x, lane = tid & 63, n = lane & 15, g = lane >> 4;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const Geom& gm = a.g;
    const int x0 = (blockIdx.x % tiles_x) * TW, y0 = gm.r0 + (blockIdx.x / tiles_x) * TH;
    const int half = a.half, RH = TH + 2 * half, NE = RH * TW, S = (16 + 2 * half + 15) / 16;
    const int BUF = NE, TP = 16 * S + 16;
    uint32_t* s_tap = s_wm + 2 * BUF;
    // the taps, once per workgroup (their first reads are after the first barrier)
    for (int i = tid; i < kNumFilt * 2 * TP; i += 256) s_tap[i] = a.vtapd[i];
    const int64_t np = gm.n_ext;
    const bool rows_inside = y0 - half >= gm.e0 && y0 - half >= 0 && y0 + TH + half <= gm.e1 && y0 + TH + half <= gm.H;
    const bool wide = (gm.W & 3) == 0;
    auto issue = [&](int f, int b) {
        dma_window(reinterpret_cast<const uint32_t*>(a.t) + (int64_t)f * np, s_wm + b * BUF, NE, tid, wv, gm, x0, y0,
                   half, rows_inside, wide);
    };
    f32x4v D[3][NRB][2];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
#pragma unroll
        for (int rb = 0; rb < NRB; ++rb) D[ch][rb][0] = D[ch][rb][1] = f32x4v{0.f, 0.f, 0.f, 0.f};
    issue(0, 0);
    for (int f = 0; f < kNumFilt; ++f) {
        __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): this wave's rows of window f have landed
        __syncthreads();                     // every wave's rows; window f - 1's readers are done
        if (f + 1 < kNumFilt) issue(f + 1, (f + 1) & 1);
        const uint32_t* win = s_wm + (f & 1) * BUF;
        // A of step s: dwords 16 s + 4 g + j - m + 15 (j = 0 .. 3) of the filter's
        // duplicated hi and lo tap rows -- a window sliding over the taps
        // (fragments read from global memory left each filter waiting on L2)
        const uint32_t* th = s_tap + f * 2 * TP + 4 * g - (lane & 15) + 15;
        f32x4v e[NRB][2];
#pragma unroll
        for (int rb = 0; rb < NRB; ++rb) e[rb][0] = e[rb][1] = f32x4v{0.f, 0.f, 0.f, 0.f};
        f16x8 PH = {}, PL = {};  // A of the previous step (block 1)
        for (int bs = 0; bs < S + NRB - 1; ++bs) {
            const int r = TH / 4 * wv + 16 * bs + 4 * g;
            u32x4 b0, b1;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int row = min(r + j, RH - 1);  // (rows past the window: zero taps, finite data)
                b0[j] = win[row * TW + n];
                b1[j] = win[row * TW + 16 + n];
            }
            const f16x8 B0 = __builtin_bit_cast(f16x8, b0), B1 = __builtin_bit_cast(f16x8, b1);
            f16x8 AH = {}, AL = {};
            if (bs < S) {
                uint4 ch, cl;
                ch.x = th[16 * bs]; ch.y = th[16 * bs + 1]; ch.z = th[16 * bs + 2]; ch.w = th[16 * bs + 3];
                cl.x = th[TP + 16 * bs]; cl.y = th[TP + 16 * bs + 1]; cl.z = th[TP + 16 * bs + 2]; cl.w = th[TP + 16 * bs + 3];
                AH = __builtin_bit_cast(f16x8, ch);
                AL = __builtin_bit_cast(f16x8, cl);
                e[0][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(AH, B0, e[0][0], 0, 0, 0);
                e[0][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(AH, B1, e[0][1], 0, 0, 0);
                e[0][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(AL, B0, e[0][0], 0, 0, 0);
                e[0][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(AL, B1, e[0][1], 0, 0, 0);
            }
            if constexpr (NRB == 2) {
                if (bs >= 1) {
                    e[1][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(PH, B0, e[1][0], 0, 0, 0);
                    e[1][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(PH, B1, e[1][1], 0, 0, 0);
                    e[1][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(PL, B0, e[1][0], 0, 0, 0);
                    e[1][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(PL, B1, e[1][1], 0, 0, 0);
                }
                PH = AH;
                PL = AL;
            }
        }
        const int chp = f == 6 ? 0 : f % 3;  // planes t1.xyz, t2.xyz, t3 -> channels x y z x y z x
#pragma unroll
        for (int rb = 0; rb < NRB; ++rb) {
            if (chp == 0) { D[0][rb][0] += e[rb][0]; D[0][rb][1] += e[rb][1]; }
            else if (chp == 1) { D[1][rb][0] += e[rb][0]; D[1][rb][1] += e[rb][1]; }
            else { D[2][rb][0] += e[rb][0]; D[2][rb][1] += e[rb][1]; }
        }
    }
    double part = 0.0;
#pragma unroll
    for (int rb = 0; rb < NRB; ++rb)
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int y = y0 + TH / 4 * wv + 16 * rb + 4 * g + i, gx = x0 + 16 * cb + n;
                if (gx < gm.W && y < gm.r1) {
                    // (x 2^-30: the data and tap scales, exactly)
                    const float3 lf = opp2f_fast(D[0][rb][cb][i] * kVOutScale, D[1][rb][cb][i] * kVOutScale,
                                                 D[2][rb][cb][i] * kVOutScale, a.m_lab);
                    const int64_t off = (int64_t)(y - gm.r0) * gm.lab_pitch + gx;
                    const float ef = delta_e_f<DE>(a.labL[off], a.labA[off], a.labB[off], lf);
                    if (a.pix_err) a.pix_err[(int64_t)(y - gm.r0) * gm.W + gx] = ef;  // test option: the per-pixel dE
                    const double wgt = a.mask ? (double)a.mask[off] : 1.0;  // pixel mask or weights (gen_vpass)
                    part += wgt != 0.0 ? (double)ef * wgt : 0.0;
                }
            }
    part = wave_sum_to_lane63(part);
    if ((tid & 63) == 63) s_red[tid >> 6] = part;
    __syncthreads();
    if (tid == 0) acc_add(a.acc, a.P, a.p, blockIdx.x, (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]));
}

// gen_hmfma: the horizontal pass on the matrix cores as well (with gen_vmfma;
// palettes in the fast range): gen_vmfma's pair scheme on its side.  D[m][n] =
// sum_k A[m][k] B[k][n] with m an output column of a 16-column block, n a row
// and k an input column: B of step s for lane (n, g) is columns 16 s + 4 g ..
// + 3 of row n's segment (one ds_read_b128 of split dwords), A the
// horizontal taps' duplicated rows (build_vtile_dup_taps with k3 signed: the
// t3 plane's horizontal taps, CL:254-267).  D's lane holds 4 adjacent output
// columns of one row: one 16-B store of split dwords per plane, which is
// gen_vmfma's input as it stands.  A workgroup: 16 rows x 128 columns (4 waves
// x 2 blocks of 16), rpt such tiles down the image per workgroup; its
// segment the 3 channels' split opponent colours, [3][16][pitch] dwords,
// pitch = 8 mod 64 (ds_read_b128's lane groups then hit 64 distinct banks).
constexpr int kHmCB = 2, kHmCols = 64 * kHmCB;
static int hmfma_seg_cols(int H) { return kHmCols - 16 + 16 * vtile_pair_steps(H); }
static int hmfma_pitch(int H) { return (hmfma_seg_cols(H) - 8 + 63) / 64 * 64 + 8; }
template <typename IT>
__global__ __launch_bounds__(256, 2) void gen_hmfma_kernel(GenArgs a, int pitch, int rpt) {  // (2 waves per SIMD: LDS allows 2 workgroups)
    extern __shared__ uint32_t s_hm[];  // [3][16][pitch] segment, then the taps [7][hi, lo][TP]
    const int tid = threadIdx.x, lane = tid & 63, n = lane & 15, g = lane >> 4;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = a.half, W = a.g.W, rows = a.g.e1 - a.g.e0;
    const int S = (16 + 2 * half + 15) / 16, TP = 16 * S + 16, SW = kHmCols - 16 + 16 * S;
    const int x0 = blockIdx.x * kHmCols, yb = blockIdx.y * 16 * rpt;
    const int nt = min(rpt, (rows - yb + 15) / 16);  // this workgroup's tiles
    uint32_t* s_tap = s_hm + 3 * 16 * pitch;
    for (int i = tid; i < kNumFilt * 2 * TP; i += 256) s_tap[i] = a.htapd[i];
    // the segment of a tile: column tid of its 16 rows (SW <= 256 for half <= 64).
    // Software pipeline over the tiles: tile t + 1's colours and tile t + 2's
    // indices are in flight while tile t's MFMAs run (the fill's two dependent
    // memory round trips were exposed once per 16 rows)
    const bool act = tid < SW;
    const IT* col = static_cast<const IT*>(a.idx) + reflect_clamp(x0 - half + tid, W);  // (past the row end: masked)
    uint32_t ix[16];
    float vx[16], vy[16], vz[16];  // (12 bytes each: the registers of two waves per SIMD)
    auto load_ix = [&](int t) {
#pragma unroll
        for (int u = 0; u < 16; ++u) ix[u] = act ? (uint32_t)col[(int64_t)min(yb + 16 * t + u, rows - 1) * W] : 0u;
    };
    auto gather = [&]() {
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const float* o = reinterpret_cast<const float*>(a.opp + ix[u]);
            vx[u] = o[0];
            vy[u] = o[1];
            vz[u] = o[2];
        }
    };
    load_ix(0);
    gather();
    if (nt > 1) load_ix(1);
    const uint32_t* sb = s_hm + n * pitch + 16 * kHmCB * wv + 4 * g;
    const uint32_t* th = s_tap + 4 * g - n + 15;  // (m = lane & 15 = n)
    uint32_t* tpl = reinterpret_cast<uint32_t*>(a.t);
    const int64_t np = a.g.n_ext;
    for (int t = 0; t < nt; ++t) {
        if (t) __syncthreads();  // tile t - 1's operand reads are done
        if (act) {
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                uint32_t* d = s_hm + u * pitch + tid;
                d[0] = split_f16(vx[u]);
                d[16 * pitch] = split_f16(vy[u]);
                d[32 * pitch] = split_f16(vz[u]);
            }
        }
        __syncthreads();
        if (t + 1 < nt) {
            gather();
            if (t + 2 < nt) load_ix(t + 2);
        }
        f32x4v D[kNumFilt][kHmCB];
#pragma unroll
        for (int f = 0; f < kNumFilt; ++f)
#pragma unroll
            for (int cb = 0; cb < kHmCB; ++cb) D[f][cb] = f32x4v{0.f, 0.f, 0.f, 0.f};
        for (int st = 0; st < S; ++st) {
            f16x8 B[3][kHmCB];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch)
#pragma unroll
                for (int cb = 0; cb < kHmCB; ++cb)
                    B[ch][cb] =
                        __builtin_bit_cast(f16x8, *reinterpret_cast<const u32x4*>(sb + ch * 16 * pitch + 16 * cb + 16 * st));
#pragma unroll
            for (int f = 0; f < kNumFilt; ++f) {
                const int ch = f == 6 ? 0 : f % 3;  // planes t1.xyz, t2.xyz, t3 -> channels x y z x y z x
                const uint32_t* tf = th + f * 2 * TP + 16 * st;
                uint4 ah, al;
                ah.x = tf[0]; ah.y = tf[1]; ah.z = tf[2]; ah.w = tf[3];
                al.x = tf[TP]; al.y = tf[TP + 1]; al.z = tf[TP + 2]; al.w = tf[TP + 3];
                const f16x8 AH = __builtin_bit_cast(f16x8, ah), AL = __builtin_bit_cast(f16x8, al);
#pragma unroll
                for (int cb = 0; cb < kHmCB; ++cb)
                    D[f][cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(AH, B[ch][cb], D[f][cb], 0, 0, 0);
#pragma unroll
                for (int cb = 0; cb < kHmCB; ++cb)
                    D[f][cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(AL, B[ch][cb], D[f][cb], 0, 0, 0);
            }
        }
        // lane (n, g): plane row y0 + n, columns 4 g .. 4 g + 3 of each block, x 2^-30
        const int y = yb + 16 * t + n;
        if (y < rows) {
#pragma unroll
            for (int cb = 0; cb < kHmCB; ++cb) {
                const int x = x0 + 16 * (kHmCB * wv + cb) + 4 * g;
                const int64_t q = (int64_t)y * W + x;
                if ((W & 3) == 0 && x + 3 < W) {
#pragma unroll
                    for (int f = 0; f < kNumFilt; ++f)
                        *reinterpret_cast<uint4*>(tpl + f * np + q) =
                            make_uint4(split_f16(D[f][cb][0] * kVOutScale), split_f16(D[f][cb][1] * kVOutScale),
                                       split_f16(D[f][cb][2] * kVOutScale), split_f16(D[f][cb][3] * kVOutScale));
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (x + i < W)
#pragma unroll
                            for (int f = 0; f < kNumFilt; ++f) tpl[f * np + q + i] = split_f16(D[f][cb][i] * kVOutScale);
                }
            }
        }
    }
}

// ---- host side: the launchers; profiling events bracket both launches of a pair ----
// gen_hrow4 with NO outputs per thread
template <bool SPLIT, int NO>
static void launch_hrow4_no(const GenArgs& a, int idx_bytes, hipStream_t s, GenTag* tag) {
    constexpr int SEG = 256 * NO;
    const dim3 hg((unsigned)((a.g.W + SEG - 1) / SEG), (unsigned)(a.g.e1 - a.g.e0));
    const size_t hl = sizeof(float4) * NO * (size_t)((SEG + 2 * a.half + 3 + NO - 1) / NO);
    with_idx(idx_bytes, [&](auto IT) {
        HQ_LAUNCH_DYN_LDS((gen_hrow4_kernel<typename decltype(IT)::type, SPLIT, NO>), hg, dim3(256), hl, s, a);
        if (tag) tag->h = 3, tag->h_outputs = NO, tag->h_split = SPLIT;
    });
}
template <bool SPLIT>
static void launch_hrow4(const GenArgs& a, int idx_bytes, hipStream_t s, GenTag* tag) {  // a.hrow_no: 4 or 8
    with_bool(a.hrow_no == 8, [&](auto EIGHT) { launch_hrow4_no<SPLIT, EIGHT.value ? 8 : 4>(a, idx_bytes, s, tag); });
}

// Explicit instantiations of the two kernels that issue dma_window from a
// lambda: the host compile defines the host handle of only the first instance
// of each it meets, however the launch names the others (in the dispatch
// lambdas below, in a function template of their own, as a pointer handed to
// a lambda: each left the same handles undefined when libhq.so is loaded).
template __global__ void gen_vmfma_kernel<0, 1>(GenArgs, int);
template __global__ void gen_vmfma_kernel<1, 1>(GenArgs, int);
template __global__ void gen_vmfma_kernel<2, 1>(GenArgs, int);
template __global__ void gen_vmfma_kernel<0, 2>(GenArgs, int);
template __global__ void gen_vmfma_kernel<1, 2>(GenArgs, int);
template __global__ void gen_vmfma_kernel<2, 2>(GenArgs, int);
template __global__ void gen_vtile2_kernel<0, HQ_VT2_RB>(GenArgs, int);
template __global__ void gen_vtile2_kernel<1, HQ_VT2_RB>(GenArgs, int);
template __global__ void gen_vtile2_kernel<2, HQ_VT2_RB>(GenArgs, int);

// Both passes on the matrix cores where the options and the half-width allow
// (gen_hmfma or gen_hrow4's split form, then gen_vmfma).
static void launch_cost_vmfma(const GenArgs& a, int de, int idx_bytes, hipStream_t s, GenTag* tag) {
    // workgroup shapes by grid size: the taller forms only when they still
    // give every CU two rounds of work (1024^2: 128-row tiles left 256
    // workgroups, one per CU)
    static const int cus = [] {
        int d = 0, n = 0;
        return hipGetDevice(&d) == hipSuccess &&
                       hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, d) == hipSuccess && n > 0
                   ? n
                   : 256;
    }();
    LaunchEventPair ev;
    const int rows = a.g.e1 - a.g.e0;
    const size_t tap_words = vtile_dup_tap_words(a.half);
    if (a.hmfma && a.htapd) {
        const int pitch = hmfma_pitch(a.half);
        const size_t hl = sizeof(uint32_t) * (3 * 16 * (size_t)pitch + tap_words);
        const int hx = (a.g.W + kHmCols - 1) / kHmCols, tiles = hx * ((rows + 15) / 16);
        // 16-row tiles per workgroup (pipelined fills): 4 on large images
        const int rpt = a.shape == 2 ? 4 : a.shape == 1 ? 1 : tiles >= 16 * cus ? 4 : tiles >= 8 * cus ? 2 : 1;
        const dim3 hg((unsigned)hx, (unsigned)((rows + 16 * rpt - 1) / (16 * rpt)));
        with_idx(idx_bytes, [&](auto IT) {
            HQ_LAUNCH_DYN_LDS((gen_hmfma_kernel<typename decltype(IT)::type>), hg, dim3(256), hl, s, a, pitch, rpt);
            if (tag) tag->h = 4, tag->h_rpt = rpt;
        });
    } else {
        launch_hrow4<true>(a, idx_bytes, s, tag);
    }
    ev.second();
    const int tx = (a.g.W + kVt2W - 1) / kVt2W;
    const bool two = a.shape == 2 || (a.shape == 0 && tx * ((a.g.r1 - a.g.r0 + 127) / 128) >= 4 * cus);  // 128-row tiles
    const int vth = two ? 128 : 64, ty = (a.g.r1 - a.g.r0 + vth - 1) / vth;
    const size_t l2 = sizeof(uint32_t) * (2 * kVt2W * (vth + 2 * (size_t)a.half) + tap_words);
    const dim3 vg((unsigned)(tx * ty));
    with_de(de, [&](auto DE) {
        with_bool(two, [&](auto TWO) {
            HQ_LAUNCH_DYN_LDS((gen_vmfma_kernel<DE.value, TWO.value ? 2 : 1>), vg, dim3(256), l2, s, a, tx);
            if (tag) tag->v = 4, tag->v_rows = TWO.value ? 128 : 64;
        });
    });
}

// The tiled generic pair (gen_hrow + gen_vtile and their faster forms).
hipError_t launch_cost_tiled_generic(const GenArgs& a, int de, int idx_bytes, hipStream_t s, GenTag* tag) {
    if (!known_de(de)) return hipErrorInvalidValue;
    if (tag) *tag = GenTag{}, tag->cost = 3;
    if (a.vmfma && a.vtapd && a.half <= kVt2MaxHalf) {  // the matrix-core vertical pass
        launch_cost_vmfma(a, de, idx_bytes, s, tag);
        return hipGetLastError();
    }
    LaunchEventPair ev;
    if (a.hrow4) {  // (option gen_hrow4, default on; gen_hrow stays as its bitwise cross-check)
        launch_hrow4<false>(a, idx_bytes, s, tag);
    } else {
        const dim3 hg((unsigned)((a.g.W + 255) / 256), (unsigned)(a.g.e1 - a.g.e0));
        const size_t hl = sizeof(float4) * (256 + 2 * (size_t)a.half);
        with_idx(idx_bytes, [&](auto IT) {
            HQ_LAUNCH(gen_hrow_kernel<typename decltype(IT)::type>, hg, dim3(256), hl, s, a);
            if (tag) tag->h = 2;
        });
    }
    ev.second();
    if (a.half <= kVt2MaxHalf && a.vtile2) {  // the double-buffered DMA form (option gen_vtile2)
        constexpr int kVt2H = 8 * HQ_VT2_RB;
        const int tx = (a.g.W + kVt2W - 1) / kVt2W, ty = (a.g.r1 - a.g.r0 + kVt2H - 1) / kVt2H;
        const size_t l2 = sizeof(float) * 2 * kVt2W * (kVt2H + 2 * (size_t)a.half);
        const dim3 vg((unsigned)(tx * ty));
        with_de(de, [&](auto DE) {
            HQ_LAUNCH_DYN_LDS((gen_vtile2_kernel<DE.value, HQ_VT2_RB>), vg, dim3(256), l2, s, a, tx);
            if (tag) tag->v = 3;
        });
        return hipGetLastError();
    }
    const int tiles_x = (a.g.W + kVtTile - 1) / kVtTile, tiles_y = (a.g.r1 - a.g.r0 + kVtTile - 1) / kVtTile;
    const size_t vl = sizeof(float) * kVtTile * (kVtTile + 2 * (size_t)a.half);
    const dim3 vg((unsigned)(tiles_x * tiles_y));
    with_de(de, [&](auto DE) {  // window rows above 64 KB (half > 95): the grant raises the limit
        HQ_LAUNCH_DYN_LDS((gen_vtile_kernel<DE.value>), vg, dim3(256), vl, s, a, tiles_x);
        if (tag) tag->v = 2;
    });
    return hipGetLastError();
}

// The plain per-pixel pair (gen_hpass + gen_vpass; option cost_variant 1).
hipError_t launch_cost_generic(const GenArgs& a, int de, int idx_bytes, hipStream_t s, GenTag* tag) {
    if (!known_de(de)) return hipErrorInvalidValue;
    if (tag) *tag = GenTag{}, tag->cost = 4;
    LaunchEventPair ev;
    with_idx(idx_bytes, [&](auto IT) {
        HQ_LAUNCH(gen_hpass_kernel<typename decltype(IT)::type>, dim3(blocks_for(a.g.n_ext)), dim3(256), 0, s, a);
        if (tag) tag->h = 1;
    });
    ev.second();
    const int64_t n_own = (int64_t)a.g.W * (a.g.r1 - a.g.r0);
    with_de(de, [&](auto DE) { HQ_LAUNCH(gen_vpass_kernel<DE.value>, dim3(blocks_for(n_own)), dim3(256), 0, s, a); });
    if (tag) tag->v = 1;
    return hipGetLastError();
}

}  // namespace hq
