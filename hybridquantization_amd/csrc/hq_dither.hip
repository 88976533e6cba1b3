// hq_dither.hip -- Floyd-Steinberg dithered index images (libhq's addition, no
// reference counterpart): the rendering the S-CIELAB cost is then taken of, in
// the place of the plain argmin's (hq_assign.hip).
//
// Definition, in the argmin's space -- the sRGB-coded planar
// floats -- every operation one fp32 operation rounded to nearest, per channel,
// none contracted into an fma:
//   a = 7 e(x-1, y)   b = 3 e(x+1, y-1)   c = 5 e(x, y-1)   d = e(x-1, y-1)
//   t = ((a + b) + (c + d)) * 0.0625
//   v = min(max(pix + s * t, 0), 1)
//   idx(x, y) = the first minimum over k of ref_dist(v, pal[k])   (CL:179-192)
//   e(x, y) = v - pal[idx]
// with e = 0 outside the image.  Pixel (x, y) needs (x-1, y), (x+1, y-1),
// (x, y-1) and (x-1, y-1): all done once the wavefront t = x + 2 y has passed,
// so the pixels of one wavefront are independent and the raster order's result
// is the wavefront order's.
#include "hq_device.h"
#include "hq_launch.h"

namespace hq {

constexpr int kDitherMaxRows = 1024;  // rows per strip at most: one thread each
constexpr int kDitherRing = 4;        // columns of a row's errors kept in LDS

// The diffusion step of one channel: the value the argmin reads.
__device__ __forceinline__ float dither_value(float pix, float el, float eur, float eu, float eul, float s) {
#pragma clang fp contract(off)
    const float a = 7.0f * el, b = 3.0f * eur, c = 5.0f * eu;
    const float t = ((a + b) + (c + eul)) * 0.0625f;
    const float m = s * t;
    return fminf(fmaxf(pix + m, 0.0f), 1.0f);
}

__device__ __forceinline__ float pick4(const float4& v, int j) {
    return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w;
}

// Columns x .. x + 3 of a row (x a multiple of 4): one 16-byte load where the
// rows are 16-byte aligned (W a multiple of 4), else the columns inside the row.
__device__ __forceinline__ float4 load_quad(const float* row, int x, int W, bool vec) {
    if (vec) return *reinterpret_cast<const float4*>(row + x);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (x < W) v.x = row[x];
    if (x + 1 < W) v.y = row[x + 1];
    if (x + 2 < W) v.z = row[x + 2];
    if (x + 3 < W) v.w = row[x + 3];
    return v;
}

// The reference's first minimum over all K colours (CL:179-192).  Ranked by the
// fma-chain d^2 as the plain assign kernels rank (dist2_rank: ref_len's own d^2
// for w = 0); a runner-up within near_d2 of the best -- v_sqrt_f32 can give two
// d^2 one distance, and then the lower index wins -- is re-resolved by the
// reference loop itself.  v and the colours are finite: no NaN arises.
__device__ __forceinline__ int dither_argmin(float r, float g, float b, const float4* s_pal, int K) {
    float best2 = dist2_rank(r, g, b, s_pal[0]), second2 = INFINITY;
    int bi = 0;
#pragma unroll 4
    for (int k = 1; k < K; ++k) {
        const float d2 = dist2_rank(r, g, b, s_pal[k]);
        const bool lt = d2 < best2;
        bi = lt ? k : bi;
        second2 = __builtin_amdgcn_fmed3f(best2, second2, d2);
        best2 = lt ? d2 : best2;
    }
    if (near_d2(best2, second2)) {
        bi = 0;
        float best = ref_dist(r, g, b, s_pal[0]);
        for (int k = 1; k < K; ++k) {
            const float d = ref_dist(r, g, b, s_pal[k]);
            if (d < best) { best = d; bi = k; }
        }
    }
    return bi;
}

// ----------------------------------------------------------------------------
// dither: grid (P), block = the strip's rows (a multiple of 64, up to 1024).
// One workgroup renders one palette's whole image and waits on no other
// workgroup: the critical path of error diffusion is W + 2 H steps whatever
// one does, so spreading an image over workgroups could buy 2x at most, against
// a wait between workgroups.  Thread r owns row y0 + r of the current strip; at
// step t it handles column x = t - 2 r.  A strip of n rows takes W + 2 (n - 1)
// steps, one barrier each.
//   LDS: the palette, the used bits, and per row a ring of the errors of its last
//   kDitherRing columns.  Row r writes slot x & 3 at step t; row r + 1, two
//   columns behind, reads column x - 1 in the same step, written one step
//   earlier, and keeps the two columns before it in registers -- so one barrier
//   per step orders every read after its write, and a slot is overwritten three
//   steps after its last read.
//   The strip's last row also stores its errors to the carry row ([P][3][W] in
//   global memory), which the next strip's first row reads, one step ahead of
//   its use.  Carry column c is read at step c - 2 of a strip and written at
//   step c + 2 (n - 1) of it (n >= 64 whenever a strip stores one), so every read
//   of a strip precedes the strip's own write of that column.
//   Pixels arrive four columns at a time, four steps ahead of their use; the four
//   indices of an aligned quad leave as one dword.
// ----------------------------------------------------------------------------
__global__ __launch_bounds__(kDitherMaxRows) void dither_kernel(DitherArgs a) {
    __shared__ __attribute__((aligned(16))) float4 s_pal[kMaxK];
    __shared__ uint32_t s_used[8];
    __shared__ float s_ring[3][kDitherRing][kDitherMaxRows];
    const int p = blockIdx.x, r = threadIdx.x, rows = blockDim.x;
    const int W = a.W, H = a.H, K = a.K;
    const float s = a.strength;
    for (int k = r; k < K; k += rows) s_pal[k] = a.pal[(int64_t)p * kMaxK + k];
    if (r < 8) s_used[r] = 0u;
    __syncthreads();
    const bool vec = (W & 3) == 0;
    const float* plane[3] = {a.R, a.G, a.B};
    float* carry = a.carry + (int64_t)p * 3 * W;
    uint8_t* idx = a.idx + (int64_t)p * a.idx_pitch;
    for (int y0 = 0; y0 < H; y0 += rows) {
        const int nr = min(rows, H - y0);  // rows of this strip (uniform)
        const int y = y0 + r;
        const bool row_on = r < nr;
        const bool from_carry = r == 0 && y0 > 0;         // the upper row is the last strip's
        const bool to_carry = r == nr - 1 && y0 + nr < H;  // the next strip reads this row
        const int64_t row0 = (int64_t)y * W;
        float el[3] = {0.f, 0.f, 0.f};                     // e(x-1, y): the row's own last error
        float eu[3] = {0.f, 0.f, 0.f}, eul[3] = {0.f, 0.f, 0.f};  // e(x, y-1), e(x-1, y-1)
        float cnext[3] = {0.f, 0.f, 0.f};                  // the carry row's column x + 1 at the next step
        float4 cur[3], nxt[3];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            cur[ch] = make_float4(0.f, 0.f, 0.f, 0.f);
            nxt[ch] = row_on ? load_quad(plane[ch] + row0, 0, W, vec) : cur[ch];
            if (from_carry) {
                eu[ch] = carry[ch * W];
                if (1 < W) cnext[ch] = carry[ch * W + 1];
            }
        }
        uint32_t pack = 0u;
        const int steps = W + 2 * (nr - 1);
        for (int t = 0; t < steps; ++t) {
            const int x = t - 2 * r;
            if (row_on && x >= -1 && x < W) {
                // e(x+1, y-1): the ring of the row above, the carry row, or nothing
                float eur[3] = {0.f, 0.f, 0.f};
                if (from_carry) {
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) {
                        eur[ch] = cnext[ch];
                        cnext[ch] = x + 2 < W ? carry[ch * W + x + 2] : 0.f;
                    }
                } else if (r > 0 && x + 1 < W) {
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) eur[ch] = s_ring[ch][(x + 1) & (kDitherRing - 1)][r - 1];
                }
                if (x >= 0) {
                    const int j = x & 3;
                    if (j == 0) {
#pragma unroll
                        for (int ch = 0; ch < 3; ++ch) {
                            cur[ch] = nxt[ch];
                            if (x + 4 < W) nxt[ch] = load_quad(plane[ch] + row0, x + 4, W, vec);
                        }
                    }
                    float v[3];
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch)
                        v[ch] = dither_value(pick4(cur[ch], j), el[ch], eur[ch], eu[ch], eul[ch], s);
                    const int k = dither_argmin(v[0], v[1], v[2], s_pal, K);
                    const float4 c = s_pal[k];
                    el[0] = v[0] - c.x;
                    el[1] = v[1] - c.y;
                    el[2] = v[2] - c.z;
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) {
                        s_ring[ch][j][r] = el[ch];
                        if (to_carry) carry[ch * W + x] = el[ch];
                    }
                    atomicOr(&s_used[k >> 5], 1u << (k & 31));
                    pack |= (uint32_t)k << (8 * j);
                    if (j == 3 || x == W - 1) {
                        if (vec) {
                            *reinterpret_cast<uint32_t*>(idx + row0 + x - 3) = pack;
                        } else {
                            for (int i = 0; i <= j; ++i) idx[row0 + x - j + i] = (uint8_t)(pack >> (8 * i));
                        }
                        pack = 0u;
                    }
                }
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    eul[ch] = eu[ch];
                    eu[ch] = eur[ch];
                }
            }
            __syncthreads();
        }
    }
    // finalize ORs the kUsedSlots copies: this one is slot 0, the others stay zero
    if (r < 8) a.used_glob[p * 8 + r] = s_used[r];
}

hipError_t launch_dither(const DitherArgs& a, int P, hipStream_t s, AssignTag* tag) {
    if (a.rows < 64 || a.rows > kDitherMaxRows || a.rows % 64 || a.K < 1 || a.K > kMaxK || a.W < 1 || a.H < 1)
        return hipErrorInvalidValue;
    const int block = min(a.rows, (a.H + 63) / 64 * 64);
    HQ_LAUNCH(dither_kernel, dim3(P), dim3(block), 0, s, a);
    if (tag) *tag = AssignTag{5, 0, 0, 0};  // (the planar floats, always)
    return hipGetLastError();
}

}  // namespace hq
