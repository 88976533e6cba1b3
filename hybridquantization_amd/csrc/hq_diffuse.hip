// hq_diffuse.hip -- error-diffused index images (libhq's addition, no reference
// counterpart): the rendering the S-CIELAB cost is then taken of, in the place of the plain
// argmin's (hq_assign.hip).  Floyd-Steinberg (hq.h: hq_dither_population), Jarvis-Judice-Ninke,
// Stucki, Burkes, the Sierra family, Atkinson, or any legal tap set (hq_diffuse_population):
// one workgroup per palette, one row per thread, strips, one barrier per step, taps that
// reach two rows up and two columns to the right.
//
// Definition, in the argmin's space -- the sRGB-coded planar floats --
// every operation one fp32 operation rounded to nearest, per channel, none contracted into
// an fma; w in scatter notation
// (w[dy][dx + 2] goes from (x, y) to (x + dx, y + dy)), so pixel (x, y) gathers:
//   acc = w[0][3] e(x-1, y) + w[0][4] e(x-2, y)
//         + w[1][0] e(x+2, y-1) + ... + w[1][4] e(x-2, y-1)
//         + w[2][0] e(x+2, y-2) + ... + w[2][4] e(x-2, y-2)      added left to right
//   t = acc / div      v = min(max(pix + s * t, 0), 1)
//   idx(x, y) = the first minimum over k of ref_dist(v, pal[k])     e(x, y) = v - pal[idx]
// with e = 0 outside the image.  An instance <R, S> adds the taps of rows 0 .. R, and of
// row 1's dx = -2 only when S = 3: a position it holds with weight 0 adds +-0, which changes
// no v; a position it leaves out has weight 0 by the classification (hq_diffuse_taps.cpp).
// With S = a + 1 (a the reach of row 1 to the right, at least 1) every source of (x, y)
// lies on an earlier wavefront t = x + S y: (x+a, y-1) one step back, (x+2, y-2) 2 S - 2
// steps back.  So the pixels of a wavefront are independent and the wavefront order's
// result is the raster order's.
// Floyd-Steinberg <1, 2> keeps the formula it was defined by (hq.h), which
// adds its four products in another order than the line above and so rounds differently:
//   t = ((7 e(x-1, y) + 3 e(x+1, y-1)) + (5 e(x, y-1) + e(x-1, y-1))) * 0.0625
// with v, idx and e as above: the instance FS, of the same kernel.
#include "hq_device.h"
#define HQ_DIFFUSE_DEVICE
#include "hq_diffuse.h"

namespace hq {

namespace {

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

// (the argmin, diffuse_argmin: hq_diffuse.h, shared with hq_dot.hip)

// The diffusion step of one channel: the value the argmin reads.  e1, e2: e(x-1, y) and
// e(x-2, y); u1[i], u2[i]: e(x + 2 - i, y-1) and e(x + 2 - i, y-2), the tap dx = i - 2.
template <int R, int S>
__device__ __forceinline__ float diffuse_value(float pix, float e1, float e2, const float (&u1)[5],
                                               const float (&u2)[5], const DiffuseArgs& a) {
#pragma clang fp contract(off)
    float acc = a.w0[0] * e1;
    acc = acc + a.w0[1] * e2;
#pragma unroll
    for (int i = S == 3 ? 0 : 1; i < 5; ++i) acc = acc + a.w1[i] * u1[i];
    if (R == 2) {
#pragma unroll
        for (int i = 0; i < 5; ++i) acc = acc + a.w2[i] * u2[i];
    }
    const float t = acc / a.div;
    const float m = a.strength * t;
    return fminf(fmaxf(pix + m, 0.0f), 1.0f);
}

// Floyd-Steinberg's own: el = e(x-1, y), eur = e(x+1, y-1), eu = e(x, y-1), eul = e(x-1, y-1).
__device__ __forceinline__ float fs_value(float pix, float el, float eur, float eu, float eul, float s) {
#pragma clang fp contract(off)
    const float a = 7.0f * el, b = 3.0f * eur, c = 5.0f * eu;
    const float t = ((a + b) + (c + eul)) * 0.0625f;
    const float m = s * t;
    return fminf(fmaxf(pix + m, 0.0f), 1.0f);
}

constexpr int max_rows(int S) { return S == 3 ? kDiffuseMaxRows3 : kDiffuseMaxRows2; }
constexpr int ring_slots(int S) { return S == 3 ? 8 : 4; }
// Columns a row starts before its first pixel, the steps that fill its windows: row y - 1's
// reaches S - 1 columns to the right, row y - 2's two.
constexpr int lead_in(int R, int S) { return R == 2 ? 2 : S - 1; }

}  // namespace

// ----------------------------------------------------------------------------
// diffuse<R, S, FS>: grid (P), block = the strip's rows (a multiple of 64, up to 1024 at
// S = 2 and 512 at S = 3).  One workgroup renders one palette's whole image and waits on no
// other workgroup: the critical path of error diffusion is W + S H steps whatever one does,
// so spreading an image over workgroups could buy S x at most, against a wait between
// workgroups.  Thread r owns row y0 + r of the current strip; at step t it stands at column
// x = t - S r, from x = -L on, L = lead_in(R, S) steps that fill its windows (2 at R = 2,
// else S - 1: 1 for <1, 2>, Floyd-Steinberg's among them).  A strip of n rows takes
// W + S (n - 1) + L steps, one barrier each.
//   Registers, per channel: the row's own last two errors, and a window of the columns
//   x + 2 .. x - 2 of rows y - 1 and y - 2 (R = 2), shifted by one column per step; at
//   S = 2 row y - 1's window starts at x + 1.
//   LDS: the palette, the used bits, and per row a ring of the errors of its last
//   ring_slots(S) columns.  Row q writes slot xq & (slots - 1) at the step it stands at
//   xq.  Row q + 1, S columns behind, reads column xq - 1 in the same step (written one
//   step earlier), the newest column of its upper window.  Row q + 2, 2 S columns behind,
//   reads column xq - 2 S + 2, the newest of its second window.  One barrier per step
//   orders every read after its write, and the columns xq - 2 S + 2 .. xq - 1 that are
//   still to be read do not share xq's slot as 2 S - 2 < slots: 4 slots at S = 2, 8 at S = 3.
//   The strip's last R rows also store their errors to the carry rows ([P][R][3][W] in
//   global memory; the last row is carry row R - 1).  In the next strip thread 0 takes
//   both its upper rows from them and thread 1 its second one, each column one step ahead
//   of its use: thread 0 loads column c of the last row's carry at step c - S and of the
//   other's at step c - 3, thread 1 of the last row's at step c - 3 + S, and the columns the
//   first step consumes (S - 1 - L of the upper row where that is >= 0, 2 - L = 0 of the
//   second) before the strip's first step.  Whatever L is, column c of a carry row is so
//   loaded at step c + S - 3 of a strip at the latest and written at step c + S (n - 2) at
//   the earliest (row n - 2; n >= 64 whenever a strip stores one), so every read of a strip
//   precedes the strip's own write of that column, and follows the last strip's, whose
//   steps all ended in a barrier.
//   Pixels arrive four columns at a time, four steps ahead of their use; the four
//   indices of an aligned quad leave as one dword.
// ----------------------------------------------------------------------------
template <int R, int S, bool FS>
__global__ __launch_bounds__(max_rows(S)) void diffuse_kernel(DiffuseArgs a) {
    static_assert(!FS || (R == 1 && S == 2), "Floyd-Steinberg's formula: one row up, slope 2");
    constexpr int kRows = max_rows(S), kSlots = ring_slots(S), kLead = lead_in(R, S);
    __shared__ __attribute__((aligned(16))) float4 s_pal[kMaxK];
    __shared__ uint32_t s_used[8];
    __shared__ float s_ring[3][kSlots][kRows];
    const int p = blockIdx.x, r = threadIdx.x, rows = blockDim.x;
    const int W = a.W, H = a.H, K = a.K;
    for (int k = r; k < K; k += rows) s_pal[k] = a.pal[(int64_t)p * kMaxK + k];
    if (r < 8) s_used[r] = 0u;
    __syncthreads();
    const bool vec = (W & 3) == 0;
    const float* plane[3] = {a.R, a.G, a.B};
    float* c_prev = a.carry + (int64_t)p * R * 3 * W;  // R = 2: the strip's last row but one
    float* c_last = c_prev + (int64_t)(R - 1) * 3 * W;  // the strip's last row
    uint8_t* idx = a.idx + (int64_t)p * a.idx_pitch;
    for (int y0 = 0; y0 < H; y0 += rows) {
        const int nr = min(rows, H - y0);  // rows of this strip (uniform)
        const int y = y0 + r;
        const bool row_on = r < nr;
        const bool more = y0 + nr < H;  // the next strip reads this one's last rows
        // rows y - 1 and y - 2: a carry row, the ring of the thread that owns it, or nothing
        const float* up1c = r == 0 && y0 > 0 ? c_last : nullptr;
        const float* up2c = R == 2 && y0 > 0 ? (r == 0 ? c_prev : r == 1 ? c_last : nullptr) : nullptr;
        const bool up1r = r >= 1, up2r = R == 2 && r >= 2;
        float* to_carry = !more ? nullptr : r == nr - 1 ? c_last : R == 2 && r == nr - 2 ? c_prev : nullptr;
        const int64_t row0 = (int64_t)y * W;
        float e1[3] = {0.f, 0.f, 0.f}, e2[3] = {0.f, 0.f, 0.f};  // e(x-1, y), e(x-2, y)
        float u1[3][5], u2[3][5];  // [i]: e(x + 2 - i, y-1), e(x + 2 - i, y-2)
        float n1[3], n2[3];        // the carry rows' columns x + S and x + 3: the next step's
        constexpr int kFirst1 = S - 1 - kLead;  // the upper row's column the first step consumes
        float4 cur[3], nxt[3];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
#pragma unroll
            for (int i = 0; i < 5; ++i) u1[ch][i] = u2[ch][i] = 0.f;
            cur[ch] = make_float4(0.f, 0.f, 0.f, 0.f);
            nxt[ch] = row_on ? load_quad(plane[ch] + row0, 0, W, vec) : cur[ch];
            // the first step stands at x = -kLead: columns kFirst1 (0, or none: -1 at <2, 2>) and 0
            n1[ch] = up1c && kFirst1 >= 0 ? up1c[ch * W + kFirst1] : 0.f;
            n2[ch] = up2c ? up2c[ch * W] : 0.f;
        }
        uint32_t pack = 0u;
        const int steps = W + S * (nr - 1);
        for (int t = -kLead; t < steps; ++t) {
            const int x = t - S * r;
            if (row_on && x >= -kLead && x < W) {
                const int col1 = x + S - 1, col2 = x + 2;  // the windows' new columns (col1 >= -1, col2 >= 0)
                // (one branch for the three channels: their ring reads leave together)
                float a1[3] = {0.f, 0.f, 0.f}, a2[3] = {0.f, 0.f, 0.f};
                if (up1c) {
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) {
                        a1[ch] = n1[ch];
                        n1[ch] = col1 + 1 < W ? up1c[ch * W + col1 + 1] : 0.f;
                    }
                } else if (up1r && (kFirst1 >= 0 || col1 >= 0) && col1 < W) {
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) a1[ch] = s_ring[ch][col1 & (kSlots - 1)][r - 1];
                }
                if (R == 2) {
                    if (up2c) {
#pragma unroll
                        for (int ch = 0; ch < 3; ++ch) {
                            a2[ch] = n2[ch];
                            n2[ch] = col2 + 1 < W ? up2c[ch * W + col2 + 1] : 0.f;
                        }
                    } else if (up2r && col2 < W) {
#pragma unroll
                        for (int ch = 0; ch < 3; ++ch) a2[ch] = s_ring[ch][col2 & (kSlots - 1)][r - 2];
                    }
                }
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
#pragma unroll
                    for (int i = 4; i > 0; --i) {
                        u1[ch][i] = u1[ch][i - 1];
                        u2[ch][i] = u2[ch][i - 1];
                    }
                    u1[ch][S == 3 ? 0 : 1] = a1[ch];
                    u2[ch][0] = a2[ch];
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
                    for (int ch = 0; ch < 3; ++ch) {
                        const float pix = pick4(cur[ch], j);
                        if constexpr (FS) v[ch] = fs_value(pix, e1[ch], u1[ch][1], u1[ch][2], u1[ch][3], a.strength);
                        else v[ch] = diffuse_value<R, S>(pix, e1[ch], e2[ch], u1[ch], u2[ch], a);
                    }
                    const int k = diffuse_argmin(v[0], v[1], v[2], s_pal, K);
                    const float4 c = s_pal[k];
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) e2[ch] = e1[ch];
                    e1[0] = v[0] - c.x;
                    e1[1] = v[1] - c.y;
                    e1[2] = v[2] - c.z;
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) {
                        s_ring[ch][x & (kSlots - 1)][r] = e1[ch];
                        if (to_carry) to_carry[ch * W + x] = e1[ch];
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
            }
            __syncthreads();
        }
    }
    // finalize ORs the kUsedSlots copies: this one is slot 0, the others stay zero
    if (r < 8) a.used_glob[p * 8 + r] = s_used[r];
}

hipError_t launch_diffuse(const DiffuseArgs& a0, int P, hipStream_t s, AssignTag* tag) {
    if (a0.rows < 64 || a0.rows > kDiffuseMaxRows2 || a0.rows % 64 || a0.K < 1 || a0.K > kMaxK || a0.W < 1 ||
        a0.H < 1 || a0.rows_up < 1 || a0.rows_up > 2 || a0.slope < 2 || a0.slope > 3 ||
        (a0.fs && (a0.rows_up != 1 || a0.slope != 2)))
        return hipErrorInvalidValue;
    DiffuseArgs a = a0;
    a.rows = min(a.rows, max_rows(a.slope));
    const int block = min(a.rows, (a.H + 63) / 64 * 64);
    if (a.fs) {
        HQ_LAUNCH((diffuse_kernel<1, 2, true>), dim3(P), dim3(block), 0, s, a);
    } else {
        with_bool(a.rows_up == 2, [&](auto r2) {
            with_bool(a.slope == 3, [&](auto s3) {
                HQ_LAUNCH((diffuse_kernel<r2.value ? 2 : 1, s3.value ? 3 : 2, false>), dim3(P), dim3(block), 0, s, a);
            });
        });
    }
    // hq.h's hq_path_argmin: HQ_ARGMIN_DITHER or HQ_ARGMIN_DIFFUSE (the planar floats, always)
    if (tag) *tag = AssignTag{a.fs ? 5 : 6, 0, 0, 0};
    return hipGetLastError();
}

}  // namespace hq
