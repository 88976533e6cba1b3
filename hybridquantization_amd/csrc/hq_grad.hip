// hq_grad.hip -- the derivative of the S-CIELAB cost with respect to the palette, the index
// images held fixed (hq_cost_gradient, hq.h).  libhq's own addition: the reference
// has no such quantity.
//
// With O(x) = opp(pal[idx(x)]), B = F O the cost's blur (CL:234-306), Lab = Opp2LAB(B) and
// E = dE76(Lab, LabRef), the kernels below make
//   g(x) = dE/dB(x) = J^T(B(x)) (Lab(x) - LabRef(x)) / E(x)     (0 where E == 0),
//   a    = F^T g, the adjoint blur in gather form: per channel and filter pair the transpose of
//          the vertical pass, then of the horizontal one, each
//          (H^T g)(y) = sum_t k[t] (g~(y - t) + g~(-y - 1 - t) + g~(2 n - y - 1 - t)),
//          g~ = g inside the image and 0 outside -- no scatter, no float atomics,
//   S[k][c] = sum over the pixels of colour k of llrint(a_c 2^s), and their count n[k]:
//          integers, so the result does not depend on the order of the atomics.
// The chain rule through the palette's opponent table and srgb_lin ends on the host, in double
// (grad_chain, hq_grad.h).
//
// Two forms.  The plain pair restates the definition one thread per pixel through global
// scratch planes, at any half-width: it cross-checks the tiled form and is the only form above
// half 24.  The tiled form keeps both passes' 7 temporaries in LDS: two launches for the
// whole population, grid (tiles, P).
#include "hq_device.h"
#include "hq_grad.h"

namespace hq {

namespace {

// g of one pixel: the fast Opp2LAB (opp2f_fast's t and f), f' of the branch it took, dE76's
// unit vector, and J^T = m^T diag(f') C^T with C the (116, 500, 200) combination.
__device__ __forceinline__ float lab_f_slope(float t, float f) {
    return t > LAB_DELTA3 ? f / (3.0f * t) : LAB_KAPPA / 116.0f;
}
__device__ __forceinline__ float4 grad_point(float ox, float oy, float oz, float Lr, float Ar, float Br,
                                             const float* m) {
    const float tx = dot3(ox, oy, oz, m + 0), ty = dot3(ox, oy, oz, m + 3), tz = dot3(ox, oy, oz, m + 6);
    const float fx = lab_f_fast(tx), fy = lab_f_fast(ty), fz = lab_f_fast(tz);
    const float dl = fmaf(116.0f, fy, -16.0f) - Lr;
    const float da = fmaf(500.0f, fx - fy, -Ar);
    const float db = fmaf(200.0f, fy - fz, -Br);
    const float e = hw_sqrt((dl * dl + da * da) + db * db);
    if (e == 0.0f) return make_float4(0.f, 0.f, 0.f, 0.f);
    const float inv = 1.0f / e;
    const float gx = 500.0f * da * inv * lab_f_slope(tx, fx);
    const float gy = (116.0f * dl - 500.0f * da + 200.0f * db) * inv * lab_f_slope(ty, fy);
    const float gz = -200.0f * db * inv * lab_f_slope(tz, fz);
    return make_float4(fmaf(gx, m[0], fmaf(gy, m[3], gz * m[6])), fmaf(gx, m[1], fmaf(gy, m[4], gz * m[7])),
                       fmaf(gx, m[2], fmaf(gy, m[5], gz * m[8])), 0.f);
}

// The tap offsets i whose folded source lies inside an image of n: the low fold -y - 1 - i
// (for y < half) and the high fold 2 n - y - 1 - i (for y >= n - half).
__device__ __forceinline__ void fold_low(int y, int n, int half, int* i0, int* i1) {
    *i0 = max(-half, -y - n);
    *i1 = -y - 1;
}
__device__ __forceinline__ void fold_high(int y, int n, int half, int* i0, int* i1) {
    *i0 = n - y;
    *i1 = min(half, 2 * n - y - 1);
}

// One pixel's a into the bins (`add(k, c, v)` for c = 0 .. 2, `count(k, n)`).  Every lane of the
// wave calls it; a wave whose pixels all have one colour adds once.
template <typename Add, typename Count>
__device__ __forceinline__ void bin_pixel(bool valid, uint32_t k, float ax, float ay, float az, float scale, Add&& add,
                                          Count&& count) {
    const unsigned long long vx = (unsigned long long)__float2ll_rn(ax * scale);
    const unsigned long long vy = (unsigned long long)__float2ll_rn(ay * scale);
    const unsigned long long vz = (unsigned long long)__float2ll_rn(az * scale);
    const uint32_t kk = valid ? k : 0xffffffffu;
    const uint32_t k0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)kk);
    if (__builtin_amdgcn_ballot_w64(kk != k0) == 0) {
        if (k0 == 0xffffffffu) return;
        const unsigned long long sx = wave_sum_u64(vx), sy = wave_sum_u64(vy), sz = wave_sum_u64(vz);
        if ((threadIdx.x & 63) == 0) {
            add(k0, 0, sx), add(k0, 1, sy), add(k0, 2, sz);
            count(k0, 64u);
        }
    } else if (valid) {
        add(k, 0, vx), add(k, 1, vy), add(k, 2, vz);
        count(k, 1u);
    }
}

}  // namespace

// ----------------------------------------------------------------------------
// The plain pair: one thread per pixel of palette p, through a.t ([7][N]).
//   grad_hfwd: the forward horizontal pass (gen_hpass_kernel's loop) -> t1.xyz, t2.xyz, t3
//   grad_g:    the forward vertical pass, then g
//   grad_vadj: the vertical passes' transposes of g -> u1.xyz, u2.xyz (|k3| on) u3
//   grad_hadj: the horizontal passes' transposes, summed -> a, into the global bins
// ----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void grad_hfwd_kernel(GradArgs a, int p) {
    const int64_t n = (int64_t)a.W * a.H;
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= n) return;
    const int y = (int)(q / a.W), x = (int)(q % a.W);
    const uint8_t* row = a.idx + (int64_t)p * a.idx_pitch + (int64_t)y * a.W;
    const float4* opp = a.opp + (int64_t)p * kMaxK;
    float t1x = 0, t1y = 0, t1z = 0, t2x = 0, t2y = 0, t2z = 0, t3 = 0;
    for (int i = -a.half, t = 0; i <= a.half; ++i, ++t) {
        const float4 in = opp[row[reflect_only(x + i, a.W)]];
        t1x = fmaf(in.x, a.k1[4 * t + 0], t1x);
        t1y = fmaf(in.y, a.k1[4 * t + 1], t1y);
        t1z = fmaf(in.z, a.k1[4 * t + 2], t1z);
        t2x = fmaf(in.x, a.k2[4 * t + 0], t2x);
        t2y = fmaf(in.y, a.k2[4 * t + 1], t2y);
        t2z = fmaf(in.z, a.k2[4 * t + 2], t2z);
        t3 = fmaf(in.x, a.k3[t], t3);
    }
    a.t[q] = t1x; a.t[n + q] = t1y; a.t[2 * n + q] = t1z;
    a.t[3 * n + q] = t2x; a.t[4 * n + q] = t2y; a.t[5 * n + q] = t2z;
    a.t[6 * n + q] = t3;
}

__global__ __launch_bounds__(256) void grad_g_kernel(GradArgs a, int p) {
    const int64_t n = (int64_t)a.W * a.H;
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= n) return;
    const int y = (int)(q / a.W), x = (int)(q % a.W);
    float ox = 0, oy = 0, oz = 0;
    for (int i = -a.half, t = 0; i <= a.half; ++i, ++t) {
        const int64_t s = (int64_t)reflect_only(y + i, a.H) * a.W + x;
        ox = fmaf(a.t[s], a.k1[4 * t + 0], fmaf(a.t[3 * n + s], a.k2[4 * t + 0], ox));
        oy = fmaf(a.t[n + s], a.k1[4 * t + 1], fmaf(a.t[4 * n + s], a.k2[4 * t + 1], oy));
        oz = fmaf(a.t[2 * n + s], a.k1[4 * t + 2], fmaf(a.t[5 * n + s], a.k2[4 * t + 2], oz));
        ox = fmaf(a.t[6 * n + s], a.absk3[t], ox);
    }
    const int64_t off = (int64_t)y * a.lab_pitch + x;
    a.g[(int64_t)p * n + q] = grad_point(ox, oy, oz, a.labL[off], a.labA[off], a.labB[off], a.m_lab);
}

__global__ __launch_bounds__(256) void grad_vadj_kernel(GradArgs a, int p) {
    const int64_t n = (int64_t)a.W * a.H;
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= n) return;
    const int y = (int)(q / a.W), x = (int)(q % a.W);
    const float4* g = a.g + (int64_t)p * n + x;
    float u1x = 0, u1y = 0, u1z = 0, u2x = 0, u2y = 0, u2z = 0, u3 = 0;
    for (int i = -a.half, t = 0; i <= a.half; ++i, ++t) {
        const int s0 = y - i, s1 = -y - 1 - i, s2 = 2 * a.H - y - 1 - i;
        float gx = 0, gy = 0, gz = 0;
        if (s0 >= 0 && s0 < a.H) { const float4 v = g[(int64_t)s0 * a.W]; gx += v.x, gy += v.y, gz += v.z; }
        if (s1 >= 0 && s1 < a.H) { const float4 v = g[(int64_t)s1 * a.W]; gx += v.x, gy += v.y, gz += v.z; }
        if (s2 >= 0 && s2 < a.H) { const float4 v = g[(int64_t)s2 * a.W]; gx += v.x, gy += v.y, gz += v.z; }
        u1x = fmaf(gx, a.k1[4 * t + 0], u1x);
        u1y = fmaf(gy, a.k1[4 * t + 1], u1y);
        u1z = fmaf(gz, a.k1[4 * t + 2], u1z);
        u2x = fmaf(gx, a.k2[4 * t + 0], u2x);
        u2y = fmaf(gy, a.k2[4 * t + 1], u2y);
        u2z = fmaf(gz, a.k2[4 * t + 2], u2z);
        u3 = fmaf(gx, a.absk3[t], u3);
    }
    a.t[q] = u1x; a.t[n + q] = u1y; a.t[2 * n + q] = u1z;
    a.t[3 * n + q] = u2x; a.t[4 * n + q] = u2y; a.t[5 * n + q] = u2z;
    a.t[6 * n + q] = u3;
}

__global__ __launch_bounds__(256) void grad_hadj_kernel(GradArgs a, int p) {
    const int64_t n = (int64_t)a.W * a.H;
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool valid = q < n;
    const int64_t qc = valid ? q : n - 1;  // (every lane goes on: the wave reduction needs them all)
    const int x = (int)(qc % a.W);
    const float* row = a.t + (qc - x);
    float ax = 0, ay = 0, az = 0;
    for (int i = -a.half, t = 0; i <= a.half; ++i, ++t) {
        const int s[3] = {x - i, -x - 1 - i, 2 * a.W - x - 1 - i};
        float u[7] = {0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 3; ++j)
            if (s[j] >= 0 && s[j] < a.W) {
#pragma unroll
                for (int f = 0; f < 7; ++f) u[f] += row[f * n + s[j]];
            }
        ax = fmaf(u[0], a.k1[4 * t + 0], fmaf(u[3], a.k2[4 * t + 0], ax));
        ay = fmaf(u[1], a.k1[4 * t + 1], fmaf(u[4], a.k2[4 * t + 1], ay));
        az = fmaf(u[2], a.k1[4 * t + 2], fmaf(u[5], a.k2[4 * t + 2], az));
        ax = fmaf(u[6], a.k3[t], ax);
    }
    const uint32_t k = a.idx[(int64_t)p * a.idx_pitch + qc];
    unsigned long long* sums = a.sums + (int64_t)p * a.K * 4;
    const uint32_t K = (uint32_t)a.K;
    bin_pixel(valid && k < K, k, ax, ay, az, a.scale,
              [&](uint32_t kk, int c, unsigned long long v) { if (v) atomicAdd(sums + 4 * kk + c, v); },
              [&](uint32_t kk, uint32_t cnt) { atomicAdd(sums + 4 * kk + 3, (unsigned long long)cnt); });
}

// ----------------------------------------------------------------------------
// The tiled form, half <= kGradMaxHalfTiled.  Grid (tiles, P), 256 threads (4 waves).
//
// grad_pixel: a tile of kGradTW x kGradPixTH pixels.  Dynamic LDS: the palette's opponent table
// [256] float4; the tile's u8 indices with a halo of half on every side, reflected as they are
// loaded ([TH + 2 half][TW + 2 half] bytes); the 7 horizontal temporaries of the tile's columns
// over its rows and the halo rows ([7][TH + 2 half][TW] floats).  The horizontal pass gathers
// the opponent colours from the table by the LDS indices; the vertical pass reads the
// temporaries column-wise (consecutive lanes, consecutive banks), then Opp2LAB with its
// Jacobian and dE76 against LabRef: g goes out as one float4 per pixel.
// ----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void grad_pixel_kernel(GradArgs a, int tiles_x) {
    constexpr int TW = kGradTW, TH = kGradPixTH;
    extern __shared__ __align__(16) unsigned char s_raw[];
    const int half = a.half, T = 2 * half + 1, RH = TH + 2 * half, RW = TW + 2 * half;
    float4* s_opp = reinterpret_cast<float4*>(s_raw);
    float* s_t = reinterpret_cast<float*>(s_raw + sizeof(float4) * kMaxK);
    uint8_t* s_idx = reinterpret_cast<uint8_t*>(s_t + 7 * RH * TW);
    const int tid = threadIdx.x, p = blockIdx.y;
    const int x0 = (int)(blockIdx.x % tiles_x) * TW, y0 = (int)(blockIdx.x / tiles_x) * TH;
    const uint8_t* idx = a.idx + (int64_t)p * a.idx_pitch;
    for (int k = tid; k < kMaxK; k += 256)
        s_opp[k] = k < a.K ? a.opp[(int64_t)p * kMaxK + k] : make_float4(0.f, 0.f, 0.f, 0.f);
    for (int e = tid; e < RH * RW; e += 256) {
        const int r = e / RW, c = e - r * RW;
        s_idx[e] = idx[(int64_t)reflect_clamp(y0 - half + r, a.H) * a.W + reflect_clamp(x0 - half + c, a.W)];
    }
    __syncthreads();
    const int plane = RH * TW;
    for (int e = tid; e < plane; e += 256) {
        const int r = e / TW, c = e % TW;
        const uint8_t* src = s_idx + r * RW + c;
        float t1x = 0, t1y = 0, t1z = 0, t2x = 0, t2y = 0, t2z = 0, t3 = 0;
        for (int t = 0; t < T; ++t) {
            const float4 in = s_opp[src[t]];
            t1x = fmaf(in.x, a.k1[4 * t + 0], t1x);
            t1y = fmaf(in.y, a.k1[4 * t + 1], t1y);
            t1z = fmaf(in.z, a.k1[4 * t + 2], t1z);
            t2x = fmaf(in.x, a.k2[4 * t + 0], t2x);
            t2y = fmaf(in.y, a.k2[4 * t + 1], t2y);
            t2z = fmaf(in.z, a.k2[4 * t + 2], t2z);
            t3 = fmaf(in.x, a.k3[t], t3);
        }
        s_t[e] = t1x; s_t[plane + e] = t1y; s_t[2 * plane + e] = t1z;
        s_t[3 * plane + e] = t2x; s_t[4 * plane + e] = t2y; s_t[5 * plane + e] = t2z;
        s_t[6 * plane + e] = t3;
    }
    __syncthreads();
    const int64_t n = (int64_t)a.W * a.H;
    for (int e = tid; e < TH * TW; e += 256) {
        const int r = e / TW, c = e % TW;
        const int y = y0 + r, x = x0 + c;
        if (y >= a.H || x >= a.W) continue;
        float ox = 0, oy = 0, oz = 0;
        const float* col = s_t + r * TW + c;
        for (int t = 0; t < T; ++t, col += TW) {
            ox = fmaf(col[0], a.k1[4 * t + 0], fmaf(col[3 * plane], a.k2[4 * t + 0], ox));
            oy = fmaf(col[plane], a.k1[4 * t + 1], fmaf(col[4 * plane], a.k2[4 * t + 1], oy));
            oz = fmaf(col[2 * plane], a.k1[4 * t + 2], fmaf(col[5 * plane], a.k2[4 * t + 2], oz));
            ox = fmaf(col[6 * plane], a.absk3[t], ox);
        }
        const int64_t off = (int64_t)y * a.lab_pitch + x;
        a.g[(int64_t)p * n + (int64_t)y * a.W + x] =
            grad_point(ox, oy, oz, a.labL[off], a.labA[off], a.labB[off], a.m_lab);
    }
}

// ----------------------------------------------------------------------------
// grad_adjoint: a tile of kGradTW x kGradAdjTH pixels.  Dynamic LDS: g over the tile and a halo
// of half on every side as three planes, zero outside the image ([3][TH + 2 half][TW + 2 half]
// floats: g~); the 7 vertical-adjoint temporaries over the tile's rows and the halo columns
// ([7][TH][TW + 2 half]); the bins ([256][3] 64-bit sums, [256] 32-bit counts).
// A source of the unfolded term lies inside the halo by construction.  A folded source
// -y - 1 - i exists only for y < half and lies in [0, half - 1 - y], a folded source
// 2 n - y - 1 - i only for y >= n - half and lies in [n - half, n - 1]: both inside the in-image
// part of the same halo, so nothing outside the image and nothing outside the LDS planes is
// read (the folds run only in the border tiles; the region index is checked all the same).
// The horizontal adjoint follows on the temporaries; each pixel's a goes into the bins by its
// index; one flush per workgroup with 64-bit global integer atomics.  No plane of a is written.
// ----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void grad_adjoint_kernel(GradArgs a, int tiles_x) {
    constexpr int TW = kGradTW, TH = kGradAdjTH;
    extern __shared__ __align__(16) unsigned char s_raw[];
    const int half = a.half, RH = TH + 2 * half, RW = TW + 2 * half;
    const int gplane = RH * RW, uplane = TH * RW;
    unsigned long long* s_bin = reinterpret_cast<unsigned long long*>(s_raw);
    uint32_t* s_cnt = reinterpret_cast<uint32_t*>(s_bin + 3 * kMaxK);
    float* s_g = reinterpret_cast<float*>(s_cnt + kMaxK);
    float* s_u = s_g + 3 * gplane;
    const int tid = threadIdx.x, p = blockIdx.y;
    const int x0 = (int)(blockIdx.x % tiles_x) * TW, y0 = (int)(blockIdx.x / tiles_x) * TH;
    const int64_t n = (int64_t)a.W * a.H;
    const float4* g = a.g + (int64_t)p * n;
    for (int e = tid; e < 3 * kMaxK; e += 256) s_bin[e] = 0ull;
    for (int e = tid; e < kMaxK; e += 256) s_cnt[e] = 0u;
    for (int e = tid; e < gplane; e += 256) {
        const int r = e / RW, c = e - r * RW;
        const int gy = y0 - half + r, gx = x0 - half + c;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) v = g[(int64_t)gy * a.W + gx];
        s_g[e] = v.x, s_g[gplane + e] = v.y, s_g[2 * gplane + e] = v.z;
    }
    __syncthreads();
    // the vertical passes' transposes: region row of image row s is s - y0 + half
    for (int e = tid; e < uplane; e += 256) {
        const int r = e / RW, c = e - r * RW;
        const int y = y0 + r;
        float u1x = 0, u1y = 0, u1z = 0, u2x = 0, u2y = 0, u2z = 0, u3 = 0;
        auto tap = [&](int i, int rr) {
            const int t = i + half, o = rr * RW + c;
            const float gx = s_g[o], gy = s_g[gplane + o], gz = s_g[2 * gplane + o];
            u1x = fmaf(gx, a.k1[4 * t + 0], u1x);
            u1y = fmaf(gy, a.k1[4 * t + 1], u1y);
            u1z = fmaf(gz, a.k1[4 * t + 2], u1z);
            u2x = fmaf(gx, a.k2[4 * t + 0], u2x);
            u2y = fmaf(gy, a.k2[4 * t + 1], u2y);
            u2z = fmaf(gz, a.k2[4 * t + 2], u2z);
            u3 = fmaf(gx, a.absk3[t], u3);
        };
        if (y < a.H) {
            for (int i = -half; i <= half; ++i) tap(i, r + half - i);
            int i0, i1;
            if (y < half) {
                fold_low(y, a.H, half, &i0, &i1);
                for (int i = i0; i <= i1; ++i) {
                    const int rr = -y - 1 - i - y0 + half;
                    if (rr >= 0 && rr < RH) tap(i, rr);
                }
            }
            if (y >= a.H - half) {
                fold_high(y, a.H, half, &i0, &i1);
                for (int i = i0; i <= i1; ++i) {
                    const int rr = 2 * a.H - y - 1 - i - y0 + half;
                    if (rr >= 0 && rr < RH) tap(i, rr);
                }
            }
        }
        s_u[e] = u1x; s_u[uplane + e] = u1y; s_u[2 * uplane + e] = u1z;
        s_u[3 * uplane + e] = u2x; s_u[4 * uplane + e] = u2y; s_u[5 * uplane + e] = u2z;
        s_u[6 * uplane + e] = u3;
    }
    __syncthreads();
    // the horizontal passes' transposes, summed: region column of image column s is s - x0 + half
    static_assert(TW * TH % 256 == 0, "every lane runs every step: the wave reductions need them all");
    for (int e = tid; e < TH * TW; e += 256) {
        const int r = e / TW, c = e % TW;
        const int y = y0 + r, x = x0 + c;
        const bool valid = y < a.H && x < a.W;
        float ax = 0, ay = 0, az = 0;
        auto tap = [&](int i, int cc) {
            const int t = i + half;
            const float* u = s_u + r * RW + cc;
            ax = fmaf(u[0], a.k1[4 * t + 0], fmaf(u[3 * uplane], a.k2[4 * t + 0], ax));
            ay = fmaf(u[uplane], a.k1[4 * t + 1], fmaf(u[4 * uplane], a.k2[4 * t + 1], ay));
            az = fmaf(u[2 * uplane], a.k1[4 * t + 2], fmaf(u[5 * uplane], a.k2[4 * t + 2], az));
            ax = fmaf(u[6 * uplane], a.k3[t], ax);
        };
        uint32_t k = 0;
        if (valid) {
            for (int i = -half; i <= half; ++i) tap(i, c + half - i);
            int i0, i1;
            if (x < half) {
                fold_low(x, a.W, half, &i0, &i1);
                for (int i = i0; i <= i1; ++i) {
                    const int cc = -x - 1 - i - x0 + half;
                    if (cc >= 0 && cc < RW) tap(i, cc);
                }
            }
            if (x >= a.W - half) {
                fold_high(x, a.W, half, &i0, &i1);
                for (int i = i0; i <= i1; ++i) {
                    const int cc = 2 * a.W - x - 1 - i - x0 + half;
                    if (cc >= 0 && cc < RW) tap(i, cc);
                }
            }
            k = a.idx[(int64_t)p * a.idx_pitch + (int64_t)y * a.W + x];  // (k <= 255: inside the bins)
        }
        bin_pixel(valid, k, ax, ay, az, a.scale,
                  [&](uint32_t kk, int ch, unsigned long long v) { if (v) atomicAdd(s_bin + 3 * kk + ch, v); },
                  [&](uint32_t kk, uint32_t cnt) { atomicAdd(s_cnt + kk, cnt); });
    }
    __syncthreads();
    unsigned long long* sums = a.sums + (int64_t)p * a.K * 4;
    for (int k = tid; k < a.K; k += 256) {
        const uint32_t cnt = s_cnt[k];
        if (!cnt) continue;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
            if (s_bin[3 * k + ch]) atomicAdd(sums + 4 * k + ch, s_bin[3 * k + ch]);
        atomicAdd(sums + 4 * k + 3, (unsigned long long)cnt);
    }
}

// ---- launchers -------------------------------------------------------------------
size_t grad_pixel_lds(int half) {
    const size_t RH = kGradPixTH + 2 * half, RW = kGradTW + 2 * half;
    return sizeof(float4) * kMaxK + sizeof(float) * 7 * RH * kGradTW + ((RH * RW + 15) & ~(size_t)15);
}
size_t grad_adjoint_lds(int half) {
    const size_t RH = kGradAdjTH + 2 * half, RW = kGradTW + 2 * half;
    return (sizeof(unsigned long long) * 3 + sizeof(uint32_t)) * kMaxK + sizeof(float) * (3 * RH * RW + 7 * kGradAdjTH * RW);
}

namespace {
bool grad_args_ok(const GradArgs& a) {
    return a.W >= 1 && a.H >= 1 && a.P >= 1 && a.K >= 1 && a.K <= kMaxK && a.half >= 0 && a.half <= a.W &&
           a.half <= a.H && 2 * a.half + 1 <= kMaxTaps && (int64_t)a.W * a.H <= a.idx_pitch;
}
}  // namespace

hipError_t launch_grad_plain(const GradArgs& a, hipStream_t s, hipEvent_t ev_pix[2], hipEvent_t ev_adj[2]) {
    if (!grad_args_ok(a) || !a.t) return hipErrorInvalidValue;
    const dim3 grid(blocks_for((int64_t)a.W * a.H)), block(256);
    for (int p = 0; p < a.P; ++p) {
        set_launch_events(ev_pix && p == 0 ? ev_pix[0] : nullptr, nullptr);
        HQ_LAUNCH(grad_hfwd_kernel, grid, block, 0, s, a, p);
        set_launch_events(nullptr, ev_pix && p == a.P - 1 ? ev_pix[1] : nullptr);
        HQ_LAUNCH(grad_g_kernel, grid, block, 0, s, a, p);
    }
    for (int p = 0; p < a.P; ++p) {
        set_launch_events(ev_adj && p == 0 ? ev_adj[0] : nullptr, nullptr);
        HQ_LAUNCH(grad_vadj_kernel, grid, block, 0, s, a, p);
        set_launch_events(nullptr, ev_adj && p == a.P - 1 ? ev_adj[1] : nullptr);
        HQ_LAUNCH(grad_hadj_kernel, grid, block, 0, s, a, p);
    }
    set_launch_events(nullptr, nullptr);
    return hipGetLastError();
}

bool grad_tiled_grant(int half) {
    return allow_dyn_lds(reinterpret_cast<const void*>(grad_pixel_kernel), grad_pixel_lds(half)) &&
           allow_dyn_lds(reinterpret_cast<const void*>(grad_adjoint_kernel), grad_adjoint_lds(half));
}

hipError_t launch_grad_tiled(const GradArgs& a, hipStream_t s, hipEvent_t ev_pix[2], hipEvent_t ev_adj[2]) {
    if (!grad_args_ok(a) || a.half > kGradMaxHalfTiled) return hipErrorInvalidValue;
    const int tiles_x = (a.W + kGradTW - 1) / kGradTW;
    const unsigned tp = (unsigned)(tiles_x * ((a.H + kGradPixTH - 1) / kGradPixTH));
    const unsigned ta = (unsigned)(tiles_x * ((a.H + kGradAdjTH - 1) / kGradAdjTH));
    set_launch_events(ev_pix ? ev_pix[0] : nullptr, ev_pix ? ev_pix[1] : nullptr);
    HQ_LAUNCH_DYN_LDS(grad_pixel_kernel, dim3(tp, (unsigned)a.P), dim3(256), grad_pixel_lds(a.half), s, a, tiles_x);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) {
        set_launch_events(ev_adj ? ev_adj[0] : nullptr, ev_adj ? ev_adj[1] : nullptr);
        HQ_LAUNCH_DYN_LDS(grad_adjoint_kernel, dim3(ta, (unsigned)a.P), dim3(256), grad_adjoint_lds(a.half), s, a,
                          tiles_x);
        e = hipGetLastError();
    }
    set_launch_events(nullptr, nullptr);
    return e;
}

}  // namespace hq
