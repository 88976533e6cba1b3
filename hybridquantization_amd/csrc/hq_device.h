// hq_device.h -- device helpers shared by the gfx950 kernels of libhq:
// colour constants and conversions (CL:77-145), the argmin distance as the
// reference computes it on gfx950 (CL:179-193), dE (CL:201-226), wave
// reductions and the XCD-aware grid relabelling.  Included by every .hip translation unit of the library.
#pragma once

// HQ_ABL_* switches are timing ablations: they drop work and give wrong
// results.  A build that sets one must say so with HQ_ABLATION_BUILD, so a
// stray -D can never produce a library that silently returns wrong costs
// (such a library says so on stderr at every hq_create; tests/test_capi.py
// checks that every HQ_ABL_ name in the sources is listed here).
#if !defined(HQ_ABLATION_BUILD) &&                                                                    \
    (defined(HQ_ABL_NOLOOP) || defined(HQ_ABL_NOSLOW) || defined(HQ_ABL_HASHLOOKUP) ||                \
     defined(HQ_ABL_COHERENT) || defined(HQ_ABL_NOLOOKUP) || defined(HQ_ABL_NOUSED) ||                \
     defined(HQ_ABL_GRID_L1ONLY) || defined(HQ_ABL_TRUNC) || defined(HQ_ABL_NOFILL) ||                \
     defined(HQ_ABL_MFMA1) || defined(HQ_ABL_NOHPASS) || defined(HQ_ABL_NOVSTORE) ||                  \
     defined(HQ_ABL_NOMFMA) || defined(HQ_ABL_NOIDX) || defined(HQ_ABL_NOTAB) ||                      \
     defined(HQ_ABL_NOLABLD) || defined(HQ_ABL_NOLAB) || defined(HQ_ABL_NORED) ||                      \
     defined(HQ_ABL_N16NOL2))
#error "HQ_ABL_* ablations give wrong results: define HQ_ABLATION_BUILD as well to build one"
#endif

#include "hq_internal.h"

#include <hip/hip_ext.h>

#include <math.h>

namespace hq {

// ----------------------------------------------------------------------------
// Colour constants (CL:77, CL:110, CL:118, CL:171; CL:120-123)
// ----------------------------------------------------------------------------
__constant__ float c_RGB2XYZ[9] = {0.4124564f, 0.3575761f, 0.1804375f, 0.2126729f, 0.7151522f,
                                   0.0721750f, 0.0193339f, 0.1191920f, 0.9503041f};
__constant__ float c_XYZ2Opp[9] = {0.2787336f,  0.7218031f, -0.1065520f, -0.4487736f, 0.2898056f,
                                   -0.0771569f, 0.0859513f, -0.5899859f, 0.5011089f};
__constant__ float c_Opp2XYZ[9] = HQ_OPP2XYZ;  // (hq_cost_layout.h: the host's opp2xyz_over_illum reads it too)
__constant__ float c_RGB2Opp[9] = {0.266413f,  0.603167f, 0.00113333f, -0.124957f, 0.0375879f,
                                   -0.133381f, -0.0803345f, -0.331467f, 0.449132f};

#define LAB_DELTA3 (216.0f / 24389.0f)
#define LAB_KAPPA (24389.0f / 27.0f)

__device__ __forceinline__ float dot3(float x, float y, float z, const float* m) {
    return (x * m[0] + y * m[1]) + z * m[2];
}

__device__ __forceinline__ float srgb_lin(float x) {  // CL:85-87, CL:194-196
    return x <= 0.04045f ? x / 12.92f : powf((x + 0.055f) / 1.055f, 2.4f);
}

__device__ __forceinline__ float lab_f(float t) {  // CL:137
    return t > LAB_DELTA3 ? cbrtf(t) : fmaf(LAB_KAPPA, t, 16.0f) * (1.0f / 116.0f);
}

// The hot path's Opp->Lab (CL:124-145): m = Opp->XYZ with row r divided by the
// illuminant's component r (opp2xyz_over_illum), so t = X/Xn etc. is one dot
// product; cube root as exp2(log2(t)/3) (v_log_f32 / v_exp_f32; ~1 ulp over
// t in (delta^3, ~1.1]: log2 t stays small, so its fp32 rounding moves the
// root by ~2e-8 relative on average -- round 3 worked on t' = 116^3 t, whose
// log2 near 20 carried 6x that), the linear segment fma(kappa / 116, t,
// 16 / 116), selected branch-free.  Off D65 t leaves that range: the tests
// cover t up to 2.16 (Z/Zn at illuminant A; |log2 t| stays below 8 down to
// delta^3) and Yn = 0.8 and 1.25, at the bars measured under D65
// (tests/test_illuminant_gpu.py, DESIGN.md "The illuminant axis").
__device__ __forceinline__ float lab_f_fast(float t) {
    // y is only selected for t > delta^3 > 0 (for t <= 0 it is 0 or NaN, discarded)
    const float y = __builtin_amdgcn_exp2f(__builtin_amdgcn_logf(t) * (1.0f / 3.0f));
    const float lin = fmaf(LAB_KAPPA / 116.0f, t, 16.0f / 116.0f);
    return t > LAB_DELTA3 ? y : lin;
}

// lab_f_fast's cube-root branch alone: for a wave whose every t is above
// delta^3 (the caller's ballot), the linear segment and the select are dead.
// (A NaN t gives NaN either way.)
__device__ __forceinline__ float lab_f_root(float t) {
    return __builtin_amdgcn_exp2f(__builtin_amdgcn_logf(t) * (1.0f / 3.0f));
}

// (f(X/Xn), f(Y/Yn), f(Z/Zn)) of an opponent colour: L = 116 f.y - 16,
// a = 500 (f.x - f.y), b = 200 (f.y - f.z).
__device__ __forceinline__ float3 opp2f_fast(float o0, float o1, float o2, const float* m) {
    return make_float3(lab_f_fast(dot3(o0, o1, o2, m + 0)), lab_f_fast(dot3(o0, o1, o2, m + 3)),
                       lab_f_fast(dot3(o0, o1, o2, m + 6)));
}

// The argmin coordinates of a colour in CIELAB (option "assign_space" 1; libhq's own addition):
// (L, a + 128, b + 128) / 256 of the unfiltered colour, from its linear RGB (srgb_lin of each
// channel) and the illuminant's reciprocals.  One isotropic scale, so the Euclidean distance
// between two coordinates is dE76 / 256, and under D65 and D50 the sRGB cube lands inside
// [0, 1]^3.  The one statement of the transform: the coordinate kernel, the palette prep and
// hq_assign_coords all call it, so a colour has one coordinate whichever way it arrives.
// The matrix rows are explicit FMA chains, not dot3: the compiler contracts dot3's sum as it
// sees fit in each kernel, and the same colour must get the same bits in all three.
__device__ __forceinline__ float assign_coord_t(float lr, float lg, float lb, const float* m, float inv) {
    return fmaf(lb, m[2], fmaf(lg, m[1], lr * m[0])) * inv;
}
__device__ __forceinline__ float3 assign_coord_lab(float lr, float lg, float lb, const float* inv_illum) {
    const float fx = lab_f_fast(assign_coord_t(lr, lg, lb, c_RGB2XYZ + 0, inv_illum[0]));
    const float fy = lab_f_fast(assign_coord_t(lr, lg, lb, c_RGB2XYZ + 3, inv_illum[1]));
    const float fz = lab_f_fast(assign_coord_t(lr, lg, lb, c_RGB2XYZ + 6, inv_illum[2]));
    return make_float3(fmaf(116.0f, fy, -16.0f) * (1.0f / 256.0f),
                       fmaf(500.0f, fx - fy, 128.0f) * (1.0f / 256.0f),
                       fmaf(200.0f, fy - fz, 128.0f) * (1.0f / 256.0f));
}

// CL:124-145 with true division (setup paths: LabRef, quantize/error image).
__device__ __forceinline__ float3 opp2lab_ref(float o0, float o1, float o2, const float* illum) {
    const float X = dot3(o0, o1, o2, c_Opp2XYZ + 0);
    const float Y = dot3(o0, o1, o2, c_Opp2XYZ + 3);
    const float Z = dot3(o0, o1, o2, c_Opp2XYZ + 6);
    const float fx = lab_f(X / illum[0]), fy = lab_f(Y / illum[1]), fz = lab_f(Z / illum[2]);
    return make_float3(116.0f * fy - 16.0f, 500.0f * (fx - fy), 200.0f * (fy - fz));
}

// CL:201-231: dE76 (distance) or dE94.  Hardware square root (v_sqrt_f32, <= 1 ulp):
// HIP's sqrtf is a correctly rounded ~10-instruction sequence, and the
// reference's OpenCL distance()/sqrt on gfx950 is v_sqrt_f32 itself (ref_len
// below); the cost is compared at 1e-6 relative.
__device__ __forceinline__ float hw_sqrt(float x) { return __builtin_amdgcn_sqrtf(x); }

// ----------------------------------------------------------------------------
// CIEDE2000 (DE = 2): libhq's own addition -- the reference's branch is empty
// (CL:227-230).  Sharma, Wu & Dalal, "The CIEDE2000 color-difference formula:
// implementation notes, supplementary test data, and mathematical
// observations", Color Res. Appl. 30(1), 2005, with kL = kC = kH = 1; sample 1
// is the original's S-CIELAB, sample 2 the candidate (the value is symmetric).
//
// Lowering.  No angle is formed except one small one.  With v_i = (a'_i, b_i),
// C'_i = |v_i|, p = C'_1 C'_2, dot = v_1 . v_2, cross = v_1 x v_2 and
// hd = p + |dot| (= 2 p cos^2(dh'/2) for dot >= 0, 2 p sin^2(dh'/2) for dot < 0):
//   dH' = 2 sqrt(p) sin(dh'/2) = cross sqrt(2 / hd)              (dot >= 0)
//                              = copysign(sqrt(2 hd), cross)      (dot <  0)
//     -- the half-angle form: neither p + dot nor p - dot is ever taken where
//     it cancels.  cross = a'_1 b_2 - b_1 a'_2 with both products rounded: its
//     error 2^-24 p moves dH' by at most 2^-24 sqrt(2 p), the size of C''s own.
//   h-bar' is the circular mean of the two hues in each of Sharma's cases (the
//     +-360 of his table is the wrap), i.e. the direction u = (c, s) of
//     u_1 + u_2 = (C'_2 v_1 + C'_1 v_2) / p, of length sqrt(2 hd / p) for
//     dot >= 0; for dot < 0 that sum cancels, and u is u_1 - u_2 = (C'_2 v_1 -
//     C'_1 v_2) / p (same length formula) turned by +-90 degrees, the sign
//     that of cross.  The formula is discontinuous at opposite hues (dH'
//     changes sign, h-bar' jumps by 180 degrees; Sharma's pairs 10 and 14 sit
//     on it): for cross = 0 exactly the side comes from q itself, which swaps
//     with the samples as cross does, so the value stays symmetric there too.
//   T = 1 - .17 cos(h - 30) + .24 cos 2h + .32 cos(3h + 6) - .20 cos(4h - 63)
//     from (c, s) by the double / triple / quadruple angle products, the phase
//     shifts folded into seven constants.
//   d-theta = 30 exp(-((h - 275) / 25)^2): (c', s') = u turned by -275 degrees,
//     phi = h - 275 = 4 atan(t), t = tan(phi / 4) = s' / (2 ch (1 + ch)), ch =
//     cos(phi / 2) = sqrt((1 + c') / 2); atan by its series to t^9.  For c' <
//     -1/2 (|phi| > 120 degrees) the Gaussian is < e^-23 and is set to 0 (c' is
//     clamped there, so t stays finite); so it is for h in [0, 35) degrees,
//     which Sharma's h-bar' in [0, 360) puts at h - 275 < -240, not at phi =
//     h + 85 (his Gaussian is not periodic: e^-11.6 would remain).
//     R_T = -sin(2 d-theta) R_C with 2 d-theta <= pi / 3 by its series to z^9.
//   x^7 = (x^2)^3 x, and sqrt(x^7 / (x^7 + 25^7)) = rsq(1 + 25^7 rcp(x^7)):
//     0 at x = 0 (rcp = inf, rsq(inf) = 0) and 1 when x^7 overflows.
// C'_1 C'_2 = 0: cross = 0, so dH' = 0; S_H and R_T only ever multiply dH', so
// h-bar' (Sharma: h'_1 + h'_2) is immaterial and any finite u serves (the
// clamps below keep rsq finite: 0 * rsq = 0).  Two greys give |dL| / S_L;
// identical colours give dL = dC' = cross = 0 and sqrt(0) = 0 exactly.
//
// Rounding.  v_sqrt / v_rcp / v_rsq / v_exp are within 1 ulp; every quantity
// above is a sum of a few products of O(1)-conditioned terms, so each of dL /
// S_L, dC' / S_C, dH' / S_H carries a relative error of a few 2^-24 plus the
// absolute 2^-24 C' of a' = (1 + G) a and C' = sqrt(.) (6e-6 at C' = 100,
// divided by S_C >= 5.5 or S_H >= 1.8 there).  u: each component within ~4
// ulp, as dot >= 0 (dot < 0) keeps |u_1 +- u_2| >= sqrt(2); T then within
// ~1e-6 and S_H within 0.015 C' 1e-6.  atan's truncation moves d-theta by <
// 2e-7 degrees (the error t^11 / 11 grows with |phi| while the Gaussian's slope
// dies: worst at phi = 62 degrees), sin's by 1.05^11 / 11! = 4e-8.  The sum
// under the final root is >= 0 in exact arithmetic (|R_T| <= sqrt(3) < 2) and
// is clamped at 0 against rounding.  Measured against a float64 statement:
// DESIGN.md 9.  Finite for every input below 1e9 in magnitude (C'^2 and the
// squares of the three terms stay below FLT_MAX); a NaN or inf input gives
// NaN or inf, which acc_add counts as bad like any other dE's.
// ----------------------------------------------------------------------------
__device__ __forceinline__ float hw_rcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ float hw_rsq(float x) { return __builtin_amdgcn_rsqf(x); }

// sqrt(x^7 / (x^7 + 25^7)), x >= 0
__device__ __forceinline__ float de00_c7(float x) {
    const float x2 = x * x;
    return hw_rsq(fmaf(6103515625.0f, hw_rcp((x2 * x2) * (x2 * x)), 1.0f));
}

__device__ __forceinline__ float ciede2000(float L1, float a1, float b1, float L2, float a2, float b2) {
    constexpr float kTiny = 0x1p-100f;  // keeps rsq finite at C' = 0; below any C'^2 that matters
    // a' = (1 + G) a, G = (1 - sqrt(Cbar^7 / (Cbar^7 + 25^7))) / 2
    const float bb1 = b1 * b1, bb2 = b2 * b2;
    const float cb = 0.5f * (hw_sqrt(fmaf(a1, a1, bb1)) + hw_sqrt(fmaf(a2, a2, bb2)));
    const float g1 = fmaf(-0.5f, de00_c7(cb), 1.5f);
    const float ap1 = g1 * a1, ap2 = g1 * a2;
    const float c1 = hw_sqrt(fmaf(ap1, ap1, bb1)), c2 = hw_sqrt(fmaf(ap2, ap2, bb2));
    const float dL = L2 - L1, dC = c2 - c1;
    const float p = c1 * c2;
    const float dot = fmaf(ap1, ap2, b1 * b2);
    // both products rounded (no contraction into an fma, which would leave one
    // product's rounding error behind): exactly antisymmetric under a swap of the
    // samples, and exactly 0 for identical colours, a zero chroma, equal or opposite hues
    float cross;
    {
#pragma clang fp contract(off)
        cross = ap1 * b2 - b1 * ap2;
    }
    const bool near = dot >= 0.f;  // hues within 90 degrees: u_1 + u_2; else u_1 - u_2
    const float hd = p + fabsf(dot);
    const float rhd = hw_rsq(fmaxf(hd, kTiny));
    const float c1s = near ? c1 : -c1;
    const float un = rhd * hw_rsq(fmaxf(p + p, kTiny));
    const float qx = fmaf(c2, ap1, c1s * ap2) * un, qy = fmaf(c2, b1, c1s * b2) * un;
    // the side of opposite hues: cross's sign; for cross = 0 exactly, a rule that
    // swaps with the samples as cross does (q = u_1 - u_2 does), so that the
    // value stays symmetric on the discontinuity itself
    const float side = copysignf(1.0f, cross != 0.f ? cross : qx != 0.f ? qx : -qy);
    const float dH = near ? 1.41421356f * (cross * rhd) : side * (1.41421356f * (hd * rhd));
    // u = (cc, ss): the mean hue's direction (dot < 0: q turned by +-90 degrees)
    const float cc = near ? qx : -(side * qy);
    const float ss = near ? qy : side * qx;
    const float cx2 = fmaf(cc, cc, -(ss * ss)), sx2 = 2.0f * (cc * ss);
    const float cx3 = fmaf(cx2, cc, -(sx2 * ss)), sx3 = fmaf(sx2, cc, cx2 * ss);
    const float cx4 = fmaf(cx2, cx2, -(sx2 * sx2)), sx4 = 2.0f * (sx2 * cx2);
    float T = fmaf(-0.147224319f, cc, 1.0f);
    T = fmaf(-0.085f, ss, T);
    T = fmaf(0.24f, cx2, T);
    T = fmaf(0.318247007f, cx3, T);
    T = fmaf(-0.0334491082f, sx3, T);
    T = fmaf(-0.0907981f, cx4, T);
    T = fmaf(-0.178201305f, sx4, T);
    // Gaussian of phi = h - 275 degrees
    const float cr = fmaf(0.0871557427f, cc, -0.996194698f * ss);
    const float sr = fmaf(0.0871557427f, ss, 0.996194698f * cc);
    const float ch = hw_sqrt(fmaf(0.5f, fmaxf(cr, -0.5f), 0.5f));
    const float t = sr * hw_rcp(fmaf(ch + ch, ch, ch + ch));
    const float t2 = t * t;
    float at = fmaf(t2, 1.0f / 9.0f, -1.0f / 7.0f);
    at = fmaf(at, t2, 1.0f / 5.0f);
    at = fmaf(at, t2, -1.0f / 3.0f);
    at = fmaf(at, t2, 1.0f);
    at *= t;
    // exp(-(phi / 25 deg)^2), phi = 4 atan t: 2^(-(720 / (25 pi))^2 log2(e) atan^2)
    const float gs = __builtin_amdgcn_exp2f(-121.243864f * (at * at));
    // Sharma's h-bar' runs over [0, 360), so h - 275 over [-275, 85): his Gaussian is
    // not periodic, and hues in [0, 35) degrees (phi in [85, 120)) are on its far side
    const bool off = cr < -0.5f || (ss >= 0.f && cc > 0.f);
    const float z = off ? 0.f : 1.04719755f * gs;  // 2 d-theta in radians
    const float z2 = z * z;
    float sn = fmaf(z2, 1.0f / 362880.0f, -1.0f / 5040.0f);
    sn = fmaf(sn, z2, 1.0f / 120.0f);
    sn = fmaf(sn, z2, -1.0f / 6.0f);
    sn = fmaf(sn * z2, z, z);
    const float cbp = 0.5f * (c1 + c2);
    const float rt = -2.0f * (sn * de00_c7(cbp));
    const float l50 = fmaf(0.5f, L1 + L2, -50.0f), l2 = l50 * l50;
    const float sl = fmaf(0.015f * l2, hw_rsq(20.0f + l2), 1.0f);
    const float sc = fmaf(0.045f, cbp, 1.0f);
    const float sh = fmaf(0.015f * cbp, T, 1.0f);
    const float tl = dL * hw_rcp(sl), tc = dC * hw_rcp(sc), th = dH * hw_rcp(sh);
    const float e2 = fmaf(tl, tl, fmaf(tc, tc, th * fmaf(rt, tc, th)));
    return hw_sqrt(fmaxf(e2, 0.f));
}

template <int DE>
__device__ __forceinline__ float delta_e(float L1, float a1, float b1, float L2, float a2,
                                         float b2) {
    static_assert(DE >= 0 && DE <= 2, "dE types: 0 CIE76, 1 CIE94, 2 CIEDE2000");
    if constexpr (DE == 0) {
        const float dl = L1 - L2, da = a1 - a2, db = b1 - b2;
        return hw_sqrt((dl * dl + da * da) + db * db);
    } else if constexpr (DE == 2) {
        return ciede2000(L1, a1, b1, L2, a2, b2);
    } else {
        const float dL = L1 - L2;
        const float c1 = hw_sqrt(fmaf(a1, a1, b1 * b1));
        const float dC = c1 - hw_sqrt(fmaf(a2, a2, b2 * b2));
        const float da = a1 - a2, db = b1 - b2;
        const float dH = hw_sqrt(fmaf(da, da, db * db) - dC * dC);
        // CL:223-224: double literals, so 1 + 0.045 c1 in double (not fused), stored as float
        const double c1d = (double)c1;
        const float sc = (float)__dadd_rn(1.0, __dmul_rn(0.045, c1d));
        const float sh = (float)__dadd_rn(1.0, __dmul_rn(0.015, c1d));
        return hw_sqrt(fmaf(dL, dL, fmaf(dC / sc, dC / sc, (dH / sh) * (dH / sh))));
    }
}

// dE (CL:201-226) between a reference Lab and the Lab of f = opp2f_fast(...):
// for dE76 each channel's difference is one fma.
template <int DE>
__device__ __forceinline__ float delta_e_f(float Lr, float Ar, float Br, float3 f) {
    if constexpr (DE == 0) {
        const float dl = fmaf(-116.0f, f.y, Lr + 16.0f);
        const float da = fmaf(-500.0f, f.x - f.y, Ar);
        const float db = fmaf(-200.0f, f.y - f.z, Br);
        return hw_sqrt((dl * dl + da * da) + db * db);
    } else {
        return delta_e<DE>(Lr, Ar, Br, fmaf(116.0f, f.y, -16.0f), 500.0f * (f.x - f.y), 200.0f * (f.y - f.z));
    }
}

// (hi, lo) f16 split of x * 2^14 in one dword, hi in bits 0-15: the vertical
// stencil's MFMA data operand (hq_cost.hip), made once per palette by the prep.
constexpr float kVDataScale = 16384.0f;  // 2^14
__device__ __forceinline__ uint32_t split_f16(float x) {
    const float xs = x * kVDataScale;
    const _Float16 hi = (_Float16)xs;
    const _Float16 lo = (_Float16)(xs - (float)hi);
    return (uint32_t)__builtin_bit_cast(uint16_t, hi) |
           ((uint32_t)__builtin_bit_cast(uint16_t, lo) << 16);
}

// CL:256-263 reflection; clamped so garbage coordinates of partial tiles stay
// in bounds (their results are masked).
__device__ __forceinline__ int reflect_clamp(int j, int n) {
    if (j < 0) j = -j - 1;
    if (j >= n) j = 2 * n - j - 1;
    return min(max(j, 0), n - 1);
}

__device__ __forceinline__ int reflect_only(int j, int n) {
    if (j < 0) return -j - 1;
    if (j >= n) return 2 * n - j - 1;
    return j;
}

// The argmin's distance, CL:179-192 `distance(pixel, colour)`, as the
// reference's own OpenCL build computes it on gfx950 (disassembly of its
// quantize / quantizeAndConvertToOpp kernels, compiled unmodified into
// oracle/_ref by oracle/Makefile):
//   d^2 = fma(dw, dw, fma(dz, dz, fma(dy, dy, dx * dx))),  d = p - c,
//   d = v_sqrt_f32(d^2) for FLT_MIN <= d^2 < inf (or NaN),
// and below FLT_MIN (or at +inf) the library's rescaled form: the components
// times 2^86 (2^-66), the same chain, v_sqrt_f32 with its own ldexp 32 / -16
// step for a subnormal sum, and back by 2^-86 (2^66).  v_sqrt_f32 is monotone
// and within 1 ulp, but not correctly rounded (15.1% of the normal floats are 1
// ulp off: scripts/mb/sqrt_probe.hip, profiles/r06_sqrt_probe.json), so two
// different d^2 can share one distance, and then the lower index wins (strict
// <).  The kernels rank by d^2 (dist2_rank: the same chain, so the same
// value) and re-resolve by ref_len any pixel whose runner-up lies within 1e-6
// relative of its best d^2 or below 2^-125 (near_d2).
__device__ __forceinline__ float ref_len_scaled(float dx, float dy, float dz, float dw, bool small) {
    const float s = small ? 0x1p86f : 0x1p-66f;
    const float x = dx * s, y = dy * s, z = dz * s, w = dw * s;
    float e = __builtin_fmaf(w, w, __builtin_fmaf(z, z, __builtin_fmaf(y, y, x * x)));
    const bool den = e < 0x1p-126f;
    e = __builtin_amdgcn_ldexpf(e, den ? 32 : 0);
    float r = __builtin_amdgcn_sqrtf(e);
    r = __builtin_amdgcn_ldexpf(r, den ? -16 : 0);
    return r * (small ? 0x1p-86f : 0x1p66f);
}
__device__ __forceinline__ float ref_len(float dx, float dy, float dz, float dw) {
    const float d2 = __builtin_fmaf(dw, dw, __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx)));
    if (__builtin_expect(!(d2 < 0x1p-126f) && d2 != INFINITY, 1)) return __builtin_amdgcn_sqrtf(d2);
    return ref_len_scaled(dx, dy, dz, dw, d2 < 0x1p-126f);
}
// pixel (r, g, b, 0) against colour c (whose .w is 0 on every argmin path:
// prep_palette / prep_wide clear it, SW:49)
__device__ __forceinline__ float ref_dist(float r, float g, float b, float4 c) {
    return ref_len(r - c.x, g - c.y, b - c.z, -c.w);
}
// pixel and colour as the reference's float4s (the final quantize, CL:147-170)
__device__ __forceinline__ float ref_dist4(float4 p, float4 c) {
    return ref_len(p.x - c.x, p.y - c.y, p.z - c.z, p.w - c.w);
}

// Ranking distance of the pruned argmin: the reference's d^2 (w = 0).
__device__ __forceinline__ float dist2_rank(float r, float g, float b, float4 c) {
    const float dx = r - c.x, dy = g - c.y, dz = b - c.z;
    return __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
}

// A pixel whose ranking by d^2 may differ from the reference's by distance:
// the runner-up within 1e-6 relative of the best d^2 (v_sqrt_f32 can merge d^2
// up to ~4 ulp apart), or itself below 2^-125 (the rescaled form's distance
// is not a function of the underflowed d^2).
__device__ __forceinline__ bool near_d2(float best2, float second2) {
    return second2 <= __builtin_fmaf(best2, 1.0f + 1e-6f, 0x1p-125f);  // (one v_fma, as the plain bound's v_mul)
}

typedef float f32x2 __attribute__((ext_vector_type(2)));

// (byte j of w) << 4 in one instruction (SDWA operand select): a list entry's
// candidate index straight to its 16-byte LDS offset.
__device__ __forceinline__ uint32_t byte_x16(uint32_t w, int j) {
    uint32_t r;
    switch (j) {
    case 0: asm("v_lshlrev_b32_sdwa %0, 4, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_0" : "=v"(r) : "v"(w)); break;
    case 1: asm("v_lshlrev_b32_sdwa %0, 4, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_1" : "=v"(r) : "v"(w)); break;
    case 2: asm("v_lshlrev_b32_sdwa %0, 4, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_2" : "=v"(r) : "v"(w)); break;
    default: asm("v_lshlrev_b32_sdwa %0, 4, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_3" : "=v"(r) : "v"(w)); break;
    }
    return r;
}

// dist2_rank with the x/y differences in one v_pk_add_f32 ({c.x, c.y} sit in
// consecutive registers after the ds_read_b128; rg = {r, g}).  c - p is the
// exact negation of p - c, so the squares and the result are bit-identical.
__device__ __forceinline__ float dist2_rank_pk(f32x2 rg, float b, float4 c) {
    const f32x2 d = f32x2{c.x, c.y} - rg;
    const float dz = c.z - b;
    return __builtin_fmaf(dz, dz, __builtin_fmaf(d.y, d.y, d.x * d.x));
}

typedef float f32x4 __attribute__((ext_vector_type(4)));
// operands and accumulator of v_mfma_f32_16x16x32_f16 (both cost files' vertical passes)
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4v __attribute__((ext_vector_type(4)));

template <typename V>
__device__ __forceinline__ V wave_sum(V v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// ---- shared by the per-colour sums (hq_centroid.hip, hq_errsum.hip, hq_hist.hip) ----
// The sum of a 64-bit integer over the wave, in every lane.
__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// Four consecutive indices of an index image, widened to 32 bits: one aligned
// load of 4, 8 or 16 bytes.
__device__ __forceinline__ uint4 load_idx4(const uint8_t* p) {
    const uint32_t v = *reinterpret_cast<const uint32_t*>(p);
    return make_uint4(v & 0xffu, (v >> 8) & 0xffu, (v >> 16) & 0xffu, v >> 24);
}
__device__ __forceinline__ uint4 load_idx4(const uint16_t* p) {
    const uint2 v = *reinterpret_cast<const uint2*>(p);
    return make_uint4(v.x & 0xffffu, v.x >> 16, v.y & 0xffffu, v.y >> 16);
}
__device__ __forceinline__ uint4 load_idx4(const uint32_t* p) { return *reinterpret_cast<const uint4*>(p); }

// q(v) = RN(v 2^32), ties to even, for v in [0, 1]: v 2^32 is exact in fp32 (a
// power-of-two scaling), already an integer from v = 2^-9 on, and at most 2^32,
// which is the one value past 32 bits.
__device__ __forceinline__ uint64_t unit_q32(float v) {
    const float x = rintf(v * 4294967296.0f);
    return x >= 4294967296.0f ? (1ull << 32) : (uint64_t)(uint32_t)x;
}

// Sum of a double over the wave with DPP moves only (no LDS round trips: the
// __shfl_down tree above is 12 dependent ds_bpermute for an f64).  Fixed order:
// row_shr 1, 2, 4, 8 leave each 16-lane row's sum in its lane 15; row_bcast 15
// and 31 fold the rows into lane 63, which alone holds the total.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_f64(double v) {
    const uint64_t u = __builtin_bit_cast(uint64_t, v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)u, CTRL, ROW_MASK, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)(u >> 32), CTRL, ROW_MASK, 0xf, true);
    return __builtin_bit_cast(double, ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}

__device__ __forceinline__ double wave_sum_to_lane63(double v) {
    v += dpp_f64<0x111, 0xf>(v);  // row_shr:1
    v += dpp_f64<0x112, 0xf>(v);  // row_shr:2
    v += dpp_f64<0x114, 0xf>(v);  // row_shr:4
    v += dpp_f64<0x118, 0xf>(v);  // row_shr:8
    v += dpp_f64<0x142, 0xa>(v);  // row_bcast:15 into rows 1 and 3
    v += dpp_f64<0x143, 0xc>(v);  // row_bcast:31 into rows 2 and 3
    return v;
}

// k/255 exactly as the host's float division makes it, from byte j of v: the
// product with RN(1/255) is off by one ulp for 126 of the 256 values; one FMA
// residual step corrects all 256 (checked exhaustively, tests/test_assign_u8.py).
__device__ __forceinline__ float u8_unit(uint32_t v, int j) {
    const float k = (float)((v >> (8 * j)) & 0xffu);
    const float c = 1.0f / 255.0f;
    const float q = k * c;
    const float r = __builtin_fmaf(-q, 255.0f, k);
    return __builtin_fmaf(r, c, q);
}

// ----------------------------------------------------------------------------
// The dE sum of a palette (IM:736-768) as a fixed-point integer sum: each
// fp64 partial x (a wave's part of a cost16w tile, a tile of the other tiled
// kernels, or 256 pixels of the generic path) adds
// v = RN(x 2^20) to kAccSlots slot counters of 64 bits (slot = its index mod
// kAccSlots, which spreads the atomics), split as v mod 2^32 into `lo` and
// v >> 32 into `hi` so neither can overflow (2^32 partials of < 2^43).
// Integer addition is associative: the total is the same bits whatever order
// the workgroups finish in, so no partial array and no ordered fold are needed
// (round 3 stored [P][tiles] partials and summed them in a fixed order in
// finalize or the SA step).  Resolution 2^-20 per partial: < 1e-10 relative at
// 4096^2.  A partial that is not a finite number in [0, 2^43) (a NaN pixel,
// an absurd palette) counts in `bad` and makes the sum NaN.
// Layout: [kAccSlots][acc_pitch(P)][4] u64: lo, hi, bad, (pad).
// ----------------------------------------------------------------------------
constexpr double kAccScale = 1048576.0;  // 2^20
__device__ __forceinline__ void acc_add(uint64_t* acc, int P, int p, int slot, double x) {
    uint64_t* a = acc + ((int64_t)(slot & (kAccSlots - 1)) * acc_pitch(P) + p) * 4;
    if (x >= 0.0 && x < 8796093022208.0) {  // 2^43 (NaN fails the test)
        const uint64_t v = (uint64_t)__double2ull_rn(x * kAccScale);
        atomicAdd((unsigned long long*)(a + 0), (unsigned long long)(v & 0xffffffffull));
        if (v >> 32) atomicAdd((unsigned long long*)(a + 1), (unsigned long long)(v >> 32));
    } else {
        atomicAdd((unsigned long long*)(a + 2), 1ull);
    }
}
// The total of palette p (any thread; kAccSlots x 3 loads, issued together).
__device__ __forceinline__ double acc_total(const uint64_t* acc, int P, int p) {
    uint64_t lo = 0, hi = 0, bad = 0;
#pragma unroll
    for (int sl = 0; sl < kAccSlots; ++sl) {
        const uint64_t* a = acc + ((int64_t)sl * acc_pitch(P) + p) * 4;
        lo += a[0];
        hi += a[1];
        bad += a[2];
    }
    // hi 2^12 and lo 2^-20 are exact doubles (hi < 2^41, lo < 2^53): one rounding
    return bad ? __builtin_nan("") : (double)hi * 4096.0 + (double)lo * (1.0 / kAccScale);
}

// Candidate-grid box bounds (build_grid, hq_search.hip; the 16-bit lists,
// hq_lists16.hip).
// Box bounds in fp32.  Box edges are multiples of 1/G (G a power of two):
// exact.  Valid colours are finite (prep_palette routes non-finite palettes to
// the exhaustive path), so every term is a correctly rounded difference,
// squared and summed with non-negative terms: each bound is within 3 ulp
// (2e-7 relative) of its exact value, and the 1e-5 margin covers that on
// both sides of the test on top of the reference's own 1.1e-6.  An fp32
// overflow (|colour| > 1e19) gives inf bounds: T = inf makes every colour a
// candidate, which overflows the list into the exhaustive loop.  (fp64 was
// ~570 VALU instructions per wave at half the fp32 rate.)
__device__ __forceinline__ float ax_min2(float c, float lo, float hi) {
    const float d = fmaxf(fmaxf(lo - c, c - hi), 0.f);
    return d * d;
}
__device__ __forceinline__ float ax_max2(float c, float lo, float hi) {
    const float d = fmaxf(c - lo, hi - c);
    return d * d;
}

#define HQ_CAND_MARGIN (1.0f + 1e-5f)

// ----------------------------------------------------------------------------
// XCD-aware relabelling of a 1-D grid of N workgroups.  Workgroups are placed
// round-robin over the 8 XCDs (b % 8), so XCD x is given the contiguous work
// range starting at x*(N/8) + min(x, N%8): neighbouring work items (the P
// palettes of one tile or pixel block, adjacent tiles) then meet in one L2 and
// LabRef / RGB reach HBM once instead of once per palette.  Bijective for any N;
// placement only affects speed, never results.
__device__ __forceinline__ int xcd_remap(int b, int N) {
    const int q = N >> 3, r = N & 7, x = b & 7, s = b >> 3;
    return x * q + min(x, r) + s;
}

}  // namespace hq
