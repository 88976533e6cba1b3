// hq_grad.h -- the palette gradient of the S-CIELAB cost (hq_cost_gradient, hq.h):
// the arguments and launchers of hq_grad.hip, for that unit and the evaluation (hq_eval.hip), and
// the host half -- the fixed-point shift and the chain rule -- that the runtime and the
// stand-alone check program share.  Not part of the public ABI.
#pragma once

#include <math.h>
#include <stdint.h>

namespace hq {

// ---- the host half (plain C++: no HIP type below this line's block) ----------------
// A bound on |a_c(x)|, the adjoint-blurred pointwise term, from the Opp->Lab matrix m (rows
// divided by the illuminant, opp2xyz_over_illum) and the taps ([T][4] k1, k2; [T] k3, |k3|):
//   |dE/df_r| <= (500, 116 + 500 + 200, 200) since (Lab - LabRef) / E is a unit vector,
//   f' <= kappa / 116 = 1 / (3 delta^2) on both branches (CL:124-145),
//   |g_c| <= f'max sum_r w_r |m[r][c]|,
//   a reflecting 1-D pass's transpose has at most three sources per tap, so
//   |a_c| <= max_c' |g_c'| ... per channel: |g_c| sum_j (3 sum |v_j|) (3 sum |h_j|).
// grad_shift: the largest s with 2^30 pixels of |a| 2^s below 2^62, capped at 30.
inline double grad_bound(const float m[9], const float* k1, const float* k2, const float* k3, const float* absk3,
                         int taps) {
    const double w[3] = {500.0, 816.0, 200.0}, fmax = 24389.0 / 27.0 / 116.0;
    double bound = 0.0;
    for (int c = 0; c < 3; ++c) {
        double g = 0.0, s1 = 0.0, s2 = 0.0, s3v = 0.0, s3h = 0.0;
        for (int r = 0; r < 3; ++r) g += w[r] * fabs((double)m[3 * r + c]);
        for (int t = 0; t < taps; ++t) {
            s1 += fabs((double)k1[4 * t + c]);
            s2 += fabs((double)k2[4 * t + c]);
            s3v += fabs((double)absk3[t]);
            s3h += fabs((double)k3[t]);
        }
        const double f = 9.0 * (s1 * s1 + s2 * s2 + (c == 0 ? s3v * s3h : 0.0));
        bound = fmax * g * f > bound ? fmax * g * f : bound;
    }
    return bound;
}
constexpr int kGradNoShift = -1000;  // a bound that is not a positive number below 2^90: no shift serves
inline int grad_shift(double bound) {
    if (!(bound > 0.0) || !(bound < 0x1p90)) return kGradNoShift;
    int e = 0;
    (void)frexp(bound, &e);  // bound < 2^e
    const int s = 32 - e;    // 2^30 2^e 2^s = 2^62
    return s > 30 ? 30 : s;
}

#if defined(__HIPCC__)
#define HQ_GRAD_HD __host__ __device__
#else
#define HQ_GRAD_HD
#endif

// d srgb_lin / dx of the branch srgb_lin takes (CL:85-87)
HQ_GRAD_HD inline double srgb_lin_slope(double x) {
    return x <= (double)0.04045f ? 1.0 / (double)12.92f
                                 : (double)2.4f / (double)1.055f * pow((x + (double)0.055f) / (double)1.055f, (double)2.4f - 1.0);
}

// The move of one channel of one colour, the one statement of it for the host's chain rule and
// step (grad_chain, descend_step) and the search's kernel (descend_update_kernel, hq_search.hip):
//   g = (sum_c ldexp(S_c, -shift) rgb2opp[c][ch]) srgb_lin'(x) / den
//   x' = clamp(x - rate g scale / n, 0, 1) in double, stored as float; x's bits when that is not finite.
// *grad (may be null) receives g.  The host's pair: den = N gives dC/dx, and the step takes that
// gradient back (s null: g is given) with scale = N.  The kernel: den = scale = 1, exact, so
// x' = clamp(x - rate srgb_lin'(x) (sum) / n, 0, 1) -- N cancels.  Nothing is contracted.
HQ_GRAD_HD inline float descend_channel(const int64_t* s, int shift, const double* rgb2opp, int ch, float x, double den,
                                        double g, double rate, double scale, double n, double* grad) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (s) {
        double v = 0.0;
        for (int c = 0; c < 3; ++c) v += ldexp((double)s[c], -shift) * rgb2opp[3 * c + ch];
        g = v * srgb_lin_slope((double)x) / den;
    }
    if (grad) *grad = g;
    if (!(n > 0.0)) return x;
    const double v = (double)x - rate * g * scale / n;
    if (!isfinite(v)) return x;
    return (float)fmin(fmax(v, 0.0), 1.0);
}

// The chain rule of one palette: sums [K][4] (S_0, S_1, S_2 in units of 2^-shift, n), pal [K][4]
// the colours whose opponent table the kernels read -> grad [K][4] (dC/dR, dC/dG, dC/dB, n).
// A colour without pixels: zeros.  rgb2opp: row-major [3][3], opp_c = sum_ch rgb2opp[c][ch] lin_ch.
inline void grad_chain(const int64_t* sums, const float* pal, int K, double n_pixels, int shift,
                       const double rgb2opp[9], double* grad) {
    for (int k = 0; k < K; ++k) {
        const int64_t* s = sums + 4 * k;
        double* g = grad + 4 * k;
        g[3] = (double)s[3];
        for (int ch = 0; ch < 3; ++ch) {
            g[ch] = 0.0;
            if (s[3] > 0) (void)descend_channel(s, shift, rgb2opp, ch, pal[4 * k + ch], n_pixels, 0.0, 0.0, 0.0, 0.0, &g[ch]);
        }
    }
}

// The descent step of one palette (hq_descend_population's rule, hq.h): for each colour k >= nfixed
// with n > 0, candidate = clamp(pal - rate grad N / n, 0, 1) in double, stored as float; every
// other colour keeps its bits.  Returns whether any bit changed.
bool descend_step(const float* pal, const double* grad, int K, int nfixed, double n_pixels, double rate,
                  float* cand);

}  // namespace hq

#ifdef __HIPCC__
#include "hq_launch.h"

namespace hq {

constexpr int kGradMaxHalfTiled = 24;  // the tiled form's half-widths (the fast cost path's)
// grad_pixel_kernel's tile and grad_adjoint_kernel's (columns x rows), 256 threads each
constexpr int kGradTW = 32, kGradPixTH = 32, kGradAdjTH = 16;

struct GradArgs {
    const uint8_t* idx;   // [P][idx_pitch] the u8 index images of the whole image
    const float4* opp;    // [P][256] the palettes' opponent tables
    const float* k1;      // [T][4]
    const float* k2;      // [T][4]
    const float* k3;      // [T]
    const float* absk3;   // [T]
    const float* labL;    // planar LabRef, pitch lab_pitch
    const float* labA;
    const float* labB;
    float* t;             // the plain pair: [7][N] scratch of one palette (both directions use it)
    float4* g;            // [P][N] the pointwise term (x, y, z, 0)
    unsigned long long* sums;  // [P][K][4] S_0, S_1, S_2 as llrint(a 2^shift), n (zeroed before the launch)
    int64_t idx_pitch;
    int W, H, lab_pitch;
    int P, K, half;
    float scale;          // 2^shift
    float m_lab[9];       // Opp->XYZ rows / illuminant (opp2xyz_over_illum)
};

// hq_grad.hip.  The plain pair: any half-width, one thread per pixel, one palette after another
// through a.t.  The tiled form: half <= kGradMaxHalfTiled, two launches for the population.
// ev_* (profiling, may be null): the pixel stage's pair and the adjoint stage's.
hipError_t launch_grad_plain(const GradArgs&, hipStream_t, hipEvent_t ev_pix[2], hipEvent_t ev_adj[2]);
hipError_t launch_grad_tiled(const GradArgs&, hipStream_t, hipEvent_t ev_pix[2], hipEvent_t ev_adj[2]);
// The tiled kernels' dynamic LDS granted at this half-width now (a search does it before its run is
// captured); false: the runtime refused, and the launcher will return its error.
bool grad_tiled_grant(int half);
size_t grad_pixel_lds(int half);
size_t grad_adjoint_lds(int half);

}  // namespace hq
#endif
