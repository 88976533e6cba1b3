// hq_cost_layout.h -- what the cost kernels (hq_cost.hip, hq_cost_generic.hip)
// and the host's table builders (hq_cost_taps.cpp) must agree on, and the
// builders' prototypes.  Plain C++ for both the host compiler and hipcc (which
// takes a constexpr function for host and device alike).
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace hq {

constexpr int kNumFilt = 7;  // separable filter pairs of the S-CIELAB stencil

// Opp->XYZ (CL:118)
#define HQ_OPP2XYZ {0.624045f, -1.87044f, -0.155304f, 1.36606f, 0.931563f, \
                   0.433903f, 1.5013f,   1.41761f,  2.53307f}

// The fast path's tap buckets: a filter of half-width H (halfSize, IM:408) runs
// centred in the smallest that holds it (fast_bucket), zeros around.  72 dpi /
// 45 cm (the default) is H = 10, 150 dpi / 30 cm 15, 96 dpi / 60 cm 19.
constexpr int kFastBuckets[4] = {10, 15, 19, 24};

template <int HALF>
struct CostTaps {
    float v[kNumFilt][2 * HALF + 1];
    float h[kNumFilt][2 * HALF + 1];
};

// The matrix-core vertical pass works on f16 (hi, lo) splits: taps x 2^16,
// inputs x 2^14; the 2^30 total scale is folded into the horizontal taps,
// exactly (a power of two).
constexpr float kVTapScale = 65536.0f;                      // 2^16
constexpr float kVOutScale = 1.0f / (16384.0f * 65536.0f);  // 2^-30
// The largest |tap| whose hi part stays finite: tap x 2^16 <= 65504, f16's
// largest finite value (0.99951171875; the largest designed tap, the centre of
// k1.x at 4 dpi / 45 cm, is 0.986).  A caller's filter set with a tap beyond
// it, or a non-finite one, takes the fp32 forms (taps_fit_split, checked at
// hq_set_filters), as a palette outside the split range does.
constexpr float kVTapMax = 65504.0f / kVTapScale;

// Region row of K slot (g = lane >> 4, j) of the vertical pass's B operand.
// Half 0 (output rows 0-7): rows 4j + g (lane group g holds every 4th row).
// Half 1 (output rows 8-15 of a 16-row tile, rows 8-39): slots 2-7 are half
// 0's slots 2-7 (rows 8-31), slots 0 and 1 are rows 32 + g and 36 + g (rows
// 36-39 carry zero taps, so slot 1 needs no gather: 0).  Every lane gathers one
// new value for half 1, and half 1's B operand is half 0's with only its first
// dword replaced (pack_b_halves).  The A fragments permute K to match.
constexpr int kv_row(int half, int g, int j) {
    return half == 0 || j >= 2 ? 4 * j + g : (j == 0 ? 32 + g : 36 + g);
}

// Region row of K slot (g, j) of step s for output-row half `half` (see above).
constexpr int kv_row_s(int half, int s, int g, int j) {
    return half == 0 || j >= 2 ? 32 * s + 4 * j + g : 32 * (s + 1) + 4 * j + g;
}

// Significant half-windows of the narrow k1.x / k1.y / k1.z filters per bucket:
// the largest over every geometry whose H falls in the bucket (checked per
// filter set at hq_set_filters: trim_window_ok; the windows of 18 dpi x 13
// distance settings were swept with the oracle's filter design, SP:66-254).
constexpr int trim_w(int HB, int ch) {
    return HB == 10 ? (ch == 0 ? 3 : ch == 1 ? 4 : 5)
         : HB == 15 ? (ch == 0 ? 4 : ch == 1 ? 5 : 7)
         : HB == 19 ? (ch == 0 ? 5 : ch == 1 ? 7 : 9)
                    : (ch == 0 ? 6 : ch == 1 ? 9 : 12);
}

// MFMA K steps per output-row half over a bucket's 8 + 2 HB region rows: of 32
// rows (cost_mfma_kernel, cost16w at HB = 10) or 16 (the (hi, lo) pair layout
// above HB = 10); gen_vmfma's steps of 16 over a 16-row block's 16 + 2 H rows.
constexpr int bucket_steps(int HB) { return (8 + 2 * HB + 31) / 32; }
constexpr int pair_steps(int HB) { return (8 + 2 * HB + 15) / 16; }
constexpr int vtile_pair_steps(int H) { return (16 + 2 * H + 15) / 16; }

// ---- the table builders (hq_cost_taps.cpp) ------------------------------------
int fast_bucket(int half);
bool trim_window_ok(const float* k1, int H, int HB);
bool taps_fit_split(const float* k1, const float* k2, const float* k3, const float* absk3, int taps);
void opp2xyz_over_illum(const float inv_illum[3], float m[9]);
int bad_illum_component(const float illum[3]);
void build_fast_taps(int HB, int H, const float* k1, const float* k2, const float* k3, const float* absk3,
                     void* out);
size_t vpass_f16_stack_fragment_halves(int HB);
void build_vpass_f16_stack_fragments(int HB, int H, const float* k1, const float* k2, const float* k3,
                                     const float* absk3, uint16_t* out);
size_t vpass_f16_pair_fragment_halves(int HB);
void build_vpass_f16_pair_fragments(int HB, int H, const float* k1, const float* k2, const float* k3,
                                    const float* absk3, uint16_t* out);
size_t vtile_dup_tap_words(int H);
void build_vtile_dup_taps(int H, const float* k1, const float* k2, const float* absk3, uint32_t* out);

}  // namespace hq
