// hq_cost_taps.cpp -- the cost kernels' host-built tables: bucket tap tables,
// the vertical pass's split-f16 MFMA fragments and duplicated tap rows, the
// trim check, the Opp->Lab matrix.  Host compiler only (Java float semantics,
// no contraction), no HIP: links alone into a CPU program.
#include "hq_cost_layout.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace hq {

// Opp->XYZ (CL:118) with row r divided by the illuminant's component r
// (lab_f_fast works on t = X/Xn, Y/Yn, Z/Zn).
void opp2xyz_over_illum(const float inv_illum[3], float m[9]) {
    static const float opp2xyz[9] = HQ_OPP2XYZ;
    for (int i = 0; i < 9; ++i) m[i] = (float)((double)opp2xyz[i] * inv_illum[i / 3]);
}

// The first component (0 .. 2) of an illuminant that is not finite and greater than 0; -1: none.
// (-0.0f, 0.0f, negative values, NaN and the infinities all fail `finite and > 0`: 1 / Xn must
// be a positive finite scale of the Opp->XYZ row.)
int bad_illum_component(const float illum[3]) {
    for (int i = 0; i < 3; ++i)
        if (!(std::isfinite(illum[i]) && illum[i] > 0.0f)) return i;
    return -1;
}

// The smallest tap bucket that holds a filter of half-width `half`; 0 = none (the generic path).
int fast_bucket(int half) {
    for (const int HB : kFastBuckets)
        if (half <= HB) return HB;
    return 0;
}

// The 7 filters (f: 0 k1.x, 1 k2.x, 2 k3 (|k3| vertical), 3 k1.y, 4 k2.y,
// 5 k1.z, 6 k2.z) of half-width H centred in 2 HB + 1 taps (zeros around):
// v[f][d], h[f][d], d = 0 .. 2 HB, row-major [7][2 HB + 1].
static void bucket_taps(const float* k1, const float* k2, const float* k3, const float* absk3, int H,
                        int HB, std::vector<float>& v, std::vector<float>& h) {
    const int T = 2 * HB + 1, off = HB - H;
    v.assign(kNumFilt * T, 0.f);
    h.assign(kNumFilt * T, 0.f);
    for (int i = 0; i < 2 * H + 1; ++i) {
        const int d = i + off;
        const float vv[7] = {k1[4 * i], k2[4 * i], absk3[i], k1[4 * i + 1], k2[4 * i + 1], k1[4 * i + 2], k2[4 * i + 2]};
        const float hh[7] = {k1[4 * i], k2[4 * i], k3[i], k1[4 * i + 1], k2[4 * i + 1], k1[4 * i + 2], k2[4 * i + 2]};
        for (int f = 0; f < kNumFilt; ++f) {
            v[f * T + d] = vv[f];
            h[f * T + d] = hh[f];
        }
    }
}

// f32 -> f16 bits, round to nearest even (host; finite inputs well inside the
// f16 range after scaling, subnormal results included).
static uint16_t host_f16(float x) {
    uint32_t u;
    std::memcpy(&u, &x, 4);
    const uint32_t sign = (u >> 16) & 0x8000u;
    const float ax = std::fabs(x);
    if (ax < 5.9604645e-08f * 0.5f) return (uint16_t)sign;          // below half the smallest subnormal
    if (ax < 6.1035156e-05f) {                                        // f16 subnormal: multiples of 2^-24
        const float q = std::nearbyint(ax * 16777216.0f);             // round-half-even (default mode)
        return (uint16_t)(sign | (uint32_t)q);
    }
    uint32_t a = u & 0x7fffffffu;
    const uint32_t mant = a & 0x7fffffu;
    int32_t e = (int32_t)(a >> 23) - 127 + 15;
    uint32_t m = mant >> 13, rem = mant & 0x1fffu;
    if (rem > 0x1000u || (rem == 0x1000u && (m & 1u))) {
        if (++m == 0x400u) { m = 0; ++e; }
    }
    return (uint16_t)(sign | ((uint32_t)e << 10) | m);
}

static float host_f16_to_f32(uint16_t h) {
    const uint32_t e = (h >> 10) & 0x1fu, m = h & 0x3ffu;
    const float v = e == 0 ? std::ldexp((float)m, -24) : std::ldexp((float)(m | 0x400u), (int)e - 25);
    return (h & 0x8000u) ? -v : v;
}

// A vertical tap as the matrix-core pass holds it: w x 2^16 = hi + lo, both f16.
struct SplitTap { uint16_t hi, lo; };
static SplitTap split_vtap(float w) {
    w *= kVTapScale;
    const uint16_t hi = host_f16(w);
    return {hi, host_f16(w - host_f16_to_f32(hi))};
}

// The filters of the vertical pass's four MFMA stacks (output rows 0-7, 8-15 of A; -1: none)
constexpr int kStack[4][2] = {{0, 1}, {2, -1}, {3, 4}, {5, 6}};
// What an A fragment holds for filter f at bucket tap d of the tv[7][2 HB + 1]
// bucket_taps: zero for no filter, outside [0, 2 HB] and, with trim, outside
// the significant window of a narrow filter (f = 0, 3, 5: k1.x, k1.y, k1.z).
static SplitTap fragment_tap(const std::vector<float>& tv, int HB, int f, int d, bool trim) {
    const int T = 2 * HB + 1;
    float w = 0.f;
    if (f >= 0 && d >= 0 && d < T) {
        w = tv[f * T + d];
        const int ch = f == 0 ? 0 : (f == 3 ? 1 : (f == 5 ? 2 : -1));
        if (trim && ch >= 0 && std::abs(d - HB) > trim_w(HB, ch)) w = 0.f;
    }
    return split_vtap(w);
}

// Split-f16 A fragments of v_mfma_f32_16x16x32_f16 for the vertical pass,
// [trim][half][step][stack][hi, lo][lane] x 8 halves (trim 0 = all taps, 1 =
// the narrow filters' significant windows).  Lane l holds A[i = l & 15][k = 8g
// + j], g = l >> 4: the tap (x 2^16) of filter stack[i >> 3] that multiplies
// the region row held in K slot k of step s into output row 8 half + (i & 7),
// i.e. bucket tap d = row - 8 half - (i & 7), zero outside [0, 2 HB] (and
// outside the trimmed window).  The region row of K slot (g, j) is
// kv_row_s(half, s, g, j): half 1 (output rows 8-15 of a 16-row tile) reuses
// six of half 0's slots per lane, so its B operand costs two gathered values
// per lane per step instead of eight.  At HB = 10 (one step) this is also the
// layout cost_mfma_kernel reads (half 0 only).
size_t vpass_f16_stack_fragment_halves(int HB) { return (size_t)2 * 2 * bucket_steps(HB) * 4 * 2 * 64 * 8; }

void build_vpass_f16_stack_fragments(int HB, int H, const float* k1, const float* k2, const float* k3,
                                     const float* absk3, uint16_t* out) {
    std::vector<float> tv, th;
    bucket_taps(k1, k2, k3, absk3, H, HB, tv, th);
    const int S = bucket_steps(HB);
    for (int trim = 0; trim < 2; ++trim)
        for (int half = 0; half < 2; ++half)
            for (int s = 0; s < S; ++s)
                for (int st = 0; st < 4; ++st)
                    for (int l = 0; l < 64; ++l)
                        for (int j = 0; j < 8; ++j) {
                            const int i = l & 15, g = l >> 4;
                            const int d = kv_row_s(half, s, g, j) - 8 * half - (i & 7);
                            const SplitTap w = fragment_tap(tv, HB, kStack[st][i >> 3], d, trim);
                            const size_t base = (((((size_t)trim * 2 + half) * S + s) * 4 + st) * 2) * 64;
                            out[((base + 0 * 64) + l) * 8 + j] = w.hi;
                            out[((base + 1 * 64) + l) * 8 + j] = w.lo;
                        }
}

// cost16w's A fragments in the (hi, lo) pair layout (see vblock_pair):
// [trim][u][stack][hi, lo][lane] x 8 halves.  Lane l holds A[i = l & 15][k =
// 8 g + 2 j + e], g = l >> 4: K slots 2 j and 2 j + 1 both stand for region row
// 4 (4 u + j) + g (the gathered dword of that row is its (hi, lo) f16 pair), so
// both hold the same tap part -- the tap's hi half in fragment hl = 0, its lo
// half in hl = 1 -- of filter stack[i >> 3] for output row i & 7: bucket tap d =
// row - (i & 7), zero outside [0, 2 HB] (and outside the trimmed window).  Half
// 1 (output rows 8-15) reads the rows 8 further on with the same fragments.
size_t vpass_f16_pair_fragment_halves(int HB) { return (size_t)2 * pair_steps(HB) * 4 * 2 * 64 * 8; }

void build_vpass_f16_pair_fragments(int HB, int H, const float* k1, const float* k2, const float* k3,
                                    const float* absk3, uint16_t* out) {
    std::vector<float> tv, th;
    bucket_taps(k1, k2, k3, absk3, H, HB, tv, th);
    const int U = pair_steps(HB);
    for (int trim = 0; trim < 2; ++trim)
        for (int u = 0; u < U; ++u)
            for (int st = 0; st < 4; ++st)
                for (int l = 0; l < 64; ++l)
                    for (int kk = 0; kk < 8; ++kk) {
                        const int i = l & 15, g = l >> 4;
                        const int d = 4 * (4 * u + (kk >> 1)) + g - (i & 7);
                        const SplitTap w = fragment_tap(tv, HB, kStack[st][i >> 3], d, trim);
                        const size_t base = ((((size_t)trim * U + u) * 4 + st) * 2) * 64;
                        out[((base + 0 * 64) + l) * 8 + kk] = w.hi;
                        out[((base + 1 * 64) + l) * 8 + kk] = w.lo;
                    }
}

// gen_vmfma's A operands come from duplicated tap rows (below): in the pair
// layout lane l = (m = l & 15, g = l >> 4) needs, in K slots 2 j + h of step s,
// part h of tap t = 16 s + 4 g + j - m -- a window sliding over the taps.
// gen_vmfma's tap rows: [7][hi, lo][TP = 16 S + 16] dwords, entry i the part of
// tap i - 15 x 2^16 in both halves (zero outside 0 .. 2 H): A of step s for
// lane (m, g) is entries 16 s + 4 g - m + 15 .. + 3 of the filter's rows.
size_t vtile_dup_tap_words(int H) { return (size_t)kNumFilt * 2 * (16 * vtile_pair_steps(H) + 16); }
void build_vtile_dup_taps(int H, const float* k1, const float* k2, const float* absk3, uint32_t* out) {
    const int TP = 16 * vtile_pair_steps(H) + 16, T = 2 * H + 1;
    for (int f = 0; f < kNumFilt; ++f)
        for (int i = 0; i < TP; ++i) {
            const int t = i - 15;
            float w = 0.f;
            if (t >= 0 && t < T) w = f < 3 ? k1[4 * t + f] : f < 6 ? k2[4 * t + f - 3] : absk3[t];
            const SplitTap p = split_vtap(w);
            out[((size_t)f * 2 + 0) * TP + i] = p.hi | ((uint32_t)p.hi << 16);
            out[((size_t)f * 2 + 1) * TP + i] = p.lo | ((uint32_t)p.lo << 16);
        }
}

// The narrow k1 filters' taps outside the bucket's trimmed windows are below
// 1e-9 of their peak (then the fast path may skip them; else it runs all taps).
bool trim_window_ok(const float* k1, int H, int HB) {
    for (int ch = 0; ch < 3; ++ch) {
        float peak = 0.f;
        for (int t = 0; t < 2 * H + 1; ++t) peak = std::max(peak, std::fabs(k1[4 * t + ch]));
        for (int t = 0; t < 2 * H + 1; ++t)
            if (std::abs(t - H) > trim_w(HB, ch) && std::fabs(k1[4 * t + ch]) > 1e-9f * peak) return false;
    }
    return true;
}

// Every tap of the set is finite and within kVTapMax: the split-f16 tables
// (split_vtap: the bucket fragments, gen_vmfma's and gen_hmfma's tap rows) hold
// it.  Else tap x 2^16 rounds to f16's infinity and the matrix-core passes
// return a non-finite cost: such a set runs on the fp32 forms.
bool taps_fit_split(const float* k1, const float* k2, const float* k3, const float* absk3, int taps) {
    const auto fits = [](float w) { return std::fabs(w) <= kVTapMax; };  // (false for NaN)
    for (int t = 0; t < taps; ++t) {
        for (int ch = 0; ch < 3; ++ch)
            if (!fits(k1[4 * t + ch]) || !fits(k2[4 * t + ch])) return false;
        if (!fits(k3[t]) || !fits(absk3[t])) return false;
    }
    return true;
}

// [0] the bucket's taps as designed, [1] the same with the horizontal taps
// scaled by 2^-30 (exact) for the matrix-core vertical pass, whose outputs
// carry 2^30.  Layout: two CostTaps<HB>.
void build_fast_taps(int HB, int H, const float* k1, const float* k2, const float* k3, const float* absk3,
                     void* out) {
    std::vector<float> tv, th;
    bucket_taps(k1, k2, k3, absk3, H, HB, tv, th);
    const size_t n = tv.size();  // == sizeof(CostTaps<HB>) / 8
    float* o = static_cast<float*>(out);
    for (int copy = 0; copy < 2; ++copy, o += 2 * n) {
        std::memcpy(o, tv.data(), n * sizeof(float));
        for (size_t i = 0; i < n; ++i) o[n + i] = copy ? th[i] * kVOutScale : th[i];
    }
}

}  // namespace hq
