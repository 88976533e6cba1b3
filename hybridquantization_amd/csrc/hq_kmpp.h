// hq_kmpp.h -- k-means++ seeding of a population (hq_kmeanspp_seed, hq.h): the
// arguments and launchers of hq_kmpp.hip, for that unit and the runtime (hq_runtime.hip), and the
// two integer rules host and device share -- the random word and a channel's value.  Not part of
// the public ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define HQ_KMPP_HD __host__ __device__
#else
#define HQ_KMPP_HD
#endif

namespace hq {

// u(p, r): the first output of a SplitMix64 generator whose state is seed + (p << 32) + r
// (mod 2^64) -- hq.h states the constants.
HQ_KMPP_HD inline uint64_t kmpp_word(uint64_t seed, uint32_t p, uint32_t r) {
    uint64_t z = seed + ((uint64_t)p << 32) + (uint64_t)r + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// q(v) of a float channel on a scale S (4095: the planar image; 255: a fixed colour next to the
// packed image's bytes): RN of the fp32 product clamp(v, 0, 1) S, ties to even; a NaN counts as 0.
constexpr float kKmppScale = 4095.0f;
HQ_KMPP_HD inline int32_t kmpp_q(float v, float scale) {
    const float c = fminf(fmaxf(v, 0.0f), 1.0f);  // (fmaxf(NaN, 0) = 0)
    return (int32_t)rintf(c * scale);
}

constexpr uint32_t kKmppSentinel = 0xffffffffu;  // minD before any centre: above every distance (3 4095^2 < 2^26)
constexpr int kKmppGroup = 64;                   // palettes a workgroup of kmpp_update_kernel serves
constexpr int kKmppBlocksPerCu = 8;              // its workgroups per CU: one resident round
constexpr uint32_t kKmppMinQspan = 2048;         // ... of at least 8 steps of 256 quads (2^13 pixels)
constexpr int64_t kKmppMaxPixels = (int64_t)1 << 30;  // 2^30 255 3 4095^2 < 2^63: T fits 64 bits

struct KmppArgs {
    const float* R;         // planar, the whole image (padded to a multiple of 4 floats)
    const float* G;
    const float* B;
    const uint32_t* rgbx;   // packed 8-bit R,G,B (AssignArgs::rgbx), else null
    const uint8_t* mask;    // a byte per pixel (padded to whole quads): the weight w, 0 / 1 under a mask; null: w = 1
    uint32_t* mind;         // [P][4 nq] D(x) of every palette: the squared distance to its nearest centre so far
    unsigned long long* part;   // [P][nspans] sum of w D over a span, per palette
    unsigned long long* wpart;  // [nspans] sum of w over a span
    int4* cent;             // [P][K] q of the centres (.w = 0); a fixed colour's are there before the first launch
    float4* out;            // [P][K] the drawn colours as the image holds them (.w = 0)
    long long* pix;         // [P][K] their raster indices
    uint32_t n;             // pixels (at most 2^30)
    uint32_t qspan;         // quads of 4 pixels per workgroup: a multiple of 256
    int nspans;             // ceil(nq / qspan), nq = ceil(n / 4)
    int P, K;
    uint64_t seed;
};

// minD <- min(minD, distance to centre k_new of each palette) (k_new < 0: no centre; init: minD starts
// from the sentinel), part <- the spans' sums of w minD, and with init wpart <- the spans' sums of w.
hipError_t launch_kmpp_update(const KmppArgs&, int k_new, bool init, hipStream_t);
// Round r of every palette: the draw into cent, out and pix at [p][r]; unit: D = 1 (no centre yet).
hipError_t launch_kmpp_pick(const KmppArgs&, int r, bool unit, hipStream_t);
// qspan and nspans of an image of n pixels: `span` pixels per workgroup asked for (test option
// "kmpp_span"; 0: by the grid, one resident round over the groups of P palettes)
void kmpp_spans(uint32_t n, int P, uint32_t span, int num_cu, uint32_t* qspan, int* nspans);

}  // namespace hq
