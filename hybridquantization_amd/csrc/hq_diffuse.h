// hq_diffuse.h -- the launcher of hq_diffuse.hip (the error-diffusion kernels of
// hq_dither_population and hq_diffuse_population) and its arguments, for that unit and the
// runtime; and the argmin those kernels share with dot diffusion's (hq_dot.hip).  A header of
// its own: no other kernel unit reads it.
#pragma once

#include "hq_launch.h"

namespace hq {

constexpr int kDiffuseMaxRows2 = 1024;  // rows per strip at most, instances of slope 2
constexpr int kDiffuseMaxRows3 = 512;   // ... of slope 3: their ring is twice as deep

// diffuse_kernel<R, S, FS>: the error-diffused index images of P palettes of K <= 256 colours
// over the whole image under a diffusion kernel (hq.h: hq_diffusion_taps), in the place of
// grid + assign.
struct DiffuseArgs {
    const float* R;         // planar, the whole image (row y at y W)
    const float* G;
    const float* B;
    const float4* pal;      // [P][256] the prepared palettes (.w = 0)
    uint8_t* idx;           // [P][idx_pitch]
    uint32_t* used_glob;    // [kUsedSlots][used_stride]: slot 0 is written, the others zeroed before the launch
    float* carry;           // [P][rows_up][3][W] the errors of a strip's last rows_up rows
    int64_t idx_pitch;
    int W, H, K;
    int rows;               // rows per strip: a multiple of 64 in 64 .. 1024 (clamped to the instance's most)
    int rows_up, slope;     // the instance (hq_diffusion_classify): R in {1, 2}, S in {2, 3}
    bool fs;                // Floyd-Steinberg's own formula (hq.h: hq_dither_population) in the place of the
                            // general one: R = 1, S = 2, and w0, w1, w2 and div are not read
    float strength;         // s in [0, 1]
    float w0[2];            // float(w[0][dx + 2]), dx = 1, 2
    float w1[5], w2[5];     // float(w[1][dx + 2]), float(w[2][dx + 2]), dx = -2 .. 2
    float div;              // float(div)
};

// floats of DiffuseArgs::carry for P palettes of an image W wide
inline size_t diffuse_carry_floats(int P, int rows_up, int W) { return (size_t)P * rows_up * 3 * W; }

hipError_t launch_diffuse(const DiffuseArgs&, int P, hipStream_t, AssignTag* tag = nullptr);

#ifdef HQ_DIFFUSE_DEVICE
// (the kernel units that render by diffusion, hq_diffuse.hip and hq_dot.hip, after hq_device.h)
// The reference's first minimum over all K colours (CL:179-192).  Ranked by the
// fma-chain d^2 as the plain assign kernels rank (dist2_rank: ref_len's own d^2
// for w = 0); a runner-up within near_d2 of the best -- v_sqrt_f32 can give two
// d^2 one distance, and then the lower index wins -- is re-resolved by the
// reference loop itself.  v and the colours are finite: no NaN arises.
__device__ __forceinline__ int diffuse_argmin(float r, float g, float b, const float4* s_pal, int K) {
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
#endif

}  // namespace hq
