// hq_diffuse.h -- the launcher of hq_diffuse.hip (the error-diffusion kernels of
// hq_dither_population and hq_diffuse_population) and its arguments, for that unit and the
// runtime.  A header of its own: no other kernel unit reads it.
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

}  // namespace hq
