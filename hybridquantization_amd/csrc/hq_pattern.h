// hq_pattern.h -- pattern dithering (hq.h: hq_pattern_population): the kernel's arguments and
// launcher (hq_pattern.hip), and the per-palette luminance order it reads (hq_pattern_tables.cpp,
// host code only).
#pragma once

#include <cstdint>

namespace hq {

constexpr int kPatternMaxK = 256;  // (kMaxK; stated here so that the host half stands alone)
constexpr int kPatternMaxN = 64;

// The luminance order of one palette (hq.h): Y_k = ((0.299f R_k) + (0.587f G_k)) + (0.114f B_k) in
// fp32 operations, none contracted; the colours ordered by (Y_k, k) ascending.  pal4: K colours of
// four floats.  rank[k]: colour k's position in that order; color[r]: the colour at position r (the
// inverse).  Both hold kPatternMaxK bytes; the entries from K on are 0.  False (nothing written) for
// a null pointer, K outside 1 .. kPatternMaxK or a Y that is not finite.
bool pattern_tables(const float* pal4, int K, uint8_t* rank, uint8_t* color);
// hq_pattern_population's `n`: 1, 2, 4, 8, 16, 32 or 64.
bool pattern_n_valid(int n);

#ifdef __HIPCC__
struct PatternArgs {
    const float *R, *G, *B;     // planar image, extended rows
    const uint32_t* rgbx;       // the packed 8-bit copy, or null: the kernel then reads the planes
    const float4* pal;          // [P][kMaxK] prepared palettes (.w = 0)
    const uint8_t* tab;         // [P][2][kMaxK]: pattern_tables' rank, then color
    const float* map;           // [mh][mw] the context's threshold map, mw and mh powers of two
    uint32_t mw_mask, mh_mask, lg_mw;
    uint8_t* idx;               // [P][idx_pitch]
    uint32_t* used_glob;        // [kUsedSlots][used_stride]: [P][8] used-colour bits per slot, zeroed before the launch
    int used_stride;
    int64_t n_ext, idx_pitch;
    uint32_t W;                 // the image's width
    uint32_t y0;                // the full-image row of extended row 0 (Geom::e0)
    int K;
    int n;                      // the list length: pattern_n_valid
    float strength;             // in [0, 1]
};

// One launch over (pixel blocks, P).  hipErrorInvalidValue, and nothing launched, for arguments the
// kernel's bounds do not cover.
hipError_t launch_pattern(const PatternArgs&, int P, hipStream_t, struct AssignTag* tag = nullptr);
#endif

}  // namespace hq
