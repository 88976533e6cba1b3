// hq_dot.h -- dot diffusion (hq.h: hq_dot_population): the per-cell tables of a class matrix
// (hq_dot_classes.cpp, host code only) and, for hipcc, the launcher of hq_dot.hip and its
// arguments.  A header of its own: no other kernel unit reads it.
#pragma once

#include <stdint.h>

#include "../../include/hq.h"

namespace hq {

// The 8 neighbour directions d = 0 .. 7, row by row around the pixel:
//   0 (-1, -1)  1 (0, -1)  2 (1, -1)  3 (-1, 0)  4 (1, 0)  5 (-1, 1)  6 (0, 1)  7 (1, 1)
// 7 - d is the opposite direction; the orthogonal ones (1, 3, 4, 6) weigh 2, the diagonal ones 1.
constexpr int kDotSide = 16;                   // the largest class matrix
constexpr int kDotCells = kDotSide * kDotSide; // ... and its cells
constexpr uint32_t kDotOrth = 0x5Au, kDotDiag = 0xA5u;  // the directions' bits by weight
constexpr uint32_t kDotEnd = 0xFu;             // a nibble of `lower` past the last neighbour
constexpr int kDotMaxP = 65535;                // palettes per call: a launch's grid is (pixel chunks, P)
inline constexpr int dot_dx(int d) { return (d + (d >= 4)) % 3 - 1; }
inline constexpr int dot_dy(int d) { return (d + (d >= 4)) / 3 - 1; }
inline constexpr int dot_weight(int d) { return (kDotOrth >> d & 1u) ? 2 : 1; }

// The two tables the kernel reads, per cell c = cy n + cx of a legal matrix (neighbours taken on
// the torus, as the tiling makes them):
//   lower[c]   nibble i: the direction of the i-th neighbour of lower class, in ascending class;
//              kDotEnd in every nibble past the last one
//   higher[c]  bit d: the neighbour in direction d has a higher class
// Both arrays hold kDotCells words; the cells past n^2 are zeroed.
void dot_tables(const hq_dot_classes& cls, uint32_t* lower, uint32_t* higher);

}  // namespace hq

#ifdef __HIPCC__
#include "hq_launch.h"

namespace hq {

// dot_kernel: the dot-diffused index images of P palettes of K <= 256 colours over the whole
// image, one launch per class in ascending class on the stream, in the place of grid + assign.
struct DotArgs {
    const float* R;         // planar, the whole image (row y at y W)
    const float* G;
    const float* B;
    const float4* pal;      // [P][256] the prepared palettes (.w = 0)
    uint8_t* idx;           // [P][idx_pitch]
    uint32_t* used_glob;    // [kUsedSlots][used_stride], zeroed before the first launch
    float* err;             // [P][3][H][W] the errors e; never zeroed (a pixel reads what this call wrote)
    const uint32_t* tab;    // [2][kDotCells]: dot_tables' lower, then higher
    const int32_t* cls;     // the matrix (host memory: the launcher orders the cells by it)
    int64_t idx_pitch;
    int used_stride;
    int W, H, K;
    int n;                  // the matrix's side: 4, 8 or 16
    float strength;         // s in [0, 1]
    int cx, cy, nx, ny;     // (set per launch) the class's cell and its pixels: columns, rows
};

// floats of DotArgs::err for P palettes (H: the rows rendered -- the image's, or a window's)
inline size_t dot_err_floats(int P, int W, int H) { return (size_t)P * 3 * W * H; }

hipError_t launch_dot(const DotArgs&, int P, hipStream_t, AssignTag* tag = nullptr);

// dot_kernel's windowed instance (hq_dot_population_partial on a row-block shard): the launches
// run over the full-image rows [a0, a1) only.  A pixel's class comes from its full-image row and
// W(p)'s border rule from the full image's H (DotArgs::H), so the window's outer edge is not an
// image border; a source outside the window contributes nothing and is never read.  Indices and
// used bits are written for rows [e0, e1) alone -- the shard's extended rows, whose pixels
// R, G, B and whose index images hold (row e0 first); the rows [a0, e0) and [e1, a1) are
// rendered for their errors, their pixels among the apron planes' rows.  err is [P][3][a1 - a0][W].
struct DotWinArgs : DotArgs {
    const float* aR;        // the apron held: rows [h0, e0), then rows [e1, h1), W floats each
    const float* aG;        // (null when it holds none)
    const float* aB;
    int h0, h1;             // h0 <= a0, a1 <= h1: the window may take less than is held
    int a0, a1;             // 0 <= a0 <= e0 < e1 <= a1 <= H
    int e0, e1;
    int y0;                 // (set per launch) the class's first row in the window
};

hipError_t launch_dot_window(const DotWinArgs&, int P, hipStream_t, AssignTag* tag = nullptr);

}  // namespace hq
#endif
