// hq_dot.h -- dot diffusion (hq.h: hq_dot_population): the per-cell tables of a class matrix
// (hq_dot_classes.cpp, host code only), the tiled form's schedule and plan and, for hipcc, the
// launchers of hq_dot.hip and hq_dot_tile.hip and their arguments.  A header of its own: no
// other kernel unit reads it (the host runtime does, through hq_runtime.h).
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

// ---- the tiled form (hq_dot_tile.hip; hq.h: option "dot_tile") ----
// The schedule a workgroup follows: the cells ordered by level (hq_dot_levels; ties by cell),
// level l's cells at cell[start[l]] .. cell[start[l + 1]), l < depth.  Every entry of start past
// depth holds n^2, every entry of cell past n^2 holds 0.  Each cell's lower neighbours in
// ascending class stay where dot_tables puts them.  An illegal matrix: depth 0.
struct DotSchedule {
    int depth;
    uint32_t cell[kDotCells];
    uint32_t start[kDotCells + 1];
};
static_assert(sizeof(DotSchedule) == sizeof(int) + sizeof(uint32_t) * (2 * kDotCells + 1), "cell, then start");
void dot_schedule(const hq_dot_classes& cls, DotSchedule* out);
// (as the device holds it: cell, then start)
constexpr int kDotSchedWords = 2 * kDotCells + 1;

// The tile shapes, smallest first (option "dot_tile_shape" 1 .. kDotTileShapes; 0: the largest
// whose window fits).  Every side is a multiple of kDotSide, so every tile sees one cell layout.
constexpr int kDotTileShapes = 3;
constexpr int kDotTileW[kDotTileShapes] = {16, 32, 64};
constexpr int kDotTileH[kDotTileShapes] = {16, 32, 32};
// The LDS a workgroup's window may take for its errors, 12 bytes per pixel: 64 KiB less the
// palette, the tables and the schedule.
constexpr int kDotTileErrBytes = 56 * 1024;
constexpr int kDotTileMaxLanes = 4;   // lanes that share one pixel's argmin, at most (what the tests reach)

// What dot_tile_eligible chose: the shape (0-based), the reach, the levels, the lanes per pixel
// (a power of two, log2) and the window's pixels at most.
struct DotTilePlan {
    int shape, tw, th;
    int above, below, left, right;
    int depth, lg_lanes;
    int window;  // (tw + left + right) (th + above + below)
};
// What the rule needs of a matrix: its reach in four directions and its levels (hq_dot_reach2,
// hq_dot_levels).  The context keeps it beside the matrix whose tables it holds, so a pass --
// every iteration of a search -- computes nothing of it again.  False: an illegal matrix.
struct DotMatrixInfo {
    int above, below, left, right, depth;
};
bool dot_matrix_info(const hq_dot_classes& cls, DotMatrixInfo* out);
// The rule (hq.h): K <= 256 and a legal matrix whose window under the shape asked for -- shape
// 1 .. kDotTileShapes, or 0: the largest one that fits, tried from the largest -- holds its errors
// in kDotTileErrBytes.  False: not eligible, *plan untouched.  (A whole image is the caller's to
// look at: the rule about the matrix is a host-only function.)
bool dot_tile_eligible(const DotMatrixInfo& info, int K, int shape, DotTilePlan* plan);
bool dot_tile_eligible(const hq_dot_classes& cls, int K, int shape, DotTilePlan* plan);  // (dot_matrix_info first)
// Option "dot_tile" -1: where an eligible pass of P palettes of K colours over W x H pixels takes
// the tiled kernel under the plan's tile shape (0-based): inside the region where it was measured
// faster than the chain -- a 32 x 32 or 64 x 32 tile, W H <= 2^20 and W H P K <= 2^28 (hq.h).
bool dot_tile_auto(int W, int H, int P, int K, int shape);

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

// dot_tile_kernel (hq_dot_tile.hip): the same index images in one launch, grid (tiles, P): a
// workgroup renders its tile's window -- the tile extended by the reach on each side, clipped to
// the image -- level by level with the errors in LDS, and writes the tile's own indices.
struct DotTileArgs {
    const float* R;         // planar, the whole image (row y at y W)
    const float* G;
    const float* B;
    const float4* pal;      // [P][256] the prepared palettes (.w = 0)
    uint8_t* idx;           // [P][idx_pitch]
    uint32_t* used_glob;    // [kUsedSlots][used_stride], zeroed before the launch
    const uint32_t* tab;    // [2][kDotCells]: dot_tables' lower, then higher
    const uint32_t* sched;  // [kDotSchedWords]: DotSchedule's cell, then start
    int64_t idx_pitch;
    int used_stride;
    int W, H, K;
    int n;                  // the matrix's side: 4, 8 or 16
    float strength;         // s in [0, 1]
    DotTilePlan plan;
};

hipError_t launch_dot_tile(const DotTileArgs&, int P, hipStream_t, AssignTag* tag = nullptr);

}  // namespace hq
#endif
