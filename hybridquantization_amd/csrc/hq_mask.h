// hq_mask.h -- the host side of the pixel mask (hq_set_mask): counting, and the
// list of output tiles the fast cost kernels launch.  Plain C++ (hq_mask.cpp,
// host compiler only), shared by the runtime and mask_check.cpp.  Not part of
// the public ABI (include/hq.h).
#pragma once

#include <stdint.h>

namespace hq {

// Non-zero bytes among mask[0 .. n).
int64_t mask_count(const uint8_t* mask, int64_t n);

// The sum of weights[0 .. n) as integers (hq_set_weights: a byte is its pixel's weight, 0 .. 255;
// of a 0 / 1 mask this is mask_count).  n < 2^55, so the sum fits int64.
int64_t weight_sum(const uint8_t* weights, int64_t n);

// The largest weight sum of the owned rows under which the planar form's integer sums (units of
// 2^-32: a pixel adds up to 255 2^32) stay below 2^63: the sum has to stay BELOW this.
constexpr int64_t kWeightSumLimit = (int64_t)1 << 31;

// The tile grid of a fast cost launch over a shard: tiles of tile_w x tile_h
// pixels, tiles_x per tile row, tile (tx, ty) = number ty tiles_x + tx covering
// columns [tx tile_w, +tile_w) and rows [grid_row0 + ty tile_h, +tile_h), both
// clipped to the image's width W and the owned rows [r0, r1).  grid_row0 <= r0
// (fast_grid_row0: r0 itself, or for dE2000 the image's tile row that holds r0).
struct TileGrid {
    int W, r0, r1;
    int grid_row0;
    int tile_w, tile_h;
    int tiles_x, ntiles;
};

// The live tiles of `grid` under the owned rows' mask (own[(y - r0) W + x], a
// byte per pixel, non-zero = in: a 0 / 1 mask or the raw bytes of a weight map), in ascending tile number into out[0 ..
// ntiles): a tile is live when it holds an in-mask owned pixel.  skip = false:
// every tile (the identity list).  Returns how many.
int mask_live_tiles(const uint8_t* own, const TileGrid& grid, bool skip, int32_t* out);

}  // namespace hq
