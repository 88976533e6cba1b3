// hq_mask.cpp -- the pixel mask's and the pixel weights' host code: the count of in-mask
// pixels, the sum of weights and the live-tile list of the fast cost kernels (hq_mask.h).  No GPU code: `make
// mask_check` builds this file alone under the sanitizers.
#include "hq_mask.h"

#include <algorithm>

namespace hq {

int64_t mask_count(const uint8_t* mask, int64_t n) {
    int64_t c = 0;
    for (int64_t i = 0; i < n; ++i) c += mask[i] != 0;
    return c;
}

int64_t weight_sum(const uint8_t* weights, int64_t n) {
    int64_t s = 0;
    for (int64_t i = 0; i < n; ++i) s += weights[i];
    return s;
}

int mask_live_tiles(const uint8_t* own, const TileGrid& g, bool skip, int32_t* out) {
    int n = 0;
    if (!skip) {
        for (int t = 0; t < g.ntiles; ++t) out[n++] = t;
        return n;
    }
    const int tiles_y = g.tiles_x > 0 ? g.ntiles / g.tiles_x : 0;
    for (int ty = 0; ty < tiles_y; ++ty) {
        // the tile row's owned rows (a dE2000 shard's first tile row starts above r0)
        const int y0 = std::max(g.grid_row0 + ty * g.tile_h, g.r0);
        const int y1 = std::min(g.grid_row0 + (ty + 1) * g.tile_h, g.r1);
        for (int tx = 0; tx < g.tiles_x; ++tx) {
            const int x0 = tx * g.tile_w, x1 = std::min(x0 + g.tile_w, g.W);
            bool live = false;
            for (int y = y0; y < y1 && !live; ++y) {
                const uint8_t* row = own + (int64_t)(y - g.r0) * g.W;
                live = std::any_of(row + x0, row + x1, [](uint8_t b) { return b != 0; });
            }
            if (live) out[n++] = ty * g.tiles_x + tx;
        }
    }
    return n;
}

}  // namespace hq
