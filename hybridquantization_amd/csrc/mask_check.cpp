// mask_check.cpp -- the live-tile list and the mask counts (hq_mask.cpp) against a
// brute-force statement on their edge cases, as a stand-alone host program built
// and run under the address and undefined-behaviour sanitizers by `make
// mask_check` (hq_mask.cpp and this file: no GPU code, no Python).
#include <cstdint>
#include <cstdio>
#include <set>
#include <vector>

#include "hq_mask.h"

namespace {

int failures = 0, cases = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

// fast_tile_dims and fast_grid_row0 restated (hq_cost.hip): th a power of two
hq::TileGrid grid(int W, int r0, int r1, int tw, int th, bool de2000) {
    hq::TileGrid g{};
    g.W = W, g.r0 = r0, g.r1 = r1;
    g.grid_row0 = de2000 ? r0 & ~(th - 1) : r0;
    g.tile_w = tw, g.tile_h = th;
    g.tiles_x = (W + tw - 1) / tw;
    g.ntiles = g.tiles_x * ((r1 - g.grid_row0 + th - 1) / th);
    return g;
}

// full: the FULL image's mask [H][W]; the shard owns rows [r0, r1)
void check(const std::vector<uint8_t>& full, int W, int H, int r0, int r1, int tw, int th, bool de2000,
           int expect_live = -1) {
    ++cases;
    const hq::TileGrid g = grid(W, r0, r1, tw, th, de2000);
    const uint8_t* own = full.data() + (size_t)r0 * W;
    // an exactly sized output: the sanitizer sees any write past ntiles
    std::vector<int32_t> out((size_t)g.ntiles), all((size_t)g.ntiles);
    const int n = hq::mask_live_tiles(own, g, true, out.data());
    std::set<int> want;
    int64_t n_own = 0, n_full = 0;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            if (!full[(size_t)y * W + x]) continue;
            ++n_full;
            if (y < r0 || y >= r1) continue;
            ++n_own;
            want.insert((y - g.grid_row0) / th * g.tiles_x + x / tw);
        }
    CHECK(n == (int)want.size());
    CHECK(std::set<int>(out.begin(), out.begin() + n) == want);
    for (int i = 1; i < n; ++i) CHECK(out[i - 1] < out[i]);
    for (int i = 0; i < n; ++i) CHECK(out[i] >= 0 && out[i] < g.ntiles);
    if (expect_live >= 0) CHECK(n == expect_live);
    CHECK(hq::mask_count(full.data(), (int64_t)W * H) == n_full);
    CHECK(hq::mask_count(own, (int64_t)W * (r1 - r0)) == n_own);
    const int na = hq::mask_live_tiles(own, g, false, all.data());
    CHECK(na == g.ntiles);
    for (int i = 0; i < na; ++i) CHECK(all[i] == i);
}

struct Shape {
    int tw, th;
};
const Shape kShapes[] = {{128, 16}, {108, 8}, {256, 16}};

}  // namespace

int main() {
    for (const Shape& s : kShapes) {
        for (int de = 0; de < 2; ++de) {
            const int W = 300, H = 40;
            {  // one pixel in each corner, values 1, 7, 255 and 128
                std::vector<uint8_t> m((size_t)W * H, 0);
                m[0] = 1, m[W - 1] = 7, m[(size_t)(H - 1) * W] = 255, m[(size_t)H * W - 1] = 128;
                check(m, W, H, 0, H, s.tw, s.th, de, (W + s.tw - 1) / s.tw > 1 ? 4 : 2);
            }
            {  // only the last partial tile column
                std::vector<uint8_t> m((size_t)W * H, 0);
                const int x0 = (W - 1) / s.tw * s.tw;
                for (int y = 0; y < H; ++y)
                    for (int x = x0; x < W; ++x) m[(size_t)y * W + x] = 1;
                check(m, W, H, 0, H, s.tw, s.th, de, (H + s.th - 1) / s.th);
            }
            {  // only the last partial tile row
                std::vector<uint8_t> m((size_t)W * H, 0);
                const int y0 = (H - 1) / s.th * s.th;
                for (int y = y0; y < H; ++y)
                    for (int x = 0; x < W; ++x) m[(size_t)y * W + x] = 1;
                check(m, W, H, 0, H, s.tw, s.th, de, (W + s.tw - 1) / s.tw);
            }
            {  // a shard whose first tile row starts above r0 (dE2000's grid), and the same rows from r0
                std::vector<uint8_t> m((size_t)W * H, 0);
                for (int y = 0; y < H; ++y)
                    for (int x = 0; x < W; ++x) m[(size_t)y * W + x] = (uint8_t)((x * 7 + y * 13) % 5 == 0);
                check(m, W, H, 21, 37, s.tw, s.th, de);
                check(m, W, H, 21, 22, s.tw, s.th, de);
                std::vector<uint8_t> one((size_t)W * H, 0);  // the pixel at (r0, 0) alone: tile 0 in either grid
                one[(size_t)21 * W] = 1;
                check(one, W, H, 21, 37, s.tw, s.th, de, 1);
            }
            {  // an empty shard: the mask lives in other rows
                std::vector<uint8_t> m((size_t)W * H, 0);
                for (int x = 0; x < W; ++x) m[(size_t)30 * W + x] = 1;
                check(m, W, H, 0, 20, s.tw, s.th, de, 0);
            }
            {  // W or H smaller than a tile
                for (const int wh : {5, 1, 3}) {
                    std::vector<uint8_t> a((size_t)wh, 1), b((size_t)wh, 0);
                    b[wh - 1] = 1;
                    check(a, wh, 1, 0, 1, s.tw, s.th, de, 1);
                    check(b, 1, wh, 0, wh, s.tw, s.th, de, 1);
                    check(b, 1, wh, wh - 1, wh, s.tw, s.th, de, 1);
                }
                std::vector<uint8_t> m(6, 0);
                m[4] = 1;
                check(m, 2, 3, 0, 3, s.tw, s.th, de, 1);
                check(m, 2, 3, 0, 2, s.tw, s.th, de, 0);
            }
        }
    }
    std::printf("mask_check: %d cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
