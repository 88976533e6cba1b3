// weights_check.cpp -- the pixel weights' sums and the live-tile list of weight maps
// (hq_mask.cpp) against a brute-force statement on their edge cases, as a stand-alone
// host program built and run under the address and undefined-behaviour sanitizers by
// `make weights_check` (hq_mask.cpp and this file: no GPU code, no Python).
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

// full: the FULL image's weights [H][W]; the shard owns rows [r0, r1).  The weight sums and the
// non-zero counts of the full image and of the owned rows, and the live tiles of the raw bytes,
// pixel by pixel.
void check(const std::vector<uint8_t>& full, int W, int H, int r0, int r1, int tw, int th, bool de2000,
           int expect_live = -1, int64_t expect_w_full = -1) {
    ++cases;
    const hq::TileGrid g = grid(W, r0, r1, tw, th, de2000);
    const uint8_t* own = full.data() + (size_t)r0 * W;
    // an exactly sized output: the sanitizer sees any write past ntiles
    std::vector<int32_t> out((size_t)g.ntiles);
    const int n = hq::mask_live_tiles(own, g, true, out.data());
    std::set<int> want;
    int64_t w_own = 0, w_full = 0, n_own = 0, n_full = 0;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const int64_t v = full[(size_t)y * W + x];
            w_full += v;
            n_full += v != 0;
            if (y < r0 || y >= r1) continue;
            w_own += v;
            n_own += v != 0;
            if (v) want.insert((y - g.grid_row0) / th * g.tiles_x + x / tw);
        }
    CHECK(n == (int)want.size());
    CHECK(std::set<int>(out.begin(), out.begin() + n) == want);
    for (int i = 1; i < n; ++i) CHECK(out[i - 1] < out[i]);
    for (int i = 0; i < n; ++i) CHECK(out[i] >= 0 && out[i] < g.ntiles);
    if (expect_live >= 0) CHECK(n == expect_live);
    CHECK(hq::weight_sum(full.data(), (int64_t)W * H) == w_full);
    CHECK(hq::weight_sum(own, (int64_t)W * (r1 - r0)) == w_own);
    CHECK(hq::mask_count(full.data(), (int64_t)W * H) == n_full);
    CHECK(hq::mask_count(own, (int64_t)W * (r1 - r0)) == n_own);
    CHECK(w_own >= n_own && w_own <= 255 * n_own);
    if (expect_w_full >= 0) CHECK(w_full == expect_w_full);
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
            {  // one non-zero pixel in each corner, weights 1, 7, 255 and 128
                std::vector<uint8_t> m((size_t)W * H, 0);
                m[0] = 1, m[W - 1] = 7, m[(size_t)(H - 1) * W] = 255, m[(size_t)H * W - 1] = 128;
                check(m, W, H, 0, H, s.tw, s.th, de, (W + s.tw - 1) / s.tw > 1 ? 4 : 2, 1 + 7 + 255 + 128);
            }
            {  // gradients: every byte value, non-uniform within every quad
                std::vector<uint8_t> hz((size_t)W * H), vt((size_t)W * H);
                for (int y = 0; y < H; ++y)
                    for (int x = 0; x < W; ++x) {
                        hz[(size_t)y * W + x] = (uint8_t)(x * 255 / (W - 1));
                        vt[(size_t)y * W + x] = (uint8_t)(y * 255 / (H - 1));
                    }
                check(hz, W, H, 0, H, s.tw, s.th, de);
                check(vt, W, H, 0, H, s.tw, s.th, de);
                check(hz, W, H, 21, 37, s.tw, s.th, de);  // a shard whose dE2000 grid starts above r0
                check(vt, W, H, 21, 22, s.tw, s.th, de);
                check(vt, W, H, 0, 1, s.tw, s.th, de, 0);  // the vertical gradient's row 0 weighs nothing
            }
            {  // noise bytes with a zero rectangle that empties whole tiles at 128 x 16
                std::vector<uint8_t> m((size_t)W * H);
                uint32_t lcg = 12345u;
                for (auto& b : m) b = (uint8_t)((lcg = lcg * 1664525u + 1013904223u) >> 24);
                for (int y = 0; y < 32; ++y)
                    for (int x = 0; x < 256; ++x) m[(size_t)y * W + x] = 0;
                check(m, W, H, 0, H, s.tw, s.th, de);
                check(m, W, H, 0, 20, s.tw, s.th, de);
                check(m, W, H, 20, H, s.tw, s.th, de);
            }
            {  // an empty shard: the weights live in other rows
                std::vector<uint8_t> m((size_t)W * H, 0);
                for (int x = 0; x < W; ++x) m[(size_t)30 * W + x] = 200;
                check(m, W, H, 0, 20, s.tw, s.th, de, 0, 200 * W);
            }
            {  // W or H smaller than a tile
                for (const int wh : {5, 1, 3}) {
                    std::vector<uint8_t> a((size_t)wh, 255), b((size_t)wh, 0);
                    b[wh - 1] = 9;
                    check(a, wh, 1, 0, 1, s.tw, s.th, de, 1, 255 * wh);
                    check(b, 1, wh, 0, wh, s.tw, s.th, de, 1, 9);
                    check(b, 1, wh, wh - 1, wh, s.tw, s.th, de, 1, 9);
                }
                std::vector<uint8_t> m(6, 0);
                m[4] = 3;
                check(m, 2, 3, 0, 3, s.tw, s.th, de, 1, 3);
                check(m, 2, 3, 0, 2, s.tw, s.th, de, 0, 3);
            }
        }
    }
    {  // the 2^31 boundary: 2904 x 2900 pixels of weight 254 stay below it, of weight 255 do not
        ++cases;
        const int64_t n = (int64_t)2904 * 2900;
        std::vector<uint8_t> m((size_t)n, 254);
        CHECK(hq::weight_sum(m.data(), n) == 2139086400ll && 2139086400ll < hq::kWeightSumLimit);
        m.assign((size_t)n, 255);
        CHECK(hq::weight_sum(m.data(), n) == 2147508000ll && 2147508000ll >= hq::kWeightSumLimit);
        // exactly the limit and one below it: 2^23 pixels of 255 and one of 255 / 254 short of ... 2^31
        const int64_t k = hq::kWeightSumLimit / 255;  // 8421504 pixels of 255: 2^31 - 128
        m.assign((size_t)k + 1, 255);
        m[(size_t)k] = 128;
        CHECK(hq::weight_sum(m.data(), k + 1) == hq::kWeightSumLimit);
        m[(size_t)k] = 127;
        CHECK(hq::weight_sum(m.data(), k + 1) == hq::kWeightSumLimit - 1);
        CHECK(hq::mask_count(m.data(), k + 1) == k + 1);
    }
    std::printf("weights_check: %d cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
