// pattern_check.cpp -- pattern_tables' and pattern_n_valid's edge cases as a stand-alone host program,
// built and run under the address and undefined-behaviour sanitizers by `make pattern_check`
// (hq_pattern_tables.cpp and this file: no GPU code, no Python).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "hq_pattern.h"

namespace {

int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

// rank and color are inverse permutations of 0 .. K-1, ascending in (Y, k), zero from K on: the
// brute-force statement, Y by the same three products and two sums.
void check_order(const std::vector<float>& pal, int K) {
    uint8_t rank[hq::kPatternMaxK], color[hq::kPatternMaxK];
    std::memset(rank, 0xee, sizeof rank), std::memset(color, 0xee, sizeof color);
    CHECK(hq::pattern_tables(pal.data(), K, rank, color));
    auto y = [&](int k) { return ((0.299f * pal[4 * k]) + (0.587f * pal[4 * k + 1])) + (0.114f * pal[4 * k + 2]); };
    for (int k = 0; k < K; ++k) {
        int below = 0;
        for (int j = 0; j < K; ++j) below += y(j) < y(k) || (y(j) == y(k) && j < k);
        CHECK(rank[k] == below);
        CHECK(color[rank[k]] == k);
    }
    for (int k = K; k < hq::kPatternMaxK; ++k) CHECK(rank[k] == 0 && color[k] == 0);
}

}  // namespace

int main() {
    for (int n = -2; n <= 130; ++n)
        CHECK(hq::pattern_n_valid(n) == (n == 1 || n == 2 || n == 4 || n == 8 || n == 16 || n == 32 || n == 64));

    // hand values: blue < red < green in luminance; two equal colours and two of equal Y tie by k
    {
        const std::vector<float> pal = {0, 1, 0, 0, /**/ 1, 0, 0, 0, /**/ 0, 0, 1, 0, /**/ 1, 0, 0, 0, /**/ 0, 0, 0, 0};
        uint8_t rank[hq::kPatternMaxK], color[hq::kPatternMaxK];
        CHECK(hq::pattern_tables(pal.data(), 5, rank, color));
        const uint8_t want_rank[5] = {4, 2, 1, 3, 0}, want_color[5] = {4, 2, 1, 3, 0};
        CHECK(!std::memcmp(rank, want_rank, 5) && !std::memcmp(color, want_color, 5));
        check_order(pal, 5);
    }
    {  // a repeated colour on both sides of a darker one
        std::vector<float> pal = {0.5f, 0.f, 0.f, 0.f, /**/ 0.f, 0.f, 0.f, 0.f, /**/ 0.5f, 0.f, 0.f, 0.f};
        check_order(pal, 3);
    }
    // one colour, the largest palette, a pseudo-random one with repeats
    check_order({0.25f, 0.5f, 0.75f, 0.f}, 1);
    for (int K : {2, 5, 255, 256}) {
        std::vector<float> pal((size_t)4 * K, 0.f);
        uint32_t x = 12345u + (uint32_t)K;
        for (int k = 0; k < K; ++k)
            for (int c = 0; c < 3; ++c) {
                x = x * 1664525u + 1013904223u;
                pal[4 * k + c] = (float)((x >> 24) & 15u) / 15.0f;  // (16 levels: many equal Y)
            }
        check_order(pal, K);
    }

    // refusals: nothing is written
    {
        uint8_t rank[hq::kPatternMaxK], color[hq::kPatternMaxK];
        std::memset(rank, 0xee, sizeof rank), std::memset(color, 0xee, sizeof color);
        std::vector<float> pal((size_t)4 * 257, 0.5f);
        CHECK(!hq::pattern_tables(nullptr, 4, rank, color));
        CHECK(!hq::pattern_tables(pal.data(), 4, nullptr, color));
        CHECK(!hq::pattern_tables(pal.data(), 4, rank, nullptr));
        CHECK(!hq::pattern_tables(pal.data(), 0, rank, color));
        CHECK(!hq::pattern_tables(pal.data(), 257, rank, color));
        pal[4] = NAN;
        CHECK(!hq::pattern_tables(pal.data(), 4, rank, color));
        pal[4] = INFINITY;
        CHECK(!hq::pattern_tables(pal.data(), 4, rank, color));
        for (int k = 0; k < hq::kPatternMaxK; ++k) CHECK(rank[k] == 0xee && color[k] == 0xee);
    }
    if (failures) {
        std::fprintf(stderr, "pattern_check: %d failure(s)\n", failures);
        return 1;
    }
    std::puts("pattern_check ok");
    return 0;
}
