// hq_pattern_tables.cpp -- pattern dithering's per-palette luminance order (hq_pattern.h), host
// code only: built without contraction (the Makefile's -ffp-contract=off), so Y is three products
// and two sums, each rounded once.
#include <algorithm>

#include "hq_pattern.h"

namespace hq {

bool pattern_n_valid(int n) { return n >= 1 && n <= kPatternMaxN && (n & (n - 1)) == 0; }

bool pattern_tables(const float* pal4, int K, uint8_t* rank, uint8_t* color) {
    if (!pal4 || !rank || !color || K < 1 || K > kPatternMaxK) return false;
    float y[kPatternMaxK];
    int order[kPatternMaxK];
    for (int k = 0; k < K; ++k) {
        const float* c = pal4 + 4 * k;
        y[k] = ((0.299f * c[0]) + (0.587f * c[1])) + (0.114f * c[2]);
        if (!(y[k] - y[k] == 0.0f)) return false;  // (not finite: no order)
        order[k] = k;
    }
    // (Y, k) ascending: a strict order on distinct k, so the result does not depend on the sort
    std::sort(order, order + K, [&](int a, int b) { return y[a] < y[b] || (y[a] == y[b] && a < b); });
    std::fill(rank, rank + kPatternMaxK, (uint8_t)0);
    std::fill(color, color + kPatternMaxK, (uint8_t)0);
    for (int r = 0; r < K; ++r) {
        color[r] = (uint8_t)order[r];
        rank[order[r]] = (uint8_t)r;
    }
    return true;
}

}  // namespace hq
