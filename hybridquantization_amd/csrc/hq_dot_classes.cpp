// hq_dot_classes.cpp -- the class matrices of hq_dot_population (hq.h): the preset, the legality
// rule, the baron count, the reach (how many rows above and below a pixel its sources lie: what a
// row-block shard renders beyond its own rows, hq_dot_population_partial) and the two per-cell
// tables the kernel reads (hq_dot.h, hq_dot.hip).
// Host code only; links alone into a CPU program (dot_check.cpp).
#include <algorithm>
#include <cstdint>
#include <cstring>

#include "hq_dot.h"

namespace {

// Knuth's 8 x 8 class matrix (hq.h), row by row.
constexpr int32_t kKnuth8[64] = {34, 48, 40, 32, 29, 15, 23, 31,  //
                                 42, 58, 56, 53, 21, 5,  7,  10,  //
                                 50, 62, 61, 45, 13, 1,  2,  18,  //
                                 38, 46, 54, 37, 25, 17, 9,  26,  //
                                 28, 14, 22, 30, 35, 49, 41, 33,  //
                                 20, 4,  6,  11, 43, 59, 57, 52,  //
                                 12, 0,  3,  19, 51, 63, 60, 44,  //
                                 24, 16, 8,  27, 39, 47, 55, 36};

// the class of the neighbour of cell (cx, cy) in direction d, on the torus
int32_t neighbour_class(const hq_dot_classes& m, int cx, int cy, int d) {
    const int n = m.n, x = (cx + hq::dot_dx(d) + n) % n, y = (cy + hq::dot_dy(d) + n) % n;
    return m.cls[y * n + x];
}

}  // namespace

namespace hq {

void dot_tables(const hq_dot_classes& m, uint32_t* lower, uint32_t* higher) {
    std::memset(lower, 0, sizeof(uint32_t) * kDotCells);
    std::memset(higher, 0, sizeof(uint32_t) * kDotCells);
    const int n = m.n;
    for (int cy = 0; cy < n; ++cy)
        for (int cx = 0; cx < n; ++cx) {
            const int32_t own = m.cls[cy * n + cx];
            int dirs[8], nl = 0;
            uint32_t hi = 0;
            for (int d = 0; d < 8; ++d) {
                if (neighbour_class(m, cx, cy, d) > own) hi |= 1u << d;
                else dirs[nl++] = d;  // (a permutation, n >= 4: never the cell's own class)
            }
            std::sort(dirs, dirs + nl,
                      [&](int a, int b) { return neighbour_class(m, cx, cy, a) < neighbour_class(m, cx, cy, b); });
            uint32_t lo = 0;
            for (int i = 0; i < 8; ++i) lo |= (i < nl ? (uint32_t)dirs[i] : kDotEnd) << (4 * i);
            lower[cy * n + cx] = lo;
            higher[cy * n + cx] = hi;
        }
}

}  // namespace hq

extern "C" {

int hq_dot_preset(int which, hq_dot_classes* out) {
    if (!out || which != HQ_DOT_KNUTH8) return HQ_ERR_ARG;
    std::memset(out, 0, sizeof *out);
    out->n = 8;
    std::memcpy(out->cls, kKnuth8, sizeof kKnuth8);
    return HQ_OK;
}

int hq_dot_classes_legal(const hq_dot_classes* m) {
    if (!m || (m->n != 4 && m->n != 8 && m->n != 16)) return 0;
    const int cells = m->n * m->n;
    bool seen[hq::kDotCells] = {};
    for (int i = 0; i < cells; ++i) {
        const int32_t c = m->cls[i];
        if (c < 0 || c >= cells || seen[c]) return 0;
        seen[c] = true;
    }
    return 1;
}

int hq_dot_barons(const hq_dot_classes* m) {
    if (!hq_dot_classes_legal(m)) return -1;
    uint32_t lower[hq::kDotCells], higher[hq::kDotCells];
    hq::dot_tables(*m, lower, higher);
    int barons = 0;
    for (int i = 0; i < m->n * m->n; ++i) barons += higher[i] == 0;
    return barons;
}

// A pixel's index depends on the pixels a path of neighbour steps with strictly descending class
// reaches from it.  The matrix is periodic, so the longest such path's extent up and down is a
// property of the cells: in ascending class each cell takes the larger of what it has and what
// each lower neighbour p, dy rows away, brings -- p's own extent shifted by dy.
int hq_dot_reach(const hq_dot_classes* m, int* above, int* below) {
    if (!above || !below || !hq_dot_classes_legal(m)) return HQ_ERR_ARG;
    const int n = m->n, cells = n * n;
    int cell_of[hq::kDotCells], up[hq::kDotCells] = {}, down[hq::kDotCells] = {};
    for (int c = 0; c < cells; ++c) cell_of[m->cls[c]] = c;
    int a = 0, b = 0;
    for (int k = 0; k < cells; ++k) {
        const int c = cell_of[k], cx = c % n, cy = c / n;
        for (int d = 0; d < 8; ++d) {
            const int dy = hq::dot_dy(d), p = (cy + dy + n) % n * n + (cx + hq::dot_dx(d) + n) % n;
            if (m->cls[p] >= k) continue;
            up[c] = std::max(up[c], up[p] - dy);
            down[c] = std::max(down[c], down[p] + dy);
        }
        a = std::max(a, up[c]);
        b = std::max(b, down[c]);
    }
    *above = a;
    *below = b;
    return HQ_OK;
}

}  // extern "C"
