// hq_dot_classes.cpp -- the class matrices of hq_dot_population (hq.h): the preset, the legality
// rule, the baron count, the reach (how many rows above and below a pixel its sources lie: what a
// row-block shard renders beyond its own rows, hq_dot_population_partial; in four directions: what
// a tile of the tiled form renders around itself), the levels (the sequential depth of the matrix)
// and the per-cell tables and the schedule the kernels read (hq_dot.h, hq_dot.hip, hq_dot_tile.hip).
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

// The cells by level, ties by cell: a counting sort over hq_dot_levels' answer.
void dot_schedule(const hq_dot_classes& m, DotSchedule* out) {
    std::memset(out, 0, sizeof *out);
    int32_t level[kDotCells];
    if (hq_dot_levels(&m, level, &out->depth)) {
        out->depth = 0;
        return;
    }
    const int cells = m.n * m.n;
    for (int c = 0; c < cells; ++c) ++out->start[level[c] + 1];
    for (int l = 0; l < out->depth; ++l) out->start[l + 1] += out->start[l];
    uint32_t next[kDotCells + 1];
    std::memcpy(next, out->start, sizeof next);
    for (int c = 0; c < cells; ++c) out->cell[next[level[c]]++] = (uint32_t)c;
    for (int l = out->depth + 1; l <= kDotCells; ++l) out->start[l] = (uint32_t)cells;
}

bool dot_matrix_info(const hq_dot_classes& m, DotMatrixInfo* out) {
    DotMatrixInfo i{};
    int32_t level[kDotCells];
    if (hq_dot_reach2(&m, &i.above, &i.below, &i.left, &i.right) || hq_dot_levels(&m, level, &i.depth)) return false;
    *out = i;
    return true;
}

// The lanes per pixel: the threads of a workgroup (256) over the pixels a level has on average,
// rounded down to a power of two, at most kDotTileMaxLanes, and no more lanes than leave each at
// least 4 colours.
bool dot_tile_eligible(const DotMatrixInfo& info, int K, int shape, DotTilePlan* plan) {
    DotTilePlan p{};
    if (K < 1 || K > 256 || shape < 0 || shape > kDotTileShapes || info.depth < 1) return false;
    p.above = info.above, p.below = info.below, p.left = info.left, p.right = info.right, p.depth = info.depth;
    const int first = shape ? shape - 1 : kDotTileShapes - 1, last = shape ? shape - 1 : 0;
    for (int s = first; s >= last; --s) {
        const int64_t window = (int64_t)(kDotTileW[s] + p.left + p.right) * (kDotTileH[s] + p.above + p.below);
        if (window * 12 > kDotTileErrBytes) continue;
        p.shape = s, p.tw = kDotTileW[s], p.th = kDotTileH[s], p.window = (int)window;
        const int per_level = std::max(1, p.window / p.depth);
        while ((2 << p.lg_lanes) <= kDotTileMaxLanes && (256 >> (p.lg_lanes + 1)) >= per_level &&
               (4 << (p.lg_lanes + 1)) <= K)
            ++p.lg_lanes;
        *plan = p;
        return true;
    }
    return false;
}

bool dot_tile_eligible(const hq_dot_classes& m, int K, int shape, DotTilePlan* plan) {
    DotMatrixInfo info;
    return dot_matrix_info(m, &info) && dot_tile_eligible(info, K, shape, plan);
}

// Measured (profiles/dot_tile_c3.json), Knuth's matrix and a 16 x 16 permutation, P = 1 and 4: with a
// 32 x 32 or 64 x 32 tile the tiled form beat the chain by more than the chain's spread in every case
// at 512^2, K = 16 and at 1024^2, K = 64; the 16 x 16 tile lost one of them (1024^2, P = 4),
// and at 4096^2 the tiled form lost at K = 256 (three cases of four).  Auto stays inside what won:
// not the 16 x 16 tile, no more pixels than 1024^2 (nothing between that and 4096^2 was measured) and
// no larger pixels x P x K than 1024^2 x 4 x 64 = 2^28.  The rule does not look at the matrix: the
// two measured ones span 64 and 256 classes.
bool dot_tile_auto(int W, int H, int P, int K, int shape) {
    const int64_t pixels = (int64_t)W * H;
    return shape >= 1 && pixels <= (int64_t)1 << 20 && pixels * P * K <= (int64_t)1 << 28;
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

// The same recurrence with the columns beside the rows: p's extent to the left and right shifted
// by dx.  (The rows are hq_dot_reach's own: the two recurrences do not meet.)
int hq_dot_reach2(const hq_dot_classes* m, int* above, int* below, int* left, int* right) {
    if (!above || !below || !left || !right || !hq_dot_classes_legal(m)) return HQ_ERR_ARG;
    const int n = m->n, cells = n * n;
    int cell_of[hq::kDotCells], lf[hq::kDotCells] = {}, rt[hq::kDotCells] = {};
    for (int c = 0; c < cells; ++c) cell_of[m->cls[c]] = c;
    int l = 0, r = 0;
    for (int k = 0; k < cells; ++k) {
        const int c = cell_of[k], cx = c % n, cy = c / n;
        for (int d = 0; d < 8; ++d) {
            const int dx = hq::dot_dx(d), p = (cy + hq::dot_dy(d) + n) % n * n + (cx + dx + n) % n;
            if (m->cls[p] >= k) continue;
            lf[c] = std::max(lf[c], lf[p] - dx);
            rt[c] = std::max(rt[c], rt[p] + dx);
        }
        l = std::max(l, lf[c]);
        r = std::max(r, rt[c]);
    }
    hq_dot_reach(m, above, below);
    *left = l;
    *right = r;
    return HQ_OK;
}

// In ascending class every lower neighbour's level is final when the cell takes its own.
int hq_dot_levels(const hq_dot_classes* m, int32_t* level, int* depth) {
    if (!level || !depth || !hq_dot_classes_legal(m)) return HQ_ERR_ARG;
    const int n = m->n, cells = n * n;
    int cell_of[hq::kDotCells];
    for (int c = 0; c < cells; ++c) cell_of[m->cls[c]] = c;
    int32_t lv[hq::kDotCells] = {};
    int deepest = 0;
    for (int k = 0; k < cells; ++k) {
        const int c = cell_of[k], cx = c % n, cy = c / n;
        int32_t own = 0;
        for (int d = 0; d < 8; ++d) {
            const int p = (cy + hq::dot_dy(d) + n) % n * n + (cx + hq::dot_dx(d) + n) % n;
            if (m->cls[p] < k) own = std::max(own, lv[p] + 1);
        }
        lv[c] = own;
        deepest = std::max(deepest, (int)own);
    }
    std::memset(level, 0, sizeof(int32_t) * hq::kDotCells);
    std::memcpy(level, lv, sizeof(int32_t) * cells);
    *depth = deepest + 1;
    return HQ_OK;
}

}  // extern "C"
