// dot_tile_check.cpp -- what the tiled form of dot diffusion rests on (hq_dot_classes.cpp):
// hq_dot_reach2 against a brute-force search of descending paths on the tiled plane, hq_dot_levels
// against its definition, the schedule (dot_schedule) against the levels, and the eligibility rule
// (dot_tile_eligible) on the matrices hq.h names -- Knuth's, random permutations of each side, the
// row-major and column-major 16 x 16.  Stand-alone, built with the address and undefined-behaviour
// sanitizers (make dot_tile_check).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <utility>
#include <vector>

#include "hq_dot.h"

namespace {

int g_failed = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::printf("%s:%d: %s\n", __FILE__, __LINE__, #cond);      \
            ++g_failed;                                                 \
        }                                                               \
    } while (0)

int class_at(const hq_dot_classes& m, int x, int y) {
    return m.cls[((y % m.n + m.n) % m.n) * m.n + (x % m.n + m.n) % m.n];
}

// The definition, searched: from every cell of one tile, every position that steps to one of the
// 8 neighbours of a strictly lower class lead to, each expanded once; the largest distance in each
// direction.  A path has at most n^2 - 1 steps, so the positions stay within n^2 of the start.
void reach_ref(const hq_dot_classes& m, int out[4]) {
    const int n = m.n, r = n * n, side = 2 * r + 1;
    std::vector<int> stamp((size_t)side * side, 0);
    int tick = 0;
    int up = 0, down = 0, left = 0, right = 0;
    std::vector<std::pair<int, int>> todo;
    for (int sy = 0; sy < n; ++sy)
        for (int sx = 0; sx < n; ++sx) {
            ++tick;
            todo.assign(1, {0, 0});
            stamp[(size_t)r * side + r] = tick;
            while (!todo.empty()) {
                const auto [ox, oy] = todo.back();
                todo.pop_back();
                up = std::max(up, -oy), down = std::max(down, oy);
                left = std::max(left, -ox), right = std::max(right, ox);
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx) {
                        if (!dx && !dy) continue;
                        if (class_at(m, sx + ox + dx, sy + oy + dy) >= class_at(m, sx + ox, sy + oy)) continue;
                        int& st = stamp[(size_t)(oy + dy + r) * side + (ox + dx + r)];
                        if (st == tick) continue;
                        st = tick;
                        todo.push_back({ox + dx, oy + dy});
                    }
            }
        }
    out[0] = up, out[1] = down, out[2] = left, out[3] = right;
}

hq_dot_classes row_major(int n) {
    hq_dot_classes m{};
    m.n = n;
    for (int i = 0; i < n * n; ++i) m.cls[i] = i;
    return m;
}

hq_dot_classes transposed(const hq_dot_classes& m) {
    hq_dot_classes t{};
    t.n = m.n;
    for (int y = 0; y < m.n; ++y)
        for (int x = 0; x < m.n; ++x) t.cls[y * m.n + x] = m.cls[x * m.n + y];
    return t;
}

void reach2(const hq_dot_classes& m, int out[4]) {
    out[0] = out[1] = out[2] = out[3] = -1;
    CHECK(hq_dot_reach2(&m, &out[0], &out[1], &out[2], &out[3]) == HQ_OK);
}

void check_reach(const hq_dot_classes& m) {
    int got[4], want[4], a = -1, b = -1;
    reach2(m, got);
    reach_ref(m, want);
    for (int i = 0; i < 4; ++i) CHECK(got[i] == want[i]);
    CHECK(hq_dot_reach(&m, &a, &b) == HQ_OK);
    CHECK(a == got[0] && b == got[1]);
    // a transpose swaps the rows with the columns
    int t[4];
    reach2(transposed(m), t);
    CHECK(t[0] == got[2] && t[1] == got[3] && t[2] == got[0] && t[3] == got[1]);
}

// The levels against the definition, cell by cell, and the schedule against the levels.
int check_levels(const hq_dot_classes& m) {
    const int n = m.n, cells = n * n;
    int32_t level[hq::kDotCells];
    std::fill(level, level + hq::kDotCells, -5);
    int depth = -5, deepest = 0;
    CHECK(hq_dot_levels(&m, level, &depth) == HQ_OK);
    for (int cy = 0; cy < n; ++cy)
        for (int cx = 0; cx < n; ++cx) {
            int want = 0;
            for (int d = 0; d < 8; ++d) {
                const int px = cx + hq::dot_dx(d), py = cy + hq::dot_dy(d);
                if (class_at(m, px, py) < m.cls[cy * n + cx])
                    want = std::max(want, 1 + level[((py + n) % n) * n + (px + n) % n]);
            }
            CHECK(level[cy * n + cx] == want);
            deepest = std::max(deepest, want);
        }
    CHECK(depth == deepest + 1);
    for (int i = cells; i < hq::kDotCells; ++i) CHECK(level[i] == 0);

    hq::DotSchedule s;
    hq::dot_schedule(m, &s);
    CHECK(s.depth == depth);
    CHECK(s.start[0] == 0 && s.start[depth] == (uint32_t)cells);
    bool seen[hq::kDotCells] = {};
    for (int l = 0; l < depth; ++l) {
        CHECK(s.start[l] < s.start[l + 1]);  // (every level has a cell)
        for (uint32_t i = s.start[l]; i < s.start[l + 1] && i < (uint32_t)cells; ++i) {
            CHECK(s.cell[i] < (uint32_t)cells && !seen[s.cell[i]] && level[s.cell[i]] == l);
            if (s.cell[i] < (uint32_t)cells) seen[s.cell[i]] = true;
        }
    }
    for (int l = depth; l <= hq::kDotCells; ++l) CHECK(s.start[l] == (uint32_t)cells);
    return depth;
}

bool eligible(const hq_dot_classes& m, int K, int shape, hq::DotTilePlan* p) {
    hq::DotTilePlan plan{};
    plan.shape = -3;
    const bool ok = hq::dot_tile_eligible(m, K, shape, &plan);
    if (!ok) CHECK(plan.shape == -3);  // (untouched)
    if (ok) {
        CHECK(plan.tw == hq::kDotTileW[plan.shape] && plan.th == hq::kDotTileH[plan.shape]);
        CHECK(plan.window == (plan.tw + plan.left + plan.right) * (plan.th + plan.above + plan.below));
        CHECK(plan.window * 12 <= hq::kDotTileErrBytes);
        CHECK(plan.lg_lanes >= 0 && (1 << plan.lg_lanes) <= hq::kDotTileMaxLanes);
        CHECK(plan.tw % hq::kDotSide == 0 && plan.th % hq::kDotSide == 0);
        if (shape) CHECK(plan.shape == shape - 1);
    }
    if (p) *p = plan;
    return ok;
}

}  // namespace

int main() {
    hq_dot_classes knuth;
    CHECK(hq_dot_preset(HQ_DOT_KNUTH8, &knuth) == HQ_OK);
    int r[4];
    reach2(knuth, r);
    CHECK(r[0] == 5 && r[1] == 5 && r[2] == 5 && r[3] == 5);
    check_reach(knuth);
    CHECK(check_levels(knuth) == 15);

    const hq_dot_classes rows = row_major(16), cols = transposed(rows);
    reach2(rows, r);
    CHECK(r[0] == 15 && r[1] == 1 && r[2] == 255 && r[3] == 17);
    check_reach(rows);
    check_reach(cols);
    CHECK(check_levels(rows) == 256);
    CHECK(check_levels(cols) == 256);
    for (int n : {4, 8}) {
        check_reach(row_major(n));
        CHECK(check_levels(row_major(n)) == n * n);
    }

    // the rule: Knuth's under every shape and every K; the row- and column-major 16 x 16 under none
    hq::DotTilePlan plan;
    for (int shape = 0; shape <= hq::kDotTileShapes; ++shape)
        for (int K : {1, 2, 6, 16, 255, 256}) {
            CHECK(eligible(knuth, K, shape, &plan));
            CHECK(plan.depth == 15 && plan.above == 5 && plan.left == 5);
            CHECK(!eligible(rows, K, shape, nullptr));
            CHECK(!eligible(cols, K, shape, nullptr));
        }
    CHECK(eligible(knuth, 256, 0, &plan) && plan.shape == hq::kDotTileShapes - 1);  // (0: the largest)
    CHECK(!eligible(knuth, 0, 0, nullptr));
    CHECK(!eligible(knuth, 257, 0, nullptr));
    CHECK(!eligible(knuth, 16, -1, nullptr));
    CHECK(!eligible(knuth, 16, hq::kDotTileShapes + 1, nullptr));
    hq_dot_classes bad = knuth;
    bad.cls[3] = bad.cls[4];
    CHECK(!eligible(bad, 16, 0, nullptr));

    // refusals: the outputs stay what they were
    int a = -7, b = -7, c = -7, d = -7, depth = -7;
    int32_t level[hq::kDotCells];
    std::fill(level, level + hq::kDotCells, -7);
    CHECK(hq_dot_reach2(nullptr, &a, &b, &c, &d) == HQ_ERR_ARG);
    CHECK(hq_dot_reach2(&knuth, nullptr, &b, &c, &d) == HQ_ERR_ARG);
    CHECK(hq_dot_reach2(&knuth, &a, nullptr, &c, &d) == HQ_ERR_ARG);
    CHECK(hq_dot_reach2(&knuth, &a, &b, nullptr, &d) == HQ_ERR_ARG);
    CHECK(hq_dot_reach2(&knuth, &a, &b, &c, nullptr) == HQ_ERR_ARG);
    CHECK(hq_dot_reach2(&bad, &a, &b, &c, &d) == HQ_ERR_ARG);
    CHECK(hq_dot_levels(&bad, level, &depth) == HQ_ERR_ARG);
    CHECK(hq_dot_levels(nullptr, level, &depth) == HQ_ERR_ARG);
    CHECK(hq_dot_levels(&knuth, nullptr, &depth) == HQ_ERR_ARG);
    CHECK(hq_dot_levels(&knuth, level, nullptr) == HQ_ERR_ARG);
    bad = knuth;
    bad.n = 5;
    CHECK(hq_dot_reach2(&bad, &a, &b, &c, &d) == HQ_ERR_ARG);
    CHECK(hq_dot_levels(&bad, level, &depth) == HQ_ERR_ARG);
    CHECK(a == -7 && b == -7 && c == -7 && d == -7 && depth == -7);
    for (int i = 0; i < hq::kDotCells; ++i) CHECK(level[i] == -7);
    hq::DotSchedule s;
    hq::dot_schedule(bad, &s);
    CHECK(s.depth == 0);

    // random permutations of each side: the search, the levels, and every one of them eligible
    // under every shape (the largest sums of reaches seen: what the LDS budget was chosen for)
    int most_rows = 0, most_cols = 0;
    std::mt19937 rng(20252);
    for (int n : {4, 8, 16})
        for (int t = 0; t < 120; ++t) {
            hq_dot_classes m = row_major(n);
            std::shuffle(m.cls, m.cls + n * n, rng);
            check_reach(m);
            const int dep = check_levels(m);
            CHECK(dep >= 2 && dep <= n * n);
            reach2(m, r);
            most_rows = std::max(most_rows, r[0] + r[1]), most_cols = std::max(most_cols, r[2] + r[3]);
            for (int shape = 0; shape <= hq::kDotTileShapes; ++shape) CHECK(eligible(m, 256, shape, nullptr));
        }
    std::printf("dot_tile_check: largest above + below %d, left + right %d over the permutations\n", most_rows, most_cols);

    if (g_failed) {
        std::printf("dot_tile_check: %d check(s) FAILED\n", g_failed);
        return 1;
    }
    std::printf("dot_tile_check: ok\n");
    return 0;
}
