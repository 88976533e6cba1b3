// dot_reach_check.cpp -- hq_dot_reach (hq_dot_classes.cpp: how many rows above and below a pixel
// the pixels its index depends on can lie) against a brute-force search of the tiled plane, on
// the matrices whose reach is known, their transposes and vertical flips, and random
// permutations of each side.  Stand-alone, built with the address and undefined-behaviour
// sanitizers (make dot_reach_check).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <utility>
#include <vector>

#include "../../include/hq.h"

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

// The definition, searched: from every cell of one tile, every position of the plane that steps
// to one of the 8 neighbours of a strictly lower class lead to (whether a position is reached
// does not depend on the way there, so each is expanded once); the largest distance up and down.
// A path has at most n^2 - 1 steps, so the positions stay within n^2 of the start.
void reach_ref(const hq_dot_classes& m, int* above, int* below) {
    const int n = m.n, r = n * n, side = 2 * r + 1;
    static std::vector<int> stamp;
    static int tick = 0;
    if ((int)stamp.size() < side * side) stamp.assign((size_t)side * side, 0), tick = 0;
    int up = 0, down = 0;
    std::vector<std::pair<int, int>> todo;
    for (int sy = 0; sy < n; ++sy)
        for (int sx = 0; sx < n; ++sx) {
            ++tick;
            todo.assign(1, {0, 0});
            stamp[(size_t)r * side + r] = tick;
            while (!todo.empty()) {
                const auto [ox, oy] = todo.back();
                todo.pop_back();
                up = std::max(up, -oy);
                down = std::max(down, oy);
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
    *above = up;
    *below = down;
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

hq_dot_classes flipped(const hq_dot_classes& m) {
    hq_dot_classes f{};
    f.n = m.n;
    for (int y = 0; y < m.n; ++y)
        for (int x = 0; x < m.n; ++x) f.cls[y * m.n + x] = m.cls[(m.n - 1 - y) * m.n + x];
    return f;
}

void check_against_search(const hq_dot_classes& m) {
    int a = -1, b = -1, ra = -2, rb = -2;
    CHECK(hq_dot_reach(&m, &a, &b) == HQ_OK);
    reach_ref(m, &ra, &rb);
    CHECK(a == ra);
    CHECK(b == rb);
    CHECK(a >= 1 && b >= 1 && a <= m.n * m.n - 1 && b <= m.n * m.n - 1);
}

void check_known(const hq_dot_classes& m, int above, int below) {
    int a = -1, b = -1;
    CHECK(hq_dot_reach(&m, &a, &b) == HQ_OK);
    CHECK(a == above);
    CHECK(b == below);
    check_against_search(m);
    // a vertical flip swaps the two sides; a transpose is another matrix, searched
    const hq_dot_classes f = flipped(m);
    CHECK(hq_dot_reach(&f, &a, &b) == HQ_OK);
    CHECK(a == below && b == above);
    check_against_search(f);
    check_against_search(transposed(m));
}

}  // namespace

int main() {
    hq_dot_classes knuth;
    CHECK(hq_dot_preset(HQ_DOT_KNUTH8, &knuth) == HQ_OK);
    check_known(knuth, 5, 5);
    check_known(row_major(4), 3, 1);
    check_known(row_major(8), 7, 1);
    check_known(row_major(16), 15, 1);

    // refusals: the outputs stay what they were
    int a = -7, b = -7;
    CHECK(hq_dot_reach(nullptr, &a, &b) == HQ_ERR_ARG);
    CHECK(hq_dot_reach(&knuth, nullptr, &b) == HQ_ERR_ARG);
    CHECK(hq_dot_reach(&knuth, &a, nullptr) == HQ_ERR_ARG);
    hq_dot_classes bad = knuth;
    bad.cls[3] = bad.cls[4];
    CHECK(hq_dot_reach(&bad, &a, &b) == HQ_ERR_ARG);
    bad = knuth;
    bad.n = 5;
    CHECK(hq_dot_reach(&bad, &a, &b) == HQ_ERR_ARG);
    CHECK(a == -7 && b == -7);

    int past_side = 0;  // a 4 x 4 permutation can reach further than its side: paths cross tile borders
    std::mt19937 rng(20251);
    for (int n : {4, 8, 16})
        for (int t = 0; t < 300; ++t) {
            hq_dot_classes m = row_major(n);
            std::shuffle(m.cls, m.cls + n * n, rng);
            check_against_search(m);
            int ra = 0, rb = 0;
            hq_dot_reach(&m, &ra, &rb);
            past_side += n == 4 && std::max(ra, rb) > 4;
        }
    CHECK(past_side > 0);

    if (g_failed) {
        std::printf("dot_reach_check: %d check(s) FAILED\n", g_failed);
        return 1;
    }
    std::printf("dot_reach_check: ok\n");
    return 0;
}
