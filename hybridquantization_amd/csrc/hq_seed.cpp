// hq_seed.cpp -- a palette from a colour histogram by median cut: the start of a
// search that knows the image (hq_median_cut, include/hq.h states the rule).
// libhq's own addition: the reference starts from random colours (SW:40-52).
// Host code only, no context; integers until the final means, which are the
// k-means update's (lloyd_mean), so a numpy restatement matches bit for bit.
#include <algorithm>
#include <cstdint>
#include <queue>
#include <vector>

#include "../../include/hq.h"
#include "hq_lloyd.h"

namespace {

struct Cell {
    uint8_t x[3];     // cell coordinates R, G, B
    int64_t sum[3];
    int64_t count;
};

// A box: the cells order[begin .. end), their tight bounds and their count.
struct Box {
    size_t begin, end;
    int lo[3], hi[3];
    int64_t count;
};

void tighten(const std::vector<Cell>& cells, Box& b) {
    for (int a = 0; a < 3; ++a) b.lo[a] = 255, b.hi[a] = 0;
    b.count = 0;
    for (size_t i = b.begin; i < b.end; ++i) {
        const Cell& c = cells[i];
        for (int a = 0; a < 3; ++a) {
            b.lo[a] = std::min<int>(b.lo[a], c.x[a]);
            b.hi[a] = std::max<int>(b.hi[a], c.x[a]);
        }
        b.count += c.count;
    }
}

int64_t priority(const Box& b) {
    int64_t e2 = 0;
    for (int a = 0; a < 3; ++a) e2 += (int64_t)(b.hi[a] - b.lo[a]) * (b.hi[a] - b.lo[a]);
    return b.count * e2;
}

struct Entry {
    int64_t prio;
    int idx;
    // (the heap's top is its largest: the highest priority, then the lowest index)
    bool operator<(const Entry& o) const { return prio != o.prio ? prio < o.prio : idx > o.idx; }
};

}  // namespace

extern "C" int hq_median_cut(const int64_t* hist, int bits, int64_t den, int K, float* palette, int* made) {
    if (!hist || !palette || !made || K < 1 || bits < 2 || bits > 6) return HQ_ERR_ARG;
    const bool bytes = den == 255;
    if (!bytes && den != ((int64_t)1 << 32)) return HQ_ERR_ARG;
    const int nb = 1 << bits;
    const size_t ncells = (size_t)1 << (3 * bits);
    const int64_t max_total = (int64_t)1 << 48;  // count (e_R^2 + e_G^2 + e_B^2) < 2^48 3 63^2 < 2^62
    int64_t total = 0;
    size_t nonempty = 0;
    for (size_t i = 0; i < ncells; ++i) {
        const int64_t n = hist[4 * i + 3];
        if (n < 0 || n > max_total || (total += n) > max_total) return HQ_ERR_ARG;
        nonempty += n > 0;
    }
    if (total == 0) return HQ_ERR_ARG;

    std::vector<Cell> cells;
    cells.reserve(nonempty);
    for (size_t i = 0; i < ncells; ++i) {
        const int64_t* h = hist + 4 * i;
        if (h[3] == 0) continue;
        Cell c;
        c.x[0] = (uint8_t)(i >> (2 * bits));
        c.x[1] = (uint8_t)((i >> bits) & (size_t)(nb - 1));
        c.x[2] = (uint8_t)(i & (size_t)(nb - 1));
        c.sum[0] = h[0], c.sum[1] = h[1], c.sum[2] = h[2];
        c.count = h[3];
        cells.push_back(c);
    }

    std::vector<Box> boxes;
    boxes.reserve(std::min<size_t>((size_t)K, nonempty));
    std::priority_queue<Entry> heap;
    {
        Box b{0, cells.size(), {}, {}, 0};
        tighten(cells, b);
        boxes.push_back(b);
        if (priority(b) > 0) heap.push({priority(b), 0});
    }
    while ((int64_t)boxes.size() < (int64_t)K && !heap.empty()) {
        const int bi = heap.top().idx;
        heap.pop();
        Box lower = boxes[bi];
        int axis = 0;  // the largest extent; a tie to R, then G, then B
        for (int a = 1; a < 3; ++a)
            if (lower.hi[a] - lower.lo[a] > lower.hi[axis] - lower.lo[axis]) axis = a;
        int64_t m[64] = {};
        for (size_t i = lower.begin; i < lower.end; ++i) m[cells[i].x[axis]] += cells[i].count;
        int t = lower.lo[axis];
        for (int64_t below = 0; t < lower.hi[axis]; ++t)
            if (2 * (below += m[t]) >= lower.count) break;
        t = std::min(t, lower.hi[axis] - 1);
        const auto mid = std::partition(cells.begin() + (std::ptrdiff_t)lower.begin, cells.begin() + (std::ptrdiff_t)lower.end,
                                        [&](const Cell& c) { return c.x[axis] <= t; });
        Box upper{(size_t)(mid - cells.begin()), lower.end, {}, {}, 0};
        lower.end = upper.begin;
        tighten(cells, lower);
        tighten(cells, upper);
        boxes[bi] = lower;
        boxes.push_back(upper);
        if (priority(lower) > 0) heap.push({priority(lower), bi});
        if (priority(upper) > 0) heap.push({priority(upper), (int)boxes.size() - 1});
    }

    const int n = (int)boxes.size();
    for (int i = 0; i < n; ++i) {
        const Box& b = boxes[i];
        int64_t sum[3] = {0, 0, 0};
        for (size_t j = b.begin; j < b.end; ++j)
            for (int a = 0; a < 3; ++a) sum[a] += cells[j].sum[a];
        for (int a = 0; a < 3; ++a) palette[4 * i + a] = hq::lloyd_mean(sum[a], b.count, bytes);
        palette[4 * i + 3] = 0.0f;
    }
    for (int i = n; i < K; ++i)
        for (int a = 0; a < 4; ++a) palette[4 * i + a] = palette[4 * (i % n) + a];
    *made = n;
    return HQ_OK;
}
