// dot_check.cpp -- hq_dot_classes.cpp (the preset, the legality rule, the baron count and the
// per-cell tables of hq_dot_population's class matrices) against a brute-force statement of
// hq.h's rules, on their edge cases and on random permutations of each side.  Stand-alone,
// built with the address and undefined-behaviour sanitizers (make dot_check).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <set>

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

// hq.h's eight offsets and weights, written out.
const int kDx[8] = {-1, 0, 1, -1, 1, -1, 0, 1}, kDy[8] = {-1, -1, -1, 0, 0, 1, 1, 1};
const int kWt[8] = {1, 2, 1, 2, 2, 1, 2, 1};

bool legal_ref(const hq_dot_classes& m) {
    if (m.n != 4 && m.n != 8 && m.n != 16) return false;
    std::set<int32_t> seen;
    for (int i = 0; i < m.n * m.n; ++i) {
        if (m.cls[i] < 0 || m.cls[i] >= m.n * m.n) return false;
        seen.insert(m.cls[i]);
    }
    return (int)seen.size() == m.n * m.n;
}

int class_at(const hq_dot_classes& m, int x, int y) {
    return m.cls[((y % m.n + m.n) % m.n) * m.n + (x % m.n + m.n) % m.n];
}

int barons_ref(const hq_dot_classes& m) {
    int barons = 0;
    for (int y = 0; y < m.n; ++y)
        for (int x = 0; x < m.n; ++x) {
            bool all_lower = true;
            for (int d = 0; d < 8; ++d) all_lower = all_lower && class_at(m, x + kDx[d], y + kDy[d]) < class_at(m, x, y);
            barons += all_lower;
        }
    return barons;
}

void check_tables(const hq_dot_classes& m) {
    uint32_t lower[hq::kDotCells], higher[hq::kDotCells];
    std::memset(lower, 0xAB, sizeof lower);
    std::memset(higher, 0xAB, sizeof higher);
    hq::dot_tables(m, lower, higher);
    for (int y = 0; y < m.n; ++y)
        for (int x = 0; x < m.n; ++x) {
            const int c = y * m.n + x, own = m.cls[c];
            int nl = 0, last = -1;
            bool ended = false;
            for (int i = 0; i < 8; ++i) {
                const uint32_t d = lower[c] >> (4 * i) & 15u;
                if (d == hq::kDotEnd) {
                    ended = true;
                    continue;
                }
                CHECK(!ended && d < 8);
                if (d >= 8) continue;
                const int k = class_at(m, x + kDx[d], y + kDy[d]);
                CHECK(k < own && k > last);  // lower, ascending, pairwise distinct
                CHECK(!(higher[c] >> d & 1u));
                last = k;
                ++nl;
            }
            int nh = 0;
            for (int d = 0; d < 8; ++d) {
                const bool hi = class_at(m, x + kDx[d], y + kDy[d]) > own;
                CHECK((higher[c] >> d & 1u) == (hi ? 1u : 0u));
                nh += hi;
            }
            CHECK(nl + nh == 8 && higher[c] < 256u);
        }
    for (int c = m.n * m.n; c < hq::kDotCells; ++c) CHECK(lower[c] == 0 && higher[c] == 0);
}

void check_one(const hq_dot_classes& m) {
    const bool want = legal_ref(m);
    CHECK(hq_dot_classes_legal(&m) == (want ? 1 : 0));
    CHECK(hq_dot_barons(&m) == (want ? barons_ref(m) : -1));
    if (want) check_tables(m);
}

hq_dot_classes identity(int n) {
    hq_dot_classes m;
    std::memset(&m, 0, sizeof m);
    m.n = n;
    for (int i = 0; i < n * n && i < hq::kDotCells; ++i) m.cls[i] = i;
    return m;
}

}  // namespace

int main() {
    // the helpers of hq_dot.h are hq.h's offsets and weights
    for (int d = 0; d < 8; ++d) {
        CHECK(hq::dot_dx(d) == kDx[d] && hq::dot_dy(d) == kDy[d] && hq::dot_weight(d) == kWt[d]);
        CHECK(hq::dot_dx(7 - d) == -kDx[d] && hq::dot_dy(7 - d) == -kDy[d]);
        CHECK(((hq::kDotOrth >> d & 1u) != 0) == (kWt[d] == 2) && ((hq::kDotDiag >> d & 1u) != 0) == (kWt[d] == 1));
    }
    // the preset
    static const int32_t kWant[64] = {34, 48, 40, 32, 29, 15, 23, 31, 42, 58, 56, 53, 21, 5,  7,  10,
                                      50, 62, 61, 45, 13, 1,  2,  18, 38, 46, 54, 37, 25, 17, 9,  26,
                                      28, 14, 22, 30, 35, 49, 41, 33, 20, 4,  6,  11, 43, 59, 57, 52,
                                      12, 0,  3,  19, 51, 63, 60, 44, 24, 16, 8,  27, 39, 47, 55, 36};
    hq_dot_classes k;
    std::memset(&k, 0x5C, sizeof k);
    CHECK(hq_dot_preset(HQ_DOT_KNUTH8, &k) == HQ_OK && k.n == 8);
    CHECK(!std::memcmp(k.cls, kWant, sizeof kWant));
    for (int i = 64; i < 256; ++i) CHECK(k.cls[i] == 0);
    CHECK(hq_dot_classes_legal(&k) == 1 && hq_dot_barons(&k) == 2 && barons_ref(k) == 2);
    check_one(k);
    CHECK(hq_dot_preset(-1, &k) == HQ_ERR_ARG && hq_dot_preset(HQ_DOT_COUNT, &k) == HQ_ERR_ARG);
    CHECK(hq_dot_preset(HQ_DOT_KNUTH8, nullptr) == HQ_ERR_ARG);
    CHECK(hq_dot_classes_legal(nullptr) == 0 && hq_dot_barons(nullptr) == -1);
    // sides
    for (int n : {-8, 0, 1, 2, 3, 5, 7, 9, 15, 17, 32, 64, 1 << 30}) {
        hq_dot_classes m = identity(n > 16 || n < 0 ? 16 : n);
        m.n = n;
        CHECK(hq_dot_classes_legal(&m) == 0 && hq_dot_barons(&m) == -1);
    }
    for (int n : {4, 8, 16}) {
        hq_dot_classes m = identity(n);
        check_one(m);
        CHECK(hq_dot_classes_legal(&m) == 1);
        // the raster order: every cell but the last has a higher one to its right or below it
        CHECK(hq_dot_barons(&m) == 1);
        hq_dot_classes bad = m;
        bad.cls[3] = bad.cls[5];  // a repeated class
        check_one(bad);
        CHECK(!hq_dot_classes_legal(&bad));
        bad = m;
        bad.cls[n * n - 1] = n * n;  // outside 0 .. n^2 - 1
        check_one(bad);
        CHECK(!hq_dot_classes_legal(&bad));
        bad = m;
        bad.cls[0] = -1;
        check_one(bad);
        CHECK(!hq_dot_classes_legal(&bad));
        if (n < 16) {  // entries past n^2 are not read
            hq_dot_classes junk = m;
            for (int i = n * n; i < 256; ++i) junk.cls[i] = -77;
            check_one(junk);
            CHECK(hq_dot_classes_legal(&junk));
        }
        // random permutations
        std::mt19937 rng(1000 + n);
        for (int rep = 0; rep < 50; ++rep) {
            hq_dot_classes r = identity(n);
            for (int i = n * n - 1; i > 0; --i) std::swap(r.cls[i], r.cls[rng() % (uint32_t)(i + 1)]);
            check_one(r);
            CHECK(hq_dot_classes_legal(&r));
        }
    }
    if (g_failed) {
        std::printf("dot_check: %d failed\n", g_failed);
        return 1;
    }
    std::printf("dot_check ok\n");
    return 0;
}
