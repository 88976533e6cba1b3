// seed_check.cpp -- hq_median_cut's edge cases as a stand-alone host program,
// built and run under the address and undefined-behaviour sanitizers by
// `make seed_check` (hq_seed.cpp and this file: no GPU code, no Python).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/hq.h"

namespace {

int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

struct Hist {
    int bits;
    std::vector<int64_t> cells;
    explicit Hist(int b) : bits(b), cells((size_t)4 << (3 * b), 0) {}
    // n pixels of the byte colour (r, g, b) into their cell (den 255)
    void add(int r, int g, int b, int64_t n) {
        const int sh = 8 - bits;
        const size_t i = ((size_t)(r >> sh) << (2 * bits)) | ((size_t)(g >> sh) << bits) | (size_t)(b >> sh);
        cells[4 * i] += r * n, cells[4 * i + 1] += g * n, cells[4 * i + 2] += b * n, cells[4 * i + 3] += n;
    }
};

int cut(const Hist& h, int64_t den, int K, std::vector<float>& pal, int* made) {
    pal.assign((size_t)4 * (K > 0 ? K : 1), -1.0f);
    *made = -1;
    return hq_median_cut(h.cells.data(), h.bits, den, K, pal.data(), made);
}

}  // namespace

int main() {
    std::vector<float> pal;
    int made;
    for (int bits = 2; bits <= 6; ++bits) {
        {  // one non-empty cell: one box, every colour equal
            Hist h(bits);
            h.add(51, 102, 204, 1000);
            CHECK(cut(h, 255, 5, pal, &made) == HQ_OK && made == 1);
            for (int i = 0; i < 5; ++i)
                CHECK(pal[4 * i] == 51.0f / 255 && pal[4 * i + 1] == 102.0f / 255 && pal[4 * i + 2] == 204.0f / 255 &&
                      pal[4 * i + 3] == 0.0f);
        }
        {  // fewer non-empty cells than K: made = their number, then the cyclic copies
            Hist h(bits);
            h.add(0, 0, 0, 3), h.add(255, 0, 0, 4), h.add(0, 255, 255, 5);
            CHECK(cut(h, 255, 8, pal, &made) == HQ_OK && made == 3);
            for (int i = 3; i < 8; ++i)
                for (int a = 0; a < 4; ++a) CHECK(pal[4 * i + a] == pal[4 * (i % 3) + a]);
            for (int i = 0; i < 3; ++i)
                for (int a = 0; a < 3; ++a) CHECK(pal[4 * i + a] == 0.0f || pal[4 * i + a] == 1.0f);
        }
        {  // K = 1: the mean of the image
            Hist h(bits);
            h.add(0, 0, 0, 1), h.add(255, 255, 255, 3);
            CHECK(cut(h, 255, 1, pal, &made) == HQ_OK && made == 1);
            CHECK(pal[0] == 0.75f && pal[1] == 0.75f && pal[2] == 0.75f && pal[3] == 0.0f);
        }
        {  // all the mass in one corner cell but one pixel: the cut is clamped to hi - 1
            Hist h(bits);
            h.add(255, 255, 255, ((int64_t)1 << 33) + 7), h.add(0, 0, 0, 1);
            CHECK(cut(h, 255, 2, pal, &made) == HQ_OK && made == 2);
            CHECK(pal[0] == 0.0f && pal[4] == 1.0f && pal[5] == 1.0f && pal[6] == 1.0f);
        }
        {  // every cell non-empty, den 2^32, more colours asked for than cells at 2 bits
            Hist h(bits);
            const int nb = 1 << bits;
            for (size_t i = 0; i < h.cells.size() / 4; ++i) {
                const int64_t n = 1 + (int64_t)(i % 7);
                const int64_t r = (int64_t)(i >> (2 * bits)), g = (int64_t)((i >> bits) & (nb - 1)), b = (int64_t)(i & (nb - 1));
                h.cells[4 * i] = n * ((r << 32) / nb), h.cells[4 * i + 1] = n * ((g << 32) / nb);
                h.cells[4 * i + 2] = n * ((b << 32) / nb), h.cells[4 * i + 3] = n;
            }
            CHECK(cut(h, (int64_t)1 << 32, 300, pal, &made) == HQ_OK);
            CHECK(made == (bits == 2 ? 64 : 300));
            for (int i = 0; i < 300; ++i)
                for (int a = 0; a < 3; ++a) CHECK(pal[4 * i + a] >= 0.0f && pal[4 * i + a] < 1.0f);
        }
    }
    {  // arguments
        Hist h(5);
        h.add(1, 2, 3, 4);
        CHECK(cut(h, 255, 0, pal, &made) == HQ_ERR_ARG);
        CHECK(cut(h, 256, 4, pal, &made) == HQ_ERR_ARG);
        CHECK(hq_median_cut(h.cells.data(), 1, 255, 4, pal.data(), &made) == HQ_ERR_ARG);
        CHECK(hq_median_cut(h.cells.data(), 7, 255, 4, pal.data(), &made) == HQ_ERR_ARG);
        Hist neg(5);
        neg.add(1, 2, 3, 4), neg.cells[4 * 77 + 3] = -1;
        CHECK(cut(neg, 255, 4, pal, &made) == HQ_ERR_ARG);
        Hist empty(5);
        CHECK(cut(empty, 255, 4, pal, &made) == HQ_ERR_ARG);
        CHECK(made == -1);  // untouched by a refusal
    }
    if (failures) {
        std::fprintf(stderr, "seed_check: %d failure(s)\n", failures);
        return EXIT_FAILURE;
    }
    std::puts("seed_check ok");
    return EXIT_SUCCESS;
}
