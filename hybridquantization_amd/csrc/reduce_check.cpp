// reduce_check.cpp -- hq_reduced_size's and hq_reduce_weights' edge cases as a stand-alone
// host program, built and run under the address and undefined-behaviour sanitizers by
// `make reduce_check` (hq_reduce.cpp and this file: no GPU code, no Python).  Every output
// vector is sized exactly, so a write past the reduced map is the sanitizer's to find.
#include <cstdint>
#include <cstdio>
#include <utility>
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

std::vector<uint8_t> reduce(const std::vector<uint8_t>& src, int w, int h, int f, int is_mask, int* rw, int* rh) {
    CHECK(hq_reduced_size(w, h, f, rw, rh) == HQ_OK);
    std::vector<uint8_t> out((size_t)*rw * *rh, 0xAB);
    CHECK(hq_reduce_weights(src.data(), w, h, f, is_mask, out.data()) == HQ_OK);
    return out;
}

// the definition, block by block, in the slowest possible way
uint8_t block(const std::vector<uint8_t>& src, int w, int h, int f, int is_mask, int X, int Y) {
    long sum = 0, n = 0;
    bool any = false;
    for (int y = Y * f; y < Y * f + f && y < h; ++y)
        for (int x = X * f; x < X * f + f && x < w; ++x) {
            const int b = src[(size_t)y * w + x];
            sum += is_mask ? (b ? 255 : 0) : b;
            any = any || b != 0;
            ++n;
        }
    long v = (2 * sum + n) / (2 * n);
    if (any && v == 0) v = 1;
    return (uint8_t)v;
}

void against_definition(const std::vector<uint8_t>& src, int w, int h, int f) {
    for (int is_mask = 0; is_mask < 2; ++is_mask) {
        int rw, rh;
        const std::vector<uint8_t> out = reduce(src, w, h, f, is_mask, &rw, &rh);
        for (int Y = 0; Y < rh; ++Y)
            for (int X = 0; X < rw; ++X) CHECK(out[(size_t)Y * rw + X] == block(src, w, h, f, is_mask, X, Y));
    }
}

}  // namespace

int main() {
    int rw = -1, rh = -1;
    // sizes: ceil, and the factor's range
    CHECK(hq_reduced_size(13, 7, 2, &rw, &rh) == HQ_OK && rw == 7 && rh == 4);
    CHECK(hq_reduced_size(16, 16, 4, &rw, &rh) == HQ_OK && rw == 4 && rh == 4);
    CHECK(hq_reduced_size(5, 9, 16, &rw, &rh) == HQ_OK && rw == 1 && rh == 1);
    CHECK(hq_reduced_size(5, 9, 1, &rw, &rh) == HQ_OK && rw == 5 && rh == 9);
    CHECK(hq_reduced_size(5, 9, 0, &rw, &rh) == HQ_ERR_ARG);
    CHECK(hq_reduced_size(5, 9, 17, &rw, &rh) == HQ_ERR_ARG);
    CHECK(hq_reduced_size(5, 9, -3, &rw, &rh) == HQ_ERR_ARG);
    CHECK(hq_reduced_size(0, 9, 2, &rw, &rh) == HQ_ERR_ARG);
    CHECK(hq_reduced_size(5, 9, 2, nullptr, &rh) == HQ_ERR_ARG);
    {
        std::vector<uint8_t> one(1, 9), out(1, 0xAB);
        CHECK(hq_reduce_weights(nullptr, 1, 1, 1, 0, out.data()) == HQ_ERR_ARG);
        CHECK(hq_reduce_weights(one.data(), 1, 1, 1, 0, nullptr) == HQ_ERR_ARG);
        CHECK(hq_reduce_weights(one.data(), 1, 1, 17, 0, out.data()) == HQ_ERR_ARG);
        CHECK(out[0] == 0xAB);  // (a refusal writes nothing)
    }
    // f = 1 is the identity for weights, and 0 / 255 for a mask
    {
        std::vector<uint8_t> src(5 * 3);
        for (size_t i = 0; i < src.size(); ++i) src[i] = (uint8_t)(i * 37 % 256);
        src[4] = 0;
        const std::vector<uint8_t> wts = reduce(src, 5, 3, 1, 0, &rw, &rh);
        CHECK(rw == 5 && rh == 3 && wts == src);
        const std::vector<uint8_t> msk = reduce(src, 5, 3, 1, 1, &rw, &rh);
        for (size_t i = 0; i < src.size(); ++i) CHECK(msk[i] == (src[i] ? 255 : 0));
    }
    // f larger than w and h: one block of the whole map, n = w h
    {
        std::vector<uint8_t> src = {10, 20, 30, 40, 50, 61};  // 3 x 2, sum 211, n 6: (422 + 6) / 12 = 35
        const std::vector<uint8_t> out = reduce(src, 3, 2, 16, 0, &rw, &rh);
        CHECK(rw == 1 && rh == 1 && out[0] == 35);
    }
    // ties round up: n = 4 sum 2 -> 0.5 -> 1; sum 6 -> 1.5 -> 2; partial blocks n = 2 (sum 1, sum 3) and n = 1
    {
        //  3 x 3 at f = 2: blocks n = 4, 2 / 2, 1
        std::vector<uint8_t> src = {1, 1, 1,
                                    0, 0, 0,
                                    2, 1, 7};
        const std::vector<uint8_t> out = reduce(src, 3, 3, 2, 0, &rw, &rh);
        CHECK(rw == 2 && rh == 2);
        CHECK(out[0] == 1);  // sum 2, n 4: 0.5 -> 1
        CHECK(out[1] == 1);  // sum 1, n 2: 0.5 -> 1
        CHECK(out[2] == 2);  // sum 3, n 2: 1.5 -> 2
        CHECK(out[3] == 7);  // n 1
        std::vector<uint8_t> six = {1, 2, 2, 1};  // sum 6, n 4: 1.5 -> 2
        CHECK(reduce(six, 2, 2, 2, 0, &rw, &rh)[0] == 2);
    }
    // the raise to 1, and the all-zero block that stays 0
    {
        std::vector<uint8_t> src(4 * 4, 0);
        src[0] = 1;  // block (0, 0): sum 1, n 4: 0.25 -> 0, raised to 1
        const std::vector<uint8_t> out = reduce(src, 4, 4, 2, 0, &rw, &rh);
        CHECK(out[0] == 1 && out[1] == 0 && out[2] == 0 && out[3] == 0);
        std::vector<uint8_t> big(16 * 16, 0);
        big[255] = 1;  // one byte of 1 in 256: far below a half
        CHECK(reduce(big, 16, 16, 16, 0, &rw, &rh)[0] == 1);
        CHECK(reduce(big, 16, 16, 16, 1, &rw, &rh)[0] == 1);  // mask: 255 / 256 -> 1 (0.996 + 0.5)
    }
    // mask against weights: a non-zero byte counts as 255
    {
        std::vector<uint8_t> src = {1, 0, 0, 0};
        CHECK(reduce(src, 2, 2, 2, 1, &rw, &rh)[0] == 64);  // 255 / 4 = 63.75 -> 64
        CHECK(reduce(src, 2, 2, 2, 0, &rw, &rh)[0] == 1);
        std::vector<uint8_t> full(4, 7);
        CHECK(reduce(full, 2, 2, 2, 1, &rw, &rh)[0] == 255);
        CHECK(reduce(full, 2, 2, 2, 0, &rw, &rh)[0] == 7);
        std::vector<uint8_t> top(16 * 16, 255);  // the largest sum: no overflow, 255 exactly
        CHECK(reduce(top, 16, 16, 16, 0, &rw, &rh)[0] == 255);
    }
    // every block of odd shapes against the definition
    {
        uint32_t s = 12345;
        for (const auto& g : {std::pair<int, int>{13, 7}, {10, 11}, {16, 16}, {5, 9}, {1, 1}, {33, 2}})
            for (int f : {1, 2, 3, 4, 7, 16}) {
                std::vector<uint8_t> src((size_t)g.first * g.second);
                for (auto& b : src) {
                    s = s * 1664525u + 1013904223u;
                    b = (s >> 28) < 5 ? 0 : (uint8_t)(s >> 16);
                }
                against_definition(src, g.first, g.second, f);
            }
    }
    if (failures) {
        std::fprintf(stderr, "reduce_check: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("reduce_check: ok\n");
    return 0;
}
