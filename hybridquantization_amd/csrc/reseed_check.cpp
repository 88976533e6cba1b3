// reseed_check.cpp -- hq_reseed_unused's and hq_reseed_unused_fixed's edge cases as a stand-alone host
// program, built and run under the address and undefined-behaviour sanitizers
// by `make reseed_check` (hq_reseed.cpp and this file: no GPU code, no Python).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

// Statistics of P palettes of K colours in hq_cluster_errors' layout.
struct Stats {
    int P, K;
    std::vector<int64_t> err;
    std::vector<float> worst, pal;
    Stats(int P_, int K_) : P(P_), K(K_), err((size_t)4 * P_ * K_, 0), worst((size_t)4 * P_ * K_, 0.f), pal((size_t)4 * P_ * K_) {
        for (size_t i = 0; i < pal.size(); ++i) pal[i] = i % 4 == 3 ? 0.f : -1.0f - (float)i;
        for (int i = 0; i < P * K; ++i) err[4 * (size_t)i + 3] = -1;
    }
    // colour k of palette p: `sum` of error over `count` pixels, the worst movable one at `pos` (-1: none)
    void set(int p, int k, int64_t sum, int64_t count, int64_t pos) {
        const size_t i = (size_t)p * K + k;
        err[4 * i] = sum, err[4 * i + 1] = count, err[4 * i + 2] = pos >= 0 ? 0x3f800000 : 0, err[4 * i + 3] = pos;
        if (pos >= 0) worst[4 * i] = (float)(100 * p + k), worst[4 * i + 1] = 0.5f, worst[4 * i + 2] = 0.25f;
    }
    int run(int max_moves, std::vector<int>* moved) {
        if (moved) moved->assign((size_t)P, -7);
        return hq_reseed_unused(err.data(), worst.data(), P, K, max_moves, pal.data(), moved ? moved->data() : nullptr);
    }
    int run_fixed(int max_moves, int nfixed, std::vector<int>* moved) {
        if (moved) moved->assign((size_t)P, -7);
        return hq_reseed_unused_fixed(err.data(), worst.data(), P, K, max_moves, nfixed, pal.data(),
                                      moved ? moved->data() : nullptr);
    }
    bool is_donor(int p, int k, int donor) const {  // colour k now holds donor's worst pixel
        const float* c = &pal[4 * ((size_t)p * K + k)];
        return c[0] == (float)(100 * p + donor) && c[1] == 0.5f && c[2] == 0.25f && c[3] == 0.0f;
    }
    bool untouched(int p, int k) const {
        const size_t i = 4 * ((size_t)p * K + k);
        return pal[i] == -1.0f - (float)i && pal[i + 1] == -2.0f - (float)i && pal[i + 2] == -3.0f - (float)i;
    }
};

}  // namespace

int main() {
    std::vector<int> moved;
    {  // the most error gives first, receivers ascending; the donors keep their colours
        Stats s(1, 5);
        s.set(0, 0, 10, 3, 7), s.set(0, 2, 50, 1, 9), s.set(0, 4, 30, 2, 0);
        CHECK(s.run(-1, &moved) == HQ_OK && moved[0] == 2);
        CHECK(s.is_donor(0, 1, 2) && s.is_donor(0, 3, 4));
        CHECK(s.untouched(0, 0) && s.untouched(0, 2) && s.untouched(0, 4));
    }
    {  // equal sums: the lower index gives first
        Stats s(1, 6);
        s.set(0, 1, 40, 1, 1), s.set(0, 3, 40, 1, 2), s.set(0, 5, 40, 1, 3);
        CHECK(s.run(-1, &moved) == HQ_OK && moved[0] == 3);
        CHECK(s.is_donor(0, 0, 1) && s.is_donor(0, 2, 3) && s.is_donor(0, 4, 5));
    }
    {  // more receivers than donors; a donor without a movable pixel is skipped
        Stats s(1, 6);
        s.set(0, 0, 99, 5, -1), s.set(0, 1, 5, 5, 4);
        CHECK(s.run(-1, &moved) == HQ_OK && moved[0] == 1);
        CHECK(s.is_donor(0, 2, 1) && s.untouched(0, 3) && s.untouched(0, 4) && s.untouched(0, 5));
    }
    {  // max_moves 0, 1 and more than there are receivers
        for (int mm : {0, 1, 9}) {
            Stats s(1, 4);
            s.set(0, 2, 8, 1, 1), s.set(0, 3, 9, 1, 2);
            CHECK(s.run(mm, &moved) == HQ_OK && moved[0] == (mm < 2 ? mm : 2));
            CHECK(mm == 0 ? s.untouched(0, 0) : s.is_donor(0, 0, 3));
            CHECK(mm == 9 ? s.is_donor(0, 1, 2) : s.untouched(0, 1));
        }
    }
    {  // no receiver, moved NULL, several palettes, K = 1
        Stats s(3, 1);
        s.set(0, 0, 1, 1, 0), s.set(2, 0, 1, 1, 0);
        CHECK(s.run(-1, nullptr) == HQ_OK);
        for (int p = 0; p < 3; ++p) CHECK(s.untouched(p, 0));  // (palette 1: a receiver and no donor)
    }
    {  // K = 300, every other colour unused, sums of 2^62
        Stats s(2, 300);
        for (int p = 0; p < 2; ++p)
            for (int k = 0; k < 300; k += 2) s.set(p, k, ((int64_t)1 << 62) + k, 1, k);
        CHECK(s.run(-1, &moved) == HQ_OK && moved[0] == 150 && moved[1] == 150);
        for (int p = 0; p < 2; ++p)
            for (int i = 0; i < 150; ++i) CHECK(s.is_donor(p, 2 * i + 1, 298 - 2 * i));
    }
    {  // refusals leave everything alone
        Stats s(1, 3);
        s.set(0, 0, 5, 1, 0), s.set(0, 2, -1, 1, 0);
        CHECK(s.run(-1, &moved) == HQ_ERR_ARG && moved[0] == -7 && s.untouched(0, 1));
        s.set(0, 2, 1, -1, 0);
        CHECK(s.run(-1, &moved) == HQ_ERR_ARG && s.untouched(0, 1));
        s.set(0, 2, 1, 1, 0);
        CHECK(hq_reseed_unused(s.err.data(), s.worst.data(), 0, 3, -1, s.pal.data(), nullptr) == HQ_ERR_ARG);
        CHECK(hq_reseed_unused(s.err.data(), s.worst.data(), 1, 0, -1, s.pal.data(), nullptr) == HQ_ERR_ARG);
        CHECK(hq_reseed_unused(nullptr, s.worst.data(), 1, 3, -1, s.pal.data(), nullptr) == HQ_ERR_ARG);
        CHECK(s.untouched(0, 1));
    }
    // ---- hq_reseed_unused_fixed: the first nfixed colours are never receivers ----
    {  // unused fixed colours stay, take no place in the receivers' order and consume no donor
        Stats s(1, 6);
        s.set(0, 2, 50, 1, 9), s.set(0, 4, 30, 2, 0);  // colours 0, 1 (fixed) and 3, 5 are unused
        CHECK(s.run_fixed(-1, 2, &moved) == HQ_OK && moved[0] == 2);
        CHECK(s.untouched(0, 0) && s.untouched(0, 1) && s.is_donor(0, 3, 2) && s.is_donor(0, 5, 4));
    }
    {  // a fixed colour gives like any other; max_moves counts free receivers only
        Stats s(1, 5);
        s.set(0, 0, 90, 4, 3), s.set(0, 3, 10, 1, 1);  // colour 0 (fixed) has the most error
        CHECK(s.run_fixed(1, 2, &moved) == HQ_OK && moved[0] == 1);
        CHECK(s.untouched(0, 0) && s.untouched(0, 1) && s.is_donor(0, 2, 0) && s.untouched(0, 4));
    }
    {  // more free receivers than donors, and the reverse; equal sums: the lower index first
        Stats s(2, 6);
        s.set(0, 1, 40, 1, 1);                                                  // palette 0: one donor
        s.set(1, 0, 40, 1, 1), s.set(1, 1, 40, 1, 2), s.set(1, 2, 40, 1, 3), s.set(1, 4, 40, 1, 5);  // palette 1: four
        CHECK(s.run_fixed(-1, 1, &moved) == HQ_OK && moved[0] == 1 && moved[1] == 2);
        CHECK(s.untouched(0, 0) && s.is_donor(0, 2, 1) && s.untouched(0, 3) && s.untouched(0, 4) && s.untouched(0, 5));
        CHECK(s.is_donor(1, 3, 0) && s.is_donor(1, 5, 1));
    }
    {  // nfixed = K: nothing moves; nfixed = 0: hq_reseed_unused itself
        Stats s(1, 4), a(1, 4), b(1, 4);
        s.set(0, 2, 8, 1, 1), a.set(0, 2, 8, 1, 1), b.set(0, 2, 8, 1, 1);
        CHECK(s.run_fixed(-1, 4, &moved) == HQ_OK && moved[0] == 0);
        for (int k = 0; k < 4; ++k) CHECK(s.untouched(0, k));
        std::vector<int> ma, mb;
        CHECK(a.run(-1, &ma) == HQ_OK && b.run_fixed(-1, 0, &mb) == HQ_OK && ma == mb);
        CHECK(std::memcmp(a.pal.data(), b.pal.data(), sizeof(float) * a.pal.size()) == 0);
    }
    {  // nfixed < 0 and nfixed > K: refused, everything left alone
        Stats s(1, 3);
        s.set(0, 0, 5, 1, 0);
        CHECK(s.run_fixed(-1, -1, &moved) == HQ_ERR_ARG && moved[0] == -7);
        CHECK(s.run_fixed(-1, 4, &moved) == HQ_ERR_ARG && moved[0] == -7);
        for (int k = 0; k < 3; ++k) CHECK(s.untouched(0, k));
    }
    if (failures) {
        std::fprintf(stderr, "reseed_check: %d failure(s)\n", failures);
        return EXIT_FAILURE;
    }
    std::puts("reseed_check ok");
    return EXIT_SUCCESS;
}
