// diffuse_check.cpp -- hq_diffuse_taps.cpp (the presets, the legality rule and the (R, S)
// classification of hq_diffuse_population's tap sets) against a brute-force statement of
// hq.h's rules, on their edge cases.  Stand-alone, built with the address and
// undefined-behaviour sanitizers (make diffuse_check).
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>

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

// hq.h's legality rule, each condition on its own.
bool legal_ref(const hq_diffusion_taps& t) {
    bool any = false;
    long double sum = 0;
    for (int dy = 0; dy < 3; ++dy)
        for (int dx = -2; dx <= 2; ++dx) {
            const int32_t w = t.w[dy][dx + 2];
            if (w < 0) return false;
            if (dy == 0 && dx < 1 && w != 0) return false;
            any = any || w != 0;
            sum += w;
        }
    return t.div >= 1 && any && sum <= (long double)t.div;
}

// R: the highest dy with a weight (at least 1); S = max(a, 1) + 1, a the largest -dx in row 1.
void classify_ref(const hq_diffusion_taps& t, int* R, int* S) {
    *R = 1;
    int a = 0;
    for (int dx = -2; dx <= 2; ++dx) {
        if (t.w[2][dx + 2]) *R = 2;
        if (t.w[1][dx + 2] && -dx > a) a = -dx;
    }
    *S = (a > 1 ? a : 1) + 1;
}

void check_one(const hq_diffusion_taps& t) {
    const bool want = legal_ref(t);
    CHECK(hq_diffusion_taps_legal(&t) == (want ? 1 : 0));
    int R = -1, S = -1;
    const int rc = hq_diffusion_classify(&t, &R, &S);
    if (!want) {
        CHECK(rc == HQ_ERR_ARG && R == -1 && S == -1);
        return;
    }
    int wantR, wantS;
    classify_ref(t, &wantR, &wantS);
    CHECK(rc == HQ_OK && R == wantR && S == wantS);
}

hq_diffusion_taps zero_taps(int32_t div) {
    hq_diffusion_taps t;
    std::memset(&t, 0, sizeof t);
    t.div = div;
    return t;
}

}  // namespace

int main() {
    // the presets: the table of hq.h, their sums and their instances
    static const struct { int which, sum, div, R, S; } kWant[HQ_DIFFUSION_COUNT] = {
        {HQ_DIFFUSION_FLOYD_STEINBERG, 16, 16, 1, 2}, {HQ_DIFFUSION_JARVIS, 48, 48, 2, 3},
        {HQ_DIFFUSION_STUCKI, 42, 42, 2, 3},          {HQ_DIFFUSION_BURKES, 32, 32, 1, 3},
        {HQ_DIFFUSION_SIERRA3, 32, 32, 2, 3},         {HQ_DIFFUSION_SIERRA2, 16, 16, 1, 3},
        {HQ_DIFFUSION_SIERRA_LITE, 4, 4, 1, 2},       {HQ_DIFFUSION_ATKINSON, 6, 8, 2, 2},
    };
    for (const auto& w : kWant) {
        hq_diffusion_taps t = zero_taps(-1);
        CHECK(hq_diffusion_preset(w.which, &t) == HQ_OK);
        int sum = 0;
        for (int dy = 0; dy < 3; ++dy)
            for (int i = 0; i < 5; ++i) sum += t.w[dy][i];
        int R = 0, S = 0;
        CHECK(sum == w.sum && t.div == w.div);
        CHECK(hq_diffusion_classify(&t, &R, &S) == HQ_OK && R == w.R && S == w.S);
        check_one(t);
    }
    hq_diffusion_taps t = zero_taps(1);
    CHECK(hq_diffusion_preset(-1, &t) == HQ_ERR_ARG && hq_diffusion_preset(HQ_DIFFUSION_COUNT, &t) == HQ_ERR_ARG);
    CHECK(hq_diffusion_preset(0, nullptr) == HQ_ERR_ARG);
    CHECK(hq_diffusion_taps_legal(nullptr) == 0);
    int R = 0, S = 0;
    CHECK(hq_diffusion_classify(nullptr, &R, &S) == HQ_ERR_ARG);
    hq_diffusion_preset(HQ_DIFFUSION_JARVIS, &t);
    CHECK(hq_diffusion_classify(&t, nullptr, &S) == HQ_ERR_ARG && hq_diffusion_classify(&t, &R, nullptr) == HQ_ERR_ARG);

    // no weight at all; every single position, legal or not, at weight 1 and at a negative one
    check_one(zero_taps(1));
    for (int dy = 0; dy < 3; ++dy)
        for (int i = 0; i < 5; ++i)
            for (int32_t w : {1, -1, INT_MAX, INT_MIN}) {
                for (int32_t div : {0, 1, -1, INT_MAX, INT_MIN}) {
                    t = zero_taps(div);
                    t.w[dy][i] = w;
                    check_one(t);
                }
            }
    // the sum against div: equal, one above, and twelve weights whose sum passes int32
    hq_diffusion_preset(HQ_DIFFUSION_STUCKI, &t);
    t.div = 41;
    check_one(t);
    CHECK(!hq_diffusion_taps_legal(&t));
    t.div = 43;
    check_one(t);
    CHECK(hq_diffusion_taps_legal(&t));
    t = zero_taps(INT_MAX);
    t.w[0][3] = t.w[0][4] = INT_MAX;
    for (int dy = 1; dy < 3; ++dy)
        for (int i = 0; i < 5; ++i) t.w[dy][i] = INT_MAX;
    check_one(t);
    CHECK(!hq_diffusion_taps_legal(&t));
    // every pattern of present / absent over the twelve legal positions: all four instances
    int seen[3][4] = {};
    for (int bits = 1; bits < 1 << 12; ++bits) {
        t = zero_taps(12);
        for (int b = 0; b < 12; ++b)
            if (bits >> b & 1) (b < 2 ? t.w[0][3 + b] : t.w[1 + (b - 2) / 5][(b - 2) % 5]) = 1;
        check_one(t);
        if (hq_diffusion_classify(&t, &R, &S) == HQ_OK) seen[R][S] = 1;
    }
    CHECK(seen[1][2] && seen[1][3] && seen[2][2] && seen[2][3]);
    if (g_failed) {
        std::printf("diffuse_check: %d failed\n", g_failed);
        return 1;
    }
    std::printf("diffuse_check ok\n");
    return 0;
}
