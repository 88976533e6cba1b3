// illum_check.cpp -- stand-alone check of the illuminant argument rule (bad_illum_component)
// and of the Opp->Lab matrix built from an accepted illuminant (opp2xyz_over_illum), both in
// hq_cost_taps.cpp.  Host code only: built with the sanitizers and run on the CPU (make
// illum_check).
#include "hq_cost_layout.h"

#include <cmath>
#include <cstdio>
#include <limits>

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

int main() {
    using hq::bad_illum_component;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    // accepted: the two white points, illuminant A, Yn != 1, the smallest and largest floats
    const float good[][3] = {{0.95047f, 1.0f, 1.0883f}, {0.966797f, 1.0f, 0.825188f}, {1.0985f, 1.0f, 0.35585f},
                             {0.760376f, 0.8f, 0.87064f}, {1.2084963f, 1.25f, 1.031485f},
                             {std::numeric_limits<float>::denorm_min(), std::numeric_limits<float>::min(),
                              std::numeric_limits<float>::max()}};
    for (const auto& g : good) CHECK(bad_illum_component(g) == -1);
    // refused, in each component: NaN, +inf, -inf, 0.0, -0.0, a negative value
    const float bad[] = {nan, inf, -inf, 0.0f, -0.0f, -1.0f, -std::numeric_limits<float>::denorm_min()};
    for (int i = 0; i < 3; ++i)
        for (const float v : bad) {
            float il[3] = {0.95047f, 1.0f, 1.0883f};
            il[i] = v;
            CHECK(bad_illum_component(il) == i);
        }
    {  // the first bad component is the one named
        const float il[3] = {1.0f, nan, 0.0f};
        CHECK(bad_illum_component(il) == 1);
    }
    // the matrix of an accepted illuminant: finite, row r = Opp->XYZ row r / illum[r] to 1 ulp,
    // and the Y row scaled by Yn != 1 (not only rows 0 and 2)
    static const float opp2xyz[9] = HQ_OPP2XYZ;
    for (const auto& g : good) {
        if (g[0] < 1e-30f) continue;  // (1 / denorm_min overflows: accepted by the rule, not a colour)
        const float inv[3] = {1.0f / g[0], 1.0f / g[1], 1.0f / g[2]};
        float m[9];
        hq::opp2xyz_over_illum(inv, m);
        for (int i = 0; i < 9; ++i) {
            const double want = (double)opp2xyz[i] / (double)g[i / 3];
            CHECK(std::isfinite(m[i]));
            CHECK(std::fabs((double)m[i] - want) <= 2.4e-7 * std::fabs(want));
        }
    }
    {
        const float a[3] = {1.0f, 1.0f, 1.0f}, b[3] = {1.0f, 1.25f, 1.0f};
        float ma[9], mb[9];
        hq::opp2xyz_over_illum(a, ma);
        hq::opp2xyz_over_illum(b, mb);
        for (int i = 0; i < 9; ++i) CHECK(i / 3 == 1 ? mb[i] == 1.25f * ma[i] : mb[i] == ma[i]);
    }
    if (failures) {
        std::printf("illum_check: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("illum_check: ok\n");
    return 0;
}
