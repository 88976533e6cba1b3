// descend_check.cpp -- the descent step's rule (hq::descend_step, hq_host.cpp) and the gradient's
// host half (grad_bound, grad_shift, grad_chain: hq_grad.h) on their edge cases as a stand-alone
// host program, built and run under the address and undefined-behaviour sanitizers by
// `make descend_check` (no GPU code, no Python).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "hq_grad.h"

namespace {

int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

bool same_bits(const float* a, const float* b, int n) { return std::memcmp(a, b, sizeof(float) * n) == 0; }

void step_rule() {
    const int K = 5;
    const double N = 1000.0;
    // colour 0 fixed; 1 moves; 2 has no pixels; 3 clamps at both ends; 4 has a gradient that is not finite
    const float pal[4 * K] = {.5f, .5f, .5f, 0.f, .4f, .6f, .2f, 0.f, .1f, .2f, .3f, 0.f, .01f, .99f, .5f, 0.f,
                              .7f, .7f, .7f, 0.f};
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double grad[4 * K] = {1., 1., 1., 100., .02, -.04, 0., 200., 5., 5., 5., 0., 10., -10., 0., 50.,
                                nan, inf, -.01, 100.};
    float cand[4 * K];
    CHECK(hq::descend_step(pal, grad, K, 1, N, 0.5, cand));
    CHECK(same_bits(cand, pal, 4));           // fixed
    CHECK(same_bits(cand + 8, pal + 8, 4));   // no pixels
    // colour 1: pal - rate grad N / n = .4 - .5 .02 5, .6 + .5 .04 5, .2
    CHECK(cand[4] == (float)((double).4f - 0.5 * .02 * N / 200.) && cand[5] == (float)((double).6f + 0.5 * .04 * N / 200.));
    CHECK(cand[6] == pal[6] && cand[7] == 0.f);
    CHECK(cand[12] == 0.f && cand[13] == 1.f && cand[14] == pal[14]);  // clamped
    CHECK(cand[16] == pal[16] && cand[17] == pal[17]);                 // NaN, inf: the bits stay
    CHECK(cand[18] == (float)((double).7f + 0.5 * .01 * N / 100.));
    // nothing to move: every colour fixed, or every gradient zero
    CHECK(!hq::descend_step(pal, grad, K, K, N, 0.5, cand) && same_bits(cand, pal, 4 * K));
    const std::vector<double> zero(4 * K, 0.0);
    CHECK(!hq::descend_step(pal, zero.data(), K, 0, N, 0.5, cand) && same_bits(cand, pal, 4 * K));
    // a colour already at the bound it is pushed against does not count as changed
    const float edge[4] = {0.f, 1.f, 0.f, 0.f};
    const double push[4] = {1., -1., 0., 10.};
    CHECK(!hq::descend_step(edge, push, 1, 0, N, 1.0, cand) && same_bits(cand, edge, 4));
    CHECK(hq::descend_step(edge, push, 1, -3, N, -1.0, cand) && cand[0] == 1.f && cand[1] == 0.f);  // (nfixed < 0: none)
}

void shift_and_chain() {
    CHECK(hq::grad_shift(1.0) == 30 && hq::grad_shift(3.9) == 30 && hq::grad_shift(4.0) == 29);
    CHECK(hq::grad_shift(262143.0) == 14 && hq::grad_shift(262144.0) == 13 && hq::grad_shift(0x1p40) == -9);
    CHECK(hq::grad_shift(0.0) == hq::kGradNoShift && hq::grad_shift(-1.0) == hq::kGradNoShift);
    CHECK(hq::grad_shift(std::numeric_limits<double>::quiet_NaN()) == hq::kGradNoShift);
    CHECK(hq::grad_shift(std::numeric_limits<double>::infinity()) == hq::kGradNoShift);
    // 2^30 pixels at the bound stay below 2^62 in magnitude
    for (double b : {1.0, 7.5, 1000.0, 262143.9, 1e9})
        CHECK(std::ldexp(b, hq::grad_shift(b)) * 0x1p30 <= 0x1p62);
    // the bound: one tap of 1, the identity matrix: (kappa / 116) 816 9 (1 + 1 [+ 1])
    const float m[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, k[4] = {1, 1, 1, 0}, k3[1] = {-1}, a3[1] = {1};
    const double fmax = 24389.0 / 27.0 / 116.0;
    CHECK(std::fabs(hq::grad_bound(m, k, k, k3, a3, 1) - fmax * 816.0 * 18.0) < 1e-9);
    const float m0[9] = {1, 0, 0, 0, 0, 0, 0, 0, 0};
    CHECK(std::fabs(hq::grad_bound(m0, k, k, k3, a3, 1) - fmax * 500.0 * 27.0) < 1e-9);
    // the chain rule: one sum on each opponent channel in turn, both srgb_lin branches, a colour without pixels
    const double r2o[9] = {1, 2, 3, 4, 5, 6, 7, 8, 9};
    const int64_t sums[12] = {1 << 10, 0, 0, 4, 0, 1 << 10, -(1 << 10), 2, 99, 99, 99, 0};
    const float pal[12] = {0.f, 0.04045f, 1.f, 0.f, .5f, .5f, .5f, 0.f, .5f, .5f, .5f, 0.f};
    double g[12];
    hq::grad_chain(sums, pal, 3, 8.0, 10, r2o, g);
    const double lo = 1.0 / (double)12.92f;
    CHECK(g[0] == 1.0 * lo / 8.0 && g[1] == 2.0 * lo / 8.0 && g[3] == 4.0);
    CHECK(std::fabs(g[2] - 3.0 * hq::srgb_lin_slope(1.0) / 8.0) < 1e-15 && hq::srgb_lin_slope(1.0) > 2.2);
    CHECK(std::fabs(g[4] - (4.0 - 7.0) * hq::srgb_lin_slope(.5) / 8.0) < 1e-15 && g[7] == 2.0);
    CHECK(g[8] == 0.0 && g[9] == 0.0 && g[10] == 0.0 && g[11] == 0.0);
}

}  // namespace

int main() {
    step_rule();
    shift_and_chain();
    if (failures) {
        std::fprintf(stderr, "descend_check: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("descend_check ok\n");
    return 0;
}
