// hq_diffuse_taps.cpp -- the diffusion kernels of hq_diffuse_population (hq.h): the presets,
// the legality rule and the (R, S) classification that picks the kernel instance
// (hq_diffuse.hip).  Host code only; links alone into a CPU program (diffuse_check.cpp).
#include <cstdint>
#include <cstring>

#include "../../include/hq.h"

namespace {

// hq.h's table: rows dy = 0 .. 2, columns dx = -2 .. 2.
constexpr hq_diffusion_taps kPresets[HQ_DIFFUSION_COUNT] = {
    {{{0, 0, 0, 7, 0}, {0, 3, 5, 1, 0}, {0, 0, 0, 0, 0}}, 16},  // Floyd-Steinberg
    {{{0, 0, 0, 7, 5}, {3, 5, 7, 5, 3}, {1, 3, 5, 3, 1}}, 48},  // Jarvis-Judice-Ninke
    {{{0, 0, 0, 8, 4}, {2, 4, 8, 4, 2}, {1, 2, 4, 2, 1}}, 42},  // Stucki
    {{{0, 0, 0, 8, 4}, {2, 4, 8, 4, 2}, {0, 0, 0, 0, 0}}, 32},  // Burkes
    {{{0, 0, 0, 5, 3}, {2, 4, 5, 4, 2}, {0, 2, 3, 2, 0}}, 32},  // Sierra (three rows)
    {{{0, 0, 0, 4, 3}, {1, 2, 3, 2, 1}, {0, 0, 0, 0, 0}}, 16},  // Sierra two-row
    {{{0, 0, 0, 2, 0}, {0, 1, 1, 0, 0}, {0, 0, 0, 0, 0}}, 4},   // Sierra Lite
    {{{0, 0, 0, 1, 1}, {0, 1, 1, 1, 0}, {0, 0, 1, 0, 0}}, 8},   // Atkinson
};

}  // namespace

extern "C" {

int hq_diffusion_preset(int which, hq_diffusion_taps* taps) {
    if (!taps || which < 0 || which >= HQ_DIFFUSION_COUNT) return HQ_ERR_ARG;
    *taps = kPresets[which];
    return HQ_OK;
}

int hq_diffusion_taps_legal(const hq_diffusion_taps* t) {
    if (!t || t->div < 1) return 0;
    int64_t sum = 0;
    for (int dy = 0; dy < 3; ++dy)
        for (int i = 0; i < 5; ++i) {
            const int32_t w = t->w[dy][i];
            if (w < 0 || (dy == 0 && i < 3 && w != 0)) return 0;
            sum += w;  // (twelve int32 at most: no overflow in 64 bits)
        }
    return sum >= 1 && sum <= t->div;
}

int hq_diffusion_classify(const hq_diffusion_taps* t, int* rows, int* slope) {
    if (!rows || !slope || !hq_diffusion_taps_legal(t)) return HQ_ERR_ARG;
    int R = 1;
    for (int i = 0; i < 5; ++i)
        if (t->w[2][i]) R = 2;
    const int a = t->w[1][0] ? 2 : 1;  // (dx = -1 or nothing right of the pixel: the slope is 2 either way)
    *rows = R;
    *slope = a + 1;
    return HQ_OK;
}

}  // extern "C"
