// hq_reduce.cpp -- hq_reduced_size and hq_reduce_weights: the host side of the
// coarse-to-fine search's image pyramid (libhq's own addition, no reference
// counterpart).  The geometry of a box reduction by an integer factor, and the
// reduction of a mask or weight map to the weight map of the reduced image.  Plain
// C++, integer arithmetic, no device code: it links alone into a CPU program
// (reduce_check.cpp).  The image itself is reduced on the device: hq_reduce.hip.
#include <algorithm>
#include <cstdint>

#include "../../include/hq.h"

extern "C" int hq_reduced_size(int w, int h, int factor, int* rw, int* rh) {
    if (w < 1 || h < 1 || factor < 1 || factor > 16 || !rw || !rh) return HQ_ERR_ARG;
    *rw = (int)(((int64_t)w + factor - 1) / factor);
    *rh = (int)(((int64_t)h + factor - 1) / factor);
    return HQ_OK;
}

extern "C" int hq_reduce_weights(const uint8_t* src, int w, int h, int factor, int is_mask, uint8_t* out) {
    int rw = 0, rh = 0;
    if (!src || !out || hq_reduced_size(w, h, factor, &rw, &rh)) return HQ_ERR_ARG;
    const int f = factor;
    for (int Y = 0; Y < rh; ++Y) {
        const int y1 = std::min(Y * f + f, h);
        for (int X = 0; X < rw; ++X) {
            const int x1 = std::min(X * f + f, w);
            // at most 16 x 16 bytes of at most 255: the sum stays below 2^16
            uint32_t sum = 0, n = 0;
            bool any = false;
            for (int y = Y * f; y < y1; ++y)
                for (int x = X * f; x < x1; ++x) {
                    const uint8_t b = src[(size_t)y * w + x];
                    any |= b != 0;
                    sum += is_mask ? (b ? 255u : 0u) : b;
                    ++n;
                }
            // round half up; a block that held a counted pixel is never lost
            const uint32_t v = (2 * sum + n) / (2 * n);
            out[(size_t)Y * rw + X] = (uint8_t)(any && v == 0 ? 1u : v);
        }
    }
    return HQ_OK;
}
