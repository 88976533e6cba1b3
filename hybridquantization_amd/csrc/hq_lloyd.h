// hq_lloyd.h -- the arithmetic of the k-means update, one function for the host
// rule (hq_centroids_from_sums, hq_host.cpp) and the device kernel
// (lloyd_update_kernel, hq_search.hip), so the two give the same bits.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define HQ_HOST_DEVICE __host__ __device__
#else
#define HQ_HOST_DEVICE
#endif

namespace hq {

// The mean of `count` > 0 pixels whose channel values add up to `sum` in units
// of 1/255 (bytes) or 2^-32: int64 -> double conversions, one fp64 product and
// one fp64 division (sum 2^-32 is exact), one rounding to float -- each
// correctly rounded on the host and on the device, and nothing to contract.
HQ_HOST_DEVICE inline float lloyd_mean(int64_t sum, int64_t count, bool bytes) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double s = (double)sum, n = (double)count;
    return bytes ? (float)(s / (255.0 * n)) : (float)(s * 0x1p-32 / n);
}

}  // namespace hq
