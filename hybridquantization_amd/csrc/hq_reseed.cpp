// hq_reseed.cpp -- hq_reseed_unused[_fixed]: the repair move's host rule (libhq's
// own addition, no reference counterpart).  Every unused colour of a palette moves
// onto the worst movable pixel of a cluster that carries much error, from the
// per-colour statistics of hq_cluster_errors; the first nfixed colours of a
// palette (hq_set_fixed_colors) never move.  Plain C++, integer arithmetic, no
// device code: it links alone into a CPU program (reseed_check.cpp).
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/hq.h"

extern "C" int hq_reseed_unused_fixed(const int64_t* err, const float* worst_rgb, int P, int K, int max_moves,
                                      int nfixed, float* palettes, int* moved) {
    if (!err || !worst_rgb || !palettes || P < 1 || K < 1 || nfixed < 0 || nfixed > K) return HQ_ERR_ARG;
    const size_t n = (size_t)P * K;
    for (size_t i = 0; i < n; ++i)  // (before anything is written: a refusal leaves the palettes alone)
        if (err[4 * i] < 0 || err[4 * i + 1] < 0) return HQ_ERR_ARG;
    std::vector<int> donors;
    donors.reserve((size_t)K);
    for (int p = 0; p < P; ++p) {
        const int64_t* e = err + (size_t)p * K * 4;
        donors.clear();
        for (int k = 0; k < K; ++k)
            if (e[4 * k + 1] > 0 && e[4 * k + 3] >= 0) donors.push_back(k);
        // the most error first, the lower index on a tie (the indices are distinct: a strict order)
        std::sort(donors.begin(), donors.end(), [e](int a, int b) {
            return e[4 * a] != e[4 * b] ? e[4 * a] > e[4 * b] : a < b;
        });
        size_t i = 0;
        // (a fixed colour is a donor like any other and never a receiver)
        for (int k = nfixed; k < K && i < donors.size() && (max_moves < 0 || i < (size_t)max_moves); ++k) {
            if (e[4 * k + 1] != 0) continue;
            const float* w = worst_rgb + ((size_t)p * K + donors[i]) * 4;
            float* c = palettes + ((size_t)p * K + k) * 4;
            c[0] = w[0], c[1] = w[1], c[2] = w[2], c[3] = 0.0f;
            ++i;
        }
        if (moved) moved[p] = (int)i;
    }
    return HQ_OK;
}

extern "C" int hq_reseed_unused(const int64_t* err, const float* worst_rgb, int P, int K, int max_moves,
                                float* palettes, int* moved) {
    return hq_reseed_unused_fixed(err, worst_rgb, P, K, max_moves, 0, palettes, moved);
}
