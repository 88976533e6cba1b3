// hq_errstats.h -- the dE distribution of an evaluated population (hq_error_stats, hq.h;
// DESIGN.md 33): the arguments and the launcher of hq_errstats.hip, for that unit and the
// evaluation (hq_eval.hip), and the span rule.  Not part of the public ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

namespace hq {

constexpr int kErrStatsMaxBins = 4096;             // the LDS histogram's counters: 16 KiB
constexpr uint32_t kErrStatsMaxSpan = 1u << 24;    // 2^24 pixels of weight 255: a 32-bit counter holds them
constexpr uint32_t kErrStatsMinSpan = 1u << 13;    // an automatic span: at least 8 steps of 256 quads
constexpr int kErrStatsBlocksPerCu = 8;            // ... and one resident round of workgroups over the P palettes

struct ErrStatsArgs {
    const float* err;        // [P][pitch] per-pixel dE of the owned rows (CostArgs::pix_err), rows W apart
    const uint8_t* mask;     // the map's byte of owned pixel 0 (ClusterArgs::mask + q0), else null
    unsigned long long* hist;       // [P][nbins]
    unsigned long long* nonfinite;  // [P]
    unsigned long long* key;        // [P] max of (bits of e) << 32 | (2^32 - 1 - pixel), 0: no finite pixel
    int64_t pitch;           // floats from one palette's plane to the next: the owned pixels, any residue mod 4
    uint32_t n;              // owned pixels
    uint32_t pos0;           // owned pixel 0's raster index in the full image
    uint32_t span;           // pixels per workgroup: a multiple of 1024, at most kErrStatsMaxSpan
    int nspans;              // ceil(n / span)
    int P, nbins;
    float scale;             // (float)nbins / top
    int weighted;            // the map's bytes are weights (else 0 / 1)
};

// span and nspans of n owned pixels: `span` pixels per workgroup asked for (test option
// "errstats_span"; 0: by the grid), rounded up to 1024 and clamped to kErrStatsMaxSpan
inline void errstats_spans(uint32_t n, int P, uint32_t span, int num_cu, uint32_t* out_span, int* nspans) {
    uint64_t s = span;
    if (!s) {
        const uint64_t want = (uint64_t)(num_cu * kErrStatsBlocksPerCu / P > 1 ? num_cu * kErrStatsBlocksPerCu / P : 1);
        s = (n + want - 1) / want;
        if (s < kErrStatsMinSpan) s = kErrStatsMinSpan;
    }
    s = (s + 1023u) / 1024u * 1024u;
    if (s > kErrStatsMaxSpan) s = kErrStatsMaxSpan;
    *out_span = (uint32_t)s;
    *nspans = (int)(((uint64_t)n + s - 1) / s);
}

// One launch for the whole population: grid (nspans, P), the three tables zero on entry.
hipError_t launch_error_stats(const ErrStatsArgs&, hipStream_t);

}  // namespace hq
