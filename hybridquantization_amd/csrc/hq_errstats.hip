// hq_errstats.hip -- the distribution of the per-pixel S-CIELAB dE of an evaluated
// population (hq_error_stats): per palette a histogram of the error image the cost
// kernels stored (option "pixel_err"), the count of the pixels without a usable dE,
// and the worst pixel.  libhq's own addition: the reference reports the mean alone.
//
// Everything is integer.  A counted pixel of weight w (1 without a map, 1 under a
// mask, its byte under weights; a byte of 0 is not counted) with fp32 error e
//   - not finite or below zero: adds w to nonfinite, nothing else;
//   - else adds w to bin b = t >= nbins ? nbins - 1 : (int)t of t = RN(e scale), one
//     fp32 multiply by the host's scale = (float)nbins / top, and enters the maximum
//     of the 64-bit key (bits of e) << 32 | (2^32 - 1 - raster index): the largest
//     dE, then the lowest index.  (A finite e >= 0 has the sign bit clear -- that of
//     -0 is cleared -- so the bits order as the values do.  t is a NaN only as 0
//     times an infinite scale: the last bin.)
// Sums and maxima of integers do not depend on the order of the atomics: the tables
// are bitwise reproducible and compare exactly against numpy.
#include "hq_device.h"
#include "hq_errstats.h"
#include "hq_launch.h"

namespace hq {

namespace {

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned long long o = __shfl_xor(v, m, 64);
        v = o > v ? o : v;
    }
    return v;
}

}  // namespace

// ----------------------------------------------------------------------------
// errstats: grid (nspans, P), block 256.  A workgroup streams span blockIdx.x of
// palette blockIdx.y's error plane: `span` consecutive owned pixels (the owned rows
// lie W apart, back to back, so a span crosses rows freely).
//
// Loads.  A plane starts p pitch floats into the buffer and pitch = W rows is any
// residue mod 4, so 16-byte alignment is found from the span's own address: up to 3
// scalar head pixels (one lane each), then quads -- a thread 4 consecutive pixels
// per step, one 16-byte load, 256 quads per workgroup and step -- then up to 3
// scalar tail pixels.  The map's 4 bytes of a quad are one 32-bit load at whatever
// alignment the quad has in the map (MSK: 0 none, 1 mask, 2 weights), issued with
// the error load.
//
// Histogram.  One copy of 32-bit counters in LDS (ds_add_u32 without return),
// 16 KiB at 4096 bins; a span holds at most 2^24 pixels of weight at most 255, so no
// counter wraps.  Real error images pile up in a few low bins, and 64 lanes on one
// LDS word serialise (a copy per wave did not help: measured).  So
// equal bins meet before the atomic: a quad's neighbours with one bin add once, and
// a wave whose 256 pixels all have one bin sums their weights across its lanes and
// adds once (every lane runs every step: the wave sum needs them all).
//
// The maximum and the non-finite weight ride in two registers per lane, are
// reduced across the wave, then across the four waves through LDS.  One flush:
// the non-zero bins, the non-finite weight and the key go out as 64-bit integer
// global atomics (add, add, max).  No workgroup waits on another.
// ----------------------------------------------------------------------------
template <int MSK>
__global__ __launch_bounds__(256) void errstats_kernel(ErrStatsArgs a) {
    static_assert((uint64_t)kErrStatsMaxSpan * 255u < (1ull << 32), "a span's weight in a 32-bit counter");
    __shared__ uint32_t s_h[kErrStatsMaxBins];
    __shared__ unsigned long long s_key[4], s_bad[4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, p = blockIdx.y;
    const int nb = a.nbins;
    for (int b = tid; b < nb; b += 256) s_h[b] = 0u;
    __syncthreads();
    const float* const e = a.err + (int64_t)p * a.pitch;
    const uint32_t s0 = blockIdx.x * a.span;  // ((nspans - 1) span < n: no wrap)
    const uint32_t len = min(a.span, a.n - s0);
    const float fnb = (float)nb;
    uint32_t bad = 0u;
    unsigned long long key = 0ull;
    // owned pixel i with error v and map byte w -> the weight it adds to bin *b (0: to none)
    auto pixel = [&](float v, uint32_t w, uint32_t i, int* b) -> uint32_t {
        *b = 0;
        if (MSK != 0 && w == 0u) return 0u;
        if (MSK != 2) w = 1u;
        if (!(v >= 0.0f && v < __builtin_inff())) {
            bad += w;
            return 0u;
        }
        const float t = __fmul_rn(v, a.scale);
        *b = !(t < fnb) ? nb - 1 : (int)t;
        const unsigned long long k =
            ((unsigned long long)(__float_as_uint(v) & 0x7fffffffu) << 32) | (0xffffffffu - (a.pos0 + i));
        key = k > key ? k : key;
        return w;
    };
    auto scalar = [&](uint32_t i) {
        int b;
        const uint32_t w = pixel(e[i], MSK != 0 ? (uint32_t)a.mask[i] : 1u, i, &b);
        if (w) atomicAdd(s_h + b, w);
    };
    const uint32_t head = min((4u - ((uint32_t)(reinterpret_cast<uintptr_t>(e + s0) >> 2) & 3u)) & 3u, len);
    const uint32_t nq = (len - head) >> 2, b0 = s0 + head;
    const uint32_t tail = len - head - 4u * nq;
    for (uint32_t jb = 0u; jb < nq; jb += 256u) {
        const uint32_t j = jb + (uint32_t)tid;
        const uint32_t i = b0 + 4u * min(j, nq - 1u);  // (past the end: the last quad again, not counted)
        const float4 v = *reinterpret_cast<const float4*>(e + i);
        uint32_t mq = 0x01010101u;
        if constexpr (MSK != 0) __builtin_memcpy(&mq, a.mask + i, 4);
        int b[4] = {0, 0, 0, 0};
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        if (j < nq) {
            w[0] = pixel(v.x, mq & 0xffu, i, &b[0]);
            w[1] = pixel(v.y, (mq >> 8) & 0xffu, i + 1u, &b[1]);
            w[2] = pixel(v.z, (mq >> 16) & 0xffu, i + 2u, &b[2]);
            w[3] = pixel(v.w, mq >> 24, i + 3u, &b[3]);
        }
#pragma unroll
        for (int q = 1; q < 4; ++q)  // a neighbour with the same bin carries the weight on
            if (b[q] == b[q - 1]) {
                w[q] += w[q - 1];
                w[q - 1] = 0u;
            }
        // every lane's weight sits in w[3] and in one bin of the wave's: one add for the wave
        const int bu = __builtin_amdgcn_readfirstlane(b[3]);
        const bool one = (w[0] | w[1] | w[2]) == 0u && (w[3] == 0u || b[3] == bu);
        if (__builtin_amdgcn_ballot_w64(!one) == 0) {
            const uint32_t ws = wave_sum(w[3]);
            if (lane == 0 && ws) atomicAdd(s_h + bu, ws);
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (w[q]) atomicAdd(s_h + b[q], w[q]);
        }
    }
    if ((uint32_t)tid < head) scalar(s0 + (uint32_t)tid);
    if ((uint32_t)tid < tail) scalar(b0 + 4u * nq + (uint32_t)tid);

    const unsigned long long wbad = wave_sum_u64((unsigned long long)bad);
    key = wave_max_u64(key);
    if (lane == 0) {
        s_bad[wave] = wbad;
        s_key[wave] = key;
    }
    __syncthreads();
    if (tid == 0) {
        unsigned long long nbad = 0ull, kmax = 0ull;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            nbad += s_bad[w];
            kmax = s_key[w] > kmax ? s_key[w] : kmax;
        }
        if (nbad) atomicAdd(a.nonfinite + p, nbad);
        if (kmax) atomicMax(a.key + p, kmax);
    }
    for (int b = tid; b < nb; b += 256)
        if (s_h[b]) atomicAdd(a.hist + (int64_t)p * nb + b, (unsigned long long)s_h[b]);
}

hipError_t launch_error_stats(const ErrStatsArgs& a, hipStream_t s) {
    if (a.P < 1 || a.P > 65535 || a.n < 1u || a.nbins < 1 || a.nbins > kErrStatsMaxBins ||
        a.span < 1024u || a.span % 1024u || a.span > kErrStatsMaxSpan ||
        (uint64_t)a.nspans != ((uint64_t)a.n + a.span - 1u) / a.span)
        return hipErrorInvalidValue;
    with_mask(a.mask != nullptr, a.weighted != 0, [&](auto MSK) {
        HQ_LAUNCH((errstats_kernel<MSK.value>), dim3((unsigned)a.nspans, (unsigned)a.P), dim3(256), 0, s, a);
    });
    return hipGetLastError();
}

}  // namespace hq
