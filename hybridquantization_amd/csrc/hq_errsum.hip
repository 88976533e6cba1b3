// hq_errsum.hip -- per-colour S-CIELAB error of an evaluated population: for
// every palette p and colour k the sum of the per-pixel dE of the pixels
// assigned to k, their count, and the cluster's worst movable pixel -- where a
// repair move (hq_reseed_unused) puts an unused colour.  libhq's own addition:
// the reference has no such move.
//
// Everything is integer: a pixel adds v = RN(e 2^20) of its fp32 dE e (exact
// scaling, ties to even), the count adds 1, and the worst pixel is the maximum
// of the 64-bit key (bits of e) << 32 | (2^32 - 1 - position) over the movable
// pixels -- the largest dE, then the lowest position.  Sums and maxima of
// integers do not depend on the order of the atomics, so the results are
// bitwise reproducible and compare exactly against numpy.
#include "hq_device.h"
#include "hq_launch.h"

namespace hq {

namespace {

__device__ __forceinline__ unsigned long long err_wave_max(unsigned long long v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned long long o = __shfl_xor(v, m, 64);
        v = o > v ? o : v;
    }
    return v;
}

}  // namespace

// ----------------------------------------------------------------------------
// cluster_err: grid (nblocks * ceil(P/4)), block 256, XCD-relabelled --
// centroid_kernel's decomposition (hq_centroid.hip): a workgroup takes one span
// of the owned pixels and one group of up to 4 palettes, a thread 4 consecutive
// pixels per step, loaded once for the group, with the group's 4 indices and 4
// errors of each.
//
// K <= kCentLdsK (u8 indices): the group's colours and the accumulators live in
// LDS, [4][256] each: a 64-bit sum (ds_add_u64), a 32-bit count (ds_add_u32; a
// span holds at most 2^22 pixels) and a 64-bit key (ds_max_u64).  One flush at
// the end: the entries with a count go out as 64-bit integer global atomics
// (add, add, max).  A sum stays below 2^22 2^40 = 2^62 per workgroup.  The
// movable test and the max run only for a pixel whose dE reaches the largest its
// cluster has in LDS so far -- a 32-bit read of the key's high word, which only
// grows -- so a typical pixel costs two LDS atomics and that read.
// K > kCentLdsK (u16 and u32 indices): the same three atomics straight to
// global memory, the colour read from the prepared palette.
// A wave whose 256 pixels all have one colour in a palette (flat regions: 64
// lanes on one LDS word) reduces them across its lanes first -- sum and count
// in one word, the count above bit 52 (256 pixels of v < 2^40: below 2^48) --
// and adds once.
//
// A pixel whose dE is not a finite number in [0, 2^20) -- as bits: not below
// those of 2^20, which the sign bit, every infinity and every NaN are -- is
// counted but left out of the sum and of the worst pixel, and sets a.bad.
// ----------------------------------------------------------------------------
template <typename IDX_T, bool U8>
__global__ __launch_bounds__(256) void cluster_err_kernel(ClusterErrArgs a, int ngroups) {
    constexpr bool LDS = sizeof(IDX_T) == 1;
    constexpr int NL = LDS ? 4 * kMaxK : 1;
    static_assert(kCentLdsK == kMaxK && kMaxK == 256, "a u8 index addresses the whole LDS table");
    static_assert(cent_max_span(true) <= (1u << 22) && cent_max_span(false) <= (1u << 22),
                  "a span's count in 32 bits, its sum of v < 2^40 in 64");
    __shared__ unsigned long long s_sum[NL], s_key[NL];
    __shared__ uint32_t s_cnt[NL];
    __shared__ float4 s_pal[NL];
    const int w = xcd_remap(blockIdx.x, a.nblocks * ngroups);
    const int blk = w / ngroups, grp = w % ngroups, tid = threadIdx.x;
    const int p0 = 4 * grp, ng = min(4, a.P - p0);
    if constexpr (LDS) {
        for (int e = tid; e < NL; e += 256) {
            const int pp = e >> 8, k = e & (kMaxK - 1);
            s_sum[e] = 0ull;
            s_key[e] = 0ull;
            s_cnt[e] = 0u;
            s_pal[e] = pp < ng && k < a.K ? a.pal[(int64_t)(p0 + pp) * a.pal_pitch + k] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        __syncthreads();
    }
    // sum v and count n of colour k of the group's palette pp, and the key (0: no movable pixel)
    auto add = [&](int pp, uint32_t k, unsigned long long v, unsigned long long n, unsigned long long key) {
        if constexpr (LDS) {  // (k <= 255: inside the tables whatever the byte)
            const int e = pp * kMaxK + (int)k;
            if (v) atomicAdd(s_sum + e, v);
            atomicAdd(s_cnt + e, (uint32_t)n);
            if (key) atomicMax(s_key + e, key);
        } else if (k < (uint32_t)a.K) {
            unsigned long long* e = a.stats + ((int64_t)(p0 + pp) * a.K + k) * 4;
            if (v) atomicAdd(e, v);
            atomicAdd(e + 1, n);
            if (key) atomicMax(e + 2, key);
        }
    };
    // Quads of 4 pixels at multiples of 4 of the extended rows' positions, as in
    // centroid_kernel: [qa, qa + 4 nq) covers [q0, q1), the pixels outside it are
    // loaded (the buffers are padded to whole quads) but not counted.
    const uint32_t qa = a.q0 & ~3u;
    const uint32_t nq = (((a.q1 + 3u) & ~3u) - qa) >> 2;
    const uint32_t j0 = (uint32_t)blk * a.qspan, j1 = min(j0 + a.qspan, nq);
    const IDX_T* idx = static_cast<const IDX_T*>(a.idx);
    const int lane = tid & 63;
    // (uniform) every palette's error image starts a multiple of 4 floats from the quads' origin
    const bool quads = ((a.q0 | (uint32_t)a.err_pitch) & 3u) == 0u;
    bool bad = false;
    // (every lane of the workgroup runs every step: the wave reductions need them all)
    for (uint32_t jb = j0; jb < j1; jb += 256u) {
        const uint32_t j = jb + (uint32_t)tid;
        const bool in = j < j1;
        const uint32_t q = qa + 4u * min(j, nq - 1u);
        uint4 kq[4];
#pragma unroll
        for (int pp = 0; pp < 4; ++pp) kq[pp] = load_idx4(idx + (int64_t)(p0 + min(pp, ng - 1)) * a.idx_pitch + q);
        float pr[4], pg[4], pb[4];  // the pixels as the argmin saw them
        bool own[4];
        if constexpr (U8) {
            const uint4 px = *reinterpret_cast<const uint4*>(a.rgbx + q);
            const uint32_t v[4] = {px.x, px.y, px.z, px.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                pr[i] = u8_unit(v[i], 0);
                pg[i] = u8_unit(v[i], 1);
                pb[i] = u8_unit(v[i], 2);
            }
        } else {
            const float4 fr = *reinterpret_cast<const float4*>(a.R + q);
            const float4 fg = *reinterpret_cast<const float4*>(a.G + q);
            const float4 fb = *reinterpret_cast<const float4*>(a.B + q);
            pr[0] = fr.x, pr[1] = fr.y, pr[2] = fr.z, pr[3] = fr.w;
            pg[0] = fg.x, pg[1] = fg.y, pg[2] = fg.z, pg[3] = fg.w;
            pb[0] = fb.x, pb[1] = fb.y, pb[2] = fb.z, pb[3] = fb.w;
        }
        uint32_t eo[4];  // the pixel's place in an error image (the owned rows), clamped into it
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            own[i] = in && q + i >= a.q0 && q + i < a.q1;
            eo[i] = min(max(q + i, a.q0), a.q1 - 1u) - a.q0;
        }
#pragma unroll
        for (int pp = 0; pp < 4; ++pp) {
            if (pp >= ng) break;
            const uint32_t k[4] = {kq[pp].x, kq[pp].y, kq[pp].z, kq[pp].w};
            const float* perr = a.pix_err + (int64_t)(p0 + pp) * a.err_pitch;
            unsigned long long v[4], key[4];
            // the quad's 4 errors: one 16-B load where the error images' quads are aligned like
            // the pixels' and the quad lies inside the owned rows, else 4 loads at clamped places
            float ev[4];
            if (quads && q >= a.q0 && q + 4u <= a.q1) {
                const float4 t = *reinterpret_cast<const float4*>(perr + (q - a.q0));
                ev[0] = t.x, ev[1] = t.y, ev[2] = t.z, ev[3] = t.w;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) ev[i] = perr[eo[i]];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float e = ev[i];
                const uint32_t bits = __float_as_uint(e);
                const bool good = own[i] && bits < 0x49800000u;  // 0 <= e < 2^20
                bad |= own[i] && !good;
                v[i] = good ? (unsigned long long)rintf(e * 1048576.0f) : 0ull;
                float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
                bool contend = good;
                if constexpr (LDS) {
                    // Only a pixel whose dE reaches the cluster's largest so far can be its worst:
                    // the high word of the key in LDS only grows, so a read that is behind the
                    // atomics lets through more, never less.  Most pixels end here, without the
                    // colour's 16 B and without the 64-bit max.
                    const int e_k = pp * kMaxK + (int)k[i];
                    contend = good && bits >= reinterpret_cast<const volatile uint32_t*>(s_key)[2 * e_k + 1];
                    if (contend) c = s_pal[e_k];
                } else if (k[i] < (uint32_t)a.K) {
                    c = a.pal[(int64_t)(p0 + pp) * a.pal_pitch + k[i]];
                }
                const bool movable = contend && (pr[i] != c.x || pg[i] != c.y || pb[i] != c.z);
                key[i] = movable ? ((unsigned long long)bits << 32) | (0xffffffffu - (a.pos0 + q + (uint32_t)i)) : 0ull;
            }
            const uint32_t k0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)k[0]);
            const bool same = k[0] == k0 && k[1] == k0 && k[2] == k0 && k[3] == k0;
            if (__builtin_amdgcn_ballot_w64(!same) == 0) {
                unsigned long long sn = 0ull, km = 0ull;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    sn += v[i] + ((unsigned long long)(own[i] ? 1 : 0) << 52);
                    km = key[i] > km ? key[i] : km;
                }
                sn = wave_sum_u64(sn);
                km = err_wave_max(km);
                if (lane == 0 && (sn >> 52)) add(pp, k0, sn & ((1ull << 52) - 1ull), sn >> 52, km);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (own[i]) add(pp, k[i], v[i], 1ull, key[i]);
            }
        }
    }
    if (bad) *a.bad = 1;
    if constexpr (LDS) {
        __syncthreads();
        for (int e = tid; e < ng * kMaxK; e += 256) {
            const int pp = e >> 8, k = e & (kMaxK - 1);
            const uint32_t n = s_cnt[e];
            if (k >= a.K || !n) continue;
            unsigned long long* o = a.stats + ((int64_t)(p0 + pp) * a.K + k) * 4;
            if (s_sum[e]) atomicAdd(o, s_sum[e]);
            atomicAdd(o + 1, (unsigned long long)n);
            if (s_key[e]) atomicMax(o + 2, s_key[e]);
        }
    }
}

// ----------------------------------------------------------------------------
// worst_rgb: one thread per palette colour.  The colour's key names its worst
// movable pixel; (R, G, B, 0) of that pixel as the argmin saw it, zeros without one.
// ----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void worst_rgb_kernel(ClusterErrArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)a.P * a.K) return;
    const unsigned long long key = a.stats[4 * i + 2];
    float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
    const uint32_t q = 0xffffffffu - (uint32_t)key - a.pos0;  // the position in the extended rows
    if (key && q >= a.q0 && q < a.q1) {
        if (a.rgbx) {
            const uint32_t v = a.rgbx[q];
            c = make_float4(u8_unit(v, 0), u8_unit(v, 1), u8_unit(v, 2), 0.f);
        } else {
            c = make_float4(a.R[q], a.G[q], a.B[q], 0.f);
        }
    }
    a.worst[i] = c;
}

// launch_cluster_sums' grid: one resident round of kCentBlocksPerCu workgroups
// per CU over all the palette groups, spans of whole 256-quad steps, no span
// above cent_max_span pixels.  Then the gather of the worst pixels' colours.
hipError_t launch_cluster_errors(const ClusterErrArgs& a0, int idx_bytes, int num_cu, hipStream_t s) {
    ClusterErrArgs a = a0;
    if (a.q1 <= a.q0 || a.P < 1 || a.K < 1) return hipErrorInvalidValue;
    const int ngroups = (a.P + 3) / 4;
    const uint32_t nq = (((a.q1 + 3u) & ~3u) - (a.q0 & ~3u)) >> 2;
    const uint32_t want = (uint32_t)std::max(1, num_cu * kCentBlocksPerCu / ngroups);
    a.qspan = std::min(((nq + want - 1) / want + 255u) / 256u * 256u, cent_max_span(a.rgbx != nullptr) / 4u);
    a.nblocks = (int)((nq + a.qspan - 1) / a.qspan);
    LaunchEventPair ev;
    with_idx(idx_bytes, [&](auto it) {
        using T = typename decltype(it)::type;
        with_bool(a.rgbx != nullptr, [&](auto U8) {
            HQ_LAUNCH((cluster_err_kernel<T, U8.value>), dim3((unsigned)(a.nblocks * ngroups)), dim3(256), 0, s, a,
                      ngroups);
        });
    });
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    ev.second();
    HQ_LAUNCH(worst_rgb_kernel, dim3(blocks_for((int64_t)a.P * a.K)), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace hq
