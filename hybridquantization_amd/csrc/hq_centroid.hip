// hq_centroid.hip -- per-colour pixel sums of an evaluated population: for
// every palette p and colour k the sum of the pixels assigned to k and their
// count, the other half of a k-means step (the argmin is assign's).  libhq's own
// addition: the reference has no k-means step.
//
// Everything is integer: the packed image adds its bytes (units of 1/255), the
// planar one q(v) = RN(v 2^32) per channel (units of 2^-32), so the sums do not
// depend on the order of the atomics and compare exactly against numpy.
#include "hq_device.h"
#include "hq_launch.h"

namespace hq {

// ----------------------------------------------------------------------------
// centroid: grid (nblocks * ceil(P/4)), block 256, XCD-relabelled.
// ----------------------------------------------------------------------------
// A workgroup takes one span of the owned pixels and one group of up to 4
// palettes: a thread loads 4 consecutive pixels once (16 B packed, 3 x 16 B
// planar) and the group's 4 indices of each (one load per palette), then adds
// every pixel to its colour's accumulators.  After the relabelling consecutive
// workgroups are the palette groups of one span (span-major, unlike assign),
// so the groups of a span run on one XCD and re-read its pixels from that L2.
//
// K <= kCentLdsK (u8 indices): the accumulators live in LDS, [4][256] colours,
// in 64-bit words that hold more than one field each (one ds_add_u64 per word:
// the LDS atomics are what the kernel waits for).  A workgroup covers at most
// cent_max_span(U8) pixels, so that no field can carry into its neighbour:
//  - packed, 2^22 pixels: 2 words of 2 fields of 32 bits, R | G << 32 and
//    B | count << 32.  A byte sum stays at or below 255 2^22 < 2^30, the count
//    at or below 2^22.
//  - planar, 2^15 pixels: 3 words, R, G and B | count << 48.  A sum of q(v) <=
//    2^32 stays at or below 2^15 2^32 = 2^47 < 2^48, the count at or below
//    2^15 < 2^16.  (With the count in a word of its own, 4 atomics per pixel
//    and palette, the noise image took 0.187 ms at C3 against assign's 0.159.)
//  One flush at the end: the non-zero fields go out as 64-bit integer global
//  atomics, field f of colour k at lane 4 k + f (a wave's atomics cover 512
//  contiguous bytes).
// K > kCentLdsK (u16 and u32 indices): 64-bit integer global atomics straight
//  away, 4 per pixel and palette; the contention on one address is the colour's
//  share of the pixels in flight, spread over more than 256 colours.
// A wave whose 256 pixels all have one colour in a palette (flat regions; a
// single-colour image is the worst case of same-address atomics, 64 lanes on
// one LDS word) sums them across its lanes first and adds once.
// MSK (a pixel mask, ClusterArgs::mask): a masked-out pixel of a quad is loaded
// and not added, like the pixels outside [q0, q1) -- so a wave with one is not
// `full` and takes no shortcut; the planar form's range flag still looks at
// every owned pixel.
// MSK = 2 (pixel weights, hq_set_weights: the mask bytes are the weights): a pixel of weight w > 0
// adds w times its channels and w to the count, one multiply per channel ahead of the same adds;
// weight 0 is the masked-out pixel.  A pixel then adds up to 255 times as much, so the fields are
// others:
//  - packed, 2^16 pixels: the same 2 words of 2 fields of 32 bits.  A sum of w byte stays at or
//    below 255 255 2^16 < 2^32, the count at or below 255 2^16.
//  - planar, 2^22 pixels: 4 whole words, R, G, B and the count.  A sum of w q(v) stays at or below
//    255 2^32 2^22 < 2^62.  (hq_cluster_sums refuses an image whose owned weights sum to 2^31 or
//    more, so that the totals stay below 2^63: hq.h.)  The 32 KiB of LDS hold 5 workgroups per
//    CU where the 3-word form's 24 KiB hold 6.
//  The uniform-wave shortcut adds the wave's weight sum for its count.
template <typename IDX_T, bool U8, int MSK = 0>
__global__ __launch_bounds__(256) void centroid_kernel(ClusterArgs a, int ngroups) {
    constexpr bool LDS = sizeof(IDX_T) == 1;
    constexpr bool WGT = MSK == 2;
    constexpr int F = U8 ? 2 : WGT ? 4 : 3;  // 64-bit words per colour
    static_assert(kCentLdsK == kMaxK && kMaxK == 256, "a u8 index addresses the whole LDS table");
    static_assert(255ull * cent_max_span(true) < (1ull << 32), "packed fields: no carry into the neighbour");
    static_assert(((uint64_t)cent_max_span(false) << 32) < (1ull << 48) && cent_max_span(false) < (1u << 16),
                  "planar B and count: no carry, the count in 16 bits");
    static_assert(255ull * 255ull * cent_max_span(true, true) < (1ull << 32),
                  "weighted packed fields: no carry into the neighbour");
    static_assert(((255ull * cent_max_span(false, true)) << 32) < (1ull << 63),
                  "weighted planar words: a workgroup's sum of w q(v) below 2^63");
    __shared__ unsigned long long s_acc[LDS ? 4 * kMaxK * F : 1];
    const int w = xcd_remap(blockIdx.x, a.nblocks * ngroups);
    const int blk = w / ngroups, grp = w % ngroups, tid = threadIdx.x;
    const int p0 = 4 * grp, ng = min(4, a.P - p0);
    if constexpr (LDS) {
        for (int e = tid; e < 4 * kMaxK * F; e += 256) s_acc[e] = 0ull;
        __syncthreads();
    }
    auto add = [&](int pp, uint32_t k, uint64_t r, uint64_t g, uint64_t b, uint64_t n) {
        if constexpr (LDS) {  // (k <= 255: inside the table whatever the byte)
            unsigned long long* e = s_acc + (pp * kMaxK + (int)k) * F;
            if constexpr (U8) {
                atomicAdd(e, r | (g << 32));
                atomicAdd(e + 1, b | (n << 32));
            } else if constexpr (WGT) {
                atomicAdd(e, r);
                atomicAdd(e + 1, g);
                atomicAdd(e + 2, b);
                atomicAdd(e + 3, n);
            } else {
                atomicAdd(e, r);
                atomicAdd(e + 1, g);
                atomicAdd(e + 2, b | (n << 48));
            }
        } else if (k < (uint32_t)a.K) {
            unsigned long long* e = a.sums + ((int64_t)(p0 + pp) * a.K + k) * 4;
            atomicAdd(e, r);
            atomicAdd(e + 1, g);
            atomicAdd(e + 2, b);
            atomicAdd(e + 3, n);
        }
    };
    // Quads of 4 pixels at multiples of 4 of the extended rows' positions (the
    // owned rows start anywhere): [qa, qa + 4 nq) covers [q0, q1), the pixels
    // outside it are loaded (the buffers are padded to whole quads) but not added.
    const uint32_t qa = a.q0 & ~3u;
    const uint32_t nq = (((a.q1 + 3u) & ~3u) - qa) >> 2;
    const uint32_t j0 = (uint32_t)blk * a.qspan, j1 = min(j0 + a.qspan, nq);
    const IDX_T* idx = static_cast<const IDX_T*>(a.idx);
    const int lane = tid & 63;
    // (every lane of the workgroup runs every step: the wave sums need them all)
    for (uint32_t jb = j0; jb < j1; jb += 256u) {
        const uint32_t j = jb + (uint32_t)tid;
        const bool in = j < j1;
        const uint32_t q = qa + 4u * min(j, nq - 1u);
        uint4 kq[4];
#pragma unroll
        for (int pp = 0; pp < 4; ++pp) kq[pp] = load_idx4(idx + (int64_t)(p0 + min(pp, ng - 1)) * a.idx_pitch + q);
        uint64_t r[4], g[4], b[4];
        bool ok[4];
        uint32_t mq = ~0u;  // MSK: the quad's mask bytes (MSK = 2: its weights)
        if constexpr (MSK != 0) mq = *reinterpret_cast<const uint32_t*>(a.mask + q);
        // what pixel i of the quad adds to its colour's count: 1, or its weight (byte i of mq)
        auto wt = [&](int i) -> uint32_t { return WGT ? (mq >> (8 * i)) & 0xffu : 1u; };
        if constexpr (U8) {
            const uint4 px = *reinterpret_cast<const uint4*>(a.rgbx + q);
            const uint32_t v[4] = {px.x, px.y, px.z, px.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                ok[i] = in && q + i >= a.q0 && q + i < a.q1;
                if constexpr (MSK != 0) ok[i] = ok[i] && ((mq >> (8 * i)) & 0xffu) != 0u;
                r[i] = v[i] & 0xffu;
                g[i] = (v[i] >> 8) & 0xffu;
                b[i] = (v[i] >> 16) & 0xffu;
                if constexpr (WGT) r[i] *= wt(i), g[i] *= wt(i), b[i] *= wt(i);
            }
        } else {
            const float4 fr = *reinterpret_cast<const float4*>(a.R + q);
            const float4 fg = *reinterpret_cast<const float4*>(a.G + q);
            const float4 fb = *reinterpret_cast<const float4*>(a.B + q);
            const float vr[4] = {fr.x, fr.y, fr.z, fr.w}, vg[4] = {fg.x, fg.y, fg.z, fg.w},
                        vb[4] = {fb.x, fb.y, fb.z, fb.w};
            bool bad = false;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const bool own = in && q + i >= a.q0 && q + i < a.q1;
                // finite and in [0, 1] (NaN fails every compare)
                const bool fits = vr[i] >= 0.f && vr[i] <= 1.f && vg[i] >= 0.f && vg[i] <= 1.f && vb[i] >= 0.f &&
                                  vb[i] <= 1.f;
                bad |= own && !fits;
                ok[i] = own && fits;
                if constexpr (MSK != 0) ok[i] = ok[i] && ((mq >> (8 * i)) & 0xffu) != 0u;
                r[i] = unit_q32(fits ? vr[i] : 0.f);
                g[i] = unit_q32(fits ? vg[i] : 0.f);
                b[i] = unit_q32(fits ? vb[i] : 0.f);
                if constexpr (WGT) r[i] *= wt(i), g[i] *= wt(i), b[i] *= wt(i);  // (at most 255 2^32: exact)
            }
            if (bad) *a.bad = 1;
        }
        const bool full = __builtin_amdgcn_ballot_w64(!(ok[0] && ok[1] && ok[2] && ok[3])) == 0;
        bool have = false;  // (wave-uniform) the wave's pixel sums, made once for all the palettes
        uint64_t wr = 0, wg = 0, wb = 0, wn = 256ull;
#pragma unroll
        for (int pp = 0; pp < 4; ++pp) {
            if (pp >= ng) break;
            const uint32_t k[4] = {kq[pp].x, kq[pp].y, kq[pp].z, kq[pp].w};
            const uint32_t k0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)k[0]);
            const bool same = k[0] == k0 && k[1] == k0 && k[2] == k0 && k[3] == k0;
            if (full && __builtin_amdgcn_ballot_w64(!same) == 0) {
                if (!have) {
                    wr = wave_sum_u64(r[0] + r[1] + r[2] + r[3]);
                    wg = wave_sum_u64(g[0] + g[1] + g[2] + g[3]);
                    wb = wave_sum_u64(b[0] + b[1] + b[2] + b[3]);
                    if constexpr (WGT) wn = wave_sum_u64((uint64_t)(wt(0) + wt(1) + wt(2) + wt(3)));  // the wave's weight sum
                    have = true;
                }
                if (lane == 0) add(pp, k0, wr, wg, wb, wn);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (ok[i]) add(pp, k[i], r[i], g[i], b[i], (uint64_t)wt(i));
            }
        }
    }
    if constexpr (LDS) {
        __syncthreads();
        // field f of colour k of palette pp at e = (pp 256 + k) 4 + f; only what is not zero
        for (int e = tid; e < ng * kMaxK * 4; e += 256) {
            const int f = e & 3, pp = e >> 10, k = (e >> 2) & (kMaxK - 1);
            unsigned long long v;
            if constexpr (U8) v = (s_acc[(e >> 2) * 2 + (f >> 1)] >> (32 * (f & 1))) & 0xffffffffull;
            else if constexpr (WGT) v = s_acc[e];
            else if (f < 2) v = s_acc[(e >> 2) * 3 + f];
            else v = f == 2 ? s_acc[(e >> 2) * 3 + 2] & 0xffffffffffffull : s_acc[(e >> 2) * 3 + 2] >> 48;
            if (k < a.K && v) atomicAdd(a.sums + ((int64_t)(p0 + pp) * a.K + k) * 4 + f, v);
        }
    }
}

// One resident round of kCentBlocksPerCu workgroups per CU over all the palette
// groups, spans of whole 256-quad steps, and no span above cent_max_span pixels
// (the LDS accumulators' bound; C3, 4096^2 in 1024 spans: 2^14 pixels each).
hipError_t launch_cluster_sums(const ClusterArgs& a0, int idx_bytes, int num_cu, hipStream_t s) {
    ClusterArgs a = a0;
    const int ngroups = (a.P + 3) / 4;
    const uint32_t nq = (((a.q1 + 3u) & ~3u) - (a.q0 & ~3u)) >> 2;
    const uint32_t want = (uint32_t)std::max(1, num_cu * kCentBlocksPerCu / ngroups);
    const bool wgt = a.mask && a.weighted;
    const uint32_t cap = cent_max_span(a.rgbx != nullptr, wgt) / 4u;
    const uint32_t by_grid = ((nq + want - 1) / want + 255u) / 256u * 256u;
    const uint32_t asked = (a.span / 4u + 255u) / 256u * 256u;  // test option "cent_span", in whole 256-quad steps
    a.qspan = std::min(a.span ? asked : by_grid, cap);
    a.nblocks = (int)((nq + a.qspan - 1) / a.qspan);
    with_idx(idx_bytes, [&](auto it) {
        using T = typename decltype(it)::type;
        with_bool(a.rgbx != nullptr, [&](auto U8) {
            with_mask(a.mask != nullptr, wgt, [&](auto MSK) {
                HQ_LAUNCH((centroid_kernel<T, U8.value, MSK.value>), dim3((unsigned)(a.nblocks * ngroups)), dim3(256),
                          0, s, a, ngroups);
            });
        });
    });
    return hipGetLastError();
}

}  // namespace hq
