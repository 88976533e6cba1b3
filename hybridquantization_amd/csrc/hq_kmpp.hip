// hq_kmpp.hip -- k-means++ seeding (Arthur & Vassilvitskii 2007) of a whole population of P
// palettes at once (hq_kmeanspp_seed).  libhq's own addition: the reference starts its search
// from uniform random colours.
//
// A round draws one pixel per palette with probability proportional to w(x) D(x), D the squared
// distance to the palette's nearest centre so far.  Everything is integer -- channel values q
// (the packed bytes, or RN(v 4095) of the planar floats), weights 0 .. 255, 64-bit sums -- and the
// draw is "the first pixel in raster order whose prefix sum of w D passes t", so the result does
// not depend on how the image is split over workgroups and compares exactly against numpy.
//
// Two kernels per round, in stream order, no host round trip:
//   kmpp_update_kernel  streams the image once for all P palettes: minD <- min(minD, d(newest
//                       centre)) per palette, and one 64-bit partial sum of w minD per (palette,
//                       span), stored plainly (no atomics: the partials are deterministic);
//   kmpp_pick_kernel    one workgroup per palette: T from the partials, t = mulhi64(u, T), a scan
//                       of the partials for the span that holds the crossing, a scan of that one
//                       span's w minD for the pixel, and the centre appended.
#include "hq_device.h"
#include "hq_kmpp.h"
#include "hq_launch.h"

namespace hq {

// The sum of a 64-bit integer over the wave with DPP moves only (wave_sum_to_lane63's order, on
// both halves of the word): lane 63 alone holds the total.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint64_t dpp_u64(uint64_t u) {
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)u, CTRL, ROW_MASK, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)(u >> 32), CTRL, ROW_MASK, 0xf, true);
    return ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo;
}
__device__ __forceinline__ uint64_t wave_sum_u64_to_lane63(uint64_t v) {
    v += dpp_u64<0x111, 0xf>(v);  // row_shr:1
    v += dpp_u64<0x112, 0xf>(v);  // row_shr:2
    v += dpp_u64<0x114, 0xf>(v);  // row_shr:4
    v += dpp_u64<0x118, 0xf>(v);  // row_shr:8
    v += dpp_u64<0x142, 0xa>(v);  // row_bcast:15 into rows 1 and 3
    v += dpp_u64<0x143, 0xc>(v);  // row_bcast:31 into rows 2 and 3
    return v;
}

// A quad of pixels: q of its channels and the weights, 0 for a pixel that does not count (past the
// image's end, outside the span's last step, masked out).
struct KmppQuad {
    int r[4], g[4], b[4];
    uint32_t w[4];
};
template <bool U8>
__device__ __forceinline__ KmppQuad kmpp_load_quad(const KmppArgs& a, uint32_t q, bool in) {
    KmppQuad k;
    uint32_t mq = 0x01010101u;
    if (a.mask) mq = *reinterpret_cast<const uint32_t*>(a.mask + q);
    if constexpr (U8) {
        const uint4 px = *reinterpret_cast<const uint4*>(a.rgbx + q);
        const uint32_t v[4] = {px.x, px.y, px.z, px.w};
#pragma unroll
        for (int i = 0; i < 4; ++i)
            k.r[i] = (int)(v[i] & 0xffu), k.g[i] = (int)((v[i] >> 8) & 0xffu), k.b[i] = (int)((v[i] >> 16) & 0xffu);
    } else {
        const float4 fr = *reinterpret_cast<const float4*>(a.R + q);
        const float4 fg = *reinterpret_cast<const float4*>(a.G + q);
        const float4 fb = *reinterpret_cast<const float4*>(a.B + q);
        const float vr[4] = {fr.x, fr.y, fr.z, fr.w}, vg[4] = {fg.x, fg.y, fg.z, fg.w}, vb[4] = {fb.x, fb.y, fb.z, fb.w};
#pragma unroll
        for (int i = 0; i < 4; ++i)
            k.r[i] = kmpp_q(vr[i], kKmppScale), k.g[i] = kmpp_q(vg[i], kKmppScale), k.b[i] = kmpp_q(vb[i], kKmppScale);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) k.w[i] = in && q + i < a.n ? (mq >> (8 * i)) & 0xffu : 0u;
    return k;
}

// ----------------------------------------------------------------------------
// kmpp_update: grid (nspans * ceil(P / 64)), block 256, XCD-relabelled.
// ----------------------------------------------------------------------------
// A workgroup takes one span of the pixels and one group of up to 64 palettes (after the
// relabelling the groups of a span are consecutive, so they meet in one L2, as centroid's).  A
// thread loads a quad of pixels once -- 16 B packed or 3 x 16 B planar, and the quad's 4 weight
// bytes -- and then walks the group's palettes: the palette's newest centre from LDS (16 B, a
// broadcast read), the palette's minD quad (16 B), four integer distances, the min, the store,
// and w minD summed over the wave by DPP into the palette's word of LDS (lane 63 adds: one word
// per palette and wave, so no atomic).  Per palette and pixel that is 8 B of traffic against the
// pixel's 4 or 12 B loaded once: the minD planes are what the kernel streams.
// init (the first launch of a call): minD starts from the sentinel instead of being loaded, and the
// spans' sums of w go to wpart (the first group's workgroups).  k_new < 0 (no centre yet: round 0
// without fixed colours): the sentinel is stored and no partial is made -- the pick reads wpart.
// No scratch: the palette loop keeps nothing per palette in registers.
template <bool U8>
__global__ __launch_bounds__(256) void kmpp_update_kernel(KmppArgs a, int k_new, int init, int ngroups) {
    __shared__ int4 s_c[kKmppGroup];
    __shared__ unsigned long long s_sum[kKmppGroup * 4];
    __shared__ unsigned long long s_w[4];
    const int w = xcd_remap(blockIdx.x, a.nspans * ngroups);
    const int span = w / ngroups, grp = w % ngroups, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p0 = kKmppGroup * grp, ng = min(kKmppGroup, a.P - p0);
    if (tid < ng) s_c[tid] = k_new >= 0 ? a.cent[(int64_t)(p0 + tid) * a.K + k_new] : make_int4(0, 0, 0, 0);
    s_sum[tid] = 0ull;  // (kKmppGroup * 4 = 256 words)
    if (tid < 4) s_w[tid] = 0ull;
    __syncthreads();
    static_assert(kKmppGroup * 4 == 256, "one word of s_sum per thread");
    const uint32_t nq = (a.n + 3u) >> 2;
    const int64_t pitch = 4 * (int64_t)nq;
    const uint32_t j0 = (uint32_t)span * a.qspan, j1 = min(j0 + a.qspan, nq);
    const bool wsum = init && grp == 0;
    // (every lane of the workgroup runs every step: the wave sums need them all)
    for (uint32_t jb = j0; jb < j1; jb += 256u) {
        const uint32_t j = jb + (uint32_t)tid;
        const bool in = j < j1;
        const uint32_t q = 4u * min(j, nq - 1u);
        const KmppQuad k = kmpp_load_quad<U8>(a, q, in);
        if (wsum) {
            const uint64_t t = wave_sum_u64_to_lane63((uint64_t)(k.w[0] + k.w[1] + k.w[2] + k.w[3]));
            if (lane == 63) s_w[wave] += t;
        }
        for (int pp = 0; pp < ng; ++pp) {
            uint32_t* md = a.mind + (int64_t)(p0 + pp) * pitch + q;
            uint4 m = make_uint4(kKmppSentinel, kKmppSentinel, kKmppSentinel, kKmppSentinel);
            if (!init && in) m = *reinterpret_cast<const uint4*>(md);
            if (k_new < 0) {
                if (in) *reinterpret_cast<uint4*>(md) = m;
                continue;
            }
            const int4 c = s_c[pp];
            uint32_t mm[4] = {m.x, m.y, m.z, m.w};
            uint64_t s = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int dr = k.r[i] - c.x, dg = k.g[i] - c.y, db = k.b[i] - c.z;
                mm[i] = min(mm[i], (uint32_t)(dr * dr + dg * dg + db * db));
                s += (uint64_t)k.w[i] * mm[i];  // (a pixel that does not count has w = 0)
            }
            if (in) *reinterpret_cast<uint4*>(md) = make_uint4(mm[0], mm[1], mm[2], mm[3]);
            const uint64_t t = wave_sum_u64_to_lane63(s);
            if (lane == 63) s_sum[pp * 4 + wave] += t;
        }
    }
    __syncthreads();
    if (tid < ng && k_new >= 0)
        a.part[(int64_t)(p0 + tid) * a.nspans + span] =
            s_sum[tid * 4] + s_sum[tid * 4 + 1] + s_sum[tid * 4 + 2] + s_sum[tid * 4 + 3];
    if (wsum && tid == 0) a.wpart[span] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// ----------------------------------------------------------------------------
// kmpp_pick: grid (P), block 256.
// ----------------------------------------------------------------------------
// A workgroup scan over 256 values in thread order, one per thread, on top of `base` (the sum of
// everything before them): hit = the thread whose inclusive prefix is the first above t (256:
// none), excl = the prefix before that thread, total = base + all 256.  The values are not
// negative and base <= t, so at most one thread has excl <= t < incl.  The wave's prefix by
// __shfl_up, the waves' totals through LDS.
struct KmppFound {
    int hit;
    uint64_t excl, total;
};
struct KmppScan {
    unsigned long long wtot[4], excl;
    int hit;
};
__device__ __forceinline__ KmppFound kmpp_find(uint64_t v, uint64_t base, uint64_t t, KmppScan& s) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint64_t inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint64_t up = __shfl_up(inc, off, 64);
        if (lane >= off) inc += up;
    }
    __syncthreads();  // (the last call's results have been read)
    if (lane == 63) s.wtot[wave] = inc;
    if (tid == 0) s.hit = 256;
    __syncthreads();
    uint64_t before = base, total = base;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint64_t x = s.wtot[i];
        before += i < wave ? x : 0ull;
        total += x;
    }
    inc += before;
    if (inc > t && inc - v <= t) s.hit = tid, s.excl = inc - v;
    __syncthreads();
    return KmppFound{s.hit, s.excl, total};
}

// The draw of round r for palette p = blockIdx.x.  `unit`: D = 1, the weights alone (round 0
// without fixed colours); it is also what the round falls back to when T = 0, every in-mask
// colour being a centre already.  T > 0 then holds (the runtime refuses a weight sum of 0), so
// the crossing exists; a workgroup that finds none writes the index -1, which the runtime reports.
template <bool U8>
__global__ __launch_bounds__(256) void kmpp_pick_kernel(KmppArgs a, int r, int unit0) {
    __shared__ KmppScan s_scan;
    const int p = blockIdx.x, tid = threadIdx.x;
    const uint32_t nq = (a.n + 3u) >> 2;
    const uint64_t kNever = ~0ull;
    const int64_t e = (int64_t)p * a.K + r;
    if (tid == 0) a.pix[e] = -1;  // (the scans' barriers lie between this store and the finder's)
    bool unit = unit0 != 0;
    const unsigned long long* part = unit ? a.wpart : a.part + (int64_t)p * a.nspans;
    auto total = [&]() {
        uint64_t sum = 0;
        for (int s0 = 0; s0 < a.nspans; s0 += 256)
            sum = kmpp_find(s0 + tid < a.nspans ? part[s0 + tid] : 0ull, sum, kNever, s_scan).total;
        return sum;
    };
    uint64_t T = total();
    if (!unit && T == 0) {  // (uniform: T is the same in every thread)
        unit = true;
        part = a.wpart;
        T = total();
    }
    const uint64_t t = __umul64hi(kmpp_word(a.seed, (uint32_t)p, (uint32_t)r), T);
    // the span whose partial takes the prefix above t
    int span = -1;
    uint64_t base = 0;
    for (int s0 = 0; s0 < a.nspans && span < 0; s0 += 256) {
        const KmppFound f = kmpp_find(s0 + tid < a.nspans ? part[s0 + tid] : 0ull, base, t, s_scan);
        if (f.hit < 256) span = s0 + f.hit, base = f.excl;
        else base = f.total;
    }
    long long chosen = -1;  // (in the thread that finds the pixel)
    if (span >= 0) {
        const uint32_t* md = a.mind + (int64_t)p * 4 * (int64_t)nq;
        const uint32_t j0 = (uint32_t)span * a.qspan, j1 = min(j0 + a.qspan, nq);
        for (uint32_t jb = j0; jb < j1; jb += 256u) {
            const uint32_t j = jb + (uint32_t)tid;
            const bool in = j < j1;
            const uint32_t q = 4u * min(j, nq - 1u);
            uint32_t mq = 0x01010101u;
            if (a.mask) mq = *reinterpret_cast<const uint32_t*>(a.mask + q);
            uint4 m = make_uint4(1u, 1u, 1u, 1u);
            if (!unit) m = *reinterpret_cast<const uint4*>(md + q);
            const uint32_t mm[4] = {m.x, m.y, m.z, m.w};
            uint64_t v[4], sum = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                v[i] = in && q + i < a.n ? (uint64_t)((mq >> (8 * i)) & 0xffu) * mm[i] : 0ull;
                sum += v[i];
            }
            const KmppFound f = kmpp_find(sum, base, t, s_scan);
            base = f.total;
            if (f.hit == 256) continue;
            if (f.hit == tid) {
                uint64_t run = f.excl;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    run += v[i];
                    if (chosen < 0 && run > t) chosen = (long long)q + i;
                }
            }
            break;
        }
    }
    if (chosen < 0) return;
    int4 c;
    float4 o;
    if constexpr (U8) {
        const uint32_t px = a.rgbx[chosen];
        c = make_int4((int)(px & 0xffu), (int)((px >> 8) & 0xffu), (int)((px >> 16) & 0xffu), 0);
        o = make_float4(u8_unit(px, 0), u8_unit(px, 1), u8_unit(px, 2), 0.f);
    } else {
        o = make_float4(a.R[chosen], a.G[chosen], a.B[chosen], 0.f);
        c = make_int4(kmpp_q(o.x, kKmppScale), kmpp_q(o.y, kKmppScale), kmpp_q(o.z, kKmppScale), 0);
    }
    a.cent[e] = c;
    a.out[e] = o;
    a.pix[e] = chosen;
}

// One resident round of kKmppBlocksPerCu workgroups per CU over all the palette groups, spans of
// whole 256-quad steps and of kKmppMinQspan quads at least (a small image is one span: more
// workgroups would only add partials for the pick to scan).
void kmpp_spans(uint32_t n, int P, uint32_t span, int num_cu, uint32_t* qspan, int* nspans) {
    const uint32_t nq = (n + 3u) >> 2;
    const int ngroups = (P + kKmppGroup - 1) / kKmppGroup;
    const uint32_t want = (uint32_t)std::max(1, num_cu * kKmppBlocksPerCu / ngroups);
    const uint32_t by_grid = std::max(((nq + want - 1) / want + 255u) / 256u * 256u, kKmppMinQspan);
    const uint32_t asked = (uint32_t)(((uint64_t)span + 3u) / 4u + 255u) / 256u * 256u;
    *qspan = span ? asked : by_grid;
    *nspans = (int)((nq + *qspan - 1) / *qspan);
}

hipError_t launch_kmpp_update(const KmppArgs& a, int k_new, bool init, hipStream_t s) {
    const int ngroups = (a.P + kKmppGroup - 1) / kKmppGroup;
    with_bool(a.rgbx != nullptr, [&](auto U8) {
        HQ_LAUNCH((kmpp_update_kernel<U8.value>), dim3((unsigned)(a.nspans * ngroups)), dim3(256), 0, s, a, k_new,
                  (int)init, ngroups);
    });
    return hipGetLastError();
}

hipError_t launch_kmpp_pick(const KmppArgs& a, int r, bool unit, hipStream_t s) {
    with_bool(a.rgbx != nullptr, [&](auto U8) {
        HQ_LAUNCH((kmpp_pick_kernel<U8.value>), dim3((unsigned)a.P), dim3(256), 0, s, a, r, (int)unit);
    });
    return hipGetLastError();
}

}  // namespace hq
