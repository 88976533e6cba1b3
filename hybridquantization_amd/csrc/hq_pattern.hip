// hq_pattern.hip -- pattern dithering (hq.h: hq_pattern_population): the index images
// and used flags of a population in one launch, in the place of grid + assign.
//
// Every pixel is independent: it runs n steps of error feedback on itself alone, each step an
// exhaustive first-minimum argmin over the K colours, keeps the n winners, and the threshold map
// picks the one at position r of their luminance order.  The work is n K distances per pixel, so
// the kernel is built around the VALU:
//
//   - grid (pixel blocks, P), 256 threads; a workgroup holds one palette: the K float4 colours
//     (padded to a multiple of 4 with a colour no pixel can be near), the rank of each colour and
//     the colour of each rank, under 5 KiB of LDS, filled once;
//   - in the K loop every lane reads the same colour at the same time, one 128-bit broadcast read
//     that no bank conflict can touch, unrolled by 4;
//   - each lane holds kPatternPx pixels in registers, so one colour read serves kPatternPx
//     distances: with one pixel per lane the loop would issue one LDS read per ten VALU
//     instructions and wait on it;
//   - a distance is dist2_rank's fma chain (6 instructions), the first minimum a strict < in
//     ascending k (2 selects), and the runner-up rides along in one v_med3 so that a near tie
//     (near_d2: v_sqrt_f32 can give two d^2 one distance) is re-resolved by the reference loop
//     itself, as every exhaustive argmin of the library does (diffuse_argmin);
//   - the n winners are kept as rank bytes, four to a dword, n / 4 dwords per pixel.  The kernel
//     is a template on n: the dword count sizes the register array, and every access to it is at
//     a compile-time position -- the dword being filled is a scalar of the rolled outer loop, and
//     it lands in the array through a chain of selects on that scalar -- so nothing goes to
//     scratch.  The loop over the dwords stays rolled: n = 64 unrolled would be 64 copies of the
//     K loop, more code than the instruction cache holds;
//   - entry r of the sorted list is found without sorting: s_r is the largest t with
//     #{i : rank_i < t} <= r, a binary search over the 8 bits of t.  The bytes are pre-split into
//     the even and the odd ones of each dword, 16 bits apart, so one add of 256 - t to both halves
//     sets bit 8 of a half exactly where rank >= t, and v_bcnt counts them: 6 instructions per
//     dword and bit, 768 at n = 64 against 10 n K for the distances;
//   - the rank goes back to its colour through the LDS table, the index out as a byte, the used
//     flag into an LDS byte per colour, flushed as assign_pipe_kernel flushes its own.
//
// Pixel j of a lane is pixel ((block kPatternPx + j) 256 + lane) of the extended rows, so a wave's
// loads and byte stores are 64 consecutive elements.  Both image forms give the same bits: the
// packed form rebuilds k / 255 exactly (u8_unit).
#include "hq_device.h"
#include "hq_launch.h"
#include "hq_pattern.h"

namespace hq {

namespace {

// Pixels per lane (2 or 4 were measured: DESIGN.md 34).
#ifndef HQ_PATTERN_PX
#define HQ_PATTERN_PX 4
#endif
constexpr int kPatternPx = HQ_PATTERN_PX;
constexpr int kPatternThreads = 256;
static_assert(kPatternMaxK == kMaxK && kMaxK == kPatternThreads, "one table entry per thread");

// The value step i's argmin reads, one channel (hq.h): a product, a sum, a clamp.
__device__ __forceinline__ float pattern_value(float pix, float e, float strength) {
#pragma clang fp contract(off)
    const float t = e * strength;
    return fminf(fmaxf(pix + t, 0.0f), 1.0f);
}
// ... and the error after it: e + (pix - colour), a difference, then a sum.
__device__ __forceinline__ float pattern_error(float e, float pix, float c) {
#pragma clang fp contract(off)
    const float d = pix - c;
    return e + d;
}

// The first minimum over the K colours of ref_dist for PX values at once (diffuse_argmin's rule
// and result, the colour reads shared).  Kp: K rounded up to 4; s_pal[K .. Kp) hold a colour far
// from the unit cube, which never wins and never comes near_d2 of a winner.
template <int PX>
__device__ __forceinline__ void pattern_argmin(const float (&vr)[PX], const float (&vg)[PX], const float (&vb)[PX],
                                               const float4* s_pal, int K, int Kp, int (&bi)[PX]) {
    float best2[PX], second2[PX];
#pragma unroll
    for (int j = 0; j < PX; ++j) best2[j] = INFINITY, second2[j] = INFINITY, bi[j] = 0;
    for (int k = 0; k < Kp; k += 4) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float4 c = s_pal[k + u];
#pragma unroll
            for (int j = 0; j < PX; ++j) {
                const float d2 = dist2_rank(vr[j], vg[j], vb[j], c);
                const bool lt = d2 < best2[j];
                bi[j] = lt ? k + u : bi[j];
                second2[j] = __builtin_amdgcn_fmed3f(best2[j], second2[j], d2);
                best2[j] = lt ? d2 : best2[j];
            }
        }
    }
#pragma unroll
    for (int j = 0; j < PX; ++j) {
        if (near_d2(best2[j], second2[j])) {  // (rare, and divergent: the reference loop itself)
            int b = 0;
            float best = ref_dist(vr[j], vg[j], vb[j], s_pal[0]);
            for (int k = 1; k < K; ++k) {
                const float d = ref_dist(vr[j], vg[j], vb[j], s_pal[k]);
                if (d < best) best = d, b = k;
            }
            bi[j] = b;
        }
    }
}

// Entry r of the ND dwords' 4 ND rank bytes in ascending order (bytes of 0xff that pad a list
// shorter than a dword sort last and r never reaches them).
template <int ND>
__device__ __forceinline__ uint32_t pattern_select(const uint32_t (&cand)[ND], int r) {
    uint32_t ev[ND], od[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d) ev[d] = cand[d] & 0x00ff00ffu, od[d] = (cand[d] >> 8) & 0x00ff00ffu;
    uint32_t ans = 0;
#pragma unroll
    for (int bit = 7; bit >= 0; --bit) {
        const uint32_t t = ans | (1u << bit);        // 1 .. 255
        const uint32_t add = (256u - t) * 0x00010001u;  // a half x + 256 - t < 512: bit 8 iff x >= t, no carry out
        uint32_t ge = 0;
#pragma unroll
        for (int d = 0; d < ND; ++d)
            ge += __popc((ev[d] + add) & 0x01000100u) + __popc((od[d] + add) & 0x01000100u);
        ans = 4 * ND - (int)ge <= r ? t : ans;  // #{rank < t} <= r: s_r >= t
    }
    return ans;
}

}  // namespace

// ----------------------------------------------------------------------------
// pattern_kernel<N, U8>: grid (ceil(n_ext / (256 kPatternPx)), P), block 256.
// ----------------------------------------------------------------------------
template <int N, bool U8>
__global__ __launch_bounds__(kPatternThreads) void pattern_kernel(PatternArgs a) {
    constexpr int PX = kPatternPx;
    constexpr int ND = N >= 4 ? N / 4 : 1;  // dwords of rank bytes per pixel
    constexpr int NT = N >= 4 ? 4 : N;      // steps per dword
    __shared__ __attribute__((aligned(16))) float4 s_pal[kMaxK];
    __shared__ __attribute__((aligned(16))) uint8_t s_rank[kMaxK], s_color[kMaxK], s_usedb[kMaxK];
    const int p = blockIdx.y, tid = threadIdx.x, K = a.K, Kp = (K + 3) & ~3;
    s_pal[tid] = tid < K ? a.pal[(int64_t)p * kMaxK + tid] : make_float4(1e15f, 1e15f, 1e15f, 0.f);
    s_rank[tid] = a.tab[(int64_t)p * 2 * kMaxK + tid];
    s_color[tid] = a.tab[(int64_t)p * 2 * kMaxK + kMaxK + tid];
    s_usedb[tid] = 0;

    // this lane's pixels; one past the image is the last pixel again, resolved and not stored
    int64_t q[PX];
    float pr[PX], pg[PX], pb[PX];
#pragma unroll
    for (int j = 0; j < PX; ++j) {
        q[j] = ((int64_t)blockIdx.x * PX + j) * kPatternThreads + tid;
        const int64_t qc = q[j] < a.n_ext ? q[j] : a.n_ext - 1;
        if constexpr (U8) {
            const uint32_t v = a.rgbx[qc];
            pr[j] = u8_unit(v, 0), pg[j] = u8_unit(v, 1), pb[j] = u8_unit(v, 2);
        } else {
            pr[j] = a.R[qc], pg[j] = a.G[qc], pb[j] = a.B[qc];
        }
    }
    __syncthreads();

    float er[PX], eg[PX], eb[PX];
    uint32_t cand[PX][ND];
    int first[PX];  // (N = 1: the one winner)
#pragma unroll
    for (int j = 0; j < PX; ++j) {
        er[j] = eg[j] = eb[j] = 0.0f;
        first[j] = 0;
#pragma unroll
        for (int d = 0; d < ND; ++d) cand[j][d] = 0u;
    }
#pragma unroll 1
    for (int dw = 0; dw < ND; ++dw) {
        uint32_t w[PX];
#pragma unroll
        for (int j = 0; j < PX; ++j) w[j] = NT < 4 ? ~0u << (8 * (NT & 3)) : 0u;  // (a list shorter than a dword: 0xff pads it)
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            float vr[PX], vg[PX], vb[PX];
            int bi[PX];
#pragma unroll
            for (int j = 0; j < PX; ++j) {
                vr[j] = pattern_value(pr[j], er[j], a.strength);
                vg[j] = pattern_value(pg[j], eg[j], a.strength);
                vb[j] = pattern_value(pb[j], eb[j], a.strength);
            }
            pattern_argmin<PX>(vr, vg, vb, s_pal, K, Kp, bi);
#pragma unroll
            for (int j = 0; j < PX; ++j) {
                const float4 c = s_pal[bi[j]];
                er[j] = pattern_error(er[j], pr[j], c.x);
                eg[j] = pattern_error(eg[j], pg[j], c.y);
                eb[j] = pattern_error(eb[j], pb[j], c.z);
                if constexpr (N == 1) first[j] = bi[j];
                else w[j] |= (uint32_t)s_rank[bi[j]] << (8 * t);
            }
        }
#pragma unroll
        for (int j = 0; j < PX; ++j)
#pragma unroll
            for (int d = 0; d < ND; ++d) cand[j][d] = d == dw ? w[j] : cand[j][d];
    }

    uint8_t* idx = a.idx + (int64_t)p * a.idx_pitch;
#pragma unroll
    for (int j = 0; j < PX; ++j) {
        int k = first[j];
        if constexpr (N > 1) {
#pragma clang fp contract(off)
            // (x, y): the position in the full image; the map read is in bounds by the masks
            const int64_t qc = q[j] < a.n_ext ? q[j] : a.n_ext - 1;
            const uint32_t row = (uint32_t)(qc / a.W), x = (uint32_t)(qc - (int64_t)row * a.W), y = row + a.y0;
            const float m = a.map[((y & a.mh_mask) << a.lg_mw) | (x & a.mw_mask)];
            const float pos = (m + 0.5f) * (float)N;
            const int r = min((int)pos, N - 1);
            k = s_color[pattern_select<ND>(cand[j], r)];
        }
        if (q[j] < a.n_ext) {
            __builtin_nontemporal_store((uint8_t)k, idx + q[j]);
            s_usedb[k] = 1;
        }
    }
    __syncthreads();
    // the workgroup's used bits into the palette's 8 words of slot blockIdx.x & 7, as
    // assign_pipe_kernel does: bytes to words by ballot, a load first so that only new bits cost an atomic
    __shared__ uint32_t s_words[8];
    const int lane = tid & 63, wv = tid >> 6;
    const uint64_t bits = __ballot(s_usedb[tid] != 0);
    if (lane < 2) s_words[2 * wv + lane] = lane ? (uint32_t)(bits >> 32) : (uint32_t)bits;
    __syncthreads();
    if (tid < 8) {
        const uint32_t mword = s_words[tid];
        uint32_t* gw = &a.used_glob[(blockIdx.x & (kUsedSlots - 1)) * a.used_stride + p * 8 + tid];
        const uint32_t seen = __hip_atomic_load(gw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (mword & ~seen) atomicOr(gw, mword);
    }
}

namespace {

template <int N>
void launch_pattern_n(const PatternArgs& a, dim3 grid, hipStream_t s) {
    with_bool(a.rgbx != nullptr, [&](auto U8) {
        HQ_LAUNCH((pattern_kernel<N, U8.value>), grid, dim3(kPatternThreads), 0, s, a);
    });
}

}  // namespace

// One launch; the pending profiling events ride on it.
hipError_t launch_pattern(const PatternArgs& a, int P, hipStream_t s, AssignTag* tag) {
    const bool planes = a.R && a.G && a.B;
    if (!pattern_n_valid(a.n) || a.K < 1 || a.K > kMaxK || P < 1 || P > 65535 || a.n_ext < 1 || a.W < 1 ||
        a.idx_pitch < a.n_ext || !(a.rgbx || planes) || !a.pal || !a.tab || !a.map || !a.idx || !a.used_glob ||
        a.mw_mask >= (uint32_t)kMaxMapSide || a.mh_mask >= (uint32_t)kMaxMapSide ||
        (a.mw_mask + 1u) != (1u << a.lg_mw) || (a.mh_mask & (a.mh_mask + 1u)) != 0 ||
        !(a.strength >= 0.0f && a.strength <= 1.0f))
        return hipErrorInvalidValue;
    const int64_t per = (int64_t)kPatternThreads * kPatternPx, blocks = (a.n_ext + per - 1) / per;
    if (blocks > INT32_MAX) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks, (unsigned)P);
    switch (a.n) {
    case 1: launch_pattern_n<1>(a, grid, s); break;
    case 2: launch_pattern_n<2>(a, grid, s); break;
    case 4: launch_pattern_n<4>(a, grid, s); break;
    case 8: launch_pattern_n<8>(a, grid, s); break;
    case 16: launch_pattern_n<16>(a, grid, s); break;
    case 32: launch_pattern_n<32>(a, grid, s); break;
    default: launch_pattern_n<64>(a, grid, s); break;
    }
    // hq.h's hq_path_argmin: HQ_ARGMIN_PATTERN, and which image form it read
    if (tag) *tag = AssignTag{8, a.rgbx != nullptr, 0, 0};
    return hipGetLastError();
}

}  // namespace hq
