// hq_hist.hip -- colour histogram of the image's owned rows: per cell of a
// 2^bits grid per channel the sum of the pixels that fall into it and their
// count (hq_color_histogram), what a median cut makes a seed palette from.
// libhq's own addition: the reference starts its search from random colours.
//
// This is hq_centroid.hip's sums kernel with the cell computed from the pixel
// instead of read from an index image, and the same integers: the packed image
// adds its bytes (units of 1/255), the planar one q(v) = RN(v 2^32) per channel
// (units of 2^-32), so the sums do not depend on the order of the atomics and
// compare exactly against numpy.
#include "hq_device.h"
#include "hq_launch.h"

namespace hq {

// Cell coordinate of a channel value in [0, 1]: min(floor(v 2^bits), 2^bits - 1);
// v 2^bits is exact in fp32 (a power-of-two scaling), at most 64.
__device__ __forceinline__ uint32_t hist_coord(float v, int bits) {
    return min((uint32_t)floorf(v * (float)(1 << bits)), (1u << bits) - 1u);
}

// ----------------------------------------------------------------------------
// hist: grid (nblocks), block 256, one resident round of workgroups.
// ----------------------------------------------------------------------------
// A workgroup takes one span of the owned pixels; a thread loads 4 consecutive
// pixels (16 B packed, 3 x 16 B planar) and adds each to its cell.  The table
// is [2^(3 bits)][4] 64-bit words in global memory (1 MiB at bits = 5: too large
// for LDS), so the sums go out as 64-bit integer global atomics, the form
// centroid takes for K > 256; the 4 words of a cell are one 32-B segment.
// Fewer of them leave the wave:
//  - the pixels of a thread's quad that share a cell are added up first, and the
//    first of them adds for all (smooth images: 4 atomics per quad, not 16);
//  - a wave whose 256 pixels all fall in one cell (flat regions; a single-colour
//    image is otherwise 64 lanes on one address) sums them across its lanes,
//    centroid's uniform-wave shortcut, and keeps the sums while the next steps
//    of its span stay in that cell: one add per run, not per step;
//  - a sum of 0 (a black channel) is not sent.
// No LDS, no scratch: every array below is indexed by unrolled constants.
// MSK (a pixel mask, HistArgs::mask): a masked-out pixel is loaded and not added,
// like the pixels outside [q0, q1); the range flag still looks at every owned pixel.
// MSK = 2 (pixel weights, hq_set_weights: the mask bytes are the weights): a pixel of weight w > 0
// adds w times its channels and w to its cell's count -- in the quad merge and in the uniform
// wave's run too, whose count grows by the wave's weight sum; weight 0 is the masked-out pixel.
// The words are whole 64-bit sums: w q(v) <= 255 2^32 per pixel, and hq_color_histogram refuses
// owned weights that sum to 2^31 or more (hq.h), so a total stays below 2^63.
template <bool U8, int MSK = 0>
__global__ __launch_bounds__(256) void hist_kernel(HistArgs a) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int bits = a.bits;
    auto add = [&](uint32_t cell, uint64_t r, uint64_t g, uint64_t b, uint64_t n) {
        unsigned long long* e = a.cells + (uint64_t)cell * 4u;  // (cell < 2^(3 bits): coordinates below 2^bits)
        if (r) atomicAdd(e, r);
        if (g) atomicAdd(e + 1, g);
        if (b) atomicAdd(e + 2, b);
        atomicAdd(e + 3, n);
    };
    // Quads of 4 pixels at multiples of 4 of the extended rows' positions (the
    // owned rows start anywhere): [qa, qa + 4 nq) covers [q0, q1), the pixels
    // outside it are loaded (the buffers are padded to whole quads) but not added.
    const uint32_t qa = a.q0 & ~3u;
    const uint32_t nq = (((a.q1 + 3u) & ~3u) - qa) >> 2;
    const uint32_t j0 = blockIdx.x * a.qspan, j1 = min(j0 + a.qspan, nq);
    // The wave's run of uniform steps (wave-uniform values; run_n = 0: none): consecutive
    // steps of one cell are added up here and go out once, when the cell changes or the span
    // ends.  Same-address atomics serialise (measured ~12 ns each on the single-colour image).
    uint32_t run_cell = 0;
    uint64_t run_r = 0, run_g = 0, run_b = 0, run_n = 0;
    auto flush = [&]() {
        if (run_n && lane == 0) add(run_cell, run_r, run_g, run_b, run_n);
        run_r = run_g = run_b = run_n = 0;
    };
    // (every lane of the workgroup runs every step: the wave sums need them all)
    for (uint32_t jb = j0; jb < j1; jb += 256u) {
        const uint32_t j = jb + (uint32_t)tid;
        const bool in = j < j1;
        const uint32_t q = qa + 4u * min(j, nq - 1u);
        uint64_t r[4], g[4], b[4];
        uint32_t cell[4];
        uint64_t wt[4] = {1ull, 1ull, 1ull, 1ull};  // what a pixel adds to its cell's count
        bool ok[4];
        uint32_t mq = ~0u;  // MSK: the quad's mask bytes (MSK = 2: its weights)
        if constexpr (MSK != 0) mq = *reinterpret_cast<const uint32_t*>(a.mask + q);
        if constexpr (U8) {
            const uint4 px = *reinterpret_cast<const uint4*>(a.rgbx + q);
            const uint32_t v[4] = {px.x, px.y, px.z, px.w};
            const int sh = 8 - bits;  // byte >> (8 - bits) = min(floor(byte / 255 2^bits), 2^bits - 1)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                ok[i] = in && q + i >= a.q0 && q + i < a.q1;
                if constexpr (MSK != 0) ok[i] = ok[i] && ((mq >> (8 * i)) & 0xffu) != 0u;
                const uint32_t rb = v[i] & 0xffu, gb = (v[i] >> 8) & 0xffu, bb = (v[i] >> 16) & 0xffu;
                r[i] = rb, g[i] = gb, b[i] = bb;
                if constexpr (MSK == 2) {
                    wt[i] = (mq >> (8 * i)) & 0xffu;
                    r[i] *= wt[i], g[i] *= wt[i], b[i] *= wt[i];
                }
                cell[i] = ((rb >> sh) << (2 * bits)) | ((gb >> sh) << bits) | (bb >> sh);
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
                const float cr = fits ? vr[i] : 0.f, cg = fits ? vg[i] : 0.f, cb = fits ? vb[i] : 0.f;
                r[i] = unit_q32(cr), g[i] = unit_q32(cg), b[i] = unit_q32(cb);
                if constexpr (MSK == 2) {  // (at most 255 2^32: exact)
                    wt[i] = (mq >> (8 * i)) & 0xffu;
                    r[i] *= wt[i], g[i] *= wt[i], b[i] *= wt[i];
                }
                cell[i] = (hist_coord(cr, bits) << (2 * bits)) | (hist_coord(cg, bits) << bits) | hist_coord(cb, bits);
            }
            if (bad) *a.bad = 1;
        }
        const bool full = __builtin_amdgcn_ballot_w64(!(ok[0] && ok[1] && ok[2] && ok[3])) == 0;
        const uint32_t c0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)cell[0]);
        const bool same = cell[0] == c0 && cell[1] == c0 && cell[2] == c0 && cell[3] == c0;
        if (full && __builtin_amdgcn_ballot_w64(!same) == 0) {
            const uint64_t wr = wave_sum_u64(r[0] + r[1] + r[2] + r[3]);
            const uint64_t wg = wave_sum_u64(g[0] + g[1] + g[2] + g[3]);
            const uint64_t wb = wave_sum_u64(b[0] + b[1] + b[2] + b[3]);
            if (run_n && run_cell != c0) flush();
            run_cell = c0;
            if constexpr (MSK == 2) run_n += wave_sum_u64(wt[0] + wt[1] + wt[2] + wt[3]);  // the wave's weight sum
            else run_n += 256ull;
            run_r += wr, run_g += wg, run_b += wb;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                bool lead = ok[i];  // the first owned pixel of its cell in the quad adds for the later ones
#pragma unroll
                for (int k = 0; k < i; ++k) lead = lead && !(ok[k] && cell[k] == cell[i]);
                uint64_t sr = r[i], sg = g[i], sb = b[i], sn = wt[i];
#pragma unroll
                for (int k = i + 1; k < 4; ++k) {
                    const bool m = ok[k] && cell[k] == cell[i];
                    sr += m ? r[k] : 0ull, sg += m ? g[k] : 0ull, sb += m ? b[k] : 0ull, sn += m ? wt[k] : 0ull;
                }
                if (lead) add(cell[i], sr, sg, sb, sn);
            }
        }
    }
    flush();
}

// One resident round of kHistBlocksPerCu workgroups per CU, spans of whole
// 256-quad steps (C3, 4096^2 on 256 CUs: 2048 spans of 2^13 pixels).
hipError_t launch_color_histogram(const HistArgs& a0, int num_cu, hipStream_t s) {
    HistArgs a = a0;
    const uint32_t nq = (((a.q1 + 3u) & ~3u) - (a.q0 & ~3u)) >> 2;
    if (nq == 0) return hipSuccess;
    const uint32_t want = (uint32_t)std::max(1, num_cu * kHistBlocksPerCu);
    a.qspan = ((nq + want - 1) / want + 255u) / 256u * 256u;
    a.nblocks = (int)((nq + a.qspan - 1) / a.qspan);
    with_bool(a.rgbx != nullptr, [&](auto U8) {
        with_mask(a.mask != nullptr, a.weighted != 0, [&](auto MSK) {
            HQ_LAUNCH((hist_kernel<U8.value, MSK.value>), dim3((unsigned)a.nblocks), dim3(256), 0, s, a);
        });
    });
    return hipGetLastError();
}

}  // namespace hq
