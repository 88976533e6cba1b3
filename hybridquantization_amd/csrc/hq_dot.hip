// hq_dot.hip -- dot-diffused index images (libhq's addition, no reference counterpart): Knuth's
// dot diffusion (hq.h: hq_dot_population), the error diffusion without a serial recurrence, in
// the place of the plain argmin's (hq_assign.hip) as hq_diffuse.hip's renderings are.
//
// Definition (hq.h), in the argmin's space -- the sRGB-coded planar floats -- per
// channel, every operation one fp32 operation rounded to nearest, none contracted into an fma.
// A class matrix of side n tiled over the image gives pixel (x, y) the class
// cls[(y mod n) n + (x mod n)]; the 8 neighbours weigh 2 (orthogonal) or 1 (diagonal):
//   W(p)   = the weights of p's in-image neighbours of higher class, summed
//   a(q)   = +0, then a = a + (float(wt(p, q)) * e(p)) / float(W(p)) over q's in-image neighbours
//            p of lower class, in ascending class of p
//   v      = min(max(pix(q) + s * a(q), 0), 1)
//   idx(q) = the first minimum over k of ref_dist(v, pal[k])       e(q) = v - pal[idx]
// Two pixels of one class are n >= 4 apart: neither is the other's neighbour, and every source
// of a pixel has a lower class.  So one launch per class, in ascending class on the stream,
// computes the definition: the stream's order is the only order between classes, and no
// workgroup waits on another.
#include "hq_device.h"
#define HQ_DIFFUSE_DEVICE
#include "hq_diffuse.h"
#include "hq_dot.h"

namespace hq {

namespace {

__device__ __forceinline__ bool inside(int x, int y, int W, int H) {
    return (unsigned)x < (unsigned)W && (unsigned)y < (unsigned)H;
}

// W(p) of the pixel p = (px, py) whose cell has the higher-class directions `hi`: all of them
// away from the image's border, else those that stay inside.
__device__ __forceinline__ int dot_weight_sum(uint32_t hi, int px, int py, int W, int H) {
    if (px >= 1 && px < W - 1 && py >= 1 && py < H - 1) return 2 * __popc(hi & kDotOrth) + __popc(hi & kDotDiag);
    int w = 0;
#pragma unroll
    for (int d = 0; d < 8; ++d)
        if ((hi >> d & 1u) && inside(px + dot_dx(d), py + dot_dy(d), W, H)) w += dot_weight(d);
    return w;
}

}  // namespace

// ----------------------------------------------------------------------------
// dot_kernel: grid (ceil(nx ny / 256), P), block 256: one launch renders the pixels of one class
// -- cell (cx, cy) of the matrix, the pixels (cx + i n, cy + j n), i < nx, j < ny -- for every
// palette, one pixel per thread, the palette in LDS.
//   Gather form: the cell's lower-class neighbours come from the table in ascending class
//   (a.tab: uniform over the launch, so scalar loads); the thread reads each in-image one's
//   error, recomputes that source's W from the source cell's higher-class bits and the source's
//   position, and writes its own index and error once.  No atomics on the errors, no scratch;
//   the used bits are ORed in LDS and each workgroup ORs its non-zero words into slot
//   blockIdx.x & 7 of the global copies (the assign kernels' way; the slots were zeroed before
//   the first launch).
//   A source q + off(d) sends to q along 7 - d, whose weight is d's.  q is itself an in-image
//   neighbour of higher class of every source it reads, so W >= wt >= 1.
// ----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dot_kernel(DotArgs a) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) float4 s_pal[kMaxK];
    __shared__ uint32_t s_used[8];
    const int p = blockIdx.y, tid = threadIdx.x;
    const int W = a.W, H = a.H, K = a.K, n = a.n;
    for (int k = tid; k < K; k += 256) s_pal[k] = a.pal[(int64_t)p * kMaxK + k];
    if (tid < 8) s_used[tid] = 0u;
    __syncthreads();
    const int t = blockIdx.x * 256 + tid;
    if (t < a.nx * a.ny) {
        const int j = t / a.nx, i = t - j * a.nx;
        const int x = a.cx + i * n, y = a.cy + j * n;  // inside the image by nx, ny
        const int64_t plane = (int64_t)W * H, q = (int64_t)y * W + x;
        const float* err = a.err + (int64_t)p * 3 * plane;
        const uint32_t low = a.tab[a.cy * n + a.cx];
        float acc[3] = {0.f, 0.f, 0.f};
        for (int s = 0; s < 8; ++s) {
            const uint32_t d = low >> (4 * s) & 15u;
            if (d == kDotEnd) break;  // (uniform)
            const int dx = dot_dx((int)d), dy = dot_dy((int)d);
            const int px = x + dx, py = y + dy;
            if (!inside(px, py, W, H)) continue;
            const uint32_t hi = a.tab[kDotCells + ((a.cy + dy) & (n - 1)) * n + ((a.cx + dx) & (n - 1))];
            const float wsum = (float)dot_weight_sum(hi, px, py, W, H);
            const float wt = (float)dot_weight((int)d);
            const int64_t src = (int64_t)py * W + px;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const float prod = wt * err[ch * plane + src];
                acc[ch] = acc[ch] + prod / wsum;
            }
        }
        const float pix[3] = {a.R[q], a.G[q], a.B[q]};
        float v[3];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float m = a.strength * acc[ch];
            v[ch] = fminf(fmaxf(pix[ch] + m, 0.0f), 1.0f);
        }
        const int k = diffuse_argmin(v[0], v[1], v[2], s_pal, K);
        const float4 c = s_pal[k];
        float* out = a.err + (int64_t)p * 3 * plane + q;
        out[0] = v[0] - c.x;
        out[plane] = v[1] - c.y;
        out[2 * plane] = v[2] - c.z;
        a.idx[(int64_t)p * a.idx_pitch + q] = (uint8_t)k;
        atomicOr(&s_used[k >> 5], 1u << (k & 31));
    }
    __syncthreads();
    if (tid < 8 && s_used[tid])
        atomicOr(&a.used_glob[(blockIdx.x & (kUsedSlots - 1)) * a.used_stride + p * 8 + tid], s_used[tid]);
}

// The launches of one call: the classes 0 .. n^2 - 1 in ascending order, each over the pixels its
// cell has in the image; a class without one (the image is smaller than the tile) gets no launch
// -- a zero-sized grid is an error.  The pending profiling events bracket the whole chain: start
// on the first launch, stop on the last.
hipError_t launch_dot(const DotArgs& a0, int P, hipStream_t s, AssignTag* tag) {
    const int n = a0.n, cells = n * n;
    if ((n != 4 && n != 8 && n != 16) || a0.K < 1 || a0.K > kMaxK || a0.W < 1 || a0.H < 1 || P < 1 || P > kDotMaxP ||
        !a0.cls || !a0.tab || !a0.err || (int64_t)a0.W * a0.H > INT32_MAX)  // (a class's pixel count fits an int)
        return hipErrorInvalidValue;
    int cell_of[kDotCells];
    for (int c = 0; c < cells; ++c) cell_of[c] = -1;
    for (int c = 0; c < cells; ++c) {
        if (a0.cls[c] < 0 || a0.cls[c] >= cells || cell_of[a0.cls[c]] >= 0) return hipErrorInvalidValue;
        cell_of[a0.cls[c]] = c;
    }
    // the classes with a pixel: cell (cx, cy) has one when cx < W and cy < H
    int first = -1, last = -1;
    for (int k = 0; k < cells; ++k)
        if (cell_of[k] % n < a0.W && cell_of[k] / n < a0.H) {
            if (first < 0) first = k;
            last = k;
        }
    const hipEvent_t start = t_ev_start, stop = t_ev_stop;
    DotArgs a = a0;
    for (int k = 0; k < cells; ++k) {
        a.cx = cell_of[k] % n, a.cy = cell_of[k] / n;
        if (a.cx >= a.W || a.cy >= a.H) continue;
        a.nx = (a.W - a.cx + n - 1) / n, a.ny = (a.H - a.cy + n - 1) / n;
        t_ev_start = k == first ? start : nullptr;
        t_ev_stop = k == last ? stop : nullptr;
        HQ_LAUNCH(dot_kernel, dim3(blocks_for((int64_t)a.nx * a.ny), P), dim3(256), 0, s, a);
    }
    t_ev_start = start, t_ev_stop = stop;
    // hq.h's hq_path_argmin: HQ_ARGMIN_DOT (the planar floats, always)
    if (tag) *tag = AssignTag{7, 0, 0, 0};
    return hipGetLastError();
}

}  // namespace hq
