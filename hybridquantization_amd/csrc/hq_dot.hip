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
#include <type_traits>

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
// (hq_dot_tile.hip holds a copy of inside() and of this function: the two must stay the same.)
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
// WIN (DotWinArgs; hq_dot_population_partial on a shard): the class's pixels in the full-image
//   rows [a0, a1) -- rows y0 + j n.  The error planes hold those rows (row a0 first).  A source
//   must also lie in the window; its W is still the full image's (H is the image's).  The
//   pixel comes from the shard's planes (rows [e0, e1)) or the apron's (the rows around them);
//   only a row in [e0, e1) writes its index and its used bit.
// ----------------------------------------------------------------------------
template <bool WIN>
__global__ __launch_bounds__(256) void dot_kernel(std::conditional_t<WIN, DotWinArgs, DotArgs> a) {
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
        // (x, y): the position in the full image; yb, rows: the first row and the rows of the error planes
        const int x = a.cx + i * n;  // inside the image (the window) by nx, ny
        int y, yb, rows;
        if constexpr (WIN) y = a.y0 + j * n, yb = a.a0, rows = a.a1 - a.a0;
        else y = a.cy + j * n, yb = 0, rows = H;
        const int64_t plane = (int64_t)W * rows, q = (int64_t)(y - yb) * W + x;
        const float* err = a.err + (int64_t)p * 3 * plane;
        const uint32_t low = a.tab[a.cy * n + a.cx];
        float acc[3] = {0.f, 0.f, 0.f};
        for (int s = 0; s < 8; ++s) {
            const uint32_t d = low >> (4 * s) & 15u;
            if (d == kDotEnd) break;  // (uniform)
            const int dx = dot_dx((int)d), dy = dot_dy((int)d);
            const int px = x + dx, py = y + dy;
            if (!inside(px, py, W, H)) continue;
            if constexpr (WIN)
                if (py < a.a0 || py >= a.a1) continue;
            const uint32_t hi = a.tab[kDotCells + ((a.cy + dy) & (n - 1)) * n + ((a.cx + dx) & (n - 1))];
            const float wsum = (float)dot_weight_sum(hi, px, py, W, H);
            const float wt = (float)dot_weight((int)d);
            const int64_t src = (int64_t)(py - yb) * W + px;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const float prod = wt * err[ch * plane + src];
                acc[ch] = acc[ch] + prod / wsum;
            }
        }
        float pix[3];
        bool keep = true;  // this row's index and used bit are written
        if constexpr (WIN) {
            keep = y >= a.e0 && y < a.e1;
            // the apron's rows: those held above the shard's (from row h0), then those below
            const int64_t ap = ((int64_t)(y < a.e0 ? y - a.h0 : a.e0 - a.h0 + y - a.e1)) * W + x;
            const int64_t in = (int64_t)(y - a.e0) * W + x;
            pix[0] = *(keep ? a.R + in : a.aR + ap);  // (one address, one load)
            pix[1] = *(keep ? a.G + in : a.aG + ap);
            pix[2] = *(keep ? a.B + in : a.aB + ap);
        } else {
            pix[0] = a.R[q], pix[1] = a.G[q], pix[2] = a.B[q];
        }
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
        if constexpr (WIN) {
            if (keep) {
                a.idx[(int64_t)p * a.idx_pitch + (int64_t)(y - a.e0) * W + x] = (uint8_t)k;
                atomicOr(&s_used[k >> 5], 1u << (k & 31));
            }
        } else {
            a.idx[(int64_t)p * a.idx_pitch + q] = (uint8_t)k;
            atomicOr(&s_used[k >> 5], 1u << (k & 31));
        }
    }
    __syncthreads();
    if (tid < 8 && s_used[tid])
        atomicOr(&a.used_glob[(blockIdx.x & (kUsedSlots - 1)) * a.used_stride + p * 8 + tid], s_used[tid]);
}

namespace {

// What both launchers refuse, and the matrix's cells by class (cell_of[k] = cy n + cx).
bool dot_cells(const DotArgs& a, int P, int rows, int* cell_of) {
    const int n = a.n, cells = n * n;
    if ((n != 4 && n != 8 && n != 16) || a.K < 1 || a.K > kMaxK || a.W < 1 || rows < 1 || P < 1 || P > kDotMaxP ||
        !a.cls || !a.tab || !a.err || (int64_t)a.W * rows > INT32_MAX)  // (a class's pixel count fits an int)
        return false;
    for (int c = 0; c < cells; ++c) cell_of[c] = -1;
    for (int c = 0; c < cells; ++c) {
        if (a.cls[c] < 0 || a.cls[c] >= cells || cell_of[a.cls[c]] >= 0) return false;
        cell_of[a.cls[c]] = c;
    }
    return true;
}

// The launches of one call: the classes 0 .. n^2 - 1 in ascending order, each over the pixels
// place(args, cell) says it has (false: none, and no launch -- a zero-sized grid is an error).
// The pending profiling events bracket the whole chain: start on the first launch, stop on the
// last.
template <bool WIN, typename Args, typename Place>
hipError_t launch_classes(const Args& a0, const int* cell_of, int P, hipStream_t s, AssignTag* tag, Place&& place) {
    const int cells = a0.n * a0.n;
    Args a = a0;
    int first = -1, last = -1;
    for (int k = 0; k < cells; ++k)
        if (place(a, cell_of[k])) {
            if (first < 0) first = k;
            last = k;
        }
    const hipEvent_t start = t_ev_start, stop = t_ev_stop;
    for (int k = 0; k < cells; ++k) {
        if (!place(a, cell_of[k])) continue;
        t_ev_start = k == first ? start : nullptr;
        t_ev_stop = k == last ? stop : nullptr;
        HQ_LAUNCH(dot_kernel<WIN>, dim3(blocks_for((int64_t)a.nx * a.ny), P), dim3(256), 0, s, a);
    }
    t_ev_start = start, t_ev_stop = stop;
    // hq.h's hq_path_argmin: HQ_ARGMIN_DOT (the planar floats, always)
    if (tag) *tag = AssignTag{7, 0, 0, 0};
    return hipGetLastError();
}

}  // namespace

// The whole image: cell (cx, cy) has a pixel when cx < W and cy < H (else the image is smaller
// than the tile).
hipError_t launch_dot(const DotArgs& a0, int P, hipStream_t s, AssignTag* tag) {
    int cell_of[kDotCells];
    if (!dot_cells(a0, P, a0.H, cell_of)) return hipErrorInvalidValue;
    return launch_classes<false>(a0, cell_of, P, s, tag, [](DotArgs& a, int cell) {
        const int n = a.n;
        a.cx = cell % n, a.cy = cell / n;
        if (a.cx >= a.W || a.cy >= a.H) return false;
        a.nx = (a.W - a.cx + n - 1) / n, a.ny = (a.H - a.cy + n - 1) / n;
        return true;
    });
}

// A window: cell (cx, cy)'s rows are the full-image rows y = cy (mod n) of [a0, a1) -- a0 is
// generally no multiple of n, so y0 is counted from it.
hipError_t launch_dot_window(const DotWinArgs& a0, int P, hipStream_t s, AssignTag* tag) {
    int cell_of[kDotCells];
    if (!(0 <= a0.a0 && a0.a0 <= a0.e0 && a0.e0 < a0.e1 && a0.e1 <= a0.a1 && a0.a1 <= a0.H) ||
        !(a0.h0 <= a0.a0 && a0.a1 <= a0.h1) ||  // (the window's rows are held)
        ((a0.a0 < a0.e0 || a0.e1 < a0.a1) && (!a0.aR || !a0.aG || !a0.aB)) ||
        !dot_cells(a0, P, a0.a1 - a0.a0, cell_of))
        return hipErrorInvalidValue;
    return launch_classes<true>(a0, cell_of, P, s, tag, [](DotWinArgs& a, int cell) {
        const int n = a.n;
        a.cx = cell % n, a.cy = cell / n;
        a.y0 = a.a0 + ((a.cy - a.a0) % n + n) % n;
        if (a.cx >= a.W || a.y0 >= a.a1) return false;
        a.nx = (a.W - a.cx + n - 1) / n, a.ny = (a.a1 - a.y0 + n - 1) / n;
        return true;
    });
}

}  // namespace hq
