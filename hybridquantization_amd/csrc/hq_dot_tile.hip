// hq_dot_tile.hip -- dot diffusion's tiled form (hq.h: option "dot_tile"): the
// index images of hq_dot.hip's chain of launches, bit for bit, in one launch.
//
// idx(q) depends only on the pixels a path of neighbour steps with strictly descending class
// reaches from q, and such a path gets no further than the matrix's reach in each of the four
// directions (hq_dot_reach2).  A workgroup therefore renders a tile from the window that extends
// it by the reach on every side, clipped to the image: inside the window a pixel near its edge may
// miss sources and come out wrong, but no path from a pixel of the tile leaves the window, so the
// tile's own pixels are the whole image's.  The window's errors live in LDS alone.
//
// The definition is hq_dot.hip's, operation for operation: classes from full-image coordinates,
// W(p)'s border rule from the full image's W and H, a source outside the window contributing
// nothing and never read, the sources added in ascending class from +0, one fp32 operation per
// step, none contracted.
//
// Inside the window the order is by level (hq_dot_levels), not by class: a pixel's sources all
// have lower levels, so the pixels of one level are independent and a barrier separates the
// levels.  Every pixel still gathers its own sources in ascending class, so the schedule does not
// change a bit.
#include "hq_device.h"
#define HQ_DIFFUSE_DEVICE
#include "hq_diffuse.h"
#include "hq_dot.h"

namespace hq {

namespace {

__device__ __forceinline__ bool inside(int x, int y, int W, int H) {
    return (unsigned)x < (unsigned)W && (unsigned)y < (unsigned)H;
}

// W(p) as dot_kernel takes it: inside() and dot_weight_sum() are hq_dot.hip's, copied so that that
// unit stays as it is.  The two copies define one W(p) and must stay the same, operation for
// operation; tests/test_dot_tile_gpu.py holds both kernels to one reference and to each other.
__device__ __forceinline__ int dot_weight_sum(uint32_t hi, int px, int py, int W, int H) {
    if (px >= 1 && px < W - 1 && py >= 1 && py < H - 1) return 2 * __popc(hi & kDotOrth) + __popc(hi & kDotDiag);
    int w = 0;
#pragma unroll
    for (int d = 0; d < 8; ++d)
        if ((hi >> d & 1u) && inside(px + dot_dx(d), py + dot_dy(d), W, H)) w += dot_weight(d);
    return w;
}

constexpr int kTileThreads = 256;

}  // namespace

// ----------------------------------------------------------------------------
// dot_tile_kernel: grid (tiles, P), block 256.  Tile t = ty tiles_x + tx covers the pixels
// [tx tw, tx tw + tw) x [ty th, ty th + th) of the image; its window adds the reach.
//   LDS: the palette, the two tables, the schedule's cells, and s_win[3][window]: a window pixel's
//   three planes hold its image value until it is rendered and its error afterwards (a source is
//   rendered before any pixel that reads it, and nobody else reads a pixel's own slot).  Within an
//   item every lane reads the slot's pixel value and lane 0 later overwrites it with the error,
//   with no barrier between: the item's lanes are adjacent lanes of one wave (kDotTileMaxLanes at
//   most, aligned), the read comes first in program order, and the LDS serves one wave's accesses
//   in order.
//   A level's work items are (cell of the level, row j, column i) over the grid of the window's
//   pixels of one cell, mx x my at most; an item past the window's edge does nothing.  Each item
//   takes 2^lg_lanes adjacent lanes: all of them gather v (the same operations, the same value),
//   each ranks the colours k = lane, lane + lanes, ... and a butterfly combines the lanes into
//   diffuse_argmin's answer:
//     best2    the smallest rank distance, the lowest index among equal ones;
//     second2  the second smallest of the multiset: min(max(best_a, best_b), second_a, second_b);
//     near_d2  then the first minimum of ref_dist over all K, the lanes combined by (distance,
//              index) -- the reference loop's result.
//   The shuffles run with every lane of the wave active: the item loop's trip count is uniform,
//   an idle item ranks nothing, and the re-resolution is entered on a wave-wide vote.
//   Lane 0 of the item writes the error and, for a pixel of the tile itself, the index and the
//   used bit.  No atomics on the errors, no scratch, no workgroup waits on another.
// ----------------------------------------------------------------------------
__global__ __launch_bounds__(kTileThreads) void dot_tile_kernel(DotTileArgs a) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) float4 s_pal[kMaxK];
    __shared__ uint32_t s_tab[2 * kDotCells];
    __shared__ uint32_t s_cell[kDotCells];
    __shared__ uint32_t s_used[8];
    extern __shared__ float s_win[];
    const int p = blockIdx.y, tid = threadIdx.x;
    const int W = a.W, H = a.H, K = a.K, n = a.n;
    const DotTilePlan& pl = a.plan;
    for (int k = tid; k < K; k += kTileThreads) s_pal[k] = a.pal[(int64_t)p * kMaxK + k];
    for (int i = tid; i < 2 * kDotCells; i += kTileThreads) s_tab[i] = a.tab[i];
    for (int i = tid; i < kDotCells; i += kTileThreads) s_cell[i] = a.sched[i];
    if (tid < 8) s_used[tid] = 0u;

    const int tiles_x = (W + pl.tw - 1) / pl.tw;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int x0 = tx * pl.tw, y0 = ty * pl.th;                          // the tile ...
    const int x1 = min(x0 + pl.tw, W), y1 = min(y0 + pl.th, H);
    const int wx0 = max(x0 - pl.left, 0), wy0 = max(y0 - pl.above, 0);   // ... and its window
    const int wx1 = min(x0 + pl.tw + pl.right, W), wy1 = min(y0 + pl.th + pl.below, H);
    const int ww = wx1 - wx0, wh = wy1 - wy0, wp = ww * wh;              // wp <= pl.window
    for (int i = tid; i < wp; i += kTileThreads) {
        const int yy = i / ww, xx = i - yy * ww;
        const int64_t q = (int64_t)(wy0 + yy) * W + wx0 + xx;
        s_win[i] = a.R[q], s_win[wp + i] = a.G[q], s_win[2 * wp + i] = a.B[q];
    }
    __syncthreads();

    const int lg = pl.lg_lanes, lanes = 1 << lg, sub = tid & (lanes - 1);
    const int mx = (ww + n - 1) / n, my = (wh + n - 1) / n, per = mx * my;
    const int lg_n = n == 4 ? 2 : n == 8 ? 3 : 4;
    for (int lvl = 0; lvl < pl.depth; ++lvl) {
        const int c0 = (int)a.sched[kDotCells + lvl], c1 = (int)a.sched[kDotCells + lvl + 1];
        const int items = (c1 - c0) * per;
        for (int base = 0; base < items; base += kTileThreads >> lg) {  // (uniform: every lane makes every trip)
            const int it = base + (tid >> lg);
            bool live = it < items;
            int x = 0, y = 0, cx = 0, cy = 0;
            if (live) {
                const int ci = it / per, r = it - ci * per;
                const int j = r / mx, i = r - j * mx;
                const int cell = (int)s_cell[c0 + ci];
                cx = cell & (n - 1), cy = cell >> lg_n;
                // the cell's first column and row in the window (wx0, wy0 are no multiples of n)
                x = wx0 + ((cx - wx0) & (n - 1)) + i * n;
                y = wy0 + ((cy - wy0) & (n - 1)) + j * n;
                live = x < wx1 && y < wy1;
            }
            float v[3] = {0.f, 0.f, 0.f};
            int wi = 0;
            if (live) {
                wi = (y - wy0) * ww + (x - wx0);
                const uint32_t low = s_tab[cy * n + cx];
                float acc[3] = {0.f, 0.f, 0.f};
                for (int s = 0; s < 8; ++s) {
                    const uint32_t d = low >> (4 * s) & 15u;
                    if (d == kDotEnd) break;
                    const int dx = dot_dx((int)d), dy = dot_dy((int)d);
                    const int px = x + dx, py = y + dy;
                    if (!inside(px, py, W, H)) continue;
                    if (px < wx0 || px >= wx1 || py < wy0 || py >= wy1) continue;
                    const uint32_t hi = s_tab[kDotCells + ((cy + dy) & (n - 1)) * n + ((cx + dx) & (n - 1))];
                    const float wsum = (float)dot_weight_sum(hi, px, py, W, H);
                    const float wt = (float)dot_weight((int)d);
                    const int src = (py - wy0) * ww + (px - wx0);
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) {
                        const float prod = wt * s_win[ch * wp + src];
                        acc[ch] = acc[ch] + prod / wsum;
                    }
                }
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    const float m = a.strength * acc[ch];
                    v[ch] = fminf(fmaxf(s_win[ch * wp + wi] + m, 0.0f), 1.0f);
                }
            }
            // this lane's colours, then the lanes of the item combined
            float best2 = INFINITY, second2 = INFINITY;
            int bi = live && sub < K ? sub : INT32_MAX;
            if (live) {
#pragma unroll 4
                for (int k = sub; k < K; k += lanes) {
                    const float d2 = dist2_rank(v[0], v[1], v[2], s_pal[k]);
                    const bool lt = d2 < best2;
                    bi = lt ? k : bi;
                    second2 = __builtin_amdgcn_fmed3f(best2, second2, d2);
                    best2 = lt ? d2 : best2;
                }
            }
            for (int m = lanes >> 1; m; m >>= 1) {
                const float ob = __shfl_xor(best2, m), os = __shfl_xor(second2, m);
                const int oi = __shfl_xor(bi, m);
                second2 = fminf(fmaxf(best2, ob), fminf(second2, os));
                const bool take = ob < best2 || (ob == best2 && oi < bi);
                bi = take ? oi : bi;
                best2 = take ? ob : best2;
            }
            const bool near = live && near_d2(best2, second2);
            if (__builtin_amdgcn_ballot_w64(near) != 0) {  // (wave-uniform: the shuffles below see every lane)
                float bd = INFINITY;
                int bk = INT32_MAX;
                if (near) {
                    for (int k = sub; k < K; k += lanes) {
                        const float d = ref_dist(v[0], v[1], v[2], s_pal[k]);
                        if (d < bd) { bd = d; bk = k; }
                    }
                }
                for (int m = lanes >> 1; m; m >>= 1) {
                    const float od = __shfl_xor(bd, m);
                    const int ok = __shfl_xor(bk, m);
                    const bool take = od < bd || (od == bd && ok < bk);
                    bk = take ? ok : bk;
                    bd = take ? od : bd;
                }
                if (near) bi = bk;
            }
            if (live && sub == 0) {
                const float4 c = s_pal[bi];
                s_win[wi] = v[0] - c.x;
                s_win[wp + wi] = v[1] - c.y;
                s_win[2 * wp + wi] = v[2] - c.z;
                if (x >= x0 && x < x1 && y >= y0 && y < y1) {
                    a.idx[(int64_t)p * a.idx_pitch + (int64_t)y * W + x] = (uint8_t)bi;
                    atomicOr(&s_used[bi >> 5], 1u << (bi & 31));
                }
            }
        }
        __syncthreads();
    }
    if (tid < 8 && s_used[tid])
        atomicOr(&a.used_glob[(blockIdx.x & (kUsedSlots - 1)) * a.used_stride + p * 8 + tid], s_used[tid]);
}

// One launch; the pending profiling events ride on it.  What it refuses is what the plan's maker
// (dot_tile_eligible) cannot have produced, and an image whose tiles do not fit a grid.
hipError_t launch_dot_tile(const DotTileArgs& a, int P, hipStream_t s, AssignTag* tag) {
    const DotTilePlan& pl = a.plan;
    if ((a.n != 4 && a.n != 8 && a.n != 16) || a.K < 1 || a.K > kMaxK || a.W < 1 || a.H < 1 || P < 1 || P > kDotMaxP ||
        !a.tab || !a.sched || pl.shape < 0 || pl.shape >= kDotTileShapes || pl.tw != kDotTileW[pl.shape] ||
        pl.th != kDotTileH[pl.shape] || pl.above < 0 || pl.below < 0 || pl.left < 0 || pl.right < 0 || pl.depth < 1 ||
        pl.depth > kDotCells || pl.lg_lanes < 0 || (1 << pl.lg_lanes) > kDotTileMaxLanes ||
        pl.window != (pl.tw + pl.left + pl.right) * (pl.th + pl.above + pl.below) ||
        (int64_t)pl.window * 12 > kDotTileErrBytes || (int64_t)a.W * a.H > INT32_MAX)
        return hipErrorInvalidValue;
    const int64_t tiles = (int64_t)((a.W + pl.tw - 1) / pl.tw) * ((a.H + pl.th - 1) / pl.th);
    if (tiles > INT32_MAX) return hipErrorInvalidValue;
    HQ_LAUNCH(dot_tile_kernel, dim3((unsigned)tiles, P), dim3(kTileThreads), sizeof(float) * 3 * pl.window, s, a);
    // hq.h's hq_path_argmin: HQ_ARGMIN_DOT (the planar floats, always), as the chain reports
    if (tag) *tag = AssignTag{7, 0, 0, 0};
    return hipGetLastError();
}

}  // namespace hq
