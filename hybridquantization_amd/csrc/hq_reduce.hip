// hq_reduce.hip -- the box reduction of a context's image by an integer factor, on the
// device (hq_set_image_reduced: the image pyramid of a coarse-to-fine search; libhq's own
// addition, no reference counterpart).  Two kernels, one per form of the source image:
//
//  reduce_u8_kernel      the packed 8-bit copy (R | G << 8 | B << 16 per pixel): per channel
//                        the integer sum s of the block's n bytes, the byte floor((2 s + n) /
//                        (2 n)) -- round half up -- and the float u8_unit makes of it, so the
//                        reduced image is on the k/255 lattice again and keeps a packed copy;
//  reduce_planar_kernel  the planar floats: the fp32 sum of the block in raster order (rows
//                        outer, columns inner) starting from its first pixel, then one
//                        correctly rounded division by (float)n.
//
// Both are streaming kernels: no LDS, no atomics.  A thread makes kOut = 4 horizontally
// adjacent output pixels of one output row, so per source row it reads 4 f consecutive
// elements: f 16-byte loads when that span lies inside the row and starts 16-byte aligned
// (the row's start is, when y W is a multiple of 4), else dwords under the column bound.
// The output goes out as one 16-byte store per plane under the same rule.  The factor is
// a template argument (1 .. kMaxReduce), so every loop over a block's columns is unrolled
// and the accumulators stay in registers.
#include <type_traits>

#include "hq_device.h"
#include "hq_launch.h"

namespace hq {

namespace {

constexpr int kOut = 4;  // output pixels per thread

template <typename T>
struct alignas(16) Quad {
    T v[4];
};

// Elements [c0, c0 + 4 F) of a source row into v, zero past column W; true when the whole span
// lies inside the row (then every output of the thread has all F columns).
template <int F, typename T>
__device__ __forceinline__ bool load_span(const T* row, int c0, int W, T (&v)[kOut * F]) {
    const T* p = row + c0;
    const bool whole = c0 + kOut * F <= W;
    if (whole && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
#pragma unroll
        for (int j = 0; j < F; ++j) {
            const Quad<T> q = reinterpret_cast<const Quad<T>*>(p)[j];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[4 * j + e] = q.v[e];
        }
    } else {
#pragma unroll
        for (int i = 0; i < kOut * F; ++i) v[i] = c0 + i < W ? p[i] : T(0);
    }
    return whole;
}

// Outputs X0 .. X0 + 3 of a reduced row (those below rw): one 16-byte store when aligned.
__device__ __forceinline__ void store_span(float* row, int X0, int rw, const float (&o)[kOut]) {
    float* p = row + X0;
    if (X0 + kOut <= rw && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
        *reinterpret_cast<Quad<float>*>(p) = Quad<float>{{o[0], o[1], o[2], o[3]}};
    } else {
#pragma unroll
        for (int j = 0; j < kOut; ++j)
            if (X0 + j < rw) p[j] = o[j];
    }
}

// The thread's place: output row Y, first output column X0; false past the reduced image.
__device__ __forceinline__ bool reduce_place(const ReduceArgs& a, int* X0, int* Y) {
    const int gx = (a.rw + kOut - 1) / kOut;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)gx * a.rh) return false;
    *Y = (int)(t / gx);
    *X0 = (int)(t % gx) * kOut;
    return true;
}

// columns of output j's block that exist: F, fewer at the right edge, 0 past it
template <int F>
__device__ __forceinline__ int block_cols(int c0, int j, int W) {
    return min(max(W - (c0 + j * F), 0), F);
}

}  // namespace

template <int F>
__global__ __launch_bounds__(256) void reduce_u8_kernel(ReduceArgs a) {
    int X0, Y;
    if (!reduce_place(a, &X0, &Y)) return;
    const int c0 = X0 * F, y0 = Y * F, ny = min(F, a.H - y0);
    // per output: R and B in the two 16-bit halves of one word, G in another (a block's sum of
    // at most 256 bytes is at most 65280)
    uint32_t rb[kOut] = {0u, 0u, 0u, 0u}, gg[kOut] = {0u, 0u, 0u, 0u};
#pragma unroll 1
    for (int dy = 0; dy < ny; ++dy) {
        uint32_t v[kOut * F];
        (void)load_span<F>(a.rgbx + (int64_t)(y0 + dy) * a.W, c0, a.W, v);  // (past W: zeros, which add nothing)
#pragma unroll
        for (int i = 0; i < kOut * F; ++i) {
            rb[i / F] += v[i] & 0x00ff00ffu;
            gg[i / F] += (v[i] >> 8) & 0xffu;
        }
    }
    float o[3][kOut];
#pragma unroll
    for (int j = 0; j < kOut; ++j) {
        const uint32_t n = (uint32_t)(max(block_cols<F>(c0, j, a.W), 1) * ny);
        const uint32_t s[3] = {rb[j] & 0xffffu, gg[j], rb[j] >> 16};
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            // round half up; a whole block's divisor is a constant
            const uint32_t b = n == (uint32_t)(F * F) ? (2u * s[ch] + F * F) / (2u * F * F) : (2u * s[ch] + n) / (2u * n);
            o[ch][j] = u8_unit(b, 0);
        }
    }
    const int64_t orow = (int64_t)Y * a.rw;
    store_span(a.oR + orow, X0, a.rw, o[0]);
    store_span(a.oG + orow, X0, a.rw, o[1]);
    store_span(a.oB + orow, X0, a.rw, o[2]);
}

template <int F>
__global__ __launch_bounds__(256) void reduce_planar_kernel(ReduceArgs a) {
    int X0, Y;
    if (!reduce_place(a, &X0, &Y)) return;
    const int c0 = X0 * F, y0 = Y * F, ny = min(F, a.H - y0);
    int nx[kOut];
#pragma unroll
    for (int j = 0; j < kOut; ++j) nx[j] = block_cols<F>(c0, j, a.W);
    const float* const src[3] = {a.R, a.G, a.B};
    float* const dst[3] = {a.oR, a.oG, a.oB};
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        float acc[kOut] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
        for (int dy = 0; dy < ny; ++dy) {
            float v[kOut * F];
            const bool whole = load_span<F>(src[ch] + (int64_t)(y0 + dy) * a.W, c0, a.W, v);
            // raster order: this row's columns left to right, onto the rows above; the sum
            // starts from the block's first pixel, not from zero
#pragma unroll
            for (int i = 0; i < kOut * F; ++i) {
                const int j = i / F, dx = i % F;
                if (dx == 0) acc[j] = dy == 0 ? v[i] : acc[j] + v[i];
                else if (whole || dx < nx[j]) acc[j] = acc[j] + v[i];
            }
        }
        float o[kOut];
#pragma unroll
        for (int j = 0; j < kOut; ++j) o[j] = __fdiv_rn(acc[j], (float)(max(nx[j], 1) * ny));
        store_span(dst[ch] + (int64_t)Y * a.rw, X0, a.rw, o);
    }
}

namespace {

// f -> the template argument F, 1 .. kMaxReduce (the caller has checked the range)
template <int F = 1, typename Fn>
void with_factor(int f, Fn&& fn) {
    if (f == F) fn(std::integral_constant<int, F>{});
    else if constexpr (F < kMaxReduce) with_factor<F + 1>(f, fn);
}

}  // namespace

hipError_t launch_reduce_image(const ReduceArgs& a, hipStream_t s) {
    if (a.factor < 1 || a.factor > kMaxReduce || a.rw < 1 || a.rh < 1) return hipErrorInvalidValue;
    const int64_t threads = (int64_t)((a.rw + kOut - 1) / kOut) * a.rh;
    with_factor(a.factor, [&](auto F) {
        if (a.rgbx) HQ_LAUNCH(reduce_u8_kernel<F.value>, dim3(blocks_for(threads)), dim3(256), 0, s, a);
        else HQ_LAUNCH(reduce_planar_kernel<F.value>, dim3(blocks_for(threads)), dim3(256), 0, s, a);
    });
    return hipGetLastError();
}

}  // namespace hq
