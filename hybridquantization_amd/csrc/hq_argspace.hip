// hq_argspace.hip -- option "assign_space": the coordinates the argmin ranks by when they are
// not the sRGB values themselves (libhq's own addition, no reference counterpart).  Under
// space 1 a colour's coordinates are its CIELAB under the context's illuminant, scaled into the
// unit cube (assign_coord_lab, hq_device.h).  The argmin kernels do not change: the runtime
// hands them these planes in the place of R/G/B and the palette prep's `arg` table in the
// place of `pal` (hq_search.hip).
//
//  coords_kernel<U8>     the extended rows' pixels, from the packed 8-bit copy (u8_unit gives
//                        the k/255 the planar image holds) or the planar floats, into three
//                        planes of the same length and padding;
//  coords_list_kernel    n colours given as float4s (hq_assign_coords), space 0 the identity.
//
// Both are streaming kernels: no LDS, no atomics.  A thread of coords_kernel takes one quad of
// four pixels: one 16-byte load per source plane (or one for the packed words) and one 16-byte
// store per coordinate plane -- the planes start 16-byte aligned and are padded to whole quads.
// As in hq_reduce.hip a thread's one step is its whole work: the grid has a thread per quad and
// there is no stride loop (an image is below 2^30 pixels, check_geom_args, so below 2^28 quads
// and 2^20 workgroups; launch_coords refuses more).  The kernel runs once per image.
#include "hq_device.h"
#include "hq_launch.h"

namespace hq {

template <bool U8>
__global__ __launch_bounds__(256) void coords_kernel(CoordArgs a) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= a.quads) return;
    float r[4], g[4], b[4];
    if constexpr (U8) {
        const uint4 v = reinterpret_cast<const uint4*>(a.rgbx)[q];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = u8_unit(w[j], 0), g[j] = u8_unit(w[j], 1), b[j] = u8_unit(w[j], 2);
    } else {
        const float4 vr = reinterpret_cast<const float4*>(a.R)[q];
        const float4 vg = reinterpret_cast<const float4*>(a.G)[q];
        const float4 vb = reinterpret_cast<const float4*>(a.B)[q];
        r[0] = vr.x, r[1] = vr.y, r[2] = vr.z, r[3] = vr.w;
        g[0] = vg.x, g[1] = vg.y, g[2] = vg.z, g[3] = vg.w;
        b[0] = vb.x, b[1] = vb.y, b[2] = vb.z, b[3] = vb.w;
    }
    float o[3][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float3 c = assign_coord_lab(srgb_lin(r[j]), srgb_lin(g[j]), srgb_lin(b[j]), a.inv_illum);
        const bool in = 4 * q + j < a.n_ext;  // (the padding of the last quad reads as zero)
        o[0][j] = in ? c.x : 0.f, o[1][j] = in ? c.y : 0.f, o[2][j] = in ? c.z : 0.f;
    }
    reinterpret_cast<float4*>(a.oR)[q] = make_float4(o[0][0], o[0][1], o[0][2], o[0][3]);
    reinterpret_cast<float4*>(a.oG)[q] = make_float4(o[1][0], o[1][1], o[1][2], o[1][3]);
    reinterpret_cast<float4*>(a.oB)[q] = make_float4(o[2][0], o[2][1], o[2][2], o[2][3]);
}

__global__ __launch_bounds__(256) void coords_list_kernel(const float4* in, float4* out, int64_t n, int space,
                                                          CoordArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float4 c = in[i];
    float3 o = make_float3(c.x, c.y, c.z);
    if (space != 0) o = assign_coord_lab(srgb_lin(c.x), srgb_lin(c.y), srgb_lin(c.z), a.inv_illum);
    out[i] = make_float4(o.x, o.y, o.z, 0.f);
}

hipError_t launch_coords(const CoordArgs& a, hipStream_t s) {
    if (a.quads < 1 || a.quads > ((int64_t)1 << 30) || a.n_ext > 4 * a.quads) return hipErrorInvalidValue;
    if (a.rgbx) HQ_LAUNCH(coords_kernel<true>, dim3(blocks_for(a.quads)), dim3(256), 0, s, a);
    else HQ_LAUNCH(coords_kernel<false>, dim3(blocks_for(a.quads)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_coords_list(const float4* in, float4* out, int64_t n, int space, const float inv_illum[3],
                              hipStream_t s) {
    if (n < 1) return hipErrorInvalidValue;
    CoordArgs a{};
    for (int i = 0; i < 3; ++i) a.inv_illum[i] = inv_illum[i];
    HQ_LAUNCH(coords_list_kernel, dim3(blocks_for(n)), dim3(256), 0, s, in, out, n, space, a);
    return hipGetLastError();
}

}  // namespace hq
