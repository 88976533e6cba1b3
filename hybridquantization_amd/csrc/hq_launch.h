// hq_launch.h -- host side of the kernel launchers: their prototypes (for the
// .hip file that defines each and the runtime that calls them), the runtime
// value -> template argument dispatch and the launch events they share.  Not
// part of the public ABI (include/hq.h).  Table builders: hq_cost_layout.h.
#pragma once

#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <type_traits>

#include "hq_internal.h"

namespace hq {

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + 255) / 256); }

// ---- runtime value -> compile-time tag ---------------------------------------
// Each helper calls f (a generic lambda) with a tag for the value; f names its
// kernel with `tag.value` / `typename decltype(tag)::type` as template argument.

// The dE types with kernels (the DE template argument: hq_delta_e's values 0
// CIE76, 1 CIE94, 2 CIEDE2000).  Every launcher that takes a `de` refuses any
// other value before with_de, so none can fall into its last arm.
inline bool known_de(int de) { return de >= 0 && de <= 2; }
template <typename F>
inline void with_de(int de, F&& f) {
    if (de == 0) f(std::integral_constant<int, 0>{});
    else if (de == 1) f(std::integral_constant<int, 1>{});
    else f(std::integral_constant<int, 2>{});
}
template <typename F>
inline void with_bool(bool b, F&& f) {
    if (b) f(std::true_type{});
    else f(std::false_type{});
}
// No mask (0), a pixel mask (1) or pixel weights (2): the MSK template argument.
template <typename F>
inline void with_mask(bool mask, bool weighted, F&& f) {
    if (!mask) f(std::integral_constant<int, 0>{});
    else if (!weighted) f(std::integral_constant<int, 1>{});
    else f(std::integral_constant<int, 2>{});
}
// Palette index width: 1 byte, 2 (chunked palettes) or 4 (K > 4096).
template <typename T>
struct type_tag { using type = T; };
template <typename F>
inline void with_idx(int idx_bytes, F&& f) {
    if (idx_bytes == 4) f(type_tag<uint32_t>{});
    else if (idx_bytes == 2) f(type_tag<uint16_t>{});
    else f(type_tag<uint8_t>{});
}

// ---- launch events and the LDS grant (hq_runtime.hip) --------------------------
// Profiling: the next launches carry start/stop events in their dispatch packet
// (hipExtLaunchKernel), so timing a kernel adds no marker packet between kernels
// (each hipEventRecord between two kernels left the GPU idle ~5 us).  Set by
// set_launch_events, read by HQ_LAUNCH in every launcher.
extern thread_local hipEvent_t t_ev_start, t_ev_stop;
void set_launch_events(hipEvent_t start, hipEvent_t stop);

// A launcher of two kernels: the pending events bracket the pair, start on the
// first launch, stop on the second (after second()); leaving scope puts the
// pending pair back, whichever return is taken.
class LaunchEventPair {
    const hipEvent_t start_ = t_ev_start, stop_ = t_ev_stop;

public:
    LaunchEventPair() { t_ev_stop = nullptr; }
    void second() { t_ev_start = nullptr, t_ev_stop = stop_; }
    ~LaunchEventPair() { t_ev_start = start_, t_ev_stop = stop_; }
};

// Dynamic LDS of `bytes` for kernel `fn` (static + dynamic may pass 64 KiB, up to
// the CU's 160 KiB on gfx950): raised once per kernel (each template instance is
// its own function; the largest size granted so far is kept per function
// pointer, a refused raise is retried at the next call).  False if the runtime
// refused it: the launcher then returns an error instead of launching.
bool allow_dyn_lds(const void* fn, size_t bytes);

#define HQ_LAUNCH(K, G, B, S, STREAM, ...)                                                   \
    do {                                                                                     \
        if (t_ev_start || t_ev_stop)                                                         \
            hipExtLaunchKernelGGL(K, G, B, S, STREAM, t_ev_start, t_ev_stop, 0, __VA_ARGS__); \
        else                                                                                 \
            hipLaunchKernelGGL(K, G, B, S, STREAM, __VA_ARGS__);                             \
    } while (0)

// HQ_LAUNCH of kernel K with S bytes of dynamic LDS that may pass 64 KiB: the
// grant first; refused, nothing is launched and the runtime's error stands for
// the launcher's hipGetLastError.
#define HQ_LAUNCH_DYN_LDS(K, G, B, S, STREAM, ...)                                                          \
    do {                                                                                                    \
        if (allow_dyn_lds(reinterpret_cast<const void*>(K), S)) HQ_LAUNCH(K, G, B, S, STREAM, __VA_ARGS__); \
    } while (0)

// ---- what a launcher chose (hq_last_path) ---------------------------------------
// Each launcher with a choice to make fills its tag next to the HQ_LAUNCH that makes
// it, through an out-parameter (null: nobody asks).  The values are hq.h's
// hq_path_argmin / hq_path_cost / hq_path_gen_h / hq_path_gen_v.
struct AssignTag { int kernel = 0, u8 = 0, cmb = 0, passes = 0; };
struct CostTag { int kernel = 0, hb = 0, de = 0, trim = 0, waves = 0, nch = 0, msk = 0; };
struct GenTag { int cost = 0, h = 0, h_outputs = 0, h_split = 0, h_rpt = 0, v = 0, v_rows = 0; };

// ---- the launchers -------------------------------------------------------------
// hq_search.hip
hipError_t launch_prep_palette(const PaletteArgs&, int P, hipStream_t);
hipError_t launch_sa_step(const SaArgs&, hipStream_t);
hipError_t launch_lloyd_update(const LloydArgs&, int P, hipStream_t);
hipError_t launch_reseed(const ReseedArgs&, int P, hipStream_t);
hipError_t launch_build_grid(const GridArgs&, int P, hipStream_t);
hipError_t launch_finalize(const FinalizeArgs&, int P, hipStream_t);
// hq_assign.hip
hipError_t launch_assign(const AssignArgs&, int P, hipStream_t, AssignTag* tag = nullptr);
void launch_used_idx16(const AssignArgs&, int P, hipStream_t);
int assign_residency(int NG);
int assign_residency_chunked();
// ... with ordered dithering (AssignArgs::map and what goes with it; K <= 256)
hipError_t launch_assign_ordered(const AssignArgs&, int P, hipStream_t, AssignTag* tag = nullptr);
int assign_residency_ordered(int NG);
// hq_lists16.hip
hipError_t launch_lists16_grid(const Lists16Args&, int P, hipStream_t);
hipError_t launch_assign16(const AssignArgs&, int P, hipStream_t, AssignTag* tag = nullptr);
// hq_wide.hip
hipError_t launch_prep_wide(const WideArgs&, int P, hipStream_t);
hipError_t launch_assign_wide(const WideArgs&, int P, hipStream_t, AssignTag* tag = nullptr);
// hq_cost.hip: half-widths up to 24
size_t fast_taps_bytes(int HB);
int fast_grid_row0(int de, int r0, int tile_rows);
void fast_tile_dims(int W, int own_rows, int tile_rows, int tile_w, int* tiles_x, int* ntiles);
int fast_tile_width(int tile_rows, int tile_w);  // columns of a tile of fast_tile_dims' grid
hipError_t launch_cost_fast(const CostArgs&, int P, int de, bool trim, int tile_rows, int tile_w, int HB,
                            hipStream_t, CostTag* tag = nullptr);
hipError_t launch_cost_chunked(const CostArgs&, int P, int nch, int de, bool trim, hipStream_t,
    CostTag* tag = nullptr);
// hq_cost_masked.hip: the same under a pixel mask (CostArgs::mask, live, nlive: nlive >= 1 tiles)
hipError_t launch_cost_fast_masked(const CostArgs&, int P, int de, bool trim, int tile_rows, int tile_w, int HB,
                                   hipStream_t, CostTag* tag = nullptr);
hipError_t launch_cost_chunked_masked(const CostArgs&, int P, int nch, int de, bool trim, hipStream_t,
    CostTag* tag = nullptr);
// hq_cost_weighted.hip: the same under pixel weights (CostArgs::mask holds the weights)
hipError_t launch_cost_fast_weighted(const CostArgs&, int P, int de, bool trim, int tile_rows, int tile_w, int HB,
                                     hipStream_t, CostTag* tag = nullptr);
hipError_t launch_cost_chunked_weighted(const CostArgs&, int P, int nch, int de, bool trim, hipStream_t,
    CostTag* tag = nullptr);
// hq_cost_generic.hip: any half-width, one palette per launch pair
hipError_t launch_cost_generic(const GenArgs&, int de, int idx_bytes, hipStream_t, GenTag* tag = nullptr);
hipError_t launch_cost_tiled_generic(const GenArgs&, int de, int idx_bytes, hipStream_t, GenTag* tag = nullptr);
// hq_centroid.hip: per-colour pixel sums; idx_bytes 1, 2 or 4, num_cu sizes the grid
hipError_t launch_cluster_sums(const ClusterArgs&, int idx_bytes, int num_cu, hipStream_t);
// hq_errsum.hip: per-colour error sums and worst pixels, then the gather of their colours
hipError_t launch_cluster_errors(const ClusterErrArgs&, int idx_bytes, int num_cu, hipStream_t);
// hq_hist.hip: the colour histogram of the owned rows; num_cu sizes the grid
hipError_t launch_color_histogram(const HistArgs&, int num_cu, hipStream_t);
// hq_reduce.hip: the box reduction of a whole image (the packed form when a.rgbx, else the planar one)
hipError_t launch_reduce_image(const ReduceArgs&, hipStream_t);
// hq_argspace.hip: the argmin coordinates (option "assign_space") of the extended rows, and of a list of colours
hipError_t launch_coords(const CoordArgs&, hipStream_t);
hipError_t launch_coords_list(const float4* in, float4* out, int64_t n, int space, const float inv_illum[3],
                              hipStream_t);
// hq_setup.hip
hipError_t launch_pack_u8(const float*, const float*, const float*, uint32_t*, int*, int64_t, hipStream_t);
hipError_t launch_labref_opp(const float*, const float*, const float*, float4*, int64_t, hipStream_t);
hipError_t launch_xyz_to_opp(const float4*, float4*, int64_t, hipStream_t);
hipError_t launch_rgb_to_xyz(const float*, const float*, const float*, float4*, int64_t, hipStream_t);
hipError_t launch_labref_hconv(const float4*, float4*, const float*, int, int, int, int64_t, hipStream_t);
hipError_t launch_labref_vconv(const float4*, float4*, const float*, int, int, int, const Geom&, hipStream_t);
hipError_t launch_labref_lab(const float4*, float*, float*, float*, float4*, int, int64_t, int,
                             const float*, hipStream_t);
hipError_t launch_lab_to_planar(const float4*, float*, float*, float*, int, int64_t, int, hipStream_t);
hipError_t launch_quantize(const float4*, const float4*, int, int*, float4*, int64_t, hipStream_t);
hipError_t launch_error_image(const float4*, const float4*, float4*, double*, int64_t, int, hipStream_t);

}  // namespace hq
