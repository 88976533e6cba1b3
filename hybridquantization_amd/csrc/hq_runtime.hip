// hq_runtime.hip -- libhq host runtime: the C ABI of include/hq.h.
//
// One hq_ctx = one GPU, one HIP stream (the reference's single in-order queue,
// IM:58-59), the device-resident image of IM:450-478 (planar RGB of the owned
// rows +- halo, planar LabRef of the owned rows), per-population work buffers,
// and optionally an RCCL communicator for row-block sharding.
#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "hq_launch.h"
#include "hq_swasa.h"

#ifndef HQ_COST_TW
#define HQ_COST_TW 128
#endif
#ifndef HQ_SA_GRAPH
#define HQ_SA_GRAPH 0  // (measured slower: C3 0.528 -> 0.540 ms, shard-of-8 0.1035 -> 0.110 ms per step)
#endif

namespace hq {  // launch state shared by every launcher (hq_launch.h)
thread_local hipEvent_t t_ev_start = nullptr, t_ev_stop = nullptr;

void set_launch_events(hipEvent_t start, hipEvent_t stop) {
    t_ev_start = start;
    t_ev_stop = stop;
}

bool allow_dyn_lds(const void* fn, size_t bytes) {
    static std::mutex mu;
    static std::unordered_map<const void*, size_t> granted;
    const std::lock_guard<std::mutex> lock(mu);
    size_t& g = granted[fn];
    if (bytes <= g) return true;
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) return false;
    g = bytes;
    return true;
}
}  // namespace hq

using namespace hq;

namespace {

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    hipError_t ensure(size_t n) {
        if (n <= bytes) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
        hipError_t e = hipMalloc(&p, n);
        if (e == hipSuccess) bytes = n;
        return e;
    }
    hipError_t upload(const void* src, size_t n) {  // ensure(n), then a blocking copy from the host
        const hipError_t e = ensure(n);
        return e != hipSuccess ? e : hipMemcpy(p, src, n, hipMemcpyHostToDevice);
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    template <typename T>
    T* as() const { return static_cast<T*>(p); }
};

struct ProfSlot {
    double ms = 0.0;
    int64_t launches = 0;
};

// Profiling events per evaluation / search iteration: start, stop of grid (0,
// 1), assign (2, 3), cost (4, 5), finalize (6, 7), sa_step (8, 9) and the
// collective (10, 11), and of hq_cluster_sums' centroid kernel (12, 13).
constexpr int kProfEvents = 14;
// A search iteration has those and, when it is a hybrid iteration, the pairs of
// its assign-only pass (grid 14, 15; assign 16, 17: enqueue_core's slots 0 .. 3
// shifted by kProfLloyd), the sums kernel (18, 19) and the update kernel (20, 21).
constexpr int kProfLloyd = kProfEvents;
// ... and, when it is a repair iteration, the pairs of its error pass (grid 22, 23; assign 24,
// 25; cost 26, 27: enqueue_core's slots 0 .. 5 shifted by kProfRepair), the error kernels
// (28, 29) and the reseed kernel (30, 31).
constexpr int kProfRepair = kProfLloyd + 8;
constexpr int kProfSearchEvents = kProfRepair + 10;

}  // namespace

struct hq_ctx {
    int device = 0;
    int de_type = HQ_DE_CIE76;
    hipStream_t stream = nullptr;
    std::string err;

    // filters (IM:800-841)
    int taps = 0, half = 0;
    std::vector<float> k1, k2, k3, absk3;
    DevBuf d_k1, d_k2, d_k3, d_absk3;
    DevBuf d_vtaps;    // tiled generic path: [7][vtap_pitch] vertical taps per plane, zero-padded
    int vtap_pitch = 0;
    int fast_hb = 0;   // fast path tap bucket (fast_bucket(half)); 0 = generic path only
    DevBuf d_taps;     // fast path taps, build_fast_taps (the filters centred in the bucket)
    DevBuf d_vfrag16;  // split-f16 MFMA A fragments of the stacked vertical taps
    DevBuf d_vfrag16p; // the same in cost16w's (hi, lo) pair layout
    DevBuf d_vfragm;   // the tiled generic path's matrix-core vertical taps (build_vtile_dup_taps)
    DevBuf d_htaps;    // gen_hrow4's packed horizontal taps [T][2] float4

    // image
    bool have_image = false;
    Geom g{};
    float illum[3] = {0.95047f, 1.0f, 1.0883f};
    DevBuf d_R, d_G, d_B;          // planar, extended rows (n_ext, padded to 4)
    DevBuf d_rgbx;                 // packed 8-bit copy of R,G,B when every channel is k/255
    bool img_u8 = false;
    DevBuf d_labL, d_labA, d_labB;  // planar LabRef, owned rows, lab_pitch

    // population work buffers
    int P_cap = 0, K_cur = 0;
    DevBuf d_pal_in, d_pal, d_opp, d_opp16, d_dup, d_pflags, d_lvl1, d_lvl2, d_idx, d_used_mask,
        d_acc, d_out, d_gen_t;
    // d_acc: two sets of fixed-point dE sums [kAccSlots][P][4] u64 (acc_add), d_used_mask two
    // sets of used bits [kUsedSlots][used_stride]; evaluation n fills set acc_par = n & 1
    int acc_par = 0;
    DevBuf d_pixerr;           // option "pixel_err": [P][n_own] per-pixel dE of the last evaluation
    DevBuf d_idx32, d_used32;  // K > 16384 (hq_wide.hip): 32-bit index images, per-colour used flags
    DevBuf d_idx16, d_dist;    // 256 < K <= 16384 (chunked): 16-bit index images, pass distances
    DevBuf d_l1n, d_l2n;       // the native 16-bit candidate lists (hq_lists16.hip)
    int nch_cur = 1;           // chunks per palette of the population being enqueued (1: K <= 256)
    int last_nch = 1;          // ... of the last evaluation (its index image: u16 when > 1)
    float* h_pal = nullptr;   // pinned [P][K][4]
    double* h_out = nullptr;  // pinned [P][1+K]
    size_t h_pal_bytes = 0, h_out_bytes = 0;
    int last_P = 0;
    // hq_cluster_sums: the index images on the device are those of a population of last_P x
    // K_cur evaluated by hq_eval_population[_partial] (a search run or a new image unsets it)
    bool sums_ok = false;
    DevBuf d_sums;             // [P][K][4] int64 sums, then the planar form's range flag
    // hybrid iterations: every owned pixel of the planar image is finite and in [0, 1], the
    // condition of the planar form's sums (-1: not established yet for this image)
    int planar_ok = -1;
    DevBuf d_hist;             // hq_color_histogram: [2^(3 bits)][4] int64 cells, then the range flag
    // hq_cluster_errors: the error image on the device is that of the last evaluation (option
    // "pixel_err" was on when hq_eval_population[_partial] enqueued it; read with sums_ok)
    bool err_ok = false;
    DevBuf d_errstat, d_worst; // [P][K][4] u64 statistics, then the flag; [P][K] float4 worst pixels
    DevBuf d_dcarry;           // hq_dither_population: [P][3][W] errors of a strip's last row

    // options
    int G2 = 32;           // argmin grid resolution (0 = exhaustive)
    int cost_variant = 0;  // 0 fast tiled (default), 1 generic two-pass (LDS-tiled), 2 the generic
                           // pair per pixel in the reference's summation order
    int cost_rows = 16;    // fast path tiles: 16 x 128 (cost16w_kernel) or 8 x 108 (cost_mfma_kernel)
    int cost_tw = HQ_COST_TW;  // 16-row tiles at HB = 10: 128 (4 waves) or 256 columns (8 waves; slower)
    int gen_hrow4 = 1;     // tiled generic path: 4 outputs per thread in the horizontal pass
    int gen_vtile2 = 1;    // tiled generic path: double-buffered LDS-DMA vertical pass (half <= 64)
    int gen_vmfma = 1;     // tiled generic path: the vertical pass on the matrix cores (half <= 64)
    int gen_hmfma = 1;     // ... and the horizontal pass (gen_hmfma) with it
    int gen_shape = 0;     // their tile shapes: 0 by grid size, 1 short, 2 tall (option gen_tile_shape)
    int gen_hrow_no = 4;   // tiled generic path: horizontal outputs per thread (4 or 8)
    int sa_graph = HQ_SA_GRAPH;  // device-resident search: each run's kernels as one hipGraph
    int assign_blocks_per_cu = 0;  // 0 = auto: assign_pipe_kernel<NG>'s residency (the occupancy
                                   // query, assign_res[NG]), one round of workgroups, each
                                   // thread a grid-stride pixel sequence
    int assign_res[5] = {};   // [NG]
    int assign_res_chunked = 0;  // the chunk-combining forms (NG = 4)
    int psplit = 0;        // with a communicator of N ranks and the whole image on every rank: rank r
                           // evaluates palettes [r P/N, (r+1) P/N), then one all-gather (option
                           // "palette_split"; SURVEY 8e's split of large populations)
    int slice_ranks = 1, slice_rank = 0;  // test only: the same slice without a communicator
    int slice_lo = 0, slice_n = 0;        // the last evaluation's palettes held on this device
    int fold_blocks = 1, fold_block = 0;  // test only: rank blocks of the counters without a communicator
    int lists16 = 1;       // native 16-bit candidate lists: 1 = chunked palettes of 4 to 32 chunks, 2 = 2 .. 32
    int chunked = 1;       // 256 < K <= 16384: palettes as 256-colour chunks through the grid and
                           // tiled kernels (option "chunked"; 0 = the exhaustive K > 256 path)
    int img_u8_path = 1;   // assign reads the packed 8-bit image when there is one (option 'img_u8')
    int shard_solo = 0;    // experiment: a sharded search without a communicator (per-rank timing)
    int sa_device = 1;     // hq_search_*: 1 = SWASA iterations resident on the device (no host
                           // round trip per iteration), 0 = host-driven (one eval call each)
    int pixel_err = 0;     // test option: the cost kernels also write the per-pixel dE
    int dither_rows = 1024;  // hq_dither_population: rows per strip (option "dither_rows")
    int trim = 1;          // skip taps < 1e-9 of the peak of the narrow k1 filters
    bool trim_ok = false;  // set by hq_set_filters (the bucket's narrow-filter windows hold)
    bool pal_generic = false;  // this population needs the generic cost path (palette_fits_fast)
    bool taps_generic = false;  // set by hq_set_filters: a tap outside the split-f16 range (taps_fit_split),
                                // so the cost runs on the fp32 forms whatever cost_variant and gen_vmfma say

    // comm
    ncclComm_t comm = nullptr;
    int nranks = 1, rank = 0;

    // profiling
    bool prof = false;
    ProfSlot prof_assign, prof_cost, prof_grid, prof_finalize, prof_sa, prof_comm, prof_centroid, prof_lloyd,
        prof_hist, prof_errsum, prof_reseed, prof_dither;
    // profiling: start/stop of grid, assign, cost, finalize, [sa_step], the collective
    hipEvent_t ev[kProfEvents] = {};
    hipEvent_t ev_hist[2] = {};  // ... and of hq_color_histogram's kernel
    hipEvent_t ev_err[2] = {};   // ... and of hq_cluster_errors' kernels (made at the first profiled call)
    int num_cu = 256;
    size_t lds_optin = 160 * 1024;  // per-workgroup LDS a kernel may opt into (hq_create's query)
};

struct hq_search {
    hq_ctx* ctx;
    SearchDriver* driver;  // host-driven search (sa_device = 0), else null
    int K;
    // device-resident search: the SWASA state lives on the device, ping-ponged
    // between [0] and [1] by sa_step_kernel; the host keeps the iteration-only
    // quantities (temperature, step width, convergence threshold) in `pol`,
    // whose RNG is unused.
    Swasa* pol = nullptr;
    hq_swasa_params prm{};
    int P = 0, ite = 0, st = 0, cd = 0;  // state and candidate buffer parities
    int every = 0;                       // hq_search_set_lloyd: iteration ite % every == 0 is hybrid (0: none)
    int repair_every = 0;                // hq_search_set_repair: iteration ite % repair_every == 0 repairs (0: none)
    int repair_moves = -1;               // ... at most so many colours per palette (< 0: no limit)
    int nch = 1;                         // chunked palettes (256 < K <= 16384): chunks per palette
    bool fold = false;                   // accept steps reduce the partials (no finalize launch)
    ncclComm_t comm = nullptr;           // the context's communicator at hq_search_create
    float t_acc = 0.f;                   // temperature / threshold of the iteration
    double keep_acc = 0.0;               // whose population awaits acceptance
    DevBuf colors[2], cand[2], err[2], seed[2], best_err[2], best_colors, jA, jC;
    std::vector<hipEvent_t> pev;         // profiling: kProfSearchEvents events per iteration of a run
    hipGraphExec_t gexec = nullptr;      // option sa_graph: the last run's iteration chain
    int gexec_iters = 0;                 // (its iteration count: the topology an update must match)
};

namespace {

int fail(hq_ctx* c, int code, const char* fmt, ...) {
    if (c) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        c->err = buf;
    }
    return code;
}

#define HIP_TRY(ctx, expr)                                                                      \
    do {                                                                                        \
        hipError_t _e = (expr);                                                                 \
        if (_e != hipSuccess)                                                                   \
            return fail((ctx), _e == hipErrorOutOfMemory ? HQ_ERR_NOMEM : HQ_ERR_DEVICE,        \
                        "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

// Option "pixel_err" forced on for a call's own evaluations, the caller's value back on every way out.
struct PixelErrScope {
    hq_ctx* c;
    int was;
    explicit PixelErrScope(hq_ctx* c_) : c(c_), was(c_->pixel_err) { c->pixel_err = 1; }
    ~PixelErrScope() { c->pixel_err = was; }
    PixelErrScope(const PixelErrScope&) = delete;
    PixelErrScope& operator=(const PixelErrScope&) = delete;
};

#define NCCL_TRY(ctx, expr)                                                                     \
    do {                                                                                        \
        ncclResult_t _r = (expr);                                                               \
        if (_r != ncclSuccess)                                                                  \
            return fail((ctx), HQ_ERR_COMM, "%s failed: %s", #expr, ncclGetErrorString(_r));    \
    } while (0)

inline int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

int bind(hq_ctx* c) {
    HIP_TRY(c, hipSetDevice(c->device));
    return HQ_OK;
}

// Geometry of the shard [r0, r1) of a (W x H) image with halo `half`.
Geom make_geom(int W, int H, int r0, int r1, int half) {
    Geom g{};
    g.W = W;
    g.H = H;
    g.r0 = r0;
    g.r1 = r1;
    g.e0 = std::max(0, r0 - half);
    g.e1 = std::min(H, r1 + half);
    g.lab_pitch = (int)round_up(W, 4);
    g.n_ext = (int64_t)W * (g.e1 - g.e0);
    g.idx_pitch = round_up(g.n_ext + 4, 256);
    return g;
}

int ensure_pinned(hq_ctx* c, size_t pal_bytes, size_t out_bytes) {
    if (pal_bytes > c->h_pal_bytes) {
        if (c->h_pal) (void)hipHostFree(c->h_pal);
        c->h_pal = nullptr;
        HIP_TRY(c, hipHostMalloc((void**)&c->h_pal, pal_bytes, hipHostMallocDefault));
        c->h_pal_bytes = pal_bytes;
    }
    if (out_bytes > c->h_out_bytes) {
        if (c->h_out) (void)hipHostFree(c->h_out);
        c->h_out = nullptr;
        HIP_TRY(c, hipHostMalloc((void**)&c->h_out, out_bytes, hipHostMallocDefault));
        c->h_out_bytes = out_bytes;
    }
    return HQ_OK;
}

// Upload one plane of the extended rows from a full-image host source with
// stride `sstride` floats between pixels and channel offset `ch`.
void gather_rows(const float* src, int sstride, int ch, const Geom& g, std::vector<float>& dst) {
    dst.assign((size_t)round_up(g.n_ext, 4), 0.0f);
    const int64_t base = (int64_t)g.e0 * g.W;
    for (int64_t i = 0; i < g.n_ext; ++i) dst[i] = src[(base + i) * sstride + ch];
}

int compute_labref_device(hq_ctx* c) {
    // IM:100 RGBtoXYZ + IM:285-370 XYZtoScielab on the extended rows.
    const Geom& g = c->g;
    const int64_t n_own = (int64_t)g.W * (g.r1 - g.r0);
    DevBuf opp, tmp, conv, k3v, ak3v;
    HIP_TRY(c, opp.ensure(sizeof(float4) * g.n_ext));
    HIP_TRY(c, tmp.ensure(sizeof(float4) * g.n_ext));
    HIP_TRY(c, conv.ensure(sizeof(float4) * std::max<int64_t>(n_own, 1)));
    std::vector<float> k3h(4 * c->taps, 0.f), ak3h(4 * c->taps, 0.f);
    for (int t = 0; t < c->taps; ++t) { k3h[4 * t] = c->k3[t]; ak3h[4 * t] = c->absk3[t]; }
    HIP_TRY(c, k3v.ensure(sizeof(float) * k3h.size()));
    HIP_TRY(c, ak3v.ensure(sizeof(float) * ak3h.size()));
    HIP_TRY(c, hipMemcpyAsync(k3v.p, k3h.data(), sizeof(float) * k3h.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(ak3v.p, ak3h.data(), sizeof(float) * ak3h.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, launch_labref_opp(c->d_R.as<float>(), c->d_G.as<float>(), c->d_B.as<float>(),
                                 opp.as<float4>(), g.n_ext, c->stream));
    // IM:319-346 filter by filter: H then V (update for filters 2 and 3)
    const float* hk[3] = {c->d_k1.as<float>(), c->d_k2.as<float>(), k3v.as<float>()};
    const float* vk[3] = {c->d_k1.as<float>(), c->d_k2.as<float>(), ak3v.as<float>()};
    for (int f = 0; f < 3; ++f) {
        const int chans = f < 2 ? 3 : 1;
        HIP_TRY(c, launch_labref_hconv(opp.as<float4>(), tmp.as<float4>(), hk[f], c->half, chans,
                                       g.W, g.n_ext, c->stream));
        HIP_TRY(c, launch_labref_vconv(tmp.as<float4>(), conv.as<float4>(), vk[f], c->half, chans,
                                       f > 0, g, c->stream));
    }
    HIP_TRY(c, launch_labref_lab(conv.as<float4>(), c->d_labL.as<float>(), c->d_labA.as<float>(),
                                 c->d_labB.as<float>(), nullptr, g.W, n_own, g.lab_pitch, c->illum,
                                 c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    opp.release(); tmp.release(); conv.release(); k3v.release(); ak3v.release();
    return HQ_OK;
}

int set_image_common(hq_ctx* c, const std::vector<float>& R, const std::vector<float>& G,
                     const std::vector<float>& B, const float* lab4_full, const float* illum) {
    const Geom& g = c->g;
    const size_t plane = sizeof(float) * (size_t)round_up(g.n_ext, 4);
    HIP_TRY(c, c->d_R.ensure(plane));
    HIP_TRY(c, c->d_G.ensure(plane));
    HIP_TRY(c, c->d_B.ensure(plane));
    HIP_TRY(c, hipMemcpyAsync(c->d_R.p, R.data(), plane, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->d_G.p, G.data(), plane, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->d_B.p, B.data(), plane, hipMemcpyHostToDevice, c->stream));
    // An image whose channels are all exactly k/255 (the reference's int-RGB
    // source, IM:100) is also kept as packed bytes: assign reads 4 B per pixel
    // instead of 12 and rebuilds k/255 exactly (u8_unit).  The check and the
    // packing run on the device (pack_u8_kernel); only a 4-byte flag returns.
    {
        HIP_TRY(c, c->d_rgbx.ensure(sizeof(uint32_t) * (size_t)round_up(g.n_ext, 4)));
        DevBuf flag;
        HIP_TRY(c, flag.ensure(sizeof(int)));
        HIP_TRY(c, hipMemsetAsync(flag.p, 0, sizeof(int), c->stream));
        HIP_TRY(c, launch_pack_u8(c->d_R.as<float>(), c->d_G.as<float>(), c->d_B.as<float>(),
                                  c->d_rgbx.as<uint32_t>(), flag.as<int>(), g.n_ext, c->stream));
        int not_u8 = 1;
        HIP_TRY(c, hipMemcpyAsync(&not_u8, flag.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        flag.release();
        c->img_u8 = not_u8 == 0;
        if (!c->img_u8) c->d_rgbx.release();
    }
    if (illum) std::memcpy(c->illum, illum, sizeof c->illum);
    c->sums_ok = false;  // (the index images of the last evaluation belong to the old image)
    c->planar_ok = -1;
    const int own = g.r1 - g.r0;
    const size_t lplane = sizeof(float) * (size_t)g.lab_pitch * std::max(own, 1);
    HIP_TRY(c, c->d_labL.ensure(lplane));
    HIP_TRY(c, c->d_labA.ensure(lplane));
    HIP_TRY(c, c->d_labB.ensure(lplane));
    HIP_TRY(c, hipMemsetAsync(c->d_labL.p, 0, lplane, c->stream));
    HIP_TRY(c, hipMemsetAsync(c->d_labA.p, 0, lplane, c->stream));
    HIP_TRY(c, hipMemsetAsync(c->d_labB.p, 0, lplane, c->stream));
    if (lab4_full) {
        const int64_t n_own = (int64_t)g.W * own;
        DevBuf tmp;
        HIP_TRY(c, tmp.ensure(sizeof(float4) * n_own));
        HIP_TRY(c, hipMemcpyAsync(tmp.p, lab4_full + (int64_t)g.r0 * g.W * 4, sizeof(float4) * n_own,
                                  hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, launch_lab_to_planar(tmp.as<float4>(), c->d_labL.as<float>(), c->d_labA.as<float>(),
                                        c->d_labB.as<float>(), g.W, n_own, g.lab_pitch, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        tmp.release();
    } else {
        int rc = compute_labref_device(c);
        if (rc) return rc;
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->have_image = true;
    return HQ_OK;
}

int check_geom_args(hq_ctx* c, int w, int h, int r0, int r1) {
    if (!c->taps) return fail(c, HQ_ERR_STATE, "filters not set (call hq_set_filters first)");
    if (w < c->half || h < c->half || w < 1 || h < 1)
        return fail(c, HQ_ERR_ARG, "image %dx%d smaller than the stencil half-width %d", w, h, c->half);
    if (r0 < 0 || r1 > h || r0 >= r1) return fail(c, HQ_ERR_ARG, "bad row range [%d,%d)", r0, r1);
    // the cost kernels address a shard's index image and its fp32 LabRef planes with
    // 32-bit unsigned byte offsets: keep 4 bytes per (padded) pixel below 2^32
    if ((int64_t)(w + 4) * (int64_t)(r1 - r0 + 2 * c->half) >= ((int64_t)1 << 30))
        return fail(c, HQ_ERR_UNSUPPORTED, "shard of %d x %d pixels exceeds 2^30; use more row blocks",
                    w, r1 - r0);
    return HQ_OK;
}

// Assign workgroups per palette group: assign_blocks_per_cu per CU, but no more
// than pixel chunks (256 pixels, one per thread): idle workgroups still fill LDS,
// and after the XCD relabelling they would all sit on the last XCDs (a 512-row
// shard ran assign on half the chip: 0.071 vs 0.053 ms).  (Evening out the
// chunks per workgroup instead -- 1064 workgroups of 2 for 2128 chunks -- was
// slower than 2048 with 80 of them taking a second chunk.)
// assign: one pixel per thread per 256-thread chunk, with one resident round
// of workgroups, makes each thread's pixel sequence a grid stride: every thread
// gets the same number of pixels +-1 (512-row shard 0.1306 -> 0.1261 ms per
// step vs 4 pixels per chunk at 16 workgroups per CU; 4096^2 unchanged).
#ifndef HQ_ASSIGN_MINPX
#define HQ_ASSIGN_MINPX 6
#endif
int assign_blocks(const hq_ctx* c, int P) {
    // at least HQ_ASSIGN_MINPX pixels per thread: a launch's fixed part (table
    // fill, pipeline start, the used-bit flush) is paid per workgroup (C2,
    // 1024^2 P = 1: 2048 workgroups of 2 pixels per thread took 14 us, 1045 of 4
    // took 12.3, 523 of 8 took 8.5; the 512-row shard, 5.5 per thread at 1536
    // workgroups, slowed from 43 to 46 us at 8)
    const int64_t chunk = 256 * HQ_ASSIGN_MINPX;
    const int ng = std::min(P, 4);
    const int res = c->nch_cur > 1 ? c->assign_res_chunked : c->assign_res[ng];
    const int per_cu = c->assign_blocks_per_cu > 0 ? c->assign_blocks_per_cu : res > 0 ? res : 4;
    const int64_t nblocks = (int64_t)c->num_cu * per_cu;
    return (int)std::max<int64_t>(1, std::min<int64_t>(nblocks, (c->g.n_ext + chunk - 1) / chunk));
}

// A row-block split (a communicator, no palette split) keeps one block of
// counters and used bits per rank in each set, [ranks][...]: every rank fills
// its own block, and a device-resident search's one all-gather per iteration
// hands every rank all the blocks, which its accept step folds (no finalize).
// (test options fold_blocks / fold_block: the same layout without a communicator,
// this context filling block fold_block and the others staying zero)
int rank_blocks(const hq_ctx* c) { return c->comm ? (c->psplit ? 1 : c->nranks) : c->fold_blocks; }
int own_block(const hq_ctx* c) { return c->comm ? (rank_blocks(c) > 1 ? c->rank : 0) : c->fold_block; }
// A device-resident search folds the partials in its accept step unless the
// palette split all-gathers finalized rows.
bool search_folds(const hq_ctx* c) { return !(c->comm && c->psplit); }

// Chunked palettes of 4 to 32 chunks take the native 16-bit lists (option lists16).
// Their kernels take up to 144 KiB (lists16_kernel at K = 8192) and 128 KiB
// (assign16_kernel) of dynamic LDS: a device that cannot grant that (less than
// gfx950's 160 KiB per workgroup) keeps the per-chunk grids.
bool use_lists16(const hq_ctx* c) {
    const int min_nch = c->lists16 >= 2 ? 2 : kN16MinNch;  // (2: also 2 and 4 chunks)
    if (!(c->lists16 > 0 && c->G2 > 0 && c->nch_cur >= min_nch && c->nch_cur <= kN16MaxNch)) return false;
    const size_t K = (size_t)kMaxK * c->nch_cur;
    const size_t grid_lds = ((K > 4096 ? 3 : 4) * sizeof(float) + sizeof(uint16_t)) * K +
                            sizeof(uint16_t) * 64 * n16_l1_words((int)K);
    const size_t assign_lds = sizeof(float4) * K * (K <= 4096 ? 2 : 1);
    return std::max(grid_lds, assign_lds) <= c->lds_optin;
}

// The population being enqueued takes the fast tiled cost kernels (else the
// generic pair, whose [7][n_ext] scratch ensure_population then allocates up
// front: nothing may allocate while a search run is captured into a graph).
// Chunked palettes: the 16 x 128 tiles at HB = 10 only.
bool cost_fast(const hq_ctx* c) {
    return c->cost_variant == 0 && c->fast_hb > 0 && !c->pal_generic && !c->taps_generic &&
           (c->nch_cur == 1 || (c->nch_cur <= kMaxNchFast && c->fast_hb == 10 && c->cost_rows == 16 &&
                                c->cost_tw == 128));
}

// Ensure population buffers for P palettes of K colours.
int ensure_population(hq_ctx* c, int P, int K) {
    const Geom& g = c->g;
    if (c->nch_cur > 1) {  // chunked palettes: 16-bit indices, then P nch sub-palettes of 256
        HIP_TRY(c, c->d_idx16.ensure(sizeof(uint16_t) * (size_t)P * g.idx_pitch + 256));
        if (c->nch_cur > 4) HIP_TRY(c, c->d_dist.ensure(sizeof(float) * (size_t)P * g.idx_pitch));
        if (use_lists16(c)) {
            HIP_TRY(c, c->d_l1n.ensure(sizeof(uint16_t) * n16_l1_words(K) * (size_t)P * kN16G1 * kN16G1 * kN16G1));
            // (palette pairs interleaved: an odd population's last pair half empty)
            HIP_TRY(c, c->d_l2n.ensure(sizeof(uint16_t) * kN16L2Words * (size_t)(P + 1) / 2 * 2 * kN16G2 * kN16G2 * kN16G2));
        }
        P *= c->nch_cur;  // (d_out, h_out: P nch (1 + 256) >= P (1 + K) doubles)
        K = kMaxK;
    }
    const int G2 = c->G2 > 0 ? c->G2 : 4;
    const int G1 = G2 / 4;
    const int64_t l1p = round_up((int64_t)G1 * G1 * G1 * 32, 256);
    const int64_t l2g = round_up((int64_t)G2 * G2 * G2 * kL2Line, 256);  // per group of 4 palettes
    const int64_t n_own = (int64_t)g.W * (g.r1 - g.r0);
    HIP_TRY(c, c->d_pal_in.ensure(sizeof(float4) * (size_t)P * K));
    HIP_TRY(c, c->d_pal.ensure(sizeof(float4) * (size_t)P * std::max(K, kMaxK)));
    HIP_TRY(c, c->d_opp.ensure(sizeof(float4) * (size_t)P * std::max(K, kMaxK)));
    if (K > kMaxK) {
        HIP_TRY(c, c->d_idx32.ensure(sizeof(uint32_t) * (size_t)P * g.idx_pitch));
        HIP_TRY(c, c->d_used32.ensure(sizeof(uint32_t) * (size_t)P * K));
    }
    HIP_TRY(c, c->d_opp16.ensure(sizeof(uint4) * (size_t)P * kMaxK));
    HIP_TRY(c, c->d_dup.ensure((size_t)P * kMaxK));
    HIP_TRY(c, c->d_pflags.ensure(sizeof(int) * (size_t)P));
    HIP_TRY(c, c->d_lvl1.ensure((size_t)P * l1p));
    HIP_TRY(c, c->d_lvl2.ensure((size_t)((P + 3) / 4) * l2g));
    // + 256: the cost kernels' interior fills read whole dword pairs, up to 7
    // bytes past a region's last column (past the buffer on the last palette's
    // last row when idx_pitch has no padding)
    HIP_TRY(c, c->d_idx.ensure((size_t)P * g.idx_pitch + 256));
    const size_t rb = (size_t)rank_blocks(c);  // counter / used-bit blocks per set
    HIP_TRY(c, c->d_used_mask.ensure(2 * rb * sizeof(uint32_t) * kUsedSlots * (size_t)used_stride(P)));
    HIP_TRY(c, c->d_acc.ensure(2 * rb * sizeof(uint64_t) * acc_words(P)));
    HIP_TRY(c, c->d_out.ensure(sizeof(double) * (size_t)P * (1 + K)));
    if (c->pixel_err) HIP_TRY(c, c->d_pixerr.ensure(sizeof(float) * (size_t)P * std::max<int64_t>(n_own, 1)));
    // the generic path's [7][n_ext] scratch, here rather than at its first launch: an
    // allocation cannot happen while a search run is being captured into a graph
    if (!cost_fast(c) || K > kMaxK) HIP_TRY(c, c->d_gen_t.ensure(sizeof(float) * 7 * (size_t)g.n_ext + 256));
    return ensure_pinned(c, sizeof(float) * 4 * (size_t)P * K, sizeof(double) * (size_t)P * (1 + K));
}

void prof_add(hq_ctx* c, ProfSlot& s, hipEvent_t a, hipEvent_t b) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, a, b) == hipSuccess) {
        s.ms += ms;
        s.launches += 1;
    } else {
        (void)hipGetLastError();  // an event pair this evaluation never recorded: not a launch error
    }
}

PaletteArgs prep_args(hq_ctx* c, int K) {
    return PaletteArgs{c->d_pal_in.as<float4>(), c->d_pal.as<float4>(), c->d_opp.as<float4>(),
                       c->d_opp16.as<uint4>(), c->d_dup.as<uint8_t>(), c->d_pflags.as<int>(), K};
}

// Enqueue the evaluation of the P prepared palettes (d_pal, d_opp, d_dup,
// d_pflags): grid, assign, cost, finalize into d_out (partial sums + used
// flags), all-reduced if a comm is set.  ev (8 events, or null): start/stop of
// the grid, assign, cost and finalize launches, carried by the launches
// themselves (set_launch_events).
// Counter set `par` of an evaluation of P palettes (P nch sub-palettes Ps).
uint64_t* acc_base(hq_ctx* c, int par, int P) {
    return c->d_acc.as<uint64_t>() + (size_t)par * rank_blocks(c) * acc_words(P);
}
uint32_t* used_base(hq_ctx* c, int par, int Ps) {
    return c->d_used_mask.as<uint32_t>() + (size_t)par * rank_blocks(c) * kUsedSlots * used_stride(Ps);
}
uint64_t* acc_set(hq_ctx* c, int par, int P) { return acc_base(c, par, P) + (size_t)own_block(c) * acc_words(P); }
uint32_t* used_set(hq_ctx* c, int par, int Ps) {
    return used_base(c, par, Ps) + (size_t)own_block(c) * kUsedSlots * used_stride(Ps);
}

GridArgs grid_args(hq_ctx* c, int P, int K, int so = 0) {
    const int G2 = c->G2 > 0 ? c->G2 : 4;
    const int G1 = G2 / 4;
    // (P = sub-palettes; the counters of set c->acc_par)
    const int nch = c->nch_cur;
    // (so: the first of the P sub-palettes in the prepared tables, a palette split's slice)
    return GridArgs{c->d_pal.as<float4>() + (int64_t)so * kMaxK, c->d_dup.as<uint8_t>() + (int64_t)so * kMaxK,
                    c->d_pflags.as<int>() + so, c->d_lvl1.as<uint8_t>(), c->d_lvl2.as<uint8_t>(),
                    used_set(c, c->acc_par, P),
                    used_stride(P), K, G1,
                    round_up((int64_t)G1 * G1 * G1 * 32, 256), round_up((int64_t)G2 * G2 * G2 * kL2Line, 256),
                    acc_set(c, c->acc_par, P / nch), P / nch, nch};
}

// The generic two-pass cost (CL:234-306 per pixel, any half-width) of P
// palettes, one launch pair each: index images at idx_base (u8, or u32 when
// u16 (chunked palettes) or u32, idx_bytes) with c->g.idx_pitch elements per palette, opponent tables of
// opp_stride entries per palette in d_opp.  The cost events time all P pairs.
int enqueue_generic_cost(hq_ctx* c, int P, const void* idx_base, int idx_bytes, int opp_stride,
                         const hipEvent_t* ev, int p_off = 0) {
    const Geom& g = c->g;
    hipStream_t s = c->stream;
    HIP_TRY(c, c->d_gen_t.ensure(sizeof(float) * 7 * (size_t)g.n_ext + 256));
    const int64_t n_own = (int64_t)g.W * (g.r1 - g.r0);
    const float inv[3] = {1.0f / c->illum[0], 1.0f / c->illum[1], 1.0f / c->illum[2]};
    for (int p = 0; p < P; ++p) {
        GenArgs gn{};
        gn.idx = static_cast<const char*>(idx_base) + (int64_t)p * g.idx_pitch * idx_bytes;
        gn.opp = c->d_opp.as<float4>() + (int64_t)(p_off + p) * opp_stride;
        gn.k1 = c->d_k1.as<float>();
        gn.k2 = c->d_k2.as<float>();
        gn.k3 = c->d_k3.as<float>();
        gn.absk3 = c->d_absk3.as<float>();
        gn.t = c->d_gen_t.as<float>();
        gn.labL = c->d_labL.as<float>();
        gn.labA = c->d_labA.as<float>();
        gn.labB = c->d_labB.as<float>();
        gn.acc = acc_set(c, c->acc_par, P);
        gn.p = p;
        gn.P = P;
        gn.g = g;
        gn.half = c->half;
        gn.pix_err = c->pixel_err ? c->d_pixerr.as<float>() + (int64_t)p * n_own : nullptr;
        gn.vtaps = c->d_vtaps.as<float>();
        gn.vtap_pitch = c->vtap_pitch;
        gn.hrow4 = c->gen_hrow4;
        gn.hrow_no = c->gen_hrow_no;
        gn.vtile2 = c->gen_vtile2;
        // split-f16 planes hold |x| < 4 (x 2^14), split taps |w| <= kVTapMax: palettes and
        // filters outside the fast range stay on fp32 (gen_hmfma runs only with gen_vmfma)
        gn.vmfma = c->gen_vmfma && !c->pal_generic && !c->taps_generic;
        gn.vtapd = c->d_vfragm.bytes ? c->d_vfragm.as<uint32_t>() : nullptr;
        gn.hmfma = c->gen_hmfma;
        gn.shape = c->gen_shape;
        gn.htapd = gn.vtapd ? gn.vtapd + vtile_dup_tap_words(c->half) : nullptr;
        gn.htaps = c->d_htaps.as<float4>();
        opp2xyz_over_illum(inv, gn.m_lab);
        // the events span every palette's launch pair: start on the first, stop on the last
        if (ev) set_launch_events(p == 0 ? ev[4] : nullptr, p == P - 1 ? ev[5] : nullptr);
        // cost_variant 2: the per-pixel pair in the reference's summation order
        const hipError_t e = c->cost_variant == 2 ? launch_cost_generic(gn, c->de_type, idx_bytes, s)
                                                  : launch_cost_tiled_generic(gn, c->de_type, idx_bytes, s);
        set_launch_events(nullptr, nullptr);
        HIP_TRY(c, e);
    }
    return HQ_OK;
}

int palette_slice(hq_ctx* c, int P, int* lo, int* n);

// K > 256 (hq_wide.hip): prep, exhaustive argmin into 32-bit indices and
// per-colour used flags, the generic cost, finalize, [all-reduce or, under a
// palette split, all-gather].  A palette split takes the same slice
// [lo, lo + Pl) as enqueue_core: the other ranks' palettes are prepped here
// too (cheap) but neither assigned nor costed, so no rank counts them.
int enqueue_wide(hq_ctx* c, int P, int K, const hipEvent_t* ev) {
    const Geom& g = c->g;
    hipStream_t s = c->stream;
    int lo = 0, Pl = P;
    if (int rc = palette_slice(c, P, &lo, &Pl)) return rc;
    WideArgs wa{c->d_pal_in.as<float4>(), c->d_pal.as<float4>(), c->d_opp.as<float4>(), c->d_pflags.as<int>(),
                c->d_R.as<float>(), c->d_G.as<float>(), c->d_B.as<float>(), c->d_idx32.as<uint32_t>(),
                c->d_used32.as<uint32_t>(), g.n_ext, g.idx_pitch, K};
    c->acc_par ^= 1;
    if (Pl < P && !c->comm)  // test-only slice: the other palettes' rows read as zero
        HIP_TRY(c, hipMemsetAsync(c->d_out.p, 0, sizeof(double) * (size_t)P * (1 + K), s));
    HIP_TRY(c, hipMemsetAsync(acc_set(c, c->acc_par, Pl), 0, sizeof(uint64_t) * acc_words(Pl), s));
    HIP_TRY(c, hipMemsetAsync(c->d_pflags.p, 0, sizeof(int) * (size_t)P, s));
    HIP_TRY(c, launch_prep_wide(wa, P, s));
    HIP_TRY(c, hipMemsetAsync(c->d_used32.p, 0, sizeof(uint32_t) * (size_t)Pl * K, s));
    // the slice's palettes: indices and used flags in rows 0 .. Pl - 1
    WideArgs ws = wa;
    ws.pal += (int64_t)lo * K;
    ws.opp += (int64_t)lo * K;
    ws.pflags += lo;
    if (ev) set_launch_events(ev[2], ev[3]);
    const hipError_t e = launch_assign_wide(ws, Pl, s);
    set_launch_events(nullptr, nullptr);
    HIP_TRY(c, e);
    int rc = enqueue_generic_cost(c, Pl, c->d_idx32.p, 4, K, ev, lo);
    if (rc) return rc;
    FinalizeArgs fa{acc_set(c, c->acc_par, Pl), nullptr, 0, c->d_out.as<double>() + (int64_t)lo * (1 + K), Pl, K,
                    c->d_used32.as<uint32_t>(), 8};
    if (ev) set_launch_events(ev[6], ev[7]);
    const hipError_t ef = launch_finalize(fa, Pl, s);
    set_launch_events(nullptr, nullptr);
    HIP_TRY(c, ef);
    if (c->comm) {
        if (ev) HIP_TRY(c, hipEventRecord(ev[10], s));
        if (c->psplit)
            NCCL_TRY(c, ncclAllGather(c->d_out.as<double>() + (int64_t)lo * (1 + K), c->d_out.p,
                                      (size_t)Pl * (1 + K), ncclFloat64, c->comm, s));
        else
            NCCL_TRY(c, ncclAllReduce(c->d_out.p, c->d_out.p, (size_t)P * (1 + K), ncclFloat64, ncclSum,
                                      c->comm, s));
        if (ev) HIP_TRY(c, hipEventRecord(ev[11], s));
    }
    c->slice_lo = lo;
    c->slice_n = Pl;
    c->last_P = P;
    c->K_cur = K;
    c->last_nch = 1;
    return HQ_OK;
}

// P palettes of K colours.  Chunked palettes (c->nch_cur = nch > 1, 256 < K <=
// 256 nch): the grid and assign run on P nch sub-palettes of 256 colours (d_pal
// etc. hold them, prep_palette made them), assign combines them into 16-bit
// indices, the cost kernel reads those with a 256 nch-entry table.
// The palettes of a P-palette population this device evaluates: a palette
// split (psplit with a communicator of N ranks, or the test-only slice options)
// takes [r P/N, (r+1) P/N) on the whole image; anything else all P.
int palette_slice(hq_ctx* c, int P, int* lo, int* n) {
    int R = 1, r = 0;
    if (c->psplit && c->comm) R = c->nranks, r = c->rank;
    else if (c->slice_ranks > 1) R = c->slice_ranks, r = c->slice_rank;
    *lo = 0;
    *n = P;
    if (R == 1) return HQ_OK;
    if (r < 0 || r >= R) return fail(c, HQ_ERR_ARG, "palette split: rank %d outside [0, %d)", r, R);
    if (P % R) return fail(c, HQ_ERR_ARG, "palette split: population %d not divisible by %d ranks", P, R);
    if (c->g.r0 != 0 || c->g.r1 != c->g.H)
        return fail(c, HQ_ERR_STATE, "palette split: every rank needs the whole image (hq_set_image)");
    *n = P / R;
    *lo = r * *n;
    return HQ_OK;
}

// Each evaluation takes the other counter set than the last one (build_grid
// zeroes it), so an accept step can read the last set while the next is filled.
// assign_only (a hybrid iteration's first pass): the argmin alone -- grid build
// or zeroing, then assign -- for the index images the sums kernel reads; no
// cost kernel, no finalize, no collective.  It fills the other set's used bits
// without making that set the current one: c->acc_par stays the set of the
// last full pass (what sa_args, the fold and the finalize read), and the full
// pass that follows takes, and zeroes, the same set again.
// err_pass (a repair iteration's first pass): grid, assign and cost -- the index
// images and, with option "pixel_err" in force, the error image the error kernel
// reads -- but no finalize and no collective, into the other set like an
// assign-only pass and for the same reason: nothing reads its sums.
// dither (hq_dither_population; null: the plain argmin): the index images are the
// Floyd-Steinberg rendering at that strength -- the counter set and the used bits
// zeroed as without a grid, then dither_kernel in the place of grid + assign (its
// events are the assign pair's), the cost and finalize as ever.
int enqueue_core(hq_ctx* c, int P, int K, const hipEvent_t* ev, bool fold = false, bool assign_only = false,
                 bool err_pass = false, const float* dither = nullptr) {
    const Geom& g = c->g;
    hipStream_t s = c->stream;
    const int nch = c->nch_cur, Ks = nch > 1 ? kMaxK : K;
    // the palettes this device evaluates: all, or a palette split's slice [lo, lo + Pl)
    int lo = 0, Pl = P;
    if (int rc = palette_slice(c, P, &lo, &Pl)) return rc;
    const int Ps = Pl * nch, so = lo * nch;  // sub-palettes, the first one's index
    if (Pl < P && !c->comm && !assign_only)  // test-only slice: the other palettes' rows read as zero
        HIP_TRY(c, hipMemsetAsync(c->d_out.p, 0, sizeof(double) * (size_t)P * (1 + K), s));
    c->acc_par ^= 1;
    struct ParRestore {  // assign_only: back to the last full pass's set on every way out
        hq_ctx* c;
        bool on;
        ~ParRestore() { if (on) c->acc_par ^= 1; }
    } restore{c, assign_only || err_pass};
    const GridArgs ga = grid_args(c, Ps, Ks, so);
    auto timed = [&](int slot) {
        if (ev) set_launch_events(ev[2 * slot], ev[2 * slot + 1]);
    };
    auto untimed = [&]() { set_launch_events(nullptr, nullptr); };
    const bool n16 = use_lists16(c);
    if (c->G2 > 0 && !dither) {  // (build_grid also zeroes the used bits and the sums)
        timed(0);
        const hipError_t e =
            n16 ? launch_lists16_grid(Lists16Args{ga.pal, ga.pflags, c->d_l1n.as<uint16_t>(), c->d_l2n.as<uint16_t>(),
                                                  ga.used_glob, used_stride(Ps), ga.acc_zero, Pl, K, nch * kMaxK, nch},
                                      Pl, s)
                : launch_build_grid(ga, Ps, s);
        untimed();
        HIP_TRY(c, e);
    } else {
        HIP_TRY(c, hipMemsetAsync(ga.used_glob, 0, sizeof(uint32_t) * kUsedSlots * (size_t)used_stride(Ps), s));
        HIP_TRY(c, hipMemsetAsync(ga.acc_zero, 0, sizeof(uint64_t) * acc_words(Pl), s));
    }
    const int nblocks = assign_blocks(c, Ps);
    AssignArgs aa{c->d_R.as<float>(), c->d_G.as<float>(), c->d_B.as<float>(),
                  c->img_u8 && c->img_u8_path ? c->d_rgbx.as<uint32_t>() : nullptr, ga.pal, ga.pflags,
                  c->d_lvl1.as<uint8_t>(), c->d_lvl2.as<uint8_t>(),
                  c->d_idx.as<uint8_t>(), ga.used_glob, used_stride(Ps), g.n_ext, g.idx_pitch,
                  ga.lvl1_pitch, ga.lvl2_gstride, Ks, c->G2, nblocks};
    if (nch > 1) {
        aa.idx16 = c->d_idx16.as<uint16_t>();
        aa.dist = nch > 4 ? c->d_dist.as<float>() : nullptr;
        aa.nch = nch;
        while ((1 << aa.lg_nch) < nch) ++aa.lg_nch;
    }
    if (n16) {  // one palette of K colours per workgroup (its table in LDS)
        aa.l1n = c->d_l1n.as<uint16_t>();
        aa.l2n = c->d_l2n.as<uint16_t>();
        aa.kpal = nch * kMaxK;
        aa.K = K;
        // one resident round of 1024-thread workgroups over the P palettes, >= 4 pixels per thread
        const int ngr = K <= 4096 ? (Pl + 1) / 2 : Pl;  // workgroup groups: palette pairs up to K = 4096
        aa.nblocks = (int)std::max<int64_t>(
            1, std::min<int64_t>(std::max(1, c->num_cu / ngr), (g.n_ext + 4095) / 4096));
    }
    const float inv[3] = {1.0f / c->illum[0], 1.0f / c->illum[1], 1.0f / c->illum[2]};
    const bool fast = cost_fast(c);
    // 8-row tiles (cost_mfma_kernel) exist for the 21-tap bucket only
    const int rows = c->fast_hb == 10 ? c->cost_rows : 16;
    const int tw = c->fast_hb == 10 ? c->cost_tw : 128;  // 256-column tiles: HB = 10 only
    CostArgs ca{};
    if (fast) {
        ca.idx = nch > 1 ? c->d_idx16.as<uint8_t>() : c->d_idx.as<uint8_t>();
        ca.opp16 = c->d_opp16.as<uint4>() + (int64_t)so * kMaxK;
        ca.taps = c->d_taps.p;
        ca.vfrag16 = c->d_vfrag16.as<uint4>();
        ca.vfrag16p = c->d_vfrag16p.as<uint4>();
        ca.labL = c->d_labL.as<float>();
        ca.labA = c->d_labA.as<float>();
        ca.labB = c->d_labB.as<float>();
        ca.acc = ga.acc_zero;
        ca.acc_P = Pl;
        ca.acc_p0 = 0;
        ca.g = g;
        ca.K = K;
        fast_tile_dims(g.W, g.r1 - fast_grid_row0(c->de_type, g.r0, rows), rows, tw, &ca.tiles_x, &ca.ntiles);
        opp2xyz_over_illum(inv, ca.m_lab);
        ca.pix_err = c->pixel_err ? c->d_pixerr.as<float>() : nullptr;
        ca.pix_pitch = (int64_t)g.W * (g.r1 - g.r0);
    }
    timed(1);
    hipError_t e = dither ? launch_dither(DitherArgs{aa.R, aa.G, aa.B, ga.pal, aa.idx, ga.used_glob,
                                                     c->d_dcarry.as<float>(), g.idx_pitch, g.W, g.H, K,
                                                     c->dither_rows, *dither},
                                          Pl, s)
                   : n16  ? launch_assign16(aa, Pl, s)
                          : launch_assign(aa, Ps, s);
    untimed();
    HIP_TRY(c, e);
    if (assign_only) {
        c->slice_lo = lo;
        c->slice_n = Pl;
        c->last_P = P;
        c->K_cur = K;
        c->last_nch = nch;
        return HQ_OK;
    }
    if (fast) {
        timed(2);
        e = nch > 1 ? launch_cost_chunked(ca, Pl, nch, c->de_type, c->trim && c->trim_ok, s)
                    : launch_cost_fast(ca, Pl, c->de_type, c->trim && c->trim_ok, rows, tw, c->fast_hb, s);
        untimed();
        HIP_TRY(c, e);
    } else {
        int rc = nch > 1 ? enqueue_generic_cost(c, Pl, c->d_idx16.p, 2, nch * kMaxK, ev, lo)
                         : enqueue_generic_cost(c, Pl, c->d_idx.p, 1, kMaxK, ev, lo);
        if (rc) return rc;
    }
    if (err_pass) {
        c->slice_lo = lo;
        c->slice_n = Pl;
        c->last_P = P;
        c->K_cur = K;
        c->last_nch = nch;
        return HQ_OK;
    }
    if (!fold) {  // (a folding search's accept step reads the sums itself)
        FinalizeArgs fa{ga.acc_zero, ga.used_glob, used_stride(Ps), c->d_out.as<double>() + (int64_t)lo * (1 + K),
                        Pl, K, nullptr, 8 * nch};
        timed(3);
        const hipError_t ef = launch_finalize(fa, Pl, s);
        untimed();
        HIP_TRY(c, ef);
    }
    if (c->comm) {
        // the collective's time (profiling only: an event record between launches
        // idles the GPU a few us, so the timed pass of bench.py records none)
        if (ev) HIP_TRY(c, hipEventRecord(ev[10], s));
        if (fold) {
            // row blocks under a folding search: every rank's counter block and
            // used-bit block to every rank (in place), one group of two
            // all-gathers; the accept step sums the integer counters and ORs the
            // bits of all the blocks itself
            const size_t na = acc_words(Pl), nu = (size_t)kUsedSlots * used_stride(Ps);
            NCCL_TRY(c, ncclGroupStart());
            NCCL_TRY(c, ncclAllGather(acc_set(c, c->acc_par, Pl), acc_base(c, c->acc_par, Pl), na, ncclUint64,
                                      c->comm, s));
            NCCL_TRY(c, ncclAllGather(used_set(c, c->acc_par, Ps), used_base(c, c->acc_par, Ps), nu, ncclUint32,
                                      c->comm, s));
            NCCL_TRY(c, ncclGroupEnd());
        } else if (c->psplit) {  // every rank's slice to every rank (in place; one rank: a no-op)
            NCCL_TRY(c, ncclAllGather(c->d_out.as<double>() + (int64_t)lo * (1 + K), c->d_out.p,
                                      (size_t)Pl * (1 + K), ncclFloat64, c->comm, s));
        } else {  // also with one rank (a no-op copy), so that path is exercised on one GPU
            NCCL_TRY(c, ncclAllReduce(c->d_out.p, c->d_out.p, (size_t)P * (1 + K), ncclFloat64, ncclSum,
                                      c->comm, s));
        }
        if (ev) HIP_TRY(c, hipEventRecord(ev[11], s));
    }
    c->slice_lo = lo;
    c->slice_n = Pl;
    c->last_P = P;
    c->K_cur = K;
    c->last_nch = nch;
    return HQ_OK;
}

// Add one evaluation's kernel times (its events have completed).
void prof_accumulate(hq_ctx* c, const hipEvent_t* ev, bool finalize = true, bool grid = true) {
    if (grid && c->G2 > 0) prof_add(c, c->prof_grid, ev[0], ev[1]);
    prof_add(c, c->prof_assign, ev[2], ev[3]);
    prof_add(c, c->prof_cost, ev[4], ev[5]);
    if (finalize) prof_add(c, c->prof_finalize, ev[6], ev[7]);
    if (c->comm) prof_add(c, c->prof_comm, ev[10], ev[11]);
}

// ... and the SA step that generated it (device-resident search: events 8, 9).
void prof_accumulate_sa(hq_ctx* c, const hipEvent_t* ev) {
    prof_add(c, c->prof_sa, ev[8], ev[9]);
}

// Host-driven evaluation of the P palettes in h_pal: upload, prep, enqueue_core,
// read back d_out into h_out.
int enqueue_eval(hq_ctx* c, int P, int K) {
    hipStream_t s = c->stream;
    const size_t n_in = c->nch_cur > 1 ? (size_t)P * c->nch_cur * kMaxK : (size_t)P * K;
    HIP_TRY(c, hipMemcpyAsync(c->d_pal_in.p, c->h_pal, sizeof(float4) * n_in, hipMemcpyHostToDevice, s));
    const hipEvent_t* ev = c->prof ? c->ev : nullptr;
    int rc;
    if (c->nch_cur > 1) {  // h_pal holds P nch sub-palettes of 256 (pack_chunks)
        HIP_TRY(c, launch_prep_palette(prep_args(c, kMaxK), P * c->nch_cur, s));
        rc = enqueue_core(c, P, K, ev);
    } else if (K > kMaxK) {
        rc = enqueue_wide(c, P, K, ev);
    } else {
        HIP_TRY(c, launch_prep_palette(prep_args(c, K), P, s));
        rc = enqueue_core(c, P, K, ev);
    }
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->h_out, c->d_out.p, sizeof(double) * (size_t)P * (1 + K),
                              hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    if (ev) prof_accumulate(c, ev, true, K <= kMaxK || c->nch_cur > 1);  // (the wide path builds no grid)
    return HQ_OK;
}

int check_eval_args(hq_ctx* c, const float* palettes, int P, int K) {
    if (!c) return HQ_ERR_ARG;
    if (!c->have_image) return fail(c, HQ_ERR_STATE, "no image set (hq_set_image)");
    if (!palettes || P < 1 || K < 1) return fail(c, HQ_ERR_ARG, "bad palettes / P=%d / K=%d", P, K);
    if (K > kMaxKWide)
        return fail(c, HQ_ERR_ARG, "K=%d > %d (the plugin's limit, HQ:192)", K, kMaxKWide);
    return HQ_OK;
}

// The fast cost kernels take the opponent colours as split f16 of x * 2^14
// (split_f16): |opp| must stay below 65504 / 2^14 ~ 4.  RGB2Opp's largest
// absolute row sum is 0.871, so a palette channel x in [-59, 1.93] keeps
// |opp| < 4 (lin(x) = x / 12.92 below 0.04045, ((x + 0.055) / 1.055)^2.4
// above).  Colours outside [-32, 1.9] -- never produced by the SA, which
// clamps to [0, 1] (SW:103-106), but accepted by hq_eval_population -- and
// non-finite colours send the population to the generic fp32 path.
// [P][K] palettes -> P nch sub-palettes of 256 colours: sub-palette p nch + c
// holds colours 256 c .. 256 c + 255 of palette p, and copies of colour 0 past
// K (a copy of colour 0 ties it and never wins the chunk combine, which keeps
// the first chunk at equal distance; hq_assign.hip).
void pack_chunks(const float* pal, int P, int K, int nch, float* out) {
    for (int p = 0; p < P; ++p)
        for (int k = 0; k < nch * kMaxK; ++k) {
            const float* src = pal + 4 * ((size_t)p * K + (k < K ? k : 0));
            float* dst = out + 4 * ((size_t)p * nch * kMaxK + k);
            dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2]; dst[3] = src[3];
        }
}

bool palette_fits_fast(const float* pal, int P, int K) {
    for (size_t i = 0, n = (size_t)P * K; i < n; ++i)
        for (int ch = 0; ch < 3; ++ch) {
            const float x = pal[4 * i + ch];
            if (!(x >= -32.0f && x <= 1.9f)) return false;
        }
    return true;
}

int eval_partial_into_hout(hq_ctx* c, const float* palettes, int P, int K) {
    int rc = check_eval_args(c, palettes, P, K);
    if (rc) return rc;
    if ((rc = bind(c))) return rc;
    const bool fits = palette_fits_fast(palettes, P, K);
    // 256 < K <= 16384: chunks of 256 colours through the grid and assign, and the
    // tiled cost kernel up to 32 chunks (the generic pair above).  Palettes outside
    // the fast range (non-finite colours among
    // them) take the exhaustive K > 256 path instead, which keeps the
    // reference's NaN semantics across all K colours.
    c->nch_cur = c->chunked && fits && c->G2 > 0 && K > kMaxK && K <= kMaxKChunked ? chunk_count(K) : 1;
    c->pal_generic = !fits;  // (before ensure_population: it sizes the generic path's scratch)
    if (!(rc = ensure_population(c, P, K))) {
        if (c->nch_cur > 1) pack_chunks(palettes, P, K, c->nch_cur, c->h_pal);
        else std::memcpy(c->h_pal, palettes, sizeof(float) * 4 * (size_t)P * K);
        rc = enqueue_eval(c, P, K);
    }
    c->pal_generic = false;  // device-resident searches generate clamped palettes
    c->nch_cur = 1;
    c->sums_ok = rc == HQ_OK;
    c->err_ok = c->sums_ok && c->pixel_err;
    return rc;
}

// The sums form assign's own condition picks: the packed bytes (den 255), else
// the planar floats (den 2^32).
bool sums_u8(const hq_ctx* c) { return c->img_u8 && c->img_u8_path; }

// The sums kernel's arguments for the index images of the last evaluation (or
// assign-only pass) of P palettes of K colours: the owned rows, as
// hq_get_indices[32] reads them, into d_sums ([P][K][4], then the range flag).
ClusterArgs cluster_args(hq_ctx* c, int P, int K, int* idx_bytes) {
    const Geom& g = c->g;
    ClusterArgs ca{};
    *idx_bytes = c->last_nch > 1 ? 2 : K > kMaxK ? 4 : 1;
    ca.idx = *idx_bytes == 2 ? c->d_idx16.p : *idx_bytes == 4 ? c->d_idx32.p : c->d_idx.p;
    ca.R = c->d_R.as<float>();
    ca.G = c->d_G.as<float>();
    ca.B = c->d_B.as<float>();
    ca.rgbx = sums_u8(c) ? c->d_rgbx.as<uint32_t>() : nullptr;
    ca.sums = c->d_sums.as<unsigned long long>();
    ca.bad = reinterpret_cast<int*>(c->d_sums.as<int64_t>() + (size_t)P * K * 4);
    ca.idx_pitch = g.idx_pitch;
    ca.q0 = (uint32_t)((int64_t)(g.r0 - g.e0) * g.W);
    ca.q1 = ca.q0 + (uint32_t)((int64_t)g.W * (g.r1 - g.r0));
    ca.P = P;
    ca.K = K;
    return ca;
}

// hq_cluster_sums into `out` ([P][K][4]); nothing is written unless HQ_OK.
int cluster_sums(hq_ctx* c, int P, int K, int64_t* out, int64_t* den) {
    if (!c->have_image || !c->sums_ok)
        return fail(c, HQ_ERR_STATE, "no population evaluated by hq_eval_population[_partial] on this image "
                                     "since the last search run");
    if (P != c->last_P || K != c->K_cur)
        return fail(c, HQ_ERR_STATE, "P=%d, K=%d: the last evaluation had P=%d, K=%d", P, K, c->last_P, c->K_cur);
    if (c->slice_n != c->last_P || c->slice_ranks > 1 || (c->psplit && c->comm))
        return fail(c, HQ_ERR_UNSUPPORTED, "palette slice: this device holds %d of the %d index images",
                    c->slice_n, c->last_P);
    int rc = bind(c);
    if (rc) return rc;
    hipStream_t s = c->stream;
    const size_t n4 = (size_t)P * K * 4;
    HIP_TRY(c, c->d_sums.ensure(sizeof(int64_t) * (n4 + 1)));
    HIP_TRY(c, hipMemsetAsync(c->d_sums.p, 0, sizeof(int64_t) * (n4 + 1), s));
    int idx_bytes = 1;
    const ClusterArgs ca = cluster_args(c, P, K, &idx_bytes);
    const bool u8 = sums_u8(c);
    if (c->prof) set_launch_events(c->ev[12], c->ev[13]);
    const hipError_t e = launch_cluster_sums(ca, idx_bytes, c->num_cu, s);
    set_launch_events(nullptr, nullptr);
    HIP_TRY(c, e);
    std::vector<int64_t> h(n4 + 1);
    HIP_TRY(c, hipMemcpyAsync(h.data(), c->d_sums.p, sizeof(int64_t) * (n4 + 1), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    if (c->prof) prof_add(c, c->prof_centroid, c->ev[12], c->ev[13]);
    if (h[n4] != 0)
        return fail(c, HQ_ERR_UNSUPPORTED, "planar image with a pixel outside [0, 1] or not finite: no exact sums");
    std::memcpy(out, h.data(), sizeof(int64_t) * n4);
    *den = u8 ? 255 : (int64_t)1 << 32;
    return HQ_OK;
}

// The error kernel's arguments for the index images, the error image and the
// prepared palettes of the last evaluation of P palettes of K colours, into
// d_errstat ([P][K][4], then the flag) and d_worst ([P][K]).
ClusterErrArgs cluster_err_args(hq_ctx* c, int P, int K, int* idx_bytes) {
    const Geom& g = c->g;
    const ClusterArgs ca = cluster_args(c, P, K, idx_bytes);
    ClusterErrArgs ea{};
    ea.idx = ca.idx;
    ea.R = ca.R;
    ea.G = ca.G;
    ea.B = ca.B;
    ea.rgbx = ca.rgbx;
    ea.pix_err = c->d_pixerr.as<float>();
    ea.pal = c->d_pal.as<float4>();
    ea.stats = c->d_errstat.as<unsigned long long>();
    ea.worst = c->d_worst.as<float4>();
    ea.bad = reinterpret_cast<int*>(c->d_errstat.as<int64_t>() + (size_t)P * K * 4);
    ea.idx_pitch = g.idx_pitch;
    ea.err_pitch = (int64_t)g.W * (g.r1 - g.r0);
    // chunked palettes: a palette's nch sub-palettes of 256 lie back to back, colour k at k
    ea.pal_pitch = c->last_nch > 1 ? (int64_t)c->last_nch * kMaxK : std::max(K, kMaxK);
    ea.q0 = ca.q0;
    ea.q1 = ca.q1;
    ea.pos0 = (uint32_t)((int64_t)g.e0 * g.W);
    ea.P = P;
    ea.K = K;
    return ea;
}

// hq_cluster_errors into err ([P][K][4]) and worst ([P][K][4]); nothing is written
// unless HQ_OK, or -- ignore_bad, the repair move inside a search -- whatever the
// flag says (the pixels it stands for are left out either way).  The index
// images, the error image, the counter sets and d_sums stay what they are.
int cluster_errors(hq_ctx* c, int P, int K, int64_t* err, float* worst, bool ignore_bad = false) {
    if (!c->have_image || !c->sums_ok)
        return fail(c, HQ_ERR_STATE, "no population evaluated by hq_eval_population[_partial] on this image "
                                     "since the last search run");
    if (P != c->last_P || K != c->K_cur)
        return fail(c, HQ_ERR_STATE, "P=%d, K=%d: the last evaluation had P=%d, K=%d", P, K, c->last_P, c->K_cur);
    const Geom& g = c->g;
    const int64_t n_own = (int64_t)g.W * (g.r1 - g.r0);
    if (!c->err_ok || c->d_pixerr.bytes < sizeof(float) * (size_t)P * (size_t)n_own)
        return fail(c, HQ_ERR_STATE, "option pixel_err was off at the last evaluation: no error image");
    if (c->slice_n != c->last_P || c->slice_ranks > 1 || (c->psplit && c->comm))
        return fail(c, HQ_ERR_UNSUPPORTED, "palette slice: this device holds %d of the %d index images",
                    c->slice_n, c->last_P);
    if ((int64_t)g.W * g.H >= ((int64_t)1 << 32))
        return fail(c, HQ_ERR_UNSUPPORTED, "image of 2^32 pixels or more: a position does not fit 32 bits");
    int rc = bind(c);
    if (rc) return rc;
    hipStream_t s = c->stream;
    const size_t n4 = (size_t)P * K * 4;
    HIP_TRY(c, c->d_errstat.ensure(sizeof(int64_t) * (n4 + 1)));
    HIP_TRY(c, c->d_worst.ensure(sizeof(float) * n4));
    HIP_TRY(c, hipMemsetAsync(c->d_errstat.p, 0, sizeof(int64_t) * (n4 + 1), s));
    int idx_bytes = 1;
    const ClusterErrArgs ea = cluster_err_args(c, P, K, &idx_bytes);
    if (c->prof && !c->ev_err[0])
        for (auto& e : c->ev_err) HIP_TRY(c, hipEventCreate(&e));
    if (c->prof) set_launch_events(c->ev_err[0], c->ev_err[1]);
    const hipError_t e = launch_cluster_errors(ea, idx_bytes, c->num_cu, s);
    set_launch_events(nullptr, nullptr);
    HIP_TRY(c, e);
    std::vector<uint64_t> h(n4 + 1);
    std::vector<float> hw(n4);
    HIP_TRY(c, hipMemcpyAsync(h.data(), c->d_errstat.p, sizeof(int64_t) * (n4 + 1), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(hw.data(), c->d_worst.p, sizeof(float) * n4, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    if (c->prof) prof_add(c, c->prof_errsum, c->ev_err[0], c->ev_err[1]);
    if (h[n4] != 0 && !ignore_bad)
        return fail(c, HQ_ERR_UNSUPPORTED, "a pixel's dE is not a finite number below 2^20 (dE94's NaN, a non-finite "
                                           "colour or LabRef): no exact error sums");
    for (size_t i = 0; i < n4; i += 4) {
        const uint64_t key = h[i + 2];
        err[i] = (int64_t)h[i];
        err[i + 1] = (int64_t)h[i + 1];
        err[i + 2] = (int64_t)(key >> 32);
        err[i + 3] = key ? (int64_t)(0xffffffffu - (uint32_t)key) : -1;
    }
    std::memcpy(worst, hw.data(), sizeof(float) * n4);
    return HQ_OK;
}

// hq_color_histogram into `out` ([2^(3 bits)][4]); nothing is written unless
// HQ_OK.  The image buffers are read, a table of its own is written: the index
// images, the counter sets and d_sums stay what they are.
int color_histogram(hq_ctx* c, int bits, int64_t* out, int64_t* den) {
    int rc = bind(c);
    if (rc) return rc;
    hipStream_t s = c->stream;
    const Geom& g = c->g;
    const size_t n4 = (size_t)4 << (3 * bits);
    HIP_TRY(c, c->d_hist.ensure(sizeof(int64_t) * (n4 + 1)));
    HIP_TRY(c, hipMemsetAsync(c->d_hist.p, 0, sizeof(int64_t) * (n4 + 1), s));
    const bool u8 = sums_u8(c);
    HistArgs ha{};
    ha.R = c->d_R.as<float>();
    ha.G = c->d_G.as<float>();
    ha.B = c->d_B.as<float>();
    ha.rgbx = u8 ? c->d_rgbx.as<uint32_t>() : nullptr;
    ha.cells = c->d_hist.as<unsigned long long>();
    ha.bad = reinterpret_cast<int*>(c->d_hist.as<int64_t>() + n4);
    ha.q0 = (uint32_t)((int64_t)(g.r0 - g.e0) * g.W);
    ha.q1 = ha.q0 + (uint32_t)((int64_t)g.W * (g.r1 - g.r0));
    ha.bits = bits;
    if (c->prof) set_launch_events(c->ev_hist[0], c->ev_hist[1]);
    const hipError_t e = launch_color_histogram(ha, c->num_cu, s);
    set_launch_events(nullptr, nullptr);
    HIP_TRY(c, e);
    std::vector<int64_t> h(n4 + 1);
    HIP_TRY(c, hipMemcpyAsync(h.data(), c->d_hist.p, sizeof(int64_t) * (n4 + 1), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    if (c->prof) prof_add(c, c->prof_hist, c->ev_hist[0], c->ev_hist[1]);
    if (h[n4] != 0)
        return fail(c, HQ_ERR_UNSUPPORTED, "planar image with a pixel outside [0, 1] or not finite: no exact sums");
    std::memcpy(out, h.data(), sizeof(int64_t) * n4);
    *den = u8 ? 255 : (int64_t)1 << 32;
    return HQ_OK;
}

}  // namespace

namespace {

// The chunk count of the population being enqueued, for one search call.
struct NchScope {
    hq_ctx* c;
    NchScope(hq_ctx* cc, int nch) : c(cc) { c->nch_cur = nch; }
    ~NchScope() { c->nch_cur = 1; }
};

// The arguments of an SA step: accept the population in cand[cd] (if `accept`,
// its counters in set c->acc_par), then generate the next candidates into
// cand[1 - cd] (if `generate`).
SaArgs sa_args(hq_search* s, bool accept, bool init, bool generate, bool random, float amax) {
    hq_ctx* c = s->ctx;
    SaArgs a{};
    a.out = c->d_out.as<double>();
    a.colors_in = s->colors[s->st].as<float>();
    a.colors_out = s->colors[1 - s->st].as<float>();
    a.cand_in = s->cand[s->cd].as<float>();
    a.cand_out = s->cand[1 - s->cd].as<float>();
    a.err_in = s->err[s->st].as<double>();
    a.err_out = s->err[1 - s->st].as<double>();
    a.seed_in = s->seed[s->st].as<uint64_t>();
    a.seed_out = s->seed[1 - s->st].as<uint64_t>();
    a.best_err_in = s->best_err[s->st].as<double>();
    a.best_err_out = s->best_err[1 - s->st].as<double>();
    a.best_colors = s->best_colors.as<float>();
    a.jump_A = s->jA.as<uint64_t>();
    a.jump_C = s->jC.as<uint64_t>();
    a.prep = prep_args(c, s->nch > 1 ? kMaxK : s->K);
    a.nch = s->nch;
    a.n_total = (double)c->g.W * (double)c->g.H;
    a.keep_threshold = s->keep_acc;
    a.temperature = s->t_acc;
    a.amax = amax;
    a.delta = s->prm.delta;
    a.P = s->P;
    a.K = s->K;
    a.accept = accept;
    a.init = init;
    a.generate = generate;
    a.random = random;
    a.convergence = s->prm.convergence;
    a.acc = acc_base(c, c->acc_par, a.P);
    a.used_glob = used_base(c, c->acc_par, a.P * s->nch);
    a.used_stride = used_stride(a.P * s->nch);
    a.fold = s->fold;
    a.nranks = rank_blocks(c);
    a.acc_rank_words = (int64_t)acc_words(a.P);
    return a;
}

void sa_advance(hq_search* s, bool generate) {
    s->st = 1 - s->st;
    if (generate) s->cd = 1 - s->cd;
}

// One sa_step launch (sa_args).
int enqueue_sa_step(hq_search* s, bool accept, bool init, bool generate, bool random, float amax,
                    const hipEvent_t* ev = nullptr) {
    hq_ctx* c = s->ctx;
    const SaArgs a = sa_args(s, accept, init, generate, random, amax);
    if (ev) set_launch_events(ev[0], ev[1]);
    const hipError_t e = launch_sa_step(a, c->stream);
    set_launch_events(nullptr, nullptr);
    HIP_TRY(c, e);
    sa_advance(s, generate);
    return HQ_OK;
}

int ensure_events(hq_search* s, size_t n) {
    while (s->pev.size() < n) {
        hipEvent_t e;
        HIP_TRY(s->ctx, hipEventCreate(&e));
        s->pev.push_back(e);
    }
    return HQ_OK;
}

// ---- hybrid iterations (hq_search_set_lloyd) -----------------------------------
// The scope of a k-means move is hq_refine_population's: the whole image on
// this context, every palette's index image here.
int lloyd_scope(hq_search* s) {
    hq_ctx* c = s->ctx;
    if (c->have_image && (c->g.r0 != 0 || c->g.r1 != c->g.H))
        return fail(c, HQ_ERR_STATE, "sharded context: a hybrid iteration needs the whole image");
    if (c->comm && c->nranks > 1)
        return fail(c, HQ_ERR_UNSUPPORTED, "hybrid iterations with a communicator of %d ranks", c->nranks);
    if (c->psplit || c->slice_ranks > 1) return fail(c, HQ_ERR_UNSUPPORTED, "hybrid iterations on a palette slice");
    if (!s->driver && s->nch > 1)
        return fail(c, HQ_ERR_UNSUPPORTED, "hybrid iterations of a device-resident search need K <= %d (K = %d): "
                                           "set option sa_device 0 before hq_search_create", kMaxK, s->K);
    return HQ_OK;
}

// A run of `iterations` from iteration `ite` (the last one done) holds an iteration
// that is a multiple of `every`.
bool period_in_run(const hq_search* s, int every, int ite, int iterations) {
    if (every <= 0) return false;
    const int last = (int)std::min<int64_t>((int64_t)ite + iterations, s->prm.imax);
    return last / every > ite / every;
}
// ... a hybrid iteration.
bool lloyd_in_run(const hq_search* s, int ite, int iterations) { return period_in_run(s, s->every, ite, iterations); }

// ---- repair iterations (hq_search_set_repair) ----------------------------------
// hq_repair_population's scope, and a dE type whose costs are numbers.
int repair_scope(hq_search* s) {
    hq_ctx* c = s->ctx;
    if (c->de_type == HQ_DE_CIE94)
        return fail(c, HQ_ERR_UNSUPPORTED, "repair iterations on a dE94 context: its costs are NaN on real images");
    if (c->have_image && (c->g.r0 != 0 || c->g.r1 != c->g.H))
        return fail(c, HQ_ERR_STATE, "sharded context: a repair iteration needs the whole image");
    if (c->comm && c->nranks > 1)
        return fail(c, HQ_ERR_UNSUPPORTED, "repair iterations with a communicator of %d ranks", c->nranks);
    if (c->psplit || c->slice_ranks > 1) return fail(c, HQ_ERR_UNSUPPORTED, "repair iterations on a palette slice");
    if (!s->driver && s->nch > 1)
        return fail(c, HQ_ERR_UNSUPPORTED, "repair iterations of a device-resident search need K <= %d (K = %d): "
                                           "set option sa_device 0 before hq_search_create", kMaxK, s->K);
    if (c->have_image && (int64_t)c->g.W * c->g.H >= ((int64_t)1 << 32))
        return fail(c, HQ_ERR_UNSUPPORTED, "image of 2^32 pixels or more: a position does not fit 32 bits");
    return HQ_OK;
}

// The planar form's sums need every owned pixel finite and in [0, 1]: a property
// of the image, established once per image by one launch of the sums kernel (one
// palette of one colour over the first index image -- any u8 index addresses the
// kernel's LDS table) and a read of its flag.
int planar_in_range(hq_ctx* c) {  // -> c->planar_ok
    if (c->planar_ok < 0) {
        int rc = bind(c);
        if (rc) return rc;
        hipStream_t st = c->stream;
        HIP_TRY(c, c->d_idx.ensure((size_t)c->g.idx_pitch + 256));
        HIP_TRY(c, c->d_sums.ensure(sizeof(int64_t) * (4 + 1)));
        HIP_TRY(c, hipMemsetAsync(c->d_sums.p, 0, sizeof(int64_t) * (4 + 1), st));
        int idx_bytes = 1;
        ClusterArgs ca = cluster_args(c, 1, 1, &idx_bytes);
        ca.idx = c->d_idx.p;  // (the u8 image, whatever the last evaluation's index width)
        HIP_TRY(c, launch_cluster_sums(ca, 1, c->num_cu, st));
        int bad = 1;
        HIP_TRY(c, hipMemcpyAsync(&bad, ca.bad, sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        c->planar_ok = bad == 0;
    }
    return HQ_OK;
}
int lloyd_validate(hq_search* s) {
    hq_ctx* c = s->ctx;
    if (!c->have_image) return fail(c, HQ_ERR_STATE, "no image set (hq_set_image)");
    if (sums_u8(c)) return HQ_OK;
    if (int rc = planar_in_range(c)) return rc;
    if (!c->planar_ok)
        return fail(c, HQ_ERR_UNSUPPORTED, "planar image with a pixel outside [0, 1] or not finite: no exact sums, "
                                           "no hybrid iteration");
    return HQ_OK;
}

// The k-means move of a device-resident hybrid iteration, after the sa_step that
// generated and prepared the candidates (now cand[cd]): the assign-only pass,
// the sums kernel into d_sums (zero on entry: the run's memset, then the update
// kernel's own zeroing) and the update kernel, which prepares the updated
// candidates for the evaluation that follows.  ev: the iteration's events.
int enqueue_lloyd(hq_search* s, const hipEvent_t* ev) {
    hq_ctx* c = s->ctx;
    int rc = enqueue_core(c, s->P, s->K, ev ? ev + kProfLloyd : nullptr, s->fold, true);
    if (rc) return rc;
    int idx_bytes = 1;
    const ClusterArgs ca = cluster_args(c, s->P, s->K, &idx_bytes);
    if (ev) set_launch_events(ev[kProfLloyd + 4], ev[kProfLloyd + 5]);
    hipError_t e = launch_cluster_sums(ca, idx_bytes, c->num_cu, c->stream);
    set_launch_events(nullptr, nullptr);
    HIP_TRY(c, e);
    const LloydArgs la{ca.sums, s->cand[s->cd].as<float>(), prep_args(c, s->K), s->K, sums_u8(c) ? 1 : 0};
    if (ev) set_launch_events(ev[kProfLloyd + 6], ev[kProfLloyd + 7]);
    e = launch_lloyd_update(la, s->P, c->stream);
    set_launch_events(nullptr, nullptr);
    HIP_TRY(c, e);
    return HQ_OK;
}

// The repair move of a device-resident repair iteration, after the sa_step that
// generated and prepared the candidates (now cand[cd]) and after the k-means move
// when the iteration is hybrid too: a full pass that stores the error image
// (option "pixel_err" forced on for it alone), the error kernels into d_errstat
// (zero on entry: the run's memset, then the reseed kernel's own zeroing) and
// d_worst, and the reseed kernel, which prepares the repaired candidates for the
// evaluation that follows.  The flag of pixels without a usable dE is not read:
// they are left out, as the host-driven form leaves them out.
int enqueue_repair(hq_search* s, const hipEvent_t* ev) {
    hq_ctx* c = s->ctx;
    int rc;
    {
        const PixelErrScope scope(c);
        rc = enqueue_core(c, s->P, s->K, ev ? ev + kProfRepair : nullptr, s->fold, false, true);
    }
    if (rc) return rc;
    int idx_bytes = 1;
    const ClusterErrArgs ea = cluster_err_args(c, s->P, s->K, &idx_bytes);
    if (ev) set_launch_events(ev[kProfRepair + 6], ev[kProfRepair + 7]);
    hipError_t e = launch_cluster_errors(ea, idx_bytes, c->num_cu, c->stream);
    set_launch_events(nullptr, nullptr);
    HIP_TRY(c, e);
    const ReseedArgs ra{ea.stats, ea.worst, s->cand[s->cd].as<float>(), prep_args(c, s->K), s->K, s->repair_moves};
    if (ev) set_launch_events(ev[kProfRepair + 8], ev[kProfRepair + 9]);
    e = launch_reseed(ra, s->P, c->stream);
    set_launch_events(nullptr, nullptr);
    HIP_TRY(c, e);
    return HQ_OK;
}

// population: hq_search_create_from's ([P][4K], checked), or null for the random one.
int device_search_create(hq_ctx* c, const hq_swasa_params* params, int K, uint64_t seed, const float* population,
                         hq_search* s) {
    const int P = params->population;
    s->prm = *params;
    s->P = P;
    // no communicator, or row blocks: nothing has to see the finalized sums, so
    // the accept step reads the fixed-point sums itself (one launch less per
    // iteration; row blocks: one all-gather of every rank's counter blocks in
    // place of finalize + the all-reduce of P (1 + K) doubles).  The palette
    // split all-gathers finalized rows.
    s->fold = search_folds(c);
    s->comm = c->comm;
    if (c->slice_ranks > 1 && !c->comm)
        return fail(c, HQ_ERR_STATE, "palette slice without a communicator (test option): no search");
    s->pol = new Swasa(*params, seed);
    const NchScope scope(c, s->nch);
    int rc = ensure_population(c, P, K);
    if (rc) return rc;
    const size_t n4 = (size_t)P * 4 * K;
    for (int i = 0; i < 2; ++i) {
        HIP_TRY(c, s->colors[i].ensure(sizeof(float) * n4));
        HIP_TRY(c, s->cand[i].ensure(sizeof(float) * n4));
        HIP_TRY(c, s->err[i].ensure(sizeof(double) * P));
        HIP_TRY(c, s->seed[i].ensure(sizeof(uint64_t)));
    }
    for (int i = 0; i < 2; ++i) HIP_TRY(c, s->best_err[i].ensure(sizeof(double)));
    HIP_TRY(c, s->best_colors.ensure(sizeof(float) * 4 * K));
    // java.util.Random jumps: n steps = A_n s + C_n (mod 2^48), n = 0 .. 3KP
    const size_t nj = (size_t)3 * K * P + 1;
    std::vector<uint64_t> A(nj), C(nj);
    const uint64_t mask = (1ull << 48) - 1, mult = 0x5DEECE66Dull;
    A[0] = 1;
    C[0] = 0;
    for (size_t n = 1; n < nj; ++n) {
        A[n] = (A[n - 1] * mult) & mask;
        C[n] = (C[n - 1] * mult + 0xBull) & mask;
    }
    HIP_TRY(c, s->jA.upload(A.data(), sizeof(uint64_t) * nj));
    HIP_TRY(c, s->jC.upload(C.data(), sizeof(uint64_t) * nj));
    const uint64_t s0 = (seed ^ mult) & mask;  // JavaRandom::set_seed
    HIP_TRY(c, hipMemcpy(s->seed[0].p, &s0, sizeof s0, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemset(s->err[0].p, 0, sizeof(double) * P));
    if (rank_blocks(c) > 1 && !c->comm) {  // test layout: the blocks no rank fills read zero
        HIP_TRY(c, hipMemsetAsync(c->d_acc.p, 0, c->d_acc.bytes, c->stream));
        HIP_TRY(c, hipMemsetAsync(c->d_used_mask.p, 0, c->d_used_mask.bytes, c->stream));
    }
    for (int i = 0; i < 2; ++i) HIP_TRY(c, hipMemset(s->best_err[i].p, 0, sizeof(double)));
    s->st = s->cd = 0;
    // IM:385-493: random population (SW:40-52), its evaluation, argmin
    if ((rc = enqueue_sa_step(s, false, false, true, true, 0.f))) return rc;
    // A given population takes the random one's place after that step has drawn it (the seed
    // is past the 3 K P draws as always): into the candidate buffer the accept step reads,
    // and through the palette prep as an evaluation uploads it (chunked palettes: pack_chunks'
    // sub-palettes), so the prep's outputs and the duplicate flags are the given colours'.
    std::vector<float> given;  // (.w = 0; read by the copy below until the synchronise)
    if (population) {
        given.assign(population, population + n4);
        for (size_t e = 3; e < n4; e += 4) given[e] = 0.0f;
        hipStream_t st = c->stream;
        HIP_TRY(c, hipMemcpyAsync(s->cand[s->cd].p, given.data(), sizeof(float) * n4, hipMemcpyHostToDevice, st));
        const size_t n_in = s->nch > 1 ? (size_t)P * s->nch * kMaxK : (size_t)P * K;
        if (s->nch > 1) pack_chunks(given.data(), P, K, s->nch, c->h_pal);
        else std::memcpy(c->h_pal, given.data(), sizeof(float) * n4);
        HIP_TRY(c, hipMemcpyAsync(c->d_pal_in.p, c->h_pal, sizeof(float4) * n_in, hipMemcpyHostToDevice, st));
        HIP_TRY(c, launch_prep_palette(prep_args(c, s->nch > 1 ? kMaxK : K), P * s->nch, st));
    }
    if ((rc = enqueue_core(c, P, K, nullptr, s->fold))) return rc;
    if ((rc = enqueue_sa_step(s, true, true, false, false, 0.f))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    s->ite = 0;
    return HQ_OK;
}

// IM:497-568 for up to `iterations` iterations, all enqueued before one sync.
int device_search_run(hq_search* s, int iterations, int* ran) {
    hq_ctx* c = s->ctx;
    int done = 0, rc;
    // The context may have changed since hq_search_create or the last run (an
    // option such as 'grid' or 'assign_blocks_per_cu', a new image): size its
    // work buffers for the current geometry before enqueueing anything.
    if (!c->have_image) return fail(c, HQ_ERR_STATE, "no image set (hq_set_image)");
    const NchScope scope(c, s->nch);
    if ((rc = ensure_population(c, s->P, s->K))) return rc;
    if (s->comm != c->comm || s->fold != search_folds(c))
        return fail(c, HQ_ERR_STATE, "communicator or palette split changed after hq_search_create: "
                                     "recreate the search");
    const bool prof = c->prof;
    if (prof && (rc = ensure_events(s, (size_t)kProfSearchEvents * iterations))) return rc;
    // hybrid iterations in this run: the sums buffer before anything is enqueued
    // (no allocation while a run is captured), zeroed once below -- the update
    // kernel leaves it zero for the next hybrid iteration
    const bool lloyd = lloyd_in_run(s, s->ite, iterations);
    const size_t sums_bytes = sizeof(int64_t) * ((size_t)s->P * s->K * 4 + 1);
    if (lloyd) HIP_TRY(c, c->d_sums.ensure(sums_bytes));
    std::vector<char> hybrid;  // per iteration of this run (profiling: whose extra events were recorded)
    // repair iterations in this run: the same for the error image, the statistics and the
    // worst pixels -- nothing of it without one
    const bool repair = period_in_run(s, s->repair_every, s->ite, iterations);
    const size_t stat_bytes = sizeof(int64_t) * ((size_t)s->P * s->K * 4 + 1);
    if (repair) {
        HIP_TRY(c, c->d_pixerr.ensure(sizeof(float) * (size_t)s->P * std::max<int64_t>((int64_t)c->g.W * (c->g.r1 - c->g.r0), 1)));
        HIP_TRY(c, c->d_errstat.ensure(stat_bytes));
        HIP_TRY(c, c->d_worst.ensure(sizeof(float) * (size_t)s->P * s->K * 4));
    }
    std::vector<char> repairs;
    // option sa_graph: the run's kernels go into one hipGraph (stream capture),
    // replayed as a whole -- a chain of dependent kernels costs ~2.7 us per
    // kernel from the stream and ~1.8 from a graph (profiles/r04_graph_gap_
    // microbench.txt).  The previous run's executable graph is updated in place
    // when the iteration count (the topology) is the same, else instantiated
    // anew.  Not with profiling events (they ride on the launches).
    const bool graph = c->sa_graph && !prof;
    if (graph) HIP_TRY(c, hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
    auto abort_capture = [&](int rc0) {
        if (graph) {
            hipGraph_t gr = nullptr;
            if (hipStreamEndCapture(c->stream, &gr) == hipSuccess && gr) (void)hipGraphDestroy(gr);
        }
        return rc0;
    };
    if (lloyd) {
        const hipError_t e = hipMemsetAsync(c->d_sums.p, 0, sums_bytes, c->stream);
        if (e != hipSuccess) {
            (void)abort_capture(0);
            HIP_TRY(c, e);
        }
    }
    if (repair) {
        const hipError_t e = hipMemsetAsync(c->d_errstat.p, 0, stat_bytes, c->stream);
        if (e != hipSuccess) {
            (void)abort_capture(0);
            HIP_TRY(c, e);
        }
    }
    for (; done < iterations && s->ite < s->prm.imax; ++done) {
        const int ite = ++s->ite;
        s->pol->reduce_temperature_if_necessary(ite);                  // IM:507
        const float amax = s->pol->max_step_width(ite) / 256.0f;       // SW:91-101
        const hipEvent_t* ev = prof ? &s->pev[(size_t)kProfSearchEvents * done] : nullptr;
        // accept the previous iteration's population (none at the first of a run)
        if ((rc = enqueue_sa_step(s, done > 0, false, true, false, amax, ev ? ev + 8 : nullptr)))
            return abort_capture(rc);
        hybrid.push_back(s->every > 0 && ite % s->every == 0);
        if (hybrid.back() && (rc = enqueue_lloyd(s, ev))) return abort_capture(rc);
        repairs.push_back(s->repair_every > 0 && ite % s->repair_every == 0);
        if (repairs.back() && (rc = enqueue_repair(s, ev))) return abort_capture(rc);
        if ((rc = enqueue_core(c, s->P, s->K, ev, s->fold))) return abort_capture(rc);
        s->t_acc = s->pol->temperature();     // SW:54-57 at this iteration
        s->keep_acc = s->pol->keep_threshold(ite);
    }
    if (done > 0 && (rc = enqueue_sa_step(s, true, false, false, false, 0.f))) return abort_capture(rc);
    if (graph) {
        hipGraph_t gr = nullptr;
        HIP_TRY(c, hipStreamEndCapture(c->stream, &gr));
        bool updated = false;
        if (s->gexec && s->gexec_iters == done) {
            hipGraphNode_t err_node = nullptr;
            hipGraphExecUpdateResult res = hipGraphExecUpdateError;
            updated = hipGraphExecUpdate(s->gexec, gr, &err_node, &res) == hipSuccess &&
                      res == hipGraphExecUpdateSuccess;
            if (!updated) (void)hipGetLastError();
        }
        if (!updated) {
            if (s->gexec) (void)hipGraphExecDestroy(s->gexec);
            s->gexec = nullptr;
            const hipError_t e = hipGraphInstantiate(&s->gexec, gr, nullptr, nullptr, 0);
            if (e != hipSuccess) {
                (void)hipGraphDestroy(gr);
                s->gexec = nullptr;
                HIP_TRY(c, e);
            }
            s->gexec_iters = done;
        }
        (void)hipGraphDestroy(gr);
        HIP_TRY(c, hipGraphLaunch(s->gexec, c->stream));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int i = 0; prof && i < done; ++i) {
        const hipEvent_t* ev = &s->pev[(size_t)kProfSearchEvents * i];
        prof_accumulate(c, ev, !s->fold);
        prof_accumulate_sa(c, ev);
        if (repairs[i]) {  // (events of an earlier run's repair iteration may sit in these slots)
            if (c->G2 > 0) prof_add(c, c->prof_grid, ev[kProfRepair], ev[kProfRepair + 1]);
            prof_add(c, c->prof_assign, ev[kProfRepair + 2], ev[kProfRepair + 3]);
            prof_add(c, c->prof_cost, ev[kProfRepair + 4], ev[kProfRepair + 5]);
            prof_add(c, c->prof_errsum, ev[kProfRepair + 6], ev[kProfRepair + 7]);
            prof_add(c, c->prof_reseed, ev[kProfRepair + 8], ev[kProfRepair + 9]);
        }
        if (!hybrid[i]) continue;  // (events of an earlier run's hybrid iteration may sit in these slots)
        if (c->G2 > 0) prof_add(c, c->prof_grid, ev[kProfLloyd], ev[kProfLloyd + 1]);
        prof_add(c, c->prof_assign, ev[kProfLloyd + 2], ev[kProfLloyd + 3]);
        prof_add(c, c->prof_centroid, ev[kProfLloyd + 4], ev[kProfLloyd + 5]);
        prof_add(c, c->prof_lloyd, ev[kProfLloyd + 6], ev[kProfLloyd + 7]);
    }
    if (ran) *ran = done;
    return HQ_OK;
}

}  // namespace

// ============================================================================
// C ABI
// ============================================================================
extern "C" {

int hq_version(void) { return HQ_VERSION; }

const char* hq_status_string(int s) {
    switch (s) {
        case HQ_OK: return "ok";
        case HQ_ERR_ARG: return "invalid argument";
        case HQ_ERR_DEVICE: return "device error";
        case HQ_ERR_STATE: return "invalid state";
        case HQ_ERR_UNSUPPORTED: return "unsupported";
        case HQ_ERR_COMM: return "communication error";
        case HQ_ERR_NOMEM: return "out of memory";
        default: return "unknown status";
    }
}

int hq_device_count(int* count) {
    if (!count) return HQ_ERR_ARG;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    *count = n;
    return HQ_OK;
}

int hq_create(int device, int delta_e_type, hq_ctx** out) {
    if (!out) return HQ_ERR_ARG;
    *out = nullptr;
#ifdef HQ_ABLATION_BUILD
    std::fprintf(stderr, "libhq: ABLATION BUILD (HQ_ABL_*): costs and indices are wrong by design\n");
#endif
    if (delta_e_type < HQ_DE_CIE76 || delta_e_type > HQ_DE_CIEDE2000) return HQ_ERR_ARG;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n)
        return HQ_ERR_DEVICE;
    hq_ctx* c = new hq_ctx();
    c->device = device;
    c->de_type = delta_e_type;
    if (hipSetDevice(device) != hipSuccess ||
        hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return HQ_ERR_DEVICE;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) {
        c->num_cu = prop.multiProcessorCount;
        c->lds_optin = std::max(prop.sharedMemPerBlockOptin, prop.sharedMemPerBlock);
    }
    for (int ng = 1; ng <= 4; ++ng) c->assign_res[ng] = assign_residency(ng);
    c->assign_res_chunked = assign_residency_chunked();
    for (auto& e : c->ev) (void)hipEventCreate(&e);
    for (auto& e : c->ev_hist) (void)hipEventCreate(&e);
    *out = c;
    return HQ_OK;
}

void hq_destroy(hq_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->comm) (void)ncclCommDestroy(c->comm);
    for (DevBuf* b : {&c->d_k1, &c->d_k2, &c->d_k3, &c->d_absk3, &c->d_vtaps, &c->d_R, &c->d_G, &c->d_B, &c->d_rgbx,
                      &c->d_labL, &c->d_labA, &c->d_labB, &c->d_pal_in, &c->d_pal, &c->d_opp, &c->d_opp16,
                      &c->d_dup, &c->d_pflags, &c->d_lvl1, &c->d_lvl2, &c->d_idx,
                      &c->d_used_mask, &c->d_acc, &c->d_out, &c->d_gen_t, &c->d_taps,
                      &c->d_vfrag16, &c->d_vfrag16p, &c->d_vfragm, &c->d_htaps, &c->d_idx32, &c->d_used32, &c->d_pixerr, &c->d_idx16, &c->d_dist, &c->d_l1n, &c->d_l2n, &c->d_sums,
                      &c->d_hist, &c->d_errstat, &c->d_worst, &c->d_dcarry})
        b->release();
    if (c->h_pal) (void)hipHostFree(c->h_pal);
    if (c->h_out) (void)hipHostFree(c->h_out);
    for (auto& e : c->ev)
        if (e) (void)hipEventDestroy(e);
    for (auto& e : c->ev_hist)
        if (e) (void)hipEventDestroy(e);
    for (auto& e : c->ev_err)
        if (e) (void)hipEventDestroy(e);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

const char* hq_last_error(const hq_ctx* c) { return c ? c->err.c_str() : "null context"; }

int hq_set_filters(hq_ctx* c, int taps, const float* k1, const float* k2, const float* k3,
                   const float* absk3) {
    if (!c) return HQ_ERR_ARG;
    if (taps < 1 || taps > kMaxTaps || !k1 || !k2 || !k3 || !absk3)
        return fail(c, HQ_ERR_ARG, "bad filters (taps=%d)", taps);
    int rc = bind(c);
    if (rc) return rc;
    c->taps = taps;
    c->half = (taps * 4) / 8;  // IM:408 filters4[0].length/8
    if (2 * c->half + 1 != taps)
        return fail(c, HQ_ERR_UNSUPPORTED, "even tap count %d (the reference assumes odd)", taps);
    c->k1.assign(k1, k1 + 4 * taps);
    c->k2.assign(k2, k2 + 4 * taps);
    c->k3.assign(k3, k3 + taps);
    c->absk3.assign(absk3, absk3 + taps);
    HIP_TRY(c, c->d_k1.upload(k1, sizeof(float) * 4 * taps));
    HIP_TRY(c, c->d_k2.upload(k2, sizeof(float) * 4 * taps));
    HIP_TRY(c, c->d_k3.upload(k3, sizeof(float) * taps));
    HIP_TRY(c, c->d_absk3.upload(absk3, sizeof(float) * taps));
    {  // the tiled generic path's vertical taps per plane (t1.xyz: k1, t2.xyz: k2, t3: |k3|)
        c->vtap_pitch = (taps + 15) / 16 * 16 + 16;
        std::vector<float> vt((size_t)kNumFilt * c->vtap_pitch, 0.f);
        for (int t = 0; t < taps; ++t) {
            for (int ch = 0; ch < 3; ++ch) {
                vt[(size_t)ch * c->vtap_pitch + t] = k1[4 * t + ch];
                vt[(size_t)(3 + ch) * c->vtap_pitch + t] = k2[4 * t + ch];
            }
            vt[(size_t)6 * c->vtap_pitch + t] = absk3[t];
        }
        HIP_TRY(c, c->d_vtaps.upload(vt.data(), sizeof(float) * vt.size()));
        std::vector<float> ht((size_t)8 * taps);
        for (int t = 0; t < taps; ++t) {
            const float v[8] = {k1[4 * t], k1[4 * t + 1], k1[4 * t + 2], k3[t], k2[4 * t], k2[4 * t + 1], k2[4 * t + 2], 0.f};
            std::copy(v, v + 8, ht.begin() + 8 * t);
        }
        HIP_TRY(c, c->d_htaps.upload(ht.data(), sizeof(float) * ht.size()));
        // gen_vmfma's vertical taps (t3: |k3|), then gen_hmfma's horizontal ones (t3: k3)
        std::vector<uint32_t> fm(2 * vtile_dup_tap_words(c->half));
        build_vtile_dup_taps(c->half, k1, k2, absk3, fm.data());
        build_vtile_dup_taps(c->half, k1, k2, k3, fm.data() + vtile_dup_tap_words(c->half));
        HIP_TRY(c, c->d_vfragm.upload(fm.data(), fm.size() * sizeof(uint32_t)));
    }
    // fast path: the filters centred in the smallest tap bucket that holds them
    // (half-widths up to 24: every dpi / viewing distance of HQ:229-231 up to
    // ~200 dpi at 45 cm); longer filters take the generic path
    c->fast_hb = fast_bucket(c->half);
    c->trim_ok = c->fast_hb > 0 && trim_window_ok(k1, c->half, c->fast_hb);
    c->taps_generic = !taps_fit_split(k1, k2, k3, absk3, taps);
    if (c->fast_hb > 0) {
        const int HB = c->fast_hb;
        std::vector<uint16_t> f16s(vpass_f16_stack_fragment_halves(HB));
        build_vpass_f16_stack_fragments(HB, c->half, k1, k2, k3, absk3, f16s.data());
        HIP_TRY(c, c->d_vfrag16.upload(f16s.data(), f16s.size() * sizeof(uint16_t)));
        std::vector<uint16_t> f16p(vpass_f16_pair_fragment_halves(HB));
        build_vpass_f16_pair_fragments(HB, c->half, k1, k2, k3, absk3, f16p.data());
        HIP_TRY(c, c->d_vfrag16p.upload(f16p.data(), f16p.size() * sizeof(uint16_t)));
        std::vector<char> tb(fast_taps_bytes(HB));
        build_fast_taps(HB, c->half, k1, k2, k3, absk3, tb.data());
        HIP_TRY(c, c->d_taps.upload(tb.data(), tb.size()));
    }
    c->have_image = false;  // halo depends on the filters
    c->sums_ok = false;
    return HQ_OK;
}

int hq_set_image_shard(hq_ctx* c, const float* rgba4, const float* lab4, int w, int h,
                       const float* illum, int row_begin, int row_end) {
    if (!c) return HQ_ERR_ARG;
    if (!rgba4) return fail(c, HQ_ERR_ARG, "null image");
    int rc = check_geom_args(c, w, h, row_begin, row_end);
    if (rc) return rc;
    if ((rc = bind(c))) return rc;
    c->g = make_geom(w, h, row_begin, row_end, c->half);
    std::vector<float> R, G, B;
    gather_rows(rgba4, 4, 0, c->g, R);
    gather_rows(rgba4, 4, 1, c->g, G);
    gather_rows(rgba4, 4, 2, c->g, B);
    return set_image_common(c, R, G, B, lab4, illum);
}

int hq_set_image(hq_ctx* c, const float* rgba4, const float* lab4, int w, int h,
                 const float* illum) {
    return hq_set_image_shard(c, rgba4, lab4, w, h, illum, 0, h);
}

int hq_set_image_planar_shard(hq_ctx* c, const float* R, const float* G, const float* B, int w,
                              int h, const float* illum, int row_begin, int row_end) {
    if (!c) return HQ_ERR_ARG;
    if (!R || !G || !B) return fail(c, HQ_ERR_ARG, "null plane");
    int rc = check_geom_args(c, w, h, row_begin, row_end);
    if (rc) return rc;
    if ((rc = bind(c))) return rc;
    c->g = make_geom(w, h, row_begin, row_end, c->half);
    std::vector<float> r, g, b;
    gather_rows(R, 1, 0, c->g, r);
    gather_rows(G, 1, 0, c->g, g);
    gather_rows(B, 1, 0, c->g, b);
    return set_image_common(c, r, g, b, nullptr, illum);
}

int hq_get_labref(hq_ctx* c, float* lab4) {
    if (!c || !lab4) return HQ_ERR_ARG;
    if (!c->have_image) return fail(c, HQ_ERR_STATE, "no image set");
    int rc = bind(c);
    if (rc) return rc;
    const Geom& g = c->g;
    const int own = g.r1 - g.r0;
    std::vector<float> L((size_t)g.lab_pitch * own), A(L.size()), B(L.size());
    HIP_TRY(c, hipMemcpy(L.data(), c->d_labL.p, sizeof(float) * L.size(), hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(A.data(), c->d_labA.p, sizeof(float) * A.size(), hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(B.data(), c->d_labB.p, sizeof(float) * B.size(), hipMemcpyDeviceToHost));
    for (int y = 0; y < own; ++y)
        for (int x = 0; x < g.W; ++x) {
            const size_t s = (size_t)y * g.lab_pitch + x, d = 4 * ((size_t)y * g.W + x);
            lab4[d] = L[s]; lab4[d + 1] = A[s]; lab4[d + 2] = B[s]; lab4[d + 3] = 0.f;
        }
    return HQ_OK;
}

int hq_eval_population_partial(hq_ctx* c, const float* palettes, int P, int K, double* partial) {
    if (!partial) return fail(c, HQ_ERR_ARG, "null output");
    int rc = eval_partial_into_hout(c, palettes, P, K);
    if (rc) return rc;
    std::memcpy(partial, c->h_out, sizeof(double) * (size_t)P * (1 + K));
    return HQ_OK;
}

// IM:712 from the [P][1+K] rows in h_out: averageArray(error) + computePenalty(used).
// After an all-reduce the used entries count the ranks using colour k; unused <=> 0.
static void costs_from_hout(const hq_ctx* c, int P, int K, float delta, double* costs, int32_t* used) {
    const double n_total = (double)c->g.W * (double)c->g.H;
    for (int p = 0; p < P; ++p) {
        const double* o = c->h_out + (size_t)p * (1 + K);
        double penalty = 0.0;
        for (int k = 0; k < K; ++k) {
            const bool u = o[1 + k] != 0.0;
            if (!u) penalty += delta;
            if (used) used[(size_t)p * K + k] = u ? 1 : 0;
        }
        costs[p] = o[0] / n_total + penalty;
    }
}

int hq_eval_population(hq_ctx* c, const float* palettes, int P, int K, float delta,
                       double* costs, int32_t* used) {
    if (!costs) return fail(c, HQ_ERR_ARG, "null output");
    int rc = eval_partial_into_hout(c, palettes, P, K);
    if (rc) return rc;
    const bool full = c->g.r0 == 0 && c->g.r1 == c->g.H;
    if ((!full || c->slice_ranks > 1) && !(c->comm && c->nranks > 1))
        return fail(c, HQ_ERR_STATE, "sharded context or palette slice without a communicator: use "
                                     "hq_eval_population_partial");
    costs_from_hout(c, P, K, delta, costs, used);
    return HQ_OK;
}

int hq_dither_population(hq_ctx* c, const float* palettes, int P, int K, float strength, float delta,
                         double* costs, int32_t* used) {
    if (!c) return HQ_ERR_ARG;
    if (!palettes || !costs || P < 1 || K < 1) return fail(c, HQ_ERR_ARG, "bad palettes / costs / P=%d / K=%d", P, K);
    if (!(strength >= 0.0f && strength <= 1.0f)) return fail(c, HQ_ERR_ARG, "strength %g not in [0, 1]", strength);
    if (!c->have_image) return fail(c, HQ_ERR_STATE, "no image set (hq_set_image)");
    if (c->g.r0 != 0 || c->g.r1 != c->g.H)
        return fail(c, HQ_ERR_STATE, "sharded context: error diffusion needs the whole image");
    if (c->comm && c->nranks > 1)
        return fail(c, HQ_ERR_UNSUPPORTED, "hq_dither_population with a communicator of %d ranks", c->nranks);
    if (c->psplit || c->slice_ranks > 1) return fail(c, HQ_ERR_UNSUPPORTED, "hq_dither_population on a palette slice");
    if (K > kMaxK)
        return fail(c, HQ_ERR_UNSUPPORTED, "K=%d > %d: the dither kernel keeps the palette in LDS and writes "
                                           "8-bit indices", K, kMaxK);
    if (!population_in_range(palettes, P, K))
        return fail(c, HQ_ERR_ARG, "palette with a channel that is not finite or outside [0, 1]");
    int rc = bind(c);
    if (rc) return rc;
    // the errors stay bounded (|e| <= 1) for pixels in [0, 1]: a property of the image, established
    // once per image as the hybrid search's is (the packed 8-bit copy exists only for k/255 images)
    if (!c->img_u8) {
        if ((rc = planar_in_range(c))) return rc;
        if (!c->planar_ok)
            return fail(c, HQ_ERR_UNSUPPORTED, "image with a pixel outside [0, 1] or not finite: no error diffusion");
    }
    c->nch_cur = 1;
    c->pal_generic = false;
    if ((rc = ensure_population(c, P, K))) return rc;
    HIP_TRY(c, c->d_dcarry.ensure(sizeof(float) * (size_t)P * 3 * c->g.W));
    std::memcpy(c->h_pal, palettes, sizeof(float) * 4 * (size_t)P * K);
    hipStream_t s = c->stream;
    c->sums_ok = c->err_ok = false;  // (a k-means or repair move from a dithered assignment is neither)
    HIP_TRY(c, hipMemcpyAsync(c->d_pal_in.p, c->h_pal, sizeof(float4) * (size_t)P * K, hipMemcpyHostToDevice, s));
    HIP_TRY(c, launch_prep_palette(prep_args(c, K), P, s));
    const hipEvent_t* ev = c->prof ? c->ev : nullptr;
    if ((rc = enqueue_core(c, P, K, ev, false, false, false, &strength))) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->h_out, c->d_out.p, sizeof(double) * (size_t)P * (1 + K), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    if (ev) {
        prof_add(c, c->prof_dither, ev[2], ev[3]);
        prof_add(c, c->prof_cost, ev[4], ev[5]);
        prof_add(c, c->prof_finalize, ev[6], ev[7]);
        if (c->comm) prof_add(c, c->prof_comm, ev[10], ev[11]);
    }
    costs_from_hout(c, P, K, delta, costs, used);
    return HQ_OK;
}

int hq_get_indices(hq_ctx* c, int p, uint8_t* idx) {
    if (!c || !idx) return HQ_ERR_ARG;
    if (p < 0 || p >= c->last_P) return fail(c, HQ_ERR_ARG, "palette %d not in last population", p);
    if (p < c->slice_lo || p >= c->slice_lo + c->slice_n)
        return fail(c, HQ_ERR_ARG, "palette %d was evaluated on another rank (palette split)", p);
    p -= c->slice_lo;
    if (c->K_cur > kMaxK)
        return fail(c, HQ_ERR_STATE, "K=%d > 256: indices are 32-bit (hq_get_indices32)", c->K_cur);
    int rc = bind(c);
    if (rc) return rc;
    const Geom& g = c->g;
    const int64_t off = (int64_t)(g.r0 - g.e0) * g.W;
    const int64_t n_own = (int64_t)g.W * (g.r1 - g.r0);
    HIP_TRY(c, hipMemcpy(idx, c->d_idx.as<uint8_t>() + (int64_t)p * g.idx_pitch + off, n_own,
                         hipMemcpyDeviceToHost));
    return HQ_OK;
}

int hq_get_indices32(hq_ctx* c, int p, uint32_t* idx) {
    if (!c || !idx) return HQ_ERR_ARG;
    if (p < 0 || p >= c->last_P) return fail(c, HQ_ERR_ARG, "palette %d not in last population", p);
    if (p < c->slice_lo || p >= c->slice_lo + c->slice_n)
        return fail(c, HQ_ERR_ARG, "palette %d was evaluated on another rank (palette split)", p);
    p -= c->slice_lo;
    int rc = bind(c);
    if (rc) return rc;
    const Geom& g = c->g;
    const int64_t off = (int64_t)(g.r0 - g.e0) * g.W;
    const int64_t n_own = (int64_t)g.W * (g.r1 - g.r0);
    if (c->last_nch > 1) {  // chunked palettes: 16-bit indices
        std::vector<uint16_t> b((size_t)n_own);
        HIP_TRY(c, hipMemcpy(b.data(), c->d_idx16.as<uint16_t>() + (int64_t)p * g.idx_pitch + off,
                             sizeof(uint16_t) * n_own, hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < n_own; ++i) idx[i] = b[i];
        return HQ_OK;
    }
    if (c->K_cur > kMaxK) {
        HIP_TRY(c, hipMemcpy(idx, c->d_idx32.as<uint32_t>() + (int64_t)p * g.idx_pitch + off,
                             sizeof(uint32_t) * n_own, hipMemcpyDeviceToHost));
        return HQ_OK;
    }
    std::vector<uint8_t> b((size_t)n_own);
    HIP_TRY(c, hipMemcpy(b.data(), c->d_idx.as<uint8_t>() + (int64_t)p * g.idx_pitch + off, n_own,
                         hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < n_own; ++i) idx[i] = b[i];
    return HQ_OK;
}

int hq_get_pixel_errors(hq_ctx* c, int p, float* err) {
    if (!c || !err) return HQ_ERR_ARG;
    if (!c->pixel_err) return fail(c, HQ_ERR_STATE, "option pixel_err is off");
    if (p < 0 || p >= c->last_P) return fail(c, HQ_ERR_ARG, "palette %d not in last population", p);
    if (p < c->slice_lo || p >= c->slice_lo + c->slice_n)
        return fail(c, HQ_ERR_ARG, "palette %d was evaluated on another rank (palette split)", p);
    p -= c->slice_lo;
    if (c->d_pixerr.bytes < sizeof(float) * (size_t)c->last_P * (size_t)c->g.W * (c->g.r1 - c->g.r0))
        return fail(c, HQ_ERR_STATE, "pixel_err was set after the last evaluation");
    int rc = bind(c);
    if (rc) return rc;
    const int64_t n_own = (int64_t)c->g.W * (c->g.r1 - c->g.r0);
    HIP_TRY(c, hipMemcpy(err, c->d_pixerr.as<float>() + (int64_t)p * n_own, sizeof(float) * n_own,
                         hipMemcpyDeviceToHost));
    return HQ_OK;
}

int hq_cluster_sums(hq_ctx* c, int P, int K, int64_t* sums, int64_t* den) {
    if (!c) return HQ_ERR_ARG;
    if (!sums || !den || P < 1 || K < 1) return fail(c, HQ_ERR_ARG, "bad sums / den / P=%d / K=%d", P, K);
    return cluster_sums(c, P, K, sums, den);
}

int hq_color_histogram(hq_ctx* c, int bits, int64_t* cells, int64_t* den) {
    if (!c) return HQ_ERR_ARG;
    if (!cells || !den || bits < 2 || bits > 6) return fail(c, HQ_ERR_ARG, "bad cells / den / bits=%d (2 .. 6)", bits);
    if (!c->have_image) return fail(c, HQ_ERR_STATE, "no image set (hq_set_image)");
    return color_histogram(c, bits, cells, den);
}

int hq_refine_population(hq_ctx* c, float* palettes, int P, int K, int steps, float delta, int keep_best,
                         double* costs, int32_t* used, double* trace) {
    if (!costs) return fail(c, HQ_ERR_ARG, "null output");
    int rc = check_eval_args(c, palettes, P, K);
    if (rc) return rc;
    if (steps < 0) return fail(c, HQ_ERR_ARG, "steps=%d < 0", steps);
    if (c->comm && c->nranks > 1)
        return fail(c, HQ_ERR_UNSUPPORTED, "hq_refine_population with a communicator of %d ranks: add the "
                                           "shards' hq_cluster_sums yourself", c->nranks);
    if (c->slice_ranks > 1) return fail(c, HQ_ERR_UNSUPPORTED, "hq_refine_population on a palette slice");
    if (c->g.r0 != 0 || c->g.r1 != c->g.H)
        return fail(c, HQ_ERR_STATE, "sharded context: hq_refine_population needs the whole image");
    const size_t n4 = (size_t)P * K * 4, nu = (size_t)P * K;
    std::vector<float> cur(palettes, palettes + n4), best_pal;
    std::vector<double> cst(P), best_cost;
    std::vector<int32_t> usd(nu), best_used;
    std::vector<int64_t> sums(n4);
    if ((rc = hq_eval_population(c, cur.data(), P, K, delta, cst.data(), usd.data()))) return rc;
    if (trace) std::copy(cst.begin(), cst.end(), trace);
    if (keep_best) best_pal = cur, best_cost = cst, best_used = usd;
    for (int s = 1; s <= steps; ++s) {
        int64_t den = 0;
        if ((rc = cluster_sums(c, P, K, sums.data(), &den))) return rc;
        if ((rc = hq_centroids_from_sums(sums.data(), den, P, K, cur.data())))
            return fail(c, rc, "hq_centroids_from_sums failed");
        if ((rc = hq_eval_population(c, cur.data(), P, K, delta, cst.data(), usd.data()))) return rc;
        if (trace) std::copy(cst.begin(), cst.end(), trace + (size_t)s * P);
        for (int p = 0; keep_best && p < P; ++p) {
            // strictly lower (the earliest step keeps a tie); a number beats a NaN, never the reverse
            const double a = cst[p], b = best_cost[p];
            if (!(a < b || (b != b && a == a))) continue;
            best_cost[p] = a;
            std::copy(cur.begin() + (size_t)p * K * 4, cur.begin() + (size_t)(p + 1) * K * 4,
                      best_pal.begin() + (size_t)p * K * 4);
            std::copy(usd.begin() + (size_t)p * K, usd.begin() + (size_t)(p + 1) * K, best_used.begin() + (size_t)p * K);
        }
    }
    const std::vector<float>& rp = keep_best ? best_pal : cur;
    const std::vector<double>& rc_ = keep_best ? best_cost : cst;
    const std::vector<int32_t>& ru = keep_best ? best_used : usd;
    std::copy(rp.begin(), rp.end(), palettes);
    std::copy(rc_.begin(), rc_.end(), costs);
    if (used) std::copy(ru.begin(), ru.end(), used);
    return HQ_OK;
}

int hq_cluster_errors(hq_ctx* c, int P, int K, int64_t* err, float* worst_rgb) {
    if (!c) return HQ_ERR_ARG;
    if (!err || !worst_rgb || P < 1 || K < 1) return fail(c, HQ_ERR_ARG, "bad err / worst_rgb / P=%d / K=%d", P, K);
    return cluster_errors(c, P, K, err, worst_rgb);
}

int hq_repair_population(hq_ctx* c, float* palettes, int P, int K, int steps, float delta, int max_moves,
                         int keep_best, double* costs, int32_t* used, double* trace) {
    if (!costs) return fail(c, HQ_ERR_ARG, "null output");
    int rc = check_eval_args(c, palettes, P, K);
    if (rc) return rc;
    if (steps < 0) return fail(c, HQ_ERR_ARG, "steps=%d < 0", steps);
    if (c->comm && c->nranks > 1)
        return fail(c, HQ_ERR_UNSUPPORTED, "hq_repair_population with a communicator of %d ranks: merge the "
                                           "shards' hq_cluster_errors yourself", c->nranks);
    if (c->slice_ranks > 1) return fail(c, HQ_ERR_UNSUPPORTED, "hq_repair_population on a palette slice");
    if (c->g.r0 != 0 || c->g.r1 != c->g.H)
        return fail(c, HQ_ERR_STATE, "sharded context: hq_repair_population needs the whole image");
    const PixelErrScope scope(c);  // the evaluations below store their error images
    const size_t n4 = (size_t)P * K * 4, nu = (size_t)P * K;
    std::vector<float> cur(palettes, palettes + n4), best_pal, worst(n4);
    std::vector<double> cst(P), best_cost;
    std::vector<int32_t> usd(nu), best_used;
    std::vector<int64_t> err(n4);
    std::vector<int> moved(P);
    if ((rc = hq_eval_population(c, cur.data(), P, K, delta, cst.data(), usd.data()))) return rc;
    if (trace) std::copy(cst.begin(), cst.end(), trace);
    if (keep_best) best_pal = cur, best_cost = cst, best_used = usd;
    for (int s = 1; s <= steps; ++s) {
        if ((rc = cluster_errors(c, P, K, err.data(), worst.data()))) return rc;
        if ((rc = hq_reseed_unused(err.data(), worst.data(), P, K, max_moves, cur.data(), moved.data())))
            return fail(c, rc, "hq_reseed_unused failed");
        if (std::all_of(moved.begin(), moved.end(), [](int m) { return m == 0; })) {
            // nothing left to repair: the remaining steps repeat this one
            for (int t = s; trace && t <= steps; ++t) std::copy(cst.begin(), cst.end(), trace + (size_t)t * P);
            break;
        }
        if ((rc = hq_eval_population(c, cur.data(), P, K, delta, cst.data(), usd.data()))) return rc;
        if (trace) std::copy(cst.begin(), cst.end(), trace + (size_t)s * P);
        for (int p = 0; keep_best && p < P; ++p) {
            // strictly lower (the earliest step keeps a tie); a number beats a NaN, never the reverse
            const double a = cst[p], b = best_cost[p];
            if (!(a < b || (b != b && a == a))) continue;
            best_cost[p] = a;
            std::copy(cur.begin() + (size_t)p * K * 4, cur.begin() + (size_t)(p + 1) * K * 4,
                      best_pal.begin() + (size_t)p * K * 4);
            std::copy(usd.begin() + (size_t)p * K, usd.begin() + (size_t)(p + 1) * K, best_used.begin() + (size_t)p * K);
        }
    }
    const std::vector<float>& rp = keep_best ? best_pal : cur;
    const std::vector<double>& rc_ = keep_best ? best_cost : cst;
    const std::vector<int32_t>& ru = keep_best ? best_used : usd;
    std::copy(rp.begin(), rp.end(), palettes);
    std::copy(rc_.begin(), rc_.end(), costs);
    if (used) std::copy(ru.begin(), ru.end(), used);
    return HQ_OK;
}

int hq_rgb_to_xyz(hq_ctx* c, const float* R, const float* G, const float* B, int64_t n,
                  float* xyz4) {
    if (!c || !R || !G || !B || !xyz4 || n < 1) return HQ_ERR_ARG;
    int rc = bind(c);
    if (rc) return rc;
    DevBuf dr, dg, db, dx;
    HIP_TRY(c, dr.ensure(sizeof(float) * n));
    HIP_TRY(c, dg.ensure(sizeof(float) * n));
    HIP_TRY(c, db.ensure(sizeof(float) * n));
    HIP_TRY(c, dx.ensure(sizeof(float4) * n));
    HIP_TRY(c, hipMemcpyAsync(dr.p, R, sizeof(float) * n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(dg.p, G, sizeof(float) * n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(db.p, B, sizeof(float) * n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, launch_rgb_to_xyz(dr.as<float>(), dg.as<float>(), db.as<float>(), dx.as<float4>(), n,
                                 c->stream));
    HIP_TRY(c, hipMemcpyAsync(xyz4, dx.p, sizeof(float4) * n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return HQ_OK;
}

int hq_xyz_to_scielab(hq_ctx* c, const float* xyz4, int w, int h, const float* illum,
                      float* lab4) {
    if (!c || !xyz4 || !lab4) return HQ_ERR_ARG;
    int rc = check_geom_args(c, w, h, 0, h);
    if (rc) return rc;
    if ((rc = bind(c))) return rc;
    const Geom g = make_geom(w, h, 0, h, c->half);
    const int64_t n = (int64_t)w * h;
    DevBuf dxyz, opp, tmp, conv, k3v, ak3v;
    HIP_TRY(c, dxyz.ensure(sizeof(float4) * n));
    HIP_TRY(c, opp.ensure(sizeof(float4) * n));
    HIP_TRY(c, tmp.ensure(sizeof(float4) * n));
    HIP_TRY(c, conv.ensure(sizeof(float4) * n));
    std::vector<float> k3h(4 * c->taps, 0.f), ak3h(4 * c->taps, 0.f);
    for (int t = 0; t < c->taps; ++t) { k3h[4 * t] = c->k3[t]; ak3h[4 * t] = c->absk3[t]; }
    HIP_TRY(c, k3v.ensure(sizeof(float) * k3h.size()));
    HIP_TRY(c, ak3v.ensure(sizeof(float) * ak3h.size()));
    HIP_TRY(c, hipMemcpyAsync(k3v.p, k3h.data(), sizeof(float) * k3h.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(ak3v.p, ak3h.data(), sizeof(float) * ak3h.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(dxyz.p, xyz4, sizeof(float4) * n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, launch_xyz_to_opp(dxyz.as<float4>(), opp.as<float4>(), n, c->stream));
    const float* hk[3] = {c->d_k1.as<float>(), c->d_k2.as<float>(), k3v.as<float>()};
    const float* vk[3] = {c->d_k1.as<float>(), c->d_k2.as<float>(), ak3v.as<float>()};
    for (int f = 0; f < 3; ++f) {
        const int chans = f < 2 ? 3 : 1;
        HIP_TRY(c, launch_labref_hconv(opp.as<float4>(), tmp.as<float4>(), hk[f], c->half, chans,
                                       w, n, c->stream));
        HIP_TRY(c, launch_labref_vconv(tmp.as<float4>(), conv.as<float4>(), vk[f], c->half, chans,
                                       f > 0, g, c->stream));
    }
    const float* il = illum ? illum : c->illum;
    HIP_TRY(c, launch_labref_lab(conv.as<float4>(), nullptr, nullptr, nullptr, dxyz.as<float4>(), w,
                                 n, 0, il, c->stream));
    HIP_TRY(c, hipMemcpyAsync(lab4, dxyz.p, sizeof(float4) * n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return HQ_OK;
}

int hq_quantize(hq_ctx* c, const float* rgba4, int64_t n, const float* colors, int K, float* out4,
                int32_t* used) {
    if (!c || !rgba4 || !colors || !out4 || n < 1 || K < 1) return HQ_ERR_ARG;
    int rc = bind(c);
    if (rc) return rc;
    DevBuf din, dcol, dused, dout;
    HIP_TRY(c, din.ensure(sizeof(float4) * n));
    HIP_TRY(c, dcol.ensure(sizeof(float4) * K));
    HIP_TRY(c, dused.ensure(sizeof(int) * K));
    HIP_TRY(c, dout.ensure(sizeof(float4) * n));
    HIP_TRY(c, hipMemcpyAsync(din.p, rgba4, sizeof(float4) * n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(dcol.p, colors, sizeof(float4) * K, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(dused.p, 0, sizeof(int) * K, c->stream));
    HIP_TRY(c, launch_quantize(din.as<float4>(), dcol.as<float4>(), K, dused.as<int>(),
                               dout.as<float4>(), n, c->stream));
    HIP_TRY(c, hipMemcpyAsync(out4, dout.p, sizeof(float4) * n, hipMemcpyDeviceToHost, c->stream));
    if (used)
        HIP_TRY(c, hipMemcpyAsync(used, dused.p, sizeof(int) * K, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return HQ_OK;
}

int hq_compute_error(hq_ctx* c, const float* orig4, const float* quant4, int64_t n,
                     float* err_img4, double* mean) {
    if (!c || !orig4 || !quant4 || n < 1 || !mean) return HQ_ERR_ARG;
    int rc = bind(c);
    if (rc) return rc;
    const int64_t nb = (n + 255) / 256;
    DevBuf da, db, de, dp;
    HIP_TRY(c, da.ensure(sizeof(float4) * n));
    HIP_TRY(c, db.ensure(sizeof(float4) * n));
    if (err_img4) HIP_TRY(c, de.ensure(sizeof(float4) * n));
    HIP_TRY(c, dp.ensure(sizeof(double) * nb));
    HIP_TRY(c, hipMemcpyAsync(da.p, orig4, sizeof(float4) * n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(db.p, quant4, sizeof(float4) * n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, launch_error_image(da.as<float4>(), db.as<float4>(), err_img4 ? de.as<float4>() : nullptr,
                                  dp.as<double>(), n, c->de_type, c->stream));
    std::vector<double> parts(nb);
    HIP_TRY(c, hipMemcpyAsync(parts.data(), dp.p, sizeof(double) * nb, hipMemcpyDeviceToHost, c->stream));
    if (err_img4)
        HIP_TRY(c, hipMemcpyAsync(err_img4, de.p, sizeof(float4) * n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    double s = 0.0;
    for (double v : parts) s += v;
    *mean = s / (double)n;  // IM:893
    return HQ_OK;
}

int hq_comm_unique_id(unsigned char id[128]) {
    if (!id) return HQ_ERR_ARG;
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
    ncclUniqueId u;
    if (ncclGetUniqueId(&u) != ncclSuccess) return HQ_ERR_COMM;
    std::memcpy(id, &u, 128);
    return HQ_OK;
}

int hq_comm_init(hq_ctx* c, int nranks, int rank, const unsigned char id[128]) {
    if (!c || !id || nranks < 1 || rank < 0 || rank >= nranks) return HQ_ERR_ARG;
    int rc = bind(c);
    if (rc) return rc;
    if (c->comm) { (void)ncclCommDestroy(c->comm); c->comm = nullptr; }
    ncclUniqueId u;
    std::memcpy(&u, id, 128);
    NCCL_TRY(c, ncclCommInitRank(&c->comm, nranks, u, rank));
    c->nranks = nranks;
    c->rank = rank;
    return HQ_OK;
}

int hq_comm_info(hq_ctx* c, int* nranks, int* rank) {
    if (!c || !nranks || !rank) return HQ_ERR_ARG;
    *nranks = 0;
    *rank = -1;
    if (!c->comm) return HQ_OK;
    // what the communicator itself reports, not what hq_comm_init was asked for
    NCCL_TRY(c, ncclCommCount(c->comm, nranks));
    NCCL_TRY(c, ncclCommUserRank(c->comm, rank));
    return HQ_OK;
}

int hq_search_create(hq_ctx* c, const hq_swasa_params* params, int K, uint64_t seed,
                     hq_search** out) {
    return hq_search_create_from(c, params, K, seed, nullptr, out);
}

int hq_search_create_from(hq_ctx* c, const hq_swasa_params* params, int K, uint64_t seed,
                          const float* population, hq_search** out) {
    if (!c || !params || !out) return HQ_ERR_ARG;
    *out = nullptr;
    if (params->population < 1 || params->imax < 1 || params->iTc < 1 || K < 1)
        return fail(c, HQ_ERR_ARG, "bad SWASA parameters");
    if (population && !population_in_range(population, params->population, K))
        return fail(c, HQ_ERR_ARG, "initial population with a channel that is not finite or outside [0, 1]");
    // device-resident: K <= 256, or chunked palettes (256 < K <= 16384); at most
    // kSaMaxP palettes (sa_step's per-palette tables) and kSaMaxSub sub-palettes
    // (its fold reads 8 used words per sub-palette, at most 4 per thread)
    const int nch = K > kMaxK && K <= kMaxKChunked && c->chunked && c->G2 > 0 ? chunk_count(K) : 1;
    const bool device = c->sa_device && params->population <= kSaMaxP && params->population * nch <= kSaMaxSub &&
                        (K <= kMaxK || nch > 1);
    hq_search* s = new hq_search{c, nullptr, K};
    int rc;
    if (device) {
        if (!c->have_image) rc = fail(c, HQ_ERR_STATE, "no image set (hq_set_image)");
        else rc = bind(c);
        if (rc) {
            hq_search_destroy(s);
            return rc;
        }
        const bool full = c->g.r0 == 0 && c->g.r1 == c->g.H;
        if (!full && !(c->comm && c->nranks > 1) && !c->shard_solo) {
            hq_search_destroy(s);
            return fail(c, HQ_ERR_STATE, "sharded context without a communicator");
        }
        s->nch = nch;
        rc = device_search_create(c, params, K, seed, population, s);
    } else {
        const float delta = params->delta;
        auto eval = [c, delta](const float* pal, int P, int KK, double* costs) {
            return hq_eval_population(c, pal, P, KK, delta, costs, nullptr);
        };
        s->driver = new SearchDriver(*params, K, seed, eval);
        // the k-means move, host-driven, is the public triple: an evaluation of the
        // candidates for their argmin (its cost pass is wasted), the sums, the update
        s->driver->set_refine([c, delta](float* pal, int P, int KK) {
            std::vector<double> costs(P);
            std::vector<int64_t> sums((size_t)P * KK * 4);
            int64_t den = 0;
            int rr = hq_eval_population(c, pal, P, KK, delta, costs.data(), nullptr);
            if (!rr) rr = cluster_sums(c, P, KK, sums.data(), &den);
            if (!rr && (rr = hq_centroids_from_sums(sums.data(), den, P, KK, pal)))
                return fail(c, rr, "hq_centroids_from_sums failed");
            return rr;
        });
        // the repair move, host-driven: an evaluation of the candidates that stores their
        // error image, the error statistics (pixels with no usable dE left out) and the rule
        s->driver->set_repair([c, delta, s](float* pal, int P, int KK) {
            const PixelErrScope scope(c);
            std::vector<double> costs(P);
            std::vector<int64_t> err((size_t)P * KK * 4);
            std::vector<float> worst((size_t)P * KK * 4);
            int rr = hq_eval_population(c, pal, P, KK, delta, costs.data(), nullptr);
            if (!rr) rr = cluster_errors(c, P, KK, err.data(), worst.data(), true);
            if (!rr && (rr = hq_reseed_unused(err.data(), worst.data(), P, KK, s->repair_moves, pal, nullptr)))
                return fail(c, rr, "hq_reseed_unused failed");
            return rr;
        });
        s->prm = *params;
        s->P = params->population;
        rc = s->driver->start(population);
    }
    c->sums_ok = false;  // (the search's own evaluations replace the index images)
    if (rc) {
        hq_search_destroy(s);
        return rc;
    }
    *out = s;
    return HQ_OK;
}

int hq_search_run(hq_search* s, int iterations, int* ran) {
    if (!s || iterations < 0) return HQ_ERR_ARG;
    int rc;
    // a hybrid iteration in this run: its scope and the image's validity first, so
    // a refusal leaves the search where it was
    if (s->ctx && lloyd_in_run(s, s->driver ? s->driver->iteration() : s->ite, iterations)) {
        if ((rc = lloyd_scope(s)) || (rc = lloyd_validate(s))) {
            if (ran) *ran = 0;
            return rc;
        }
    }
    if (s->ctx && period_in_run(s, s->repair_every, s->driver ? s->driver->iteration() : s->ite, iterations)) {
        if ((rc = repair_scope(s))) {
            if (ran) *ran = 0;
            return rc;
        }
    }
    if (!s->driver) {
        rc = bind(s->ctx);
        if (!rc) rc = device_search_run(s, iterations, ran);
    } else {
        rc = s->driver->run(iterations, ran, nullptr);
    }
    if (s->ctx) s->ctx->sums_ok = false;  // (hq_cluster_sums: a search run has evaluated since)
    return rc;
}

int hq_search_set_lloyd(hq_search* s, int every) {
    if (!s || !s->ctx) return HQ_ERR_ARG;
    if (every < 0) return fail(s->ctx, HQ_ERR_ARG, "every=%d < 0", every);
    if (every > 0)
        if (int rc = lloyd_scope(s)) return rc;
    s->every = every;
    if (s->driver) s->driver->set_every(every);
    return HQ_OK;
}

int hq_search_set_repair(hq_search* s, int every, int max_moves) {
    if (!s || !s->ctx) return HQ_ERR_ARG;
    if (every < 0) return fail(s->ctx, HQ_ERR_ARG, "every=%d < 0", every);
    if (every > 0)
        if (int rc = repair_scope(s)) return rc;
    s->repair_every = every;
    s->repair_moves = max_moves;
    if (s->driver) s->driver->set_repair_every(every);
    return HQ_OK;
}

int hq_search_best(const hq_search* s, float* colors, double* best_error, int* iteration) {
    if (!s) return HQ_ERR_ARG;
    if (!s->driver) {
        hq_ctx* c = s->ctx;
        int rc = bind(c);
        if (rc) return rc;
        if (colors)
            HIP_TRY(c, hipMemcpy(colors, s->best_colors.p, sizeof(float) * 4 * s->K, hipMemcpyDeviceToHost));
        if (best_error)
            HIP_TRY(c, hipMemcpy(best_error, s->best_err[s->st].p, sizeof(double), hipMemcpyDeviceToHost));
        if (iteration) *iteration = s->ite;
        return HQ_OK;
    }
    if (colors) std::copy(s->driver->best_colors().begin(), s->driver->best_colors().end(), colors);
    if (best_error) *best_error = s->driver->best_error();
    if (iteration) *iteration = s->driver->iteration();
    return HQ_OK;
}

void hq_search_destroy(hq_search* s) {
    if (!s) return;
    if (!s->driver && s->ctx) {
        (void)hipSetDevice(s->ctx->device);
        (void)hipStreamSynchronize(s->ctx->stream);
    }
    for (hipEvent_t e : s->pev) (void)hipEventDestroy(e);
    if (s->gexec) (void)hipGraphExecDestroy(s->gexec);
    for (DevBuf* b : {&s->colors[0], &s->colors[1], &s->cand[0], &s->cand[1], &s->err[0], &s->err[1],
                      &s->seed[0], &s->seed[1], &s->best_err[0], &s->best_err[1], &s->best_colors, &s->jA,
                      &s->jC})
        b->release();
    delete s->pol;
    delete s->driver;
    delete s;
}

int hq_profile_enable(hq_ctx* c, int on) {
    if (!c) return HQ_ERR_ARG;
    c->prof = on != 0;
    return HQ_OK;
}

int hq_profile_reset(hq_ctx* c) {
    if (!c) return HQ_ERR_ARG;
    c->prof_assign = c->prof_cost = c->prof_grid = c->prof_finalize = c->prof_sa = c->prof_comm = c->prof_centroid =
        c->prof_lloyd = c->prof_hist = c->prof_errsum = c->prof_reseed = c->prof_dither = ProfSlot{};
    return HQ_OK;
}

int hq_profile_get(hq_ctx* c, const char* kernel, double* total_ms, int64_t* launches) {
    if (!c || !kernel) return HQ_ERR_ARG;
    const ProfSlot* s = nullptr;
    if (!std::strcmp(kernel, "assign")) s = &c->prof_assign;
    else if (!std::strcmp(kernel, "cost")) s = &c->prof_cost;
    else if (!std::strcmp(kernel, "grid")) s = &c->prof_grid;
    else if (!std::strcmp(kernel, "finalize")) s = &c->prof_finalize;
    else if (!std::strcmp(kernel, "sa_step")) s = &c->prof_sa;
    else if (!std::strcmp(kernel, "comm")) s = &c->prof_comm;
    else if (!std::strcmp(kernel, "centroid")) s = &c->prof_centroid;
    else if (!std::strcmp(kernel, "lloyd")) s = &c->prof_lloyd;
    else if (!std::strcmp(kernel, "hist")) s = &c->prof_hist;
    else if (!std::strcmp(kernel, "errsum")) s = &c->prof_errsum;
    else if (!std::strcmp(kernel, "reseed")) s = &c->prof_reseed;
    else if (!std::strcmp(kernel, "dither")) s = &c->prof_dither;
    else return fail(c, HQ_ERR_ARG, "unknown kernel '%s'", kernel);
    if (total_ms) *total_ms = s->ms;
    if (launches) *launches = s->launches;
    return HQ_OK;
}

int hq_set_option(hq_ctx* c, const char* name, int value) {
    if (!c || !name) return HQ_ERR_ARG;
    if (!std::strcmp(name, "grid")) {
        if (value != 0 && value != 16 && value != 32 && value != 64)
            return fail(c, HQ_ERR_ARG, "grid must be 0, 16, 32 or 64");
        c->G2 = value;
    } else if (!std::strcmp(name, "cost_variant")) {
        if (value < 0 || value > 2) return fail(c, HQ_ERR_ARG, "cost_variant must be 0, 1 or 2");
        c->cost_variant = value;
    } else if (!std::strcmp(name, "trim")) {
        c->trim = value != 0;
    } else if (!std::strcmp(name, "cost_rows")) {
        if (value != 8 && value != 16) return fail(c, HQ_ERR_ARG, "cost_rows must be 8 or 16");
        c->cost_rows = value;
    } else if (!std::strcmp(name, "sa_graph")) {
        c->sa_graph = value != 0;
    } else if (!std::strcmp(name, "gen_hrow_outputs")) {
        if (value != 4 && value != 8) return fail(c, HQ_ERR_ARG, "gen_hrow_outputs must be 4 or 8");
        c->gen_hrow_no = value;
    } else if (!std::strcmp(name, "gen_vmfma")) {
        c->gen_vmfma = value != 0;
    } else if (!std::strcmp(name, "gen_hmfma")) {
        c->gen_hmfma = value != 0;
    } else if (!std::strcmp(name, "gen_tile_shape")) {
        if (value < 0 || value > 2) return fail(c, HQ_ERR_ARG, "gen_tile_shape: 0, 1 or 2");
        c->gen_shape = (int)value;
    } else if (!std::strcmp(name, "gen_vtile2")) {
        c->gen_vtile2 = value != 0;
    } else if (!std::strcmp(name, "gen_hrow4")) {
        c->gen_hrow4 = value != 0;
    } else if (!std::strcmp(name, "cost_tw")) {
        if (value != 128 && value != 256) return fail(c, HQ_ERR_ARG, "cost_tw must be 128 or 256");
        c->cost_tw = value;

    } else if (!std::strcmp(name, "sa_device")) {
        c->sa_device = value != 0;
    } else if (!std::strcmp(name, "shard_solo")) {
        c->shard_solo = value != 0;
    } else if (!std::strcmp(name, "palette_split")) {
        c->psplit = value != 0;
    } else if (!std::strcmp(name, "slice_ranks")) {
        if (value < 1) return fail(c, HQ_ERR_ARG, "slice_ranks must be >= 1");
        c->slice_ranks = value;
    } else if (!std::strcmp(name, "slice_rank")) {
        // (checked against slice_ranks again at each evaluation: the options may come in either order)
        if (value < 0) return fail(c, HQ_ERR_ARG, "slice_rank must be >= 0");
        c->slice_rank = value;
    } else if (!std::strcmp(name, "fold_blocks")) {
        if (value < 1 || value > 64) return fail(c, HQ_ERR_ARG, "fold_blocks in [1, 64]");
        c->fold_blocks = value;
        c->fold_block = 0;
    } else if (!std::strcmp(name, "fold_block")) {
        if (value < 0 || value >= c->fold_blocks) return fail(c, HQ_ERR_ARG, "fold_block in [0, fold_blocks)");
        c->fold_block = value;
    } else if (!std::strcmp(name, "lists16")) {
        if (value < 0 || value > 2) return fail(c, HQ_ERR_ARG, "lists16: 0, 1 or 2");
        c->lists16 = (int)value;
        if (!value) {  // (the lists' 10 MiB per palette are re-allocated when turned on again)
            c->d_l1n.release();
            c->d_l2n.release();
        }
    } else if (!std::strcmp(name, "chunked")) {
        c->chunked = value != 0;
    } else if (!std::strcmp(name, "pixel_err")) {
        c->pixel_err = value != 0;
    } else if (!std::strcmp(name, "dither_rows")) {
        if (value < 64 || value > 1024 || value % 64)
            return fail(c, HQ_ERR_ARG, "dither_rows must be a multiple of 64 in 64 .. 1024");
        c->dither_rows = value;
    } else if (!std::strcmp(name, "img_u8")) {
        c->img_u8_path = value != 0;
    } else if (!std::strcmp(name, "assign_blocks_per_cu")) {
        if (value < 0 || value > 64) return fail(c, HQ_ERR_ARG, "assign_blocks_per_cu in [0,64] (0 = auto)");
        c->assign_blocks_per_cu = value;
    } else {
        return fail(c, HQ_ERR_ARG, "unknown option '%s'", name);
    }
    return HQ_OK;
}

}  // extern "C"
