// hq_runtime.h -- what the host runtime's translation units share: the context and
// the search (the opaque types of include/hq.h), the owners of their device memory,
// pinned memory and events, the pass value, the profiling tables and the checks
// written once.  hq_runtime.hip: context, filters, image, options, profiling and
// the stand-alone utilities; hq_eval.hip: population buffers and evaluation;
// hq_search_run.hip: the device-resident search and hq_search_*.  Not part of the
// public ABI.
//
// Ownership: a DevBuf, PinBuf or EventSet frees what it holds when it goes out of
// scope or its owner is deleted; nothing in the runtime frees one by hand except
// to give memory back early (option lists16 = 0).
#pragma once

#include <rccl/rccl.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <variant>
#include <vector>

#include "hq_dot.h"
#include "hq_launch.h"
#include "hq_mask.h"
#include "hq_swasa.h"

#ifndef HQ_COST_TW
#define HQ_COST_TW 128
#endif
#ifndef HQ_SA_GRAPH
#define HQ_SA_GRAPH 0  // (measured slower: C3 0.528 -> 0.540 ms, shard-of-8 0.1035 -> 0.110 ms per step)
#endif

namespace hq {

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    hipError_t ensure(size_t n) {
        if (n <= bytes) return hipSuccess;
        release();
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

// Pinned host memory, grown like a DevBuf.
struct PinBuf {
    void* p = nullptr;
    size_t bytes = 0;
    PinBuf() = default;
    PinBuf(const PinBuf&) = delete;
    PinBuf& operator=(const PinBuf&) = delete;
    ~PinBuf() { if (p) (void)hipHostFree(p); }
    hipError_t ensure(size_t n) {
        if (n <= bytes) return hipSuccess;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        bytes = 0;
        hipError_t e = hipHostMalloc(&p, n, hipHostMallocDefault);
        if (e == hipSuccess) bytes = n;
        return e;
    }
    template <typename T>
    T* as() const { return static_cast<T*>(p); }
};

// Profiling events.  A slot whose event could not be created stays null: a launch
// under a null event is an untimed launch.
struct EventSet {
    std::vector<hipEvent_t> ev;
    EventSet() = default;
    EventSet(const EventSet&) = delete;
    EventSet& operator=(const EventSet&) = delete;
    ~EventSet() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    hipError_t ensure(size_t n) {
        if (n > ev.size()) ev.resize(n, nullptr);
        for (hipEvent_t& e : ev)
            if (!e) {
                const hipError_t r = hipEventCreate(&e);
                if (r != hipSuccess) {
                    e = nullptr;
                    return r;
                }
            }
        return hipSuccess;
    }
};

// ---- profiling: stages (hq_profile_get's names) and event pairs ----------------
struct ProfSlot {
    double ms = 0.0;
    int64_t launches = 0;
};

enum Stage {
    kStGrid, kStAssign, kStCost, kStFinalize, kStSaStep, kStComm, kStCentroid, kStLloyd, kStHist, kStErrsum,
    kStReseed, kStDither, kStReduce, kStDot, kStCoords, kStages
};
inline constexpr const char* kStageNames[kStages] = {"grid", "assign", "cost", "finalize", "sa_step", "comm",
                                                     "centroid", "lloyd", "hist", "errsum", "reseed", "dither",
                                                     "reduce", "dot", "coords"};

// The start/stop event pairs of one evaluation (the context's EventSet) or of one
// search iteration (kPairs pairs per iteration of a run in hq_search::pev).  A pass
// takes four consecutive pairs -- grid, assign, cost, finalize -- from its first
// (pass_pairs): the main evaluation's, a hybrid iteration's assign-only pass's or
// a repair iteration's cost pass's.
enum Pair {
    kPGrid, kPAssign, kPCost, kPFinalize,  // the evaluation
    kPSaStep,                              // the SA step that generated its population
    kPComm,                                // its collective
    kPDither,                              // diffuse_kernel in the place of grid + assign
    kPLloydGrid, kPLloydAssign,            // hybrid iteration: the assign-only pass,
    kPSums, kPLloydUpdate,                 // the sums kernel (also hq_cluster_sums'), the update kernel
    kPRepGrid, kPRepAssign, kPRepCost,     // repair iteration: the cost pass,
    kPErrsum, kPReseed,                    // the error kernels (also hq_cluster_errors'), the reseed kernel
    kPHist,                                // hq_color_histogram's kernel
    kPReduce,                              // hq_set_image_reduced's kernel
    kPDot,                                 // dot_kernel's launches (one per class), or dot_tile_kernel's one, in the place of grid + assign
    kPCoords,                              // coords_kernel (option "assign_space" 1), in front of a pass: ensure_assign_coords
    kPairs
};
// The stage each pair's time and launch count go to.
inline constexpr Stage kPairStage[kPairs] = {kStGrid, kStAssign, kStCost, kStFinalize, kStSaStep, kStComm,
                                             kStDither, kStGrid, kStAssign, kStCentroid, kStLloyd, kStGrid,
                                             kStAssign, kStCost, kStErrsum, kStReseed, kStHist, kStReduce,
                                             kStDot, kStCoords};

// One evaluation's or iteration's events and which pairs it recorded (events of an
// earlier call may sit in the other slots, so only recorded pairs are accumulated).
struct ProfRec {
    const hipEvent_t* ev = nullptr;  // 2 kPairs events; null: not profiling
    uint32_t recorded = 0;           // bit p: pair p
};

// `launch()` with pair p's events riding on it (start / stop: which of the two; a
// launch loop times its first and last).  The pending events are cleared on every
// way out, so the caller may return on the error at once.
template <typename F>
inline hipError_t timed_launch(ProfRec& pr, Pair p, F&& launch, bool start = true, bool stop = true) {
    if (pr.ev) {
        set_launch_events(start ? pr.ev[2 * p] : nullptr, stop ? pr.ev[2 * p + 1] : nullptr);
        pr.recorded |= 1u << p;
    }
    const hipError_t e = launch();
    set_launch_events(nullptr, nullptr);
    return e;
}

// ---- a pass: how far an evaluation goes and how its index images are made -------
// The rendering, how the argmin stage makes the index images: one alternative, with its own
// parameters and nobody else's (hq.h says what each computes).
//   Plain: grid, then assign.
//   Ordered: the same grid, then assign's ordered-dithering instances with the context's
//     threshold map at `amp` per channel.  K <= 256.
//   Diffused: the counter set and the used bits zeroed as without a grid, then diffuse_kernel's
//     instance <rows, slope> (hq_diffusion_classify) of `taps` in the place of grid + assign.
//     floyd_steinberg: that preset's taps, whoever gave them: the kernel's own formula, no instance.
//   Dot: zeroed the same way, then dot_kernel's launches under the context's class matrix (c->dot_cls,
//     its tables on the device: ensure_dot_tables); on a row-block shard its windowed instance over rows
//     [a0, a1), the extended rows and what of the apron the matrix's reach needs (dot_window).  On a whole
//     image dot_tile_kernel's one launch in their place where dot_tiled (hq_eval.hip) says so (option "dot_tile").
struct Plain {};
struct Ordered { float amp[3]; };
struct Diffused { float strength; hq_diffusion_taps taps; int rows, slope; bool floyd_steinberg; };
struct Dot { float strength; int a0, a1; };
using Rendering = std::variant<Plain, Ordered, Diffused, Dot>;

// The kind, how far the pass goes.  Full: grid, assign, cost, finalize into d_out, the collective on d_out.
// Fold: a folding search's evaluation -- no finalize (the accept step reads the
//   fixed-point sums itself); the collective gathers the ranks' counter blocks.
// AssignOnly (a hybrid iteration's first pass): the argmin alone -- grid build or
//   zeroing, then assign -- for the index images the sums kernel reads.
// CostOnly (a repair iteration's first pass): grid, assign and cost -- the index
//   images and, with option "pixel_err" in force, the error image the error kernel
//   reads.
// Any kind may be plain or ordered.  A diffused rendering exists on a full pass only: its
// constructor takes no kind, and the members are const.  A dot rendering may also be a folding
// search's evaluation (hq_search_set_dot): Full or Fold, nothing else.
// Counter-set parity: each pass takes the other counter set than the last one
// (build_grid zeroes it), so an accept step can read the last set while the next
// is filled.  A side pass (AssignOnly, CostOnly: nothing reads its sums, so no
// finalize and no collective) fills the other set without making it the current
// one: c->acc_par stays the set of the last full pass (what sa_args, the fold and
// the finalize read), and the full pass that follows takes, and zeroes, the same
// set again.
struct Pass {
    enum Kind { Full, Fold, AssignOnly, CostOnly };
    const Kind kind;
    const Rendering rendering;
    Pass(Kind k = Full) : kind(k) {}
    Pass(Kind k, const Ordered& o) : kind(k), rendering(o) {}
    Pass(const Diffused& d) : kind(Full), rendering(d) {}
    Pass(const Dot& d) : kind(Full), rendering(d) {}
    Pass(bool fold, const Dot& d) : kind(fold ? Fold : Full), rendering(d) {}
    template <typename R>
    const R* as() const { return std::get_if<R>(&rendering); }     // the alternative's parameters, or null
    bool rendered() const { return !as<Plain>(); }                 // the getters answer for a rendering
    bool gridless() const { return as<Diffused>() || as<Dot>(); }  // no grid is built: HQ_PASS_DITHER
    bool side() const { return kind == AssignOnly || kind == CostOnly; }
    Pair pairs() const { return kind == AssignOnly ? kPLloydGrid : kind == CostOnly ? kPRepGrid : kPGrid; }
};

// ---- what the last pass left on the device ---------------------------------------
// Whose index images the device holds -- an evaluation's (hq_eval_population[_partial]), a
// rendering's (dithered or ordered) or a search's last candidates' -- of P palettes of K colours
// in nch chunks, [lo, lo + n) of them here; whether that pass stored its error image ("pixel_err");
// the tiles per palette its fast cost launch ran and has in all (hq_mask_info; 0: the generic cost).
// It vouches for the index images, d_pixerr, the prepared palettes and the counter and used-bit
// sets, and changes in drop() and commit() alone.
struct Resident {
    enum Owner { None, Eval, Render, Search } owner = None;
    int P = 0, K = 0, nch = 1, lo = 0, n = 0;
    bool err_image = false;  // (never a search's: its side passes store candidates' it then moves)
    int64_t tiles_run = 0, tiles_all = 0;
    // What may be read; by construction err_ok => sums_ok => idx_ok and pixerr_ok => idx_ok.
    bool idx_ok() const { return owner != None; }              // hq_get_indices[32]
    bool sums_ok() const { return owner == Eval; }             // hq_cluster_sums: no rendering's, no search's
    bool err_ok() const { return sums_ok() && err_image; }     // hq_cluster_errors
    bool pixerr_ok() const { return idx_ok() && err_image; }   // hq_get_pixel_errors
    // The same images once a search has evaluated through hq_*_population: the indices alone.
    Resident of_search() const {
        return Resident{owner == None ? None : Search, P, K, nch, lo, n, false, tiles_run, tiles_all};
    }
};

}  // namespace hq

struct hq_ctx {
    int device = 0;
    int de_type = HQ_DE_CIE76;
    hipStream_t stream = nullptr;
    std::string err;

    // filters (IM:800-841)
    int taps = 0, half = 0;
    std::vector<float> k1, k2, k3, absk3;
    hq::DevBuf d_k1, d_k2, d_k3, d_absk3;
    hq::DevBuf d_vtaps;    // tiled generic path: [7][vtap_pitch] vertical taps per plane, zero-padded
    int vtap_pitch = 0;
    int fast_hb = 0;   // fast path tap bucket (fast_bucket(half)); 0 = generic path only
    hq::DevBuf d_taps;     // fast path taps, build_fast_taps (the filters centred in the bucket)
    hq::DevBuf d_vfrag16;  // split-f16 MFMA A fragments of the stacked vertical taps
    hq::DevBuf d_vfrag16p; // the same in cost16w's (hi, lo) pair layout
    hq::DevBuf d_vfragm;   // the tiled generic path's matrix-core vertical taps (build_vtile_dup_taps)
    hq::DevBuf d_htaps;    // gen_hrow4's packed horizontal taps [T][2] float4

    // image
    bool have_image = false;
    hq::Geom g{};
    float illum[3] = {0.95047f, 1.0f, 1.0883f};
    hq::DevBuf d_R, d_G, d_B;          // planar, extended rows (n_ext, padded to 4)
    hq::DevBuf d_rgbx;                 // packed 8-bit copy of R,G,B when every channel is k/255
    bool img_u8 = false;
    hq::DevBuf d_labL, d_labA, d_labB;  // planar LabRef, owned rows, lab_pitch
    // option "assign_space" (0 sRGB, 1 CIELAB): the pixels' argmin coordinates, three planes of
    // d_R's length and padding, made on the device from the image the context holds by the
    // first evaluation that needs them (ensure_assign_coords) and the image's and the
    // illuminant's: begin_image says they are stale.  d_arg: the palettes' coordinates
    // ([P][256], PaletteArgs::arg).  With space 0 none of the four is allocated or read.
    int assign_space = 0;
    hq::DevBuf d_cR, d_cG, d_cB, d_arg;
    bool coords_ok = false;

    // population work buffers
    hq::Resident res;  // what the last pass left in them (drop, commit)
    // hq_last_path: the kernels the last enqueued pass took, written by enqueue_core and
    // enqueue_wide where each launch is chosen (record_path); path.sequence counts the passes
    hq_path_info path{};
    hq::DevBuf d_pal_in, d_pal, d_opp, d_opp16, d_dup, d_pflags, d_lvl1, d_lvl2, d_idx, d_used_mask,
        d_acc, d_out, d_gen_t;
    // d_acc: two sets of fixed-point dE sums [kAccSlots][P][4] u64 (acc_add), d_used_mask two
    // sets of used bits [kUsedSlots][used_stride]; evaluation n fills set acc_par = n & 1
    int acc_par = 0;
    hq::DevBuf d_pixerr;           // option "pixel_err": [P][n_own] per-pixel dE of the last evaluation
    hq::DevBuf d_idx32, d_used32;  // K > 16384 (hq_wide.hip): 32-bit index images, per-colour used flags
    hq::DevBuf d_idx16, d_dist;    // 256 < K <= 16384 (chunked): 16-bit index images, pass distances
    hq::DevBuf d_l1n, d_l2n;       // the native 16-bit candidate lists (hq_lists16.hip)
    int nch_cur = 1;           // chunks per palette of the population being enqueued (1: K <= 256)
    hq::PinBuf h_pal;          // pinned [P][K][4] float
    hq::PinBuf h_out;          // pinned [P][1+K] double
    hq::DevBuf d_sums;             // [P][K][4] int64 sums, then the planar form's range flag
    // hybrid iterations: every owned pixel of the planar image is finite and in [0, 1], the
    // condition of the planar form's sums (-1: not established yet for this image)
    int planar_ok = -1;
    hq::DevBuf d_hist;             // hq_color_histogram: [2^(3 bits)][4] int64 cells, then the range flag
    hq::DevBuf d_errstat, d_worst; // [P][K][4] u64 statistics, then the flag; [P][K] float4 worst pixels
    hq::DevBuf d_dcarry;           // a Diffused pass: [P][R][3][W] errors of a strip's last R rows (DiffuseArgs::carry)
    // dot diffusion: the class matrix of the last hq_dot_population (n = 0: none yet), its two
    // per-cell tables on the device ([2][kDotCells] words, uploaded when the matrix changes:
    // ensure_dot_tables) and the errors e of a Dot pass ([P][3][H][W] floats, never zeroed)
    hq_dot_classes dot_cls{};
    hq::DevBuf d_dottab, d_doterr;
    // the tiled form (hq_dot_tile.hip): the schedule of the same matrix on the device
    // ([kDotSchedWords] words, uploaded with the tables); options "dot_tile" (-1 auto, 0 the
    // chain, 1 tiled wherever eligible) and "dot_tile_shape" (0: the largest shape whose window
    // fits, else 1 .. kDotTileShapes); what hq_dot_form reports: the form of the last dot pass
    // enqueued (0 none yet, 1 chain, 2 tiled), its tile and the matrix's levels
    hq::DevBuf d_dotsched;
    hq::DotMatrixInfo dot_info{};  // dot_cls' reach and levels, made where its tables are (ensure_dot_tables)
    int dot_tile = -1, dot_tile_shape = 0;
    int dot_form = 0, dot_form_tw = 0, dot_form_th = 0, dot_form_levels = 0;
    // dot diffusion on a row-block shard (hq_dot_population_partial): the apron, the image rows
    // [e0 - apron_above, e0) and [e1, e1 + apron_below) kept beyond the extended rows by
    // hq_set_image[_planar]_shard under option "dot_apron" -- [3][apron_above + apron_below][W]
    // planar floats, the rows above first.  The image's: begin_image drops it.  apron_ok: every
    // float of it, and of the extended rows outside the owned ones, is finite and in [0, 1]
    // (found on the host when it is gathered: the rows the device's range flag does not look at)
    int dot_apron = 0;             // the option: rows asked for by the next shard
    int apron_above = 0, apron_below = 0;
    bool apron_ok = true;
    hq::DevBuf d_apron;
    // ordered dithering: the threshold map (hq_set_dither_map; empty: the default, Bayer 16 x 16)
    // and its device copy, kMaxMapSide^2 floats made once by ensure_dither_map (its address is
    // in captured launches) and written by it whenever the host map has changed
    std::vector<float> dmap;
    int dmap_w = 0, dmap_h = 0;
    hq::DevBuf d_dmap;
    bool dmap_dirty = true;
    // fixed palette colours (hq_set_fixed_colors; a property of the context like the map, kept by
    // hq_set_image*): [fixed_n][4], .w = 0.  A search latches them at creation; the polishes read
    // fixed_n when called
    std::vector<float> fixed;
    int fixed_n = 0;
    // pixel mask (hq_set_mask; a property of the context like the map, dropped by hq_set_image*):
    // the owned rows on the host (0 / 1, W bytes per row: what the live-tile list is built from),
    // on the device at the LabRef planes' pitch (the cost kernels) and over the extended rows'
    // positions (the sums and histogram kernels), and the counts hq_mask_info reports
    bool mask_on = false;
    std::vector<uint8_t> mask_own;
    hq::DevBuf d_mask, d_maskq;
    int64_t mask_n_full = 0, mask_n_own = 0;
    // pixel weights (hq_set_weights) are the same piece of state: mask_on and weights_on, the
    // three copies hold the raw bytes (non-zero = the pixel counts, by its byte), mask_n_* count
    // the non-zero ones and mask_w_* are the weight sums (of a mask: mask_n_*)
    bool weights_on = false;
    int64_t mask_w_full = 0, mask_w_own = 0;
    // the live-tile list of the fast cost launch (ensure_live_tiles): rebuilt when the mask or
    // the launch's tile grid or whether it skips has changed, never inside a capture
    hq::DevBuf d_live;
    int n_live = 0;
    bool live_dirty = true;
    int live_rows = 0, live_tw = 0, live_skip = -1;
    int mask_skip = 1;     // option "mask_skip": the fast cost pass launches live tiles only

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
    int assign_res_ord[5] = {};  // [NG]: the ordered-dithering forms
    int psplit = 0;        // with a communicator of N ranks and the whole image on every rank: rank r
                           // evaluates palettes [r P/N, (r+1) P/N), then one all-gather (option
                           // "palette_split"; SURVEY 8e's split of large populations)
    int slice_ranks = 1, slice_rank = 0;  // test only: the same slice without a communicator
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
    int cent_span = 0;       // test option "cent_span": the sums kernel's pixels per workgroup (0: by the grid)
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
    hq::ProfSlot prof_stage[hq::kStages];
    hq::EventSet ev;  // 2 kPairs events, made by hq_create
    int num_cu = 256;
    size_t lds_optin = 160 * 1024;  // per-workgroup LDS a kernel may opt into (hq_create's query)
};

struct hq_search {
    hq_ctx* ctx;
    hq::SearchDriver* driver;  // host-driven search (sa_device = 0), else null
    int K;
    // device-resident search: the SWASA state lives on the device, ping-ponged
    // between [0] and [1] by sa_step_kernel; the host keeps the iteration-only
    // quantities (temperature, step width, convergence threshold) in `pol`,
    // whose RNG is unused.
    hq::Swasa* pol = nullptr;
    hq_swasa_params prm{};
    int P = 0, ite = 0, st = 0, cd = 0;  // state and candidate buffer parities
    int every = 0;                       // hq_search_set_lloyd: iteration ite % every == 0 is hybrid (0: none)
    int repair_every = 0;                // hq_search_set_repair: iteration ite % repair_every == 0 repairs (0: none)
    int repair_moves = -1;               // ... at most so many colours per palette (< 0: no limit)
    int nch = 1;                         // chunked palettes (256 < K <= 16384): chunks per palette
    bool ordered = false;                // hq_search_set_ordered: every evaluation is the ordered one
    hq::Ordered ord{};                   // ... at this amplitude per channel
    bool dot = false;                    // hq_search_set_dot: every evaluation is the dot-diffused one
    float dot_strength = 0.f;            // ... at this strength
    hq_dot_classes dot_cls{};            // ... under this matrix, the search's own (latched at the call)
    int nfixed = 0;                      // the context's fixed colours at hq_search_create: colours
    std::vector<float> fixed;            // 0 .. nfixed-1 of every member, [nfixed][4], for the search's life
    bool fold = false;                   // accept steps reduce the partials (no finalize launch)
    ncclComm_t comm = nullptr;           // the context's communicator at hq_search_create
    int assign_space = 0;                // ... and its option "assign_space": a run under another value is refused
    float t_acc = 0.f;                  // temperature / threshold of the iteration
    double keep_acc = 0.0;               // whose population awaits acceptance
    hq::DevBuf colors[2], cand[2], err[2], seed[2], best_err[2], best_colors, jA, jC;
    hq::EventSet pev;                    // profiling: 2 kPairs events per iteration of a run
    hipGraphExec_t gexec = nullptr;      // option sa_graph: the last run's iteration chain
    int gexec_iters = 0;                 // (its iteration count: the topology an update must match)
    bool graphed = false;                // hq_search_info: the last run was captured and replayed
};

namespace hq {

int fail(hq_ctx* c, int code, const char* fmt, ...);

#define HIP_TRY(ctx, expr)                                                                      \
    do {                                                                                        \
        hipError_t _e = (expr);                                                                 \
        if (_e != hipSuccess)                                                                   \
            return fail((ctx), _e == hipErrorOutOfMemory ? HQ_ERR_NOMEM : HQ_ERR_DEVICE,        \
                        "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

#define NCCL_TRY(ctx, expr)                                                                     \
    do {                                                                                        \
        ncclResult_t _r = (expr);                                                               \
        if (_r != ncclSuccess)                                                                  \
            return fail((ctx), HQ_ERR_COMM, "%s failed: %s", #expr, ncclGetErrorString(_r));    \
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

// The chunk count of the population being enqueued, for one search call.
struct NchScope {
    hq_ctx* c;
    NchScope(hq_ctx* cc, int nch) : c(cc) { c->nch_cur = nch; }
    ~NchScope() { c->nch_cur = 1; }
};

inline int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }
inline bool whole_image(const hq_ctx* c) { return c->g.r0 == 0 && c->g.r1 == c->g.H; }

// A row-block split (a communicator, no palette split) keeps one block of
// counters and used bits per rank in each set, [ranks][...]: every rank fills
// its own block, and a device-resident search's one all-gather per iteration
// hands every rank all the blocks, which its accept step folds (no finalize).
// (test options fold_blocks / fold_block: the same layout without a communicator,
// this context filling block fold_block and the others staying zero)
inline int rank_blocks(const hq_ctx* c) { return c->comm ? (c->psplit ? 1 : c->nranks) : c->fold_blocks; }
inline int own_block(const hq_ctx* c) { return c->comm ? (rank_blocks(c) > 1 ? c->rank : 0) : c->fold_block; }
// A device-resident search folds the partials in its accept step unless the
// palette split all-gathers finalized rows.
inline bool search_folds(const hq_ctx* c) { return !(c->comm && c->psplit); }
// The sums form assign's own condition picks: the packed bytes (den 255), else
// the planar floats (den 2^32).
inline bool sums_u8(const hq_ctx* c) { return c->img_u8 && c->img_u8_path; }
// The owned rows: their pixels, the first one's position among the extended rows' (the index
// images' and planes' origin), and both ends as the 32-bit positions the table kernels take.
inline int64_t n_own(const Geom& g) { return (int64_t)g.W * (g.r1 - g.r0); }
inline int64_t own_first(const Geom& g) { return (int64_t)(g.r0 - g.e0) * g.W; }
inline void owned_range(const Geom& g, uint32_t* q0, uint32_t* q1) {
    *q0 = (uint32_t)own_first(g);
    *q1 = *q0 + (uint32_t)n_own(g);
}

// hq_runtime.hip
int bind(hq_ctx* c);
// `what` (a call's or a move's name) works on the whole image, with every palette's index image on
// this context: refused on a row-block shard (HQ_ERR_STATE), with a communicator of more than one
// rank (HQ_ERR_UNSUPPORTED; comm_hint: what to do instead) and on a palette slice
// (HQ_ERR_UNSUPPORTED; psplit_alone: also under option "palette_split" without a communicator,
// where it slices nothing).
int whole_image_only(hq_ctx* c, const char* what, const char* comm_hint = "", bool psplit_alone = true);
ProfRec prof_begin(hq_ctx* c);  // the context's events (profiling on) or none
// Add the recorded pairs' kernel times to their stages (the events have completed).
void prof_accumulate(hq_ctx* c, const ProfRec& pr);

// hq_eval.hip
// The record's two transitions: nothing is vouched for; the pass that has come back left `r`.
// resident_of: what a pass of P x K leaves, from the state it was enqueued in (nch_cur,
// pal_generic, options, mask): called before that state is reset.
void drop(hq_ctx* c);
void commit(hq_ctx* c, const Resident& r);
Resident resident_of(hq_ctx* c, Resident::Owner owner, int P, int K);
// (drops the record when, and only when, it reallocates a buffer the record vouches for)
int ensure_population(hq_ctx* c, int P, int K);
// option "assign_space" 1: the pixels' coordinate planes in place and current (one launch of
// coords_kernel when they are stale; ensure_population calls it, so never inside a capture).
// assign_space_excludes: HQ_ERR_UNSUPPORTED "<what> under option assign_space 1 ..." when the
// option is on, for the calls that keep the sRGB rule.  inv_illuminant: 1 / the illuminant.
int ensure_assign_coords(hq_ctx* c);
int assign_space_excludes(hq_ctx* c, const char* what);
inline void inv_illuminant(const hq_ctx* c, float inv[3]) {
    for (int i = 0; i < 3; ++i) inv[i] = 1.0f / c->illum[i];
}
// P palettes of K colours ([P][4K]) into d_pal_in -- from the host (through h_pal; chunked:
// pack_chunks' sub-palettes) or, host null, from the device -- and the palette prep (K > 256
// unchunked: the upload alone, enqueue_wide preps).
int upload_and_prep(hq_ctx* c, const float* host, const void* dev, int P, int K);
PaletteArgs prep_args(hq_ctx* c, int K);
uint64_t* acc_base(hq_ctx* c, int par, int P);
uint32_t* used_base(hq_ctx* c, int par, int Ps);
int enqueue_core(hq_ctx* c, int P, int K, ProfRec& pr, const Pass& pass = {});
void pack_chunks(const float* pal, int P, int K, int nch, float* out);
ClusterArgs cluster_args(hq_ctx* c, int P, int K, int nch, int* idx_bytes);
ClusterErrArgs cluster_err_args(hq_ctx* c, int P, int K, int nch, int* idx_bytes);
// the last evaluation's sums -> centroids, in place; the first nfixed colours of every palette keep their bits
int kmeans_move(hq_ctx* c, int P, int K, int nfixed, float* pal);
// (the rule: hq_reseed_unused_fixed)
int repair_move(hq_ctx* c, int P, int K, int max_moves, int nfixed, bool ignore_bad, float* pal, int* moved);
// planar_ok established (once per image), else HQ_ERR_UNSUPPORTED "<subject> with a pixel outside
// [0, 1] or not finite: <what>"
int require_unit_range_image(hq_ctx* c, const char* subject, const char* what);
// ordered dithering: amp (may be null: HQ_ERR_ARG) finite and in [0, 1]; what a context must be
// for it (K <= 256, no palette slice, the image in [0, 1]); the map on the device
int check_ordered_amp(hq_ctx* c, const float* amp);
int ordered_scope(hq_ctx* c, int K);
int ensure_dither_map(hq_ctx* c);
// A search under the dot-diffused cost (hq_search_set_dot): where it may run -- hq_dot_population's
// scope, K and image range, in that order -- and, before anything is enqueued or captured, matrix m's
// tables on the device and the scratch the form that will run needs for P palettes of K colours.
int dot_search_scope(hq_ctx* c, int K);
int ensure_dot_pass(hq_ctx* c, const hq_dot_classes& m, int P, int K);
// pixel mask: the divisor that finishes a cost (the in-mask pixels of the full image; without a
// mask W H, the expression it always was); the refusal of a palette slice under a mask; the
// live-tile list on the device for the launch the options in force select (ensure_population
// calls it: before anything is enqueued or captured)
// (pixel weights: their sum over the full image, below 2^53 and so exact)
inline double cost_divisor(const hq_ctx* c) {
    return c->mask_on ? (double)c->mask_w_full : (double)c->g.W * (double)c->g.H;
}
int mask_scope(hq_ctx* c);
// "a pixel mask" / "(hq_set_mask)" or "pixel weights" / "(hq_set_weights)": the refusals' wording
inline const char* mask_noun(const hq_ctx* c) { return c->weights_on ? "pixel weights" : "a pixel mask"; }
inline const char* mask_call(const hq_ctx* c) { return c->weights_on ? "hq_set_weights" : "hq_set_mask"; }
// pixel weights on the planar form (sums in units of 2^-32): HQ_ERR_UNSUPPORTED when the owned
// rows' weights sum to 2^31 or more (a total could pass 2^63); made on the host, before `what`
// enqueues anything
int weighted_sums_scope(hq_ctx* c, const char* what);
int ensure_live_tiles(hq_ctx* c);

}  // namespace hq
