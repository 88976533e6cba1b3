// hq_eval.hip -- libhq host runtime, evaluation: the population buffers, the pass
// over a prepared population (enqueue_core, enqueue_wide, the generic cost), the
// evaluation, dither, dot-diffusion, ordered-dither, index, sums, error and histogram entry
// points, and the two improvement loops built on them (refine, repair).  Shared declarations:
// hq_runtime.h.
#include <cmath>

#include "hq_diffuse.h"
#include "hq_dot.h"
#include "hq_runtime.h"

using namespace hq;

namespace {

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
int assign_blocks(const hq_ctx* c, int P, bool ordered = false) {
    // at least HQ_ASSIGN_MINPX pixels per thread: a launch's fixed part (table
    // fill, pipeline start, the used-bit flush) is paid per workgroup (C2,
    // 1024^2 P = 1: 2048 workgroups of 2 pixels per thread took 14 us, 1045 of 4
    // took 12.3, 523 of 8 took 8.5; the 512-row shard, 5.5 per thread at 1536
    // workgroups, slowed from 43 to 46 us at 8)
    const int64_t chunk = 256 * HQ_ASSIGN_MINPX;
    const int ng = std::min(P, 4);
    const int res = ordered ? c->assign_res_ord[ng] : c->nch_cur > 1 ? c->assign_res_chunked : c->assign_res[ng];
    const int per_cu = c->assign_blocks_per_cu > 0 ? c->assign_blocks_per_cu : res > 0 ? res : 4;
    const int64_t nblocks = (int64_t)c->num_cu * per_cu;
    return (int)std::max<int64_t>(1, std::min<int64_t>(nblocks, (c->g.n_ext + chunk - 1) / chunk));
}

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
// (as the reasons why not, hq_path_why's bits: enqueue_core records the value it dispatches on)
uint32_t cost_slow_why(const hq_ctx* c) {
    uint32_t why = 0;
    if (c->fast_hb <= 0) why |= HQ_WHY_HALF;
    if (c->cost_variant != 0) why |= HQ_WHY_VARIANT;
    if (c->pal_generic) why |= HQ_WHY_PALETTE;
    if (c->taps_generic) why |= HQ_WHY_TAPS;
    if (c->nch_cur > kMaxNchFast) why |= HQ_WHY_NCH;
    else if (c->nch_cur > 1 && c->fast_hb > 0 && !(c->fast_hb == 10 && c->cost_rows == 16 && c->cost_tw == 128))
        why |= HQ_WHY_CHUNK_FORM;
    return why;
}
bool cost_fast(const hq_ctx* c) { return cost_slow_why(c) == 0; }

// hq_last_path: the pass that has been enqueued becomes the context's record.
void record_path(hq_ctx* c, hq_path_info pi) {
    pi.sequence = c->path.sequence + 1;
    pi.previous_pass = c->path.pass, pi.previous_cost = c->path.cost;
    c->path = pi;
}
void record_argmin(hq_path_info& pi, const AssignTag& at) {
    pi.argmin = at.kernel;
    pi.argmin_cmb = at.cmb;
    pi.argmin_passes = at.passes;
    pi.pixels = at.kernel == HQ_ARGMIN_NONE ? HQ_PIXELS_NONE : at.u8 ? HQ_PIXELS_U8 : HQ_PIXELS_PLANAR;
}

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
    if (!whole_image(c))
        return fail(c, HQ_ERR_STATE, "palette split: every rank needs the whole image (hq_set_image)");
    *n = P / R;
    *lo = r * *n;
    return HQ_OK;
}

// The fast launch's tile grid under the options in force: 8-row tiles (cost_mfma_kernel) and
// 256-column tiles exist for the 21-tap bucket only; dE2000's grid starts at a tile row.
struct FastGrid { int rows, tw, row0, tiles_x, ntiles; };
FastGrid fast_grid(const hq_ctx* c) {
    FastGrid f{};
    f.rows = c->fast_hb == 10 ? c->cost_rows : 16;
    f.tw = c->fast_hb == 10 ? c->cost_tw : 128;
    f.row0 = fast_grid_row0(c->de_type, c->g.r0, f.rows);
    fast_tile_dims(c->g.W, c->g.r1 - f.row0, f.rows, f.tw, &f.tiles_x, &f.ntiles);
    return f;
}
// (the live-tile list on the device is that launch's)
bool live_tiles_current(const hq_ctx* c, const FastGrid& f) {
    return !c->live_dirty && f.rows == c->live_rows && f.tw == c->live_tw &&
           c->live_skip == (c->mask_skip && !c->pixel_err);
}

// The argmin grid's levels: resolutions, bytes per palette (level 1) and per 4 palettes (level 2).
struct GridLayout { int G1, G2; int64_t l1p, l2g; };
GridLayout grid_layout(const hq_ctx* c) {
    const int G2 = c->G2 > 0 ? c->G2 : 4, G1 = G2 / 4;
    return GridLayout{G1, G2, round_up((int64_t)G1 * G1 * G1 * 32, 256),
                      round_up((int64_t)G2 * G2 * G2 * kL2Line, 256)};
}

void lab_matrix(const hq_ctx* c, float m[9]) {
    const float inv[3] = {1.0f / c->illum[0], 1.0f / c->illum[1], 1.0f / c->illum[2]};
    opp2xyz_over_illum(inv, m);  // (the cost kernels' m_lab)
}

}  // namespace

namespace hq {

void drop(hq_ctx* c) { c->res = Resident{}; }
void commit(hq_ctx* c, const Resident& r) { c->res = r; }

Resident resident_of(hq_ctx* c, Resident::Owner owner, int P, int K) {
    int lo = 0, n = P;
    (void)palette_slice(c, P, &lo, &n);  // (the pass has taken this slice: it cannot fail here)
    const bool fast = cost_fast(c) && !(K > kMaxK && c->nch_cur == 1);  // (enqueue_wide: the generic cost)
    const int64_t all = fast ? fast_grid(c).ntiles : 0;
    return Resident{owner, P, K, c->nch_cur, lo, n, owner != Resident::Search && c->pixel_err,
                    fast && c->mask_on ? c->n_live : all, all};
}

// The live-tile list of the fast cost launch that the population being enqueued will take
// (hq_mask.cpp), on the device.  Its inputs are the mask's owned rows, the launch's tile grid
// (the tile shape, dE2000's shard grid) and whether the launch skips (option "mask_skip", and
// nothing with "pixel_err": every tile then stores its pixels' dE); rebuilt when one of them has
// changed.  The buffer's address sits in captured launches and its contents are read by them, so
// it is written here only -- ensure_population calls this before anything is enqueued or a
// capture begins -- with nothing of the context in flight (every entry point synchronises).
int ensure_live_tiles(hq_ctx* c) {
    if (!c->mask_on || !cost_fast(c)) return HQ_OK;
    const FastGrid f = fast_grid(c);
    if (live_tiles_current(c, f)) return HQ_OK;
    const int skip = c->mask_skip && !c->pixel_err;
    const TileGrid tg{c->g.W, c->g.r0, c->g.r1, f.row0, fast_tile_width(f.rows, f.tw), f.rows, f.tiles_x, f.ntiles};
    std::vector<int32_t> live((size_t)std::max(tg.ntiles, 1));
    const int n = mask_live_tiles(c->mask_own.data(), tg, skip != 0, live.data());
    if (int rc = bind(c)) return rc;
    HIP_TRY(c, c->d_live.ensure(sizeof(int32_t) * live.size()));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(c->d_live.p, live.data(), sizeof(int32_t) * live.size(), hipMemcpyHostToDevice));
    c->n_live = n;
    c->live_rows = f.rows, c->live_tw = f.tw, c->live_skip = skip;
    c->live_dirty = false;
    return HQ_OK;
}

// Ensure population buffers for P palettes of K colours.
int ensure_population(hq_ctx* c, int P, int K) {
    const Geom& g = c->g;
    // a buffer the record vouches for: ensure frees what it grows, so the record goes first
    auto vouched = [c](DevBuf& b, size_t n) {
        if (n > b.bytes) drop(c);
        return b.ensure(n);
    };
    if (c->nch_cur > 1) {  // chunked palettes: 16-bit indices, then P nch sub-palettes of 256
        HIP_TRY(c, vouched(c->d_idx16, sizeof(uint16_t) * (size_t)P * g.idx_pitch + 256));
        if (c->nch_cur > 4) HIP_TRY(c, c->d_dist.ensure(sizeof(float) * (size_t)P * g.idx_pitch));
        if (use_lists16(c)) {
            HIP_TRY(c, c->d_l1n.ensure(sizeof(uint16_t) * n16_l1_words(K) * (size_t)P * kN16G1 * kN16G1 * kN16G1));
            // (palette pairs interleaved: an odd population's last pair half empty)
            HIP_TRY(c, c->d_l2n.ensure(sizeof(uint16_t) * kN16L2Words * (size_t)(P + 1) / 2 * 2 * kN16G2 * kN16G2 * kN16G2));
        }
        P *= c->nch_cur;  // (d_out, h_out: P nch (1 + 256) >= P (1 + K) doubles)
        K = kMaxK;
    }
    const GridLayout gl = grid_layout(c);
    HIP_TRY(c, c->d_pal_in.ensure(sizeof(float4) * (size_t)P * K));
    HIP_TRY(c, vouched(c->d_pal, sizeof(float4) * (size_t)P * std::max(K, kMaxK)));
    HIP_TRY(c, c->d_opp.ensure(sizeof(float4) * (size_t)P * std::max(K, kMaxK)));
    if (K > kMaxK) {
        HIP_TRY(c, vouched(c->d_idx32, sizeof(uint32_t) * (size_t)P * g.idx_pitch));
        HIP_TRY(c, vouched(c->d_used32, sizeof(uint32_t) * (size_t)P * K));
    }
    HIP_TRY(c, c->d_opp16.ensure(sizeof(uint4) * (size_t)P * kMaxK));
    HIP_TRY(c, c->d_dup.ensure((size_t)P * kMaxK));
    HIP_TRY(c, c->d_pflags.ensure(sizeof(int) * (size_t)P));
    HIP_TRY(c, c->d_lvl1.ensure((size_t)P * gl.l1p));
    HIP_TRY(c, c->d_lvl2.ensure((size_t)((P + 3) / 4) * gl.l2g));
    // + 256: the cost kernels' interior fills read whole dword pairs, up to 7
    // bytes past a region's last column (past the buffer on the last palette's
    // last row when idx_pitch has no padding)
    HIP_TRY(c, vouched(c->d_idx, (size_t)P * g.idx_pitch + 256));
    const size_t rb = (size_t)rank_blocks(c);  // counter / used-bit blocks per set
    HIP_TRY(c, vouched(c->d_used_mask, 2 * rb * sizeof(uint32_t) * kUsedSlots * (size_t)used_stride(P)));
    HIP_TRY(c, vouched(c->d_acc, 2 * rb * sizeof(uint64_t) * acc_words(P)));
    HIP_TRY(c, c->d_out.ensure(sizeof(double) * (size_t)P * (1 + K)));
    if (c->pixel_err) HIP_TRY(c, vouched(c->d_pixerr, sizeof(float) * (size_t)P * std::max<int64_t>(n_own(g), 1)));
    // the generic path's [7][n_ext] scratch, here rather than at its first launch: an
    // allocation cannot happen while a search run is being captured into a graph
    if (!cost_fast(c) || K > kMaxK) HIP_TRY(c, c->d_gen_t.ensure(sizeof(float) * 7 * (size_t)g.n_ext + 256));
    HIP_TRY(c, c->h_pal.ensure(sizeof(float) * 4 * (size_t)P * K));
    HIP_TRY(c, c->h_out.ensure(sizeof(double) * (size_t)P * (1 + K)));
    if (c->assign_space) {  // the argmin's own views: the palettes' coordinates, the pixels'
        HIP_TRY(c, c->d_arg.ensure(sizeof(float4) * (size_t)P * std::max(K, kMaxK)));
        if (int rc = ensure_assign_coords(c)) return rc;
    }
    return ensure_live_tiles(c);  // (a pixel mask on the fast path: the list its launch reads)
}

// The pixels' coordinate planes under option "assign_space" 1: allocated at the image planes'
// size and filled by one launch from the packed copy when the context has one, else from the
// planar floats -- both hold the same k/255 (u8_unit), so the option "img_u8" does not matter
// here.  Stale after a new image or illuminant (begin_image).  The launch is enqueued on the
// context's stream, in front of the pass that reads the planes.
int ensure_assign_coords(hq_ctx* c) {
    if (c->coords_ok || !c->have_image) return HQ_OK;
    if (int rc = bind(c)) return rc;
    const int64_t quads = round_up(c->g.n_ext, 4) / 4;
    const size_t plane = sizeof(float) * 4 * (size_t)quads;
    HIP_TRY(c, c->d_cR.ensure(plane));
    HIP_TRY(c, c->d_cG.ensure(plane));
    HIP_TRY(c, c->d_cB.ensure(plane));
    CoordArgs a{c->img_u8 ? c->d_rgbx.as<uint32_t>() : nullptr, c->d_R.as<float>(), c->d_G.as<float>(),
                c->d_B.as<float>(), c->d_cR.as<float>(), c->d_cG.as<float>(), c->d_cB.as<float>(), c->g.n_ext, quads, {}};
    inv_illuminant(c, a.inv_illum);
    // (profiling: timed here and now -- once per image, so the synchronise costs nothing that
    // matters, and the context's events are free again for the pass that follows)
    ProfRec pr = prof_begin(c);
    HIP_TRY(c, timed_launch(pr, kPCoords, [&] { return launch_coords(a, c->stream); }));
    if (pr.ev) {
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        prof_accumulate(c, pr);
    }
    c->coords_ok = true;
    return HQ_OK;
}

int assign_space_excludes(hq_ctx* c, const char* what) {
    if (!c->assign_space) return HQ_OK;
    return fail(c, HQ_ERR_UNSUPPORTED, "%s under option assign_space 1 (CIELAB nearest colour): it keeps the sRGB "
                                       "rule, set assign_space 0", what);
}

PaletteArgs prep_args(hq_ctx* c, int K) {
    PaletteArgs a{c->d_pal_in.as<float4>(), c->d_pal.as<float4>(), c->d_opp.as<float4>(),
                  c->d_opp16.as<uint4>(), c->d_dup.as<uint8_t>(), c->d_pflags.as<int>(), K,
                  c->assign_space ? c->d_arg.as<float4>() : c->d_pal.as<float4>(), c->assign_space, {}};
    inv_illuminant(c, a.inv_illum);
    return a;
}

// Counter set `par` of an evaluation of P palettes (P nch sub-palettes Ps).
uint64_t* acc_base(hq_ctx* c, int par, int P) {
    return c->d_acc.as<uint64_t>() + (size_t)par * rank_blocks(c) * acc_words(P);
}
uint32_t* used_base(hq_ctx* c, int par, int Ps) {
    return c->d_used_mask.as<uint32_t>() + (size_t)par * rank_blocks(c) * kUsedSlots * used_stride(Ps);
}

}  // namespace hq

namespace {

uint64_t* acc_set(hq_ctx* c, int par, int P) { return acc_base(c, par, P) + (size_t)own_block(c) * acc_words(P); }
uint32_t* used_set(hq_ctx* c, int par, int Ps) {
    return used_base(c, par, Ps) + (size_t)own_block(c) * kUsedSlots * used_stride(Ps);
}

GridArgs grid_args(hq_ctx* c, int P, int K, int so = 0) {
    const GridLayout gl = grid_layout(c);
    // (P = sub-palettes; the counters of set c->acc_par)
    const int nch = c->nch_cur;
    // option "assign_space": the argmin's table is the palettes' coordinates (PaletteArgs::arg);
    // the grid, the native lists and assign all take it from here (ga.pal)
    const float4* const table = c->assign_space ? c->d_arg.as<float4>() : c->d_pal.as<float4>();
    // (so: the first of the P sub-palettes in the prepared tables, a palette split's slice)
    return GridArgs{table + (int64_t)so * kMaxK, c->d_dup.as<uint8_t>() + (int64_t)so * kMaxK,
                    c->d_pflags.as<int>() + so, c->d_lvl1.as<uint8_t>(), c->d_lvl2.as<uint8_t>(),
                    used_set(c, c->acc_par, P),
                    used_stride(P), K, gl.G1, gl.l1p, gl.l2g,
                    acc_set(c, c->acc_par, P / nch), P / nch, nch};
}

// The generic two-pass cost (CL:234-306 per pixel, any half-width) of P
// palettes, one launch pair each: index images at idx_base (u8, u16 (chunked
// palettes) or u32: idx_bytes) with c->g.idx_pitch elements per palette, opponent
// tables of opp_stride entries per palette in d_opp.  Pair `cost` times all P pairs.
int enqueue_generic_cost(hq_ctx* c, int P, const void* idx_base, int idx_bytes, int opp_stride, ProfRec& pr,
                         Pair cost, hq_path_info& pi, int p_off = 0) {
    const Geom& g = c->g;
    hipStream_t s = c->stream;
    GenTag gt;
    HIP_TRY(c, c->d_gen_t.ensure(sizeof(float) * 7 * (size_t)g.n_ext + 256));
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
        gn.pix_err = c->pixel_err ? c->d_pixerr.as<float>() + (int64_t)p * n_own(g) : nullptr;
        gn.mask = c->mask_on ? c->d_mask.as<uint8_t>() : nullptr;
        pi.cost_instance = !c->mask_on ? HQ_INSTANCE_PLAIN : c->weights_on ? HQ_INSTANCE_WEIGHTED : HQ_INSTANCE_MASKED;
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
        lab_matrix(c, gn.m_lab);
        // the events span every palette's launch pair: start on the first, stop on the last;
        // cost_variant 2: the per-pixel pair in the reference's summation order
        HIP_TRY(c, timed_launch(pr, cost, [&] {
            return c->cost_variant == 2 ? launch_cost_generic(gn, c->de_type, idx_bytes, s, &gt)
                                        : launch_cost_tiled_generic(gn, c->de_type, idx_bytes, s, &gt);
        }, p == 0, p == P - 1));
    }
    pi.cost = gt.cost, pi.cost_de = c->de_type;
    pi.gen_h = gt.h, pi.gen_h_outputs = gt.h_outputs, pi.gen_h_split = gt.h_split, pi.gen_h_rpt = gt.h_rpt;
    pi.gen_v = gt.v, pi.gen_v_rows = gt.v_rows;
    pi.idx_bytes = idx_bytes;
    return HQ_OK;
}

// The collective that ends a pass of P palettes (this device's: [lo, lo + Pl), Ps
// sub-palettes) on a context with a communicator, under the comm pair (profiling
// only: an event record between launches idles the GPU a few us, so the timed pass
// of bench.py records none).
int enqueue_collective(hq_ctx* c, bool fold, int P, int K, int lo, int Pl, int Ps, ProfRec& pr) {
    hipStream_t s = c->stream;
    if (pr.ev) {
        HIP_TRY(c, hipEventRecord(pr.ev[2 * kPComm], s));
        pr.recorded |= 1u << kPComm;
    }
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
    } else if (c->psplit) {  // every rank's slice of d_out to every rank (in place; one rank: a no-op)
        NCCL_TRY(c, ncclAllGather(c->d_out.as<double>() + (int64_t)lo * (1 + K), c->d_out.p,
                                  (size_t)Pl * (1 + K), ncclFloat64, c->comm, s));
    } else {  // also with one rank (a no-op copy), so that path is exercised on one GPU
        NCCL_TRY(c, ncclAllReduce(c->d_out.p, c->d_out.p, (size_t)P * (1 + K), ncclFloat64, ncclSum,
                                  c->comm, s));
    }
    if (pr.ev) HIP_TRY(c, hipEventRecord(pr.ev[2 * kPComm + 1], s));
    return HQ_OK;
}

// A pass over P palettes begins: the slice [lo, lo + Pl) this device takes; on a test-only
// slice the other palettes' rows of d_out zeroed (writes_out: the pass ends in d_out); the
// other counter set taken.  A side pass hands the set back on every way out (ParRestore).
int begin_pass(hq_ctx* c, int P, int K, bool writes_out, int* lo, int* Pl) {
    if (int rc = palette_slice(c, P, lo, Pl)) return rc;
    if (*Pl < P && !c->comm && writes_out)  // test-only slice: the other palettes' rows read as zero
        HIP_TRY(c, hipMemsetAsync(c->d_out.p, 0, sizeof(double) * (size_t)P * (1 + K), c->stream));
    c->acc_par ^= 1;
    return HQ_OK;
}
struct ParRestore { hq_ctx* c; bool on; ~ParRestore() { if (on) c->acc_par ^= 1; } };
// ... and ends: finalize into this device's rows of d_out (not a folding search's, whose accept
// step reads the sums itself), then the collective.  A side pass has neither.
int end_pass(hq_ctx* c, const Pass& pass, const FinalizeArgs& fa, int P, int K, int lo, int Pl, int Ps,
             ProfRec& pr) {
    if (pass.side()) return HQ_OK;
    if (pass.kind != Pass::Fold)
        HIP_TRY(c, timed_launch(pr, Pair(pass.pairs() + 3), [&] { return launch_finalize(fa, Pl, c->stream); }));
    return c->comm ? enqueue_collective(c, pass.kind == Pass::Fold, P, K, lo, Pl, Ps, pr) : HQ_OK;
}

// K > 256 (hq_wide.hip): prep, exhaustive argmin into 32-bit indices and
// per-colour used flags, the generic cost, finalize, [all-reduce or, under a
// palette split, all-gather].  A palette split takes the same slice
// [lo, lo + Pl) as enqueue_core: the other ranks' palettes are prepped here
// too (cheap) but neither assigned nor costed, so no rank counts them.
int enqueue_wide(hq_ctx* c, int P, int K, ProfRec& pr) {
    const Geom& g = c->g;
    hipStream_t s = c->stream;
    int lo = 0, Pl = P;
    if (int rc = begin_pass(c, P, K, true, &lo, &Pl)) return rc;
    hq_path_info pi{};
    pi.pass = HQ_PASS_FULL, pi.P = Pl, pi.K = K, pi.nch = 1;
    // (this path has no fast cost to decline: HQ_WHY_WIDE is its own bit, and the others say what
    // the state it was entered in would have kept from the fast kernels anyway -- run_pass sends a
    // palette outside the range here, a long filter goes to the generic pair on every path)
    pi.why_not_fast = cost_slow_why(c) | HQ_WHY_WIDE;
    AssignTag at;
    WideArgs wa{c->d_pal_in.as<float4>(), c->d_pal.as<float4>(), c->d_opp.as<float4>(), c->d_pflags.as<int>(),
                c->d_R.as<float>(), c->d_G.as<float>(), c->d_B.as<float>(), c->d_idx32.as<uint32_t>(),
                c->d_used32.as<uint32_t>(), g.n_ext, g.idx_pitch, K};
    HIP_TRY(c, hipMemsetAsync(acc_set(c, c->acc_par, Pl), 0, sizeof(uint64_t) * acc_words(Pl), s));
    HIP_TRY(c, hipMemsetAsync(c->d_pflags.p, 0, sizeof(int) * (size_t)P, s));
    HIP_TRY(c, launch_prep_wide(wa, P, s));
    HIP_TRY(c, hipMemsetAsync(c->d_used32.p, 0, sizeof(uint32_t) * (size_t)Pl * K, s));
    // the slice's palettes: indices and used flags in rows 0 .. Pl - 1
    WideArgs ws = wa;
    ws.pal += (int64_t)lo * K;
    ws.opp += (int64_t)lo * K;
    ws.pflags += lo;
    HIP_TRY(c, timed_launch(pr, kPAssign, [&] { return launch_assign_wide(ws, Pl, s, &at); }));
    record_argmin(pi, at);
    if (int rc = enqueue_generic_cost(c, Pl, c->d_idx32.p, 4, K, pr, kPCost, pi, lo)) return rc;
    record_path(c, pi);
    const FinalizeArgs fa{acc_set(c, c->acc_par, Pl), nullptr, 0, c->d_out.as<double>() + (int64_t)lo * (1 + K), Pl,
                          K, c->d_used32.as<uint32_t>(), 8};
    return end_pass(c, Pass{}, fa, P, K, lo, Pl, Pl, pr);
}

// ---- the stages of enqueue_core ---------------------------------------------------
// The grid (build_grid or the native 16-bit lists; both also zero the used bits and the sums),
// or without one -- G2 = 0, a dithered pass -- the zeroing.
int enqueue_grid(hq_ctx* c, const GridArgs& ga, bool build, bool n16, int K, int Pl, int Ps, Pair pgrid,
                 ProfRec& pr, hq_path_info& pi) {
    hipStream_t s = c->stream;
    if (!build) {
        pi.grid = HQ_GRID_NONE;
        HIP_TRY(c, hipMemsetAsync(ga.used_glob, 0, sizeof(uint32_t) * kUsedSlots * (size_t)used_stride(Ps), s));
        HIP_TRY(c, hipMemsetAsync(ga.acc_zero, 0, sizeof(uint64_t) * acc_words(Pl), s));
        return HQ_OK;
    }
    const int nch = c->nch_cur;
    HIP_TRY(c, timed_launch(pr, pgrid, [&] {
        if (n16) {
            pi.grid = HQ_GRID_LISTS16;
            return launch_lists16_grid(Lists16Args{ga.pal, ga.pflags, c->d_l1n.as<uint16_t>(),
                                                   c->d_l2n.as<uint16_t>(), ga.used_glob, used_stride(Ps),
                                                   ga.acc_zero, Pl, K, nch * kMaxK, nch},
                                       Pl, s);
        }
        pi.grid = HQ_GRID_BUILD_GRID;
        return launch_build_grid(ga, Ps, s);
    }));
    return HQ_OK;
}

// assign over Ps sub-palettes of Ks colours (chunked palettes: into the 16-bit images) ...
AssignArgs assign_args(hq_ctx* c, const GridArgs& ga, int Ps, int Ks, bool ordered) {
    const Geom& g = c->g;
    const int nch = c->nch_cur;
    // option "assign_space" 1: the pixels' coordinate planes and no packed form, so every argmin
    // kernel runs its planar instance on them (ga.pal is the coordinate table already)
    const bool sp = c->assign_space != 0;
    AssignArgs aa{(sp ? c->d_cR : c->d_R).as<float>(), (sp ? c->d_cG : c->d_G).as<float>(),
                  (sp ? c->d_cB : c->d_B).as<float>(),
                  !sp && sums_u8(c) ? c->d_rgbx.as<uint32_t>() : nullptr, ga.pal, ga.pflags,
                  c->d_lvl1.as<uint8_t>(), c->d_lvl2.as<uint8_t>(),
                  c->d_idx.as<uint8_t>(), ga.used_glob, used_stride(Ps), g.n_ext, g.idx_pitch,
                  ga.lvl1_pitch, ga.lvl2_gstride, Ks, c->G2, assign_blocks(c, Ps, ordered)};
    if (nch > 1) {
        aa.idx16 = c->d_idx16.as<uint16_t>();
        aa.dist = nch > 4 ? c->d_dist.as<float>() : nullptr;
        aa.nch = nch;
        while ((1 << aa.lg_nch) < nch) ++aa.lg_nch;
    }
    return aa;
}

// ---- the argmin stage: one function per rendering, each launching under its own pair ---------
// (the native 16-bit lists: one palette of K colours per workgroup, its table in LDS)
hipError_t argmin_plain(hq_ctx* c, AssignArgs& aa, bool n16, int K, int Pl, int Ps, Pair pair, ProfRec& pr,
                        AssignTag* at) {
    if (n16) {
        aa.l1n = c->d_l1n.as<uint16_t>(), aa.l2n = c->d_l2n.as<uint16_t>();
        aa.kpal = c->nch_cur * kMaxK, aa.K = K;
        // one resident round of 1024-thread workgroups over the P palettes, >= 4 pixels per thread
        const int ngr = K <= 4096 ? (Pl + 1) / 2 : Pl;  // workgroup groups: palette pairs up to K = 4096
        aa.nblocks = (int)std::max<int64_t>(
            1, std::min<int64_t>(std::max(1, c->num_cu / ngr), (c->g.n_ext + 4095) / 4096));
    }
    return timed_launch(pr, pair, [&] {
        return n16 ? launch_assign16(aa, Pl, c->stream, at) : launch_assign(aa, Ps, c->stream, at);
    });
}

// (the map is on the device and K <= 256: enqueue_argmin has looked)
hipError_t argmin_ordered(hq_ctx* c, const Ordered& o, AssignArgs& aa, int Ps, Pair pair, ProfRec& pr, AssignTag* at) {
    const int mw = c->dmap.empty() ? 16 : c->dmap_w, mh = c->dmap.empty() ? 16 : c->dmap_h;
    aa.map = c->d_dmap.as<float>();
    aa.mw_mask = (uint32_t)mw - 1u, aa.mh_mask = (uint32_t)mh - 1u;
    while ((1u << aa.lg_mw) < (uint32_t)mw) ++aa.lg_mw;
    for (int ch = 0; ch < 3; ++ch) aa.amp[ch] = o.amp[ch];
    aa.W = (uint32_t)c->g.W, aa.y0 = (uint32_t)c->g.e0;
    return timed_launch(pr, pair, [&] { return launch_assign_ordered(aa, Ps, c->stream, at); });
}

// (HQ_ARGMIN_DITHER, the Floyd-Steinberg formula, reports no instance)
hipError_t argmin_diffused(hq_ctx* c, const Diffused& d, const AssignArgs& aa, const GridArgs& ga, int K, int Pl,
                           ProfRec& pr, AssignTag* at, hq_path_info& pi) {
    const Geom& g = c->g;
    DiffuseArgs da{aa.R, aa.G, aa.B, ga.pal, aa.idx, ga.used_glob, c->d_dcarry.as<float>(), g.idx_pitch,
                   g.W, g.H, K, c->dither_rows, d.rows, d.slope, d.floyd_steinberg, d.strength};
    da.w0[0] = (float)d.taps.w[0][3], da.w0[1] = (float)d.taps.w[0][4];
    for (int i = 0; i < 5; ++i) da.w1[i] = (float)d.taps.w[1][i], da.w2[i] = (float)d.taps.w[2][i];
    da.div = (float)d.taps.div;
    if (!d.floyd_steinberg) pi.diffuse_rows = d.rows, pi.diffuse_slope = d.slope;
    return timed_launch(pr, kPDither, [&] { return launch_diffuse(da, Pl, c->stream, at); });
}

// The form a dot pass over P palettes of K colours takes under the context's matrix (c->dot_cls), one
// function for the scratch (ensure_render_scratch) and the launch (argmin_dot): the tiled kernel on a whole
// image whose matrix dot_tile_eligible admits, under option "dot_tile" 1 always and under -1 (auto) where it
// was measured faster than the chain (hq.h states the rule); else the chain.
bool dot_tiled(const hq_ctx* c, int P, int K, DotTilePlan* plan) {
    if (!whole_image(c) || c->dot_tile == 0 || !c->d_dotsched.p) return false;
    DotTilePlan pl;
    if (c->dot_cls.n == 0 || !dot_tile_eligible(c->dot_info, K, c->dot_tile_shape, &pl)) return false;
    if (c->dot_tile < 0 && !dot_tile_auto(c->g.W, c->g.H, P, K, pl.shape)) return false;
    if (plan) *plan = pl;
    return true;
}

// (the matrix read on the host here is the one whose tables d_dottab holds: ensure_dot_tables)
hipError_t argmin_dot(hq_ctx* c, const Dot& d, const AssignArgs& aa, const GridArgs& ga, int K, int Pl, int Ps,
                      ProfRec& pr, AssignTag* at) {
    const Geom& g = c->g;
    DotTilePlan plan;
    if (dot_tiled(c, Pl, K, &plan)) {
        const DotTileArgs ta{aa.R, aa.G, aa.B, ga.pal, aa.idx, ga.used_glob, c->d_dottab.as<uint32_t>(),
                             c->d_dotsched.as<uint32_t>(), g.idx_pitch, used_stride(Ps), g.W, g.H, K, c->dot_cls.n,
                             d.strength, plan};
        const hipError_t e = timed_launch(pr, kPDot, [&] { return launch_dot_tile(ta, Pl, c->stream, at); });
        if (e == hipSuccess) c->dot_form = 2, c->dot_form_tw = plan.tw, c->dot_form_th = plan.th, c->dot_form_levels = plan.depth;
        return e;
    }
    // (the chain's errors were sized by the same rule: ensure_render_scratch)
    if (c->d_doterr.bytes < sizeof(float) * dot_err_floats(Pl, g.W, whole_image(c) ? g.H : d.a1 - d.a0))
        return hipErrorInvalidValue;
    DotWinArgs wa{};  // (on a whole image the DotArgs in it alone)
    static_cast<DotArgs&>(wa) = DotArgs{aa.R, aa.G, aa.B, ga.pal, aa.idx, ga.used_glob, c->d_doterr.as<float>(),
                                        c->d_dottab.as<uint32_t>(), c->dot_cls.cls, g.idx_pitch, used_stride(Ps), g.W,
                                        g.H, K, c->dot_cls.n, d.strength};
    if (!whole_image(c)) {  // a row-block shard: the window's rows, the apron's planes from the row it holds first
        const int64_t aplane = (int64_t)(c->apron_above + c->apron_below) * g.W;
        const float* ap = c->d_apron.as<float>();
        wa.a0 = d.a0, wa.a1 = d.a1, wa.e0 = g.e0, wa.e1 = g.e1;
        wa.h0 = g.e0 - c->apron_above, wa.h1 = g.e1 + c->apron_below;
        wa.aR = ap, wa.aG = ap ? ap + aplane : nullptr, wa.aB = ap ? ap + 2 * aplane : nullptr;
    }
    const hipError_t e = timed_launch(pr, kPDot, [&] {
        return whole_image(c) ? launch_dot(wa, Pl, c->stream, at) : launch_dot_window(wa, Pl, c->stream, at);
    });
    if (e == hipSuccess) c->dot_form = 1, c->dot_form_tw = c->dot_form_th = 0, c->dot_form_levels = c->dot_info.depth;
    return e;
}

// The index images of `pass`: its rendering's function, then what the launch reported.
int enqueue_argmin(hq_ctx* c, const Pass& pass, const GridArgs& ga, bool n16, int K, int Pl, int Ps, ProfRec& pr,
                   hq_path_info& pi) {
    const Ordered* const o = pass.as<Ordered>();
    if (o && (c->nch_cur > 1 || !c->d_dmap.p)) return fail(c, HQ_ERR_STATE, "ordered pass: K > 256 or no map");
    AssignArgs aa = assign_args(c, ga, Ps, c->nch_cur > 1 ? kMaxK : K, o != nullptr);
    const Pair pair = Pair(pass.pairs() + 1);
    AssignTag at;
    hipError_t launched;
    if (o) launched = argmin_ordered(c, *o, aa, Ps, pair, pr, &at);
    else if (const Diffused* d = pass.as<Diffused>()) launched = argmin_diffused(c, *d, aa, ga, K, Pl, pr, &at, pi);
    else if (const Dot* d = pass.as<Dot>()) launched = argmin_dot(c, *d, aa, ga, K, Pl, Ps, pr, &at);
    else launched = argmin_plain(c, aa, n16, K, Pl, Ps, pair, pr, &at);
    HIP_TRY(c, launched);
    pi.idx_bytes = aa.idx16 ? 2 : 1;
    record_argmin(pi, at);
    return HQ_OK;
}

// The fast cost launch; under a mask its live-tile list, which has to be this launch's.
int cost_args(hq_ctx* c, const GridArgs& ga, const FastGrid& f, int K, int so, int Pl, CostArgs* out) {
    CostArgs ca{};
    ca.idx = c->nch_cur > 1 ? c->d_idx16.as<uint8_t>() : c->d_idx.as<uint8_t>();
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
    ca.g = c->g;
    ca.K = K;
    ca.tiles_x = f.tiles_x;
    ca.ntiles = f.ntiles;
    lab_matrix(c, ca.m_lab);
    ca.pix_err = c->pixel_err ? c->d_pixerr.as<float>() : nullptr;
    ca.pix_pitch = n_own(c->g);
    if (c->mask_on) {
        if (!live_tiles_current(c, f))
            return fail(c, HQ_ERR_STATE, "%s: the live-tile list is not that of this launch", mask_noun(c));
        ca.mask = c->d_mask.as<uint8_t>();
        ca.live = c->d_live.as<int32_t>();
        ca.nlive = c->n_live;
    }
    *out = ca;
    return HQ_OK;
}

// The cost: the fast launch (under a mask over its live tiles, and none without one: the
// zeroed counters are the partial), else the generic pair.
int enqueue_cost(hq_ctx* c, const CostArgs& ca, bool fast, const FastGrid& f, int lo, int Pl, Pair pcost,
                 ProfRec& pr, hq_path_info& pi) {
    hipStream_t s = c->stream;
    const int nch = c->nch_cur, de = c->de_type;
    const bool trim = c->trim && c->trim_ok;
    if (!fast)
        return nch > 1 ? enqueue_generic_cost(c, Pl, c->d_idx16.p, 2, nch * kMaxK, pr, pcost, pi, lo)
                       : enqueue_generic_cost(c, Pl, c->d_idx.p, 1, kMaxK, pr, pcost, pi, lo);
    pi.tiles_all = f.ntiles;
    pi.tiles_run = c->mask_on ? ca.nlive : f.ntiles;
    pi.cost_instance = !c->mask_on ? HQ_INSTANCE_PLAIN : c->weights_on ? HQ_INSTANCE_WEIGHTED : HQ_INSTANCE_MASKED;
    if (c->mask_on && ca.nlive == 0) return HQ_OK;
    CostTag ct;
    HIP_TRY(c, timed_launch(pr, pcost, [&] {
        if (c->mask_on && c->weights_on)
            return nch > 1 ? launch_cost_chunked_weighted(ca, Pl, nch, de, trim, s, &ct)
                           : launch_cost_fast_weighted(ca, Pl, de, trim, f.rows, f.tw, c->fast_hb, s, &ct);
        if (c->mask_on)
            return nch > 1 ? launch_cost_chunked_masked(ca, Pl, nch, de, trim, s, &ct)
                           : launch_cost_fast_masked(ca, Pl, de, trim, f.rows, f.tw, c->fast_hb, s, &ct);
        return nch > 1 ? launch_cost_chunked(ca, Pl, nch, de, trim, s, &ct)
                       : launch_cost_fast(ca, Pl, de, trim, f.rows, f.tw, c->fast_hb, s, &ct);
    }));
    // (the instance is the launcher's own: each of the three translation units reports its MSK)
    pi.cost = ct.kernel, pi.cost_hb = ct.hb, pi.cost_de = ct.de, pi.cost_trim = ct.trim;
    pi.cost_waves = ct.waves, pi.cost_nch = ct.nch, pi.cost_instance = ct.msk;
    return HQ_OK;
}

}  // namespace

// Enqueue pass `pass` (hq_runtime.h: how far it goes, its index images, its
// counter set) over the P prepared palettes of K colours (d_pal, d_opp, d_dup,
// d_pflags).  pr: the launches carry their pairs' events themselves
// (timed_launch), four pairs from pass.pairs().
// Chunked palettes (c->nch_cur = nch > 1, 256 < K <= 256 nch): the grid and
// assign run on P nch sub-palettes of 256 colours (d_pal etc. hold them,
// prep_palette made them), assign combines them into 16-bit indices, the cost
// kernel reads those with a 256 nch-entry table.
// What it leaves on the device is the caller's to commit (resident_of).
int hq::enqueue_core(hq_ctx* c, int P, int K, ProfRec& pr, const Pass& pass) {
    const int nch = c->nch_cur, Ks = nch > 1 ? kMaxK : K;
    const bool costed = pass.kind != Pass::AssignOnly;
    const int p0 = pass.pairs();
    // the palettes this device evaluates: all, or a palette split's slice [lo, lo + Pl)
    int lo = 0, Pl = P;
    if (int rc = begin_pass(c, P, K, costed, &lo, &Pl)) return rc;
    const ParRestore restore{c, pass.side()};
    const int Ps = Pl * nch, so = lo * nch;  // sub-palettes, the first one's index
    const GridArgs ga = grid_args(c, Ps, Ks, so);
    const bool n16 = use_lists16(c);
    hq_path_info pi{};
    pi.pass = pass.gridless() ? HQ_PASS_DITHER : costed ? HQ_PASS_FULL : HQ_PASS_ASSIGN_ONLY;
    pi.ordered = pass.as<Ordered>() != nullptr, pi.P = Pl, pi.K = K, pi.nch = nch;
    if (int rc = enqueue_grid(c, ga, c->G2 > 0 && !pass.gridless(), n16, K, Pl, Ps, Pair(p0), pr, pi)) return rc;
    const uint32_t why = cost_slow_why(c);  // (cost_fast)
    const bool fast = why == 0;
    const FastGrid f = fast_grid(c);
    CostArgs ca{};
    if (fast)
        if (int rc = cost_args(c, ga, f, K, so, Pl, &ca)) return rc;
    if (int rc = enqueue_argmin(c, pass, ga, n16, K, Pl, Ps, pr, pi)) return rc;
    if (costed) {
        pi.why_not_fast = why;
        if (int rc = enqueue_cost(c, ca, fast, f, lo, Pl, Pair(p0 + 2), pr, pi)) return rc;
    }
    record_path(c, pi);
    const FinalizeArgs fa{ga.acc_zero, ga.used_glob, used_stride(Ps), c->d_out.as<double>() + (int64_t)lo * (1 + K),
                          Pl, K, nullptr, 8 * nch};
    return end_pass(c, pass, fa, P, K, lo, Pl, Ps, pr);
}

namespace hq {

int upload_and_prep(hq_ctx* c, const float* host, const void* dev, int P, int K) {
    hipStream_t s = c->stream;
    const int nch = c->nch_cur;
    const size_t n_in = (size_t)P * (nch > 1 ? nch * kMaxK : K);
    if (host) {
        if (nch > 1) pack_chunks(host, P, K, nch, c->h_pal.as<float>());
        else std::memcpy(c->h_pal.p, host, sizeof(float) * 4 * n_in);
        HIP_TRY(c, hipMemcpyAsync(c->d_pal_in.p, c->h_pal.p, sizeof(float4) * n_in, hipMemcpyHostToDevice, s));
    } else {
        HIP_TRY(c, hipMemcpyAsync(c->d_pal_in.p, dev, sizeof(float4) * n_in, hipMemcpyDeviceToDevice, s));
    }
    if (nch == 1 && K > kMaxK) return HQ_OK;
    HIP_TRY(c, launch_prep_palette(prep_args(c, nch > 1 ? kMaxK : K), P * nch, s));
    return HQ_OK;
}

}  // namespace hq

namespace {

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
bool palette_fits_fast(const float* pal, int P, int K) {
    for (size_t i = 0, n = (size_t)P * K; i < n; ++i)
        for (int ch = 0; ch < 3; ++ch) {
            const float x = pal[4 * i + ch];
            if (!(x >= -32.0f && x <= 1.9f)) return false;
        }
    return true;
}

// The scratch a rendering needs -- dot diffusion's errors over the rows rendered (the chain's), a raster diffusion's carry
// rows -- ensured by run_pass before anything is enqueued: nothing allocates between prof_begin and the
// synchronise; a search under the dot-diffused cost asks for it before its run's capture begins (ensure_dot_pass),
// so nothing allocates inside a captured run (its other passes are plain or ordered and need none).
int ensure_render_scratch(hq_ctx* c, const Pass& pass, int P, int K) {
    if (const Dot* d = pass.as<Dot>(); d && !dot_tiled(c, P, K, nullptr))  // (the tiled form keeps its errors in LDS)
        HIP_TRY(c, c->d_doterr.ensure(sizeof(float) * dot_err_floats(P, c->g.W, whole_image(c) ? c->g.H : d->a1 - d->a0)));
    if (const Diffused* d = pass.as<Diffused>())
        HIP_TRY(c, c->d_dcarry.ensure(sizeof(float) * diffuse_carry_floats(P, d->rows, c->g.W)));
    return HQ_OK;
}

// One host-driven pass, after the caller's last refusal: upload, prep, `pass` (K > 256
// unchunked: enqueue_wide), d_out back into h_out ([P][1 + K]).  The record is dropped before
// the first buffer is grown or written and committed when the pass has come back.
// 256 < K <= 16384: chunks of 256 colours through the grid and assign, and the tiled cost
// kernel up to 32 chunks.  Palettes outside the fast range (never a rendering's) take the
// exhaustive K > 256 path instead, which keeps the reference's NaN semantics.
int run_pass(hq_ctx* c, const float* palettes, int P, int K, const Pass& pass) {
    if (int rc = bind(c)) return rc;
    const bool fits = palette_fits_fast(palettes, P, K);
    const int nch = c->chunked && fits && c->G2 > 0 && K > kMaxK && K <= kMaxKChunked ? chunk_count(K) : 1;
    if (K > kMaxK && nch == 1)  // (enqueue_wide: its argmin reads the colours themselves)
        if (int rc = assign_space_excludes(c, "K > 256 outside the chunked path (K > 16384, option chunked 0, grid 0 or "
                                              "a palette outside the fast range)"))
            return rc;
    drop(c);
    struct Reset {  // device-resident searches generate clamped palettes of their own chunk count
        hq_ctx* c;
        ~Reset() { c->pal_generic = false, c->nch_cur = 1; }
    } reset{c};
    c->nch_cur = nch;
    c->pal_generic = !fits;  // (before ensure_population: it sizes the generic path's scratch)
    if (int rc = ensure_population(c, P, K)) return rc;
    if (int rc = ensure_render_scratch(c, pass, P, K)) return rc;
    hipStream_t s = c->stream;
    ProfRec pr = prof_begin(c);
    int rc = upload_and_prep(c, palettes, nullptr, P, K);
    if (!rc) rc = K > kMaxK && c->nch_cur == 1 ? enqueue_wide(c, P, K, pr) : enqueue_core(c, P, K, pr, pass);
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->h_out.p, c->d_out.p, sizeof(double) * (size_t)P * (1 + K), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    prof_accumulate(c, pr);
    commit(c, resident_of(c, pass.rendered() ? Resident::Render : Resident::Eval, P, K));
    return HQ_OK;
}

int eval_partial_into_hout(hq_ctx* c, const float* palettes, int P, int K) {
    if (int rc = check_eval_args(c, palettes, P, K)) return rc;
    if (int rc = mask_scope(c)) return rc;
    return run_pass(c, palettes, P, K, Pass{});
}

// The index images of a pass over K colours in nch chunks: their base and element width.
const void* index_images(const hq_ctx* c, int K, int nch, int* idx_bytes) {
    *idx_bytes = nch > 1 ? 2 : K > kMaxK ? 4 : 1;
    return *idx_bytes == 2 ? c->d_idx16.p : *idx_bytes == 4 ? c->d_idx32.p : c->d_idx.p;
}

// P, K are the last evaluation's (by hq_eval_population[_partial], on this image,
// no search run since) and every palette's index image is on this device.
int check_last_population(hq_ctx* c, int P, int K) {
    const Resident& r = c->res;
    if (!c->have_image || !r.sums_ok())
        return fail(c, HQ_ERR_STATE, "no population evaluated by hq_eval_population[_partial] on this image "
                                     "since the last search run");
    if (P != r.P || K != r.K)
        return fail(c, HQ_ERR_STATE, "P=%d, K=%d: the last evaluation had P=%d, K=%d", P, K, r.P, r.K);
    if (r.n != r.P || c->slice_ranks > 1 || (c->psplit && c->comm))
        return fail(c, HQ_ERR_UNSUPPORTED, "palette slice: this device holds %d of the %d index images", r.n, r.P);
    return HQ_OK;
}

// hq_get_indices[32], hq_get_pixel_errors: the index images on the device are those of an
// evaluation on the image and filters in force (Resident::idx_ok), and palette p of
// that population is on this device: *local, its place among them.
int check_local_palette(hq_ctx* c, int p, int* local) {
    const Resident& r = c->res;
    if (!c->have_image || !r.idx_ok())
        return fail(c, HQ_ERR_STATE, "no population evaluated on the current image and filters (the image or the "
                                     "filters were set, or an evaluation failed, since the last one)");
    if (p < 0 || p >= r.P) return fail(c, HQ_ERR_ARG, "palette %d not in last population", p);
    if (p < r.lo || p >= r.lo + r.n)
        return fail(c, HQ_ERR_ARG, "palette %d was evaluated on another rank (palette split)", p);
    *local = p - r.lo;
    return HQ_OK;
}

const char* const kNoExactSums = "planar image with a pixel outside [0, 1] or not finite: no exact sums";
int64_t sums_den(const hq_ctx* c) { return sums_u8(c) ? 255 : (int64_t)1 << 32; }

// One call of a table kernel: `table` (n 64-bit words, then the kernel's flag) zeroed; launch(),
// which builds its arguments now that the table is in place; table and flag back into h [and
// extra_src into extra_dst] after one synchronise.  A set flag refuses with `bad` (null: never).
template <typename Launch>
int run_table_kernel(hq_ctx* c, DevBuf& table, size_t n, Pair pair, const char* bad, std::vector<int64_t>& h,
                     Launch&& launch, void* extra_dst = nullptr, const DevBuf* extra_src = nullptr,
                     size_t extra_bytes = 0) {
    if (int rc = bind(c)) return rc;
    hipStream_t s = c->stream;
    const size_t bytes = sizeof(int64_t) * (n + 1);
    HIP_TRY(c, table.ensure(bytes));
    HIP_TRY(c, hipMemsetAsync(table.p, 0, bytes, s));
    ProfRec pr = prof_begin(c);
    HIP_TRY(c, timed_launch(pr, pair, launch));
    h.resize(n + 1);
    HIP_TRY(c, hipMemcpyAsync(h.data(), table.p, bytes, hipMemcpyDeviceToHost, s));
    if (extra_dst) HIP_TRY(c, hipMemcpyAsync(extra_dst, extra_src->p, extra_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    prof_accumulate(c, pr);
    if (bad && h[n] != 0) return fail(c, HQ_ERR_UNSUPPORTED, "%s", bad);
    return HQ_OK;
}

// hq_color_histogram into `out` ([2^(3 bits)][4]); nothing is written unless
// HQ_OK.  The image buffers are read, a table of its own is written: the index
// images, the counter sets and d_sums stay what they are.
int color_histogram(hq_ctx* c, int bits, int64_t* out, int64_t* den) {
    if (int rc = weighted_sums_scope(c, "hq_color_histogram")) return rc;
    const size_t n4 = (size_t)4 << (3 * bits);
    std::vector<int64_t> h;
    int rc = run_table_kernel(c, c->d_hist, n4, kPHist, kNoExactSums, h, [&] {
        HistArgs ha{};
        ha.R = c->d_R.as<float>();
        ha.G = c->d_G.as<float>();
        ha.B = c->d_B.as<float>();
        ha.rgbx = sums_u8(c) ? c->d_rgbx.as<uint32_t>() : nullptr;
        ha.cells = c->d_hist.as<unsigned long long>();
        ha.bad = reinterpret_cast<int*>(c->d_hist.as<int64_t>() + n4);
        owned_range(c->g, &ha.q0, &ha.q1);
        ha.bits = bits;
        ha.mask = c->mask_on ? c->d_maskq.as<uint8_t>() : nullptr;
        ha.weighted = c->mask_on && c->weights_on;
        return launch_color_histogram(ha, c->num_cu, c->stream);
    });
    if (rc) return rc;
    std::memcpy(out, h.data(), sizeof(int64_t) * n4);
    *den = sums_den(c);
    return HQ_OK;
}

// IM:712 from the [P][1+K] rows in h_out: averageArray(error) + computePenalty(used).
// After an all-reduce the used entries count the ranks using colour k; unused <=> 0.
// partial_from_hout: the rows themselves, as a _partial call returns them.  (Both return HQ_OK:
// the last line of an entry point whose pass has come back.)
int costs_from_hout(const hq_ctx* c, int P, int K, float delta, double* costs, int32_t* used) {
    const double n_total = cost_divisor(c);  // (a pixel mask: its pixels in the full image)
    for (int p = 0; p < P; ++p) {
        const double* o = c->h_out.as<double>() + (size_t)p * (1 + K);
        double penalty = 0.0;
        for (int k = 0; k < K; ++k) {
            const bool u = o[1 + k] != 0.0;
            if (!u) penalty += delta;
            if (used) used[(size_t)p * K + k] = u ? 1 : 0;
        }
        costs[p] = o[0] / n_total + penalty;
    }
    return HQ_OK;
}
int partial_from_hout(const hq_ctx* c, int P, int K, double* partial) {
    std::memcpy(partial, c->h_out.p, sizeof(double) * (size_t)P * (1 + K));
    return HQ_OK;
}

// The improvement loop of hq_refine_population and hq_repair_population: evaluate,
// then `steps` times move(cur, &changed) -> status on the palettes in place and
// evaluate again, tracing every evaluation's costs and returning the last
// population or, keep_best, each palette's best.  A move that changed nothing
// ends the loop: the remaining steps would repeat this one, and the trace says so.
template <typename Move>
int improve_population(hq_ctx* c, float* palettes, int P, int K, int steps, float delta, int keep_best,
                       double* costs, int32_t* used, double* trace, Move&& move) {
    const size_t n4 = (size_t)P * K * 4, nu = (size_t)P * K;
    std::vector<float> cur(palettes, palettes + n4), best_pal;
    std::vector<double> cst(P), best_cost;
    std::vector<int32_t> usd(nu), best_used;
    int rc;
    if ((rc = hq_eval_population(c, cur.data(), P, K, delta, cst.data(), usd.data()))) return rc;
    if (trace) std::copy(cst.begin(), cst.end(), trace);
    if (keep_best) best_pal = cur, best_cost = cst, best_used = usd;
    for (int s = 1; s <= steps; ++s) {
        bool changed = true;
        if ((rc = move(cur.data(), &changed))) return rc;
        if (!changed) {
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

// The argument checks hq_refine_population and hq_repair_population share (`what`: the call's
// name, hint: what a multi-rank caller does instead).
int check_improve_args(hq_ctx* c, const float* palettes, int P, int K, int steps, const double* costs,
                       const char* what, const char* hint) {
    if (!costs) return fail(c, HQ_ERR_ARG, "null output");
    if (int rc = check_eval_args(c, palettes, P, K)) return rc;
    if (steps < 0) return fail(c, HQ_ERR_ARG, "steps=%d < 0", steps);
    if (c->fixed_n > K)
        return fail(c, HQ_ERR_ARG, "%d fixed colours (hq_set_fixed_colors) in palettes of K=%d", c->fixed_n, K);
    // (option "palette_split" without a communicator slices nothing: these two go on)
    return whole_image_only(c, what, hint, false);
}

}  // namespace

namespace hq {

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

// The sums kernel's arguments for the index images of a pass over P palettes of K
// colours in nch chunks (the last evaluation's, or an assign-only pass's): the owned
// rows, as hq_get_indices[32] reads them, into d_sums ([P][K][4], then the range flag).
ClusterArgs cluster_args(hq_ctx* c, int P, int K, int nch, int* idx_bytes) {
    ClusterArgs ca{};
    ca.idx = index_images(c, K, nch, idx_bytes);
    ca.R = c->d_R.as<float>();
    ca.G = c->d_G.as<float>();
    ca.B = c->d_B.as<float>();
    ca.rgbx = sums_u8(c) ? c->d_rgbx.as<uint32_t>() : nullptr;
    ca.sums = c->d_sums.as<unsigned long long>();
    ca.bad = reinterpret_cast<int*>(c->d_sums.as<int64_t>() + (size_t)P * K * 4);
    ca.idx_pitch = c->g.idx_pitch;
    owned_range(c->g, &ca.q0, &ca.q1);
    ca.P = P;
    ca.K = K;
    ca.mask = c->mask_on ? c->d_maskq.as<uint8_t>() : nullptr;
    ca.weighted = c->mask_on && c->weights_on;
    ca.span = (uint32_t)c->cent_span;
    return ca;
}

// hq_cluster_sums into `out` ([P][K][4]); nothing is written unless HQ_OK.
int cluster_sums(hq_ctx* c, int P, int K, int64_t* out, int64_t* den) {
    if (int rc = check_last_population(c, P, K)) return rc;
    if (int rc = weighted_sums_scope(c, "hq_cluster_sums")) return rc;
    const size_t n4 = (size_t)P * K * 4;
    std::vector<int64_t> h;
    int rc = run_table_kernel(c, c->d_sums, n4, kPSums, kNoExactSums, h, [&] {
        int idx_bytes = 1;
        const ClusterArgs ca = cluster_args(c, P, K, c->res.nch, &idx_bytes);
        return launch_cluster_sums(ca, idx_bytes, c->num_cu, c->stream);
    });
    if (rc) return rc;
    std::memcpy(out, h.data(), sizeof(int64_t) * n4);
    *den = sums_den(c);
    return HQ_OK;
}

// The error kernel's arguments for the index images, the error image and the
// prepared palettes of a pass over P palettes of K colours in nch chunks, into
// d_errstat ([P][K][4], then the flag) and d_worst ([P][K]).
ClusterErrArgs cluster_err_args(hq_ctx* c, int P, int K, int nch, int* idx_bytes) {
    const Geom& g = c->g;
    const ClusterArgs ca = cluster_args(c, P, K, nch, idx_bytes);
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
    ea.err_pitch = n_own(g);
    // chunked palettes: a palette's nch sub-palettes of 256 lie back to back, colour k at k
    ea.pal_pitch = nch > 1 ? (int64_t)nch * kMaxK : std::max(K, kMaxK);
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
int cluster_errors(hq_ctx* c, int P, int K, int64_t* err, float* worst, bool ignore_bad) {
    if (int rc = check_last_population(c, P, K)) return rc;
    const Geom& g = c->g;
    if (!c->res.err_ok() || c->d_pixerr.bytes < sizeof(float) * (size_t)P * (size_t)n_own(g))
        return fail(c, HQ_ERR_STATE, "option pixel_err was off at the last evaluation: no error image");
    if ((int64_t)g.W * g.H >= ((int64_t)1 << 32))
        return fail(c, HQ_ERR_UNSUPPORTED, "image of 2^32 pixels or more: a position does not fit 32 bits");
    if (int rc = bind(c)) return rc;
    const size_t n4 = (size_t)P * K * 4;
    HIP_TRY(c, c->d_worst.ensure(sizeof(float) * n4));
    std::vector<int64_t> h;
    std::vector<float> hw(n4);
    const char* bad = ignore_bad ? nullptr
                                 : "a pixel's dE is not a finite number below 2^20 (dE94's NaN, a non-finite "
                                   "colour or LabRef): no exact error sums";
    int rc = run_table_kernel(c, c->d_errstat, n4, kPErrsum, bad, h, [&] {
        int idx_bytes = 1;
        const ClusterErrArgs ea = cluster_err_args(c, P, K, c->res.nch, &idx_bytes);
        return launch_cluster_errors(ea, idx_bytes, c->num_cu, c->stream);
    }, hw.data(), &c->d_worst, sizeof(float) * n4);
    if (rc) return rc;
    for (size_t i = 0; i < n4; i += 4) {
        const uint64_t key = (uint64_t)h[i + 2];
        err[i] = h[i];
        err[i + 1] = h[i + 1];
        err[i + 2] = (int64_t)(key >> 32);
        err[i + 3] = key ? (int64_t)(0xffffffffu - (uint32_t)key) : -1;
    }
    std::memcpy(worst, hw.data(), sizeof(float) * n4);
    return HQ_OK;
}

// The k-means move on the last evaluation's index images: its exact sums, then the centroids
// into the palettes in place.  The repair move: its error statistics (ignore_bad: pixels
// with no usable dE left out), then the rule; moved (may be null): colours moved per palette.
// Fixed colours: the first nfixed colours of every palette come out of either move with the
// bits they went in with (the k-means move: their 16 bytes put back; the repair move: the rule).
int kmeans_move(hq_ctx* c, int P, int K, int nfixed, float* pal) {
    std::vector<int64_t> sums((size_t)P * K * 4);
    int64_t den = 0;
    int r = cluster_sums(c, P, K, sums.data(), &den);
    if (r) return r;
    std::vector<float> kept((size_t)P * 4 * nfixed);
    for (int p = 0; p < P && nfixed > 0; ++p)
        std::memcpy(&kept[(size_t)p * 4 * nfixed], pal + (size_t)p * 4 * K, sizeof(float) * 4 * nfixed);
    if ((r = hq_centroids_from_sums(sums.data(), den, P, K, pal))) return fail(c, r, "hq_centroids_from_sums failed");
    for (int p = 0; p < P && nfixed > 0; ++p)
        std::memcpy(pal + (size_t)p * 4 * K, &kept[(size_t)p * 4 * nfixed], sizeof(float) * 4 * nfixed);
    return r;
}
int repair_move(hq_ctx* c, int P, int K, int max_moves, int nfixed, bool ignore_bad, float* pal, int* moved) {
    std::vector<int64_t> err((size_t)P * K * 4);
    std::vector<float> worst(err.size());
    int r = cluster_errors(c, P, K, err.data(), worst.data(), ignore_bad);
    if (!r && (r = hq_reseed_unused_fixed(err.data(), worst.data(), P, K, max_moves, nfixed, pal, moved)))
        return fail(c, r, "hq_reseed_unused_fixed failed");
    return r;
}

// The planar form's sums need every owned pixel finite and in [0, 1]: a property
// of the image, established once per image by one launch of the sums kernel (one
// palette of one colour over the first index image -- any u8 index addresses the
// kernel's LDS table) and a read of its flag.
int planar_in_range(hq_ctx* c) {
    if (c->planar_ok < 0) {
        int rc = bind(c);
        if (rc) return rc;
        hipStream_t st = c->stream;
        HIP_TRY(c, c->d_idx.ensure((size_t)c->g.idx_pitch + 256));
        HIP_TRY(c, c->d_sums.ensure(sizeof(int64_t) * (4 + 1)));
        HIP_TRY(c, hipMemsetAsync(c->d_sums.p, 0, sizeof(int64_t) * (4 + 1), st));
        int idx_bytes = 1;
        ClusterArgs ca = cluster_args(c, 1, 1, 1, &idx_bytes);  // (the u8 image, d_idx)
        ca.mask = nullptr;    // (the flag looks at every owned pixel with or without a mask)
        ca.weighted = 0;
        HIP_TRY(c, launch_cluster_sums(ca, 1, c->num_cu, st));
        int bad = 1;
        HIP_TRY(c, hipMemcpyAsync(&bad, ca.bad, sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        c->planar_ok = bad == 0;
    }
    return HQ_OK;
}

int require_unit_range_image(hq_ctx* c, const char* subject, const char* what) {
    if (int rc = planar_in_range(c)) return rc;
    if (!c->planar_ok)
        return fail(c, HQ_ERR_UNSUPPORTED, "%s with a pixel outside [0, 1] or not finite: %s", subject, what);
    return HQ_OK;
}

int check_ordered_amp(hq_ctx* c, const float* amp) {
    if (!amp) return fail(c, HQ_ERR_ARG, "null amp");
    for (int ch = 0; ch < 3; ++ch)
        if (!(amp[ch] >= 0.0f && amp[ch] <= 1.0f))
            return fail(c, HQ_ERR_ARG, "amp[%d] = %g not in [0, 1]", ch, amp[ch]);
    return HQ_OK;
}

// Ordered dithering lives in assign's 8-bit instances, every palette's index image on this
// device, and its clamp stands for `inside` only when the pixels themselves are in [0, 1]
// (the range flag, established once per image; the packed copy exists only for k/255 images).
int ordered_scope(hq_ctx* c, int K) {
    if (K > kMaxK)
        return fail(c, HQ_ERR_UNSUPPORTED, "K=%d > %d: ordered dithering is built into the 8-bit argmin only", K, kMaxK);
    if (c->psplit || c->slice_ranks > 1) return fail(c, HQ_ERR_UNSUPPORTED, "ordered dithering on a palette slice");
    return c->have_image && !c->img_u8 ? require_unit_range_image(c, "image", "no ordered dithering") : HQ_OK;
}

// The context's map on the device: the buffer once, its contents when the host map changed.
// (Nothing of this context is in flight: every entry point synchronises its stream.)
int ensure_dither_map(hq_ctx* c) {
    if (int rc = bind(c)) return rc;
    HIP_TRY(c, c->d_dmap.ensure(sizeof(float) * kMaxMapSide * kMaxMapSide));
    if (!c->dmap_dirty) return HQ_OK;
    std::vector<float> def;
    if (c->dmap.empty()) {
        def.resize(16 * 16);
        hq_bayer_map(4, def.data());
    }
    const std::vector<float>& m = c->dmap.empty() ? def : c->dmap;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(c->d_dmap.p, m.data(), sizeof(float) * m.size(), hipMemcpyHostToDevice));
    c->dmap_dirty = false;
    return HQ_OK;
}

}  // namespace hq

namespace {

// ---- the rendered entry points ----------------------------------------------------------------
// A rendered call as its checks see it: the population, the output (costs, or a _partial call's
// [P][1 + K] rows), and its family with that family's parameter: the amplitudes per channel
// (ordered), else the strength.
struct RenderCall {
    const float* palettes;
    const void* out;
    int P, K;
    bool partial, ordered;
    const float* amp;
    float strength;
};

// Every check of a rendered evaluation on the call and the context; a refused call has touched
// nothing.  scope(): where the call may run (the diffused family's whole_image_only or dot_window,
// the ordered family's shard without _partial).  Both families open with the arguments, the
// parameter and the image.  After that each keeps its own order, because the order decides which
// refusal wins when two conditions hold (tests/golden/render_contract.json): under a mask on a palette
// slice the diffused family names the slice and the ordered family the mask.
template <typename Scope>
int check_rendered(hq_ctx* c, const RenderCall& r, Scope&& scope) {
    if (!r.palettes || !r.out || r.P < 1 || r.K < 1)
        return fail(c, HQ_ERR_ARG, "bad palettes / %s / P=%d / K=%d", r.ordered ? "output" : r.partial ? "partial" : "costs",
                    r.P, r.K);
    int rc = HQ_OK;
    if (r.ordered && (rc = check_ordered_amp(c, r.amp))) return rc;
    if (!r.ordered && !(r.strength >= 0.0f && r.strength <= 1.0f))
        return fail(c, HQ_ERR_ARG, "strength %g not in [0, 1]", r.strength);
    if (!c->have_image) return fail(c, HQ_ERR_STATE, "no image set (hq_set_image)");
    if (int rc0 = assign_space_excludes(c, r.ordered ? "ordered dithering" : "error diffusion")) return rc0;
    auto palette_range = [&] {
        if (population_in_range(r.palettes, r.P, r.K)) return (int)HQ_OK;
        return fail(c, HQ_ERR_ARG, "palette with a channel that is not finite or outside [0, 1]");
    };
    if (r.ordered) {  // mask, palette range, scope, then ordered_scope's K, palette slice and image range
        if ((rc = mask_scope(c)) || (r.K <= kMaxK && (rc = palette_range())) || (rc = scope())) return rc;
        return ordered_scope(c, r.K);
    }
    // the diffused family: scope, mask, K, palette range, image range
    if ((rc = scope()) || (rc = mask_scope(c))) return rc;
    if (r.K > kMaxK)
        return fail(c, HQ_ERR_UNSUPPORTED, "K=%d > %d: the dither kernel keeps the palette in LDS and writes "
                                           "8-bit indices", r.K, kMaxK);
    if ((rc = palette_range())) return rc;
    // the errors stay bounded (|e| <= 1) for pixels in [0, 1]: a property of the image, established
    // once per image as the hybrid search's is (the packed 8-bit copy exists only for k/255 images)
    if (!c->img_u8 && (rc = require_unit_range_image(c, "image", "no error diffusion"))) return rc;
    // ... and of the rows a shard renders beyond its owned ones (found on the host with the apron)
    if (r.partial && !c->apron_ok)
        return fail(c, HQ_ERR_UNSUPPORTED, "image with a pixel outside [0, 1] or not finite in the rows held around "
                                           "the owned ones: no error diffusion");
    return HQ_OK;
}

// hq_ordered_population[_partial] into h_out (the getters then answer for the ordered rendering).
int ordered_into_hout(hq_ctx* c, const RenderCall& r) {
    if (!c) return HQ_ERR_ARG;
    int rc = check_rendered(c, r, [&] {
        if (r.partial || whole_image(c) || (c->comm && c->nranks > 1)) return (int)HQ_OK;
        return fail(c, HQ_ERR_STATE, "sharded context without a communicator: use hq_ordered_population_partial");
    });
    if (rc || (rc = ensure_dither_map(c))) return rc;
    return run_pass(c, r.palettes, r.P, r.K, Pass{Pass::Full, Ordered{{r.amp[0], r.amp[1], r.amp[2]}}});
}

// The tables of class matrix m on the device: the buffer once, its contents when m differs from
// the matrix of the last call (c->dot_cls; compared over n and its n^2 entries).
// (Nothing of this context is in flight: every entry point synchronises its stream.)
int ensure_dot_tables(hq_ctx* c, const hq_dot_classes& m) {
    if (int rc = bind(c)) return rc;
    const bool had = c->d_dottab.p != nullptr;
    HIP_TRY(c, c->d_dottab.ensure(sizeof(uint32_t) * 2 * kDotCells));
    HIP_TRY(c, c->d_dotsched.ensure(sizeof(uint32_t) * kDotSchedWords));
    if (had && c->dot_cls.n == m.n && !std::memcmp(c->dot_cls.cls, m.cls, sizeof(int32_t) * m.n * m.n)) return HQ_OK;
    uint32_t tab[2 * kDotCells];
    dot_tables(m, tab, tab + kDotCells);
    c->dot_cls.n = 0;  // (no matrix while the copy may fail)
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(c->d_dottab.p, tab, sizeof tab, hipMemcpyHostToDevice));
    DotMatrixInfo info;
    if (!dot_matrix_info(m, &info)) return fail(c, HQ_ERR_ARG, "illegal class matrix");
    DotSchedule sched;  // (the tiled form's: cell, then start)
    dot_schedule(m, &sched);
    HIP_TRY(c, hipMemcpy(c->d_dotsched.p, sched.cell, sizeof(uint32_t) * kDotSchedWords, hipMemcpyHostToDevice));
    std::memset(&c->dot_cls, 0, sizeof c->dot_cls);
    c->dot_cls.n = m.n;
    std::memcpy(c->dot_cls.cls, m.cls, sizeof(int32_t) * m.n * m.n);
    c->dot_info = info;
    return HQ_OK;
}

// hq_dot_population_partial's scope and window.  A palette slice and a communicator of more than
// one rank are refused as hq_dot_population refuses them; a row-block shard is served when the
// apron it holds covers, on each side, the reach of matrix m or all the rows up to the image's
// border.  [*a0, *a1): the rows to render -- the extended rows and the apron rows needed (a whole
// image: all its rows, the whole-image launches).
int dot_window(hq_ctx* c, const hq_dot_classes& m, int* a0, int* a1) {
    const char* const what = "hq_dot_population_partial";
    if (c->comm && c->nranks > 1)
        return fail(c, HQ_ERR_UNSUPPORTED, "%s with a communicator of %d ranks: add the ranks' partials yourself", what,
                    c->nranks);
    if (c->psplit || c->slice_ranks > 1) return fail(c, HQ_ERR_UNSUPPORTED, "%s on a palette slice", what);
    const Geom& g = c->g;
    *a0 = g.e0, *a1 = g.e1;
    if (whole_image(c)) return HQ_OK;
    int above = 0, below = 0;
    if (hq_dot_reach(&m, &above, &below)) return fail(c, HQ_ERR_ARG, "illegal class matrix");
    const int need_a = std::min(above, g.e0), need_b = std::min(below, g.H - g.e1);
    if (c->apron_above < need_a || c->apron_below < need_b)
        return fail(c, HQ_ERR_STATE, "%s on rows [%d, %d) of %d: the class matrix reaches %d rows above and %d below, "
                                     "so %d and %d rows are needed beyond the extended rows [%d, %d) and %d and %d are "
                                     "held (option dot_apron before hq_set_image_shard)",
                    what, g.r0, g.r1, g.H, above, below, need_a, need_b, g.e0, g.e1, c->apron_above, c->apron_below);
    *a0 = g.e0 - need_a, *a1 = g.e1 + need_b;
    return HQ_OK;
}

// hq_dot_population[_partial] into h_out: the class matrix (the caller's when legal, Knuth's for none), the
// checks -- a _partial call may be a row-block shard's, over the window dot_window finds -- and the pass.
int dot_into_hout(hq_ctx* c, const RenderCall& r, const hq_dot_classes* cls) {
    if (cls && !hq_dot_classes_legal(cls))
        return fail(c, HQ_ERR_ARG, "illegal class matrix: side 4, 8 or 16 and a permutation of 0 .. n*n - 1 (hq.h)");
    hq_dot_classes m;
    if (cls) m = *cls;
    else hq_dot_preset(HQ_DOT_KNUTH8, &m);
    int a0 = 0, a1 = 0;
    int rc = check_rendered(c, r, [&] {
        return r.partial ? dot_window(c, m, &a0, &a1) : whole_image_only(c, "hq_dither_population (error diffusion)");
    });
    if (rc) return rc;
    if (r.P > kDotMaxP)
        return fail(c, HQ_ERR_UNSUPPORTED, "P=%d > %d: a dot-diffusion launch holds the palettes in its grid's y", r.P,
                    kDotMaxP);
    if ((rc = ensure_dot_tables(c, m))) return rc;
    return run_pass(c, r.palettes, r.P, r.K, Pass{Dot{r.strength, a0, a1}});  // (the getters then answer for it)
}

}  // namespace

namespace hq {

int dot_search_scope(hq_ctx* c, int K) {
    if (int rc = whole_image_only(c, "hq_dither_population (error diffusion)")) return rc;
    if (K > kMaxK)
        return fail(c, HQ_ERR_UNSUPPORTED, "K=%d > %d: the dither kernel keeps the palette in LDS and writes "
                                           "8-bit indices", K, kMaxK);
    return c->have_image && !c->img_u8 ? require_unit_range_image(c, "image", "no error diffusion") : HQ_OK;
}

int ensure_dot_pass(hq_ctx* c, const hq_dot_classes& m, int P, int K) {
    if (int rc = ensure_dot_tables(c, m)) return rc;
    return ensure_render_scratch(c, Pass{Dot{0.f, 0, 0}}, P, K);
}

}  // namespace hq

extern "C" {

int hq_set_dither_map(hq_ctx* c, const float* map, int mw, int mh) {
    if (!c) return HQ_ERR_ARG;
    if (map) {
        auto side = [](int v) { return v >= 1 && v <= kMaxMapSide && (v & (v - 1)) == 0; };
        if (!side(mw) || !side(mh))
            return fail(c, HQ_ERR_ARG, "map of %d x %d: each side a power of two in 1 .. %d", mw, mh, kMaxMapSide);
        for (int i = 0; i < mw * mh; ++i)
            if (!(map[i] >= -0.5f && map[i] <= 0.5f))
                return fail(c, HQ_ERR_ARG, "map[%d] = %g not in [-0.5, 0.5]", i, map[i]);
        c->dmap.assign(map, map + (size_t)mw * mh);
        c->dmap_w = mw;
        c->dmap_h = mh;
    } else {
        c->dmap.clear();
        c->dmap_w = c->dmap_h = 0;
    }
    c->dmap_dirty = true;  // (uploaded by the next ordered evaluation or search run: ensure_dither_map)
    return HQ_OK;
}

int hq_ordered_population(hq_ctx* c, const float* palettes, int P, int K, const float amp[3], float delta,
                          double* costs, int32_t* used) {
    const int rc = ordered_into_hout(c, RenderCall{palettes, costs, P, K, false, true, amp, 0.f});
    return rc ? rc : costs_from_hout(c, P, K, delta, costs, used);
}

int hq_ordered_population_partial(hq_ctx* c, const float* palettes, int P, int K, const float amp[3],
                                  double* partial) {
    const int rc = ordered_into_hout(c, RenderCall{palettes, partial, P, K, true, true, amp, 0.f});
    return rc ? rc : partial_from_hout(c, P, K, partial);
}

int hq_eval_population_partial(hq_ctx* c, const float* palettes, int P, int K, double* partial) {
    if (!partial) return fail(c, HQ_ERR_ARG, "null output");
    const int rc = eval_partial_into_hout(c, palettes, P, K);
    return rc ? rc : partial_from_hout(c, P, K, partial);
}

int hq_eval_population(hq_ctx* c, const float* palettes, int P, int K, float delta,
                       double* costs, int32_t* used) {
    if (!costs) return fail(c, HQ_ERR_ARG, "null output");
    int rc = eval_partial_into_hout(c, palettes, P, K);
    if (rc) return rc;
    if ((!whole_image(c) || c->slice_ranks > 1) && !(c->comm && c->nranks > 1))
        return fail(c, HQ_ERR_STATE, "sharded context or palette slice without a communicator: use "
                                     "hq_eval_population_partial");
    costs_from_hout(c, P, K, delta, costs, used);
    return HQ_OK;
}

// (the Floyd-Steinberg preset; its taps, whoever gives them, take the kernel's own formula: hq.h)
int hq_dither_population(hq_ctx* c, const float* palettes, int P, int K, float strength, float delta,
                         double* costs, int32_t* used) {
    hq_diffusion_taps fs;
    hq_diffusion_preset(HQ_DIFFUSION_FLOYD_STEINBERG, &fs);
    return hq_diffuse_population(c, palettes, P, K, &fs, strength, delta, costs, used);
}

int hq_diffuse_population(hq_ctx* c, const float* palettes, int P, int K, const hq_diffusion_taps* taps,
                          float strength, float delta, double* costs, int32_t* used) {
    if (!c) return HQ_ERR_ARG;
    if (!hq_diffusion_taps_legal(taps)) return fail(c, HQ_ERR_ARG, "null or illegal diffusion taps (hq.h)");
    int rc = check_rendered(c, RenderCall{palettes, costs, P, K, false, false, nullptr, strength},
                            [&] { return whole_image_only(c, "hq_dither_population (error diffusion)"); });
    if (rc) return rc;
    Diffused d{strength, *taps, 0, 0, false};
    if (hq_diffusion_classify(taps, &d.rows, &d.slope)) return fail(c, HQ_ERR_ARG, "illegal diffusion taps");
    hq_diffusion_taps fs;
    hq_diffusion_preset(HQ_DIFFUSION_FLOYD_STEINBERG, &fs);
    d.floyd_steinberg = !std::memcmp(&fs, taps, sizeof fs);
    rc = run_pass(c, palettes, P, K, Pass{d});  // (the getters then answer for the rendering)
    return rc ? rc : costs_from_hout(c, P, K, delta, costs, used);
}

int hq_dot_population(hq_ctx* c, const float* palettes, int P, int K, const hq_dot_classes* cls, float strength,
                      float delta, double* costs, int32_t* used) {
    if (!c) return HQ_ERR_ARG;
    const int rc = dot_into_hout(c, RenderCall{palettes, costs, P, K, false, false, nullptr, strength}, cls);
    return rc ? rc : costs_from_hout(c, P, K, delta, costs, used);
}

int hq_dot_form(hq_ctx* c, int* form, int* tile_w, int* tile_h, int* levels) {
    if (!c) return HQ_ERR_ARG;
    if (form) *form = c->dot_form;
    if (tile_w) *tile_w = c->dot_form_tw;
    if (tile_h) *tile_h = c->dot_form_th;
    if (levels) *levels = c->dot_form_levels;
    return HQ_OK;
}

int hq_dot_population_partial(hq_ctx* c, const float* palettes, int P, int K, const hq_dot_classes* cls,
                              float strength, double* partial) {
    if (!c) return HQ_ERR_ARG;
    if (!partial) return fail(c, HQ_ERR_ARG, "null output");
    const int rc = dot_into_hout(c, RenderCall{palettes, partial, P, K, true, false, nullptr, strength}, cls);
    return rc ? rc : partial_from_hout(c, P, K, partial);
}

int hq_get_indices(hq_ctx* c, int p, uint8_t* idx) {
    if (!c || !idx) return HQ_ERR_ARG;
    int rc = check_local_palette(c, p, &p);
    if (rc) return rc;
    if (c->res.K > kMaxK)
        return fail(c, HQ_ERR_STATE, "K=%d > 256: indices are 32-bit (hq_get_indices32)", c->res.K);
    if ((rc = bind(c))) return rc;
    const Geom& g = c->g;
    HIP_TRY(c, hipMemcpy(idx, c->d_idx.as<uint8_t>() + (int64_t)p * g.idx_pitch + own_first(g), n_own(g),
                         hipMemcpyDeviceToHost));
    return HQ_OK;
}

int hq_get_indices32(hq_ctx* c, int p, uint32_t* idx) {
    if (!c || !idx) return HQ_ERR_ARG;
    int rc = check_local_palette(c, p, &p);
    if (rc) return rc;
    if ((rc = bind(c))) return rc;
    const Geom& g = c->g;
    const int64_t n = n_own(g);
    // the image at its own width (u16: chunked palettes; u32: K > 16384), widened here
    int idx_bytes = 1;
    const char* base = static_cast<const char*>(index_images(c, c->res.K, c->res.nch, &idx_bytes));
    std::vector<unsigned char> raw((size_t)n * idx_bytes);
    HIP_TRY(c, hipMemcpy(raw.data(), base + ((int64_t)p * g.idx_pitch + own_first(g)) * idx_bytes, raw.size(),
                         hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < n; ++i) {
        uint32_t v = 0;
        std::memcpy(&v, raw.data() + i * idx_bytes, idx_bytes);  // (little-endian host)
        idx[i] = v;
    }
    return HQ_OK;
}

int hq_get_pixel_errors(hq_ctx* c, int p, float* err) {
    if (!c || !err) return HQ_ERR_ARG;
    if (!c->pixel_err) return fail(c, HQ_ERR_STATE, "option pixel_err is off");
    int rc = check_local_palette(c, p, &p);
    if (rc) return rc;
    if (!c->res.pixerr_ok())
        return fail(c, HQ_ERR_STATE, "no error image of the last evaluation: pixel_err was set after it, or a search "
                                     "has run since");
    if ((rc = bind(c))) return rc;
    const int64_t n = n_own(c->g);
    HIP_TRY(c, hipMemcpy(err, c->d_pixerr.as<float>() + (int64_t)p * n, sizeof(float) * n, hipMemcpyDeviceToHost));
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

int hq_cluster_errors(hq_ctx* c, int P, int K, int64_t* err, float* worst_rgb) {
    if (!c) return HQ_ERR_ARG;
    if (!err || !worst_rgb || P < 1 || K < 1) return fail(c, HQ_ERR_ARG, "bad err / worst_rgb / P=%d / K=%d", P, K);
    if (c->mask_on) return fail(c, HQ_ERR_UNSUPPORTED, "hq_cluster_errors under %s (%s)", mask_noun(c), mask_call(c));
    return cluster_errors(c, P, K, err, worst_rgb, false);
}

int hq_refine_population(hq_ctx* c, float* palettes, int P, int K, int steps, float delta, int keep_best,
                         double* costs, int32_t* used, double* trace) {
    int rc = check_improve_args(c, palettes, P, K, steps, costs, "hq_refine_population",
                                ": add the shards' hq_cluster_sums yourself");
    if (rc) return rc;
    if (steps > 0 && (rc = weighted_sums_scope(c, "hq_refine_population"))) return rc;
    return improve_population(c, palettes, P, K, steps, delta, keep_best, costs, used, trace,
                              [&](float* cur, bool*) { return kmeans_move(c, P, K, c->fixed_n, cur); });
}

int hq_repair_population(hq_ctx* c, float* palettes, int P, int K, int steps, float delta, int max_moves,
                         int keep_best, double* costs, int32_t* used, double* trace) {
    int rc = check_improve_args(c, palettes, P, K, steps, costs, "hq_repair_population",
                                ": merge the shards' hq_cluster_errors yourself");
    if (rc) return rc;
    if (c->mask_on)
        return fail(c, HQ_ERR_UNSUPPORTED, "hq_repair_population under %s (%s)", mask_noun(c), mask_call(c));
    const PixelErrScope scope(c);  // the evaluations below store their error images
    std::vector<int> moved(P);
    return improve_population(c, palettes, P, K, steps, delta, keep_best, costs, used, trace,
                              [&](float* cur, bool* changed) {
        const int r = repair_move(c, P, K, max_moves, c->fixed_n, false, cur, moved.data());
        // nothing left to repair: the remaining steps repeat this one
        *changed = !std::all_of(moved.begin(), moved.end(), [](int m) { return m == 0; });
        return r;
    });
}

}  // extern "C"
