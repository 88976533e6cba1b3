// hq_runtime.hip -- libhq host runtime: the C ABI of include/hq.h.
//
// One hq_ctx = one GPU, one HIP stream (the reference's single in-order queue,
// IM:58-59), the device-resident image of IM:450-478 (planar RGB of the owned
// rows +- halo, planar LabRef of the owned rows), per-population work buffers,
// and optionally an RCCL communicator for row-block sharding.
//
// This file: the context (create, destroy, filters, image, options, profiling, the
// communicator) and the stand-alone utilities.  Evaluation: hq_eval.hip; the
// search: hq_search_run.hip; what they share: hq_runtime.h.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <mutex>
#include <unordered_map>

#include "hq_runtime.h"

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

int bind(hq_ctx* c) {
    HIP_TRY(c, hipSetDevice(c->device));
    return HQ_OK;
}

int whole_image_only(hq_ctx* c, const char* what, const char* comm_hint, bool psplit_alone) {
    if (c->have_image && !whole_image(c))
        return fail(c, HQ_ERR_STATE, "sharded context: the whole image is needed for %s", what);
    if (c->comm && c->nranks > 1)
        return fail(c, HQ_ERR_UNSUPPORTED, "%s with a communicator of %d ranks%s", what, c->nranks, comm_hint);
    if ((psplit_alone && c->psplit) || c->slice_ranks > 1)
        return fail(c, HQ_ERR_UNSUPPORTED, "%s on a palette slice", what);
    return HQ_OK;
}

// A pixel mask measures the whole population on every device that holds pixels: a palette
// slice (its rows of d_out, its counters) under one is left out.
int mask_scope(hq_ctx* c) {
    if (c->mask_on && (c->psplit || c->slice_ranks > 1))
        return fail(c, HQ_ERR_UNSUPPORTED, "a palette slice (option palette_split or slice_ranks) under %s", mask_noun(c));
    return HQ_OK;
}

int weighted_sums_scope(hq_ctx* c, const char* what) {
    if (c->mask_on && c->weights_on && !sums_u8(c) && c->mask_w_own >= kWeightSumLimit)
        return fail(c, HQ_ERR_UNSUPPORTED, "%s: the owned rows' weights sum to %lld >= 2^31, and the planar form's "
                                           "sums (units of 2^-32) could pass 2^63", what, (long long)c->mask_w_own);
    return HQ_OK;
}

ProfRec prof_begin(hq_ctx* c) { return ProfRec{c->prof ? c->ev.ev.data() : nullptr, 0}; }

void prof_accumulate(hq_ctx* c, const ProfRec& pr) {
    for (int p = 0; pr.ev && p < kPairs; ++p) {
        if (!(pr.recorded >> p & 1)) continue;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, pr.ev[2 * p], pr.ev[2 * p + 1]) == hipSuccess) {
            c->prof_stage[kPairStage[p]].ms += ms;
            c->prof_stage[kPairStage[p]].launches += 1;
        } else {
            (void)hipGetLastError();  // a pair without its events (none could be made): not a launch error
        }
    }
}

}  // namespace hq

using namespace hq;

namespace {

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

// Upload one plane of the extended rows from a full-image host source with
// stride `sstride` floats between pixels and channel offset `ch`.
void gather_rows(const float* src, int sstride, int ch, const Geom& g, std::vector<float>& dst) {
    dst.assign((size_t)round_up(g.n_ext, 4), 0.0f);
    const int64_t base = (int64_t)g.e0 * g.W;
    for (int64_t i = 0; i < g.n_ext; ++i) dst[i] = src[(base + i) * sstride + ch];
}

// IM:319-346, the S-CIELAB spatial filtering of geometry g's extended rows: the
// opponent planes make_opp(float4*) writes (g.n_ext pixels) into the filtered
// planes of the owned rows in t.conv, filter by filter, H then V (update for
// filters 2 and 3).  k3 and |k3| are staged as float4 taps here.  The caller keeps
// `t` until it has synchronised the stream: the copies and kernels read it.
struct ScielabTmp {
    DevBuf opp, tmp, conv, k3v, ak3v;
    std::vector<float> k3h, ak3h;
};
template <typename MakeOpp>
int scielab_filter(hq_ctx* c, const Geom& g, ScielabTmp& t, MakeOpp&& make_opp) {
    HIP_TRY(c, t.opp.ensure(sizeof(float4) * g.n_ext));
    HIP_TRY(c, t.tmp.ensure(sizeof(float4) * g.n_ext));
    HIP_TRY(c, t.conv.ensure(sizeof(float4) * std::max<int64_t>(n_own(g), 1)));
    t.k3h.assign(4 * c->taps, 0.f);
    t.ak3h.assign(4 * c->taps, 0.f);
    for (int i = 0; i < c->taps; ++i) { t.k3h[4 * i] = c->k3[i]; t.ak3h[4 * i] = c->absk3[i]; }
    const size_t kb = sizeof(float) * t.k3h.size();
    HIP_TRY(c, t.k3v.ensure(kb));
    HIP_TRY(c, t.ak3v.ensure(kb));
    HIP_TRY(c, hipMemcpyAsync(t.k3v.p, t.k3h.data(), kb, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(t.ak3v.p, t.ak3h.data(), kb, hipMemcpyHostToDevice, c->stream));
    if (int rc = make_opp(t.opp.as<float4>())) return rc;
    const float* hk[3] = {c->d_k1.as<float>(), c->d_k2.as<float>(), t.k3v.as<float>()};
    const float* vk[3] = {c->d_k1.as<float>(), c->d_k2.as<float>(), t.ak3v.as<float>()};
    for (int f = 0; f < 3; ++f) {
        const int chans = f < 2 ? 3 : 1;
        HIP_TRY(c, launch_labref_hconv(t.opp.as<float4>(), t.tmp.as<float4>(), hk[f], c->half, chans,
                                       g.W, g.n_ext, c->stream));
        HIP_TRY(c, launch_labref_vconv(t.tmp.as<float4>(), t.conv.as<float4>(), vk[f], c->half, chans,
                                       f > 0, g, c->stream));
    }
    return HQ_OK;
}

int compute_labref_device(hq_ctx* c) {
    // IM:100 RGBtoXYZ + IM:285-370 XYZtoScielab on the extended rows.
    const Geom& g = c->g;
    ScielabTmp t;
    int rc = scielab_filter(c, g, t, [&](float4* opp) {
        HIP_TRY(c, launch_labref_opp(c->d_R.as<float>(), c->d_G.as<float>(), c->d_B.as<float>(), opp, g.n_ext,
                                     c->stream));
        return (int)HQ_OK;
    });
    if (rc) return rc;
    HIP_TRY(c, launch_labref_lab(t.conv.as<float4>(), c->d_labL.as<float>(), c->d_labA.as<float>(),
                                 c->d_labB.as<float>(), nullptr, g.W, n_own(g), g.lab_pitch, c->illum,
                                 c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return HQ_OK;
}

// A new image on the context, in three steps: begin_image (the geometry c->g is the new image's
// already), the planes filled on the context's stream -- uploaded from the host
// (set_image_common) or reduced from another context's image on the device
// (hq_set_image_reduced) -- and finish_image, the same tail for both.
//
// begin_image: what belonged to the old image goes, and the planes have the new one's size.
int begin_image(hq_ctx* c) {
    const Geom& g = c->g;
    // c->g is the new image's already: nothing evaluated on the old one may be read at it
    c->have_image = false;  // (until every plane is in place: finish_image)
    drop(c);
    c->mask_on = c->weights_on = false;  // a mask, or a weight map, belongs to an image
    c->live_dirty = true;
    c->d_apron.release();  // ... and so does a shard's apron (set_apron brings the new image's)
    c->apron_above = c->apron_below = 0;
    c->apron_ok = true;
    c->coords_ok = false;  // option "assign_space": the coordinates were the old image's and illuminant's
    const size_t plane = sizeof(float) * (size_t)round_up(g.n_ext, 4);
    HIP_TRY(c, c->d_R.ensure(plane));
    HIP_TRY(c, c->d_G.ensure(plane));
    HIP_TRY(c, c->d_B.ensure(plane));
    return HQ_OK;
}

// finish_image: the planes are in place (enqueued on c->stream).  The packed-form check, the
// illuminant, LabRef -- the caller's (lab4_full, the full image's) or computed on the device
// under the context's filters -- and the flags.
int finish_image(hq_ctx* c, const float* lab4_full, const float* illum) {
    const Geom& g = c->g;
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
        c->img_u8 = not_u8 == 0;
        if (!c->img_u8) c->d_rgbx.release();  // (no packed copy: its memory back now)
    }
    if (illum) std::memcpy(c->illum, illum, sizeof c->illum);
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
        const int64_t n = n_own(g);
        DevBuf tmp;
        HIP_TRY(c, tmp.ensure(sizeof(float4) * n));
        HIP_TRY(c, hipMemcpyAsync(tmp.p, lab4_full + (int64_t)g.r0 * g.W * 4, sizeof(float4) * n,
                                  hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, launch_lab_to_planar(tmp.as<float4>(), c->d_labL.as<float>(), c->d_labA.as<float>(),
                                        c->d_labB.as<float>(), g.W, n, g.lab_pitch, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    } else {
        int rc = compute_labref_device(c);
        if (rc) return rc;
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->have_image = true;
    return HQ_OK;
}

int set_image_common(hq_ctx* c, const std::vector<float>& R, const std::vector<float>& G,
                     const std::vector<float>& B, const float* lab4_full, const float* illum) {
    if (int rc = begin_image(c)) return rc;
    const size_t plane = sizeof(float) * (size_t)round_up(c->g.n_ext, 4);
    HIP_TRY(c, hipMemcpyAsync(c->d_R.p, R.data(), plane, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->d_G.p, G.data(), plane, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->d_B.p, B.data(), plane, hipMemcpyHostToDevice, c->stream));
    return finish_image(c, lab4_full, illum);
}

// The apron of the shard just set (option "dot_apron", hq.h): the rows [max(0, e0 - A), e0) and
// [e1, min(H, e1 + A)) of the full-image host source -- plane ch at src[ch] with `sstride` floats
// between pixels -- into storage of their own, and whether they are all in [0, 1].  A whole image
// or A = 0 holds none and allocates nothing.  Failing leaves the context without an image.
int set_apron(hq_ctx* c, const float* const src[3], int sstride) {
    const Geom& g = c->g;
    const int A = whole_image(c) ? 0 : c->dot_apron;
    const int a0 = std::max(0, g.e0 - A), a1 = std::min(g.H, g.e1 + A);
    const int above = g.e0 - a0, below = a1 - g.e1;
    if (above + below == 0) return HQ_OK;
    const size_t plane = (size_t)(above + below) * g.W;
    std::vector<float> rows(3 * plane);
    bool ok = true;
    for (int ch = 0; ch < 3; ++ch) {
        for (int r = 0; r < above + below; ++r) {
            const int64_t y = r < above ? a0 + r : g.e1 + (r - above);
            for (int x = 0; x < g.W; ++x) {
                const float v = src[ch][(y * g.W + x) * sstride];
                ok = ok && v >= 0.0f && v <= 1.0f;  // (a NaN fails both)
                rows[ch * plane + (size_t)r * g.W + x] = v;
            }
        }
        // (the extended rows outside the owned ones are rendered with them, and the device's flag
        // looks at the owned rows alone)
        for (int64_t y = g.e0; y < g.e1; ++y) {
            if (y >= g.r0 && y < g.r1) continue;
            for (int x = 0; x < g.W; ++x) {
                const float v = src[ch][(y * g.W + x) * sstride];
                ok = ok && v >= 0.0f && v <= 1.0f;
            }
        }
    }
    c->have_image = false;
    HIP_TRY(c, c->d_apron.upload(rows.data(), sizeof(float) * rows.size()));
    c->apron_above = above, c->apron_below = below;
    c->apron_ok = ok;
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

// An illuminant a caller gave (NULL: none given, the context's stays): every component finite
// and greater than 0, or 1.0f / illum is infinite or NaN and every cost with it.  Checked with
// the other arguments, before anything of the context changes.
int check_illum_arg(hq_ctx* c, const float* illum) {
    const int i = illum ? bad_illum_component(illum) : -1;
    if (i < 0) return HQ_OK;
    return fail(c, HQ_ERR_ARG, "illum[%d] (%cn) is %g: every component of the illuminant must be finite and "
                               "greater than 0", i, "XYZ"[i], (double)illum[i]);
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
    for (int ng = 1; ng <= 4; ++ng) c->assign_res_ord[ng] = assign_residency_ordered(ng);
    (void)c->ev.ensure(2 * kPairs);
    *out = c;
    return HQ_OK;
}

// The order the code below does not show as a condition: the context's device
// current, its stream drained (nothing in flight reads a buffer or records an
// event), the communicator destroyed (it holds the stream) -- and only then may the
// members let go of their memory and events (delete), and the stream go last.
void hq_destroy(hq_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->comm) (void)ncclCommDestroy(c->comm);
    const hipStream_t stream = c->stream;
    delete c;
    if (stream) (void)hipStreamDestroy(stream);
}

const char* hq_last_error(const hq_ctx* c) { return c ? c->err.c_str() : "null context"; }

int hq_set_filters(hq_ctx* c, int taps, const float* k1, const float* k2, const float* k3,
                   const float* absk3) {
    if (!c) return HQ_ERR_ARG;
    if (taps < 1 || taps > kMaxTaps || !k1 || !k2 || !k3 || !absk3)
        return fail(c, HQ_ERR_ARG, "bad filters (taps=%d)", taps);
    int rc = bind(c);
    if (rc) return rc;
    // the halo depends on the filters: the image, and what was evaluated on it, go with them
    // (before the first early return below, which leaves the new half-width behind)
    c->have_image = false;
    drop(c);
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
    return HQ_OK;
}

int hq_set_image_shard(hq_ctx* c, const float* rgba4, const float* lab4, int w, int h,
                       const float* illum, int row_begin, int row_end) {
    if (!c) return HQ_ERR_ARG;
    if (!rgba4) return fail(c, HQ_ERR_ARG, "null image");
    int rc = check_geom_args(c, w, h, row_begin, row_end);
    if (rc) return rc;
    if ((rc = check_illum_arg(c, illum))) return rc;
    if ((rc = bind(c))) return rc;
    c->g = make_geom(w, h, row_begin, row_end, c->half);
    std::vector<float> R, G, B;
    gather_rows(rgba4, 4, 0, c->g, R);
    gather_rows(rgba4, 4, 1, c->g, G);
    gather_rows(rgba4, 4, 2, c->g, B);
    if ((rc = set_image_common(c, R, G, B, lab4, illum))) return rc;
    const float* const planes[3] = {rgba4, rgba4 + 1, rgba4 + 2};
    return set_apron(c, planes, 4);
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
    if ((rc = check_illum_arg(c, illum))) return rc;
    if ((rc = bind(c))) return rc;
    c->g = make_geom(w, h, row_begin, row_end, c->half);
    std::vector<float> r, g, b;
    gather_rows(R, 1, 0, c->g, r);
    gather_rows(G, 1, 0, c->g, g);
    gather_rows(B, 1, 0, c->g, b);
    if ((rc = set_image_common(c, r, g, b, nullptr, illum))) return rc;
    const float* const planes[3] = {R, G, B};
    return set_apron(c, planes, 1);
}

// The box reduction of src's image as dst's whole image: the second way into finish_image.
// Every refusal comes before dst is touched.  The kernel runs on dst's stream and reads src's
// buffers; both contexts are idle here, since every entry point synchronises its stream.
int hq_set_image_reduced(hq_ctx* dst, hq_ctx* src, int factor, const float* illum) {
    if (!dst) return HQ_ERR_ARG;
    if (!src || src == dst) return fail(dst, HQ_ERR_ARG, "hq_set_image_reduced: a null source, or the source itself");
    if (src->device != dst->device)
        return fail(dst, HQ_ERR_UNSUPPORTED, "hq_set_image_reduced: source on device %d, destination on device %d",
                    src->device, dst->device);
    if (!src->have_image) return fail(dst, HQ_ERR_STATE, "hq_set_image_reduced: no image set on the source");
    if (!whole_image(src))
        return fail(dst, HQ_ERR_STATE, "hq_set_image_reduced: the source is a row-block shard (rows [%d, %d) of %d)",
                    src->g.r0, src->g.r1, src->g.H);
    int rw = 0, rh = 0;
    if (hq_reduced_size(src->g.W, src->g.H, factor, &rw, &rh))
        return fail(dst, HQ_ERR_ARG, "hq_set_image_reduced: factor %d outside 1 .. %d", factor, kMaxReduce);
    int rc = check_geom_args(dst, rw, rh, 0, rh);
    if (rc) return rc;
    if ((rc = check_illum_arg(dst, illum))) return rc;
    if ((rc = bind(dst))) return rc;
    float il[3];  // (src's, read before anything of dst changes)
    std::memcpy(il, illum ? illum : src->illum, sizeof il);
    dst->g = make_geom(rw, rh, 0, rh, dst->half);
    if ((rc = begin_image(dst))) return rc;
    ReduceArgs a{};
    a.rgbx = src->img_u8 ? src->d_rgbx.as<uint32_t>() : nullptr;
    a.R = src->d_R.as<float>();
    a.G = src->d_G.as<float>();
    a.B = src->d_B.as<float>();
    a.oR = dst->d_R.as<float>();
    a.oG = dst->d_G.as<float>();
    a.oB = dst->d_B.as<float>();
    a.W = src->g.W;
    a.H = src->g.H;
    a.rw = rw;
    a.rh = rh;
    a.factor = factor;
    ProfRec pr = prof_begin(dst);
    HIP_TRY(dst, timed_launch(pr, kPReduce, [&] { return launch_reduce_image(a, dst->stream); }));
    rc = finish_image(dst, nullptr, il);
    if (!rc) prof_accumulate(dst, pr);  // (finish_image has synchronised the stream)
    return rc;
}

int hq_dot_apron(hq_ctx* c, int* above, int* below) {
    if (!c) return HQ_ERR_ARG;
    if (!above || !below) return fail(c, HQ_ERR_ARG, "null output");
    *above = c->have_image ? c->apron_above : 0;
    *below = c->have_image ? c->apron_below : 0;
    return HQ_OK;
}

int hq_get_image(hq_ctx* c, float* rgba4) {
    if (!c || !rgba4) return HQ_ERR_ARG;
    if (!c->have_image) return fail(c, HQ_ERR_STATE, "no image set");
    int rc = bind(c);
    if (rc) return rc;
    const Geom& g = c->g;
    const size_t n = (size_t)n_own(g), first = (size_t)own_first(g);
    std::vector<float> R(n), G(n), B(n);
    HIP_TRY(c, hipMemcpy(R.data(), c->d_R.as<float>() + first, sizeof(float) * n, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(G.data(), c->d_G.as<float>() + first, sizeof(float) * n, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(B.data(), c->d_B.as<float>() + first, sizeof(float) * n, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) {
        rgba4[4 * i] = R[i]; rgba4[4 * i + 1] = G[i]; rgba4[4 * i + 2] = B[i]; rgba4[4 * i + 3] = 0.f;
    }
    return HQ_OK;
}

namespace {

// hq_set_mask (weights false: the copies hold 0 / 1) and hq_set_weights (the raw bytes)
int set_mask_or_weights(hq_ctx* c, const uint8_t* mask, int w, int h, bool weights) {
    if (!c) return HQ_ERR_ARG;
    const char* const what = weights ? "weight map" : "mask";
    if (!mask) {  // no mask: the state of a fresh context
        c->mask_on = c->weights_on = false;
        c->live_dirty = true;
        return HQ_OK;
    }
    if (!c->have_image) return fail(c, HQ_ERR_STATE, "no image set (hq_set_image)");
    const Geom& g = c->g;
    if (w != g.W || h != g.H) return fail(c, HQ_ERR_ARG, "%s of %d x %d on an image of %d x %d", what, w, h, g.W, g.H);
    const int64_t n_full = mask_count(mask, (int64_t)g.W * g.H);
    if (n_full == 0) return fail(c, HQ_ERR_ARG, "%s without a non-zero byte: no pixel would count", what);
    int rc = bind(c);
    if (rc) return rc;
    // the three copies, built aside so that a failure leaves the mask in force as it was: the
    // owned rows as 0 / 1 (weights: the bytes as they are); at the LabRef planes' pitch (the cost
    // kernels read a dword of 4 pixels next to their LabRef float4s); over the extended rows'
    // positions (the quads of the sums and histogram kernels), zero outside the owned rows and in
    // the padding
    const int own = g.r1 - g.r0;
    std::vector<uint8_t> rows((size_t)g.W * own), lab((size_t)g.lab_pitch * std::max(own, 1) + 16, 0),
        ext((size_t)round_up(g.n_ext, 4) + 16, 0);
    for (int y = 0; y < own; ++y)
        for (int x = 0; x < g.W; ++x) {
            const uint8_t b = mask[(size_t)(g.r0 + y) * g.W + x], v = weights ? b : (uint8_t)(b != 0);
            rows[(size_t)y * g.W + x] = v;
            lab[(size_t)y * g.lab_pitch + x] = v;
            ext[(size_t)(g.r0 - g.e0 + y) * g.W + x] = v;
        }
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // (nothing of this context is in flight)
    DevBuf d_lab, d_ext;
    HIP_TRY(c, d_lab.upload(lab.data(), lab.size()));
    HIP_TRY(c, d_ext.upload(ext.data(), ext.size()));
    std::swap(c->d_mask.p, d_lab.p), std::swap(c->d_mask.bytes, d_lab.bytes);
    std::swap(c->d_maskq.p, d_ext.p), std::swap(c->d_maskq.bytes, d_ext.bytes);
    c->mask_own.swap(rows);
    c->mask_n_full = n_full;
    c->mask_n_own = mask_count(c->mask_own.data(), (int64_t)c->mask_own.size());
    c->mask_w_full = weights ? weight_sum(mask, (int64_t)g.W * g.H) : n_full;
    c->mask_w_own = weight_sum(c->mask_own.data(), (int64_t)c->mask_own.size());
    c->mask_on = true;
    c->weights_on = weights;
    c->live_dirty = true;  // (the list: built by the next evaluation, ensure_live_tiles)
    return HQ_OK;
}

}  // namespace

int hq_set_mask(hq_ctx* c, const uint8_t* mask, int w, int h) { return set_mask_or_weights(c, mask, w, h, false); }

int hq_set_weights(hq_ctx* c, const uint8_t* weights, int w, int h) {
    return set_mask_or_weights(c, weights, w, h, true);
}

int hq_weights_info(hq_ctx* c, int64_t* w_full, int64_t* w_owned) {
    if (!c) return HQ_ERR_ARG;
    const Geom& g = c->g;
    if (w_full) *w_full = c->mask_on ? c->mask_w_full : c->have_image ? (int64_t)g.W * g.H : 0;
    if (w_owned) *w_owned = c->mask_on ? c->mask_w_own : c->have_image ? n_own(g) : 0;
    return HQ_OK;
}

int hq_mask_info(hq_ctx* c, int64_t* n_full, int64_t* n_owned, int64_t* tiles_run, int64_t* tiles_all) {
    if (!c) return HQ_ERR_ARG;
    const Geom& g = c->g;
    if (n_full) *n_full = c->mask_on ? c->mask_n_full : c->have_image ? (int64_t)g.W * g.H : 0;
    if (n_owned) *n_owned = c->mask_on ? c->mask_n_own : c->have_image ? n_own(g) : 0;
    if (tiles_run) *tiles_run = c->res.tiles_run;
    if (tiles_all) *tiles_all = c->res.tiles_all;
    return HQ_OK;
}

// The context's fixed palette colours: host state alone (a search latches it at creation, the
// polishes read its count when called), so nothing on the device and no record changes.
int hq_set_fixed_colors(hq_ctx* c, const float* colors, int n) {
    if (!c) return HQ_ERR_ARG;
    if (n < 0 || n > kMaxKChunked) return fail(c, HQ_ERR_ARG, "n=%d fixed colours: 0 .. %d", n, kMaxKChunked);
    if (!colors) n = 0;
    if (n > 0 && !population_in_range(colors, 1, n))
        return fail(c, HQ_ERR_ARG, "fixed colour with a channel that is not finite or outside [0, 1]");
    c->fixed.assign(colors, colors + (size_t)4 * n);
    for (size_t e = 3; e < c->fixed.size(); e += 4) c->fixed[e] = 0.0f;
    c->fixed_n = n;
    return HQ_OK;
}

int hq_fixed_colors(hq_ctx* c, int* n, float* colors) {
    if (!c) return HQ_ERR_ARG;
    if (n) *n = c->fixed_n;
    if (colors) std::copy(c->fixed.begin(), c->fixed.end(), colors);
    return HQ_OK;
}

int hq_last_path(hq_ctx* c, hq_path_info* info) {
    if (!c || !info || info->size < (int32_t)sizeof(int32_t)) return HQ_ERR_ARG;
    hq_path_info pi = c->path;
    pi.size = std::min<int32_t>(info->size, (int32_t)sizeof(hq_path_info));
    std::memcpy(info, &pi, (size_t)pi.size);
    return HQ_OK;
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
    if ((rc = check_illum_arg(c, illum))) return rc;
    if ((rc = bind(c))) return rc;
    const Geom g = make_geom(w, h, 0, h, c->half);
    const int64_t n = (int64_t)w * h;
    DevBuf dxyz;
    ScielabTmp t;
    HIP_TRY(c, dxyz.ensure(sizeof(float4) * n));
    rc = scielab_filter(c, g, t, [&](float4* opp) {
        HIP_TRY(c, hipMemcpyAsync(dxyz.p, xyz4, sizeof(float4) * n, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, launch_xyz_to_opp(dxyz.as<float4>(), opp, n, c->stream));
        return (int)HQ_OK;
    });
    if (rc) return rc;
    const float* il = illum ? illum : c->illum;
    HIP_TRY(c, launch_labref_lab(t.conv.as<float4>(), nullptr, nullptr, nullptr, dxyz.as<float4>(), w,
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

int hq_assign_coords(hq_ctx* c, int space, const float* rgba4, int64_t n, float* out4) {
    if (!c) return HQ_ERR_ARG;
    if (!rgba4 || !out4 || n < 1) return fail(c, HQ_ERR_ARG, "bad colours / output / n=%lld", (long long)n);
    if (space != 0 && space != 1) return fail(c, HQ_ERR_ARG, "space must be 0 (sRGB) or 1 (CIELAB)");
    int rc = bind(c);
    if (rc) return rc;
    DevBuf din, dout;
    HIP_TRY(c, din.ensure(sizeof(float4) * n));
    HIP_TRY(c, dout.ensure(sizeof(float4) * n));
    float inv[3];
    inv_illuminant(c, inv);
    HIP_TRY(c, hipMemcpyAsync(din.p, rgba4, sizeof(float4) * n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, launch_coords_list(din.as<float4>(), dout.as<float4>(), n, space, inv, c->stream));
    HIP_TRY(c, hipMemcpyAsync(out4, dout.p, sizeof(float4) * n, hipMemcpyDeviceToHost, c->stream));
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

int hq_profile_enable(hq_ctx* c, int on) {
    if (!c) return HQ_ERR_ARG;
    c->prof = on != 0;
    return HQ_OK;
}

int hq_profile_reset(hq_ctx* c) {
    if (!c) return HQ_ERR_ARG;
    std::fill(c->prof_stage, c->prof_stage + kStages, ProfSlot{});
    return HQ_OK;
}

int hq_profile_get(hq_ctx* c, const char* kernel, double* total_ms, int64_t* launches) {
    if (!c || !kernel) return HQ_ERR_ARG;
    for (int s = 0; s < kStages; ++s) {
        if (std::strcmp(kernel, kStageNames[s])) continue;
        if (total_ms) *total_ms = c->prof_stage[s].ms;
        if (launches) *launches = c->prof_stage[s].launches;
        return HQ_OK;
    }
    return fail(c, HQ_ERR_ARG, "unknown kernel '%s'", kernel);
}

int hq_set_option(hq_ctx* c, const char* name, int value) {
    if (!c || !name) return HQ_ERR_ARG;
    static const struct { const char* name; int hq_ctx::*flag; } kOnOff[] = {
        {"trim", &hq_ctx::trim}, {"sa_graph", &hq_ctx::sa_graph}, {"gen_vmfma", &hq_ctx::gen_vmfma},
        {"gen_hmfma", &hq_ctx::gen_hmfma}, {"gen_vtile2", &hq_ctx::gen_vtile2}, {"gen_hrow4", &hq_ctx::gen_hrow4},
        {"sa_device", &hq_ctx::sa_device}, {"shard_solo", &hq_ctx::shard_solo}, {"palette_split", &hq_ctx::psplit},
        {"chunked", &hq_ctx::chunked}, {"mask_skip", &hq_ctx::mask_skip}, {"pixel_err", &hq_ctx::pixel_err},
        {"img_u8", &hq_ctx::img_u8_path}};
    for (const auto& o : kOnOff)
        if (!std::strcmp(name, o.name)) {
            c->*o.flag = value != 0;
            return HQ_OK;
        }
    if (!std::strcmp(name, "assign_space")) {
        // (the coordinates stay current across a change of the option: they depend on the image
        // and the illuminant alone, and space 0 reads none of them)
        if (value != 0 && value != 1) return fail(c, HQ_ERR_ARG, "assign_space must be 0 (sRGB) or 1 (CIELAB)");
        c->assign_space = value;
    } else if (!std::strcmp(name, "grid")) {
        if (value != 0 && value != 16 && value != 32 && value != 64)
            return fail(c, HQ_ERR_ARG, "grid must be 0, 16, 32 or 64");
        c->G2 = value;
    } else if (!std::strcmp(name, "cost_variant")) {
        if (value < 0 || value > 2) return fail(c, HQ_ERR_ARG, "cost_variant must be 0, 1 or 2");
        c->cost_variant = value;
    } else if (!std::strcmp(name, "cost_rows")) {
        if (value != 8 && value != 16) return fail(c, HQ_ERR_ARG, "cost_rows must be 8 or 16");
        c->cost_rows = value;
    } else if (!std::strcmp(name, "gen_hrow_outputs")) {
        if (value != 4 && value != 8) return fail(c, HQ_ERR_ARG, "gen_hrow_outputs must be 4 or 8");
        c->gen_hrow_no = value;
    } else if (!std::strcmp(name, "gen_tile_shape")) {
        if (value < 0 || value > 2) return fail(c, HQ_ERR_ARG, "gen_tile_shape: 0, 1 or 2");
        c->gen_shape = (int)value;
    } else if (!std::strcmp(name, "cost_tw")) {
        if (value != 128 && value != 256) return fail(c, HQ_ERR_ARG, "cost_tw must be 128 or 256");
        c->cost_tw = value;
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
    } else if (!std::strcmp(name, "dither_rows")) {
        if (value < 64 || value > 1024 || value % 64)
            return fail(c, HQ_ERR_ARG, "dither_rows must be a multiple of 64 in 64 .. 1024");
        c->dither_rows = value;
    } else if (!std::strcmp(name, "dot_apron")) {
        if (value < 0 || value > 255) return fail(c, HQ_ERR_ARG, "dot_apron must be in 0 .. 255");
        c->dot_apron = value;  // (read by the next hq_set_image[_planar]_shard: set_apron)
    } else if (!std::strcmp(name, "dot_tile")) {
        if (value < -1 || value > 1) return fail(c, HQ_ERR_ARG, "dot_tile must be -1, 0 or 1");
        c->dot_tile = value;
    } else if (!std::strcmp(name, "dot_tile_shape")) {
        if (value < 0 || value > kDotTileShapes)
            return fail(c, HQ_ERR_ARG, "dot_tile_shape must be in 0 .. %d", kDotTileShapes);
        c->dot_tile_shape = value;
    } else if (!std::strcmp(name, "cent_span")) {
        if (value < 0) return fail(c, HQ_ERR_ARG, "cent_span must be >= 0 (0 = auto)");
        c->cent_span = value;
    } else if (!std::strcmp(name, "assign_blocks_per_cu")) {
        if (value < 0 || value > 64) return fail(c, HQ_ERR_ARG, "assign_blocks_per_cu in [0,64] (0 = auto)");
        c->assign_blocks_per_cu = value;
    } else {
        return fail(c, HQ_ERR_ARG, "unknown option '%s'", name);
    }
    return HQ_OK;
}

}  // extern "C"
