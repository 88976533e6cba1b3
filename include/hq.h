/*
 * hq.h -- C ABI of libhq, the MI355X-native SWASA dE cost evaluator.
 *
 * Drop-in boundary: every entry point below replaces one method of the
 * reference's JavaCL backend `ImageManipulation` (IM) or its helpers, and is
 * what a JNI shim bound to that class calls (INTEGRATION.md shows the Java
 * side).  Reference files live under
 *   /root/reference/src/plugins/dbrasseur/hybridquantization/
 * with tags IM = ImageManipulation.java, SP = ScielabProcessor.java,
 * SW = SWASA.java, HQ = HybridQuantization.java, CL = OptimizedConvolution.cl.
 *
 * Conventions
 *  - Plain C types only; host pointers are caller-owned and only read/written
 *    for the duration of the call.
 *  - "inline float4" = the reference's RGBA / Lab layout: float[4*N], pixel
 *    p = y*w + x at [4p .. 4p+3], .w = 0 (HQ:279-291 makeinline).
 *  - Palettes: float[4*K] per palette with .w = 0 (SW:40-52); populations are
 *    P palettes back to back.
 *  - Every function returns HQ_OK (0) or a positive HQ_ERR_* code; the message
 *    of the last failure is available from hq_last_error(ctx).  The JNI shim
 *    maps a non-zero status to an exception (IM:79-92 fallback semantics).
 *  - One host thread per context at a time (IM's single in-order queue).
 */
#ifndef HQ_H
#define HQ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HQ_VERSION 1

enum hq_status {
    HQ_OK = 0,
    HQ_ERR_ARG = 1,          /* invalid argument / shape */
    HQ_ERR_DEVICE = 2,       /* HIP runtime failure or no device */
    HQ_ERR_STATE = 3,        /* call order violated (e.g. no image set) */
    HQ_ERR_UNSUPPORTED = 4,  /* valid request outside what this build supports */
    HQ_ERR_COMM = 5,         /* RCCL failure */
    HQ_ERR_NOMEM = 6
};

/* IM:20 enum deltaETypes.  CIE76 is what the plugin always uses (HQ:96, HQ:145).
 * CIE94 is the reference's (CL:217-226), its unclamped dH included: NaN on real
 * images.  CIEDE2000 is libhq's own addition -- the reference's branch is empty
 * (CL:227-230): the formula of Sharma, Wu & Dalal, "The CIEDE2000
 * color-difference formula: implementation notes, supplementary test data, and
 * mathematical observations", Color Res. Appl. 30(1), 2005, kL = kC = kH = 1,
 * sample 1 the original's S-CIELAB and sample 2 the candidate's; finite (no
 * NaN of the CIE94 kind) for Lab values below 1e9 in magnitude, on every path a
 * context of the other types takes. */
enum hq_delta_e { HQ_DE_CIE76 = 0, HQ_DE_CIE94 = 1, HQ_DE_CIEDE2000 = 2 };

/* SP:19 enum Whitepoint */
enum hq_whitepoint { HQ_WP_D50 = 0, HQ_WP_D65 = 1 };

typedef struct hq_ctx hq_ctx;
typedef struct hq_search hq_search;

int hq_version(void);
const char *hq_status_string(int status);
/* Number of visible HIP devices (0 when none).  Never initialises a context. */
int hq_device_count(int *count);

/* IM:52 ImageManipulation(deltaEType, verbose, convergence): binds `device`,
 * creates the context's stream.  Fails with HQ_ERR_DEVICE when no GPU is
 * usable -- the caller's fallback path of IM:79-92. */
int hq_create(int device, int delta_e_type, hq_ctx **out);
/* IM:265 close(): releases every device buffer, stream and communicator. */
void hq_destroy(hq_ctx *ctx);
const char *hq_last_error(const hq_ctx *ctx);

/* SP:66-181 ScielabProcessor constructor (filter design) followed by the
 * packing of IM:800-841.  Host-only.  Writes k1[4*T], k2[4*T] (float4 taps:
 * channel filters (g0j, g1j, g2j, 0)), k3[T] = g02 and absk3[T] = |g02|;
 * *taps = T, illum[3] = whitepoint.  Buffers must hold max_taps taps. */
int hq_design_filters(int dpi, double viewing_distance, int whitepoint, int max_taps,
                      float *k1, float *k2, float *k3, float *absk3, int *taps,
                      float *illum);

/* IM:800 updateOpenCLFilters(filters, absfilters): uploads the packed taps.
 * halfSize = (4*taps)/8 as IM:408.  Any taps are accepted.  The matrix-core
 * cost kernels hold a tap as f16 parts of tap * 2^16, so a set with a tap of
 * magnitude above 65504 / 65536 (0.99951; every designed tap is below 0.987)
 * or a non-finite tap is evaluated by the fp32 cost kernels instead: the same
 * results within fp32 rounding, at the generic path's speed. */
int hq_set_filters(hq_ctx *ctx, int taps, const float *k1, const float *k2, const float *k3,
                   const float *absk3);

/* IM:100 RGBtoXYZ: planar R,G,B (n floats each) -> inline XYZ float4 (CL:79-90). */
int hq_rgb_to_xyz(hq_ctx *ctx, const float *R, const float *G, const float *B, int64_t n,
                  float *xyz4);
/* IM:285 XYZtoScielab(XYZ, filters, absfilters, w, illuminant): inline XYZ ->
 * inline S-CIELAB Lab (CL:111-116, CL:2-74 filter by filter, CL:124-145).
 * illum: the white point (Xn, Yn, Zn) of CL:124-131; NULL means the context's
 * current illuminant (see hq_set_image).  The call never changes the context's
 * illuminant.  A component that is not finite and greater than 0: HQ_ERR_ARG, as
 * for hq_set_image. */
int hq_xyz_to_scielab(hq_ctx *ctx, const float *xyz4, int w, int h, const float *illum,
                      float *lab4);

/* Device-resident state of IM:383 findBestQuantization (IM:450-478):
 * uploads the inline RGBA image and its S-CIELAB (inline Lab float4) once.
 * lab4 may be NULL: the S-CIELAB of the image is then computed on the device
 * (IM:100 + IM:285 semantics).  Requires w, h >= halfSize.
 * illum: the white point (Xn, Yn, Zn) that Opp->Lab divides by (CL:124-131), any
 * three floats, each finite and greater than 0 (Yn need not be 1); it becomes the
 * context's illuminant, which every later evaluation, rendering and search pass
 * reads.  illum == NULL keeps the context's current illuminant: D65 (0.95047, 1,
 * 1.0883) on a new context, else the one the last successful hq_set_image* /
 * hq_set_image_reduced call left.  A component that is NaN, infinite, zero (either
 * sign) or negative: HQ_ERR_ARG, hq_last_error names the component (illum[i]), and
 * nothing of the context changes -- its image, illuminant, evaluated population and
 * what the getters read stay, and a live search runs on.  The same holds for
 * hq_set_image_shard, hq_set_image_planar_shard, the explicit illum of
 * hq_set_image_reduced and hq_xyz_to_scielab. */
int hq_set_image(hq_ctx *ctx, const float *rgba4, const float *lab4, int w, int h,
                 const float *illum);
/* Row-block shard of a (w x h) image for multi-GPU evaluation:
 * this context owns rows [row_begin, row_end); rgba4/lab4 point at the FULL
 * image (only the owned rows +- halfSize halo rows are read). */
int hq_set_image_shard(hq_ctx *ctx, const float *rgba4, const float *lab4, int w, int h,
                       const float *illum, int row_begin, int row_end);
/* Same as hq_set_image_shard but planar float R,G,B of the FULL image (no Lab:
 * it is always computed on the device).  Used by bench.py. */
int hq_set_image_planar_shard(hq_ctx *ctx, const float *R, const float *G, const float *B,
                              int w, int h, const float *illum, int row_begin, int row_end);
/* Reads back the device S-CIELAB of the owned rows as inline float4. */
int hq_get_labref(hq_ctx *ctx, float *lab4);
/* Reads back the device image of the owned rows as the argmin sees it, inline RGBA
 * float4 with .w = 0 (w*(row_end-row_begin) pixels): the planar floats; the packed
 * 8-bit copy, where there is one, rebuilds the same bits.  HQ_ERR_STATE: no image
 * set.  Pairs with hq_get_labref; the test surface of hq_set_image_reduced. */
int hq_get_image(hq_ctx *ctx, float *rgba4);

/* IM:620 computeQuantizationErrorPopulation for P palettes of K colours
 * (K in [1, 2^24] as the plugin allows, HQ:192).  K <= 256: the pruned grid
 * argmin and the tiled fast stencil.  256 < K <= 16384: chunked palettes (nch
 * sub-palettes of 256, 16-bit indices; 512 < K <= 8192: one grid of 16-bit
 * candidate lists over all K colours, option "lists16", otherwise a grid and
 * assign pass per chunk; the fast stencil up to K = 8192, the generic one
 * above; option "chunked").  K > 16384,
 * palettes with non-finite colours or
 * outside the fast path's range, option "chunked" 0 or "grid" 0: the exhaustive
 * argmin with 32-bit indices and the generic stencil path.  All give the same
 * indices and used flags (bit-exact) and the same cost (1e-6 relative):
 * costs[p] = mean dE + delta * #unused (IM:712, SW:74-82), dE of the context's
 * type: dE76, the reference's dE94, or CIEDE2000 (libhq's addition, Sharma, Wu
 * & Dalal 2005; see hq_delta_e) -- the argmin is nearest in RGB whatever the
 * type, so indices and used flags do not depend on it; used[p*K+k] in
 * {0,1} (CL:193), may be NULL.  On a sharded context with a communicator the
 * partial sums are all-reduced over RCCL first. */
int hq_eval_population(hq_ctx *ctx, const float *palettes, int P, int K, float delta,
                       double *costs, int32_t *used);
/* Shard-local partial results without the all-reduce: partial[p*(1+K)] = fp64
 * sum of dE over the owned rows, partial[p*(1+K)+1+k] = 1.0 if colour k is used
 * by an owned-or-halo pixel else 0.0. */
int hq_eval_population_partial(hq_ctx *ctx, const float *palettes, int P, int K,
                               double *partial);
/* The read-back rule of hq_get_indices, hq_get_indices32 and hq_get_pixel_errors:
 * they answer for the last evaluation on the image and filters in force -- the
 * last successful hq_eval_population[_partial], hq_dither_population (the
 * dithered rendering), hq_ordered_population[_partial] (the ordered rendering), or
 * evaluation inside hq_refine_population,
 * hq_repair_population, hq_search_create[_from] and hq_search_run (the last
 * candidates the search evaluated; a run that evaluates nothing changes nothing,
 * unless it had to reallocate the buffers read here -- a larger image set since
 * hq_search_create -- which ends it like a failed evaluation).
 * hq_set_image*, hq_set_filters and an evaluation that fails after it has
 * passed its argument checks end that: until the next successful evaluation the
 * three return HQ_ERR_STATE with a message and write nothing.
 * hq_get_pixel_errors needs in addition that the evaluation stored its error
 * image (option "pixel_err" 1 when it was enqueued) and that the option is
 * still 1; after hq_search_create[_from] or hq_search_run it is HQ_ERR_STATE
 * until the next evaluation call (a repair iteration's side pass stores the
 * error image of candidates that the search then moves).
 *
 * Per-pixel palette indices (u8, K <= 256) of the last evaluated population's
 * palette p over the owned rows (w*(row_end-row_begin) bytes).  HQ_ERR_STATE
 * when that population had K > 256 colours, and by the rule above. */
int hq_get_indices(hq_ctx *ctx, int p, uint8_t *idx);
/* The same for any K (1 .. 2^24, HQ:192): 32-bit indices, w*(row_end-row_begin)
 * of them -- the reference's int index of CL:172-193.  HQ_ERR_STATE by the
 * rule above. */
int hq_get_indices32(hq_ctx *ctx, int p, uint32_t *idx);
/* Test surface: the per-pixel dE of palette p of the last evaluation over the
 * owned rows (w*(row_end-row_begin) floats) -- the error image the reference
 * reads back per member (IM:663-667, CL:201-209).  Needs option "pixel_err" = 1
 * before that evaluation (the cost kernels then also store it); HQ_ERR_STATE
 * otherwise, and by the read-back rule above: an error image that an earlier
 * evaluation stored is never returned for a later one that stored none. */
int hq_get_pixel_errors(hq_ctx *ctx, int p, float *err);

/* ---- k-means palette refinement: libhq's additions, no reference counterpart ----
 * The plugin implements Schaefer & Nolle's hybrid quantization, of which the
 * reference holds the simulated-annealing half only.  A k-means step replaces
 * each palette colour by the mean of the pixels assigned to it; the assignment
 * is the evaluation's argmin (the index images stay on the device), the three
 * entry points below add the means.
 *
 * hq_cluster_sums: per palette and colour of the population last evaluated by
 * hq_eval_population or hq_eval_population_partial on this context, the sum of
 * the assigned pixels and their count over the owned rows (halo rows are not
 * counted): sums[((p*K)+k)*4 + {0,1,2,3}] = (sum R, sum G, sum B, count), exact
 * integers in units of 1 / *den.  *den = 255 when the evaluation's argmin read
 * the packed 8-bit copy of a k/255 image (sums of the bytes), else 2^32: each
 * channel value v adds llrint(v * 2^32) (round half to even; exact for every
 * float in [2^-9, 1], the nearest multiple of 2^-32 below).  Option "img_u8" 0
 * gives 2^32 on every image.  The sums of disjoint shards of one image add up
 * exactly to the whole image's when their den agree.  Every argmin path and
 * index width is served (K <= 256, chunked palettes, K > 16384, "grid" 0).
 * HQ_ERR_STATE: no population evaluated yet, P or K other than that
 * evaluation's, or a search run has evaluated since.  HQ_ERR_UNSUPPORTED: a
 * palette slice ("slice_ranks" > 1, "palette_split"), or (den 2^32) a pixel of
 * the owned rows that is not finite or lies outside [0, 1] -- sums and den are
 * then left untouched.  With at most 2^30 pixels per shard no sum overflows. */
int hq_cluster_sums(hq_ctx *ctx, int P, int K, int64_t *sums, int64_t *den);
/* The k-means update from such sums (of one context, or several shards' added
 * up).  Host-only, needs no context.  Every colour with count > 0 becomes the
 * mean of its pixels, channel c = (float)((double)sum_c / (255.0 * (double)count))
 * for den = 255, (float)(ldexp((double)sum_c, -32) / (double)count) for
 * den = 2^32, and .w = 0.  A colour with count 0 keeps its bits: a duplicate at
 * a higher index, a colour no pixel is nearest to, a non-finite colour.  Any
 * other den: HQ_ERR_ARG. */
int hq_centroids_from_sums(const int64_t *sums, int64_t den, int P, int K, float *palettes);
/* Evaluates the P palettes, then `steps` times: hq_cluster_sums, the update
 * above, an evaluation of the updated palettes.  trace (may be NULL) receives
 * the costs of step 0 (the input) to step `steps`, trace[s*P + p].  keep_best 0:
 * palettes, costs and used are those of the last step.  keep_best 1: per
 * palette those of its lowest-cost step, the earliest on a tie; a NaN cost
 * never beats a number.  k-means lowers the RGB distortion while the cost is
 * S-CIELAB dE plus delta per unused colour, so the cost can rise: keep_best 1
 * refuses that.  steps = 0 is hq_eval_population.  used may be NULL.  Needs
 * the whole image on this context (HQ_ERR_STATE on a shard) and no
 * communicator of more than one rank (HQ_ERR_UNSUPPORTED). */
int hq_refine_population(hq_ctx *ctx, float *palettes, int P, int K, int steps, float delta,
                         int keep_best, double *costs, int32_t *used, double *trace);

/* ---- repairing unused colours: libhq's additions, no reference counterpart ----
 * The cost is mean dE + delta per unused colour (IM:712, SW:74-82), and neither
 * a k-means move (a colour without pixels keeps its bits) nor a median cut of an
 * image with few colours (the copies past *made) brings an unused colour back.
 * The entry points below do: the per-colour error of an evaluated population on
 * the device, a host rule that moves every unused colour onto the worst pixel of
 * a cluster that carries much error, and a polish call around the two.
 *
 * hq_cluster_errors: per palette and colour of the population last evaluated by
 * hq_eval_population[_partial] on this context with option "pixel_err" 1 in
 * force, over the owned rows (halo rows are not counted),
 * err[((p*K)+k)*4 + {0,1,2,3}]:
 *  [0] the sum over the pixels assigned to k of llrint(e * 2^20), e the pixel's
 *      fp32 dE as the cost kernel stored it (hq_get_pixel_errors), widened to
 *      double: the product is exact, the rounding half to even.  Exact integers,
 *      independent of any order; no overflow while a cluster's dE sum stays
 *      below 2^43.
 *  [1] the count of those pixels: hq_cluster_sums' count.
 *  [2], [3] the cluster's worst movable pixel.  A pixel is movable when its RGB
 *      as the argmin saw it (the planar floats, or the packed bytes' value
 *      k/255 rebuilt in fp32) differs from colour k in at least one channel
 *      under fp32 != -- moving a colour onto a pixel it already equals changes
 *      nothing.  The worst one has the largest dE, on a tie the lowest position
 *      y*w + x in the FULL image.  [2] = the bits of that dE as a non-negative
 *      integer, [3] = the position; no movable pixel: [2] = 0, [3] = -1.
 * worst_rgb[((p*K)+k)*4 ..] = (R, G, B, 0) of that pixel as the argmin saw it,
 * zeros without one.
 * Shards: [0] and [1] of disjoint shards of one image add up exactly to the
 * whole image's; [2], [3] and worst_rgb merge by the same rule as inside a
 * shard -- the larger [2] wins, then the lower [3], worst_rgb follows the winner.
 * (The whole image's: where the shards' stored dE are.  The cost kernels give a
 * pixel the same dE bits in every sharding for CIEDE2000; for dE76 and dE94
 * when a row block starts on a multiple of their tile rows, 16 by default.)
 * Every argmin path and index width is served, as by hq_cluster_sums, and the
 * evaluated population is not disturbed (hq_cluster_sums, hq_get_indices and
 * hq_get_pixel_errors answer after it as before it).
 * HQ_ERR_STATE: no population evaluated yet, P or K other than that
 * evaluation's, a search run has evaluated since, or "pixel_err" was off at
 * that evaluation.  HQ_ERR_UNSUPPORTED: a palette slice ("slice_ranks" > 1,
 * "palette_split"); a full image of 2^32 pixels or more; an owned pixel whose dE
 * is not a finite number in [0, 2^20) (dE94's NaN, a non-finite palette colour,
 * a caller's NaN LabRef) -- such a pixel is counted in [1] but left out of [0]
 * and of the worst pixel, and both outputs are then left untouched. */
int hq_cluster_errors(hq_ctx *ctx, int P, int K, int64_t *err, float *worst_rgb);
/* The repair rule from such statistics (of one context, or several shards'
 * merged as above).  Host-only, needs no context, integer arithmetic,
 * deterministic.  Per palette: the receivers are the colours with count 0, in
 * ascending index; the donors are the colours with count > 0 and [3] >= 0,
 * ordered by [0] descending, the lower index first on a tie.  The i-th
 * receiver becomes the i-th donor's worst_rgb, .w = 0, until the receivers, the
 * donors or max_moves (< 0: no limit) run out.  Each donor gives once and keeps
 * its own colour.  Two donors cannot hand out equal colours (equal RGB has one
 * argmin, so the two pixels would sit in one cluster), and a reseeded colour
 * differs from its donor's (the pixel is movable).  moved[p] (moved may be
 * NULL) = the number of colours replaced.  HQ_ERR_ARG: a negative count or
 * sum, P < 1, K < 1, a null pointer; the palettes are then left untouched. */
int hq_reseed_unused(const int64_t *err, const float *worst_rgb, int P, int K, int max_moves,
                     float *palettes, int *moved);
/* The same rule when the first nfixed colours of every palette are fixed
 * (hq_set_fixed_colors): a receiver is a colour k >= nfixed with count 0.  A
 * fixed colour is never a receiver -- unused, it stays where it is, takes no
 * place in the receivers' order and consumes no donor -- and is a donor like any
 * other colour.  nfixed = 0 is hq_reseed_unused bit for bit.  HQ_ERR_ARG in
 * addition: nfixed < 0 or nfixed > K; the palettes are then left untouched. */
int hq_reseed_unused_fixed(const int64_t *err, const float *worst_rgb, int P, int K,
                           int max_moves, int nfixed, float *palettes, int *moved);
/* Evaluates the P palettes with "pixel_err" forced on for the call (the
 * caller's value is back afterwards), then `steps` times: hq_cluster_errors,
 * hq_reseed_unused(max_moves), an evaluation of the repaired palettes.  trace,
 * keep_best, costs and used as in hq_refine_population.  A step that moves no
 * colour of any palette ends the loop: the remaining trace rows repeat the last
 * step's costs.  hq_refine_population's scope: the whole image on this context
 * (HQ_ERR_STATE on a shard), no communicator of more than one rank
 * (HQ_ERR_UNSUPPORTED); hq_cluster_errors' refusals are passed on. */
int hq_repair_population(hq_ctx *ctx, float *palettes, int P, int K, int steps, float delta,
                         int max_moves, int keep_best, double *costs, int32_t *used,
                         double *trace);

/* ---- dithered rendering: libhq's addition, no reference counterpart ----
 * S-CIELAB blurs the opponent channels as the eye does before it takes dE; the
 * nearest-colour rendering's error is low-frequency and survives that blur, an
 * error-diffused rendering's does not.  hq_dither_population evaluates the P
 * palettes (K <= 256) on the context's image as hq_eval_population does, with
 * the index images chosen by raster Floyd-Steinberg error diffusion instead of
 * the argmin alone.  In the argmin's space (the sRGB-coded planar floats), per
 * channel, every operation one fp32 operation rounded to nearest and none
 * contracted into an fma, e = 0 outside the image, s = strength:
 *     a = 7 e(x-1, y)   b = 3 e(x+1, y-1)   c = 5 e(x, y-1)   d = e(x-1, y-1)
 *     t = ((a + b) + (c + d)) * 0.0625
 *     v = min(max(pix + s * t, 0), 1)
 *     idx(x, y) = the first minimum over k of the argmin's distance(v, pal[k])
 *     e(x, y) = v - pal[idx]          (pal[k].w taken as 0)
 * At strength 0 the indices, used flags and costs are hq_eval_population's, bit
 * for bit.  costs[p] = mean dE + delta * #unused of the dithered rendering: the
 * context's dE type and whichever cost path its filters and options select; a
 * colour is used when it appears in the dithered index image.  used may be NULL.
 * Afterwards hq_get_indices, hq_get_indices32 and hq_get_pixel_errors answer for
 * the dithered rendering, and hq_cluster_sums and hq_cluster_errors return
 * HQ_ERR_STATE until the next hq_eval_population[_partial] (a k-means or repair
 * move from a dithered assignment is neither).  Toward a live hq_search the
 * call behaves as hq_eval_population does.
 * HQ_ERR_ARG: P < 1, K < 1, a null palettes or costs, a strength outside
 * [0, 1] (NaN included), a palette channel that is not finite or outside [0, 1]
 * (hq_search_create_from's rule).  HQ_ERR_STATE: no image set, a row-block
 * shard.  HQ_ERR_UNSUPPORTED: a communicator of more than one rank, option
 * "palette_split" or "slice_ranks" > 1, K > 256, an image pixel that is not
 * finite or outside [0, 1] (found on the device once per image).  On any refusal
 * the outputs and the evaluated state are untouched. */
int hq_dither_population(hq_ctx *ctx, const float *palettes, int P, int K, float strength,
                         float delta, double *costs, int32_t *used);

/* ---- error diffusion with other kernels: libhq's addition ----
 * A diffusion kernel in scatter notation, as the literature writes it:
 * w[dy][dx + 2] / div is the share of its error that pixel (x, y) sends to
 * (x + dx, y + dy), dy = 0 .. 2, dx = -2 .. 2.  A tap set is legal when every
 * weight is >= 0, row 0 holds weights at dx = 1 and 2 only (the raster order has
 * passed the others), div >= 1, at least one weight is non-zero and the weights'
 * sum is at most div (and so fits an int32) -- under which every |e| and |t|
 * below stays <= 1.
 * The rendering is hq_dither_population's with another value for the argmin: in
 * the argmin's space, per channel, every operation one fp32 operation rounded to
 * nearest and none contracted into an fma, e = 0 outside the image, s = strength:
 *     acc = the products float(w[dy][dx+2]) * e(x-dx, y-dy), added one at a time in
 *           the order dy = 0 (dx = 1, 2), dy = 1 (dx = -2 .. 2), dy = 2 (dx = -2 .. 2);
 *           acc starts as the first product
 *     t   = acc / float(div)                 (IEEE division, correctly rounded)
 *     v   = min(max(pix + s * t, 0), 1)
 *     idx(x, y) = the first minimum over k of the argmin's distance(v, pal[k])
 *     e(x, y) = v - pal[idx]                 (pal[k].w taken as 0)
 * The device adds the product of every tap position its kernel instance holds,
 * zero weights included: such a product is +-0 and changes no v.
 * hq_diffusion_preset fills *taps with a kernel of the literature (HQ_ERR_ARG: a
 * null taps, an unknown preset). */
typedef struct hq_diffusion_taps {
    int32_t w[3][5];
    int32_t div;
} hq_diffusion_taps;
enum hq_diffusion {
    HQ_DIFFUSION_FLOYD_STEINBERG = 0, /* 7 | 3 5 1                           / 16 */
    HQ_DIFFUSION_JARVIS = 1,          /* 7 5 | 3 5 7 5 3 | 1 3 5 3 1         / 48 */
    HQ_DIFFUSION_STUCKI = 2,          /* 8 4 | 2 4 8 4 2 | 1 2 4 2 1         / 42 */
    HQ_DIFFUSION_BURKES = 3,          /* 8 4 | 2 4 8 4 2                     / 32 */
    HQ_DIFFUSION_SIERRA3 = 4,         /* 5 3 | 2 4 5 4 2 | 0 2 3 2 0         / 32 */
    HQ_DIFFUSION_SIERRA2 = 5,         /* 4 3 | 1 2 3 2 1                     / 16 */
    HQ_DIFFUSION_SIERRA_LITE = 6,     /* 2 | 1 1 (dx = -1, 0)                /  4 */
    HQ_DIFFUSION_ATKINSON = 7,        /* 1 1 | 1 1 1 (dx = -1 .. 1) | 1 (dx = 0) / 8 */
    HQ_DIFFUSION_COUNT = 8
};
int hq_diffusion_preset(int which, hq_diffusion_taps *taps);
/* 1 when the tap set is legal (above), else 0 (a null pointer included). */
int hq_diffusion_taps_legal(const hq_diffusion_taps *taps);
/* The kernel instance a legal tap set runs: *rows = R, the highest dy that holds a
 * weight, at least 1; *slope = S = max(a, 1) + 1 with a the largest -dx among row
 * 1's weights, the slope of the wavefronts t = x + S y whose order is the raster
 * order's.  HQ_ERR_ARG: a null pointer, an illegal tap set. */
int hq_diffusion_classify(const hq_diffusion_taps *taps, int *rows, int *slope);

/* hq_dither_population with the diffusion kernel *taps: its refusals, the state
 * afterwards (the getters answer for the rendering, hq_cluster_sums and
 * hq_cluster_errors return HQ_ERR_STATE), its behaviour toward a live hq_search, a
 * mask and weights, and in addition HQ_ERR_ARG for a null or illegal tap set.
 * A tap set equal to the Floyd-Steinberg preset (weights and div) runs
 * hq_dither_population's kernel with hq_dither_population's formula -- the result
 * is that call's bit for bit (its formula multiplies by 1/16 and pairs the sums,
 * which the division and the order above need not reproduce); hq_last_path then
 * reports HQ_ARGMIN_DITHER.  Every other tap set runs the definition above
 * (HQ_ARGMIN_DIFFUSE, with diffuse_rows and diffuse_slope).  The results do not
 * depend on option "dither_rows"; instances of slope 3 run strips of at most 512
 * rows. */
int hq_diffuse_population(hq_ctx *ctx, const float *palettes, int P, int K,
                          const hq_diffusion_taps *taps, float strength, float delta,
                          double *costs, int32_t *used);

/* ---- dot diffusion: libhq's addition, no reference counterpart ----
 * Knuth's dot diffusion (1987) is error diffusion without the raster recurrence.
 * A class matrix of side n in {4, 8, 16}, tiled over the image, gives every pixel
 * a class: cls[y*n + x] is a permutation of 0 .. n*n - 1 (anything else is
 * illegal; entries past n*n are not read), and the class of pixel (x, y) is
 * cls[(y mod n)*n + (x mod n)].  Pixels are taken in ascending class, and each
 * hands its error only to those of its 8 neighbours that have a higher class.
 * Two pixels of one class are at least n apart and share no neighbour, so a class
 * is one parallel step over all its pixels: the device runs one launch per class,
 * in ascending class on the context's stream (a class without a pixel -- the image
 * is smaller than the tile -- gets none).
 * The 8 neighbour offsets: the four orthogonal ones have weight wt = 2, the four
 * diagonal ones wt = 1.  In the argmin's space (the pixel as hq_dither_population
 * reads it), per channel, every operation one fp32 operation rounded to nearest and
 * none contracted into an fma, s = strength:
 *     W(p)   = the sum of the weights of p's neighbours that lie inside the image
 *              and have a class above p's
 *     a(q)   = +0, then, for q's in-image neighbours p of lower class, in ascending
 *              class of p (they are pairwise distinct):
 *                  a = a + (float(wt(p, q)) * e(p)) / float(W(p))   (IEEE division)
 *     v      = min(max(pix(q) + s * a(q), 0), 1)
 *     idx(q) = the first minimum over k of the argmin's distance(v, pal[k])
 *     e(q)   = v - pal[idx]                 (pal[k].w taken as 0)
 * A pixel with no in-image neighbour of higher class (a "baron", or a pixel an edge
 * makes one) drops its error.  At strength 0 the indices, used flags and costs are
 * hq_eval_population's, bit for bit.  A colour is used when it appears in the index
 * image; the costs are this rendering's under the context's dE type, cost path,
 * mask or weights, exactly as for hq_dither_population.
 * HQ_DOT_KNUTH8 is Knuth's 8 x 8 class matrix, row by row:
 *     34 48 40 32 29 15 23 31        28 14 22 30 35 49 41 33
 *     42 58 56 53 21  5  7 10        20  4  6 11 43 59 57 52
 *     50 62 61 45 13  1  2 18        12  0  3 19 51 63 60 44
 *     38 46 54 37 25 17  9 26        24 16  8 27 39 47 55 36
 * (rows 0 .. 3 on the left, 4 .. 7 on the right); tiled, it has 2 barons.
 * Measured on one MI355X (profiles/dot_c3.json): the 64 launches take
 * 2.89 ms at 4096 x 4096, K = 256 for one palette and 7.37 ms for four, against 338 ms
 * for hq_dither_population's kernel in the same process; 0.36 against 2.41 ms at
 * 512 x 512, K = 16.  On a 64 x 64 ramp under the eight cube corners the cost is 0.514
 * of the nearest-colour one (Floyd-Steinberg 0.479).  A search under this objective:
 * hq_search_set_dot.  Not measured: more than one GPU (refused), K > 256 (refused).  On a whole image the
 * launches may be one (the tiled form below, option "dot_tile"): the same indices, bit for bit. */
typedef struct hq_dot_classes {
    int32_t n;
    int32_t cls[256];
} hq_dot_classes;
enum hq_dot_matrix { HQ_DOT_KNUTH8 = 0, HQ_DOT_COUNT = 1 };
/* Fills *out with a built-in matrix (entries past n*n are 0).  HQ_ERR_ARG: a null
 * out, an unknown preset. */
int hq_dot_preset(int which, hq_dot_classes *out);
/* 1 when the matrix is legal (above), else 0 (a null pointer included). */
int hq_dot_classes_legal(const hq_dot_classes *cls);
/* The number of cells whose 8 neighbours on the torus all have a lower class
 * (informational); -1 for an illegal matrix. */
int hq_dot_barons(const hq_dot_classes *cls);
/* hq_dither_population with the dot-diffused rendering under *cls (NULL: the
 * HQ_DOT_KNUTH8 matrix): its refusals, the state afterwards (the getters answer for
 * the rendering, hq_cluster_sums and hq_cluster_errors return HQ_ERR_STATE until the
 * next hq_eval_population[_partial]), its behaviour toward a live hq_search, a mask
 * and weights, and in addition HQ_ERR_ARG for an illegal matrix and
 * HQ_ERR_UNSUPPORTED for P > 65535 (a launch holds the palettes in its grid).  On any
 * refusal the outputs and the evaluated state are untouched.  hq_last_path reports
 * HQ_ARGMIN_DOT (diffuse_rows and diffuse_slope 0).  The matrix's tables are
 * uploaded when it differs from the last call's. */
int hq_dot_population(hq_ctx *ctx, const float *palettes, int P, int K, const hq_dot_classes *cls,
                      float strength, float delta, double *costs, int32_t *used);

/* ---- dot diffusion on row-block shards ----
 * idx(q) depends on the pixels a path of neighbour steps with strictly descending class
 * reaches from q, and on nothing else.  The matrix is periodic, so how far above and below q
 * such a path can get is a property of the matrix alone, its reach.  A shard that also
 * renders that many rows above and below its extended rows (its owned rows +- the filters'
 * half-width) therefore produces the whole image's indices on its extended rows bit for bit,
 * with no exchange between devices; the rows beyond the extended ones (the apron) are
 * rendered for their errors alone.
 *
 * hq_dot_reach: *above is the largest number of rows by which a pixel that idx(q) depends on
 * can lie above q, *below the same below q, over all q of the tiled plane (host-only).  In
 * ascending class, for a cell c and each neighbour p of lower class at offset (dx, dy), taken
 * on the torus:  above[c] = max(above[c], above[p] - dy),  below[c] = max(below[c], below[p] + dy),
 * both from 0; the result is the maximum over the cells.  Both lie in 1 .. n*n - 1 and may
 * exceed n (paths cross tile borders).  HQ_DOT_KNUTH8: (5, 5); the row-major 16 x 16 matrix:
 * (15, 1).  HQ_ERR_ARG (outputs untouched): an illegal matrix, a null pointer. */
int hq_dot_reach(const hq_dot_classes *cls, int *above, int *below);
/* Option "dot_apron" (rows, 0 .. 255, default 0) is read by hq_set_image_shard and
 * hq_set_image_planar_shard: a shard with extended rows [e0, e1) of an image of h rows also
 * keeps the planar floats of rows [max(0, e0 - A), e0) and [e1, min(h, e1 + A)), in storage of
 * its own that no other call reads.  A whole image keeps none whatever the option says, and
 * changing the option afterwards does not change what is held; the apron goes where the image
 * goes and is replaced by the next hq_set_image*.  hq_dot_apron reports the rows held on each
 * side (0, 0 without an image).  HQ_ERR_ARG: a null pointer. */
int hq_dot_apron(hq_ctx *ctx, int *above, int *below);
/* hq_dot_population without the final division and penalty, in hq_eval_population_partial's
 * layout partial[P][1 + K]: the partials of disjoint shards of one image add up to the whole
 * image's, and the used flags OR.  On a whole image it is hq_dot_population's rendering
 * (the same launches).  On a row-block shard the held apron must be at least
 * min(reach, rows between the extended rows and the image's border) on each side, under the
 * reach of *cls (NULL: HQ_DOT_KNUTH8); else HQ_ERR_STATE, and hq_last_error names the needed
 * and the held rows.  The shard's launches run over the window [e0 - above, e1 + below)
 * (clipped to the image): the class of a pixel comes from its full-image row and the border
 * rule of W(p) from the full image's height, a pixel outside the window is never read, and
 * indices and used flags are written for the extended rows only -- they are the whole
 * image's.  A class without a pixel in the window gets no launch.
 * Everything else is hq_dot_population's: its refusals (K > 256, a palette slice, a
 * communicator of more than one rank -- the reduction across ranks is the caller's --, an
 * illegal matrix, palette or strength, P > 65535, an image pixel outside [0, 1] or not
 * finite, the apron's rows included), the outputs and the evaluated state untouched on a
 * refusal, a mask and weights as hq_eval_population_partial composes them on a shard, the
 * getters afterwards (hq_get_indices and hq_get_pixel_errors answer for the owned rows of
 * this rendering; hq_cluster_sums and hq_cluster_errors return HQ_ERR_STATE), and
 * HQ_ARGMIN_DOT in hq_last_path.
 * Measured on one MI355X (profiles/dot_shards_c3.json); more than one GPU has
 * not been run. */
int hq_dot_population_partial(hq_ctx *ctx, const float *palettes, int P, int K,
                              const hq_dot_classes *cls, float strength, double *partial);

/* ---- dot diffusion in one launch: the tiled form ----
 * The reach holds sideways as it holds for rows, and the same argument makes a tile exact: a
 * workgroup that renders a tile together with the window around it -- the tile extended by
 * the reach on each of its four sides, clipped to the image -- produces the whole image's
 * indices on the tile, bit for bit, with the window's errors in LDS and none in global
 * memory.  Classes come from full-image coordinates, W(p)'s border rule from the full image,
 * a source outside the window contributes nothing.  One launch renders every tile of every
 * palette (dot_tile_kernel, hq_dot_tile.hip) in the place of the chain of n*n launches.
 *
 * hq_dot_reach2: hq_dot_reach's recurrence applied to the columns as well:
 *     left[c] = max(left[c], left[p] - dx),  right[c] = max(right[c], right[p] + dx),
 * so *left is the largest number of columns by which a pixel that idx(q) depends on can lie
 * left of q, *right the same to the right; *above and *below are hq_dot_reach's exactly.
 * HQ_DOT_KNUTH8: (5, 5, 5, 5); the row-major 16 x 16 matrix: (15, 1, 255, 17).
 * HQ_ERR_ARG (outputs untouched): an illegal matrix, a null pointer.
 *
 * hq_dot_levels: inside a window the order need not be by class.  A cell's level is 0 when none
 * of its 8 neighbours on the torus has a lower class, else 1 + the largest level among those
 * that have; level[cy*n + cx] receives it (entries past n*n: 0) and *depth the number of
 * levels, 1 + the largest.  Cells of one level do not depend on each other, so a level is one
 * parallel step and a barrier separates two; every pixel still adds its sources in ascending
 * class, so the bits are the chain's.  HQ_DOT_KNUTH8 has 15 levels, the row-major 16 x 16
 * matrix 256.  HQ_ERR_ARG (outputs untouched): an illegal matrix, a null pointer.
 *
 * Eligibility (one host-side rule, dot_tile_eligible): a whole image (not a row-block shard:
 * hq_dot_population_partial on a shard keeps the chain), K <= 256, and a matrix whose window
 * holds its errors, 12 bytes per pixel, in 56 KiB of LDS under the tile shape in force:
 *     (tw + left + right) * (th + above + below) * 12 <= 57344.
 * The shapes tw x th are 16 x 16, 32 x 32 and 64 x 32; option "dot_tile_shape" 1, 2 or 3 names
 * one, 0 (default) takes the largest that fits.  Knuth's matrix and every 16 x 16 permutation
 * tried (360 of them; above + below up to 21, left + right up to 20) fit all three; the row-major and column-major 16 x 16
 * matrices fit none.  Whatever is not eligible takes the chain.
 *
 * Option "dot_tile": -1 (default) auto, 0 always the chain, 1 the tiled kernel wherever it is
 * eligible.  The results do not depend on it, bit for bit; hq_last_path reports HQ_ARGMIN_DOT
 * and the profile counts one "dot" launch per pass under either form.  The tiled form sizes no
 * error planes ([P][3][H][W] floats for the chain).
 * Auto takes the tiled kernel for an eligible pass whose tile is 32 x 32 or 64 x 32 (never under
 * "dot_tile_shape" 1), with W * H <= 2^20 and W * H * P * K <= 2^28; anything else takes the
 * chain.  That is the region in which every measured case beat the chain by more than the spread
 * of the chain's own repeated runs in the same process, bounded in pixels and in the product by
 * the largest case measured there.  Measured on one MI355X (DESIGN.md 28,
 * profiles/dot_tile_c3.json; "dot" stage, median of 5, chain against tiled 64 x 32, ms):
 *                              Knuth's 8 x 8            a 16 x 16 permutation
 *                              P = 1         P = 4         P = 1          P = 4
 *     512 x 512,   K = 16    0.359 / 0.071  0.377 / 0.082  1.409 / 0.107  1.451 / 0.121
 *     1024 x 1024, K = 64    0.492 / 0.121  0.628 / 0.347  1.885 / 0.175  2.188 / 0.658
 *     4096 x 4096, K = 256   2.878 / 2.980  7.302 / 11.60  6.271 / 5.590  15.82 / 22.10
 * The first two rows are the region: all 8 cases won, under the 32 x 32 tile too; the 16 x 16
 * tile lost one of them (1024 x 1024, P = 4, Knuth's), so auto does not take it.  At 4096 x 4096,
 * the only larger image measured, the tiled form lost three cases of four, so auto stays on the
 * chain above 2^20 pixels whatever K is.  The rule is a region around 8 measured points, not a
 * measurement of every shape in it: images below 512 x 512, other K at these sizes and other
 * matrices than these two were not timed.
 * The device-resident search under this cost (hq_search_set_dot) at 4096 x 4096, K = 256, P = 4:
 * 8.49 ms per iteration with the chain, 13.40 with the tiled kernel, the plain step
 * 0.551 in the same process.  Not measured: more than one GPU.
 *
 * hq_dot_form: the form the last dot pass enqueued on the context took: *form 0 = none yet,
 * 1 = the chain, 2 = the tiled kernel; *tile_w and *tile_h its tile (0 for the chain), *levels
 * the levels of its matrix.  A refused call leaves the answer as it was.  Any pointer but ctx
 * may be NULL; HQ_ERR_ARG for a null ctx. */
int hq_dot_reach2(const hq_dot_classes *cls, int *above, int *below, int *left, int *right);
int hq_dot_levels(const hq_dot_classes *cls, int32_t level[256], int *depth);
int hq_dot_form(hq_ctx *ctx, int *form, int *tile_w, int *tile_h, int *levels);

/* ---- ordered dithering: libhq's addition, no reference counterpart ----
 * Error diffusion is a serial recurrence (one workgroup per palette); a threshold
 * map gives most of its S-CIELAB gain with every pixel independent, so it lives
 * inside the pruned-grid argmin, runs on row-block shards and can be the objective
 * of a device-resident search.  In the argmin's space, per channel c, every
 * operation one fp32 operation rounded to nearest and none contracted into an fma:
 *     m   = map[(y mod mh) * mw + (x mod mw)]     x, y: the position in the FULL image
 *     t_c = amp[c] * m
 *     v_c = min(max(pix_c + t_c, 0), 1)
 *     idx(x, y) = the first minimum over k of the argmin's distance(v, pal[k])
 * pix is the planar float, or k/255 rebuilt in fp32 from the packed 8-bit copy's
 * byte k -- the two are equal, so both image forms (option "img_u8" 0 / 1) give the
 * same indices.  At amp = (0, 0, 0) the indices, used flags and costs are
 * hq_eval_population's, bit for bit.
 *
 * hq_bayer_map: the Bayer map of side n = 2^log2n, log2n in 0 .. 6 (else HQ_ERR_ARG),
 * host-only.  With L = log2n,
 *     B(x, y) = OR over i < L of (((x ^ y) >> i) & 1) << (2 (L-1-i) + 1)
 *                              | ((y >> i) & 1)       << (2 (L-1-i))
 * a permutation of 0 .. n^2 - 1, and map[y n + x] = (B + 0.5) / n^2 - 0.5, exact in
 * fp32 (n = 2: rows [-0.375, 0.125], [0.375, -0.125]). */
int hq_bayer_map(int log2n, float *map);
/* The context's threshold map, mh rows of mw values: mw and mh each a power of two
 * in 1 .. 64, every value finite and in [-0.5, 0.5], else HQ_ERR_ARG and the map in
 * force stays.  map NULL (mw, mh ignored) restores the default a fresh context has,
 * Bayer 16 x 16.  The map is a property of the context like an option: it does not
 * end the read-back getters' answers, and a search under the ordered cost uses the
 * map in force when an iteration is enqueued. */
int hq_set_dither_map(hq_ctx *ctx, const float *map, int mw, int mh);
/* hq_eval_population with the index images chosen as above: costs[p] = mean dE +
 * delta * #unused of the ordered rendering, from the unchanged cost path (every dE
 * type, filter half-width and cost option); a colour is used when it appears in
 * that index image.  used may be NULL.  K <= 256; option "grid" 0, 16, 32 and 64 all
 * give the same indices.  Row-block shards are served: y is the full-image row, so
 * a shard's indices are the whole image's rows, and with a communicator the call
 * behaves as hq_eval_population does (the collective is the same; more than one
 * rank has not been run).  Afterwards hq_get_indices[32] and hq_get_pixel_errors
 * answer for this rendering, and hq_cluster_sums and hq_cluster_errors return
 * HQ_ERR_STATE until the next hq_eval_population[_partial] (hq_dither_population's
 * rule).
 * HQ_ERR_ARG: P < 1, K < 1, a null palettes, costs or amp, an amp[c] that is not
 * finite or outside [0, 1], a palette channel that is not finite or outside [0, 1].
 * HQ_ERR_STATE: no image set; a row-block shard without a communicator (use the
 * partial form).  HQ_ERR_UNSUPPORTED: K > 256, option "palette_split" or
 * "slice_ranks" > 1, an image pixel that is not finite or outside [0, 1] (the range
 * flag, found on the device once per image).  On any refusal the outputs and the
 * evaluated state are untouched. */
int hq_ordered_population(hq_ctx *ctx, const float *palettes, int P, int K, const float amp[3],
                          float delta, double *costs, int32_t *used);
/* The same without the final division and penalty, in hq_eval_population_partial's
 * layout: the partials of disjoint shards of one image add up to the whole image's. */
int hq_ordered_population_partial(hq_ctx *ctx, const float *palettes, int P, int K,
                                  const float amp[3], double *partial);

/* ---- a pixel mask on the cost: libhq's addition, no reference counterpart ----
 * Every cost above is a mean over all w * h pixels.  A mask restricts what is
 * measured to a region: one byte per pixel of the FULL image, mask[y*w + x],
 * non-zero = the pixel counts (1, 7 and 255 mean the same); N = the number of
 * in-mask pixels of the full image.  With a mask in force:
 *  - the argmin and the stencil are what they are without one.  Index images, the
 *    used flags (a colour is used when it appears in the index image, so the
 *    penalty term is unchanged) and, with option "pixel_err" 1, the stored dE of
 *    every owned pixel, masked-out ones included, keep their bits: a masked-out
 *    pixel's colour is still displayed, and still feeds its neighbours' blur.
 *  - costs[p] = (sum over the in-mask pixels of dE) / N + delta * #unused.  A
 *    masked-out pixel is left out by a select, so its dE may be NaN (dE94's, for
 *    example) without reaching the sum.  hq_eval_population_partial's
 *    partial[p*(1+K)] is the masked sum over the owned rows.  This holds for every
 *    evaluation: plain, partial, dithered, ordered, a search's (host-driven and
 *    device-resident agree bit for bit, as without a mask), hq_refine_population's.
 *  - hq_cluster_sums (and so hq_refine_population's and a hybrid iteration's
 *    k-means move): sums and count over the in-mask owned pixels; a colour without
 *    one has count 0 and keeps its bits; den is unchanged.  The planar form's
 *    range check (HQ_ERR_UNSUPPORTED for a pixel outside [0, 1]) keeps looking at
 *    every owned pixel, masked-out ones included.
 *  - hq_color_histogram: cells over the in-mask owned pixels, so hq_median_cut of
 *    it seeds from the region.
 *  Both use the mask in force when they are called.
 * An all-ones mask gives the unmasked library's outputs bit for bit; no mask set
 * is the unmasked code path itself.  Weights other than 0 / 1: hq_set_weights,
 * below.
 *
 * hq_set_mask: `mask` points at the full image's mask, as hq_set_image_shard's
 * pointers do; a shard keeps its owned rows, every rank passes the same mask, and
 * N is counted here from the full mask.  mask NULL (w, h ignored): no mask, the
 * state of a fresh context.  HQ_ERR_STATE: no image set.  HQ_ERR_ARG: w, h other
 * than the image's, or a mask without a non-zero byte; the mask in force stays.
 * hq_set_image* drops the mask (it belongs to an image); hq_set_filters keeps it.
 * The mask is a property of the context like the dither map: setting it does not
 * end the read-back getters' answers (indices and stored dE do not depend on it).
 * A search uses the mask in force when an iteration is enqueued, so it may change
 * between hq_search_run calls; the errors of the members accepted before are
 * then stale, exactly as after an option change -- nothing is re-evaluated.
 * While a mask is set, HQ_ERR_UNSUPPORTED with outputs and evaluated state
 * untouched: any evaluation or search call under option "palette_split" or
 * "slice_ranks" > 1; hq_cluster_errors and hq_repair_population (a masked error
 * statistic does not exist); hq_search_set_repair(every > 0), and an
 * hq_search_run that would run a repair iteration (*ran = 0, the search not
 * advanced).
 * Option "mask_skip" (default 1): the fast cost kernels launch one workgroup per
 * output tile and palette; with 1 only the tiles that hold an in-mask owned pixel
 * are launched (a list built on the host when the mask, the tile shape or this
 * option has changed), unless "pixel_err" is 1, when every tile stores its
 * pixels' dE.  0: every tile.  The results are the same bit for bit.  The generic
 * cost kernels never skip. */
int hq_set_mask(hq_ctx *ctx, const uint8_t *mask, int w, int h);
/* *n_full = in-mask pixels of the full image (w * h without a mask), *n_owned = of
 * the owned rows, *tiles_run / *tiles_all = output tiles per palette the last
 * evaluation's fast cost pass launched / would launch without a mask (both 0
 * when that evaluation took the generic path or none ran on this image).  Any
 * pointer may be NULL. */
int hq_mask_info(hq_ctx *ctx, int64_t *n_full, int64_t *n_owned, int64_t *tiles_run,
                 int64_t *tiles_all);

/* ---- pixel weights on the cost: libhq's addition, no reference counterpart ----
 * An importance map: one byte per pixel of the FULL image, weights[y*w + x]; the
 * pixel's weight w is the byte's integer value, 0 .. 255, and says how much the
 * pixel's dE matters.  W = the sum of the weights over the full image.  Mask and
 * weights are ONE piece of state: the last of hq_set_mask / hq_set_weights wins,
 * NULL to either clears it, hq_set_image* drops it, hq_set_filters keeps it.  With
 * weights in force everything the mask's block says holds, with these changes:
 *  - the argmin, the stencil, index images, used flags and the stored per-pixel dE
 *    keep their bits, as under a mask.
 *  - costs[p] = (sum over the owned pixels with w > 0 of w * dE) / W + delta *
 *    #unused; hq_eval_population_partial's partial[p*(1+K)] is the weighted sum over
 *    the owned rows.  A pixel of weight 0 is left out by a select, so its NaN stays
 *    out.  The arithmetic, operation by operation: the fast cost kernels add a
 *    pixel to its thread's fp32 partial by one fused multiply-add, part = fma(dE,
 *    (float)w, part), over the pixels in the masked kernels' order; the partials
 *    then go the masked kernels' way (to double, wave sum, fixed point).  The
 *    generic kernels add the exact double product (double)dE * (double)w to their
 *    double partial.  The finished sum is divided by (double)W, exact below 2^53.
 *    Consequences: a weight map of zeros and ones is hq_set_mask of the same map
 *    BIT FOR BIT in every output (fma(e, 1, part) = part + e), and so all ones is
 *    the unmasked library.  A uniform map of value c > 1 is the unweighted cost
 *    within 1e-6 relative, NOT bit for bit: each fma rounds c * dE + part once,
 *    where the unweighted kernel rounds dE + part.
 *    This holds for every evaluation the mask serves: plain, partial, dithered,
 *    ordered, hq_refine_population's, host-driven and device-resident searches
 *    (bit for bit the same search, option "sa_graph" 0 and 1), hybrid iterations,
 *    hq_search_create_from.
 *  - hq_cluster_sums (and hq_refine_population's, a hybrid iteration's and the
 *    device-resident search's k-means move): sums = (sum w*qR, sum w*qG, sum w*qB,
 *    sum w) over the owned pixels of non-zero weight, den and units unchanged, so
 *    hq_centroids_from_sums' sum / (den * count) is the weighted mean.  The planar
 *    form's range check keeps looking at every owned pixel.
 *    den = 255: nothing can overflow (a pixel adds at most 255 * 255; 2^30 pixels
 *    stay below 2^46).  den = 2^32: a pixel adds up to 255 * 2^32, so the sums are
 *    safe exactly while the owned rows' weights sum to LESS THAN 2^31; at or above
 *    that hq_cluster_sums, hq_color_histogram, hq_refine_population (steps > 0) and
 *    the hq_search_run that would run a hybrid iteration return
 *    HQ_ERR_UNSUPPORTED, outputs and state untouched, *ran = 0; the check is made on
 *    the host before anything is enqueued.  This admits a planar 4096 x 4096 image
 *    only up to a mean weight just under 128 (2^31 / 2^24); the packed 8-bit form
 *    has no such limit.
 *  - hq_color_histogram: cells weighted the same way, count = sum w; hq_median_cut
 *    takes such cells unchanged, so the seed follows the weights.
 *  - hq_mask_info's n_full / n_owned count the pixels of non-zero weight;
 *    tiles_run / tiles_all keep their meaning (a tile is live when it holds an
 *    owned pixel of non-zero weight; option "mask_skip" as under a mask).
 * Refused while weights are set, exactly as under a mask (HQ_ERR_UNSUPPORTED,
 * outputs and evaluated state untouched): palette slices ("palette_split",
 * "slice_ranks" > 1); hq_cluster_errors, hq_repair_population,
 * hq_search_set_repair(every > 0) and a run with a repair iteration.  Left out: a
 * weighted error statistic and repair; weights other than bytes; a weight-aware
 * used[]; the JNI / Java binding.
 *
 * hq_set_weights: pointer, shard, argument and error rules are hq_set_mask's
 * (HQ_ERR_STATE without an image; HQ_ERR_ARG for w, h other than the image's or an
 * all-zero map, the state in force kept; NULL clears).  Like the mask it does not
 * end the read-back getters' answers, and a search uses what is in force when an
 * iteration is enqueued. */
int hq_set_weights(hq_ctx *ctx, const uint8_t *weights, int w, int h);
/* *w_full = the sum of the weights over the full image, *w_owned = over the owned
 * rows.  Under a mask or with nothing set every counted pixel weighs 1: these are
 * then hq_mask_info's n_full and n_owned.  Either pointer may be NULL. */
int hq_weights_info(hq_ctx *ctx, int64_t *w_full, int64_t *w_owned);

/* ---- seeding the search from the image: libhq's additions, no reference counterpart ----
 * The reference starts every search from uniform random palettes (SW:40-52).
 * The three entry points below give a start that knows the image: a colour
 * histogram on the device, a median cut of it on the host, and (further down)
 * hq_search_create_from, a search that starts from a given population.
 *
 * hq_color_histogram: cells[2^(3 bits)][4] = (sum R, sum G, sum B, count) of the
 * owned rows of the context's image (halo rows are not counted), exact integers
 * in hq_cluster_sums' units: *den = 255 and byte sums when the argmin reads the
 * packed 8-bit copy of a k/255 image (option "img_u8" 1, the default), else
 * *den = 2^32 and q(v) = RN(v 2^32) per channel value.  The cell of a pixel is
 * (r << 2 bits) | (g << bits) | b, a channel value v having the coordinate
 * min(floor(v 2^bits), 2^bits - 1) -- a power-of-two scaling, exact in fp32; on
 * a k/255 image it equals byte >> (8 - bits), so both forms of one image fill the
 * same cells.  The histograms of disjoint shards of one image add up exactly to
 * the whole image's when their den agree.  bits in 2 .. 6, else HQ_ERR_ARG; no
 * image set: HQ_ERR_STATE; (den 2^32) an owned pixel that is not finite or lies
 * outside [0, 1]: HQ_ERR_UNSUPPORTED, cells and den untouched.  Needs no
 * evaluated population and disturbs none: hq_cluster_sums and hq_get_indices
 * answer after it as before it. */
int hq_color_histogram(hq_ctx *ctx, int bits, int64_t *cells, int64_t *den);
/* A palette of K colours from such a histogram (of one context, or several
 * shards' added up) by median cut.  Host-only, needs no context, deterministic,
 * integer arithmetic until the final means.
 *  - A box is an inclusive range of cell coordinates per axis, always shrunk to
 *    the tight bounds of its non-empty cells.  The first box holds every
 *    non-empty cell; boxes are split until there are K or every box is one cell.
 *  - The box to split is the one with the largest count (e_R^2 + e_G^2 + e_B^2),
 *    e = hi - lo per axis in cells (64-bit integers; 0 exactly for a single
 *    cell), the lowest box index on a tie; along the axis of the largest e, a
 *    tie to R, then G, then B.
 *  - With m[x] the box's counts per coordinate x = lo .. hi of that axis, t is the
 *    smallest x with 2 sum_{x' <= x} m[x'] >= count, then min(t, hi - 1); the
 *    part [lo, t] keeps the box's index, [t + 1, hi] is appended as a new box.
 *  - Colour i < *made (the number of boxes) is the mean of box i's pixels per
 *    channel by hq_centroids_from_sums' rule, .w = 0; colour i >= *made copies
 *    colour i mod *made (an image of fewer non-empty cells than K).
 * HQ_ERR_ARG: K < 1, bits outside 2 .. 6, den other than 255 or 2^32, a negative
 * count, a total count of 0 or above 2^48 (the priority would leave 64 bits). */
int hq_median_cut(const int64_t *cells, int bits, int64_t den, int K, float *palette, int *made);

/* ---- an image pyramid on the device: libhq's additions, no reference counterpart ----
 * Every search runs at the image's full resolution, yet the cost is a blurred dE: it
 * changes little when the image is box-reduced and the filters are designed for the
 * correspondingly lower dpi.  The entry points below make the levels of a
 * coarse-to-fine search: the reduced image without a trip through the host, and the
 * reduced mask or weight map.  hq_search_population (further down) hands a level's
 * population to hq_search_create_from on the next; the policy that chains them is the
 * Python binding's pyramidSearch.  Left out: a sharded source or one on another
 * device, non-integer or anisotropic factors, any filter other than the box, a
 * pyramid inside one context or inside hq_search_run, the JNI / Java binding.
 *
 * hq_reduced_size: *rw = ceil(w / factor), *rh = ceil(h / factor), the size of the
 * reduction of a w x h image.  Host-only.  HQ_ERR_ARG: factor outside 1 .. 16, w or
 * h < 1, a null pointer. */
int hq_reduced_size(int w, int h, int factor, int *rw, int *rh);
/* The reduction of a mask (is_mask != 0: a non-zero byte counts as 255) or a weight map
 * src[h][w] to out[rh][rw], a weight map for hq_set_weights on the reduced image.
 * Host-only, needs no context, integer arithmetic.  Output block (X, Y) covers source
 * columns [f X, min(f X + f, w)) and the rows likewise, n pixels of byte sum S:
 *     out = floor((2 S + n) / (2 n))            (round half up)
 * raised to 1 when any byte of the block is non-zero, so a reduced region never loses
 * a block that held a counted pixel; an all-zero block stays 0.  factor 1 is the
 * identity for weights and 0 / 255 for a mask.  HQ_ERR_ARG: hq_reduced_size's, a null
 * pointer; nothing is written then. */
int hq_reduce_weights(const uint8_t *src, int w, int h, int factor, int is_mask, uint8_t *out);
/* dst receives the box reduction by `factor` of src's image as its whole image, made
 * on the device from the image src holds (nothing is downloaded or uploaded).  dst
 * otherwise behaves as after hq_set_image(dst, reduced, NULL, rw, rh, illum): the
 * record of the last evaluation is dropped (the read-back rule), mask and weights are
 * dropped, LabRef is computed on the device under dst's own filters, and the reduced
 * image goes through the packed-form check.  illum NULL means src's; an illum with a
 * component that is not finite and greater than 0 is HQ_ERR_ARG (hq_set_image's rule),
 * before dst is touched.  Nothing of src
 * changes, what its getters may still read included.  Output pixel (X, Y) is made
 * from the block of hq_reduce_weights, n pixels, in one of two forms, each stated so
 * that numpy restates it bit for bit:
 *  - src holds the packed 8-bit copy of a k/255 image (whatever its option "img_u8"
 *    says): per channel the integer sum s of the block's bytes, the byte
 *    floor((2 s + n) / (2 n)), and dst's plane gets exactly the float k/255 of that
 *    byte, as a host float division makes it.  dst therefore passes the packed check
 *    and keeps the 4-byte argmin path; hq_last_path's `pixels` says which form dst
 *    took.
 *  - otherwise, per channel the fp32 sum of the block in raster order (rows outer,
 *    columns inner), starting from the block's first pixel, every addition rounded to
 *    nearest; then one correctly rounded fp32 division by (float)n.
 * Refusals, dst left exactly as it was: a null dst or src, src == dst: HQ_ERR_ARG;
 * contexts on different devices: HQ_ERR_UNSUPPORTED; src without an image, or src a
 * row-block shard: HQ_ERR_STATE; dst without filters: HQ_ERR_STATE; factor outside
 * 1 .. 16: HQ_ERR_ARG; a reduced width or height below dst's halfSize: HQ_ERR_ARG
 * (hq_set_image's rule).  The message is dst's hq_last_error.  One host thread for
 * the two contexts during the call. */
int hq_set_image_reduced(hq_ctx *dst, hq_ctx *src, int factor, const float *illum);

/* IM:770 quantize(inlineImageRGB, colors): chosen colour per pixel (CL:147-170).
 * used (K ints) may be NULL. */
int hq_quantize(hq_ctx *ctx, const float *rgba4, int64_t n, const float *colors, int K,
                float *out4, int32_t *used);
/* IM:858 computeError(original, quantized, errorImage): mean dE (configured
 * type; HQ_DE_CIEDE2000 is libhq's addition, Sharma, Wu & Dalal 2005: see
 * hq_delta_e) and errImg4 = (255-e)^2/255^2 replicated in .xyz (IM:886-893). */
int hq_compute_error(hq_ctx *ctx, const float *orig4, const float *quant4, int64_t n,
                     float *err_img4, double *mean);

/* RCCL communicator over xGMI for row-block sharded evaluation.
 * Rank 0 calls hq_comm_unique_id and ships the 128 bytes to every rank. */
int hq_comm_unique_id(unsigned char id[128]);
int hq_comm_init(hq_ctx *ctx, int nranks, int rank, const unsigned char id[128]);
/* The ranks of the context's communicator as RCCL reports them (ncclCommCount,
 * ncclCommUserRank); *nranks = 0 and *rank = -1 without one.  bench.py reports
 * it next to its own world size. */
int hq_comm_info(hq_ctx *ctx, int *nranks, int *rank);

/* SWASA parameters (SW:14-28; GUI defaults HQ:192-224). */
typedef struct hq_swasa_params {
    int population;      /* 4    */
    int imax;            /* 5000 */
    int iTc;             /* 20   */
    float delta;         /* 2    */
    float conv_delay;    /* 0.75 */
    float conv_spread;   /* 0.15 */
    float t0;            /* 20   */
    float alpha;         /* 0.9  */
    float s0;            /* 100  */
    float beta;          /* 5.3  */
    int convergence;     /* 1    */
} hq_swasa_params;

void hq_swasa_default_params(hq_swasa_params *p);

/* IM:383-591 findBestQuantization as a resumable search: create() draws the
 * initial population (SW:40-52) with a java.util.Random-compatible generator
 * seeded with `seed`, evaluates it; run() advances up to `iterations` SA
 * iterations (IM:497-568) and reports how many ran; a JNI caller checks its
 * stop flag between run() calls (IM:499). */
int hq_search_create(hq_ctx *ctx, const hq_swasa_params *params, int K, uint64_t seed,
                     hq_search **out);
/* The same search from a given population (libhq's addition): IM:385-493 with
 * the colours replaced.  The 3 K P nextFloat draws of the random population are
 * still made and thrown away, so after creation the generator is where
 * hq_search_create leaves it; `population` ([P][4K], P = params->population) is
 * what gets evaluated, ranked (IM:843-856, the first of equal minima), recorded
 * as best and moved by iteration 1.  Everything after creation is
 * hq_search_create's search: hq_search_set_lloyd, "sa_device", "sa_graph", the
 * communicator paths (every rank passes the same population).  A population
 * equal to the draws is hq_search_create bit for bit; population NULL is
 * hq_search_create itself.  .w is stored as 0.  HQ_ERR_ARG: a channel that is
 * not finite or lies outside [0, 1], where the search keeps its colours
 * (SW:96-98). */
int hq_search_create_from(hq_ctx *ctx, const hq_swasa_params *params, int K, uint64_t seed,
                          const float *population, hq_search **out);
int hq_search_run(hq_search *s, int iterations, int *ran);
int hq_search_best(const hq_search *s, float *colors, double *best_error, int *iteration);
/* The search's current population (libhq's addition; hq_search_best reads its best
 * member only): the P palettes the next iteration moves, in the order the search
 * holds them, colors[P][4K] with .w = 0, and errors[p] (errors may be NULL), each
 * member's error as the accept step holds it (IM:518-545: its own accepted
 * candidate's, or the iteration's minimum after a convergence copy).  After
 * hq_search_create_from it is the given population and its evaluation.  Plain [P][4K]
 * for chunked palettes (K > 256) too, never the padded chunk layout.  A
 * device-resident search copies from its state buffers after a stream synchronise, a
 * host-driven one from its driver; the two agree bit for bit.  A search created from
 * the returned population starts from the returned errors, bit for bit.  The best
 * error is at most min(errors): the best member may have been replaced since. */
int hq_search_population(const hq_search *s, float *colors, double *errors);
void hq_search_destroy(hq_search *s);
/* Hybrid iterations (libhq's addition: Schaefer & Nolle interleave a k-means
 * step with the annealing moves, the reference holds the annealing half only).
 * every = 0 (the default) is the plain search, bit for bit.  With every > 0,
 * iteration ite -- the 1-based count hq_search_best reports, continuing across
 * hq_search_run calls -- is a hybrid iteration when ite % every == 0; the initial
 * population is never refined.  In a hybrid iteration the candidates are drawn
 * as always (SW:91-101, the same random stream, no extra draws); each member's
 * candidate X is then replaced by one k-means update of X -- the assignment is
 * the evaluation's argmin of X, the sums are hq_cluster_sums' (the same den),
 * the update is hq_centroids_from_sums' rule exactly -- and the updated
 * candidate is what is evaluated, accepted or rejected, copied by the
 * convergence step and recorded as best (IM:515-545).
 * Callable any time after hq_search_create, also between runs; it applies to
 * the iterations that follow.  every < 0: HQ_ERR_ARG.  every > 0 on a row-block
 * shard (option "shard_solo" included): HQ_ERR_STATE; with a communicator of
 * more than one rank, "palette_split" or "slice_ranks" > 1: HQ_ERR_UNSUPPORTED;
 * on a device-resident search of K > 256 (chunked palettes):
 * HQ_ERR_UNSUPPORTED -- a host-driven search (option "sa_device" 0) takes every
 * K hq_cluster_sums serves.  The device-resident search (K <= 256) runs a
 * hybrid iteration without a host round trip: an assign-only pass, the sums
 * kernel, the update kernel ("lloyd" in hq_profile_get), then the evaluation.
 * When the sums would be the planar form's (den 2^32) and the image holds a
 * pixel that is not finite or lies outside [0, 1] -- hq_cluster_sums'
 * HQ_ERR_UNSUPPORTED -- the hq_search_run call that would run the first hybrid
 * iteration returns HQ_ERR_UNSUPPORTED with *ran = 0 and the search has not
 * advanced (checked once per image, before anything is enqueued). */
int hq_search_set_lloyd(hq_search *s, int every);
/* Repair iterations (libhq's addition): hq_search_set_lloyd's iteration rule,
 * call times, scope and refusals with a period of its own, and in addition
 * HQ_ERR_UNSUPPORTED on a context of HQ_DE_CIE94 (its costs are NaN on real
 * images).  every = 0 (the default) is the search without them, bit for bit:
 * nothing is enqueued, allocated or written for them.  In a repair iteration
 * the candidates are drawn as always (no extra draws); when the iteration is a
 * hybrid one too the k-means update runs first; then each candidate is
 * evaluated with its error image stored, repaired by hq_cluster_errors' and
 * hq_reseed_unused(max_moves)'s rules, and the repaired candidate is what is
 * evaluated, accepted or rejected, copied by the convergence step and recorded
 * as best.  Pixels without a usable dE (hq_cluster_errors' HQ_ERR_UNSUPPORTED)
 * are simply left out.  Option "pixel_err" stays what the caller set.  The
 * host-driven search (option "sa_device" 0) takes every K; the device-resident
 * one (K <= 256) runs a repair iteration without a host round trip, as one
 * linear chain ("sa_graph" 1 captures it): a full pass that stores the error
 * image -- into the other counter set, like the hybrid iteration's assign-only
 * pass -- the error kernels ("errsum" in hq_profile_get), the reseed kernel
 * ("reseed"), then the evaluation.  Both forms give the same search bit for bit. */
int hq_search_set_repair(hq_search *s, int every, int max_moves);
/* A search whose objective is the ordered rendering (libhq's addition): from this
 * call on every evaluation of the search is hq_ordered_population's at `amp` -- the
 * candidates of the runs that follow and, when no iteration has run yet, the
 * initial population too, which is evaluated and ranked again (IM:490-493; no
 * draws).  amp NULL or zeros is the plain search, bit for bit: nothing extra is
 * enqueued.  Serves the device-resident search ("sa_graph" 1 included: the pass is
 * the plain one with assign's ordered instances) and the host-driven one
 * ("sa_device" 0); the two give the same search bit for bit.  The map in force when
 * an iteration is enqueued is the one used.  HQ_ERR_ARG: an amp[c] that is not
 * finite or outside [0, 1].  HQ_ERR_UNSUPPORTED (non-zero amp): K > 256; a k-means
 * or repair period set -- and hq_search_set_lloyd and hq_search_set_repair refuse a
 * period likewise while it is on; "palette_split" or "slice_ranks" > 1; an image
 * pixel outside [0, 1] (also checked by each hq_search_run, *ran = 0). */
int hq_search_set_ordered(hq_search *s, const float amp[3]);
/* The same for dot diffusion: from now on every evaluation of the search is hq_dot_population's
 * at `strength` under *cls (NULL: HQ_DOT_KNUTH8), in whichever form option "dot_tile" and the
 * eligibility rule give (the results do not depend on the form).  The matrix is latched at the
 * call and is the search's own: every hq_search_run puts its tables in place before anything is
 * enqueued, so an hq_dot_population call with another matrix between two runs changes nothing.
 * Strength 0 turns it off: the search is then the plain search bit for bit.  Before the first
 * iteration the initial population is re-ranked under the new evaluation; afterwards the change
 * takes effect from the next iteration.  Device-resident (also with "sa_graph" 1) and
 * host-driven searches give the same results bit for bit.  Fixed colours, hq_search_create_from,
 * a mask and weights compose as for the plain search (the rendering does not read the mask, the
 * cost does).  HQ_ERR_ARG: a null search, an illegal matrix, a strength outside [0, 1] or NaN.
 * HQ_ERR_UNSUPPORTED: hybrid or repair iterations set (and hq_search_set_lloyd /
 * hq_search_set_repair under this cost), an ordered cost in force (and hq_search_set_ordered
 * under this one: one rendering per search), K > 256, an image pixel outside [0, 1] or not
 * finite; a sharded context, a communicator of more than one rank and a palette slice get
 * hq_dot_population's answers.  A refused call leaves the search as it was. */
int hq_search_set_dot(hq_search *s, const hq_dot_classes *cls, float strength);

/* Host-only SWASA driver with a caller-supplied population evaluator; same
 * policy code as hq_search_*.  Used to test the SA semantics without a GPU.
 * eval(user, palettes[P*K*4], P, K, costs[P]) returns 0 on success.
 * trace (optional) receives per iteration: best_error then the P errors. */
typedef int (*hq_eval_fn)(void *user, const float *palettes, int P, int K, double *costs);
int hq_swasa_search_host(const hq_swasa_params *params, int K, uint64_t seed, int iterations,
                         hq_eval_fn eval, void *user, float *best_colors, double *best_error,
                         double *trace);
/* The same with hybrid iterations (hq_search_set_lloyd's semantics, the same
 * driver code as a host-driven hq_search_*): on iteration ite with
 * ite % every == 0, refine(user, palettes[P*K*4], P, K) updates the candidates
 * in place between their generation and their evaluation; it returns 0 on
 * success, any other value ends the search and is returned as is.  every = 0
 * or a NULL refine is hq_swasa_search_host bit for bit; every < 0: HQ_ERR_ARG. */
typedef int (*hq_refine_fn)(void *user, float *palettes, int P, int K);
int hq_swasa_search_host_lloyd(const hq_swasa_params *params, int K, uint64_t seed, int iterations,
                               hq_eval_fn eval, hq_refine_fn refine, int every, void *user,
                               float *best_colors, double *best_error, double *trace);
/* The same from a given population (hq_search_create_from's semantics, the same
 * driver code as a host-driven search): population [P][4K] or NULL, which is
 * hq_swasa_search_host_lloyd.  HQ_ERR_ARG: a channel that is not finite or lies
 * outside [0, 1], a null eval. */
int hq_swasa_search_host_from(const hq_swasa_params *params, int K, uint64_t seed, int iterations,
                              hq_eval_fn eval, hq_refine_fn refine, int every,
                              const float *population, void *user,
                              float *best_colors, double *best_error, double *trace);

/* ---- fixed palette colours: libhq's addition, no reference counterpart ----
 * "These colours are given, optimise the others": the first n colours of every
 * palette are fixed, and no move of a search or a polish changes them.  (No other
 * placement: a caller orders the palette.)
 *
 * hq_set_fixed_colors: colors [n][4], .w ignored and stored as 0.  n = 0 or
 * colors NULL clears them, the state of a fresh context.  HQ_ERR_ARG: n < 0,
 * n > 16384, a channel that is not finite or lies outside [0, 1]; the colours in
 * force stay.  A property of the context like the threshold map: hq_set_image*,
 * hq_set_filters, hq_set_mask and hq_set_weights keep it, and setting it does not
 * end the read-back getters' answers.  hq_fixed_colors reads it back: *n (n may be
 * NULL) and, colors not NULL, its [n][4] floats.
 *
 * A search: hq_search_create[_from] reads the context's fixed colours once and
 * keeps that n and those values for its life; a later hq_set_fixed_colors does not
 * reach it.  n > K: HQ_ERR_ARG.  The random population's 3 K P draws are made as
 * always (or the given population replaces them); then colours 0 .. n-1 of every
 * member are overwritten with the fixed colours, and that population is what is
 * evaluated, ranked and recorded as best.  In every iteration the candidates'
 * draws are made exactly as without fixed colours -- the same stream at the same
 * positions -- and for k < n the draw is discarded: the candidate's colour k is
 * the member's colour k, its bits.  Acceptance, best and the convergence copy move
 * whole members, whose first n colours are all the same.  Chunked palettes
 * (K > 256): with n > 0 the chunk padding, copies of candidate colour 0, is the
 * member's colour 0 itself.  A hybrid iteration's k-means update leaves colours
 * k < n alone whatever their count; a repair iteration's rule is
 * hq_reseed_unused_fixed with the search's n, so an unused fixed colour stays
 * where it is and keeps paying delta -- the cost's definition does not change.
 * It composes with what a search composes with ("sa_device" 0 / 1, "sa_graph",
 * hq_search_set_lloyd, _repair and _ordered under their own refusals, mask and
 * weights, a communicator or row-block shards where every rank sets the same
 * colours); the device-resident and the host-driven search agree bit for bit.
 *
 * The polishes: hq_refine_population and hq_repair_population read the context's n
 * when called (the values are not used) and never change colours 0 .. n-1 of the
 * palettes they are given, in any step or in the kept-best copy; n > K:
 * HQ_ERR_ARG.  Everything else -- hq_eval_population*, the ditherings,
 * hq_cluster_sums, hq_cluster_errors, hq_centroids_from_sums, hq_reseed_unused,
 * the histogram, the median cut -- does not look at the fixed colours, and with
 * none set every output of the library is what it was without this section.
 * Left out: a seed that takes the fixed colours into account, a delta that exempts
 * them, fixed colours at arbitrary indices, quantised channel depth. */
int hq_set_fixed_colors(hq_ctx *ctx, const float *colors, int n);
int hq_fixed_colors(hq_ctx *ctx, int *n, float *colors);
/* hq_swasa_search_host_from under fixed colours (the semantics above, the same
 * driver code as a host-driven hq_search_*): fixed_colors [nfixed][4] overwrite
 * the first nfixed colours of every member at the start; fixed_colors NULL with
 * nfixed > 0 means the first nfixed colours of the population, or of the draws,
 * are the fixed ones as they stand.  All 3 K draws per member are still made in
 * every iteration.  The driver itself puts the fixed colours back after `refine`
 * returns, so a refine callback need not know about them.  nfixed = 0 is
 * hq_swasa_search_host_from bit for bit.  HQ_ERR_ARG in addition: nfixed < 0,
 * nfixed > K, a fixed channel that is not finite or lies outside [0, 1]. */
int hq_swasa_search_host_fixed(const hq_swasa_params *params, int K, uint64_t seed, int iterations,
                               hq_eval_fn eval, hq_refine_fn refine, int every,
                               const float *population, const float *fixed_colors, int nfixed,
                               void *user, float *best_colors, double *best_error, double *trace);

/* Kernel timing of the dominant kernels, measured with HIP events on the
 * context stream while enabled (bench.py roofline). */
int hq_profile_enable(hq_ctx *ctx, int on);
/* names: "assign", "cost", "grid", "finalize", "sa_step" (device-resident search), "comm" (the
 * per-evaluation RCCL all-reduce or all-gather, with a communicator), "centroid"
 * (hq_cluster_sums' kernel), "lloyd" (the update kernel of a device-resident
 * hybrid iteration, whose assign-only pass and sums kernel count under "grid",
 * "assign" and "centroid"), "hist" (hq_color_histogram's kernel), "errsum" (hq_cluster_errors'
 * kernels: the statistics and the gather of the worst pixels' colours), "reseed" (the reseed
 * kernel of a device-resident repair iteration, whose error pass counts under "grid", "assign"
 * and "cost"), "dither" (hq_dither_population's and hq_diffuse_population's kernels, which stand in the place of "grid"
 * and "assign": a dithered evaluation counts nothing under those; an ordered evaluation's grid
 * and argmin count under "grid" and "assign" like the plain one's), "reduce" (hq_set_image_reduced's
 * kernel, on the destination context), "dot" (hq_dot_population's launches, one per class or the
 * tiled form's one, in the place of "grid" and "assign": the time from the first one's start to
 * the last one's end, counted as one launch per call), "coords" (option "assign_space" 1: the
 * kernel that makes the pixels' argmin coordinates, once per image and illuminant, in front of
 * the evaluation that first needs them); returns total ms and launch
 * count (HIP events on the context stream). */
int hq_profile_get(hq_ctx *ctx, const char *kernel, double *total_ms, int64_t *launches);
int hq_profile_reset(hq_ctx *ctx);

/* ---- the kernel path of the last pass (test surface): libhq's addition ----
 * Nearly every fall-back of the dispatcher gives the same results, often bit for
 * bit, so results cannot tell which kernels produced them.  hq_last_path reports
 * it: the record of the last pass enqueued on the context -- an evaluation's, a
 * rendering's, the last one of hq_refine_population, hq_repair_population or an
 * hq_search_create / hq_search_run (host-driven or device-resident).  It is
 * written on the host where each launch is chosen; no kernel knows of it.
 * The caller sets info->size = sizeof(hq_path_info); at most that many bytes are
 * filled (the struct may grow at its end) and size is set to the bytes filled.
 * Before the first pass: sequence 0 and every kind 0 ("none").  A call refused
 * before it enqueues anything (HQ_ERR_ARG, HQ_ERR_STATE, HQ_ERR_UNSUPPORTED)
 * leaves the record as it was.  HQ_ERR_ARG: a null pointer, size < 4. */
enum hq_path_pass { HQ_PASS_NONE = 0, HQ_PASS_FULL = 1, HQ_PASS_ASSIGN_ONLY = 2, HQ_PASS_DITHER = 3 };
enum hq_path_pixels { HQ_PIXELS_NONE = 0, HQ_PIXELS_U8 = 1, HQ_PIXELS_PLANAR = 2 };
enum hq_path_grid { HQ_GRID_NONE = 0, HQ_GRID_BUILD_GRID = 1, HQ_GRID_LISTS16 = 2 };
enum hq_path_argmin {
    HQ_ARGMIN_NONE = 0, HQ_ARGMIN_ASSIGN_PIPE = 1, HQ_ARGMIN_ASSIGN_PIPE_ORDERED = 2, HQ_ARGMIN_ASSIGN16 = 3,
    HQ_ARGMIN_ASSIGN_WIDE = 4, HQ_ARGMIN_DITHER = 5,
    HQ_ARGMIN_DIFFUSE = 6,   /* hq_diffuse_population's kernels (hq_diffuse.hip) */
    HQ_ARGMIN_DOT = 7        /* hq_dot_population's kernels: hq_dot.hip, one launch per class, or
                              * hq_dot_tile.hip, one launch (hq_dot_form says which) */
};
enum hq_path_cost {
    HQ_COST_NONE = 0,        /* an assign-only pass, or a mask without a live tile */
    HQ_COST_16W = 1,         /* cost16w_kernel: 16-row tiles */
    HQ_COST_MFMA = 2,        /* cost_mfma_kernel: 8 x 108 tiles */
    HQ_COST_TILED_GENERIC = 3,
    HQ_COST_PIXEL_GENERIC = 4 /* option "cost_variant" 2 */
};
enum hq_path_instance { HQ_INSTANCE_PLAIN = 0, HQ_INSTANCE_MASKED = 1, HQ_INSTANCE_WEIGHTED = 2 };
enum hq_path_gen_h { HQ_GENH_NONE = 0, HQ_GENH_HPASS = 1, HQ_GENH_HROW = 2, HQ_GENH_HROW4 = 3, HQ_GENH_HMFMA = 4 };
enum hq_path_gen_v { HQ_GENV_NONE = 0, HQ_GENV_VPASS = 1, HQ_GENV_VTILE = 2, HQ_GENV_VTILE2 = 3, HQ_GENV_VMFMA = 4 };
/* why the cost did not take the fast kernels: one bit per reason, 0 on the fast path */
enum hq_path_why {
    HQ_WHY_HALF = 1,         /* halfSize above 24: no tap bucket */
    HQ_WHY_VARIANT = 2,      /* option "cost_variant" 1 or 2 */
    HQ_WHY_PALETTE = 4,      /* a palette channel outside [-32, 1.9] or not finite */
    HQ_WHY_TAPS = 8,         /* a tap outside the split-f16 range (hq_set_filters) */
    HQ_WHY_CHUNK_FORM = 16,  /* chunked palette at a bucket or tile form without a chunked kernel */
    HQ_WHY_NCH = 32,         /* more than 32 chunks (K > 8192) */
    HQ_WHY_WIDE = 64         /* the exhaustive 32-bit path: K > 16384, "chunked" 0, "grid" 0, HQ_WHY_PALETTE */
};
typedef struct hq_path_info {
    int32_t size;            /* in: sizeof(hq_path_info); out: the bytes filled */
    int32_t pass;            /* hq_path_pass; a repair iteration's cost-only pass counts as full */
    int64_t sequence;        /* passes enqueued on this context since hq_create */
    int32_t ordered;         /* the argmin is the ordered-dithering one */
    int32_t P, K, nch;       /* this device's palettes, colours, chunks per palette */
    int32_t idx_bytes;       /* index width: 1, 2 or 4 */
    int32_t pixels;          /* hq_path_pixels: what the argmin reads */
    int32_t grid;            /* hq_path_grid */
    int32_t argmin;          /* hq_path_argmin */
    int32_t argmin_cmb;      /* assign_pipe: chunks combined per launch (1, 2 or 4) */
    int32_t argmin_passes;   /* assign_pipe: launches over the chunk groups (nch / 4 above 4 chunks, else 1) */
    int32_t cost;            /* hq_path_cost */
    int32_t cost_hb, cost_de, cost_trim, cost_waves, cost_nch; /* the fast kernels' template tuple */
    int32_t cost_instance;   /* hq_path_instance (fast and generic kernels alike) */
    int32_t gen_h;           /* hq_path_gen_h */
    int32_t gen_h_outputs;   /* gen_hrow4: outputs per thread, 4 or 8 */
    int32_t gen_h_split;     /* gen_hrow4: writes the split-f16 planes (feeds gen_vmfma) */
    int32_t gen_h_rpt;       /* gen_hmfma: 16-row tiles per workgroup */
    int32_t gen_v;           /* hq_path_gen_v */
    int32_t gen_v_rows;      /* gen_vmfma: rows per tile, 64 or 128 */
    uint32_t why_not_fast;   /* hq_path_why bits */
    int32_t previous_pass;   /* hq_path_pass of the pass before this one (sequence - 1) ... */
    int32_t previous_cost;   /* ... and its hq_path_cost: a hybrid iteration is assign-only, then full */
    int64_t tiles_run, tiles_all; /* hq_mask_info's, of this pass (0: not a fast cost launch) */
    int32_t diffuse_rows;    /* HQ_ARGMIN_DIFFUSE: R of the instance (hq_diffusion_classify), else 0 */
    int32_t diffuse_slope;   /* HQ_ARGMIN_DIFFUSE: S of the instance, else 0 */
} hq_path_info;
int hq_last_path(hq_ctx *ctx, hq_path_info *info);
/* *device_resident = 1 when the search's iterations run on the device, 0 when the
 * host-driven driver makes one evaluation call each (option "sa_device" 0, a
 * population above 64 palettes or 512 sub-palettes, K > 16384, "chunked" 0 or
 * "grid" 0 at K > 256); *nch = its chunks per palette (1 when host-driven: each of
 * its evaluations chooses its own); *graph = 1 when the last hq_search_run's
 * kernels went into a hipGraph and were replayed (option "sa_graph" 1 on a
 * device-resident search without profiling; 0 before the first run).  Any pointer
 * may be NULL. */
int hq_search_info(const hq_search *s, int *device_resident, int *nch, int *graph);

/* Tuning knobs (testing / benchmarking; defaults are the measured best).  They
 * may change between calls, also between hq_search_run calls of one search:
 * every evaluation sizes the context's work buffers for the options and image
 * in force when it is enqueued.
 *   "grid"         argmin pruning resolution G2: 0 = exhaustive, 16, 32 (default), 64
 *   "cost_variant" 0 = fast tiled path (default; filters up to halfSize 24), 1 = generic
 *                  two-pass path, LDS-tiled (any filter length; halfSize > 24 takes it),
 *                  2 = the generic pair per pixel in the reference's summation order
 *   "gen_hrow4"    the LDS-tiled generic path's horizontal pass: 1 (default) = 4 adjacent
 *                  outputs per thread over a sliding window, 0 = one output per thread
 *                  (same planes bit for bit)
 *   "gen_vmfma"    the LDS-tiled generic path's vertical pass (halfSize <= 64) on the matrix
 *                  cores in split f16 (as the fast path's; default 1), 0 = fp32 FMAs (gen_vtile2)
 *   "gen_hmfma"    with gen_vmfma: the horizontal pass on the matrix cores too (default 1;
 *                  palettes in the fast range), 0 = fp32 FMAs (gen_hrow4)
 *   "gen_tile_shape" the matrix-core generic pair's workgroup shapes: 0 (default) by grid size
 *                  (4 row tiles per gen_hmfma workgroup and 128-row gen_vmfma tiles on large
 *                  images), 1 the short forms, 2 the tall forms (same results within the split bars)
 *   "lists16"      chunked palettes: native 16-bit candidate lists (one grid over all K
 *                  colours, one lookup per pixel): 1 (default) for 4 to 32 chunks (512 < K
 *                  <= 8192), 2 for 2 .. 32 chunks, 0 = a grid and assign pass per chunk
 *   "gen_vtile2"   the LDS-tiled generic path's vertical pass (halfSize <= 64): 1 (default) =
 *                  32 x 64 tiles, windows double-buffered by LDS DMA; 0 = 64 x 64 tiles with
 *                  one window at a time (same results bit for bit)
 *   "cost_rows"    fast path tiles: 16 (16 x 128 outputs, default) or 8 (8 x 108)
 *   "cost_tw"      16-row tiles at the default filter width: 128 columns (4 waves,
 *                  default) or 256 (8 waves per workgroup)
 *   "trim"         1 = skip the narrow k1 filters' taps below 1e-9 of their peak
 *                  (default; only when the filters allow it), 0 = all taps
 *   "assign_blocks_per_cu" workgroups per CU of the assign grid (0 = default: one
 *                  resident round, at least 6 pixels per thread)
 *   "img_u8"       1 (default) = assign reads the packed 8-bit copy of an image whose
 *                  channels are all k/255; 0 = the planar floats
 *   "sa_device"    hq_search_*: 1 (default) = the SWASA iterations run on the device
 *                  (accept/generate kernel, no host round trip per iteration; needs
 *                  population <= 64), 0 = host-driven, one evaluation call each
 *   "sa_graph"     hq_search_*: 1 = each run's kernels captured into one hipGraph and
 *                  replayed (0, default: measured slower, 0.540 against 0.528 ms per C3 step)
 *   "shard_solo"   experiment only: let a row-block shard run hq_search_* without a
 *                  communicator (its own partial costs; per-rank timing at N GPUs)
 *   "pixel_err"    1 = the cost kernels also write the per-pixel dE (hq_get_pixel_errors, the
 *                  test surface; hq_cluster_errors reads it; hq_repair_population and repair
 *                  iterations set it for their own passes and put the caller's value back)
 *   "dither_rows"  hq_dither_population: rows per strip of the dither kernel, a multiple of 64
 *                  in 64 .. 1024 (default 1024; anything else is HQ_ERR_ARG).  The results do
 *                  not depend on it, bit for bit: it lets small test images cross strips
 *   "dot_apron"    rows (0 .. 255, default 0; anything else is HQ_ERR_ARG) a row-block shard keeps
 *                  beyond its extended rows on each side for hq_dot_population_partial; read by
 *                  hq_set_image_shard and hq_set_image_planar_shard (hq_dot_apron)
 *   "dot_tile"     hq_dot_population[_partial] on a whole image: -1 (default) = the tiled kernel where
 *                  it was measured faster (a 32 x 32 or 64 x 32 tile, W * H <= 2^20, W * H * P * K <= 2^28), 0 = the chain of one launch
 *                  per class, 1 = the tiled kernel wherever it is eligible (hq_dot_form; anything
 *                  else is HQ_ERR_ARG).  The results do not depend on it, bit for bit
 *   "dot_tile_shape" the tiled kernel's tile: 0 (default) = the largest of 16 x 16, 32 x 32 and
 *                  64 x 32 whose window fits, 1, 2, 3 = that one (anything else is HQ_ERR_ARG).  The
 *                  results do not depend on it, bit for bit: 1 lets small test images cross tiles
 *   "cent_span"    test only: pixels per workgroup of the k-means sums kernel (0, default: by
 *                  the grid), rounded up to whole steps of 1024 and clamped to the bound of the
 *                  kernel's accumulator fields.  The results do not depend on it, bit for bit:
 *                  it lets small test images reach that bound
 *   "mask_skip"    under a pixel mask (hq_set_mask) or weights: 1 (default) = the fast cost kernels launch
 *                  only the tiles that hold an in-mask owned pixel (every tile with "pixel_err"
 *                  1); 0 = every tile.  The results do not depend on it, bit for bit
 *   "palette_split" 1 = with a communicator of N ranks, each holding the whole image
 *                  (hq_set_image): rank r evaluates palettes [r P/N, (r+1) P/N) and one
 *                  all-gather gives every rank all P results (SURVEY 8e's split of large
 *                  populations; P must divide by N); 0 (default) = row-block shards
 *   "slice_ranks", "slice_rank"  test only: the same palette slice without a
 *                  communicator (hq_eval_population_partial: other rows read 0)
 *
 * Not a tuning knob, since it changes what is computed:
 *   "assign_space" the space in which a pixel's nearest palette colour is found: 0 (default) =
 *                  sRGB, the reference's rule (CL:172-199), every output and launch what it was;
 *                  1 = CIELAB under the context's illuminant (libhq's own addition); anything else
 *                  is HQ_ERR_ARG.  Under 1 a colour (R, G, B) has the coordinates (L, a + 128,
 *                  b + 128) / 256 of its unfiltered CIELAB (hq_assign_coords), whose Euclidean
 *                  distance is dE76 / 256, and the same exact argmin kernels run on the pixels'
 *                  and the palettes' coordinates in their planar form (hq_last_path reports
 *                  HQ_PIXELS_PLANAR); the index images, used flags and costs are that
 *                  assignment's.  The stencil cost, the k-means sums, the error statistics, the
 *                  repair rule and the histogram read colours as before, so a k-means or repair
 *                  move works from the CIELAB assignment and stays in RGB.  The pixels'
 *                  coordinates are made on the device before the next evaluation that needs them
 *                  and again after a new image or illuminant (hq_set_image*, hq_set_image_reduced).
 *                  Under D65 and D50 the whole sRGB cube lands inside [0, 1]^3; under illuminant A
 *                  saturated blues do not (b < -128), and such pixels take the argmin's exact
 *                  reference loop for pixels outside the cube: correct and slow.  The coordinates
 *                  are not rescaled per illuminant.  The sRGB gamut fills about 7 % of the coordinate cube,
 *                  so a palette's candidate lists are as long as those of one 14 times as large under 0:
 *                  at K = 256 set "grid" 64 with it (at C3 the argmin takes 0.20 ms there against 2.26 ms
 *                  under the default 32, where most pixels fall back to the exhaustive loop).
 *                  Served under 1: hq_eval_population[_partial] (row-block shards, a communicator),
 *                  every cost path, dE type, mask and weights, "grid" 0 .. 64, K <= 16384 on the
 *                  chunked path, hq_cluster_sums, hq_cluster_errors, hq_refine_population,
 *                  hq_repair_population, fixed colours, hq_search_* (a search latches the value at
 *                  hq_search_create*; hq_search_run under another value is HQ_ERR_STATE, ran = 0).
 *                  HQ_ERR_UNSUPPORTED under 1: K > 256 off the chunked path (K > 16384, "chunked" 0,
 *                  "grid" 0, a palette outside the fast range), hq_dither_population,
 *                  hq_diffuse_population, hq_dot_population[_partial],
 *                  hq_ordered_population[_partial], hq_search_set_ordered and hq_search_set_dot with
 *                  a non-zero parameter.  hq_quantize keeps the reference's sRGB rule (CL:147-170)
 *                  whatever the option says. */
int hq_set_option(hq_ctx *ctx, const char *name, int value);

/* The argmin coordinates of n colours (rgba4, n x 4 floats) in space `space` (option
 * "assign_space"'s values) under the context's illuminant, by the device function the
 * evaluation itself uses; out4 is n x 4 floats, .w = 0.  space 0 copies R, G, B.  A null
 * pointer, n < 1 or another space: HQ_ERR_ARG. */
int hq_assign_coords(hq_ctx *ctx, int space, const float *rgba4, int64_t n, float *out4);

#ifdef __cplusplus
}
#endif
#endif /* HQ_H */
