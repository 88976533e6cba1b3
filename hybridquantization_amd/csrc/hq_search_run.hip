// hq_search_run.hip -- libhq host runtime, the search: the device-resident SWASA
// run (its SA steps, hybrid and repair iterations, the optional graph capture) and
// the hq_search_* entry points, host-driven searches among them.  The kernels:
// hq_search.hip; shared declarations: hq_runtime.h.
#include "hq_runtime.h"

using namespace hq;

namespace {

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
    a.n_total = cost_divisor(c);  // (a pixel mask: its pixels in the full image)
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
    a.nfixed = random ? 0 : s->nfixed;  // (the random population's draws are all kept: create overwrites after them)
    a.acc = acc_base(c, c->acc_par, a.P);
    a.used_glob = used_base(c, c->acc_par, a.P * s->nch);
    a.used_stride = used_stride(a.P * s->nch);
    a.fold = s->fold;
    a.nranks = rank_blocks(c);
    a.acc_rank_words = (int64_t)acc_words(a.P);
    return a;
}

// One sa_step launch (sa_args).
int enqueue_sa_step(hq_search* s, bool accept, bool init, bool generate, bool random, float amax, ProfRec& pr) {
    hq_ctx* c = s->ctx;
    const SaArgs a = sa_args(s, accept, init, generate, random, amax);
    HIP_TRY(c, timed_launch(pr, kPSaStep, [&] { return launch_sa_step(a, c->stream); }));
    s->st = 1 - s->st;
    if (generate) s->cd = 1 - s->cd;
    return HQ_OK;
}

// What a hybrid or a repair iteration of a device-resident search needs beyond the whole image.
int device_move_scope(hq_search* s, const char* what) {
    if (!s->driver && s->nch > 1)
        return fail(s->ctx, HQ_ERR_UNSUPPORTED, "%s of a device-resident search need K <= %d (K = %d): "
                                                "set option sa_device 0 before hq_search_create", what, kMaxK, s->K);
    return HQ_OK;
}

// ---- hybrid iterations (hq_search_set_lloyd) -----------------------------------
// The scope of a k-means move is hq_refine_population's: the whole image on
// this context, every palette's index image here.
int lloyd_scope(hq_search* s) {
    if (int rc = whole_image_only(s->ctx, "hybrid iterations")) return rc;
    return device_move_scope(s, "hybrid iterations");
}

// A run of `iterations` from iteration `ite` (the last one done) holds an iteration
// that is a multiple of `every`.
bool period_in_run(const hq_search* s, int every, int ite, int iterations) {
    if (every <= 0) return false;
    const int last = (int)std::min<int64_t>((int64_t)ite + iterations, s->prm.imax);
    return last / every > ite / every;
}

// ---- repair iterations (hq_search_set_repair) ----------------------------------
// hq_repair_population's scope, and a dE type whose costs are numbers.
int repair_scope(hq_search* s) {
    hq_ctx* c = s->ctx;
    if (c->mask_on)  // (a masked error statistic does not exist: hq_cluster_errors' refusal)
        return fail(c, HQ_ERR_UNSUPPORTED, "repair iterations under %s (%s)", mask_noun(c), mask_call(c));
    if (c->de_type == HQ_DE_CIE94)
        return fail(c, HQ_ERR_UNSUPPORTED, "repair iterations on a dE94 context: its costs are NaN on real images");
    if (int rc = whole_image_only(c, "repair iterations")) return rc;
    if (int rc = device_move_scope(s, "repair iterations")) return rc;
    if (c->have_image && (int64_t)c->g.W * c->g.H >= ((int64_t)1 << 32))
        return fail(c, HQ_ERR_UNSUPPORTED, "image of 2^32 pixels or more: a position does not fit 32 bits");
    return HQ_OK;
}

int lloyd_validate(hq_search* s) {
    hq_ctx* c = s->ctx;
    if (!c->have_image) return fail(c, HQ_ERR_STATE, "no image set (hq_set_image)");
    if (int rc = weighted_sums_scope(c, "hybrid iterations")) return rc;
    return sums_u8(c) ? HQ_OK : require_unit_range_image(c, "planar image", "no exact sums, no hybrid iteration");
}

// The k-means move of a device-resident hybrid iteration, after the sa_step that
// generated and prepared the candidates (now cand[cd]): the assign-only pass,
// the sums kernel into d_sums (zero on entry: the run's memset, then the update
// kernel's own zeroing) and the update kernel, which prepares the updated
// candidates for the evaluation that follows.  pr: the iteration's events.
int enqueue_lloyd(hq_search* s, ProfRec& pr) {
    hq_ctx* c = s->ctx;
    int rc = enqueue_core(c, s->P, s->K, pr, Pass{Pass::AssignOnly});
    if (rc) return rc;
    int idx_bytes = 1;
    const ClusterArgs ca = cluster_args(c, s->P, s->K, s->nch, &idx_bytes);
    HIP_TRY(c, timed_launch(pr, kPSums, [&] { return launch_cluster_sums(ca, idx_bytes, c->num_cu, c->stream); }));
    const LloydArgs la{ca.sums, s->cand[s->cd].as<float>(), prep_args(c, s->K), s->K, sums_u8(c) ? 1 : 0, s->nfixed};
    HIP_TRY(c, timed_launch(pr, kPLloydUpdate, [&] { return launch_lloyd_update(la, s->P, c->stream); }));
    return HQ_OK;
}

// The repair move of a device-resident repair iteration, after the sa_step that
// generated and prepared the candidates (now cand[cd]) and after the k-means move
// when the iteration is hybrid too: a cost pass that stores the error image
// (option "pixel_err" forced on for it alone), the error kernels into d_errstat
// (zero on entry: the run's memset, then the reseed kernel's own zeroing) and
// d_worst, and the reseed kernel, which prepares the repaired candidates for the
// evaluation that follows.  The flag of pixels without a usable dE is not read:
// they are left out, as the host-driven form leaves them out.
int enqueue_repair(hq_search* s, ProfRec& pr) {
    hq_ctx* c = s->ctx;
    int rc;
    {
        const PixelErrScope scope(c);
        rc = enqueue_core(c, s->P, s->K, pr, Pass{Pass::CostOnly});
    }
    if (rc) return rc;
    int idx_bytes = 1;
    const ClusterErrArgs ea = cluster_err_args(c, s->P, s->K, s->nch, &idx_bytes);
    HIP_TRY(c, timed_launch(pr, kPErrsum, [&] { return launch_cluster_errors(ea, idx_bytes, c->num_cu, c->stream); }));
    const ReseedArgs ra{ea.stats, ea.worst, s->cand[s->cd].as<float>(), prep_args(c, s->K), s->K, s->repair_moves,
                        s->nfixed};
    HIP_TRY(c, timed_launch(pr, kPReseed, [&] { return launch_reseed(ra, s->P, c->stream); }));
    return HQ_OK;
}

// The end of hq_search_create*, hq_search_run and hq_search_set_ordered (status rc, so many
// evaluations enqueued).  What the getters may read then (hq.h) is the index images of the
// last candidates evaluated and nothing else: a device-resident search enqueued its passes
// itself (resident_of, under its chunk count), a host-driven one went through
// hq_*_population, whose record becomes a search's.  A failure drops the record; a call that
// evaluated nothing leaves it alone.
void search_commit(hq_search* s, int rc, int evaluations) {
    hq_ctx* c = s->ctx;
    const NchScope scope(c, s->nch);
    if (rc) drop(c);
    else if (evaluations > 0)
        commit(c, s->driver ? c->res.of_search() : resident_of(c, Resident::Search, s->P, s->K));
}

// A search's evaluation pass: folding (search_folds) or full.
// (hq_search_set_ordered: the ordered one at the search's amplitude; hq_search_set_dot: the
// dot-diffused one at the search's strength, under the tables ensure_dot_pass has put in place)
Pass search_pass(const hq_search* s) {
    const Pass::Kind kind = s->fold ? Pass::Fold : Pass::Full;
    if (s->dot) return Pass{s->fold, Dot{s->dot_strength, 0, 0}};  // (a whole image: no window)
    return s->ordered ? Pass{kind, s->ord} : Pass{kind};
}

// A search under the ordered cost moves by annealing alone: a k-means or repair move from a
// dithered assignment is neither (hq_ordered_population's rule for hq_cluster_sums).
int ordered_excludes(hq_search* s, const char* what) {
    if (s->ordered)
        return fail(s->ctx, HQ_ERR_UNSUPPORTED, "%s in a search under the ordered cost (hq_search_set_ordered)", what);
    if (s->dot)
        return fail(s->ctx, HQ_ERR_UNSUPPORTED, "%s in a search under the dot-diffused cost (hq_search_set_dot)", what);
    return HQ_OK;
}

// hq_search_set_ordered before the first iteration: the initial population (still in
// cand[cd], the buffer create's accept step read) through the palette prep, the search's
// pass and the initial accept step again -- IM:490-493 under the evaluation now in force.
// The accept step draws nothing, so the generator stays where create left it.
int device_search_rerank(hq_search* s) {
    hq_ctx* c = s->ctx;
    int rc = bind(c);
    if (rc) return rc;
    if (!c->have_image) return fail(c, HQ_ERR_STATE, "no image set (hq_set_image)");
    const NchScope scope(c, s->nch);
    if ((rc = ensure_population(c, s->P, s->K))) return rc;
    if (s->ordered && (rc = ensure_dither_map(c))) return rc;
    if (s->dot && (rc = ensure_dot_pass(c, s->dot_cls, s->P, s->K))) return rc;
    if (s->nch > 1) return fail(c, HQ_ERR_UNSUPPORTED, "K=%d > %d", s->K, kMaxK);
    if ((rc = upload_and_prep(c, nullptr, s->cand[s->cd].p, s->P, s->K))) return rc;
    ProfRec untimed;
    if ((rc = enqueue_core(c, s->P, s->K, untimed, search_pass(s)))) return rc;
    if ((rc = enqueue_sa_step(s, true, true, false, false, 0.f, untimed))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
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
    drop(c);  // (the search's own evaluation replaces the index images)
    int rc = ensure_population(c, P, K);
    if (rc) return rc;
    const size_t n4 = (size_t)P * 4 * K;
    for (int i = 0; i < 2; ++i) {
        HIP_TRY(c, s->colors[i].ensure(sizeof(float) * n4));
        HIP_TRY(c, s->cand[i].ensure(sizeof(float) * n4));
        HIP_TRY(c, s->err[i].ensure(sizeof(double) * P));
        HIP_TRY(c, s->seed[i].ensure(sizeof(uint64_t)));
        HIP_TRY(c, s->best_err[i].ensure(sizeof(double)));
    }
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
    ProfRec untimed;
    // IM:385-493: random population (SW:40-52), its evaluation, argmin
    if ((rc = enqueue_sa_step(s, false, false, true, true, 0.f, untimed))) return rc;
    // A given population takes the random one's place after that step has drawn it (the seed
    // is past the 3 K P draws as always): into the candidate buffer the accept step reads,
    // and through the palette prep as an evaluation uploads it (upload_and_prep), so the prep's
    // outputs and the duplicate flags are the given colours'.
    // Fixed colours: colours 0 .. nfixed-1 of every member of that population, given or drawn, are
    // overwritten.  The draws are java.util.Random's on either side (SW:40-52), so without a given
    // population the host makes them once more and goes the given population's way.
    std::vector<float> given;  // (.w = 0; read by the copy below until the synchronise)
    if (population || s->nfixed > 0) {
        if (population) {
            given.assign(population, population + n4);
        } else {
            given.resize(n4);
            Swasa draws(*params, seed);
            for (int i = 0; i < P; ++i) draws.generate_random_colors(K, &given[(size_t)i * 4 * K]);
        }
        for (size_t e = 3; e < n4; e += 4) given[e] = 0.0f;
        for (int i = 0; i < P; ++i) std::copy(s->fixed.begin(), s->fixed.end(), &given[(size_t)i * 4 * K]);
        HIP_TRY(c, hipMemcpyAsync(s->cand[s->cd].p, given.data(), sizeof(float) * n4, hipMemcpyHostToDevice,
                                  c->stream));
        if ((rc = upload_and_prep(c, given.data(), nullptr, P, K))) return rc;
    }
    if ((rc = enqueue_core(c, P, K, untimed, search_pass(s)))) return rc;
    if ((rc = enqueue_sa_step(s, true, true, false, false, 0.f, untimed))) return rc;
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
    if (s->ordered && (rc = ensure_dither_map(c))) return rc;  // (before a capture begins)
    // the search's own matrix, whatever hq_dot_population has put there since, and the chain's errors
    if (s->dot && (rc = ensure_dot_pass(c, s->dot_cls, s->P, s->K))) return rc;
    if (s->comm != c->comm || s->fold != search_folds(c))
        return fail(c, HQ_ERR_STATE, "communicator or palette split changed after hq_search_create: "
                                     "recreate the search");
    // profiling: each iteration's events and the pairs it records (events of an earlier run's
    // hybrid or repair iteration may sit in the slots this run does not use)
    const bool prof = c->prof;
    if (prof) HIP_TRY(c, s->pev.ensure((size_t)2 * kPairs * iterations));
    std::vector<ProfRec> recs(prof ? iterations : 0);
    ProfRec untimed;
    // hybrid iterations in this run: the sums buffer before anything is enqueued
    // (no allocation while a run is captured), zeroed once below -- the update
    // kernel leaves it zero for the next hybrid iteration
    const bool lloyd = period_in_run(s, s->every, s->ite, iterations);
    const size_t sums_bytes = sizeof(int64_t) * ((size_t)s->P * s->K * 4 + 1);  // (d_sums' and d_errstat's)
    if (lloyd) HIP_TRY(c, c->d_sums.ensure(sums_bytes));
    // repair iterations in this run: the same for the error image, the statistics and the
    // worst pixels -- nothing of it without one
    const bool repair = period_in_run(s, s->repair_every, s->ite, iterations);
    if (repair) {
        HIP_TRY(c, c->d_pixerr.ensure(sizeof(float) * (size_t)s->P * std::max<int64_t>(n_own(c->g), 1)));
        HIP_TRY(c, c->d_errstat.ensure(sums_bytes));
        HIP_TRY(c, c->d_worst.ensure(sizeof(float) * (size_t)s->P * s->K * 4));
    }
    // option sa_graph: the run's kernels go into one hipGraph (stream capture),
    // replayed as a whole -- a chain of dependent kernels costs ~2.7 us per
    // kernel from the stream and ~1.8 from a graph (profiles/r04_graph_gap_
    // microbench.txt).  The previous run's executable graph is updated in place
    // when the iteration count (the topology) is the same, else instantiated
    // anew.  Not with profiling events (they ride on the launches).
    const bool graph = c->sa_graph && !prof;
    s->graphed = graph;
    if (graph) HIP_TRY(c, hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
    auto abort_capture = [&](int rc0) {
        if (graph) {
            hipGraph_t gr = nullptr;
            if (hipStreamEndCapture(c->stream, &gr) == hipSuccess && gr) (void)hipGraphDestroy(gr);
        }
        return rc0;
    };
    auto zero_table = [&](const DevBuf& b, size_t bytes) {  // (a failure ends the capture)
        const hipError_t e = hipMemsetAsync(b.p, 0, bytes, c->stream);
        if (e != hipSuccess) (void)abort_capture(0);
        return e;
    };
    if (lloyd) HIP_TRY(c, zero_table(c->d_sums, sums_bytes));
    if (repair) HIP_TRY(c, zero_table(c->d_errstat, sums_bytes));
    for (; done < iterations && s->ite < s->prm.imax; ++done) {
        const int ite = ++s->ite;
        s->pol->reduce_temperature_if_necessary(ite);                  // IM:507
        const float amax = s->pol->max_step_width(ite) / 256.0f;       // SW:91-101
        ProfRec& pr = prof ? recs[done] : untimed;
        if (prof) pr.ev = &s->pev.ev[(size_t)2 * kPairs * done];
        // accept the previous iteration's population (none at the first of a run)
        if ((rc = enqueue_sa_step(s, done > 0, false, true, false, amax, pr))) return abort_capture(rc);
        if (s->every > 0 && ite % s->every == 0 && (rc = enqueue_lloyd(s, pr))) return abort_capture(rc);
        if (s->repair_every > 0 && ite % s->repair_every == 0 && (rc = enqueue_repair(s, pr)))
            return abort_capture(rc);
        if ((rc = enqueue_core(c, s->P, s->K, pr, search_pass(s)))) return abort_capture(rc);
        s->t_acc = s->pol->temperature();     // SW:54-57 at this iteration
        s->keep_acc = s->pol->keep_threshold(ite);
    }
    if (done > 0 && (rc = enqueue_sa_step(s, true, false, false, false, 0.f, untimed))) return abort_capture(rc);
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
    for (int i = 0; prof && i < done; ++i) prof_accumulate(c, recs[i]);
    if (ran) *ran = done;
    return HQ_OK;
}

// What a run of `iterations` needs of the context as it is now (the image or an option may
// have changed): a hybrid iteration in it, its scope and the image's validity; a repair
// iteration, its scope; no palette slice under a pixel mask; the ordered cost's scope.
int run_scope(hq_search* s, int iterations) {
    const int ite = s->driver ? s->driver->iteration() : s->ite;
    int rc;
    // the errors a search holds were measured under the argmin rule it was created with
    if (s->assign_space != s->ctx->assign_space)
        return fail(s->ctx, HQ_ERR_STATE, "option assign_space changed after hq_search_create (%d, now %d): "
                                          "recreate the search", s->assign_space, s->ctx->assign_space);
    if (period_in_run(s, s->every, ite, iterations) && ((rc = lloyd_scope(s)) || (rc = lloyd_validate(s)))) return rc;
    if (period_in_run(s, s->repair_every, ite, iterations) && (rc = repair_scope(s))) return rc;
    if ((rc = mask_scope(s->ctx))) return rc;
    if (s->dot) return dot_search_scope(s->ctx, s->K);
    return s->ordered ? ordered_scope(s->ctx, s->K) : HQ_OK;
}

}  // namespace

extern "C" {

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
    if (c->fixed_n > K)
        return fail(c, HQ_ERR_ARG, "%d fixed colours (hq_set_fixed_colors) in palettes of K=%d", c->fixed_n, K);
    if (int rc = mask_scope(c)) return rc;
    // device-resident: K <= 256, or chunked palettes (256 < K <= 16384); at most
    // kSaMaxP palettes (sa_step's per-palette tables) and kSaMaxSub sub-palettes
    // (its fold reads 8 used words per sub-palette, at most 4 per thread)
    const int nch = K > kMaxK && K <= kMaxKChunked && c->chunked && c->G2 > 0 ? chunk_count(K) : 1;
    const bool device = c->sa_device && params->population <= kSaMaxP && params->population * nch <= kSaMaxSub &&
                        (K <= kMaxK || nch > 1);
    hq_search* s = new hq_search{c, nullptr, K};
    s->nfixed = c->fixed_n;  // latched: a later hq_set_fixed_colors does not reach this search
    s->fixed = c->fixed;
    s->assign_space = c->assign_space;  // latched too: hq_search_run refuses another value
    int rc;
    if (device) {
        if (!c->have_image) rc = fail(c, HQ_ERR_STATE, "no image set (hq_set_image)");
        else if (!(rc = bind(c)) && !whole_image(c) && !(c->comm && c->nranks > 1) && !c->shard_solo)
            rc = fail(c, HQ_ERR_STATE, "sharded context without a communicator");
        if (rc) {  // (a refusal: nothing of the context has been touched)
            hq_search_destroy(s);
            return rc;
        }
        s->nch = nch;
        rc = device_search_create(c, params, K, seed, population, s);
    } else {
        const float delta = params->delta;
        auto eval = [c, delta, s](const float* pal, int P, int KK, double* costs) {
            if (s->dot) return hq_dot_population(c, pal, P, KK, &s->dot_cls, s->dot_strength, delta, costs, nullptr);
            return s->ordered ? hq_ordered_population(c, pal, P, KK, s->ord.amp, delta, costs, nullptr)
                              : hq_eval_population(c, pal, P, KK, delta, costs, nullptr);
        };
        s->driver = new SearchDriver(*params, K, seed, eval);
        // the k-means move, host-driven, is the public triple: an evaluation of the
        // candidates for their argmin (its cost pass is wasted), the sums, the update
        s->driver->set_refine([c, delta, s](float* pal, int P, int KK) {
            std::vector<double> costs(P);
            const int rr = hq_eval_population(c, pal, P, KK, delta, costs.data(), nullptr);
            return rr ? rr : kmeans_move(c, P, KK, s->nfixed, pal);
        });
        // the repair move, host-driven: an evaluation of the candidates that stores their
        // error image, the error statistics (pixels with no usable dE left out) and the rule
        s->driver->set_repair([c, delta, s](float* pal, int P, int KK) {
            const PixelErrScope scope(c);
            std::vector<double> costs(P);
            const int rr = hq_eval_population(c, pal, P, KK, delta, costs.data(), nullptr);
            return rr ? rr : repair_move(c, P, KK, s->repair_moves, s->nfixed, true, pal, nullptr);
        });
        s->prm = *params;
        s->P = params->population;
        s->driver->set_fixed(s->nfixed, s->nfixed > 0 ? s->fixed.data() : nullptr);
        rc = s->driver->start(population);
    }
    search_commit(s, rc, 1);
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
    if (s->ctx && (rc = run_scope(s, iterations))) {  // (first, so a refusal leaves the search where it was)
        if (ran) *ran = 0;
        return rc;
    }
    int done = 0;  // (the caller's `ran` is written as before; without one, a count of our own)
    int* const count = ran ? ran : &done;
    if (!s->driver) {
        rc = bind(s->ctx);
        if (!rc) rc = device_search_run(s, iterations, count);
    } else {
        rc = s->driver->run(iterations, count, nullptr);
    }
    if (s->ctx) search_commit(s, rc, rc ? 0 : *count);
    return rc;
}

int hq_search_set_lloyd(hq_search* s, int every) {
    if (!s || !s->ctx) return HQ_ERR_ARG;
    if (every < 0) return fail(s->ctx, HQ_ERR_ARG, "every=%d < 0", every);
    if (every > 0) {
        if (int rc = ordered_excludes(s, "hybrid iterations")) return rc;
        if (int rc = lloyd_scope(s)) return rc;
    }
    s->every = every;
    if (s->driver) s->driver->set_every(every);
    return HQ_OK;
}

int hq_search_set_repair(hq_search* s, int every, int max_moves) {
    if (!s || !s->ctx) return HQ_ERR_ARG;
    if (every < 0) return fail(s->ctx, HQ_ERR_ARG, "every=%d < 0", every);
    if (every > 0) {
        if (int rc = ordered_excludes(s, "repair iterations")) return rc;
        if (int rc = repair_scope(s)) return rc;
    }
    s->repair_every = every;
    s->repair_moves = max_moves;
    if (s->driver) s->driver->set_repair_every(every);
    return HQ_OK;
}

int hq_search_set_ordered(hq_search* s, const float amp[3]) {
    if (!s || !s->ctx) return HQ_ERR_ARG;
    hq_ctx* c = s->ctx;
    const float zeros[3] = {0.f, 0.f, 0.f};
    if (!amp) amp = zeros;
    if (int rc = check_ordered_amp(c, amp)) return rc;
    const bool on = amp[0] != 0.f || amp[1] != 0.f || amp[2] != 0.f;
    if (on) {
        if (s->every > 0 || s->repair_every > 0)
            return fail(c, HQ_ERR_UNSUPPORTED, "a search with hybrid or repair iterations: no ordered cost");
        if (s->dot) return fail(c, HQ_ERR_UNSUPPORTED, "a search under the dot-diffused cost: one rendering per search");
        if (int rc = assign_space_excludes(c, "hq_search_set_ordered")) return rc;
        if (int rc = ordered_scope(c, s->K)) return rc;
    }
    const Ordered old = s->ord;
    if (on == s->ordered && (!on || (amp[0] == old.amp[0] && amp[1] == old.amp[1] && amp[2] == old.amp[2])))
        return HQ_OK;  // (nothing changes: nothing is enqueued)
    const bool was = s->ordered;
    s->ordered = on;
    for (int ch = 0; ch < 3; ++ch) s->ord.amp[ch] = on ? amp[ch] : 0.f;  // (zeros: the plain pass itself)
    const int ite = s->driver ? s->driver->iteration() : s->ite;
    if (ite != 0) return HQ_OK;
    // before the first iteration: the initial population's errors and its best are the new evaluation's
    const int rc = s->driver ? s->driver->rerank() : device_search_rerank(s);
    search_commit(s, rc, 1);
    if (rc) s->ordered = was, s->ord = old;
    return rc;
}

int hq_search_set_dot(hq_search* s, const hq_dot_classes* cls, float strength) {
    if (!s || !s->ctx) return HQ_ERR_ARG;
    hq_ctx* c = s->ctx;
    if (cls && !hq_dot_classes_legal(cls))
        return fail(c, HQ_ERR_ARG, "illegal class matrix: side 4, 8 or 16 and a permutation of 0 .. n*n - 1 (hq.h)");
    if (!(strength >= 0.0f && strength <= 1.0f)) return fail(c, HQ_ERR_ARG, "strength %g not in [0, 1]", strength);
    const bool on = strength != 0.f;
    hq_dot_classes m;
    if (cls) m = *cls;
    else hq_dot_preset(HQ_DOT_KNUTH8, &m);
    if (on) {
        if (s->every > 0 || s->repair_every > 0)
            return fail(c, HQ_ERR_UNSUPPORTED, "a search with hybrid or repair iterations: no dot-diffused cost");
        if (s->ordered) return fail(c, HQ_ERR_UNSUPPORTED, "a search under the ordered cost: one rendering per search");
        if (int rc = assign_space_excludes(c, "hq_search_set_dot")) return rc;
        if (int rc = dot_search_scope(c, s->K)) return rc;
    }
    const bool same_matrix = s->dot_cls.n == m.n && !std::memcmp(s->dot_cls.cls, m.cls, sizeof(int32_t) * m.n * m.n);
    if (on == s->dot && (!on || (strength == s->dot_strength && same_matrix))) return HQ_OK;  // (nothing changes)
    const bool was = s->dot;
    const float old_strength = s->dot_strength;
    const hq_dot_classes old_cls = s->dot_cls;
    s->dot = on;
    s->dot_strength = on ? strength : 0.f;  // (off: the plain pass itself)
    if (on) {
        std::memset(&s->dot_cls, 0, sizeof s->dot_cls);
        s->dot_cls.n = m.n;
        std::memcpy(s->dot_cls.cls, m.cls, sizeof(int32_t) * m.n * m.n);
    }
    const int ite = s->driver ? s->driver->iteration() : s->ite;
    if (ite != 0) return HQ_OK;
    // before the first iteration: the initial population's errors and its best are the new evaluation's
    const int rc = s->driver ? s->driver->rerank() : device_search_rerank(s);
    search_commit(s, rc, 1);
    if (rc) s->dot = was, s->dot_strength = old_strength, s->dot_cls = old_cls;
    return rc;
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

// The state the next iteration starts from.  Device-resident: the state buffers the last accept
// step wrote (colors[st], err[st]: plain [P][4K] and [P] whatever the chunk count -- the chunk
// padding lives in the prepared palettes alone), after the stream has drained.
int hq_search_population(const hq_search* s, float* colors, double* errors) {
    if (!s || !colors) return HQ_ERR_ARG;
    if (!s->driver) {
        hq_ctx* c = s->ctx;
        int rc = bind(c);
        if (rc) return rc;
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        HIP_TRY(c, hipMemcpy(colors, s->colors[s->st].p, sizeof(float) * 4 * s->K * s->P, hipMemcpyDeviceToHost));
        if (errors) HIP_TRY(c, hipMemcpy(errors, s->err[s->st].p, sizeof(double) * s->P, hipMemcpyDeviceToHost));
        return HQ_OK;
    }
    std::copy(s->driver->colors().begin(), s->driver->colors().end(), colors);
    if (errors) std::copy(s->driver->current_errors().begin(), s->driver->current_errors().end(), errors);
    return HQ_OK;
}

int hq_search_info(const hq_search* s, int* device_resident, int* nch, int* graph) {
    if (!s) return HQ_ERR_ARG;
    if (device_resident) *device_resident = s->driver ? 0 : 1;  // (hq_search_create_from built one or the other)
    if (nch) *nch = s->nch;
    if (graph) *graph = s->graphed ? 1 : 0;
    return HQ_OK;
}

// As hq_destroy: the context's device current and its stream drained (a run's
// kernels read the state buffers and record the events) before the members let go
// of their memory and events (delete s).
void hq_search_destroy(hq_search* s) {
    if (!s) return;
    if (!s->driver && s->ctx) {
        (void)hipSetDevice(s->ctx->device);
        (void)hipStreamSynchronize(s->ctx->stream);
    }
    if (s->gexec) (void)hipGraphExecDestroy(s->gexec);
    delete s->pol;
    delete s->driver;
    delete s;
}

}  // extern "C"
