// hq_swasa.h -- host-side SWASA policy and search driver (internal).
//
// SW:3-116 (policy) and IM:383-591 (findBestQuantization main loop) restated
// in C++.  The population evaluator is abstract so the same driver runs on the
// GPU context (hq_search_*) and on a host callback (hq_swasa_search_host).
#pragma once

#include <cmath>
#include <cstdint>
#include <functional>
#include <utility>
#include <vector>

#include "../../include/hq.h"

namespace hq {

// java.util.Random: 48-bit LCG; nextFloat = next(24)/2^24; nextDouble 53 bits.
class JavaRandom {
   public:
    explicit JavaRandom(uint64_t seed) { set_seed(seed); }
    void set_seed(uint64_t s) { seed_ = (s ^ kMult) & kMask; }
    int32_t next(int bits) {
        seed_ = (seed_ * kMult + 0xBull) & kMask;
        return (int32_t)(int64_t)(seed_ >> (48 - bits));
    }
    float next_float() { return (float)next(24) / (float)(1 << 24); }
    double next_double() {
        return (double)(((int64_t)next(26) << 27) + next(27)) * (1.0 / (double)(1LL << 53));
    }

   private:
    static constexpr uint64_t kMult = 0x5DEECE66Dull;
    static constexpr uint64_t kMask = (1ull << 48) - 1;
    uint64_t seed_;
};

// SW:3-116.  Fields kept in fp32 like the Java class.
class Swasa {
   public:
    Swasa(const hq_swasa_params& p, uint64_t seed);
    void reset();                                           // SW:30-34
    void generate_random_colors(int K, float* out) ;        // SW:40-52
    bool is_accepted(double delta_e);                       // SW:54-57
    bool keeps_his_values(int iteration);                   // SW:59-62
    double keep_threshold(int iteration) const;             // its left-hand side
    float max_step_width(int i) const;                      // SW:69-72
    double compute_penalty(const int32_t* used, int K) const;  // SW:74-82
    void reduce_temperature_if_necessary(int iteration);    // SW:84-89
    // SW:91-101.  nfixed (libhq's addition): the draws of colour k < nfixed are made and
    // discarded, and next's colour k is colors' colour k, its bits.
    void generate_neighboring_colors(const float* colors, float* next, int K, int iteration, int nfixed = 0);
    const hq_swasa_params& params() const { return p_; }
    float temperature() const { return temperature_; }

   private:
    hq_swasa_params p_;
    JavaRandom rng_;
    float temperature_, step_width_;
};

// A population a search may start from: every R, G, B finite and in [0, 1].
bool population_in_range(const float* population, int P, int K);

using PopulationEval = std::function<int(const float* palettes, int P, int K, double* costs)>;
// The k-means move of a hybrid iteration: updates the candidates in place.
using PopulationRefine = std::function<int(float* palettes, int P, int K)>;

// IM:383-591 as a resumable state machine.
class SearchDriver {
   public:
    SearchDriver(const hq_swasa_params& p, int K, uint64_t seed, PopulationEval eval);
    // IM:385-493: reset, initial population, argmin.  With a population ([P][4K]; libhq's
    // addition) the random colours are drawn and thrown away and the given ones take their
    // place, .w = 0: the generator ends where the plain start leaves it.
    int start(const float* population = nullptr);
    int run(int iterations, int* ran, std::vector<double>* trace);   // IM:497-568
    // The evaluator has changed before the first iteration (hq_search_set_ordered): the
    // initial population evaluated and ranked again (IM:490-493); no draws.  HQ_ERR_STATE
    // once an iteration has run.
    int rerank();
    // Hybrid iterations (libhq's addition): with every > 0 and a refine step,
    // the candidates of iteration ite (1-based, counted across run calls) with
    // ite % every == 0 go through `refine` between their generation and their
    // evaluation.  Applies to the iterations that follow.
    void set_refine(PopulationRefine refine) { refine_ = std::move(refine); }
    void set_every(int every) { every_ = every; }
    // Repair iterations (libhq's addition), the same way with a period of their own:
    // `repair` runs after `refine` when an iteration is both.
    void set_repair(PopulationRefine repair) { repair_ = std::move(repair); }
    void set_repair_every(int every) { repair_every_ = every; }
    // Fixed colours (libhq's addition, hq_set_fixed_colors' semantics), set before start():
    // the first n colours of every member are `colors` ([n][4], .w stored as 0; null: as the
    // population or the draws have them) and no iteration changes them -- their draws are
    // made and discarded, and they are put back after `refine` and `repair` return.
    void set_fixed(int n, const float* colors) {
        nfixed_ = n;
        fixed_.clear();
        if (colors) {
            fixed_.assign(colors, colors + (size_t)4 * n);
            for (size_t e = 3; e < fixed_.size(); e += 4) fixed_[e] = 0.0f;
        }
    }
    const std::vector<float>& best_colors() const { return best_colors_; }
    double best_error() const { return best_error_; }
    int iteration() const { return ite_; }
    // The current population [P][4K] and each member's error as the accept step holds it
    // (hq_search_population).
    const std::vector<float>& colors() const { return colors_; }
    const std::vector<double>& current_errors() const { return current_errors_; }

   private:
    Swasa sw_;
    int K_, P_;
    PopulationEval eval_;
    PopulationRefine refine_;
    int every_ = 0;
    PopulationRefine repair_;
    int repair_every_ = 0;
    int nfixed_ = 0;
    std::vector<float> fixed_;              // [nfixed][4], or empty
    std::vector<float> colors_, current_;   // [P][4K]
    std::vector<double> current_errors_, errors_;
    std::vector<float> best_colors_;
    double best_error_ = 0.0;
    int ite_ = 0;
    bool started_ = false;
};

}  // namespace hq
