// classify.hpp -- triple classification on the device: per-relation thresholds
// fitted on labelled triples, the classification itself and generated
// negatives.  Its own translation unit (classify.hip) behind
// kb2e_fit_thresholds / kb2e_classify_triples / kb2e_corrupt_triples; the
// energies are predict.hip's triple-scoring kernels (score_triples_device).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "eval.hpp"
#include "predict.hpp"

namespace kb2e {

struct LabelledTriples {
    const int32_t *heads, *tails, *relations;
    const uint8_t* labels;  // 1 holds, 0 does not
    int64_t count;
};

// thresholds [nr], counts [nr][3] = positives, negatives, correct; the rule is
// in include/kb2e_engine.h (kb2e_fit_thresholds).  global_threshold /
// global_correct may be null.
void fit_thresholds(const EvalTables& t, const LabelledTriples& q, double* thresholds, int64_t* counts,
                    double* global_threshold, int64_t* global_correct, const PredictHooks* hooks = nullptr);

// labels_out[i] = energy_i <= thresholds[relations[i]]; energy may be null.
void classify_triples(const EvalTables& t, const int32_t* heads, const int32_t* tails, const int32_t* relations,
                      int64_t count, const double* thresholds, uint8_t* labels_out, double* energy,
                      const PredictHooks* hooks = nullptr);

struct CorruptQuery {
    const int32_t *heads, *tails, *relations;
    int64_t count;
    const int32_t *kh, *kt, *kr;  // the known triples
    int64_t nknown;
    uint64_t seed;
    int32_t side;         // 0 head, 1 tail, 2 a coin per triple
    int32_t constrained;  // stage 1 draws from the (relation, slot) pool
};

// neg_heads / neg_tails [count] (-1, -1 where every draw was rejected); returns the number of those.
int64_t corrupt_triples(const EvalTables& t, const CorruptQuery& q, int32_t* neg_heads, int32_t* neg_tails,
                        const PredictHooks* hooks = nullptr);

}  // namespace kb2e
