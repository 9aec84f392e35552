// complete.hpp -- knowledge-base completion on the device: per relation the k
// most plausible triples (h, t, r) that are not known yet, over every pair of
// candidate entities.  Its own translation unit (complete.hip) behind
// kb2e_complete_triples; the stateless FP64 energies are the evaluator's
// (eval.hpp, eval_shared.hpp).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "eval.hpp"
#include "predict.hpp"

namespace kb2e {

struct CompleteQuery {
    const int32_t* relations;  // query q mines relations[q]
    int64_t nrel;
    int32_t k;                    // 1..kPredictMaxK
    const int32_t *kh, *kt, *kr;  // the known triples: excluded, and the pools of a constrained call
    int64_t nknown;
    int32_t constrained, exclude_loops;  // 0 / 1
};

// kb2e_counter's numbers of one call
struct CompleteStats {
    int64_t candidates = 0;      // pairs scored
    int64_t records = 0;         // records appended
    int64_t strips = 0;          // score + select steps
    int64_t buffer_records = 0;  // the record buffer's capacity
};

// heads / tails / energy [nrel][k], found [nrel]: per query the
// found = min(k, candidates - excluded) candidates of smallest energy in
// ascending (energy, head id, tail id) order, then -1 / -1 / +inf.
void complete_triples(const EvalTables& t, const CompleteQuery& q, int32_t* heads, int32_t* tails, double* energy,
                      int64_t* found, CompleteStats* stats, const PredictHooks* hooks = nullptr);

}  // namespace kb2e
