// foldin.hpp -- entity fold-in on the device: the rows of new ("free") entities
// are learnt from a few example triples while every other row, relation vector,
// TransH normal and TransR matrix stays frozen.  Its own translation unit
// (foldin.hip) behind kb2e_fold_in_entities; the semantics of one step are in
// include/kb2e_engine.h.
//
// Deliberate difference from the reference's transRNorm (transr/trainer.cpp:
// 35-64): that loop updates the entity row and the matrix in place, column by
// column, so column i + 1 already sees the row changed by column i.  Here the
// matrix is frozen, and the constraint loop is the plain gradient step of
// |yW|^2 with every column taken at the row as the sweep found it
// (y_j -= lr * sum_k 2 q_k W[j][k], q = yW).  The two differ by O(lr^2) a
// sweep; the simultaneous form costs two dependent wave steps a sweep instead
// of n.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "eval.hpp"
#include "predict.hpp"

namespace kb2e {

struct FoldQuery {
    const int32_t* free_entities;
    int64_t nfree;
    const int32_t *heads, *tails, *relations;  // the examples
    int64_t count;
    const int32_t *kh, *kt, *kr;  // the known triples
    int64_t nknown;
    int32_t epochs;
    uint64_t seed;
    int32_t side;        // 0 head, 1 tail, 2 a coin per sample
    int32_t max_sweeps;  // 0: kFoldDefaultSweeps
    double lr, margin;
    const double* rows_in;  // [nfree][n] or null: the rows as they stand in the table
};

// Writes the free entities' rows of t.ent (the only device memory of the
// context that changes); rows_out [nfree][n] (may be null) receives them as
// stored, loss [nfree][2] the first and the last pass's summed hinge loss,
// counts [nfree][3] active, failed and capped over all passes.  Synchronises
// t.stream first and last.
void fold_in_entities(const EvalTables& t, const FoldQuery& q, double* rows_out, double* loss, int64_t* counts,
                      const PredictHooks* hooks = nullptr);

}  // namespace kb2e
