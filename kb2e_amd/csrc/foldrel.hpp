// foldrel.hpp -- relation fold-in on the device: the rows of new ("free")
// relations (TransH: and their normals; TransR: and their matrices) are learnt
// from example triples while every entity row and every other relation's
// parameters stay frozen.  Its own translation unit (foldrel.hip) behind
// kb2e_fold_in_relations; the semantics of one batch are in
// include/kb2e_engine.h.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "eval.hpp"
#include "predict.hpp"

namespace kb2e {

struct FoldRelQuery {
    const int32_t* free_relations;
    int64_t nfree;
    const int32_t *heads, *tails, *relations;  // the examples
    int64_t count;
    const int32_t *kh, *kt, *kr;  // the known triples
    int64_t nknown;
    int32_t epochs;
    int64_t batch_size;
    uint64_t seed;
    int32_t side;        // 0 head, 1 tail, 2 a coin per sample
    int32_t max_sweeps;  // 0: kFoldDefaultSweeps
    double lr, margin;
    const double* rel_in;  // [nfree][n] or null: the rows as they stand in the table
    const double* w_in;    // [nfree][n] (TransH) / [nfree][n][n] (TransR) or null
    void* w_mirror;        // TransR: a second device copy of the weight table that receives the same rows, or null
};

// The widest TransR matrix foldrel.hip keeps in LDS (wider ones, and every one
// with KB2E_FOLDREL_W_L2=1, are worked on in a global scratch).
int32_t fold_rel_lds_limit();

// Writes the free relations' rows of t.rel and t.w (the only device memory of
// the context that changes); rel_out [nfree][n] and w_out [nfree][n or n * n]
// (may be null) receive them as stored, loss [nfree][2] the first and the last
// pass's summed hinge loss, counts [nfree][3] active, failed and capped over
// all passes.  Synchronises t.stream first and last.
void fold_in_relations(const EvalTables& t, const FoldRelQuery& q, double* rel_out, double* w_out, double* loss,
                       int64_t* counts, const PredictHooks* hooks = nullptr);

}  // namespace kb2e
