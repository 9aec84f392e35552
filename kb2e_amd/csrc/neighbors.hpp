// neighbors.hpp -- entity neighbours on the device: per query entity the k
// nearest entities in the entity space or in a relation's projected space, with
// no key buffer (a fused score + per-row select).  Its own translation unit
// (neighbors.hip) behind kb2e_neighbors; the stateless FP64 sums are the
// evaluator's (eval.hpp, eval_shared.hpp).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "eval.hpp"
#include "predict.hpp"

namespace kb2e {

struct NeighborsQuery {
    const int32_t* entities;  // query q asks for the neighbours of entities[q]
    int64_t nq;
    int32_t relation;      // -1: the entity space; r >= 0: relation r's projected space
    int32_t k;             // 1..kNeighborsMaxK
    int32_t include_self;  // 0 / 1
};

// kb2e_counter's numbers of one call
struct NeighborsStats {
    int64_t candidates = 0;  // pairs scored
    int64_t slices = 0;      // candidate slices of a tile
    int64_t chunks = 0;      // runs of queries that shared the partial records
    int64_t prunes = 0;      // cuts of a row's list to its k best (the bound was lowered)
};

// ids / dist [nq][k], found [nq]: per query the found = min(k, candidates)
// nearest entities in ascending (distance, id) order, then -1 / +inf.
void neighbors(const EvalTables& t, const NeighborsQuery& q, int32_t* ids, double* dist, int32_t* found,
               NeighborsStats* stats, const PredictHooks* hooks = nullptr);

}  // namespace kb2e
