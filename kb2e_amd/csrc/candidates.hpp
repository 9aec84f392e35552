// candidates.hpp -- scoring and ranking against caller-supplied candidate
// lists on the device: per query (entity, relation, side) the energies of the
// listings of its list, or the rank of a truth among them, with no expanded
// triple arrays.  Its own translation unit (candidates.hip) behind
// kb2e_score_candidates / kb2e_rank_candidates; the stateless FP64 energies are
// the evaluator's (eval.hpp, eval_shared.hpp).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "eval.hpp"
#include "predict.hpp"

namespace kb2e {

struct CandidatesQuery {
    const int32_t *ent, *rel, *side;  // query q: (ent[q], ?, rel[q]) for side 1, (?, ent[q], rel[q]) for side 0
    const int32_t* truth;             // rank_candidates: the entity to rank per query (else null)
    const int32_t* lists;             // the list of each query (null: list q)
    int64_t nq;
    const int64_t* offsets;           // [nlists + 1]
    const int32_t* candidates;        // [offsets[nlists]]
    int64_t nlists;
    const int32_t *fh, *ft, *fr;      // rank_candidates: the filter set
    int64_t nfilter;
};

// kb2e_counter's numbers of one call
struct CandidatesStats {
    int64_t listings = 0;     // energies computed for a listing
    int64_t items = 0;        // wave-sized work items
    int64_t chunks = 0;       // runs of queries that shared the device buffers
    int64_t projections = 0;  // TransR: per-relation projections made (compact or full)
    int64_t probes = 0;       // filter-set probes
};

// energy: the queries' energies back to back in query order, each in its list's order.
void score_candidates(const EvalTables& t, const CandidatesQuery& q, double* energy, CandidatesStats* stats,
                      const PredictHooks* hooks = nullptr);

// ranks [nq][2]: raw and filtered rank of truth[q] among the listings of query
// q; counted [nq][2] (or null): the listings that took part in each.
void rank_candidates(const EvalTables& t, const CandidatesQuery& q, int64_t* ranks, int64_t* counted,
                     CandidatesStats* stats, const PredictHooks* hooks = nullptr);

}  // namespace kb2e
