// predict.hpp -- using a trained model on the device: the energy of given
// triples, the top-k candidates of one-sided queries and relation prediction.
// Its own translation unit (predict.hip) behind kb2e_score_triples /
// kb2e_predict / kb2e_predict_relations / kb2e_rank_relations /
// kb2e_predict_joint / kb2e_rank_joint; the stateless
// FP64 energies are the evaluator's (eval.hpp, eval_shared.hpp).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "eval.hpp"

namespace kb2e {

// Timing of the kernel families (the engine's profile): begin() returns the
// start event of a span on the tables' stream (null when profiling is off),
// end() records its stop event under `name`.
struct PredictHooks {
    void* ud;
    hipEvent_t (*begin)(void* ud);
    void (*end)(void* ud, const char* name, hipEvent_t a);
};

// One timed span of a kernel family (nothing when hooks are null or profiling is off).
struct Span {
    const PredictHooks* h;
    const char* name;
    hipEvent_t a = nullptr;
    Span(const PredictHooks* hooks, const char* nm) : h(hooks), name(nm) {
        if (h && h->begin) a = h->begin(h->ud);
    }
    void end() {
        if (h && h->end && a) h->end(h->ud, name, a);
        a = nullptr;
    }
};

struct PredictQuery {
    const int32_t *ent, *rel, *side;  // query q: (ent[q], ?, rel[q]) for side 1, (?, ent[q], rel[q]) for side 0
    int64_t nq;
    int32_t k;                        // 1..kPredictMaxK
    const int32_t *fh, *ft, *fr;      // candidates whose triple is listed here are excluded
    int64_t nfilter;
};

constexpr int kPredictMaxK = 1024;

// ids / energy [nq][k], found [nq]: per query the found = min(k, |E| - excluded)
// candidates of smallest energy in ascending (energy, id) order, then -1 / +inf.
void predict_topk(const EvalTables& t, const PredictQuery& q, int32_t* ids, double* energy, int32_t* found,
                  const PredictHooks* hooks = nullptr);

// energy[i] = tripleEnergy(heads[i], tails[i], relations[i]) (TransR from zeroed work vectors).
void score_triples(const EvalTables& t, const int32_t* heads, const int32_t* tails, const int32_t* relations,
                   int64_t count, double* energy);

// The same kernels on arrays that are already on the device (classify.hip: the
// energies never leave the card between scoring and fitting).  The ids must be
// in range (the caller checks them on the host).  Queued on t.stream in
// launches of at most 2^22 triples; no synchronisation.
void score_triples_device(const EvalTables& t, const int32_t* d_heads, const int32_t* d_tails,
                          const int32_t* d_relations, int64_t count, double* d_energy);

// Relation prediction: query q is the pair (heads[q], tails[q]) and its
// candidates are the triples (h, t, r) of every relation r.
struct RelationQuery {
    const int32_t *heads, *tails;
    const int32_t* truth;  // rank_relations: the true relation of each pair (else null)
    int64_t nq;
    int32_t k;             // predict_relations: 1..kPredictMaxK
    const int32_t *fh, *ft, *fr;
    int64_t nfilter;
};

// ids / energy [nq][k], found [nq]: per pair the found = min(k, |R| - excluded)
// relations of smallest energy in ascending (energy, id) order, then -1 / +inf.
void predict_relations(const EvalTables& t, const RelationQuery& q, int32_t* ids, double* energy, int32_t* found,
                       const PredictHooks* hooks = nullptr);

// ranks[q * 2 + 0..1] = raw and filtered rank of truth[q] among the |R|
// candidates of pair q (1 + the candidates of strictly smaller energy; the
// filtered rank leaves out the other relations whose triple is in the filter).
void rank_relations(const EvalTables& t, const RelationQuery& q, int64_t* ranks, const PredictHooks* hooks = nullptr);

// Conjunctive queries: query q owns the constraint rows offsets[q] ..
// offsets[q + 1] - 1 (1..64 of them), each a one-sided pattern (ent, rel, side)
// as PredictQuery's; the joint energy of a candidate x is the sum of its
// energies over those rows, added in the caller's order, and x is excluded iff
// every one of its triples is in the filter.
struct JointQuery {
    const int64_t* offsets;           // [nq + 1]
    const int32_t *ent, *rel, *side;  // [offsets[nq]]
    const int32_t* truth;             // rank_joint: the entity to rank per query (else null)
    int64_t nq;
    int32_t k;                        // predict_joint: 1..kPredictMaxK
    const int32_t *fh, *ft, *fr;
    int64_t nfilter;
};

// The last call's numbers (kb2e_counter "joint_*").
struct JointStats {
    int64_t chunks = 0;       // runs of queries whose rows shared the key buffer
    int64_t rows = 0;         // constraint rows scored
    int64_t projections = 0;  // project_any calls
};

// ids / energy [nq][k], found [nq]: as predict_topk, on the joint energies.
void predict_joint(const EvalTables& t, const JointQuery& q, int32_t* ids, double* energy, int32_t* found,
                   JointStats* stats = nullptr, const PredictHooks* hooks = nullptr);

// ranks[q * 2 + 0..1] = raw and filtered rank of truth[q] among the |E| candidates of query q.
void rank_joint(const EvalTables& t, const JointQuery& q, int64_t* ranks, JointStats* stats = nullptr,
                const PredictHooks* hooks = nullptr);

// Path queries: query q starts at anchors[q] and owns the hops offsets[q] ..
// offsets[q + 1] - 1 (1..8 of them), each (rel, side) as PredictQuery's: side 1
// steps from the head to the tail of the relation, side 0 backwards.  The path
// energy of an entity is the smallest sum of hop energies, added in hop order,
// over the paths that end in it; after every hop but the last only the `beam`
// entities of smallest (energy, id) are kept (0: all of them).
struct PathQuery {
    const int32_t* anchors;      // [nq]
    const int64_t* offsets;      // [nq + 1]
    const int32_t *rel, *side;   // [offsets[nq]]
    const int32_t* truth;        // rank_path: the entity to rank per query (else null)
    int64_t nq;
    int32_t k;                   // predict_path: 1..kPredictMaxK
    int32_t beam, no_loops;      // 0..1024; 0 / 1
    const int32_t *fh, *ft, *fr;
    int64_t nfilter;
};

// The last call's numbers (kb2e_counter "path_*").
struct PathStats {
    int64_t chunks = 0;       // runs of queries that shared the device rows
    int64_t hops = 0;         // query-levels the hop kernel ran (hops 2..L of every query)
    int64_t projections = 0;  // project_any calls
};

// ids / energy [nq][k], found [nq]: as predict_topk, on the path energies; via
// [nq][k][7] (or null): the intermediate entities of each answer's winning path.
void predict_path(const EvalTables& t, const PathQuery& q, int32_t* ids, double* energy, int32_t* found, int32_t* via,
                  PathStats* stats = nullptr, const PredictHooks* hooks = nullptr);

// ranks[q * 2 + 0..1] = raw and filtered rank of truth[q] among the |E| candidates of query q.
void rank_path(const EvalTables& t, const PathQuery& q, int64_t* ranks, PathStats* stats = nullptr,
               const PredictHooks* hooks = nullptr);

}  // namespace kb2e
