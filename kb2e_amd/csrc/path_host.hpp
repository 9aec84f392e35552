// path_host.hpp -- host side of the path queries (kb2e_predict_path,
// kb2e_rank_path), free of HIP so that it can be checked on the CPU
// (tests/native/path_check.cpp).
//
// Query q starts at anchors[q] and owns the hops offsets[q] .. offsets[q + 1] - 1,
// each (relation, side) in kb2e_predict's convention.  Here live: the check of
// `offsets`, the plan that cuts the queries into chunks whose device rows fit
// the budget, the order of a chunk's queries and the plan of one hop level, the
// walk of the filter triples along a path (the answers the graph already
// states) and the back-tracking of the winning path from the per-level
// frontiers and their back-pointers.
#pragma once

#include <algorithm>
#include <cstdint>
#include <numeric>
#include <utility>
#include <vector>

#include "predict_host.hpp"

namespace kb2e {

constexpr int kPathMaxHops = 8;     // KB2E_PATH_MAX_HOPS
constexpr int kPathMaxBeam = 1024;  // the select kernel's sort buffer

// nullptr when offsets [nq + 1] is well-formed (nq >= 1), else what is wrong.
inline const char* path_check_offsets(const int64_t* offsets, int64_t nq) {
    if (nq < 1) return "no queries";
    if (!offsets) return "no offsets";
    if (offsets[0] != 0) return "offsets must start at 0";
    for (int64_t q = 0; q < nq; ++q) {
        // (compared, not subtracted: a hostile pair of offsets must not overflow)
        if (offsets[q + 1] <= offsets[q]) return "offsets must increase: a query without hops";
        if (offsets[q + 1] > (int64_t)INT32_MAX) return "more than 2^31 - 1 hops in one call";
        if (offsets[q + 1] - offsets[q] > kPathMaxHops) return "a query with more than 8 hops";
    }
    return nullptr;
}

// What a query of L hops holds on the device, in rows of |E| 4-byte words: a
// key row is two of them, a predecessor row one.  Beam search keeps one key row
// and (L >= 2) one predecessor row, both rewritten by every hop.  The exact form
// (beam = 0) reads the previous level's key row as the frontier's costs while it
// writes the next (two key rows) and keeps a back-pointer row per hop 2..L.
inline int64_t path_query_units(int64_t hops, bool exact) {
    if (hops < 2) return 2;
    return exact ? 4 + (hops - 1) : 3;
}

struct PathChunk {
    int64_t q0, q1;  // the queries [q0, q1)
};

// The queries in the caller's order, cut into the longest runs whose units fit
// max(budget_units, the largest query) and that hold at most max_queries
// queries: every query in exactly one chunk, never split.
inline std::vector<PathChunk> path_plan_chunks(const int64_t* offsets, int64_t nq, bool exact, int64_t budget_units,
                                               int64_t max_queries) {
    int64_t budget = budget_units;
    for (int64_t q = 0; q < nq; ++q) budget = std::max(budget, path_query_units(offsets[q + 1] - offsets[q], exact));
    max_queries = std::max<int64_t>(1, max_queries);
    std::vector<PathChunk> chunks;
    for (int64_t q0 = 0; q0 < nq;) {
        int64_t q1 = q0, units = 0;
        while (q1 < nq && q1 - q0 < max_queries) {
            const int64_t u = path_query_units(offsets[q1 + 1] - offsets[q1], exact);
            if (units + u > budget) break;
            units += u;
            ++q1;
        }
        chunks.push_back(PathChunk{q0, q1});
        q0 = q1;
    }
    return chunks;
}

// The device order of a chunk's queries: by falling number of hops, so that the
// queries still walking at level i are the rows [0, live(i)) and those that end
// there the rows [live(i + 1), live(i)); among equal lengths by (relation, side)
// of the first hop (stable), so that hop 1 -- the one-sided score kernel, which
// writes a dense run of rows -- finds a relation's rows side by side.
// order[row] = the query.
inline std::vector<int64_t> path_chunk_order(const int64_t* offsets, const int32_t* relations, const int32_t* side,
                                             int64_t q0, int64_t q1) {
    std::vector<int64_t> order((size_t)(q1 - q0));
    std::iota(order.begin(), order.end(), q0);
    std::stable_sort(order.begin(), order.end(), [&](int64_t x, int64_t y) {
        const int64_t lx = offsets[x + 1] - offsets[x], ly = offsets[y + 1] - offsets[y];
        if (lx != ly) return lx > ly;
        const int64_t a = offsets[x], b = offsets[y];
        return relations[a] != relations[b] ? relations[a] < relations[b] : side[a] < side[b];
    });
    return order;
}

// The rows of `order` whose query has at least `level` hops (a prefix).
inline int64_t path_live(const int64_t* offsets, const std::vector<int64_t>& order, int level) {
    int64_t m = 0;
    while (m < (int64_t)order.size() && offsets[order[(size_t)m] + 1] - offsets[order[(size_t)m]] >= level) ++m;
    return m;
}

// Hop level `level` (from 1) of a chunk: its live rows sorted stably by
// (relation, side) of that hop, so that a relation's rows are one run and the
// relation is projected once.
struct PathLevel {
    std::vector<int32_t> row;   // [live] slot -> row of the chunk
    std::vector<int32_t> rel;   // [live] the hop's relation
    std::vector<int32_t> side;  // [live] and side
    int64_t relations = 0;      // distinct relations
};

inline PathLevel path_plan_level(const int64_t* offsets, const int32_t* relations, const int32_t* side,
                                 const std::vector<int64_t>& order, int level) {
    PathLevel pl;
    const int64_t live = path_live(offsets, order, level);
    pl.row.resize((size_t)live);
    std::iota(pl.row.begin(), pl.row.end(), 0);
    auto hop = [&](int32_t row) { return offsets[order[(size_t)row]] + level - 1; };
    std::stable_sort(pl.row.begin(), pl.row.end(), [&](int32_t x, int32_t y) {
        const int64_t a = hop(x), b = hop(y);
        return relations[a] != relations[b] ? relations[a] < relations[b] : side[a] < side[b];
    });
    pl.rel.resize((size_t)live), pl.side.resize((size_t)live);
    for (int64_t s = 0; s < live; ++s) {
        pl.rel[(size_t)s] = relations[hop(pl.row[(size_t)s])];
        pl.side[(size_t)s] = side[hop(pl.row[(size_t)s])];
        if (s == 0 || pl.rel[(size_t)s] != pl.rel[(size_t)s - 1]) ++pl.relations;
    }
    return pl;
}

// ---- the answers the graph already states.  The filter triples as one sorted,
// distinct list of (query_key(entity, relation, side), neighbour): (h, t, r) is
// the step h -> t of (r, side 1) and t -> h of (r, side 0).  Only the (relation,
// side) pairs some hop uses are kept.
struct PathAdjacency {
    std::vector<std::pair<uint64_t, int32_t>> steps;
    int64_t nr = 0;
};

inline PathAdjacency path_build_adjacency(const int32_t* hop_rel, const int32_t* hop_side, int64_t nhops,
                                          const int32_t* fh, const int32_t* ft, const int32_t* fr, int64_t nfilter,
                                          int64_t nr) {
    PathAdjacency adj;
    adj.nr = nr;
    if (nfilter < 1) return adj;
    std::vector<uint8_t> used((size_t)nr * 2, 0);
    for (int64_t c = 0; c < nhops; ++c) used[(size_t)hop_rel[c] * 2 + (size_t)(hop_side[c] & 1)] = 1;
    for (int64_t k = 0; k < nfilter; ++k) {
        if (used[(size_t)fr[k] * 2 + 1]) adj.steps.emplace_back(query_key(fh[k], fr[k], 1, nr), ft[k]);
        if (used[(size_t)fr[k] * 2]) adj.steps.emplace_back(query_key(ft[k], fr[k], 0, nr), fh[k]);
    }
    std::sort(adj.steps.begin(), adj.steps.end());
    adj.steps.erase(std::unique(adj.steps.begin(), adj.steps.end()), adj.steps.end());
    return adj;
}

// S_L of one query (ascending, distinct): S_0 = {anchor}, S_i = the entities one
// filter triple of hop i's (relation, side) away from a member of S_{i-1};
// no_loops: a triple with h == t is no step.
inline void path_walk_known(const PathAdjacency& adj, int32_t anchor, const int32_t* rel, const int32_t* side,
                            int64_t hops, bool no_loops, std::vector<int32_t>& out) {
    out.assign(1, anchor);
    std::vector<int32_t> next;
    for (int64_t i = 0; i < hops && !out.empty(); ++i) {
        next.clear();
        for (const int32_t e : out) {
            const uint64_t key = query_key(e, rel[i], side[i], adj.nr);
            auto it = std::lower_bound(adj.steps.begin(), adj.steps.end(), std::make_pair(key, (int32_t)INT32_MIN));
            for (; it != adj.steps.end() && it->first == key; ++it)
                if (!(no_loops && it->second == e)) next.push_back(it->second);
        }
        std::sort(next.begin(), next.end());
        next.erase(std::unique(next.begin(), next.end()), next.end());
        out.swap(next);
    }
}

// Per query the excluded answers: off [nq + 1] indexes ids.
struct PathKnown {
    std::vector<int64_t> off;
    std::vector<int32_t> ids;
};

inline PathKnown path_known_answers(const int32_t* anchors, const int64_t* offsets, const int32_t* relations,
                                    const int32_t* side, int64_t nq, bool no_loops, const int32_t* fh,
                                    const int32_t* ft, const int32_t* fr, int64_t nfilter, int64_t nr) {
    PathKnown pk;
    pk.off.assign((size_t)nq + 1, 0);
    if (nfilter < 1) return pk;
    const PathAdjacency adj = path_build_adjacency(relations, side, offsets[nq], fh, ft, fr, nfilter, nr);
    std::vector<int32_t> cur;
    for (int64_t q = 0; q < nq; ++q) {
        path_walk_known(adj, anchors[q], relations + offsets[q], side + offsets[q], offsets[q + 1] - offsets[q],
                        no_loops, cur);
        pk.ids.insert(pk.ids.end(), cur.begin(), cur.end());
        pk.off[(size_t)q + 1] = (int64_t)pk.ids.size();
    }
    return pk;
}

// ---- the winning path of one answer under beam search.  Level i (1 .. hops - 1)
// of the query has the frontier ids fid[(i - 1) * level_stride + j], j < beam
// (-1: no entry), and for i >= 2 the predecessor back[(i - 1) * level_stride + j]
// of entry j, a member of level i - 1's frontier.  last_pred is the predecessor
// of the answer itself, x_{hops-1}.  Fills via[i] = x_{i+1} for i < hops - 1 and
// -1 behind; false (and all -1) if a predecessor is in no frontier.
inline bool path_backtrack(int hops, int32_t beam, const int32_t* fid, const int32_t* back, int64_t level_stride,
                           int32_t last_pred, int32_t* via /* [kPathMaxHops - 1] */) {
    std::fill(via, via + (kPathMaxHops - 1), -1);
    if (hops < 2) return true;
    int32_t x = last_pred;
    for (int lev = hops - 1; lev >= 1; --lev) {
        if (x < 0) break;
        via[lev - 1] = x;
        if (lev == 1) return true;
        const int32_t* f = fid + (int64_t)(lev - 1) * level_stride;
        const int32_t* p = std::find(f, f + beam, x);
        x = p == f + beam ? -1 : back[(int64_t)(lev - 1) * level_stride + (p - f)];
    }
    std::fill(via, via + (kPathMaxHops - 1), -1);
    return false;
}

}  // namespace kb2e
