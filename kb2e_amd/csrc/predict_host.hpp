// predict_host.hpp -- host side of the top-k queries (kb2e_predict) and of
// relation prediction (kb2e_predict_relations, kb2e_rank_relations), free of
// HIP so that it can be checked on the CPU (tests/native/predict_check.cpp,
// tests/native/relpred_check.cpp).
//
// A query is (entity e, relation r, side): side 1 asks for tails of (e, ?, r),
// side 0 for heads of (?, e, r).  The filtered form excludes every candidate x
// whose triple is a known one.  Probing a hash set per (query, candidate)
// would cost nq * |E| random reads; instead the known candidates of every
// distinct (e, r, side) are listed once from the filter triples, in
// O(nfilter + nq) plus the sort of each list, and the device overwrites
// exactly those keys (predict_mask_kernel).
#pragma once

#include <algorithm>
#include <cstdint>
#include <unordered_map>
#include <vector>

namespace kb2e {

struct KnownCandidates {
    std::vector<int32_t> group;  // [nq]: the list of query q (queries that share (e, r, side) share one)
    std::vector<int64_t> off;    // [ngroups + 1]
    std::vector<int32_t> ids;    // known candidates of each list: ascending, distinct
};

inline uint64_t query_key(int64_t e, int64_t r, int64_t side, int64_t nr) {
    return (((uint64_t)e * (uint64_t)nr + (uint64_t)r) << 1) | (uint64_t)(side & 1);
}

// ids must be in range (the callers check).  nfilter == 0: every list is empty.
inline KnownCandidates build_known_candidates(const int32_t* qe, const int32_t* qr, const int32_t* qside, int64_t nq,
                                              const int32_t* fh, const int32_t* ft, const int32_t* fr,
                                              int64_t nfilter, int64_t nr) {
    KnownCandidates kc;
    kc.group.resize((size_t)nq);
    std::unordered_map<uint64_t, int32_t> groups;
    groups.reserve((size_t)nq * 2 + 16);
    for (int64_t q = 0; q < nq; ++q) {
        auto it = groups.emplace(query_key(qe[q], qr[q], qside[q], nr), (int32_t)groups.size()).first;
        kc.group[(size_t)q] = it->second;
    }
    const size_t ng = groups.size();
    kc.off.assign(ng + 1, 0);
    // a filter triple (h, t, r) is a known tail t of (h, r, 1) and a known head h of (t, r, 0)
    auto each = [&](auto&& f) {
        for (int64_t k = 0; k < nfilter; ++k) {
            auto a = groups.find(query_key(fh[k], fr[k], 1, nr));
            if (a != groups.end()) f(a->second, ft[k]);
            auto b = groups.find(query_key(ft[k], fr[k], 0, nr));
            if (b != groups.end()) f(b->second, fh[k]);
        }
    };
    each([&](int32_t g, int32_t) { ++kc.off[(size_t)g + 1]; });
    for (size_t g = 0; g < ng; ++g) kc.off[g + 1] += kc.off[g];
    std::vector<int32_t> all((size_t)kc.off[ng]);
    std::vector<int64_t> fill(kc.off.begin(), kc.off.end() - 1);
    each([&](int32_t g, int32_t x) { all[(size_t)fill[(size_t)g]++] = x; });
    // duplicate filter triples: each candidate once
    kc.ids.reserve(all.size());
    std::vector<int64_t> off2(ng + 1, 0);
    for (size_t g = 0; g < ng; ++g) {
        auto b = all.begin() + kc.off[g], e = all.begin() + kc.off[g + 1];
        std::sort(b, e);
        e = std::unique(b, e);
        kc.ids.insert(kc.ids.end(), b, e);
        off2[g + 1] = (int64_t)kc.ids.size();
    }
    kc.off.swap(off2);
    return kc;
}

// ---- relation prediction (kb2e_predict_relations, kb2e_rank_relations): a
// query is a pair (h, t) and its candidates are the relations.  The known
// relations of every distinct pair are listed once from the filter triples in
// the same way: O(nfilter + nq) plus the sort of each list.

inline uint64_t pair_key(int64_t h, int64_t t, int64_t ne) { return (uint64_t)h * (uint64_t)ne + (uint64_t)t; }

// group[q]: the list of query q (queries on the same (h, t) share one); ids: the
// relations r with (h, t, r) in the filter, ascending and distinct.
inline KnownCandidates build_known_relations(const int32_t* qh, const int32_t* qt, int64_t nq, const int32_t* fh,
                                             const int32_t* ft, const int32_t* fr, int64_t nfilter, int64_t ne) {
    KnownCandidates kc;
    kc.group.resize((size_t)nq);
    std::unordered_map<uint64_t, int32_t> groups;
    groups.reserve((size_t)nq * 2 + 16);
    for (int64_t q = 0; q < nq; ++q) {
        auto it = groups.emplace(pair_key(qh[q], qt[q], ne), (int32_t)groups.size()).first;
        kc.group[(size_t)q] = it->second;
    }
    const size_t ng = groups.size();
    kc.off.assign(ng + 1, 0);
    std::vector<int32_t> fg((size_t)nfilter);  // the list a filter triple belongs to, -1: no query asks
    for (int64_t k = 0; k < nfilter; ++k) {
        auto a = groups.find(pair_key(fh[k], ft[k], ne));
        fg[(size_t)k] = a == groups.end() ? -1 : a->second;
        if (fg[(size_t)k] >= 0) ++kc.off[(size_t)fg[(size_t)k] + 1];
    }
    for (size_t g = 0; g < ng; ++g) kc.off[g + 1] += kc.off[g];
    std::vector<int32_t> all((size_t)kc.off[ng]);
    std::vector<int64_t> fill(kc.off.begin(), kc.off.end() - 1);
    for (int64_t k = 0; k < nfilter; ++k)
        if (fg[(size_t)k] >= 0) all[(size_t)fill[(size_t)fg[(size_t)k]]++] = fr[k];
    // duplicate filter triples: each relation once
    kc.ids.reserve(all.size());
    std::vector<int64_t> off2(ng + 1, 0);
    for (size_t g = 0; g < ng; ++g) {
        auto b = all.begin() + kc.off[g], e = all.begin() + kc.off[g + 1];
        std::sort(b, e);
        e = std::unique(b, e);
        kc.ids.insert(kc.ids.end(), b, e);
        off2[g + 1] = (int64_t)kc.ids.size();
    }
    kc.off.swap(off2);
    return kc;
}

// The distinct entities of a run of pairs, in order of first appearance, and
// each pair as two indices into that list (TransR projects every listed entity
// once per relation instead of twice per pair).
struct PairEntities {
    std::vector<int32_t> ents;    // [|U|] entity ids
    std::vector<int32_t> hi, ti;  // [nq] index of the head / tail in ents
};

inline PairEntities build_pair_entities(const int32_t* qh, const int32_t* qt, int64_t nq) {
    PairEntities pe;
    pe.hi.resize((size_t)nq);
    pe.ti.resize((size_t)nq);
    std::unordered_map<int32_t, int32_t> slot;
    slot.reserve((size_t)nq * 2 + 16);
    auto index = [&](int32_t e) {
        auto it = slot.emplace(e, (int32_t)pe.ents.size());
        if (it.second) pe.ents.push_back(e);
        return it.first->second;
    };
    for (int64_t q = 0; q < nq; ++q) {
        pe.hi[(size_t)q] = index(qh[q]);
        pe.ti[(size_t)q] = index(qt[q]);
    }
    return pe;
}

}  // namespace kb2e
