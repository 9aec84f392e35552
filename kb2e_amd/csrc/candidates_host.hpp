// candidates_host.hpp -- host side of the candidate-list calls
// (kb2e_score_candidates / kb2e_rank_candidates, candidates.hip), free of HIP
// so that it can be checked on the CPU (tests/native/candidates_check.cpp).
//
// * check_candidates: the argument checks of both calls (std::invalid_argument).
// * plan_candidates: cuts every query's list into wave-sized work items
//   (query, first listing, count <= width) and the queries into chunks whose
//   listings fit a cap (a query is never split; one that is longer than the cap
//   is a chunk of its own).  A list that many queries name is never expanded:
//   an item points into the caller's candidate array.  For TransR the items of
//   a chunk are grouped by relation and every group gets the distinct entities
//   it touches (anchors, truths, listings) in order of first appearance: the
//   columns of its compact projection.
#pragma once

#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

namespace kb2e {

constexpr int kCandidatesWave = 64;                                 // listings of a work item: the lanes of a wave
constexpr int64_t kCandidatesChunkListings = (int64_t)1 << 21;      // the default cap on a chunk's listings
constexpr int64_t kCandidatesChunkQueries = (int64_t)1 << 20;       // ... and on its queries
constexpr int64_t kCandidatesMaxListings = ((int64_t)1 << 31) - 1;  // offsets[nlists]

// One wave's work: `count` listings candidates[first .. first + count - 1] of
// one query, which is carried along so that no query array goes to the device.
struct CandItem {
    int32_t ent, rel, side, truth;  // truth: -1 when the call has none
    int32_t first, count;           // 1 <= count <= width
    int32_t out;                    // of its first listing among the chunk's energies
    int32_t query;
};
static_assert(sizeof(CandItem) == 32, "uploaded as it is");

// A run of a chunk's items that share a projection (TransR: a relation; else the whole chunk).
struct CandGroup {
    int32_t rel;            // -1: no projection
    int64_t item0, nitems;  // into CandPlan::items
    int64_t ent0, nents;    // into CandPlan::distinct
};

struct CandChunk {
    int64_t q0, q1;           // its queries [q0, q1)
    int64_t out0, listings;   // its energies are [out0, out0 + listings) of the output
    int64_t item0, nitems;    // into CandPlan::items
    int64_t group0, ngroups;  // into CandPlan::groups
};

struct CandPlan {
    std::vector<CandItem> items;
    std::vector<CandGroup> groups;
    std::vector<CandChunk> chunks;
    std::vector<int32_t> distinct;
    int64_t listings = 0;      // of the whole call
    int64_t max_listings = 0;  // of a chunk
    int64_t max_items = 0;     // of a chunk
    int64_t max_distinct = 0;  // of a group
};

inline void check_candidates(const int32_t* ent, const int32_t* rel, const int32_t* side, const int32_t* truth,
                             const int32_t* lists, int64_t nq, const int64_t* offsets, const int32_t* candidates,
                             int64_t nlists, int64_t ne, int64_t nr) {
    if (nq < 1) throw std::invalid_argument("no queries");
    if (nlists < 1) throw std::invalid_argument("no candidate lists");
    if (!ent || !rel || !side || !offsets) throw std::invalid_argument("a NULL array with a count > 0");
    if (!lists && nlists != nq) throw std::invalid_argument("lists == NULL needs one list per query");
    if (offsets[0] != 0) throw std::invalid_argument("offsets[0] must be 0");
    for (int64_t l = 0; l < nlists; ++l)
        if (offsets[l + 1] < offsets[l]) throw std::invalid_argument("offsets must not decrease");
    if (offsets[nlists] > kCandidatesMaxListings) throw std::invalid_argument("more than 2^31 - 1 listings");
    if (offsets[nlists] > 0 && !candidates) throw std::invalid_argument("a NULL array with a count > 0");
    for (int64_t q = 0; q < nq; ++q) {
        if (side[q] != 0 && side[q] != 1) throw std::invalid_argument("query side must be 0 (head) or 1 (tail)");
        if (ent[q] < 0 || ent[q] >= ne || rel[q] < 0 || rel[q] >= nr)
            throw std::invalid_argument("query " + std::to_string(q) + " has an id out of range");
        if (truth && (truth[q] < 0 || truth[q] >= ne))
            throw std::invalid_argument("truth " + std::to_string(q) + " is out of range");
        if (lists && (lists[q] < 0 || lists[q] >= nlists))
            throw std::invalid_argument("query " + std::to_string(q) + " names no list");
    }
    for (int64_t x = 0; x < offsets[nlists]; ++x)
        if (candidates[x] < 0 || candidates[x] >= ne)
            throw std::invalid_argument("candidate " + std::to_string(x) + " is out of range");
}

// Checked arguments (check_candidates).  width: listings per item, 1..64;
// cap >= 1: listings per chunk; by_relation: group a chunk's items by relation
// and list every group's distinct entities (TransR).
inline CandPlan plan_candidates(const int32_t* ent, const int32_t* rel, const int32_t* side, const int32_t* truth,
                                const int32_t* lists, int64_t nq, const int64_t* offsets, const int32_t* candidates,
                                int64_t ne, int64_t nr, int width, int64_t cap, bool by_relation,
                                int64_t cap_queries = kCandidatesChunkQueries) {
    CandPlan p;
    std::vector<int64_t> stamp(by_relation ? (size_t)ne : 0, -1);
    std::vector<int64_t> count, start;
    std::vector<CandItem> sorted;
    int64_t out_total = 0;
    for (int64_t q0 = 0; q0 < nq;) {
        CandChunk c{};
        c.q0 = q0;
        c.out0 = out_total;
        c.item0 = (int64_t)p.items.size();
        c.group0 = (int64_t)p.groups.size();
        int64_t q = q0;
        for (; q < nq && q - q0 < cap_queries; ++q) {
            const int64_t l = lists ? lists[q] : q;
            const int64_t first = offsets[l], len = offsets[l + 1] - first;
            if (q > q0 && c.listings + len > cap) break;
            for (int64_t j = 0; j < len; j += width) {
                CandItem it;
                it.ent = ent[q];
                it.rel = rel[q];
                it.side = side[q];
                it.truth = truth ? truth[q] : -1;
                it.first = (int32_t)(first + j);
                it.count = (int32_t)std::min<int64_t>(width, len - j);
                it.out = (int32_t)(c.listings + j);
                it.query = (int32_t)q;
                p.items.push_back(it);
            }
            c.listings += len;
        }
        c.q1 = q;
        c.nitems = (int64_t)p.items.size() - c.item0;
        if (!by_relation) {
            if (c.nitems > 0) p.groups.push_back(CandGroup{-1, c.item0, c.nitems, 0, 0});
        } else if (c.nitems > 0) {
            // a stable counting sort of the chunk's items on the relation
            count.assign((size_t)nr + 1, 0);
            for (int64_t i = 0; i < c.nitems; ++i) ++count[(size_t)p.items[(size_t)(c.item0 + i)].rel + 1];
            for (int64_t r = 0; r < nr; ++r) count[(size_t)r + 1] += count[(size_t)r];
            start = count;
            sorted.resize((size_t)c.nitems);
            for (int64_t i = 0; i < c.nitems; ++i) {
                const CandItem& it = p.items[(size_t)(c.item0 + i)];
                sorted[(size_t)start[(size_t)it.rel]++] = it;
            }
            std::copy(sorted.begin(), sorted.end(), p.items.begin() + c.item0);
            for (int64_t r = 0; r < nr; ++r) {
                const int64_t i0 = count[(size_t)r], i1 = count[(size_t)r + 1];
                if (i0 == i1) continue;
                CandGroup g{(int32_t)r, c.item0 + i0, i1 - i0, (int64_t)p.distinct.size(), 0};
                const int64_t mark = (int64_t)p.groups.size();
                auto see = [&](int32_t x) {
                    if (stamp[(size_t)x] != mark) {
                        stamp[(size_t)x] = mark;
                        p.distinct.push_back(x);
                    }
                };
                for (int64_t i = g.item0; i < g.item0 + g.nitems; ++i) {
                    const CandItem& it = p.items[(size_t)i];
                    see(it.ent);
                    if (it.truth >= 0) see(it.truth);
                    for (int32_t j = 0; j < it.count; ++j) see(candidates[it.first + j]);
                }
                g.nents = (int64_t)p.distinct.size() - g.ent0;
                p.max_distinct = std::max(p.max_distinct, g.nents);
                p.groups.push_back(g);
            }
        }
        c.ngroups = (int64_t)p.groups.size() - c.group0;
        p.max_listings = std::max(p.max_listings, c.listings);
        p.max_items = std::max(p.max_items, c.nitems);
        out_total += c.listings;
        p.chunks.push_back(c);
        q0 = q;
    }
    p.listings = out_total;
    return p;
}

}  // namespace kb2e
