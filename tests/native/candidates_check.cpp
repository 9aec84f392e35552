// candidates_check.cpp -- the host planner of the candidate-list calls
// (kb2e_amd/csrc/candidates_host.hpp) against brute force on random ragged
// lists, shared and private.  Stand-alone: built with ASan + UBSan by
// tests/test_candidates_host.py and run directly.  Prints "ok".
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <vector>

#include "candidates_host.hpp"

using namespace kb2e;

#define REQUIRE(cond)                                                          \
    do {                                                                       \
        if (!(cond)) {                                                         \
            printf("line %d: %s (case %d)\n", __LINE__, #cond, g_case);        \
            exit(1);                                                           \
        }                                                                      \
    } while (0)

static int g_case = 0;

template <typename F>
static bool throws(F&& f) {
    try {
        f();
    } catch (const std::invalid_argument&) {
        return true;
    }
    return false;
}

static void check_plan(std::mt19937_64& rng) {
    const int64_t ne = 1 + (int64_t)(rng() % 40), nr = 1 + (int64_t)(rng() % 5);
    const int64_t nlists = 1 + (int64_t)(rng() % 12);
    const bool shared = rng() % 2;
    const int64_t nq = shared ? 1 + (int64_t)(rng() % 30) : nlists;
    const int width = (rng() % 3 == 0) ? 1 + (int)(rng() % 64) : (rng() % 2 ? 64 : 63);
    const int64_t cap = 1 + (int64_t)(rng() % 300);
    const int64_t cap_queries = rng() % 4 == 0 ? 1 + (int64_t)(rng() % 5) : kCandidatesChunkQueries;
    const bool by_rel = rng() % 2, with_truth = rng() % 2;
    std::vector<int64_t> off(1, 0);
    std::vector<int32_t> cand;
    for (int64_t l = 0; l < nlists; ++l) {
        const int kind = (int)(rng() % 6);
        const int64_t len = kind == 0 ? 0 : kind == 1 ? 1 : kind == 2 ? 63 + (int64_t)(rng() % 3) : (int64_t)(rng() % 200);
        for (int64_t j = 0; j < len; ++j) cand.push_back((int32_t)(rng() % ne));
        off.push_back((int64_t)cand.size());
    }
    std::vector<int32_t> ent(nq), rel(nq), side(nq), truth(nq), lists(nq);
    for (int64_t q = 0; q < nq; ++q) {
        ent[q] = (int32_t)(rng() % ne);
        rel[q] = (int32_t)(rng() % nr);
        side[q] = (int32_t)(rng() % 2);
        truth[q] = (int32_t)(rng() % ne);
        lists[q] = (int32_t)(rng() % nlists);
    }
    const int32_t* lp = shared ? lists.data() : nullptr;
    check_candidates(ent.data(), rel.data(), side.data(), with_truth ? truth.data() : nullptr, lp, nq, off.data(),
                     cand.data(), nlists, ne, nr);
    const CandPlan p = plan_candidates(ent.data(), rel.data(), side.data(), with_truth ? truth.data() : nullptr, lp, nq,
                                       off.data(), cand.data(), ne, nr, width, cap, by_rel, cap_queries);
    auto list_of = [&](int64_t q) { return shared ? (int64_t)lists[q] : q; };
    auto len_of = [&](int64_t q) { return off[list_of(q) + 1] - off[list_of(q)]; };

    // the energy offsets are the prefix sums of the queries' list lengths
    std::vector<int64_t> start(nq + 1, 0);
    for (int64_t q = 0; q < nq; ++q) start[q + 1] = start[q] + len_of(q);
    REQUIRE(p.listings == start[nq]);

    // chunks: consecutive, whole queries, within the caps but for one oversize query
    int64_t q_next = 0, item_next = 0, group_next = 0, max_l = 0, max_i = 0;
    for (const CandChunk& c : p.chunks) {
        REQUIRE(c.q0 == q_next && c.q1 > c.q0 && c.q1 <= nq);
        REQUIRE(c.out0 == start[c.q0] && c.listings == start[c.q1] - start[c.q0]);
        REQUIRE(c.listings <= cap || c.q1 - c.q0 == 1);
        REQUIRE(c.q1 - c.q0 <= cap_queries);
        // greedy: the next query would not have fitted
        if (c.q1 < nq) REQUIRE(c.listings + len_of(c.q1) > cap || c.q1 - c.q0 == cap_queries);
        REQUIRE(c.item0 == item_next && c.group0 == group_next);
        q_next = c.q1;
        item_next += c.nitems;
        group_next += c.ngroups;
        max_l = std::max(max_l, c.listings);
        max_i = std::max(max_i, c.nitems);
        // every listing of the chunk in exactly one item, at its own output slot
        std::vector<int> seen((size_t)c.listings, 0);
        for (int64_t i = c.item0; i < c.item0 + c.nitems; ++i) {
            const CandItem& it = p.items[(size_t)i];
            REQUIRE(it.count >= 1 && it.count <= width && it.count <= kCandidatesWave);
            REQUIRE(it.query >= c.q0 && it.query < c.q1);
            const int64_t q = it.query;
            REQUIRE(it.ent == ent[q] && it.rel == rel[q] && it.side == side[q]);
            REQUIRE(it.truth == (with_truth ? truth[q] : -1));
            const int64_t first = off[list_of(q)];
            REQUIRE(it.first >= first && it.first + it.count <= first + len_of(q));
            REQUIRE(it.out == (start[q] - c.out0) + (it.first - first));
            for (int32_t j = 0; j < it.count; ++j) {
                REQUIRE(it.out + j < c.listings);
                ++seen[(size_t)(it.out + j)];
            }
        }
        for (int v : seen) REQUIRE(v == 1);
        // groups: they tile the chunk's items; by relation each holds one relation, ascending
        int64_t gi_next = c.item0;
        int32_t last_rel = -1;
        for (int64_t g = c.group0; g < c.group0 + c.ngroups; ++g) {
            const CandGroup& G = p.groups[(size_t)g];
            REQUIRE(G.item0 == gi_next && G.nitems >= 1);
            gi_next += G.nitems;
            if (!by_rel) {
                REQUIRE(G.rel == -1 && G.nents == 0);
                continue;
            }
            REQUIRE(G.rel > last_rel);
            last_rel = G.rel;
            // the remap: the distinct entities of the group, each once, nothing else
            std::set<int32_t> want;
            for (int64_t i = G.item0; i < G.item0 + G.nitems; ++i) {
                const CandItem& it = p.items[(size_t)i];
                REQUIRE(it.rel == G.rel);
                want.insert(it.ent);
                if (it.truth >= 0) want.insert(it.truth);
                for (int32_t j = 0; j < it.count; ++j) want.insert(cand[(size_t)(it.first + j)]);
            }
            std::vector<int32_t> remap((size_t)ne, -1);
            REQUIRE(G.nents == (int64_t)want.size());
            REQUIRE(G.nents <= p.max_distinct);
            for (int64_t u = 0; u < G.nents; ++u) {
                const int32_t x = p.distinct[(size_t)(G.ent0 + u)];
                REQUIRE(want.count(x) && remap[(size_t)x] == -1);
                remap[(size_t)x] = (int32_t)u;
            }
        }
        REQUIRE(gi_next == c.item0 + c.nitems);
    }
    REQUIRE(q_next == nq && item_next == (int64_t)p.items.size() && group_next == (int64_t)p.groups.size());
    REQUIRE(p.max_listings == max_l && p.max_items == max_i);
}

static void check_errors() {
    const int32_t e[2] = {0, 1}, r[2] = {0, 0}, s[2] = {0, 1}, t[2] = {1, 2}, l[2] = {0, 0}, c[3] = {0, 1, 2};
    const int64_t off[3] = {0, 1, 3};
    auto call = [&](const int32_t* ee, const int32_t* rr, const int32_t* ss, const int32_t* tt, const int32_t* ll, int64_t nq,
                    const int64_t* oo, const int32_t* cc, int64_t nl) {
        return throws([&] { check_candidates(ee, rr, ss, tt, ll, nq, oo, cc, nl, 3, 1); });
    };
    REQUIRE(!call(e, r, s, t, nullptr, 2, off, c, 2));
    REQUIRE(!call(e, r, s, nullptr, l, 2, off, c, 1));
    REQUIRE(call(e, r, s, t, nullptr, 0, off, c, 2));
    REQUIRE(call(e, r, s, t, nullptr, 2, off, c, 0));
    REQUIRE(call(e, r, s, t, nullptr, 2, off, c, 1));  // lists == NULL, nlists != nq
    REQUIRE(call(nullptr, r, s, t, nullptr, 2, off, c, 2));
    REQUIRE(call(e, r, s, t, nullptr, 2, off, nullptr, 2));
    const int64_t bad0[3] = {1, 1, 3}, dec[3] = {0, 2, 1}, big[3] = {0, 1, (int64_t)1 << 31};
    REQUIRE(call(e, r, s, t, nullptr, 2, bad0, c, 2));
    REQUIRE(call(e, r, s, t, nullptr, 2, dec, c, 2));
    REQUIRE(call(e, r, s, t, nullptr, 2, big, c, 2));
    const int32_t l2[2] = {0, 2}, lm[2] = {-1, 0}, s2[2] = {0, 2}, e3[2] = {0, 3}, r1[2] = {0, 1}, t3[2] = {-1, 0};
    const int32_t c3[3] = {0, 3, 2};
    REQUIRE(call(e, r, s, t, l2, 2, off, c, 2));
    REQUIRE(call(e, r, s, t, lm, 2, off, c, 2));
    REQUIRE(call(e, r, s2, t, nullptr, 2, off, c, 2));
    REQUIRE(call(e3, r, s, t, nullptr, 2, off, c, 2));
    REQUIRE(call(e, r1, s, t, nullptr, 2, off, c, 2));
    REQUIRE(call(e, r, s, t3, nullptr, 2, off, c, 2));
    REQUIRE(call(e, r, s, t, nullptr, 2, off, c3, 2));
    // empty lists only: no candidate array needed
    const int64_t none[3] = {0, 0, 0};
    REQUIRE(!call(e, r, s, t, nullptr, 2, none, nullptr, 2));
}

int main() {
    std::mt19937_64 rng(20240607);
    for (g_case = 0; g_case < 600; ++g_case) check_plan(rng);
    g_case = -1;
    check_errors();
    printf("ok\n");
    return 0;
}
