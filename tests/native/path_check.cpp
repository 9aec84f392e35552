// Host check of the path queries' plan (kb2e_amd/csrc/path_host.hpp) against
// brute force: the offsets check, the chunk plan, the chunk order and the level
// plan, the walk of the filter triples along a path and the back-tracking of a
// winning path.  Stand-alone; tests/test_path_host.py builds it with ASan +
// UBSan and runs it.  Prints "ok".
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <tuple>

#include "path_host.hpp"

using namespace kb2e;

#define REQUIRE(cond)                                                   \
    do {                                                                \
        if (!(cond)) {                                                  \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            exit(1);                                                    \
        }                                                               \
    } while (0)

static void check_offsets() {
    const int64_t good[] = {0, 1, 9, 12};
    REQUIRE(path_check_offsets(good, 3) == nullptr);
    REQUIRE(path_check_offsets(good, 0) != nullptr);
    REQUIRE(path_check_offsets(good, -1) != nullptr);
    REQUIRE(path_check_offsets(nullptr, 3) != nullptr);
    const int64_t bad[][4] = {{1, 2, 3, 4},    // does not start at 0
                              {0, 0, 3, 4},    // a query without hops
                              {0, 3, 2, 4},    // decreasing
                              {0, 1, 10, 11},  // nine hops
                              {-1, 1, 2, 3},
                              {0, 1, 2, INT64_MAX},          // hostile: the difference must not overflow
                              {0, INT64_MIN, 2, 3},
                              {0, 1, INT64_MAX, INT64_MIN},
                              {0, 8, 16, (int64_t)INT32_MAX + 1}};
    for (const auto& b : bad) REQUIRE(path_check_offsets(b, 3) != nullptr);
    const int64_t eight[] = {0, 8};
    REQUIRE(path_check_offsets(eight, 1) == nullptr);
    const int64_t nine[] = {0, 9};
    REQUIRE(path_check_offsets(nine, 1) != nullptr);
}

static void check_units() {
    REQUIRE(path_query_units(1, false) == 2 && path_query_units(1, true) == 2);
    REQUIRE(path_query_units(2, false) == 3 && path_query_units(8, false) == 3);
    REQUIRE(path_query_units(2, true) == 5 && path_query_units(8, true) == 11);
}

static void check_chunks(std::mt19937& rng) {
    for (int round = 0; round < 400; ++round) {
        const int64_t nq = 1 + rng() % 40;
        std::vector<int64_t> off(1, 0);
        for (int64_t q = 0; q < nq; ++q) off.push_back(off.back() + 1 + rng() % kPathMaxHops);
        const bool exact = rng() & 1;
        const int64_t budget = 1 + rng() % 40, cap = 1 + rng() % 12;
        int64_t largest = 0;
        for (int64_t q = 0; q < nq; ++q) largest = std::max(largest, path_query_units(off[q + 1] - off[q], exact));
        const int64_t limit = std::max(budget, largest);
        const auto chunks = path_plan_chunks(off.data(), nq, exact, budget, cap);
        int64_t next = 0;
        for (size_t c = 0; c < chunks.size(); ++c) {
            REQUIRE(chunks[c].q0 == next && chunks[c].q1 > chunks[c].q0);  // every query once, in order
            next = chunks[c].q1;
            int64_t units = 0;
            for (int64_t q = chunks[c].q0; q < chunks[c].q1; ++q) units += path_query_units(off[q + 1] - off[q], exact);
            REQUIRE(units <= limit && chunks[c].q1 - chunks[c].q0 <= cap);
            if (next < nq)  // maximal: the next query would not have fitted
                REQUIRE(chunks[c].q1 - chunks[c].q0 == cap ||
                        units + path_query_units(off[next + 1] - off[next], exact) > limit);
        }
        REQUIRE(next == nq);
    }
    const int64_t off[] = {0, 1, 3, 6, 7, 8};  // units under beam search: 2 3 3 2 2
    const auto c = path_plan_chunks(off, 5, false, 5, 100);
    REQUIRE(c.size() == 3 && c[0].q1 == 2 && c[1].q1 == 4 && c[2].q1 == 5);
    const auto one = path_plan_chunks(off, 5, true, 1, 100);  // the budget rises to the largest query (6)
    REQUIRE(one.size() == 4 && one[0].q1 == 1 && one[1].q1 == 2 && one[2].q1 == 3 && one[3].q1 == 5);
}

static void check_levels(std::mt19937& rng) {
    for (int round = 0; round < 300; ++round) {
        const int64_t nq = 1 + rng() % 30, nr = 1 + rng() % 4;
        std::vector<int64_t> off(1, 0);
        for (int64_t q = 0; q < nq; ++q) off.push_back(off.back() + 1 + rng() % kPathMaxHops);
        std::vector<int32_t> rel((size_t)off.back()), side((size_t)off.back());
        for (auto& r : rel) r = (int32_t)(rng() % nr);
        for (auto& s : side) s = (int32_t)(rng() & 1);
        const int64_t q0 = rng() % nq, q1 = q0 + 1 + rng() % (nq - q0);
        const auto order = path_chunk_order(off.data(), rel.data(), side.data(), q0, q1);
        std::vector<int64_t> sorted(order);
        std::sort(sorted.begin(), sorted.end());
        for (int64_t x = 0; x < q1 - q0; ++x) REQUIRE(sorted[(size_t)x] == q0 + x);  // a permutation of the chunk
        auto len = [&](int64_t q) { return off[q + 1] - off[q]; };
        for (size_t x = 1; x < order.size(); ++x) {
            const int64_t a = order[x - 1], b = order[x];
            REQUIRE(len(a) >= len(b));
            if (len(a) == len(b)) {
                const auto ka = std::make_tuple(rel[off[a]], side[off[a]]), kb = std::make_tuple(rel[off[b]], side[off[b]]);
                REQUIRE(ka <= kb);
                if (ka == kb) REQUIRE(a < b);  // stable
            }
        }
        for (int level = 1; level <= kPathMaxHops + 1; ++level) {
            int64_t live = 0;
            for (int64_t q : order) live += len(q) >= level;
            REQUIRE(path_live(off.data(), order, level) == live);
            for (int64_t x = 0; x < (int64_t)order.size(); ++x) REQUIRE((len(order[(size_t)x]) >= level) == (x < live));
            if (level > kPathMaxHops) continue;
            const PathLevel pl = path_plan_level(off.data(), rel.data(), side.data(), order, level);
            REQUIRE((int64_t)pl.row.size() == live && pl.rel.size() == pl.row.size() && pl.side.size() == pl.row.size());
            std::vector<int> seen((size_t)live, 0);
            std::set<int32_t> distinct;
            for (int64_t s = 0; s < live; ++s) {
                const int32_t row = pl.row[(size_t)s];
                REQUIRE(row >= 0 && row < live && !seen[(size_t)row]++);  // each live query once
                const int64_t hop = off[order[(size_t)row]] + level - 1;
                REQUIRE(pl.rel[(size_t)s] == rel[hop] && pl.side[(size_t)s] == side[hop]);
                distinct.insert(rel[hop]);
                if (s > 0) {
                    const auto ka = std::make_tuple(pl.rel[(size_t)s - 1], pl.side[(size_t)s - 1]);
                    const auto kb = std::make_tuple(pl.rel[(size_t)s], pl.side[(size_t)s]);
                    REQUIRE(ka <= kb);
                    if (ka == kb) REQUIRE(pl.row[(size_t)s - 1] < row);  // stable
                }
            }
            REQUIRE(pl.relations == (int64_t)distinct.size());
        }
    }
}

// S_L by enumeration of every filter path
static std::set<int32_t> brute_known(const std::set<std::tuple<int, int, int>>& filt, int anchor, const int32_t* rel,
                                     const int32_t* side, int hops, bool no_loops) {
    std::set<int32_t> ends;
    std::vector<int> path(1, anchor);
    std::vector<std::tuple<int, int, int>> list(filt.begin(), filt.end());
    auto rec = [&](auto&& self, int level, int at) -> void {
        if (level == hops) {
            ends.insert(at);
            return;
        }
        for (const auto& [h, t, r] : list) {
            if (r != rel[level] || (no_loops && h == t)) continue;
            if (side[level] == 1 && h == at) self(self, level + 1, t);
            if (side[level] == 0 && t == at) self(self, level + 1, h);
        }
    };
    rec(rec, 0, anchor);
    return ends;
}

static void check_known(std::mt19937& rng) {
    for (int round = 0; round < 300; ++round) {
        const int ne = 2 + (int)(rng() % 7), nr = 1 + (int)(rng() % 3);
        const int nf = (int)(rng() % 25);
        std::vector<int32_t> fh, ft, fr;
        std::set<std::tuple<int, int, int>> fset;
        for (int x = 0; x < nf; ++x) {
            int h = (int)(rng() % ne), t = rng() % 4 == 0 ? h : (int)(rng() % ne), r = (int)(rng() % nr);
            const int copies = 1 + (rng() % 3 == 0);  // duplicates count once
            for (int c = 0; c < copies; ++c) fh.push_back(h), ft.push_back(t), fr.push_back(r);
            fset.insert({h, t, r});
        }
        const int64_t nq = 1 + rng() % 6;
        std::vector<int64_t> off(1, 0);
        std::vector<int32_t> anchors;
        for (int64_t q = 0; q < nq; ++q) {
            off.push_back(off.back() + 1 + rng() % 4);
            anchors.push_back((int32_t)(rng() % ne));
        }
        std::vector<int32_t> rel((size_t)off.back()), side((size_t)off.back());
        for (auto& r : rel) r = (int32_t)(rng() % nr);
        for (auto& s : side) s = (int32_t)(rng() & 1);
        for (int nl = 0; nl < 2; ++nl) {
            const PathKnown pk = path_known_answers(anchors.data(), off.data(), rel.data(), side.data(), nq, nl != 0,
                                                    fh.data(), ft.data(), fr.data(), (int64_t)fh.size(), nr);
            REQUIRE((int64_t)pk.off.size() == nq + 1 && pk.off[0] == 0 && pk.off[(size_t)nq] == (int64_t)pk.ids.size());
            for (int64_t q = 0; q < nq; ++q) {
                const auto want = brute_known(fset, anchors[(size_t)q], rel.data() + off[q], side.data() + off[q],
                                              (int)(off[q + 1] - off[q]), nl != 0);
                const std::vector<int32_t> got(pk.ids.begin() + pk.off[(size_t)q], pk.ids.begin() + pk.off[(size_t)q + 1]);
                REQUIRE(got == std::vector<int32_t>(want.begin(), want.end()));  // ascending, distinct
            }
        }
    }
    // no filter: nothing is known
    const int32_t a[] = {3}, r[] = {0, 0}, s[] = {1, 0};
    const int64_t off[] = {0, 2};
    const PathKnown none = path_known_answers(a, off, r, s, 1, false, nullptr, nullptr, nullptr, 0, 1);
    REQUIRE(none.ids.empty() && none.off.size() == 2 && none.off[1] == 0);
}

static void check_backtrack() {
    const int W = kPathMaxHops - 1;
    int32_t via[W];
    REQUIRE(path_backtrack(1, 4, nullptr, nullptr, 0, -1, via));
    for (int i = 0; i < W; ++i) REQUIRE(via[i] == -1);
    // beam 3, four hops; the level stride is 5 (rows of other queries lie between the levels)
    //            level 1          level 2          level 3
    const int32_t fid[] = {7, 2, 9, 0, 0, 4, 7, -1, 0, 0, 5, 1, 8};
    const int32_t back[] = {0, 0, 0, 0, 0, 9, 2, -1, 0, 0, 7, 7, 4};  // (level 1 has none)
    REQUIRE(path_backtrack(4, 3, fid, back, 5, 8, via));  // 8 <- 4 <- 9
    REQUIRE(via[0] == 9 && via[1] == 4 && via[2] == 8 && via[3] == -1 && via[6] == -1);
    REQUIRE(path_backtrack(4, 3, fid, back, 5, 1, via));  // 1 <- 7 <- 2
    REQUIRE(via[0] == 2 && via[1] == 7 && via[2] == 1 && via[3] == -1);
    REQUIRE(path_backtrack(2, 3, fid, back, 5, 9, via));
    REQUIRE(via[0] == 9 && via[1] == -1);
    REQUIRE(path_backtrack(3, 3, fid, back, 5, 7, via));  // level 2's entry 7 <- 2
    REQUIRE(via[0] == 2 && via[1] == 7 && via[2] == -1);
    REQUIRE(!path_backtrack(4, 3, fid, back, 5, 6, via));  // 6 is in no frontier
    for (int i = 0; i < W; ++i) REQUIRE(via[i] == -1);
    REQUIRE(!path_backtrack(2, 3, fid, back, 5, -1, via));  // an answer without a predecessor
}

int main() {
    std::mt19937 rng(12345);
    check_offsets();
    check_units();
    check_chunks(rng);
    check_levels(rng);
    check_known(rng);
    check_backtrack();
    printf("ok\n");
    return 0;
}
