// joint_check.cpp -- the host half of the conjunctive queries
// (kb2e_amd/csrc/joint_host.hpp: the check of the offsets, the chunk plan and the
// per-query intersection of the known-candidate lists) against brute force, on
// the CPU (tests/test_joint_host.py builds this with ASan + UBSan and runs it).
#include <cstdint>
#include <cstdio>
#include <random>
#include <set>
#include <tuple>
#include <vector>

#include "joint_host.hpp"

namespace {

int fail(const char* what) {
    printf("%s\n", what);
    return 1;
}

int check_offsets() {
    using V = std::vector<int64_t>;
    auto ok = [](const V& o) { return kb2e::joint_check_offsets(o.data(), (int64_t)o.size() - 1) == nullptr; };
    if (!ok({0, 1}) || !ok({0, 64}) || !ok({0, 3, 4, 68}) || !ok({0, 1, 2, 3})) return fail("good offsets refused");
    if (ok({1, 2})) return fail("offsets starting at 1 accepted");
    if (ok({-1, 0})) return fail("offsets starting below 0 accepted");
    if (ok({0, 0})) return fail("an empty query accepted");
    if (ok({0, 2, 2, 3})) return fail("an empty query in the middle accepted");
    if (ok({0, 3, 2})) return fail("decreasing offsets accepted");
    if (ok({0, 65})) return fail("65 constraints accepted");
    if (ok({0, 5, 70})) return fail("65 constraints in the second query accepted");
    if (ok({0, INT64_MIN})) return fail("a hostile negative offset accepted");
    if (ok({0, INT64_MAX})) return fail("a hostile huge offset accepted");
    if (ok({0, 1, (int64_t)INT32_MAX + 1})) return fail("offsets past 2^31 - 1 accepted");
    const int64_t one[2] = {0, 1};
    if (kb2e::joint_check_offsets(one, 0) == nullptr) return fail("nq = 0 accepted");
    if (kb2e::joint_check_offsets(one, -3) == nullptr) return fail("nq < 0 accepted");
    if (kb2e::joint_check_offsets(nullptr, 1) == nullptr) return fail("NULL offsets accepted");
    std::vector<int64_t> big;
    for (int64_t v = 0; v <= 640; v += 64) big.push_back(v);
    if (!ok(big)) return fail("queries of 64 refused");
    return 0;
}

int check_plan(const std::vector<int64_t>& ms, int64_t cap) {
    std::vector<int64_t> off(1, 0);
    for (int64_t m : ms) off.push_back(off.back() + m);
    const int64_t nq = (int64_t)ms.size();
    int64_t maxm = 0;
    for (int64_t m : ms) maxm = std::max(maxm, m);
    if (kb2e::joint_max_constraints(off.data(), nq) != maxm) return fail("largest query miscounted");
    const int64_t budget = std::max(cap, maxm);
    const std::vector<kb2e::JointChunk> plan = kb2e::joint_plan_chunks(off.data(), nq, cap);
    int64_t next = 0;
    for (size_t i = 0; i < plan.size(); ++i) {
        const kb2e::JointChunk& ch = plan[i];
        if (ch.q0 != next) return fail("chunks skip or repeat a query");
        if (ch.q1 <= ch.q0 || ch.q1 > nq) return fail("empty or overlong chunk");
        const int64_t rows = off[(size_t)ch.q1] - off[(size_t)ch.q0];
        // (the budget is the cap unless a single query is larger than the cap)
        if (rows > budget) return fail("chunk over budget");
        // the longest run: the next query would not have fitted
        if (ch.q1 < nq && off[(size_t)ch.q1 + 1] - off[(size_t)ch.q0] <= budget) return fail("chunk not maximal");
        next = ch.q1;
    }
    if (next != nq) return fail("queries left over");
    return 0;
}

int check_plans() {
    // the chunking case of the GPU test: [1,2] [3] [5] [4,1] [1,3]
    const std::vector<int64_t> ms = {1, 2, 3, 5, 4, 1, 1, 3};
    std::vector<int64_t> off(1, 0);
    for (int64_t m : ms) off.push_back(off.back() + m);
    const auto plan = kb2e::joint_plan_chunks(off.data(), 8, 5);
    const int64_t want[5][2] = {{0, 2}, {2, 3}, {3, 4}, {4, 6}, {6, 8}};
    if (plan.size() != 5) return fail("the 5-row plan has not five chunks");
    for (int i = 0; i < 5; ++i)
        if (plan[(size_t)i].q0 != want[i][0] || plan[(size_t)i].q1 != want[i][1]) return fail("the 5-row plan differs");
    if (kb2e::joint_plan_chunks(off.data(), 8, 1000).size() != 1) return fail("a roomy budget makes more than one chunk");
    if (kb2e::joint_plan_chunks(off.data(), 8, 1).size() != 5) return fail("cap 1 does not rise to the largest query");
    const int64_t three[2] = {0, 3};
    if (kb2e::joint_plan_chunks(three, 1, 1).size() != 1) return fail("a query larger than the cap is split or lost");
    std::mt19937 rng(12345);
    for (int it = 0; it < 400; ++it) {
        const int nq = 1 + (int)(rng() % 40);
        std::vector<int64_t> m((size_t)nq);
        for (auto& v : m) v = 1 + (int64_t)(rng() % (it % 3 == 0 ? 64 : 6));
        for (int64_t cap : {(int64_t)1, (int64_t)2, (int64_t)5, (int64_t)17, (int64_t)64, (int64_t)100, (int64_t)100000})
            if (check_plan(m, cap)) {
                printf("plan case %d cap %lld\n", it, (long long)cap);
                return 1;
            }
    }
    return 0;
}

int check_intersections() {
    std::mt19937 rng(777);
    for (int it = 0; it < 300; ++it) {
        const int ne = 2 + (int)(rng() % 12), nr = 1 + (int)(rng() % 3);
        const int nq = 1 + (int)(rng() % 8);
        std::vector<int64_t> off(1, 0);
        std::vector<int32_t> qe, qr, qs;
        for (int q = 0; q < nq; ++q) {
            const int m = 1 + (int)(rng() % 4);
            for (int c = 0; c < m; ++c) {
                if (c > 0 && rng() % 4 == 0) {  // a repeated constraint
                    const size_t src = (size_t)off.back() + rng() % (size_t)c;
                    qe.push_back(qe[src]), qr.push_back(qr[src]), qs.push_back(qs[src]);
                } else {
                    qe.push_back((int32_t)(rng() % ne)), qr.push_back((int32_t)(rng() % nr)), qs.push_back((int32_t)(rng() % 2));
                }
            }
            off.push_back((int64_t)qe.size());
        }
        // a dense random filter with duplicates (it % 5 == 0: none at all)
        std::vector<int32_t> fh, ft, fr;
        const int nf = it % 5 == 0 ? 0 : (int)(rng() % (unsigned)(ne * ne * nr * 2));
        for (int f = 0; f < nf; ++f) {
            if (f > 0 && rng() % 5 == 0) {
                const size_t src = rng() % (size_t)f;
                fh.push_back(fh[src]), ft.push_back(ft[src]), fr.push_back(fr[src]);
            } else {
                fh.push_back((int32_t)(rng() % ne)), ft.push_back((int32_t)(rng() % ne)), fr.push_back((int32_t)(rng() % nr));
            }
        }
        std::set<std::tuple<int, int, int>> known;
        for (int f = 0; f < nf; ++f) known.insert({fh[(size_t)f], ft[(size_t)f], fr[(size_t)f]});
        const kb2e::KnownCandidates kc = kb2e::build_known_candidates(qe.data(), qr.data(), qs.data(), (int64_t)qe.size(),
                                                                     fh.data(), ft.data(), fr.data(), nf, nr);
        const kb2e::JointKnown jk = kb2e::joint_intersect_known(off.data(), nq, kc);
        if (jk.off.size() != (size_t)nq + 1 || jk.off[0] != 0 || jk.off.back() != (int64_t)jk.ids.size())
            return fail("intersection offsets malformed");
        for (int q = 0; q < nq; ++q) {
            std::vector<int32_t> want;
            for (int x = 0; x < ne; ++x) {
                bool all = true;
                for (int64_t c = off[(size_t)q]; c < off[(size_t)q + 1] && all; ++c) {
                    const int e = qe[(size_t)c], r = qr[(size_t)c];
                    all = qs[(size_t)c] ? known.count({e, x, r}) > 0 : known.count({x, e, r}) > 0;
                }
                if (all) want.push_back(x);
            }
            const std::vector<int32_t> got(jk.ids.begin() + jk.off[(size_t)q], jk.ids.begin() + jk.off[(size_t)q + 1]);
            if (got != want) {
                printf("intersection case %d query %d\n", it, q);
                return 1;
            }
        }
    }
    return 0;
}

}  // namespace

int main() {
    if (check_offsets() || check_plans() || check_intersections()) return 1;
    printf("ok\n");
    return 0;
}
