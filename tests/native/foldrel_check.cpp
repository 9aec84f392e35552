// foldrel_check.cpp -- the host half of relation fold-in
// (kb2e_amd/csrc/foldrel_host.hpp) against brute force: the grouping of the
// examples by free relation, the unit order, the longest group, the batch cap,
// the known set, and every argument the plan must refuse.  Built with ASan +
// UBSan and run directly (tests/test_foldrel_host.py); prints "ok".
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <tuple>

#include "foldrel_host.hpp"

using namespace kb2e;

#define CHECK(cond)                                                   \
    do {                                                              \
        if (!(cond)) {                                                \
            std::printf("%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                             \
        }                                                             \
    } while (0)

struct Input {
    int64_t ne, nr;
    std::vector<int32_t> free, h, t, r, kh, kt, kr;
};

static FoldRelPlan plan_of(const Input& in) {
    return plan_fold_rel(in.free.data(), (int64_t)in.free.size(), in.h.data(), in.t.data(), in.r.data(),
                         (int64_t)in.h.size(), in.kh.data(), in.kt.data(), in.kr.data(), (int64_t)in.kh.size(), in.ne,
                         in.nr);
}

static bool refused(const Input& in) {
    try {
        plan_of(in);
    } catch (const std::invalid_argument&) {
        return true;
    }
    return false;
}

// `skew`: most examples go to the first free relation
static Input random_input(std::mt19937_64& g, int64_t ne, int64_t nr, int nfree, int count, int nknown, bool skew = false) {
    Input in;
    in.ne = ne;
    in.nr = nr;
    std::vector<int32_t> ids((size_t)nr);
    for (int64_t r = 0; r < nr; ++r) ids[(size_t)r] = (int32_t)r;
    std::shuffle(ids.begin(), ids.end(), g);
    in.free.assign(ids.begin(), ids.begin() + nfree);
    for (int k = 0; k < count; ++k) {
        in.h.push_back((int32_t)(g() % (uint64_t)ne));
        in.t.push_back((int32_t)(g() % (uint64_t)ne));
        in.r.push_back(skew && g() % 4 ? in.free[0] : in.free[g() % in.free.size()]);
    }
    for (int k = 0; k < nknown; ++k) {
        in.kh.push_back((int32_t)(g() % (uint64_t)ne));
        in.kt.push_back((int32_t)(g() % (uint64_t)ne));
        in.kr.push_back((int32_t)(g() % (uint64_t)nr));
    }
    return in;
}

static void check_plan(const Input& in) {
    const FoldRelPlan p = plan_of(in);
    const int64_t nfree = (int64_t)in.free.size(), count = (int64_t)in.h.size();
    CHECK((int64_t)p.off.size() == nfree + 1 && p.off[0] == 0 && p.off[(size_t)nfree] == count);
    CHECK((int64_t)p.perm.size() == count);
    // grouping: free relation f's list is exactly its examples, in the caller's order
    int64_t longest = 0;
    for (int64_t f = 0; f < nfree; ++f) {
        std::vector<int32_t> want;
        for (int64_t k = 0; k < count; ++k)
            if (in.r[(size_t)k] == in.free[(size_t)f]) want.push_back((int32_t)k);
        std::vector<int32_t> got(p.perm.begin() + p.off[(size_t)f], p.perm.begin() + p.off[(size_t)f + 1]);
        CHECK(got == want);
        longest = std::max<int64_t>(longest, (int64_t)want.size());
    }
    CHECK(p.longest == longest);
    // units: a permutation of the free indices, work never rising, ties by index
    std::vector<int> seen((size_t)nfree, 0);
    for (int64_t u = 0; u < nfree; ++u) {
        const int32_t f = p.unit_free[(size_t)u];
        CHECK(f >= 0 && f < nfree && !seen[(size_t)f]++);
        if (u > 0) {
            const int32_t b = p.unit_free[(size_t)u - 1];
            const int64_t wb = p.off[(size_t)b + 1] - p.off[(size_t)b], wf = p.off[(size_t)f + 1] - p.off[(size_t)f];
            CHECK(wb > wf || (wb == wf && b < f));
        }
    }
    // known set = known + examples, nothing else
    const FilterSet set = fold_known_set(in.h.data(), in.t.data(), in.r.data(), count, in.kh.data(), in.kt.data(),
                                         in.kr.data(), (int64_t)in.kh.size(), in.ne, in.nr);
    std::set<std::tuple<int32_t, int32_t, int32_t>> want;
    for (int64_t k = 0; k < count; ++k) want.insert({in.h[(size_t)k], in.r[(size_t)k], in.t[(size_t)k]});
    for (size_t k = 0; k < in.kh.size(); ++k) want.insert({in.kh[k], in.kr[k], in.kt[k]});
    if (in.ne * in.nr * in.ne <= 40000) {
        for (int32_t h = 0; h < in.ne; ++h)
            for (int32_t r = 0; r < in.nr; ++r)
                for (int32_t t = 0; t < in.ne; ++t) CHECK(set.has(h, r, t) == (want.count({h, r, t}) > 0));
    } else {
        for (const auto& k : want) CHECK(set.has(std::get<0>(k), std::get<1>(k), std::get<2>(k)));
    }
}

int main() {
    std::mt19937_64 g(20260201);
    check_plan(random_input(g, 12, 3, 2, 9, 7));
    check_plan(random_input(g, 40, 6, 3, 30, 60));
    check_plan(random_input(g, 30, 5, 5, 100, 0));          // every relation is free
    check_plan(random_input(g, 65, 2, 1, 0, 5));            // no examples at all
    check_plan(random_input(g, 300, 90, 70, 200, 50));      // many relations, some without examples
    check_plan(random_input(g, 3000, 7, 4, 3100, 500, true));  // one long group

    // ---- refusals
    const Input ok = random_input(g, 20, 5, 3, 10, 5);
    CHECK(!refused(ok));
    std::set<int32_t> okfree(ok.free.begin(), ok.free.end());
    int32_t frozen = 0;
    while (okfree.count(frozen)) ++frozen;
    {
        Input in = ok;  // nfree < 1
        in.free.clear();
        in.h.clear(), in.t.clear(), in.r.clear();
        CHECK(refused(in));
    }
    for (int32_t bad : {-1, 20}) {
        Input in = ok;  // entity ids out of range
        in.h[3] = bad;
        CHECK(refused(in));
        in = ok;
        in.t[3] = bad;
        CHECK(refused(in));
        in = ok;
        in.kh[2] = bad;
        CHECK(refused(in));
        in = ok;
        in.kt[2] = bad;
        CHECK(refused(in));
    }
    for (int32_t bad : {-1, 5}) {
        Input in = ok;  // relation ids out of range
        in.free[1] = bad;
        CHECK(refused(in));
        in = ok;
        in.r[0] = bad;
        CHECK(refused(in));
        in = ok;
        in.kr[0] = bad;
        CHECK(refused(in));
    }
    {
        Input in = ok;  // a free id listed twice
        in.free[2] = in.free[0];
        CHECK(refused(in));
        in = ok;  // an example whose relation is not free
        in.r[4] = frozen;
        CHECK(refused(in));
    }
    {
        // NULL arrays with a count > 0
        bool threw = false;
        try {
            plan_fold_rel(ok.free.data(), 3, nullptr, ok.t.data(), ok.r.data(), 10, nullptr, nullptr, nullptr, 0, 20, 5);
        } catch (const std::invalid_argument&) {
            threw = true;
        }
        CHECK(threw);
        threw = false;
        try {
            plan_fold_rel(ok.free.data(), 3, ok.h.data(), ok.t.data(), ok.r.data(), 10, ok.kh.data(), nullptr, ok.kr.data(),
                          5, 20, 5);
        } catch (const std::invalid_argument&) {
            threw = true;
        }
        CHECK(threw);
        threw = false;
        try {
            plan_fold_rel(nullptr, 3, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, 20, 5);
        } catch (const std::invalid_argument&) {
            threw = true;
        }
        CHECK(threw);
        // ... and a count of 0 with NULL arrays is legal
        const FoldRelPlan p = plan_fold_rel(ok.free.data(), 3, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0,
                                            20, 5);
        CHECK(p.off.back() == 0 && p.unit_free.size() == 3 && p.longest == 0);
    }
    CHECK(fold_rel_batch_cap(1, 50) == 1 && fold_rel_batch_cap(300, 50) == 50 && fold_rel_batch_cap(7, 0) == 1 &&
          fold_rel_batch_cap(INT32_MAX, 2000) == 2000);
    CHECK(fold_sweep_cap(0) == kFoldDefaultSweeps && fold_sweep_cap(7) == 7);
    std::puts("ok");
    return 0;
}
