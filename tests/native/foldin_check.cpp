// foldin_check.cpp -- the host half of entity fold-in (kb2e_amd/csrc/foldin_host.hpp)
// against brute force: the grouping of the examples by free entity, the slot
// flags, the unit order, the bitmap, the known set, and every argument the
// plan must refuse.  Built with ASan + UBSan and run directly
// (tests/test_foldin_host.py); prints "ok".
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <tuple>

#include "foldin_host.hpp"

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

static FoldPlan plan_of(const Input& in) {
    return plan_fold(in.free.data(), (int64_t)in.free.size(), in.h.data(), in.t.data(), in.r.data(), (int64_t)in.h.size(),
                     in.kh.data(), in.kt.data(), in.kr.data(), (int64_t)in.kh.size(), in.ne, in.nr);
}

static bool refused(const Input& in) {
    try {
        plan_of(in);
    } catch (const std::invalid_argument&) {
        return true;
    }
    return false;
}

static Input random_input(std::mt19937_64& g, int64_t ne, int64_t nr, int nfree, int count, int nknown) {
    Input in;
    in.ne = ne;
    in.nr = nr;
    std::vector<int32_t> ids((size_t)ne);
    for (int64_t e = 0; e < ne; ++e) ids[(size_t)e] = (int32_t)e;
    std::shuffle(ids.begin(), ids.end(), g);
    in.free.assign(ids.begin(), ids.begin() + nfree);
    std::vector<int32_t> frozen(ids.begin() + nfree, ids.end());
    for (int k = 0; k < count; ++k) {
        const int32_t f = in.free[g() % in.free.size()], o = frozen[g() % frozen.size()];
        const bool head = g() & 1;
        in.h.push_back(head ? f : o);
        in.t.push_back(head ? o : f);
        in.r.push_back((int32_t)(g() % (uint64_t)nr));
    }
    for (int k = 0; k < nknown; ++k) {
        in.kh.push_back((int32_t)(g() % (uint64_t)ne));
        in.kt.push_back((int32_t)(g() % (uint64_t)ne));
        in.kr.push_back((int32_t)(g() % (uint64_t)nr));
    }
    return in;
}

static void check_plan(const Input& in) {
    const FoldPlan p = plan_of(in);
    const int64_t nfree = (int64_t)in.free.size(), count = (int64_t)in.h.size();
    CHECK((int64_t)p.off.size() == nfree + 1 && p.off[0] == 0 && p.off[(size_t)nfree] == count);
    CHECK((int64_t)p.perm.size() == count && (int64_t)p.slot.size() == count);
    // grouping: free entity f's list is exactly its examples, in the caller's order
    for (int64_t f = 0; f < nfree; ++f) {
        std::vector<int32_t> want;
        for (int64_t k = 0; k < count; ++k)
            if (in.h[(size_t)k] == in.free[(size_t)f] || in.t[(size_t)k] == in.free[(size_t)f]) want.push_back((int32_t)k);
        std::vector<int32_t> got(p.perm.begin() + p.off[(size_t)f], p.perm.begin() + p.off[(size_t)f + 1]);
        CHECK(got == want);
        for (int32_t k : got) CHECK(p.slot[(size_t)k] == (in.t[(size_t)k] == in.free[(size_t)f] ? 1 : 0));
    }
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
    // bitmap
    std::set<int32_t> fs(in.free.begin(), in.free.end());
    CHECK((int64_t)p.bitmap.size() == (in.ne + 63) / 64);
    for (int64_t e = 0; e < in.ne; ++e) CHECK(((p.bitmap[(size_t)(e >> 6)] >> (e & 63)) & 1) == (fs.count((int32_t)e) ? 1u : 0u));
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
    std::mt19937_64 g(20260101);
    check_plan(random_input(g, 12, 3, 2, 9, 7));
    check_plan(random_input(g, 40, 4, 5, 30, 60));
    check_plan(random_input(g, 64, 1, 63, 100, 0));    // one frozen entity; the bitmap's last bit of a word
    check_plan(random_input(g, 65, 2, 1, 0, 5));       // no examples at all
    check_plan(random_input(g, 3000, 7, 2000, 3100, 500));
    {
        Input in = random_input(g, 30, 3, 6, 0, 0);    // some free entities without examples, uneven work
        for (int k = 0; k < 20; ++k) {
            in.h.push_back(in.free[(size_t)(k % 3)]);
            in.t.push_back(0);
            in.r.push_back(k % 3);
        }
        // the tail must be frozen: take any entity that is not free
        std::set<int32_t> fs(in.free.begin(), in.free.end());
        int32_t frozen = 0;
        while (fs.count(frozen)) ++frozen;
        for (auto& t : in.t) t = frozen;
        check_plan(in);
    }

    // ---- refusals
    const Input ok = random_input(g, 20, 3, 4, 10, 5);
    CHECK(!refused(ok));
    std::set<int32_t> okfree(ok.free.begin(), ok.free.end());
    int32_t frozen = 0;
    while (okfree.count(frozen)) ++frozen;
    {
        Input in = ok;  // nfree < 1
        in.free.clear();
        CHECK(refused(in));
    }
    for (int32_t bad : {-1, 20}) {
        Input in = ok;  // ids out of range
        in.free[1] = bad;
        CHECK(refused(in));
        in = ok;
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
    for (int32_t bad : {-1, 3}) {
        Input in = ok;
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
    }
    {
        Input in = ok;  // no free entity in an example
        in.h[0] = in.t[0] = frozen;
        CHECK(refused(in));
        in = ok;  // the same free entity in both slots
        in.h[0] = in.t[0] = in.free[0];
        CHECK(refused(in));
        in = ok;  // two different free entities
        in.h[0] = in.free[0];
        in.t[0] = in.free[1];
        CHECK(refused(in));
    }
    {
        // NULL arrays with a count > 0
        bool threw = false;
        try {
            plan_fold(ok.free.data(), 4, nullptr, ok.t.data(), ok.r.data(), 10, nullptr, nullptr, nullptr, 0, 20, 3);
        } catch (const std::invalid_argument&) {
            threw = true;
        }
        CHECK(threw);
        threw = false;
        try {
            plan_fold(ok.free.data(), 4, ok.h.data(), ok.t.data(), ok.r.data(), 10, ok.kh.data(), nullptr, ok.kr.data(), 5, 20,
                      3);
        } catch (const std::invalid_argument&) {
            threw = true;
        }
        CHECK(threw);
        // ... and a count of 0 with NULL arrays is legal
        const FoldPlan p = plan_fold(ok.free.data(), 4, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, 20, 3);
        CHECK(p.off.back() == 0 && p.unit_free.size() == 4);
    }
    CHECK(fold_sweep_cap(0) == kFoldDefaultSweeps && fold_sweep_cap(7) == 7);
    std::puts("ok");
    return 0;
}
