// predict_check.cpp -- the known-candidate builder of the top-k queries
// (kb2e_amd/csrc/predict_host.hpp) against a brute-force loop, on the CPU
// (tests/test_predict_host.py builds this with ASan + UBSan and runs it).
#include <cstdint>
#include <cstdio>
#include <random>
#include <set>
#include <vector>

#include "predict_host.hpp"

namespace {

struct Case {
    int ne, nr;
    std::vector<int32_t> qe, qr, qs, fh, ft, fr;
};

int check(const char* name, const Case& c) {
    const int64_t nq = (int64_t)c.qe.size(), nf = (int64_t)c.fh.size();
    const kb2e::KnownCandidates kc = kb2e::build_known_candidates(
        c.qe.data(), c.qr.data(), c.qs.data(), nq, nf ? c.fh.data() : nullptr, nf ? c.ft.data() : nullptr,
        nf ? c.fr.data() : nullptr, nf, c.nr);
    if ((int64_t)kc.group.size() != nq || kc.off.empty() || kc.off[0] != 0 ||
        kc.off.back() != (int64_t)kc.ids.size()) {
        printf("%s: malformed lists\n", name);
        return 1;
    }
    for (int64_t q = 0; q < nq; ++q) {
        std::set<int32_t> want;  // brute force: every filter triple against this query
        for (int64_t k = 0; k < nf; ++k) {
            if (c.fr[k] != c.qr[q]) continue;
            if (c.qs[q] == 1 && c.fh[k] == c.qe[q]) want.insert(c.ft[k]);
            if (c.qs[q] == 0 && c.ft[k] == c.qe[q]) want.insert(c.fh[k]);
        }
        const int32_t g = kc.group[(size_t)q];
        if (g < 0 || (size_t)g + 1 >= kc.off.size()) {
            printf("%s: query %lld has list %d out of range\n", name, (long long)q, g);
            return 1;
        }
        const std::vector<int32_t> got(kc.ids.begin() + kc.off[(size_t)g], kc.ids.begin() + kc.off[(size_t)g + 1]);
        const std::vector<int32_t> exp(want.begin(), want.end());  // ascending, distinct
        if (got != exp) {
            printf("%s: query %lld (e %d, r %d, side %d): %zu candidates, expected %zu\n", name, (long long)q,
                   c.qe[q], c.qr[q], c.qs[q], got.size(), exp.size());
            return 1;
        }
        for (int64_t p = 0; p < q; ++p)  // queries that share (e, r, side) share one list, others do not
            if ((c.qe[p] == c.qe[q] && c.qr[p] == c.qr[q] && c.qs[p] == c.qs[q]) != (kc.group[(size_t)p] == g)) {
                printf("%s: queries %lld and %lld grouped wrongly\n", name, (long long)p, (long long)q);
                return 1;
            }
    }
    return 0;
}

Case random_case(uint32_t seed, int ne, int nr, int nq, int nf, bool duplicates) {
    std::mt19937 g(seed);
    Case c;
    c.ne = ne;
    c.nr = nr;
    for (int k = 0; k < nf; ++k) {
        c.fh.push_back((int32_t)(g() % ne));
        c.ft.push_back((int32_t)(g() % ne));
        c.fr.push_back((int32_t)(g() % nr));
        if (duplicates && k % 3 == 0) {  // the same triple again
            c.fh.push_back(c.fh.back());
            c.ft.push_back(c.ft.back());
            c.fr.push_back(c.fr.back());
        }
    }
    for (int k = 0; k < nq; ++k) {
        if (k % 4 == 3 && k > 0) {  // a repeated query
            const size_t p = g() % c.qe.size();
            c.qe.push_back(c.qe[p]);
            c.qr.push_back(c.qr[p]);
            c.qs.push_back(c.qs[p]);
        } else {
            c.qe.push_back((int32_t)(g() % ne));
            c.qr.push_back((int32_t)(g() % nr));
            c.qs.push_back((int32_t)(g() % 2));
        }
    }
    return c;
}

}  // namespace

int main() {
    int bad = 0;
    bad += check("empty filter", random_case(1, 50, 4, 40, 0, false));
    bad += check("both sides", random_case(2, 30, 3, 200, 600, false));
    bad += check("duplicate filter triples", random_case(3, 20, 2, 100, 500, true));
    bad += check("one query", random_case(4, 10, 1, 1, 80, true));
    bad += check("sparse", random_case(5, 5000, 40, 300, 2000, false));
    {
        // h == t filter triples and a query entity on both sides of one relation
        Case c{4, 1, {1, 1, 2}, {0, 0, 0}, {1, 0, 0}, {1, 1, 3, 1}, {1, 2, 1, 1}, {0, 0, 0, 0}};
        bad += check("self loops", c);
    }
    if (bad) return 1;
    printf("ok\n");
    return 0;
}
