// relpred_check.cpp -- the host half of relation prediction
// (kb2e_amd/csrc/predict_host.hpp: the known relations of every (head, tail)
// pair and the distinct-entity list of a run of pairs) against brute-force
// loops, on the CPU (tests/test_relpred_host.py builds this with ASan + UBSan
// and runs it).
#include <cstdint>
#include <cstdio>
#include <random>
#include <set>
#include <vector>

#include "predict_host.hpp"

namespace {

struct Case {
    int ne, nr;
    std::vector<int32_t> qh, qt, fh, ft, fr;
};

int check(const char* name, const Case& c) {
    const int64_t nq = (int64_t)c.qh.size(), nf = (int64_t)c.fh.size();
    const kb2e::KnownCandidates kc =
        kb2e::build_known_relations(c.qh.data(), c.qt.data(), nq, nf ? c.fh.data() : nullptr,
                                    nf ? c.ft.data() : nullptr, nf ? c.fr.data() : nullptr, nf, c.ne);
    if ((int64_t)kc.group.size() != nq || kc.off.empty() || kc.off[0] != 0 ||
        kc.off.back() != (int64_t)kc.ids.size()) {
        printf("%s: malformed lists\n", name);
        return 1;
    }
    for (int64_t q = 0; q < nq; ++q) {
        std::set<int32_t> want;  // brute force: every filter triple against this pair
        for (int64_t k = 0; k < nf; ++k)
            if (c.fh[k] == c.qh[q] && c.ft[k] == c.qt[q]) want.insert(c.fr[k]);
        const int32_t g = kc.group[(size_t)q];
        if (g < 0 || (size_t)g + 1 >= kc.off.size()) {
            printf("%s: query %lld has list %d out of range\n", name, (long long)q, g);
            return 1;
        }
        const std::vector<int32_t> got(kc.ids.begin() + kc.off[(size_t)g], kc.ids.begin() + kc.off[(size_t)g + 1]);
        const std::vector<int32_t> exp(want.begin(), want.end());  // ascending, distinct
        if (got != exp) {
            printf("%s: query %lld (h %d, t %d): %zu relations, expected %zu\n", name, (long long)q, c.qh[q],
                   c.qt[q], got.size(), exp.size());
            return 1;
        }
        for (int64_t p = 0; p < q; ++p)  // queries on the same pair share one list, others do not
            if ((c.qh[p] == c.qh[q] && c.qt[p] == c.qt[q]) != (kc.group[(size_t)p] == g)) {
                printf("%s: queries %lld and %lld grouped wrongly\n", name, (long long)p, (long long)q);
                return 1;
            }
    }
    // the entity list: distinct, covers every pair, and the indices point back at the pair
    const kb2e::PairEntities pe = kb2e::build_pair_entities(c.qh.data(), c.qt.data(), nq);
    std::set<int32_t> distinct(pe.ents.begin(), pe.ents.end()), want;
    for (int64_t q = 0; q < nq; ++q) {
        want.insert(c.qh[q]);
        want.insert(c.qt[q]);
    }
    if (distinct.size() != pe.ents.size() || distinct != want || (int64_t)pe.hi.size() != nq ||
        (int64_t)pe.ti.size() != nq) {
        printf("%s: entity list is not the distinct entities of the pairs\n", name);
        return 1;
    }
    for (int64_t q = 0; q < nq; ++q) {
        const int32_t a = pe.hi[(size_t)q], b = pe.ti[(size_t)q];
        if (a < 0 || (size_t)a >= pe.ents.size() || b < 0 || (size_t)b >= pe.ents.size() ||
            pe.ents[(size_t)a] != c.qh[q] || pe.ents[(size_t)b] != c.qt[q]) {
            printf("%s: query %lld indexes the wrong entities\n", name, (long long)q);
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
        if (k % 4 == 3) {  // a repeated pair
            const size_t p = g() % c.qh.size();
            c.qh.push_back(c.qh[p]);
            c.qt.push_back(c.qt[p]);
        } else if (k % 4 == 1 && nf > 0) {  // a pair the filter knows
            const size_t p = g() % c.fh.size();
            c.qh.push_back(c.fh[p]);
            c.qt.push_back(c.ft[p]);
        } else {
            c.qh.push_back((int32_t)(g() % ne));
            c.qt.push_back((int32_t)(g() % ne));
        }
    }
    return c;
}

}  // namespace

int main() {
    int bad = 0;
    bad += check("empty filter", random_case(1, 50, 4, 40, 0, false));
    bad += check("dense", random_case(2, 6, 5, 200, 600, false));
    bad += check("duplicate filter triples", random_case(3, 8, 3, 100, 500, true));
    bad += check("one query", random_case(4, 3, 2, 1, 80, true));
    bad += check("sparse", random_case(5, 5000, 40, 300, 2000, false));
    {
        // the pair (1, 2) has every one of the 3 relations known (one listed twice);
        // (2, 2) and (0, 0) are h == t queries, one known and one not; (2, 1) is the
        // reversed pair and shares nothing with (1, 2)
        Case c{3, 3, {1, 2, 0, 2, 1}, {2, 2, 0, 1, 2}, {1, 1, 1, 1, 2, 2}, {2, 2, 2, 2, 2, 1}, {2, 0, 1, 0, 1, 0}};
        bad += check("every relation known, self loops", c);
        const kb2e::KnownCandidates kc = kb2e::build_known_relations(c.qh.data(), c.qt.data(), 5, c.fh.data(),
                                                                     c.ft.data(), c.fr.data(), 6, c.ne);
        const int32_t g = kc.group[0];
        if (kc.off[(size_t)g + 1] - kc.off[(size_t)g] != 3 || kc.group[4] != g) {
            printf("every relation known: the list of (1, 2) does not hold all 3 relations\n");
            ++bad;
        }
    }
    if (bad) return 1;
    printf("ok\n");
    return 0;
}
