// classify_check.cpp -- the host half of triple classification
// (kb2e_amd/csrc/classify_host.hpp: the per-(relation, slot) candidate lists of
// kb2e_corrupt_triples and the labelled-file parser of classifyTrans*) against
// brute-force loops, on the CPU (tests/test_classify_host.py builds this with
// ASan + UBSan and runs it).  argv[1]: a directory to write the parser's files in.
#include <cstdint>
#include <cstdio>
#include <map>
#include <random>
#include <set>
#include <string>
#include <tuple>
#include <vector>

#include "classify_host.hpp"

namespace {

struct Case {
    int ne, nr;
    std::vector<int32_t> kh, kt, kr;
};

int check(const char* name, const Case& c) {
    const int64_t nk = (int64_t)c.kh.size();
    const kb2e::SlotPools sp = kb2e::build_slot_pools(nk ? c.kh.data() : nullptr, nk ? c.kt.data() : nullptr,
                                                      nk ? c.kr.data() : nullptr, nk, c.nr);
    if (sp.off.size() != (size_t)c.nr * 2 + 1 || sp.off[0] != 0 || sp.off.back() != (int64_t)sp.ids.size()) {
        printf("%s: malformed lists\n", name);
        return 1;
    }
    for (int r = 0; r < c.nr; ++r)
        for (int slot = 0; slot < 2; ++slot) {
            std::set<int32_t> want;  // brute force: every known triple against this (relation, slot)
            for (int64_t k = 0; k < nk; ++k)
                if (c.kr[k] == r) want.insert(slot ? c.kt[k] : c.kh[k]);
            const size_t l = (size_t)r * 2 + slot;
            if (sp.off[l] > sp.off[l + 1]) {
                printf("%s: list %zu has a negative length\n", name, l);
                return 1;
            }
            const std::vector<int32_t> got(sp.ids.begin() + sp.off[l], sp.ids.begin() + sp.off[l + 1]);
            const std::vector<int32_t> exp(want.begin(), want.end());  // ascending, distinct
            if (got != exp) {
                printf("%s: relation %d slot %d: %zu entities, expected %zu\n", name, r, slot, got.size(), exp.size());
                return 1;
            }
        }
    return 0;
}

int check_stream() {
    // SplitMix64 from state 0: the first output is mix(0 + golden gamma); the
    // finaliser alone on the published first state must give the published value
    if (kb2e::corrupt_mix(0x9E3779B97F4A7C15ull) != 0xE220A8397B1DCDAFull) {
        printf("corrupt_mix is not SplitMix64's finaliser\n");
        return 1;
    }
    const uint64_t st = kb2e::corrupt_mix(7);
    if (kb2e::corrupt_u(st, 3, 5) != kb2e::corrupt_mix(st + (3ull << 7) + 5)) {
        printf("corrupt_u is not mix(state + (i << 7) + a)\n");
        return 1;
    }
    return 0;
}

int check_parser(const std::string& dir) {
    const std::map<std::string, int> ent{{"a", 0}, {"b", 1}, {"c", 2}}, rel{{"r", 0}, {"s", 1}};
    const std::string path = dir + "/labelled.txt";
    FILE* f = fopen(path.c_str(), "w");
    if (!f) {
        printf("cannot write %s\n", path.c_str());
        return 1;
    }
    // line 3 names an unknown entity, line 5 carries label 2, line 7 is short,
    // line 8 has an over-long token: all skipped without touching memory
    fputs("a\tb\tr\t1\nb\tc\ts\t-1\nzz\ta\tr\t1\nc\ta\tr\t0\na\tc\ts\t2\nb\ta\ts\t1\n", f);
    fputs("a\tb\n", f);
    fputs((std::string(2000, 'q') + "\ta\tr\t1\n").c_str(), f);
    fclose(f);
    std::vector<std::tuple<int, int, int, int>> got;
    if (!kb2e::load_labelled_file(path, ent, rel, [&](int h, int t, int r, int l) { got.emplace_back(h, t, r, l); })) {
        printf("labelled file not opened\n");
        return 1;
    }
    const std::vector<std::tuple<int, int, int, int>> want{{0, 1, 0, 1}, {1, 2, 1, 0}, {2, 0, 0, 0}, {1, 0, 1, 1}};
    if (got.size() < want.size() || !std::equal(want.begin(), want.end(), got.begin())) {
        printf("labelled file: %zu triples parsed, the first %zu differ from the expected ones\n", got.size(),
               want.size());
        return 1;
    }
    for (size_t k = want.size(); k < got.size(); ++k) {  // whatever the ragged tail yields stays in range
        const auto [h, t, r, l] = got[k];
        if (h < 0 || h > 2 || t < 0 || t > 2 || r < 0 || r > 1 || l < 0 || l > 1) {
            printf("labelled file: triple %zu out of range\n", k);
            return 1;
        }
    }
    if (kb2e::load_labelled_file(dir + "/absent.txt", ent, rel, [](int, int, int, int) {})) {
        printf("an absent labelled file was reported as read\n");
        return 1;
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    int bad = 0;
    bad += check("empty known", Case{5, 3, {}, {}, {}});
    bad += check("duplicates", Case{4, 2, {0, 0, 0, 1, 1}, {1, 1, 1, 2, 2}, {0, 0, 0, 1, 1}});
    bad += check("relation absent", Case{6, 4, {0, 1, 2, 5}, {1, 2, 3, 0}, {0, 0, 3, 3}});
    bad += check("single entity in a slot", Case{5, 2, {2, 2, 2, 2}, {0, 1, 3, 4}, {1, 1, 1, 1}});
    std::mt19937 rng(11);
    for (int rep = 0; rep < 20; ++rep) {
        Case c;
        c.ne = 2 + (int)(rng() % 40);
        c.nr = 1 + (int)(rng() % 300);
        const int nk = (int)(rng() % 600);
        for (int k = 0; k < nk; ++k) {
            c.kh.push_back((int32_t)(rng() % (unsigned)c.ne));
            c.kt.push_back((int32_t)(rng() % (unsigned)c.ne));
            c.kr.push_back((int32_t)(rng() % (unsigned)c.nr));
        }
        bad += check("random", c);
    }
    bad += check_stream();
    if (argc > 1) bad += check_parser(argv[1]);
    else {
        printf("usage: classify_check DIR\n");
        return 2;
    }
    if (bad) return 1;
    printf("ok\n");
    return 0;
}
