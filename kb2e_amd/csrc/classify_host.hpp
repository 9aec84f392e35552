// classify_host.hpp -- host side of triple classification (kb2e_corrupt_triples
// and the classifyTrans* binaries), free of HIP so that it can be checked on
// the CPU (tests/native/classify_check.cpp).
//
// * build_slot_pools: per (relation, slot) the distinct entities seen in that
//   slot of that relation among the known triples -- the pool a constrained
//   negative is drawn from (Socher et al. 2013).  CSR layout, list
//   relation * 2 + slot (slot 0 = head, 1 = tail), ids ascending and distinct.
//   O(nknown) plus the sort of each list.
// * corrupt_mix / corrupt_u: the counter-based stream of kb2e_corrupt_triples
//   (include/kb2e_engine.h), shared with the device kernel.
// * load_labelled_file: the "head<TAB>tail<TAB>relation<TAB>label" files of
//   classifyTrans* (--validlabels / --testlabels).
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define KB2E_HD __host__ __device__
#else
#define KB2E_HD
#endif

namespace kb2e {

constexpr int kCorruptDraws = 32;  // draws per stage

// SplitMix64's finaliser
KB2E_HD inline uint64_t corrupt_mix(uint64_t z) {
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

// draw a of triple i: a = 0 the coin (top bit), 1..32 stage 1, 33..64 stage 2
KB2E_HD inline uint64_t corrupt_u(uint64_t state, uint64_t i, uint64_t a) { return corrupt_mix(state + (i << 7) + a); }

struct SlotPools {
    std::vector<int64_t> off;  // [2 * nr + 1]
    std::vector<int32_t> ids;  // the lists: ascending, distinct
};

// ids must be in range (the caller checks).  nknown == 0: every list is empty.
inline SlotPools build_slot_pools(const int32_t* kh, const int32_t* kt, const int32_t* kr, int64_t nknown, int64_t nr) {
    SlotPools sp;
    const size_t nl = (size_t)nr * 2;
    std::vector<int64_t> off(nl + 1, 0);
    for (int64_t k = 0; k < nknown; ++k) {
        ++off[(size_t)kr[k] * 2 + 1];
        ++off[(size_t)kr[k] * 2 + 2];
    }
    for (size_t l = 0; l < nl; ++l) off[l + 1] += off[l];
    std::vector<int32_t> all((size_t)off[nl]);
    std::vector<int64_t> fill(off.begin(), off.end() - 1);
    for (int64_t k = 0; k < nknown; ++k) {
        all[(size_t)fill[(size_t)kr[k] * 2]++] = kh[k];
        all[(size_t)fill[(size_t)kr[k] * 2 + 1]++] = kt[k];
    }
    // an entity that fills a slot in several triples: once
    sp.off.assign(nl + 1, 0);
    sp.ids.reserve(all.size());
    for (size_t l = 0; l < nl; ++l) {
        auto b = all.begin() + off[l], e = all.begin() + off[l + 1];
        std::sort(b, e);
        e = std::unique(b, e);
        sp.ids.insert(sp.ids.end(), b, e);
        sp.off[l + 1] = (int64_t)sp.ids.size();
    }
    return sp;
}

// One labelled triple per line: "head<TAB>tail<TAB>relation<TAB>label" with the
// names of the id files; label 1 is a positive, -1 or 0 a negative.  Lines that
// name an unknown entity or relation, or carry another label, are reported and
// skipped (as the triple loader does, common/loader.cpp:40-57).  Returns false
// if the file cannot be opened.  cb(head, tail, relation, label 0 / 1).
template <typename F>
bool load_labelled_file(const std::string& path, const std::map<std::string, int>& ent,
                        const std::map<std::string, int>& rel, F&& cb) {
    FILE* f = fopen(path.c_str(), "r");
    if (!f) return false;
    char hb[512], tb[512], rb[512], lb[512];
    while (fscanf(f, "%511s\t%511s\t%511s\t%511s", hb, tb, rb, lb) == 4) {
        auto h = ent.find(hb), t = ent.find(tb);
        auto r = rel.find(rb);
        int label = -1;
        if (!strcmp(lb, "1")) label = 1;
        else if (!strcmp(lb, "-1") || !strcmp(lb, "0")) label = 0;
        if (h == ent.end() || t == ent.end() || r == rel.end() || label < 0) {
            printf("Labelled triple skipped (unknown name or label): %s %s %s %s\n", hb, tb, rb, lb);
            continue;
        }
        cb(h->second, t->second, r->second, label);
    }
    fclose(f);
    return true;
}

}  // namespace kb2e
