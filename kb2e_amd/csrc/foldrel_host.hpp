// foldrel_host.hpp -- host side of relation fold-in (kb2e_fold_in_relations,
// foldrel.hip), free of HIP so that it can be checked on the CPU
// (tests/native/foldrel_check.cpp).
//
// * plan_fold_rel: argument validation (throws std::invalid_argument), the
//   stable grouping of the examples by their relation (CSR: offsets by free
//   index + a permutation that keeps the caller's order inside a group), the
//   units ordered by descending number of examples (ties by free index, so the
//   order is a function of the arguments alone) and the longest group.
// * The known set is foldin_host.hpp's fold_known_set (known + examples), the
//   sweep cap its fold_sweep_cap.
// * fold_rel_batch_cap: the number of records a workgroup stages at once,
//   min(batch_size, longest group), at least 1.
#pragma once

#include <algorithm>
#include <cstdint>
#include <numeric>
#include <stdexcept>
#include <string>
#include <vector>

#include "foldin_host.hpp"

namespace kb2e {

struct FoldRelPlan {
    std::vector<int64_t> off;        // [nfree + 1] by free index: its examples are perm[off[f] .. off[f + 1])
    std::vector<int32_t> perm;       // [count] example indices, grouped, the caller's order inside a group
    std::vector<int32_t> unit_free;  // [nfree] unit u works on free index unit_free[u]; descending work
    int64_t longest = 0;             // examples of the longest group
};

inline FoldRelPlan plan_fold_rel(const int32_t* free_relations, int64_t nfree, const int32_t* heads,
                                 const int32_t* tails, const int32_t* relations, int64_t count, const int32_t* kh,
                                 const int32_t* kt, const int32_t* kr, int64_t nknown, int64_t ne, int64_t nr) {
    if (nfree < 1) throw std::invalid_argument("no free relations");
    if (count < 0 || nknown < 0) throw std::invalid_argument("negative count");
    if (!free_relations || (count > 0 && (!heads || !tails || !relations)) || (nknown > 0 && (!kh || !kt || !kr)))
        throw std::invalid_argument("a NULL array with a count > 0");
    if (count > INT32_MAX) throw std::invalid_argument("too many examples in one call");
    FoldRelPlan p;
    std::vector<int32_t> index((size_t)nr, -1);  // relation -> free index
    for (int64_t f = 0; f < nfree; ++f) {
        const int64_t r = free_relations[f];
        if (r < 0 || r >= nr) throw std::invalid_argument("free relation " + std::to_string(f) + " is out of range");
        if (index[(size_t)r] >= 0) throw std::invalid_argument("free relation " + std::to_string(r) + " is listed twice");
        index[(size_t)r] = (int32_t)f;
    }
    for (int64_t k = 0; k < nknown; ++k)
        if (kh[k] < 0 || kh[k] >= ne || kt[k] < 0 || kt[k] >= ne || kr[k] < 0 || kr[k] >= nr)
            throw std::invalid_argument("known triple " + std::to_string(k) + " has an id out of range");
    p.off.assign((size_t)nfree + 1, 0);
    std::vector<int32_t> owner((size_t)count);
    for (int64_t k = 0; k < count; ++k) {
        if (heads[k] < 0 || heads[k] >= ne || tails[k] < 0 || tails[k] >= ne || relations[k] < 0 || relations[k] >= nr)
            throw std::invalid_argument("example " + std::to_string(k) + " has an id out of range");
        const int32_t f = index[(size_t)relations[k]];
        if (f < 0) throw std::invalid_argument("the relation of example " + std::to_string(k) + " is not free");
        owner[(size_t)k] = f;
        ++p.off[(size_t)f + 1];
    }
    for (int64_t f = 0; f < nfree; ++f) {
        p.longest = std::max(p.longest, p.off[(size_t)f + 1]);
        p.off[(size_t)f + 1] += p.off[(size_t)f];
    }
    p.perm.assign((size_t)count, 0);
    std::vector<int64_t> fill(p.off.begin(), p.off.end() - 1);
    for (int64_t k = 0; k < count; ++k) p.perm[(size_t)fill[(size_t)owner[(size_t)k]]++] = (int32_t)k;
    p.unit_free.resize((size_t)nfree);
    std::iota(p.unit_free.begin(), p.unit_free.end(), 0);
    std::stable_sort(p.unit_free.begin(), p.unit_free.end(), [&](int32_t a, int32_t b) {
        return p.off[(size_t)a + 1] - p.off[(size_t)a] > p.off[(size_t)b + 1] - p.off[(size_t)b];
    });
    return p;
}

inline int64_t fold_rel_batch_cap(int64_t batch_size, int64_t longest) {
    return std::max<int64_t>(1, std::min(batch_size, longest));
}

}  // namespace kb2e
