// foldin_host.hpp -- host side of entity fold-in (kb2e_fold_in_entities,
// foldin.hip), free of HIP so that it can be checked on the CPU
// (tests/native/foldin_check.cpp).
//
// * plan_fold: argument validation (throws std::invalid_argument), the stable
//   grouping of the examples by the free entity they mention (CSR: offsets by
//   free index + a permutation that keeps the caller's order inside a group),
//   the slot the free entity fills in each example, the units ordered by
//   descending work (so that the longest chains start first; ties by free
//   index, so the order is a function of the arguments alone) and the bitmap
//   of the free entities.
// * fold_known_set: the set a corrupted triple must not be in -- the caller's
//   known triples with the examples added (FilterSet of host_data.hpp, probed
//   on the device through FilterView's layout).
// * fold_sweep_cap: max_sweeps, 0 meaning kFoldDefaultSweeps.
#pragma once

#include <algorithm>
#include <cstdint>
#include <numeric>
#include <stdexcept>
#include <string>
#include <vector>

#include "host_data.hpp"

namespace kb2e {

constexpr int32_t kFoldDefaultSweeps = 10000;
constexpr int kFoldDraws = 32;  // candidate draws per sample (kb2e_corrupt_triples' stage 2 length)

inline int32_t fold_sweep_cap(int32_t max_sweeps) { return max_sweeps == 0 ? kFoldDefaultSweeps : max_sweeps; }

struct FoldPlan {
    std::vector<int64_t> off;        // [nfree + 1] by free index: its examples are perm[off[f] .. off[f + 1])
    std::vector<int32_t> perm;       // [count] example indices, grouped, the caller's order inside a group
    std::vector<uint8_t> slot;       // [count] by example index: 0 the free entity is the head, 1 the tail
    std::vector<int32_t> unit_free;  // [nfree] unit u works on free index unit_free[u]; descending work
    std::vector<uint64_t> bitmap;    // [(ne + 63) / 64] bit e: entity e is free
};

inline FoldPlan plan_fold(const int32_t* free_entities, int64_t nfree, const int32_t* heads, const int32_t* tails,
                          const int32_t* relations, int64_t count, const int32_t* kh, const int32_t* kt,
                          const int32_t* kr, int64_t nknown, int64_t ne, int64_t nr) {
    if (nfree < 1) throw std::invalid_argument("no free entities");
    if (count < 0 || nknown < 0) throw std::invalid_argument("negative count");
    if (!free_entities || (count > 0 && (!heads || !tails || !relations)) || (nknown > 0 && (!kh || !kt || !kr)))
        throw std::invalid_argument("a NULL array with a count > 0");
    if (count > INT32_MAX) throw std::invalid_argument("too many examples in one call");
    FoldPlan p;
    std::vector<int32_t> index((size_t)ne, -1);  // entity -> free index
    p.bitmap.assign((size_t)((ne + 63) / 64), 0);
    for (int64_t f = 0; f < nfree; ++f) {
        const int64_t e = free_entities[f];
        if (e < 0 || e >= ne) throw std::invalid_argument("free entity " + std::to_string(f) + " is out of range");
        if (index[(size_t)e] >= 0) throw std::invalid_argument("free entity " + std::to_string(e) + " is listed twice");
        index[(size_t)e] = (int32_t)f;
        p.bitmap[(size_t)(e >> 6)] |= 1ull << (e & 63);
    }
    for (int64_t k = 0; k < nknown; ++k)
        if (kh[k] < 0 || kh[k] >= ne || kt[k] < 0 || kt[k] >= ne || kr[k] < 0 || kr[k] >= nr)
            throw std::invalid_argument("known triple " + std::to_string(k) + " has an id out of range");
    p.off.assign((size_t)nfree + 1, 0);
    p.slot.assign((size_t)count, 0);
    std::vector<int32_t> owner((size_t)count);
    for (int64_t k = 0; k < count; ++k) {
        if (heads[k] < 0 || heads[k] >= ne || tails[k] < 0 || tails[k] >= ne || relations[k] < 0 || relations[k] >= nr)
            throw std::invalid_argument("example " + std::to_string(k) + " has an id out of range");
        const int32_t fh = index[(size_t)heads[k]], ft = index[(size_t)tails[k]];
        if (fh < 0 && ft < 0) throw std::invalid_argument("example " + std::to_string(k) + " mentions no free entity");
        if (fh >= 0 && ft >= 0)
            throw std::invalid_argument("example " + std::to_string(k) + " has a free entity in both slots");
        owner[(size_t)k] = fh >= 0 ? fh : ft;
        p.slot[(size_t)k] = fh >= 0 ? 0 : 1;
        ++p.off[(size_t)owner[(size_t)k] + 1];
    }
    for (int64_t f = 0; f < nfree; ++f) p.off[(size_t)f + 1] += p.off[(size_t)f];
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

// known + examples (ids already checked by plan_fold)
inline FilterSet fold_known_set(const int32_t* heads, const int32_t* tails, const int32_t* relations, int64_t count,
                                const int32_t* kh, const int32_t* kt, const int32_t* kr, int64_t nknown, int64_t ne,
                                int64_t nr) {
    std::vector<int32_t> H, T, R;
    H.reserve((size_t)(nknown + count));
    T.reserve((size_t)(nknown + count));
    R.reserve((size_t)(nknown + count));
    if (nknown > 0) {
        H.assign(kh, kh + nknown);
        T.assign(kt, kt + nknown);
        R.assign(kr, kr + nknown);
    }
    if (count > 0) {
        H.insert(H.end(), heads, heads + count);
        T.insert(T.end(), tails, tails + count);
        R.insert(R.end(), relations, relations + count);
    }
    FilterSet fs;
    fs.build(H, T, R, ne, nr);
    return fs;
}

}  // namespace kb2e
