// neighbors_host.hpp -- host side of entity neighbours (kb2e_neighbors,
// neighbors.hip), free of HIP so that it can be checked on the CPU
// (tests/native/neighbors_check.cpp).
//
// * plan_slices: how the |E| candidates are cut into slices and the nq queries
//   into chunks so that the partial records of a chunk (rows x slices x k)
//   always fit the fixed cap.
// * mutual_pairs: the pairs (a, b), a < b, that list each other -- the
//   duplicate candidates of a kNN graph (the CLI's --pairs; linkpred.py has
//   the same routine in numpy).
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <tuple>
#include <unordered_map>
#include <vector>

namespace kb2e {

constexpr int kNeighborsTile = 16;                            // query rows per tile (kQ)
constexpr int kNeighborsMaxK = 128;                           // the fused kernel's LDS budget: 16 rows x 256 records x 12 B
constexpr int64_t kNeighborsRecordBytes = 12;                 // (distance bits, entity id)
constexpr int64_t kNeighborsPartialBytes = (int64_t)64 << 20; // the cap on a chunk's partial records
constexpr int64_t kNeighborsTargetBlocks = 2048;              // tiles x slices the default plan aims at
constexpr int64_t kNeighborsMaxDefaultSlices = 16;            // ... with at most this many slices
constexpr int64_t kNeighborsMinDefaultSlice = 1024;           // ... of at least this many candidates
constexpr int64_t kNeighborsMaxChunkRows = (int64_t)1 << 20;  // rows of one launch

struct SlicePlan {
    int64_t cap_records = 0;  // partial records a chunk may hold
    int64_t slice_len = 0;    // candidates per slice (the last one may be shorter)
    int64_t slices = 0;       // slice s holds the candidates [s * slice_len, min(ne, (s + 1) * slice_len))
    int64_t chunk_rows = 0;   // query rows per chunk, a multiple of the tile
    int64_t chunks = 0;
};

// ne, nq >= 1, 1 <= k <= kNeighborsMaxK.  forced_slice > 0 sets the slice
// length (it is raised where 16 rows x slices x k records would not fit the
// cap); forced_rows > 0 caps the chunk (rounded down to whole tiles, at least
// one).  Otherwise: as many slices as bring tiles x slices to
// kNeighborsTargetBlocks, at most kNeighborsMaxDefaultSlices of them and none
// shorter than kNeighborsMinDefaultSlice, a multiple of 256 candidates each so
// that a slice is whole steps of the kernel; the merge then reads at most
// 16 x k records a query.  chunk_rows * slices * k <= cap_records always.
inline SlicePlan plan_slices(int64_t ne, int64_t nq, int64_t k, int64_t forced_slice, int64_t forced_rows,
                             int64_t cap_bytes = kNeighborsPartialBytes) {
    SlicePlan p;
    p.cap_records = std::max<int64_t>(cap_bytes / kNeighborsRecordBytes, kNeighborsTile * k);
    const int64_t tiles = (nq + kNeighborsTile - 1) / kNeighborsTile;
    int64_t len;
    if (forced_slice > 0) {
        len = forced_slice;
    } else {
        int64_t want = (kNeighborsTargetBlocks + tiles - 1) / tiles;
        want = std::min(want, kNeighborsMaxDefaultSlices);
        len = (ne + want - 1) / want;
        len = std::max(len, kNeighborsMinDefaultSlice);
        len = (len + 255) / 256 * 256;
    }
    len = std::min(len, ne);
    const int64_t max_slices = p.cap_records / (kNeighborsTile * k);  // >= 1
    if ((ne + len - 1) / len > max_slices) len = (ne + max_slices - 1) / max_slices;
    p.slice_len = len;
    p.slices = (ne + len - 1) / len;
    int64_t rows = p.cap_records / (p.slices * k) / kNeighborsTile * kNeighborsTile;  // >= one tile
    rows = std::min(rows, kNeighborsMaxChunkRows);
    if (forced_rows > 0) rows = std::min(rows, std::max<int64_t>(kNeighborsTile, forced_rows / kNeighborsTile * kNeighborsTile));
    rows = std::min(rows, tiles * kNeighborsTile);
    p.chunk_rows = rows;
    p.chunks = (nq + rows - 1) / rows;
    return p;
}

struct MutualPair {
    int32_t a, b;  // a < b
    double dist;   // of b in a's list
};

// ids / dist [nq][k], found [nq], entities [nq] (the query of each row; a
// query listed twice counts once, its first listing).  A pair (a, b), a < b, is
// mutual when b is among a's found neighbours and a among b's.  Ascending
// (distance bits as listed in a's row, a, b).
inline std::vector<MutualPair> mutual_pairs(const int32_t* entities, int64_t nq, int32_t k, const int32_t* ids,
                                            const double* dist, const int32_t* found) {
    std::unordered_map<int32_t, int64_t> row;
    for (int64_t q = 0; q < nq; ++q) row.emplace(entities[q], q);
    auto lists = [&](int64_t q, int32_t x) {
        for (int32_t j = 0; j < found[q]; ++j)
            if (ids[q * k + j] == x) return true;
        return false;
    };
    std::vector<MutualPair> out;
    for (const auto& [a, q] : row)
        for (int32_t j = 0; j < found[q]; ++j) {
            const int32_t b = ids[q * k + j];
            if (b <= a) continue;
            const auto it = row.find(b);
            if (it != row.end() && lists(it->second, a)) out.push_back(MutualPair{a, b, dist[q * k + j]});
        }
    std::sort(out.begin(), out.end(), [](const MutualPair& x, const MutualPair& y) {
        return std::tie(x.dist, x.a, x.b) < std::tie(y.dist, y.a, y.b);
    });
    return out;
}

}  // namespace kb2e
