// neighbors_check.cpp -- the host half of entity neighbours
// (kb2e_amd/csrc/neighbors_host.hpp) against brute force: plan_slices (every
// candidate in exactly one slice, chunk rows x slices x k under the cap, whole
// tiles, every query in exactly one chunk) and mutual_pairs (an O(n^2) loop).
// Built with ASan + UBSan and run directly by tests/test_neighbors_host.py.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <tuple>
#include <vector>

#include "neighbors_host.hpp"

using namespace kb2e;

#define REQUIRE(cond)                                                        \
    do {                                                                     \
        if (!(cond)) {                                                       \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);         \
            exit(1);                                                         \
        }                                                                    \
    } while (0)

static void check_plan(int64_t ne, int64_t nq, int64_t k, int64_t slice, int64_t rows, int64_t cap_bytes) {
    const SlicePlan p = plan_slices(ne, nq, k, slice, rows, cap_bytes);
    REQUIRE(p.slice_len >= 1 && p.slices >= 1 && p.chunk_rows >= kNeighborsTile && p.chunks >= 1);
    REQUIRE(p.chunk_rows % kNeighborsTile == 0);
    REQUIRE(p.cap_records >= cap_bytes / kNeighborsRecordBytes);
    // the cap: what is asked for, or one tile's single slice where that is more
    REQUIRE(p.cap_records * kNeighborsRecordBytes <= std::max(cap_bytes, kNeighborsTile * k * kNeighborsRecordBytes));
    REQUIRE(p.chunk_rows * p.slices * k <= p.cap_records);
    // every candidate in exactly one slice (the kernel's own bounds)
    if (ne <= 5000) {
        std::vector<int> seen((size_t)ne, 0);
        for (int64_t s = 0; s < p.slices; ++s) {
            const int64_t s0 = s * p.slice_len, s1 = std::min(ne, s0 + p.slice_len);
            REQUIRE(s0 < s1);  // no empty slice
            for (int64_t x = s0; x < s1; ++x) ++seen[(size_t)x];
        }
        for (int64_t x = 0; x < ne; ++x) REQUIRE(seen[(size_t)x] == 1);
    } else {
        REQUIRE((p.slices - 1) * p.slice_len < ne && p.slices * p.slice_len >= ne);
    }
    // every query in exactly one chunk
    REQUIRE((p.chunks - 1) * p.chunk_rows < nq && p.chunks * p.chunk_rows >= nq);
    // the knobs
    if (slice > 0 && (ne + std::min(slice, ne) - 1) / std::min(slice, ne) * kNeighborsTile * k <= p.cap_records)
        REQUIRE(p.slice_len == std::min(slice, ne));
    if (rows > 0) REQUIRE(p.chunk_rows <= std::max<int64_t>(kNeighborsTile, rows));
    if (slice == 0) REQUIRE(p.slices <= kNeighborsMaxDefaultSlices);
    if (slice == 0 && cap_bytes == kNeighborsPartialBytes) {  // (a small cap may lengthen the slices)
        REQUIRE(p.slices == 1 || (p.slice_len >= kNeighborsMinDefaultSlice && p.slice_len % 256 == 0));
    }
}

static void check_pairs(std::mt19937& rng, int ne, int nq, int k, bool graph) {
    std::vector<int32_t> ents((size_t)nq), ids((size_t)nq * k), found((size_t)nq);
    std::vector<double> dist((size_t)nq * k);
    for (int q = 0; q < nq; ++q) {
        ents[(size_t)q] = graph ? q : (int32_t)(rng() % ne);
        // a random list of distinct entities, a few distances shared
        std::vector<int32_t> perm((size_t)ne);
        for (int x = 0; x < ne; ++x) perm[(size_t)x] = x;
        std::shuffle(perm.begin(), perm.end(), rng);
        found[(size_t)q] = (int32_t)(rng() % (std::min(k, ne) + 1));
        for (int j = 0; j < k; ++j) {
            const bool live = j < found[(size_t)q];
            ids[(size_t)q * k + j] = live ? perm[(size_t)j] : -1;
            dist[(size_t)q * k + j] = live ? (double)(rng() % 4) * 0.25 : std::numeric_limits<double>::infinity();
        }
    }
    const std::vector<MutualPair> got = mutual_pairs(ents.data(), nq, k, ids.data(), dist.data(), found.data());
    // brute force over the first listing of every entity
    std::vector<int> row((size_t)ne, -1);
    for (int q = nq - 1; q >= 0; --q) row[(size_t)ents[(size_t)q]] = q;
    auto lists = [&](int a, int b, double* d) {
        const int q = row[(size_t)a];
        if (q < 0) return false;
        for (int j = 0; j < found[(size_t)q]; ++j)
            if (ids[(size_t)q * k + j] == b) {
                if (d) *d = dist[(size_t)q * k + j];
                return true;
            }
        return false;
    };
    std::vector<std::tuple<double, int, int>> want;
    for (int a = 0; a < ne; ++a)
        for (int b = a + 1; b < ne; ++b) {
            double d = 0;
            if (lists(a, b, &d) && lists(b, a, nullptr)) want.emplace_back(d, a, b);
        }
    std::sort(want.begin(), want.end());
    REQUIRE(got.size() == want.size());
    for (size_t i = 0; i < got.size(); ++i)
        REQUIRE(std::make_tuple(got[i].dist, (int)got[i].a, (int)got[i].b) == want[i]);
}

int main() {
    const int64_t big = kNeighborsPartialBytes;
    for (int64_t ne : {1, 2, 15, 16, 17, 255, 256, 257, 300, 1023, 1024, 1025, 4999, 14951, 40943, 1000000})
        for (int64_t nq : {1, 15, 16, 17, 300, 14951, 1000000})
            for (int64_t k : {1, 10, 127, 128})
                for (int64_t slice : {0, 1, 64, 300, 100000})
                    for (int64_t rows : {0, 1, 16, 40, 4096})
                        for (int64_t cap : {big, (int64_t)1 << 20, (int64_t)4096, (int64_t)12}) check_plan(ne, nq, k, slice, rows, cap);
    // the default plan of the FB15k graph: 935 tiles, 3 slices of 5,120, one chunk
    {
        const SlicePlan p = plan_slices(14951, 14951, 10, 0, 0);
        REQUIRE(p.slice_len == 5120 && p.slices == 3 && p.chunks == 1 && p.chunk_rows == 14960);
    }
    // a forced slice of 1 at a large |E|: raised until one tile's records fit
    {
        const SlicePlan p = plan_slices(1000000, 16, 128, 1, 0);
        REQUIRE(p.slice_len > 1 && kNeighborsTile * p.slices * 128 <= p.cap_records && p.chunk_rows == 16);
    }
    std::mt19937 rng(20240607u);
    for (int round = 0; round < 40; ++round) {
        check_pairs(rng, 1 + (int)(rng() % 40), 1 + (int)(rng() % 60), 1 + (int)(rng() % 8), false);
        const int ne = 1 + (int)(rng() % 40);
        check_pairs(rng, ne, ne, 1 + (int)(rng() % 8), true);
    }
    printf("ok\n");
    return 0;
}
