// complete_host.hpp -- host side of knowledge-base completion
// (kb2e_complete_triples, complete.hip), free of HIP so that it can be checked
// on the CPU (tests/native/complete_check.cpp).
//
// * pair_id / pair_head / pair_tail: a candidate (h, t) as one 64-bit number
//   whose order is (head id, tail id) order.
// * plan_strips: how the |H| x |T| candidates of one relation are walked so
//   that the records of one step always fit the record buffer.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace kb2e {

constexpr int kCompleteTile = 16;                        // heads per tile (kQ)
constexpr int64_t kCompleteRecordBytes = 16;             // (energy bits, pair id)
constexpr int64_t kCompleteMinRecords = 1024;            // the smallest buffer: 16 KiB
constexpr int64_t kCompleteMaxTiles = (int64_t)1 << 20;  // head tiles of one launch

inline uint64_t pair_id(int64_t h, int64_t t, int64_t ne) { return (uint64_t)h * (uint64_t)ne + (uint64_t)t; }
inline int32_t pair_head(uint64_t p, int64_t ne) { return (int32_t)(p / (uint64_t)ne); }
inline int32_t pair_tail(uint64_t p, int64_t ne) { return (int32_t)(p % (uint64_t)ne); }

// One step: the heads [h0, h0 + nh) and tails [t0, t0 + nt) of the candidate lists.
struct Strip {
    int64_t h0, nh, t0, nt;
};

struct StripPlan {
    int64_t cap_records = 0;  // records the buffer holds
    int64_t tail_chunk = 0;   // tails per step (all of them unless a tile of them overflows the buffer)
    int64_t strip_heads = 0;  // heads of the strips after the first
    std::vector<Strip> strips;
};

// nh, nt >= 1.  buffer_bytes: the record buffer (raised to kCompleteMinRecords
// records).  strip_cap > 0 caps the heads of the later strips.  The first head
// strip is one tile: it sets a bound at the price of 16 x |T| records.  Every
// strip's heads are a multiple of the tile except the last one's, and
// nh * nt <= cap_records holds for every strip: the buffer cannot overflow.
inline StripPlan plan_strips(int64_t nh, int64_t nt, int64_t buffer_bytes, int64_t strip_cap) {
    StripPlan p;
    p.cap_records = std::max(kCompleteMinRecords, buffer_bytes / kCompleteRecordBytes);
    p.tail_chunk = std::min(nt, p.cap_records / kCompleteTile);
    int64_t hs = p.cap_records / p.tail_chunk / kCompleteTile * kCompleteTile;
    hs = std::min(hs, kCompleteMaxTiles * kCompleteTile);
    if (strip_cap > 0) hs = std::min(hs, std::max<int64_t>(kCompleteTile, strip_cap / kCompleteTile * kCompleteTile));
    p.strip_heads = hs;
    for (int64_t h0 = 0; h0 < nh;) {
        const int64_t m = std::min(nh - h0, h0 == 0 ? (int64_t)kCompleteTile : hs);
        for (int64_t t0 = 0; t0 < nt; t0 += p.tail_chunk)
            p.strips.push_back(Strip{h0, m, t0, std::min(p.tail_chunk, nt - t0)});
        h0 += m;
    }
    return p;
}

}  // namespace kb2e
