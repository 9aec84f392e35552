// complete_check.cpp -- the host half of knowledge-base completion
// (kb2e_amd/csrc/complete_host.hpp: the strip plan of a relation's |H| x |T|
// candidates and the pair id) against brute force, on the CPU
// (tests/test_complete_host.py builds this with ASan + UBSan and runs it).
#include <cstdint>
#include <cstdio>
#include <set>
#include <vector>

#include "complete_host.hpp"

namespace {

// every (head, tail) position is covered once, in head-major strip order, and
// no strip holds more candidates than the buffer holds records
int check_plan(int64_t nh, int64_t nt, int64_t bytes, int64_t cap) {
    const kb2e::StripPlan p = kb2e::plan_strips(nh, nt, bytes, cap);
    auto bad = [&](const char* what) {
        printf("plan(%lld, %lld, %lld, %lld): %s\n", (long long)nh, (long long)nt, (long long)bytes, (long long)cap, what);
        return 1;
    };
    if (p.cap_records < kb2e::kCompleteMinRecords) return bad("buffer under the minimum");
    if (bytes / kb2e::kCompleteRecordBytes >= kb2e::kCompleteMinRecords &&
        p.cap_records != bytes / kb2e::kCompleteRecordBytes)
        return bad("capacity is not the buffer's");
    if (p.strip_heads < kb2e::kCompleteTile || p.strip_heads % kb2e::kCompleteTile) return bad("strip is no whole tiles");
    if (cap >= kb2e::kCompleteTile && p.strip_heads > cap) return bad("strip over the cap");
    if (p.strips.empty()) return bad("no strips");
    std::vector<uint8_t> seen((size_t)(nh * nt), 0);
    int64_t last_h0 = -1;
    for (size_t s = 0; s < p.strips.size(); ++s) {
        const kb2e::Strip& st = p.strips[s];
        if (st.nh < 1 || st.nt < 1 || st.h0 < 0 || st.t0 < 0 || st.h0 + st.nh > nh || st.t0 + st.nt > nt)
            return bad("strip out of range");
        if (st.nh * st.nt > p.cap_records) return bad("strip overflows the buffer");
        if ((st.nh + kb2e::kCompleteTile - 1) / kb2e::kCompleteTile > kb2e::kCompleteMaxTiles) return bad("too many tiles");
        if (st.h0 % kb2e::kCompleteTile) return bad("strip starts inside a tile");
        if (st.h0 == 0 && st.nh > kb2e::kCompleteTile) return bad("first strip is more than a tile");
        if (st.h0 < last_h0) return bad("heads go backwards");
        last_h0 = st.h0;
        for (int64_t h = st.h0; h < st.h0 + st.nh; ++h)
            for (int64_t t = st.t0; t < st.t0 + st.nt; ++t)
                if (seen[(size_t)(h * nt + t)]++) return bad("pair covered twice");
    }
    for (uint8_t v : seen)
        if (v != 1) return bad("pair not covered");
    return 0;
}

int check_pairs() {
    const int64_t nes[] = {1, 2, 3, 300, 14951, 2147483647};
    for (int64_t ne : nes) {
        std::set<int64_t> ids;  // ascending, distinct, in range
        for (int64_t x : {(int64_t)0, (int64_t)1, ne / 2, ne - 2, ne - 1})
            if (x >= 0 && x < ne) ids.insert(x);
        uint64_t prev = 0;
        bool first = true;
        for (int64_t h : ids)
            for (int64_t t : ids) {
                const uint64_t p = kb2e::pair_id(h, t, ne);
                if (kb2e::pair_head(p, ne) != h || kb2e::pair_tail(p, ne) != t) {
                    printf("pair (%lld, %lld) of %lld does not round-trip\n", (long long)h, (long long)t, (long long)ne);
                    return 1;
                }
                // (head, tail) order is the order of the pair ids
                if (!first && p <= prev) {
                    printf("pair ids of %lld do not ascend\n", (long long)ne);
                    return 1;
                }
                prev = p;
                first = false;
            }
    }
    return 0;
}

}  // namespace

int main() {
    int fails = check_pairs();
    const int64_t sizes[] = {1, 2, 15, 16, 17, 31, 32, 33, 100, 300};
    const int64_t buffers[] = {0, 1, 16384, 16400, 20000, 76800, 80000, 1 << 20, (int64_t)256 << 20};
    const int64_t caps[] = {0, 1, 16, 31, 32, 48, 1000};
    for (int64_t nh : sizes)
        for (int64_t nt : sizes)
            for (int64_t b : buffers)
                for (int64_t c : caps) fails += check_plan(nh, nt, b, c);
    // tails that do not fit a tile's worth of the smallest buffer: chunked
    fails += check_plan(40, 3000, 0, 0);
    fails += check_plan(17, 5000, 16384, 16);
    {  // the shapes of the header's numbers: FB15k with the default buffer
        const kb2e::StripPlan p = kb2e::plan_strips(14951, 14951, (int64_t)256 << 20, 0);
        if (p.cap_records != 16777216 || p.tail_chunk != 14951 || p.strip_heads != 1120 || p.strips.size() != 15) {
            printf("FB15k plan: %lld records, chunk %lld, strips of %lld, %zu strips\n", (long long)p.cap_records,
                   (long long)p.tail_chunk, (long long)p.strip_heads, p.strips.size());
            ++fails;
        }
    }
    if (fails) return 1;
    printf("ok\n");
    return 0;
}
