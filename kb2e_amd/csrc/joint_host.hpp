// joint_host.hpp -- host side of the conjunctive queries (kb2e_predict_joint,
// kb2e_rank_joint), free of HIP so that it can be checked on the CPU
// (tests/native/joint_check.cpp).
//
// Query q owns the constraint rows offsets[q] .. offsets[q + 1] - 1, each a
// one-sided pattern (entity, relation, side) as kb2e_predict takes it.  Three
// pieces live here: the check of `offsets`, the plan that cuts the queries into
// chunks whose rows fit the key buffer, and the per-query list of excluded
// candidates -- the entities known for every one of the query's patterns, the
// intersection of the sorted, distinct lists build_known_candidates yields.
#pragma once

#include <algorithm>
#include <cstdint>
#include <iterator>
#include <vector>

#include "predict_host.hpp"

namespace kb2e {

constexpr int kJointMaxConstraints = 64;  // KB2E_JOINT_MAX_CONSTRAINTS

// nullptr when offsets [nq + 1] is well-formed (nq >= 1), else what is wrong.
inline const char* joint_check_offsets(const int64_t* offsets, int64_t nq) {
    if (nq < 1) return "no queries";
    if (!offsets) return "no offsets";
    if (offsets[0] != 0) return "offsets must start at 0";
    for (int64_t q = 0; q < nq; ++q) {
        // (compared, not subtracted: a hostile pair of offsets must not overflow)
        if (offsets[q + 1] <= offsets[q]) return "offsets must increase: a query without constraints";
        if (offsets[q + 1] > (int64_t)INT32_MAX) return "more than 2^31 - 1 constraints in one call";
        if (offsets[q + 1] - offsets[q] > kJointMaxConstraints) return "a query with more than 64 constraints";
    }
    return nullptr;
}

inline int64_t joint_max_constraints(const int64_t* offsets, int64_t nq) {
    int64_t m = 0;
    for (int64_t q = 0; q < nq; ++q) m = std::max(m, offsets[q + 1] - offsets[q]);
    return m;
}

struct JointChunk {
    int64_t q0, q1;  // the queries [q0, q1); their rows are offsets[q0] .. offsets[q1] - 1
};

// The queries in the caller's order, cut into the longest runs whose rows fit
// max(cap_rows, the largest query): every query in exactly one chunk, never split.
inline std::vector<JointChunk> joint_plan_chunks(const int64_t* offsets, int64_t nq, int64_t cap_rows) {
    const int64_t budget = std::max(cap_rows, joint_max_constraints(offsets, nq));
    std::vector<JointChunk> chunks;
    for (int64_t q0 = 0; q0 < nq;) {
        int64_t q1 = q0 + 1;
        while (q1 < nq && offsets[q1 + 1] - offsets[q0] <= budget) ++q1;
        chunks.push_back(JointChunk{q0, q1});
        q0 = q1;
    }
    return chunks;
}

// Per query the candidates that are known for every one of its constraints
// (ascending, distinct): kc lists the known candidates per constraint row
// (kc.group has one entry per row).  off [nq + 1] indexes ids.
struct JointKnown {
    std::vector<int64_t> off;
    std::vector<int32_t> ids;
};

inline JointKnown joint_intersect_known(const int64_t* offsets, int64_t nq, const KnownCandidates& kc) {
    JointKnown jk;
    jk.off.assign((size_t)nq + 1, 0);
    std::vector<int32_t> cur, next;
    for (int64_t q = 0; q < nq; ++q) {
        const int32_t g0 = kc.group[(size_t)offsets[q]];
        cur.assign(kc.ids.begin() + kc.off[(size_t)g0], kc.ids.begin() + kc.off[(size_t)g0 + 1]);
        for (int64_t c = offsets[q] + 1; c < offsets[q + 1] && !cur.empty(); ++c) {
            const int32_t g = kc.group[(size_t)c];
            next.clear();
            std::set_intersection(cur.begin(), cur.end(), kc.ids.begin() + kc.off[(size_t)g],
                                  kc.ids.begin() + kc.off[(size_t)g + 1], std::back_inserter(next));
            cur.swap(next);
        }
        jk.ids.insert(jk.ids.end(), cur.begin(), cur.end());
        jk.off[(size_t)q + 1] = (int64_t)jk.ids.size();
    }
    return jk;
}

}  // namespace kb2e
