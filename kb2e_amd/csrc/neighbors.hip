// neighbors.hip -- entity neighbours on the device.  Part of libkb2e.so
// (kb2e_neighbors in engine.hip calls in here).
//
// A query is an entity a; its candidates are all entities x (but a itself,
// unless asked for) and the answer is the k of smallest distance
// d(a, x) = sum_k |P(x)_k - P(a)_k| (or the squares) in the chosen space.
// Nothing of size nq x |E| is ever held: a candidate is written down only
// while it can still be among the k best of its row.
//
// * eval_project_kernel projects every entity once (the entity space is the
//   TransE projection: the row itself).
// * neighbors_score_select_kernel, one workgroup per (tile of kQ query rows,
//   candidate slice): complete_score_kernel's loop -- the tile's rows in LDS,
//   256 threads along the candidates, one serial FP64 sum per (thread, row) in
//   the evaluator's operand order -- but every tile row keeps its own best k of
//   the slice in LDS: a sorted list of <= k records and a staging list behind
//   it.  A candidate whose key is at most the row's bound (the k-th key of the
//   list, all-ones until k are held; ties pass, the id decides them later) is
//   ballot-compacted into the staging list, one LDS atomic per wave and row.
//   When a staging list overflows, the lists of the tile are bitonic-sorted on
//   (key, id), cut to k and the bounds lowered; the candidates that found no
//   room are offered again against the new bound.  The slice's k best of every
//   row go to partial[row][slice][k].
// * neighbors_merge_kernel, one workgroup per query: the slices' records, all
//   distinct (key, id) values, are sorted in LDS (in rounds when they are more
//   than the sort buffer holds), and the first k are written out, padded.
//
// What is kept and what is dropped depends on the order of arrival; the set of
// the k smallest (key, id) does not.  Everything of a call is queued on the
// tables' stream; there is one synchronisation, at the end.  No workgroup waits
// on another.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <stdexcept>
#include <string>

#include "eval_shared.hpp"
#include "hip_util.hpp"
#include "neighbors.hpp"
#include "neighbors_host.hpp"

namespace kb2e {
namespace {

static_assert(kNeighborsTile == kQ, "a chunk is a whole number of score tiles");

constexpr int kNbThreads = 256;
constexpr int kNbMinStage = 64;       // a staging list holds at least this many records
constexpr uint32_t kNoId = ~0u;       // the id of an empty slot: sorts behind every record
constexpr int kMergeCap = 2048;       // the merge's sort buffer, in records

static_assert(kNeighborsMaxK + kNbMinStage <= 256, "a row's lists are at most 256 records");

__device__ __forceinline__ bool rec_gt(uint64_t ka, uint32_t ia, uint64_t kb, uint32_t ib) {
    return ka > kb || (ka == kb && ia > ib);
}

// Bitonic sort on (key, id) of `lists` arrays of P records each (P a power of
// two), lying P apart; list l is skipped where todo[l] == 0 (null: none is).
// All threads of the workgroup call it; ends on a barrier.
__device__ __forceinline__ void bitonic_lists(uint64_t* key, uint32_t* id, int lists, int P, const uint32_t* todo) {
    const int half = P >> 1;
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int x = threadIdx.x; x < lists * half; x += (int)blockDim.x) {
                const int l = x / half, t = x & (half - 1);
                if (todo && todo[l] == 0) continue;
                const int lo = l * P + 2 * t - (t & (stride - 1));
                const int hi = lo + stride;
                const uint64_t ka = key[lo], kb = key[hi];
                const uint32_t ia = id[lo], ib = id[hi];
                const bool asc = ((2 * t - (t & (stride - 1))) & size) == 0;
                if (rec_gt(ka, ia, kb, ib) == asc) {
                    key[lo] = kb;
                    key[hi] = ka;
                    id[lo] = ib;
                    id[hi] = ia;
                }
            }
            __syncthreads();
        }
    }
}

// ------------------------------------------------------------ score + select

struct NeighborsScoreArgs {
    const double* PT;    // [n][ne]
    int32_t n, ne, l1;
    const int32_t* ent;  // the chunk's query entities [rows]
    int32_t rows;
    int32_t slices, slice_len;
    int32_t k, P;        // P: records of a row's two lists, a power of two >= k + kNbMinStage
    int32_t include_self;
    uint64_t* pkey;      // [rows][slices][k]
    uint32_t* pid;
    unsigned long long* prunes;
};

// Flat grid: block b takes the slice b % slices of the tile b / slices.
// Dynamic LDS: the lists' keys [kQ][P], (kRowsInLds) the tile's rows [n][kQ],
// the lists' ids [kQ][P].  Row q's sorted list is [0, cnt[q]), its staging
// list [k, k + nst[q]) of the P records.
template <bool kRowsInLds>
__global__ __launch_bounds__(kNbThreads) void neighbors_score_select_kernel(NeighborsScoreArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    __shared__ uint64_t tau[kQ];
    __shared__ uint32_t cnt[kQ], nst[kQ];
    __shared__ int qid[kQ];  // the tile's query entities (rows behind the last repeat it)
    uint64_t* lkey = (uint64_t*)lds_raw;
    double* kr = (double*)(lkey + kQ * a.P);
    uint32_t* lid = (uint32_t*)(kr + (kRowsInLds ? kQ * a.n : 0));
    const int tid = threadIdx.x, lane = tid & 63;
    const int tile = blockIdx.x / a.slices, slice = blockIdx.x % a.slices;
    const int q0 = tile * kQ;
    const int nq = min(kQ, a.rows - q0);
    const int k = a.k, P = a.P;
    const uint32_t cap = (uint32_t)(P - k);  // of a staging list
    if constexpr (kRowsInLds) {
        for (int x = tid; x < kQ * a.n; x += kNbThreads) {
            const int c = x / kQ, q = x % kQ;  // [n][kQ]: a step reads its kQ values side by side
            kr[x] = a.PT[(int64_t)c * a.ne + a.ent[q0 + min(q, nq - 1)]];
        }
    }
    if (tid < kQ) {
        qid[tid] = a.ent[q0 + min(tid, nq - 1)];
        tau[tid] = ~0ull;
        cnt[tid] = 0;
        nst[tid] = 0;
    }
    __syncthreads();

    int cuts = 0;  // (threads 0..kQ-1: the cuts of their row)
    // sort every row that has staged records, cut it to k, lower its bound
    auto prune = [&]() {
        for (int x = tid; x < kQ * P; x += kNbThreads) {
            const int q = x / P, j = x & (P - 1);
            const uint32_t ns = min(nst[q], cap);
            if (ns > 0 && ((j >= (int)cnt[q] && j < k) || j >= k + (int)ns)) {
                lkey[x] = ~0ull;
                lid[x] = kNoId;
            }
        }
        __syncthreads();
        bitonic_lists(lkey, lid, kQ, P, nst);
        if (tid < kQ) {
            const uint32_t ns = min(nst[tid], cap);
            if (ns > 0) {
                const uint32_t c = min((uint32_t)k, cnt[tid] + ns);
                cnt[tid] = c;
                tau[tid] = c == (uint32_t)k ? lkey[tid * P + k - 1] : ~0ull;
                nst[tid] = 0;
                ++cuts;
            }
        }
        __syncthreads();
    };

    const int s0 = slice * a.slice_len;
    const int s1 = min(a.ne, s0 + a.slice_len);
    const uint64_t below_lanes = (1ull << lane) - 1;
    for (int base = s0; base < s1; base += kNbThreads) {
        const int i = base + tid;
        const bool live = i < s1;
        const int x = min(i, s1 - 1);
        double e[kQ];
#pragma unroll
        for (int q = 0; q < kQ; ++q) e[q] = 0;
        for (int c = 0; c < a.n; ++c) {
            const double* col = a.PT + (int64_t)c * a.ne;
            const double v = col[x];
#pragma unroll
            for (int q = 0; q < kQ; ++q) {
                const double p = kRowsInLds ? kr[c * kQ + q] : col[qid[q]];
                const double d = v - p;  // P(x) - P(a); the evaluator's (P(t) - P(h)) - r with r = 0
                e[q] += a.l1 ? fabs(d) : d * d;
            }
        }
        // bit q: this candidate has still to be offered to row q
        uint32_t pend = live ? (1u << nq) - 1u : 0u;
        if (!a.include_self) {
#pragma unroll
            for (int q = 0; q < kQ; ++q)
                if (x == qid[q]) pend &= ~(1u << q);
        }
        while (true) {
            // against the bounds: what is beyond its row's is dropped
            uint32_t pass = 0;
#pragma unroll
            for (int q = 0; q < kQ; ++q)
                if ((uint64_t)__double_as_longlong(e[q]) <= tau[q]) pass |= 1u << q;
            pass &= pend;
            pend = pass;
            // (wave-uniform; the common case once the bounds are set: nothing passes)
            if (__ballot(pass != 0) != 0) {
#pragma unroll 1
                for (int q = 0; q < kQ; ++q) {
                    const bool mine = (pass >> q) & 1u;
                    const uint64_t m = __ballot(mine);
                    if (m == 0) continue;  // (wave-uniform)
                    double eq = e[0];
#pragma unroll
                    for (int j = 1; j < kQ; ++j) eq = q == j ? e[j] : eq;
                    const int leader = __ffsll((long long)m) - 1;
                    uint32_t at = 0;
                    if (lane == leader) at = atomicAdd(&nst[q], (uint32_t)__popcll(m));
                    at = __shfl(at, leader);
                    const uint32_t pos = at + (uint32_t)__popcll(m & below_lanes);
                    if (mine && pos < cap) {
                        lkey[q * P + k + pos] = (uint64_t)__double_as_longlong(eq);
                        lid[q * P + k + pos] = (uint32_t)x;
                        pend &= ~(1u << q);
                    }
                }
            }
            // (block-uniform: the barrier's own result)
            if (!__syncthreads_or(pend != 0)) break;
            prune();
        }
    }
    prune();
    for (int x = tid; x < nq * k; x += kNbThreads) {
        const int q = x / k, j = x % k;
        const bool held = j < (int)cnt[q];
        const int64_t o = ((int64_t)(q0 + q) * a.slices + slice) * k + j;
        a.pkey[o] = held ? lkey[q * P + j] : ~0ull;
        a.pid[o] = held ? lid[q * P + j] : kNoId;
    }
    if (tid < kQ && cuts > 0) atomicAdd(a.prunes, (unsigned long long)cuts);
}

// ------------------------------------------------------------ merge

struct NeighborsMergeArgs {
    const uint64_t* pkey;  // [rows][slices][k]
    const uint32_t* pid;
    int32_t slices, k, P;  // P: the sort buffer, a power of two; P >= slices * k or P == kMergeCap
    int32_t* ids;          // [rows][k]
    double* dist;
    int32_t* found;        // [rows]
};

// One workgroup per query row.  Dynamic LDS: keys [P], ids [P].
__global__ __launch_bounds__(kNbThreads) void neighbors_merge_kernel(NeighborsMergeArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    uint64_t* mkey = (uint64_t*)lds_raw;
    uint32_t* mid = (uint32_t*)(mkey + a.P);
    const int tid = threadIdx.x, k = a.k, P = a.P;
    const int total = a.slices * k;
    const int64_t src = (int64_t)blockIdx.x * total;
    // the k best so far stay in [0, held); the next records fill the rest
    int held = 0;
    for (int pos = 0; pos < total;) {
        const int take = min(P - held, total - pos);
        for (int x = tid; x < P - held; x += kNbThreads) {
            mkey[held + x] = x < take ? a.pkey[src + pos + x] : ~0ull;
            mid[held + x] = x < take ? a.pid[src + pos + x] : kNoId;
        }
        __syncthreads();
        bitonic_lists(mkey, mid, 1, P, nullptr);
        held = min(k, held + take);
        pos += take;
    }
    // (k <= kNbThreads: one record a thread; P >= k or the slots behind P are empty)
    const bool real = tid < k && tid < P && mid[tid] != kNoId;
    const int nf = __syncthreads_count(real);
    if (tid < k) {
        const int64_t o = (int64_t)blockIdx.x * k + tid;
        a.ids[o] = real ? (int32_t)mid[tid] : -1;
        a.dist[o] = real ? __longlong_as_double((long long)mkey[tid]) : __longlong_as_double(0x7ff0000000000000ll);
    }
    if (tid == 0) a.found[blockIdx.x] = nf;
}

// ------------------------------------------------------------ host side

bool env_on(const char* name) {
    const char* v = getenv(name);
    return v && v[0] == '1';
}

long long env_ll(const char* name) {
    const char* v = getenv(name);
    return v ? atoll(v) : 0;
}

int pow2_at_least(int v) {
    int p = 2;
    while (p < v) p <<= 1;
    return p;
}

}  // namespace

void neighbors(const EvalTables& t, const NeighborsQuery& q, int32_t* ids, double* dist, int32_t* found,
               NeighborsStats* stats, const PredictHooks* hooks) {
    const int ne = t.ne, n = t.n, k = q.k;
    const int64_t nq = q.nq;
    if (nq < 1) throw std::invalid_argument("no entities to find neighbours of");
    if (k < 1 || k > kNeighborsMaxK) throw std::invalid_argument("k must be in 1.." + std::to_string(kNeighborsMaxK));
    if (q.include_self != 0 && q.include_self != 1) throw std::invalid_argument("include_self must be 0 or 1");
    if (q.relation < -1 || q.relation >= t.nr) throw std::invalid_argument("relation out of range (-1: the entity space)");
    for (int64_t x = 0; x < nq; ++x)
        if (q.entities[x] < 0 || q.entities[x] >= ne)
            throw std::invalid_argument("entity " + std::to_string(x) + " has an id out of range");

    const SlicePlan plan = plan_slices(ne, nq, k, std::max<long long>(0, env_ll("KB2E_NEIGHBORS_SLICE")),
                                       std::max<long long>(0, env_ll("KB2E_NEIGHBORS_CHUNK_ROWS")));
    const int S = (int)plan.slices;
    const int P = pow2_at_least(k + kNbMinStage);
    const size_t list_lds = (size_t)kQ * P * 12;
    // the tile's rows in LDS where they fit beside the lists; KB2E_EVAL_ROWS_L2=1
    // forces the L2 form as in the evaluator
    // (1 KiB is left for the kernel's static LDS: the bounds and counts)
    const bool rows_lds = list_lds + (size_t)kQ * n * 8 + 1024 <= kLdsMax && !env_on("KB2E_EVAL_ROWS_L2");
    const size_t score_lds = list_lds + (rows_lds ? (size_t)kQ * n * 8 : 0);
    if (rows_lds) allow_lds(neighbors_score_select_kernel<true>, score_lds);
    else allow_lds(neighbors_score_select_kernel<false>, score_lds);
    const int64_t per_query = (int64_t)S * k;
    const int PM = per_query <= kMergeCap ? pow2_at_least((int)per_query) : kMergeCap;
    const size_t merge_lds = (size_t)PM * 12;

    DevBuf d_PT, d_relv, d_ent, d_pkey, d_pid, d_ids, d_dist, d_found, d_prunes;
    d_PT.alloc((size_t)n * ne * 8);
    d_relv.alloc((size_t)n * 8);
    d_ent.alloc((size_t)nq * 4);
    d_pkey.alloc((size_t)plan.chunk_rows * per_query * 8);
    d_pid.alloc((size_t)plan.chunk_rows * per_query * 4);
    d_ids.alloc((size_t)nq * k * 4);
    d_dist.alloc((size_t)nq * k * 8);
    d_found.alloc((size_t)nq * 4);
    d_prunes.alloc(8);
    HIPCHK(hipMemcpyAsync(d_ent.p, q.entities, (size_t)nq * 4, hipMemcpyHostToDevice, t.stream));

    NeighborsStats ns;
    {
        Span sp(hooks, "neighbors_score");
        if (q.relation < 0) {
            EvalTables te = t;  // the entity space: the rows themselves
            te.model = 0;
            project_any(te, 0, d_PT.as<double>(), d_relv.as<double>());
        } else {
            project_any(t, q.relation, d_PT.as<double>(), d_relv.as<double>());
        }
        sp.end();
    }
    for (int64_t r0 = 0; r0 < nq; r0 += plan.chunk_rows) {
        const int64_t rows = std::min(plan.chunk_rows, nq - r0);
        const int64_t tiles = (rows + kQ - 1) / kQ;
        {
            Span sp(hooks, "neighbors_score");
            NeighborsScoreArgs sa{d_PT.as<double>(), n, ne, t.l1, d_ent.as<int32_t>() + r0, (int32_t)rows, S,
                                  (int32_t)plan.slice_len, k, P, q.include_self, d_pkey.as<uint64_t>(),
                                  d_pid.as<uint32_t>(), d_prunes.as<unsigned long long>()};
            const unsigned grid = (unsigned)(tiles * S);
            if (rows_lds) neighbors_score_select_kernel<true><<<grid, kNbThreads, score_lds, t.stream>>>(sa);
            else neighbors_score_select_kernel<false><<<grid, kNbThreads, score_lds, t.stream>>>(sa);
            HIPCHK(hipGetLastError());
            sp.end();
        }
        {
            Span sp(hooks, "neighbors_merge");
            NeighborsMergeArgs ma{d_pkey.as<uint64_t>(), d_pid.as<uint32_t>(), S, k, PM, d_ids.as<int32_t>() + r0 * k,
                                  d_dist.as<double>() + r0 * k, d_found.as<int32_t>() + r0};
            neighbors_merge_kernel<<<(unsigned)rows, kNbThreads, merge_lds, t.stream>>>(ma);
            HIPCHK(hipGetLastError());
            sp.end();
        }
        ns.candidates += rows * (int64_t)ne;
        ns.slices += tiles * S;
        ++ns.chunks;
    }
    unsigned long long prunes = 0;
    HIPCHK(hipMemcpyAsync(ids, d_ids.p, (size_t)nq * k * 4, hipMemcpyDeviceToHost, t.stream));
    HIPCHK(hipMemcpyAsync(dist, d_dist.p, (size_t)nq * k * 8, hipMemcpyDeviceToHost, t.stream));
    HIPCHK(hipMemcpyAsync(found, d_found.p, (size_t)nq * 4, hipMemcpyDeviceToHost, t.stream));
    HIPCHK(hipMemcpyAsync(&prunes, d_prunes.p, 8, hipMemcpyDeviceToHost, t.stream));
    HIPCHK(hipStreamSynchronize(t.stream));
    ns.prunes = (int64_t)prunes;
    if (stats) *stats = ns;
}

}  // namespace kb2e
