// complete.hip -- knowledge-base completion on the device.  Part of libkb2e.so
// (kb2e_complete_triples in engine.hip calls in here).
//
// A query is a relation r; its candidates are the triples (h, t, r) of every
// head h and tail t of the candidate lists (all entities, or the relation's
// head / tail pools), and the answer is the k candidates of smallest energy
// that are not known.  Nothing here ever holds the |H| x |T| keys of a
// relation: a candidate is written down only if it can still be among the k
// best.
//
// * eval_project_kernel projects every entity for the relation once.
// * complete_score_kernel is predict_score_kernel with a tail query -- a tile
//   of kQ head rows in LDS, threads along the tails, one serial FP64 sum per
//   (thread, head), the same operand order, so kb2e_score_triples' bits -- but
//   it stores no key row.  A candidate whose key is at most the relation's
//   bound tau (the k-th best key so far, all-ones until k are held), that is
//   no excluded loop and that the filter set does not hold is appended to the
//   record buffer as (energy bits, h * |E| + t): one ballot per tile row, one
//   atomic per wave and row that has a survivor.  The filter is probed for the
//   survivors of the bound only.
// * The heads are walked in strips sized so that every candidate of a strip
//   fits the buffer (complete_host.hpp): it cannot overflow, and the host
//   never waits for a count.  The first strip is one tile and sets the bound.
// * complete_select_kernel, one 1,024-thread workgroup, after each strip: the
//   relation's running best (<= k records) and the strip's records are one
//   set of distinct 128-bit values (key, pair id).  An 8-bit radix select from
//   the top digit of the key down to the last digit of the pair id narrows a
//   prefix around the k-th smallest until the values at or below it fit the
//   sort buffer -- ties of the key are told apart by the pair id, never by the
//   position in the buffer, whose order differs from run to run --; those are
//   gathered, bitonic-sorted in LDS and become the new best and the new tau.
//   The record count is reset for the next strip on the device.
//
// Everything of a call is queued on the tables' stream, the relations one
// after the other; there is one synchronisation, at the end.  No waiting
// between workgroups anywhere.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "classify_host.hpp"
#include "complete.hpp"
#include "complete_host.hpp"
#include "eval_shared.hpp"
#include "hip_util.hpp"
#include "host_data.hpp"

namespace kb2e {
namespace {

static_assert(kCompleteTile == kQ, "a strip is a whole number of score tiles");

// The record buffer's default capacity: a choice (16 Mi records; at FB15k's
// |E| = 14,951 that is strips of 1,120 heads, 15 steps a relation), not the
// result of a sweep.
constexpr int64_t kCompleteBufferBytes = (int64_t)256 << 20;

// ------------------------------------------------------------ per-query state

// best [nq][k] records, then per query: tau, the held count, and (shared by
// the queries, which run one after the other) the buffer's record count and
// the call's appended-records total.
struct CompleteState {
    ulonglong2* best;                // [nq][k]  .x key, .y pair id; sorted
    uint64_t* tau;                   // [nq]
    uint32_t* nbest;                 // [nq]
    uint32_t* count;                 // records in the buffer
    unsigned long long* appended;    // records appended by the call
};

__global__ __launch_bounds__(256) void complete_init_kernel(CompleteState s, int32_t nq) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x < nq) {
        s.tau[x] = ~0ull;
        s.nbest[x] = 0;
    }
    if (x == 0) {
        *s.count = 0;
        *s.appended = 0;
    }
}

// ------------------------------------------------------------ scoring

struct CompleteScoreArgs {
    const double* PT;    // [n][ne]
    const double* relv;  // [n]
    int32_t n, ne, l1, r;
    const int32_t* hl;  // candidate heads, ascending ids (null: every entity)
    const int32_t* tl;  // candidate tails (null: every entity)
    int32_t h0, nh;     // the strip's heads: list positions [h0, h0 + nh)
    int32_t t0, nt;     // its tails: list positions [t0, t0 + nt)
    int32_t tblocks;    // blocks of 256 tails
    int32_t no_loops;   // h == t is no candidate
    FilterView known;
    const uint64_t* tau;
    uint32_t* count;
    ulonglong2* rec;  // [cap]
    uint32_t cap;
};

// Flat grid: block b takes the tail block b % tblocks of the head tile
// b / tblocks.  Dynamic LDS (kRowsInLds): P(h) of the tile's heads [kQ][n] +
// r [n]; else they are read from the projection table, as predict_score_kernel does.
template <bool kRowsInLds>
__global__ __launch_bounds__(256) void complete_score_kernel(CompleteScoreArgs a) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double* kr = lds;
    double* rv = kr + kQ * a.n;
    const int tile = blockIdx.x / a.tblocks, tb = blockIdx.x % a.tblocks;
    const int q0 = tile * kQ;
    const int nq = min(kQ, a.nh - q0);
    int hid[kQ];
#pragma unroll
    for (int q = 0; q < kQ; ++q) {
        const int pos = a.h0 + q0 + min(q, nq - 1);
        hid[q] = a.hl ? a.hl[pos] : pos;
    }
    if constexpr (kRowsInLds) {
        for (int x = threadIdx.x; x < kQ * a.n; x += blockDim.x) {
            const int q = x / a.n, k = x % a.n;
            const int pos = a.h0 + q0 + min(q, nq - 1);
            kr[x] = a.PT[(int64_t)k * a.ne + (a.hl ? a.hl[pos] : pos)];
        }
        for (int k = threadIdx.x; k < a.n; k += blockDim.x) rv[k] = a.relv[k];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int i = tb * (int)blockDim.x + threadIdx.x;
    const bool live = i < a.nt;
    const int tpos = a.t0 + min(i, a.nt - 1);
    const int tid = a.tl ? a.tl[tpos] : tpos;
    double e[kQ];
#pragma unroll
    for (int q = 0; q < kQ; ++q) e[q] = 0;
    for (int k = 0; k < a.n; ++k) {
        const double* col = a.PT + (int64_t)k * a.ne;
        const double v = col[tid];
        const double r = kRowsInLds ? rv[k] : a.relv[k];
#pragma unroll
        for (int q = 0; q < kQ; ++q) {
            const double p = kRowsInLds ? kr[q * a.n + k] : col[hid[q]];
            const double d = v - p - r;  // (P(t) - P(h)) - r
            e[q] += a.l1 ? fabs(d) : d * d;
        }
    }
    const uint64_t tau = *a.tau;
    const uint64_t below_lanes = (1ull << lane) - 1;
#pragma unroll
    for (int q = 0; q < kQ; ++q) {
        const uint64_t key = (uint64_t)__double_as_longlong(e[q]);
        bool pass = live && q < nq && key <= tau && !(a.no_loops && hid[q] == tid);
        if (pass) pass = !a.known.has(hid[q], a.r, tid);
        const uint64_t m = __ballot(pass);
        if (m == 0) continue;  // (wave-uniform)
        const int leader = __ffsll((long long)m) - 1;
        uint32_t base = 0;
        if (lane == leader) base = atomicAdd(a.count, (uint32_t)__popcll(m));
        base = __shfl(base, leader);
        if (pass) {
            const uint32_t pos = base + (uint32_t)__popcll(m & below_lanes);
            // (a strip's candidates fit the buffer; the check only keeps a store in bounds)
            if (pos < a.cap)
                a.rec[pos] = make_ulonglong2(key, (unsigned long long)hid[q] * (unsigned long long)a.ne +
                                                      (unsigned long long)tid);
        }
    }
}

// ------------------------------------------------------------ selection

constexpr int kSelThreads = 1024;  // one workgroup walks the records: the loads in flight are what it has
constexpr int kSelCap = kPredictMaxK;  // sort buffer, in records
constexpr int kSelMinCap = 256;        // narrow until this many records (or k, if larger) remain

struct CompleteSelectArgs {
    CompleteState s;
    int32_t q, k;
    const ulonglong2* rec;
    uint32_t cap;
};

// digit d of the 128-bit value (key, pair): 0..7 the key's bytes from the top, 8..15 the pair's
__device__ __forceinline__ uint32_t complete_digit(const ulonglong2& v, int d) {
    const uint64_t w = d < 8 ? v.x : v.y;
    return (uint32_t)(w >> (56 - 8 * (d & 7))) & 255u;
}

__global__ __launch_bounds__(kSelThreads) void complete_select_kernel(CompleteSelectArgs a) {
    __shared__ ulonglong2 sv[kSelCap];
    __shared__ uint32_t hist[256];
    __shared__ uint32_t wtot[4];
    __shared__ uint32_t misc[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    ulonglong2* best = a.s.best + (int64_t)a.q * a.k;
    const uint32_t nb = a.s.nbest[a.q];
    const uint32_t nrec = min(*a.s.count, a.cap);
    const uint32_t total = nb + nrec;
    const uint32_t kk = min((uint32_t)a.k, total);
    auto load = [&](uint32_t i) { return i < nb ? best[i] : a.rec[i - nb]; };
    if (nrec == 0) return;  // (block-uniform; nothing new: best, tau and the zero count stand)

    // radix select on the distinct values (key, pair): (pk, pp) under the masks
    // (mk, mp) closes in on the kk-th smallest.  `below` values are under the
    // prefix, `c` on it, and the kk-th is the remaining-th of those.  The
    // values are distinct, so after the last digit c is 1: the loop ends with
    // below + c <= cap at the latest there.
    const uint32_t cap = max(kk, (uint32_t)kSelMinCap);
    uint64_t pk = 0, mk = 0, pp = 0, mp = 0;
    uint32_t below = 0, remaining = kk, c = total;
    for (int d = 0; d < 16 && below + c > cap; ++d) {
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        for (uint32_t base = 0; base < total; base += kSelThreads) {
            const uint32_t i = base + tid;
            bool act = false;
            uint32_t dg = 0;
            if (i < total) {
                const ulonglong2 v = load(i);
                act = (v.x & mk) == pk && (v.y & mp) == pp;
                dg = complete_digit(v, d);
            }
            uint64_t peers = __ballot(act);
            if (peers == 0) continue;  // (wave-uniform)
            // the lanes that hold the same digit add to its bin once
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                const bool bit = (dg >> b) & 1u;
                const uint64_t bal = __ballot(act && bit);
                peers &= bit ? bal : ~bal;
            }
            if (act && lane == __ffsll((long long)peers) - 1) atomicAdd(&hist[dg], (uint32_t)__popcll(peers));
        }
        __syncthreads();
        // the bin that holds the remaining-th value: inclusive scan of the 256 bins
        // by the first four waves (wave-uniform branches)
        uint32_t h = 0, incl = 0;
        if (tid < 256) {
            h = hist[tid];
            incl = h;
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t up = __shfl_up(incl, o);
                if (lane >= o) incl += up;
            }
            if (lane == 63) wtot[wv] = incl;
        }
        __syncthreads();
        if (tid < 256) {
            for (int w = 0; w < wv; ++w) incl += wtot[w];
            const uint32_t excl = incl - h;
            if (excl < remaining && remaining <= incl) {
                misc[0] = (uint32_t)tid;
                misc[1] = excl;
                misc[2] = h;
            }
        }
        __syncthreads();
        const uint32_t bin = misc[0], before = misc[1];
        c = misc[2];
        below += before;
        remaining -= before;
        const int shift = 56 - 8 * (d & 7);
        if (d < 8) {
            pk |= (uint64_t)bin << shift;
            mk |= 0xFFull << shift;
        } else {
            pp |= (uint64_t)bin << shift;
            mp |= 0xFFull << shift;
        }
    }

    // gather the below + c <= cap values at or under the prefix, in any order
    if (tid == 0) misc[3] = 0;
    __syncthreads();
    for (uint32_t i = tid; i < total; i += kSelThreads) {
        const ulonglong2 v = load(i);
        const uint64_t vk = v.x & mk, vp = v.y & mp;
        if (vk < pk || (vk == pk && vp <= pp)) {
            const uint32_t pos = atomicAdd(&misc[3], 1u);
            if (pos < (uint32_t)kSelCap) sv[pos] = v;
        }
    }
    __syncthreads();
    const int nsel = (int)min(misc[3], (uint32_t)kSelCap);
    int P = 2;
    while (P < nsel) P <<= 1;
    for (int i = nsel + tid; i < P; i += kSelThreads) sv[i] = make_ulonglong2(~0ull, ~0ull);
    __syncthreads();
    // bitonic sort of the P values on (key, pair)
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < P / 2; t += kSelThreads) {
                const int lo = 2 * t - (t & (stride - 1));
                const int hi = lo + stride;
                const ulonglong2 va = sv[lo], vb = sv[hi];
                const bool gt = va.x > vb.x || (va.x == vb.x && va.y > vb.y);
                const bool asc = (lo & size) == 0;
                if (gt == asc) {
                    sv[lo] = vb;
                    sv[hi] = va;
                }
            }
            __syncthreads();
        }
    }
    // (every read of the old best and of the records is behind the barriers above)
    for (uint32_t j = tid; j < kk; j += kSelThreads) best[j] = sv[j];
    if (tid == 0) {
        a.s.nbest[a.q] = kk;
        a.s.tau[a.q] = kk == (uint32_t)a.k ? sv[kk - 1].x : ~0ull;
        *a.s.appended += nrec;
        *a.s.count = 0;
    }
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

}  // namespace

void complete_triples(const EvalTables& t, const CompleteQuery& q, int32_t* heads, int32_t* tails, double* energy,
                      int64_t* found, CompleteStats* stats, const PredictHooks* hooks) {
    const int ne = t.ne, n = t.n, k = q.k;
    if (q.nrel < 1) throw std::invalid_argument("no relations to complete");
    if (q.nrel > INT32_MAX) throw std::invalid_argument("too many relations in one call");
    if (k < 1 || k > kPredictMaxK) throw std::invalid_argument("k must be in 1.." + std::to_string(kPredictMaxK));
    if ((q.constrained != 0 && q.constrained != 1) || (q.exclude_loops != 0 && q.exclude_loops != 1))
        throw std::invalid_argument("constrained and exclude_loops must be 0 or 1");
    for (int64_t x = 0; x < q.nrel; ++x)
        if (q.relations[x] < 0 || q.relations[x] >= t.nr)
            throw std::invalid_argument("relation " + std::to_string(x) + " has an id out of range");
    for (int64_t x = 0; x < q.nknown; ++x)
        if (q.kh[x] < 0 || q.kh[x] >= ne || q.kt[x] < 0 || q.kt[x] >= ne || q.kr[x] < 0 || q.kr[x] >= t.nr)
            throw std::invalid_argument("known triple out of range");
    const int64_t nq = q.nrel;

    int64_t buffer_bytes = kCompleteBufferBytes;
    if (const long long v = env_ll("KB2E_COMPLETE_BUFFER_BYTES"); v >= 1) buffer_bytes = std::min<int64_t>(buffer_bytes, v);
    const int64_t strip_cap = std::max<long long>(0, env_ll("KB2E_COMPLETE_STRIP_HEADS"));
    const int64_t cap_records = plan_strips(1, 1, buffer_bytes, strip_cap).cap_records;

    // the known set (FilterSet, as the evaluator's filter) and the pools
    FilterSet fs;
    {
        std::vector<int32_t> H(q.kh, q.kh + q.nknown), T(q.kt, q.kt + q.nknown), R(q.kr, q.kr + q.nknown);
        fs.build(H, T, R, ne, t.nr);
    }
    SlotPools pools;
    if (q.constrained) pools = build_slot_pools(q.kh, q.kt, q.kr, q.nknown, t.nr);

    // n <= 1200 fits; KB2E_EVAL_ROWS_L2=1 forces the L2 form as in the evaluator
    const bool rows_lds = (size_t)(kQ + 1) * n * 8 <= kLdsMax && !env_on("KB2E_EVAL_ROWS_L2");
    const size_t score_lds = rows_lds ? (size_t)(kQ + 1) * n * 8 : 0;
    if (rows_lds) allow_lds(complete_score_kernel<true>, score_lds);

    // the walk of every query, and the largest step: the buffer is allocated for
    // that (never more than its capacity)
    std::vector<StripPlan> plans((size_t)nq);
    int64_t need_records = 1;
    for (int64_t x = 0; x < nq; ++x) {
        const int r = q.relations[x];
        const int64_t nh = q.constrained ? pools.off[(size_t)r * 2 + 1] - pools.off[(size_t)r * 2] : ne;
        const int64_t nt = q.constrained ? pools.off[(size_t)r * 2 + 2] - pools.off[(size_t)r * 2 + 1] : ne;
        if (nh < 1 || nt < 1) continue;  // no candidates: found = 0
        plans[(size_t)x] = plan_strips(nh, nt, buffer_bytes, strip_cap);
        for (const Strip& s : plans[(size_t)x].strips) need_records = std::max(need_records, s.nh * s.nt);
    }
    const uint32_t rec_cap = (uint32_t)std::min(need_records, cap_records);

    DevBuf d_slots, d_pool, d_PT, d_relv, d_rec, d_best, d_tau, d_nbest, d_misc;
    d_slots.alloc(fs.slots.size() * 8);
    HIPCHK(hipMemcpyAsync(d_slots.p, fs.slots.data(), fs.slots.size() * 8, hipMemcpyHostToDevice, t.stream));
    const FilterView known{d_slots.as<uint64_t>(), fs.mask, (uint64_t)t.nr, (uint64_t)ne};
    if (q.constrained && !pools.ids.empty()) {
        d_pool.alloc(pools.ids.size() * 4);
        HIPCHK(hipMemcpyAsync(d_pool.p, pools.ids.data(), pools.ids.size() * 4, hipMemcpyHostToDevice, t.stream));
    }
    d_PT.alloc((size_t)n * ne * 8);
    d_relv.alloc((size_t)n * 8);
    d_rec.alloc((size_t)rec_cap * kCompleteRecordBytes);
    d_best.alloc((size_t)nq * k * 16);
    d_tau.alloc((size_t)nq * 8);
    d_nbest.alloc((size_t)nq * 4);
    d_misc.alloc(16);  // appended (8 bytes), count (4)
    CompleteState st{d_best.as<ulonglong2>(), d_tau.as<uint64_t>(), d_nbest.as<uint32_t>(),
                     d_misc.as<uint32_t>() + 2, d_misc.as<unsigned long long>()};
    complete_init_kernel<<<(unsigned)((nq + 255) / 256), 256, 0, t.stream>>>(st, (int32_t)nq);
    HIPCHK(hipGetLastError());

    CompleteStats cs;
    cs.buffer_records = cap_records;
    int cur_rel = -1;  // the relation d_PT holds
    for (int64_t x = 0; x < nq; ++x) {
        const int r = q.relations[x];
        const int32_t *hl = nullptr, *tl = nullptr;
        if (q.constrained) {
            hl = d_pool.as<int32_t>() + pools.off[(size_t)r * 2];
            tl = d_pool.as<int32_t>() + pools.off[(size_t)r * 2 + 1];
        }
        for (const Strip& s : plans[(size_t)x].strips) {
            {
                Span sp(hooks, "complete_score");
                if (r != cur_rel) {
                    project_any(t, r, d_PT.as<double>(), d_relv.as<double>());
                    cur_rel = r;
                }
                const int64_t tblocks = (s.nt + 255) / 256, tiles = (s.nh + kQ - 1) / kQ;
                CompleteScoreArgs sa{d_PT.as<double>(), d_relv.as<double>(), n, ne, t.l1, r, hl, tl,
                                     (int32_t)s.h0, (int32_t)s.nh, (int32_t)s.t0, (int32_t)s.nt, (int32_t)tblocks,
                                     q.exclude_loops, known, st.tau + x, st.count, d_rec.as<ulonglong2>(), rec_cap};
                const unsigned grid = (unsigned)(tblocks * tiles);
                if (rows_lds) complete_score_kernel<true><<<grid, 256, score_lds, t.stream>>>(sa);
                else complete_score_kernel<false><<<grid, 256, 0, t.stream>>>(sa);
                HIPCHK(hipGetLastError());
                sp.end();
            }
            {
                Span sp(hooks, "complete_select");
                CompleteSelectArgs la{st, (int32_t)x, k, d_rec.as<ulonglong2>(), rec_cap};
                complete_select_kernel<<<1, kSelThreads, 0, t.stream>>>(la);
                HIPCHK(hipGetLastError());
                sp.end();
            }
            cs.candidates += s.nh * s.nt;
            ++cs.strips;
        }
    }

    std::vector<ulonglong2> hbest((size_t)nq * k);
    std::vector<uint32_t> hnbest((size_t)nq);
    unsigned long long appended = 0;
    HIPCHK(hipMemcpyAsync(hbest.data(), d_best.p, hbest.size() * 16, hipMemcpyDeviceToHost, t.stream));
    HIPCHK(hipMemcpyAsync(hnbest.data(), d_nbest.p, hnbest.size() * 4, hipMemcpyDeviceToHost, t.stream));
    HIPCHK(hipMemcpyAsync(&appended, d_misc.p, 8, hipMemcpyDeviceToHost, t.stream));
    HIPCHK(hipStreamSynchronize(t.stream));
    cs.records = (int64_t)appended;
    for (int64_t x = 0; x < nq; ++x) {
        const int64_t nf = hnbest[(size_t)x];
        found[x] = nf;
        for (int64_t j = 0; j < k; ++j) {
            const size_t o = (size_t)(x * k + j);
            if (j < nf) {
                const ulonglong2 v = hbest[o];
                heads[o] = pair_head(v.y, ne);
                tails[o] = pair_tail(v.y, ne);
                const long long bits = (long long)v.x;
                double e;
                static_assert(sizeof(e) == sizeof(bits), "IEEE-754 double");
                __builtin_memcpy(&e, &bits, 8);
                energy[o] = e;
            } else {
                heads[o] = tails[o] = -1;
                energy[o] = std::numeric_limits<double>::infinity();
            }
        }
    }
    if (stats) *stats = cs;
}

}  // namespace kb2e
