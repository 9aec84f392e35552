// predict.hip -- top-k link-prediction queries, relation prediction and triple
// scoring on the device.  Part of libkb2e.so (kb2e_predict, kb2e_score_triples,
// kb2e_predict_relations, kb2e_rank_relations in engine.hip call in here).
//
// A query (e, r, side) asks for the k entities x of smallest energy of
// (e, x, r) (side 1: the tail is unknown) or (x, e, r) (side 0: the head is),
// known triples excluded.  Energies are the evaluator's stateless ones:
// eval_project_kernel projects every entity for one relation, and
// predict_score_kernel -- the one-sided form of eval_rank_kernel, same operand
// order, so the same bits -- gives one thread per candidate and a tile of kQ
// queries, and stores each energy's IEEE-754 bit pattern as the candidate's
// key in keys[query][|E|].  Energies are sums of fabs() or squares, so >= +0,
// and unsigned order of the patterns is numeric order.
//
// * predict_mask_kernel overwrites the keys of the known candidates with ~0:
//   the host lists them per distinct (e, r, side) from the filter triples
//   (predict_host.hpp), so no hash set is probed per (query, candidate).
// * predict_select_kernel, one 256-thread workgroup per query: the key row is
//   staged in LDS while it is small enough to leave four workgroups a CU, else
//   re-read from L2 on every pass (FB15k's 120 KB row fits the 160 KB, but
//   one workgroup a CU measured 3.2x slower); an 8-bit radix select from the top digit
//   narrows a prefix around the k-th smallest key (256-bin LDS histogram, the
//   lanes of a wave that share a digit add once) until the keys at or below
//   the prefix fit the sort buffer; those are compacted in id order -- every
//   key below the prefix, keys on it in ascending id until there are enough --
//   and bitonic-sorted on (key, id) in LDS.  No communication between
//   workgroups, no waiting on other work, no device-side allocation.
//
// The key buffer holds a bounded chunk of queries (<= 1 GiB), so a whole test
// set's queries never need nq x |E| at once.
//
// Relation prediction (a pair (h, t) against every relation) writes
// keys[query][|R|] with kernels of its own -- relpred_direct_kernel for TransE /
// TransH, relpred_project_kernel + relpred_pair_kernel for TransR -- and shares
// the mask and the selection; relpred_rank_kernel counts the per-triple ranks.
//
// Conjunctive queries (kb2e_predict_joint, kb2e_rank_joint: several one-sided
// patterns about one unknown entity) score every pattern as a row with
// predict_score_kernel, add a query's rows with joint_combine_kernel and share
// the mask, the selection and the rank count.
//
// Path queries (kb2e_predict_path, kb2e_rank_path: the entities at the end of a
// relation path) score the first hop with predict_score_kernel, take every
// further hop with the fused min-plus path_hop_kernel and share the mask, the
// selection and the rank count (the last section of this file).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <limits>
#include <numeric>
#include <stdexcept>
#include <vector>

#include "eval_shared.hpp"
#include "hip_util.hpp"
#include "joint_host.hpp"
#include "kernels_common.hpp"
#include "path_host.hpp"
#include "predict.hpp"
#include "predict_host.hpp"

namespace kb2e {
namespace {

constexpr uint64_t kMasked = ~0ull;

// ------------------------------------------------------------ candidate keys

struct ScoreArgs {
    const double* PT;    // [n][ne]
    const double* relv;  // [n]
    int32_t n, ne, l1;
    const int32_t* qe;     // the known entity of each query of this relation
    const int32_t* qside;  // 1: candidates are tails, 0: heads
    int32_t nq;
    uint64_t* keys;  // [nq][ne]
};

// grid.x: entity blocks of 256; grid.y: query tiles of kQ.  Dynamic LDS: P(e)
// of the tile's queries [kQ][n] + r [n]; kRowsInLds false reads them from the
// projection table (L1 / L2 broadcast), as eval_rank_kernel does.
template <bool kRowsInLds>
__global__ __launch_bounds__(256) void predict_score_kernel(ScoreArgs a) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double* kr = lds;
    double* rv = kr + kQ * a.n;
    const int q0 = blockIdx.y * kQ;
    const int nq = min(kQ, a.nq - q0);
    if constexpr (kRowsInLds) {
        for (int x = threadIdx.x; x < kQ * a.n; x += blockDim.x) {
            const int q = x / a.n, k = x % a.n;
            if (q < nq) kr[x] = a.PT[(int64_t)k * a.ne + a.qe[q0 + q]];
        }
        for (int k = threadIdx.x; k < a.n; k += blockDim.x) rv[k] = a.relv[k];
    }
    int qev[kQ];
    bool tailq[kQ];
#pragma unroll
    for (int q = 0; q < kQ; ++q) {
        qev[q] = q < nq ? a.qe[q0 + q] : 0;
        tailq[q] = q < nq ? a.qside[q0 + q] != 0 : false;
    }
    __syncthreads();
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.ne) return;
    double e[kQ];
#pragma unroll
    for (int q = 0; q < kQ; ++q) e[q] = 0;
    for (int k = 0; k < a.n; ++k) {
        const double* col = a.PT + (int64_t)k * a.ne;
        const double v = col[i];
        const double r = kRowsInLds ? rv[k] : a.relv[k];
#pragma unroll
        for (int q = 0; q < kQ; ++q) {
            const double p = kRowsInLds ? kr[q * a.n + k] : col[qev[q]];
            // (P(x) - P(h)) - r with x the tail, (P(t) - P(x)) - r with x the head
            const double d = tailq[q] ? v - p - r : p - v - r;
            e[q] += a.l1 ? fabs(d) : d * d;
        }
    }
#pragma unroll
    for (int q = 0; q < kQ; ++q)
        if (q < nq) a.keys[(int64_t)(q0 + q) * a.ne + i] = (uint64_t)__double_as_longlong(e[q]);
}

struct MaskArgs {
    uint64_t* keys;  // [rows][ne]
    int32_t ne;
    const int32_t* group;  // [rows]
    const int64_t* off;
    const int32_t* ids;
};

// One block per query row: the known candidates of its (e, r, side) get the key ~0.
__global__ __launch_bounds__(256) void predict_mask_kernel(MaskArgs a) {
    const int g = a.group[blockIdx.x];
    uint64_t* row = a.keys + (int64_t)blockIdx.x * a.ne;
    for (int64_t j = a.off[g] + threadIdx.x; j < a.off[g + 1]; j += blockDim.x) row[a.ids[j]] = kMasked;
}

// ------------------------------------------------------------ selection

constexpr int kSelThreads = 256;
constexpr int kSelCap = kPredictMaxK;  // sort buffer, in pairs
constexpr int kSelMinCap = 256;        // narrow until this many pairs (or k, if larger) remain
// scratch: keys [1024] u64, ids [1024] i32, histogram [256] u32, wave totals [2][4][2] u32, misc [8] u32
constexpr size_t kSelOffIds = (size_t)kSelCap * 8;
constexpr size_t kSelOffHist = kSelOffIds + (size_t)kSelCap * 4;
constexpr size_t kSelOffWtot = kSelOffHist + 256 * 4;
constexpr size_t kSelOffMisc = kSelOffWtot + 16 * 4;
constexpr size_t kSelScratchBytes = kSelOffMisc + 16 * 4;
static_assert(kSelScratchBytes % 16 == 0, "the key row behind the scratch is 8-byte data");

struct SelectArgs {
    const uint64_t* keys;  // [rows][ne]
    int32_t ne, k;
    int32_t* ids;    // [rows][k]
    double* energy;  // [rows][k]
    int32_t* found;  // [rows]
};

template <bool kRowLds>
__global__ __launch_bounds__(kSelThreads) void predict_select_kernel(SelectArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
    uint64_t* skey = (uint64_t*)sm;
    int32_t* sid = (int32_t*)(sm + kSelOffIds);
    uint32_t* hist = (uint32_t*)(sm + kSelOffHist);
    uint32_t* wtot = (uint32_t*)(sm + kSelOffWtot);
    uint32_t* misc = (uint32_t*)(sm + kSelOffMisc);
    uint64_t* lrow = (uint64_t*)(sm + kSelScratchBytes);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int ne = a.ne;
    const uint64_t* grow = a.keys + (int64_t)blockIdx.x * ne;
    const uint64_t* row = kRowLds ? lrow : grow;
    const uint64_t below_lanes = (1ull << lane) - 1;

    // stage the row, count the candidates left
    uint32_t mine = 0;
    for (int i = tid; i < ne; i += kSelThreads) {
        const uint64_t key = grow[i];
        if constexpr (kRowLds) lrow[i] = key;
        mine += key != kMasked;
    }
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o);
    if (lane == 0) misc[4 + wv] = mine;  // (slots no later phase writes)
    __syncthreads();
    const int valid = (int)(misc[4] + misc[5] + misc[6] + misc[7]);
    const int kk = min(a.k, valid);
    int32_t* oid = a.ids + (int64_t)blockIdx.x * a.k;
    double* oen = a.energy + (int64_t)blockIdx.x * a.k;
    if (tid == 0) a.found[blockIdx.x] = kk;
    if (kk == 0) {  // (block-uniform)
        for (int j = tid; j < a.k; j += kSelThreads) {
            oid[j] = -1;
            oen[j] = INFINITY;
        }
        return;
    }

    // radix select: (prefix, pmask) closes in on the kk-th smallest key.  `below`
    // keys are under the prefix, `c` keys on it (the masked ones too while pmask
    // is 0), and the kk-th is the remaining-th of those.
    const uint32_t cap = (uint32_t)max(kk, kSelMinCap);
    uint64_t prefix = 0, pmask = 0;
    uint32_t below = 0, remaining = (uint32_t)kk, c = (uint32_t)ne;
    for (int shift = 56; shift >= 0 && below + c > cap; shift -= 8) {
        hist[tid] = 0;
        __syncthreads();
        for (int base = 0; base < ne; base += kSelThreads) {
            const int i = base + tid;
            bool act = false;
            uint32_t dg = 0;
            if (i < ne) {
                const uint64_t key = row[i];
                act = (key & pmask) == prefix;
                dg = (uint32_t)(key >> shift) & 255u;
            }
            if (__ballot(act) == 0) continue;  // (wave-uniform)
            // the lanes that hold the same digit add to its bin once
            uint64_t peers = __ballot(act);
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                const bool bit = (dg >> b) & 1u;
                const uint64_t bal = __ballot(act && bit);
                peers &= bit ? bal : ~bal;
            }
            if (act && lane == __ffsll((long long)peers) - 1) atomicAdd(&hist[dg], (uint32_t)__popcll(peers));
        }
        __syncthreads();
        // the bin that holds the remaining-th key: inclusive scan of the 256 bins
        const uint32_t h = hist[tid];
        uint32_t incl = h;
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t up = __shfl_up(incl, o);
            if (lane >= o) incl += up;
        }
        if (lane == 63) wtot[wv] = incl;
        __syncthreads();
        for (int w = 0; w < wv; ++w) incl += wtot[w];
        const uint32_t excl = incl - h;
        if (excl < remaining && remaining <= incl) {
            misc[0] = (uint32_t)tid;
            misc[1] = excl;
            misc[2] = h;
        }
        __syncthreads();
        const uint32_t bin = misc[0], before = misc[1];
        c = misc[2];
        below += before;
        remaining -= before;
        prefix |= (uint64_t)bin << shift;
        pmask |= 0xFFull << shift;
    }
    // every key on the prefix when they fit; else (all digits fixed: equal keys)
    // the first `remaining` of them by id
    const uint32_t need_eq = below + c <= cap ? c : remaining;

    // compaction in id order: keys under the prefix to [0, below), keys on it
    // behind them; never a masked key
    uint32_t run_l = 0, run_e = 0;
    int it = 0;
    for (int base = 0; base < ne; base += kSelThreads, ++it) {
        const int i = base + tid;
        bool L = false, E = false;
        uint64_t key = 0;
        if (i < ne) {
            key = row[i];
            if (key != kMasked) {
                const uint64_t mk = key & pmask;
                L = mk < prefix;
                E = mk == prefix;
            }
        }
        const uint64_t mL = __ballot(L), mE = __ballot(E);
        uint32_t* wt = wtot + (it & 1) * 8;
        if (lane == 0) {
            wt[wv * 2] = (uint32_t)__popcll(mL);
            wt[wv * 2 + 1] = (uint32_t)__popcll(mE);
        }
        __syncthreads();
        uint32_t off_l = run_l, off_e = run_e;
#pragma unroll
        for (int w = 0; w < kSelThreads / 64; ++w) {
            const uint32_t cl = wt[w * 2], ce = wt[w * 2 + 1];
            if (w < wv) {
                off_l += cl;
                off_e += ce;
            }
            run_l += cl;
            run_e += ce;
        }
        if (L) {
            const uint32_t pos = off_l + (uint32_t)__popcll(mL & below_lanes);
            if (pos < (uint32_t)kSelCap) {
                skey[pos] = key;
                sid[pos] = i;
            }
        }
        if (E) {
            const uint32_t rk = off_e + (uint32_t)__popcll(mE & below_lanes);
            const uint32_t pos = below + rk;
            if (rk < need_eq && pos < (uint32_t)kSelCap) {
                skey[pos] = key;
                sid[pos] = i;
            }
        }
    }
    const int nsel = (int)min(below + min(run_e, need_eq), (uint32_t)kSelCap);
    int P = 2;
    while (P < nsel) P <<= 1;
    for (int i = nsel + tid; i < P; i += kSelThreads) {
        skey[i] = kMasked;
        sid[i] = INT_MAX;
    }
    __syncthreads();
    // bitonic sort of the P pairs on (key, id)
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < P / 2; t += kSelThreads) {
                const int lo = 2 * t - (t & (stride - 1));
                const int hi = lo + stride;
                const uint64_t ka = skey[lo], kb = skey[hi];
                const int32_t ia = sid[lo], ib = sid[hi];
                const bool gt = ka > kb || (ka == kb && ia > ib);
                const bool asc = (lo & size) == 0;
                if (gt == asc) {
                    skey[lo] = kb;
                    skey[hi] = ka;
                    sid[lo] = ib;
                    sid[hi] = ia;
                }
            }
            __syncthreads();
        }
    }
    for (int j = tid; j < a.k; j += kSelThreads) {
        const bool have = j < kk;
        oid[j] = have ? sid[j] : -1;
        oen[j] = have ? __longlong_as_double((long long)skey[j]) : (double)INFINITY;
    }
}

// ------------------------------------------------------------ triple energies

template <typename T>
struct TripleArgs {
    int32_t model, n, ld, l1;
    const T* ent;
    const T* rel;
    const T* w;
    const int32_t *h, *t, *r;
    int32_t count;
    double* out;
};

// TransE (transe/transe.cpp) and TransH (transh/transh.cpp:10-29): one thread
// per triple, the reference's serial loops in FP64.
template <typename T>
__global__ __launch_bounds__(256) void score_triples_kernel(TripleArgs<T> a) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= a.count) return;
    const T* h = a.ent + (int64_t)a.h[x] * a.ld;
    const T* t = a.ent + (int64_t)a.t[x] * a.ld;
    const T* r = a.rel + (int64_t)a.r[x] * a.ld;
    double e = 0;
    if (a.model == 0) {
        for (int k = 0; k < a.n; ++k) {
            const double d = (double)t[k] - (double)h[k] - (double)r[k];
            e += a.l1 ? fabs(d) : d * d;
        }
    } else {
        const T* w = a.w + (int64_t)a.r[x] * a.ld;
        double hs = 0, ts = 0;
        for (int k = 0; k < a.n; ++k) {
            hs += (double)w[k] * (double)h[k];
            ts += (double)w[k] * (double)t[k];
        }
        for (int k = 0; k < a.n; ++k)
            e += fabs((double)t[k] - ts * (double)w[k] - ((double)h[k] - hs * (double)w[k]) - (double)r[k]);
    }
    a.out[x] = e;
}

// TransR (transr/transr.cpp:13-37, zeroed work vectors): one wave per triple.
// Lane i (+64c) accumulates headVec[i] and tailVec[i] over j in order from
// zero; the terms go through LDS and lane 0 adds them over i in order.
// Dynamic LDS: [waves][n] doubles.
template <typename T>
__global__ __launch_bounds__(256) void score_triples_transr_kernel(TripleArgs<T> a) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int wv = threadIdx.x >> 6, l = lane_id();
    const int x = blockIdx.x * (blockDim.x >> 6) + wv;
    if (x >= a.count) return;  // (wave-uniform; no workgroup barrier below)
    double* term = lds + (size_t)wv * a.n;
    const T* h = a.ent + (int64_t)a.h[x] * a.ld;
    const T* t = a.ent + (int64_t)a.t[x] * a.ld;
    const T* r = a.rel + (int64_t)a.r[x] * a.ld;
    const T* W = a.w + (int64_t)a.r[x] * a.n * a.ld;
    for (int i = l; i < a.n; i += 64) {
        double hv = 0, tv = 0;
        for (int j = 0; j < a.n; ++j) {
            const double w = (double)W[(int64_t)j * a.ld + i];
            hv += w * (double)h[j];
            tv += w * (double)t[j];
        }
        const double d = tv - hv - (double)r[i];
        term[i] = a.l1 ? fabs(d) : d * d;
    }
    wave_lds_sync();
    if (l == 0) {
        double e = 0;
        for (int i = 0; i < a.n; ++i) e += term[i];
        a.out[x] = e;
    }
}

// ------------------------------------------------------------ relation prediction
//
// A query is a pair (h, t) and its candidates are the |R| relations: the keys
// are keys[query][|R|], every energy the bits score_triples_kernel /
// score_triples_transr_kernel give for the same triple (the same expressions,
// each sum serial from zero in the reference's order).

// FP64 transposed copy [n][|R|] of a [|R|][ld] table (relation rows, TransH
// normals), made once per call: with one thread per relation candidate, the
// loads of element k of 64 neighbouring relations are then one 512-byte
// segment instead of 64 rows ld apart, and FP32 tables are widened once.
template <typename T>
__global__ __launch_bounds__(256) void relpred_transpose_kernel(const T* src, int32_t n, int32_t ld, int32_t nr,
                                                                double* dst) {
    const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= (int64_t)n * nr) return;
    const int k = (int)(x / nr), r = (int)(x % nr);
    dst[x] = (double)src[(int64_t)r * ld + k];
}

template <typename T>
struct RelDirectArgs {
    int32_t n, ld, nr, l1;
    const T* ent;
    const double* RT;        // [n][nr] relation rows
    const double* WT;        // [n][nr] TransH normals
    const int32_t *qh, *qt;  // the chunk's pairs
    int32_t nq;
    uint64_t* keys;  // [nq][nr]
};

// TransE / TransH.  grid.x: relation blocks of 256; grid.y: query tiles of kQ.
// Dynamic LDS: the tile's head and tail rows widened to FP64, interleaved
// [kQ][n][2] so that one 16-byte LDS read (a broadcast: every lane reads the
// same address) gives both.  One thread per relation walks score_triples_kernel's
// loops for the kQ pairs; the key stores run along the relations (coalesced).
template <typename T, bool kTransH>
__global__ __launch_bounds__(256) void relpred_direct_kernel(RelDirectArgs<T> a) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int n = a.n;
    const int q0 = blockIdx.y * kQ;
    const int nq = min(kQ, a.nq - q0);
    for (int x = threadIdx.x; x < kQ * n; x += blockDim.x) {
        const int q = x / n, k = x % n;
        const bool in = q < nq;
        lds[2 * x] = in ? (double)a.ent[(int64_t)a.qh[q0 + q] * a.ld + k] : 0.0;
        lds[2 * x + 1] = in ? (double)a.ent[(int64_t)a.qt[q0 + q] * a.ld + k] : 0.0;
    }
    __syncthreads();
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.nr) return;
    const double2* ht = (const double2*)lds;  // .x head, .y tail
    double e[kQ];
#pragma unroll
    for (int q = 0; q < kQ; ++q) e[q] = 0;
    if constexpr (!kTransH) {
        for (int k = 0; k < n; ++k) {
            const double rv = a.RT[(int64_t)k * a.nr + r];
#pragma unroll
            for (int q = 0; q < kQ; ++q) {
                const double2 p = ht[q * n + k];
                const double d = p.y - p.x - rv;
                e[q] += a.l1 ? fabs(d) : d * d;
            }
        }
    } else {
        double hs[kQ], ts[kQ];
#pragma unroll
        for (int q = 0; q < kQ; ++q) hs[q] = ts[q] = 0;
        for (int k = 0; k < n; ++k) {
            const double w = a.WT[(int64_t)k * a.nr + r];
#pragma unroll
            for (int q = 0; q < kQ; ++q) {
                const double2 p = ht[q * n + k];
                hs[q] += w * p.x;
                ts[q] += w * p.y;
            }
        }
        for (int k = 0; k < n; ++k) {
            const double w = a.WT[(int64_t)k * a.nr + r];
            const double rv = a.RT[(int64_t)k * a.nr + r];
#pragma unroll
            for (int q = 0; q < kQ; ++q) {
                const double2 p = ht[q * n + k];
                e[q] += fabs(p.y - ts[q] * w - (p.x - hs[q] * w) - rv);
            }
        }
    }
#pragma unroll
    for (int q = 0; q < kQ; ++q)
        if (q < nq) a.keys[(int64_t)(q0 + q) * a.nr + r] = (uint64_t)__double_as_longlong(e[q]);
}

template <typename T>
struct RelProjArgs {
    int32_t n, ld, nu, r0;
    const T* ent;
    const T* w;
    const int32_t* ents;  // [nu] the chunk's distinct entities
    double* PT;           // [batch][n][nu]
};

constexpr int kProjK = 8;  // outputs a thread accumulates at once

// TransR.  grid.x: blocks of 256 listed entities; grid.y: the relations of the
// batch; grid.z: groups of kProjK outputs k.  A thread projects entity ents[u]
// with relation r0 + blockIdx.y for its group's outputs: eval_project_kernel's
// sum for each k (the same j order from zero: the bits of
// score_triples_transr_kernel's hv / tv), kProjK of them side by side, so that
// each e[j] is loaded once per group instead of once per output.  W_r is read
// at workgroup-uniform addresses (scalar loads through the scalar cache and
// L2), not staged in LDS: DESIGN.md 14.  kFull: the group lies inside the row
// (its kProjK matrix elements of a step are one contiguous run); the ragged
// last group clamps its column and skips the stores past n.
template <typename T, bool kFull>
__device__ __forceinline__ void relpred_project_group(const T* __restrict__ e, const T* __restrict__ W, int n, int ld,
                                                      int k0, double* __restrict__ out, int64_t nu) {
    int col[kProjK];
#pragma unroll
    for (int c = 0; c < kProjK; ++c) col[c] = kFull ? k0 + c : min(k0 + c, n - 1);
    double s[kProjK];
#pragma unroll
    for (int c = 0; c < kProjK; ++c) s[c] = 0;
#pragma unroll 2
    for (int j = 0; j < n; ++j) {
        const double ej = (double)e[j];
        const T* wr = W + (int64_t)j * ld;
#pragma unroll
        for (int c = 0; c < kProjK; ++c) s[c] += (double)wr[col[c]] * ej;
    }
#pragma unroll
    for (int c = 0; c < kProjK; ++c)
        if (kFull || k0 + c < n) out[(int64_t)(k0 + c) * nu] = s[c];
}

template <typename T>
__global__ __launch_bounds__(256) void relpred_project_kernel(RelProjArgs<T> a) {
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= a.nu) return;
    const int b = blockIdx.y, k0 = blockIdx.z * kProjK;
    const T* e = a.ent + (int64_t)a.ents[u] * a.ld;
    const T* W = a.w + (int64_t)(a.r0 + b) * a.n * a.ld;
    double* out = a.PT + (int64_t)b * a.n * a.nu + u;
    if (k0 + kProjK <= a.n) relpred_project_group<T, true>(e, W, a.n, a.ld, k0, out, a.nu);
    else relpred_project_group<T, false>(e, W, a.n, a.ld, k0, out, a.nu);
}

constexpr int kPairQ = 64;  // pairs per tile: the lanes of a wave
constexpr int kPairR = 32;  // relations per tile: 256-byte runs of a key row

template <typename T>
struct RelPairArgs {
    int32_t n, ld, nu, nr, l1, r0, nb;
    const T* rel;
    const double* PT;        // [nb][n][nu]
    const int32_t *hi, *ti;  // [nq] the pairs as indices into the entity list
    int32_t nq;
    uint64_t* keys;  // [nq][nr]
};

// TransR.  grid.x: tiles of kPairQ pairs; grid.y: tiles of kPairR relations of
// the batch.  Lanes run along the pairs (the two gathers of a step stay inside
// one row PT[b][i][.] of the list), each wave takes every fourth relation of the
// tile: (P_r(t) - P_r(h)) - r term by term, summed over i in order.  The store
// to keys[q][r] has a stride of |R| * 8 bytes along the lanes; kTranspose turns
// the tile through LDS so that 32 lanes write one 256-byte run of a key row.
template <typename T, bool kTranspose>
__global__ __launch_bounds__(256) void relpred_pair_kernel(RelPairArgs<T> a) {
    __shared__ uint64_t tile[kTranspose ? kPairQ : 1][kPairR + 1];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int q = blockIdx.x * kPairQ + lane;
    const bool live = q < a.nq;
    const int hu = live ? a.hi[q] : 0, tu = live ? a.ti[q] : 0;
    const int b0 = blockIdx.y * kPairR;
    for (int rl = wv; rl < kPairR; rl += 4) {
        const int b = b0 + rl;
        if (b >= a.nb) break;  // (wave-uniform)
        const double* P = a.PT + (int64_t)b * a.n * a.nu;
        const T* rv = a.rel + (int64_t)(a.r0 + b) * a.ld;
        double e = 0;
        for (int i = 0; i < a.n; ++i) {
            const double* row = P + (int64_t)i * a.nu;
            const double d = row[tu] - row[hu] - (double)rv[i];
            e += a.l1 ? fabs(d) : d * d;
        }
        const uint64_t key = (uint64_t)__double_as_longlong(e);
        if constexpr (kTranspose) tile[lane][rl] = key;
        else if (live) a.keys[(int64_t)q * a.nr + a.r0 + b] = key;
    }
    if constexpr (kTranspose) {
        __syncthreads();
        for (int x = threadIdx.x; x < kPairQ * kPairR; x += blockDim.x) {
            const int ql = x / kPairR, rl = x % kPairR;
            const int qq = blockIdx.x * kPairQ + ql, b = b0 + rl;
            if (qq < a.nq && b < a.nb) a.keys[(int64_t)qq * a.nr + a.r0 + b] = tile[ql][rl];
        }
    }
}

struct RelRankArgs {
    const uint64_t* keys;  // [rows][nr], not yet masked
    int32_t nr;
    const int32_t* truth;  // [rows]
    const int32_t* group;  // [rows]
    const int64_t* off;
    const int32_t* ids;
    int64_t* ranks;  // [rows][2]
};

// One workgroup per row: the keys strictly below the truth's are the raw rank;
// those of the pair's known relations (other than the truth) that are also
// below it do not count in the filtered one.
__global__ __launch_bounds__(256) void relpred_rank_kernel(RelRankArgs a) {
    __shared__ uint32_t part[4][2];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t* row = a.keys + (int64_t)blockIdx.x * a.nr;
    const int tr = a.truth[blockIdx.x];
    const uint64_t tkey = row[tr];
    uint32_t below = 0, known = 0;
    for (int i = threadIdx.x; i < a.nr; i += blockDim.x) below += row[i] < tkey;
    const int g = a.group[blockIdx.x];
    for (int64_t j = a.off[g] + threadIdx.x; j < a.off[g + 1]; j += blockDim.x) {
        const int id = a.ids[j];
        known += id != tr && row[id] < tkey;
    }
    for (int o = 32; o > 0; o >>= 1) {
        below += __shfl_down(below, o);
        known += __shfl_down(known, o);
    }
    if (lane == 0) {
        part[wv][0] = below;
        part[wv][1] = known;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int64_t b = (int64_t)part[0][0] + part[1][0] + part[2][0] + part[3][0];
        const int64_t kn = (int64_t)part[0][1] + part[1][1] + part[2][1] + part[3][1];
        a.ranks[(int64_t)blockIdx.x * 2] = 1 + b;
        a.ranks[(int64_t)blockIdx.x * 2 + 1] = 1 + b - kn;
    }
}

// ------------------------------------------------------------ host side

bool env_on(const char* name) {
    const char* v = getenv(name);
    return v && v[0] == '1';
}

template <typename T>
void run_score_triples(const EvalTables& t, const int32_t* dh, const int32_t* dt, const int32_t* dr, int32_t count,
                       double* dout) {
    TripleArgs<T> a{t.model, t.n, t.ld, t.l1, (const T*)t.ent, (const T*)t.rel, (const T*)t.w, dh, dt, dr, count, dout};
    if (t.model == 2) {
        const size_t lds = (size_t)4 * t.n * 8;
        score_triples_transr_kernel<T><<<(count + 3) / 4, 256, lds, t.stream>>>(a);
    } else {
        score_triples_kernel<T><<<(count + 255) / 256, 256, 0, t.stream>>>(a);
    }
    HIPCHK(hipGetLastError());
}

}  // namespace

void score_triples_device(const EvalTables& t, const int32_t* dh, const int32_t* dt, const int32_t* dr, int64_t count,
                          double* dout) {
    const int64_t chunk = (int64_t)1 << 22;
    for (int64_t c0 = 0; c0 < count; c0 += chunk) {
        const int32_t m = (int32_t)std::min(chunk, count - c0);
        if (t.f64) run_score_triples<double>(t, dh + c0, dt + c0, dr + c0, m, dout + c0);
        else run_score_triples<float>(t, dh + c0, dt + c0, dr + c0, m, dout + c0);
    }
}

void score_triples(const EvalTables& t, const int32_t* heads, const int32_t* tails, const int32_t* relations,
                   int64_t count, double* energy) {
    if (count < 1) throw std::invalid_argument("no triples to score");
    for (int64_t k = 0; k < count; ++k)
        if (heads[k] < 0 || heads[k] >= t.ne || tails[k] < 0 || tails[k] >= t.ne || relations[k] < 0 ||
            relations[k] >= t.nr)
            throw std::invalid_argument("triple " + std::to_string(k) + " has an id out of range");
    const int64_t chunk = std::min<int64_t>(count, (int64_t)1 << 22);
    DevBuf d_h, d_t, d_r, d_out;
    d_h.alloc((size_t)chunk * 4);
    d_t.alloc((size_t)chunk * 4);
    d_r.alloc((size_t)chunk * 4);
    d_out.alloc((size_t)chunk * 8);
    for (int64_t c0 = 0; c0 < count; c0 += chunk) {
        const int32_t m = (int32_t)std::min(chunk, count - c0);
        HIPCHK(hipMemcpyAsync(d_h.p, heads + c0, (size_t)m * 4, hipMemcpyHostToDevice, t.stream));
        HIPCHK(hipMemcpyAsync(d_t.p, tails + c0, (size_t)m * 4, hipMemcpyHostToDevice, t.stream));
        HIPCHK(hipMemcpyAsync(d_r.p, relations + c0, (size_t)m * 4, hipMemcpyHostToDevice, t.stream));
        if (t.f64) run_score_triples<double>(t, d_h.as<int32_t>(), d_t.as<int32_t>(), d_r.as<int32_t>(), m, d_out.as<double>());
        else run_score_triples<float>(t, d_h.as<int32_t>(), d_t.as<int32_t>(), d_r.as<int32_t>(), m, d_out.as<double>());
        HIPCHK(hipMemcpyAsync(energy + c0, d_out.p, (size_t)m * 8, hipMemcpyDeviceToHost, t.stream));
        HIPCHK(hipStreamSynchronize(t.stream));
    }
}

void predict_topk(const EvalTables& t, const PredictQuery& q, int32_t* ids, double* energy, int32_t* found,
                  const PredictHooks* hooks) {
    const int ne = t.ne, n = t.n, k = q.k;
    if (q.nq < 1) throw std::invalid_argument("no queries");
    if (q.nq > INT32_MAX) throw std::invalid_argument("too many queries in one call");
    if (k < 1 || k > kPredictMaxK) throw std::invalid_argument("k must be in 1.." + std::to_string(kPredictMaxK));
    for (int64_t x = 0; x < q.nq; ++x) {
        if (q.side[x] != 0 && q.side[x] != 1) throw std::invalid_argument("query side must be 0 (head) or 1 (tail)");
        if (q.ent[x] < 0 || q.ent[x] >= ne || q.rel[x] < 0 || q.rel[x] >= t.nr)
            throw std::invalid_argument("query " + std::to_string(x) + " has an id out of range");
    }
    for (int64_t x = 0; x < q.nfilter; ++x)
        if (q.fh[x] < 0 || q.fh[x] >= ne || q.ft[x] < 0 || q.ft[x] >= ne || q.fr[x] < 0 || q.fr[x] >= t.nr)
            throw std::invalid_argument("filter triple out of range");
    const int64_t nq = q.nq;

    // queries grouped by relation (stable: the caller's order within one)
    std::vector<int64_t> order((size_t)nq);
    std::iota(order.begin(), order.end(), (int64_t)0);
    std::stable_sort(order.begin(), order.end(), [&](int64_t x, int64_t y) { return q.rel[x] < q.rel[y]; });
    const KnownCandidates kc =
        build_known_candidates(q.ent, q.rel, q.side, nq, q.fh, q.ft, q.fr, q.nfilter, t.nr);
    std::vector<int32_t> se((size_t)nq), ss((size_t)nq), sg((size_t)nq), srel((size_t)nq);
    for (int64_t x = 0; x < nq; ++x) {
        se[x] = q.ent[order[x]];
        ss[x] = q.side[order[x]];
        sg[x] = kc.group[(size_t)order[x]];
        srel[x] = q.rel[order[x]];
    }

    // rows of the key buffer: <= 1 GiB (KB2E_PREDICT_CHUNK_ROWS caps it further: tests)
    int64_t rows = std::max<int64_t>(1, ((int64_t)1 << 30) / ((int64_t)ne * 8));
    if (const char* cr = getenv("KB2E_PREDICT_CHUNK_ROWS")) {
        const long v = atol(cr);
        if (v >= 1) rows = std::min<int64_t>(rows, v);
    }
    rows = std::min(rows, nq);
    // n <= 1200 fits; KB2E_EVAL_ROWS_L2=1 forces the L2 form as in the evaluator
    const bool rows_lds = (size_t)(kQ + 1) * n * 8 <= kLdsMax && !env_on("KB2E_EVAL_ROWS_L2");
    const size_t score_lds = rows_lds ? (size_t)(kQ + 1) * n * 8 : 0;
    // the key row in LDS while that still leaves four workgroups a CU (|E| <= 3,400);
    // a larger row is re-read from L2 -- at FB15k's 120 KB one workgroup a CU made the
    // selection 3.2x slower than the L2 form.  KB2E_PREDICT_KEYS_L2=1
    // forces the L2 form, =0 the LDS form whenever the row fits the 160 KB (tests)
    const size_t staged = kSelScratchBytes + (size_t)ne * 8;
    const char* kl2 = getenv("KB2E_PREDICT_KEYS_L2");
    bool keys_lds = staged <= kLdsMax / 4;
    if (kl2 && kl2[0] == '1') keys_lds = false;
    if (kl2 && kl2[0] == '0') keys_lds = staged <= kLdsMax;
    const size_t select_lds = kSelScratchBytes + (keys_lds ? (size_t)ne * 8 : 0);
    if (rows_lds) allow_lds(predict_score_kernel<true>, score_lds);
    if (keys_lds) allow_lds(predict_select_kernel<true>, select_lds);

    DevBuf d_e, d_s, d_g, d_off, d_kid, d_keys, d_PT, d_relv, d_ids, d_en, d_found;
    d_e.alloc((size_t)nq * 4);
    d_s.alloc((size_t)nq * 4);
    d_g.alloc((size_t)nq * 4);
    d_off.alloc(kc.off.size() * 8);
    d_kid.alloc(kc.ids.size() * 4);
    HIPCHK(hipMemcpyAsync(d_e.p, se.data(), (size_t)nq * 4, hipMemcpyHostToDevice, t.stream));
    HIPCHK(hipMemcpyAsync(d_s.p, ss.data(), (size_t)nq * 4, hipMemcpyHostToDevice, t.stream));
    HIPCHK(hipMemcpyAsync(d_g.p, sg.data(), (size_t)nq * 4, hipMemcpyHostToDevice, t.stream));
    HIPCHK(hipMemcpyAsync(d_off.p, kc.off.data(), kc.off.size() * 8, hipMemcpyHostToDevice, t.stream));
    if (!kc.ids.empty())
        HIPCHK(hipMemcpyAsync(d_kid.p, kc.ids.data(), kc.ids.size() * 4, hipMemcpyHostToDevice, t.stream));
    d_keys.alloc((size_t)rows * ne * 8);
    d_PT.alloc((size_t)n * ne * 8);
    d_relv.alloc((size_t)n * 8);
    d_ids.alloc((size_t)rows * k * 4);
    d_en.alloc((size_t)rows * k * 8);
    d_found.alloc((size_t)rows * 4);
    std::vector<int32_t> hids((size_t)rows * k), hfound((size_t)rows);
    std::vector<double> hen((size_t)rows * k);

    int cur_rel = -1;  // the relation d_PT holds (a relation's queries may span two chunks)
    for (int64_t c0 = 0; c0 < nq; c0 += rows) {
        const int64_t c1 = std::min(nq, c0 + rows);
        {
            Span sp(hooks, "predict_score");
            for (int64_t a0 = c0; a0 < c1;) {
                const int r = srel[a0];
                int64_t a1 = a0;
                while (a1 < c1 && srel[a1] == r) ++a1;
                if (r != cur_rel) {
                    project_any(t, r, d_PT.as<double>(), d_relv.as<double>());
                    cur_rel = r;
                }
                ScoreArgs sa{d_PT.as<double>(), d_relv.as<double>(), n, ne, t.l1, d_e.as<int32_t>() + a0,
                             d_s.as<int32_t>() + a0, (int32_t)(a1 - a0), d_keys.as<uint64_t>() + (a0 - c0) * ne};
                dim3 grid((ne + 255) / 256, (unsigned)((a1 - a0 + kQ - 1) / kQ));
                if (rows_lds) predict_score_kernel<true><<<grid, 256, score_lds, t.stream>>>(sa);
                else predict_score_kernel<false><<<grid, 256, 0, t.stream>>>(sa);
                HIPCHK(hipGetLastError());
                a0 = a1;
            }
            sp.end();
        }
        const unsigned m = (unsigned)(c1 - c0);
        if (!kc.ids.empty()) {
            Span sp(hooks, "predict_mask");
            MaskArgs ma{d_keys.as<uint64_t>(), ne, d_g.as<int32_t>() + c0, d_off.as<int64_t>(), d_kid.as<int32_t>()};
            predict_mask_kernel<<<m, 256, 0, t.stream>>>(ma);
            HIPCHK(hipGetLastError());
            sp.end();
        }
        {
            Span sp(hooks, "predict_select");
            SelectArgs sa{d_keys.as<uint64_t>(), ne, k, d_ids.as<int32_t>(), d_en.as<double>(), d_found.as<int32_t>()};
            if (keys_lds) predict_select_kernel<true><<<m, kSelThreads, select_lds, t.stream>>>(sa);
            else predict_select_kernel<false><<<m, kSelThreads, select_lds, t.stream>>>(sa);
            HIPCHK(hipGetLastError());
            sp.end();
        }
        HIPCHK(hipMemcpyAsync(hids.data(), d_ids.p, (size_t)m * k * 4, hipMemcpyDeviceToHost, t.stream));
        HIPCHK(hipMemcpyAsync(hen.data(), d_en.p, (size_t)m * k * 8, hipMemcpyDeviceToHost, t.stream));
        HIPCHK(hipMemcpyAsync(hfound.data(), d_found.p, (size_t)m * 4, hipMemcpyDeviceToHost, t.stream));
        HIPCHK(hipStreamSynchronize(t.stream));
        for (int64_t x = c0; x < c1; ++x) {  // back to the caller's order
            const int64_t o = order[x];
            std::copy_n(hids.data() + (x - c0) * k, k, ids + o * k);
            std::copy_n(hen.data() + (x - c0) * k, k, energy + o * k);
            found[o] = hfound[x - c0];
        }
    }
}

// ------------------------------------------------------------ relation prediction: host side

namespace {

// The relation batch's projections PT[batch][n][|U|] stay under this: a choice
// (comfortably inside the card's memory beside the 1 GiB of keys, and large
// enough that FB15k's 1,345 relations at n = 50 take 16 batches), not the result of a sweep.
constexpr int64_t kRelPTCapBytes = (int64_t)512 << 20;
constexpr int64_t kRelMaxBatch = 32768;  // grid.y of the projection kernel

long env_long(const char* name) {
    const char* v = getenv(name);
    return v ? atol(v) : 0;
}

// predict_relations (ids / energy / found) when q.truth is null, else rank_relations (ranks).
template <typename T>
void run_relations(const EvalTables& t, const RelationQuery& q, int32_t* ids, double* energy, int32_t* found,
                   int64_t* ranks, const PredictHooks* hooks) {
    const int ne = t.ne, nr = t.nr, n = t.n, k = q.k;
    const bool ranking = q.truth != nullptr;
    if (q.nq < 1) throw std::invalid_argument("no queries");
    if (q.nq > INT32_MAX) throw std::invalid_argument("too many queries in one call");
    if (!ranking && (k < 1 || k > kPredictMaxK))
        throw std::invalid_argument("k must be in 1.." + std::to_string(kPredictMaxK));
    for (int64_t x = 0; x < q.nq; ++x)
        if (q.heads[x] < 0 || q.heads[x] >= ne || q.tails[x] < 0 || q.tails[x] >= ne ||
            (ranking && (q.truth[x] < 0 || q.truth[x] >= nr)))
            throw std::invalid_argument("query " + std::to_string(x) + " has an id out of range");
    for (int64_t x = 0; x < q.nfilter; ++x)
        if (q.fh[x] < 0 || q.fh[x] >= ne || q.ft[x] < 0 || q.ft[x] >= ne || q.fr[x] < 0 || q.fr[x] >= nr)
            throw std::invalid_argument("filter triple out of range");
    const int64_t nq = q.nq;
    const KnownCandidates kc = build_known_relations(q.heads, q.tails, nq, q.fh, q.ft, q.fr, q.nfilter, ne);

    // rows of the key buffer: predict_topk's rule with the row length |R|
    int64_t rows = std::max<int64_t>(1, ((int64_t)1 << 30) / ((int64_t)nr * 8));
    if (const long v = env_long("KB2E_PREDICT_CHUNK_ROWS"); v >= 1) rows = std::min<int64_t>(rows, v);
    rows = std::min(rows, nq);
    const size_t staged = kSelScratchBytes + (size_t)nr * 8;
    const char* kl2 = getenv("KB2E_PREDICT_KEYS_L2");
    bool keys_lds = staged <= kLdsMax / 4;
    if (kl2 && kl2[0] == '1') keys_lds = false;
    if (kl2 && kl2[0] == '0') keys_lds = staged <= kLdsMax;
    const size_t select_lds = kSelScratchBytes + (keys_lds ? (size_t)nr * 8 : 0);
    if (!ranking && keys_lds) allow_lds(predict_select_kernel<true>, select_lds);

    const bool transr = t.model == 2;
    DevBuf d_h, d_t, d_g, d_off, d_kid, d_truth, d_keys, d_RT, d_WT, d_PT, d_ents, d_ids, d_en, d_found, d_ranks;
    d_g.alloc((size_t)nq * 4);
    d_off.alloc(kc.off.size() * 8);
    d_kid.alloc(kc.ids.size() * 4);
    HIPCHK(hipMemcpyAsync(d_g.p, kc.group.data(), (size_t)nq * 4, hipMemcpyHostToDevice, t.stream));
    HIPCHK(hipMemcpyAsync(d_off.p, kc.off.data(), kc.off.size() * 8, hipMemcpyHostToDevice, t.stream));
    if (!kc.ids.empty())
        HIPCHK(hipMemcpyAsync(d_kid.p, kc.ids.data(), kc.ids.size() * 4, hipMemcpyHostToDevice, t.stream));
    if (ranking) {
        d_truth.alloc((size_t)nq * 4);
        HIPCHK(hipMemcpyAsync(d_truth.p, q.truth, (size_t)nq * 4, hipMemcpyHostToDevice, t.stream));
        d_ranks.alloc((size_t)rows * 2 * 8);
    } else {
        d_ids.alloc((size_t)rows * k * 4);
        d_en.alloc((size_t)rows * k * 8);
        d_found.alloc((size_t)rows * 4);
    }
    d_keys.alloc((size_t)rows * nr * 8);

    // TransE / TransH: the pairs as entity ids, the relation tables transposed once
    const size_t direct_lds = (size_t)2 * kQ * n * 8;
    // TransR: the pairs of a chunk as indices into its entity list (<= 2 * rows, <= |E|)
    const int64_t umax = std::min<int64_t>(2 * rows, ne);
    int64_t batch = 1;
    const bool transpose = !env_on("KB2E_RELPRED_KEYS_STRIDED");
    if (!transr) {
        d_h.alloc((size_t)nq * 4);
        d_t.alloc((size_t)nq * 4);
        HIPCHK(hipMemcpyAsync(d_h.p, q.heads, (size_t)nq * 4, hipMemcpyHostToDevice, t.stream));
        HIPCHK(hipMemcpyAsync(d_t.p, q.tails, (size_t)nq * 4, hipMemcpyHostToDevice, t.stream));
        d_RT.alloc((size_t)n * nr * 8);
        const unsigned tb = (unsigned)(((int64_t)n * nr + 255) / 256);
        Span sp(hooks, "relpred_score");
        relpred_transpose_kernel<T><<<tb, 256, 0, t.stream>>>((const T*)t.rel, n, t.ld, nr, d_RT.as<double>());
        HIPCHK(hipGetLastError());
        if (t.model == 1) {
            d_WT.alloc((size_t)n * nr * 8);
            relpred_transpose_kernel<T><<<tb, 256, 0, t.stream>>>((const T*)t.w, n, t.ld, nr, d_WT.as<double>());
            HIPCHK(hipGetLastError());
            allow_lds(relpred_direct_kernel<T, true>, direct_lds);
        } else {
            allow_lds(relpred_direct_kernel<T, false>, direct_lds);
        }
        sp.end();
    } else {
        d_h.alloc((size_t)rows * 4);  // head / tail indices of the chunk
        d_t.alloc((size_t)rows * 4);
        d_ents.alloc((size_t)umax * 4);
        const int64_t per = (int64_t)n * umax * 8;
        batch = std::min<int64_t>(std::min<int64_t>(nr, kRelMaxBatch), std::max<int64_t>(1, kRelPTCapBytes / per));
        if (const long v = env_long("KB2E_RELPRED_REL_BATCH"); v >= 1) batch = std::min<int64_t>(batch, v);
        d_PT.alloc((size_t)(batch * per));
    }

    for (int64_t c0 = 0; c0 < nq; c0 += rows) {
        const int64_t c1 = std::min(nq, c0 + rows);
        const int32_t m = (int32_t)(c1 - c0);
        PairEntities pe;  // (lives until the chunk's synchronise: its copies are queued)
        if (!transr) {
            Span sp(hooks, "relpred_score");
            RelDirectArgs<T> da{n, t.ld, nr, t.l1, (const T*)t.ent, d_RT.as<double>(), d_WT.as<double>(),
                                d_h.as<int32_t>() + c0, d_t.as<int32_t>() + c0, m, d_keys.as<uint64_t>()};
            dim3 grid((nr + 255) / 256, (unsigned)((m + kQ - 1) / kQ));
            if (t.model == 1) relpred_direct_kernel<T, true><<<grid, 256, direct_lds, t.stream>>>(da);
            else relpred_direct_kernel<T, false><<<grid, 256, direct_lds, t.stream>>>(da);
            HIPCHK(hipGetLastError());
            sp.end();
        } else {
            pe = build_pair_entities(q.heads + c0, q.tails + c0, m);
            const int32_t nu = (int32_t)pe.ents.size();
            HIPCHK(hipMemcpyAsync(d_ents.p, pe.ents.data(), (size_t)nu * 4, hipMemcpyHostToDevice, t.stream));
            HIPCHK(hipMemcpyAsync(d_h.p, pe.hi.data(), (size_t)m * 4, hipMemcpyHostToDevice, t.stream));
            HIPCHK(hipMemcpyAsync(d_t.p, pe.ti.data(), (size_t)m * 4, hipMemcpyHostToDevice, t.stream));
            Span sp(hooks, "relpred_score");
            for (int64_t r0 = 0; r0 < nr; r0 += batch) {  // PT is rebuilt per chunk: its entity list differs
                const int32_t nb = (int32_t)std::min<int64_t>(batch, nr - r0);
                RelProjArgs<T> pa{n, t.ld, nu, (int32_t)r0, (const T*)t.ent, (const T*)t.w, d_ents.as<int32_t>(),
                                  d_PT.as<double>()};
                relpred_project_kernel<T><<<dim3((nu + 255) / 256, nb, (n + kProjK - 1) / kProjK), 256, 0, t.stream>>>(pa);
                HIPCHK(hipGetLastError());
                RelPairArgs<T> ra{n, t.ld, nu, nr, t.l1, (int32_t)r0, nb, (const T*)t.rel, d_PT.as<double>(),
                                  d_h.as<int32_t>(), d_t.as<int32_t>(), m, d_keys.as<uint64_t>()};
                dim3 grid((m + kPairQ - 1) / kPairQ, (nb + kPairR - 1) / kPairR);
                if (transpose) relpred_pair_kernel<T, true><<<grid, 256, 0, t.stream>>>(ra);
                else relpred_pair_kernel<T, false><<<grid, 256, 0, t.stream>>>(ra);
                HIPCHK(hipGetLastError());
            }
            sp.end();
        }
        if (ranking) {
            Span sp(hooks, "relpred_rank");
            RelRankArgs ra{d_keys.as<uint64_t>(), nr, d_truth.as<int32_t>() + c0, d_g.as<int32_t>() + c0,
                           d_off.as<int64_t>(), d_kid.as<int32_t>(), d_ranks.as<int64_t>()};
            relpred_rank_kernel<<<(unsigned)m, 256, 0, t.stream>>>(ra);
            HIPCHK(hipGetLastError());
            sp.end();
            HIPCHK(hipMemcpyAsync(ranks + c0 * 2, d_ranks.p, (size_t)m * 2 * 8, hipMemcpyDeviceToHost, t.stream));
        } else {
            if (!kc.ids.empty()) {
                Span sp(hooks, "relpred_mask");
                MaskArgs ma{d_keys.as<uint64_t>(), nr, d_g.as<int32_t>() + c0, d_off.as<int64_t>(), d_kid.as<int32_t>()};
                predict_mask_kernel<<<(unsigned)m, 256, 0, t.stream>>>(ma);
                HIPCHK(hipGetLastError());
                sp.end();
            }
            Span sp(hooks, "relpred_select");
            SelectArgs sa{d_keys.as<uint64_t>(), nr, k, d_ids.as<int32_t>(), d_en.as<double>(), d_found.as<int32_t>()};
            if (keys_lds) predict_select_kernel<true><<<(unsigned)m, kSelThreads, select_lds, t.stream>>>(sa);
            else predict_select_kernel<false><<<(unsigned)m, kSelThreads, select_lds, t.stream>>>(sa);
            HIPCHK(hipGetLastError());
            sp.end();
            HIPCHK(hipMemcpyAsync(ids + c0 * k, d_ids.p, (size_t)m * k * 4, hipMemcpyDeviceToHost, t.stream));
            HIPCHK(hipMemcpyAsync(energy + c0 * k, d_en.p, (size_t)m * k * 8, hipMemcpyDeviceToHost, t.stream));
            HIPCHK(hipMemcpyAsync(found + c0, d_found.p, (size_t)m * 4, hipMemcpyDeviceToHost, t.stream));
        }
        HIPCHK(hipStreamSynchronize(t.stream));
    }
}

}  // namespace

void predict_relations(const EvalTables& t, const RelationQuery& q, int32_t* ids, double* energy, int32_t* found,
                       const PredictHooks* hooks) {
    if (q.truth) throw std::invalid_argument("predict_relations takes no true relations");
    if (t.f64) run_relations<double>(t, q, ids, energy, found, nullptr, hooks);
    else run_relations<float>(t, q, ids, energy, found, nullptr, hooks);
}

void rank_relations(const EvalTables& t, const RelationQuery& q, int64_t* ranks, const PredictHooks* hooks) {
    if (!q.truth) throw std::invalid_argument("rank_relations needs the true relations");
    if (t.f64) run_relations<double>(t, q, nullptr, nullptr, nullptr, ranks, hooks);
    else run_relations<float>(t, q, nullptr, nullptr, nullptr, ranks, hooks);
}

// ------------------------------------------------------------ conjunctive queries
//
// Query q owns 1..64 constraint rows, each one of predict_topk's one-sided
// patterns.  Every row is scored by predict_score_kernel into a row buffer
// (relation by relation, one projection per distinct relation of the chunk);
// joint_combine_kernel adds a query's rows in the caller's order into the
// query's key row, and the mask, the selection and the rank count run on those
// key rows unchanged -- the keys are sums of energies >= +0, so still >= +0.

namespace {

struct CombineArgs {
    const uint64_t* rows;   // [chunk rows][ne] energies as bit patterns, in scoring (relation) order
    const int32_t* rowidx;  // [chunk rows] caller row -> its row of `rows`
    const int32_t* qoff;    // [chunk queries + 1] caller rows of each query
    int32_t ne, xblocks;
    uint64_t* keys;  // [chunk queries][ne]
};

// One thread per (query, candidate): workgroup b takes candidates
// (b % xblocks) * 256 .. of query b / xblocks (a flat grid: the queries of a
// chunk may outnumber grid.y).  The query's row list sits in LDS, so every row
// base is workgroup-uniform; the lanes run along the candidates (512-byte
// segments per wave and row).  The loads of four rows are issued together; the
// additions stay serial in the caller's order, one rounding each.
__global__ __launch_bounds__(256) void joint_combine_kernel(CombineArgs a) {
    __shared__ int32_t ridx[kJointMaxConstraints];
    const int q = blockIdx.x / a.xblocks;
    const int c0 = a.qoff[q], m = a.qoff[q + 1] - c0;
    if ((int)threadIdx.x < m) ridx[threadIdx.x] = a.rowidx[c0 + threadIdx.x];
    __syncthreads();
    const int x = (blockIdx.x % a.xblocks) * blockDim.x + threadIdx.x;
    if (x >= a.ne) return;
    const uint64_t* col = a.rows + x;
    double s = __longlong_as_double((long long)col[(int64_t)ridx[0] * a.ne]);
    int j = 1;
    for (; j + 4 <= m; j += 4) {
        double v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = __longlong_as_double((long long)col[(int64_t)ridx[j + u] * a.ne]);
#pragma unroll
        for (int u = 0; u < 4; ++u) s += v[u];
    }
    for (; j < m; ++j) s += __longlong_as_double((long long)col[(int64_t)ridx[j] * a.ne]);
    a.keys[(int64_t)q * a.ne + x] = (uint64_t)__double_as_longlong(s);
}

constexpr int64_t kScoreMaxRows = (int64_t)65535 * kQ;  // grid.y of one score launch

// predict_joint (ids / energy / found) when q.truth is null, else rank_joint (ranks).
void run_joint(const EvalTables& t, const JointQuery& q, int32_t* ids, double* energy, int32_t* found, int64_t* ranks,
               JointStats* stats, const PredictHooks* hooks) {
    const int ne = t.ne, n = t.n, k = q.k;
    const bool ranking = q.truth != nullptr;
    if (q.nq < 1) throw std::invalid_argument("no queries");
    if (q.nq > INT32_MAX) throw std::invalid_argument("too many queries in one call");
    if (!ranking && (k < 1 || k > kPredictMaxK))
        throw std::invalid_argument("k must be in 1.." + std::to_string(kPredictMaxK));
    if (const char* why = joint_check_offsets(q.offsets, q.nq)) throw std::invalid_argument(why);
    const int64_t nq = q.nq, nrows = q.offsets[nq];
    for (int64_t c = 0; c < nrows; ++c) {
        if (q.side[c] != 0 && q.side[c] != 1) throw std::invalid_argument("constraint side must be 0 (head) or 1 (tail)");
        if (q.ent[c] < 0 || q.ent[c] >= ne || q.rel[c] < 0 || q.rel[c] >= t.nr)
            throw std::invalid_argument("constraint " + std::to_string(c) + " has an id out of range");
    }
    if (ranking)
        for (int64_t x = 0; x < nq; ++x)
            if (q.truth[x] < 0 || q.truth[x] >= ne)
                throw std::invalid_argument("query " + std::to_string(x) + " has a truth out of range");
    for (int64_t x = 0; x < q.nfilter; ++x)
        if (q.fh[x] < 0 || q.fh[x] >= ne || q.ft[x] < 0 || q.ft[x] >= ne || q.fr[x] < 0 || q.fr[x] >= t.nr)
            throw std::invalid_argument("filter triple out of range");

    // excluded per query: the candidates known for every one of its constraints
    const JointKnown jk = joint_intersect_known(
        q.offsets, nq, build_known_candidates(q.ent, q.rel, q.side, nrows, q.fh, q.ft, q.fr, q.nfilter, t.nr));

    // scored rows held at a time: <= 1 GiB (KB2E_JOINT_CHUNK_ROWS lowers that: tests), but
    // never less than the largest query; the key rows, one per query, come on top
    int64_t cap = std::max<int64_t>(1, ((int64_t)1 << 30) / ((int64_t)ne * 8));
    if (const long v = env_long("KB2E_JOINT_CHUNK_ROWS"); v >= 1) cap = std::min<int64_t>(cap, v);
    const std::vector<JointChunk> chunks = joint_plan_chunks(q.offsets, nq, cap);
    int64_t maxr = 0, maxq = 0;
    for (const JointChunk& ch : chunks) {
        maxr = std::max(maxr, q.offsets[ch.q1] - q.offsets[ch.q0]);
        maxq = std::max(maxq, ch.q1 - ch.q0);
    }
    // the score and selection forms: predict_topk's rules
    const bool rows_lds = (size_t)(kQ + 1) * n * 8 <= kLdsMax && !env_on("KB2E_EVAL_ROWS_L2");
    const size_t score_lds = rows_lds ? (size_t)(kQ + 1) * n * 8 : 0;
    const size_t staged = kSelScratchBytes + (size_t)ne * 8;
    const char* kl2 = getenv("KB2E_PREDICT_KEYS_L2");
    bool keys_lds = staged <= kLdsMax / 4;
    if (kl2 && kl2[0] == '1') keys_lds = false;
    if (kl2 && kl2[0] == '0') keys_lds = staged <= kLdsMax;
    const size_t select_lds = kSelScratchBytes + (keys_lds ? (size_t)ne * 8 : 0);
    if (rows_lds) allow_lds(predict_score_kernel<true>, score_lds);
    if (!ranking && keys_lds) allow_lds(predict_select_kernel<true>, select_lds);

    std::vector<int32_t> group((size_t)nq);  // one list per query
    std::iota(group.begin(), group.end(), 0);
    DevBuf d_e, d_s, d_ridx, d_qoff, d_g, d_off, d_kid, d_truth, d_rows, d_keys, d_PT, d_relv, d_ids, d_en, d_found,
        d_ranks;
    d_g.alloc((size_t)nq * 4);
    d_off.alloc(jk.off.size() * 8);
    d_kid.alloc(jk.ids.size() * 4);
    HIPCHK(hipMemcpyAsync(d_g.p, group.data(), (size_t)nq * 4, hipMemcpyHostToDevice, t.stream));
    HIPCHK(hipMemcpyAsync(d_off.p, jk.off.data(), jk.off.size() * 8, hipMemcpyHostToDevice, t.stream));
    if (!jk.ids.empty())
        HIPCHK(hipMemcpyAsync(d_kid.p, jk.ids.data(), jk.ids.size() * 4, hipMemcpyHostToDevice, t.stream));
    if (ranking) {
        d_truth.alloc((size_t)nq * 4);
        HIPCHK(hipMemcpyAsync(d_truth.p, q.truth, (size_t)nq * 4, hipMemcpyHostToDevice, t.stream));
        d_ranks.alloc((size_t)maxq * 2 * 8);
    } else {
        d_ids.alloc((size_t)maxq * k * 4);
        d_en.alloc((size_t)maxq * k * 8);
        d_found.alloc((size_t)maxq * 4);
    }
    d_e.alloc((size_t)maxr * 4);
    d_s.alloc((size_t)maxr * 4);
    d_ridx.alloc((size_t)maxr * 4);
    d_qoff.alloc((size_t)(maxq + 1) * 4);
    d_rows.alloc((size_t)maxr * ne * 8);
    d_keys.alloc((size_t)maxq * ne * 8);
    d_PT.alloc((size_t)n * ne * 8);
    d_relv.alloc((size_t)n * 8);

    // (the chunk's host arrays live until its synchronise: their copies are queued)
    std::vector<int32_t> order, se, ss, srel, ridx, qoff;
    const int32_t xblocks = (ne + 255) / 256;
    int cur_rel = -1;  // the relation d_PT holds (kept across chunks)
    for (const JointChunk& ch : chunks) {
        const int64_t r0 = q.offsets[ch.q0], m = q.offsets[ch.q1] - r0, mq = ch.q1 - ch.q0;
        // the chunk's rows grouped by relation (stable: the caller's order within one)
        order.resize((size_t)m);
        std::iota(order.begin(), order.end(), 0);
        std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return q.rel[r0 + x] < q.rel[r0 + y]; });
        se.resize((size_t)m), ss.resize((size_t)m), srel.resize((size_t)m), ridx.resize((size_t)m);
        for (int64_t p = 0; p < m; ++p) {
            const int64_t c = r0 + order[(size_t)p];
            se[(size_t)p] = q.ent[c];
            ss[(size_t)p] = q.side[c];
            srel[(size_t)p] = q.rel[c];
            ridx[(size_t)order[(size_t)p]] = (int32_t)p;
        }
        qoff.resize((size_t)mq + 1);
        for (int64_t x = 0; x <= mq; ++x) qoff[(size_t)x] = (int32_t)(q.offsets[ch.q0 + x] - r0);
        HIPCHK(hipMemcpyAsync(d_e.p, se.data(), (size_t)m * 4, hipMemcpyHostToDevice, t.stream));
        HIPCHK(hipMemcpyAsync(d_s.p, ss.data(), (size_t)m * 4, hipMemcpyHostToDevice, t.stream));
        HIPCHK(hipMemcpyAsync(d_ridx.p, ridx.data(), (size_t)m * 4, hipMemcpyHostToDevice, t.stream));
        HIPCHK(hipMemcpyAsync(d_qoff.p, qoff.data(), (size_t)(mq + 1) * 4, hipMemcpyHostToDevice, t.stream));
        {
            Span sp(hooks, "joint_score");
            for (int64_t a0 = 0; a0 < m;) {
                const int r = srel[(size_t)a0];
                int64_t a1 = a0;
                while (a1 < m && srel[(size_t)a1] == r && a1 - a0 < kScoreMaxRows) ++a1;
                if (r != cur_rel) {
                    project_any(t, r, d_PT.as<double>(), d_relv.as<double>());
                    cur_rel = r;
                    if (stats) ++stats->projections;
                }
                ScoreArgs sa{d_PT.as<double>(), d_relv.as<double>(), n, ne, t.l1, d_e.as<int32_t>() + a0,
                             d_s.as<int32_t>() + a0, (int32_t)(a1 - a0), d_rows.as<uint64_t>() + a0 * ne};
                dim3 grid((unsigned)xblocks, (unsigned)((a1 - a0 + kQ - 1) / kQ));
                if (rows_lds) predict_score_kernel<true><<<grid, 256, score_lds, t.stream>>>(sa);
                else predict_score_kernel<false><<<grid, 256, 0, t.stream>>>(sa);
                HIPCHK(hipGetLastError());
                a0 = a1;
            }
            sp.end();
        }
        {
            Span sp(hooks, "joint_combine");
            CombineArgs ca{d_rows.as<uint64_t>(), d_ridx.as<int32_t>(), d_qoff.as<int32_t>(), ne, xblocks,
                           d_keys.as<uint64_t>()};
            joint_combine_kernel<<<(unsigned)(mq * xblocks), 256, 0, t.stream>>>(ca);
            HIPCHK(hipGetLastError());
            sp.end();
        }
        if (ranking) {
            // relpred_rank_kernel's count with the row length |E|: the truth's key is read from
            // the unmasked row, the query's excluded candidates other than the truth are left out
            Span sp(hooks, "joint_rank");
            RelRankArgs ra{d_keys.as<uint64_t>(), ne, d_truth.as<int32_t>() + ch.q0, d_g.as<int32_t>() + ch.q0,
                           d_off.as<int64_t>(), d_kid.as<int32_t>(), d_ranks.as<int64_t>()};
            relpred_rank_kernel<<<(unsigned)mq, 256, 0, t.stream>>>(ra);
            HIPCHK(hipGetLastError());
            sp.end();
            HIPCHK(hipMemcpyAsync(ranks + ch.q0 * 2, d_ranks.p, (size_t)mq * 2 * 8, hipMemcpyDeviceToHost, t.stream));
        } else {
            if (!jk.ids.empty()) {
                Span sp(hooks, "joint_mask");
                MaskArgs ma{d_keys.as<uint64_t>(), ne, d_g.as<int32_t>() + ch.q0, d_off.as<int64_t>(), d_kid.as<int32_t>()};
                predict_mask_kernel<<<(unsigned)mq, 256, 0, t.stream>>>(ma);
                HIPCHK(hipGetLastError());
                sp.end();
            }
            Span sp(hooks, "joint_select");
            SelectArgs sa{d_keys.as<uint64_t>(), ne, k, d_ids.as<int32_t>(), d_en.as<double>(), d_found.as<int32_t>()};
            if (keys_lds) predict_select_kernel<true><<<(unsigned)mq, kSelThreads, select_lds, t.stream>>>(sa);
            else predict_select_kernel<false><<<(unsigned)mq, kSelThreads, select_lds, t.stream>>>(sa);
            HIPCHK(hipGetLastError());
            sp.end();
            HIPCHK(hipMemcpyAsync(ids + ch.q0 * k, d_ids.p, (size_t)mq * k * 4, hipMemcpyDeviceToHost, t.stream));
            HIPCHK(hipMemcpyAsync(energy + ch.q0 * k, d_en.p, (size_t)mq * k * 8, hipMemcpyDeviceToHost, t.stream));
            HIPCHK(hipMemcpyAsync(found + ch.q0, d_found.p, (size_t)mq * 4, hipMemcpyDeviceToHost, t.stream));
        }
        HIPCHK(hipStreamSynchronize(t.stream));
        if (stats) {
            ++stats->chunks;
            stats->rows += m;
        }
    }
}

}  // namespace

void predict_joint(const EvalTables& t, const JointQuery& q, int32_t* ids, double* energy, int32_t* found,
                   JointStats* stats, const PredictHooks* hooks) {
    if (q.truth) throw std::invalid_argument("predict_joint takes no true entities");
    run_joint(t, q, ids, energy, found, nullptr, stats, hooks);
}

void rank_joint(const EvalTables& t, const JointQuery& q, int64_t* ranks, JointStats* stats, const PredictHooks* hooks) {
    if (!q.truth) throw std::invalid_argument("rank_joint needs the true entities");
    run_joint(t, q, nullptr, nullptr, nullptr, ranks, stats, hooks);
}

// ------------------------------------------------------------ path queries
//
// Query q walks 1..8 hops from its anchor.  c_1[x] is the one-sided score row of
// the anchor (predict_score_kernel, unchanged); hop i >= 2 is the min-plus step
// c_i[y] = min over the frontier p of (c_{i-1}[p] + e_i(p, y)), which
// path_hop_kernel computes without writing the |frontier| x |E| energies down.
// The frontier is the whole previous key row (beam = 0) or its `beam` smallest
// (cost, id) pairs, picked by predict_select_kernel on the unmasked row.  The
// rows of the queries that end at a level are masked (the answers the filter's
// paths already state, path_host.hpp), selected or ranked exactly as the joint
// rows are.

namespace {

struct HopArgs {
    const double* PT;    // [n][ne]
    const double* relv;  // [n]
    int32_t n, ne, l1, no_loops, eblocks;
    int32_t stride;          // of fid / fcost rows: the beam, or ne for the identity frontier
    const int32_t* slot;     // [slots] the chunk row of each query of this launch
    const int32_t* sside;    // [slots] the hop's side: 1 walks head -> tail
    const int32_t* fid;      // [rows][stride] frontier ids, or null: the identity list 0 .. ne - 1
    const uint64_t* fcost;   // [rows][stride] their cumulative energies as bit patterns (~0: no path)
    const int32_t* fcount;   // [rows] frontier entries, or null: ne
    uint64_t* keys;          // [rows][ne] out: the bit pattern of the minimum (~0: no path)
    int32_t* pred;           // [rows][ne] out: the frontier entity that gives it (-1: none)
};

// A flat grid: workgroup b takes targets (b % eblocks) * 256 .. of the launch's
// query b / eblocks.  One thread per target y walks the query's frontier in
// tiles of kQ rows: kQ serial FP64 sums in predict_score_kernel's operand order
// (the hop energies, the bits of kb2e_score_triples), then per frontier row one
// addition c[p] + e and a compare on (sum bits, predecessor id) -- the smallest
// id wins among equal sums whatever order the frontier is walked in.  Dynamic
// LDS (kRowsInLds): the tile's projected rows [kQ][n], r [n], the tile's costs
// [kQ] and ids [kQ]; otherwise all of them are read from global memory at
// workgroup-uniform addresses.
template <bool kRowsInLds>
__global__ __launch_bounds__(256) void path_hop_kernel(HopArgs a) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double* kr = lds;
    double* rv = kr + kQ * a.n;
    uint64_t* tcost = (uint64_t*)(rv + a.n);
    int32_t* tid = (int32_t*)(tcost + kQ);
    const int s = blockIdx.x / a.eblocks;
    const int row = a.slot[s];
    const bool tail = a.sside[s] != 0;
    const int count = a.fcount ? a.fcount[row] : a.ne;
    const int32_t* fid = a.fid ? a.fid + (int64_t)row * a.stride : nullptr;
    const uint64_t* fcost = a.fcost + (int64_t)row * a.stride;
    const int y = (blockIdx.x % a.eblocks) * blockDim.x + threadIdx.x;
    const int yc = min(y, a.ne - 1);  // (the threads past |E| stay for the barriers and store nothing)
    if constexpr (kRowsInLds)
        for (int k = threadIdx.x; k < a.n; k += blockDim.x) rv[k] = a.relv[k];
    uint64_t best = kMasked;
    int32_t bestp = -1;
    for (int t0 = 0; t0 < count; t0 += kQ) {  // (count is workgroup-uniform)
        const int nt = min(kQ, count - t0);
        if constexpr (kRowsInLds) {
            __syncthreads();  // the last tile has been read
            if ((int)threadIdx.x < kQ) {
                const int q = threadIdx.x;
                const int id = q < nt ? (fid ? fid[t0 + q] : t0 + q) : -1;
                tid[q] = id;
                tcost[q] = id >= 0 ? fcost[t0 + q] : kMasked;
            }
            for (int x = threadIdx.x; x < kQ * a.n; x += blockDim.x) {
                const int q = x / a.n, k = x % a.n;
                if (q < nt) {
                    const int id = fid ? fid[t0 + q] : t0 + q;
                    kr[x] = a.PT[(int64_t)k * a.ne + max(id, 0)];
                }
            }
            __syncthreads();
        }
        int pid[kQ];  // (the L2 form's row addresses; the LDS form reads the ids where it needs them)
#pragma unroll
        for (int q = 0; q < kQ; ++q) pid[q] = kRowsInLds ? 0 : (q < nt ? (fid ? fid[t0 + q] : t0 + q) : -1);
        double e[kQ];
#pragma unroll
        for (int q = 0; q < kQ; ++q) e[q] = 0;
        for (int k = 0; k < a.n; ++k) {
            const double* col = a.PT + (int64_t)k * a.ne;
            const double v = col[yc];
            const double r = kRowsInLds ? rv[k] : a.relv[k];
#pragma unroll
            for (int q = 0; q < kQ; ++q) {
                const double p = kRowsInLds ? kr[q * a.n + k] : col[max(pid[q], 0)];
                // (P(y) - P(p)) - r walking head -> tail, (P(p) - P(y)) - r backwards
                const double d = tail ? v - p - r : p - v - r;
                e[q] += a.l1 ? fabs(d) : d * d;
            }
        }
#pragma unroll
        for (int q = 0; q < kQ; ++q) {
            const int p = kRowsInLds ? tid[q] : pid[q];
            const uint64_t cb = kRowsInLds ? tcost[q] : (p >= 0 ? fcost[t0 + q] : kMasked);
            if (cb == kMasked || (a.no_loops && p == y)) continue;
            const double sum = __longlong_as_double((long long)cb) + e[q];
            const uint64_t sb = (uint64_t)__double_as_longlong(sum);
            if (sb < best || (sb == best && p < bestp)) {
                best = sb;
                bestp = p;
            }
        }
    }
    if (y < a.ne) {
        a.keys[(int64_t)row * a.ne + y] = best;
        a.pred[(int64_t)row * a.ne + y] = bestp;
    }
}

struct GatherArgs {
    const int32_t* src;  // [rows][ne]
    int32_t ne, m;
    const int32_t* idx;  // [rows][m]
    int32_t* out;        // [rows][m] = src[row][idx[row][j]], -1 where idx is
};

// One workgroup per row: the predecessors of the selected ids (a frontier's
// back-pointers, the last step of the k answers, a step of the via chain).
__global__ __launch_bounds__(256) void path_gather_kernel(GatherArgs a) {
    const int32_t* src = a.src + (int64_t)blockIdx.x * a.ne;
    const int32_t* idx = a.idx + (int64_t)blockIdx.x * a.m;
    int32_t* out = a.out + (int64_t)blockIdx.x * a.m;
    for (int j = threadIdx.x; j < a.m; j += blockDim.x) {
        const int id = idx[j];
        out[j] = id >= 0 && id < a.ne ? src[id] : -1;
    }
}

// predict_path (ids / energy / found / via) when q.truth is null, else rank_path (ranks).
void run_path(const EvalTables& t, const PathQuery& q, int32_t* ids, double* energy, int32_t* found, int32_t* via,
              int64_t* ranks, PathStats* stats, const PredictHooks* hooks) {
    const int ne = t.ne, n = t.n, k = q.k;
    const bool ranking = q.truth != nullptr;
    if (q.nq < 1) throw std::invalid_argument("no queries");
    if (q.nq > INT32_MAX) throw std::invalid_argument("too many queries in one call");
    if (!ranking && (k < 1 || k > kPredictMaxK))
        throw std::invalid_argument("k must be in 1.." + std::to_string(kPredictMaxK));
    if (q.beam < 0 || q.beam > kPathMaxBeam) throw std::invalid_argument("beam must be in 0..1024");
    if (q.no_loops != 0 && q.no_loops != 1) throw std::invalid_argument("no_loops must be 0 or 1");
    if (const char* why = path_check_offsets(q.offsets, q.nq)) throw std::invalid_argument(why);
    const int64_t nq = q.nq, nhops = q.offsets[nq];
    for (int64_t c = 0; c < nhops; ++c) {
        if (q.side[c] != 0 && q.side[c] != 1) throw std::invalid_argument("hop side must be 0 (backwards) or 1");
        if (q.rel[c] < 0 || q.rel[c] >= t.nr) throw std::invalid_argument("hop " + std::to_string(c) + " has a relation out of range");
    }
    for (int64_t x = 0; x < nq; ++x) {
        if (q.anchors[x] < 0 || q.anchors[x] >= ne)
            throw std::invalid_argument("query " + std::to_string(x) + " has an anchor out of range");
        if (ranking && (q.truth[x] < 0 || q.truth[x] >= ne))
            throw std::invalid_argument("query " + std::to_string(x) + " has a truth out of range");
    }
    for (int64_t x = 0; x < q.nfilter; ++x)
        if (q.fh[x] < 0 || q.fh[x] >= ne || q.ft[x] < 0 || q.ft[x] >= ne || q.fr[x] < 0 || q.fr[x] >= t.nr)
            throw std::invalid_argument("filter triple out of range");

    const bool exact = q.beam == 0, no_loops = q.no_loops != 0, want_via = !ranking && via != nullptr;
    const int32_t B = exact ? 0 : std::min<int32_t>(q.beam, ne);  // (a frontier holds no more than |E|)
    int maxL = 1;
    for (int64_t x = 0; x < nq; ++x) maxL = std::max(maxL, (int)(q.offsets[x + 1] - q.offsets[x]));
    if (want_via) std::fill(via, via + nq * (int64_t)k * (kPathMaxHops - 1), -1);

    // excluded per query: the ends of the filter's own paths
    const PathKnown pk = path_known_answers(q.anchors, q.offsets, q.rel, q.side, nq, no_loops, q.fh, q.ft, q.fr,
                                            q.nfilter, t.nr);

    // the |E|-long rows of a chunk: <= 1 GiB, counted in rows of |E| 4-byte words
    // (KB2E_PATH_CHUNK_ROWS lowers that: tests); the short per-query buffers
    // (frontiers, back-pointers, answers) of a chunk: <= 256 MiB
    int64_t budget = std::max<int64_t>(1, ((int64_t)1 << 30) / ((int64_t)ne * 4));
    if (const long v = env_long("KB2E_PATH_CHUNK_ROWS"); v >= 1) budget = std::min<int64_t>(budget, v);
    const int64_t small = (int64_t)(maxL - 1) * B * 8 + (int64_t)B * 12 + 64 +
                          (ranking ? 16 : (int64_t)k * (12 + 4 * (kPathMaxHops - 1)));
    const std::vector<PathChunk> chunks = path_plan_chunks(q.offsets, nq, exact, budget, ((int64_t)256 << 20) / small);
    int64_t maxq = 0, maxlive2 = 0, maxpred = 0;  // rows of the largest chunk; with >= 2 hops; back-pointer rows
    for (const PathChunk& ch : chunks) {
        int64_t live2 = 0, prows = 0;
        for (int64_t x = ch.q0; x < ch.q1; ++x) {
            const int64_t L = q.offsets[x + 1] - q.offsets[x];
            live2 += L >= 2;
            prows += exact ? L - 1 : (L >= 2);
        }
        maxq = std::max(maxq, ch.q1 - ch.q0);
        maxlive2 = std::max(maxlive2, live2);
        maxpred = std::max(maxpred, prows);
    }

    // the score, hop and selection forms: predict_topk's rules
    const bool l2 = env_on("KB2E_EVAL_ROWS_L2");
    const bool rows_lds = (size_t)(kQ + 1) * n * 8 <= kLdsMax && !l2;
    const size_t score_lds = rows_lds ? (size_t)(kQ + 1) * n * 8 : 0;
    const size_t hop_bytes = (size_t)(kQ + 1) * n * 8 + (size_t)kQ * 12;
    const bool hop_rows_lds = hop_bytes <= kLdsMax && !l2;
    const size_t hop_lds = hop_rows_lds ? hop_bytes : 0;
    const size_t staged = kSelScratchBytes + (size_t)ne * 8;
    const char* kl2 = getenv("KB2E_PREDICT_KEYS_L2");
    bool keys_lds = staged <= kLdsMax / 4;
    if (kl2 && kl2[0] == '1') keys_lds = false;
    if (kl2 && kl2[0] == '0') keys_lds = staged <= kLdsMax;
    const size_t select_lds = kSelScratchBytes + (keys_lds ? (size_t)ne * 8 : 0);
    if (rows_lds) allow_lds(predict_score_kernel<true>, score_lds);
    if (hop_rows_lds && maxL >= 2) allow_lds(path_hop_kernel<true>, hop_lds);
    if (keys_lds) allow_lds(predict_select_kernel<true>, select_lds);

    DevBuf d_anchor, d_side1, d_iota, d_iota64, d_g, d_off, d_kid, d_truth, d_slot, d_sside, d_keys0, d_keys1, d_pred,
        d_fid, d_back, d_fcost, d_fcount, d_ids, d_en, d_found, d_last, d_via, d_ranks, d_PT, d_relv;
    d_anchor.alloc((size_t)maxq * 4);
    d_side1.alloc((size_t)maxq * 4);
    d_g.alloc((size_t)maxq * 4);
    d_off.alloc(pk.off.size() * 8);
    d_kid.alloc(pk.ids.size() * 4);
    HIPCHK(hipMemcpyAsync(d_off.p, pk.off.data(), pk.off.size() * 8, hipMemcpyHostToDevice, t.stream));
    if (!pk.ids.empty())
        HIPCHK(hipMemcpyAsync(d_kid.p, pk.ids.data(), pk.ids.size() * 4, hipMemcpyHostToDevice, t.stream));
    std::vector<int32_t> iota;
    std::vector<int64_t> iota64;
    if (no_loops) {  // hop 1 leaves out x_1 == the anchor: one masked key per row
        iota.resize((size_t)maxq), iota64.resize((size_t)maxq + 1);
        std::iota(iota.begin(), iota.end(), 0);
        std::iota(iota64.begin(), iota64.end(), (int64_t)0);
        d_iota.alloc((size_t)maxq * 4);
        d_iota64.alloc((size_t)(maxq + 1) * 8);
        HIPCHK(hipMemcpyAsync(d_iota.p, iota.data(), (size_t)maxq * 4, hipMemcpyHostToDevice, t.stream));
        HIPCHK(hipMemcpyAsync(d_iota64.p, iota64.data(), (size_t)(maxq + 1) * 8, hipMemcpyHostToDevice, t.stream));
    }
    if (ranking) {
        d_truth.alloc((size_t)maxq * 4);
        d_ranks.alloc((size_t)maxq * 2 * 8);
    } else {
        d_ids.alloc((size_t)maxq * k * 4);
        d_en.alloc((size_t)maxq * k * 8);
        d_found.alloc((size_t)maxq * 4);
    }
    d_keys0.alloc((size_t)maxq * ne * 8);
    if (maxlive2 > 0) {
        d_slot.alloc((size_t)(maxL - 1) * maxlive2 * 4);
        d_sside.alloc((size_t)(maxL - 1) * maxlive2 * 4);
        d_pred.alloc((size_t)maxpred * ne * 4);
        if (exact) {
            d_keys1.alloc((size_t)maxlive2 * ne * 8);
            if (want_via) d_via.alloc((size_t)(maxL - 1) * maxlive2 * k * 4);
        } else {
            d_fid.alloc((size_t)(maxL - 1) * maxlive2 * B * 4);
            d_fcost.alloc((size_t)maxlive2 * B * 8);
            d_fcount.alloc((size_t)maxlive2 * 4);
            if (want_via) {
                d_back.alloc((size_t)(maxL - 1) * maxlive2 * B * 4);
                d_last.alloc((size_t)maxlive2 * k * 4);
            }
        }
    }
    d_PT.alloc((size_t)n * ne * 8);
    d_relv.alloc((size_t)n * 8);

    const int32_t eblocks = (ne + 255) / 256;
    const int64_t fstride = maxlive2 * B;  // of one level in d_fid / d_back
    // (the chunk's host arrays live until its synchronise: their copies are queued)
    std::vector<int32_t> h_anchor, h_side1, h_g, h_truth, hids, hfound, hlast, hvia, hfid, hback;
    std::vector<double> hen;
    std::vector<int64_t> hranks;
    std::vector<PathLevel> levels;
    int cur_rel = -1;  // the relation d_PT holds (kept across levels and chunks)
    auto project_once = [&](int r) {
        if (r == cur_rel) return;
        Span sp(hooks, "path_score");
        project_any(t, r, d_PT.as<double>(), d_relv.as<double>());
        sp.end();
        cur_rel = r;
        if (stats) ++stats->projections;
    };
    auto gather = [&](const int32_t* src, const int32_t* idx, int32_t m, int32_t* out, int64_t rows) {
        path_gather_kernel<<<(unsigned)rows, 256, 0, t.stream>>>(GatherArgs{src, ne, m, idx, out});
        HIPCHK(hipGetLastError());
    };
    for (const PathChunk& ch : chunks) {
        const std::vector<int64_t> order = path_chunk_order(q.offsets, q.rel, q.side, ch.q0, ch.q1);
        const int64_t mq = ch.q1 - ch.q0;
        int64_t live[kPathMaxHops + 2], lvl_off[kPathMaxHops + 2];  // rows with >= i hops; exact: level i's first pred row
        for (int i = 1; i <= kPathMaxHops + 1; ++i) live[i] = path_live(q.offsets, order, i);
        lvl_off[2] = 0;
        for (int i = 3; i <= kPathMaxHops + 1; ++i) lvl_off[i] = lvl_off[i - 1] + (exact ? live[i - 1] : 0);
        h_anchor.resize((size_t)mq), h_side1.resize((size_t)mq), h_g.resize((size_t)mq);
        for (int64_t x = 0; x < mq; ++x) {
            const int64_t o = order[(size_t)x];
            h_anchor[(size_t)x] = q.anchors[o];
            h_side1[(size_t)x] = q.side[q.offsets[o]];
            h_g[(size_t)x] = (int32_t)o;
        }
        HIPCHK(hipMemcpyAsync(d_anchor.p, h_anchor.data(), (size_t)mq * 4, hipMemcpyHostToDevice, t.stream));
        HIPCHK(hipMemcpyAsync(d_side1.p, h_side1.data(), (size_t)mq * 4, hipMemcpyHostToDevice, t.stream));
        HIPCHK(hipMemcpyAsync(d_g.p, h_g.data(), (size_t)mq * 4, hipMemcpyHostToDevice, t.stream));
        if (ranking) {
            h_truth.resize((size_t)mq);
            for (int64_t x = 0; x < mq; ++x) h_truth[(size_t)x] = q.truth[order[(size_t)x]];
            HIPCHK(hipMemcpyAsync(d_truth.p, h_truth.data(), (size_t)mq * 4, hipMemcpyHostToDevice, t.stream));
        }
        levels.clear();
        levels.reserve(kPathMaxHops);  // (no reallocation: the copies of a level's arrays are queued)
        int chunkL = 1;
        while (chunkL < kPathMaxHops && live[chunkL + 1] > 0) ++chunkL;
        for (int i = 1; i <= chunkL; ++i) {
            levels.push_back(path_plan_level(q.offsets, q.rel, q.side, order, i));
            const PathLevel& pl = levels.back();
            const int64_t m = live[i];
            // hop i writes this buffer; the exact form reads the other one as the frontier's costs
            uint64_t* kout = (exact && (i & 1) == 0 ? d_keys1 : d_keys0).as<uint64_t>();
            if (i == 1) {
                // the rows of a (relation, side) are consecutive inside one length class: one launch per such run
                for (int64_t a0 = 0; a0 < m;) {
                    const int r = pl.rel[(size_t)a0];
                    int64_t a1 = a0 + 1;
                    while (a1 < m && pl.rel[(size_t)a1] == r && pl.row[(size_t)a1] == pl.row[(size_t)a1 - 1] + 1 &&
                           a1 - a0 < kScoreMaxRows)
                        ++a1;
                    project_once(r);
                    const int64_t r0 = pl.row[(size_t)a0];
                    Span sp(hooks, "path_score");
                    ScoreArgs sa{d_PT.as<double>(), d_relv.as<double>(), n, ne, t.l1, d_anchor.as<int32_t>() + r0,
                                 d_side1.as<int32_t>() + r0, (int32_t)(a1 - a0), kout + r0 * ne};
                    dim3 grid((unsigned)eblocks, (unsigned)((a1 - a0 + kQ - 1) / kQ));
                    if (rows_lds) predict_score_kernel<true><<<grid, 256, score_lds, t.stream>>>(sa);
                    else predict_score_kernel<false><<<grid, 256, 0, t.stream>>>(sa);
                    HIPCHK(hipGetLastError());
                    sp.end();
                    a0 = a1;
                }
                if (no_loops) {
                    Span sp(hooks, "path_mask");
                    MaskArgs ma{kout, ne, d_iota.as<int32_t>(), d_iota64.as<int64_t>(), d_anchor.as<int32_t>()};
                    predict_mask_kernel<<<(unsigned)mq, 256, 0, t.stream>>>(ma);
                    HIPCHK(hipGetLastError());
                    sp.end();
                }
            } else {
                int32_t* dslot = d_slot.as<int32_t>() + (int64_t)(i - 2) * maxlive2;
                int32_t* dside = d_sside.as<int32_t>() + (int64_t)(i - 2) * maxlive2;
                HIPCHK(hipMemcpyAsync(dslot, pl.row.data(), (size_t)m * 4, hipMemcpyHostToDevice, t.stream));
                HIPCHK(hipMemcpyAsync(dside, pl.side.data(), (size_t)m * 4, hipMemcpyHostToDevice, t.stream));
                for (int64_t a0 = 0; a0 < m;) {
                    const int r = pl.rel[(size_t)a0];
                    int64_t a1 = a0;
                    while (a1 < m && pl.rel[(size_t)a1] == r) ++a1;
                    project_once(r);
                    Span sp(hooks, "path_hop");
                    HopArgs ha{d_PT.as<double>(), d_relv.as<double>(), n, ne, t.l1, no_loops ? 1 : 0, eblocks,
                               exact ? ne : B, dslot + a0, dside + a0,
                               exact ? nullptr : d_fid.as<int32_t>() + (int64_t)(i - 2) * fstride,
                               exact ? ((i & 1) == 0 ? d_keys0 : d_keys1).as<uint64_t>() : d_fcost.as<uint64_t>(),
                               exact ? nullptr : d_fcount.as<int32_t>(), kout,
                               d_pred.as<int32_t>() + lvl_off[i] * ne};
                    const unsigned blocks = (unsigned)((a1 - a0) * eblocks);
                    if (hop_rows_lds) path_hop_kernel<true><<<blocks, 256, hop_lds, t.stream>>>(ha);
                    else path_hop_kernel<false><<<blocks, 256, 0, t.stream>>>(ha);
                    HIPCHK(hipGetLastError());
                    sp.end();
                    a0 = a1;
                }
                if (stats) stats->hops += m;
            }
            const int32_t* pred_i = i >= 2 ? d_pred.as<int32_t>() + lvl_off[i] * ne : nullptr;
            // the queries that end here: rows [live[i + 1], live[i])
            const int64_t f0 = live[i + 1], nf = live[i] - f0;
            if (nf > 0 && ranking) {
                Span sp(hooks, "path_rank");
                RelRankArgs ra{kout + f0 * ne, ne, d_truth.as<int32_t>() + f0, d_g.as<int32_t>() + f0,
                               d_off.as<int64_t>(), d_kid.as<int32_t>(), d_ranks.as<int64_t>() + f0 * 2};
                relpred_rank_kernel<<<(unsigned)nf, 256, 0, t.stream>>>(ra);
                HIPCHK(hipGetLastError());
                sp.end();
            } else if (nf > 0) {
                if (!pk.ids.empty()) {
                    Span sp(hooks, "path_mask");
                    MaskArgs ma{kout + f0 * ne, ne, d_g.as<int32_t>() + f0, d_off.as<int64_t>(), d_kid.as<int32_t>()};
                    predict_mask_kernel<<<(unsigned)nf, 256, 0, t.stream>>>(ma);
                    HIPCHK(hipGetLastError());
                    sp.end();
                }
                Span sp(hooks, "path_select");
                SelectArgs sa{kout + f0 * ne, ne, k, d_ids.as<int32_t>() + f0 * k, d_en.as<double>() + f0 * k,
                              d_found.as<int32_t>() + f0};
                if (keys_lds) predict_select_kernel<true><<<(unsigned)nf, kSelThreads, select_lds, t.stream>>>(sa);
                else predict_select_kernel<false><<<(unsigned)nf, kSelThreads, select_lds, t.stream>>>(sa);
                HIPCHK(hipGetLastError());
                if (want_via && i >= 2) {
                    if (exact) {
                        // x_{i-1} of the answers, then x_{i-2} of those, ...: each level's back-pointer rows are kept
                        const int32_t* cur = d_ids.as<int32_t>() + f0 * k;
                        for (int lev = i; lev >= 2; --lev) {
                            int32_t* out = d_via.as<int32_t>() + ((int64_t)(lev - 2) * maxlive2 + f0) * k;
                            gather(d_pred.as<int32_t>() + (lvl_off[lev] + f0) * ne, cur, k, out, nf);
                            cur = out;
                        }
                    } else {
                        gather(pred_i + f0 * ne, d_ids.as<int32_t>() + f0 * k, k, d_last.as<int32_t>() + f0 * k, nf);
                    }
                }
                sp.end();
            }
            // the frontier of the queries that walk on: rows [0, live[i + 1])
            if (!exact && f0 > 0) {
                Span sp(hooks, "path_select");
                int32_t* fid_i = d_fid.as<int32_t>() + (int64_t)(i - 1) * fstride;
                SelectArgs sa{kout, ne, B, fid_i, d_fcost.as<double>(), d_fcount.as<int32_t>()};
                if (keys_lds) predict_select_kernel<true><<<(unsigned)f0, kSelThreads, select_lds, t.stream>>>(sa);
                else predict_select_kernel<false><<<(unsigned)f0, kSelThreads, select_lds, t.stream>>>(sa);
                HIPCHK(hipGetLastError());
                if (want_via && i >= 2) gather(pred_i, fid_i, B, d_back.as<int32_t>() + (int64_t)(i - 1) * fstride, f0);
                sp.end();
            }
        }
        // only the answers, and for their witnesses the frontiers' ids and back-pointers, leave the card
        const int64_t l2rows = live[2];
        if (ranking) {
            hranks.resize((size_t)mq * 2);
            HIPCHK(hipMemcpyAsync(hranks.data(), d_ranks.p, (size_t)mq * 2 * 8, hipMemcpyDeviceToHost, t.stream));
        } else {
            hids.resize((size_t)mq * k), hen.resize((size_t)mq * k), hfound.resize((size_t)mq);
            HIPCHK(hipMemcpyAsync(hids.data(), d_ids.p, (size_t)mq * k * 4, hipMemcpyDeviceToHost, t.stream));
            HIPCHK(hipMemcpyAsync(hen.data(), d_en.p, (size_t)mq * k * 8, hipMemcpyDeviceToHost, t.stream));
            HIPCHK(hipMemcpyAsync(hfound.data(), d_found.p, (size_t)mq * 4, hipMemcpyDeviceToHost, t.stream));
            if (want_via && l2rows > 0) {
                if (exact) {
                    hvia.resize((size_t)(chunkL - 1) * maxlive2 * k);
                    HIPCHK(hipMemcpyAsync(hvia.data(), d_via.p, hvia.size() * 4, hipMemcpyDeviceToHost, t.stream));
                } else {
                    hfid.resize((size_t)(chunkL - 1) * fstride), hback.resize(hfid.size()), hlast.resize((size_t)l2rows * k);
                    HIPCHK(hipMemcpyAsync(hfid.data(), d_fid.p, hfid.size() * 4, hipMemcpyDeviceToHost, t.stream));
                    HIPCHK(hipMemcpyAsync(hback.data(), d_back.p, hback.size() * 4, hipMemcpyDeviceToHost, t.stream));
                    HIPCHK(hipMemcpyAsync(hlast.data(), d_last.p, hlast.size() * 4, hipMemcpyDeviceToHost, t.stream));
                }
            }
        }
        HIPCHK(hipStreamSynchronize(t.stream));
        for (int64_t x = 0; x < mq; ++x) {  // back to the caller's order
            const int64_t o = order[(size_t)x];
            if (ranking) {
                ranks[o * 2] = hranks[(size_t)x * 2];
                ranks[o * 2 + 1] = hranks[(size_t)x * 2 + 1];
                continue;
            }
            std::copy_n(hids.data() + x * k, k, ids + o * k);
            std::copy_n(hen.data() + x * k, k, energy + o * k);
            found[o] = hfound[(size_t)x];
            const int L = (int)(q.offsets[o + 1] - q.offsets[o]);
            if (!want_via || L < 2) continue;
            for (int j = 0; j < hfound[(size_t)x]; ++j) {
                int32_t* w = via + (o * k + j) * (kPathMaxHops - 1);
                if (exact) {
                    for (int lev = 2; lev <= L; ++lev) w[lev - 2] = hvia[(size_t)(((int64_t)(lev - 2) * maxlive2 + x) * k + j)];
                } else if (!path_backtrack(L, B, hfid.data() + x * B, hback.data() + x * B, fstride,
                                           hlast[(size_t)(x * k + j)], w)) {
                    throw std::runtime_error("path query: a predecessor outside its frontier");
                }
            }
        }
        if (stats) ++stats->chunks;
    }
}

}  // namespace

void predict_path(const EvalTables& t, const PathQuery& q, int32_t* ids, double* energy, int32_t* found, int32_t* via,
                  PathStats* stats, const PredictHooks* hooks) {
    if (q.truth) throw std::invalid_argument("predict_path takes no true entities");
    run_path(t, q, ids, energy, found, via, nullptr, stats, hooks);
}

void rank_path(const EvalTables& t, const PathQuery& q, int64_t* ranks, PathStats* stats, const PredictHooks* hooks) {
    if (!q.truth) throw std::invalid_argument("rank_path needs the true entities");
    run_path(t, q, nullptr, nullptr, nullptr, nullptr, ranks, stats, hooks);
}

}  // namespace kb2e
