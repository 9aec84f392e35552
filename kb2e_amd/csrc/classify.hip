// classify.hip -- triple classification on the device.  Part of libkb2e.so
// (kb2e_fit_thresholds, kb2e_classify_triples, kb2e_corrupt_triples in
// engine.hip call in here).
//
// Fit.  The labelled triples are scored on the card (predict.hip's kernels:
// kb2e_score_triples' bits) and sorted there on the composite key (relation,
// energy bit pattern) with the 32-bit original index as payload.  Energies are
// sums of fabs() or squares, so >= +0, and unsigned order of the patterns is
// numeric order (as in predict.hip).  The sort is a stable least-significant-
// digit radix with 8-bit digits: the eight energy digits, then the digits of
// the relation id.  A pass is three launches -- sort_hist_kernel (a histogram
// per workgroup over its contiguous chunk), sort_scan_kernel (one workgroup per
// digit scans hist[digit][workgroup] in place) and sort_scatter_kernel (the
// same chunks again in order; an element's place is its digit's base + the
// earlier workgroups' count + its rank among the chunk's earlier elements of
// that digit, the in-wave part by the match-by-ballot idiom of
// predict_select_kernel).  The launch boundary is the only synchronisation
// between workgroups.  sort_prepare_kernel ORs and ANDs every key first; a
// digit in which the two agree is the same for every key and its pass is
// skipped (one read-back).
//
// After the energy passes the array is in energy order: fit_kernel, as one
// workgroup over [0, count), gives the global threshold.  After the relation
// passes segment_kernel stores each relation's first and one-past-last position
// (an element that differs from its predecessor writes both: unique writers,
// plain stores) and fit_kernel runs with one workgroup per relation.  The sweep
// walks a segment in tiles of 256 with the positives so far carried along;
// with P(j) the positives among the first j elements, cutting behind element j
// classifies  correct = N_total + (P(j) - (j - P(j)))  triples correctly, so it
// maximises g(j) = 2 P(j) - j over the j that end a run of equal keys (a cut
// inside a run is no threshold), from the -inf candidate j = 0, g = 0, and
// keeps the earliest maximum: (g, -j) packed into one word, reduced with max.
//
// Corrupt.  One thread per triple probes the filter set of the known triples
// (FilterView) with draws of the counter-based stream of classify_host.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "classify.hpp"
#include "classify_host.hpp"
#include "eval_shared.hpp"
#include "hip_util.hpp"
#include "host_data.hpp"

namespace kb2e {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

// ------------------------------------------------------------ radix sort

struct SortArgs {
    const uint64_t* ekey;  // [count] energy bit patterns, in the current order
    const uint32_t* idx;   // [count] original index of each
    const int32_t* rel;    // [count] relation by original index
    int64_t count;
    int64_t chunk;   // elements per workgroup (a multiple of kThreads)
    int32_t shift;   // of the digit, inside the energy pattern or the relation id
    int32_t by_rel;  // the digit is the relation's
    uint32_t* hist;  // [256][gridDim.x]: counts, then (sort_scan_kernel) exclusive sums along a row
    const uint32_t* total;  // [256] keys per digit
    uint64_t* out_ekey;
    uint32_t* out_idx;
};

__device__ __forceinline__ uint32_t sort_digit(const SortArgs& a, int64_t i) {
    if (a.by_rel) return ((uint32_t)a.rel[a.idx[i]] >> a.shift) & 255u;
    return (uint32_t)(a.ekey[i] >> a.shift) & 255u;
}

// The lanes of the wave that are active and hold the same digit as this one.
__device__ __forceinline__ uint64_t digit_peers(bool act, uint32_t dg) {
    uint64_t peers = __ballot(act);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const bool bit = (dg >> b) & 1u;
        const uint64_t bal = __ballot(act && bit);
        peers &= bit ? bal : ~bal;
    }
    return peers;
}

// Inclusive sum over the workgroup's 256 threads in thread order; *all = the
// workgroup's total.  wtot: [kWaves] LDS words; the caller keeps a barrier
// between two calls that share them.
__device__ __forceinline__ uint32_t block_inclusive_sum(uint32_t v, uint32_t* wtot, uint32_t* all) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t incl = v;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(incl, o);
        if (lane >= o) incl += up;
    }
    if (lane == 63) wtot[wv] = incl;
    __syncthreads();
    uint32_t sum = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        const uint32_t x = wtot[w];
        if (w < wv) incl += x;
        sum += x;
    }
    *all = sum;
    return incl;
}

struct PrepareArgs {
    const uint64_t* ekey;
    const int32_t* rel;
    int64_t count;
    uint32_t* idx;   // <- 0, 1, 2, ...
    uint64_t* bits;  // [4]: OR and AND of the energy patterns, OR and AND of the relation ids
};

__global__ __launch_bounds__(kThreads) void sort_prepare_kernel(PrepareArgs a) {
    uint64_t oe = 0, ae = ~0ull, orl = 0, arl = ~0ull;
    const int64_t step = (int64_t)gridDim.x * kThreads;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < a.count; i += step) {
        a.idx[i] = (uint32_t)i;
        const uint64_t e = a.ekey[i], r = (uint64_t)(uint32_t)a.rel[i];
        oe |= e;
        ae &= e;
        orl |= r;
        arl &= r;
    }
    for (int o = 32; o > 0; o >>= 1) {
        oe |= (uint64_t)__shfl_xor((unsigned long long)oe, o);
        ae &= (uint64_t)__shfl_xor((unsigned long long)ae, o);
        orl |= (uint64_t)__shfl_xor((unsigned long long)orl, o);
        arl &= (uint64_t)__shfl_xor((unsigned long long)arl, o);
    }
    if ((threadIdx.x & 63) == 0) {
        atomicOr((unsigned long long*)&a.bits[0], (unsigned long long)oe);
        atomicAnd((unsigned long long*)&a.bits[1], (unsigned long long)ae);
        atomicOr((unsigned long long*)&a.bits[2], (unsigned long long)orl);
        atomicAnd((unsigned long long*)&a.bits[3], (unsigned long long)arl);
    }
}

__global__ __launch_bounds__(kThreads) void sort_hist_kernel(SortArgs a) {
    __shared__ uint32_t hist[256];
    const int tid = threadIdx.x, lane = tid & 63;
    hist[tid] = 0;
    __syncthreads();
    const int64_t c0 = (int64_t)blockIdx.x * a.chunk, c1 = c0 + a.chunk < a.count ? c0 + a.chunk : a.count;
    for (int64_t base = c0; base < c1; base += kThreads) {  // (workgroup-uniform trip count)
        const int64_t i = base + tid;
        const bool act = i < c1;
        const uint32_t dg = act ? sort_digit(a, i) : 0u;
        const uint64_t peers = digit_peers(act, dg);
        // the lanes that hold the same digit add to its bin once
        if (act && lane == __ffsll((long long)peers) - 1) atomicAdd(&hist[dg], (uint32_t)__popcll(peers));
    }
    __syncthreads();
    a.hist[(int64_t)tid * gridDim.x + blockIdx.x] = hist[tid];
}

// One workgroup per digit: its row hist[digit][0..nwg) becomes the exclusive
// sums along the row, total[digit] the row's sum.
__global__ __launch_bounds__(kThreads) void sort_scan_kernel(uint32_t* hist, int32_t nwg, uint32_t* total) {
    __shared__ uint32_t wtot[kWaves];
    uint32_t* row = hist + (int64_t)blockIdx.x * nwg;
    uint32_t carry = 0;
    for (int base = 0; base < nwg; base += kThreads) {
        const int i = base + (int)threadIdx.x;
        const uint32_t v = i < nwg ? row[i] : 0u;
        uint32_t all;
        const uint32_t incl = block_inclusive_sum(v, wtot, &all);
        if (i < nwg) row[i] = carry + incl - v;
        carry += all;
        __syncthreads();  // (wtot is written again)
    }
    if (threadIdx.x == 0) total[blockIdx.x] = carry;
}

__global__ __launch_bounds__(kThreads) void sort_scatter_kernel(SortArgs a) {
    __shared__ uint32_t run[256];          // where the workgroup's next key of each digit goes
    __shared__ uint32_t wcnt[kWaves][256];  // the tile's keys per (wave, digit)
    __shared__ uint32_t wtot[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint64_t below_lanes = (1ull << lane) - 1;
    {
        // digit bases: the exclusive sums of total[256]
        const uint32_t tv = a.total[tid];
        uint32_t all;
        const uint32_t incl = block_inclusive_sum(tv, wtot, &all);
        run[tid] = incl - tv + a.hist[(int64_t)tid * gridDim.x + blockIdx.x];
#pragma unroll
        for (int w = 0; w < kWaves; ++w) wcnt[w][tid] = 0;
    }
    __syncthreads();
    const int64_t c0 = (int64_t)blockIdx.x * a.chunk, c1 = c0 + a.chunk < a.count ? c0 + a.chunk : a.count;
    for (int64_t base = c0; base < c1; base += kThreads) {  // (workgroup-uniform trip count)
        const int64_t i = base + tid;
        const bool act = i < c1;
        uint64_t ek = 0;
        uint32_t ix = 0, dg = 0;
        if (act) {
            ek = a.ekey[i];
            ix = a.idx[i];
            dg = sort_digit(a, i);
        }
        const uint64_t peers = digit_peers(act, dg);
        if (act && lane == __ffsll((long long)peers) - 1) wcnt[wv][dg] = (uint32_t)__popcll(peers);  // (one writer)
        __syncthreads();
        if (act) {
            uint32_t pos = run[dg] + (uint32_t)__popcll(peers & below_lanes);
#pragma unroll
            for (int w = 0; w < kWaves; ++w)
                if (w < wv) pos += wcnt[w][dg];
            a.out_ekey[pos] = ek;
            a.out_idx[pos] = ix;
        }
        __syncthreads();
        {  // thread d owns digit d: advance its place, clear its counts
            uint32_t s = 0;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) {
                s += wcnt[w][tid];
                wcnt[w][tid] = 0;
            }
            run[tid] += s;
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------ fit

struct SegmentArgs {
    const uint32_t* idx;
    const int32_t* rel;
    int64_t count;
    int32_t* seg_start;  // [nr], -1: the relation has no triple
    int32_t* seg_end;    // [nr]
};

__global__ __launch_bounds__(kThreads) void segment_kernel(SegmentArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= a.count) return;
    const int32_t r = a.rel[a.idx[i]];
    const int32_t p = i > 0 ? a.rel[a.idx[i - 1]] : -1;
    if (r != p) {
        a.seg_start[r] = (int32_t)i;
        if (p >= 0) a.seg_end[p] = (int32_t)i;
    }
    if (i == a.count - 1) a.seg_end[r] = (int32_t)a.count;
}

struct FitArgs {
    const uint64_t* ekey;
    const uint32_t* idx;
    const uint8_t* labels;     // by original index
    const int32_t* seg_start;  // null: one segment, [0, count)
    const int32_t* seg_end;
    int64_t count;
    const double* fallback;  // the threshold of an empty segment
    double* thr;             // [segments]
    int64_t* counts;         // [segments][3]
};

// (g, j) -> one word whose maximum is the largest g and, among those, the smallest j
__device__ __forceinline__ uint64_t umax64(uint64_t x, uint64_t y) { return x > y ? x : y; }

__device__ __forceinline__ uint64_t fit_pack(int64_t g, uint32_t j) {
    return ((uint64_t)(uint32_t)(g + 2147483648ll) << 32) | (uint64_t)(~j);
}

__global__ __launch_bounds__(kThreads) void fit_kernel(FitArgs a) {
    __shared__ uint32_t wtot[kWaves];
    __shared__ uint64_t wbest[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int seg = blockIdx.x;
    int64_t s0 = 0, s1 = a.count;
    if (a.seg_start) {
        s0 = a.seg_start[seg];
        s1 = a.seg_end[seg];
    }
    if (s0 < 0) {  // (workgroup-uniform)
        if (tid == 0) {
            a.thr[seg] = *a.fallback;
            a.counts[(int64_t)seg * 3] = a.counts[(int64_t)seg * 3 + 1] = a.counts[(int64_t)seg * 3 + 2] = 0;
        }
        return;
    }
    uint32_t positives = 0;             // in [s0, base)
    uint64_t best = fit_pack(0, 0u);    // the -inf candidate
    for (int64_t base = s0; base < s1; base += kThreads) {  // (workgroup-uniform trip count)
        const int64_t i = base + tid;
        const bool act = i < s1;
        uint64_t key = 0;
        uint32_t lab = 0;
        bool run_end = false;
        if (act) {
            key = a.ekey[i];
            lab = a.labels[a.idx[i]];
            run_end = i + 1 >= s1 || a.ekey[i + 1] != key;
        }
        uint32_t all;
        const uint32_t incl = block_inclusive_sum(lab, wtot, &all);
        const uint32_t j = (uint32_t)(i - s0 + 1);  // elements up to and including this one
        uint64_t cand = run_end ? fit_pack(2 * (int64_t)(positives + incl) - (int64_t)j, j) : 0ull;
        for (int o = 32; o > 0; o >>= 1) cand = umax64(cand, (uint64_t)__shfl_xor((unsigned long long)cand, o));
        if (lane == 0) wbest[wv] = cand;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < kWaves; ++w) best = umax64(best, wbest[w]);
        positives += all;
    }
    if (tid == 0) {
        const int64_t len = s1 - s0, neg = len - (int64_t)positives;
        const int64_t g = (int64_t)(uint32_t)(best >> 32) - 2147483648ll;
        const uint32_t j = ~(uint32_t)best;
        a.thr[seg] = j == 0 ? -(double)INFINITY : __longlong_as_double((long long)a.ekey[s0 + j - 1]);
        a.counts[(int64_t)seg * 3] = positives;
        a.counts[(int64_t)seg * 3 + 1] = neg;
        a.counts[(int64_t)seg * 3 + 2] = neg + g;
    }
}

// ------------------------------------------------------------ classify

__global__ __launch_bounds__(kThreads) void classify_kernel(const double* energy, const int32_t* rel,
                                                            const double* thr, int32_t count, uint8_t* out) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= count) return;
    out[x] = energy[x] <= thr[rel[x]] ? 1 : 0;
}

// ------------------------------------------------------------ corrupt

struct CorruptArgs {
    const int32_t *h, *t, *r;
    int64_t count;
    FilterView known;
    const int64_t* pool_off;  // [2 * nr + 1]
    const int32_t* pool_ids;
    uint64_t state;  // corrupt_mix(seed)
    int32_t ne, side, constrained;
    int32_t *nh, *nt;
};

__global__ __launch_bounds__(kThreads) void corrupt_kernel(CorruptArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= a.count) return;
    const int32_t h = a.h[i], t = a.t[i], r = a.r[i];
    const int slot = a.side == 2 ? (int)(corrupt_u(a.state, (uint64_t)i, 0) >> 63) : a.side;
    const int32_t old = slot ? t : h;
    const int64_t p0 = a.pool_off[(int64_t)r * 2 + slot], plen = a.pool_off[(int64_t)r * 2 + slot + 1] - p0;
    int32_t got = -1;
    const int first = a.constrained && plen > 0 ? 1 : kCorruptDraws + 1;
    for (int d = first; d <= 2 * kCorruptDraws && got < 0; ++d) {
        const uint64_t u = corrupt_u(a.state, (uint64_t)i, (uint64_t)d);
        const int32_t x = d <= kCorruptDraws ? a.pool_ids[p0 + (int64_t)(u % (uint64_t)plen)]
                                             : (int32_t)(u % (uint64_t)a.ne);
        if (x == old) continue;
        if (slot ? a.known.has(h, r, x) : a.known.has(x, r, t)) continue;
        got = x;
    }
    a.nh[i] = got < 0 ? -1 : slot ? h : got;
    a.nt[i] = got < 0 ? -1 : slot ? got : t;
}

// ------------------------------------------------------------ host side

void check_triples(const EvalTables& t, const int32_t* h, const int32_t* tl, const int32_t* r, int64_t count,
                   const char* what) {
    for (int64_t k = 0; k < count; ++k)
        if (h[k] < 0 || h[k] >= t.ne || tl[k] < 0 || tl[k] >= t.ne || r[k] < 0 || r[k] >= t.nr)
            throw std::invalid_argument(std::string(what) + " " + std::to_string(k) + " has an id out of range");
}

unsigned blocks_of(int64_t count) { return (unsigned)((count + kThreads - 1) / kThreads); }

// Elements per workgroup of a sort pass: 2,048, more once that would take over
// 4,096 workgroups (the scan walks a row of that length per digit).
// KB2E_CLASSIFY_SORT_CHUNK=<multiple of 256> sets it (tests: the result does
// not depend on it).
int64_t sort_chunk(int64_t count) {
    int64_t chunk = 2048;
    if ((count + chunk - 1) / chunk > 4096) chunk = ((count + 4095) / 4096 + kThreads - 1) / kThreads * kThreads;
    if (const char* v = getenv("KB2E_CLASSIFY_SORT_CHUNK")) {
        const long c = atol(v);
        if (c >= kThreads && c % kThreads == 0) chunk = c;
    }
    return chunk;
}

}  // namespace

void fit_thresholds(const EvalTables& t, const LabelledTriples& q, double* thresholds, int64_t* counts,
                    double* global_threshold, int64_t* global_correct, const PredictHooks* hooks) {
    const int64_t count = q.count;
    const int nr = t.nr;
    if (count < 1) throw std::invalid_argument("no labelled triples");
    if (count > INT32_MAX) throw std::invalid_argument("too many labelled triples in one call");
    check_triples(t, q.heads, q.tails, q.relations, count, "triple");
    for (int64_t k = 0; k < count; ++k)
        if (q.labels[k] > 1) throw std::invalid_argument("label " + std::to_string(k) + " is neither 0 nor 1");

    DevBuf d_h, d_t, d_r, d_lab, d_key[2], d_idx[2], d_bits, d_hist, d_total, d_seg, d_thr, d_cnt;
    d_h.alloc((size_t)count * 4);
    d_t.alloc((size_t)count * 4);
    d_r.alloc((size_t)count * 4);
    d_lab.alloc((size_t)count);
    for (int b = 0; b < 2; ++b) {
        d_key[b].alloc((size_t)count * 8);
        d_idx[b].alloc((size_t)count * 4);
    }
    const int64_t chunk = sort_chunk(count);
    const int32_t nwg = (int32_t)((count + chunk - 1) / chunk);
    d_bits.alloc(4 * 8);
    d_hist.alloc((size_t)256 * nwg * 4);
    d_total.alloc(256 * 4);
    d_seg.alloc((size_t)nr * 2 * 4);
    d_thr.alloc((size_t)(nr + 1) * 8);      // [nr] the relations', then the global one
    d_cnt.alloc((size_t)(nr + 1) * 3 * 8);  // likewise
    HIPCHK(hipMemcpyAsync(d_h.p, q.heads, (size_t)count * 4, hipMemcpyHostToDevice, t.stream));
    HIPCHK(hipMemcpyAsync(d_t.p, q.tails, (size_t)count * 4, hipMemcpyHostToDevice, t.stream));
    HIPCHK(hipMemcpyAsync(d_r.p, q.relations, (size_t)count * 4, hipMemcpyHostToDevice, t.stream));
    HIPCHK(hipMemcpyAsync(d_lab.p, q.labels, (size_t)count, hipMemcpyHostToDevice, t.stream));
    const uint64_t bits0[4] = {0ull, ~0ull, 0ull, ~0ull};
    HIPCHK(hipMemcpyAsync(d_bits.p, bits0, sizeof(bits0), hipMemcpyHostToDevice, t.stream));
    HIPCHK(hipMemsetAsync(d_seg.p, 0xFF, (size_t)nr * 2 * 4, t.stream));

    {
        // a double's bit pattern is the key: the energies land in the first key buffer
        Span sp(hooks, "classify_score");
        score_triples_device(t, d_h.as<int32_t>(), d_t.as<int32_t>(), d_r.as<int32_t>(), count, d_key[0].as<double>());
        sp.end();
    }
    uint64_t bits[4];
    {
        Span sp(hooks, "classify_sort");
        PrepareArgs pa{d_key[0].as<uint64_t>(), d_r.as<int32_t>(), count, d_idx[0].as<uint32_t>(), d_bits.as<uint64_t>()};
        sort_prepare_kernel<<<std::min(blocks_of(count), 1024u), kThreads, 0, t.stream>>>(pa);
        HIPCHK(hipGetLastError());
        sp.end();
    }
    HIPCHK(hipMemcpyAsync(bits, d_bits.p, sizeof(bits), hipMemcpyDeviceToHost, t.stream));
    HIPCHK(hipStreamSynchronize(t.stream));
    const uint64_t vary_e = bits[0] ^ bits[1], vary_r = bits[2] ^ bits[3];  // bits that differ between keys

    int cur = 0;  // the buffer pair that holds the current order
    auto pass = [&](int shift, int by_rel) {
        Span sp(hooks, "classify_sort");
        SortArgs sa{d_key[cur].as<uint64_t>(), d_idx[cur].as<uint32_t>(), d_r.as<int32_t>(), count, chunk, shift, by_rel,
                    d_hist.as<uint32_t>(), d_total.as<uint32_t>(), d_key[cur ^ 1].as<uint64_t>(),
                    d_idx[cur ^ 1].as<uint32_t>()};
        sort_hist_kernel<<<(unsigned)nwg, kThreads, 0, t.stream>>>(sa);
        HIPCHK(hipGetLastError());
        sort_scan_kernel<<<256, kThreads, 0, t.stream>>>(d_hist.as<uint32_t>(), nwg, d_total.as<uint32_t>());
        HIPCHK(hipGetLastError());
        sort_scatter_kernel<<<(unsigned)nwg, kThreads, 0, t.stream>>>(sa);
        HIPCHK(hipGetLastError());
        sp.end();
        cur ^= 1;
    };
    auto fit = [&](bool global) {
        FitArgs fa{d_key[cur].as<uint64_t>(), d_idx[cur].as<uint32_t>(), d_lab.as<uint8_t>(),
                   global ? nullptr : d_seg.as<int32_t>(), global ? nullptr : d_seg.as<int32_t>() + nr, count,
                   d_thr.as<double>() + nr, d_thr.as<double>() + (global ? nr : 0),
                   d_cnt.as<int64_t>() + (global ? (int64_t)nr * 3 : 0)};
        fit_kernel<<<global ? 1u : (unsigned)nr, kThreads, 0, t.stream>>>(fa);
        HIPCHK(hipGetLastError());
    };

    for (int d = 0; d < 8; ++d)
        if ((vary_e >> (8 * d)) & 0xFFull) pass(8 * d, 0);
    {
        Span sp(hooks, "classify_fit");
        fit(true);  // energy order: the global threshold
        sp.end();
    }
    for (int d = 0; d < 4; ++d)
        if ((vary_r >> (8 * d)) & 0xFFull) pass(8 * d, 1);
    {
        Span sp(hooks, "classify_fit");
        SegmentArgs ga{d_idx[cur].as<uint32_t>(), d_r.as<int32_t>(), count, d_seg.as<int32_t>(), d_seg.as<int32_t>() + nr};
        segment_kernel<<<blocks_of(count), kThreads, 0, t.stream>>>(ga);
        HIPCHK(hipGetLastError());
        fit(false);
        sp.end();
    }
    std::vector<double> hthr((size_t)nr + 1);
    std::vector<int64_t> hcnt(((size_t)nr + 1) * 3);
    HIPCHK(hipMemcpyAsync(hthr.data(), d_thr.p, hthr.size() * 8, hipMemcpyDeviceToHost, t.stream));
    HIPCHK(hipMemcpyAsync(hcnt.data(), d_cnt.p, hcnt.size() * 8, hipMemcpyDeviceToHost, t.stream));
    HIPCHK(hipStreamSynchronize(t.stream));
    std::copy_n(hthr.data(), nr, thresholds);
    std::copy_n(hcnt.data(), (size_t)nr * 3, counts);
    if (global_threshold) *global_threshold = hthr[(size_t)nr];
    if (global_correct) *global_correct = hcnt[(size_t)nr * 3 + 2];
}

void classify_triples(const EvalTables& t, const int32_t* heads, const int32_t* tails, const int32_t* relations,
                      int64_t count, const double* thresholds, uint8_t* labels_out, double* energy,
                      const PredictHooks* hooks) {
    if (count < 1) throw std::invalid_argument("no triples to classify");
    check_triples(t, heads, tails, relations, count, "triple");
    const int64_t chunk = std::min<int64_t>(count, (int64_t)1 << 22);
    DevBuf d_h, d_t, d_r, d_e, d_thr, d_lab;
    d_h.alloc((size_t)chunk * 4);
    d_t.alloc((size_t)chunk * 4);
    d_r.alloc((size_t)chunk * 4);
    d_e.alloc((size_t)chunk * 8);
    d_lab.alloc((size_t)chunk);
    d_thr.alloc((size_t)t.nr * 8);
    HIPCHK(hipMemcpyAsync(d_thr.p, thresholds, (size_t)t.nr * 8, hipMemcpyHostToDevice, t.stream));
    for (int64_t c0 = 0; c0 < count; c0 += chunk) {
        const int32_t m = (int32_t)std::min(chunk, count - c0);
        HIPCHK(hipMemcpyAsync(d_h.p, heads + c0, (size_t)m * 4, hipMemcpyHostToDevice, t.stream));
        HIPCHK(hipMemcpyAsync(d_t.p, tails + c0, (size_t)m * 4, hipMemcpyHostToDevice, t.stream));
        HIPCHK(hipMemcpyAsync(d_r.p, relations + c0, (size_t)m * 4, hipMemcpyHostToDevice, t.stream));
        Span sp(hooks, "classify_score");
        score_triples_device(t, d_h.as<int32_t>(), d_t.as<int32_t>(), d_r.as<int32_t>(), m, d_e.as<double>());
        classify_kernel<<<blocks_of(m), kThreads, 0, t.stream>>>(d_e.as<double>(), d_r.as<int32_t>(), d_thr.as<double>(), m,
                                                               d_lab.as<uint8_t>());
        HIPCHK(hipGetLastError());
        sp.end();
        HIPCHK(hipMemcpyAsync(labels_out + c0, d_lab.p, (size_t)m, hipMemcpyDeviceToHost, t.stream));
        if (energy) HIPCHK(hipMemcpyAsync(energy + c0, d_e.p, (size_t)m * 8, hipMemcpyDeviceToHost, t.stream));
        HIPCHK(hipStreamSynchronize(t.stream));
    }
}

int64_t corrupt_triples(const EvalTables& t, const CorruptQuery& q, int32_t* neg_heads, int32_t* neg_tails,
                        const PredictHooks* hooks) {
    const int64_t count = q.count;
    if (count < 1) throw std::invalid_argument("no triples to corrupt");
    if (count > INT32_MAX) throw std::invalid_argument("too many triples in one call");
    if (q.side < 0 || q.side > 2) throw std::invalid_argument("side must be 0 (head), 1 (tail) or 2 (a coin per triple)");
    check_triples(t, q.heads, q.tails, q.relations, count, "triple");
    check_triples(t, q.kh, q.kt, q.kr, q.nknown, "known triple");

    FilterSet fs;
    fs.build(std::vector<int32_t>(q.kh, q.kh + q.nknown), std::vector<int32_t>(q.kt, q.kt + q.nknown),
             std::vector<int32_t>(q.kr, q.kr + q.nknown), t.ne, t.nr);
    const SlotPools sp = build_slot_pools(q.kh, q.kt, q.kr, q.nknown, t.nr);

    DevBuf d_h, d_t, d_r, d_slots, d_off, d_ids, d_nh, d_nt;
    d_h.alloc((size_t)count * 4);
    d_t.alloc((size_t)count * 4);
    d_r.alloc((size_t)count * 4);
    d_nh.alloc((size_t)count * 4);
    d_nt.alloc((size_t)count * 4);
    d_slots.alloc(fs.slots.size() * 8);
    d_off.alloc(sp.off.size() * 8);
    d_ids.alloc(sp.ids.size() * 4);
    HIPCHK(hipMemcpyAsync(d_h.p, q.heads, (size_t)count * 4, hipMemcpyHostToDevice, t.stream));
    HIPCHK(hipMemcpyAsync(d_t.p, q.tails, (size_t)count * 4, hipMemcpyHostToDevice, t.stream));
    HIPCHK(hipMemcpyAsync(d_r.p, q.relations, (size_t)count * 4, hipMemcpyHostToDevice, t.stream));
    HIPCHK(hipMemcpyAsync(d_slots.p, fs.slots.data(), fs.slots.size() * 8, hipMemcpyHostToDevice, t.stream));
    HIPCHK(hipMemcpyAsync(d_off.p, sp.off.data(), sp.off.size() * 8, hipMemcpyHostToDevice, t.stream));
    if (!sp.ids.empty())
        HIPCHK(hipMemcpyAsync(d_ids.p, sp.ids.data(), sp.ids.size() * 4, hipMemcpyHostToDevice, t.stream));
    {
        Span span(hooks, "classify_corrupt");
        CorruptArgs ca{d_h.as<int32_t>(), d_t.as<int32_t>(), d_r.as<int32_t>(), count,
                       FilterView{d_slots.as<uint64_t>(), fs.mask, fs.nr, fs.ne}, d_off.as<int64_t>(),
                       d_ids.as<int32_t>(), corrupt_mix(q.seed), t.ne, q.side, q.constrained ? 1 : 0,
                       d_nh.as<int32_t>(), d_nt.as<int32_t>()};
        corrupt_kernel<<<blocks_of(count), kThreads, 0, t.stream>>>(ca);
        HIPCHK(hipGetLastError());
        span.end();
    }
    HIPCHK(hipMemcpyAsync(neg_heads, d_nh.p, (size_t)count * 4, hipMemcpyDeviceToHost, t.stream));
    HIPCHK(hipMemcpyAsync(neg_tails, d_nt.p, (size_t)count * 4, hipMemcpyDeviceToHost, t.stream));
    HIPCHK(hipStreamSynchronize(t.stream));
    int64_t failed = 0;
    for (int64_t k = 0; k < count; ++k) failed += neg_heads[k] < 0;
    return failed;
}

}  // namespace kb2e
