// foldrel.hip -- relation fold-in on the device.  Part of libkb2e.so
// (kb2e_fold_in_relations in engine.hip calls in here).
//
// With every entity row frozen, each free relation is an SGD problem of its
// own: its samples read frozen entity rows and its own parameters, and write
// its own parameters.  fold_rel_kernel gives each free relation one unit -- a
// four-wave workgroup -- for all passes.  Units never communicate: no flag, no
// spin wait, no barrier between workgroups; the rows are stored once, after
// the last pass.  So the result depends neither on the grid size
// (KB2E_FOLDREL_GRID=<workgroups>: tests) nor on the order of the units, which
// the host sorts by descending number of examples.
//
// A batch has two phases (the reference's prebatch / postbatch rule: every
// gradient of a batch is taken at the parameters the batch found).
//
// Phase 1, side by side.  The batch's samples are dealt to the four waves
// (sample s to wave s mod 4).  A wave makes the 32 candidate draws of a sample
// side by side (lane a - 1 takes draw a, a ballot finds the first accepted
// one), loads the three entity rows (lane l holds the elements l + 64 c, c <
// NC), turns them into the model's features with the parameters in LDS, takes
// both energies as wave sums and leaves one record: flag, slot and negative
// id, the loss term, and per triple the gradient direction x[n] (TransH: and
// headSum, tailSum, sum_x).  A record is 2 (n + 4) doubles; the batch's
// records lie in LDS while they fit kRecLdsBytes beside the parameters, else in
// a global scratch of this workgroup.
//
// Phase 2, in sample order.  Every thread owns fixed elements of the working
// parameters: of r and the TransH normal the elements tid + 256 c (in
// registers across the unit; copied to LDS for phase 1 at the start of a
// batch), of the TransR matrix the rows j = wave (mod 4), lane l the columns
// l + 64 c.  The deltas of the active records are applied in order; lengths
// and loop tests are workgroup sums in a fixed tree (wave_sum, then the four
// wave results added in wave order), so every thread takes the same branch.
// There are no atomics.  The frozen-entity transRNorm needs q = aW: every wave
// sums its own rows per column, the four partial vectors meet in LDS, and every
// wave adds them in wave order; a sweep is W -= 2 lr a (x) q on the wave's own
// rows.
//
// The TransR matrix lives in LDS with the row pitch n | 1 (odd: the row-wise
// and the column-wise walks are both conflict-free) up to n =
// fold_rel_lds_limit(); wider, or with KB2E_FOLDREL_W_L2=1, it is worked on in
// a global FP64 scratch of this workgroup with the same pitch.
//
// Every loop is bounded: the coupling loops (the free r / w loop of TransH
// included) by the sweep cap, the known-set probe by the table size.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

#include "classify_host.hpp"
#include "eval_shared.hpp"
#include "foldrel.hpp"
#include "foldrel_host.hpp"
#include "hip_util.hpp"
#include "kernels_common.hpp"

namespace kb2e {
namespace {

constexpr int kThreads = 256, kWaves = 4;
constexpr size_t kRecLdsBytes = 32 * 1024;  // the longest record staging kept in LDS
constexpr int kRedDoubles = 16;             // two buffers of four wave results (and padding)

template <typename T>
struct FoldRelArgs {
    int32_t n, ld, ne, l1, nfree, epochs, side, cap, ldp, rec_lds;
    int64_t bcap, batch, count;
    const T* ent;
    T* rel;
    T* w;
    T* w_mirror;  // a second copy of the weight table to keep equal (may be null)
    double lr, margin;
    const int32_t *h, *t;
    const int32_t* unit_free;
    const int32_t* free_ids;
    const int64_t* off;
    const int32_t* perm;
    FilterView known;
    uint64_t state;  // corrupt_mix(seed)
    const double* rel_in;
    const double* w_in;
    double* rel_out;
    double* w_out;
    double* loss;
    int64_t* counts;
    double* rec_scratch;  // [grid][bcap][2 (n + 4)] unless rec_lds
    double* w_scratch;    // TransR without LDS staging: [grid][n][ldp]
};

// FilterView::has with the probe bounded by the table size
__device__ __forceinline__ bool rel_known(const FilterView& v, int64_t h, int64_t r, int64_t t) {
    const uint64_t k = ((uint64_t)h * v.nr64 + (uint64_t)r) * v.ne64 + (uint64_t)t;
    uint64_t p = eval_mix64(k) & v.mask;
    for (uint64_t step = 0; step <= v.mask; ++step) {
        const uint64_t s = v.slots[p];
        if (s == k) return true;
        if (s == ~0ull) return false;
        p = (p + 1) & v.mask;
    }
    return true;  // (a full table: not reached, the table is at most half full)
}

template <typename T, int NC>
__device__ __forceinline__ void rel_load(const T* row, int n, double (&out)[NC]) {
    const int l = lane_id();
#pragma unroll
    for (int c = 0; c < NC; ++c) out[c] = l + 64 * c < n ? (double)row[l + 64 * c] : 0.0;
}

template <int NC>
__device__ __forceinline__ double rel_dot(const double (&a)[NC], const double (&b)[NC]) {
    double s = 0;
#pragma unroll
    for (int c = 0; c < NC; ++c) s += a[c] * b[c];  // (elements past n are zero)
    return wave_sum(s);
}

// The workgroup's sum of v: a wave sum, then the four wave results in wave
// order.  Two result buffers alternate (par), so one barrier a sum is enough:
// a buffer is written again only after every wave has passed the barrier of
// the sum in between.  Every thread gets the same bits.
__device__ __forceinline__ double block_sum(double v, double* red, int& par) {
    v = wave_sum(v);
    if (lane_id() == 0) red[par * kWaves + (threadIdx.x >> 6)] = v;
    __syncthreads();
    const double* q = red + par * kWaves;
    const double s = ((q[0] + q[1]) + q[2]) + q[3];
    par ^= 1;
    return s;
}

// common::norm (common/utils.cpp:70-77) of a vector spread over the workgroup
template <int NV>
__device__ __forceinline__ void block_norm(double (&v)[NV], bool shrink, double* red, int& par) {
    double s = 0;
#pragma unroll
    for (int c = 0; c < NV; ++c) s += v[c] * v[c];
    const double len = sqrt(block_sum(s, red, par));
    if (!shrink || len > 1.0) {
#pragma unroll
        for (int c = 0; c < NV; ++c) v[c] = v[c] / len;
    }
}

// common::norm(a, b, rate) (common/utils.cpp:79-111), `sum` carried from sweep
// to sweep as there; frozen: the statement that writes a is removed.
template <int NV>
__device__ __forceinline__ void block_orth(double (&av)[NV], double (&bv)[NV], bool frozen, double lr, int cap,
                                           int64_t& capped, double* red, int& par) {
    block_norm<NV>(bv, false, red, par);
    double sum = 0;
    int sweeps = 0;
    while (true) {
        double s = 0;
#pragma unroll
        for (int c = 0; c < NV; ++c) s += bv[c] * bv[c];
        sum = sqrt(sum + block_sum(s, red, par));
        double x = 0;
#pragma unroll
        for (int c = 0; c < NV; ++c) {
            bv[c] = bv[c] / sum;
            x += bv[c] * av[c];
        }
        x = block_sum(x, red, par);
        if (!(x > 0.1)) break;
        if (sweeps == cap) {
            ++capped;
            break;
        }
#pragma unroll
        for (int c = 0; c < NV; ++c) {
            if (!frozen) av[c] = av[c] - lr * bv[c];
            bv[c] = bv[c] - lr * av[c];
        }
        ++sweeps;
    }
    block_norm<NV>(bv, false, red, par);
}

// LDS doubles before the records: red | r | TransH: w | TransR: 4 x 3n phase-1
// vectors, 3n staged entity rows, 2 x 4 x n partial projections, the matrix
__host__ __device__ inline size_t rel_lds_base(int model, int n, bool wl) {
    size_t d = kRedDoubles + (size_t)n;
    if (model == 1) d += (size_t)n;
    if (model == 2) d += (size_t)(12 + 3 + 8) * n + (wl ? (size_t)n * (n | 1) : 0);
    return d;
}

// MODEL 0 TransE, 1 TransH, 2 TransR; WL (TransR): the matrix is in LDS.
template <typename T, int MODEL, int NC, bool WL>
__global__ __launch_bounds__(kThreads) void fold_rel_kernel(FoldRelArgs<T> a) {
    constexpr int NV = NC > 4 ? 2 : 1;  // elements tid + 256 c of a vector
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int tid = threadIdx.x, l = lane_id(), wave = tid >> 6;
    const int n = a.n, ldp = a.ldp;
    const int reclen = 2 * (n + 4);
    double* const red = lds;
    double* const rl = lds + kRedDoubles;
    double* const wl = rl + n;                                   // TransH
    double* const pvec = rl + n + (size_t)wave * 3 * n;          // TransR: this wave's phase-1 vectors
    double* const stage = rl + n + (size_t)12 * n;               // TransR: head, tail, entity[rho]
    double* const part = stage + 3 * n;                          // TransR: [2][4][n]
    double* W;
    if constexpr (WL) W = part + 8 * n;
    else W = MODEL == 2 ? a.w_scratch + (size_t)blockIdx.x * n * ldp : nullptr;
    double* const recs = a.rec_lds ? lds + rel_lds_base(MODEL, n, WL)
                                   : a.rec_scratch + (size_t)blockIdx.x * (size_t)a.bcap * reclen;
    int par = 0, pp = 0;

    for (int u = blockIdx.x; u < a.nfree; u += gridDim.x) {
        const int fi = a.unit_free[u];
        const int32_t rho = a.free_ids[fi];
        // ---- the working parameters
        double rv[NV], wv[NV];
#pragma unroll
        for (int c = 0; c < NV; ++c) {
            const int e = tid + kThreads * c;
            rv[c] = wv[c] = 0;
            if (e < n) {
                rv[c] = a.rel_in ? a.rel_in[(int64_t)fi * n + e] : (double)a.rel[(int64_t)rho * a.ld + e];
                if constexpr (MODEL == 1)
                    wv[c] = a.w_in ? a.w_in[(int64_t)fi * n + e] : (double)a.w[(int64_t)rho * a.ld + e];
            }
        }
        if constexpr (MODEL == 2) {
            __syncthreads();  // (the previous unit's final reads of the matrix)
            for (int idx = tid; idx < n * n; idx += kThreads) {
                const int j = idx / n, k = idx - j * n;
                W[j * ldp + k] = a.w_in ? a.w_in[(int64_t)fi * n * n + idx]
                                        : (double)a.w[((int64_t)rho * n + j) * a.ld + k];
            }
        }
        const int64_t e0 = a.off[fi], cnt = a.off[fi + 1] - e0;
        int64_t active = 0, failed = 0, capped = 0;
        double loss_first = 0, loss_last = 0;

        for (int p = 0; p < a.epochs; ++p) {
            double lossp = 0;
            for (int64_t b0 = 0; b0 < cnt; b0 += a.batch) {
                const int64_t bn = cnt - b0 < a.batch ? cnt - b0 : a.batch;
                // ---- the snapshot for phase 1
#pragma unroll
                for (int c = 0; c < NV; ++c) {
                    const int e = tid + kThreads * c;
                    if (e < n) {
                        rl[e] = rv[c];
                        if constexpr (MODEL == 1) wl[e] = wv[c];
                    }
                }
                __syncthreads();

                // ================= phase 1: the batch's samples over the four waves
                for (int64_t s = wave; s < bn; s += kWaves) {
                    double* const rec = recs + s * reclen;
                    const int32_t i = a.perm[e0 + b0 + s];
                    const int32_t h = a.h[i], t = a.t[i];
                    const uint64_t ctr = (uint64_t)p * (uint64_t)a.count + (uint64_t)i;
                    const int cslot = a.side == 2 ? (int)(corrupt_u(a.state, ctr, 0) >> 63) : a.side;
                    const int32_t old = cslot ? t : h;
                    bool ok = false;
                    int32_t cand = 0;
                    if (l < kFoldDraws) {
                        cand = (int32_t)(corrupt_u(a.state, ctr, (uint64_t)(l + 1)) % (uint64_t)a.ne);
                        ok = cand != old &&
                             !(cslot ? rel_known(a.known, h, rho, cand) : rel_known(a.known, cand, rho, t));
                    }
                    const uint64_t accepted = __ballot(ok);
                    if (!accepted) {  // (wave-uniform)
                        if (l == 0) rec[0] = -1.0;
                        continue;
                    }
                    const int32_t got = __shfl(cand, __ffsll((long long)accepted) - 1);

                    // ---- features of the head, the tail and the drawn entity
                    double xe[3][NC], ft[3][NC], rr[NC], wr[NC];
                    rel_load<T, NC>(a.ent + (int64_t)h * a.ld, n, xe[0]);
                    rel_load<T, NC>(a.ent + (int64_t)t * a.ld, n, xe[1]);
                    rel_load<T, NC>(a.ent + (int64_t)got * a.ld, n, xe[2]);
#pragma unroll
                    for (int c = 0; c < NC; ++c) {
                        rr[c] = l + 64 * c < n ? rl[l + 64 * c] : 0.0;
                        wr[c] = 0;
                    }
                    double dots[3] = {0, 0, 0};  // TransH: w . row
                    if constexpr (MODEL == 0) {
#pragma unroll
                        for (int q = 0; q < 3; ++q)
#pragma unroll
                            for (int c = 0; c < NC; ++c) ft[q][c] = xe[q][c];
                    } else if constexpr (MODEL == 1) {
#pragma unroll
                        for (int c = 0; c < NC; ++c) wr[c] = l + 64 * c < n ? wl[l + 64 * c] : 0.0;
#pragma unroll
                        for (int q = 0; q < 3; ++q) {
                            dots[q] = rel_dot<NC>(wr, xe[q]);
#pragma unroll
                            for (int c = 0; c < NC; ++c) ft[q][c] = xe[q][c] - dots[q] * wr[c];
                        }
                    } else {
                        wave_lds_sync();  // (the previous sample's reads of the vectors are done)
#pragma unroll
                        for (int q = 0; q < 3; ++q)
#pragma unroll
                            for (int c = 0; c < NC; ++c)
                                if (l + 64 * c < n) pvec[q * n + l + 64 * c] = xe[q][c];
                        wave_lds_sync();
#pragma unroll
                        for (int q = 0; q < 3; ++q)
#pragma unroll
                            for (int c = 0; c < NC; ++c) ft[q][c] = 0;
                        // column sums p_k = sum_j W[j][k] v[j], j ascending (transr/transr.cpp:20-25); lane = column
                        for (int j = 0; j < n; ++j) {
                            const double v0 = pvec[j], v1 = pvec[n + j], v2 = pvec[2 * n + j];
#pragma unroll
                            for (int c = 0; c < NC; ++c) {
                                const int k = l + 64 * c;
                                if (k < n) {
                                    const double wjk = W[j * ldp + k];
                                    ft[0][c] += wjk * v0;
                                    ft[1][c] += wjk * v1;
                                    ft[2][c] += wjk * v2;
                                }
                            }
                        }
                    }

                    // ---- energies: d = feature(tail) - feature(head) - r
                    double dpos[NC], dneg[NC];
                    double sp = 0, sn = 0;
#pragma unroll
                    for (int c = 0; c < NC; ++c) {
                        const double nh = cslot == 0 ? ft[2][c] : ft[0][c], nt = cslot == 1 ? ft[2][c] : ft[1][c];
                        dpos[c] = ft[1][c] - ft[0][c] - rr[c];
                        dneg[c] = nt - nh - rr[c];
                        if (l + 64 * c < n) {
                            sp += a.l1 ? fabs(dpos[c]) : dpos[c] * dpos[c];
                            sn += a.l1 ? fabs(dneg[c]) : dneg[c] * dneg[c];
                        }
                    }
                    const double epos = wave_sum(sp), eneg = wave_sum(sn);
                    if (!(epos + a.margin > eneg)) {  // (wave-uniform)
                        if (l == 0) rec[0] = 0.0;
                        continue;
                    }
                    // ---- the record: x of both triples (TransH: and the three sums)
                    double sxp = 0, sxn = 0;
#pragma unroll
                    for (int c = 0; c < NC; ++c) {
                        double gp = 2.0 * dpos[c], gn = 2.0 * dneg[c];
                        if (a.l1) {
                            gp = gp > 0 ? 1.0 : -1.0;
                            gn = gn > 0 ? 1.0 : -1.0;
                        }
                        if (l + 64 * c < n) {
                            rec[4 + l + 64 * c] = gp;
                            rec[n + 8 + l + 64 * c] = gn;
                            sxp += gp * wr[c];
                            sxn += gn * wr[c];
                        }
                    }
                    if constexpr (MODEL == 1) {
                        sxp = wave_sum(sxp);
                        sxn = wave_sum(sxn);
                    }
                    if (l == 0) {
                        rec[0] = (double)(1 + 2 * cslot) + 4.0 * (double)got;
                        rec[1] = dots[0];
                        rec[2] = dots[1];
                        rec[3] = sxp;
                        rec[n + 4] = a.margin + epos - eneg;
                        rec[n + 5] = cslot == 0 ? dots[2] : dots[0];
                        rec[n + 6] = cslot == 1 ? dots[2] : dots[1];
                        rec[n + 7] = sxn;
                    }
                }
                __syncthreads();  // the records are complete; phase 1 has read the snapshot

                // ================= phase 2: the active records in sample order
                for (int64_t s = 0; s < bn; ++s) {
                    const double* const rec = recs + s * reclen;
                    const double meta = rec[0];  // (the same for every thread)
                    if (meta < 0) {
                        ++failed;
                        continue;
                    }
                    if (meta == 0) continue;
                    ++active;
                    lossp += rec[n + 4];
                    const int64_t m = (int64_t)meta;
                    const int cslot = (int)((m >> 1) & 1);
                    const int32_t got = (int32_t)(m >> 2);
                    const int32_t i = a.perm[e0 + b0 + s];
                    for (int neg = 0; neg < 2; ++neg) {
                        const int32_t eh = neg && cslot == 0 ? got : a.h[i], et = neg && cslot == 1 ? got : a.t[i];
                        const double* const x = rec + neg * (n + 4) + 4;
                        const double bl = (neg ? 1.0 : -1.0) * a.lr;
                        if constexpr (MODEL == 0) {
                            // transe/trainer.cpp:38, 43
#pragma unroll
                            for (int c = 0; c < NV; ++c) {
                                const int e = tid + kThreads * c;
                                if (e < n) rv[c] = rv[c] - bl * x[e];
                            }
                            block_norm<NV>(rv, true, red, par);
                        } else if constexpr (MODEL == 1) {
                            // transh/trainer.cpp:34, 39-40, 44-45, 48, 52, 56-58
                            const double hs = x[-3], ts = x[-2], sx = x[-1];
                            double av[NV], bv[NV];
#pragma unroll
                            for (int c = 0; c < NV; ++c) {
                                const int e = tid + kThreads * c;
                                av[c] = bv[c] = 0;
                                if (e < n) {
                                    av[c] = (double)a.ent[(int64_t)eh * a.ld + e];
                                    bv[c] = (double)a.ent[(int64_t)et * a.ld + e];
                                    const double xe = x[e];
                                    rv[c] = rv[c] - bl * xe;
                                    wv[c] = wv[c] + bl * xe * hs;
                                    wv[c] = wv[c] - bl * xe * ts;
                                    wv[c] = wv[c] + bl * sx * av[c];
                                    wv[c] = wv[c] - bl * sx * bv[c];
                                }
                            }
                            block_norm<NV>(rv, true, red, par);
                            block_norm<NV>(wv, false, red, par);
                            block_orth<NV>(rv, wv, false, a.lr, a.cap, capped, red, par);
                            block_orth<NV>(av, wv, true, a.lr, a.cap, capped, red, par);
                            block_orth<NV>(bv, wv, true, a.lr, a.cap, capped, red, par);
                        } else {
                            // transr/trainer.cpp:167, 171, 174, 178-180, 185-187
                            const bool third = rho < a.ne;
                            __syncthreads();  // (the previous triple's loops have read the staged rows)
#pragma unroll
                            for (int c = 0; c < NV; ++c) {
                                const int e = tid + kThreads * c;
                                if (e < n) {
                                    stage[e] = (double)a.ent[(int64_t)eh * a.ld + e];
                                    stage[n + e] = (double)a.ent[(int64_t)et * a.ld + e];
                                    if (third) stage[2 * n + e] = (double)a.ent[(int64_t)rho * a.ld + e];
                                    rv[c] = rv[c] - bl * x[e];
                                }
                            }
                            block_norm<NV>(rv, false, red, par);  // (its barrier also publishes the staged rows)
                            double xk[NC];
#pragma unroll
                            for (int c = 0; c < NC; ++c) xk[c] = l + 64 * c < n ? bl * x[l + 64 * c] : 0.0;
                            for (int j = wave; j < n; j += kWaves) {
                                const double dj = stage[j] - stage[n + j];
                                double sq = 0, row[NC];
#pragma unroll
                                for (int c = 0; c < NC; ++c) {
                                    const int k = l + 64 * c;
                                    row[c] = 0;
                                    if (k < n) {
                                        row[c] = W[j * ldp + k] - xk[c] * dj;
                                        sq += row[c] * row[c];
                                    }
                                }
                                const double len = sqrt(wave_sum(sq));
#pragma unroll
                                for (int c = 0; c < NC; ++c) {
                                    const int k = l + 64 * c;
                                    if (k < n) W[j * ldp + k] = row[c] / len;
                                }
                            }
                            // transRNorm with `a[j] -= ...` removed: head, tail, entity[rho]
                            for (int q = 0; q < (third ? 3 : 2); ++q) {
                                const double* const av = stage + q * n;
                                int sweeps = 0;
                                while (true) {
                                    double pk[NC];
#pragma unroll
                                    for (int c = 0; c < NC; ++c) pk[c] = 0;
                                    for (int j = wave; j < n; j += kWaves) {
                                        const double aj = av[j];
#pragma unroll
                                        for (int c = 0; c < NC; ++c) {
                                            const int k = l + 64 * c;
                                            if (k < n) pk[c] += W[j * ldp + k] * aj;
                                        }
                                    }
                                    double* const mine = part + (size_t)(pp * kWaves + wave) * n;
#pragma unroll
                                    for (int c = 0; c < NC; ++c)
                                        if (l + 64 * c < n) mine[l + 64 * c] = pk[c];
                                    __syncthreads();
                                    const double* const all = part + (size_t)pp * kWaves * n;
                                    pp ^= 1;
                                    double qk[NC], sq = 0;
#pragma unroll
                                    for (int c = 0; c < NC; ++c) {
                                        const int k = l + 64 * c;
                                        qk[c] = k < n ? ((all[k] + all[n + k]) + all[2 * n + k]) + all[3 * n + k] : 0.0;
                                        sq += qk[c] * qk[c];
                                    }
                                    const double xx = wave_sum(sq);  // (the same bits in every wave)
                                    if (!(xx > 1.0)) break;
                                    if (sweeps == a.cap) {
                                        ++capped;
                                        break;
                                    }
                                    for (int j = wave; j < n; j += kWaves) {
                                        const double aj = av[j];
#pragma unroll
                                        for (int c = 0; c < NC; ++c) {
                                            const int k = l + 64 * c;
                                            if (k < n) W[j * ldp + k] = W[j * ldp + k] - a.lr * (2.0 * qk[c]) * aj;
                                        }
                                    }
                                    ++sweeps;
                                }
                            }
                        }
                    }
                }
                __syncthreads();  // phase 2 is done with the records and the matrix rows
            }
            if (p == 0) loss_first = lossp;
            if (p == a.epochs - 1) loss_last = lossp;
        }

        // ---- the rows are rounded to the table's precision once, here
#pragma unroll
        for (int c = 0; c < NV; ++c) {
            const int e = tid + kThreads * c;
            if (e < n) {
                const T stored = (T)rv[c];
                a.rel[(int64_t)rho * a.ld + e] = stored;
                if (a.rel_out) a.rel_out[(int64_t)fi * n + e] = (double)stored;
                if constexpr (MODEL == 1) {
                    const T sw = (T)wv[c];
                    a.w[(int64_t)rho * a.ld + e] = sw;
                    if (a.w_out) a.w_out[(int64_t)fi * n + e] = (double)sw;
                }
            }
        }
        if constexpr (MODEL == 2) {
            for (int idx = tid; idx < n * n; idx += kThreads) {
                const int j = idx / n, k = idx - j * n;
                const T sw = (T)W[j * ldp + k];
                a.w[((int64_t)rho * n + j) * a.ld + k] = sw;
                if (a.w_mirror) a.w_mirror[((int64_t)rho * n + j) * a.ld + k] = sw;
                if (a.w_out) a.w_out[(int64_t)fi * n * n + idx] = (double)sw;
            }
        }
        if (tid == 0) {
            a.loss[(int64_t)fi * 2] = loss_first;
            a.loss[(int64_t)fi * 2 + 1] = loss_last;
            a.counts[(int64_t)fi * 3] = active;
            a.counts[(int64_t)fi * 3 + 1] = failed;
            a.counts[(int64_t)fi * 3 + 2] = capped;
        }
    }
}

template <typename T, int MODEL, int NC, bool WL>
void launch_rel(const FoldRelArgs<T>& a, unsigned grid, size_t lds, hipStream_t stream) {
    auto kernel = fold_rel_kernel<T, MODEL, NC, WL>;
    if (lds > 48 * 1024) allow_lds(kernel, lds);
    kernel<<<grid, kThreads, lds, stream>>>(a);
    HIPCHK(hipGetLastError());
}

template <typename T, int MODEL, bool WL>
void launch_rel_nc(const FoldRelArgs<T>& a, unsigned grid, size_t lds, hipStream_t stream) {
    if (a.n <= 64) launch_rel<T, MODEL, 1, WL>(a, grid, lds, stream);
    else if (a.n <= 128) launch_rel<T, MODEL, 2, WL>(a, grid, lds, stream);
    else if (a.n <= 256) launch_rel<T, MODEL, 4, WL>(a, grid, lds, stream);
    else if constexpr (!WL) launch_rel<T, MODEL, 8, WL>(a, grid, lds, stream);
    else throw std::logic_error("relation fold-in: a staged matrix this wide");  // (the host never asks for it)
}

bool want_w_lds(int n) {
    const char* l2 = getenv("KB2E_FOLDREL_W_L2");
    return n <= fold_rel_lds_limit() && !(l2 && atoi(l2) != 0);
}

template <typename V>
void upload(DevBuf& d, const V* src, size_t count, hipStream_t stream) {
    d.alloc(count * sizeof(V));
    if (count) HIPCHK(hipMemcpyAsync(d.p, src, count * sizeof(V), hipMemcpyHostToDevice, stream));
}

}  // namespace

int32_t fold_rel_lds_limit() {
    static const int32_t limit = [] {
        int32_t n = 1;
        while (rel_lds_base(2, n + 1, true) * 8 <= kLdsMax) ++n;
        return n;
    }();
    return limit;
}

void fold_in_relations(const EvalTables& t, const FoldRelQuery& q, double* rel_out, double* w_out, double* loss,
                       int64_t* counts, const PredictHooks* hooks) {
    if (q.epochs < 1) throw std::invalid_argument("epochs must be at least 1");
    if (q.batch_size < 1) throw std::invalid_argument("batch_size must be at least 1");
    if (q.side < 0 || q.side > 2) throw std::invalid_argument("side must be 0 (head), 1 (tail) or 2 (a coin per sample)");
    if (q.max_sweeps < 0) throw std::invalid_argument("max_sweeps must not be negative");
    if (!loss || !counts) throw std::invalid_argument("loss and counts are required");
    if (t.model == 0 && (q.w_in || w_out)) throw std::invalid_argument("TransE has no normals or matrices (w_in / w_out)");
    const FoldRelPlan plan = plan_fold_rel(q.free_relations, q.nfree, q.heads, q.tails, q.relations, q.count, q.kh, q.kt,
                                           q.kr, q.nknown, t.ne, t.nr);
    const FilterSet fs = fold_known_set(q.heads, q.tails, q.relations, q.count, q.kh, q.kt, q.kr, q.nknown, t.ne, t.nr);
    const int64_t nfree = q.nfree, n = t.n;
    const int64_t wlen = t.model == 1 ? n : n * n;  // doubles of one relation's normal / matrix

    unsigned grid = (unsigned)std::min<int64_t>(nfree, 1024);
    if (const char* v = getenv("KB2E_FOLDREL_GRID")) {
        const long g = atol(v);
        if (g >= 1 && g < (long)grid) grid = (unsigned)g;
    }
    const bool wl = t.model == 2 && want_w_lds(t.n);
    if (t.model == 2 && !wl) grid = std::min(grid, 256u);  // (one matrix scratch per workgroup)
    const int64_t bcap = fold_rel_batch_cap(q.batch_size, plan.longest);
    const size_t reclen = (size_t)2 * (n + 4), base = rel_lds_base(t.model, t.n, wl);
    const bool rec_lds = (size_t)bcap * reclen * 8 <= kRecLdsBytes && (base + (size_t)bcap * reclen) * 8 <= kLdsMax;
    const size_t lds = (base + (rec_lds ? (size_t)bcap * reclen : 0)) * 8;

    HIPCHK(hipStreamSynchronize(t.stream));
    DevBuf d_free, d_h, d_t, d_unit, d_off, d_perm, d_slots, d_rin, d_win, d_rout, d_wout, d_loss, d_cnt, d_rec, d_w;
    upload(d_free, q.free_relations, (size_t)nfree, t.stream);
    upload(d_h, q.heads, (size_t)q.count, t.stream);
    upload(d_t, q.tails, (size_t)q.count, t.stream);
    upload(d_unit, plan.unit_free.data(), plan.unit_free.size(), t.stream);
    upload(d_off, plan.off.data(), plan.off.size(), t.stream);
    upload(d_perm, plan.perm.data(), plan.perm.size(), t.stream);
    upload(d_slots, fs.slots.data(), fs.slots.size(), t.stream);
    if (q.rel_in) upload(d_rin, q.rel_in, (size_t)(nfree * n), t.stream);
    if (q.w_in) upload(d_win, q.w_in, (size_t)(nfree * wlen), t.stream);
    d_rout.alloc((size_t)(nfree * n) * 8);
    if (t.model != 0) d_wout.alloc((size_t)(nfree * wlen) * 8);
    d_loss.alloc((size_t)nfree * 2 * 8);
    d_cnt.alloc((size_t)nfree * 3 * 8);
    if (!rec_lds) d_rec.alloc((size_t)grid * (size_t)bcap * reclen * 8);
    if (t.model == 2 && !wl) d_w.alloc((size_t)grid * (size_t)n * (size_t)(n | 1) * 8);

    auto fill = [&](auto& a) {
        a.n = t.n;
        a.ld = t.ld;
        a.ne = t.ne;
        a.l1 = t.l1;
        a.nfree = (int32_t)nfree;
        a.epochs = q.epochs;
        a.side = q.side;
        a.cap = fold_sweep_cap(q.max_sweeps);
        a.ldp = t.n | 1;
        a.rec_lds = rec_lds;
        a.bcap = bcap;
        a.batch = q.batch_size;
        a.count = q.count;
        a.lr = q.lr;
        a.margin = q.margin;
        a.h = d_h.as<int32_t>();
        a.t = d_t.as<int32_t>();
        a.unit_free = d_unit.as<int32_t>();
        a.free_ids = d_free.as<int32_t>();
        a.off = d_off.as<int64_t>();
        a.perm = d_perm.as<int32_t>();
        a.known = FilterView{d_slots.as<uint64_t>(), fs.mask, fs.nr, fs.ne};
        a.state = corrupt_mix(q.seed);
        a.rel_in = q.rel_in ? d_rin.as<double>() : nullptr;
        a.w_in = q.w_in ? d_win.as<double>() : nullptr;
        a.rel_out = d_rout.as<double>();
        a.w_out = t.model != 0 ? d_wout.as<double>() : nullptr;
        a.loss = d_loss.as<double>();
        a.counts = d_cnt.as<int64_t>();
        a.rec_scratch = rec_lds ? nullptr : d_rec.as<double>();
        a.w_scratch = t.model == 2 && !wl ? d_w.as<double>() : nullptr;
    };
    auto run = [&](auto tag) {
        using T = decltype(tag);
        FoldRelArgs<T> a{};
        fill(a);
        a.ent = (const T*)t.ent;
        a.rel = (T*)const_cast<void*>(t.rel);
        a.w = (T*)const_cast<void*>(t.w);
        a.w_mirror = t.model == 2 ? (T*)q.w_mirror : nullptr;
        if (t.model == 0) launch_rel_nc<T, 0, false>(a, grid, lds, t.stream);
        else if (t.model == 1) launch_rel_nc<T, 1, false>(a, grid, lds, t.stream);
        else if (wl) launch_rel_nc<T, 2, true>(a, grid, lds, t.stream);
        else launch_rel_nc<T, 2, false>(a, grid, lds, t.stream);
    };
    {
        Span sp(hooks, "foldrel");
        if (t.f64) run(double{});
        else run(float{});
        sp.end();
    }
    if (rel_out) HIPCHK(hipMemcpyAsync(rel_out, d_rout.p, (size_t)(nfree * n) * 8, hipMemcpyDeviceToHost, t.stream));
    if (w_out) HIPCHK(hipMemcpyAsync(w_out, d_wout.p, (size_t)(nfree * wlen) * 8, hipMemcpyDeviceToHost, t.stream));
    HIPCHK(hipMemcpyAsync(loss, d_loss.p, (size_t)nfree * 2 * 8, hipMemcpyDeviceToHost, t.stream));
    HIPCHK(hipMemcpyAsync(counts, d_cnt.p, (size_t)nfree * 3 * 8, hipMemcpyDeviceToHost, t.stream));
    HIPCHK(hipStreamSynchronize(t.stream));
}

}  // namespace kb2e
