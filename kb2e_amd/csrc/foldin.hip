// foldin.hip -- entity fold-in on the device.  Part of libkb2e.so
// (kb2e_fold_in_entities in engine.hip calls in here).
//
// With every row but the free entities' frozen, each free entity is an SGD
// problem of its own: its samples read frozen rows and its own row, and write
// its own row.  fold_kernel gives each free entity one unit -- one wave, alone
// in its workgroup -- for all passes.  The unit keeps the working row x (and
// the row under construction y) in registers, lane l holding the elements
// l + 64 c for c < NC = ceil(n / 64) (a compile-time 1, 2, 4 or 8), in FP64
// whatever the tables are; every sum over the row is a wave reduction
// (wave_sum).  Units never communicate: no flag, no spin wait, no barrier
// between workgroups.  A unit reads no row another unit writes, because a
// candidate draw that is a free entity is rejected and an example holds exactly
// one free entity; the rows are stored once, after the last pass.  So the
// result depends neither on the grid size (KB2E_FOLD_GRID=<workgroups>: tests)
// nor on the order of the units, which the host sorts by descending number of
// examples so that the longest chains start first.
//
// A sample.  The 32 candidate draws of a sample are made side by side, lane a - 1
// taking draw a; a ballot finds the first accepted one.  The rows of the
// positive's other entity o and of the drawn entity q are loaded beside x, and
// the three are turned into the model's "features" (TransE: the row; TransH:
// row - (w . row) w; TransR: row W_r), from which both energies and both
// gradient directions follow: d = feature(tail) - feature(head) - r.
//
// TransR.  The matrix of the sample's relation is staged into LDS (and kept
// while consecutive samples share the relation) when n (n | 1) + 4 n doubles fit
// the CU's 160 KiB, which holds up to n = 141.  The LDS row pitch is n | 1
// doubles: a column sum (lane = column k, W[j][k] for j ascending) reads
// consecutive addresses, and a row sum (lane = row j, W[j][k] for k ascending)
// reads addresses an odd number of doubles apart, which puts the 32 lanes of a
// ds_read_b64 group on 32 different bank pairs.  Above that width, or with
// KB2E_FOLD_W_L2=1, the matrix is read from global memory (L2) in both
// patterns.  Vectors that every lane needs (x, o, q for the projections, the
// direction g for the row update) go through four n-double LDS vectors.
//
// Every loop is bounded: the coupling loops by the sweep cap, the known-set
// probe by the table size.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

#include "classify_host.hpp"
#include "eval_shared.hpp"
#include "foldin.hpp"
#include "foldin_host.hpp"
#include "hip_util.hpp"
#include "kernels_common.hpp"

namespace kb2e {
namespace {

template <typename T>
struct FoldArgs {
    int32_t n, ld, ne, l1, nfree, epochs, side, cap, ldp;
    T* ent;
    const T* rel;
    const T* w;
    double lr, margin;
    const int32_t *h, *t, *r;
    const uint8_t* slot;  // by example: the slot the free entity fills
    int64_t count;
    const int32_t* unit_free;
    const int32_t* free_ids;
    const int64_t* off;
    const int32_t* perm;
    const uint64_t* bitmap;
    FilterView known;
    uint64_t state;  // corrupt_mix(seed)
    const double* rows_in;
    double* rows_out;
    double* loss;
    int64_t* counts;
};

// FilterView::has with the probe bounded by the table size
__device__ __forceinline__ bool fold_known(const FilterView& v, int64_t h, int64_t r, int64_t t) {
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
__device__ __forceinline__ void fold_load(const T* row, int n, double (&out)[NC]) {
    const int l = lane_id();
#pragma unroll
    for (int c = 0; c < NC; ++c) out[c] = l + 64 * c < n ? (double)row[l + 64 * c] : 0.0;
}

template <int NC>
__device__ __forceinline__ void fold_to_lds(double* v, int n, const double (&x)[NC]) {
    const int l = lane_id();
#pragma unroll
    for (int c = 0; c < NC; ++c)
        if (l + 64 * c < n) v[l + 64 * c] = x[c];
}

template <int NC>
__device__ __forceinline__ double fold_dot(const double (&a)[NC], const double (&b)[NC]) {
    double s = 0;
#pragma unroll
    for (int c = 0; c < NC; ++c) s += a[c] * b[c];  // (elements past n are zero)
    return wave_sum(s);
}

// W[j][k] of the staged (LDS, pitch ldp) or the stored (global, pitch ld) matrix
template <typename T, bool WL>
__device__ __forceinline__ double fold_w(const T* Wg, const double* Wl, int ld, int ldp, int j, int k) {
    if constexpr (WL) return Wl[j * ldp + k];
    else return (double)Wg[(int64_t)j * ld + k];
}

// Column sums of up to three vectors at once: p_k = sum_j W[j][k] v[j], j
// ascending from zero (transr/transr.cpp:20-25); lane = column.
template <typename T, int NC, bool WL, int NV>
__device__ __forceinline__ void fold_project(const T* Wg, const double* Wl, int n, int ld, int ldp, const double* v,
                                             double (&p)[NV][NC]) {
    const int l = lane_id();
#pragma unroll
    for (int q = 0; q < NV; ++q)
#pragma unroll
        for (int c = 0; c < NC; ++c) p[q][c] = 0;
    for (int j = 0; j < n; ++j) {
        double vj[NV];
#pragma unroll
        for (int q = 0; q < NV; ++q) vj[q] = v[q * n + j];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const int k = l + 64 * c;
            if (k < n) {
                const double w = fold_w<T, WL>(Wg, Wl, ld, ldp, j, k);
#pragma unroll
                for (int q = 0; q < NV; ++q) p[q][c] += w * vj[q];
            }
        }
    }
}

// scale to unit length: always, or (shrink) only a row longer than 1 (common/utils.cpp:70-77)
template <int NC>
__device__ __forceinline__ void fold_norm(double (&y)[NC], bool shrink) {
    const double len = sqrt(fold_dot(y, y));
    if (!shrink || len > 1.0) {
#pragma unroll
        for (int c = 0; c < NC; ++c) y[c] = y[c] / len;
    }
}

// MODEL 0 TransE, 1 TransH, 2 TransR; WL (TransR): the matrix is staged in LDS.
// Dynamic LDS (TransR): 4 vectors of n doubles, then [n][ldp] doubles if WL.
template <typename T, int MODEL, int NC, bool WL>
__global__ __launch_bounds__(64) void fold_kernel(FoldArgs<T> a) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int l = lane_id();
    const int n = a.n;
    double* const vec = lds;           // [0] x / y, [1] o, [2] q (one block: fold_project reads v[q * n + j])
    double* const vg = lds + 3 * n;    // the direction every row sum needs
    double* const Wl = lds + 4 * n;
    bool valid[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) valid[c] = l + 64 * c < n;

    for (int u = blockIdx.x; u < a.nfree; u += gridDim.x) {
        const int fi = a.unit_free[u];
        const int32_t f = a.free_ids[fi];
        double x[NC];
        if (a.rows_in) fold_load<double, NC>(a.rows_in + (int64_t)fi * n, n, x);
        else fold_load<T, NC>(a.ent + (int64_t)f * a.ld, n, x);
        const int64_t e0 = a.off[fi], e1 = a.off[fi + 1];
        int64_t active = 0, failed = 0, capped = 0;
        double loss_first = 0, loss_last = 0;
        int staged = -1;  // the relation whose matrix is in LDS

        for (int p = 0; p < a.epochs; ++p) {
            double lossp = 0;
            for (int64_t e = e0; e < e1; ++e) {
                const int32_t i = a.perm[e];
                const int32_t h = a.h[i], t = a.t[i], r = a.r[i];
                const int fslot = a.slot[i];
                // ---- slot and negative
                const uint64_t ctr = (uint64_t)p * (uint64_t)a.count + (uint64_t)i;
                const int cslot = a.side == 2 ? (int)(corrupt_u(a.state, ctr, 0) >> 63) : a.side;
                const int32_t old = cslot ? t : h;
                bool ok = false;
                int32_t cand = 0;
                if (l < kFoldDraws) {
                    cand = (int32_t)(corrupt_u(a.state, ctr, (uint64_t)(l + 1)) % (uint64_t)a.ne);
                    ok = !((a.bitmap[cand >> 6] >> (cand & 63)) & 1ull) && cand != old &&
                         !(cslot ? fold_known(a.known, h, r, cand) : fold_known(a.known, cand, r, t));
                }
                const uint64_t accepted = __ballot(ok);
                if (!accepted) {  // (wave-uniform)
                    ++failed;
                    continue;
                }
                const int32_t got = __shfl(cand, __ffsll((long long)accepted) - 1);
                const int32_t o = fslot ? h : t;  // the positive's other entity
                const bool f_in_neg = cslot != fslot;  // the corrupted triple still holds f

                // ---- features of x, o and q
                double xo[NC], xq[NC], rr[NC];
                fold_load<T, NC>(a.ent + (int64_t)o * a.ld, n, xo);
                fold_load<T, NC>(a.ent + (int64_t)got * a.ld, n, xq);
                fold_load<T, NC>(a.rel + (int64_t)r * a.ld, n, rr);
                double ft[3][NC];  // features of x, o, q
                double wr[NC];     // TransH: the normal
                const T* Wg = nullptr;
                if constexpr (MODEL == 0) {
#pragma unroll
                    for (int c = 0; c < NC; ++c) ft[0][c] = x[c], ft[1][c] = xo[c], ft[2][c] = xq[c];
                } else if constexpr (MODEL == 1) {
                    fold_load<T, NC>(a.w + (int64_t)r * a.ld, n, wr);
                    const double sx = fold_dot(wr, x), so = fold_dot(wr, xo), sq = fold_dot(wr, xq);
#pragma unroll
                    for (int c = 0; c < NC; ++c) {
                        ft[0][c] = x[c] - sx * wr[c];
                        ft[1][c] = xo[c] - so * wr[c];
                        ft[2][c] = xq[c] - sq * wr[c];
                    }
                } else {
                    Wg = a.w + (int64_t)r * n * a.ld;
                    wave_lds_sync();  // (earlier reads of the vectors and of the matrix are done)
                    if (WL && staged != r) {
                        for (int j = 0; j < n; ++j)
                            for (int k = l; k < n; k += 64) Wl[j * a.ldp + k] = (double)Wg[(int64_t)j * a.ld + k];
                        staged = r;
                    }
                    fold_to_lds<NC>(vec, n, x);
                    fold_to_lds<NC>(vec + n, n, xo);
                    fold_to_lds<NC>(vec + 2 * n, n, xq);
                    wave_lds_sync();
                    fold_project<T, NC, WL, 3>(Wg, Wl, n, a.ld, a.ldp, vec, ft);
                }

                // ---- energies: d = feature(tail) - feature(head) - r
                double dpos[NC], dneg[NC];
                double sp = 0, sn = 0;
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    const double ph = fslot ? ft[1][c] : ft[0][c], pt = fslot ? ft[0][c] : ft[1][c];
                    const double nh = cslot == 0 ? ft[2][c] : ph, nt = cslot == 1 ? ft[2][c] : pt;
                    dpos[c] = pt - ph - rr[c];
                    dneg[c] = nt - nh - rr[c];
                    if (valid[c]) {
                        sp += a.l1 ? fabs(dpos[c]) : dpos[c] * dpos[c];
                        sn += a.l1 ? fabs(dneg[c]) : dneg[c] * dneg[c];
                    }
                }
                const double epos = wave_sum(sp), eneg = wave_sum(sn);
                if (!(epos + a.margin > eneg)) continue;  // (wave-uniform)
                lossp += a.margin + epos - eneg;
                ++active;

                // ---- update: the positive with beta = -1, then the corrupted triple with +1
                double y[NC];
#pragma unroll
                for (int c = 0; c < NC; ++c) y[c] = x[c];
                for (int side = 0; side < 2; ++side) {
                    if (side == 1 && !f_in_neg) break;
                    const double coef = (side ? 1.0 : -1.0) * a.lr;
                    double g[NC];
#pragma unroll
                    for (int c = 0; c < NC; ++c) {
                        const double d = side ? dneg[c] : dpos[c];
                        g[c] = 2.0 * d;
                        if (a.l1) g[c] = g[c] > 0 ? 1.0 : -1.0;
                    }
                    if constexpr (MODEL != 2) {
#pragma unroll
                        for (int c = 0; c < NC; ++c)
                            if (valid[c]) y[c] = fslot ? y[c] + coef * g[c] : y[c] - coef * g[c];
                        fold_norm<NC>(y, true);
                    } else {
                        wave_lds_sync();
                        fold_to_lds<NC>(vg, n, g);
                        wave_lds_sync();
                        // lane = row j: y_j -+= (coef g_k) W[j][k], k ascending (transr/trainer.cpp:160-170)
                        for (int k = 0; k < n; ++k) {
                            const double cg = coef * vg[k];
#pragma unroll
                            for (int c = 0; c < NC; ++c) {
                                const int j = l + 64 * c;
                                if (j < n) {
                                    const double w = fold_w<T, WL>(Wg, Wl, a.ld, a.ldp, j, k);
                                    y[c] = fslot ? y[c] + cg * w : y[c] - cg * w;
                                }
                            }
                        }
                        fold_norm<NC>(y, false);
                    }
                    // ---- the coupling loop against the stored normal / matrix
                    if constexpr (MODEL == 1) {
                        int sweeps = 0;
                        while (fold_dot(wr, y) > 0.1) {
                            if (sweeps == a.cap) {
                                ++capped;
                                break;
                            }
#pragma unroll
                            for (int c = 0; c < NC; ++c) y[c] = y[c] - a.lr * wr[c];
                            ++sweeps;
                        }
                    } else if constexpr (MODEL == 2) {
                        int sweeps = 0;
                        while (true) {
                            double qv[1][NC];
                            wave_lds_sync();
                            fold_to_lds<NC>(vec, n, y);
                            wave_lds_sync();
                            fold_project<T, NC, WL, 1>(Wg, Wl, n, a.ld, a.ldp, vec, qv);
                            if (!(fold_dot(qv[0], qv[0]) > 1.0)) break;
                            if (sweeps == a.cap) {
                                ++capped;
                                break;
                            }
                            double q2[NC];
#pragma unroll
                            for (int c = 0; c < NC; ++c) q2[c] = 2.0 * qv[0][c];
                            wave_lds_sync();
                            fold_to_lds<NC>(vg, n, q2);
                            wave_lds_sync();
                            double s[NC];
#pragma unroll
                            for (int c = 0; c < NC; ++c) s[c] = 0;
                            for (int k = 0; k < n; ++k) {
                                const double qk = vg[k];
#pragma unroll
                                for (int c = 0; c < NC; ++c) {
                                    const int j = l + 64 * c;
                                    if (j < n) s[c] += qk * fold_w<T, WL>(Wg, Wl, a.ld, a.ldp, j, k);
                                }
                            }
#pragma unroll
                            for (int c = 0; c < NC; ++c) y[c] = y[c] - a.lr * s[c];
                            ++sweeps;
                        }
                    }
                }
#pragma unroll
                for (int c = 0; c < NC; ++c) x[c] = y[c];
            }
            if (p == 0) loss_first = lossp;
            if (p == a.epochs - 1) loss_last = lossp;
        }

        // ---- the row is rounded to the table's precision once, here
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const int k = l + 64 * c;
            if (k < n) {
                const T stored = (T)x[c];
                a.ent[(int64_t)f * a.ld + k] = stored;
                if (a.rows_out) a.rows_out[(int64_t)fi * n + k] = (double)stored;
            }
        }
        if (l == 0) {
            a.loss[(int64_t)fi * 2] = loss_first;
            a.loss[(int64_t)fi * 2 + 1] = loss_last;
            a.counts[(int64_t)fi * 3] = active;
            a.counts[(int64_t)fi * 3 + 1] = failed;
            a.counts[(int64_t)fi * 3 + 2] = capped;
        }
    }
}

template <typename T, int MODEL, int NC, bool WL>
void launch_fold(const FoldArgs<T>& a, unsigned grid, size_t lds, hipStream_t stream) {
    auto kernel = fold_kernel<T, MODEL, NC, WL>;
    if (lds > 48 * 1024) allow_lds(kernel, lds);
    kernel<<<grid, 64, lds, stream>>>(a);
    HIPCHK(hipGetLastError());
}

template <typename T, int MODEL, bool WL>
void launch_fold_nc(const FoldArgs<T>& a, unsigned grid, size_t lds, hipStream_t stream) {
    if (a.n <= 64) launch_fold<T, MODEL, 1, WL>(a, grid, lds, stream);
    else if (a.n <= 128) launch_fold<T, MODEL, 2, WL>(a, grid, lds, stream);
    else if (a.n <= 256) launch_fold<T, MODEL, 4, WL>(a, grid, lds, stream);
    else if constexpr (!WL) launch_fold<T, MODEL, 8, WL>(a, grid, lds, stream);
    else throw std::logic_error("fold-in: a staged matrix this wide");  // (the host never asks for it)
}

template <typename T>
void run_fold(const EvalTables& t, FoldArgs<T> a, unsigned grid) {
    a.ent = (T*)const_cast<void*>(t.ent);
    a.rel = (const T*)t.rel;
    a.w = (const T*)t.w;
    if (t.model == 0) return launch_fold_nc<T, 0, false>(a, grid, 0, t.stream);
    if (t.model == 1) return launch_fold_nc<T, 1, false>(a, grid, 0, t.stream);
    const size_t vecs = (size_t)4 * t.n * 8, staged = vecs + (size_t)t.n * a.ldp * 8;
    const char* l2 = getenv("KB2E_FOLD_W_L2");
    if (staged <= kLdsMax && !(l2 && atoi(l2) != 0)) return launch_fold_nc<T, 2, true>(a, grid, staged, t.stream);
    launch_fold_nc<T, 2, false>(a, grid, vecs, t.stream);
}

template <typename V>
void upload(DevBuf& d, const V* src, size_t count, hipStream_t stream) {
    d.alloc(count * sizeof(V));
    if (count) HIPCHK(hipMemcpyAsync(d.p, src, count * sizeof(V), hipMemcpyHostToDevice, stream));
}

}  // namespace

void fold_in_entities(const EvalTables& t, const FoldQuery& q, double* rows_out, double* loss, int64_t* counts,
                      const PredictHooks* hooks) {
    if (q.epochs < 1) throw std::invalid_argument("epochs must be at least 1");
    if (q.side < 0 || q.side > 2) throw std::invalid_argument("side must be 0 (head), 1 (tail) or 2 (a coin per sample)");
    if (q.max_sweeps < 0) throw std::invalid_argument("max_sweeps must not be negative");
    if (!loss || !counts) throw std::invalid_argument("loss and counts are required");
    const FoldPlan plan = plan_fold(q.free_entities, q.nfree, q.heads, q.tails, q.relations, q.count, q.kh, q.kt, q.kr,
                                    q.nknown, t.ne, t.nr);
    const FilterSet fs = fold_known_set(q.heads, q.tails, q.relations, q.count, q.kh, q.kt, q.kr, q.nknown, t.ne, t.nr);
    const int64_t nfree = q.nfree, n = t.n;

    HIPCHK(hipStreamSynchronize(t.stream));
    DevBuf d_free, d_h, d_t, d_r, d_slot, d_unit, d_off, d_perm, d_bitmap, d_slots, d_in, d_out, d_loss, d_cnt;
    upload(d_free, q.free_entities, (size_t)nfree, t.stream);
    upload(d_h, q.heads, (size_t)q.count, t.stream);
    upload(d_t, q.tails, (size_t)q.count, t.stream);
    upload(d_r, q.relations, (size_t)q.count, t.stream);
    upload(d_slot, plan.slot.data(), plan.slot.size(), t.stream);
    upload(d_unit, plan.unit_free.data(), plan.unit_free.size(), t.stream);
    upload(d_off, plan.off.data(), plan.off.size(), t.stream);
    upload(d_perm, plan.perm.data(), plan.perm.size(), t.stream);
    upload(d_bitmap, plan.bitmap.data(), plan.bitmap.size(), t.stream);
    upload(d_slots, fs.slots.data(), fs.slots.size(), t.stream);
    if (q.rows_in) upload(d_in, q.rows_in, (size_t)(nfree * n), t.stream);
    d_out.alloc((size_t)(nfree * n) * 8);
    d_loss.alloc((size_t)nfree * 2 * 8);
    d_cnt.alloc((size_t)nfree * 3 * 8);

    unsigned grid = (unsigned)nfree;
    if (const char* v = getenv("KB2E_FOLD_GRID")) {
        const long g = atol(v);
        if (g >= 1 && g < (long)grid) grid = (unsigned)g;
    }
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
        a.lr = q.lr;
        a.margin = q.margin;
        a.h = d_h.as<int32_t>();
        a.t = d_t.as<int32_t>();
        a.r = d_r.as<int32_t>();
        a.slot = d_slot.as<uint8_t>();
        a.count = q.count;
        a.unit_free = d_unit.as<int32_t>();
        a.free_ids = d_free.as<int32_t>();
        a.off = d_off.as<int64_t>();
        a.perm = d_perm.as<int32_t>();
        a.bitmap = d_bitmap.as<uint64_t>();
        a.known = FilterView{d_slots.as<uint64_t>(), fs.mask, fs.nr, fs.ne};
        a.state = corrupt_mix(q.seed);
        a.rows_in = q.rows_in ? d_in.as<double>() : nullptr;
        a.rows_out = d_out.as<double>();
        a.loss = d_loss.as<double>();
        a.counts = d_cnt.as<int64_t>();
    };
    {
        Span sp(hooks, "foldin");
        if (t.f64) {
            FoldArgs<double> a{};
            fill(a);
            run_fold<double>(t, a, grid);
        } else {
            FoldArgs<float> a{};
            fill(a);
            run_fold<float>(t, a, grid);
        }
        sp.end();
    }
    if (rows_out) HIPCHK(hipMemcpyAsync(rows_out, d_out.p, (size_t)(nfree * n) * 8, hipMemcpyDeviceToHost, t.stream));
    HIPCHK(hipMemcpyAsync(loss, d_loss.p, (size_t)nfree * 2 * 8, hipMemcpyDeviceToHost, t.stream));
    HIPCHK(hipMemcpyAsync(counts, d_cnt.p, (size_t)nfree * 3 * 8, hipMemcpyDeviceToHost, t.stream));
    HIPCHK(hipStreamSynchronize(t.stream));
}

}  // namespace kb2e
