// candidates.hip -- scoring and ranking against caller-supplied candidate
// lists on the device.  Part of libkb2e.so (kb2e_score_candidates and
// kb2e_rank_candidates in engine.hip call in here).
//
// A query is (entity e, relation r, side) and a list of entities; listing x
// stands for the triple (e, x, r) (side 1) or (x, e, r) (side 0), and its
// energy is kb2e_score_triples' for that triple, bit for bit: with P the
// evaluator's projection for r, d_k = (P(tail)_k - P(head)_k) - r_k, summed
// over k from zero as |d_k| or d_k * d_k -- the expressions of
// score_triples_kernel, score_triples_transr_kernel and eval_project_kernel.
//
// * plan_candidates (candidates_host.hpp) cuts the lists into work items of at
//   most 64 listings and the queries into chunks; an item carries its query,
//   so neither query arrays nor expanded triples go to the device, and a list
//   that many queries share is uploaded once.
// * candidates_kernel, one wave per work item, four items a workgroup: the
//   anchor's projected row and the relation row (TransH: and the normal) are
//   read once per item into the wave's LDS (a context's dim is at most 512:
//   48 KiB a workgroup at most), then every lane owns one listing and makes
//   the serial sum over k.  The listing's row is either streamed by
//   its lane with 16-byte loads (8-byte for FP32 tables) or staged by the whole
//   wave, a panel of kPanelK columns of the 64 rows at a time, into a padded
//   LDS tile (kPanel).  TransH computes w . x per listing inline, in a first
//   sweep over the row.  TransR reads projected columns PT[k][col(x)]: per
//   chunk and relation the distinct entities are projected once
//   (candidates_project_kernel, eval_project_kernel's sum) into a compact
//   table read through a remap, or the whole table with project_any where
//   they are at least half of |E|.
// * rank: items hold at most 63 listings and lane 63 scores the truth, so the
//   truth's energy is there without a pass of its own; every lane compares,
//   probes the filter only where its listing counts, and the wave's ballots
//   go to the query's four counters with one integer atomic each.  No energy
//   leaves the card.
//
// Everything of a call is queued on the tables' stream; there is one
// synchronisation, at the end.  No wave waits on another.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "candidates.hpp"
#include "candidates_host.hpp"
#include "eval_shared.hpp"
#include "hip_util.hpp"
#include "host_data.hpp"
#include "kernels_common.hpp"

namespace kb2e {
namespace {

constexpr int kCandWaves = 4;        // work items of a workgroup
constexpr int kCandMaxN = 512;       // the widest context (kb2e_create): the rows of an item fit LDS
constexpr int kPanelK = 16;          // columns of a staged panel
constexpr int kPanelLd = kPanelK + 1;  // its padded stride, in doubles

template <typename T>
struct CandArgs {
    int32_t n, ld, l1, nu;
    const T* ent;
    const T* rel;
    const T* w;
    const double* PT;      // TransR: [n][nu] projected columns
    const int32_t* remap;  // TransR: entity -> column (null: the entity itself)
    const int32_t* cand;   // the call's candidate array
    const CandItem* items;
    int32_t nitems;
    int32_t wave_doubles;  // LDS of a wave
    double* energy;        // score: the chunk's energies
    unsigned long long* cnt;  // rank: [nq][4] below raw, below filtered, counted raw, counted filtered
    int32_t probe_all;        // rank: counted is asked for (else only listings below the truth are probed)
    int32_t has_filter;
    FilterView fv;
    unsigned long long* probes;
};

template <typename T>
struct Pair;
template <>
struct Pair<double> {
    using type = double2;
};
template <>
struct Pair<float> {
    using type = float2;
};

template <typename T, int kModel, bool kPanel>
__global__ __launch_bounds__(256) void candidates_kernel(CandArgs<T> a) {
    static_assert(!(kPanel && kModel == 2), "TransR gathers projected columns");
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t it = (int64_t)blockIdx.x * kCandWaves + wv;
    if (it >= a.nitems) return;  // (wave-uniform; no workgroup barrier below)
    const CandItem I = a.items[it];
    const int n = a.n;
    const bool rank = a.cnt != nullptr;
    int x = a.cand[(int64_t)I.first + min(lane, I.count - 1)];
    if (rank && lane == 63) x = I.truth;

    double* pa = lds + (size_t)wv * a.wave_doubles;  // the anchor's projected row
    double* rv = pa + n;                             // the relation row
    double* wn = rv + n;                             // TransH: the normal
    double* tile = pa + (kModel == 1 ? 3 : 2) * n;   // kPanel: [64][kPanelLd]

    const T* er = a.ent + (int64_t)I.ent * a.ld;
    const T* rr = a.rel + (int64_t)I.rel * a.ld;
    const T* wr = kModel == 1 ? a.w + (int64_t)I.rel * a.ld : nullptr;
    double hs = 0;  // TransH: w . e
    if constexpr (kModel == 1)
        for (int k = 0; k < n; ++k) hs += (double)wr[k] * (double)er[k];
    int ce = 0, cx = 0;  // TransR: the columns of e and x
    if constexpr (kModel == 2) {
        ce = a.remap ? a.remap[I.ent] : I.ent;
        cx = a.remap ? a.remap[x] : x;
    }
    auto anchor = [&](int k) -> double {
        if constexpr (kModel == 0) return (double)er[k];
        else if constexpr (kModel == 1) return (double)er[k] - hs * (double)wr[k];
        else return a.PT[(int64_t)k * a.nu + ce];
    };
    for (int k = lane; k < n; k += 64) {
        pa[k] = anchor(k);
        rv[k] = (double)rr[k];
        if constexpr (kModel == 1) wn[k] = (double)wr[k];
    }
    wave_lds_sync();

    // step(k, v) for k = 0 .. n-1 in order, v = element k of entity x's row
    const T* xr = a.ent + (int64_t)x * a.ld;
    auto sweep = [&](auto&& step) {
        if constexpr (kPanel) {
            for (int k0 = 0; k0 < n; k0 += kPanelK) {
                const int kp = min(kPanelK, n - k0);
                const int kk = lane & (kPanelK - 1);
#pragma unroll 4
                for (int i = 0; i < 64 * kPanelK / 64; ++i) {
                    const int row = i * (64 / kPanelK) + (lane / kPanelK);
                    const int xrow = __shfl(x, row);
                    tile[row * kPanelLd + kk] = kk < kp ? (double)a.ent[(int64_t)xrow * a.ld + k0 + kk] : 0.0;
                }
                wave_lds_sync();
                for (int j = 0; j < kp; ++j) step(k0 + j, tile[lane * kPanelLd + j]);
                wave_lds_sync();
            }
        } else {
            using P2 = typename Pair<T>::type;
            int k = 0;
            for (; k + 2 <= n; k += 2) {  // (ld is even: the pair is aligned and inside the row)
                const P2 v = *(const P2*)(xr + k);
                step(k, (double)v.x);
                step(k + 1, (double)v.y);
            }
            if (k < n) step(k, (double)xr[k]);
        }
    };

    double e = 0;
    auto term = [&](int k, double px) {
        const double pe = pa[k];
        const double pt = I.side ? px : pe, ph = I.side ? pe : px;
        const double d = pt - ph - rv[k];
        e += (kModel == 1 || a.l1) ? fabs(d) : d * d;
    };
    if constexpr (kModel == 0) {
        sweep(term);
    } else if constexpr (kModel == 1) {
        double xs = 0;
        sweep([&](int k, double v) { xs += wn[k] * v; });
        sweep([&](int k, double v) { term(k, v - xs * wn[k]); });
    } else {
        for (int k = 0; k < n; ++k) term(k, a.PT[(int64_t)k * a.nu + cx]);
    }

    if (!rank) {
        if (lane < I.count) a.energy[(int64_t)I.out + lane] = e;
        return;
    }
    const uint64_t key = (uint64_t)__double_as_longlong(e);
    const uint64_t tkey = (uint64_t)__double_as_longlong(__shfl(e, 63));
    const bool counts = lane < I.count && x != I.truth;
    const bool below = counts && key < tkey;
    const bool probe = a.has_filter && (a.probe_all ? counts : below);
    bool known = false;
    if (probe) known = I.side ? a.fv.has(I.ent, I.rel, x) : a.fv.has(x, I.rel, I.ent);  // (head, relation, tail)
    const uint64_t b0 = __ballot(below), b1 = __ballot(below && !known);
    const uint64_t c0 = __ballot(counts), c1 = __ballot(counts && !known), np = __ballot(probe);
    if (lane == 0) {
        unsigned long long* c = a.cnt + (int64_t)I.query * 4;
        if (b0) atomicAdd(c + 0, (unsigned long long)__popcll(b0));
        if (b1) atomicAdd(c + 1, (unsigned long long)__popcll(b1));
        if (c0) atomicAdd(c + 2, (unsigned long long)__popcll(c0));
        if (c1) atomicAdd(c + 3, (unsigned long long)__popcll(c1));
        if (np) atomicAdd(a.probes, (unsigned long long)__popcll(np));
    }
}

template <typename T>
struct CandProjArgs {
    int32_t n, ld, nu, r;
    const T* ent;
    const T* w;
    const int32_t* ents;  // [nu] the group's distinct entities
    double* PT;           // [n][nu]
    int32_t* remap;       // [ne]: remap[ents[u]] = u
};

// TransR.  grid.x: blocks of 256 listed entities; grid.y: the output k.  A
// thread makes eval_project_kernel's sum for (ents[u], k): over j in order from
// zero, the matrix element at a workgroup-uniform address.
template <typename T>
__global__ __launch_bounds__(256) void candidates_project_kernel(CandProjArgs<T> a) {
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= a.nu) return;
    const int k = blockIdx.y;
    const int x = a.ents[u];
    const T* e = a.ent + (int64_t)x * a.ld;
    const T* W = a.w + (int64_t)a.r * a.n * a.ld;
    double s = 0;
    for (int j = 0; j < a.n; ++j) s += (double)W[(int64_t)j * a.ld + k] * (double)e[j];
    a.PT[(int64_t)k * a.nu + u] = s;
    if (k == 0) a.remap[x] = u;
}

// ------------------------------------------------------------ host side

enum class Rows { kStream, kPanel };

const char* env_str(const char* name) {
    const char* v = getenv(name);
    return v ? v : "";
}

template <typename T, int kModel>
void launch_items(const EvalTables& t, CandArgs<T> a, Rows rows) {
    if (t.n > kCandMaxN) throw Unsupported("candidate lists: dim above " + std::to_string(kCandMaxN));
    const bool panel = kModel != 2 && rows == Rows::kPanel;
    a.wave_doubles = (kModel == 1 ? 3 : 2) * t.n + (panel ? 64 * kPanelLd : 0);
    const size_t lds = (size_t)kCandWaves * a.wave_doubles * 8;
    const unsigned grid = (unsigned)((a.nitems + kCandWaves - 1) / kCandWaves);
    auto go = [&](auto kernel) {
        allow_lds(kernel, lds);
        kernel<<<grid, 64 * kCandWaves, lds, t.stream>>>(a);
        HIPCHK(hipGetLastError());
    };
    if constexpr (kModel == 2) {
        go(candidates_kernel<T, 2, false>);
    } else {
        if (panel) go(candidates_kernel<T, kModel, true>);
        else go(candidates_kernel<T, kModel, false>);
    }
}

template <typename T>
void run(const EvalTables& t, const CandidatesQuery& q, double* energy, int64_t* ranks, int64_t* counted,
         CandidatesStats* stats, const PredictHooks* hooks) {
    const bool rank = ranks != nullptr;
    check_candidates(q.ent, q.rel, q.side, q.truth, q.lists, q.nq, q.offsets, q.candidates, q.nlists, t.ne, t.nr);
    if (q.nq > INT32_MAX) throw std::invalid_argument("too many queries in one call");
    const int64_t total = q.offsets[q.nlists];

    // the filter set (FilterSet, as the evaluator's filter)
    FilterSet fs;
    DevBuf d_slots, d_cnt, d_probes;
    if (rank) {
        std::vector<int32_t> H(q.fh, q.fh + q.nfilter), T_(q.ft, q.ft + q.nfilter), R(q.fr, q.fr + q.nfilter);
        for (int64_t k = 0; k < q.nfilter; ++k)
            if (H[k] < 0 || H[k] >= t.ne || T_[k] < 0 || T_[k] >= t.ne || R[k] < 0 || R[k] >= t.nr)
                throw std::invalid_argument("filter triple out of range");
        fs.build(H, T_, R, t.ne, t.nr);
        d_slots.alloc(fs.slots.size() * 8);
        HIPCHK(hipMemcpyAsync(d_slots.p, fs.slots.data(), fs.slots.size() * 8, hipMemcpyHostToDevice, t.stream));
        d_cnt.alloc((size_t)q.nq * 4 * 8);
        d_probes.alloc(8);
    }

    const char* cs = getenv("KB2E_CANDIDATES_CHUNK");
    const int64_t cap = cs && atoll(cs) > 0 ? atoll(cs) : kCandidatesChunkListings;
    const bool transr = t.model == 2;
    const CandPlan plan = plan_candidates(q.ent, q.rel, q.side, rank ? q.truth : nullptr, q.lists, q.nq, q.offsets,
                                          q.candidates, t.ne, t.nr, rank ? kCandidatesWave - 1 : kCandidatesWave, cap,
                                          transr);
    const std::string force = env_str("KB2E_CANDIDATES_PROJECT");
    if (!force.empty() && force != "compact" && force != "full")
        throw std::invalid_argument("KB2E_CANDIDATES_PROJECT must be compact or full");
    auto full = [&](const CandGroup& g) {
        return force == "full" || (force.empty() && g.nents * 2 >= (int64_t)t.ne);
    };
    const std::string rs = env_str("KB2E_CANDIDATES_ROWS");
    if (!rs.empty() && rs != "stream" && rs != "panel")
        throw std::invalid_argument("KB2E_CANDIDATES_ROWS must be stream or panel");
    const Rows rows = rs == "panel" ? Rows::kPanel : Rows::kStream;

    DevBuf d_cand, d_items, d_energy, d_PT, d_relv, d_remap, d_ents;
    d_cand.alloc((size_t)total * 4);
    if (total > 0) HIPCHK(hipMemcpyAsync(d_cand.p, q.candidates, (size_t)total * 4, hipMemcpyHostToDevice, t.stream));
    d_items.alloc((size_t)plan.max_items * sizeof(CandItem));
    if (!rank) d_energy.alloc((size_t)plan.max_listings * 8);
    if (transr) {
        int64_t cols = 0;
        for (const CandGroup& g : plan.groups) cols = std::max<int64_t>(cols, full(g) ? t.ne : g.nents);
        d_PT.alloc((size_t)t.n * cols * 8);
        d_relv.alloc((size_t)t.n * 8);
        d_remap.alloc((size_t)t.ne * 4);
        d_ents.alloc((size_t)plan.max_distinct * 4);
    }

    CandidatesStats st;
    const char* family = rank ? "candidates_rank" : "candidates_score";
    for (const CandChunk& c : plan.chunks) {
        ++st.chunks;
        if (c.nitems == 0) continue;
        HIPCHK(hipMemcpyAsync(d_items.p, plan.items.data() + c.item0, (size_t)c.nitems * sizeof(CandItem),
                              hipMemcpyHostToDevice, t.stream));
        for (int64_t gi = c.group0; gi < c.group0 + c.ngroups; ++gi) {
            const CandGroup& g = plan.groups[(size_t)gi];
            CandArgs<T> a{};
            a.n = t.n;
            a.ld = t.ld;
            a.l1 = t.l1;
            a.ent = (const T*)t.ent;
            a.rel = (const T*)t.rel;
            a.w = (const T*)t.w;
            a.cand = d_cand.as<int32_t>();
            a.items = d_items.as<CandItem>() + (g.item0 - c.item0);
            a.nitems = (int32_t)g.nitems;
            a.energy = d_energy.as<double>();
            a.cnt = rank ? d_cnt.as<unsigned long long>() : nullptr;
            a.probe_all = counted != nullptr;
            a.has_filter = q.nfilter > 0;
            a.fv = FilterView{d_slots.as<uint64_t>(), fs.mask, (uint64_t)t.nr, (uint64_t)t.ne};
            a.probes = d_probes.as<unsigned long long>();
            if (transr) {
                Span sp(hooks, "candidates_project");
                if (full(g)) {
                    project_any(t, g.rel, d_PT.as<double>(), d_relv.as<double>());
                    a.nu = t.ne;
                    a.remap = nullptr;
                } else {
                    HIPCHK(hipMemcpyAsync(d_ents.p, plan.distinct.data() + g.ent0, (size_t)g.nents * 4,
                                          hipMemcpyHostToDevice, t.stream));
                    CandProjArgs<T> pa{t.n, t.ld, (int32_t)g.nents, g.rel, (const T*)t.ent, (const T*)t.w,
                                       d_ents.as<int32_t>(), d_PT.as<double>(), d_remap.as<int32_t>()};
                    candidates_project_kernel<T><<<dim3((unsigned)((g.nents + 255) / 256), (unsigned)t.n), 256, 0, t.stream>>>(pa);
                    HIPCHK(hipGetLastError());
                    a.nu = (int32_t)g.nents;
                    a.remap = d_remap.as<int32_t>();
                }
                a.PT = d_PT.as<double>();
                ++st.projections;
                sp.end();
            }
            Span sp(hooks, family);
            if (t.model == 0) launch_items<T, 0>(t, a, rows);
            else if (t.model == 1) launch_items<T, 1>(t, a, rows);
            else launch_items<T, 2>(t, a, rows);
            sp.end();
        }
        if (!rank)
            HIPCHK(hipMemcpyAsync(energy + c.out0, d_energy.p, (size_t)c.listings * 8, hipMemcpyDeviceToHost, t.stream));
        st.items += c.nitems;
        st.listings += c.listings;
    }
    std::vector<unsigned long long> cnt;
    unsigned long long probes = 0;
    if (rank) {
        cnt.resize((size_t)q.nq * 4);
        HIPCHK(hipMemcpyAsync(cnt.data(), d_cnt.p, cnt.size() * 8, hipMemcpyDeviceToHost, t.stream));
        HIPCHK(hipMemcpyAsync(&probes, d_probes.p, 8, hipMemcpyDeviceToHost, t.stream));
    }
    HIPCHK(hipStreamSynchronize(t.stream));
    if (rank) {
        for (int64_t x = 0; x < q.nq; ++x) {
            ranks[x * 2] = 1 + (int64_t)cnt[(size_t)x * 4];
            ranks[x * 2 + 1] = 1 + (int64_t)cnt[(size_t)x * 4 + 1];
            if (counted) {
                counted[x * 2] = (int64_t)cnt[(size_t)x * 4 + 2];
                counted[x * 2 + 1] = (int64_t)cnt[(size_t)x * 4 + 3];
            }
        }
        st.probes = (int64_t)probes;
    }
    if (stats) *stats = st;
}

}  // namespace

void score_candidates(const EvalTables& t, const CandidatesQuery& q, double* energy, CandidatesStats* stats,
                      const PredictHooks* hooks) {
    if (t.f64) run<double>(t, q, energy, nullptr, nullptr, stats, hooks);
    else run<float>(t, q, energy, nullptr, nullptr, stats, hooks);
}

void rank_candidates(const EvalTables& t, const CandidatesQuery& q, int64_t* ranks, int64_t* counted,
                     CandidatesStats* stats, const PredictHooks* hooks) {
    if (t.f64) run<double>(t, q, nullptr, ranks, counted, stats, hooks);
    else run<float>(t, q, nullptr, ranks, counted, stats, hooks);
}

}  // namespace kb2e
