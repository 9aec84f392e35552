// kernels_transr_pipe.hpp -- the per-relation sequential transRNorm of the
// PARALLEL TransR schedule (kernels_transr_seq.hpp explains the semantics:
// every pair against the matrix the relation's earlier pairs left,
// transr/trainer.cpp:35-64, :185-187; CPU model oracle/parallel.py
// transr_constraint, cons="chunk1"), software-pipelined across chunks.
//
// transr_cons_chain_kernel spends a chunk of 32 pairs as: all four waves make
// P = A W_c and the Gram matrix (MFMA), barrier, wave 0 walks the violators,
// barrier, all waves fold the violators into W_c, barrier -- the projections
// of a chunk wait for the previous chunk's walk.  Here the three other waves
// make the NEXT chunk's projections while wave 0 walks the current one:
//   X_{k+1} = A_{k+1} W_{k-1}                  (the matrix before chunk k's walk)
//   C       = A_{k+1} A_k^T                    (cross Gram, next x current)
//   P_{k+1} = X_{k+1} - lr C[:, vio_k] G_k     (chunk k's shrinks, W_k = W_{k-1} - lr A_k^T G_k)
// so after the walk only a rank-|vio_k| correction and the next chunk's |p|^2
// sit between two walks.  The working matrix W_c lives in registers of waves
// 1-3 as the MFMA B fragments of their column slices (slice cb on wave
// 1 + cb % 3), so X's tiles read no B operand from LDS, and chunk k's update
// W_c -= lr A_k^T G_k is made by waves 1-3 at the start of chunk k+1, while wave
// 0 walks chunk k+1, instead of between the two walks (a wave touches only its
// own slices' columns of the P buffers, so reading G_k and writing X_{k+2} into
// the same buffer need no barrier).  The walk keeps the chunk's projection
// rows in registers (lane j: half l >> 5 of row j & 31), so a violator's
// rank-1 move of the later rows is FMAs on registers with the violator's G row
// read as LDS broadcasts.  That update also writes the moved rows back, so the
// chunk's rows in LDS stay current and a violator's row is read for V = p_v K0 as
// it stands (broadcast reads, no row move between the pick and V), in small groups
// with a group's FMAs under the next group's reads: the staging registers stay few
// and K0's column never leaves the arch VGPRs.  (Taking p_v by v_readlane from the
// two lanes that hold the row instead was measured and lost: 104 readlanes cost
// 1.1k cycles a violator against 0.33k for the LDS form.)
// The walker's only stores are to LDS: the rows, the violator's G row, its vl entry
// and the publish word.  Everything of a chunk that goes to global memory -- the
// violators' pair records G, their vio slots, the chunk's pair flags -- is written
// by the helper waves from the published G rows (chunk_outputs), so the walker's
// release store waits on no global store.  The relation's last-update chunk starts
// after W_c's rows are renormalised: its projections are then made afresh (all
// waves).  The KB2E_RPAR_STATS counters are a template parameter: the product
// instantiation has no stamp code.  Beside the phases of the walk they stamp what lies
// outside the violator loop (hot relations, g_seq_stats 52..68): a window's set-up apart
// from the per-chunk "chunk start", the walker's wait at the chunk barrier B1 by the
// chunk's violator count, helper wave 1's work between helper_sync and B1 without its
// polling (row staging, corrections, what follows the walk's end), and the record pass on
// wave 0 (pipe_records).
// RParBufs::pipe_opt (KB2E_RPAR_PIPE_OPT, read at every batch; 0: the path before) switches
// the chunk hand-over step, kPipeOptHandover: the next chunk's rows read once ahead of the
// helpers' polling, no rewriting of the always-zero |p|^2 partials, the pair flags stored
// after B1, the helpers' tiles with all their LDS reads ahead of the MFMAs, the debt with two
// violators' reads in flight; kPipeOptDefer: a relation of bf.rec_defer chunks or more runs no
// record pass -- its G rows stay in the record tables under the relation's stamp (bf.rec_stamp)
// and the entity pass, the next launch, makes da from them on the waves that add it
// (rpar_record_convert, kernels_transr_parallel.hpp: the hottest relation's ~100 records no longer
// queue on four waves behind its chain); kPipeOptPublish: the walker publishes a violator right
// behind its G row, ahead of the later rows' update, so the helpers' correction runs under that
// update.  Loads and stores move; every sum keeps its operands and order, so all paths give the
// same bits (tests/test_gpu_transr_pipe_outside.py, tests/test_gpu_transr_pipe_defer.py).
#pragma once

#include <type_traits>

#include "kernels_transr_cons.hpp"  // pair_sum32
#include "kernels_transr_seq.hpp"

namespace kb2e {

constexpr int kPipeList = 1536;  // pairs of one relation a window (entity and slot lists in LDS)

// LDS (elements of T): W_c [NP][L] (W' for K0; the final matrix for the records) |
// A [3][R][L] | P [2][R][L] (K0 [NP][L] in the prologue) | Gram [2][R][LG] | cross
// Gram [R][LG] | |p|^2 partials [4][R] | row partials [4][NP]; ints: pair entities,
// slots [kPipeList] each | pre [kSeqMaxTiles + 1] | misc [8] | the violators of the
// last two chunks [2][R]
template <typename T>
__host__ __device__ constexpr size_t pipe_lds(int n) {
    return sizeof(T) * ((size_t)rm_np(n) * rm_ld(n) + 5 * (size_t)kChainRows * rm_ld(n) +
                        3 * (size_t)kChainRows * (kChainRows + 1) + 4 * kChainRows + 4 * (size_t)rm_np(n)) +
           sizeof(int) * (size_t)(2 * kPipeList + kSeqMaxTiles + 1 + 8 + 2 * kChainRows);
}

constexpr int kRecGroup = 32;  // G rows a wave has in flight from global memory (pipe_records: one round of
                               // loads for the hottest relation's ~25 records a wave)
constexpr int kRecReads = 8;   // 16-byte LDS reads of a staged G row a group (two groups in flight)

// The relation's pair records G -> da = -lr W G with its final matrix
// (transr/trainer.cpp:59-60; first order in lr the same as the matrix at the
// pair's chunk), at the end of its chain: the nvt violator slots in vio (written
// during the chain), W_c in LDS (stride L).  (Made here, the records of the ~440
// relations that finish early overlap the hottest relation's chain instead of
// following it in a kernel of their own.)  W_c's row is the same for every record of
// the relation: lane j takes row j of the final W_c into registers once (the
// walker's K0 column and the helpers' W_c fragments are dead by now), and a wave
// stages its records' G rows a stage-full at a time -- kRecGroup global loads in
// flight a lane, then LDS -- in the A slots and P buffers the walk left (`stage`,
// STAGE elements: a quarter a wave; `slots`: the wave's record slots, the window
// lists' space).  A record is then NP / 2 16-byte LDS reads that every lane makes at
// the same address (no bank conflicts) and NP FMAs: the four chains by i mod 4 over
// i = 0 .. NP - 1, (acc0 + acc1) + (acc2 + acc3), then -lr da (no other order: the
// records are compared bit for bit across changes of this pass).  Wave
// w takes records w, w + 4, ...; nothing here needs a workgroup barrier.  The first
// nslist violator slots are also in LDS (slist, written beside vio during the chain),
// which saves the hottest relation a round trip to global memory.  bf.rec_cap
// (tests): fewer records a stage-full, so small relations take several.
// STATS: wave 0's stamps of the pass into ph[0..4] (thread 0: W_c's row to registers, the
// slot lists, the issue of the G-row loads, their arrival + the staging stores, the record
// loops)
template <typename T, int NP, int L, int STAGE, bool STATS>
__device__ __forceinline__ void pipe_records(const RParArgs& a, const RParBufs<T>& bf, int r, const int32_t* vio,
                                             int nvt, const T* Wc, T* stage, int* slots, const int* slist,
                                             int nslist, unsigned long long* ph) {
    typedef T T2 __attribute__((ext_vector_type(2)));
    constexpr int NW = kChainThreads / kWave;
    constexpr int CAPW = STAGE / (NW * NP);  // records a wave stages at a time
    static_assert(CAPW >= 1 && NW * CAPW <= kPipeList, "the record slots borrow a window list");
    static_assert(NP % 4 == 0 && (L * sizeof(T)) % 16 == 0 && (NP * sizeof(T)) % 16 == 0, "16-byte LDS reads");
    const int n = a.n, ld = a.ld, w = threadIdx.x >> 6, l = lane_id();
    const int nmine = nvt > w ? (nvt - w + NW - 1) / NW : 0;  // records w, w + NW, ...
    if (nmine == 0) return;
    long long tq = STATS ? clock64() : 0;
    auto tick = [&](int k) {
        if constexpr (STATS) {
            if (threadIdx.x == 0) {
                const long long t = clock64();
                ph[k] += (unsigned long long)(t - tq);
                tq = t;
            }
        }
    };
    const int capw = bf.rec_cap >= NW && bf.rec_cap < NW * CAPW ? bf.rec_cap / NW : CAPW;
    T* gs = stage + w * (CAPW * NP);
    int* sl = slots + w * CAPW;
    auto row_of = [&](int s) { return s >= 0 ? bf.pair + (int64_t)s * ld : bf.relpair + (int64_t)r * ld; };
    T wr[NP];  // row j of the final matrix
    {
        const T2* w2 = (const T2*)(Wc + (l < NP ? l : 0) * L);
#pragma unroll
        for (int q = 0; q < NP / 2; ++q) {
            const T2 x = w2[q];
            wr[2 * q] = x.x;
            wr[2 * q + 1] = x.y;
        }
    }
    if constexpr (STATS) {
        T sink = T(0);  // (the row has arrived)
#pragma unroll
        for (int q = 0; q < NP; ++q) sink += wr[q];
        asm volatile("" ::"v"(sink));
    }
    tick(0);
    for (int m0 = 0; m0 < nmine; m0 += capw) {
        const int cnt = nmine - m0 < capw ? nmine - m0 : capw;
        for (int i = l; i < cnt; i += kWave) {
            const int k = w + NW * (m0 + i);
            sl[i] = k < nslist ? slist[k] : vio[k];
        }
        wave_lds_sync();
        tick(1);
        for (int i0 = 0; i0 < cnt; i0 += kRecGroup) {
            // the group's slots as wave-uniform values (one LDS read; past the end the last
            // record's again, so the loads and the LDS stores need no branches)
            const int iu = i0 + (l & (kRecGroup - 1));
            const int sv = sl[iu < cnt ? iu : cnt - 1];
            T g[kRecGroup];
#pragma unroll
            for (int u = 0; u < kRecGroup; ++u) g[u] = row_of(__builtin_amdgcn_readlane(sv, u))[l < n ? l : 0];
            if constexpr (STATS) {
                __builtin_amdgcn_sched_barrier(0);
                tick(2);
                __builtin_amdgcn_sched_barrier(0);
            }
            if (l < NP) {
#pragma unroll
                for (int u = 0; u < kRecGroup; ++u)
                    gs[(i0 + u < cnt ? i0 + u : cnt - 1) * NP + l] = l < n ? g[u] : T(0);
            }
            tick(3);
        }
        wave_lds_sync();
        // A record's staged row in groups of kRecReads reads, LA groups in flight across
        // the records (the next record's first groups are read under this one's last
        // FMAs; after the last record the same row again), so the LDS, which the four
        // waves share, stays busy: all NP / 2 reads of a record at once would take the
        // registers that hold W_c's row and leave the LDS idle during the FMAs.
        constexpr int NG = (NP / 2 + kRecReads - 1) / kRecReads, LA = NG >= 2 ? 2 : 1;
        T2 gr[NP / 2];
        auto g_load = [&](int i, int gq) {
            const T2* g2 = (const T2*)(gs + i * NP);
#pragma unroll
            for (int q = gq * kRecReads; q < (gq + 1) * kRecReads && q < NP / 2; ++q) gr[q] = g2[q];
        };
#pragma unroll
        for (int gq = 0; gq < LA; ++gq) g_load(0, gq);
        for (int i = 0; i < cnt; ++i) {
            T* row = row_of(sl[i]);
            const int inext = i + 1 < cnt ? i + 1 : i;
            T acc[4] = {T(0), T(0), T(0), T(0)};
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int gq = 0; gq < NG; ++gq) {
#pragma unroll
                for (int q = gq * kRecReads; q < (gq + 1) * kRecReads && q < NP / 2; ++q) {
                    acc[(2 * q) & 3] = fma(wr[2 * q], gr[q].x, acc[(2 * q) & 3]);
                    acc[(2 * q + 1) & 3] = fma(wr[2 * q + 1], gr[q].y, acc[(2 * q + 1) & 3]);
                }
                __builtin_amdgcn_sched_barrier(0);
                if (gq + LA < NG) g_load(i, gq + LA);
                else g_load(inext, gq + LA - NG);
                __builtin_amdgcn_sched_barrier(0);
            }
            T da = (acc[0] + acc[1]) + (acc[2] + acc[3]);
            asm volatile("" : "+v"(da));  // (keeps the FMAs out of the store's lane branch, between the reads)
            if (l < n) row[l] = -(T)a.lr * da;
        }
        wave_lds_sync();  // (every lane has read the staged rows before the next stage-full lands)
        tick(4);
    }
}

// STATS: the KB2E_RPAR_STATS instantiation (cycle stamps of the phases, violator and
// round counts); the product kernel carries none of it
template <typename T, int KS, bool STATS>
__global__ __launch_bounds__(kChainThreads) void transr_cons_pipe_kernel(RParArgs a, RParBufs<T> bf) {
    using M = Mfma16<T>;
    static_assert(sizeof(T) == 8, "the D-row / k-step identity below is the FP64 fragment layout");
    constexpr int NB = (4 * KS + 15) / 16;  // column slices of 16
    constexpr int NP = 16 * NB, L = NP + 2, R = kChainRows, LG = R + 1;
    constexpr int NH = 2 * KS;              // columns of a row half (walk registers; 4 KS >= n, the rest zero)
    constexpr int NSW = (NB + 2) / 3;       // column slices a helper wave owns (slice cb: wave 1 + cb % 3)
    static_assert(2 * R * L >= NP * L, "the K0 image borrows the two P buffers");
    static_assert(NSW * KS <= 4 * KS, "the helpers' slices share the walk's K0 registers");
    const int t0 = a.batch_t0[a.batch], t1 = a.batch_t0[a.batch + 1];
    int g0, r;  // the relation's first tile within the batch
    if (!chain_first_tile(a, t0, t1, g0, r)) return;
    const int n = a.n, ld = a.ld;
    const int w = threadIdx.x >> 6, l = lane_id(), kq = l >> 4, l16 = l & 15;
    const bool mine = w < NB;  // this wave computes a column slice of K0
    const int col = 16 * w + l16;
    const int hw = w - 1;      // helper wave index (waves 1-3)
    const T lr = (T)a.lr;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    T* Wc = (T*)smem;
    T* Abuf = Wc + NP * L;      // [3][R][L] entity rows of chunks k, k+1, k+2
    T* Pbuf = Abuf + 3 * R * L;  // [2][R][L] projections (then the violators' G rows) of chunks k, k+1
    T* Gbuf = Pbuf + 2 * R * L;  // [2][R][LG] Gram matrices A A^T of chunks k, k+1
    T* Cx = Gbuf + 2 * R * LG;   // [R][LG] A_{k+1} A_k^T (correct_q; unused since the dots are made on the fly)
    int* slist = (int*)Cx;       // ... so it holds the relation's first kSlist violator slots for pipe_records
    constexpr int kSlist = 2 * R * LG;
    T* qpart = Cx + R * LG;      // [4][R] |p_j|^2 partials of the column slices (next chunk)
    T* rp = qpart + 4 * R;       // [4][NP] row partials of the tail renorm
    int* pe = (int*)(rp + 4 * NP);
    int* ps = pe + kPipeList;
    int* pre = ps + kPipeList;
    int* misc = pre + kSeqMaxTiles + 1;
    int* vlist = misc + 8;  // [2][R] the chunks' violators in order, by chunk parity (misc[2]: the count)
    const long long ck0 = STATS ? clock64() : 0;
    int n_chunks = 0;
    unsigned long long n_vio = 0, n_rounds = 0, max_m = 0;
    constexpr int kPh = 40;
    __shared__ unsigned long long ph[STATS ? kPh : 1];  // (LDS, not forty 64-bit registers)
    if (STATS && threadIdx.x < kPh) ph[threadIdx.x] = 0;
    __shared__ long long pubt[STATS ? kChainRows : 1];  // (STATS: thread 0's clock at a violator's publish)
    long long tq = ck0, dtq = 0;
    // (phases 12..15 on thread 64, helper wave 1: debt, tiles, helper_sync wait, rows +
    // corrections incl. the wait for the walk's end; 16..19 on thread 0, what follows the
    // chunk loop: a window's last debt + barrier, the helpers' slices to LDS + barrier,
    // the records, the W write-back.  20 on thread 0: a window's set-up (tile prefix, list
    // build, the first row loads, chunk 0 afresh), which phase 1 held before; 21..24 the B1
    // wait of thread 0 by the chunk's violators (0, 1-2, 3-5, 6+), 25..28 those chunks; 29..31
    // on thread 64 with a clock of their own, between helper_sync and B1 without the
    // polling: what follows the walk's end (flags, P_n back, |p|^2), the row staging and
    // the P_n loads, the violators' corrections and outputs; 32..36 wave 0's record pass,
    // pipe_records; 37, 38 on thread 64: from the walker's publish of a violator to the end of
    // its correction, and those violators)
    auto tick = [&](int k) {
        if constexpr (STATS) {
            if (threadIdx.x == ((k >= 12 && k < 16) || k == 5 ? 64u : 0u)) {
                const long long t = clock64();
                dtq = t - tq;
                ph[k] += (unsigned long long)dtq;
                tq = t;
            }
        }
    };
    // the hand-over steps (RParBufs::pipe_opt; wave-uniform)
    const bool o_hand = (bf.pipe_opt & kPipeOptHandover) != 0;
    const bool o_defer = (bf.pipe_opt & kPipeOptDefer) != 0 && bf.rec_stamp != nullptr;
    const bool o_pub = (bf.pipe_opt & kPipeOptPublish) != 0;

    // W'_r, zero padded to NP x NP
    for (int idx = threadIdx.x; idx < NP * NP; idx += kChainThreads) {
        const int j = idx / NP, i = idx % NP;
        Wc[j * L + i] = (j < n && i < n) ? bf.W[((int64_t)r * n + j) * ld + i] : T(0);
    }
    // the relation's run of tiles, its last active sample's tile and how many of
    // that tile's pairs belong to the sample's corrupted-triple update (the tail)
    if (w == 0) {
        int run = 0, npt = 0;  // (npt: the run's pairs, this lane's tiles; o_defer alone reads them)
        for (int m0 = 0;; m0 += kWave) {
            const int g = g0 + m0 + l;
            const uint64_t b = __ballot(t0 + g < t1 && a.td_r[t0 + g] == r);
            const int k = b == ~0ull ? kWave : __builtin_ctzll(~b);
            if (o_defer && l < k) npt += bf.cnrows[g] & 127;
            run += k;
            if (k < kWave) break;
        }
        if (o_defer) {
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) npt += __shfl_xor(npt, s);
        }
        const int c0 = bf.cnrows[g0] & 127;
        const int rel = c0 > 0 && bf.cpairs[(int64_t)g0 * 2 * kCPairs + kCPairs + c0 - 1] == -2;
        int kl = -1, gt = -1;
        for (int g = g0 + run - 1; g >= g0 && kl < 0; --g) {
            const int cs = a.td_cnt[t0 + g] & 255;
            const int kk = l < cs ? a.td_kk[(t0 + g) * 8 + l] : -1;
            const uint64_t b = __ballot(kk >= 0 && a.act[kk]);
            if (b) {
                kl = __shfl(kk, 63 - __builtin_clzll(b));
                gt = g;
            }
        }
        int ntail = 0;
        if (gt >= 0) {
            const int cp = bf.cnrows[gt] & 127;
            const int sl = l < cp ? bf.cpairs[(int64_t)gt * 2 * kCPairs + kCPairs + l] : -3;
            ntail = __builtin_popcountll(__ballot(sl >= 0 && (sl >> 1) == kl * 2 + 1));
        }
        if (l == 0) {
            misc[3] = rel;
            misc[4] = gt;
            misc[5] = run;
            misc[6] = ntail;
            misc[7] = npt;
        }
    }
    __syncthreads();
    const int run = misc[5], has_rel = misc[3], g_tail = misc[4], n_tail = misc[6];
    // o_defer: a relation of bf.rec_defer chunks or more (of R pairs; the tail's chunk of its own is not
    // counted) leaves its records to the entity pass -- see the tail below
    const bool defer = o_defer && bf.rec_defer > 0 && (misc[7] + kChainRows - 1) / kChainRows >= bf.rec_defer;
    // K0 = W'^T W' (four waves, MFMA) into the P buffers; wave 0 keeps column l of it,
    // the helper waves their slices of W' (the working matrix) -- in the same registers
    T reg[4 * KS];
    {
        T* K0 = Pbuf;
        if (mine) {
#pragma unroll
            for (int ib = 0; ib < NB; ++ib) {
                typename M::acc_t acc = {T(0), T(0), T(0), T(0)};
                T av[KS], bv[KS];
#pragma unroll
                for (int s = 0; s < KS; ++s) {
                    av[s] = Wc[(4 * s + kq) * L + ib * 16 + l16];
                    bv[s] = Wc[(4 * s + kq) * L + col];
                }
#pragma unroll
                for (int s = 0; s < KS; ++s) acc = M::mma(av[s], bv[s], acc);
#pragma unroll
                for (int qq = 0; qq < 4; ++qq) K0[(ib * 16 + kq + 4 * qq) * L + col] = acc[qq];
            }
        }
        __syncthreads();
        if (w == 0) {
            const int cK = l < NP ? l : 0;
#pragma unroll
            for (int i = 0; i < 4 * KS; ++i) reg[i] = K0[i * L + cK];
        } else {
#pragma unroll
            for (int i = 0; i < 4 * KS; ++i) reg[i] = T(0);
#pragma unroll
            for (int si = 0; si < NSW; ++si) {
                const int cb = hw + 3 * si;
                if (cb < NB) {
#pragma unroll
                    for (int s = 0; s < KS; ++s) reg[si * KS + s] = Wc[(4 * s + kq) * L + cb * 16 + l16];
                }
            }
        }
        if (threadIdx.x == 0) {  // (every thread has read misc[3..6] above)
            misc[5] = 0;   // helper-wave arrivals (helper_sync)
            misc[6] = -1;  // the chunk whose walk is complete
            misc[7] = -1;  // (chunk << 6) | violators published so far
        }
        __syncthreads();  // the P buffers are free again
    }
    bool changed = false;
    int32_t* const vio = bf.vio + (int64_t)g0 * kCPairs;  // the relation's violators (run * kCPairs >= its pairs)
    int nvt = 0;
    // the chunk whose W_c update the helper waves still owe (nv 0: none)
    int pend_nv = 0, pend_par = 0, pend_pc = 0, pend_ka = 0;
    tick(0);

    // one 16 x 16 MFMA tile: rows rt of A (Ar) against rows cb of B (a Gram tile);
    // out[(rt 16 + d) * ldo + cb 16 + l16]
    // (ahead, a std::bool_constant: every LDS read of the tile in flight before its first MFMA;
    // left to itself the compiler, short of registers in the walk, reads two k-steps at a time
    // and waits for each pair.  The MFMAs and their order are the same.)
    auto gram_tile = [&](const T* Ar, const T* Bm, int rt, int cb, T* out, int ldo, auto ahead) {
        typename M::acc_t acc = {T(0), T(0), T(0), T(0)};
        T av[KS], bv[KS];
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            av[s] = Ar[(rt * 16 + l16) * L + 4 * s + kq];
            bv[s] = Bm[(cb * 16 + l16) * L + 4 * s + kq];
        }
        if constexpr (decltype(ahead)::value) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s = 0; s < KS; ++s) acc = M::mma(av[s], bv[s], acc);
#pragma unroll
        for (int q = 0; q < 4; ++q) out[(rt * 16 + kq + 4 * q) * ldo + cb * 16 + l16] = acc[q];
    };
    // rows rt of A against the helper's column slice si (its W_c fragments)
    auto proj_tile = [&](const T* Ar, int rt, int si, T* out, auto ahead) {
        const int cb = hw + 3 * si;
        typename M::acc_t acc = {T(0), T(0), T(0), T(0)};
        T av[KS];
#pragma unroll
        for (int s = 0; s < KS; ++s) av[s] = Ar[(rt * 16 + l16) * L + 4 * s + kq];
        if constexpr (decltype(ahead)::value) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s = 0; s < KS; ++s) acc = M::mma(av[s], reg[si * KS + s], acc);
#pragma unroll
        for (int q = 0; q < 4; ++q) out[(rt * 16 + kq + 4 * q) * L + cb * 16 + l16] = acc[q];
    };
    // rows of chunk [b, e) of the window: the helper waves stage them (R NP / 192
    // elements a thread, in registers), so the walker never waits on them
    constexpr int kHT = kChainThreads - kWave;
    constexpr int kRowsPer = (R * NP + kHT - 1) / kHT;
    static_assert(kRowsPer <= 32, "rows_ok bits");
    const int ht = (int)threadIdx.x - kWave;  // helper thread (w > 0)
    T rows[kRowsPer];
    uint32_t rows_ok = 0;
    auto load_rows = [&](int b, int e) {
        if (w == 0) return;
        int ent[kRowsPer];
#pragma unroll
        for (int q = 0; q < kRowsPer; ++q) {
            const int f = b + (ht + q * kHT) / NP;
            ent[q] = pe[f < kPipeList ? f : kPipeList - 1];
        }
        rows_ok = 0;
#pragma unroll
        for (int q = 0; q < kRowsPer; ++q) {
            const int idx = ht + q * kHT;
            const int k = idx / NP, j = idx % NP;
            const bool ok = idx < R * NP && b + k < e && ent[q] >= 0 && j < n;
            rows[q] = bf.ent[ok ? (uint32_t)ent[q] * (uint32_t)ld + (uint32_t)j : 0u];
            rows_ok |= (ok ? 1u : 0u) << q;
        }
    };
    auto store_rows = [&](int slot) {
        if (w == 0) return;
#pragma unroll
        for (int q = 0; q < kRowsPer; ++q) {
            const int idx = ht + q * kHT;
            if (idx < R * NP) Abuf[slot * R * L + (idx / NP) * L + idx % NP] = ((rows_ok >> q) & 1) ? rows[q] : T(0);
        }
    };
    // The helper waves meet (no s_barrier: the walker runs on): every helper has paid
    // its debt and written its projection / Gram tiles.  Bounded; a timeout sets
    // *bf.err (the host fails loudly) and gives up.
    int hsync_target = 0;
    auto helper_sync = [&]() {
        hsync_target += kChainThreads / kWave - 1;
        // (dbg 32, tests: helper wave 1 never arrives, so the others' waits time out)
        if (l == 0 && !((bf.dbg & 32) && hw == 0))
            __hip_atomic_fetch_add(&misc[5], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        for (uint32_t sp = 0;
             __hip_atomic_load(&misc[5], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < hsync_target; ++sp) {
            if (sp > (1u << 22)) {
                if (l == 0) __hip_atomic_store(bf.err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                break;
            }
            __builtin_amdgcn_s_sleep(1);
        }
    };
    // The next chunk's corrections P_n -= lr C[:, v] g_v, by the helper waves while
    // the walker walks: each violator as soon as the walker publishes it (misc[7]:
    // (chunk << 6) | count, after its G row and vl entry; misc[6] = chunk when the
    // walk ends), so after the walk only its last violators remain.  Then the
    // |p_j|^2 partials (qpart[0], the other slices' partials zero).  Sixteen threads a
    // row (one DPP row), NP / 16 columns each, rows rs, rs + 12, rs + 24.  The same
    // FMAs per element in the same order as correct_q.
    // The chunk's outputs to global memory are made here too, off the walker: each
    // violator's pair record G (da = -lr W G with the final matrix: pipe_records) and
    // vio slot as it is published (the sixteen threads of row group 0 hold the G row),
    // and after the walk the chunk's pair flags from the walker's mask (misc[1 + 2 vpar],
    // written before misc[6]); (entity'[r], r) marks the relation.  cn = 0 (the
    // window's last chunk): the outputs alone.  base: the chunk's first pair in the
    // window lists, cc its pairs.
    auto chunk_outputs = [&](T* Pn, int cn, const T* Pc, const T* An, const T* Ac, const int* vl, int ck, int base,
                             int cc, int vpar, long long t_sync) {
        constexpr int NE = NP / 16, NPS = (R + 11) / 12;
        const int rs = ht >> 4, cb = (ht & 15) * NE;
        T x[NPS][NE];
#pragma unroll
        for (int p = 0; p < NPS; ++p) {
            const int j = rs + 12 * p;
#pragma unroll
            for (int u = 0; u < NE; ++u) x[p][u] = j < cn ? Pn[j * L + cb + u] : T(0);
        }
        // o_hand: the next chunk's rows, the same for every violator, read once ahead of the
        // polling (they are in place since the chunk before), not once a violator behind its
        // vl entry: a violator's correction is then one LDS round trip shorter, the last one's
        // on the walker's path to the barrier
        T anr[NPS][NE];
#pragma unroll
        for (int p = 0; p < NPS; ++p) {
            const int j = rs + 12 * p;
#pragma unroll
            for (int u = 0; u < NE; ++u) anr[p][u] = o_hand && cn > 0 && j < R ? An[j * L + cb + u] : T(0);
        }
        int used = 0;
        long long tw = 0;  // (STATS, thread 64: the work between helper_sync and B1, the polling left out)
        if constexpr (STATS) {
            if (threadIdx.x == 64u) {
                T sink = T(0);  // (the P_n loads have arrived)
#pragma unroll
                for (int p = 0; p < NPS; ++p)
#pragma unroll
                    for (int u = 0; u < NE; ++u) sink += x[p][u];
                asm volatile("" ::"v"(sink));
                ph[30] += (unsigned long long)(clock64() - t_sync);
            }
        }
        for (uint32_t sp = 0;; ++sp) {
            const bool done = __hip_atomic_load(&misc[6], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) == ck;
            const int pw = __hip_atomic_load(&misc[7], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
            const int avail = (pw >> 6) == ck ? (pw & 63) : 0;
            if constexpr (STATS) tw = clock64();
            for (; used < avail; ++used) {
                const int v = vl[used];
                const int slv = ps[base + v];  // the violator's record slot (-2: (entity'[r], r))
                T gv[NE], av[NE], d[NPS];
#pragma unroll
                for (int u = 0; u < NE; ++u) {
                    gv[u] = Pc[v * L + cb + u];
                    av[u] = Ac[v * L + cb + u];
                }
                if (cn > 0) {
#pragma unroll
                    for (int p = 0; p < NPS; ++p) {  // a_{k+1}[j] . a_v, this thread's columns
                        const int j = rs + 12 * p;
                        d[p] = T(0);
                        if (o_hand) {
#pragma unroll
                            for (int u = 0; u < NE; ++u) d[p] = fma(anr[p][u], av[u], d[p]);
                        } else {
#pragma unroll
                            for (int u = 0; u < NE; ++u) d[p] = fma(j < R ? An[j * L + cb + u] : T(0), av[u], d[p]);
                        }
                    }
                    row16_sums<T, NPS>(d);
#pragma unroll
                    for (int p = 0; p < NPS; ++p) {
                        const int j = rs + 12 * p;
                        if (j < cn) {
                            const T gl = -lr * d[p];
#pragma unroll
                            for (int u = 0; u < NE; ++u) x[p][u] = fma(gl, gv[u], x[p][u]);
                        }
                    }
                }
                if (rs == 0) {
                    T* dst = slv >= 0 ? bf.pair + (int64_t)slv * ld : bf.relpair + (int64_t)r * ld;
#pragma unroll
                    for (int u = 0; u < NE; ++u)
                        if (cb + u < n) dst[cb + u] = gv[u];
                    if (ht == 0) {
                        vio[nvt + used] = slv;
                        if (nvt + used < kSlist) slist[nvt + used] = slv;
                    }
                }
                if constexpr (STATS) {  // from the walker's publish of the violator to the end of its correction
                    if (threadIdx.x == 64u) {
                        ph[37] += (unsigned long long)(clock64() - pubt[used]);
                        ph[38] += 1;
                    }
                }
            }
            if constexpr (STATS) {
                const long long t = clock64();
                if (threadIdx.x == 64u) ph[31] += (unsigned long long)(t - tw);
                tw = t;
            }
            if (done) {
                // (o_hand: the flags follow the barrier, from the same mask: chunk_flags)
                if (!o_hand && ht < cc) {
                    const int sl = ps[base + ht];
                    const bool vio_l = ((uint32_t)misc[1 + 2 * vpar] >> ht) & 1;
                    if (sl >= 0) bf.pflag[sl] = vio_l ? 1 : 0;
                    else if (vio_l) bf.relpair_stamp[r] = bf.stamp;
                }
                break;
            }
            if (sp > (1u << 22)) {
                if (l == 0) __hip_atomic_store(bf.err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                break;
            }
            __builtin_amdgcn_s_sleep(1);
        }
        auto post = [&] {
            if constexpr (STATS) {
                if (threadIdx.x == 64u) ph[29] += (unsigned long long)(clock64() - tw);
            }
        };
        if (cn == 0) return post();
        T sq[NPS];
#pragma unroll
        for (int p = 0; p < NPS; ++p) {
            const int j = rs + 12 * p;
            sq[p] = T(0);
            if (j < cn) {
#pragma unroll
                for (int u = 0; u < NE; ++u) {
                    if (used) Pn[j * L + cb + u] = x[p][u];
                    sq[p] = fma(x[p][u], x[p][u], sq[p]);
                }
            }
        }
        row16_sums<T, NPS>(sq);
        if ((ht & 15) == 0) {
#pragma unroll
            for (int p = 0; p < NPS; ++p) {
                const int j = rs + 12 * p;
                if (j < R) {
                    qpart[j] = j < cn ? sq[p] : T(0);
                    // (o_hand: the other slices' partials are zero since the window's first
                    // chunk, or the tail, was made afresh -- correct_q -- and nothing else
                    // writes them)
                    if (!o_hand)
                        for (int v = 1; v < NB; ++v) qpart[v * R + j] = T(0);
                }
            }
        }
        post();
    };
    // o_hand: the chunk's pair flags after the barrier, off the hand-over (the helpers'
    // first work of the next chunk; vmask: the walker's mask, misc[1 + 2 par])
    auto chunk_flags = [&](int base, int cc, uint32_t vmask) {
        if (w == 0 || ht >= cc) return;
        const int sl = ps[base + ht];
        const bool vio_l = (vmask >> ht) & 1;
        if (sl >= 0) bf.pflag[sl] = vio_l ? 1 : 0;
        else if (vio_l) bf.relpair_stamp[r] = bf.stamp;
    };
    // P_n -= lr C[:, vio] G over the chunk's nv violators (vl; G: their rows of
    // Pc) and the |p_j|^2 partials of the cn rows (qpart[0]; the other slices'
    // partials zero), eight threads a row, NP / 8 columns each (on the VALU: the
    // few violators of a chunk make an MFMA form latency-bound)
    auto correct_q = [&](T* Pn, int cn, int nv, const T* Pc, const int* vl) {
        constexpr int NE = NP / 8;
        const int j = threadIdx.x >> 3, cb = (threadIdx.x & 7) * NE;
        T sq = T(0);
        if (j < cn) {
            T x[NE];
#pragma unroll
            for (int u = 0; u < NE; ++u) x[u] = Pn[j * L + cb + u];
            for (int k = 0; k < nv; ++k) {
                const int v = vl[k];
                const T gl = -lr * Cx[j * LG + v];
#pragma unroll
                for (int u = 0; u < NE; ++u) x[u] = fma(gl, Pc[v * L + cb + u], x[u]);
            }
#pragma unroll
            for (int u = 0; u < NE; ++u) {
                if (nv) Pn[j * L + cb + u] = x[u];
                sq = fma(x[u], x[u], sq);
            }
        }
        // the row's eight lanes: quad perms, then the half-row mirror (DPP, no LDS
        // round trips; the same sums as xor 1, 2, 4)
        sq += dpp_mov<0xB1>(sq);
        sq += dpp_mov<0x4E>(sq);
        sq += dpp_mov<0x141>(sq);
        if ((threadIdx.x & 7) == 0) {
            qpart[j] = j < cn ? sq : T(0);
            for (int v = 1; v < NB; ++v) qpart[v * R + j] = T(0);
        }
    };
    // the helper waves' debt: the pending chunk's W_c -= lr A^T G on their slices
    // (its G rows in P buffer pend_pc, its rows in A slot pend_ka)
    auto apply_pending = [&]() {
        if (w == 0 || pend_nv == 0) return;
        const T* Pp = Pbuf + pend_pc * R * L;
        const T* Ap = Abuf + pend_ka * R * L;
        const int* vl = vlist + pend_par * R;
        // the violators' rows as wave-uniform values (one LDS read for all of them); a
        // violator's a row serves every slice, and the next violator's reads are in flight
        // while this one's FMAs run (per element the same order of updates)
        const int vmine = l < pend_nv ? vl[l] : 0;
        T an[KS], gn[NSW];
        auto ldv = [&](int k) {
            const int v = __builtin_amdgcn_readlane(vmine, k);
#pragma unroll
            for (int s = 0; s < KS; ++s) an[s] = Ap[v * L + 4 * s + kq];
#pragma unroll
            for (int si = 0; si < NSW; ++si) {
                const int cb = hw + 3 * si;
                gn[si] = cb < NB ? -lr * Pp[v * L + cb * 16 + l16] : T(0);
            }
        };
        const int nvu = (bf.dbg & 16) ? 0 : pend_nv;  // (dbg 16, 8: timing experiments)
        if (o_hand) {
            // two violators' reads in flight in two register sets of their own (no copies
            // between them), the slices' G elements read without a lane branch: per
            // element the same FMAs in the same order
            T a0[KS], a1[KS], ga[NSW], gb[NSW];
            auto ld2 = [&](int k, T(&av)[KS], T(&gv)[NSW]) {
                const int v = __builtin_amdgcn_readlane(vmine, k);
#pragma unroll
                for (int s = 0; s < KS; ++s) av[s] = Ap[v * L + 4 * s + kq];
#pragma unroll
                for (int si = 0; si < NSW; ++si) {
                    const int cb = hw + 3 * si;
                    gv[si] = Pp[v * L + (cb < NB ? cb : 0) * 16 + l16];
                }
            };
            auto fm2 = [&](const T(&av)[KS], const T(&gv)[NSW]) {
#pragma unroll
                for (int si = 0; si < NSW; ++si)
                    if (hw + 3 * si < NB) {
                        const T gc = -lr * gv[si];
#pragma unroll
                        for (int s = 0; s < KS; ++s) reg[si * KS + s] = fma(av[s], gc, reg[si * KS + s]);
                    }
            };
            if (nvu > 0) ld2(0, a0, ga);
            if (nvu > 1) ld2(1, a1, gb);
            for (int k = 0; k < nvu; k += 2) {
                fm2(a0, ga);
                if (k + 2 < nvu) ld2(k + 2, a0, ga);
                if (k + 1 < nvu) {
                    fm2(a1, gb);
                    if (k + 3 < nvu) ld2(k + 3, a1, gb);
                }
            }
            return;
        }
        if (nvu > 0) ldv(0);
        for (int k = 0; k < nvu; ++k) {
            T ac[KS], gc[NSW];
#pragma unroll
            for (int s = 0; s < KS; ++s) ac[s] = an[s];
#pragma unroll
            for (int si = 0; si < NSW; ++si) gc[si] = gn[si];
            if (k + 1 < nvu) ldv(k + 1);
#pragma unroll
            for (int si = 0; si < NSW; ++si)
                if (hw + 3 * si < NB) {
#pragma unroll
                    for (int s = 0; s < KS; ++s) reg[si * KS + s] = fma(ac[s], gc[si], reg[si * KS + s]);
                }
        }
        // (the pair records G were written in chunk_outputs as the walker published each violator)
    };
    // the relation's last update renormalises W_c's rows before its own pairs'
    // shrinks (transr/trainer.cpp:178-180): row sums of the slices in DPP rows, then
    // LDS; ends with a barrier.  The pending update must be applied first.
    auto renorm = [&] {
        if (w > 0) {
#pragma unroll
            for (int si = 0; si < NSW; ++si) {
                const int cb = hw + 3 * si;
#pragma unroll
                for (int s = 0; s < KS; ++s) {
                    T x[1] = {reg[si * KS + s] * reg[si * KS + s]};
                    row16_sums<T, 1>(x);
                    if (cb < NB && l16 == 0) rp[cb * NP + 4 * s + kq] = x[0];
                }
            }
        }
        __syncthreads();
        if (w > 0) {
#pragma unroll
            for (int si = 0; si < NSW; ++si) {
                if (hw + 3 * si >= NB) continue;
#pragma unroll
                for (int s = 0; s < KS; ++s) {
                    const int jr = 4 * s + kq;
                    T ss = rp[jr];
                    for (int v = 1; v < NB; ++v) ss += rp[v * NP + jr];
                    if (jr < n) reg[si * KS + s] = reg[si * KS + s] / sqrt(ss);
                }
            }
        }
        __syncthreads();
    };
    // projections and Gram matrix of a chunk afresh (the helpers their slices, wave 0
    // the Gram tiles), then the |p|^2 partials (two barriers; the chunk's rows in LDS)
    auto fresh = [&](const T* A, int cc, T* P, T* G) {
        const int nrt = cc > 16 ? 2 : 1;
        if (w > 0) {
#pragma unroll
            for (int si = 0; si < NSW; ++si)
                if (hw + 3 * si < NB)
                    for (int rt = 0; rt < nrt; ++rt) proj_tile(A, rt, si, P, std::false_type{});
        } else {
            for (int gi = 0; gi < (nrt == 2 ? 3 : 1); ++gi)
                gram_tile(A, A, gi == 0 ? 0 : 1, gi == 2 ? 1 : 0, G, LG, std::false_type{});
        }
        __syncthreads();
        correct_q(P, cc, 0, nullptr, vlist);
        __syncthreads();
    };

    // pairs a window: the LDS lists, or fewer (bf.chain_list >= 64 > a tile's
    // pairs, so every window takes at least one tile)
    // tiles a window: the prefix table, or fewer (bf.chain_tiles >= 1: tests force
    // windows that end before the relation's trailing inactive tiles)
    const int tile_cap = bf.chain_tiles >= 1 && bf.chain_tiles < kSeqMaxTiles ? bf.chain_tiles : kSeqMaxTiles;
    const int list_cap = bf.chain_list >= 64 && bf.chain_list < kPipeList ? bf.chain_list : kPipeList;
    int pc = 0;  // P / Gram buffer of the current chunk
    int par = 0;  // vlist parity of the current chunk
    for (int gw = g0; gw < g0 + run || gw == g0;) {
        if (w == 0) {  // exclusive prefix of the window's tile pair counts (the relation pair left out)
            const int nt = g0 + run - gw < tile_cap ? g0 + run - gw : tile_cap;
            int carry = 0, fit = 0;
            for (int m0 = 0; m0 < nt; m0 += kWave) {
                const int g = m0 + l;
                int c = g < nt ? (bf.cnrows[gw + g] & 127) : 0;
                if (gw + g == g0 && has_rel) c -= 1;
                int x = c;
#pragma unroll
                for (int s = 1; s < kWave; s <<= 1) {
                    const int y = __shfl_up(x, s);
                    if (l >= s) x += y;
                }
                if (g < nt) pre[g] = carry + x - c;
                fit += __builtin_popcountll(__ballot(g < nt && carry + x <= list_cap - 1));
                carry += __shfl(x, kWave - 1);
            }
            if (l == 0) {
                if (fit == nt) pre[nt] = carry;
                misc[0] = fit;
            }
        }
        __syncthreads();
        const int ntile = misc[0];
        // the window holding the relation's last active sample is its last: the
        // tiles after it hold no pairs (only inactive samples), so a window cut by
        // the tile cap after it would otherwise lose the tail's renorm
        const bool last = gw + ntile == g0 + run || (g_tail >= 0 && gw + ntile > g_tail);
        const int ntp = pre[ntile];
        const int npairs = ntp + (last && has_rel ? 1 : 0);
        const int tail_start = last && g_tail >= gw ? ntp - n_tail : npairs;
        for (int f = threadIdx.x; f < npairs; f += kChainThreads) {
            int e = r, sl = -2;
            if (f < ntp) {
                int lo = 0, hi = ntile - 1;
                while (lo < hi) {
                    const int mid = (lo + hi + 1) >> 1;
                    if (pre[mid] <= f) lo = mid;
                    else hi = mid - 1;
                }
                const int32_t* cp = bf.cpairs + (int64_t)(gw + lo) * 2 * kCPairs;
                e = cp[f - pre[lo]];
                sl = cp[kCPairs + f - pre[lo]];
            }
            pe[f] = e;
            ps[f] = sl;
        }
        // chunks of R pairs; the relation's last update's pairs (and (entity'[r], r)) alone
        auto chunk_end = [&](int b) {
            return b < tail_start ? (b + R < tail_start ? b + R : tail_start) : npairs;
        };
        __syncthreads();
        if (npairs > 0) {
            // prologue: rows of chunks 0 and 1 into A slots 0 and 1, chunk 2's in flight,
            // chunk 0's projections afresh
            const int e0 = chunk_end(0);
            const int e1 = e0 < npairs ? chunk_end(e0) : e0;
            load_rows(0, e0);
            store_rows(0);
            load_rows(e0, e1);
            store_rows(1);
            load_rows(e1, e1 < npairs ? chunk_end(e1) : e1);
            if (tail_start == 0 && changed) renorm();  // (barriers: the row stores are then visible)
            __syncthreads();
            pc = 0;
            fresh(Abuf, e0, Pbuf, Gbuf);
        }
        tick(20);
        int ka = 0;  // A slot of the current chunk
        for (int base = 0; base < npairs;) {
            const int nbase = chunk_end(base);
            const int cc = nbase - base;
            const int nb2 = nbase < npairs ? chunk_end(nbase) : nbase;
            const int cn = nb2 - nbase;  // pairs of the next chunk (0: none)
            const T* A = Abuf + ka * R * L;
            const T* An = Abuf + (ka == 2 ? 0 : ka + 1) * R * L;
            T* P = Pbuf + pc * R * L;
            T* Pn = Pbuf + (pc ^ 1) * R * L;
            T* Gm = Gbuf + pc * R * LG;
            T* Gn = Gbuf + (pc ^ 1) * R * LG;
            int* vl = vlist + par * R;
            const int ck = n_chunks;  // the chunk's tag in the publish words (misc[6], misc[7])
            ++n_chunks;
            tick(1);
            if (w == 0) {
                // Walk: the pairs in order, each against the matrix the earlier ones left
                // (transr/trainer.cpp:35-64 per pair).  A violator v's shrink
                // W_c -= lr a_v^T g_v moves every later projection by -lr (a_j . a_v) g_v.
                const int j = l & (R - 1);
                T q = T(0);
                if (j < cc) {
                    q = qpart[j];
                    for (int v = 1; v < NB; ++v) q += qpart[v * R + j];
                }
                uint32_t vmask = 0;
                int npub = 0;  // violators published to the helper waves (chunk_outputs)
                if (__ballot(j < cc && q > T(1)) != 0) {
                    const T aaj = Gm[j * LG + j];  // |a_j|^2 (the Gram diagonal), off the violators' path
                    const int c0 = (l >> 5) * NH;
                    T x[NH];  // row j, columns c0 .. c0 + NH - 1
#pragma unroll
                    for (int u = 0; u < NH; ++u) x[u] = P[j * L + c0 + u];
                    int cursor = 0;
                    const T eps = T(2) * lr;
                    for (;;) {
                        const uint64_t cand = __ballot(l < R && j < cc && j >= cursor && q > T(1));
                        if (!cand) break;
                        const int v = __builtin_ctzll(cand);
                        const int c = l;  // column
                        // the scalars known at the pick, ahead of V: |p_v|^2, 1 / |p_v|^2, |a_v|^2
                        const T pp = readlane_f(q, v);
                        const T aa = readlane_f(aaj, v);
                        const T cjv = Gm[j * LG + v];  // a_j . a_v for the later rows' update
                        tick(4);
                        // V = p_v K0.  The chunk's rows in LDS are current (the later rows' update
                        // below writes them back), so the violator's row is read as it stands: no
                        // row move on the path.  The row is staged in NG groups of k-steps, two
                        // groups in flight, a group's FMAs under the next one's reads, so the
                        // staging registers beside K0's column stay few; the four chains and
                        // their order as ever.
                        T vv4[4] = {T(0), T(0), T(0), T(0)};
                        constexpr int NG = 6;
                        T pr[4 * KS];
                        auto v_load = [&](int g) {
#pragma unroll
                            for (int t = g * KS / NG; t < (g + 1) * KS / NG; ++t)
#pragma unroll
                                for (int u = 0; u < 4; ++u) pr[4 * t + u] = P[v * L + 4 * t + u];
                        };
                        auto v_fma = [&](int g) {
#pragma unroll
                            for (int t = g * KS / NG; t < (g + 1) * KS / NG; ++t)
#pragma unroll
                                for (int u = 0; u < 4; ++u) vv4[u] = fma(pr[4 * t + u], reg[4 * t + u], vv4[u]);
                        };
                        v_load(0);
                        v_load(1);
                        const T pv = c < NP ? P[v * L + c] : T(0);
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int g = 0; g < NG; ++g) {
                            v_fma(g);
                            if (g + 2 < NG) {
                                __builtin_amdgcn_sched_barrier(0);
                                v_load(g + 2);
                                __builtin_amdgcn_sched_barrier(0);
                            }
                        }
                        const T Vc = c < n ? (vv4[0] + vv4[1]) + (vv4[2] + vv4[3]) : T(0);
                        tick(7);
                        T s2[2] = {pv * Vc, Vc * Vc};
                        // 1 / |p_v|^2: v_rcp_f64 and two Newton steps, as LLVM's own f64 division
                        // before its final correction (the reciprocal to within an ulp; kappa =
                        // pvd / pp then differs from the quotient by at most an ulp or so, which
                        // moves rho = 1 - 2 lr kappa by ~1e-3 ulp: no round test flips on it),
                        // issued beside the wave sums, off the violator's critical path
                        T rpp = __builtin_amdgcn_rcp(pp);
                        rpp = fma(fma(-pp, rpp, T(1)), rpp, rpp);
                        rpp = fma(fma(-pp, rpp, T(1)), rpp, rpp);
                        wave_sums<T, 2>(s2);
                        tick(8);
                        const T pV = s2[0], VV = s2[1];
                        const T pvd = pV + aa * pp, vvd = VV + T(2) * aa * pV + aa * aa * pp;
                        const T kappa = pvd * rpp;
                        const T w2t = vvd - kappa * pvd;
                        const T w2 = w2t > T(0) ? w2t : T(0);
                        const T rho = T(1) - eps * kappa;
                        T S0, S1;
                        const int m = transr_rounds_violator4(pp, w2, eps, rho, S0, S1);
                        if constexpr (STATS) {
                            n_rounds += (unsigned long long)m;
                            max_m = max_m > (unsigned long long)m ? max_m : (unsigned long long)m;
                        }
                        const T cpf = T(2) * (S0 + eps * S1 * kappa), cvf = T(2) * eps * S1;
                        const T g = c < n ? cpf * pv - cvf * (Vc + aa * pv) : T(0);
                        tick(9);
                        // the violator's row now holds G (its pair record in global memory and
                        // its vio slot are the helper waves', chunk_outputs)
                        if (c < NP) P[v * L + c] = g;
                        tick(10);
                        // o_pub: v is published here, right behind its G row's store and ahead of the later
                        // rows' update, which no reader of the publish word needs (chunk_outputs reads the G
                        // row, A's row v, the vl entry and the slot): the helpers correct v while the later
                        // rows move, and the last violator's correction is off the walker's way to B1.  (The
                        // release waits for the G row's store before the later rows' reads of it are issued.
                        // With the publish between those reads and their FMAs instead, so that the two waits
                        // coincide, the kernel took 53 more AGPRs and 260 more v_accvgpr moves under the
                        // lanes' branch and was slower on the bench than this order: DESIGN.md 7, round 11.)
                        if (o_pub && l == 0) {
                            vl[npub] = v;
                            if constexpr (STATS) pubt[npub] = clock64();
                            __hip_atomic_store(&misc[7], (ck << 6) | (npub + 1), __ATOMIC_RELEASE,
                                               __HIP_MEMORY_SCOPE_WORKGROUP);
                        }
                        const bool upd = j > v && j < cc;
                        T qh = T(0);  // this lane's half of |p_j|^2
                        if (upd) {
                            const T gl = -lr * cjv;
                            T s4[4] = {T(0), T(0), T(0), T(0)};
                            // (every read of the G row in flight before the first FMA)
                            T gr[NH];
#pragma unroll
                            for (int u = 0; u < NH; ++u) gr[u] = P[v * L + c0 + u];
                            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                            for (int u = 0; u < NH; ++u) {
                                x[u] = fma(gl, gr[u], x[u]);
                                s4[u & 3] = fma(x[u], x[u], s4[u & 3]);
                            }
                            // the row back to LDS: the next violator's row is read from there
#pragma unroll
                            for (int u = 0; u < NH; ++u) P[j * L + c0 + u] = x[u];
                            qh = (s4[0] + s4[1]) + (s4[2] + s4[3]);
                        }
                        {
                            const T tot = pair_sum32(qh);  // lanes j and j + 32: the same bits
                            if (upd) q = tot;
                        }
                        // publish v to the helper waves: its G row (above) and vl entry first
                        if (!o_pub && l == 0) {
                            vl[npub] = v;
                            if constexpr (STATS) pubt[npub] = clock64();
                            __hip_atomic_store(&misc[7], (ck << 6) | (npub + 1), __ATOMIC_RELEASE,
                                               __HIP_MEMORY_SCOPE_WORKGROUP);
                        }
                        ++npub;
                        vmask |= 1u << v;
                        cursor = v + 1;
                        if constexpr (STATS) ++n_vio;
                        tick(11);
                    }
                }
                if (l == 0) {  // (the chunk's pair flags: the helper waves, from this mask)
                    misc[1 + 2 * par] = (int)vmask;
                    misc[2 + 2 * par] = npub;
                    __hip_atomic_store(&misc[6], ck, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
                tick(2);
            } else {
                // chunk k-1's W_c update and records, then the next chunk against W_{k-1}:
                // X = A_{k+1} W_c (each helper its own slices), its Gram matrix and the cross
                // Gram A_{k+1} A_k^T (waves 2 and 3)
                apply_pending();
                tick(12);
                if (cn > 0) {
                    const int nrt = cn > 16 ? 2 : 1, crt = cc > 16 ? 2 : 1;
#pragma unroll
                    for (int si = 0; si < NSW; ++si)
                        if (hw + 3 * si < NB)
                            for (int rt = 0; rt < nrt; ++rt) {
                                if (o_hand) proj_tile(An, rt, si, Pn, std::true_type{});
                                else proj_tile(An, rt, si, Pn, std::false_type{});
                            }
                    // the Gram tiles to the helpers with the fewest projection tiles (the
                    // same greedy choice on every helper); no cross Gram: chunk_outputs takes
                    // the few violators' dots a_{k+1}[j] . a_v on the fly
                    const int ng = nrt == 2 ? 3 : 1;
                    int load[3];
#pragma unroll
                    for (int h = 0; h < 3; ++h) load[h] = nrt * ((NB - h + 2) / 3);  // slices h, h + 3, ...
                    for (int tl = 0; tl < ng; ++tl) {
                        int best = 0;
#pragma unroll
                        for (int h = 1; h < 3; ++h) best = load[h] < load[best] ? h : best;
                        ++load[best];
                        if (best == hw) {
                            if (o_hand) gram_tile(An, An, tl == 0 ? 0 : 1, tl == 2 ? 1 : 0, Gn, LG, std::true_type{});
                            else gram_tile(An, An, tl == 0 ? 0 : 1, tl == 2 ? 1 : 0, Gn, LG, std::false_type{});
                        }
                    }
                    (void)crt;
                }
                // every helper past its debt (chunk k-1's A slot and G rows are free) and its
                // tiles (P_n, the Gram matrices complete)
                tick(13);
                helper_sync();
                tick(14);
                const long long t_sync = STATS ? clock64() : 0;
                // chunk k+2's rows into the slot chunk k-1 left, chunk k+3's in flight
                if (nb2 < npairs || cn > 0) {
                    store_rows(ka == 0 ? 2 : ka - 1);
                    const int n3 = nb2 < npairs ? chunk_end(nb2) : nb2;
                    load_rows(n3, n3 < npairs ? chunk_end(n3) : n3);
                }
                // chunk k's violators into P_{k+1} as the walker publishes them, then |p|^2;
                // its records and pair flags to global memory
                chunk_outputs(Pn, cn, P, An, A, vl, ck, base, cc, par, t_sync);
                tick(15);
            }
            __syncthreads();  // B1: the walk, the next chunk's corrected projections and |p|^2
            tick(w == 0 ? 3 : 5);
            const uint32_t vmask = (uint32_t)misc[1 + 2 * par];
            const int nv = misc[2 + 2 * par];
            if constexpr (STATS) {
                if (threadIdx.x == 0) {
                    const int bk = nv == 0 ? 0 : nv <= 2 ? 1 : nv <= 5 ? 2 : 3;
                    ph[21 + bk] += (unsigned long long)dtq;
                    ph[25 + bk] += 1;
                }
            }
            if (o_hand) chunk_flags(base, cc, vmask);
            // chunk k's debt passes to the helpers (paid at the next chunk, or below)
            pend_nv = nv;
            pend_par = par;
            pend_pc = pc;
            pend_ka = ka;
            nvt += nv;
            if (vmask) changed = true;
            const bool restart = nbase == tail_start && changed && cn > 0;  // the tail: afresh
            tick(6);
            if (restart) {
                apply_pending();  // the matrix up to date before the rows' renorm
                pend_nv = 0;
                __syncthreads();
                renorm();
                fresh(An, cn, Pn, Gn);
            }
            pc ^= 1;
            par ^= 1;
            ka = ka == 2 ? 0 : ka + 1;
            base = nbase;
        }
        // the window's last debt before its lists are rebuilt
        apply_pending();
        pend_nv = 0;
        __syncthreads();
        tick(16);
        gw += ntile;
        if (last || gw >= g0 + run) break;
    }
    // the helpers' slices into LDS: the relation's final matrix, for the records and HBM
    if (w > 0) {
#pragma unroll
        for (int si = 0; si < NSW; ++si) {
            const int cb = hw + 3 * si;
            if (cb < NB) {
#pragma unroll
                for (int s = 0; s < KS; ++s) Wc[(4 * s + kq) * L + cb * 16 + l16] = reg[si * KS + s];
            }
        }
    }
    __syncthreads();
    tick(17);
    // the records first (the A slots, the P buffers and the window lists are free), so
    // that their G row loads queue behind no store; then the matrix to HBM, whole rows
    // by all threads
    // o_defer, a long relation: no record pass behind its chain.  Its violators' rows of bf.pair / bf.relpair
    // keep the G rows chunk_outputs wrote, the relation carries this launch's stamp, and the entity pass makes
    // da = -lr W G from the matrix written back below (rpar_record_convert: the same sum), on the waves that
    // add the records, all over the GPU instead of on this workgroup's four
    if (!defer) pipe_records<T, NP, L, 5 * R * L, STATS>(a, bf, r, vio, nvt, Wc, Abuf, pe, slist, kSlist, ph + (STATS ? 32 : 0));
    else if (threadIdx.x == 0 && nvt > 0) bf.rec_stamp[r] = bf.stamp;
    if constexpr (STATS) {
        __syncthreads();  // (the slowest wave's records)
        tick(18);
    }
    {
        constexpr int NWB = NP * NP / kChainThreads;  // (every LDS read in flight before the first store)
        static_assert(NWB * kChainThreads == NP * NP, "whole rounds of the write-back");
        T wv[NWB];
#pragma unroll
        for (int q = 0; q < NWB; ++q) {
            const int idx = threadIdx.x + q * kChainThreads;
            wv[q] = Wc[(idx / NP) * L + idx % NP];
        }
#pragma unroll
        for (int q = 0; q < NWB; ++q) {
            const int idx = threadIdx.x + q * kChainThreads;
            const int jj = idx / NP, i = idx % NP;
            if (jj < n && i < n) bf.W[((int64_t)r * n + jj) * ld + i] = wv[q];
        }
    }
    if constexpr (STATS) {
        tick(19);
        if (threadIdx.x == 0) {
            const unsigned long long cyc = (unsigned long long)(clock64() - ck0);
            atomicAdd(&g_seq_stats[0], 1ull);
            atomicAdd(&g_seq_stats[1], (unsigned long long)n_chunks);
            atomicAdd(&g_seq_stats[2], n_vio);
            atomicAdd(&g_seq_stats[3], n_rounds);
            atomicAdd(&g_seq_stats[4], cyc);
            atomicMax(&g_seq_stats[5], cyc);
            atomicMax(&g_seq_stats[6], (unsigned long long)n_chunks);
            atomicMax(&g_seq_stats[7], max_m);
            for (int k = 0; k < 16; ++k) atomicAdd(&g_seq_stats[8 + k], ph[k]);
            for (int k = 0; k < 4; ++k) atomicAdd(&g_seq_stats[44 + k], ph[16 + k]);
            if (n_chunks >= 12) {  // (the hottest relation of a default half-batch walks 15-18 chunks)
                for (int k = 0; k < 16; ++k) atomicAdd(&g_seq_stats[24 + k], ph[k]);
                atomicAdd(&g_seq_stats[40], (unsigned long long)n_chunks);
                atomicAdd(&g_seq_stats[41], 1ull);
                atomicAdd(&g_seq_stats[42], n_vio);
                atomicAdd(&g_seq_stats[43], cyc);
                for (int k = 0; k < 4; ++k) atomicAdd(&g_seq_stats[48 + k], ph[16 + k]);
                for (int k = 20; k < 39; ++k) atomicAdd(&g_seq_stats[32 + k], ph[k]);  // 52..70
            }
            if (defer && nvt > 0) {
                atomicAdd(&g_seq_stats[71], 1ull);
                atomicAdd(&g_seq_stats[72], (unsigned long long)nvt);
            }
        }
    }
}

}  // namespace kb2e
