// engine_transr_parallel.inc -- host orchestration of TransR under the PARALLEL
// schedule (kernels_transr_parallel.hpp).  Included by engine.hip.
namespace {

constexpr int32_t kRParLongMin = 128;  // entity segments this long take a whole workgroup

// the matrix-core tile kernel for NP / 16 = nb column blocks (n <= 128)
template <typename T, bool P, bool G>
const void* tile_fn(int nb) {
    switch (nb) {
        case 1: return (const void*)transr_tile_mfma_kernel<T, P, G, 1>;
        case 2: return (const void*)transr_tile_mfma_kernel<T, P, G, 2>;
        case 3: return (const void*)transr_tile_mfma_kernel<T, P, G, 3>;
        case 4: return (const void*)transr_tile_mfma_kernel<T, P, G, 4>;
        case 5: return (const void*)transr_tile_mfma_kernel<T, P, G, 5>;
        case 6: return (const void*)transr_tile_mfma_kernel<T, P, G, 6>;
        case 7: return (const void*)transr_tile_mfma_kernel<T, P, G, 7>;
        case 8: return (const void*)transr_tile_mfma_kernel<T, P, G, 8>;
    }
    throw std::runtime_error("TransR tile kernel: n > 128");
}

// the transRNorm tile kernel for NP / 16 = nb column blocks (n <= 128)
template <typename T>
const void* cons_tile_fn(int nb) {
    switch (nb) {
        case 1: return (const void*)transr_cons_tile_kernel<T, 1>;
        case 2: return (const void*)transr_cons_tile_kernel<T, 2>;
        case 3: return (const void*)transr_cons_tile_kernel<T, 3>;
        case 4: return (const void*)transr_cons_tile_kernel<T, 4>;
        case 5: return (const void*)transr_cons_tile_kernel<T, 5>;
        case 6: return (const void*)transr_cons_tile_kernel<T, 6>;
        case 7: return (const void*)transr_cons_tile_kernel<T, 7>;
        case 8: return (const void*)transr_cons_tile_kernel<T, 8>;
    }
    throw std::runtime_error("transRNorm tile kernel: n > 128");
}

template <typename T>
size_t rpar_lds(const kb2e_ctx* c) {
    return rpar_tile_lds<T>(c->n, c->ld, c->rpar_St);
}

template <typename T>
size_t rmfma_lds(const kb2e_ctx* c, bool cons) {
    return cons ? rmfma_cons_lds<T>(c->n, c->rpar_St) : rmfma_tile_lds<T>(c->n, c->rpar_St);
}

// run_l [kScanChunk][2n] + the chunk-prefix partials [1024 / 2n][2n] (1024-thread blocks)
// (ahead, the kPassOptScan kernels, n <= 64: a set of partials for every sub-batch a block reads ahead -- a
// thread takes at most two of the kScanQuarters (set, run) slots a sub-batch: rpar_scan_ahead_slots)
size_t rpar_scan_lds(const kb2e_ctx* c, bool ahead = false) {
    const int G = std::max(1, 1024 / (2 * c->n));
    const int sets = ahead && c->n <= 64 ? std::max(1, std::min<int>(c->sub, 2 * G / kScanQuarters)) : 1;
    return (size_t)kScanChunk * 2 * c->n * 8 + (size_t)sets * G * 2 * c->n * 8;
}

// Matrix-core path: the largest St <= 8 whose tile and transRNorm images both
// fit in 150 KiB (one 8-wave workgroup per CU); 0 if none does.  (St = 16
// halves the tiles of FB15k-shaped batches but lengthens each more than that.)
// tile_only: transRNorm runs in the wide chain kernel (n > 64, FP64), so only the
// tile image has to fit -- in 96 KiB (n = 100: St = 8; the compat launches' images,
// projection-only 73 KiB and gradient-only 29 KiB, still fit two or more a CU).
// (KB2E_RPAR_TILE_KB=k: that budget in KiB for the tile-only case, A/B)
int choose_mfma_samples(int n, int esize, bool tile_only = false) {
    const char* tk = getenv("KB2E_RPAR_TILE_KB");
    // (96 KiB: St = 8 at n = 100, A/B r21 K5 1.19 against 1.17x10^7 with 76 KiB / St = 4)
    const size_t tile_kb = tk ? (size_t)std::max(16, std::min(160, atoi(tk))) : 96;
    for (int St = 8; St >= 1; St >>= 1) {
        const size_t a = esize == 8 ? rmfma_tile_lds<double>(n, St) : rmfma_tile_lds<float>(n, St);
        const size_t b = tile_only ? 0 : esize == 8 ? rmfma_cons_lds<double>(n, St) : rmfma_cons_lds<float>(n, St);
        if (std::max(a, b) <= (tile_only ? tile_kb : 150) * 1024) return St;
    }
    return 0;
}

// Samples per tile: the largest power of two <= 32 whose LDS image fits in
// 64 KiB (two workgroups per CU), or in 150 KiB when one matrix alone is larger.
int choose_tile_samples(int n, int ld, int esize) {
    const size_t budget = (size_t)n * ld * esize > 40 * 1024 ? 150 * 1024 : 64 * 1024;
    for (int St = 32; St > 1; St >>= 1) {
        const size_t b = esize == 8 ? rpar_tile_lds<double>(n, ld, St) : rpar_tile_lds<float>(n, ld, St);
        if (b <= budget) return St;
    }
    return 1;
}

void setup_transr_parallel(kb2e_ctx* c) {
    const kb2e_config& g = c->cfg;
    const size_t es = (size_t)c->esize;
    // n > 64 in FP64: transRNorm runs in the wide chain kernel, so the matrix-core
    // tile kernels only need their own image to fit (n = 100: St = 4, one workgroup a CU)
    const char* ck0 = getenv("KB2E_RPAR_CONS");
    const bool wide_planned = c->f64() && c->n > 64 && cons_chainw_supported(c->n) &&
                              !(ck0 && (std::string(ck0) == "jacobi" || std::string(ck0) == "tile"));
    // 128 < n <= 512: the wide kernels (matrices from global memory) take the whole step
    c->rpar_widep = wide_par_supported(c->n);
    const int mst = c->rpar_widep ? 0 : choose_mfma_samples(c->n, c->esize, wide_planned);
    const char* mf = getenv("KB2E_RPAR_MFMA");  // 0: force the VALU tile kernels (tests)
    c->rpar_mfma = mst > 0 && !(mf && mf[0] == '0');
    if (c->rpar_widep) c->rpar_wg = wide_setup(c->n, c->ld, c->esize);
    c->rpar_St = c->rpar_widep ? c->rpar_wg.St : c->rpar_mfma ? mst : choose_tile_samples(c->n, c->ld, c->esize);
    if (const char* nc = getenv("KB2E_RPAR_NOC")) c->rpar_no_constraint = nc[0] == '1';  // debugging
    // matrix-core tile kernels: four waves per workgroup, several workgroups per CU
    // (eight waves when the image allows one workgroup a CU only)
    c->rpar_tile_threads = wide_planned && c->rpar_mfma ? 512 : 256;
    if (const char* tt = getenv("KB2E_RPAR_TILE_THREADS")) c->rpar_tile_threads = atoi(tt) >= 512 ? 512 : 256;
    // eight-wave tile blocks run groups of a relation's tiles: one matrix partial and
    // one W staging a group instead of a tile (KB2E_RPAR_TGROUP=1: a tile a block)
    c->rpar_tgroup = c->rpar_tile_threads == 512 ? 8 : 1;
    if (const char* tg = getenv("KB2E_RPAR_TGROUP")) c->rpar_tgroup = std::max(1, std::min(kTileGroupMax, atoi(tg)));
    if (const char* st = getenv("KB2E_RPAR_ST")) c->rpar_St = std::max(1, std::min(c->rpar_St, atoi(st)));
    // transr_cons_tile_kernel: one lane per pair (4 St + 1 <= 64), one wave per 16-row block (of 8)
    if (c->rpar_mfma && 4 * c->rpar_St + 1 > 64) throw std::runtime_error("transRNorm tile: St > 15");
    c->rpar_max_tiles = (int)(std::min<int64_t>(g.num_relations, c->B) + c->B / c->rpar_St + 1);
    const int64_t nkeys = c->S * c->slots;
    c->rpar_y.alloc((size_t)c->B * 2 * c->ld * es);
    // matrix partials: one per tile (gradient step), one per (tile, row block) for
    // the register-resident transRNorm kernel
    const bool cw = cons_wave_supported(c->n) && mst > 0;
    // sub-batches on the n <= 64 wave path (the condition of rpar_cons_wave below): phase
    // A once a batch for all of them (KB2E_RPAR_MERGE_A=0: per sub-batch, on the
    // start-of-batch copies), unless the compat scan of a sub-batch takes the chunk
    // prefix kernel (more than kScanDirectMax chunks, or KB2E_RPAR_SCAN_PREFIX=1)
    c->rpar_merge_a = false;
    c->rpar_merge = RParMerge{};
    if (c->sub > 1 && c->rpar_mfma && cw && c->rpar_St <= 8 && !(ck0 && std::string(ck0) == "tile")) {
        const char* ma = getenv("KB2E_RPAR_MERGE_A");
        const char* sp = getenv("KB2E_RPAR_SCAN_PREFIX");
        const int64_t nch = (2 * c->Bs + kScanChunk - 1) / kScanChunk;
        const bool use_pre = g.transr_compat && (sp ? sp[0] == '1' : nch > kScanDirectMax);
        c->rpar_merge_a = !(ma && ma[0] == '0') && !use_pre;
    }
    // tile slots: of a batch, or (merged phase A) `sub` times a sub-batch's, side by side
    int64_t tslots = c->rpar_max_tiles;
    if (c->rpar_merge_a) {
        RParMerge& m = c->rpar_merge;
        m.sub = c->sub;
        m.Bs = (int32_t)c->Bs;
        m.Blast = (int32_t)(c->B - (int64_t)(c->sub - 1) * c->Bs);
        m.tcap = (int32_t)(std::min<int64_t>(g.num_relations, c->Bs) + c->Bs / c->rpar_St + 1);
        m.nch = (int32_t)((2 * c->Bs + kScanChunk - 1) / kScanChunk);
        m.brel_cap = (int32_t)std::min<int64_t>(g.num_relations, c->Bs);
        tslots = (int64_t)m.sub * m.tcap;
    }
    c->rpar_wpart.alloc((size_t)tslots * (cw ? kConsPpt : 1) * c->n * c->ld * es);
    c->rpar_rpart.alloc((size_t)tslots * c->ld * es);
    c->rpar_tile_act.alloc((size_t)(nkeys + 1) * 4);
    c->rpar_pair.alloc((size_t)c->B * 4 * c->ld * es);
    c->rpar_relpair.alloc((size_t)g.num_relations * c->ld * es);
    c->rpar_relpair_stamp.alloc((size_t)g.num_relations * 4 * 2);  // (then RParBufs::rec_stamp, [R])
    memset_sync(c->rpar_relpair_stamp.p, 0, c->rpar_relpair_stamp.bytes);
    c->rpar_tiles.alloc((size_t)(nkeys + 1) * sizeof(RTile));
    c->rpar_ntiles.alloc((size_t)(nkeys + 1) * 4);
    c->rpar_tile_first.alloc((size_t)(nkeys + 1) * 4);
    c->rpar_rel_begin.alloc((size_t)c->nbi * 4);
    c->rpar_brel_cap = std::min<int64_t>(g.num_relations, c->Bs);
    c->rpar_brel.alloc((size_t)c->nbi * c->rpar_brel_cap * 4);
    // (three counts an index batch: its relations, its entity segments, the long ones of them: rel_list_kernel)
    c->rpar_bnrel.alloc((size_t)c->nbi * 3 * 4);
    for (int32_t** h : {&c->pin_bnrel, &c->pin_sh_bnrel}) {
        if (*h) (void)hipHostFree(*h);
        *h = nullptr;
        HIPCHK(hipHostMalloc((void**)h, (size_t)c->nbi * 3 * 4, 0));
        std::memset(*h, 0, (size_t)c->nbi * 3 * 4);
    }
    if (c->rpar_widep) c->rpar_wsc.alloc((size_t)c->rpar_brel_cap * c->n * c->ld * 8);
    else c->rpar_wsc.free();
    if (c->sub > 1 && !c->rpar_merge_a) {  // the start-of-batch tables phase A reads while phase B runs sub-batch by sub-batch
        c->snap_ent.alloc(c->ent.bytes);
        c->snap_rel.alloc(c->rel.bytes);
        c->snap_w.alloc(c->w.bytes);
        for (DevBuf* d : {&c->snap_ent, &c->snap_rel, &c->snap_w}) memset_sync(d->p, 0, d->bytes);
        if (!c->suba_stream) {
            int lo = 0, hi = 0;
            HIPCHK(hipDeviceGetStreamPriorityRange(&lo, &hi));
            HIPCHK(hipStreamCreateWithPriority(&c->suba_stream, hipStreamNonBlocking, hi));
            for (hipEvent_t* e : {&c->ev_adone[0], &c->ev_adone[1], &c->ev_bdone[0], &c->ev_bdone[1]})
                HIPCHK(hipEventCreateWithFlags(e, hipEventDisableTiming));
        }
    } else {
        for (DevBuf* d : {&c->snap_ent, &c->snap_rel, &c->snap_w}) d->free();
    }
    if (g.num_entities >= (1 << kPtabEntBits) - 1 || g.num_relations >= (1 << kPtabRelBits) - 1 ||
        c->B * 4 >= (1 << kPtabSlotBits))
        throw std::invalid_argument("PARALLEL TransR: at most 2^24 - 2 entities, 2^18 - 2 relations, 2^20 - 1 samples a batch");
    {  // the pair-dedupe tables: >= 3x the batch's update slots, a power of two, all empty;
       // three of them in rotation (sub-batches: phase A runs one sub-batch ahead), or
       // (merged phase A) two groups of `sub`, each for a sub-batch's slots
        size_t sz = 1024;
        while (sz < (size_t)(c->rpar_merge_a ? c->Bs : c->B) * 4 * 3) sz <<= 1;
        const size_t ntab = c->rpar_merge_a ? 2 * (size_t)c->sub : 3;
        c->rpar_ptab_mask = (uint32_t)(sz - 1);
        c->rpar_ptab.alloc(ntab * sz * 8);
        memset_sync(c->rpar_ptab.p, 0xff, ntab * sz * 8);
        c->rpar_merge_batches = 0;
    }
    const int scan_chunk = c->rpar_widep ? c->rpar_wg.chunk : kScanChunk;
    // (merged phase A: every sub-batch its own chunking, m.nch chunk slots each)
    c->rpar_scan.alloc((size_t)std::max<int64_t>((2 * c->B + scan_chunk - 1) / scan_chunk,
                                                  (int64_t)c->rpar_merge.sub * c->rpar_merge.nch) *
                       2 * c->n * 8);
    c->rpar_scan_pre.alloc(c->rpar_scan.bytes);
    c->rpar_pflag.alloc((size_t)c->B * 4);
    c->rpar_cons_tile.alloc((size_t)tslots * (cw ? kConsPpt : 1) * 4);
    if (cw) {  // register-fragment kernels: compacted transRNorm pairs
        c->rpar_cpairs.alloc((size_t)tslots * 2 * kCPairs * 4);
        c->rpar_vio.alloc((size_t)tslots * kCPairs * 4);
        c->rpar_cnrows.alloc((size_t)tslots * 4);
    }
    size_t tb = 0;
    HIPCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, (int32_t*)nullptr, (int32_t*)nullptr, (int)(nkeys + 1),
                                            c->stream));
    if (tb > c->sort_tmp_bytes) {
        c->sort_tmp_bytes = tb;
        c->sort_tmp.alloc(tb);
    }
    const size_t lds = c->f64() ? rpar_lds<double>(c) : rpar_lds<float>(c);
    auto allow = [&](const void* k) {
        (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    };
    allow((const void*)transr_tile_kernel<double, true, true>);
    allow((const void*)transr_tile_kernel<double, true, false>);
    allow((const void*)transr_tile_kernel<double, false, true>);
    allow((const void*)transr_tile_kernel<float, true, true>);
    allow((const void*)transr_tile_kernel<float, true, false>);
    allow((const void*)transr_tile_kernel<float, false, true>);
    allow((const void*)transr_constraint_kernel<double>);
    allow((const void*)transr_constraint_kernel<float>);
    c->rpar_cons_wave = false;
    if (c->rpar_mfma) {
        const size_t l1 = c->f64() ? rmfma_lds<double>(c, false) : rmfma_lds<float>(c, false);
        const size_t l2 = c->f64() ? rmfma_lds<double>(c, true) : rmfma_lds<float>(c, true);
        const int nb = rm_np(c->n) / 16;
        for (const void* k : {tile_fn<double, true, true>(nb), tile_fn<double, true, false>(nb),
                              tile_fn<double, false, true>(nb), tile_fn<float, true, true>(nb),
                              tile_fn<float, true, false>(nb), tile_fn<float, false, true>(nb)})
            (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)l1);
        if (!wide_planned)  // (the Jacobi transRNorm tile image; too large for the wide-chain widths)
            for (int nb = 1; nb <= 8; ++nb)
                (void)hipFuncSetAttribute(c->f64() ? cons_tile_fn<double>(nb) : cons_tile_fn<float>(nb),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)l2);
        // n <= 64: the rounds in one wave's registers (KB2E_RPAR_CONS=tile: the LDS-round kernel)
        const char* ck = getenv("KB2E_RPAR_CONS");
        // (the wave kernels take St <= 8: choose_mfma_samples never exceeds it)
        c->rpar_cons_wave = cw && c->rpar_St <= 8 && !(ck && std::string(ck) == "tile");
        if (c->rpar_merge_a && !c->rpar_cons_wave) throw std::logic_error("merged phase A off the wave path");
        if (c->rpar_cons_wave) c->rpar_cons_lds = cons_wave_setup(c->n, c->rpar_St, c->esize);
        // FP64: the relation's pairs one after another, each against the matrix the
        // earlier ones left (default on the wave path; KB2E_RPAR_CONS=jacobi: every pair
        // of the batch against the same W', the register-resident tile kernel)
        c->rpar_cons_seq = c->rpar_cons_wave && c->f64() && !(ck && std::string(ck) == "jacobi");
        if (c->rpar_cons_seq) {
            c->rpar_seq_lds = cons_seq_setup(c->n);
        }
    }
    {
        // FP64 off the n <= 64 matrix-core chain (the VALU tile path, n = 65 .. 112):
        // the same pair-by-pair chain (kernels_transr_chainw.hpp); KB2E_RPAR_CONS=jacobi
        // or =tile keeps the Jacobi kernels
        const char* ck = getenv("KB2E_RPAR_CONS");
        const bool jac = ck && (std::string(ck) == "jacobi" || std::string(ck) == "tile");
        const char* chn = getenv("KB2E_RPAR_CHAIN");
        c->rpar_cons_wide = !c->rpar_cons_seq && c->f64() && cons_chainw_supported(c->n) && !jac;
        if (c->rpar_cons_wide) c->rpar_wide_lds = cons_chainw_setup(c->n);
        // FP32 tables and 112 < n <= 128: the same pair-by-pair chain in double arithmetic
        // (kernels_transr_chaing.hpp; KB2E_RPAR_CHAIN=gen forces it for any n <= 128, tests)
        const bool force_gen = chn && std::string(chn) == "gen";
        if (force_gen && !jac) c->rpar_cons_seq = c->rpar_cons_wide = false;
        c->rpar_cons_gen = !c->rpar_cons_seq && !c->rpar_cons_wide && !jac && cons_chaing_supported(c->n);
        if (c->rpar_cons_gen) c->rpar_gen_lds = cons_chaing_setup(c->n, c->esize);
        if (c->rpar_widep) c->rpar_cons_seq = c->rpar_cons_wide = c->rpar_cons_gen = false;  // (its own chain)
        // the pair-by-pair transRNorm is the only default (the Jacobi form moves the loss
        // ~20 % off the reference's, DESIGN.md 7): KB2E_RPAR_CONS=jacobi asks for it by name
        if (!c->rpar_cons_seq && !c->rpar_cons_wide && !c->rpar_cons_gen && !c->rpar_widep && !c->rpar_no_constraint &&
            !jac)
            throw Unsupported("PARALLEL TransR: no pair-by-pair transRNorm at this width");
    }
    // tile descriptors: at most rpar_max_tiles a batch (the wave kernels' inputs; the
    // matrix-core tile kernels' entity ids, one load instead of key -> sample -> triple)
    if (c->rpar_cons_wave || c->rpar_mfma) {
        const size_t nt = (size_t)c->nbi * c->rpar_max_tiles + 1;
        c->rpar_batch_t0.alloc((size_t)(c->nbi + 1) * 4);
        c->rpar_td_r.alloc(nt * 4);
        c->rpar_td_cnt.alloc(nt * 4);
        c->rpar_td_kk.alloc(nt * 8 * 4);
        c->rpar_td_ent.alloc(nt * 32 * 4);
    } else {
        for (DevBuf* d : {&c->rpar_batch_t0, &c->rpar_td_r, &c->rpar_td_cnt, &c->rpar_td_kk, &c->rpar_td_ent}) d->free();
    }
    // sub-batches: phase A's second export set (the same sizes; merged phase A: none,
    // its sub-batches' exports lie side by side in the first set)
    {
        const std::pair<DevBuf*, DevBuf*> sets[] = {
            {&c->sb_x, &c->xreal}, {&c->sb_d, &c->aux}, {&c->sb_y, &c->rpar_y}, {&c->sb_wpart, &c->rpar_wpart},
            {&c->sb_rpart, &c->rpar_rpart}, {&c->sb_pflag, &c->rpar_pflag}, {&c->sb_cons_tile, &c->rpar_cons_tile},
            {&c->sb_cpairs, &c->rpar_cpairs}, {&c->sb_vio, &c->rpar_vio}, {&c->sb_cnrows, &c->rpar_cnrows}};
        for (const auto& pr : sets) {
            pr.first->free();
            if (c->sub > 1 && !c->rpar_merge_a && pr.second->p) {
                pr.first->alloc(pr.second->bytes);
                memset_sync(pr.first->p, 0, pr.first->bytes);
            }
        }
    }
    for (const void* k : {(const void*)rpar_scan_energy_kernel<double>, (const void*)rpar_scan_energy_kernel<float>,
                          (const void*)rpar_scan_energy_merged_kernel<double>,
                          (const void*)rpar_scan_energy_merged_kernel<float>,
                          (const void*)rpar_scan_energy_ahead_kernel<double>,
                          (const void*)rpar_scan_energy_ahead_kernel<float>,
                          (const void*)rpar_scan_energy_merged_ahead_kernel<double>,
                          (const void*)rpar_scan_energy_merged_ahead_kernel<float>})
        (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)rpar_scan_lds(c, true));
    // a refused limit above (an image no launch of this context uses) must not linger
    // as the sticky last error for the next launch check
    (void)hipGetLastError();
}

// Per epoch, after the event index: the tile list (relation segments cut into
// chunks of St samples) and the first relation segment of every batch.
void build_transr_tiles(kb2e_ctx* c, bool tiles, hipStream_t st, int set) {
    const int64_t nkeys = c->S * c->slots;
    rtile_count_kernel<<<1024, 256, 0, st>>>(c->keys_sorted.as<uint64_t>(), c->seg_start.as<int32_t>(),
                                                    c->nseg.as<int32_t>(), nkeys + 1, c->kl, c->cfg.num_entities,
                                                    c->rpar_St, c->rpar_ntiles.as<int32_t>(),
                                                    c->rpar_rel_begin.as<int32_t>());
    HIPCHK(hipGetLastError());
    if (!tiles) return;  // TransH: the first relation segment of each batch is all it needs
    size_t tb = c->sort_tmp_bytes;
    HIPCHK(hipcub::DeviceScan::ExclusiveSum(c->sort_tmp.p, tb, c->rpar_ntiles.as<int32_t>(),
                                            c->rpar_tile_first.as<int32_t>(), (int)(nkeys + 1), st));
    rtile_scatter_kernel<<<1024, 256, 0, st>>>(c->rpar_ntiles.as<int32_t>(), c->rpar_tile_first.as<int32_t>(),
                                                      c->nseg.as<int32_t>(), c->rpar_tiles.as<RTile>());
    HIPCHK(hipGetLastError());
    if (c->rpar_brel.p) {  // each batch's relations, most frequent first, and their count (host copy)
        rel_list_kernel<<<(int)c->nbi, 1024, 0, st>>>(c->rpar_rel_begin.as<int32_t>(), c->batch_seg.as<int32_t>(),
                                                     c->seg_row.as<int32_t>(), c->cfg.num_entities,
                                                     c->rel_order.as<int32_t>(), c->cfg.num_relations,
                                                     c->rpar_brel_cap, c->rpar_brel.as<int32_t>(),
                                                     c->rpar_bnrel.as<int32_t>(), c->seg_start.as<int32_t>(),
                                                     kRParLongMin);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(c->pin_bnrel, c->rpar_bnrel.p, (size_t)c->nbi * 3 * 4, hipMemcpyDeviceToHost, st));
    }
    if (c->rpar_td_r.p) {  // the wave kernels' tile descriptors
        RTileDescArgs d{};
        d.keys = c->keys_sorted.as<uint64_t>();
        d.seg_start = c->seg_start.as<int32_t>();
        d.seg_row = c->seg_row.as<int32_t>();
        d.tiles = c->rpar_tiles.as<RTile>();
        d.tile_first = c->rpar_tile_first.as<int32_t>();
        d.nseg = c->nseg.as<int32_t>();
        d.batch_seg = c->batch_seg.as<int32_t>();
        d.nb = (int32_t)c->nbi;
        d.sub = c->sub;
        d.Bs = (int32_t)c->Bs;
        d.St = c->rpar_St;
        d.ne = c->cfg.num_entities;
        d.B = (int32_t)c->B;
        d.kl = c->kl;
        d.si = c->si_[set].as<int32_t>();
        d.sj = c->sj_[set].as<int32_t>();
        d.side = c->side_[set].as<uint8_t>();
        d.heads = c->heads.as<int32_t>();
        d.tails = c->tails.as<int32_t>();
        d.batch_t0 = c->rpar_batch_t0.as<int32_t>();
        d.td_r = c->rpar_td_r.as<int32_t>();
        d.td_cnt = c->rpar_td_cnt.as<int32_t>();
        d.td_kk = c->rpar_td_kk.as<int32_t>();
        d.td_ent = c->rpar_td_ent.as<int32_t>();
        rtile_desc_kernel<<<2048, 256, 0, st>>>(d);
        HIPCHK(hipGetLastError());
    }
}

// buffer set 0 or 1 of a double-buffered export (sub-batches)
DevBuf& buf_set(int set, DevBuf& s0, DevBuf& s1) { return set ? s1 : s0; }

// sub-batches: phase A on its own stream beside phase B (KB2E_SUB_OVERLAP=0: everything
// in line on the batch stream, A/B and tests; read at every batch)
bool sub_overlap_on() {
    const char* e = getenv("KB2E_SUB_OVERLAP");
    return !(e && e[0] == '0');
}

// pipelined chain kernel: the steps outside its violator loop (a bit each: kPipeOptHandover,
// kPipeOptDefer, kPipeOptPublish; default all, KB2E_RPAR_PIPE_OPT=0 the path before them: A/B and
// the bit comparisons of the tests; read at every batch)
int32_t pipe_opt_bits() {
    const char* e = getenv("KB2E_RPAR_PIPE_OPT");
    return e && e[0] ? (int32_t)(atoi(e) & kPipeOptAll) : kPipeOptAll;
}

// the entity rows' y-row fetch and the gradient kernel's partial stores (a bit each: kRowsOptDeep,
// kRowsOptStore; default all, KB2E_RPAR_ROWS_OPT=0 the path before them: A/B and the bit comparisons
// of the tests; read at every batch)
int32_t rows_opt_bits() {
    const char* e = getenv("KB2E_RPAR_ROWS_OPT");
    return e && e[0] ? (int32_t)(atoi(e) & kRowsOptAll) : kRowsOptAll;
}

// the entity passes' wave-a-segment form and the compat energy launch's loads ahead of its barriers (a bit
// each: kPassOptRound, kPassOptScan; default all, KB2E_RPAR_PASS_OPT=0 the path before them: A/B and the bit
// comparisons of the tests; read at every batch)
int32_t pass_opt_bits() {
    const char* e = getenv("KB2E_RPAR_PASS_OPT");
    return e && e[0] ? (int32_t)(atoi(e) & kPassOptAll) : kPassOptAll;
}

// KB2E_RPAR_INDEX_STATS (tools): the epoch's index batches in figures, one line to stderr an epoch -- mean,
// minimum and maximum over the index batches of the entity segments, of those with kRParLongMin events or
// more, of the relations, and of the relation-row waves with a relation (four rows a wave for n <= 64)
void rpar_index_stats(const kb2e_ctx* c) {
    const int64_t nb = c->nbi;
    const int rw = c->n <= 64 ? (c->n + 4) / 4 : c->n + 1;
    const char* names[4] = {"entity segments", "segments >= 128 events", "relations", "relation-row waves"};
    fprintf(stderr, "rpar index: %lld index batches", (long long)nb);
    for (int k = 0; k < 4; ++k) {
        const int32_t* p = c->pin_bnrel + (k == 0 ? nb : k == 1 ? 2 * nb : 0);
        int64_t sum = 0, lo = INT64_MAX, hi = 0;
        for (int64_t b = 0; b < nb; ++b) {
            const int64_t v = (int64_t)p[b] * (k == 3 ? rw : 1);
            sum += v;
            lo = std::min(lo, v);
            hi = std::max(hi, v);
        }
        fprintf(stderr, "; %s mean %.1f min %lld max %lld", names[k], nb ? (double)sum / nb : 0.0, (long long)lo,
                (long long)hi);
    }
    fprintf(stderr, "\n");
}

// kPipeOptDefer: the chunks from which a relation defers its records (KB2E_RPAR_REC_DEFER; 0: none
// does, 1: every relation with a pair, tests; the results do not depend on it; read at every batch)
constexpr int32_t kRecDeferChunks = 12;  // (swept 4 / 8 / 12 / 16 on the bench: DESIGN.md 7, round 11)
int32_t rec_defer_chunks() {
    const char* e = getenv("KB2E_RPAR_REC_DEFER");
    return e && e[0] ? std::max(0, atoi(e)) : kRecDeferChunks;
}

// The kernel arguments of sub-batch j of batch b (the whole batch when c->sub == 1), its
// exports in buffer set `set`; all but the pair-dedupe tables and the stamp.
template <typename T>
void fill_rpar(kb2e_ctx* c, int64_t b, int j, int set, RParArgs& a, RParBufs<T>& bf) {
    const int64_t ib = b * c->sub + j;                   // index batch
    const int64_t first = b * c->B + (int64_t)j * c->Bs;  // its first sample
    const int64_t cnt = std::min<int64_t>(c->Bs, c->B - (int64_t)j * c->Bs);
    a = RParArgs{};
    a.heads = c->heads.as<int32_t>();
    a.tails = c->tails.as<int32_t>();
    a.rels = c->rels.as<int32_t>();
    a.si = c->si() + first;
    a.sj = c->sj() + first;
    a.side = c->side() + first;
    a.B = (int32_t)cnt;
    a.n = c->n;
    a.ld = c->ld;
    a.ne = c->cfg.num_entities;
    a.nr = c->cfg.num_relations;
    a.St = c->rpar_St;
    a.tgroup = c->rpar_tgroup;
    a.batch = (int32_t)ib;
    a.lr = c->cfg.learning_rate;
    a.margin = c->cfg.margin;
    a.compat = c->cfg.transr_compat;
    a.l1 = c->cfg.distance == 0;
    a.keys = c->keys_sorted.as<uint64_t>();
    a.seg_start = c->seg_start.as<int32_t>();
    a.batch_seg = c->batch_seg.as<int32_t>();
    a.seg_row = c->seg_row.as<int32_t>();
    a.rel_begin = c->rpar_rel_begin.as<int32_t>();
    a.tile_first = c->rpar_tile_first.as<int32_t>();
    a.tiles = c->rpar_tiles.as<RTile>();
    a.kl = c->kl;
    a.act = c->act.as<uint8_t>() + first;
    a.loss = c->loss.as<double>() + first;
    a.proj = c->aux2.as<double>();
    a.tile_act = c->rpar_tile_act.as<int32_t>();
    a.batch_t0 = c->rpar_batch_t0.as<int32_t>();
    a.td_r = c->rpar_td_r.as<int32_t>();
    a.td_cnt = c->rpar_td_cnt.as<int32_t>();
    a.td_kk = c->rpar_td_kk.as<int32_t>();
    a.td_ent = c->rpar_td_ent.as<int32_t>();
    a.brel = c->rpar_brel.as<int32_t>() + ib * c->rpar_brel_cap;
    a.nrel = c->pin_bnrel[ib];
    if (a.nrel < 1 || a.nrel > c->rpar_brel_cap) throw std::logic_error("batch relation count out of range");
    bf = RParBufs<T>{};
    bf.ent = c->ent.as<T>();
    bf.rel = c->rel.as<T>();
    bf.W = c->w.as<T>();
    bf.x = buf_set(set, c->xreal, c->sb_x).as<T>();
    bf.d = buf_set(set, c->aux, c->sb_d).as<T>();
    bf.y = buf_set(set, c->rpar_y, c->sb_y).as<T>();
    bf.wpart = buf_set(set, c->rpar_wpart, c->sb_wpart).as<T>();
    bf.rpart = buf_set(set, c->rpar_rpart, c->sb_rpart).as<T>();
    bf.pair = c->rpar_pair.as<T>();
    bf.relpair = c->rpar_relpair.as<T>();
    bf.relpair_stamp = c->rpar_relpair_stamp.as<uint32_t>();
    bf.err = c->dataflow_err.as<uint32_t>() + 1;
    bf.rows_opt = rows_opt_bits();
    bf.pass_opt = pass_opt_bits();
    if (c->rpar_mfma) {
        bf.pflag = buf_set(set, c->rpar_pflag, c->sb_pflag).as<uint8_t>();
        bf.cons_tile = buf_set(set, c->rpar_cons_tile, c->sb_cons_tile).as<int32_t>();
        bf.cons_ppt = c->rpar_cons_wave ? kConsPpt : 1;
        bf.cpairs = buf_set(set, c->rpar_cpairs, c->sb_cpairs).as<int32_t>();
        bf.vio = buf_set(set, c->rpar_vio, c->sb_vio).as<int32_t>();
        bf.cnrows = buf_set(set, c->rpar_cnrows, c->sb_cnrows).as<int32_t>();
        bf.stats = getenv("KB2E_RPAR_STATS") != nullptr;
        bf.last_renorm = c->rpar_cons_seq ? 1 : 0;
        if (const char* dbg = getenv("KB2E_CONS_DBG")) bf.dbg = atoi(dbg);  // timing experiments only
        if (const char* cl = getenv("KB2E_RPAR_CHAIN_LIST")) bf.chain_list = std::max(64, atoi(cl));  // tests
        if (const char* ct = getenv("KB2E_RPAR_CHAIN_TILES")) bf.chain_tiles = std::max(1, atoi(ct));  // tests
        if (const char* rc = getenv("KB2E_RPAR_REC_CAP")) bf.rec_cap = std::max(4, atoi(rc));  // tests
        bf.pipe_opt = pipe_opt_bits();
        if (c->rpar_cons_seq) {  // the pipelined chain: long relations leave their records to the entity pass
            bf.rec_stamp = bf.relpair_stamp + c->cfg.num_relations;
            bf.rec_defer = rec_defer_chunks();
        }
    }
    if (c->rpar_cons_wide || c->rpar_cons_gen || c->rpar_widep) {  // the chains past n = 64: pair flags, pre / post split
        bf.pflag = buf_set(set, c->rpar_pflag, c->sb_pflag).as<uint8_t>();
        if (const char* dbg = getenv("KB2E_CONS_DBG")) bf.dbg = atoi(dbg);  // timing experiments only
        bf.stats = getenv("KB2E_RPAR_STATS") != nullptr;
        bf.last_renorm = 1;
    }
}

template <typename T>
void transr_phase_b(kb2e_ctx* c, RParArgs a, RParBufs<T> bf);

// One index batch: sub-batch j of batch b (the whole batch when c->sub == 1).  Phase
// A (energies, hinge, directions, the matrix partials) reads the tables bfa names
// -- the start-of-batch copies when the batch runs in sub-batches -- and phase B
// applies the sub-batch's sums, norms and transRNorm pairs to the live tables.
template <typename T>
void run_subbatch_transr_parallel(kb2e_ctx* c, int64_t b, int j) {
    // sub-batches: phase A of sub-batch j >= 1 on its own stream (it reads the
    // start-of-batch copies, so it runs beside phase B of sub-batch j - 1), its exports
    // in buffer set j & 1 (the set phase B of sub-batch j - 2 no longer reads); phase A
    // of sub-batch 0 in line on the batch stream (a wait across queues costs ~12 us:
    // r23 timeline)
    const bool ov = c->sub > 1 && sub_overlap_on();
    const bool side = ov && j > 0;
    const int set = ov ? (j & 1) : 0;
    hipStream_t sa = side ? c->suba_stream : c->stream;
    RParArgs a;
    RParBufs<T> bf;
    fill_rpar<T>(c, b, j, set, a, bf);
    {  // this batch's pair-dedupe table and the next one's (batches alternate)
        unsigned long long* t0 = c->rpar_ptab.as<unsigned long long>();
        const size_t sz = (size_t)c->rpar_ptab_mask + 1;
        // (three tables in rotation: the one a sub-batch's phase A inserts into, the one
        // phase B of the sub-batch before it may still read, the next one it clears)
        a.ptab = t0 + (c->batch_stamp % 3) * sz;
        a.ptab_next = t0 + ((c->batch_stamp + 1) % 3) * sz;
        a.ptab_mask = c->rpar_ptab_mask;
    }
    bf.stamp = ++c->batch_stamp;
    RParBufs<T> bfa = bf;  // phase A's tables: the start-of-batch copies in sub-batch mode
    if (c->sub > 1) {
        bfa.ent = c->snap_ent.as<T>();
        bfa.rel = c->snap_rel.as<T>();
        bfa.W = c->snap_w.as<T>();
    }
    // the side stream's phase A: sub-batch 1's after sub-batch 0's (the compat scan's
    // carried work vectors, the pair-table rotation; the copies are before both), later
    // ones after phase B of the sub-batch two before (its buffer set); phase B waits
    // for its phase A
    if (side && j == 1) HIPCHK(hipStreamWaitEvent(sa, c->ev_adone[0], 0));
    if (side && j >= 2) HIPCHK(hipStreamWaitEvent(sa, c->ev_bdone[set], 0));
    auto a_done = [&] {
        if (!ov) return;
        HIPCHK(hipEventRecord(c->ev_adone[set], sa));
        if (side) HIPCHK(hipStreamWaitEvent(c->stream, c->ev_adone[set], 0));
    };
    auto b_done = [&] {
        if (ov) HIPCHK(hipEventRecord(c->ev_bdone[set], c->stream));
    };
    if (c->rpar_widep) {  // 128 < n <= 512: the wide kernels take the whole step
        c->timed_on(sa, "score", [&] {
            wide_phase_a<T>(a, bfa, c->rpar_wg, c->rpar_max_tiles, c->rpar_scan.as<double>(),
                            c->rpar_scan_pre.as<double>(), c->transr_work.as<double>(),
                            c->transr_work_alt.as<double>(), sa);
        });
        if (c->cfg.transr_compat) std::swap(c->transr_work.p, c->transr_work_alt.p);  // carried work vectors
        a_done();
        c->timed("apply", [&] {
            wide_phase_b<T>(a, bf, c->rpar_wg, c->rpar_wsc.as<double>(), !c->rpar_no_constraint,
                            (int)std::min<int64_t>(c->cfg.num_relations, c->Bs), c->stream);
        });
        b_done();
        if (c->pending.size() > 4096) c->flush_timers();
        return;
    }
    const size_t lds = rpar_lds<T>(c);
    const int tgrid = c->rpar_max_tiles;
    const bool mf = c->rpar_mfma;
    const size_t lt = mf ? rmfma_lds<T>(c, false) : lds;
    const int tb = mf ? c->rpar_tile_threads : 256;
    auto tile = [&](auto proj, auto grad) {
        constexpr bool P = decltype(proj)::value, G = decltype(grad)::value;
        if (mf) {
            void* args[] = {&a, &bfa};
            // a projection-only launch shares nothing across tiles: four-wave blocks, more
            // of them a CU to overlap their latency chains (KB2E_RPAR_PROJ_THREADS=512: eight)
            int pt = tb;
            if (P && !G) {
                pt = 256;
                if (const char* e = getenv("KB2E_RPAR_PROJ_THREADS")) pt = atoi(e) >= 512 ? 512 : 256;
            }
            HIPCHK(hipLaunchKernel(tile_fn<T, P, G>(rm_np(c->n) / 16), dim3(tgrid), dim3(pt), args,
                                   rmfma_tile_lds<T>(c->n, c->rpar_St, P, G), sa));
        } else {
            transr_tile_kernel<T, P, G><<<tgrid, tb, lt, sa>>>(a, bfa);
        }
        HIPCHK(hipGetLastError());
    };
    using yes = std::true_type;
    using no = std::false_type;
    // the pair-dedupe table is filled where the hinge is decided (rpar_scan_energy,
    // transr_proj_wave); the fixed-energy tile kernels need the separate pass
    auto pair_first = [&] {
        if (c->rpar_no_constraint) return;
        transr_pair_first_kernel<<<(int)((4 * c->B + 255) / 256), 256, 0, sa>>>(a);
        HIPCHK(hipGetLastError());
    };
    c->timed_on(sa, "score", [&] {
        if (c->cfg.transr_compat) {
            if (c->rpar_cons_wave) proj_wave_launch<T>(a, bfa, tgrid, sa);
            else tile(yes(), no());
            const int64_t calls = 2 * (int64_t)a.B;  // (this sub-batch's calls: the carry must not see stale ones)
            const int nchunks = (int)((calls + kScanChunk - 1) / kScanChunk);
            rpar_scan_sums_kernel<<<nchunks, 256, 0, sa>>>(a.proj, calls, c->ld, c->n,
                                                                  c->rpar_scan.as<double>());
            // many chunks (K5): their prefix once (KB2E_RPAR_SCAN_PREFIX=1 / 0 forces it on / off: tests)
            const char* sp = getenv("KB2E_RPAR_SCAN_PREFIX");
            const bool use_pre = sp ? sp[0] == '1' : nchunks > kScanDirectMax;
            double* pre = nullptr;
            if (use_pre) {
                pre = c->rpar_scan_pre.as<double>();
                rpar_scan_prefix_kernel<<<(2 * c->n + 31) / 32, 1024, 0, sa>>>(
                    c->rpar_scan.as<double>(), nchunks, 2 * c->n, c->transr_work.as<double>(), pre);
            }
            if (rpar_scan_ahead_slots(bfa.pass_opt, c->n, 0) == 1)  // kPassOptScan, n <= 64
                rpar_scan_energy_ahead_kernel<T><<<nchunks, 1024, rpar_scan_lds(c, true), sa>>>(
                    a, bfa, c->rpar_scan.as<double>(), nchunks, c->transr_work.as<double>(),
                    c->transr_work_alt.as<double>(), pre);
            else
                rpar_scan_energy_kernel<T><<<nchunks, 1024, rpar_scan_lds(c), sa>>>(
                    a, bfa, c->rpar_scan.as<double>(), nchunks, c->transr_work.as<double>(),
                    c->transr_work_alt.as<double>(), pre);
            HIPCHK(hipGetLastError());
            std::swap(c->transr_work.p, c->transr_work_alt.p);  // the carried work vectors, ping-pong
            if (c->rpar_cons_wave) grad_wave_launch<T>(a, bfa, tgrid, sa);
            else tile(no(), yes());
        } else if (c->rpar_cons_wave) {  // projections + hinge, then the partials from the exports
            proj_wave_launch<T>(a, bfa, tgrid, sa);
            grad_wave_launch<T>(a, bfa, tgrid, sa);
        } else {
            tile(yes(), yes());
            pair_first();
        }
    });
    a_done();
    transr_phase_b<T>(c, a, bf);
    b_done();
    if (c->pending.size() > 4096) c->flush_timers();
}

// Phase B of one index batch on the batch stream: its sums, norms and transRNorm pairs
// applied to the live tables (the tile and chain paths below 128 < n's wide kernels).
template <typename T>
void transr_phase_b(kb2e_ctx* c, RParArgs a, RParBufs<T> bf) {
    // (merged phase A: a sub-batch's tile slots, the next one's follow them)
    const int tgrid = c->rpar_merge_a ? c->rpar_merge.tcap : c->rpar_max_tiles;
    const int rel_waves = (int)std::min<int64_t>(c->cfg.num_relations, c->B) * (c->n + 1);
    const int rgrid = (rel_waves + 3) / 4;
    const int egrid = 256;
    const bool mf = c->rpar_mfma;
    const size_t lc = mf ? rmfma_lds<T>(c, true) : rpar_lds<T>(c);
    // phase B (five kernels) timed as one span, from the first kernel's start
    // to the last one's end; rocprofv3 has the split
    hipEvent_t e0, e1;
    c->ev_begin("apply", e0);
    // the relation rows and the entity rows of a pass touch disjoint tables: one launch
    // for the gradient pass (KB2E_RPAR_FUSE=0: two; the transRNorm pass is faster as
    // two: its entity part is short and the 1024-thread relation blocks place worse)
    const char* fz = getenv("KB2E_RPAR_FUSE");
    const bool fuse = !(fz && fz[0] == '0');
    // four relation rows a wave (transr_rel_rows4_wave): four elements a lane for n <= 64;
    // KB2E_RPAR_ROWS8=1: eight a lane up to n = 128 (A/B: K5 1.38 against 1.29 ms a row
    // a wave, r21 -- the hot relations' long partial lists dominate, not the wave count)
    const char* r8 = getenv("KB2E_RPAR_ROWS8");
    const int rmode = c->n <= 64 ? 4 : (c->n <= 128 && r8 && r8[0] == '1') ? 8 : 0;
    const bool rows4 = rmode != 0;
    const int rel_waves4 = (int)std::min<int64_t>(c->cfg.num_relations, c->B) * ((c->n + 4) / 4);
    const int rw = rows4 ? rel_waves4 : rel_waves;
    const int fgrid = egrid + (rw + 15) / 16;
    auto rows_fn = [&](auto pass1) {
        constexpr bool P = decltype(pass1)::value;
        return rmode == 4 ? transr_rows_kernel<T, P, 4> : rmode == 8 ? transr_rows_kernel<T, P, 8>
                                                                     : transr_rows_kernel<T, P, 0>;
    };
    using yes1 = std::true_type;
    // kPassOptRound: 256-thread workgroups, a wave a short entity segment, a workgroup for every four entity
    // segments of the index batch (their count came to the host with the index, behind the relation counts);
    // the fused launches' relation-row workgroups follow, four waves each
    // -- while the segments are a few rounds of the GPU's waves at the most: with many more, workgroups that
    // stride over the segments win (K5, ~144,000 segments an index batch: 17.5 ms a batch against 18.3 in this
    // form; ~5,100 and ~8,000, the FB15k shape at k = 2 and 1, gain; between them nobody has measured:
    // DESIGN.md 7, round 13)
    constexpr int kRoundSegMax = 4 * 256 * kRParWaves;  // four times the waves of the grid before
    const int nseg_ent = c->pin_bnrel[c->nbi + a.batch];
    if (nseg_ent < 0 || nseg_ent > (int64_t)c->B * c->slots)
        throw std::logic_error("batch entity segment count out of range");
    const bool round1 = (bf.pass_opt & kPassOptRound) != 0 && nseg_ent <= kRoundSegMax;
    const int egrid4 = std::max(1, (nseg_ent + kEntWaves - 1) / kEntWaves);
    const int fgrid4 = egrid4 + (rw + 3) / 4;
    auto rows4_fn = [&](auto pass1) {
        constexpr bool P = decltype(pass1)::value;
        return rmode == 4 ? transr_rows4_kernel<T, P, 4> : rmode == 8 ? transr_rows4_kernel<T, P, 8>
                                                                     : transr_rows4_kernel<T, P, 0>;
    };
    auto entity_launch = [&](auto grad, hipEvent_t ev1) {  // the entity rows alone
        constexpr bool G = decltype(grad)::value;
        if (round1) c->launch(transr_entity4_kernel<T, G>, dim3(egrid4), dim3(256), 0, nullptr, ev1, a, bf, kRParLongMin);
        else c->launch(transr_entity_kernel<T, G>, dim3(egrid), dim3(1024), 0, nullptr, ev1, a, bf, kRParLongMin);
    };
    auto rows_launch = [&](auto pass1, hipEvent_t ev0, hipEvent_t ev1) {  // the fused launch of a pass
        if (round1) c->launch(rows4_fn(pass1), dim3(fgrid4), dim3(256), 0, ev0, ev1, a, bf, kRParLongMin, egrid4);
        else c->launch(rows_fn(pass1), dim3(fgrid), dim3(1024), 0, ev0, ev1, a, bf, kRParLongMin, egrid);
    };
    if (c->rpar_no_constraint) {
        c->ev_end(e1);
        rows_launch(yes1(), e0, e1);
        return;
    }
    if (fuse) {
        rows_launch(yes1(), e0, nullptr);
    } else {
        c->launch(transr_rel_rows_kernel<T, true>, dim3(rgrid), dim3(256), 0, e0, nullptr, a, bf);
        entity_launch(yes1(), nullptr);
    }
    if (mf && c->rpar_cons_seq) {
        if constexpr (std::is_same<T, double>::value) cons_seq_launch(a, bf, c->rpar_seq_lds, c->stream);
    } else if (c->rpar_cons_gen) {
        cons_chaing_launch<T>(a, bf, c->rpar_gen_lds, c->stream);
    } else if (c->rpar_cons_wide) {
        if constexpr (std::is_same<T, double>::value) cons_chainw_launch(a, bf, c->rpar_wide_lds, c->stream);
    } else if (mf && c->rpar_cons_wave) {
        cons_wave_launch<T>(a, bf, tgrid, c->rpar_cons_lds, c->stream);
    } else if (mf) {
        void* args[] = {&a, &bf};
        HIPCHK(hipLaunchKernel(cons_tile_fn<T>(rm_np(c->n) / 16), dim3(tgrid), dim3(512), args, lc, c->stream));
    } else {
        transr_constraint_kernel<T><<<tgrid, 256, lc, c->stream>>>(a, bf);
    }
    HIPCHK(hipGetLastError());
    c->ev_end(e1);
    const char* f2 = getenv("KB2E_RPAR_FUSE2");
    if (c->rpar_cons_seq || c->rpar_cons_wide || c->rpar_cons_gen) {  // the matrices are final: only the entity rows take pair records
        entity_launch(std::false_type(), e1);
    } else if (f2 && f2[0] == '1') {
        rows_launch(std::false_type(), nullptr, e1);
    } else {
        if (rmode == 4) transr_rel_rows4_kernel<T, false, 4><<<(rel_waves4 + 3) / 4, 256, 0, c->stream>>>(a, bf);
        else if (rmode == 8) transr_rel_rows4_kernel<T, false, 8><<<(rel_waves4 + 3) / 4, 256, 0, c->stream>>>(a, bf);
        else transr_rel_rows_kernel<T, false><<<rgrid, 256, 0, c->stream>>>(a, bf);
        HIPCHK(hipGetLastError());
        entity_launch(std::false_type(), e1);
    }
}

// A batch of sub-batches on the n <= 64 wave path: phase A of all of them once, in line
// on the live tables -- the values every sub-batch's phase A reads, since no phase B of
// the batch has run yet -- then phase B of sub-batch 0 .. sub - 1; one stream, no copies.
// Sub-batch j's exports lie at the strides of rpar_sub_view in the first buffer set.
template <typename T>
void run_batch_transr_merged(kb2e_ctx* c, int64_t b) {
    const RParMerge& m = c->rpar_merge;
    RParArgs a0;
    RParBufs<T> bf0;
    fill_rpar<T>(c, b, 0, 0, a0, bf0);
    {  // the batch's group of pair-dedupe tables, and the other one, which its inserting launch clears
        unsigned long long* t0 = c->rpar_ptab.as<unsigned long long>();
        const size_t gsz = (size_t)m.sub * ((size_t)c->rpar_ptab_mask + 1);
        const uint32_t grp = c->rpar_merge_batches++ & 1;
        a0.ptab = t0 + grp * gsz;
        a0.ptab_next = t0 + (grp ^ 1) * gsz;
        a0.ptab_mask = c->rpar_ptab_mask;
    }
    c->timed("score", [&] {
        proj_wave_merged_launch<T>(a0, bf0, m, c->stream);
        if (c->cfg.transr_compat) {
            const int last = (int)((2 * (int64_t)m.Blast + kScanChunk - 1) / kScanChunk);
            const int grid = (m.sub - 1) * m.nch + last;
            rpar_scan_sums_merged_kernel<<<grid, 256, 0, c->stream>>>(a0.proj, m, c->ld, c->n,
                                                                         c->rpar_scan.as<double>());
            // kPassOptScan: when the last sub-batch's blocks can take their slots (at most two a thread)
            if (rpar_scan_ahead_slots(bf0.pass_opt, c->n, m.sub - 1))
                rpar_scan_energy_merged_ahead_kernel<T><<<grid, 1024, rpar_scan_lds(c, true), c->stream>>>(
                    a0, bf0, m, c->rpar_scan.as<double>(), c->transr_work.as<double>(),
                    c->transr_work_alt.as<double>());
            else
                rpar_scan_energy_merged_kernel<T><<<grid, 1024, rpar_scan_lds(c), c->stream>>>(
                    a0, bf0, m, c->rpar_scan.as<double>(), c->transr_work.as<double>(),
                    c->transr_work_alt.as<double>());
            HIPCHK(hipGetLastError());
            std::swap(c->transr_work.p, c->transr_work_alt.p);  // the carried work vectors: one ping-pong a batch
        }
        grad_wave_merged_launch<T>(a0, bf0, m, c->stream);
    });
    for (int j = 0; j < m.sub; ++j) {
        RParArgs a = a0;
        RParBufs<T> bf = bf0;
        rpar_sub_view(a, bf, m, j);
        a.nrel = c->pin_bnrel[b * c->sub + j];
        if (a.nrel < 1 || a.nrel > c->rpar_brel_cap) throw std::logic_error("batch relation count out of range");
        bf.stamp = ++c->batch_stamp;
        transr_phase_b<T>(c, a, bf);
    }
    if (c->pending.size() > 4096) c->flush_timers();
}

template <typename T>
void run_batch_transr_parallel(kb2e_ctx* c, int64_t b) {
    if (c->rpar_merge_a) {
        run_batch_transr_merged<T>(c, b);
        return;
    }
    if (c->sub > 1) {  // the start-of-batch tables for every sub-batch's phase A
        // (made on the side stream beside phase A of sub-batch 0, which then read the live
        // tables, they gained nothing: DESIGN.md section 7 round 8)
        for (auto pr : {std::make_pair(&c->snap_ent, &c->ent), std::make_pair(&c->snap_rel, &c->rel),
                        std::make_pair(&c->snap_w, &c->w)})
            HIPCHK(hipMemcpyAsync(pr.first->p, pr.second->p, pr.second->bytes, hipMemcpyDeviceToDevice, c->stream));
    }
    for (int j = 0; j < c->sub; ++j) run_subbatch_transr_parallel<T>(c, b, j);
}

}  // namespace
