// engine_merge.inc -- the multi-GPU epoch merge behind the C ABI (included at
// the end of engine.hip; SURVEY.md 8(e), include/kb2e_engine.h "Multi-GPU").
//
// Every rank trains its head-hash shard of the triples on a full replica of
// the tables (the single-GPU schedule); at an epoch boundary the ranks merge
//
//     T <- renorm(T0 + sum_r (T_r - T0))
//
// with all the work on each context's own stream (no cross-stream hazards,
// no host round trip):
//   1. deltas: entity deltas into the reduce-scatter buffer, relation / weight
//      deltas in place;
//   2. RCCL: a reduce-scatter of the entity deltas to the owner of each block
//      of rows, an all-reduce (sum) of the relation and weight deltas (one
//      ncclGroup);
//   3. each owner adds the summed deltas to its block and renormalises the units
//      whose summed delta has a non-zero element (the model's constraint,
//      renorm_rows; a row whose deltas cancel exactly is left as it was); every
//      rank does the same for the relations and weights (identical sums everywhere);
//   4. RCCL: an all-gather of the owners' blocks;
//   5. the merged tables become the next epoch's base.
// The collectives come either from RCCL -- one communicator per rank
// (kb2e_comm_init_rank: one process per GPU) or one per device of an
// in-process group (kb2e_comm_init_group: ncclCommInitAll, one host thread
// driving every device) -- or, for contexts sharing a device (RCCL refuses two
// ranks on one GPU: the one-GPU test box), from plain kernels over the
// group's buffers ("local" backend).  Both backends run the same phases.
#include <rccl/rccl.h>

struct MergeState {
    ncclComm_t comm = nullptr;
    bool local = false;  // in-process group without RCCL (contexts on shared devices)
    int nranks = 1, rank = 0;
    int64_t block = 0, lo = 0, hi = 0;  // entity rows per owner; this rank's [lo, hi)
    DevBuf base[3], send, recv, mask, tmp;
    ~MergeState() {
        if (comm) (void)ncclCommDestroy(comm);
    }
};

void merge_free(MergeState* m) { delete m; }

namespace {

#define NCCLCHK(expr)                                                                                 \
    do {                                                                                              \
        ncclResult_t _r = (expr);                                                                     \
        if (_r != ncclSuccess)                                                                        \
            throw ::kb2e::HipError(std::string(#expr) + ": " + ncclGetErrorString(_r) + " @" +        \
                                   std::string(__FILE__) + ":" + std::to_string(__LINE__));           \
    } while (0)

constexpr int kLocalMaxRanks = 16;

template <typename T>
struct SrcList {
    const T* p[kLocalMaxRanks];
};

template <typename T>
__global__ __launch_bounds__(256) void merge_delta_kernel(T* __restrict__ out, const T* __restrict__ cur,
                                                          const T* __restrict__ base, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = cur[i] - base[i];
}

// dst = base + sum; mask[unit] = 1 for every unit with a non-zero summed delta
// (mask zeroed before; the racing stores all write 1)
template <typename T>
__global__ __launch_bounds__(256) void merge_apply_kernel(T* dst, const T* __restrict__ base, const T* sum, int64_t n,
                                                          int64_t unit_len, uint8_t* __restrict__ mask) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const T s = sum[i];
        dst[i] = base[i] + s;
        if (s != T(0)) mask[i / unit_len] = 1;
    }
}

// local backend: out = sum over the ranks' buffers, in rank order
template <typename T>
__global__ __launch_bounds__(256) void merge_sum_kernel(T* __restrict__ out, SrcList<T> src, int nsrc, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        T s = src.p[0][i];
        for (int k = 1; k < nsrc; ++k) s += src.p[k][i];
        out[i] = s;
    }
}

int merge_grid(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 8192)); }

int merge_ntab(const kb2e_ctx* c) { return c->cfg.model == KB2E_TRANSE ? 2 : 3; }

DevBuf& merge_table(kb2e_ctx* c, int t) { return t == 0 ? c->ent : t == 1 ? c->rel : c->w; }

int64_t merge_units(const kb2e_ctx* c, int t) { return t == 0 ? c->cfg.num_entities : c->cfg.num_relations; }

// elements per unit (row; TransR weights: the n x ld matrix of a relation)
int64_t merge_unit_len(const kb2e_ctx* c, int t) {
    return t == 2 && c->cfg.model == KB2E_TRANSR ? (int64_t)c->n * c->ld : c->ld;
}

int64_t merge_elems(const kb2e_ctx* c, int t) { return merge_units(c, t) * merge_unit_len(c, t); }

ncclDataType_t merge_type(const kb2e_ctx* c) { return c->f64() ? ncclDouble : ncclFloat; }

template <class F>
void typed(const kb2e_ctx* c, F&& f) {
    if (c->f64()) f(double());
    else f(float());
}

void merge_check_group(kb2e_ctx* const* cs, int n) {
    for (int k = 0; k < n; ++k) {
        if (!cs[k]) throw std::invalid_argument("null context in the group");
        if (!cs[k]->have_params) throw std::invalid_argument("upload or init the tables before kb2e_comm_init");
        const kb2e_config &a = cs[0]->cfg, &b = cs[k]->cfg;
        if (a.model != b.model || a.dim != b.dim || a.num_entities != b.num_entities ||
            a.num_relations != b.num_relations || a.precision != b.precision)
            throw std::invalid_argument("the group's contexts differ in model / dim / table sizes / precision");
    }
}

// buffers of one rank once its communicator (or local group slot) is known
void merge_setup(kb2e_ctx* c, MergeState* m) {
    TallyScope ts(&c->device_bytes);  // (a group's setup runs under another context's entry point)
    const int64_t ne = c->cfg.num_entities, ld = c->ld;
    const size_t es = (size_t)c->esize;
    m->block = (ne + m->nranks - 1) / m->nranks;
    m->lo = std::min<int64_t>(ne, m->rank * m->block);
    m->hi = std::min<int64_t>(ne, m->lo + m->block);
    m->send.alloc((size_t)m->block * m->nranks * ld * es);
    HIPCHK(hipMemsetAsync(m->send.p, 0, m->send.bytes, c->stream));  // rows past |E| stay zero
    m->recv.alloc((size_t)m->block * ld * es);
    m->mask.alloc((size_t)std::max<int64_t>(ne, c->cfg.num_relations));
    for (int t = 0; t < merge_ntab(c); ++t) m->base[t].alloc((size_t)merge_elems(c, t) * es);
}

// the tables after a broadcast / merge become the base of the next epoch's deltas
void merge_snapshot(kb2e_ctx* c) {
    MergeState* m = c->mg;
    for (int t = 0; t < merge_ntab(c); ++t)
        HIPCHK(hipMemcpyAsync(m->base[t].p, merge_table(c, t).p, (size_t)merge_elems(c, t) * c->esize,
                              hipMemcpyDeviceToDevice, c->stream));
}

void merge_finish(kb2e_ctx* c) {
    HIPCHK(hipStreamSynchronize(c->stream));
    sync_wsnap(c);  // TransR: the committed matrices follow
}

void merge_sync_all(kb2e_ctx* const* cs, int n) {
    for (int k = 0; k < n; ++k) {
        HIPCHK(hipSetDevice(cs[k]->cfg.device));
        HIPCHK(hipStreamSynchronize(cs[k]->stream));
    }
}

// rank 0's tables to every rank (the ranks may have drawn different init streams)
void merge_broadcast(kb2e_ctx* const* cs, int n) {
    MergeState* m0 = cs[0]->mg;
    if (m0->local) {
        merge_sync_all(cs, n);
        for (int k = 1; k < n; ++k) {
            HIPCHK(hipSetDevice(cs[k]->cfg.device));
            for (int t = 0; t < merge_ntab(cs[k]); ++t)
                HIPCHK(hipMemcpy(merge_table(cs[k], t).p, merge_table(cs[0], t).p,
                                 (size_t)merge_elems(cs[k], t) * cs[k]->esize, hipMemcpyDefault));
        }
        return;
    }
    NCCLCHK(ncclGroupStart());
    for (int k = 0; k < n; ++k) {
        kb2e_ctx* c = cs[k];
        HIPCHK(hipSetDevice(c->cfg.device));
        for (int t = 0; t < merge_ntab(c); ++t) {
            void* p = merge_table(c, t).p;
            NCCLCHK(ncclBroadcast(p, p, (size_t)merge_elems(c, t), merge_type(c), 0, c->mg->comm, c->stream));
        }
    }
    NCCLCHK(ncclGroupEnd());
}

// phase 1: deltas
void merge_deltas(kb2e_ctx* c) {
    MergeState* m = c->mg;
    typed(c, [&](auto tag) {
        using T = decltype(tag);
        const int64_t ne = merge_elems(c, 0);
        merge_delta_kernel<T><<<merge_grid(ne), 256, 0, c->stream>>>(m->send.as<T>(), c->ent.as<T>(),
                                                                      m->base[0].as<T>(), ne);
        for (int t = 1; t < merge_ntab(c); ++t) {
            const int64_t e = merge_elems(c, t);
            T* p = merge_table(c, t).as<T>();
            merge_delta_kernel<T><<<merge_grid(e), 256, 0, c->stream>>>(p, p, m->base[t].as<T>(), e);
        }
    });
    HIPCHK(hipGetLastError());
}

// phase 2: reduce-scatter of the entity deltas, all-reduce of the others
void merge_reduce(kb2e_ctx* const* cs, int n) {
    if (!cs[0]->mg->local) {
        NCCLCHK(ncclGroupStart());
        for (int k = 0; k < n; ++k) {
            kb2e_ctx* c = cs[k];
            MergeState* m = c->mg;
            HIPCHK(hipSetDevice(c->cfg.device));
            NCCLCHK(ncclReduceScatter(m->send.p, m->recv.p, (size_t)(m->block * c->ld), merge_type(c), ncclSum,
                                      m->comm, c->stream));
            for (int t = 1; t < merge_ntab(c); ++t) {
                void* p = merge_table(c, t).p;
                NCCLCHK(ncclAllReduce(p, p, (size_t)merge_elems(c, t), merge_type(c), ncclSum, m->comm, c->stream));
            }
        }
        NCCLCHK(ncclGroupEnd());
        return;
    }
    merge_sync_all(cs, n);
    kb2e_ctx* c0 = cs[0];
    HIPCHK(hipSetDevice(c0->cfg.device));
    typed(c0, [&](auto tag) {
        using T = decltype(tag);
        const int64_t bl = c0->mg->block * c0->ld;
        for (int k = 0; k < n; ++k) {  // rank k's block of every rank's entity deltas
            SrcList<T> src{};
            for (int j = 0; j < n; ++j) src.p[j] = cs[j]->mg->send.template as<T>() + (int64_t)k * bl;
            merge_sum_kernel<T><<<merge_grid(bl), 256, 0, c0->stream>>>(cs[k]->mg->recv.template as<T>(), src, n, bl);
        }
        for (int t = 1; t < merge_ntab(c0); ++t) {
            const int64_t e = merge_elems(c0, t);
            DevBuf& tmp = c0->mg->tmp;
            if (tmp.bytes < (size_t)e * sizeof(T)) tmp.alloc((size_t)e * sizeof(T));
            SrcList<T> src{};
            for (int j = 0; j < n; ++j) src.p[j] = merge_table(cs[j], t).template as<T>();
            merge_sum_kernel<T><<<merge_grid(e), 256, 0, c0->stream>>>(tmp.as<T>(), src, n, e);
            for (int j = 0; j < n; ++j)
                HIPCHK(hipMemcpyAsync(merge_table(cs[j], t).p, tmp.p, (size_t)e * sizeof(T), hipMemcpyDefault,
                                      c0->stream));
        }
    });
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c0->stream));
}

// phase 3: apply the summed deltas, renormalise the changed rows
void merge_apply(kb2e_ctx* c) {
    MergeState* m = c->mg;
    const int64_t ld = c->ld, n_own = m->hi - m->lo;
    typed(c, [&](auto tag) {
        using T = decltype(tag);
        if (n_own > 0) {
            T* own = c->ent.as<T>() + m->lo * ld;
            HIPCHK(hipMemsetAsync(m->mask.p, 0, (size_t)n_own, c->stream));
            merge_apply_kernel<T><<<merge_grid(n_own * ld), 256, 0, c->stream>>>(
                own, m->base[0].as<T>() + m->lo * ld, m->recv.as<T>(), n_own * ld, ld, m->mask.as<uint8_t>());
            renorm_rows(c, 0, m->lo, n_own, m->mask.as<uint8_t>());
            HIPCHK(hipMemcpyAsync(m->recv.p, own, (size_t)(n_own * ld) * sizeof(T), hipMemcpyDeviceToDevice, c->stream));
        }
        for (int t = 1; t < merge_ntab(c); ++t) {
            const int64_t e = merge_elems(c, t), units = merge_units(c, t);
            T* p = merge_table(c, t).as<T>();
            HIPCHK(hipMemsetAsync(m->mask.p, 0, (size_t)units, c->stream));
            merge_apply_kernel<T><<<merge_grid(e), 256, 0, c->stream>>>(p, m->base[t].as<T>(), p, e,
                                                                         merge_unit_len(c, t), m->mask.as<uint8_t>());
            renorm_rows(c, t, 0, units, m->mask.as<uint8_t>());
        }
    });
    HIPCHK(hipGetLastError());
}

// phase 4: every rank gets every owner's block
void merge_gather(kb2e_ctx* const* cs, int n) {
    if (!cs[0]->mg->local) {
        NCCLCHK(ncclGroupStart());
        for (int k = 0; k < n; ++k) {
            kb2e_ctx* c = cs[k];
            HIPCHK(hipSetDevice(c->cfg.device));
            NCCLCHK(ncclAllGather(c->mg->recv.p, c->mg->send.p, (size_t)(c->mg->block * c->ld), merge_type(c),
                                  c->mg->comm, c->stream));
        }
        NCCLCHK(ncclGroupEnd());
        return;
    }
    merge_sync_all(cs, n);
    kb2e_ctx* c0 = cs[0];
    HIPCHK(hipSetDevice(c0->cfg.device));
    const size_t bl = (size_t)(c0->mg->block * c0->ld) * c0->esize;
    for (int j = 0; j < n; ++j)
        for (int k = 0; k < n; ++k)
            HIPCHK(hipMemcpyAsync((char*)cs[j]->mg->send.p + k * bl, cs[k]->mg->recv.p, bl, hipMemcpyDefault,
                                  c0->stream));
    HIPCHK(hipStreamSynchronize(c0->stream));
}

// phase 5: the gathered entity table, the next epoch's base
void merge_commit(kb2e_ctx* c) {
    HIPCHK(hipMemcpyAsync(c->ent.p, c->mg->send.p, (size_t)merge_elems(c, 0) * c->esize, hipMemcpyDeviceToDevice,
                          c->stream));
    merge_snapshot(c);
}

void merge_run(kb2e_ctx* const* cs, int n) {
    for (int k = 0; k < n; ++k) {
        if (!cs[k]->mg) throw std::logic_error("kb2e_comm_init first");
        HIPCHK(hipSetDevice(cs[k]->cfg.device));
        merge_deltas(cs[k]);
    }
    merge_reduce(cs, n);
    for (int k = 0; k < n; ++k) {
        HIPCHK(hipSetDevice(cs[k]->cfg.device));
        merge_apply(cs[k]);
    }
    merge_gather(cs, n);
    for (int k = 0; k < n; ++k) {
        HIPCHK(hipSetDevice(cs[k]->cfg.device));
        merge_commit(cs[k]);
    }
    for (int k = 0; k < n; ++k) {
        HIPCHK(hipSetDevice(cs[k]->cfg.device));
        merge_finish(cs[k]);
    }
}

// after the communicators exist: buffers, rank 0's tables everywhere, the base
void merge_start(kb2e_ctx* const* cs, int n) {
    for (int k = 0; k < n; ++k) {
        HIPCHK(hipSetDevice(cs[k]->cfg.device));
        merge_setup(cs[k], cs[k]->mg);
    }
    merge_broadcast(cs, n);
    for (int k = 0; k < n; ++k) {
        HIPCHK(hipSetDevice(cs[k]->cfg.device));
        merge_snapshot(cs[k]);
        merge_finish(cs[k]);
    }
}

// every rank's (model, dim, |E|, |R|, precision) over the new communicator: a rank
// whose tables differ would issue collectives of other sizes or types (a hang or
// corrupted tables) instead of failing
void merge_check_ranks(kb2e_ctx* c, MergeState* m) {
    const kb2e_config& g = c->cfg;
    const int64_t mine[5] = {g.model, g.dim, g.num_entities, g.num_relations, g.precision};
    DevBuf all;
    all.alloc((size_t)m->nranks * sizeof(mine));
    char* slot = (char*)all.p + (size_t)m->rank * sizeof(mine);
    HIPCHK(hipMemcpyAsync(slot, mine, sizeof(mine), hipMemcpyHostToDevice, c->stream));
    NCCLCHK(ncclAllGather(slot, all.p, 5, ncclInt64, m->comm, c->stream));  // (in place)
    std::vector<int64_t> h((size_t)m->nranks * 5);
    HIPCHK(hipMemcpyAsync(h.data(), all.p, all.bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int k = 0; k < m->nranks; ++k)
        if (!std::equal(mine, mine + 5, h.begin() + 5 * k))
            throw std::invalid_argument("rank " + std::to_string(k) +
                                        " differs in model / dim / table sizes / precision");
}

// attach the group's merge states and start them; on any failure the contexts are
// left without one (and the communicators destroyed), so kb2e_comm_init can be retried
void merge_attach(kb2e_ctx* const* cs, int n, std::vector<std::unique_ptr<MergeState>>& ms) {
    for (int k = 0; k < n; ++k) cs[k]->mg = ms[k].get();
    try {
        merge_start(cs, n);
    } catch (...) {
        for (int k = 0; k < n; ++k) cs[k]->mg = nullptr;
        throw;  // (ms destroys the states and their communicators)
    }
    for (auto& m : ms) (void)m.release();
}

// a group-wide call: the status and message go to every context
template <class F>
kb2e_status guarded_group(kb2e_ctx* const* cs, int n, F&& f) {
    if (!cs || n < 1) return KB2E_EINVAL;
    for (int k = 0; k < n; ++k)
        if (!cs[k]) return KB2E_EINVAL;
    kb2e_status s = guarded(cs[0], f);
    for (int k = 1; k < n; ++k)
        if (s != KB2E_OK) cs[k]->err = cs[0]->err;
    return s;
}

}  // namespace

extern "C" {

kb2e_status kb2e_comm_unique_id(uint8_t* id) {
    if (!id) return KB2E_EINVAL;
    static_assert(sizeof(ncclUniqueId) == KB2E_COMM_ID_BYTES, "RCCL unique id size");
    ncclUniqueId u;
    if (ncclGetUniqueId(&u) != ncclSuccess) return KB2E_EDEVICE;
    std::memcpy(id, &u, sizeof(u));
    return KB2E_OK;
}

kb2e_status kb2e_comm_init_rank(kb2e_ctx* c, int32_t nranks, int32_t rank, const uint8_t* id) {
    return guarded(c, [&] {
        if (!id || nranks < 1 || rank < 0 || rank >= nranks) return fail(c, KB2E_EINVAL, "bad rank / id");
        if (c->mg) return fail(c, KB2E_ESTATE, "communicator already initialised");
        merge_check_group(&c, 1);
        HIPCHK(hipSetDevice(c->cfg.device));
        std::vector<std::unique_ptr<MergeState>> ms;
        ms.emplace_back(new MergeState());
        MergeState* m = ms[0].get();
        m->nranks = nranks;
        m->rank = rank;
        ncclUniqueId u;
        std::memcpy(&u, id, sizeof(u));
        NCCLCHK(ncclCommInitRank(&m->comm, nranks, u, rank));
        merge_check_ranks(c, m);
        merge_attach(&c, 1, ms);
        return KB2E_OK;
    });
}

kb2e_status kb2e_comm_init_group(kb2e_ctx* const* cs, int32_t n) {
    return guarded_group(cs, n, [&] {
        merge_check_group(cs, n);
        for (int k = 0; k < n; ++k)
            if (cs[k]->mg) return fail(cs[0], KB2E_ESTATE, "communicator already initialised");
        std::vector<int> devs(n);
        bool shared = false, one_device = true;
        for (int k = 0; k < n; ++k) {
            devs[k] = cs[k]->cfg.device;
            one_device &= devs[k] == devs[0];
            for (int j = 0; j < k; ++j) shared |= devs[j] == devs[k];
        }
        // the local backend reads every rank's buffers from cs[0]'s device: one device
        // only (RCCL refuses two ranks on one device, so a mixed group has no backend)
        const char* lv = getenv("KB2E_MERGE_LOCAL");
        const bool local = shared || (lv && lv[0] == '1');
        if (local && !one_device)
            return fail(cs[0], KB2E_EUNSUPPORTED, "the local merge backend needs every context on one device");
        if (local && n > kLocalMaxRanks) return fail(cs[0], KB2E_EUNSUPPORTED, "local merge group too large");
        std::vector<std::unique_ptr<MergeState>> ms;
        for (int k = 0; k < n; ++k) {
            ms.emplace_back(new MergeState());
            ms[k]->local = local;
            ms[k]->nranks = n;
            ms[k]->rank = k;
        }
        if (!local) {
            std::vector<ncclComm_t> comms(n, nullptr);
            NCCLCHK(ncclCommInitAll(comms.data(), n, devs.data()));
            for (int k = 0; k < n; ++k) ms[k]->comm = comms[k];
        }
        merge_attach(cs, n, ms);
        return KB2E_OK;
    });
}

kb2e_status kb2e_merge_epoch(kb2e_ctx* c) {
    return guarded(c, [&] {
        if (!c->mg) return fail(c, KB2E_ESTATE, "kb2e_comm_init_rank first");
        if (c->mg->local) return fail(c, KB2E_ESTATE, "a local group merges with kb2e_merge_epoch_group");
        merge_run(&c, 1);
        return KB2E_OK;
    });
}

kb2e_status kb2e_merge_epoch_group(kb2e_ctx* const* cs, int32_t n) {
    return guarded_group(cs, n, [&] {
        for (int k = 0; k < n; ++k)
            if (!cs[k]->mg || cs[k]->mg->nranks != n || cs[k]->mg->rank != k)
                return fail(cs[0], KB2E_ESTATE, "kb2e_comm_init_group on this group first");
        merge_run(cs, n);
        return KB2E_OK;
    });
}

kb2e_status kb2e_comm_info(kb2e_ctx* c, int32_t* nranks, int32_t* rank, int64_t* first_entity,
                           int64_t* entity_count) {
    return guarded(c, [&] {
        if (!c->mg) return fail(c, KB2E_ESTATE, "no communicator");
        if (nranks) *nranks = c->mg->nranks;
        if (rank) *rank = c->mg->rank;
        if (first_entity) *first_entity = c->mg->lo;
        if (entity_count) *entity_count = c->mg->hi - c->mg->lo;
        return KB2E_OK;
    });
}

}  // extern "C"
