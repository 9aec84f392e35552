/*
 * kb2e_engine.h -- the drop-in C ABI of the kb2e_amd MI355X training engine.
 *
 * The reference (eriq-augustine/KB2E) runs its per-triple SGD hot path inside
 * the C++ class common::Trainer (common/trainer.h:14-78).  Its protected
 * virtual bfgs() (common/trainer.h:59, common/trainer.cpp:69-107) loops over
 * epochs and batches, draws a corrupted triple per sample, scores both triples
 * with the model's tripleEnergy() and applies gradientUpdate() to the *_next_
 * tables (transe/trainer.cpp:25-56, transh/trainer.cpp:11-75,
 * transr/trainer.cpp:35-188).  This ABI replaces exactly that loop: a host
 * trainer overrides bfgs() and calls the functions below (INTEGRATION.md shows
 * the binding).  Everything else (argument parsing, file loading, writing the
 * embedding text files, evaluation binaries) stays on the host.
 *
 * Conventions: plain C types, caller-owned buffers borrowed only for the call,
 * row-major contiguous tables, status codes instead of exceptions.  One host
 * thread per context; contexts are independent (one per GPU / rank).
 */
#ifndef KB2E_ENGINE_H_
#define KB2E_ENGINE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    KB2E_OK = 0,
    KB2E_EINVAL = 1,      /* bad argument / shape (reference: printf + exit(1)) */
    KB2E_EDEVICE = 2,     /* HIP runtime or kernel failure */
    KB2E_ESTATE = 3,      /* call order violated (e.g. train before upload) */
    KB2E_ENOMEM = 4,
    KB2E_EUNSUPPORTED = 5,
    KB2E_ESAMPLER = 6     /* a negative could not be drawn (every entity is a
                             known triple: the reference loops forever here,
                             common/trainer.cpp:89-96) */
} kb2e_status;

typedef enum { KB2E_TRANSE = 0, KB2E_TRANSH = 1, KB2E_TRANSR = 2 } kb2e_model;

/* Where the sample stream (train index i, corrupting entity j, side) comes from. */
typedef enum {
    KB2E_SAMPLER_GLIBC = 0,  /* the reference's own stream: glibc TYPE_3 rand()
                                seeded by `seed`, consumed exactly as
                                common/trainer.cpp:79-98 (default) */
    KB2E_SAMPLER_REPLAY = 1  /* caller supplies the stream (kb2e_set_sample_stream) */
} kb2e_sampler;

/* How a batch's updates are applied to the *_next_ tables.  Both schedules
 * score every sample and compute every update direction from the
 * start-of-batch tables, as the reference does (common/trainer.cpp:130-149). */
typedef enum {
    KB2E_SCHEDULE_ORDERED = 0,  /* the reference's sequence: sample by sample, a
                                   norm after every update (transe/trainer.cpp:38-45,
                                   transh/trainer.cpp:48-58, transr/trainer.cpp:
                                   166-187); results equal the reference's (default) */
    KB2E_SCHEDULE_PARALLEL = 1  /* each touched row / relation gets its summed
                                   delta, then the model's norms and constraints
                                   once per batch; equal to ORDERED for rows with
                                   one update per batch, O(lr^2) apart otherwise.
                                   Parity is statistical (link-prediction quality,
                                   DESIGN.md) */
} kb2e_schedule;

typedef struct {
    int32_t model;          /* kb2e_model */
    int32_t dim;            /* --size (common/args.cpp:71-74) */
    int32_t num_entities;
    int32_t num_relations;
    double learning_rate;   /* --rate */
    double margin;          /* --margin */
    int32_t method;         /* 0 unif, 1 bern (common/constants.h:7-8) */
    int32_t distance;       /* 0 L1, 1 L2 (common/constants.h:16-17); TransH is always L1 */
    int32_t num_batches;    /* --batches */
    uint32_t seed;          /* --seed: srand() in main (transe/bin/trainTransE.cpp:13) */
    int32_t precision;      /* 64 = FP64 tables and arithmetic like the reference; 32 = FP32 */
    int32_t sampler;        /* kb2e_sampler */
    int32_t transr_compat;  /* 1: reproduce the accumulating TransR energy of
                               transr/transr.cpp:20-25; 0: zeroed work vectors */
    int32_t device;         /* HIP device ordinal */
    int32_t schedule;       /* kb2e_schedule */
    int32_t sub_batches;    /* PARALLEL TransR: each batch's summed updates, norms and
                               transRNorm pairs applied in this many ordered sub-batches
                               of ceil(B / k) samples (the energies, hinge decisions and
                               update directions stay on the start-of-batch tables,
                               common/trainer.cpp:132-133); nearer the reference's
                               norm after every update (transr/trainer.cpp:174-187).
                               1 = one per batch; 0 (kb2e_default_config) = by width:
                               the smallest count whose loss stays inside the
                               reference's seed envelope where measured (2 for
                               dim <= 64, 3 above).  Ignored by the other
                               models and the ORDERED schedule. */
} kb2e_config;

typedef struct kb2e_ctx kb2e_ctx;

/* Fill `cfg` with the reference defaults (common/constants.h:28-40). */
void kb2e_default_config(kb2e_config* cfg);

kb2e_status kb2e_create(const kb2e_config* cfg, kb2e_ctx** out);
/* The context's configuration with the defaults resolved (sub_batches 0 -> the
 * count the context runs). */
kb2e_status kb2e_get_config(const kb2e_ctx* ctx, kb2e_config* out);
void kb2e_destroy(kb2e_ctx* ctx);
const char* kb2e_last_error(const kb2e_ctx* ctx);

/* Trainer::add for every training triple, in train-file order, plus the
 * per-relation head/tail co-occurrence means of Trainer::loadFiles
 * (common/trainer.cpp:26-32, 151-201).  Builds the negative-sample filter and
 * the Bernoulli table on the device.  Contexts take dim <= 512 for every
 * model and schedule, PARALLEL TransR included (above 128 on the wide
 * kernels), checked at kb2e_create (KB2E_EINVAL above); wide TransR keeps a
 * relation's matrix in L2 instead of LDS. */
kb2e_status kb2e_upload_triples(kb2e_ctx* ctx, const int32_t* heads, const int32_t* tails,
                                const int32_t* relations, int64_t count);

/* Trainer::prepTrain (common/trainer.cpp:34-58; transh/trainer.cpp:77-88;
 * transr/trainer.cpp:70-86 up to the seed files): draws the initial tables from
 * the context's glibc stream exactly as the reference does, uploads them, and
 * (if the pointers are non-NULL) returns them.  Weights: TransH R x n, TransR
 * R x n x n ([r][j][i]). */
kb2e_status kb2e_init_params(kb2e_ctx* ctx, double* entity, double* relation, double* weights);

/* TransR's seed step (transr/trainer.cpp:88-113): entity rows from the
 * seed TransE run are scaled to unit length (common::norm(v, false)),
 * relation rows are taken verbatim; the relation matrices keep the identity
 * that kb2e_init_params set.  Call after kb2e_init_params. */
kb2e_status kb2e_transr_seed(kb2e_ctx* ctx, const double* entity, const double* relation);

/* Trainer::prepTrain's draws made on the device: the same
 * randn values (common/utils.cpp:26-38), row norms and TransH / TransR weight
 * init as kb2e_init_params, taken from the same glibc stream and leaving it at
 * the same position -- the epochs that follow are unchanged.  Every rejection
 * attempt is evaluated in parallel (the stream is made on the device from the
 * generator's 31-word window) and the accepted ones are compacted in order.
 * *near_ties (may be NULL) = accept/reject decisions within a few ulps of the
 * density, where the device exp and glibc's could round differently. */
kb2e_status kb2e_init_params_device(kb2e_ctx* ctx, double* entity, double* relation, double* weights,
                                    int64_t* near_ties);

/* Text tables.  table: 0 entities (|E| rows), 1 relations
 * (|R| rows), 2 weights (TransH |R| rows, TransR |R|*n rows).
 * kb2e_write_table writes the device table as Trainer::write does
 * (common/trainer.cpp:109-127, transh/trainer.cpp:94-105,
 * transr/trainer.cpp:128-142): "%.6lf\t" per value, "\n" per row, formatted
 * on the device byte for byte as glibc printf; kb2e_format_table returns the
 * same bytes in `buf` (*len = the length needed; KB2E_EINVAL if cap is short).
 * kb2e_read_table loads a table from "%lf" text as the TransR seed step reads
 * its files (transr/trainer.cpp:88-113): whitespace-separated tokens, the first
 * rows*n used, converted on the device (correctly rounded, as strtod), then
 * optionally normalised per row.  KB2E_EINVAL with the reference's message when
 * the file holds fewer numbers. */
enum { KB2E_READ_VERBATIM = 0, KB2E_READ_UNIT = 1 /* common::norm(row, false) */,
       KB2E_READ_SHRINK = 2 /* common::norm(row): only rows longer than 1 */ };
kb2e_status kb2e_write_table(kb2e_ctx* ctx, int32_t table, const char* path);
kb2e_status kb2e_format_table(kb2e_ctx* ctx, int32_t table, char* buf, int64_t cap, int64_t* len);
kb2e_status kb2e_read_table(kb2e_ctx* ctx, int32_t table, const char* path, int32_t mode);

/* Upload tables (row-major FP64 as in the reference's vectors).  `weights` may
 * be NULL for TransE.  Used for TransR seeding (transr/trainer.cpp:88-113; the
 * caller applies the entity unit norm as the reference does) and for restarts. */
kb2e_status kb2e_upload_params(kb2e_ctx* ctx, const double* entity, const double* relation,
                               const double* weights);
kb2e_status kb2e_download_params(kb2e_ctx* ctx, double* entity, double* relation, double* weights);

/* TransR energy work vectors (transr/trainer.h:28-29), for compat-mode state. */
kb2e_status kb2e_get_transr_work(kb2e_ctx* ctx, double* head_work, double* tail_work);
kb2e_status kb2e_set_transr_work(kb2e_ctx* ctx, const double* head_work, const double* tail_work);

/* KB2E_SAMPLER_REPLAY: the next `count` samples (i = train index, j = entity,
 * side = 1 corrupt tail / 0 corrupt head).  Consumed batch by batch. */
kb2e_status kb2e_set_sample_stream(kb2e_ctx* ctx, const int32_t* i, const int32_t* j,
                                   const uint8_t* side, int64_t count);

/* The sample stream of the epoch in progress (after its first batch was
 * queued) or, between epochs, of the last one: up to `count` samples in order.
 * Returns KB2E_ESTATE before the first epoch on the uploaded triple set. */
kb2e_status kb2e_get_sample_stream(kb2e_ctx* ctx, int32_t* i, int32_t* j, uint8_t* side, int64_t count);

/* One epoch of Trainer::bfgs (common/trainer.cpp:72-106): numBatches batches of
 * floor(|train| / numBatches) samples.  *loss = the epoch loss the reference
 * prints at :105; *active = hinge-active samples.  Either pointer may be NULL. */
kb2e_status kb2e_train_epoch(kb2e_ctx* ctx, double* loss, int64_t* active);

/* `nbatches` batches continuing the current epoch position (wrapping into the
 * next epoch).  Asynchronous: returns once queued; results land at the next
 * kb2e_synchronize / kb2e_epoch_stats. */
kb2e_status kb2e_train_batches(kb2e_ctx* ctx, int32_t nbatches);
kb2e_status kb2e_synchronize(kb2e_ctx* ctx);
/* Loss and active count accumulated since the last call (resets them). */
kb2e_status kb2e_take_stats(kb2e_ctx* ctx, double* loss, int64_t* active);

/* Link prediction on the current device tables (EmbeddingEvaluation::run,
 * common/evaluation.cpp:181-251): for each test triple, corrupt the head and
 * the tail with every entity, rank the true triple by energy; filtered ranks
 * skip corruptions that are in the filter set (the reference passes test +
 * train + valid, common/evaluation.cpp:41-62).  out[0..3] = raw mean rank,
 * raw hits@10, filtered mean rank, filtered hits@10 (hits as fractions, as
 * printed at :249-250).  Energies are bit-identical FP64 restatements of the
 * reference's; ties with the true triple are not counted above it.  TransR
 * uses the zeroed (fixed) work vectors here; kb2e_evaluate_transr_compat is
 * the reference evalTransR's stateful energy.  Every dim a context takes
 * (kb2e_create: <= 512); the ranking itself has no limit (the query rows of a
 * rank tile are staged in LDS up to dim 600, read from L2 above).
 * KB2E_EINVAL (here and in kb2e_evaluate_transr_compat): ntest < 1,
 * nfilter < 0, an id out of range in the test set or the filter. */
kb2e_status kb2e_evaluate(kb2e_ctx* ctx, const int32_t* heads, const int32_t* tails, const int32_t* relations,
                          int64_t ntest, const int32_t* filter_heads, const int32_t* filter_tails,
                          const int32_t* filter_relations, int64_t nfilter, double* out);

/* TransR as the reference's evalTransR computes it: the energy work vectors
 * are never zeroed (transr/transr.cpp:20-25, transr/evaluation.cpp:22-32), so
 * every energy depends on all energies computed before it in the evaluator's
 * cached relation-major loop (common/evaluation.cpp:107-121, 181-238; the
 * per-relation energy cache is used when |E| <= 40000, common/evaluation.h:11).
 * That sequence is replayed exactly in FP64 on the device.  `work` = 2 x dim
 * doubles (head then tail work vector): in, the state to start from (NULL =
 * zeros, as a fresh evalTransR process); out, the state after the run.
 * out[0..3] as kb2e_evaluate; out[4] = candidates whose energy equals the true
 * triple's (std::sort orders those arbitrarily, :138; they are ranked after
 * the truth here).  `progress` (may be NULL) is called after each relation
 * with the fraction of test triples done (the reference prints it, :240).
 * Every dim a context takes (W in LDS up to 140, read from L2 above). */
kb2e_status kb2e_evaluate_transr_compat(kb2e_ctx* ctx, const int32_t* heads, const int32_t* tails,
                                        const int32_t* relations, int64_t ntest, const int32_t* filter_heads,
                                        const int32_t* filter_tails, const int32_t* filter_relations,
                                        int64_t nfilter, double* work, double* out,
                                        void (*progress)(double fraction, void* user), void* user);

/* ---- Using a trained model.  The five calls below read the current device
 * tables and change nothing: not the tables, the training state, the RNG or
 * the TransR work vectors.  They use kb2e_evaluate's stateless energies for
 * every model, distance, precision and dim a context takes: FP64 arithmetic
 * with each sum in the reference's serial order (TransH is L1; TransR from
 * zeroed work vectors; FP32 tables are widened to FP64 first).  transr_compat
 * is ignored: the accumulating energy depends on every call made before and
 * has no meaning for a stand-alone query.  Every device buffer they allocate
 * is freed before they return (kb2e_device_bytes is the same before and
 * after), and they return after a stream synchronisation. */

/* energy[i] = tripleEnergy(heads[i], tails[i], relations[i]), bit-identical to
 * transe/transe.cpp, transh/transh.cpp:10-29 and transr/transr.cpp:13-37 (with
 * zeroed vectors).  count >= 1; an id out of range is KB2E_EINVAL. */
kb2e_status kb2e_score_triples(kb2e_ctx* ctx, const int32_t* heads, const int32_t* tails,
                               const int32_t* relations, int64_t count, double* energy);

/* Top-k link prediction.  Query q is (entities[q], relations[q], side[q]); side
 * follows the sample stream's convention: 1 = the tail is unknown, candidates
 * (e, x, r) for every entity x; 0 = the head is unknown, candidates (x, e, r).
 * A candidate whose triple is among the nfilter filter triples is excluded
 * (nfilter == 0 with NULL arrays: nothing is).  Nothing else is excluded:
 * x == e is a candidate, as in the reference's corruption loop -- and the true
 * answer of a test triple is excluded too if the caller lists that triple in
 * the filter (pass train + valid to rank the truth, train + valid + test to
 * see only new answers).
 * Per query: the k remaining candidates of smallest energy in ascending
 * (energy, entity id) order in ids[q*k + j], energy[q*k + j];
 * found[q] = min(k, |E| - excluded); slots at and after found[q] hold -1 and
 * +inf.  1 <= k <= 1024 (k may exceed |E|).  KB2E_EINVAL: k out of range, a
 * side other than 0 / 1, nq < 1, an id out of range in a query or the filter.
 * The candidate keys of at most 1 GiB worth of queries are held at a time, so
 * nq is not bounded by device memory. */
kb2e_status kb2e_predict(kb2e_ctx* ctx, const int32_t* entities, const int32_t* relations, const int32_t* side,
                         int64_t nq, int32_t k, const int32_t* filter_heads, const int32_t* filter_tails,
                         const int32_t* filter_relations, int64_t nfilter, int32_t* ids, double* energy,
                         int32_t* found);

/* kb2e_evaluate's ranks per test triple, in the caller's order:
 * ranks[i*4 + 0..3] = head raw, head filtered, tail raw, tail filtered rank of
 * test triple i (1 + the candidates ranked above the truth; ties are not).
 * kb2e_evaluate's four numbers are their means and <= 10 fractions. */
kb2e_status kb2e_rank_triples(kb2e_ctx* ctx, const int32_t* heads, const int32_t* tails, const int32_t* relations,
                              int64_t ntest, const int32_t* filter_heads, const int32_t* filter_tails,
                              const int32_t* filter_relations, int64_t nfilter, int64_t* ranks);

/* Relation prediction: which relation holds between heads[q] and tails[q]?
 * The candidates of query q are the triples (heads[q], tails[q], r) of every
 * relation r, each with the energy kb2e_score_triples gives it, bit for bit.
 * A candidate whose triple is among the nfilter filter triples is excluded and
 * nothing else is (heads[q] == tails[q] is a legal query).  Output as
 * kb2e_predict: the k remaining relations of smallest energy in ascending
 * (energy, relation id) order in ids[q*k + j], energy[q*k + j];
 * found[q] = min(k, |R| - excluded), which is 0 when every relation of the pair
 * is in the filter; slots at and after found[q] hold -1 and +inf.
 * 1 <= k <= 1024 (k may exceed |R|).  KB2E_EINVAL: k out of range, nq < 1, an
 * id out of range in a query or the filter, NULL arrays with a count > 0.
 * TransE and TransH score a pair against every relation directly; TransR
 * projects the distinct entities of the queries once per relation (in relation
 * batches whose projections stay under 512 MiB; KB2E_RELPRED_REL_BATCH=<n>
 * lowers the batch) instead of twice per (pair, relation).  The key buffer is
 * chunked as kb2e_predict's. */
kb2e_status kb2e_predict_relations(kb2e_ctx* ctx, const int32_t* heads, const int32_t* tails, int64_t nq, int32_t k,
                                   const int32_t* filter_heads, const int32_t* filter_tails,
                                   const int32_t* filter_relations, int64_t nfilter, int32_t* ids, double* energy,
                                   int32_t* found);

/* The rank of the true relation of each test triple, in the caller's order:
 * ranks[i*2 + 0] = raw rank of relations[i] among the |R| candidates of
 * (heads[i], tails[i]): 1 + the candidates of strictly smaller energy (ties are
 * not counted above the truth, as in kb2e_rank_triples); ranks[i*2 + 1] = the
 * same with the candidates r' != relations[i] whose triple is in the filter
 * left out.  Mean rank and Hits@1 of these are the relation-prediction numbers
 * of the PTransE line of work. */
kb2e_status kb2e_rank_relations(kb2e_ctx* ctx, const int32_t* heads, const int32_t* tails, const int32_t* relations,
                                int64_t ntest, const int32_t* filter_heads, const int32_t* filter_tails,
                                const int32_t* filter_relations, int64_t nfilter, int64_t* ranks /* [ntest][2] */);

/* Conjunctive queries: which entity fits several triple patterns at once
 * ("born in X and works for Y and won Z"; or: which known entity is this
 * record, given the triples that mention it -- the counterpart of
 * kb2e_fold_in_entities, which embeds an entity the model does not have).  Both
 * calls follow the contract of "Using a trained model" above.
 *   Constraints.  Query q owns the constraints c = offsets[q] ..
 *   offsets[q+1]-1, each (entities[c], relations[c], side[c]) in kb2e_predict's
 *   convention: side 1, the unknown x is the tail of (entities[c], x,
 *   relations[c]); side 0, the head of (x, entities[c], relations[c]).
 *   offsets[0] == 0, offsets is strictly increasing and
 *   1 <= m_q = offsets[q+1] - offsets[q] <= KB2E_JOINT_MAX_CONSTRAINTS.  A
 *   constraint may appear twice in a query; each listing counts.
 *   Candidates.  Every entity x is a candidate of every query, x == entities[c]
 *   included, as in kb2e_predict.  The energy of x for constraint c is what
 *   kb2e_score_triples returns for that triple, bit for bit.
 *   Joint energy.  s = e_first; s += e_next; ... over the query's constraints
 *   in the caller's order, in FP64, one rounding per addition.  The order of a
 *   query's constraints is therefore part of the result: a permutation of them
 *   may move the last bit of a joint energy.
 *   Exclusion.  The filter triples form a set (duplicates count once;
 *   nfilter == 0 with NULL arrays is legal).  A candidate is excluded iff every
 *   one of its m_q triples is in the filter: it is then a known answer to the
 *   whole conjunction.  A candidate that satisfies only some of the patterns
 *   stays in.  With m_q == 1 this is kb2e_predict's rule.
 *   kb2e_predict_joint.  Layout and ordering as kb2e_predict: per query the
 *   found[q] = min(k, |E| - excluded) remaining candidates of smallest joint
 *   energy in ascending (energy, entity id) order in ids[q*k + j],
 *   energy[q*k + j]; the remaining slots hold -1 and +inf.  1 <= k <= 1024.
 *   With m_q == 1 for every query the three outputs equal kb2e_predict's, bit
 *   for bit.
 *   kb2e_rank_joint.  ranks[q*2 + 0] = 1 + the candidates whose joint energy is
 *   strictly smaller than truth[q]'s (ties are not counted above the truth);
 *   ranks[q*2 + 1] = the same count with the excluded candidates other than
 *   truth[q] left out.  With m_q == 1 these are the matching two columns of
 *   kb2e_rank_triples.
 * The queries are walked in the caller's order in chunks: a chunk is the
 * longest run of consecutive queries whose constraint rows fit
 * max(largest m_q of the call, the rows of |E| keys that fit 1 GiB)
 * (KB2E_JOINT_CHUNK_ROWS=<n> lowers the 1 GiB term, for tests); a query is never
 * split, and the chunk's joint keys -- one row per query -- are held beside its
 * constraint rows.  Per chunk every distinct relation is projected once.
 * KB2E_EINVAL: nq < 1, k out of range, a malformed offsets (not starting at 0,
 * not increasing, a query with 0 or more than 64 constraints,
 * offsets[nq] > 2^31 - 1), a side other than 0 / 1, an id out of range in a
 * constraint, in truth or in the filter, a NULL array with a count > 0.
 * KB2E_ESTATE: no embeddings on the device. */
enum { KB2E_JOINT_MAX_CONSTRAINTS = 64 };
kb2e_status kb2e_predict_joint(kb2e_ctx* ctx, const int64_t* offsets /* [nq + 1] */, const int32_t* entities,
                               const int32_t* relations, const int32_t* side /* [offsets[nq]] */, int64_t nq, int32_t k,
                               const int32_t* filter_heads, const int32_t* filter_tails,
                               const int32_t* filter_relations, int64_t nfilter, int32_t* ids /* [nq][k] */,
                               double* energy /* [nq][k] */, int32_t* found /* [nq] */);
kb2e_status kb2e_rank_joint(kb2e_ctx* ctx, const int64_t* offsets, const int32_t* entities, const int32_t* relations,
                            const int32_t* side, const int32_t* truth /* [nq] */, int64_t nq,
                            const int32_t* filter_heads, const int32_t* filter_tails, const int32_t* filter_relations,
                            int64_t nfilter, int64_t* ranks /* [nq][2] */);

/* Path queries: the entities at the end of a relation path ("where was the
 * spouse of X born?" is X --spouse--> ? --born_in--> ?; the intermediate entity
 * is unknown too).  For translation models a path of relations is a sum of
 * translations; the two calls find the cheapest instantiation of the whole path
 * on the card.  Both follow the contract of "Using a trained model" above.
 *   Path.  Query q starts at x_0 = anchors[q] and owns the hops c = offsets[q]
 *   .. offsets[q+1]-1; offsets[0] == 0, offsets is strictly increasing and
 *   1 <= L_q = offsets[q+1] - offsets[q] <= KB2E_PATH_MAX_HOPS.  Hop i
 *   (1 .. L_q) is (relations[c], side[c]), c = offsets[q] + i - 1, in
 *   kb2e_predict's convention: side 1, the step's triple is (x_{i-1}, x_i, r);
 *   side 0, it is (x_i, x_{i-1}, r) -- the relation walked backwards.  Every
 *   entity is a candidate for every x_i, the entity the hop leaves and the
 *   anchor included; with no_loops == 1 a step with x_i == x_{i-1} is no step.
 *   Hop energy.  What kb2e_score_triples returns for the step's triple, bit for
 *   bit.
 *   Path energy.  s = e_1; s += e_2; ... in hop order, FP64, one rounding per
 *   addition.  The energy of an answer y is the minimum of s over the admissible
 *   paths that end in y.  Rounding is monotone, so this is the recurrence
 *   c_1[x] = e_1(x_0, x), c_i[y] = min over p of (c_{i-1}[p] + e_i(p, y)), which
 *   is what the device computes.
 *   Frontier.  After hop i < L_q only the frontier F_i is walked on.  beam == 0:
 *   F_i is every entity that has a path, and the result is the exact minimum
 *   over all |E|^(L_q - 1) intermediate tuples.  1 <= beam <= 1024: F_i is the
 *   min(beam, entities with a path) entities of smallest (c_i, entity id) --
 *   beam search; a beam of |E| or more gives the exact result.  The filter never
 *   touches an intermediate hop: known facts are what a path should walk on.
 *   Predecessor.  The predecessor of y at hop i is the p in F_{i-1} that gives
 *   the minimum, the smallest entity id among equal sums.
 *   Exclusion.  The filter triples form a set (duplicates count once;
 *   nfilter == 0 with NULL arrays is legal).  Per query they are walked along
 *   the path: S_0 = {anchor}; S_i = the entities one filter triple of hop i's
 *   relation and side away from a member of S_{i-1} (with no_loops == 1 no
 *   triple with h == t is taken).  y is excluded iff it is in S_{L_q}: an answer
 *   the graph already states.  With L_q == 1 this is kb2e_predict's rule.
 *   kb2e_predict_path.  Layout and ordering as kb2e_predict: per query the
 *   found[q] = min(k, candidates with a path - excluded) candidates of smallest
 *   path energy in ascending (energy, entity id) order in ids[q*k + j],
 *   energy[q*k + j]; the remaining slots hold -1 and +inf.  1 <= k <= 1024.
 *   via (may be NULL): via[(q*k + j)*(KB2E_PATH_MAX_HOPS-1) + i] = x_{i+1} of
 *   the winning path of answer j for i < L_q - 1, every other slot -1.  With
 *   L_q == 1 for every query ids, energy and found equal kb2e_predict's, bit for
 *   bit.
 *   kb2e_rank_path.  ranks[q*2 + 0] = 1 + the candidates whose path energy is
 *   strictly smaller than truth[q]'s (ties are not counted above the truth; a
 *   candidate without a path is larger than every energy); ranks[q*2 + 1] = the
 *   same count with the excluded candidates other than truth[q] left out.  With
 *   L_q == 1 these are the matching two columns of kb2e_rank_triples.
 * Only the k answers, and for via the frontiers' ids and back-pointers (beam
 * entries per level), leave the card; no key or predecessor row does.  The
 * queries are walked in the caller's order in chunks: a chunk is the longest run
 * of consecutive queries whose |E|-long device rows fit 1 GiB, counted in rows
 * of |E| 4-byte words -- a query of one hop holds 2 (its key row); a longer one
 * 3 under beam search (key row + predecessor row) and 4 + (L_q - 1) with
 * beam == 0 (two key rows, a back-pointer row per hop 2..L_q) --
 * (KB2E_PATH_CHUNK_ROWS=<n> lowers the budget to n such rows, for tests; it is
 * never less than the largest query), and whose short per-query buffers
 * (frontiers, back-pointers, answers) fit 256 MiB; a query is never split.  Per chunk and
 * hop level every distinct relation is projected once.
 * KB2E_EINVAL: nq < 1, k out of range, beam outside 0..1024, no_loops other than
 * 0 / 1, a malformed offsets (not starting at 0, not increasing, a query with 0
 * or more than 8 hops, offsets[nq] > 2^31 - 1), a side other than 0 / 1, an id
 * out of range in an anchor, a hop, truth or the filter, a NULL array with a
 * count > 0.  KB2E_ESTATE: no embeddings on the device. */
enum { KB2E_PATH_MAX_HOPS = 8 };
kb2e_status kb2e_predict_path(kb2e_ctx* ctx, const int32_t* anchors /* [nq] */, const int64_t* offsets /* [nq + 1] */,
                              const int32_t* relations, const int32_t* side /* [offsets[nq]] */, int64_t nq, int32_t k,
                              int32_t beam, int32_t no_loops, const int32_t* filter_heads,
                              const int32_t* filter_tails, const int32_t* filter_relations, int64_t nfilter,
                              int32_t* ids /* [nq][k] */, double* energy /* [nq][k] */, int32_t* found /* [nq] */,
                              int32_t* via /* [nq][k][KB2E_PATH_MAX_HOPS - 1] or NULL */);
kb2e_status kb2e_rank_path(kb2e_ctx* ctx, const int32_t* anchors, const int64_t* offsets, const int32_t* relations,
                           const int32_t* side, const int32_t* truth /* [nq] */, int64_t nq, int32_t beam,
                           int32_t no_loops, const int32_t* filter_heads, const int32_t* filter_tails,
                           const int32_t* filter_relations, int64_t nfilter, int64_t* ranks /* [nq][2] */);

/* ---- Triple classification (Socher et al. 2013; TransH 4.3, TransR 4.3): a
 * triple holds iff its energy is at most the threshold of its relation, fitted
 * on labelled validation triples.  The three calls below follow the contract of
 * the block above (read-only, stateless FP64 energies, transr_compat ignored,
 * every device buffer freed before return, a stream synchronisation at the
 * end).  Labels are uint8_t: 1 = the triple holds, 0 = it does not. */

/* Fit one threshold per relation.  A triple is classified positive iff
 * energy <= delta.  The candidates for delta_r are -inf and every energy
 * (kb2e_score_triples' bits) of relation r's labelled triples; delta_r maximises
 *     correct(delta) = #{positives with e <= delta} + #{negatives with e > delta}
 * and among the maxima the smallest delta wins.  thresholds[r] = delta_r,
 * counts[r*3 + 0..2] = positives, negatives, correct(delta_r) of relation r.
 * The global threshold is the same fit over all `count` triples with the
 * relation ignored (*global_threshold, *global_correct; either may be NULL);
 * a relation without a labelled triple gets thresholds[r] = the global
 * threshold and counts {0, 0, 0}.  The energies are sorted on the device
 * (stable LSD radix on (relation, energy bits)) and swept there; nothing about
 * the result depends on the launch geometry.  KB2E_EINVAL: count < 1 or
 * count > 2^31 - 1, a label other than 0 / 1, an id out of range, a NULL
 * array. */
kb2e_status kb2e_fit_thresholds(kb2e_ctx* ctx, const int32_t* heads, const int32_t* tails, const int32_t* relations,
                                const uint8_t* labels, int64_t count, double* thresholds /* [R] */,
                                int64_t* counts /* [R][3] */, double* global_threshold, int64_t* global_correct);

/* labels_out[i] = energy_i <= thresholds[relations[i]] (thresholds has
 * num_relations entries; -inf and +inf are legal); energy (may be NULL)
 * receives the energies, bit-identical to kb2e_score_triples.  KB2E_EINVAL:
 * count < 1, an id out of range, a NULL array. */
kb2e_status kb2e_classify_triples(kb2e_ctx* ctx, const int32_t* heads, const int32_t* tails,
                                  const int32_t* relations, int64_t count, const double* thresholds /* [R] */,
                                  uint8_t* labels_out, double* energy);

/* One negative per positive triple, for data sets that ship none: the head
 * (slot 0) or the tail (slot 1) of triple i is replaced; the relation stays.
 * side: 0 replaces the head, 1 the tail, 2 flips a fair coin per triple.
 * The `known` triples (pass train + valid + test; nknown == 0 with NULL arrays
 * is legal) give (a) the set of triples that are no negatives and (b) per
 * (relation, slot) the pool: the distinct entities seen in that slot of that
 * relation, ascending.  A draw x is rejected if it equals the entity it
 * replaces or if the new triple is known; x equal to the other slot of the
 * triple stays legal, as in the reference's corruption loop.
 *   stage 1 (constrained = 1 and a non-empty pool; the protocol of Socher et
 *            al. that TransH and TransR use for FB15k): 32 draws from the pool;
 *   stage 2 (constrained = 0, an empty pool, or stage 1 exhausted): 32 draws
 *            from all entities.
 * The first accepted draw is the negative: neg_heads[i], neg_tails[i] are the
 * new triple's head and tail.  If every draw is rejected both are -1 and the
 * triple counts in *failed (may be NULL).
 * The random stream is counter-based and stateless (the context's glibc stream
 * is not touched), all arithmetic modulo 2^64:
 *     mix(z):  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27;
 *              z *= 0x94D049BB133111EB; z ^= z >> 31          (SplitMix64)
 *     state   = mix(seed)
 *     u(i, a) = mix(state + (i << 7) + a)        i = index of the triple
 *     slot    = side, or for side 2 the top bit of u(i, 0)
 *     stage 1, draw a = 1..32:   x = pool[u(i, a) % |pool|]
 *     stage 2, draw a = 33..64:  x = u(i, a) % num_entities
 * KB2E_EINVAL: count < 1 or count > 2^31 - 1, a side other than 0 / 1 / 2, an
 * id out of range in the triples or in `known`, a NULL array. */
kb2e_status kb2e_corrupt_triples(kb2e_ctx* ctx, const int32_t* heads, const int32_t* tails,
                                 const int32_t* relations, int64_t count, const int32_t* known_heads,
                                 const int32_t* known_tails, const int32_t* known_relations, int64_t nknown,
                                 uint64_t seed, int32_t side, int32_t constrained, int32_t* neg_heads,
                                 int32_t* neg_tails, int64_t* failed);

/* ---- Knowledge-base completion: which facts are missing from the graph?
 * Query q is the relation relations[q]; its candidates are the triples
 * (h, t, relations[q]) of every pair of candidate entities, and the answer is
 * the k most plausible of them that are not known yet (upstream KB2E's
 * e1_e2.txt, "the top-500 entity pairs which are calculated by TransE", is
 * such a list).  The call follows the contract of "Using a trained model"
 * above: read-only (tables, training state, glibc stream and TransR work
 * vectors stay), stateless FP64 energies with transr_compat ignored, FP32
 * tables widened first, every model, distance, precision and dim, every device
 * buffer freed before return (also on the error paths), a stream
 * synchronisation at the end.
 *   Candidates.  constrained = 0: every h and every t in 0..|E|-1.
 *   constrained = 1: h from the head pool of the relation and t from its tail
 *   pool, the distinct entities seen in that slot of that relation among the
 *   `known` triples (kb2e_corrupt_triples' pools); a relation with an empty
 *   pool has no candidates.
 *   Exclusions.  A candidate listed among the `known` triples, and with
 *   exclude_loops = 1 every candidate with h == t.  Nothing else; nknown == 0
 *   with NULL arrays is legal.
 *   Energy.  What kb2e_score_triples gives the same triple, bit for bit: the
 *   evaluator's (P_r(t) - P_r(h)) - r_k, one serial FP64 sum over k from zero.
 *   Output.  Per query the found[q] = min(k, candidates - excluded) remaining
 *   candidates of smallest energy in ascending (energy, head id, tail id) order
 *   in heads[q*k + j], tails[q*k + j], energy[q*k + j]; slots at and after
 *   found[q] hold -1, -1 and +inf.  1 <= k <= 1024 (k may exceed the candidate
 *   count).  A relation may be listed more than once; each listing is answered.
 * The |E|^2 keys of a relation are never held.  Besides the projection table
 * [dim][|E|] and the set of known triples, the call's device memory is a record
 * buffer of fixed capacity, 256 MiB whatever |E| is
 * (KB2E_COMPLETE_BUFFER_BYTES=<bytes> lowers it, for tests): the heads are
 * walked in strips whose candidates fit the buffer -- the first strip is 16
 * heads, KB2E_COMPLETE_STRIP_HEADS=<n> caps the later ones (tests) -- and a
 * candidate becomes a record only if its energy is at most the k-th best so far
 * and it is neither an excluded loop nor known; after each strip the k best
 * are selected on the device on (energy, head id, tail id).  The result does
 * not depend on the launch geometry, the strip size, the buffer size or the
 * order in which the records were appended.
 * KB2E_EINVAL: nrel < 1, k out of range, a flag other than 0 / 1, an id out of
 * range in `relations` or in `known`, a NULL array with a count > 0. */
kb2e_status kb2e_complete_triples(kb2e_ctx* ctx, const int32_t* relations, int64_t nrel, int32_t k,
                                  const int32_t* known_heads, const int32_t* known_tails,
                                  const int32_t* known_relations, int64_t nknown, int32_t constrained,
                                  int32_t exclude_loops, int32_t* heads /* [nrel][k] */, int32_t* tails /* [nrel][k] */,
                                  double* energy /* [nrel][k] */, int64_t* found /* [nrel] */);

/* ---- Entity neighbours: which entities lie close to a given one?  Over all
 * entities as queries this is the k-nearest-neighbour graph of the model, and
 * two entities that list each other are the candidates for being the same
 * thing -- the counterpart of the conjunctive queries above, which match a
 * record to a known entity.  The call follows the contract of "Using a trained
 * model" above: read-only (tables, training state, glibc stream and TransR work
 * vectors stay), stateless FP64 arithmetic with transr_compat ignored, FP32
 * tables widened first, every model, distance, precision and dim, every device
 * buffer freed before return (also on the error paths), one stream
 * synchronisation, at the end.
 *   Space.  relation == -1: the entity space, P(x) is row x of the entity
 *   table.  relation == r >= 0: relation r's space, P(x) is the evaluator's
 *   projection for r -- TransE the row itself, TransH x - (w_r . x) w_r, TransR
 *   M_r x from zeroed work vectors -- which answers "similar as an argument
 *   of r".
 *   Distance.  d(a, x) = sum_k |P(x)_k - P(a)_k| (L1) or sum_k (P(x)_k -
 *   P(a)_k)^2 (L2), the norm of the context's energies (a TransH context is
 *   L1), one serial FP64 sum over k from zero in the evaluator's operand order:
 *   bit for bit the energy kb2e_score_triples gives (a, x, r) when relation
 *   r's vector is zero, and in the entity space that of a TransE model on the
 *   same entity table with a zero relation.  d(a, x) and d(x, a) have the same
 *   bits.
 *   Output.  Per query the found[q] = min(k, candidates) nearest entities in
 *   ascending (distance, entity id) order in ids[q*k + j], dist[q*k + j]; slots
 *   at and after found[q] hold -1 and +inf.  The candidates are all |E|
 *   entities, minus entities[q] itself when include_self == 0.  An entity may
 *   be queried more than once; each listing is answered.
 *   Limits.  1 <= k <= 128 (k may exceed |E|).  The bound is a choice of the
 *   fused kernel's LDS budget -- 16 query rows, each with a k-list and a
 *   staging list of 12-byte records, 48 KiB at k = 128 -- not of the method.
 * Nothing of size nq x |E| is ever allocated.  Besides the projected table
 * [dim][|E|] and the outputs, the call's device memory is the partial records
 * (rows of a chunk x candidate slices x k, 12 bytes each), and nq is walked in
 * chunks so that they stay under 64 MiB whatever nq and |E| are
 * (KB2E_NEIGHBORS_CHUNK_ROWS=<rows> lowers the chunk, for tests).  The
 * candidates are cut into slices so that tiles x slices fills the card
 * (KB2E_NEIGHBORS_SLICE=<candidates> forces the slice length, tests; it is
 * raised where one tile's partial records would not fit the cap).  Selection
 * is on the total order (distance bits, entity id) of distinct values: the
 * result does not depend on the launch geometry, the slice length, the
 * chunking or the order in which candidates were appended.
 * KB2E_EINVAL: nq < 1, k out of range, include_self other than 0 / 1, relation
 * outside -1..|R|-1, an entity id out of range, a NULL array with a
 * count > 0. */
kb2e_status kb2e_neighbors(kb2e_ctx* ctx, const int32_t* entities, int64_t nq, int32_t relation, int32_t k,
                           int32_t include_self, int32_t* ids /* [nq][k] */, double* dist /* [nq][k] */,
                           int32_t* found /* [nq] */);

/* Candidate lists: score or rank a triple pattern against a list of entities
 * the caller supplies (fixed negatives of a sampled evaluation, the entities
 * seen in a slot of a relation, the output of a retriever or of another query)
 * instead of all |E|.  The contract of the calls above: read-only, stateless
 * FP64 energies (transr_compat ignored), FP32 tables widened first, every
 * model, distance, precision and dim, every device buffer freed before return
 * (also on the error paths), one stream synchronisation, at the end.
 *   Lists.  List l is candidates[offsets[l] .. offsets[l+1]-1]; offsets[0] == 0,
 *   offsets does not decrease, an empty list is legal, offsets[nlists] <=
 *   2^31 - 1.  Query q uses list lists[q]; lists == NULL means list q and needs
 *   nlists == nq.  Many queries may name one list (one pool per relation and
 *   slot): it is uploaded once and expanded nowhere, host or device.
 *   Query.  (entities[q], relations[q], side[q]) as kb2e_predict's: with
 *   side 1 a listing x stands for the triple (e, x, r), with side 0 for
 *   (x, e, r).  x == e is a legal listing.
 *   Energy.  What kb2e_score_triples returns for that triple, bit for bit.
 *   kb2e_score_candidates.  energy holds the queries' energies back to back in
 *   query order: query q starts at the sum of the list lengths of the queries
 *   before it, and its listings keep the list's order; a duplicate listing gets
 *   its own, equal, entry.
 *   kb2e_rank_candidates.  ranks[q*2+0] = 1 + the listings x != truth[q] whose
 *   energy is strictly below that of the truth's triple (ties are not counted
 *   above the truth; every listing counts, duplicates too); ranks[q*2+1] = the
 *   same without the listings whose triple is in the filter set (a set:
 *   duplicates count once; nfilter == 0 with NULL arrays is legal).
 *   counted[q*2+0..1] = the listings that took part in each comparison --
 *   x != truth, and for the second also not in the filter -- which a caller
 *   needs to normalise a rank.  A listing equal to truth[q] is ignored and the
 *   truth need not be in its list; an empty list gives rank 1, counted 0.  With
 *   a list that names every entity once the two columns are the matching two
 *   columns of kb2e_rank_triples.  The ranking is fused: no energy leaves the
 *   card, and the filter is probed only for listings that count (all listings
 *   x != truth when counted is asked for, else those below the truth).
 * TransR never projects per listing: per chunk and relation the distinct
 * entities (anchors, truths, listings) are projected once into a compact
 * table, or the whole entity table where they are at least half of |E|
 * (KB2E_CANDIDATES_PROJECT=compact|full forces either; the result does not
 * depend on it).  Nothing of size nq x |E| and no expanded triple array is
 * allocated.  Besides the candidate array, the filter set and the per-query
 * counters of the ranks, the call's device memory does not depend on nq: the
 * queries are walked in chunks of at most 2^21 listings and 2^20 queries (a
 * query is never split; one longer list is a chunk of its own), and a chunk
 * holds 8 bytes of energy per listing, a 32-byte work item per 64 listings or
 * shorter list, and for TransR 4 bytes per distinct entity, an |E| x 4-byte
 * remap and one projected table of dim x min(distinct, |E|) x 8 bytes.  The
 * cap: 16 MiB of energies, 64 MiB of work items (lists of one listing; 1 MiB
 * for lists of 64 and more), 16 MiB of distinct entities, the remap and that
 * one table (KB2E_CANDIDATES_CHUNK=<listings> lowers the chunk, for tests).  The results
 * do not depend on the launch geometry, the chunking, the projection path or
 * on whether a list is shared or private.
 * KB2E_EINVAL: nq < 1, nlists < 1, a malformed offsets, lists[q] outside
 * 0..nlists-1, lists == NULL with nlists != nq, a side other than 0 / 1, an id
 * out of range in a query, in truth, in candidates or in the filter, a NULL
 * array with a count > 0.  KB2E_ESTATE: no embeddings on the device. */
kb2e_status kb2e_score_candidates(kb2e_ctx* ctx, const int32_t* entities, const int32_t* relations, const int32_t* side,
                                  const int32_t* lists /* [nq] or NULL */, int64_t nq,
                                  const int64_t* offsets /* [nlists + 1] */, const int32_t* candidates, int64_t nlists,
                                  double* energy /* query-major */);
kb2e_status kb2e_rank_candidates(kb2e_ctx* ctx, const int32_t* entities, const int32_t* relations, const int32_t* side,
                                 const int32_t* truth /* [nq] */, const int32_t* lists /* [nq] or NULL */, int64_t nq,
                                 const int64_t* offsets /* [nlists + 1] */, const int32_t* candidates, int64_t nlists,
                                 const int32_t* filter_heads, const int32_t* filter_tails,
                                 const int32_t* filter_relations, int64_t nfilter, int64_t* ranks /* [nq][2] */,
                                 int64_t* counted /* [nq][2] or NULL */);

/* ---- Entity fold-in: give new entities a row without retraining.  The free
 * entities' rows of the device entity table are learnt from example triples
 * while everything else is frozen: every other entity row, the relation and
 * weight tables, the training state, the glibc stream, the TransR work vectors
 * and kb2e_device_bytes are the same, bit for bit, before and after, and
 * training may continue afterwards.  Every model, distance, precision and dim a
 * context takes.  The call synchronises the stream first and last.
 *   Context values: width n, learning rate lr, margin g, distance (L1 / L2;
 *   TransH always L1).  A free entity f has a working row x in FP64; FP32 tables
 *   are widened on load and a free row is rounded to FP32 once, when it is
 *   stored at the end.  Every example holds exactly one free entity, as head or
 *   as tail.  For each free entity the call runs `epochs` passes over its
 *   examples in the caller's order; the free entities do not interact, and the
 *   result depends neither on their order nor on the launch geometry.  For pass
 *   p and example i (its index in the caller's arrays), triple (h, t, r):
 *   1. Slot: side 0 corrupts the head, 1 the tail, 2 a fair coin (the
 *      reference's unif): the top bit of u(p, i, 0), 1 = tail.  The stream is
 *      kb2e_corrupt_triples' SplitMix64, stateless (the glibc stream is not
 *      touched):  state = mix(seed),
 *                 u(p, i, a) = mix(state + ((p * count + i) << 7) + a).
 *   2. Negative: for draws a = 1..32, e = u(p, i, a) % |E|; a draw is rejected
 *      if e is a free entity (any of them), if e is the entity it replaces, or
 *      if the new triple is among the `known` triples or the examples.  The
 *      first accepted draw gives the corrupted triple; without one the sample is
 *      skipped and counted as failed.  (So no row is read that the call writes.)
 *   3. Energies E+ and E- of the two triples: kb2e_score_triples' stateless
 *      formulas with x as the row of f (TransR from zeroed work vectors;
 *      transr_compat is ignored); sums over the row are 64-lane reductions.
 *   4. Hinge: unless E+ + g > E- the sample is done.  Otherwise
 *      loss_p += g + E+ - E- and the sample counts as active.
 *   5. Update, y = x first; then the positive triple with b = -1 and the
 *      corrupted triple with b = +1, skipping a triple that does not hold f (the
 *      corrupted one, when f's own slot was replaced).  Every gradient is taken
 *      at x, the row before this sample (the reference's snapshot rule for a
 *      batch of one sample).  Per triple:
 *      TransE (transe/trainer.cpp:28-45): g_k = 2 (t_k - h_k - r_k), under L1
 *        then 1 if g_k > 0 and -1 otherwise; f the head: y_k -= b lr g_k, f the
 *        tail: y_k += b lr g_k; then norm(y), which scales to unit length only
 *        if |y| > 1.
 *      TransH (transh/trainer.cpp:14-37): hs = w.h, ts = w.t, g_k the L1 sign of
 *        2 ((t_k - ts w_k) - (h_k - hs w_k) - r_k); y and norm(y) as TransE;
 *        then, against the stored w: while w.y > 0.1, y -= lr w.
 *      TransR (transr/trainer.cpp:147-176): hp_k = sum_j W[j][k] h_j, tp_k
 *        likewise, g_k = 2 (tp_k - hp_k - r_k) with the L1 sign as above; f the
 *        head: y_j -= b lr g_k W[j][k] for k ascending (f the tail: +=); then y
 *        is scaled to unit length (always); then, against the stored W with
 *        q = yW: while sum_k q_k^2 > 1, y_j -= lr sum_k 2 q_k W[j][k].  That
 *        loop is the gradient step of |yW|^2, the simultaneous form of the
 *        reference's transRNorm with the matrix held fixed; it differs from the
 *        reference's in-place column sweep by O(lr^2) -- deliberately: W is
 *        frozen here, and a sweep costs two dependent wave steps instead of n.
 *      A coupling loop makes at most max_sweeps steps (0 means 10000); one that
 *      still fails its test then stops with the row as it stands and counts as
 *      capped.  The cap is a safety bound, not a tuning knob.
 *   6. x = y.
 *   For TransE this is the reference's prebatch; train_kb; postbatch on a
 *   one-sample batch with every row but f's put back afterwards, and the same
 *   holds for TransH and TransR whenever neither coupling loop fires.
 * rows_in [nfree][dim] gives the rows to start from (NULL: the rows as they
 * stand in the table); rows_out [nfree][dim] (may be NULL) receives the rows as
 * stored; loss[f*2 + 0..1] = the first and the last pass's loss of free entity
 * f; counts[f*3 + 0..2] = its active, failed and capped counts over all passes.
 * A free entity without examples is legal: its row is rows_in's or unchanged
 * and its loss is 0.  nknown == 0 and count == 0 with NULL arrays are legal.
 * One wave owns one free entity for all passes, its row in registers; TransR
 * stages the sample's matrix in LDS up to n = 141 and reads it from L2 above
 * (KB2E_FOLD_W_L2=1 forces that; KB2E_FOLD_GRID=<n> caps the workgroups: tests).
 * KB2E_EINVAL: nfree < 1, epochs < 1, a side other than 0 / 1 / 2,
 * max_sweeps < 0, an id out of range, a free id listed twice, an example with
 * no free entity or with a free entity in both slots (the same one or two
 * different ones), a NULL array with a count > 0.  KB2E_ESTATE: no embeddings
 * on the device.  New relations are folded in by kb2e_fold_in_relations. */
kb2e_status kb2e_fold_in_entities(kb2e_ctx* ctx, const int32_t* free_entities, int64_t nfree,
                                  const int32_t* heads, const int32_t* tails, const int32_t* relations, int64_t count,
                                  const int32_t* known_heads, const int32_t* known_tails,
                                  const int32_t* known_relations, int64_t nknown, int32_t epochs, uint64_t seed,
                                  int32_t side, int32_t max_sweeps, const double* rows_in /* [nfree][dim] or NULL */,
                                  double* rows_out /* [nfree][dim] or NULL */, double* loss /* [nfree][2] */,
                                  int64_t* counts /* [nfree][3] */);

/* ---- Relation fold-in: give new relations their parameters without
 * retraining.  For each free relation rho the call learns its row of the
 * relation table, for TransH also its normal w and for TransR also its matrix W,
 * from example triples, while everything else is frozen: the entity table, every
 * other relation's rows, the training state, the glibc stream, the TransR work
 * vectors and kb2e_device_bytes are the same, bit for bit, before and after, and
 * training may continue afterwards.  Every model, distance, precision and dim a
 * context takes.  The call synchronises the stream first and last.
 *   In one sentence: for each free relation, the reference's `prebatch;
 *   train_kb ...; postbatch` (common/trainer.cpp:69-149) over that relation's
 *   examples, with every statement that writes an entity row removed.
 *   Working precision: working values are FP64; FP32 tables are widened on load
 *   and the free rows are rounded once, at the final store.
 *   Examples and batches: every example's relation must be a free relation.  Per
 *   free relation the call runs `epochs` passes over its examples in the caller's
 *   order; a pass is cut into consecutive batches of batch_size samples, the last
 *   one may be shorter, and a batch_size above the relation's example count means
 *   one batch.  batch_size = 1 is the reference's one-sample batch, the rule
 *   kb2e_fold_in_entities uses.  Free relations do not interact; the result
 *   depends neither on their order nor on the launch geometry.
 *   Per sample (pass p, example i = its index in the caller's arrays, triple
 *   (h, t, rho)): the slot and the negative are kb2e_fold_in_entities' steps 1
 *   and 2 -- the same stateless SplitMix64 stream with the counter p * count + i,
 *   side 0 / 1 / 2 and 32 draws; a draw is rejected if it equals the entity it
 *   replaces or if the new triple is among `known` or the examples.  There is no
 *   free-entity rule: every entity row is frozen and readable.  Without an
 *   accepted draw the sample is skipped and counted as failed.
 *   Phase 1, at the batch's snapshot (rho's parameters as the batch finds
 *   them): E+ and E- are kb2e_score_triples' stateless formulas (transr_compat is
 *   ignored, the work vectors are zero).  A sample is active iff E+ + g > E-; it
 *   then adds g + E+ - E- to the pass's loss, which is summed in sample order.
 *   For each triple of an active sample the quantities of the reference's
 *   gradientUpdate are taken from the snapshot only: x_k = 2 (t'_k - h'_k - r_k)
 *   of the model's features (under L1: 1 if that is > 0, else -1); TransH also
 *   headSum = w.h, tailSum = w.t and sum_x = sum_k x_k w_k; TransR x_k from the
 *   projections by the snapshot W.
 *   Phase 2, in sample order, on the working copy of rho's parameters: for every
 *   active sample the positive triple with b = -1, then the corrupted triple with
 *   b = +1.  Per triple (head h, tail t):
 *     TransE (transe/trainer.cpp:28-45): r_k -= b lr x_k; norm(r), which scales
 *       to unit length only if |r| > 1.
 *     TransH (transh/trainer.cpp:18-58): r_k -= b lr x_k; w_k += b lr x_k
 *       headSum; w_k -= b lr x_k tailSum; w_k += b lr sum_x h_k; w_k -= b lr sum_x
 *       t_k; norm(r); norm(w, false); norm(r, w, lr) exactly, including its
 *       running `sum` (common/utils.cpp:79-111); then norm(h, w, lr) and
 *       norm(t, w, lr) with the statement that writes the entity
 *       (a[i] -= rate * b[i]) removed, so w alone moves.
 *     TransR (transr/trainer.cpp:147-187): W[j][i] -= b lr x_i (h_j - t_j);
 *       r_i -= b lr x_i; norm(r, false); every row of W normed with false; then
 *       transRNorm for the head, the tail and the reference's third call -- on
 *       the entity whose id is the relation's id (trainer.cpp:187), skipped when
 *       that id >= |E| -- with a[j] -= ... removed.  With a frozen the columns
 *       decouple and a sweep is exactly W -= 2 lr a (x) (aW): no O(lr^2)
 *       deviation remains, unlike kb2e_fold_in_entities.
 *   Every loop against an entity row, and the r / w loop of TransH, makes at most
 *   max_sweeps steps (0 means 10000); one that still fails its test then stops
 *   (TransH: with the closing norm(w, false) still applied) and counts as capped.
 *   The cap is a safety bound, not a tuning knob.
 *   For TransE this is the reference's batch with the entity rows put back, bit
 *   for bit up to the order of sums; for TransH and TransR the same holds
 *   whenever no loop against an entity row fires.
 * rel_in [nfree][dim] and w_in [nfree][dim] (TransH) / [nfree][dim][dim]
 * (TransR, [j][i] as the weight table) give the parameters to start from (NULL:
 * as they stand in the tables); rel_out and w_out (may be NULL) receive them as
 * stored; loss[f*2 + 0..1] = the first and the last pass's loss of free relation
 * f; counts[f*3 + 0..2] = its active, failed and capped counts over all passes.
 * A free relation without examples is legal: its parameters are rel_in's / w_in's
 * or unchanged and its loss is 0.  nknown == 0 and count == 0 with NULL arrays
 * are legal.
 * One 256-thread workgroup owns one free relation for all passes: phase 1
 * spreads a batch's samples over its four waves and leaves one record a sample
 * (in LDS while a batch's records fit 32 KiB, else in a scratch of min(batch_size,
 * longest relation) * 2 (dim + 4) doubles per workgroup, allocated in the call and
 * freed before it returns), phase 2 applies the records in order.  The TransR
 * matrix lives in LDS up to dim = 131 and in a global scratch above
 * (KB2E_FOLDREL_W_L2=1 forces that; KB2E_FOLDREL_GRID=<n> caps the workgroups:
 * tests).
 * KB2E_EINVAL: nfree < 1, epochs < 1, batch_size < 1, a side other than 0 / 1 /
 * 2, max_sweeps < 0, an id out of range, a free relation listed twice, an example
 * whose relation is not free, a NULL array with a count > 0, w_in / w_out given
 * for TransE.  KB2E_ESTATE: no embeddings on the device. */
kb2e_status kb2e_fold_in_relations(kb2e_ctx* ctx, const int32_t* free_relations, int64_t nfree,
                                   const int32_t* heads, const int32_t* tails, const int32_t* relations, int64_t count,
                                   const int32_t* known_heads, const int32_t* known_tails,
                                   const int32_t* known_relations, int64_t nknown, int32_t epochs, int64_t batch_size,
                                   uint64_t seed, int32_t side, int32_t max_sweeps,
                                   const double* rel_in /* [nfree][dim] or NULL */,
                                   const double* w_in /* [nfree][dim or dim*dim] or NULL */,
                                   double* rel_out /* [nfree][dim] or NULL */,
                                   double* w_out /* [nfree][dim or dim*dim] or NULL */, double* loss /* [nfree][2] */,
                                   int64_t* counts /* [nfree][3] */);

/* Raw glibc stream access (the context's RNG, as std::rand() in the reference). */
int32_t kb2e_rng_next(kb2e_ctx* ctx);

/* Timing of the engine's device kernels on the engine's own HIP stream (HIP
 * events around each launch; off by default).  `name` is a kernel family
 * ("score", "fold", "apply", "relowner", "index", "sample", ...; kb2e_predict:
 * "predict_score", "predict_mask", "predict_select"; kb2e_predict_relations /
 * kb2e_rank_relations: "relpred_score" (projection + key write), "relpred_mask",
 * "relpred_select", "relpred_rank"; kb2e_predict_joint / kb2e_rank_joint:
 * "joint_score" (projection + the constraint rows), "joint_combine" (the sums),
 * "joint_mask", "joint_select", "joint_rank"; kb2e_predict_path / kb2e_rank_path:
 * "path_score" (projections + hop 1), "path_hop" (the fused min-plus hops),
 * "path_select" (frontiers, answers and their predecessors), "path_mask",
 * "path_rank"; kb2e_fit_thresholds / kb2e_classify_triples:
 * "classify_score" (energies, and the comparison of kb2e_classify_triples),
 * "classify_sort" (every radix pass), "classify_fit" (segment starts and both
 * sweeps); kb2e_corrupt_triples: "classify_corrupt"; kb2e_complete_triples:
 * "complete_score" (projection + the tile kernel), "complete_select";
 * kb2e_neighbors: "neighbors_score" (projection + the fused score and select
 * kernel), "neighbors_merge"; kb2e_score_candidates / kb2e_rank_candidates:
 * "candidates_project" (TransR: the compact or full projection of a chunk's
 * relation), "candidates_score", "candidates_rank" (the work-item kernel, with
 * the comparisons, filter probes and counts when ranking);
 * kb2e_fold_in_entities: "foldin"; kb2e_fold_in_relations: "foldrel").  Returns total
 * milliseconds and launch count since kb2e_profile_enable.  on = 0: off;
 * on = P >= 1: the batch kernels of every P-th batch are timed (event records
 * cost device time of their own; sampling keeps the rest of the run unperturbed),
 * per-epoch kernels always. */
kb2e_status kb2e_profile_enable(kb2e_ctx* ctx, int32_t on);
kb2e_status kb2e_profile_query(kb2e_ctx* ctx, const char* name, double* total_ms, int64_t* launches);

/* Schedule counters kept on the device (no reference counterpart: they say which
 * branch of a schedule choice ran, for tests and tools).  Synchronises the
 * context's stream.  Names: "transh_orth_rel_batches" -- PARALLEL TransH batches
 * whose normOrth relation pass ran (the gate on the previous batch's normOrth
 * work, kernels_transh_parallel.hpp); the other batches took the one-wave pass
 * alone.  Of the last kb2e_complete_triples call (kept on the host):
 * "complete_candidates" -- pairs scored, "complete_records" -- records
 * appended, "complete_strips" -- score + select steps,
 * "complete_buffer_records" -- the record buffer's capacity in records.
 * Of the last kb2e_neighbors call: "neighbors_candidates" -- pairs scored,
 * "neighbors_slices" -- (tile, candidate slice) workgroups of the fused kernel,
 * "neighbors_chunks" -- runs of queries that shared the partial records,
 * "neighbors_prunes" -- cuts of a row's list to its k best, each of which
 * lowered that row's bound.
 * Of the last kb2e_score_candidates / kb2e_rank_candidates call:
 * "candidates_listings" -- listings scored, "candidates_items" -- wave-sized
 * work items (at most 64 listings each; 63 when ranking, where the last lane
 * scores the truth), "candidates_chunks" -- runs of queries that shared the
 * device buffers, "candidates_projections" -- TransR projections made (one per
 * chunk and relation), "candidates_probes" -- filter-set probes.
 * Of the last kb2e_predict_joint / kb2e_rank_joint call (kept on the host):
 * "joint_chunks" -- runs of queries that shared the key buffer, "joint_rows" --
 * constraint rows scored, "joint_projections" -- per-relation projections made.
 * Of the last kb2e_predict_path / kb2e_rank_path call: "path_chunks" -- runs of
 * queries that shared the device rows, "path_hops" -- query-levels the hop
 * kernel ran (hops 2..L of every query), "path_projections" -- per-relation
 * projections made.
 * A constant of the build: "foldrel_lds_limit" -- the widest TransR matrix
 * kb2e_fold_in_relations keeps in LDS.
 * KB2E_EINVAL for an unknown name. */
kb2e_status kb2e_counter(kb2e_ctx* ctx, const char* name, int64_t* value);

/* Device memory the context holds, in bytes: every device buffer it has allocated
 * and not freed (tables, epoch streams and index, exports, merge state). */
int64_t kb2e_device_bytes(const kb2e_ctx* ctx);

/* Multi-GPU epoch merge (the reference is single-process, so
 * this replaces no reference call: it is the exchange step that lets N
 * contexts, each training a head-hash shard of the triples with the
 * single-GPU schedule, act as one trainer).  At an epoch boundary every rank
 * holds T_r; the merge sets, on every rank,
 *     T <- renorm(T0 + sum_r (T_r - T0))
 * where T0 is the tables after the previous merge: the entity deltas are
 * reduce-scattered to the owner of each block of rows over RCCL, the owner
 * adds them and re-applies the model's norm constraint (as kb2e_renormalize) to
 * the changed units -- a unit (a row; for the TransR weights one relation's
 * whole matrix) is renormalised when its SUMMED delta has a non-zero element,
 * and a row whose deltas cancel exactly across the ranks is left as it was --
 * and an all-gather returns the merged table; relation and weight deltas are
 * all-reduced and every rank renormalises the changed units.  All work runs on the contexts' own streams; the calls return
 * when the merged tables are in place.  Two ways to build the communicator:
 *  - one process per GPU (torchrun): rank 0 makes an id with
 *    kb2e_comm_unique_id, the caller hands it to every rank (any side channel),
 *    and each rank calls kb2e_comm_init_rank (collective) and then
 *    kb2e_merge_epoch at every epoch boundary (collective);
 *  - one process driving N devices (one host thread, SURVEY.md 8(b)
 *    "Threading"): kb2e_comm_init_group over the N contexts, then
 *    kb2e_merge_epoch_group.  Contexts that all share one device (or
 *    KB2E_MERGE_LOCAL=1, which also needs one device) merge with plain device
 *    kernels instead of RCCL, which refuses two ranks on one GPU; a group that
 *    mixes shared and distinct devices is KB2E_EUNSUPPORTED.
 * Initialisation broadcasts rank 0's tables to every rank, so the ranks may
 * be created with different seeds (distinct sample streams).  The contexts must
 * agree on model, dim, table sizes and precision (kb2e_comm_init_rank checks
 * the other ranks' over the new communicator: KB2E_EINVAL on a difference);
 * their tables must be loaded (kb2e_init_params / kb2e_upload_params /
 * kb2e_transr_seed) first.  A failed init leaves the context without a
 * communicator, so it can be retried.  The N > 1 RCCL paths (several
 * processes, or ncclCommInitAll over several devices) are built for the
 * 8-GPU driver run and are not exercised on the one-GPU test box: the tests
 * cover one RCCL rank and the shared-device local backend. */
#define KB2E_COMM_ID_BYTES 128
kb2e_status kb2e_comm_unique_id(uint8_t* id /* KB2E_COMM_ID_BYTES */);
kb2e_status kb2e_comm_init_rank(kb2e_ctx* ctx, int32_t nranks, int32_t rank, const uint8_t* id);
kb2e_status kb2e_comm_init_group(kb2e_ctx* const* ctxs, int32_t n);
kb2e_status kb2e_merge_epoch(kb2e_ctx* ctx);
kb2e_status kb2e_merge_epoch_group(kb2e_ctx* const* ctxs, int32_t n);
/* This rank's place in the communicator and the entity rows it owns in the merge. */
kb2e_status kb2e_comm_info(kb2e_ctx* ctx, int32_t* nranks, int32_t* rank, int64_t* first_entity,
                           int64_t* entity_count);

/* Raw device pointers of the parameter tables (row-major, leading dimension
 * round_up(dim, 2), FP64 or FP32 by precision) and their element counts, for a
 * caller-side communicator (kb2e_amd/distributed.py: torch.distributed gloo in
 * the CPU tests). */
kb2e_status kb2e_device_tables(kb2e_ctx* ctx, void** entity, void** relation, void** weights,
                               int64_t* n_entity, int64_t* n_relation, int64_t* n_weights);
/* Re-apply the per-row norm constraints of the model, to the rows flagged
 * non-zero in the host masks (NULL = every row): TransE rows and TransH
 * entity/relation rows are shrunk to length <= 1 (common/utils.cpp:70-77),
 * TransH normals and TransR entity/relation/matrix rows scaled to unit length
 * (transh/trainer.cpp:52, transr/trainer.cpp:174-180).  Weight masks are per
 * relation. */
kb2e_status kb2e_renormalize(kb2e_ctx* ctx, const uint8_t* entity_rows, const uint8_t* relation_rows,
                             const uint8_t* weight_rows);
/* The same constraint on `count` units of one table from `first` (table 0:
 * entities, 1: relations, 2: weights, in relations), with the row mask in
 * DEVICE memory (device_mask[k] for unit first + k; NULL = every row).
 * Returns when the rows are renormalised. */
kb2e_status kb2e_renormalize_rows(kb2e_ctx* ctx, int32_t table, int64_t first, int64_t count,
                                  const uint8_t* device_mask);

#ifdef __cplusplus
}
#endif

#endif /* KB2E_ENGINE_H_ */
