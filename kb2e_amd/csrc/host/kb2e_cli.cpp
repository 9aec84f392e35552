// kb2e_cli.cpp -- drop-in command-line front end: trainTransE / trainTransH /
// trainTransR and evalTransE / evalTransH / evalTransR (dispatch on argv[0]),
// plus predictTransE / predictTransH / predictTransR (no reference counterpart:
// top-k answers to (h, ?, r) / (?, t, r) entity queries and (h, t, ?) relation
// queries from the trained tables; --queries FILE, --topk K, --filtered 0|1)
// and classifyTransE / classifyTransH / classifyTransR (triple classification:
// thresholds fitted on the valid split, accuracy on the test split) and
// completeTransE / completeTransH / completeTransR (knowledge-base completion:
// the top-k new triples of each relation) and foldinTransE / foldinTransH /
// foldinTransR (entity fold-in: rows for new entities with the trained tables
// frozen) and foldrelTransE / foldrelTransH / foldrelTransR (relation fold-in:
// parameters for new relations with everything else frozen) and jointTransE /
// jointTransH / jointTransR (conjunctive queries: the top-k entities that fit
// several patterns at once) and pathTransE / pathTransH / pathTransR (path
// queries: the top-k entities at the end of a relation path) and
// neighborsTransE / neighborsTransH / neighborsTransR (entity neighbours: the
// k nearest entities of given entities or of all, and the mutual pairs) and
// candidatesTransE / candidatesTransH / candidatesTransR (candidate lists:
// given entities ordered and a truth ranked among them; type-constrained
// evaluation).
//
// Same flags, defaults, stdout lines and files as the reference binaries
// (transe/bin/trainTransE.cpp, common/args.cpp, common/loader.cpp,
// common/trainer.cpp:109-127, common/evaluation.cpp:181-266).  The Trainer
// class below keeps the shape of common::Trainer (common/trainer.h:14-78):
// add / loadFiles / train / write, with prepTrain and bfgs as the overridable
// steps -- and bfgs() runs on the GPU through include/kb2e_engine.h.
// GPU-only flags are additive: --precision 64|32, --device N, --transrcompat 0|1,
// --schedule 0|1 (0 = ORDERED, the reference's sequence; 1 = PARALLEL, summed
// per-row deltas with one norm per batch, kb2e_engine.h kb2e_schedule), --gpus N,
// --subbatches K (PARALLEL TransR: each batch applied in K sub-batches).
#include <sys/stat.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <fstream>
#include <functional>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "../../../include/kb2e_engine.h"
#include "../classify_host.hpp"
#include "../neighbors_host.hpp"

namespace kb2e_host {

// ------------------------------------------------------------ arguments

enum { METHOD_UNIF = 0, METHOD_BERN = 1 };
const char* method_name(int m) { return m == METHOD_UNIF ? "unif" : "bern"; }

struct EmbeddingArguments {  // common/args.h:9-25, defaults common/constants.h:28-40
    std::string dataDir = "../data";
    std::string outputDir = ".";
    int embeddingSize = 100;
    double learningRate = 0.001;
    double margin = 1.0;
    int method = METHOD_BERN;
    int numBatches = 100;
    int maxEpochs = 1000;
    int distanceType = 0;
    std::string seedDataDir = ".";
    int seedMethod = METHOD_UNIF;
    unsigned int seed = (unsigned int)time(NULL);
    // GPU engine options (additive)
    int precision = 64;
    int device = 0;
    int transrCompat = 1;
    int schedule = 0;
    int gpus = 1;
    int subBatches = 0;  // 0: the engine's default (kb2e_config.sub_batches)

    std::string to_string() const {  // common/args.cpp:33-50
        std::string r = "Options: [";
        r += "datadir: '" + dataDir + "', ";
        r += "outdir: '" + outputDir + "', ";
        r += "size: " + std::to_string(embeddingSize) + ", ";
        r += "rate: " + std::to_string(learningRate) + ", ";
        r += "margin: " + std::to_string(margin) + ", ";
        r += std::string("method: ") + method_name(method) + ", ";
        r += "batches: " + std::to_string(numBatches) + ", ";
        r += "epochs: " + std::to_string(maxEpochs) + ", ";
        r += "distance: " + std::to_string(distanceType) + ", ";
        r += "seeddatadir: '" + seedDataDir + "', ";
        r += std::string("seedmethod: ") + method_name(seedMethod) + ", ";
        r += "seed: " + std::to_string(seed) + "]";
        return r;
    }
};

// "-flag" or "--flag"; every flag needs a value (common/utils.cpp:55-68).
int argpos(const char* flag, bool hasValue, int argc, char** argv) {
    for (int i = 1; i < argc; i++) {
        if (!strcmp((std::string("-") + flag).c_str(), argv[i]) || !strcmp((std::string("--") + flag).c_str(), argv[i])) {
            if (hasValue && i == argc - 1) {
                printf("Argument missing for %s\n", flag);
                exit(1);
            }
            return i;
        }
    }
    return -1;
}

void printUsage(const char* invoked) {  // common/args.cpp:125-142
    printf("USAGE: %s [option value] ...\n", invoked);
    printf("       %s --help\n", invoked);
    printf("All options require a value.\n");
    printf("Options:\n");
    printf("   --datadir [../data]\n");
    printf("   --outdir [.]\n");
    printf("   --size [100]\n");
    printf("   --rate [0.001000]\n");
    printf("   --margin [1.000000]\n");
    printf("   --method [1 (bern)]\n");
    printf("   --batches [100]\n");
    printf("   --epochs [1000]\n");
    printf("   --distance [0]\n");
    printf("   --seeddatadir [.] (TransR only)\n");
    printf("   --seedmethod [0 (unif)] (TransR only)\n");
    printf("   --seed [now]\n");
    printf("   --precision [64] (GPU: 64 or 32)\n");
    printf("   --device [0] (GPU ordinal)\n");
    printf("   --transrcompat [1] (TransR: reproduce the accumulating energy)\n");
    printf("   --schedule [0] (GPU: 0 ordered = the reference's sequence, 1 parallel)\n");
    printf("   --gpus [1] (GPU: devices --device .. --device+N-1, triples sharded by head, epoch merge over RCCL)\n");
    printf("   --subbatches [engine default] (GPU, parallel TransR: each batch's updates in this many sub-batches)\n");
    printf("   --queries FILE (predictTrans*: head<TAB>tail<TAB>relation lines, ? for the unknown head, tail or relation)\n");
    printf("   --topk [10] (predictTrans*)\n");
    printf("   --filtered [1] (predictTrans*: known triples are not answers)\n");
    printf("   --queries FILE --topk [10] --filtered [1] (jointTrans*: query<TAB>head<TAB>tail<TAB>relation lines, ? for the unknown head or tail; consecutive lines with one query token are one conjunction)\n");
    printf("   --queries FILE --topk [10] --beam [64] --noloops --filtered [1] (pathTrans*: anchor<TAB>relation[<TAB>relation...] lines, a relation with a leading ^ is walked backwards; --beam 0: exact)\n");
    printf("   --negseed [0] (classifyTrans*: seed of the generated negatives; the test split uses seed + 1)\n");
    printf("   --constrained [1] (classifyTrans*: negatives from the entities seen in that slot of the relation)\n");
    printf("   --validlabels FILE (classifyTrans*: head<TAB>tail<TAB>relation<TAB>label lines, 1 / -1 or 0; instead of generated negatives)\n");
    printf("   --testlabels FILE (classifyTrans*: likewise for the test split)\n");
    printf("   --out FILE (classifyTrans*: label<TAB>energy of every classified test triple)\n");
    printf("   --relations FILE (completeTrans*: relation names, one per line; every relation without it)\n");
    printf("   --topk [10] --constrained [1] (completeTrans*: heads / tails from the entities seen in that slot of the relation)\n");
    printf("   --loops [0] (completeTrans*: 1 = head == tail may be an answer)\n");
    printf("   --filtered [1] (completeTrans*: known = train + valid + test; 0 = train + valid)\n");
    printf("   --queries FILE | --typed (candidatesTrans*: head<TAB>tail<TAB>relation<TAB>cand,cand,...[<TAB>truth] lines with ? in the unknown slot; or the type-constrained metrics of test.txt)\n");
    printf("   --entities FILE | --all, --topk [10] --relation NAME --self --pairs (neighborsTrans*: entity names, one per line, or every entity; the space of a relation instead of the entity space; the entity itself is a candidate; the mutual pairs instead of the lists)\n");
    printf("   --new FILE --foldout DIR (foldinTrans*: triples that mention the new entities; where the full entity table goes)\n");
    printf("   --epochs [1000] --seed [now] --side [2] (foldinTrans*: passes, seed of the new rows and of the negatives, slot to corrupt)\n");
    printf("   --new FILE --foldout DIR --epochs --seed --side --batch [1] (foldrelTrans*: the new relations' triples; where the full relation tables go; samples per batch)\n");
}

EmbeddingArguments parseArgs(int argc, char** argv) {  // common/args.cpp:53-122
    if (argpos("help", false, argc, argv) != -1) {
        printUsage(argv[0]);
        exit(0);
    }
    EmbeddingArguments a;
    int i;
    if ((i = argpos("datadir", true, argc, argv)) != -1) a.dataDir = argv[i + 1];
    if ((i = argpos("outdir", true, argc, argv)) != -1) a.outputDir = argv[i + 1];
    if ((i = argpos("size", true, argc, argv)) != -1) a.embeddingSize = atoi(argv[i + 1]);
    if ((i = argpos("rate", true, argc, argv)) != -1) a.learningRate = atof(argv[i + 1]);
    if ((i = argpos("margin", true, argc, argv)) != -1) a.margin = atof(argv[i + 1]);
    if ((i = argpos("method", true, argc, argv)) != -1) a.method = atoi(argv[i + 1]);
    if ((i = argpos("batches", true, argc, argv)) != -1) a.numBatches = atoi(argv[i + 1]);
    if ((i = argpos("epochs", true, argc, argv)) != -1) a.maxEpochs = atoi(argv[i + 1]);
    if ((i = argpos("distance", true, argc, argv)) != -1) a.distanceType = atoi(argv[i + 1]);
    if ((i = argpos("seeddatadir", true, argc, argv)) != -1) a.seedDataDir = argv[i + 1];
    if ((i = argpos("seedmethod", true, argc, argv)) != -1) a.seedMethod = atoi(argv[i + 1]);
    if ((i = argpos("seed", true, argc, argv)) != -1) a.seed = atoi(argv[i + 1]);
    if ((i = argpos("precision", true, argc, argv)) != -1) a.precision = atoi(argv[i + 1]);
    if ((i = argpos("device", true, argc, argv)) != -1) a.device = atoi(argv[i + 1]);
    if ((i = argpos("transrcompat", true, argc, argv)) != -1) a.transrCompat = atoi(argv[i + 1]);
    if ((i = argpos("schedule", true, argc, argv)) != -1) a.schedule = atoi(argv[i + 1]) ? 1 : 0;
    if ((i = argpos("gpus", true, argc, argv)) != -1) a.gpus = std::max(1, atoi(argv[i + 1]));
    if ((i = argpos("subbatches", true, argc, argv)) != -1) a.subBatches = std::max(1, atoi(argv[i + 1]));
    return a;
}

bool fileExists(const std::string& path) {
    struct stat b;
    return stat(path.c_str(), &b) == 0;
}

// -------------------------------------------------------------- loader

void loadIdFile(const std::string& path, std::map<std::string, int>& ids) {  // common/loader.cpp:15-24
    FILE* f = fopen(path.c_str(), "r");
    if (!f) {
        printf("Could not open id file: %s\n", path.c_str());
        exit(2);
    }
    char buf[512];
    int id;
    while (fscanf(f, "%511s\t%d", buf, &id) == 2) ids[std::string(buf)] = id;
    fclose(f);
}

void loadTripleFile(const std::string& path, std::map<std::string, int>& ent, std::map<std::string, int>& rel,
                    const std::function<void(int, int, int)>& cb) {  // common/loader.cpp:26-62
    FILE* f = fopen(path.c_str(), "r");
    if (!f) {
        printf("Could not open triple file: %s\n", path.c_str());
        exit(2);
    }
    char hb[512], tb[512], rb[512];
    while (fscanf(f, "%511s\t%511s\t%511s", hb, tb, rb) == 3) {
        bool fail = false;
        if (!ent.count(hb)) {
            std::cout << "Head entity found in triple file that was not found in the identity file: " << hb << std::endl;
            fail = true;
        }
        if (!ent.count(tb)) {
            std::cout << "Tail entity found in triple file that was not found in the identity file: " << tb << std::endl;
            fail = true;
        }
        if (!rel.count(rb)) {
            std::cout << "Relation found in triple file that was not found in the identity file: " << rb << std::endl;
            fail = true;
        }
        if (fail) continue;
        cb(ent[hb], ent[tb], rel[rb]);
    }
    fclose(f);
}

void check(kb2e_ctx* ctx, kb2e_status st, const char* what) {
    if (st != KB2E_OK) {
        printf("kb2e engine error in %s (status %d): %s\n", what, (int)st, ctx ? kb2e_last_error(ctx) : "");
        exit(1);
    }
}

// common/trainer.cpp:109-127: "%.6lf\t" per value, "\n" per row, from the
// device table (formatted on the device).
void writeTable(kb2e_ctx* ctx, int table, const std::string& path) {
    if (kb2e_write_table(ctx, table, path.c_str()) != KB2E_OK) {
        printf("Could not open output file: %s\n", path.c_str());
        exit(1);
    }
}

// transr/trainer.cpp:90-113: the seed file into a device table (parsed on the
// device), with the reference's message when it holds too few numbers.
void readSeed(kb2e_ctx* ctx, int table, const std::string& path, int mode) {
    if (kb2e_read_table(ctx, table, path.c_str(), mode) != KB2E_OK) {
        printf("Failed to read embedding values from seed file: '%s'\n", path.c_str());
        exit(1);
    }
}

// ------------------------------------------------------------- trainer

class Trainer {  // the interface of common::Trainer (common/trainer.h:14-78)
   public:
    Trainer(EmbeddingArguments args, kb2e_model model) : args_(args), model_(model) {}
    virtual ~Trainer() {
        for (kb2e_ctx* c : ranks_) kb2e_destroy(c);
    }

    void add(int head, int tail, int relation) {
        heads_.push_back(head);
        tails_.push_back(tail);
        relations_.push_back(relation);
    }

    void loadFiles() {  // common/trainer.cpp:151-201
        std::map<std::string, int> entity2id, relation2id;
        loadIdFile(args_.dataDir + "/entity2id.txt", entity2id);
        loadIdFile(args_.dataDir + "/relation2id.txt", relation2id);
        loadTripleFile(args_.dataDir + "/train.txt", entity2id, relation2id,
                       [this](int h, int t, int r) { this->add(h, t, r); });
        numRelations_ = (int)relation2id.size();
        numEntities_ = (int)entity2id.size();
        std::cout << "Number of Relations: " << relation2id.size() << std::endl;
        std::cout << "Number of Entities: " << entity2id.size() << std::endl;
    }

    void train() {  // common/trainer.cpp:60-63
        prepTrain();
        if (ranks_.size() > 1)  // rank 0's tables everywhere, the merge's communicator
            check(ctx_, kb2e_comm_init_group(ranks_.data(), (int32_t)ranks_.size()), "comm_init_group");
        bfgs();
    }

    // common/trainer.cpp:109-127: the device tables formatted on the device
    virtual void write() {
        const std::string m = method_name(args_.method);
        writeTable(ctx_, 1, args_.outputDir + "/relation2vec." + m);
        writeTable(ctx_, 0, args_.outputDir + "/entity2vec." + m);
    }

   protected:
    EmbeddingArguments args_;
    kb2e_model model_;
    kb2e_ctx* ctx_ = nullptr;          // rank 0 (the tables write() prints)
    std::vector<kb2e_ctx*> ranks_;     // one context per GPU (--gpus)
    int numRelations_ = 0, numEntities_ = 0;
    std::vector<int> heads_, tails_, relations_;

    // common/trainer.cpp:34-58: the initial tables, drawn from the same
    // glibc stream (seeded with --seed) inside the engine.  --gpus N: one
    // context per device, each training the triples whose head hashes to it
    //  in batches of the single-GPU size (numBatches / N
    // batches an epoch), rank k seeded with seed + k (distinct sample streams;
    // the merge starts every rank from rank 0's tables).
    virtual void prepTrain() {
        const int N = args_.gpus;
        for (int k = 0; k < N; ++k) {
            std::vector<int> h, t, r;
            for (size_t i = 0; i < heads_.size(); ++i)
                if (N == 1 || head_owner(heads_[i], N) == k) {
                    h.push_back(heads_[i]);
                    t.push_back(tails_[i]);
                    r.push_back(relations_[i]);
                }
            ranks_.push_back(make_rank(k, h, t, r));
        }
        ctx_ = ranks_[0];
    }

    // common/trainer.cpp:69-107, on the GPU.
    virtual void bfgs() {
        const int32_t nb = (int32_t)std::max(1, args_.numBatches / args_.gpus);
        for (int epoch = 0; epoch < args_.maxEpochs; epoch++) {
            double loss = 0;
            int64_t active = 0;
            if (ranks_.size() == 1) {
                check(ctx_, kb2e_train_epoch(ctx_, &loss, &active), "train_epoch");
            } else {
                for (kb2e_ctx* c : ranks_) check(c, kb2e_train_batches(c, nb), "train_batches");  // queued
                for (kb2e_ctx* c : ranks_) {
                    double l = 0;
                    int64_t a = 0;
                    check(c, kb2e_take_stats(c, &l, &a), "take_stats");
                    loss += l;
                    active += a;
                }
                check(ctx_, kb2e_merge_epoch_group(ranks_.data(), (int32_t)ranks_.size()), "merge_epoch");
            }
            printf("Epoch: %d, Loss: %f\n", epoch, loss);
            fflush(stdout);
        }
    }

    // the shard owner of a head entity (kb2e_amd/distributed.py shard_heads)
    static int head_owner(int head, int world) {
        const uint64_t h = (uint64_t)(uint32_t)head * 0x9E3779B97F4A7C15ull;
        return (int)((h >> 40) % (uint64_t)world);
    }

    kb2e_ctx* make_rank(int k, const std::vector<int>& h, const std::vector<int>& t, const std::vector<int>& r) {
        kb2e_config cfg;
        kb2e_default_config(&cfg);
        cfg.model = model_;
        cfg.dim = args_.embeddingSize;
        cfg.num_entities = numEntities_;
        cfg.num_relations = numRelations_;
        cfg.learning_rate = args_.learningRate;
        cfg.margin = args_.margin;
        cfg.method = args_.method;
        cfg.distance = args_.distanceType;
        cfg.num_batches = std::max(1, args_.numBatches / args_.gpus);
        cfg.seed = args_.seed + (unsigned)k;
        cfg.precision = args_.precision;
        // KB2E_CLI_ONE_DEVICE=1: every rank on --device (the one-GPU test box; the
        // merge then runs on the engine's local backend instead of RCCL)
        const char* one = getenv("KB2E_CLI_ONE_DEVICE");
        cfg.device = (one && one[0] == '1') ? args_.device : args_.device + k;
        cfg.transr_compat = args_.transrCompat;
        cfg.schedule = args_.schedule ? KB2E_SCHEDULE_PARALLEL : KB2E_SCHEDULE_ORDERED;
        if (args_.subBatches > 0) cfg.sub_batches = args_.subBatches;
        if (h.empty()) {
            printf("kb2e: GPU %d has no training triples (--gpus %d)\n", k, args_.gpus);
            exit(1);
        }
        kb2e_ctx* c = nullptr;
        check(nullptr, kb2e_create(&cfg, &c), "create");
        check(c, kb2e_upload_triples(c, h.data(), t.data(), r.data(), (int64_t)h.size()), "upload_triples");
        // the reference's randn draws and row norms, made on the device from the
        // same stream (kb2e_init_params is the host form of the same thing)
        int64_t ties = 0;
        check(c, kb2e_init_params_device(c, nullptr, nullptr, nullptr, &ties), "init_params");
        if (ties > 0) {
            // an accept/reject decision sat within a few ulps of the density, where
            // the device exp could round unlike glibc's: redo the init on the host
            // (exact) from a fresh context, so the stream position is the reference's
            fprintf(stderr, "kb2e: %lld near-tie randn decisions on the device; initialising on the host\n",
                    (long long)ties);
            kb2e_destroy(c);
            c = nullptr;
            check(nullptr, kb2e_create(&cfg, &c), "create");
            check(c, kb2e_upload_triples(c, h.data(), t.data(), r.data(), (int64_t)h.size()), "upload_triples");
            check(c, kb2e_init_params(c, nullptr, nullptr, nullptr), "init_params");
        }
        return c;
    }
};

class TransHTrainer : public Trainer {  // transh/trainer.cpp:94-105
   public:
    using Trainer::Trainer;
    void write() override {
        Trainer::write();
        writeTable(ctx_, 2, args_.outputDir + "/weights." + method_name(args_.method));
    }
};

class TransRTrainer : public Trainer {
   public:
    using Trainer::Trainer;
    void write() override {  // transr/trainer.cpp:128-142
        Trainer::write();
        writeTable(ctx_, 2, args_.outputDir + "/weights." + method_name(args_.method));
    }

   protected:
    void prepTrain() override {  // transr/trainer.cpp:70-114
        Trainer::prepTrain();
        // seed files parsed on the device; entities unit-normed, relations verbatim
        // (rank 0's tables are broadcast to the other ranks by the merge's init)
        std::string path = args_.seedDataDir + "/entity2vec." + method_name(args_.seedMethod);
        readSeed(ctx_, 0, path, KB2E_READ_UNIT);
        path = args_.seedDataDir + "/relation2vec." + method_name(args_.seedMethod);
        readSeed(ctx_, 1, path, KB2E_READ_VERBATIM);
    }
};

int train_main(int argc, char** argv, kb2e_model model) {
    EmbeddingArguments args = parseArgs(argc, argv);
    printf("%s\n", args.to_string().c_str());
    Trainer* t = model == KB2E_TRANSE ? new Trainer(args, model)
                 : model == KB2E_TRANSH ? (Trainer*)new TransHTrainer(args, model)
                                        : (Trainer*)new TransRTrainer(args, model);
    t->loadFiles();
    t->train();
    t->write();
    delete t;
    return 0;
}

// ------------------------------------------------------------- evaluation

double vec_len(const double* a, int n) {
    double res = 0;
    for (int i = 0; i < n; i++) res += a[i] * a[i];
    return std::sqrt(res);
}

// What the eval and predict binaries load: the id files, the three triple files
// (test triples; filter = test + train + valid, common/evaluation.cpp:41-62) and
// a context holding the embedding files (EmbeddingEvaluation::loadEmbeddings).
struct LoadedModel {
    std::map<std::string, int> entity2id, relation2id;
    std::vector<int> th, tt, tr, fh, ft, fr;
    kb2e_ctx* ctx = nullptr;
};

void load_model(const EmbeddingArguments& args, kb2e_model model, LoadedModel& L) {
    const std::string m = method_name(args.method);
    const std::string relPath = args.outputDir + "/relation2vec." + m;
    const std::string entPath = args.outputDir + "/entity2vec." + m;
    const std::string wPath = args.outputDir + "/weights." + m;
    if (!fileExists(relPath)) {
        printf("Could not find relation embedding file: %s. Make sure to specify the path and/or train.\n", relPath.c_str());
        exit(2);
    }
    if (!fileExists(entPath)) {
        printf("Could not find entity embedding file: %s. Make sure to specify the path and/or train.\n", entPath.c_str());
        exit(2);
    }
    std::map<std::string, int>& entity2id = L.entity2id;
    std::map<std::string, int>& relation2id = L.relation2id;
    loadIdFile(args.dataDir + "/entity2id.txt", entity2id);
    loadIdFile(args.dataDir + "/relation2id.txt", relation2id);
    const int ne = (int)entity2id.size(), nr = (int)relation2id.size(), n = args.embeddingSize;
    std::vector<int>&th = L.th, &tt = L.tt, &tr = L.tr, &fh = L.fh, &ft = L.ft, &fr = L.fr;
    auto addFilter = [&](int h, int t, int r) { fh.push_back(h); ft.push_back(t); fr.push_back(r); };
    loadTripleFile(args.dataDir + "/test.txt", entity2id, relation2id, [&](int h, int t, int r) {
        th.push_back(h); tt.push_back(t); tr.push_back(r); addFilter(h, t, r); });
    loadTripleFile(args.dataDir + "/train.txt", entity2id, relation2id, addFilter);
    loadTripleFile(args.dataDir + "/valid.txt", entity2id, relation2id, addFilter);
    if ((model != KB2E_TRANSE) && !fileExists(wPath)) {
        printf("Could not find weight embedding file: %s. Make sure to specify the path and/or train.\n", wPath.c_str());
        exit(2);
    }
    kb2e_config cfg;
    kb2e_default_config(&cfg);
    cfg.model = model;
    cfg.dim = n;
    cfg.num_entities = ne;
    cfg.num_relations = nr;
    cfg.method = args.method;
    cfg.distance = args.distanceType;
    cfg.precision = 64;
    cfg.device = args.device;
    kb2e_ctx*& ctx = L.ctx;
    check(nullptr, kb2e_create(&cfg, &ctx), "create");
    // the embedding files parsed on the device (EmbeddingEvaluation::loadEmbeddings)
    if (kb2e_read_table(ctx, 1, relPath.c_str(), KB2E_READ_VERBATIM) != KB2E_OK) {
        printf("Failed to read embedding values from file: '%s'\n", relPath.c_str());
        exit(1);
    }
    if (kb2e_read_table(ctx, 0, entPath.c_str(), KB2E_READ_VERBATIM) != KB2E_OK) {
        printf("Failed to read embedding values from file: '%s'\n", entPath.c_str());
        exit(1);
    }
    {
        std::vector<double> E((size_t)ne * n);
        check(ctx, kb2e_download_params(ctx, E.data(), nullptr, nullptr), "download_params");
        for (int i = 0; i < ne; i++) {  // common/evaluation.cpp:99-102
            const double len = vec_len(&E[(size_t)i * n], n);
            if (len - 1 > 1e-3) std::cout << "wrong_entity" << i << ' ' << len << std::endl;
        }
    }
    if (model != KB2E_TRANSE && kb2e_read_table(ctx, 2, wPath.c_str(), KB2E_READ_VERBATIM) != KB2E_OK) {
        printf("Failed to read embedding weight values from seed file: '%s'\n", wPath.c_str());
        exit(1);
    }
}

// EmbeddingEvaluation::prepare + run (common/evaluation.cpp:181-266) with the
// ranking on the GPU (kb2e_evaluate; TransR with --transrcompat 1, the default:
// kb2e_evaluate_transr_compat, the reference's stateful energy).
int eval_main(int argc, char** argv, kb2e_model model) {
    EmbeddingArguments args = parseArgs(argc, argv);
    printf("%s\n", args.to_string().c_str());
    LoadedModel L;
    load_model(args, model, L);
    kb2e_ctx* ctx = L.ctx;
    std::vector<int>&th = L.th, &tt = L.tt, &tr = L.tr, &fh = L.fh, &ft = L.ft, &fr = L.fr;
    double out[5];
    if (model == KB2E_TRANSR && args.transrCompat) {
        // the reference's evalTransR: energy work vectors accumulate over the
        // whole run (transr/transr.cpp:20-25); progress per relation (:240)
        auto progress = [](double f, void*) {
            printf("\rProcessed %05.2f%% ...", f * 100.0);
            fflush(stdout);
        };
        check(ctx, kb2e_evaluate_transr_compat(ctx, th.data(), tt.data(), tr.data(), (int64_t)th.size(), fh.data(),
                                               ft.data(), fr.data(), (int64_t)fh.size(), nullptr, out, progress,
                                               nullptr), "evaluate");
    } else {
        check(ctx, kb2e_evaluate(ctx, th.data(), tt.data(), tr.data(), (int64_t)th.size(), fh.data(), ft.data(),
                                 fr.data(), (int64_t)fh.size(), out), "evaluate");
        printf("\rProcessed %05.2f%% ...", 100.0);
    }
    printf("\n");
    printf("Raw      -- Rank: %f, Hits@10: %f\n", out[0], out[1]);
    printf("Filtered -- Rank: %f, Hits@10: %f\n", out[2], out[3]);
    kb2e_destroy(ctx);
    return 0;
}

// predictTransE|H|R: the reference's flags and files as evalTrans* loads them,
// plus --queries FILE (lines "head<TAB>tail<TAB>relation" in the triple files'
// column order with a literal ? for the unknown head or tail, or for the
// unknown relation: "head<TAB>tail<TAB>?" asks which relation holds), --topk K
// [10] and --filtered 0|1 [1: known triples (train + valid + test) are not
// answers].  One line per answer: query index (its line in FILE, from 0),
// position (from 1), entity (relation) name, energy.  Entity and relation
// queries may be mixed; the answers come out interleaved, in the order of the
// queries' lines.
int predict_main(int argc, char** argv, kb2e_model model) {
    EmbeddingArguments args = parseArgs(argc, argv);
    printf("%s\n", args.to_string().c_str());
    int i, topk = 10, filtered = 1;
    std::string queries;
    if ((i = argpos("queries", true, argc, argv)) != -1) queries = argv[i + 1];
    if ((i = argpos("topk", true, argc, argv)) != -1) topk = atoi(argv[i + 1]);
    if ((i = argpos("filtered", true, argc, argv)) != -1) filtered = atoi(argv[i + 1]);
    if (queries.empty()) {
        printf("Argument missing for queries\n");
        exit(1);
    }
    FILE* f = fopen(queries.c_str(), "r");
    if (!f) {
        printf("Could not open query file: %s\n", queries.c_str());
        exit(2);
    }
    LoadedModel L;
    load_model(args, model, L);
    std::vector<std::string> names(L.entity2id.size());
    for (const auto& kv : L.entity2id)
        if (kv.second >= 0 && (size_t)kv.second < names.size()) names[(size_t)kv.second] = kv.first;
    std::vector<std::string> rnames(L.relation2id.size());
    for (const auto& kv : L.relation2id)
        if (kv.second >= 0 && (size_t)kv.second < rnames.size()) rnames[(size_t)kv.second] = kv.first;
    std::vector<int32_t> qe, qr, qs, qline;  // entity queries
    std::vector<int32_t> rh, rt, rline;      // relation queries
    char hb[512], tb[512], rb[512];
    for (int line = 0; fscanf(f, "%511s\t%511s\t%511s", hb, tb, rb) == 3; ++line) {
        const bool noHead = !strcmp(hb, "?"), noTail = !strcmp(tb, "?"), noRel = !strcmp(rb, "?");
        bool fail = false;
        if (noRel && (noHead || noTail)) {
            std::cout << "Relation query needs both the head and the tail: " << hb << ' ' << tb << std::endl;
            fail = true;
        }
        if (!noRel && noHead == noTail) {
            std::cout << "Query needs exactly one ? in the head or the tail column: " << hb << ' ' << tb << std::endl;
            fail = true;
        }
        if (!noHead && !L.entity2id.count(hb)) {
            std::cout << "Head entity found in triple file that was not found in the identity file: " << hb << std::endl;
            fail = true;
        }
        if (!noTail && !L.entity2id.count(tb)) {
            std::cout << "Tail entity found in triple file that was not found in the identity file: " << tb << std::endl;
            fail = true;
        }
        if (!noRel && !L.relation2id.count(rb)) {
            std::cout << "Relation found in triple file that was not found in the identity file: " << rb << std::endl;
            fail = true;
        }
        if (fail) continue;
        if (noRel) {
            rh.push_back(L.entity2id[hb]);
            rt.push_back(L.entity2id[tb]);
            rline.push_back(line);
        } else {
            qe.push_back(L.entity2id[noTail ? hb : tb]);
            qr.push_back(L.relation2id[rb]);
            qs.push_back(noTail ? 1 : 0);
            qline.push_back(line);
        }
    }
    fclose(f);
    const size_t nq = qe.size(), nrq = rh.size(), k = (size_t)std::max(topk, 1);
    const int64_t nf = filtered ? (int64_t)L.fh.size() : 0;
    const int32_t *fh = nf ? L.fh.data() : nullptr, *ft = nf ? L.ft.data() : nullptr, *fr = nf ? L.fr.data() : nullptr;
    std::vector<int32_t> ids(nq * k), found(nq), rids(nrq * k), rfound(nrq);
    std::vector<double> energy(nq * k), renergy(nrq * k);
    if (nq)
        check(L.ctx, kb2e_predict(L.ctx, qe.data(), qr.data(), qs.data(), (int64_t)nq, topk, fh, ft, fr, nf, ids.data(),
                                  energy.data(), found.data()), "predict");
    if (nrq)
        check(L.ctx, kb2e_predict_relations(L.ctx, rh.data(), rt.data(), (int64_t)nrq, topk, fh, ft, fr, nf,
                                            rids.data(), renergy.data(), rfound.data()), "predict_relations");
    // both kinds interleaved, in the order of their lines in FILE
    for (size_t q = 0, p = 0; q < nq || p < nrq;) {
        if (p == nrq || (q < nq && qline[q] < rline[p])) {
            for (int j = 0; j < found[q]; ++j)
                printf("%d\t%d\t%s\t%.6lf\n", qline[q], j + 1, names[(size_t)ids[q * k + j]].c_str(), energy[q * k + j]);
            ++q;
        } else {
            for (int j = 0; j < rfound[p]; ++j)
                printf("%d\t%d\t%s\t%.6lf\n", rline[p], j + 1, rnames[(size_t)rids[p * k + j]].c_str(),
                       renergy[p * k + j]);
            ++p;
        }
    }
    kb2e_destroy(L.ctx);
    return 0;
}

// jointTransE|H|R: conjunctive queries (kb2e_predict_joint) on the tables
// predictTrans* loads, with its flags: --queries FILE, --topk K [10], --filtered
// 0|1 [1: an entity known (train + valid + test) for every pattern of a query is
// no answer].  A line of FILE is "query<TAB>head<TAB>tail<TAB>relation" with a
// literal ? for exactly one of head and tail; consecutive lines with the same
// first token are the patterns of one query, in that order (a token that comes
// back later starts a new query).  A line with an unknown name is reported as
// predictTrans* reports it, and the whole query that holds it is dropped.  One
// line per answer: query token, position (from 1), entity name, joint energy.
int joint_main(int argc, char** argv, kb2e_model model) {
    EmbeddingArguments args = parseArgs(argc, argv);
    printf("%s\n", args.to_string().c_str());
    int i, topk = 10, filtered = 1;
    std::string queries;
    if ((i = argpos("queries", true, argc, argv)) != -1) queries = argv[i + 1];
    if ((i = argpos("topk", true, argc, argv)) != -1) topk = atoi(argv[i + 1]);
    if ((i = argpos("filtered", true, argc, argv)) != -1) filtered = atoi(argv[i + 1]);
    if (queries.empty()) {
        printf("Argument missing for queries\n");
        exit(1);
    }
    FILE* f = fopen(queries.c_str(), "r");
    if (!f) {
        printf("Could not open query file: %s\n", queries.c_str());
        exit(2);
    }
    LoadedModel L;
    load_model(args, model, L);
    std::vector<std::string> names(L.entity2id.size());
    for (const auto& kv : L.entity2id)
        if (kv.second >= 0 && (size_t)kv.second < names.size()) names[(size_t)kv.second] = kv.first;
    std::vector<std::string> tokens;  // of the queries kept
    std::vector<int64_t> offsets(1, 0);
    std::vector<int32_t> qe, qr, qs;
    std::string cur;
    bool open = false, bad = false;
    auto close_query = [&] {
        if (!open) return;
        const size_t m = qe.size() - (size_t)offsets.back();
        if (!bad && m > (size_t)KB2E_JOINT_MAX_CONSTRAINTS) {
            std::cout << "Query has more than " << (int)KB2E_JOINT_MAX_CONSTRAINTS << " patterns: " << cur << std::endl;
            bad = true;
        }
        if (bad || m == 0) {  // dropped whole
            qe.resize((size_t)offsets.back());
            qr.resize((size_t)offsets.back());
            qs.resize((size_t)offsets.back());
        } else {
            offsets.push_back((int64_t)qe.size());
            tokens.push_back(cur);
        }
        open = bad = false;
    };
    char qb[512], hb[512], tb[512], rb[512];
    while (fscanf(f, "%511s\t%511s\t%511s\t%511s", qb, hb, tb, rb) == 4) {
        if (!open || cur != qb) {
            close_query();
            cur = qb;
            open = true;
        }
        const bool noHead = !strcmp(hb, "?"), noTail = !strcmp(tb, "?");
        bool fail = false;
        if (noHead == noTail) {
            std::cout << "Query needs exactly one ? in the head or the tail column: " << hb << ' ' << tb << std::endl;
            fail = true;
        }
        if (!noHead && !L.entity2id.count(hb)) {
            std::cout << "Head entity found in triple file that was not found in the identity file: " << hb << std::endl;
            fail = true;
        }
        if (!noTail && !L.entity2id.count(tb)) {
            std::cout << "Tail entity found in triple file that was not found in the identity file: " << tb << std::endl;
            fail = true;
        }
        if (!L.relation2id.count(rb)) {
            std::cout << "Relation found in triple file that was not found in the identity file: " << rb << std::endl;
            fail = true;
        }
        if (fail) {
            bad = true;
            continue;
        }
        qe.push_back(L.entity2id[noTail ? hb : tb]);
        qr.push_back(L.relation2id[rb]);
        qs.push_back(noTail ? 1 : 0);
    }
    close_query();
    fclose(f);
    const size_t nq = tokens.size(), k = (size_t)std::max(topk, 1);
    if (nq == 0) {
        printf("No queries to answer\n");
        kb2e_destroy(L.ctx);
        return 0;
    }
    const int64_t nf = filtered ? (int64_t)L.fh.size() : 0;
    const int32_t *fh = nf ? L.fh.data() : nullptr, *ft = nf ? L.ft.data() : nullptr, *fr = nf ? L.fr.data() : nullptr;
    std::vector<int32_t> ids(nq * k), found(nq);
    std::vector<double> energy(nq * k);
    check(L.ctx, kb2e_predict_joint(L.ctx, offsets.data(), qe.data(), qr.data(), qs.data(), (int64_t)nq, topk, fh, ft, fr,
                                    nf, ids.data(), energy.data(), found.data()), "predict_joint");
    for (size_t q = 0; q < nq; ++q)
        for (int j = 0; j < found[q]; ++j)
            printf("%s\t%d\t%s\t%.6lf\n", tokens[q].c_str(), j + 1, names[(size_t)ids[q * k + j]].c_str(),
                   energy[q * k + j]);
    kb2e_destroy(L.ctx);
    return 0;
}

// pathTransE|H|R: path queries (kb2e_predict_path) on the tables predictTrans*
// loads: --queries FILE, --topk K [10], --beam B [64; 0: every entity, the exact
// minimum], --noloops [a hop may not stay on its entity], --filtered 0|1 [1: an
// answer that train + valid + test triples themselves reach along the path is
// no answer].  A line of FILE is "anchor<TAB>relation[<TAB>relation...]", 1..8
// relations; a relation token with a leading ^ is walked backwards (from its
// tail to its head).  A line with an unknown name or too many hops is reported
// and dropped.  One line per answer: the query's line number in FILE (from 1),
// position (from 1), entity name, path energy, and the intermediate entities of
// the winning path joined by commas (empty for one hop).
int path_main(int argc, char** argv, kb2e_model model) {
    EmbeddingArguments args = parseArgs(argc, argv);
    printf("%s\n", args.to_string().c_str());
    int i, topk = 10, filtered = 1, beam = 64;
    const int noloops = argpos("noloops", false, argc, argv) != -1 ? 1 : 0;
    std::string queries;
    if ((i = argpos("queries", true, argc, argv)) != -1) queries = argv[i + 1];
    if ((i = argpos("topk", true, argc, argv)) != -1) topk = atoi(argv[i + 1]);
    if ((i = argpos("beam", true, argc, argv)) != -1) beam = atoi(argv[i + 1]);
    if ((i = argpos("filtered", true, argc, argv)) != -1) filtered = atoi(argv[i + 1]);
    if (queries.empty()) {
        printf("Argument missing for queries\n");
        exit(1);
    }
    std::ifstream f(queries);
    if (!f) {
        printf("Could not open query file: %s\n", queries.c_str());
        exit(2);
    }
    LoadedModel L;
    load_model(args, model, L);
    std::vector<std::string> names(L.entity2id.size());
    for (const auto& kv : L.entity2id)
        if (kv.second >= 0 && (size_t)kv.second < names.size()) names[(size_t)kv.second] = kv.first;
    std::vector<int> lineno;  // of the queries kept
    std::vector<int32_t> anchors, qr, qs;
    std::vector<int64_t> offsets(1, 0);
    std::string line;
    for (int ln = 1; std::getline(f, line); ++ln) {
        std::vector<std::string> tok;
        std::istringstream is(line);
        for (std::string w; is >> w;) tok.push_back(w);
        if (tok.empty()) continue;
        bool fail = false;
        if (!L.entity2id.count(tok[0])) {
            std::cout << "Head entity found in triple file that was not found in the identity file: " << tok[0] << std::endl;
            fail = true;
        }
        if (tok.size() < 2 || tok.size() - 1 > (size_t)KB2E_PATH_MAX_HOPS) {
            std::cout << "Query needs 1 to " << (int)KB2E_PATH_MAX_HOPS << " relations: " << tok[0] << std::endl;
            fail = true;
        }
        for (size_t x = 1; x < tok.size() && !fail; ++x) {
            const bool back = tok[x][0] == '^';
            const std::string rn = back ? tok[x].substr(1) : tok[x];
            if (!L.relation2id.count(rn)) {
                std::cout << "Relation found in triple file that was not found in the identity file: " << rn << std::endl;
                fail = true;
                break;
            }
            qr.push_back(L.relation2id[rn]);
            qs.push_back(back ? 0 : 1);
        }
        if (fail) {  // dropped whole
            qr.resize((size_t)offsets.back());
            qs.resize((size_t)offsets.back());
            continue;
        }
        anchors.push_back(L.entity2id[tok[0]]);
        offsets.push_back((int64_t)qr.size());
        lineno.push_back(ln);
    }
    const size_t nq = anchors.size(), k = (size_t)std::max(topk, 1);
    if (nq == 0) {
        printf("No queries to answer\n");
        kb2e_destroy(L.ctx);
        return 0;
    }
    const int64_t nf = filtered ? (int64_t)L.fh.size() : 0;
    const int32_t *fh = nf ? L.fh.data() : nullptr, *ft = nf ? L.ft.data() : nullptr, *fr = nf ? L.fr.data() : nullptr;
    const size_t W = (size_t)KB2E_PATH_MAX_HOPS - 1;
    std::vector<int32_t> ids(nq * k), found(nq), via(nq * k * W);
    std::vector<double> energy(nq * k);
    check(L.ctx, kb2e_predict_path(L.ctx, anchors.data(), offsets.data(), qr.data(), qs.data(), (int64_t)nq, topk, beam,
                                   noloops, fh, ft, fr, nf, ids.data(), energy.data(), found.data(), via.data()),
          "predict_path");
    for (size_t q = 0; q < nq; ++q)
        for (int j = 0; j < found[q]; ++j) {
            std::string w;
            for (size_t x = 0; x < W && via[(q * k + (size_t)j) * W + x] >= 0; ++x)
                w += (x ? "," : "") + names[(size_t)via[(q * k + (size_t)j) * W + x]];
            printf("%d\t%d\t%s\t%.6lf\t%s\n", lineno[q], j + 1, names[(size_t)ids[q * k + (size_t)j]].c_str(),
                   energy[q * k + (size_t)j], w.c_str());
        }
    kb2e_destroy(L.ctx);
    return 0;
}

// classifyTransE|H|R: triple classification (Socher et al. 2013; TransH 4.3,
// TransR 4.3) of the tables evalTrans* loads.  Per-relation thresholds are
// fitted on the valid split and applied to the test split.  A split is either
// a labelled file (--validlabels / --testlabels: "head<TAB>tail<TAB>relation
// <TAB>label", 1 positive, -1 or 0 negative) or the split's triples followed by
// one generated negative each (kb2e_corrupt_triples with known = test + train +
// valid, a coin per triple, --constrained [1], seed --negseed [0] for valid and
// seed + 1 for test; negatives that could not be drawn are dropped).  One line
// per relation with test triples: relation, threshold, valid accuracy ("nan"
// without a valid triple: the global threshold is used), test count, test
// accuracy; then the overall test accuracy.  --out FILE: predicted label and
// energy of every classified test triple, in the order of the list (the test
// triples, then their generated negatives).
struct LabelledList {
    std::vector<int32_t> h, t, r;
    std::vector<uint8_t> label;
    void add(int hh, int tt, int rr, int ll) {
        h.push_back(hh);
        t.push_back(tt);
        r.push_back(rr);
        label.push_back((uint8_t)ll);
    }
};

int classify_main(int argc, char** argv, kb2e_model model) {
    EmbeddingArguments args = parseArgs(argc, argv);
    printf("%s\n", args.to_string().c_str());
    int i, constrained = 1;
    unsigned long long negseed = 0;
    std::string labelFile[2], outPath;
    if ((i = argpos("negseed", true, argc, argv)) != -1) negseed = strtoull(argv[i + 1], nullptr, 10);
    if ((i = argpos("constrained", true, argc, argv)) != -1) constrained = atoi(argv[i + 1]) ? 1 : 0;
    if ((i = argpos("validlabels", true, argc, argv)) != -1) labelFile[0] = argv[i + 1];
    if ((i = argpos("testlabels", true, argc, argv)) != -1) labelFile[1] = argv[i + 1];
    if ((i = argpos("out", true, argc, argv)) != -1) outPath = argv[i + 1];
    LoadedModel L;
    load_model(args, model, L);
    kb2e_ctx* ctx = L.ctx;
    const int nr = (int)L.relation2id.size();
    std::vector<std::string> rnames((size_t)nr);
    for (const auto& kv : L.relation2id)
        if (kv.second >= 0 && kv.second < nr) rnames[(size_t)kv.second] = kv.first;

    LabelledList split[2];  // valid, test
    for (int s = 0; s < 2; ++s) {
        LabelledList& S = split[s];
        if (!labelFile[s].empty()) {
            if (!kb2e::load_labelled_file(labelFile[s], L.entity2id, L.relation2id,
                                          [&](int h, int t, int r, int l) { S.add(h, t, r, l); })) {
                printf("Could not open labelled triple file: %s\n", labelFile[s].c_str());
                exit(2);
            }
        } else {
            if (s == 0)
                loadTripleFile(args.dataDir + "/valid.txt", L.entity2id, L.relation2id,
                               [&](int h, int t, int r) { S.add(h, t, r, 1); });
            else
                for (size_t k = 0; k < L.th.size(); ++k) S.add(L.th[k], L.tt[k], L.tr[k], 1);
            const size_t np = S.h.size();
            if (np) {
                std::vector<int32_t> nh(np), nt(np);
                int64_t failed = 0;
                check(ctx, kb2e_corrupt_triples(ctx, S.h.data(), S.t.data(), S.r.data(), (int64_t)np, L.fh.data(),
                                                L.ft.data(), L.fr.data(), (int64_t)L.fh.size(), negseed + (unsigned)s, 2,
                                                constrained, nh.data(), nt.data(), &failed), "corrupt_triples");
                if (failed)
                    printf("%lld %s negatives could not be drawn and are left out\n", (long long)failed,
                           s == 0 ? "valid" : "test");
                for (size_t k = 0; k < np; ++k)
                    if (nh[k] >= 0) S.add(nh[k], nt[k], S.r[k], 0);
            }
        }
        if (S.h.empty()) {
            printf("No %s triples to classify\n", s == 0 ? "valid" : "test");
            exit(1);
        }
    }
    std::vector<double> thr((size_t)nr);
    std::vector<int64_t> counts((size_t)nr * 3);
    double gthr = 0;
    int64_t gcorrect = 0;
    check(ctx, kb2e_fit_thresholds(ctx, split[0].h.data(), split[0].t.data(), split[0].r.data(), split[0].label.data(),
                                   (int64_t)split[0].h.size(), thr.data(), counts.data(), &gthr, &gcorrect),
          "fit_thresholds");
    const LabelledList& T = split[1];
    std::vector<uint8_t> predicted(T.h.size());
    std::vector<double> energy(T.h.size());
    check(ctx, kb2e_classify_triples(ctx, T.h.data(), T.t.data(), T.r.data(), (int64_t)T.h.size(), thr.data(),
                                     predicted.data(), energy.data()), "classify_triples");
    std::vector<int64_t> n((size_t)nr, 0), ok((size_t)nr, 0);
    int64_t total_ok = 0;
    for (size_t k = 0; k < T.h.size(); ++k) {
        ++n[(size_t)T.r[k]];
        if (predicted[k] == T.label[k]) {
            ++ok[(size_t)T.r[k]];
            ++total_ok;
        }
    }
    for (int r = 0; r < nr; ++r) {
        if (!n[(size_t)r]) continue;
        const int64_t nv = counts[(size_t)r * 3] + counts[(size_t)r * 3 + 1];
        printf("%s\t%.6lf\t", rnames[(size_t)r].c_str(), thr[(size_t)r]);
        if (nv) printf("%.6lf", (double)counts[(size_t)r * 3 + 2] / (double)nv);
        else printf("nan");
        printf("\t%lld\t%.6lf\n", (long long)n[(size_t)r], (double)ok[(size_t)r] / (double)n[(size_t)r]);
    }
    printf("accuracy: %.6lf (%lld triples)\n", (double)total_ok / (double)T.h.size(), (long long)T.h.size());
    if (!outPath.empty()) {
        FILE* f = fopen(outPath.c_str(), "w");
        if (!f) {
            printf("Could not open output file: %s\n", outPath.c_str());
            exit(1);
        }
        for (size_t k = 0; k < T.h.size(); ++k) fprintf(f, "%d\t%.6lf\n", (int)predicted[k], energy[k]);
        fclose(f);
    }
    kb2e_destroy(ctx);
    return 0;
}

// completeTransE|H|R: knowledge-base completion of the tables evalTrans* loads
// (kb2e_complete_triples): per relation the --topk K [10] most plausible
// triples that are not known.  --relations FILE names the relations, one per
// line (unknown names are reported and skipped, in the loader's wording);
// without it every relation is mined.  --constrained 0|1 [1: heads and tails
// from the entities seen in that slot of the relation among the known triples],
// --loops 0|1 [0: head == tail is no answer], --filtered 0|1 [1: known = train +
// valid + test; 0: train + valid, so that test triples can be found].  One line
// per answer: relation name, position (from 1), head name, tail name, energy.
int complete_main(int argc, char** argv, kb2e_model model) {
    EmbeddingArguments args = parseArgs(argc, argv);
    printf("%s\n", args.to_string().c_str());
    int i, topk = 10, constrained = 1, loops = 0, filtered = 1;
    std::string relFile;
    if ((i = argpos("relations", true, argc, argv)) != -1) relFile = argv[i + 1];
    if ((i = argpos("topk", true, argc, argv)) != -1) topk = atoi(argv[i + 1]);
    if ((i = argpos("constrained", true, argc, argv)) != -1) constrained = atoi(argv[i + 1]) ? 1 : 0;
    if ((i = argpos("loops", true, argc, argv)) != -1) loops = atoi(argv[i + 1]) ? 1 : 0;
    if ((i = argpos("filtered", true, argc, argv)) != -1) filtered = atoi(argv[i + 1]);
    FILE* f = nullptr;
    if (!relFile.empty() && !(f = fopen(relFile.c_str(), "r"))) {
        printf("Could not open relation file: %s\n", relFile.c_str());
        exit(2);
    }
    LoadedModel L;
    load_model(args, model, L);
    const int nr = (int)L.relation2id.size();
    std::vector<std::string> names(L.entity2id.size()), rnames((size_t)nr);
    for (const auto& kv : L.entity2id)
        if (kv.second >= 0 && (size_t)kv.second < names.size()) names[(size_t)kv.second] = kv.first;
    for (const auto& kv : L.relation2id)
        if (kv.second >= 0 && kv.second < nr) rnames[(size_t)kv.second] = kv.first;
    std::vector<int32_t> rels;
    if (f) {
        char rb[512];
        while (fscanf(f, "%511s", rb) == 1) {
            if (!L.relation2id.count(rb)) {
                std::cout << "Relation found in triple file that was not found in the identity file: " << rb << std::endl;
                continue;
            }
            rels.push_back(L.relation2id[rb]);
        }
        fclose(f);
    } else {
        for (int r = 0; r < nr; ++r) rels.push_back(r);
    }
    if (rels.empty()) {
        printf("No relations to complete\n");
        exit(1);
    }
    // load_model lists the test triples first: without them the rest is train + valid
    const size_t skip = filtered ? 0 : L.th.size();
    const int64_t nknown = (int64_t)(L.fh.size() - skip);
    const int32_t *kh = nknown ? L.fh.data() + skip : nullptr, *kt = nknown ? L.ft.data() + skip : nullptr,
                  *kr = nknown ? L.fr.data() + skip : nullptr;
    const size_t nq = rels.size(), k = (size_t)std::max(topk, 1);
    std::vector<int32_t> heads(nq * k), tails(nq * k);
    std::vector<double> energy(nq * k);
    std::vector<int64_t> found(nq);
    check(L.ctx, kb2e_complete_triples(L.ctx, rels.data(), (int64_t)nq, topk, kh, kt, kr, nknown, constrained,
                                       loops ? 0 : 1, heads.data(), tails.data(), energy.data(), found.data()),
          "complete_triples");
    for (size_t q = 0; q < nq; ++q)
        for (int64_t j = 0; j < found[q]; ++j)
            printf("%s\t%lld\t%s\t%s\t%.6lf\n", rnames[(size_t)rels[q]].c_str(), (long long)(j + 1),
                   names[(size_t)heads[q * k + j]].c_str(), names[(size_t)tails[q * k + j]].c_str(), energy[q * k + j]);
    kb2e_destroy(L.ctx);
    return 0;
}

// neighborsTransE|H|R: entity neighbours (kb2e_neighbors) on the tables
// evalTrans* loads.  --entities FILE names the query entities, one per line
// (unknown names are reported and skipped, in the loader's wording), --all asks
// for every entity: the kNN graph.  --topk K [10], --relation NAME: relation
// NAME's projected space instead of the entity space, --self: the entity itself
// is a candidate.  One line per answer: entity name, position (from 1),
// neighbour name, distance.  --pairs: the mutual pairs of the lists instead, one
// line each: the two names and the distance, ascending.
int neighbors_main(int argc, char** argv, kb2e_model model) {
    EmbeddingArguments args = parseArgs(argc, argv);
    printf("%s\n", args.to_string().c_str());
    int i, topk = 10, relation = -1;
    std::string entFile, relName;
    if ((i = argpos("entities", true, argc, argv)) != -1) entFile = argv[i + 1];
    if ((i = argpos("topk", true, argc, argv)) != -1) topk = atoi(argv[i + 1]);
    if ((i = argpos("relation", true, argc, argv)) != -1) relName = argv[i + 1];
    const bool all = argpos("all", false, argc, argv) != -1;
    const int self = argpos("self", false, argc, argv) != -1 ? 1 : 0;
    const bool pairs = argpos("pairs", false, argc, argv) != -1;
    if (all == !entFile.empty()) {
        printf("Give either --entities FILE or --all\n");
        exit(1);
    }
    FILE* f = nullptr;
    if (!all && !(f = fopen(entFile.c_str(), "r"))) {
        printf("Could not open entity file: %s\n", entFile.c_str());
        exit(2);
    }
    LoadedModel L;
    load_model(args, model, L);
    std::vector<std::string> names(L.entity2id.size());
    for (const auto& kv : L.entity2id)
        if (kv.second >= 0 && (size_t)kv.second < names.size()) names[(size_t)kv.second] = kv.first;
    if (!relName.empty()) {
        if (!L.relation2id.count(relName)) {
            std::cout << "Relation found in triple file that was not found in the identity file: " << relName << std::endl;
            exit(1);
        }
        relation = L.relation2id[relName];
    }
    std::vector<int32_t> ents;
    if (f) {
        char eb[512];
        while (fscanf(f, "%511s", eb) == 1) {
            if (!L.entity2id.count(eb)) {
                std::cout << "Entity found in triple file that was not found in the identity file: " << eb << std::endl;
                continue;
            }
            ents.push_back(L.entity2id[eb]);
        }
        fclose(f);
    } else {
        for (size_t e = 0; e < names.size(); ++e) ents.push_back((int32_t)e);
    }
    if (ents.empty()) {
        printf("No entities to find neighbours of\n");
        exit(1);
    }
    const size_t nq = ents.size(), k = (size_t)std::max(topk, 1);
    std::vector<int32_t> ids(nq * k), found(nq);
    std::vector<double> dist(nq * k);
    check(L.ctx, kb2e_neighbors(L.ctx, ents.data(), (int64_t)nq, relation, topk, self, ids.data(), dist.data(), found.data()),
          "neighbors");
    if (pairs) {
        for (const kb2e::MutualPair& p : kb2e::mutual_pairs(ents.data(), (int64_t)nq, (int32_t)k, ids.data(), dist.data(), found.data()))
            printf("%s\t%s\t%.6lf\n", names[(size_t)p.a].c_str(), names[(size_t)p.b].c_str(), p.dist);
    } else {
        for (size_t q = 0; q < nq; ++q)
            for (int32_t j = 0; j < found[q]; ++j)
                printf("%s\t%d\t%s\t%.6lf\n", names[(size_t)ents[q]].c_str(), j + 1, names[(size_t)ids[q * k + j]].c_str(),
                       dist[q * k + j]);
    }
    kb2e_destroy(L.ctx);
    return 0;
}

// candidatesTransE|H|R: candidate lists (kb2e_score_candidates,
// kb2e_rank_candidates) on the tables evalTrans* loads.  --queries FILE: lines
// "head<TAB>tail<TAB>relation<TAB>cand,cand,...[<TAB>truth]" with a literal ? in
// the unknown head or tail; unknown names are reported in the loader's wording
// (a listing is skipped, a line with an unknown head, tail, relation or truth is
// dropped).  Per line its listings in ascending (energy, entity id, position in
// the list) order, one line each: line (from 0), position (from 1), entity
// name, energy; where a truth is given also "line<TAB>rank<TAB>raw<TAB>filtered
// <TAB>counted raw<TAB>counted filtered", the filter being train + valid + test
// as in predictTrans*.  --typed takes no query file: every test triple is ranked
// on both sides against the entities seen in that slot of its relation in train
// + valid + test (one shared list per relation and slot), and the metrics are
// printed beside those against all entities (kb2e_rank_triples).
void print_rank_metrics(const char* label, const std::vector<int64_t>& ranks, size_t stride, size_t c0, size_t c1) {
    double sum = 0, rr = 0, h1 = 0, h3 = 0, h10 = 0, count = 0;
    for (size_t x = 0; x * stride < ranks.size(); ++x)
        for (size_t c : {c0, c1}) {
            const double r = (double)ranks[x * stride + c];
            sum += r;
            rr += 1.0 / r;
            h1 += r <= 1;
            h3 += r <= 3;
            h10 += r <= 10;
            count += 1;
        }
    printf("%s -- Rank: %f, MRR: %f, Hits@1: %f, Hits@3: %f, Hits@10: %f\n", label, sum / count, rr / count, h1 / count,
           h3 / count, h10 / count);
}

int candidates_main(int argc, char** argv, kb2e_model model) {
    EmbeddingArguments args = parseArgs(argc, argv);
    printf("%s\n", args.to_string().c_str());
    int i;
    std::string queries;
    if ((i = argpos("queries", true, argc, argv)) != -1) queries = argv[i + 1];
    const bool typed = argpos("typed", false, argc, argv) != -1;
    if (typed == !queries.empty()) {
        printf("Give either --queries FILE or --typed\n");
        exit(1);
    }
    std::ifstream in;
    if (!typed) {
        in.open(queries);
        if (!in) {
            printf("Could not open query file: %s\n", queries.c_str());
            exit(2);
        }
    }
    LoadedModel L;
    load_model(args, model, L);
    const int64_t nf = (int64_t)L.fh.size();
    if (typed) {
        const size_t nt = L.th.size();
        const int64_t nr = (int64_t)L.relation2id.size();
        if (nt == 0) {
            printf("No test triples\n");
            exit(1);
        }
        const kb2e::SlotPools sp = kb2e::build_slot_pools(L.fh.data(), L.ft.data(), L.fr.data(), nf, nr);
        // per test triple: the head query (side 0, the heads' pool), then the tail query
        std::vector<int32_t> qe(nt * 2), qr(nt * 2), qs(nt * 2), qt(nt * 2), ql(nt * 2);
        for (size_t k = 0; k < nt; ++k) {
            qe[k * 2] = L.tt[k], qt[k * 2] = L.th[k], qs[k * 2] = 0, ql[k * 2] = L.tr[k] * 2;
            qe[k * 2 + 1] = L.th[k], qt[k * 2 + 1] = L.tt[k], qs[k * 2 + 1] = 1, ql[k * 2 + 1] = L.tr[k] * 2 + 1;
            qr[k * 2] = qr[k * 2 + 1] = L.tr[k];
        }
        std::vector<int64_t> ranks(nt * 4), counted(nt * 4), full(nt * 4);
        check(L.ctx, kb2e_rank_candidates(L.ctx, qe.data(), qr.data(), qs.data(), qt.data(), ql.data(), (int64_t)nt * 2,
                                          sp.off.data(), sp.ids.data(), nr * 2, L.fh.data(), L.ft.data(), L.fr.data(), nf,
                                          ranks.data(), counted.data()), "rank_candidates");
        check(L.ctx, kb2e_rank_triples(L.ctx, L.th.data(), L.tt.data(), L.tr.data(), (int64_t)nt, L.fh.data(), L.ft.data(),
                                       L.fr.data(), nf, full.data()), "rank_triples");
        long long c0 = 0, c1 = 0;
        for (size_t x = 0; x < nt * 2; ++x) c0 += counted[x * 2], c1 += counted[x * 2 + 1];
        print_rank_metrics("Typed raw     ", ranks, 4, 0, 2);
        print_rank_metrics("Typed filtered", ranks, 4, 1, 3);
        printf("Typed counted  -- raw: %lld, filtered: %lld\n", c0, c1);
        print_rank_metrics("Full raw      ", full, 4, 0, 2);
        print_rank_metrics("Full filtered ", full, 4, 1, 3);
        kb2e_destroy(L.ctx);
        return 0;
    }
    std::vector<std::string> names(L.entity2id.size());
    for (const auto& kv : L.entity2id)
        if (kv.second >= 0 && (size_t)kv.second < names.size()) names[(size_t)kv.second] = kv.first;
    std::vector<int32_t> qe, qr, qs, qt, qline, cand;
    std::vector<int64_t> off(1, 0);
    std::string text;
    for (int line = 0; std::getline(in, text); ++line) {
        std::vector<std::string> col;
        size_t b = 0;
        for (size_t e; (e = text.find('\t', b)) != std::string::npos; b = e + 1) col.push_back(text.substr(b, e - b));
        col.push_back(text.substr(b));
        if (!col.empty() && !col.back().empty() && col.back().back() == '\r') col.back().pop_back();
        if (col.size() == 1 && col[0].empty()) continue;
        if (col.size() < 4 || col.size() > 5) {
            std::cout << "Query needs head, tail, relation and candidates: " << text << std::endl;
            continue;
        }
        const bool noHead = col[0] == "?", noTail = col[1] == "?";
        bool fail = false;
        if (noHead == noTail) {
            std::cout << "Query needs exactly one ? in the head or the tail column: " << col[0] << ' ' << col[1] << std::endl;
            fail = true;
        }
        if (!noHead && !L.entity2id.count(col[0])) {
            std::cout << "Head entity found in triple file that was not found in the identity file: " << col[0] << std::endl;
            fail = true;
        }
        if (!noTail && !L.entity2id.count(col[1])) {
            std::cout << "Tail entity found in triple file that was not found in the identity file: " << col[1] << std::endl;
            fail = true;
        }
        if (!L.relation2id.count(col[2])) {
            std::cout << "Relation found in triple file that was not found in the identity file: " << col[2] << std::endl;
            fail = true;
        }
        if (col.size() == 5 && !L.entity2id.count(col[4])) {
            std::cout << "Entity found in triple file that was not found in the identity file: " << col[4] << std::endl;
            fail = true;
        }
        if (fail) continue;
        std::stringstream ss(col[3]);
        for (std::string name; std::getline(ss, name, ',');) {
            if (name.empty()) continue;
            if (!L.entity2id.count(name)) {
                std::cout << "Entity found in triple file that was not found in the identity file: " << name << std::endl;
                continue;
            }
            cand.push_back(L.entity2id[name]);
        }
        off.push_back((int64_t)cand.size());
        qe.push_back(L.entity2id[noTail ? col[0] : col[1]]);
        qr.push_back(L.relation2id[col[2]]);
        qs.push_back(noTail ? 1 : 0);
        qt.push_back(col.size() == 5 ? L.entity2id[col[4]] : -1);
        qline.push_back(line);
    }
    const size_t nq = qe.size();
    if (nq == 0) {
        printf("No queries\n");
        exit(1);
    }
    std::vector<double> energy((size_t)std::max<int64_t>(off[nq], 1));
    check(L.ctx, kb2e_score_candidates(L.ctx, qe.data(), qr.data(), qs.data(), nullptr, (int64_t)nq, off.data(),
                                       cand.data(), (int64_t)nq, energy.data()), "score_candidates");
    // the lines with a truth, ranked in one call against their own lists
    std::vector<int32_t> re, rr, rs, rt, rl;
    std::vector<int64_t> slot(nq, -1);
    for (size_t q = 0; q < nq; ++q)
        if (qt[q] >= 0) {
            slot[q] = (int64_t)re.size();
            re.push_back(qe[q]), rr.push_back(qr[q]), rs.push_back(qs[q]), rt.push_back(qt[q]), rl.push_back((int32_t)q);
        }
    std::vector<int64_t> ranks(re.size() * 2), counted(re.size() * 2);
    if (!re.empty())
        check(L.ctx, kb2e_rank_candidates(L.ctx, re.data(), rr.data(), rs.data(), rt.data(), rl.data(), (int64_t)re.size(),
                                          off.data(), cand.data(), (int64_t)nq, nf ? L.fh.data() : nullptr,
                                          nf ? L.ft.data() : nullptr, nf ? L.fr.data() : nullptr, nf, ranks.data(),
                                          counted.data()), "rank_candidates");
    std::vector<int64_t> order;
    for (size_t q = 0; q < nq; ++q) {
        order.resize((size_t)(off[q + 1] - off[q]));
        for (size_t j = 0; j < order.size(); ++j) order[j] = off[q] + (int64_t)j;
        std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) {
            if (energy[(size_t)a] != energy[(size_t)b]) return energy[(size_t)a] < energy[(size_t)b];
            if (cand[(size_t)a] != cand[(size_t)b]) return cand[(size_t)a] < cand[(size_t)b];
            return a < b;
        });
        for (size_t j = 0; j < order.size(); ++j)
            printf("%d\t%d\t%s\t%.6lf\n", qline[q], (int)j + 1, names[(size_t)cand[(size_t)order[j]]].c_str(),
                   energy[(size_t)order[j]]);
        if (slot[q] >= 0) {
            const size_t s = (size_t)slot[q];
            printf("%d\trank\t%lld\t%lld\t%lld\t%lld\n", qline[q], (long long)ranks[s * 2], (long long)ranks[s * 2 + 1],
                   (long long)counted[s * 2], (long long)counted[s * 2 + 1]);
        }
    }
    kb2e_destroy(L.ctx);
    return 0;
}

// foldinTransE|H|R: rows for entities the model was not trained on
// (kb2e_fold_in_entities).  --datadir D holds entity2id.txt with the old
// entities first and the new ones after them; the tables in --outdir O have rows
// for the old entities only.  --new FILE lists the triples that mention the new
// entities (exactly one new entity each), --foldout DIR receives the full
// entity2vec.<method>: the old entities' lines byte for byte as they are in O,
// then one line per new entity.  A new row starts as kb2e_init_params draws it
// for --seed; known = train + valid + test + FILE.  Pass p is one call with
// seed --seed + p (its negatives differ from pass to pass and its summed loss is
// printed: "Pass: p, Loss: x").
int foldin_main(int argc, char** argv, kb2e_model model) {
    EmbeddingArguments args = parseArgs(argc, argv);
    printf("%s\n", args.to_string().c_str());
    int i, side = 2;
    std::string newFile, foldOut;
    if ((i = argpos("new", true, argc, argv)) != -1) newFile = argv[i + 1];
    if ((i = argpos("foldout", true, argc, argv)) != -1) foldOut = argv[i + 1];
    if ((i = argpos("side", true, argc, argv)) != -1) side = atoi(argv[i + 1]);
    if (newFile.empty() || foldOut.empty()) {
        printf("Argument missing for %s\n", newFile.empty() ? "new" : "foldout");
        exit(1);
    }
    const std::string m = method_name(args.method);
    const std::string relPath = args.outputDir + "/relation2vec." + m, entPath = args.outputDir + "/entity2vec." + m,
                      wPath = args.outputDir + "/weights." + m;
    std::map<std::string, int> entity2id, relation2id;
    loadIdFile(args.dataDir + "/entity2id.txt", entity2id);
    loadIdFile(args.dataDir + "/relation2id.txt", relation2id);
    const int ne = (int)entity2id.size(), nr = (int)relation2id.size(), n = args.embeddingSize;
    // the old entity table: its lines are kept as they are
    std::vector<std::string> lines;
    {
        FILE* f = fopen(entPath.c_str(), "r");
        if (!f) {
            printf("Could not find entity embedding file: %s. Make sure to specify the path and/or train.\n", entPath.c_str());
            exit(2);
        }
        std::string line;
        int ch;
        while ((ch = fgetc(f)) != EOF) {
            line.push_back((char)ch);
            if (ch == '\n') {
                lines.push_back(line);
                line.clear();
            }
        }
        fclose(f);
    }
    const int neOld = (int)lines.size();
    if (neOld < 1 || neOld >= ne) {
        printf("%s has %d rows and entity2id.txt %d entities: no new entity\n", entPath.c_str(), neOld, ne);
        exit(1);
    }
    kb2e_config cfg;
    kb2e_default_config(&cfg);
    cfg.model = model;
    cfg.dim = n;
    cfg.num_entities = ne;
    cfg.num_relations = nr;
    cfg.learning_rate = args.learningRate;
    cfg.margin = args.margin;
    cfg.method = args.method;
    cfg.distance = args.distanceType;
    cfg.seed = args.seed;
    cfg.precision = 64;
    cfg.device = args.device;
    kb2e_ctx* ctx = nullptr;
    check(nullptr, kb2e_create(&cfg, &ctx), "create");
    const size_t wn = model == KB2E_TRANSE ? 0 : model == KB2E_TRANSH ? (size_t)nr * n : (size_t)nr * n * n;
    std::vector<double> E((size_t)ne * n), R((size_t)nr * n), W(wn);
    check(ctx, kb2e_init_params(ctx, E.data(), R.data(), wn ? W.data() : nullptr), "init_params");  // the new rows
    for (int e = 0; e < neOld; ++e) {
        const char* p = lines[(size_t)e].c_str();
        for (int k = 0; k < n; ++k) {
            char* end = nullptr;
            E[(size_t)e * n + k] = strtod(p, &end);
            if (end == p) {
                printf("Failed to read embedding values from file: '%s'\n", entPath.c_str());
                exit(1);
            }
            p = end;
        }
    }
    if (kb2e_read_table(ctx, 1, relPath.c_str(), KB2E_READ_VERBATIM) != KB2E_OK) {
        printf("Failed to read embedding values from file: '%s'\n", relPath.c_str());
        exit(1);
    }
    if (wn && kb2e_read_table(ctx, 2, wPath.c_str(), KB2E_READ_VERBATIM) != KB2E_OK) {
        printf("Failed to read embedding weight values from seed file: '%s'\n", wPath.c_str());
        exit(1);
    }
    check(ctx, kb2e_download_params(ctx, nullptr, R.data(), wn ? W.data() : nullptr), "download_params");
    check(ctx, kb2e_upload_params(ctx, E.data(), R.data(), wn ? W.data() : nullptr), "upload_params");

    std::vector<int32_t> xh, xt, xr, kh, kt, kr;
    auto addKnown = [&](int h, int t, int r) { kh.push_back(h); kt.push_back(t); kr.push_back(r); };
    loadTripleFile(newFile, entity2id, relation2id, [&](int h, int t, int r) {
        xh.push_back(h); xt.push_back(t); xr.push_back(r); addKnown(h, t, r); });
    for (const char* split : {"/train.txt", "/valid.txt", "/test.txt"})
        loadTripleFile(args.dataDir + split, entity2id, relation2id, addKnown);
    std::vector<int32_t> free((size_t)(ne - neOld));
    for (int e = neOld; e < ne; ++e) free[(size_t)(e - neOld)] = e;
    std::vector<double> rows(free.size() * (size_t)n), loss(free.size() * 2);
    std::vector<int64_t> counts(free.size() * 3);
    for (int p = 0; p < args.maxEpochs; ++p) {
        check(ctx, kb2e_fold_in_entities(ctx, free.data(), (int64_t)free.size(), xh.data(), xt.data(), xr.data(),
                                         (int64_t)xh.size(), kh.data(), kt.data(), kr.data(), (int64_t)kh.size(), 1,
                                         (uint64_t)args.seed + (uint64_t)p, side, 0, nullptr, rows.data(), loss.data(),
                                         counts.data()), "fold_in_entities");
        double sum = 0;
        for (size_t f = 0; f < free.size(); ++f) sum += loss[f * 2];
        printf("Pass: %d, Loss: %f\n", p, sum);
        fflush(stdout);
    }
    const std::string outPath = foldOut + "/entity2vec." + m;
    FILE* out = fopen(outPath.c_str(), "w");
    if (!out) {
        printf("Could not open output file: %s\n", outPath.c_str());
        exit(1);
    }
    for (const std::string& line : lines) fwrite(line.data(), 1, line.size(), out);
    for (size_t f = 0; f < free.size(); ++f) {  // common/trainer.cpp:109-127
        for (int k = 0; k < n; ++k) fprintf(out, "%.6lf\t", rows[f * n + k]);
        fprintf(out, "\n");
    }
    fclose(out);
    kb2e_destroy(ctx);
    return 0;
}

// foldrelTransE|H|R: parameters for relations the model was not trained on
// (kb2e_fold_in_relations).  --datadir D holds relation2id.txt with the old
// relations first and the new ones after them; relation2vec.<method> (and, for
// TransH / TransR, weights.<method>) in --outdir O have rows for the old
// relations only.  --new FILE lists the new relations' triples, --foldout DIR
// receives the full relation2vec.<method> (and weights.<method>): the old
// relations' lines byte for byte as they are in O, then the new relations' rows.
// A new row starts as kb2e_init_params draws it for --seed; known = train +
// valid + test + FILE.  Pass p is one call with seed --seed + p and batches of
// --batch [1] samples; its summed loss is printed: "Pass: p, Loss: x".
namespace {
std::vector<std::string> read_lines(const std::string& path, const char* what) {
    std::vector<std::string> lines;
    FILE* f = fopen(path.c_str(), "r");
    if (!f) {
        printf("Could not find %s file: %s. Make sure to specify the path and/or train.\n", what, path.c_str());
        exit(2);
    }
    std::string line;
    int ch;
    while ((ch = fgetc(f)) != EOF) {
        line.push_back((char)ch);
        if (ch == '\n') {
            lines.push_back(line);
            line.clear();
        }
    }
    fclose(f);
    return lines;
}

// n values from each of the first `rows` lines
void parse_rows(const std::vector<std::string>& lines, size_t rows, int n, double* dst, const std::string& path) {
    for (size_t r = 0; r < rows; ++r) {
        const char* p = lines[r].c_str();
        for (int k = 0; k < n; ++k) {
            char* end = nullptr;
            dst[r * n + k] = strtod(p, &end);
            if (end == p) {
                printf("Failed to read embedding values from file: '%s'\n", path.c_str());
                exit(1);
            }
            p = end;
        }
    }
}

void write_rows(const std::string& path, const std::vector<std::string>& lines, const double* rows, size_t count, int n) {
    FILE* out = fopen(path.c_str(), "w");
    if (!out) {
        printf("Could not open output file: %s\n", path.c_str());
        exit(1);
    }
    for (const std::string& line : lines) fwrite(line.data(), 1, line.size(), out);
    for (size_t f = 0; f < count; ++f) {  // common/trainer.cpp:109-127
        for (int k = 0; k < n; ++k) fprintf(out, "%.6lf\t", rows[f * n + k]);
        fprintf(out, "\n");
    }
    fclose(out);
}
}  // namespace

int foldrel_main(int argc, char** argv, kb2e_model model) {
    EmbeddingArguments args = parseArgs(argc, argv);
    printf("%s\n", args.to_string().c_str());
    int i, side = 2;
    long long batch = 1;
    std::string newFile, foldOut;
    if ((i = argpos("new", true, argc, argv)) != -1) newFile = argv[i + 1];
    if ((i = argpos("foldout", true, argc, argv)) != -1) foldOut = argv[i + 1];
    if ((i = argpos("side", true, argc, argv)) != -1) side = atoi(argv[i + 1]);
    if ((i = argpos("batch", true, argc, argv)) != -1) batch = atoll(argv[i + 1]);
    if (newFile.empty() || foldOut.empty()) {
        printf("Argument missing for %s\n", newFile.empty() ? "new" : "foldout");
        exit(1);
    }
    const std::string m = method_name(args.method);
    const std::string relPath = args.outputDir + "/relation2vec." + m, entPath = args.outputDir + "/entity2vec." + m,
                      wPath = args.outputDir + "/weights." + m;
    std::map<std::string, int> entity2id, relation2id;
    loadIdFile(args.dataDir + "/entity2id.txt", entity2id);
    loadIdFile(args.dataDir + "/relation2id.txt", relation2id);
    const int ne = (int)entity2id.size(), nr = (int)relation2id.size(), n = args.embeddingSize;
    // the old tables: their lines are kept as they are
    const std::vector<std::string> rlines = read_lines(relPath, "relation embedding");
    const int nrOld = (int)rlines.size();
    if (nrOld < 1 || nrOld >= nr) {
        printf("%s has %d rows and relation2id.txt %d relations: no new relation\n", relPath.c_str(), nrOld, nr);
        exit(1);
    }
    const size_t wper = model == KB2E_TRANSE ? 0 : model == KB2E_TRANSH ? (size_t)n : (size_t)n * n;  // doubles a relation
    std::vector<std::string> wlines;
    if (wper) {
        wlines = read_lines(wPath, "embedding weight");
        if (wlines.size() != (size_t)nrOld * (wper / n)) {
            printf("%s has %zu rows, not the %zu of %d relations\n", wPath.c_str(), wlines.size(),
                   (size_t)nrOld * (wper / n), nrOld);
            exit(1);
        }
    }
    kb2e_config cfg;
    kb2e_default_config(&cfg);
    cfg.model = model;
    cfg.dim = n;
    cfg.num_entities = ne;
    cfg.num_relations = nr;
    cfg.learning_rate = args.learningRate;
    cfg.margin = args.margin;
    cfg.method = args.method;
    cfg.distance = args.distanceType;
    cfg.seed = args.seed;
    cfg.precision = 64;
    cfg.device = args.device;
    kb2e_ctx* ctx = nullptr;
    check(nullptr, kb2e_create(&cfg, &ctx), "create");
    std::vector<double> E((size_t)ne * n), R((size_t)nr * n), W((size_t)nr * wper);
    check(ctx, kb2e_init_params(ctx, E.data(), R.data(), wper ? W.data() : nullptr), "init_params");  // the new rows
    parse_rows(rlines, (size_t)nrOld, n, R.data(), relPath);
    if (wper) parse_rows(wlines, wlines.size(), n, W.data(), wPath);
    check(ctx, kb2e_upload_params(ctx, E.data(), R.data(), wper ? W.data() : nullptr), "upload_params");
    if (kb2e_read_table(ctx, 0, entPath.c_str(), KB2E_READ_VERBATIM) != KB2E_OK) {
        printf("Failed to read embedding values from file: '%s'\n", entPath.c_str());
        exit(1);
    }

    std::vector<int32_t> xh, xt, xr, kh, kt, kr;
    auto addKnown = [&](int h, int t, int r) { kh.push_back(h); kt.push_back(t); kr.push_back(r); };
    loadTripleFile(newFile, entity2id, relation2id, [&](int h, int t, int r) {
        xh.push_back(h); xt.push_back(t); xr.push_back(r); addKnown(h, t, r); });
    for (const char* split : {"/train.txt", "/valid.txt", "/test.txt"})
        loadTripleFile(args.dataDir + split, entity2id, relation2id, addKnown);
    std::vector<int32_t> free((size_t)(nr - nrOld));
    for (int r = nrOld; r < nr; ++r) free[(size_t)(r - nrOld)] = r;
    std::vector<double> rows(free.size() * (size_t)n), wrows(free.size() * wper), loss(free.size() * 2);
    std::vector<int64_t> counts(free.size() * 3);
    for (int p = 0; p < args.maxEpochs; ++p) {
        check(ctx, kb2e_fold_in_relations(ctx, free.data(), (int64_t)free.size(), xh.data(), xt.data(), xr.data(),
                                          (int64_t)xh.size(), kh.data(), kt.data(), kr.data(), (int64_t)kh.size(), 1,
                                          (int64_t)batch, (uint64_t)args.seed + (uint64_t)p, side, 0, nullptr, nullptr,
                                          rows.data(), wper ? wrows.data() : nullptr, loss.data(), counts.data()),
              "fold_in_relations");
        double sum = 0;
        for (size_t f = 0; f < free.size(); ++f) sum += loss[f * 2];
        printf("Pass: %d, Loss: %f\n", p, sum);
        fflush(stdout);
    }
    write_rows(foldOut + "/relation2vec." + m, rlines, rows.data(), free.size(), n);
    if (wper) write_rows(foldOut + "/weights." + m, wlines, wrows.data(), free.size() * (wper / n), n);
    kb2e_destroy(ctx);
    return 0;
}

}  // namespace kb2e_host

#ifndef KB2E_CLI_NO_MAIN  // (tests/native/host_check.cpp includes this file for its parser and loader)
int main(int argc, char** argv) {
    std::string prog = argv[0];
    size_t slash = prog.find_last_of('/');
    if (slash != std::string::npos) prog = prog.substr(slash + 1);
    using namespace kb2e_host;
    if (prog == "trainTransE") return train_main(argc, argv, KB2E_TRANSE);
    if (prog == "trainTransH") return train_main(argc, argv, KB2E_TRANSH);
    if (prog == "trainTransR") return train_main(argc, argv, KB2E_TRANSR);
    if (prog == "evalTransE") return eval_main(argc, argv, KB2E_TRANSE);
    if (prog == "evalTransH") return eval_main(argc, argv, KB2E_TRANSH);
    if (prog == "evalTransR") return eval_main(argc, argv, KB2E_TRANSR);
    if (prog == "predictTransE") return predict_main(argc, argv, KB2E_TRANSE);
    if (prog == "predictTransH") return predict_main(argc, argv, KB2E_TRANSH);
    if (prog == "predictTransR") return predict_main(argc, argv, KB2E_TRANSR);
    if (prog == "classifyTransE") return classify_main(argc, argv, KB2E_TRANSE);
    if (prog == "classifyTransH") return classify_main(argc, argv, KB2E_TRANSH);
    if (prog == "classifyTransR") return classify_main(argc, argv, KB2E_TRANSR);
    if (prog == "completeTransE") return complete_main(argc, argv, KB2E_TRANSE);
    if (prog == "completeTransH") return complete_main(argc, argv, KB2E_TRANSH);
    if (prog == "completeTransR") return complete_main(argc, argv, KB2E_TRANSR);
    if (prog == "foldinTransE") return foldin_main(argc, argv, KB2E_TRANSE);
    if (prog == "foldinTransH") return foldin_main(argc, argv, KB2E_TRANSH);
    if (prog == "foldinTransR") return foldin_main(argc, argv, KB2E_TRANSR);
    if (prog == "foldrelTransE") return foldrel_main(argc, argv, KB2E_TRANSE);
    if (prog == "foldrelTransH") return foldrel_main(argc, argv, KB2E_TRANSH);
    if (prog == "foldrelTransR") return foldrel_main(argc, argv, KB2E_TRANSR);
    if (prog == "jointTransE") return joint_main(argc, argv, KB2E_TRANSE);
    if (prog == "jointTransH") return joint_main(argc, argv, KB2E_TRANSH);
    if (prog == "jointTransR") return joint_main(argc, argv, KB2E_TRANSR);
    if (prog == "pathTransE") return path_main(argc, argv, KB2E_TRANSE);
    if (prog == "pathTransH") return path_main(argc, argv, KB2E_TRANSH);
    if (prog == "pathTransR") return path_main(argc, argv, KB2E_TRANSR);
    if (prog == "neighborsTransE") return neighbors_main(argc, argv, KB2E_TRANSE);
    if (prog == "neighborsTransH") return neighbors_main(argc, argv, KB2E_TRANSH);
    if (prog == "neighborsTransR") return neighbors_main(argc, argv, KB2E_TRANSR);
    if (prog == "candidatesTransE") return candidates_main(argc, argv, KB2E_TRANSE);
    if (prog == "candidatesTransH") return candidates_main(argc, argv, KB2E_TRANSH);
    if (prog == "candidatesTransR") return candidates_main(argc, argv, KB2E_TRANSR);
    fprintf(stderr,
            "invoke as trainTransE|H|R, evalTransE|H|R, predictTransE|H|R, classifyTransE|H|R, completeTransE|H|R, "
            "foldinTransE|H|R, foldrelTransE|H|R, jointTransE|H|R, pathTransE|H|R, neighborsTransE|H|R or candidatesTransE|H|R (got %s)\n",
            prog.c_str());
    return 2;
}
#endif
