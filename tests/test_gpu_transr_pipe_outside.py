"""The pipelined transRNorm chain (kernels_transr_pipe.hpp) outside its violator
loop: the prologue, a window's set-up, the chunk hand-over, the tail.

KB2E_RPAR_PIPE_OPT switches the steps of these parts (a bit each, default all on;
0: the path before them).  They move loads and stores and change no sum, so every
case trains the same batches twice, with KB2E_RPAR_PIPE_OPT=0 and with the
default, and asks for bit-for-bit equal entity, relation and matrix tables, equal
loss and active counts, and an epoch that returns (a bounded in-workgroup wait
that times out sets the kernel's err flag, and the engine then raises).  The
default run is also held against the CPU model (oracle/parallel.py,
cons="chunk1") at the bar of tests/test_gpu_transr_walk.py: the same active
count, loss within 1e-9 relative, tables within 1e-9.

One to three PARALLEL TransR FP64 batches a case, on hub sets built as in
tests/test_gpu_transr_walk.py.  What a case is there for is asserted from the
model's own record of its constraint calls (_Record): per call and relation the
pairs in the kernel's order, which of them fired, where the last update's tail
starts, whether (entity'[r], r) is a pair of its own.  The kernel cuts a
relation's head pairs into chunks of 32 and walks the tail as a chunk of its own.
"""
import numpy as np
import pytest

import oracle.parallel as par
from gpu_common import max_abs
from kb2e_amd import data
from kb2e_amd.engine import Engine
from oracle import orc

pytestmark = pytest.mark.gpu

ATOL = 1e-9
RATE = 0.01
ST = 8
SEED = 3
CHUNK = 32  # kChainRows


def _hub_dataset(ne=300, nr=6, count=4000, seed=5):
    """The hub set of tests/test_gpu_transr_walk.py: entity 0 heads about half the triples."""
    rng = np.random.default_rng(seed)
    h = np.where(rng.random(count) < 0.5, 0, rng.integers(1, ne, count))
    t = rng.integers(1, ne, count)
    r = rng.integers(0, nr, count)
    tr = np.unique(np.stack([h, t, r], 1).astype(np.int32), axis=0)
    tr = tr[rng.permutation(len(tr))]
    return data.Dataset(ne, nr, tr, tr[:0], tr[:0])


class _Events(dict):
    """The `stats` dict of transr_constraint, keeping the order of its updates: the model
    adds to "fired" at every violator and to "pairs" after every chunk (one pair at chunk1)."""

    def __init__(self):
        super().__init__()
        self.log = []

    def __setitem__(self, key, value):
        if key == "fired":
            self.log.append("f")
        elif key == "pairs":
            self.log.append("p")
        super().__setitem__(key, value)


class _Record:
    """Per constraint call, per relation with an active sample (the model's order): `fired`
    (a flag a pair, the kernel's order), `n_head` (pairs before the last update's tail),
    `relpair` ((entity'[r], r) is a pair of its own); and `empty`, the call's relations whose
    samples are all inactive (chains without a pair)."""

    def __init__(self, monkeypatch):
        self.events = _Events()
        self.calls = []
        model_constraint = par.transr_constraint

        def recording(ent, W, h, t, nh, nt, r, act, rate, St=None, **kw):
            ne = ent.shape[0]
            rels = []
            for rr in np.unique(r[act]):
                items = par._relation_items(r, rr, act, h, t, nh, nt, True, ne)
                kl = int(np.nonzero((r == rr) & act)[0][-1])
                n_tail = sum(1 for it in items if it[1] == (kl, 1) or it[1] is None)
                rels.append(dict(r=int(rr), n=len(items), n_head=len(items) - n_tail,
                                 relpair=items[-1][1] is None))
            start = len(self.events.log)
            model_constraint(ent, W, h, t, nh, nt, r, act, rate, St, **kw)
            log = self.events.log[start:]
            flags = []  # a flag a pair: "f" precedes the "p" of its pair
            fired = False
            for ev in log:
                if ev == "f":
                    fired = True
                else:
                    flags.append(fired)
                    fired = False
            assert len(flags) == sum(x["n"] for x in rels), (len(flags), rels)
            pos = 0
            for x in rels:
                x["fired"] = flags[pos:pos + x["n"]]
                pos += x["n"]
            self.calls.append(dict(rels=rels, empty=len(np.unique(r)) - len(rels)))

        monkeypatch.setattr(par, "transr_constraint", recording)

    def relations(self):
        return [x for c in self.calls for x in c["rels"]]


def _head_chunks(x):
    """Violators of each of the relation's head chunks."""
    f = x["fired"][:x["n_head"]]
    return [sum(f[c0:c0 + CHUNK]) for c0 in range(0, len(f), CHUNK)]


def _restarts(x):
    """The tail is made afresh after a renorm: a violator before it and a tail to walk."""
    return x["n_head"] < x["n"] and any(x["fired"][:x["n_head"]])


# what each case is there for, from the model's record
def _check_small(rec, B):
    assert any(c["empty"] > 0 for c in rec.calls), "no relation with an empty chain"
    sizes = sorted(x["n"] for x in rec.relations())
    assert sizes[0] <= 4, sizes  # (a sample's h', t', its corrupted entity: a chunk and the tail)
    assert any(sum(x["fired"]) == 0 for x in rec.relations()), "no chain without a violator"


def _check_hub(rec, B):
    big = [x for x in rec.relations() if 2 * CHUNK < x["n_head"] <= 3 * CHUNK]
    assert big, [x["n_head"] for x in rec.relations()]
    per = [_head_chunks(x) for x in big]
    assert any(0 in p for p in per), per           # a chunk without a violator
    assert any(max(p) >= 3 for p in per), per      # a chunk with several


def _check_tail(rec, B):
    assert any(_restarts(x) for x in rec.relations())
    assert any(any(x["fired"][x["n_head"]:]) for x in rec.relations()), "no violator in a tail"


def _check_relpair(rec, B):
    rels = rec.relations()
    assert any(x["relpair"] for x in rels) and any(not x["relpair"] for x in rels), [x["relpair"] for x in rels]
    assert any(x["relpair"] and x["fired"][-1] for x in rels), "(entity'[r], r) never fires"


def _check_windows(rec, B):
    # KB2E_RPAR_CHAIN_LIST=64, KB2E_RPAR_CHAIN_TILES=2: a window holds < 64 pairs of at most two
    # tiles, so the relation takes three windows or more
    assert max(x["n"] for x in rec.relations()) > 2 * 64, [x["n"] for x in rec.relations()]


def _check_records(rec, B):
    # KB2E_RPAR_REC_CAP=4: a record a wave a stage-full
    assert max(sum(x["fired"]) for x in rec.relations()) >= 3 * 4, [sum(x["fired"]) for x in rec.relations()]


def _check_wide(rec, B):
    assert any(len(_head_chunks(x)) >= 2 and sum(x["fired"]) >= 8 for x in rec.relations())


def _check_ragged(rec, B):
    assert B % 2 == 1, B  # the second sub-batch is one sample short of the first
    assert len(rec.calls) == 2 * 2


HUB1 = dict(ne=300, nr=1, count=4000)   # one relation owns every pair
HUB6 = dict(ne=300, nr=6, count=4000)   # the walk test's set
SPARSE = dict(ne=400, nr=200, count=600)

# (id, data set, dim, batches an epoch, batches trained, sub-batches, environment, check)
CASES = [
    ("small_and_empty_n20", SPARSE, 20, 4, 2, 1, {}, _check_small),
    ("hub70_n33", HUB1, 33, 50, 3, 1, {}, _check_hub),
    ("hub70_n50", HUB1, 50, 61, 3, 1, {}, _check_hub),
    ("tail_restart_n50", HUB6, 50, 5, 2, 2, {}, _check_tail),
    ("relpair_n50", HUB6, 50, 5, 2, 2, {}, _check_relpair),
    ("windows_n50", HUB1, 50, 8, 2, 2, {"KB2E_RPAR_CHAIN_LIST": "64", "KB2E_RPAR_CHAIN_TILES": "2"},
     _check_windows),
    ("record_stages_n50", HUB6, 50, 5, 2, 2, {"KB2E_RPAR_REC_CAP": "4"}, _check_records),
    ("widest_n64", HUB6, 64, 5, 1, 2, {}, _check_wide),
    ("ragged_n50", HUB6, 50, 7, 2, 2, {}, _check_ragged),
]


def _model(ds, dim, batches, trained, sub, monkeypatch):
    """The CPU model's tables, loss and active count after `trained` batches, and its record."""
    rec = _Record(monkeypatch)
    m = orc.Model("R", dim, ds.num_entities, ds.num_relations, rate=RATE, distance=0, batches=batches,
                  transr_compat=True)
    m.set_triples(ds.train)
    orc.srand(SEED)
    m.prep_train()
    pe, pr, pw = m.tables()
    init = (pe.copy(), pr.copy(), pw.copy())
    pe = pe / np.linalg.norm(pe, axis=1, keepdims=True)
    B = m.batch_size()
    si, sj, side = m.sample_stream(B * batches)
    lo, ao = par.transr_parallel_batches(pe, pr, pw, ds.train, si, sj, side, B, trained, rate=RATE, l1=True,
                                         compat=True, work=[np.zeros(dim), np.zeros(dim)], St=ST, cons="chunk1",
                                         stats=rec.events, sub=sub)
    return init, (pe, pr, pw), lo, ao, rec, B


def _engine(ds, dim, batches, trained, sub, init):
    eng = Engine("R", dim, ds.num_entities, ds.num_relations, rate=RATE, distance=0, batches=batches, seed=SEED,
                 schedule="parallel", transr_compat=True, sub_batches=sub)
    eng.upload_triples(ds.train)
    e0, r0, w0 = eng.init_params()
    assert all(np.array_equal(a, b) for a, b in zip((e0, r0, w0), init))
    eng.transr_seed(e0, r0)
    eng.train_batches(trained)  # raises if the chain's err flag is set
    loss, act = eng.take_stats()
    tabs = eng.download_params()
    eng.close()
    return tabs, loss, act


@pytest.mark.parametrize("name,shape,dim,batches,trained,sub,env,check", CASES, ids=[c[0] for c in CASES])
def test_pipe_outside_same_bits(name, shape, dim, batches, trained, sub, env, check, monkeypatch):
    ds = _hub_dataset(**shape)
    monkeypatch.setenv("KB2E_RPAR_ST", str(ST))
    monkeypatch.setenv("KB2E_RPAR_MFMA", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    init, want, lo, ao, rec, B = _model(ds, dim, batches, trained, sub, monkeypatch)
    check(rec, B)
    monkeypatch.setenv("KB2E_RPAR_PIPE_OPT", "0")
    tabs0, loss0, act0 = _engine(ds, dim, batches, trained, sub, init)
    monkeypatch.delenv("KB2E_RPAR_PIPE_OPT")
    tabs1, loss1, act1 = _engine(ds, dim, batches, trained, sub, init)
    for which, a, b in zip(("entity", "relation", "matrix"), tabs0, tabs1):
        assert np.array_equal(a, b), (which, max_abs(a, b))
    assert loss0 == loss1 and act0 == act1, (loss0, loss1, act0, act1)
    # the model, at the walk test's bar
    errs = tuple(max_abs(g, m) for g, m in zip(tabs1, want))
    print(f"{name}: active {act1}, max|diff| to the model {errs}")
    assert act1 == ao, (act1, ao)
    assert abs(loss1 - lo) <= 1e-9 * max(1.0, abs(lo)), (loss1, lo)
    assert max(errs) < ATOL, errs
