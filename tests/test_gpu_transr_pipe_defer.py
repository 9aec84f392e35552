"""The pipelined transRNorm chain's deferred records and early publish
(kernels_transr_pipe.hpp, KB2E_RPAR_PIPE_OPT bits 8 and 16).

Bit 8: a relation of KB2E_RPAR_REC_DEFER chunks or more runs no record pass; its
violators' G rows stay in the record tables under the relation's stamp and the entity
pass makes da = -lr W G from them (rpar_record_convert, the same operands in the same
order).  Bit 16: the walker publishes a violator behind its G row, ahead of the later
rows' update.  Neither changes a sum, so every case trains the same batches twice, with
the two bits off (KB2E_RPAR_PIPE_OPT=2, the path before them) and with the default bits
(KB2E_RPAR_REC_DEFER=1, every relation with a pair defers, unless the case sets a
threshold), and asks for bit-for-bit equal entity, relation and matrix tables and equal
loss and active counts.  The default run is also held against the CPU model
(oracle/parallel.py, cons="chunk1") at the bar of tests/test_gpu_transr_pipe_outside.py:
the same active count, loss within 1e-9 relative, tables within 1e-9.

The sets, the engine and model runs are those of tests/test_gpu_transr_pipe_outside.py;
what a case is there for is asserted from the model's own record of its constraint calls
(_Record here also keeps each pair's entity and the loop updates).

Two things the issue's table names cannot occur on these sets, and why:
  - violator slots past kSlist (the chain's LDS copy of the first 2112 slots): a relation
    has at most one pair an entity and (entity'[r], r), so <= 401 pairs here; the windows
    case keeps several windows with every record deferred.
  - an event that adds two records (src and src2 of rpar_entity_events): on this path a
    pair (entity, r) is deduplicated to one slot of the batch, so an update whose head and
    tail are the same entity carries one flagged slot, never two; the loop case asserts
    that such an update's pair fires and is deferred (one record, through `src`).
"""
import numpy as np
import pytest

import oracle.parallel as par
import test_gpu_transr_pipe_outside as base
from gpu_common import max_abs
from kb2e_amd import data
from oracle import orc

pytestmark = pytest.mark.gpu

CHUNK = base.CHUNK
LONG_MIN = 128  # kRParLongMin: entity segments this long take the 1024-thread path
OFF = "2"       # KB2E_RPAR_PIPE_OPT: the hand-over step alone, the path before this change


def _skewed_dataset(ne=300, count=4000, seed=5, p=(0.42, 0.3, 0.16, 0.07, 0.03, 0.02)):
    """The hub set with six relations of very different sizes."""
    rng = np.random.default_rng(seed)
    h = np.where(rng.random(count) < 0.5, 0, rng.integers(1, ne, count))
    t = rng.integers(1, ne, count)
    r = rng.choice(len(p), count, p=p)
    tr = np.unique(np.stack([h, t, r], 1).astype(np.int32), axis=0)
    tr = tr[rng.permutation(len(tr))]
    return data.Dataset(ne, len(p), tr, tr[:0], tr[:0])


class _Record:
    """base._Record, and per relation `ents` (each pair's entity, the kernel's order) and
    `loops` (entities that are head and tail of one active update of the relation); per
    call `hub_events`, the updates that touch entity 0 as head or tail."""

    def __init__(self, monkeypatch):
        self.events = base._Events()
        self.calls = []
        model_constraint = par.transr_constraint

        def recording(ent, W, h, t, nh, nt, r, act, rate, St=None, **kw):
            ne = ent.shape[0]
            rels = []
            for rr in np.unique(r[act]):
                items = par._relation_items(r, rr, act, h, t, nh, nt, True, ne)
                kl = int(np.nonzero((r == rr) & act)[0][-1])
                n_tail = sum(1 for it in items if it[1] == (kl, 1) or it[1] is None)
                sel = np.nonzero((r == rr) & act)[0]
                loops = {int(h[k]) for k in sel if h[k] == t[k]} | {int(nh[k]) for k in sel if nh[k] == nt[k]}
                rels.append(dict(r=int(rr), n=len(items), n_head=len(items) - n_tail, relpair=items[-1][1] is None,
                                 ents=[it[0] for it in items], loops=loops))
            start = len(self.events.log)
            model_constraint(ent, W, h, t, nh, nt, r, act, rate, St, **kw)
            flags, fired = [], False
            for ev in self.events.log[start:]:
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
            hub = int(((h == 0) | (t == 0)).sum() + ((nh == 0) | (nt == 0)).sum())
            self.calls.append(dict(rels=rels, empty=len(np.unique(r)) - len(rels), hub_events=hub))

        monkeypatch.setattr(par, "transr_constraint", recording)

    def relations(self):
        return [x for c in self.calls for x in c["rels"]]


def _chunks(x):
    """The fired flags of each chunk the kernel walks: the head pairs in 32s, then the tail."""
    f, nh = x["fired"], x["n_head"]
    out = [f[c0:min(c0 + CHUNK, nh)] for c0 in range(0, nh, CHUNK)]
    if nh < x["n"]:
        out.append(f[nh:])
    return out


def _n_chunks(x):
    return (x["n"] + CHUNK - 1) // CHUNK


def _check_all_deferred(rec, B, env):
    for c in rec.calls:
        assert len(c["rels"]) == 1, "one relation owns every pair"
    assert all(sum(x["fired"]) >= 3 for x in rec.relations()), [sum(x["fired"]) for x in rec.relations()]
    assert any(len(_chunks(x)) >= 3 for x in rec.relations())


def _check_small(rec, B, env):
    base._check_small(rec, B)
    assert any(sum(x["fired"]) > 0 for x in rec.relations()), "no deferred record at all"


def _check_relpair(rec, B, env):
    base._check_relpair(rec, B)  # (entity'[r], r) a pair of its own that fires: the deferred relpair row


def _check_tail(rec, B, env):
    base._check_tail(rec, B)
    # a relation with records before its last update (pre) and among its pairs (post)
    assert any(base._restarts(x) and any(x["fired"][x["n_head"]:]) for x in rec.relations())


def _check_mixed(rec, B, env):
    th = int(env["KB2E_RPAR_REC_DEFER"])
    both = False
    for c in rec.calls:
        # (a chunk of margin on either side of the threshold)
        yes = [x for x in c["rels"] if _n_chunks(x) >= th + 1 and any(x["fired"])]
        no = [x for x in c["rels"] if _n_chunks(x) <= th - 1 and any(x["fired"])]
        hub = lambda xs: any(e == 0 and f for x in xs for e, f in zip(x["ents"], x["fired"]))
        both |= bool(yes) and bool(no) and hub(yes) and hub(no) and c["hub_events"] >= LONG_MIN
    assert both, [[(_n_chunks(x), sum(x["fired"])) for x in c["rels"]] for c in rec.calls]


def _check_windows(rec, B, env):
    base._check_windows(rec, B)
    assert max(sum(x["fired"]) for x in rec.relations()) >= 8


def _check_loop(rec, B, env):
    hit = [x for x in rec.relations() if any(f and e in x["loops"] for e, f in zip(x["ents"], x["fired"]))]
    assert hit, "no fired pair of an update whose head and tail are one entity"


def _check_publish(rec, B, env):
    chunks = [c for x in rec.relations() for c in _chunks(x)]
    assert any(sum(c) == 1 and c[-1] for c in chunks), "no chunk whose only violator is its last row"
    assert any(c[0] for c in chunks), "no chunk whose row 0 fires"
    assert any(sum(c) >= 6 for c in chunks), "no chunk of six violators"


def _check_ragged(rec, B, env):
    base._check_ragged(rec, B)


DEFER1 = {"KB2E_RPAR_REC_DEFER": "1"}
SKEW = "skew"

# (id, data set, dim, batches an epoch, batches trained, sub-batches, environment, check)
CASES = [
    ("all_deferred_n33", base.HUB1, 33, 50, 3, 1, DEFER1, _check_all_deferred),
    ("all_deferred_n50", base.HUB1, 50, 61, 3, 1, DEFER1, _check_all_deferred),
    ("all_deferred_n64", base.HUB1, 64, 50, 2, 1, DEFER1, _check_all_deferred),
    ("sparse_n20", base.SPARSE, 20, 4, 2, 1, DEFER1, _check_small),
    ("relpair_n50", base.HUB6, 50, 5, 2, 2, DEFER1, _check_relpair),
    ("tail_restart_n50", base.HUB6, 50, 5, 2, 2, DEFER1, _check_tail),
    ("mixed_threshold_n50", SKEW, 50, 5, 2, 1, {"KB2E_RPAR_REC_DEFER": "4"}, _check_mixed),
    ("windows_n50", base.HUB1, 50, 8, 2, 2,
     dict(DEFER1, KB2E_RPAR_CHAIN_LIST="64", KB2E_RPAR_CHAIN_TILES="2"), _check_windows),
    ("loop_update_n50", base.HUB6, 50, 5, 2, 2, DEFER1, _check_loop),
    ("publish_chunks_n50", base.HUB6, 50, 5, 2, 2, DEFER1, _check_publish),
    ("ragged_n50", base.HUB6, 50, 7, 2, 2, DEFER1, _check_ragged),
]


def _model(ds, dim, batches, trained, sub, monkeypatch):
    """base._model with this file's record."""
    rec = _Record(monkeypatch)
    m = orc.Model("R", dim, ds.num_entities, ds.num_relations, rate=base.RATE, distance=0, batches=batches,
                  transr_compat=True)
    m.set_triples(ds.train)
    orc.srand(base.SEED)
    m.prep_train()
    pe, pr, pw = m.tables()
    init = (pe.copy(), pr.copy(), pw.copy())
    pe = pe / np.linalg.norm(pe, axis=1, keepdims=True)
    B = m.batch_size()
    si, sj, side = m.sample_stream(B * batches)
    lo, ao = par.transr_parallel_batches(pe, pr, pw, ds.train, si, sj, side, B, trained, rate=base.RATE, l1=True,
                                         compat=True, work=[np.zeros(dim), np.zeros(dim)], St=base.ST,
                                         cons="chunk1", stats=rec.events, sub=sub)
    return init, (pe, pr, pw), lo, ao, rec, B


@pytest.mark.parametrize("name,shape,dim,batches,trained,sub,env,check", CASES, ids=[c[0] for c in CASES])
def test_pipe_defer_publish_same_bits(name, shape, dim, batches, trained, sub, env, check, monkeypatch):
    ds = _skewed_dataset() if shape == SKEW else base._hub_dataset(**shape)
    monkeypatch.setenv("KB2E_RPAR_ST", str(base.ST))
    monkeypatch.setenv("KB2E_RPAR_MFMA", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    init, want, lo, ao, rec, B = _model(ds, dim, batches, trained, sub, monkeypatch)
    check(rec, B, env)
    monkeypatch.setenv("KB2E_RPAR_PIPE_OPT", OFF)
    tabs0, loss0, act0 = base._engine(ds, dim, batches, trained, sub, init)
    monkeypatch.delenv("KB2E_RPAR_PIPE_OPT")
    tabs1, loss1, act1 = base._engine(ds, dim, batches, trained, sub, init)
    for which, a, b in zip(("entity", "relation", "matrix"), tabs0, tabs1):
        assert np.array_equal(a, b), (which, max_abs(a, b))
    assert loss0 == loss1 and act0 == act1, (loss0, loss1, act0, act1)
    # the model, at the walk test's bar
    errs = tuple(max_abs(g, m) for g, m in zip(tabs1, want))
    print(f"{name}: active {act1}, max|diff| to the model {errs}")
    assert act1 == ao, (act1, ao)
    assert abs(loss1 - lo) <= 1e-9 * max(1.0, abs(lo)), (loss1, lo)
    assert max(errs) < base.ATOL, errs
