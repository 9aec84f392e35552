"""The TransR row passes and the gradient kernel's partial stores under
KB2E_RPAR_ROWS_OPT (kernels_transr_parallel.hpp, kernels_transr_wave.hpp).

A bit a step, all on by default, 0 the path before them:

2  the gradient pass of the entity rows fetches 16 y rows at a time instead of four
   (rpar_entity_events; the record pass's pair rows stay at four);
4  the gradient kernel skips the partials of a tile without an active update and
   stores the others two columns (16 bytes in FP64, 8 in FP32: the same code path)
   a lane (transr_grad_wave_block).

(The long-segment combine of the gradient pass reads the waves' partials five waves at a
time under either setting: the same sums in the same order, no bit gates it.  The runs
against the model hold it.  Bit 1, a relation's row groups spread over workgroups, was measured and dropped with
its code -- DESIGN.md 7, round 12 -- so there is no run of it alone; the relation
cases stay: they hold the partials' skip and stores against their reader.)

They move loads and stores and change no sum, so every
case trains the same batches with KB2E_RPAR_ROWS_OPT=0 and at the default and asks
for bit-for-bit equal entity, relation and matrix tables, equal loss and active
counts; two cases also run each bit alone against 0.  The default run is held
against the CPU model (oracle/parallel.py) at the bar of
tests/test_gpu_transr_pipe_outside.py: the same active count, loss within 1e-9
relative, tables within 1e-9 -- at cons="chunk1", the form the FP64 engine runs,
and at cons="jacobi" for the KB2E_RPAR_CONS=jacobi case, whose GPU form that is
(tests/test_gpu_parallel.py holds it to the same bar).  The FP32 case follows
tests/test_gpu_transr_merged_phase_a.py, whose FP32 bar is bit identity between the
two paths and finite tables: the FP64 model is no 1e-9 reference for it.

The data sets and helpers are those of tests/test_gpu_transr_pipe_outside.py.  What a
case is there for is asserted from the model's own inputs to its constraint calls --
per sub-batch the samples, their relations and which are active -- with the kernels'
constants: tiles of ST samples in sample order within a relation, NQ = 8 partial rows
in flight, 64 events a chunk of an entity segment,
segments of 128 events or more on the whole-workgroup path.
"""
import numpy as np
import pytest

import oracle.parallel as par
import test_gpu_transr_pipe_outside as outside
from gpu_common import max_abs
from kb2e_amd import data
from kb2e_amd.engine import Engine
from oracle import orc

pytestmark = pytest.mark.gpu

HUB1, HUB6, SPARSE = outside.HUB1, outside.HUB6, outside.SPARSE
ST, RATE, SEED = outside.ST, outside.RATE, outside.SEED
ATOL = 1e-9
NQ = 8             # transr_rel_rows4_wave: partial rows in flight (the reader of the gradient kernel's partials)
LONG_MIN = 128     # kRParLongMin
DEEP_GRAD, DEEP_PAIR = 16, 4  # y rows in flight (kEntDeep), pair rows in flight
HUB2 = 150         # the second hub of _two_hub_dataset (no relation has this index)


def _two_hub_dataset(ne=300, nr=40, count=4000, seed=5):
    """The hub set with a second hub: entity 0 heads about half the triples, entity HUB2 about a
    tenth; 40 relations, so that HUB2 meets more relations a sub-batch than pair rows in flight."""
    rng = np.random.default_rng(seed)
    x = rng.random(count)
    h = np.where(x < 0.5, 0, np.where(x < 0.6, HUB2, rng.integers(1, ne, count)))
    t = rng.integers(1, ne, count)
    r = rng.integers(0, nr, count)
    tr = np.unique(np.stack([h, t, r], 1).astype(np.int32), axis=0)
    tr = tr[rng.permutation(len(tr))]
    return data.Dataset(ne, nr, tr, tr[:0], tr[:0])


class _Calls:
    """The inputs of every constraint call of the model (one a sub-batch): h, t, nh, nt, r of the
    batch, the active flags of the sub-batch's samples, and the pairs that fired with their entities
    (chunk1 only: from outside._Record)."""

    def __init__(self, monkeypatch, fired):
        self.calls = []
        inner = par.transr_constraint

        def capture(ent, W, h, t, nh, nt, r, act, rate, St=None, **kw):
            items = {}
            if fired:
                for rr in np.unique(r[act]):
                    items[int(rr)] = par._relation_items(r, rr, act, h, t, nh, nt, True, ent.shape[0])
            self.calls.append(dict(h=h.copy(), t=t.copy(), nh=nh.copy(), nt=nt.copy(), r=r.copy(), act=act.copy(),
                                   items=items))
            inner(ent, W, h, t, nh, nt, r, act, rate, St, **kw)

        monkeypatch.setattr(par, "transr_constraint", capture)
        self.rec = outside._Record(monkeypatch) if fired else None  # (wraps the capture)

    def subs(self, B, sub):
        """(call, first sample, end sample) of every sub-batch trained."""
        bounds = par.sub_batch_bounds(B, sub)
        return [(c, *bounds[k % len(bounds)]) for k, c in enumerate(self.calls)]


def _tiles(c, s0, s1):
    """Per relation of the sub-batch: the active-update count of each of its tiles."""
    out = {}
    r, act = c["r"][s0:s1], c["act"][s0:s1]
    for rr in np.unique(r):
        a = act[r == rr]
        out[int(rr)] = [int(a[q:q + ST].sum()) for q in range(0, len(a), ST)]
    return out


def _events(c, s0, s1, e):
    """Entity e's events of the sub-batch in (sample, update) order: True where the event adds a y
    row (an active update with e as head or tail, not both)."""
    ev = []
    for kk in range(s0, s1):
        for hh, tt in ((c["h"][kk], c["t"][kk]), (c["nh"][kk], c["nt"][kk])):
            if hh == e or tt == e:
                ev.append(bool(c["act"][kk]) and (hh == e) != (tt == e))
    return ev


# what each case is there for
def _check_many_tiles(calls, B, sub, n):
    for c, s0, s1 in calls.subs(B, sub):
        (tl,) = _tiles(c, s0, s1).values()  # one relation
        assert sum(x > 0 for x in tl) > 2 * NQ, tl  # several rounds of NQ partial rows


def _check_ragged(calls, B, sub, n):
    assert B % 2 == 1 and sub == 2, B  # the second sub-batch is one sample short
    assert (n + 1) % 4 != 0  # the last row group of a relation is a partial one
    for c, s0, s1 in calls.subs(B, sub):
        tl = _tiles(c, s0, s1)
        assert len(tl) == 6 and all(sum(x > 0 for x in v) >= 2 for v in tl.values()), tl


def _check_sparse(calls, B, sub, n):
    assert (n + 15) // 16 == 2
    for c, s0, s1 in calls.subs(B, sub):
        tl = _tiles(c, s0, s1)
        assert sum(len(v) == 1 for v in tl.values()) > len(tl) // 2, "most relations have one tile"
        flat = [x for v in tl.values() for x in v]
        assert any(x == 0 for x in flat) and any(x > 0 for x in flat), flat  # skipped partials beside live ones


def _live_tiles(calls, B, sub):
    return sum(x > 0 for c, s0, s1 in calls.subs(B, sub) for v in _tiles(c, s0, s1).values() for x in v)


def _check_odd(calls, B, sub, n):
    assert (n + 15) // 16 == 3 and n % 2 == 1  # every live tile stores column n - 1 on its own
    assert _live_tiles(calls, B, sub) > 0


def _check_full(calls, B, sub, n):
    assert n == 64
    assert _live_tiles(calls, B, sub) > 0


def _check_long(calls, B, sub, n):
    for c, s0, s1 in calls.subs(B, sub):
        assert len(_events(c, s0, s1, 0)) >= LONG_MIN


def _check_medium(calls, B, sub, n):
    reached_grad = reached_pair = False
    for k, (c, s0, s1) in enumerate(calls.subs(B, sub)):
        ev = _events(c, s0, s1, HUB2)
        if not 64 < len(ev) < LONG_MIN:  # (two chunks on one wave)
            continue
        reached_grad |= sum(ev[:64]) > DEEP_GRAD  # several deep groups in a chunk
        # HUB2's pair rows of the record pass: its pairs that fired (a pair a relation)
        rels = calls.rec.calls[k]["rels"]
        moved = sum(1 for x in rels for (e, _), f in zip(c["items"][x["r"]], x["fired"]) if f and e == HUB2)
        reached_pair |= moved > 2 * DEEP_PAIR  # more than a fetch group in one of its two chunks
    assert reached_grad and reached_pair, (reached_grad, reached_pair)


def _check_defer(calls, B, sub, n):
    # KB2E_RPAR_REC_DEFER=1: every relation with a pair leaves its records to the entity pass; entity 0
    # takes more converted rows a sub-batch than a fetch group holds
    for k, (c, s0, s1) in enumerate(calls.subs(B, sub)):
        rels = calls.rec.calls[k]["rels"]
        moved = sum(1 for x in rels for (e, _), f in zip(c["items"][x["r"]], x["fired"]) if f)
        assert moved > DEEP_PAIR, moved


def _check_jacobi(calls, B, sub, n):
    for c, s0, s1 in calls.subs(B, sub):
        assert len(_tiles(c, s0, s1)) == 6


def _check_fp32(calls, B, sub, n):
    assert _live_tiles(calls, B, sub) > 0


TWOHUB = dict(ne=300, nr=40, count=4000)

# (id, data set, dim, batches an epoch, batches trained, sub-batches, environment, precision, model form, check)
CASES = [
    ("one_relation_n50_sub1", HUB1, 50, 8, 2, 1, {}, 64, "chunk1", _check_many_tiles),
    ("one_relation_n50_sub2", HUB1, 50, 8, 2, 2, {}, 64, "chunk1", _check_many_tiles),
    ("ragged_n50", HUB6, 50, 7, 2, 2, {}, 64, "chunk1", _check_ragged),
    ("sparse_n20", SPARSE, 20, 4, 2, 1, {}, 64, "chunk1", _check_sparse),
    ("odd_n33", HUB6, 33, 5, 2, 2, {}, 64, "chunk1", _check_odd),
    ("full_n64", HUB1, 64, 8, 1, 2, {}, 64, "chunk1", _check_full),
    ("long_entity_n50", HUB6, 50, 5, 2, 2, {}, 64, "chunk1", _check_long),
    ("medium_entity_n50", TWOHUB, 50, 5, 2, 2, {}, 64, "chunk1", _check_medium),
    ("deferred_n50", HUB1, 50, 8, 2, 2, {"KB2E_RPAR_REC_DEFER": "1"}, 64, "chunk1", _check_defer),
    ("jacobi_n50", HUB6, 50, 5, 2, 2, {"KB2E_RPAR_CONS": "jacobi"}, 64, "jacobi", _check_jacobi),
    ("fp32_n50", HUB6, 50, 5, 2, 2, {}, 32, None, _check_fp32),
]
BIT_CASES = [c for c in CASES if c[0] in ("ragged_n50", "sparse_n20")]


def _dataset(shape):
    return _two_hub_dataset(**shape) if shape is TWOHUB else outside._hub_dataset(**shape)


def _model(ds, dim, batches, trained, sub, cons, monkeypatch):
    """outside._model with the constraint calls' inputs kept and the model's form a parameter."""
    calls = _Calls(monkeypatch, fired=cons == "chunk1")
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
    stats = calls.rec.events if calls.rec else None
    lo, ao = par.transr_parallel_batches(pe, pr, pw, ds.train, si, sj, side, B, trained, rate=RATE, l1=True,
                                         compat=True, work=[np.zeros(dim), np.zeros(dim)], St=ST,
                                         cons=cons or "chunk1", stats=stats, sub=sub)
    return init, (pe, pr, pw), lo, ao, calls, B


def _engine(ds, dim, batches, trained, sub, precision, init):
    if precision == 64:
        return outside._engine(ds, dim, batches, trained, sub, init)
    eng = Engine("R", dim, ds.num_entities, ds.num_relations, rate=RATE, distance=0, batches=batches, seed=SEED,
                 schedule="parallel", transr_compat=True, sub_batches=sub, precision=precision)
    eng.upload_triples(ds.train)
    e0, r0, _ = eng.init_params()
    eng.transr_seed(e0, r0)
    eng.train_batches(trained)
    loss, act = eng.take_stats()
    tabs = eng.download_params()
    eng.close()
    return tabs, loss, act


def _run(opt, monkeypatch, ds, dim, batches, trained, sub, precision, init):
    if opt is None:
        monkeypatch.delenv("KB2E_RPAR_ROWS_OPT", raising=False)
    else:
        monkeypatch.setenv("KB2E_RPAR_ROWS_OPT", str(opt))
    return _engine(ds, dim, batches, trained, sub, precision, init)


def _same(x, y):
    (tabs0, loss0, act0), (tabs1, loss1, act1) = x, y
    for which, a, b in zip(("entity", "relation", "matrix"), tabs0, tabs1):
        assert np.array_equal(a, b), (which, max_abs(a, b))
    assert loss0 == loss1 and act0 == act1, (loss0, loss1, act0, act1)


def _setup(shape, dim, batches, trained, sub, env, cons, check, monkeypatch):
    ds = _dataset(shape)
    monkeypatch.setenv("KB2E_RPAR_ST", str(ST))
    monkeypatch.setenv("KB2E_RPAR_MFMA", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    init, want, lo, ao, calls, B = _model(ds, dim, batches, trained, sub, cons, monkeypatch)
    check(calls, B, sub, dim)
    return ds, init, want, lo, ao


@pytest.mark.parametrize("name,shape,dim,batches,trained,sub,env,precision,cons,check", CASES,
                         ids=[c[0] for c in CASES])
def test_rows_opt_same_bits(name, shape, dim, batches, trained, sub, env, precision, cons, check, monkeypatch):
    ds, init, want, lo, ao = _setup(shape, dim, batches, trained, sub, env, cons, check, monkeypatch)
    args = (monkeypatch, ds, dim, batches, trained, sub, precision, init)
    before = _run(0, *args)
    after = _run(None, *args)
    _same(before, after)
    tabs1, loss1, act1 = after
    assert all(np.isfinite(t).all() for t in tabs1)
    if cons is None:  # FP32: bit identity between the two paths is the bar
        print(f"{name}: active {act1}, loss {loss1}")
        return
    errs = tuple(max_abs(g, m) for g, m in zip(tabs1, want))
    print(f"{name}: active {act1} (model {ao}), loss {loss1} (model {lo}), max|diff| to the model {errs}")
    assert act1 == ao, (act1, ao)
    assert abs(loss1 - lo) <= 1e-9 * max(1.0, abs(lo)), (loss1, lo)
    assert max(errs) < ATOL, errs


@pytest.mark.parametrize("name,shape,dim,batches,trained,sub,env,precision,cons,check", BIT_CASES,
                         ids=[c[0] for c in BIT_CASES])
def test_rows_opt_each_bit_alone(name, shape, dim, batches, trained, sub, env, precision, cons, check, monkeypatch):
    ds, init, _, _, _ = _setup(shape, dim, batches, trained, sub, env, cons, check, monkeypatch)
    args = (monkeypatch, ds, dim, batches, trained, sub, precision, init)
    before = _run(0, *args)
    for bit in (2, 4):
        _same(before, _run(bit, *args))
