"""The TransR entity passes and the compat energy launch under KB2E_RPAR_PASS_OPT
(kernels_transr_parallel.hpp).

A bit a step, all on by default, 0 the path before them:

1  the entity passes (gradient and record pass, alone or in the fused row launch) run as
   four-wave workgroups, a wave a short segment and a workgroup for every four entity
   segments of the index batch, so no wave takes a second segment; a segment of 128
   events or more takes its whole workgroup, sixteen chunk streams (chunks st, st + 16,
   ...) at four a wave, combined in stream order (transr_entity_block4);
4  the compat energy launch fetches everything that depends on no sum -- the earlier
   chunks' sums, the last chunk's calls of every earlier sub-batch, its own calls, the
   samples' relation rows -- ahead of its first barrier, sixteen calls a thread, and walks
   the additions in their order (rpar_scan_energy_ahead).

(Bit 2, the head loads of a wave's next segment ahead of the current one's finish, was
not built: with bit 1 no wave takes a second segment.  DESIGN.md 7, round 13.)

They change which wave takes which segment and when a load is issued, and no sum, so
every case trains the same batches with KB2E_RPAR_PASS_OPT=0 and at the default and asks
for bit-for-bit equal entity, relation and matrix tables, equal loss and active counts;
two cases also run each bit alone against 0.  The default FP64 run is held against the
CPU model (oracle/parallel.py, cons="chunk1") at the bar of
tests/test_gpu_transr_rows_opt.py: the same active count, loss within 1e-9 relative,
tables within 1e-9.  The FP32 case is held to bit identity between the two paths and
finite tables, as there.

The data sets and helpers are those of tests/test_gpu_transr_pipe_outside.py and
tests/test_gpu_transr_rows_opt.py, cut to a number of triples that gives the batch size a
case needs.  What a case is there for is asserted from the model's own inputs to its
constraint calls, with the kernels' constants: 64 calls (two a sample) a chunk of the
scan, 64 events a chunk of an entity segment, segments of 128 events or more on the
whole-workgroup path, sixteen chunk streams.
"""
import numpy as np
import pytest

import oracle.parallel as par
import test_gpu_transr_pipe_outside as outside
import test_gpu_transr_rows_opt as rows
from gpu_common import max_abs
from kb2e_amd import data
from kb2e_amd.engine import Engine
from oracle import orc

pytestmark = pytest.mark.gpu

HUB1, HUB6, SPARSE, TWOHUB = outside.HUB1, outside.HUB6, outside.SPARSE, rows.TWOHUB
ST, RATE, SEED = outside.ST, outside.RATE, outside.SEED
ATOL = 1e-9
SCAN_CHUNK = 64      # kScanChunk: calls a chunk, two a sample
EVENT_CHUNK = 64     # events a chunk of an entity segment
LONG_MIN = 128       # kRParLongMin
STREAMS = 16         # kRParWaves: chunk streams of a long segment
BLOCK_WAVES = 16     # waves of a workgroup of the path before (four with bit 1)
HUB, HUB2 = 0, rows.HUB2
WRAP = dict(ne=1000, nr=6, count=6000)  # the hub set, larger: the hub takes more than 16 chunks a sub-batch
BITS = (1, 4)


def _dataset(shape, count):
    """The set of `shape`, cut to its first `count` triples (None: all of them)."""
    ds = rows._dataset(shape)
    if count is None:
        return ds
    assert len(ds.train) >= count, (len(ds.train), count)
    return data.Dataset(ds.num_entities, ds.num_relations, ds.train[:count], ds.train[:0], ds.train[:0])


def _entities(c, s0, s1):
    """The entities with an event in the sub-batch."""
    return np.unique(np.concatenate([c[k][s0:s1] for k in ("h", "t", "nh", "nt")]))


def _records(calls, k, c, e):
    """Entity e's pair records of constraint call k: its pairs that fired."""
    rels = calls.rec.calls[k]["rels"]
    return sum(1 for x in rels for (ee, _), f in zip(c["items"][x["r"]], x["fired"]) if f and ee == e)


# what each case is there for
def _check_scan(last, chunks_min):
    def check(calls, B, sub, n):
        subs = calls.subs(B, sub)
        assert len({(s0, s1) for _, s0, s1 in subs}) == sub
        for _, s0, s1 in subs[:max(1, sub - 1)]:  # the full sub-batches: the carry-in reads their last chunk
            ncalls = 2 * (s1 - s0)
            assert (ncalls - 1) % SCAN_CHUNK + 1 == last, (ncalls, last)
            assert -(-ncalls // SCAN_CHUNK) >= chunks_min, ncalls
    return check


def _check_ragged(calls, B, sub, n):
    assert B % 2 == 1 and sub == 2, B  # the second sub-batch is one sample short
    _check_scan(34, 3)(calls, B, sub, n)


def _check_one_chunk(calls, B, sub, n):
    for _, s0, s1 in calls.subs(B, sub):
        assert 2 * (s1 - s0) <= SCAN_CHUNK
    assert sub == 3  # two carry steps


def _check_post_delta(calls, B, sub, n):
    """An (entity'[r], r) delta of a row no update of the sub-batch touches (it is added after the
    norm, "post"), beside the scan's last chunk."""
    _check_scan(18, 3)(calls, B, sub, n)
    found = False
    for c, s0, s1 in calls.subs(B, sub):
        act = c["act"][s0:s1]
        touched = set(_entities({key: c[key][s0:s1][act] for key in ("h", "t", "nh", "nt")}, 0, None).tolist())
        found |= any(int(r) not in touched for r in np.unique(c["r"][s0:s1][act]))
    assert found


def _check_wrap(calls, B, sub, n):
    both = pre = False
    for k, (c, s0, s1) in enumerate(calls.subs(B, sub)):
        ev = rows._events(c, s0, s1, HUB)
        assert len(ev) >= (STREAMS + 1) * EVENT_CHUNK, len(ev)  # stream 0 takes a second chunk
        assert sum(ev[STREAMS * EVENT_CHUNK:]) > 0  # ... with a y row to add
        assert _records(calls, k, c, HUB) > 0  # the record pass has rows of it
        assert len(_entities(c, s0, s1)) > 4 * BLOCK_WAVES  # more short segments than a workgroup's waves
        act = c["act"][s0:s1]
        # an entity that is head and tail of one active update
        both |= bool(np.any(act & ((c["h"][s0:s1] == c["t"][s0:s1]) | (c["nh"][s0:s1] == c["nt"][s0:s1]))))
        # (entity'[r], r) deltas of rows that an active update renormalises (they are added before the norm):
        # the hub is relation 0's row, and the other relations' rows are tails of the set
        active_rels = np.unique(c["r"][s0:s1][act])
        ents_act = _entities({key: c[key][s0:s1][act] for key in ("h", "t", "nh", "nt")}, 0, None)
        pre |= HUB in active_rels and sum(int(r) in ents_act for r in active_rels) >= 2
    assert both and pre, (both, pre)


def _check_stream(calls, B, sub, n):
    hit = False
    for k, (c, s0, s1) in enumerate(calls.subs(B, sub)):
        ev = rows._events(c, s0, s1, HUB2)
        if LONG_MIN <= len(ev) < 3 * EVENT_CHUNK and sum(ev) > 0 and _records(calls, k, c, HUB2) > 0:
            hit = True  # a long segment of three chunks at the most: one stream a wave busy
        assert len(_entities(c, s0, s1)) > 4 * BLOCK_WAVES
    assert hit


def _check_defer(calls, B, sub, n):
    rows._check_defer(calls, B, sub, n)
    for c, s0, s1 in calls.subs(B, sub):  # the hub's segment is a long one: converted rows in the streams
        assert len(rows._events(c, s0, s1, HUB)) >= LONG_MIN


def _check_segments(calls, B, sub, n):
    for c, s0, s1 in calls.subs(B, sub):
        assert len(_entities(c, s0, s1)) > 4 * BLOCK_WAVES
        assert len(rows._events(c, s0, s1, HUB)) >= LONG_MIN


# (id, data set, triples, dim, batches an epoch, batches trained, sub-batches, environment, precision, compat, check)
CASES = [
    ("scan_last2_n20_k1", SPARSE, 4 * 65, 20, 4, 2, 1, {}, 64, True, _check_scan(2, 3)),
    ("scan_last18_post_n33_k1", HUB6, 4 * 73, 33, 4, 2, 1, {}, 64, True, _check_post_delta),
    ("scan_last34_ragged_n50_k2", HUB6, 3 * 161, 50, 3, 2, 2, {}, 64, True, _check_ragged),
    ("scan_last62_n64_k3", HUB6, 2 * 284, 64, 2, 2, 3, {}, 64, True, _check_scan(62, 3)),
    ("scan_full64_n50_k2", HUB6, 3 * 128, 50, 3, 2, 2, {}, 64, True, _check_scan(64, 2)),
    ("scan_one_chunk_n50_k3", HUB6, 4 * 75, 50, 4, 2, 3, {}, 64, True, _check_one_chunk),
    ("fixed_energy_n50_k2", HUB6, None, 50, 5, 2, 2, {}, 64, False, _check_segments),
    ("wrap_n20_k2", WRAP, None, 20, 1, 1, 2, {}, 64, True, _check_wrap),
    ("stream_n50_k2", TWOHUB, None, 50, 2, 1, 2, {}, 64, True, _check_stream),
    ("deferred_n50_k2", HUB6, None, 50, 5, 2, 2, {"KB2E_RPAR_REC_DEFER": "1"}, 64, True, _check_defer),
    ("fuse0_n33_k2", HUB6, None, 33, 5, 2, 2, {"KB2E_RPAR_FUSE": "0"}, 64, True, _check_segments),
    ("fp32_n50_k2", HUB6, None, 50, 5, 2, 2, {}, 32, True, _check_segments),
]
BIT_CASES = [c for c in CASES if c[0] in ("scan_last34_ragged_n50_k2", "deferred_n50_k2")]
IDS = "name,shape,count,dim,batches,trained,sub,env,precision,compat,check"


def _model(ds, dim, batches, trained, sub, compat, monkeypatch):
    """rows._model with the energy form a parameter."""
    calls = rows._Calls(monkeypatch, fired=True)
    m = orc.Model("R", dim, ds.num_entities, ds.num_relations, rate=RATE, distance=0, batches=batches,
                  transr_compat=compat)
    m.set_triples(ds.train)
    orc.srand(SEED)
    m.prep_train()
    pe, pr, pw = m.tables()
    init = (pe.copy(), pr.copy(), pw.copy())
    pe = pe / np.linalg.norm(pe, axis=1, keepdims=True)
    B = m.batch_size()
    si, sj, side = m.sample_stream(B * batches)
    lo, ao = par.transr_parallel_batches(pe, pr, pw, ds.train, si, sj, side, B, trained, rate=RATE, l1=True,
                                         compat=compat, work=[np.zeros(dim), np.zeros(dim)] if compat else None,
                                         St=ST, cons="chunk1", stats=calls.rec.events, sub=sub)
    return init, (pe, pr, pw), lo, ao, calls, B


def _engine(ds, dim, batches, trained, sub, precision, compat, init):
    eng = Engine("R", dim, ds.num_entities, ds.num_relations, rate=RATE, distance=0, batches=batches, seed=SEED,
                 schedule="parallel", transr_compat=compat, sub_batches=sub, precision=precision)
    eng.upload_triples(ds.train)
    e0, r0, w0 = eng.init_params()
    if precision == 64:
        assert all(np.array_equal(a, b) for a, b in zip((e0, r0, w0), init))
    eng.transr_seed(e0, r0)
    eng.train_batches(trained)
    loss, act = eng.take_stats()
    tabs = eng.download_params()
    eng.close()
    return tabs, loss, act


def _run(opt, monkeypatch, *args):
    if opt is None:
        monkeypatch.delenv("KB2E_RPAR_PASS_OPT", raising=False)
    else:
        monkeypatch.setenv("KB2E_RPAR_PASS_OPT", str(opt))
    return _engine(*args)


def _setup(shape, count, dim, batches, trained, sub, env, compat, check, monkeypatch):
    ds = _dataset(shape, count)
    monkeypatch.setenv("KB2E_RPAR_ST", str(ST))
    monkeypatch.setenv("KB2E_RPAR_MFMA", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    init, want, lo, ao, calls, B = _model(ds, dim, batches, trained, sub, compat, monkeypatch)
    if count is not None:
        assert B * batches == count, (B, batches, count)
    check(calls, B, sub, dim)
    return ds, init, want, lo, ao


@pytest.mark.parametrize(IDS, CASES, ids=[c[0] for c in CASES])
def test_pass_opt_same_bits(name, shape, count, dim, batches, trained, sub, env, precision, compat, check,
                            monkeypatch):
    ds, init, want, lo, ao = _setup(shape, count, dim, batches, trained, sub, env, compat, check, monkeypatch)
    args = (monkeypatch, ds, dim, batches, trained, sub, precision, compat, init)
    before = _run(0, *args)
    after = _run(None, *args)
    rows._same(before, after)
    tabs1, loss1, act1 = after
    assert all(np.isfinite(t).all() for t in tabs1)
    if precision == 32:  # bit identity between the two paths is the bar
        print(f"{name}: active {act1}, loss {loss1}")
        return
    errs = tuple(max_abs(g, m) for g, m in zip(tabs1, want))
    print(f"{name}: active {act1} (model {ao}), loss {loss1} (model {lo}), max|diff| to the model {errs}")
    assert act1 == ao, (act1, ao)
    assert abs(loss1 - lo) <= 1e-9 * max(1.0, abs(lo)), (loss1, lo)
    assert max(errs) < ATOL, errs


@pytest.mark.parametrize(IDS, BIT_CASES, ids=[c[0] for c in BIT_CASES])
def test_pass_opt_each_bit_alone(name, shape, count, dim, batches, trained, sub, env, precision, compat, check,
                                 monkeypatch):
    ds, init, _, _, _ = _setup(shape, count, dim, batches, trained, sub, env, compat, check, monkeypatch)
    args = (monkeypatch, ds, dim, batches, trained, sub, precision, compat, init)
    before = _run(0, *args)
    for bit in BITS:
        rows._same(before, _run(bit, *args))
