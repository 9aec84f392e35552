"""Entity neighbours (kb2e_neighbors) against the oracle.

The oracle for a space is plain numpy over the energies of orc.Model(...,
transr_compat=False) with an all-zero relation table: d(a, x) is the energy of
(a, x, r), in the entity space that of a TransE model on the same entity table.
Per query: the row of |E| energies, the query itself dropped unless asked for,
np.lexsort((ids, energy))[:k].  All device arithmetic is FP64 in the evaluator's
order and ties break on the entity id, so ids, distance bits and found counts
must be EQUAL (no tolerance anywhere in this file).
"""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from gpu_common import MANIFEST, tiny
from kb2e_amd import data, linkpred
from kb2e_amd.engine import Engine, EngineError, lib
from oracle import orc

pytestmark = pytest.mark.gpu

KNOBS = ("KB2E_NEIGHBORS_SLICE", "KB2E_NEIGHBORS_CHUNK_ROWS", "KB2E_EVAL_ROWS_L2")


# ------------------------------------------------------------------ helpers

def _random_tables(model, ne, nr, n, seed, scale=0.3):
    """tests/test_gpu_predict.py _tables' recipe."""
    rng = np.random.default_rng(seed)
    if model == "R":
        ent = rng.standard_normal((ne, n))
        ent /= np.linalg.norm(ent, axis=1, keepdims=True)
        rel = rng.standard_normal((nr, n)) * scale
        w = np.eye(n)[None] + rng.standard_normal((nr, n, n)) * (scale / np.sqrt(n))
        return ent, rel, w
    ent = rng.standard_normal((ne, n)) * 0.2
    rel = rng.standard_normal((nr, n)) * 0.2
    w = None
    if model == "H":
        w = rng.standard_normal((nr, n))
        w /= np.linalg.norm(w, axis=1, keepdims=True)
    return ent, rel, w


def _f32(tables):
    return tuple(None if t is None else t.astype(np.float32).astype(np.float64) for t in tables)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    return all(np.array_equal(_bits(x) if x.dtype == np.float64 else x, _bits(y) if y.dtype == np.float64 else y)
               for x, y in zip(a, b))


def _counters(eng):
    return {c: eng.counter("neighbors_" + c) for c in ("candidates", "slices", "chunks", "prunes")}


class Setup:
    """An engine and the oracle on the same tables.  The distance matrix of a
    space is computed once from the oracle and never modified."""

    def __init__(self, model, n, ne, nr, tables, *, distance=0, precision=64):
        self.model, self.n, self.ne, self.nr = model, n, ne, nr
        self.eng = Engine(model, n, ne, nr, distance=distance, precision=precision)
        self.eng.upload_params(*tables)
        self.tables = _f32(tables) if precision == 32 else tables
        self.odist = 0 if (model == "H" or distance == 0) else 1  # (a TransH context is L1)
        self._D = {}

    def distances(self, rel):
        if rel not in self._D:
            ent, _, w = self.tables
            if rel < 0:
                m = orc.Model("E", self.n, self.ne, 1, distance=self.odist, transr_compat=False)
                m.set_tables(ent, np.zeros((1, self.n)))
                r = 0
            else:
                m = orc.Model(self.model, self.n, self.ne, self.nr, distance=self.odist, transr_compat=False)
                m.set_tables(ent, np.zeros((self.nr, self.n)), w)
                r = rel
            D = np.array([m.energy(a, x, r) for a in range(self.ne) for x in range(self.ne)]).reshape(self.ne, self.ne)
            D.setflags(write=False)
            self._D[rel] = D
        return self._D[rel]

    def expect(self, ents, k, rel, include_self):
        D = self.distances(rel)
        ents = np.asarray(ents).reshape(-1)
        ids = np.full((len(ents), k), -1, np.int32)
        dist = np.full((len(ents), k), np.inf)
        found = np.zeros(len(ents), np.int32)
        every = np.arange(self.ne)
        for q, a in enumerate(ents.tolist()):
            cand = every if include_self else every[every != a]
            e = D[a, cand]
            order = np.lexsort((cand, e))[:k]
            found[q] = len(order)
            ids[q, :len(order)] = cand[order]
            dist[q, :len(order)] = e[order]
        return ids, dist, found

    def check(self, ents, k, rel=-1, include_self=False):
        got = self.eng.neighbors(ents, k, relation=rel, include_self=include_self)
        exp = self.expect(ents, k, rel, include_self)
        ids, dist, found = got
        nq = len(np.asarray(ents).reshape(-1))
        assert ids.shape == dist.shape == (nq, k) and found.shape == (nq,)
        assert ids.dtype == np.int32 and dist.dtype == np.float64 and found.dtype == np.int32
        assert np.array_equal(found, exp[2])
        assert np.array_equal(ids, exp[0])
        assert np.array_equal(_bits(dist), _bits(exp[1]))  # the bits (+inf padding included)
        return got


def _golden_tables(name):
    """The trained tables of a golden run, after its last epoch."""
    run = MANIFEST["runs"][name]
    d = os.path.join(GOLDEN, name)
    last = run["flags"]["epochs"] - 1
    ent = np.load(os.path.join(d, f"epoch{last}_ent.npy"))
    rel = np.load(os.path.join(d, f"epoch{last}_rel.npy"))
    w = np.load(os.path.join(d, f"epoch{last}_w.npy")) if run["model"] != "E" else None
    return run, (ent, rel, w)


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    for key in KNOBS:
        monkeypatch.delenv(key, raising=False)


# ------------------------------------------------------------------ 1. oracle, golden models

@pytest.mark.parametrize("name", ["transe_l1_bern", "transe_l2_unif", "transh_bern", "transr_fixed"])
def test_neighbors_golden_models_against_oracle(name):
    """The golden-trained tables of one run per model (E L1, E L2, H, R): the
    graph of all 200 entities in the entity space and in the spaces of relations
    2 and 7; k = 1, 10, 128; with and without the entity itself."""
    run, tables = _golden_tables(name)
    f = run["flags"]
    s = Setup(run["model"], f["size"], 200, 10, tables, distance=f["distance"])
    every = np.arange(200, dtype=np.int32)
    for rel, k, own in itertools.product((-1, 2, 7), (1, 10, 128), (False, True)):
        ids, dist, found = s.check(every, k, rel, own)
        assert (found == k).all()
        if own:  # d(a, a) = +0 and nothing is nearer
            assert (dist[:, 0] == 0).all()
    # the graph is that call
    assert _same(s.eng.knn_graph(10, relation=7), s.eng.neighbors(every, 10, relation=7))
    c = _counters(s.eng)
    assert c["candidates"] == 200 * 200 and c["chunks"] == 1 and c["slices"] == 13 and c["prunes"] > 0


# ------------------------------------------------------------------ 2. shapes

SHAPES = [("E", 7, 0, 64), ("E", 50, 1, 64), ("E", 512, 0, 64), ("H", 50, 0, 64), ("R", 7, 1, 64), ("R", 50, 0, 64),
          ("E", 50, 0, 32)]


@pytest.mark.parametrize("model,n,distance,precision", SHAPES)
def test_neighbors_shapes_geometry_and_row_forms(model, n, distance, precision, monkeypatch):
    """|E| = 300: 19 query tiles, the last ragged, and two steps of 256
    candidates, the second ragged; n = 7 (odd, padded leading dimension), 50 and
    512.  Forced slices of 64 and 300 candidates, chunks of 16 rows and the
    tile rows read from L2 give the default run's results, which are the
    oracle's (FP32 tables: the oracle on the widened tables); the counters show
    the slices, the chunks and the bound at work."""
    ne, nr = 300, 3
    s = Setup(model, n, ne, nr, _random_tables(model, ne, nr, n, seed=n + distance), distance=distance,
              precision=precision)
    every = np.arange(ne, dtype=np.int32)
    cases = [(10, -1, False), (128, -1, True), (10, 1, False), (128, 1, False)]
    plain = []
    for k, rel, own in cases:
        plain.append(s.check(every, k, rel, own))
        c = _counters(s.eng)
        assert c == {"candidates": ne * ne, "slices": 19, "chunks": 1, "prunes": c["prunes"]} and c["prunes"] > 0
    for knobs, slices, chunks in (({"KB2E_NEIGHBORS_SLICE": "64"}, 19 * 5, 1),
                                  ({"KB2E_NEIGHBORS_SLICE": "300"}, 19, 1),
                                  ({"KB2E_NEIGHBORS_CHUNK_ROWS": "16"}, 19, 19),
                                  ({"KB2E_NEIGHBORS_SLICE": "64", "KB2E_NEIGHBORS_CHUNK_ROWS": "16"}, 19 * 5, 19),
                                  ({"KB2E_EVAL_ROWS_L2": "1", "KB2E_NEIGHBORS_SLICE": "64"}, 19 * 5, 1)):
        for key in KNOBS:
            monkeypatch.delenv(key, raising=False)
        for key, v in knobs.items():
            monkeypatch.setenv(key, v)
        for (k, rel, own), base in zip(cases, plain):
            got = s.eng.neighbors(every, k, relation=rel, include_self=own)
            assert _same(got, base), (knobs, k, rel, own)
            c = _counters(s.eng)
            assert (c["candidates"], c["slices"], c["chunks"]) == (ne * ne, slices, chunks) and c["prunes"] > 0


# ------------------------------------------------------------------ 3. ties

@pytest.mark.parametrize("distance", [0, 1])
def test_neighbors_ties_break_on_the_entity_id(distance, monkeypatch):
    """Entities 50..199 share one row: 150 entities at distance +0 of each
    other, more than k = 128, with a slice length (128) that cuts the class in
    two.  The class comes out by ascending id, self-exclusion removes exactly
    the query's own id, and two queries inside the class get different lists."""
    ne, nr, n = 300, 2, 12
    ent, rel, _ = _random_tables("E", ne, nr, n, seed=31)
    ent[50:200] = ent[50]
    s = Setup("E", n, ne, nr, (ent, rel, None), distance=distance)
    D = s.distances(-1)
    assert (D[50:200, 50:200] == 0).all() and (D[50, :50] > 0).all() and (D[50, 200:] > 0).all()  # the guard
    queries = np.array([50, 51, 127, 128, 199, 10, 250], np.int32)
    for slice_len in (None, "128", "64"):
        if slice_len:
            monkeypatch.setenv("KB2E_NEIGHBORS_SLICE", slice_len)
        for k, own in itertools.product((128, 10), (False, True)):
            ids, dist, found = s.check(queries, k, -1, own)
            for q, a in enumerate(queries[:5].tolist()):
                cls = [x for x in range(50, 200) if own or x != a][:k]
                assert ids[q].tolist() == cls and (dist[q] == 0).all() and not np.signbit(dist[q]).any()
            assert ids[0].tolist() != ids[1].tolist() or own
            if not own:
                assert (ids != queries[:, None]).all()
                assert 51 in ids[0] and 50 in ids[1] and 50 not in ids[0] and 51 not in ids[1]


# ------------------------------------------------------------------ 4. edges

def test_neighbors_k_at_least_the_entity_count():
    ne, nr = 20, 2
    s = Setup("E", 8, ne, nr, _random_tables("E", ne, nr, 8, seed=1))
    every = np.arange(ne, dtype=np.int32)
    for k in (20, 128):
        ids, dist, found = s.check(every, k, -1, False)
        assert (found == ne - 1).all()
        assert (ids[:, ne - 1:] == -1).all() and np.isposinf(dist[:, ne - 1:]).all()
        assert (ids[:, :ne - 1] >= 0).all() and np.isfinite(dist[:, :ne - 1]).all()
        ids, dist, found = s.check(every, k, 1, True)
        assert (found == ne).all() and (ids[:, ne:] == -1).all() and np.isposinf(dist[:, ne:]).all()
    ids, dist, found = s.check(every, 19, -1, False)
    assert (found == 19).all() and (ids >= 0).all()


@pytest.mark.parametrize("model", ["E", "H", "R"])
def test_neighbors_one_query_seventeen_and_a_repeated_entity(model):
    ne, nr, n = 300, 3, 10
    s = Setup(model, n, ne, nr, _random_tables(model, ne, nr, n, seed=6))
    for rel in (-1, 2):
        s.check([299], 10, rel)                                   # nq = 1, the last entity
        s.check(np.arange(100, 117), 10, rel, True)                # nq = 17: a full tile and a tile of one row
        ids, dist, _ = s.check([5, 9, 5, 5, 299, 9], 7, rel)       # listed twice: each listing is answered
        assert np.array_equal(ids[0], ids[2]) and np.array_equal(ids[0], ids[3]) and np.array_equal(ids[1], ids[5])
        assert np.array_equal(_bits(dist[0]), _bits(dist[3]))


def test_neighbors_of_the_only_entity():
    ent, rel, _ = _random_tables("E", 1, 1, 6, seed=2)
    s = Setup("E", 6, 1, 1, (ent, rel, None))
    ids, dist, found = s.check([0], 5, -1, False)
    assert found.tolist() == [0] and (ids == -1).all() and np.isposinf(dist).all()
    ids, dist, found = s.check([0, 0], 5, 0, True)
    assert found.tolist() == [1, 1] and ids[:, 0].tolist() == [0, 0] and (dist[:, 0] == 0).all()


# ------------------------------------------------------------------ 5. symmetry

@pytest.mark.parametrize("model,distance,rel", [("E", 0, -1), ("E", 1, -1), ("H", 0, 1), ("R", 1, 2), ("R", 0, -1)])
def test_neighbors_distance_is_symmetric_in_bits(model, distance, rel):
    ne, nr, n = 300, 3, 24
    eng = Engine(model, n, ne, nr, distance=distance)
    eng.upload_params(*_random_tables(model, ne, nr, n, seed=44))
    ids, dist, found = eng.knn_graph(40, relation=rel)
    assert (found == 40).all()
    seen = {(a, int(b)): _bits(dist[a, j:j + 1])[0] for a in range(ne) for j, b in enumerate(ids[a])}
    both = [(a, b) for (a, b) in seen if (b, a) in seen]
    assert len(both) > ne  # (nearness is mostly mutual: the check is not vacuous)
    assert all(seen[a, b] == seen[b, a] for a, b in both)


# ------------------------------------------------------------------ 6. the composed route

def test_neighbors_equal_predict_on_a_zero_relation_copy():
    """|E| = 2,000, TransE n = 50: a second engine holds the same entity table and
    a zeroed relation table; its (e, ?, 0) tail queries are the neighbours of e
    in the entity space, e itself included."""
    ne, nr, n, k = 2000, 2, 50, 10
    ent, rel, _ = _random_tables("E", ne, nr, n, seed=8)
    eng = Engine("E", n, ne, nr)
    eng.upload_params(ent, rel)
    zero = Engine("E", n, ne, nr)
    zero.upload_params(ent, np.zeros_like(rel))
    every = np.arange(ne, dtype=np.int32)
    want = zero.predict(every, np.zeros(ne, np.int32), np.ones(ne, np.int32), k)
    got = eng.neighbors(every, k, include_self=True)
    assert _same(got, want)
    c = _counters(eng)
    assert c["candidates"] == ne * ne and c["chunks"] == 1 and c["slices"] == 125 * 2 and c["prunes"] > 0
    # and without the entity itself: the same lists with their first entry (the entity, at +0) taken out
    want11 = zero.predict(every, np.zeros(ne, np.int32), np.ones(ne, np.int32), k + 1)
    ids, dist, found = eng.knn_graph(k)
    assert (want11[0][:, 0] == every).all()
    assert np.array_equal(ids, want11[0][:, 1:]) and np.array_equal(_bits(dist), _bits(want11[1][:, 1:]))
    assert (found == k).all()


# ------------------------------------------------------------------ 7. contract

@pytest.mark.parametrize("model,n", [("E", 20), ("H", 32), ("R", 20)])
def test_neighbors_leave_the_context_unchanged(model, n):
    ds = tiny()
    tables = _random_tables(model, 200, 10, n, seed=11)
    streams = []
    for run in (False, True):
        eng = Engine(model, n, 200, 10, seed=5)
        first = [eng.rng_next() for _ in range(5)]
        if run:
            eng.upload_triples(ds.train)  # (TransR's work vectors exist once the triples are up)
            eng.upload_params(*tables)
            if model == "R":
                eng.set_transr_work(np.arange(n) * 0.5, np.arange(n) * -0.25)
                work = eng.transr_work()
            before = eng.download_params()
            eng.profile(True)
            b0 = eng.device_bytes()
            one = eng.knn_graph(10, relation=4)
            assert eng.device_bytes() == b0
            two = eng.knn_graph(10, relation=4)
            assert eng.device_bytes() == b0
            assert _same(one, two)
            assert _same(eng.neighbors([3, 4], 128, include_self=True), eng.neighbors([3, 4], 128, include_self=True))
            assert eng.device_bytes() == b0
            for fam in ("neighbors_score", "neighbors_merge"):
                ms, cnt = eng.profile_query(fam)
                assert cnt > 0 and ms > 0, fam
            eng.profile(False)
            for a, b in zip(before, eng.download_params()):
                assert (a is None and b is None) or np.array_equal(a, b)
            if model == "R":
                hw, tw = eng.transr_work()
                assert np.array_equal(hw, work[0]) and np.array_equal(tw, work[1])
        streams.append(first + [eng.rng_next() for _ in range(20)])
    assert streams[0] == streams[1]


def test_neighbors_bad_arguments_are_refused():
    ne, nr = 200, 10
    eng = Engine("E", 20, ne, nr)
    eng.upload_params(*_random_tables("E", ne, nr, 20, seed=13))
    b0 = eng.device_bytes()
    eng.neighbors([3], 5)
    assert eng.device_bytes() == b0
    for args, kw in ((([3], 0), {}), (([3], 129), {}), (([3], -1), {}),                   # k out of range
                     ((np.zeros(0, np.int32), 5), {}),                                     # nq < 1
                     (([3], 5), {"include_self": 2}), (([3], 5), {"include_self": -1}),    # include_self
                     (([3], 5), {"relation": nr}), (([3], 5), {"relation": -2}),           # relation
                     (([ne], 5), {}), (([-1], 5), {}), (([3, ne], 5), {})):                # an entity id
        with pytest.raises(EngineError):
            eng.neighbors(*args, **kw)
        assert eng.device_bytes() == b0
    # the C ABI itself: the flag, and NULL arrays with a count > 0
    e = np.array([3], np.int32)
    ids, dist, found = np.zeros(5, np.int32), np.zeros(5), np.zeros(1, np.int32)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    dp = dist.ctypes.data_as(C.POINTER(C.c_double))
    call = lib().kb2e_neighbors
    assert call(eng.h, ip(e), 1, -1, 5, 0, ip(ids), dp, ip(found)) == 0
    assert call(eng.h, ip(e), 1, -1, 5, 2, ip(ids), dp, ip(found)) == 1
    assert call(eng.h, ip(e), 1, -1, 5, -1, ip(ids), dp, ip(found)) == 1
    assert call(eng.h, ip(e), 0, -1, 5, 0, ip(ids), dp, ip(found)) == 1
    assert call(eng.h, None, 1, -1, 5, 0, ip(ids), dp, ip(found)) == 1
    assert call(eng.h, ip(e), 1, -1, 5, 0, None, dp, ip(found)) == 1
    assert call(eng.h, ip(e), 1, -1, 5, 0, ip(ids), None, ip(found)) == 1
    assert call(eng.h, ip(e), 1, -1, 5, 0, ip(ids), dp, None) == 1
    assert eng.device_bytes() == b0
    with pytest.raises(EngineError):
        eng.counter("neighbors_nothing")
    # a context without embeddings is a state error, not a crash
    with pytest.raises(EngineError):
        Engine("E", 20, ne, nr).neighbors([3], 5)
    # still usable
    assert eng.neighbors([3], 5)[2].tolist() == [5]


# ------------------------------------------------------------------ 8. the driver

class _Recording(Engine):
    """An Engine that keeps what neighbors() returned last."""
    last = None

    def neighbors(self, entities, k, relation=-1, include_self=False):
        out = super().neighbors(entities, k, relation=relation, include_self=include_self)
        _Recording.last = (np.asarray(entities).copy(), k, relation, include_self, out)
        return out


@pytest.mark.parametrize("model,relation", [("E", -1), ("H", 3)])
def test_duplicate_detection_counts_what_the_graph_holds(model, relation):
    """A small planted set.  No quality bar: the recalls must be the ones a
    recomputation from Engine.neighbors' raw output gives, and every planted pair
    the driver counts as found must really be mutual."""
    ds = data.synthetic("tiny", seed=4)
    count, k = 20, 5
    res = linkpred.duplicate_detection(ds, model, 16, count, epochs=5, k=k, seed=2, relation=relation, rate=0.01,
                                       batches=10, make_engine=_Recording)
    ents, kk, rel, own, (ids, dist, found) = _Recording.last
    ne = ds.num_entities + count
    assert (kk, rel, bool(own)) == (k, relation, False) and np.array_equal(ents, np.arange(ne))
    assert ids.shape == (ne, k) and (found == k).all()
    pairs = res["pairs"]
    assert np.array_equal(pairs, linkpred.duplicate_split(ds, count, 2)[1])
    hit1 = sum(int(ids[t, 0] == o) for o, t in pairs.tolist())
    hitk = sum(int(o in ids[t, :found[t]].tolist()) for o, t in pairs.tolist())
    print(f"duplicate_detection {model} relation {relation}: recall@1 {hit1}/{count}, recall@{k} {hitk}/{count}, "
          f"mutual {res['mutual']}, planted among them {len(res['mutual_planted'])}, baseline {res['baseline']:.4f}")
    assert res["recall@1"] == hit1 / count and res["recall@k"] == hitk / count
    assert res["baseline"] == k / (ne - 1) and res["entities"] == ne and res["planted"] == count
    lists = [set(ids[a, :found[a]].tolist()) for a in range(ne)]
    mutual = {(a, b) for a in range(ne) for b in lists[a] if a < b and a in lists[b]}
    assert res["mutual"] == len(mutual)
    planted = {(o, t) for o, t in pairs.tolist()}
    assert set(res["mutual_planted"]) == mutual & planted
    assert res["mutual_share"] == (len(mutual & planted) / len(mutual) if mutual else None)


# ------------------------------------------------------------------ 9. CLI

def test_neighbors_cli_matches_engine(tmp_path):
    name = "transe_l1_bern"
    f = MANIFEST["runs"][name]["flags"]
    ds = tiny()
    d = os.path.join(GOLDEN, name)
    exe = tmp_path / "neighborsTransE"
    exe.symlink_to(os.path.join(ROOT, "bin", "kb2e"))
    base = [str(exe), "--datadir", os.path.join(GOLDEN, "tiny"), "--outdir", d, "--size", str(f["size"]), "--method",
            str(f["method"]), "--distance", str(f["distance"])]
    eng = Engine("E", f["size"], ds.num_entities, ds.num_relations, distance=f["distance"])
    eng.upload_params(data.read_table(os.path.join(d, "entity2vec.bern"), ds.num_entities, f["size"]),
                      data.read_table(os.path.join(d, "relation2vec.bern"), ds.num_relations, f["size"]))
    names = {v: k for k, v in data._load_ids(os.path.join(GOLDEN, "tiny", "entity2id.txt")).items()}
    rnames = {v: k for k, v in data._load_ids(os.path.join(GOLDEN, "tiny", "relation2id.txt")).items()}
    every = np.arange(ds.num_entities, dtype=np.int32)

    def lines(extra, tabs):
        res = subprocess.run(base + extra, capture_output=True, text=True, timeout=300, check=True)
        return res.stdout, [l for l in res.stdout.splitlines() if l.count("\t") == tabs]

    # the graph
    _, got = lines(["--all", "--topk", "5"], 3)
    ids, dist, found = eng.neighbors(every, 5)
    want = ["%s\t%d\t%s\t%.6f" % (names[a], j + 1, names[int(ids[a, j])], dist[a, j])
            for a in range(ds.num_entities) for j in range(found[a])]
    assert len(want) == 5 * ds.num_entities and got == want
    # its mutual pairs
    _, got = lines(["--all", "--topk", "5", "--pairs"], 2)
    pairs, pd = linkpred.mutual_pairs(ids, dist, found)
    assert len(pairs) > 0
    assert got == ["%s\t%s\t%.6f" % (names[a], names[b], x) for (a, b), x in zip(pairs.tolist(), pd.tolist())]
    # listed entities (one unknown name, one twice), a relation's space, the entity itself included
    entfile = tmp_path / "entities.txt"
    entfile.write_text(f"{names[7]}\n/m/nothing\n{names[150]}\n{names[7]}\n")
    out, got = lines(["--entities", str(entfile), "--topk", "3", "--relation", rnames[6], "--self"], 3)
    assert "Entity found in triple file that was not found in the identity file: /m/nothing" in out
    q = [7, 150, 7]
    ids, dist, found = eng.neighbors(q, 3, relation=6, include_self=True)
    assert got == ["%s\t%d\t%s\t%.6f" % (names[a], j + 1, names[int(ids[i, j])], dist[i, j])
                   for i, a in enumerate(q) for j in range(found[i])]
    # neither --entities nor --all
    assert subprocess.run(base + ["--topk", "3"], capture_output=True, text=True, timeout=300).returncode == 1
