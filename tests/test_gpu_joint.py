"""Conjunctive queries (kb2e_predict_joint, kb2e_rank_joint) against the oracle.

The oracle is plain numpy over orc.Model(..., transr_compat=False).energy: for
each candidate a Python left-to-right float sum of its energies over the query's
constraints, the candidates whose triples are all in the filter dropped,
np.lexsort((ids, energy)), the first k.  All device arithmetic is FP64 in the
reference's order, the sum runs in the caller's order and ties break on the
entity id, so ids, energies, found counts and ranks must be EQUAL (no tolerance
anywhere in this file; the CLI's printed %.6lf is compared as text).
"""
import ctypes as C
import functools
import operator
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


# ------------------------------------------------------------------ helpers

def _tables(model, ds, n, seed, scale=0.3):
    """tests/test_gpu_predict.py _tables' recipe."""
    rng = np.random.default_rng(seed)
    if model == "R":
        ent = rng.standard_normal((ds.num_entities, n))
        ent /= np.linalg.norm(ent, axis=1, keepdims=True)
        rel = rng.standard_normal((ds.num_relations, n)) * scale
        w = np.eye(n)[None] + rng.standard_normal((ds.num_relations, n, n)) * (scale / np.sqrt(n))
        return ent, rel, w
    ent = rng.standard_normal((ds.num_entities, n)) * 0.2
    rel = rng.standard_normal((ds.num_relations, n)) * 0.2
    w = None
    if model == "H":
        w = rng.standard_normal((ds.num_relations, n))
        w /= np.linalg.norm(w, axis=1, keepdims=True)
    return ent, rel, w


def _f32(tables):
    return tuple(None if t is None else t.astype(np.float32).astype(np.float64) for t in tables)


def _q(*rows):
    return np.array(rows, np.int32).reshape(-1, 3)


class Setup:
    """An engine and the oracle on the same tables; oracle rows (the energies of
    all candidates of one constraint) are memoised and never modified."""

    def __init__(self, model, n, ds, *, distance=0, precision=64, seed=0, tables=None, **kw):
        self.ds, self.ne, self.nr = ds, ds.num_entities, ds.num_relations
        self.tables = _tables(model, ds, n, seed) if tables is None else tables
        self.eng = Engine(model, n, ds.num_entities, ds.num_relations, distance=distance, precision=precision, **kw)
        self.eng.upload_params(*self.tables)
        self.m = orc.Model(model, n, ds.num_entities, ds.num_relations, distance=distance, transr_compat=False)
        self.m.set_tables(*(_f32(self.tables) if precision == 32 else self.tables))
        self.filt = np.concatenate([ds.train, ds.valid, ds.test])
        self._rows = {}
        self._known = None

    def row(self, e, r, side):
        key = (int(e), int(r), int(side))
        if key not in self._rows:
            e, r, side = key
            row = np.array([self.m.energy(e, x, r) if side else self.m.energy(x, e, r) for x in range(self.ne)])
            row.setflags(write=False)
            self._rows[key] = row
        return self._rows[key]

    def known(self, filt):
        if filt is None:
            return frozenset()
        if self._known is None or self._known[0] is not filt:
            self._known = (filt, frozenset(map(tuple, np.asarray(filt).tolist())))
        return self._known[1]

    def joint(self, query):
        """energy float64[ne] of one query: per candidate a Python left-to-right float
        sum in the caller's order."""
        cols = np.stack([self.row(*c) for c in np.asarray(query).tolist()], axis=1).tolist()
        return np.array([functools.reduce(operator.add, c) for c in cols])

    def excluded(self, query, filt):
        known = self.known(filt)
        out = np.zeros(self.ne, bool)
        if not known:
            return out
        cons = np.asarray(query).tolist()
        for x in range(self.ne):
            out[x] = all(((e, x, r) if side else (x, e, r)) in known for e, r, side in cons)
        return out

    def expect(self, queries, k, filt=None):
        ids = np.full((len(queries), k), -1, np.int32)
        en = np.full((len(queries), k), np.inf)
        found = np.zeros(len(queries), np.int32)
        for q, query in enumerate(queries):
            row = self.joint(query)
            keep = ~self.excluded(query, filt)
            cand = np.arange(self.ne)[keep]
            order = np.lexsort((cand, row[keep]))[:k]
            found[q] = len(order)
            ids[q, :len(order)] = cand[order]
            en[q, :len(order)] = row[keep][order]
        return ids, en, found

    def expect_ranks(self, queries, truth, filt):
        ranks = np.zeros((len(queries), 2), np.int64)
        for q, query in enumerate(queries):
            row = self.joint(query)
            above = row < row[truth[q]]
            ranks[q, 0] = 1 + above.sum()
            ex = self.excluded(query, filt)
            ex[truth[q]] = False
            ranks[q, 1] = 1 + (above & ~ex).sum()
        return ranks

    def check(self, queries, k, filt=None):
        ids, en, found = self.eng.predict_joint(queries, k, filt)
        xi, xe, xf = self.expect(queries, k, filt)
        assert ids.shape == (len(queries), k) and ids.dtype == np.int32 and en.dtype == np.float64
        assert np.array_equal(found, xf)
        assert np.array_equal(ids, xi)
        assert np.array_equal(en, xe)
        return ids, en, found

    def check_ranks(self, queries, truth, filt):
        ranks = self.eng.rank_joint(queries, truth, filt)
        assert ranks.shape == (len(queries), 2) and ranks.dtype == np.int64
        exp = self.expect_ranks(queries, truth, filt)
        assert np.array_equal(ranks, exp)
        return ranks


def _mention_queries(ds, count, ms=(1, 2, 3)):
    """Queries from test triples that share an entity (linkpred.identification_queries),
    their sizes cycling through `ms`: (truth entities, queries)."""
    ents, patterns = linkpred.identification_queries(ds.test, max(ms))
    ents, patterns = ents[:count], patterns[:count]
    return ents, [p[:ms[i % len(ms)]] for i, p in enumerate(patterns)]


def _random_query(rng, ds, m, relation=None):
    return np.stack([rng.integers(0, ds.num_entities, m),
                     np.full(m, relation) if relation is not None else rng.integers(0, ds.num_relations, m),
                     rng.integers(0, 2, m)], axis=1).astype(np.int32)


def _ds70():
    return data.synthetic("small", seed=4, counts=(70, 3, 400, 20, 20))


def _ds2085():
    return data.synthetic("small", seed=4, counts=(2085, 7, 3000, 50, 50))


@pytest.fixture(scope="module")
def tiny_e():
    return Setup("E", 20, tiny(), seed=1)


@pytest.fixture(scope="module")
def e70():
    return Setup("E", 20, _ds70(), seed=2)


@pytest.fixture(scope="module")
def e2085():
    return Setup("E", 20, _ds2085(), seed=3)


# ------------------------------------------------------------------ 1. models and precisions

@pytest.mark.parametrize("model,distance,precision", [("E", 0, 64), ("E", 1, 64), ("H", 0, 64), ("R", 0, 64), ("R", 1, 64),
                                                      ("E", 0, 32), ("H", 0, 32), ("R", 0, 32)])
def test_joint_models_tiny(model, distance, precision):
    """E / H / R at n = 20 on the golden tiny set: 24 queries from test triples that
    share an entity, m in {1, 2, 3} mixed in one call, raw and filtered."""
    s = Setup(model, 20, tiny(), distance=distance, precision=precision, seed=5 + distance)
    ents, queries = _mention_queries(s.ds, 24)
    assert len(queries) == 24 and sorted({len(q) for q in queries}) == [1, 2, 3]
    s.check(queries, 10)
    _, _, found = s.check(queries, s.ne, s.filt)
    # the entity behind a query is a known answer to all of its patterns
    assert (found < s.ne).all()
    raw = s.check_ranks(queries, ents, None)
    assert np.array_equal(raw[:, 0], raw[:, 1])
    s.check_ranks(queries, ents, s.filt)
    s.eng.close()


# ------------------------------------------------------------------ 2. m = 1 is kb2e_predict

def test_joint_single_constraint_equals_predict(tiny_e):
    s = tiny_e
    pick = s.ds.test[:30]
    e = np.concatenate([pick[:, 0], pick[:, 1]]).astype(np.int32)
    r = np.concatenate([pick[:, 2], pick[:, 2]]).astype(np.int32)
    side = np.array([1] * 30 + [0] * 30, np.int32)
    queries = [_q((e[i], r[i], side[i])) for i in range(60)]
    for filt in (None, s.filt):
        for k in (1, 10, 300):
            a = s.eng.predict_joint(queries, k, filt)
            b = s.eng.predict(e, r, side, k, filt)
            for x, y in zip(a, b):
                assert x.dtype == y.dtype and np.array_equal(x, y)
    ranks = s.eng.rank_triples(pick, s.filt)  # head raw, head filtered, tail raw, tail filtered
    truth = np.concatenate([pick[:, 1], pick[:, 0]]).astype(np.int32)
    joint = s.eng.rank_joint(queries, truth, s.filt)
    assert np.array_equal(joint[:30], ranks[:, 2:4]) and np.array_equal(joint[30:], ranks[:, 0:2])
    assert (joint[:, 1] < joint[:, 0]).any()  # (the filter bites)


# ------------------------------------------------------------------ 3. entity-count and m edges

@pytest.mark.parametrize("which", ["e70", "e2085"])
def test_joint_entity_count_and_constraint_count_edges(which, request):
    """70 entities: fewer than one block of 256; 2,085: eight blocks and a ragged
    one.  m = 17 on one relation: the query's rows straddle a 16-row score tile;
    m = 64: the limit; mixed sizes around them in one call."""
    s = request.getfixturevalue(which)
    rng = np.random.default_rng(11)
    ents, mention = _mention_queries(s.ds, 6, ms=(2, 1))
    queries = [_random_query(rng, s.ds, 17, relation=1), mention[0], _random_query(rng, s.ds, 64), mention[1],
               _random_query(rng, s.ds, 17), _random_query(rng, s.ds, 16, relation=0), mention[2],
               _random_query(rng, s.ds, 33, relation=2)]
    s.check(queries, 10)
    s.check(queries, 10, s.filt)
    truth = np.array([3, ents[0], s.ne - 1, ents[1], 0, 5, ents[2], s.ne // 2], np.int32)
    s.check_ranks(queries, truth, s.filt)
    b0 = s.eng.device_bytes()
    with pytest.raises(EngineError):
        s.eng.predict_joint([_random_query(rng, s.ds, 65)], 10)
    with pytest.raises(EngineError):
        s.eng.rank_joint([mention[0], _random_query(rng, s.ds, 65)], [0, 1], s.filt)
    assert s.eng.device_bytes() == b0


# ------------------------------------------------------------------ 4. chunking

def test_joint_chunked_row_buffer(tiny_e, monkeypatch):
    """KB2E_JOINT_CHUNK_ROWS=5 with m = [1, 2, 3, 5, 4, 1, 1, 3]: the chunks are
    [1,2] [3] [5] [4,1] [1,3]; a query is never split; the answers do not change."""
    s = tiny_e
    rng = np.random.default_rng(21)
    ms = [1, 2, 3, 5, 4, 1, 1, 3]
    queries = [_random_query(rng, s.ds, m) for m in ms]
    truth = rng.integers(0, s.ne, len(ms)).astype(np.int32)
    whole = s.eng.predict_joint(queries, 10, s.filt)
    whole_ranks = s.eng.rank_joint(queries, truth, s.filt)
    assert s.eng.counter("joint_chunks") == 1 and s.eng.counter("joint_rows") == 20
    distinct = len({int(r) for q in queries for r in q[:, 1]})
    assert s.eng.counter("joint_projections") == distinct
    monkeypatch.setenv("KB2E_JOINT_CHUNK_ROWS", "5")
    chunks = [queries[0:2], queries[2:3], queries[3:4], queries[4:6], queries[6:8]]
    per_chunk = sum(len({int(r) for q in ch for r in q[:, 1]}) for ch in chunks)
    for call in (lambda: s.eng.predict_joint(queries, 10, s.filt), lambda: s.eng.rank_joint(queries, truth, s.filt)):
        got = call()
        assert s.eng.counter("joint_chunks") == 5
        assert s.eng.counter("joint_rows") == 20
        assert distinct <= s.eng.counter("joint_projections") <= per_chunk
        if isinstance(got, tuple):
            for x, y in zip(got, whole):
                assert np.array_equal(x, y)
        else:
            assert np.array_equal(got, whole_ranks)
    s.check(queries, 10, s.filt)
    # the budget rises to the largest query
    monkeypatch.setenv("KB2E_JOINT_CHUNK_ROWS", "1")
    three = [queries[2], queries[0], queries[5]]
    s.check(three, 10, s.filt)
    assert s.eng.counter("joint_chunks") == 2 and s.eng.counter("joint_rows") == 5


# ------------------------------------------------------------------ 5. exclusion

def test_joint_exclusion_needs_every_constraint(tiny_e):
    s = tiny_e
    ne = s.ne
    query = _q((3, 1, 1), (8, 2, 0))  # x is the tail of (3, x, r1) and the head of (x, 8, r2)
    # 20 is known for the first pattern only, 21 for the second only, 22 and 23 for both
    filt = np.array([(3, 20, 1), (21, 8, 2), (3, 22, 1), (22, 8, 2), (3, 23, 1), (23, 8, 2), (22, 3, 1), (8, 22, 2)],
                    np.int32)
    ids, _, found = s.check([query], ne, filt)
    assert found[0] == ne - 2
    kept = set(ids[0, :found[0]].tolist())
    assert 20 in kept and 21 in kept and 22 not in kept and 23 not in kept
    # a filter triple listed twice changes nothing
    twice = np.concatenate([filt, filt[2:4], filt[:1]])
    for x, y in zip(s.eng.predict_joint([query], ne, twice), s.expect([query], ne, filt)):
        assert np.array_equal(x, y)
    # with one pattern the rule is kb2e_predict's
    ids1, _, found1 = s.check([query[:1]], ne, filt)
    assert found1[0] == ne - 3 and not {20, 22, 23} & set(ids1[0, :found1[0]].tolist())
    # every candidate known: nothing is found
    full = np.array([(3, x, 1) for x in range(ne)] + [(x, 8, 2) for x in range(ne)], np.int32)
    other = _q((5, 0, 1))
    ids, en, found = s.check([query, other, query[::-1]], 7, full)
    assert found.tolist() == [0, 7, 0]
    assert (ids[0] == -1).all() and np.isinf(en[0]).all() and (ids[2] == -1).all() and np.isinf(en[2]).all()
    # the truth is never excluded, the other excluded candidates are
    ranks = s.check_ranks([query, query, query], [22, 20, 40], filt)
    row = s.joint(query)
    for i, tr in enumerate((22, 20, 40)):
        assert ranks[i, 0] - ranks[i, 1] == sum(row[x] < row[tr] for x in (22, 23) if x != tr)
    ranks = s.check_ranks([query], [22], full)
    assert ranks[0, 1] == 1


# ------------------------------------------------------------------ 6. duplicates and ties

def test_joint_duplicated_constraint_and_ties():
    ds = tiny()
    ent, rel, _ = _tables("E", ds, 20, 31)
    group = [4, 9, 17, 33, 58, 120]
    ent[group] = ent[4]  # identical rows: identical energies wherever they are candidates
    s = Setup("E", 20, ds, tables=(ent, rel, None))
    c = (7, 3, 1)
    ids1, en1, found1 = s.eng.predict_joint([_q(c)], s.ne)
    ids2, en2, found2 = s.check([_q(c, c)], s.ne)
    assert found1[0] == s.ne and found2[0] == s.ne
    e1 = np.empty(s.ne)
    e1[ids1[0]] = en1[0]
    assert np.array_equal(en2[0], e1[ids2[0]] + e1[ids2[0]])
    # the tie group comes out in id order, inside a k that is larger than it
    query = _q((7, 3, 1), (12, 5, 0), (7, 3, 1))
    ids, en, _ = s.check([query], s.ne)
    pos = [int(np.nonzero(ids[0] == x)[0][0]) for x in group]
    assert pos == list(range(pos[0], pos[0] + len(group)))
    assert len(set(en[0, pos].tolist())) == 1
    k = pos[0] + len(group) + 2
    s.check([query], k)
    s.check([query], pos[0] + 2)  # (and a k that cuts the group)
    ranks = s.check_ranks([query] * 2, [group[0], group[-1]], None)
    assert ranks[0, 0] == ranks[1, 0] == pos[0] + 1  # ties are not counted above the truth
    s.eng.close()


# ------------------------------------------------------------------ 7. k edges

def test_joint_k_edges(e70):
    s = e70
    _, queries = _mention_queries(s.ds, 5)
    for k in (1, 100, 1024):
        ids, en, found = s.check(queries, k, s.filt)
        assert (found <= min(k, 70)).all()
        if k > 70:
            assert (ids[:, 70:] == -1).all() and np.isinf(en[:, 70:]).all()


# ------------------------------------------------------------------ 8. wide rows

@pytest.mark.parametrize("rows_l2", ["0", "1"])
@pytest.mark.parametrize("model", ["E", "H", "R"])
def test_joint_wide_rows(model, rows_l2, monkeypatch):
    """n = 260, and KB2E_EVAL_ROWS_L2=1: the score kernel reads the constraint rows
    from the projection table instead of LDS."""
    monkeypatch.setenv("KB2E_EVAL_ROWS_L2", rows_l2)
    s = Setup(model, 260, _ds70(), seed=41)
    ents, queries = _mention_queries(s.ds, 6)
    s.check(queries, 10, s.filt)
    s.check_ranks(queries, ents, s.filt)
    s.eng.close()


# ------------------------------------------------------------------ 9. contract

def _raw_predict_joint(eng, offsets, rows, k):
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    rows = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1, 3)
    cols = [np.ascontiguousarray(rows[:, c]) for c in range(3)]
    nq = len(offsets) - 1
    ids = np.zeros((nq, k), np.int32)
    en = np.zeros((nq, k))
    found = np.zeros(nq, np.int32)
    i32p = C.POINTER(C.c_int32)
    return lib().kb2e_predict_joint(eng.h, offsets.ctypes.data_as(C.POINTER(C.c_int64)),
                                    *[c.ctypes.data_as(i32p) for c in cols], nq, k, None, None, None, 0,
                                    ids.ctypes.data_as(i32p), en.ctypes.data_as(C.POINTER(C.c_double)),
                                    found.ctypes.data_as(i32p))


def test_joint_bad_arguments_are_refused(tiny_e):
    s = tiny_e
    eng, ne, nr = s.eng, s.ne, s.nr
    b0 = eng.device_bytes()
    good = _q((3, 1, 1), (8, 2, 0))
    rows = np.concatenate([good, good])
    assert _raw_predict_joint(eng, [0, 2, 4], rows, 5) == 0
    EINVAL = 1
    for offsets in ([1, 2, 4], [0, 2, 2], [0, 0, 4], [0, 3, 2], [-1, 2, 4]):
        assert _raw_predict_joint(eng, offsets, rows, 5) == EINVAL, offsets
        assert eng.device_bytes() == b0
    assert _raw_predict_joint(eng, [0, 65], np.tile(good[:1], (65, 1)), 5) == EINVAL
    assert _raw_predict_joint(eng, [0, 64], np.tile(good[:1], (64, 1)), 5) == 0
    bad_filters = [np.array([t], np.int32) for t in ((0, ne, 0), (-1, 1, 0), (0, 1, nr), (0, 1, -1))]
    for queries, k, filt in (([good], 0, None), ([good], 1025, None), ([good], -1, None),
                             ([np.zeros((0, 3), np.int32)], 5, None), ([good, np.zeros((0, 3), np.int32)], 5, None),
                             ([], 5, None),
                             ([_q((3, 1, 2))], 5, None), ([_q((3, 1, -1))], 5, None), ([good, _q((3, 1, 1), (3, 1, 2))], 5, None),
                             ([_q((ne, 1, 1))], 5, None), ([_q((-1, 1, 1))], 5, None), ([_q((3, nr, 1))], 5, None),
                             ([_q((3, -1, 0))], 5, None), ([good, _q((3, 1, 1), (ne, 1, 0))], 5, None),
                             *[([good], 5, f) for f in bad_filters]):
        with pytest.raises(EngineError, match="EINVAL"):
            eng.predict_joint(queries, k, filt)
        assert eng.device_bytes() == b0
    for queries, truth, filt in (([good], [ne], None), ([good], [-1], None), ([good, good], [0, ne], s.filt),
                                 ([_q((3, 1, 2))], [0], None), ([_q((ne, 1, 1))], [0], None),
                                 ([np.zeros((0, 3), np.int32)], [0], None), ([], [], None),
                                 *[([good], [0], f) for f in bad_filters]):
        with pytest.raises(EngineError, match="EINVAL"):
            eng.rank_joint(queries, truth, filt)
        assert eng.device_bytes() == b0
    # still usable
    s.check([good], 5, s.filt)
    fresh = Engine("E", 20, ne, nr)
    with pytest.raises(EngineError, match="ESTATE"):
        fresh.predict_joint([good], 5)
    with pytest.raises(EngineError, match="ESTATE"):
        fresh.rank_joint([good], [0], None)
    fresh.close()


@pytest.mark.parametrize("model", ["E", "H", "R"])
def test_joint_calls_leave_the_context_unchanged(model):
    """Tables, the glibc stream, the TransR work vectors and device_bytes() are the
    same after the calls, refused ones included; the five profile families report."""
    ds = tiny()
    n = 20
    tables = _tables(model, ds, n, 51)
    ents, queries = _mention_queries(ds, 12)
    filt = np.concatenate([ds.train, ds.valid, ds.test])
    streams = []
    for run in (False, True):
        eng = Engine(model, n, ds.num_entities, ds.num_relations, seed=5)
        first = [eng.rng_next() for _ in range(5)]
        eng.upload_triples(ds.train)  # (TransR's work vectors exist once the triples are up)
        eng.upload_params(*tables)
        if model == "R":
            eng.set_transr_work(np.arange(n) * 0.5, np.arange(n) * -0.25)
        if run:
            before = eng.download_params()
            work = eng.transr_work() if model == "R" else None
            eng.profile(True)
            b0 = eng.device_bytes()
            eng.predict_joint(queries, 10, filt)
            assert eng.device_bytes() == b0
            eng.predict_joint(queries, 10)
            assert eng.device_bytes() == b0
            eng.rank_joint(queries, ents, filt)
            assert eng.device_bytes() == b0
            for refused in (lambda: eng.predict_joint(queries, 0), lambda: eng.predict_joint([_q((3, 1, 2))], 5),
                            lambda: eng.rank_joint(queries[:1], [ds.num_entities], filt)):
                with pytest.raises(EngineError):
                    refused()
                assert eng.device_bytes() == b0
            for fam in ("joint_score", "joint_combine", "joint_mask", "joint_select", "joint_rank"):
                ms, cnt = eng.profile_query(fam)
                assert cnt > 0 and ms > 0, fam
            eng.profile(False)
            after = eng.download_params()
            for a, b in zip(before, after):
                assert (a is None and b is None) or np.array_equal(a, b)
            if model == "R":
                hw, tw = eng.transr_work()
                assert np.array_equal(hw, work[0]) and np.array_equal(tw, work[1])
        streams.append(first + [eng.rng_next() for _ in range(20)])
        eng.close()
    assert streams[0] == streams[1]


# ------------------------------------------------------------------ 10. consistency

@pytest.mark.parametrize("model,n,distance", [("E", 50, 1), ("H", 32, 0), ("R", 20, 0)])
def test_joint_energies_are_sums_of_score_triples_bits(model, n, distance):
    s = Setup(model, n, tiny(), distance=distance, seed=61)
    _, queries = _mention_queries(s.ds, 9)
    ids, en, found = s.eng.predict_joint(queries, 8)
    assert (found == 8).all()
    for q, query in enumerate(queries):
        total = None
        for e, r, side in query.tolist():
            trip = np.array([(e, x, r) if side else (x, e, r) for x in ids[q].tolist()], np.int32)
            part = s.eng.score(trip)
            total = part if total is None else total + part
        assert np.array_equal(total, en[q])
    s.eng.close()


def test_entity_identification_matches_oracle_ranks(tiny_e):
    s = tiny_e
    res = linkpred.entity_identification(s.eng, s.ds, constraints=(1, 3))
    ents, patterns = linkpred.identification_queries(s.ds.test, 3)
    assert res[1]["count"] == res[3]["count"] == len(ents) == 46
    for m in (1, 3):
        exp = s.expect_ranks([p[:m] for p in patterns], ents, s.filt)
        assert res[m]["raw"]["mean_rank"] == exp[:, 0].mean() and res[m]["filtered"]["mean_rank"] == exp[:, 1].mean()
        assert res[m]["filtered"]["mrr"] == (1.0 / exp[:, 1]).mean()
        assert res[m]["filtered"]["hits@10"] == (exp[:, 1] <= 10).mean()


# ------------------------------------------------------------------ 11. CLI

def test_joint_cli_matches_engine(tmp_path):
    name = "transe_l1_bern"
    f = MANIFEST["runs"][name]["flags"]
    ds = tiny()
    d = os.path.join(GOLDEN, name)
    qfile = tmp_path / "queries.txt"
    # "b" holds an unknown entity and is dropped whole; "a" comes back later as a new query;
    # "d" has a line without a ? and is dropped; "e" is one pattern
    qfile.write_text("a\t/m/e25\t?\t/r/r4\na\t?\t/m/e58\t/r/r1\n"
                     "b\t/m/e3\t?\t/r/r0\nb\t/m/nobody\t?\t/r/r1\nb\t?\t/m/e7\t/r/r2\n"
                     "c\t?\t/m/e105\t/r/r0\nc\t/m/e114\t?\t/r/r4\nc\t/m/e25\t?\t/r/r4\n"
                     "a\t/m/e9\t?\t/r/r3\n"
                     "d\t/m/e1\t/m/e2\t/r/r3\nd\t/m/e1\t?\t/r/r3\n"
                     "e\t?\t/m/e30\t/r/r2\n")
    tokens = ["a", "c", "a", "e"]
    queries = [_q((25, 4, 1), (58, 1, 0)), _q((105, 0, 0), (114, 4, 1), (25, 4, 1)), _q((9, 3, 1)), _q((30, 2, 0))]
    exe = tmp_path / "jointTransE"
    exe.symlink_to(os.path.join(ROOT, "bin", "kb2e"))
    base = [str(exe), "--datadir", os.path.join(GOLDEN, "tiny"), "--outdir", d, "--size", str(f["size"]), "--method",
            str(f["method"]), "--distance", str(f["distance"]), "--queries", str(qfile)]
    eng = Engine("E", f["size"], ds.num_entities, ds.num_relations, distance=f["distance"])
    eng.upload_params(data.read_table(os.path.join(d, "entity2vec.bern"), ds.num_entities, f["size"]),
                      data.read_table(os.path.join(d, "relation2vec.bern"), ds.num_relations, f["size"]))
    names = {v: k for k, v in data._load_ids(os.path.join(GOLDEN, "tiny", "entity2id.txt")).items()}
    assert names[25] == "/m/e25"
    filt = np.concatenate([ds.test, ds.train, ds.valid])
    for extra, k, fl in (([], 10, filt), (["--topk", "3", "--filtered", "0"], 3, None)):
        res = subprocess.run(base + extra, capture_output=True, text=True, timeout=300, check=True)
        assert "Head entity found in triple file that was not found in the identity file: /m/nobody" in res.stdout
        assert "Query needs exactly one ? in the head or the tail column: /m/e1 /m/e2" in res.stdout
        rows = [l.split("\t") for l in res.stdout.splitlines() if l.count("\t") == 3]
        ids, en, found = eng.predict_joint(queries, k, fl)
        assert (found == k).all()
        expect = [[tokens[q], str(j + 1), names[int(ids[q, j])], "%.6f" % en[q, j]]
                  for q in range(len(queries)) for j in range(found[q])]
        assert rows == expect
    eng.close()
