"""Knowledge-base completion (kb2e_complete_triples) against the oracle.

The oracle for a relation r is plain numpy over orc.Model(..., transr_compat=
False).energy of every candidate pair (h, t): the known pairs (and, where asked,
the loops h == t) dropped, np.lexsort((tails, heads, energy)), the first k.  All
device arithmetic is FP64 in the reference's order and ties break on the head
id, then on the tail id, so heads, tails, energy bits and found counts must be
EQUAL (no tolerance anywhere in this file except where a printed %.6lf is
compared).
"""
import itertools
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from gpu_common import MANIFEST, tiny
from kb2e_amd import data, linkpred
from kb2e_amd.engine import Engine, EngineError
from oracle import orc

pytestmark = pytest.mark.gpu


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


def _all_pairs(ne, r):
    h, t = np.divmod(np.arange(ne * ne, dtype=np.int64), ne)
    return np.stack([h, t, np.full(ne * ne, r)], 1).astype(np.int32)


def _expect_one(E, r, k, known, constrained, exclude_loops):
    """The oracle's answer for relation r from its energy matrix E[h, t]."""
    ne = E.shape[0]
    kn = np.zeros((0, 3), np.int64) if known is None else np.asarray(known, dtype=np.int64).reshape(-1, 3)
    kn = kn[kn[:, 2] == r]
    hl = np.unique(kn[:, 0]) if constrained else np.arange(ne)
    tl = np.unique(kn[:, 1]) if constrained else np.arange(ne)
    H, T = (a.reshape(-1) for a in np.meshgrid(hl, tl, indexing="ij"))
    is_known = np.zeros((ne, ne), bool)
    is_known[kn[:, 0], kn[:, 1]] = True
    keep = ~is_known[H, T]
    if exclude_loops:
        keep &= H != T
    H, T = H[keep], T[keep]
    e = E[H, T]
    order = np.lexsort((T, H, e))[:k]
    heads = np.full(k, -1, np.int32)
    tails = np.full(k, -1, np.int32)
    en = np.full(k, np.inf)
    heads[:len(order)], tails[:len(order)], en[:len(order)] = H[order], T[order], e[order]
    return heads, tails, en, len(order)


class Setup:
    """An engine and the oracle on the same tables.  The energy matrix of a
    relation is computed once -- from the oracle for the relations in `oracle`,
    from Engine.score (pinned to the oracle by tests/test_gpu_predict.py) for
    the others -- and never modified."""

    def __init__(self, model, n, ne, nr, tables, *, distance=0, precision=64, oracle=()):
        self.ne, self.nr = ne, nr
        self.eng = Engine(model, n, ne, nr, distance=distance, precision=precision)
        self.eng.upload_params(*tables)
        self.m = orc.Model(model, n, ne, nr, distance=distance, transr_compat=False)
        self.m.set_tables(*(_f32(tables) if precision == 32 else tables))
        self.from_oracle = set(oracle)
        self._E = {}

    def energies(self, r):
        if r not in self._E:
            if r in self.from_oracle:
                E = np.array([self.m.energy(h, t, r) for h in range(self.ne) for t in range(self.ne)])
            else:
                E = self.eng.score(_all_pairs(self.ne, r))
            E = E.reshape(self.ne, self.ne)
            E.setflags(write=False)
            self._E[r] = E
        return self._E[r]

    def expect(self, rels, k, known=None, constrained=False, exclude_loops=False):
        rows = [_expect_one(self.energies(int(r)), int(r), k, known, constrained, exclude_loops) for r in rels]
        return (np.stack([x[0] for x in rows]), np.stack([x[1] for x in rows]), np.stack([x[2] for x in rows]),
                np.array([x[3] for x in rows], np.int64))

    def check(self, rels, k, known=None, constrained=False, exclude_loops=False):
        got = self.eng.complete(rels, k, known, constrained=constrained, exclude_loops=exclude_loops)
        exp = self.expect(rels, k, known, constrained, exclude_loops)
        heads, tails, en, found = got
        assert heads.shape == tails.shape == en.shape == (len(rels), k)
        assert heads.dtype == tails.dtype == np.int32 and en.dtype == np.float64 and found.dtype == np.int64
        assert np.array_equal(found, exp[3])
        assert np.array_equal(heads, exp[0])
        assert np.array_equal(tails, exp[1])
        assert np.array_equal(en.view(np.uint64), exp[2].view(np.uint64))  # the bits (+inf padding included)
        return got


def _same(a, b):
    return all(np.array_equal(x.view(np.uint64) if x.dtype == np.float64 else x,
                              y.view(np.uint64) if y.dtype == np.float64 else y) for x, y in zip(a, b))


def _counters(eng):
    return {c: eng.counter("complete_" + c) for c in ("candidates", "records", "strips", "buffer_records")}


def _golden_tables(name):
    """The trained tables of a golden run, after its last epoch."""
    run = MANIFEST["runs"][name]
    d = os.path.join(GOLDEN, name)
    last = run["flags"]["epochs"] - 1
    ent = np.load(os.path.join(d, f"epoch{last}_ent.npy"))
    rel = np.load(os.path.join(d, f"epoch{last}_rel.npy"))
    w = np.load(os.path.join(d, f"epoch{last}_w.npy")) if run["model"] != "E" else None
    return run, (ent, rel, w)


# ------------------------------------------------------------------ 1. oracle, tiny set

@pytest.mark.parametrize("name", ["transe_l1_bern", "transe_l2_unif", "transh_bern", "transr_fixed"])
def test_complete_golden_models_against_oracle(name):
    """The golden-trained tables of one run per model (E L1, E L2, H, R); all 10
    relations of the 200-entity set in one call, relations 2 and 7 against the
    oracle's 40,000 energies each, the others against the same sort over
    Engine.score; k = 1, 10, 1024; filtered and not; constrained and not; loops
    excluded and not."""
    run, tables = _golden_tables(name)
    ds = tiny()
    assert (ds.num_entities, ds.num_relations) == (200, 10)
    f = run["flags"]
    s = Setup(run["model"], f["size"], 200, 10, tables, distance=f["distance"], oracle=(2, 7))
    for r in (2, 7):  # (the two routes to an energy matrix agree, so the other eight stand on the oracle too)
        assert np.array_equal(s.energies(r).reshape(-1), s.eng.score(_all_pairs(200, r)))
    known = np.concatenate([ds.train, ds.valid, ds.test])
    rels = np.arange(10, dtype=np.int32)
    for k, kn, constrained, loops in itertools.product((1, 10, 1024), (None, known), (False, True), (False, True)):
        _, _, _, found = s.check(rels, k, kn, constrained, loops)
        if constrained:
            assert (found == 0).all() == (kn is None)  # (no known triple: every pool is empty)
        else:
            assert (found == k).all()


# ------------------------------------------------------------------ 2. shapes

KNOBS = [
    # 65,536 records < 90,000 pairs; strips of 32 heads: 1 + 9 strips, the last with 28 heads
    {"KB2E_COMPLETE_STRIP_HEADS": "32", "KB2E_COMPLETE_BUFFER_BYTES": str(1 << 20)},
    # 5,000 records: a tile of 16 x 300 fits, two do not: 19 strips of one tile, the last with 12 heads
    {"KB2E_COMPLETE_BUFFER_BYTES": "80000"},
    # 1,024 records: a tile takes 64 tails at a time: 19 x 5 steps, the last tail chunk with 44
    {"KB2E_COMPLETE_BUFFER_BYTES": "16384"},
]


@pytest.mark.parametrize("model,n,distance,precision", [("E", 7, 0, 64), ("E", 50, 1, 64), ("E", 512, 0, 64),
                                                        ("H", 7, 0, 64), ("R", 7, 1, 64), ("R", 50, 0, 64),
                                                        ("E", 50, 0, 32), ("H", 50, 0, 32), ("R", 7, 0, 32)])
def test_complete_shapes_strips_and_small_buffers(model, n, distance, precision, monkeypatch):
    """|E| = 300: two tail blocks of 256, the second ragged, and 19 head tiles,
    the last ragged; n = 7 (odd, padded leading dimension), 50 and 512.  The
    strip and buffer knobs force many strips, strips of one tile and chunked
    tails: the counters show more than one strip, fewer records than candidates
    and a buffer smaller than |E|^2, and the results equal the default run's and
    the oracle's (FP32 tables: the oracle on the widened tables)."""
    ne, nr = 300, 3
    ds = data.synthetic("small", seed=5, counts=(ne, nr, 3000, 100, 100))
    known = np.concatenate([ds.train, ds.valid, ds.test])
    s = Setup(model, n, ne, nr, _random_tables(model, ne, nr, n, seed=n + distance), distance=distance,
              precision=precision, oracle=(1,))
    assert np.array_equal(s.energies(1).reshape(-1), s.eng.score(_all_pairs(ne, 1)))
    rels = np.array([0, 1, 2], np.int32)
    cases = [(10, known, False, True), (1024, known, False, False), (10, None, False, False), (10, known, True, True)]
    plain = []
    for k, kn, constrained, loops in cases:
        plain.append(s.check(rels, k, kn, constrained, loops))
        c = _counters(s.eng)
        if not constrained:
            # the default buffer: the first strip of one tile, then the rest of the heads
            assert c["strips"] == 6 and c["records"] < c["candidates"] == 3 * ne * ne
    for knobs in KNOBS:
        for key in ("KB2E_COMPLETE_STRIP_HEADS", "KB2E_COMPLETE_BUFFER_BYTES"):
            monkeypatch.delenv(key, raising=False)
        for key, v in knobs.items():
            monkeypatch.setenv(key, v)
        for (k, kn, constrained, loops), base in zip(cases, plain):
            got = s.check(rels, k, kn, constrained, loops)
            assert _same(got, base)
            c = _counters(s.eng)
            assert c["buffer_records"] == int(knobs["KB2E_COMPLETE_BUFFER_BYTES"]) // 16 < ne * ne
            if not constrained:
                assert c["strips"] > 6
                assert c["records"] < c["candidates"] == 3 * ne * ne
                want = {"32": 3 * 10, "80000": 3 * 19, "16384": 3 * 19 * 5}
                assert c["strips"] == want[knobs.get("KB2E_COMPLETE_STRIP_HEADS", knobs["KB2E_COMPLETE_BUFFER_BYTES"])]


@pytest.mark.parametrize("model,n,distance", [("E", 7, 1), ("H", 50, 0), ("R", 20, 0)])
def test_complete_head_rows_from_l2(model, n, distance, monkeypatch):
    """KB2E_EVAL_ROWS_L2=1 forces the tile kernel's form for dims whose head rows do
    not fit LDS (they are read from the projection table): the same bits."""
    ne, nr = 300, 3
    rng = np.random.default_rng(21)
    known = np.stack([rng.integers(0, ne, 2000), rng.integers(0, ne, 2000), rng.integers(0, nr, 2000)], 1).astype(np.int32)
    s = Setup(model, n, ne, nr, _random_tables(model, ne, nr, n, seed=22), distance=distance, oracle=(2,))
    rels = np.array([2, 0, 1], np.int32)
    plain = [s.check(rels, 10, known, False, True), s.check(rels, 1024, known, True, False)]
    monkeypatch.setenv("KB2E_EVAL_ROWS_L2", "1")
    monkeypatch.setenv("KB2E_COMPLETE_STRIP_HEADS", "48")
    forced = [s.check(rels, 10, known, False, True), s.check(rels, 1024, known, True, False)]
    assert all(_same(a, b) for a, b in zip(plain, forced))


# ------------------------------------------------------------------ 3. ties

def test_complete_ties_break_on_head_then_tail(monkeypatch):
    """Rows from {-1, -1/2, 0, 1/2, 1}^4 under L1: every sum is exact and at most
    25 energies are shared by 90,000 pairs.  Relation 0 is the zero row, so the
    pairs of equal entity rows all have energy 0: more of them than the sort
    buffer holds.  The k-th and the (k+1)-th candidate tie, so only the (head,
    tail) order decides -- across strips, and across 1,024 ties."""
    ne, nr, n = 300, 3, 4
    rng = np.random.default_rng(12)
    values = np.array([-1.0, -0.5, 0.0, 0.5, 1.0])
    ent = rng.choice(values, size=(ne, n), p=[0.1, 0.1, 0.6, 0.1, 0.1])
    rel = rng.choice(values, size=(nr, n))
    rel[0] = 0.0
    s = Setup("E", n, ne, nr, (ent, rel, None), distance=0, oracle=(0, 1, 2))
    for r in range(nr):
        assert len(np.unique(s.energies(r))) <= 25
    for k in (10, 1024):
        # the guard, on the oracle's own energies
        e = np.sort(s.energies(0).reshape(-1))
        assert e[k - 1] == e[k]
        assert (e == e[k - 1]).sum() > 1024
    rels = np.array([0, 1, 2], np.int32)
    known = np.stack([rng.integers(0, ne, 500), rng.integers(0, ne, 500), rng.integers(0, nr, 500)], 1).astype(np.int32)
    base = {}
    for k, kn in itertools.product((10, 1024), (None, known)):
        base[k, kn is None] = s.check(rels, k, kn)
    for knobs in KNOBS:
        for key in ("KB2E_COMPLETE_STRIP_HEADS", "KB2E_COMPLETE_BUFFER_BYTES"):
            monkeypatch.delenv(key, raising=False)
        for key, v in knobs.items():
            monkeypatch.setenv(key, v)
        for k, kn in itertools.product((10, 1024), (None, known)):
            assert _same(s.check(rels, k, kn), base[k, kn is None])
            assert s.eng.counter("complete_strips") >= 30


# ------------------------------------------------------------------ 4. edges

def test_complete_k_larger_than_the_candidate_count():
    ne, nr = 20, 2
    s = Setup("E", 8, ne, nr, _random_tables("E", ne, nr, 8, seed=1), oracle=(0, 1))
    heads, tails, en, found = s.check([0, 1], 1024)
    assert found.tolist() == [400, 400]
    assert (heads[:, 400:] == -1).all() and (tails[:, 400:] == -1).all() and np.isposinf(en[:, 400:]).all()
    assert (heads[:, :400] >= 0).all() and np.isfinite(en[:, :400]).all()
    _, _, _, found = s.check([1], 1024, np.array([(3, 4, 1), (3, 4, 0), (5, 5, 1)], np.int32), exclude_loops=True)
    assert found.tolist() == [400 - 20 - 1]


def test_complete_every_pair_known():
    ne, nr = 3, 2
    s = Setup("E", 8, ne, nr, _random_tables("E", ne, nr, 8, seed=2), oracle=(0, 1))
    known = np.array([(h, t, 1) for h in range(3) for t in range(3)], np.int32)
    for constrained in (False, True):
        heads, tails, en, found = s.check([1, 0, 1], 5, known, constrained)
        assert found[0] == found[2] == 0
        assert (heads[[0, 2]] == -1).all() and (tails[[0, 2]] == -1).all() and np.isposinf(en[[0, 2]]).all()
        # relation 0 has no known triple: 9 candidates, or none from its empty pools
        assert found[1] == (0 if constrained else 5)


def test_complete_relation_listed_twice_and_relation_without_pool():
    ds = tiny()
    s = Setup("H", 12, 200, 10, _random_tables("H", 200, 10, 12, seed=3))
    known = np.concatenate([ds.train, ds.valid])
    heads, tails, en, found = s.check([4, 1, 4, 4, 9], 7, known, True, True)
    for a in (heads, tails, en):
        assert np.array_equal(a[0], a[2]) and np.array_equal(a[0], a[3])
    assert found[0] == found[2] == found[3] == 7
    # constrained: a relation without a known triple has no pools and no candidates
    without = known[known[:, 2] != 5]
    heads, tails, en, found = s.check([5, 4, 5], 7, without, True)
    assert found.tolist() == [0, 7, 0]
    assert (heads[[0, 2]] == -1).all() and (tails[[0, 2]] == -1).all() and np.isposinf(en[[0, 2]]).all()
    assert s.check([5], 7, without, False)[3].tolist() == [7]


def test_complete_pool_of_one_head():
    """A head pool of one entity is a tile with one live row.  Every pair of that
    head with a tail of the pool is a known triple (the tail is in the pool
    because of it), so nothing is new; a second head makes its missing pairs the
    answer."""
    ne, nr = 60, 2
    s = Setup("R", 6, ne, nr, _random_tables("R", ne, nr, 6, seed=4), oracle=(1,))
    one = np.array([(33, t, 1) for t in range(0, 60, 2)] + [(h, 7, 0) for h in range(5)], np.int32)
    _, _, _, found = s.check([1, 0], 64, one, True)
    assert found.tolist() == [0, 0]
    c = _counters(s.eng)
    assert c["candidates"] == 30 + 5 and c["strips"] == 2
    two = np.concatenate([one, [(34, 1, 1), (34, 3, 1)]]).astype(np.int32)
    heads, tails, _, found = s.check([1], 64, two, True)
    assert found.tolist() == [32]  # 2 x 32 pairs, 32 of them known
    assert set(zip(heads[0, :32].tolist(), tails[0, :32].tolist())) == \
        {(33, 1), (33, 3)} | {(34, t) for t in range(0, 60, 2)}


def test_complete_exclude_loops_when_the_best_is_a_loop():
    ne, nr = 40, 2
    ent, rel, _ = _random_tables("E", ne, nr, 10, seed=5)
    rel[1] = 0.0  # t - h - r = 0 exactly for h == t: every loop has energy 0
    s = Setup("E", 10, ne, nr, (ent, rel, None), distance=1, oracle=(1,))
    heads, tails, en, found = s.check([1], 50)
    assert (heads[0, :40] == tails[0, :40]).all() and (en[0, :40] == 0).all() and heads[0, :40].tolist() == list(range(40))
    assert en[0, 40] > 0
    h2, t2, e2, found = s.check([1], 50, None, False, True)
    assert (h2[0] != t2[0]).all() and (e2[0] > 0).all()
    assert np.array_equal(h2[0, :10], heads[0, 40:]) and np.array_equal(t2[0, :10], tails[0, 40:])


# ------------------------------------------------------------------ 5. the composed route

@pytest.mark.parametrize("model,n", [("E", 20), ("R", 20)])
def test_complete_equals_predict_over_every_head(model, n):
    """|E| = 2,000: Engine.predict with every entity as a head query (side 1),
    the same filter and k, flattened and sorted by (energy, head, tail)."""
    ne, nr, k = 2000, 2, 50
    rng = np.random.default_rng(7)
    eng = Engine(model, n, ne, nr)
    eng.upload_params(*_random_tables(model, ne, nr, n, seed=8))
    known = np.stack([rng.integers(0, ne, 6000), rng.integers(0, ne, 6000), rng.integers(0, nr, 6000)], 1).astype(np.int32)
    ids, en, found = eng.predict(np.arange(ne, dtype=np.int32), np.ones(ne, np.int32), np.ones(ne, np.int32), k, known)
    assert (found == k).all()
    H = np.repeat(np.arange(ne), k)
    T, E = ids.reshape(-1), en.reshape(-1)
    order = np.lexsort((T, H, E))[:k]
    heads, tails, energy, cfound = eng.complete([1], k, known)
    assert cfound.tolist() == [k]
    assert np.array_equal(heads[0], H[order]) and np.array_equal(tails[0], T[order])
    assert np.array_equal(energy[0], E[order])
    c = _counters(eng)
    assert c["candidates"] == ne * ne and c["records"] < c["candidates"] // 10 and c["strips"] == 2


# ------------------------------------------------------------------ 6. contract

@pytest.mark.parametrize("model,n", [("E", 20), ("H", 32), ("R", 20)])
def test_complete_leaves_the_context_unchanged(model, n):
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
            known = np.concatenate([ds.train, ds.valid])
            eng.profile(True)
            b0 = eng.device_bytes()
            one = eng.complete(np.arange(10), 10, known, constrained=True, exclude_loops=True)
            assert eng.device_bytes() == b0
            two = eng.complete(np.arange(10), 10, known, constrained=True, exclude_loops=True)
            assert eng.device_bytes() == b0
            assert _same(one, two)
            assert _same(eng.complete([3], 1024), eng.complete([3], 1024))
            assert eng.device_bytes() == b0
            for fam in ("complete_score", "complete_select"):
                ms, cnt = eng.profile_query(fam)
                assert cnt > 0 and ms > 0, fam
            eng.profile(False)
            for a, b in zip(before, eng.download_params()):
                assert (a is None and b is None) or np.array_equal(a, b)
            if model == "R":
                hw, tw = eng.transr_work()
                assert np.array_equal(hw, work[0]) and np.array_equal(tw, work[1])
            # (and the energies did not see those work vectors)
            heads, tails, en, found = one
            trip = np.stack([heads[4], tails[4], np.full(10, 4)], 1)
            assert np.array_equal(eng.score(trip), en[4])
            res = linkpred.completion(eng, ds, 10)
            assert res["relations"] == 10 and 0 < res["mined"] <= 100 and 0 <= res["hits"] <= res["test"]
        streams.append(first + [eng.rng_next() for _ in range(20)])
    assert streams[0] == streams[1]


def test_complete_bad_arguments_are_refused():
    ne, nr = 200, 10
    eng = Engine("E", 20, ne, nr)
    eng.upload_params(*_random_tables("E", ne, nr, 20, seed=13))
    b0 = eng.device_bytes()
    ok = np.array([(0, 1, 2)], np.int32)
    eng.complete([3], 5, ok)
    assert eng.device_bytes() == b0
    for args, kw in ((([3], 0), {}), (([3], 1025), {}), (([3], -1), {}), (([nr], 5), {}), (([-1], 5), {}),
                     (([3, nr], 5), {}), ((np.zeros(0, np.int32), 5), {}),
                     (([3], 5, np.array([(ne, 1, 0)], np.int32)), {}), (([3], 5, np.array([(0, -1, 0)], np.int32)), {}),
                     (([3], 5, np.array([(0, 1, nr)], np.int32)), {}), (([3], 5, np.array([(0, 1, -1)], np.int32)), {}),
                     (([3], 5, ok), {"constrained": 2}), (([3], 5, ok), {"exclude_loops": -1})):
        with pytest.raises(EngineError):
            eng.complete(*args, **kw)
        assert eng.device_bytes() == b0
    # the C ABI itself: flags other than 0 / 1 and NULL arrays with a count > 0
    import ctypes as C
    from kb2e_amd.engine import lib
    r = np.array([3], np.int32)
    h, t = np.zeros(5, np.int32), np.zeros(5, np.int32)
    e, f = np.zeros(5), np.zeros(1, np.int64)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    out = (ip(h), ip(t), e.ctypes.data_as(C.POINTER(C.c_double)), f.ctypes.data_as(C.POINTER(C.c_int64)))
    call = lib().kb2e_complete_triples
    assert call(eng.h, ip(r), 1, 5, None, None, None, 0, 0, 0, *out) == 0
    assert call(eng.h, ip(r), 1, 5, None, None, None, 0, 2, 0, *out) == 1
    assert call(eng.h, ip(r), 1, 5, None, None, None, 0, 0, 7, *out) == 1
    assert call(eng.h, ip(r), 1, 5, None, None, None, 3, 0, 0, *out) == 1
    assert call(eng.h, None, 1, 5, None, None, None, 0, 0, 0, *out) == 1
    assert call(eng.h, ip(r), 0, 5, None, None, None, 0, 0, 0, *out) == 1
    assert eng.device_bytes() == b0
    with pytest.raises(EngineError):
        eng.counter("complete_nothing")
    # still usable
    assert eng.complete([3], 5, ok)[3].tolist() == [5]


# ------------------------------------------------------------------ 7. CLI

def test_complete_cli_matches_engine(tmp_path):
    name = "transe_l1_bern"
    f = MANIFEST["runs"][name]["flags"]
    ds = tiny()
    d = os.path.join(GOLDEN, name)
    exe = tmp_path / "completeTransE"
    exe.symlink_to(os.path.join(ROOT, "bin", "kb2e"))
    base = [str(exe), "--datadir", os.path.join(GOLDEN, "tiny"), "--outdir", d, "--size", str(f["size"]), "--method",
            str(f["method"]), "--distance", str(f["distance"])]
    eng = Engine("E", f["size"], ds.num_entities, ds.num_relations, distance=f["distance"])
    eng.upload_params(data.read_table(os.path.join(d, "entity2vec.bern"), ds.num_entities, f["size"]),
                      data.read_table(os.path.join(d, "relation2vec.bern"), ds.num_relations, f["size"]))
    names = {v: k for k, v in data._load_ids(os.path.join(GOLDEN, "tiny", "entity2id.txt")).items()}
    rnames = {v: k for k, v in data._load_ids(os.path.join(GOLDEN, "tiny", "relation2id.txt")).items()}
    relfile = tmp_path / "relations.txt"
    relfile.write_text(f"{rnames[6]}\n/r/nothing\n{rnames[0]}\n{rnames[6]}\n")
    every = list(range(ds.num_relations))
    full = np.concatenate([ds.test, ds.train, ds.valid])
    part = np.concatenate([ds.train, ds.valid])
    for extra, rels, k, known, constrained, loops in (
            ([], every, 10, full, True, False),
            (["--topk", "3", "--filtered", "0", "--constrained", "0", "--loops", "1"], every, 3, part, False, True),
            (["--relations", str(relfile), "--topk", "4"], [6, 0, 6], 4, full, True, False)):
        res = subprocess.run(base + extra, capture_output=True, text=True, timeout=300, check=True)
        reported = "Relation found in triple file that was not found in the identity file: /r/nothing" in res.stdout
        assert reported == ("--relations" in extra)
        rows = [l.split("\t") for l in res.stdout.splitlines() if l.count("\t") == 4]
        heads, tails, en, found = eng.complete(rels, k, known, constrained=constrained, exclude_loops=not loops)
        assert found.sum() > 0
        expect = [(rnames[r], j + 1, names[int(heads[q, j])], names[int(tails[q, j])], en[q, j])
                  for q, r in enumerate(rels) for j in range(found[q])]
        assert len(rows) == len(expect)
        for (rn, pos, hn, tn, val), (xr, xp, xh, xt, xv) in zip(rows, expect):
            assert (rn, int(pos), hn, tn) == (xr, xp, xh, xt)
            assert abs(float(val) - xv) <= 5.000001e-7
