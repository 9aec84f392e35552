"""Relation prediction (kb2e_predict_relations, kb2e_rank_relations) against the
oracle.

The oracle for a pair (h, t) is plain numpy over orc.Model(..., transr_compat=
False).energy: the energies of all |R| relations, the known relations dropped,
np.lexsort((ids, energy)), the first k.  All device arithmetic is FP64 in the
reference's order and ties break on the relation id, so ids, energies and found
counts must be EQUAL (no tolerance anywhere in this file except where a printed
%.6lf is compared).
"""
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

def _random_transr(ds, n, seed, scale=0.3):
    """tests/test_gpu_eval.py _random_transr's recipe."""
    rng = np.random.default_rng(seed)
    ent = rng.standard_normal((ds.num_entities, n))
    ent /= np.linalg.norm(ent, axis=1, keepdims=True)
    rel = rng.standard_normal((ds.num_relations, n)) * scale
    w = np.eye(n)[None] + rng.standard_normal((ds.num_relations, n, n)) * (scale / np.sqrt(n))
    return ent, rel, w


def _tables(model, ds, n, seed):
    """tests/test_gpu_predict.py _tables' recipe."""
    if model == "R":
        return _random_transr(ds, n, seed)
    rng = np.random.default_rng(seed)
    ent = rng.standard_normal((ds.num_entities, n)) * 0.2
    rel = rng.standard_normal((ds.num_relations, n)) * 0.2
    w = None
    if model == "H":
        w = rng.standard_normal((ds.num_relations, n))
        w /= np.linalg.norm(w, axis=1, keepdims=True)
    return ent, rel, w


def _f32(tables):
    return tuple(None if t is None else t.astype(np.float32).astype(np.float64) for t in tables)


def _known(filt):
    """(h, t) -> the relations a filter excludes."""
    table = {}
    for h, t, r in np.asarray(filt).tolist():
        table.setdefault((h, t), set()).add(r)
    return table


class Setup:
    """An engine and the oracle on the same tables; oracle rows (the energies of
    all relations of a pair) are memoised and never modified."""

    def __init__(self, model, n, ds, *, distance=0, precision=64, seed=0, tables=None, **kw):
        self.ds, self.nr = ds, ds.num_relations
        self.tables = _tables(model, ds, n, seed) if tables is None else tables
        self.eng = Engine(model, n, ds.num_entities, ds.num_relations, distance=distance, precision=precision, **kw)
        self.eng.upload_params(*self.tables)
        self.m = orc.Model(model, n, ds.num_entities, ds.num_relations, distance=distance, transr_compat=False)
        self.m.set_tables(*(_f32(self.tables) if precision == 32 else self.tables))
        self.filt = np.concatenate([ds.train, ds.valid, ds.test])
        self._rows = {}
        self._known = None

    def row(self, h, t):
        key = (int(h), int(t))
        if key not in self._rows:
            row = np.array([self.m.energy(key[0], key[1], r) for r in range(self.nr)])
            row.setflags(write=False)
            self._rows[key] = row
        return self._rows[key]

    def known(self, filt):
        if filt is None:
            return {}
        if self._known is None or self._known[0] is not filt:
            self._known = (filt, _known(filt))
        return self._known[1]

    def expect(self, h, t, k, filt=None):
        known = self.known(filt)
        ids = np.full((len(h), k), -1, np.int32)
        en = np.full((len(h), k), np.inf)
        found = np.zeros(len(h), np.int32)
        for q in range(len(h)):
            row = self.row(h[q], t[q])
            keep = np.ones(self.nr, bool)
            keep[list(known.get((int(h[q]), int(t[q])), ()))] = False
            cand = np.arange(self.nr)[keep]
            order = np.lexsort((cand, row[keep]))[:k]
            found[q] = len(order)
            ids[q, :len(order)] = cand[order]
            en[q, :len(order)] = row[keep][order]
        return ids, en, found

    def check(self, h, t, k, filt=None):
        h, t = (np.asarray(a, dtype=np.int32) for a in (h, t))
        ids, en, found = self.eng.predict_relations(h, t, k, filt)
        xi, xe, xf = self.expect(h, t, k, filt)
        assert ids.shape == (len(h), k) and ids.dtype == np.int32 and en.dtype == np.float64
        assert np.array_equal(found, xf)
        assert np.array_equal(ids, xi)
        assert np.array_equal(en, xe)
        return ids, en, found

    def expect_ranks(self, test, filt):
        known = self.known(filt)
        ranks = np.zeros((len(test), 2), np.int64)
        for i, (h, t, r) in enumerate(np.asarray(test).tolist()):
            row = self.row(h, t)
            above = row < row[r]
            ranks[i, 0] = 1 + above.sum()
            others = [x for x in known.get((h, t), ()) if x != r]
            above[others] = False
            ranks[i, 1] = 1 + above.sum()
        return ranks

    def known_counts(self, pairs, filt):
        known = self.known(filt)
        return np.array([len(known.get((int(h), int(t)), ())) for h, t in np.asarray(pairs)[:, :2]])


# The datasets of the issue: the filter bites on each (pairs with several known relations).
def _ds1345():
    return data.synthetic("small", seed=3, counts=(300, 1345, 3000, 50, 50))


def _ds2085():
    return data.synthetic("small", seed=3, counts=(60, 2085, 4000, 50, 50))


def _ds300():
    return data.synthetic("small", seed=3, counts=(40, 300, 3000, 100, 100))


@pytest.fixture(scope="module")
def tiny_e():
    return Setup("E", 20, tiny(), seed=1)


@pytest.fixture(scope="module")
def tiny_r():
    return Setup("R", 20, tiny(), seed=2)


@pytest.fixture(scope="module")
def e1345():
    return Setup("E", 20, _ds1345(), seed=3)


@pytest.fixture(scope="module")
def e2085():
    return Setup("E", 20, _ds2085(), seed=4)


@pytest.fixture(scope="module")
def e300():
    return Setup("E", 20, _ds300(), seed=5)


# ------------------------------------------------------------------ 1. models

@pytest.mark.parametrize("model,n,distance", [("E", 20, 0), ("E", 50, 1), ("H", 32, 0), ("R", 20, 0), ("R", 20, 1)])
def test_relpred_models_tiny_all_test_pairs(model, n, distance):
    """Every test pair of the golden tiny set (200 queries), k = 10 = |R|, raw and
    filtered (train + valid + test): found = 10 - known per pair."""
    s = Setup(model, n, tiny(), distance=distance, seed=n + distance)
    h, t = s.ds.test[:, 0], s.ds.test[:, 1]
    assert len(h) == 200 and s.nr == 10
    _, _, found = s.check(h, t, 10)
    assert (found == 10).all()
    _, _, found = s.check(h, t, 10, s.filt)
    assert np.array_equal(found, 10 - s.known_counts(s.ds.test, s.filt))
    assert len(set(found.tolist())) > 1


# ------------------------------------------------------------------ 2. |R| edges

@pytest.mark.parametrize("model", ["E", "R"])
def test_relpred_1345_relations(model, e1345):
    """|R| = 1,345 (FB15k's): six candidate blocks of 256, the last one ragged.
    A TransR context takes no more relations than entities (kb2e_create), so its
    set has 1,345 entities instead of 300: 9 of its 50 test pairs have more than
    one known relation (20 of 50 on the 300-entity set)."""
    if model == "E":
        s = e1345
    else:
        s = Setup("R", 20, data.synthetic("small", seed=3, counts=(1345, 1345, 3000, 50, 50)), seed=6)
    h, t = s.ds.test[:, 0], s.ds.test[:, 1]
    assert (s.known_counts(s.ds.test, s.filt) > 1).sum() >= 9
    s.check(h, t, 10, s.filt)
    s.check(h, t, 10)
    _, _, found = s.check(h, t, 1000, s.filt)
    assert (found == 1000).all()


def test_relpred_2085_relations(e2085):
    """More keys than the 1,024-pair sort buffer: the radix passes run."""
    s = e2085
    h, t = s.ds.test[:, 0], s.ds.test[:, 1]
    assert s.known_counts(s.ds.test, s.filt).max() > 100
    s.check(h, t, 10, s.filt)
    _, _, found = s.check(h, t, 1024)
    assert (found == 1024).all()
    s.check(h, t, 1024, s.filt)


def test_relpred_300_relations_k_equals_r(e300):
    s = e300
    h, t = s.ds.test[:, 0], s.ds.test[:, 1]
    ids, en, found = s.check(h, t, 300, s.filt)
    kn = s.known_counts(s.ds.test, s.filt)
    assert np.array_equal(found, 300 - kn) and (kn > 1).sum() >= 50
    for q in range(len(h)):
        assert (ids[q, found[q]:] == -1).all() and np.isposinf(en[q, found[q]:]).all()
        assert (ids[q, :found[q]] >= 0).all() and np.isfinite(en[q, :found[q]]).all()
    _, _, found = s.check(h, t, 300)
    assert (found == 300).all()


@pytest.mark.parametrize("model", ["E", "R"])
def test_relpred_three_relations(model):
    """A row far shorter than a wave."""
    ds = data.synthetic("small", seed=4, counts=(50, 3, 300, 20, 20))
    s = Setup(model, 20, ds, seed=7)
    h, t = ds.test[:, 0], ds.test[:, 1]
    _, _, found = s.check(h, t, 3)
    assert (found == 3).all()
    _, _, found = s.check(h, t, 3, s.filt)
    assert (found < 3).all()
    s.check(h, t, 1, s.filt)
    s.check(h, t, 10, s.filt)  # k > |R|


# ------------------------------------------------------------------ 3. all candidates known

@pytest.mark.parametrize("which", ["tiny_e", "tiny_r", "e1345"])
def test_relpred_every_relation_known(which, request):
    s = request.getfixturevalue(which)
    test = s.ds.test
    h, t = test[:5, 0].copy(), test[:5, 1].copy()
    hq, tq = int(h[2]), int(t[2])
    assert sum(1 for a, b in zip(h, t) if (a, b) == (hq, tq)) == 1
    every = np.array([(hq, tq, r) for r in range(s.nr)], dtype=np.int32)
    filt = np.concatenate([s.filt, every])
    ids, en, found = s.check(h, t, 10, filt)
    assert found[2] == 0 and (ids[2] == -1).all() and np.isposinf(en[2]).all()
    # the neighbouring queries of the same call are what they are without that pair
    keep = [0, 1, 3, 4]
    ids2, en2, found2 = s.eng.predict_relations(h[keep], t[keep], 10, s.filt)
    assert np.array_equal(ids[keep], ids2) and np.array_equal(en[keep], en2) and np.array_equal(found[keep], found2)
    assert (found2 > 0).all()
    # a call that is nothing but such a pair
    ids, en, found = s.check([hq], [tq], 7, every)
    assert found[0] == 0 and (ids == -1).all() and np.isposinf(en).all()


# ------------------------------------------------------------------ 4. nq edges

@pytest.mark.parametrize("which", ["tiny_e", "tiny_r"])
def test_relpred_nq_edges(which, request):
    s = request.getfixturevalue(which)
    test = s.ds.test
    s.check(test[:1, 0], test[:1, 1], 10, s.filt)  # nq = 1
    s.check(test[:1, 0], test[:1, 1], 4)
    s.check(test[:17, 0], test[:17, 1], 10, s.filt)  # one past a tile of 16
    s.check(test[:17, 0], test[:17, 1], 7)
    # repeated identical pairs (they share one known-relation list)
    s.check(np.repeat(test[:3, 0], 6), np.repeat(test[:3, 1], 6), 10, s.filt)
    # h == t, alone and among others
    s.check([5], [5], 10, s.filt)
    s.check([5, 7, int(test[0, 0]), 7], [5, 7, int(test[0, 1]), 9], 10, s.filt)
    # pairs that appear in no filter triple: nothing is excluded
    kn = s.known(s.filt)
    free = [(a, b) for a in range(3) for b in range(40, 60) if (a, b) not in kn][:9]
    assert len(free) == 9
    fh, ft = [a for a, _ in free], [b for _, b in free]
    _, _, found = s.check(fh, ft, 10, s.filt)
    assert (found == 10).all()
    # ... mixed with pairs that do
    s.check(fh + test[:4, 0].tolist(), ft + test[:4, 1].tolist(), 10, s.filt)


# ------------------------------------------------------------------ 5. TransR shapes and forced paths

@pytest.mark.parametrize("n", [100, 160])
def test_relpred_transr_wide(n):
    """Two and three elements a lane in score_triples_transr_kernel; W_r past any LDS size."""
    s = Setup("R", n, tiny(), seed=n)
    test = s.ds.test[:12]
    s.check(test[:, 0], test[:, 1], 10, s.filt)
    s.check(test[:, 0], test[:, 1], 3)


@pytest.mark.parametrize("env", [{"KB2E_RELPRED_REL_BATCH": "3"}, {"KB2E_RELPRED_REL_BATCH": "1"},
                                 {"KB2E_PREDICT_CHUNK_ROWS": "3"}, {"KB2E_PREDICT_KEYS_L2": "1"},
                                 {"KB2E_RELPRED_KEYS_STRIDED": "1"},
                                 {"KB2E_RELPRED_REL_BATCH": "3", "KB2E_PREDICT_CHUNK_ROWS": "3",
                                  "KB2E_RELPRED_KEYS_STRIDED": "1"}])
@pytest.mark.parametrize("which", ["tiny_r", "tiny_e"])
def test_relpred_forced_paths(which, env, request, monkeypatch):
    """Relation batches of 3 on |R| = 10 (four batches, the last with one relation)
    and of 1; key-buffer chunks of 3 rows with 17 queries (six chunks, the last
    short; TransR rebuilds its entity list per chunk); the select kernel's L2 form;
    the pair kernel's plain strided key store.  Each equals the unforced result
    and the oracle."""
    s = request.getfixturevalue(which)
    test = s.ds.test[:17]
    h, t = test[:, 0], test[:, 1]
    plain = [s.eng.predict_relations(h, t, 10, s.filt), s.eng.predict_relations(h, t, 4)]
    plain_ranks = s.eng.rank_relations(test, s.filt)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    forced = [s.check(h, t, 10, s.filt), s.check(h, t, 4)]
    for a, b in zip(plain, forced):
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
    assert np.array_equal(s.eng.rank_relations(test, s.filt), plain_ranks)
    assert np.array_equal(plain_ranks, s.expect_ranks(test, s.filt))


def test_relpred_forced_paths_many_relations(e2085, monkeypatch):
    """The L2 form of the selection where the radix passes run, in chunks."""
    s = e2085
    test = s.ds.test[:7]
    monkeypatch.setenv("KB2E_PREDICT_KEYS_L2", "1")
    monkeypatch.setenv("KB2E_PREDICT_CHUNK_ROWS", "3")
    s.check(test[:, 0], test[:, 1], 10, s.filt)
    s.check(test[:, 0], test[:, 1], 1024, s.filt)


# ------------------------------------------------------------------ 6. ties

def test_relpred_ties_break_on_relation_id():
    ds = _ds300()
    ent, rel, _ = _tables("E", ds, 20, 8)
    h, t = 3, 17
    for r in (41, 130, 256):
        rel[r] = ent[t] - ent[h]
    s = Setup("E", 20, ds, tables=(ent, rel, None))
    row = s.row(h, t)
    assert row[41] == row[130] == row[256] and (np.delete(row, [41, 130, 256]) > row[41]).all()
    ids, _, _ = s.check([h], [t], 2)
    assert ids[0].tolist() == [41, 130]
    ids, _, _ = s.check([h], [t], 3)
    assert ids[0].tolist() == [41, 130, 256]
    ids, _, _ = s.check([h], [t], 4)
    assert ids[0, :3].tolist() == [41, 130, 256]
    filt = np.array([(h, t, 130)], dtype=np.int32)
    ids, _, found = s.check([h], [t], 300, filt)
    assert ids[0, :2].tolist() == [41, 256] and found[0] == 299 and 130 not in ids[0].tolist()
    # ties with the truth are not counted above it
    ranks = s.eng.rank_relations(np.array([(h, t, 41), (h, t, 130), (h, t, 256)], dtype=np.int32), None)
    assert ranks.tolist() == [[1, 1]] * 3


# ------------------------------------------------------------------ 7. FP32 tables

@pytest.mark.parametrize("model,n,distance", [("E", 20, 0), ("H", 32, 0), ("R", 20, 1)])
def test_relpred_fp32_tables(model, n, distance):
    """precision=32: the tables are widened to FP64 first, so the oracle on the
    tables rounded through float32 gives the same bits."""
    s = Setup(model, n, tiny(), distance=distance, precision=32, seed=9)
    test = s.ds.test[:40]
    s.check(test[:, 0], test[:, 1], 10, s.filt)
    s.check(test[:, 0], test[:, 1], 10)
    assert np.array_equal(s.eng.rank_relations(test, s.filt), s.expect_ranks(test, s.filt))


# ------------------------------------------------------------------ 8. consistency

@pytest.mark.parametrize("model,n,distance", [("E", 50, 1), ("H", 32, 0), ("R", 20, 0), ("R", 100, 1)])
def test_relpred_energies_are_score_triples_bits(model, n, distance):
    s = Setup(model, n, tiny(), distance=distance, seed=10)
    test = s.ds.test[:20]
    ids, en, found = s.eng.predict_relations(test[:, 0], test[:, 1], s.nr)
    assert (found == s.nr).all()
    trip = np.stack([np.repeat(test[:, 0], s.nr), np.repeat(test[:, 1], s.nr), ids.reshape(-1)], 1)
    assert np.array_equal(s.eng.score(trip), en.reshape(-1))


def test_rank_relations_agree_with_predict_relations(tiny_e):
    """k = |R|, no filter: the truth's position in the list is its raw rank, on tables without ties."""
    s = tiny_e
    test = s.ds.test
    for h, t, _ in test.tolist():
        assert len(set(s.row(h, t).tolist())) == s.nr
    ranks = s.eng.rank_relations(test, s.filt)
    ids, _, found = s.eng.predict_relations(test[:, 0], test[:, 1], s.nr)
    assert (found == s.nr).all()
    for i, (_, _, r) in enumerate(test.tolist()):
        assert int(np.nonzero(ids[i] == r)[0][0]) + 1 == ranks[i, 0]


@pytest.mark.parametrize("which", ["tiny_e", "tiny_r", "e1345", "e2085", "e300"])
def test_rank_relations_match_numpy_count(which, request):
    s = request.getfixturevalue(which)
    test = s.ds.test
    ranks = s.eng.rank_relations(test, s.filt)
    assert ranks.shape == (len(test), 2) and ranks.dtype == np.int64
    exp = s.expect_ranks(test, s.filt)
    assert np.array_equal(ranks, exp)
    assert (exp[:, 1] < exp[:, 0]).any()  # (the filter bites)
    raw = s.eng.rank_relations(test, None)
    assert np.array_equal(raw[:, 0], exp[:, 0]) and np.array_equal(raw[:, 1], exp[:, 0])
    # the caller's order
    perm = np.random.default_rng(1).permutation(len(test))[:33]
    assert np.array_equal(s.eng.rank_relations(test[perm], s.filt), exp[perm])
    assert np.array_equal(s.eng.rank_relations(test[:1], s.filt), exp[:1])
    res = linkpred.relation_prediction(s.eng, test, s.filt)
    assert res["count"] == len(test)
    assert res["raw"]["mean_rank"] == exp[:, 0].mean() and res["filtered"]["mean_rank"] == exp[:, 1].mean()
    assert res["raw"]["hits@1"] == (exp[:, 0] <= 1).mean() and res["filtered"]["hits@10"] == (exp[:, 1] <= 10).mean()


# ------------------------------------------------------------------ 9. contract

def test_relpred_bad_arguments_are_refused(tiny_e):
    s = tiny_e
    eng, ne, nr = s.eng, s.ds.num_entities, s.ds.num_relations
    b0 = eng.device_bytes()
    eng.predict_relations([3], [2], 5)
    bad = np.array([(0, ne, 0)], dtype=np.int32)
    for args in (([3], [2], 0), ([3], [2], 1025), ([3], [2], -1), ([ne], [2], 5), ([3], [-1], 5), ([3], [ne], 5),
                 ([3], [2], 5, bad), ([3], [2], 5, np.array([(0, 1, -1)], dtype=np.int32)),
                 ([3], [2], 5, np.array([(-1, 1, 0)], dtype=np.int32)),
                 ([3], [2], 5, np.array([(0, 1, nr)], dtype=np.int32)),
                 (np.zeros(0, np.int32), np.zeros(0, np.int32), 5)):
        with pytest.raises(EngineError):
            eng.predict_relations(*args)
        assert eng.device_bytes() == b0
    for test in ([(ne, 0, 0)], [(0, -1, 0)], [(0, 1, nr)], [(0, 1, -1)]):
        with pytest.raises(EngineError):
            eng.rank_relations(np.array(test, dtype=np.int32), s.filt)
        assert eng.device_bytes() == b0
    with pytest.raises(EngineError):
        eng.rank_relations(np.zeros((0, 3), np.int32), s.filt)
    with pytest.raises(EngineError):
        eng.rank_relations(s.ds.test[:2], bad)
    assert eng.device_bytes() == b0
    # still usable
    s.check([3], [2], 5)


def _entity_oracle(s, e, r, side, k, filt):
    """Engine.predict's answer from the oracle (tests/test_gpu_predict.py Setup.expect)."""
    ne = s.ds.num_entities
    known = {}
    for h, t, rr in np.asarray(filt).tolist():
        known.setdefault((h, rr, 1), set()).add(t)
        known.setdefault((t, rr, 0), set()).add(h)
    ids = np.full((len(e), k), -1, np.int32)
    en = np.full((len(e), k), np.inf)
    rows = []
    for q in range(len(e)):
        row = np.array([s.m.energy(int(e[q]), x, int(r[q])) if side[q] else s.m.energy(x, int(e[q]), int(r[q]))
                        for x in range(ne)])
        rows.append(row)
        keep = np.ones(ne, bool)
        keep[list(known.get((int(e[q]), int(r[q]), int(side[q])), ()))] = False
        cand = np.arange(ne)[keep]
        order = np.lexsort((cand, row[keep]))[:k]
        ids[q, :len(order)] = cand[order]
        en[q, :len(order)] = row[keep][order]
    return ids, en, rows, known


@pytest.mark.parametrize("model,n", [("E", 20), ("H", 32), ("R", 20)])
def test_relpred_calls_leave_the_context_unchanged(model, n):
    """device_bytes() before == after each call (every buffer freed), the tables
    and the TransR work vectors untouched, the four profile families reported,
    and the entity-side calls of the same engine still match their oracle."""
    s = Setup(model, n, tiny(), seed=11)
    eng, ds = s.eng, s.ds
    if model == "R":
        eng.upload_triples(ds.train)  # (the work vectors exist once the triples are up)
        eng.upload_params(*s.tables)
        eng.set_transr_work(np.arange(n) * 0.5, np.arange(n) * -0.25)
    before = eng.download_params()
    work = eng.transr_work() if model == "R" else None
    test = ds.test[:20]
    eng.profile(True)
    b0 = eng.device_bytes()
    eng.predict_relations(test[:, 0], test[:, 1], 10, s.filt)
    assert eng.device_bytes() == b0
    eng.predict_relations(test[:, 0], test[:, 1], 10)
    assert eng.device_bytes() == b0
    eng.rank_relations(test, s.filt)
    assert eng.device_bytes() == b0
    eng.rank_relations(test, None)
    assert eng.device_bytes() == b0
    with pytest.raises(EngineError):
        eng.predict_relations(test[:, 0], test[:, 1], 0)
    assert eng.device_bytes() == b0
    for fam in ("relpred_score", "relpred_mask", "relpred_select", "relpred_rank"):
        ms, cnt = eng.profile_query(fam)
        assert cnt > 0 and ms > 0, fam
    eng.profile(False)
    after = eng.download_params()
    for a, b in zip(before, after):
        assert (a is None and b is None) or np.array_equal(a, b)
    if model == "R":
        hw, tw = eng.transr_work()
        assert np.array_equal(hw, work[0]) and np.array_equal(tw, work[1])
    # (and the energies did not see those work vectors)
    s.check(test[:4, 0], test[:4, 1], 5, s.filt)
    # predict, score and rank_triples afterwards
    pick = ds.test[:4]
    e = np.concatenate([pick[:, 0], pick[:, 1]]).astype(np.int32)
    r = np.concatenate([pick[:, 2], pick[:, 2]]).astype(np.int32)
    side = np.array([1] * 4 + [0] * 4, np.int32)
    xi, xe, rows, known = _entity_oracle(s, e, r, side, 10, s.filt)
    ids, en, found = eng.predict(e, r, side, 10, s.filt)
    assert np.array_equal(ids, xi) and np.array_equal(en, xe) and (found == 10).all()
    trip = ds.test[:50]
    assert np.array_equal(eng.score(trip), np.array([s.m.energy(int(a), int(b), int(c)) for a, b, c in trip]))
    ranks = eng.rank_triples(pick, s.filt)
    for i, (h, t, rr) in enumerate(pick.tolist()):
        for sd, fixed, truth, row in ((1, h, t, rows[i]), (0, t, h, rows[4 + i])):
            above = row < row[truth]
            assert ranks[i, 2 * sd] == 1 + above.sum()
            above[[x for x in known.get((fixed, rr, sd), ()) if x != truth]] = False
            assert ranks[i, 2 * sd + 1] == 1 + above.sum()


# ------------------------------------------------------------------ 10. CLI

def test_relpred_cli_matches_engine(tmp_path):
    name = "transe_l1_bern"
    f = MANIFEST["runs"][name]["flags"]
    ds = tiny()
    d = os.path.join(GOLDEN, name)
    ph, pt = (int(x) for x in ds.test[0, :2])
    qfile = tmp_path / "queries.txt"
    # line 3 names an unknown entity in a relation query, line 6 has no tail: reported and skipped
    qfile.write_text(f"/m/e25\t?\t/r/r4\n/m/e{ph}\t/m/e{pt}\t?\n?\t/m/e58\t/r/r1\n/m/nobody\t/m/e3\t?\n"
                     "/m/e7\t/m/e7\t?\n/m/e114\t?\t/r/r4\n/m/e9\t?\t?\n/m/e30\t/m/e12\t?\n?\t/m/e105\t/r/r0\n")
    kinds = {0: ("ent", 0), 1: ("rel", 0), 2: ("ent", 1), 4: ("rel", 1), 5: ("ent", 2), 7: ("rel", 2), 8: ("ent", 3)}
    e, r, side = [25, 58, 114, 105], [4, 1, 4, 0], [1, 0, 1, 0]
    rh, rt = [ph, 7, 30], [pt, 7, 12]
    exe = tmp_path / "predictTransE"
    exe.symlink_to(os.path.join(ROOT, "bin", "kb2e"))
    base = [str(exe), "--datadir", os.path.join(GOLDEN, "tiny"), "--outdir", d, "--size", str(f["size"]), "--method",
            str(f["method"]), "--distance", str(f["distance"]), "--queries", str(qfile)]
    eng = Engine("E", f["size"], ds.num_entities, ds.num_relations, distance=f["distance"])
    eng.upload_params(data.read_table(os.path.join(d, "entity2vec.bern"), ds.num_entities, f["size"]),
                      data.read_table(os.path.join(d, "relation2vec.bern"), ds.num_relations, f["size"]))
    names = {v: k for k, v in data._load_ids(os.path.join(GOLDEN, "tiny", "entity2id.txt")).items()}
    rnames = {v: k for k, v in data._load_ids(os.path.join(GOLDEN, "tiny", "relation2id.txt")).items()}
    filt = np.concatenate([ds.test, ds.train, ds.valid])
    for extra, k, fl in (([], 10, filt), (["--topk", "3", "--filtered", "0"], 3, None)):
        res = subprocess.run(base + extra, capture_output=True, text=True, timeout=300, check=True)
        assert "Head entity found in triple file that was not found in the identity file: /m/nobody" in res.stdout
        assert "Relation query needs both the head and the tail: /m/e9 ?" in res.stdout
        rows = [l.split("\t") for l in res.stdout.splitlines() if l.count("\t") == 3 and l.split("\t")[0].isdigit()]
        ids, en, found = eng.predict(e, r, side, k, fl)
        rids, ren, rfound = eng.predict_relations(rh, rt, k, fl)
        assert (found == k).all()
        if fl is not None:
            assert rfound[0] < 10  # (the test pair's own relation is known)
        expect = []
        for line in sorted(kinds):  # interleaved, in line order
            kind, q = kinds[line]
            if kind == "ent":
                expect += [(line, j + 1, names[int(ids[q, j])], en[q, j]) for j in range(found[q])]
            else:
                expect += [(line, j + 1, rnames[int(rids[q, j])], ren[q, j]) for j in range(rfound[q])]
        assert len(rows) == len(expect)
        for (qi, pos, nm, val), (xl, xp, xn, xv) in zip(rows, expect):
            assert (int(qi), int(pos), nm) == (xl, xp, xn)
            assert abs(float(val) - xv) <= 5.000001e-7
