"""Top-k link-prediction queries, triple scoring and per-triple ranks
(kb2e_predict, kb2e_score_triples, kb2e_rank_triples) against the oracle.

The oracle for a query is plain numpy over orc.Model(..., transr_compat=False)
.energy: the energies of all |E| candidates, the known candidates dropped,
np.lexsort((ids, energy)), the first k.  All device arithmetic is FP64 in the
reference's order and ties break on the entity id, so ids, energies and found
counts must be EQUAL (no tolerance anywhere in this file except where a printed
%.6lf or evaluate()'s float means are compared).
"""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from gpu_common import MANIFEST, tiny
from kb2e_amd import data
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


class Setup:
    """An engine and the oracle on the same tables; oracle candidate rows are memoised."""

    def __init__(self, model, n, ds, *, distance=0, precision=64, seed=0, tables=None, **kw):
        self.ds, self.ne = ds, ds.num_entities
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
            en = self.m.energy
            self._rows[key] = np.array([en(key[0], x, key[1]) if key[2] else en(x, key[0], key[1])
                                        for x in range(self.ne)])
        return self._rows[key]

    @staticmethod
    def known(filt):
        """(e, r, side) -> the candidates a filter excludes."""
        table = {}
        for h, t, rr in np.asarray(filt).tolist():
            table.setdefault((h, rr, 1), set()).add(t)
            table.setdefault((t, rr, 0), set()).add(h)
        return table

    def expect(self, e, r, side, k, filt=None):
        if filt is None:
            known = {}
        else:
            if self._known is None or self._known[0] is not filt:
                self._known = (filt, self.known(filt))
            known = self._known[1]
        ids = np.full((len(e), k), -1, np.int32)
        en = np.full((len(e), k), np.inf)
        found = np.zeros(len(e), np.int32)
        for q in range(len(e)):
            row = self.row(e[q], r[q], side[q])
            keep = np.ones(self.ne, bool)
            keep[list(known.get((int(e[q]), int(r[q]), int(side[q])), ()))] = False
            cand = np.arange(self.ne)[keep]
            order = np.lexsort((cand, row[keep]))[:k]
            found[q] = len(order)
            ids[q, :len(order)] = cand[order]
            en[q, :len(order)] = row[keep][order]
        return ids, en, found

    def check(self, e, r, side, k, filt=None):
        e, r, side = (np.asarray(a, dtype=np.int32) for a in (e, r, side))
        ids, en, found = self.eng.predict(e, r, side, k, filt)
        xi, xe, xf = self.expect(e, r, side, k, filt)
        assert ids.shape == (len(e), k) and ids.dtype == np.int32 and en.dtype == np.float64
        assert np.array_equal(found, xf)
        assert np.array_equal(ids, xi)
        assert np.array_equal(en, xe)
        return ids, en, found


def _both_sides(test):
    """Every test triple as a tail query and a head query."""
    test = np.asarray(test)
    e = np.concatenate([test[:, 0], test[:, 1]])
    r = np.concatenate([test[:, 2], test[:, 2]])
    side = np.concatenate([np.ones(len(test), np.int32), np.zeros(len(test), np.int32)])
    return e.astype(np.int32), r.astype(np.int32), side


def _serial_transe_rows(ent, rel, fixed, r, side, l1):
    """TransE energies of every candidate against `fixed`, summed over the
    dimension in the reference's serial order (elementwise FP64 numpy steps):
    the oracle's bits (checked against orc.Model.energy where it is used)."""
    e = np.zeros(len(ent))
    for k in range(ent.shape[1]):
        d = (ent[:, k] - ent[fixed, k]) - rel[r, k] if side else (ent[fixed, k] - ent[:, k]) - rel[r, k]
        e += np.abs(d) if l1 else d * d
    return e


# ------------------------------------------------------------------ 1. models

@pytest.mark.parametrize("model,n,distance", [("E", 20, 0), ("E", 50, 1), ("H", 32, 0), ("R", 20, 0), ("R", 20, 1)])
def test_predict_models_tiny_all_test_queries(model, n, distance):
    """Every test triple of the golden tiny set on both sides (400 queries), k = 10,
    raw and filtered (train + valid + test)."""
    s = Setup(model, n, tiny(), distance=distance, seed=n + distance)
    e, r, side = _both_sides(s.ds.test)
    assert len(e) == 400
    s.check(e, r, side, 10)
    _, _, found = s.check(e, r, side, 10, s.filt)
    assert (found == 10).all()


# ------------------------------------------------------------------ 2. k and nq

@pytest.fixture(scope="module")
def tiny_e():
    return Setup("E", 20, tiny(), seed=1)


def test_predict_k_edges(tiny_e):
    s = tiny_e
    e, r, side = _both_sides(s.ds.test[:30])
    s.check(e, r, side, 1)
    s.check(e, r, side, 1, s.filt)
    # k = |E| filtered: found = 200 - known, then -1 / +inf
    ids, en, found = s.check(e, r, side, 200, s.filt)
    assert (found < 200).all() and (found > 0).all()
    for q in range(len(e)):
        assert (ids[q, found[q]:] == -1).all() and np.isposinf(en[q, found[q]:]).all()
        assert (ids[q, :found[q]] >= 0).all() and np.isfinite(en[q, :found[q]]).all()
    # k > |E|
    ids, en, found = s.check(e, r, side, 256)
    assert (found == 200).all()
    ids, en, found = s.check(e, r, side, 256, s.filt)
    assert (found < 200).all()


def test_predict_nq_edges(tiny_e):
    s = tiny_e
    t = s.ds.test
    s.check(t[:1, 0], t[:1, 2], [1], 10, s.filt)  # nq = 1
    s.check(t[:1, 1], t[:1, 2], [0], 10)
    # nq = 17: one past a tile of 16; sides and relations mixed in one call; relation 4 has no query
    pick = t[t[:, 2] != 4][:17]
    assert len(pick) == 17 and len(set(pick[:, 2].tolist())) >= 3
    side = (np.arange(17) % 3 != 0).astype(np.int32)
    e = np.where(side == 1, pick[:, 0], pick[:, 1])
    s.check(e, pick[:, 2], side, 10, s.filt)
    s.check(e, pick[:, 2], side, 7)
    # repeated identical queries (they share one known-candidate list)
    e2 = np.repeat(e[:3], 6)
    s.check(e2, np.repeat(pick[:3, 2], 6), np.repeat(side[:3], 6), 10, s.filt)


# ------------------------------------------------------------------ 3. |E|

@pytest.fixture(scope="module")
def set2085():
    ds = data.synthetic("small", seed=3, counts=(2085, 7, 3000, 50, 50))
    return Setup("E", 20, ds, seed=2)


def test_predict_several_entity_blocks_ragged(set2085):
    """2,085 entities: nine entity blocks, the last one ragged; the radix passes run
    (more keys than the sort buffer); k = 1024 fills it."""
    s = set2085
    e, r, side = _both_sides(s.ds.test[:12])
    s.check(e, r, side, 10, s.filt)
    s.check(e, r, side, 300)
    ids, _, found = s.check(e, r, side, 1024, s.filt)
    assert (found == 1024).all()


def test_predict_fewer_entities_than_a_block():
    ds = data.synthetic("small", seed=4, counts=(70, 3, 400, 20, 20))
    s = Setup("E", 20, ds, seed=3)
    e, r, side = _both_sides(ds.test)
    s.check(e, r, side, 64, s.filt)
    s.check(e, r, side, 64)
    _, _, found = s.check(e, r, side, 70)
    assert (found == 70).all()
    _, _, found = s.check(e, r, side, 70, s.filt)
    assert (found < 70).all()


@pytest.mark.parametrize("ne,keys_l2", [(14951, None), (14951, "0"), (19000, "0"), (3500, None), (3300, None)])
def test_predict_large_entity_counts(ne, keys_l2, monkeypatch):
    """14,951 entities (FB15k's): by default the key row is re-read from L2;
    KB2E_PREDICT_KEYS_L2=0 stages its 120 KB in LDS beside the scratch; at 19,000
    it no longer fits the 160 KB.  3,300 / 3,500: either side of the size up to
    which the row is staged by default (four workgroups a CU)."""
    if keys_l2 is not None:
        monkeypatch.setenv("KB2E_PREDICT_KEYS_L2", keys_l2)
    ds = data.synthetic("small", seed=5, counts=(ne, 5, 3000, 50, 50))
    s = Setup("E", 20, ds, seed=4)
    e, r, side = _both_sides(ds.test[:3])
    s.check(e, r, side, 10, s.filt)
    s.check(e, r, side, 1000)


# ------------------------------------------------------------------ 4. paths

def test_predict_keys_from_l2(tiny_e, set2085, monkeypatch):
    """KB2E_PREDICT_KEYS_L2=1: the select kernel re-reads the key row from L2."""
    monkeypatch.setenv("KB2E_PREDICT_KEYS_L2", "1")
    e, r, side = _both_sides(tiny_e.ds.test[:30])
    tiny_e.check(e, r, side, 10, tiny_e.filt)
    tiny_e.check(e, r, side, 200)
    e, r, side = _both_sides(set2085.ds.test[:12])
    set2085.check(e, r, side, 10, set2085.filt)
    set2085.check(e, r, side, 1024, set2085.filt)


def test_predict_chunked_key_buffer(tiny_e, monkeypatch):
    """KB2E_PREDICT_CHUNK_ROWS=3 with 17 queries: six chunks, the last one short,
    relations spanning chunk boundaries."""
    monkeypatch.setenv("KB2E_PREDICT_CHUNK_ROWS", "3")
    s = tiny_e
    pick = s.ds.test[:17]
    side = (np.arange(17) % 2).astype(np.int32)
    e = np.where(side == 1, pick[:, 0], pick[:, 1])
    s.check(e, pick[:, 2], side, 10, s.filt)
    s.check(e, pick[:, 2], side, 200, s.filt)


@pytest.mark.parametrize("model,n,rows_l2", [("E", 200, "0"), ("E", 512, "0"), ("R", 160, "0"), ("E", 50, "1"),
                                             ("H", 32, "1")])
def test_predict_wide_rows_and_l2_rows(model, n, rows_l2, monkeypatch):
    """Wide dims, and KB2E_EVAL_ROWS_L2=1: the score kernel reads the query rows
    from the projection table instead of LDS (the evaluator's fallback)."""
    monkeypatch.setenv("KB2E_EVAL_ROWS_L2", rows_l2)
    s = Setup(model, n, tiny(), seed=n)
    e, r, side = _both_sides(s.ds.test[:10])
    s.check(e, r, side, 10, s.filt)
    s.check(e, r, side, 10)


# ------------------------------------------------------------------ 5. ties

def test_predict_ties_break_on_entity_id():
    ds = tiny()
    ent, rel, _ = _tables("E", ds, 20, 5)
    h, r = 40, 3
    for x in (5, 9, 13):
        ent[x] = ent[h] + rel[r]
    s = Setup("E", 20, ds, tables=(ent, rel, None))
    row = s.row(h, r, 1)
    assert row[5] == row[9] == row[13] and (np.delete(row, [5, 9, 13]) > row[5]).all()
    ids, _, _ = s.check([h], [r], [1], 2)
    assert ids[0].tolist() == [5, 9]
    ids, _, _ = s.check([h], [r], [1], 3)
    assert ids[0].tolist() == [5, 9, 13]
    ids, _, _ = s.check([h], [r], [1], 4)
    assert ids[0, :3].tolist() == [5, 9, 13]
    filt = np.array([(h, 9, r)], dtype=np.int32)
    ids, _, _ = s.check([h], [r], [1], 2, filt)
    assert ids[0].tolist() == [5, 13]


def test_predict_more_ties_than_the_sort_buffer():
    """1,192 candidates share the smallest energy bit for bit, more than the 1,024
    pairs the select kernel sorts: all eight radix digits are fixed and the
    tied keys are taken in ascending id order."""
    ds = data.synthetic("small", seed=3, counts=(2085, 7, 3000, 50, 50))
    ent, rel, _ = _tables("E", ds, 20, 6)
    h, r = 6, 2  # 6 % 7 >= 4: not one of the tied rows
    tied = [x for x in range(2085) if x % 7 < 4]
    ent[tied] = ent[h] + rel[r]
    s = Setup("E", 20, ds, tables=(ent, rel, None))
    row = s.row(h, r, 1)
    assert len(tied) > 1024 and (row[tied] == row[tied[0]]).all() and (np.delete(row, tied) > row[tied[0]]).all()
    ids, _, _ = s.check([h], [r], [1], 10)
    assert ids[0].tolist() == tied[:10]
    ids, _, _ = s.check([h], [r], [1], 1024)
    assert ids[0].tolist() == tied[:1024]
    filt = np.array([(h, tied[0], r), (h, tied[700], r)], dtype=np.int32)
    ids, _, _ = s.check([h, h], [r, r], [1, 1], 1024, filt)
    assert ids[0].tolist() == [x for x in tied if x not in (tied[0], tied[700])][:1024]


# ------------------------------------------------------------------ 6. FP32 tables

@pytest.mark.parametrize("model,n,distance", [("E", 20, 0), ("H", 32, 0), ("R", 20, 1)])
def test_predict_fp32_tables(model, n, distance):
    """precision=32: the tables are widened to FP64 first, so the oracle on the
    tables rounded through float32 gives the same bits."""
    s = Setup(model, n, tiny(), distance=distance, precision=32, seed=7)
    e, r, side = _both_sides(s.ds.test[:40])
    s.check(e, r, side, 10, s.filt)
    trip = s.ds.test[:50]
    exp = np.array([s.m.energy(int(h), int(t), int(rr)) for h, t, rr in trip])
    assert np.array_equal(s.eng.score(trip), exp)


# ------------------------------------------------------------------ 7. score

@pytest.mark.parametrize("model,n,distance", [("E", 20, 0), ("E", 50, 1), ("H", 32, 0), ("R", 20, 0), ("R", 100, 1),
                                             ("R", 160, 0)])
def test_score_triples_bit_equal(model, n, distance):
    """300 triples with repeats; TransR n = 20, 100, 160: one, two, three elements a lane."""
    s = Setup(model, n, tiny(), distance=distance, seed=8)
    rng = np.random.default_rng(n)
    trip = np.concatenate([s.ds.test[:150], s.ds.train[rng.integers(0, len(s.ds.train), 100)], s.ds.test[:50]])
    trip[200:210, 1] = trip[200:210, 0]  # head == tail
    assert len(trip) == 300
    got = s.eng.score(trip)
    exp = np.array([s.m.energy(int(h), int(t), int(r)) for h, t, r in trip])
    assert got.dtype == np.float64 and got.shape == (300,)
    assert np.array_equal(got, exp)
    assert np.array_equal(s.eng.score(trip[:1]), exp[:1])


# ------------------------------------------------------------------ 8. rank_triples

def _oracle_ranks(ent, rel, test, filt, l1=True):
    known = {}
    for h, t, r in np.asarray(filt).tolist():
        known.setdefault((h, r, 1), []).append(t)
        known.setdefault((t, r, 0), []).append(h)
    ranks = np.zeros((len(test), 4), np.int64)
    for i, (h, t, r) in enumerate(np.asarray(test).tolist()):
        for side, fixed, truth in ((0, t, h), (1, h, t)):
            row = _serial_transe_rows(ent, rel, fixed, r, side, l1)
            above = row < row[truth]
            above[truth] = False
            ranks[i, 2 * side] = 1 + above.sum()
            above[known.get((fixed, r, side), [])] = False
            ranks[i, 2 * side + 1] = 1 + above.sum()
    return ranks


@pytest.mark.parametrize("which", ["tiny", "small"])
def test_rank_triples_match_oracle_and_evaluate(which):
    ds = tiny() if which == "tiny" else data.synthetic("small", seed=3)
    n = 50
    s = Setup("E", n, ds, seed=0)
    ent, rel, _ = s.tables
    filt = np.concatenate([ds.test, ds.train, ds.valid])
    # the vectorised serial-order energies are the oracle's, bit for bit
    for h, t, r in ds.test[:5].tolist():
        assert np.array_equal(_serial_transe_rows(ent, rel, h, r, 1, True),
                              np.array([s.m.energy(h, x, r) for x in range(ds.num_entities)]))
        assert np.array_equal(_serial_transe_rows(ent, rel, t, r, 0, True),
                              np.array([s.m.energy(x, t, r) for x in range(ds.num_entities)]))
    ranks = s.eng.rank_triples(ds.test, filt)
    assert ranks.shape == (len(ds.test), 4) and ranks.dtype == np.int64
    assert np.array_equal(ranks, _oracle_ranks(ent, rel, ds.test, filt))
    res = s.eng.evaluate(ds.test, filt)
    assert ranks[:, [0, 2]].mean() == pytest.approx(res["raw_rank"], abs=1e-12)
    assert ranks[:, [1, 3]].mean() == pytest.approx(res["filtered_rank"], abs=1e-12)
    assert (ranks[:, [0, 2]] <= 10).mean() == pytest.approx(res["raw_hits10"], abs=1e-12)
    assert (ranks[:, [1, 3]] <= 10).mean() == pytest.approx(res["filtered_hits10"], abs=1e-12)
    # the caller's order, not the evaluator's relation-grouped one
    perm = np.random.default_rng(1).permutation(len(ds.test))[:64]
    assert np.array_equal(s.eng.rank_triples(ds.test[perm], filt), ranks[perm])


def test_rank_triples_agree_with_predict(tiny_e):
    """k = |E|, no filter: the truth's position in the tail (head) query's list is
    its raw tail (head) rank, on tables without ties."""
    s = tiny_e
    ds = s.ds
    filt = np.concatenate([ds.test, ds.train, ds.valid])
    assert s.m.evaluate(ds.test, filt)["ties"] == 0
    ranks = s.eng.rank_triples(ds.test, filt)
    e, r, side = _both_sides(ds.test)
    ids, _, found = s.eng.predict(e, r, side, ds.num_entities)
    assert (found == ds.num_entities).all()
    nt = len(ds.test)
    for i, (h, t, _) in enumerate(ds.test.tolist()):
        assert int(np.nonzero(ids[i] == t)[0][0]) + 1 == ranks[i, 2]
        assert int(np.nonzero(ids[nt + i] == h)[0][0]) + 1 == ranks[i, 0]


# ------------------------------------------------------------------ 9. contract

def test_bad_arguments_are_refused(tiny_e):
    s = tiny_e
    eng, ne, nr = s.eng, s.ds.num_entities, s.ds.num_relations
    ok = ([3], [2], [1])
    eng.predict(*ok, 5)
    with pytest.raises(EngineError):
        eng.predict(*ok, 0)
    with pytest.raises(EngineError):
        eng.predict(*ok, 1025)
    with pytest.raises(EngineError):
        eng.predict([3], [2], [2], 5)
    with pytest.raises(EngineError):
        eng.predict([ne], [2], [1], 5)
    with pytest.raises(EngineError):
        eng.predict([3], [-1], [1], 5)
    with pytest.raises(EngineError):
        eng.predict([3], [nr], [0], 5)
    with pytest.raises(EngineError):
        eng.predict(*ok, 5, np.array([(0, ne, 0)], dtype=np.int32))
    with pytest.raises(EngineError):
        eng.predict(*ok, 5, np.array([(0, 1, -1)], dtype=np.int32))
    with pytest.raises(EngineError):
        eng.predict(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), 5)
    with pytest.raises(EngineError):
        eng.score(np.array([(0, ne, 0)], dtype=np.int32))
    with pytest.raises(EngineError):
        eng.score(np.array([(0, 1, nr)], dtype=np.int32))
    with pytest.raises(EngineError):
        eng.score(np.zeros((0, 3), np.int32))
    with pytest.raises(EngineError):
        eng.rank_triples(np.array([(ne, 0, 0)], dtype=np.int32), s.filt)
    # still usable
    s.check(*ok, 5)


@pytest.mark.parametrize("model,n", [("E", 20), ("R", 20)])
def test_calls_leave_the_context_unchanged(model, n):
    """device_bytes() before == after each call (every buffer freed), the tables
    and the TransR work vectors untouched, profiling families reported."""
    s = Setup(model, n, tiny(), seed=9)
    eng, ds = s.eng, s.ds
    if model == "R":
        eng.upload_triples(ds.train)  # (the work vectors exist once the triples are up)
        eng.upload_params(*s.tables)
        eng.set_transr_work(np.arange(n) * 0.5, np.arange(n) * -0.25)
    before = eng.download_params()
    work = eng.transr_work() if model == "R" else None
    e, r, side = _both_sides(ds.test[:20])
    eng.profile(True)
    b0 = eng.device_bytes()
    eng.predict(e, r, side, 10, s.filt)
    assert eng.device_bytes() == b0
    eng.predict(e, r, side, 10)
    assert eng.device_bytes() == b0
    eng.score(ds.test)
    assert eng.device_bytes() == b0
    eng.rank_triples(ds.test[:20], s.filt)
    assert eng.device_bytes() == b0
    with pytest.raises(EngineError):
        eng.predict(e, r, side, 0)
    assert eng.device_bytes() == b0
    for fam, launches in (("predict_score", 2), ("predict_mask", 1), ("predict_select", 2)):
        ms, cnt = eng.profile_query(fam)
        assert cnt == launches and ms > 0, fam
    eng.profile(False)
    after = eng.download_params()
    for a, b in zip(before, after):
        assert (a is None and b is None) or np.array_equal(a, b)
    if model == "R":
        hw, tw = eng.transr_work()
        assert np.array_equal(hw, work[0]) and np.array_equal(tw, work[1])
        # (and the energies did not see those work vectors)
        s.check(e[:4], r[:4], side[:4], 5)


# ------------------------------------------------------------------ 10. CLI

def test_predict_cli_matches_engine(tmp_path):
    name = "transe_l1_bern"
    f = MANIFEST["runs"][name]["flags"]
    ds = tiny()
    d = os.path.join(GOLDEN, name)
    qfile = tmp_path / "queries.txt"
    # (line 2 names an unknown entity: reported and skipped)
    qfile.write_text("/m/e25\t?\t/r/r4\n?\t/m/e58\t/r/r1\n/m/nobody\t?\t/r/r4\n/m/e114\t?\t/r/r4\n?\t/m/e105\t/r/r0\n")
    e, r, side = [25, 58, 114, 105], [4, 1, 4, 0], [1, 0, 1, 0]
    lines = [0, 1, 3, 4]
    exe = tmp_path / "predictTransE"
    exe.symlink_to(os.path.join(ROOT, "bin", "kb2e"))
    base = [str(exe), "--datadir", os.path.join(GOLDEN, "tiny"), "--outdir", d, "--size", str(f["size"]), "--method",
            str(f["method"]), "--distance", str(f["distance"]), "--queries", str(qfile)]
    eng = Engine("E", f["size"], ds.num_entities, ds.num_relations, distance=f["distance"])
    eng.upload_params(data.read_table(os.path.join(d, "entity2vec.bern"), ds.num_entities, f["size"]),
                      data.read_table(os.path.join(d, "relation2vec.bern"), ds.num_relations, f["size"]))
    names = {v: k for k, v in data._load_ids(os.path.join(GOLDEN, "tiny", "entity2id.txt")).items()}
    filt = np.concatenate([ds.test, ds.train, ds.valid])
    for extra, k, fl in (([], 10, filt), (["--topk", "3", "--filtered", "0"], 3, None)):
        res = subprocess.run(base + extra, capture_output=True, text=True, timeout=300, check=True)
        assert "Head entity found in triple file that was not found in the identity file: /m/nobody" in res.stdout
        rows = [l.split("\t") for l in res.stdout.splitlines() if l.count("\t") == 3 and l.split("\t")[0].isdigit()]
        ids, en, found = eng.predict(e, r, side, k, fl)
        assert (found == k).all() and len(rows) == 4 * k
        it = iter(rows)
        for q in range(4):
            for j in range(k):
                qi, pos, nm, val = next(it)
                assert (int(qi), int(pos), nm) == (lines[q], j + 1, names[int(ids[q, j])])
                assert abs(float(val) - en[q, j]) <= 5.000001e-7
