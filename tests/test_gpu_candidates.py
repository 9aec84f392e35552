"""Candidate lists (kb2e_score_candidates, kb2e_rank_candidates) against the oracle.

The oracle is orc.Model(..., transr_compat=False).energy on the same tables (FP32
contexts: on the tables rounded through float32); a rank is a numpy count over
those energies.  All device arithmetic is FP64 in the reference's order, so
energies must be EQUAL bit for bit and ranks and counts equal as integers (no
tolerance anywhere in this file).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from gpu_common import MANIFEST, golden_engine, tiny
from kb2e_amd import data, linkpred
from kb2e_amd.engine import Engine, EngineError, lib
from oracle import orc

pytestmark = pytest.mark.gpu

KNOBS = ("KB2E_CANDIDATES_CHUNK", "KB2E_CANDIDATES_PROJECT", "KB2E_CANDIDATES_ROWS")
COUNTERS = ("listings", "items", "chunks", "projections", "probes")


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


def _counters(eng):
    return {c: eng.counter("candidates_" + c) for c in COUNTERS}


class Setup:
    """An engine and the oracle on the same tables; oracle energies are computed
    once per triple and kept."""

    def __init__(self, model, n, ne, nr, tables, *, distance=0, precision=64):
        self.model, self.n, self.ne, self.nr = model, n, ne, nr
        self.eng = Engine(model, n, ne, nr, distance=distance, precision=precision)
        self.eng.upload_params(*tables)
        tables = _f32(tables) if precision == 32 else tables
        odist = 0 if (model == "H" or distance == 0) else 1  # (a TransH context is L1)
        self.m = orc.Model(model, n, ne, nr, distance=odist, transr_compat=False)
        self.m.set_tables(*tables)
        self._e = {}

    def energy(self, h, t, r):
        key = (int(h), int(t), int(r))
        if key not in self._e:
            self._e[key] = self.m.energy(*key)
        return self._e[key]

    def triple(self, e, r, s, x):
        return (e, x, r) if s == 1 else (x, e, r)

    def expect_scores(self, ent, rel, side, cands, lists=None):
        out = []
        for q in range(len(ent)):
            ids = cands[q if lists is None else lists[q]]
            out.append(np.array([self.energy(*self.triple(ent[q], rel[q], side[q], int(x))) for x in ids], np.float64))
        return out

    def check_scores(self, ent, rel, side, cands, lists=None):
        got = self.eng.score_candidates(ent, rel, side, cands, lists=lists)
        exp = self.expect_scores(ent, rel, side, cands, lists)
        assert len(got) == len(exp) == len(ent)
        for q, (g, x) in enumerate(zip(got, exp)):
            assert g.dtype == np.float64 and g.shape == x.shape, q
            assert np.array_equal(_bits(g), _bits(x)), q
        # and the parent's only route: kb2e_score_triples on the expanded triples
        rows = [self.triple(int(ent[q]), int(rel[q]), int(side[q]), int(x)) for q in range(len(ent))
                for x in cands[q if lists is None else lists[q]]]
        if rows:
            flat = np.concatenate(got)
            assert np.array_equal(_bits(flat), _bits(self.eng.score(np.array(rows, np.int32))))
        return got

    def expect_ranks(self, ent, rel, side, truth, cands, filt, lists=None):
        known = set() if filt is None else {tuple(int(v) for v in row) for row in np.asarray(filt).reshape(-1, 3)}
        ranks = np.zeros((len(ent), 2), np.int64)
        counted = np.zeros((len(ent), 2), np.int64)
        energies = self.expect_scores(ent, rel, side, cands, lists)
        for q in range(len(ent)):
            ids = np.asarray(cands[q if lists is None else lists[q]], dtype=np.int64)
            te = self.energy(*self.triple(ent[q], rel[q], side[q], int(truth[q])))
            takes = ids != truth[q]
            free = np.array([self.triple(int(ent[q]), int(rel[q]), int(side[q]), int(x)) not in known for x in ids], bool)
            below = energies[q] < te
            ranks[q] = 1 + (takes & below).sum(), 1 + (takes & below & free).sum()
            counted[q] = takes.sum(), (takes & free).sum()
        return ranks, counted

    def check_ranks(self, ent, rel, side, truth, cands, filt, lists=None):
        ranks, counted = self.eng.rank_candidates(ent, rel, side, truth, cands, filt, lists=lists)
        er, ec = self.expect_ranks(ent, rel, side, truth, cands, filt, lists)
        assert ranks.dtype == counted.dtype == np.int64 and ranks.shape == counted.shape == (len(ent), 2)
        assert np.array_equal(ranks, er)
        assert np.array_equal(counted, ec)
        return ranks, counted


def _queries(rng, nq, ne, nr):
    return (rng.integers(0, ne, nq).astype(np.int32), rng.integers(0, nr, nq).astype(np.int32),
            (np.arange(nq) % 2).astype(np.int32))


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    for key in KNOBS:
        monkeypatch.delenv(key, raising=False)


# ------------------------------------------------------------------ 1. energy bits

# 1, 5, 65: odd widths (the pair loads' last element); 15, 16, 17: the edge of a
# staged panel of 16 columns; 64, 65, 130: one, just over one and over two waves
# of anchor columns; 512: the widest context there is (kb2e_create refuses more), so
# the rows a work item keeps in LDS have no width beyond which another path runs.
WIDTHS = (1, 5, 15, 16, 17, 64, 65, 130)
ENERGY_CASES = ([(m, n, d, 64) for n in WIDTHS for m, d in (("E", 0), ("E", 1), ("H", 0), ("R", 0), ("R", 1))]
                + [(m, n, d, 32) for n in (5, 64, 130) for m, d in (("E", 1), ("H", 0), ("R", 0))]
                + [("E", 512, 0, 64), ("H", 512, 0, 64), ("R", 512, 0, 64), ("E", 512, 1, 32)])


@pytest.mark.parametrize("model,n,distance,precision", ENERGY_CASES)
def test_score_candidates_energy_bits(model, n, distance, precision, monkeypatch):
    """12 queries of both sides on ragged private lists (0..70 listings) of
    |E| = 40, against the oracle and against Engine.score on the expanded
    triples; TransE / TransH with both ways of reading the listings' rows,
    TransR with both projections."""
    ne, nr, nq = 40, 3, 12
    s = Setup(model, n, ne, nr, _random_tables(model, ne, nr, n, seed=n + distance), distance=distance,
              precision=precision)
    rng = np.random.default_rng(n * 7 + distance)
    ent, rel, side = _queries(rng, nq, ne, nr)
    cands = [rng.integers(0, ne, int(m)).astype(np.int32) for m in rng.integers(0, 71, nq)]
    cands[3] = np.array([ent[3]], np.int32)  # the anchor itself
    base = s.check_scores(ent, rel, side, cands)
    knob, values = ("KB2E_CANDIDATES_PROJECT", ("compact", "full")) if model == "R" else \
        ("KB2E_CANDIDATES_ROWS", ("stream", "panel"))
    for v in values:
        monkeypatch.setenv(knob, v)
        got = s.eng.score_candidates(ent, rel, side, cands)
        assert all(np.array_equal(_bits(g), _bits(b)) for g, b in zip(got, base)), v


# ------------------------------------------------------------------ 2. list shapes

@pytest.mark.parametrize("model", ["E", "H", "R"])
def test_list_shapes_shared_private_and_empty(model):
    """|E| = 97 and lists of 0, 1, 63, 64, 65 and 300 listings (duplicates are
    forced), named by one query or by several; lists = NULL; a list that names
    the anchor and one that names the truth."""
    ne, nr, n = 97, 4, 20
    s = Setup(model, n, ne, nr, _random_tables(model, ne, nr, n, seed=3))
    rng = np.random.default_rng(17)
    cands = [rng.integers(0, ne, m).astype(np.int32) for m in (0, 1, 63, 64, 65, 300)]
    lists = np.array([0, 1, 2, 3, 4, 5, 5, 5, 2, 0, 4], np.int32)
    ent, rel, side = _queries(rng, len(lists), ne, nr)
    truth = rng.integers(0, ne, len(lists)).astype(np.int32)
    cands[1][0] = ent[1]        # a list naming its anchor
    truth[4] = cands[4][7]      # a truth in its list, listed ...
    cands[4][40] = truth[4]     # ... twice
    known = np.array([s.triple(int(ent[q]), int(rel[q]), int(side[q]), int(x)) for q in (2, 5, 6)
                      for x in cands[lists[q]][::3]], np.int32)
    got = s.check_scores(ent, rel, side, cands, lists)
    assert [len(g) for g in got] == [0, 1, 63, 64, 65, 300, 300, 300, 63, 0, 65]
    c = _counters(s.eng)
    assert c["listings"] == 1221 and c["chunks"] == 1 and c["items"] == 1 + 1 + 1 + 2 + 3 * 5 + 1 + 2
    s.check_ranks(ent, rel, side, truth, cands, known, lists)
    c = _counters(s.eng)
    assert c["items"] == 1 + 1 + 2 + 2 + 3 * 5 + 1 + 2 and c["probes"] > 0  # (63 listings a work item)
    # lists = NULL: one list per query
    ent6, rel6, side6 = ent[:6], rel[:6], side[:6]
    s.check_scores(ent6, rel6, side6, cands)
    s.check_ranks(ent6, rel6, side6, truth[:6], cands, known)
    # shared or copied per query: the same answers
    copied = [cands[l].copy() for l in lists]
    for a, b in zip(got, s.eng.score_candidates(ent, rel, side, copied)):
        assert np.array_equal(_bits(a), _bits(b))


# ------------------------------------------------------------------ 3. ranks

@pytest.mark.parametrize("model,distance", [("E", 0), ("E", 1), ("H", 0), ("R", 0), ("R", 1)])
def test_rank_candidates_filter_ties_and_empty_lists(model, distance):
    """Entities 5, 6 and 7 share one row, so listings 6 and 7 tie with the truth 5
    bit for bit and must not count; the filter holds listings, the truth's own
    triple and duplicates; an empty list gives rank 1, counted 0."""
    ne, nr, n = 60, 3, 24
    tables = _random_tables(model, ne, nr, n, seed=5)
    tables[0][6] = tables[0][5]
    tables[0][7] = tables[0][5]
    s = Setup(model, n, ne, nr, tables, distance=distance)
    rng = np.random.default_rng(23)
    nq = 14
    ent, rel, side = _queries(rng, nq, ne, nr)
    ent[ent == 5] = 8
    truth = rng.integers(8, ne, nq).astype(np.int32)
    truth[:4] = 5
    cands = [rng.integers(0, ne, int(m)).astype(np.int32) for m in rng.integers(20, 140, nq)]
    for q in range(4):
        cands[q][:6] = [6, 7, 5, 6, truth[q], 7]
        assert s.energy(*s.triple(ent[q], rel[q], side[q], 6)) == s.energy(*s.triple(ent[q], rel[q], side[q], 5))
    cands[9] = np.zeros(0, np.int32)
    cands[10] = np.array([truth[10]] * 3, np.int32)  # nothing but the truth
    rows = [s.triple(int(ent[q]), int(rel[q]), int(side[q]), int(x)) for q in range(nq) for x in cands[q][::2]]
    rows += [s.triple(int(ent[q]), int(rel[q]), int(side[q]), int(truth[q])) for q in range(nq)]
    filt = np.array(rows + rows[:50], np.int32)  # (a set: duplicates count once)
    ranks, counted = s.check_ranks(ent, rel, side, truth, cands, filt)
    assert ranks[9].tolist() == [1, 1] and counted[9].tolist() == [0, 0]
    assert ranks[10].tolist() == [1, 1] and counted[10].tolist() == [0, 0]
    assert (ranks[:, 1] <= ranks[:, 0]).all() and (ranks[:, 0] > ranks[:, 1]).any()  # (the filter bites)
    assert (ranks > 1).any()
    probes_all = s.eng.counter("candidates_probes")
    assert probes_all == counted[:, 0].sum()
    # no filter at all
    r0, c0 = s.check_ranks(ent, rel, side, truth, cands, None)
    assert np.array_equal(r0[:, 0], r0[:, 1]) and np.array_equal(c0[:, 0], c0[:, 1]) and np.array_equal(r0[:, 0], ranks[:, 0])
    assert s.eng.counter("candidates_probes") == 0
    # counted == NULL: the same ranks from fewer probes (only listings below the truth are looked up)
    off = np.zeros(nq + 1, np.int64)
    off[1:] = np.cumsum([len(c) for c in cands])
    flat = np.concatenate(cands).astype(np.int32)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    lp = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))  # noqa: E731
    fc = [np.ascontiguousarray(filt[:, k]) for k in range(3)]
    out = np.zeros((nq, 2), np.int64)
    assert lib().kb2e_rank_candidates(s.eng.h, ip(ent), ip(rel), ip(side), ip(truth), None, nq, lp(off), ip(flat), nq,
                                      ip(fc[0]), ip(fc[1]), ip(fc[2]), len(filt), lp(out), None) == 0
    assert np.array_equal(out, ranks)
    assert s.eng.counter("candidates_probes") == (ranks[:, 0] - 1).sum() < probes_all


# ------------------------------------------------------------------ 4. the full list

@pytest.mark.parametrize("name", ["transe_l1_bern", "transh_bern", "transr_fixed"])
def test_full_list_gives_rank_triples_columns(name):
    """One shared list that names every entity once: the two columns are
    kb2e_rank_triples' (0, 1) for the head side and (2, 3) for the tail side."""
    eng, run, ds, _ = golden_engine(name)
    eng.train_epoch()
    filt = np.concatenate([ds.train, ds.valid, ds.test]).astype(np.int32)
    want = eng.rank_triples(ds.test, filt)
    ent, rel, side, truth = linkpred.side_queries(ds.test)
    every = np.arange(ds.num_entities, dtype=np.int32)
    ranks, counted = eng.rank_candidates(ent, rel, side, truth, [every], filt, lists=np.zeros(len(ent), np.int32))
    assert np.array_equal(ranks.reshape(-1, 4), want)
    assert (counted[:, 0] == ds.num_entities - 1).all() and (counted[:, 1] <= counted[:, 0]).all()
    assert (want[:, [0, 2]] > 1).any()
    eng.close()


# ------------------------------------------------------------------ 5. invariance

@pytest.mark.parametrize("model", ["E", "H", "R"])
def test_results_do_not_depend_on_chunks_projection_or_sharing(model, monkeypatch):
    ne, nr, n, nq = 120, 5, 30, 40
    s = Setup(model, n, ne, nr, _random_tables(model, ne, nr, n, seed=9))
    rng = np.random.default_rng(41)
    ent, rel, side = _queries(rng, nq, ne, nr)
    truth = rng.integers(0, ne, nq).astype(np.int32)
    pools = [rng.integers(0, ne, int(m)).astype(np.int32) for m in (150, 70, 64, 1, 9, 130, 5, 200, 63, 33)]
    lists = (rel * 2 + side).astype(np.int32)  # one pool per relation and slot
    filt = np.array([s.triple(int(ent[q]), int(rel[q]), int(side[q]), int(x)) for q in range(nq)
                     for x in pools[lists[q]][::4]], np.int32)
    lens = np.array([len(pools[l]) for l in lists])
    scores = s.check_scores(ent, rel, side, pools, lists)
    base_c = _counters(s.eng)
    ranks = s.check_ranks(ent, rel, side, truth, pools, filt, lists)
    nrel = len(set(rel.tolist()))
    assert base_c["listings"] == lens.sum() and base_c["chunks"] == 1
    assert base_c["items"] == ((lens + 63) // 64).sum()
    assert base_c["projections"] == (nrel if model == "R" else 0)

    def same():
        got = s.eng.score_candidates(ent, rel, side, pools, lists=lists)
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got, scores))
        c = _counters(s.eng)
        r, k = s.eng.rank_candidates(ent, rel, side, truth, pools, filt, lists=lists)
        assert np.array_equal(r, ranks[0]) and np.array_equal(k, ranks[1])
        return c

    for project in (None, "compact", "full"):
        for chunk in ("1", "64", None):
            for key, v in (("KB2E_CANDIDATES_PROJECT", project), ("KB2E_CANDIDATES_CHUNK", chunk)):
                if v is None:
                    monkeypatch.delenv(key, raising=False)
                else:
                    monkeypatch.setenv(key, v)
            if project is not None and model != "R" and chunk is not None:
                continue  # (the projection knob is TransR's)
            c = same()
            assert c["listings"] == lens.sum() and c["items"] == base_c["items"]
            if chunk == "1":  # every query a chunk of its own
                assert c["chunks"] == nq and c["projections"] == (nq if model == "R" else 0)
            elif chunk == "64":  # greedy: queries are added while the listings stay within 64
                chunks, fill, rels, proj = 0, None, set(), 0
                for q in range(nq):
                    if fill is None or fill + lens[q] > 64:
                        chunks, fill, proj, rels = chunks + 1, 0, proj + len(rels), set()
                    fill += lens[q]
                    rels.add(int(rel[q]))
                proj += len(rels)
                assert chunks > 1 and c["chunks"] == chunks and c["projections"] == (proj if model == "R" else 0)
            else:
                assert c["chunks"] == 1 and c["projections"] == (nrel if model == "R" else 0)
    # a list given as shared or copied per query
    for key in KNOBS:
        monkeypatch.delenv(key, raising=False)
    copied = [pools[l].copy() for l in lists]
    got = s.eng.score_candidates(ent, rel, side, copied)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got, scores))
    r, k = s.eng.rank_candidates(ent, rel, side, truth, copied, filt)
    assert np.array_equal(r, ranks[0]) and np.array_equal(k, ranks[1])


# ------------------------------------------------------------------ 6. contract

@pytest.mark.parametrize("model,n", [("E", 20), ("H", 32), ("R", 20)])
def test_candidate_calls_leave_the_context_unchanged(model, n):
    ds = tiny()
    tables = _random_tables(model, 200, 10, n, seed=11)
    rng = np.random.default_rng(2)
    ent, rel, side = _queries(rng, 30, 200, 10)
    truth = rng.integers(0, 200, 30).astype(np.int32)
    cands = [rng.integers(0, 200, 90).astype(np.int32) for _ in range(30)]
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
            one = eng.score_candidates(ent, rel, side, cands)
            assert eng.device_bytes() == b0
            two = eng.score_candidates(ent, rel, side, cands)
            assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(one, two))
            r1 = eng.rank_candidates(ent, rel, side, truth, cands, ds.train)
            assert eng.device_bytes() == b0
            r2 = eng.rank_candidates(ent, rel, side, truth, cands, ds.train)
            assert np.array_equal(r1[0], r2[0]) and np.array_equal(r1[1], r2[1])
            for fam in ("candidates_score", "candidates_rank") + (("candidates_project",) if model == "R" else ()):
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


def test_candidate_calls_refuse_bad_arguments():
    ne, nr = 50, 4
    eng = Engine("E", 12, ne, nr)
    eng.upload_params(*_random_tables("E", ne, nr, 12, seed=13))
    b0 = eng.device_bytes()
    e, r, s, t = (np.array(v, np.int32) for v in ([1, 2], [0, 3], [0, 1], [4, 5]))
    cands = [np.array([1, 2, 3], np.int32), np.array([4], np.int32)]
    filt = np.array([(1, 2, 0)], np.int32)
    assert [len(x) for x in eng.score_candidates(e, r, s, cands)] == [3, 1]
    eng.rank_candidates(e, r, s, t, cands, filt)
    assert eng.device_bytes() == b0
    bad = [
        dict(entities=np.zeros(0, np.int32), relations=np.zeros(0, np.int32), side=np.zeros(0, np.int32),
             truth=np.zeros(0, np.int32)),                                   # nq < 1
        dict(candidates=[], lists=np.array([0, 0], np.int32)),               # nlists < 1
        dict(candidates=cands[:1]),                                          # lists == NULL, nlists != nq
        dict(lists=np.array([0, 2], np.int32)), dict(lists=np.array([-1, 0], np.int32)),
        dict(side=np.array([0, 2], np.int32)), dict(side=np.array([-1, 1], np.int32)),
        dict(entities=np.array([1, ne], np.int32)), dict(entities=np.array([-1, 2], np.int32)),
        dict(relations=np.array([0, nr], np.int32)), dict(relations=np.array([-1, 0], np.int32)),
        dict(candidates=[cands[0], np.array([ne], np.int32)]), dict(candidates=[np.array([-1], np.int32), cands[1]]),
    ]
    for kw in bad:
        a = dict(entities=e, relations=r, side=s, candidates=cands, lists=None)
        a.update({k: v for k, v in kw.items() if k != "truth"})
        with pytest.raises(EngineError, match="EINVAL"):
            eng.score_candidates(a["entities"], a["relations"], a["side"], a["candidates"], lists=a["lists"])
        with pytest.raises(EngineError, match="EINVAL"):
            eng.rank_candidates(a["entities"], a["relations"], a["side"], kw.get("truth", t), a["candidates"], filt,
                                lists=a["lists"])
        assert eng.device_bytes() == b0
    for tr in ([4, ne], [-1, 5]):  # truth
        with pytest.raises(EngineError, match="EINVAL"):
            eng.rank_candidates(e, r, s, np.array(tr, np.int32), cands, filt)
    for row in ((ne, 0, 0), (0, -1, 0), (0, 0, nr)):  # the filter
        with pytest.raises(EngineError, match="EINVAL"):
            eng.rank_candidates(e, r, s, t, cands, np.array([row], np.int32))
    assert eng.device_bytes() == b0
    # the C ABI itself: malformed offsets and NULL arrays with a count > 0
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    lp = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))  # noqa: E731
    flat = np.array([1, 2, 3, 4], np.int32)
    off = np.array([0, 3, 4], np.int64)
    en = np.zeros(4)
    dp = en.ctypes.data_as(C.POINTER(C.c_double))
    ranks, counted = np.zeros((2, 2), np.int64), np.zeros((2, 2), np.int64)
    f = [np.ascontiguousarray(filt[:, k]) for k in range(3)]
    score, rank = lib().kb2e_score_candidates, lib().kb2e_rank_candidates
    assert score(eng.h, ip(e), ip(r), ip(s), None, 2, lp(off), ip(flat), 2, dp) == 0
    assert rank(eng.h, ip(e), ip(r), ip(s), ip(t), None, 2, lp(off), ip(flat), 2, None, None, None, 0, lp(ranks),
                lp(counted)) == 0
    for o in ([1, 3, 4], [0, 4, 3], [0, 3, 2 ** 31]):
        o = np.array(o, np.int64)
        assert score(eng.h, ip(e), ip(r), ip(s), None, 2, lp(o), ip(flat), 2, dp) == 1
        assert rank(eng.h, ip(e), ip(r), ip(s), ip(t), None, 2, lp(o), ip(flat), 2, None, None, None, 0, lp(ranks),
                    lp(counted)) == 1
    for args in ((None, ip(r), ip(s), None, 2, lp(off), ip(flat), 2, dp), (ip(e), None, ip(s), None, 2, lp(off), ip(flat), 2, dp),
                 (ip(e), ip(r), None, None, 2, lp(off), ip(flat), 2, dp), (ip(e), ip(r), ip(s), None, 2, None, ip(flat), 2, dp),
                 (ip(e), ip(r), ip(s), None, 2, lp(off), None, 2, dp), (ip(e), ip(r), ip(s), None, 2, lp(off), ip(flat), 2, None),
                 (ip(e), ip(r), ip(s), None, 0, lp(off), ip(flat), 2, dp), (ip(e), ip(r), ip(s), None, 2, lp(off), ip(flat), 0, dp)):
        assert score(eng.h, *args) == 1
    tail = (None, 2, lp(off), ip(flat), 2)
    assert rank(eng.h, ip(e), ip(r), ip(s), None, *tail, None, None, None, 0, lp(ranks), lp(counted)) == 1
    assert rank(eng.h, ip(e), ip(r), ip(s), ip(t), *tail, None, None, None, 0, None, lp(counted)) == 1
    assert rank(eng.h, ip(e), ip(r), ip(s), ip(t), *tail, None, ip(f[1]), ip(f[2]), 1, lp(ranks), lp(counted)) == 1
    assert rank(eng.h, ip(e), ip(r), ip(s), ip(t), *tail, ip(f[0]), ip(f[1]), ip(f[2]), -1, lp(ranks), lp(counted)) == 1
    assert rank(eng.h, ip(e), ip(r), ip(s), ip(t), *tail, ip(f[0]), ip(f[1]), ip(f[2]), 1, lp(ranks), lp(counted)) == 0
    assert eng.device_bytes() == b0
    with pytest.raises(EngineError):
        eng.counter("candidates_nothing")
    # a context without embeddings is a state error, not a crash
    fresh = Engine("E", 12, ne, nr)
    with pytest.raises(EngineError, match="ESTATE"):
        fresh.score_candidates(e, r, s, cands)
    with pytest.raises(EngineError, match="ESTATE"):
        fresh.rank_candidates(e, r, s, t, cands, filt)
    # still usable
    assert [len(x) for x in eng.score_candidates(e, r, s, cands)] == [3, 1]


def test_rerank_sorts_on_energy_id_and_position():
    ne, nr, n = 40, 2, 10
    tables = _random_tables("E", ne, nr, n, seed=21)
    tables[0][9] = tables[0][4]  # entities 4 and 9 tie
    eng = Engine("E", n, ne, nr)
    eng.upload_params(*tables)
    cands = [np.array([9, 3, 4, 9, 20, 4], np.int32), np.zeros(0, np.int32)]
    e, r, s = np.array([1, 2], np.int32), np.array([0, 1], np.int32), np.array([1, 0], np.int32)
    en = eng.score_candidates(e, r, s, cands)
    top = eng.rerank(e, r, s, cands, 4)
    order = sorted(range(6), key=lambda j: (en[0][j], cands[0][j], j))[:4]
    assert top[0][0].tolist() == cands[0][order].tolist() and top[0][2].tolist() == order
    assert np.array_equal(_bits(top[0][1]), _bits(en[0][order]))
    assert len(top[1][0]) == 0
    assert len(eng.rerank(e, r, s, cands, 100)[0][0]) == 6


# ------------------------------------------------------------------ 7. drivers

@pytest.fixture(scope="module")
def trained():
    """The golden TransE run after one epoch, with what rank_triples says of its test set."""
    eng, run, ds, _ = golden_engine("transe_l1_bern")
    eng.train_epoch()
    filt = np.concatenate([ds.train, ds.valid, ds.test]).astype(np.int32)
    yield eng, ds, filt, eng.rank_triples(ds.test, filt)
    eng.close()


def test_sampled_evaluation_on_every_entity_is_rank_triples(trained):
    eng, ds, filt, full = trained
    res = linkpred.sampled_evaluation(eng, ds.test, filt, negatives=np.arange(ds.num_entities))
    assert np.array_equal(res["ranks"], full)
    for col, cols in (("raw", [0, 2]), ("filtered", [1, 3])):
        want = linkpred.rank_metrics(full[:, cols])
        assert {k: res[col][k] for k in want} == want
        assert res[col]["hits@3"] == float((full[:, cols] <= 3).mean())
    assert res["counted"]["raw"] == 2 * len(ds.test) * (ds.num_entities - 1)
    # drawn negatives: seeded, and a rank among 50 is at most 51
    a = linkpred.sampled_evaluation(eng, ds.test, filt, negatives=50, seed=1)
    b = linkpred.sampled_evaluation(eng, ds.test, filt, negatives=50, seed=1)
    assert np.array_equal(a["ranks"], b["ranks"]) and a["ranks"].max() <= 51 and a["ranks"].min() >= 1
    assert a["counted"]["raw"] <= 2 * len(ds.test) * 50


def test_type_constrained_evaluation_against_brute_force(trained):
    eng, ds, filt, full = trained
    res = linkpred.type_constrained_evaluation(eng, ds)
    con = res["constrained"]
    assert np.array_equal(res["unconstrained"]["ranks"], full)
    assert (con["ranks"][:, [1, 3]] <= full[:, [1, 3]]).all() and (con["ranks"] <= full).all()
    assert (con["ranks"] < full).any()
    # numpy over Engine.score on the expanded triples
    pools = linkpred.slot_pools(filt, ds.num_relations)
    known = {tuple(row) for row in filt.tolist()}
    want = np.zeros((len(ds.test), 4), np.int64)
    total = [0, 0]
    for i, (h, t, r) in enumerate(ds.test.tolist()):
        for side, truth in ((0, h), (1, t)):
            pool = pools[r * 2 + side]
            rows = np.array([(x, t, r) if side == 0 else (h, x, r) for x in pool.tolist()], np.int32)
            en = eng.score(rows)
            te = eng.score(np.array([(h, t, r)], np.int32))[0]
            takes = pool != truth
            free = np.array([tuple(row) not in known for row in rows.tolist()], bool)
            want[i, side * 2] = 1 + (takes & (en < te)).sum()
            want[i, side * 2 + 1] = 1 + (takes & free & (en < te)).sum()
            total[0] += int(takes.sum())
            total[1] += int((takes & free).sum())
    assert np.array_equal(con["ranks"], want)
    assert con["counted"] == {"raw": total[0], "filtered": total[1]}
    assert con["raw"] == linkpred.candidate_metrics(want[:, [0, 2]])
    assert con["filtered"] == linkpred.candidate_metrics(want[:, [1, 3]])


# ------------------------------------------------------------------ 8. CLI

def test_candidates_cli_matches_engine(tmp_path):
    name = "transe_l1_bern"
    f = MANIFEST["runs"][name]["flags"]
    ds = tiny()
    d = os.path.join(GOLDEN, name)
    exe = tmp_path / "candidatesTransE"
    exe.symlink_to(os.path.join(ROOT, "bin", "kb2e"))
    base = [str(exe), "--datadir", os.path.join(GOLDEN, "tiny"), "--outdir", d, "--size", str(f["size"]), "--method",
            str(f["method"]), "--distance", str(f["distance"])]
    eng = Engine("E", f["size"], ds.num_entities, ds.num_relations, distance=f["distance"])
    eng.upload_params(data.read_table(os.path.join(d, "entity2vec.bern"), ds.num_entities, f["size"]),
                      data.read_table(os.path.join(d, "relation2vec.bern"), ds.num_relations, f["size"]))
    names = {v: k for k, v in data._load_ids(os.path.join(GOLDEN, "tiny", "entity2id.txt")).items()}
    rnames = {v: k for k, v in data._load_ids(os.path.join(GOLDEN, "tiny", "relation2id.txt")).items()}
    filt = np.concatenate([ds.train, ds.valid, ds.test]).astype(np.int32)
    rng = np.random.default_rng(6)
    h, t, r = (int(v) for v in ds.test[0])
    queries = [(1, h, r, rng.integers(0, ds.num_entities, 70).tolist(), t),      # (h, ?, r) with its truth
               (0, t, r, rng.integers(0, ds.num_entities, 5).tolist(), None),    # (?, t, r)
               (1, 7, 3, [], None),                                              # an empty list
               (0, 9, 2, [4, 4, 11], 4)]
    text = []
    for side, e, rel, cand, truth in queries:
        cols = [names[e], "?", rnames[rel]] if side == 1 else ["?", names[e], rnames[rel]]
        cols.append(",".join(names[x] for x in cand))
        if truth is not None:
            cols.append(names[truth])
        text.append("\t".join(cols))
    text.insert(2, "\t".join([names[1], "?", rnames[0], names[2] + ",/m/nothing," + names[3]]))  # an unknown listing
    text.insert(3, "\t".join(["/m/nothing", "?", rnames[0], names[2]]))                           # a dropped line
    queries.insert(2, (1, 1, 0, [2, 3], None))
    lines_of = [0, 1, 2, 4, 5]
    qfile = tmp_path / "c.txt"
    qfile.write_text("\n".join(text) + "\n")
    res = subprocess.run(base + ["--queries", str(qfile)], capture_output=True, text=True, timeout=300, check=True)
    assert res.stdout.count("not found in the identity file: /m/nothing") == 2
    got = [l for l in res.stdout.splitlines() if l.count("\t") in (3, 5)]
    want = []
    for line, (side, e, rel, cand, truth) in zip(lines_of, queries):
        (ids, en, _), = eng.rerank([e], [rel], [side], [cand], len(cand))
        want += ["%d\t%d\t%s\t%.6f" % (line, j + 1, names[int(x)], v) for j, (x, v) in enumerate(zip(ids, en))]
        if truth is not None:
            rk, cn = eng.rank_candidates([e], [rel], [side], [truth], [cand], filt)
            want.append("%d\trank\t%d\t%d\t%d\t%d" % (line, rk[0, 0], rk[0, 1], cn[0, 0], cn[0, 1]))
    assert got == want and sum("\trank\t" in l for l in got) == 2
    # --typed: the driver's numbers
    out = subprocess.run(base + ["--typed"], capture_output=True, text=True, timeout=300, check=True).stdout
    rep = linkpred.type_constrained_evaluation(eng, ds)
    fmt = "%s -- Rank: %f, MRR: %f, Hits@1: %f, Hits@3: %f, Hits@10: %f"
    row = lambda label, m: fmt % (label, m["mean_rank"], m["mrr"], m["hits@1"], m["hits@3"], m["hits@10"])  # noqa: E731
    con, unc = rep["constrained"], rep["unconstrained"]
    for line in (row("Typed raw     ", con["raw"]), row("Typed filtered", con["filtered"]),
                 "Typed counted  -- raw: %d, filtered: %d" % (con["counted"]["raw"], con["counted"]["filtered"]),
                 row("Full raw      ", unc["raw"]), row("Full filtered ", unc["filtered"])):
        assert line in out.splitlines(), line
    # neither --queries nor --typed
    assert subprocess.run(base, capture_output=True, text=True, timeout=300).returncode == 1
