"""Path queries (kb2e_predict_path, kb2e_rank_path) against the oracle.

The oracle is a numpy dynamic program over orc.Model(..., transr_compat=False)
.energy: c_1 is the anchor's one-sided energy row, c_i = min over the frontier p
(ascending id, first minimum: the smallest predecessor id among equal sums) of
c_{i-1}[p] + E_i[p, :], the frontier np.lexsort((ids, c))[:beam], the answers
np.lexsort((ids, c)) after the ends of the filter's own paths are dropped.  All
device arithmetic is FP64 in the reference's order and one rounding per
addition, so ids, energies, found counts, predecessors and ranks must be EQUAL
(no tolerance anywhere in this file; the CLI's printed %.6lf is compared as
text).  Exact mode (beam = 0) is used at 70 entities only, and at 2,085 entities
beams of at most 33, so that the oracle scores at most 33 x 2,085 triples a hop.
"""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from gpu_common import MANIFEST, tiny
from kb2e_amd import data, linkpred
from kb2e_amd.engine import PATH_MAX_HOPS, Engine, EngineError, lib
from oracle import orc

pytestmark = pytest.mark.gpu

W = PATH_MAX_HOPS - 1


# ------------------------------------------------------------------ helpers

def _tables(model, ds, n, seed, scale=0.3):
    """tests/test_gpu_joint.py _tables' recipe."""
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


def _p(*hops):
    return np.array(hops, np.int32).reshape(-1, 2)


class Setup:
    """An engine and the oracle on the same tables; oracle rows (the energies of
    one step from one entity to every entity) are memoised and never modified."""

    def __init__(self, model, n, ds, *, distance=0, precision=64, seed=0, tables=None, **kw):
        self.ds, self.ne, self.nr = ds, ds.num_entities, ds.num_relations
        self.tables = _tables(model, ds, n, seed) if tables is None else tables
        self.eng = Engine(model, n, ds.num_entities, ds.num_relations, distance=distance, precision=precision, **kw)
        self.eng.upload_params(*self.tables)
        self.m = orc.Model(model, n, ds.num_entities, ds.num_relations, distance=distance, transr_compat=False)
        self.m.set_tables(*(_f32(self.tables) if precision == 32 else self.tables))
        self.filt = np.concatenate([ds.train, ds.valid, ds.test])
        self.ids = np.arange(self.ne)
        self._rows = {}

    def row(self, p, r, side):
        """Energies of the step from p to every y: the triple (p, y, r) for side 1, (y, p, r) for side 0."""
        key = (int(p), int(r), int(side))
        if key not in self._rows:
            p, r, side = key
            row = np.array([self.m.energy(p, y, r) if side else self.m.energy(y, p, r) for y in range(self.ne)])
            row.setflags(write=False)
            self._rows[key] = row
        return self._rows[key]

    def walk(self, anchor, path, beam=0, no_loops=False):
        """(c float64[ne] with +inf where no path ends, preds: per hop 2..L the
        predecessor of every entity, frontiers: per hop 1..L-1 the frontier in
        (cost, id) order)."""
        hops = np.asarray(path).reshape(-1, 2).tolist()
        c = self.row(anchor, *hops[0]).copy()
        if no_loops:
            c[anchor] = np.inf
        preds, frontiers = [], []
        for r, side in hops[1:]:
            reach = self.ids[np.isfinite(c)]
            front = reach[np.lexsort((reach, c[reach]))]
            if beam:
                front = front[:beam]
            frontiers.append(front)
            fs = np.sort(front)
            if len(fs) == 0:
                c = np.full(self.ne, np.inf)
                preds.append(np.full(self.ne, -1))
                continue
            sums = c[fs, None] + np.stack([self.row(p, r, side) for p in fs])
            if no_loops:
                sums[np.arange(len(fs)), fs] = np.inf
            arg = sums.argmin(axis=0)  # the first minimum: the smallest id
            c = sums[arg, self.ids]
            preds.append(np.where(np.isfinite(c), fs[arg], -1))
        return c, preds, frontiers

    def excluded(self, anchor, path, filt, no_loops=False):
        out = np.zeros(self.ne, bool)
        if filt is None or len(filt) == 0:
            return out
        triples = set(map(tuple, np.asarray(filt).tolist()))
        cur = {int(anchor)}
        for r, side in np.asarray(path).reshape(-1, 2).tolist():
            nxt = set()
            for h, t, fr in triples:
                if fr != r or (no_loops and h == t):
                    continue
                if side and h in cur:
                    nxt.add(t)
                if not side and t in cur:
                    nxt.add(h)
            cur = nxt
        out[list(cur)] = True
        return out

    def expect(self, anchors, paths, k, filt=None, beam=0, no_loops=False):
        nq = len(paths)
        ids = np.full((nq, k), -1, np.int32)
        en = np.full((nq, k), np.inf)
        found = np.zeros(nq, np.int32)
        via = np.full((nq, k, W), -1, np.int32)
        fronts = []
        for q in range(nq):
            c, preds, frontiers = self.walk(anchors[q], paths[q], beam, no_loops)
            fronts.append(frontiers)
            keep = np.isfinite(c) & ~self.excluded(anchors[q], paths[q], filt, no_loops)
            cand = self.ids[keep]
            order = np.lexsort((cand, c[keep]))[:k]
            found[q] = len(order)
            ids[q, :len(order)] = cand[order]
            en[q, :len(order)] = c[keep][order]
            for j, y in enumerate(cand[order].tolist()):
                x = y
                for lev in range(len(preds), 0, -1):  # preds[lev - 1]: the predecessors at hop lev + 1
                    x = int(preds[lev - 1][x])
                    via[q, j, lev - 1] = x
        return ids, en, found, via, fronts

    def expect_ranks(self, anchors, paths, truth, filt, beam=0, no_loops=False):
        ranks = np.zeros((len(paths), 2), np.int64)
        for q in range(len(paths)):
            c, _, _ = self.walk(anchors[q], paths[q], beam, no_loops)
            above = c < c[truth[q]]
            ranks[q, 0] = 1 + above.sum()
            ex = self.excluded(anchors[q], paths[q], filt, no_loops)
            ex[truth[q]] = False
            ranks[q, 1] = 1 + (above & ~ex).sum()
        return ranks

    def check(self, anchors, paths, k, filt=None, beam=0, no_loops=False):
        ids, en, found, via = self.eng.predict_path(anchors, paths, k, filt, beam=beam, no_loops=no_loops, via=True)
        xi, xe, xf, xv, fronts = self.expect(anchors, paths, k, filt, beam, no_loops)
        assert ids.shape == (len(paths), k) and ids.dtype == np.int32 and en.dtype == np.float64
        assert via.shape == (len(paths), k, W) and via.dtype == np.int32
        assert np.array_equal(found, xf)
        assert np.array_equal(ids, xi)
        assert np.array_equal(en, xe)
        assert np.array_equal(via, xv)
        # every via entity belongs to the oracle's frontier of its level
        for q in range(len(paths)):
            for lev, front in enumerate(fronts[q]):
                assert set(via[q, :found[q], lev].tolist()) <= set(front.tolist())
        plain = self.eng.predict_path(anchors, paths, k, filt, beam=beam, no_loops=no_loops)
        for x, y in zip(plain, (ids, en, found)):
            assert np.array_equal(x, y)
        return ids, en, found, via

    def check_ranks(self, anchors, paths, truth, filt, beam=0, no_loops=False):
        ranks = self.eng.rank_path(anchors, paths, truth, filt, beam=beam, no_loops=no_loops)
        assert ranks.shape == (len(paths), 2) and ranks.dtype == np.int64
        assert np.array_equal(ranks, self.expect_ranks(anchors, paths, truth, filt, beam, no_loops))
        return ranks


def _random_paths(rng, ds, lengths):
    anchors = rng.integers(0, ds.num_entities, len(lengths)).astype(np.int32)
    paths = [np.stack([rng.integers(0, ds.num_relations, m), rng.integers(0, 2, m)], axis=1).astype(np.int32)
             for m in lengths]
    return anchors, paths


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
def test_path_models(model, distance, precision):
    """E / H / R at n = 20 on 70 entities: lengths 1, 2 and 3 with mixed sides in
    one call, exact and with a beam of 5, raw and filtered, top-k and ranks."""
    s = Setup(model, 20, _ds70(), distance=distance, precision=precision, seed=5 + distance)
    qs = linkpred.path_query_set(s.ds, 3, seed=1)
    anchors = np.concatenate([qs[0][:4], s.ds.test[:4, 0], [3, 9]]).astype(np.int32)
    paths = qs[1][:4] + [_p((r, 1)) for r in s.ds.test[:4, 2]] + [_p((0, 1), (2, 0)), _p((1, 0), (1, 0))]
    truth = np.concatenate([qs[2][:4], s.ds.test[:4, 1], [5, 6]]).astype(np.int32)
    assert sorted({len(p) for p in paths}) == [1, 2, 3] and {int(x) for p in paths for x in p[:, 1]} == {0, 1}
    for beam in (0, 5):
        s.check(anchors, paths, 10, None, beam)
        _, _, found, _ = s.check(anchors, paths, s.ne, s.filt, beam)
        assert (found[:8] < s.ne).all()  # the test tail is an answer the graph states
        raw = s.check_ranks(anchors, paths, truth, None, beam)
        assert np.array_equal(raw[:, 0], raw[:, 1])
        s.check_ranks(anchors, paths, truth, s.filt, beam)
    s.eng.close()


# ------------------------------------------------------------------ 2. one hop is kb2e_predict

def test_path_single_hop_equals_predict(tiny_e):
    s = tiny_e
    pick = s.ds.test[:30]
    e = np.concatenate([pick[:, 0], pick[:, 1]]).astype(np.int32)
    r = np.concatenate([pick[:, 2], pick[:, 2]]).astype(np.int32)
    side = np.array([1] * 30 + [0] * 30, np.int32)
    paths = [_p((r[i], side[i])) for i in range(60)]
    for filt in (None, s.filt):
        for k, beam in ((1, 0), (10, 7), (300, 0)):
            a = s.eng.predict_path(e, paths, k, filt, beam=beam, via=True)
            b = s.eng.predict(e, r, side, k, filt)
            for x, y in zip(a[:3], b):
                assert x.dtype == y.dtype and np.array_equal(x, y)
            assert (a[3] == -1).all()
    ranks = s.eng.rank_triples(pick, s.filt)  # head raw, head filtered, tail raw, tail filtered
    truth = np.concatenate([pick[:, 1], pick[:, 0]]).astype(np.int32)
    for beam in (0, 3):
        got = s.eng.rank_path(e, paths, truth, s.filt, beam=beam)
        assert np.array_equal(got[:30], ranks[:, 2:4]) and np.array_equal(got[30:], ranks[:, 0:2])
    assert (got[:, 1] < got[:, 0]).any()  # (the filter bites)
    assert s.eng.counter("path_hops") == 0


# ------------------------------------------------------------------ 3. lengths

def test_path_lengths_and_projection_count(e70):
    s = e70
    rng = np.random.default_rng(11)
    anchors, paths = _random_paths(rng, s.ds, [2, 3, 8, 1, 3, 2, 8, 1, 5])
    truth = rng.integers(0, s.ne, len(paths)).astype(np.int32)
    for beam in (0, 5):
        s.check(anchors, paths, 10, s.filt, beam)
        s.check_ranks(anchors, paths, truth, s.filt, beam)
        assert s.eng.counter("path_hops") == sum(len(p) - 1 for p in paths)
        assert s.eng.counter("path_chunks") == 1
    b0 = s.eng.device_bytes()
    nine = _random_paths(rng, s.ds, [9])
    with pytest.raises(EngineError, match="EINVAL"):
        s.eng.predict_path(nine[0], nine[1], 10)
    with pytest.raises(EngineError, match="EINVAL"):
        s.eng.rank_path([0, 1], [paths[0], nine[1][0]], [0, 1], s.filt)
    assert s.eng.device_bytes() == b0
    # level 1: relations {0, 1}; level 2: two queries share relation 2, the other two walk 0 and 1:
    # 2 + 3 projections (no level ends on the relation the next one starts with)
    four = [_p((0, 1), (2, 1)), _p((1, 0), (2, 0)), _p((0, 0), (1, 1)), _p((1, 1), (0, 1))]
    s.check([1, 2, 3, 4], four, 5, None, 4)
    assert s.eng.counter("path_projections") == 5 and s.eng.counter("path_hops") == 4
    same = [_p((1, 1), (2, 1)), _p((1, 0), (2, 0))]
    s.check([1, 2], same, 5, None, 4)
    assert s.eng.counter("path_projections") == 2


# ------------------------------------------------------------------ 4. frontier tiles

@pytest.mark.parametrize("beam", [1, 5, 16, 17, 33, 100, 1024])
def test_path_frontier_tiles_70(e70, beam):
    """70 entities, less than one block of targets: beams around the tile of 16
    frontier rows; a beam above |E| is the exact form."""
    s = e70
    anchors, paths = _random_paths(np.random.default_rng(12), s.ds, [3, 2, 2])
    got = s.check(anchors, paths, 12, s.filt, beam)
    s.check_ranks(anchors, paths, [4, 40, 69], s.filt, beam)
    if beam >= s.ne:
        exact = s.eng.predict_path(anchors, paths, 12, s.filt, beam=0, via=True)
        for x, y in zip(got, exact):
            assert np.array_equal(x, y)


@pytest.mark.parametrize("beam", [1, 5, 16, 17, 33])
def test_path_frontier_tiles_2085(e2085, beam):
    """2,085 entities: eight blocks of targets and a ragged one."""
    s = e2085
    anchors, paths = _random_paths(np.random.default_rng(13), s.ds, [2, 3])
    s.check(anchors, paths, 10, s.filt, beam)
    s.check_ranks(anchors, paths, [2084, 7], s.filt, beam)


# ------------------------------------------------------------------ 5. wide rows

@pytest.mark.parametrize("rows_l2", ["0", "1"])
@pytest.mark.parametrize("model", ["E", "H", "R"])
def test_path_wide_rows(model, rows_l2, monkeypatch):
    """n = 260, and KB2E_EVAL_ROWS_L2=1: the hop kernel reads the frontier's rows
    from the projection table instead of LDS."""
    monkeypatch.setenv("KB2E_EVAL_ROWS_L2", rows_l2)
    s = Setup(model, 260, _ds70(), seed=41)
    anchors, paths = _random_paths(np.random.default_rng(14), s.ds, [2, 3, 1])
    for beam in (0, 17):
        s.check(anchors, paths, 10, s.filt, beam)
        s.check_ranks(anchors, paths, [1, 2, 3], s.filt, beam)
    s.eng.close()


# ------------------------------------------------------------------ 6. ties

def test_path_ties_take_the_smaller_id():
    ds = _ds70()
    ent, rel, _ = _tables("E", ds, 20, 31)
    twins = [9, 4, 33]
    # identical rows: identical energies as candidates and as predecessors; one step of relation 1 from
    # entity 7, so that they are the cheapest first stop of the first query and win many targets
    ent[twins] = ent[7] + rel[1]
    s = Setup("E", 20, ds, tables=(ent, rel, None))
    anchors, paths = [7, 12], [_p((1, 1), (2, 0)), _p((0, 0), (1, 1), (2, 1))]
    for beam in (0, 40, 3):
        ids, en, found, via = s.check(anchors, paths, s.ne, None, beam)
        assert not np.isin(via, [9, 33]).any()  # 4 gives the same sum
        for q in range(2):
            pos = [int(np.nonzero(ids[q] == x)[0][0]) for x in sorted(twins)]
            assert pos == list(range(pos[0], pos[0] + 3)) and len(set(en[q, pos].tolist())) == 1
            s.check(anchors[q:q + 1], paths[q:q + 1], pos[0] + 2, None, beam)  # a k that cuts the group
    _, preds, _ = s.walk(7, paths[0])
    assert (preds[0] == 4).sum() > 10  # (the twins do win)
    ranks = s.check_ranks([7, 7], [paths[0]] * 2, [4, 33], None)
    assert ranks[0, 0] == ranks[1, 0]  # ties are not counted above the truth
    s.eng.close()


# ------------------------------------------------------------------ 7. no_loops

def test_path_no_loops(e70):
    s = e70
    anchors, paths = _random_paths(np.random.default_rng(15), s.ds, [2, 3, 1, 4])
    loops = np.array([(x, x, r) for x in range(0, 70, 3) if x != anchors[2] for r in range(3)], np.int32)
    filt = np.concatenate([s.filt, loops])
    for beam in (0, 6):
        on = s.check(anchors, paths, s.ne, filt, beam, no_loops=True)
        off = s.check(anchors, paths, s.ne, filt, beam, no_loops=False)
        assert not np.array_equal(on[1], off[1])
        assert anchors[2] not in on[0][2] and anchors[2] in off[0][2]  # one hop: the anchor itself is no answer
        for q in range(4):  # no step of a winning path stays on its entity
            for j in range(on[2][q]):
                chain = [int(anchors[q])] + [int(x) for x in on[3][q, j] if x >= 0] + [int(on[0][q, j])]
                assert all(a != b for a, b in zip(chain, chain[1:]))
        s.check_ranks(anchors, paths, [0, 1, 2, 3], filt, beam, no_loops=True)


def test_path_no_loops_two_entities():
    """Two entities, two hops from 0 without loops: 0 -> 1 -> 0 is the only path;
    entity 1 has none (key ~0), so one answer is found."""
    ds = types.SimpleNamespace(num_entities=2, num_relations=1, train=np.array([(0, 1, 0)], np.int32),
                               valid=np.zeros((0, 3), np.int32), test=np.zeros((0, 3), np.int32))
    s = Setup("E", 20, ds, seed=3)
    for beam in (0, 1, 2):
        ids, en, found, via = s.check([0], [_p((0, 1), (0, 1))], 2, None, beam, no_loops=True)
        assert found.tolist() == [1] and ids.tolist() == [[0, -1]] and np.isinf(en[0, 1])
        assert via[0, 0].tolist() == [1] + [-1] * (W - 1) and (via[0, 1] == -1).all()
        assert en[0, 0] == s.m.energy(0, 1, 0) + s.m.energy(1, 0, 0)
        ranks = s.check_ranks([0, 0], [_p((0, 1), (0, 1))] * 2, [0, 1], None, beam, no_loops=True)
        assert ranks[:, 0].tolist() == [1, 2]
        _, _, found, _ = s.check([0], [_p((0, 1), (0, 1))], 2, None, beam, no_loops=False)
        assert found.tolist() == [2]
    # three hops: 0 -> 1 -> 0 -> 1 only
    ids, _, found, via = s.check([0], [_p((0, 1), (0, 0), (0, 1))], 2, None, 0, no_loops=True)
    assert found.tolist() == [1] and ids[0, 0] == 1 and via[0, 0, :2].tolist() == [1, 0]
    s.eng.close()


# ------------------------------------------------------------------ 8. exclusion

def test_path_exclusion_follows_the_filter_along_the_path(e70):
    s = e70
    ne = s.ne
    path = _p((1, 1), (2, 0))  # 3 --r1--> x, then r2 backwards: (y, x, r2)
    # 20: known along the whole path (3 -> 40 -> 20); 21: the last hop only (41 is not known from 3);
    # 22: along the whole path, over two intermediates; 23: the first hop's triple points the wrong way
    filt = np.array([(3, 40, 1), (20, 40, 2), (21, 41, 2), (3, 42, 1), (3, 43, 1), (22, 42, 2), (22, 43, 2),
                     (44, 3, 1), (23, 44, 2)], np.int32)
    for beam in (0, 9):
        ids, _, found, _ = s.check([3], [path], ne, filt, beam)
        assert found[0] == ne - 2
        kept = set(ids[0, :found[0]].tolist())
        assert 20 not in kept and 22 not in kept and {21, 23, 40, 42} <= kept
        # a filter triple listed twice changes nothing
        twice = np.concatenate([filt, filt[:3], filt[5:6]])
        for x, y in zip(s.eng.predict_path([3], [path], ne, twice, beam=beam), s.expect([3], [path], ne, filt, beam)):
            assert np.array_equal(x, y)
        # one hop: kb2e_predict's rule
        ids1, _, found1, _ = s.check([3], [path[:1]], ne, filt, beam)
        assert found1[0] == ne - 3 and not {40, 42, 43} & set(ids1[0, :found1[0]].tolist())
        # everything known: nothing is found
        full = np.array([(3, 40, 1)] + [(y, 40, 2) for y in range(ne)], np.int32)
        ids, en, found, via = s.check([3, 5], [path, _p((0, 1))], 7, full, beam)
        assert found.tolist() == [0, 7] and (ids[0] == -1).all() and np.isinf(en[0]).all() and (via[0] == -1).all()
        # the truth is never excluded, the other excluded candidates are
        ranks = s.check_ranks([3, 3, 3], [path] * 3, [22, 21, 60], filt, beam)
        c, _, _ = s.walk(3, path, beam)
        for i, tr in enumerate((22, 21, 60)):
            assert ranks[i, 0] - ranks[i, 1] == sum(c[x] < c[tr] for x in (20, 22) if x != tr)
        assert s.check_ranks([3], [path], [20], full, beam)[0, 1] == 1


# ------------------------------------------------------------------ 9. witnesses

@pytest.mark.parametrize("model,n,distance", [("E", 50, 1), ("H", 32, 0), ("R", 20, 0)])
def test_path_energies_are_sums_of_score_triples_bits(model, n, distance):
    s = Setup(model, n, _ds70(), distance=distance, seed=61)
    anchors, paths = _random_paths(np.random.default_rng(16), s.ds, [1, 2, 3, 5, 8])
    for beam in (0, 9):
        ids, en, found, via = s.eng.predict_path(anchors, paths, 8, beam=beam, via=True)
        assert (found == 8).all()
        for q, path in enumerate(paths):
            assert (via[q, :, len(path) - 1:] == -1).all() and (via[q, :, :len(path) - 1] >= 0).all()
            for j in range(8):
                chain = [int(anchors[q])] + via[q, j, :len(path) - 1].tolist() + [int(ids[q, j])]
                trip = np.array([(a, b, r) if side else (b, a, r)
                                 for (a, b), (r, side) in zip(zip(chain, chain[1:]), path.tolist())], np.int32)
                total = None
                for e in s.eng.score(trip).tolist():  # left to right
                    total = e if total is None else total + e
                assert total == en[q, j]
    s.eng.close()


# ------------------------------------------------------------------ 10. chunking

def test_path_chunked_rows(e70, monkeypatch):
    """KB2E_PATH_CHUNK_ROWS=7 with lengths [1, 2, 3, 1, 1, 4, 2]: under beam search
    the queries hold 2 3 3 2 2 3 3 rows of |E| words -> [1,2] [3,1,1] [4,2]; exactly
    2 5 6 2 2 7 5 -> [1,2] [3] [1,1] [4] [2].  The answers do not change."""
    s = e70
    rng = np.random.default_rng(21)
    anchors, paths = _random_paths(rng, s.ds, [1, 2, 3, 1, 1, 4, 2])
    truth = rng.integers(0, s.ne, len(paths)).astype(np.int32)
    whole = {b: (s.eng.predict_path(anchors, paths, 10, s.filt, beam=b, via=True),
                 s.eng.rank_path(anchors, paths, truth, s.filt, beam=b)) for b in (0, 6)}
    assert s.eng.counter("path_chunks") == 1
    monkeypatch.setenv("KB2E_PATH_CHUNK_ROWS", "7")
    for beam, chunks in ((6, 3), (0, 5)):
        got = s.eng.predict_path(anchors, paths, 10, s.filt, beam=beam, via=True)
        assert s.eng.counter("path_chunks") == chunks and s.eng.counter("path_hops") == 7
        for x, y in zip(got, whole[beam][0]):
            assert np.array_equal(x, y)
        assert np.array_equal(s.eng.rank_path(anchors, paths, truth, s.filt, beam=beam), whole[beam][1])
        assert s.eng.counter("path_chunks") == chunks
        s.check(anchors, paths, 10, s.filt, beam)
    # the budget rises to the largest query: 7 exactly (the same plan), 3 under beam search (one query a chunk)
    monkeypatch.setenv("KB2E_PATH_CHUNK_ROWS", "1")
    s.check(anchors, paths, 10, s.filt, 0)
    assert s.eng.counter("path_chunks") == 5
    s.check(anchors, paths, 10, s.filt, 6)
    assert s.eng.counter("path_chunks") == 7


# ------------------------------------------------------------------ 11. contract

def _raw_predict_path(eng, anchors, offsets, hops, k, beam=0, no_loops=0):
    anchors = np.ascontiguousarray(anchors, dtype=np.int32)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    hops = np.ascontiguousarray(hops, dtype=np.int32).reshape(-1, 2)
    cols = [np.ascontiguousarray(hops[:, c]) for c in range(2)]
    nq = len(offsets) - 1
    ids = np.zeros((nq, max(k, 1)), np.int32)
    en = np.zeros((nq, max(k, 1)))
    found = np.zeros(nq, np.int32)
    i32p = C.POINTER(C.c_int32)
    return lib().kb2e_predict_path(eng.h, anchors.ctypes.data_as(i32p), offsets.ctypes.data_as(C.POINTER(C.c_int64)),
                                   *[c.ctypes.data_as(i32p) for c in cols], nq, k, beam, no_loops, None, None, None, 0,
                                   ids.ctypes.data_as(i32p), en.ctypes.data_as(C.POINTER(C.c_double)),
                                   found.ctypes.data_as(i32p), None)


def test_path_bad_arguments_are_refused(tiny_e):
    s = tiny_e
    eng, ne, nr = s.eng, s.ne, s.nr
    b0 = eng.device_bytes()
    good = _p((1, 1), (2, 0))
    hops = np.concatenate([good, good])
    EINVAL = 1
    assert _raw_predict_path(eng, [3, 4], [0, 2, 4], hops, 5) == 0
    for offsets in ([1, 2, 4], [0, 2, 2], [0, 0, 4], [0, 3, 2], [-1, 2, 4]):
        assert _raw_predict_path(eng, [3, 4], offsets, hops, 5) == EINVAL, offsets
        assert eng.device_bytes() == b0
    assert _raw_predict_path(eng, [3], [0, 9], np.tile(good[:1], (9, 1)), 5) == EINVAL
    assert _raw_predict_path(eng, [3], [0, 8], np.tile(good[:1], (8, 1)), 5, 4) == 0
    for beam, no_loops in ((-1, 0), (1025, 0), (0, 2), (0, -1)):
        assert _raw_predict_path(eng, [3, 4], [0, 2, 4], hops, 5, beam, no_loops) == EINVAL
        assert eng.device_bytes() == b0
    assert _raw_predict_path(eng, [3, 4], [0, 2, 4], hops, 5, 1024, 1) == 0
    bad_filters = [np.array([t], np.int32) for t in ((0, ne, 0), (-1, 1, 0), (0, 1, nr), (0, 1, -1))]
    empty = np.zeros((0, 2), np.int32)
    for anchors, paths, k, filt in (([3], [good], 0, None), ([3], [good], 1025, None), ([3], [good], -1, None),
                                    ([3], [empty], 5, None), ([3, 4], [good, empty], 5, None), ([], [], 5, None),
                                    ([3], [_p((1, 2))], 5, None), ([3], [_p((1, -1))], 5, None),
                                    ([3, 4], [good, _p((1, 1), (1, 2))], 5, None),
                                    ([ne], [good], 5, None), ([-1], [good], 5, None), ([3], [_p((nr, 1))], 5, None),
                                    ([3], [_p((1, 1), (-1, 0))], 5, None), ([3, ne], [good, good], 5, None),
                                    *[([3], [good], 5, f) for f in bad_filters]):
        with pytest.raises(EngineError, match="EINVAL"):
            eng.predict_path(anchors, paths, k, filt, beam=4)
        assert eng.device_bytes() == b0
    for anchors, paths, truth, filt in (([3], [good], [ne], None), ([3], [good], [-1], None),
                                        ([3, 4], [good, good], [0, ne], s.filt), ([3], [_p((1, 2))], [0], None),
                                        ([ne], [good], [0], None), ([3], [empty], [0], None), ([], [], [], None),
                                        *[([3], [good], [0], f) for f in bad_filters]):
        with pytest.raises(EngineError, match="EINVAL"):
            eng.rank_path(anchors, paths, truth, filt)
        assert eng.device_bytes() == b0
    s.check([3], [good], 5, s.filt, 4)  # still usable
    fresh = Engine("E", 20, ne, nr)
    with pytest.raises(EngineError, match="ESTATE"):
        fresh.predict_path([3], [good], 5)
    with pytest.raises(EngineError, match="ESTATE"):
        fresh.rank_path([3], [good], [0])
    fresh.close()


@pytest.mark.parametrize("model", ["E", "H", "R"])
def test_path_calls_leave_the_context_unchanged(model):
    """Tables, the glibc stream, the TransR work vectors and device_bytes() are the
    same after the calls, refused ones included; the five profile families report."""
    ds = tiny()
    n = 20
    tables = _tables(model, ds, n, 51)
    anchors, paths, truth = linkpred.path_query_set(ds, 3, seed=2)
    anchors, paths, truth = anchors[:12], paths[:12], truth[:12]
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
            for beam in (0, 8):
                eng.predict_path(anchors, paths, 10, filt, beam=beam, via=True)
                assert eng.device_bytes() == b0
                eng.predict_path(anchors, paths, 10, beam=beam, no_loops=True)
                assert eng.device_bytes() == b0
                eng.rank_path(anchors, paths, truth, filt, beam=beam)
                assert eng.device_bytes() == b0
            for refused in (lambda: eng.predict_path(anchors, paths, 0), lambda: eng.predict_path([3], [_p((1, 2))], 5),
                            lambda: eng.rank_path(anchors[:1], paths[:1], [ds.num_entities], filt)):
                with pytest.raises(EngineError):
                    refused()
                assert eng.device_bytes() == b0
            for fam in ("path_score", "path_hop", "path_select", "path_mask", "path_rank"):
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


# ------------------------------------------------------------------ 12. evaluation driver

def test_path_evaluation_matches_oracle_ranks(e70):
    s = e70
    res = linkpred.path_evaluation(s.eng, s.ds, hops=(1, 2), beam=9, seed=4)
    for m in (1, 2):
        anchors, paths, truth = linkpred.path_query_set(s.ds, m, seed=4)
        assert res[m]["count"] == len(anchors) > 0
        exp = s.expect_ranks(anchors, paths, truth, s.filt, 9)
        assert res[m]["raw"]["mean_rank"] == exp[:, 0].mean() and res[m]["filtered"]["mean_rank"] == exp[:, 1].mean()
        assert res[m]["filtered"]["mrr"] == (1.0 / exp[:, 1]).mean()
        assert res[m]["filtered"]["hits@10"] == (exp[:, 1] <= 10).mean()


# ------------------------------------------------------------------ 13. CLI

def test_path_cli_matches_engine(tmp_path):
    name = "transe_l1_bern"
    f = MANIFEST["runs"][name]["flags"]
    ds = tiny()
    d = os.path.join(GOLDEN, name)
    qfile = tmp_path / "paths.txt"
    # line 2 holds an unknown entity, line 4 an unknown relation, line 6 nine hops: dropped
    qfile.write_text("/m/e25\t/r/r4\t^/r/r1\n/m/nobody\t/r/r0\n/m/e105\t^/r/r0\n/m/e3\t/r/r0\t/r/nothing\n"
                     "/m/e9\t/r/r3\t/r/r2\t^/r/r4\n/m/e1" + "\t/r/r1" * 9 + "\n/m/e30\t/r/r2\t/r/r2\n")
    lines = [1, 3, 5, 7]
    anchors = [25, 105, 9, 30]
    paths = [_p((4, 1), (1, 0)), _p((0, 0)), _p((3, 1), (2, 1), (4, 0)), _p((2, 1), (2, 1))]
    exe = tmp_path / "pathTransE"
    exe.symlink_to(os.path.join(ROOT, "bin", "kb2e"))
    base = [str(exe), "--datadir", os.path.join(GOLDEN, "tiny"), "--outdir", d, "--size", str(f["size"]), "--method",
            str(f["method"]), "--distance", str(f["distance"]), "--queries", str(qfile)]
    eng = Engine("E", f["size"], ds.num_entities, ds.num_relations, distance=f["distance"])
    eng.upload_params(data.read_table(os.path.join(d, "entity2vec.bern"), ds.num_entities, f["size"]),
                      data.read_table(os.path.join(d, "relation2vec.bern"), ds.num_relations, f["size"]))
    names = {v: k for k, v in data._load_ids(os.path.join(GOLDEN, "tiny", "entity2id.txt")).items()}
    assert names[25] == "/m/e25"
    filt = np.concatenate([ds.test, ds.train, ds.valid])
    for extra, k, fl, beam, nl in (([], 10, filt, 64, False),
                                   (["--topk", "3", "--filtered", "0", "--beam", "0", "--noloops"], 3, None, 0, True),
                                   (["--topk", "4", "--beam", "5"], 4, filt, 5, False)):
        res = subprocess.run(base + extra, capture_output=True, text=True, timeout=300, check=True)
        assert "Head entity found in triple file that was not found in the identity file: /m/nobody" in res.stdout
        assert "Relation found in triple file that was not found in the identity file: /r/nothing" in res.stdout
        assert "Query needs 1 to 8 relations: /m/e1" in res.stdout
        rows = [l.split("\t") for l in res.stdout.splitlines() if l.count("\t") == 4]
        ids, en, found, via = eng.predict_path(anchors, paths, k, fl, beam=beam, no_loops=nl, via=True)
        assert (found == k).all()
        expect = [[str(lines[q]), str(j + 1), names[int(ids[q, j])], "%.6f" % en[q, j],
                   ",".join(names[int(x)] for x in via[q, j] if x >= 0)]
                  for q in range(len(paths)) for j in range(found[q])]
        assert rows == expect
    eng.close()
