"""The host half of entity neighbours (kb2e_amd/csrc/neighbors_host.hpp): the
plan that cuts the candidates into slices and the queries into chunks whose
partial records fit the cap, and the mutual pairs of a kNN graph.  A stand-alone
program checks them against brute force, built with ASan + UBSan and run
directly.  Also linkpred.mutual_pairs, duplicate_split and
duplicate_detection's arithmetic on a stub engine."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from kb2e_amd import data, linkpred


def test_slice_plan_and_mutual_pairs_match_brute_force(tmp_path):
    exe = tmp_path / "neighbors_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "kb2e_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "neighbors_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip() == "ok"


def _brute_pairs(ents, ids, dist, found):
    row = {}
    for q, e in enumerate(ents):
        row.setdefault(int(e), q)
    lists = {e: {int(ids[q, j]): dist[q, j] for j in range(found[q])} for e, q in row.items()}
    out = []
    for a in lists:
        for b in lists:
            if a < b and b in lists[a] and a in lists[b]:
                out.append((lists[a][b], a, b))
    return sorted(out)


def test_mutual_pairs_against_an_n_squared_loop():
    rng = np.random.default_rng(4)
    for graph in (True, False):
        for _ in range(30):
            ne, k = int(rng.integers(1, 30)), int(rng.integers(1, 7))
            nq = ne if graph else int(rng.integers(1, 50))
            ents = np.arange(ne) if graph else rng.integers(0, ne, nq)
            found = rng.integers(0, min(k, ne) + 1, nq)
            ids = np.full((nq, k), -1, np.int32)
            dist = np.full((nq, k), np.inf)
            for q in range(nq):
                ids[q, :found[q]] = rng.permutation(ne)[:found[q]]
                dist[q, :found[q]] = rng.integers(0, 4, found[q]) * 0.25
            pairs, d = linkpred.mutual_pairs(ids, dist, found, None if graph else ents)
            want = _brute_pairs(ents, ids, dist, found)
            assert pairs.dtype == np.int32 and pairs.shape == (len(want), 2) and d.dtype == np.float64
            assert [(x, a, b) for (a, b), x in zip(pairs.tolist(), d.tolist())] == want
    # nothing found anywhere
    pairs, d = linkpred.mutual_pairs(np.full((3, 2), -1), np.full((3, 2), np.inf), np.zeros(3, int))
    assert pairs.shape == (0, 2) and len(d) == 0
    with pytest.raises(ValueError):
        linkpred.mutual_pairs(np.zeros((3, 2), int), np.zeros((3, 2)), np.zeros(3, int), [0, 1])


def _mentions(train, e):
    return int(((train[:, 0] == e) | (train[:, 1] == e)).sum())


def test_duplicate_split_is_seeded_and_loses_nothing():
    ds = data.synthetic("tiny", seed=3)
    a, pa = linkpred.duplicate_split(ds, 25, seed=9)
    b, pb = linkpred.duplicate_split(ds, 25, seed=9)
    c, pc = linkpred.duplicate_split(ds, 25, seed=10)
    assert np.array_equal(a.train, b.train) and np.array_equal(pa, pb)
    assert not (np.array_equal(a.train, c.train) and np.array_equal(pa, pc))
    assert a.num_entities == ds.num_entities + 25 and a.num_relations == ds.num_relations
    assert np.array_equal(a.valid, ds.valid) and np.array_equal(a.test, ds.test)
    assert pa.dtype == np.int32 and pa.shape == (25, 2)
    assert pa[:, 1].tolist() == list(range(ds.num_entities, ds.num_entities + 25))
    assert len(set(pa[:, 0].tolist())) == 25 and (np.diff(pa[:, 0]) > 0).all()
    for orig, twin in pa.tolist():
        assert _mentions(ds.train, orig) >= 4
        assert _mentions(a.train, orig) >= 2 and _mentions(a.train, twin) >= 2
    # no triple lost or duplicated: folding every twin back onto its original gives the training set, row by row
    back = a.train.copy()
    for orig, twin in pa.tolist():
        back[back == twin] = orig  # (entity columns only: twins are above every relation id too)
    assert a.train.shape == ds.train.shape and np.array_equal(back[:, :2], ds.train[:, :2])
    assert np.array_equal(a.train[:, 2], ds.train[:, 2])
    assert ds.train.max() < ds.num_entities  # the caller's set is untouched
    # the coin really moves triples and really keeps some
    moved = (a.train[:, :2] != ds.train[:, :2]).any(axis=1).sum()
    assert 25 <= moved < sum(_mentions(ds.train, o) for o in pa[:, 0].tolist())
    # too many twins
    with pytest.raises(ValueError):
        linkpred.duplicate_split(ds, ds.num_entities + 1)
    # an entity with exactly four triples: two and two, whatever the coins say
    small = data.Dataset(6, 1, np.array([(0, 1, 0), (0, 2, 0), (3, 0, 0), (0, 0, 0), (4, 5, 0)], np.int32),
                         np.zeros((0, 3), np.int32), np.zeros((0, 3), np.int32))
    for seed in range(8):
        s, p = linkpred.duplicate_split(small, 1, seed=seed)
        assert p.tolist() == [[0, 6]] and _mentions(s.train, 0) == 2 and _mentions(s.train, 6) == 2
        assert all(set(row[:2]) != {0, 6} for row in s.train.tolist())  # the loop (0, 0) moves as a whole


class _Graph:
    """Stands in for an Engine: trains nothing and returns a hand-made graph."""
    made = []

    def __init__(self, model, dim, ne, nr, **kw):
        self.ne, self.kw, self.calls = ne, kw, []
        _Graph.made.append(self)

    def upload_triples(self, t):
        self.calls.append(("triples", len(t)))

    def init_params(self):
        return None, None, None

    def train_epoch(self):
        self.calls.append("epoch")

    def synchronize(self):
        pass

    def close(self):
        self.calls.append("close")

    def knn_graph(self, k, relation=-1):
        self.calls.append(("graph", k, relation))
        ids = np.full((self.ne, k), -1, np.int32)
        dist = np.full((self.ne, k), np.inf)
        found = np.zeros(self.ne, np.int32)
        for a, row in self.lists.items():
            found[a] = len(row)
            ids[a, :len(row)] = row
            dist[a, :len(row)] = np.arange(len(row)) + a * 0.001
        return ids, dist, found


def test_duplicate_detection_on_a_hand_made_graph():
    ds = data.synthetic("tiny", seed=3)
    _, pairs = linkpred.duplicate_split(ds, 4, seed=1)
    (o0, t0), (o1, t1), (o2, t2), (o3, t3) = pairs.tolist()
    other = [e for e in range(ds.num_entities) if e not in pairs[:, 0].tolist()][:3]
    # twin 0: original first and mutual; twin 1: original third, not mutual; twin 2: missed;
    # twin 3: original second and mutual; one mutual pair that is not planted
    _Graph.lists = {t0: [o0, other[0]], o0: [other[1], t0], t1: [other[0], other[1], o1], o1: [other[2]],
                    t2: [other[0]], t3: [other[2], o3], o3: [t3], other[0]: [other[1]], other[1]: [other[0]]}
    _Graph.made.clear()
    res = linkpred.duplicate_detection(ds, "E", 8, 4, epochs=3, k=3, seed=1, relation=2, make_engine=_Graph)
    eng = _Graph.made[0]
    assert eng.ne == ds.num_entities + 4 and eng.kw["transr_compat"] is False
    assert eng.calls == [("triples", len(ds.train)), "epoch", "epoch", "epoch", ("graph", 3, 2), "close"]
    assert np.array_equal(res["pairs"], pairs)
    assert (res["k"], res["entities"], res["planted"]) == (3, ds.num_entities + 4, 4)
    assert res["recall@1"] == 1 / 4 and res["recall@k"] == 3 / 4
    assert res["mutual"] == 3 and sorted(res["mutual_planted"]) == sorted([(o0, t0), (o3, t3)])
    assert res["mutual_share"] == 2 / 3
    assert res["baseline"] == 3 / (ds.num_entities + 3)
