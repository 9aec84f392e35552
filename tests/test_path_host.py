"""The host half of the path queries (kb2e_amd/csrc/path_host.hpp): the check of
the offsets, the chunk plan, the chunk order and the level plan, the walk of the
filter triples along a path and the back-tracking of a winning path.  A
stand-alone program checks them against brute force, built with ASan + UBSan and
run directly.  Also linkpred.path_query_set on a hand-made graph and
linkpred.path_evaluation's arithmetic on a stand-in engine that returns
hand-made ranks."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from kb2e_amd import linkpred


def test_offsets_plans_known_answers_and_backtracking_match_brute_force(tmp_path):
    exe = tmp_path / "path_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "kb2e_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "path_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip() == "ok"


class _Dataset:
    num_entities, num_relations = 7, 3
    # mentions -- 0: [0]; 1: [0]; 2: [1, 2]; 3: [1]; 4: [2]; 5 and 6: none
    train = np.array([(0, 1, 0), (2, 3, 1), (4, 2, 0)], np.int32)
    valid = np.array([(6, 5, 2)], np.int32)
    test = np.array([(1, 5, 2), (3, 6, 1), (5, 0, 0), (2, 0, 1)], np.int32)


def test_path_query_set_on_a_hand_made_graph():
    ds = _Dataset()
    anchors, paths, truth = linkpred.path_query_set(ds, 1, seed=3)
    assert anchors.dtype == np.int32 and truth.dtype == np.int32
    assert anchors.tolist() == [1, 3, 5, 2] and truth.tolist() == [5, 6, 0, 0]
    assert [p.tolist() for p in paths] == [[[2, 1]], [[1, 1]], [[0, 1]], [[1, 1]]]

    for seed in range(6):  # both choices at entity 2 come up
        # the draws: one per step taken, none for the dropped triple
        rng = np.random.default_rng(seed)
        assert rng.integers(1) == 0 and rng.integers(1) == 0
        pick = int(rng.integers(2))
        anchors, paths, truth = linkpred.path_query_set(ds, 2, seed=seed)
        # (1, 5, 2): 1 is the tail of (0, 1, 0) -> forwards from 0; (3, 6, 1): 3 is the tail of (2, 3, 1);
        # (5, 0, 0): no train triple mentions 5; (2, 0, 1): 2 is the head of (2, 3, 1) -> backwards from 3,
        # or the tail of (4, 2, 0) -> forwards from 4
        last = (3, [[1, 0], [1, 1]]) if pick == 0 else (4, [[0, 1], [1, 1]])
        assert anchors.tolist() == [0, 2, last[0]] and truth.tolist() == [5, 6, 0]
        assert [p.tolist() for p in paths] == [[[0, 1], [2, 1]], [[1, 1], [1, 1]], last[1]]
        assert all(p.dtype == np.int32 and p.shape == (2, 2) for p in paths)
    seen = {linkpred.path_query_set(ds, 2, seed=s)[0][2] for s in range(6)}
    assert seen == {3, 4}

    # three hops from (1, 5, 2): 1 <- 0 over (0, 1, 0), then 0 is that triple's head: backwards from 1
    anchors, paths, truth = linkpred.path_query_set(ds, 3, seed=0)
    assert anchors[0] == 1 and paths[0].tolist() == [[0, 0], [0, 1], [2, 1]] and truth[0] == 5
    assert len(anchors) == 3
    with pytest.raises(ValueError):
        linkpred.path_query_set(ds, 0)


class _Ranked:
    """Stands in for an Engine: rank_path() records its arguments and returns the ranks it was given."""

    def __init__(self, ranks):
        self.ranks, self.calls = ranks, []

    def rank_path(self, anchors, paths, truth, filt=None, *, beam=0, no_loops=False):
        m = len(paths[0])
        self.calls.append((np.asarray(anchors).tolist(), [np.asarray(p).tolist() for p in paths],
                           np.asarray(truth).tolist(), np.asarray(filt).tolist(), beam, no_loops))
        return np.array(self.ranks[m], np.int64)


def test_path_evaluation_on_hand_made_ranks():
    ds = _Dataset()
    ranks = {1: [[5, 4], [1, 1], [20, 10], [2, 1]], 2: [[2, 2], [1, 1], [11, 3]], 3: [[1, 1], [12, 12], [4, 2]]}
    eng = _Ranked(ranks)
    res = linkpred.path_evaluation(eng, ds, beam=7, seed=2)
    filt = np.concatenate([ds.train, ds.valid, ds.test]).tolist()
    assert len(eng.calls) == 3 and sorted(res) == [1, 2, 3]
    for m, (anchors, paths, truth, passed, beam, no_loops) in zip((1, 2, 3), eng.calls):
        xa, xp, xt = linkpred.path_query_set(ds, m, seed=2)
        assert anchors == xa.tolist() and paths == [p.tolist() for p in xp] and truth == xt.tolist()
        assert passed == filt and beam == 7 and no_loops is False
        r = np.array(ranks[m], float)
        assert res[m]["count"] == len(r)
        for col, name in enumerate(("raw", "filtered")):
            got = res[m][name]
            assert got["mean_rank"] == r[:, col].mean()
            assert got["mrr"] == (1.0 / r[:, col]).mean()
            assert got["hits@1"] == (r[:, col] <= 1).mean()
            assert got["hits@10"] == (r[:, col] <= 10).mean()
    assert res[1]["filtered"] == {"mean_rank": 4.0, "mrr": (1 / 4 + 1 + 1 / 10 + 1) / 4, "hits@1": 0.5, "hits@10": 1.0}
    assert res[3]["raw"]["hits@10"] == 2 / 3
    eng = _Ranked({2: [[1, 1]] * 3})
    res = linkpred.path_evaluation(eng, ds, hops=(2,), beam=0)
    assert eng.calls[0][4] == 0 and res[2]["count"] == 3
    with pytest.raises(ValueError):
        linkpred.path_evaluation(eng, ds, hops=())
    with pytest.raises(ValueError):
        linkpred.path_evaluation(eng, ds, hops=(0, 1))
