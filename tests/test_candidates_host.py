"""The host half of the candidate-list calls (kb2e_amd/csrc/candidates_host.hpp):
the planner that cuts the lists into wave-sized work items and the queries into
chunks, and the argument checks.  A stand-alone program checks them against
brute force on random ragged lists, built with ASan + UBSan and run directly.
Also the arithmetic of linkpred's drivers (side_queries, candidate_metrics,
sampled_evaluation, slot_pools, type_constrained_evaluation) on a stub engine
with hand-made ranks."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from kb2e_amd import data, linkpred


def test_planner_matches_brute_force(tmp_path):
    exe = tmp_path / "candidates_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "kb2e_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "candidates_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip() == "ok"


def test_side_queries_interleave_head_and_tail():
    test = np.array([(3, 5, 1), (7, 2, 0)], np.int32)
    ent, rel, side, truth = linkpred.side_queries(test)
    assert ent.tolist() == [5, 3, 2, 7] and truth.tolist() == [3, 5, 7, 2]
    assert rel.tolist() == [1, 1, 0, 0] and side.tolist() == [0, 1, 0, 1]
    assert all(a.dtype == np.int32 for a in (ent, rel, side, truth))


def test_candidate_metrics_from_hand_made_ranks():
    m = linkpred.candidate_metrics([1, 2, 3, 4, 10, 11, 100, 1])
    assert m["mean_rank"] == (1 + 2 + 3 + 4 + 10 + 11 + 100 + 1) / 8
    assert m["mrr"] == pytest.approx((1 + 1 / 2 + 1 / 3 + 1 / 4 + 1 / 10 + 1 / 11 + 1 / 100 + 1) / 8, rel=1e-15)
    assert m["hits@1"] == 2 / 8 and m["hits@3"] == 4 / 8 and m["hits@10"] == 6 / 8


class _Stub:
    """Stands in for an Engine: records the calls and returns hand-made ranks."""

    def __init__(self, ne, ranks, counted, full=None):
        self.ne, self.ranks, self.counted, self.full, self.calls = ne, ranks, counted, full, []

    def rank_candidates(self, ent, rel, side, truth, candidates, filt=None, lists=None):
        self.calls.append(dict(ent=np.array(ent), rel=np.array(rel), side=np.array(side), truth=np.array(truth),
                               candidates=[np.array(c) for c in candidates], filt=filt,
                               lists=None if lists is None else np.array(lists)))
        return np.array(self.ranks, np.int64), np.array(self.counted, np.int64)

    def rank_triples(self, test, filt):
        self.calls.append(("rank_triples", np.array(test), np.array(filt)))
        return np.array(self.full, np.int64)


def test_sampled_evaluation_arithmetic_and_draws():
    test = np.array([(0, 1, 0), (2, 3, 1)], np.int32)
    filt = np.array([(0, 1, 0)], np.int32)
    ranks = [(1, 1), (4, 2), (11, 10), (3, 3)]
    counted = [(5, 4), (5, 5), (5, 3), (5, 5)]
    eng = _Stub(9, ranks, counted)
    res = linkpred.sampled_evaluation(eng, test, filt, negatives=5, seed=3)
    call = eng.calls[0]
    want = np.random.default_rng(3).integers(0, 9, size=(4, 5), dtype=np.int32)
    assert call["lists"] is None and len(call["candidates"]) == 4
    assert all(np.array_equal(c, w) for c, w in zip(call["candidates"], want))
    assert call["ent"].tolist() == [1, 0, 3, 2] and call["truth"].tolist() == [0, 1, 2, 3]
    assert call["filt"] is filt
    assert res["queries"] == 4 and res["counted"] == {"raw": 20, "filtered": 17}
    assert res["raw"]["mean_rank"] == (1 + 4 + 11 + 3) / 4 and res["filtered"]["mean_rank"] == (1 + 2 + 10 + 3) / 4
    assert res["raw"]["hits@1"] == 1 / 4 and res["raw"]["hits@3"] == 2 / 4 and res["raw"]["hits@10"] == 3 / 4
    assert res["filtered"]["hits@3"] == 3 / 4 and res["filtered"]["hits@10"] == 1.0
    assert res["filtered"]["mrr"] == pytest.approx((1 + 1 / 2 + 1 / 10 + 1 / 3) / 4, rel=1e-15)
    assert res["ranks"].tolist() == [[1, 1, 4, 2], [11, 10, 3, 3]]
    # a different seed draws other lists; the same seed the same
    eng2 = _Stub(9, ranks, counted)
    linkpred.sampled_evaluation(eng2, test, filt, negatives=5, seed=4)
    assert not all(np.array_equal(a, b) for a, b in zip(eng2.calls[0]["candidates"], call["candidates"]))
    # one shared list: uploaded once, named by every query
    eng3 = _Stub(9, ranks, counted)
    linkpred.sampled_evaluation(eng3, test, filt, negatives=np.arange(9))
    assert len(eng3.calls[0]["candidates"]) == 1 and eng3.calls[0]["lists"].tolist() == [0, 0, 0, 0]
    # one list per query
    eng4 = _Stub(9, ranks, counted)
    linkpred.sampled_evaluation(eng4, test, filt, negatives=np.arange(8).reshape(4, 2))
    assert [c.tolist() for c in eng4.calls[0]["candidates"]] == [[0, 1], [2, 3], [4, 5], [6, 7]]
    with pytest.raises(ValueError):
        linkpred.sampled_evaluation(eng4, test, filt, negatives=np.arange(6).reshape(3, 2))
    with pytest.raises(ValueError):
        linkpred.sampled_evaluation(eng4, np.zeros((0, 3), np.int32), filt)


def test_slot_pools_and_type_constrained_evaluation():
    train = np.array([(0, 1, 0), (0, 2, 0), (3, 1, 0), (4, 4, 1)], np.int32)
    valid = np.array([(5, 1, 0)], np.int32)
    test = np.array([(3, 2, 0), (4, 0, 1)], np.int32)
    ds = data.Dataset(6, 3, train, valid, test)
    pools = linkpred.slot_pools(np.concatenate([train, valid, test]), 3)
    assert [p.tolist() for p in pools] == [[0, 3, 5], [1, 2], [4], [0, 4], [], []]
    assert all(p.dtype == np.int32 for p in pools)
    eng = _Stub(6, [(1, 1), (2, 1), (1, 1), (2, 2)], [(2, 1), (1, 0), (0, 0), (1, 1)],
                full=[(2, 1, 3, 1), (1, 1, 5, 4)])
    res = linkpred.type_constrained_evaluation(eng, ds)
    call = eng.calls[0]
    assert call["lists"].tolist() == [0, 1, 2, 3]  # relation * 2 + side
    assert [c.tolist() for c in call["candidates"]] == [p.tolist() for p in pools]
    assert np.array_equal(call["filt"], np.concatenate([train, valid, test]))
    assert eng.calls[1][0] == "rank_triples" and np.array_equal(eng.calls[1][1], test)
    con, unc = res["constrained"], res["unconstrained"]
    assert con["raw"]["mean_rank"] == 6 / 4 and con["filtered"]["mean_rank"] == 5 / 4
    assert con["counted"] == {"raw": 4, "filtered": 2}
    assert unc["raw"]["mean_rank"] == (2 + 3 + 1 + 5) / 4 and unc["filtered"]["mean_rank"] == (1 + 1 + 1 + 4) / 4
    assert unc["filtered"]["hits@3"] == 3 / 4 and unc["raw"]["hits@1"] == 1 / 4
