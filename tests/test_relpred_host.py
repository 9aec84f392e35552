"""The host half of relation prediction (kb2e_amd/csrc/predict_host.hpp): the
known relations of every (head, tail) pair, listed once from the filter triples,
and the distinct-entity list of a run of pairs.  A stand-alone program checks
them against brute-force loops (empty filter, duplicate filter triples, queries
sharing a pair, a pair with every relation known, h == t), built with ASan +
UBSan and run directly.  Also linkpred.relation_prediction's arithmetic on
hand-made ranks."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from kb2e_amd import linkpred


def test_known_relation_lists_match_brute_force(tmp_path):
    exe = tmp_path / "relpred_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "kb2e_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "relpred_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip() == "ok"


class _Ranks:
    """Stands in for an Engine: rank_relations returns what it was given."""

    def __init__(self, ranks):
        self.ranks = np.asarray(ranks, dtype=np.int64)
        self.calls = []

    def rank_relations(self, test, filt):
        self.calls.append((len(test), len(filt)))
        return self.ranks


def test_relation_prediction_on_hand_made_ranks():
    # raw, filtered
    ranks = [(1, 1), (3, 1), (12, 10), (11, 11), (2, 2)]
    eng = _Ranks(ranks)
    test = np.zeros((5, 3), np.int32)
    filt = np.zeros((9, 3), np.int32)
    res = linkpred.relation_prediction(eng, test, filt)
    assert eng.calls == [(5, 9)]
    assert res["count"] == 5
    assert res["raw"] == {"mean_rank": 29 / 5, "hits@1": 1 / 5, "hits@10": 3 / 5}
    assert res["filtered"] == {"mean_rank": 25 / 5, "hits@1": 2 / 5, "hits@10": 4 / 5}
    res = linkpred.relation_prediction(eng, test, filt, at=(2, 11))
    assert res["raw"] == {"mean_rank": 29 / 5, "hits@2": 2 / 5, "hits@11": 4 / 5}
    assert res["filtered"] == {"mean_rank": 25 / 5, "hits@2": 3 / 5, "hits@11": 5 / 5}
    with pytest.raises(ValueError):
        linkpred.relation_metrics(np.zeros((0, 2), np.int64))
