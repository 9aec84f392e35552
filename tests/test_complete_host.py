"""The host half of knowledge-base completion (kb2e_amd/csrc/complete_host.hpp):
the strip plan that walks a relation's |H| x |T| candidates without ever
overflowing the record buffer, and the pair id.  A stand-alone program checks
them against brute force (every pair covered once, no strip larger than the
buffer, ragged last strips, tails chunked when a tile of them does not fit),
built with ASan + UBSan and run directly.  Also linkpred.completion's
arithmetic on hand-made Engine.complete output."""
import os
import subprocess

import numpy as np

from conftest import ROOT
from kb2e_amd import linkpred


def test_strip_plan_and_pair_ids_match_brute_force(tmp_path):
    exe = tmp_path / "complete_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "kb2e_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "complete_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip() == "ok"


class _Dataset:
    num_entities, num_relations = 6, 4
    train = np.array([(0, 1, 0), (1, 2, 0), (2, 3, 1)], np.int32)
    valid = np.array([(3, 4, 1), (0, 5, 2)], np.int32)
    # relation 0: two new test triples and one that is also a training triple;
    # relation 1: one (listed twice); relation 2: none; relation 3: one
    test = np.array([(0, 2, 0), (4, 5, 0), (0, 1, 0), (5, 0, 1), (5, 0, 1), (1, 1, 3)], np.int32)


class _Mined:
    """Stands in for an Engine: complete() returns what it was given."""

    def __init__(self, rows, k):
        self.rows, self.k, self.calls = rows, k, []

    def complete(self, relations, k, known=None, constrained=False, exclude_loops=False):
        self.calls.append((np.asarray(relations).tolist(), k, np.asarray(known).tolist(), constrained, exclude_loops))
        nrel = len(relations)
        heads = np.full((nrel, k), -1, np.int32)
        tails = np.full((nrel, k), -1, np.int32)
        en = np.full((nrel, k), np.inf)
        found = np.zeros(nrel, np.int64)
        for q, r in enumerate(np.asarray(relations).tolist()):
            pairs = self.rows[r]
            found[q] = len(pairs)
            for j, (h, t) in enumerate(pairs):
                heads[q, j], tails[q, j], en[q, j] = h, t, float(j)
        return heads, tails, en, found


def test_completion_on_hand_made_output():
    ds = _Dataset()
    rows = {0: [(0, 2), (3, 3), (4, 5)], 1: [(1, 0), (0, 5), (2, 2)], 2: [(1, 4)], 3: []}
    eng = _Mined(rows, 3)
    res = linkpred.completion(eng, ds, 3)
    known = np.concatenate([ds.train, ds.valid]).tolist()
    assert eng.calls == [([0, 1, 2, 3], 3, known, True, True)]
    per = res["per_relation"]
    assert per[0] == {"mined": 3, "test": 2, "hits": 2, "recall": 1.0, "precision": 2 / 3}
    assert per[1] == {"mined": 3, "test": 1, "hits": 0, "recall": 0.0, "precision": 0.0}
    assert per[2] == {"mined": 1, "test": 0, "hits": 0, "recall": None, "precision": 0.0}
    assert per[3] == {"mined": 0, "test": 1, "hits": 0, "recall": 0.0, "precision": None}
    assert (res["k"], res["relations"], res["mined"], res["test"], res["hits"]) == (3, 4, 7, 4, 2)
    assert res["recall"] == 2 / 4 and res["precision"] == 2 / 7
    # chosen relations, one of them twice; the flags go through
    eng = _Mined(rows, 3)
    res = linkpred.completion(eng, ds, 3, constrained=False, exclude_loops=False, relations=[1, 0, 1])
    assert eng.calls == [([1, 0, 1], 3, known, False, False)]
    assert sorted(res["per_relation"]) == [0, 1]
    assert (res["relations"], res["mined"], res["test"], res["hits"]) == (2, 6, 3, 2)
    assert res["recall"] == 2 / 3 and res["precision"] == 2 / 6
    # nothing mined, no test triple of the relation: no rate at all
    res = linkpred.completion_metrics(np.full((1, 2), -1), np.full((1, 2), -1), [0], [2], ds.test, known, 2)
    assert res["recall"] is None and res["precision"] is None and res["mined"] == 0
