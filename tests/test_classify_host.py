"""The host half of triple classification (kb2e_amd/csrc/classify_host.hpp): the
per-(relation, slot) candidate lists a constrained negative is drawn from, the
counter-based stream's mixer and the labelled-file parser of classifyTrans*.
A stand-alone program checks them against brute-force loops (empty known set,
duplicate triples, a relation absent from it, a slot with a single entity,
malformed labelled lines), built with ASan + UBSan and run directly.  Also
linkpred.triple_classification's arithmetic on a stub engine with hand-made
labels, failed negatives included."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from kb2e_amd import data, linkpred


def test_candidate_lists_and_label_parser_match_brute_force(tmp_path):
    exe = tmp_path / "classify_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "kb2e_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "classify_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().splitlines()[-1] == "ok"
    assert out.stdout.count("Labelled triple skipped") == 4


class _Stub:
    """Stands in for an Engine: energy = head + tail (exact small integers);
    corrupt replaces the tail by tail + 10 and fails on the rows it was told to."""

    def __init__(self, fail_rows=()):
        self.fail_rows = set(fail_rows)
        self.calls = []

    def corrupt(self, triples, known, seed=0, side=2, constrained=True):
        self.calls.append(("corrupt", len(triples), len(known), seed, side, constrained))
        neg = np.array(triples, dtype=np.int32)
        neg[:, 1] += 10
        failed = 0
        for i in range(len(neg)):
            if (seed, i) in self.fail_rows:
                neg[i, :2] = -1
                failed += 1
        return neg, failed

    @staticmethod
    def _energy(t):
        return (t[:, 0] + t[:, 1]).astype(np.float64)

    def fit_thresholds(self, triples, labels):
        self.calls.append(("fit", len(triples)))
        self.fitted = (np.array(triples), np.array(labels))
        # the positives of relation 0 have energy <= 9, its negatives >= 10;
        # relation 1 is cut too low on purpose; relation 2 has no valid triple
        return np.array([9.0, 2.0, 5.0]), np.zeros((3, 3), np.int64), 5.0, 0

    def classify(self, triples, thresholds, with_energy=False):
        t = np.asarray(triples)
        return (self._energy(t) <= np.asarray(thresholds)[t[:, 2]]).astype(np.uint8)


def test_triple_classification_arithmetic_on_a_stub():
    ds = data.Dataset(40, 3, train=np.array([[0, 1, 0]], np.int32),
                      valid=np.array([[1, 2, 0], [2, 3, 0], [1, 3, 1], [0, 1, 1]], np.int32),
                      test=np.array([[3, 4, 0], [1, 1, 1], [2, 2, 1], [0, 2, 2], [4, 4, 2]], np.int32))
    eng = _Stub(fail_rows={(5, 1), (6, 0), (6, 4)})  # valid row 1; test rows 0 and 4 (seed + 1)
    res = linkpred.triple_classification(eng, ds, seed=5, constrained=False)
    assert eng.calls[0] == ("corrupt", 4, 10, 5, 2, False) and eng.calls[1] == ("corrupt", 5, 10, 6, 2, False)
    # the failed valid negative is dropped: 4 positives + 3 negatives are fitted
    assert eng.calls[2] == ("fit", 7)
    vt, vl = eng.fitted
    assert vl.tolist() == [1, 1, 1, 1, 0, 0, 0]
    assert vt[4:].tolist() == [[1, 12, 0], [1, 13, 1], [0, 11, 1]]
    assert res["valid"]["failed"] == 1 and res["test"]["failed"] == 2
    assert res["valid"]["count"] == 7 and res["test"]["count"] == 8
    # valid: relation 0 (thr 9): positives 3, 5 and negative 13 -> 3 of 3; relation 1 (thr 2):
    # positives 4 (missed), 1 (hit), negatives 14, 11 (hit) -> 3 of 4
    assert res["valid"]["per_relation"] == {0: {"count": 3, "accuracy": 1.0}, 1: {"count": 4, "accuracy": 0.75}}
    assert res["valid"]["accuracy"] == 6 / 7
    # test: relation 0: positive 7 (hit), its negative failed -> 1 of 1; relation 1: positives 2 (hit), 4
    # (missed), negatives 12, 14 (hit) -> 3 of 4; relation 2 (thr 5): positives 2 (hit), 8 (missed),
    # negative 12 (hit; the other failed) -> 2 of 3
    assert res["test"]["per_relation"] == {0: {"count": 1, "accuracy": 1.0}, 1: {"count": 4, "accuracy": 0.75},
                                           2: {"count": 3, "accuracy": 2 / 3}}
    assert res["test"]["accuracy"] == 6 / 8
    assert res["thresholds"].tolist() == [9.0, 2.0, 5.0] and res["global_threshold"] == 5.0


def test_triple_classification_takes_labelled_splits():
    ds = data.Dataset(40, 3, train=np.zeros((1, 3), np.int32), valid=np.zeros((0, 3), np.int32),
                      test=np.zeros((0, 3), np.int32))
    eng = _Stub()
    valid = (np.array([[1, 2, 0], [5, 6, 0]]), [1, 0])
    test = (np.array([[1, 3, 0], [9, 9, 0], [1, 0, 1]]), [1, 0, 0])
    res = linkpred.triple_classification(eng, ds, valid=valid, test=test)
    assert eng.calls == [("fit", 2)]  # no negatives are generated
    assert res["valid"]["accuracy"] == 1.0 and res["valid"]["failed"] == 0
    # test: 4 <= 9 positive (hit), 18 > 9 negative (hit), relation 1: 1 <= 2 says positive, labelled 0 (missed)
    assert res["test"]["accuracy"] == 2 / 3
    assert res["test"]["per_relation"] == {0: {"count": 2, "accuracy": 1.0}, 1: {"count": 1, "accuracy": 0.0}}
    with pytest.raises(ValueError):
        linkpred.triple_classification(eng, ds, valid=(np.zeros((2, 3)), [1]), test=test)
