"""The host half of relation fold-in (kb2e_amd/csrc/foldrel_host.hpp): argument
validation, the stable grouping of the examples by free relation, the unit
order, the batch cap and the known set, checked against brute force by a
stand-alone program built with ASan + UBSan and run directly.  Also
linkpred.fold_in_relations_split / fold_in_relations_evaluation on a stub
engine."""
import os
import subprocess

import numpy as np

from conftest import ROOT
from kb2e_amd import linkpred


def test_grouping_and_validation_match_brute_force(tmp_path):
    exe = tmp_path / "foldrel_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "kb2e_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "foldrel_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip() == "ok"


class _Dataset:
    num_entities, num_relations = 6, 4
    # relations 2 and 3 are held out
    train = np.array([(0, 1, 0), (1, 2, 2), (2, 3, 1), (3, 4, 2), (4, 5, 3), (0, 2, 2)], np.int32)
    valid = np.array([(1, 3, 0), (5, 0, 2), (1, 2, 2)], np.int32)   # the last repeats a training triple
    test = np.array([(2, 0, 3), (4, 1, 2), (5, 5, 1)], np.int32)


def test_fold_in_relations_split():
    ds = _Dataset()
    train, sup, qry, known = linkpred.fold_in_relations_split(ds, [3, 2], support=0.5)
    assert train.tolist() == [[0, 1, 0], [2, 3, 1]]
    assert known.tolist() == np.concatenate([ds.train, ds.valid, ds.test]).tolist()
    # 2: (1,2,2) (3,4,2) (0,2,2) (5,0,2) (4,1,2) -> 3 + 2; 3: (4,5,3) (2,0,3) -> 1 + 1
    assert sup.tolist() == [[1, 2, 2], [3, 4, 2], [0, 2, 2], [4, 5, 3]]
    assert qry.tolist() == [[5, 0, 2], [4, 1, 2], [2, 0, 3]]
    _, sup1, qry1, _ = linkpred.fold_in_relations_split(ds, [2, 3], support=0.0)  # at least one example each
    assert sup1.tolist() == [[1, 2, 2], [4, 5, 3]] and len(qry1) == 5


class _Stub:
    """Stands in for an Engine: records the calls; ranks improve once fold_in_relations ran."""
    log = []

    def __init__(self, model, dim, ne, nr, **kw):
        _Stub.log.append(("create", model, dim, ne, nr, kw["transr_compat"], kw["schedule"]))
        self.dim, self.folded = dim, False

    def upload_triples(self, t):
        _Stub.log.append(("upload", np.asarray(t).tolist()))

    def init_params(self):
        return np.zeros((6, self.dim)), np.zeros((4, self.dim)), None

    def transr_seed(self, ent, rel):
        _Stub.log.append(("transr_seed",))

    def train_epoch(self):
        _Stub.log.append(("epoch",))
        return 0.0, 0

    def synchronize(self):
        pass

    def rank_triples(self, test, filt):
        _Stub.log.append(("rank", np.asarray(test).tolist(), len(filt)))
        base = np.array([[9, 8, 7, 6], [5, 4, 3, 2], [20, 12, 30, 10]], np.int64)
        return base // 2 if self.folded else base

    def rank_relations(self, test, filt):
        _Stub.log.append(("rank_relations", np.asarray(test).tolist(), len(filt)))
        base = np.array([[4, 3], [4, 4], [2, 2]], np.int64)
        return base - 1 if self.folded else base

    def fold_in_relations(self, free, examples, known=None, *, epochs, batch_size=1, seed=0, side=2, max_sweeps=0,
                          rel=None, w=None):
        _Stub.log.append(("fold_in_relations", np.asarray(free).tolist(), np.asarray(examples).tolist(), len(known),
                          epochs, batch_size, seed, side))
        self.folded = True
        return (np.ones((2, self.dim)), np.ones((2, self.dim, self.dim)), np.array([[3.0, 1.0], [2.0, 0.5]]),
                np.array([[4, 1, 0], [2, 0, 1]], np.int64))

    def close(self):
        _Stub.log.append(("close",))


def test_fold_in_relations_evaluation_on_a_stub_engine():
    ds = _Dataset()
    _Stub.log = []
    res = linkpred.fold_in_relations_evaluation(ds, "R", 4, [2, 3], support=0.5, epochs=2, fold_epochs=7, batch_size=5,
                                                fold_seed=3, side=1, make_engine=_Stub)
    qry = [[5, 0, 2], [4, 1, 2], [2, 0, 3]]
    assert _Stub.log == [("create", "R", 4, 6, 4, False, "ordered"), ("upload", [[0, 1, 0], [2, 3, 1]]),
                         ("transr_seed",), ("epoch",), ("epoch",), ("rank", qry, 12), ("rank_relations", qry, 12),
                         ("fold_in_relations", [2, 3], [[1, 2, 2], [3, 4, 2], [0, 2, 2], [4, 5, 3]], 12, 7, 5, 3, 1),
                         ("rank", qry, 12), ("rank_relations", qry, 12), ("close",)]
    assert (res["held_out"], res["support"], res["query"]) == (2, 4, 3)
    assert res["rank_before"] == (8 + 6 + 4 + 2 + 12 + 10) / 6 and res["rank_after"] == (4 + 3 + 2 + 1 + 6 + 5) / 6
    assert res["hits10_before"] == 5 / 6 and res["hits10_after"] == 1.0
    assert res["rel_rank_before"] == (3 + 4 + 2) / 3 and res["rel_rank_after"] == (2 + 3 + 1) / 3
    assert (res["loss_first"], res["loss_last"]) == (5.0, 1.5)
    assert (res["active"], res["failed"], res["capped"]) == (6, 1, 1)
    assert res["rel_rows"].shape == (2, 4) and res["w_rows"].shape == (2, 4, 4)
