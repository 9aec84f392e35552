"""The host half of the conjunctive queries (kb2e_amd/csrc/joint_host.hpp): the
check of the offsets, the chunk plan and the per-query intersection of the
known-candidate lists.  A stand-alone program checks them against brute force,
built with ASan + UBSan and run directly.  Also
linkpred.entity_identification's arithmetic on a stand-in engine that returns
hand-made ranks."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from kb2e_amd import linkpred


def test_offsets_chunk_plan_and_intersections_match_brute_force(tmp_path):
    exe = tmp_path / "joint_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "kb2e_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "joint_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip() == "ok"


class _Dataset:
    num_entities, num_relations = 8, 3
    train = np.array([(0, 1, 0), (6, 7, 2)], np.int32)
    valid = np.array([(7, 6, 1)], np.int32)
    # mentions in file order -- 0: four (one loop skipped), 1: three, 2: three,
    # 3: two, 4: one, 5: one (and a loop)
    test = np.array([(0, 1, 0), (2, 0, 1), (0, 0, 2), (1, 2, 2), (0, 3, 1), (3, 1, 0), (4, 2, 0), (0, 5, 2), (5, 5, 1)],
                    np.int32)


class _Ranked:
    """Stands in for an Engine: rank_joint() records its arguments and returns the ranks it was given."""

    def __init__(self, ranks):
        self.ranks, self.calls = ranks, []

    def rank_joint(self, queries, truth, filt):
        m = len(queries[0])
        self.calls.append(([np.asarray(q).tolist() for q in queries], np.asarray(truth).tolist(),
                           np.asarray(filt).tolist()))
        return np.array(self.ranks[m], np.int64)


def test_entity_identification_on_hand_made_ranks():
    ds = _Dataset()
    # entity 0: (0,1,0) head -> (1, 0, 0); (2,0,1) tail -> (2, 1, 1); the loop (0,0,2) is skipped; (0,3,1) -> (3, 1, 0)
    # entity 1: (0,1,0) tail -> (0, 0, 1); (1,2,2) head -> (2, 2, 0); (3,1,0) tail -> (3, 0, 1)
    # entity 2: (2,0,1) head -> (0, 1, 0); (1,2,2) tail -> (1, 2, 1); (4,2,0) tail -> (4, 0, 1)
    full = {0: [[1, 0, 0], [2, 1, 1], [3, 1, 0]], 1: [[0, 0, 1], [2, 2, 0], [3, 0, 1]], 2: [[0, 1, 0], [1, 2, 1], [4, 0, 1]]}
    ents, patterns = linkpred.identification_queries(ds.test, 3)
    assert ents.tolist() == [0, 1, 2] and ents.dtype == np.int32
    assert [p.tolist() for p in patterns] == [full[0], full[1], full[2]]
    ents2, patterns2 = linkpred.identification_queries(ds.test, 2)
    assert ents2.tolist() == [0, 1, 2, 3]
    assert patterns2[3].tolist() == [[0, 1, 1], [1, 0, 0]]

    ranks = {1: [[5, 4], [1, 1], [20, 10]], 2: [[2, 2], [1, 1], [11, 3]], 3: [[1, 1], [1, 1], [4, 2]]}
    eng = _Ranked(ranks)
    res = linkpred.entity_identification(eng, ds)
    filt = np.concatenate([ds.train, ds.valid, ds.test]).tolist()
    assert len(eng.calls) == 3
    for m, (queries, truth, passed) in zip((1, 2, 3), eng.calls):
        assert queries == [full[e][:m] for e in (0, 1, 2)]
        assert truth == [0, 1, 2]
        assert passed == filt
    assert sorted(res) == [1, 2, 3]
    for m in (1, 2, 3):
        r = np.array(ranks[m], float)
        assert res[m]["count"] == 3
        for col, name in enumerate(("raw", "filtered")):
            got = res[m][name]
            assert got["mean_rank"] == r[:, col].mean()
            assert got["mrr"] == (1.0 / r[:, col]).mean()
            assert got["hits@1"] == (r[:, col] <= 1).mean()
            assert got["hits@10"] == (r[:, col] <= 10).mean()
    assert res[1]["filtered"] == {"mean_rank": 5.0, "mrr": (1 / 4 + 1 + 1 / 10) / 3, "hits@1": 1 / 3, "hits@10": 1.0}
    assert res[1]["raw"]["hits@10"] == 2 / 3

    # the query set follows the largest m: with (1, 2) entity 3 joins
    eng = _Ranked({1: [[1, 1]] * 4, 2: [[2, 1]] * 4})
    res = linkpred.entity_identification(eng, ds, constraints=(1, 2))
    assert [c[1] for c in eng.calls] == [[0, 1, 2, 3]] * 2
    assert eng.calls[1][0][3] == [[0, 1, 1], [1, 0, 0]]
    assert res[2]["count"] == 4 and res[2]["raw"]["mean_rank"] == 2.0
    with pytest.raises(ValueError):
        linkpred.entity_identification(eng, ds, constraints=(5,))
