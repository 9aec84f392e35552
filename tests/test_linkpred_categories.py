"""relation_categories / hits_by_category (kb2e_amd/linkpred.py) on a hand-made
set with one relation per category, and hand-made ranks."""
import numpy as np
import pytest

from kb2e_amd.linkpred import hits_by_category, relation_categories

# (head, tail, relation)
TRAIN = np.array([
    # r0, 1-1: three disjoint pairs
    (0, 1, 0), (2, 3, 0), (4, 5, 0),
    # r1, 1-N: each head has three tails, each tail one head
    (0, 10, 1), (0, 11, 1), (0, 12, 1), (1, 13, 1), (1, 14, 1), (1, 15, 1),
    # r2, N-1: each tail has two heads
    (20, 7, 2), (21, 7, 2), (22, 8, 2), (23, 8, 2),
    # r3, N-N: complete 2 x 2
    (30, 40, 3), (30, 41, 3), (31, 40, 3), (31, 41, 3),
    # a duplicate line counts once
    (0, 1, 0),
], dtype=np.int32)


def test_relation_categories():
    cats, tph, hpt = relation_categories(TRAIN, 5)
    assert cats == ["1-1", "1-N", "N-1", "N-N", "1-1"]  # r4 has no triples
    assert tph.tolist() == [1.0, 3.0, 1.0, 2.0, 0.0]
    assert hpt.tolist() == [1.0, 1.0, 2.0, 2.0, 0.0]


def test_threshold_is_inclusive_at_one_and_a_half():
    # two heads: one with two tails, one with one -> tph = 1.5 -> "many"
    train = np.array([(0, 1, 0), (0, 2, 0), (3, 4, 0)], dtype=np.int32)
    cats, tph, hpt = relation_categories(train, 1)
    assert tph[0] == 1.5 and hpt[0] == 1.0 and cats == ["1-N"]


def test_hits_by_category():
    cats = ["1-1", "1-N", "N-1", "N-N"]
    test = np.array([(0, 1, 0), (2, 3, 0), (0, 10, 1), (1, 13, 1), (1, 14, 1), (20, 7, 2)], dtype=np.int32)
    # head raw, head filtered, tail raw, tail filtered
    ranks = np.array([
        (50, 1, 50, 11),
        (50, 10, 50, 10),
        (1, 30, 1, 2),
        (1, 3, 1, 40),
        (1, 11, 1, 10),
        (1, 10, 1, 1),
    ], dtype=np.int64)
    out = hits_by_category(ranks, test, cats)
    assert out["1-1"] == {"count": 2, "head": 1.0, "tail": 0.5}
    assert out["1-N"]["count"] == 3
    assert out["1-N"]["head"] == pytest.approx(1 / 3) and out["1-N"]["tail"] == pytest.approx(2 / 3)
    assert out["N-1"] == {"count": 1, "head": 1.0, "tail": 1.0}
    assert out["N-N"] == {"count": 0, "head": None, "tail": None}
    at1 = hits_by_category(ranks, test, cats, at=1)
    assert at1["1-1"] == {"count": 2, "head": 0.5, "tail": 0.0}
    with pytest.raises(ValueError):
        hits_by_category(ranks[:2], test, cats)
