"""The per-triple rank reference itself (tests/eval_ranks.py), CPU only.

test_gpu_eval_ranks.py holds the engine to eval_ranks.reference_ranks with no
tolerance, so the reference is pinned here to the C oracle (oracle/orc.c, itself
bit-exact against the compiled reference's fixtures, test_oracle_golden.py):

  * sampled candidate rows of its energies equal orc.Model.energy bit for bit,
    for every model, distance and width of the GPU grid, on both table makers,
    FP64 and with the tables rounded through float32;
  * the means and <= 10 fractions of its ranks equal orc.Model.evaluate's four
    numbers (the oracle ranks ties after the truth too, so this holds with ties
    present);
  * on the exact tables the energies do not depend on the order of their sums
    (forwards == backwards, every candidate of every test side);
  * a condition, not a measurement: on the exact tables at least one test side in
    eight has a candidate tying the truth, the oracle counts ties too, and at
    least three test triples have entity 0 or one of its copies as head or tail
    -- so the tie cases cannot silently become tie-free.

Observed tie shares of the 120 sides (exact tables, seed n; printed with -s):
1.000 at E2-L1 down to 0.158 = 19 / 120 at H130, H512, R65-L2 and R130-L2, where
only the copies of entity 0 still tie; bar 0.125.
"""
import numpy as np
import pytest

import eval_ranks as er
from oracle import orc

_MEMO = {}


def _setup():
    if "ds" not in _MEMO:
        _MEMO["ds"] = er.tiny_set()
    return _MEMO["ds"]


def _oracle(model, n, l1, ds, tables):
    m = orc.Model(model, n, ds.num_entities, ds.num_relations, distance=0 if l1 else 1, transr_compat=False)
    m.set_tables(*tables)
    return m


def _check_against_oracle(model, n, l1, tables, precision=64):
    ds, test, filt = _setup()
    en = er.reference_energies(model, tables, test, l1, precision)
    m = _oracle(model, n, l1, ds, tuple(er.round32(t) for t in tables) if precision == 32 else tables)
    ne = ds.num_entities
    for i in (0, 17, er.NTEST - 1):
        h, t, r = (int(x) for x in test[i])
        assert np.array_equal(en[i, 0], np.array([m.energy(x, t, r) for x in range(ne)])), (i, "head")
        assert np.array_equal(en[i, 1], np.array([m.energy(h, x, r) for x in range(ne)])), (i, "tail")
    ranks = er.ranks_from_energies(en, test, filt)
    assert ranks.shape == (er.NTEST, 4) and ranks.dtype == np.int64 and (ranks >= 1).all()
    assert (ranks[:, 1] <= ranks[:, 0]).all() and (ranks[:, 3] <= ranks[:, 2]).all()
    exp = m.evaluate(test, filt)
    got = er.summary(ranks)
    for k in ("raw_rank", "raw_hits10", "filtered_rank", "filtered_hits10"):
        assert got[k] == pytest.approx(exp[k], abs=1e-12), k
    return en, exp


@pytest.mark.parametrize("case", er.GRID, ids=er.grid_id)
def test_reference_matches_oracle_random_tables(case):
    model, n, l1 = case
    ds, _, _ = _setup()
    _check_against_oracle(model, n, l1, er.grid_tables("random", model, ds.num_entities, ds.num_relations, n))


@pytest.mark.parametrize("case", er.GRID, ids=er.grid_id)
def test_reference_matches_oracle_exact_tables_with_ties(case):
    model, n, l1 = case
    ds, test, _ = _setup()
    tables = er.exact_tables(model, ds.num_entities, ds.num_relations, n, n)
    assert all(t is None or np.array_equal(t, er.round32(t)) for t in tables)
    en, exp = _check_against_oracle(model, n, l1, tables)
    # order-independent: summed backwards, not one energy differs
    assert np.array_equal(en, er.reference_energies(model, tables, test, l1, reverse=True))
    # the tie condition
    share = er.tie_sides(en, test).mean()
    print(f"{er.grid_id(case)}: tie share {share:.3f}, oracle ties {exp['ties']}")
    assert share >= er.MIN_TIE_SHARE, share
    assert exp["ties"] > 0
    dup = er.duplicate_entities(ds.num_entities)
    assert (np.isin(test[:, 0], dup) | np.isin(test[:, 1], dup)).sum() >= 3
    assert (tables[0][dup] == tables[0][0]).all()


@pytest.mark.parametrize("case", [("E", 20, True), ("E", 130, False), ("H", 20, True), ("H", 130, True),
                                  ("R", 20, True), ("R", 65, False)], ids=er.grid_id)
def test_reference_fp32_tables_match_oracle_on_rounded_tables(case):
    model, n, l1 = case
    ds, test, _ = _setup()
    tables = er.grid_tables("random", model, ds.num_entities, ds.num_relations, n)
    assert not np.array_equal(tables[0], er.round32(tables[0]))
    en, _ = _check_against_oracle(model, n, l1, tables, precision=32)
    assert not np.array_equal(en, er.reference_energies(model, tables, test, l1))


def test_tie_and_filter_rules_on_a_hand_made_row():
    """Five entities in one dimension, relation 0 = 0: energies are |x - fixed|."""
    ent = np.array([[0.0], [1.0], [1.0], [3.0], [-1.0]])
    rel = np.zeros((1, 1))
    test = np.array([(3, 0, 0)])  # truth energy 3
    en = er.reference_energies("E", (ent, rel, None), test, True)
    assert en[0, 0].tolist() == [0.0, 1.0, 1.0, 3.0, 1.0]   # heads x of (x, 0, 0)
    assert en[0, 1].tolist() == [3.0, 2.0, 2.0, 0.0, 4.0]   # tails x of (3, x, 0)
    # head side: 0, 1, 2, 4 strictly below the truth; tail side: 1, 2, 3 below, 4 above
    assert er.ranks_from_energies(en, test, None).tolist() == [[5, 5, 4, 4]]
    # a tying candidate is not counted: entity 4 moved to the truth's energy on the head side
    ent2 = ent.copy()
    ent2[4] = -3.0
    en2 = er.reference_energies("E", (ent2, rel, None), test, True)
    assert en2[0, 0, 4] == en2[0, 0, 3] and er.tie_sides(en2, test).tolist() == [[True, False]]
    assert er.ranks_from_energies(en2, test, None)[0, 0] == 4
    # filter rows are (head, tail, relation): (1, 0, 0) removes head candidate 1 only,
    # its mirror (0, 1, 0) removes nothing of this triple, (3, 2, 0) removes tail candidate 2
    assert er.ranks_from_energies(en, test, np.array([(1, 0, 0)])).tolist() == [[5, 4, 4, 4]]
    assert er.ranks_from_energies(en, test, np.array([(0, 1, 0)])).tolist() == [[5, 5, 4, 4]]
    assert er.ranks_from_energies(en, test, np.array([(3, 2, 0), (3, 2, 0)])).tolist() == [[5, 5, 4, 3]]
    # the truth's own row in the filter changes nothing
    assert er.ranks_from_energies(en, test, np.array([(3, 0, 0)])).tolist() == [[5, 5, 4, 4]]
