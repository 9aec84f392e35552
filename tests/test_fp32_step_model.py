"""The per-batch FP32 guard itself (tests/fp32_step.py), CPU only.

The GPU cases (test_gpu_fp32_step.py) are worth what their comparator and their
preconditions are worth, so both are checked here on the FP64 oracle alone:
planted errors of the kinds a float kernel could make are flagged at the bar the
GPU cases use and localised to the table and row they sit in (the oracle against
itself is exact, so every other row differs by exactly zero); a clean run passes;
sign_args reproduces the oracle's own update directions; and every committed seed
meets the hinge and sign guards on the reference alone, its tables rounded to
float between the batches -- the CPU-checkable half of every GPU case.
"""
import numpy as np
import pytest

import fp32_step as fs
from fp32_step import ELEM_ATOL, RATE, Case
from oracle import orc
from oracle.parallel import transe_parallel_batches, transr_parallel_batches

ALL_CASES = fs.ORDERED_CASES + fs.PARALLEL_CASES
# the planted errors: one small case a model and schedule family
PLANT_CASES = [c for c in ALL_CASES if c.id in ("ord-E17-L1", "ord-H33-L1", "ord-R20-L1", "par-E17-L1", "par-R20-L1-sub1")]


def _first_batch(case):
    """(before, reference after, touches) of the case's first batch, reference alone."""
    res = next(fs.lockstep(case))
    before, after, _ = res.tables
    return before, after, res.pre["touches"]


def _copy(tabs):
    return [None if t is None else np.array(t) for t in tabs]


def test_plant_cases_present():
    assert len(PLANT_CASES) == 5


@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c.id)
def test_committed_seed_meets_preconditions(case):
    """The reference alone: hinge slack >= 1e-4 over every sample and, under L1,
    |x| >= 1e-6 over every sign argument of the active samples, in each of the
    compared batches; and rounding the tables to float stays far below the bar."""
    n = 0
    for res in fs.lockstep(case):
        fs.assert_preconditions(res.pre, case.l1, (case.id, res.batch))
        # what a missed update would cost: >= 3 orders above the bar under L1 (steps of rate), >= 2
        # under L2 (steps of 2 rate |d|, with |d| ~ 0.1 from the init draws)
        assert res.moved > (1e3 if case.l1 else 1e2) * case.atol, (case.id, res.moved)
        assert max(v[0] for v in res.diffs.values()) < 1e-7     # float rounding of unit-ball rows
        assert res.pre["touches"]["ent"].max() <= 40, res.pre["touches"]["ent"].max()
        n += 1
    assert n == fs.NB


@pytest.mark.parametrize("case", PLANT_CASES, ids=lambda c: c.id)
def test_clean_self_comparison_passes(case):
    for res in fs.lockstep(case):
        assert fs.check_batch(case, res) < 1e-7
        _, after, _ = res.tables
        assert fs.rows_over(after, _copy(after), 0.0) == []
        assert all(v[0] == 0.0 for v in fs.compare_tables(_copy(after), after).values())


@pytest.mark.parametrize("case", PLANT_CASES, ids=lambda c: c.id)
def test_planted_element_error_is_localised(case):
    """One element of one touched row off by rate / 8."""
    _, after, touches = _first_batch(case)
    for name, idx in (("ent", 0), ("rel", 1)):
        row = int(np.nonzero(touches[name])[0][-1])
        got = _copy(after)
        got[idx][row, case.dim // 2] += RATE / 8
        assert fs.rows_over(got, after, ELEM_ATOL) == [(name, (row,))]
        assert fs.rows_over(got, after, 0.0) == [(name, (row,))]
        d = fs.compare_tables(got, after)
        assert d[name][1] == (row,) and abs(d[name][0] - RATE / 8) < 1e-15
        assert all(v[0] == 0.0 for k, v in d.items() if k != name)


@pytest.mark.parametrize("case", PLANT_CASES, ids=lambda c: c.id)
def test_planted_norm_tail_drop_is_localised(case):
    """One touched row scaled as if its last element had been left out of the norm
    sum: u / sqrt(1 - u_last^2) for the unit row u."""
    _, after, touches = _first_batch(case)
    ent = after[0]
    touched = np.nonzero(touches["ent"])[0]
    row = int(touched[np.abs(ent[touched, -1]).argmax()])
    got = _copy(after)
    u = ent[row] / np.linalg.norm(ent[row])
    got[0][row] = ent[row] / np.sqrt(1.0 - u[-1] ** 2)
    assert fs.rows_over(got, after, ELEM_ATOL) == [("ent", (row,))]
    assert fs.compare_tables(got, after)["ent"][1] == (row,)


@pytest.mark.parametrize("case", [c for c in PLANT_CASES if c.model == "R"], ids=lambda c: c.id)
def test_planted_stale_relation_matrix_is_localised(case):
    """One relation's matrix left at its pre-batch value (a skipped relation)."""
    before, after, touches = _first_batch(case)
    rel = int(np.nonzero(touches["rel"])[0][0])
    got = _copy(after)
    got[2][rel] = before[2][rel]
    over = fs.rows_over(got, after, ELEM_ATOL)
    assert over and all(name == "w" and row[0] == rel for name, row in over)
    d = fs.compare_tables(got, after)
    assert d["w"][1][0] == rel and d["w"][0] > 10 * ELEM_ATOL
    assert d["ent"][0] == 0.0 and d["rel"][0] == 0.0
    # and the same for TransR's relation row: the relation's translation left behind
    got = _copy(after)
    got[1][rel] = before[1][rel]
    assert fs.rows_over(got, after, ELEM_ATOL) == [("rel", (rel,))]


def test_check_batch_rejects_planted_error():
    case = PLANT_CASES[2]
    res = next(fs.lockstep(case))
    row = int(np.nonzero(res.pre["touches"]["ent"])[0][0])
    got = _copy(res.tables[2])
    got[0][row, -1] += RATE / 8
    res.diffs = fs.compare_tables(got, res.tables[1])
    with pytest.raises(AssertionError, match="tables"):
        fs.check_batch(case, res)
    res.diffs = fs.compare_tables(res.tables[2], res.tables[1])
    res.got = (res.ref[0], res.ref[1] + 1)
    with pytest.raises(AssertionError, match="active"):
        fs.check_batch(case, res)


@pytest.mark.parametrize("corrupted", [False, True])
@pytest.mark.parametrize("model", ["E", "H", "R"])
def test_sign_args_match_the_oracle(model, corrupted):
    """A one-update batch at n = 5: the oracle's relation row moves by
    -modifier * rate * sign(x) (oracle/orc.c *_update; TransR then scales it to unit
    length), so sign(sign_args) must reproduce rel_next - rel.  Rows are kept short,
    so common::norm and the TransH orthogonality loop (w.r <= |r| < 0.1) do not
    touch the relation row."""
    n, ne, nr = 5, 6, 2
    rng = np.random.default_rng(7)
    ent = rng.standard_normal((ne, n))
    ent *= 0.3 / np.linalg.norm(ent, axis=1, keepdims=True)
    rel = rng.standard_normal((nr, n))
    rel *= 0.05 / np.linalg.norm(rel, axis=1, keepdims=True)
    w = None
    if model == "H":
        w = rng.standard_normal((nr, n))
        w /= np.linalg.norm(w, axis=1, keepdims=True)
    elif model == "R":
        w = np.eye(n)[None] + 0.2 * rng.standard_normal((nr, n, n))
    m = orc.Model(model, n, ne, nr, rate=RATE, batches=1, transr_compat=False)
    for (h, t, r) in ((0, 1, 0), (4, 2, 1), (3, 3, 1)):
        m.set_tables(ent, rel, w)
        x = fs.sign_args(model, ent, rel, w, h, t, r)
        assert np.abs(x).min() > 1e-6
        m.begin_batch()
        m.gradient_update(h, t, r, corrupted)
        m.end_batch()
        _, rel_next, _ = m.tables()
        s = np.where(x > 0, 1.0, -1.0)
        want = rel[r] + (-1.0 if corrupted else 1.0) * RATE * s
        if model == "R":
            want = want / np.linalg.norm(want)
        assert np.abs(rel_next[r] - want).max() < 1e-15, (rel_next[r] - rel[r], s)
        assert np.array_equal(rel_next[1 - r], rel[1 - r])


def test_batch_preconditions_see_a_near_decision():
    """A sample made to sit on the hinge, and a sign argument made to vanish, are
    both reported: the guard can fail."""
    case = Case("E", 17, 3)
    ds = fs.dataset()
    m = fs.oracle_for(case, ds)
    orc.srand(case.seed)
    m.prep_train()
    si, sj, side = m.sample_stream(m.batch_size())
    pre = fs.batch_preconditions(m, ds, si, sj, side, True)
    assert pre["slack"] > 0 and pre["min_abs_x"] > 0 and 0 < pre["active"] <= len(si)
    assert pre["touches"]["ent"].sum() == 4 * pre["active"] and pre["touches"]["rel"].sum() == 2 * pre["active"]
    # margin moved onto the first sample's energy difference: slack 0 there
    h, t, r = ds.train[si[0]]
    nh, nt = (h, sj[0]) if side[0] else (sj[0], t)
    gap = m.energy(int(nh), int(nt), int(r)) - m.energy(int(h), int(t), int(r))
    assert fs.batch_preconditions(m, ds, si, sj, side, True, margin=gap)["slack"] == 0.0
    # the first active sample's relation row set so that x[0] = 0
    ent, rel, _ = m.tables()
    rel[r, 0] = ent[t, 0] - ent[h, 0]
    m.set_tables(ent, rel)
    assert fs.batch_preconditions(m, ds, si[:1], sj[:1], side[:1], True, margin=1e9)["min_abs_x"] == 0.0
    with pytest.raises(AssertionError, match="min"):
        fs.assert_preconditions({"slack": 1.0, "min_abs_x": 0.0, "active": 1}, True)
    with pytest.raises(AssertionError, match="slack"):
        fs.assert_preconditions({"slack": 9e-5, "min_abs_x": 1.0, "active": 1}, True)


def test_parallel_record_matches_batch_preconditions_and_changes_nothing():
    """The PARALLEL models' optional `record` reports the same slack and |x| as
    batch_preconditions does from the C oracle's energies, and leaves the models'
    results bit for bit as they are without it."""
    ds = fs.dataset()
    for case in (Case("E", 17, 2, schedule="parallel"), Case("R", 8, 2, schedule="parallel", sub=2)):
        m = fs.oracle_for(case, ds)
        orc.srand(case.seed)
        m.prep_train()
        B = m.batch_size()
        si, sj, side = m.sample_stream(B)
        pre = fs.batch_preconditions(m, ds, si, sj, side, True)
        outs = []
        for rec in (None, {}):
            ent, rel, w = m.tables()
            if case.model == "E":
                la = transe_parallel_batches(ent, rel, ds.train, si, sj, side, B, 1, rate=RATE, record=rec)
            else:
                la = transr_parallel_batches(ent, rel, w, ds.train, si, sj, side, B, 1, rate=RATE, cons="chunk1", sub=2,
                                             record=rec)
            outs.append((la, ent, rel, w))
        assert outs[0][0] == outs[1][0]
        for a, b in zip(outs[0][1:], outs[1][1:]):
            assert a is None or np.array_equal(a, b)
        assert abs(rec["slack"][0].min() - pre["slack"]) < 1e-12
        assert abs(rec["min_abs_x"][0].min() - pre["min_abs_x"]) < 1e-12
        assert int(rec["active"][0].sum()) == pre["active"] == outs[0][0][1]
