"""The numpy model of entity fold-in (tests/fold_in_model.py) against the FP64
oracle, on the CPU.

For one sample the frozen step is the reference's `prebatch; train_kb;
postbatch` on a batch of that one sample, with every row but the free entity's
put back afterwards -- exactly for TransE, and for TransH / TransR whenever
neither coupling loop fires (the oracle's loops move the normal / the matrix
too, the frozen ones cannot).  Where the model's loops do fire, their
post-conditions and sweep counts are checked against a plain restatement.
Also: the committed GPU cases keep every guard on the model alone.
"""
import numpy as np
import pytest

import fold_in_model as fm
from oracle import orc


def _no_loop_case(model, l1, dim, seed):
    """Inputs on which the coupling loops stay mostly quiet: TransH normals that are unit vectors of axes on
    which every entity row is zero; TransR matrices of half the identity's size."""
    c = fm.Case(model, l1, dim, 2, seed, epochs=4, scale=0.9, wscale=0.0 if model == "H" else 0.5)
    # (TransR: the oracle normalises the updated matrix's rows, after which about half of its loops fire)
    ent, rel, w, free, ex, known = fm.random_case(c, per_free=100 if model == "R" else 30)
    if model == "H":
        w = np.zeros_like(w)
        for r in range(len(w)):
            w[r, r] = 1.0
        ent[:, :len(w)] = 0.0
    return c, ent, rel, w, free, ex, known


def _site_iterations():
    return [orc.lib().orc_site_iterations(s) for s in range(3)]


@pytest.mark.parametrize("model,l1", [("E", True), ("E", False), ("H", True), ("R", True), ("R", False)])
def test_model_is_the_oracles_one_sample_batch(model, l1):
    c, ent, rel, w, free, ex, known = _no_loop_case(model, l1, 12, 3)
    res = fm.fold_in(model, ent, rel, w, free, ex, known, lr=c.lr, margin=c.margin, l1=l1, epochs=c.epochs,
                     seed=c.seed, side=2, trace=True)
    m = orc.Model(model, c.dim, ent.shape[0], rel.shape[0], rate=c.lr, margin=c.margin, distance=0 if l1 else 1,
                  transr_compat=False)
    compared = 0
    for tr in res.trace:
        if any(sweeps for _, _, sweeps, _ in tr["loops"]):
            continue  # the model's own loop fired
        f = tr["f"]
        tab = ent.copy()
        tab[f] = tr["before"]
        m.set_tables(tab, rel, w)
        assert m.energy(*tr["pos"]) == tr["epos"] and m.energy(*tr["neg"]) == tr["eneg"]
        before = _site_iterations()
        m.begin_batch()
        m.gradient_update(*tr["pos"], False)
        m.gradient_update(*tr["neg"], True)
        m.end_batch()
        if _site_iterations() != before:
            continue  # the oracle's loop fired (it also sees the updated normal / matrix)
        got = m.tables()[0][f]
        assert np.array_equal(got, tr["after"]), (tr["pos"], tr["neg"], np.max(np.abs(got - tr["after"])))
        compared += 1
    assert compared >= 200, compared


@pytest.mark.parametrize("c", [c for c in fm.CASES if c.model != "E"], ids=lambda c: c.id)
def test_coupling_loops_meet_their_post_conditions(c):
    ent, rel, w, free, ex, known = fm.random_case(c)
    res = fm.fold_in(c.model, ent, rel, w, free, ex, known, lr=c.lr, margin=c.margin, l1=c.l1, epochs=c.epochs,
                     seed=c.seed, side=c.side, trace=True)
    fired = 0
    for tr in res.trace:
        for r, entered, sweeps, left in tr["loops"]:
            # a plain restatement of the loop from the row it was entered with
            y, n = entered.copy(), 0
            if c.model == "H":
                while w[r] @ y > 0.1:
                    y, n = y - c.lr * w[r], n + 1
                assert fm.ssum(w[r] * left) <= 0.1
            else:
                while np.sum((y @ w[r]) ** 2) > 1:
                    y, n = y - c.lr * 2.0 * (w[r] @ (y @ w[r])), n + 1
                assert fm.ssum(fm.colsum(w[r], left) ** 2) <= 1
            assert n == sweeps
            assert np.allclose(y, left, rtol=0, atol=1e-12)
            fired += sweeps > 0
    assert fired >= 1 and res.counts[:, 2].sum() == 0


def test_sweep_cap_stops_the_loop_and_counts():
    c = next(c for c in fm.CASES if c.model == "H" and c.dim == 8 and c.side == 2)
    full, capped = fm.run_case(c), fm.run_case(c, max_sweeps=5)
    assert max(full.sweeps) > 5 and full.counts[:, 2].sum() == 0
    assert capped.counts[:, 2].sum() >= 1 and max(capped.sweeps) == 5
    assert not np.array_equal(full.rows, capped.rows)


@pytest.mark.parametrize("c", fm.CASES + fm.BOUNDARY + fm.BOUNDARY_L2, ids=lambda c: c.id)
def test_committed_gpu_cases_meet_the_guards(c):
    res = fm.run_case(c)
    assert res.min_slack >= fm.GUARD and res.min_abs_g >= fm.GUARD and res.min_loop_gap >= fm.GUARD
    if c in fm.CASES:
        assert fm.case_ok(c, res)


def test_special_gpu_inputs_meet_the_guards():
    for name, make in fm.SPECIAL.items():
        res = make()[1]
        assert res.guards() >= fm.GUARD, name


def test_stream_is_kb2e_corrupt_triples():
    # the state is mix(seed); the counter (p * count + i) << 7 and the draw index are added before mixing
    assert fm.mix(0) == 0
    assert fm.draw(fm.mix(7), 2, 10, 3, 5) == fm.mix(fm.mix(7) + ((2 * 10 + 3) << 7) + 5)
    assert fm.draw(fm.mix(7), 0, 10, 3, 0) != fm.draw(fm.mix(7), 1, 10, 3, 0)
