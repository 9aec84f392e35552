"""The numpy model of relation fold-in (tests/fold_rel_model.py) against the
FP64 oracle, on the CPU.

A batch of the model is the reference's `prebatch; train_kb ...; postbatch` over
the batch's active samples with the entity rows put back afterwards: exactly for
TransE, and for TransH / TransR whenever no loop against an entity row fires
(the oracle's loops see and move the updated entity rows, the frozen ones
cannot).  The pin drives the oracle's begin_batch / gradient_update / end_batch
over the same active triples and demands the same bits.  Where the model's
frozen loops do fire, their post-conditions and sweep counts are checked
against a plain restatement.  Also: the committed GPU cases keep every guard on
the model alone and contain what the GPU tests need them to contain.
"""
import numpy as np
import pytest

import fold_in_model as fm
import fold_rel_model as frm
from oracle import orc

MODELS = [("E", True), ("E", False), ("H", True), ("R", True), ("R", False)]


def _quiet_case(model, l1, dim, seed):
    """Inputs on which the loops against entity rows stay quiet, in the model and in the oracle (whose loops see
    the entity rows after their own update and normalisation).  TransH: start normals that are unit vectors of
    axes on which every entity row is zero.  TransR: start matrices whose rows 2m and 2m + 1 are both the unit
    vector of axis 2m, and entity rows with e[2m + 1] = -e[2m] / 2, so that |eW|^2 = |e|^2 / 5."""
    c = frm.Case(model, l1, dim, 2, seed, epochs=3, scale=0.6)
    ent, rel, w, free, ex, known = frm.random_case(c, per_free=60)
    nr = len(rel)
    if model == "H":
        w = np.zeros_like(w)
        for r in range(nr):
            w[r, r] = 1.0
        ent[:, :nr] = 0.0
    if model == "R":
        rng = np.random.default_rng(seed + 100)
        ent[:, 1::2] = -0.5 * ent[:, 0::2]
        w = np.zeros_like(w)
        for j in range(dim):
            w[:, j, j - j % 2] = 1.0
        w += rng.normal(size=w.shape) * 0.01
    return c, ent, rel, w, free, ex, known


def _sites(model):
    # TransH: site 0 is the loop of r against w, which relation fold-in keeps whole
    return [orc.lib().orc_site_iterations(s) for s in ((1, 2) if model == "H" else (0, 1, 2))]


@pytest.mark.parametrize("batch_size", [1, 4])
@pytest.mark.parametrize("model,l1", MODELS)
def test_model_is_the_oracles_batch_with_the_entity_writes_removed(model, l1, batch_size):
    c, ent, rel, w, free, ex, known = _quiet_case(model, l1, 12, 3)
    res = frm.fold_in_relations(model, ent, rel, w, free, ex, known, lr=c.lr, margin=c.margin, l1=l1, epochs=c.epochs,
                                batch_size=batch_size, seed=c.seed, side=2, trace=True)
    m = orc.Model(model, c.dim, ent.shape[0], rel.shape[0], rate=c.lr, margin=c.margin, distance=0 if l1 else 1,
                  transr_compat=False)
    compared = batches = 0
    for tr in res.trace:
        if tr["coupled"]:
            continue  # a frozen loop of the model fired
        rho = tr["rho"]
        rtab, wtab = rel.copy(), None if w is None else w.copy()
        rtab[rho] = tr["rel"]
        if w is not None:
            wtab[rho] = tr["w"]
        m.set_tables(ent, rtab, wtab)
        for pos, neg, epos, eneg in tr["active"]:
            assert m.energy(*pos) == epos and m.energy(*neg) == eneg
        before = _sites(model)
        m.begin_batch()
        for pos, neg, _, _ in tr["active"]:
            m.gradient_update(*pos, False)
            m.gradient_update(*neg, True)
        m.end_batch()
        if model != "E" and _sites(model) != before:
            continue  # a loop of the oracle against an entity row fired
        got = m.tables()
        assert np.array_equal(got[1][rho], tr["rel_after"]), np.max(np.abs(got[1][rho] - tr["rel_after"]))
        if w is not None:
            assert np.array_equal(got[2][rho], tr["w_after"]), np.max(np.abs(got[2][rho] - tr["w_after"]))
        # the oracle left every other relation alone, as the model does by construction
        others = np.setdiff1d(np.arange(len(rel)), [rho])
        assert np.array_equal(got[1][others], rtab[others])
        compared += len(tr["active"])
        batches += 1
    print(f"{model} l1={l1} batch_size={batch_size}: {compared} active samples in {batches} batches compared, "
          f"{len(res.trace) - batches} batches with a firing loop left out")
    assert compared >= 200, compared
    if batch_size > 1:
        assert compared > batches  # some batches did hold several active samples


@pytest.mark.parametrize("c", [c for c in frm.CASES if c.model != "E"], ids=lambda c: c.id)
def test_frozen_loops_meet_their_post_conditions(c):
    ent, rel, w, free, ex, known = frm.random_case(c)
    res = frm.fold_in_relations(c.model, ent, rel, w, free, ex, known, lr=c.lr, margin=c.margin, l1=c.l1,
                                epochs=c.epochs, batch_size=3, seed=c.seed, side=c.side, trace=True)
    fired = 0
    for a, entered, tested, left, sweeps, capped in res.loops:
        assert not capped
        if c.model == "H":
            # the test holds on the normal as the loop last scaled it by its running `sum` (from the second sweep
            # on that is not the unit normal: common/utils.cpp:86-93); the closing norm(w, false) rescales it
            assert a @ tested <= 0.1 and np.allclose(left, tested / np.linalg.norm(tested), rtol=0, atol=1e-15)
            b, run, k = entered / np.linalg.norm(entered), 0.0, 0  # a plain restatement, running sum included
            while True:
                run = np.sqrt(run + b @ b)
                b = b / run
                if not b @ a > 0.1:
                    break
                b, k = b - c.lr * a, k + 1
            assert k == sweeps
            assert np.allclose(b / np.linalg.norm(b), left, rtol=0, atol=1e-12)
        else:
            assert fm.ssum(fm.colsum(left, a) ** 2) <= 1 and tested is left
            W, k = entered.copy(), 0
            while np.sum((a @ W) ** 2) > 1:
                W, k = W - 2.0 * c.lr * np.outer(a, a @ W), k + 1
            assert k == sweeps
            assert np.allclose(W, left, rtol=0, atol=1e-12)
        fired += sweeps > 0
    assert fired >= 1 and res.counts[:, 2].sum() == 0


def test_sweep_cap_stops_the_loop_and_counts():
    c = next(c for c in frm.CASES if c.model == "H" and c.dim == 8 and c.side == 2)
    full, capped = frm.run_case(c, 3), frm.run_case(c, 3, max_sweeps=2)
    assert max(full.sweeps) > 2 and full.counts[:, 2].sum() == 0
    assert capped.counts[:, 2].sum() >= 1 and max(capped.sweeps) == 2
    assert not np.array_equal(full.w, capped.w)


@pytest.mark.parametrize("c", frm.CASES, ids=lambda c: c.id)
def test_committed_gpu_cases_meet_the_guards_and_hold_what_they_must(c):
    for b in frm.BATCHES:
        res = frm.run_case(c, b)
        assert res.min_slack >= fm.GUARD and res.min_abs_g >= fm.GUARD
        assert res.min_norm_gap >= fm.GUARD and res.min_loop_gap >= fm.GUARD
        assert res.inactive >= 1 and res.counts[:, 0].sum() >= 1  # inactive and active hinges
        assert res.rejected >= 1                                    # a rejected draw
        if c.model == "E":
            assert res.norms_fired >= 1                             # a firing norm
        else:
            assert max(res.sweeps) >= 2                             # an entity-coupled loop of >= 2 sweeps
    assert frm.case_ok(c, frm.run_case(c, 1))


@pytest.mark.parametrize("c", frm.BOUNDARY + frm.STAGING, ids=lambda c: c.id)
def test_boundary_cases_meet_the_guards(c):
    for b in (1, 5):
        assert frm.run_case(c, b).guards() >= fm.GUARD


def test_special_gpu_inputs_meet_the_guards():
    for name, make in frm.SPECIAL.items():
        res = make()[1]
        assert res.guards() >= fm.GUARD, name
    inputs, res = frm.long_batch()
    assert np.bincount(inputs[5][:, 2], minlength=5).tolist() == [0, 0, 310, 0, 2000]
    inputs, res = frm.many()
    assert len(inputs[4]) == 70 and res.counts[:, 0].sum() >= 70
    assert frm.one_candidate()[1].counts[:, 1].sum() >= 1 and frm.one_candidate()[1].counts[:, 0].sum() >= 1
    assert frm.complete_graph()[1].counts[:, 1].tolist() == [2 * 3, 4 * 3]


def test_stream_is_kb2e_corrupt_triples():
    # fold_rel_model draws with fold_in_model's functions, which test_fold_in_model pins to kb2e_corrupt_triples:
    # the state is mix(seed); the counter (p * count + i) << 7 and the draw index are added before mixing
    assert frm.draw is fm.draw and frm.mix is fm.mix
    assert fm.draw(fm.mix(7), 2, 10, 3, 5) == fm.mix(fm.mix(7) + ((2 * 10 + 3) << 7) + 5)
    # the model's negatives are the first accepted draws of that stream
    c = frm.CASES[0]
    ent, rel, w, free, ex, known = frm.random_case(c)
    res = frm.fold_in_relations(c.model, ent, rel, w, free, ex, known, lr=c.lr, margin=c.margin, l1=c.l1, epochs=1,
                                seed=c.seed, side=0, trace=True)
    kset = set(map(tuple, known.tolist())) | set(map(tuple, ex.tolist()))
    index = {tuple(t): i for i, t in reversed(list(enumerate(ex.tolist())))}
    checked = 0
    for tr in res.trace:
        for pos, neg, _, _ in tr["active"]:
            i = index[pos]
            if ex.tolist().count(list(pos)) > 1:
                continue
            draws = [fm.draw(fm.mix(c.seed), 0, len(ex), i, a) % len(ent) for a in range(1, 33)]
            ok = [e for e in draws if e != pos[0] and (e, pos[1], pos[2]) not in kset]
            assert neg == (ok[0], pos[1], pos[2])
            checked += 1
    assert checked >= 5
