"""kb2e_renormalize (host masks) and kb2e_renormalize_rows (a device mask over
a range of units) against tests/merge_model.expected_renorm: numpy float64, the
length from a sequential sum of squares, from the tables as the engine holds them.

The tables mix long (1.3..2.0) and short (0.3..0.7) rows, and every mask has a
third of its units off: a row that is masked off must come back bit for bit, a
short row under the shrink constraint (TransE, TransH entities / relations) too,
and the TransH normals and every TransR row go to unit length.  TransR weight
masks have one entry per relation, n matrix rows each.  A device mask is indexed
from `first`.  The padding element of an odd width stays zero (RowReg::load
reads it into every later norm).  Bars as tests/test_gpu_merge_shapes.py: FP64
1e-12, FP32 1e-5 (one wave sum of n <= 512 squares, a square root, a divide).
"""
import itertools

import numpy as np
import pytest
import torch

import merge_model as mm
from gpu_common import tiny
from kb2e_amd.distributed import engine_tables
from kb2e_amd.engine import Engine, EngineError

NE, NR = 37, 5
BAR = {64: 1e-12, 32: 1e-5}


def _engine(model, n, precision):
    return Engine(model, n, NE, NR, precision=precision)


def _upload(eng, tabs):
    eng.upload_params(tabs[0], tabs[1], tabs[2])


def _padding_is_zero(eng, n):
    ld = (n + 1) & ~1
    return all(not t.view(-1, ld)[:, n:].any().item() for t in engine_tables(eng))


def _compare(eng, model, n, tabs, exp, untouched, bar):
    """Downloaded tables against `exp`; `untouched[t]` marks the units that must be bit-identical."""
    got = eng.download_params()
    worst = 0.0
    for t in range(3):
        if tabs[t] is None:
            continue
        assert np.array_equal(got[t][untouched[t]], tabs[t][untouched[t]]), ("untouched unit moved", t)
        worst = max(worst, float(np.abs(got[t] - exp[t]).max()))
    assert worst <= bar, worst
    assert _padding_is_zero(eng, n)
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("n", [3, 65, 129, 385, 512])
@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("model", ["E", "H", "R"])
def test_renormalize_host_masks(model, precision, n):
    tabs, masks = mm.renorm_tables(model, n, NE, NR, precision)
    ntab = 2 if model == "E" else 3
    eng = _engine(model, n, precision)
    worst = 0.0
    try:
        combos = list(itertools.product([False, True], repeat=ntab)) + ["zeros"]
        for combo in combos:
            if combo == "zeros":  # a mask of all zeros changes nothing
                use = [np.zeros(len(masks[t]), np.uint8) for t in range(ntab)]
            else:
                use = [masks[t] if combo[t] else None for t in range(ntab)]
            use += [None] * (3 - ntab)
            _upload(eng, tabs)
            eng.renormalize(*use)
            exp = [None if tabs[t] is None else mm.expected_renorm(model, t, tabs[t], use[t]) for t in range(3)]
            off = [None if tabs[t] is None else
                   (np.zeros(len(tabs[t]), bool) if use[t] is None else use[t] == 0) for t in range(3)]
            worst = max(worst, _compare(eng, model, n, tabs, exp, off, BAR[precision]))
            if combo == "zeros":
                assert all(tabs[t] is None or np.array_equal(exp[t], tabs[t]) for t in range(3))
        # the last call above left the tables as uploaded; one unmasked call: the constraints themselves
        eng.renormalize()
        got = eng.download_params()
        tol = 1e-6 if precision == 32 else 1e-14
        for t in range(ntab):
            before = np.linalg.norm(tabs[t].reshape(-1, n), axis=1)
            after = np.linalg.norm(got[t].reshape(-1, n), axis=1)
            if mm.unit_constraint(model, t):
                assert np.abs(after - 1).max() < tol, (t, "unit length")
            else:  # long rows to length 1, short rows as they were
                assert np.abs(after[before > 1] - 1).max() < tol and np.array_equal(
                    got[t].reshape(-1, n)[before < 1], tabs[t].reshape(-1, n)[before < 1]), (t, "shrink")
    finally:
        eng.close()
    print(f"renormalize {model} fp{precision} n={n}: max |engine - reference| {worst:.3e} (bar {BAR[precision]:.0e})")


def _device_mask(mask):
    m = torch.tensor(np.asarray(mask, dtype=np.uint8), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("model,n,precision", [("E", 65, 64), ("H", 129, 32), ("H", 3, 64), ("R", 65, 64),
                                               ("R", 129, 32), ("R", 385, 64)])
def test_renormalize_rows_device_mask(model, n, precision):
    tabs, _ = mm.renorm_tables(model, n, NE, NR, precision)
    ntab = 2 if model == "E" else 3
    eng = _engine(model, n, precision)
    rng = np.random.default_rng(5)
    worst = 0.0
    try:
        for t in range(ntab):
            units = len(tabs[t])
            ranges = [(3 if units > 8 else 2, units - 5 if units > 8 else 3, "mask"),  # first > 0, masked
                      (2, 0, "mask"), (2, 0, None),  # count = 0
                      (2, 1, "mask"), (units - 1, 1, "mask"),  # one unit; the last unit
                      (1, units - 2, None), (0, units, None)]  # NULL: the whole range, nothing outside
            moved = 0
            for first, count, kind in ranges:
                mask = None
                if kind == "mask":
                    mask = np.ones(max(count, 1), np.uint8)
                    if count > 1:  # not periodic, so an index from 0 or from 2 * first shows
                        mask[:] = rng.random(count) < 0.6
                        mask[0], mask[1], mask[-1] = 1, 0, 1
                _upload(eng, tabs)
                keep = None if mask is None else _device_mask(mask)
                eng.renormalize_rows(t, first, count, None if keep is None else keep.data_ptr())
                exp = [None if x is None else x.copy() for x in tabs]
                on = np.zeros(units, bool)
                if count:
                    m = None if mask is None else mask[:count]
                    exp[t][first:first + count] = mm.expected_renorm(model, t, tabs[t][first:first + count], m)
                    on[first:first + count] = True if m is None else m != 0
                off = [None if x is None else np.ones(len(x), bool) for x in tabs]
                off[t] = ~on
                worst = max(worst, _compare(eng, model, n, tabs, exp, off, BAR[precision]))
                moved += not np.array_equal(exp[t], tabs[t])
            assert moved >= 4, (t, moved)  # the ranges with more than one unit did something
    finally:
        eng.close()
    print(f"renormalize_rows {model} fp{precision} n={n}: max |engine - reference| {worst:.3e} "
          f"(bar {BAR[precision]:.0e})")


@pytest.mark.gpu
def test_renormalize_rows_refuses_bad_ranges():
    for model in ("E", "H"):
        tabs, _ = mm.renorm_tables(model, 20, NE, NR)
        eng = _engine(model, 20, 64)
        try:
            _upload(eng, tabs)
            bad = [(3, 0, 1), (0, -1, 2), (0, NE - 1, 2), (1, NR, 1), (0, 0, NE + 1), (-1, 0, 1), (0, 0, -1)]
            if model == "E":
                bad.append((2, 0, 1))  # TransE has no table 2
            for table, first, count in bad:
                with pytest.raises(EngineError, match="EINVAL"):
                    eng.renormalize_rows(table, first, count)
                got = eng.download_params()
                assert all(x is None or np.array_equal(g, x) for g, x in zip(got, tabs)), (table, first, count)
        finally:
            eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["renormalize", "renormalize_rows"])
def test_training_follows_renormalized_transr_weights(how):
    """ORDERED TransR trains on its committed copy of the matrices: after a
    renormalize of non-unit weights the next epoch equals that of a fresh context
    given the renormalised tables through kb2e_upload_params."""
    ds = tiny()
    n = 20

    def trainer():
        eng = Engine("R", n, ds.num_entities, ds.num_relations, rate=0.01, batches=10, seed=7)
        eng.upload_triples(ds.train)
        e0, r0, _ = eng.init_params()
        eng.transr_seed(e0, r0)
        return eng

    a, b = trainer(), trainer()
    try:
        ent, rel, w = a.download_params()
        rng = np.random.default_rng(11)
        w = w * rng.uniform(1.5, 3.0, (w.shape[0], n, 1))  # rows 1.5 .. 3 times too long
        a.upload_params(ent, rel, w)
        if how == "renormalize":
            a.renormalize()
        else:
            a.renormalize_rows(2, 0, ds.num_relations)
        fixed = a.download_params()
        exp = mm.expected_renorm("R", 2, w)
        assert np.abs(fixed[2] - exp).max() <= 1e-12 and not np.array_equal(fixed[2], w)
        b.upload_params(*fixed)
        la, aa = a.train_epoch()
        lb, ab = b.train_epoch()
        assert aa == ab and aa > 0
        assert abs(la - lb) <= 1e-12 * max(1.0, abs(lb)), (la, lb)
        ta, tb = a.download_params(), b.download_params()
        worst = max(float(np.abs(x - y).max()) for x, y in zip(ta, tb))
        worst = max(worst, max(float(np.abs(x - y).max()) for x, y in zip(a.transr_work(), b.transr_work())))
        print(f"{how}: max |renormalised context - fresh context| after an epoch {worst:.3e}")
        assert worst <= 1e-12
    finally:
        a.close()
        b.close()
