"""Relation fold-in on the device (kb2e_fold_in_relations,
kb2e_amd/csrc/foldrel.hip) against its numpy FP64 restatement
(tests/fold_rel_model.py).

The committed inputs keep every decision of the model (hinge, L1 sign, norm
test, loop test) at least 1e-7 from its threshold (tests/test_fold_rel_model.py
checks that on the CPU), a workgroup sum moves an energy by ~1e-13, so the
device must take the same decisions: counts are equal, losses agree to rtol
1e-9, and rows to gpu_common.F64_ATOL where no loop against an entity row
iterates and F64_ATOL_COUPLED where one does -- the project's constants for
exactly this difference in sum order.
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import fold_in_model as fm
import fold_rel_model as frm
from conftest import GOLDEN, ROOT
from gpu_common import F64_ATOL, F64_ATOL_COUPLED, MANIFEST, tiny
from kb2e_amd import data, linkpred
from kb2e_amd.engine import Engine, EngineError, lib

pytestmark = pytest.mark.gpu

LOSS_RTOL = 1e-9


def make_engine(model, ent, rel, w, *, lr, margin, l1, precision=64, **kw):
    eng = Engine(model, ent.shape[1], ent.shape[0], rel.shape[0], rate=lr, margin=margin, distance=0 if l1 else 1,
                 precision=precision, transr_compat=False, **kw)
    eng.upload_params(ent, rel, w)
    return eng


def run_engine(inputs, precision=64, eng=None, **over):
    """Engine.fold_in_relations on a model input tuple (on `eng`, after uploading the tables again, or on an
    engine of its own); returns (rel rows, w rows, loss, counts, tables after)."""
    model, ent, rel, w, free, ex, known, kw = inputs
    kw = {**kw, **over}
    own = eng is None
    if own:
        eng = make_engine(model, ent, rel, w, lr=kw["lr"], margin=kw["margin"], l1=kw["l1"], precision=precision)
    else:
        eng.upload_params(ent, rel, w)
    try:
        rows, wrows, loss, counts = eng.fold_in_relations(
            free, ex, known, epochs=kw["epochs"], batch_size=kw["batch_size"], seed=kw["seed"], side=kw["side"],
            max_sweeps=kw.get("max_sweeps", 0), rel=kw.get("rel_in"), w=kw.get("w_in"))
        tables = eng.download_params()
    finally:
        if own:
            eng.close()
    return rows, wrows, loss, counts, tables


def case_inputs(c, batch_size=1):
    ent, rel, w, free, ex, known = frm.random_case(c)
    return (c.model, ent, rel, w, free, ex, known,
            dict(lr=c.lr, margin=c.margin, l1=c.l1, epochs=c.epochs, seed=c.seed, side=c.side, batch_size=batch_size))


def assert_parity(got, want, inputs):
    rows, wrows, loss, counts, tables = got
    atol = F64_ATOL_COUPLED if want.sweeps else F64_ATOL
    diff = float(np.max(np.abs(rows - want.rel)))
    wdiff = 0.0 if want.w is None else float(np.max(np.abs(wrows - want.w)))
    print(f"rel max |diff| {diff:.3e}, w max |diff| {wdiff:.3e} (atol {atol:g}), loops {len(want.sweeps)}, "
          f"counts {want.counts.sum(0).tolist()}")
    assert np.array_equal(counts, want.counts)
    np.testing.assert_allclose(loss, want.loss, rtol=LOSS_RTOL, atol=0)
    assert diff <= atol and wdiff <= atol
    assert (wrows is None) == (want.w is None)
    # the tables hold the returned rows, and nothing else moved
    ent, rel, w, free = inputs[1], inputs[2], inputs[3], np.asarray(inputs[4])
    frozen = np.setdiff1d(np.arange(len(rel)), free)
    assert np.array_equal(tables[0], ent)
    assert np.array_equal(tables[1][free], rows) and np.array_equal(tables[1][frozen], rel[frozen])
    if w is not None:
        assert np.array_equal(tables[2][free], wrows) and np.array_equal(tables[2][frozen], w[frozen])


def parity_over_batches(c, batches):
    inputs = case_inputs(c)
    kw = inputs[7]
    eng = make_engine(c.model, *inputs[1:4], lr=kw["lr"], margin=kw["margin"], l1=kw["l1"])
    try:
        for b in batches:
            want = frm.run_case(c, b)
            if c in frm.CASES:
                assert frm.case_ok(c, want)
            assert_parity(run_engine(inputs, eng=eng, batch_size=b), want, inputs)
    finally:
        eng.close()


@pytest.mark.parametrize("c", frm.CASES, ids=lambda c: c.id)
def test_parity_with_the_model(c):
    # one sample a batch; a ragged last batch; uneven over the four waves; more than any relation has
    assert frm.BATCHES == (1, 3, 7, 64) and frm.PER_FREE == 9
    parity_over_batches(c, frm.BATCHES)


@pytest.mark.parametrize("c", frm.BOUNDARY, ids=lambda c: c.id)
def test_lane_boundaries(c):
    parity_over_batches(c, (1, 5))


def lds_limit():
    eng = Engine("R", 8, 4, 2)
    try:
        return eng.counter("foldrel_lds_limit")
    finally:
        eng.close()


@pytest.mark.parametrize("c", frm.STAGING, ids=lambda c: c.id)
def test_transr_matrix_on_each_side_of_the_lds_limit(c):
    assert lds_limit() == frm.LDS_LIMIT and [s.dim for s in frm.STAGING] == [frm.LDS_LIMIT, frm.LDS_LIMIT + 1]
    parity_over_batches(c, (5,))


def test_transr_matrix_in_global_memory(monkeypatch):
    monkeypatch.setenv("KB2E_FOLDREL_W_L2", "1")
    c = next(c for c in frm.CASES if c.model == "R" and c.dim == 20 and c.side == 2 and c.l1)
    parity_over_batches(c, (1, 7))


def test_long_batches_a_long_relation_and_one_without_examples():
    inputs, want = frm.long_batch()
    per = np.bincount(inputs[5][:, 2], minlength=5)[inputs[4]].tolist()
    assert per == [2000, 310, 0] and inputs[7]["batch_size"] == 300  # 300 records of 48 doubles: past the LDS staging
    got = run_engine(inputs)
    assert_parity(got, want, inputs)
    assert np.array_equal(got[0][2], inputs[2][inputs[4][2]]) and not got[2][2].any() and not got[3][2].any()


def test_many_relations():
    inputs, want = frm.many()
    assert len(inputs[4]) == 70
    assert_parity(run_engine(inputs), want, inputs)


def test_no_dependence_on_unit_order_or_grid(monkeypatch):
    c = next(c for c in frm.CASES if c.model == "R" and c.dim == 20 and c.side == 2 and c.l1)
    inputs = case_inputs(c, 3)
    rows, wrows = run_engine(inputs)[:2]
    perm = np.array([2, 0, 1])
    shuffled = list(inputs)
    shuffled[4] = np.asarray(inputs[4])[perm]
    got = run_engine(tuple(shuffled))
    assert np.array_equal(got[0], rows[perm]) and np.array_equal(got[1], wrows[perm])
    many, _ = frm.many()
    base = run_engine(many)
    for grid in ("1", "3"):
        monkeypatch.setenv("KB2E_FOLDREL_GRID", grid)
        got = run_engine(inputs)
        assert np.array_equal(got[0], rows) and np.array_equal(got[1], wrows)
        got = run_engine(many)  # 70 units over one and over three workgroups
        assert all(np.array_equal(x, y) for x, y in zip(got[:4], base[:4]))


@pytest.mark.parametrize("model", ["E", "H", "R"])
def test_fp32_tables(model):
    c = next(c for c in frm.CASES if c.model == model and c.dim == 20 and c.side == 2 and c.l1)
    m, ent, rel, w, free, ex, known, kw = case_inputs(c, 3)
    wide = [None if a is None else a.astype(np.float32).astype(np.float64) for a in (ent, rel, w)]
    want = frm.fold_in_relations(m, *wide, free, ex, known, **kw, precision=32)
    assert want.guards() >= fm.GUARD
    rows, wrows, loss, counts, tables = run_engine((m, ent, rel, w, free, ex, known, kw), precision=32)
    assert np.array_equal(counts, want.counts)
    np.testing.assert_allclose(loss, want.loss, rtol=LOSS_RTOL, atol=0)
    for got, ref in ((rows, want.rel),) + (() if w is None else ((wrows, want.w),)):
        assert np.array_equal(got, got.astype(np.float32).astype(np.float64))  # rounded once, at the store
        ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
        assert np.all(np.abs(got - ref) <= ulp)
    assert np.array_equal(tables[1][free], rows) and np.array_equal(tables[0], wide[0])


def test_known_set_that_leaves_one_candidate():
    inputs, want = frm.one_candidate()
    assert want.counts[:, 1].sum() >= 1 and want.counts[:, 0].sum() >= 1
    assert_parity(run_engine(inputs), want, inputs)


def test_complete_graph_fails_every_sample():
    inputs, want = frm.complete_graph()
    rows, wrows, loss, counts, tables = run_engine(inputs)
    nex = np.array([2, 4])
    assert np.array_equal(counts, np.stack([0 * nex, nex * inputs[7]["epochs"], 0 * nex], axis=1))
    assert np.array_equal(counts, want.counts) and not loss.any()
    assert np.array_equal(rows, inputs[2][inputs[4]]) and np.array_equal(tables[1], inputs[2])


@pytest.mark.parametrize("model", ["H", "R"])
def test_sweep_cap(model):
    c = next(c for c in frm.CASES if c.model == model and c.dim == 8 and c.side == 2 and c.l1)
    inputs = case_inputs(c, 3)
    want = frm.run_case(c, 3, max_sweeps=2)
    assert want.counts[:, 2].sum() >= 1 and want.guards() >= fm.GUARD
    assert_parity(run_engine(inputs, max_sweeps=2), want, inputs)


@pytest.mark.parametrize("model", ["E", "H", "R"])
def test_start_rows_are_honoured(model):
    c = next(c for c in frm.CASES if c.model == model and c.dim == 8 and c.side == 2 and c.l1)
    m, ent, rel, w, free, ex, known, kw = case_inputs(c, 3)
    rng = np.random.default_rng(3)
    rel_in = rng.normal(size=(len(free), c.dim)) * 0.2
    w_in = None
    if model == "H":
        w_in = rng.normal(size=(len(free), c.dim))
        w_in /= np.linalg.norm(w_in, axis=1, keepdims=True)
    elif model == "R":
        w_in = np.stack([np.eye(c.dim)] * len(free)) * 0.9 + rng.normal(size=(len(free), c.dim, c.dim)) * 0.1
    ex = ex[ex[:, 2] != free[1]]  # free[1] has no example left
    want = frm.fold_in_relations(m, ent, rel, w, free, ex, known, **kw, rel_in=rel_in, w_in=w_in)
    assert want.guards() >= fm.GUARD and want.counts[:, 0].sum() >= 1
    inputs = (m, ent, rel, w, free, ex, known, kw)
    got = run_engine(inputs, rel_in=rel_in, w_in=w_in)
    assert_parity(got, want, inputs)
    assert np.array_equal(got[0][1], rel_in[1]) and not got[2][1].any() and not got[3][1].any()
    if w_in is not None:
        assert np.array_equal(got[1][1], w_in[1])
    # no examples at all: every row is the start row
    got = run_engine((m, ent, rel, w, free, np.zeros((0, 3), np.int32), None, kw), rel_in=rel_in, w_in=w_in)
    assert np.array_equal(got[0], rel_in) and not got[2].any() and not got[3].any()
    assert w_in is None or np.array_equal(got[1], w_in)


@pytest.mark.parametrize("model", ["E", "H", "R"])
def test_everything_else_is_frozen_and_training_continues(model):
    ds = tiny()
    n = 8

    def fresh():
        eng = Engine(model, n, ds.num_entities, ds.num_relations, rate=0.01, batches=30, seed=3, transr_compat=True)
        eng.upload_triples(ds.train)
        ent, rel, _ = eng.init_params()
        if model == "R":
            eng.transr_seed(ent, rel)
        return eng

    free = np.array([ds.num_relations - 1, 0], np.int32)
    ex = ds.train[np.isin(ds.train[:, 2], free)][:40]
    assert len(ex) >= 4 and set(ex[:, 2].tolist()) == set(free.tolist())
    a, b = fresh(), fresh()
    try:
        a.train_batches(2)
        b.train_batches(2)
        a.synchronize()
        before = a.download_params()
        work, nbytes = a.transr_work() if model == "R" else None, a.device_bytes()
        a.profile(True)
        rows, wrows, loss, counts = a.fold_in_relations(free, ex, ds.train, epochs=3, batch_size=4, seed=1)
        ms, launches = a.profile_query("foldrel")
        assert launches == 1 and ms > 0
        a.profile(False)
        after = a.download_params()
        frozen = np.setdiff1d(np.arange(ds.num_relations), free)
        assert np.array_equal(after[0], before[0])                                   # the entity table
        assert np.array_equal(after[1][frozen], before[1][frozen]) and np.array_equal(after[1][free], rows)
        assert counts[:, 0].sum() >= 1 and not np.array_equal(after[1][free], before[1][free])
        if model != "E":
            assert np.array_equal(after[2][frozen], before[2][frozen]) and np.array_equal(after[2][free], wrows)
        assert a.device_bytes() == nbytes
        if model == "R":
            assert all(np.array_equal(x, y) for x, y in zip(a.transr_work(), work))
        # training goes on as from the same tables in a context that never folded anything in
        b.synchronize()
        b.upload_params(*after)
        a.train_batches(3)
        b.train_batches(3)
        a.synchronize()
        b.synchronize()
        assert all(x is y or np.array_equal(x, y) for x, y in zip(a.download_params(), b.download_params()))
        assert a.rng_next() == b.rng_next()
    finally:
        a.close()
        b.close()


def test_invalid_arguments():
    c = next(c for c in frm.CASES if c.model == "H")
    m, ent, rel, w, free, ex, known, kw = case_inputs(c)
    eng = make_engine(m, ent, rel, w, lr=kw["lr"], margin=kw["margin"], l1=kw["l1"])
    ne, nr = ent.shape[0], rel.shape[0]

    def bad(free_=free, ex_=ex, known_=known, **over):
        args = dict(epochs=1, batch_size=1, seed=0, side=2, max_sweeps=0)
        args.update(over)
        with pytest.raises(EngineError, match="EINVAL"):
            eng.fold_in_relations(free_, ex_, known_, **args)

    def edited(a, row, col, value):
        a = np.array(a)
        a[row, col] = value
        return a

    try:
        before = eng.download_params()
        bad(free_=np.zeros(0, np.int32), ex_=np.zeros((0, 3), np.int32))          # nfree < 1
        bad(epochs=0)
        bad(batch_size=0)
        bad(side=3)
        bad(side=-1)
        bad(max_sweeps=-1)
        for v in (-1, ne):                                                          # ids out of range
            bad(ex_=edited(ex, 0, 0, v))
            bad(ex_=edited(ex, 0, 1, v))
            bad(known_=edited(known, 0, 0, v))
            bad(known_=edited(known, 0, 1, v))
        for v in (-1, nr):
            bad(free_=np.array([free[0], v], np.int32), ex_=ex[ex[:, 2] == free[0]])
            bad(ex_=edited(ex, 0, 2, v))
            bad(known_=edited(known, 0, 2, v))
        bad(free_=np.array([free[0], free[1], free[2], free[0]], np.int32))         # a free relation listed twice
        bad(ex_=edited(ex, 0, 2, 0))                                                # an example whose relation is not free
        # NULL arrays with a count > 0 (not reachable through Engine.fold_in_relations)
        f = np.ascontiguousarray(free, np.int32)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        col = np.ascontiguousarray(ex[:, 2], np.int32)
        loss, counts = np.zeros((len(f), 2)), np.zeros((len(f), 3), np.int64)
        out = (loss.ctypes.data_as(C.POINTER(C.c_double)), counts.ctypes.data_as(C.POINTER(C.c_int64)))
        call = lib().kb2e_fold_in_relations
        assert call(eng.h, ip(f), len(f), None, ip(col), ip(col), len(ex), None, None, None, 0, 1, 1, 0, 2, 0, None, None,
                    None, None, *out) == 1
        assert call(eng.h, ip(f), len(f), None, None, None, 0, ip(col), None, ip(col), 4, 1, 1, 0, 2, 0, None, None, None,
                    None, *out) == 1
        assert call(eng.h, None, len(f), None, None, None, 0, None, None, None, 0, 1, 1, 0, 2, 0, None, None, None, None,
                    *out) == 1
        assert all(np.array_equal(x, y) for x, y in zip(eng.download_params(), before))  # a refused call changes nothing
    finally:
        eng.close()
    # w_in / w_out given for TransE
    te = next(c for c in frm.CASES if c.model == "E")
    m, ent, rel, w, free, ex, known, kw = case_inputs(te)
    eng = make_engine(m, ent, rel, None, lr=kw["lr"], margin=kw["margin"], l1=kw["l1"])
    try:
        with pytest.raises(EngineError, match="EINVAL"):
            eng.fold_in_relations(free, ex, known, epochs=1, w=np.zeros((len(free), te.dim)))
        f = np.ascontiguousarray(free, np.int32)
        loss, counts, wout = np.zeros((len(f), 2)), np.zeros((len(f), 3), np.int64), np.zeros((len(f), te.dim))
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        assert lib().kb2e_fold_in_relations(eng.h, f.ctypes.data_as(C.POINTER(C.c_int32)), len(f), None, None, None, 0,
                                            None, None, None, 0, 1, 1, 0, 2, 0, None, None, None, dp(wout), dp(loss),
                                            counts.ctypes.data_as(C.POINTER(C.c_int64))) == 1
    finally:
        eng.close()
    empty = Engine("E", 8, ne, nr)
    try:
        with pytest.raises(EngineError, match="ESTATE"):
            empty.fold_in_relations(free, ex, known, epochs=1)
    finally:
        empty.close()


# ------------------------------------------------------------------ end to end

def test_end_to_end_fold_in_improves_held_out_ranks():
    # Two of the six relations are held out with their ~1,000 triples each way.  An L1 step moves every coordinate
    # of r by lr, so at the synthetic tests' usual lr = 0.01 a relation with 500 examples is through its descent
    # inside the first pass and first and last loss differ by the noise of the negatives alone; lr = 0.002 (and
    # 200 epochs of training at that rate) leaves a descent to see.  A metric assertion, not parity.
    ds = data.synthetic(counts=(300, 6, 6000, 300, 300), planted=True)
    res = linkpred.fold_in_relations_evaluation(ds, "E", 20, [0, 3], support=0.5, epochs=200, fold_epochs=30,
                                                batch_size=4, rate=0.002, batches=10, seed=7)
    print({k: v for k, v in res.items() if k not in ("rel_rows", "w_rows")})
    assert res["held_out"] == 2 and res["query"] >= 30
    assert res["rank_after"] < res["rank_before"]
    assert res["loss_last"] < res["loss_first"]


# ------------------------------------------------------------------ command line

def test_foldrel_cli_matches_engine(tmp_path):
    run = MANIFEST["runs"]["transe_l1_bern"]
    flags = run["flags"]
    n, method = flags["size"], "bern"
    src, gold = os.path.join(GOLDEN, "tiny"), os.path.join(GOLDEN, "transe_l1_bern")
    ds = tiny()
    nr_old = ds.num_relations - 2
    new = np.arange(nr_old, ds.num_relations)
    # the data directory: the id files as they are, the splits without the new relations; FILE: the training
    # triples of the new relations
    names = {int(line.split()[1]): line.split()[0] for line in open(os.path.join(src, "entity2id.txt"))}
    rnames = {int(line.split()[1]): line.split()[0] for line in open(os.path.join(src, "relation2id.txt"))}
    ddir, odir, fdir = tmp_path / "data", tmp_path / "out", tmp_path / "fold"
    for d in (ddir, odir, fdir):
        d.mkdir()
    for f in ("entity2id.txt", "relation2id.txt"):
        shutil.copy(os.path.join(src, f), ddir / f)
    splits = {}
    for split in ("train", "valid", "test"):
        t = getattr(ds, split)
        splits[split] = t[~np.isin(t[:, 2], new)]
        with open(ddir / f"{split}.txt", "w") as out:
            for h, tl, r in splits[split].tolist():
                out.write(f"{names[h]}\t{names[tl]}\t{rnames[r]}\n")
    ex = ds.train[np.isin(ds.train[:, 2], new)]
    assert len(ex) >= 5
    with open(tmp_path / "new.txt", "w") as out:
        for h, tl, r in ex.tolist():
            out.write(f"{names[h]}\t{names[tl]}\t{rnames[r]}\n")
    shutil.copy(os.path.join(gold, f"entity2vec.{method}"), odir / f"entity2vec.{method}")
    old_lines = open(os.path.join(gold, f"relation2vec.{method}"), "rb").read().splitlines(keepends=True)[:nr_old]
    open(odir / f"relation2vec.{method}", "wb").write(b"".join(old_lines))

    exe = tmp_path / "foldrelTransE"
    exe.symlink_to(os.path.join(ROOT, "bin", "kb2e"))
    args = [str(exe), "--datadir", str(ddir), "--outdir", str(odir), "--new", str(tmp_path / "new.txt"), "--foldout",
            str(fdir), "--size", str(n), "--rate", str(flags["rate"]), "--margin", str(flags["margin"]), "--method",
            str(flags["method"]), "--distance", str(flags["distance"]), "--epochs", "3", "--seed", "5", "--batch", "4"]
    res = subprocess.run(args, capture_output=True, text=True, timeout=300, check=True)
    passes = [l for l in res.stdout.splitlines() if l.startswith("Pass: ")]
    assert [l.split(",")[0] for l in passes] == ["Pass: 0", "Pass: 1", "Pass: 2"]

    eng = Engine("E", n, ds.num_entities, ds.num_relations, rate=flags["rate"], margin=flags["margin"],
                 method=flags["method"], distance=flags["distance"], seed=5)
    try:
        _, rel, _ = eng.init_params()
        ent = data.read_table(str(odir / f"entity2vec.{method}"), ds.num_entities, n)
        rel[:nr_old] = data.read_table(str(odir / f"relation2vec.{method}"), nr_old, n)
        eng.upload_params(ent, rel)
        known = np.concatenate([ex, splits["train"], splits["valid"], splits["test"]])
        losses = []
        for p in range(3):
            rows, _, loss, _ = eng.fold_in_relations(new, ex, known, epochs=1, batch_size=4, seed=5 + p)
            losses.append(loss[:, 0].sum())
    finally:
        eng.close()
    got = open(fdir / f"relation2vec.{method}", "rb").read().splitlines(keepends=True)
    assert len(got) == ds.num_relations and got[:nr_old] == old_lines
    want = ["".join("%.6f\t" % v for v in row) + "\n" for row in rows]
    assert [l.decode() for l in got[nr_old:]] == want
    assert [float(l.split("Loss: ")[1]) for l in passes] == [float("%f" % v) for v in losses]
