"""Entity fold-in on the device (kb2e_fold_in_entities, kb2e_amd/csrc/foldin.hip)
against its numpy FP64 restatement (tests/fold_in_model.py).

The committed inputs keep every decision of the model (hinge, L1 sign, loop
test) at least 1e-7 from its threshold (tests/test_fold_in_model.py checks that
on the CPU), a wave sum moves an energy by ~1e-13, so the device must take the
same decisions: counts are equal, losses agree to rtol 1e-9, and rows to
gpu_common.F64_ATOL where no coupling loop iterates and F64_ATOL_COUPLED where
one does -- the project's constants for exactly this difference in sum order.
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import fold_in_model as fm
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


def run_engine(inputs, precision=64, **over):
    """Engine.fold_in on a model input tuple; returns (rows, loss, counts, entity table after)."""
    model, ent, rel, w, free, ex, known, kw = inputs
    kw = {**kw, **over}
    eng = make_engine(model, ent, rel, w, lr=kw["lr"], margin=kw["margin"], l1=kw["l1"], precision=precision)
    try:
        rows, loss, counts = eng.fold_in(free, ex, known, epochs=kw["epochs"], seed=kw["seed"], side=kw["side"],
                                         max_sweeps=kw.get("max_sweeps", 0))
        table = eng.download_params()[0]
    finally:
        eng.close()
    return rows, loss, counts, table


def case_inputs(c):
    ent, rel, w, free, ex, known = fm.random_case(c)
    return (c.model, ent, rel, w, free, ex, known,
            dict(lr=c.lr, margin=c.margin, l1=c.l1, epochs=c.epochs, seed=c.seed, side=c.side))


def assert_parity(got, want, inputs):
    rows, loss, counts, table = got
    atol = F64_ATOL_COUPLED if want.sweeps else F64_ATOL
    diff = float(np.max(np.abs(rows - want.rows)))
    print(f"rows max |diff| {diff:.3e} (atol {atol:g}), loops {len(want.sweeps)}, counts {want.counts.sum(0).tolist()}")
    assert np.array_equal(counts, want.counts)
    np.testing.assert_allclose(loss, want.loss, rtol=LOSS_RTOL, atol=0)
    assert diff <= atol
    # the table holds the returned rows, and nothing else moved
    ent, free = inputs[1], np.asarray(inputs[4])
    assert np.array_equal(table[free], rows)
    frozen = np.setdiff1d(np.arange(len(ent)), free)
    assert np.array_equal(table[frozen], ent[frozen])


@pytest.mark.parametrize("c", fm.CASES, ids=lambda c: c.id)
def test_parity_with_the_model(c):
    inputs = case_inputs(c)
    want = fm.run_case(c)
    assert fm.case_ok(c, want)
    assert_parity(run_engine(inputs), want, inputs)


@pytest.mark.parametrize("c", fm.BOUNDARY, ids=lambda c: c.id)
def test_lane_and_staging_boundaries(c):
    inputs = case_inputs(c)
    assert_parity(run_engine(inputs), fm.run_case(c), inputs)


@pytest.mark.parametrize("c", fm.BOUNDARY_L2, ids=lambda c: c.id)
def test_transr_matrix_from_l2(c, monkeypatch):
    if c.dim <= 141:
        monkeypatch.setenv("KB2E_FOLD_W_L2", "1")  # (n = 150 takes the L2 form by itself)
    inputs = case_inputs(c)
    assert_parity(run_engine(inputs), fm.run_case(c), inputs)


def test_one_hub():
    inputs, want = fm.hub()
    assert want.counts[0, 0] > 3000 and want.guards() >= fm.GUARD
    assert_parity(run_engine(inputs), want, inputs)


def test_many_units():
    inputs, want = fm.many()
    assert len(inputs[4]) == 2000 and want.guards() >= fm.GUARD
    assert_parity(run_engine(inputs), want, inputs)


def test_no_dependence_on_unit_order_or_grid(monkeypatch):
    c = next(c for c in fm.CASES if c.model == "R" and c.dim == 20 and c.side == 2 and c.l1)
    inputs = case_inputs(c)
    rows = run_engine(inputs)[0]
    perm = np.array([3, 0, 4, 2, 1])
    shuffled = list(inputs)
    shuffled[4] = np.asarray(inputs[4])[perm]
    assert np.array_equal(run_engine(tuple(shuffled))[0], rows[perm])
    monkeypatch.setenv("KB2E_FOLD_GRID", "2")  # two workgroups walk the five units
    assert np.array_equal(run_engine(inputs)[0], rows)


@pytest.mark.parametrize("model", ["E", "R"])
def test_fp32_tables(model):
    c = next(c for c in fm.CASES if c.model == model and c.dim == 20 and c.side == 2 and c.l1)
    m, ent, rel, w, free, ex, known, kw = case_inputs(c)
    wide = [None if a is None else a.astype(np.float32).astype(np.float64) for a in (ent, rel, w)]
    want = fm.fold_in(m, *wide, free, ex, known, **kw, precision=32)
    assert want.guards() >= fm.GUARD
    rows, loss, counts, table = run_engine((m, ent, rel, w, free, ex, known, kw), precision=32)
    assert np.array_equal(counts, want.counts)
    np.testing.assert_allclose(loss, want.loss, rtol=LOSS_RTOL, atol=0)
    assert np.array_equal(rows, rows.astype(np.float32).astype(np.float64))  # rounded once, at the store
    ulp = np.spacing(np.abs(want.rows).astype(np.float32)).astype(np.float64)
    assert np.all(np.abs(rows - want.rows) <= ulp)
    assert np.array_equal(table[free], rows)


def test_known_set_that_leaves_one_candidate():
    inputs, want = fm.one_candidate()
    assert want.counts[:, 1].sum() >= 1 and want.counts[:, 0].sum() >= 1
    assert_parity(run_engine(inputs), want, inputs)


def test_complete_graph_fails_every_sample():
    inputs, want = fm.complete_graph()
    rows, loss, counts, table = run_engine(inputs)
    nex = np.array([3, 3])
    assert np.array_equal(counts, np.stack([0 * nex, nex * inputs[7]["epochs"], 0 * nex], axis=1))
    assert np.array_equal(counts, want.counts) and not loss.any()
    assert np.array_equal(rows, inputs[1][inputs[4]]) and np.array_equal(table, inputs[1])


def test_sweep_cap():
    c = next(c for c in fm.CASES if c.model == "H" and c.dim == 8 and c.side == 2)
    inputs = case_inputs(c)
    want = fm.run_case(c, max_sweeps=5)
    assert want.counts[:, 2].sum() >= 1
    assert_parity(run_engine(inputs, max_sweeps=5), want, inputs)


def test_rows_in_and_entities_without_examples():
    c = next(c for c in fm.CASES if c.model == "E" and c.dim == 8 and c.side == 2 and c.l1)
    m, ent, rel, w, free, ex, known, kw = case_inputs(c)
    rng = np.random.default_rng(3)
    start = rng.normal(size=(len(free), c.dim)) * 0.3
    ex = ex[(ex[:, 0] != free[1]) & (ex[:, 1] != free[1])]  # free[1] has no example left
    want = fm.fold_in(m, ent, rel, w, free, ex, known, **kw, rows=start)
    assert want.guards() >= fm.GUARD
    eng = make_engine(m, ent, rel, w, lr=kw["lr"], margin=kw["margin"], l1=kw["l1"])
    try:
        rows, loss, counts = eng.fold_in(free, ex, known, epochs=kw["epochs"], seed=kw["seed"], side=kw["side"],
                                         rows=start)
        assert np.array_equal(counts, want.counts) and np.max(np.abs(rows - want.rows)) <= F64_ATOL
        assert np.array_equal(rows[1], start[1]) and not loss[1].any() and not counts[1].any()
        # no examples at all: every row is rows_in's
        rows, loss, counts = eng.fold_in(free, np.zeros((0, 3), np.int32), None, epochs=2, rows=start)
        assert np.array_equal(rows, start) and not loss.any() and not counts.any()
    finally:
        eng.close()


@pytest.mark.parametrize("model", ["H", "R"])
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

    free = np.array([7, 150, 42], np.int32)
    ex = np.array([(7, 1, 0), (2, 7, 1), (150, 3, 2), (9, 150, 0), (42, 11, 1), (12, 42, 3)], np.int32)
    ex[:, 2] %= ds.num_relations
    a, b = fresh(), fresh()
    try:
        a.train_batches(2)
        b.train_batches(2)
        a.synchronize()
        before = a.download_params()
        work, nbytes = a.transr_work() if model == "R" else None, a.device_bytes()
        a.profile(True)
        rows, loss, counts = a.fold_in(free, ex, ds.train, epochs=3, seed=1)
        ms, launches = a.profile_query("foldin")
        assert launches == 1 and ms > 0
        a.profile(False)
        after = a.download_params()
        frozen = np.setdiff1d(np.arange(ds.num_entities), free)
        assert np.array_equal(after[0][frozen], before[0][frozen]) and np.array_equal(after[0][free], rows)
        assert counts[:, 0].sum() >= 1 and not np.array_equal(after[0][free], before[0][free])
        assert np.array_equal(after[1], before[1]) and np.array_equal(after[2], before[2])
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
        assert all(np.array_equal(x, y) for x, y in zip(a.download_params(), b.download_params()))
        assert a.rng_next() == b.rng_next()
    finally:
        a.close()
        b.close()


def test_invalid_arguments():
    c = fm.CASES[0]
    m, ent, rel, w, free, ex, known, kw = case_inputs(c)
    eng = make_engine(m, ent, rel, w, lr=kw["lr"], margin=kw["margin"], l1=kw["l1"])
    ne, nr = ent.shape[0], rel.shape[0]
    frozen = 0

    def bad(free_=free, ex_=ex, known_=known, **over):
        args = dict(epochs=1, seed=0, side=2, max_sweeps=0)
        args.update(over)
        with pytest.raises(EngineError, match="EINVAL"):
            eng.fold_in(free_, ex_, known_, **args)

    def edited(a, row, col, value):
        a = np.array(a)
        a[row, col] = value
        return a

    try:
        before = eng.download_params()[0]
        bad(free_=np.zeros(0, np.int32), ex_=np.zeros((0, 3), np.int32))          # nfree < 1
        bad(epochs=0)
        bad(side=3)
        bad(side=-1)
        bad(max_sweeps=-1)
        for v in (-1, ne):                                                          # ids out of range
            bad(free_=np.array([free[0], v], np.int32), ex_=ex[(ex[:, 0] == free[0]) | (ex[:, 1] == free[0])])
            bad(known_=edited(known, 0, 0, v))
            bad(known_=edited(known, 0, 1, v))
            own = 0 if ex[0, 0] in free else 1
            bad(ex_=edited(ex, 0, 1 - own, v))
        for v in (-1, nr):
            bad(ex_=edited(ex, 0, 2, v))
            bad(known_=edited(known, 0, 2, v))
        bad(free_=np.array([free[0], free[1], free[0]], np.int32))                  # a free id listed twice
        bad(ex_=edited(edited(ex, 0, 0, frozen), 0, 1, frozen + 1))                 # no free entity
        bad(ex_=edited(edited(ex, 0, 0, free[0]), 0, 1, free[0]))                   # the same one in both slots
        bad(ex_=edited(edited(ex, 0, 0, free[0]), 0, 1, free[1]))                   # two different ones
        # NULL arrays with a count > 0 (not reachable through Engine.fold_in)
        f = np.ascontiguousarray(free, np.int32)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        col = np.ascontiguousarray(ex[:, 0], np.int32)
        loss, counts = np.zeros((len(f), 2)), np.zeros((len(f), 3), np.int64)
        out = (loss.ctypes.data_as(C.POINTER(C.c_double)), counts.ctypes.data_as(C.POINTER(C.c_int64)))
        assert lib().kb2e_fold_in_entities(eng.h, ip(f), len(f), None, ip(col), ip(col), len(ex), None, None, None, 0, 1,
                                           0, 2, 0, None, None, *out) == 1
        assert lib().kb2e_fold_in_entities(eng.h, ip(f), len(f), None, None, None, 0, ip(col), None, ip(col), 4, 1, 0, 2,
                                           0, None, None, *out) == 1
        assert lib().kb2e_fold_in_entities(eng.h, None, len(f), None, None, None, 0, None, None, None, 0, 1, 0, 2, 0,
                                           None, None, *out) == 1
        assert np.array_equal(eng.download_params()[0], before)  # a refused call changes nothing
    finally:
        eng.close()
    empty = Engine("E", 8, ne, nr)
    try:
        with pytest.raises(EngineError, match="ESTATE"):
            empty.fold_in(free, ex, known, epochs=1)
    finally:
        empty.close()


# ------------------------------------------------------------------ end to end

def held_out_entities(ds, count=30):
    """Entities of middling degree (the hubs stay: removing them would take most of the training set away)."""
    deg = np.bincount(np.concatenate([ds.train[:, 0], ds.train[:, 1]]), minlength=ds.num_entities)
    order = np.argsort(-deg, kind="stable")
    return np.sort(order[20:20 + count]).astype(np.int32)


def test_end_to_end_fold_in_improves_held_out_ranks():
    ds = data.synthetic(counts=(300, 6, 6000, 300, 300), planted=True)
    res = linkpred.fold_in_evaluation(ds, "E", 20, held_out_entities(ds), support=0.5, epochs=30, fold_epochs=30,
                                      rate=0.01, batches=10, seed=7)
    print({k: v for k, v in res.items() if k != "rows"})
    assert res["held_out"] == 30 and res["query"] >= 30
    assert res["rank_after"] < res["rank_before"]
    assert res["loss_last"] < res["loss_first"]


# ------------------------------------------------------------------ command line

def test_foldin_cli_matches_engine(tmp_path):
    run = MANIFEST["runs"]["transe_l1_bern"]
    flags = run["flags"]
    n, method = flags["size"], "bern"
    src, gold = os.path.join(GOLDEN, "tiny"), os.path.join(GOLDEN, "transe_l1_bern")
    ds = tiny()
    ne_old = ds.num_entities - 5
    new = np.arange(ne_old, ds.num_entities)
    # the data directory: the id files as they are, the splits without the new entities; FILE: the training
    # triples that mention exactly one new entity
    names = {}
    for line in open(os.path.join(src, "entity2id.txt")):
        name, idx = line.split()
        names[int(idx)] = name
    rnames = {int(line.split()[1]): line.split()[0] for line in open(os.path.join(src, "relation2id.txt"))}
    ddir, odir, fdir = tmp_path / "data", tmp_path / "out", tmp_path / "fold"
    for d in (ddir, odir, fdir):
        d.mkdir()
    for f in ("entity2id.txt", "relation2id.txt"):
        shutil.copy(os.path.join(src, f), ddir / f)
    mentions = lambda t: np.isin(t[:, 0], new).astype(int) + np.isin(t[:, 1], new).astype(int)
    splits = {}
    for split in ("train", "valid", "test"):
        t = getattr(ds, split)
        splits[split] = t[mentions(t) == 0]
        with open(ddir / f"{split}.txt", "w") as out:
            for h, tl, r in splits[split].tolist():
                out.write(f"{names[h]}\t{names[tl]}\t{rnames[r]}\n")
    ex = ds.train[mentions(ds.train) == 1]
    assert len(ex) >= 5
    with open(tmp_path / "new.txt", "w") as out:
        for h, tl, r in ex.tolist():
            out.write(f"{names[h]}\t{names[tl]}\t{rnames[r]}\n")
    old_lines = open(os.path.join(gold, f"entity2vec.{method}"), "rb").read().splitlines(keepends=True)[:ne_old]
    open(odir / f"entity2vec.{method}", "wb").write(b"".join(old_lines))
    shutil.copy(os.path.join(gold, f"relation2vec.{method}"), odir / f"relation2vec.{method}")

    exe = tmp_path / "foldinTransE"
    exe.symlink_to(os.path.join(ROOT, "bin", "kb2e"))
    args = [str(exe), "--datadir", str(ddir), "--outdir", str(odir), "--new", str(tmp_path / "new.txt"), "--foldout",
            str(fdir), "--size", str(n), "--rate", str(flags["rate"]), "--margin", str(flags["margin"]), "--method",
            str(flags["method"]), "--distance", str(flags["distance"]), "--epochs", "3", "--seed", "5"]
    res = subprocess.run(args, capture_output=True, text=True, timeout=300, check=True)
    passes = [l for l in res.stdout.splitlines() if l.startswith("Pass: ")]
    assert [l.split(",")[0] for l in passes] == ["Pass: 0", "Pass: 1", "Pass: 2"]

    eng = Engine("E", n, ds.num_entities, ds.num_relations, rate=flags["rate"], margin=flags["margin"],
                 method=flags["method"], distance=flags["distance"], seed=5)
    try:
        ent, _, _ = eng.init_params()
        ent[:ne_old] = data.read_table(str(odir / f"entity2vec.{method}"), ne_old, n)
        rel = data.read_table(str(odir / f"relation2vec.{method}"), ds.num_relations, n)
        eng.upload_params(ent, rel)
        known = np.concatenate([ex, splits["train"], splits["valid"], splits["test"]])
        losses = []
        for p in range(3):
            rows, loss, _ = eng.fold_in(new, ex, known, epochs=1, seed=5 + p)
            losses.append(loss[:, 0].sum())
    finally:
        eng.close()
    got = open(fdir / f"entity2vec.{method}", "rb").read().splitlines(keepends=True)
    assert len(got) == ds.num_entities and got[:ne_old] == old_lines
    want = ["".join("%.6f\t" % v for v in row) + "\n" for row in rows]
    assert [l.decode() for l in got[ne_old:]] == want
    assert [float(l.split("Loss: ")[1]) for l in passes] == [float("%f" % v) for v in losses]
