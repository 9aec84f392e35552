"""Triple classification (kb2e_fit_thresholds, kb2e_classify_triples,
kb2e_corrupt_triples) against numpy brute force.

The fit's expected values are a brute force over ALL candidates (-inf and every
energy of the relation, correct(delta) counted from scratch for each), written
here; energies come from orc.Model(..., transr_compat=False).energy on the tiny
set and from Engine.score elsewhere (tests/test_gpu_predict.py pins that to the
oracle bit for bit).  The negatives' expected values are a numpy restatement of
the rule in include/kb2e_engine.h.  Every comparison is equality; the only
tolerance is where a printed %.6lf is parsed (the CLI test).
"""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from gpu_common import MANIFEST, tiny
from kb2e_amd import data, linkpred
from kb2e_amd.engine import Engine, EngineError
from oracle import orc

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1


# ------------------------------------------------------------------ helpers

def _tables(model, ds, n, seed, scale=0.3):
    """tests/test_gpu_relpred.py _tables' recipe."""
    rng = np.random.default_rng(seed)
    if model == "R":
        ent = rng.standard_normal((ds.num_entities, n))
        ent /= np.linalg.norm(ent, axis=1, keepdims=True)
        rel = rng.standard_normal((ds.num_relations, n)) * scale
        w = np.eye(n)[None] + rng.standard_normal((ds.num_relations, n, n)) * (scale / np.sqrt(n))
        return ent, rel, w
    ent = rng.standard_normal((ds.num_entities, n)) * 0.2
    rel = rng.standard_normal((ds.num_relations, n)) * 0.2
    w = None
    if model == "H":
        w = rng.standard_normal((ds.num_relations, n))
        w /= np.linalg.norm(w, axis=1, keepdims=True)
    return ent, rel, w


def _f32(tables):
    return tuple(None if t is None else t.astype(np.float32).astype(np.float64) for t in tables)


def _engine(model, n, ds, *, distance=0, precision=64, seed=0, **kw):
    tables = _tables(model, ds, n, seed)
    eng = Engine(model, n, ds.num_entities, ds.num_relations, distance=distance, precision=precision, **kw)
    eng.upload_params(*tables)
    return eng, tables


def _mix(z):
    z &= M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z


def np_corrupt(triples, known, ne, nr, seed=0, side=2, constrained=True):
    """include/kb2e_engine.h kb2e_corrupt_triples, restated.  Returns (negatives
    [count, 3], failed, stage2: rows that reached the all-entities stage)."""
    known = np.asarray(known, dtype=np.int64).reshape(-1, 3)
    kset = set(map(tuple, known.tolist()))
    pools = {}
    for r in range(nr):
        rows = known[known[:, 2] == r]
        pools[(r, 0)] = np.unique(rows[:, 0]).tolist()
        pools[(r, 1)] = np.unique(rows[:, 1]).tolist()
    state = _mix(seed)
    out = np.full((len(triples), 3), -1, np.int32)
    failed, stage2 = 0, 0
    for i, (h, t, r) in enumerate(np.asarray(triples).tolist()):
        u = lambda a: _mix(state + (i << 7) + a)  # noqa: E731
        slot = (u(0) >> 63) if side == 2 else side
        old = t if slot else h
        pool = pools[(r, slot)]
        got = -1
        first = 1 if constrained and pool else 33
        for a in range(first, 65):
            if a == 33:
                stage2 += 1
            x = pool[u(a) % len(pool)] if a <= 32 else u(a) % ne
            if x == old or ((h, x, r) if slot else (x, t, r)) in kset:
                continue
            got = x
            break
        out[i, 2] = r
        if got < 0:
            failed += 1
        else:
            out[i, 0], out[i, 1] = (h, got) if slot else (got, t)
    return out, failed, stage2


def labelled(positives, known, ne, nr, seed=0):
    """The positives followed by one restated negative each (failed ones dropped)."""
    neg, _, _ = np_corrupt(positives, known, ne, nr, seed=seed)
    neg = neg[neg[:, 0] >= 0]
    triples = np.concatenate([np.asarray(positives, dtype=np.int32), neg]).astype(np.int32)
    return triples, np.concatenate([np.ones(len(positives), np.uint8), np.zeros(len(neg), np.uint8)])


def _brute_one(e, lab):
    """(delta, correct): every candidate (-inf and each energy), correct counted
    from scratch; the smallest delta among the maxima."""
    cands = np.concatenate([[-np.inf], np.unique(e)])  # ascending
    pos, neg = lab == 1, lab == 0
    best_c, best_d = -1, None
    for c0 in range(0, len(cands), 512):
        d = cands[c0:c0 + 512, None]
        le = e[None, :] <= d
        correct = (le & pos[None, :]).sum(1) + (~le & neg[None, :]).sum(1)
        k = int(np.argmax(correct))  # (the first maximum of the block)
        if correct[k] > best_c:
            best_c, best_d = int(correct[k]), float(d[k, 0])
    return best_d, best_c


def brute_fit(energy, labels, rel, nr):
    gthr, gcorrect = _brute_one(energy, labels)
    thr = np.full(nr, gthr)
    counts = np.zeros((nr, 3), np.int64)
    for r in np.unique(rel):
        sel = rel == r
        thr[r], c = _brute_one(energy[sel], labels[sel])
        counts[r] = (int((labels[sel] == 1).sum()), int((labels[sel] == 0).sum()), c)
    return thr, counts, gthr, gcorrect


def check_fit(eng, triples, labels, energy=None):
    triples = np.asarray(triples, dtype=np.int32).reshape(-1, 3)
    labels = np.asarray(labels, dtype=np.uint8)
    energy = eng.score(triples) if energy is None else energy
    thr, counts, gthr, gcorrect = eng.fit_thresholds(triples, labels)
    xt, xc, xg, xgc = brute_fit(energy, labels, triples[:, 2], eng.nr)
    print(f"fit: {len(triples)} triples, relations fitted {int((xc[:, :2].sum(1) > 0).sum())} of {eng.nr}, "
          f"global {gthr!r}/{gcorrect} expected {xg!r}/{xgc}, threshold mismatches {int((thr != xt).sum())}, "
          f"count mismatches {int((counts != xc).any(1).sum())}")
    assert thr.dtype == np.float64 and counts.dtype == np.int64 and counts.shape == (eng.nr, 3)
    assert gthr == xg and gcorrect == xgc
    assert np.array_equal(counts, xc)
    assert np.array_equal(thr, xt)
    return thr, counts, gthr, gcorrect


# ------------------------------------------------------------------ 1. fit on the tiny set

@pytest.mark.parametrize("model,distance,precision", [("E", 0, 64), ("E", 1, 64), ("H", 0, 64), ("R", 0, 64),
                                                      ("E", 0, 32)])
def test_fit_tiny_against_oracle_energies(model, distance, precision):
    ds = tiny()
    n = 20
    eng, tables = _engine(model, n, ds, distance=distance, precision=precision, seed=n + distance)
    m = orc.Model(model, n, ds.num_entities, ds.num_relations, distance=distance, transr_compat=False)
    m.set_tables(*(_f32(tables) if precision == 32 else tables))
    known = np.concatenate([ds.train, ds.valid, ds.test])
    triples, labels = labelled(ds.valid, known, ds.num_entities, ds.num_relations, seed=1)
    assert len(triples) == 400
    energy = np.array([m.energy(int(h), int(t), int(r)) for h, t, r in triples])
    assert np.array_equal(eng.score(triples), energy)
    _, counts, _, _ = check_fit(eng, triples, labels, energy)
    assert (counts[:, 2] >= counts[:, :2].max(1)).all()


# ------------------------------------------------------------------ 2. sort and tile edges

@pytest.fixture(scope="module")
def tiny_e():
    ds = tiny()
    eng, _ = _engine("E", 20, ds, seed=3)
    return eng, ds


@pytest.mark.parametrize("count", [1, 2, 255, 256, 257, 2049])
def test_fit_list_lengths(count, tiny_e):
    eng, ds = tiny_e
    rng = np.random.default_rng(count)
    triples = ds.train[rng.integers(0, len(ds.train), count)]
    labels = rng.integers(0, 2, count).astype(np.uint8)
    check_fit(eng, triples, labels)


def test_fit_equal_keys_and_pure_relations(tiny_e, monkeypatch):
    eng, ds = tiny_e
    rng = np.random.default_rng(5)
    tr = ds.train
    by_size = np.argsort(-np.bincount(tr[:, 2], minlength=ds.num_relations), kind="stable")
    r_run, r_dup, r_pos, r_neg = (int(r) for r in by_size[:4])
    parts, labs = [], []
    # r_pos: all positives (delta = its largest energy); r_neg: all negatives (delta = -inf)
    for r, lab in ((r_pos, 1), (r_neg, 0)):
        rows = tr[tr[:, 2] == r][:40]
        parts.append(rows)
        labs.append(np.full(len(rows), lab, np.uint8))
    # r_dup: the same triples under both labels (runs of two equal keys, mixed labels)
    rows = tr[tr[:, 2] == r_dup][:30]
    parts += [rows, rows]
    labs += [np.ones(len(rows), np.uint8), np.zeros(len(rows), np.uint8)]
    # r_run: 300 copies of one triple with alternating labels among others: the
    # run of equal keys straddles a tile boundary of the relation's segment
    rows = tr[tr[:, 2] == r_run][:120]
    parts += [rows, np.repeat(rows[60:61], 300, axis=0)]
    labs += [rng.integers(0, 2, len(rows)).astype(np.uint8), (np.arange(300) % 2).astype(np.uint8)]
    triples, labels = np.concatenate(parts), np.concatenate(labs)
    order = rng.permutation(len(triples))
    triples, labels = triples[order], labels[order]
    thr, counts, _, _ = check_fit(eng, triples, labels)
    energy = eng.score(triples)
    assert thr[r_pos] == energy[triples[:, 2] == r_pos].max() and counts[r_pos].tolist() == [40, 0, 40]
    assert thr[r_neg] == -np.inf and counts[r_neg].tolist() == [0, 40, 40]
    assert counts[r_run, :2].sum() == 420  # more than one tile; the 300 equal keys cannot fit inside one
    # the result does not depend on the sort's launch geometry
    monkeypatch.setenv("KB2E_CLASSIFY_SORT_CHUNK", "256")
    again = eng.fit_thresholds(triples, labels)
    assert np.array_equal(again[0], thr) and np.array_equal(again[1], counts)


# ------------------------------------------------------------------ 3. skew

def test_fit_skewed_relations_carry_the_best_cut_across_tiles():
    ds = data.synthetic("small", seed=5, counts=(400, 3, 6000, 10, 10))
    eng, _ = _engine("E", 16, ds, seed=6)
    known = np.concatenate([ds.train, ds.valid, ds.test])
    triples, labels = labelled(ds.train, known, ds.num_entities, ds.num_relations, seed=2)
    per_rel = np.bincount(triples[:, 2], minlength=3)
    assert per_rel.max() >= 2049
    thr, counts, _, _ = check_fit(eng, triples, labels)
    hot = int(per_rel.argmax())
    energy = eng.score(triples)
    cut = int((energy[triples[:, 2] == hot] <= thr[hot]).sum())
    assert cut > 256  # the best cut lies beyond the first tile of the hottest segment


# ------------------------------------------------------------------ 4. two relation digits, global fallback

def _ds1345():
    return data.synthetic("small", seed=3, counts=(1345, 1345, 3000, 400, 400))


@pytest.fixture(scope="module")
def known1345():
    ds = _ds1345()
    return ds, np.concatenate([ds.train, ds.valid, ds.test])


@pytest.mark.parametrize("model", ["E", "R"])
def test_fit_1345_relations(model, known1345):
    ds, known = known1345
    eng, _ = _engine(model, 8, ds, seed=8)
    triples, labels = labelled(ds.valid, known, ds.num_entities, ds.num_relations, seed=7)
    thr, counts, gthr, _ = check_fit(eng, triples, labels)
    fitted = counts[:, :2].sum(1) > 0
    assert 0 < fitted.sum() < ds.num_relations
    assert (thr[~fitted] == gthr).all() and (counts[~fitted] == 0).all()
    assert fitted[256:].any()  # a relation id that needs the second digit


# ------------------------------------------------------------------ 5. classify

@pytest.mark.parametrize("model,precision", [("E", 64), ("H", 64), ("R", 64), ("R", 32)])
def test_classify_matches_score(model, precision):
    ds = tiny()
    eng, _ = _engine(model, 20, ds, precision=precision, seed=9)
    triples = np.concatenate([ds.test, ds.valid])
    energy = eng.score(triples)
    thr = np.sort(energy)[np.linspace(0, len(energy) - 1, ds.num_relations).astype(int)].copy()
    thr[0], thr[1] = -np.inf, np.inf
    lab, en = eng.classify(triples, thr, with_energy=True)
    assert lab.dtype == np.uint8 and np.array_equal(en, energy)
    assert np.array_equal(lab, (energy <= thr[triples[:, 2]]).astype(np.uint8))
    assert np.array_equal(eng.classify(triples, thr), lab)
    assert not lab[triples[:, 2] == 0].any() and lab[triples[:, 2] == 1].all()
    assert 0 < lab.sum() < len(lab)
    one = eng.classify(triples[:1], thr)
    assert np.array_equal(one, lab[:1])


# ------------------------------------------------------------------ 6. corrupt

def check_negatives(triples, neg, known, side):
    kset = set(map(tuple, np.asarray(known).tolist()))
    for (h, t, r), (nh, nt, nr_) in zip(np.asarray(triples).tolist(), neg.tolist()):
        assert nr_ == r
        if nh < 0:
            assert nt == -1
            continue
        assert (nh, nt, r) not in kset
        changed = (nh != h, nt != t)
        assert sum(changed) == 1
        if side != 2:
            assert changed[side]


@pytest.mark.parametrize("side", [0, 1, 2])
@pytest.mark.parametrize("constrained", [True, False])
def test_corrupt_tiny(side, constrained, tiny_e):
    eng, ds = tiny_e
    known = np.concatenate([ds.train, ds.valid, ds.test])
    neg, failed = eng.corrupt(ds.valid, known, seed=11, side=side, constrained=constrained)
    exp, xfailed, _ = np_corrupt(ds.valid, known, ds.num_entities, ds.num_relations, 11, side, constrained)
    assert neg.dtype == np.int32 and neg.shape == (len(ds.valid), 3)
    assert failed == xfailed and np.array_equal(neg, exp)
    check_negatives(ds.valid, neg, known, side)
    if side == 2:
        heads = int((neg[:, 0] != ds.valid[:, 0]).sum())
        assert 0 < heads < len(neg)
    again, _ = eng.corrupt(ds.valid, known, seed=11, side=side, constrained=constrained)
    assert np.array_equal(again, neg)
    other, _ = eng.corrupt(ds.valid, known, seed=12, side=side, constrained=constrained)
    assert not np.array_equal(other, neg)


def test_corrupt_1345_relations_takes_stage_two(known1345):
    ds, known = known1345
    eng, _ = _engine("E", 8, ds, seed=8)
    exp, xfailed, stage2 = np_corrupt(ds.valid, known, ds.num_entities, ds.num_relations, 7, 2, True)
    print(f"restatement: stage 2 for {stage2} of {len(ds.valid)} triples, failed {xfailed}")
    assert stage2 >= 1 and xfailed == 0
    neg, failed = eng.corrupt(ds.valid, known, seed=7, side=2, constrained=True)
    assert failed == 0 and np.array_equal(neg, exp)
    check_negatives(ds.valid, neg, known, 2)


def test_corrupt_complete_graph_fails_everywhere():
    full = np.array([(h, t, 0) for h in range(3) for t in range(3)], np.int32)
    eng = Engine("E", 4, 3, 1)
    for constrained in (True, False):
        neg, failed = eng.corrupt(full, full, seed=3, side=2, constrained=constrained)
        assert failed == len(full) and (neg[:, :2] == -1).all() and (neg[:, 2] == 0).all()
    # no known triples at all: every pool is empty, stage 2 draws from all entities
    neg, failed = eng.corrupt(full, None, seed=3, side=1, constrained=True)
    exp, xfailed, _ = np_corrupt(full, np.zeros((0, 3), np.int32), 3, 1, 3, 1, True)
    assert failed == xfailed and np.array_equal(neg, exp)


def test_corrupt_leaves_the_glibc_stream_alone(tiny_e):
    _, ds = tiny_e
    known = np.concatenate([ds.train, ds.valid, ds.test])
    streams = []
    for corrupt in (False, True):
        eng = Engine("E", 8, ds.num_entities, ds.num_relations, seed=5)
        first = [eng.rng_next() for _ in range(5)]
        if corrupt:
            eng.corrupt(ds.valid, known, seed=1)
        streams.append(first + [eng.rng_next() for _ in range(20)])
    assert streams[0] == streams[1]


# ------------------------------------------------------------------ 7. contract

def _trainer(ds):
    eng = Engine("E", 20, ds.num_entities, ds.num_relations, rate=0.01, batches=10, seed=7)
    eng.upload_triples(ds.train)
    eng.init_params()
    eng.train_epoch()
    return eng


def test_calls_change_nothing():
    ds = tiny()
    known = np.concatenate([ds.train, ds.valid, ds.test])
    triples, labels = labelled(ds.valid, known, ds.num_entities, ds.num_relations, seed=1)
    plain, eng = _trainer(ds), _trainer(ds)
    before, nbytes = eng.download_params(), eng.device_bytes()
    calls = (lambda: eng.fit_thresholds(triples, labels),
             lambda: eng.classify(triples, np.zeros(ds.num_relations), with_energy=True),
             lambda: eng.corrupt(ds.valid, known, seed=2))
    for call in calls:
        call()
        assert eng.device_bytes() == nbytes
        after = eng.download_params()
        assert all(np.array_equal(a, b) for a, b in zip(before[:2], after[:2]))
    assert eng.train_epoch() == plain.train_epoch()


def test_invalid_arguments(tiny_e):
    eng, ds = tiny_e
    nbytes = eng.device_bytes()
    t, lab = ds.valid[:10].copy(), np.ones(10, np.uint8)
    thr = np.zeros(ds.num_relations)
    empty = np.zeros((0, 3), np.int32)
    bad_e, bad_r = t.copy(), t.copy()
    bad_e[3, 1] = ds.num_entities
    bad_r[4, 2] = -1
    two = lab.copy()
    two[7] = 2
    calls = [lambda: eng.fit_thresholds(empty, lab[:0]), lambda: eng.fit_thresholds(t, two),
             lambda: eng.fit_thresholds(bad_e, lab), lambda: eng.fit_thresholds(bad_r, lab),
             lambda: eng.classify(empty, thr), lambda: eng.classify(bad_e, thr),
             lambda: eng.classify(t, thr[:-1]), lambda: eng.classify(t, np.zeros(ds.num_relations + 1)),
             lambda: eng.corrupt(empty, ds.train), lambda: eng.corrupt(bad_r, ds.train),
             lambda: eng.corrupt(t, bad_e), lambda: eng.corrupt(t, ds.train, side=3)]
    for k, call in enumerate(calls):
        with pytest.raises(EngineError, match="EINVAL"):
            call()
            pytest.fail(f"call {k} was accepted")
    assert eng.device_bytes() == nbytes


# ------------------------------------------------------------------ 8. end to end

def test_triple_classification_end_to_end():
    ds = tiny()
    eng = Engine("E", 20, ds.num_entities, ds.num_relations, rate=0.01, batches=10, seed=7, schedule="parallel")
    eng.upload_triples(ds.train)
    eng.init_params()
    for _ in range(5):
        eng.train_epoch()
    res = linkpred.triple_classification(eng, ds, seed=4)
    thr, counts = res["thresholds"], res["counts"]
    fitted = counts[:, :2].sum(1) > 0
    assert fitted.any() and (counts[fitted, 2] >= counts[fitted, :2].max(1)).all()
    known = np.concatenate([ds.train, ds.valid, ds.test])
    for name, pos, seed in (("valid", ds.valid, 4), ("test", ds.test, 5)):
        neg, failed = eng.corrupt(pos, known, seed=seed)
        neg = neg[neg[:, 0] >= 0]
        triples = np.concatenate([pos, neg])
        labels = np.concatenate([np.ones(len(pos), np.uint8), np.zeros(len(neg), np.uint8)])
        hit = eng.classify(triples, thr) == labels
        assert res[name]["failed"] == failed and res[name]["count"] == len(triples)
        assert res[name]["accuracy"] == hit.sum() / len(hit)
        for r, v in res[name]["per_relation"].items():
            sel = triples[:, 2] == r
            assert v["count"] == sel.sum() and v["accuracy"] == hit[sel].sum() / sel.sum()
        print(f"{name}: accuracy {res[name]['accuracy']:.4f} over {len(triples)} triples, failed {failed}")
    # the valid accuracy is the fit's own count
    assert res["valid"]["accuracy"] == counts[:, 2].sum() / res["valid"]["count"]


# ------------------------------------------------------------------ 9. CLI

def test_classify_cli_matches_linkpred(tmp_path):
    name = "transe_l1_bern"
    f = MANIFEST["runs"][name]["flags"]
    ds = tiny()
    d = os.path.join(GOLDEN, name)
    exe = tmp_path / "classifyTransE"
    exe.symlink_to(os.path.join(ROOT, "bin", "kb2e"))
    out = tmp_path / "labels.txt"
    cmd = [str(exe), "--datadir", os.path.join(GOLDEN, "tiny"), "--outdir", d, "--size", str(f["size"]), "--method",
           str(f["method"]), "--distance", str(f["distance"]), "--negseed", "9", "--out", str(out)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=300, check=True)
    eng = Engine("E", f["size"], ds.num_entities, ds.num_relations, distance=f["distance"])
    eng.upload_params(data.read_table(os.path.join(d, "entity2vec.bern"), ds.num_entities, f["size"]),
                      data.read_table(os.path.join(d, "relation2vec.bern"), ds.num_relations, f["size"]))
    exp = linkpred.triple_classification(eng, ds, seed=9)
    rid = data._load_ids(os.path.join(GOLDEN, "tiny", "relation2id.txt"))
    rows = [l.split("\t") for l in res.stdout.splitlines() if l.count("\t") == 4]
    assert sorted(rid[r[0]] for r in rows) == sorted(exp["test"]["per_relation"])
    for rname, thr, vacc, tcount, tacc in rows:
        r = rid[rname]
        assert float(thr) == pytest.approx(exp["thresholds"][r], abs=5.1e-7)
        assert float(vacc) == pytest.approx(exp["valid"]["per_relation"][r]["accuracy"], abs=5.1e-7)
        assert int(tcount) == exp["test"]["per_relation"][r]["count"]
        assert float(tacc) == pytest.approx(exp["test"]["per_relation"][r]["accuracy"], abs=5.1e-7)
    last = res.stdout.strip().splitlines()[-1]
    assert last == "accuracy: %.6f (%d triples)" % (exp["test"]["accuracy"], exp["test"]["count"])
    lines = out.read_text().splitlines()
    assert len(lines) == exp["test"]["count"] and exp["test"]["count"] >= len(ds.test)
    neg, _ = eng.corrupt(ds.test, np.concatenate([ds.train, ds.valid, ds.test]), seed=10)
    triples = np.concatenate([ds.test, neg[neg[:, 0] >= 0]])
    lab, en = eng.classify(triples, exp["thresholds"], with_energy=True)
    assert [l.split("\t")[0] for l in lines] == [str(int(x)) for x in lab]
    assert [l.split("\t")[1] for l in lines] == ["%.6f" % x for x in en]
