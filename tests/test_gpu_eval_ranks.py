"""The evaluator's per-triple ranks (eval_rank_kernel behind kb2e_rank_triples and
kb2e_evaluate) against tests/eval_ranks.py, element by element.

Every comparison is np.array_equal(eng.rank_triples(test, filt),
reference_ranks(...)): no tolerance anywhere.  The reference's energies are
bit-identical restatements of the oracle's (test_eval_ranks_model.py), and on the
exact tables they do not depend on the order of their sums either.  Each case
also holds eng.evaluate's four numbers to the means and <= 10 fractions of those
ranks (abs 1e-12, test_gpu_predict.py's bar for the float means).

  a  models, distances, precisions, widths: eval_ranks.GRID on tiny_set() (200
     entities, 10 relations, 60 test triples), exact and random tables, FP64;
     FP32 tables at one narrow and one wide n a model
  b  KB2E_EVAL_ROWS_L2=1 (eval_rank_kernel<false>) against the default form and
     the reference, one narrow and one wide n a model
  c  candidate blocks of 256: |E| = 255, 256, 257, 777 with the truth, a tying
     duplicate and a filtered candidate at ids 0, 255, 256, |E| - 1
  d  query tiles of 16: relations with 17, 1, 0, 33, 16, 15 test triples,
     interleaved; a shuffled copy; ntest = 1
  e  ties: the exact tables of a (19 .. 120 of 120 sides tie), and a table whose
     entity rows are all identical (every rank 1)
  f  head == tail test triples, one triple three times, (t, t, r) and (h, h, r)
     filter rows
  g  filters: doubled, without the test triples, every candidate of one side,
     mirrored (t, h, r) rows only, none
  h  contract: nfilter < 0 and out-of-range ids are KB2E_EINVAL from kb2e_evaluate,
     kb2e_evaluate_transr_compat and kb2e_rank_triples alike

The conditions a case rests on (a tie is present, a filtered candidate did rank
above the truth, ...) are asserted on the reference alone before the engine is
asked.

Observed on an MI355X (87 cases, 4.8 s in all; no case failed and no kernel
needed a fix):

  case                                   time
  a  FP64 grid, first case               0.33 s (the process's first launch)
  a  FP64 / FP32 at n = 512, R at 130    0.13 s each
  a, b  every narrower width             under 0.1 s
  c .. h  every case                     under 0.1 s

Against one-token changes of eval_rank_kernel (scratch builds, never committed):
`<` to `<=` on the head side turns every exact-table case of a and b red, c at
all four sizes, d, e and f[exact]; filt.has(i, r, t) with head and tail swapped
turns 82 of the 87 red, among them c, d, f and the doubled, partial, one-sided
and mirrored filters of g.  Dropping `i != h` changes no output and no case:
the candidate i == h computes the truth's own energy with the same operations in
the same order as eval_target_kernel (the build does not contract to FMA), so
`eh < target` is false for it whatever the inputs; the guard is redundant next
to the strict comparison, and only a change of the comparison would expose it
(that is the first change).
"""
import ctypes as C

import numpy as np
import pytest

import eval_ranks as er
from kb2e_amd import data
from kb2e_amd.engine import Engine, EngineError, lib

pytestmark = pytest.mark.gpu

_MEMO = {}
NO_FILTER = np.zeros((0, 3), np.int32)
KEYS = ("raw_rank", "raw_hits10", "filtered_rank", "filtered_hits10")


def _frozen(a):
    if a is not None:
        a.flags.writeable = False
    return a


def _tiny():
    if "tiny" not in _MEMO:
        ds, test, filt = er.tiny_set()
        _MEMO["tiny"] = (ds, _frozen(test), _frozen(filt))
    return _MEMO["tiny"]


def _grid_reference(maker, model, n, l1, precision=64):
    """(tables, ranks) of a grid case on tiny_set(), computed once and read-only."""
    key = (maker, model, n, l1, precision)
    if key not in _MEMO:
        ds, test, filt = _tiny()
        tables = tuple(_frozen(t) for t in er.grid_tables(maker, model, ds.num_entities, ds.num_relations, n))
        _MEMO[key] = (tables, _frozen(er.reference_ranks(model, tables, test, filt, l1, precision)))
    return _MEMO[key]


def _engine(model, tables, l1=True, precision=64):
    ent, rel, _ = tables
    eng = Engine(model, ent.shape[1], len(ent), len(rel), distance=0 if l1 else 1, precision=precision,
                 transr_compat=False)
    eng.upload_params(*tables)
    return eng


def _check(eng, test, filt, want):
    """rank_triples == want, element by element, and evaluate's four numbers are their means."""
    got = eng.rank_triples(test, filt)
    assert got.shape == (len(test), 4) and got.dtype == np.int64
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert np.array_equal(got, want), (len(bad), [(int(i), np.asarray(test)[i].tolist(), got[i].tolist(),
                                                   want[i].tolist()) for i in bad[:5]])
    res = eng.evaluate(test, NO_FILTER if filt is None else filt)
    exp = er.summary(want)
    for k in KEYS:
        assert res[k] == pytest.approx(exp[k], abs=1e-12), k
    return got


def _ids(cases):
    return [f"{maker}-{er.grid_id(case)}" for maker, case in cases]


# ------------------------------------------------------------------ a. the grid

GRID64 = [(maker, case) for maker in ("exact", "random") for case in er.GRID]
NARROW_WIDE = [("E", 20, True), ("E", 512, False), ("H", 20, True), ("H", 512, True), ("R", 20, False),
               ("R", 130, True)]
GRID_NW = [(maker, case) for maker in ("exact", "random") for case in NARROW_WIDE]


@pytest.mark.parametrize("maker,case", GRID64, ids=_ids(GRID64))
def test_ranks_fp64(maker, case):
    model, n, l1 = case
    _, test, filt = _tiny()
    tables, want = _grid_reference(maker, model, n, l1)
    _check(_engine(model, tables, l1), test, filt, want)


@pytest.mark.parametrize("maker,case", GRID_NW, ids=_ids(GRID_NW))
def test_ranks_fp32_tables(maker, case):
    """precision=32: float tables widened on the device; the reference on the tables
    rounded through float32 (the exact tables are float32 values as they stand)."""
    model, n, l1 = case
    _, test, filt = _tiny()
    tables, want = _grid_reference(maker, model, n, l1, 32)
    if maker == "exact":
        assert np.array_equal(want, _grid_reference(maker, model, n, l1)[1])
    _check(_engine(model, tables, l1, precision=32), test, filt, want)


# ------------------------------------------------------------------ b. both kernel forms

@pytest.mark.parametrize("maker,case", GRID_NW, ids=_ids(GRID_NW))
def test_ranks_rows_from_l2_equal_rows_in_lds(maker, case, monkeypatch):
    model, n, l1 = case
    _, test, filt = _tiny()
    tables, want = _grid_reference(maker, model, n, l1)
    eng = _engine(model, tables, l1)
    monkeypatch.setenv("KB2E_EVAL_ROWS_L2", "0")
    lds = _check(eng, test, filt, want)
    monkeypatch.setenv("KB2E_EVAL_ROWS_L2", "1")
    l2 = _check(eng, test, filt, want)
    assert np.array_equal(l2, lds)


# ------------------------------------------------------------------ c. candidate blocks

@pytest.mark.parametrize("ne", [255, 256, 257, 777])
def test_ranks_candidate_block_edges(ne):
    nr, n = 5, 20
    ds = data.synthetic("small", seed=3, counts=(ne, nr, 1500, 50, 50))
    ent, rel, _ = er.exact_tables("E", ne, nr, n, ne)
    spots = sorted({p for p in (0, 255, 256, ne - 1) if p < ne})
    partner = {p: (1 if p == 0 else p - 5) for p in spots}  # the row that entity p duplicates
    for p in spots[1:]:
        ent[p] = ent[partner[p]]
    assert (ent[1] == ent[0]).all()
    tables = (ent, rel, None)
    busy = set(spots) | set(partner.values())
    test, planted, truth_at, tie_at, filtered_at = [], [], [], [], []
    for j, p in enumerate(spots):
        a, r = 100 + j, j % nr
        truth_at += [len(test), len(test) + 1]
        test += [(p, a, r), (a, p, r)]
        tie_at += [(len(test), 0, p, partner[p]), (len(test) + 1, 1, p, partner[p])]
        test += [(partner[p], a, r), (a, partner[p], r)]
        # the worst entity as the truth, so that candidate p ranks above it; p's triple goes into the filter
        P = er.projections("E", tables, r)
        rows = er.energy_rows(P, rel[r], [a, a], [0, 1], True)
        rows[:, sorted(busy)] = -1
        h, t = int(rows[0].argmax()), int(rows[1].argmax())
        filtered_at += [(len(test), 0, p), (len(test) + 1, 1, p)]
        test += [(h, a, r), (a, t, r)]
        planted += [(p, a, r), (a, p, r)]
    test = np.concatenate([ds.test[:20], np.array(test, np.int32)])
    off = 20
    filt = np.concatenate([ds.train, ds.valid, ds.test, np.array(planted, np.int32)])
    en = er.reference_energies("E", tables, test, True)
    want = er.ranks_from_energies(en, test, filt)
    without = er.ranks_from_energies(en, test, filt[:-len(planted)])
    for i, side, p, x in tie_at:
        assert en[off + i, side, p] == en[off + i, side, x] and test[off + i, side] == x
    for i, side, p in filtered_at:
        truth = test[off + i, side]
        assert en[off + i, side, p] < en[off + i, side, truth]
        assert want[off + i, 2 * side + 1] < without[off + i, 2 * side + 1] <= want[off + i, 2 * side]
    at = off + np.array(truth_at)
    assert set(spots) <= set(test[at[0::2], 0].tolist()) and set(spots) <= set(test[at[1::2], 1].tolist())
    _check(_engine("E", tables), test, filt, want)


# ------------------------------------------------------------------ d. query tiles

def _tile_case():
    if "tile" not in _MEMO:
        ne, nr, n = 200, 6, 20
        rng = np.random.default_rng(16)
        counts = [17, 1, 0, 33, 16, 15]
        r = rng.permutation(np.repeat(np.arange(nr), counts))
        assert (np.bincount(r, minlength=nr) == counts).all() and (np.diff(r) < 0).any()
        test = np.stack([rng.integers(0, ne, len(r)), rng.integers(0, ne, len(r)), r], axis=1).astype(np.int32)
        extra = np.stack([rng.integers(0, ne, 600), rng.integers(0, ne, 600), rng.integers(0, nr, 600)], axis=1)
        filt = np.concatenate([test, extra.astype(np.int32)])
        tables = er.exact_tables("E", ne, nr, n, 16)
        _MEMO["tile"] = (tables, _frozen(test), _frozen(filt), _frozen(er.reference_ranks("E", tables, test, filt, True)))
    return _MEMO["tile"]


def test_ranks_query_tile_edges_in_the_callers_order():
    tables, test, filt, want = _tile_case()
    assert len(test) == 82 and (want[:, 1] < want[:, 0]).any() and len(np.unique(want[:, 0])) > 20
    eng = _engine("E", tables)
    _check(eng, test, filt, want)
    perm = np.random.default_rng(1).permutation(len(test))
    _check(eng, test[perm], filt, want[perm])
    back = np.arange(len(test))[::-1]
    _check(eng, test[back], filt, want[back])


def test_ranks_single_test_triple():
    tables, test, filt, want = _tile_case()
    eng = _engine("E", tables)
    lone = int(np.nonzero(test[:, 2] == 1)[0][0])  # the relation with one test triple
    for i in (0, lone, len(test) - 1):
        _check(eng, test[i:i + 1], filt, want[i:i + 1])


# ------------------------------------------------------------------ e. ties

@pytest.mark.parametrize("model", ["E", "H", "R"])
def test_ranks_all_entity_rows_identical(model):
    """Every candidate ties the truth bit for bit: every rank, raw and filtered, is 1."""
    ds, test, filt = _tiny()
    ent, rel, w = er.exact_tables(model, ds.num_entities, ds.num_relations, 20, 5)
    ent[:] = ent[3]
    want = er.reference_ranks(model, (ent, rel, w), test, filt, True)
    assert (want == 1).all()
    _check(_engine(model, (ent, rel, w)), test, filt, want)


# ------------------------------------------------------------------ f. test-triple shapes

@pytest.mark.parametrize("maker", ["exact", "random"])
def test_ranks_loops_repeats_and_loop_filter_rows(maker):
    ds, tiny_test, tiny_filt = _tiny()
    tables, _ = _grid_reference(maker, "E", 20, True)
    base = tiny_test[:12]
    loops = np.stack([base[:6, 0], base[:6, 0], base[:6, 2]], axis=1)        # head == tail
    loops = np.concatenate([loops, [(0, 0, 1), (1, 1, 1)]]).astype(np.int32)  # (entity 0 and its copy)
    test = np.concatenate([base, loops, base[3:4], base[3:4], base[3:4], loops[:1]])
    # (t, t, r): a head-side candidate of (h, t, r); (h, h, r): a tail-side candidate
    loop_rows = np.concatenate([np.stack([base[:, 1], base[:, 1], base[:, 2]], axis=1),
                                np.stack([base[:, 0], base[:, 0], base[:, 2]], axis=1)]).astype(np.int32)
    filt = np.concatenate([tiny_filt, loop_rows])
    en = er.reference_energies("E", tables, test, True)
    want = er.ranks_from_energies(en, test, filt)
    without = er.ranks_from_energies(en, test, tiny_filt)
    # the loop rows did remove candidates on both sides
    assert (want[:12, 1] < without[:12, 1]).any() and (want[:12, 3] < without[:12, 3]).any()
    assert len(test) == 24 and (want[20:23] == want[3]).all() and np.array_equal(want[23], want[12])
    assert (test[12:20, 0] == test[12:20, 1]).all()
    _check(_engine("E", tables), test, filt, want)


# ------------------------------------------------------------------ g. filters

@pytest.fixture(scope="module")
def tiny_random():
    """TransE n = 20 on the random tables: no ties, ranks spread over 1 .. 200."""
    tables, want = _grid_reference("random", "E", 20, True)
    return _engine("E", tables), tables, want


def test_filter_rows_listed_twice(tiny_random):
    eng, tables, want = tiny_random
    _, test, filt = _tiny()
    twice = np.concatenate([filt, filt])
    assert np.array_equal(er.reference_ranks("E", tables, test, twice, True), want)
    _check(eng, test, twice, want)
    _check(eng, test, np.repeat(filt, 2, axis=0), want)


def test_filter_without_the_test_triples(tiny_random):
    eng, tables, _ = tiny_random
    ds, test, _ = _tiny()
    filt = np.concatenate([ds.train, ds.valid])
    keys = {tuple(row) for row in filt.tolist()}
    assert not any(tuple(row) in keys for row in test.tolist())
    _check(eng, test, filt, er.reference_ranks("E", tables, test, filt, True))


@pytest.mark.parametrize("side", [0, 1])
def test_filter_lists_every_candidate_of_one_side(tiny_random, side):
    eng, tables, full = tiny_random
    ds, test, _ = _tiny()
    ne = ds.num_entities
    i = int(np.argmax(np.minimum(full[:, 0], full[:, 2])))  # a triple ranked low on both sides
    h, t, r = test[i].tolist()
    every = np.arange(ne)
    rows = (every, np.full(ne, t), np.full(ne, r)) if side == 0 else (np.full(ne, h), every, np.full(ne, r))
    filt = np.stack(rows, axis=1).astype(np.int32)
    raw = er.reference_ranks("E", tables, test[i:i + 1], None, True)
    assert raw[0, 0] > 1 and raw[0, 2] > 1
    want = raw.copy()
    want[0, 2 * side + 1] = 1  # that side's filtered rank; the other side's stays the raw one
    assert np.array_equal(er.reference_ranks("E", tables, test[i:i + 1], filt, True), want)
    _check(eng, test[i:i + 1], filt, want)


def test_filter_of_mirrored_triples_changes_nothing(tiny_random):
    """For the test triple (h, t, r): the rows (t, x, r) and (x, h, r), the mirror
    images of every head candidate (x, t, r) and tail candidate (h, x, r), without
    the two loops (t, t, r) and (h, h, r), which are candidates themselves.  None
    of them is a candidate's triple, so filtered == raw; a probe with head and tail
    swapped would find every one of them."""
    eng, tables, full = tiny_random
    ds, test, _ = _tiny()
    ne = ds.num_entities
    picks = np.argsort(-np.minimum(full[:, 0], full[:, 2]))[:4]
    for i in picks.tolist():
        h, t, r = test[i].tolist()
        assert h != t
        xs = np.arange(ne)
        a = np.stack([np.full(ne, t), xs, np.full(ne, r)], axis=1)[xs != t]
        b = np.stack([xs, np.full(ne, h), np.full(ne, r)], axis=1)[xs != h]
        filt = np.concatenate([a, b]).astype(np.int32)
        raw = er.reference_ranks("E", tables, test[i:i + 1], None, True)
        assert raw[0, 0] > 1 and raw[0, 2] > 1 and raw[0, 0] == raw[0, 1] and raw[0, 2] == raw[0, 3]
        assert np.array_equal(er.reference_ranks("E", tables, test[i:i + 1], filt, True), raw)
        _check(eng, test[i:i + 1], filt, raw)
    # and over the whole test set: the mirror images of its own filter, minus what the filter holds
    _, _, filt = _tiny()
    keys = {tuple(row) for row in filt.tolist()}
    mirror = np.array([row for row in filt[:, [1, 0, 2]].tolist() if tuple(row) not in keys], np.int32)
    assert len(mirror) > len(filt) // 2
    raw = er.reference_ranks("E", tables, test, None, True)
    want = er.reference_ranks("E", tables, test, mirror, True)
    _check(eng, test, mirror, want)
    assert (want[:, [0, 2]] == raw[:, [0, 2]]).all()


def test_no_filter_gives_filtered_equal_raw(tiny_random):
    eng, tables, full = tiny_random
    _, test, _ = _tiny()
    want = er.reference_ranks("E", tables, test, None, True)
    assert np.array_equal(want[:, 0], want[:, 1]) and np.array_equal(want[:, 2], want[:, 3])
    assert np.array_equal(want[:, [0, 2]], full[:, [0, 2]]) and (want[:, [1, 3]] > full[:, [1, 3]]).any()
    got = _check(eng, test, None, want)
    assert np.array_equal(got, eng.rank_triples(test, NO_FILTER))


# ------------------------------------------------------------------ h. contract

EINVAL = 1


def _cols(a):
    a = np.ascontiguousarray(a, dtype=np.int32).reshape(-1, 3)
    cols = [np.ascontiguousarray(a[:, k]) for k in range(3)]
    return cols, [c.ctypes.data_as(C.POINTER(C.c_int32)) for c in cols]


def _abi_calls(eng, test, filt, nfilter):
    """The status of kb2e_evaluate, kb2e_rank_triples and (TransR) kb2e_evaluate_transr_compat."""
    L = lib()
    tk, tp = _cols(test)
    fk, fp = _cols(filt)
    out = np.zeros(5)
    ranks = np.zeros((len(test), 4), np.int64)
    work = np.zeros(2 * eng.n)
    dp = C.POINTER(C.c_double)
    st = {"evaluate": L.kb2e_evaluate(eng.h, *tp, len(test), *fp, nfilter, out.ctypes.data_as(dp)),
          "rank_triples": L.kb2e_rank_triples(eng.h, *tp, len(test), *fp, nfilter,
                                              ranks.ctypes.data_as(C.POINTER(C.c_int64)))}
    if eng.kind == 2:
        st["evaluate_transr_compat"] = L.kb2e_evaluate_transr_compat(eng.h, *tp, len(test), *fp, nfilter,
                                                                     work.ctypes.data_as(dp), out.ctypes.data_as(dp),
                                                                     None, None)
    del tk, fk
    return st


@pytest.mark.parametrize("model", ["E", "R"])
def test_bad_filter_counts_and_ids_are_refused(model):
    ds, test, filt = _tiny()
    ne, nr = ds.num_entities, ds.num_relations
    tables, want = _grid_reference("random", model, 20, True)
    eng = _engine(model, tables)
    test, filt = test[:8], filt[:50]
    ok = _abi_calls(eng, test, filt, len(filt))
    assert set(ok.values()) == {0} and len(ok) == (3 if model == "R" else 2)
    for nfilter in (-1, -len(filt), -2 ** 40):
        assert set(_abi_calls(eng, test, filt, nfilter).values()) == {EINVAL}, nfilter
    for bad in ((ne, 0, 0), (0, ne, 0), (0, 0, nr), (-1, 0, 0), (0, -1, 0), (0, 0, -1)):
        t2 = np.concatenate([test, [bad]]).astype(np.int32)
        assert set(_abi_calls(eng, t2, filt, len(filt)).values()) == {EINVAL}, ("test", bad)
        f2 = np.concatenate([filt, [bad]]).astype(np.int32)
        assert set(_abi_calls(eng, test, f2, len(f2)).values()) == {EINVAL}, ("filter", bad)
    with pytest.raises(EngineError):
        eng.evaluate(np.array([(ne, 0, 0)], np.int32), filt)
    # still usable, and unchanged
    _check(eng, _tiny()[1], _tiny()[2], want)
