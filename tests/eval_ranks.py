"""The evaluator's per-triple ranks in plain numpy (tests/ only; a helper module
like fp32_step.py, not a conftest).

reference_ranks restates EmbeddingEvaluation::evalCorruption
(common/evaluation.cpp:124-179) for the stateless energies: per test triple and
corruption side, the energies of all |E| candidates, then

  raw rank      = 1 + candidates other than the truth with energy strictly below
                  the truth's (a candidate tying the truth is ranked after it:
                  std::sort leaves the order of equal energies open, the oracle
                  and the engine both settle it this way)
  filtered rank = the same count without the candidates whose triple is a row
                  of the filter.

The energies are tripleEnergy's through per-relation projections -- TransE the
row itself, TransH e - (w.e) w (transh/transh.cpp:18-26), TransR W^T e from
zeroed work vectors (transr/transr.cpp:20-25) -- and every sum runs over the
dimension in the reference's serial order, one elementwise FP64 numpy step per
element, so the bits are oracle/orc.c's (test_eval_ranks_model.py pins that).

Two table makers:

  exact_tables   small dyadic rationals: every product, difference, absolute
                 value, square and partial sum is exact in FP64 (and the entries
                 are float32 values), so an energy does not depend on the order
                 of its sum, and exact ties with the truth are plentiful; the
                 entities 1, 8, 15, ... are copies of entity 0 on top of that
  random_tables  test_gpu_predict.py's recipes (_tables, _random_transr): not
                 exact, the bits are the serial order's; tie-free in practice

Shared by test_eval_ranks_model.py (the reference against the C oracle, CPU) and
test_gpu_eval_ranks.py (the engine against the reference).
"""
from __future__ import annotations

import numpy as np

DUP_STRIDE = 7  # exact_tables: entity rows 1, 8, 15, ... are copies of row 0


# The model / width / distance grid of the tiny set, FP64 (TransH has no L2
# distance): both test files run every entry on both table makers.
GRID = ([("E", n, l1) for l1 in (True, False) for n in (2, 20, 64, 65, 130, 512)]
        + [("H", n, True) for n in (20, 65, 130, 512)]
        + [("R", n, l1) for l1 in (True, False) for n in (20, 65, 130)])
NTEST = 60         # the first 60 test triples of tiny_set()
MIN_TIE_SHARE = 1 / 8  # exact tables: share of the 2 * NTEST sides with a candidate tying the truth


def tiny_set():
    """(dataset, test, filter): data.synthetic("tiny", seed=5) -- 200 entities, 10
    relations -- its first NTEST test triples, and every triple of it as the filter.
    19 of the 2 * NTEST truths are entity 0 or a copy of it in exact_tables."""
    from kb2e_amd import data
    ds = data.synthetic("tiny", seed=5)
    return ds, ds.test[:NTEST], np.concatenate([ds.test, ds.train, ds.valid])


def grid_id(case):
    model, n, l1 = case
    return f"{model}{n}-{'L1' if l1 else 'L2'}"


def grid_tables(maker, model, ne, nr, n):
    """The grid's tables: seed n for either maker."""
    return (exact_tables if maker == "exact" else random_tables)(model, ne, nr, n, n)


def round32(t):
    return None if t is None else np.asarray(t, np.float64).astype(np.float32).astype(np.float64)


def duplicate_entities(ne):
    """Entity 0 and its copies in exact_tables."""
    return np.concatenate([[0], np.arange(1, ne, DUP_STRIDE)])


def exact_tables(model, ne, nr, n, seed):
    """(ent, rel, w): entities and relations k / 8 with integer |k| <= 8, TransH
    normals k / 2 with |k| <= 2, TransR matrices k / 4 with |k| <= 2.  At n <= 512
    every intermediate of every energy is a multiple of 2^-10 below 2^27: exact."""
    rng = np.random.default_rng(seed)
    ent = rng.integers(-8, 9, (ne, n)) / 8.0
    rel = rng.integers(-8, 9, (nr, n)) / 8.0
    ent[1::DUP_STRIDE] = ent[0]
    w = None
    if model == "H":
        w = rng.integers(-2, 3, (nr, n)) / 2.0
    elif model == "R":
        w = rng.integers(-2, 3, (nr, n, n)) / 4.0
    return ent, rel, w


def random_tables(model, ne, nr, n, seed, scale=0.3):
    """test_gpu_predict.py's _tables / _random_transr."""
    rng = np.random.default_rng(seed)
    if model == "R":
        ent = rng.standard_normal((ne, n))
        ent /= np.linalg.norm(ent, axis=1, keepdims=True)
        rel = rng.standard_normal((nr, n)) * scale
        w = np.eye(n)[None] + rng.standard_normal((nr, n, n)) * (scale / np.sqrt(n))
        return ent, rel, w
    ent = rng.standard_normal((ne, n)) * 0.2
    rel = rng.standard_normal((nr, n)) * 0.2
    w = None
    if model == "H":
        w = rng.standard_normal((nr, n))
        w /= np.linalg.norm(w, axis=1, keepdims=True)
    return ent, rel, w


def projections(model, tables, r, reverse=False):
    """float64[ne, n]: every entity's projection for relation r, its sums over the
    dimension taken serially (reverse: from the last element down, for the
    order-independence check of the exact tables)."""
    ent, _, w = tables
    n = ent.shape[1]
    ks = range(n - 1, -1, -1) if reverse else range(n)
    if model == "E":
        return np.array(ent, np.float64)
    if model == "H":
        s = np.zeros(len(ent))
        for k in ks:
            s = s + w[r, k] * ent[:, k]
        return ent - s[:, None] * w[r][None, :]
    assert model == "R", model
    P = np.zeros((len(ent), n))
    for j in ks:  # (W^T e)[i] = sum_j W[j][i] e[j], j ascending from zero
        P = P + ent[:, j][:, None] * w[r, j][None, :]
    return P


def energy_rows(P, relv, fixed, side, l1, reverse=False):
    """float64[len(fixed), ne]: row q holds the energies of every candidate x of
    query q -- (fixed[q], x, r) where side[q] is 1 (the tail is replaced),
    (x, fixed[q], r) where it is 0 -- from the relation's projections P."""
    fixed = np.asarray(fixed, np.int64)
    tail = np.asarray(side).astype(bool)[:, None]
    e = np.zeros((len(fixed), len(P)))
    n = P.shape[1]
    for k in (range(n - 1, -1, -1) if reverse else range(n)):
        c, f = P[None, :, k], P[fixed, k][:, None]
        d = np.where(tail, c - f, f - c) - relv[k]  # (P(t) - P(h)) - r
        e = e + (np.abs(d) if l1 else d * d)
    return e


def _known(filt):
    """(fixed entity, relation, side) -> the candidates the filter lists."""
    table = {}
    if filt is None:
        return table
    for h, t, r in np.asarray(filt, np.int64).reshape(-1, 3).tolist():
        table.setdefault((h, r, 1), []).append(t)
        table.setdefault((t, r, 0), []).append(h)
    return table


def reference_energies(model, tables, test, l1, precision=64, reverse=False):
    """float64[ntest, 2, ne]: per test triple the head-side and the tail-side
    candidate energies."""
    if precision == 32:
        tables = tuple(round32(t) for t in tables)
    test = np.asarray(test, np.int64).reshape(-1, 3)
    ne = len(tables[0])
    out = np.zeros((len(test), 2, ne))
    for r in np.unique(test[:, 2]).tolist():
        idx = np.nonzero(test[:, 2] == r)[0]
        P = projections(model, tables, r, reverse)
        relv = np.asarray(tables[1], np.float64)[r]
        out[idx, 0] = energy_rows(P, relv, test[idx, 1], np.zeros(len(idx), int), l1, reverse)
        out[idx, 1] = energy_rows(P, relv, test[idx, 0], np.ones(len(idx), int), l1, reverse)
    return out


def ranks_from_energies(energies, test, filt):
    """int64[ntest, 4]: head raw, head filtered, tail raw, tail filtered."""
    test = np.asarray(test, np.int64).reshape(-1, 3)
    known = _known(filt)
    ranks = np.zeros((len(test), 4), np.int64)
    for i, (h, t, r) in enumerate(test.tolist()):
        for side, fixed, truth in ((0, t, h), (1, h, t)):
            row = energies[i, side]
            above = row < row[truth]
            above[truth] = False
            ranks[i, 2 * side] = 1 + above.sum()
            above[known.get((fixed, r, side), [])] = False
            ranks[i, 2 * side + 1] = 1 + above.sum()
    return ranks


def reference_ranks(model, tables, test, filt, l1, precision=64):
    return ranks_from_energies(reference_energies(model, tables, test, l1, precision), test, filt)


def tie_sides(energies, test):
    """bool[ntest, 2]: the sides on which a candidate other than the truth has the
    truth's energy bit for bit."""
    test = np.asarray(test, np.int64).reshape(-1, 3)
    out = np.zeros((len(test), 2), bool)
    for i, (h, t, _) in enumerate(test.tolist()):
        for side, truth in ((0, h), (1, t)):
            row = energies[i, side]
            out[i, side] = (row == row[truth]).sum() > 1
    return out


def summary(ranks):
    """evaluate()'s four numbers from per-triple ranks (common/evaluation.cpp:246-250)."""
    ranks = np.asarray(ranks)
    return {"raw_rank": ranks[:, [0, 2]].mean(), "raw_hits10": (ranks[:, [0, 2]] <= 10).mean(),
            "filtered_rank": ranks[:, [1, 3]].mean(), "filtered_hits10": (ranks[:, [1, 3]] <= 10).mean()}
