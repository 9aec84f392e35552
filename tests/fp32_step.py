"""One FP32 batch at a time against the FP64 oracle (tests/ only; a plain helper
module like gpu_common.py, not a conftest).

Within a batch every energy, hinge decision and L1 sign comes from the
batch-start tables (oracle/orc.c orc_begin_batch / train_kb; the engine does the
same).  So when both sides start a batch from the same float-representable
tables and no sample of that batch sits near a decision, the FP32 engine must
agree with the FP64 reference to FP32 rounding, element by element.  This module
holds the pieces of that comparison:

  sign_args            the reference's L1 sign arguments x, in numpy FP64
  batch_preconditions  how near a batch comes to a decision (ORDERED)
  lockstep             the batch-by-batch driver (engine, or the reference alone)
  compare_tables       largest |difference| per table and the row it sits in
  find_seeds           the seed search behind the committed cases (run by hand:
                       `python tests/fp32_step.py`)

and the cases themselves (ORDERED_CASES, PARALLEL_CASES), shared by
test_gpu_fp32_step.py (the engine) and test_fp32_step_model.py (the CPU half:
the committed seeds meet the preconditions on the reference alone).
"""
from __future__ import annotations

import os
import sys
from dataclasses import dataclass, field, replace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:  # run by hand (the seed search); under pytest conftest.py did this
    sys.path.insert(0, ROOT)

from kb2e_amd import data  # noqa: E402
from oracle import orc  # noqa: E402
from oracle.parallel import (transe_parallel_batches, transh_parallel_batches,  # noqa: E402
                             transr_parallel_batches)

RATE = 0.01
MARGIN = 1.0
NB = 3                 # batches compared per case
# the guards: the reference's own numbers, never the engine's
MIN_SLACK = 1e-4       # smallest |E+ + margin - E-| of any sample of a compared batch
MIN_ABS_X = 1e-6       # smallest |x| of an L1 sign argument of an active sample: about ten
#                        times the float error of an n-term projection at these magnitudes
# the bars
LOSS_RTOL = 1e-5
ELEM_ATOL = 1e-3 * RATE  # a wrong order or a missed element shows at the learning-rate scale (a
#                          batch moves touched rows by >= 7e-2); FP32 rounding is 2^-24 a store,
#                          <= 31 touches a row, wave sums of n <= 512 terms: a few 1e-6
ELEM_ATOL_CEIL = RATE / 50  # no case's bar may rise above this, whatever it measured


@dataclass(frozen=True)
class Case:
    model: str               # "E", "H", "R" (TransR: the fixed, zeroed energy)
    dim: int
    seed: int                # orc.srand seed, chosen on the CPU (find_seeds)
    schedule: str = "ordered"
    distance: int = 0        # 0 L1, 1 L2 (TransH is always L1)
    batches: int = 30        # B = 3000 / batches
    sub: int | None = None   # PARALLEL TransR sub-batches (None: the engine's default by width)
    env: tuple = ()          # ((name, value), ...) set before the engine is created
    atol: float = ELEM_ATOL  # raised only with a written cause next to the case
    note: str = ""

    @property
    def l1(self):
        return self.model == "H" or self.distance == 0

    @property
    def id(self):
        s = f"{self.schedule[:3]}-{self.model}{self.dim}-{'L1' if self.l1 else 'L2'}"
        if self.sub is not None:
            s += f"-sub{self.sub}"
        elif self.schedule == "parallel" and self.model == "R":
            s += "-subdef"
        for k, v in self.env:
            s += f"-{k.replace('KB2E_RPAR_', '').lower()}{v}"
        return s


# Seeds (find_seeds): the first of 1..32 at which the reference alone, its tables
# rounded to float before every batch, meets MIN_SLACK and MIN_ABS_X with a factor
# two to spare (the engine's tables differ from that run's by FP32 rounding).  The
# wide L1 rows of TransE and TransH start from draws of sigma = 1 / n, so their sign
# arguments are small and dense around zero in the first batches and few seeds
# qualify; no guard is lowered for them, the search is longer:
#   E 200 ordered    seed 28, the only one of 1..32 (min |x| 1.17e-6)
#   E 130 parallel   seeds 2 and 16 of 1..32 reach 1.5e-6; 35 is the first past 3e-6
#   H 130            seed 10 of 1..32 reaches 1.57e-6; 395 is the first past 2.3e-6
#                    under both schedules
#   H 260 ordered    none of 1..32 (best 4.9e-7) and TransH has no L2 distance to
#                    fall back on; 3894 is the first of 1..8000 (1.07e-6)
#   H 260 parallel   none of 1..8000 (3894 does not carry over: after the first batch
#                    the two schedules' tables, and so the later sign arguments, differ)
#   H 300            none of 1..299 under either schedule
#   E 300 ordered L1 none of 1..199
# So the four-chunk float builds (257 <= n <= 512) are compared under L2, where no sign
# argument enters: seed 1 at every width under both schedules (slack 0.997: at sigma = 1 / n
# the energies are far below the margin, every sample is active and moves its rows).  FP32
# L1 at four chunks rests on ord-H260-L1 and, for the sign-word layout that L1 adds to L2,
# on the FP64 cases of test_gpu_wide_rows.py, which share the float builds' templates.
ORDERED_CASES = [
    Case("E", 17, 1), Case("E", 130, 1, distance=1), Case("E", 200, 28),
    Case("E", 300, 1, distance=1), Case("E", 385, 1, distance=1), Case("E", 512, 1, distance=1),
    Case("H", 33, 1), Case("H", 130, 395), Case("H", 260, 3894),
    Case("R", 20, 1), Case("R", 50, 1), Case("R", 33, 2), Case("R", 64, 1),
    Case("R", 100, 1), Case("R", 190, 9), Case("R", 200, 3),
    Case("R", 512, 25, batches=60),
    Case("R", 50, 1, distance=1),
]

_P = dict(schedule="parallel")
PARALLEL_CASES = [
    Case("E", 17, 1, **_P), Case("E", 130, 35, **_P),
    Case("E", 257, 1, distance=1, **_P), Case("E", 300, 1, distance=1, **_P),
    Case("E", 385, 1, distance=1, **_P), Case("E", 512, 1, distance=1, **_P),
    Case("H", 33, 1, **_P), Case("H", 130, 395, **_P),
    Case("R", 20, 1, sub=1, **_P), Case("R", 50, 1, sub=1, **_P), Case("R", 100, 2, sub=1, **_P),
    Case("R", 128, 2, sub=1, **_P), Case("R", 160, 1, sub=1, **_P), Case("R", 260, 2, sub=1, **_P),
    Case("R", 50, 1, **_P),
    Case("R", 50, 1, sub=1, env=(("KB2E_RPAR_MFMA", "1"),), **_P),
    Case("R", 50, 1, sub=1, env=(("KB2E_RPAR_MFMA", "0"),), **_P),
]


def dataset():
    return data.synthetic("tiny", seed=5)


def resolved_sub(case):
    """kb2e_config.sub_batches as the context resolves it (include/kb2e_engine.h)."""
    if case.schedule != "parallel" or case.model != "R":
        return 1
    return case.sub if case.sub is not None else (2 if case.dim <= 64 else 3)


def round32(t):
    return None if t is None else np.asarray(t, np.float64).astype(np.float32).astype(np.float64)


def float_representable(t):
    return t is None or np.array_equal(t, round32(t))


# ------------------------------------------------------------ the reference's x

def sign_args(model, ent, rel, w, h, t, r):
    """The vector whose signs are the L1 update direction of triple (h, t, r), from
    the snapshot tables in FP64 (oracle/orc.c transe_update, transh_update,
    transr_update): E t - h - r; H (t - (w.t) w) - (h - (w.h) w) - r;
    R W^T (t - h) - r."""
    eh, et, er = ent[h], ent[t], rel[r]
    if model == "E":
        return et - eh - er
    if model == "H":
        wr = w[r]
        return (et - (wr @ et) * wr) - (eh - (wr @ eh) * wr) - er
    assert model == "R", model
    return w[r].T @ (et - eh) - er


def _samples(ds, si, sj, side):
    h, t, r = ds.train[si, 0], ds.train[si, 1], ds.train[si, 2]
    sd = np.asarray(side).astype(bool)
    return h, t, r, np.where(sd, h, sj), np.where(sd, sj, t)


def touch_counts(ds, si, sj, side, active):
    """Updates a batch applies to every entity / relation row (two per active
    sample and role)."""
    h, t, r, nh, nt = _samples(ds, si, sj, side)
    a = np.nonzero(active)[0]
    ent = np.bincount(np.concatenate([h[a], t[a], nh[a], nt[a]]), minlength=ds.num_entities)
    rel = 2 * np.bincount(r[a], minlength=ds.num_relations)
    return {"ent": ent, "rel": rel}


def batch_preconditions(m, ds, si, sj, side, l1, margin=MARGIN):
    """How near a batch comes to a decision, on the reference alone: `m` holds the
    batch-start tables.  Returns the smallest hinge slack |E+ + margin - E-| over
    every sample (m.energy), the smallest |x| of a sign argument over the positive
    and corrupted triples of the active samples (L1 only, else inf), and the
    per-row touch counts."""
    ent, rel, w = m.tables()
    kind = "EHR"[m.kind]
    h, t, r, nh, nt = _samples(ds, si, sj, side)
    slack = np.empty(len(si))
    active = np.zeros(len(si), bool)
    min_x = np.inf
    for k in range(len(si)):
        ep = m.energy(int(h[k]), int(t[k]), int(r[k]))
        en = m.energy(int(nh[k]), int(nt[k]), int(r[k]))
        slack[k] = abs(ep + margin - en)
        active[k] = ep + margin > en
        if l1 and active[k]:
            for (a, b) in ((h[k], t[k]), (nh[k], nt[k])):
                min_x = min(min_x, float(np.abs(sign_args(kind, ent, rel, w, a, b, r[k])).min()))
    return {"slack": float(slack.min()), "min_abs_x": float(min_x), "active": int(active.sum()),
            "touches": touch_counts(ds, si, sj, side, active)}


def assert_preconditions(pre, l1, where=""):
    """Asserted, never skipped on; nothing is left out of the comparison."""
    assert pre["slack"] >= MIN_SLACK, (where, "hinge slack", pre["slack"])
    if l1:
        assert pre["min_abs_x"] >= MIN_ABS_X, (where, "min |x|", pre["min_abs_x"])
    assert pre["active"] > 0, (where, "no active sample: the batch moves nothing")


# ------------------------------------------------------------ comparator

def compare_tables(got, ref):
    """{table: (largest |got - ref|, row index)} for "ent", "rel", "w"; the row is
    the index without the last axis ((relation, matrix row) for TransR's w)."""
    out = {}
    for name, g, r in zip(("ent", "rel", "w"), got, ref):
        if r is None:
            assert g is None, name
            continue
        d = np.abs(np.asarray(g, np.float64) - np.asarray(r, np.float64))
        assert d.shape == np.shape(r), (name, d.shape)
        rows = d.reshape(-1, d.shape[-1]).max(1)
        k = int(rows.argmax())
        out[name] = (float(rows[k]), tuple(int(i) for i in np.unravel_index(k, d.shape[:-1])))
    return out


def rows_over(got, ref, bar):
    """Every (table, row) whose largest |got - ref| exceeds `bar`."""
    out = []
    for name, g, r in zip(("ent", "rel", "w"), got, ref):
        if r is None:
            continue
        d = np.abs(np.asarray(g, np.float64) - np.asarray(r, np.float64))
        rows = d.reshape(-1, d.shape[-1]).max(1)
        out += [(name, tuple(int(i) for i in np.unravel_index(k, d.shape[:-1]))) for k in np.nonzero(rows > bar)[0]]
    return out


# ------------------------------------------------------------ the reference's batch

def oracle_for(case, ds):
    m = orc.Model(case.model, case.dim, ds.num_entities, ds.num_relations, rate=RATE, margin=MARGIN, method=1,
                  distance=case.distance, batches=case.batches, transr_compat=False)
    m.set_triples(ds.train)
    return m


def reference_step(case, m, ds, tabs, si, sj, side):
    """One batch of the FP64 reference from `tabs`: the C oracle for ORDERED, the
    numpy model of the PARALLEL schedule otherwise.  Returns (loss, active, tables
    after, preconditions)."""
    if case.schedule == "ordered":
        m.set_tables(*tabs)
        pre = batch_preconditions(m, ds, si, sj, side, case.l1)
        loss, act = m.train_replay(si, sj, side)
        return loss, act, m.tables(), pre
    ent, rel, w = (None if t is None else np.array(t, np.float64) for t in tabs)
    B, rec = len(si), {}
    if case.model == "E":
        loss, act = transe_parallel_batches(ent, rel, ds.train, si, sj, side, B, 1, rate=RATE, margin=MARGIN,
                                            l1=case.l1, record=rec)
    elif case.model == "H":
        loss, act = transh_parallel_batches(ent, rel, w, ds.train, si, sj, side, B, 1, rate=RATE, margin=MARGIN,
                                            record=rec)
    else:
        loss, act = transr_parallel_batches(ent, rel, w, ds.train, si, sj, side, B, 1, rate=RATE, margin=MARGIN,
                                            l1=case.l1, compat=False, cons="chunk1", sub=resolved_sub(case),
                                            record=rec)
    mx = rec["min_abs_x"][0] if case.l1 else np.zeros(0)
    pre = {"slack": float(rec["slack"][0].min()), "min_abs_x": float(mx.min()) if mx.size else np.inf,
           "active": int(act), "touches": touch_counts(ds, si, sj, side, rec["active"][0])}
    return loss, act, (ent, rel, w), pre


# ------------------------------------------------------------ lock-step driver

def make_engine(case, ds):
    """One FP32 context for the case, initialised as the reference's trainer
    (TransR: seeded with its own init draws)."""
    from kb2e_amd.engine import Engine
    eng = Engine(case.model, case.dim, ds.num_entities, ds.num_relations, rate=RATE, margin=MARGIN, method=1,
                 distance=case.distance, batches=case.batches, seed=case.seed, precision=32, transr_compat=False,
                 schedule=case.schedule, sub_batches=case.sub)
    eng.upload_triples(ds.train)
    e0, r0, _ = eng.init_params()
    if case.model == "R":
        eng.transr_seed(e0, r0)
    assert eng.cfg.sub_batches == resolved_sub(case), (eng.cfg.sub_batches, resolved_sub(case))
    return eng


@dataclass
class BatchResult:
    batch: int
    pre: dict
    ref: tuple           # (loss, active) of the reference
    got: tuple           # (loss, active) of the engine (the reference's own without one)
    diffs: dict          # compare_tables(engine after, reference after)
    moved: float = 0.0   # largest |reference after - before|: what a missed update would cost
    tables: tuple = field(default=(), repr=False)  # (before, reference after, got after)


def lockstep(case, engine=None, nb=NB, ds=None):
    """The batches of a case in lock step, yielding a BatchResult each.  Before
    every batch the reference takes the engine's tables (float-representable),
    draws the batch's samples from its glibc stream -- the engine keeps the same
    stream (orc.srand(seed) / kb2e_config.seed, the same init draws) and so draws
    the same samples -- and both run the batch.  Without an engine the reference
    runs alone, its tables rounded to float between batches: the CPU-checkable
    half (preconditions) of the same case."""
    ds = ds or dataset()
    m = oracle_for(case, ds)
    orc.srand(case.seed)
    m.prep_train()
    B = m.batch_size()
    if engine is None:
        if case.model == "R":
            e0, r0, _ = m.tables()
            m.transr_seed(e0, r0)
        tabs = tuple(round32(t) for t in m.tables())
    else:
        tabs = engine.download_params()
    for b in range(nb):
        assert all(float_representable(t) for t in tabs), "tables are not float-representable"
        si, sj, side = m.sample_stream(B)
        lo, ao, ref_tabs, pre = reference_step(case, m, ds, tabs, si, sj, side)
        if engine is None:
            lg, ag, new = lo, ao, tuple(round32(t) for t in ref_tabs)
        else:
            engine.train_batches(1)
            lg, ag = engine.take_stats()
            new = engine.download_params()
        moved = max(float(np.abs(a - c).max()) for a, c in zip(ref_tabs, tabs) if a is not None)
        yield BatchResult(b, pre, (lo, ao), (lg, ag), compare_tables(new, ref_tabs), moved, (tabs, ref_tabs, new))
        tabs = new


def check_batch(case, res):
    """Preconditions, then the bars: equal active counts, batch loss within
    LOSS_RTOL, every table element within the case's bar."""
    where = (case.id, res.batch)
    assert_preconditions(res.pre, case.l1, where)
    assert res.got[1] == res.ref[1], (where, "active", res.got[1], res.ref[1])
    assert abs(res.got[0] - res.ref[0]) <= LOSS_RTOL * abs(res.ref[0]), (where, "loss", res.got[0], res.ref[0])
    assert case.atol <= ELEM_ATOL_CEIL
    worst = max(v[0] for v in res.diffs.values())
    assert worst <= case.atol, (where, "tables", res.diffs)
    return worst


# ------------------------------------------------------------ seed search (by hand)

def find_seeds(case, seeds=range(1, 33), spare=2.0, first=True):
    """Seeds at which the reference alone meets the guards over the case's batches
    with a factor `spare` in hand: [(seed, min slack, min |x|)]."""
    ds, out = dataset(), []
    for s in seeds:
        slack = mx = np.inf
        for res in lockstep(replace(case, seed=s), ds=ds):
            slack = min(slack, res.pre["slack"])
            mx = min(mx, res.pre["min_abs_x"])
            if slack < spare * MIN_SLACK or (case.l1 and mx < spare * MIN_ABS_X):
                break  # (most seeds fail in the first batch)
        else:
            out.append((s, slack, mx))
            if first:
                break
    return out


if __name__ == "__main__":
    only = sys.argv[1:]
    for c in ORDERED_CASES + PARALLEL_CASES:
        if only and not any(o in c.id for o in only):
            continue
        print(c.id, find_seeds(c), flush=True)
