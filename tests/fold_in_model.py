"""Entity fold-in in numpy FP64 (tests/ only; a plain helper module like
fp32_step.py, not a conftest): a restatement of the frozen step of
include/kb2e_engine.h (kb2e_fold_in_entities), every sum serial
(np.cumsum(...)[-1]) as the reference's loops are.

  fold_in        rows, losses and counts of one call, plus how near the run came
                 to a decision: the smallest hinge slack |E+ + margin - E-|, the
                 smallest |g_k| of an L1 sign argument and the smallest distance
                 of a coupling-loop test from its threshold (0.1, 1)
  random_case    the random tables and examples the GPU parity tests use
  CASES          the committed parity cases; their seeds were searched by hand
                 (`python tests/fold_in_model.py`) so that every guard holds on
                 the model alone (tests/test_fold_in_model.py re-checks that)

A wave sum moves an energy by ~1e-13, so with every guard >= GUARD no decision
of the device can differ from the model's.
"""
from __future__ import annotations

import functools
import os
import sys
from dataclasses import dataclass, field

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:  # run by hand (the seed search); under pytest conftest.py did this
    sys.path.insert(0, ROOT)

M64 = (1 << 64) - 1
DRAWS = 32
DEFAULT_SWEEPS = 10000
GUARD = 1e-7


def mix(z):
    """SplitMix64's finaliser (kb2e_corrupt_triples' stream)."""
    z &= M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z


def draw(state, p, count, i, a):
    return mix(state + (((p * count + i) << 7) & M64) + a)


def ssum(a):
    """The serial sum of a 1-d array, in index order."""
    return float(np.cumsum(a)[-1]) if len(a) else 0.0


def colsum(W, v):
    """p_k = sum_j W[j][k] v[j], j ascending."""
    return np.cumsum(W * v[:, None], axis=0)[-1]


def rowsum(W, g):
    """s_j = sum_k g[k] W[j][k], k ascending."""
    return np.cumsum(W * g[None, :], axis=1)[:, -1]


@dataclass
class Result:
    rows: np.ndarray            # [nfree, n] as stored (rounded to float once for precision 32)
    loss: np.ndarray            # [nfree, 2] first pass, last pass
    counts: np.ndarray          # [nfree, 3] active, failed, capped
    min_slack: float = np.inf   # hinge
    min_abs_g: float = np.inf   # L1 sign arguments of active samples
    min_loop_gap: float = np.inf
    inactive: int = 0
    sweeps: list = field(default_factory=list)  # sweeps of every coupling loop that ran at least once
    trace: list = field(default_factory=list)   # per active sample (with trace=True): see fold_in

    def guards(self):
        return min(self.min_slack, self.min_abs_g, self.min_loop_gap)


def fold_in(model, ent, rel, w, free, examples, known=None, *, lr, margin, l1=True, epochs, seed=0, side=2,
            max_sweeps=0, rows=None, precision=64, trace=False):
    """model "E" / "H" / "R"; ent, rel, w: FP64 arrays (FP32 tables widened); free [nfree]; examples and known
    [., 3] rows (head, tail, relation).  trace=True records, per active sample, a dict with the free entity f,
    the positive and the corrupted triple, both energies, the row before and after and, per processed triple,
    the row after its update and normalisation (before the coupling loop) and the loop's sweeps."""
    ent = np.asarray(ent, np.float64)
    ne, n = ent.shape
    free = [int(f) for f in free]
    examples = np.asarray(examples, np.int64).reshape(-1, 3)
    count = len(examples)
    l1 = True if model == "H" else bool(l1)
    cap = DEFAULT_SWEEPS if max_sweeps == 0 else max_sweeps
    is_free = set(free)
    kset = set(map(tuple, np.asarray(known, np.int64).reshape(-1, 3).tolist())) if known is not None else set()
    kset |= set(map(tuple, examples.tolist()))
    state = mix(seed)
    res = Result(np.zeros((len(free), n)), np.zeros((len(free), 2)), np.zeros((len(free), 3), np.int64))

    def feature(row, r):
        if model == "E":
            return row
        if model == "H":
            return row - ssum(w[r] * row) * w[r]
        return colsum(w[r], row)

    groups = {f: [] for f in free}
    for i in range(count):
        groups[int(examples[i, 0]) if int(examples[i, 0]) in is_free else int(examples[i, 1])].append(i)

    for fi, f in enumerate(free):
        x = np.array(ent[f] if rows is None else np.asarray(rows, np.float64)[fi], np.float64)
        mine = groups[f]
        for p in range(epochs):
            lossp = 0.0
            for i in mine:
                h, t, r = (int(v) for v in examples[i])
                fslot = 0 if h == f else 1
                cslot = (draw(state, p, count, i, 0) >> 63) if side == 2 else side
                old = t if cslot else h
                got = -1
                for a in range(1, DRAWS + 1):
                    e = draw(state, p, count, i, a) % ne
                    if e in is_free or e == old or ((h, e, r) if cslot else (e, t, r)) in kset:
                        continue
                    got = e
                    break
                if got < 0:
                    res.counts[fi, 1] += 1
                    continue
                o = h if fslot else t
                fx, fo, fq = feature(x, r), feature(ent[o], r), feature(ent[got], r)
                ph, pt = (fo, fx) if fslot else (fx, fo)
                nh = fq if cslot == 0 else ph
                nt = fq if cslot == 1 else pt
                dpos, dneg = pt - ph - rel[r], nt - nh - rel[r]
                epos = ssum(np.abs(dpos) if l1 else dpos * dpos)
                eneg = ssum(np.abs(dneg) if l1 else dneg * dneg)
                res.min_slack = min(res.min_slack, abs(epos + margin - eneg))
                if not (epos + margin > eneg):
                    res.inactive += 1
                    continue
                lossp += margin + epos - eneg
                res.counts[fi, 0] += 1
                y = x.copy()
                tr = dict(f=f, pos=(h, t, r), neg=(got if cslot == 0 else h, got if cslot == 1 else t, r), epos=epos,
                          eneg=eneg, before=x.copy(), loops=[])
                for beta, d in ((-1.0, dpos), (1.0, dneg)):
                    if beta > 0 and cslot == fslot:
                        break  # the corrupted triple lost f
                    g = 2.0 * d
                    if l1:
                        res.min_abs_g = min(res.min_abs_g, float(np.min(np.abs(g))))
                        g = np.where(g > 0, 1.0, -1.0)
                    coef = beta * lr
                    if model != "R":
                        y = y + coef * g if fslot else y - coef * g
                        ln = np.sqrt(ssum(y * y))
                        if ln > 1:
                            y = y / ln
                    else:
                        terms = (coef * g)[None, :] * w[r]
                        y = np.cumsum(np.concatenate([y[:, None], terms if fslot else -terms], axis=1), axis=1)[:, -1]
                        y = y / np.sqrt(ssum(y * y))
                    if model == "E":
                        continue
                    sweeps = 0
                    entered = y.copy()
                    while True:
                        if model == "H":
                            test, thr = ssum(w[r] * y), 0.1
                        else:
                            q = colsum(w[r], y)
                            test, thr = ssum(q * q), 1.0
                        res.min_loop_gap = min(res.min_loop_gap, abs(test - thr))
                        if not test > thr:
                            break
                        if sweeps == cap:
                            res.counts[fi, 2] += 1
                            break
                        y = y - lr * w[r] if model == "H" else y - lr * rowsum(w[r], 2.0 * q)
                        sweeps += 1
                    if sweeps:
                        res.sweeps.append(sweeps)
                    tr["loops"].append((r, entered, sweeps, y.copy()))
                x = y
                if trace:
                    tr["after"] = x.copy()
                    res.trace.append(tr)
            if p == 0:
                res.loss[fi, 0] = lossp
            if p == epochs - 1:
                res.loss[fi, 1] = lossp
        res.rows[fi] = x.astype(np.float32).astype(np.float64) if precision == 32 else x
    return res


# ------------------------------------------------------------------ the parity cases

NE, NR, NFREE, PER_FREE = 40, 4, 5, 6


@dataclass(frozen=True)
class Case:
    model: str      # "E", "H", "R"
    l1: bool
    dim: int
    side: int
    seed: int       # of the tables and examples (np.random.default_rng) and of the call
    lr: float = 0.01
    margin: float = 1.0
    epochs: int = 3
    scale: float = 1.0   # of the frozen entity rows: spreads the energies so that some hinges are inactive
    wscale: float = 1.0  # TransH: length of the normals' component along the rows; TransR: of the matrices

    @property
    def id(self):
        return f"{self.model}{'L1' if self.l1 else 'L2'}-n{self.dim}-side{self.side}"


def random_case(c, ne=NE, nr=NR, nfree=NFREE, per_free=PER_FREE):
    """Tables, free entities (the last nfree ids), examples with the free entity in both slots, known triples."""
    rng = np.random.default_rng(c.seed)
    n = c.dim
    ent = rng.normal(size=(ne, n))
    ent *= c.scale / np.linalg.norm(ent, axis=1, keepdims=True)
    rel = rng.normal(size=(nr, n))
    rel *= 0.5 / np.linalg.norm(rel, axis=1, keepdims=True)
    w = None
    if c.model == "H":
        w = rng.normal(size=(nr, n))
        w /= np.linalg.norm(w, axis=1, keepdims=True)
    elif c.model == "R":
        w = np.stack([np.eye(n)] * nr) * c.wscale + rng.normal(size=(nr, n, n)) * (0.3 / np.sqrt(n))
    free = np.arange(ne - nfree, ne, dtype=np.int32)
    ex = []
    for f in free:
        for k in range(per_free):
            o, r = int(rng.integers(0, ne - nfree)), int(rng.integers(0, nr))
            ex.append((f, o, r) if k % 2 == 0 else (o, f, r))
    ex = np.array(ex, np.int32)
    ex = ex[rng.permutation(len(ex))]
    known = np.stack([rng.integers(0, ne - nfree, 60), rng.integers(0, ne - nfree, 60), rng.integers(0, nr, 60)],
                     axis=1).astype(np.int32)
    if c.model == "H":  # free rows that start along the normal, so that the orthogonality loop has work
        ent[free] += c.wscale * w[rng.integers(0, nr, nfree)]
    return ent, rel, w, free, ex, known


def run_case(c, **kw):
    ent, rel, w, free, ex, known = random_case(c)
    return fold_in(c.model, ent, rel, w, free, ex, known, lr=c.lr, margin=c.margin, l1=c.l1, epochs=c.epochs,
                   seed=c.seed, side=c.side, **kw)


def case_ok(c, res):
    """What a committed case must show on the model alone: the guards, an inactive and an active hinge, and for
    TransH / TransR a coupling loop of at least two sweeps."""
    return (res.guards() >= GUARD and res.inactive >= 1 and res.counts[:, 0].sum() >= 1 and
            (c.model == "E" or (res.sweeps and max(res.sweeps) >= 2)))


def _shape(model, l1, dim, side):
    if model == "E":
        return dict(scale=0.9)
    if model == "H":
        return dict(scale=0.9, wscale=0.6)
    return dict(scale=0.9, wscale=1.02, lr=0.01)


def find_seeds(limit=400):
    """Print a CASES table whose seeds meet case_ok (run by hand)."""
    for model, l1 in (("E", True), ("E", False), ("H", True), ("R", True), ("R", False)):
        for dim in (8, 20):
            for side in (0, 1, 2):
                for seed in range(1, limit):
                    c = Case(model, l1, dim, side, seed, **_shape(model, l1, dim, side))
                    res = run_case(c)
                    if case_ok(c, res):
                        print(f"    {c!r},  # guards {res.guards():.1e}, inactive {res.inactive}, "
                              f"max sweeps {max(res.sweeps) if res.sweeps else 0}")
                        break
                else:
                    print(f"    # no seed below {limit} for {model} l1={l1} n={dim} side={side}")


# Seed 1 meets case_ok for every combination (find_seeds prints the table with the guards it measured:
# between 2.8e-05 and 7.8e-02, inactive hinges 2..19, longest loops 47..62 sweeps for TransH and 6..8 for TransR).
CASES = [Case(model, l1, dim, side, 1, **_shape(model, l1, dim, side))
         for model, l1 in (("E", True), ("E", False), ("H", True), ("R", True), ("R", False))
         for dim in (8, 20) for side in (0, 1, 2)]

# Lane and staging boundaries: one lane chunk exactly full (64), one element into the second (65), the third
# chunk in use and the widest staged TransR matrices (130), past the LDS form (150).
BOUNDARY = [Case(model, l1, dim, 2, 1, epochs=2, **_shape(model, l1, dim, 2))
            for dim in (64, 65, 130) for model, l1 in (("E", True), ("E", False), ("H", True), ("R", True), ("R", False))]
BOUNDARY_L2 = [Case("R", True, 20, 2, 1, **_shape("R", True, 20, 2)),           # with KB2E_FOLD_W_L2=1
               Case("R", False, 150, 2, 1, epochs=2, **_shape("R", False, 150, 2))]


# ------------------------------------------------------------------ the other GPU inputs
# Each returns ((model, ent, rel, w, free, examples, known, keyword arguments), the model's Result), computed once.

def _special(model, l1, dim, ne, nr, free, ex, known, seed, epochs, side=2, lr=0.01, margin=1.0):
    c = Case(model, l1, dim, side, seed, lr=lr, margin=margin, epochs=epochs, **_shape(model, l1, dim, side))
    ent, rel, w, _, _, _ = random_case(c, ne=ne, nr=nr, nfree=len(free), per_free=0)
    kw = dict(lr=lr, margin=margin, l1=l1, epochs=epochs, seed=seed, side=side)
    return (model, ent, rel, w, free, ex, known, kw), fold_in(model, ent, rel, w, free, ex, known, **kw)


@functools.lru_cache(None)
def hub():
    """One free entity with 3,000 examples, two passes, TransE n = 20."""
    rng = np.random.default_rng(11)
    ne, nr = 2000, 4
    f = ne - 1
    o, r = rng.integers(0, ne - 1, 3000), rng.integers(0, nr, 3000)
    ex = np.where((np.arange(3000) % 2 == 0)[:, None], np.stack([np.full(3000, f), o, r], 1),
                  np.stack([o, np.full(3000, f), r], 1)).astype(np.int32)
    return _special("E", True, 20, ne, nr, np.array([f], np.int32), ex, None, 11, 2)


@functools.lru_cache(None)
def many(seed=19):  # (searched by hand: guards 4.5e-06)
    """2,000 free entities with one or two examples each: more units than a card holds resident waves for."""
    rng = np.random.default_rng(seed)
    ne, nr, nfree = 2600, 4, 2000
    free = np.arange(ne - nfree, ne, dtype=np.int32)
    ex = []
    for f in free:
        for k in range(int(rng.integers(1, 3))):
            o, r = int(rng.integers(0, ne - nfree)), int(rng.integers(0, nr))
            ex.append((f, o, r) if (f + k) % 2 == 0 else (o, f, r))
    ex = np.array(ex, np.int32)
    return _special("H", True, 20, ne, nr, free[rng.permutation(nfree)], ex[rng.permutation(len(ex))], None, seed, 2)


def _rejections(spare):
    """12 entities, 2 of them free; the tail of (f, o, r) / the head of (o, f, r) is corrupted and `known` holds
    the triple of every legal replacement but `spare` of them."""
    ne, nr = 12, 2
    free = np.array([10, 11], np.int32)
    ex = np.array([(10, 0, 0), (1, 10, 1), (11, 2, 1), (3, 11, 0), (10, 4, 1), (5, 11, 1)], np.int32)
    known = []
    for h, t, r in ex.tolist():
        legal = [e for e in range(10) if e != (t if h >= 10 else h)]
        for e in legal[spare:]:
            known.append((h, e, r) if h >= 10 else (e, t, r))
    known = np.array(known, np.int32)
    return ne, nr, free, ex, known


@functools.lru_cache(None)
def one_candidate():
    ne, nr, free, ex, known = _rejections(1)
    # side 2: a sample whose coin picks the slot of the frozen entity has exactly one legal candidate among
    # the 12 entities (32 draws miss it now and then: `failed`), the other kind has nine
    return _special("E", True, 8, ne, nr, free, ex, known, 5, 40)


@functools.lru_cache(None)
def complete_graph():
    ne, nr, free, ex, _ = _rejections(0)
    known = np.array([(h, t, r) for h in range(ne) for t in range(ne) for r in range(nr)], np.int32)
    return _special("E", True, 8, ne, nr, free, ex, known, 5, 3)


SPECIAL = {"hub": hub, "many": many, "one_candidate": one_candidate}


if __name__ == "__main__":
    find_seeds()
