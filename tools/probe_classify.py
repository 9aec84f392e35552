#!/usr/bin/env python3
"""GPU probe: what do the device sort and sweep of kb2e_fit_thresholds cost on
top of the scoring that existed before, and against the host alternative?

On the FB15k-shaped synthetic set with TransE n=50 (a few PARALLEL epochs, so the
energies are a trained model's): the valid triples plus their generated
negatives are fitted, the test split (plus negatives) is classified.  After a
warm-up of every call, alternating in one process:

* (a) Engine.fit_thresholds against Engine.score over the same triples (score is
  the part that existed; the difference is what sort and sweep add, less the
  energy download that score alone pays);
* (b) Engine.fit_thresholds against the host route a user had: Engine.score,
  np.lexsort on (energy, relation), a numpy sweep per relation (the same rule;
  its result is compared with the device's);
* (d) Engine.corrupt against a numpy restatement of the documented rule (on the
  first --corrupt-check triples: it is a Python loop; results compared).

Host clock around calls that end in a stream synchronise; median and range over
the repeats.  (c) One more fit / classify / corrupt runs with the engine's
profile on for the classify_* kernel families.  (e) The valid and test accuracy.
Prints one JSON line.

  python tools/probe_classify.py --repeats 5
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from kb2e_amd import data, linkpred  # noqa: E402
from kb2e_amd.engine import Engine  # noqa: E402

M64 = (1 << 64) - 1


def _mix(z):
    z &= M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z


def host_corrupt(triples, kset, pools, ne, seed):
    """include/kb2e_engine.h kb2e_corrupt_triples (side 2, constrained), restated."""
    state = _mix(seed)
    out = np.full((len(triples), 3), -1, np.int32)
    for i, (h, t, r) in enumerate(triples.tolist()):
        slot = _mix(state + (i << 7)) >> 63
        old = t if slot else h
        pool = pools[slot].get(r, [])
        out[i, 2] = r
        for a in range(1 if pool else 33, 65):
            u = _mix(state + (i << 7) + a)
            x = pool[u % len(pool)] if a <= 32 else u % ne
            if x == old or ((h, x, r) if slot else (x, t, r)) in kset:
                continue
            out[i, 0], out[i, 1] = (h, x) if slot else (x, t)
            break
    return out


def host_fit(energy, labels, rel, nr):
    """np.lexsort + a sweep: the rule of kb2e_fit_thresholds on the host."""
    def sweep(e, lab):  # e ascending
        g = 2 * np.cumsum(lab, dtype=np.int64) - np.arange(1, len(e) + 1)
        g[:-1][e[1:] == e[:-1]] = np.iinfo(np.int64).min  # a cut inside a run of equal energies is none
        k = int(np.argmax(g))
        neg = len(e) - int(lab.sum())
        return (e[k], neg + int(g[k])) if g[k] > 0 else (-np.inf, neg)
    order = np.lexsort((energy, rel))
    e, lab, r = energy[order], labels[order].astype(np.int64), rel[order]
    go = np.argsort(energy, kind="stable")
    gthr, gcorrect = sweep(energy[go], labels[go].astype(np.int64))
    thr = np.full(nr, gthr)
    counts = np.zeros((nr, 3), np.int64)
    starts = np.flatnonzero(np.r_[True, r[1:] != r[:-1]])
    ends = np.r_[starts[1:], len(r)]
    for s0, s1 in zip(starts, ends):
        d, c = sweep(e[s0:s1], lab[s0:s1])
        p = int(lab[s0:s1].sum())
        thr[r[s0]], counts[r[s0]] = d, (p, s1 - s0 - p, c)
    return thr, counts, gthr, gcorrect


def stats(xs):
    xs = sorted(xs)
    return {"median_ms": 1e3 * xs[len(xs) // 2], "min_ms": 1e3 * xs[0], "max_ms": 1e3 * xs[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="fb15k")
    ap.add_argument("--dim", type=int, default=50)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--corrupt-check", type=int, default=5000, help="triples of the numpy restatement")
    args = ap.parse_args()
    ds = data.synthetic(args.shape, seed=0)
    known = np.concatenate([ds.train, ds.valid, ds.test])
    eng = Engine("E", args.dim, ds.num_entities, ds.num_relations, rate=0.01, seed=7, schedule="parallel")
    eng.upload_triples(ds.train)
    eng.init_params()
    for _ in range(args.epochs):
        eng.train_epoch()

    def timed(f):
        t0 = time.perf_counter()
        out = f()
        return time.perf_counter() - t0, out

    _, (neg, failed) = timed(lambda: eng.corrupt(ds.valid, known, seed=0))  # (warm-up of corrupt too)
    neg = neg[neg[:, 0] >= 0]
    triples = np.concatenate([ds.valid, neg]).astype(np.int32)
    labels = np.concatenate([np.ones(len(ds.valid), np.uint8), np.zeros(len(neg), np.uint8)])
    rel = triples[:, 2]

    def host_route():
        return host_fit(eng.score(triples), labels, rel, ds.num_relations)

    dev = eng.fit_thresholds(triples, labels)  # warm-up; and the two routes agree
    host = host_route()
    same = bool(np.array_equal(dev[0], host[0]) and np.array_equal(dev[1], host[1]) and dev[2:] == host[2:])
    t_fit, t_score, t_host, t_corrupt = [], [], [], []
    for _ in range(args.repeats):
        t_fit.append(timed(lambda: eng.fit_thresholds(triples, labels))[0])
        t_score.append(timed(lambda: eng.score(triples))[0])
        t_host.append(timed(host_route)[0])
        t_corrupt.append(timed(lambda: eng.corrupt(ds.valid, known, seed=0))[0])

    # (d) the restatement on a prefix (the stream depends on the row index alone, so a prefix compares)
    m = min(args.corrupt_check, len(ds.valid))
    t0 = time.perf_counter()
    kset = set(map(tuple, known.tolist()))
    pools = ({}, {})
    for slot in (0, 1):
        pairs = np.unique(known[:, [2, slot]], axis=0)
        for r, x in pairs.tolist():
            pools[slot].setdefault(r, []).append(x)
    t_build = time.perf_counter() - t0
    t_np, ref = timed(lambda: host_corrupt(ds.valid[:m], kset, pools, ds.num_entities, 0))
    dneg, _ = eng.corrupt(ds.valid, known, seed=0)
    corrupt_same = bool(np.array_equal(dneg[:m], ref))

    # (c) the kernel families
    eng.profile(True)
    eng.fit_thresholds(triples, labels)
    eng.classify(triples, dev[0])
    eng.corrupt(ds.valid, known, seed=0)
    prof = {k: dict(zip(("ms", "launches"), eng.profile_query(k)))
            for k in ("classify_score", "classify_sort", "classify_fit", "classify_corrupt")}
    eng.profile(False)

    res = linkpred.triple_classification(eng, ds, seed=0)
    per_rel = np.bincount(rel, minlength=ds.num_relations)
    print(json.dumps({
        "shape": args.shape, "dim": args.dim, "epochs": args.epochs, "fitted_triples": int(len(triples)),
        "relations_fitted": int((per_rel > 0).sum()), "hottest_relation": int(per_rel.max()),
        "fit_thresholds": stats(t_fit), "score": stats(t_score), "host_score_lexsort_sweep": stats(t_host),
        "device_equals_host": same, "corrupt": stats(t_corrupt), "corrupt_triples": int(len(ds.valid)),
        "corrupt_failed": int(failed), "numpy_corrupt": {"triples": m, "ms": 1e3 * t_np, "build_ms": 1e3 * t_build},
        "corrupt_equals_numpy": corrupt_same, "profile": prof,
        "valid_accuracy": res["valid"]["accuracy"], "test_accuracy": res["test"]["accuracy"],
        "test_triples": res["test"]["count"], "test_failed": res["test"]["failed"]}))


if __name__ == "__main__":
    main()
