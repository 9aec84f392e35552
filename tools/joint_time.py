#!/usr/bin/env python3
"""Time the conjunctive queries on the FB15k-shaped synthetic set.

Per model, `--queries` queries of `--m` patterns each, built from the test
triples (an entity's mentions first, random patterns to fill up), are answered
with kb2e_predict_joint, and the same patterns, one query each, with
kb2e_predict.  One warm-up call, then `--repeats` timed ones; per kernel family
the device time of each repeat (kb2e_profile_query: HIP events on the engine's
stream).  One JSON line per model: the joint_* spans, predict's spans over the
same rows, and the combine kernel's bytes/s against its algorithmic
8 (m + 1) |E| nq bytes.  With --identify, also linkpred.entity_identification
after a TransE training run.

    python tools/joint_time.py [--models E:100,R:50] [--queries 1000] [--m 3] [--repeats 5]
    python tools/joint_time.py --identify [--epochs 1000] [--dim 100]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from kb2e_amd import data, linkpred  # noqa: E402
from kb2e_amd.engine import Engine  # noqa: E402

JOINT = ("joint_score", "joint_combine", "joint_mask", "joint_select")
PREDICT = ("predict_score", "predict_mask", "predict_select")


def spans(eng, call, families, repeats):
    """{family: [ms per repeat]} of `repeats` calls after one warm-up."""
    call()
    out = {f: [] for f in families}
    for _ in range(repeats):
        eng.profile(True)  # (clears the timers)
        call()
        for f in families:
            out[f].append(eng.profile_query(f)[0])
    eng.profile(False)
    return out


def summary(ms):
    return {f: {"min_ms": min(v), "median_ms": statistics.median(v)} for f, v in ms.items()}


def time_model(model, dim, ds, nq, m, repeats, k):
    rng = np.random.default_rng(0)
    _, patterns = linkpred.identification_queries(ds.test, m)
    queries = [p[:m] for p in patterns[:nq]]
    while len(queries) < nq:
        queries.append(np.stack([rng.integers(0, ds.num_entities, m), rng.integers(0, ds.num_relations, m),
                                 rng.integers(0, 2, m)], axis=1).astype(np.int32))
    rows = np.concatenate(queries)
    filt = np.concatenate([ds.train, ds.valid, ds.test]).astype(np.int32)
    eng = Engine(model, dim, ds.num_entities, ds.num_relations, seed=7, transr_compat=False)
    try:
        eng.upload_triples(ds.train)
        ent, rel, _ = eng.init_params()
        if model == "R":
            eng.transr_seed(ent, rel)
        joint = spans(eng, lambda: eng.predict_joint(queries, k, filt), JOINT, repeats)
        projections = eng.counter("joint_projections")
        single = spans(eng, lambda: eng.predict(rows[:, 0], rows[:, 1], rows[:, 2], k, filt), PREDICT, repeats)
        combine_bytes = 8 * (m + 1) * ds.num_entities * nq
        best = min(joint["joint_combine"])
        print(json.dumps({"model": model, "dim": dim, "entities": ds.num_entities, "queries": nq, "m": m, "k": k,
                          "rows": int(len(rows)), "distinct_relations": int(len(np.unique(rows[:, 1]))),
                          "joint_projections": projections,
                          "repeats": repeats, "joint": summary(joint), "predict_same_rows": summary(single),
                          "combine_bytes": combine_bytes,
                          "combine_bytes_per_s": combine_bytes / (best * 1e-3) if best else None}), flush=True)
    finally:
        eng.close()


def identify(ds, dim, epochs, constraints):
    eng = Engine("E", dim, ds.num_entities, ds.num_relations, rate=0.001, batches=100, seed=7, schedule="parallel")
    try:
        eng.upload_triples(ds.train)
        eng.init_params()
        eng.train_batches(epochs * 100)
        eng.synchronize()
        res = linkpred.entity_identification(eng, ds, constraints)
        print(json.dumps({"model": "E", "dim": dim, "epochs": epochs, "schedule": "parallel",
                          "identification": {str(m): v for m, v in res.items()}}), flush=True)
    finally:
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="E:100,R:50")
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--m", type=int, default=3)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--identify", action="store_true")
    ap.add_argument("--epochs", type=int, default=1000)
    ap.add_argument("--dim", type=int, default=100)
    args = ap.parse_args()
    ds = data.synthetic("fb15k", seed=0)
    if args.identify:
        identify(ds, args.dim, args.epochs, (1, 2, 3))
        return
    for spec in args.models.split(","):
        model, dim = spec.split(":")
        time_model(model, int(dim), ds, args.queries, args.m, args.repeats, args.k)


if __name__ == "__main__":
    main()
