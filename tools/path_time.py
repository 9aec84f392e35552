#!/usr/bin/env python3
"""Time the path queries on the FB15k-shaped synthetic set.

Per model and beam B, `--rows` // B queries of `--hops` hops
(linkpred.path_query_set: a train walk that ends in a test triple) are answered
with kb2e_predict_path, and in the same process kb2e_predict answers nq * B
one-sided rows of the relations and sides of the queries' second hops -- the
rows the hop kernel scores without writing them down.  One warm-up call, then
`--repeats` timed ones; per kernel family the device time of each repeat
(kb2e_profile_query: HIP events on the engine's stream).  One JSON line per
model and beam: the path_* spans, predict's spans, and the time per frontier
row of path_hop against predict_score.  With --evaluate, also
linkpred.path_evaluation after a TransE training run.

    python tools/path_time.py [--models E:100,R:50] [--beams 64,1024] [--rows 65536] [--hops 2] [--repeats 5]
    python tools/path_time.py --evaluate [--epochs 1000] [--dim 100] [--beam 64] [--limit 2000]
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

PATH = ("path_score", "path_hop", "path_select", "path_mask")
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


def time_model(model, dim, ds, beams, rows, hops, repeats, k):
    filt = np.concatenate([ds.train, ds.valid, ds.test]).astype(np.int32)
    all_anchors, all_paths, _ = linkpred.path_query_set(ds, hops, seed=0)
    eng = Engine(model, dim, ds.num_entities, ds.num_relations, seed=7, transr_compat=False)
    try:
        eng.upload_triples(ds.train)
        ent, rel, _ = eng.init_params()
        if model == "R":
            eng.transr_seed(ent, rel)
        for beam in beams:
            nq = max(1, rows // beam)
            anchors, paths = all_anchors[:nq], all_paths[:nq]
            path = spans(eng, lambda: eng.predict_path(anchors, paths, k, filt, beam=beam), PATH, repeats)
            counters = {c: eng.counter(c) for c in ("path_chunks", "path_hops", "path_projections")}
            # the frontier rows of the second hops as one-sided queries: the same relations and sides, B rows each
            rng = np.random.default_rng(1)
            hop2 = np.array([p[1] for p in paths], np.int32)
            qr, qs = np.repeat(hop2[:, 0], beam), np.repeat(hop2[:, 1], beam)
            qe = rng.integers(0, ds.num_entities, len(qr)).astype(np.int32)
            single = spans(eng, lambda: eng.predict(qe, qr, qs, k, filt), PREDICT, repeats)
            hop_rows = sum(len(p) - 1 for p in paths) * beam
            per_hop = min(path["path_hop"]) / hop_rows
            per_score = min(single["predict_score"]) / len(qr)
            print(json.dumps({"model": model, "dim": dim, "entities": ds.num_entities, "queries": int(nq), "hops": hops,
                              "beam": beam, "k": k, "repeats": repeats, **counters,
                              "distinct_hop2_relations": int(len(np.unique(hop2[:, 0]))),
                              "path": summary(path), "predict_same_rows": summary(single),
                              "frontier_rows": int(hop_rows), "predict_rows": int(len(qr)),
                              "path_hop_us_per_row": per_hop * 1e3, "predict_score_us_per_row": per_score * 1e3,
                              "ratio": per_hop / per_score}), flush=True)
    finally:
        eng.close()


def evaluate(ds, dim, epochs, beam, limit):
    eng = Engine("E", dim, ds.num_entities, ds.num_relations, rate=0.001, batches=100, seed=7, schedule="parallel")
    try:
        eng.upload_triples(ds.train)
        eng.init_params()
        eng.train_batches(epochs * 100)
        eng.synchronize()
        res = linkpred.path_evaluation(eng, ds, (1, 2, 3), beam=beam, seed=0, limit=limit)
        exact = linkpred.path_evaluation(eng, ds, (2,), beam=0, seed=0, limit=limit)
        print(json.dumps({"model": "E", "dim": dim, "epochs": epochs, "schedule": "parallel", "beam": beam, "limit": limit,
                          "paths": {str(m): v for m, v in res.items()}, "exact": {"2": exact[2]}}), flush=True)
    finally:
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="E:100,R:50")
    ap.add_argument("--beams", default="64,1024")
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--hops", type=int, default=2)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--evaluate", action="store_true")
    ap.add_argument("--epochs", type=int, default=1000)
    ap.add_argument("--dim", type=int, default=100)
    ap.add_argument("--beam", type=int, default=64)
    ap.add_argument("--limit", type=int, default=2000)
    args = ap.parse_args()
    ds = data.synthetic("fb15k", seed=0)
    if args.evaluate:
        evaluate(ds, args.dim, args.epochs, args.beam, args.limit)
        return
    for spec in args.models.split(","):
        model, dim = spec.split(":")
        time_model(model, int(dim), ds, [int(b) for b in args.beams.split(",")], args.rows, args.hops, args.repeats,
                   args.k)


if __name__ == "__main__":
    main()
