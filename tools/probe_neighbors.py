#!/usr/bin/env python3
"""GPU probe: what does kb2e_neighbors cost against the route a caller had
before it -- kb2e_predict over every entity on a copy of the model whose
relation table is zero, with the entity itself dropped on the host?

On the FB15k-shaped synthetic set (14,951 entities) with TransE at --dim after
--epochs PARALLEL epochs, the entity-space graph of all entities, k = --topk;
after a warm-up of both routes, alternating in one process:

* Engine.knn_graph(k);
* the composed route: a second engine holds the trained entity table and a
  zeroed relation table; Engine.predict of (e, ?, 0) for every entity e with
  k + 1, then numpy drops e from its own row and keeps k.

Host clock around calls that end in a stream synchronise; median and range over
the repeats.  One more Engine.knn_graph call runs with the engine's profile on
for the two neighbors_* kernel families, and the counters of that call are
reported.  Eight rows are checked for equality between the routes.  A TransR
line on the same data times the graph of a relation's space alone.  Last,
linkpred.duplicate_detection's recalls for --twins planted twins against the
random baseline: a measurement of the model, not a bar.  Prints one JSON line
each.

  python tools/probe_neighbors.py --repeats 5
  python tools/probe_neighbors.py --duplicates-only --epochs 300
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


def stat(v):
    return {"median_s": round(float(np.median(v)), 6), "min_s": round(min(v), 6), "max_s": round(max(v), 6)}


def trained(model, ds, args):
    eng = Engine(model, args.dim, ds.num_entities, ds.num_relations, rate=0.01, seed=7, schedule="parallel")
    eng.upload_triples(ds.train)
    ent, rel, _ = eng.init_params()
    if model == "R":
        eng.transr_seed(ent, rel)
    for _ in range(args.epochs):
        eng.train_epoch()
    eng.synchronize()
    return eng


def composed(zero, ne, k):
    """The k nearest of every entity from Engine.predict on the zero-relation copy."""
    ents = np.arange(ne, dtype=np.int32)
    ids, en, _ = zero.predict(ents, np.zeros(ne, np.int32), np.ones(ne, np.int32), k + 1)
    keep = ids != ents[:, None]
    # (a row without itself among its k + 1 -- an exact duplicate with a smaller id ahead of it -- drops its last)
    keep[keep.all(axis=1), -1] = False
    return ids[keep].reshape(ne, k), en[keep].reshape(ne, k)


def profile_and_counters(eng, call, out):
    eng.profile(True)
    call()
    out["families_ms"] = {}
    for name in ("neighbors_score", "neighbors_merge"):
        ms, cnt = eng.profile_query(name)
        out["families_ms"][name] = {"ms": round(ms, 3), "spans": cnt}
    eng.profile(False)
    out["counters"] = {c: eng.counter("neighbors_" + c) for c in ("candidates", "slices", "chunks", "prunes")}
    out["device_bytes"] = eng.device_bytes()


def probe_entity_space(ds, args):
    ne, k = ds.num_entities, args.topk
    eng = trained("E", ds, args)
    ent, rel, _ = eng.download_params()
    zero = Engine("E", args.dim, ne, ds.num_relations)
    zero.upload_params(ent, np.zeros_like(rel))

    def run_new():
        t0 = time.perf_counter()
        out = eng.knn_graph(k)
        return time.perf_counter() - t0, out

    def run_old():
        t0 = time.perf_counter()
        out = composed(zero, ne, k)
        return time.perf_counter() - t0, out

    run_new()
    run_old()
    tn, to = [], []
    for _ in range(args.repeats):
        tn.append(run_new()[0])
        to.append(run_old()[0])
    out = {"model": "E", "space": "entity", "dim": args.dim, "entities": ne, "k": k, "epochs": args.epochs,
           "repeats": args.repeats, "knn_graph": stat(tn), "composed": stat(to),
           "ratio": round(float(np.median(tn) / np.median(to)), 4),
           "ranges_overlap": not (max(tn) < min(to) or max(to) < min(tn))}
    ids, dist, found = run_new()[1]
    cids, cen = run_old()[1]
    rows = np.linspace(0, ne - 1, 8).astype(np.int64)
    for a in rows.tolist():
        if not (found[a] == k and np.array_equal(ids[a], cids[a]) and
                np.array_equal(dist[a].view(np.uint64), cen[a].view(np.uint64))):
            raise SystemExit(f"knn_graph disagrees with the composed route for entity {a}")
    out["rows_checked"] = len(rows)
    profile_and_counters(eng, lambda: eng.knn_graph(k), out)
    eng.close()
    zero.close()
    print(json.dumps(out), flush=True)


def probe_relation_space(ds, args):
    eng = trained("R", ds, args)
    r = int(np.argmax(np.bincount(ds.train[:, 2], minlength=ds.num_relations)))
    eng.knn_graph(args.topk, relation=r)
    t = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        eng.knn_graph(args.topk, relation=r)
        t.append(time.perf_counter() - t0)
    out = {"model": "R", "space": f"relation {r}", "dim": args.dim, "entities": ds.num_entities, "k": args.topk,
           "epochs": args.epochs, "repeats": args.repeats, "knn_graph": stat(t)}
    profile_and_counters(eng, lambda: eng.knn_graph(args.topk, relation=r), out)
    eng.close()
    print(json.dumps(out), flush=True)


def probe_duplicates(ds, args):
    res = linkpred.duplicate_detection(ds, "E", args.dim, args.twins, epochs=args.epochs, k=args.topk, seed=0, rate=0.01,
                                       schedule="parallel")
    out = {"duplicates": {k: res[k] for k in ("k", "entities", "planted", "recall@1", "recall@k", "mutual",
                                              "mutual_share", "baseline")}}
    out["duplicates"]["mutual_planted"] = len(res["mutual_planted"])
    out["epochs"] = args.epochs
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="fb15k")
    ap.add_argument("--dim", type=int, default=50)
    ap.add_argument("--topk", type=int, default=10)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--twins", type=int, default=200)
    ap.add_argument("--duplicates-only", action="store_true", help="skip the timings (a longer-trained model's recalls)")
    args = ap.parse_args()
    ds = data.synthetic(args.shape, seed=0)
    if not args.duplicates_only:
        probe_entity_space(ds, args)
        probe_relation_space(ds, args)
    probe_duplicates(ds, args)


if __name__ == "__main__":
    main()
