#!/usr/bin/env python3
"""GPU probe: what does kb2e_complete_triples cost against the route a caller had
before it -- kb2e_predict with every entity as a head query, then a merge on
the host?

On the FB15k-shaped synthetic set (14,951 entities, 1,345 relations) with TransE
at --dim after --epochs PARALLEL epochs, for the --relations relations with the
most training triples, k = --topk, known = train + valid + test, unconstrained,
loops allowed; after a warm-up of both routes, alternating:

* Engine.complete for all the relations in one call;
* the composed route: per relation, Engine.predict of (h, ?, r) for every entity
  h with the same filter and k, then the numpy merge of the |E| * k answers:
  everything at or under the k-th smallest energy, sorted by (energy, head,
  tail), the first k.

Host clock around calls that end in a stream synchronise; median and range over
the repeats.  One more Engine.complete call runs with the engine's profile on for
the two complete_* kernel families, and the counters of that call are reported
(records / candidates is what the bound let through).  Two relations are checked
for equality with the composed route.  A TransR line on the same data times the
new call alone.  Prints one JSON line per model.

  python tools/probe_complete.py --repeats 5
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from kb2e_amd import data  # noqa: E402
from kb2e_amd.engine import Engine  # noqa: E402


def stat(v):
    return {"median_s": round(float(np.median(v)), 4), "min_s": round(min(v), 4), "max_s": round(max(v), 4)}


def composed(eng, ne, r, k, known):
    """The k best (h, t) of relation r from Engine.predict over every head."""
    ents = np.arange(ne, dtype=np.int32)
    ids, en, _ = eng.predict(ents, np.full(ne, r, np.int32), np.ones(ne, np.int32), k, known)
    heads = np.repeat(ents, ids.shape[1])
    tails, energy = ids.reshape(-1), en.reshape(-1)
    live = np.flatnonzero(tails >= 0)
    kk = min(k, len(live))
    if kk == 0:
        return heads[:0], tails[:0], energy[:0]
    bound = np.partition(energy[live], kk - 1)[kk - 1]
    live = live[energy[live] <= bound]
    order = live[np.lexsort((tails[live], heads[live], energy[live]))[:kk]]
    return heads[order], tails[order], energy[order]


def probe(model, ds, args, compare):
    known = np.concatenate([ds.train, ds.valid, ds.test])
    ne = ds.num_entities
    eng = Engine(model, args.dim, ne, ds.num_relations, rate=0.01, seed=7, schedule="parallel")
    eng.upload_triples(ds.train)
    ent, rel, _ = eng.init_params()
    if model == "R":
        eng.transr_seed(ent, rel)
    for _ in range(args.epochs):
        eng.train_epoch()
    rels = np.argsort(-np.bincount(ds.train[:, 2], minlength=ds.num_relations), kind="stable")[:args.relations]
    rels = rels.astype(np.int32)

    def run_new():
        t0 = time.perf_counter()
        out = eng.complete(rels, args.topk, known)
        return time.perf_counter() - t0, out

    def run_old(which=rels):
        t0 = time.perf_counter()
        out = [composed(eng, ne, int(r), args.topk, known) for r in which]
        return time.perf_counter() - t0, out

    run_new()
    out = {"model": model, "dim": args.dim, "entities": ne, "relations": [int(r) for r in rels], "k": args.topk,
           "known": int(len(known)), "epochs": args.epochs, "repeats": args.repeats}
    if compare:
        run_old(rels[:1])
        tn, to = [], []
        for _ in range(args.repeats):
            tn.append(run_new()[0])
            to.append(run_old()[0])
        out.update({"complete": stat(tn), "composed": stat(to),
                    "ratio": round(float(np.median(tn) / np.median(to)), 4),
                    "ranges_overlap": not (max(tn) < min(to) or max(to) < min(tn))})
        heads, tails, en, found = run_new()[1]
        for q in (0, len(rels) - 1):
            h, t, e = run_old(rels[q:q + 1])[1][0]
            if not (found[q] == len(h) and np.array_equal(heads[q, :len(h)], h) and np.array_equal(tails[q, :len(h)], t)
                    and np.array_equal(en[q, :len(h)], e)):
                raise SystemExit(f"complete disagrees with the composed route for relation {int(rels[q])}")
        out["relations_checked"] = 2
    else:
        out["complete"] = stat([run_new()[0] for _ in range(args.repeats)])
    eng.profile(True)
    run_new()
    out["families_ms"] = {}
    for name in ("complete_score", "complete_select"):
        ms, cnt = eng.profile_query(name)
        out["families_ms"][name] = {"ms": round(ms, 3), "spans": cnt}
    eng.profile(False)
    out["counters"] = {c: eng.counter("complete_" + c) for c in ("candidates", "records", "strips", "buffer_records")}
    out["records_per_candidate"] = out["counters"]["records"] / max(1, out["counters"]["candidates"])
    out["device_bytes"] = eng.device_bytes()
    eng.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="fb15k")
    ap.add_argument("--models", default="E,R", help="the first is compared with the composed route, the others run alone")
    ap.add_argument("--dim", type=int, default=50)
    ap.add_argument("--topk", type=int, default=100)
    ap.add_argument("--relations", type=int, default=16)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    ds = data.synthetic(args.shape, seed=0)
    for i, model in enumerate(args.models.split(",")):
        probe(model, ds, args, compare=i == 0)


if __name__ == "__main__":
    main()
