#!/usr/bin/env python3
"""GPU probe: what do the key write, the mask and the selection of kb2e_predict
cost on top of the scoring the evaluator already does?

On the FB15k-shaped synthetic set with TransE n=50 (a few PARALLEL epochs, so the
energies are a trained model's), after a warm-up of both calls, alternating:

* Engine.predict for the 2 * ntest one-sided queries of the test set, k = 10,
  filtered (train + valid + test);
* Engine.evaluate over the same ntest triples (the same |E| * n scoring work per
  query side, plus its per-candidate filter probes).

Host clock around calls that end in a stream synchronise; median and range over
the repeats.  One more predict call runs with the engine's profile on for the
three predict_* kernel families (event pairs around each chunk's launches).
Prints one JSON line.

  python tools/probe_predict.py --repeats 5
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="fb15k")
    ap.add_argument("--dim", type=int, default=50)
    ap.add_argument("--topk", type=int, default=10)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ntest", type=int, default=0, help="first N test triples (0: all)")
    args = ap.parse_args()
    ds = data.synthetic(args.shape, seed=0)
    test = ds.test[:args.ntest] if args.ntest else ds.test
    filt = np.concatenate([ds.train, ds.valid, ds.test])
    eng = Engine("E", args.dim, ds.num_entities, ds.num_relations, rate=0.01, seed=7, schedule="parallel")
    eng.upload_triples(ds.train)
    eng.init_params()
    for _ in range(args.epochs):
        eng.train_epoch()
    e = np.concatenate([test[:, 0], test[:, 1]]).astype(np.int32)
    r = np.concatenate([test[:, 2], test[:, 2]]).astype(np.int32)
    side = np.concatenate([np.ones(len(test), np.int32), np.zeros(len(test), np.int32)])

    def run_predict():
        t0 = time.perf_counter()
        out = eng.predict(e, r, side, args.topk, filt)
        return time.perf_counter() - t0, out

    def run_evaluate():
        t0 = time.perf_counter()
        out = eng.evaluate(test, filt)
        return time.perf_counter() - t0, out

    run_predict()
    run_evaluate()
    tp, te = [], []
    for _ in range(args.repeats):
        tp.append(run_predict()[0])
        te.append(run_evaluate()[0])
    eng.profile(True)
    _, (_, _, found) = run_predict()
    fam = {}
    for name in ("predict_score", "predict_mask", "predict_select"):
        ms, cnt = eng.profile_query(name)
        fam[name] = {"ms": round(ms, 3), "spans": cnt}
    eng.profile(False)

    # the answers at this size, for a few queries: a numpy sort over the device's own
    # triple energies (kb2e_score_triples), the known candidates dropped
    ids, en, _ = eng.predict(e, r, side, args.topk, filt)
    allx = np.arange(ds.num_entities, dtype=np.int32)
    checked = 0
    for q in np.random.default_rng(0).integers(0, len(e), 8).tolist():
        fixed, rel = np.full_like(allx, e[q]), np.full_like(allx, r[q])
        trip = np.stack([fixed, allx, rel], 1) if side[q] else np.stack([allx, fixed, rel], 1)
        row = eng.score(trip)
        sel = filt[(filt[:, 2] == r[q]) & (filt[:, 0 if side[q] else 1] == e[q])]
        keep = np.ones(len(allx), bool)
        keep[sel[:, 1 if side[q] else 0]] = False
        cand = allx[keep]
        order = np.lexsort((cand, row[keep]))[:args.topk]
        if not (np.array_equal(ids[q, :len(order)], cand[order]) and np.array_equal(en[q, :len(order)], row[keep][order])):
            raise SystemExit(f"predict disagrees with a sort over score() for query {q}")
        checked += 1

    def stat(v):
        return {"median_s": round(float(np.median(v)), 4), "min_s": round(min(v), 4), "max_s": round(max(v), 4)}

    print(json.dumps({"shape": args.shape, "entities": ds.num_entities, "relations": ds.num_relations,
                      "dim": args.dim, "queries": int(len(e)), "test": int(len(test)), "k": args.topk,
                      "filter": int(len(filt)), "repeats": args.repeats, "predict": stat(tp), "evaluate": stat(te),
                      "ratio": round(float(np.median(tp) / np.median(te)), 3), "families_ms": fam,
                      "found_min": int(found.min()), "queries_checked": checked, "device_bytes": eng.device_bytes()}))


if __name__ == "__main__":
    main()
