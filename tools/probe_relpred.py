#!/usr/bin/env python3
"""GPU probe: what does kb2e_predict_relations cost against the route a caller
had before it -- kb2e_score_triples over the expanded nq * |R| triple list?

On the FB15k-shaped synthetic set (14,951 entities, 1,345 relations, 59,071 test
pairs) with TransE and TransR at --dim after a few PARALLEL epochs, after a
warm-up of both calls, alternating:

* Engine.predict_relations for the test pairs, k = 10, filtered (train + valid +
  test);
* Engine.score over every (pair, relation) triple of the same pairs.  The triple
  list is built before the clock starts, and the numpy filtering, sorting and
  top-k a caller would still have to do afterwards are not counted at all.

TransE scores all test pairs both ways.  TransR's expanded route costs two n x n
projections per triple, so both routes run on the first --transr-pairs test
pairs (a fixed subset, stated in the output).

Host clock around calls that end in a stream synchronise; median and range over
the repeats.  One more predict_relations and rank_relations call each run with
the engine's profile on for the four relpred_* kernel families; for TransR the
pair kernel's key store is timed both ways (through LDS in 256-byte runs, and
the plain store with a stride of |R| * 8 bytes: KB2E_RELPRED_KEYS_STRIDED=1).
Eight queries are checked against a numpy sort over Engine.score at this size.
Prints one JSON line per model.

  python tools/probe_relpred.py --repeats 5
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


def families(eng, call):
    eng.profile(True)
    call()
    fam = {}
    for name in ("relpred_score", "relpred_mask", "relpred_select", "relpred_rank"):
        ms, cnt = eng.profile_query(name)
        fam[name] = {"ms": round(ms, 3), "spans": cnt}
    eng.profile(False)
    return fam


def probe(model, ds, args):
    filt = np.concatenate([ds.train, ds.valid, ds.test])
    nr = ds.num_relations
    eng = Engine(model, args.dim, ds.num_entities, ds.num_relations, rate=0.01, seed=7, schedule="parallel")
    eng.upload_triples(ds.train)
    ent, rel, _ = eng.init_params()
    if model == "R":
        eng.transr_seed(ent, rel)
    for _ in range(args.epochs):
        eng.train_epoch()
    npairs = len(ds.test) if model == "E" else min(args.transr_pairs, len(ds.test))
    if args.pairs:
        npairs = min(npairs, args.pairs)
    test = ds.test[:npairs]
    h, t = np.ascontiguousarray(test[:, 0]), np.ascontiguousarray(test[:, 1])
    trip = np.stack([np.repeat(h, nr), np.repeat(t, nr), np.tile(np.arange(nr, dtype=np.int32), npairs)], 1)

    def run_new():
        t0 = time.perf_counter()
        out = eng.predict_relations(h, t, args.topk, filt)
        return time.perf_counter() - t0, out

    def run_old():
        t0 = time.perf_counter()
        out = eng.score(trip)
        return time.perf_counter() - t0, out

    run_new()
    run_old()
    tn, to = [], []
    for _ in range(args.repeats):
        tn.append(run_new()[0])
        to.append(run_old()[0])
    out = {"model": model, "dim": args.dim, "entities": ds.num_entities, "relations": nr, "pairs": int(npairs),
           "pairs_are": "all test pairs" if npairs == len(ds.test) else f"the first {npairs} test pairs",
           "k": args.topk, "filter": int(len(filt)), "repeats": args.repeats, "predict_relations": stat(tn),
           "score_expanded": stat(to), "ratio": round(float(np.median(tn) / np.median(to)), 4)}
    out["families_ms"] = families(eng, lambda: eng.predict_relations(h, t, args.topk, filt))
    out["rank_families_ms"] = families(eng, lambda: eng.rank_relations(test, filt))
    if model == "R":
        # the pair kernel's key store both ways, alternating, on ALL test pairs (the
        # new route alone: the FB15k shape of the key buffer)
        hf, tf = np.ascontiguousarray(ds.test[:, 0]), np.ascontiguousarray(ds.test[:, 1])

        def run_full(strided):
            if strided:
                os.environ["KB2E_RELPRED_KEYS_STRIDED"] = "1"
            try:
                t0 = time.perf_counter()
                eng.predict_relations(hf, tf, args.topk, filt)
                return time.perf_counter() - t0
            finally:
                os.environ.pop("KB2E_RELPRED_KEYS_STRIDED", None)

        run_full(False)
        ts, tt = [], []
        for _ in range(args.repeats):
            ts.append(run_full(True))
            tt.append(run_full(False))
        fam_t = families(eng, lambda: run_full(False))
        fam_s = families(eng, lambda: run_full(True))
        out["all_pairs"] = {"pairs": int(len(hf)), "transposed": stat(tt), "strided": stat(ts),
                            "families_ms_transposed": fam_t, "families_ms_strided": fam_s}

    # the answers at this size, for a few queries: a numpy sort over the device's own
    # triple energies (kb2e_score_triples), the known relations dropped
    ids, en, _ = eng.predict_relations(h, t, args.topk, filt)
    energies = run_old()[1].reshape(npairs, nr)
    allr = np.arange(nr, dtype=np.int32)
    checked = 0
    for q in np.random.default_rng(0).integers(0, npairs, 8).tolist():
        sel = filt[(filt[:, 0] == h[q]) & (filt[:, 1] == t[q])]
        keep = np.ones(nr, bool)
        keep[sel[:, 2]] = False
        cand = allr[keep]
        order = np.lexsort((cand, energies[q][keep]))[:args.topk]
        if not (np.array_equal(ids[q, :len(order)], cand[order])
                and np.array_equal(en[q, :len(order)], energies[q][keep][order])):
            raise SystemExit(f"predict_relations disagrees with a sort over score() for query {q}")
        checked += 1
    out["queries_checked"] = checked
    out["device_bytes"] = eng.device_bytes()
    eng.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="fb15k")
    ap.add_argument("--models", default="E,R")
    ap.add_argument("--dim", type=int, default=50)
    ap.add_argument("--topk", type=int, default=10)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=0, help="first N test pairs (0: all)")
    ap.add_argument("--transr-pairs", type=int, default=2000, help="TransR: first N test pairs for both routes")
    args = ap.parse_args()
    ds = data.synthetic(args.shape, seed=0)
    for model in args.models.split(","):
        probe(model, ds, args)


if __name__ == "__main__":
    main()
