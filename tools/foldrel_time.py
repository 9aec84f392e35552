#!/usr/bin/env python3
"""Time relation fold-in on the FB15k-shaped synthetic set.

10 % of the relations (134) are held out: the model is trained without their
triples, then they are folded in from half of their triples
(linkpred.fold_in_relations_split), once with batch_size 1 and once with a
larger batch.  Printed per model and batch size, one JSON line: the device time
of kb2e_fold_in_relations (kb2e_profile_query("foldrel")), its wall time,
samples/s (passes x examples / device time), and next to it the wall time of
training the whole set -- new relations included -- for the same number of
epochs, which is what giving the new relations parameters costs without
fold-in.

    python tools/foldrel_time.py [--passes 20] [--models E:100,H:100,R:50] [--batch 64] [--schedule parallel]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from kb2e_amd import data, linkpred  # noqa: E402
from kb2e_amd.engine import Engine  # noqa: E402


def trained(model, dim, ds, triples, epochs, schedule):
    eng = Engine(model, dim, ds.num_entities, ds.num_relations, rate=0.001, batches=100, seed=7, transr_compat=False,
                 schedule=schedule)
    eng.upload_triples(triples)
    ent, rel, _ = eng.init_params()
    if model == "R":
        eng.transr_seed(ent, rel)
    eng.train_epoch()  # (the first epoch builds the sampler's tables)
    eng.synchronize()
    t0 = time.perf_counter()
    for _ in range(epochs):
        eng.train_epoch()
    eng.synchronize()
    return eng, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=20)
    ap.add_argument("--models", default="E:100,H:100,R:50")
    ap.add_argument("--schedule", default="parallel")
    ap.add_argument("--held", type=int, default=134)
    ap.add_argument("--batch", type=int, default=64)
    args = ap.parse_args()
    ds = data.synthetic("fb15k", seed=0)
    rng = np.random.default_rng(0)
    held = np.sort(rng.choice(ds.num_relations, args.held, replace=False)).astype(np.int32)
    train, sup, qry, known = linkpred.fold_in_relations_split(ds, held, 0.5)
    for spec in args.models.split(","):
        model, dim = spec.split(":")
        dim = int(dim)
        full, retrain_s = trained(model, dim, ds, ds.train, args.passes, args.schedule)
        full.close()
        eng, _ = trained(model, dim, ds, train, args.passes, args.schedule)
        try:
            start = eng.download_params()
            for batch in (1, args.batch):
                eng.upload_params(*start)
                eng.profile(True)
                t0 = time.perf_counter()
                _, _, loss, counts = eng.fold_in_relations(held, sup, known, epochs=args.passes, batch_size=batch, seed=0)
                wall = time.perf_counter() - t0
                ms, launches = eng.profile_query("foldrel")
                eng.profile(False)
                samples = args.passes * len(sup)
                print(json.dumps({"model": model, "dim": dim, "held_out": int(len(held)), "examples": int(len(sup)),
                                  "passes": args.passes, "batch_size": batch, "foldrel_device_ms": ms,
                                  "foldrel_wall_ms": wall * 1e3, "launches": launches,
                                  "samples_per_s": samples / (ms * 1e-3) if ms else None,
                                  "most_examples": int(np.bincount(sup[:, 2]).max()),
                                  "active": int(counts[:, 0].sum()), "failed": int(counts[:, 1].sum()),
                                  "capped": int(counts[:, 2].sum()), "loss_first": float(loss[:, 0].sum()),
                                  "loss_last": float(loss[:, 1].sum()), "retrain_schedule": args.schedule,
                                  "retrain_wall_ms": retrain_s * 1e3}), flush=True)
        finally:
            eng.close()


if __name__ == "__main__":
    main()
