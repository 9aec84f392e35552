"""Train-then-evaluate driver for link-prediction comparisons (host side).

Runs the reference's train binary sequence (``transe/bin/trainTransE.cpp:9-20``:
prepTrain, bfgs epochs) on the GPU engine and scores the result with the GPU
evaluator (``kb2e_evaluate`` = ``EmbeddingEvaluation::run``,
``common/evaluation.cpp:181-251``; filter = train + valid + test as the
reference's eval binaries pass it, ``common/evaluation.cpp:41-62``).

TransR starts from TransE tables ("TransE-init", ``transr/trainer.cpp:88-113``):
``transe_seed`` trains TransE with the ORDERED schedule (the reference's exact
semantics) and round-trips the tables through the reference's ``%.6lf`` text
format, exactly what ``trainTransR --seeddatadir`` reads.

Used by tools/hits_parity.py (FB15k-shaped runs) and the schedule-parity GPU
test (tests/test_gpu_hits_parity.py).

``relation_categories`` / ``hits_by_category`` give the 1-1 / 1-N / N-1 / N-N
Hits@k table of the TransE, TransH and TransR papers from the per-triple ranks
of ``Engine.rank_triples``; ``relation_prediction`` gives the mean rank and
Hits@k of the true relation (the relation-prediction numbers of the PTransE line
of work) from ``Engine.rank_relations``.  ``triple_classification`` is the third
evaluation task of those papers (Socher et al. 2013; TransH 4.3, TransR 4.3):
per-relation energy thresholds fitted on the validation split
(``Engine.fit_thresholds``), negatives generated on the device where the data
set ships none (``Engine.corrupt``), accuracy on the test split
(``Engine.classify``).  ``completion`` is the hold-out measure of knowledge-base
completion: the k most plausible new triples of each relation mined on the
device (``Engine.complete``) against the relation's test triples.
``fold_in_evaluation`` measures entity fold-in (``Engine.fold_in``): entities
held out of training get their rows from a share of their triples with the
trained model frozen, and their remaining triples are ranked before and after.
``entity_identification`` is its counterpart for entities the model has: the
test triples that mention an entity, with the entity taken out, are one
conjunctive query (``Engine.rank_joint``) that should rank it first.
``path_evaluation`` ranks the tail of every test triple at the end of a relation
path that reaches its head through train triples (``Engine.rank_path``).
``duplicate_detection`` is the hold-out measure of entity neighbours
(``Engine.knn_graph``): twins are planted (``duplicate_split``), the model is
trained on the split set, and each twin's original is looked up among the
twin's nearest entities and among the graph's mutual pairs (``mutual_pairs``).
"""
from __future__ import annotations

import os
import tempfile
import time

import numpy as np

from . import data
from .engine import Engine


def transe_seed(ds, dim, epochs, *, rate=0.001, seed=7, batches=100, device=0):
    """TransE n=dim unif (the reference's historical seed method) -> (entity, relation)
    tables as trainTransR reads them back from entity2vec.unif / relation2vec.unif."""
    eng = Engine("E", dim, ds.num_entities, ds.num_relations, rate=rate, method=0, seed=seed, batches=batches,
                 device=device, schedule="ordered")
    try:
        eng.upload_triples(ds.train)
        eng.init_params()
        if epochs:
            eng.train_batches(epochs * batches)
        eng.synchronize()
        ent, rel, _ = eng.download_params()
    finally:
        eng.close()
    with tempfile.TemporaryDirectory() as d:
        data.write_table(os.path.join(d, "entity2vec.unif"), ent)
        data.write_table(os.path.join(d, "relation2vec.unif"), rel)
        return (data.read_table(os.path.join(d, "entity2vec.unif"), ds.num_entities, dim),
                data.read_table(os.path.join(d, "relation2vec.unif"), ds.num_relations, dim))


def train_and_evaluate(ds, model, dim, schedule, epochs, *, test=None, rate=0.001, method=1, distance=0,
                       batches=100, seed=7, transr_compat=True, seed_tables=None, device=0, log=None,
                       sub_batches=None):
    """Train `epochs` epochs with one schedule and evaluate; returns a dict with
    the four EmbeddingEvaluation::run numbers, losses and timing."""
    test = ds.test if test is None else test
    filt = np.concatenate([ds.train, ds.valid, ds.test])
    eng = Engine(model, dim, ds.num_entities, ds.num_relations, rate=rate, method=method, distance=distance,
                 batches=batches, seed=seed, transr_compat=transr_compat, device=device, schedule=schedule,
                 sub_batches=sub_batches)
    try:
        eng.upload_triples(ds.train)
        ent, rel, _ = eng.init_params()
        if model in ("R", "transr", 2):
            eng.transr_seed(*(seed_tables if seed_tables is not None else (ent, rel)))
        losses = []
        t0 = time.perf_counter()
        for ep in range(epochs):
            loss, act = eng.train_epoch()
            losses.append((ep, float(loss), int(act)))
            if log is not None and (ep % max(1, epochs // 10) == 0 or ep == epochs - 1):
                log(f"[{model}/{schedule}] epoch {ep} loss {loss:.3f} active {act}")
        train_s = time.perf_counter() - t0
        res = eng.evaluate(test, filt)
    finally:
        eng.close()
    S = (len(ds.train) // batches) * batches
    return {"train_s": train_s, "samples_per_s": epochs * S / max(train_s, 1e-9), "losses": losses,
            **{k: float(v) for k, v in res.items()}}


def schedule_parity(ds, model, dim, epochs, *, seed_epochs=0, test=None, schedules=("ordered", "parallel"),
                    **kw):
    """Both schedules from the same initial tables and the same glibc sample
    stream; returns {schedule: result, "delta_filtered_hits10_pp": ...}."""
    seed_tables = None
    if model == "R":
        seed_tables = transe_seed(ds, dim, seed_epochs, rate=kw.get("rate", 0.001), seed=kw.get("seed", 7),
                                  batches=kw.get("batches", 100), device=kw.get("device", 0))
    out = {"model": model, "dim": dim, "epochs": epochs, "seed_epochs": seed_epochs,
           "test": int(len(ds.test if test is None else test)), "entities": ds.num_entities,
           "random_hits10": 10.0 / ds.num_entities}
    for s in schedules:
        out[s] = train_and_evaluate(ds, model, dim, s, epochs, test=test, seed_tables=seed_tables, **kw)
    if len(schedules) == 2:
        a, b = schedules
        for k in ("filtered_hits10", "raw_hits10"):
            out[f"delta_{k}_pp"] = 100.0 * (out[b][k] - out[a][k])
        out["delta_filtered_rank"] = out[b]["filtered_rank"] - out[a]["filtered_rank"]
    return out


CATEGORIES = ("1-1", "1-N", "N-1", "N-N")


def relation_categories(train, num_relations, threshold=1.5):
    """Per relation: the mean number of tails per (head, relation) pair (tph) and
    of heads per (tail, relation) pair (hpt) over the distinct training triples,
    and its category with the 1.5 threshold of Bordes et al. (2013): "1-1" (both
    below), "1-N" (tph at or above: many tails for a head), "N-1" (hpt at or
    above), "N-N" (both).  A relation without training triples has means 0 and
    counts as 1-1.  Returns (cats list[str], tph float64[R], hpt float64[R])."""
    t = np.unique(np.asarray(train, dtype=np.int64).reshape(-1, 3), axis=0)
    tph = np.zeros(num_relations)
    hpt = np.zeros(num_relations)
    for r in range(num_relations):
        rows = t[t[:, 2] == r]
        if len(rows):
            tph[r] = len(rows) / len(np.unique(rows[:, 0]))
            hpt[r] = len(rows) / len(np.unique(rows[:, 1]))
    cats = []
    for r in range(num_relations):
        many_t, many_h = tph[r] >= threshold, hpt[r] >= threshold
        cats.append("N-N" if many_t and many_h else "1-N" if many_t else "N-1" if many_h else "1-1")
    return cats, tph, hpt


def hits_by_category(ranks, test, cats, at=10):
    """Filtered Hits@`at` per relation category and prediction side, from
    ``Engine.rank_triples`` output (columns head raw, head filtered, tail raw,
    tail filtered).  Returns {category: {"count", "head", "tail"}}; the
    fractions are None for a category without test triples."""
    ranks = np.asarray(ranks).reshape(-1, 4)
    test = np.asarray(test).reshape(-1, 3)
    if len(ranks) != len(test):
        raise ValueError("ranks and test differ in length")
    cat_of = np.array([CATEGORIES.index(cats[r]) for r in test[:, 2]], dtype=np.int64)
    out = {}
    for c, name in enumerate(CATEGORIES):
        sel = cat_of == c
        m = int(sel.sum())
        out[name] = {"count": m,
                     "head": float((ranks[sel, 1] <= at).mean()) if m else None,
                     "tail": float((ranks[sel, 3] <= at).mean()) if m else None}
    return out


def relation_metrics(ranks, at=(1, 10)):
    """Mean rank and Hits@k of ``Engine.rank_relations`` output (columns raw,
    filtered).  Returns {"count", "raw": {"mean_rank", "hits@k"...}, "filtered": {...}}."""
    ranks = np.asarray(ranks).reshape(-1, 2)
    if len(ranks) == 0:
        raise ValueError("no ranks")
    out = {"count": int(len(ranks))}
    for col, name in enumerate(("raw", "filtered")):
        out[name] = {"mean_rank": float(ranks[:, col].mean()),
                     **{f"hits@{k}": float((ranks[:, col] <= k).mean()) for k in at}}
    return out


def relation_prediction(eng, test, filt, at=(1, 10)):
    """Relation prediction over the test triples: the true relation of each
    (head, tail) pair ranked among all relations on the device
    (``Engine.rank_relations``), raw and with the other known relations of the
    pair (rows of `filt`) left out; mean rank and Hits@k for every k of `at`."""
    return relation_metrics(eng.rank_relations(test, filt), at)


def _labelled_split(eng, given, positives, known, seed, constrained):
    """(triples, labels, failed): the caller's labelled pair, or the positives
    followed by one generated negative each (failed ones dropped)."""
    if given is not None:
        triples, labels = given
        triples = np.ascontiguousarray(triples, dtype=np.int32).reshape(-1, 3)
        labels = np.ascontiguousarray(labels, dtype=np.uint8).reshape(-1)
        if len(triples) != len(labels):
            raise ValueError("triples and labels differ in length")
        return triples, labels, 0
    positives = np.ascontiguousarray(positives, dtype=np.int32).reshape(-1, 3)
    neg, failed = eng.corrupt(positives, known, seed=seed, side=2, constrained=constrained)
    neg = neg[neg[:, 0] >= 0]
    triples = np.concatenate([positives, neg]).astype(np.int32)
    labels = np.concatenate([np.ones(len(positives), np.uint8), np.zeros(len(neg), np.uint8)])
    return triples, labels, int(failed)


def classification_accuracy(predicted, labels, relations, num_relations):
    """{"count", "accuracy", "per_relation": {r: {"count", "accuracy"}}} of predicted
    against true labels; only relations with a triple are listed."""
    predicted, labels, relations = (np.asarray(a).reshape(-1) for a in (predicted, labels, relations))
    hit = predicted == labels
    n = np.bincount(relations, minlength=num_relations)
    ok = np.bincount(relations, weights=hit, minlength=num_relations).astype(np.int64)
    return {"count": int(len(hit)), "accuracy": float(hit.sum() / len(hit)) if len(hit) else None,
            "per_relation": {int(r): {"count": int(n[r]), "accuracy": float(ok[r] / n[r])}
                             for r in np.flatnonzero(n)}}


def triple_classification(eng, ds, *, seed=0, constrained=True, valid=None, test=None):
    """Triple classification of a trained engine: thresholds fitted on the valid
    split, accuracy on the test split.  `valid` / `test` are optional (triples,
    labels) pairs for data sets that ship labels (WN11, FB13); otherwise one
    negative per triple of ``ds.valid`` / ``ds.test`` is generated with
    known = train + valid + test (stream seeds `seed` and `seed + 1`), failed
    ones dropped.  Returns {"thresholds", "counts", "global_threshold",
    "global_correct", "valid": {...}, "test": {...}}, each split with "count",
    "accuracy", "per_relation" and "failed"."""
    known = np.concatenate([ds.train, ds.valid, ds.test])
    vt, vl, vfail = _labelled_split(eng, valid, ds.valid, known, seed, constrained)
    tt, tl, tfail = _labelled_split(eng, test, ds.test, known, seed + 1, constrained)
    thr, counts, gthr, gcorrect = eng.fit_thresholds(vt, vl)
    out = {"thresholds": thr, "counts": counts, "global_threshold": gthr, "global_correct": gcorrect}
    for name, triples, labels, failed in (("valid", vt, vl, vfail), ("test", tt, tl, tfail)):
        res = classification_accuracy(eng.classify(triples, thr), labels, triples[:, 2], ds.num_relations)
        res["failed"] = failed
        out[name] = res
    return out


def completion_metrics(heads, tails, found, relations, test, known, k):
    """Recall@k and precision@k of ``Engine.complete`` output (one row per entry
    of `relations`) against the hold-out triples `test`: per relation the number
    of its test triples -- distinct, and not among the rows of `known`, which the
    mining excludes -- that are among the mined pairs.  recall = hits / test
    triples (None without one), precision = hits / mined (None when nothing was
    mined).  Returns {"k", "relations", "mined", "test", "hits", "recall",
    "precision", "per_relation": {r: {"mined", "test", "hits", "recall",
    "precision"}}}; a relation listed twice is counted once."""
    heads, tails = np.asarray(heads), np.asarray(tails)
    found = np.asarray(found).reshape(-1)
    relations = np.asarray(relations).reshape(-1)
    test = np.asarray(test, dtype=np.int64).reshape(-1, 3)
    known = np.asarray(known, dtype=np.int64).reshape(-1, 3)
    hold = {}
    for h, t, r in test.tolist():
        hold.setdefault(r, set()).add((h, t))
    for h, t, r in known.tolist():
        if r in hold:
            hold[r].discard((h, t))
    per = {}
    for q, r in enumerate(relations.tolist()):
        if r in per:
            continue
        nf = int(found[q])
        mined = set(zip(heads[q, :nf].tolist(), tails[q, :nf].tolist()))
        truth = hold.get(r, set())
        hits = len(mined & truth)
        per[int(r)] = {"mined": nf, "test": len(truth), "hits": hits,
                       "recall": hits / len(truth) if truth else None,
                       "precision": hits / nf if nf else None}
    mined = sum(v["mined"] for v in per.values())
    ntest = sum(v["test"] for v in per.values())
    hits = sum(v["hits"] for v in per.values())
    return {"k": int(k), "relations": len(per), "mined": mined, "test": ntest, "hits": hits,
            "recall": hits / ntest if ntest else None, "precision": hits / mined if mined else None,
            "per_relation": per}


def completion(eng, ds, k, *, constrained=True, exclude_loops=True, relations=None):
    """Knowledge-base completion with a hold-out: the k most plausible new triples
    of each relation (every relation unless `relations` lists some) are mined on
    the device with known = train + valid (``Engine.complete``), and the
    relation's test triples are looked up among them: recall@k and precision@k
    per relation and overall (``completion_metrics``)."""
    known = np.concatenate([ds.train, ds.valid]).astype(np.int32)
    rels = np.arange(ds.num_relations, dtype=np.int32) if relations is None else \
        np.ascontiguousarray(relations, dtype=np.int32).reshape(-1)
    heads, tails, _, found = eng.complete(rels, k, known, constrained=constrained, exclude_loops=exclude_loops)
    return completion_metrics(heads, tails, found, rels, ds.test, known, k)


def fold_in_split(ds, held_out, support=0.5):
    """The data of a fold-in experiment.  Returns (train, support, query, known):
    `train` = the training triples that mention no held-out entity; the distinct
    triples of all three splits that mention exactly one held-out entity are
    divided per held-out entity, in the order train, valid, test, into its first
    ceil(support * m) triples (`support`, the fold-in examples; at least one) and
    the rest (`query`); `known` = every triple of the three splits.  A triple with
    two held-out entities can be neither an example nor a fair query and is left
    out."""
    held = np.unique(np.asarray(held_out, dtype=np.int64).reshape(-1))
    known = np.concatenate([ds.train, ds.valid, ds.test]).astype(np.int32)
    train = np.asarray(ds.train, dtype=np.int32)
    train = train[~(np.isin(train[:, 0], held) | np.isin(train[:, 1], held))]
    _, first = np.unique(known, axis=0, return_index=True)
    distinct = known[np.sort(first)]
    hh, ht = np.isin(distinct[:, 0], held), np.isin(distinct[:, 1], held)
    one = distinct[hh ^ ht]
    owner = np.where(np.isin(one[:, 0], held), one[:, 0], one[:, 1])
    sup, qry = [], []
    for e in held.tolist():
        mine = one[owner == e]
        k = min(len(mine), max(1, int(np.ceil(support * len(mine))))) if len(mine) else 0
        sup.append(mine[:k])
        qry.append(mine[k:])
    empty = np.zeros((0, 3), np.int32)
    return (train, np.concatenate(sup + [empty]).astype(np.int32), np.concatenate(qry + [empty]).astype(np.int32),
            known)


def fold_in_evaluation(ds, model, dim, held_out, *, support=0.5, epochs=50, fold_epochs=50, fold_seed=0, side=2,
                       rate=0.001, margin=1.0, method=1, distance=0, batches=100, seed=7, schedule="ordered",
                       device=0, make_engine=Engine):
    """Hold entities out, train without them, fold them in, and rank what is left:
    every triple that mentions a held-out entity is removed from training
    (``fold_in_split``), the model is trained `epochs` epochs on the rest, the
    held-out entities are folded in from the `support` share of their triples
    (``Engine.fold_in``, `fold_epochs` passes, known = all triples), and their
    remaining triples are ranked (``Engine.rank_triples``, filtered) first with
    the rows the held-out entities had after training -- their initial rows, which
    no training sample touched -- and then with the folded rows.  Returns
    {"held_out", "support", "query", "rank_before", "rank_after" (filtered mean
    rank over both sides), "hits10_before", "hits10_after", "loss_first",
    "loss_last" (summed over the held-out entities), "active", "failed",
    "capped", "rows"}."""
    held = np.unique(np.asarray(held_out, dtype=np.int32).reshape(-1))
    train, sup, qry, known = fold_in_split(ds, held, support)
    if len(qry) == 0:
        raise ValueError("no query triples: the held-out entities have too few triples")
    eng = make_engine(model, dim, ds.num_entities, ds.num_relations, rate=rate, margin=margin, method=method,
                      distance=distance, batches=batches, seed=seed, transr_compat=False, device=device,
                      schedule=schedule)
    try:
        eng.upload_triples(train)
        ent, rel, _ = eng.init_params()
        if model in ("R", "transr", 2):
            eng.transr_seed(ent, rel)
        for _ in range(epochs):
            eng.train_epoch()
        eng.synchronize()
        before = np.asarray(eng.rank_triples(qry, known)).reshape(-1, 4)
        rows, loss, counts = eng.fold_in(held, sup, known, epochs=fold_epochs, seed=fold_seed, side=side)
        after = np.asarray(eng.rank_triples(qry, known)).reshape(-1, 4)
    finally:
        eng.close()
    filt = [1, 3]
    return {"held_out": int(len(held)), "support": int(len(sup)), "query": int(len(qry)),
            "rank_before": float(before[:, filt].mean()), "rank_after": float(after[:, filt].mean()),
            "hits10_before": float((before[:, filt] <= 10).mean()), "hits10_after": float((after[:, filt] <= 10).mean()),
            "loss_first": float(loss[:, 0].sum()), "loss_last": float(loss[:, 1].sum()),
            "active": int(counts[:, 0].sum()), "failed": int(counts[:, 1].sum()), "capped": int(counts[:, 2].sum()),
            "rows": rows}


def fold_in_relations_split(ds, held_out, support=0.5):
    """The data of a relation fold-in experiment.  Returns (train, support,
    query, known): `train` = the training triples of the other relations; the
    distinct triples of all three splits that belong to a held-out relation are
    divided per held-out relation, in the order train, valid, test, into its
    first ceil(support * m) triples (`support`, the fold-in examples; at least
    one) and the rest (`query`); `known` = every triple of the three splits."""
    held = np.unique(np.asarray(held_out, dtype=np.int64).reshape(-1))
    known = np.concatenate([ds.train, ds.valid, ds.test]).astype(np.int32)
    train = np.asarray(ds.train, dtype=np.int32)
    train = train[~np.isin(train[:, 2], held)]
    _, first = np.unique(known, axis=0, return_index=True)
    distinct = known[np.sort(first)]
    sup, qry = [], []
    for r in held.tolist():
        mine = distinct[distinct[:, 2] == r]
        k = min(len(mine), max(1, int(np.ceil(support * len(mine))))) if len(mine) else 0
        sup.append(mine[:k])
        qry.append(mine[k:])
    empty = np.zeros((0, 3), np.int32)
    return (train, np.concatenate(sup + [empty]).astype(np.int32), np.concatenate(qry + [empty]).astype(np.int32),
            known)


def fold_in_relations_evaluation(ds, model, dim, held_out, *, support=0.5, epochs=50, fold_epochs=50, batch_size=1,
                                 fold_seed=0, side=2, rate=0.001, margin=1.0, method=1, distance=0, batches=100,
                                 seed=7, schedule="ordered", device=0, make_engine=Engine):
    """Hold relations out, train without them, fold them in, and rank what is
    left: every triple of a held-out relation is removed from training
    (``fold_in_relations_split``; a relation without a training triple is never
    sampled, so its parameters stay as initialised), the model is trained `epochs`
    epochs on the rest, the held-out relations are folded in from the `support`
    share of their triples (``Engine.fold_in_relations``, `fold_epochs` passes in
    batches of `batch_size`, known = all triples), and their remaining triples
    are ranked -- the entities with ``Engine.rank_triples``, the relation with
    ``Engine.rank_relations``, both filtered -- first with the parameters the
    held-out relations had after training and then with the folded ones.  Returns
    fold_in_evaluation's keys ("rank_*" and "hits10_*" over both entity sides)
    with "rel_rank_before" / "rel_rank_after" (filtered mean rank of the
    relation) added, and "rel_rows" / "w_rows" in place of "rows"."""
    held = np.unique(np.asarray(held_out, dtype=np.int32).reshape(-1))
    train, sup, qry, known = fold_in_relations_split(ds, held, support)
    if len(qry) == 0:
        raise ValueError("no query triples: the held-out relations have too few triples")
    eng = make_engine(model, dim, ds.num_entities, ds.num_relations, rate=rate, margin=margin, method=method,
                      distance=distance, batches=batches, seed=seed, transr_compat=False, device=device,
                      schedule=schedule)
    try:
        eng.upload_triples(train)
        ent, rel, _ = eng.init_params()
        if model in ("R", "transr", 2):
            eng.transr_seed(ent, rel)
        for _ in range(epochs):
            eng.train_epoch()
        eng.synchronize()
        before = np.asarray(eng.rank_triples(qry, known)).reshape(-1, 4)
        rel_before = np.asarray(eng.rank_relations(qry, known)).reshape(-1, 2)
        rows, wrows, loss, counts = eng.fold_in_relations(held, sup, known, epochs=fold_epochs, batch_size=batch_size,
                                                          seed=fold_seed, side=side)
        after = np.asarray(eng.rank_triples(qry, known)).reshape(-1, 4)
        rel_after = np.asarray(eng.rank_relations(qry, known)).reshape(-1, 2)
    finally:
        eng.close()
    filt = [1, 3]
    return {"held_out": int(len(held)), "support": int(len(sup)), "query": int(len(qry)),
            "rank_before": float(before[:, filt].mean()), "rank_after": float(after[:, filt].mean()),
            "hits10_before": float((before[:, filt] <= 10).mean()), "hits10_after": float((after[:, filt] <= 10).mean()),
            "rel_rank_before": float(rel_before[:, 1].mean()), "rel_rank_after": float(rel_after[:, 1].mean()),
            "loss_first": float(loss[:, 0].sum()), "loss_last": float(loss[:, 1].sum()),
            "active": int(counts[:, 0].sum()), "failed": int(counts[:, 1].sum()), "capped": int(counts[:, 2].sum()),
            "rel_rows": rows, "w_rows": wrows}


def identification_queries(test, m_max):
    """The mentions behind ``entity_identification``.  For every entity the
    triples of `test` that mention it, in file order (a triple with the entity in
    both slots is skipped), each as the pattern it leaves once the entity is
    taken out: (tail, relation, 0) where the entity is the head -- the unknown is
    the head of (?, tail, relation) -- and (head, relation, 1) where it is the
    tail.  Returns (entities int32[nq], patterns list of int32[m_max, 3]): the
    entities with at least `m_max` mentions, ascending, and their first `m_max`
    patterns."""
    mentions = {}
    for h, t, r in np.asarray(test, dtype=np.int64).reshape(-1, 3).tolist():
        if h == t:
            continue
        mentions.setdefault(h, []).append((t, r, 0))
        mentions.setdefault(t, []).append((h, r, 1))
    ents = sorted(e for e, rows in mentions.items() if len(rows) >= m_max)
    return np.array(ents, np.int32), [np.array(mentions[e][:m_max], np.int32).reshape(-1, 3) for e in ents]


def rank_metrics(ranks):
    """{"mean_rank", "mrr", "hits@1", "hits@10"} of a column of ranks."""
    ranks = np.asarray(ranks, dtype=np.float64).reshape(-1)
    return {"mean_rank": float(ranks.mean()), "mrr": float((1.0 / ranks).mean()),
            "hits@1": float((ranks <= 1).mean()), "hits@10": float((ranks <= 10).mean())}


def entity_identification(eng, ds, constraints=(1, 2, 3)):
    """Which known entity is this record?  The counterpart of entity fold-in: every
    entity that ``ds.test`` mentions at least max(constraints) times is taken out
    of its own test triples, and for each m of `constraints` its first m mentions
    (``identification_queries``) are one conjunctive query whose answer should be
    the entity: ``Engine.rank_joint`` with truth = the entity and filter = train +
    valid + test.  Returns {m: {"count", "raw": {...}, "filtered": {...}}} with
    mean rank, MRR, Hits@1 and Hits@10 (``rank_metrics``)."""
    constraints = tuple(int(m) for m in constraints)
    if not constraints or min(constraints) < 1:
        raise ValueError("constraints must be positive")
    ents, patterns = identification_queries(ds.test, max(constraints))
    if len(ents) == 0:
        raise ValueError("no entity has that many test mentions")
    filt = np.concatenate([ds.train, ds.valid, ds.test]).astype(np.int32)
    out = {}
    for m in constraints:
        ranks = np.asarray(eng.rank_joint([p[:m] for p in patterns], ents, filt)).reshape(-1, 2)
        out[m] = {"count": int(len(ents)), "raw": rank_metrics(ranks[:, 0]), "filtered": rank_metrics(ranks[:, 1])}
    return out


def path_query_set(ds, hops, seed=0):
    """Path queries whose last hop is a test triple.  For every row (h, t, r) of
    ``ds.test``, in order, walk ``hops - 1`` steps backwards from h through
    ``ds.train``: at entity e one of the train triples that mention e, in either
    role, is chosen uniformly (``numpy.random.default_rng(seed)``, one draw per
    step, over the triples in file order); (a, e, r') is the forward hop
    (r', 1) from a, (e, b, r') the hop (r', 0) -- r' walked backwards -- from b.
    A test triple whose walk meets an entity no train triple mentions is
    dropped.  Returns (anchors int32[nq], paths list of int32[hops, 2] rows of
    (relation, side), truth int32[nq]): the walk's last entity, the hops from
    it to h followed by (r, 1), and t."""
    hops = int(hops)
    if hops < 1:
        raise ValueError("hops must be positive")
    train = np.asarray(ds.train, dtype=np.int64).reshape(-1, 3)
    mentions = {}
    if hops > 1:
        for i, (h, t, _) in enumerate(train.tolist()):
            mentions.setdefault(h, []).append(i)
            if t != h:
                mentions.setdefault(t, []).append(i)
    rng = np.random.default_rng(seed)
    anchors, paths, truth = [], [], []
    for h, t, r in np.asarray(ds.test, dtype=np.int64).reshape(-1, 3).tolist():
        at, back = h, []
        for _ in range(hops - 1):
            cand = mentions.get(at)
            if not cand:
                back = None
                break
            a, b, rr = train[cand[int(rng.integers(len(cand)))]].tolist()
            if b == at:  # (a, at, rr): forwards from a
                back.append((rr, 1))
                at = a
            else:        # (at, b, rr): backwards from b
                back.append((rr, 0))
                at = b
        if back is None:
            continue
        anchors.append(at)
        paths.append(np.array(back[::-1] + [(r, 1)], np.int32).reshape(-1, 2))
        truth.append(t)
    return np.array(anchors, np.int32), paths, np.array(truth, np.int32)


def path_evaluation(eng, ds, hops=(1, 2, 3), beam=64, seed=0, limit=None):
    """Link prediction at the end of a path: for each length of `hops` the queries
    of ``path_query_set`` (the first `limit` of them, if given) are ranked by
    ``Engine.rank_path`` with the given beam (0: exact) and filter = train +
    valid + test.  Returns {length: {"count",
    "raw": {...}, "filtered": {...}}} with mean rank, MRR, Hits@1 and Hits@10
    (``rank_metrics``)."""
    hops = tuple(int(m) for m in hops)
    if not hops or min(hops) < 1:
        raise ValueError("hops must be positive")
    filt = np.concatenate([ds.train, ds.valid, ds.test]).astype(np.int32)
    out = {}
    for m in hops:
        anchors, paths, truth = path_query_set(ds, m, seed)
        if limit is not None:
            anchors, paths, truth = anchors[:limit], paths[:limit], truth[:limit]
        if len(anchors) == 0:
            raise ValueError("no test triple has a path of %d hops" % m)
        ranks = np.asarray(eng.rank_path(anchors, paths, truth, filt, beam=beam)).reshape(-1, 2)
        out[m] = {"count": int(len(anchors)), "raw": rank_metrics(ranks[:, 0]), "filtered": rank_metrics(ranks[:, 1])}
    return out


def mutual_pairs(ids, dist, found, entities=None):
    """The duplicate candidates of a kNN graph.  `ids`, `dist`, `found` are
    ``Engine.neighbors`` output; row q is the list of entities[q] (None: of
    entity q, as ``Engine.knn_graph`` returns it; an entity listed twice counts
    once, its first listing).  A pair (a, b), a < b, is mutual when b is among
    a's found neighbours and a among b's.  Returns (pairs int32[m, 2], dist
    float64[m]): the distance is the one listed in a's row, the order ascending
    (distance, a, b)."""
    ids = np.asarray(ids, dtype=np.int64)
    dist = np.asarray(dist, dtype=np.float64)
    found = np.asarray(found, dtype=np.int64).reshape(-1)
    nq, k = ids.shape
    ents = np.arange(nq, dtype=np.int64) if entities is None else np.asarray(entities, dtype=np.int64).reshape(-1)
    if len(ents) != nq:
        raise ValueError("entities and ids differ in length")
    if nq:
        _, first = np.unique(ents, return_index=True)
        keep = np.zeros(nq, bool)
        keep[first] = True
    else:
        keep = np.zeros(0, bool)
    live = (np.arange(k)[None, :] < found[:, None]) & keep[:, None]
    a = np.broadcast_to(ents[:, None], ids.shape)[live]
    b = ids[live]
    d = dist[live]
    span = int(max(ents.max(initial=0), ids.max(initial=0))) + 1
    edge = a * span + b
    back = b * span + a
    sel = (a < b) & np.isin(back, edge)
    a, b, d = a[sel], b[sel], d[sel]
    order = np.lexsort((b, a, d))
    return np.stack([a[order], b[order]], axis=1).astype(np.int32).reshape(-1, 2), d[order]


def duplicate_split(ds, count, seed=0):
    """Plant duplicates: `count` entities with at least 4 training triples are
    drawn (``numpy.random.default_rng(seed)``), each gets a twin with the id
    |E| + i (i its position among the drawn entities, ascending by id), and each
    training triple that mentions the entity is moved to the twin -- the entity
    replaced by the twin wherever the triple names it -- on a fair coin of the
    same stream; where the coins leave fewer than two triples on a side, the
    first triples of the other side, in file order, change over.  Valid and test
    stay.  Returns (Dataset with |E| + count entities and as many training
    triples as before, pairs int32[count, 2] of (original, twin))."""
    train = np.array(ds.train, dtype=np.int32).reshape(-1, 3)
    ne = int(ds.num_entities)
    mentions = np.bincount(np.concatenate([train[:, 0], train[train[:, 1] != train[:, 0], 1]]), minlength=ne)
    eligible = np.flatnonzero(mentions >= 4)
    if count < 0 or count > len(eligible):
        raise ValueError(f"{count} twins asked for, {len(eligible)} entities have at least 4 training triples")
    rng = np.random.default_rng(seed)
    chosen = np.sort(rng.choice(eligible, size=count, replace=False))
    pairs = np.stack([chosen, ne + np.arange(count)], axis=1).astype(np.int32).reshape(-1, 2)
    # (the mentions are read from the caller's triples: a twin never gets a twin of its own)
    src = np.asarray(ds.train, dtype=np.int32).reshape(-1, 3)
    for e, twin in pairs.tolist():
        rows = np.flatnonzero((src[:, 0] == e) | (src[:, 1] == e))
        move = rng.integers(0, 2, size=len(rows)).astype(bool)
        for side in (True, False):  # at least two moved, at least two kept
            short = 2 - int((move == side).sum())
            if short > 0:
                move[np.flatnonzero(move != side)[:short]] = side
        for i in rows[move].tolist():
            for slot in (0, 1):
                if src[i, slot] == e:
                    train[i, slot] = twin
    out = data.Dataset(ne + count, ds.num_relations, train, np.asarray(ds.valid), np.asarray(ds.test))
    return out, pairs


def duplicate_metrics(ids, dist, found, pairs, k):
    """``duplicate_detection``'s numbers from a kNN graph (``Engine.knn_graph``
    output, row = entity) and the planted (original, twin) pairs: recall@1 and
    recall@k of "the twin's original is among the twin's nearest", the mutual
    pairs of the graph, the planted pairs among them and their share, and the
    random baseline k / (|E| - 1)."""
    ids = np.asarray(ids)
    found = np.asarray(found).reshape(-1)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    ne = len(ids)
    hit1 = hitk = 0
    for orig, twin in pairs.tolist():
        row = ids[twin, :found[twin]]
        hit1 += int(len(row) > 0 and row[0] == orig)
        hitk += int(orig in row[:k].tolist())
    mp, md = mutual_pairs(ids, dist, found)
    planted = {(min(a, b), max(a, b)) for a, b in pairs.tolist()}
    got = [p for p in map(tuple, mp.tolist()) if p in planted]
    n = len(pairs)
    return {"k": int(k), "entities": int(ne), "planted": int(n),
            "recall@1": hit1 / n if n else None, "recall@k": hitk / n if n else None,
            "mutual": int(len(mp)), "mutual_planted": got,
            "mutual_share": len(got) / len(mp) if len(mp) else None,
            "baseline": k / (ne - 1) if ne > 1 else None}


def duplicate_detection(ds, model, dim, count, *, epochs, k=10, seed=0, relation=-1, rate=0.001, margin=1.0,
                        method=1, distance=0, batches=100, train_seed=7, schedule="ordered", device=0,
                        make_engine=Engine):
    """Which two known entities are the same thing?  The hold-out measure of
    ``Engine.knn_graph``: `count` duplicates are planted (``duplicate_split``
    with `seed`), the model is trained `epochs` epochs on the split set, the
    k-nearest-neighbour graph of all entities is built on the device in the
    entity space (or relation `relation`'s), and the planted pairs are looked up
    in it (``duplicate_metrics``).  Returns its dict with "pairs" added."""
    split, pairs = duplicate_split(ds, count, seed)
    eng = make_engine(model, dim, split.num_entities, split.num_relations, rate=rate, margin=margin, method=method,
                      distance=distance, batches=batches, seed=train_seed, transr_compat=False, device=device,
                      schedule=schedule)
    try:
        eng.upload_triples(split.train)
        ent, rel, _ = eng.init_params()
        if model in ("R", "transr", 2):
            eng.transr_seed(ent, rel)
        for _ in range(epochs):
            eng.train_epoch()
        eng.synchronize()
        ids, dist, found = eng.knn_graph(k, relation=relation)
    finally:
        eng.close()
    out = duplicate_metrics(ids, dist, found, pairs, k)
    out["pairs"] = pairs
    return out


# ------------------------------------------------------------ candidate lists

def candidate_metrics(ranks):
    """``rank_metrics`` plus "hits@3" of a column (or block) of ranks."""
    ranks = np.asarray(ranks, dtype=np.float64).reshape(-1)
    out = rank_metrics(ranks)
    out["hits@3"] = float((ranks <= 3).mean())
    return out


def side_queries(test):
    """Both one-sided queries of every test triple, interleaved: row 2i asks for
    the head of triple i (its tail, side 0, truth = the head), row 2i + 1 for the
    tail (its head, side 1, truth = the tail).  Returns int32 arrays (entities,
    relations, side, truth) of length 2 * ntest; ranks of these queries reshaped
    to [ntest, 4] are in ``Engine.rank_triples``' column order."""
    test = np.asarray(test, dtype=np.int32).reshape(-1, 3)
    nt = len(test)
    ent = np.empty(2 * nt, np.int32)
    truth = np.empty(2 * nt, np.int32)
    ent[0::2], ent[1::2] = test[:, 1], test[:, 0]
    truth[0::2], truth[1::2] = test[:, 0], test[:, 1]
    rel = np.repeat(test[:, 2], 2).astype(np.int32)
    side = np.tile(np.array([0, 1], np.int32), nt)
    return ent, rel, side, truth


def _candidate_report(ranks, counted):
    ranks = np.asarray(ranks, dtype=np.int64).reshape(-1, 2)
    counted = np.asarray(counted, dtype=np.int64).reshape(-1, 2)
    return {"raw": candidate_metrics(ranks[:, 0]), "filtered": candidate_metrics(ranks[:, 1]),
            "counted": {"raw": int(counted[:, 0].sum()), "filtered": int(counted[:, 1].sum())},
            "queries": int(len(ranks)), "ranks": ranks.reshape(-1, 4), "counted_per_query": counted}


def sampled_evaluation(eng, test, filt, negatives=500, seed=0):
    """Link prediction against sampled negatives (the fixed-negatives protocol
    of large benchmarks): every test triple is ranked on both sides
    (``side_queries``) among `negatives` entity ids per query, drawn uniformly
    with ``numpy.random.default_rng(seed)`` -- or among the ids given: an int
    array [2 * ntest, m] holds one list per query, a 1-d array one list that every
    query shares.  ``Engine.rank_candidates`` with filter `filt`.  Returns
    {"raw", "filtered"} -> mean rank, MRR, Hits@1/3/10 over both sides,
    "counted" -> the listings compared in all (raw, filtered), "queries",
    "ranks" int64[ntest, 4] (head raw, head filtered, tail raw, tail filtered)
    and "counted_per_query" int64[2 * ntest, 2]."""
    ent, rel, side, truth = side_queries(test)
    nq = len(ent)
    if nq == 0:
        raise ValueError("no test triples")
    if np.ndim(negatives) == 0:
        m = int(negatives)
        if m < 0:
            raise ValueError("negatives must not be negative")
        lists_of = np.random.default_rng(seed).integers(0, eng.ne, size=(nq, m), dtype=np.int32)
    else:
        lists_of = np.asarray(negatives, dtype=np.int32)
    if lists_of.ndim == 1:
        ranks, counted = eng.rank_candidates(ent, rel, side, truth, [lists_of], filt, lists=np.zeros(nq, np.int32))
    elif lists_of.ndim == 2 and len(lists_of) == nq:
        ranks, counted = eng.rank_candidates(ent, rel, side, truth, list(lists_of), filt)
    else:
        raise ValueError("negatives must be a count, one list, or one list per query (2 * ntest of them)")
    return _candidate_report(ranks, counted)


def slot_pools(triples, num_relations):
    """Per (relation, slot) the distinct entities seen there among `triples`,
    ascending: a list of 2 * num_relations int32 arrays, relation * 2 + slot
    (slot 0 = head, 1 = tail) -- classify_host.hpp's build_slot_pools."""
    t = np.asarray(triples, dtype=np.int64).reshape(-1, 3)
    pools = []
    for r in range(int(num_relations)):
        rows = t[t[:, 2] == r]
        pools.append(np.unique(rows[:, 0]).astype(np.int32))
        pools.append(np.unique(rows[:, 1]).astype(np.int32))
    return pools


def type_constrained_evaluation(eng, ds):
    """Type-constrained link prediction (Krompass et al. 2015): every test triple
    is ranked on both sides only against the entities observed in that slot of its
    relation in train + valid + test (``slot_pools``; one shared list per
    relation and slot, named by many queries), filter = train + valid + test.
    Returns {"constrained": ``sampled_evaluation``'s report, "unconstrained":
    {"raw", "filtered", "ranks"} from ``Engine.rank_triples`` on the same
    triples}."""
    known = np.concatenate([ds.train, ds.valid, ds.test]).astype(np.int32)
    test = np.asarray(ds.test, dtype=np.int32).reshape(-1, 3)
    ent, rel, side, truth = side_queries(test)
    if len(ent) == 0:
        raise ValueError("no test triples")
    pools = slot_pools(known, ds.num_relations)
    ranks, counted = eng.rank_candidates(ent, rel, side, truth, pools, known, lists=rel * 2 + side)
    full = np.asarray(eng.rank_triples(test, known), dtype=np.int64).reshape(-1, 4)
    return {"constrained": _candidate_report(ranks, counted),
            "unconstrained": {"raw": candidate_metrics(full[:, [0, 2]]), "filtered": candidate_metrics(full[:, [1, 3]]),
                              "ranks": full}}
