"""Shared helpers for the GPU parity tests (tests/ only)."""
import json
import os

import numpy as np

from conftest import GOLDEN
from kb2e_amd import data
from kb2e_amd.engine import SAMPLER_GLIBC, SAMPLER_REPLAY, Engine
from oracle import orc

MANIFEST = json.load(open(os.path.join(GOLDEN, "manifest.json")))

# FP64 engine vs the FP64 reference: same operations in the same order per
# element; only the order of the 64-lane sums (energies, vector lengths)
# differs, which moves results by a few ulps per update.
F64_ATOL = 1e-11
# Multi-epoch runs with the coupling loops (TransH orthogonality, TransR
# transRNorm) iterating: those loops divide by running sums and amplify the
# ulp-level differences of the 64-lane sums.  An ordering error would show up
# at the learning-rate scale (1e-3..1e-2), eight orders above this.
F64_ATOL_COUPLED = 1e-9
# FP32 engine vs FP64 reference over one epoch of the tiny set.
F32_ATOL = 2e-4


def tiny():
    return data.load(os.path.join(GOLDEN, "tiny"))


def golden_engine(name, precision=64, sampler=SAMPLER_GLIBC, schedule="ordered"):
    run = MANIFEST["runs"][name]
    f = run["flags"]
    ds = tiny()
    eng = Engine(run["model"], f["size"], ds.num_entities, ds.num_relations, rate=f["rate"], margin=f["margin"],
                 method=f["method"], distance=f["distance"], batches=f["batches"], seed=f["seed"],
                 precision=precision, sampler=sampler, transr_compat=not run["transr_fixed"], schedule=schedule)
    eng.upload_triples(ds.train)
    init = eng.init_params()
    if run["model"] == "R":
        sd = os.path.join(GOLDEN, "transe_seed_unif")
        ent = data.read_table(os.path.join(sd, "entity2vec.unif"), ds.num_entities, f["size"])
        rel = data.read_table(os.path.join(sd, "relation2vec.unif"), ds.num_relations, f["size"])
        eng.transr_seed(ent, rel)
    return eng, run, ds, init


def oracle_model(kind, ds, dim, **kw):
    m = orc.Model(kind, dim, ds.num_entities, ds.num_relations, **kw)
    m.set_triples(ds.train)
    return m


def max_abs(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)))) if np.size(a) else 0.0


# ---------------------------------------------------------------- training drivers
#
# One reference run (`*_reference`), then the engine against it (`*_vs_*`).  A
# reference is a plain record -- the init tables and, per epoch, (loss, active,
# tables) -- so the tests that run one case through several kernel paths compute
# it once and hand it to every variant (`ref=`); nothing writes to it.  Every
# driver returns {"active": [...], "errs": [...], "worst": largest table error of
# any epoch} and, with keep=True, the open engine under "eng".

# PARALLEL TransE: the CPU model follows the same arithmetic (L1 deltas as integer
# sign counts), so the bar is the ulp-level difference of the 64-lane norm sums.
P_ATOL = 1e-11


def _compare_epochs(eng, ref, atol, before, keep):
    out = {"active": [], "errs": [], "worst": 0.0}
    try:
        if before is not None:
            before(eng)
        for ep, (lo, ao, tabs) in enumerate(ref["epochs"]):
            lg, ag = eng.train_epoch()
            assert ag == ao, (ep, ag, ao)
            assert abs(lg - lo) <= 1e-9 * max(1.0, abs(lo)), (ep, lg, lo)
            errs = tuple(max_abs(g, t) for g, t in zip(eng.download_params(), tabs) if t is not None)
            assert max(errs) < atol, (ep, errs)
            out["active"].append(ag)
            out["errs"].append(errs)
            out["worst"] = max(out["worst"], max(errs))
    except BaseException:
        eng.close()
        raise
    if keep:
        out["eng"] = eng
    else:
        eng.close()
    return out


def ordered_reference(kind, ds, dim, epochs, *, distance=0, method=1, batches=20, rate=0.01, seed=3):
    """`epochs` epochs of the C oracle (oracle/orc.c) from orc.srand(seed); "fired" counts
    the iterations of the coupling loops (orc_site_iterations) over the run."""
    m = oracle_model(kind, ds, dim, rate=rate, margin=1.0, method=method, distance=distance, batches=batches)
    orc.srand(seed)
    m.prep_train()
    ref = {"init": m.tables(), "epochs": []}
    L = orc.lib()
    before = [L.orc_site_iterations(s) for s in range(3)]
    for _ in range(epochs):
        lo, ao = m.train_epoch()
        ref["epochs"].append((lo, ao, m.tables()))
    ref["fired"] = sum(L.orc_site_iterations(s) - before[s] for s in range(3))
    return ref


def ordered_vs_oracle(kind, ds, dim, epochs, *, distance=0, method=1, batches=20, rate=0.01, seed=3, atol=F64_ATOL,
                      ref=None, before=None, keep=False):
    """The ORDERED engine against the C oracle: bit-equal init tables, then per epoch
    equal active counts, loss within 1e-9 relative, every table within `atol`."""
    if ref is None:
        ref = ordered_reference(kind, ds, dim, epochs, distance=distance, method=method, batches=batches, rate=rate,
                                seed=seed)
    assert len(ref["epochs"]) == epochs
    eng = Engine(kind, dim, ds.num_entities, ds.num_relations, rate=rate, margin=1.0, method=method,
                 distance=distance, batches=batches, seed=seed)
    eng.upload_triples(ds.train)
    for g, t in zip(eng.init_params(), ref["init"]):
        assert (g is None and t is None) or np.array_equal(g, t)
    return _compare_epochs(eng, ref, atol, before, keep)


def parallel_reference(kind, ds, dim, epochs, *, distance=0, method=1, batches=20, rate=0.01, seed=3, orth_min=None):
    """`epochs` epochs of the PARALLEL schedule's CPU model (oracle/parallel.py) on the C
    oracle's init draws and sample stream."""
    from oracle.parallel import ORTH_REL_MIN, transe_parallel_batches, transh_parallel_batches
    m = orc.Model(kind, dim, ds.num_entities, ds.num_relations, rate=rate, method=method, distance=distance,
                  batches=batches)
    m.set_triples(ds.train)
    orc.srand(seed)
    m.prep_train()
    pe, pr, pw = m.tables()
    ref = {"init": (pe.copy(), pr.copy(), None if pw is None else pw.copy()), "epochs": []}
    B = m.batch_size()
    state = {}  # TransH: the previous batch's flagged samples, across epochs as in the engine
    for _ in range(epochs):
        si, sj, side = m.sample_stream(B * batches)
        if kind == "E":
            lo, ao = transe_parallel_batches(pe, pr, ds.train, si, sj, side, B, batches, rate=rate, l1=distance == 0)
        else:
            assert kind == "H", kind
            lo, ao = transh_parallel_batches(pe, pr, pw, ds.train, si, sj, side, B, batches, rate=rate, state=state,
                                             orth_rel_min=ORTH_REL_MIN if orth_min is None else orth_min)
        ref["epochs"].append((lo, ao, (pe.copy(), pr.copy(), None if pw is None else pw.copy())))
    return ref


def parallel_vs_model(kind, ds, dim, epochs, *, distance=0, method=1, batches=20, rate=0.01, seed=3, atol=P_ATOL,
                      orth_min=None, ref=None, before=None, keep=False):
    """The PARALLEL engine (TransE, TransH) against oracle/parallel.py; the same checks
    as ordered_vs_oracle.  `orth_min` tells the TransH model the gate the engine was
    given in KB2E_HPAR_ORTH_MIN (None: the default of both)."""
    if ref is None:
        ref = parallel_reference(kind, ds, dim, epochs, distance=distance, method=method, batches=batches, rate=rate,
                                 seed=seed, orth_min=orth_min)
    assert len(ref["epochs"]) == epochs
    eng = Engine(kind, dim, ds.num_entities, ds.num_relations, rate=rate, method=method, distance=distance,
                 batches=batches, seed=seed, schedule="parallel")
    eng.upload_triples(ds.train)
    for g, t in zip(eng.init_params(), ref["init"]):
        assert (g is None and t is None) or np.array_equal(g, t)
    return _compare_epochs(eng, ref, atol, before, keep)
