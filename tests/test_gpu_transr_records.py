"""The record pass of the pipelined transRNorm chain (kernels_transr_pipe.hpp
pipe_records): after a relation's walk its violators' pair records G become
da = -lr W G with the relation's final matrix, lane j holding row j of W_c in
registers and the G rows staged in LDS, a stage-full at a time.

Same method as tests/test_gpu_transr_walk.py (engine against oracle/parallel.py,
cons="chunk1": per epoch the same active count, loss within 1e-9 relative,
tables within 1e-9), with cases chosen for the record pass instead of the walk:

- one relation owning every record (ne=1500, nr=1, count=6000, dim 50): 232-344
  records a constraint call, more than one stage-full (164 at NP = 64) and no
  multiple of the four waves;
- the walk test's 6-relation hub set at dim 33 (NB = 3: wave 3 owns no column
  slice, NP = 48, lanes >= 48 idle), 64 (no pad columns) and 2 (one k-step);
- dim 50 on the 6-relation set with the stage capacity forced below a relation's
  record count (KB2E_RPAR_REC_CAP), so the multi-pass path runs at small size;
- three sub-batches, and two sub-batches with KB2E_SUB_OVERLAP=0 (everything in
  line on the batch stream), against the same model.

The model's own counters guard the coverage: records per constraint call.
"""
import numpy as np
import pytest

import oracle.parallel as par
from gpu_common import max_abs
from kb2e_amd import data
from kb2e_amd.engine import Engine
from oracle import orc

pytestmark = pytest.mark.gpu

ATOL = 1e-9
RATE = 0.01
EPOCHS = 2
ST = 8
SEED = 3


def _hub_dataset(ne=300, nr=6, count=4000, seed=5):
    """The hub set of tests/test_gpu_transr_walk.py: entity 0 heads about half the triples."""
    rng = np.random.default_rng(seed)
    h = np.where(rng.random(count) < 0.5, 0, rng.integers(1, ne, count))
    t = rng.integers(1, ne, count)
    r = rng.integers(0, nr, count)
    tr = np.unique(np.stack([h, t, r], 1).astype(np.int32), axis=0)
    tr = tr[rng.permutation(len(tr))]
    return data.Dataset(ne, nr, tr, tr[:0], tr[:0])


BIG = dict(ne=1500, nr=1, count=6000)
HUB = dict(ne=300, nr=6, count=4000)

# (id, data set, dim, batches, sub, environment, least records of the fullest constraint call)
CASES = [
    ("one_rel_b2_s1", BIG, 50, 2, 1, {}, 200),
    ("one_rel_b1_s2", BIG, 50, 1, 2, {}, 200),
    ("dim33_nb3", HUB, 33, 5, 2, {}, 20),
    ("dim64_no_pad", HUB, 64, 2, 2, {}, 20),
    ("dim2_one_kstep", HUB, 2, 2, 2, {}, 20),
    ("dim50_cap8", HUB, 50, 2, 2, {"KB2E_RPAR_REC_CAP": "8"}, 20),
    ("dim50_sub3", HUB, 50, 2, 3, {}, 20),
    ("dim50_sub2_no_overlap", HUB, 50, 2, 2, {"KB2E_SUB_OVERLAP": "0"}, 20),
]


@pytest.mark.parametrize("name,shape,dim,batches,sub,env,min_records", CASES, ids=[c[0] for c in CASES])
def test_transr_records(name, shape, dim, batches, sub, env, min_records, monkeypatch):
    """Compat energy, L1, two epochs; the records of every constraint call counted on the model."""
    ds = _hub_dataset(**shape)
    monkeypatch.setenv("KB2E_RPAR_ST", str(ST))
    monkeypatch.setenv("KB2E_RPAR_MFMA", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    calls = []  # records (violators) of every constraint call
    model_rounds, model_constraint = par.transr_norm_rounds, par.transr_constraint

    def counting_rounds(*args, **kw):
        calls[-1] += 1
        return model_rounds(*args, **kw)

    def counting_constraint(*args, **kw):
        calls.append(0)
        return model_constraint(*args, **kw)

    monkeypatch.setattr(par, "transr_norm_rounds", counting_rounds)
    monkeypatch.setattr(par, "transr_constraint", counting_constraint)
    m = orc.Model("R", dim, ds.num_entities, ds.num_relations, rate=RATE, distance=0, batches=batches,
                  transr_compat=True)
    m.set_triples(ds.train)
    orc.srand(SEED)
    m.prep_train()
    pe, pr, pw = m.tables()
    eng = Engine("R", dim, ds.num_entities, ds.num_relations, rate=RATE, distance=0, batches=batches, seed=SEED,
                 schedule="parallel", transr_compat=True, sub_batches=sub)
    eng.upload_triples(ds.train)
    e0, r0, w0 = eng.init_params()
    assert np.array_equal(e0, pe) and np.array_equal(r0, pr) and np.array_equal(w0, pw)
    eng.transr_seed(e0, r0)
    pe = pe / np.linalg.norm(pe, axis=1, keepdims=True)
    work = [np.zeros(dim), np.zeros(dim)]
    B = m.batch_size()
    for ep in range(EPOCHS):
        si, sj, side = m.sample_stream(B * batches)
        lo, ao = par.transr_parallel_batches(pe, pr, pw, ds.train, si, sj, side, B, batches, rate=RATE, l1=True,
                                             compat=True, work=work, St=ST, cons="chunk1", sub=sub)
        lg, ag = eng.train_epoch()
        assert ag == ao, (ep, ag, ao)
        assert abs(lg - lo) <= 1e-9 * max(1.0, abs(lo)), (ep, lg, lo)
        ge, gr, gw = eng.download_params()
        errs = (max_abs(ge, pe), max_abs(gr, pr), max_abs(gw, pw))
        print(f"{name} epoch {ep}: active {ag}, max|diff| {errs}")
        assert max(errs) < ATOL, (ep, errs)
    eng.close()
    # coverage guard: the constraint calls of the two epochs and their records
    print(f"{name}: records a constraint call {calls}")
    assert len(calls) == EPOCHS * batches * sub, calls
    assert max(calls) >= min_records, calls
    assert np.isfinite(pe).all() and np.isfinite(pw).all()
