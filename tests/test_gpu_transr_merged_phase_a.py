"""Merged phase A of PARALLEL TransR sub-batches (engine_transr_parallel.inc
run_batch_transr_merged): on the n <= 64 wave path the projection, scan-sums,
scan-energy and gradient kernels run once a batch for all its sub-batches, in line
on the live tables, instead of once a sub-batch on start-of-batch copies
(KB2E_RPAR_MERGE_A=0).

Both paths compute the same thing by construction -- the same additions in the same
order, the compat scan's carried work vectors included -- so the bar between them is
bit identity: per epoch the same loss and active count, np.array_equal tables.  Two
epochs, so that the carried work vectors and the pair-table rotation cross an epoch
boundary.  Cases:

- tiny(), n = 50, compat, L1: sub 2 at 9 batches and sub 3 at 7 (ragged last
  sub-batch, partial last chunk);
- tiny(), n = 20, fixed energy, L2, sub 3: no scan, transr_proj_wave_kernel fills the
  pair tables;
- the hub set of test_gpu_transr_records.py cut to exactly 1,280 triples, 2 batches,
  n = 50, compat: sub 2 (Bs = 320: 10 full chunks) and sub 4 (Bs = 160: 5), every
  sub-batch ending on a chunk boundary;
- synthetic "small", n = 50, compat, 10 batches, sub 2, one epoch: ~47 chunks a
  sub-batch, several 16-chunk thread groups of the prefix sum take part;
- n = 64 and n = 33 on tiny(), sub 2 (other k-step counts);
- one FP32 case.

The 1,280-triple set at sub 2 also runs against oracle/parallel.py (existing tests
hold no chunk-aligned sub-batch), and device_bytes() guards the coverage: the merged
path holds no start-of-batch copies, so it is smaller; were the switch ignored the two
would be equal.
"""
import numpy as np
import pytest

import oracle.parallel as par
from gpu_common import max_abs, tiny
from kb2e_amd import data
from kb2e_amd.engine import Engine
from oracle import orc

pytestmark = pytest.mark.gpu

RATE = 0.01
SEED = 3


def _hub1280():
    """The hub set of tests/test_gpu_transr_records.py (entity 0 heads about half the
    triples, 6 relations), cut to exactly 1,280 triples."""
    rng = np.random.default_rng(5)
    ne, nr, count = 300, 6, 4000
    h = np.where(rng.random(count) < 0.5, 0, rng.integers(1, ne, count))
    t = rng.integers(1, ne, count)
    r = rng.integers(0, nr, count)
    tr = np.unique(np.stack([h, t, r], 1).astype(np.int32), axis=0)
    tr = tr[rng.permutation(len(tr))][:1280]
    assert len(tr) == 1280
    return data.Dataset(ne, nr, tr, tr[:0], tr[:0])


def _engine(ds, dim, batches, sub, *, compat, distance, precision=64):
    eng = Engine("R", dim, ds.num_entities, ds.num_relations, rate=RATE, distance=distance, batches=batches, seed=SEED,
                 schedule="parallel", transr_compat=compat, sub_batches=sub, precision=precision)
    eng.upload_triples(ds.train)
    e0, r0, _ = eng.init_params()
    eng.transr_seed(e0, r0)
    return eng


def _run(ds, dim, batches, sub, epochs, merged, monkeypatch, **kw):
    monkeypatch.setenv("KB2E_RPAR_MERGE_A", "1" if merged else "0")
    eng = _engine(ds, dim, batches, sub, **kw)
    stats = [eng.train_epoch() for _ in range(epochs)]
    tables = eng.download_params()
    nbytes = eng.device_bytes()
    eng.close()
    return stats, tables, nbytes


_DATASETS = {"tiny": tiny, "hub1280": _hub1280, "small": lambda: data.synthetic("small", seed=1)}

# (id, data set, dim, batches, sub, epochs, compat, distance, precision)
CASES = [
    ("tiny_n50_compat_sub2_b9", "tiny", 50, 9, 2, 2, True, 0, 64),
    ("tiny_n50_compat_sub3_b7", "tiny", 50, 7, 3, 2, True, 0, 64),
    ("tiny_n20_fixed_l2_sub3", "tiny", 20, 10, 3, 2, False, 1, 64),
    ("hub1280_n50_compat_sub2", "hub1280", 50, 2, 2, 2, True, 0, 64),
    ("hub1280_n50_compat_sub4", "hub1280", 50, 2, 4, 2, True, 0, 64),
    ("small_n50_compat_sub2_b10", "small", 50, 10, 2, 1, True, 0, 64),
    ("tiny_n64_compat_sub2", "tiny", 64, 9, 2, 2, True, 0, 64),
    ("tiny_n33_compat_sub2", "tiny", 33, 9, 2, 2, True, 0, 64),
    ("tiny_n50_compat_sub2_fp32", "tiny", 50, 9, 2, 2, True, 0, 32),
]


@pytest.mark.parametrize("name,dsname,dim,batches,sub,epochs,compat,distance,precision", CASES,
                         ids=[c[0] for c in CASES])
def test_merged_phase_a_bit_identical(name, dsname, dim, batches, sub, epochs, compat, distance, precision,
                                      monkeypatch):
    """Merged phase A against phase A per sub-batch: equal losses and active counts
    every epoch, equal tables bit for bit."""
    ds = _DATASETS[dsname]()
    kw = dict(compat=compat, distance=distance, precision=precision)
    s_old, t_old, _ = _run(ds, dim, batches, sub, epochs, False, monkeypatch, **kw)
    s_new, t_new, _ = _run(ds, dim, batches, sub, epochs, True, monkeypatch, **kw)
    print(f"{name}: per sub-batch {s_old}, merged {s_new}")
    for ep, ((l0, a0), (l1, a1)) in enumerate(zip(s_old, s_new)):
        assert a0 == a1, (ep, a0, a1)
        assert l0 == l1, (ep, l0, l1)
    for which, t0, t1 in zip(("entities", "relations", "matrices"), t_old, t_new):
        assert np.array_equal(t0, t1), (which, max_abs(t0, t1))
    assert all(np.isfinite(t).all() for t in t_new)


def test_merged_phase_a_vs_model_chunk_aligned(monkeypatch):
    """The 1,280-triple set, 2 batches, sub 2 (every sub-batch 10 full scan chunks)
    against oracle/parallel.py, the method of test_gpu_parallel._transr_vs_model: equal
    active count, loss within 1e-9 relative, tables within 1e-9."""
    ds = _hub1280()
    dim, batches, sub, St = 50, 2, 2, 8
    monkeypatch.setenv("KB2E_RPAR_ST", str(St))
    monkeypatch.setenv("KB2E_RPAR_MFMA", "1")
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
    assert B == 640
    for ep in range(2):
        si, sj, side = m.sample_stream(B * batches)
        lo, ao = par.transr_parallel_batches(pe, pr, pw, ds.train, si, sj, side, B, batches, rate=RATE, l1=True,
                                             compat=True, work=work, St=St, cons="chunk1", sub=sub)
        lg, ag = eng.train_epoch()
        assert ag == ao, (ep, ag, ao)
        assert abs(lg - lo) <= 1e-9 * max(1.0, abs(lo)), (ep, lg, lo)
        ge, gr, gw = eng.download_params()
        errs = (max_abs(ge, pe), max_abs(gr, pr), max_abs(gw, pw))
        print(f"epoch {ep}: active {ag}, max|diff| {errs}")
        assert max(errs) < 1e-9, (ep, errs)
    eng.close()


def test_merged_phase_a_holds_no_table_copies(monkeypatch):
    """Coverage guard: at sub 2 the merged path allocates less than the per-sub-batch
    path (no start-of-batch copies of the three tables, one export set).  Were
    KB2E_RPAR_MERGE_A ignored the two figures would be equal."""
    ds = tiny()
    kw = dict(compat=True, distance=0)
    _, tabs, b_old = _run(ds, 50, 9, 2, 1, False, monkeypatch, **kw)
    _, _, b_new = _run(ds, 50, 9, 2, 1, True, monkeypatch, **kw)
    ld = (50 + 1) // 2 * 2  # rows are padded to an even length on the device
    copies = sum(int(np.prod(t.shape[:-1])) * ld * 8 for t in tabs)
    print(f"device bytes: per sub-batch {b_old}, merged {b_new}, difference {b_old - b_new}; "
          f"one copy of the three tables is about {copies}")
    assert b_new < b_old, (b_new, b_old)
