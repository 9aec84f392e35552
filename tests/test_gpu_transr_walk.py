"""The pipelined transRNorm walker (kernels_transr_pipe.hpp) on dense chunks.

The tiny set gives the chain a violator or two a chunk.  The hub set at rate
0.01 gives every relation 80-200 pairs a sub-batch with about a dozen violators
a 32-pair chunk, so the walker's violator loop (pick, V = p_v K0, the wave
sums, the rounds, the later rows' move, the publish to the helper waves) runs
hundreds of times a case, the rounds loop after the four straight-line rounds
included.  The engine is checked against the CPU model (oracle/parallel.py,
cons="chunk1") as tests/test_gpu_parallel.py does: per epoch the same active
count, loss within 1e-9 relative, tables within 1e-9.

Widths (KS = ceil(n / 4) k-steps, row halves of 2 KS columns, NP = 16
ceil(4 KS / 16)): 2 and 4 have one k-step; 13 has 4 KS = NP; 50 is the
headline (zero columns inside the second half, 12 LDS-only pad columns); 61 has
three pad columns at KS = 16; 64 has none.
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
RATE = 0.01  # (0.05 diverges in the model)
EPOCHS = 2
ST = 8
SEED = 3


def _hub_dataset(ne=300, nr=6, count=4000, seed=5):
    """The hub set of tests/test_gpu_parallel.py: entity 0 heads about half the triples."""
    rng = np.random.default_rng(seed)
    h = np.where(rng.random(count) < 0.5, 0, rng.integers(1, ne, count))
    t = rng.integers(1, ne, count)
    r = rng.integers(0, nr, count)
    tr = np.unique(np.stack([h, t, r], 1).astype(np.int32), axis=0)
    tr = tr[rng.permutation(len(tr))]
    return data.Dataset(ne, nr, tr, tr[:0], tr[:0])


@pytest.mark.parametrize("dim,batches,sub", [(2, 5, 2), (4, 5, 1), (13, 5, 2), (13, 2, 1), (50, 5, 2), (50, 2, 2),
                                             (61, 5, 2), (64, 2, 2)])
def test_transr_walk_dense_chunks(dim, batches, sub, monkeypatch):
    """Compat energy, L1, two epochs on the hub set; the model's own counters say
    that the case still exercises the walker (>= 500 violators, one with more
    than four rounds)."""
    ds = _hub_dataset()
    monkeypatch.setenv("KB2E_RPAR_ST", str(ST))
    monkeypatch.setenv("KB2E_RPAR_MFMA", "1")
    rounds = []
    model_rounds = par.transr_norm_rounds

    def recording_rounds(*args, **kw):
        G, m = model_rounds(*args, **kw)
        rounds.append(m)
        return G, m

    monkeypatch.setattr(par, "transr_norm_rounds", recording_rounds)
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
    stats = {}
    B = m.batch_size()
    for ep in range(EPOCHS):
        si, sj, side = m.sample_stream(B * batches)
        lo, ao = par.transr_parallel_batches(pe, pr, pw, ds.train, si, sj, side, B, batches, rate=RATE, l1=True,
                                             compat=True, work=work, St=ST, cons="chunk1", stats=stats, sub=sub)
        lg, ag = eng.train_epoch()
        assert ag == ao, (ep, ag, ao)
        assert abs(lg - lo) <= 1e-9 * max(1.0, abs(lo)), (ep, lg, lo)
        ge, gr, gw = eng.download_params()
        errs = (max_abs(ge, pe), max_abs(gr, pr), max_abs(gw, pw))
        print(f"dim {dim} batches {batches} sub {sub} epoch {ep}: active {ag}, max|diff| {errs}")
        assert max(errs) < ATOL, (ep, errs)
    eng.close()
    # coverage guard: the case walks many violators, one past the four straight-line rounds
    print(f"dim {dim} batches {batches} sub {sub}: fired {stats.get('fired', 0)}, most rounds {max(rounds, default=0)}")
    assert stats.get("fired", 0) >= 500, stats
    assert max(rounds, default=0) > 4, max(rounds, default=0)
