"""FP32 training kernels, one batch at a time, element by element against the
FP64 oracle (tests/fp32_step.py holds the driver, the guards and the cases).

The float builds have geometry of their own -- the ORDERED TransR owner keeps its
matrix in LDS up to n = 195 (137 in FP64), transr_owner_reg_kernel<float, 20|32|
50|64> are instantiations of their own, PARALLEL FP32 TransR takes the generic
chain and the wide kernels, and every owner sizes its LDS by sizeof(T) -- and the
epoch-long FP32 tests can only be statistical (hinge decisions flip at the margin
and the dynamics diverge).  Over ONE batch that does not hold: every energy,
hinge decision and L1 sign comes from the batch-start tables.  So each case runs
three batches in lock step: the reference takes the engine's (float) tables,
draws the same samples from the same glibc stream, and both run the batch.

Guards, asserted on the reference's own numbers, never skipped on, nothing left
out of the comparison: the smallest hinge slack |E+ + margin - E-| of any sample
is >= 1e-4 and, under L1, the smallest |x| of a sign argument of an active sample
is >= 1e-6.  The committed orc.srand seeds were chosen on the CPU
(fp32_step.find_seeds; test_fp32_step_model.py re-checks them).

Bars: equal active counts per batch; batch loss within 1e-5 relative; every table
element within 1e-3 * rate = 1e-5 absolute.  A wrong order, a missed element or a
skipped relation shows at the learning-rate scale (a batch moves touched rows by
>= 7e-2, three orders above the bar); FP32 rounding is 2^-24 a store with <= 31
touches a row and wave sums of n <= 512 terms, a few 1e-6.

All cases: precision 32, data.synthetic("tiny", seed=5), B = 100 (ord-R512-L1: 50),
rate 0.01, bern, TransR with the fixed (zeroed) energy.

Out of scope: TransR's compat energy.  Its energies accumulate over the whole
batch, so the FP32 slack grows along the chain and a fixed decision guard says
nothing; the statistical tests (test_gpu_transr.py, test_gpu_parallel.py) keep
covering it.

Observed maxima on an MI355X (largest |element difference| of any table over the
three batches; every case prints its own, run with -s); the bar is 1e-5 everywhere,
no case needed a raised one:

  ord-E17-L1    2.80e-08   ord-R20-L1    5.85e-07   par-E17-L1             1.37e-08
  ord-E130-L2   9.43e-09   ord-R50-L1    4.42e-07   par-E130-L1            1.16e-08
  ord-E200-L1   1.94e-08   ord-R33-L1    4.04e-07   par-H33-L1             5.79e-08
  ord-H33-L1    2.67e-07   ord-R64-L1    6.80e-07   par-H130-L1            4.72e-08
  ord-H130-L1   2.33e-07   ord-R100-L1   8.57e-07   par-R20-L1-sub1        9.01e-08
  ord-H260-L1   1.63e-07   ord-R190-L1   4.56e-06   par-R50-L1-sub1        6.30e-08
                           ord-R200-L1   7.56e-07   par-R100-L1-sub1       5.46e-08
                           ord-R512-L1   3.79e-06   par-R128-L1-sub1       1.32e-07
                           ord-R50-L2    5.86e-07   par-R160-L1-sub1       2.24e-07
                                                    par-R260-L1-sub1       6.45e-08
                                                    par-R50-L1-subdef      9.72e-08
                                                    par-R50-L1-sub1-mfma1  6.30e-08
                                                    par-R50-L1-sub1-mfma0  7.14e-08

and the four-chunk float builds of TransE (257 <= n <= 512, L2; fp32_step.py says why
not L1):

  ord-E300-L2   5.41e-09   par-E257-L2   5.56e-10
  ord-E385-L2   4.14e-09   par-E300-L2   5.62e-10
  ord-E512-L2   3.16e-09   par-E385-L2   4.80e-10
                           par-E512-L2   4.24e-10

The largest sit in TransR's matrices at the widest rows (n = 190 in LDS, n = 512
from L2), a few 1e-6 as the rounding argument predicts, 2x below the bar.  (PARALLEL
FP32 TransR runs its transRNorm chain in double arithmetic on float storage, hence
its 1e-7.)

Found by ord-H260-L1: at 257 <= n <= 384 the TransE / TransH kernels wrote eight
sign words an update into a buffer laid out for six, so each update's last words
cleared the next one's first (elements 0..127 took the sign -1): 0.2 off in one
batch, in FP64 as well.  Fixed in setup_buffers (engine.hip); the FP64 regressions
are test_gpu_transe / test_gpu_transh test_oracle_parity_three_chunks.

ord-R512-L1 takes about 6 s, 3 s of it the reference's rejection sampler drawing
the 512-wide initial tables, once on each side; every other case is under 1.5 s.
"""
import pytest

import fp32_step as fs

pytestmark = pytest.mark.gpu


def _run(case, monkeypatch):
    for name, value in case.env:
        monkeypatch.setenv(name, value)
    eng = fs.make_engine(case, fs.dataset())
    try:
        worst, rows = 0.0, []
        for res in fs.lockstep(case, engine=eng):
            rows.append(res)
            print(f"fp32-step {case.id} batch {res.batch}: active {res.got[1]}/{res.ref[1]} "
                  f"loss rel {abs(res.got[0] - res.ref[0]) / abs(res.ref[0]):.2e} slack {res.pre['slack']:.2e} "
                  f"min|x| {res.pre['min_abs_x']:.2e} moved {res.moved:.2e} "
                  + " ".join(f"{k} {v[0]:.2e}@{v[1]}" for k, v in res.diffs.items()))
            worst = max(worst, max(v[0] for v in res.diffs.values()))
        print(f"fp32-step {case.id} max {worst:.2e}")
        for res in rows:
            fs.check_batch(case, res)
        assert len(rows) == fs.NB
    finally:
        eng.close()


@pytest.mark.parametrize("case", fs.ORDERED_CASES, ids=lambda c: c.id)
def test_ordered_fp32_batch_parity(case, monkeypatch):
    """TransE n = 17 (L1), 130 (L2: two chunks, the second nearly empty), 200, and L2
    on the four-chunk build at 300 (three chunks), 385 and 512 (four, the last full);
    TransH n = 33 (one chunk, ragged), 130 (two), 260 (four, ragged last); TransR
    n = 20, 50 (named register instantiations), 33 (reg<64>), 64, 100 (LDS owner),
    190 / 200 (either side of the FP32 LDS limit of 195), 512 (B = 50), and L2 at 50."""
    _run(case, monkeypatch)


@pytest.mark.parametrize("case", fs.PARALLEL_CASES, ids=lambda c: c.id)
def test_parallel_fp32_batch_parity(case, monkeypatch):
    """Against oracle/parallel.py from the engine's own tables: TransE n = 17, 130, and
    L2 at 257, 300, 385, 512 (transe_score_kernel / transe_apply_kernel<float, 4, false>);
    TransH n = 33, 130; TransR n = 20, 50, 100 (generic chain), 128, 160, 260 (wide
    kernels) with sub_batches = 1, n = 50 also at the default sub-batch count and
    with KB2E_RPAR_MFMA both ways."""
    _run(case, monkeypatch)
