"""TransE and TransH training at two and four chunks a lane, both schedules.

The row kernels are built for 1, 2 and 4 chunks of 128 elements a lane
(engine.hip setup_buffers; three chunks run the four-chunk build).  This file
runs the four-chunk build where the other training tests do not: PARALLEL at
every width above 256, ORDERED at 385..512 (four real chunks; at 512 no lane of
any chunk is masked), both sides of every chunk edge (128 | 129, 256 | 257,
384 | 385, and 511, an odd width in the top chunk with ld = n + 1), and the
long-segment kernels with their thresholds set, not left to how the data falls.

References, as everywhere: ORDERED against oracle/orc.c, PARALLEL against
oracle/parallel.py, both FP64 on the CPU from the same glibc stream
(gpu_common.ordered_vs_oracle / parallel_vs_model, the drivers of
test_gpu_transe.py, test_gpu_transh.py and test_gpu_parallel.py).  Bars, those
tests' own: equal hinge-active counts and loss within 1e-9 relative every
epoch; tables within F64_ATOL (ORDERED TransE), F64_ATOL_COUPLED (ORDERED
TransH), P_ATOL (PARALLEL TransE), 1e-9 (PARALLEL TransH).

All cases: data.synthetic("tiny", seed=5) (200 entities, 10 relations, 3,000
triples), two epochs, rate 0.01, bern.  Every L1 case also asserts that the
hinge still decides something after the second epoch (active strictly between 0
and the sample count; the L2 cases keep every sample active on this data, which
is why L1 carries every width).  A reference is computed once for each (model,
schedule, width, distance, batches) and shared, unchanged, by the variants of
part 2.  Every case prints its largest table error (run with -s).

Observed on an MI355X (largest |table difference| of any epoch, every width and
variant of the group; no case failed and no kernel needed a fix):

  ORDERED TransE    L1 1.4e-16 .. 3.1e-16, L2 0 (bit-equal)       bar 1e-11
    long segments   1.5e-16 .. 3.3e-16 (fold_long, Gram, plain)   bar 1e-11
  PARALLEL TransE   L1 5.6e-17 .. 8.3e-17, L2 9.0e-17 .. 2.8e-16  bar 1e-11
    KB2E_APPLY_LONG the same figures at 0, 1 and 64
  ORDERED TransH    4.8e-15 .. 1.1e-14                            bar 1e-9
  PARALLEL TransH   1.1e-16 .. 4.2e-16, every n = 300 variant 2.5e-16   bar 1e-9
    relation pass   3 of 20 batches at n = 128, 129 (default gate); 17, 15, 14, 12,
                    11, 6, 5 at 256, 257, 300, 384, 385, 511, 512 (gate 8)

Every case takes under 2.5 s, the TransH cases at 511 and 512 the longest (the CPU
references' share).

FP32 at these widths, one batch at a time: fp32_step.py / test_gpu_fp32_step.py.
"""
import pytest

from gpu_common import (F64_ATOL, F64_ATOL_COUPLED, P_ATOL, ordered_reference, ordered_vs_oracle, parallel_reference,
                        parallel_vs_model)
from kb2e_amd import data

pytestmark = pytest.mark.gpu

EPOCHS = 2
RATE = 0.01
H_PAR_ATOL = 1e-9           # test_gpu_parallel.py _transh_vs_model
SEED_E, SEED_H_ORD, SEED_H_PAR = 3, 5, 3  # the extended tests' own seeds

ORD_WIDTHS = [128, 129, 256, 257, 385, 511, 512]
PAR_WIDTHS = [128, 129, 256, 257, 300, 384, 385, 511, 512]
L2_WIDTHS = [257, 385, 512]
E_ORD_CASES = [(n, 0) for n in ORD_WIDTHS] + [(n, 1) for n in L2_WIDTHS]
E_PAR_CASES = [(n, 0) for n in PAR_WIDTHS] + [(n, 1) for n in L2_WIDTHS]

_DS = []
_REFS = {}


def _ds():
    if not _DS:
        _DS.append(data.synthetic("tiny", seed=5))
    return _DS[0]


def _ref(schedule, kind, dim, distance, batches, seed, **kw):
    """The reference run of a case, computed once; the drivers only read it."""
    key = (schedule, kind, dim, distance, batches, seed, tuple(sorted(kw.items())))
    if key not in _REFS:
        make = ordered_reference if schedule == "ordered" else parallel_reference
        _REFS[key] = make(kind, _ds(), dim, EPOCHS, distance=distance, batches=batches, rate=RATE, seed=seed, **kw)
    return _REFS[key]


def _run(schedule, kind, dim, *, distance=0, batches=10, seed, atol, before=None, keep=False, tag="", **kw):
    ref = _ref(schedule, kind, dim, distance, batches, seed, **kw)
    drive = ordered_vs_oracle if schedule == "ordered" else parallel_vs_model
    out = drive(kind, _ds(), dim, EPOCHS, distance=distance, batches=batches, rate=RATE, seed=seed, atol=atol,
                ref=ref, before=before, keep=keep, **kw)
    samples = (len(_ds().train) // batches) * batches
    l1 = kind == "H" or distance == 0
    print(f"wide-rows {schedule[:3]}-{kind}{dim}-{'L1' if l1 else 'L2'}{tag}: active {out['active']} of {samples}, "
          f"max table error {out['worst']:.2e} (bar {atol:.0e})")
    if l1:
        assert 0 < out["active"][-1] < samples, (out["active"], samples)
    out["ref"] = ref
    return out


# ------------------------------------------------ 1. FP64 parity across the chunk edges

@pytest.mark.parametrize("dim,distance", E_ORD_CASES)
def test_transe_ordered_chunk_edges(dim, distance):
    """transe_score_kernel / transe_fold_kernel<double, CH> at CH = 1 | 2 (128 | 129),
    2 | 4 (256 | 257) and four real chunks (385, 511, 512)."""
    _run("ordered", "E", dim, distance=distance, seed=SEED_E, atol=F64_ATOL)


@pytest.mark.parametrize("dim,distance", E_PAR_CASES)
def test_transe_parallel_chunk_edges(dim, distance):
    """transe_score_kernel<double, CH, *, true> and transe_apply_kernel<double, CH, *>:
    CH = 4 from 257 on (the event sign words, ev_words, at that build's stride)."""
    _run("parallel", "E", dim, distance=distance, seed=SEED_E, atol=P_ATOL)


@pytest.mark.parametrize("dim", ORD_WIDTHS)
def test_transh_ordered_chunk_edges(dim):
    """The ORDERED TransH owner kernels (kernels_relowner.hpp); the orthogonality loop
    must iterate in the oracle run being matched, as in test_oracle_parity_with_coupling."""
    out = _run("ordered", "H", dim, seed=SEED_H_ORD, atol=F64_ATOL_COUPLED)
    assert out["ref"]["fired"] > 0, "the coupling loop never iterated: test does not exercise the dataflow"


def _orth_gate(dim):
    """KB2E_HPAR_ORTH_MIN for a width (None: the default, 64).  The relation pass of a
    batch runs when the previous batch's normOrth work -- orth_norm's loop count, one a
    call plus one an iteration -- reached the gate.  Counted on the CPU model alone over
    the 20 batches, that work is 13..98 a batch at n = 128 and 8..75 at 129 (three batches
    with a next one reach 67 at each: the default gate gives both passes), but at most 33 at 256, 44 at 257,
    63 at 300, 58 at 384, 32 at 385 and 13 at 511 and 512 (wider rows start nearer
    orthogonal: the draws are of sigma 1 / n), where the default would never take the
    relation pass.  There the gate is 8, as in test_transh_parallel_orth_gate: 5 (n = 512)
    to 17 (n = 256) of the 19 batches that have a previous one reach it."""
    return None if dim <= 129 else 8


def _transh_parallel(dim, monkeypatch, env=(), tag=""):
    gate = _orth_gate(dim)
    if gate is not None:
        monkeypatch.setenv("KB2E_HPAR_ORTH_MIN", str(gate))
    for name, value in env:
        monkeypatch.setenv(name, value)
    out = _run("parallel", "H", dim, seed=SEED_H_PAR, atol=H_PAR_ATOL, keep=True, orth_min=gate, tag=tag)
    try:
        ran = out["eng"].counter("transh_orth_rel_batches")
    finally:
        out["eng"].close()
    print(f"wide-rows par-H{dim}{tag}: relation pass in {ran} of {EPOCHS * 10} batches (gate {gate or 'default'})")
    # some batches took the relation pass and some did not: both normOrth passes ran
    assert 0 < ran < EPOCHS * 10, (ran, EPOCHS * 10)


@pytest.mark.parametrize("dim", PAR_WIDTHS)
def test_transh_parallel_chunk_edges(dim, monkeypatch):
    """transh_phase_b_kernel, transh_orth_rel_kernel and the one-wave orth pass
    <double, CH>; the relation pass must have run in some batches and not in others
    (_orth_gate), so both normOrth passes ran."""
    _transh_parallel(dim, monkeypatch)


# ------------------------------------------------ 2. the long-segment kernels at CH = 2, 4

@pytest.mark.parametrize("env", [(("KB2E_FOLD_LONG", "64"),), (("KB2E_FOLD_LONG", "0"),), (("KB2E_GRAM_MIN", "0"),)],
                         ids=["fold_long64", "gram", "plain"])
@pytest.mark.parametrize("dim", [200, 300, 512])
def test_transe_ordered_long_segments(dim, env, monkeypatch):
    """B = 600 (batches = 5): the hottest relation has 195 samples a batch.
    KB2E_FOLD_LONG=64 sends its segments (and every other of >= 64 events) through
    transe_fold_long_kernel<double, 2 | 4>; KB2E_FOLD_LONG=0 leaves everything of
    >= KB2E_GRAM_MIN (48) events to the Gram scalar recurrence of transe_fold_kernel;
    KB2E_GRAM_MIN=0 uses neither.  One oracle run for the three."""
    for name, value in env:
        monkeypatch.setenv(name, value)
    fold_long = env[0] == ("KB2E_FOLD_LONG", "64")
    out = _run("ordered", "E", dim, batches=5, seed=SEED_E, atol=F64_ATOL, keep=True, tag=f" {env[0][0]}={env[0][1]}",
               before=(lambda eng: eng.profile(1)) if fold_long else None)
    try:
        if fold_long:
            _, launches = out["eng"].profile_query("fold_long")
            assert launches > 0, "transe_fold_long_kernel never ran"
    finally:
        out["eng"].close()


@pytest.mark.parametrize("apply_long", [0, 1, 64])
@pytest.mark.parametrize("dim,distance", [(300, 0), (512, 1)])
def test_transe_parallel_long_segments(dim, distance, apply_long, monkeypatch):
    """KB2E_APPLY_LONG: no segment through transe_apply_kernel<double, 4, *>'s 16-wave
    branch (0), every one (1), those of >= 64 events (the hot relations and entities
    of a B = 300 batch)."""
    monkeypatch.setenv("KB2E_APPLY_LONG", str(apply_long))
    _run("parallel", "E", dim, distance=distance, seed=SEED_E, atol=P_ATOL, tag=f" KB2E_APPLY_LONG={apply_long}")


@pytest.mark.parametrize("env", [(("KB2E_APPLY_LONG", "0"),), (("KB2E_APPLY_LONG", "1"),),
                                 (("KB2E_HPAR_FUSE", "0"), ("KB2E_WAPPLY_WAVES", "16")),
                                 (("KB2E_HPAR_FUSE", "0"), ("KB2E_WAPPLY_WAVES", "4")),
                                 (("KB2E_HPAR_ORTH_Q", "0"),)],
                         ids=["apply_long0", "apply_long1", "unfused16", "unfused4", "orth_requeue"])
def test_transh_parallel_variants_four_chunks(env, monkeypatch):
    """n = 300 on the four-chunk build: the row sums' 16-wave branch off and on, phase B
    as two launches with the normals' workgroups of 16 and 4 waves, and the one-wave
    orth pass listing its second sweep's flags again.  One CPU model run for all (and
    for test_transh_parallel_chunk_edges[300])."""
    _transh_parallel(300, monkeypatch, env, tag=" " + " ".join(f"{k}={v}" for k, v in env))
