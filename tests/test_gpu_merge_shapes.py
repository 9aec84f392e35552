"""The epoch merge (kb2e_amd/csrc/engine_merge.inc) over its widths, both
precisions and its rank counts, against tests/merge_model.py: numpy float64
renorm(T0 + sum_r (T_r - T0)) from the tables as the engine holds them.

Driver: `world` contexts on device 0 (no triples, the default ORDERED
schedule), the base on rank 0 and garbage on the others, kb2e_comm_init_group
(every rank then equals rank 0 bit for bit), every rank's constructed table
through kb2e_upload_params, kb2e_merge_epoch_group, every rank downloaded.
After the merge all ranks are bit-identical, the units whose summed delta is
zero (the long base rows nobody touched, the rows whose deltas cancel across two
ranks, the TransR matrix without a delta) carry the base's bits, everything else
is within the bar of the reference, and the padding element of every row of an
odd width is zero.  A second round of deltas over the merged tables follows (the
base must have moved).  The same for one context on a one-rank RCCL
communicator (the ncclFloat path, an odd width, the three-chunk build).

Bars: FP64 1e-12 (the bar of tests/test_gpu_merge.py; values are below 4),
FP32 1e-5 (the bar of tests/test_gpu_fp32_step.py: a merged element takes at
most 16 float adds, a wave sum of n <= 512 squares, a square root and a divide).

Continuation: a group of two trains an epoch on the tiny set and merges; beside
every rank a solo context (same seed and shard, the group's start tables) trains
the same epoch and then receives the merged tables through kb2e_upload_params.
Both then train a second epoch, which must agree (active counts equal, loss
1e-12 relative, tables and the TransR work vectors 1e-12): a stale
table-derived copy after the merge would move rows at the rate scale, 1e-3.

Observed on an MI355X (largest |engine - reference| per family, both rounds):
widths FP64 1.9e-16, widths FP32 5.2e-8, rank counts (FP64) 2.2e-16, the 270,000-row
case 3.3e-16, one-rank RCCL 1.1e-16 (FP64) and 3.6e-8 (FP32); every continuation
path 0 (the group rank and its solo context end bit-identical).  The renormalize
calls (tests/test_gpu_renormalize.py): 1.9e-16 in FP64, 9.2e-8 in FP32.  That is
four (FP64) and two (FP32) orders below the bars, as the rounding argument says.
"""
import numpy as np
import pytest
import torch  # noqa: F401  (first: torch's own RCCL in the process, as tests/test_gpu_merge.py)

import merge_model as mm
from gpu_common import tiny
from kb2e_amd.distributed import engine_tables, shard_heads
from kb2e_amd.engine import Engine, EngineError, comm_init_group, merge_epoch_group

BAR = {64: 1e-12, 32: 1e-5}


def _engine(c, seed=0, n=None):
    return Engine(c.model, c.n if n is None else n, c.ne, c.nr, seed=seed, precision=c.precision)


def _upload(eng, tabs):
    eng.upload_params(tabs[0], tabs[1], tabs[2])


def _garbage(c, k, seed):
    rng = np.random.default_rng([seed, 99])
    return [None if t is None else rng.uniform(-3, 3, t.shape) for t in k.base]


def _padding_is_zero(eng, c):
    ld = (c.n + 1) & ~1
    for t in engine_tables(eng):
        rows = t.view(-1, ld).cpu().numpy()
        if ld > c.n and not np.array_equal(rows[:, c.n:], np.zeros_like(rows[:, c.n:])):
            return False
    return True


def _check_round(c, engs, base, ranks, merge):
    """Upload, merge, download; the assertions of one round.  Returns the merged
    tables and the largest difference from the reference."""
    for eng, tabs in zip(engs, ranks):
        _upload(eng, tabs)
    merge()
    exp = mm.expected_merge(c.model, base, ranks, c.precision)
    changed = mm.changed_units(base, ranks, c.precision)
    got = [eng.download_params() for eng in engs]
    worst = 0.0
    for r, eng in enumerate(engs):
        for t in range(3):
            if base[t] is None:
                continue
            assert np.array_equal(got[r][t], got[0][t]), ("ranks differ", r, t)
            assert np.array_equal(got[r][t][~changed[t]], base[t][~changed[t]]), ("unchanged unit moved", r, t)
            worst = max(worst, float(np.abs(got[r][t] - exp[t]).max()))
        assert _padding_is_zero(eng, c), ("padding", r)
    return got[0], worst


def _run_group(c):
    k = mm.build(c)
    assert k.min_len_margin >= 0.3 and k.min_delta >= 2.0 ** -6
    engs = [_engine(c, seed=r) for r in range(c.world)]
    try:
        for r, eng in enumerate(engs):
            _upload(eng, k.base if r == 0 else _garbage(c, k, r))
        comm_init_group(engs)
        for r, eng in enumerate(engs):
            for g, b in zip(eng.download_params(), k.base):
                assert (g is None and b is None) or np.array_equal(g, b), ("broadcast", r)
            assert eng.comm_info() == (c.world, r) + k.owners[r]
        merged, w1 = _check_round(c, engs, k.base, k.ranks, lambda: merge_epoch_group(engs))
        base2, ranks2 = mm.second_round(k, merged)
        margin, dmin = mm.guards(c.model, base2, ranks2, c.precision)
        assert margin >= 0.3 and dmin >= 2.0 ** -6
        assert not np.array_equal(base2[0], k.base[0])
        _, w2 = _check_round(c, engs, base2, ranks2, lambda: merge_epoch_group(engs))
    finally:
        for eng in engs:
            eng.close()
    print(f"{c.id}: max |engine - reference| round 1 {w1:.3e}, round 2 {w2:.3e} (bar {BAR[c.precision]:.0e})")
    assert max(w1, w2) <= BAR[c.precision], (w1, w2)


@pytest.mark.gpu
@pytest.mark.parametrize("c", mm.WIDTH_CASES, ids=lambda c: c.id)
def test_merge_widths(c):
    """World 3 at |E| = 37 (blocks 13, 13, 11): one, two and four chunks a lane,
    odd and even widths, both precisions."""
    _run_group(c)


@pytest.mark.gpu
@pytest.mark.parametrize("c", mm.RANK_CASES, ids=lambda c: c.id)
def test_merge_rank_counts(c):
    """1..5 and 16 owners of 37 rows (at 16 the block is 3, rank 12 owns one row,
    ranks 13..15 none), 4 owners of 3 rows, 2 owners of 1 row."""
    _run_group(c)


@pytest.mark.gpu
@pytest.mark.parametrize("c", mm.STRIDE_CASES, ids=lambda c: c.id)
def test_merge_grid_stride(c):
    """More rows than renorm_kernel's 65,535 x 4 waves and more elements than
    merge_grid's 8,192 x 256 threads: the grid-stride loops take a second turn."""
    assert c.ne > 65535 * 4 and c.ne * ((c.n + 1) & ~1) > 8192 * 256
    _run_group(c)


@pytest.mark.gpu
@pytest.mark.parametrize("c", mm.RCCL_CASES, ids=lambda c: c.id)
def test_merge_one_rank_rccl(c):
    k = mm.build(c)
    eng = _engine(c)
    try:
        _upload(eng, k.base)
        eng.comm_init_rank(1, 0, Engine.comm_unique_id())
        assert eng.comm_info() == (1, 0, 0, c.ne)
        merged, w1 = _check_round(c, [eng], k.base, k.ranks, eng.merge_epoch)
        base2, ranks2 = mm.second_round(k, merged)
        _, w2 = _check_round(c, [eng], base2, ranks2, eng.merge_epoch)
    finally:
        eng.close()
    print(f"{c.id}: max |engine - reference| round 1 {w1:.3e}, round 2 {w2:.3e} (bar {BAR[c.precision]:.0e})")
    assert max(w1, w2) <= BAR[c.precision], (w1, w2)


# ---- the contract around the group calls (host checks only)

def _same(a, b):
    return all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.gpu
def test_group_contract():
    c = mm.RANK_CASES[1]  # TransE, n = 20, 37 entities
    k = mm.build(c)
    engs = [_engine(c, seed=r) for r in range(17)]
    odd = _engine(c, n=c.n + 2)
    try:
        for r, eng in enumerate(engs):
            _upload(eng, k.base if r == 0 else k.ranks[r % 2])
        _upload(odd, [np.zeros((c.ne, c.n + 2)), np.zeros((c.nr, c.n + 2)), None])
        everyone = engs + [odd]

        def refused(status, call):
            before = [(e.download_params(), e.device_bytes()) for e in everyone]
            with pytest.raises(EngineError, match=status):
                call()
            for e, (tabs, nbytes) in zip(everyone, before):
                assert _same(e.download_params(), tabs) and e.device_bytes() == nbytes

        refused("EUNSUPPORTED", lambda: comm_init_group(engs))  # 17: past the local backend's 16
        refused("EINVAL", lambda: comm_init_group([engs[0], odd]))  # the dims differ
        pair = engs[:2]
        refused("ESTATE", lambda: merge_epoch_group(pair))  # no communicator yet
        comm_init_group(pair)  # the retry the header promises
        assert _same(pair[1].download_params(), k.base)
        refused("ESTATE", lambda: comm_init_group(pair))
        refused("ESTATE", lambda: comm_init_group([engs[2], engs[0]]))
        refused("ESTATE", lambda: merge_epoch_group(pair[:1]))
        refused("ESTATE", lambda: merge_epoch_group(pair[::-1]))
        refused("ESTATE", lambda: merge_epoch_group(pair + [engs[2]]))
        refused("ESTATE", pair[0].merge_epoch)  # a local group merges as a group
        merge_epoch_group(pair)  # and the group still works
    finally:
        for e in engs + [odd]:
            e.close()


# ---- training continues from the merged tables

CONTINUATION = [("R", "ordered", 20, 64), ("R", "parallel", 50, 64), ("R", "parallel", 160, 64),
                ("H", "parallel", 20, 64), ("E", "parallel", 130, 64), ("R", "ordered", 20, 32)]


def _trainer(ds, model, schedule, dim, precision, rank):
    eng = Engine(model, dim, ds.num_entities, ds.num_relations, rate=0.01, batches=10, seed=7 + rank,
                 schedule=schedule, precision=precision)
    eng.upload_triples(shard_heads(ds.train, rank, 2))
    e0, r0, _ = eng.init_params()
    if model == "R":
        eng.transr_seed(e0, r0)
    return eng


def _worst(a, b):
    return max(float(np.abs(x - y).max()) for x, y in zip(a, b) if x is not None)


@pytest.mark.gpu
@pytest.mark.parametrize("model,schedule,dim,precision", CONTINUATION,
                         ids=[f"{m}-{s}-n{d}-fp{p}" for m, s, d, p in CONTINUATION])
def test_training_continues_from_the_merged_tables(model, schedule, dim, precision):
    ds = tiny()
    group = [_trainer(ds, model, schedule, dim, precision, r) for r in range(2)]
    solo = [_trainer(ds, model, schedule, dim, precision, r) for r in range(2)]
    try:
        comm_init_group(group)
        start = group[0].download_params()
        for r in range(2):
            _upload(solo[r], start)
            first = group[r].train_epoch()
            assert solo[r].train_epoch()[1] == first[1]
        trained = [e.download_params() for e in group]
        assert not np.array_equal(trained[0][0], trained[1][0])  # the shards differ
        merge_epoch_group(group)
        merged = group[0].download_params()
        assert not np.array_equal(merged[0], trained[0][0]) and _same(group[1].download_params(), merged)
        worst = 0.0
        for r in range(2):
            _upload(solo[r], merged)
            lg, ag = group[r].train_epoch()
            ls, as_ = solo[r].train_epoch()
            assert ag == as_ and ag > 0, (r, ag, as_)
            assert abs(lg - ls) <= 1e-12 * max(1.0, abs(ls)), (r, lg, ls)
            err = _worst(group[r].download_params(), solo[r].download_params())
            if model == "R":
                err = max(err, _worst(group[r].transr_work(), solo[r].transr_work()))
            worst = max(worst, err)
    finally:
        for e in group + solo:
            e.close()
    print(f"continuation {model} {schedule} n={dim} fp{precision}: max |group rank - solo| {worst:.3e}")
    assert worst <= 1e-12
