"""The device sampler's stream against the host glibc stream, sample by sample.

Every case runs one driver: the oracle's `sample_stream` (oracle/orc.c, pinned
to the compiled reference by test_oracle_golden.py) and the engine's stream of
the epoch in progress (`kb2e_get_sample_stream`) from the same seed, compared
with `np.array_equal` on (si, sj, side) every epoch, and five `rand()` values
after the last epoch.  The tables are uploaded (`upload_params` draws no random
word) and TransE runs at dim 4..8, so only the sampler is under test.  The
comparison is on integers: there are no tolerances.

What each case reaches (kernels_sampler.hpp, kernels_glibc.hpp, engine.hip):

* geometry: S = 1 (K = max(1, bits_for(0))), B = 1, two superchunks with
  ntrain % batches != 0, and 900,000 samples on a sparse set: >= 4.5M words, 69+
  superchunks, so chain_top_kernel carries s_cur / s_base into its second tile,
  and the words' blocks reach level 10 of the power table (block 1,024+).  Its
  second epoch draws from the tight 1.03 x used buffer.  No counter names the
  chain's form, so that case bounds the live device bytes the run added
  instead: the sampler's buffers cost 17 bytes a word position with one level
  of next[] (about 95 MB at 6 words a sample), pointer doubling holds
  bits_for(S - 1) = 20 levels of >= 4.5M words (>= 360 MB more).
* forms: pointer doubling (also S = 4,096 and 4,097: 12 and 13 levels), the
  overflow of the chunked chain (KB2E_SAMPLER_EMAX: 7, which this sparse set's
  5-word samples never exceed, and 1, which every sample across a chunk edge
  does; the second epoch then runs on the sticky doubling), the 16-byte triple
  table, sample_len's grid-stride loop (1 and 3 workgroups), the host sampler.
* rejection-heavy: every (h, r) and (r, t) keeps one free entity of 40: about
  109 words a sample, so the 64-word entry table overflows naturally, samples
  span whole chunks, and the word buffer grows by x1.5 about eight times.
* packing: 2 eb + rb + 10 = 64 (8-byte table) and 65 (16-byte), eb = 20 and
  21, entity ne - 1 as head and tail, and relation nr - 1 with a threshold
  >= 512, which sets bit 63 of the packed word.
* thresholds: pr = 750.0, 250.0, 500.0 exactly and 666.67 in one set; the
  drawn residues rand() % 1000 include thr - 1 and thr for every relation.
* across epochs: the window after `consumed` words, the two stream sets (the
  stream read again after the epoch's last batch, while the next one is
  prefetched into the other set), rng_next between epochs (the prefetched
  stream is redrawn), and another triple set after an epoch.

Measured on an MI355X, each test whole (data set, host stream, engine), 24
cases in 2.7 s:
  test_second_tile_of_the_top_walk   0.74 s  (host: 0.13 s data set, about 0.3 s
                                             a 900,000-sample stream; the run
                                             added 94,070,168 device bytes)
  test_one_sample                    0.32 s  (the process's first: HIP start-up)
  test_threshold_edges               0.22 s  (the replay loop in Python)
  test_packing_edges                 0.10 - 0.12 s each
  test_one_free_entity               0.06 s each
  test_state_across_epochs           0.03 - 0.05 s each
  test_sampler_forms, test_doubling_level_count, test_two_superchunks,
  test_batches_of_one                0.02 - 0.03 s each
"""
import numpy as np
import pytest

from kb2e_amd import data
from kb2e_amd.engine import Engine
from oracle import orc

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- data sets
def _random_set(ne, nr, count, seed, extra=None):
    """`count` distinct random triples (numpy only), `extra` rows first."""
    rng = np.random.default_rng(seed)
    space = ne * ne * nr
    keys = np.unique(rng.integers(0, space, size=int(count * 1.2) + 16, dtype=np.int64))
    rng.shuffle(keys)
    h, rest = keys // (ne * nr), keys % (ne * nr)
    tr = np.stack([h, rest // nr, rest % nr], 1).astype(np.int32)
    if extra is not None:
        extra = np.asarray(extra, dtype=np.int32)
        own = (tr[:, None, :] == extra[None, :, :]).all(2).any(1)
        tr = np.concatenate([extra, tr[~own]])
    assert len(tr) >= count
    tr = tr[:count]
    return data.Dataset(ne, nr, tr, tr[:0], tr[:0])


def _sparse_14003():
    return _random_set(2000, 10, 14003, seed=11)


def _tables(ne, nr, dim, w=False):
    rng = np.random.default_rng(5)
    ent = rng.uniform(-1, 1, (ne, dim))
    ent /= np.linalg.norm(ent, axis=1, keepdims=True)
    rel = rng.uniform(-1, 1, (nr, dim))
    rel /= np.linalg.norm(rel, axis=1, keepdims=True)
    wm = np.ascontiguousarray(np.broadcast_to(np.eye(dim), (nr, dim, dim))) if w else None
    return ent, rel, wm


def _pr(train, nr):
    """1000 tailMean / (tailMean + headMean) per relation (common/trainer.cpp:163-194): the
    means are triples per distinct tail / head of the relation.  NaN without triples."""
    out = np.full(nr, np.nan)
    for r in np.unique(train[:, 2]):
        sel = train[train[:, 2] == r]
        hmean = len(sel) / len(np.unique(sel[:, 0]))
        tmean = len(sel) / len(np.unique(sel[:, 1]))
        out[r] = 1000 * tmean / (tmean + hmean)
    return out


# ---------------------------------------------------------------- the driver
class _Pair:
    """The oracle and the engine on one data set, from one seed."""

    def __init__(self, ds, *, method, batches, seed, model="E", dim=4, schedule="ordered"):
        self.ds, self.method, self.batches, self.dim = ds, method, batches, dim
        self.eng = Engine(model, dim, ds.num_entities, ds.num_relations, rate=0.001, method=method, distance=0,
                          batches=batches, seed=seed, schedule=schedule)
        try:
            self.eng.upload_triples(ds.train)
            self.eng.upload_params(*_tables(ds.num_entities, ds.num_relations, dim, w=model == "R"))
            self.set_oracle(ds.train)
            orc.srand(seed)
        except BaseException:
            self.eng.close()
            raise

    def set_oracle(self, train):
        # (a fresh model: the oracle's rand() state is the process's, not the model's)
        self.m = orc.Model("E", self.dim, self.ds.num_entities, self.ds.num_relations, method=self.method,
                           batches=self.batches)
        self.m.set_triples(train)
        self.S = (len(train) // self.batches) * self.batches
        assert self.m.batch_size() * self.batches == self.S

    def upload_triples(self, train):
        self.eng.upload_triples(train)
        self.set_oracle(train)

    def epoch(self, tag, finish=True):
        """One epoch: the stream after the first batch against the oracle's."""
        ref = self.m.sample_stream(self.S)
        self.eng.train_batches(1)
        self.eng.synchronize()
        _same(self.eng.sample_stream(self.S), ref, tag)
        if finish and self.batches > 1:
            self.eng.train_batches(self.batches - 1)
        return ref

    def rng_next(self):
        a, b = self.eng.rng_next(), orc.rand()
        assert a == b, (a, b)

    def finish(self):
        got = [self.eng.rng_next() for _ in range(5)]
        assert got == [orc.rand() for _ in range(5)]

    def close(self):
        self.eng.close()


def _same(got, ref, tag):
    for name, g, r in zip(("si", "sj", "side"), got, ref):
        if not np.array_equal(g, r):
            bad = np.flatnonzero(g != r)
            raise AssertionError(f"{tag}: {name} differs at {bad.size} of {r.size} samples, first at {bad[0]}: "
                                 f"{g[bad[0]]} for {r[bad[0]]}")


def _run(ds, *, method=1, batches, seed, epochs, **kw):
    p = _Pair(ds, method=method, batches=batches, seed=seed, **kw)
    try:
        for ep in range(epochs):
            p.epoch(f"epoch {ep}")
        p.finish()
    finally:
        p.close()


# ---------------------------------------------------------------- geometry
def test_one_sample():
    """ntrain = 1, one batch: S = 1."""
    tr = np.array([[0, 1, 0]], dtype=np.int32)
    _run(data.Dataset(3, 1, tr, tr[:0], tr[:0]), batches=1, seed=3, epochs=3)


def test_batches_of_one():
    """ntrain = batches = 7: B = 1."""
    _run(_random_set(5, 2, 7, seed=2), batches=7, seed=4, epochs=3)


def test_two_superchunks():
    """S = 14,000 of 14,003 triples: >= 70,000 words, two superchunks."""
    _run(_sparse_14003(), batches=10, seed=5, epochs=2)


def test_second_tile_of_the_top_walk():
    """900,000 samples: the chain's top walk enters its second tile of 64
    superchunks, the words' blocks pass 1,024 (power level 10); two epochs, the
    second from the tight buffer.  The bound on the device bytes the run added
    (module docstring) holds only for the chunked form."""
    ds = _random_set(20000, 50, 900000, seed=13)
    p = _Pair(ds, method=1, batches=100, seed=7, schedule="parallel")
    try:
        before = p.eng.device_bytes()
        for ep in range(2):
            p.epoch(f"epoch {ep}")
        added = p.eng.device_bytes() - before
        print(f"device bytes added by the run: {added}")
        assert added < 200e6, added
        p.finish()
    finally:
        p.close()


# ---------------------------------------------------------------- forms
@pytest.mark.parametrize("env", [None, ("KB2E_SAMPLER_DOUBLING", "1"), ("KB2E_SAMPLER_EMAX", "7"),
                                 ("KB2E_SAMPLER_EMAX", "1"), ("KB2E_SAMPLER_TRIP16", "1"), ("KB2E_SAMPLE_GRID", "1"),
                                 ("KB2E_SAMPLE_GRID", "3"), ("KB2E_HOST_SAMPLER", "1")],
                         ids=lambda e: "default" if e is None else "=".join(e))
def test_sampler_forms(monkeypatch, env):
    if env is not None:
        monkeypatch.setenv(*env)
    _run(_sparse_14003(), batches=10, seed=6, epochs=2)


@pytest.mark.parametrize("ntrain,batches", [(4096, 16), (4097, 17)])
def test_doubling_level_count(monkeypatch, ntrain, batches):
    """S = 4,096 and 4,097: bits_for(S - 1) = 12 and 13 levels of next[]."""
    monkeypatch.setenv("KB2E_SAMPLER_DOUBLING", "1")
    ds = _random_set(2000, 10, ntrain, seed=12)
    assert (ntrain // batches) * batches == ntrain
    _run(ds, batches=batches, seed=8, epochs=2)


# ---------------------------------------------------------------- rejection-heavy
def _one_free_entity_set(ne=40, nr=2):
    h, t, r = np.meshgrid(np.arange(ne), np.arange(ne), np.arange(nr), indexing="ij")
    keep = (t - h - r) % ne >= 1
    tr = np.stack([h[keep], t[keep], r[keep]], 1).astype(np.int32)
    np.random.default_rng(3).shuffle(tr)
    return data.Dataset(ne, nr, tr, tr[:0], tr[:0])


@pytest.mark.parametrize("method", [0, 1])
def test_one_free_entity(method):
    """3,120 of 3,200 keys are training triples: every corrupted side has one
    free entity of 40 (about 109 words a sample on the host)."""
    ds = _one_free_entity_set()
    assert len(ds.train) == 3120
    _run(ds, method=method, batches=8, seed=7, epochs=2)


# ---------------------------------------------------------------- packing edges
@pytest.mark.parametrize("ne,nr,bits", [(2 ** 20, 2 ** 14, 64), (2 ** 20, 2 ** 14 + 1, 65),
                                        (2 ** 20 + 1, 2 ** 12, 64), (2 ** 20 + 1, 2 ** 12 + 1, 65)])
def test_packing_edges(ne, nr, bits):
    """3,000 triples whose ids need exactly 64 and 65 bits with the threshold."""
    eb, rb = int(ne - 1).bit_length(), int(nr - 1).bit_length()
    assert 2 * eb + rb + 10 == bits
    last = nr - 1
    extra = [[100 + k, ne - 1, last] for k in range(40)] + [[ne - 1, 5, last], [ne - 1, ne - 1, 0]]
    ds = _random_set(ne, nr, 3000, seed=21, extra=extra)
    tr = ds.train
    assert (tr[:, 0] == ne - 1).any() and (tr[:, 1] == ne - 1).any()
    pr = _pr(tr, nr)[last]  # 40 heads on one tail: the tail side is corrupted almost always
    assert 512 <= pr < 1000, pr
    _run(ds, method=1, batches=10, seed=9, epochs=2)


# ---------------------------------------------------------------- threshold edges
def _ratio_set():
    """Four relations, 20,001+ triples each: 3 triples a tail and 1 a head
    (pr = 750), 1 and 3 (250), 1 and 1 (500), 2 and 1 (666.67)."""
    g3, g2 = np.arange(6667), np.arange(10001)
    rows = []
    for i in range(3):
        rows.append(np.stack([3 * g3 + i, g3 + 20100, 0 * g3], 1))      # relation 0: three heads a tail
        rows.append(np.stack([g3 + 20100, 3 * g3 + i, 0 * g3 + 1], 1))  # relation 1: three tails a head
    g1 = np.arange(20001)
    rows.append(np.stack([g1, (g1 + 17) % 20001, 0 * g1 + 2], 1))       # relation 2: one to one
    for i in range(2):
        rows.append(np.stack([2 * g2 + i, g2 + 20100, 0 * g2 + 3], 1))  # relation 3: two heads a tail
    tr = np.concatenate(rows).astype(np.int32)
    np.random.default_rng(4).shuffle(tr)
    return data.Dataset(32000, 4, tr, tr[:0], tr[:0])


def test_threshold_edges():
    """pr exactly 750, 250, 500 beside 666.67: thr = 750, 250, 500, 667.  The
    first epoch's words are replayed with orc.rand() to show that the residues
    thr - 1 and thr were drawn for every relation (a condition on this test's
    inputs); the engine must then take the reference's side at each of them."""
    ds = _ratio_set()
    tr, ne, batches, seed = ds.train, ds.num_entities, 10, 10
    pr = _pr(tr, 4)
    assert pr[0] == 750.0 and pr[1] == 250.0 and pr[2] == 500.0 and abs(pr[3] - 2000 / 3) < 1e-9
    thr = np.ceil(pr).astype(int)
    assert thr.tolist() == [750, 250, 500, 667]
    assert np.bincount(tr[:, 2]).min() >= 20000
    m = orc.Model("E", 4, ne, 4, method=1, batches=batches)
    m.set_triples(tr)
    S = (len(tr) // batches) * batches
    orc.srand(seed)
    si, sj, side = m.sample_stream(S)
    orc.srand(seed)
    seen = np.zeros((4, 1000), np.int64)
    for s in range(S):
        assert orc.randmax(len(tr)) == si[s]
        j = orc.randmax(ne)
        r = tr[si[s], 2]
        res = orc.rand() % 1000
        seen[r, res] += 1
        assert side[s] == (res < thr[r])
        while j != sj[s]:  # a rejected j completes a training triple, so it is never the accepted one
            j = orc.randmax(ne)
    for r in range(4):
        assert seen[r, thr[r] - 1] > 0 and seen[r, thr[r]] > 0, (r, seen[r, thr[r] - 1], seen[r, thr[r]])
    _run(ds, method=1, batches=batches, seed=seed, epochs=1)


# ---------------------------------------------------------------- across epochs
@pytest.mark.parametrize("model,schedule", [("E", "ordered"), ("E", "parallel"), ("R", "parallel")])
def test_state_across_epochs(model, schedule):
    """Four epochs at S = 14,000.  Epoch 2's stream is read again after its last
    batch: the next epoch's prefetch, queued after the first batch, wrote the
    other set.  One rand() on both sides before epoch 3: the prefetched stream
    no longer follows the generator and is redrawn.  A smaller triple set (5,000,
    other triples) after epoch 3: a stale prefetch would index the old set.
    TransR PARALLEL builds its shadow event index right after each prefetch."""
    ds = _sparse_14003()
    p = _Pair(ds, method=1, batches=10, seed=14, model=model, dim=8, schedule=schedule)
    try:
        p.epoch("epoch 1")
        ref = p.epoch("epoch 2")
        p.eng.synchronize()
        _same(p.eng.sample_stream(p.S), ref, "epoch 2 after its last batch")
        p.rng_next()
        p.epoch("epoch 3")
        small = _random_set(ds.num_entities, ds.num_relations, 5000, seed=15)
        p.upload_triples(small.train)
        assert p.S == 5000
        ref = p.epoch("epoch 4")
        assert ref[0].max() < 5000
        p.finish()
    finally:
        p.close()
