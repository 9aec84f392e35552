"""The merge reference and its cases (tests/merge_model.py), on the CPU:

* every committed case keeps its guards (a shrink decision is >= 0.3 away from
  length 1, every non-zero delta element is >= 2^-6, in the case's own
  precision), in the first and in the second round, holds the row categories it
  is there for, and has its idle owners where the block arithmetic puts them;
* expected_merge agrees with the second implementation of the merge,
  kb2e_amd.distributed.TableMerger, over gloo on CPU tensors at world 2 and 3 --
  the cancellation rows included, which ties the summed-delta rule to it.
"""
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import merge_model as mm
from kb2e_amd.distributed import TableMerger

ROW_CATEGORIES = {"owner_first", "owner_last", "row0", "row_last", "one_rank", "elem0_only", "elem_last_only",
                  "long_unchanged"}


def _wanted(c):
    """The categories a case of this shape must hold."""
    want = set(ROW_CATEGORIES)
    if c.ne < 3 and c.nr < 3:  # one row a table: nothing can stay unchanged
        want.discard("long_unchanged")
    if c.model != "R":
        want |= {"shrink_long", "shrink_short"}
    else:  # relation u is of kind u % 5
        want |= {m for m, need in (("w_single_row", 2), ("w_unchanged", 3), ("w_last_element", 5)) if c.nr >= need}
    if c.world >= 2:
        want.add("all_ranks")
        if c.nr >= 4:
            want.add("cancel_rel")
        # an entity row no owner's block begins or ends with
        if c.ne - len({r for lo, n in mm.owner_blocks(c.ne, c.world) if n for r in (lo, lo + n - 1)}) >= 2:
            want.add("cancel_ent")
    return want


@pytest.mark.parametrize("c", mm.ALL_CASES, ids=lambda c: c.id)
def test_case_guards_and_categories(c):
    k = mm.build(c)
    print(f"{c.id}: min |len - 1| {k.min_len_margin:.3f}, min |delta| {k.min_delta:.5f}, "
          f"categories {sorted(k.categories)}, idle owners {k.idle}")
    assert k.min_len_margin >= 0.3 and k.min_delta >= 2.0 ** -6
    assert _wanted(c) <= set(k.categories), _wanted(c) - set(k.categories)
    for tabs in [k.base] + k.ranks:
        assert max(np.abs(t).max() for t in tabs if t is not None) < 4
    # the categories are what they say, measured from the tables
    changed = mm.changed_units(k.base, k.ranks, k.precision)
    flat = [None if t is None else t.reshape(t.shape[0], -1) for t in k.base]
    delta = [[None if t is None else (t - b).reshape(t.shape[0], -1) for t, b in zip(tr, k.base)] for tr in k.ranks]
    for name, where in k.categories.items():
        for t, u in where:
            touched = [r for r in range(k.world) if (delta[r][t][u] != 0).any()]
            if name.startswith("cancel"):
                assert not changed[t][u] and len(touched) == 2
                assert mm.seq_len(flat[t][u:u + 1])[0] > 1.3
                assert np.array_equal(flat[t][u] * 1024, np.round(flat[t][u] * 1024))
            elif name in ("long_unchanged", "w_unchanged"):
                assert not changed[t][u] and not touched
                ln = mm.seq_len(k.base[t][u].reshape(-1, k.n))
                assert (np.abs(ln - 1) >= 0.09).all() if name == "w_unchanged" else 1.3 <= ln[0] <= 1.7
            else:
                assert changed[t][u]
            if name == "one_rank":
                assert len(touched) == 1
            if name == "all_ranks":
                assert len(touched) == k.world
            if name == "elem0_only":
                assert all(np.nonzero(delta[r][t][u])[0].tolist() == [0] for r in touched)
            if name == "elem_last_only":
                assert all(np.nonzero(delta[r][t][u])[0].tolist() == [k.n - 1] for r in touched)
            if name == "w_single_row":
                rows = {int(i) // k.n for r in touched for i in np.nonzero(delta[r][t][u])[0]}
                assert len(rows) == 1
            if name == "w_last_element":
                assert all(np.nonzero(delta[r][t][u])[0].tolist() == [k.n * k.n - 1] for r in touched)
    # block ownership: the idle owners, the short last block
    block = -(-c.ne // c.world)
    assert k.owners == [(min(c.ne, r * block), max(0, min(c.ne, (r + 1) * block) - min(c.ne, r * block)))
                        for r in range(c.world)]
    assert sum(n for _, n in k.owners) == c.ne
    assert k.idle == [r for r in range(c.world) if r * block >= c.ne]
    if (c.ne, c.world) == (37, 16):
        assert block == 3 and k.idle == [13, 14, 15] and k.owners[12] == (36, 1)
    if (c.ne, c.world) == (3, 4):
        assert k.idle == [3]
    if (c.ne, c.world) == (1, 2):
        assert k.idle == [1]
    # the second round keeps the guards over the moved base, and moves other rows
    merged = mm.expected_merge(k.model, k.base, k.ranks, k.precision)
    base2, ranks2 = mm.second_round(k, merged)
    margin, dmin = mm.guards(k.model, base2, ranks2, k.precision)
    assert margin >= 0.3 and dmin >= 2.0 ** -6
    ch2 = mm.changed_units(base2, ranks2, k.precision)
    assert ch2[0].any() and ch2[1].any()
    for t, u in k.categories.get("long_unchanged", []):
        assert not ch2[t][u]


def test_reference_restates_the_constraints():
    """expected_renorm against a scalar loop (common::norm's sequential sum), and
    the summed-delta rule against the per-rank rule on a cancellation row."""
    rng = np.random.default_rng(3)
    rows = rng.uniform(-1, 1, (6, 5))
    mask = np.array([1, 0, 1, 1, 0, 1])
    for model, table, unit in (("E", 0, False), ("H", 1, False), ("H", 2, True), ("R", 0, True)):
        exp = rows.copy()
        for i in range(6):
            s = 0.0
            for x in rows[i]:
                s += x * x
            if mask[i] and (unit or np.sqrt(s) > 1):
                exp[i] = rows[i] / np.sqrt(s)
        assert np.array_equal(mm.expected_renorm(model, table, rows, mask), exp)
    w = rng.uniform(-1, 1, (3, 4, 4))
    got = mm.expected_renorm("R", 2, w, [0, 1, 0])
    assert np.array_equal(got[[0, 2]], w[[0, 2]])
    assert np.abs(np.linalg.norm(got[1], axis=1) - 1).max() < 1e-15
    base = [np.array([[1.5, 0.5]]), np.array([[0.25, 0.25]]), None]
    up = [np.array([[1.75, 0.5]]), np.array([[0.25, 0.25]]), None]
    down = [np.array([[1.25, 0.5]]), np.array([[0.25, 0.25]]), None]
    got = mm.expected_merge("E", base, [up, down])
    assert np.array_equal(got[0], base[0])  # long, touched by both ranks, summed delta zero: left alone
    got = mm.expected_merge("E", base, [up, base])
    assert abs(np.linalg.norm(got[0][0]) - 1) < 1e-15


# ---- against kb2e_amd.distributed.TableMerger over gloo

GLOO_NE, GLOO_NR, GLOO_N = 11, 5, 3


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


class ModelRows:
    """TableMerger's rows object over CPU tensors: expected_renorm on the range."""

    def __init__(self, model, tables, shapes):
        self.model, self.tables, self.shapes = model, tables, shapes

    def synchronize(self):
        pass

    def renormalize(self, table, first, count, mask):
        t = self.tables[table].view(self.shapes[table])[first:first + count]
        m = None if mask is None else mask.numpy()
        t.copy_(torch.from_numpy(mm.expected_renorm(self.model, table, t.numpy(), m)))


def _gloo_worker(rank, world, port, model, out):
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    k = mm.build_case(model, GLOO_N, GLOO_NE, GLOO_NR, world)
    present = [t for t in k.base if t is not None]
    # rank 0's tables win the initial broadcast: the others start from garbage
    tables = [torch.tensor(t if rank == 0 else t + 5.0).reshape(-1) for t in present]
    shapes = [t.shape for t in present]
    m = TableMerger(tables, [t.shape[0] for t in present], [int(np.prod(t.shape[1:])) for t in present],
                    ModelRows(model, tables, shapes), dist)
    for t, mine in zip(tables, [x for x in k.ranks[rank] if x is not None]):
        t.copy_(torch.tensor(mine).reshape(-1))
    m.merge()
    out[rank] = [t.numpy().reshape(s).copy() for t, s in zip(tables, shapes)]
    dist.destroy_process_group()


@pytest.mark.timeout(120)
@pytest.mark.parametrize("model", ["E", "R"])
@pytest.mark.parametrize("world", [2, 3])
def test_expected_merge_matches_the_torch_merger(world, model):
    out = mp.Manager().dict()
    mp.spawn(_gloo_worker, args=(world, _free_port(), model, out), nprocs=world, join=True)
    k = mm.build_case(model, GLOO_N, GLOO_NE, GLOO_NR, world)
    assert {"cancel_ent", "cancel_rel"} <= set(k.categories)
    if model == "R":
        assert {"w_single_row", "w_unchanged"} <= set(k.categories)
    exp = mm.expected_merge(model, k.base, k.ranks)
    changed = mm.changed_units(k.base, k.ranks)
    worst = 0.0
    for r in range(world):
        got = iter(out[r])
        for t in range(3):
            if k.base[t] is None:
                continue
            g = next(got)
            worst = max(worst, float(np.abs(g - exp[t]).max()))
            assert np.array_equal(g[~changed[t]], k.base[t][~changed[t]]), (r, t)
    print(f"world {world} model {model}: max |TableMerger - expected_merge| {worst:.3e}")
    assert worst <= 1e-12
