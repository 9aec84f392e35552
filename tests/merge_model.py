"""The epoch merge and the norm constraint restated in numpy float64, and the
cases the merge tests run (tests/test_merge_model.py on the CPU,
tests/test_gpu_merge_shapes.py and tests/test_gpu_renormalize.py on the GPU).
No test functions here.

The merge (kb2e_amd/csrc/engine_merge.inc, kb2e_amd/distributed.TableMerger):

    T <- renorm(T0 + sum_r (T_r - T0))

* the deltas are summed in rank order;
* a unit (a row; for the TransR weights one relation's whole n x n matrix) is
  CHANGED iff its summed delta has a non-zero element -- deltas that cancel
  exactly across the ranks leave the unit alone;
* changed units take the model's constraint: TransE rows and TransH entity /
  relation rows shrink to length <= 1, TransH normals and every TransR row scale
  to unit length; the length is the square root of a sequential sum of squares;
* unchanged units keep the base's bits.

Everything starts from the inputs as the engine holds them: for precision 32
they are rounded through float32 first and all arithmetic is float64 from there.

The case builder makes the SUMMED row first and splits it into the ranks'
deltas, so the guards hold by construction (and `guards` measures them from the
data again): a shrink decision `len > 1` has a margin >= 0.3, every non-zero
delta element is >= 2^-6.
"""
from types import SimpleNamespace

import numpy as np

SHORT, LONG, CHANGED, CANCEL, NODELTA = 0, 1, 2, 3, 4  # what the builder did with a row


def engine_round(t, precision):
    """The table as an engine of this precision holds it (float64 values)."""
    if t is None:
        return None
    t = np.asarray(t, dtype=np.float64)
    return t.astype(np.float32).astype(np.float64) if precision == 32 else t.copy()


def unit_constraint(model, k):
    """True: rows of table k scale to unit length; False: they shrink to length <= 1."""
    return model == "R" or (model == "H" and k == 2)


def seq_len(rows):
    """Row lengths: the square root of a sequential float64 sum of squares."""
    s = np.zeros(rows.shape[0])
    for j in range(rows.shape[1]):
        s += rows[:, j] * rows[:, j]
    return np.sqrt(s)


def expected_renorm(model, table, rows, mask=None):
    """The constraint of `table` (0 entities, 1 relations, 2 weights) on the units
    of `rows` ((U, n), or (U, n, n) for the TransR matrices) whose mask entry is
    non-zero (None: all).  Everything else is returned as it came."""
    a = np.array(rows, dtype=np.float64)
    units = a.shape[0]
    flat = a.reshape(-1, a.shape[-1])
    sel = np.ones(units, bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    assert len(sel) == units
    sel = np.repeat(sel, flat.shape[0] // max(units, 1))
    ln = seq_len(flat)
    if not unit_constraint(model, table):
        sel = sel & (ln > 1)
    out = flat.copy()
    out[sel] = flat[sel] / ln[sel, None]
    return out.reshape(a.shape)


def summed_delta(base, per_rank_tables, k, precision=64):
    b = engine_round(base[k], precision)
    s = np.zeros_like(b)
    for tr in per_rank_tables:  # rank order
        s += engine_round(tr[k], precision) - b
    return b, s


def changed_units(base, per_rank_tables, precision=64):
    """Per table, the units whose SUMMED delta has a non-zero element."""
    out = []
    for k in range(3):
        if base[k] is None:
            out.append(None)
            continue
        b, s = summed_delta(base, per_rank_tables, k, precision)
        out.append((s.reshape(b.shape[0], -1) != 0).any(1))
    return out


def expected_merge(model, base, per_rank_tables, precision=64):
    """renorm(T0 + sum_r (T_r - T0)) per table (None where the model has none)."""
    out = []
    for k in range(3):
        if base[k] is None:
            out.append(None)
            continue
        b, s = summed_delta(base, per_rank_tables, k, precision)
        changed = (s.reshape(b.shape[0], -1) != 0).any(1)
        res = expected_renorm(model, k, b + s, changed)
        res[~changed] = b[~changed]  # the base's bits
        out.append(res)
    return out


def owner_blocks(ne, world):
    """[(lo, count)] of every rank's entity block (count 0: an idle owner)."""
    block = (ne + world - 1) // world
    out = []
    for r in range(world):
        lo = min(ne, r * block)
        out.append((lo, min(ne, lo + block) - lo))
    return out


def guards(model, base, per_rank_tables, precision=64):
    """(smallest |len - 1| of a shrink decision, smallest non-zero |delta|),
    measured from the tables (inf where there is none)."""
    margin, dmin = np.inf, np.inf
    for k in range(3):
        if base[k] is None:
            continue
        b, s = summed_delta(base, per_rank_tables, k, precision)
        for tr in per_rank_tables:
            d = np.abs(engine_round(tr[k], precision) - b)
            if (d != 0).any():
                dmin = min(dmin, float(d[d != 0].min()))
        if not unit_constraint(model, k):
            ch = (s != 0).any(1)
            if ch.any():
                margin = min(margin, float(np.abs(seq_len((b + s)[ch]) - 1).min()))
    return margin, dmin


# ------------------------------------------------------------- the builder

def _directions(rng, rows, n):
    g = rng.standard_normal((rows, n))
    g[:, 0] += np.where(np.abs(g).max(1) < 1e-3, 1.0, 0.0)
    return g / np.linalg.norm(g, axis=1, keepdims=True)


def _off_unit(rng, rows):
    """Lengths in [0.5, 0.9] or [1.1, 2.0]: never a unit row by accident."""
    return np.where(rng.random(rows) < 0.4, rng.uniform(0.5, 0.9, rows), rng.uniform(1.1, 2.0, rows))


def _plan_rows(units, world, forced, want_cancel):
    """What every row of a row table is: forced rows are changed; of the others
    one is the cancellation row, then long-unchanged / changed / short-unchanged
    in turn, topped up to a third long-unchanged."""
    kind = np.full(units, SHORT)
    f = np.zeros(units, bool)
    f[[i for i in forced if 0 <= i < units]] = True
    kind[f] = CHANGED
    free = np.nonzero(~f)[0]
    if want_cancel and world >= 2 and len(free) >= 2:
        kind[free[0]] = CANCEL
        free = free[1:]
    kind[free[0::3]] = LONG
    kind[free[1::3]] = CHANGED
    short = free[2::3]
    lack = units // 3 - int((kind == LONG).sum())
    if lack > 0:
        kind[short[:lack]] = LONG
    return kind


def _changed_specs(rng, rows_changed, n, world, shift=0):
    """Who changes a changed row and where: in turn one rank / element 0 only, all
    ranks / element n - 1 only, then four rows changed throughout by 1..3 ranks
    (table k starts the turn at `shift` = k)."""
    m = len(rows_changed)
    part = np.zeros((m, world), bool)
    elem = np.ones((m, n), bool)
    style = (np.arange(m) + shift) % 6
    one = style == 0
    part[one, (np.arange(m)[one] // 6) % world] = True
    elem[one] = False
    elem[one, 0] = True
    al = style == 1
    part[al] = True
    elem[al] = False
    elem[al, n - 1] = True
    gen = np.nonzero(style >= 2)[0]
    cnt = rng.integers(1, min(world, 3) + 1, len(gen))
    order = np.argsort(rng.random((len(gen), world)), axis=1)
    rank_pos = np.argsort(order, axis=1)  # a random permutation's position of every rank
    part[gen] = rank_pos < cnt[:, None]
    return part, elem, style


def _realise(rng, n, world, kind, part, elem, length, precision):
    """The tables of one row table: (base, [rank tables]).  Changed rows: the
    summed row S of the wanted length first, the total delta D (every selected
    element p * [1, 1.5] / 16 for p ranks), the base S - D, and D split into
    parts no smaller than D / 2p."""
    rows = len(kind)
    summed = _directions(rng, rows, n) * length[:, None]
    base = summed.copy()
    ch =np.nonzero(kind == CHANGED)[0]
    p = part.sum(1)
    mag = rng.uniform(1.0, 1.5, (len(ch), n)) * p[:, None] / 16.0
    delta = np.where(rng.random((len(ch), n)) < 0.5, -mag, mag) * elem
    base[ch] = summed[ch] - delta
    share = (1.0 + rng.random((len(ch), world))) * part
    share /= share.sum(1, keepdims=True)
    # cancellation rows: multiples of 2^-10 below 4, exact in float and double
    cn = np.nonzero(kind == CANCEL)[0]
    base[cn] = np.round(base[cn] * 1024.0) / 1024.0
    cdelta = rng.integers(16, 513, (len(cn), n)) * np.where(rng.random((len(cn), n)) < 0.5, -1, 1) / 1024.0
    base = engine_round(base, precision)
    ranks = []
    for r in range(world):
        t = base.copy()
        t[ch] = base[ch] + delta * share[:, r:r + 1]
        if r == 0:
            t[cn] = base[cn] + cdelta
        if r == world - 1 and world >= 2:
            t[cn] = base[cn] - cdelta
        ranks.append(engine_round(t, precision))
    return base, ranks


def _row_table(rng, units, n, world, unit, forced, precision, cats, k):
    kind = _plan_rows(units, world, forced, want_cancel=True)
    ch = np.nonzero(kind == CHANGED)[0]
    part, elem, style = _changed_specs(rng, ch, n, world, shift=k)
    length = rng.uniform(0.3, 0.5, units)  # short unchanged rows
    lu = kind == LONG
    length[lu] = rng.uniform(1.32, 1.68, int(lu.sum()))
    length[kind == CANCEL] = 1.5
    if unit:
        length[ch] = _off_unit(rng, len(ch))
    else:  # half short, half long
        lng = np.arange(len(ch)) % 2 == 0
        length[ch] = np.where(lng, rng.uniform(1.52, 1.98, len(ch)), rng.uniform(0.52, 0.68, len(ch)))
        cats["shrink_long"] += [(k, int(i)) for i in ch[lng][:4]]
        cats["shrink_short"] += [(k, int(i)) for i in ch[~lng][:4]]
    cats["one_rank"] += [(k, int(i)) for i in ch[part.sum(1) == 1][:4]]
    if world >= 2:
        cats["all_ranks"] += [(k, int(i)) for i in ch[part.sum(1) == world][:4]]
    cats["elem0_only"] += [(k, int(i)) for i in ch[style == 0][:4]]
    cats["elem_last_only"] += [(k, int(i)) for i in ch[style == 1][:4]]
    cats["long_unchanged"] += [(k, int(i)) for i in np.nonzero(lu)[0][:8]]
    cats["cancel_ent" if k == 0 else "cancel_rel" if k == 1 else "cancel_w"] += [
        (k, int(i)) for i in np.nonzero(kind == CANCEL)[0]]
    base, ranks = _realise(rng, n, world, kind, part, elem, length, precision)
    return base, ranks, kind


def _matrix_table(rng, nr, n, world, precision, cats):
    """The TransR weights, as nr * n rows.  Relation u, by u % 5: 0 changed
    throughout; 1 a delta in ONE matrix row (all n rows are renormalised); 2 no
    delta, non-unit rows (bit-identical); 3 changed by every rank; 4 one rank, the
    last element of the last row only."""
    rows = nr * n
    kind = np.full(rows, NODELTA)
    part = []
    elem = []
    for u in range(nr):
        r0, what = u * n, u % 5
        if what == 0 or what == 3:
            kind[r0:r0 + n] = CHANGED
            for _ in range(n):
                pr = np.ones(world, bool)
                if what == 0:
                    pr = np.zeros(world, bool)
                    pr[rng.permutation(world)[:rng.integers(1, min(world, 3) + 1)]] = True
                part.append(pr)
                elem.append(np.ones(n, bool))
        elif what == 1:
            kind[r0 + min(1, n - 1)] = CHANGED
            pr = np.zeros(world, bool)
            pr[rng.permutation(world)[:min(world, 2)]] = True
            part.append(pr)
            elem.append(np.ones(n, bool))
            cats["w_single_row"].append((2, u))
        elif what == 2:
            kind[r0:r0 + n] = LONG
            cats["w_unchanged"].append((2, u))
        else:
            kind[r0 + n - 1] = CHANGED
            pr = np.zeros(world, bool)
            pr[u % world] = True
            part.append(pr)
            el = np.zeros(n, bool)
            el[n - 1] = True
            elem.append(el)
            cats["w_last_element"].append((2, u))
    part = np.array(part).reshape(-1, world)
    elem = np.array(elem).reshape(-1, n)
    base, ranks = _realise(rng, n, world, kind, part, elem, _off_unit(rng, rows), precision)
    shape = (nr, n, n)
    return base.reshape(shape), [t.reshape(shape) for t in ranks], kind


def build_case(model, n, ne, nr, world, precision=64, seed=0):
    """One merge case: base tables, every rank's tables, the categories placed
    ((table, unit) lists), the owners' blocks and the measured guards."""
    rng = np.random.default_rng([seed, n, ne, nr, world, precision, "EHR".index(model)])
    cats = {c: [] for c in ("owner_first", "owner_last", "row0", "row_last", "one_rank", "all_ranks", "elem0_only",
                            "elem_last_only", "long_unchanged", "shrink_long", "shrink_short", "cancel_ent",
                            "cancel_rel", "cancel_w", "w_single_row", "w_unchanged", "w_last_element")}
    owners = owner_blocks(ne, world)
    forced = [0, ne - 1]
    for lo, cnt in owners:
        if cnt:
            forced += [lo, lo + cnt - 1]
            cats["owner_first"].append((0, lo))
            cats["owner_last"].append((0, lo + cnt - 1))
    cats["row0"].append((0, 0))
    cats["row_last"].append((0, ne - 1))
    base, ranks, kinds = [None] * 3, [[None] * 3 for _ in range(world)], [None] * 3
    ntab = 2 if model == "E" else 3
    for k in range(ntab):
        if k == 2 and model == "R":
            b, rs, kind = _matrix_table(rng, nr, n, world, precision, cats)
        else:
            units = ne if k == 0 else nr
            b, rs, kind = _row_table(rng, units, n, world, unit_constraint(model, k),
                                     forced if k == 0 else [0, units - 1], precision, cats, k)
        base[k], kinds[k] = b, kind
        for r in range(world):
            ranks[r][k] = rs[r]
    margin, dmin = guards(model, base, ranks, precision)
    return SimpleNamespace(model=model, n=n, ne=ne, nr=nr, world=world, precision=precision, seed=seed, base=base,
                           ranks=ranks, kinds=kinds, categories={c: v for c, v in cats.items() if v},
                           owners=owners, idle=[r for r, (_, cnt) in enumerate(owners) if cnt == 0],
                           min_len_margin=margin, min_delta=dmin)


def second_round(case, merged, seed=1):
    """New rank tables over the merged tables (the moved base).  Every second row
    the first round changed (length <= 1 now) gets, from one rank, a delta t * u
    along its own signs, |u_i| in [1, 1.2], with t solved so that the summed row
    has a length in [1.6, 1.98]: every |delta| >= 0.6 / (1.2 sqrt(n)) > 2^-6 up to
    n = 512, and the row is long by >= 0.6.  Every short unchanged row gets one
    element moved by [1, 1.5] / 16 by one rank and stays below 0.6.  Long
    unchanged rows, the cancellation rows and the unchanged matrices stay."""
    rng = np.random.default_rng([seed, case.seed, case.n, case.ne, case.world])
    world, n, prec = case.world, case.n, case.precision
    base = [engine_round(t, prec) for t in merged]
    ranks = [[None if t is None else t.copy() for t in base] for _ in range(world)]
    for k in range(3):
        if base[k] is None:
            continue
        flat = base[k].reshape(-1, n)
        views = [ranks[r][k].reshape(-1, n) for r in range(world)]
        ch = np.nonzero(case.kinds[k] == CHANGED)[0]
        ch = ch[1::2] if len(ch) > 1 else ch
        if len(ch):
            m = flat[ch]
            u = np.where(m < 0, -1.0, 1.0) * rng.uniform(1.0, 1.2, m.shape)
            want = rng.uniform(1.6, 1.98, len(ch))
            mu, uu, mm = (m * u).sum(1), (u * u).sum(1), (m * m).sum(1)
            t = (-mu + np.sqrt(mu * mu + uu * (want * want - mm))) / uu
            who = np.arange(len(ch)) % world
            for r in range(world):
                sel = who == r
                views[r][ch[sel]] = m[sel] + t[sel, None] * u[sel]
        sh = np.nonzero(case.kinds[k] == SHORT)[0]
        if len(sh):
            who = (np.arange(len(sh)) + 1) % world
            col = np.arange(len(sh)) % n
            d = rng.uniform(1.0, 1.5, len(sh)) / 16.0 * np.where(rng.random(len(sh)) < 0.5, -1, 1)
            for r in range(world):
                sel = who == r
                views[r][sh[sel], col[sel]] += d[sel]
    ranks = [[engine_round(t, prec) for t in tr] for tr in ranks]
    return base, ranks


def renorm_tables(model, n, ne, nr, precision=64, seed=0):
    """Tables for the renormalize tests (no merge): long and short rows mixed, and
    per table a mask with a third of the units off."""
    rng = np.random.default_rng([seed, n, ne, nr, precision, "EHR".index(model), 77])
    tabs, masks = [None] * 3, [None] * 3
    for k in range(2 if model == "E" else 3):
        units = ne if k == 0 else nr
        shape = (units, n, n) if k == 2 and model == "R" else (units, n)
        rows = int(np.prod(shape[:-1]))
        ln = np.where(np.arange(rows) % 2 == 0, rng.uniform(1.3, 2.0, rows), rng.uniform(0.3, 0.7, rows))
        tabs[k] = engine_round((_directions(rng, rows, n) * ln[:, None]).reshape(shape), precision)
        m = np.ones(units, np.uint8)
        m[1::3] = 0
        masks[k] = m
    return tabs, masks


# ------------------------------------------------------ the committed cases

def _case(family, model, n, ne, nr, world, precision=64):
    return SimpleNamespace(id=f"{family}-{model}-n{n}-E{ne}-w{world}-fp{precision}", family=family, model=model, n=n,
                           ne=ne, nr=nr, world=world, precision=precision)


WIDTH_CASES = (
    [_case("width", "E", n, 37, 5, 3) for n in (3, 64, 65, 127, 128, 129, 256, 257, 384, 385, 511, 512)]
    + [_case("width", m, n, 37, 5, 3) for m in "HR" for n in (3, 65, 129, 257, 385, 512)]
    + [_case("width", m, n, 37, 5, 3, 32) for m in "EHR" for n in (65, 129, 385, 512)])
RANK_CASES = (
    [_case("ranks", m, 20, 37, 5, w) for m in "ER" for w in (1, 2, 3, 4, 5, 16)]
    # (TransR contexts need |R| <= |E|)
    + [_case("ranks", "E", 20, 3, 5, 4), _case("ranks", "R", 20, 3, 3, 4)]
    + [_case("ranks", "E", 20, 1, 5, 2), _case("ranks", "R", 20, 1, 1, 2)])
STRIDE_CASES = [_case("stride", "E", 7, 270000, 3, 2)]
RCCL_CASES = [_case("rccl", "H", 65, 37, 5, 1), _case("rccl", "R", 129, 37, 5, 1, 32),
              _case("rccl", "E", 385, 37, 5, 1, 32)]
GROUP_CASES = WIDTH_CASES + RANK_CASES + STRIDE_CASES
ALL_CASES = GROUP_CASES + RCCL_CASES


def build(c, seed=0):
    return build_case(c.model, c.n, c.ne, c.nr, c.world, c.precision, seed)
