"""The pair rule restated for the tests (include/slime_rs.h, "pair locate";
slime_amd/csrc/locate_rule.hpp, pair_slots): the reference of every GPU test of
test_gpu_locate_pairs.py, pinned to the C++ rule on the same planted cases by
test_locate_pairs_host.py.  Nothing here comes from a kernel.

classify() is the rule on one column in Python integers, as the header states
it: the one-shard rule first (locate_ref.classify), then the two mismatching
rows, then every pair of slots {a, b} whose columns are independent and explain
the syndrome with two non-zero coefficients -- solved with inverses by
elimination, where the C++ rule cross-multiplies.  slots_of_object() is the
same over all columns of one object at once: the computed rows come from
oracle_c.apply_matrix, the one-shard answers from locate_ref.slots_of_object,
and the columns those leave unlocated go through the pairs in uint64 arithmetic
(a product of two values below 2**32 is exact there).
"""
import numpy as np

import locate_ref as R

P = R.P
CLEAN = R.CLEAN
NONE = -1  # no second slot
PAIR_ROWS = 4


def column(coeff, a, i):
    """h_a[i]: the coefficient column of an input, the unit vector of an output row."""
    rows, k = len(coeff), len(coeff[0])
    return int(coeff[i][a]) % P if a < k else (1 if a - k == i else 0)


def _eliminate(coeff, a, b):
    """What solving s = alpha h_a + beta h_b needs and the syndrome does not change: pivot rows
    r1, r2, 1 / h_a[r1], f = h_b[r1] / h_a[r1], 1 / (h_b[r2] - f h_a[r2]); None when h_a and h_b
    are dependent."""
    rows = len(coeff)
    r1 = next((i for i in range(rows) if column(coeff, a, i)), None)
    if r1 is None:
        return None
    inv1 = pow(column(coeff, a, r1), -1, P)
    f = column(coeff, b, r1) * inv1 % P
    for r2 in range(rows):
        v = (column(coeff, b, r2) - f * column(coeff, a, r2)) % P
        if r2 != r1 and v:
            return r1, r2, inv1, f, pow(v, -1, P)
    return None


def explains(coeff, s, a, b):
    e = _eliminate(coeff, a, b)
    if e is None:
        return False
    r1, r2, inv1, f, inv2 = e
    g = s[r1] * inv1 % P
    beta = (s[r2] - g * column(coeff, a, r2)) * inv2 % P
    alpha = (g - beta * f) % P
    return bool(alpha and beta and all(s[i] == (alpha * column(coeff, a, i) + beta * column(coeff, b, i)) % P
                                       for i in range(len(coeff))))


_TABLES = {}


def _tables(coeff):
    """(h, eliminations) of a matrix, computed once: h[a, i] and _eliminate for every a < b."""
    key = (coeff.shape, coeff.tobytes())
    if key not in _TABLES:
        rows, k = coeff.shape
        lists = coeff.tolist()
        h = np.array([[column(lists, a, i) for i in range(rows)] for a in range(k + rows)], dtype=np.uint64)
        _TABLES[key] = h, {(a, b): _eliminate(lists, a, b) for a in range(k + rows) for b in range(a + 1, k + rows)}
    return _TABLES[key]


def classify(coeff, x, stored):
    """(a, b) of one column: a is CLEAN, a slot or k + rows (unlocated) and b NONE, or a < b are the
    two slots of a pair."""
    rows, k = len(coeff), len(coeff[0])
    computed = [sum(int(coeff[i][j]) * int(x[j]) for j in range(k)) % P for i in range(rows)]
    one = R.classify(coeff, x, stored, computed)
    if one != k + rows or rows < PAIR_ROWS:
        return one, NONE
    d = [i for i in range(rows) if int(stored[i]) != computed[i]]
    if len(d) == 2:
        return k + d[0], k + d[1]
    s = [(int(stored[i]) % P - computed[i]) % P for i in range(rows)]
    found = [(a, b) for a in range(k + rows) for b in range(a + 1, k + rows) if explains(coeff, s, a, b)]
    return found[0] if len(found) == 1 else (k + rows, NONE)


def slots_of_object(coeff, ins, stored):
    """(a, b) of every column of one object: two int64 arrays, a CLEAN where clean, b NONE where
    the column is no pair."""
    coeff = np.asarray(coeff, dtype=np.uint32)
    rows, k = coeff.shape
    L = len(stored[0])
    a_out = R.slots_of_object(coeff, ins, stored)
    b_out = np.full(L, NONE, dtype=np.int64)
    open_ = np.flatnonzero(a_out == k + rows)
    if rows < PAIR_ROWS or not open_.size:
        return a_out, b_out
    comp = np.stack([np.asarray(r, dtype=np.uint32) for r in
                     R.OC.apply_matrix(coeff, [np.ascontiguousarray(v)[open_] for v in ins])]).reshape(rows, -1)
    st = np.stack([np.asarray(v, dtype=np.uint32)[open_] for v in stored]).reshape(rows, -1)
    d = st != comp
    two = d.sum(axis=0) == 2
    if two.any():
        a_out[open_[two]] = k + np.argmax(d[:, two], axis=0)
        b_out[open_[two]] = k + rows - 1 - np.argmax(d[::-1, two], axis=0)
    rest = np.flatnonzero(~two)
    if not rest.size:
        return a_out, b_out
    p = np.uint64(P)
    s = (st[:, rest].astype(np.uint64) % p + p - comp[:, rest].astype(np.uint64)) % p
    h, elim = _tables(coeff)
    n = np.zeros(rest.size, dtype=np.int64)
    fa = np.full(rest.size, k + rows, dtype=np.int64)
    fb = np.full(rest.size, NONE, dtype=np.int64)
    for a in range(k + rows):
        for b in range(a + 1, k + rows):
            e = elim[a, b]
            if e is None:
                continue
            r1, r2, inv1, f, inv2 = (np.uint64(v) if i > 1 else v for i, v in enumerate(e))
            g = s[r1] * inv1 % p
            beta = (s[r2] + p - g * h[a, r2] % p) % p * inv2 % p
            alpha = (g + p - beta * f % p) % p
            live = np.flatnonzero((alpha != 0) & (beta != 0))
            for i in range(rows):  # every row, the pivots' too; the columns still in thin out fast
                if not live.size:
                    break
                live = live[s[i, live] == (alpha[live] * h[a, i] % p + beta[live] * h[b, i] % p) % p]
            n[live] += 1
            fa[live], fb[live] = a, b
    single = n == 1
    a_out[open_[rest]] = np.where(single, fa, k + rows)
    b_out[open_[rest]] = np.where(single, fb, NONE)
    return a_out, b_out


def tally(slots, nslots):
    """(counts, first) of one object from its columns' (a, b): a pair counts for both slots."""
    a, b = slots
    ca, fa = R.tally(a, nslots)
    cb, fb = R.tally(b, nslots)  # NONE == CLEAN: columns that are no pair add nothing
    big = np.iinfo(np.int64).max
    first = np.minimum(np.where(fa < 0, big, fa), np.where(fb < 0, big, fb))
    return ca + cb, np.where(first == big, -1, first)


def clean_results(nobj, k, rows):
    return R.clean_results(nobj, k, rows)


def _grouped(coeff, objects, nslots, counts, first, fix=None):
    """Classifies the columns of several objects of one plan in one pass (their shards
    concatenated: the pair enumeration runs once) and tallies each object's own."""
    if not objects:
        return
    ins = [np.concatenate([obj[1][j] for obj in objects]) for j in range(len(objects[0][1]))]
    stored = [np.concatenate([obj[2][i] for obj in objects]) for i in range(len(objects[0][2]))]
    a, b = slots_of_object(coeff, ins, stored)
    at = 0
    for o, i_, s_ in objects:
        L = len(s_[0])
        own = a[at: at + L], b[at: at + L]
        counts[o], first[o] = tally(own if fix is None else fix(own), nslots)
        at += L


def locate_batch(coeff, in_shards, out_shards, src, src_places, cmp, cmp_places, lengths, skip=()):
    """locate_ref.locate_batch under the pair rule."""
    k, rows = len(in_shards), len(out_shards)
    counts, first = clean_results(len(lengths), k, rows)
    objects = []
    for o, L in enumerate(lengths):
        if L == 0 or o in skip:
            continue
        so, ss = src_places[o]
        co, cs = cmp_places[o]
        objects.append((o, [src[so + s * ss: so + s * ss + L] for s in in_shards],
                        [cmp[co + s * cs: co + s * cs + L] for s in out_shards]))
    _grouped(coeff, objects, k + rows + 1, counts, first)
    return counts, first


def set_slots(slots, k, rows, max_rows):
    """(a, b) arrays of an object under its own plan -> its slots in a set's result row
    (planset_locate_ref.set_slot on a; b is a slot of the object's own plan and keeps its number)."""
    a, b = slots
    a = a.copy()
    dirty = a != CLEAN
    if rows < 2:
        a[dirty] = k + max_rows
    else:
        a[dirty & (a == k + rows)] = k + max_rows
    return a, b


def locate_set_batch(plans, plan_of, max_rows, src, src_places, cmp, cmp_places, lengths, no_plan, skip=()):
    """planset_locate_ref.locate_batch under the pair rule: objects whose own plan has four rows or
    more get it, the others the one-shard rule (slots_of_object does that by itself)."""
    k = len(plans[0][1])
    counts, first = clean_results(len(lengths), k, max_rows)
    groups = {}
    for o, L in enumerate(lengths):
        if L == 0 or o in skip or int(plan_of[o]) == no_plan:
            continue
        coeff, in_shards, out_shards = plans[int(plan_of[o])]
        so, ss = src_places[o]
        co, cs = cmp_places[o]
        groups.setdefault(int(plan_of[o]), []).append((o, [src[so + s * ss: so + s * ss + L] for s in in_shards],
                                                       [cmp[co + s * cs: co + s * cs + L] for s in out_shards]))
    for i, objects in groups.items():
        coeff, _, out_shards = plans[i]
        _grouped(coeff, objects, k + max_rows + 1, counts, first,
                 fix=lambda own, r=len(out_shards): set_slots(own, k, r, max_rows))
    return counts, first
