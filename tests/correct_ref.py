"""The correct rule restated for the tests (include/slime_rs.h, "correct";
slime_amd/csrc/correct_rule.hpp), on top of locate_ref / locate_pairs_ref: the
reference of test_gpu_correct.py, pinned to the C++ rule on the same planted
cases by test_correct_host.py.  Nothing here comes from a kernel.

correct_column() is the rule on one column in Python integers, as the header
states it: the slots come from the locate references, a named output row becomes
the row computed over the corrected inputs, a named input x_j becomes
x_j + s_r / c[r][j] with pow(c, -1, p), a pair is solved by elimination (where
the C++ rule takes Cramer's numerators over one Fermat inverse).  The batch
helpers give every column's slots from host copies, their tally, and the buffer
a correct call must leave behind -- built from the CLEAN buffer and the test's
own damage, never from what a correction computes.
"""
import numpy as np

import locate_pairs_ref as PR
import locate_ref as R

P = R.P
CLEAN = R.CLEAN
NONE = PR.NONE


def correct_column(coeff, x, stored, max_wrong=1):
    """(a, b, x after, stored after) of one column: a is CLEAN, a slot or k + rows (unlocated), b
    NONE unless the column is a pair.  x and stored are Python ints (any uint32)."""
    rows, k = len(coeff), len(coeff[0])
    x, stored = [int(v) for v in x], [int(v) for v in stored]
    a, b = PR.classify(coeff, x, stored) if max_wrong == 2 else (R.classify(coeff, x, stored), NONE)
    if a == CLEAN or a == k + rows:
        return a, b, x, stored
    computed = [sum(int(coeff[i][j]) * x[j] for j in range(k)) % P for i in range(rows)]
    s = [(stored[i] % P - computed[i]) % P for i in range(rows)]
    fixed = list(x)
    if b == NONE:
        if a < k:
            r = next((i for i in range(rows) if int(coeff[i][a]) % P), None)
            if r is None:  # an all-zero coefficient column: unsolvable -> unlocated, nothing written
                return k + rows, NONE, x, stored
            fixed[a] = (x[a] + s[r] * pow(int(coeff[r][a]) % P, -1, P)) % P
    else:
        e = PR._eliminate(coeff, a, b)
        r1, r2, inv1, f, inv2 = e
        g = s[r1] * inv1 % P
        beta = (s[r2] - g * PR.column(coeff, a, r2)) * inv2 % P
        alpha = (g - beta * f) % P
        for slot, d in ((a, alpha), (b, beta)):
            if slot < k:
                fixed[slot] = (x[slot] + d) % P
    out = list(stored)
    for slot in (a, b):
        if slot != NONE and slot >= k:  # the row over the corrected inputs
            out[slot - k] = sum(int(coeff[slot - k][j]) * fixed[j] for j in range(k)) % P
    return a, b, fixed, out


def object_slots(coeff, ins, stored, max_wrong):
    """(a, b) int64 arrays of every column of one object under the launch's rule."""
    if max_wrong == 2:
        return PR.slots_of_object(coeff, ins, stored)
    a = R.slots_of_object(coeff, ins, stored)
    return a, np.full(len(a), NONE, dtype=np.int64)


def batch_slots(coeff, in_shards, out_shards, src, src_places, cmp, cmp_places, lengths, max_wrong, skip=()):
    """{object: (a, b)} of a one-plan batch from host copies; objects in `skip` and L == 0 are absent."""
    out = {}
    for o, L in enumerate(lengths):
        if L == 0 or o in skip:
            continue
        so, ss = src_places[o]
        co, cs = cmp_places[o]
        out[o] = object_slots(coeff, [src[so + s * ss: so + s * ss + L] for s in in_shards],
                              [cmp[co + s * cs: co + s * cs + L] for s in out_shards], max_wrong)
    return out


def set_batch_slots(plans, plan_of, max_rows, h, places, lengths, no_plan, max_wrong, skip=()):
    """batch_slots for a planned batch in place: every object under its own plan (coeff, inputs,
    outputs), its slots moved into the set's result row (`unlocated` is k + max_rows)."""
    out = {}
    for o, L in enumerate(lengths):
        if L == 0 or o in skip or int(plan_of[o]) == no_plan:
            continue
        coeff, in_shards, out_shards = plans[int(plan_of[o])]
        off, ss = places[o]
        own = object_slots(coeff, [h[off + s * ss: off + s * ss + L] for s in in_shards],
                           [h[off + s * ss: off + s * ss + L] for s in out_shards], max_wrong)
        out[o] = PR.set_slots(own, len(in_shards), len(out_shards), max_rows)
    return out


def results(slots, nobj, nslots):
    """(counts, first) of a batch from batch_slots' answer; absent objects keep (0, -1)."""
    counts = np.zeros((nobj, nslots), dtype=np.int64)
    first = np.full((nobj, nslots), -1, dtype=np.int64)
    for o, own in slots.items():
        counts[o], first[o] = PR.tally(own, nslots)
    return counts, first


def left_columns(slots, unlocated):
    """{object: bool mask of the columns the rule leaves unlocated}."""
    return {o: a == unlocated for o, (a, _) in slots.items()}


def healed(clean, damaged, spans, canonical=True):
    """The buffer a correct call leaves: `clean`, with the original's canonical residue at every
    word the test damaged (canonical=False: the original word itself -- chunk bytes, whose symbols
    are canonical) -- except in the columns a span keeps, where the damaged words stay.  clean and
    damaged are uint32 views of the same layout; spans: [((offset, shard stride), L, shards, keep)]
    with keep None (the object is corrected), True (it is not touched) or a bool mask of columns."""
    out = np.array(clean, dtype=np.uint32)
    for (off, ss), L, shards, keep in spans:
        for s in shards:
            sl = slice(off + s * ss, off + s * ss + L)
            c, d = clean[sl], damaged[sl]
            diff = d != c
            stay = diff & (np.ones(L, dtype=bool) if keep is True else np.zeros(L, dtype=bool) if keep is None else keep)
            w = out[sl]
            fix = diff & ~stay
            w[fix] = c[fix] % np.uint32(P) if canonical else c[fix]
            w[stay] = d[stay]
    return out
