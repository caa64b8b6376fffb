"""The plan-set locate's reference (include/slime_rs.h, "plan-set locate"): locate_ref's rule
applied to every object with that object's own plan, then the set's slot numbering -- objects
whose plan has fewer than two rows report every mismatching column as unlocated, and
`unlocated` is slot k + max_rows for every object.  The reference of every GPU test of
test_gpu_planset_locate.py, pinned to the C++ function (locate_rule.hpp, set_slot) on printed
cases by test_planset_locate_host.py.  Nothing here comes from a kernel: the computed rows are
oracle_c.apply_matrix's, over host copies."""
import numpy as np

import locate_ref as R

CLEAN = R.CLEAN


def set_slot(slot, k, rows, max_rows):
    """The slot in a set's result row of a column whose slot under its own plan is `slot`."""
    if slot == CLEAN:
        return CLEAN
    if rows < 2 or slot == k + rows:
        return k + max_rows
    return slot


def classify(coeff, x, stored, max_rows):
    rows, k = len(coeff), len(coeff[0])
    return set_slot(R.classify(coeff, x, stored), k, rows, max_rows)


def slots_of_object(coeff, ins, stored, max_rows):
    """The set slot of every column of one object (int64 array, CLEAN where clean)."""
    coeff = np.asarray(coeff, dtype=np.uint32)
    rows, k = coeff.shape
    own = R.slots_of_object(coeff, ins, stored)
    out = own.copy()
    dirty = own != CLEAN
    if rows < 2:
        out[dirty] = k + max_rows
    else:
        out[dirty & (own == k + rows)] = k + max_rows
    return out


def clean_results(nobj, k, max_rows):
    return R.clean_results(nobj, k, max_rows)


def locate_batch(plans, plan_of, max_rows, src, src_places, cmp, cmp_places, lengths, no_plan, skip=()):
    """(counts, first) of a planned batch from host copies.  plans[i] = (coeff rows_i x k, input
    shards, output shards); plan_of[o] the object's plan or no_plan.  Objects without a plan, in
    `skip`, or with L == 0 keep the initial values, and so do the slots past an object's rows."""
    k = len(plans[0][1])
    counts, first = clean_results(len(lengths), k, max_rows)
    for o, L in enumerate(lengths):
        if L == 0 or o in skip or int(plan_of[o]) == no_plan:
            continue
        coeff, in_shards, out_shards = plans[int(plan_of[o])]
        so, ss = src_places[o]
        co, cs = cmp_places[o]
        ins = [src[so + s * ss: so + s * ss + L] for s in in_shards]
        stored = [cmp[co + s * cs: co + s * cs + L] for s in out_shards]
        counts[o], first[o] = R.tally(slots_of_object(coeff, ins, stored, max_rows), k + max_rows + 1)
    return counts, first
