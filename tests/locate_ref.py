"""The locate rule restated for the tests (include/slime_rs.h, "ragged locate";
slime_amd/csrc/locate_rule.hpp): the reference of every GPU locate test, and
pinned to the C++ rule on the same planted cases by test_locate_host.py.

classify() is the rule on one column in Python integers.  locate_object() is the
same rule over all columns of one object at once: the computed rows come from
oracle_c.apply_matrix, columns with fewer than two mismatching rows are decided
with array compares, the others go through the relation in uint64 arithmetic
(a product of two values below 2**32 is exact there).  Neither inverts anything.
"""
import numpy as np

from oracle import oracle_c as OC
from slime_amd import gf

P = gf.MaxVal
CLEAN = -1


def classify(coeff, x, stored, computed=None):
    """The slot of one column: coeff rows x k, x the k input words, stored the rows' stored words
    (Python ints, any uint32).  CLEAN, an input 0..k-1, an output row k+i, or k+rows (unlocated)."""
    rows, k = len(coeff), len(coeff[0])
    if computed is None:
        computed = [sum(int(coeff[i][j]) * int(x[j]) for j in range(k)) % P for i in range(rows)]
    d = [int(stored[i]) != int(computed[i]) for i in range(rows)]
    s = [(int(stored[i]) % P - int(computed[i])) % P for i in range(rows)]
    if not any(d):
        return CLEAN
    if sum(d) == 1:
        return k + d.index(True)
    J = [j for j in range(k) if s[0] != 0 and all((s[i] * int(coeff[0][j])) % P == (s[0] * int(coeff[i][j])) % P
                                                  for i in range(rows))]
    return J[0] if len(J) == 1 else k + rows


def slots_of_object(coeff, ins, stored):
    """The slot of every column of one object (int64 array, CLEAN where clean)."""
    coeff = np.asarray(coeff, dtype=np.uint32)
    rows, k = coeff.shape
    L = len(stored[0])
    comp = np.stack([np.asarray(r, dtype=np.uint32) for r in
                     OC.apply_matrix(coeff, [np.ascontiguousarray(v) for v in ins])]).reshape(rows, L)
    st = np.stack([np.asarray(v, dtype=np.uint32) for v in stored]).reshape(rows, L)
    d = st != comp
    nd = d.sum(axis=0)
    out = np.full(L, CLEAN, dtype=np.int64)
    one = nd == 1
    out[one] = k + np.argmax(d[:, one], axis=0)
    many = np.flatnonzero(nd >= 2)
    if many.size:
        s = (st[:, many].astype(np.uint64) % np.uint64(P) + np.uint64(P) - comp[:, many].astype(np.uint64)) % np.uint64(P)
        c = coeff.astype(np.uint64) % np.uint64(P)
        ok = np.zeros((k, many.size), dtype=bool)
        for j in range(k):
            okj = s[0] != 0
            for i in range(rows):
                okj &= (s[i] * c[0, j]) % np.uint64(P) == (s[0] * c[i, j]) % np.uint64(P)
            ok[j] = okj
        nj = ok.sum(axis=0)
        out[many] = np.where(nj == 1, np.argmax(ok, axis=0), k + rows)
    return out


def tally(slots, nslots):
    """(counts, first) of one object from its columns' slots."""
    counts = np.zeros(nslots, dtype=np.int64)
    first = np.full(nslots, -1, dtype=np.int64)
    cols = np.flatnonzero(slots != CLEAN)
    for c in cols[::-1]:
        first[slots[c]] = c
    np.add.at(counts, slots[cols], 1)
    return counts, first


def clean_results(nobj, k, rows):
    return np.zeros((nobj, k + rows + 1), dtype=np.int64), np.full((nobj, k + rows + 1), -1, dtype=np.int64)


def locate_batch(coeff, in_shards, out_shards, src, src_places, cmp, cmp_places, lengths, skip=()):
    """(counts, first) of a whole batch from host copies: src / cmp flat uint32 arrays, places
    [(offset, shard stride)] per object.  Objects in `skip`, and L == 0, keep the initial values."""
    k, rows = len(in_shards), len(out_shards)
    counts, first = clean_results(len(lengths), k, rows)
    for o, L in enumerate(lengths):
        if L == 0 or o in skip:
            continue
        so, ss = src_places[o]
        co, cs = cmp_places[o]
        ins = [src[so + s * ss: so + s * ss + L] for s in in_shards]
        stored = [cmp[co + s * cs: co + s * cs + L] for s in out_shards]
        counts[o], first[o] = tally(slots_of_object(coeff, ins, stored), k + rows + 1)
    return counts, first
