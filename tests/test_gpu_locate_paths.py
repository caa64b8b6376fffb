"""The parts of the locate kernels (rs_locate_ragged_kernel.hpp) that test_gpu_locate.py and
test_gpu_planset_locate.py do not reach:

  A. dense damage -- every column of an object wrong, each in a shard of its own, so a wave's
     fold (tally_slots) meets many distinct slots at once and several waves meet in the atomics;
  B. the order of `first` -- the rare path walks word-then-unit, not column order, and Tally::add
     must keep the lowest column whichever comes first;
  C. row blocks past the first (plans of 3, 5, 8, 9, 47 and 60 rows: flag_tile's block loop, its
     clipped last block) and all 63 slots in use (16/63, 3/63, 61/63, 17/63: `unlocated` in lane 63);
  D. src and cmp as different tensors with different offsets and shard strides;
  E. single plans whose input and output indices are a permutation (reconstruct-shaped plans).

Every expectation comes from tests/locate_ref.py or tests/planset_locate_ref.py on host copies,
with coefficient rows from the oracle (parity_matrix, invert_matrix) pinned to
plan.coefficients() -- never from a kernel.  Every case runs through the symbol and the byte
entry point (mappings 0, 1 << 31 and random values per object), as the plan and as a one-plan
PlanSet, without a filter and with the matching ragged verify's counts as the filter; that
verify is itself compared with the oracle's rows (expect_batch).  Result arrays are pre-filled
with garbage and the data buffers are compared with their host copies after the launches.
"""
import numpy as np
import pytest

import locate_ref as R
import planset_locate_ref as SR
from oracle import oracle_c as OC
from slime_amd import _native as N
from test_gpu_locate import plant, planted_words, raw_locate, to_chunks
from test_gpu_planset_locate import blank, planned_batch, raw_set_locate, scrub_set, set_reference
from test_gpu_ragged import P, SENTINEL, encode_case, encode_plan, geometry, shard, to_dev, to_host, torch_dev  # noqa: F401
from test_gpu_ragged_verify import assert_results, expect_batch, flip_positions, host, step_boundaries, step_rule
from test_gpu_verify import expected

pytestmark = pytest.mark.gpu

# Plans whose rows do not fit the R = 4 stored rows a step carries, or fit them with a clipped row:
# 4/7 (3 rows), 3/8 (5), 3/11 (8), 3/12 and 8/17 (9), 16/63 (47, the widest vector form), 3/63
# (60), and the column form with all 63 slots, 61/63 (cand has 61 bits) and 17/63.
ROW_CODES = [(4, 7), (3, 8), (3, 11), (3, 12), (8, 17), (16, 63), (3, 63), (61, 63), (17, 63)]
DENSE_CODES = [(3, 5), (8, 12), (16, 20), (17, 20)] + ROW_CODES
# need, total, have (data and parity mixed, out of order), want (all the other shards)
PERMUTED = [(4, 6, [5, 2, 4, 1], [0, 3]),
            (8, 12, [11, 0, 9, 3, 4, 10, 6, 1], [7, 2, 8, 5]),
            (17, 20, [18, 3, 0, 19, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 1], [4, 17, 2])]


# ------------------------------------------------------------------ helpers

class Lay:
    """One plan over one batch layout: the plan and a one-plan PlanSet of it, an unplanned and a
    planned Batch of the same spans, and what the references need -- coefficient rows (checked
    against the plan's), the input and output shards, the places of the src and the cmp side and
    how many shards an object has in each buffer (for the byte form of the buffers)."""

    def __init__(self, plan, coeff, ins, outs, lengths, sp, cp=None, nsrc=None, ncmp=None):
        from slime_amd import device as D
        assert np.array_equal(plan.coefficients(), coeff), "the oracle's rows are the plan's"
        self.plan, self.coeff, self.ins, self.outs = plan, coeff, list(ins), list(outs)
        self.k, self.rows, self.n = len(self.ins), len(self.outs), len(self.ins) + len(self.outs)
        self.lengths, self.sp, self.cp = list(lengths), sp, sp if cp is None else cp
        self.nsrc, self.ncmp = nsrc, nsrc if ncmp is None else ncmp
        spans = [(so, ss, do, ds, L) for (so, ss), (do, ds), L in zip(self.sp, self.cp, self.lengths)]
        self.batch = D.Batch(spans, self.k)
        self.pbatch = D.Batch(spans, self.k, plans=np.zeros(len(spans), dtype=np.uint32), nplans=1)
        self.pset = D.PlanSet([plan])
        assert (self.pset.nplans, self.pset.k, self.pset.max_rows) == (1, self.k, self.rows)
        assert self.pset.locate_slots(0) == plan.locate_slots() == self.ins + self.outs

    def reference(self, src_h, cmp_h=None, skip=()):
        return R.locate_batch(self.coeff, self.ins, self.outs, src_h, self.sp, src_h if cmp_h is None else cmp_h,
                              self.cp, self.lengths, skip)

    def slots(self, o, src_h, cmp_h=None):
        """locate_ref's slot of every column of object o."""
        L, c = self.lengths[o], src_h if cmp_h is None else cmp_h
        return R.slots_of_object(self.coeff, [shard(src_h, self.sp[o], s, L) for s in self.ins],
                                 [shard(c, self.cp[o], s, L) for s in self.outs])


def encode_lay(need, total, lengths, places):
    """The encode plan in place: inputs 0..need-1, outputs need..total-1, the oracle's parity rows."""
    return Lay(encode_plan(need, total), OC.parity_matrix(need, total - need)[need:], range(need), range(need, total),
               lengths, places, nsrc=total)


def mappings(nobj, seed):
    rng = np.random.default_rng(seed)
    return [[0, 1 << 31, int(rng.integers(0, 2**32))][o % 3] for o in range(nobj)]


def run_ways(torch, lay, src_h, cmp_h=None, exp=None, cleared=None, what=None):
    """Every way of asking: the plan and the one-plan set, symbols and bytes, without a filter,
    with the matching verify's counts (themselves compared with the oracle's rows), and -- for
    `cleared`, an object -- with that object's filter row zeroed by hand, which keeps its initial
    values whatever its data says.  Returns the reference's (counts, first)."""
    from slime_amd import device as D
    exp = lay.reference(src_h, cmp_h) if exp is None else exp
    cmp_ = src_h if cmp_h is None else cmp_h
    vexp = expect_batch(lay.coeff, lay.ins, lay.outs, src_h, lay.sp, cmp_, lay.cp, lay.lengths)
    exp_cleared = None if cleared is None else lay.reference(src_h, cmp_h, skip=(cleared,))
    ms = mappings(len(lay.lengths), lay.k * 131 + lay.rows)
    mt = to_dev(torch, np.array(ms, dtype=np.uint32))
    s = to_dev(torch, src_h)
    c = s if cmp_h is None else to_dev(torch, cmp_h)
    sb_h = to_chunks(src_h, lay.sp, lay.lengths, lay.nsrc, ms)
    cb_h = sb_h if cmp_h is None else to_chunks(cmp_h, lay.cp, lay.lengths, lay.ncmp, ms)
    sb = torch.from_numpy(sb_h.copy()).cuda()
    cb = sb if cmp_h is None else torch.from_numpy(cb_h.copy()).cuda()
    for who, batch, raw in ((lay.plan, lay.batch, raw_locate), (lay.pset, lay.pbatch, raw_set_locate)):
        for mapping, a, b in ((None, s, c), (mt, sb, cb)):
            tag = (what, type(who).__name__, "symbols" if mapping is None else "bytes")
            mism = who.verify_batch(a, b, batch) if mapping is None else D.verify_objects_batch(who, a, b, batch, mt)
            assert_results(host(torch, mism), vexp, tag + ("verify",))
            assert_results(host(torch, raw(torch, who, batch, a, b, mapping=mapping)), exp, tag + ("no filter",))
            assert_results(host(torch, raw(torch, who, batch, a, b, mapping=mapping, filter=mism[0])), exp,
                           tag + ("verify's counts as the filter",))
            if cleared is not None:
                hand = mism[0].clone()
                hand[cleared] = 0
                assert_results(host(torch, raw(torch, who, batch, a, b, mapping=mapping, filter=hand)), exp_cleared,
                               tag + ("a filter row cleared by hand",))
    assert np.array_equal(to_host(torch, s), src_h) and np.array_equal(sb.cpu().numpy(), sb_h), "locate writes only results"
    if cmp_h is not None:
        assert np.array_equal(to_host(torch, c), cmp_h) and np.array_equal(cb.cpu().numpy(), cb_h)
    return exp


def tallied(nobj, n, slots_of):
    """(counts, first) from planted per-column slots {object: int array, -1 where clean}."""
    ec, ef = R.clean_results(nobj, n, 0)
    for o, sl in slots_of.items():
        ec[o], ef[o] = R.tally(np.asarray(sl, dtype=np.int64), n + 1)
    return ec, ef


# ------------------------------------------------------------------ A. dense damage

def dense_lengths(k):
    """Several waves on one object (three units and a tail), a wave and a bit, one vector and two
    tail columns, tail columns only, nothing -- and an undamaged object between them."""
    T, C = geometry(k)
    return [2 * C * T + T + 7, T + 1, 6, T + 1, 3, 0], (0, 1, 2, 4)


def dense_damage(h, lay, damaged, seed, second):
    """One wrong word in every column of every damaged object, in a shard drawn uniformly from all
    of the plan's; with `second`, about 2% of the columns get a second wrong shard.  The words cycle
    EDGES and random values; an input differs mod p, a stored row bitwise.  Returns the planted
    slot of every column (the first shard's) per object."""
    rng = np.random.default_rng(seed)
    words = planted_words(seed)
    shards = lay.ins + lay.outs
    planted, i = {}, 0
    for o in damaged:
        L = lay.lengths[o]
        slots = rng.integers(0, lay.n, size=L)
        two = (rng.random(L) < 0.02) if second else np.zeros(L, dtype=bool)
        other = rng.integers(1, lay.n, size=L)
        for col in range(L):
            for sl in [int(slots[col])] + ([int(slots[col] + other[col]) % lay.n] if two[col] else []):
                plant(h, lay.sp[o], L, shards[sl], col, words[i % len(words)], sl < lay.k)
                i += 1
        planted[o] = slots
    return planted


def run_dense(torch, lay, clean_h, damaged, seed, second):
    h = clean_h.copy()
    planted = dense_damage(h, lay, damaged, seed, second)
    exp = lay.reference(h)
    nobj = len(lay.lengths)
    for o in range(nobj):  # the condition, on the reference, before the GPU is asked
        if o not in damaged:
            assert exp[0][o].sum() == 0 and (exp[1][o] == -1).all(), ("undamaged", o)
    if not second:
        for o in damaged:
            assert np.array_equal(lay.slots(o, h), planted[o]), ("the reference names the planted shard in every column", o)
        assert_results(exp, tallied(nobj, lay.n, planted), "counts are the planted histogram, nothing unlocated")
        assert (exp[0][:, lay.n] == 0).all()
    else:
        for o in damaged:
            if lay.lengths[o] > 2 * geometry(lay.k)[0]:  # the multi-unit object: not vacuous
                assert exp[0][o, lay.n] >= 1, "the reference leaves some two-shard column unlocated"
                assert exp[0][o, :lay.n].sum() >= lay.lengths[o] * 9 // 10
    run_ways(torch, lay, h, exp=exp, cleared=damaged[0], what=("dense", second))


@pytest.mark.parametrize("second", [False, True], ids=["one-shard", "second-shard"])
@pytest.mark.parametrize("need,total", DENSE_CODES)
def test_dense_damage_every_column_a_shard_of_its_own(torch_dev, need, total, second):
    """Every column of four objects wrong, each in a shard drawn from all `total`: a wave's fold
    meets up to 64 columns of many slots at once, three units of one object meet in the atomics,
    and the tail items add theirs.  17/20, 61/63 and 17/63 take the column form."""
    lengths, damaged = dense_lengths(need)
    _, want, places, _ = encode_case(need, total, lengths, 1, seed=need * 4001 + total)
    lay = encode_lay(need, total, lengths, places)
    assert lay.batch.units >= 3
    run_dense(torch_dev, lay, want, damaged, need * 4003 + total + second, second)


# ------------------------------------------------------------------ B. the order of `first`

@pytest.mark.parametrize("need,total", [(3, 5), (8, 12)])
def test_first_is_the_lowest_column_in_whatever_order_they_are_met(torch_dev, need, total):
    """Two wrong words of one slot per pair, in an object of two tiles and a tail.  The rare path
    walks q = 4 * unit + word and, inside one q, the lanes: (41, 44) is met higher column first
    (lane 11's word 0 before lane 10's word 1), (80, 85) lower first, (39, 276) is unit 0's word 3
    and unit 1's word 0 of one step, (T - 1, T) the last column of a tile and the first of the next,
    (2, 2 T + 1) vector 0 and a tail item's atomic.  Object o puts pair p on slot (p + o) % total."""
    T, _ = geometry(need)
    rows = total - need
    assert step_rule(need, rows)[0] >= 512, "a step holds two units: columns 256..511 are unit 1 of step 0"
    L = 2 * T + 3
    pairs = [(41, 44), (80, 85), (39, 276), (T - 1, T), (2, 2 * T + 1)]
    lengths = [L] * total
    _, want, places, _ = encode_case(need, total, lengths, 1, seed=need * 4007 + total)
    lay = encode_lay(need, total, lengths, places)
    h = want.copy()
    ec, ef = R.clean_results(total, need, rows)
    words = planted_words(need * 4007 + total)
    for o in range(total):
        for p, (lo, hi) in enumerate(pairs):
            slot = (p + o) % total
            for col in (hi, lo):
                plant(h, places[o], L, slot, col, words[(5 * o + p + col) % len(words)], slot < need)
            ec[o, slot], ef[o, slot] = 2, lo
    exp = lay.reference(h)
    assert_results(exp, (ec, ef), "the reference: two columns a slot, the lower one first")
    run_ways(torch_dev, lay, h, exp=exp, what="first")


# ------------------------------------------------------------------ C. row counts and slot limits

def boundary_objects(need, total):
    """At least `total` objects over the boundary lengths of a vector, a wave, a tile and a unit."""
    T, C = geometry(need)
    base = [1, 3, 4, 5, 257, T - 1, T, T + 1, C * T + 1]
    return [base[(o + o // len(base)) % len(base)] for o in range(max(total, len(base)))]


@pytest.mark.parametrize("need,total", ROW_CODES)
def test_row_blocks_past_the_first_and_all_63_slots(torch_dev, need, total):
    """Clean data over the boundary lengths; one wrong word per object with object o on slot
    o % total, so every input and every row of every block is named (rows R, R + 1, the first row
    of the last block and the last row asserted); and two wrong shards in one column, which the
    reference calls unlocated -- slot k + rows, lane 63 of the wave's tally for the 63-slot codes,
    in a whole vector and in a tail item."""
    torch = torch_dev
    rows = total - need
    lengths = boundary_objects(need, total)
    nobj = len(lengths)
    _, want, places, _ = encode_case(need, total, lengths, 1, seed=need * 4013 + total)
    lay = encode_lay(need, total, lengths, places)
    assert_results(run_ways(torch, lay, want, what="clean"), R.clean_results(nobj, need, rows),
                   "the reference finds oracle codewords clean")
    # one wrong word per object
    h = want.copy()
    ec, ef = R.clean_results(nobj, need, rows)
    words = planted_words(need * 4013 + total)
    for o, L in enumerate(lengths):
        slot, q = o % total, flip_positions(L, need, rows)
        col = q[(o + o // total) % len(q)]
        plant(h, places[o], L, slot, col, words[o % len(words)], slot < need)
        ec[o, slot], ef[o, slot] = 1, col
    exp = lay.reference(h)
    assert_results(exp, (ec, ef), "the reference names the planted slot")
    block = 2 if rows <= 2 else 4  # verify_step::stored_rows
    for i in {min(block, rows - 1), min(block + 1, rows - 1), (rows - 1) // block * block, rows - 1}:
        assert exp[0][:, need + i].sum() >= 1, ("row", i, "is named")
    assert (exp[0][:, :total].sum(axis=0) >= 1).all() and (exp[0][:, total] == 0).all()
    run_ways(torch, lay, h, exp=exp, what="one wrong word")
    # two wrong shards in one column: unlocated
    h = want.copy()
    ec, ef = R.clean_results(nobj, need, rows)
    kinds = [(0, need - 1), (1 % need, need), (need, total - 1), (need - 1, total - 1)]  # input+input ... input+row
    hit = 0
    for o, L in enumerate(lengths):
        if L < 3 or (o % 2 and L != 3):
            continue
        col = 2 if L == 3 else [L // 4 * 4 - 3, 0, L // 4 * 2][hit % 3]  # a tail item; the last, first, a middle vector
        for sh in kinds[hit % len(kinds)]:
            plant(h, places[o], L, sh, col, words[(o + sh) % len(words)], sh < need)
        ec[o, total], ef[o, total] = 1, col
        hit += 1
    assert hit >= 4 and any(L == 3 and ec[o, total] for o, L in enumerate(lengths))
    exp = lay.reference(h)
    assert_results(exp, (ec, ef), "the reference says unlocated")
    run_ways(torch, lay, h, exp=exp, what="unlocated")


def set_verify_reference(plans, plan_of, max_rows, h, places, lengths):
    """PlanSet.verify_batch's (mismatches, first) from the oracle's rows, every object by its own plan."""
    em, ef = np.zeros((len(lengths), max_rows), dtype=np.int64), np.full((len(lengths), max_rows), -1, dtype=np.int64)
    for o, L in enumerate(lengths):
        if L and int(plan_of[o]) != N.NO_PLAN:
            coeff, have, want = plans[int(plan_of[o])]
            r = len(want)
            em[o, :r], ef[o, :r] = expected(coeff, [np.ascontiguousarray(shard(h, places[o], s, L)) for s in have],
                                            [shard(h, places[o], s, L) for s in want])
    return em, ef


def test_scrub_set_with_nine_rows_down_to_one(torch_dev):
    """PlanSet.for_scrub(3, 12) with 0 to 8 shards missing per object: max_rows = 9, and plans of
    9 down to 2 rows beside one-row plans in one launch (R = 4 from max_rows; row_bases and
    flag_tile clip to each object's own rows).  Every column of every object has one wrong word in
    a present shard of its own: objects of two rows or more name it, one-row objects report all L
    columns unlocated.  Checked against planset_locate_ref."""
    torch = torch_dev
    from slime_amd import device as D
    need, total, max_rows = 3, 12, 9
    T, C = geometry(need)
    rng = np.random.default_rng(4019)
    lengths, missing = [], []
    for m in range(9):
        for L in (T + 1, 5, C * T + 1):
            lengths.append(L)
            missing.append(tuple(sorted(int(x) for x in rng.choice(total, size=m, replace=False))))
    nobj = len(lengths)
    _, want, places, _ = encode_case(need, total, lengths, 1, seed=4021)
    pset, plan_of, plans = scrub_set(need, total, missing)
    assert pset.max_rows == max_rows and {len(p[2]) for p in plans} == set(range(1, 10))
    batch = planned_batch(lengths, places, need, plan_of, pset.nplans)
    clean = want.copy()
    blank(clean, places, lengths, missing)
    h = clean.copy()
    words = planted_words(4021)
    planted, i = {}, 0
    for o, L in enumerate(lengths):
        coeff, have, want_ = plans[plan_of[o]]
        shards = have + want_
        slots = rng.integers(0, len(shards), size=L)
        for col in range(L):
            sl = int(slots[col])
            plant(h, places[o], L, shards[sl], col, words[i % len(words)], sl < need)
            i += 1
        planted[o] = slots if len(want_) >= 2 else np.full(L, need + max_rows)  # one row: all unlocated
    ms = mappings(nobj, 4027)
    mt = to_dev(torch, np.array(ms, dtype=np.uint32))
    for name, hb in (("clean", clean), ("dense", h)):
        exp = set_reference(plans, plan_of, max_rows, hb, places, lengths)
        want_res = tallied(nobj, need + max_rows, planted) if name == "dense" else SR.clean_results(nobj, need, max_rows)
        assert_results(exp, want_res, ("the reference names every planted shard; one-row objects are unlocated", name))
        vexp = set_verify_reference(plans, plan_of, max_rows, hb, places, lengths)
        buf = to_dev(torch, hb)
        bytes_h = to_chunks(hb, places, lengths, total, ms)
        bbuf = torch.from_numpy(bytes_h.copy()).cuda()
        for mapping, b in ((None, buf), (mt, bbuf)):
            mism = pset.verify_batch(b, b, batch) if mapping is None else D.verify_objects_batch(pset, b, b, batch, mt)
            assert_results(host(torch, mism), vexp, (name, "verify", mapping is None))
            assert_results(host(torch, raw_set_locate(torch, pset, batch, b, b, mapping=mapping)), exp, (name, mapping is None))
            assert_results(host(torch, raw_set_locate(torch, pset, batch, b, b, mapping=mapping, filter=mism[0])), exp,
                           (name, "filter", mapping is None))
        assert np.array_equal(to_host(torch, buf), hb) and np.array_equal(bbuf.cpu().numpy(), bytes_h)


# ------------------------------------------------------------------ D. separate layouts

@pytest.mark.parametrize("need,total", [(3, 5), (8, 12), (17, 20)])
def test_separate_cmp_tensor_with_its_own_spans(torch_dev, need, total):
    """test_gpu_ragged_verify's layout: src holds the data shards packed with stride L (its parity
    slots hold a sentinel here); cmp is another tensor that holds only the parity rows, objects in
    reverse order behind a gap, odd shard strides (L rounded to 8, plus 1); the plan's outputs are
    cmp shards 0..rows-1.  A wrong input word in src and a wrong row word in cmp, in different
    objects and both in one, are each named by their own slot; then the same through
    Plan.locate_batch and PlanSet.locate_batch with non-zero src_offset / cmp_offset."""
    torch = torch_dev
    from slime_amd import device as D
    rows = total - need
    T, C = geometry(need)
    lengths = [T + 1, 0, 3, C * T + 5, 257, 4, 2 * T + 2] + [c + 1 for c in step_boundaries(need, rows)]
    nobj = len(lengths)
    _, want, sp, _ = encode_case(need, total, lengths, 1, seed=need * 4049 + total)
    cp, off = [None] * nobj, 9
    for o in reversed(range(nobj)):
        ss = -(-lengths[o] // 8) * 8 + 1
        cp[o] = (off, ss)
        off += rows * ss + 3
    cmp_clean = np.full(off + 4, SENTINEL, dtype=np.uint32)
    src_clean = want.copy()
    for o, L in enumerate(lengths):
        for i in range(rows):
            shard(cmp_clean, cp[o], i, L)[:] = shard(want, sp[o], need + i, L)
            shard(src_clean, sp[o], need + i, L)[:] = SENTINEL
    plan = D.Plan.encode(need, total)  # outputs 0..rows-1
    lay = Lay(plan, OC.parity_matrix(need, rows)[need:], range(need), range(rows), lengths, sp, cp, nsrc=total, ncmp=rows)
    assert_results(run_ways(torch, lay, src_clean, cmp_clean, what="clean"), R.clean_results(nobj, need, rows))
    src_h, cmp_h = src_clean.copy(), cmp_clean.copy()
    ec, ef = R.clean_results(nobj, need, rows)
    words = planted_words(need * 4049 + total)
    seen = set()
    for o, L in enumerate(lengths):
        if L == 0:
            continue
        kind = o % 3 if L > 1 else 0  # an input in src; a row in cmp; both, in columns of their own
        j, i = o % need, (o // 3) % rows
        if kind in (0, 2):
            plant(src_h, sp[o], L, j, L - 1, 0x1234 + o, True)
            ec[o, j], ef[o, j] = 1, L - 1
        if kind in (1, 2):
            plant(cmp_h, cp[o], L, i, 0, words[o % len(words)], False)
            ec[o, need + i], ef[o, need + i] = 1, 0
        seen.add(kind)
    assert seen == {0, 1, 2}
    exp = lay.reference(src_h, cmp_h)
    assert_results(exp, (ec, ef), "the reference names the input in src and the row in cmp")
    run_ways(torch, lay, src_h, cmp_h, exp=exp, cleared=3, what="damaged")
    # offsets through the Python entry points: both tensors behind a few words of padding
    def padded(a, n):
        return to_dev(torch, np.concatenate([np.full(n, SENTINEL, dtype=np.uint32), a]))
    s, c = padded(src_h, 5), padded(cmp_h, 11)
    assert_results(host(torch, plan.locate_batch(s, c, lay.batch, src_offset=5, cmp_offset=11)), exp, "Plan offsets")
    assert_results(host(torch, lay.pset.locate_batch(s, c, lay.pbatch, src_offset=5, cmp_offset=11)), exp, "PlanSet offsets")
    mism = plan.verify_batch(s, c, lay.batch, src_offset=5, cmp_offset=11)
    assert_results(host(torch, plan.locate_batch(s, c, lay.batch, filter=mism[0], src_offset=5, cmp_offset=11)), exp)
    ms = mappings(nobj, need)
    mt = to_dev(torch, np.array(ms, dtype=np.uint32))
    sb = torch.from_numpy(to_chunks(src_h, sp, lengths, total, ms).copy()).cuda()
    cb = torch.from_numpy(to_chunks(cmp_h, cp, lengths, rows, ms).copy()).cuda()
    assert_results(host(torch, D.locate_objects_batch(plan, sb, cb, lay.batch, mt)), exp, "bytes, Plan")
    assert_results(host(torch, D.locate_objects_batch(lay.pset, sb, cb, lay.pbatch, mt)), exp, "bytes, PlanSet")


# ------------------------------------------------------------------ E. permuted single plans

def reconstruct_rows(need, total, have, want):
    """m[want] . m[have]^-1 from the oracle alone, in Python integers."""
    m = OC.parity_matrix(need, total - need)
    rc, inv = OC.invert_matrix(m[have])
    assert rc == 0
    a, b = m[want].astype(object), inv.astype(object)
    return np.array([[sum(int(a[i, t]) * int(b[t, j]) for t in range(need)) % P for j in range(need)]
                     for i in range(len(want))], dtype=np.uint32).reshape(len(want), need)


def permuted_lay(need, total, have, want, lengths, places):
    from slime_amd import device as D
    assert sorted(have + want) == list(range(total)) and have != sorted(have)
    assert any(s < need for s in have) and any(s >= need for s in have) and any(s < need for s in want)
    plan = D.Plan.reconstruct(need, total, have, want).set_outputs(want)
    lay = Lay(plan, reconstruct_rows(need, total, have, want), have, want, lengths, places, nsrc=total)
    assert plan.locate_slots() == have + want
    return lay


def canonical(want, places, lengths, need):
    """The codewords with every data word reduced mod p, as an ingest stores them: a checked data
    shard then equals what the survivors rebuild bit for bit (the parity shards do not change)."""
    h = want.copy()
    for place, L in zip(places, lengths):
        for s in range(need):
            shard(h, place, s, L)[:] %= np.uint32(P)
    return h


@pytest.mark.parametrize("need,total,have,want", PERMUTED)
def test_permuted_single_plan_names_every_shard_by_its_slot(torch_dev, need, total, have, want):
    """Plan.reconstruct with shuffled survivors (data and parity) and every other shard as a checked
    output, in place over the encode plan's layout: object o has one wrong word in shard o, named
    at slot (have + want).index(o).  The single-plan vector kernel reads sb[j] through in_idx[j]
    and classify_column through in_idx / out_idx; 17/20 takes the column form."""
    T, C = geometry(need)
    base = [T + 1, 5, 257, C * T + 1, 3, T, 4]
    lengths = [base[o % len(base)] for o in range(total)]
    _, codeword, places, _ = encode_case(need, total, lengths, 1, seed=need * 4051 + total)
    clean = canonical(codeword, places, lengths, need)
    lay = permuted_lay(need, total, have, want, lengths, places)
    rows = len(want)
    assert_results(run_ways(torch_dev, lay, clean, what="clean"), R.clean_results(total, need, rows))
    h = clean.copy()
    ec, ef = R.clean_results(total, need, rows)
    words = planted_words(need * 4051 + total)
    for o, L in enumerate(lengths):
        slot, q = (have + want).index(o), flip_positions(L, need, rows)
        col = q[o % len(q)]
        plant(h, places[o], L, o, col, words[o % len(words)], slot < need)
        ec[o, slot], ef[o, slot] = 1, col
    exp = lay.reference(h)
    assert_results(exp, (ec, ef), "the reference names every shard by its slot")
    run_ways(torch_dev, lay, h, exp=exp, what="one wrong word")


@pytest.mark.parametrize("need,total,have,want", PERMUTED)
def test_permuted_single_plan_dense_damage(torch_dev, need, total, have, want):
    lengths, damaged = dense_lengths(need)
    _, codeword, places, _ = encode_case(need, total, lengths, 1, seed=need * 4057 + total)
    lay = permuted_lay(need, total, have, want, lengths, places)
    run_dense(torch_dev, lay, canonical(codeword, places, lengths, need), damaged, need * 4073 + total, False)
