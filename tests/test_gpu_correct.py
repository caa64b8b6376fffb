"""Correct (slime_rs_plan_correct_batch, slime_rs_correct_objects_batch and their plan-set twins)
on the GPU: the locate launches that also rewrite, in place, every word they name.

No expectation comes from a kernel.  Counts and firsts are tests/correct_ref.py's (the locate
references' slots; pinned to the C++ rule by test_correct_host.py).  The buffer a call must leave
is built from the CLEAN host buffer: at the words the test damaged stands the original's canonical
residue (symbols) or the original bytes (byte form), except in the columns the reference leaves
unlocated and in objects the launch passes over, where the damaged words stay.  Whole buffers are
compared, sentinel gaps included, so a stray write fails.  Before the GPU is asked each case
asserts that the reference alone names what was planted.  All damage is to data values inside the
buffers; shapes are the locate tests' boundary lengths, seeds are fixed.
"""
import ctypes

import numpy as np
import pytest

import correct_ref as CR
from oracle import oracle_c as OC
from slime_amd import _native as N
from test_gpu_locate import plant, planted_words, to_chunks
from test_gpu_locate_paths import (PERMUTED, Lay, boundary_objects, canonical, dense_lengths, encode_lay, mappings,
                                   permuted_lay)
from test_gpu_planset_locate import blank, planned_batch, scrub_set
from test_gpu_ragged import P, SENTINEL, encode_case, geometry, mode, shard, to_dev, to_host, torch_dev  # noqa: F401
from test_gpu_ragged_verify import assert_results, flip_positions, host, verify_lengths
from test_gpu_verify import GARBAGE

pytestmark = pytest.mark.gpu

VECTOR_CODES = [(3, 5), (3, 7), (8, 12), (10, 14), (16, 20)]
COLUMN_CODES = [(17, 21), (33, 50)]


# ------------------------------------------------------------------ helpers

def raw_correct(torch, who, batch, src, cmp, max_wrong, filter=None, mapping=None, stream=None, src_off_bytes=0,
                cmp_off_bytes=0):
    """The C entry point of a Plan or a PlanSet into result arrays pre-filled with garbage (the
    byte form when a mapping is given)."""
    from slime_amd import device as D
    is_set = isinstance(who, D.PlanSet)
    n = who.k + (who.max_rows if is_set else who.rows) + 1
    counts = torch.full((batch.nobj, n), GARBAGE, dtype=torch.int64, device="cuda")
    first = torch.full((batch.nobj, n), GARBAGE, dtype=torch.int64, device="cuda")
    f = ctypes.c_void_p(filter.data_ptr()) if filter is not None else None
    tail = (f, max_wrong, ctypes.c_void_p(counts.data_ptr()), ctypes.c_void_p(first.data_ptr()),
            D._stream_handle(0, stream))
    a, b = ctypes.c_void_p(src.data_ptr() + src_off_bytes), ctypes.c_void_p(cmp.data_ptr() + cmp_off_bytes)
    if mapping is None:
        call = N.lib.slime_rs_planset_correct_batch if is_set else N.lib.slime_rs_plan_correct_batch
        N.check(call(who._h, batch._h, a, b, *tail))
    else:
        call = N.lib.slime_rs_planset_correct_objects_batch if is_set else N.lib.slime_rs_correct_objects_batch
        N.check(call(who._h, batch._h, a, b, ctypes.c_void_p(mapping.data_ptr()), *tail))
    return counts, first


def lay_slots(lay, src_h, cmp_h, max_wrong):
    return CR.batch_slots(lay.coeff, lay.ins, lay.outs, src_h, lay.sp, src_h if cmp_h is None else cmp_h, lay.cp,
                          lay.lengths, max_wrong)


def wanted(lay, clean, damaged, slots, canonical_words=True):
    """(src, cmp) a correct call must leave, from the clean and the damaged host buffers (pairs
    (src, cmp), cmp None in place) and the reference's slots; objects absent from `slots` were
    passed over and keep their damage."""
    left = CR.left_columns(slots, lay.n)

    def spans(places, shards):
        return [(places[o], L, shards, True if o not in slots else left[o] if left[o].any() else None)
                for o, L in enumerate(lay.lengths) if L]
    if clean[1] is None:
        return CR.healed(clean[0], damaged[0], spans(lay.sp, lay.ins + lay.outs), canonical_words), None
    return (CR.healed(clean[0], damaged[0], spans(lay.sp, lay.ins), canonical_words),
            CR.healed(clean[1], damaged[1], spans(lay.cp, lay.outs), canonical_words))


def unlocated_total(slots, n):
    return sum(int((a == n).sum()) for a, _ in slots.values())


def same(got, want, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())


def run_ways(torch, lay, clean_s, src_h, max_wrong, clean_c=None, cmp_h=None, cleared=None, what=None, sets=True,
             byte_form=True):
    """Every way of asking: the plan and the one-plan set, symbols and bytes, without a filter, with
    the matching ragged verify's counts as the filter and -- for `cleared`, an object -- with that
    object's filter row zeroed by hand, which must stay damaged.  Each way starts from a fresh copy
    of the damaged buffers; counts, firsts and the whole buffers are compared.  Where nothing is left
    unlocated a following verify is all zero, and a second correct reports zeros and writes nothing."""
    from slime_amd import device as D
    slots = lay_slots(lay, src_h, cmp_h, max_wrong)
    nobj = len(lay.lengths)
    ms = mappings(nobj, lay.k * 131 + lay.rows)
    mt = to_dev(torch, np.array(ms, dtype=np.uint32))
    in_place = cmp_h is None

    def chunks(s, c):
        sb = to_chunks(s, lay.sp, lay.lengths, lay.nsrc, ms).view(np.uint32)
        return sb, None if c is None else to_chunks(c, lay.cp, lay.lengths, lay.ncmp, ms).view(np.uint32)
    forms = [(None, (clean_s, clean_c), (src_h, cmp_h), True)]
    if byte_form:
        forms.append((mt, chunks(clean_s, clean_c), chunks(src_h, cmp_h), False))
    variants = [("no filter", slots), ("verify's counts as the filter", slots)]
    if cleared is not None:
        assert cleared in slots and (slots[cleared][0] != CR.CLEAN).any(), "the cleared object is a damaged one"
        variants.append(("a filter row cleared by hand", {o: v for o, v in slots.items() if o != cleared}))
    for who, batch in ((lay.plan, lay.batch), (lay.pset, lay.pbatch)) if sets else ((lay.plan, lay.batch),):
        for mapping, clean, damaged, canon in forms:
            for name, vslots in variants:
                tag = (what, type(who).__name__, "symbols" if mapping is None else "bytes", name)
                want_s, want_c = wanted(lay, clean, damaged, vslots, canon)

                def up(w):
                    return to_dev(torch, w) if mapping is None else torch.from_numpy(w.view(np.uint8).copy()).cuda()

                def down(t):
                    return to_host(torch, t) if mapping is None else t.cpu().numpy().view(np.uint32)

                def verify(a, b):
                    return (who.verify_batch(a, b, batch) if mapping is None
                            else D.verify_objects_batch(who, a, b, batch, mt))
                a = up(damaged[0])
                b = a if in_place else up(damaged[1])
                filt = None
                if name != "no filter":
                    filt = verify(a, b)[0]
                    if name.startswith("a filter row"):
                        filt = filt.clone()
                        filt[cleared] = 0
                res = host(torch, raw_correct(torch, who, batch, a, b, max_wrong, filter=filt, mapping=mapping))
                assert_results(res, CR.results(vslots, nobj, lay.n + 1), tag)
                same(down(a), want_s, tag + ("src",))
                if not in_place:
                    same(down(b), want_c, tag + ("cmp",))
                if vslots is slots and unlocated_total(slots, lay.n) == 0:
                    m, f = host(torch, verify(a, b))
                    assert not m.any() and (f == -1).all(), tag + ("a following verify is all zero",)
                    again = host(torch, raw_correct(torch, who, batch, a, b, max_wrong, mapping=mapping))
                    assert_results(again, CR.results({}, nobj, lay.n + 1), tag + ("a second correct",))
                    same(down(a), want_s, tag + ("a second correct writes nothing",))
    return slots


def quick(torch, lay, clean, h, max_wrong, what=None):
    """The plan over symbols without a filter: results and the whole buffer."""
    slots = lay_slots(lay, h, None, max_wrong)
    buf = to_dev(torch, h)
    res = host(torch, raw_correct(torch, lay.plan, lay.batch, buf, buf, max_wrong))
    assert_results(res, CR.results(slots, len(lay.lengths), lay.n + 1), what)
    same(to_host(torch, buf), wanted(lay, (clean, None), (h, None), slots)[0], what)
    return slots


def canonical_case(need, total, lengths, seed):
    """(lay, clean): the encode plan in place over oracle codewords whose data is canonical, as an
    ingest stores it -- a corrected word then equals the original bit for bit, bytes included."""
    _, want, places, _ = encode_case(need, total, lengths, 1, seed=seed)
    return encode_lay(need, total, lengths, places), canonical(want, places, lengths, need)


def planted_results(lay, columns):
    """(counts, first) from planted per-column slots {object: (a array, b array)}, -1 where none."""
    return CR.results({o: (np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)) for o, (a, b) in columns.items()},
                      len(lay.lengths), lay.n + 1)


def replace_shard(h, place, s, L, rng):
    """Every word of the shard replaced by another one (different mod p as well: the distance is
    below 2^31)."""
    shard(h, place, s, L)[:] ^= rng.integers(1, 2**31, size=L, dtype=np.uint64).astype(np.uint32)


# ------------------------------------------------------------------ 1. one wrong word per object

@pytest.mark.parametrize("need,total", VECTOR_CODES + COLUMN_CODES)
def test_one_wrong_word_at_every_flip_position(torch_dev, need, total):
    """Round p plants one word at the p-th flip position of every object that has one, the shards
    taken in turn (objects of 261 columns are added until there are at least `total` words, so
    that every slot is a member): the buffers return to clean.  Two rounds run every way (plan and one-plan set,
    symbols and bytes, the three filters), the others the plan over symbols; odd rounds of plans
    with four rows take the pair rule, which answers as the one-shard rule."""
    rows, seed = total - need, need * 6007 + total
    lengths = verify_lengths(need, rows)
    while sum(len(flip_positions(L, need, rows)) for L in lengths) < total:
        lengths.append(261)
    lay, clean = canonical_case(need, total, lengths, seed)
    pos = [flip_positions(L, need, rows) for L in lengths]
    words = planted_words(seed)
    members, turn = set(), 0
    nrounds = max(len(q) for q in pos)
    for p in range(nrounds):
        h = clean.copy()
        columns = {}
        for o, (L, q) in enumerate(zip(lengths, pos)):
            if p < len(q):
                s = turn % total
                turn += 1
                plant(h, lay.sp[o], L, s, q[p], words[(3 * o + p) % len(words)], s < need)
                a = np.full(L, -1)
                a[q[p]] = s
                columns[o] = (a, np.full(L, -1))
                members.add(s)
        mw = 2 if rows >= 4 and p % 2 else 1
        slots = lay_slots(lay, h, None, mw)
        assert_results(CR.results(slots, len(lengths), total + 1), planted_results(lay, columns),
                       ("the reference names the planted slot", p))
        if p in (0, nrounds // 2):
            run_ways(torch_dev, lay, clean, h, mw, cleared=min(columns), what=("one word", p))
        else:
            quick(torch_dev, lay, clean, h, mw, what=("one word", p))
    assert members == set(range(total)), "every slot is a member"


# ------------------------------------------------------------------ 2. more wrong shards than rows

@pytest.mark.parametrize("need,total", [(3, 5), (8, 12), (17, 21)])
def test_wrong_words_in_more_shards_than_the_code_has_rows(torch_dev, need, total):
    """rows + 1 shards of an object wrong, each in a column of its own (five shards at 8/12):
    erasure repair cannot take it -- erasures_from_counts on the locate result asks for more
    erasures than the code has rows -- and column by column everything is corrected."""
    torch = torch_dev
    from slime_amd import device as D
    rows, seed = total - need, need * 6011 + total
    T, C = geometry(need)
    lengths = [T + 9, 70, C * T + T + 3, 0, 23]
    lay, clean = canonical_case(need, total, lengths, seed)
    words = planted_words(seed)
    h = clean.copy()
    columns = {}
    for o, L in enumerate(lengths):
        if L == 0:
            continue
        a = np.full(L, -1)
        for i in range(rows + 1):
            s = (2 * o + i) % total
            col = L - 1 - i * ((L - 1) // rows)  # the last column (a tail item) down to column 0
            plant(h, lay.sp[o], L, s, col, words[(o + 5 * i) % len(words)], s < need)
            a[col] = s
        columns[o] = (a, np.full(L, -1))
    for mw in (1, 2) if rows >= 4 else (1,):
        slots = lay_slots(lay, h, None, mw)
        assert_results(CR.results(slots, len(lengths), total + 1), planted_results(lay, columns),
                       "the reference names every planted word")
    buf = to_dev(torch, h)
    counts, _ = lay.plan.locate_batch(buf, buf, lay.batch)
    erasures = D.erasures_from_counts(counts, lay.plan.locate_slots())
    assert erasures == D.erasures_from_counts(CR.results(slots, len(lengths), total + 1)[0], list(range(total)))
    assert all(len(e) == rows + 1 > rows for o, e in enumerate(erasures) if lengths[o]), "beyond erasure repair"
    for mw in (1, 2) if rows >= 4 else (1,):
        run_ways(torch, lay, clean, h, mw, cleared=0, what=("spread", mw))


# ------------------------------------------------------------------ 3. a whole shard wrong

@pytest.mark.parametrize("need,total", [(3, 5), (8, 12), (16, 20), (17, 21)])
def test_a_whole_shard_wrong_in_every_column(torch_dev, need, total):
    """One shard of four objects replaced in every column -- a data shard, the last data shard, the
    first and the last parity shard -- around an undamaged object: the rare path runs on every
    lane of every step, three units of one object meet in the atomics, tail items add theirs."""
    rows, seed = total - need, need * 6029 + total
    lengths, damaged = dense_lengths(need)
    lay, clean = canonical_case(need, total, lengths, seed)
    rng = np.random.default_rng(seed)
    h = clean.copy()
    columns = {}
    for n, o in enumerate(damaged):
        s = [0, need - 1, need, total - 1][n % 4]
        replace_shard(h, lay.sp[o], s, lengths[o], rng)
        columns[o] = (np.full(lengths[o], s), np.full(lengths[o], -1))
    for mw in (1, 2) if (need, total) == (8, 12) else (1,):
        slots = lay_slots(lay, h, None, mw)
        assert_results(CR.results(slots, len(lengths), total + 1), planted_results(lay, columns),
                       "the reference names the shard in every column")
        run_ways(torch_dev, lay, clean, h, mw, cleared=damaged[0], what=("whole shard", mw))


# ------------------------------------------------------------------ 4. two whole shards wrong

@pytest.mark.parametrize("need,total", [(8, 12), (16, 20), (17, 21)])
def test_two_whole_shards_wrong_in_every_column(torch_dev, need, total):
    """max_wrong=2: input+input, input+row, row+row and input+row again, one kind per damaged
    object, in every column."""
    seed = need * 6037 + total
    lengths, damaged = dense_lengths(need)
    lay, clean = canonical_case(need, total, lengths, seed)
    rng = np.random.default_rng(seed)
    h = clean.copy()
    columns = {}
    for n, o in enumerate(damaged):
        pa = [(0, need - 1), (1, need), (need, total - 1), (need - 1, total - 2)][n % 4]
        for s in pa:
            replace_shard(h, lay.sp[o], s, lengths[o], rng)
        columns[o] = (np.full(lengths[o], pa[0]), np.full(lengths[o], pa[1]))
    slots = lay_slots(lay, h, None, 2)
    assert_results(CR.results(slots, len(lengths), total + 1), planted_results(lay, columns),
                   "the reference names both shards in every column")
    run_ways(torch_dev, lay, clean, h, 2, cleared=damaged[0], what="two whole shards")


@pytest.mark.parametrize("need,total", [(3, 12), (3, 63), (59, 63)])
def test_pairs_in_later_row_blocks_and_all_63_slots(torch_dev, need, total):
    """max_wrong=2, one pair per object on slots o % total and half the code further: every slot is
    a member, rows of later row blocks are, 3/63 asks for the 60 KiB strip and 59/63 takes the
    column form.  A second column of every other object has three wrong shards: unlocated, and
    left bit for bit."""
    rows, seed = total - need, need * 6043 + total
    lengths = boundary_objects(need, total)
    lay, clean = canonical_case(need, total, lengths, seed)
    words = planted_words(seed)
    h = clean.copy()
    columns, members, triples = {}, set(), 0
    for o, L in enumerate(lengths):
        a = o % total
        b = (a + total // 2) % total
        a, b = min(a, b), max(a, b)
        q = flip_positions(L, need, rows)
        col = q[(o + o // total) % len(q)]
        for i, s in enumerate((a, b)):
            plant(h, lay.sp[o], L, s, col, words[(o + 5 * i) % len(words)], s < need)
        ca, cb = np.full(L, -1), np.full(L, -1)
        ca[col], cb[col] = a, b
        members |= {a, b}
        if L >= 5 and o % 2 == 0:
            c3 = (col + 2) % L
            for i, s in enumerate(((a + 1) % total, (b + 1) % total, (b + 2) % total)):
                plant(h, lay.sp[o], L, s, c3, words[(o + i) % len(words)], s < need)
            ca[c3] = total
            triples += 1
        columns[o] = (ca, cb)
    assert members == set(range(total)) and triples >= 3
    slots = lay_slots(lay, h, None, 2)
    assert_results(CR.results(slots, len(lengths), total + 1), planted_results(lay, columns),
                   "the reference names every pair and leaves exactly the triples unlocated")
    run_ways(torch_dev, lay, clean, h, 2, what="slots")


# ------------------------------------------------------------------ 5. beyond the rule: unlocated, untouched

@pytest.mark.parametrize("need,total", [(8, 12), (17, 21)])
def test_more_wrong_shards_in_a_column_than_the_rule_handles(torch_dev, need, total):
    """Two wrong shards in one column under max_wrong=1 and three under max_wrong=2: those columns
    are reported unlocated and left bit for bit, while a single wrong word elsewhere in the same
    object is corrected."""
    rows, seed = total - need, need * 6047 + total
    lengths = boundary_objects(need, total)
    lay, clean = canonical_case(need, total, lengths, seed)
    words = planted_words(seed)
    for mw in (1, 2):
        h = clean.copy()
        columns = {}
        for o, L in enumerate(lengths):
            q = flip_positions(L, need, rows)
            col = q[o % len(q)]
            ca = np.full(L, -1)
            for i in range(mw + 1):
                s = (o + i * (total // 3 + 1)) % total
                plant(h, lay.sp[o], L, s, col, words[(o + 3 * i) % len(words)], s < need)
            ca[col] = total
            if L >= 3:
                other, s = (col + 1) % L, (o + 1) % total
                plant(h, lay.sp[o], L, s, other, words[(o + 11) % len(words)], s < need)
                ca[other] = s
            columns[o] = (ca, np.full(L, -1))
        slots = lay_slots(lay, h, None, mw)
        assert_results(CR.results(slots, len(lengths), total + 1), planted_results(lay, columns),
                       ("the reference leaves exactly the planted columns unlocated", mw))
        for o, (a, _) in slots.items():
            assert np.array_equal(a == total, columns[o][0] == total)
        assert unlocated_total(slots, total) == len(lengths)
        run_ways(torch_dev, lay, clean, h, mw, what=("beyond", mw))


# ------------------------------------------------------------------ 6. scrub sets

@pytest.mark.parametrize("max_wrong", [1, 2])
def test_scrub_set_with_nine_rows_down_to_one(torch_dev, max_wrong):
    """PlanSet.for_scrub(3, 12) with 0 to 9 shards missing per object -- plans of nine rows down to
    one, an object no plan can check (SLIME_RS_NO_PLAN) and an empty one -- and max_wrong present
    shards of each object wrong in every column.  max_wrong=2: objects whose plan has four rows or
    more are corrected by the pair rule; at two and three rows the long object has ONE wrong shard,
    which the one-shard rule behind the pair launch corrects (its syndrome read from the strip), and
    the short one has two, which stay unlocated and untouched; one row reports every column
    unlocated.  max_wrong=1: corrected from two rows up; nothing of a one-row object is written.
    The unchecked object is untouched."""
    torch = torch_dev
    from slime_amd import device as D
    need, total, max_rows = 3, 12, 9
    T, C = geometry(need)
    rng = np.random.default_rng(6053 + max_wrong)
    lengths, missing = [], []
    for m in range(10):
        for L in (T + 1, 5):
            lengths.append(L)
            missing.append(tuple(sorted(int(x) for x in rng.choice(total, size=m, replace=False))))
    lengths.append(0)
    missing.append(())
    nobj = len(lengths)
    _, want, places, _ = encode_case(need, total, lengths, 1, seed=6067)
    pset, plan_of, plans = scrub_set(need, total, missing)
    assert pset.max_rows == max_rows and {len(p[2]) for p in plans} == set(range(1, 10))
    assert sum(int(p) == N.NO_PLAN for p in plan_of) == 2
    batch = planned_batch(lengths, places, need, plan_of, pset.nplans)
    clean = canonical(want, places, lengths, need)
    blank(clean, places, lengths, missing)
    h = clean.copy()
    ec, ef = CR.results({}, nobj, need + max_rows + 1)
    healed_objects, shards_of, one_shard_under_pairs = set(), {}, 0
    for o, L in enumerate(lengths):
        if L == 0:
            continue
        if int(plan_of[o]) == N.NO_PLAN:  # damaged all the same: it must stay
            replace_shard(h, places[o], [s for s in range(total) if s not in missing[o]][0], L, rng)
            continue
        coeff, have, checked = plans[int(plan_of[o])]
        shards_of[o] = have + checked
        nwrong = 1 if max_wrong == 2 and 2 <= len(checked) < 4 and L > 5 else max_wrong
        hit = [int(x) for x in rng.choice(len(shards_of[o]), size=nwrong, replace=False)]
        for sl in hit:
            replace_shard(h, places[o], shards_of[o][sl], L, rng)
        if len(checked) >= (4 if nwrong == 2 else 2):
            healed_objects.add(o)
            one_shard_under_pairs += max_wrong == 2 and len(checked) < 4
            for sl in hit:
                ec[o, sl], ef[o, sl] = L, 0
        else:
            ec[o, need + max_rows], ef[o, need + max_rows] = L, 0
    slots = CR.set_batch_slots(plans, plan_of, max_rows, h, places, lengths, N.NO_PLAN, max_wrong)
    assert_results(CR.results(slots, nobj, need + max_rows + 1), (ec, ef),
                   "the reference: named where the object's rows decide it, unlocated below")
    assert healed_objects and len(healed_objects) < len(shards_of)
    assert one_shard_under_pairs == (2 if max_wrong == 2 else 0), "a two-row and a three-row object under the pair launch"
    spans = [(places[o], L, shards_of[o] if o in shards_of else list(range(total)), None if o in healed_objects else True)
             for o, L in enumerate(lengths) if L]
    ms = mappings(nobj, 6073)
    mt = to_dev(torch, np.array(ms, dtype=np.uint32))
    for mapping in (None, mt):
        if mapping is None:
            d, want_h = h, CR.healed(clean, h, spans)
            buf = to_dev(torch, d)
        else:
            d = to_chunks(h, places, lengths, total, ms).view(np.uint32)
            want_h = CR.healed(to_chunks(clean, places, lengths, total, ms).view(np.uint32), d, spans, canonical=False)
            buf = torch.from_numpy(d.view(np.uint8).copy()).cuda()
        for filtered in (False, True):
            if mapping is None:
                buf.copy_(to_dev(torch, d))
                filt = pset.verify_batch(buf, buf, batch)[0] if filtered else None
            else:
                buf.copy_(torch.from_numpy(d.view(np.uint8).copy()).cuda())
                filt = D.verify_objects_batch(pset, buf, buf, batch, mt)[0] if filtered else None
            res = host(torch, raw_correct(torch, pset, batch, buf, buf, max_wrong, filter=filt, mapping=mapping))
            assert_results(res, (ec, ef), (mapping is None, filtered))
            got = to_host(torch, buf) if mapping is None else buf.cpu().numpy().view(np.uint32)
            same(got, want_h, (mapping is None, filtered))
    buf = to_dev(torch, h)
    assert_results(host(torch, pset.correct_batch(buf, buf, batch, max_wrong=max_wrong)), (ec, ef), "PlanSet.correct_batch")
    same(to_host(torch, buf), CR.healed(clean, h, spans), "PlanSet.correct_batch")
    bbuf = torch.from_numpy(to_chunks(h, places, lengths, total, ms).copy()).cuda()
    assert_results(host(torch, D.correct_objects_batch(pset, bbuf, bbuf, batch, mt, max_wrong=max_wrong)), (ec, ef), "bytes")


# ------------------------------------------------------------------ 7. addressing and modes

@pytest.mark.parametrize("need,total", [(8, 12), (17, 21)])
def test_separate_cmp_tensor_with_its_own_offsets(torch_dev, need, total):
    """src holds the data shards, cmp is another tensor with the parity rows only, objects in
    reverse order, odd shard strides: a wrong input is rewritten in src, a wrong row in cmp (one of
    each per object, in different columns; then both in one column under the pair rule), also
    through the wrappers' offsets behind a few words of padding."""
    torch = torch_dev
    from slime_amd import device as D
    rows = total - need
    T, C = geometry(need)
    lengths = [T + 1, 0, 3, C * T + 5, 257, 4]
    nobj = len(lengths)
    _, want, sp, _ = encode_case(need, total, lengths, 1, seed=need * 6079 + total)
    want = canonical(want, sp, lengths, need)
    cp, off = [None] * nobj, 9
    for o in reversed(range(nobj)):
        ss = -(-lengths[o] // 8) * 8 + 1
        cp[o] = (off, ss)
        off += rows * ss + 3
    clean_c = np.full(off + 4, SENTINEL, dtype=np.uint32)
    clean_s = want.copy()
    for o, L in enumerate(lengths):
        for i in range(rows):
            shard(clean_c, cp[o], i, L)[:] = shard(want, sp[o], need + i, L)
            shard(clean_s, sp[o], need + i, L)[:] = SENTINEL
    plan = D.Plan.encode(need, total)  # outputs 0..rows-1
    lay = Lay(plan, OC.parity_matrix(need, rows)[need:], range(need), range(rows), lengths, sp, cp, nsrc=total, ncmp=rows)
    for mw in (1, 2):
        src_h, cmp_h = clean_s.copy(), clean_c.copy()
        columns = {}
        for o, L in enumerate(lengths):
            if L == 0:
                continue
            j, i, col = o % need, (o + 1) % rows, L - 1 if o % 2 else L // 2
            rcol = col if mw == 2 else (col + 1) % L
            plant(src_h, sp[o], L, j, col, 0x1234 + o, True)
            plant(cmp_h, cp[o], L, i, rcol, P + o % 5, False)
            ca, cb = np.full(L, -1), np.full(L, -1)
            if mw == 2:
                ca[col], cb[col] = j, need + i
            else:
                ca[col], ca[rcol] = j, need + i
            columns[o] = (ca, cb)
        slots = lay_slots(lay, src_h, cmp_h, mw)
        assert_results(CR.results(slots, nobj, total + 1), planted_results(lay, columns),
                       "the reference names the input in src and the row in cmp")
        run_ways(torch, lay, clean_s, src_h, mw, clean_c=clean_c, cmp_h=cmp_h, cleared=0, what=("separate", mw))

        def padded(a, n):
            return to_dev(torch, np.concatenate([np.full(n, SENTINEL, dtype=np.uint32), a]))
        s, c = padded(src_h, 5), padded(cmp_h, 11)
        mism, _ = plan.verify_batch(s, c, lay.batch, src_offset=5, cmp_offset=11)
        res = plan.correct_batch(s, c, lay.batch, filter=mism, src_offset=5, cmp_offset=11, max_wrong=mw)
        assert_results(host(torch, res), CR.results(slots, nobj, total + 1), "Plan.correct_batch with offsets")
        got_s, got_c = to_host(torch, s), to_host(torch, c)
        assert (got_s[:5] == SENTINEL).all() and (got_c[:11] == SENTINEL).all()
        same(got_s[5:], clean_s, "src behind its padding")
        same(got_c[11:], clean_c, "cmp behind its padding")


@pytest.mark.parametrize("need,total,have,want", PERMUTED[1:])
def test_permuted_plan_rewrites_the_shard_behind_each_slot(torch_dev, need, total, have, want):
    """Plan.reconstruct with shuffled survivors and every other shard as a checked output, in place:
    object o has one wrong word in shard o -- slot (have + want).index(o) -- and it is that shard's
    word that is rewritten."""
    T, C = geometry(need)
    base = [T + 1, 5, 257, C * T + 1, 3, T, 4]
    lengths = [base[o % len(base)] for o in range(total)]
    _, codeword, places, _ = encode_case(need, total, lengths, 1, seed=need * 6089 + total)
    lay = permuted_lay(need, total, have, want, lengths, places)
    clean = canonical(codeword, places, lengths, need)
    words = planted_words(need * 6089 + total)
    h = clean.copy()
    columns = {}
    for o, L in enumerate(lengths):
        q = flip_positions(L, need, len(want))
        col = q[o % len(q)]
        # every shard is compared bit for bit with what the survivors rebuild: any other word is wrong
        plant(h, places[o], L, o, col, words[o % len(words)], o < need)
        ca = np.full(L, -1)
        ca[col] = (have + want).index(o)
        columns[o] = (ca, np.full(L, -1))
    slots = lay_slots(lay, h, None, 1)
    assert_results(CR.results(slots, total, total + 1), planted_results(lay, columns), "the reference names shard o's slot")
    run_ways(torch_dev, lay, clean, h, 1, cleared=1, what="permuted")


def test_non_canonical_originals_come_back_as_their_residues(torch_dev):
    """Symbol form over codewords whose data holds p, p + 1, p + 4 and 0xFFFFFFFF: those words are
    damaged, and come back as their canonical residues; untouched aliases stay bit for bit."""
    need, total = 8, 12
    lengths = verify_lengths(need, total - need)[:12] + [5, 300]
    _, raw, places, _ = encode_case(need, total, lengths, 1, seed=6091)
    lay = encode_lay(need, total, lengths, places)
    h = raw.copy()
    hit = kept = 0
    for o, L in enumerate(lengths):
        taken = set()
        for s in range(need):
            w = shard(h, places[o], s, L)
            for col in np.flatnonzero(shard(raw, places[o], s, L) >= P):
                if int(col) in taken or (o + s) % 3 == 0:  # one wrong shard a column; some aliases stay
                    kept += 1
                    continue
                taken.add(int(col))
                w[col] = (int(w[col]) % P + 1 + 7 * o) % P
                hit += 1
    assert hit >= 10 and kept >= 3
    slots = lay_slots(lay, h, None, 1)
    assert unlocated_total(slots, total) == 0 and sum(int((a != CR.CLEAN).sum()) for a, _ in slots.values()) == hit
    quick(torch_dev, lay, raw, h, 1, "aliases")
    want = wanted(lay, (raw, None), (h, None), slots)[0]
    assert int(((raw >= P) & (want < P) & (raw != SENTINEL)).sum()) == hit
    assert int(((want >= P) & (want != SENTINEL)).sum()) >= kept


def test_every_schedule_and_pipeline_mode_corrects_the_same(torch_dev, mode):
    need, total = 8, 12
    lengths, damaged = dense_lengths(need)
    lay, clean = canonical_case(need, total, lengths, 6101)
    rng = np.random.default_rng(6101)
    h = clean.copy()
    for n, o in enumerate(damaged):
        for s in [(0, need), (3, 5), (need, total - 1), (need - 1, total - 2)][n % 4]:
            replace_shard(h, lay.sp[o], s, lengths[o], rng)
    slots = quick(torch_dev, lay, clean, h, 2, mode)
    assert unlocated_total(slots, total) == 0
    assert sum(int((b != CR.NONE).sum()) for _, b in slots.values()) == sum(lengths[o] for o in damaged)


# ------------------------------------------------------------------ 8. a captured chain

@pytest.mark.parametrize("need,total", [(8, 12), (17, 21)])
def test_captured_verify_and_correct_replays(torch_dev, need, total):
    """verify_batch then correct_batch with its counts as the filter, captured as one graph on a
    non-default stream: replayed on two different damages, both heal; a third replay, on the data
    the second left, reports zeros."""
    torch = torch_dev
    lengths, damaged = dense_lengths(need)
    lay, clean = canonical_case(need, total, lengths, need * 6113 + total)
    plan, batch = lay.plan, lay.batch
    buf = to_dev(torch, clean)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm the launch paths outside the capture, on the stream itself
        m0, _ = plan.verify_batch(buf, buf, batch, stream=s)
        res = raw_correct(torch, plan, batch, buf, buf, 2, filter=m0, stream=s)
    s.synchronize()
    zeros = CR.results({}, len(lengths), total + 1)
    assert_results(host(torch, res), zeros)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        gm, _ = plan.verify_batch(buf, buf, batch, stream=s)
        gc, gf_ = plan.correct_batch(buf, buf, batch, filter=gm, stream=s, max_wrong=2)
    torch.cuda.synchronize()
    rng = np.random.default_rng(need * 6113 + total)
    for rnd in range(2):
        h = clean.copy()
        for n, o in enumerate(damaged[rnd:]):
            for sh in [(0, need), (need - 1,), (need, total - 1), (1, 2)][(n + rnd) % 4]:
                replace_shard(h, lay.sp[o], sh, lengths[o], rng)
        slots = lay_slots(lay, h, None, 2)
        assert unlocated_total(slots, total) == 0 and len([o for o, (a, _) in slots.items() if (a != CR.CLEAN).all()]) == len(damaged) - rnd
        buf.copy_(to_dev(torch, h))
        gc.fill_(GARBAGE)
        gf_.fill_(GARBAGE)
        torch.cuda.synchronize()
        g.replay()
        assert_results(host(torch, (gc, gf_)), CR.results(slots, len(lengths), total + 1), rnd)
        same(to_host(torch, buf), clean, ("healed", rnd))
    g.replay()
    assert_results(host(torch, (gc, gf_)), zeros, "a replay on clean data")
    same(to_host(torch, buf), clean, "a replay on clean data")
    del g  # before the batch: the graph's kernel nodes read its tables
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 9. refusals

def test_refusals(torch_dev):
    torch = torch_dev
    from slime_amd import device as D
    buf = to_dev(torch, np.zeros(4096, dtype=np.uint32))
    res = torch.full((2 * 70,), GARBAGE, dtype=torch.int64, device="cuda")
    p, r = ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(res.data_ptr())
    sym, byt = N.lib.slime_rs_plan_correct_batch, N.lib.slime_rs_correct_objects_batch
    ssym, sbyt = N.lib.slime_rs_planset_correct_batch, N.lib.slime_rs_planset_correct_objects_batch

    def refused(fn, args, text):
        assert fn(*args, None) == N.ERR_INVALID_ARG
        assert N.lib.slime_rs_last_error().decode() == text

    four, b8 = D.Plan.encode(8, 12).set_outputs([8, 9, 10, 11]), D.Batch([(0, 16, 0, 16, 16)], 8)
    three, b4 = D.Plan.encode(4, 7), D.Batch([(0, 16, 0, 16, 16)], 4)
    one, b3 = D.Plan.encode(3, 4), D.Batch([(0, 16, 0, 16, 16)], 3)
    text = "max_wrong = 3 is neither 1 (one wrong shard per column) nor 2 (a pair)"
    refused(sym, (four._h, b8._h, p, p, None, 3, r, r), "plan_correct_batch: " + text)
    refused(byt, (four._h, b8._h, p, p, p, None, 3, r, r), "correct_objects_batch: " + text)
    refused(sym, (None, None, None, None, None, 3, None, None), "plan_correct_batch: " + text)  # the first check
    refused(sym, (None, b8._h, p, p, None, 1, r, r), "plan_correct_batch: null plan")
    text = "the plan has 3 rows: two wrong shards in a column take four rows to name"
    refused(sym, (three._h, b4._h, p, p, None, 2, r, r), "plan_correct_batch: " + text)
    refused(byt, (three._h, b4._h, p, p, p, None, 2, r, r), "correct_objects_batch: " + text)
    refused(sym, (three._h, b4._h, None, None, None, 2, None, None), "plan_correct_batch: " + text)  # before the nulls
    refused(sym, (one._h, b3._h, p, p, None, 1, r, r),
            "plan_correct_batch: the plan has 1 row: one parity row cannot tell which shard is wrong")
    set3, pb4 = D.PlanSet([three]), D.Batch([(0, 16, 0, 16, 16)], 4, plans=np.zeros(1, dtype=np.uint32), nplans=1)
    text = "no plan of the set has more than 3 rows: two wrong shards in a column take four rows to name"
    refused(ssym, (set3._h, pb4._h, p, p, None, 2, r, r), "planset_correct_batch: " + text)
    refused(sbyt, (set3._h, pb4._h, p, p, p, None, 2, r, r), "planset_correct_objects_batch: " + text)
    refused(ssym, (set3._h, b4._h, p, p, None, 1, r, r),
            "planset_correct_batch: the batch carries no plan indices (create it with slime_rs_batch_create_planned)")
    wide, b40 = D.Plan.encode(40, 64), D.Batch([(0, 1, 0, 1, 1)], 40)
    text = "k + rows = 64 exceeds 63 (a wave's tally keeps one slot per lane)"
    refused(sym, (wide._h, b40._h, p, p, None, 1, r, r), "plan_correct_batch: " + text)
    refused(byt, (wide._h, b40._h, p, p, p, None, 2, r, r), "correct_objects_batch: " + text)
    w = "plan_correct_batch: "
    refused(sym, (four._h, b8._h, p, p, None, 1, None, r), w + "null result array")
    refused(sym, (four._h, b8._h, None, p, None, 2, r, r), w + "null buffer")
    refused(byt, (four._h, b8._h, p, p, None, None, 1, r, r), "correct_objects_batch: null mapping")
    refused(sym, (four._h, b4._h, p, p, None, 1, r, r), w + "the batch was created for k = 4 on device 0, "
                                                            "the plan has k = 8 on device 0")
    with pytest.raises(N.NativeError, match="take four rows"):
        three.correct_batch(buf, buf, b4, max_wrong=2)
    with pytest.raises(ValueError, match="max_wrong"):
        four.correct_batch(buf, buf, b8, max_wrong=3)
    torch.cuda.synchronize()
    assert (res == GARBAGE).all() and not to_host(torch, buf).any(), "a refused call touches nothing"
    four.set_outputs([8, 9, 10, 11])  # refusals do not mark the plan
    zeros = CR.results({}, 1, 13)
    assert_results(host(torch, four.correct_batch(buf, buf, b8, max_wrong=2)), zeros)  # zeros are a codeword
    assert not to_host(torch, buf).any()
    with pytest.raises(N.NativeError, match="already launched"):
        four.set_outputs([0, 1, 2, 3])
    none = D.Batch([], 8)
    assert sym(four._h, none._h, p, p, None, 1, r, r, None) == 0  # nobj == 0 touches nothing
    torch.cuda.synchronize()
    assert (res == GARBAGE).all()
    c, f = four.correct_batch(buf, buf, none, max_wrong=2)
    assert c.shape == f.shape == (0, 13)
    c, f = D.correct_objects_batch(four, buf.view(torch.uint8), buf.view(torch.uint8), none,
                                   to_dev(torch, np.zeros(1, dtype=np.uint32)))
    assert c.shape == f.shape == (0, 13)
