"""Pair locate (slime_rs_plan_locate_pairs_batch, slime_rs_locate_pairs_objects_batch and their
plan-set twins) on the GPU: the locate launches with the pair rule behind them, which name two
wrong shards of a column where the one-shard calls say unlocated.

Every expectation comes from tests/locate_pairs_ref.py on host copies (the rule as the header
states it, over oracle_c.apply_matrix rows; pinned to the C++ rule by test_locate_pairs_host.py),
never from a kernel -- the one exception is the case that asks for equality with the one-shard
calls, which is compared with both.  Result arrays are pre-filled with garbage, data buffers are
compared with their host copies afterwards, and before any comparison with the GPU each case
asserts that the reference alone names what was planted.  Shapes are the locate tests' boundary
lengths (a vector, a wave, a tile, a unit, verify's step boundaries), not workloads.
"""
import ctypes

import numpy as np
import pytest

import locate_pairs_ref as PR
import locate_ref as R
from oracle import oracle_c as OC
from slime_amd import _native as N
from test_gpu_locate import one_word_rounds, plant, planted_words, raw_locate, to_chunks
from test_gpu_locate_paths import boundary_objects, dense_lengths, mappings
from test_gpu_planset_locate import blank, planned_batch, raw_set_locate, scrub_set
from test_gpu_ragged import P, SENTINEL, encode_case, encode_plan, geometry, mode, shard, to_dev, to_host, torch_dev  # noqa: F401
from test_gpu_ragged_verify import assert_results, flip_positions, host, step_rule, verify_lengths
from test_gpu_verify import GARBAGE

pytestmark = pytest.mark.gpu

VECTOR_CODES = [(3, 7), (8, 12), (10, 14), (16, 20)]
COLUMN_CODES = [(17, 21), (33, 50)]


# ------------------------------------------------------------------ helpers

def raw_pairs(torch, who, batch, src, cmp, filter=None, mapping=None, stream=None, src_off_bytes=0, cmp_off_bytes=0):
    """The pair C entry point of a Plan or a PlanSet into result arrays pre-filled with garbage
    (the byte form when a mapping is given)."""
    from slime_amd import device as D
    is_set = isinstance(who, D.PlanSet)
    n = who.k + (who.max_rows if is_set else who.rows) + 1
    counts = torch.full((batch.nobj, n), GARBAGE, dtype=torch.int64, device="cuda")
    first = torch.full((batch.nobj, n), GARBAGE, dtype=torch.int64, device="cuda")
    f = ctypes.c_void_p(filter.data_ptr()) if filter is not None else None
    tail = (f, ctypes.c_void_p(counts.data_ptr()), ctypes.c_void_p(first.data_ptr()), D._stream_handle(0, stream))
    a, b = ctypes.c_void_p(src.data_ptr() + src_off_bytes), ctypes.c_void_p(cmp.data_ptr() + cmp_off_bytes)
    if mapping is None:
        call = N.lib.slime_rs_planset_locate_pairs_batch if is_set else N.lib.slime_rs_plan_locate_pairs_batch
        N.check(call(who._h, batch._h, a, b, *tail))
    else:
        call = (N.lib.slime_rs_planset_locate_pairs_objects_batch if is_set
                else N.lib.slime_rs_locate_pairs_objects_batch)
        N.check(call(who._h, batch._h, a, b, ctypes.c_void_p(mapping.data_ptr()), *tail))
    return counts, first


class Case:
    """The encode plan of need/total in place over a packed layout: what the references need on the
    host, and (gpu()) the plan, a one-plan PlanSet and the two batches."""

    def __init__(self, need, total, lengths, seed):
        self.k, self.rows, self.n = need, total - need, total
        self.lengths = list(lengths)
        _, self.clean, self.places, _ = encode_case(need, total, self.lengths, 1, seed=seed)
        self.coeff = OC.parity_matrix(need, total - need)[need:]
        self.ins, self.outs = list(range(need)), list(range(need, total))
        self._gpu = None

    def reference(self, h, skip=()):
        return PR.locate_batch(self.coeff, self.ins, self.outs, h, self.places, h, self.places, self.lengths, skip)

    def one_shard_reference(self, h, skip=()):
        return R.locate_batch(self.coeff, self.ins, self.outs, h, self.places, h, self.places, self.lengths, skip)

    def gpu(self):
        from slime_amd import device as D
        if self._gpu is None:
            plan = encode_plan(self.k, self.n)
            spans = [(off, ss, off, ss, L) for (off, ss), L in zip(self.places, self.lengths)]
            batch = D.Batch(spans, self.k)
            pbatch = D.Batch(spans, self.k, plans=np.zeros(len(spans), dtype=np.uint32), nplans=1)
            self._gpu = plan, batch, D.PlanSet([plan]), pbatch
        return self._gpu


def planted_results(case, columns):
    """(counts, first) from planted per-column slots {object: (a array, b array)}, -1 where none."""
    ec, ef = PR.clean_results(len(case.lengths), case.n, 0)
    for o, (a, b) in columns.items():
        ec[o], ef[o] = PR.tally((np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)), case.n + 1)
    return ec, ef


def run_ways(torch, case, h, exp, cleared=None, what=None, sets=True, byte_form=True):
    """Every way of asking the pair calls: the plan and the one-plan set, symbols and bytes, without
    a filter, with the matching ragged verify's counts as the filter and -- for `cleared`, an
    object -- with that object's filter row zeroed by hand.  The buffers must come back unchanged."""
    from slime_amd import device as D
    plan, batch, pset, pbatch = case.gpu()
    exp_cleared = None if cleared is None else case.reference(h, skip=(cleared,))
    ms = mappings(len(case.lengths), case.k * 131 + case.rows)
    mt = to_dev(torch, np.array(ms, dtype=np.uint32))
    s = to_dev(torch, h)
    sb_h = to_chunks(h, case.places, case.lengths, case.n, ms)
    sb = torch.from_numpy(sb_h.copy()).cuda()
    for who, b in ((plan, batch), (pset, pbatch)) if sets else ((plan, batch),):
        for mapping, a in ((None, s), (mt, sb)) if byte_form else ((None, s),):
            tag = (what, type(who).__name__, "symbols" if mapping is None else "bytes")
            mism, _ = who.verify_batch(a, a, b) if mapping is None else D.verify_objects_batch(who, a, a, b, mt)
            assert_results(host(torch, raw_pairs(torch, who, b, a, a, mapping=mapping)), exp, tag + ("no filter",))
            assert_results(host(torch, raw_pairs(torch, who, b, a, a, mapping=mapping, filter=mism)), exp,
                           tag + ("verify's counts as the filter",))
            if cleared is not None:
                hand = mism.clone()
                hand[cleared] = 0
                assert_results(host(torch, raw_pairs(torch, who, b, a, a, mapping=mapping, filter=hand)), exp_cleared,
                               tag + ("a filter row cleared by hand",))
    assert np.array_equal(to_host(torch, s), h) and np.array_equal(sb.cpu().numpy(), sb_h), "locate writes only results"


def kind_of(case, a, b):
    return ("input" if a < case.k else "row") + "+" + ("input" if b < case.k else "row")


def replace_shard(h, case, o, s, rng):
    """Every word of shard s of object o replaced by another one (different mod p as well: the
    distance is below 2^31)."""
    w = shard(h, case.places[o], s, case.lengths[o])
    w[:] ^= rng.integers(1, 2**31, size=len(w), dtype=np.uint64).astype(np.uint32)


# ------------------------------------------------------------------ 1. equality with the one-shard calls

@pytest.mark.parametrize("need,total", VECTOR_CODES + COLUMN_CODES)
def test_clean_and_one_wrong_word_equal_the_one_shard_calls(torch_dev, need, total):
    """Clean data and one wrong word per object (column 0, the last whole vector, the last flip
    position) through the pair calls: exactly the one-shard calls' results, which are the one-shard
    reference's -- over symbols and bytes, as plan and as one-plan set."""
    torch = torch_dev
    from slime_amd import device as D
    rows = total - need
    lengths, places, rounds = one_word_rounds(need, total, seed=need * 5003 + total)
    plan = encode_plan(need, total)
    spans = [(off, ss, off, ss, L) for (off, ss), L in zip(places, lengths)]
    batch = D.Batch(spans, need)
    pbatch = D.Batch(spans, need, plans=np.zeros(len(spans), dtype=np.uint32), nplans=1)
    pset = D.PlanSet([plan])
    coeff = OC.parity_matrix(need, rows)[need:]
    ms = mappings(len(lengths), need * 7 + total)
    mt = to_dev(torch, np.array(ms, dtype=np.uint32))
    _, clean, _, _ = encode_case(need, total, lengths, 1, seed=need * 5003 + total)
    data = [(clean, R.clean_results(len(lengths), need, rows))] + [rounds[p] for p in (0, 1, len(rounds) - 1)]
    for n, (h, planted) in enumerate(data):
        exp = R.locate_batch(coeff, list(range(need)), list(range(need, total)), h, places, h, places, lengths)
        assert_results(exp, planted, ("the one-shard reference names the planted slot", n))
        assert_results(PR.locate_batch(coeff, list(range(need)), list(range(need, total)), h, places, h, places, lengths),
                       exp, ("the pair reference says the same", n))
        buf = to_dev(torch, h)
        hb = to_chunks(h, places, lengths, total, ms)
        bbuf = torch.from_numpy(hb.copy()).cuda()
        for who, b, one in ((plan, batch, raw_locate), (pset, pbatch, raw_set_locate)):
            for mapping, a in ((None, buf), (mt, bbuf)):
                tag = (n, type(who).__name__, mapping is None)
                single = host(torch, one(torch, who, b, a, a, mapping=mapping))
                assert_results(single, exp, tag + ("one-shard call",))
                assert_results(host(torch, raw_pairs(torch, who, b, a, a, mapping=mapping)), single, tag + ("pair call",))
        assert_results(host(torch, plan.locate_batch(buf, buf, batch, max_wrong=2)), exp, "Plan.locate_batch")
        assert_results(host(torch, pset.locate_batch(buf, buf, pbatch, max_wrong=2)), exp, "PlanSet.locate_batch")
        assert_results(host(torch, D.locate_objects_batch(plan, bbuf, bbuf, batch, mt, max_wrong=2)), exp, "bytes")
        assert_results(host(torch, D.locate_objects_batch(pset, bbuf, bbuf, pbatch, mt, max_wrong=2)), exp, "bytes, set")
        assert np.array_equal(to_host(torch, buf), h) and np.array_equal(bbuf.cpu().numpy(), hb)


# ------------------------------------------------------------------ 2. one pair per object

def pair_rounds(case, seed):
    """Round p plants, in every object that has a p-th flip position, two wrong words in that
    column, in a pair of slots that rotates over input+input, input+row and row+row with o + p.  The words cycle EDGES (non-canonical stored rows among them) and random values;
    plant() steps past data-shard aliases.  [(host buffer, planted per-column slots)]."""
    pos = [flip_positions(L, case.k, case.rows) for L in case.lengths]
    words = planted_words(seed)
    out, drawn = [], [0, 0, 0]
    for p in range(max(len(q) for q in pos)):
        h = case.clean.copy()
        columns = {}
        for o, (L, q) in enumerate(zip(case.lengths, pos)):
            if p >= len(q):
                continue
            k, rows, kind = case.k, case.rows, (o + p) % 3
            c = drawn[kind]  # the kind's own counter: inputs are swept from both ends, rows in turn
            drawn[kind] += 1
            if kind == 0:  # input + input
                a = c % k
                b = (a + 1 + (c // k) % (k - 1)) % k
            elif kind == 1:  # input + row
                a, b = k - 1 - c % k, k + c % rows
            else:  # row + row
                a = k + c % rows
                b = k + (c % rows + 1 + (c // rows) % (rows - 1)) % rows
            a, b = min(a, b), max(a, b)
            for i, s in enumerate((a, b)):
                plant(h, case.places[o], L, s, q[p], words[(3 * o + p + 7 * i) % len(words)], s < case.k)
            ca, cb = np.full(L, -1), np.full(L, -1)
            ca[q[p]], cb[q[p]] = a, b
            columns[o] = (ca, cb)
        out.append((h, columns))
    return out


@pytest.mark.parametrize("need,total", VECTOR_CODES + [(17, 21)])
def test_one_pair_per_object_at_every_flip_position(torch_dev, need, total):
    torch = torch_dev
    case = Case(need, total, verify_lengths(need, total - need), seed=need * 5009 + total)
    rounds = pair_rounds(case, need * 5009 + total)
    members, kinds = set(), set()
    plan, batch, _, _ = case.gpu()
    buf = to_dev(torch, rounds[0][0])
    for p, (h, columns) in enumerate(rounds):
        for a, b in columns.values():
            pa, pb = int(a.max()), int(b.max())
            members |= {pa, pb}
            kinds.add(kind_of(case, pa, pb))
        exp = case.reference(h)
        assert_results(exp, planted_results(case, columns), ("the reference names both planted slots", p))
        assert (exp[0][:, case.n] == 0).all()
        if p in (0, len(rounds) // 2):
            run_ways(torch, case, h, exp, what=("pair", p))
        else:
            buf.copy_(to_dev(torch, h))
            assert_results(host(torch, raw_pairs(torch, plan, batch, buf, buf)), exp, p)
            assert np.array_equal(to_host(torch, buf), h)
    assert members == set(range(case.n)), "every slot is a member of some pair"
    assert kinds == {"input+input", "input+row", "row+row"}


# ------------------------------------------------------------------ 3. two whole shards wrong

def whole_shard_damage(case, damaged, variant, seed):
    """same: shards a_o and b_o of object o replaced in every column.  rotating: every column has
    two wrong words in a pair of its own.  third: `same`, and a third wrong shard in about 2% of
    the columns.  Returns (host buffer, planted per-column slots, columns with a third)."""
    rng = np.random.default_rng(seed)
    h = case.clean.copy()
    words = planted_words(seed)
    columns, thirds = {}, {}
    for n, o in enumerate(damaged):
        L = case.lengths[o]
        if variant == "rotating":
            a = rng.integers(0, case.n, size=L)
            b = (a + rng.integers(1, case.n, size=L)) % case.n
            a, b = np.minimum(a, b), np.maximum(a, b)
            for col in range(L):
                for i, s in enumerate((int(a[col]), int(b[col]))):
                    plant(h, case.places[o], L, s, col, words[(col + 3 * i + o) % len(words)], s < case.k)
        else:
            pa = [(0, case.k - 1), (1 % case.k, case.k), (case.k, case.n - 1), (case.k - 1, case.n - 2)][n % 4]
            for s in pa:
                replace_shard(h, case, o, s, rng)
            a, b = np.full(L, min(pa)), np.full(L, max(pa))
            if variant == "third":
                hit = np.flatnonzero(rng.random(L) < 0.02)
                if L > 100 and not hit.size:
                    hit = np.array([L // 2])
                others = [s for s in range(case.n) if s not in pa]
                for col in hit:
                    s = others[int(rng.integers(0, len(others)))]
                    plant(h, case.places[o], L, s, int(col), words[int(col) % len(words)], s < case.k)
                thirds[o] = hit
        columns[o] = (a, b)
    return h, columns, thirds


@pytest.mark.parametrize("variant", ["same", "rotating", "third"])
@pytest.mark.parametrize("need,total", [(3, 7), (8, 12), (16, 20), (17, 21)])
def test_two_whole_shards_wrong_in_every_column(torch_dev, need, total, variant):
    """Objects of 2 C T + T + 7, T + 1, 6, 3 and 0 columns around an undamaged one: three units of
    one object meet in the atomics, a wave's fold meets many slots (rotating), tail items add
    theirs.  17/21 takes the column form."""
    lengths, damaged = dense_lengths(need)
    case = Case(need, total, lengths, seed=need * 5011 + total)
    h, columns, thirds = whole_shard_damage(case, damaged, variant, need * 5021 + total)
    exp = case.reference(h)
    for o in range(len(lengths)):
        if o not in damaged:
            assert exp[0][o].sum() == 0 and (exp[1][o] == -1).all(), ("undamaged", o)
    if variant != "third":
        assert_results(exp, planted_results(case, columns), "the reference names both shards in every column")
        assert (exp[0][:, case.n] == 0).all()
    else:
        o = damaged[0]
        assert len(thirds[o]) >= 1 and exp[0][o, case.n] >= 1, "the reference leaves three-shard columns unlocated"
        assert exp[0][o, case.n] <= len(thirds[o])
        a, b = int(columns[o][0][0]), int(columns[o][1][0])
        assert exp[0][o, a] >= lengths[o] - len(thirds[o]) and exp[0][o, b] >= lengths[o] - len(thirds[o])
    run_ways(torch_dev, case, h, exp, cleared=damaged[0], what=variant)


# ------------------------------------------------------------------ 4. the order of `first`

@pytest.mark.parametrize("need,total", [(3, 7), (8, 12)])
def test_first_of_both_slots_is_the_lowest_column(torch_dev, need, total):
    """Two columns per slot pair, met by the rare path in either order (test_gpu_locate_paths, B:
    higher column first, lower first, two units of one step, the last column of a tile and the
    first of the next, a vector and a tail item's atomic)."""
    T, _ = geometry(need)
    assert step_rule(need, total - need)[0] >= 512
    L = 2 * T + 3
    spots = [(41, 44), (80, 85), (39, 276), (T - 1, T), (2, 2 * T + 1)]
    case = Case(need, total, [L] * total, seed=need * 5023 + total)
    h = case.clean.copy()
    words = planted_words(need * 5023 + total)
    columns = {}
    for o in range(total):
        ca, cb = np.full(L, -1), np.full(L, -1)
        for p, (lo, hi) in enumerate(spots):
            a = (2 * p + o) % total
            b = (a + 1 + o % (total - 1)) % total
            a, b = min(a, b), max(a, b)
            for col in (hi, lo):
                for i, s in enumerate((a, b)):
                    plant(h, case.places[o], L, s, col, words[(5 * o + p + col + i) % len(words)], s < need)
                ca[col], cb[col] = a, b
        columns[o] = (ca, cb)
    exp = case.reference(h)
    want = planted_results(case, columns)
    assert_results(exp, want, "the reference: both slots of every pair, the lower column first")
    assert (want[0].sum(axis=1) == 4 * len(spots)).all()
    run_ways(torch_dev, case, h, exp, what="first")


# ------------------------------------------------------------------ 5. row blocks and slot limits

@pytest.mark.parametrize("need,total", [(3, 12), (3, 63), (59, 63)])
def test_row_blocks_and_all_63_slots(torch_dev, need, total):
    """One pair per object, object o on slots o % total and half the code further: every slot is a
    member, rows of later row blocks and of the clipped last block are, and some pair's rows sit in
    different row blocks.  A second column of the longer objects has three wrong shards:
    `unlocated`, lane 63 of the wave's tally at 63 slots.  3/63 asks for the largest LDS strip
    (60 rows); 59/63 takes the column form."""
    rows = total - need
    lengths = boundary_objects(need, total)
    case = Case(need, total, lengths, seed=need * 5039 + total)
    h = case.clean.copy()
    words = planted_words(need * 5039 + total)
    columns, members, split, triples = {}, set(), 0, 0
    for o, L in enumerate(lengths):
        a = o % total
        b = (a + total // 2) % total
        a, b = min(a, b), max(a, b)
        q = flip_positions(L, need, rows)
        col = q[(o + o // total) % len(q)]
        for i, s in enumerate((a, b)):
            plant(h, case.places[o], L, s, col, words[(o + 5 * i) % len(words)], s < need)
        ca, cb = np.full(L, -1), np.full(L, -1)
        ca[col], cb[col] = a, b
        members |= {a, b}
        split += a >= need and (a - need) // 4 != (b - need) // 4
        if L >= 5 and o % 2 == 0:  # three wrong shards in another column
            c3 = (col + 2) % L
            for i, s in enumerate(((a + 1) % total, (b + 1) % total, (b + 2) % total)):
                plant(h, case.places[o], L, s, c3, words[(o + i) % len(words)], s < need)
            ca[c3] = total
            triples += 1
        columns[o] = (ca, cb)
    assert members == set(range(total)) and triples >= 3
    assert split >= 1 or rows <= 4, "a pair whose rows sit in different row blocks"
    exp = case.reference(h)
    assert_results(exp, planted_results(case, columns), "the reference names every pair and leaves the triples unlocated")
    assert (exp[0][:, :total].sum(axis=0) >= 1).all() and exp[0][:, total].sum() == triples
    run_ways(torch_dev, case, h, exp, what="slots")


# ------------------------------------------------------------------ 6. scrub sets

def test_scrub_set_with_nine_rows_down_to_one(torch_dev):
    """PlanSet.for_scrub(3, 12) with 0 to 8 shards missing per object (plans of 9 down to 1 rows in
    one launch) and two present shards of each object wrong in every column: objects whose plan has
    four rows or more name both, two or three rows report every column unlocated, and so does one
    row."""
    torch = torch_dev
    from slime_amd import device as D
    need, total, max_rows = 3, 12, 9
    T, C = geometry(need)
    rng = np.random.default_rng(5051)
    lengths, missing = [], []
    for m in range(9):
        for L in (T + 1, 5):
            lengths.append(L)
            missing.append(tuple(sorted(int(x) for x in rng.choice(total, size=m, replace=False))))
    nobj = len(lengths)
    _, want, places, _ = encode_case(need, total, lengths, 1, seed=5053)
    pset, plan_of, plans = scrub_set(need, total, missing)
    assert pset.max_rows == max_rows and {len(p[2]) for p in plans} == set(range(1, 10))
    batch = planned_batch(lengths, places, need, plan_of, pset.nplans)
    h = want.copy()
    blank(h, places, lengths, missing)
    ec, ef = PR.clean_results(nobj, need, max_rows)
    for o, L in enumerate(lengths):
        coeff, have, checked = plans[plan_of[o]]
        shards = have + checked
        sa, sb = (int(x) for x in rng.choice(len(shards), size=2, replace=False))
        for sl in (sa, sb):
            w = shard(h, places[o], shards[sl], L)
            w[:] ^= rng.integers(1, 2**31, size=L, dtype=np.uint64).astype(np.uint32)
        named = (sa, sb) if len(checked) >= 4 else (need + max_rows,)
        for sl in named:
            ec[o, sl], ef[o, sl] = L, 0
    exp = PR.locate_set_batch(plans, plan_of, max_rows, h, places, h, places, lengths, N.NO_PLAN)
    assert_results(exp, (ec, ef), "the reference: both shards from four rows up, unlocated below")
    ms = mappings(nobj, 5059)
    mt = to_dev(torch, np.array(ms, dtype=np.uint32))
    buf = to_dev(torch, h)
    bytes_h = to_chunks(h, places, lengths, total, ms)
    bbuf = torch.from_numpy(bytes_h.copy()).cuda()
    for mapping, b in ((None, buf), (mt, bbuf)):
        mism, _ = pset.verify_batch(b, b, batch) if mapping is None else D.verify_objects_batch(pset, b, b, batch, mt)
        assert_results(host(torch, raw_pairs(torch, pset, batch, b, b, mapping=mapping)), exp, mapping is None)
        assert_results(host(torch, raw_pairs(torch, pset, batch, b, b, mapping=mapping, filter=mism)), exp,
                       ("filter", mapping is None))
    assert_results(host(torch, pset.locate_batch(buf, buf, batch, max_wrong=2)), exp, "PlanSet.locate_batch")
    erasures = D.erasures_from_set_counts(pset.locate_batch(buf, buf, batch, max_wrong=2)[0], pset, plan_of, missing)
    for o in range(nobj):
        if len(plans[plan_of[o]][2]) >= 4:
            assert len(erasures[o]) == len(missing[o]) + 2, "erasures_from_set_counts works on the new counts"
    assert np.array_equal(to_host(torch, buf), h) and np.array_equal(bbuf.cpu().numpy(), bytes_h)


# ------------------------------------------------------------------ 7. launch conditions

def same_pair_case(need, total, seed):
    lengths, damaged = dense_lengths(need)
    case = Case(need, total, lengths, seed=seed)
    h, columns, _ = whole_shard_damage(case, damaged, "same", seed + 1)
    exp = case.reference(h)
    assert_results(exp, planted_results(case, columns), "the reference names both shards in every column")
    return case, h, exp


def test_every_schedule_and_pipeline_mode_gives_the_same_results(torch_dev, mode):
    torch = torch_dev
    case, h, exp = same_pair_case(8, 12, 5077)
    plan, batch, _, _ = case.gpu()
    buf = to_dev(torch, h)
    assert_results(host(torch, raw_pairs(torch, plan, batch, buf, buf)), exp, mode)


@pytest.mark.parametrize("need,total", [(8, 12), (17, 21)])
def test_separate_cmp_tensor_with_its_own_offsets(torch_dev, need, total):
    """src holds the data shards, cmp is another tensor with the parity rows only, objects in
    reverse order, odd shard strides, both behind a few words of padding: an input in src and a row
    in cmp wrong in one column are both named."""
    torch = torch_dev
    from slime_amd import device as D
    rows = total - need
    T, C = geometry(need)
    lengths = [T + 1, 0, 3, C * T + 5, 257, 4]
    nobj = len(lengths)
    _, want, sp, _ = encode_case(need, total, lengths, 1, seed=need * 5081 + total)
    cp, off = [None] * nobj, 9
    for o in reversed(range(nobj)):
        ss = -(-lengths[o] // 8) * 8 + 1
        cp[o] = (off, ss)
        off += rows * ss + 3
    cmp_h = np.full(off + 4, SENTINEL, dtype=np.uint32)
    src_h = want.copy()
    for o, L in enumerate(lengths):
        for i in range(rows):
            shard(cmp_h, cp[o], i, L)[:] = shard(want, sp[o], need + i, L)
            shard(src_h, sp[o], need + i, L)[:] = SENTINEL
    ec, ef = PR.clean_results(nobj, need, rows)
    for o, L in enumerate(lengths):
        if L == 0:
            continue
        j, i, col = o % need, (o + 1) % rows, L - 1 if o % 2 else L // 2
        plant(src_h, sp[o], L, j, col, 0x1234 + o, True)
        plant(cmp_h, cp[o], L, i, col, P + o % 5, False)
        ec[o, j], ef[o, j], ec[o, need + i], ef[o, need + i] = 1, col, 1, col
    coeff = OC.parity_matrix(need, rows)[need:]
    exp = PR.locate_batch(coeff, list(range(need)), list(range(rows)), src_h, sp, cmp_h, cp, lengths)
    assert_results(exp, (ec, ef), "the reference names the input in src and the row in cmp")
    plan = D.Plan.encode(need, total)  # outputs 0..rows-1
    assert np.array_equal(plan.coefficients(), coeff)
    batch = D.Batch([(so, ss, do, ds, L) for (so, ss), (do, ds), L in zip(sp, cp, lengths)], need)

    def padded(a, n):
        return to_dev(torch, np.concatenate([np.full(n, SENTINEL, dtype=np.uint32), a]))
    s, c = padded(src_h, 5), padded(cmp_h, 11)
    assert_results(host(torch, raw_pairs(torch, plan, batch, s, c, src_off_bytes=20, cmp_off_bytes=44)), exp, "raw")
    mism, _ = plan.verify_batch(s, c, batch, src_offset=5, cmp_offset=11)
    assert_results(host(torch, plan.locate_batch(s, c, batch, filter=mism, src_offset=5, cmp_offset=11, max_wrong=2)), exp)
    assert np.array_equal(to_host(torch, s)[5:], src_h) and np.array_equal(to_host(torch, c)[11:], cmp_h)


@pytest.mark.parametrize("need,total", [(8, 12), (17, 21)])
def test_captured_verify_and_pair_locate_replays(torch_dev, need, total):
    """verify_batch then the pair locate with its counts as the filter, captured as one graph on a
    non-default stream and replayed twice with the damage changed in between."""
    torch = torch_dev
    lengths, damaged = dense_lengths(need)
    case = Case(need, total, lengths, seed=need * 5087 + total)
    plan, batch, _, _ = case.gpu()
    buf = to_dev(torch, case.clean)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm the launch paths outside the capture, on the stream itself
        m0, _ = plan.verify_batch(buf, buf, batch, stream=s)
        res = raw_pairs(torch, plan, batch, buf, buf, filter=m0, stream=s)
    s.synchronize()
    assert_results(host(torch, res), PR.clean_results(len(lengths), need, total - need))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        gm, _ = plan.verify_batch(buf, buf, batch, stream=s)
        gc, gf_ = plan.locate_batch(buf, buf, batch, filter=gm, stream=s, max_wrong=2)
    torch.cuda.synchronize()
    for rnd, variant in enumerate(("same", "rotating")):
        h, columns, _ = whole_shard_damage(case, damaged[rnd:], variant, need * 5099 + total + rnd)
        exp = case.reference(h)
        assert_results(exp, planted_results(case, columns), ("the reference names what was planted", rnd))
        buf.copy_(to_dev(torch, h))
        gc.fill_(GARBAGE)
        gf_.fill_(GARBAGE)
        torch.cuda.synchronize()
        g.replay()
        assert_results(host(torch, (gc, gf_)), exp, rnd)
    del g  # before the batch: the graph's kernel nodes read its tables
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 8. refusals

def test_refusals(torch_dev):
    torch = torch_dev
    from slime_amd import device as D
    buf = to_dev(torch, np.zeros(4096, dtype=np.uint32))
    res = torch.full((2 * 70,), GARBAGE, dtype=torch.int64, device="cuda")
    p, r = ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(res.data_ptr())
    sym, byt = N.lib.slime_rs_plan_locate_pairs_batch, N.lib.slime_rs_locate_pairs_objects_batch
    ssym, sbyt = N.lib.slime_rs_planset_locate_pairs_batch, N.lib.slime_rs_planset_locate_pairs_objects_batch

    def refused(fn, args, text):
        assert fn(*args, None) == N.ERR_INVALID_ARG
        assert N.lib.slime_rs_last_error().decode() == text

    three, b4 = D.Plan.encode(4, 7), D.Batch([(0, 16, 0, 16, 16)], 4)
    text = "the plan has 3 rows: two wrong shards in a column take four rows to name"
    refused(sym, (three._h, b4._h, p, p, None, r, r), "plan_locate_pairs_batch: " + text)
    refused(byt, (three._h, b4._h, p, p, p, None, r, r), "locate_pairs_objects_batch: " + text)
    refused(sym, (three._h, b4._h, None, None, None, None, None), "plan_locate_pairs_batch: " + text)  # before the nulls
    set3, pb4 = D.PlanSet([three]), D.Batch([(0, 16, 0, 16, 16)], 4, plans=np.zeros(1, dtype=np.uint32), nplans=1)
    text = "no plan of the set has more than 3 rows: two wrong shards in a column take four rows to name"
    refused(ssym, (set3._h, pb4._h, p, p, None, r, r), "planset_locate_pairs_batch: " + text)
    refused(sbyt, (set3._h, pb4._h, p, p, p, None, r, r), "planset_locate_pairs_objects_batch: " + text)
    refused(ssym, (set3._h, b4._h, p, p, None, r, r),
            "planset_locate_pairs_batch: the batch carries no plan indices (create it with slime_rs_batch_create_planned)")
    wide, b40 = D.Plan.encode(40, 64), D.Batch([(0, 1, 0, 1, 1)], 40)
    text = "k + rows = 64 exceeds 63 (a wave's tally keeps one slot per lane)"
    refused(sym, (wide._h, b40._h, p, p, None, r, r), "plan_locate_pairs_batch: " + text)
    refused(byt, (wide._h, b40._h, p, p, p, None, r, r), "locate_pairs_objects_batch: " + text)
    four, b8 = D.Plan.encode(8, 12).set_outputs([8, 9, 10, 11]), D.Batch([(0, 16, 0, 16, 16)], 8)
    w = "plan_locate_pairs_batch: "
    refused(sym, (four._h, b8._h, p, p, None, None, r), w + "null result array")
    refused(sym, (four._h, b8._h, None, p, None, r, r), w + "null buffer")
    refused(byt, (four._h, b8._h, p, p, None, None, r, r), "locate_pairs_objects_batch: null mapping")
    refused(sym, (four._h, b4._h, p, p, None, r, r), w + "the batch was created for k = 4 on device 0, "
                                                         "the plan has k = 8 on device 0")
    with pytest.raises(N.NativeError, match="take four rows"):
        three.locate_batch(buf, buf, b4, max_wrong=2)
    with pytest.raises(ValueError, match="max_wrong"):
        four.locate_batch(buf, buf, b8, max_wrong=3)
    torch.cuda.synchronize()
    assert (res == GARBAGE).all(), "a refused call touches nothing"
    four.set_outputs([8, 9, 10, 11])  # refusals do not mark the plan
    c, f = four.locate_batch(buf, buf, b8, max_wrong=2)  # zeros are a codeword
    assert_results(host(torch, (c, f)), PR.clean_results(1, 8, 4))
    with pytest.raises(N.NativeError, match="already launched"):
        four.set_outputs([0, 1, 2, 3])
    none = D.Batch([], 8)
    assert sym(four._h, none._h, p, p, None, r, r, None) == 0  # nobj == 0 touches nothing
    torch.cuda.synchronize()
    assert (res == GARBAGE).all()
    c, f = four.locate_batch(buf, buf, none, max_wrong=2)
    assert c.shape == f.shape == (0, 13)


# ------------------------------------------------------------------ 9. the one-shard calls are unchanged

@pytest.mark.parametrize("need,total", [(8, 12), (17, 21)])
def test_one_shard_calls_still_report_the_pairs_as_unlocated(torch_dev, need, total):
    torch = torch_dev
    case, h, exp = same_pair_case(need, total, need * 5101 + total)
    one = case.one_shard_reference(h)
    damaged = [o for o in range(len(case.lengths)) if exp[0][o].sum()]
    for o in damaged:
        assert one[0][o, case.n] == case.lengths[o] and one[0][o, :case.n].sum() == 0, "unlocated for the one-shard rule"
    plan, batch, pset, pbatch = case.gpu()
    buf = to_dev(torch, h)
    assert_results(host(torch, raw_locate(torch, plan, batch, buf, buf)), one, "plan")
    assert_results(host(torch, raw_set_locate(torch, pset, pbatch, buf, buf)), one, "set")
    assert_results(host(torch, plan.locate_batch(buf, buf, batch)), one, "max_wrong defaults to 1")
    assert_results(host(torch, raw_pairs(torch, plan, batch, buf, buf)), exp, "and the pair call names them")


# ------------------------------------------------------------------ 10. end to end

def test_scrub_locate_pairs_repair_restores_two_overwritten_chunks(torch_dev):
    """8/12: two whole chunks of a third of the objects overwritten (data+data, data+parity,
    parity+parity), then verify_batch -> locate_batch(max_wrong=2) -> erasures_from_counts ->
    PlanSet.for_erasures with a planned Batch -> execute_batch: the buffer equals the original
    codewords bit for bit and a second verify is clean."""
    torch = torch_dev
    from slime_amd import device as D
    need, total = 8, 12
    T, C = geometry(need)
    lengths = [T + 5, 3, C * T + 1, 0, 260, 7, 2 * T, 64, 1030, 4, T - 1, 513]
    case = Case(need, total, lengths, seed=5107)
    plan, batch, _, _ = case.gpu()
    # A repair writes canonical residues: the objects' data is canonical, as an ingest stores it.
    start = case.clean.copy()
    for place, L in zip(case.places, lengths):
        for s_ in range(need):
            shard(start, place, s_, L)[:] %= np.uint32(P)
    buf = to_dev(torch, start)
    plan.execute_batch(buf, buf, batch)
    original = to_host(torch, buf).copy()
    assert case.reference(original)[0].sum() == 0
    h = original.copy()
    rng = np.random.default_rng(5113)
    expect = [[] for _ in lengths]
    pairs = [(1, 6), (3, 9), (8, 11), (0, 10)]
    for n, o in enumerate(range(0, len(lengths), 3)):
        if lengths[o] == 0:
            continue
        for s in pairs[n % len(pairs)]:
            if n % 2:
                shard(h, case.places[o], s, lengths[o])[:] = 0  # a zeroed chunk
            else:
                replace_shard(h, case, o, s, rng)  # a stale one
        expect[o] = sorted(pairs[n % len(pairs)])
    assert sum(1 for e in expect if e) == 3
    exp = case.reference(h)
    buf.copy_(to_dev(torch, h))
    mism, _ = plan.verify_batch(buf, buf, batch)
    counts, first = plan.locate_batch(buf, buf, batch, filter=mism, max_wrong=2)
    assert_results(host(torch, (counts, first)), exp)
    assert int(counts[:, total].sum()) == 0, "nothing unlocated"
    erasures = D.erasures_from_counts(counts, plan.locate_slots())
    assert D.erasures_from_counts(exp[0], list(range(total))) == expect, "the reference names the overwritten chunks"
    assert erasures == expect
    pset, plan_of = D.PlanSet.for_erasures(need, total, erasures)
    spans = [(off, ss, off, ss, L) for (off, ss), L in zip(case.places, lengths)]
    planned = D.Batch(spans, need, plans=plan_of, nplans=pset.nplans)
    pset.execute_batch(buf, buf, planned)
    assert np.array_equal(to_host(torch, buf), original), "repaired bit for bit"
    m2, f2 = plan.verify_batch(buf, buf, batch)
    torch.cuda.synchronize()
    assert int(m2.sum()) == 0 and bool((f2 == -1).all())
