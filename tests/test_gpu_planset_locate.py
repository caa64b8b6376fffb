"""Plan-set locate (slime_rs_planset_locate_batch, slime_rs_planset_locate_objects_batch) on the
GPU: degraded objects located from their own survivor sets in one launch.

Every expectation comes from tests/planset_locate_ref.py on host copies: locate_ref's rule over
oracle_c.apply_matrix rows with each object's own plan, whose coefficient rows are the oracle's
too (parity_matrix rows of the checked shards times the oracle's inverse of the survivors'
rows) -- never from a kernel.  Result arrays are pre-filled with garbage, so every launch also
proves the initialisation; data buffers are compared with their host copies afterwards.
Lengths are test_gpu_ragged_verify's boundary lengths, planted columns its flip positions.
"""
import ctypes

import numpy as np
import pytest

import locate_ref as R
import planset_locate_ref as SR
from oracle import oracle_c as OC
from slime_amd import _native as N
from test_gpu_locate import LOCATE_CODES, one_word_rounds, plant, planted_words, reference, to_chunks
from test_gpu_ragged import (P, encode_case, encode_plan, geometry, mode, packed_spans, shard, to_dev,  # noqa: F401
                             to_host, torch_dev)
from test_gpu_ragged_verify import assert_results, flip_positions, host, verify_lengths
from test_gpu_verify import GARBAGE

pytestmark = pytest.mark.gpu

MISSING = 0xE7A5ED00  # what the slot of an absent shard holds (>= p: never a canonical residue)


# ------------------------------------------------------------------ helpers

_scrub = {}


def scrub_rows(need, total, key):
    """(coeff, have, want) of the scrub plan for the absent shards `key`, from the oracle alone:
    the first `need` present shards rebuild the data (the oracle's inverse of their rows), the
    parity matrix's rows of the other present shards map the data onto the checked shards."""
    k = (need, total, tuple(key))
    if k not in _scrub:
        present = [i for i in range(total) if i not in key]
        have, want = present[:need], present[need:]
        m = OC.parity_matrix(need, total - need)
        rc, inv = OC.invert_matrix(m[have])
        assert rc == 0
        a, b = m[want].astype(object), inv.astype(object)
        coeff = np.array([[sum(int(a[i, t]) * int(b[t, j]) for t in range(need)) % P for j in range(need)]
                          for i in range(len(want))], dtype=np.uint32).reshape(len(want), need)
        _scrub[k] = (coeff, have, want)
    return _scrub[k]


def keys_of(missing):
    return [tuple(sorted(set(int(x) for x in pat))) if pat is not None else () for pat in missing]


def scrub_set(need, total, missing):
    """PlanSet.for_scrub's set and indices, the indices checked against their restatement, and
    the reference's plans [(coeff, have, want)] in the set's order."""
    from slime_amd import device as D
    pset, plan_of = D.PlanSet.for_scrub(need, total, missing)
    index, mine = {}, []
    for key in keys_of(missing):
        mine.append(N.NO_PLAN if total - len(key) == need else index.setdefault(key, len(index)))
    assert plan_of.dtype == np.uint32 and plan_of.tolist() == mine
    plans = [scrub_rows(need, total, key) for key in index]
    assert pset.nplans == len(plans) and pset.k == need and pset.max_rows == max(len(p[2]) for p in plans)
    for i, (coeff, have, want) in enumerate(plans):
        assert all(w >= need for w in want), "the checked shards are parity rows"
        assert pset.locate_slots(i) == have + want + [None] * (pset.max_rows - len(want))
    return pset, plan_of, plans


def planned_batch(lengths, places, k, plan_of, nplans):
    from slime_amd import device as D
    return D.Batch([(off, ss, off, ss, L) for (off, ss), L in zip(places, lengths)], k, plans=plan_of, nplans=nplans)


def blank(h, places, lengths, missing):
    for place, L, pat in zip(places, lengths, missing):
        for s in (pat or ()):
            shard(h, place, s, L)[:] = MISSING


def set_reference(plans, plan_of, max_rows, h, places, lengths, skip=()):
    return SR.locate_batch(plans, plan_of, max_rows, h, places, h, places, lengths, N.NO_PLAN, skip)


def raw_set_locate(torch, pset, batch, src, cmp, filter=None, mapping=None, stream=None, src_off_bytes=0,
                   cmp_off_bytes=0):
    """The C entry point into result arrays pre-filled with garbage (bytes form when mapping is given)."""
    from slime_amd import device as D
    n = pset.k + pset.max_rows + 1
    counts = torch.full((batch.nobj, n), GARBAGE, dtype=torch.int64, device="cuda")
    first = torch.full((batch.nobj, n), GARBAGE, dtype=torch.int64, device="cuda")
    f = ctypes.c_void_p(filter.data_ptr()) if filter is not None else None
    tail = (f, ctypes.c_void_p(counts.data_ptr()), ctypes.c_void_p(first.data_ptr()), D._stream_handle(0, stream))
    a, b = ctypes.c_void_p(src.data_ptr() + src_off_bytes), ctypes.c_void_p(cmp.data_ptr() + cmp_off_bytes)
    if mapping is None:
        N.check(N.lib.slime_rs_planset_locate_batch(pset._h, batch._h, a, b, *tail))
    else:
        N.check(N.lib.slime_rs_planset_locate_objects_batch(pset._h, batch._h, a, b,
                                                            ctypes.c_void_p(mapping.data_ptr()), *tail))
    return counts, first


def slot_of_shard(plan, s):
    coeff, have, want = plan
    return (have + want).index(s)


# ------------------------------------------------------------------ 1. a one-plan set equals the plan

@pytest.mark.parametrize("need,total", LOCATE_CODES)
def test_one_plan_set_equals_the_plan(torch_dev, need, total):
    """PlanSet([encode plan]) with every object on plan 0: clean data, then one wrong word per
    object over every flip position -- exactly the single-plan reference's results (17/20 and
    33/50 take the column form)."""
    torch = torch_dev
    from slime_amd import device as D
    rows = total - need
    lengths, places, rounds = one_word_rounds(need, total, seed=need * 3011 + total)
    plan = encode_plan(need, total)
    pset = D.PlanSet([plan])
    assert (pset.nplans, pset.k, pset.max_rows) == (1, need, rows)
    assert pset.locate_slots(0) == plan.locate_slots() == list(range(total))
    batch = planned_batch(lengths, places, need, np.zeros(len(lengths), dtype=np.uint32), 1)
    _, want, _, _ = encode_case(need, total, lengths, 1, seed=need * 3011 + total)
    buf = to_dev(torch, want)
    assert_results(host(torch, raw_set_locate(torch, pset, batch, buf, buf)), R.clean_results(len(lengths), need, rows))
    c, f = pset.locate_batch(buf, buf, batch)
    assert c.shape == f.shape == (len(lengths), total + 1) and c.dtype == f.dtype == torch.int64
    assert_results(host(torch, (c, f)), R.clean_results(len(lengths), need, rows))
    for p, (h, planted) in enumerate(rounds):
        exp = reference(need, total, h, places, lengths)
        assert_results(exp, planted, ("the reference names the planted slot", p))
        buf.copy_(to_dev(torch, h))
        assert_results(host(torch, raw_set_locate(torch, pset, batch, buf, buf)), exp, p)
        assert np.array_equal(to_host(torch, buf), h)


# ------------------------------------------------------------------ 2. mixed survivor sets

_mixed = {}


def mixed_case():
    """8/12, 198 objects over verify's lengths, missing[o] rotating over (), every single shard and
    every pair -- all 79 for_scrub plans.  Objects 5 and 40 are overridden to NO_PLAN (damaged all
    the same).  Round r plants one wrong word per object, the slot class rotating with o + r: an
    input of its plan, a checked row, a data-shard input given a value >= p.  Cached, read-only:
    (lengths, places, missing, no_plan, [(host buffer, planted (counts, first))])."""
    if _mixed:
        return _mixed["case"]
    need, total, max_rows = 8, 12, 4
    base = verify_lengths(need, max_rows)
    singles = [(s,) for s in (0, 11, 3, 8, 1, 2, 4, 5, 6, 7, 9, 10)]
    pairs = [(a, b) for a in range(total) for b in range(a + 1, total)]
    pairs.sort(key=lambda ab: (ab != (0, 11), ab))  # shard 0 and shard 11 together comes first
    nobj = 3 * len(pairs)
    lengths = [base[(o + o // len(base)) % len(base)] for o in range(nobj)]
    missing = [[(), singles[(o // 3) % 12], pairs[(o // 3) % 66]][o % 3] for o in range(nobj)]
    no_plan = (5, 40)
    _, want, places, _ = encode_case(need, total, lengths, 1, seed=8 * 3083 + 12)
    clean = want.copy()
    blank(clean, places, lengths, missing)
    words = planted_words(3083)
    big = [int(w) for w in words if int(w) >= P]
    rounds = []
    for r in range(3):
        h = clean.copy()
        ec, ef = SR.clean_results(nobj, need, max_rows)
        for o, L in enumerate(lengths):
            if L == 0:
                continue
            coeff, have, want_ = scrub_rows(need, total, keys_of([missing[o]])[0])
            q = flip_positions(L, need, max_rows)
            col = q[(o + r) % len(q)]
            kind = (o + r) % 3
            if kind == 0:
                slot = (o // 3 + r) % need
                plant(h, places[o], L, have[slot], col, words[(3 * o + r) % len(words)], True)  # inputs count mod p
            elif kind == 1:
                slot = need + (o // 3 + r) % len(want_)
                plant(h, places[o], L, want_[slot - need], col, words[(3 * o + r) % len(words)], False)
            else:
                data = [j for j, s in enumerate(have) if s < need]
                slot = data[(o // 3 + r) % len(data)]
                plant(h, places[o], L, have[slot], col, big[(o + r) % len(big)], True)
            if o not in no_plan:
                ec[o, slot], ef[o, slot] = 1, col
        rounds.append((h, (ec, ef)))
    _mixed["case"] = (lengths, places, missing, no_plan, rounds)
    return _mixed["case"]


_sets = {}


def mixed_set(torch):
    """The mixed case's set, indices (with the NO_PLAN overrides), reference plans and batch; cached."""
    if "s" not in _sets:
        lengths, places, missing, no_plan, _ = mixed_case()
        pset, plan_of, plans = scrub_set(8, 12, missing)
        assert pset.nplans == 79 and pset.max_rows == 4
        assert sorted(len(p[2]) for p in plans) == [2] * 66 + [3] * 12 + [4]
        plan_of = plan_of.copy()
        for o in no_plan:
            plan_of[o] = N.NO_PLAN
        _sets["s"] = (pset, plan_of, plans, planned_batch(lengths, places, 8, plan_of, pset.nplans))
    return _sets["s"]


def test_mixed_survivor_sets(torch_dev):
    """Every object located with its own plan: the planted slot, count 1 and column exactly;
    NO_PLAN objects, L == 0 objects and the slots past an object's rows keep the initial values."""
    torch = torch_dev
    lengths, places, missing, no_plan, rounds = mixed_case()
    pset, plan_of, plans, batch = mixed_set(torch)
    assert lengths.count(0) >= 3 and {len(keys_of([m])[0]) for m in missing} == {0, 1, 2}
    buf = to_dev(torch, rounds[0][0])
    seen = set()
    for r, (h, planted) in enumerate(rounds):
        exp = set_reference(plans, plan_of, 4, h, places, lengths)
        assert_results(exp, planted, ("the reference names every planted shard, nothing unlocated", r))
        assert (exp[0][:, 12] == 0).all()
        for o in range(len(lengths)):
            rows_o = 12 - 8 - len(keys_of([missing[o]])[0])
            assert (exp[0][o, 8 + rows_o: 12] == 0).all() and (exp[1][o, 8 + rows_o: 12] == -1).all()
            seen |= {"input" if s < 8 else "row" for s in np.flatnonzero(exp[0][o])}
        for o in no_plan:
            assert lengths[o] > 0 and exp[0][o].sum() == 0
        buf.copy_(to_dev(torch, h))
        assert_results(host(torch, raw_set_locate(torch, pset, batch, buf, buf)), exp, r)
        assert np.array_equal(to_host(torch, buf), h), "locate writes nothing but its results"
    assert seen == {"input", "row"}
    c, f = pset.locate_batch(buf, buf, batch)
    assert c.shape == f.shape == (len(lengths), 13)
    assert_results(host(torch, (c, f)), set_reference(plans, plan_of, 4, rounds[-1][0], places, lengths))


# ------------------------------------------------------------------ 3. objects whose plan has one row

@pytest.mark.parametrize("need,total,nmiss", [(3, 5, 1), (4, 6, 1), (8, 12, 3)])
def test_one_row_objects_are_unlocated_beside_located_ones(torch_dev, need, total, nmiss):
    """Objects with total - need - 1 shards absent keep one checked row: a wrong word anywhere in
    them is `unlocated` at slot k + max_rows; their intact neighbours (max_rows rows: R = 4 for
    8/12) are located normally."""
    torch = torch_dev
    rows = total - need
    assert rows - nmiss == 1
    T, C = geometry(need)
    lengths = [T + 9, 7, 260, C * T + 5, 0, 3, 2 * T + 2, T, 5, 257]
    _, want, places, _ = encode_case(need, total, lengths, 1, seed=need * 3089 + total)
    pats = [tuple(sorted((o + 5 * i) % total for i in range(nmiss))) for o in range(len(lengths))]
    missing = [() if o % 2 == 0 else pats[o] for o in range(len(lengths))]
    assert all(len(set(m)) == len(m) for m in missing)
    pset, plan_of, plans = scrub_set(need, total, missing)
    assert pset.max_rows == rows and 1 in [len(p[2]) for p in plans]
    batch = planned_batch(lengths, places, need, plan_of, pset.nplans)
    h = want.copy()
    blank(h, places, lengths, missing)
    ec, ef = SR.clean_results(len(lengths), need, rows)
    unl = need + rows
    for o, L in enumerate(lengths):
        if L == 0:
            continue
        coeff, have, want_ = plans[plan_of[o]]
        q = flip_positions(L, need, rows)
        if len(want_) == 1:
            # one word in an input, and (where there is a second position) one in the checked row
            s = have[o % need]
            plant(h, places[o], L, s, q[-1], 0x1234 + o, True)
            cols = [q[-1]]
            if len(q) > 1:
                plant(h, places[o], L, want_[0], q[0], P + o % 5, False)
                cols.append(q[0])
            ec[o, unl], ef[o, unl] = len(cols), min(cols)
        else:
            slot = (o // 2) % total
            plant(h, places[o], L, slot, q[o % len(q)], 77 + o, slot < need)
            ec[o, slot], ef[o, slot] = 1, q[o % len(q)]
    exp = set_reference(plans, plan_of, rows, h, places, lengths)
    assert_results(exp, (ec, ef), "the reference: one-row objects unlocated, the others named")
    buf = to_dev(torch, h)
    assert_results(host(torch, raw_set_locate(torch, pset, batch, buf, buf)), exp)
    mism, _ = pset.verify_batch(buf, buf, batch)
    assert_results(host(torch, raw_set_locate(torch, pset, batch, buf, buf, filter=mism)), exp)
    assert np.array_equal(to_host(torch, buf), h)


# ------------------------------------------------------------------ 4. two wrong shards

def test_two_wrong_shards_of_degraded_objects(torch_dev):
    """In different columns of one object each is named; in the same column the reference says
    unlocated (asserted), and the GPU agrees."""
    torch = torch_dev
    need, total = 8, 12
    T, C = geometry(need)
    lengths = [C * T + 7, 260, 2 * T + 2, 6, T + 9, 516]
    missing = [(0,), (11,), (3, 9), (), (1,), (2, 10)]
    _, want, places, _ = encode_case(need, total, lengths, 1, seed=3109)
    pset, plan_of, plans = scrub_set(need, total, missing)
    batch = planned_batch(lengths, places, need, plan_of, pset.nplans)
    h = want.copy()
    blank(h, places, lengths, missing)
    ec, ef = SR.clean_results(len(lengths), need, 4)
    for o, L in enumerate(lengths):
        coeff, have, want_ = plans[plan_of[o]]
        a, b = have[(o + 1) % need], want_[o % len(want_)]
        if o < 3:  # different columns
            ca, cb = (L - 1, 0) if o % 2 else (1, L - 2)
            plant(h, places[o], L, a, ca, 0x4321 + o, True)
            plant(h, places[o], L, b, cb, P + o, False)
            sa, sb_ = slot_of_shard(plans[plan_of[o]], a), slot_of_shard(plans[plan_of[o]], b)
            ec[o, sa], ef[o, sa], ec[o, sb_], ef[o, sb_] = 1, ca, 1, cb
        else:      # the same column: input + row, two inputs, two rows
            col = [L - 1, 2, 257][o - 3]
            pair = [(a, b), (have[0], have[need - 1]), (want_[0], want_[-1])][o - 3]
            assert pair[0] != pair[1]
            for s in pair:
                plant(h, places[o], L, s, col, 0x9E3779B9 * (o + s + 1) & 0xFFFFFFFF, s in have)
            ec[o, 12], ef[o, 12] = 1, col
    exp = set_reference(plans, plan_of, 4, h, places, lengths)
    assert_results(exp, (ec, ef), "the reference names both shards, or says unlocated for one column")
    buf = to_dev(torch, h)
    assert_results(host(torch, raw_set_locate(torch, pset, batch, buf, buf)), exp)


# ------------------------------------------------------------------ 5. a whole shard wrong

def test_whole_shard_of_a_degraded_object_wrong(torch_dev):
    """Every word of one survivor XOR 1 in multi-unit degraded objects: that slot counts L from
    column 0 -- an input in one object, a checked row in the other (tally_slots flushing across
    units and waves)."""
    torch = torch_dev
    need, total = 8, 12
    T, C = geometry(need)
    L = 2 * C * T + T + 6
    lengths = [L, 9, L]
    missing = [(1, 9), (), (0,)]
    _, want, places, _ = encode_case(need, total, lengths, 1, seed=3119)
    pset, plan_of, plans = scrub_set(need, total, missing)
    batch = planned_batch(lengths, places, need, plan_of, pset.nplans)
    assert batch.units >= 6
    h = want.copy()
    blank(h, places, lengths, missing)
    hit = [plans[plan_of[0]][1][3], None, plans[plan_of[2]][2][1]]  # an input of object 0, a row of object 2
    ec, ef = SR.clean_results(3, need, 4)
    for o, s in enumerate(hit):
        if s is not None:
            shard(h, places[o], s, L)[:] ^= np.uint32(1)
            slot = slot_of_shard(plans[plan_of[o]], s)
            ec[o, slot], ef[o, slot] = L, 0
    exp = set_reference(plans, plan_of, 4, h, places, lengths)
    assert_results(exp, (ec, ef), "the reference blames the replaced shard in every column")
    buf = to_dev(torch, h)
    assert_results(host(torch, raw_set_locate(torch, pset, batch, buf, buf)), exp)
    assert np.array_equal(to_host(torch, buf), h)


# ------------------------------------------------------------------ 6. the filter

def filter_case():
    need, total = 8, 12
    T, C = geometry(need)
    lengths = [C * T + 5, 3, T + 1, 0, 2 * C * T + 2, 257, 6, T, 64]
    missing = [(2,), (), (0, 11), (5,), (), (7, 8), (10,), (1, 4), ()]
    _, want, places, _ = encode_case(need, total, lengths, 1, seed=3121)
    clean = want.copy()
    blank(clean, places, lengths, missing)
    return need, total, lengths, missing, places, clean


def test_filter_skips_clean_objects_on_the_device(torch_dev):
    torch = torch_dev
    need, total, lengths, missing, places, clean = filter_case()
    pset, plan_of, plans = scrub_set(need, total, missing)
    batch = planned_batch(lengths, places, need, plan_of, pset.nplans)
    h = clean.copy()
    dirty = {0: 5, 2: geometry(need)[0], 5: 256, 6: 5}  # object: column
    for o, col in dirty.items():
        coeff, have, want_ = plans[plan_of[o]]
        s = (have + want_)[(3 * o + 1) % (need + len(want_))]
        plant(h, places[o], lengths[o], s, col, 77 + o, s in have)
    full = set_reference(plans, plan_of, 4, h, places, lengths)
    assert sorted(np.flatnonzero(full[0].sum(axis=1))) == sorted(dirty) and full[0][:, 12].sum() == 0
    buf = to_dev(torch, h)
    mism, _ = pset.verify_batch(buf, buf, batch)
    assert mism.shape == (len(lengths), 4)
    assert sorted(np.flatnonzero(mism.cpu().numpy().sum(axis=1))) == sorted(dirty)
    assert_results(host(torch, raw_set_locate(torch, pset, batch, buf, buf, filter=mism)), full,
                   "dirty objects as with filter=None, clean ones at their initial values")
    assert_results(host(torch, pset.locate_batch(buf, buf, batch, filter=mism)), full)
    assert_results(host(torch, raw_set_locate(torch, pset, batch, buf, buf)), full)
    # a filter of zeros skips everything, even on damaged data
    zeros = torch.zeros_like(mism)
    assert_results(host(torch, raw_set_locate(torch, pset, batch, buf, buf, filter=zeros)),
                   SR.clean_results(len(lengths), need, 4))
    # a hand-made filter that clears dirty objects: the skip is the device's, whatever the data says
    hand = mism.clone()
    hand[0] = 0
    hand[5] = 0
    hand[7, 3] = 9  # a clean object the filter calls dirty (in a row past its own two) is scanned, and found clean
    cleared = set_reference(plans, plan_of, 4, h, places, lengths, skip=(0, 5))
    assert cleared[0][0].sum() == 0 and cleared[0][2].sum() == 1
    assert_results(host(torch, raw_set_locate(torch, pset, batch, buf, buf, filter=hand)), cleared)
    assert np.array_equal(to_host(torch, buf), h)


def test_captured_scrub_and_locate_chain_replays_clean(torch_dev):
    """PlanSet.verify_batch then locate_batch(filter=mismatches) captured in one graph on a
    non-default stream and replayed twice over the same damage: the same results each time, the
    arrays starting clean on each replay (they are filled with garbage in between)."""
    torch = torch_dev
    need, total, lengths, missing, places, clean = filter_case()
    pset, plan_of, plans = scrub_set(need, total, missing)
    batch = planned_batch(lengths, places, need, plan_of, pset.nplans)
    h = clean.copy()
    for o, col in {0: 9, 4: 1025, 7: 767}.items():
        coeff, have, want_ = plans[plan_of[o]]
        s = (have + want_)[(5 * o + 2) % (need + len(want_))]
        plant(h, places[o], lengths[o], s, col, 31 + o, s in have)
    exp = set_reference(plans, plan_of, 4, h, places, lengths)
    assert int(exp[0].sum()) == 3 and exp[0][:, 12].sum() == 0
    buf = to_dev(torch, clean)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm the launch paths outside the capture, on the stream itself
        m0, _ = pset.verify_batch(buf, buf, batch, stream=s)
        res = raw_set_locate(torch, pset, batch, buf, buf, filter=m0, stream=s)
    s.synchronize()
    assert_results(host(torch, res), SR.clean_results(len(lengths), need, 4))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        gm, _ = pset.verify_batch(buf, buf, batch, stream=s)
        gc, gf_ = pset.locate_batch(buf, buf, batch, filter=gm, stream=s)
    torch.cuda.synchronize()
    buf.copy_(to_dev(torch, h))
    for rnd in range(2):
        gc.fill_(GARBAGE)
        gf_.fill_(GARBAGE)
        torch.cuda.synchronize()
        g.replay()
        assert_results(host(torch, (gc, gf_)), exp, rnd)
    del g  # before the batch: the graph's kernel nodes read its tables
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 7. bytes

def test_bytes_mixed_survivor_sets_and_filter(torch_dev):
    """The mixed case and the filter through slime_rs_planset_locate_objects_batch with a mapping
    per object (0, 1 << 31 and random values): the symbol reference's results."""
    torch = torch_dev
    from slime_amd import device as D
    lengths, places, missing, no_plan, rounds = mixed_case()
    pset, plan_of, plans, batch = mixed_set(torch)
    rng = np.random.default_rng(3137)
    ms = [[0, 1 << 31, int(rng.integers(0, 2**32))][(o // 2) % 3] for o in range(len(lengths))]
    mt = to_dev(torch, np.array(ms, dtype=np.uint32))
    for r in (0, 2):
        h = rounds[r][0]
        hb = to_chunks(h, places, lengths, 12, ms)
        buf = torch.from_numpy(hb.copy()).cuda()
        exp = set_reference(plans, plan_of, 4, h, places, lengths)
        assert exp[0].sum() >= 150 and exp[0][:, 12].sum() == 0
        assert_results(host(torch, raw_set_locate(torch, pset, batch, buf, buf, mapping=mt)), exp, r)
        assert np.array_equal(buf.cpu().numpy(), hb)
    assert_results(host(torch, D.locate_objects_batch(pset, buf, buf, batch, mt)), exp)
    # the filter: a byte verify's mismatches, zeros, and a few objects cleared by hand
    mism, _ = D.verify_objects_batch(pset, buf, buf, batch, mt)
    assert mism.shape == (len(lengths), 4)
    assert_results(host(torch, raw_set_locate(torch, pset, batch, buf, buf, mapping=mt, filter=mism)), exp)
    assert_results(host(torch, D.locate_objects_batch(pset, buf, buf, batch, mt, filter=mism)), exp)
    assert_results(host(torch, raw_set_locate(torch, pset, batch, buf, buf, mapping=mt, filter=torch.zeros_like(mism))),
                   SR.clean_results(len(lengths), 8, 4))
    hand = mism.clone()
    skip = (0, 7, 100)
    for o in skip:
        hand[o] = 0
    cleared = set_reference(plans, plan_of, 4, h, places, lengths, skip=skip)
    assert cleared[0].sum() < exp[0].sum()
    assert_results(host(torch, raw_set_locate(torch, pset, batch, buf, buf, mapping=mt, filter=hand)), cleared)
    assert np.array_equal(buf.cpu().numpy(), hb)


def test_bytes_captured_chain(torch_dev):
    """verify_objects_batch + locate_objects_batch of a set captured in one graph, replayed twice."""
    torch = torch_dev
    from slime_amd import device as D
    need, total, lengths, missing, places, clean = filter_case()
    pset, plan_of, plans = scrub_set(need, total, missing)
    batch = planned_batch(lengths, places, need, plan_of, pset.nplans)
    h = clean.copy()
    for o, col in {2: 3, 4: 770, 8: 63}.items():
        coeff, have, want_ = plans[plan_of[o]]
        s = (have + want_)[(7 * o + 3) % (need + len(want_))]
        plant(h, places[o], lengths[o], s, col, 41 + o, s in have)
    exp = set_reference(plans, plan_of, 4, h, places, lengths)
    assert int(exp[0].sum()) == 3 and exp[0][:, 12].sum() == 0
    ms = [0, 1 << 31, 0xDEADBEEF, 5, 0x80000001, 0, 1 << 31, 77, 0x7FFFFFFF]
    mt = to_dev(torch, np.array(ms, dtype=np.uint32))
    buf = torch.from_numpy(to_chunks(clean, places, lengths, total, ms).copy()).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        m0, _ = D.verify_objects_batch(pset, buf, buf, batch, mt, stream=s)
        res = D.locate_objects_batch(pset, buf, buf, batch, mt, filter=m0, stream=s)
    s.synchronize()
    assert_results(host(torch, res), SR.clean_results(len(lengths), need, 4))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        gm, _ = D.verify_objects_batch(pset, buf, buf, batch, mt, stream=s)
        gc, gf_ = D.locate_objects_batch(pset, buf, buf, batch, mt, filter=gm, stream=s)
    torch.cuda.synchronize()
    buf.copy_(torch.from_numpy(to_chunks(h, places, lengths, total, ms).copy()).cuda())
    for rnd in range(2):
        gc.fill_(GARBAGE)
        gf_.fill_(GARBAGE)
        torch.cuda.synchronize()
        g.replay()
        assert_results(host(torch, (gc, gf_)), exp, rnd)
    del g
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 8. the column form by alignment

@pytest.mark.parametrize("src_off,cmp_off", [(2, 0), (0, 2), (2, 2)])
def test_bases_not_word_aligned_take_the_column_form(torch_dev, src_off, cmp_off):
    torch = torch_dev
    lengths, places, missing, no_plan, rounds = mixed_case()
    pset, plan_of, plans, batch = mixed_set(torch)
    h = rounds[1][0]
    exp = set_reference(plans, plan_of, 4, h, places, lengths)
    assert exp[0].sum() >= 150

    def shifted(a, off):
        b = np.full(a.size * 4 + 8, 0xA5, dtype=np.uint8)
        b[off: off + a.size * 4] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        return torch.from_numpy(b).cuda()

    src, cmp = shifted(h, src_off), shifted(h, cmp_off)
    got = raw_set_locate(torch, pset, batch, src, cmp, src_off_bytes=src_off, cmp_off_bytes=cmp_off)
    assert_results(host(torch, got), exp)


# ------------------------------------------------------------------ 9. schedule and pipeline modes

def test_every_schedule_and_pipeline_mode_gives_the_same_results(torch_dev, mode):
    torch = torch_dev
    lengths, places, missing, no_plan, rounds = mixed_case()
    pset, plan_of, plans, batch = mixed_set(torch)
    h = rounds[1][0]
    buf = to_dev(torch, h)
    assert_results(host(torch, raw_set_locate(torch, pset, batch, buf, buf)),
                   set_reference(plans, plan_of, 4, h, places, lengths))


# ------------------------------------------------------------------ 10. refusals

def test_refusals(torch_dev):
    torch = torch_dev
    from slime_amd import device as D
    lengths = [16, 5]
    _, want, places, _ = encode_case(4, 6, lengths, 1, seed=3163)
    buf = to_dev(torch, want)
    pset, plan_of, plans = scrub_set(4, 6, [(), (5,)])
    assert pset.nplans == 2 and pset.max_rows == 2
    batch = planned_batch(lengths, places, 4, plan_of, 2)
    res = torch.full((2 * 7,), GARBAGE, dtype=torch.int64, device="cuda")
    p, r = ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(res.data_ptr())
    sym, byt = N.lib.slime_rs_planset_locate_batch, N.lib.slime_rs_planset_locate_objects_batch

    def refused(fn, args, text):
        assert fn(*args, None) == N.ERR_INVALID_ARG
        assert N.lib.slime_rs_last_error().decode() == text

    unplanned = D.Batch([(off, ss, off, ss, L) for (off, ss), L in zip(places, lengths)], 4)
    three = planned_batch(lengths, places, 4, plan_of, 3)
    one = D.PlanSet([D.Plan.encode(1, 2)])
    b1 = D.Batch([(0, 4, 0, 4, 4)], 1, plans=[0], nplans=1)
    wide = D.PlanSet([D.Plan.encode(40, 64)])
    b40 = D.Batch([(0, 1, 0, 1, 1)], 40, plans=[0], nplans=1)
    for fn, w, m in ((sym, "planset_locate_batch: ", ()), (byt, "planset_locate_objects_batch: ", (p,))):
        refused(fn, (None, batch._h, p, p, *m, None, r, r), w + "null set")
        refused(fn, (pset._h, None, p, p, *m, None, r, r), w + "null batch")
        refused(fn, (pset._h, unplanned._h, p, p, *m, None, r, r),
                w + "the batch carries no plan indices (create it with slime_rs_batch_create_planned)")
        refused(fn, (pset._h, three._h, p, p, *m, None, r, r),
                w + "the batch was created for 3 plans of k = 4 on device 0, the set has 2 plans of k = 4 on device 0")
        # max_rows < 2 and k + max_rows > 63 come before the null checks
        refused(fn, (one._h, b1._h, None, None, *m, None, None, None),
                w + "no plan of the set has more than 1 row: one parity row cannot tell which shard is wrong")
        refused(fn, (wide._h, b40._h, None, None, *m, None, None, None),
                w + "k + max_rows = 64 exceeds 63 (a wave's tally keeps one slot per lane)")
        refused(fn, (pset._h, batch._h, None, p, *m, None, None, r), w + "null result array")
        refused(fn, (pset._h, batch._h, p, p, *m, None, r, None), w + "null result array")
        refused(fn, (pset._h, batch._h, None, p, *m, None, r, r), w + "null buffer")
        refused(fn, (pset._h, batch._h, p, None, *m, None, r, r), w + "null buffer")
    refused(byt, (pset._h, batch._h, None, p, None, None, r, r), "planset_locate_objects_batch: null buffer")
    refused(byt, (pset._h, batch._h, p, p, None, None, r, r), "planset_locate_objects_batch: null mapping")
    with pytest.raises(ValueError, match="carries no plan indices"):
        pset.locate_batch(buf, buf, unplanned)
    with pytest.raises(ValueError, match="batch is for 3 plans"):
        pset.locate_batch(buf, buf, three)
    with pytest.raises(ValueError, match="addresses element"):
        pset.locate_batch(buf, buf[:-6].contiguous(), batch)
    with pytest.raises(N.NativeError, match="one parity row"):
        one.locate_batch(buf, buf, b1)
    torch.cuda.synchronize()
    assert (res == GARBAGE).all(), "a refused call touches nothing"
    assert_results(host(torch, pset.locate_batch(buf, buf, batch)), SR.clean_results(2, 4, 2))
    # nobj == 0 touches nothing
    none = D.Batch([], 4, plans=[], nplans=2)
    assert sym(pset._h, none._h, p, p, None, r, r, None) == 0
    torch.cuda.synchronize()
    assert (res == GARBAGE).all()
    c, f = pset.locate_batch(buf, buf, none)
    assert c.shape == f.shape == (0, 7)


# ------------------------------------------------------------------ 11. the loop closes

def test_scrub_locate_repair_of_degraded_objects(torch_dev):
    """for_scrub -> planned Batch -> verify_batch -> locate_batch(filter) -> erasures_from_set_counts
    (with what was already missing) -> PlanSet.for_erasures -> a new planned Batch -> execute_batch
    in place: every shard of every object equals the oracle's codeword again, rebuilt data shards
    as the oracle's recover_data returns them, untouched objects bit for bit."""
    torch = torch_dev
    from slime_amd import device as D
    need, total = 8, 12
    T, C = geometry(need)
    lengths = [T + 5, 3, C * T + 1, 0, 260, 7, 2 * T, 64, 1030, 4, T - 1, 513]
    missing = [(), (0,), (3, 11), (5,), (), (8,), (1, 2), (), (10, 11), (7,), (0, 9), ()]
    corrupt = {1: 5, 2: 0, 5: 11, 6: 9, 8: 4, 10: 3, 11: 6}  # object: a further survivor, wrong in several columns
    rng = np.random.default_rng(3167)
    places, size = packed_spans(lengths, total, 1, start=3)
    original = np.full(size + 5, 0x5EA15EA1, dtype=np.uint32)
    for place, L in zip(places, lengths):
        if L:
            word = np.zeros((total, L), dtype=np.uint32)
            word[:need] = rng.integers(0, P, size=(need, L), dtype=np.uint64).astype(np.uint32)  # canonical, as ingested
            OC.encode_object(word, need, total)
            for s in range(total):
                shard(original, place, s, L)[:] = word[s]
    h = original.copy()
    blank(h, places, lengths, missing)
    expect = []
    for o, L in enumerate(lengths):
        bad = set(missing[o])
        if o in corrupt and L:
            s = corrupt[o]
            assert s not in bad
            for c in sorted(set(int(c) for c in rng.integers(0, L, size=3))):
                plant(h, places[o], L, s, c, rng.integers(0, 2**32), s in scrub_rows(need, total, missing[o])[1])
            bad.add(s)
        expect.append(sorted(bad))
    pset, plan_of, plans = scrub_set(need, total, missing)
    batch = planned_batch(lengths, places, need, plan_of, pset.nplans)
    buf = to_dev(torch, h)
    mism, _ = pset.verify_batch(buf, buf, batch)
    counts, first = pset.locate_batch(buf, buf, batch, filter=mism)
    exp = set_reference(plans, plan_of, pset.max_rows, h, places, lengths)
    assert_results(host(torch, (counts, first)), exp)
    assert int(counts[:, need + pset.max_rows].sum()) == 0, "nothing unlocated"
    erasures = D.erasures_from_set_counts(counts, pset, plan_of, missing)
    assert erasures == expect
    assert max(len(e) for e in erasures) == 3
    rset, rplan_of = D.PlanSet.for_erasures(need, total, erasures)
    rbatch = planned_batch(lengths, places, need, rplan_of, rset.nplans)
    rset.execute_batch(buf, buf, rbatch)
    got = to_host(torch, buf)
    for o, (place, L) in enumerate(zip(places, lengths)):
        for s in range(total):
            assert np.array_equal(shard(got, place, s, L), shard(original, place, s, L)), (o, s)
        rebuilt = [s for s in erasures[o] if s < need]
        if rebuilt and L:
            have = [s for s in range(total) if s not in erasures[o]][:need]
            rc, data = OC.recover_data([np.ascontiguousarray(shard(h, place, s, L)) for s in have], have)
            assert rc == 0
            for s in rebuilt:
                assert np.array_equal(shard(got, place, s, L), data[s]), (o, s)
        if not erasures[o]:
            assert rplan_of[o] == N.NO_PLAN
    assert np.array_equal(got, original), "guard words and untouched objects bit for bit"
    full, full_of, _ = scrub_set(need, total, [()] * len(lengths))
    m2, f2 = full.verify_batch(buf, buf, planned_batch(lengths, places, need, full_of, 1))
    torch.cuda.synchronize()
    assert int(m2.sum()) == 0 and bool((f2 == -1).all())
