"""Ragged locate (slime_rs_plan_locate_batch, slime_rs_locate_objects_batch) on the
GPU: after a scrub, one launch that names the wrong shard of every column.

Every expectation comes from tests/locate_ref.py on host copies (the rule over
oracle_c.apply_matrix rows; pinned to the C++ rule by test_locate_host.py), never
from a kernel.  Result arrays are pre-filled with garbage, so every launch also
proves the initialisation; data buffers are compared with their host copies
afterwards, so every launch also proves that locate wrote nothing but results.
Shapes are test_gpu_ragged_verify's: the boundary lengths of a vector, a wave, a
tile, a unit and a ticket group plus verify's step boundaries.
"""
import ctypes

import numpy as np
import pytest

import locate_ref as R
from slime_amd import _native as N
from test_gpu_ragged import (CODES, EDGES, P, encode_case, encode_plan, geometry, in_place_batch, mode,  # noqa: F401
                             shard, to_dev, to_host, torch_dev)
from test_gpu_ragged_verify import assert_results, flip_positions, host, verify_lengths
from test_gpu_verify import GARBAGE

pytestmark = pytest.mark.gpu

LOCATE_CODES = [c for c in CODES if c != (1, 2)]


def raw_locate(torch, plan, batch, src, cmp, filter=None, mapping=None, stream=None, src_off_bytes=0, cmp_off_bytes=0):
    """The C entry point into result arrays pre-filled with garbage (bytes form when mapping is given)."""
    from slime_amd import device as D
    n = plan.k + plan.rows + 1
    counts = torch.full((batch.nobj, n), GARBAGE, dtype=torch.int64, device="cuda")
    first = torch.full((batch.nobj, n), GARBAGE, dtype=torch.int64, device="cuda")
    f = ctypes.c_void_p(filter.data_ptr()) if filter is not None else None
    tail = (f, ctypes.c_void_p(counts.data_ptr()), ctypes.c_void_p(first.data_ptr()), D._stream_handle(0, stream))
    a, b = ctypes.c_void_p(src.data_ptr() + src_off_bytes), ctypes.c_void_p(cmp.data_ptr() + cmp_off_bytes)
    if mapping is None:
        N.check(N.lib.slime_rs_plan_locate_batch(plan._h, batch._h, a, b, *tail))
    else:
        N.check(N.lib.slime_rs_locate_objects_batch(plan._h, batch._h, a, b, ctypes.c_void_p(mapping.data_ptr()), *tail))
    return counts, first


def reference(need, total, h, places, lengths, skip=()):
    coeff = R.OC.parity_matrix(need, total - need)[need:]
    return R.locate_batch(coeff, list(range(need)), list(range(need, total)), h, places, h, places, lengths, skip)


def plant(h, place, L, s, col, value, data):
    """Store `value` (moved on until it differs from what is there: bit-different for a parity
    shard, different mod p for a data shard, whose aliases are not errors)."""
    w = shard(h, place, s, L)
    v, old = int(value), int(w[col])
    while (v % P == old % P) if data else (v == old):
        v = (v + 1) & 0xFFFFFFFF
    w[col] = v


def planted_words(seed):
    rng = np.random.default_rng(seed)
    return np.concatenate([EDGES, rng.integers(0, 2**32, size=22, dtype=np.uint64).astype(np.uint32)])


# ------------------------------------------------------------------ 1. clean data

@pytest.mark.parametrize("align", [1, 64])
@pytest.mark.parametrize("need,total", LOCATE_CODES)
def test_clean_every_boundary_length(torch_dev, need, total, align):
    torch = torch_dev
    rows = total - need
    lengths = verify_lengths(need, rows)
    np.random.default_rng(need * 41 + total).shuffle(lengths)
    _, want, places, _ = encode_case(need, total, lengths, align, seed=need * 3001 + total)
    batch = in_place_batch(lengths, places, need)
    plan = encode_plan(need, total)
    exp = reference(need, total, want, places, lengths)
    assert_results(exp, R.clean_results(len(lengths), need, rows), "the reference finds oracle codewords clean")
    buf = to_dev(torch, want)
    assert_results(host(torch, raw_locate(torch, plan, batch, buf, buf)), exp)
    c, f = plan.locate_batch(buf, buf, batch)
    assert c.shape == f.shape == (len(lengths), total + 1) and c.dtype == f.dtype == torch.int64
    assert_results(host(torch, (c, f)), exp)
    assert np.array_equal(to_host(torch, buf), want), "locate writes nothing but its results"


# ------------------------------------------------------------------ 2. one wrong word per object

def one_word_rounds(need, total, seed):
    """Round p plants, in every object that has a p-th flip position, one word at that position in
    shard (o + p) % total: [(host buffer, planted (counts, first))]."""
    rows = total - need
    lengths = verify_lengths(need, rows)
    _, want, places, _ = encode_case(need, total, lengths, 1, seed=seed)
    pos = [flip_positions(L, need, rows) for L in lengths]
    words = planted_words(seed)
    out = []
    for p in range(max(len(q) for q in pos)):
        h = want.copy()
        ec, ef = R.clean_results(len(lengths), need, rows)
        for o, (L, q) in enumerate(zip(lengths, pos)):
            if p < len(q):
                s = (o + p) % total
                plant(h, places[o], L, s, q[p], words[(3 * o + p) % len(words)], s < need)
                ec[o, s], ef[o, s] = 1, q[p]
        out.append((h, (ec, ef)))
    return lengths, places, out


@pytest.mark.parametrize("need,total", LOCATE_CODES)
def test_one_wrong_word_per_object(torch_dev, need, total):
    """Exactly the planted (object, slot) reports count 1 and the planted column, over every flip
    position, every shard as the slot, planted words from EDGES and random values.  17/20 and 33/50
    take the column form."""
    torch = torch_dev
    lengths, places, rounds = one_word_rounds(need, total, seed=need * 3011 + total)
    batch = in_place_batch(lengths, places, need)
    plan = encode_plan(need, total)
    assert plan.locate_slots() == list(range(total))
    buf = to_dev(torch, rounds[0][0])
    for p, (h, planted) in enumerate(rounds):
        exp = reference(need, total, h, places, lengths)
        assert_results(exp, planted, ("the reference names the planted slot", p))
        buf.copy_(to_dev(torch, h))
        assert_results(host(torch, raw_locate(torch, plan, batch, buf, buf)), exp, p)
        assert np.array_equal(to_host(torch, buf), h)


def test_every_schedule_and_pipeline_mode_gives_the_same_results(torch_dev, mode):
    torch = torch_dev
    need, total = 8, 12
    lengths, places, rounds = one_word_rounds(need, total, seed=need * 3011 + total)
    h, planted = rounds[1]
    buf = to_dev(torch, h)
    got = raw_locate(torch, encode_plan(need, total), in_place_batch(lengths, places, need), buf, buf)
    assert_results(host(torch, got), reference(need, total, h, places, lengths))


# ------------------------------------------------------------------ 3, 4. two wrong shards

@pytest.mark.parametrize("need,total", [(3, 5), (8, 12), (16, 20), (17, 20)])
def test_two_shards_wrong_in_different_columns(torch_dev, need, total):
    torch = torch_dev
    rows = total - need
    T, C = geometry(need)
    lengths = [C * T + 7, 260, 2 * T + 2, 6]
    _, want, places, _ = encode_case(need, total, lengths, 1, seed=need * 3023 + total)
    h = want.copy()
    ec, ef = R.clean_results(len(lengths), need, rows)
    for o, L in enumerate(lengths):
        a, b = o % need, need + (o + 1) % rows  # a data shard and a parity shard
        ca, cb = (L - 1, 0) if o % 2 else (1, L - 2)
        plant(h, places[o], L, a, ca, 0x1234 + o, True)
        plant(h, places[o], L, b, cb, P + o, False)
        ec[o, a], ef[o, a], ec[o, b], ef[o, b] = 1, ca, 1, cb
    o, L = 0, lengths[0]  # and two data shards, both named
    plant(h, places[o], L, 1, T, 5, True)
    plant(h, places[o], L, 2, T + 1, 6, True)
    assert ec[o, 1] == ec[o, 2] == 0  # object 0's first pair is shard 0 and a parity shard
    ec[o, 1], ef[o, 1], ec[o, 2], ef[o, 2] = 1, T, 1, T + 1
    exp = reference(need, total, h, places, lengths)
    assert (exp[0][:, total] == 0).all() and (exp[0][:, :total].sum(axis=1) >= 2).all()
    assert np.array_equal(exp[0], ec), "the reference names both planted shards"
    buf = to_dev(torch, h)
    batch = in_place_batch(lengths, places, need)
    assert_results(host(torch, raw_locate(torch, encode_plan(need, total), batch, buf, buf)), exp)


@pytest.mark.parametrize("need,total", [(3, 5), (8, 12), (10, 14), (33, 50)])
def test_two_shards_wrong_in_the_same_column_are_unlocated(torch_dev, need, total):
    """Beyond what `rows` syndromes decide: the result is the reference's, and for these seeds the
    reference says unlocated (a third shard is blamed with probability about k / p)."""
    torch = torch_dev
    rows = total - need
    T, _ = geometry(need)
    lengths = [T + 9, 7, 516]
    _, want, places, _ = encode_case(need, total, lengths, 1, seed=need * 3037 + total)
    h = want.copy()
    rng = np.random.default_rng(need + total)
    cols = []
    for o, L in enumerate(lengths):
        col = [L - 1, 2, 257][o]
        pairs = [(0, need - 1), (1 % need, need), (need, total - 1)][o]  # data+data, data+parity, parity+parity
        for s in pairs:
            plant(h, places[o], L, s, col, rng.integers(0, 2**32), s < need)
        cols.append(col)
    exp = reference(need, total, h, places, lengths)
    for o, col in enumerate(cols):
        want_c = np.zeros(total + 1, dtype=np.int64)
        want_c[total] = 1
        assert np.array_equal(exp[0][o], want_c) and exp[1][o, total] == col, "the reference says unlocated"
    buf = to_dev(torch, h)
    batch = in_place_batch(lengths, places, need)
    assert_results(host(torch, raw_locate(torch, encode_plan(need, total), batch, buf, buf)), exp)


# ------------------------------------------------------------------ 5. a whole shard, objects without work

@pytest.mark.parametrize("need,total", [(3, 5), (8, 12), (16, 20), (17, 20)])
def test_whole_shard_replaced_and_objects_without_work(torch_dev, need, total):
    """Every word of one shard XOR 1 in a multi-unit object: that slot counts L from column 0, for
    a data shard and for a parity shard.  A planned SLIME_RS_NO_PLAN neighbour (damaged too) and an
    L == 0 neighbour keep the initial values."""
    torch = torch_dev
    from slime_amd import device as D
    rows = total - need
    T, C = geometry(need)
    L = 2 * C * T + T + 6
    lengths = [L, L, 0, L]
    _, want, places, _ = encode_case(need, total, lengths, 1, seed=need * 3041 + total)
    h = want.copy()
    hit = [need - 1, need + 1, None, 0]
    for o, s in enumerate(hit):
        if s is not None:
            shard(h, places[o], s, L)[:] ^= np.uint32(1)
    exp = reference(need, total, h, places, lengths, skip=(3,))
    ec, ef = R.clean_results(4, need, rows)
    ec[0, hit[0]], ef[0, hit[0]], ec[1, hit[1]], ef[1, hit[1]] = L, 0, L, 0
    assert_results(exp, (ec, ef), "the reference blames the replaced shard in every column")
    spans = [(off, ss, off, ss, n) for (off, ss), n in zip(places, lengths)]
    batch = D.Batch(spans, need, plans=[0, 0, 0, N.NO_PLAN], nplans=1)
    assert batch.units >= 6
    buf = to_dev(torch, h)
    assert_results(host(torch, raw_locate(torch, encode_plan(need, total), batch, buf, buf)), exp)
    assert np.array_equal(to_host(torch, buf), h)


# ------------------------------------------------------------------ 6. the filter

@pytest.mark.parametrize("need,total", [(3, 5), (8, 12), (17, 20)])
def test_filter_skips_clean_objects_on_the_device(torch_dev, need, total):
    torch = torch_dev
    rows = total - need
    T, C = geometry(need)
    lengths = [C * T + 5, 3, T + 1, 0, 2 * C * T + 2, 257, 6, T]
    _, want, places, _ = encode_case(need, total, lengths, 1, seed=need * 3049 + total)
    h = want.copy()
    dirty = {0: (0, 5), 2: (need, T), 5: (need - 1, 256), 6: (total - 1, 5)}  # object: (shard, column)
    for o, (s, col) in dirty.items():
        plant(h, places[o], lengths[o], s, col, 77 + o, s < need)
    full = reference(need, total, h, places, lengths)
    assert sorted(np.flatnonzero(full[0].sum(axis=1))) == sorted(dirty)
    plan = encode_plan(need, total)
    batch = in_place_batch(lengths, places, need)
    buf = to_dev(torch, h)
    mism, _ = plan.verify_batch(buf, buf, batch)
    got = raw_locate(torch, plan, batch, buf, buf, filter=mism)
    assert sorted(np.flatnonzero(mism.cpu().numpy().sum(axis=1))) == sorted(dirty)
    assert_results(host(torch, got), full, "dirty objects as with filter=None, clean ones at their initial values")
    assert_results(host(torch, plan.locate_batch(buf, buf, batch, filter=mism)), full)
    assert_results(host(torch, raw_locate(torch, plan, batch, buf, buf)), full)
    # a hand-made filter that clears dirty objects: the skip is the device's, whatever the data says
    hand = mism.clone()
    hand[0] = 0
    hand[5] = 0
    hand[1, 0] = 9  # a clean object the filter calls dirty is scanned, and found clean
    cleared = reference(need, total, h, places, lengths, skip=(0, 5))
    assert cleared[0][0].sum() == 0 and cleared[0][2].sum() == 1
    assert_results(host(torch, raw_locate(torch, plan, batch, buf, buf, filter=hand)), cleared)
    assert np.array_equal(to_host(torch, buf), h)


# ------------------------------------------------------------------ 7. bytes

def to_chunks(h, places, lengths, total, ms):
    """The symbol buffer as stored chunk bytes: word = BE(symbol ^ mapping[o])."""
    b = h.copy()
    for (off, ss), L, m in zip(places, lengths, ms):
        if L:
            b[off: off + (total - 1) * ss + L] ^= np.uint32(m)
    return b.byteswap().view(np.uint8)


@pytest.mark.parametrize("need,total", [(3, 5), (8, 12), (16, 20), (17, 20)])
def test_bytes_match_the_symbol_reference(torch_dev, need, total):
    """Cases 2, 3 and 5 through slime_rs_locate_objects_batch with a mapping per object (0, 1 << 31
    and random values): the results equal the symbol reference on the unpacked symbols."""
    torch = torch_dev
    from slime_amd import device as D
    rows = total - need
    lengths, places, rounds = one_word_rounds(need, total, seed=need * 3011 + total)
    rng = np.random.default_rng(need * 7 + total)
    ms = [[0, 1 << 31, int(rng.integers(0, 2**32))][o % 3] for o in range(len(lengths))]
    mt = to_dev(torch, np.array(ms, dtype=np.uint32))
    batch = in_place_batch(lengths, places, need)
    plan = encode_plan(need, total)
    for p in (0, 1, len(rounds) - 1):  # column 0, the last whole vector, the last flip position
        h = rounds[p][0]
        hb = to_chunks(h, places, lengths, total, ms)
        buf = torch.from_numpy(hb.copy()).cuda()
        exp = reference(need, total, h, places, lengths)
        assert exp[0].sum() >= 1
        assert_results(host(torch, raw_locate(torch, plan, batch, buf, buf, mapping=mt)), exp, p)
        assert_results(host(torch, D.locate_objects_batch(plan, buf, buf, batch, mt)), exp, p)
        assert np.array_equal(buf.cpu().numpy(), hb)
    # two shards in different columns, and a whole shard replaced, in one buffer
    T, C = geometry(need)
    L = C * T + T + 6
    lens = [L, 9, L, 0]
    _, want, pl, _ = encode_case(need, total, lens, 1, seed=need * 3061 + total)
    h = want.copy()
    plant(h, pl[1], 9, 0, 8, P + 1, True)
    plant(h, pl[1], 9, total - 1, 3, 0xFFFFFFFF, False)
    shard(h, pl[0], need - 1, L)[:] ^= np.uint32(1)
    shard(h, pl[2], need, L)[:] ^= np.uint32(1)
    ms = [0xDEADBEEF, 1 << 31, 0, 5]
    exp = reference(need, total, h, pl, lens)
    assert exp[0][0, need - 1] == L and exp[0][2, need] == L and exp[0][1].sum() == 2 and exp[0][:, total].sum() == 0
    hb = to_chunks(h, pl, lens, total, ms)
    buf = torch.from_numpy(hb.copy()).cuda()
    mt = to_dev(torch, np.array(ms, dtype=np.uint32))
    b2 = in_place_batch(lens, pl, need)
    mism, _ = D.verify_objects_batch(plan, buf, buf, b2, mt)
    assert_results(host(torch, raw_locate(torch, plan, b2, buf, buf, mapping=mt)), exp)
    assert_results(host(torch, raw_locate(torch, plan, b2, buf, buf, mapping=mt, filter=mism)), exp)
    assert np.array_equal(buf.cpu().numpy(), hb)


# ------------------------------------------------------------------ 8. the column form by alignment

@pytest.mark.parametrize("need,total", [(4, 6), (8, 12)])
@pytest.mark.parametrize("src_off,cmp_off", [(2, 0), (0, 2), (2, 2)])
def test_bases_not_word_aligned_take_the_column_form(torch_dev, need, total, src_off, cmp_off):
    torch = torch_dev
    lengths, places, rounds = one_word_rounds(need, total, seed=need * 3011 + total)
    h = rounds[2][0]
    exp = reference(need, total, h, places, lengths)
    assert exp[0].sum() >= 4

    def shifted(a, off):
        b = np.full(a.size * 4 + 8, 0xA5, dtype=np.uint8)
        b[off: off + a.size * 4] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        return torch.from_numpy(b).cuda()

    src, cmp = shifted(h, src_off), shifted(h, cmp_off)
    got = raw_locate(torch, encode_plan(need, total), in_place_batch(lengths, places, need), src, cmp,
                     src_off_bytes=src_off, cmp_off_bytes=cmp_off)
    assert_results(host(torch, got), exp)


# ------------------------------------------------------------------ 9. capture and streams

@pytest.mark.parametrize("need,total", [(4, 6), (17, 20)])
def test_captured_scrub_and_locate_chain_reports_the_current_damage(torch_dev, need, total):
    """verify_batch then locate_batch(filter=mismatches) captured as one chain on a non-default
    stream and replayed three times with the damage changed in between."""
    torch = torch_dev
    rows = total - need
    T, C = geometry(need)
    lengths = [4 * C * T + 5, 3, T + 1, 0, 256, C * T]
    _, want, places, _ = encode_case(need, total, lengths, 1, seed=need * 3067 + total)
    batch = in_place_batch(lengths, places, need)
    plan = encode_plan(need, total)
    buf = to_dev(torch, want)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm the launch paths outside the capture, on the stream itself
        m0, _ = plan.verify_batch(buf, buf, batch, stream=s)
        res = raw_locate(torch, plan, batch, buf, buf, filter=m0, stream=s)
    s.synchronize()
    assert_results(host(torch, res), R.clean_results(len(lengths), need, rows))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        gm, _ = plan.verify_batch(buf, buf, batch, stream=s)
        gc, gf_ = plan.locate_batch(buf, buf, batch, filter=gm, stream=s)
    torch.cuda.synchronize()
    damage = [[(0, 0, 9)], [(2, need, T), (4, need - 1, 255)], []]  # per replay: (object, shard, column)
    for rnd, todo in enumerate(damage):
        h = want.copy()
        for o, sh, col in todo:
            plant(h, places[o], lengths[o], sh, col, 31 + rnd, sh < need)
        buf.copy_(to_dev(torch, h))
        gc.fill_(GARBAGE)
        gf_.fill_(GARBAGE)
        torch.cuda.synchronize()
        g.replay()
        exp = reference(need, total, h, places, lengths)
        assert int(exp[0].sum()) == len(todo)
        assert_results(host(torch, (gc, gf_)), exp, rnd)
    del g  # before the batch: the graph's kernel nodes read its tables
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 10. errors

def test_refusals_and_the_launched_mark(torch_dev):
    torch = torch_dev
    from slime_amd import device as D
    lengths = [16, 5]
    _, want, places, _ = encode_case(4, 6, lengths, 1, seed=3071)
    buf = to_dev(torch, want)
    batch = in_place_batch(lengths, places, 4)
    plan = D.Plan.encode(4, 6).set_outputs([4, 5])
    res = torch.full((2 * 7,), GARBAGE, dtype=torch.int64, device="cuda")
    p, r = ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(res.data_ptr())
    sym, byt = N.lib.slime_rs_plan_locate_batch, N.lib.slime_rs_locate_objects_batch

    def refused(fn, args, text):
        assert fn(*args, None) == N.ERR_INVALID_ARG
        assert N.lib.slime_rs_last_error().decode() == text

    w = "plan_locate_batch: "
    refused(sym, (None, batch._h, p, p, None, r, r), w + "null plan")
    refused(sym, (plan._h, None, p, p, None, r, r), w + "null batch")
    refused(sym, (plan._h, batch._h, None, p, None, r, r), w + "null buffer")
    refused(sym, (plan._h, batch._h, p, None, None, r, r), w + "null buffer")
    refused(sym, (plan._h, batch._h, p, p, None, None, r), w + "null result array")
    refused(sym, (plan._h, batch._h, p, p, None, r, None), w + "null result array")
    w = "locate_objects_batch: "
    refused(byt, (None, batch._h, p, p, p, None, r, r), w + "null plan")
    refused(byt, (plan._h, None, p, p, p, None, r, r), w + "null batch")
    refused(byt, (plan._h, batch._h, None, p, p, None, r, r), w + "null buffer")
    refused(byt, (plan._h, batch._h, p, p, None, None, r, r), w + "null mapping")
    refused(byt, (plan._h, batch._h, p, p, p, None, None, r), w + "null result array")
    # one parity row; more slots than a wave has lanes; a plan of another k
    one, b1 = D.Plan.encode(1, 2), D.Batch([(0, 4, 0, 4, 4)], 1)
    text = "the plan has 1 row: one parity row cannot tell which shard is wrong"
    refused(sym, (one._h, b1._h, p, p, None, r, r), "plan_locate_batch: " + text)
    refused(byt, (one._h, b1._h, p, p, p, None, r, r), "locate_objects_batch: " + text)
    wide, b40 = D.Plan.encode(40, 64), D.Batch([(0, 1, 0, 1, 1)], 40)
    text = "k + rows = 64 exceeds 63 (a wave's tally keeps one slot per lane)"
    refused(sym, (wide._h, b40._h, p, p, None, r, r), "plan_locate_batch: " + text)
    refused(byt, (wide._h, b40._h, p, p, p, None, r, r), "locate_objects_batch: " + text)
    other = D.Plan.encode(5, 7)
    refused(sym, (other._h, batch._h, p, p, None, r, r), "plan_locate_batch: the batch was created for k = 4 on device 0, "
                                                        "the plan has k = 5 on device 0")
    with pytest.raises(ValueError, match="batch is for k"):
        other.locate_batch(buf, buf, batch)
    with pytest.raises(ValueError, match="addresses element"):
        plan.locate_batch(buf, buf[:-6].contiguous(), batch)
    with pytest.raises(N.NativeError, match="one parity row"):
        one.locate_batch(buf, buf, b1)
    torch.cuda.synchronize()
    assert (res == GARBAGE).all(), "a refused call touches nothing"
    plan.set_outputs([4, 5])  # refusals do not mark the plan
    assert_results(host(torch, plan.locate_batch(buf, buf, batch)), R.clean_results(2, 4, 2))
    with pytest.raises(N.NativeError, match="already launched"):
        plan.set_outputs([0, 1])
    # nobj == 0 touches nothing
    none = D.Batch([], 4)
    assert sym(plan._h, none._h, p, p, None, r, r, None) == 0
    torch.cuda.synchronize()
    assert (res == GARBAGE).all()
    c, f = plan.locate_batch(buf, buf, none)
    assert c.shape == f.shape == (0, 7)


# ------------------------------------------------------------------ 11. end to end

@pytest.mark.parametrize("need,total", [(3, 5), (8, 12)])
def test_scrub_locate_repair_restores_every_object(torch_dev, need, total):
    """Encode, damage one or two shards (data and parity) in a third of the objects, then
    verify_batch -> locate_batch -> erasures_from_counts -> PlanSet.for_erasures with a planned
    Batch -> PlanSet.execute_batch: the buffer equals the original bit for bit and a second
    verify_batch is clean."""
    torch = torch_dev
    from slime_amd import device as D
    rows = total - need
    T, C = geometry(need)
    lengths = [T + 5, 3, C * T + 1, 0, 260, 7, 2 * T, 64, 1030, 4, T - 1, 513]
    init, _, places, _ = encode_case(need, total, lengths, 1, seed=need * 3079 + total)
    batch = in_place_batch(lengths, places, need)
    plan = encode_plan(need, total)
    # A repair writes canonical residues, so a data word stored at or above p would not come back
    # bit for bit: the objects' data is canonical, as an ingest stores it.
    start = init.copy()
    for place, L in zip(places, lengths):
        for s_ in range(need):
            shard(start, place, s_, L)[:] %= np.uint32(P)
    buf = to_dev(torch, start)
    plan.execute_batch(buf, buf, batch)
    original = to_host(torch, buf).copy()
    assert reference(need, total, original, places, lengths)[0].sum() == 0
    h = original.copy()
    rng = np.random.default_rng(need)
    expect = [[] for _ in lengths]
    for o in range(0, len(lengths), 3):  # a third of the objects (one of them is empty)
        L = lengths[o]
        if L == 0:
            continue
        # a data shard; a parity shard; a data and a parity shard in columns of their own
        hit = [[(o + 1) % need], [need + o % rows], [o % need, need + o % rows]][(o // 3) % 3 if L > 1 else 0]
        cols = [int(c) for c in rng.permutation(L)]
        for c in cols[:min(2, L - (len(hit) - 1))]:
            plant(h, places[o], L, hit[0], c, rng.integers(0, 2**32), hit[0] < need)
        if len(hit) == 2:
            plant(h, places[o], L, hit[1], cols[-1], rng.integers(0, 2**32), False)
        expect[o] = sorted(hit)
    assert sorted(len(e) for e in expect if e) == [1, 1, 2]
    buf.copy_(to_dev(torch, h))
    mism, _ = plan.verify_batch(buf, buf, batch)
    counts, first = plan.locate_batch(buf, buf, batch, filter=mism)
    assert_results(host(torch, (counts, first)), reference(need, total, h, places, lengths))
    assert int(counts[:, total].sum()) == 0, "nothing unlocated"
    erasures = D.erasures_from_counts(counts, plan.locate_slots())
    assert erasures == expect
    pset, plan_of = D.PlanSet.for_erasures(need, total, erasures)
    spans = [(off, ss, off, ss, L) for (off, ss), L in zip(places, lengths)]
    planned = D.Batch(spans, need, plans=plan_of, nplans=pset.nplans)
    pset.execute_batch(buf, buf, planned)
    assert np.array_equal(to_host(torch, buf), original), "repaired bit for bit"
    m2, f2 = plan.verify_batch(buf, buf, batch)
    torch.cuda.synchronize()
    assert int(m2.sum()) == 0 and bool((f2 == -1).all())
