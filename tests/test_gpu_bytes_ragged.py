"""Ragged byte objects on the GPU: slime_rs_decode_objects_batch,
slime_rs_planset_decode_objects_batch, slime_rs_verify_objects_batch and
slime_rs_planset_verify_objects_batch -- the ragged launches over stored chunk
BYTES, each object with its own mapping value.

Every expectation comes from the C oracle and numpy on host copies, never from
a kernel under test.  Stored objects are built on the host: symbols
(test_gpu_ragged.symbols), OC.encode_object, chunk bytes = (word ^ m).byteswap()
(`stored`).  Expected decode outputs are OC.apply_matrix over the plan's
coefficient rows on byteswap(bytes) ^ m, XOR-ed with m and swapped back -- for
codewords that is `stored` of the symbol-domain expectation the symbol suites
already compute (repair_case, encode_case).  Verify expectations are the
oracle's rows against the stored rows in the symbol view (expect_batch): a
column mismatches iff BE(stored) != computed ^ m iff BE(stored) ^ m != computed.
Buffers are sentinel-filled and compared whole, result arrays are pre-filled
with garbage.  References are computed once per shape and shared by the
schedule / pipeline modes.
"""
import ctypes

import numpy as np
import pytest

from oracle import oracle_c as OC
from slime_amd import _native as N
from test_gpu_planset import PATTERNS, cycle, make_set, planned_batch, repair_case, survivors
from test_gpu_ragged import (P, SENTINEL, boundary_lengths, encode_case, geometry, in_place_batch,  # noqa: F401
                             mode, packed_spans, shard, symbols, torch_dev)
from test_gpu_ragged_verify import (assert_results, clean_results, expect_batch, flip_positions, host,
                                    matrix_case, verify_lengths)
from test_gpu_schedule import _held_settles
from test_gpu_verify import GARBAGE

pytestmark = pytest.mark.gpu

CODES = [(1, 2), (3, 5), (8, 12), (16, 20), (17, 20), (33, 50)]
# One erasure pattern per code for the single-plan repairs: data and parity targets.
ERASE = {(1, 2): (0,), (3, 5): (1, 4), (8, 12): (0, 3, 8, 11), (16, 20): (0, 5, 16, 19), (17, 20): (0, 16, 19),
         (33, 50): (0, 9, 32, 33, 49)}


def mappings(n, seed=0):
    """n mapping values cycling over 0, 1<<31, 0xFFFFFFFF and a seeded random word: neighbouring
    objects always differ."""
    r = int(np.random.default_rng(1000 + seed).integers(1, 2**31))  # none of the other three
    base = [0, 1 << 31, 0xFFFFFFFF, r]
    return np.array([base[o % 4] for o in range(n)], dtype=np.uint32)


def stored(sym, places, lengths, nshards, ms):
    """The chunk bytes of a symbol-domain buffer (as uint32 words in memory order): every object's
    words XOR-ed with its mapping and byte-swapped; the words between objects are left alone.
    Its own inverse."""
    out = np.array(sym, dtype=np.uint32)
    for place, L, m in zip(places, lengths, ms):
        for s in range(nshards):
            v = shard(out, place, s, L)
            v[:] = (v ^ np.uint32(m)).byteswap()
    return out


def unstored(b, places, lengths, nshards, ms):
    """The symbol view of chunk bytes: byteswap(bytes) ^ m."""
    out = np.array(b, dtype=np.uint32)
    for place, L, m in zip(places, lengths, ms):
        for s in range(nshards):
            v = shard(out, place, s, L)
            v[:] = v.byteswap() ^ np.uint32(m)
    return out


def bytes_dev(torch, a, shift=0):
    """The words of `a` as a uint8 device tensor whose base is `shift` bytes past an aligned address."""
    raw = np.ascontiguousarray(a, dtype=np.uint32).view(np.uint8)
    b = np.full(raw.size + 16, 0xA5, dtype=np.uint8)
    b[shift: shift + raw.size] = raw
    t = torch.from_numpy(b).cuda()
    assert t.data_ptr() % 16 == 0
    return t[shift: shift + raw.size]


def bytes_host(torch, t):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint32)


def map_dev(torch, ms):
    return torch.from_numpy(np.array(ms, dtype=np.uint32).view(np.int32)).cuda()


def assert_equal(got, want):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad.size, bad[:8], got[bad[:8]], want[bad[:8]])


def repair_plan(need, total, pat):
    """The in-place reconstruct plan of one erasure pattern: outputs are the erased chunks."""
    from slime_amd import device as D
    return D.Plan.reconstruct(need, total, survivors(need, total, pat), list(pat)).set_outputs(list(pat))


_stored = {}


def stored_repair_case(need, total, lengths, patterns, align, seed, ms):
    """repair_case in chunk bytes: (init, want, places).  init holds oracle-encoded objects with a
    sentinel in the erased chunks, want the same buffer with the erased chunks as the oracle
    rebuilds them -- OC.apply_matrix over the plan's rows on the survivors' symbols, which are
    byteswap(bytes) ^ m, then XOR-ed with m and swapped back.  Cached, read-only."""
    key = (need, total, tuple(lengths), tuple(patterns), align, seed, tuple(int(m) for m in ms))
    if key not in _stored:
        init, want, places, _ = repair_case(need, total, lengths, patterns, align, seed)
        a, b = stored(init, places, lengths, total, ms), stored(want, places, lengths, total, ms)
        a.setflags(write=False)
        b.setflags(write=False)
        _stored[key] = (a, b, places)
    return _stored[key]


def run_decode(torch, plan_or_set, batch, init, want, ms, stream=None):
    from slime_amd import device as D
    buf = bytes_dev(torch, init)
    D.decode_objects_batch(plan_or_set, buf, buf, batch, map_dev(torch, ms), stream=stream)
    assert_equal(bytes_host(torch, buf), want)


# ------------------------------------------------------------------ decode: lengths, guard bytes, mappings

@pytest.mark.parametrize("align", [1, 64])
@pytest.mark.parametrize("need,total", CODES)
def test_every_boundary_length_repaired_in_place(torch_dev, mode, need, total, align):
    """One batch of objects at every boundary length, shuffled, neighbouring objects with different
    mappings, repaired in place by ONE reconstruct plan whose outputs are the erased chunks.  The
    erased chunks hold a sentinel; the whole buffer is compared, so nothing outside the output
    chunks' 4L bytes is written."""
    pat = ERASE[(need, total)]
    lengths = boundary_lengths(need)
    np.random.default_rng(need * 131 + total).shuffle(lengths)
    ms = mappings(len(lengths), need)
    init, want, places = stored_repair_case(need, total, lengths, [pat] * len(lengths), align, need * 7 + total, ms)
    run_decode(torch_dev, repair_plan(need, total, pat), in_place_batch(lengths, places, need), init, want, ms)


@pytest.mark.parametrize("need,total", [(3, 5), (8, 12), (16, 20)])
def test_same_mapping_then_mappings_rotated_by_one(torch_dev, mode, need, total):
    """The batch above with one mapping for all objects, then with the cycling mappings rotated by
    one object: a kernel that keeps the walk's current mapping for the tile in flight passes the
    first run and fails the second."""
    pat = ERASE[(need, total)]
    lengths = boundary_lengths(need)
    np.random.default_rng(need * 131 + total).shuffle(lengths)
    n = len(lengths)
    plan = repair_plan(need, total, pat)
    for ms in (np.full(n, mappings(4, need)[3], dtype=np.uint32), np.roll(mappings(n, need), 1)):
        init, want, places = stored_repair_case(need, total, lengths, [pat] * n, 1, need * 7 + total, ms)
        run_decode(torch_dev, plan, in_place_batch(lengths, places, need), init, want, ms)


@pytest.mark.parametrize("need,total,nobj", [(3, 5, 1100), (8, 12, 1100), (16, 20, 4200)])
def test_waves_walk_units_of_different_objects(torch_dev, mode, need, total, nobj):
    """More one-unit objects (64 columns) than the static grid has waves, neighbours with
    different mappings AND different plans: every wave that takes a second unit stores a tile of
    one object after issuing the loads of another.  The mapping (and the plan) must be the stored
    tile's own.  The static walk gives wave w the objects w and w + waves: the mappings' cycle is
    shifted by one after `waves` objects, so that those two differ as neighbours do."""
    lengths = [64] * nobj
    waves = 4096 if need > 12 else 1024
    assert nobj > waves
    pats = cycle(PATTERNS[(need, total)], nobj)  # period 6 against the mappings' 4
    ms = mappings(4, need)[[(o + o // waves) % 4 for o in range(nobj)]]
    assert (ms[:-1] != ms[1:]).all() and (ms[:-waves] != ms[waves:]).all()
    init, want, places = stored_repair_case(need, total, lengths, pats, 1, 91 + need, ms)
    pset, plan_of = make_set(need, total, pats)
    batch = planned_batch(lengths, places, need, plan_of, pset.nplans)
    assert batch.units == nobj
    run_decode(torch_dev, pset, batch, init, want, ms)


@pytest.mark.parametrize("need,total", [(3, 5), (8, 12)])
def test_every_pipelined_tile_crosses_objects(torch_dev, mode, need, total):
    """Thirteen objects of exactly one tile with one plan and cycling mappings: whenever a wave
    takes two units in a row, the tile it stores and the tile it loads have different mappings."""
    T, _ = geometry(need)
    lengths = [T] * 13
    pat = ERASE[(need, total)]
    ms = mappings(13, need + 1)
    init, want, places = stored_repair_case(need, total, lengths, [pat] * 13, 64, 1300 + need, ms)
    run_decode(torch_dev, repair_plan(need, total, pat), in_place_batch(lengths, places, need), init, want, ms)


_noncanon = {}


def noncanonical_case(need, total):
    """Stored objects whose survivor chunks hold words that after ^ m equal p, p + 4 and
    0xFFFFFFFF (corrupt chunks), in a tail column, in the first vector and at tile boundaries; the
    expected erased chunks are the oracle's rows over exactly those symbols."""
    key = (need, total)
    if key not in _noncanon:
        from slime_amd import device as D
        pat = ERASE[key]
        have = survivors(need, total, pat)
        plan = D.Plan.reconstruct(need, total, have, list(pat))
        coeff = plan.coefficients()
        plan.close()
        T, C = geometry(need)
        lengths = [5, T + 6, 257, 3, C * T + 1]
        ms = mappings(len(lengths), 77)
        places, size = packed_spans(lengths, total, 1, start=3)
        rng = np.random.default_rng(need + 5)
        init = np.full(size + 5, SENTINEL, dtype=np.uint32)
        want = init.copy()
        bad = [P, P + 4, 0xFFFFFFFF]
        for o, (place, L) in enumerate(zip(places, lengths)):
            word = np.zeros((total, L), dtype=np.uint32)
            word[:need] = rng.integers(0, P, size=(need, L), dtype=np.uint64).astype(np.uint32)
            OC.encode_object(word, need, total)
            for n, c in enumerate(c for c in (0, 2, L - 1, 255, 256, T - 1, T, T + 4, C * T) if c < L):
                word[have[(o + n) % need], c] = bad[(o + n) % 3]
            out = OC.apply_matrix(coeff, [np.ascontiguousarray(word[s]) for s in have])
            for s in range(total):
                shard(init, place, s, L)[:] = 0xE7A5ED00 if s in pat else word[s]
                shard(want, place, s, L)[:] = out[pat.index(s)] if s in pat else word[s]
        _noncanon[key] = (lengths, places, ms, stored(init, places, lengths, total, ms),
                          stored(want, places, lengths, total, ms))
    return _noncanon[key]


@pytest.mark.parametrize("need,total", [(3, 5), (8, 12), (17, 20)])
def test_noncanonical_survivor_words(torch_dev, mode, need, total):
    lengths, places, ms, init, want = noncanonical_case(need, total)
    sym = unstored(init, places, lengths, total, ms)
    assert {int(x) for x in (P, P + 4, 0xFFFFFFFF)} <= {int(x) for x in sym[sym >= P]}
    run_decode(torch_dev, repair_plan(need, total, ERASE[(need, total)]), in_place_batch(lengths, places, need), init,
               want, ms)


# ------------------------------------------------------------------ decode: a separate dst, alignments

@pytest.mark.parametrize("need,total", [(3, 5), (8, 12)])
@pytest.mark.parametrize("src_shift,dst_shift", [(0, 0), (2, 0), (0, 2), (4, 4), (12, 4)])
def test_separate_dst_other_spans_and_unaligned_bases(torch_dev, mode, need, total, src_shift, dst_shift):
    """src holds the stored chunks packed with stride L; dst is another tensor that receives only
    the rebuilt chunks (plan outputs 0..rows-1), objects in reverse order behind a gap, odd chunk
    strides.  A base 2 bytes off a word boundary (src or dst) takes the column form; bases that are
    4-byte but not 16-byte aligned take the vector form."""
    torch = torch_dev
    from slime_amd import device as D
    pat = ERASE[(need, total)]
    have = survivors(need, total, pat)
    rows = len(pat)
    T, C = geometry(need)
    lengths = [T + 1, 0, 3, C * T + 5, 257, 4]
    ms = mappings(len(lengths), 5)
    _, full, src_places, _ = encode_case(need, total, lengths, 1, seed=177 + need)
    dst_places, off = [None] * len(lengths), 9
    for o in reversed(range(len(lengths))):
        ss = -(-lengths[o] // 8) * 8 + 1
        dst_places[o] = (off, ss)
        off += rows * ss + 3
    plan = D.Plan.reconstruct(need, total, have, list(pat))  # outputs 0..rows-1
    coeff = plan.coefficients()
    want = np.full(off + 4, SENTINEL, dtype=np.uint32)
    for sp, dp, L in zip(src_places, dst_places, lengths):
        if L:
            for i, r in enumerate(OC.apply_matrix(coeff, [np.ascontiguousarray(shard(full, sp, s, L)) for s in have])):
                shard(want, dp, i, L)[:] = r
    want = stored(want, dst_places, lengths, rows, ms)
    src_h = stored(full, src_places, lengths, total, ms)
    batch = D.Batch([(so, ss, do, ds, L) for (so, ss), (do, ds), L in zip(src_places, dst_places, lengths)], need)
    src = bytes_dev(torch, src_h, src_shift)
    dst = bytes_dev(torch, np.full(off + 4, SENTINEL, dtype=np.uint32), dst_shift)
    assert (src.data_ptr() % 16, dst.data_ptr() % 16) == (src_shift, dst_shift)
    D.decode_objects_batch(plan, src, dst, batch, map_dev(torch, ms))
    assert_equal(bytes_host(torch, dst), want)
    assert_equal(bytes_host(torch, src), src_h)


# ------------------------------------------------------------------ decode: plan sets

@pytest.mark.parametrize("align", [1, 64])
@pytest.mark.parametrize("need,total", [(3, 5), (8, 12), (16, 20), (17, 20), (33, 50)])
def test_plan_sets_repair_every_boundary_length(torch_dev, mode, need, total, align):
    """Objects at every boundary length (L == 0 among them) with 1 to total - need erasures each,
    every fifth intact (SLIME_RS_NO_PLAN); neighbours have different plans and different mappings.
    Bit-identical to the per-object oracle result, intact objects untouched."""
    lengths = boundary_lengths(need)
    np.random.default_rng(need * 137 + total).shuffle(lengths)
    allp = PATTERNS[(need, total)]
    pats = [None if o % 5 == 3 else allp[o % len(allp)] for o in range(len(lengths))]
    assert {len(p) for p in pats if p} >= {1, total - need} and 0 in lengths
    ms = mappings(len(lengths), total)
    init, want, places = stored_repair_case(need, total, lengths, pats, align, need * 11 + total, ms)
    pset, plan_of = make_set(need, total, pats)
    assert (plan_of == N.NO_PLAN).any()
    run_decode(torch_dev, pset, planned_batch(lengths, places, need, plan_of, pset.nplans), init, want, ms)


def test_planned_batch_through_the_single_plan_launch(torch_dev, mode):
    """The single-plan form accepts a planned batch: plan indices ignored, NO_PLAN objects skipped."""
    need, total = 8, 12
    pat = ERASE[(need, total)]
    lengths = [5, 770, 0, 257, 1537]
    pats = [pat, None, pat, pat, None]
    ms = mappings(len(lengths), 3)
    init, want, places = stored_repair_case(need, total, lengths, pats, 1, 55, ms)
    batch = planned_batch(lengths, places, need, np.array([0, N.NO_PLAN, 2, 1, N.NO_PLAN], dtype=np.uint32), 3)
    run_decode(torch_dev, repair_plan(need, total, pat), batch, init, want, ms)


# ------------------------------------------------------------------ decode: equal to the uniform byte path

def test_equal_lengths_agree_with_decode_objects_chunked(torch_dev, mode):
    torch = torch_dev
    from slime_amd import device as D
    need, total = 8, 12
    pat = ERASE[(need, total)]
    T, _ = geometry(need)
    L, nobj = 3 * T + 5, 5
    lengths = [L] * nobj
    ms = mappings(nobj, 8)
    init, want, places = stored_repair_case(need, total, lengths, [pat] * nobj, 1, 812, ms)
    assert places == [(3 + o * total * L, L) for o in range(nobj)]
    plan = repair_plan(need, total, pat)
    a = bytes_dev(torch, init)
    mt = map_dev(torch, ms)
    D.decode_objects_batch(plan, a, a, in_place_batch(lengths, places, need), mt)
    ga = bytes_host(torch, a)
    assert_equal(ga, want)  # the oracle first
    b = bytes_dev(torch, init[3:])  # the same bytes as nobj uniform slots from an aligned base
    D.decode_objects(plan, b, 4 * total * L, L, nobj, mt)
    assert_equal(bytes_host(torch, b), ga[3:])


# ------------------------------------------------------------------ verify

def raw_verify(torch, plan_or_set, batch, src, cmp, mt, stream=None):
    """The C call into result arrays pre-filled with garbage."""
    from slime_amd import device as D
    is_set = isinstance(plan_or_set, D.PlanSet)
    rows = plan_or_set.max_rows if is_set else plan_or_set.rows
    call = N.lib.slime_rs_planset_verify_objects_batch if is_set else N.lib.slime_rs_verify_objects_batch
    mism = torch.full((batch.nobj, rows), GARBAGE, dtype=torch.int64, device="cuda")
    first = torch.full((batch.nobj, rows), GARBAGE, dtype=torch.int64, device="cuda")
    N.check(call(plan_or_set._h, batch._h, ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(cmp.data_ptr()),
                 ctypes.c_void_p(mt.data_ptr()), ctypes.c_void_p(mism.data_ptr()), ctypes.c_void_p(first.data_ptr()),
                 D._stream_handle(0, stream)))
    return mism, first


def parity_plan(need, total):
    """The encode-shaped plan over a full object: inputs 0..need-1, outputs need..total-1."""
    from slime_amd import device as D
    plan = D.Plan.encode(need, total).set_outputs(list(range(need, total)))
    assert np.array_equal(plan.coefficients(), OC.parity_matrix(need, total - need)[need:])
    return plan


@pytest.mark.parametrize("align", [1, 64])
@pytest.mark.parametrize("need,total", CODES)
def test_verify_clean_every_boundary_length(torch_dev, mode, need, total, align):
    """Oracle-encoded stored objects at every boundary length and step boundary, neighbours with
    different mappings: all counts 0, all firsts -1 over garbage-filled result arrays, through the
    C call and through the wrapper, and the data buffer unchanged."""
    torch = torch_dev
    from slime_amd import device as D
    rows = total - need
    lengths = verify_lengths(need, rows)
    np.random.default_rng(need * 37 + total).shuffle(lengths)
    ms = mappings(len(lengths), need)
    _, full, places, _ = encode_case(need, total, lengths, align, seed=need * 2003 + total)
    h = stored(full, places, lengths, total, ms)
    batch = in_place_batch(lengths, places, need)
    plan = parity_plan(need, total)
    buf, mt = bytes_dev(torch, h), map_dev(torch, ms)
    assert_results(host(torch, raw_verify(torch, plan, batch, buf, buf, mt)), clean_results(len(lengths), rows))
    m, f = D.verify_objects_batch(plan, buf, buf, batch, mt)
    assert m.shape == f.shape == (len(lengths), rows) and m.dtype == f.dtype == torch.int64
    assert_results(host(torch, (m, f)), clean_results(len(lengths), rows))
    assert_equal(bytes_host(torch, buf), h)


_flips = {}


def flip_case(need, total):
    """Round p flips one BYTE at the p-th position of flip_positions in every object that has
    one: even objects in a stored (parity) chunk, odd objects in an input chunk -- neighbours have
    different mappings.  The expectation is the oracle's over the symbol view of the flipped
    bytes.  [(bytes, results)] per round, cached."""
    key = (need, total)
    if key not in _flips:
        rows = total - need
        lengths = verify_lengths(need, rows)
        ms = mappings(len(lengths), total)
        _, full, places, _ = encode_case(need, total, lengths, 1, seed=need * 2011 + total)
        clean = stored(full, places, lengths, total, ms)
        coeff = OC.parity_matrix(need, rows)[need:]
        pos = [flip_positions(L, need, rows) for L in lengths]
        rounds = []
        for p in range(max(len(q) for q in pos)):
            h = clean.copy()
            hb = h.view(np.uint8)
            hits = 0
            for o, (L, q) in enumerate(zip(lengths, pos)):
                if p < len(q):
                    s = need + (o + p) % rows if o % 2 == 0 else (o + p) % need
                    word = places[o][0] + s * places[o][1] + q[p]
                    hb[4 * word + (o + p) % 4] ^= np.uint8(1 << ((o + p) % 8))
                    hits += 1
            sym = unstored(h, places, lengths, total, ms)
            res = expect_batch(coeff, list(range(need)), list(range(need, total)), sym, places, sym, places, lengths)
            assert res[0].sum() >= hits
            for o, (L, q) in enumerate(zip(lengths, pos)):
                if p < len(q) and o % 2 == 0:  # a stored flip: exactly that (object, row), once
                    assert (res[0][o, (o + p) % rows], res[1][o, (o + p) % rows]) == (1, q[p])
            rounds.append((h, res))
        _flips[key] = (lengths, places, ms, rounds)
    return _flips[key]


@pytest.mark.parametrize("need,total", CODES)
def test_verify_one_flipped_byte_per_object(torch_dev, mode, need, total):
    torch = torch_dev
    lengths, places, ms, rounds = flip_case(need, total)
    batch = in_place_batch(lengths, places, need)
    plan = parity_plan(need, total)
    mt = map_dev(torch, ms)
    for p, (h, want) in enumerate(rounds):
        buf = bytes_dev(torch, h)
        assert_results(host(torch, raw_verify(torch, plan, batch, buf, buf, mt)), want, p)
        assert_equal(bytes_host(torch, buf), h)


@pytest.mark.parametrize("src_shift,cmp_shift", [(2, 0), (0, 2), (4, 12)])
def test_verify_separate_cmp_and_unaligned_bases(torch_dev, mode, src_shift, cmp_shift):
    """Round 0 of the flip case with src and cmp as two tensors at other base alignments: 2 bytes
    off takes the column form, 4 and 12 the vector form; same answers."""
    torch = torch_dev
    need, total = 8, 12
    lengths, places, ms, rounds = flip_case(need, total)
    h, want = rounds[0]
    src, cmp = bytes_dev(torch, h, src_shift), bytes_dev(torch, h, cmp_shift)
    got = raw_verify(torch, parity_plan(need, total), in_place_batch(lengths, places, need), src, cmp,
                     map_dev(torch, ms))
    assert_results(host(torch, got), want)


def test_verify_stored_word_plus_p_is_a_mismatch(torch_dev, mode):
    """A stored BE((computed + p) ^ m) where 3 is computed counts as a mismatch, whatever m is; an
    input symbol p + 3 with 3 stored does not."""
    torch = torch_dev
    from slime_amd import device as D
    lengths = [5, 1030, 257, 4]
    ms = mappings(len(lengths), 9)
    places, size = packed_spans(lengths, 2, 1, start=3)
    rng = np.random.default_rng(5)
    sym = np.full(size + 4, SENTINEL, dtype=np.uint32)
    em, ef = clean_results(len(lengths), 1)
    for o, (place, L) in enumerate(zip(places, lengths)):
        x = rng.integers(0, P, size=L, dtype=np.uint64).astype(np.uint32)
        x[L - 1], x[2] = 3, P + 3
        shard(sym, place, 0, L)[:] = x
        shard(sym, place, 1, L)[:] = x % np.uint32(P)  # row 0 = 1 * input 0, canonical
        shard(sym, place, 1, L)[L - 1] = P + 3
        em[o, 0], ef[o, 0] = 1, L - 1
    plan = D.Plan.matrix(np.array([[1]], dtype=np.uint32), [0]).set_outputs([1])
    assert_results(expect_batch(plan.coefficients(), [0], [1], sym, places, sym, places, lengths), (em, ef),
                   "the oracle agrees with the planted expectation")
    buf = bytes_dev(torch, stored(sym, places, lengths, 2, ms))
    got = raw_verify(torch, plan, in_place_batch(lengths, places, 1), buf, buf, map_dev(torch, ms))
    assert_results(host(torch, got), (em, ef))


@pytest.mark.parametrize("need,total", [(3, 5), (8, 12), (16, 20), (17, 20)])
def test_verify_plan_set_after_repair(torch_dev, mode, need, total):
    """The set form over what the oracle's repair leaves: clean; rows at or past an object's own
    plan's row count, NO_PLAN objects and L == 0 objects keep the initial values; then one flipped
    byte in one rebuilt chunk of every repaired object is reported at that (object, row) only."""
    torch = torch_dev
    from slime_amd import device as D
    allp = PATTERNS[(need, total)]
    max_rows = max(len(p) for p in allp)
    lengths = verify_lengths(need, max_rows)
    np.random.default_rng(need * 41 + total).shuffle(lengths)
    pats = [None if o % 5 == 3 else allp[o % len(allp)] for o in range(len(lengths))]
    assert {len(p) for p in pats if p} >= {1, 2, total - need}
    ms = mappings(len(lengths), need + total)
    _, want, places = stored_repair_case(need, total, lengths, pats, 1, need * 3001 + total, ms)
    pset, plan_of = make_set(need, total, pats)
    batch = planned_batch(lengths, places, need, plan_of, pset.nplans)
    mt = map_dev(torch, ms)
    buf = bytes_dev(torch, want)
    assert_results(host(torch, raw_verify(torch, pset, batch, buf, buf, mt)), clean_results(len(lengths), max_rows))
    m, f = D.verify_objects_batch(pset, buf, buf, batch, mt)
    assert m.shape == f.shape == (len(lengths), max_rows)
    assert_results(host(torch, (m, f)), clean_results(len(lengths), max_rows))
    h = want.copy()
    hb = h.view(np.uint8)
    em, ef = clean_results(len(lengths), max_rows)
    for o, (L, pat) in enumerate(zip(lengths, pats)):
        q = flip_positions(L, need, max_rows)
        if pat and q:
            i, c = o % len(pat), q[o % len(q)]
            hb[4 * (places[o][0] + sorted(pat)[i] * places[o][1] + c) + o % 4] ^= np.uint8(0x10)
            em[o, i], ef[o, i] = 1, c
        elif pat is None and L:  # an intact object's chunks may hold anything
            hb[4 * (places[o][0] + (total - 1) * places[o][1])] ^= np.uint8(1)
    hbuf = bytes_dev(torch, h)
    assert_results(host(torch, raw_verify(torch, pset, batch, hbuf, hbuf, mt)), (em, ef))
    assert_equal(bytes_host(torch, hbuf), h)


@pytest.mark.parametrize("k,rows", [(33, 67), (3, 70)])
def test_verify_more_than_64_rows(torch_dev, mode, k, rows):
    """Row blocks of 64: the encode plan of (33, 100) -- 67 rows, the column form -- and a random
    70 x 3 matrix through the vector form.  Flips in rows 0, 63, 64 and the last."""
    torch = torch_dev
    from slime_amd import device as D
    lengths = [515, 5, 0, 511]
    ms = mappings(len(lengths), rows)
    coeff, src_s, src_places, cmp_s, cmp_places = matrix_case(k, rows, lengths, seed=rows * 7 + k)
    if k == 33:  # the code's own parity rows, with the oracle's stored rows
        coeff = OC.parity_matrix(33, 67)[33:]
        cmp_s = np.array(cmp_s)
        for sp, cp, L in zip(src_places, cmp_places, lengths):
            if L:
                for i, r in enumerate(OC.apply_matrix(coeff, [np.ascontiguousarray(shard(src_s, sp, j, L))
                                                              for j in range(k)])):
                    shard(cmp_s, cp, i, L)[:] = r
        plan = D.Plan.encode(33, 100)
        assert np.array_equal(plan.coefficients(), coeff)
    else:
        plan = D.Plan.matrix(coeff, list(range(k)))
    batch = D.Batch([(so, ss, do, ds, n) for (so, ss), (do, ds), n in zip(src_places, cmp_places, lengths)], k)
    src = bytes_dev(torch, stored(src_s, src_places, lengths, k, ms))
    mt = map_dev(torch, ms)
    clean = stored(cmp_s, cmp_places, lengths, rows, ms)
    assert_results(host(torch, raw_verify(torch, plan, batch, src, bytes_dev(torch, clean), mt)),
                   clean_results(len(lengths), rows))
    h = clean.copy()
    em, ef = clean_results(len(lengths), rows)
    for o, i, c in ((0, 0, 1), (0, 63, 514), (3, 64, 0), (1, 64, 4), (3, rows - 1, 255), (1, rows - 1, 0)):
        shard(h, cmp_places[o], i, lengths[o])[c] ^= np.uint32(0x20)
        em[o, i], ef[o, i] = 1, c
    sym = unstored(h, cmp_places, lengths, rows, ms)
    assert_results(expect_batch(coeff, list(range(k)), list(range(rows)), np.array(src_s), src_places, sym, cmp_places,
                                lengths), (em, ef), "the oracle agrees with the planted expectation")
    assert_results(host(torch, raw_verify(torch, plan, batch, src, bytes_dev(torch, h), mt)), (em, ef))


def test_verify_empty_batches_only_initialise(torch_dev, mode):
    torch = torch_dev
    from slime_amd import device as D
    plan = parity_plan(4, 6)
    buf = bytes_dev(torch, np.full(64, SENTINEL, dtype=np.uint32))
    for spans in ([(0, 0, 0, 0, 0)] * 7, [(10**9, 8, 10**9, 8, 0)]):
        batch = D.Batch(spans, 4)
        mt = map_dev(torch, mappings(len(spans)))
        dyn0 = N.schedule_counts(0)
        assert_results(host(torch, raw_verify(torch, plan, batch, buf, buf, mt)), clean_results(len(spans), 2))
        assert_results(host(torch, D.verify_objects_batch(plan, buf, buf, batch, mt)), clean_results(len(spans), 2))
        assert N.schedule_counts(0) == dyn0, "an empty batch launches nothing but the initialisation"
        D.decode_objects_batch(plan, buf, buf, batch, mt)
        assert N.lib.slime_rs_decode_objects_batch(plan._h, batch._h, None, None, None, None) == 0  # not even buffers
        assert N.schedule_counts(0) == dyn0
    none = D.Batch([], 4)
    g = torch.full((4,), GARBAGE, dtype=torch.int64, device="cuda")
    p = ctypes.c_void_p(buf.data_ptr())
    assert N.lib.slime_rs_verify_objects_batch(plan._h, none._h, p, p, None, ctypes.c_void_p(g.data_ptr()),
                                               ctypes.c_void_p(g.data_ptr()), None) == 0
    torch.cuda.synchronize()
    assert (g == GARBAGE).all()
    assert (bytes_host(torch, buf) == SENTINEL).all()


# ------------------------------------------------------------------ counter sets, graphs

def test_dynamic_launches_leave_their_counter_sets_zero(torch_dev, mode):
    """Outside a capture the byte launches take the dynamic path in schedule modes 1 and 2, the
    static modes ask for no set; nothing is held after a synchronize, and the launches that follow
    on sets the earlier ones used are still exact."""
    torch = torch_dev
    from slime_amd import device as D
    sched, pipe = mode
    need, total = 3, 5
    T, C = geometry(need)
    lengths = [4 * C * T + 5, T, 5, 0, 3 * C * T, 257] * 8
    pats = cycle(PATTERNS[(need, total)], len(lengths))
    ms = mappings(len(lengths), 4)
    init, want, places = stored_repair_case(need, total, lengths, pats, 1, 4242, ms)
    pset, plan_of = make_set(need, total, pats)
    batch = planned_batch(lengths, places, need, plan_of, pset.nplans)
    assert batch.units > 64
    mt = map_dev(torch, ms)
    torch.cuda.synchronize()
    _, held0 = N.ticket_sets(0)
    dyn0, fb0 = N.schedule_counts(0)
    bufs = [bytes_dev(torch, init) for _ in range(3)]
    for b in bufs:  # back to back: each launch finds a zero set
        D.decode_objects_batch(pset, b, b, batch, mt)
    res = [raw_verify(torch, pset, batch, b, b, mt) for b in bufs]
    dyn1, fb1 = N.schedule_counts(0)
    want_dyn = 6 if sched in (1, 2) and pipe == 1 else 0
    assert (dyn1 - dyn0, fb1 - fb0) == (want_dyn, 0)
    for b, r in zip(bufs, res):
        assert_equal(bytes_host(torch, b), want)
        assert_results(host(torch, r), clean_results(len(lengths), pset.max_rows))
    assert N.ticket_sets(0)[1] == held0, "nothing is held after the launches finished"


@pytest.mark.parametrize("sched", [1, 2])
@pytest.mark.parametrize("need,total", [(3, 5), (17, 20)])
def test_graph_captured_decode_and_verify_replay_exactly(torch_dev, sched, need, total):
    """One decode and one verify captured as a linear chain and replayed twice with the data
    restored (to another batch's bytes, then back) in between: both replays repair exactly and
    report what the host expects.  Mode 1 captures the static forms (no counter set), mode 2 the
    dynamic ones, which hold a set each for the graph's life; the sets return to the pool with it."""
    torch = torch_dev
    from slime_amd import device as D
    s0 = N.lib.slime_rs_kernel_schedule(-1)
    assert N.lib.slime_rs_kernel_schedule(sched) == 0
    try:
        T, C = geometry(need)
        lengths = [4 * C * T + 5, 3, T + 1, 0, 256, C * T] * 2
        pats = cycle(PATTERNS[(need, total)], len(lengths))
        ms = mappings(len(lengths), 6)
        cases = [stored_repair_case(need, total, lengths, pats, 1, sd, ms) for sd in (31, 32)]
        places = cases[0][2]
        pset, plan_of = make_set(need, total, pats)
        batch = planned_batch(lengths, places, need, plan_of, pset.nplans)
        check = repair_plan(need, total, pats[0])  # verify: every object against the first pattern's plan
        mt = map_dev(torch, ms)
        buf = bytes_dev(torch, cases[0][0])
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):  # warm the launch paths outside the capture
            D.decode_objects_batch(pset, buf, buf, batch, mt, stream=s)
            D.verify_objects_batch(check, buf, buf, batch, mt, stream=s)
        torch.cuda.synchronize()
        _, held0 = N.ticket_sets(0)
        dyn0, _ = N.schedule_counts(0)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            D.decode_objects_batch(pset, buf, buf, batch, mt, stream=s)
            gm, gf_ = D.verify_objects_batch(check, buf, buf, batch, mt, stream=s)
        torch.cuda.synchronize()
        took = (N.ticket_sets(0)[1] - held0, N.schedule_counts(0)[0] - dyn0)
        if sched == 2 and need <= 16:
            assert took == (2, 2), "both captured launches took the dynamic schedule"
        else:
            assert took == (0, 0), "both captured launches took a static form"
        for init, want, _ in (cases[1], cases[0]):
            buf.copy_(bytes_dev(torch, init))
            gm.fill_(GARBAGE)
            gf_.fill_(GARBAGE)
            torch.cuda.synchronize()
            g.replay()
            assert_equal(bytes_host(torch, buf), want)
            sym = unstored(want, places, lengths, total, ms)
            exp = expect_batch(check.coefficients(), survivors(need, total, pats[0]), list(pats[0]), sym, places, sym,
                               places, [L if p else 0 for L, p in zip(lengths, pats)])
            assert_results(host(torch, (gm, gf_)), exp)
        del g  # before the batch and the set: the graph's kernel nodes read their tables
        torch.cuda.synchronize()
        assert _held_settles(held0), "the destroyed graph's counter sets went back to the pool"
    finally:
        N.lib.slime_rs_kernel_schedule(s0)


# ------------------------------------------------------------------ refusals

def test_argument_errors_launch_nothing(torch_dev):
    torch = torch_dev
    from slime_amd import device as D
    need, total = 8, 12
    lengths, pats = [100, 7], [(0,), (2, 5)]
    ms = mappings(2)
    init, _, places = stored_repair_case(need, total, lengths, pats, 1, 1, ms)
    pset, plan_of = make_set(need, total, pats)
    batch = planned_batch(lengths, places, need, plan_of, 2)
    plan = repair_plan(need, total, (0,))
    buf, mt = bytes_dev(torch, init), map_dev(torch, ms)
    res = torch.full((4,), GARBAGE, dtype=torch.int64, device="cuda")
    p, r, m = ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(res.data_ptr()), ctypes.c_void_p(mt.data_ptr())
    L = N.lib
    dyn0 = N.schedule_counts(0)

    def refused(call, *args):
        assert call(*args, None) == N.ERR_INVALID_ARG, (call.__name__, args)
        assert call.__name__.replace("slime_rs_", "") in L.slime_rs_last_error().decode()

    unplanned = D.Batch([(o, s, o, s, n) for (o, s), n in zip(places, lengths)], need)
    three = planned_batch(lengths, places, need, plan_of, 3)
    other_k = planned_batch(lengths, places, need - 1, plan_of, 2)
    for call, head in ((L.slime_rs_decode_objects_batch, plan), (L.slime_rs_planset_decode_objects_batch, pset)):
        refused(call, None, batch._h, p, p, m)
        refused(call, head._h, None, p, p, m)
        for args in ((None, p, m), (p, None, m), (p, p, None)):
            refused(call, head._h, batch._h, *args)
        refused(call, head._h, other_k._h, p, p, m)
    for call, head in ((L.slime_rs_verify_objects_batch, plan), (L.slime_rs_planset_verify_objects_batch, pset)):
        refused(call, None, batch._h, p, p, m, r, r)
        refused(call, head._h, None, p, p, m, r, r)
        for args in ((None, p, m, r, r), (p, None, m, r, r), (p, p, None, r, r), (p, p, m, None, r), (p, p, m, r, None)):
            refused(call, head._h, batch._h, *args)
        refused(call, head._h, other_k._h, p, p, m, r, r)
    for b in (unplanned, three):  # the set forms: an unplanned batch, another nplans
        refused(L.slime_rs_planset_decode_objects_batch, pset._h, b._h, p, p, m)
        refused(L.slime_rs_planset_verify_objects_batch, pset._h, b._h, p, p, m, r, r)
    with pytest.raises(ValueError, match="no plan indices"):
        D.decode_objects_batch(pset, buf, buf, unplanned, mt)
    with pytest.raises(ValueError, match="3 plans"):
        D.verify_objects_batch(pset, buf, buf, three, mt)
    with pytest.raises(ValueError, match="k=7"):
        D.decode_objects_batch(pset, buf, buf, other_k, mt)
    with pytest.raises(ValueError, match="addresses element"):
        D.decode_objects_batch(pset, buf, buf[:-4 * 48], batch, mt)  # ends inside chunk 5 of the last object
    with pytest.raises(ValueError, match="mapping"):
        D.verify_objects_batch(plan, buf, buf, batch, mt[:1])
    with pytest.raises(ValueError, match="uint8"):
        D.decode_objects_batch(plan, buf.view(torch.int32), buf, batch, mt)
    torch.cuda.synchronize()
    assert (res == GARBAGE).all() and N.schedule_counts(0) == dyn0, "a refused call launches nothing"
    assert_equal(bytes_host(torch, buf), init)
    plan.set_outputs([0])  # refusals do not mark the plan; the set forms mark nothing
    D.decode_objects_batch(plan, buf, buf, unplanned, mt)
    with pytest.raises(N.NativeError, match="already launched"):
        plan.set_outputs([1])
