"""Ragged byte encode on the GPU: slime_rs_encode_objects_batch and
slime_rs_resolve_fallbacks_batch -- objects of different sizes written in one
launch, each with its own padding, data-chunk tail and MapToGF mapping.

Every expectation is the C oracle's, object by object on the host
(test_gpu_parity._oracle_chunks: OC.map_to_gf -> split -> OC.create_parity ->
OC.map_from_gf), never a kernel's.  Buffers are SENTINEL-filled, the bytes past
an object's size inside its data chunks hold 0xFF garbage on entry (words that
would raise both flags if a kernel counted them), and whole buffers are
compared: data tails, parity, and every byte outside the objects' chunks.
mapping and status are pre-filled with garbage.  References are computed once
per object content and shared by the schedule / pipeline modes.

The candidate stream behind slime_gf_seed is the library's own generator: the
fallback cases assert what holds for any stream (the mapping fits, is neither 0
nor 1<<31, and the bytes are the oracle's with that mapping), and
test_first_seeded_candidate_that_fails_is_passed_over learns the stream's first
candidate from a run, then makes it fail by construction.
"""
import ctypes

import numpy as np
import pytest

from slime_amd import _native as N
from slime_amd import gf
from test_gpu_bytes_ragged import assert_equal, bytes_dev, bytes_host
from test_gpu_parity import _oracle_chunks
from test_gpu_planset import PATTERNS, cycle, make_set, planned_batch
from test_gpu_ragged import (P, SENTINEL, boundary_lengths, encode_plan, geometry, in_place_batch,  # noqa: F401
                             mode, packed_spans, torch_dev)
from test_gpu_schedule import _held_settles

pytestmark = pytest.mark.gpu

HIGH = 1 << 31
GARBAGE32 = 0x5EEDBEEF
FF, LOW = 0xFFFFFFFF, 0x7FFFFFFE  # a word >= p (bit 0), a word whose ^ 1<<31 is >= p (bit 1 alone)


def L_of(S, k):
    return -(-(-(-S // 4)) // k)


def clean_obj(rng, S):
    """S bytes whose big-endian words are all below p: mapping 0."""
    nw = -(-S // 4)
    return rng.integers(0, P, size=nw, dtype=np.uint64).astype(np.uint32).byteswap().tobytes()[:S]


def plant(obj, w, value):
    b = bytearray(obj)
    b[4 * w: 4 * w + 4] = int(value).to_bytes(4, "big")
    return bytes(b)


_ref = {}


def oracle(obj, need, total, cands=()):
    key = (need, total, tuple(cands), obj)
    if key not in _ref:
        _ref[key] = _oracle_chunks(obj, need, total, list(cands))
    return _ref[key]


def layout(need, total, sizes, align):
    lengths = [L_of(S, need) for S in sizes]
    places, size = packed_spans(lengths, total, align, start=3 if align == 1 else 64)
    return lengths, places, size + 5


def make_init(need, objs, lengths, places, size):
    """The buffer going in: data chunks with 0xFF past the object's bytes, SENTINEL everywhere else."""
    init = np.full(size, SENTINEL, dtype=np.uint32)
    ib = init.view(np.uint8)
    for obj, (off, ss), L in zip(objs, places, lengths):
        a = np.frombuffer(obj, dtype=np.uint8)
        for j in range(need if L else 0):
            c0 = 4 * (off + j * ss)
            ib[c0: c0 + 4 * L] = 0xFF
            part = a[4 * j * L: 4 * (j + 1) * L]
            ib[c0: c0 + part.size] = part
    return init


def make_want(need, total, objs, lengths, places, size, cands=None, skip=()):
    """(want, ms): the oracle's chunks in the same places, and its mappings (objects in `skip`
    are left as SENTINEL, mapping 0)."""
    want = np.full(size, SENTINEL, dtype=np.uint32)
    wb = want.view(np.uint8)
    ms = np.zeros(len(objs), dtype=np.uint32)
    for o, (obj, (off, ss), L) in enumerate(zip(objs, places, lengths)):
        if L == 0 or o in skip:
            continue
        m, chunks = oracle(obj, need, total, cands[o] if cands else ())
        ms[o] = m
        for c in range(total):
            c0 = 4 * (off + c * ss)
            wb[c0: c0 + 4 * L] = np.frombuffer(chunks[c], dtype=np.uint8)
    return want, ms


def build(need, total, objs, lengths, places, size, cands=None):
    """(init, want, ms)"""
    return (make_init(need, objs, lengths, places, size),) + make_want(need, total, objs, lengths, places, size, cands)


def garbage(torch, n):
    return torch.full((n,), GARBAGE32, dtype=torch.int32, device="cuda")


def words(torch, t):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint32)


def run_encode(torch, plan, batch, init, sizes, stream=None):
    from slime_amd import device as D
    buf = bytes_dev(torch, init)
    mp, st = garbage(torch, batch.nobj), garbage(torch, batch.nobj)
    D.encode_objects_batch(plan, buf, buf, batch, sizes, mp, st, stream=stream)
    return buf, mp, st


def check(torch, buf, mp, st, want, ms, status=None):
    assert_equal(words(torch, mp), ms)
    assert_equal(words(torch, st), np.zeros(len(ms), dtype=np.uint32) if status is None else status)
    assert_equal(bytes_host(torch, buf), want)


# ------------------------------------------------------------------ 1: boundary lengths and size classes

CODES = [(1, 2), (3, 5), (8, 12), (16, 20), (17, 20), (33, 50)]
_cases = {}


def boundary_case(need, total, align):
    key = (need, total, align)
    if key not in _cases:
        rng = np.random.default_rng(need * 977 + total)
        sizes = []
        for n, L in enumerate(L for L in boundary_lengths(need) if L):
            k4 = 4 * need
            rot = [k4 * L, k4 * L - 1, k4 * L - 2, k4 * L - 3, k4 * (L - 1) + 1, k4 * (L - 1) + 4]
            S = rot[n % 6]
            sizes.append(S if S > 0 and L_of(S, need) == L else k4 * L)
        # whole chunks of padding (nw < k), S = 1, L = 0
        sizes += [1, 0, 4 * (need - 1) if need > 1 else 3, 5 if need > 2 else 2, 0]
        rng.shuffle(sizes)
        assert {L_of(S, need) for S in sizes} >= set(boundary_lengths(need))
        objs = [clean_obj(rng, S) for S in sizes]
        lengths, places, size = layout(need, total, sizes, align)
        _cases[key] = (sizes, lengths, places) + build(need, total, objs, lengths, places, size)
    return _cases[key]


@pytest.mark.parametrize("align", [1, 64])
@pytest.mark.parametrize("need,total", CODES)
def test_boundary_lengths_and_size_classes(torch_dev, mode, need, total, align):
    """Every L of boundary_lengths(k) in one batch, the sizes rotating over 4kL, 4kL-1, 4kL-2,
    4kL-3, 4k(L-1)+1 and 4k(L-1)+4, plus objects of fewer words than chunks, S = 1 and L = 0; 0xFF
    garbage past S.  No word is >= p: every mapping and status 0, every chunk byte the oracle's."""
    sizes, lengths, places, init, want, ms = boundary_case(need, total, align)
    assert not ms.any()
    buf, mp, st = run_encode(torch_dev, encode_plan(need, total), in_place_batch(lengths, places, need), init, sizes)
    check(torch_dev, buf, mp, st, want, ms)


# ------------------------------------------------------------------ 2: switch and flag position

def position_case(need, total, value):
    """Objects of one size, odd ones with a single planted word at one position class each."""
    key = ("pos", need, total, value)
    if key not in _cases:
        T, C = geometry(need)
        L = C * T + T + 6  # two units, L % 4 == 2
        S = 4 * need * L - 9  # nw = kL - 2, the last word partial, two padding words
        assert L_of(S, need) == L and need >= 3
        where = [(0, 0),              # word 0
                 (1, 3),              # the last word of a vector
                 (need - 1, T - 1),   # the last lane of a tile
                 (0, C * T),          # the first column of the second unit
                 (0, T),              # the first column of a unit's second tile
                 (0, L - 1),          # a column of L % 4
                 (1, L - 5),          # an edge column inside the whole vectors
                 (need - 1, L - 4)]   # the last whole word, nw - 2
        assert where[-1][0] * L + where[-1][1] == -(-S // 4) - 2
        rng = np.random.default_rng(need + 400)
        objs, hot = [], []
        for j, c in where:
            objs += [clean_obj(rng, S), plant(clean_obj(rng, S), j * L + c, value)]
            hot.append(len(objs) - 1)
        objs.append(clean_obj(rng, S))
        sizes = [S] * len(objs)
        lengths, places, size = layout(need, total, sizes, 1)
        _cases[key] = (sizes, lengths, places, hot) + build(need, total, objs, lengths, places, size)
    return _cases[key]


@pytest.mark.parametrize("value", [FF, P, LOW], ids=["ffffffff", "p", "7ffffffe"])
@pytest.mark.parametrize("need,total", [(3, 5), (8, 12), (16, 20), (17, 20)])
def test_switch_and_flag_position(torch_dev, mode, need, total, value):
    """One word in [p, 2^32) at each position class, every such object between clean neighbours:
    mapping 1<<31 for exactly those objects (padding words BE(1<<31), bytes the oracle's).  The
    same with a word in [2^31 - 5, 2^31), which sets the other flag bit alone: every mapping 0."""
    sizes, lengths, places, hot, init, want, ms = position_case(need, total, value)
    exp = np.zeros(len(sizes), dtype=np.uint32)
    if value != LOW:
        exp[hot] = HIGH
    assert_equal(ms, exp)  # the oracle agrees with the statement above
    buf, mp, st = run_encode(torch_dev, encode_plan(need, total), in_place_batch(lengths, places, need), init, sizes)
    check(torch_dev, buf, mp, st, want, ms)


# ------------------------------------------------------------------ 3: flags follow the tile

def many_case(need, total, nobj, shift):
    key = ("many", need, total, nobj, shift)
    if key not in _cases:
        T, _ = geometry(need)
        base = ("manybase", need, total, nobj)
        if base not in _cases:
            rng = np.random.default_rng(need * 31 + 7)
            tiles = [1, 1, 2, 1, 1, 3, 1, 1, 1, 2, 1]  # period 11 against the switched set's 7
            sizes = [4 * need * T * tiles[o % 11] - (o % 3) for o in range(nobj)]
            _cases[base] = (sizes, [clean_obj(rng, S) for S in sizes])
        sizes, clean = _cases[base]
        objs = [plant(b, (o * 37) % (len(b) // 4), FF) if o % 7 == shift else b for o, b in enumerate(clean)]
        lengths, places, size = layout(need, total, sizes, 1)
        _cases[key] = (sizes, lengths, places) + build(need, total, objs, lengths, places, size)
    return _cases[key]


@pytest.mark.parametrize("need,total,nobj", [(3, 5, 1100), (8, 12, 1100), (16, 20, 4200)])
def test_flags_follow_the_tile(torch_dev, mode, need, total, nobj):
    """More objects of one to three tiles than the static grid has waves, every 7th switched, then
    the switched set shifted by one object.  A wave consumes a tile of one object after its walk
    has moved to the next: a build that ORs the flags into the walk's CURRENT object marks the
    neighbour instead (or as well), so mapping and status differ per object in one run or the other."""
    plan = encode_plan(need, total)
    for shift in (0, 1):
        sizes, lengths, places, init, want, ms = many_case(need, total, nobj, shift)
        assert_equal(ms, np.array([HIGH if o % 7 == shift else 0 for o in range(nobj)], dtype=np.uint32))
        batch = in_place_batch(lengths, places, need)
        assert batch.units >= nobj > (4096 if need > 12 else 1024)
        buf, mp, st = run_encode(torch_dev, plan, batch, init, sizes)
        check(torch_dev, buf, mp, st, want, ms)


# ------------------------------------------------------------------ 4: fallback

def fallback_objs(need, rng):
    T, C = geometry(need)
    L = C * T + 10
    S = 4 * need * L - 6
    assert L_of(S, need) == L
    nw = -(-S // 4)
    edge = (need - 1) * L + L - 3  # a whole word of the last chunk, in an edge column
    assert edge < nw - 1
    both = [(5, 9), (7, 2 * L + 11), (edge, 3), (L + T, edge)]  # one chunk; two chunks; an edge column, twice
    objs, kind = [], []
    for a, b in both:
        objs += [clean_obj(rng, S), plant(plant(clean_obj(rng, S), a, FF), b, LOW), plant(clean_obj(rng, S), a, FF)]
        kind += [0, 1, 2]
    objs += [clean_obj(rng, 4 * need * 3 - 1)]
    kind += [0]
    return objs, np.array(kind)


@pytest.mark.parametrize("need,total", [(3, 5), (8, 12), (17, 20)])
def test_fallback_objects_are_resolved_and_only_they(torch_dev, mode, need, total):
    torch = torch_dev
    from slime_amd import device as D
    key = ("fb", need, total)
    if key not in _cases:
        objs, kind = fallback_objs(need, np.random.default_rng(need + 77))
        sizes = [len(b) for b in objs]
        _cases[key] = (objs, kind, sizes) + layout(need, total, sizes, 1)
    objs, kind, sizes, lengths, places, size = _cases[key]
    fb = np.flatnonzero(kind == 1)
    init = make_init(need, objs, lengths, places, size)
    # before the resolve: the oracle's bytes for every other object
    want0, ms0 = make_want(need, total, objs, lengths, places, size, skip=set(int(o) for o in fb))
    plan, batch = encode_plan(need, total), in_place_batch(lengths, places, need)
    buf, mp, st = run_encode(torch, plan, batch, init, sizes)
    assert_equal(words(torch, st), (kind == 1).astype(np.uint32))
    snap = bytes_host(torch, buf).copy()
    mine = np.zeros(size, dtype=bool)  # the fallback objects' chunks
    for o in fb:
        for c in range(total):
            mine[places[o][0] + c * places[o][1]: places[o][0] + c * places[o][1] + lengths[o]] = True
    assert_equal(snap[~mine], want0[~mine])
    assert_equal(words(torch, mp)[kind != 1], ms0[kind != 1])
    gf.Seed(need * 100 + total)
    assert D.resolve_fallbacks_batch(plan, buf, buf, batch, sizes, mp, st) == len(fb)
    got_m = words(torch, mp).copy()
    assert not words(torch, st).any()
    cands = [()] * len(objs)
    for o in fb:
        m = int(got_m[o])
        assert m not in (0, HIGH)
        w = np.frombuffer(objs[o] + bytes(-len(objs[o]) % 4), dtype=">u4").astype(np.uint32)
        assert int((w ^ np.uint32(m)).max()) < P, "the mapping fits every word"
        cands[o] = (m,)
    _, want, ms = build(need, total, objs, lengths, places, size, cands)
    assert_equal(got_m, ms)
    after = bytes_host(torch, buf)
    assert_equal(after, want)
    assert_equal(after[~mine], snap[~mine])  # every other object's bytes unchanged by the resolve
    assert D.resolve_fallbacks_batch(plan, buf, buf, batch, sizes, mp, st) == 0


def test_first_seeded_candidate_that_fails_is_passed_over(torch_dev):
    """The first non-zero FIT wins, not the first candidate.  The stream is learned, not
    predicted: after gf.Seed(n) a two-word fallback object (which nearly every candidate fits)
    takes the stream's first non-zero candidate m0.  An object that also holds the word
    m0 ^ 0xFFFFFFFF makes m0 fail by construction (that word ^ m0 is 0xFFFFFFFF >= p): after the
    same seed it must get another mapping that fits, and the oracle's bytes with that mapping."""
    torch = torch_dev
    from slime_amd import device as D
    need, total = 8, 12
    plan = encode_plan(need, total)

    def resolve(objs):
        sizes = [len(b) for b in objs]
        lengths, places, size = layout(need, total, sizes, 1)
        batch = in_place_batch(lengths, places, need)
        buf, mp, st = run_encode(torch, plan, batch, make_init(need, objs, lengths, places, size), sizes)
        assert_equal(words(torch, st), np.ones(len(objs), dtype=np.uint32))
        gf.Seed(4711)
        assert D.resolve_fallbacks_batch(plan, buf, buf, batch, sizes, mp, st) == len(objs)
        ms = [int(m) for m in words(torch, mp)]
        want, wm = make_want(need, total, objs, lengths, places, size, [(m,) for m in ms])
        assert [int(m) for m in wm] == ms and not words(torch, st).any()
        assert_equal(bytes_host(torch, buf), want)
        return ms

    m0, = resolve([FF.to_bytes(4, "big") + LOW.to_bytes(4, "big")])
    assert m0 not in (0, HIGH)
    T, _ = geometry(need)
    rng = np.random.default_rng(12)
    S = 4 * need * (T + 9) - 2
    obj = plant(plant(plant(clean_obj(rng, S), 3, FF), T + 20, LOW), 2 * (T + 9) + 1, m0 ^ 0xFFFFFFFF)
    m1, = resolve([obj])
    assert m1 not in (0, HIGH, m0), "m0 cannot fit: the word m0 ^ 0xFFFFFFFF maps to 0xFFFFFFFF"
    w = np.frombuffer(obj + bytes(-len(obj) % 4), dtype=">u4").astype(np.uint32)
    assert int((w ^ np.uint32(m1)).max()) < P and int((w ^ np.uint32(m0)).max()) >= P


# ------------------------------------------------------------------ 5: agreement with the uniform pipeline

@pytest.mark.parametrize("align", [1, 64])
def test_equal_lengths_agree_with_the_uniform_pipeline(torch_dev, mode, align):
    """Equal lengths, in-place slots, the kinds plain, high and fallback: mapping, status and every
    slot byte equal slime_rs_encode_objects_chunked plus slime_rs_resolve_fallbacks_chunked over
    the same bytes after the same seed -- with the chunk stride given as 4L (align 1) and as the
    span's padded shard stride (align 64)."""
    torch = torch_dev
    from slime_amd import device as D
    need, total, nobj = 8, 12, 6
    T, _ = geometry(need)
    L = 3 * T + 5
    S = 4 * need * L - 7
    rng = np.random.default_rng(55)
    objs = []
    for o in range(nobj):
        b = clean_obj(rng, S)
        if o % 3 >= 1:
            b = plant(b, 11 + o * L, FF)
        if o % 3 == 2:
            b = plant(b, 2 * L + 3, LOW)
        objs.append(b)
    sizes = [S] * nobj
    lengths, places, size = layout(need, total, sizes, align)
    ss, start = -(-L // align) * align, places[0][0]
    assert places == [(start + o * total * ss, ss) for o in range(nobj)]
    init = make_init(need, objs, lengths, places, size)  # object byte i in chunk i // 4L at offset i % 4L
    gf.Seed(99)
    plan = encode_plan(need, total)
    batch = in_place_batch(lengths, places, need)
    a, mp, st = run_encode(torch, plan, batch, init, sizes)
    assert_equal(words(torch, st), np.array([o % 3 == 2 for o in range(nobj)], dtype=np.uint32))
    assert D.resolve_fallbacks_batch(plan, a, a, batch, sizes, mp, st) == 2
    ga, gm, gs = bytes_host(torch, a), words(torch, mp).copy(), words(torch, st).copy()
    gf.Seed(99)
    b = bytes_dev(torch, init[start:])  # the same bytes as nobj uniform slots
    ump, ust = garbage(torch, nobj), garbage(torch, nobj)
    up = D.Plan.encode(need, total)
    N.check(N.lib.slime_rs_encode_objects_chunked(up._h, ctypes.c_void_p(b.data_ptr()), 4 * total * ss, 4 * ss, S, nobj,
                                                  ctypes.c_void_p(ump.data_ptr()), ctypes.c_void_p(ust.data_ptr()),
                                                  None))
    assert D.resolve_fallbacks(up, b, 4 * total * ss, S, nobj, ump, ust, chunk_stride=4 * ss) == 2  # _chunked
    assert_equal(gm, words(torch, ump))
    assert_equal(gs, words(torch, ust))
    assert_equal(ga[start:], bytes_host(torch, b))
    assert [int(m) for m in gm[:2]] == [0, HIGH] and int(gm[2]) not in (0, HIGH)


# ------------------------------------------------------------------ 6: round trip through the siblings

@pytest.mark.parametrize("need,total", [(3, 5), (8, 12), (17, 20)])
def test_round_trip_through_verify_and_planset_decode(torch_dev, mode, need, total):
    torch = torch_dev
    from slime_amd import device as D
    T, C = geometry(need)
    rng = np.random.default_rng(need + 600)
    sizes = [4 * need * (C * T + 5) - 2, 7, 4 * need * T, 4 * need * 257 - 5, 0, 4 * need * (4 * C * T + 5) - 11,
             4 * need * 3]
    objs = [clean_obj(rng, S) for S in sizes]
    objs[0] = plant(objs[0], 17, FF)
    objs[3] = plant(objs[3], 300, P + 1)
    lengths, places, size = layout(need, total, sizes, 64)
    init, want, ms = build(need, total, objs, lengths, places, size)
    assert sorted(set(int(m) for m in ms)) == [0, HIGH]
    plan = encode_plan(need, total)
    buf, mp, st = run_encode(torch, plan, in_place_batch(lengths, places, need), init, sizes)
    check(torch, buf, mp, st, want, ms)
    mism, first = D.verify_objects_batch(plan, buf, buf, in_place_batch(lengths, places, need), mp)
    torch.cuda.synchronize()
    assert int(mism.sum()) == 0 and bool((first == -1).all())
    pats = cycle([p for p in PATTERNS[(need, total)] if len(p) == total - need], len(sizes))
    pset, plan_of = make_set(need, total, pats)
    erased = want.copy()
    for (off, ss), L, pat in zip(places, lengths, pats):
        for c in pat:
            erased[off + c * ss: off + c * ss + L] = 0xE7A5ED00
    b2 = bytes_dev(torch, erased)
    D.decode_objects_batch(pset, b2, b2, planned_batch(lengths, places, need, plan_of, pset.nplans), mp)
    assert_equal(bytes_host(torch, b2), want)


# ------------------------------------------------------------------ 7: a separate dst, other spans, base shifts

@pytest.mark.parametrize("need,total", [(3, 5), (8, 12)])
@pytest.mark.parametrize("src_shift,dst_shift", [(0, 0), (2, 0), (0, 2), (4, 4), (12, 4)])
def test_separate_dst_other_spans_and_base_shifts(torch_dev, mode, need, total, src_shift, dst_shift):
    """src holds only the data chunks; dst, another tensor, receives only the parity (plan outputs
    0..rows-1), objects in reverse order behind a gap, odd chunk strides.  A base 2 bytes off a word
    boundary takes the column form.  src changes in its data tails only."""
    torch = torch_dev
    from slime_amd import device as D
    rows = total - need
    T, C = geometry(need)
    rng = np.random.default_rng(177 + need)
    sizes = [4 * need * (T + 1) - 3, 0, 4 * need * 3 - 1, 4 * need * (C * T + 5) - 6, 4 * need * 257, 4 * need * 4 - 9]
    objs = [clean_obj(rng, S) for S in sizes]
    objs[3] = plant(objs[3], 4 * T + 1, FF)
    lengths = [L_of(S, need) for S in sizes]
    src_places, ssize = packed_spans(lengths, need, 1, start=3)
    dst_places, off = [None] * len(sizes), 9
    for o in reversed(range(len(sizes))):
        ss = -(-lengths[o] // 8) * 8 + 1
        dst_places[o] = (off, ss)
        off += rows * ss + 3
    src_h = np.full(ssize + 5, SENTINEL, dtype=np.uint32)
    src_w = src_h.copy()
    dst_w = np.full(off + 4, SENTINEL, dtype=np.uint32)
    ms = np.zeros(len(sizes), dtype=np.uint32)
    for o, (obj, L) in enumerate(zip(objs, lengths)):
        if L == 0:
            continue
        ms[o], chunks = oracle(obj, need, total)
        a = np.frombuffer(obj, dtype=np.uint8)
        for j in range(need):
            c0 = 4 * (src_places[o][0] + j * src_places[o][1])
            src_h.view(np.uint8)[c0: c0 + 4 * L] = 0xFF
            part = a[4 * j * L: 4 * (j + 1) * L]
            src_h.view(np.uint8)[c0: c0 + part.size] = part
            src_w.view(np.uint8)[c0: c0 + 4 * L] = np.frombuffer(chunks[j], dtype=np.uint8)
        for i in range(rows):
            c0 = 4 * (dst_places[o][0] + i * dst_places[o][1])
            dst_w.view(np.uint8)[c0: c0 + 4 * L] = np.frombuffer(chunks[need + i], dtype=np.uint8)
    assert ms[3] == HIGH
    batch = D.Batch([(so, ss, do, ds, L) for (so, ss), (do, ds), L in zip(src_places, dst_places, lengths)], need)
    src = bytes_dev(torch, src_h, src_shift)
    dst = bytes_dev(torch, np.full(off + 4, SENTINEL, dtype=np.uint32), dst_shift)
    assert (src.data_ptr() % 16, dst.data_ptr() % 16) == (src_shift, dst_shift)
    mp, st = garbage(torch, len(sizes)), garbage(torch, len(sizes))
    D.encode_objects_batch(D.Plan.encode(need, total), src, dst, batch, sizes, mp, st)  # outputs 0..rows-1
    assert_equal(words(torch, mp), ms)
    assert not words(torch, st).any()
    assert_equal(bytes_host(torch, dst), dst_w)
    assert_equal(bytes_host(torch, src), src_w)


# ------------------------------------------------------------------ 8, 9: graphs, counter sets

def moving_cases(need, total):
    """Three data sets over one layout, the switched objects moving each time."""
    T, C = geometry(need)
    sizes = [4 * need * (4 * C * T + 5) - 3, 9, 4 * need * (T + 1), 0, 4 * need * 256 - 1, 4 * need * C * T] * 2
    lengths, places, size = layout(need, total, sizes, 1)
    out = []
    for r in range(3):
        key = ("move", need, total, r)
        if key not in _cases:
            rng = np.random.default_rng(900 + need + r)
            objs = [clean_obj(rng, S) for S in sizes]
            for o in range(r, len(sizes), 3):
                if sizes[o] >= 8:
                    objs[o] = plant(objs[o], (5 * o + r) % (sizes[o] // 4), FF)
            _cases[key] = build(need, total, objs, lengths, places, size)
        out.append(_cases[key])
    assert len({tuple(c[2]) for c in out}) == 3
    return sizes, lengths, places, out


@pytest.mark.parametrize("sched", [1, 2])
@pytest.mark.parametrize("need,total", [(3, 5), (17, 20)])
def test_graph_captured_encode_replays_exactly(torch_dev, sched, need, total):
    """One encode captured and replayed three times over data changed between the replays, the set
    of switched objects moving each time: mapping, status and bytes exact each time.  Mode 1
    captures the static walks, mode 2 the dynamic ones: each pass holds its own counter set for the
    graph's life, and they return to the pool with it."""
    torch = torch_dev
    from slime_amd import device as D
    s0 = N.lib.slime_rs_kernel_schedule(-1)
    assert N.lib.slime_rs_kernel_schedule(sched) == 0
    try:
        sizes, lengths, places, cases = moving_cases(need, total)
        plan, batch = encode_plan(need, total), in_place_batch(lengths, places, need)
        buf = bytes_dev(torch, cases[0][0])
        mp, st = garbage(torch, len(sizes)), garbage(torch, len(sizes))
        sz = torch.tensor(sizes, dtype=torch.int64, device="cuda")
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):  # warm the launch paths outside the capture
            D.encode_objects_batch(plan, buf, buf, batch, sz, mp, st, stream=s)
        torch.cuda.synchronize()
        _, held0 = N.ticket_sets(0)
        dyn0, _ = N.schedule_counts(0)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            D.encode_objects_batch(plan, buf, buf, batch, sz, mp, st, stream=s)
        torch.cuda.synchronize()
        took = (N.ticket_sets(0)[1] - held0, N.schedule_counts(0)[0] - dyn0)
        assert took == ((2, 2) if sched == 2 and need <= 16 else (0, 0))
        for init, want, ms in (cases[1], cases[2], cases[0]):
            buf.copy_(bytes_dev(torch, init))
            mp.fill_(GARBAGE32)
            st.fill_(GARBAGE32)
            torch.cuda.synchronize()
            g.replay()
            check(torch, buf, mp, st, want, ms)
        del g  # before the batch: the graph's kernel nodes read its tables
        torch.cuda.synchronize()
        assert _held_settles(held0), "the destroyed graph's counter sets went back to the pool"
    finally:
        N.lib.slime_rs_kernel_schedule(s0)


def test_dynamic_launches_leave_their_counter_sets_zero(torch_dev, mode):
    """Outside a capture both passes take the dynamic walk in schedule modes 1 and 2 (a set each);
    nothing is held after a synchronize, and launches on the sets earlier ones used are exact."""
    torch = torch_dev
    sched, pipe = mode
    need, total = 3, 5
    sizes, lengths, places, cases = moving_cases(need, total)
    plan, batch = encode_plan(need, total), in_place_batch(lengths, places, need)
    assert batch.units > 4
    torch.cuda.synchronize()
    _, held0 = N.ticket_sets(0)
    dyn0, fb0 = N.schedule_counts(0)
    runs = [run_encode(torch, plan, batch, c[0], sizes) for c in cases + cases]
    dyn1, fb1 = N.schedule_counts(0)
    assert (dyn1 - dyn0, fb1 - fb0) == (12 if sched in (1, 2) and pipe == 1 else 0, 0)
    for (buf, mp, st), (_, want, ms) in zip(runs, cases + cases):
        check(torch, buf, mp, st, want, ms)
    assert N.ticket_sets(0)[1] == held0, "nothing is held after the launches finished"


# ------------------------------------------------------------------ 10: refusals

def test_argument_errors_launch_nothing(torch_dev):
    torch = torch_dev
    from slime_amd import device as D
    need, total = 8, 12
    sizes = [4 * need * 100 - 3, 4 * need * 7]
    lengths, places, size = layout(need, total, sizes, 1)
    rng = np.random.default_rng(3)
    init, want, ms = build(need, total, [clean_obj(rng, S) for S in sizes], lengths, places, size)
    plan, batch = encode_plan(need, total), in_place_batch(lengths, places, need)
    buf = bytes_dev(torch, init)
    mp, st = garbage(torch, 2), garbage(torch, 2)
    sz = torch.tensor(sizes, dtype=torch.int64, device="cuda")
    p, m, s_, z = (ctypes.c_void_p(t.data_ptr()) for t in (buf, mp, st, sz))
    L = N.lib
    dyn0 = N.schedule_counts(0)
    n = ctypes.c_int(-1)
    calls = ((L.slime_rs_encode_objects_batch, ()), (L.slime_rs_resolve_fallbacks_batch, (ctypes.byref(n),)))

    def refused(call, tail, *args):
        assert call(*args, None, *tail) == N.ERR_INVALID_ARG, (call.__name__, args)
        assert call.__name__.replace("slime_rs_", "") in L.slime_rs_last_error().decode()

    other_k = in_place_batch(lengths, places, need - 1)
    permuted = D.Plan.reconstruct(need, total, [1, 0] + list(range(2, need)), [need]).set_outputs([need])
    shifted = D.Plan.reconstruct(need, total, list(range(1, need + 1)), [0]).set_outputs([0])
    for call, tail in calls:
        refused(call, tail, None, batch._h, p, p, z, m, s_)
        refused(call, tail, plan._h, None, p, p, z, m, s_)
        for args in ((None, p, z, m, s_), (p, None, z, m, s_), (p, p, None, m, s_), (p, p, z, None, s_),
                     (p, p, z, m, None)):
            refused(call, tail, plan._h, batch._h, *args)
        refused(call, tail, plan._h, other_k._h, p, p, z, m, s_)
        for bad in (permuted, shifted):  # inputs that are not 0..k-1 in that order
            refused(call, tail, bad._h, batch._h, p, p, z, m, s_)
            assert "0..k-1" in L.slime_rs_last_error().decode()
    with pytest.raises(ValueError, match="k=7"):
        D.encode_objects_batch(plan, buf, buf, other_k, sizes, mp, st)
    with pytest.raises(ValueError, match="addresses element"):
        D.encode_objects_batch(plan, buf, buf[:-4 * 30], batch, sizes, mp, st)
    with pytest.raises(ValueError, match="L=7"):
        D.encode_objects_batch(plan, buf, buf, batch, [sizes[0], sizes[1] + 1], mp, st)
    with pytest.raises(ValueError, match="status"):
        D.resolve_fallbacks_batch(plan, buf, buf, batch, sizes, mp, st[:1])
    torch.cuda.synchronize()
    assert N.schedule_counts(0) == dyn0, "a refused call launches nothing"
    assert (words(torch, mp) == GARBAGE32).all() and (words(torch, st) == GARBAGE32).all()
    assert_equal(bytes_host(torch, buf), init)
    # an empty batch: only the initialisation, not even buffers or sizes
    empty = D.Batch([(0, 0, 0, 0, 0), (5, 3, 5, 3, 0)], need)
    assert L.slime_rs_encode_objects_batch(plan._h, empty._h, None, None, None, m, s_, None) == 0
    torch.cuda.synchronize()
    assert N.schedule_counts(0) == dyn0
    assert not words(torch, mp).any() and not words(torch, st).any()
    assert_equal(bytes_host(torch, buf), init)
    plan.set_outputs(list(range(need, total)))  # refusals and the empty batch aside, a launch marks the plan
    D.encode_objects_batch(plan, buf, buf, batch, sizes, mp, st)
    check(torch, buf, mp, st, want, ms)
    with pytest.raises(N.NativeError, match="already launched"):
        plan.set_outputs(list(range(need, total)))
