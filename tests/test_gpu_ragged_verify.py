"""Ragged verify (slime_rs_plan_verify_batch) on the GPU: one launch that scrubs
objects of different lengths.

Every expectation comes from the C oracle or numpy on host copies: clean
objects are oracle-encoded codewords (test_gpu_ragged.encode_case), a flipped
word's report follows from the position it was planted at, and everything else
is OC.apply_matrix over the plan's coefficient rows compared with the stored
rows on the host (test_gpu_verify.expected) -- never a kernel under test.
Result arrays are pre-filled with garbage, so every launch also proves the
initialisation; data buffers are compared with their host copies afterwards, so
every launch also proves that verify wrote nothing.  References are computed
once per shape and shared by the schedule / pipeline modes.
"""
import ctypes

import numpy as np
import pytest

from oracle import oracle_c as OC
from slime_amd import _native as N
from test_gpu_ragged import (CODES, P, SENTINEL, boundary_lengths, encode_case, encode_plan, geometry,  # noqa: F401
                             in_place_batch, mode, packed_spans, shard, symbols, to_dev, to_host, torch_dev)
from test_gpu_verify import GARBAGE, expected

pytestmark = pytest.mark.gpu


def step_rule(k, rows):
    """(columns a step covers, steps a whole tile takes): verify_step.hpp restated.  A batch tile
    is U = T / 256 vectors a lane; verify's budget is 24 / (k + R) vectors clipped to 1..4, R = 2
    for up to two rows else 4; the tile goes in ceil(U / budget) steps of ceil(U / steps)."""
    T, _ = geometry(k)
    U, R = T // 256, 2 if rows <= 2 else 4
    budget = max(1, min(4, 24 // (k + R)))
    steps = -(-U // budget)
    return 256 * -(-U // steps), steps


def step_boundaries(k, rows):
    """The columns inside a tile at which a new step starts (none for the column form)."""
    if k > 16:
        return []
    cols, steps = step_rule(k, rows)
    return [s * cols for s in range(1, steps)]


def verify_lengths(k, rows):
    """test_gpu_ragged's boundary lengths plus every step boundary inside a tile, in the first
    tile and in the last tile of a two-tile object."""
    T, _ = geometry(k)
    out = boundary_lengths(k)
    for c in step_boundaries(k, rows):
        out += [c - 1, c, c + 1, T + c - 1, T + c + 2]
    return out


def raw_verify_batch(torch, plan, batch, src, cmp, rows=None, stream=None, src_off_bytes=0, cmp_off_bytes=0):
    """slime_rs_plan_verify_batch into result arrays pre-filled with garbage."""
    from slime_amd import device as D
    rows = plan.rows if rows is None else rows
    mism = torch.full((batch.nobj, rows), GARBAGE, dtype=torch.int64, device="cuda")
    first = torch.full((batch.nobj, rows), GARBAGE, dtype=torch.int64, device="cuda")
    N.check(N.lib.slime_rs_plan_verify_batch(plan._h, batch._h, ctypes.c_void_p(src.data_ptr() + src_off_bytes),
                                             ctypes.c_void_p(cmp.data_ptr() + cmp_off_bytes),
                                             ctypes.c_void_p(mism.data_ptr()), ctypes.c_void_p(first.data_ptr()),
                                             D._stream_handle(0, stream)))
    return mism, first


def host(torch, res):
    torch.cuda.synchronize()
    return res[0].cpu().numpy(), res[1].cpu().numpy()


def clean_results(nobj, rows):
    return np.zeros((nobj, rows), dtype=np.int64), np.full((nobj, rows), -1, dtype=np.int64)


def assert_results(got, want, what=None):
    (m, f), (em, ef) = got, want
    bad = np.argwhere((m != em) | (f != ef))
    assert bad.size == 0, (what, bad[:6].tolist(), [(int(m[o, i]), int(f[o, i]), int(em[o, i]), int(ef[o, i]))
                                                    for o, i in bad[:6]])


def expect_batch(coeff, in_shards, out_shards, src, src_places, cmp, cmp_places, lengths):
    """Counts and firsts of every (object, row): oracle rows over the host copy of src against the
    host copy of cmp."""
    em, ef = clean_results(len(lengths), len(out_shards))
    for o, L in enumerate(lengths):
        if L:
            ins = [np.ascontiguousarray(shard(src, src_places[o], s, L)) for s in in_shards]
            stored = [shard(cmp, cmp_places[o], s, L) for s in out_shards]
            em[o], ef[o] = expected(coeff, ins, stored)
    return em, ef


def flip_positions(L, k, rows):
    """Column 0; the last column of the last whole vector; a tail column; T-1 and T; C*T-1 and
    C*T; each step boundary and the column before it, in the first and in the second tile."""
    T, C = geometry(k)
    cand = [0, L // 4 * 4 - 1, L - 1 if L % 4 else -1, T - 1, T, C * T - 1, C * T]
    for c in step_boundaries(k, rows):
        cand += [c - 1, c, T + c - 1, T + c]
    out = []
    for c in cand:
        if 0 <= c < L and c not in out:
            out.append(c)
    return out


# ------------------------------------------------------------------ clean data

@pytest.mark.parametrize("align", [1, 64])
@pytest.mark.parametrize("need,total", CODES)
def test_clean_every_boundary_length(torch_dev, mode, need, total, align):
    """Oracle-encoded objects at every boundary length and step boundary, packed with shard
    strides of exactly L and of L rounded to 64: all counts 0, all firsts -1, and the whole data
    buffer unchanged."""
    torch = torch_dev
    rows = total - need
    lengths = verify_lengths(need, rows)
    np.random.default_rng(need * 37 + total).shuffle(lengths)
    _, want, places, _ = encode_case(need, total, lengths, align, seed=need * 2003 + total)
    batch = in_place_batch(lengths, places, need)
    plan = encode_plan(need, total)
    buf = to_dev(torch, want)
    assert_results(host(torch, raw_verify_batch(torch, plan, batch, buf, buf)), clean_results(len(lengths), rows))
    m, f = plan.verify_batch(buf, buf, batch)
    assert m.shape == f.shape == (len(lengths), rows) and m.dtype == f.dtype == torch.int64
    assert_results(host(torch, (m, f)), clean_results(len(lengths), rows))
    assert np.array_equal(to_host(torch, buf), want), "verify writes nothing but its results"


# ------------------------------------------------------------------ planted corruption

@pytest.mark.parametrize("need,total", CODES)
def test_one_flipped_stored_word_per_object(torch_dev, mode, need, total):
    """Round p flips, in every object that has a p-th position, one bit of one stored word at that
    position in row (o + p) % rows: exactly that (object, row) reports count 1 and that column."""
    torch = torch_dev
    rows = total - need
    lengths = verify_lengths(need, rows)
    _, want, places, _ = encode_case(need, total, lengths, 1, seed=need * 2011 + total)
    batch = in_place_batch(lengths, places, need)
    plan = encode_plan(need, total)
    pos = [flip_positions(L, need, rows) for L in lengths]
    buf = to_dev(torch, want)
    for p in range(max(len(q) for q in pos)):
        h = want.copy()
        em, ef = clean_results(len(lengths), rows)
        for o, (L, q) in enumerate(zip(lengths, pos)):
            if p < len(q):
                i = (o + p) % rows
                shard(h, places[o], need + i, L)[q[p]] ^= np.uint32(1 << ((o + p) % 32))
                em[o, i], ef[o, i] = 1, q[p]
        buf.copy_(to_dev(torch, h))
        assert_results(host(torch, raw_verify_batch(torch, plan, batch, buf, buf)), (em, ef), p)


@pytest.mark.parametrize("need,total", CODES)
def test_one_corrupted_input_word_per_object(torch_dev, mode, need, total):
    """One input word of every object changed by 1: every row whose coefficient for that input is
    non-zero reports that column once, the other rows stay clean."""
    torch = torch_dev
    rows = total - need
    lengths = verify_lengths(need, rows)
    _, want, places, _ = encode_case(need, total, lengths, 1, seed=need * 2017 + total)
    batch = in_place_batch(lengths, places, need)
    plan = encode_plan(need, total)
    coeff = plan.coefficients()
    h = want.copy()
    em, ef = clean_results(len(lengths), rows)
    for o, L in enumerate(lengths):
        q = flip_positions(L, need, rows)
        if q:
            j, c = o % need, q[o % len(q)]
            shard(h, places[o], j, L)[c] ^= np.uint32(1)  # +-1: never a multiple of p
            hit = coeff[:, j] % P != 0
            assert hit.any()
            em[o, hit], ef[o, hit] = 1, c
    assert_results(host(torch, raw_verify_batch(torch, plan, batch, to_dev(torch, h), to_dev(torch, h))), (em, ef))


def test_noncanonical_stored_word_is_a_mismatch(torch_dev, mode):
    """A stored p + 3 where 3 is computed counts; an input p + 3 with 3 stored does not."""
    torch = torch_dev
    from slime_amd import device as D
    lengths = [5, 1030, 257]
    places, size = packed_spans(lengths, 2, 1, start=3)
    rng = np.random.default_rng(5)
    h = np.full(size + 4, SENTINEL, dtype=np.uint32)
    em, ef = clean_results(len(lengths), 1)
    for o, (place, L) in enumerate(zip(places, lengths)):
        x = rng.integers(0, P, size=L, dtype=np.uint64).astype(np.uint32)
        x[L - 1], x[2] = 3, P + 3
        shard(h, place, 0, L)[:] = x
        shard(h, place, 1, L)[:] = x % np.uint32(P)  # row 0 = 1 * input 0, canonical
        shard(h, place, 1, L)[L - 1] = P + 3
        em[o, 0], ef[o, 0] = 1, L - 1
    plan = D.Plan.matrix(np.array([[1]], dtype=np.uint32), [0]).set_outputs([1])
    batch = in_place_batch(lengths, places, 1)
    want = expect_batch(plan.coefficients(), [0], [1], h, places, h, places, lengths)
    assert_results(want, (em, ef), "the oracle agrees with the planted expectation")
    buf = to_dev(torch, h)
    assert_results(host(torch, raw_verify_batch(torch, plan, batch, buf, buf)), (em, ef))


_corrupt = {}


def corruption_case(need, total):
    """A mixed-length batch, its oracle codewords, and two corrupted copies with numpy's results:
    about 1% of all words (inputs and stored rows alike) changed, and every stored word changed."""
    key = (need, total)
    if key not in _corrupt:
        T, C = geometry(need)
        rows = total - need
        lengths = [4 * C * T + 5, 3, T + 1, 0, 2 * C * T + 2, 257, C * T, 6]
        _, want, places, _ = encode_case(need, total, lengths, 1, seed=need * 2027 + total)
        rng = np.random.default_rng(need + 7 * total)
        some = want.copy()
        hit = rng.random(some.size) < 0.01
        some[hit] ^= rng.integers(1, 2**32, size=int(hit.sum()), dtype=np.uint64).astype(np.uint32)
        every = want.copy()
        for place, L in zip(places, lengths):
            for s in range(need, total):
                shard(every, place, s, L)[:] ^= np.uint32(0x10)
        coeff = OC.parity_matrix(need, rows)[need:]
        ins, outs = list(range(need)), list(range(need, total))
        res = [expect_batch(coeff, ins, outs, b, places, b, places, lengths) for b in (some, every)]
        assert res[0][0].sum() > 100 and [int(x) for x in res[1][0][:, 0]] == lengths
        _corrupt[key] = (lengths, places, (some, every), res)
    return _corrupt[key]


@pytest.mark.parametrize("need,total", [(3, 5), (8, 12), (10, 14), (16, 20), (17, 20)])
def test_random_and_total_corruption_match_numpy(torch_dev, mode, need, total):
    torch = torch_dev
    lengths, places, bufs, res = corruption_case(need, total)
    batch = in_place_batch(lengths, places, need)
    plan = encode_plan(need, total)
    for h, want in zip(bufs, res):
        buf = to_dev(torch, h)
        assert_results(host(torch, raw_verify_batch(torch, plan, batch, buf, buf)), want)
        assert np.array_equal(to_host(torch, buf), h)


# ------------------------------------------------------------------ the pipeline across objects

@pytest.mark.parametrize("need,total", [(3, 5), (8, 12), (10, 14), (16, 20)])
def test_every_pipelined_step_crosses_objects(torch_dev, mode, need, total):
    """Thirteen objects of exactly one tile; object o has o + 1 flipped words in row o % rows.
    Whenever a wave takes two units in a row, the step it compares and the step it loads belong to
    different objects: a tally credited to the walk's current object lands on the wrong one."""
    torch = torch_dev
    rows = total - need
    T, _ = geometry(need)
    lengths = [T] * 13
    _, want, places, _ = encode_case(need, total, lengths, 64, seed=1300 + need)
    h = want.copy()
    em, ef = clean_results(len(lengths), rows)
    rng = np.random.default_rng(need)
    for o in range(len(lengths)):
        cols = np.sort(rng.choice(T, size=o + 1, replace=False))
        shard(h, places[o], need + o % rows, T)[cols] ^= np.uint32(0x100)
        em[o, o % rows], ef[o, o % rows] = o + 1, cols[0]
    batch = in_place_batch(lengths, places, need)
    buf = to_dev(torch, h)
    assert_results(host(torch, raw_verify_batch(torch, encode_plan(need, total), batch, buf, buf)), (em, ef))


@pytest.mark.parametrize("need,total,nobj", [(3, 5, 1100), (8, 12, 1100), (16, 20, 4200)])
def test_waves_walk_units_of_different_objects(torch_dev, mode, need, total, nobj):
    """More one-unit objects (64 columns) than the static grid has waves (256 blocks of 4; 1024
    blocks for the one-vector steps of k > 12): every wave that takes a second unit compares a
    step of one object after issuing the loads of another.  Object o has 1 + o % 61 flipped words
    in row o % rows from column o % 3 on -- counts, rows and firsts differ between any two objects
    a wave takes in a row."""
    torch = torch_dev
    rows = total - need
    L = 64
    lengths = [L] * nobj
    assert nobj > (4096 if need > 12 else 1024)
    _, want, places, _ = encode_case(need, total, lengths, 1, seed=91 + need)
    h = want.copy()
    em, ef = clean_results(nobj, rows)
    for o in range(nobj):
        n, c0, i = 1 + o % 61, o % 3, o % rows
        shard(h, places[o], need + i, L)[c0:c0 + n] ^= np.uint32(4)
        em[o, i], ef[o, i] = n, c0
    batch = in_place_batch(lengths, places, need)
    assert batch.units == nobj
    buf = to_dev(torch, h)
    assert_results(host(torch, raw_verify_batch(torch, encode_plan(need, total), batch, buf, buf)), (em, ef))


# ------------------------------------------------------------------ layouts

@pytest.mark.parametrize("need,total", [(8, 12), (3, 5), (17, 20)])
def test_separate_cmp_tensor_with_its_own_spans(torch_dev, mode, need, total):
    """src holds the data shards packed with stride L; cmp is another tensor that holds only the
    parity rows, objects in reverse order behind a gap, odd shard strides (L rounded to 8, plus 1);
    the plan's outputs are cmp shards 0..rows-1."""
    torch = torch_dev
    from slime_amd import device as D
    rows = total - need
    T, C = geometry(need)
    lengths = [T + 1, 0, 3, C * T + 5, 257, 4] + [c + 1 for c in step_boundaries(need, rows)]
    _, want, src_places, _ = encode_case(need, total, lengths, 1, seed=177 + need)
    order = list(reversed(range(len(lengths))))
    cmp_places, off = [None] * len(lengths), 9
    for o in order:
        ss = -(-lengths[o] // 8) * 8 + 1
        cmp_places[o] = (off, ss)
        off += rows * ss + 3
    cmp_h = np.full(off + 4, SENTINEL, dtype=np.uint32)
    for o, L in enumerate(lengths):
        for i in range(rows):
            shard(cmp_h, cmp_places[o], i, L)[:] = shard(want, src_places[o], need + i, L)
    batch = D.Batch([(so, ss, do, ds, L) for (so, ss), (do, ds), L in zip(src_places, cmp_places, lengths)], need)
    plan = D.Plan.encode(need, total)  # outputs 0..rows-1
    src = to_dev(torch, want)
    assert_results(host(torch, raw_verify_batch(torch, plan, batch, src, to_dev(torch, cmp_h))),
                   clean_results(len(lengths), rows))
    em, ef = clean_results(len(lengths), rows)
    for o, L in enumerate(lengths):
        if L:
            shard(cmp_h, cmp_places[o], o % rows, L)[L - 1] ^= np.uint32(2)
            em[o, o % rows], ef[o, o % rows] = 1, L - 1
    cmp = to_dev(torch, cmp_h)
    assert_results(host(torch, plan.verify_batch(src, cmp, batch)), (em, ef))
    assert np.array_equal(to_host(torch, cmp), cmp_h) and np.array_equal(to_host(torch, src), want)


@pytest.mark.parametrize("need,total,have,want_rows", [(4, 6, [5, 2, 4, 1], [0, 3]), (8, 12, [11, 0, 9, 3, 4, 10, 6, 1],
                                                                                      [2, 5, 7])])
def test_reconstruct_plan_over_the_encode_plans_batch(torch_dev, mode, need, total, have, want_rows):
    """A reconstruct plan with shuffled survivors and data targets, its outputs set to the targets'
    own slots, over the batch the encode plan uses: the stored data shards are checked against
    what the survivors rebuild.  Data words the oracle's inputs hold at or above p are mismatches
    (the canonical residue is stored nowhere); numpy says which."""
    torch = torch_dev
    from slime_amd import device as D
    lengths = verify_lengths(need, len(want_rows))
    _, want, places, _ = encode_case(need, total, lengths, 1, seed=need * 2029 + total)
    h = want.copy()
    shard(h, places[len(lengths) - 1], want_rows[0], lengths[-1])[0] ^= np.uint32(1)
    plan = D.Plan.reconstruct(need, total, have, want_rows).set_outputs(want_rows)
    batch = in_place_batch(lengths, places, need)
    exp = expect_batch(plan.coefficients(), have, want_rows, h, places, h, places, lengths)
    assert exp[0][len(lengths) - 1, 0] >= 1
    buf = to_dev(torch, h)
    assert_results(host(torch, raw_verify_batch(torch, plan, batch, buf, buf)), exp)


# ------------------------------------------------------------------ the column form by alignment

@pytest.mark.parametrize("need,total", [(4, 6), (8, 12)])
@pytest.mark.parametrize("src_off,cmp_off", [(2, 0), (0, 2), (2, 2)])
def test_bases_not_word_aligned_take_the_column_form(torch_dev, mode, need, total, src_off, cmp_off):
    """src or cmp two bytes off a 4-byte boundary: every column runs one per lane, same answers."""
    torch = torch_dev
    rows = total - need
    lengths = verify_lengths(need, rows)
    _, want, places, _ = encode_case(need, total, lengths, 1, seed=need * 2039 + total)
    h = want.copy()
    em, ef = clean_results(len(lengths), rows)
    for o, L in enumerate(lengths):
        q = flip_positions(L, need, rows)
        if q:
            c = q[o % len(q)]
            shard(h, places[o], need + o % rows, L)[c] ^= np.uint32(0x400)
            em[o, o % rows], ef[o, o % rows] = 1, c

    def shifted(a, off):
        b = np.full(a.size * 4 + 8, 0xA5, dtype=np.uint8)
        b[off: off + a.size * 4] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        return torch.from_numpy(b).cuda()

    src, cmp = shifted(h, src_off), shifted(h, cmp_off)
    batch = in_place_batch(lengths, places, need)
    got = raw_verify_batch(torch, encode_plan(need, total), batch, src, cmp, src_off_bytes=src_off,
                           cmp_off_bytes=cmp_off)
    assert_results(host(torch, got), (em, ef))


# ------------------------------------------------------------------ more than 64 rows

_matrix = {}


def matrix_case(k, rows, lengths, seed):
    """A random rows x k matrix over random uint32 inputs: src (k shards an object, stride L) and
    cmp (rows shards an object) host buffers with the oracle's output rows stored."""
    key = (k, rows, tuple(lengths), seed)
    if key not in _matrix:
        rng = np.random.default_rng(seed)
        coeff = rng.integers(1, P, size=(rows, k), dtype=np.uint64).astype(np.uint32)
        src_places, ssize = packed_spans(lengths, k, 1, start=3)
        cmp_places, csize = packed_spans(lengths, rows, 1, start=5)
        src = np.full(ssize + 4, SENTINEL, dtype=np.uint32)
        cmp = np.full(csize + 4, SENTINEL, dtype=np.uint32)
        for sp, cp, L in zip(src_places, cmp_places, lengths):
            if L:
                x = rng.integers(0, 2**32, size=(k, L), dtype=np.uint64).astype(np.uint32)
                for j in range(k):
                    shard(src, sp, j, L)[:] = x[j]
                for i, r in enumerate(OC.apply_matrix(coeff, list(x))):
                    shard(cmp, cp, i, L)[:] = r
        src.setflags(write=False)
        cmp.setflags(write=False)
        _matrix[key] = (coeff, src, src_places, cmp, cmp_places)
    return _matrix[key]


@pytest.mark.parametrize("k,rows,L", [(3, 70, 1031), (8, 129, 515)])
def test_plans_of_more_than_64_rows(torch_dev, mode, k, rows, L):
    """Row blocks of 64, each a launch of its own: coefficient rows, output shards and result
    entries are offset per block."""
    torch = torch_dev
    from slime_amd import device as D
    lengths = [L, 5, 0, L - 4]
    coeff, src_h, src_places, cmp_h, cmp_places = matrix_case(k, rows, lengths, seed=rows * 7 + k)
    plan = D.Plan.matrix(coeff, list(range(k)))
    batch = D.Batch([(so, ss, do, ds, n) for (so, ss), (do, ds), n in zip(src_places, cmp_places, lengths)], k)
    src = to_dev(torch, src_h)
    assert_results(host(torch, raw_verify_batch(torch, plan, batch, src, to_dev(torch, cmp_h))),
                   clean_results(len(lengths), rows))
    h = cmp_h.copy()
    for o, i, c in ((0, 0, 1), (0, 63, L - 1), (3, 64, 0), (3, 64, 700 % (L - 4)), (0, 65, L - 2), (1, 64, 4),
                    (3, rows - 1, L // 2), (1, rows - 1, 0)):
        shard(h, cmp_places[o], i, lengths[o])[c] ^= np.uint32(0x20)
    shard(h, cmp_places[3], rows - 2, L - 4)[:] ^= np.uint32(1)  # a whole row of the last block
    exp = expect_batch(coeff, list(range(k)), list(range(rows)), src_h, src_places, h, cmp_places, lengths)
    assert exp[0][3, 64] == 2 and exp[0][3, rows - 2] == L - 4 and exp[0].sum() == L - 4 + 8
    assert_results(host(torch, raw_verify_batch(torch, plan, batch, src, to_dev(torch, h))), exp)


# ------------------------------------------------------------------ result arrays, launched mark

def test_results_are_initialised_for_empty_objects_and_untouched_for_no_objects(torch_dev, mode):
    torch = torch_dev
    from slime_amd import device as D
    plan = encode_plan(4, 6)
    buf = to_dev(torch, np.full(64, SENTINEL, dtype=np.uint32))
    for spans in ([(0, 0, 0, 0, 0)] * 7, [(10**9, 8, 10**9, 8, 0)]):  # empty batches with objects
        batch = D.Batch(spans, 4)
        dyn0 = N.schedule_counts(0)
        assert_results(host(torch, raw_verify_batch(torch, plan, batch, buf, buf)), clean_results(len(spans), 2))
        assert_results(host(torch, plan.verify_batch(buf, buf, batch)), clean_results(len(spans), 2))
        assert N.schedule_counts(0) == dyn0, "an empty batch launches nothing but the initialisation"
    # L == 0 objects among others keep their initial values
    lengths = [0, 9, 0, 4, 0]
    _, want, places, _ = encode_case(4, 6, lengths, 1, seed=404)
    full = to_dev(torch, want)
    assert_results(host(torch, raw_verify_batch(torch, plan, in_place_batch(lengths, places, 4), full, full)),
                   clean_results(5, 2))
    # nobj == 0: returns 0 and touches nothing
    none = D.Batch([], 4)
    g = torch.full((4,), GARBAGE, dtype=torch.int64, device="cuda")
    h = g.clone()
    p = ctypes.c_void_p(buf.data_ptr())
    assert N.lib.slime_rs_plan_verify_batch(plan._h, none._h, p, p, ctypes.c_void_p(g.data_ptr()),
                                            ctypes.c_void_p(h.data_ptr()), None) == 0
    torch.cuda.synchronize()
    assert (g == GARBAGE).all() and (h == GARBAGE).all()
    m, f = plan.verify_batch(buf, buf, none)
    assert m.shape == f.shape == (0, 2)
    assert (to_host(torch, buf) == SENTINEL).all()


def test_refusals_and_the_launched_mark(torch_dev):
    torch = torch_dev
    from slime_amd import device as D
    lengths = [16, 5]
    _, want, places, _ = encode_case(4, 6, lengths, 1, seed=405)
    buf = to_dev(torch, want)
    batch = in_place_batch(lengths, places, 4)
    plan = D.Plan.encode(4, 6).set_outputs([4, 5])
    res = torch.full((4,), GARBAGE, dtype=torch.int64, device="cuda")
    p, r = ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(res.data_ptr())
    for args in ((None, batch._h, p, p, r, r), (plan._h, None, p, p, r, r), (plan._h, batch._h, None, p, r, r),
                 (plan._h, batch._h, p, None, r, r), (plan._h, batch._h, p, p, None, r),
                 (plan._h, batch._h, p, p, r, None)):
        assert N.lib.slime_rs_plan_verify_batch(*args, None) == N.ERR_INVALID_ARG
        assert "plan_verify_batch" in N.lib.slime_rs_last_error().decode()
    other = D.Plan.encode(5, 7)
    assert N.lib.slime_rs_plan_verify_batch(other._h, batch._h, p, p, r, r, None) == N.ERR_INVALID_ARG
    with pytest.raises(ValueError, match="batch is for k"):
        other.verify_batch(buf, buf, batch)
    with pytest.raises(ValueError, match="addresses element"):
        plan.verify_batch(buf, buf[:-6].contiguous(), batch)  # one element short of the last parity shard
    torch.cuda.synchronize()
    assert (res == GARBAGE).all(), "a refused call touches nothing"
    plan.set_outputs([4, 5])  # refusals do not mark the plan
    assert_results(host(torch, plan.verify_batch(buf, buf, batch)), clean_results(2, 2))
    with pytest.raises(N.NativeError, match="already launched"):
        plan.set_outputs([0, 1])


# ------------------------------------------------------------------ equal to the uniform call

@pytest.mark.parametrize("need,total", [(3, 5), (8, 12), (16, 20), (17, 20)])
def test_uniform_layout_equals_plan_verify(torch_dev, mode, need, total):
    torch = torch_dev
    from slime_amd import device as D
    T, _ = geometry(need)
    L, nobj = 3 * T + 5, 5
    rng = np.random.default_rng(need + 61)
    h = symbols(rng, (nobj, total, L))
    for o in range(nobj):
        ref = np.ascontiguousarray(h[o])
        OC.encode_object(ref, need, total)
        h[o] = ref
    hit = rng.random(h.shape) < 0.01
    h[hit] ^= np.uint32(0x8000)
    plan = encode_plan(need, total)
    lay = D.layout_of(total, L)
    buf = to_dev(torch, h)
    batch = D.Batch([(o * total * L, L, o * total * L, L, L) for o in range(nobj)], need)
    a = host(torch, plan.verify_batch(buf, buf, batch))
    b = host(torch, plan.verify(buf, lay, buf, lay, L, nobj))
    assert a[0].sum() > 0
    assert_results(a, b)
    cnt, first = expected(plan.coefficients(), list(h[2, :need]), list(h[2, need:]))
    assert np.array_equal(a[0][2], cnt) and np.array_equal(a[1][2], first)


# ------------------------------------------------------------------ streams, graphs, counter sets

def stream_case(need, total):
    T, C = geometry(need)
    lengths = [4 * C * T + 5, 3, T + 1, 0, 256, C * T] * 2
    _, want, places, _ = encode_case(need, total, lengths, 1, seed=33)
    return lengths, want, places


def test_non_default_stream(torch_dev, mode):
    torch = torch_dev
    need, total = 8, 12
    lengths, want, places = stream_case(need, total)
    h = want.copy()
    shard(h, places[5], need + 1, lengths[5])[77] ^= np.uint32(1)
    em, ef = clean_results(len(lengths), total - need)
    em[5, 1], ef[5, 1] = 1, 77
    plan = encode_plan(need, total)
    batch = in_place_batch(lengths, places, need)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        buf = to_dev(torch, h)
        res = raw_verify_batch(torch, plan, batch, buf, buf, stream=s)
        res2 = plan.verify_batch(buf, buf, batch)  # the current stream is `s`
    s.synchronize()
    assert_results(host(torch, res), (em, ef))
    assert_results(host(torch, res2), (em, ef))


@pytest.mark.parametrize("sched", [1, 2])
@pytest.mark.parametrize("need,total", [(4, 6), (17, 20)])
def test_graph_captured_verify_replays_from_a_clean_state(torch_dev, sched, need, total):
    """A captured ragged verify replayed twice with a word flipped in between: each replay
    re-initialises the results, the second shows only the new state.  Mode 1 captures the static
    form (no counter set), mode 2 the dynamic one, which holds its set for the graph's life."""
    torch = torch_dev
    s0 = N.lib.slime_rs_kernel_schedule(-1)
    assert N.lib.slime_rs_kernel_schedule(sched) == 0
    try:
        rows = total - need
        lengths, want, places = stream_case(need, total)
        batch = in_place_batch(lengths, places, need)
        plan = encode_plan(need, total)
        h = want.copy()
        shard(h, places[2], need, lengths[2])[5] ^= np.uint32(8)
        buf = to_dev(torch, h)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):  # warm the launch path outside the capture
            plan.verify_batch(buf, buf, batch, stream=s)
        torch.cuda.synchronize()
        _, held0 = N.ticket_sets(0)
        dyn0, _ = N.schedule_counts(0)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            gm, gf_ = plan.verify_batch(buf, buf, batch, stream=s)
        torch.cuda.synchronize()
        _, held1 = N.ticket_sets(0)
        dyn1, _ = N.schedule_counts(0)
        if sched == 2 and need <= 16:
            assert (held1 - held0, dyn1 - dyn0) == (1, 1), "the captured launch took the dynamic schedule"
        else:
            assert (held1 - held0, dyn1 - dyn0) == (0, 0), "the captured launch took a static form"
        gm.fill_(GARBAGE)
        gf_.fill_(GARBAGE)
        torch.cuda.synchronize()
        g.replay()
        em, ef = clean_results(len(lengths), rows)
        em[2, 0], ef[2, 0] = 1, 5
        assert_results(host(torch, (gm, gf_)), (em, ef))
        h2 = want.copy()  # repaired, and two new ones elsewhere
        shard(h2, places[0], need + rows - 1, lengths[0])[[9, lengths[0] - 1]] ^= np.uint32(8)
        buf.copy_(to_dev(torch, h2))
        torch.cuda.synchronize()
        g.replay()
        em, ef = clean_results(len(lengths), rows)
        em[0, rows - 1], ef[0, rows - 1] = 2, 9
        assert_results(host(torch, (gm, gf_)), (em, ef))
        del g  # before the batch: the graph's kernel nodes read its tables
        torch.cuda.synchronize()
    finally:
        N.lib.slime_rs_kernel_schedule(s0)


def test_dynamic_verify_leaves_its_counter_set_zero(torch_dev, mode):
    """test_gpu_ragged's check for the verify launch: in schedule mode 1 (and 2) outside a capture
    it takes the dynamic path; after a synchronize no counter set is held; and a uniform
    plan_execute that follows on the same stream -- it may draw the same set -- is still exact,
    so the verify kernel left the set zero.  The static modes must not touch a set."""
    torch = torch_dev
    from slime_amd import device as D
    sched, pipe = mode
    need, total = 4, 6
    T, C = geometry(need)
    lengths = [4 * C * T + 5, T, 5, 0, 3 * C * T, 257] * 8  # 88 units
    _, want, places, _ = encode_case(need, total, lengths, 1, seed=4242)
    batch = in_place_batch(lengths, places, need)
    assert batch.units > 64
    plan = encode_plan(need, total)
    torch.cuda.synchronize()
    _, held0 = N.ticket_sets(0)
    dyn0, fb0 = N.schedule_counts(0)
    buf = to_dev(torch, want)
    res = [raw_verify_batch(torch, plan, batch, buf, buf) for _ in range(3)]  # back to back: each finds a zero set
    dyn1, fb1 = N.schedule_counts(0)
    if sched in (1, 2) and pipe == 1:
        assert (dyn1 - dyn0, fb1 - fb0) == (3, 0), "ragged verify outside a capture takes the dynamic path"
    else:
        assert (dyn1 - dyn0, fb1 - fb0) == (0, 0), "static modes ask for no counter set"
    # a uniform launch next on the same stream
    L, nobj = 5 * 4 * 3 * 1024 + 5, 6
    h = symbols(np.random.default_rng(99), (nobj, total, L))
    ubuf = to_dev(torch, h)
    lay = D.layout_of(total, L)
    plan(ubuf, lay, ubuf, lay, L, nobj)
    for r in res:
        assert_results(host(torch, r), clean_results(len(lengths), total - need))
    ref = np.ascontiguousarray(h.transpose(1, 0, 2).reshape(total, nobj * L))
    OC.encode_object(ref, need, total)
    assert np.array_equal(to_host(torch, ubuf).reshape(nobj, total, L), ref.reshape(total, nobj, L).transpose(1, 0, 2))
    assert N.ticket_sets(0)[1] == held0, "nothing is held after the launches finished"
