"""Ragged batches (slime_rs_batch_create, slime_rs_plan_execute_batch) on the GPU.

Every expectation comes from the C oracle, applied object by object to host
copies: OC.encode_object for the encode plans, OC.apply_matrix over
plan.coefficients() for the reconstruct plans (whose rows are checked against
the oracle's codeword) -- never from a kernel under test.  Buffers are filled
with a sentinel before the data goes in, and whole buffers are compared, so
every assertion also proves that nothing outside the objects' output columns
was written.  References are computed once per shape and shared by the
schedule / pipeline modes.
"""
import ctypes

import numpy as np
import pytest

from slime_amd import _native as N
from slime_amd import gf
from oracle import oracle_c as OC

pytestmark = pytest.mark.gpu

P = gf.MaxVal
SENTINEL = 0xA5C3F00D
CODES = [(1, 2), (3, 5), (4, 6), (8, 12), (10, 14), (16, 20), (17, 20), (33, 50)]
EDGES = np.array([0, 1, 2, P - 1, P, P + 1, P + 4, 0xFFFFFFFF, 0x7FFFFFFF, 0x80000000], dtype=np.uint32)


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    assert N.device_count() > 0
    return torch


MODES = [(1, 1), (0, 1), (2, 1), (1, 0), (0, 0), (2, 0)]


@pytest.fixture(params=MODES, ids=[f"schedule{s}-pipeline{p}" for s, p in MODES])
def mode(request):
    """slime_rs_kernel_schedule x slime_rs_kernel_pipeline, restored afterwards.  Pipeline 0 runs
    the static walk one tile at a time whatever the schedule; shapes that take the column form
    (k > 16) run it in every mode and are asserted all the same."""
    sched, pipe = request.param
    s0, p0 = N.lib.slime_rs_kernel_schedule(-1), N.lib.slime_rs_kernel_pipeline(-1)
    assert N.lib.slime_rs_kernel_schedule(sched) == 0 and N.lib.slime_rs_kernel_pipeline(pipe) == 0
    yield request.param
    N.lib.slime_rs_kernel_schedule(s0)
    N.lib.slime_rs_kernel_pipeline(p0)


def geometry(k):
    """(T, C): a tile's columns 256 U and a unit's tiles (ragged_plan.hpp, geometry_for_k)."""
    if k <= 4:
        return 1024, 3
    if k <= 12:
        return 768, 2
    return 256, 6


def boundary_lengths(k):
    """The boundaries of a vector, a wave, a tile, a unit and a group of four units."""
    T, C = geometry(k)
    return [0, 1, 3, 4, 5, 255, 256, 257, T - 1, T, T + 1, C * T - 1, C * T, C * T + 1, 4 * C * T + 5]


def units_of(L, k):
    """Units of an object of L columns: its whole vectors' tiles in groups of C."""
    T, C = geometry(k)
    tiles = -(-(L // 4 * 4) // T)
    return -(-tiles // C)


def symbols(rng, shape):
    a = rng.integers(0, P, size=shape, dtype=np.uint64).astype(np.uint32)
    flat = a.reshape(-1)
    n = min(flat.size, EDGES.size)
    if n:
        flat[rng.choice(flat.size, size=n, replace=False)] = EDGES[:n]  # non-canonical inputs too
    return a


def packed_spans(lengths, nshards, align, start=0):
    """Batch.packed's layout, restated: [(offset, shard stride)] per object and the total."""
    out, off = [], start
    for L in lengths:
        ss = -(-L // align) * align
        out.append((off, ss))
        off += nshards * ss
    return out, off


def shard(buf, place, s, L):
    off, ss = place
    return buf[off + s * ss: off + s * ss + L]


def to_dev(torch, a):
    return torch.from_numpy(np.array(a, dtype=np.uint32).view(np.int32).reshape(-1)).cuda()  # a writable copy


def to_host(torch, t):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint32)


_cases = {}


def encode_case(need, total, lengths, align, seed):
    """(init, want, places, size): a sentinel-filled packed buffer with random data shards, and
    the same buffer with every object's parity shards as the oracle encodes them.  Cached."""
    key = (need, total, tuple(lengths), align, seed)
    if key not in _cases:
        rng = np.random.default_rng(seed)
        # guard words ahead: 3 with align 1 (bases 4- but not 16-byte aligned), a whole 256 bytes otherwise
        places, size = packed_spans(lengths, total, align, start=3 if align == 1 else 64)
        init = np.full(size + 5, SENTINEL, dtype=np.uint32)
        for place, L in zip(places, lengths):
            data = symbols(rng, (need, L))
            for s in range(need):
                shard(init, place, s, L)[:] = data[s]
        want = init.copy()
        for place, L in zip(places, lengths):
            if L == 0:
                continue
            obj = np.zeros((total, L), dtype=np.uint32)
            for s in range(need):
                obj[s] = shard(init, place, s, L)
            OC.encode_object(obj, need, total)
            for s in range(need, total):
                shard(want, place, s, L)[:] = obj[s]
        init.setflags(write=False)
        want.setflags(write=False)
        _cases[key] = (init, want, places, size + 5)
    return _cases[key]


def encode_plan(need, total):
    """The encode plan writing parity into the object's own slots need..total-1; its rows are
    the oracle's parity rows."""
    from slime_amd import device as D
    plan = D.Plan.encode(need, total).set_outputs(list(range(need, total)))
    assert np.array_equal(plan.coefficients(), OC.parity_matrix(need, total - need)[need:])
    return plan


def in_place_batch(lengths, places, k):
    from slime_amd import device as D
    return D.Batch([(off, ss, off, ss, L) for (off, ss), L in zip(places, lengths)], k)


def run_in_place(torch, need, total, lengths, align, seed, stream=None):
    init, want, places, _ = encode_case(need, total, lengths, align, seed)
    batch = in_place_batch(lengths, places, need)
    assert (batch.nobj, batch.columns) == (len(lengths), sum(lengths))
    buf = to_dev(torch, init)
    encode_plan(need, total).execute_batch(buf, buf, batch, stream=stream)
    got = to_host(torch, buf)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad[:8], got[bad[:8]], want[bad[:8]])
    return batch


# ------------------------------------------------------------------ lengths and guard words

@pytest.mark.parametrize("align", [1, 64])
@pytest.mark.parametrize("need,total", CODES)
def test_every_boundary_length_in_place(torch_dev, mode, need, total, align):
    """One batch of objects at every boundary length, shuffled, packed with shard strides of
    exactly L (align 1: most objects start 4- but not 16-byte aligned) and of L rounded to 64;
    encoded in place.  The whole buffer is compared: every parity symbol, and the data shards,
    each shard's padding, the words between, before and after the objects unchanged."""
    lengths = boundary_lengths(need)
    np.random.default_rng(need * 131 + total).shuffle(lengths)
    batch = run_in_place(torch_dev, need, total, lengths, align, seed=need * 1009 + total)
    assert batch.units == sum(units_of(L, need) for L in lengths)


def test_packed_constructor_matches_the_layout(torch_dev):
    """Batch.packed places objects as packed_spans does (the tests' own restatement)."""
    from slime_amd import device as D
    lengths = [5, 0, 64, 65, 1000]
    for align in (1, 64):
        batch, total = D.Batch.packed(lengths, 5, 3, align=align)
        places, size = packed_spans(lengths, 5, align)
        assert total == size
        assert [(int(r[0]), int(r[1])) for r in batch.spans] == places
        assert [(int(r[2]), int(r[3]), int(r[4])) for r in batch.spans] == [(o, s, L) for (o, s), L in
                                                                          zip(places, lengths)]


# ------------------------------------------------------------------ reconstruct, one batch for a code's plans

@pytest.mark.parametrize("need,total,erase", [(8, 12, [0, 3, 8, 11]), (3, 5, [1, 4])])
def test_reconstruct_into_a_separate_layout_with_the_encode_plans_batch(torch_dev, mode, need, total, erase):
    """src holds full codewords packed with stride L; dst is another tensor with other offsets
    (objects in reverse order, a gap ahead) and strides (L rounded to 8).  One Batch serves the
    encode plan (parity rows to dst shards 0..rows-1) and the reconstruct plan over a mixed
    erasure pattern with a parity target (erased rows to dst shards 0..nwant-1): the binding is
    to k.  A plan with another k is refused."""
    torch = torch_dev
    from slime_amd import device as D
    rows = total - need
    assert len(erase) == rows  # both plans write the same dst shards
    T, C = geometry(need)
    lengths = [T + 1, 0, 3, C * T + 5, 257, 4]
    init, want, src_places, _ = encode_case(need, total, lengths, 1, seed=77 + need)
    order = list(reversed(range(len(lengths))))
    rev_places, dst_size = packed_spans([lengths[o] for o in order], rows, 8, start=9)
    dst_places = [None] * len(lengths)
    for place, o in zip(rev_places, order):
        dst_places[o] = place
    batch = D.Batch([(so, ss, do, ds, L) for (so, ss), (do, ds), L in zip(src_places, dst_places, lengths)], need)
    have = [i for i in range(total) if i not in erase][:need]

    def expect(row_of):
        w = np.full(dst_size + 4, SENTINEL, dtype=np.uint32)
        for place, splace, L in zip(dst_places, src_places, lengths):
            for i in range(rows):
                shard(w, place, i, L)[:] = row_of(splace, i, L)
        return w

    # encode: dst shard i = parity row need + i (the oracle's, from encode_case)
    enc = D.Plan.encode(need, total)
    dst = to_dev(torch, np.full(dst_size + 4, SENTINEL, dtype=np.uint32))
    src = to_dev(torch, init)
    enc.execute_batch(src, dst, batch)
    assert np.array_equal(to_host(torch, dst), expect(lambda sp, i, L: shard(want, sp, need + i, L)))
    assert np.array_equal(to_host(torch, src), init), "src is only read"
    # reconstruct: dst shard i = codeword row erase[i], from the survivors alone
    rec = D.Plan.reconstruct(need, total, have, erase)
    coeff = rec.coefficients()
    full = to_dev(torch, want)  # whole codewords; the erased shards are never read
    dst = to_dev(torch, np.full(dst_size + 4, SENTINEL, dtype=np.uint32))
    rec.execute_batch(full, dst, batch)
    got = to_host(torch, dst)

    def rebuilt(sp, i, L):
        if L == 0:
            return np.zeros(0, dtype=np.uint32)
        r = OC.apply_matrix(coeff, [shard(want, sp, s, L) for s in have])[i]
        assert np.array_equal(r, shard(want, sp, erase[i], L) % np.uint32(P) if erase[i] < need
                              else shard(want, sp, erase[i], L)), "the plan's rows rebuild the oracle's codeword"
        return r

    assert np.array_equal(got, expect(rebuilt))
    # another k: refused by the wrapper and by the C call
    other = D.Plan.encode(need + 1, total + 1)
    with pytest.raises(ValueError, match="batch is for k"):
        other.execute_batch(src, dst, batch)
    rc = N.lib.slime_rs_plan_execute_batch(other._h, batch._h, ctypes.c_void_p(src.data_ptr()),
                                           ctypes.c_void_p(dst.data_ptr()), None)
    assert rc == N.ERR_INVALID_ARG and "plan_execute_batch" in N.lib.slime_rs_last_error().decode()
    assert np.array_equal(to_host(torch, dst), got), "a refused launch writes nothing"


# ------------------------------------------------------------------ counter sets and the schedule taken

def test_dynamic_launch_leaves_its_counter_set_zero(torch_dev, mode):
    """In schedule mode 1 (and 2) outside a capture the ragged launch takes the dynamic path
    (slime_rs_schedule_counts); after a synchronize no counter set is held; and a uniform
    plan_execute that follows on the same stream -- it may draw the same set -- is still exact,
    so the ragged kernel left the set zero.  The static modes must not touch a set."""
    torch = torch_dev
    from slime_amd import device as D
    sched, pipe = mode
    need, total = 4, 6
    T, C = geometry(need)
    lengths = [4 * C * T + 5, T, 5, 0, 3 * C * T, 257] * 8  # 88 units
    init, want, places, _ = encode_case(need, total, lengths, 1, seed=4242)
    batch = in_place_batch(lengths, places, need)
    assert batch.units > 64
    plan = encode_plan(need, total)
    torch.cuda.synchronize()
    _, held0 = N.ticket_sets(0)
    dyn0, fb0 = N.schedule_counts(0)
    buf = to_dev(torch, init)
    for _ in range(3):  # back to back: each launch finds a zero set
        plan.execute_batch(buf, buf, batch)
    dyn1, fb1 = N.schedule_counts(0)
    if sched in (1, 2) and pipe == 1:
        assert (dyn1 - dyn0, fb1 - fb0) == (3, 0), "ragged launches outside a capture take the dynamic path"
    else:
        assert (dyn1 - dyn0, fb1 - fb0) == (0, 0), "static modes ask for no counter set"
    # a uniform launch next on the same stream
    L, nobj = 5 * 4 * 3 * 1024 + 5, 6
    rng = np.random.default_rng(99)
    h = symbols(rng, (nobj, total, L))
    ubuf = to_dev(torch, h)
    lay = D.layout_of(total, L)
    plan(ubuf, lay, ubuf, lay, L, nobj)
    assert np.array_equal(to_host(torch, buf), want)
    ref = np.ascontiguousarray(h.transpose(1, 0, 2).reshape(total, nobj * L))
    OC.encode_object(ref, need, total)
    assert np.array_equal(to_host(torch, ubuf).reshape(nobj, total, L), ref.reshape(total, nobj, L).transpose(1, 0, 2))
    assert N.ticket_sets(0)[1] == held0, "nothing is held after the launches finished"


# ------------------------------------------------------------------ equal to the uniform launch

@pytest.mark.parametrize("need,total", [(3, 5), (8, 12), (16, 20), (17, 20)])
def test_uniform_layout_is_bit_identical_to_plan_execute(torch_dev, mode, need, total):
    torch = torch_dev
    from slime_amd import device as D
    T, _ = geometry(need)
    L, nobj = 3 * T + 5, 5
    h = symbols(np.random.default_rng(need + 31), (nobj, total, L))
    plan = encode_plan(need, total)
    lay = D.layout_of(total, L)
    a, b = to_dev(torch, h), to_dev(torch, h)
    batch = D.Batch([(o * total * L, L, o * total * L, L, L) for o in range(nobj)], need)
    plan.execute_batch(a, a, batch)
    plan(b, lay, b, lay, L, nobj)
    ga, gb = to_host(torch, a), to_host(torch, b)
    assert np.array_equal(ga, gb)
    ref = np.ascontiguousarray(h[2].copy())
    OC.encode_object(ref, need, total)
    assert np.array_equal(ga.reshape(nobj, total, L)[2], ref)


# ------------------------------------------------------------------ shapes of real batches

@pytest.mark.parametrize("need,total", [(3, 5), (8, 12), (17, 20)])
def test_many_tiny_objects(torch_dev, mode, need, total):
    """5000 objects of 1 to 9 columns: more units and more tail items than waves."""
    lengths = [int(x) for x in np.random.default_rng(need).integers(1, 10, size=5000)]
    batch = run_in_place(torch_dev, need, total, lengths, 1, seed=5000 + need)
    assert batch.units == sum(1 for L in lengths if L >= 4) > 2 * 1024  # over twice the dynamic grid's waves


@pytest.mark.parametrize("need,total", [(3, 5), (8, 12), (17, 20)])
def test_one_large_object_among_small_ones(torch_dev, mode, need, total):
    """One object of 64 tiles among 63 of 5 columns: the large one's units spread over many
    waves while the tails belong to the others."""
    T, C = geometry(need)
    lengths = [5] * 63
    lengths.insert(20, 64 * T)
    batch = run_in_place(torch_dev, need, total, lengths, 1, seed=640 + need)
    assert batch.units == 63 + units_of(64 * T, need)


def test_empty_batches_launch_nothing(torch_dev, mode):
    torch = torch_dev
    from slime_amd import device as D
    plan = encode_plan(3, 5)
    buf = to_dev(torch, np.full(64, SENTINEL, dtype=np.uint32))
    for spans in ([], [(0, 0, 0, 0, 0)] * 7, [(10**9, 8, 10**9, 8, 0)]):
        batch = D.Batch(spans, 3)
        assert (batch.nobj, batch.columns, batch.units) == (len(spans), 0, 0)
        dyn0 = N.schedule_counts(0)
        plan.execute_batch(buf, buf, batch)
        assert N.lib.slime_rs_plan_execute_batch(plan._h, batch._h, None, None, None) == 0  # not even buffers
        assert N.schedule_counts(0) == dyn0
    assert (to_host(torch, buf) == SENTINEL).all()


# ------------------------------------------------------------------ streams and graphs

def test_non_default_stream(torch_dev, mode):
    torch = torch_dev
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    lengths = boundary_lengths(8)
    with torch.cuda.stream(s):
        run_in_place(torch, 8, 12, lengths, 1, seed=812, stream=s)


@pytest.mark.parametrize("sched", [1, 2])
@pytest.mark.parametrize("need,total", [(4, 6), (17, 20)])
def test_graph_captured_launch_replays_exactly(torch_dev, sched, need, total):
    """A captured ragged launch replayed twice with the input changed in between: both replays
    exact.  Mode 1 captures the static form (no counter set), mode 2 the dynamic one, which holds
    its set for the graph's life and leaves it zero after every replay."""
    torch = torch_dev
    s0 = N.lib.slime_rs_kernel_schedule(-1)
    assert N.lib.slime_rs_kernel_schedule(sched) == 0
    try:
        T, C = geometry(need)
        lengths = [4 * C * T + 5, 3, T + 1, 0, 256, C * T] * 2
        cases = [encode_case(need, total, lengths, 1, seed=sd) for sd in (31, 32)]
        places = cases[0][2]
        batch = in_place_batch(lengths, places, need)
        plan = encode_plan(need, total)
        buf = to_dev(torch, cases[0][0])
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):  # warm the launch path outside the capture
            plan.execute_batch(buf, buf, batch, stream=s)
        torch.cuda.synchronize()
        _, held0 = N.ticket_sets(0)
        dyn0, fb0 = N.schedule_counts(0)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            plan.execute_batch(buf, buf, batch, stream=s)
        torch.cuda.synchronize()
        _, held1 = N.ticket_sets(0)
        dyn1, _ = N.schedule_counts(0)
        if sched == 2 and need <= 16:
            assert (held1 - held0, dyn1 - dyn0) == (1, 1), "the captured launch took the dynamic schedule"
        else:
            assert (held1 - held0, dyn1 - dyn0) == (0, 0), "the captured launch took a static form"
        for init, want, _, _ in (cases[1], cases[0]):
            buf.copy_(to_dev(torch, init))
            torch.cuda.synchronize()
            g.replay()
            assert np.array_equal(to_host(torch, buf), want)
        del g  # before the batch: the graph's kernel node reads its tables
        torch.cuda.synchronize()
    finally:
        N.lib.slime_rs_kernel_schedule(s0)
