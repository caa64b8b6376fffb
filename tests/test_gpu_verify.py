"""Device-side verify (slime_rs_plan_verify, slime_rs_verify_objects) on the GPU.

Every expectation is computed on the CPU: stored shards come from the C
oracle (encode_object / create_parity / apply_matrix over the plan's
coefficient rows) and counts and first columns from numpy over host copies --
never from the kernels under test.  Except where a test is about the Python
wrappers' own tensors, the result arrays are filled with garbage before the
call, so every assertion also proves that the call initialises them.
"""
import ctypes

import numpy as np
import pytest

from slime_amd import _native as N
from slime_amd import gf
from oracle import oracle_c as OC
from oracle import oracle_py as OP

pytestmark = pytest.mark.gpu

P = gf.MaxVal
EDGES = np.array([0, 1, 2, P - 1, P, P + 1, P + 4, 0xFFFFFFFF, 0x7FFFFFFF, 0x80000000], dtype=np.uint32)
GARBAGE = 0x5A5A5A5A5A5A5A5A
CODES = [(1, 2), (3, 5), (4, 6), (8, 12), (10, 14), (16, 20), (17, 20), (33, 50)]


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    assert N.device_count() > 0
    return torch


@pytest.fixture(params=[1, 0], ids=["pipelined", "offsets64"])
def pipeline(request):
    """The vector verify kernel's two forms (slime_rs_kernel_pipeline): shapes
    the pipelined form does not take (k > 16, unaligned bases) run the form
    that applies in both settings, and are asserted all the same."""
    before = N.lib.slime_rs_kernel_pipeline(-1)
    assert N.lib.slime_rs_kernel_pipeline(request.param) == 0
    yield request.param
    N.lib.slime_rs_kernel_pipeline(before)


def tile_cols(k, rows):
    """Columns of one wave's tile, 256 * U (rs_verify.hip verify_unroll_c: about 24
    vectors of inputs and stored rows a lane); a block's 256 for the column form."""
    if k > 16:
        return 256
    return 256 * min(4, max(1, 24 // (k + (2 if rows <= 2 else 4))))


def lengths(k, rows):
    T = tile_cols(k, rows)
    return [1, 3, 4, 5, 255, 256, 257, T - 1, T, T + 1, 3 * T + 5]


def encoded(need, total, L, nobj, seed, stride=None):
    """[nobj][total][stride] uint32, columns [0, L) encoded by the oracle, the
    rest (shard padding) random."""
    rng = np.random.default_rng(seed)
    ss = L if stride is None else stride
    a = rng.integers(0, P, size=(nobj, total, ss), dtype=np.uint64).astype(np.uint32)
    # one oracle call: the objects side by side as one object of nobj * L columns
    wide = np.ascontiguousarray(a[:, :, :L].transpose(1, 0, 2).reshape(total, nobj * L))
    OC.encode_object(wide, need, total)
    a[:, :, :L] = wide.reshape(total, nobj, L).transpose(1, 0, 2)
    return a


def to_dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).reshape(-1)).cuda()


def raw_verify(torch, plan, src, src_lay, cmp, cmp_lay, L, nobj, src_offset=0, cmp_offset=0, stream=None):
    """slime_rs_plan_verify into result arrays pre-filled with garbage."""
    from slime_amd import device as D
    mism = torch.full((nobj, plan.rows), GARBAGE, dtype=torch.int64, device="cuda")
    first = torch.full((nobj, plan.rows), GARBAGE, dtype=torch.int64, device="cuda")
    N.check(N.lib.slime_rs_plan_verify(plan._h, ctypes.c_void_p(src.data_ptr() + 4 * src_offset), src_lay,
                                       ctypes.c_void_p(cmp.data_ptr() + 4 * cmp_offset), cmp_lay, L, nobj,
                                       ctypes.c_void_p(mism.data_ptr()), ctypes.c_void_p(first.data_ptr()),
                                       D._stream_handle(0, stream)))
    return mism, first


def host(torch, res):
    torch.cuda.synchronize()
    return res[0].cpu().numpy(), res[1].cpu().numpy()


def assert_clean(torch, res, what=None):
    m, f = host(torch, res)
    assert not m.any(), (what, m)
    assert (f == -1).all(), (what, f)


def expected(coeff, ins, stored):
    """Counts and first columns of one object: oracle rows over `ins` against `stored`."""
    want = OC.apply_matrix(coeff, ins)
    cnt = np.zeros(len(stored), dtype=np.int64)
    first = np.full(len(stored), -1, dtype=np.int64)
    for i, (w, s) in enumerate(zip(want, stored)):
        d = np.flatnonzero(w != s)
        cnt[i] = d.size
        if d.size:
            first[i] = d[0]
    return cnt, first


def encode_plan(need, total):
    """The encode plan over a full-slot layout: inputs 0..need-1, outputs need..total-1;
    its rows are the oracle's parity rows."""
    from slime_amd import device as D
    plan = D.Plan.encode(need, total).set_outputs(list(range(need, total)))
    assert np.array_equal(plan.coefficients(), OC.parity_matrix(need, total - need)[need:])
    return plan


def flip_positions(L, T):
    """Column 0, the last column of the first tile, the first of the second,
    the first tail column (past the last whole vector) and the last column."""
    return sorted({c for c in (0, T - 1, T, L - L % 4, L - 1) if 0 <= c < L})


# ------------------------------------------------------------------ clean data

@pytest.mark.parametrize("need,total", CODES)
def test_clean_full_slot_every_length(torch_dev, pipeline, need, total):
    torch = torch_dev
    from slime_amd import device as D
    plan = encode_plan(need, total)
    for L in lengths(need, total - need):
        for nobj in (1, 3):
            buf = to_dev(torch, encoded(need, total, L, nobj, seed=need * 100003 + L))
            lay = D.layout_of(total, L)
            assert_clean(torch, raw_verify(torch, plan, buf, lay, buf, lay, L, nobj), (L, nobj))
            m, f = plan.verify(buf, lay, buf, lay, L, nobj)  # the wrapper's own result tensors
            assert m.shape == f.shape == (nobj, total - need) and m.dtype == f.dtype == torch.int64
            assert_clean(torch, (m, f), (L, nobj, "wrapper"))


@pytest.mark.parametrize("need,total", [(4, 6), (8, 12), (10, 14), (17, 20)])
def test_clean_several_segments_per_object(torch_dev, pipeline, need, total):
    """L = 20483: five column segments an object (object_segments), tail columns after them."""
    torch = torch_dev
    from slime_amd import device as D
    L, nobj = 5 * 4096 + 3, 3
    plan = encode_plan(need, total)
    a = encoded(need, total, L, nobj, seed=total)
    buf = to_dev(torch, a)
    lay = D.layout_of(total, L)
    assert_clean(torch, raw_verify(torch, plan, buf, lay, buf, lay, L, nobj))
    # one flipped word in each segment of the middle object's last row: the segments add up
    cols = [7, 4096 + 1, 2 * 4096 + 2, 3 * 4096 + 3, 5 * 4096 - 1, L - 1]
    v = buf.view(nobj, total, L)
    for c in cols:
        v[1, total - 1, c] ^= 1
    m, f = host(torch, raw_verify(torch, plan, buf, lay, buf, lay, L, nobj))
    em = np.zeros((nobj, total - need), dtype=np.int64)
    ef = np.full((nobj, total - need), -1, dtype=np.int64)
    em[1, -1], ef[1, -1] = len(cols), cols[0]
    assert np.array_equal(m, em) and np.array_equal(f, ef)


@pytest.mark.parametrize("need,total,L", [(8, 12, 1031), (4, 6, 2 * 1024 + 3), (16, 20, 777), (17, 20, 515)])
def test_clean_separate_tensors_odd_strides_and_offsets(torch_dev, pipeline, need, total, L):
    """src and cmp in separate tensors with different layouts: shard strides
    that are no multiple of 4 words, an odd src_offset, cmp rows in reverse order."""
    torch = torch_dev
    from slime_amd import device as D
    nobj, r = 3, total - need
    a = encoded(need, total, L, nobj, seed=L)
    rng = np.random.default_rng(L + 1)
    s_ss, s_obj, s_off = L + 1, (L + 1) * need + 3, 1
    src_h = rng.integers(0, 2**32, size=s_off + nobj * s_obj, dtype=np.uint64).astype(np.uint32)
    c_ss, c_obj, c_off = L + 3, (L + 3) * r + 2, 6
    cmp_h = rng.integers(0, 2**32, size=c_off + nobj * c_obj, dtype=np.uint64).astype(np.uint32)
    outs = list(range(r))[::-1]  # row i is stored at cmp shard r-1-i
    for o in range(nobj):
        for j in range(need):
            at = s_off + o * s_obj + j * s_ss
            src_h[at: at + L] = a[o, j, :L]
        for i in range(r):
            at = c_off + o * c_obj + outs[i] * c_ss
            cmp_h[at: at + L] = a[o, need + i, :L]
    plan = D.Plan.encode(need, total).set_outputs(outs)
    src, cmp = to_dev(torch, src_h), to_dev(torch, cmp_h)
    args = (plan, src, N.Layout(s_obj, s_ss), cmp, N.Layout(c_obj, c_ss), L, nobj)
    assert_clean(torch, raw_verify(torch, *args, src_offset=s_off, cmp_offset=c_off))
    assert_clean(torch, plan.verify(*args[1:], src_offset=s_off, cmp_offset=c_off))
    # a flipped word in the last stored row's last column, last object
    cmp[c_off + (nobj - 1) * c_obj + outs[r - 1] * c_ss + L - 1] ^= 4
    m, f = host(torch, raw_verify(torch, *args, src_offset=s_off, cmp_offset=c_off))
    em = np.zeros((nobj, r), dtype=np.int64)
    ef = np.full((nobj, r), -1, dtype=np.int64)
    em[-1, -1], ef[-1, -1] = 1, L - 1
    assert np.array_equal(m, em) and np.array_equal(f, ef)


@pytest.mark.parametrize("k,rows,L", [(5, 3, 1031), (8, 4, 2 * 512 + 6), (3, 2, 4 * 1024 + 1), (20, 5, 300)])
def test_matrix_plan_noncanonical_inputs_against_its_own_output(torch_dev, pipeline, k, rows, L):
    """Plan.matrix with arbitrary coefficients and permuted in_shards over any
    uint32 inputs (EDGES): verify against the output of plan(...) itself gives
    zero, and that output is the oracle's."""
    torch = torch_dev
    from slime_amd import device as D
    rng = np.random.default_rng(k * 31 + L)
    nobj, nsh = 3, k + 2
    src_h = rng.integers(0, 2**32, size=(nobj, nsh, L), dtype=np.uint64).astype(np.uint32)
    for o in range(nobj):
        for j in range(nsh):
            n = min(L, EDGES.size)
            src_h[o, j, rng.choice(L, size=n, replace=False)] = EDGES[:n]
    coeff = rng.integers(0, P, size=(rows, k), dtype=np.uint64).astype(np.uint32)
    coeff[0] = P - 1
    coeff[-1, 0] = 0
    in_shards = [int(x) for x in rng.permutation(nsh)[:k]]
    plan = D.Plan.matrix(coeff, in_shards)
    src = to_dev(torch, src_h)
    out = torch.zeros(nobj * rows * L, dtype=torch.int32, device="cuda")
    slay, olay = D.layout_of(nsh, L), D.layout_of(rows, L)
    plan(src, slay, out, olay, L, nobj)
    torch.cuda.synchronize()
    out_h = out.cpu().numpy().view(np.uint32).reshape(nobj, rows, L)
    for o in range(nobj):
        want = OC.apply_matrix(coeff, [src_h[o, j] for j in in_shards])
        assert all(np.array_equal(out_h[o, i], want[i]) for i in range(rows))
    assert_clean(torch, raw_verify(torch, plan, src, slay, out, olay, L, nobj))
    # corrupt one input word of object 1: the oracle's recomputation gives every row's count
    col = L // 2
    src.view(nobj, nsh, L)[1, in_shards[0], col] ^= 0x10
    src_h[1, in_shards[0], col] ^= 0x10
    m, f = host(torch, raw_verify(torch, plan, src, slay, out, olay, L, nobj))
    for o in range(nobj):
        cnt, first = expected(coeff, [src_h[o, j] for j in in_shards], out_h[o])
        assert np.array_equal(m[o], cnt) and np.array_equal(f[o], first), o
    assert m[1, 0] == 1 and m[1, -1] == 0  # coeff[-1][0] is zero: that row does not see the word


@pytest.mark.parametrize("need,total,have,want", [(4, 6, [5, 2, 4, 1], [0, 3]), (4, 6, [3, 0, 5, 4], [1, 2]),
                                                  (8, 12, [11, 1, 9, 3, 10, 5, 8, 7], [0, 2, 4, 6])])
def test_reconstruct_plans_data_targets_shuffled_survivors(torch_dev, pipeline, need, total, have, want):
    torch = torch_dev
    from slime_amd import device as D
    L, nobj = 3 * 1024 + 5, 3
    a = encoded(need, total, L, nobj, seed=sum(have))
    buf = to_dev(torch, a)
    lay = D.layout_of(total, L)
    plan = D.Plan.reconstruct(need, total, have, want).set_outputs(want)
    assert_clean(torch, raw_verify(torch, plan, buf, lay, buf, lay, L, nobj))
    # a corrupt survivor: counts from the oracle over the plan's rows
    a[2, have[1], 1000] ^= 0x8000
    buf.view(nobj, total, L)[2, have[1], 1000] ^= 0x8000
    m, f = host(torch, raw_verify(torch, plan, buf, lay, buf, lay, L, nobj))
    for o in range(nobj):
        cnt, first = expected(plan.coefficients(), [a[o, j] for j in have], [a[o, t] for t in want])
        assert np.array_equal(m[o], cnt) and np.array_equal(f[o], first), o
    assert m[2].sum() >= 1 and not m[:2].any()


# ------------------------------------------------------------- one wrong word

@pytest.mark.parametrize("need,total", CODES)
def test_one_flipped_stored_word(torch_dev, pipeline, need, total):
    """One flipped word in a stored row, at each position class, in the first
    and last object and in each row: exactly that entry has count 1 and that
    first column."""
    torch = torch_dev
    from slime_amd import device as D
    r, nobj = total - need, 3
    T = tile_cols(need, r)
    plan = encode_plan(need, total)
    for L in (3 * T + 7, T + 1, 5):
        buf = to_dev(torch, encoded(need, total, L, nobj, seed=need + L))
        lay = D.layout_of(total, L)
        v = buf.view(nobj, total, L)
        for col in flip_positions(L, T):
            for o in (0, nobj - 1):
                for i in range(r):
                    v[o, need + i, col] ^= 1 << (col % 31)
                    m, f = host(torch, raw_verify(torch, plan, buf, lay, buf, lay, L, nobj))
                    v[o, need + i, col] ^= 1 << (col % 31)
                    em = np.zeros((nobj, r), dtype=np.int64)
                    ef = np.full((nobj, r), -1, dtype=np.int64)
                    em[o, i], ef[o, i] = 1, col
                    assert np.array_equal(m, em) and np.array_equal(f, ef), (L, col, o, i)
        assert_clean(torch, raw_verify(torch, plan, buf, lay, buf, lay, L, nobj), L)  # all flips undone


@pytest.mark.parametrize("need,total", CODES)
def test_one_corrupted_input_word(torch_dev, pipeline, need, total):
    """One corrupted input word: the expected per-row counts come from the
    oracle's recomputation; every parity row has a non-zero coefficient for
    every input, so each shows 1 at that column."""
    torch = torch_dev
    from slime_amd import device as D
    r, nobj = total - need, 3
    T = tile_cols(need, r)
    L = 3 * T + 7
    plan = encode_plan(need, total)
    assert plan.coefficients().all()
    a = encoded(need, total, L, nobj, seed=need * 7 + 1)
    buf = to_dev(torch, a)
    lay = D.layout_of(total, L)
    v = buf.view(nobj, total, L)
    for col in flip_positions(L, T):
        for o, j in ((0, 0), (nobj - 1, need - 1)):
            v[o, j, col] ^= 2
            a[o, j, col] ^= 2
            m, f = host(torch, raw_verify(torch, plan, buf, lay, buf, lay, L, nobj))
            for q in range(nobj):
                cnt, first = expected(plan.coefficients(), list(a[q, :need]), list(a[q, need:]))
                assert np.array_equal(m[q], cnt) and np.array_equal(f[q], first), (col, o, q)
            assert (m[o] == 1).all() and (f[o] == col).all() and m.sum() == r
            v[o, j, col] ^= 2
            a[o, j, col] ^= 2


def test_noncanonical_stored_word_is_a_mismatch(torch_dev, pipeline):
    """A stored p+3 where the plan computes 3 counts (execute would change it);
    a non-canonical INPUT p+3 is fine, as everywhere in the library."""
    torch = torch_dev
    from slime_amd import device as D
    L, nobj = 1029, 2
    coeff = np.array([[1, 0], [1, 1]], dtype=np.uint32)
    plan = D.Plan.matrix(coeff, [0, 1])
    src_h = np.zeros((nobj, 2, L), dtype=np.uint32)
    src_h[:, 0, :] = 3
    src_h[1, 0, 5] = P + 3  # the same residue, non-canonical
    out_h = np.full((nobj, 2, L), 3, dtype=np.uint32)
    for o in range(nobj):
        want = OC.apply_matrix(coeff, list(src_h[o]))
        assert all(np.array_equal(want[i], out_h[o, i]) for i in range(2))
    spots = [(0, 0, 0), (0, 1, 1027), (1, 0, 1028), (1, 1, 600)]  # vector columns and a tail column
    for o, i, c in spots:
        out_h[o, i, c] = P + 3
    src, out = to_dev(torch, src_h), to_dev(torch, out_h)
    lay = D.layout_of(2, L)
    m, f = host(torch, raw_verify(torch, plan, src, lay, out, lay, L, nobj))
    assert np.array_equal(m, np.ones((nobj, 2), dtype=np.int64))
    assert np.array_equal(f, np.array([[0, 1027], [1028, 600]], dtype=np.int64))


# ------------------------------------------- accumulation and flush: many mismatches

@pytest.mark.parametrize("need,total,L,nobj", [(8, 12, 5 * 4096 + 3, 5), (4, 6, 6 * 4096 + 1, 4), (3, 5, 4 * 4096 + 2, 3),
                                               (16, 20, 3 * 4096 + 3, 3), (17, 20, 4099, 3), (33, 50, 1500, 2)])
def test_random_and_total_corruption_match_numpy(torch_dev, pipeline, need, total, L, nobj):
    """About 1% of the stored columns flipped at random over every object and
    row -- many waves and segments contribute to each entry -- and, separately,
    every column of one row: counts and firsts equal numpy's exactly."""
    torch = torch_dev
    from slime_amd import device as D
    r = total - need
    plan = encode_plan(need, total)
    a = encoded(need, total, L, nobj, seed=L + need)
    lay = D.layout_of(total, L)
    rng = np.random.default_rng(L)

    def check(b):
        m, f = host(torch, raw_verify(torch, plan, to_dev(torch, b), lay, to_dev(torch, b), lay, L, nobj))
        for o in range(nobj):
            cnt, first = expected(plan.coefficients(), list(b[o, :need]), list(b[o, need:]))
            assert np.array_equal(m[o], cnt) and np.array_equal(f[o], first), o
        return m

    b = a.copy()
    hit = rng.random((nobj, r, L)) < 0.01
    b[:, need:, :][hit] ^= rng.integers(1, 2**32, size=int(hit.sum()), dtype=np.uint64).astype(np.uint32)
    m = check(b)
    assert np.array_equal(m, hit.sum(axis=2)) and m.min() > 0
    b = a.copy()
    b[nobj - 1, need + r // 2, :] ^= 0x01000000  # a whole row of the last object
    m = check(b)
    assert m[nobj - 1, r // 2] == L and m.sum() == L
    b = a.copy()
    b[:, need:, :] = ~b[:, need:, :]  # everything wrong everywhere
    assert (check(b) == L).all()


@pytest.mark.parametrize("need,total,L", [(4, 6, 2 * 65536 + 3), (8, 12, 65536 + 3)])
def test_many_tiles_per_wave(torch_dev, pipeline, need, total, L):
    """64 objects of four segments each on a one-block-wide grid: every wave
    walks eight tiles of its segment, so the pipelined form's two register sets
    alternate several times.  Clean, then 0.1% of the stored words flipped."""
    torch = torch_dev
    from slime_amd import device as D
    nobj, r = 64, total - need
    rng = np.random.default_rng(L)
    wide = rng.integers(0, P, size=(total, nobj * L), dtype=np.uint32)
    OC.encode_object(wide, need, total)
    a = np.ascontiguousarray(wide.reshape(total, nobj, L).transpose(1, 0, 2))
    del wide
    plan = encode_plan(need, total)
    lay = D.layout_of(total, L)
    buf = to_dev(torch, a)
    assert_clean(torch, raw_verify(torch, plan, buf, lay, buf, lay, L, nobj))
    hit = rng.random((nobj, r, L)) < 0.001
    hit[nobj - 1, r - 1, L - 1] = hit[0, 0, 0] = True
    flips = torch.from_numpy(hit).cuda()
    buf.view(nobj, total, L)[:, need:, :] ^= flips.to(torch.int32) << 9
    m, f = host(torch, raw_verify(torch, plan, buf, lay, buf, lay, L, nobj))
    assert np.array_equal(m, hit.sum(axis=2))
    assert np.array_equal(f, np.where(hit.any(axis=2), hit.argmax(axis=2), -1))
    assert f[0, 0] == 0 and m.min() > 0


def test_65537_objects_pass_the_grid_cap(torch_dev, pipeline):
    """More objects than gridDim.y holds (65535): the launch strides over them."""
    torch = torch_dev
    from slime_amd import device as D
    need, total, L, nobj = 4, 6, 5, 65537
    plan = encode_plan(need, total)
    a = encoded(need, total, L, nobj, seed=65537)
    lay = D.layout_of(total, L)
    buf = to_dev(torch, a)
    assert_clean(torch, raw_verify(torch, plan, buf, lay, buf, lay, L, nobj))
    em = np.zeros((nobj, 2), dtype=np.int64)
    ef = np.full((nobj, 2), -1, dtype=np.int64)
    v = buf.view(nobj, total, L)
    for o, i, c in ((0, 0, 4), (65534, 1, 0), (65535, 0, 3), (65536, 1, 4), (65536, 1, 2), (40000, 0, 1)):
        v[o, need + i, c] ^= 0x100
        em[o, i] += 1
        ef[o, i] = c if ef[o, i] < 0 else min(ef[o, i], c)
    m, f = host(torch, raw_verify(torch, plan, buf, lay, buf, lay, L, nobj))
    assert np.array_equal(m, em) and np.array_equal(f, ef)


def matrix_case(torch, k, rows, L, nobj, seed):
    """A Plan.matrix over random uint32 inputs and its oracle output rows."""
    from slime_amd import device as D
    rng = np.random.default_rng(seed)
    src_h = rng.integers(0, 2**32, size=(nobj, k, L), dtype=np.uint64).astype(np.uint32)
    coeff = rng.integers(1, P, size=(rows, k), dtype=np.uint64).astype(np.uint32)
    out_h = np.stack([np.stack(OC.apply_matrix(coeff, list(src_h[o]))) for o in range(nobj)])
    return D.Plan.matrix(coeff, list(range(k))), coeff, src_h, out_h


@pytest.mark.parametrize("k,rows,L", [(3, 70, 1031), (8, 129, 515), (20, 67, 300)])
def test_plans_of_more_than_64_rows(torch_dev, pipeline, k, rows, L):
    """A launch tallies 64 rows, a lane each: larger plans run in row blocks of
    64 whose coefficient rows, output shards and result entries are offset."""
    torch = torch_dev
    from slime_amd import device as D
    nobj = 2
    plan, coeff, src_h, out_h = matrix_case(torch, k, rows, L, nobj, seed=rows * 7 + k)
    slay, olay = D.layout_of(k, L), D.layout_of(rows, L)
    src = to_dev(torch, src_h)
    assert_clean(torch, raw_verify(torch, plan, src, slay, to_dev(torch, out_h), olay, L, nobj))
    for o, i, c in ((0, 0, 1), (0, 63, L - 1), (1, 64, 0), (1, 64, 700 % L), (0, 65, L - 2), (1, rows - 1, L // 2)):
        out_h[o, i, c] ^= 0x20
    out_h[1, rows - 2, :] ^= 1  # a whole row of the last block
    m, f = host(torch, raw_verify(torch, plan, src, slay, to_dev(torch, out_h), olay, L, nobj))
    for o in range(nobj):
        cnt, first = expected(coeff, list(src_h[o]), list(out_h[o]))
        assert np.array_equal(m[o], cnt) and np.array_equal(f[o], first), o
    assert m[1, 64] == 2 and m[1, rows - 2] == L and m[0, 63] == 1 and m.sum() == L + 6


@pytest.mark.parametrize("k,rows,L", [(4, 2, 1031), (8, 4, 777), (20, 3, 130)])
@pytest.mark.parametrize("src_off,cmp_off", [(2, 0), (0, 2), (2, 2), (1, 3)])
def test_bases_not_word_aligned_take_the_column_form(torch_dev, pipeline, k, rows, L, src_off, cmp_off):
    """src or cmp off a 4-byte boundary (a byte offset into a byte buffer):
    every column runs one per lane, with the same answers."""
    torch = torch_dev
    from slime_amd import device as D
    nobj = 3
    plan, coeff, src_h, out_h = matrix_case(torch, k, rows, L, nobj, seed=L + src_off * 4 + cmp_off)
    out_h[2, rows - 1, L - 1] ^= 0x400
    out_h[0, 0, 5] ^= 0x400
    out_h[0, 0, 300 % L] ^= 0x400

    def shifted(a, off):
        b = np.full(a.size * 4 + 8, 0xA5, dtype=np.uint8)
        b[off: off + a.size * 4] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        return torch.from_numpy(b).cuda()

    src, cmp = shifted(src_h, src_off), shifted(out_h, cmp_off)
    mism = torch.full((nobj, rows), GARBAGE, dtype=torch.int64, device="cuda")
    first = torch.full((nobj, rows), GARBAGE, dtype=torch.int64, device="cuda")
    N.check(N.lib.slime_rs_plan_verify(plan._h, ctypes.c_void_p(src.data_ptr() + src_off), D.layout_of(k, L),
                                       ctypes.c_void_p(cmp.data_ptr() + cmp_off), D.layout_of(rows, L), L, nobj,
                                       ctypes.c_void_p(mism.data_ptr()), ctypes.c_void_p(first.data_ptr()), None))
    m, f = host(torch, (mism, first))
    for o in range(nobj):
        cnt, fst = expected(coeff, list(src_h[o]), list(out_h[o]))
        assert np.array_equal(m[o], cnt) and np.array_equal(f[o], fst), o
    assert m[0, 0] == 2 and f[0, 0] == 5 and m[2, rows - 1] == 1 and m.sum() == 3


# ------------------------------------------------ result arrays, streams, graphs

def test_results_are_initialised_for_empty_shards_and_untouched_for_no_objects(torch_dev):
    torch = torch_dev
    from slime_amd import device as D
    plan = encode_plan(4, 6)
    buf = torch.zeros(64, dtype=torch.int32, device="cuda")
    lay = D.layout_of(6, 0)
    assert_clean(torch, raw_verify(torch, plan, buf, lay, buf, lay, 0, 3))  # L == 0, nobj > 0
    m, f = plan.verify(buf, lay, buf, lay, 0, 3)
    assert_clean(torch, (m, f))
    m, f = plan.verify(buf, lay, buf, lay, 0, 0)
    assert m.shape == f.shape == (0, 2)
    # nobj == 0 returns 0 and touches nothing
    g = torch.full((4,), GARBAGE, dtype=torch.int64, device="cuda")
    h = g.clone()
    assert N.lib.slime_rs_plan_verify(plan._h, ctypes.c_void_p(buf.data_ptr()), lay, ctypes.c_void_p(buf.data_ptr()),
                                      lay, 8, 0, ctypes.c_void_p(g.data_ptr()), ctypes.c_void_p(h.data_ptr()),
                                      None) == 0
    torch.cuda.synchronize()
    assert (g == GARBAGE).all() and (h == GARBAGE).all()
    # null results or buffers with work to do, and too many objects, are refused
    p = ctypes.c_void_p(buf.data_ptr())
    r = ctypes.c_void_p(g.data_ptr())
    lay8 = D.layout_of(6, 8)
    for args in ((p, lay8, p, lay8, 8, 1, None, r), (p, lay8, p, lay8, 8, 1, r, None), (None, lay8, p, lay8, 8, 1, r, r),
                 (p, lay8, None, lay8, 8, 1, r, r), (p, lay8, p, lay8, 8, 1 << 32, r, r)):
        assert N.lib.slime_rs_plan_verify(plan._h, *args, None) == N.ERR_INVALID_ARG
        assert "plan_verify" in N.lib.slime_rs_last_error().decode()


def test_verify_marks_the_plan_as_launched(torch_dev):
    torch = torch_dev
    from slime_amd import device as D
    plan = D.Plan.encode(4, 6).set_outputs([4, 5])
    buf = to_dev(torch, encoded(4, 6, 16, 1, seed=3))
    lay = D.layout_of(6, 16)
    assert_clean(torch, plan.verify(buf, lay, buf, lay, 16, 1))
    with pytest.raises(N.NativeError, match="already launched"):
        plan.set_outputs([0, 1])


def test_non_default_stream_and_graph_replays(torch_dev, pipeline):
    """On a side stream, then captured into one graph and replayed twice with a
    corruption added in between: each replay re-initialises the results, the
    second shows the corruption and carries nothing over from the first."""
    torch = torch_dev
    from slime_amd import device as D
    need, total, L, nobj = 8, 12, 3 * 512 + 5, 3
    r = total - need
    plan = encode_plan(need, total)
    buf = to_dev(torch, encoded(need, total, L, nobj, seed=99))
    lay = D.layout_of(total, L)
    v = buf.view(nobj, total, L)
    v[1, need + 2, 77] ^= 1
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        res = raw_verify(torch, plan, buf, lay, buf, lay, L, nobj, stream=side)
        res2 = plan.verify(buf, lay, buf, lay, L, nobj)  # the current stream is `side`
    side.synchronize()
    em = np.zeros((nobj, r), dtype=np.int64)
    ef = np.full((nobj, r), -1, dtype=np.int64)
    em[1, 2], ef[1, 2] = 1, 77
    for got in (res, res2):
        m, f = host(torch, got)
        assert np.array_equal(m, em) and np.array_equal(f, ef)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gm, gf_ = plan.verify(buf, lay, buf, lay, L, nobj)
    gm.fill_(GARBAGE)
    gf_.fill_(GARBAGE)
    g.replay()
    m, f = host(torch, (gm, gf_))
    assert np.array_equal(m, em) and np.array_equal(f, ef)
    v[1, need + 2, 77] ^= 1  # repaired ...
    v[0, need, 5] ^= 8       # ... and two new ones elsewhere
    v[0, need, 1500] ^= 8
    g.replay()
    m, f = host(torch, (gm, gf_))
    em[:], ef[:] = 0, -1
    em[0, 0], ef[0, 0] = 2, 5
    assert np.array_equal(m, em) and np.array_equal(f, ef)


# ------------------------------------------------------------------ object slots

def oracle_chunks(obj, need, total, cands=()):
    """The reference's writeChunks framing (multi_store.go:526-554) via the oracle."""
    rc, m, words = OC.map_to_gf(obj, list(cands))
    assert rc == 0
    parts = OP.split_vector(words, need)
    parity = [OC.create_parity(parts, need + i)[1] for i in range(total - need)]
    return m, [OC.map_from_gf(m, p) for p in parts + parity]


def expected_bytes(h, stride, cs, L, nobj, ms, coeff, ins, outs):
    """Counts and firsts of every slot of the host copy h: big-endian words XOR
    the mapping through the oracle's rows, against the stored chunks."""
    em = np.zeros((nobj, len(outs)), dtype=np.int64)
    ef = np.full((nobj, len(outs)), -1, dtype=np.int64)

    def words(o, c):
        return h[o * stride + c * cs: o * stride + c * cs + 4 * L].view(">u4").astype(np.uint32)

    for o in range(nobj):
        want = OC.apply_matrix(coeff, [words(o, c) ^ np.uint32(ms[o]) for c in ins])
        for i, c in enumerate(outs):
            d = np.flatnonzero((want[i] ^ np.uint32(ms[o])) != words(o, c))
            em[o, i] = d.size
            if d.size:
                ef[o, i] = d[0]
    return em, ef


def raw_verify_objects(torch, plan, slots, stride, cs, L, nobj, mapping):
    mism = torch.full((nobj, plan.rows), GARBAGE, dtype=torch.int64, device="cuda")
    first = torch.full((nobj, plan.rows), GARBAGE, dtype=torch.int64, device="cuda")
    N.check(N.lib.slime_rs_verify_objects(plan._h, ctypes.c_void_p(slots.data_ptr()), stride, cs, L, nobj,
                                          ctypes.c_void_p(mapping.data_ptr()), ctypes.c_void_p(mism.data_ptr()),
                                          ctypes.c_void_p(first.data_ptr()), None))
    return mism, first


@pytest.mark.parametrize("align", [1, 256], ids=["wire", "chunks256"])
@pytest.mark.parametrize("need,total", [(4, 6), (10, 14)])
@pytest.mark.parametrize("size", [(0, 1), (4, -1), (4, 0), (4, 1), (0, 1031), (0, 3 * (1 << 20) + 7)],
                         ids=["1", "4need-1", "4need", "4need+1", "1031", "3MiB+7"])
def test_verify_objects(torch_dev, need, total, size, align):
    """Slots encoded by encode_objects (+ resolve_fallbacks) and checked against
    the oracle's framing: mappings 0, 1<<31 and a fallback value; clean slots
    give zero, one flipped parity byte gives count 1 at byte/4, one flipped data
    byte the oracle's per-row counts; with a 256-byte chunk stride the random
    padding between chunks never counts."""
    torch = torch_dev
    from slime_amd import device as D
    S = size[0] * need + size[1]
    r, nobj = total - need, 3
    rng = np.random.default_rng(S * 131 + need + align)
    objs = [bytearray(rng.integers(0, 256, size=S, dtype=np.uint8).tobytes()) for _ in range(nobj)]
    if S >= 4:
        objs[1][0:4] = b"\xff\xff\xff\xfd"  # a word >= p: mapping 1<<31
    if S >= 8:
        objs[2][0:8] = b"\xff\xff\xff\xff\x7f\xff\xff\xff"  # neither 0 nor 1<<31 fits: a fallback mapping
    objs = [bytes(b) for b in objs]
    L, cs, slot = D.slot_geometry(S, need, total, chunk_align=align)
    stride = slot + 12
    host_slots = rng.integers(0, 256, size=nobj * stride, dtype=np.uint8)  # padding and slack: random bytes
    for o, b in enumerate(objs):
        a = np.frombuffer(b, dtype=np.uint8)
        for j in range(need):
            part = a[j * 4 * L: (j + 1) * 4 * L]
            host_slots[o * stride + j * cs: o * stride + j * cs + part.size] = part
    slots = torch.from_numpy(host_slots).cuda()
    enc = D.Plan.encode(need, total)
    mapping = torch.empty(nobj, dtype=torch.int32, device="cuda")
    status = torch.empty(nobj, dtype=torch.int32, device="cuda")
    D.encode_objects(enc, slots, stride, S, nobj, mapping, status, chunk_stride=cs)
    torch.cuda.synchronize()
    st = status.cpu().numpy().tolist()
    if any(st):
        assert D.resolve_fallbacks(enc, slots, stride, S, nobj, mapping, status, chunk_stride=cs) == sum(st)
    torch.cuda.synchronize()
    ms = mapping.cpu().numpy().view(np.uint32)
    h = slots.cpu().numpy()
    for o, obj in enumerate(objs):  # the slots are the oracle's framing before anything is asserted about verify
        m, chunks = oracle_chunks(obj, need, total, [int(ms[o])] if st[o] else [])
        assert ms[o] == m
        for c in range(total):
            assert h[o * stride + c * cs: o * stride + c * cs + 4 * L].tobytes() == chunks[c], (o, c)
    assert ms[0] == 0
    if S >= 4:
        assert ms[1] == 1 << 31
    if S >= 8:
        assert st[2] == 1 and ms[2] not in (0, 1 << 31)
    plan = D.Plan.encode(need, total).set_outputs(list(range(need, total)))
    ins, outs = list(range(need)), list(range(need, total))
    coeff = OC.parity_matrix(need, r)[need:]
    assert_clean(torch, raw_verify_objects(torch, plan, slots, stride, cs, L, nobj, mapping))
    assert_clean(torch, D.verify_objects(plan, slots, stride, L, nobj, mapping, chunk_stride=cs))
    if align == 1:
        assert_clean(torch, D.verify_objects(plan, slots, stride, L, nobj, mapping))  # chunk_stride 0 selects 4L
    # one flipped byte in a parity chunk: count 1 at column byte/4
    for o, i, byte in ((0, 0, 0), (nobj - 1, r - 1, 4 * L - 1), (1, r // 2, (4 * L) // 2)):
        at = o * stride + (need + i) * cs + byte
        slots[at] ^= 0x40
        m, f = host(torch, raw_verify_objects(torch, plan, slots, stride, cs, L, nobj, mapping))
        slots[at] ^= 0x40
        em = np.zeros((nobj, r), dtype=np.int64)
        ef = np.full((nobj, r), -1, dtype=np.int64)
        em[o, i], ef[o, i] = 1, byte // 4
        assert np.array_equal(m, em) and np.array_equal(f, ef), (o, i, byte)
    # one flipped byte in a data chunk: the oracle's per-row counts
    for o, j, byte in ((0, 0, 4 * L - 1), (nobj - 1, need - 1, 0)):
        at = o * stride + j * cs + byte
        slots[at] ^= 0x01
        h[at] ^= 0x01
        m, f = host(torch, D.verify_objects(plan, slots, stride, L, nobj, mapping, chunk_stride=cs))
        em, ef = expected_bytes(h, stride, cs, L, nobj, ms, coeff, ins, outs)
        assert np.array_equal(m, em) and np.array_equal(f, ef), (o, j, byte)
        assert (em[o] == 1).all() and (ef[o] == byte // 4).all() and em.sum() == r
        slots[at] ^= 0x01
        h[at] ^= 0x01
    # a reconstruct plan that targets an erased data chunk (and a parity chunk) also verifies clean
    erase = [0, total - 1][:r]
    have = [c for c in range(total) if c not in erase][:need]
    rec = D.Plan.reconstruct(need, total, have, erase).set_outputs(erase)
    assert_clean(torch, raw_verify_objects(torch, rec, slots, stride, cs, L, nobj, mapping))
    slots[(nobj - 1) * stride + 3] ^= 0x80  # data chunk 0, column 0 of the last object
    m, f = host(torch, raw_verify_objects(torch, rec, slots, stride, cs, L, nobj, mapping))
    assert m[nobj - 1, 0] == 1 and f[nobj - 1, 0] == 0 and m.sum() == 1


@pytest.mark.parametrize("need,total,L", [(4, 6, 1029), (10, 14, 515), (20, 24, 130)])
def test_verify_objects_hand_chosen_mapping(torch_dev, need, total, L):
    """An object built on the CPU with a third mapping value, checked with a
    decode plan: symbols below p from the oracle, chunks = BE(symbol ^ m)."""
    torch = torch_dev
    from slime_amd import device as D
    m3 = 0x12345678
    nobj, cs = 2, 4 * L + 252 - (4 * L) % 4
    stride = total * cs + 8
    sym = encoded(need, total, L, nobj, seed=L)
    rng = np.random.default_rng(L)
    h = rng.integers(0, 256, size=nobj * stride, dtype=np.uint8)
    ms = np.array([m3, 0x00C0FFEE], dtype=np.uint32)
    for o in range(nobj):
        for c in range(total):
            h[o * stride + c * cs: o * stride + c * cs + 4 * L] = np.frombuffer(
                OC.map_from_gf(int(ms[o]), sym[o, c]), dtype=np.uint8)
    slots = torch.from_numpy(h).cuda()
    mapping = to_dev(torch, ms)
    erase = [1, need]
    have = [c for c in range(total) if c not in erase][:need][::-1]
    rec = D.Plan.reconstruct(need, total, have, erase).set_outputs(erase)
    assert_clean(torch, raw_verify_objects(torch, rec, slots, stride, cs, L, nobj, mapping))
    # with the wrong mapping nearly every column differs: expectation from the oracle's rows
    wrong = np.array([m3 ^ 0x100, 0x00C0FFEE], dtype=np.uint32)
    m, f = host(torch, raw_verify_objects(torch, rec, slots, stride, cs, L, nobj, to_dev(torch, wrong)))
    em, ef = expected_bytes(h, stride, cs, L, nobj, wrong, rec.coefficients(), have, erase)
    assert np.array_equal(m, em) and np.array_equal(f, ef)
    assert em[0].min() > L // 2 and not em[1].any()
