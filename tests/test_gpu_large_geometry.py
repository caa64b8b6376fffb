"""Shards of 2-4 GiB and layouts at the 32-bit offset limits ("Size rules").

Every fast kernel family keeps 32-bit byte offsets somewhere and is guarded by a size rule
in its launcher; the rest of the suite reaches the far side of those rules only through the
process-wide switches at a few thousand columns.  Here the lengths themselves cross them:

  LA = 2^29 + 259   in-shard byte offsets cross 2^31; L % 4 == 3
  LB = 2^30 - 1     the last length the 32-bit forms take (tail columns at bytes 2^32-12 .. 2^32-4)
  LC = 2^30         the first length of the 64-bit forms
  LD = 2^30 + 5     tail columns past byte 2^32

The reference is tests/bigref.py (torch int64 arithmetic on the device, pinned to the C oracle
by tests/test_bigref.py); every test also checks three 4096-column windows of the kernel's
output against the oracle itself.  Whole destination buffers are compared, sentinel gaps
included, and the first differing index is reported.  No test keeps more than 24 GiB of
device tensors alive; each frees what it made.
"""
import ctypes

import numpy as np
import pytest

import bigref as BR
from oracle import oracle_c as OC
from slime_amd import _native as N

pytestmark = pytest.mark.gpu

P = 4294967291
EDGES = np.array([0, 1, 2, P - 1, P, P + 1, P + 4, 0xFFFFFFFF, 0x7FFFFFFF, 0x80000000], dtype=np.uint32)
LA, LB, LC, LD = (1 << 29) + 259, (1 << 30) - 1, 1 << 30, (1 << 30) + 5
SMALL = 5507
MID = 1 << 29
SENT = 0x5EA7BEEF  # what destinations and gaps hold before a launch


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


@pytest.fixture
def switches():
    """The process-wide kernel switches, restored after the test."""
    names = ("slime_rs_kernel_schedule", "slime_rs_kernel_pipeline", "slime_rs_kernel_matrix_cores",
             "slime_rs_switch_bits")
    before = {n: getattr(N.lib, n)(-1) for n in names}

    def set_(schedule=None, pipeline=None, matrix_cores=None, switch_bits=None):
        for n, v in zip(names, (schedule, pipeline, matrix_cores, switch_bits)):
            if v is not None:
                getattr(N.lib, n)(v)

    yield set_
    for n, v in before.items():
        getattr(N.lib, n)(v)


def up64(n: int) -> int:
    return -(-n // 64) * 64


def edges_t(torch, n: int, roll: int = 0):
    return torch.from_numpy(np.roll(np.resize(EDGES, n), roll).view(np.int32)).cuda()


def plant(torch, t, roll: int = 0, width: int = 64):
    """EDGES (non-canonical inputs) over the first and last `width` words of the 1-D view t and
    the `width` words around column 2^29."""
    n = t.numel()
    t[:width] = edges_t(torch, width, roll)
    t[n - width:] = edges_t(torch, width, roll + 3)
    if n >= MID + width:
        t[MID - width // 2: MID + width // 2] = edges_t(torch, width, roll + 5)


def windows(L: int):
    """Three 4096-column windows: the start, the one straddling column 2^29 (from 2^30 columns
    on: the one straddling 2^30 - 2048) and the end; one window for a short object."""
    if L <= 3 * 4096:
        return [(0, L)]
    mid = MID if L < (1 << 30) else (1 << 30) - 2048
    return [(0, 4096), (mid - 2048, mid + 2048), (L - 4096, L)]


def host(t) -> np.ndarray:
    return t.cpu().numpy().view(np.uint32)


def check_windows(coeff, ins, outs, L, what):
    """The kernel's output against the C oracle on windows(L) of every row."""
    for a, b in windows(L):
        want = OC.apply_matrix(coeff, [host(x[a:b]) for x in ins])
        for i, o in enumerate(outs):
            got = host(o[a:b])
            assert np.array_equal(got, want[i]), (what, "row", i, "column", a + int(np.argmax(got != want[i])))


def check_same(got, want, what):
    d = BR.first_diff(got, want)
    assert d == -1, (what, "first differing element", d, hex(int(got[d]) & 0xFFFFFFFF),
                     hex(int(want[d]) & 0xFFFFFFFF))


def free(torch):
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ A. uniform apply, k <= 16

@pytest.mark.parametrize("padded", [False, True], ids=["dense", "padded"])
def test_encode_2_4_in_place_at_la(torch_dev, switches, padded):
    """Plan.encode(2, 4) in place at LA on the dynamic and the static schedule: in-shard byte
    offsets cross 2^31.  dense: shard stride L, so shard bases are 4- but not 16-byte aligned;
    padded: 64-element aligned strides with sentinel gaps."""
    torch = torch_dev
    from slime_amd import device as D
    L = LA
    ss = up64(L) if padded else L
    buf = torch.empty(4 * ss, dtype=torch.int32, device="cuda")
    D.fill_symbols(buf, 0xA11 + padded)
    for s in range(2):
        plant(torch, buf[s * ss: s * ss + L], s)
    buf[2 * ss:] = SENT
    plan = D.Plan.encode(2, 4)
    coeff = plan.coefficients()
    ins = [buf[s * ss: s * ss + L] for s in range(2)]
    outs = [buf[(2 + i) * ss: (2 + i) * ss + L] for i in range(2)]
    want = buf.clone()
    BR.apply_rows(coeff, ins, out=[want[(2 + i) * ss: (2 + i) * ss + L] for i in range(2)])
    lay = D.layout_of(4, L, ss)
    for schedule in (1, 0):
        switches(schedule=schedule)
        buf[2 * ss:] = SENT
        plan(buf, lay, buf, lay, L, 1, dst_offset=2 * ss)
        torch.cuda.synchronize()
        check_same(buf, want, ("schedule", schedule))
        check_windows(coeff, ins, outs, L, ("schedule", schedule))
    plan.close()
    del buf, want, ins, outs
    free(torch)


NONCANON_1X2 = np.array([[0xFFFFFFFF, P + 3]], dtype=np.uint32)  # = 4 and 3 mod p


def _matrix_1x2(torch, switches, L, expect_dynamic):
    from slime_amd import device as D
    src = torch.empty(2 * L, dtype=torch.int32, device="cuda")  # dense: shard 1 at byte 4L
    D.fill_symbols(src, 0xB22 + (L & 0xFF))
    ins = [src[:L], src[L:]]
    for s in range(2):
        plant(torch, ins[s], s)
    G = 64  # sentinel words before and after the one output shard
    dst = torch.empty(L + 2 * G, dtype=torch.int32, device="cuda")
    dst[:] = SENT
    want = dst.clone()
    plan = D.Plan.matrix(NONCANON_1X2, [0, 1])
    BR.apply_rows(NONCANON_1X2, ins, out=[want[G: G + L]])
    for schedule in (1, 0):
        switches(schedule=schedule)
        dst[:] = SENT
        before = N.schedule_counts(0)
        plan(src, D.layout_of(2, L), dst, D.layout_of(1, L), L, 1, dst_offset=G)
        torch.cuda.synchronize()
        after = N.schedule_counts(0)
        if schedule == 1:  # the rule taken by size: ncols < 2^30 runs the dynamic (pipelined) kernel
            assert after[0] - before[0] == expect_dynamic, (L, before, after)
            assert after[1] == before[1]
        else:
            assert after == before
        check_same(dst, want, (L, "schedule", schedule))
        check_windows(NONCANON_1X2, ins, [dst[G: G + L]], L, (L, "schedule", schedule))
    plan.close()
    del src, dst, want, ins
    free(torch)


def test_matrix_1x2_at_lb_takes_the_32_bit_forms(torch_dev, switches):
    """LB = 2^30 - 1, the last length of the pipelined kernels: the tail columns sit at bytes
    2^32 - 12 .. 2^32 - 4 of each shard and the dynamic-schedule count rises by one."""
    _matrix_1x2(torch_dev, switches, LB, 1)


def test_matrix_1x2_at_lc_takes_the_64_bit_forms(torch_dev, switches):
    """LC = 2^30: the first length `ncols < 2^30` refuses -- the dynamic count does not move."""
    _matrix_1x2(torch_dev, switches, LC, 0)


def test_matrix_1x2_at_ld_tail_past_4_gib(torch_dev, switches):
    """LD = 2^30 + 5: one tail column and a last whole vector past byte 2^32 of each shard."""
    _matrix_1x2(torch_dev, switches, LD, 0)


def test_matrix_1x2_at_la_bases_two_bytes_off(torch_dev):
    """Source and destination bases 2 bytes off a word boundary: the one-column-per-lane form,
    at LA.  Called through the C-ABI (a torch int32 view cannot sit at such an address); the
    bytes before and after the destination stay as they were."""
    torch = torch_dev
    from slime_amd import device as D
    L = LA
    al = torch.empty(2 * L, dtype=torch.int32, device="cuda")  # the sources, aligned, for the reference
    D.fill_symbols(al, 0xC33)
    ins = [al[:L], al[L:]]
    for s in range(2):
        plant(torch, ins[s], s)
    raw_src = torch.empty(8 * L + 16, dtype=torch.uint8, device="cuda")
    raw_src[2: 2 + 8 * L] = al.view(torch.uint8)
    raw_dst = torch.full((4 * L + 16,), 0x5A, dtype=torch.uint8, device="cuda")
    plan = D.Plan.matrix(NONCANON_1X2, [0, 1])
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    N.check(N.lib.slime_rs_plan_execute(plan._h, ctypes.c_void_p(raw_src.data_ptr() + 2), D.layout_of(2, L),
                                        ctypes.c_void_p(raw_dst.data_ptr() + 2), D.layout_of(1, L), L, 1, stream))
    torch.cuda.synchronize()
    assert raw_dst[:2].tolist() == [0x5A] * 2 and raw_dst[2 + 4 * L:].tolist() == [0x5A] * 14
    del raw_src
    got = raw_dst[2: 2 + 4 * L].clone().view(torch.int32)
    del raw_dst
    want = BR.apply_rows(NONCANON_1X2, ins)[0]
    check_same(got, want, "bases + 2 bytes")
    check_windows(NONCANON_1X2, ins, [got], L, "bases + 2 bytes")
    plan.close()
    del al, ins, got, want
    free(torch)


# ------------------------------------------------------------------ B. uniform apply, wide

def wide_coeff(rows, k, seed):
    rng = np.random.default_rng(seed)
    c = rng.integers(1, P, size=(rows, k), dtype=np.uint64).astype(np.uint32)
    c[0, 0], c[-1, -1], c[0, k // 2] = 0xFFFFFFFF, P - 1, P + 2  # non-canonical ones too
    return c


def _wide(torch, switches, k, rows, L, src_ss, forms, seed):
    """A rows x k plan over k source shards `src_ss` elements apart in one buffer (they overlap
    when src_ss < L: reads are reads), outputs on padded strides between sentinel gaps; one
    reference, one launch per form (keyword arguments of `switches`)."""
    from slime_amd import device as D
    src = torch.empty((k - 1) * src_ss + L, dtype=torch.int32, device="cuda")
    D.fill_symbols(src, seed)
    ins = [src[j * src_ss: j * src_ss + L] for j in range(k)]
    for j in range(k):
        plant(torch, ins[j], j)
    G, dss = 64, up64(L) + 64
    dst = torch.empty(G + rows * dss, dtype=torch.int32, device="cuda")
    dst[:] = SENT
    want = dst.clone()
    coeff = wide_coeff(rows, k, seed)
    plan = D.Plan.matrix(coeff, list(range(k)))
    BR.apply_rows(coeff, ins, out=[want[G + i * dss: G + i * dss + L] for i in range(rows)])
    outs = [dst[G + i * dss: G + i * dss + L] for i in range(rows)]
    for form in forms:
        switches(**form)
        dst[:] = SENT
        plan(src, D.layout_of(k, L, src_ss), dst, D.layout_of(rows, L, dss), L, 1, dst_offset=G)
        torch.cuda.synchronize()
        check_same(dst, want, (k, rows, L, form))
        check_windows(coeff, ins, outs, L, (k, rows, L, form))
    plan.close()
    del src, dst, want, ins, outs
    free(torch)


def test_wide_17x1_at_la_k32_pipe(torch_dev, switches):
    """17 inputs 64 elements apart in one 2 GiB buffer, LA columns: the k <= 32 pipelined
    kernel, on both schedules."""
    _wide(torch_dev, switches, 17, 1, LA, 64, [dict(schedule=1), dict(schedule=0)], 0xD17)


def test_wide_33x1_at_la_matrix_cores(torch_dev, switches):
    """33 inputs 64 elements apart, one output, LA columns: both spans are just over 2 GiB, so
    the launch is on the matrix cores with per-lane byte offsets in [2^31, 2^32); then the
    same on the VALU wide-pipe kernel."""
    k, L = 33, LA
    assert ((k - 1) * 64 + L) * 4 < 1 << 32 and L * 4 >= 1 << 31  # mfma_eligible's rule, both sides
    _wide(torch_dev, switches, k, 1, L, 64, [dict(matrix_cores=1), dict(matrix_cores=0)], 0xD33)


def test_wide_33x2_at_la(torch_dev, switches):
    """33 x 2 at LA with matrix_cores(1) and (0).  The two outputs cannot overlap, so the
    output side spans (stride + L) * 4 >= 2^32 bytes and the matrix-core rule hands the launch
    with matrix_cores(1) to the wide-pipe kernel as well: the rule's output side, taken by size
    (33 x 1 above is the shape that stays on the matrix cores at LA)."""
    assert (up64(LA) + 64 + LA) * 4 >= 1 << 32
    _wide(torch_dev, switches, 33, 2, LA, 64, [dict(matrix_cores=1), dict(matrix_cores=0)], 0xD34)


def test_wide_33x2_at_la_source_span_over_4_gib(torch_dev, switches):
    """33 sources 2^25 elements apart: the input side spans over 4 GiB, VALU by the rule."""
    assert (32 * (1 << 25) + LA) * 4 >= 1 << 32
    _wide(torch_dev, switches, 33, 2, LA, 1 << 25, [dict(matrix_cores=1)], 0xD35)


def test_wide_17x1_at_lc_non_pipelined(torch_dev, switches):
    """17 x 1 at LC = 2^30 columns: launch_wide_k, the 64-bit wide form."""
    _wide(torch_dev, switches, 17, 1, LC, 64, [dict()], 0xD18)


# ------------------------------------------------------------------ C. matrix-core limits, small L

def _limit_strides(in_max: int, L: int):
    """The largest 64-aligned stride with (in_max*stride + L)*4 < 2^32, and the next one."""
    under = ((1 << 30) - 1 - L) // in_max // 64 * 64
    assert (in_max * under + L) * 4 < 1 << 32 and (1 << 32) - (in_max * under + L) * 4 <= 256 * in_max
    assert (in_max * (under + 64) + L) * 4 >= 1 << 32
    return under, under + 64


def small_inputs(k, L, seed):
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 1 << 32, size=(k, L), dtype=np.uint64).astype(np.uint32)
    for j in range(k):
        x[j, rng.choice(L, size=EDGES.size, replace=False)] = EDGES
        x[j, :4], x[j, L - 4:] = EDGES[j % 7: j % 7 + 4], EDGES[(j + 3) % 7: (j + 3) % 7 + 4]
    return x


@pytest.mark.parametrize("case", ["both_under", "in_over", "out_over"])
def test_matrix_core_span_limits_small_l(torch_dev, switches, case):
    """33 x 2, L = 5507, shard strides that put (in_max*stride + L)*4 (and the same on the
    output side) as close under 2^32 as a 64-element aligned stride allows -- the matrix-core
    kernel with per-lane offsets up to the limit -- and each side in turn one step over it,
    where the rule hands the launch to the VALU kernels.  The 4 GiB buffers are barely
    touched; the whole destination is compared."""
    torch = torch_dev
    from slime_amd import device as D
    k, rows, L = 33, 2, SMALL
    in_under, in_over = _limit_strides(k - 1, L)
    out_under, out_over = _limit_strides(rows - 1, L)
    iss = in_over if case == "in_over" else in_under
    oss = out_over if case == "out_over" else out_under
    x = small_inputs(k, L, 0xC0 + len(case))
    coeff = wide_coeff(rows, k, 0xC1)
    ref = OC.apply_matrix(coeff, list(x))
    src = torch.empty((k - 1) * iss + L, dtype=torch.int32, device="cuda")
    for j in range(k):
        src[j * iss: j * iss + L] = torch.from_numpy(x[j].view(np.int32)).cuda()
    G = 64
    dst = torch.empty(G + (rows - 1) * oss + L + G, dtype=torch.int32, device="cuda")
    dst[:] = SENT
    want = dst.clone()
    for i in range(rows):
        want[G + i * oss: G + i * oss + L] = torch.from_numpy(ref[i].view(np.int32)).cuda()
    plan = D.Plan.matrix(coeff, list(range(k)))
    switches(matrix_cores=1)
    plan(src, D.layout_of(k, L, iss), dst, D.layout_of(rows, L, oss), L, 1, dst_offset=G)
    torch.cuda.synchronize()
    check_same(dst, want, (case, iss, oss))
    plan.close()
    del src, dst, want
    free(torch)


@pytest.mark.parametrize("matrix_cores", [1, 0])
def test_object_stride_over_2_32_elements(torch_dev, switches, matrix_cores):
    """Two 33/35 objects 2^32 + 64 elements (over 16 GiB) apart in one buffer, encoded in
    place: the object stride is a 64-bit quantity on every kernel form."""
    torch = torch_dev
    from slime_amd import device as D
    k, rows, L, nobj = 33, 2, SMALL, 2
    ss, ostride, G = up64(L), (1 << 32) + 64, 4096
    span = (k + rows) * ss
    buf = torch.empty(ostride + span + G, dtype=torch.int32, device="cuda")
    coeff = wide_coeff(rows, k, 0xC2)
    plan = D.Plan.matrix(coeff, list(range(k)))
    wants = []
    for o in range(nobj):
        x = small_inputs(k, L, 0xC3 + o)
        ref = OC.apply_matrix(coeff, list(x))
        region = np.full(span + G, SENT, dtype=np.uint32)
        for j in range(k):
            region[j * ss: j * ss + L] = x[j]
        buf[o * ostride: o * ostride + span + G] = torch.from_numpy(region.view(np.int32)).cuda()
        for i in range(rows):
            region[(k + i) * ss: (k + i) * ss + L] = ref[i]
        wants.append(region)
    switches(matrix_cores=matrix_cores)
    lay = N.Layout(obj_stride=ostride, shard_stride=ss)
    plan(buf, lay, buf, lay, L, nobj, dst_offset=k * ss)
    torch.cuda.synchronize()
    for o in range(nobj):
        got = host(buf[o * ostride: o * ostride + span + G])
        bad = np.flatnonzero(got != wants[o])
        assert bad.size == 0, (o, "first differing element", int(bad[0]))
    plan.close()
    del buf
    free(torch)


# ------------------------------------------------------------------ D. uniform verify

def flip_columns(L: int):
    """Columns 0, 2^29 - 1, 2^29, the last column of the last whole vector, every tail column."""
    cols = [0, MID - 1, MID, 4 * (L // 4) - 1] + list(range(4 * (L // 4), L))
    return sorted(set(c for c in cols if 0 <= c < L))


def _verify(torch, switches, plan, coeff, ins, cmp_views, call, L, overlap=0):
    """cmp_views hold bigref's rows.  Clean, then stored words flipped (row 0: flip_columns,
    last row: column 2^29 alone), then one input word corrupted at a column >= 2^29; on both
    schedules.  overlap: the inputs are views of one buffer `overlap` elements apart, so the
    corrupted word is input j's column at + (k-1-j)*overlap for every j where that is below L."""
    rows, k = coeff.shape
    cols = flip_columns(L)
    at = MID + 77
    hit = sum(1 for j in range(k) if at + (k - 1 - j) * overlap < L) if overlap else 1
    assert all(int(coeff[i, j]) % P != 0 for i in range(rows) for j in (range(k) if overlap else [k - 1]))
    check_windows(coeff, ins, cmp_views, L, "bigref's stored rows")
    for schedule in (1, 0):
        switches(schedule=schedule)
        mism, first = call()
        assert mism.tolist() == [[0] * rows] and first.tolist() == [[-1] * rows], ("clean", schedule, mism, first)
        for c in cols:
            cmp_views[0][c] ^= 1
        if rows > 1:
            cmp_views[rows - 1][MID] ^= 1 << 31
        mism, first = call()
        want_m = [len(cols)] + [0] * (rows - 2) + ([1] if rows > 1 else [])
        want_f = [cols[0]] + [-1] * (rows - 2) + ([MID] if rows > 1 else [])
        for c in cols:
            cmp_views[0][c] ^= 1
        if rows > 1:
            cmp_views[rows - 1][MID] ^= 1 << 31
        assert mism.tolist() == [want_m] and first.tolist() == [want_f], ("stored", schedule, mism, first)
        ins[k - 1][at] ^= 0x10  # every row's coefficient of this input is non-zero
        mism, first = call()
        ins[k - 1][at] ^= 0x10
        assert mism.tolist() == [[hit] * rows] and first.tolist() == [[at] * rows], ("input", schedule, mism, first)


@pytest.mark.parametrize("L", [LA, LC], ids=["la", "lc"])
def test_verify_encode_2_4(torch_dev, switches, L):
    """Plan.verify of 2/4 codewords whose parity bigref wrote, in place: at LA the pipelined
    form, at LC = 2^30 columns the 64-bit form (16 GiB, two rows with their own `first`)."""
    torch = torch_dev
    from slime_amd import device as D
    ss = up64(L)
    buf = torch.empty(4 * ss, dtype=torch.int32, device="cuda")
    D.fill_symbols(buf, 0xE11)
    ins = [buf[s * ss: s * ss + L] for s in range(2)]
    for s in range(2):
        plant(torch, ins[s], s)
    plan = D.Plan.encode(2, 4)
    coeff = plan.coefficients()
    outs = [buf[(2 + i) * ss: (2 + i) * ss + L] for i in range(2)]
    BR.apply_rows(coeff, ins, out=outs)
    lay = D.layout_of(4, L, ss)
    _verify(torch, switches, plan, coeff, ins, outs,
            lambda: plan.verify(buf, lay, buf, lay, L, 1, cmp_offset=2 * ss), L)
    plan.close()
    del buf, ins, outs
    free(torch)


@pytest.mark.parametrize("L", [LA, LC], ids=["la", "lc"])
def test_verify_matrix_1x2(torch_dev, switches, L):
    """Plan.verify of the non-canonical 1 x 2 plan over dense shards, at LA and at LC."""
    torch = torch_dev
    from slime_amd import device as D
    src = torch.empty(2 * L, dtype=torch.int32, device="cuda")
    D.fill_symbols(src, 0xE22)
    ins = [src[:L], src[L:]]
    for s in range(2):
        plant(torch, ins[s], s)
    cmp = torch.empty(L, dtype=torch.int32, device="cuda")
    plan = D.Plan.matrix(NONCANON_1X2, [0, 1])
    BR.apply_rows(NONCANON_1X2, ins, out=[cmp])
    _verify(torch, switches, plan, NONCANON_1X2, ins, [cmp],
            lambda: plan.verify(src, D.layout_of(2, L), cmp, D.layout_of(1, L), L, 1), L)
    plan.close()
    del src, cmp, ins
    free(torch)


def test_verify_17x1_at_la(torch_dev, switches):
    """Plan.verify of a 17 x 1 plan at LA: the column form wide codes take."""
    torch = torch_dev
    from slime_amd import device as D
    k, L = 17, LA
    src = torch.empty((k - 1) * 64 + L, dtype=torch.int32, device="cuda")
    D.fill_symbols(src, 0xE33)
    ins = [src[j * 64: j * 64 + L] for j in range(k)]
    for j in range(k):
        plant(torch, ins[j], j)
    cmp = torch.empty(L, dtype=torch.int32, device="cuda")
    coeff = wide_coeff(1, k, 0xE34)
    plan = D.Plan.matrix(coeff, list(range(k)))
    BR.apply_rows(coeff, ins, out=[cmp])
    _verify(torch, switches, plan, coeff, ins, [cmp],
            lambda: plan.verify(src, D.layout_of(k, L, 64), cmp, D.layout_of(1, L), L, 1), L, overlap=64)
    plan.close()
    del src, cmp, ins
    free(torch)


# ------------------------------------------------------------------ E. ragged, planned, ragged verify

FORMS = [dict(schedule=s, pipeline=p) for s in (1, 0) for p in (1, 0)]
SS0 = (1 << 30) + 64  # shard stride of the big object and of the far-strided small one
OFF1 = (1 << 32) + 4096  # the small object whose offsets need 33 bits


def _ragged_spans(L0, far_strided):
    """(src_off, shard stride, L) per object, in one in-place 2/4 tensor of 2^32 + 65536
    elements (16 GiB): the big object at 0 with shards 2^30 + 64 apart; a 5507-column object
    whose shards are 2^30 + 64 apart too, each right behind a shard of the big one (only when
    they fit there: far_strided); a 5507-column object at element 2^32 + 4096; a 7-column object."""
    spans = [(0, SS0, L0)]
    if far_strided:
        spans.append((up64(L0) + 64, SS0, SMALL))
    spans += [(OFF1, up64(SMALL), SMALL), (OFF1 + 32768, 64, 7)]
    return spans, OFF1 + 65536


def _guards(spans):
    """Sentinel words behind every shard of every object: 61 or more up to the next thing."""
    return [(off + s * ss + L, 57) for off, ss, L in spans for s in range(4)]


def _ragged_fill(torch, buf, spans, seed):
    """Sources: fill_symbols + EDGES for the big object, host words for the small ones; sentinel
    in every parity shard and guard.  Returns the small objects' full 4-shard codewords (oracle)."""
    from slime_amd import device as D
    coeff = D.Plan.encode(2, 4).coefficients()
    small = {}
    for o, (off, ss, L) in enumerate(spans):
        if o == 0:
            for s in range(2):
                D.fill_symbols(buf[off + s * ss: off + s * ss + L], seed + s)
                plant(torch, buf[off + s * ss: off + s * ss + L], s)
        else:
            x = small_inputs(2, L, seed + 16 * o) if L > 16 else np.resize(EDGES, 2 * L).reshape(2, L).copy()
            small[o] = np.stack(list(x) + OC.apply_matrix(coeff, list(x)))
            for s in range(2):
                buf[off + s * ss: off + s * ss + L] = torch.from_numpy(x[s].view(np.int32)).cuda()
        for s in (2, 3):
            buf[off + s * ss: off + s * ss + L] = SENT
    for a, n in _guards(spans):
        buf[a: a + n] = SENT
    return coeff, small


def _shard(buf, span, s):
    off, ss, L = span
    return buf[off + s * ss: off + s * ss + L]


def _check_guards(buf, spans, what):
    for a, n in _guards(spans):
        assert bool((buf[a: a + n] == SENT).all()), (what, "guard at", a)


def _check_small(buf, spans, small, shards, what, canonical=False):
    for o, cw in small.items():
        for s in shards.get(o, ()):
            want = cw[s] % np.uint32(P) if canonical else cw[s]
            got = host(_shard(buf, spans[o], s))
            assert np.array_equal(got, want), (what, "object", o, "shard", s, int(np.argmax(got != want)))


def _results(nobj, hits):
    """(mismatches, first) lists of an nobj x 2 result with hits = {(object, row): (count, first)}."""
    m, f = [[0, 0] for _ in range(nobj)], [[-1, -1] for _ in range(nobj)]
    for (o, r), (n, c) in hits.items():
        m[o][r], f[o][r] = n, c
    return m, f


def _canon_(t):
    """t mod p in place, a chunk at a time: what a repair rebuilds of a non-canonical data shard."""
    for c0 in range(0, t.numel(), BR.CHUNK):
        t[c0: c0 + BR.CHUNK] = BR.i32(BR.u32(t[c0: c0 + BR.CHUNK]) % P)


def _ragged_case(torch, switches, L0, far_strided, seed):
    """execute_batch, verify_batch (clean, stored words flipped, an input word corrupted), then
    the same spans as a planned batch -- pattern {1, 3} for the big (and the far-strided) object,
    {0} for the object past element 2^32, the 7-column object NO_PLAN -- through
    PlanSet.execute_batch and PlanSet.verify_batch; all of it on both schedules and on the
    pipelined and non-pipelined forms.  The big object's reference rows are bigref's, written
    into one stash and compared one at a time: the 16 GiB tensor and the stash of one shard are
    all that is alive."""
    from slime_amd import device as D
    spans, total = _ragged_spans(L0, far_strided)
    nobj = len(spans)
    o_far, o_at, o_7 = (1 if far_strided else None), nobj - 2, nobj - 1
    buf = torch.empty(total, dtype=torch.int32, device="cuda")
    coeff, small = _ragged_fill(torch, buf, spans, seed)
    big = spans[0]
    ins = [_shard(buf, big, s) for s in range(2)]
    stash = torch.empty(L0, dtype=torch.int32, device="cuda")
    sums = [int(x.sum(dtype=torch.int64)) for x in ins]
    rows_spans = [(off, ss, off, ss, L) for off, ss, L in spans]
    batch = D.Batch(rows_spans, 2)
    enc = D.Plan.encode(2, 4).set_outputs([2, 3])
    patterns = [[1, 3]] + ([[1, 3]] if far_strided else []) + [[0], None]
    pset, plan_of = D.PlanSet.for_erasures(2, 4, patterns)
    assert plan_of.tolist() == [0] + ([0] if far_strided else []) + [1, N.NO_PLAN]
    pbatch = D.Batch(rows_spans, 2, plans=plan_of, nplans=pset.nplans)
    rec = D.Plan.reconstruct(2, 4, [0, 2], [1, 3])
    assert (rec.coefficients() % P != 0).all()  # every survivor word reaches both rebuilt rows
    rec.close()
    cols = flip_columns(L0)
    at = MID + 77

    def flip(sites):
        for o, s, c, bit in sites:
            _shard(buf, spans[o], s)[c] ^= bit

    for form in FORMS:
        switches(**form)
        for o in range(nobj):
            for s in (2, 3):
                _shard(buf, spans[o], s)[:] = SENT
        enc.execute_batch(buf, buf, batch)
        torch.cuda.synchronize()
        for i in range(2):
            BR.apply_rows(coeff[i: i + 1], ins, out=[stash])
            check_same(_shard(buf, big, 2 + i), stash, (form, "execute_batch row", i))
        check_windows(coeff, ins, [_shard(buf, big, 2), _shard(buf, big, 3)], L0, (form, "execute_batch"))
        _check_small(buf, spans, small, {o: (0, 1, 2, 3) for o in small}, (form, "execute_batch"))
        _check_guards(buf, spans, (form, "execute_batch"))
        # ragged verify: clean, stored words flipped, one input word corrupted
        m, f = enc.verify_batch(buf, buf, batch)
        assert (m.tolist(), f.tolist()) == _results(nobj, {}), (form, "clean", m, f)
        sites = [(0, 2, c, 1) for c in cols] + [(0, 3, MID, 1 << 31), (o_at, 3, SMALL - 1, 1), (o_7, 2, 6, 1)]
        hits = {(0, 0): (len(cols), 0), (0, 1): (1, MID), (o_at, 1): (1, SMALL - 1), (o_7, 0): (1, 6)}
        if far_strided:
            sites.append((o_far, 2, 0, 1))
            hits[(o_far, 0)] = (1, 0)
        flip(sites)
        m, f = enc.verify_batch(buf, buf, batch)
        flip(sites)
        assert (m.tolist(), f.tolist()) == _results(nobj, hits), (form, "stored", m, f)
        flip([(0, 1, at, 0x10)])
        m, f = enc.verify_batch(buf, buf, batch)
        flip([(0, 1, at, 0x10)])
        assert (m.tolist(), f.tolist()) == _results(nobj, {(0, 0): (1, at), (0, 1): (1, at)}), (form, "input", m, f)
        # planned repair: erase, rebuild each object by its own plan, compare with what was there
        # (stash holds bigref's row 1, the big object's shard 3)
        erased = {0: (1, 3), o_at: (0,)}
        if far_strided:
            erased[o_far] = (1, 3)
        for o, shards in erased.items():
            for s in shards:
                _shard(buf, spans[o], s)[:] = SENT
        pset.execute_batch(buf, buf, pbatch)
        torch.cuda.synchronize()
        check_same(_shard(buf, big, 3), stash, (form, "repair of shard 3"))
        D.fill_symbols(stash, seed + 1)  # data shard 1 as _ragged_fill made it, then mod p
        plant(torch, stash, 1)
        _canon_(stash)
        check_same(_shard(buf, big, 1), stash, (form, "repair of shard 1"))
        BR.apply_rows(coeff[0:1], ins, out=[stash])  # shard 1 is canonical now: the same row mod p
        check_same(_shard(buf, big, 2), stash, (form, "survivor shard 2"))
        _check_small(buf, spans, small, erased, (form, "repair"), canonical=True)
        kept = {o: tuple(s for s in range(4) if s not in erased.get(o, ())) for o in small}
        _check_small(buf, spans, small, kept, (form, "repair leaves"))
        _check_guards(buf, spans, (form, "repair"))
        m, f = pset.verify_batch(buf, buf, pbatch)
        assert (m.tolist(), f.tolist()) == _results(nobj, {}), (form, "planned clean", m, f)
        # an intact (NO_PLAN) object is not looked at; the far-strided one stays clean
        sites = [(0, 1, c, 1) for c in cols] + [(0, 3, MID, 1 << 31), (o_at, 0, SMALL - 1, 1), (o_7, 2, 6, 1)]
        hits = {(0, 0): (len(cols), 0), (0, 1): (1, MID), (o_at, 0): (1, SMALL - 1)}
        flip(sites)
        m, f = pset.verify_batch(buf, buf, pbatch)
        flip(sites)
        assert (m.tolist(), f.tolist()) == _results(nobj, hits), (form, "planned stored", m, f)
        flip([(0, 0, at, 0x10)])
        m, f = pset.verify_batch(buf, buf, pbatch)
        flip([(0, 0, at, 0x10)])
        assert (m.tolist(), f.tolist()) == _results(nobj, {(0, 0): (1, at), (0, 1): (1, at)}), (form, "planned input", m, f)
        # the repair left rebuilt data shards canonical: put the non-canonical sources back
        D.fill_symbols(ins[1], seed + 1)
        plant(torch, ins[1], 1)
        for o in small:
            for s in range(2):
                _shard(buf, spans[o], s)[:] = torch.from_numpy(small[o][s].view(np.int32)).cuda()
        assert [int(x.sum(dtype=torch.int64)) for x in ins] == sums, (form, "sources changed")
    for h in (batch, pbatch, pset, enc):
        h.close()
    del buf, ins, stash
    free(torch)


def test_ragged_batch_in_one_16_gib_tensor(torch_dev, switches):
    """One in-place 2/4 tensor of 16 GiB: an object at LA with shard strides over 4 GiB, a small
    object with the same strides, a small object past element 2^32 and a 7-column one."""
    _ragged_case(torch_dev, switches, LA, True, 0xE50)


def test_ragged_batch_with_lb(torch_dev, switches):
    """The same legs with LB = 2^30 - 1 columns in the big object, the last length a batch
    accepts (2^30 is refused, here and in tests/test_ragged_host.py).  Four 4 GiB shards leave
    no room for the far-strided small object inside 20 GiB, so the batch holds the other three."""
    from slime_amd import device as D
    with pytest.raises(N.NativeError, match="2\\^30"):
        D.Batch([(0, SS0, 0, SS0, 1 << 30)], 2)
    _ragged_case(torch_dev, switches, LB, False, 0xE60)


# ------------------------------------------------------------------ C (bytes). matrix-core limit of the byte path

def _band_free(words: np.ndarray) -> np.ndarray:
    """No word in a MapToGF band: none >= p, none in [p ^ 2^31, 2^31)."""
    w = words.copy()
    w[(w >= P) | ((w >= (P ^ (1 << 31))) & (w < (1 << 31)))] = 0x12345678
    return w


@pytest.mark.parametrize("over", [False, True], ids=["under", "over"])
@pytest.mark.parametrize("kind", ["encode", "decode"])
def test_byte_path_matrix_core_limit(torch_dev, switches, kind, over):
    """33/40 byte objects of L = 5507 on chunk strides that put (hi_chunk + 1)*chunk_stride + 4L
    just under 2^32 (the matrix-core byte kernel with window offsets up to the limit) and at or
    over it (the VALU kernels by the rule); hi_chunk as the launcher counts it: k + the highest
    output index, or the highest input chunk.  Object 0 maps with 0, object 1 with 1<<31.  The
    whole 2 x 4.x GiB of slots is compared, gaps between chunks included."""
    torch = torch_dev
    from slime_amd import device as D
    need, total, L, nobj = 33, 40, SMALL, 2
    erase = [0, 3]
    have = [c for c in range(total) if c not in erase][:need]
    hi = total - 1 if kind == "encode" else max(need + max(erase), max(have))
    cs = ((1 << 32) - 4 * L - 1) // (hi + 1) // 256 * 256
    assert (hi + 1) * cs + 4 * L < 1 << 32 and (hi + 1) * (cs + 256) + 4 * L >= 1 << 32
    cs += 256 if over else 0
    slot = total * cs
    enc = D.Plan.encode(need, total)
    coeff = enc.coefficients()
    rng = np.random.default_rng(0xCB + over)
    chunks, maps = [], []
    for o in range(nobj):
        w = _band_free(rng.integers(0, 1 << 32, size=need * L, dtype=np.uint64).astype(np.uint32))
        if o == 1:
            w[100] = 0xFFFFFFFE
        rc, m, words = OC.map_to_gf(w.astype(">u4").tobytes())
        assert rc == 0 and m == (0, 1 << 31)[o]
        parts = [np.ascontiguousarray(words[j * L: (j + 1) * L]) for j in range(need)]
        chunks.append([np.frombuffer(OC.map_from_gf(m, p), dtype=np.uint8) for p in parts + OC.apply_matrix(coeff, parts)])
        maps.append(m)
    want = torch.full((nobj * slot,), 0x5A, dtype=torch.uint8, device="cuda")
    for o in range(nobj):
        for c in range(total):
            want[o * slot + c * cs: o * slot + c * cs + 4 * L] = torch.from_numpy(chunks[o][c].copy()).cuda()
    slots = want.clone()
    wiped = range(need, total) if kind == "encode" else erase
    for o in range(nobj):
        for c in wiped:
            slots[o * slot + c * cs: o * slot + c * cs + 4 * L] = 0x5A
    switches(matrix_cores=1)
    mapping = torch.full((nobj,), -1, dtype=torch.int32, device="cuda")
    if kind == "encode":
        status = torch.full((nobj,), -1, dtype=torch.int32, device="cuda")
        D.encode_objects(enc, slots, slot, 4 * need * L, nobj, mapping, status, chunk_stride=cs)
        torch.cuda.synchronize()
        assert status.tolist() == [0, 0] and host(mapping).tolist() == maps
    else:
        mapping[:] = torch.from_numpy(np.array(maps, dtype=np.uint32).view(np.int32)).cuda()
        rec = D.Plan.reconstruct(need, total, have, erase).set_outputs(erase)
        D.decode_objects(rec, slots, slot, L, nobj, mapping, chunk_stride=cs)
        torch.cuda.synchronize()
        rec.close()
    d = BR.first_diff(slots, want)
    assert d == -1, (kind, over, "object", d // slot, "chunk", d % slot // cs, "byte", d % slot % cs)
    enc.close()
    del slots, want
    free(torch)


# ------------------------------------------------------------------ F. byte objects with chunks over 2 GiB

def _object_words(torch, L, need, o, j):
    """Canonical words of data chunk j of object o, no word in a MapToGF band: the mapping is 0
    by construction.  Object 1 ends in 0xFFFFFFFD: its mapping is 1<<31 and every earlier unit
    of the first pass is redone."""
    from slime_amd import device as D
    w = torch.empty(L, dtype=torch.int32, device="cuda")
    D.fill_symbols(w, 0xF00 + 16 * o + j)
    w.masked_fill_(w >= 0x7FFFFFFB, 0x12345678)           # [p ^ 2^31, 2^31)
    w.masked_fill_((w < 0) & (w >= -5), 0x12345678)       # >= p
    if o == 1 and j == need - 1:
        w[L - 1] = -3
    return w


def _byte_objects(torch, switches, need, total, L):
    from slime_amd import device as D
    assert total == need + 1
    nobj, chunk = 2, 4 * L
    S, slot = need * chunk, total * chunk
    maps = [0, 1 << 31]
    slots = torch.empty(nobj * slot, dtype=torch.uint8, device="cuda")
    enc = D.Plan.encode(need, total)
    coeff = enc.coefficients()

    def at(o, c):
        return slots[o * slot + c * chunk: o * slot + (c + 1) * chunk]

    exp = []  # the parity chunk's bytes of each object: bigref's row + MapFromGF's framing
    for o in range(nobj):
        ws = []
        for j in range(need):
            w = _object_words(torch, L, need, o, j)
            BR.be_bytes(w, 0, out=at(o, j))
            ws.append(w ^ (-(1 << 31)) if maps[o] else w)
            del w
        par = BR.apply_rows(coeff, ws)[0]
        del ws
        exp.append(BR.be_bytes(par, maps[o]))
        del par
    mapping = torch.empty(nobj, dtype=torch.int32, device="cuda")
    status = torch.empty(nobj, dtype=torch.int32, device="cuda")
    for switch_bits in (0, 2):  # 0: at this size the top-bit correction by rule; 2: re-encode
        for schedule in (1, 0):
            switches(schedule=schedule, switch_bits=switch_bits)
            what = ("switch_bits", switch_bits, "schedule", schedule)
            mapping[:] = -1
            status[:] = -1
            for o in range(nobj):
                at(o, need)[:] = 0x5A
            D.encode_objects(enc, slots, slot, S, nobj, mapping, status)
            torch.cuda.synchronize()
            assert status.tolist() == [0, 0] and host(mapping).tolist() == maps, (what, status, mapping)
            for o in range(nobj):
                d = BR.first_diff(at(o, need), exp[o])
                assert d == -1, (what, "object", o, "parity byte", d)
    def check_data(what):  # every data chunk holds the object's bytes
        for o in range(nobj):
            for j in range(need):
                b = BR.be_bytes(_object_words(torch, L, need, o, j))
                d = BR.first_diff(at(o, j), b)
                assert d == -1, (what, "object", o, "data chunk", j, "byte", d)
                del b

    check_data("after the encodes")
    for o in range(nobj):  # the oracle's framing on three windows of the parity the last encode wrote
        for a, b in windows(L):
            ws = [OC.map_to_gf_with(at(o, j)[4 * a: 4 * b].cpu().numpy().tobytes(), maps[o]) for j in range(need)]
            want = OC.map_from_gf(maps[o], OC.apply_matrix(coeff, ws)[0])
            assert at(o, need)[4 * a: 4 * b].cpu().numpy().tobytes() == want, ("oracle window", o, a)
    scrub = D.Plan.encode(need, total).set_outputs([need])  # stored parity read at chunk `need`
    m, f = D.verify_objects(scrub, slots, slot, L, nobj, mapping)
    assert m.tolist() == [[0], [0]] and f.tolist() == [[-1], [-1]], (m, f)
    at(1, need)[chunk - 1] ^= 0x40  # the last byte of the last slot: column L - 1
    m, f = D.verify_objects(scrub, slots, slot, L, nobj, mapping)
    at(1, need)[chunk - 1] ^= 0x40
    assert m.tolist() == [[0], [1]] and f.tolist() == [[-1], [L - 1]], (m, f)
    scrub.close()
    # decode: chunk 0 from the others, then the parity chunk from the data
    rec0 = D.Plan.reconstruct(need, total, list(range(1, total)), [0]).set_outputs([0])
    for o in range(nobj):
        at(o, 0)[:] = 0x5A
    D.decode_objects(rec0, slots, slot, L, nobj, mapping)
    recp = D.Plan.reconstruct(need, total, list(range(need)), [need]).set_outputs([need])
    for o in range(nobj):
        at(o, need)[:] = 0x5A
    D.decode_objects(recp, slots, slot, L, nobj, mapping)
    torch.cuda.synchronize()
    for o in range(nobj):
        d = BR.first_diff(at(o, need), exp[o])
        assert d == -1, ("decode", "object", o, "parity byte", d)
    del exp
    check_data("after the decodes")  # chunk 0 rebuilt byte for byte, the others left alone
    for h in (enc, rec0, recp):
        h.close()
    del slots
    free(torch)


def test_byte_objects_2_3_chunks_over_2_gib(torch_dev, switches):
    """2/3 objects of S = 8 LA bytes: chunks just over 2 GiB, S and the slot cross 2^32."""
    _byte_objects(torch_dev, switches, 2, 3, LA)


def test_byte_objects_3_4_chunks_over_1_gib(torch_dev, switches):
    """3/4 at L = 2^28 + 259: chunks of 1 GiB, only S and the slot cross 2^31 and 2^32 -- a
    failure here and not above is in the object's offsets, not in the chunk's."""
    _byte_objects(torch_dev, switches, 3, 4, (1 << 28) + 259)
