"""The field's boundary values on the GPU: steered sums and mapping words.

Every data kernel ends in fold96 plus one conditional subtract of p
(slime_amd/csrc/gfp.hpp); random data takes the fold's rare branches
(`u >> 32 == 1`, `w >= p`) with probability about 2^-30 a column.  Here the
inputs are steered (tests/steering.py): r inputs of a column are solved so
that its output rows are chosen residues -- 0..40, p-40..p-1, 2^31-2..2^31+2,
64 columns each, rolled by row, plus 0..4 in the three columns past the last
whole vector.  tests/test_steering.py asserts, without a GPU, that these
columns reach every branch for every code used here.

Steering only chooses inputs.  Every expectation is the C oracle applied to
those inputs (apply_matrix / encode_object / recover_data / map_to_gf and the
writeChunks framing), and every comparison is bit for bit over whole buffers.
The steered columns lie in the middle object of a batch of 2-3, one launch a
case; references are computed once per code and shared by the kernel forms.

The second half plants MapToGF's threshold words (p-1 / p, and p ^ 2^31 - 1 /
p ^ 2^31) in device byte objects: the three device flag computations (the VALU
byte encode, the matrix-core encode, the codec kernel) against OC.map_to_gf.
"""
import ctypes

import numpy as np
import pytest

import steering as ST
from slime_amd import _native as N
from slime_amd import gf
from oracle import oracle_c as OC
from oracle import oracle_py as OP

pytestmark = pytest.mark.gpu

P = ST.P
L = ST.NCOLS                 # 5507 columns: several tiles at every geometry, L % 4 == 3
SS = -(-L // 64) * 64        # shard stride, 256-byte aligned
NOBJ = 3
HIGH = 1 << 31


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    assert N.device_count() > 0
    return torch


@pytest.fixture
def forms():
    """The process-wide kernel switches, saved and restored: call
    forms(schedule=, pipeline=, matrix_cores=, switch_bits=) to set any."""
    fns = {"schedule": N.lib.slime_rs_kernel_schedule, "pipeline": N.lib.slime_rs_kernel_pipeline,
           "matrix_cores": N.lib.slime_rs_kernel_matrix_cores, "switch_bits": N.lib.slime_rs_switch_bits}
    before = {name: fn(-1) for name, fn in fns.items()}

    def set_forms(**kw):
        for name, mode in kw.items():
            assert fns[name](mode) == 0 and fns[name](-1) == mode, (name, mode)

    yield set_forms
    for name, fn in fns.items():
        fn(before[name])


def to_dev(torch, a):
    return torch.from_numpy(np.array(a, dtype=np.uint32).view(np.int32).reshape(-1)).cuda()  # a writable copy


def to_host(torch, t):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint32)


def shifted(torch, a, off):
    """a's bytes at byte offset `off` of a 0xA5-filled byte tensor: a base off a 4-byte boundary."""
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    b = np.full(raw.size + 8, 0xA5, dtype=np.uint8)
    b[off: off + raw.size] = raw
    return torch.from_numpy(b).cuda()


def unshifted(torch, t, off, shape):
    torch.cuda.synchronize()
    h = t.cpu().numpy()
    n = int(np.prod(shape)) * 4
    assert (h[:off] == 0xA5).all() and (h[off + n:] == 0xA5).all(), "wrote around the destination"
    return h[off: off + n].copy().view(np.uint32).reshape(shape)


def canon(a):
    return np.where(a >= P, a - np.uint32(P), a).astype(np.uint32)


def apply_rows(coeff, ins3):
    """The oracle's rows over [nobj][k][cols] inputs -> [nobj][rows][cols], in one call."""
    nobj, k, cols = ins3.shape
    wide = np.ascontiguousarray(ins3.transpose(1, 0, 2).reshape(k, nobj * cols))
    out = OC.apply_matrix(coeff, list(wide))
    return np.stack(out).reshape(len(out), nobj, cols).transpose(1, 0, 2)


_cache = {}


def cached(key, make):
    if key not in _cache:
        val = make()
        for a in val if isinstance(val, tuple) else (val,):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[key] = val
    return _cache[key]


# ------------------------------------------------------------------ symbol apply

def symbol_case(need, total, prefix=None):
    """(init, want): [NOBJ][total][SS] with random (full uint32 range) data
    shards, the middle object's the steered inputs; `want` has the parity
    shards' L columns as the oracle encodes them, everything else untouched."""
    def make():
        coeff, x, tg, mask = ST.encode_case(need, total, prefix)
        rng = np.random.default_rng([need, total, 7])
        init = rng.integers(0, 2**32, size=(NOBJ, total, SS), dtype=np.uint64).astype(np.uint32)
        init[1, :need, :L] = x
        want = init.copy()
        want[:, need:, :L] = apply_rows(coeff, init[:, :need, :L])
        if prefix is None:  # the steering held: the oracle's parity of the steered object is the targets
            for i in range(total - need):
                assert np.array_equal(want[1, need + i, :L][mask[i]], tg[i][mask[i]])
        return init, want
    return cached(("sym", need, total, prefix), make)


def run_encode(torch, need, total, prefix=None):
    from slime_amd import device as D
    init, want = symbol_case(need, total, prefix)
    buf = to_dev(torch, init)
    lay = D.layout_of(total, L, SS)
    D.Plan.encode(need, total)(buf, lay, buf, lay, L, NOBJ, dst_offset=need * SS)
    got = to_host(torch, buf).reshape(NOBJ, total, SS)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"first differing (object, shard, column): {bad[0]}, {len(bad)} in all"


ENCODE_FORMS = [(need, total, sched, pipe, mc) for need, total in ST.ENCODE_CODES for sched in (1, 0)
                for pipe in (1, 0) for mc in ((1, 0) if need > 16 else (1,))]


@pytest.mark.parametrize("need,total,sched,pipe,mc", ENCODE_FORMS)
def test_encode_steered_rows_every_form(torch_dev, forms, need, total, sched, pipe, mc):
    """Encode with every parity row of the middle object steered onto the
    target residues, in every kernel form: schedule {1, 0} x pipeline {1, 0},
    and the wide codes (k > 16) on the matrix cores and on the VALU kernels."""
    forms(schedule=sched, pipeline=pipe, matrix_cores=mc)
    run_encode(torch_dev, need, total)


@pytest.mark.parametrize("mc", [1, 0], ids=["matrix_cores", "valu"])
@pytest.mark.parametrize("need,total,prefix", ST.PREFIXES)
def test_encode_steered_prefix_sums(torch_dev, forms, need, total, prefix, mc):
    """k > 16: the partial sum over the first 16, 32 or 48 inputs is steered,
    which is what a kernel that folds a running residue every 16 inputs folds there."""
    forms(matrix_cores=mc)
    run_encode(torch_dev, need, total, prefix)


@pytest.mark.parametrize("need,total", ST.ENCODE_CODES)
def test_encode_steered_rows_unaligned_base(torch_dev, need, total):
    """src and dst two bytes off a 4-byte boundary: the one-column-per-lane form."""
    from slime_amd import device as D
    torch = torch_dev
    init, want = symbol_case(need, total)
    rows = total - need
    src = shifted(torch, init[:, :need, :L], 2)
    dst = shifted(torch, np.full((NOBJ, rows, L), 0xA5A5A5A5, dtype=np.uint32), 2)
    plan = D.Plan.encode(need, total)
    N.check(N.lib.slime_rs_plan_execute(plan._h, ctypes.c_void_p(src.data_ptr() + 2), D.layout_of(need, L),
                                        ctypes.c_void_p(dst.data_ptr() + 2), D.layout_of(rows, L), L, NOBJ, None))
    got = unshifted(torch, dst, 2, (NOBJ, rows, L))
    assert np.array_equal(got, want[:, need:, :L])


SAT_COEFF = np.array([1, P - 1, 127 * 0x01010101, P - 128 * 0x01010101, HIGH], dtype=np.uint32)
SAT_WORD = np.array([0, 0x80808080, 0x7F7F7F7F, 0xFFFFFFFF], dtype=np.uint32)


def saturated_case(k):
    """8 rows x k coefficients and [2][k][L] inputs, all from the saturated
    sets (every digit of the matrix-core table and every input byte at an edge
    of its int8 window): five rows of one coefficient each and three mixed;
    20 columns of one word each against every row, the rest mixed."""
    def make():
        rng = np.random.default_rng(k)
        coeff = np.concatenate([np.repeat(SAT_COEFF[:, None], k, axis=1), rng.choice(SAT_COEFF, size=(3, k))])
        x = rng.choice(SAT_WORD, size=(2, k, L))
        for c in range(20):
            x[:, :, c] = SAT_WORD[c % 4]
            x[:, :, L - 1 - c] = SAT_WORD[c % 4]
        return coeff.astype(np.uint32), x.astype(np.uint32), apply_rows(coeff, x)
    return cached(("sat", k), make)


@pytest.mark.parametrize("mc", [1, 0], ids=["matrix_cores", "valu"])
@pytest.mark.parametrize("k", [16, 33, 112])
def test_saturated_matrix(torch_dev, forms, k, mc):
    """Plan.matrix of saturated coefficients over saturated inputs: the largest
    sums and accumulator magnitudes a k-input row reaches."""
    from slime_amd import device as D
    torch = torch_dev
    forms(matrix_cores=mc)
    coeff, x, want = saturated_case(k)
    src = to_dev(torch, x)
    dst = torch.zeros(2 * 8 * L, dtype=torch.int32, device="cuda")
    D.Plan.matrix(coeff, list(range(k)))(src, D.layout_of(k, L), dst, D.layout_of(8, L), L, 2)
    assert np.array_equal(to_host(torch, dst).reshape(2, 8, L), want)


# ------------------------------------------------------------------ reconstruct

RECON_VALUES = np.concatenate([ST.TARGET_VALUES, np.array([P, P + 1, P + 2, P + 3, P + 4, 0xFFFFFFFF], dtype=np.uint32)])
RL = RECON_VALUES.size * 60 + 3   # 5523 columns, RL % 4 == 3
RSS = -(-RL // 64) * 64
RECON = {(4, 6): [1, 3], (8, 12): [0, 2, 5, 7], (33, 50): list(range(17))}


def recon_case(need, total):
    """(full, want_rows): [NOBJ][total][RSS] codewords whose middle object's
    DATA rows are the target values themselves (p..p+4 and 2^32-1 included,
    which the oracle encodes as it does any symbol), and the oracle's
    RecoverData rows for the erased shards, [NOBJ][len(erase)][RL]: exactly
    t, or t - p where t >= p."""
    def make():
        erase = RECON[(need, total)]
        have = [i for i in range(total) if i not in erase][:need]
        rng = np.random.default_rng([need, total, 11])
        full = rng.integers(0, 2**32, size=(NOBJ, total, RSS), dtype=np.uint64).astype(np.uint32)
        # rolled by row; the tail columns hold 0..4 in even rows and p..p+4 in odd ones
        tg = np.array(ST.targets(need, values=RECON_VALUES, per=60))
        tg[1::2, -3:] += np.uint32(P)
        full[1, :need, :RL] = tg
        full[:, need:, :RL] = apply_rows(OC.parity_matrix(need, total - need)[need:], full[:, :need, :RL])
        wide = [np.ascontiguousarray(full[:, s, :RL].reshape(-1)) for s in have]
        rc, data = OC.recover_data(wide, have)
        assert rc == 0
        want = np.stack([data[t].reshape(NOBJ, RL) for t in erase], axis=1)
        assert np.array_equal(want[1], canon(tg[erase])), "a rebuilt data row is the canonical target"
        assert (tg[erase] >= P).any()
        return full, want
    return cached(("recon", need, total), make)


@pytest.mark.parametrize("need,total,sched,pipe", [(n, t, s, p) for n, t in [(4, 6), (8, 12)] for s in (1, 0)
                                                   for p in (1, 0)])
def test_reconstruct_target_rows_in_place(torch_dev, forms, need, total, sched, pipe):
    from slime_amd import device as D
    torch = torch_dev
    forms(schedule=sched, pipeline=pipe)
    full, want_rows = recon_case(need, total)
    erase = RECON[(need, total)]
    have = [i for i in range(total) if i not in erase][:need]
    init = full.copy()
    init[:, erase, :RL] = 0xDEADBEEF
    want = full.copy()
    want[:, erase, :RL] = want_rows
    buf = to_dev(torch, init)
    lay = D.layout_of(total, RL, RSS)
    D.Plan.reconstruct(need, total, have, erase).set_outputs(erase)(buf, lay, buf, lay, RL, NOBJ)
    assert np.array_equal(to_host(torch, buf).reshape(NOBJ, total, RSS), want)


@pytest.mark.parametrize("mc", [1, 0], ids=["matrix_cores", "valu"])
def test_reconstruct_target_rows_separate_layout(torch_dev, forms, mc):
    """33/50, 17 data rows rebuilt into a buffer of its own with a dense (odd) shard stride."""
    from slime_amd import device as D
    torch = torch_dev
    forms(matrix_cores=mc)
    need, total = 33, 50
    full, want_rows = recon_case(need, total)
    erase = RECON[(need, total)]
    have = [i for i in range(total) if i not in erase][:need]
    buf = to_dev(torch, full)
    out = torch.full((NOBJ * len(erase) * RL + 5,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    D.Plan.reconstruct(need, total, have, erase)(buf, D.layout_of(total, RL, RSS), out,
                                                 D.layout_of(len(erase), RL), RL, NOBJ, dst_offset=1)
    got = to_host(torch, out)
    assert got[0] == 0x5A5A5A5A and (got[1 + NOBJ * len(erase) * RL:] == 0x5A5A5A5A).all()
    assert np.array_equal(got[1: 1 + NOBJ * len(erase) * RL].reshape(NOBJ, len(erase), RL), want_rows)


# ------------------------------------------------------------------ ragged

def ragged_geometry(k):
    """(T, C): a tile's columns and a unit's tiles (ragged_plan.hpp, geometry_for_k)."""
    return (1024, 3) if k <= 4 else (768, 2) if k <= 12 else (256, 6)


def ragged_case(need, total):
    """Five objects in Batch.packed's layout (64-word aligned shards, sentinel
    between them) with steered columns over a tile edge, a unit edge, the tail
    of an object, a whole seven-column object and the start and both tile and
    unit edges of a long one; (lengths, init, want)."""
    def make():
        coeff, x, tg, mask = ST.encode_case(need, total)
        T, C = ragged_geometry(need)
        lengths = [T + 67, C * T + 131, 2 * T + 3, 7, 2 * C * T + T + 5]
        windows = [[(T - 32, T + 32)], [(C * T - 32, C * T + 32)], [(2 * T - 29, 2 * T + 3)], [(0, 7)],
                   [(0, 64), (C * T - 32, C * T + 32), (2 * C * T + T - 27, 2 * C * T + T + 5)]]
        rng = np.random.default_rng([need, total, 13])
        size = sum(-(-n // 64) * 64 * total for n in lengths)
        init = np.full(size, 0xA5C3F00D, dtype=np.uint32)
        want = None
        off, places, pick = 0, [], 0
        for n, wins in zip(lengths, windows):
            ss = -(-n // 64) * 64
            data = rng.integers(0, 2**32, size=(need, n), dtype=np.uint64).astype(np.uint32)
            for a, b in wins:
                # consecutive window columns take consecutive target values (64 steered columns apart)
                cols = (np.arange(pick, pick + b - a) * 64 + 7) % (L - 3)
                if b == n:  # the object's last columns: the steered tail columns too
                    cols[-3:] = [L - 3, L - 2, L - 1]
                data[:, a:b] = x[:, cols]
                pick += b - a
            for s in range(need):
                init[off + s * ss: off + s * ss + n] = data[s]
            places.append((off, ss, n))
            off += total * ss
        want = init.copy()
        for o, ss, n in places:
            ins = np.stack([init[o + s * ss: o + s * ss + n] for s in range(need)])
            par = OC.apply_matrix(coeff, list(ins))
            for i in range(total - need):
                want[o + (need + i) * ss: o + (need + i) * ss + n] = par[i]
        return lengths, init, want
    return cached(("ragged", need, total), make)


@pytest.mark.parametrize("sched,pipe", [(1, 1), (0, 1), (1, 0), (0, 0)])
@pytest.mark.parametrize("need,total", [(4, 6), (8, 12), (16, 20), (17, 20)])
def test_ragged_batch_steered_edges(torch_dev, forms, need, total, sched, pipe):
    from slime_amd import device as D
    torch = torch_dev
    forms(schedule=sched, pipeline=pipe)
    lengths, init, want = ragged_case(need, total)
    batch, size = D.Batch.packed(lengths, total, need, align=64)
    assert size == init.size
    buf = to_dev(torch, init)
    D.Plan.encode(need, total).set_outputs(list(range(need, total))).execute_batch(buf, buf, batch)
    got = to_host(torch, buf)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"first differing word {bad[0]}, {bad.size} in all"
    batch.close()


# ------------------------------------------------------------------ verify

VERIFY_CODES = [(3, 5), (4, 6), (8, 12), (16, 20), (17, 20), (33, 50)]
GARBAGE = 0x5A5A5A5A5A5A5A5A


def raw_verify(torch, plan, src, src_lay, cmp, cmp_lay, ncols, nobj, src_ptr=None, cmp_ptr=None):
    """slime_rs_plan_verify into result arrays pre-filled with garbage -> host (mism, first)."""
    mism = torch.full((nobj, plan.rows), GARBAGE, dtype=torch.int64, device="cuda")
    first = torch.full((nobj, plan.rows), GARBAGE, dtype=torch.int64, device="cuda")
    N.check(N.lib.slime_rs_plan_verify(plan._h, ctypes.c_void_p(src_ptr or src.data_ptr()), src_lay,
                                       ctypes.c_void_p(cmp_ptr or cmp.data_ptr()), cmp_lay, ncols, nobj,
                                       ctypes.c_void_p(mism.data_ptr()), ctypes.c_void_p(first.data_ptr()), None))
    torch.cuda.synchronize()
    return mism.cpu().numpy(), first.cpu().numpy()


def planted_columns(tg_row):
    """Ten steered columns of a row whose residues are 0..4, two of each."""
    cols = sorted(int(c) for t in range(5) for c in np.flatnonzero(tg_row[:L - 3] == t)[[3, 40]])
    assert len(cols) == 10
    return cols


@pytest.mark.parametrize("pipe", [1, 0], ids=["pipelined", "offsets64"])
@pytest.mark.parametrize("need,total", VERIFY_CODES)
def test_verify_steered_codewords(torch_dev, forms, need, total, pipe):
    """Clean steered codewords (the oracle's) verify with zero mismatches in both
    vector forms and, two bytes off a word boundary, in the column form; p + t
    stored where the parity is t in 0..4, at ten steered columns of one row of
    the middle object, counts exactly those ten and reports the first."""
    from slime_amd import device as D
    torch = torch_dev
    forms(pipeline=pipe)
    _, want = symbol_case(need, total)
    coeff, x, tg, mask = ST.encode_case(need, total)
    rows = total - need
    plan = D.Plan.encode(need, total).set_outputs(list(range(need, total)))
    lay = D.layout_of(total, L, SS)
    row = rows - 1
    cols = planted_columns(tg[row])
    assert mask[row][cols].all()
    dirty = want.copy()
    dirty[1, need + row, cols] += np.uint32(P)  # p + t, t in 0..4: no wrap
    assert (dirty[1, need + row, cols] >= P).all()
    em = np.zeros((NOBJ, rows), dtype=np.int64)
    ef = np.full((NOBJ, rows), -1, dtype=np.int64)
    for stored, planted in ((want, False), (dirty, True)):
        if planted:
            em[1, row], ef[1, row] = 10, cols[0]
        buf = to_dev(torch, stored)
        m, f = raw_verify(torch, plan, buf, lay, buf, lay, L, NOBJ)
        assert np.array_equal(m, em) and np.array_equal(f, ef), ("vector form", planted)
        byt = shifted(torch, stored, 2)
        m, f = raw_verify(torch, plan, byt, lay, byt, lay, L, NOBJ, byt.data_ptr() + 2, byt.data_ptr() + 2)
        assert np.array_equal(m, em) and np.array_equal(f, ef), ("column form", planted)


# ------------------------------------------------------------------ byte encode / decode / verify_objects

def in_band(a):
    """Words MapToGF's decision turns on: >= p, or in [p ^ 2^31, 2^31)."""
    return (a >= P) | ((a >= 0x7FFFFFFB) & (a < 0x80000000))


def byte_case(need, total, prefix=None):
    """Three objects of about 1 MiB (S = 4 need Lb, Lb % 4 == 3) and what the
    oracle makes of them: (S, Lb, objs, mappings, chunks).  Object 0 maps with
    0; object 1 has 0xFFFFFFFD as its last whole word, so maps with 1<<31;
    object 2 is random bytes.  In objects 0 and 1 the parity SYMBOLS (under the
    object's final mapping) of the first 2752 and the last 2755 columns are
    the steered targets -- except object 1's very last column, which holds the
    planted word.  prefix=n: the partial sums over the first n data chunks are
    the targets instead (the wide kernels' running residues)."""
    def make():
        coeff, x, tg, mask = ST.encode_case(need, total, prefix, canonical=True)
        x = np.array(x)
        Lb = ((1 << 18) // need) | 3
        S = 4 * need * Lb
        assert Lb % 4 == 3 and Lb >= L
        rng = np.random.default_rng([need, total, 17])
        # A steered data symbol in a band MapToGF reacts to would change the object's
        # mapping: re-draw that column's random part (about need * 2^-30 a column).
        for attempt in range(1, 5):
            bad = np.flatnonzero(in_band(x).any(axis=0) | in_band(x ^ np.uint32(HIGH)).any(axis=0))
            if not bad.size:
                break
            x2 = ST.steer(coeff, tg, np.random.default_rng([need, total, 17, attempt]), prefix=prefix, canonical=True)
            x[:, bad] = x2[:, bad]
        assert not in_band(x).any() and not in_band(x ^ np.uint32(HIGH)).any()
        head, cols = 2752, np.r_[0:2752, Lb - (L - 2752):Lb]
        objs, mappings, chunks = [], [], []
        for o, m in enumerate((0, HIGH, None)):
            if m is None:
                objs.append(rng.integers(0, 256, size=S, dtype=np.uint8).tobytes())
            else:
                sym = rng.integers(0, P, size=(need, Lb), dtype=np.uint64).astype(np.uint32)
                sym[in_band(sym) | in_band(sym ^ np.uint32(HIGH))] = 0x01020304
                sym[:, :head] = x[:, :head]
                sym[:, Lb - (L - head):] = x[:, head:]
                words = sym ^ np.uint32(m)
                if m:
                    words[need - 1, Lb - 1] = 0xFFFFFFFD
                assert not in_band(words.reshape(-1)[:-1]).any()
                objs.append(words.astype(">u4").tobytes())
            rc, mo, w = OC.map_to_gf(objs[-1])
            assert rc == 0 and (m is None or mo == m)
            parts = [np.ascontiguousarray(p) for p in OP.split_vector(w, need)]
            parity = OC.apply_matrix(coeff, parts)
            if m is not None:  # the steering held under the object's final mapping
                keep = cols[:-1] if m else cols
                tcols = np.r_[0:L][: keep.size]
                steered = parity if prefix is None else OC.apply_matrix(coeff[:, :prefix], parts[:prefix])
                for i in range(total - need):
                    sel = mask[i][tcols]
                    assert np.array_equal(steered[i][keep][sel], tg[i][tcols][sel])
            mappings.append(mo)
            chunks.append(b"".join(OC.map_from_gf(mo, p) for p in parts + parity))
        return S, Lb, objs, mappings, chunks
    return cached(("bytes", need, total, prefix), make)


def byte_params():
    out = []
    for need, total in ST.BYTE_CODES:
        for pipe, sched in ((1, 1), (1, 0), (0, 1)):
            for bits in ((1, 2) if need <= 10 else (0,)):
                for mc in ((1, 0) if need > 32 else (1,)):
                    out.append((need, total, pipe, sched, bits, mc))
    return out


def run_byte_objects(torch_dev, forms, need, total, pipe, sched, bits, mc, prefix=None):
    """Device writeChunks, scrub and repair of 1 MiB objects whose parity
    symbols are the target residues (byte_case), every chunk byte against the
    oracle's framing, in the three byte-kernel forms (queue, pipelined with
    static shares, non-pipelined), with the second pass correcting from top bits
    (switch_bits 1) and re-encoding (2) for need <= 10, and 33/50 on the matrix
    cores and on the wide VALU kernel.

    Object 1's word >= p is its LAST whole word, so every unit encoded before
    the wave that meets it assumed mapping 0 and is redone by the second pass.
    Which units were redone is decided by the schedule (the order in which
    waves took their work), not by this test; the comparison is exact either
    way, and in the correcting mode the FINAL parity 0..4 is what reaches the
    table add's `s2 >= p` band.

    Then verify_objects over the encoded slots finds nothing, and a repair of
    two data chunks and a parity chunk (one data chunk where the code has two
    parity chunks) restores every byte: the rebuilt parity is the steered one."""
    from slime_amd import device as D
    torch = torch_dev
    forms(pipeline=pipe, schedule=sched, switch_bits=bits, matrix_cores=mc)
    S, Lb, objs, mappings, chunks = byte_case(need, total, prefix)
    chunk, slot = 4 * Lb, 4 * Lb * total
    stride = slot + 64
    host = np.full(3 * stride, 0xA5, dtype=np.uint8)
    want = host.copy()
    for o in range(3):
        host[o * stride: o * stride + S] = np.frombuffer(objs[o], dtype=np.uint8)
        host[o * stride + S: o * stride + slot] = 0
        want[o * stride: o * stride + slot] = np.frombuffer(chunks[o], dtype=np.uint8)
    slots = torch.from_numpy(host).cuda()
    plan = D.Plan.encode(need, total)
    mapping = torch.full((3,), 0x55, dtype=torch.int32, device="cuda")
    status = torch.full((3,), 0x55, dtype=torch.int32, device="cuda")
    D.encode_objects(plan, slots, stride, S, 3, mapping, status)
    torch.cuda.synchronize()
    assert status.cpu().numpy().tolist() == [0, 0, 0]
    assert mapping.cpu().numpy().view(np.uint32).tolist() == mappings
    got = slots.cpu().numpy()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"first differing byte {bad[0]} (object {bad[0] // stride}, chunk " \
                          f"{bad[0] % stride // chunk}, column {bad[0] % stride % chunk // 4}), {bad.size} in all"
    # scrub: the parity chunks are what the plan computes
    vplan = D.Plan.encode(need, total).set_outputs(list(range(need, total)))
    m, f = D.verify_objects(vplan, slots, stride, Lb, 3, mapping)
    torch.cuda.synchronize()
    assert not m.cpu().numpy().any() and (f.cpu().numpy() == -1).all()
    # repair
    erase = [0, 2, need] if total - need >= 3 else [0, need]
    have = [i for i in range(total) if i not in erase][:need]
    rec = D.Plan.reconstruct(need, total, have, erase).set_outputs(erase)
    v = slots.view(3, stride)[:, :slot].view(3, total, chunk)
    v[:, erase, :] = 0x5A
    D.decode_objects(rec, slots, stride, Lb, 3, mapping)
    torch.cuda.synchronize()
    assert np.array_equal(slots.cpu().numpy(), want), erase


@pytest.mark.parametrize("need,total,pipe,sched,bits,mc", byte_params())
def test_byte_objects_steered_parity(torch_dev, forms, need, total, pipe, sched, bits, mc):
    run_byte_objects(torch_dev, forms, need, total, pipe, sched, bits, mc)


@pytest.mark.parametrize("pipe,sched", [(1, 1), (1, 0), (0, 1)], ids=["queue", "pipelined", "fallback"])
@pytest.mark.parametrize("need,total,prefix", ST.BYTE_PREFIXES)
def test_byte_objects_steered_prefix_sums(torch_dev, forms, need, total, prefix, pipe, sched):
    """The wide VALU byte kernels (need > 16, matrix cores off) keep a running
    residue a row and fold it after every chunk of 16 or 32 data chunks: the
    partial sums over the first 16 and 32 are steered."""
    run_byte_objects(torch_dev, forms, need, total, pipe, sched, 0, 0, prefix)


@pytest.mark.parametrize("need,total", [(4, 6), (8, 12), (33, 50)])
def test_verify_objects_counts_noncanonical_stored_parity(torch_dev, need, total):
    """The oracle's chunks, with BE((p + t) ^ mapping) stored at ten steered
    columns of the last parity chunk of objects 0 (mapping 0) and 1 (1<<31)
    where the parity symbol is t in 0..4: the computed value is canonical, so
    each is one mismatch -- ten a chunk, first at the lowest column."""
    from slime_amd import device as D
    torch = torch_dev
    S, Lb, objs, mappings, chunks = byte_case(need, total)
    coeff, x, tg, mask = ST.encode_case(need, total, canonical=True)
    chunk, slot = 4 * Lb, 4 * Lb * total
    host = np.frombuffer(b"".join(chunks), dtype=np.uint8).copy()
    row = total - need - 1
    case_cols = planted_columns(tg[row])
    assert mask[row][case_cols].all()
    cols = sorted(c if c < 2752 else Lb - L + c for c in case_cols)  # where byte_case put steered column c
    em = np.zeros((3, total - need), dtype=np.int64)
    ef = np.full((3, total - need), -1, dtype=np.int64)
    for o in (0, 1):
        w = host[o * slot + (total - 1) * chunk: o * slot + total * chunk].view(">u4")
        t = (w[cols].astype(np.uint32)) ^ np.uint32(mappings[o])
        assert np.array_equal(np.sort(t), np.repeat(np.arange(5, dtype=np.uint32), 2))
        w[cols] = (t + np.uint32(P)) ^ np.uint32(mappings[o])
        em[o, row], ef[o, row] = 10, cols[0]
    slots = torch.from_numpy(host).cuda()
    mapping = torch.from_numpy(np.array(mappings, dtype=np.uint32).view(np.int32)).cuda()
    plan = D.Plan.encode(need, total).set_outputs(list(range(need, total)))
    m, f = D.verify_objects(plan, slots, slot, Lb, 3, mapping)
    torch.cuda.synchronize()
    assert np.array_equal(m.cpu().numpy(), em) and np.array_equal(f.cpu().numpy(), ef)


# ------------------------------------------------------------------ mapping thresholds

# (name, the word at the varied position, a second word at a fixed position, the mapping MapToGF picks)
WORD_CASES = [("p-1", 0xFFFFFFFA, None, 0),
              ("p", 0xFFFFFFFB, None, HIGH),
              ("p and p^2^31-1", 0x7FFFFFFA, 0xFFFFFFFB, HIGH),
              ("p^2^31-1 and p", 0xFFFFFFFB, 0x7FFFFFFA, HIGH),
              ("p and p^2^31", 0x7FFFFFFB, 0xFFFFFFFB, None),   # neither 0 nor 1<<31 fits: the random fallback
              ("p^2^31 and p", 0xFFFFFFFB, 0x7FFFFFFB, None),
              ("2^31", 0x80000000, None, 0),
              ("2^31-1", 0x7FFFFFFF, None, 0)]
FIXED_WORD = 777


def threshold_positions(need, Lt, S):
    """Word indices (word w is column w % Lt of data chunk w // Lt): the first
    word; the last whole word (in the edge tile of the last, partly filled
    chunk) and its neighbours; each of a lane's four columns; lane 63 of the
    first wave; the middle of the first and of the last chunk; the last column
    of a full chunk."""
    last = S // 4 - 1
    mid = need // 2
    pos = [0, last, last - 1, last - 4,
           mid * Lt + 20, mid * Lt + 21, mid * Lt + 22, mid * Lt + 23,
           4 * 63 + 1, (min(1, need - 1)) * Lt + 4 * 63 + 2,
           Lt // 2, (need - 1) * Lt + Lt // 3, (need - 1) * Lt - 1]
    assert len(set(pos)) == len(pos) and FIXED_WORD not in pos and max(pos) == last
    return pos


def scrubbed(rng, S):
    """Random object bytes with no word the mapping decision reacts to, nor a threshold's neighbour."""
    b = rng.integers(0, 256, size=S, dtype=np.uint8)
    w = b[: S // 4 * 4].view(">u4")
    w[(w >= 0xFFFFFFF0) | ((w >= 0x7FFFFFF0) & (w <= 0x80000000))] = 0x01020304
    return b


def plant(b, at, word):
    b[4 * at: 4 * at + 4] = np.frombuffer(int(word).to_bytes(4, "big"), dtype=np.uint8)


def oracle_chunks(obj, need, total, cands=()):
    """writeChunks' framing (multi_store.go:526-554) via the oracle: (mapping, the slot's bytes)."""
    rc, m, words = OC.map_to_gf(obj, list(cands))
    assert rc == 0
    parts = [np.ascontiguousarray(p) for p in OP.split_vector(words, need)]
    parity = OC.apply_matrix(OC.parity_matrix(need, total - need)[need:], parts)
    return m, b"".join(OC.map_from_gf(m, p) for p in parts + parity)


@pytest.mark.parametrize("name,word,second,mapped", WORD_CASES, ids=[c[0] for c in WORD_CASES])
@pytest.mark.parametrize("need,total", [(4, 6), (8, 12), (33, 40)])
def test_mapping_thresholds_in_encode_objects(torch_dev, need, total, name, word, second, mapped):
    """The device byte encode's MapToGF decision at its exact thresholds
    (map.go:47-66): 4/6 and 8/12 on the VALU kernels, 33/40 on the matrix
    cores.  One launch a position: the planted object and an unplanted control
    that must keep mapping 0; objects of 256 KiB less 149 bytes, so the last
    chunk is partly filled and the object ends in a partial word.  Mapping
    word, status and every chunk byte against OC.map_to_gf plus the framing;
    fallbacks are resolved on the device and checked with the oracle given the
    mapping the device drew."""
    from slime_amd import device as D
    torch = torch_dev
    S = (1 << 18) - 4 * 37 - 1
    Lt, _, slot = D.slot_geometry(S, need, total)
    plan = D.Plan.encode(need, total)
    rng = np.random.default_rng([need, total, 19])
    base = scrubbed(rng, S)
    control = scrubbed(rng, S)
    cm, cwant = oracle_chunks(control.tobytes(), need, total)
    assert cm == 0
    stride = slot + 16
    for at in threshold_positions(need, Lt, S):
        obj = base.copy()
        plant(obj, at, word)
        if second is not None:
            plant(obj, FIXED_WORD, second)
        host = np.full(2 * stride, 0xA5, dtype=np.uint8)
        for o, b in enumerate((obj, control)):
            host[o * stride: o * stride + S] = b
            host[o * stride + S: o * stride + slot] = 0
        slots = torch.from_numpy(host).cuda()
        mapping = torch.full((2,), 0x55, dtype=torch.int32, device="cuda")
        status = torch.full((2,), 0x55, dtype=torch.int32, device="cuda")
        D.encode_objects(plan, slots, stride, S, 2, mapping, status)
        torch.cuda.synchronize()
        st = status.cpu().numpy().tolist()
        assert st == [1 if mapped is None else 0, 0], (at, st)
        if mapped is None:
            assert D.resolve_fallbacks(plan, slots, stride, S, 2, mapping, status) == 1
            torch.cuda.synchronize()
            assert status.cpu().numpy().tolist() == [0, 0]
        ms = mapping.cpu().numpy().view(np.uint32).tolist()
        m, want = oracle_chunks(obj.tobytes(), need, total, [] if mapped is not None else [ms[0]])
        assert ms == [m, 0] and (mapped is None or m == mapped), (at, ms)
        if mapped is None:
            assert m not in (0, HIGH)
        got = slots.cpu().numpy()
        assert got[:slot].tobytes() == want, at
        assert got[stride: stride + slot].tobytes() == cwant, at
        assert (got[slot: stride] == 0xA5).all() and (got[stride + slot:] == 0xA5).all(), "wrote past the chunks"


@pytest.mark.parametrize("name,word,second,mapped", WORD_CASES, ids=[c[0] for c in WORD_CASES])
def test_mapping_thresholds_in_the_device_codec(torch_dev, name, word, second, mapped):
    """gf.MapToGF with the codec kernels on the GPU (slime_gf_codec_placement 1)
    at the same thresholds and positions: mapping and every symbol."""
    S = (1 << 18) - 4 * 37 - 1
    base = scrubbed(np.random.default_rng(23), S)
    prev = gf.codec_placement(1)
    try:
        for at in threshold_positions(4, -(-((S + 3) // 4) // 4), S):
            obj = base.copy()
            plant(obj, at, word)
            if second is not None:
                plant(obj, FIXED_WORD, second)
            gf.Seed(at)
            n, v = gf.MapToGF(obj.tobytes())
            rc, n2, v2 = OC.map_to_gf(obj.tobytes(), [] if mapped is not None else [n])
            assert rc == 0 and n == n2 and (mapped is None or n == mapped), (at, n)
            if mapped is None:
                assert n not in (0, HIGH)
            assert np.array_equal(v, v2) and int(v.max()) < P, at
    finally:
        gf.codec_placement(prev)
