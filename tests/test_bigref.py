"""tests/bigref.py (the torch int64 reference of the 2-4 GiB shard tests) against the C
oracle, on CPU tensors: the same code the GPU tests run on the device."""
import numpy as np
import pytest
import torch

import bigref as BR
from oracle import oracle_c as OC

P = BR.P
EDGE_COEFF = np.array([P - 1, 0xFFFFFFFF, 0, 1, P, P + 1, 0x80000000, 0x7FFFFFFF, 0x00010000, 0x0000FFFF],
                      dtype=np.uint32)
EDGE_IN = np.array([P, P + 4, 0xFFFFFFFF, 0x80000000, 0, 1, 2, P - 1, P + 1, 0x7FFFFFFF], dtype=np.uint32)


def _case(k, rows, L, seed):
    rng = np.random.default_rng(seed)
    coeff = rng.integers(0, 1 << 32, size=(rows, k), dtype=np.uint64).astype(np.uint32)
    coeff.reshape(-1)[: min(coeff.size, EDGE_COEFF.size)] = EDGE_COEFF[: coeff.size]
    ins = rng.integers(0, 1 << 32, size=(k, L), dtype=np.uint64).astype(np.uint32)
    for j in range(k):  # every edge input meets every coefficient of column j
        ins[j, : EDGE_IN.size] = EDGE_IN
        ins[j, L - EDGE_IN.size:] = np.roll(EDGE_IN, j)
    return coeff, ins


def _t(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(a.view(np.int32))


@pytest.mark.parametrize("k", [1, 2, 17, 33])
def test_apply_rows_equals_the_oracle(k):
    """Random and edge coefficients (p-1, 2^32-1, 0, p, ...) over random and edge inputs
    (p, p+4, 2^32-1, 2^31, ...), bit for bit, with the default chunk (one piece) and a chunk
    that does not divide L."""
    rows, L = (3 if k < 33 else 2), 4099
    coeff, ins = _case(k, rows, L, 100 + k)
    want = OC.apply_matrix(coeff, list(ins))
    shards = [_t(ins[j]) for j in range(k)]
    for chunk in (BR.CHUNK, 1000):
        got = BR.apply_rows(coeff, shards, chunk)
        for i in range(rows):
            assert np.array_equal(got[i].numpy().view(np.uint32), want[i]), (k, chunk, i)


def test_apply_rows_every_edge_pair():
    """Every edge coefficient against every edge input, one column each."""
    c, x = np.meshgrid(EDGE_COEFF, EDGE_IN, indexing="ij")
    for ci in range(EDGE_COEFF.size):
        want = OC.apply_matrix(c[ci: ci + 1, :1], [x[ci]])
        got = BR.apply_rows(c[ci: ci + 1, :1], [_t(np.ascontiguousarray(x[ci]))])
        assert np.array_equal(got[0].numpy().view(np.uint32), want[0]), ci


def test_apply_rows_overlapping_inputs_and_out_views():
    """Input views that overlap each other (a shard stride below L) and results written into
    views of a caller's buffer: what the large tests do with one 2 GiB source."""
    k, rows, L, ss = 5, 2, 1003, 64
    coeff, _ = _case(k, rows, L, 7)
    rng = np.random.default_rng(8)
    src = rng.integers(0, 1 << 32, size=(k - 1) * ss + L, dtype=np.uint64).astype(np.uint32)
    ins = [src[j * ss: j * ss + L] for j in range(k)]
    want = OC.apply_matrix(coeff, ins)
    dst = torch.full((rows * 1100,), -1, dtype=torch.int32)
    outs = [dst[i * 1100: i * 1100 + L] for i in range(rows)]
    BR.apply_rows(coeff, [_t(src)[j * ss: j * ss + L] for j in range(k)], 300, out=outs)
    for i in range(rows):
        assert np.array_equal(dst[i * 1100: i * 1100 + L].numpy().view(np.uint32), want[i])
        assert bool((dst[i * 1100 + L: (i + 1) * 1100] == -1).all())  # nothing written past L


@pytest.mark.parametrize("n", [0, 1, 3, 4, 4096, 4099, 10001])
def test_be_words_and_bytes_equal_the_oracle(n):
    rng = np.random.default_rng(n)
    raw = rng.integers(0, 256, size=n, dtype=np.uint8)
    b = torch.from_numpy(raw)
    for mapping in (0, 1 << 31):
        want = OC.map_to_gf_with(raw.tobytes(), mapping)
        got = BR.be_words(b, mapping, chunk=1000)
        assert np.array_equal(got.numpy().view(np.uint32), want), (n, mapping)
        back = BR.be_bytes(got, mapping, chunk=999)
        assert back.numpy().tobytes() == OC.map_from_gf(mapping, want), (n, mapping)
        assert back.numpy()[:n].tobytes() == raw.tobytes()


def test_be_words_equals_map_to_gf_for_both_fixed_mappings():
    """OC.map_to_gf (MapToGF itself) picks 0 for canonical words and 1<<31 once a word >= p
    appears and no word lies in [p ^ 2^31, 2^31): be_words(., mapping) gives its words."""
    rng = np.random.default_rng(5)
    w = rng.integers(0, 1 << 31, size=5000, dtype=np.uint64).astype(np.uint32)
    w[(w >= (P ^ (1 << 31)))] = 0x12345678  # no word in the 1<<31 band
    w[17] = P - 1
    raw0 = w.astype(">u4").tobytes()
    w[4999] = 0xFFFFFFFD
    raw1 = w.astype(">u4").tobytes()
    for raw, mapping in ((raw0, 0), (raw1, 1 << 31)):
        rc, m, want = OC.map_to_gf(raw)
        assert rc == 0 and m == mapping
        got = BR.be_words(torch.frombuffer(bytearray(raw), dtype=torch.uint8), m)
        assert np.array_equal(got.numpy().view(np.uint32), want)
        assert BR.be_bytes(got, m).numpy().tobytes() == OC.map_from_gf(m, want) == raw


def test_first_diff():
    a = torch.arange(1000, dtype=torch.int32)
    assert BR.first_diff(a, a.clone(), chunk=64) == -1
    for at in (0, 63, 64, 65, 999):
        b = a.clone()
        b[at] ^= 1 << 31
        b[999] ^= 1
        assert BR.first_diff(a, b, chunk=64) == at
    assert BR.first_diff(a[:0], a[:0]) == -1
