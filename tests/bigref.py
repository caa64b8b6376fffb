"""An exact reference that scales to 2^30-column shards: plain torch int64
arithmetic on whatever device the tensors live on, independent of every kernel
under test (tests/test_gpu_large_geometry.py).  tests/test_bigref.py pins it to
the C oracle on the CPU; the GPU tests pin it to the oracle again on windows of
every result.

out[i] = sum_j coeff[i][j] * shards[j] mod p, p = 2^32 - 5, for ANY uint32
coefficient and input word (non-canonical ones included).  With c = coeff mod p
split into c1 = c >> 16 and c0 = c & 0xFFFF, and x the input word as an int64
in [0, 2^32):

    t   = (x * c1) % p                  x*c1 < 2^48
    t   = (t * 65536 + x * c0) % p      < 2^48 + 2^48 = 2^49
    acc = (acc + t) % p                 < 2^33

so every intermediate stays below 2^49 and int64 never wraps.
"""
from typing import Optional, Sequence

import numpy as np
import torch

P = 4294967291
CHUNK = 1 << 24


def u32(t: torch.Tensor) -> torch.Tensor:
    """int32 bits -> the uint32 value as an int64."""
    return t.to(torch.int64) & 0xFFFFFFFF


def i32(t: torch.Tensor) -> torch.Tensor:
    """An int64 in [0, 2^32) -> the int32 tensor with the same low 32 bits."""
    return torch.where(t >= 1 << 31, t - (1 << 32), t).to(torch.int32)


def apply_rows(coeff, shards: Sequence[torch.Tensor], chunk: int = CHUNK,
               out: Optional[Sequence[torch.Tensor]] = None) -> list:
    """coeff: rows x k integers below 2^32; shards: k 1-D int32 views of one length L (they may
    overlap each other).  Returns rows int32 tensors of L words, written into `out` if given
    (views that overlap no shard).  Worked `chunk` columns at a time: the temporaries are a few
    int64 tensors of `chunk` elements, whatever L is."""
    c = np.asarray(coeff, dtype=np.uint64).reshape(-1, len(shards)) % P
    rows, k = c.shape
    L = shards[0].numel()
    assert all(s.dim() == 1 and s.dtype == torch.int32 and s.numel() == L for s in shards)
    dev = shards[0].device
    if out is None:
        out = [torch.empty(L, dtype=torch.int32, device=dev) for _ in range(rows)]
    assert len(out) == rows and all(o.dtype == torch.int32 and o.numel() == L for o in out)
    for c0 in range(0, L, chunk):
        c1 = min(L, c0 + chunk)
        acc = [torch.zeros(c1 - c0, dtype=torch.int64, device=dev) for _ in range(rows)]
        for j in range(k):
            x = u32(shards[j][c0:c1])
            for i in range(rows):
                hi, lo = int(c[i, j]) >> 16, int(c[i, j]) & 0xFFFF
                t = (x * hi).remainder_(P)
                t = t.mul_(65536).add_(x * lo).remainder_(P)
                acc[i] = acc[i].add_(t).remainder_(P)
        for i in range(rows):
            out[i][c0:c1] = i32(acc[i])
    return list(out)


def be_words(b: torch.Tensor, mapping: int = 0, chunk: int = CHUNK // 4) -> torch.Tensor:
    """MapToGFWith(mapping): the big-endian words of a uint8 tensor (a last partial word padded
    with zero bytes) XOR mapping, as int32 bits."""
    assert b.dim() == 1 and b.dtype == torch.uint8
    n = (b.numel() + 3) // 4
    out = torch.empty(n, dtype=torch.int32, device=b.device)
    whole = b.numel() // 4
    for w0 in range(0, whole, chunk):
        w1 = min(whole, w0 + chunk)
        q = b[4 * w0: 4 * w1].view(-1, 4).to(torch.int64)
        out[w0:w1] = i32(((q[:, 0] << 24) | (q[:, 1] << 16) | (q[:, 2] << 8) | q[:, 3]) ^ mapping)
    if n > whole:
        q = torch.zeros(4, dtype=torch.int64, device=b.device)
        q[: b.numel() - 4 * whole] = b[4 * whole:].to(torch.int64)
        out[whole] = i32(((q[0] << 24) | (q[1] << 16) | (q[2] << 8) | q[3]) ^ mapping)
    return out


def be_bytes(w: torch.Tensor, mapping: int = 0, chunk: int = CHUNK // 4,
             out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """MapFromGF(mapping): the inverse of be_words -- 4 bytes per int32 word, big-endian, of
    word XOR mapping; written into `out` (uint8, 4 * len) if given."""
    assert w.dim() == 1 and w.dtype == torch.int32
    if out is None:
        out = torch.empty(4 * w.numel(), dtype=torch.uint8, device=w.device)
    assert out.dtype == torch.uint8 and out.numel() == 4 * w.numel()
    for w0 in range(0, w.numel(), chunk):
        w1 = min(w.numel(), w0 + chunk)
        x = u32(w[w0:w1]) ^ mapping
        q = torch.stack(((x >> 24) & 0xFF, (x >> 16) & 0xFF, (x >> 8) & 0xFF, x & 0xFF), dim=1)
        out[4 * w0: 4 * w1] = q.to(torch.uint8).view(-1)
    return out


def first_diff(a: torch.Tensor, b: torch.Tensor, chunk: int = 1 << 26) -> int:
    """The lowest index at which two 1-D tensors of one length and dtype differ, -1 if none;
    compared `chunk` elements at a time where they live."""
    assert a.shape == b.shape and a.dim() == 1 and a.dtype == b.dtype
    for c0 in range(0, a.numel(), chunk):
        ne = a[c0: c0 + chunk] != b[c0: c0 + chunk]
        if bool(ne.any()):
            return c0 + int(ne.to(torch.uint8).argmax())
    return -1
