"""Host-side checks of ragged batches (no GPU): the work tables' CPU test
program, the C calls' refusals (null arguments, bad k, oversized shards), and
the Python wrappers' extent, dtype and device refusals before any C call."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from slime_amd import _native as N
from slime_amd import device as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "ragged_plan_test")


def test_ragged_plan_tables():
    """slime_amd/csrc/ragged_plan.hpp for every tile geometry the library uses:
    every (object, tile) in exactly one unit of at most C tiles inside one
    object, objects under 4 columns without units, every column past a last
    whole vector listed once, descriptors 64 bytes apart, the ticket dealing a
    bijection onto the list, L = 2^30 and 2^32 units refused."""
    subprocess.run(["make", "-C", ROOT, "tests/cpp/ragged_plan_test"], check=True, capture_output=True)
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    for name in ("TestHandMade", "TestOrder", "TestRandom", "TestRefusals"):
        assert f"ok   {name}" in r.stdout


def _detail():
    return N.lib.slime_rs_last_error().decode()


def _spans(rows):
    return (N.Span * len(rows))(*[N.Span(*r) for r in rows])


def test_batch_create_refuses_bad_arguments():
    h = ctypes.c_void_p()
    one = _spans([(0, 8, 0, 8, 8)])
    assert N.lib.slime_rs_batch_create(0, 4, one, 1, None) == N.ERR_INVALID_ARG
    assert "batch_create" in _detail()
    assert N.lib.slime_rs_batch_create(0, 4, None, 1, ctypes.byref(h)) == N.ERR_INVALID_ARG
    assert "batch_create" in _detail() and "spans" in _detail()
    for k in (0, -3):
        assert N.lib.slime_rs_batch_create(0, k, one, 1, ctypes.byref(h)) == N.ERR_INVALID_ARG
        assert "batch_create" in _detail() and "k" in _detail()
    big = _spans([(0, 8, 0, 8, 8), (0, 1 << 30, 0, 1 << 30, 1 << 30)])
    assert N.lib.slime_rs_batch_create(0, 4, big, 2, ctypes.byref(h)) == N.ERR_INVALID_ARG
    assert "batch_create" in _detail() and "span 1" in _detail() and "2^30" in _detail()
    assert not h.value


@pytest.mark.skipif(N.device_count() > 0, reason="a HIP device is visible: batch_create succeeds here")
def test_batch_create_without_a_device_is_no_device_after_validation():
    h = ctypes.c_void_p()
    one = _spans([(0, 8, 0, 8, 8)])
    assert N.lib.slime_rs_batch_create(0, 4, one, 1, ctypes.byref(h)) == N.ERR_NO_DEVICE
    assert N.lib.slime_rs_batch_create(0, 4, None, 0, ctypes.byref(h)) == N.ERR_NO_DEVICE  # an empty batch too
    assert not h.value
    # arguments are validated first
    bad = _spans([(0, 8, 0, 8, 1 << 30)])
    assert N.lib.slime_rs_batch_create(0, 4, bad, 1, ctypes.byref(h)) == N.ERR_INVALID_ARG


def test_batch_calls_refuse_null_handles():
    n = ctypes.c_uint64()
    assert N.lib.slime_rs_batch_info(None, ctypes.byref(n), None, None) == N.ERR_INVALID_ARG
    assert "batch_info" in _detail()
    assert N.lib.slime_rs_batch_destroy(None) == N.ERR_INVALID_ARG
    assert "batch_destroy" in _detail()
    assert N.lib.slime_rs_plan_execute_batch(None, None, None, None, None) == N.ERR_INVALID_ARG
    assert "plan_execute_batch" in _detail() and "plan" in _detail()


def test_ragged_signatures_match_the_header():
    """Arity of the four calls against include/slime_rs.h, and the span's five 64-bit fields."""
    text = open(os.path.join(ROOT, "include", "slime_rs.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    sig = {name: args for name, _, args in N.SIGNATURES}
    for name in ("slime_rs_batch_create", "slime_rs_batch_info", "slime_rs_batch_destroy",
                 "slime_rs_plan_execute_batch"):
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text)
        assert m, name
        assert len(sig[name]) == len(m.group(1).split(",")), name
    assert len(sig["slime_rs_batch_create"]) == 5 and len(sig["slime_rs_plan_execute_batch"]) == 5
    assert ctypes.sizeof(N.Span) == 40 and [f for f, _ in N.Span._fields_] == [
        "src_off", "src_shard_stride", "dst_off", "dst_shard_stride", "L"]
    body = re.search(r"typedef struct slime_rs_span \{(.*?)\} slime_rs_span_t;", text, flags=re.S).group(1)
    assert re.findall(r"uint64_t\s+(\w+);", body) == [f for f, _ in N.Span._fields_]


class _NoCalls:
    """Stands in for the native library: any C call fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"C call {name} reached")


def _batch(rows, k, device=0):
    """A Batch with no native handle over the given spans."""
    b = D.Batch.__new__(D.Batch)
    b._h, b.k, b.device, b._extents = None, k, device, {}
    b.spans = np.asarray(rows, dtype=np.uint64).reshape(-1, 5)
    return b


@pytest.fixture
def plan(monkeypatch):
    """An 8/12 encode-shaped plan with outputs 8..11 and no native handle, over
    CPU tensors that pass for device 0; the native library is unreachable."""
    monkeypatch.setattr(D, "lib", _NoCalls())
    monkeypatch.setattr(D, "_dev_index", lambda t: 0)
    p = D.Plan.__new__(D.Plan)
    p._h, p.device, p.in_max, p.out_max, p.rows, p.k = None, 0, 7, 11, 4, 8
    return p


def test_execute_batch_refuses_an_extent_past_the_tensor(plan):
    # two objects of 100 and 7 columns, 12 shards each, packed
    rows = [(0, 100, 0, 100, 100), (1200, 7, 1200, 7, 7)]
    total = 1200 + 12 * 7
    buf = torch.zeros(total, dtype=torch.int32)
    with pytest.raises(ValueError, match="addresses element"):
        plan.execute_batch(buf, buf[:-1].contiguous(), _batch(rows, 8))  # one element short of the last parity shard
    # the inputs end at shard 7 of the last object: a tensor that ends there passes for src, not for dst
    src_only = torch.zeros(1200 + 8 * 7, dtype=torch.int32)
    with pytest.raises(ValueError, match="span 1 addresses element"):
        plan.execute_batch(src_only, src_only, _batch(rows, 8))  # dst reaches shard 11
    with pytest.raises(ValueError, match="addresses element"):
        plan.execute_batch(src_only, buf, _batch(rows, 8), src_offset=1)
    with pytest.raises(ValueError, match="addresses element"):
        plan.execute_batch(buf, buf, _batch(rows, 8), dst_offset=1)
    with pytest.raises(ValueError, match="addresses element"):
        plan.execute_batch(buf, buf, _batch(rows, 8), src_offset=-1)
    # the furthest span need not be the last one
    far = [(5000, 100, 0, 100, 100), (0, 7, 1200, 7, 7)]
    with pytest.raises(ValueError, match="span 0 addresses element 5800"):
        plan.execute_batch(buf, buf, _batch(far, 8))
    # an object of no columns addresses nothing, wherever its offsets point
    empty = [(0, 100, 0, 100, 100), (10**12, 7, 10**12, 7, 0)]
    with pytest.raises(AssertionError, match="slime_rs_plan_execute_batch reached"):
        plan.execute_batch(buf, buf, _batch(empty, 8))  # passes every check: the C call is next


def test_execute_batch_refuses_a_wrong_dtype(plan):
    rows = [(0, 16, 0, 16, 16)]
    good = torch.zeros(12 * 16, dtype=torch.int32)
    for bad in (torch.zeros(12 * 16, dtype=torch.int64), torch.zeros(12 * 16, dtype=torch.float32),
                torch.zeros(12 * 16, 2, dtype=torch.int32)[:, 0]):  # the last: not contiguous
        with pytest.raises(TypeError):
            plan.execute_batch(bad, good, _batch(rows, 8))
        with pytest.raises(TypeError):
            plan.execute_batch(good, bad, _batch(rows, 8))


def test_execute_batch_refuses_another_device_or_k(plan, monkeypatch):
    rows = [(0, 16, 0, 16, 16)]
    good = torch.zeros(12 * 16, dtype=torch.int32)
    with pytest.raises(ValueError, match="k=4"):
        plan.execute_batch(good, good, _batch(rows, 4))
    with pytest.raises(ValueError, match="device 1"):
        plan.execute_batch(good, good, _batch(rows, 8, device=1))
    monkeypatch.setattr(D, "_dev_index", lambda t: 1)
    with pytest.raises(ValueError, match="plan's device"):
        plan.execute_batch(good, good, _batch(rows, 8))


def test_packed_layout_offsets(monkeypatch):
    """Batch.packed: shards align-rounded L apart, objects one after another, src == dst."""
    made = {}

    def fake_init(self, spans, k, device=0):
        made["spans"], made["k"], made["device"] = spans, k, device

    monkeypatch.setattr(D.Batch, "__init__", fake_init)
    monkeypatch.setattr(D.Batch, "__del__", lambda self: None)
    _, total = D.Batch.packed([5, 0, 64, 65], nshards=3, k=2, align=64, device=0)
    assert made["spans"] == [(0, 64, 0, 64, 5), (192, 0, 192, 0, 0), (192, 64, 192, 64, 64), (384, 128, 384, 128, 65)]
    assert total == 384 + 3 * 128 and made["k"] == 2
    _, total = D.Batch.packed([5, 1], nshards=3, k=2, align=1)
    assert made["spans"] == [(0, 5, 0, 5, 5), (15, 1, 15, 1, 1)] and total == 18
