"""Host-side checks of the verify entry points (no GPU): the C calls refuse a
null plan with a detail that names them, and the Python wrappers refuse bad
extents, dtypes and chunk strides before any C call."""
import ctypes

import pytest
import torch

from slime_amd import _native as N
from slime_amd import device as D


def test_plan_verify_null_plan_is_invalid_arg():
    lay = N.Layout(obj_stride=8, shard_stride=4)
    rc = N.lib.slime_rs_plan_verify(None, None, lay, None, lay, 4, 1, None, None, None)
    assert rc == N.ERR_INVALID_ARG
    assert "plan_verify" in N.lib.slime_rs_last_error().decode()


def test_verify_objects_null_plan_is_invalid_arg():
    rc = N.lib.slime_rs_verify_objects(None, None, 64, 0, 4, 1, None, None, None, None)
    assert rc == N.ERR_INVALID_ARG
    assert "verify_objects" in N.lib.slime_rs_last_error().decode()


class _NoCalls:
    """Stands in for the native library: any C call fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"C call {name} reached")


@pytest.fixture
def plan(monkeypatch):
    """An 8/12 encode-shaped plan with outputs 8..11 and no native handle, over
    CPU tensors that pass for device 0; the native library is unreachable."""
    monkeypatch.setattr(D, "lib", _NoCalls())
    monkeypatch.setattr(D, "_dev_index", lambda t: 0)
    p = D.Plan.__new__(D.Plan)
    p._h, p.device, p.in_max, p.out_max, p.rows, p.k = None, 0, 7, 11, 4, 8
    return p


def test_plan_verify_refuses_an_extent_past_the_tensor(plan):
    L, nobj = 100, 3
    lay = D.layout_of(12, L)
    buf = torch.zeros(nobj * 12 * L, dtype=torch.int32)
    with pytest.raises(ValueError, match="addresses element"):
        plan.verify(buf, lay, buf, lay, L, nobj + 1)  # one object too many
    data = torch.zeros(nobj * 8 * L, dtype=torch.int32)  # the inputs alone, packed
    with pytest.raises(ValueError, match="addresses element"):
        plan.verify(data, D.layout_of(8, L), buf, lay, L, nobj, src_offset=1)  # the last input row ends past it
    with pytest.raises(ValueError, match="addresses element"):
        plan.verify(buf, lay, buf, lay, L, nobj, cmp_offset=1)  # the last stored row does
    short = torch.zeros(nobj * 12 * L - 4 * L, dtype=torch.int32)  # holds the inputs, not the parity rows
    with pytest.raises(ValueError, match="addresses element"):
        plan.verify(buf, lay, short, lay, L, nobj)


def test_plan_verify_refuses_a_wrong_dtype(plan):
    L, nobj = 16, 2
    lay = D.layout_of(12, L)
    good = torch.zeros(nobj * 12 * L, dtype=torch.int32)
    for bad in (torch.zeros(nobj * 12 * L, dtype=torch.int64), torch.zeros(nobj * 12 * L, dtype=torch.float32),
                torch.zeros(nobj * 12 * L, 2, dtype=torch.int32)[:, 0]):  # the last: not contiguous
        with pytest.raises(TypeError):
            plan.verify(bad, lay, good, lay, L, nobj)
        with pytest.raises(TypeError):
            plan.verify(good, lay, bad, lay, L, nobj)


def test_verify_objects_refuses_bad_layouts(plan):
    L, nobj = 1025, 2
    slot = 4 * L * 12
    slots = torch.zeros(nobj * slot, dtype=torch.uint8)
    mapping = torch.zeros(nobj, dtype=torch.int32)
    for cs in (4 * L - 4, 4 * L + 2):  # below 4L; not a multiple of 4
        with pytest.raises(ValueError, match="chunk_stride"):
            D.verify_objects(plan, slots, slot, L, nobj, mapping, chunk_stride=cs)
    with pytest.raises(ValueError, match="slot layout"):
        D.verify_objects(plan, slots, slot, L, nobj + 1, mapping)  # an extent past the tensor
    with pytest.raises(ValueError, match="slot layout"):
        D.verify_objects(plan, slots, slot, L, nobj, mapping, chunk_stride=4 * L + 4)  # chunks outgrow the slot
    with pytest.raises(TypeError):
        D.verify_objects(plan, slots.to(torch.int32), slot, L, nobj, mapping)  # a wrong dtype
    with pytest.raises(ValueError, match="mapping"):
        D.verify_objects(plan, slots, slot, L, nobj, mapping.to(torch.int64))
    with pytest.raises(ValueError, match="mapping"):
        D.verify_objects(plan, slots, slot, L, nobj, mapping[:1])


def test_verify_signatures_match_the_header():
    """Both calls are bound with ten arguments, the results and stream last."""
    sig = {name: args for name, _, args in N.SIGNATURES}
    assert len(sig["slime_rs_plan_verify"]) == 10 and sig["slime_rs_plan_verify"][2] is N.Layout
    assert len(sig["slime_rs_verify_objects"]) == 10
    assert sig["slime_rs_verify_objects"][2:6] == [ctypes.c_uint64] * 4
