"""Host-side checks of plan sets (no GPU): the table layout's CPU test program,
the unedited ragged table test against the extended header, the C calls'
refusals that return before any device is touched, and the Python wrappers'
refusals before any C call."""
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


def _run_cpp(name):
    subprocess.run(["make", "-C", ROOT, f"tests/cpp/{name}"], check=True, capture_output=True)
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", name)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_planset_tables():
    """slime_amd/csrc/planset_table.hpp over seeded random sets (k 1..40, rows 1..8): 64-byte
    aligned, in-bounds, non-overlapping records and blocks that round-trip; its refusals; and
    ragged_plan.hpp's planned build (index in the descriptor, NO_PLAN like L == 0, the unplanned
    lists over the remaining objects, an index >= nplans refused)."""
    out = _run_cpp("planset_table_test")
    for name in ("TestRandomSets", "TestSetRefusals", "TestPlannedBatch"):
        assert f"ok   {name}" in out


def test_ragged_plan_test_still_passes_against_the_extended_header():
    """tests/cpp/ragged_plan_test.cpp calls count() and build() with their old signatures."""
    out = _run_cpp("ragged_plan_test")
    for name in ("TestHandMade", "TestOrder", "TestRandom", "TestRefusals"):
        assert f"ok   {name}" in out


def _detail():
    return N.lib.slime_rs_last_error().decode()


def test_planset_create_refuses_null_arguments_and_no_plans():
    h = ctypes.c_void_p(1)
    arr = (ctypes.c_void_p * 2)(None, None)
    assert N.lib.slime_rs_planset_create(arr, 2, None) == N.ERR_INVALID_ARG
    assert "planset_create" in _detail() and "null set" in _detail()
    assert N.lib.slime_rs_planset_create(None, 2, ctypes.byref(h)) == N.ERR_INVALID_ARG
    assert "planset_create" in _detail() and "null plans" in _detail()
    assert not h.value  # cleared on every refusal
    h = ctypes.c_void_p(1)
    assert N.lib.slime_rs_planset_create(arr, 0, ctypes.byref(h)) == N.ERR_INVALID_ARG
    assert "at least one plan" in _detail() and not h.value
    assert N.lib.slime_rs_planset_create(arr, 2, ctypes.byref(h)) == N.ERR_INVALID_ARG  # null members
    assert "plan 0 is null" in _detail()


def test_planset_calls_refuse_null_handles():
    n = ctypes.c_uint32()
    assert N.lib.slime_rs_planset_info(None, ctypes.byref(n), None, None, None, None) == N.ERR_INVALID_ARG
    assert "planset_info" in _detail()
    assert N.lib.slime_rs_planset_destroy(None) == N.ERR_INVALID_ARG
    assert "planset_destroy" in _detail()
    assert N.lib.slime_rs_planset_execute_batch(None, None, None, None, None) == N.ERR_INVALID_ARG
    assert "planset_execute_batch" in _detail() and "set" in _detail()


def _spans(rows):
    return (N.Span * len(rows))(*[N.Span(*r) for r in rows])


def test_batch_create_planned_refuses_bad_arguments():
    h = ctypes.c_void_p()
    two = _spans([(0, 8, 0, 8, 8), (96, 8, 96, 8, 8)])
    u32 = ctypes.c_uint32 * 2
    assert N.lib.slime_rs_batch_create_planned(0, 4, two, u32(0, 1), 2, 2, None) == N.ERR_INVALID_ARG
    assert "batch_create_planned" in _detail()
    assert N.lib.slime_rs_batch_create_planned(0, 4, two, None, 2, 2, ctypes.byref(h)) == N.ERR_INVALID_ARG
    assert "plan_of" in _detail()
    assert N.lib.slime_rs_batch_create_planned(0, 4, None, u32(0, 1), 2, 2, ctypes.byref(h)) == N.ERR_INVALID_ARG
    assert "spans" in _detail()
    for nplans in (0, N.PLANSET_MAX_PLANS + 1):
        assert N.lib.slime_rs_batch_create_planned(0, 4, two, u32(0, 0), nplans, 2, ctypes.byref(h)) == N.ERR_INVALID_ARG
        assert "nplans" in _detail()
    # plan_of[o] < nplans is checked on the host, before the device
    assert N.lib.slime_rs_batch_create_planned(0, 4, two, u32(0, 2), 2, 2, ctypes.byref(h)) == N.ERR_INVALID_ARG
    assert "span 1" in _detail() and "plan index 2" in _detail()
    assert N.lib.slime_rs_batch_create_planned(0, 0, two, u32(0, 1), 2, 2, ctypes.byref(h)) == N.ERR_INVALID_ARG
    assert not h.value
    assert N.NO_PLAN == 2**32 - 1 and N.PLANSET_MAX_PLANS >= 65536


def test_planset_signatures_match_the_header():
    text = open(os.path.join(ROOT, "include", "slime_rs.h")).read()
    assert re.search(r"#define SLIME_RS_NO_PLAN UINT32_MAX", text)
    m = re.search(r"#define SLIME_RS_PLANSET_MAX_PLANS \(1u << (\d+)\)", text)
    assert m and 1 << int(m.group(1)) == N.PLANSET_MAX_PLANS
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    sig = {name: args for name, _, args in N.SIGNATURES}
    for name in ("slime_rs_planset_create", "slime_rs_planset_info", "slime_rs_planset_destroy",
                 "slime_rs_batch_create_planned", "slime_rs_planset_execute_batch"):
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text)
        assert m, name
        assert len(sig[name]) == len(m.group(1).split(",")), name
    # §15's out-of-scope clause is gone from the header
    assert "one batch per group" not in open(os.path.join(ROOT, "include", "slime_rs.h")).read()


class _NoCalls:
    """Stands in for the native library: any C call fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"C call {name} reached")


def _batch(rows, k, plans=None, nplans=None, device=0):
    b = D.Batch.__new__(D.Batch)
    b._h, b.k, b.device, b._extents = None, k, device, {}
    b.spans = np.asarray(rows, dtype=np.uint64).reshape(-1, 5)
    b.plans = None if plans is None else np.asarray(plans, dtype=np.uint32)
    b.nplans = nplans
    return b


@pytest.fixture
def pset(monkeypatch):
    """A two-plan 8/12 set (inputs up to shard 9, outputs up to shard 11) with no native handle."""
    monkeypatch.setattr(D, "lib", _NoCalls())
    monkeypatch.setattr(D, "_dev_index", lambda t: 0)
    s = D.PlanSet.__new__(D.PlanSet)
    s._h, s.device, s.nplans, s.k, s.max_rows, s.in_max, s.out_max = None, 0, 2, 8, 4, 9, 11
    return s


def test_planset_execute_batch_checks_extents_with_the_set_wide_indices(pset):
    rows = [(0, 100, 0, 100, 100), (1200, 7, 1200, 7, 7)]
    buf = torch.zeros(1200 + 12 * 7, dtype=torch.int32)
    with pytest.raises(AssertionError, match="slime_rs_planset_execute_batch reached"):
        pset.execute_batch(buf, buf, _batch(rows, 8, [0, 1], 2))  # passes every check
    with pytest.raises(ValueError, match="span 1 addresses element"):
        pset.execute_batch(buf, buf[:-1].contiguous(), _batch(rows, 8, [0, 1], 2))
    ten = torch.zeros(1200 + 10 * 7, dtype=torch.int32)  # ends after shard 9 of the last object: src only
    with pytest.raises(ValueError, match="span 1 addresses element"):
        pset.execute_batch(ten, ten, _batch(rows, 8, [0, 1], 2))
    with pytest.raises(AssertionError, match="reached"):
        pset.execute_batch(ten, buf, _batch(rows, 8, [0, 1], 2))
    with pytest.raises(ValueError, match="addresses element"):
        pset.execute_batch(buf, buf, _batch(rows, 8, [0, 1], 2), dst_offset=1)
    # an intact object addresses nothing, wherever its offsets point
    far = [(0, 100, 0, 100, 100), (10**12, 7, 10**12, 7, 7)]
    with pytest.raises(AssertionError, match="reached"):
        pset.execute_batch(buf, buf, _batch(far, 8, [1, N.NO_PLAN], 2))
    with pytest.raises(ValueError, match="span 1 addresses element"):
        pset.execute_batch(buf, buf, _batch(far, 8, [1, 0], 2))


def test_planset_execute_batch_refuses_wrong_batches_and_tensors(pset, monkeypatch):
    rows = [(0, 16, 0, 16, 16)]
    good = torch.zeros(12 * 16, dtype=torch.int32)
    with pytest.raises(ValueError, match="no plan indices"):
        pset.execute_batch(good, good, _batch(rows, 8))
    with pytest.raises(ValueError, match="3 plans"):
        pset.execute_batch(good, good, _batch(rows, 8, [0], 3))
    with pytest.raises(ValueError, match="k=4"):
        pset.execute_batch(good, good, _batch(rows, 4, [0], 2))
    with pytest.raises(ValueError, match="device 1"):
        pset.execute_batch(good, good, _batch(rows, 8, [0], 2, device=1))
    with pytest.raises(TypeError):
        pset.execute_batch(torch.zeros(12 * 16, dtype=torch.int64), good, _batch(rows, 8, [0], 2))
    monkeypatch.setattr(D, "_dev_index", lambda t: 1)
    with pytest.raises(ValueError, match="plan set's device"):
        pset.execute_batch(good, good, _batch(rows, 8, [0], 2))


def test_for_erasures_dedups_patterns(monkeypatch):
    """One plan per distinct pattern in first-seen order: the first `need` survivors in, the erased
    indices out and as outputs; intact objects get NO_PLAN."""
    made = []

    class FakePlan:
        def __init__(self, need, total, have, want, device):
            self.args, self.outs = (need, total, list(have), list(want), device), None

        def set_outputs(self, outs):
            self.outs = list(outs)
            return self

        def close(self):
            pass

    def fake_reconstruct(need, total, have, want, device=0):
        made.append(FakePlan(need, total, have, want, device))
        return made[-1]

    monkeypatch.setattr(D.Plan, "reconstruct", staticmethod(fake_reconstruct))
    monkeypatch.setattr(D.PlanSet, "__init__", lambda self, plans: setattr(self, "got", list(plans)))
    monkeypatch.setattr(D.PlanSet, "__del__", lambda self: None)
    pats = [[0], [], [5, 2], [0], None, (2, 5), [0, 3, 8, 11], np.array([11])]
    s, idx = D.PlanSet.for_erasures(8, 12, pats, device=0)
    assert idx.dtype == np.uint32 and list(idx) == [0, N.NO_PLAN, 1, 0, N.NO_PLAN, 1, 2, 3]
    assert [p.args for p in s.got] == [
        (8, 12, [1, 2, 3, 4, 5, 6, 7, 8], [0], 0),
        (8, 12, [0, 1, 3, 4, 6, 7, 8, 9], [2, 5], 0),
        (8, 12, [1, 2, 4, 5, 6, 7, 9, 10], [0, 3, 8, 11], 0),
        (8, 12, [0, 1, 2, 3, 4, 5, 6, 7], [11], 0)]
    assert [p.outs for p in s.got] == [[0], [2, 5], [0, 3, 8, 11], [11]]
    with pytest.raises(ValueError, match="fewer than 8"):
        D.PlanSet.for_erasures(8, 12, [[0, 1, 2, 3, 4]])
    with pytest.raises(ValueError, match="fewer than 8"):
        D.PlanSet.for_erasures(8, 12, [[12]])
    with pytest.raises(ValueError, match="nothing to repair"):
        D.PlanSet.for_erasures(8, 12, [[], None])


def test_planned_batch_arguments(monkeypatch):
    monkeypatch.setattr(D, "lib", _NoCalls())
    rows = [(0, 16, 0, 16, 16), (192, 16, 192, 16, 16)]
    with pytest.raises(ValueError, match="one index"):
        D.Batch(rows, 8, plans=[0])
    with pytest.raises(ValueError, match="one index"):
        D.Batch(rows, 8, plans=[0, -1], nplans=2)
    with pytest.raises(ValueError, match="nplans"):
        D.Batch(rows, 8, plans=[0, 1])
    with pytest.raises(ValueError, match="nplans needs"):
        D.Batch(rows, 8, nplans=2)
    with pytest.raises(AssertionError, match="slime_rs_batch_create_planned reached"):
        D.Batch(rows, 8, plans=[0, N.NO_PLAN], nplans=2)
