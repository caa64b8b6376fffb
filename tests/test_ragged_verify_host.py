"""Host-side checks of the ragged verify (no GPU): the step rule's CPU test
program, the two C entry points' refusal of null arguments, their signatures
against the header, and the Python wrappers' refusals before any C call."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from slime_amd import _native as N
from slime_amd import device as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "verify_step_test")
CALLS = ("slime_rs_plan_verify_batch", "slime_rs_planset_verify_batch")


def test_verify_step_rule():
    """slime_amd/csrc/verify_step.hpp for every k = 1..16 and R in {2, 4}: the steps cover each
    batch tile's vectors exactly once and in order, and no step holds more vectors a lane than
    the budget 24 / (k + R) clipped to 1..4."""
    subprocess.run(["make", "-C", ROOT, "tests/cpp/verify_step_test"], check=True, capture_output=True)
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "verify_step_test ok" in r.stdout


def _detail():
    return N.lib.slime_rs_last_error().decode()


def test_verify_batch_calls_refuse_null_arguments():
    a = np.zeros(8, dtype=np.uint64)
    p = a.ctypes.data  # any non-null address: the handles are checked first, nothing is read
    assert N.lib.slime_rs_plan_verify_batch(None, None, None, None, None, None, None) == N.ERR_INVALID_ARG
    assert "plan_verify_batch" in _detail() and "plan" in _detail()
    assert N.lib.slime_rs_plan_verify_batch(None, None, p, p, p, p, None) == N.ERR_INVALID_ARG
    assert "plan_verify_batch" in _detail()
    assert N.lib.slime_rs_planset_verify_batch(None, None, None, None, None, None, None) == N.ERR_INVALID_ARG
    assert "planset_verify_batch" in _detail() and "set" in _detail()
    assert N.lib.slime_rs_planset_verify_batch(None, None, p, p, p, p, None) == N.ERR_INVALID_ARG
    assert "planset_verify_batch" in _detail()


def test_verify_batch_signatures_match_the_header():
    text = open(os.path.join(ROOT, "include", "slime_rs.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    sig = {name: args for name, _, args in N.SIGNATURES}
    for name in CALLS:
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text)
        assert m, name
        assert len(sig[name]) == len(m.group(1).split(",")) == 7, name


class _NoCalls:
    """Stands in for the native library: any C call fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"C call {name} reached")


def _batch(rows, k, device=0, plans=None, nplans=None):
    """A Batch with no native handle over the given spans."""
    b = D.Batch.__new__(D.Batch)
    b._h, b.k, b.device, b._extents = None, k, device, {}
    b.spans = np.asarray(rows, dtype=np.uint64).reshape(-1, 5)
    b.nobj, b.plans, b.nplans = len(b.spans), plans, nplans
    return b


@pytest.fixture
def plan(monkeypatch):
    """An 8/12 encode-shaped plan with outputs 8..11 and no native handle, over CPU tensors that
    pass for device 0; the native library is unreachable and result tensors are CPU tensors."""
    monkeypatch.setattr(D, "lib", _NoCalls())
    monkeypatch.setattr(D, "_dev_index", lambda t: 0)
    monkeypatch.setattr(D, "_verify_results", lambda nobj, rows, device: (torch.empty((nobj, rows), dtype=torch.int64),
                                                                         torch.empty((nobj, rows), dtype=torch.int64)))
    p = D.Plan.__new__(D.Plan)
    p._h, p.device, p.in_max, p.out_max, p.rows, p.k = None, 0, 7, 11, 4, 8
    return p


def test_plan_verify_batch_checks_extents_dtype_and_k_first(plan):
    rows = [(0, 100, 0, 100, 100), (1200, 7, 1200, 7, 7)]
    buf = torch.zeros(1200 + 12 * 7, dtype=torch.int32)
    with pytest.raises(ValueError, match="span 1 addresses element"):
        plan.verify_batch(buf, buf[:-1].contiguous(), _batch(rows, 8))  # cmp one short of the last stored row
    src_only = torch.zeros(1200 + 8 * 7, dtype=torch.int32)  # ends with the last object's inputs
    with pytest.raises(ValueError, match="span 1 addresses element"):
        plan.verify_batch(src_only, src_only, _batch(rows, 8))
    with pytest.raises(ValueError, match="addresses element"):
        plan.verify_batch(buf, buf, _batch(rows, 8), cmp_offset=1)
    with pytest.raises(ValueError, match="addresses element"):
        plan.verify_batch(buf, buf, _batch(rows, 8), src_offset=-1)
    with pytest.raises(TypeError):
        plan.verify_batch(buf.to(torch.int64), buf, _batch(rows, 8))
    with pytest.raises(TypeError):
        plan.verify_batch(buf, torch.zeros(len(buf), 2, dtype=torch.int32)[:, 0], _batch(rows, 8))
    with pytest.raises(ValueError, match="k=4"):
        plan.verify_batch(buf, buf, _batch(rows, 4))
    with pytest.raises(ValueError, match="device 1"):
        plan.verify_batch(buf, buf, _batch(rows, 8, device=1))
    with pytest.raises(AssertionError, match="slime_rs_plan_verify_batch reached"):
        plan.verify_batch(src_only, buf, _batch(rows, 8))  # passes every check: the C call is next
    m, f = plan.verify_batch(buf, buf, _batch([], 8))  # no objects: no results, no C call
    assert m.shape == f.shape == (0, 4)


def test_planset_verify_batch_checks_the_batch_first(plan):
    pset = D.PlanSet.__new__(D.PlanSet)
    pset._h, pset.device, pset.nplans, pset.k, pset.max_rows, pset.in_max, pset.out_max = None, 0, 2, 8, 4, 9, 11
    rows = [(0, 100, 0, 100, 100), (1200, 7, 1200, 7, 7)]
    buf = torch.zeros(1200 + 12 * 7, dtype=torch.int32)
    planned = dict(plans=np.array([0, 1], dtype=np.uint32), nplans=2)
    with pytest.raises(ValueError, match="no plan indices"):
        pset.verify_batch(buf, buf, _batch(rows, 8))
    with pytest.raises(ValueError, match="3 plans"):
        pset.verify_batch(buf, buf, _batch(rows, 8, plans=planned["plans"], nplans=3))
    with pytest.raises(ValueError, match="k=4"):
        pset.verify_batch(buf, buf, _batch(rows, 4, **planned))
    with pytest.raises(ValueError, match="span 1 addresses element"):
        pset.verify_batch(buf, buf[:-1].contiguous(), _batch(rows, 8, **planned))
    with pytest.raises(TypeError):
        pset.verify_batch(buf.to(torch.int16), buf, _batch(rows, 8, **planned))
    # an intact object addresses nothing, wherever its offsets point
    far = [(0, 100, 0, 100, 100), (10**12, 7, 10**12, 7, 7)]
    intact = np.array([0, N.NO_PLAN], dtype=np.uint32)
    with pytest.raises(AssertionError, match="slime_rs_planset_verify_batch reached"):
        pset.verify_batch(buf, buf, _batch(far, 8, plans=intact, nplans=2))
