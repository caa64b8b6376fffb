"""Host-side checks of the ragged byte launches (no GPU): the four C entry
points are exported with ctypes signatures that match the header, they refuse
null handles, the Python wrappers refuse bad arguments before any C call, and
the header no longer calls the byte-slot ragged forms out of scope."""
import os
import re

import numpy as np
import pytest
import torch

from slime_amd import _native as N
from slime_amd import device as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {"slime_rs_decode_objects_batch": 6, "slime_rs_planset_decode_objects_batch": 6,
         "slime_rs_verify_objects_batch": 8, "slime_rs_planset_verify_objects_batch": 8}


def _header():
    return open(os.path.join(ROOT, "include", "slime_rs.h")).read()


def test_symbols_are_exported_with_signatures_that_match_the_header():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    sig = {name: args for name, _, args in N.SIGNATURES}
    for name, nargs in CALLS.items():
        fn = getattr(N.lib, name)  # AttributeError: the built library does not export it
        assert fn.restype is not None and len(fn.argtypes) == nargs, name
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text)
        assert m, name
        assert len(sig[name]) == len(m.group(1).split(",")) == nargs, name


def test_calls_refuse_null_handles():
    a = np.zeros(8, dtype=np.uint64)
    p = a.ctypes.data  # any non-null address: the handles are checked first, nothing is read
    for name, nargs in CALLS.items():
        fn = getattr(N.lib, name)
        assert fn(*([None] * nargs)) == N.ERR_INVALID_ARG
        detail = N.lib.slime_rs_last_error().decode()
        assert name.replace("slime_rs_", "") in detail and ("set" if "planset" in name else "plan") in detail
        assert fn(None, None, *([p] * (nargs - 3)), None) == N.ERR_INVALID_ARG


def test_header_names_what_remains_out_of_scope():
    flat = " ".join(_header().split()).replace(" * ", " ")  # comment text without its line breaks
    for gone in ("ragged forms of the byte-slot pipeline", "plan sets for the byte-slot pipeline",
                 "ragged or planned forms of slime_rs_verify_objects, locating"):
        assert gone not in flat, gone
    # the three reworded sentences and the new section each name what remains
    assert flat.count("ragged byte encode") >= 4 and flat.count("matrix-core forms") >= 4


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
    monkeypatch.setattr(D, "_note_unprobed", lambda t: None)
    monkeypatch.setattr(D, "_verify_results", lambda nobj, rows, device: (torch.empty((nobj, rows), dtype=torch.int64),
                                                                         torch.empty((nobj, rows), dtype=torch.int64)))
    p = D.Plan.__new__(D.Plan)
    p._h, p.device, p.in_max, p.out_max, p.rows, p.k = None, 0, 7, 11, 4, 8
    return p


ROWS = [(0, 100, 0, 100, 100), (1200, 7, 1200, 7, 7)]
WORDS = 1200 + 12 * 7


@pytest.mark.parametrize("call", ["decode_objects_batch", "verify_objects_batch"])
def test_plan_forms_check_dtype_mapping_extent_and_k_first(plan, call):
    fn = getattr(D, call)
    buf = torch.zeros(4 * WORDS, dtype=torch.uint8)
    mp = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="uint8"):
        fn(plan, torch.zeros(WORDS, dtype=torch.int32), buf, _batch(ROWS, 8), mp)  # a wrong dtype
    with pytest.raises(ValueError, match="uint8"):
        fn(plan, buf, torch.zeros(4 * WORDS, 2, dtype=torch.uint8)[:, 0], _batch(ROWS, 8), mp)  # not contiguous
    with pytest.raises(ValueError, match="mapping needs 2"):
        fn(plan, buf, buf, _batch(ROWS, 8), mp[:1])  # a short mapping
    with pytest.raises(ValueError, match="mapping needs 2"):
        fn(plan, buf, buf, _batch(ROWS, 8), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="span 1 addresses element"):
        fn(plan, buf, buf[:-1], _batch(ROWS, 8), mp)  # one byte short of the last output chunk
    src_only = torch.zeros(4 * (1200 + 8 * 7), dtype=torch.uint8)  # ends with the last object's inputs
    with pytest.raises(ValueError, match="span 1 addresses element"):
        fn(plan, src_only, src_only, _batch(ROWS, 8), mp)
    with pytest.raises(ValueError, match="k=4"):
        fn(plan, buf, buf, _batch(ROWS, 4), mp)
    with pytest.raises(ValueError, match="device 1"):
        fn(plan, buf, buf, _batch(ROWS, 8, device=1), mp)
    with pytest.raises(ValueError, match="Plan or a PlanSet"):
        fn(object(), buf, buf, _batch(ROWS, 8), mp)
    with pytest.raises(AssertionError, match="slime_rs_" + call + " reached"):
        fn(plan, src_only, buf, _batch(ROWS, 8), mp)  # passes every check: the C call is next


@pytest.mark.parametrize("call", ["decode_objects_batch", "verify_objects_batch"])
def test_set_forms_check_the_batch_first(plan, call):
    fn = getattr(D, call)
    pset = D.PlanSet.__new__(D.PlanSet)
    pset._h, pset.device, pset.nplans, pset.k, pset.max_rows, pset.in_max, pset.out_max = None, 0, 2, 8, 4, 9, 11
    buf = torch.zeros(4 * WORDS, dtype=torch.uint8)
    mp = torch.zeros(2, dtype=torch.int32)
    planned = dict(plans=np.array([0, 1], dtype=np.uint32), nplans=2)
    with pytest.raises(ValueError, match="no plan indices"):
        fn(pset, buf, buf, _batch(ROWS, 8), mp)
    with pytest.raises(ValueError, match="3 plans"):
        fn(pset, buf, buf, _batch(ROWS, 8, plans=planned["plans"], nplans=3), mp)
    with pytest.raises(ValueError, match="k=4"):
        fn(pset, buf, buf, _batch(ROWS, 4, **planned), mp)
    with pytest.raises(ValueError, match="span 1 addresses element"):
        fn(pset, buf, buf[:-1], _batch(ROWS, 8, **planned), mp)
    with pytest.raises(ValueError, match="uint8"):
        fn(pset, buf.to(torch.int16), buf, _batch(ROWS, 8, **planned), mp)
    with pytest.raises(ValueError, match="mapping needs 2"):
        fn(pset, buf, buf, _batch(ROWS, 8, **planned), mp[:1])
    # an intact object addresses nothing, wherever its offsets point
    far = [(0, 100, 0, 100, 100), (10**12, 7, 10**12, 7, 7)]
    intact = np.array([0, N.NO_PLAN], dtype=np.uint32)
    with pytest.raises(AssertionError, match="slime_rs_planset_" + call + " reached"):
        fn(pset, buf, buf, _batch(far, 8, plans=intact, nplans=2), mp)


def test_verify_wrapper_returns_empty_results_for_no_objects(plan):
    buf = torch.zeros(16, dtype=torch.uint8)
    m, f = D.verify_objects_batch(plan, buf, buf, _batch([], 8), torch.zeros(0, dtype=torch.int32))
    assert m.shape == f.shape == (0, 4)
