"""Host-side checks of the ragged byte encode (no GPU): the entry points are
exported with ctypes signatures that match the header, they refuse null
handles, the Python wrappers refuse bad arguments before any C call, the header
states what stays out of scope, and the edge geometry (encode_edge.hpp) holds
against a brute-force classification of every word (tests/cpp/encode_edge_test.cpp)."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from slime_amd import _native as N
from slime_amd import device as D
from test_bytes_ragged_host import _NoCalls, _batch, _header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {"slime_rs_encode_objects_batch": 8, "slime_rs_encode_objects_batch_phased": 9,
         "slime_rs_resolve_fallbacks_batch": 9}


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
        assert name.replace("slime_rs_", "").replace("_phased", "") in detail and "plan" in detail
        assert fn(None, None, *([p] * (nargs - 3)), None) == N.ERR_INVALID_ARG


def test_header_states_the_scope():
    flat = " ".join(_header().split()).replace(" * ", " ")
    assert "a ragged byte encode" not in flat, "no sentence calls it out of scope any more"
    for phrase in ("mid-object switch, redo lists and top-bit correction for ragged objects",
                   "a matrix-core or k-template ragged encode", "a plan-set encode", "host entry points and digests"):
        assert phrase in flat, phrase


@pytest.fixture
def plan(monkeypatch):
    """An 8/12 encode plan with outputs 8..11 and no native handle, over CPU tensors that pass for
    device 0; the native library is unreachable."""
    monkeypatch.setattr(D, "lib", _NoCalls())
    monkeypatch.setattr(D, "_dev_index", lambda t: 0)
    monkeypatch.setattr(D, "_note_unprobed", lambda t: None)
    p = D.Plan.__new__(D.Plan)
    p._h, p.device, p.in_max, p.out_max, p.rows, p.k = None, 0, 7, 11, 4, 8
    return p


ROWS = [(0, 100, 0, 100, 100), (1200, 7, 1200, 7, 7)]
WORDS = 1200 + 12 * 7
SIZES = [4 * 8 * 100 - 3, 4 * 8 * 7 - 30]


def _both(plan, *args, **kw):
    """The two wrappers with the same arguments (resolve needs mapping and status)."""
    yield lambda: D.encode_objects_batch(plan, *args, **kw)
    if kw.get("mapping") is not None and kw.get("status") is not None:
        yield lambda: D.resolve_fallbacks_batch(plan, *args, **kw)


def test_wrappers_check_everything_before_any_c_call(plan, monkeypatch):
    buf = torch.zeros(4 * WORDS, dtype=torch.uint8)
    mp, st = torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    ok = dict(mapping=mp, status=st)

    def refused(match, *args, **kw):
        for call in _both(plan, *args, **kw):
            with pytest.raises(ValueError, match=match):
                call()

    refused("uint8", torch.zeros(WORDS, dtype=torch.int32), buf, _batch(ROWS, 8), SIZES, **ok)  # a wrong dtype
    refused("uint8", buf, torch.zeros(4 * WORDS, 2, dtype=torch.uint8)[:, 0], _batch(ROWS, 8), SIZES, **ok)
    refused("mapping needs 2", buf, buf, _batch(ROWS, 8), SIZES, mapping=mp[:1], status=st)
    refused("status needs 2", buf, buf, _batch(ROWS, 8), SIZES, mapping=mp, status=torch.zeros(2, dtype=torch.int64))
    refused("span 1 addresses element", buf, buf[:-1], _batch(ROWS, 8), SIZES, **ok)  # one byte short
    refused("k=4", buf, buf, _batch(ROWS, 4), SIZES, **ok)
    refused("device 1", buf, buf, _batch(ROWS, 8, device=1), SIZES, **ok)
    refused("sizes needs 2 entries", buf, buf, _batch(ROWS, 8), SIZES[:1], **ok)  # short sizes
    refused("sizes needs 2", buf, buf, _batch(ROWS, 8), torch.zeros(1, dtype=torch.int64), **ok)
    refused("sizes needs 2", buf, buf, _batch(ROWS, 8), torch.zeros(2, dtype=torch.int32), **ok)
    refused("L=7", buf, buf, _batch(ROWS, 8), [SIZES[0], 4 * 8 * 7 + 1], **ok)  # a size that contradicts L
    refused("L=100", buf, buf, _batch(ROWS, 8), [4 * 8 * 99, SIZES[1]], **ok)
    pset = D.PlanSet.__new__(D.PlanSet)
    with pytest.raises(ValueError, match="takes a Plan"):
        D.encode_objects_batch(pset, buf, buf, _batch(ROWS, 8), SIZES, **ok)
    with pytest.raises(ValueError, match="needs the mapping and status"):
        D.resolve_fallbacks_batch(plan, buf, buf, _batch(ROWS, 8), SIZES, None, None)
    # passes every check: the C call is next; an object without work may carry any size
    with pytest.raises(AssertionError, match="slime_rs_encode_objects_batch_phased reached"):
        D.encode_objects_batch(plan, buf, buf, _batch(ROWS, 8), SIZES, **ok)
    with pytest.raises(AssertionError, match="slime_rs_encode_objects_batch_phased reached"):
        D.encode_objects_batch(plan, buf, buf, _batch(ROWS, 8), SIZES)  # mapping and status made by the wrapper
    far = [(0, 100, 0, 100, 100), (10**12, 7, 10**12, 7, 0)]
    with pytest.raises(AssertionError, match="slime_rs_resolve_fallbacks_batch reached"):
        D.resolve_fallbacks_batch(plan, buf, buf, _batch(far, 8), [SIZES[0], 12345], mp, st)
    monkeypatch.setattr(D, "_dev_index", lambda t: 1 if t.dtype == torch.int64 else 0)  # sizes alone elsewhere
    refused("sizes needs 2", buf, buf, _batch(ROWS, 8), torch.zeros(2, dtype=torch.int64), **ok)


def test_edge_geometry_against_brute_force():
    """tests/cpp/encode_edge_test.cpp: for every k <= 20 and S <= 4k * 70 no column below the
    interior bound holds a partial or padding word in any chunk, and at most k + 3 columns lie at
    or past it."""
    subprocess.run(["make", "-C", ROOT, "tests/cpp/encode_edge_test"], check=True, capture_output=True)
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "encode_edge_test")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "encode_edge_test ok" in r.stdout and "at most 23 edge columns" in r.stdout
