"""Host-side checks of correct (no GPU): the correct rule's CPU test program
(correct_rule.hpp is what the device runs), tests/correct_ref.py pinned to the
C++ rule on the cases the program prints, the four C entry points' signatures
and their refusal of max_wrong and null handles, and the Python calls' checks
before any C call."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import correct_ref as CR
from slime_amd import _native as N
from slime_amd import device as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "correct_rule_test")
CALLS = {"slime_rs_plan_correct_batch": 9, "slime_rs_correct_objects_batch": 10,
         "slime_rs_planset_correct_batch": 9, "slime_rs_planset_correct_objects_batch": 10}
NO_SLOT = 0xFFFFFFFF


@pytest.fixture(scope="module")
def binary():
    subprocess.run(["make", "-C", ROOT, "tests/cpp/correct_rule_test"], check=True, capture_output=True)
    return BIN


def test_correct_rule(binary):
    """inv at the edge values and 10^5 random ones; every planted slot and every planted pair of
    3/7 ... 33/50, 59/63 and 3/63 comes back exactly; aliases p + t; the degenerate matrices never
    take a write that leaves a column dirty."""
    r = subprocess.run([binary], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "correct_rule_test ok" in r.stdout


def _cases(binary):
    r = subprocess.run([binary, "--cases"], capture_output=True, text=True, timeout=600, check=True)
    out = []
    for line in r.stdout.splitlines():
        f = line.split("|")
        if len(f) != 8:
            continue
        rows, k = (int(v) for v in f[0].split())
        coeff = np.array(f[1].split(), dtype=np.uint64).astype(np.uint32).reshape(rows, k).tolist()
        x, stored = [int(v) for v in f[2].split()], [int(v) for v in f[3].split()]
        a, b = (int(v) for v in f[5].split())
        out.append((coeff, x, stored, int(f[4]), (CR.CLEAN if a == NO_SLOT else a, CR.NONE if b == NO_SLOT else b),
                    [int(v) for v in f[6].split()], [int(v) for v in f[7].split()]))
    return out


def test_python_reference_equals_the_cpp_rule(binary):
    """The cases the C++ program prints through correct_ref.correct_column: the same slots and the
    same column afterwards, over every kind of outcome."""
    cases = _cases(binary)
    assert len(cases) > 1000
    seen = set()
    for coeff, x, stored, max_wrong, slots, x_after, stored_after in cases:
        rows, k = len(coeff), len(coeff[0])
        a, b, fx, fs = CR.correct_column(coeff, x, stored, max_wrong)
        assert ((a, b), fx, fs) == (slots, x_after, stored_after), (k, rows, max_wrong, x, stored)
        wrote = (fx, fs) != (x, stored)
        if b != CR.NONE:
            assert wrote
            seen.add("pair of " + " and ".join("input" if s < k else "row" for s in (a, b)))
        elif a == CR.CLEAN or a == k + rows:
            assert not wrote
            seen.add("clean" if a == CR.CLEAN else "unlocated")
        else:
            assert wrote
            seen.add("input" if a < k else "row")
        if wrote:
            assert CR.correct_column(coeff, fx, fs, max_wrong)[0] == CR.CLEAN, "a corrected column is clean"
    assert seen == {"clean", "input", "row", "unlocated", "pair of input and input", "pair of input and row",
                    "pair of row and row"}
    # an all-zero coefficient column named alone: unsolvable, reported unlocated, nothing written
    zero = [[0, 5], [0, 7]]
    assert CR.R.classify(zero, [1, 2], [3, 4]) == 0
    assert CR.correct_column(zero, [1, 2], [3, 4]) == (4, CR.NONE, [1, 2], [3, 4])


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
        args = [" ".join(a.split()) for a in m.group(1).split(",")]
        assert len(sig[name]) == len(args) == nargs, name
        # the locate twin's argument list, the data pointers writable and max_wrong behind the filter
        twin = re.search(r"\b" + name.replace("correct", "locate") + r"\s*\(([^)]*)\)", text)
        targs = [" ".join(a.split()).replace("const uint32_t *src", "uint32_t *src")
                 .replace("const uint32_t *cmp", "uint32_t *cmp").replace("const uint8_t *", "uint8_t *")
                 for a in twin.group(1).split(",")]
        at = targs.index("const uint64_t *filter") + 1
        assert args == targs[:at] + ["int max_wrong"] + targs[at:], name
        import ctypes
        assert sig[name][at] is ctypes.c_int


def test_calls_refuse_max_wrong_first_and_then_null_handles():
    a = np.zeros(8, dtype=np.uint64)
    p = a.ctypes.data  # any non-null address: the checks come first, nothing is read
    for name, nargs in CALLS.items():
        fn = getattr(N.lib, name)
        what = name.replace("slime_rs_", "")
        at = nargs - 4  # max_wrong sits before counts, first and the stream
        for bad in (0, 3, -1):
            args = [None] * nargs
            args[at] = bad
            assert fn(*args) == N.ERR_INVALID_ARG
            assert N.lib.slime_rs_last_error().decode() == (
                f"{what}: max_wrong = {bad} is neither 1 (one wrong shard per column) nor 2 (a pair)")
        for ok in (1, 2):
            args = [None] * nargs
            args[at] = ok
            assert fn(*args) == N.ERR_INVALID_ARG
            assert N.lib.slime_rs_last_error().decode() == what + (": null set" if "planset" in name else ": null plan")
            args = [None, None] + [p] * (nargs - 3) + [None]
            args[at] = ok
            assert fn(*args) == N.ERR_INVALID_ARG


def test_header_states_the_contract():
    flat = " ".join(_header().split()).replace(" * ", " ")
    for phrase in ("fix the words locate names, in place", "max_wrong neither 1 nor 2", "cmp may be src",
                   "do not overlap in memory", "counted under `unlocated`", "canonical residues",
                   "BE(sym ^ mapping[o])", "k / p per such column", "(k + rows)^2 / (2 p^(rows - 2))",
                   "three or more wrong shards per column", "host-memory entry points", "the Go shim"):
        assert phrase in flat, phrase


class _NoCalls:
    """Stands in for the native library: any C call fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"C call {name} reached")


def _batch(rows, k, device=0):
    b = D.Batch.__new__(D.Batch)
    b._h, b.k, b.device, b._extents = None, k, device, {}
    b.spans = np.asarray(rows, dtype=np.uint64).reshape(-1, 5)
    b.nobj, b.plans, b.nplans = len(b.spans), None, None
    return b


def test_python_checks_run_before_any_c_call(monkeypatch):
    monkeypatch.setattr(D, "lib", _NoCalls())
    monkeypatch.setattr(D, "_dev_index", lambda t: 0)
    monkeypatch.setattr(D, "_verify_results", lambda nobj, rows, device: (torch.empty((nobj, rows), dtype=torch.int64),
                                                                         torch.empty((nobj, rows), dtype=torch.int64)))
    p = D.Plan.__new__(D.Plan)
    p._h, p.device, p.in_max, p.out_max, p.rows, p.k = None, 0, 7, 11, 4, 8
    rows = [(0, 100, 0, 100, 100), (1200, 7, 1200, 7, 7)]
    buf = torch.zeros(1200 + 12 * 7, dtype=torch.int32)
    chunks = torch.zeros(4 * len(buf), dtype=torch.uint8)
    mt = torch.zeros(2, dtype=torch.int32)
    for bad in (0, 3, -1, None, "2", 2.5, True):
        with pytest.raises(ValueError, match="max_wrong must be 1 or 2"):
            p.correct_batch(buf, buf, _batch(rows, 8), max_wrong=bad)
        with pytest.raises(ValueError, match="max_wrong must be 1 or 2"):
            D.correct_objects_batch(p, chunks, chunks, _batch(rows, 8), mt, max_wrong=bad)
    for mw in (1, 2):
        with pytest.raises(ValueError, match="span 1 addresses element"):
            p.correct_batch(buf, buf[:-1].contiguous(), _batch(rows, 8), max_wrong=mw)
        with pytest.raises(TypeError):
            p.correct_batch(buf.to(torch.int64), buf, _batch(rows, 8), max_wrong=mw)
        with pytest.raises(ValueError, match="k=4"):
            p.correct_batch(buf, buf, _batch(rows, 4), max_wrong=mw)
        with pytest.raises(ValueError, match="filter needs the 2 x 4"):
            p.correct_batch(buf, buf, _batch(rows, 8), filter=torch.zeros((2, 3), dtype=torch.int64), max_wrong=mw)
        with pytest.raises(AssertionError, match="slime_rs_plan_correct_batch reached"):
            p.correct_batch(buf, buf, _batch(rows, 8), filter=torch.zeros((2, 4), dtype=torch.int64), max_wrong=mw)
        c, f = p.correct_batch(buf, buf, _batch([], 8), max_wrong=mw)  # no objects: no results, no C call
        assert c.shape == f.shape == (0, 13)
        with pytest.raises(ValueError, match="addresses element"):
            D.correct_objects_batch(p, chunks, chunks[:-4].contiguous(), _batch(rows, 8), mt, max_wrong=mw)
        with pytest.raises(ValueError, match="mapping needs 2"):
            D.correct_objects_batch(p, chunks, chunks, _batch(rows, 8), mt[:1], max_wrong=mw)
        with pytest.raises(ValueError, match="filter needs the 2 x 4"):
            D.correct_objects_batch(p, chunks, chunks, _batch(rows, 8), mt, filter=torch.zeros(3, dtype=torch.int64),
                                    max_wrong=mw)
        with pytest.raises(AssertionError, match="slime_rs_correct_objects_batch reached"):
            D.correct_objects_batch(p, chunks, chunks, _batch(rows, 8), mt, max_wrong=mw)
    with pytest.raises(ValueError, match="takes a Plan or a PlanSet"):
        D.correct_objects_batch(object(), chunks, chunks, _batch(rows, 8), mt)
