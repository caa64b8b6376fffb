"""Host-side checks of the ragged locate (no GPU): the rule's CPU test program
(locate_rule.hpp is what the device runs), tests/locate_ref.py pinned to the C++
rule on the same planted cases, the two C entry points' signatures and refusal
of null handles, and the Python helpers."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import locate_ref as R
from slime_amd import _native as N
from slime_amd import device as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "locate_rule_test")
CALLS = {"slime_rs_plan_locate_batch": 8, "slime_rs_locate_objects_batch": 9}


@pytest.fixture(scope="module")
def binary():
    subprocess.run(["make", "-C", ROOT, "tests/cpp/locate_rule_test"], check=True, capture_output=True)
    return BIN


def test_locate_rule(binary):
    """Every single-shard error in every slot of 3/5 ... 33/50, 61/63, 3/63 and of a matrix with zeros is named,
    aliases classify as the rule says, and 10^5 random syndromes and double errors per matrix
    agree with the brute-force restatement."""
    r = subprocess.run([binary], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "locate_rule_test ok" in r.stdout


def _cases(binary):
    r = subprocess.run([binary, "--cases"], capture_output=True, text=True, timeout=300, check=True)
    out = []
    for line in r.stdout.splitlines():
        f = line.split("|")
        if len(f) != 5:
            continue
        rows, k = (int(v) for v in f[0].split())
        coeff = np.array(f[1].split(), dtype=np.uint64).astype(np.uint32).reshape(rows, k)
        x = [int(v) for v in f[2].split()]
        stored = [int(v) for v in f[3].split()]
        slot = int(f[4])
        assert len(x) == k and len(stored) == rows
        out.append((coeff, x, stored, R.CLEAN if slot == 0xFFFFFFFF else slot))
    return out


def test_python_reference_equals_the_cpp_rule(binary):
    """The planted cases the C++ program prints, through both forms of the Python reference."""
    cases = _cases(binary)
    assert len(cases) > 500
    seen = set()
    for coeff, x, stored, slot in cases:
        rows, k = coeff.shape
        assert R.classify(coeff.tolist(), x, stored) == slot, (k, rows, x, stored)
        ins = [np.array([v], dtype=np.uint32) for v in x]
        st = [np.array([v], dtype=np.uint32) for v in stored]
        assert R.slots_of_object(coeff, ins, st)[0] == slot, (k, rows, x, stored)
        seen.add("clean" if slot == R.CLEAN else "input" if slot < k else "row" if slot < k + rows else "unlocated")
    assert seen == {"clean", "input", "row", "unlocated"}
    # the two codes that fill all 63 slots: every input of k = 61 (bits of `cand` above 32) and
    # every one of 60 rows is named at least once, and both say unlocated at slot 63
    for k, rows in ((61, 2), (3, 60)):
        named = {slot for coeff, _, _, slot in cases if coeff.shape == (rows, k)}
        assert named == set(range(64)) | {R.CLEAN}, (k, rows, sorted(set(range(64)) - named))


def test_reference_tally():
    slots = np.array([R.CLEAN, 2, 5, 2, R.CLEAN, 0], dtype=np.int64)
    c, f = R.tally(slots, 6)
    assert c.tolist() == [1, 0, 2, 0, 0, 1] and f.tolist() == [5, -1, 1, -1, -1, 2]


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
        assert detail == name.replace("slime_rs_", "") + ": null plan"
        assert fn(None, None, *([p] * (nargs - 3)), None) == N.ERR_INVALID_ARG


def test_header_no_longer_calls_locating_out_of_scope():
    flat = " ".join(_header().split()).replace(" * ", " ")
    assert "locating which shard is wrong" not in flat
    for phrase in ("plan-set locate", "correcting more than one wrong shard per column", "device digests",
                   "blamed on a third shard"):
        assert phrase in flat, phrase


def test_erasures_from_counts_and_locate_slots():
    counts = np.array([[0, 0, 0, 0, 0, 0], [3, 0, 0, 0, 1, 0], [0, 0, 0, 0, 0, 7], [0, 1, 0, 2, 0, 0]])
    slots = [4, 0, 2, 1, 3]  # a reconstruct-shaped plan: inputs 4, 0, 2 and outputs 1, 3
    assert D.erasures_from_counts(counts, slots) == [[], [3, 4], [], [0, 1]]
    assert D.erasures_from_counts(torch.from_numpy(counts), slots) == [[], [3, 4], [], [0, 1]]
    with pytest.raises(ValueError, match="shape"):
        D.erasures_from_counts(counts[:, :5], slots)
    p = D.Plan.__new__(D.Plan)
    p.rows, p.k, p.in_shards, p.out_shards = 2, 3, [4, 0, 2], None
    assert p.locate_slots() == [4, 0, 2, 0, 1]
    p.out_shards = [1, 3]
    assert p.locate_slots() == slots
    p.in_shards = None
    with pytest.raises(ValueError, match="input shards"):
        p.locate_slots()


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


def test_locate_batch_runs_verify_batchs_checks_first(monkeypatch):
    monkeypatch.setattr(D, "lib", _NoCalls())
    monkeypatch.setattr(D, "_dev_index", lambda t: 0)
    monkeypatch.setattr(D, "_verify_results", lambda nobj, rows, device: (torch.empty((nobj, rows), dtype=torch.int64),
                                                                         torch.empty((nobj, rows), dtype=torch.int64)))
    p = D.Plan.__new__(D.Plan)
    p._h, p.device, p.in_max, p.out_max, p.rows, p.k = None, 0, 7, 11, 4, 8
    rows = [(0, 100, 0, 100, 100), (1200, 7, 1200, 7, 7)]
    buf = torch.zeros(1200 + 12 * 7, dtype=torch.int32)
    with pytest.raises(ValueError, match="span 1 addresses element"):
        p.locate_batch(buf, buf[:-1].contiguous(), _batch(rows, 8))
    with pytest.raises(ValueError, match="addresses element"):
        p.locate_batch(buf, buf, _batch(rows, 8), cmp_offset=1)
    with pytest.raises(TypeError):
        p.locate_batch(buf.to(torch.int64), buf, _batch(rows, 8))
    with pytest.raises(ValueError, match="k=4"):
        p.locate_batch(buf, buf, _batch(rows, 4))
    with pytest.raises(ValueError, match="filter needs the 2 x 4"):
        p.locate_batch(buf, buf, _batch(rows, 8), filter=torch.zeros((2, 3), dtype=torch.int64))
    with pytest.raises(ValueError, match="filter needs"):
        p.locate_batch(buf, buf, _batch(rows, 8), filter=torch.zeros((2, 4), dtype=torch.int32))
    with pytest.raises(AssertionError, match="slime_rs_plan_locate_batch reached"):
        p.locate_batch(buf, buf, _batch(rows, 8), filter=torch.zeros((2, 4), dtype=torch.int64))
    c, f = p.locate_batch(buf, buf, _batch([], 8))  # no objects: no results, no C call
    assert c.shape == f.shape == (0, 13)
    chunks = torch.zeros(4 * len(buf), dtype=torch.uint8)
    mt = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="addresses element"):
        D.locate_objects_batch(p, chunks, chunks[:-4].contiguous(), _batch(rows, 8), mt)
    with pytest.raises(ValueError, match="mapping needs 2"):
        D.locate_objects_batch(p, chunks, chunks, _batch(rows, 8), mt[:1])
    with pytest.raises(AssertionError, match="slime_rs_locate_objects_batch reached"):
        D.locate_objects_batch(p, chunks, chunks, _batch(rows, 8), mt)
