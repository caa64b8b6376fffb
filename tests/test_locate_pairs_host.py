"""Host-side checks of the pair locate (no GPU): the pair rule's CPU test program
(locate_rule.hpp is what the device runs) against its brute-force statement,
tests/locate_pairs_ref.py pinned to the C++ rule on the same planted cases, the
four C entry points' signatures and refusal of null handles, and the max_wrong
keyword of the Python calls with its checks before any C call."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import locate_pairs_ref as PR
from slime_amd import _native as N
from slime_amd import device as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "locate_pairs_rule_test")
CALLS = {"slime_rs_plan_locate_pairs_batch": 8, "slime_rs_locate_pairs_objects_batch": 9,
         "slime_rs_planset_locate_pairs_batch": 8, "slime_rs_planset_locate_pairs_objects_batch": 9}
NO_SLOT = 0xFFFFFFFF


@pytest.fixture(scope="module")
def binary():
    subprocess.run(["make", "-C", ROOT, "tests/cpp/locate_pairs_rule_test"], check=True, capture_output=True)
    return BIN


def test_pair_rule(binary):
    """Every planted pair of slots of 3/7 ... 33/50, 59/63 and 3/63 is named, single errors keep the
    one-shard rule's slot, aliases classify as the rule says, planted triples are unlocated, and
    10^5 random syndromes per matrix -- matrices with zeros and dependent columns among them --
    agree with the brute-force statement."""
    r = subprocess.run([binary], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "locate_pairs_rule_test ok" in r.stdout


def _cases(binary):
    r = subprocess.run([binary, "--cases"], capture_output=True, text=True, timeout=600, check=True)
    out = []
    for line in r.stdout.splitlines():
        f = line.split("|")
        if len(f) != 5:
            continue
        rows, k = (int(v) for v in f[0].split())
        coeff = np.array(f[1].split(), dtype=np.uint64).astype(np.uint32).reshape(rows, k)
        x = [int(v) for v in f[2].split()]
        stored = [int(v) for v in f[3].split()]
        a, b = (int(v) for v in f[4].split())
        assert len(x) == k and len(stored) == rows
        out.append((coeff, x, stored, (PR.CLEAN if a == NO_SLOT else a, PR.NONE if b == NO_SLOT else b)))
    return out


def test_python_reference_equals_the_cpp_rule(binary):
    """The planted cases the C++ program prints, through both forms of the Python reference."""
    cases = _cases(binary)
    assert len(cases) > 1000
    seen = set()
    for coeff, x, stored, want in cases:
        rows, k = coeff.shape
        assert PR.classify(coeff.tolist(), x, stored) == want, (k, rows, x, stored)
        ins = [np.array([v], dtype=np.uint32) for v in x]
        st = [np.array([v], dtype=np.uint32) for v in stored]
        a, b = PR.slots_of_object(coeff, ins, st)
        assert (int(a[0]), int(b[0])) == want, (k, rows, x, stored)
        a, b = want
        if b != PR.NONE:
            seen.add("pair of " + " and ".join("input" if s < k else "row" for s in (a, b)))
        else:
            seen.add("clean" if a == PR.CLEAN else "input" if a < k else "row" if a < k + rows else "unlocated")
    assert seen == {"clean", "input", "row", "unlocated", "pair of input and input", "pair of input and row",
                    "pair of row and row"}
    # the two codes that fill all 63 slots: every slot is named, and both say unlocated at slot 63
    for k, rows in ((59, 4), (3, 60)):
        named = set()
        for coeff, _, _, (a, b) in cases:
            if coeff.shape == (rows, k):
                named |= {a, b}
        assert named >= set(range(64)), (k, rows, sorted(set(range(64)) - named))
    # a plan of three rows answers as the one-shard rule does
    three = [(c, w) for c, _, _, w in cases if c.shape[0] == 3]
    assert three and all(w[1] == PR.NONE for _, w in three)


def test_reference_tally_counts_a_pair_for_both_slots():
    a = np.array([PR.CLEAN, 2, 5, 2, PR.CLEAN, 0, 6], dtype=np.int64)
    b = np.array([PR.NONE, 4, PR.NONE, PR.NONE, PR.NONE, 3, PR.NONE], dtype=np.int64)
    c, f = PR.tally((a, b), 7)
    assert c.tolist() == [1, 0, 2, 1, 1, 1, 1] and f.tolist() == [5, -1, 1, 5, 1, 2, 6]
    a2, b2 = PR.set_slots((a, b), 2, 4, 6)  # k = 2, four rows of a set's six: unlocated moves to slot 8
    assert a2.tolist() == [PR.CLEAN, 2, 5, 2, PR.CLEAN, 0, 8] and b2 is b


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
        twin = re.search(r"\b" + name.replace("_pairs", "") + r"\s*\(([^)]*)\)", text)
        assert " ".join(m.group(1).split()) == " ".join(twin.group(1).split()), "the argument list of its one-shard twin"


def test_calls_refuse_null_handles():
    a = np.zeros(8, dtype=np.uint64)
    p = a.ctypes.data  # any non-null address: the handles are checked first, nothing is read
    for name, nargs in CALLS.items():
        fn = getattr(N.lib, name)
        assert fn(*([None] * nargs)) == N.ERR_INVALID_ARG
        detail = N.lib.slime_rs_last_error().decode()
        what = name.replace("slime_rs_", "")
        assert detail == what + (": null set" if "planset" in name else ": null plan")
        assert fn(None, None, *([p] * (nargs - 3)), None) == N.ERR_INVALID_ARG


def test_header_states_the_pair_rule_and_keeps_the_one_shard_sentences():
    flat = " ".join(_header().split()).replace(" * ", " ")
    for phrase in ("pair locate", "exactly two d_i set", "adds 1 to counts of BOTH slots", "rows < 4",
                   "three or more wrong shards per column",
                   # the one-shard calls' sentences, still true of them
                   "correcting more than one wrong shard per column", "blamed on a third shard"):
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


def test_max_wrong_selects_the_pair_calls_after_the_same_checks(monkeypatch):
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
            p.locate_batch(buf, buf, _batch(rows, 8), max_wrong=bad)
        with pytest.raises(ValueError, match="max_wrong must be 1 or 2"):
            D.locate_objects_batch(p, chunks, chunks, _batch(rows, 8), mt, max_wrong=bad)
    with pytest.raises(ValueError, match="span 1 addresses element"):
        p.locate_batch(buf, buf[:-1].contiguous(), _batch(rows, 8), max_wrong=2)
    with pytest.raises(TypeError):
        p.locate_batch(buf.to(torch.int64), buf, _batch(rows, 8), max_wrong=2)
    with pytest.raises(ValueError, match="k=4"):
        p.locate_batch(buf, buf, _batch(rows, 4), max_wrong=2)
    with pytest.raises(ValueError, match="filter needs the 2 x 4"):
        p.locate_batch(buf, buf, _batch(rows, 8), filter=torch.zeros((2, 3), dtype=torch.int64), max_wrong=2)
    with pytest.raises(AssertionError, match="slime_rs_plan_locate_pairs_batch reached"):
        p.locate_batch(buf, buf, _batch(rows, 8), filter=torch.zeros((2, 4), dtype=torch.int64), max_wrong=2)
    with pytest.raises(AssertionError, match="slime_rs_plan_locate_batch reached"):
        p.locate_batch(buf, buf, _batch(rows, 8), max_wrong=1)
    c, f = p.locate_batch(buf, buf, _batch([], 8), max_wrong=2)  # no objects: no results, no C call
    assert c.shape == f.shape == (0, 13)
    with pytest.raises(ValueError, match="addresses element"):
        D.locate_objects_batch(p, chunks, chunks[:-4].contiguous(), _batch(rows, 8), mt, max_wrong=2)
    with pytest.raises(ValueError, match="mapping needs 2"):
        D.locate_objects_batch(p, chunks, chunks, _batch(rows, 8), mt[:1], max_wrong=2)
    with pytest.raises(AssertionError, match="slime_rs_locate_pairs_objects_batch reached"):
        D.locate_objects_batch(p, chunks, chunks, _batch(rows, 8), mt, max_wrong=2)
    with pytest.raises(AssertionError, match="slime_rs_locate_objects_batch reached"):
        D.locate_objects_batch(p, chunks, chunks, _batch(rows, 8), mt)
