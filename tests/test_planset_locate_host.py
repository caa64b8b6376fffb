"""Host-side checks of the plan-set locate (no GPU): the C++ program over the rule's plan-set
function (locate_rule.hpp, set_slot -- what the device runs), tests/planset_locate_ref.py pinned
to it on the cases the program prints, the two C entry points' signatures and refusal of null
handles, and the Python bookkeeping (PlanSet.locate_slots, erasures_from_set_counts, the checks
PlanSet.locate_batch makes before any C call)."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import planset_locate_ref as SR
from slime_amd import _native as N
from slime_amd import device as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "planset_locate_rule_test")
CALLS = {"slime_rs_planset_locate_batch": 8, "slime_rs_planset_locate_objects_batch": 9}


@pytest.fixture(scope="module")
def binary():
    subprocess.run(["make", "-C", ROOT, "tests/cpp/planset_locate_rule_test"], check=True, capture_output=True)
    return BIN


def test_set_slot_rule(binary):
    """set_slot / Column::slot_in_set against the brute-force statement: plans of 1 .. all parity
    rows of 3/5, 4/6 and 8/12 under every max_rows up to rows + 3."""
    r = subprocess.run([binary], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "planset_locate_rule_test ok" in r.stdout


def _cases(binary):
    r = subprocess.run([binary, "--cases"], capture_output=True, text=True, timeout=300, check=True)
    out = []
    for line in r.stdout.splitlines():
        f = line.split("|")
        if len(f) != 5:
            continue
        rows, k, max_rows = (int(v) for v in f[0].split())
        coeff = np.array(f[1].split(), dtype=np.uint64).astype(np.uint32).reshape(rows, k)
        x = [int(v) for v in f[2].split()]
        stored = [int(v) for v in f[3].split()]
        slot = int(f[4])
        assert len(x) == k and len(stored) == rows
        out.append((coeff, max_rows, x, stored, SR.CLEAN if slot == 0xFFFFFFFF else slot))
    return out


def test_python_reference_equals_the_cpp_rule(binary):
    """The planted cases the C++ program prints, through both forms of the Python reference."""
    cases = _cases(binary)
    assert len(cases) > 500
    seen = set()
    for coeff, max_rows, x, stored, slot in cases:
        rows, k = coeff.shape
        assert SR.classify(coeff.tolist(), x, stored, max_rows) == slot, (k, rows, max_rows, x, stored)
        ins = [np.array([v], dtype=np.uint32) for v in x]
        st = [np.array([v], dtype=np.uint32) for v in stored]
        assert SR.slots_of_object(coeff, ins, st, max_rows)[0] == slot, (k, rows, max_rows, x, stored)
        assert slot == SR.CLEAN or slot < k + rows or slot == k + max_rows, "never a slot past the plan's rows"
        kind = "clean" if slot == SR.CLEAN else "input" if slot < k else "row" if slot < k + rows else "unlocated"
        seen.add((kind, "one row" if rows < 2 else "wider" if max_rows > rows else "widest"))
    for width in ("wider", "widest"):
        assert {(kind, width) for kind in ("clean", "input", "row", "unlocated")} <= seen
    assert {k for k, w in seen if w == "one row"} == {"clean", "unlocated"}


def test_set_slot_in_words():
    k = 8
    assert SR.set_slot(SR.CLEAN, k, 1, 4) == SR.CLEAN
    assert SR.set_slot(k + 0, k, 1, 4) == k + 4  # one row: its only row's slot is not an answer
    assert SR.set_slot(3, k, 2, 4) == 3 and SR.set_slot(k + 1, k, 2, 4) == k + 1
    assert SR.set_slot(k + 2, k, 2, 4) == k + 4  # the plan's own `unlocated` moves to the set's column
    assert SR.set_slot(k + 4, k, 4, 4) == k + 4


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
        assert "slime_rs_planset_t set" in m.group(1)


def test_calls_refuse_null_handles():
    a = np.zeros(8, dtype=np.uint64)
    p = a.ctypes.data  # any non-null address: the handles are checked first, nothing is read
    for name, nargs in CALLS.items():
        fn = getattr(N.lib, name)
        assert fn(*([None] * nargs)) == N.ERR_INVALID_ARG
        detail = N.lib.slime_rs_last_error().decode()
        assert detail == name.replace("slime_rs_", "") + ": null set"
        assert fn(None, None, *([p] * (nargs - 3)), None) == N.ERR_INVALID_ARG


def test_header_describes_plan_set_locate():
    flat = " ".join(_header().split()).replace(" * ", " ")
    for phrase in ("`unlocated` is ALWAYS slot k + max_rows", "rows_o < 2 reports every mismatching column as unlocated",
                   "max_rows < 2 (no object of the set could be located)", "k + max_rows > 63"):
        assert phrase in flat, phrase
    single = flat[flat.index("ragged locate: name the corrupt shards"):flat.index("plan-set locate: name the corrupt")]
    assert "plan-set locate, matrix-core" not in single, "no longer listed as out of scope"


def _set(members, k):
    """A PlanSet's host bookkeeping without a device: members = [(in shards, out shards, rows)]."""
    s = D.PlanSet.__new__(D.PlanSet)
    s._h, s.device, s.k, s.nplans = None, 0, k, len(members)
    s.max_rows = max(m[2] for m in members)
    s.in_max = max(max(m[0]) for m in members if m[0] is not None)
    s.out_max = max(max(m[1]) for m in members)
    s._members = members
    return s


def test_locate_slots_and_erasures_from_set_counts():
    # 3/5: all present; shard 1 missing (one row left); shard 4 missing; unknown inputs
    s = _set([([0, 1, 2], [3, 4], 2), ([0, 2, 3], [4], 1), ([0, 1, 2], [3], 1), (None, [0, 1], 2)], 3)
    assert s.locate_slots(0) == [0, 1, 2, 3, 4]
    assert s.locate_slots(1) == [0, 2, 3, 4, None]
    assert s.locate_slots(2) == [0, 1, 2, 3, None]
    with pytest.raises(ValueError, match="plan 3's input shards are unknown"):
        s.locate_slots(3)
    plan_of = np.array([0, 1, N.NO_PLAN, 0, 1, 2], dtype=np.uint32)
    missing = [(), (1,), (3, 4), None, [1], (4,)]
    counts = np.array([[0, 2, 0, 0, 1, 0],    # inputs 1 and row 1 -> shards 1, 4
                       [0, 0, 0, 0, 0, 9],    # a one-row object: only unlocated, which names nothing
                       [0, 0, 0, 0, 0, 0],    # no plan: just what it misses
                       [0, 0, 0, 0, 0, 0],    # clean
                       [0, 1, 0, 0, 0, 0],    # plan 1's input 1 is shard 2
                       [0, 0, 0, 1, 0, 0]])   # plan 2's row 0 is shard 3
    want = [[1, 4], [1], [3, 4], [], [1, 2], [3, 4]]
    assert D.erasures_from_set_counts(counts, s, plan_of, missing) == want
    assert D.erasures_from_set_counts(torch.from_numpy(counts), s, plan_of, missing) == want
    assert D.erasures_from_set_counts(counts, s, plan_of) == [[1, 4], [], [], [], [2], [3]]
    with pytest.raises(ValueError, match="shape"):
        D.erasures_from_set_counts(counts[:, :5], s, plan_of)
    with pytest.raises(ValueError, match="shape"):
        D.erasures_from_set_counts(counts[:5], s, plan_of)
    with pytest.raises(ValueError, match="one entry per object"):
        D.erasures_from_set_counts(counts, s, plan_of, missing[:3])
    bad = counts.copy()
    bad[1, 4] = 1  # a slot past the plan's rows never counts
    with pytest.raises(ValueError, match="past its plan's rows"):
        D.erasures_from_set_counts(bad, s, plan_of)
    bad = counts.copy()
    bad[2, 0] = 1
    with pytest.raises(ValueError, match="no plan"):
        D.erasures_from_set_counts(bad, s, plan_of)


def test_for_scrub_refuses_before_any_plan_is_built(monkeypatch):
    class NoPlans:
        @staticmethod
        def reconstruct(*a, **k):
            raise AssertionError("a plan was built")

    monkeypatch.setattr(D, "Plan", NoPlans)
    with pytest.raises(ValueError, match="fewer than 3 of 5"):
        D.PlanSet.for_scrub(3, 5, [(), (0, 1, 2)])
    with pytest.raises(ValueError, match="not shards"):
        D.PlanSet.for_scrub(3, 5, [(5,)])
    with pytest.raises(ValueError, match="nothing to scrub"):
        D.PlanSet.for_scrub(3, 5, [(0, 1), (3, 4)])
    with pytest.raises(AssertionError, match="a plan was built"):
        D.PlanSet.for_scrub(3, 5, [(0, 1), None])


class _NoCalls:
    """Stands in for the native library: any C call fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"C call {name} reached")


def _batch(rows, k, plans=None, nplans=None, device=0):
    b = D.Batch.__new__(D.Batch)
    b._h, b.k, b.device, b._extents = None, k, device, {}
    b.spans = np.asarray(rows, dtype=np.uint64).reshape(-1, 5)
    b.nobj = len(b.spans)
    b.plans = None if plans is None else np.asarray(plans, dtype=np.uint32)
    b.nplans = nplans
    return b


def test_locate_batch_runs_verify_batchs_checks_first(monkeypatch):
    monkeypatch.setattr(D, "lib", _NoCalls())
    monkeypatch.setattr(D, "_dev_index", lambda t: 0)
    monkeypatch.setattr(D, "_verify_results", lambda nobj, rows, device: (torch.empty((nobj, rows), dtype=torch.int64),
                                                                         torch.empty((nobj, rows), dtype=torch.int64)))
    s = _set([(list(range(8)), [8, 9, 10, 11], 4), ([1, 2, 3, 4, 5, 6, 7, 8], [9, 11], 2)], 8)
    rows = [(0, 100, 0, 100, 100), (1200, 7, 1200, 7, 7)]
    buf = torch.zeros(1200 + 12 * 7, dtype=torch.int32)
    planned = lambda: _batch(rows, 8, plans=[0, 1], nplans=2)  # noqa: E731
    with pytest.raises(ValueError, match="span 1 addresses element"):
        s.locate_batch(buf, buf[:-1].contiguous(), planned())
    with pytest.raises(ValueError, match="addresses element"):
        s.locate_batch(buf, buf, planned(), cmp_offset=1)
    with pytest.raises(TypeError):
        s.locate_batch(buf.to(torch.int64), buf, planned())
    with pytest.raises(ValueError, match="carries no plan indices"):
        s.locate_batch(buf, buf, _batch(rows, 8))
    with pytest.raises(ValueError, match="batch is for 3 plans"):
        s.locate_batch(buf, buf, _batch(rows, 8, plans=[0, 1], nplans=3))
    with pytest.raises(ValueError, match="filter needs the 2 x 4"):
        s.locate_batch(buf, buf, planned(), filter=torch.zeros((2, 2), dtype=torch.int64))
    with pytest.raises(ValueError, match="filter needs"):
        s.locate_batch(buf, buf, planned(), filter=torch.zeros((2, 4), dtype=torch.int32))
    with pytest.raises(AssertionError, match="slime_rs_planset_locate_batch reached"):
        s.locate_batch(buf, buf, planned(), filter=torch.zeros((2, 4), dtype=torch.int64))
    c, f = s.locate_batch(buf, buf, _batch([], 8, plans=[], nplans=2))  # no objects: no results, no C call
    assert c.shape == f.shape == (0, 13)
    chunks = torch.zeros(4 * len(buf), dtype=torch.uint8)
    mt = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="addresses element"):
        D.locate_objects_batch(s, chunks, chunks[:-4].contiguous(), planned(), mt)
    with pytest.raises(ValueError, match="carries no plan indices"):
        D.locate_objects_batch(s, chunks, chunks, _batch(rows, 8), mt)
    with pytest.raises(ValueError, match="filter needs the 2 x 4"):
        D.locate_objects_batch(s, chunks, chunks, planned(), mt, filter=torch.zeros((2, 2), dtype=torch.int64))
    with pytest.raises(AssertionError, match="slime_rs_planset_locate_objects_batch reached"):
        D.locate_objects_batch(s, chunks, chunks, planned(), mt)
    c, f = D.locate_objects_batch(s, chunks, chunks, _batch([], 8, plans=[], nplans=2), mt)
    assert c.shape == f.shape == (0, 13)
