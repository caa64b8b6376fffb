"""Plan-set verify (slime_rs_planset_verify_batch) on the GPU: one launch that checks every
object of a planned batch against its own plan -- the result of a repair sweep, or degraded
objects scrubbed from a different survivor set each.

The repaired contents are the oracle's (test_gpu_planset.repair_case: codewords encoded by the C
oracle, erased shards rebuilt on the host by OC.apply_matrix over each plan's rows) -- never
PlanSet.execute_batch's; planted flips are reported where they were planted, and the wide-row
expectations are OC.apply_matrix against the host copy.  Result arrays are pre-filled with
garbage, and data buffers are compared with their host copies afterwards.
"""
import ctypes

import numpy as np
import pytest

from oracle import oracle_c as OC
from slime_amd import _native as N
from test_gpu_planset import PATTERNS, cycle, make_set, planned_batch, repair_case
from test_gpu_ragged import (P, SENTINEL, boundary_lengths, geometry, mode, packed_spans, shard, to_dev,  # noqa: F401
                             to_host, torch_dev)
from test_gpu_ragged_verify import (assert_results, clean_results, expect_batch, flip_positions, host,
                                    verify_lengths)
from test_gpu_verify import GARBAGE

pytestmark = pytest.mark.gpu


def raw_set_verify(torch, pset, batch, src, cmp, stream=None):
    """slime_rs_planset_verify_batch into result arrays pre-filled with garbage."""
    from slime_amd import device as D
    mism = torch.full((batch.nobj, pset.max_rows), GARBAGE, dtype=torch.int64, device="cuda")
    first = torch.full((batch.nobj, pset.max_rows), GARBAGE, dtype=torch.int64, device="cuda")
    N.check(N.lib.slime_rs_planset_verify_batch(pset._h, batch._h, ctypes.c_void_p(src.data_ptr()),
                                                ctypes.c_void_p(cmp.data_ptr()), ctypes.c_void_p(mism.data_ptr()),
                                                ctypes.c_void_p(first.data_ptr()), D._stream_handle(0, stream)))
    return mism, first


def planted(lengths, pats, places, want, max_rows, k, pick=0):
    """A copy of `want` with one flipped word in one rebuilt shard of every repaired object, and the
    results that must come back: that (object, row) only."""
    h = want.copy()
    em, ef = clean_results(len(lengths), max_rows)
    for o, (L, pat) in enumerate(zip(lengths, pats)):
        q = flip_positions(L, k, max_rows)
        if pat and q:
            i, c = (o + pick) % len(pat), q[(o + pick) % len(q)]
            shard(h, places[o], sorted(pat)[i], L)[c] ^= np.uint32(1 << (o % 32))
            em[o, i], ef[o, i] = 1, c
    return h, (em, ef)


# ------------------------------------------------------------------ clean after repair, attribution

@pytest.mark.parametrize("align", [1, 64])
@pytest.mark.parametrize("need,total", [(3, 5), (8, 12), (16, 20), (17, 20)])
def test_clean_after_repair_and_attribution(torch_dev, mode, need, total, align):
    """Objects at every boundary length and step boundary, each with its own erasure pattern (1, 2
    and total - need rows) or intact, holding what the oracle's repair leaves: all results clean;
    rows at or past a plan's own row count and NO_PLAN objects hold their initial values whatever
    the slots hold.  Then one flipped word in one rebuilt shard of each object is reported at that
    (object, row) only."""
    torch = torch_dev
    allp = PATTERNS[(need, total)]
    max_rows = max(len(p) for p in allp)
    lengths = verify_lengths(need, max_rows)
    np.random.default_rng(need * 41 + total).shuffle(lengths)
    pats = [None if o % 5 == 3 else allp[o % len(allp)] for o in range(len(lengths))]
    assert {len(p) for p in pats if p} >= {1, 2, total - need}
    _, want, places, _ = repair_case(need, total, lengths, pats, align, seed=need * 3001 + total)
    pset, plan_of = make_set(need, total, pats)
    batch = planned_batch(lengths, places, need, plan_of, pset.nplans)
    buf = to_dev(torch, want)
    assert_results(host(torch, raw_set_verify(torch, pset, batch, buf, buf)), clean_results(len(lengths), max_rows))
    m, f = pset.verify_batch(buf, buf, batch)
    assert m.shape == f.shape == (len(lengths), pset.max_rows)
    assert_results(host(torch, (m, f)), clean_results(len(lengths), max_rows))
    assert np.array_equal(to_host(torch, buf), want), "verify writes nothing but its results"
    for pick in (0, 1):
        h, exp = planted(lengths, pats, places, want, max_rows, need, pick)
        # an intact object's slots may hold anything: it is not looked at
        for o, pat in enumerate(pats):
            if pat is None and lengths[o]:
                shard(h, places[o], total - 1, lengths[o])[0] ^= np.uint32(1)
        hb = to_dev(torch, h)
        assert_results(host(torch, raw_set_verify(torch, pset, batch, hb, hb)), exp, pick)


# ------------------------------------------------------------------ the pipeline across plans

@pytest.mark.parametrize("need,total", [(3, 5), (8, 12), (16, 20)])
def test_every_pipelined_step_crosses_plans(torch_dev, mode, need, total):
    """Twelve objects of exactly one tile whose plans cycle through patterns of 1, 2 and
    total - need rows; object o has o + 1 flipped words in its plan's row o % rows_o.  Whenever a
    wave takes two units in a row, the step it compares and the step it loads belong to different
    plans: a compare that read the walk's current plan uses the wrong rows and outputs."""
    torch = torch_dev
    T, _ = geometry(need)
    allp = PATTERNS[(need, total)]
    lengths, pats = [T] * 12, cycle(allp, 12)
    assert {len(p) for p in pats} >= {1, 2, total - need}
    max_rows = max(len(p) for p in pats)
    _, want, places, _ = repair_case(need, total, lengths, pats, 64, seed=1200 + need)
    h = want.copy()
    em, ef = clean_results(12, max_rows)
    rng = np.random.default_rng(need)
    for o, pat in enumerate(pats):
        i = o % len(pat)
        cols = np.sort(rng.choice(T, size=o + 1, replace=False))
        shard(h, places[o], sorted(pat)[i], T)[cols] ^= np.uint32(0x200)
        em[o, i], ef[o, i] = o + 1, cols[0]
    pset, plan_of = make_set(need, total, pats)
    batch = planned_batch(lengths, places, need, plan_of, pset.nplans)
    buf = to_dev(torch, h)
    assert_results(host(torch, raw_set_verify(torch, pset, batch, buf, buf)), (em, ef))


@pytest.mark.parametrize("need,total,nobj", [(3, 5, 1100), (8, 12, 1100), (16, 20, 4200)])
def test_waves_walk_units_of_different_plans(torch_dev, mode, need, total, nobj):
    """More one-unit objects (4 to 9 columns) than the static grid has waves, plans cycling with a
    period that divides neither grid: every wave that takes a second unit compares a step of one
    plan after issuing the loads of a step of another.  Object o has one flipped word in its
    plan's row o % rows_o at column o % 4."""
    torch = torch_dev
    allp = PATTERNS[(need, total)]
    assert 1024 % len(allp) and 4096 % len(allp) and nobj > (4096 if need > 12 else 1024)
    lengths = [4 + o % 6 for o in range(nobj)]
    pats = cycle(allp, nobj)
    max_rows = max(len(p) for p in allp)
    _, want, places, _ = repair_case(need, total, lengths, pats, 1, seed=77 + need)
    h = want.copy()
    em, ef = clean_results(nobj, max_rows)
    for o, pat in enumerate(pats):
        i = o % len(pat)
        shard(h, places[o], sorted(pat)[i], lengths[o])[o % 4] ^= np.uint32(2)
        em[o, i], ef[o, i] = 1, o % 4
    pset, plan_of = make_set(need, total, pats)
    batch = planned_batch(lengths, places, need, plan_of, pset.nplans)
    buf = to_dev(torch, h)
    assert_results(host(torch, raw_set_verify(torch, pset, batch, buf, buf)), (em, ef))


# ------------------------------------------------------------------ more than 64 rows in a set

def test_a_70_row_plan_beside_a_2_row_plan(torch_dev, mode):
    """Two row blocks: the 2-row plan's units have no row in the second and do no loads there; its
    rows 2..69 keep their initial values."""
    torch = torch_dev
    from slime_amd import device as D
    k, wide, L = 3, 70, 1031
    lengths = [L, 5, L - 4, 0, 257, 2 * 1024 + 3]
    which = [0, 1, 1, 0, N.NO_PLAN, 0]
    rng = np.random.default_rng(70)
    coeffs = [rng.integers(1, P, size=(r, k), dtype=np.uint64).astype(np.uint32) for r in (wide, 2)]
    src_places, ssize = packed_spans(lengths, k, 1, start=3)
    cmp_places, csize = packed_spans(lengths, wide, 1, start=5)  # every object has room for 70 stored rows
    src_h = np.full(ssize + 4, SENTINEL, dtype=np.uint32)
    cmp_h = np.full(csize + 4, SENTINEL, dtype=np.uint32)
    for sp, cp, n, w in zip(src_places, cmp_places, lengths, which):
        if n and w != N.NO_PLAN:
            x = rng.integers(0, 2**32, size=(k, n), dtype=np.uint64).astype(np.uint32)
            for j in range(k):
                shard(src_h, sp, j, n)[:] = x[j]
            for i, r in enumerate(OC.apply_matrix(coeffs[w], list(x))):
                shard(cmp_h, cp, i, n)[:] = r
    plans = [D.Plan.matrix(c, list(range(k))) for c in coeffs]
    pset = D.PlanSet(plans)
    assert (pset.nplans, pset.max_rows, pset.out_max) == (2, wide, wide - 1)
    batch = D.Batch([(so, ss, do, ds, n) for (so, ss), (do, ds), n in zip(src_places, cmp_places, lengths)], k,
                    plans=which, nplans=2)
    src = to_dev(torch, src_h)
    assert_results(host(torch, raw_set_verify(torch, pset, batch, src, to_dev(torch, cmp_h))),
                   clean_results(len(lengths), wide))
    h = cmp_h.copy()
    for o, i, c in ((0, 0, 1), (0, 63, L - 1), (0, 64, 0), (0, 69, L - 2), (5, 64, 2 * 1024), (5, 65, 2 * 1024 + 2),
                    (1, 1, 4), (2, 0, L - 5), (2, 1, 0)):
        shard(h, cmp_places[o], i, lengths[o])[c] ^= np.uint32(0x20)
    shard(h, cmp_places[5], 68, lengths[5])[:] ^= np.uint32(1)  # a whole row of the second block
    em, ef = clean_results(len(lengths), wide)
    for o, w in enumerate(which):
        if w != N.NO_PLAN and lengths[o]:
            r = len(coeffs[w])
            m1, f1 = expect_batch(coeffs[w], list(range(k)), list(range(r)), src_h, src_places[o:o + 1], h,
                                  cmp_places[o:o + 1], lengths[o:o + 1])
            em[o, :r], ef[o, :r] = m1[0], f1[0]
    assert em[5, 68] == lengths[5] and em.sum() == lengths[5] + 9 and not em[1, 2:].any()
    assert_results(host(torch, raw_set_verify(torch, pset, batch, src, to_dev(torch, h))), (em, ef))


# ------------------------------------------------------------------ refusals

def test_refusals(torch_dev):
    torch = torch_dev
    from slime_amd import device as D
    need, total = 8, 12
    lengths, pats = [100, 7], [(0,), (2, 5)]
    _, want, places, _ = repair_case(need, total, lengths, pats, 1, seed=1)
    pset, plan_of = make_set(need, total, pats)
    batch = planned_batch(lengths, places, need, plan_of, 2)
    buf = to_dev(torch, want)
    res = torch.full((4,), GARBAGE, dtype=torch.int64, device="cuda")
    p, r = ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(res.data_ptr())

    def refused(set_h, batch_h, *rest):
        args = rest or (p, p, r, r)
        assert N.lib.slime_rs_planset_verify_batch(set_h, batch_h, *args, None) == N.ERR_INVALID_ARG
        assert "planset_verify_batch" in N.lib.slime_rs_last_error().decode()

    refused(None, batch._h)
    refused(pset._h, None)
    for args in ((None, p, r, r), (p, None, r, r), (p, p, None, r), (p, p, r, None)):
        refused(pset._h, batch._h, *args)
    unplanned = D.Batch([(o, s, o, s, L) for (o, s), L in zip(places, lengths)], need)
    refused(pset._h, unplanned._h)
    with pytest.raises(ValueError, match="no plan indices"):
        pset.verify_batch(buf, buf, unplanned)
    three = planned_batch(lengths, places, need, plan_of, 3)  # another nplans
    refused(pset._h, three._h)
    with pytest.raises(ValueError, match="3 plans"):
        pset.verify_batch(buf, buf, three)
    other_k = planned_batch(lengths, places, need - 1, plan_of, 2)
    refused(pset._h, other_k._h)
    with pytest.raises(ValueError, match="k=7"):
        pset.verify_batch(buf, buf, other_k)
    with pytest.raises(ValueError, match="addresses element"):
        pset.verify_batch(buf, buf[:-48].contiguous(), batch)  # ends inside shard 5 of the last object
    torch.cuda.synchronize()
    assert (res == GARBAGE).all(), "a refused call touches nothing"
    assert_results(host(torch, pset.verify_batch(buf, buf, batch)), clean_results(2, 2))


# ------------------------------------------------------------------ graph capture, dynamic schedule

def test_graph_capture_at_schedule_2(torch_dev):
    """The captured set verify takes the dynamic schedule with a counter set held by the graph;
    two replays with a word flipped in between: the second starts clean and shows only the new
    state."""
    torch = torch_dev
    need, total = 4, 6
    s0 = N.lib.slime_rs_kernel_schedule(-1)
    assert N.lib.slime_rs_kernel_schedule(2) == 0
    try:
        T, C = geometry(need)
        lengths = [4 * C * T + 5, 3, T + 1, 0, 256, C * T] * 2
        pats = cycle(PATTERNS[(need, total)], len(lengths))
        _, want, places, _ = repair_case(need, total, lengths, pats, 1, seed=31)
        pset, plan_of = make_set(need, total, pats)
        batch = planned_batch(lengths, places, need, plan_of, pset.nplans)
        h = want.copy()
        shard(h, places[0], sorted(pats[0])[0], lengths[0])[T] ^= np.uint32(8)
        buf = to_dev(torch, h)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):  # warm the launch path outside the capture
            pset.verify_batch(buf, buf, batch, stream=s)
        torch.cuda.synchronize()
        _, held0 = N.ticket_sets(0)
        dyn0, _ = N.schedule_counts(0)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            gm, gf_ = pset.verify_batch(buf, buf, batch, stream=s)
        torch.cuda.synchronize()
        assert (N.ticket_sets(0)[1] - held0, N.schedule_counts(0)[0] - dyn0) == (1, 1)
        gm.fill_(GARBAGE)
        gf_.fill_(GARBAGE)
        torch.cuda.synchronize()
        g.replay()
        em, ef = clean_results(len(lengths), pset.max_rows)
        em[0, 0], ef[0, 0] = 1, T
        assert_results(host(torch, (gm, gf_)), (em, ef))
        h2 = want.copy()
        last = len(lengths) - 1
        i = len(pats[last]) - 1
        shard(h2, places[last], sorted(pats[last])[i], lengths[last])[[7, 300]] ^= np.uint32(8)
        buf.copy_(to_dev(torch, h2))
        torch.cuda.synchronize()
        g.replay()
        em, ef = clean_results(len(lengths), pset.max_rows)
        em[last, i], ef[last, i] = 2, 7
        assert_results(host(torch, (gm, gf_)), (em, ef))
        del g  # before the batch and the set: the graph's kernel nodes read their tables
        torch.cuda.synchronize()
    finally:
        N.lib.slime_rs_kernel_schedule(s0)
