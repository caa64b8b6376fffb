"""Plan sets (slime_rs_planset_create, slime_rs_batch_create_planned,
slime_rs_planset_execute_batch) on the GPU: one launch that repairs objects
with different erasure patterns.

Every expectation comes from the C oracle: objects are oracle-encoded
codewords, and each erased shard is expected to be OC.apply_matrix of its
plan's coefficient rows on the plan's survivors (checked against the oracle's
codeword: rebuilt parity rows equal it, rebuilt data rows are its canonical
residues, so a planted word >= p in an erased data shard comes back reduced,
as the reference's RecoverData gives it).  Before the launch the erased slots
hold a second sentinel, so a kernel that reads an erased shard as an input
fails; whole buffers are compared, guard words, shard padding and untouched
objects included.  References are computed once per shape and shared by the
schedule / pipeline modes (the fixture of test_gpu_ragged.py).
"""
import ctypes

import numpy as np
import pytest

import steering as ST
from oracle import oracle_c as OC
from slime_amd import _native as N
from test_gpu_ragged import (P, SENTINEL, boundary_lengths, geometry, mode, packed_spans, shard,  # noqa: F401
                             symbols, to_dev, to_host, torch_dev)

pytestmark = pytest.mark.gpu

ERASED = 0xE7A5ED00  # what an erased slot holds before the repair (>= p: never a canonical result)

# Erasure patterns by code: one, two and total - need rows, data and parity targets.
PATTERNS = {
    (3, 5): [(0,), (4,), (1, 3), (0, 1), (3, 4), (2,)],
    (4, 6): [(a,) for a in range(6)] + [(a, b) for a in range(6) for b in range(a + 1, 6)],  # all 6 + all 15
    (8, 12): [(0,), (11,), (2, 5), (0, 3, 8, 11), (0, 1, 2, 3), (8, 9, 10, 11)],
    (16, 20): [(0,), (19,), (7, 16), (0, 5, 16, 19), (0, 1, 2, 3), (16, 17, 18, 19)],
    (17, 20): [(0,), (19,), (3, 18), (0, 16, 19), (17, 18, 19)],
    (33, 50): [(0,), (49,), (5, 40), tuple(range(17)), tuple(range(33, 50)), (0, 9, 32, 33, 49)],
}


def survivors(need, total, pat):
    return [i for i in range(total) if i not in pat][:need]


_rows = {}


def plan_rows(need, total, pat):
    """The reconstruct plan's coefficient rows for one pattern (host matrix code, no kernel)."""
    from slime_amd import device as D
    key = (need, total, tuple(pat))
    if key not in _rows:
        plan = D.Plan.reconstruct(need, total, survivors(need, total, pat), list(pat))
        _rows[key] = plan.coefficients()
        plan.close()
    return _rows[key]


def rebuilt(need, total, pat, word):
    """The oracle's values of the erased shards of one codeword (total x L), from the survivors alone."""
    have = survivors(need, total, pat)
    out = OC.apply_matrix(plan_rows(need, total, pat), [np.ascontiguousarray(word[s]) for s in have])
    for r, t in zip(out, pat):
        assert np.array_equal(r, word[t] % np.uint32(P) if t < need else word[t]), "the rows rebuild the codeword"
    return out


_cases = {}


def repair_case(need, total, lengths, patterns, align, seed):
    """(init, want, places, size).  init: a sentinel-filled packed buffer of oracle-encoded
    codewords whose erased shards (patterns[o], None = intact) hold ERASED; want: the same buffer
    with every erased shard as the oracle rebuilds it.  Cached, read-only."""
    key = (need, total, tuple(lengths), tuple(patterns), align, seed)
    if key not in _cases:
        rng = np.random.default_rng(seed)
        places, size = packed_spans(lengths, total, align, start=3 if align == 1 else 64)
        init = np.full(size + 5, SENTINEL, dtype=np.uint32)
        want = init.copy()
        for place, L, pat in zip(places, lengths, patterns):
            word = np.zeros((total, L), dtype=np.uint32)
            word[:need] = symbols(rng, (need, L))  # non-canonical data words too
            if L:
                OC.encode_object(word, need, total)
            fixed = rebuilt(need, total, pat, word) if pat and L else []
            for s in range(total):
                shard(init, place, s, L)[:] = ERASED if pat and s in pat else word[s]
                shard(want, place, s, L)[:] = fixed[pat.index(s)] if pat and s in pat and L else word[s]
        init.setflags(write=False)
        want.setflags(write=False)
        _cases[key] = (init, want, places, size + 5)
    return _cases[key]


def make_set(need, total, patterns):
    from slime_amd import device as D
    pset, plan_of = D.PlanSet.for_erasures(need, total, [p or () for p in patterns])
    distinct = []
    for p in patterns:
        if p and tuple(sorted(p)) not in distinct:
            distinct.append(tuple(sorted(p)))
    assert pset.nplans == len(distinct) and pset.k == need
    assert pset.max_rows == max(len(p) for p in distinct)
    assert pset.out_max == max(max(p) for p in distinct)
    assert pset.in_max == max(max(survivors(need, total, p)) for p in distinct)
    assert [int(x) for x in plan_of] == [distinct.index(tuple(sorted(p))) if p else N.NO_PLAN for p in patterns]
    return pset, plan_of


def planned_batch(lengths, places, k, plan_of, nplans, dst_places=None):
    from slime_amd import device as D
    dst_places = dst_places or places
    return D.Batch([(so, ss, do, ds, L) for (so, ss), (do, ds), L in zip(places, dst_places, lengths)], k,
                   plans=plan_of, nplans=nplans)


def assert_equal(got, want):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad.size, bad[:8], got[bad[:8]], want[bad[:8]])


def run_repair(torch, need, total, lengths, patterns, align, seed, stream=None):
    init, want, places, _ = repair_case(need, total, lengths, patterns, align, seed)
    pset, plan_of = make_set(need, total, patterns)
    batch = planned_batch(lengths, places, need, plan_of, pset.nplans)
    assert batch.nobj == len(lengths)
    assert batch.columns == sum(L for L, p in zip(lengths, patterns) if p)
    buf = to_dev(torch, init)
    pset.execute_batch(buf, buf, batch, stream=stream)
    assert_equal(to_host(torch, buf), want)
    return pset, batch


def cycle(pats, n):
    return [pats[i % len(pats)] for i in range(n)]


# ------------------------------------------------------------------ the pipeline across plans

@pytest.mark.parametrize("need,total", [(3, 5), (8, 12), (16, 20)])
def test_every_pipelined_step_crosses_plans(torch_dev, mode, need, total):
    """Twelve objects of exactly one tile whose plans cycle through patterns of 1, 2 and
    total - need rows: whenever a wave takes two units in a row, the tile it stores and the tile
    it loads belong to different plans with different row counts and outputs."""
    T, _ = geometry(need)
    pats = PATTERNS[(need, total)]
    assert {len(p) for p in pats} >= {1, 2, total - need}
    run_repair(torch_dev, need, total, [T] * 12, cycle(pats, 12), 64, seed=1200 + need)


@pytest.mark.parametrize("need,total,nobj", [(3, 5, 1500), (8, 12, 1500), (16, 20, 5000)])
def test_waves_walk_units_of_different_plans(torch_dev, mode, need, total, nobj):
    """More one-unit objects than the largest grid has waves (1024; 4096 for k > 12), of 4 to 9
    columns, plans cycling: on the static walk wave w takes units w, w + nwaves, ..., and neither
    grid is a multiple of the patterns' period, so EVERY wave that takes a second unit stores a
    tile of one plan after issuing the loads of a tile of another.  A store that used the
    walk's current plan instead of its own tile's fails here in every mode."""
    pats = PATTERNS[(need, total)]
    assert 1024 % len(pats) and 4096 % len(pats) and nobj > (4096 if need > 12 else 1024)
    lengths = [4 + o % 6 for o in range(nobj)]
    run_repair(torch_dev, need, total, lengths, cycle(pats, nobj), 1, seed=77 + need)


# ------------------------------------------------------------------ lengths, alignments, guard words

@pytest.mark.parametrize("align", [1, 64])
@pytest.mark.parametrize("need,total", sorted(PATTERNS))
def test_every_boundary_length_repaired_in_place(torch_dev, mode, need, total, align):
    """Objects at every boundary length (4/6: twice over, so that all 15 two-erasure and all 6
    one-erasure patterns are in one batch), plans round-robin, repaired in place; 17/20 and 33/50
    take the column form.  The whole buffer is compared."""
    pats = PATTERNS[(need, total)]
    lengths = boundary_lengths(need) * (2 if (need, total) == (4, 6) else 1)
    np.random.default_rng(need * 17 + total).shuffle(lengths)
    assert len(lengths) >= len(pats)
    run_repair(torch_dev, need, total, lengths, cycle(pats, len(lengths)), align, seed=need * 1013 + total)


def test_intact_objects_are_left_alone(torch_dev, mode):
    """NO_PLAN objects interleaved with planned ones: no unit, no tail, their bytes unchanged."""
    need, total = 8, 12
    lengths = boundary_lengths(need)
    pats = [None if o % 3 == 1 else PATTERNS[(need, total)][o % 6] for o in range(len(lengths))]
    _, batch = run_repair(torch_dev, need, total, lengths, pats, 1, seed=31)
    plain = planned_batch(lengths, repair_case(need, total, lengths, pats, 1, 31)[2], need,
                          [0] * len(lengths), 1)
    assert batch.units < plain.units and batch.columns < plain.columns


def test_planned_batch_through_the_single_plan_launch(torch_dev, mode):
    """Plan.execute_batch over a planned batch: the indices are ignored (every planned object gets
    the one plan), NO_PLAN objects are skipped."""
    torch = torch_dev
    from slime_amd import device as D
    need, total, pat = 8, 12, (2, 5)
    lengths = [769, 5, 0, 3 * 768 + 1, 256, 4]
    pats = [pat, None, pat, pat, None, pat]
    init, want, places, _ = repair_case(need, total, lengths, pats, 1, seed=58)
    plan_of = [2, N.NO_PLAN, 0, 1, N.NO_PLAN, 2]  # indices of some three-plan set: not looked at
    batch = planned_batch(lengths, places, need, plan_of, 3)
    plan = D.Plan.reconstruct(need, total, survivors(need, total, pat), list(pat)).set_outputs(list(pat))
    buf = to_dev(torch, init)
    plan.execute_batch(buf, buf, batch)
    assert_equal(to_host(torch, buf), want)


@pytest.mark.parametrize("need,total", [(3, 5), (8, 12), (17, 20)])
def test_a_set_of_one_plan_equals_the_single_plan_launch(torch_dev, mode, need, total):
    torch = torch_dev
    from slime_amd import device as D
    pat = PATTERNS[(need, total)][3]
    lengths = boundary_lengths(need)
    pats = [pat] * len(lengths)
    init, want, places, _ = repair_case(need, total, lengths, pats, 1, seed=90 + need)
    plan = D.Plan.reconstruct(need, total, survivors(need, total, pat), list(pat)).set_outputs(list(pat))
    pset = D.PlanSet([plan])
    assert (pset.nplans, pset.max_rows, pset.in_max, pset.out_max) == (1, len(pat), plan.in_max, max(pat))
    a, b = to_dev(torch, init), to_dev(torch, init)
    pset.execute_batch(a, a, planned_batch(lengths, places, need, [0] * len(lengths), 1))
    plan.execute_batch(b, b, D.Batch([(o, s, o, s, L) for (o, s), L in zip(places, lengths)], need))
    ga, gb = to_host(torch, a), to_host(torch, b)
    assert np.array_equal(ga, gb)
    assert_equal(ga, want)


def test_a_set_is_a_snapshot_of_its_plans(torch_dev):
    """Outputs are those set before the set was made; a later set_outputs on a member, and
    destroying the members, do not reach it; making the set does not mark a plan launched."""
    torch = torch_dev
    from slime_amd import device as D
    need, total = 3, 5
    lengths, pats = [1025, 7], [(1, 3), (4,)]
    init, want, places, _ = repair_case(need, total, lengths, pats, 1, seed=5)
    plans = [D.Plan.reconstruct(need, total, survivors(need, total, p), list(p)).set_outputs(list(p)) for p in pats]
    pset = D.PlanSet(plans)
    plans[0].set_outputs([0, 2])  # still allowed: the set launched nothing of the plan's
    for p in plans:
        p.close()
    buf = to_dev(torch, init)
    pset.execute_batch(buf, buf, planned_batch(lengths, places, need, [0, 1], 2))
    assert_equal(to_host(torch, buf), want)


@pytest.mark.parametrize("need,total", [(8, 12), (3, 5), (33, 50)])
def test_repair_into_a_separate_layout(torch_dev, mode, need, total):
    """dst is another tensor, objects in reverse order with other strides: only the erased shards'
    slots of dst are written, src is only read."""
    torch = torch_dev
    T, C = geometry(need)
    lengths = [T + 1, 0, 3, C * T + 5, 257, 4, 2 * T]
    pats = cycle(PATTERNS[(need, total)], len(lengths))
    pats[4] = None
    init, want, places, _ = repair_case(need, total, lengths, pats, 1, seed=700 + need)
    order = list(reversed(range(len(lengths))))
    rev, dst_size = packed_spans([lengths[o] for o in order], total, 8, start=9)
    dst_places = [None] * len(lengths)
    for place, o in zip(rev, order):
        dst_places[o] = place
    expect = np.full(dst_size + 4, SENTINEL, dtype=np.uint32)
    for sp, dp, L, pat in zip(places, dst_places, lengths, pats):
        for s in pat or ():
            shard(expect, dp, s, L)[:] = shard(want, sp, s, L)
    pset, plan_of = make_set(need, total, pats)
    batch = planned_batch(lengths, places, need, plan_of, pset.nplans, dst_places)
    src = to_dev(torch, init)
    dst = to_dev(torch, np.full(dst_size + 4, SENTINEL, dtype=np.uint32))
    pset.execute_batch(src, dst, batch)
    assert_equal(to_host(torch, dst), expect)
    assert np.array_equal(to_host(torch, src), init), "src is only read"


# ------------------------------------------------------------------ the field's boundary values

_steered = {}


def steered_case():
    """Two 8/12 objects of ST.NCOLS columns whose survivors are solved so that the rebuilt rows
    are the residues next to 0, p and 2^31 (fold96's rare branches), one per pattern."""
    if not _steered:
        need, total, L = 8, 12, ST.NCOLS
        pats = [(0, 3, 8, 11), (2, 5)]
        places, size = packed_spans([L, L], total, 1, start=3)
        init = np.full(size + 5, SENTINEL, dtype=np.uint32)
        want = init.copy()
        for o, (place, pat) in enumerate(zip(places, pats)):
            coeff = plan_rows(need, total, pat)
            tg = ST.targets(len(pat))
            x = ST.steer(coeff, tg, np.random.default_rng([812, o]))
            have = survivors(need, total, pat)
            out = OC.apply_matrix(coeff, [np.ascontiguousarray(r) for r in x])
            mask = ST.steered_rows(len(pat), need, L)
            assert all(np.array_equal(out[i][mask[i]], tg[i][mask[i]]) for i in range(len(pat))), "the steering held"
            for s in range(total):
                v = x[have.index(s)] if s in have else ERASED
                shard(init, place, s, L)[:] = v
                shard(want, place, s, L)[:] = out[pat.index(s)] if s in pat else v
        init.setflags(write=False)
        want.setflags(write=False)
        _steered["case"] = (init, want, places, pats)
    return _steered["case"]


def test_steered_boundary_columns_through_a_two_pattern_set(torch_dev, mode):
    torch = torch_dev
    init, want, places, pats = steered_case()
    pset, plan_of = make_set(8, 12, pats)
    batch = planned_batch([ST.NCOLS] * 2, places, 8, plan_of, pset.nplans)
    buf = to_dev(torch, init)
    pset.execute_batch(buf, buf, batch)
    assert_equal(to_host(torch, buf), want)


# ------------------------------------------------------------------ streams, graphs, counter sets

def test_non_default_stream(torch_dev, mode):
    torch = torch_dev
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    lengths = boundary_lengths(8)
    with torch.cuda.stream(s):
        run_repair(torch, 8, 12, lengths, cycle(PATTERNS[(8, 12)], len(lengths)), 1, seed=812, stream=s)


def test_dynamic_launch_leaves_its_counter_set_zero(torch_dev, mode):
    """Schedule 1 and 2 outside a capture: the planned launch takes the dynamic path; nothing is
    held after a synchronize; a uniform plan_execute next on the stream, which may draw the same
    set, is exact, so the planned kernel left the set zero.  Static modes touch no set."""
    torch = torch_dev
    from slime_amd import device as D
    sched, pipe = mode
    need, total = 4, 6
    T, C = geometry(need)
    lengths = [4 * C * T + 5, T, 5, 0, 3 * C * T, 257] * 8
    pats = cycle(PATTERNS[(need, total)], len(lengths))
    init, want, places, _ = repair_case(need, total, lengths, pats, 1, seed=4242)
    pset, plan_of = make_set(need, total, pats)
    batch = planned_batch(lengths, places, need, plan_of, pset.nplans)
    assert batch.units > 64
    torch.cuda.synchronize()
    _, held0 = N.ticket_sets(0)
    dyn0, fb0 = N.schedule_counts(0)
    buf = to_dev(torch, init)
    for _ in range(3):  # in place and idempotent: the survivors are never written
        pset.execute_batch(buf, buf, batch)
    dyn1, fb1 = N.schedule_counts(0)
    if sched in (1, 2) and pipe == 1:
        assert (dyn1 - dyn0, fb1 - fb0) == (3, 0), "planned launches outside a capture take the dynamic path"
    else:
        assert (dyn1 - dyn0, fb1 - fb0) == (0, 0), "static modes ask for no counter set"
    L, nobj = 5 * 4 * 3 * 1024 + 5, 6
    h = symbols(np.random.default_rng(99), (nobj, total, L))
    ubuf = to_dev(torch, h)
    lay = D.layout_of(total, L)
    D.Plan.encode(need, total)(ubuf, lay, ubuf, lay, L, nobj, dst_offset=need * L)
    assert_equal(to_host(torch, buf), want)
    ref = np.ascontiguousarray(h.transpose(1, 0, 2).reshape(total, nobj * L))
    OC.encode_object(ref, need, total)
    assert np.array_equal(to_host(torch, ubuf).reshape(nobj, total, L), ref.reshape(total, nobj, L).transpose(1, 0, 2))
    assert N.ticket_sets(0)[1] == held0, "nothing is held after the launches finished"


@pytest.mark.parametrize("sched", [1, 2])
@pytest.mark.parametrize("need,total", [(4, 6), (17, 20)])
def test_graph_captured_launch_replays_exactly(torch_dev, sched, need, total):
    """A captured planned launch replayed twice with the input changed in between.  Schedule 1
    captures the static form, 2 the dynamic one with a counter set held by the graph."""
    torch = torch_dev
    s0 = N.lib.slime_rs_kernel_schedule(-1)
    assert N.lib.slime_rs_kernel_schedule(sched) == 0
    try:
        T, C = geometry(need)
        lengths = [4 * C * T + 5, 3, T + 1, 0, 256, C * T] * 2
        pats = cycle(PATTERNS[(need, total)], len(lengths))
        cases = [repair_case(need, total, lengths, pats, 1, seed=sd) for sd in (31, 32)]
        places = cases[0][2]
        pset, plan_of = make_set(need, total, pats)
        batch = planned_batch(lengths, places, need, plan_of, pset.nplans)
        buf = to_dev(torch, cases[0][0])
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):  # warm the launch path outside the capture
            pset.execute_batch(buf, buf, batch, stream=s)
        torch.cuda.synchronize()
        _, held0 = N.ticket_sets(0)
        dyn0, _ = N.schedule_counts(0)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            pset.execute_batch(buf, buf, batch, stream=s)
        torch.cuda.synchronize()
        _, held1 = N.ticket_sets(0)
        dyn1, _ = N.schedule_counts(0)
        if sched == 2 and need <= 16:
            assert (held1 - held0, dyn1 - dyn0) == (1, 1), "the captured launch took the dynamic schedule"
        else:
            assert (held1 - held0, dyn1 - dyn0) == (0, 0), "the captured launch took a static form"
        for init, want, _, _ in (cases[1], cases[0]):
            buf.copy_(to_dev(torch, init))
            torch.cuda.synchronize()
            g.replay()
            assert_equal(to_host(torch, buf), want)
        del g  # before the batch and the set: the graph's kernel node reads their tables
        torch.cuda.synchronize()
    finally:
        N.lib.slime_rs_kernel_schedule(s0)


# ------------------------------------------------------------------ refusals

def test_refusals(torch_dev):
    torch = torch_dev
    from slime_amd import device as D
    need, total = 8, 12
    lengths, pats = [100, 7], [(0,), (2, 5)]
    init, want, places, size = repair_case(need, total, lengths, pats, 1, seed=1)
    pset, plan_of = make_set(need, total, pats)
    batch = planned_batch(lengths, places, need, plan_of, 2)
    buf = to_dev(torch, init)
    ptr = ctypes.c_void_p(buf.data_ptr())

    def refused(rc, *words):
        detail = N.lib.slime_rs_last_error().decode()
        assert rc == N.ERR_INVALID_ARG and all(w in detail for w in ("planset_execute_batch",) + words), detail

    spans = [(o, s, o, s, L) for (o, s), L in zip(places, lengths)]
    unplanned = D.Batch(spans, need)
    with pytest.raises(ValueError, match="no plan indices"):
        pset.execute_batch(buf, buf, unplanned)
    refused(N.lib.slime_rs_planset_execute_batch(pset._h, unplanned._h, ptr, ptr, None), "no plan indices")
    three = D.Batch(spans, need, plans=plan_of, nplans=3)
    with pytest.raises(ValueError, match="3 plans"):
        pset.execute_batch(buf, buf, three)
    refused(N.lib.slime_rs_planset_execute_batch(pset._h, three._h, ptr, ptr, None), "3 plans")
    other_k = D.Batch(spans, need + 1, plans=plan_of, nplans=2)
    with pytest.raises(ValueError, match="k=9"):
        pset.execute_batch(buf, buf, other_k)
    refused(N.lib.slime_rs_planset_execute_batch(pset._h, other_k._h, ptr, ptr, None), "k = 9")
    with pytest.raises(ValueError, match="addresses element"):
        pset.execute_batch(buf, buf[:places[1][0] + 5 * places[1][1] + 6].contiguous(), batch)  # ends inside shard 5
    refused(N.lib.slime_rs_planset_execute_batch(pset._h, batch._h, None, ptr, None), "null buffer")
    refused(N.lib.slime_rs_planset_execute_batch(pset._h, batch._h, ptr, None, None), "null buffer")
    with pytest.raises(N.NativeError, match="plan index 2"):
        D.Batch(spans, need, plans=[0, 2], nplans=2)
    mixed = [D.Plan.encode(8, 12), D.Plan.encode(3, 5)]
    with pytest.raises(N.NativeError, match="share k"):
        D.PlanSet(mixed)
    assert np.array_equal(to_host(torch, buf), init), "a refused launch writes nothing"
    pset.execute_batch(buf, buf, batch)
    assert_equal(to_host(torch, buf), want)
