#!/usr/bin/env python3
"""Correct in place against the locate call it extends and the erasure repair it replaces.

In one process, 2 warm-ups and then interleaved rounds timed with HIP events (no host sync inside
a timed region), medians.  Every buffer, batch, plan and result array is kept until the process
ends (tools/ragged_bench.py says why).  Every leg's results are asserted before anything is timed
and again afterwards.  The timed calls go through ctypes with prebuilt arguments and preallocated
result arrays: a C caller's loop.  A correct call heals its buffer, so a leg that needs damage
gets it put back before its timed region, on the same stream.  Run one process per code and rule.

ragged_bench's seeded log-uniform mix, 4 KiB - 64 MiB, about 3 GiB of shards, packed with
64-element shard alignment, the encode plan with outputs need..total-1:

  A    the locate twin (max_wrong 1: slime_rs_plan_locate_batch, 2: _locate_pairs_batch) with
       filter = NULL on clean data: the baseline
  C    slime_rs_plan_correct_batch(filter = NULL) on the same clean data: the same fast path,
       judged against A with the allowance |median A - median A'|
  VL   verify + the filtered locate twin on a copy with one wrong word in 1% of the objects
  VC   verify + the filtered correct on such a copy (the words put back first): VC / VL
  E    correct on a copy with one whole shard wrong in every object (restored first): every
       column takes the rare path and one store
  L    the locate twin on the same damage (never healed): what the old path pays to learn the
       erasures, and what E pays before its fixes
  R    PlanSet.execute_batch repairing the same damage as erasures, device time only; the old
       path's host steps (counts to the host, erasures_from_counts, PlanSet.for_erasures, the
       planned batch) are timed once with the wall clock and reported apart
  A'   a second A (the A/A noise)

Prints one JSON line.

    python tools/correct_bench.py [--rounds 12] [--warmup 2] [--code 8/12] [--max-wrong 1]
"""
import argparse
import ctypes
import json
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from slime_amd import _native as N  # noqa: E402
from slime_amd import device as D  # noqa: E402
from tools.ragged_bench import mixed_lengths, table_counts, timed  # noqa: E402

KEEP = []  # nothing is freed before the process ends


def results(nobj, n):
    m = torch.full((nobj, n), 0x5A5A, dtype=torch.int64, device="cuda")
    f = torch.full((nobj, n), 0x5A5A, dtype=torch.int64, device="cuda")
    KEEP.append((m, f))
    return m, f


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def run_code(code, max_wrong, rounds, warmup, seed):
    need, total = (int(x) for x in code.split("/"))
    rows, nslots = total - need, total + 1
    assert rows >= (4 if max_wrong == 2 else 2)
    lengths = mixed_lengths(need, total, seed)
    nobj = len(lengths)
    batch, numel = D.Batch.packed(lengths, total, need, align=64)
    spans = batch.spans.tolist()
    plan = D.Plan.encode(need, total).set_outputs(list(range(need, total)))
    buf = D.device_empty(numel, torch.int32, 0)
    D.fill_symbols(buf, 0xFACE + need)
    plan.execute_batch(buf, buf, batch)
    rng = random.Random(seed + 1)

    def copy(of=buf):
        b = D.device_empty(numel, torch.int32, 0)
        b.copy_(of)
        return b

    # one wrong word in 1% of the objects: lbuf keeps it (the locate leg), dbuf gets it put back
    hits = {}
    for o in rng.sample(range(nobj), max(1, nobj // 100)):
        off, ss, _, _, L = spans[o]
        s, col = rng.randrange(total), rng.randrange(L)
        hits[o] = (s, col, off + s * ss + col)
    where = torch.tensor([w for _, _, w in hits.values()], dtype=torch.int64, device="cuda")
    wrong = buf[where] ^ 1
    lbuf, dbuf = copy(), copy()
    lbuf[where] = wrong
    # one whole shard wrong in every object: emaster keeps it, ebuf is restored from it, rbuf is repaired
    emaster = copy()
    e_shard = [rng.randrange(total) for _ in range(nobj)]
    for (off, ss, _, _, L), s in zip(spans, e_shard):
        emaster[off + s * ss: off + s * ss + L] ^= 1
    ebuf, rbuf = copy(emaster), copy(emaster)
    stream = D._stream_handle(0, None)
    ra, rc, rl, rd, re, rm = (results(nobj, nslots) for _ in range(6))
    rvl, rvd = results(nobj, rows), results(nobj, rows)
    verify, correct = N.lib.slime_rs_plan_verify_batch, N.lib.slime_rs_plan_correct_batch
    locate = N.lib.slime_rs_plan_locate_pairs_batch if max_wrong == 2 else N.lib.slime_rs_plan_locate_batch

    # the old path's host steps, once, by the wall clock: locate's counts -> erasures -> plans -> batch
    locate(plan._h, batch._h, ptr(emaster), ptr(emaster), None, ptr(re[0]), ptr(re[1]), stream)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    erasures = D.erasures_from_counts(re[0], plan.locate_slots())
    t1 = time.perf_counter()
    pset, plan_of = D.PlanSet.for_erasures(need, total, erasures)
    t2 = time.perf_counter()
    planned = D.Batch([tuple(int(v) for v in sp) for sp in spans], need, plans=plan_of, nplans=pset.nplans)
    t3 = time.perf_counter()
    assert erasures == [[s] for s in e_shard]
    KEEP.append((buf, lbuf, dbuf, emaster, ebuf, rbuf, batch, plan, pset, planned, where, wrong))
    base, lbase, dbase, ebase, mbase = ptr(buf), ptr(lbuf), ptr(dbuf), ptr(ebuf), ptr(emaster)

    def run_a():
        locate(plan._h, batch._h, base, base, None, ptr(ra[0]), ptr(ra[1]), stream)

    def run_c():
        correct(plan._h, batch._h, base, base, None, max_wrong, ptr(rc[0]), ptr(rc[1]), stream)

    def run_vl():
        verify(plan._h, batch._h, lbase, lbase, ptr(rvl[0]), ptr(rvl[1]), stream)
        locate(plan._h, batch._h, lbase, lbase, ptr(rvl[0]), ptr(rl[0]), ptr(rl[1]), stream)

    def prep_vc():
        dbuf[where] = wrong

    def run_vc():
        verify(plan._h, batch._h, dbase, dbase, ptr(rvd[0]), ptr(rvd[1]), stream)
        correct(plan._h, batch._h, dbase, dbase, ptr(rvd[0]), max_wrong, ptr(rd[0]), ptr(rd[1]), stream)

    def prep_e():
        ebuf.copy_(emaster)

    def run_e():
        correct(plan._h, batch._h, ebase, ebase, None, max_wrong, ptr(re[0]), ptr(re[1]), stream)

    def run_l():
        locate(plan._h, batch._h, mbase, mbase, None, ptr(rm[0]), ptr(rm[1]), stream)

    def run_r():
        pset.execute_batch(rbuf, rbuf, planned)

    def clean(b):
        m, f = plan.verify_batch(b, b, batch)
        return int((m != 0).sum()) == 0 and int((f != -1).sum()) == 0

    def check():
        torch.cuda.synchronize()
        for what, (m, f) in (("A", ra), ("C", rc)):
            assert int((m != 0).sum()) == 0 and int((f != -1).sum()) == 0, f"{code} {what}: clean data is not clean"
        for what, (m, f) in (("VL", rl), ("VC", rd)):
            c, f = m.cpu(), f.cpu()
            assert int(c.sum()) == len(hits), f"{code} {what}: {int(c.sum())} slots named, {len(hits)} planted"
            for o, (s, col, _) in hits.items():
                assert int(c[o, s]) == 1 and int(f[o, s]) == col, f"{code} {what}: object {o}"
        want = torch.zeros_like(re[0].cpu())
        for o, s in enumerate(e_shard):
            want[o, s] = spans[o][4]
        for what, (m, _) in (("E", re), ("L", rm)):
            assert bool((m.cpu() == want).all()), f"{code} {what}: a wrong shard's count is not its length"
        assert clean(buf) and clean(dbuf) and clean(ebuf) and clean(rbuf), f"{code}: a corrected buffer is not clean"
        assert not clean(lbuf) and not clean(emaster)

    legs = [("a", None, run_a), ("c", None, run_c), ("vl", None, run_vl), ("vc", prep_vc, run_vc), ("e", prep_e, run_e),
            ("l", None, run_l), ("r", None, run_r), ("a2", None, run_a)]
    for _, prep, fn in legs:
        if prep:
            prep()
        fn()
    check()
    ev = {k: [] for k, _, _ in legs}
    for r in range(warmup + rounds):
        for key, prep, fn in legs:
            if prep:
                prep()
            e = timed(fn)
            if r >= warmup:
                ev[key].append(e)
    torch.cuda.synchronize()
    ms = {k: [a.elapsed_time(b) for a, b in v] for k, v in ev.items()}
    check()
    med = {k: statistics.median(v) for k, v in ms.items()}
    moved = total * 4 * sum(lengths)
    noise = abs(med["a"] - med["a2"])
    over = med["c"] - med["a"]
    return {"code": code, "max_wrong": max_wrong, "seed": seed, "rounds": rounds, "objects": nobj, "shard_bytes": moved,
            "columns": sum(lengths), "min_L": min(lengths), "max_L": max(lengths), "hit_objects": len(hits),
            **{k + "_ms": round(v, 4) for k, v in med.items()}, "aa_noise_ms": round(noise, 4),
            "a_gibs": round(moved / 2**30 / (med["a"] / 1e3), 1), "c_gibs": round(moved / 2**30 / (med["c"] / 1e3), 1),
            "c_over_a": round(med["c"] / med["a"], 4), "c_minus_a_ms": round(over, 4),
            "c_within_allowance": bool(over <= noise),
            "vc_over_vl": round(med["vc"] / med["vl"], 4),
            "e_over_r": round(med["e"] / med["r"], 4), "e_over_l": round(med["e"] / med["l"], 4),
            "e_over_l_plus_r": round(med["e"] / (med["l"] + med["r"]), 4), "e_over_a": round(med["e"] / med["a"], 4),
            "e_ns_per_column": round(med["e"] * 1e6 / sum(lengths), 3),
            "old_path_host_ms": {"erasures_from_counts": round((t1 - t0) * 1e3, 3),
                                 "planset_for_erasures": round((t2 - t1) * 1e3, 3),
                                 "planned_batch": round((t3 - t2) * 1e3, 3), "plans": pset.nplans},
            "tables": table_counts(lengths, need), "batch_units": batch.units,
            **{k + "_ms_all": [round(x, 4) for x in v] for k, v in ms.items()}, "placement": D.placement(buf)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--code", default="8/12")
    ap.add_argument("--max-wrong", type=int, default=1, choices=(1, 2))
    ap.add_argument("--seed", type=int, default=20240611)
    a = ap.parse_args()
    p = torch.cuda.get_device_properties(0)
    out = {"tool": "correct_bench", "device": p.name, "schedule": N.lib.slime_rs_kernel_schedule(-1),
           "result": run_code(a.code, a.max_wrong, a.rounds, a.warmup, a.seed)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
