#!/usr/bin/env python3
"""Plan-set locate against the single-plan locate and the plan-set verify it follows.

tools/locate_bench.py's method: one process, 2 warm-ups and then interleaved rounds timed with
HIP events (no host sync inside a timed region), medians; every buffer, batch, plan and result
array is kept until the process ends; every leg's results are asserted before and after the
rounds; all legs go through ctypes with prebuilt arguments and preallocated result arrays.

ragged_bench's seeded log-uniform mix, 4 KiB - 64 MiB, about 3 GiB of shards, packed with
64-element shard alignment, at 3/5 and 8/12:

  A    slime_rs_plan_locate_batch(filter = NULL), the encode plan, clean data: the baseline
  A'   a second A: |median A - median A'| is the allowance
  B    slime_rs_planset_locate_batch(filter = NULL) on the same data with a one-plan set and a
       planned batch: B - A is the cost of reading a plan record per object
  CV   slime_rs_planset_verify_batch with PlanSet.for_scrub's set, every object missing 0 to
       min(2, rows - 2) shards (their slots hold a sentinel), otherwise clean: C's baseline
  CL   slime_rs_planset_locate_batch(filter = NULL) on the same
  DV   the plan-set verify on a copy with one wrong word in a survivor of 1% of the objects
  D    DV followed by the plan-set locate with DV's mismatches as the filter

Prints one JSON line.

    python tools/planset_locate_bench.py [--rounds 12] [--warmup 2] [--mixed 3/5,8/12]
"""
import argparse
import ctypes
import json
import os
import random
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from slime_amd import _native as N  # noqa: E402
from slime_amd import device as D  # noqa: E402
from tools.ragged_bench import mixed_lengths, rounds_of, table_counts  # noqa: E402

KEEP = []  # nothing is freed before the process ends
SENTINEL = 0xE7A5ED00 - (1 << 32)  # as int32


def results(nobj, n):
    m = torch.full((nobj, n), 0x5A5A, dtype=torch.int64, device="cuda")
    f = torch.full((nobj, n), 0x5A5A, dtype=torch.int64, device="cuda")
    KEEP.append((m, f))
    return m, f


def ptr(t, byte_off=0):
    return ctypes.c_void_p(t.data_ptr() + byte_off)


def run_mixed(code, rounds, warmup, seed):
    need, total = (int(x) for x in code.split("/"))
    rows, nslots = total - need, total + 1
    lengths = mixed_lengths(need, total, seed)
    nobj = len(lengths)
    batch, numel = D.Batch.packed(lengths, total, need, align=64)
    spans = batch.spans.tolist()
    plan = D.Plan.encode(need, total).set_outputs(list(range(need, total)))
    buf = D.device_empty(numel, torch.int32, 0)
    D.fill_symbols(buf, 0xFACE + need)
    plan.execute_batch(buf, buf, batch)
    one = D.PlanSet([plan])
    one_batch, _ = D.Batch.packed(lengths, total, need, align=64, plans=np.zeros(nobj, dtype=np.uint32), nplans=1)
    # C: every object misses 0 .. min(2, rows - 2) shards, so every plan keeps two rows or more
    rng = random.Random(seed + 2)
    most = max(0, min(2, rows - 2))
    missing = [tuple(sorted(rng.sample(range(total), rng.randint(0, most)))) for _ in range(nobj)]
    pset, plan_of = D.PlanSet.for_scrub(need, total, missing)
    sbatch, _ = D.Batch.packed(lengths, total, need, align=64, plans=plan_of, nplans=pset.nplans)
    max_rows, sslots = pset.max_rows, need + pset.max_rows + 1
    cbuf = D.device_empty(numel, torch.int32, 0)
    cbuf.copy_(buf)
    for (off, ss, _, _, L), pat in zip(spans, missing):
        for s in pat:
            cbuf[off + s * ss: off + s * ss + L] = SENTINEL
    # D: one wrong word in a survivor of 1% of the objects
    dbuf = D.device_empty(numel, torch.int32, 0)
    dbuf.copy_(cbuf)
    d_hits = {}
    for o in rng.sample(range(nobj), max(1, nobj // 100)):
        off, ss, _, _, L = spans[o]
        s = rng.choice([i for i in range(total) if i not in missing[o]])
        col = rng.randrange(L)
        dbuf[off + s * ss + col] ^= 1
        d_hits[o] = (pset.locate_slots(int(plan_of[o])).index(s), col)
    stream = D._stream_handle(0, None)
    ra, rb = results(nobj, nslots), results(nobj, nslots)
    rcv, rcl = results(nobj, max_rows), results(nobj, sslots)
    rdv, rd = results(nobj, max_rows), results(nobj, sslots)
    KEEP.append((buf, cbuf, dbuf, batch, one_batch, sbatch, plan, one, pset))
    locate, set_locate = N.lib.slime_rs_plan_locate_batch, N.lib.slime_rs_planset_locate_batch
    set_verify = N.lib.slime_rs_planset_verify_batch
    base, cbase, dbase = ptr(buf), ptr(cbuf), ptr(dbuf)

    def run_a():
        locate(plan._h, batch._h, base, base, None, ptr(ra[0]), ptr(ra[1]), stream)

    def run_b():
        set_locate(one._h, one_batch._h, base, base, None, ptr(rb[0]), ptr(rb[1]), stream)

    def run_cv():
        set_verify(pset._h, sbatch._h, cbase, cbase, ptr(rcv[0]), ptr(rcv[1]), stream)

    def run_cl():
        set_locate(pset._h, sbatch._h, cbase, cbase, None, ptr(rcl[0]), ptr(rcl[1]), stream)

    def run_dv():
        set_verify(pset._h, sbatch._h, dbase, dbase, ptr(rdv[0]), ptr(rdv[1]), stream)

    def run_d():
        run_dv()
        set_locate(pset._h, sbatch._h, dbase, dbase, ptr(rdv[0]), ptr(rd[0]), ptr(rd[1]), stream)

    def check():
        torch.cuda.synchronize()
        for what, (m, f) in (("A", ra), ("B", rb), ("CV", rcv), ("CL", rcl)):
            assert int((m != 0).sum()) == 0 and int((f != -1).sum()) == 0, f"{code} {what}: clean data is not clean"
        assert int((rdv[0].sum(dim=1) != 0).sum()) == len(d_hits), f"{code} DV: not the planted objects"
        c, f = rd[0].cpu(), rd[1].cpu()
        assert int(c.sum()) == len(d_hits), f"{code} D: {int(c.sum())} columns blamed, {len(d_hits)} planted"
        for o, (slot, col) in d_hits.items():
            assert int(c[o, slot]) == 1 and int(f[o, slot]) == col, f"{code} D: object {o}"

    legs = [("a", run_a), ("b", run_b), ("cv", run_cv), ("cl", run_cl), ("dv", run_dv), ("d", run_d), ("a2", run_a)]
    for _, fn in legs:
        fn()
    check()
    ms = rounds_of(legs, rounds, warmup)
    check()
    med = {k: statistics.median(v) for k, v in ms.items()}
    moved = total * 4 * sum(lengths)
    noise = abs(med["a"] - med["a2"])
    extra = med["b"] - med["a"]
    return {"code": code, "seed": seed, "rounds": rounds, "objects": nobj, "shard_bytes": moved,
            "min_L": min(lengths), "max_L": max(lengths), "scrub_plans": pset.nplans, "max_rows": max_rows,
            "missing_histogram": [sum(1 for m in missing if len(m) == n) for n in range(most + 1)],
            "d_objects": len(d_hits),
            **{k + "_ms": round(v, 4) for k, v in med.items()}, "aa_noise_ms": round(noise, 4),
            "b_over_a": round(med["b"] / med["a"], 4), "b_minus_a_ms": round(extra, 4),
            "b_within_allowance": bool(extra <= noise),
            "cl_over_cv": round(med["cl"] / med["cv"], 4), "cl_minus_cv_ms": round(med["cl"] - med["cv"], 4),
            "d_over_dv": round(med["d"] / med["dv"], 4),
            "tables": table_counts(lengths, need), "batch_units": batch.units,
            **{k + "_ms_all": [round(x, 4) for x in v] for k, v in ms.items()}, "placement": D.placement(buf)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--mixed", default="3/5,8/12")
    ap.add_argument("--seed", type=int, default=20240611)
    a = ap.parse_args()
    p = torch.cuda.get_device_properties(0)
    out = {"tool": "planset_locate_bench", "device": p.name, "schedule": N.lib.slime_rs_kernel_schedule(-1), "mixed": {}}
    for code in [s for s in a.mixed.split(",") if s]:
        out["mixed"][code] = run_mixed(code, a.rounds, a.warmup, a.seed)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
