#!/usr/bin/env python3
"""Ragged locate against the ragged verify it follows.

In one process, 2 warm-ups and then interleaved rounds timed with HIP events (no host sync
inside a timed region), medians.  Every buffer, batch, plan and result array is kept until the
process ends (tools/ragged_bench.py says why).  Every leg's results are asserted before anything
is timed.  All legs are called through ctypes with prebuilt arguments and preallocated result
arrays: a C caller's loop.

ragged_bench's seeded log-uniform mix, 4 KiB - 64 MiB, about 3 GiB of shards, packed with
64-element shard alignment, the encode plan with outputs need..total-1, at 3/5 and 8/12:

  A    slime_rs_plan_verify_batch on clean data: the baseline
  B    slime_rs_plan_locate_batch(filter = NULL) on clean data: judged against A, allowance
       |median A - median A'|
  C    A followed by slime_rs_plan_locate_batch(filter = A's mismatches) on clean data:
       C - A is the cost of walking the units to skip them
  D    as C on a copy with one wrong word in 1% of the objects
  E    filter = NULL on a copy with one whole shard wrong (every word XOR 1) in every object:
       every column takes the rare path, the worst case
  A'   a second A (the A/A noise)

Prints one JSON line.

    python tools/locate_bench.py [--rounds 12] [--warmup 2] [--mixed 3/5,8/12]
"""
import argparse
import ctypes
import json
import os
import random
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from slime_amd import _native as N  # noqa: E402
from slime_amd import device as D  # noqa: E402
from tools.ragged_bench import mixed_lengths, rounds_of, table_counts  # noqa: E402

KEEP = []  # nothing is freed before the process ends


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
    rng = random.Random(seed + 1)
    # D: one wrong word in 1% of the objects, any shard
    dbuf = D.device_empty(numel, torch.int32, 0)
    dbuf.copy_(buf)
    d_hits = {}
    for o in rng.sample(range(nobj), max(1, nobj // 100)):
        off, ss, _, _, L = spans[o]
        s, col = rng.randrange(total), rng.randrange(L)
        dbuf[off + s * ss + col] ^= 1
        d_hits[o] = (s, col)
    # E: one whole shard wrong in every object
    ebuf = D.device_empty(numel, torch.int32, 0)
    ebuf.copy_(buf)
    e_shard = [rng.randrange(total) for _ in range(nobj)]
    for (off, ss, _, _, L), s in zip(spans, e_shard):
        ebuf[off + s * ss: off + s * ss + L] ^= 1
    stream = D._stream_handle(0, None)
    ra, rb, rc, rd, re_ = (results(nobj, rows), results(nobj, nslots), results(nobj, nslots), results(nobj, nslots),
                           results(nobj, nslots))
    rdm = results(nobj, rows)
    KEEP.append((buf, dbuf, ebuf, batch, plan))
    verify, locate = N.lib.slime_rs_plan_verify_batch, N.lib.slime_rs_plan_locate_batch
    base, dbase, ebase = ptr(buf), ptr(dbuf), ptr(ebuf)

    def run_a():
        verify(plan._h, batch._h, base, base, ptr(ra[0]), ptr(ra[1]), stream)

    def run_b():
        locate(plan._h, batch._h, base, base, None, ptr(rb[0]), ptr(rb[1]), stream)

    def run_c():
        run_a()
        locate(plan._h, batch._h, base, base, ptr(ra[0]), ptr(rc[0]), ptr(rc[1]), stream)

    def run_d():
        verify(plan._h, batch._h, dbase, dbase, ptr(rdm[0]), ptr(rdm[1]), stream)
        locate(plan._h, batch._h, dbase, dbase, ptr(rdm[0]), ptr(rd[0]), ptr(rd[1]), stream)

    def run_e():
        locate(plan._h, batch._h, ebase, ebase, None, ptr(re_[0]), ptr(re_[1]), stream)

    def check():
        torch.cuda.synchronize()
        for what, (m, f) in (("A", ra), ("B", rb), ("C", rc)):
            assert int((m != 0).sum()) == 0 and int((f != -1).sum()) == 0, f"{code} {what}: clean data is not clean"
        c, f = rd[0].cpu(), rd[1].cpu()
        assert int(c.sum()) == len(d_hits), f"{code} D: {int(c.sum())} columns blamed, {len(d_hits)} planted"
        for o, (s, col) in d_hits.items():
            assert int(c[o, s]) == 1 and int(f[o, s]) == col, f"{code} D: object {o}"
        c, f = re_[0].cpu(), re_[1].cpu()
        want = torch.zeros_like(c)
        for o, s in enumerate(e_shard):
            want[o, s] = spans[o][4]
        assert bool((c == want).all()), f"{code} E: a shard's count is not its length"

    for fn in (run_a, run_b, run_c, run_d, run_e):
        fn()
    check()
    ms = rounds_of([("a", run_a), ("b", run_b), ("c", run_c), ("d", run_d), ("e", run_e), ("a2", run_a)], rounds, warmup)
    check()
    med = {k: statistics.median(v) for k, v in ms.items()}
    moved = total * 4 * sum(lengths)
    noise = abs(med["a"] - med["a2"])
    short = med["b"] - med["a"]
    return {"code": code, "seed": seed, "rounds": rounds, "objects": nobj, "shard_bytes": moved,
            "min_L": min(lengths), "max_L": max(lengths), "d_objects": len(d_hits),
            **{k + "_ms": round(v, 4) for k, v in med.items()}, "aa_noise_ms": round(noise, 4),
            "a_gibs": round(moved / 2**30 / (med["a"] / 1e3), 1), "b_gibs": round(moved / 2**30 / (med["b"] / 1e3), 1),
            "b_over_a": round(med["b"] / med["a"], 4), "b_minus_a_ms": round(short, 4),
            "b_within_allowance": bool(short <= noise),
            "c_minus_a_ms": round(med["c"] - med["a"], 4), "d_over_a": round(med["d"] / med["a"], 4),
            "e_over_a": round(med["e"] / med["a"], 4),
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
    out = {"tool": "locate_bench", "device": p.name, "schedule": N.lib.slime_rs_kernel_schedule(-1), "mixed": {}}
    for code in [s for s in a.mixed.split(",") if s]:
        out["mixed"][code] = run_mixed(code, a.rounds, a.warmup, a.seed)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
