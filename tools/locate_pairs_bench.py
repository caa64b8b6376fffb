#!/usr/bin/env python3
"""Pair locate against the one-shard locate it extends.

In one process, 2 warm-ups and then interleaved rounds timed with HIP events (no host sync
inside a timed region), medians.  Every buffer, batch, plan and result array is kept until the
process ends (tools/ragged_bench.py says why).  Every leg's results are asserted before anything
is timed and again afterwards.  All legs are called through ctypes with prebuilt arguments and
preallocated result arrays: a C caller's loop.  Run one process per code.

ragged_bench's seeded log-uniform mix, 4 KiB - 64 MiB, about 3 GiB of shards, packed with
64-element shard alignment, the encode plan with outputs need..total-1 (rows >= 4):

  A    slime_rs_plan_locate_batch(filter = NULL) on clean data: the baseline
  B    slime_rs_plan_locate_pairs_batch(filter = NULL) on clean data: the same fast path, judged
       against A with the allowance |median A - median A'|
  V    slime_rs_plan_verify_batch on a copy with two shards wrong in one column in 1% of the objects
  D    V followed by the pair locate with V's mismatches as the filter: reported as D / V
  E1s  the one-shard locate on a copy with one whole shard wrong (every word XOR 1) in every object
  E1   the pair locate on the same copy: both take the one-shard rule in every column
  E2   the pair locate on a copy with two whole shards wrong in every object: every column goes
       through the pair enumeration -- the leg the feature exists for, reported as E2 / A
  A'   a second A (the A/A noise)

Prints one JSON line.

    python tools/locate_pairs_bench.py [--rounds 12] [--warmup 2] [--code 8/12]
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


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def run_code(code, rounds, warmup, seed):
    need, total = (int(x) for x in code.split("/"))
    rows, nslots = total - need, total + 1
    assert rows >= 4, "the pair calls need four rows"
    lengths = mixed_lengths(need, total, seed)
    nobj = len(lengths)
    batch, numel = D.Batch.packed(lengths, total, need, align=64)
    spans = batch.spans.tolist()
    plan = D.Plan.encode(need, total).set_outputs(list(range(need, total)))
    buf = D.device_empty(numel, torch.int32, 0)
    D.fill_symbols(buf, 0xFACE + need)
    plan.execute_batch(buf, buf, batch)
    rng = random.Random(seed + 1)

    def copy():
        b = D.device_empty(numel, torch.int32, 0)
        b.copy_(buf)
        return b

    # D: two shards wrong in one column in 1% of the objects
    dbuf = copy()
    d_hits = {}
    for o in rng.sample(range(nobj), max(1, nobj // 100)):
        off, ss, _, _, L = spans[o]
        (s1, s2), col = sorted(rng.sample(range(total), 2)), rng.randrange(L)
        dbuf[off + s1 * ss + col] ^= 1
        dbuf[off + s2 * ss + col] ^= 1
        d_hits[o] = (s1, s2, col)
    # E1: one whole shard wrong in every object; E2: two
    e1buf, e2buf = copy(), copy()
    e_shards = [sorted(rng.sample(range(total), 2)) for _ in range(nobj)]
    for (off, ss, _, _, L), (s1, s2) in zip(spans, e_shards):
        e1buf[off + s1 * ss: off + s1 * ss + L] ^= 1
        e2buf[off + s1 * ss: off + s1 * ss + L] ^= 1
        e2buf[off + s2 * ss: off + s2 * ss + L] ^= 1
    stream = D._stream_handle(0, None)
    ra, rb, rd, re1s, re1, re2 = (results(nobj, nslots) for _ in range(6))
    rv = results(nobj, rows)
    KEEP.append((buf, dbuf, e1buf, e2buf, batch, plan))
    verify, locate, pairs = (N.lib.slime_rs_plan_verify_batch, N.lib.slime_rs_plan_locate_batch,
                             N.lib.slime_rs_plan_locate_pairs_batch)
    base, dbase, e1base, e2base = ptr(buf), ptr(dbuf), ptr(e1buf), ptr(e2buf)

    def run_a():
        locate(plan._h, batch._h, base, base, None, ptr(ra[0]), ptr(ra[1]), stream)

    def run_b():
        pairs(plan._h, batch._h, base, base, None, ptr(rb[0]), ptr(rb[1]), stream)

    def run_v():
        verify(plan._h, batch._h, dbase, dbase, ptr(rv[0]), ptr(rv[1]), stream)

    def run_d():
        run_v()
        pairs(plan._h, batch._h, dbase, dbase, ptr(rv[0]), ptr(rd[0]), ptr(rd[1]), stream)

    def run_e1s():
        locate(plan._h, batch._h, e1base, e1base, None, ptr(re1s[0]), ptr(re1s[1]), stream)

    def run_e1():
        pairs(plan._h, batch._h, e1base, e1base, None, ptr(re1[0]), ptr(re1[1]), stream)

    def run_e2():
        pairs(plan._h, batch._h, e2base, e2base, None, ptr(re2[0]), ptr(re2[1]), stream)

    def check():
        torch.cuda.synchronize()
        for what, (m, f) in (("A", ra), ("B", rb)):
            assert int((m != 0).sum()) == 0 and int((f != -1).sum()) == 0, f"{code} {what}: clean data is not clean"
        c, f = rd[0].cpu(), rd[1].cpu()
        assert int(c.sum()) == 2 * len(d_hits), f"{code} D: {int(c.sum())} slots blamed, {2 * len(d_hits)} planted"
        for o, (s1, s2, col) in d_hits.items():
            assert int(c[o, s1]) == int(c[o, s2]) == 1 and int(f[o, s1]) == int(f[o, s2]) == col, f"{code} D: object {o}"
        want1, want2 = torch.zeros_like(c), torch.zeros_like(c)
        for o, (s1, s2) in enumerate(e_shards):
            want1[o, s1] = want2[o, s1] = want2[o, s2] = spans[o][4]
        for what, (m, _), want in (("E1s", re1s, want1), ("E1", re1, want1), ("E2", re2, want2)):
            assert bool((m.cpu() == want).all()), f"{code} {what}: a wrong shard's count is not its length"

    legs = [("a", run_a), ("b", run_b), ("v", run_v), ("d", run_d), ("e1s", run_e1s), ("e1", run_e1), ("e2", run_e2),
            ("a2", run_a)]
    for _, fn in legs:
        fn()
    check()
    ms = rounds_of(legs, rounds, warmup)
    check()
    med = {k: statistics.median(v) for k, v in ms.items()}
    moved = total * 4 * sum(lengths)
    noise = abs(med["a"] - med["a2"])
    short = med["b"] - med["a"]
    return {"code": code, "seed": seed, "rounds": rounds, "objects": nobj, "shard_bytes": moved,
            "columns": sum(lengths), "min_L": min(lengths), "max_L": max(lengths), "d_objects": len(d_hits),
            **{k + "_ms": round(v, 4) for k, v in med.items()}, "aa_noise_ms": round(noise, 4),
            "a_gibs": round(moved / 2**30 / (med["a"] / 1e3), 1), "b_gibs": round(moved / 2**30 / (med["b"] / 1e3), 1),
            "b_over_a": round(med["b"] / med["a"], 4), "b_minus_a_ms": round(short, 4),
            "b_within_allowance": bool(short <= noise),
            "d_over_v": round(med["d"] / med["v"], 4), "e1_over_e1s": round(med["e1"] / med["e1s"], 4),
            "e2_over_a": round(med["e2"] / med["a"], 4),
            "e2_ns_per_column": round(med["e2"] * 1e6 / sum(lengths), 3),
            "tables": table_counts(lengths, need), "batch_units": batch.units,
            **{k + "_ms_all": [round(x, 4) for x in v] for k, v in ms.items()}, "placement": D.placement(buf)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--code", default="8/12")
    ap.add_argument("--seed", type=int, default=20240611)
    a = ap.parse_args()
    p = torch.cuda.get_device_properties(0)
    out = {"tool": "locate_pairs_bench", "device": p.name, "schedule": N.lib.slime_rs_kernel_schedule(-1),
           "result": run_code(a.code, a.rounds, a.warmup, a.seed)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
