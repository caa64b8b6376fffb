#!/usr/bin/env python3
"""A repair sweep in one launch (plan sets) against one launch per erasure pattern.

In one process, interleaved rounds timed with HIP events (no host sync inside
a timed region), the batch buffer from device_empty and kept, with every table,
until the process ends (tools/ragged_bench.py says why).  The workload is
ragged_bench's seeded log-uniform mix of object sizes between 4 KiB and 64 MiB
totalling about 3 GiB of shards, packed with 64-element shard alignment; every
object draws 1..total-need erasures uniformly (a uniform count, then a uniform
subset of that size) and is repaired in place from its first `need` survivors.

  M   one PlanSet.execute_batch over a planned batch
  M'  a second M in every round: |median M - median M'| is the M/M noise
  G   what a caller without plan sets does: one Batch per distinct pattern and
      one Plan.execute_batch each, back to back on the same stream (called
      through ctypes with prebuilt arguments: a C caller's loop)
  U   one single-plan Plan.execute_batch over the same spans with a plan of
      total - need rows (four at 8/12): the untouched single-plan kernel moving
      at least as many bytes

M and G must leave bit-identical buffers (asserted before anything is timed).
GiB/s are over each leg's own algorithmic bytes, sum over objects of
4 L (k + rows of the object's plan); M does fewer rows than U on average.
Prints one JSON line.

    python tools/repair_bench.py [--rounds 12] [--warmup 2] [--codes 8/12,3/5] [--erasures N]
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
from tools.ragged_bench import mixed_lengths, rounds_of  # noqa: E402

KEEP = []  # buffers, batches, sets and plans: nothing is freed before the process ends


def draw_patterns(nobj, need, total, seed, erasures=0):
    """erasures == 0: a uniform count in 1..total - need per object; else that many for every object."""
    rng = random.Random(seed ^ 0x5EED)
    return [tuple(sorted(rng.sample(range(total), erasures or rng.randint(1, total - need)))) for _ in range(nobj)]


def run_code(code, rounds, warmup, seed, erasures=0):
    need, total = (int(x) for x in code.split("/"))
    lengths = mixed_lengths(need, total, seed)
    nobj = len(lengths)
    patterns = draw_patterns(nobj, need, total, seed, erasures)
    pset, plan_of = D.PlanSet.for_erasures(need, total, patterns)
    batch, numel = D.Batch.packed(lengths, total, need, align=64, plans=plan_of, nplans=pset.nplans)
    buf = D.device_empty(numel, torch.int32, 0)
    D.fill_symbols(buf, 0xFACE + need)
    stream = D._stream_handle(0, None)
    spans = batch.spans.tolist()

    # G: the objects grouped by pattern, one batch and one plan per group.
    distinct = {}
    for o, pat in enumerate(patterns):
        distinct.setdefault(pat, []).append(o)
    groups = []
    for pat, objs in distinct.items():
        have = [i for i in range(total) if i not in pat][:need]
        plan = D.Plan.reconstruct(need, total, have, list(pat)).set_outputs(list(pat))
        groups.append((plan, D.Batch([spans[o] for o in objs], need)))
    assert len(groups) == pset.nplans
    execute_batch = N.lib.slime_rs_plan_execute_batch
    base = ctypes.c_void_p(buf.data_ptr())
    g_calls = [(p._h, b._h) for p, b in groups]

    # U: one plan of total - need rows over every object.
    u_pat = tuple(range(total - need))
    u_plan = D.Plan.reconstruct(need, total, list(range(total - need, total)), list(u_pat)).set_outputs(list(u_pat))
    u_batch = D.Batch(spans, need)

    def run_m():
        pset.execute_batch(buf, buf, batch)

    def run_g():
        for ph, bh in g_calls:
            execute_batch(ph, bh, base, base, stream)

    def run_u():
        u_plan.execute_batch(buf, buf, u_batch)

    run_g()
    ref = buf.clone()
    D.fill_symbols(buf, 0xFACE + need)  # the erased slots hold the fill again
    run_m()
    torch.cuda.synchronize()
    same = bool(torch.equal(ref, buf))
    differ = None
    if not same:
        idx = (ref != buf).nonzero().flatten()
        differ = {"words": int(idx.numel()), "first": int(idx[0]), "last": int(idx[-1])}
    KEEP.append((buf, ref, batch, pset, groups, u_plan, u_batch))
    assert same, f"{code}: M and G differ: {differ}"

    ms = rounds_of([("m", run_m), ("g", run_g), ("u", run_u), ("m2", run_m)], rounds, warmup)
    med = {k: statistics.median(v) for k, v in ms.items()}
    bytes_m = sum(4 * L * (need + len(p)) for L, p in zip(lengths, patterns))  # G's too
    bytes_u = sum(4 * L * total for L in lengths)
    gibs = {k: (bytes_u if k == "u" else bytes_m) / 2**30 / (med[k] / 1e3) for k in med}
    rows = [len(p) for p in patterns]
    return {"code": code, "erasures": erasures or "uniform", "seed": seed, "rounds": rounds, "m_equals_g": same,
            "objects": nobj,
            "patterns": pset.nplans, "rows_mean": round(sum(rows) / nobj, 3),
            "rows_hist": {r: rows.count(r) for r in sorted(set(rows))},
            "min_L": min(lengths), "max_L": max(lengths), "batch_units": batch.units,
            "bytes_m": bytes_m, "bytes_u": bytes_u,
            "m_ms": round(med["m"], 4), "m2_ms": round(med["m2"], 4), "g_ms": round(med["g"], 4),
            "u_ms": round(med["u"], 4), "mm_noise_ms": round(abs(med["m"] - med["m2"]), 4),
            "m_gibs": round(gibs["m"], 1), "m2_gibs": round(gibs["m2"], 1), "g_gibs": round(gibs["g"], 1),
            "u_gibs": round(gibs["u"], 1),
            "mm_noise_pct": round(100 * abs(gibs["m"] - gibs["m2"]) / gibs["m"], 3),
            "m_over_g_ms": round(med["m"] / med["g"], 4),
            "m_over_u_gibs": round(gibs["m"] / gibs["u"], 4),
            "m_ms_all": [round(x, 4) for x in ms["m"]], "m2_ms_all": [round(x, 4) for x in ms["m2"]],
            "g_ms_all": [round(x, 4) for x in ms["g"]], "u_ms_all": [round(x, 4) for x in ms["u"]],
            "placement": D.placement(buf)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--codes", default="8/12,3/5")
    ap.add_argument("--seed", type=int, default=20240611)
    ap.add_argument("--erasures", type=int, default=0,
                    help="erasures of every object (default 0: 1..total-need, drawn uniformly); with total-need "
                         "M moves exactly U's bytes, which separates the planned kernel's cost from the byte mix")
    a = ap.parse_args()
    p = torch.cuda.get_device_properties(0)
    bdf = f"{getattr(p, 'pci_domain_id', 0):04x}:{p.pci_bus_id:02x}:{getattr(p, 'pci_device_id', 0):02x}.0"
    out = {"tool": "repair_bench", "bdf": bdf, "device": p.name, "codes": {}}
    for code in [s for s in a.codes.split(",") if s]:
        out["codes"][code] = run_code(code, a.rounds, a.warmup, a.seed, a.erasures)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
