#!/usr/bin/env python3
"""Ragged verify against the uniform verify, against one verify per object, and -- for plan
sets -- against one launch per erasure pattern.

In one process, 2 warm-ups and then interleaved rounds timed with HIP events (no host sync
inside a timed region), medians.  Every buffer, batch, set, plan and result array is kept until
the process ends (tools/ragged_bench.py says why: DESIGN.md §15 records an unexplained mismatch
after freeing and re-creating batch buffers in one process).  Every leg's data is made
consistent first and every leg's results are asserted clean before anything is timed: clean
data is the scrubber's common case, and it issues no atomics.  All verify legs are called
through ctypes with prebuilt arguments and preallocated result arrays: a C caller's loop.

Equal lengths -- the price of raggedness -- at C2 (4/6, 32 x 64 MiB objects) and C3 (8/12,
128 x 256 MiB), full-slot layout, the encode plan with outputs need..total-1:

  A    slime_rs_plan_verify_batch over spans describing the uniform layout
  A'   a second A in every round: |median A - median A'| is the A/A noise
  B    slime_rs_plan_verify over the same buffer
  A_s  A with the static walk (slime_rs_kernel_schedule(0) around the call): the uniform verify
       is always static, so A_s against B isolates the unit list from the ticket walk
  E_A  slime_rs_plan_execute_batch on the same buffer into its own parity slots
  E_B  slime_rs_plan_execute likewise: (E_A - E_B) / E_B where positive is what raggedness
       already costs the execute, measured in the same rounds

Mixed lengths: ragged_bench's seeded log-uniform mix, 4 KiB - 64 MiB, about 3 GiB of shards,
packed with 64-element shard alignment, at 3/5, 4/6 and 8/12:

  M    one slime_rs_plan_verify_batch
  N    one slime_rs_plan_verify per object, back to back on the same stream
  U    one uniform verify over as many equal objects moving the same bytes (a second buffer,
       encoded under the uniform layout so that it is clean too)
  M'   a second M (the M/M noise);  E_M / E_U: the two executes, as above

The same mix with repair_bench's erasure draw (every object 1..total-need erased shards; the
buffer holds whole codewords, so each object is checked from its first `need` survivors):

  M    one slime_rs_planset_verify_batch over a planned batch
  G    one Batch and one slime_rs_plan_verify_batch per distinct pattern, back to back
  M'   a second M

Prints one JSON line; GiB/s are over each leg's own algorithmic bytes.

    python tools/scrub_bench.py [--rounds 12] [--warmup 2] [--equal c2,c3] [--mixed 3/5,4/6,8/12]
                                [--repair 8/12,3/5] [--schedule 0]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from slime_amd import _native as N  # noqa: E402
from slime_amd import device as D  # noqa: E402
from tools.ragged_bench import SHAPES, mixed_lengths, rounds_of, table_counts  # noqa: E402
from tools.repair_bench import draw_patterns  # noqa: E402

KEEP = []  # buffers, batches, sets, plans and result arrays: nothing is freed before the process ends


def results(nobj, rows):
    m = torch.full((nobj, rows), 0x5A5A, dtype=torch.int64, device="cuda")
    f = torch.full((nobj, rows), 0x5A5A, dtype=torch.int64, device="cuda")
    KEEP.append((m, f))
    return m, f


def ptr(t, byte_off=0):
    return ctypes.c_void_p(t.data_ptr() + byte_off)


def assert_clean(what, *pairs):
    torch.cuda.synchronize()
    for m, f in pairs:
        bad = int((m != 0).sum()), int((f != -1).sum())
        assert bad == (0, 0), f"{what}: {bad[0]} counts and {bad[1]} firsts are not clean"


def med_of(ms):
    return {k: statistics.median(v) for k, v in ms.items()}


def allowance(noise_ms, ea, eb, base_ms):
    """The allowed shortfall of a ragged verify against a uniform one taking base_ms: the run's
    noise plus the shortfall of the ragged execute against the uniform execute, where positive."""
    exec_short = max(0.0, (ea - eb) / eb)
    return {"exec_shortfall_pct": round(100 * exec_short, 3), "noise_pct": round(100 * noise_ms / base_ms, 3),
            "allowed_pct": round(100 * (exec_short + noise_ms / base_ms), 3)}


def run_equal(name, rounds, warmup):
    need, total, nobj, mib = SHAPES[name]
    rows = total - need
    L = (mib << 20) // (4 * need)
    buf = D.device_empty(nobj * total * L, torch.int32, 0)
    D.fill_symbols(buf, 0xC0DE + need)
    lay = D.layout_of(total, L)
    plan = D.Plan.encode(need, total).set_outputs(list(range(need, total)))
    batch = D.Batch([(o * total * L, L, o * total * L, L, L) for o in range(nobj)], need)
    stream = D._stream_handle(0, None)
    ra, rb = results(nobj, rows), results(nobj, rows)
    base = ptr(buf)
    KEEP.append((buf, batch, plan))

    def run_a():
        N.lib.slime_rs_plan_verify_batch(plan._h, batch._h, base, base, ptr(ra[0]), ptr(ra[1]), stream)

    def run_b():
        N.lib.slime_rs_plan_verify(plan._h, base, lay, base, lay, L, nobj, ptr(rb[0]), ptr(rb[1]), stream)

    def run_as():
        mode = N.lib.slime_rs_kernel_schedule(-1)
        N.lib.slime_rs_kernel_schedule(0)
        run_a()
        N.lib.slime_rs_kernel_schedule(mode)

    def run_ea():
        N.lib.slime_rs_plan_execute_batch(plan._h, batch._h, base, base, stream)

    def run_eb():
        N.lib.slime_rs_plan_execute(plan._h, base, lay, base, lay, L, nobj, stream)

    run_eb()  # the parity slots now hold the plan's rows; E_A and E_B rewrite the same values
    run_a()
    run_b()
    assert_clean(name, ra, rb)
    ms = rounds_of([("a", run_a), ("b", run_b), ("as", run_as), ("ea", run_ea), ("eb", run_eb), ("a2", run_a)],
                   rounds, warmup)
    assert_clean(name + " after the rounds", ra, rb)
    med = med_of(ms)
    moved = total * L * 4 * nobj
    noise = abs(med["a"] - med["a2"])
    allow = allowance(noise, med["ea"], med["eb"], med["b"])
    short = 100 * (med["a"] - med["b"]) / med["b"]
    return {"shape": f"{need}/{total} x {nobj} x {mib} MiB", "L": L, "rounds": rounds,
            "a_ms": round(med["a"], 4), "a2_ms": round(med["a2"], 4), "b_ms": round(med["b"], 4),
            "ea_ms": round(med["ea"], 4), "eb_ms": round(med["eb"], 4), "aa_noise_ms": round(noise, 4),
            "as_ms": round(med["as"], 4), "as_shortfall_pct": round(100 * (med["as"] - med["b"]) / med["b"], 3),
            "a_over_b": round(med["a"] / med["b"], 4), "a_shortfall_pct": round(short, 3), **allow,
            "within_allowance": bool(short <= allow["allowed_pct"]),
            "a_gibs": round(moved / 2**30 / (med["a"] / 1e3), 1), "b_gibs": round(moved / 2**30 / (med["b"] / 1e3), 1),
            "ea_gibs": round(moved / 2**30 / (med["ea"] / 1e3), 1),
            "eb_gibs": round(moved / 2**30 / (med["eb"] / 1e3), 1),
            "batch_units": batch.units, **{k + "_ms_all": [round(x, 4) for x in v] for k, v in ms.items()},
            "placement": D.placement(buf)}


def run_mixed(code, rounds, warmup, seed):
    need, total = (int(x) for x in code.split("/"))
    rows = total - need
    lengths = mixed_lengths(need, total, seed)
    nobj = len(lengths)
    batch, numel = D.Batch.packed(lengths, total, need, align=64)
    Lu = -(-sum(lengths) // nobj)  # U: equal objects moving the same bytes
    Lu = -(-Lu // 64) * 64
    buf = D.device_empty(numel, torch.int32, 0)
    ubuf = D.device_empty(nobj * total * Lu, torch.int32, 0)
    D.fill_symbols(buf, 0xFACE + need)
    D.fill_symbols(ubuf, 0xFACE + need)
    plan = D.Plan.encode(need, total).set_outputs(list(range(need, total)))
    lay_u = D.layout_of(total, Lu)
    stream = D._stream_handle(0, None)
    rm, rn, ru = results(nobj, rows), results(nobj, rows), results(nobj, rows)
    base, ubase = ptr(buf), ptr(ubuf)
    KEEP.append((buf, ubuf, batch, plan))
    calls = []  # N: prebuilt arguments of one slime_rs_plan_verify per object
    for o, (off, ss, _, _, L) in enumerate(batch.spans.tolist()):
        if L:
            p = ptr(buf, 4 * off)
            calls.append((p, N.Layout(obj_stride=ss * total, shard_stride=ss), L, ptr(rn[0], 8 * rows * o),
                          ptr(rn[1], 8 * rows * o)))
    verify = N.lib.slime_rs_plan_verify

    def run_m():
        N.lib.slime_rs_plan_verify_batch(plan._h, batch._h, base, base, ptr(rm[0]), ptr(rm[1]), stream)

    def run_n():
        for p, lay, L, m, f in calls:
            verify(plan._h, p, lay, p, lay, L, 1, m, f, stream)

    def run_u():
        verify(plan._h, ubase, lay_u, ubase, lay_u, Lu, nobj, ptr(ru[0]), ptr(ru[1]), stream)

    def run_em():
        N.lib.slime_rs_plan_execute_batch(plan._h, batch._h, base, base, stream)

    def run_eu():
        N.lib.slime_rs_plan_execute(plan._h, ubase, lay_u, ubase, lay_u, Lu, nobj, stream)

    run_em()
    run_eu()
    run_m()
    run_n()
    run_u()
    assert len(calls) == nobj
    assert_clean(code, rm, rn, ru)
    ms = rounds_of([("m", run_m), ("n", run_n), ("u", run_u), ("em", run_em), ("eu", run_eu), ("m2", run_m)],
                   rounds, warmup)
    assert_clean(code + " after the rounds", rm, rn, ru)
    med = med_of(ms)
    moved, moved_u = total * 4 * sum(lengths), total * 4 * Lu * nobj
    gibs = {k: (moved_u if k in ("u", "eu") else moved) / 2**30 / (med[k] / 1e3) for k in med}
    noise = abs(med["m"] - med["m2"])
    # per byte: U moves slightly more (Lu is rounded up)
    short = 100 * (gibs["u"] - gibs["m"]) / gibs["u"]
    exec_short = max(0.0, (gibs["eu"] - gibs["em"]) / gibs["eu"])
    allowed = 100 * (exec_short + noise / med["m"])
    return {"code": code, "seed": seed, "rounds": rounds, "objects": nobj, "shard_bytes": moved,
            "min_L": min(lengths), "max_L": max(lengths), "uniform_L": Lu,
            **{k + "_ms": round(v, 4) for k, v in med.items()}, "mm_noise_ms": round(noise, 4),
            **{k + "_gibs": round(v, 1) for k, v in gibs.items()},
            "m_over_n": round(med["m"] / med["n"], 4), "m_over_u": round(med["m"] / med["u"], 4),
            "m_shortfall_vs_u_pct": round(short, 3), "exec_shortfall_pct": round(100 * exec_short, 3),
            "noise_pct": round(100 * noise / med["m"], 3), "allowed_pct": round(allowed, 3),
            "within_allowance": bool(short <= allowed),
            "tables": table_counts(lengths, need), "batch_units": batch.units,
            **{k + "_ms_all": [round(x, 4) for x in v] for k, v in ms.items()}, "placement": D.placement(buf)}


def run_repair(code, rounds, warmup, seed):
    need, total = (int(x) for x in code.split("/"))
    lengths = mixed_lengths(need, total, seed)
    nobj = len(lengths)
    patterns = draw_patterns(nobj, need, total, seed)
    pset, plan_of = D.PlanSet.for_erasures(need, total, patterns)
    batch, numel = D.Batch.packed(lengths, total, need, align=64, plans=plan_of, nplans=pset.nplans)
    buf = D.device_empty(numel, torch.int32, 0)
    D.fill_symbols(buf, 0xFACE + need)
    enc = D.Plan.encode(need, total).set_outputs(list(range(need, total)))
    enc.execute_batch(buf, buf, batch)  # whole codewords: every pattern's rebuilt shards equal the stored ones
    stream = D._stream_handle(0, None)
    spans = batch.spans.tolist()
    base = ptr(buf)
    rm = results(nobj, pset.max_rows)
    distinct = {}
    for o, pat in enumerate(patterns):
        distinct.setdefault(pat, []).append(o)
    g_calls, groups = [], []
    for pat, objs in distinct.items():
        have = [i for i in range(total) if i not in pat][:need]
        plan = D.Plan.reconstruct(need, total, have, list(pat)).set_outputs(list(pat))
        gb = D.Batch([spans[o] for o in objs], need)
        res = results(len(objs), len(pat))
        groups.append((plan, gb, res))
        g_calls.append((plan._h, gb._h, ptr(res[0]), ptr(res[1])))
    assert len(groups) == pset.nplans
    KEEP.append((buf, batch, pset, enc, groups))

    def run_m():
        N.lib.slime_rs_planset_verify_batch(pset._h, batch._h, base, base, ptr(rm[0]), ptr(rm[1]), stream)

    def run_g():
        for ph, bh, m, f in g_calls:
            N.lib.slime_rs_plan_verify_batch(ph, bh, base, base, m, f, stream)

    run_m()
    run_g()
    assert_clean(code + " repair", rm, *[g[2] for g in groups])
    ms = rounds_of([("m", run_m), ("g", run_g), ("m2", run_m)], rounds, warmup)
    assert_clean(code + " repair after the rounds", rm, *[g[2] for g in groups])
    med = med_of(ms)
    moved = sum(4 * L * (need + len(p)) for L, p in zip(lengths, patterns))
    rows = [len(p) for p in patterns]
    return {"code": code, "seed": seed, "rounds": rounds, "objects": nobj, "patterns": pset.nplans,
            "rows_mean": round(sum(rows) / nobj, 3), "bytes": moved,
            **{k + "_ms": round(v, 4) for k, v in med.items()}, "mm_noise_ms": round(abs(med["m"] - med["m2"]), 4),
            **{k + "_gibs": round(moved / 2**30 / (v / 1e3), 1) for k, v in med.items()},
            "m_over_g": round(med["m"] / med["g"], 4), "batch_units": batch.units,
            **{k + "_ms_all": [round(x, 4) for x in v] for k, v in ms.items()}, "placement": D.placement(buf)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--equal", default="c2,c3")
    ap.add_argument("--mixed", default="3/5,4/6,8/12")
    ap.add_argument("--repair", default="8/12,3/5")
    ap.add_argument("--seed", type=int, default=20240611)
    ap.add_argument("--schedule", type=int, default=-1,
                    help="slime_rs_kernel_schedule for the whole run (default: leave it; 0 = static walks)")
    a = ap.parse_args()
    if a.schedule >= 0:
        assert N.lib.slime_rs_kernel_schedule(a.schedule) == 0
    p = torch.cuda.get_device_properties(0)
    bdf = f"{getattr(p, 'pci_domain_id', 0):04x}:{p.pci_bus_id:02x}:{getattr(p, 'pci_device_id', 0):02x}.0"
    out = {"tool": "scrub_bench", "bdf": bdf, "device": p.name, "schedule": N.lib.slime_rs_kernel_schedule(-1), "equal": {}, "mixed": {}, "repair": {}}
    for name in [s for s in a.equal.split(",") if s]:
        out["equal"][name] = run_equal(name, a.rounds, a.warmup)
    for code in [s for s in a.mixed.split(",") if s]:
        out["mixed"][code] = run_mixed(code, a.rounds, a.warmup, a.seed)
    for code in [s for s in a.repair.split(",") if s]:
        out["repair"][code] = run_repair(code, a.rounds, a.warmup, a.seed)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
