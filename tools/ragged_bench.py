#!/usr/bin/env python3
"""Ragged batches against the uniform launch and against one launch per object.

In one process, interleaved rounds timed with HIP events (no host sync inside
a timed region), batch buffers from device_empty, every launch an in-place
encode (outputs need..total-1 of each object's own slots).

Equal lengths -- the price of raggedness -- at C2 (4/6, 32 x 64 MiB objects)
and C3 (8/12, 128 x 256 MiB):

  A   Plan.execute_batch over a batch whose spans describe the uniform layout
  B   slime_rs_plan_execute over the same buffer
  A'  a second A in every round: |median A - median A'| is the A/A noise

Mixed lengths -- the point of the feature -- a seeded log-uniform mix of object
sizes between 4 KiB and 64 MiB totalling about 3 GiB of shards, packed with
64-element shard alignment, at 3/5, 4/6 and 8/12:

  M   one Plan.execute_batch
  N   one slime_rs_plan_execute per object, back to back on the same stream
      (called through ctypes with prebuilt arguments: a C caller's loop)
  U   one uniform launch over as many equal objects moving the same bytes
  M'  a second M in every round (the M/M noise)

M and N must leave bit-identical buffers (checked once, outside the timing).
Prints one JSON line; GiB/s are over (k + rows) * 4 * sum(L).

    python tools/ragged_bench.py [--rounds 12] [--warmup 2] [--equal c2,c3] [--mixed 3/5,4/6,8/12]
"""
import argparse
import ctypes
import json
import math
import os
import random
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from slime_amd import _native as N  # noqa: E402
from slime_amd import device as D  # noqa: E402

SHAPES = {"c3": (8, 12, 128, 256), "c2": (4, 6, 32, 64)}  # need, total, objects, MiB per object
# Every leg's batch buffer stays allocated to the end of the process: with the buffers freed and
# re-created between legs, the M == N check of the second and third mixed leg failed over a
# contiguous region that began on a 2 MiB boundary ("Measured").
KEEP = []


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def rounds_of(legs, rounds, warmup):
    """Interleaved rounds over legs [(key, fn)]: per-leg lists of milliseconds."""
    ev = {k: [] for k, _ in legs}
    for r in range(warmup + rounds):
        for key, fn in legs:
            e = timed(fn)
            if r >= warmup:
                ev[key].append(e)
    torch.cuda.synchronize()
    return {k: [a.elapsed_time(b) for a, b in v] for k, v in ev.items()}


def geometry(k):
    """Tile columns and tiles per unit (slime_amd/csrc/ragged_plan.hpp)."""
    return (1024, 3) if k <= 4 else (768, 2) if k <= 12 else (256, 6)


def table_counts(lengths, k):
    T, C = geometry(k)
    tiles = [-(-(L // 4 * 4) // T) for L in lengths]
    cols = sum(lengths)
    return {"objects": len(lengths), "columns": cols, "tiles": sum(tiles), "units": sum(-(-t // C) for t in tiles),
            "tail_columns": sum(L % 4 for L in lengths),
            # columns the tiles span over the columns they hold: the partial last tiles' share
            "tile_fill": round(cols / max(1, sum(tiles) * T), 4),
            "unit_fill": round(sum(tiles) / max(1, sum(-(-t // C) for t in tiles) * C), 4),
            "objects_under_one_tile": sum(1 for L in lengths if L < T)}


def run_equal(name, rounds, warmup):
    need, total, nobj, mib = SHAPES[name]
    L = (mib << 20) // (4 * need)
    buf = D.device_empty(nobj * total * L, torch.int32, 0)
    D.fill_symbols(buf, 0xC0DE + need)
    lay = D.layout_of(total, L)
    plan = D.Plan.encode(need, total).set_outputs(list(range(need, total)))
    batch = D.Batch([(o * total * L, L, o * total * L, L, L) for o in range(nobj)], need)

    def run_a():
        plan.execute_batch(buf, buf, batch)

    def run_b():
        plan(buf, lay, buf, lay, L, nobj)

    run_b()
    ref = buf.clone()
    run_a()
    same = bool(torch.equal(ref, buf))
    del ref
    ms = rounds_of([("a", run_a), ("b", run_b), ("a2", run_a)], rounds, warmup)
    med = {k: statistics.median(v) for k, v in ms.items()}
    moved = total * L * 4 * nobj
    out = {"shape": f"{need}/{total} x {nobj} x {mib} MiB", "L": L, "rounds": rounds, "a_equals_b": same,
           "a_ms": round(med["a"], 4), "a2_ms": round(med["a2"], 4), "b_ms": round(med["b"], 4),
           "aa_noise_ms": round(abs(med["a"] - med["a2"]), 4), "a_minus_b_ms": round(med["a"] - med["b"], 4),
           "a_over_b": round(med["a"] / med["b"], 4),
           "a_gibs": round(moved / 2**30 / (med["a"] / 1e3), 1), "b_gibs": round(moved / 2**30 / (med["b"] / 1e3), 1),
           "tables": table_counts([L] * nobj, need), "batch_units": batch.units,
           "a_ms_all": [round(x, 4) for x in ms["a"]], "b_ms_all": [round(x, 4) for x in ms["b"]],
           "a2_ms_all": [round(x, 4) for x in ms["a2"]], "placement": D.placement(buf)}
    KEEP.append((buf, batch))
    return out


def mixed_lengths(need, total, seed, target_bytes=3 << 30, lo=4 << 10, hi=64 << 20):
    """Log-uniform object sizes in [lo, hi] bytes until their shards total target_bytes."""
    rng = random.Random(seed)
    lengths, moved = [], 0
    while moved < target_bytes:
        size = int(math.exp(rng.uniform(math.log(lo), math.log(hi))))
        L = -(-(-(-size // 4)) // need)
        lengths.append(L)
        moved += total * L * 4
    return lengths


def run_mixed(code, rounds, warmup, seed):
    need, total = (int(x) for x in code.split("/"))
    lengths = mixed_lengths(need, total, seed)
    nobj = len(lengths)
    batch, numel = D.Batch.packed(lengths, total, need, align=64)
    Lu = -(-sum(lengths) // nobj)  # U: equal objects moving the same bytes
    Lu = -(-Lu // 64) * 64
    buf = D.device_empty(max(numel, nobj * total * Lu), torch.int32, 0)
    D.fill_symbols(buf, 0xFACE + need)
    plan = D.Plan.encode(need, total).set_outputs(list(range(need, total)))
    lay_u = D.layout_of(total, Lu)
    stream = D._stream_handle(0, None)
    calls = []  # N: prebuilt arguments of one slime_rs_plan_execute per object
    for off, ss, _, _, L in batch.spans.tolist():
        if L:
            p = ctypes.c_void_p(buf.data_ptr() + 4 * off)
            calls.append((p, N.Layout(obj_stride=ss * total, shard_stride=ss), L))
    execute = N.lib.slime_rs_plan_execute

    def run_m():
        plan.execute_batch(buf, buf, batch)

    def run_n():
        for p, lay, L in calls:
            execute(plan._h, p, lay, p, lay, L, 1, stream)

    def run_u():
        plan(buf, lay_u, buf, lay_u, Lu, nobj)

    run_n()
    ref = buf.clone()
    D.fill_symbols(buf, 0xFACE + need)  # the parity slots hold the fill again
    run_m()
    same = bool(torch.equal(ref, buf))
    differ = None
    if not same:  # where, and which side still holds the fill (a skipped unit)
        idx = (ref != buf).nonzero().flatten()
        fill = torch.empty_like(buf)
        D.fill_symbols(fill, 0xFACE + need)
        first = int(idx[0])
        where = next(((o, (first - off) // ss if ss else 0, (first - off) % ss if ss else 0)
                      for o, (off, ss, _, _, L) in enumerate(batch.spans.tolist())
                      if L and off <= first < off + total * ss), None)
        differ = {"words": int(idx.numel()), "first": first, "last": int(idx[-1]),
                  "first_object_shard_column": where,
                  "m_holds_fill": int((buf[idx] == fill[idx]).sum()), "n_holds_fill": int((ref[idx] == fill[idx]).sum())}
        del fill, idx
    del ref
    ms = rounds_of([("m", run_m), ("n", run_n), ("u", run_u), ("m2", run_m)], rounds, warmup)
    med = {k: statistics.median(v) for k, v in ms.items()}
    moved = total * 4 * sum(lengths)
    moved_u = total * 4 * Lu * nobj
    out = {"code": code, "seed": seed, "rounds": rounds, "m_equals_n": same, "m_n_differ": differ, "objects": nobj,
           "shard_bytes": moved, "min_L": min(lengths), "max_L": max(lengths), "uniform_L": Lu,
           "m_ms": round(med["m"], 4), "m2_ms": round(med["m2"], 4), "n_ms": round(med["n"], 4),
           "u_ms": round(med["u"], 4), "mm_noise_ms": round(abs(med["m"] - med["m2"]), 4),
           "m_over_n": round(med["m"] / med["n"], 4), "m_over_u": round(med["m"] / med["u"], 4),
           "m_gibs": round(moved / 2**30 / (med["m"] / 1e3), 1), "n_gibs": round(moved / 2**30 / (med["n"] / 1e3), 1),
           "u_gibs": round(moved_u / 2**30 / (med["u"] / 1e3), 1),
           "tables": table_counts(lengths, need), "batch_units": batch.units,
           "m_ms_all": [round(x, 4) for x in ms["m"]], "n_ms_all": [round(x, 4) for x in ms["n"]],
           "u_ms_all": [round(x, 4) for x in ms["u"]], "placement": D.placement(buf)}
    KEEP.append((buf, batch))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--equal", default="c2,c3")
    ap.add_argument("--mixed", default="3/5,4/6,8/12")
    ap.add_argument("--seed", type=int, default=20240611)
    a = ap.parse_args()
    p = torch.cuda.get_device_properties(0)
    bdf = f"{getattr(p, 'pci_domain_id', 0):04x}:{p.pci_bus_id:02x}:{getattr(p, 'pci_device_id', 0):02x}.0"
    out = {"tool": "ragged_bench", "bdf": bdf, "device": p.name, "equal": {}, "mixed": {}}
    for name in [s for s in a.equal.split(",") if s]:
        out["equal"][name] = run_equal(name, a.rounds, a.warmup)
    for code in [s for s in a.mixed.split(",") if s]:
        out["mixed"][code] = run_mixed(code, a.rounds, a.warmup, a.seed)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
