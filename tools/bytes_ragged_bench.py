#!/usr/bin/env python3
"""Ragged byte objects: one launch over stored chunks against what a caller had before.

In one process, interleaved rounds timed with HIP events (no host sync inside
a timed region), medians; the batch buffer comes from device_empty and is kept,
with every table, until the process ends (tools/ragged_bench.py says why).  The
workload is repair_bench's: ragged_bench's seeded log-uniform mix of object
sizes between 4 KiB and 64 MiB totalling about 3 GiB of chunks, packed with
64-word chunk alignment; every object draws 1..total-need erasures and has its
own mapping value (0, 1<<31 or a random word).  The buffer holds arbitrary
bytes: every byte pattern decodes.

  (a) repair   B   one planset decode_objects_batch over the planned batch
               N   the existing alternative: one slime_rs_decode_objects_chunked
                   per object with that object's plan, back to back on the same
                   stream (ctypes with prebuilt arguments: a C caller's loop)
               B and N must leave bit-identical buffers (asserted before timing).
  (b) bytes vs symbols
               B   the byte launch
               S   slime_rs_planset_execute_batch over the same spans of the same
                   buffer read as symbols: identical bytes moved
               S'  a second S in every round: |S - S'| is the A/A spread of the
                   symbol launch, the byte launch's allowance
  (c) scrub    V   one verify_objects_batch with the encode-shaped plan
               P   slime_gf_pack_device per object (its own mapping) into a word
                   buffer, then one plan_verify_batch over the words
               P0  one pack of the whole buffer with mapping 0, then the same
                   verify: the least a pack pass can cost (right only where every
                   object's mapping is 0)

GiB/s are over each leg's algorithmic bytes: repair 4 L (k + rows of the
object's plan) summed over objects, scrub 4 L total.  Prints one JSON line.
Run every code as a step of its own under a time limit:

    timeout 300 python tools/bytes_ragged_bench.py --codes 3/5
    timeout 300 python tools/bytes_ragged_bench.py --codes 8/12
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
from tools.repair_bench import draw_patterns  # noqa: E402

KEEP = []  # buffers, batches, sets and plans: nothing is freed before the process ends


def draw_mappings(nobj, seed):
    rng = random.Random(seed ^ 0x3A9)
    return [rng.choice((0, 1 << 31, rng.getrandbits(32))) for _ in range(nobj)]


def run_code(code, rounds, warmup, seed, compare):
    need, total = (int(x) for x in code.split("/"))
    lengths = mixed_lengths(need, total, seed)
    nobj = len(lengths)
    patterns = draw_patterns(nobj, need, total, seed)
    maps = draw_mappings(nobj, seed)
    pset, plan_of = D.PlanSet.for_erasures(need, total, patterns)
    batch, numel = D.Batch.packed(lengths, total, need, align=64, plans=plan_of, nplans=pset.nplans)
    words = D.device_empty(numel, torch.int32, 0)
    D.fill_symbols(words, 0xFACE + need)
    buf = words.view(torch.uint8)  # the same memory as chunk bytes
    mt = torch.tensor([m - (1 << 32) if m >= 1 << 31 else m for m in maps], dtype=torch.int32, device="cuda:0")
    stream = D._stream_handle(0, None)
    spans = batch.spans.tolist()
    KEEP.append((words, buf, mt, batch, pset))
    bytes_m = sum(4 * L * (need + len(p)) for L, p in zip(lengths, patterns))
    bytes_v = sum(4 * L * total for L in lengths)
    out = {"code": code, "seed": seed, "rounds": rounds, "objects": nobj, "patterns": pset.nplans,
           "min_L": min(lengths), "max_L": max(lengths), "batch_units": batch.units,
           "mappings": {"zero": maps.count(0), "top_bit": maps.count(1 << 31),
                        "random": nobj - maps.count(0) - maps.count(1 << 31)},
           "bytes_repair": bytes_m, "bytes_scrub": bytes_v, "placement": D.placement(words)}

    def run_b():
        D.decode_objects_batch(pset, buf, buf, batch, mt)

    def med_gibs(ms, nbytes):
        med = {k: statistics.median(v) for k, v in ms.items()}
        return med, {k: nbytes / 2**30 / (med[k] / 1e3) for k in med}

    if "a" in compare:
        plans = {}
        for pat in patterns:
            if pat not in plans:
                have = [i for i in range(total) if i not in pat][:need]
                plans[pat] = D.Plan.reconstruct(need, total, have, list(pat)).set_outputs(list(pat))
        decode = N.lib.slime_rs_decode_objects_chunked
        calls = []
        for o, ((off, ss, _, _, L), pat) in enumerate(zip(spans, patterns)):
            if L:
                calls.append((plans[pat]._h, ctypes.c_void_p(buf.data_ptr() + 4 * off), 4 * ss * total, 4 * ss, L, 1,
                              ctypes.c_void_p(mt.data_ptr() + 4 * o), stream))
        KEEP.append(plans)

        def run_n():
            for c in calls:
                decode(*c)

        run_n()
        ref = buf.clone()
        D.fill_symbols(words, 0xFACE + need)  # the erased chunks hold the fill again
        run_b()
        torch.cuda.synchronize()
        same = bool(torch.equal(ref, buf))
        KEEP.append(ref)
        assert same, f"{code}: the ragged launch and the per-object launches differ"
        ms = rounds_of([("b", run_b), ("n", run_n), ("b2", run_b)], rounds, warmup)
        med, gibs = med_gibs(ms, bytes_m)
        out["repair"] = {"b_equals_n": same, "launches_n": len(calls),
                         "b_ms": round(med["b"], 4), "b2_ms": round(med["b2"], 4), "n_ms": round(med["n"], 4),
                         "b_gibs": round(gibs["b"], 1), "n_gibs": round(gibs["n"], 1),
                         "n_over_b_ms": round(med["n"] / med["b"], 3),
                         "bb_noise_pct": round(100 * abs(med["b"] - med["b2"]) / med["b"], 3),
                         "b_ms_all": [round(x, 4) for x in ms["b"]], "n_ms_all": [round(x, 4) for x in ms["n"]]}

    if "b" in compare:
        def run_s():
            pset.execute_batch(words, words, batch)

        ms = rounds_of([("s", run_s), ("b", run_b), ("s2", run_s), ("b2", run_b)], rounds, warmup)
        med, gibs = med_gibs(ms, bytes_m)
        aa = 100 * abs(med["s"] - med["s2"]) / med["s"]
        gap = 100 * (med["b"] - med["s"]) / med["s"]
        out["bytes_vs_symbols"] = {"s_ms": round(med["s"], 4), "s2_ms": round(med["s2"], 4),
                                   "b_ms": round(med["b"], 4), "b2_ms": round(med["b2"], 4),
                                   "s_gibs": round(gibs["s"], 1), "b_gibs": round(gibs["b"], 1),
                                   "aa_spread_pct": round(aa, 3), "b_slower_than_s_pct": round(gap, 3),
                                   "within_allowance": bool(gap <= aa),
                                   "s_ms_all": [round(x, 4) for x in ms["s"]],
                                   "s2_ms_all": [round(x, 4) for x in ms["s2"]],
                                   "b_ms_all": [round(x, 4) for x in ms["b"]]}

    if "c" in compare:
        plan = D.Plan.encode(need, total).set_outputs(list(range(need, total)))
        plain = D.Batch(spans, need)
        packed = D.device_empty(numel, torch.int32, 0)
        packed0 = D.device_empty(numel, torch.int32, 0)
        KEEP.append((plan, plain, packed, packed0))
        # A scrub's normal case is clean data: every object's parity chunks as its mapping stores them
        # (the byte launch with the encode-shaped plan), so no leg runs the mismatch path.
        D.decode_objects_batch(plan, buf, buf, plain, mt)
        pack = N.lib.slime_gf_pack_device
        pcalls = []
        for (off, ss, _, _, L), m in zip(spans, maps):
            if L:
                pcalls.append((0, ctypes.c_void_p(buf.data_ptr() + 4 * off), 4 * ss * total, m,
                               ctypes.c_void_p(packed.data_ptr() + 4 * off), None, stream))
        results = []

        def run_v():
            results[:] = [D.verify_objects_batch(plan, buf, buf, plain, mt)]

        def run_p():
            for c in pcalls:
                pack(*c)
            results[:] = [plan.verify_batch(packed, packed, plain)]

        def run_p0():  # the pack's cost over the whole buffer, then the verify over the rightly packed words
            D.pack_bytes(buf, 0, packed0)
            results[:] = [plan.verify_batch(packed, packed, plain)]

        run_v()
        v = [t.clone() for t in results[0]]
        run_p()
        torch.cuda.synchronize()
        same = all(bool(torch.equal(a, b)) for a, b in zip(v, results[0]))
        assert same, f"{code}: the byte verify and pack + symbol verify report differently"
        assert int(v[0].sum()) == 0, f"{code}: the scrubbed data is not clean"
        ms = rounds_of([("v", run_v), ("p", run_p), ("p0", run_p0), ("v2", run_v)], rounds, warmup)
        med, gibs = med_gibs(ms, bytes_v)
        out["scrub"] = {"v_equals_p": same, "pack_launches": len(pcalls),
                        "v_ms": round(med["v"], 4), "v2_ms": round(med["v2"], 4), "p_ms": round(med["p"], 4),
                        "p0_ms": round(med["p0"], 4), "v_gibs": round(gibs["v"], 1), "p_gibs": round(gibs["p"], 1),
                        "p0_gibs": round(gibs["p0"], 1), "p_over_v_ms": round(med["p"] / med["v"], 3),
                        "p0_over_v_ms": round(med["p0"] / med["v"], 3),
                        "vv_noise_pct": round(100 * abs(med["v"] - med["v2"]) / med["v"], 3),
                        "v_ms_all": [round(x, 4) for x in ms["v"]], "p_ms_all": [round(x, 4) for x in ms["p"]],
                        "p0_ms_all": [round(x, 4) for x in ms["p0"]]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--codes", default="3/5,8/12")
    ap.add_argument("--seed", type=int, default=20240611)
    ap.add_argument("--compare", default="abc", help="which of the comparisons (a) repair, (b) bytes vs symbols, "
                                                      "(c) scrub to run")
    a = ap.parse_args()
    p = torch.cuda.get_device_properties(0)
    bdf = f"{getattr(p, 'pci_domain_id', 0):04x}:{p.pci_bus_id:02x}:{getattr(p, 'pci_device_id', 0):02x}.0"
    out = {"tool": "bytes_ragged_bench", "bdf": bdf, "device": p.name, "codes": {}}
    for code in [s for s in a.codes.split(",") if s]:
        out["codes"][code] = run_code(code, a.rounds, a.warmup, a.seed, a.compare)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
