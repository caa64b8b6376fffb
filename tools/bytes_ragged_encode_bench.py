#!/usr/bin/env python3
"""Ragged byte encode: one launch over objects of different sizes against what a caller had before.

In one process, interleaved rounds timed with HIP events (no host sync inside a
timed region), medians; the batch buffer comes from device_empty and is kept,
with every table, until the process ends (tools/ragged_bench.py says why).  The
workload is bytes_ragged_bench's: ragged_bench's seeded log-uniform mix of
object sizes between 4 KiB and 64 MiB totalling about 3 GiB of chunks, packed
with 64-word chunk alignment, encoded in place (parity into chunks need..total-1).

  (a) ingest   B   one encode_objects_batch over the batch, random bytes, sizes
                   anywhere inside their size class (partial words, padding)
               N   the existing alternative: one slime_rs_encode_objects_chunked
                   per object, back to back on the same stream (ctypes with
                   prebuilt arguments: a C caller's loop)
               B and N must leave bit-identical buffers, mappings and statuses
               (asserted before timing).
  (b) flags and edges
               E   the encode over clean data (no word >= p, sizes filling every
                   chunk), with an event after the speculative pass: E0 is the
                   initialisation and pass 0, E the whole call (+ select, the
                   skipped pass 1, clear)
               D   slime_rs_decode_objects_batch with the encode-shaped plan and
                   all-zero mappings over the same spans: the same bytes moved by
                   the same walk, no flags, no edges
               D'  a second D in every round: |D - D'| is the A/A spread of the
                   decode launch, the encode's allowance
  (c) switching
               the clean data of (b) with the first word of 2%, 25% and 100% of the
               objects set to 0xFFFFFFFF (mapping 1<<31: pass 1 re-encodes them),
               E and D interleaved as in (b) on the same buffer

GiB/s are over the algorithmic bytes 4 L total summed over objects.  Prints one
JSON line.  Run every code as a step of its own under a time limit:

    timeout 300 python tools/bytes_ragged_encode_bench.py --codes 3/5
    timeout 300 python tools/bytes_ragged_encode_bench.py --codes 8/12
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

KEEP = []  # buffers, batches and plans: nothing is freed before the process ends


def med(ms):
    return {k: statistics.median(v) for k, v in ms.items()}


def phased_rounds(run_e, run_d, rounds, warmup):
    """Interleaved rounds of D, E (with its phase event), D': per-leg lists of milliseconds,
    e0 = start of E to the event after pass 0."""
    rec = []
    for r in range(warmup + rounds):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(7)]
        ev[3].record()  # torch creates events lazily: the phase event must exist before the call
        ev[0].record()
        run_d()
        ev[1].record()
        ev[2].record()
        run_e(ev[3])
        ev[4].record()
        ev[5].record()
        run_d()
        ev[6].record()
        if r >= warmup:
            rec.append(ev)
    torch.cuda.synchronize()
    return {"d": [e[0].elapsed_time(e[1]) for e in rec], "e0": [e[2].elapsed_time(e[3]) for e in rec],
            "e": [e[2].elapsed_time(e[4]) for e in rec], "d2": [e[5].elapsed_time(e[6]) for e in rec]}


def run_code(code, rounds, warmup, seed, compare):
    need, total = (int(x) for x in code.split("/"))
    lengths = mixed_lengths(need, total, seed)
    nobj = len(lengths)
    batch, numel = D.Batch.packed(lengths, total, need, align=64)
    words = D.device_empty(numel, torch.int32, 0)
    buf = words.view(torch.uint8)  # the same memory as chunk bytes
    plan = D.Plan.encode(need, total).set_outputs(list(range(need, total)))
    spans = batch.spans.tolist()
    stream = D._stream_handle(0, None)
    mp = torch.zeros(nobj, dtype=torch.int32, device="cuda:0")
    st = torch.zeros(nobj, dtype=torch.int32, device="cuda:0")
    zeros = torch.zeros(nobj, dtype=torch.int32, device="cuda:0")
    KEEP.append((words, buf, plan, batch, mp, st, zeros))
    nbytes = sum(4 * L * total for L in lengths)
    out = {"code": code, "seed": seed, "rounds": rounds, "objects": nobj, "min_L": min(lengths),
           "max_L": max(lengths), "batch_units": batch.units, "bytes": nbytes, "placement": D.placement(words)}

    def gibs(ms_):
        return round(nbytes / 2**30 / (ms_ / 1e3), 1)

    if "a" in compare:
        rng = random.Random(seed ^ 0xE1C)
        sizes = [4 * need * L - rng.randrange(4 * need) if L else 0 for L in lengths]
        sz = torch.tensor(sizes, dtype=torch.int64, device="cuda:0")
        uplan = D.Plan.encode(need, total)  # the uniform call writes row i to chunk need + i
        ump = torch.zeros(nobj, dtype=torch.int32, device="cuda:0")
        ust = torch.zeros(nobj, dtype=torch.int32, device="cuda:0")
        KEEP.append((sz, uplan, ump, ust))
        encode = N.lib.slime_rs_encode_objects_chunked
        calls = []
        for o, ((off, ss, _, _, L), S) in enumerate(zip(spans, sizes)):
            if L:
                calls.append((uplan._h, ctypes.c_void_p(buf.data_ptr() + 4 * off), 4 * ss * total, 4 * ss, S, 1,
                              ctypes.c_void_p(ump.data_ptr() + 4 * o), ctypes.c_void_p(ust.data_ptr() + 4 * o), stream))

        def run_n():
            for c in calls:
                encode(*c)

        def run_b():
            D.encode_objects_batch(plan, buf, buf, batch, sz, mp, st)

        D.fill_symbols(words, 0xFACE + need)
        run_n()
        ref = buf.clone()
        D.fill_symbols(words, 0xFACE + need)
        run_b()
        torch.cuda.synchronize()
        same = bool(torch.equal(ref, buf)) and bool(torch.equal(mp, ump)) and bool(torch.equal(st, ust))
        del ref
        assert same, f"{code}: the ragged launch and the per-object launches differ"
        ms = rounds_of([("b", run_b), ("n", run_n), ("b2", run_b)], rounds, warmup)
        m = med(ms)
        out["ingest"] = {"b_equals_n": same, "launches_n": len(calls), "switched": int((mp != 0).sum()),
                         "fallback": int(st.sum()),
                         "b_ms": round(m["b"], 4), "b2_ms": round(m["b2"], 4), "n_ms": round(m["n"], 4),
                         "b_gibs": gibs(m["b"]), "n_gibs": gibs(m["n"]), "n_over_b_ms": round(m["n"] / m["b"], 3),
                         "bb_noise_pct": round(100 * abs(m["b"] - m["b2"]) / m["b"], 3),
                         "b_ms_all": [round(x, 4) for x in ms["b"]], "n_ms_all": [round(x, 4) for x in ms["n"]]}

    if "b" in compare or "c" in compare:
        full = torch.tensor([4 * need * L for L in lengths], dtype=torch.int64, device="cuda:0")
        KEEP.append(full)
        D.fill_symbols(words, 0xFACE + need)
        buf.bitwise_and_(0x7F)  # every word below 2^31 - 2^24: neither flag bit anywhere
        order = list(range(nobj))
        random.Random(seed ^ 0x5117).shuffle(order)
        order = [o for o in order if lengths[o]]

        def run_e(ev=None):
            D.encode_objects_batch(plan, buf, buf, batch, full, mp, st, phase_event=ev)

        def run_d():
            D.decode_objects_batch(plan, buf, buf, batch, zeros)

        planted = 0
        for frac in (0.0, 0.02, 0.25, 1.0):
            if frac and "c" not in compare:
                break
            want = round(frac * len(order))
            for o in order[planted:want]:
                buf[4 * spans[o][0]: 4 * spans[o][0] + 4] = 0xFF
            planted = max(planted, want)
            run_e()
            torch.cuda.synchronize()
            assert int((mp != 0).sum()) == planted and int(st.sum()) == 0, (code, frac)
            ms = phased_rounds(run_e, run_d, rounds, warmup)
            m = med(ms)
            aa = 100 * abs(m["d"] - m["d2"]) / m["d"]
            rec = {"switched_objects": planted, "switched_bytes_pct": round(
                       100 * sum(lengths[o] for o in order[:planted]) / max(1, sum(lengths)), 2),
                   "d_ms": round(m["d"], 4), "d2_ms": round(m["d2"], 4), "e0_ms": round(m["e0"], 4),
                   "e_ms": round(m["e"], 4), "d_gibs": gibs(m["d"]), "e_gibs": gibs(m["e"]),
                   "aa_spread_pct": round(aa, 3),
                   "e0_slower_than_d_pct": round(100 * (m["e0"] - m["d"]) / m["d"], 3),
                   "e_slower_than_d_pct": round(100 * (m["e"] - m["d"]) / m["d"], 3),
                   "after_pass0_ms": round(m["e"] - m["e0"], 4),
                   "d_ms_all": [round(x, 4) for x in ms["d"]], "d2_ms_all": [round(x, 4) for x in ms["d2"]],
                   "e0_ms_all": [round(x, 4) for x in ms["e0"]], "e_ms_all": [round(x, 4) for x in ms["e"]]}
            if frac == 0.0:
                rec["e0_within_allowance"] = bool(m["e0"] - m["d"] <= abs(m["d"] - m["d2"]))
                rec["e_within_allowance"] = bool(m["e"] - m["d"] <= abs(m["d"] - m["d2"]))
                out["flags_and_edges"] = rec
                clean_e = m["e"]
            else:
                rec["e_over_clean_e"] = round(m["e"] / clean_e, 3)
                out.setdefault("switching", {})[f"{int(100 * frac)}%"] = rec
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--codes", default="3/5,8/12")
    ap.add_argument("--seed", type=int, default=20240611)
    ap.add_argument("--compare", default="abc", help="which of (a) ingest, (b) flags and edges, (c) switching to run")
    a = ap.parse_args()
    p = torch.cuda.get_device_properties(0)
    bdf = f"{getattr(p, 'pci_domain_id', 0):04x}:{p.pci_bus_id:02x}:{getattr(p, 'pci_device_id', 0):02x}.0"
    out = {"tool": "bytes_ragged_encode_bench", "bdf": bdf, "device": p.name, "codes": {}}
    for code in [s for s in a.codes.split(",") if s]:
        out["codes"][code] = run_code(code, a.rounds, a.warmup, a.seed, a.compare)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
