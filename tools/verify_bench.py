#!/usr/bin/env python3
"""Device-side verify against the encode launch and the composed check.

In one process, interleaved A/B/C/A rounds timed with HIP events (no host sync
inside a timed region), at C3 (8/12, 128 x 256 MiB objects) and C2 (4/6,
32 x 64 MiB), the batch buffer from device_empty:

  A  Plan.verify over the full-slot layout (reads need + rows shards, writes nothing)
  B  the plan(...) encode launch over the same buffer (reads need, writes rows)
  C  what a caller had before verify: B into a scratch buffer, then
     torch.ne(scratch, stored).sum(dim=2) over the rows
  A' a second A in every round: |median A - median A'| is the process's A/A noise

Also one A over fully corrupt stored rows (every column of every row counts).
Prints one JSON line.

    python tools/verify_bench.py [--rounds 12] [--warmup 2] [--shapes c3,c2]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from slime_amd import device as D  # noqa: E402

SHAPES = {"c3": (8, 12, 128, 256), "c2": (4, 6, 32, 64)}  # need, total, objects, MiB per object


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def run_shape(name, rounds, warmup):
    need, total, nobj, mib = SHAPES[name]
    rows = total - need
    L = (mib << 20) // (4 * need)
    buf = D.device_empty(nobj * total * L, torch.int32, 0)
    D.fill_symbols(buf, 0xC0DE + need)
    lay = D.layout_of(total, L)
    plan = D.Plan.encode(need, total).set_outputs(list(range(need, total)))
    scratch = torch.empty(nobj * rows * L, dtype=torch.int32, device="cuda:0")
    slay = D.layout_of(rows, L)
    plan_scratch = D.Plan.encode(need, total)  # outputs 0..rows-1 of the scratch layout
    stored = buf.view(nobj, total, L)[:, need:, :]
    res = {}

    def run_a():
        res["a"] = plan.verify(buf, lay, buf, lay, L, nobj)

    def run_b():
        plan(buf, lay, buf, lay, L, nobj)

    def run_c():
        plan_scratch(buf, lay, scratch, slay, L, nobj)
        res["c"] = torch.ne(scratch.view(nobj, rows, L), stored).sum(dim=2)

    run_b()  # encode: the batch is clean from here on
    ev = {"a": [], "b": [], "c": [], "a2": []}
    dirty_a = torch.zeros((), dtype=torch.int64, device="cuda:0")
    dirty_c = torch.zeros((), dtype=torch.int64, device="cuda:0")
    for r in range(warmup + rounds):
        keep = r >= warmup
        for key, fn in (("a", run_a), ("b", run_b), ("c", run_c), ("a2", run_a)):
            e = timed(fn)
            if keep:
                ev[key].append(e)
            if fn is run_a:  # every A must come back clean, not only the last (outside the timed region, no sync)
                dirty_a += (res["a"][0] != 0).sum() + (res["a"][1] != -1).sum()
            elif fn is run_c:
                dirty_c += (res["c"] != 0).sum()
    torch.cuda.synchronize()
    ms = {k: [a.elapsed_time(b) for a, b in v] for k, v in ev.items()}
    med = {k: statistics.median(v) for k, v in ms.items()}
    clean_a, clean_c = int(dirty_a) == 0, int(dirty_c) == 0
    # every stored word wrong: the accounting's worst case
    D.fill_symbols(scratch, 0xBAD)
    bad = []
    for _ in range(3):
        bad.append(timed(lambda: res.__setitem__("bad", plan_scratch.verify(buf, lay, scratch, slay, L, nobj))))
    torch.cuda.synchronize()
    bad_ms = statistics.median(a.elapsed_time(b) for a, b in bad)
    bm, bf = res["bad"]
    # the exact expectation: the stored rows are the plan's output, the scratch is the fill
    ne = torch.ne(scratch.view(nobj, rows, L), stored)
    bad_ok = bool(torch.equal(bm, ne.sum(dim=2))) and bool(torch.equal(bf, ne.to(torch.uint8).argmax(dim=2)))
    del ne
    moved = (need + rows) * L * 4 * nobj
    out = {
        "shape": f"{need}/{total} x {nobj} x {mib} MiB", "L": L, "rounds": rounds,
        "a_ms": round(med["a"], 4), "a2_ms": round(med["a2"], 4), "b_ms": round(med["b"], 4),
        "c_ms": round(med["c"], 4), "aa_noise_ms": round(abs(med["a"] - med["a2"]), 4),
        "a_minus_b_ms": round(med["a"] - med["b"], 4), "c_over_a": round(med["c"] / med["a"], 3),
        "c_over_a_bytes": round((need + 3 * rows) / (need + rows), 3),
        "a_gibs": round(moved / 2**30 / (med["a"] / 1e3), 1), "b_gibs": round(moved / 2**30 / (med["b"] / 1e3), 1),
        "a_all_corrupt_ms": round(bad_ms, 4),
        "a_all_corrupt_counts_ok": bad_ok,
        "a_clean": clean_a, "c_clean": clean_c, "a_dirty_entries": int(dirty_a), "c_dirty_columns": int(dirty_c),
        "a_ms_all": [round(x, 4) for x in ms["a"]], "b_ms_all": [round(x, 4) for x in ms["b"]],
        "placement": D.placement(buf),
    }
    del buf, scratch, stored, res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="c3,c2")
    a = ap.parse_args()
    p = torch.cuda.get_device_properties(0)
    bdf = f"{getattr(p, 'pci_domain_id', 0):04x}:{p.pci_bus_id:02x}:{getattr(p, 'pci_device_id', 0):02x}.0"
    out = {"tool": "verify_bench", "bdf": bdf, "device": p.name, "shapes": {}}
    for name in a.shapes.split(","):
        out["shapes"][name] = run_shape(name, a.rounds, a.warmup)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
