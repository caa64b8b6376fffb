#!/usr/bin/env python3
"""Machine-code identity of every gfx950 kernel in a library or an object file
(slime_amd/codeobj.py): one line `size sha256 mangled-name` per function
symbol, sorted by (size, sha256, name).

    python tools/kernel_ids.py slime_amd/lib/libslime_rs.so > tree.txt
    python tools/kernel_ids.py --ids slime_amd/lib/libslime_rs.so > tree_ids.txt
    python tools/kernel_ids.py --diff parent.txt tree.txt

--ids writes the same sorted list without names, eight `size:sha256[:16]` a
line: a record small enough to keep.

--diff compares two lists of either form as multisets of (size, sha256[:16]): a kernel that
was renamed or moved to another file with the same instruction bytes does not
show; what shows is `-` (only in the first list) and `+` (only in the second).
Exit status 0 whether or not the lists differ.  Pure Python, nothing spawned."""
import argparse
import collections
import importlib.util
import os


def codeobj():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "slime_amd", "codeobj.py")
    spec = importlib.util.spec_from_file_location("slime_codeobj", path)  # not the package: no library is loaded
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def read_list(path):
    rows = []
    for line in open(path):
        f = line.split()
        if f and ":" in f[0]:  # --ids
            rows += [(int(t.split(":")[0]), t.split(":")[1], "") for t in f]
        elif f:
            rows.append((int(f[0]), f[1][:16], f[2]))
    return rows


def diff(a, b):
    left = collections.Counter((s, h) for s, h, _ in a)
    right = collections.Counter((s, h) for s, h, _ in b)
    out = []
    for sign, rows, other in (("-", a, right), ("+", b, left)):
        seen = collections.Counter()
        for s, h, name in rows:
            seen[(s, h)] += 1
            if seen[(s, h)] > other[(s, h)]:
                out.append(f"{sign} {s} {h} {name}".rstrip())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--diff", action="store_true", help="compare two lists written by this tool")
    ap.add_argument("--ids", action="store_true", help="sizes and short hashes only, eight a line")
    ap.add_argument("paths", nargs="+")
    a = ap.parse_args()
    if a.diff:
        if len(a.paths) != 2:
            ap.error("--diff takes two lists")
        for line in diff(read_list(a.paths[0]), read_list(a.paths[1])):
            print(line)
        return
    rows = sorted((size, sha, name) for p in a.paths for name, size, sha in codeobj().kernel_codes(p))
    if a.ids:
        ids = [f"{size}:{sha[:16]}" for size, sha, _ in rows]
        for i in range(0, len(ids), 8):
            print(" ".join(ids[i:i + 8]))
        return
    for size, sha, name in rows:
        print(size, sha, name)


if __name__ == "__main__":
    main()
