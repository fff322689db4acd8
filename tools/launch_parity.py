#!/usr/bin/env python3
"""Do two runs launch the same kernels with the same geometry?   python tools/launch_parity.py A.csv B.csv

Reads two `rocprofv3 --kernel-trace --output-format csv` traces of the same program under two builds of the library and compares, per kernel
name, the call count and the multiset of (grid x, y, z, workgroup size x, y, z, LDS bytes).  Order is not compared: the two queues of a pass
interleave differently from run to run.  Prints every difference; exit status 1 when there is one."""
import collections
import csv
import sys


def launches(path):
    with open(path, newline="") as fh:
        rows = list(csv.DictReader(fh))
    if not rows:
        sys.exit(f"{path}: no kernel dispatches")
    lds = [c for c in rows[0] if c.startswith("LDS")]
    cols = [f"Grid_Size_{a}" for a in "XYZ"] + [f"Workgroup_Size_{a}" for a in "XYZ"] + lds[:1]
    missing = [c for c in cols if c not in rows[0]] + ([] if lds else ["LDS_*"])
    if missing:
        sys.exit(f"{path}: columns missing: {missing}")
    out = collections.defaultdict(collections.Counter)
    for r in rows:
        out[r["Kernel_Name"]][tuple(int(r[c]) for c in cols)] += 1
    return out


def main(a_path, b_path):
    a, b = launches(a_path), launches(b_path)
    diffs = 0
    for name in sorted(set(a) | set(b)):
        ca, cb = a.get(name, collections.Counter()), b.get(name, collections.Counter())
        if ca == cb:
            continue
        diffs += 1
        print(f"{name}: {sum(ca.values())} calls against {sum(cb.values())}")
        for geom in sorted(set(ca) | set(cb)):
            if ca[geom] != cb[geom]:
                print(f"    grid {geom[0:3]} workgroup {geom[3:6]} lds {geom[6]}: {ca[geom]} against {cb[geom]}")
    print(f"{len(set(a) | set(b))} kernels, {sum(sum(c.values()) for c in a.values())} against {sum(sum(c.values()) for c in b.values())} launches, "
          f"{diffs} kernels differ")
    return 1 if diffs else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
