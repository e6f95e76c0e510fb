#!/usr/bin/env python
"""Compare two kernel traces of scripts/probes/tile_sweep.py launch by launch.

    python scripts/probes/tile_sweep_compare.py OLD_kernel_trace.csv NEW_kernel_trace.csv LISTING [LISTING ...]

The traces are rocprofv3 --kernel-trace CSV files of the same sweep on two builds; LISTING is the output of
scripts/isa_compare.py for those two builds (it pairs every old kernel with a new one and gives both digests).
Per launch index the grid, the workgroup size and the LDS bytes must be equal, and the two kernels must be
one of the listing's class A / B pairs (kernels that are in no listing, such as the pack or the reduce, must
have the same name).  Exit status 1 on any difference.
"""
import csv
import re
import sys


def norm(name):
    return re.sub(r"\s+", "", re.sub(r"^void ", "", name.strip().strip('"')))


def trace(path):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))  # the order of submission (two streams may overlap in time)
    geo = ("Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z", "Workgroup_Size_X", "Workgroup_Size_Y", "Workgroup_Size_Z",
           "LDS_Block_Size")
    return [(norm(r["Kernel_Name"]), tuple(int(r[k]) for k in geo)) for r in rows]


def pairs(listings):
    """old name -> (new name, class) of the isa_compare listings"""
    out = {}
    for path in listings:
        for ln in open(path):
            m = re.match(r"\s+\d+ (A|B|FAIL)\s.* \| old (.*) \| new (.*)", ln)
            if m:
                out[norm(m.group(2))] = (norm(m.group(3)), m.group(1))
    return out


def main():
    old, new = trace(sys.argv[1]), trace(sys.argv[2])
    pr = pairs(sys.argv[3:])
    bad = 0
    if len(old) != len(new):
        print("launch counts differ: %d / %d" % (len(old), len(new)))
        bad += 1
    seen = set()
    for i, ((on, og), (nn, ng)) in enumerate(zip(old, new)):
        want = pr.get(on)
        ok = og == ng and (want[0] == nn and want[1] in "AB" if want else on == nn)
        if want:
            seen.add(nn)
        if not ok:
            bad += 1
            print("launch %d differs:\n  old %s %s\n  new %s %s\n  listing pairs the old kernel with %s" %
                  (i, on, og, nn, ng, want))
    print("%d launches, %d distinct conv kernels of the listings launched, %d differences" % (len(old), len(seen), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
