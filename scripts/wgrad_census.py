#!/usr/bin/env python3
"""Static instruction census of a kernel's main loop from hipcc's device assembly (-S).

usage: wgrad_census.py FILE.s KERNEL_SUBSTRING [KERNEL_SUBSTRING ...]

For each kernel whose mangled name contains the substring, every backward branch delimits a loop
[label, branch]; the ranges that hold MFMAs are merged where they overlap (one loop with several
back edges) and printed with their opcode counts, grouped
into classes (MFMA, LDS reads, LDS-DMA, integer multiplies, other VALU, SALU, waits/barriers).
"""
import collections
import re
import sys


def kernel_body(lines, sub):
    start = None
    for i, l in enumerate(lines):
        m = re.match(r"^(_Z\w+):", l)
        if m and sub in m.group(1) and start is None:
            start, name = i, m.group(1)
        elif start is not None and l.startswith(".Lfunc_end"):
            return name, lines[start:i]
    return None, []


def klass(op):
    if op.startswith("v_mfma"):
        return "mfma"
    if op.startswith("ds_read"):
        return "lds_read"
    if op.startswith("global_load_lds"):
        return "lds_dma"
    if op.startswith(("v_mul_lo", "v_mul_hi", "v_mad_u64", "v_mad_i64", "v_mad_u32", "v_mul_u32")):
        return "v_int_mul"
    if op.startswith("v_pk_"):
        return "v_packed"
    if op.startswith("v_"):
        return "v_other"
    if op.startswith(("s_waitcnt", "s_barrier", "s_nop", "s_setprio")):
        return "wait_sync"
    if op.startswith(("s_cbranch", "s_branch")):
        return "branch"
    if op.startswith("s_"):
        return "salu"
    return "other"


def loops(body):
    labels = {}
    for i, l in enumerate(body):
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            labels[m.group(1)] = i
    out = []
    for i, l in enumerate(body):
        m = re.match(r"^\s+s_c?branch\w*\s+(\.LBB\d+_\d+)", l)
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            out.append((labels[m.group(1)], i))
    return out


def main():
    lines = open(sys.argv[1]).read().split("\n")
    for sub in sys.argv[2:]:
        name, body = kernel_body(lines, sub)
        if not body:
            print("no kernel matching", sub)
            continue
        print("==", name)
        ls = loops(body)
        # the main loop has several back edges (the stage's scalar branches end in different blocks):
        # every back-edge range that holds an MFMA belongs to it, and overlapping ranges are merged, so
        # the count covers all of the loop's blocks -- the bias blocks and the deferred stepping too
        ls = sorted((a, b) for (a, b) in ls if any("v_mfma" in l for l in body[a:b + 1]))
        inner = []
        for a, b in ls:
            if inner and a <= inner[-1][1]:
                inner[-1] = (inner[-1][0], max(inner[-1][1], b))
            else:
                inner.append((a, b))
        for a, b in inner:
            ops = collections.Counter()
            cls = collections.Counter()
            for l in body[a:b + 1]:
                m = re.match(r"^\s+([a-z]\w+)", l)
                if not m:
                    continue
                ops[m.group(1)] += 1
                cls[klass(m.group(1))] += 1
            if not cls["mfma"]:
                continue
            print("loop lines %d..%d: %d instructions" % (a, b, sum(ops.values())))
            print("  classes:", dict(sorted(cls.items())))
            vo = {k: v for k, v in ops.items() if klass(k) in ("v_other", "v_int_mul", "v_packed")}
            print("  valu:", dict(sorted(vo.items(), key=lambda kv: -kv[1])))


if __name__ == "__main__":
    main()
