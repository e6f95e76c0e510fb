#!/usr/bin/env python
"""Kernel-by-kernel comparison of the kernels' gfx950 assembly between two source trees.

A refactor of kernel templates must leave the machine code alone.  This compiles the same sources of
two trees (device code only, the flags of alphago_amd/_build.py; nothing is linked or run), or reads two
assembly files, and pairs their kernels by position within each kernel family (the template name).
Per kernel it prints the demangled name, a digest of the body and the register / LDS metadata.

The digest is taken over the body with the kernel's own symbol masked, the `.LBB<n>_` label prefix
renumbered per kernel (in the loop comments too) and `__hip_cuid` lines dropped, so a renamed template
argument or a kernel added earlier in the file does not show.

--added REGEX: kernels of the NEW side whose demangled name matches are new instantiations of an old
template (a compile-time flag such as the fp8 skip operand).  They are taken out of the pairing and
listed with their metadata after the families; every other kernel must still pair.

Every pair is classified:
  A  the digests are equal;
  B  the metadata is equal in every field but sgpr_count, the multiset of mnemonics is equal, and the
     mnemonic sequence from the first v_mfma to the end of the kernel is equal (a prologue whose scalar
     instructions were reordered);
  FAIL  anything else.  Different kernel counts in a family are an error.

    python scripts/isa_compare.py OLD NEW [--flavor prod|debug|lab] [--sources a.hip,b.hip] [--out listing.txt]
                                  [--keep DIR] [--brief]

OLD / NEW: a source tree (the directory that holds alphago_amd/), an assembly file, or several assembly
files joined with commas (one per source file, the same order on both sides).  The lab flavour
compiles conv.hip, conv_lab.hip, conv_fwd_variants.hip and conv_wgrad_row.hip; the others conv.hip.
--sources names other files under csrc/kernels instead (the head family has no MFMA, so its pairs are
class A or FAIL; a failed pair lists both sides' metadata and the difference of the mnemonic multisets,
to be judged by hand).  About a minute per tree and file.  Exit status 1 when a pair fails.
"""
from __future__ import annotations

import argparse
import collections
import hashlib
import os
import re
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from epilogue_listing import compile_asm, demangle, kernels_of, metadata  # noqa: E402

SOURCES = {"prod": ["conv.hip"], "debug": ["conv.hip"],
           "lab": ["conv.hip", "conv_lab.hip", "conv_fwd_variants.hip", "conv_wgrad_row.hip"]}
META = ("vgpr", "agpr", "sgpr", "scratch", "vspill", "sspill", "lds", "kernarg")


def mnemonics(body):
    out = []
    for ln in body:
        t = ln.split(";")[0].strip()
        if not t or t.startswith(".") or t.endswith(":"):
            continue
        out.append(t.split()[0])
    return out


def digest(sym, body):
    lines = []
    for ln in body:
        if "__hip_cuid" in ln:
            continue
        ln = ln.replace(sym, "<kernel>")
        ln = re.sub(r"BB\d+_", "BB_", ln)  # labels (.LBB<n>_) and the loop comments that name them (BB<n>_)
        ln = re.sub(r"\.Lfunc_end\d+", ".Lfunc_end", ln)
        ln = re.sub(r"\s+;", " ;", ln)  # a comment's column moves with the digits of the label before it
        lines.append(ln.rstrip())
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16]


def kernarg_sizes(text):
    return {m.group(2): int(m.group(1)) for m in
            re.finditer(r"\.kernarg_segment_size:\s+(\d+)(?:(?!\.kernarg_segment_size)[\s\S])*?\.symbol:\s+(\S+)\.kd",
                        text)}


def family(dem):
    m = re.match(r"(?:void )?(?:\w+::)*(\w+)", dem)
    return m.group(1) if m else dem


def split_added(rows, pattern):
    """(rows to pair, rows whose demangled name matches pattern)"""
    if not pattern:
        return rows, []
    rx = re.compile(pattern)
    return [r for r in rows if not rx.search(r[1])], [r for r in rows if rx.search(r[1])]


def load(text):
    """[(family, demangled name, digest, metadata dict, mnemonics)] in file order"""
    meta = metadata(text)
    ka = kernarg_sizes(text)
    ks = list(kernels_of(text))
    dem = demangle([s for s, _ in ks])
    rows = []
    for sym, body in ks:
        m = dict(meta.get(sym, {}))
        m["kernarg"] = ka.get(sym, -1)
        d = re.sub(r"^void ", "", dem.get(sym, sym))
        rows.append((family(d), d, digest(sym, body), m, mnemonics(body)))
    return rows


def classify(a, b):
    if a[2] == b[2]:
        return "A"
    ma, mb = a[3], b[3]
    if any(ma.get(k) != mb.get(k) for k in META if k != "sgpr"):
        return "FAIL"
    na, nb = a[4], b[4]
    if collections.Counter(na) != collections.Counter(nb):
        return "FAIL"
    fa = next((i for i, x in enumerate(na) if x.startswith("v_mfma")), None)
    fb = next((i for i, x in enumerate(nb) if x.startswith("v_mfma")), None)
    if fa is None or fb is None or na[fa:] != nb[fb:]:
        return "FAIL"
    return "B"


def compare(old, new, out, brief=False):
    fams = []
    by = ({}, {})
    for side, rows in enumerate((old, new)):
        for r in rows:
            if r[0] not in fams:
                fams.append(r[0])
            by[side].setdefault(r[0], []).append(r)
    counts = collections.Counter()
    ok = True
    for f in fams:
        a, b = by[0].get(f, []), by[1].get(f, [])
        print("family %s: %d / %d kernels" % (f, len(a), len(b)), file=out)
        if brief and len(a) == len(b):  # one line per family: the classes, and one digest over the new side's, in order
            cl = collections.Counter(classify(x, y) for x, y in zip(a, b))
            print("  class A %d, class B %d, failed %d; digest of the digests %s" % (
                cl["A"], cl["B"], cl["FAIL"], hashlib.sha256(" ".join(y[2] for y in b).encode()).hexdigest()[:16]), file=out)
        if len(a) != len(b):
            print("  ERROR: the kernel counts differ", file=out)
            ok = False
            continue
        for n, (x, y) in enumerate(zip(a, b)):
            c = classify(x, y)
            counts[c] += 1
            ok = ok and c != "FAIL"
            if brief and c == "A":
                continue
            ms = " ".join("%s=%d" % (k, y[3].get(k, -1)) for k in META)
            print("  %3d %-4s %s %s  %s | old %s | new %s" % (n, c, x[2], y[2], ms, x[1], y[1]), file=out)
            if c != "A":
                print("           old metadata %s" % " ".join("%s=%d" % (k, x[3].get(k, -1)) for k in META), file=out)
                ca, cb = collections.Counter(x[4]), collections.Counter(y[4])
                print("           mnemonics %d -> %d: %s" % (len(x[4]), len(y[4]), " ".join(
                    "%s%+d" % (k, cb[k] - ca[k]) for k in sorted(set(ca) | set(cb)) if ca[k] != cb[k]) or "same multiset"),
                      file=out)
    print("class A %d, class B %d, failed %d; %s" % (counts["A"], counts["B"], counts["FAIL"],
                                                      "OK" if ok else "NOT EQUIVALENT"), file=out)
    return ok


def asm_of(path, flavor, keep, tag, sources):
    """assembly texts of a tree (compiled) or of one assembly file"""
    files = path.split(",")
    if all(os.path.isfile(f) for f in files):
        return [open(f).read() for f in files]
    kdir = os.path.join(path, "alphago_amd", "csrc", "kernels")
    with tempfile.TemporaryDirectory() as td:
        d = keep or td
        outs = [os.path.join(d, "%s_%s_%s.s" % (tag, flavor, s[:-4])) for s in sources]
        with ThreadPoolExecutor(len(outs)) as ex:
            list(ex.map(lambda so: compile_asm(os.path.join(kdir, so[0]), flavor, so[1]), zip(sources, outs)))
        return [open(o).read() for o in outs]


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--flavor", default="prod", choices=tuple(SOURCES))
    ap.add_argument("--sources", default="", help="files under alphago_amd/csrc/kernels, joined with commas, "
                    "instead of the flavour's conv sources")
    ap.add_argument("--out", default="", help="write the listing here instead of standard output")
    ap.add_argument("--keep", default="", help="keep the assembly files in this directory")
    ap.add_argument("--brief", action="store_true", help="one line per family; kernels are listed only outside class A")
    ap.add_argument("--added", default="", help="regular expression over demangled names: kernels of NEW that OLD "
                    "does not have (listed apart, not paired)")
    args = ap.parse_args()
    if args.keep:
        os.makedirs(args.keep, exist_ok=True)
    sources = args.sources.split(",") if args.sources else SOURCES[args.flavor]
    old = [r for t in asm_of(args.old, args.flavor, args.keep, "old", sources) for r in load(t)]
    new = [r for t in asm_of(args.new, args.flavor, args.keep, "new", sources) for r in load(t)]
    new, added = split_added(new, args.added)
    out = open(args.out, "w") if args.out else sys.stdout
    print("isa_compare %s build: %d / %d kernels" % (args.flavor, len(old), len(new)), file=out)
    for r in added:
        print("  added %s  %s | %s" % (r[2], " ".join("%s=%d" % (k, r[3].get(k, -1)) for k in META), r[1]), file=out)
    ok = compare(old, new, out, args.brief)
    if args.out:
        out.close()
        print(open(args.out).read().rstrip().split("\n")[-1])
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
