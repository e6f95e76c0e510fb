#!/usr/bin/env python
"""Epilogue listing of the conv forward / dgrad kernels.

Compiles csrc/kernels/conv.hip to gfx950 assembly with the flags of alphago_amd/_build.py (device
code only, nothing is linked or run) and prints, for every conv forward kernel in it, the
load / store / vmcnt-wait sequence after the last MFMA together with the kernel's register budget.

Legend: L = global load, S4 = 16-byte store, S = 8-byte store, s = 4-byte store, A = atomic,
wN = s_waitcnt with vmcnt(N), | = a branch or a branch target (control-flow join).
The sequence is in the order of the assembly text, which is the execution order except where the
compiler lays a row's body out of line (behind the kernel's s_endpgm).
`waits inside` counts the vmcnt waits between the first and the last store: each of them can make a
row's stores wait for the stores before it (vmcnt retires in issue order).

    python scripts/epilogue_listing.py [--flavor prod|lab] [--src conv.hip] [--keep out.s] [--match TEXT]

About 35 s per run (one hipcc -S of conv.hip).
"""
from __future__ import annotations

import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from alphago_amd import _build  # noqa: E402

MODES = {0: "bias+ReLU", 1: "mask", 2: "none", 3: "MASKBITS", 4: "bias+ReLU+res", 7: "MASKBITS+res"}


def compile_asm(src: str, flavor: str, out: str) -> None:
    common, hip_flags, inc_flags, _ = _build.hip_compile_flags(flavor)
    hipcc = os.path.join(_build.ROCM, "bin", "hipcc")
    cmd = [hipcc, "-x", "hip", *common, *hip_flags, *inc_flags, "--cuda-device-only", "-S", src, "-o", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise SystemExit("hipcc failed:\n" + r.stdout)


def demangle(names):
    filt = os.path.join(_build.ROCM, "llvm", "bin", "llvm-cxxfilt")
    if not os.path.exists(filt):
        filt = "c++filt"
    r = subprocess.run([filt], input="\n".join(names), stdout=subprocess.PIPE, text=True)
    out = r.stdout.split("\n")
    return dict(zip(names, out))


def short_name(dem: str) -> str:
    """conv_fwd_kernel<192, 0, agk::Tile386, false> -> conv_fwd_kernel<192, bias+ReLU, Tile386, 0>: the template
    arguments (a tile description may carry its own, WgradRow<192, 3>) without the namespace, bools as 0/1
    and the mode spelled out."""
    m = re.search(r"(conv_\w+)<", dem)
    if not m:
        return dem
    args, depth, cur = [], 1, ""
    for ch in dem[m.end():]:
        depth += (ch == "<") - (ch == ">")
        if depth == 0:
            break
        if ch == "," and depth == 1:
            args.append(cur)
            cur = ""
        else:
            cur += ch
    args.append(cur)
    args = [re.sub(r"\bfalse\b", "0", re.sub(r"\btrue\b", "1", re.sub(r"\bagk(_lab)?::", "", a.strip()))) for a in args]
    args = [re.sub(r"^\(\w+\)", "", a) for a in args]
    if len(args) > 1 and args[1].isdigit():
        args[1] = MODES.get(int(args[1]), args[1])
    return "%s<%s>" % (m.group(1), ", ".join(args))


def kernels_of(text: str):
    """yields (symbol, body lines) for every kernel (.amdhsa_kernel symbols) of an assembly file"""
    syms = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    lines = text.split("\n")
    starts = {}
    for n, ln in enumerate(lines):
        m = re.match(r"^([A-Za-z_]\w*):", ln)  # `symbol:   ; @symbol`
        if m:
            starts.setdefault(m.group(1), n)
    for s in syms:
        if s not in starts:
            continue
        body = []
        for ln in lines[starts[s] + 1:]:
            body.append(ln)
            if ln.startswith(".Lfunc_end"):  # not the first s_endpgm: row bodies may be laid out behind it
                break
        yield s, body


def metadata(text: str):
    """symbol -> dict of .vgpr_count / .sgpr_count / .agpr_count / scratch / spills from the amdhsa metadata"""
    out = {}
    for blk in re.split(r"\n\s*- \.agpr_count:", text)[1:]:
        blk = ".agpr_count:" + blk
        name = re.search(r"\.symbol:\s+(\S+)\.kd", blk)
        if not name:
            continue
        g = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))  # noqa: E731
        out[name.group(1)] = dict(agpr=g("agpr_count"), vgpr=g("vgpr_count"), sgpr=g("sgpr_count"),
                                  scratch=g("private_segment_fixed_size"), vspill=g("vgpr_spill_count"),
                                  sspill=g("sgpr_spill_count"), lds=g("group_segment_fixed_size"))
    return out


def epilogue_tokens(body):
    last = max((n for n, ln in enumerate(body) if "v_mfma" in ln), default=-1)
    toks = []
    for ln in body[last + 1:]:
        t = ln.strip()
        if not t or t.startswith(";"):
            continue
        op = t.split()[0]
        if re.match(r"^\.LBB\w+:", t) or op.startswith("s_cbranch") or op == "s_branch":
            if toks and toks[-1] != "|":
                toks.append("|")
        elif op.startswith(("global_load", "buffer_load", "flat_load")):
            toks.append("L")
        elif op.startswith(("global_atomic", "buffer_atomic", "flat_atomic")):
            toks.append("A")
        elif op.startswith(("global_store", "buffer_store", "flat_store")):
            toks.append("S4" if op.endswith("dwordx4") else "S" if op.endswith("dwordx2") else
                        "S3" if op.endswith("dwordx3") else "s")
        elif op == "s_waitcnt":
            m = re.search(r"vmcnt\((\d+)\)", t)
            if m:
                toks.append("w" + m.group(1))
        elif op.startswith("scratch_"):
            toks.append("SCRATCH")
    return toks


def compress(toks):
    out, i = [], 0
    while i < len(toks):
        j = i
        while j < len(toks) and toks[j] == toks[i]:
            j += 1
        out.append(toks[i] if j - i == 1 else "%sx%d" % (toks[i], j - i))
        i = j
    return " ".join(out)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--flavor", default="prod", choices=("prod", "debug", "lab"))
    ap.add_argument("--src", default="conv.hip", help="file under alphago_amd/csrc/kernels")
    ap.add_argument("--keep", default="", help="keep the assembly at this path")
    ap.add_argument("--asm", default="", help="read this assembly file instead of compiling")
    ap.add_argument("--match", default="conv_fwd", help="kernels whose demangled name contains this")
    args = ap.parse_args()

    if args.asm:
        text = open(args.asm).read()
    else:
        with tempfile.TemporaryDirectory() as td:
            out = args.keep or os.path.join(td, "listing.s")
            compile_asm(os.path.join(_build.CSRC, "kernels", args.src), args.flavor, out)
            text = open(out).read()
    meta = metadata(text)
    ks = list(kernels_of(text))
    dem = demangle([s for s, _ in ks])
    rows = []
    for sym, body in ks:
        d = dem.get(sym, sym)
        if args.match not in d:
            continue
        toks = epilogue_tokens(body)
        st = [n for n, t in enumerate(toks) if t[0] in "Ss" and t != "SCRATCH"]
        inside = [t for t in toks[st[0]:st[-1]] if t[0] == "w"] if st else []
        nstore = {k: toks.count(k) for k in ("S4", "S", "s")}
        rows.append((short_name(d), meta.get(sym, {}), toks, inside, nstore))
    rows.sort(key=lambda r: r[0])
    print("%d kernels (%s, %s build)" % (len(rows), args.src, args.flavor))
    bad = 0
    for name, m, toks, inside, ns in rows:
        print()
        print(name)
        if m:
            print("  VGPRs %d  AGPRs %d  SGPRs %d  scratch %d B  spills %d/%d  LDS %d B" %
                  (m["vgpr"], m["agpr"], m["sgpr"], m["scratch"], m["vspill"], m["sspill"], m["lds"]))
        print("  stores: %d x 16 B, %d x 8 B, %d x 4 B;  vmcnt waits inside the store sequence: %d%s" %
              (ns["S4"], ns["S"], ns["s"], len(inside), (" (" + " ".join(inside) + ")") if inside else ""))
        print("  " + compress(toks))
        bad += bool(inside)
    print()
    print("kernels with a vmcnt wait between their first and last epilogue store: %d of %d" % (bad, len(rows)))


if __name__ == "__main__":
    main()
