"""Instruction classes of a kernel's loops, read from the gfx950 code object inside libmpcbatch.so (no GPU, no recompilation).
    python tools/isa_census.py [--so path/to/libmpcbatch.so | --elf code_object] [--kernel 'mpcb_kernel_kin<1, false, false>']
                               [--trips L3=7,L5=15] [--root L2]
A loop is a backward branch: the instructions from its target to the branch.  Every loop is listed in address order with its nesting
depth, its static class counts (the whole range) and the counts of its own body without the loops inside it.  --trips gives trip
counts of inner loops; with --root the tool then prints the dynamic count of ONE trip of that loop: its own body once, every loop
inside it times its trip count (default 1).  Classes only: FP64 arithmetic, other VALU, lane reads (v_readlane / v_readfirstlane),
v_writelane, v_accvgpr moves, DPP moves, DS reads / writes, scalar ALU, scalar memory, vector memory, s_waitcnt."""
import argparse
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools import kernel_resources as kr   # noqa: E402

CLASSES = ["fp64", "valu_other", "lane_read", "writelane", "accvgpr", "dpp", "ds_read", "ds_write", "salu", "smem", "vmem", "waitcnt", "other"]
_FP64 = re.compile(r"^v_(add|mul|fma|fmac|max|min|rcp|rsq|sqrt|div_scale|div_fmas|div_fixup|ldexp|frexp_mant|trunc|floor|ceil|rndne|fract)_f64")


def classify(mnemonic, operands):
    m = mnemonic
    if m.startswith("s_waitcnt"):
        return "waitcnt"
    if m.startswith("v_readlane") or m.startswith("v_readfirstlane"):
        return "lane_read"
    if m.startswith("v_writelane"):
        return "writelane"
    if m.startswith("v_accvgpr"):
        return "accvgpr"
    if m.startswith("ds_"):
        return "ds_write" if ("write" in m or "store" in m) else "ds_read"      # (ds_bpermute / ds_swizzle count as reads: they return data)
    if m.startswith("v_"):
        if m.endswith("_dpp") or "quad_perm" in operands or "row_" in operands:
            return "dpp"
        return "fp64" if _FP64.match(m) else "valu_other"
    if m.startswith("s_load") or m.startswith("s_buffer_load"):
        return "smem"
    if m.startswith("global_") or m.startswith("buffer_") or m.startswith("flat_") or m.startswith("scratch_"):
        return "vmem"
    if m.startswith("s_"):
        return "salu"
    return "other"


def instructions(dis_text, mangled):
    """[(offset, class, branch target offset or None)] of one function of an llvm-objdump -d listing."""
    out, on, base = [], False, None
    for line in dis_text.splitlines():
        m = re.match(r"^([0-9a-f]+) <(\S+)>:", line)
        if m:
            on = m.group(2) == mangled
            base = int(m.group(1), 16)
            continue
        if not on:
            continue
        m = re.match(r"^\s+(\S+)\s*(.*?)\s*// ([0-9A-F]+):", line)
        if not m:
            continue
        mnem, ops, addr = m.group(1), m.group(2), int(m.group(3), 16)
        tgt = None
        if mnem.startswith("s_cbranch") or mnem == "s_branch":
            t = re.search(r"<%s\+0x([0-9a-f]+)>" % re.escape(mangled), line)
            tgt = int(t.group(1), 16) if t else (0 if "<%s>" % mangled in line else None)
        out.append((addr - base, classify(mnem, ops), tgt))
    return out


def loops(ins):
    """Back edges as (start, end) offset ranges, merged per loop header, in address order."""
    by_head = {}
    for off, _, tgt in ins:
        if tgt is not None and tgt <= off:
            by_head[tgt] = max(by_head.get(tgt, 0), off)
    # back edges whose ranges overlap without nesting (several latches or exits of one loop after block placement) are one loop
    ls = sorted(by_head.items())
    merged = True
    while merged:
        merged = False
        for i in range(len(ls)):
            for j in range(i + 1, len(ls)):
                (a0, a1), (b0, b1) = ls[i], ls[j]
                if a0 < b0 <= a1 < b1 or (a0 == b0 and a1 != b1) or (a1 == b1 and a0 != b0):
                    ls[i] = (min(a0, b0), max(a1, b1)); del ls[j]
                    merged = True
                    break
            if merged:
                break
    return sorted(set(ls))


def count(ins, lo, hi, holes=()):
    c = dict.fromkeys(CLASSES, 0)
    for off, cl, _ in ins:
        if lo <= off <= hi and not any(a <= off <= b for a, b in holes):
            c[cl] += 1
    return c


def census(ins, trips=None, root=None):
    ls = loops(ins)
    names = ["L%d" % i for i in range(len(ls))]
    inside = lambda a, b: b[0] <= a[0] and a[1] <= b[1] and a != b   # noqa: E731
    children = {n: [m for m, r in zip(names, ls) if inside(r, ls[i]) and not any(inside(r, q) and inside(q, ls[i]) for q in ls)]
                for i, n in enumerate(names)}
    lines = ["# loop  depth  range                 " + " ".join("%10s" % c for c in CLASSES) + "        all"]
    own = {}
    for i, n in enumerate(names):
        depth = sum(inside(ls[i], q) for q in ls)
        tot = count(ins, *ls[i])
        own[n] = count(ins, ls[i][0], ls[i][1], [ls[names.index(m)] for m in children[n]])
        for tag, c in (("all", tot), ("own", own[n])):
            lines.append("%-5s %s %5d  0x%05x-0x%05x       " % (n, tag, depth, ls[i][0], ls[i][1]) + " ".join("%10d" % c[k] for k in CLASSES) + " %10d" % sum(c.values()))
    if root:
        trips = trips or {}

        def dyn(n):
            c = dict(own[n])
            for m in children[n]:
                d = dyn(m)
                for k in CLASSES:
                    c[k] += trips.get(m, 1) * d[k]
            return c
        c = dyn(root)
        lines.append("# one trip of %s with inner trip counts %s" % (root, ",".join("%s=%d" % kv for kv in sorted(trips.items())) or "all 1"))
        lines.append("dynamic                                  " + " ".join("%10d" % c[k] for k in CLASSES) + " %10d" % sum(c.values()))
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--so", default=kr.DEFAULT_SO)
    ap.add_argument("--elf", help="an already extracted gfx950 code object instead of a library")
    ap.add_argument("--kernel", default="mpcb_kernel_kin<1, false, false>")
    ap.add_argument("--trips", default="")
    ap.add_argument("--root")
    a = ap.parse_args()
    co = a.elf or kr.code_object(a.so)
    syms = subprocess.run([os.path.join(kr.LLVM, "llvm-readelf"), "-s", "-W", co], check=True, capture_output=True, text=True).stdout
    funcs = sorted({l.split()[7] for l in syms.splitlines() if len(l.split()) >= 8 and l.split()[3] == "FUNC"})
    mangled = dict(zip(kr.demangle(funcs), funcs)).get(a.kernel)
    if mangled is None:
        sys.exit("no kernel %r in %s" % (a.kernel, co))
    dis = subprocess.run([os.path.join(kr.LLVM, "llvm-objdump"), "-d", co], check=True, capture_output=True, text=True).stdout
    trips = {k: int(v) for k, v in (kv.split("=") for kv in a.trips.split(",") if kv)}
    print("# %s" % a.kernel)
    print(census(instructions(dis, mangled), trips, a.root))


if __name__ == "__main__":
    main()
