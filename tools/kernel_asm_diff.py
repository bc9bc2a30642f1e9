#!/usr/bin/env python3
"""Compare the device assembly of kernels between two builds of one .hip file.

    hipcc <the library's flags> --cuda-device-only -S csrc/pr_batch.hip -o new.s     (this commit)
    hipcc <the library's flags> --cuda-device-only -S csrc/pr_batch.hip -o old.s     (the parent)
    tools/kernel_asm_diff.py old.s new.s --match 'k_batch_|k_btopk_'

For every kernel symbol of old.s whose demangled-or-not name matches --match, the instruction lines
between its label and its .Lfunc_end are compared with the kernel of the same symbol in new.s.
Set aside: comments, directives, block-label numbers (.LBB12_3 -> .LBB_3) and symbol names other
than the kernel's own (LDS variables are renamed by position).  Prints one line per kernel and a
summary; exits 1 when a kernel differs or is missing from new.s.  Also prints, with --resources,
the compiler's VGPR / SGPR / LDS / scratch / occupancy figures from the .s comments.
"""
import argparse
import re
import sys


def kernels(path):
    """symbol -> (instruction lines, resource dict) for every .amdhsa_kernel of the file."""
    lines = open(path).read().split("\n")
    names = [m.group(1) for l in lines if (m := re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l))]
    out = {}
    for name in names:
        start = next((i for i, l in enumerate(lines) if l.startswith(name + ":")), None)
        if start is None:
            continue
        body, res, i = [], {}, start + 1
        while i < len(lines) and not lines[i].startswith(".Lfunc_end"):
            body.append(lines[i])
            i += 1
        for l in lines[i: i + 80]:
            m = re.match(r"\s*;\s*(NumVgprs|NumAgprs|NumSgprs|ScratchSize|Occupancy|LDSByteSize|codeLenInByte)\s*[:=]\s*(\d+)", l)
            if m:
                res.setdefault(m.group(1), int(m.group(2)))
        out[name] = (body, res)
    return out


def normalise(body):
    syms = {}
    out = []
    for l in body:
        l = l.split(";")[0].rstrip()
        s = l.strip()
        if not s or (s.startswith(".") and not s.startswith(".LBB")):
            continue  # directives (.p2align, .loc, ...) and blanks
        l = re.sub(r"\.LBB\d+_", ".LBB_", s)
        # symbols of LDS variables and the like: named by order of first appearance
        l = re.sub(r"\b(_Z\w+|__hip\w+)", lambda m: syms.setdefault(m.group(1), f"sym{len(syms)}"), l)
        out.append(l)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--match", default=".")
    ap.add_argument("--resources", action="store_true")
    a = ap.parse_args()
    old, new = kernels(a.old), kernels(a.new)
    pat = re.compile(a.match)
    same = diff = 0
    for name in sorted(old):
        if not pat.search(name):
            continue
        if name not in new:
            print(f"MISSING  {name}")
            diff += 1
            continue
        x, y = normalise(old[name][0]), normalise(new[name][0])
        if x == y:
            same += 1
            print(f"same     {name}  ({len(x)} lines)")
        else:
            diff += 1
            first = next((i for i, (p, q) in enumerate(zip(x, y)) if p != q), min(len(x), len(y)))
            print(f"DIFFERS  {name}  ({len(x)} vs {len(y)} lines, first at {first})")
    added = sorted(n for n in new if pat.search(n) and n not in old)
    print(f"{same} kernels identical, {diff} differ or are missing, {len(added)} new")
    if a.resources:
        for name in sorted(new):
            if pat.search(name):
                r = new[name][1]
                print(f"{'new ' if name in added else '    '}{name}  " + "  ".join(f"{k}={v}" for k, v in r.items()))
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())
