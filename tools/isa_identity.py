#!/usr/bin/env python3
"""Kernel-by-kernel comparison of two builds' device code from hipcc's -S output (no GPU needed).

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC --cuda-device-only -S \
          epidemicmodeling_amd/csrc/epiekf.hip -o new.s          (the flags of _build.py; the same for the other tree)
    python tools/isa_identity.py old.s new.s [--old LABEL] [--new LABEL] [--drop 'kernel:i,j' ...]

A kernel is its function (`.type <sym>,@function` ... `.Lfunc_end`), which holds its `.amdhsa_kernel <sym>` descriptor block
(registers, LDS, scratch).  Comments and the function index in local labels (`.LBB<n>_<m>`, `.Lfunc_end<n>`) are stripped.
--drop names template arguments (0-based) that the new build's kernel of that name no longer has: the old kernel is compared
with the new kernel of the name that is left.  Exit status 1 when a kernel differs or an old kernel has no partner that
--gone does not name."""
import argparse
import re
import subprocess
import sys


def demangle(syms):
    out = subprocess.run(["c++filt"] + syms, capture_output=True, text=True, stdin=subprocess.DEVNULL, timeout=120).stdout.split("\n")
    return [re.sub(r"^void ", "", re.sub(r"\(.*", "", n)).replace("epi::", "") for n in out[:len(syms)]]


def kernels(path):
    """{mangled: normalised text} of every kernel of an assembly file"""
    lines = open(path).read().split("\n")
    out = {}
    i = 0
    while i < len(lines):
        if (m := re.match(r"\s*\.type\s+(\S+),@function", lines[i])):
            sym = m.group(1)
            j = next(k for k in range(i, len(lines)) if re.match(r"\.Lfunc_end\d+:", lines[k]))
            if any(l.strip() == ".amdhsa_kernel " + sym for l in lines[i:j]):      # (hipcc puts the descriptor block ahead of .Lfunc_end)
                text = []
                for l in lines[i:j + 1]:
                    l = l.split(";")[0].strip()
                    l = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", l)
                    l = re.sub(r"\.Lfunc_end\d+", ".Lfunc_end", l)
                    if l:
                        text.append(l.replace(sym[2:], "SELF"))     # (the symbol is also part of the names of its LDS objects)
                out[sym] = text
            i = j
        i += 1
    return out


def drop_args(name, drops):
    m = re.match(r"^(\w+)<(.*)>$", name)
    if not m or m.group(1) not in drops:
        return name
    args = [a.strip() for a in m.group(2).split(",")]
    return "%s<%s>" % (m.group(1), ", ".join(a for k, a in enumerate(args) if k not in drops[m.group(1)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old_s")
    ap.add_argument("new_s")
    ap.add_argument("--old", default="old")
    ap.add_argument("--new", default="new")
    ap.add_argument("--drop", action="append", default=[], help="kernel:i,j -- template arguments the new build dropped")
    ap.add_argument("--gone", action="append", default=[], help="a kernel (demangled) that the new build is meant to lack")
    a = ap.parse_args()
    drops = {d.split(":")[0]: {int(x) for x in d.split(":")[1].split(",")} for d in a.drop}
    ko, kn = kernels(a.old_s), kernels(a.new_s)
    no = dict(zip(demangle(list(ko)), ko.values()))
    nn = dict(zip(demangle(list(kn)), kn.values()))
    print("old: %s   %d kernels" % (a.old, len(no)))
    print("new: %s   %d kernels" % (a.new, len(nn)))
    renamed, differ, missing, same = [], [], [], 0
    seen = set()
    for name, text in no.items():
        to = drop_args(name, drops)
        if to != name:
            renamed.append((name, to))
        if to not in nn:
            missing.append(name)
            continue
        seen.add(to)
        if text == nn[to]:
            same += 1
        else:
            differ.append((name, len(text), len(nn[to])))
    added = [n for n in nn if n not in seen]
    print("\nname map (old -> new, template arguments dropped): %d" % len(renamed))
    for o, n in renamed:
        print("  %-44s -> %s" % (o, n))
    print("\nkernels of the old build that the new one lacks: %d" % len(missing))
    for n in missing:
        print("  %s%s" % (n, "" if n in a.gone else "   UNEXPECTED"))
    print("\nkernels only in the new build: %d" % len(added))
    for n in added:
        print("  " + n)
    print("\nidentical (instructions and descriptor): %d" % same)
    print("differing: %d" % len(differ))
    for n, lo, ln in differ:
        print("  %s   (%d -> %d lines)" % (n, lo, ln))
    bad = differ or added or [n for n in missing if n not in a.gone] or [g for g in a.gone if g not in missing]
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
