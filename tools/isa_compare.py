#!/usr/bin/env python3
"""Per-kernel resource figures of two ISA listings of geodesic.hip, side by side.

    make -C schwarzschild-raytracer_amd isa     # build/geodesic.s of a tree
    tools/isa_compare.py PARENT.s NEW.s [--drop-trailing N] > isa_compare.txt

Kernels are matched by demangled name. A tree that appended template
parameters (with defaults) to a kernel names the parent's instantiations with
that many more arguments: --drop-trailing N also tries each new name with its
last 1 .. N template arguments dropped. Exit status 1 when a parent kernel is
missing from the new listing or any of its figures differs.
"""
from __future__ import annotations

import argparse
import re
import subprocess
import sys

FIGURES = ["NumVgprs", "NumAgprs", "TotalNumSgprs", "vgpr_spill", "sgpr_spill", "ScratchSize", "LDSByteSize",
           "Occupancy", "codeLenInByte"]


def demangle(names: list[str]) -> list[str]:
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    return [re.sub(r"\(.*$", "", line).strip() for line in out.splitlines()]


def kernels(path: str) -> dict[str, dict[str, int]]:
    text = open(path).read()
    figs: dict[str, dict[str, int]] = {}
    # the comment block the assembler printer puts behind each kernel
    current, block = None, None
    for line in text.splitlines():
        m = re.search(r"; -- Begin function (\S+)", line)
        if m:
            current = m.group(1)
        elif line.startswith("; Kernel info:"):
            block = figs.setdefault(current, {})
        elif block is not None:
            m = re.match(r"^; (\w+)\s*[:=]\s*(\d+)", line)
            if m:
                block[m.group(1)] = int(m.group(2))
            elif not line.startswith(";"):
                block = None
    # the spill counts are in the code object's metadata only
    for m in re.finditer(r"^    \.name:\s+(\S+)\n(.*?)^    \.wavefront_size", text, re.M | re.S):
        if m.group(1) in figs:
            for key in ("sgpr_spill", "vgpr_spill"):
                v = re.search(r"\.%s_count:\s+(\d+)" % key, m.group(2))
                figs[m.group(1)][key] = int(v.group(1)) if v else -1
    names = list(figs)
    return {d: figs[n] for n, d in zip(names, demangle(names))}


def drop_args(name: str, n: int) -> str:
    m = re.match(r"^(.*)<(.*)>$", name)
    if not m:
        return name
    args = [a.strip() for a in m.group(2).split(",")]
    return name if n >= len(args) else "%s<%s>" % (m.group(1), ", ".join(args[: len(args) - n]))


def row(d: dict[str, int]) -> str:
    return " ".join(str(d.get(k, -1)) for k in FIGURES)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--drop-trailing", type=int, default=0)
    a = ap.parse_args()
    old, new = kernels(a.parent), kernels(a.new)
    matched: dict[str, str] = {}
    for name in new:
        for n in range(a.drop_trailing + 1):
            short = drop_args(name, n)
            if short in old and short not in matched:
                matched[short] = name
                break
    print("kernel | " + " ".join(FIGURES))
    differing = 0
    for name, figs in old.items():
        if name not in matched:
            print("GONE %s | %s" % (name, row(figs)))
            differing += 1
        elif row(new[matched[name]]) == row(figs):
            print("SAME %s | %s" % (name, row(figs)))
        else:
            print("DIFF %s | %s -> %s" % (name, row(figs), row(new[matched[name]])))
            differing += 1
    print("--- new kernels")
    for name, figs in new.items():
        if name not in matched.values():
            print("NEW  %s | %s" % (name, row(figs)))
    print("parent kernels: %d new listing's kernels: %d differing: %d" % (len(old), len(new), differing))
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main())
