#!/usr/bin/env python3
"""Instruction-level diff of two builds of libmatcha_hip.so, kernel by kernel: each gfx950 code object is disassembled
(llvm-objdump -d) and split by kernel symbol; per kernel the instruction count and the histogram of mnemonics are
compared. Kernels are matched as tools/kernel_regs.py matches them. Prints every kernel where either differs, with the
differing mnemonics and their counts (base->new), and a one-line summary. A refactor that leaves a kernel's code alone
shows nothing for it (register names and instruction order are not compared). CPU only.
Usage: python tools/isa_diff.py base.so new.so [name filter regex]"""
import collections
import os
import re
import subprocess
import sys
import tempfile

from kernel_regs import LLVM, code_objects, demangle, shorten


def histograms(so):
    """-> {demangled kernel name: Counter of mnemonics}"""
    hist = {}
    with tempfile.TemporaryDirectory() as td:
        for co in code_objects(so, td):
            # the kernels: function symbols with a kernel descriptor (NAME.kd); each one's code is [value, value + size),
            # which leaves out the padding up to the next symbol
            syms = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-s", "--wide", co], check=True,
                                  capture_output=True, text=True).stdout.split("\n")
            rows = [ln.split() for ln in syms if re.match(r"\s*\d+:", ln)]
            kds = {r[7][:-3] for r in rows if len(r) > 7 and r[7].endswith(".kd")}
            end = {r[7]: int(r[1], 16) + int(r[2]) for r in rows if len(r) > 7 and r[3] == "FUNC" and r[7] in kds}
            text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co], check=True,
                                  capture_output=True, text=True).stdout
            cur, lim = None, 0
            for line in text.splitlines():
                m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
                if m:  # a symbol: a kernel, a label inside the current one (kept with it), or something else
                    if m.group(1) in end:
                        cur, lim = hist.setdefault(m.group(1), collections.Counter()), end[m.group(1)]
                    continue
                m = re.match(r"^\s+(\S+).*// ([0-9A-Fa-f]+):", line)
                if m and cur is not None and int(m.group(2), 16) < lim:
                    cur[m.group(1)] += 1
    names = list(hist)
    return {d: hist[n] for n, d in zip(names, demangle(names))}


def main():
    base, new = histograms(sys.argv[1]), histograms(sys.argv[2])
    flt = re.compile(sys.argv[3]) if len(sys.argv) > 3 else None
    bshort = {shorten(k): v for k, v in base.items()}
    same = diff = only = 0
    for name, h in sorted(new.items()):
        if flt and not flt.search(name):
            continue
        b = base.get(name) or bshort.get(shorten(name))
        if b is None:
            only += 1
            print("NEW ", name, sum(h.values()), "instructions")
        elif b == h:
            same += 1
        else:
            diff += 1
            ms = sorted(m for m in set(b) | set(h) if b[m] != h[m])
            print("DIFF", name, f"instructions {sum(b.values())}->{sum(h.values())}:",
                  " ".join(f"{m} {b[m]}->{h[m]}" for m in ms))
    nshort = {shorten(n) for n in new}
    gone = [k for k in base if k not in new and shorten(k) not in nshort and (not flt or flt.search(k))]
    for k in gone:
        print("GONE", k)
    print(f"{same} kernels with equal instruction count and mnemonic histogram, {diff} that differ, {only} only in the "
          f"new build, {len(gone)} only in the base build")


if __name__ == "__main__":
    main()
