#!/usr/bin/env python3
"""Register allocation of two builds of libmatcha_hip.so, kernel by kernel, from the gfx950 code object's metadata
(.sgpr_count, .vgpr_count, .sgpr_spill_count, .vgpr_spill_count, .private_segment_fixed_size = scratch bytes per lane,
.group_segment_fixed_size = LDS bytes per workgroup).
Kernels are matched by demangled name; a template argument list the newer build extended with trailing defaulted
arguments (..., 0>) matches its shorter form. Prints every kernel whose figures differ, the kernels only one build
has (with their spills), and a summary. CPU only.
Usage: python tools/kernel_regs.py base.so new.so [name filter regex]"""
import os
import re
import subprocess
import sys
import tempfile

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
LLVM = os.path.join(ROCM, "llvm", "bin")
FIELDS = (".sgpr_count", ".vgpr_count", ".sgpr_spill_count", ".vgpr_spill_count", ".private_segment_fixed_size",
          ".group_segment_fixed_size")


def code_objects(so, td):
    """Writes the gfx950 code objects of library `so` into directory td; -> their paths (tools/isa_diff.py too)."""
    # the library's .hip_fatbin section holds one uncompressed offload bundle per translation unit: magic, entry count,
    # then (offset, size, triple length, triple) per entry
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    fb = os.path.join(td, "fatbin")
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", so, fb], check=True)
    blob = open(fb, "rb").read()
    pos, cos = blob.find(magic), []
    assert pos >= 0, f"{so}: no uncompressed offload bundle in .hip_fatbin"
    while pos >= 0:
        cnt = int.from_bytes(blob[pos + 24:pos + 32], "little")
        p = pos + 32
        for _ in range(cnt):
            off, size, tl = (int.from_bytes(blob[p + 8 * i:p + 8 * i + 8], "little") for i in range(3))
            triple = blob[p + 24:p + 24 + tl].decode()
            p += 24 + tl
            if "gfx950" in triple and size:
                cos.append(os.path.join(td, f"co{len(cos)}"))
                open(cos[-1], "wb").write(blob[pos + off:pos + off + size])
        pos = blob.find(magic, pos + 24)
    return cos


def demangle(names):
    filt = os.path.join(LLVM, "llvm-cxxfilt")
    return subprocess.run([filt if os.path.exists(filt) else "c++filt"], input="\n".join(names), capture_output=True,
                          text=True, check=True).stdout.splitlines()


def kernels(so):
    with tempfile.TemporaryDirectory() as td:
        notes = "".join(subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True,
                                       capture_output=True, text=True).stdout for co in code_objects(so, td))
    # amdhsa.kernels is a list of maps with sorted keys: a record starts at a "- " item of the list's own indentation
    # (its .args items sit deeper), and its fields come before as well as after its .name
    out, rec, ind = {}, None, None
    for line in notes.splitlines():
        if "amdhsa.kernels:" in line:
            ind = -1
            continue
        m = re.match(r"(\s*)(- )?(\.[a-z_]+):\s*(.*)$", line)
        if not m or ind is None:
            if not m and not line.startswith(" "):  # the list has ended
                ind = None
            continue
        col = len(m.group(1))
        if m.group(2) and ind in (-1, col):
            ind, rec = col, {}
        if rec is None or col + (2 if m.group(2) else 0) != ind + 2:
            continue
        k, v = m.group(3), m.group(4).strip()
        if k == ".name":
            out[v.strip("'\"")] = rec
        elif k in FIELDS:
            rec[k] = int(v)
    names = list(out)
    return {d: out[n] for n, d in zip(names, demangle(names)) if out[n]}


def shorten(name):
    prev = None
    while prev != name:
        prev = name
        name = re.sub(r", 0>", ">", name)
    return name


def main():
    base, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    flt = re.compile(sys.argv[3]) if len(sys.argv) > 3 else None
    bshort = {shorten(k): v for k, v in base.items()}
    same = diff = 0
    only_new = []
    for name, v in sorted(new.items()):
        if flt and not flt.search(name):
            continue
        b = base.get(name) or bshort.get(shorten(name))
        if b is None:
            only_new.append((name, v))
        elif b == v:
            same += 1
        else:
            diff += 1
            print("DIFF", name, " ".join(f"{f[1:]} {b.get(f)}->{v.get(f)}" for f in FIELDS if b.get(f) != v.get(f)))
    wt_same = 0
    for name, v in only_new:
        # a write-through instantiation (store policy 16 as the last template argument; mt_vconv: flag 262144 in the
        # first) against its plain twin of the same build
        t = re.sub(r"(, |<)16>\(", lambda m: m.group(1) + "0>(", name)
        m = re.search(r"vconv_kernel<(\d+),", name)
        if m and int(m.group(1)) & 262144:
            t = name.replace(m.group(0), f"vconv_kernel<{int(m.group(1)) & ~262144},", 1)
        tw = new.get(t) if t != name else None
        if tw is not None and tw == v:
            wt_same += 1
        elif tw is not None:
            print("WT  ", name, " ".join(f"{f[1:]} {tw.get(f)}->{v.get(f)}" for f in FIELDS if tw.get(f) != v.get(f)))
        else:
            print("NEW ", name, " ".join(f"{f[1:]} {v.get(f)}" for f in FIELDS))
    print(f"{wt_same} write-through instantiations with their plain twin's figures")
    gone = [k for k in base if k not in new and shorten(k) not in {shorten(n) for n in new}]
    for k in gone:
        if not flt or flt.search(k):
            print("GONE", k)
    print(f"{same} kernels with identical figures, {diff} that differ, {len(only_new)} only in the new build, "
          f"{len(gone)} only in the base build")


if __name__ == "__main__":
    main()
