#!/usr/bin/env python3
"""Is the device code of two builds the same?  tools/codeobj_diff.py BUILD_DIR_A BUILD_DIR_B [unit ...]

For every unit (default: the thirteen objects of gusto.jl_amd/build) the gfx950 code object is taken out of UNIT.o of both
directories and compared symbol by symbol: the instruction bytes of every function of .text, the 64 bytes of every kernel
descriptor (.kd: VGPR / AGPR / SGPR granules, scratch, LDS, kernarg size) and the kernel's entry of the amdhsa metadata
note.  Symbol order and addresses may differ, bytes may not; __hip_cuid_<hash>, the one-byte tag hipcc names after a hash of
the unit's source, is left out.  One line per unit; exit status 1 on any difference.
Needs clang-offload-bundler, llvm-objcopy and llvm-readelf (ROCM_LLVM, default /opt/rocm/llvm/bin); no GPU."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
UNITS = ["gusto_hip", "shoot", "verify", "tvlqr", "simulate", "lincov"] + [f"model_{i}" for i in range(7)]


def run(*cmd):
    return subprocess.check_output(cmd, stderr=subprocess.DEVNULL).decode()


def code_object(obj, tmp):
    fat, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "co")
    for f in (fat, co):
        if os.path.exists(f):
            os.remove(f)
    try:
        run(f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", obj, os.devnull)
    except subprocess.CalledProcessError:
        return None                                       # a unit without device code: no such section
    run(f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}",
        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}")
    return co if os.path.getsize(co) else None


def symbols(co):
    """{name: bytes} of the functions and kernel descriptors, {kernel: metadata text} of the note"""
    raw = open(co, "rb").read()
    secs = {}
    for m in re.finditer(r"\[\s*(\d+)\]\s+(\S+)\s+\S+\s+([0-9a-f]{16})\s+([0-9a-f]+)\s+([0-9a-f]+)", run(f"{LLVM}/llvm-readelf", "-S", "-W", co)):
        secs[int(m.group(1))] = (int(m.group(3), 16), int(m.group(4), 16))
    out = {}
    for ln in run(f"{LLVM}/llvm-readelf", "-s", "-W", "--symbols", co).splitlines():
        f = ln.split()
        if len(f) == 8 and f[3] in ("FUNC", "OBJECT") and f[6].isdigit() and not f[7].startswith("__hip_cuid_"):
            addr, off = secs[int(f[6])]
            at = int(f[1], 16) - addr + off
            out[f[7]] = raw[at:at + int(f[2])]
    notes = run(f"{LLVM}/llvm-readelf", "--notes", "-W", co)
    meta = {}
    for blk in re.split(r"\n(?=\s*- \.(?:agpr_count|args):)", notes[notes.find("amdhsa.kernels"):notes.find("amdhsa.target")]):
        name = re.search(r"\.name:\s+(\S+)", blk)
        if name:
            meta[name.group(1)] = blk.strip()
    return out, meta


def main():
    a, b = sys.argv[1:3]
    units = sys.argv[3:] or UNITS
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        for u in units:
            ca = code_object(os.path.join(a, u + ".o"), tmp)
            ra = symbols(ca) if ca else ({}, {})
            cb = code_object(os.path.join(b, u + ".o"), tmp)
            rb = symbols(cb) if cb else ({}, {})
            diff = sorted(k for k in set(ra[0]) | set(rb[0]) if ra[0].get(k) != rb[0].get(k))
            mdiff = sorted(k for k in set(ra[1]) | set(rb[1]) if ra[1].get(k) != rb[1].get(k))
            nk = sum(k.endswith(".kd") for k in ra[0])
            print(f"{u}: {len(ra[0]) - nk} functions ({sum(len(v) for k, v in ra[0].items() if not k.endswith('.kd'))} bytes of .text), "
                  f"{nk} kernel descriptors, {len(ra[1])} metadata entries: " +
                  ("identical" if not diff and not mdiff else f"DIFFERENT {diff} {mdiff}"))
            bad += bool(diff or mdiff)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
