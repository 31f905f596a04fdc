#!/usr/bin/env python
"""Fingerprint the device code of csrc translation units, kernel by kernel: each source is
compiled for the device only with the project's flags (_build.HIPCC_FLAGS + FILE_FLAGS, csrc on
the include path), and for every kernel of the code object one line is printed --

  <mangled name> <code bytes> <sha256 of its bytes in .text> <sha256 of its 64-byte .kd descriptor>

(the first 128 bits of each sha256, as 32 hex digits, to keep committed listings small)

sorted by name, after a `# file` line per source. The descriptor is hashed with its
kernel_code_entry_byte_offset (bytes 16..23: the distance from the descriptor to the code, which
moves with every other kernel of the file) zeroed; the rest -- LDS and scratch sizes, kernarg
size, the register and feature words -- is the kernel's own (a listing says nothing about the
entry offset itself; the loader resolves it, and the kernel's tests cover it). Two listings that
agree line for line (the `#` lines aside) hold the same machine code and the same launch
descriptors, so a refactor that only moves kernels between files can show that it moved them
and nothing else.

  python tools/kernel_code_hashes.py graphconvgeo_amd/csrc/dense_*.hip > after.txt
  python tools/kernel_code_hashes.py --flag=-fno-slp-vectorize /elsewhere/old.hip > before.txt
"""
import argparse
import concurrent.futures as cf
import hashlib
import os
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from graphconvgeo_amd import _build  # noqa: E402


def llvm_tool(name):
    """llvm-objdump / llvm-objcopy: LLVM_BIN if set, beside the hipcc in use, /opt/rocm, PATH."""
    root = os.path.dirname(os.path.dirname(os.path.realpath(_build._hipcc())))
    dirs = [os.environ.get("LLVM_BIN"), os.path.join(root, "llvm", "bin"),
            os.path.join(root, "lib", "llvm", "bin"), "/opt/rocm/llvm/bin"]
    for d in dirs:
        if d and os.path.exists(os.path.join(d, name)):
            return os.path.join(d, name)
    found = shutil.which(name)
    if found is None:
        raise SystemExit(f"{name} not found (set LLVM_BIN to the directory that holds it)")
    return found


def tool(name, *args):
    return subprocess.run([llvm_tool(name), *args], check=True, capture_output=True,
                          text=True).stdout


def sections(co):
    """name -> (vma, bytes) of the code object's .text and .rodata."""
    out = {}
    for line in tool("llvm-objdump", "-h", co).splitlines():
        f = line.split()
        if len(f) >= 5 and f[1] in (".text", ".rodata"):
            raw = co + f[1] + ".bin"
            tool("llvm-objcopy", "-O", "binary", f"--only-section={f[1]}", co, raw)
            with open(raw, "rb") as fh:
                out[f[1]] = (int(f[3], 16), fh.read())
    return out


def kernels(co):
    """[(name, size, code sha256, descriptor sha256)] of one code object."""
    sec = sections(co)
    sym = {}  # name -> (section, address, size)
    for line in tool("llvm-objdump", "-t", co).splitlines():
        f = line.split()  # address, flags, section, size, [visibility,] name
        at = [i for i, w in enumerate(f[:-2]) if w in sec]
        if at:
            sym[f[-1]] = (f[at[0]], int(f[0], 16), int(f[at[0] + 1], 16))

    def digest(name, zero=(0, 0)):
        s, addr, size = sym[name]
        vma, data = sec[s]
        b = bytearray(data[addr - vma:addr - vma + size])
        b[zero[0]:zero[1]] = bytes(zero[1] - zero[0])
        return hashlib.sha256(b).hexdigest()[:32]

    rows = []
    for kd in sorted(n for n in sym if n.endswith(".kd")):
        name = kd[:-3]
        assert sym[kd][2] == 64 and name in sym, kd
        rows.append((name, sym[name][2], digest(name), digest(kd, (16, 24))))
    return rows


def compile_device(src, extra, tmpd):
    name = os.path.basename(src)
    co = os.path.join(tmpd, name + ".co")
    cmd = [_build._hipcc(), *_build.HIPCC_FLAGS, *_build.FILE_FLAGS.get(name, []), *extra,
           f"-I{_build.CSRC}", '-DGCG_SOURCE_HASH="hashes"', "--cuda-device-only",
           "--no-gpu-bundle-output", "-c", "-o", co, src]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise SystemExit(f"hipcc failed on {src}:\n{res.stderr}")
    return co


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("sources", nargs="+")
    ap.add_argument("--flag", action="append", default=[],
                    help="extra hipcc flag, for a file FILE_FLAGS does not name")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory(prefix="gcg_hashes_") as tmpd:
        with cf.ThreadPoolExecutor(max_workers=min(len(a.sources), 8)) as ex:
            cos = list(ex.map(lambda s: compile_device(s, a.flag, tmpd), a.sources))
        for src, co in zip(a.sources, cos):
            rows = kernels(co)
            print(f"# {os.path.basename(src)}: {len(rows)} kernels")
            for name, size, code, kd in rows:
                print(name, size, code, kd)


if __name__ == "__main__":
    main()
