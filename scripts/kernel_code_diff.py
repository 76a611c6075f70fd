#!/usr/bin/env python3
"""Compare the machine code of the kernels in two sets of gfx950 code objects.

    scripts/kernel_code_diff.py --old OLD... --new NEW... [-D MACRO]...

OLD / NEW are device code objects (the output of `hipcc --cuda-device-only -c`) or `.hip` sources, which are first
compiled device-only with the flags of mvster_amd/csrc/Makefile (plus the -D macros).  A kernel is a FUNC symbol with a
`<name>.kd` descriptor beside it; per kernel the symbol's bytes and the descriptor (registers, LDS, scratch, launch
bounds; all 64 bytes but the offset from descriptor to code, which is the linker's layout) are compared over the union of
each side's files.  A kernel defined in two files of one side is an error
of its own.  Prints one summary line and the names that differ; exit status 0 only for "0 differ" with equal name sets.

This is how a pure restructuring of a translation unit is checked without a GPU: split or shared source, same bytes.
"""
import argparse
import os
import shutil
import struct
import subprocess
import sys
import tempfile

DEVICE_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only"]
STT_OBJECT, STT_FUNC = 1, 2
BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def compile_device(src, out, defines=(), hipcc=None):
    """src (.hip) -> device code object `out`, the library's flags."""
    hipcc = hipcc or os.environ.get("HIPCC") or shutil.which("hipcc") or \
        os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    subprocess.run([hipcc, *DEVICE_FLAGS, *[f"-D{d}" for d in defines], "-c", src, "-o", out], check=True)
    return out


def read_kernels(path):
    """{kernel name: (code bytes, descriptor bytes)} of one ELF64 little-endian code object."""
    with open(path, "rb") as f:
        data = f.read()
    if data.startswith(BUNDLE_MAGIC):       # hipcc -c wraps the device ELF: [offset, size, len(triple), triple] per entry
        pos, device = len(BUNDLE_MAGIC) + 8, None
        for _ in range(struct.unpack_from("<Q", data, len(BUNDLE_MAGIC))[0]):
            off, size, tlen = struct.unpack_from("<QQQ", data, pos)
            if data[pos + 24:pos + 24 + tlen].startswith(b"hip") and size:
                device = data[off:off + size]
            pos += 24 + tlen
        if device is None:
            raise ValueError(f"{path}: offload bundle without a device code object")
        data = device
    if data[:6] != b"\x7fELF\x02\x01":
        raise ValueError(f"{path}: not a 64-bit little-endian ELF file")
    shoff, = struct.unpack_from("<Q", data, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", data, 0x3A)
    sections = []       # (type, addr, offset, size, link, entsize)
    for i in range(shnum):
        _, typ, _, addr, off, size, link, _, _, entsize = struct.unpack_from("<IIQQQQIIQQ", data, shoff + i * shentsize)
        sections.append((typ, addr, off, size, link, entsize))
    symtab = next((s for s in sections if s[0] == 2), None)      # SHT_SYMTAB
    if symtab is None:
        raise ValueError(f"{path}: no symbol table")
    _, _, soff, ssize, slink, sent = symtab
    stroff = sections[slink][2]
    symbols = {}        # name -> (type, bytes)
    for o in range(soff, soff + ssize, sent):
        name, info, _, shndx, value, size = struct.unpack_from("<IBBHQQ", data, o)
        typ = info & 0xF
        if typ not in (STT_OBJECT, STT_FUNC) or shndx == 0 or shndx >= shnum:
            continue
        end = data.index(b"\0", stroff + name)
        _, saddr, sfile, _, _, _ = sections[shndx]
        start = sfile + (value - saddr)
        symbols[data[stroff + name:end].decode()] = (typ, data[start:start + size])
    kernels = {}
    for name, (typ, code) in symbols.items():
        kd = symbols.get(name + ".kd")
        if typ == STT_FUNC and kd is not None and kd[0] == STT_OBJECT:
            # (bytes 16..23 of a descriptor are the distance from it to the code: where the linker put the two, not the kernel)
            kernels[name] = (code, kd[1][:16] + kd[1][24:])
    return kernels


def union_kernels(paths):
    """Kernels of several code objects; (merged dict, names defined in more than one file)."""
    merged, twice = {}, []
    for p in paths:
        for name, k in read_kernels(p).items():
            if name in merged:
                twice.append(name)
            merged[name] = k
    return merged, sorted(twice)


def compare(old_paths, new_paths):
    """-> dict(old, new: kernel counts; only_old, only_new, differ, twice: sorted name lists)."""
    old, twice_old = union_kernels(old_paths)
    new, twice_new = union_kernels(new_paths)
    return {
        "old": len(old),
        "new": len(new),
        "only_old": sorted(set(old) - set(new)),
        "only_new": sorted(set(new) - set(old)),
        "differ": sorted(n for n in set(old) & set(new) if old[n] != new[n]),
        "twice": sorted(set(twice_old + twice_new)),
    }


def identical(r):
    return not (r["only_old"] or r["only_new"] or r["differ"] or r["twice"])


def report(r):
    lines = [f"kernels: {r['old']} old, {r['new']} new; {len(r['only_old'])} only old, {len(r['only_new'])} only new, "
             f"{len(r['twice'])} defined twice, {len(r['differ'])} differ"]
    for key in ("only_old", "only_new", "twice", "differ"):
        lines += [f"  {key}: {n}" for n in r[key]]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--old", nargs="+", required=True)
    ap.add_argument("--new", nargs="+", required=True)
    ap.add_argument("-D", dest="defines", action="append", default=[], help="macro for the .hip inputs")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        def objects(paths, side):
            return [compile_device(p, os.path.join(tmp, f"{side}{i}.co"), args.defines) if p.endswith(".hip") else p
                    for i, p in enumerate(paths)]
        r = compare(objects(args.old, "old"), objects(args.new, "new"))
    print(report(r))
    return 0 if identical(r) else 1


if __name__ == "__main__":
    sys.exit(main())
