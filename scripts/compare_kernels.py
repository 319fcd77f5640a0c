#!/usr/bin/env python3
"""Compare the device code of two builds kernel by kernel (no GPU needed).

    scripts/compare_kernels.py BUILD_DIR_A BUILD_DIR_B [--arch gfx950]

For every *.hip.o of each directory: unbundle the device code object, take
every FUNC symbol and every `.kd` kernel descriptor from `llvm-readelf -sW`,
and hash its bytes from its section.  The union over all objects, {symbol:
hash}, must be equal as maps: the same kernels, each with the same machine
code and the same descriptor.  Whole-object comparison is not the criterion:
instantiation order moves kernels around inside .text.

One field of a descriptor depends on the layout and not on the kernel:
kernel_code_entry_byte_offset (bytes 16-23), the distance from the descriptor
to the code.  It is checked to point at the FUNC symbol of the same name and
left out of the hash.

Exit status 0 when the maps are equal, 1 otherwise.
"""
import argparse
import glob
import hashlib
import os
import shutil
import struct
import subprocess
import sys
import tempfile


def tool(name):
    p = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", name)
    p = p if os.path.exists(p) else shutil.which(name)
    if not p:
        sys.exit(f"{name} not found")
    return p


def sections(readelf, path):
    """{section index: (address, file offset, size, type)}"""
    out = {}
    text = subprocess.run([readelf, "-SW", path], check=True, capture_output=True, text=True).stdout
    for line in text.splitlines():
        line = line.strip()
        if not line.startswith("["):
            continue
        idx, rest = line[1:].split("]", 1)
        f = rest.split()
        if not idx.strip().isdigit() or len(f) < 5 or f[0] == "NULL":
            continue
        # Name Type Address Off Size ...
        out[int(idx)] = (int(f[2], 16), int(f[3], 16), int(f[4], 16), f[1])
    return out


def symbols(readelf, path):
    """[(name, value, size, type, section index)] of the defined symbols"""
    out = []
    text = subprocess.run([readelf, "-sW", path], check=True, capture_output=True, text=True).stdout
    for line in text.splitlines():
        f = line.split()
        # Num: Value Size Type Bind Vis Ndx Name
        if len(f) < 8 or not f[0].rstrip(":").isdigit() or not f[6].isdigit():
            continue
        out.append((f[7], int(f[1], 16), int(f[2]), f[3], int(f[6])))
    return out


def object_kernels(tools, obj, arch, tmp):
    bundler, readelf, objcopy = tools
    # the host object carries the offload bundle in its .hip_fatbin section
    fb = os.path.join(tmp, os.path.basename(obj) + ".fatbin")
    co = os.path.join(tmp, os.path.basename(obj) + ".co")
    subprocess.run([objcopy, f"--dump-section=.hip_fatbin={fb}", obj], check=True, capture_output=True)
    subprocess.run([bundler, "--unbundle", "--type=o", f"--targets=hipv4-amdgcn-amd-amdhsa--{arch}",
                    f"--input={fb}", f"--output={co}"], check=True, capture_output=True)
    data = open(co, "rb").read()
    if not data:
        return {}
    secs = sections(readelf, co)
    syms = symbols(readelf, co)
    funcs = {name: value for name, value, _, typ, _ in syms if typ == "FUNC"}
    out = {}
    for name, value, size, typ, ndx in syms:
        kd = name.endswith(".kd") and typ == "OBJECT"
        if typ != "FUNC" and not kd:
            continue
        addr, off, ssize, stype = secs[ndx]
        if stype == "NOBITS" or value < addr or value + size > addr + ssize:
            sys.exit(f"{obj}: {name} lies outside its section")
        b = bytearray(data[off + value - addr: off + value - addr + size])
        if kd:
            if size != 64:
                sys.exit(f"{obj}: {name}: descriptor of {size} bytes")
            entry = value + struct.unpack_from("<q", b, 16)[0]
            if funcs.get(name[:-3]) != entry:
                sys.exit(f"{obj}: {name}: entry offset does not point at {name[:-3]}")
            b[16:24] = bytes(8)
        out[name] = (size, hashlib.sha256(bytes(b)).hexdigest())
    return out


def build_kernels(tools, build, arch):
    objs = sorted(glob.glob(os.path.join(build, "*.hip.o")))
    if not objs:
        sys.exit(f"no *.hip.o in {build}")
    union, per_obj = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for obj in objs:
            k = object_kernels(tools, obj, arch, tmp)
            per_obj[os.path.basename(obj)] = k
            for name, h in k.items():
                if union.setdefault(name, h) != h:
                    sys.exit(f"{build}: {name} differs between two objects of one build")
    return union, per_obj


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("build_a")
    ap.add_argument("build_b")
    ap.add_argument("--arch", default="gfx950")
    a = ap.parse_args()
    tools = tool("clang-offload-bundler"), tool("llvm-readelf"), tool("llvm-objcopy")
    ua, pa = build_kernels(tools, a.build_a, a.arch)
    ub, pb = build_kernels(tools, a.build_b, a.arch)
    for o in sorted(set(pa) | set(pb)):
        ka, kb = pa.get(o, {}), pb.get(o, {})
        print(f"{o}: {len(ka)} -> {len(kb)} symbols, "
              f"{sum(1 for n in ka if kb.get(n) == ka[n])} identical, "
              f"{'same set' if set(ka) == set(kb) else 'SET DIFFERS'}")
    only_a, only_b = sorted(set(ua) - set(ub)), sorted(set(ub) - set(ua))
    changed = sorted(n for n in set(ua) & set(ub) if ua[n] != ub[n])
    for n in only_a:
        print(f"only in {a.build_a}: {n}")
    for n in only_b:
        print(f"only in {a.build_b}: {n}")
    for n in changed:
        print(f"differs: {n} ({ua[n][0]} -> {ub[n][0]} bytes)")
    nk = sum(1 for n in ua if n.endswith(".kd"))
    print(f"union: {len(ua)} -> {len(ub)} symbols ({nk} kernel descriptors), "
          f"{len(only_a)} only in A, {len(only_b)} only in B, {len(changed)} with different bytes")
    return 1 if (only_a or only_b or changed) else 0


if __name__ == "__main__":
    sys.exit(main())
