#!/usr/bin/env python3
"""Are the gfx950 kernels of two builds of libtooncrafter_hip.so the same code?  Unbundles every code object of both
libraries, compares the sets of kernel symbols and the `llvm-objdump -d` text of every kernel.

    python scripts/isa_compare.py OLD.so NEW.so > profiles/<name>_isa.txt      (exit status 1 on any difference)
"""
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(so, tmp):
    fat = os.path.join(tmp, "fatbin")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", so, fat])
    data = open(fat, "rb").read()
    out = []
    for m in re.finditer(MAGIC, data):
        base = m.start()
        (n,) = struct.unpack_from("<Q", data, base + len(MAGIC))
        pos = base + len(MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", data, pos)
            triple = data[pos + 24:pos + 24 + tlen].decode()
            pos += 24 + tlen
            if "gfx950" in triple and size:
                path = os.path.join(tmp, f"co{len(out)}.o")
                open(path, "wb").write(data[base + off:base + off + size])
                out.append(path)
    return out


def kernels(so):
    """{demangled symbol: [disassembly text]} over every gfx950 code object of the library"""
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        for co in code_objects(so, tmp):
            body = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "-C", co], text=True)
            for blk in re.split(r"\n(?=[0-9a-f]+ <)", body):
                m = re.match(r"[0-9a-f]+ <(.*)>:\n", blk)
                if not m:
                    continue
                # drop the addresses (a kernel may move inside its code object), keep encodings and text
                lines = [re.sub(r"^\s*[0-9a-f]+:\s*", "", re.sub(r"//\s*[0-9A-F]+:", "//", l)) for l in blk.splitlines()[1:]]
                res.setdefault(m.group(1), []).append("\n".join(lines))
    return res


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    only_old, only_new = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    same = [k for k in old if k in new and old[k] == new[k]]
    diff = sorted(k for k in old if k in new and old[k] != new[k])
    print(f"kernel symbols: old {len(old)}, new {len(new)}; only in old {len(only_old)}, only in new {len(only_new)}")
    print(f"disassembly (llvm-objdump -d, encodings included, addresses dropped): {len(same)} identical, {len(diff)} different")
    for tag, names in (("only in old", only_old), ("only in new", only_new), ("different", diff)):
        for k in names:
            print(f"  {tag}: {k}")
    return 1 if (only_old or only_new or diff) else 0


if __name__ == "__main__":
    sys.exit(main())
