#!/usr/bin/env python
"""Per-kernel table of the gfx950 code objects inside a BUILT library (no GPU, no recompilation):

    python tools/kernel_table.py [path/to/libmyosim_hip.so] [OUT.json]

name -> instruction count, VGPRs, AGPRs, SGPRs, spill counts, scratch bytes, and a hash of the disassembly (addresses dropped).
Two builds of a kernel whose rows agree execute the same machine code: tests/test_rows128.py compares the shipped one-row kernels
with profiles/kernel_table_before_rows128.json, the table of the commit before the two-rows-per-lane kernels went in."""
import hashlib
import json
import os
import re
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_stats as S   # noqa: E402

NOTE_KEYS = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")


def device_objects(path):
    """the gfx950 code objects of every offload bundle in the library"""
    d = open(path, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    i = d.find(magic)
    while i >= 0:
        p = i + len(magic)
        (n,) = struct.unpack_from("<Q", d, p); p += 8
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", d, p); p += 24
            triple = d[p:p + tl].decode(); p += tl
            if "gfx950" in triple and size:
                yield d[i + off:i + off + size]
        i = d.find(magic, i + len(magic))


def disassembly(obj):
    """name -> (instruction count, sha256 over mnemonics + operands + encodings)"""
    txt = subprocess.check_output([f"{S.LLVM}/llvm-objdump", "-d", obj], text=True)
    out, name, cur, n = {}, None, None, 0
    for line in txt.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:", line)
        if m:
            if name is not None:
                out[name] = (n, cur.hexdigest())
            name, cur, n = m.group(1), hashlib.sha256(), 0
            continue
        if cur is not None and re.match(r"^\s+[a-z_0-9]+", line):
            cur.update(re.sub(r"^\s*", "", line).split("//")[0].encode())
            n += 1
    if name is not None:
        out[name] = (n, cur.hexdigest())
    return out


def table(lib):
    tab = {}
    with tempfile.TemporaryDirectory() as tmp:
        for k, blob in enumerate(device_objects(lib)):
            f = os.path.join(tmp, f"{k}.co")
            open(f, "wb").write(blob)
            dis = disassembly(f)
            for rec in S.notes(f):
                name = rec.get("name")
                if name not in dis:
                    continue
                row = {key: int(rec[key]) for key in NOTE_KEYS if key in rec}
                row["instructions"], row["sha256"] = dis[name]
                tab[name] = row
    return tab


def main():
    from myosuite_amd import engine as E
    lib = sys.argv[1] if len(sys.argv) > 1 else E.LIB_PATH
    tab = table(lib)
    if len(sys.argv) > 2:
        json.dump(tab, open(sys.argv[2], "w"), indent=1, sort_keys=True)
    for name in sorted(tab):
        r = tab[name]
        print(f"{S.demangle(name):64s} insts {r['instructions']:6d} vgpr {r['vgpr_count']:3d} sgpr {r['sgpr_count']:3d} vspill {r['vgpr_spill_count']:3d} "
              f"sspill {r['sgpr_spill_count']:3d} scratch {r['private_segment_fixed_size']:4d}")


if __name__ == "__main__":
    main()
