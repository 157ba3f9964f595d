#!/usr/bin/env python3
"""Compare the per-kernel resource metadata of two builds of a kernel library (no GPU needed).

    python tools/kernel_meta_diff.py OLD/_hcb_kernels.so NEW/_hcb_kernels.so

Unbundles the gfx950 code object of each library (clang-offload-bundler), reads its AMDGPU metadata
note (llvm-readelf --notes) and reports, for every kernel of OLD, whether .vgpr_count, .sgpr_count,
.private_segment_fixed_size (scratch) and .group_segment_fixed_size (static LDS) are unchanged in NEW;
then lists the kernels only NEW has, flagging any that uses scratch. Kernels are matched by demangled
name with defaulted trailing template arguments ("..., false>" of the INF flag) stripped, so adding a
defaulted template parameter does not hide a kernel from the comparison. Exit status 1 on any change
or any new kernel with scratch."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
ARCH = os.environ.get("HCB_OFFLOAD_ARCH", "gfx950")
FIELDS = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def kernels(so: str) -> dict:
    with tempfile.TemporaryDirectory() as d:
        # the library's .hip_fatbin section holds one offload bundle per translation unit
        fat = os.path.join(d, "fat.bin")
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", so,
                        os.path.join(d, "unused")], check=True)
        data = open(fat, "rb").read()
        magic = b"__CLANG_OFFLOAD_BUNDLE__"
        starts = [m.start() for m in re.finditer(magic, data)] + [len(data)]
        notes = ""
        for i, (a, b) in enumerate(zip(starts, starts[1:])):
            piece, co = os.path.join(d, f"b{i}.bin"), os.path.join(d, f"b{i}.co")
            open(piece, "wb").write(data[a:b])
            subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={piece}",
                            f"--output={co}", f"--targets=hipv4-amdgcn-amd-amdhsa--{ARCH}"], check=True)
            notes += subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True,
                                    capture_output=True, text=True).stdout
    out, cur, sym = {}, {}, None
    for line in notes.splitlines():
        m = re.match(r"\s*(?:- )?(\.[a-z_]+):\s*(.*)$", line)
        if not m:
            continue
        k, v = m.group(1), m.group(2).strip().strip("'")
        if k == ".symbol":
            sym = v[:-3] if v.endswith(".kd") else v
        elif k in FIELDS:
            cur[k] = int(v)
            if k == ".vgpr_count":  # a kernel's keys are sorted: the last of the four, after .symbol
                out[sym] = cur
                cur = {}
    return out


def demangle(names):
    tool = os.path.join(LLVM, "llvm-cxxfilt")
    r = subprocess.run([tool if os.path.exists(tool) else "c++filt"], input="\n".join(names), capture_output=True, text=True,
                       check=True)
    return r.stdout.splitlines()


def norm(name: str) -> str:
    name = re.sub(r"\bhcb16::", "hcb::", name)
    while True:
        n = re.sub(r", false>", ">", name)
        if n == name:
            return name
        name = n


def main(old_so, new_so):
    old, new = kernels(old_so), kernels(new_so)
    od = dict(zip(map(norm, demangle(list(old))), old.values()))
    nd = dict(zip(demangle(list(new)), new.values()))
    nn = {}
    for k, v in nd.items():
        nn.setdefault(norm(k), []).append((k, v))
    bad = 0
    matched = set()
    for k, v in sorted(od.items()):
        cands = [c for c in nn.get(k, []) if not c[0].endswith(", true>")]
        if not cands:
            print("MISSING in new:", k)
            bad += 1
            continue
        matched.add(cands[0][0])
        if cands[0][1] != v:
            print("CHANGED:", k, v, "->", cands[0][1])
            bad += 1
    added = [(k, v) for k, v in sorted(nd.items()) if k not in matched]
    scratch = [(k, v) for k, v in added if v.get(".private_segment_fixed_size", 0) != 0]
    print(f"{len(od)} kernels in old, {len(nd)} in new; {len(od) - bad} unchanged, {bad} changed / missing, "
          f"{len(added)} added, {len(scratch)} of them with scratch")
    for k, v in scratch:
        print("SCRATCH:", k, v)
    if "-v" in sys.argv:
        for k, v in added:
            print("added:", k, v)
    return 1 if bad or scratch else 0


if __name__ == "__main__":
    a = [x for x in sys.argv[1:] if not x.startswith("-")]
    sys.exit(main(a[0], a[1]))
