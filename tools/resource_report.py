#!/usr/bin/env python3
"""Register, occupancy, LDS and scratch figures of the kernels of one csrc/*.hip file, as the compiler reports them
(-Rpass-analysis=kernel-resource-usage; device code only, nothing is linked or run - works on a machine without a GPU):
  tools/resource_report.py elem.hip [name filter regex] [--src DIR]  > profiles/<tag>_resource_elem.txt
Flags as csrc/Makefile's, EXTRA_<file> included.  --src: another checkout's csrc (tools/build_base.sh leaves the parent's under
csrc/build_base/src/gan-reverser_amd/csrc)."""
import os
import re
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    args = sys.argv[1:]
    src = os.path.join(ROOT, "gan-reverser_amd", "csrc")
    if "--src" in args:
        i = args.index("--src")
        src = os.path.abspath(args[i + 1])
        del args[i:i + 2]
    name = args[0] if args else "elem.hip"
    flt = re.compile(args[1] if len(args) > 1 else ".")
    stem = os.path.splitext(name)[0]
    inc = os.path.normpath(os.path.join(src, "..", "..", "include"))
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I" + inc,
           "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(src, name), "-o", os.devnull]
    extra = re.search(r"^EXTRA_" + re.escape(stem) + r"\s*=\s*(.*)$", open(os.path.join(src, "Makefile")).read(), re.M)     # the per-file flags of that checkout
    if extra:
        cmd[5:5] = extra.group(1).split()
    err = subprocess.run(cmd, stderr=subprocess.PIPE, stdout=subprocess.DEVNULL, text=True, check=True).stderr
    rows, cur = [], None
    for line in err.splitlines():
        m = re.search(r"remark: (?:Function Name: (\S+)|\s*([A-Za-z/\[\] ]+?): (\d+))", line)
        if not m:
            continue
        if m.group(1):
            cur = {"name": m.group(1)}
            rows.append(cur)
        elif cur is not None:
            cur[m.group(2).strip()] = int(m.group(3))
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    mangled = [r["name"] for r in rows]
    demangle = subprocess.run([filt], input="\n".join(mangled), stdout=subprocess.PIPE, text=True).stdout.splitlines() if filt else mangled
    print(f"{'VGPRs':>5} {'AGPRs':>5} {'SGPRs':>5} {'waves/SIMD':>10} {'LDS B':>6} {'scratch B':>9} {'VGPR spill':>10}  kernel")
    for r, d in zip(rows, demangle):
        d = re.sub(r"\(.*$", "", d.replace("void ", "").replace("gr::", ""))
        if not flt.search(d):
            continue
        print(f"{r.get('VGPRs', 0):>5} {r.get('AGPRs', 0):>5} {r.get('TotalSGPRs', 0):>5} {r.get('Occupancy [waves/SIMD]', 0):>10} {r.get('LDS Size [bytes/block]', 0):>6} "
              f"{r.get('ScratchSize [bytes/lane]', 0):>9} {r.get('VGPRs Spill', 0):>10}  {d}")


if __name__ == "__main__":
    main()
