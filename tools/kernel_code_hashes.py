#!/usr/bin/env python3
"""Compare the machine code of two builds, kernel by kernel.

    tools/kernel_code_hashes.py build SRC_DIR OUT_DIR [tu ...]   compile each translation unit of SRC_DIR (a csrc directory) for the device only,
                                                                write OUT_DIR/<tu>.co, OUT_DIR/<tu>.remarks (the compiler's resource remarks) and
                                                                OUT_DIR/<tu>.hashes: one line "sha1 instructions demangled-name" per kernel, sorted by name
    tools/kernel_code_hashes.py hash FILE.co ...                the .hashes file of code objects built before
    tools/kernel_code_hashes.py diff OUT_A OUT_B                print the kernels whose name or code differs; exit status 1 if any

A kernel's code is its llvm-objdump disassembly with addresses, encodings and comments stripped (branch targets are offsets inside the kernel).
"""
import hashlib
import os
import re
import subprocess
import sys

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt",
         "-Wno-unused-function", "-Wno-pass-failed", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage"]
TUS = ["meepo_table", "meepo_find", "meepo_export", "meepo_apply", "meepo_dedup", "meepo_router", "meepo_group", "meepo_sharded", "meepo_mixed", "meepo_move", "meepo_padded", "meepo_pool_max"]


def hashes(co):
    if open(co, "rb").read(24) == b"__CLANG_OFFLOAD_BUNDLE__":   # what -c leaves with --cuda-device-only: the code object inside a bundle
        elf = co + ".elf"
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={co}", f"--output={elf}"], check=True)
        co = elf
    dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co], check=True, capture_output=True, text=True).stdout
    kernels, name = {}, None
    for line in dis.splitlines():
        m = re.match(r"^(?:[0-9a-f]+ )?<(\S+)>:$", line)
        if m:
            name = m.group(1)
            kernels[name] = []
        elif name and line.strip() and line.strip() != "...":   # "...": the padding up to the next kernel's alignment, which the last kernel of a code object lacks
            kernels[name].append(re.sub(r"\s*//.*$", "", line).strip())
    names = list(kernels)
    demangled = subprocess.run(["c++filt"], input="\n".join(names), check=True, capture_output=True, text=True).stdout.splitlines()
    rows = []
    for n, d in zip(names, demangled):
        rows.append((d, len(kernels[n]), hashlib.sha1("\n".join(kernels[n]).encode()).hexdigest()))
    return sorted(rows)


def write_hashes(co):
    with open(co[:-3] + ".hashes", "w") as f:
        for d, n, h in hashes(co):
            f.write(f"{h} {n} {d}\n")


def build(src, out, tus):
    os.makedirs(out, exist_ok=True)
    jobs = []
    for tu in tus:
        co = os.path.join(out, tu + ".co")
        jobs.append((tu, co, subprocess.Popen([HIPCC, *FLAGS, "-c", os.path.join(src, tu + ".hip"), "-o", co], stderr=open(os.path.join(out, tu + ".remarks"), "w"))))
    for tu, co, p in jobs:
        if p.wait() != 0:
            sys.exit(f"{tu}: the compiler failed, see {out}/{tu}.remarks")
        write_hashes(co)


def diff(a, b):
    bad = 0
    for fn in sorted(set(os.listdir(a)) | set(os.listdir(b))):
        if not fn.endswith(".hashes"):
            continue
        rows = []
        for d in (a, b):
            p = os.path.join(d, fn)
            rows.append({l.split(" ", 2)[2]: l.split(" ", 2)[:2] for l in open(p).read().splitlines()} if os.path.exists(p) else {})
        same = 0
        for k in sorted(set(rows[0]) | set(rows[1])):
            if rows[0].get(k) == rows[1].get(k):
                same += 1
            else:
                bad += 1
                print(f"{fn}: {k}: {rows[0].get(k, 'absent')} -> {rows[1].get(k, 'absent')}")
        print(f"{fn}: {same} kernels identical of {len(set(rows[0]) | set(rows[1]))}")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "build":
        build(sys.argv[2], sys.argv[3], sys.argv[4:] or TUS)
    elif len(sys.argv) >= 3 and sys.argv[1] == "hash":
        for co in sys.argv[2:]:
            write_hashes(co)
    elif len(sys.argv) == 4 and sys.argv[1] == "diff":
        sys.exit(diff(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
