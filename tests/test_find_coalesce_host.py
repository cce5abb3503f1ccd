"""CPU: the host bookkeeping of captured finds (csrc/meepo_find_coalesce.h: overlap test, descriptor rebuild, table of recorded nodes) under
AddressSanitizer + UndefinedBehaviorSanitizer, in a stand-alone program of its own (tests/cabi/find_coalesce_host.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_find_coalesce_host_logic_under_asan_ubsan(tmp_path):
    cxx = os.environ.get("ROCM_CLANGXX", "/opt/rocm/lib/llvm/bin/clang++")
    exe = str(tmp_path / "find_coalesce_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "meepoembedding_amd", "csrc"), os.path.join(ROOT, "tests", "cabi", "find_coalesce_host.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "find_coalesce_host ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr[-4000:]
