"""The host layer of the pooled lookups and of the optimizer steps, pinned without a GPU: tests/cabi/host_transcript.cpp walks every entry point of the
two families — the valid calls over the row shapes, launch shapes, dtypes and forms, and every refusal, some two at a time — against the host halves of
csrc/*.hip, linked to the HIP stand-in whose launches do nothing but log (tests/cabi/hip_host_stub.cpp).  What it prints — return code, message, and
the kernels launched with their template arguments, grid and block — must equal tests/golden/host_transcript.txt byte for byte.  The golden file was
written by the same driver linked against the sources as they were before the host layer was consolidated (one launch path for the pooled lookups, one
for the steps); it is a record of that behaviour, not of the current code: a deliberate change of a refusal or a launch edits it by hand, line by line."""
import difflib
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_transcript_matches_golden(tmp_path):
    out = os.path.join(ROOT, "build", "san_address")
    # (the directory of the older sanitizer test: the script rebuilds only what is stale, so the two share the host-only objects)
    b = subprocess.run(["bash", os.path.join(ROOT, "tests", "cabi", "build_sanitized.sh"), "address", out], capture_output=True, text=True)
    assert b.returncode == 0, "build_sanitized.sh failed:\n" + b.stdout[-2000:] + b.stderr[-6000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([os.path.join(out, "host_transcript"), str(tmp_path / "launches.log")], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr, r.stdout[-1000:] + r.stderr[-6000:]
    with open(os.path.join(ROOT, "tests", "golden", "host_transcript.txt")) as f:
        golden = f.read()
    if r.stdout != golden:
        diff = list(difflib.unified_diff(golden.splitlines(), r.stdout.splitlines(), "golden", "driver", lineterm="", n=0))
        raise AssertionError("%d transcript lines differ:\n%s" % (len(diff), "\n".join(diff[:80])))
