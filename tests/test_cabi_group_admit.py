"""GPU: the plain C++ host program tests/cabi/group_admit_test.cpp — admission over a table group through the C-ABI and the C++ wrapper only."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_group_admission_from_plain_cpp(dev):
    """create / two admitting calls checked on the host (found, size, rows) / per-member thresholds / decay / argument errors / destroy"""
    exe = os.path.join(ROOT, "build", "group_admit_test")
    assert os.path.exists(exe), "build/group_admit_test missing: run __graft_entry__.build()"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "group_admit_test ok" in r.stdout
