"""GPU: the plain C++ host program tests/cabi/mixed_group_test.cpp — a mixed group (members of different dims) through the C-ABI only."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_mixed_group_from_plain_cpp(dev):
    """create / layout / one pooled lookup checked against host sums in position order / argument errors / destroy"""
    exe = os.path.join(ROOT, "build", "mixed_group_test")
    assert os.path.exists(exe), "build/mixed_group_test missing: run __graft_entry__.build()"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "mixed_group_test ok" in r.stdout
