"""GPU: the plain C++ host program tests/cabi/tiered_bags_test.cpp — the pooled lookup of a hot/cold pair through the C-ABI only."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_tiered_bags_from_plain_cpp(dev):
    """two tables (HBM, pinned host) / pooled sums and means checked against host sums in position order / found mask / the hit counters the
    count flags feed / argument errors / destroy"""
    exe = os.path.join(ROOT, "build", "tiered_bags_test")
    assert os.path.exists(exe), "build/tiered_bags_test missing: run __graft_entry__.build()"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "tiered_bags_test ok" in r.stdout
