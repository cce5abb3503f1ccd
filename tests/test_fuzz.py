"""Short runs of the randomised checks under tools/ (fuzz_dedup_sum.py, fuzz_apply.py) inside the GPU suite: streams that change their skew from batch to batch, every
path of the dedup and apply kernels, against torch references.  The long runs of the round are under profiles/ (r05_fuzz_*.txt)."""
import importlib.util
import os

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("seed", [101, 102])
def test_fuzz_dedup_sum(dev, seed):
    assert _tool("fuzz_dedup_sum").run(3, seed, quiet=True) >= 6


@pytest.mark.parametrize("seed", [201, 202])
def test_fuzz_apply(dev, seed):
    assert _tool("fuzz_apply").run(3, seed, quiet=True) >= 3


@pytest.mark.parametrize("opt,seed", [("adagrad", 203), ("adam", 204)])
def test_fuzz_apply_wide_dims(dev, opt, seed):
    """The same streams at row widths beyond one 16-lane column chunk of the run-time instance (100, 260) and at DIM4 = 32 (128), both optimizers."""
    assert _tool("fuzz_apply").run(3, seed, quiet=True, dims=[100, 128, 260], opt=opt) >= 3
