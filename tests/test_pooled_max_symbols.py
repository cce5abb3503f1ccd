"""No GPU: max pooling (SPEC.md §3 find_pooled_max / pooled_max_backward) as the library exports it and as the Python layer offers it — the four entry
points in the header, the loader and the C++ wrappers, the new methods' signatures, the reference scan against torch.nn.functional.embedding_bag on
the CPU bit for bit, and the layer's wiring over a CPU fake."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from _pooled_max_ref import NO_ARGMAX, bits, pooled_max, pooled_max_backward

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mee_find_pooled_max", "mee_group_find_pooled_max", "mee_group_pooled_max_backward", "mee_pooled_max_backward"]
DIM = 8


def test_the_four_symbols(built):
    from meepoembedding_amd import _lib
    header = open(os.path.join(ROOT, "include", "meepo_embedding.h")).read()
    assert sorted(set(re.findall(r"\bint\s+(mee_\w*pooled_max\w*)\(", header))) == NAMES
    L = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name), f"{name} is not exported"
        assert name in _lib.PROTOTYPES, f"{name} is not bound"
        decl = re.sub(r"/\*.*?\*/", "", re.search(r"\bint\s+" + name + r"\(([^;]*)\);", header).group(1), flags=re.S)
        assert len(_lib.PROTOTYPES[name][1]) == decl.count(",") + 1, f"{name}: bound with another number of arguments than declared"
    assert len(_lib.PROTOTYPES["mee_find_pooled_max"][1]) == len(_lib.PROTOTYPES["mee_group_find_pooled_max"][1]) == 10
    assert len(_lib.PROTOTYPES["mee_pooled_max_backward"][1]) == len(_lib.PROTOTYPES["mee_group_pooled_max_backward"][1]) == 8
    assert _lib.lib().mee_abi_version() == 2 == _lib.ABI_VERSION
    assert re.search(r"#define\s+MEE_ABI_VERSION\s+2\b", header)


def test_cpp_wrappers_present():
    hpp = open(os.path.join(ROOT, "include", "meepo_embedding.hpp")).read()
    for name in NAMES:
        assert re.search(r"check\(" + name + r"\(", hpp), f"include/meepo_embedding.hpp has no wrapper around {name}"


def test_signatures():
    from meepoembedding_amd import LookupTable, TableGroup
    for cls in (LookupTable, TableGroup):
        sig = inspect.signature(cls.find_pooled_max).parameters
        assert list(sig) == ["self", "keys", "bag_offsets", "out", "found", "argmax", "out_dtype", "with_argmax"], cls.__name__
        assert sig["out"].default is None and sig["found"].default is None and sig["argmax"].default is None
        assert sig["out_dtype"].default == torch.float32 and sig["with_argmax"].default is False
        sig = inspect.signature(cls.pooled_max_backward).parameters
        assert list(sig) == ["self", "bag_offsets", "argmax", "bag_grads", "n", "grads"] and sig["grads"].default is None, cls.__name__
    # find_pooled's own signatures are what they were
    assert list(inspect.signature(LookupTable.find_pooled).parameters) == ["self", "keys", "bag_offsets", "mode", "out", "found", "weights", "located", "out_dtype"]
    assert list(inspect.signature(TableGroup.find_pooled).parameters) == ["self", "keys", "bag_offsets", "mode", "out", "found", "located", "weights", "out_dtype",
                                                                          "layout", "step_index"]


def test_find_pooled_forwards_mode_max_and_refuses_the_other_forms(built, monkeypatch):
    from meepoembedding_amd import LookupTable, TableGroup
    from meepoembedding_amd import table as tm
    calls = []

    class Recorder:   # stands in for the library: records what would have been launched
        def __getattr__(self, name):
            calls.append(name)
            return lambda *a: 0

    monkeypatch.setattr(tm._lib, "lib", lambda: Recorder())
    monkeypatch.setattr(tm, "_stream_ptr", lambda device: 0)
    t = LookupTable.__new__(LookupTable)
    t._h, t.device, t.dim = None, torch.device("cpu"), 8
    g = TableGroup.__new__(TableGroup)
    g._h, g.tables, g.device, g.dim = None, [t, t], torch.device("cpu"), 8
    keys = torch.arange(6, dtype=torch.int64)
    off, goff = torch.tensor([0, 2, 6]), torch.tensor([0, 1, 3, 4, 6])
    for bad in (dict(weights=torch.ones(6)), dict(located=torch.empty(6, dtype=torch.int64))):
        with pytest.raises(ValueError, match="max"):
            t.find_pooled(keys, off, "max", **bad)
        with pytest.raises(ValueError, match="max"):
            g.find_pooled(keys, goff, "max", **bad)
    for bad in (dict(layout="keyed"), dict(step_index=torch.empty(6, dtype=torch.int32))):
        with pytest.raises(ValueError, match="max"):
            g.find_pooled(keys, goff, "max", **bad)
    assert calls == []
    out, found = t.find_pooled(keys, off, "max")
    assert out.shape == (2, 8) and out.dtype == torch.float32 and found.shape == (6,)
    out, found = g.find_pooled(keys, goff, "max", out_dtype=torch.bfloat16)
    assert out.shape == (4, 8) and out.dtype == torch.bfloat16
    out, found, am = t.find_pooled_max(keys, off, with_argmax=True)
    assert am.shape == (2, 8) and am.dtype == torch.uint32
    t.pooled_max_backward(off, am, torch.zeros(2, 8), 6)
    g.pooled_max_backward(goff, torch.zeros((4, 8), dtype=torch.int32), torch.zeros(4, 8), 6)
    assert calls == ["mee_find_pooled_max", "mee_group_find_pooled_max", "mee_find_pooled_max", "mee_pooled_max_backward", "mee_group_pooled_max_backward"]


# ---- the reference scan is torch's embedding_bag(mode="max") on the CPU ------------------------------------------------------------------------------
def crafted():
    """a weight matrix [12, DIM], ids and offsets in which every special case of the scan occurs: -> (W, ids, off, the cases found)"""
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    rng = np.random.default_rng(5)
    W = rng.standard_normal((12, DIM)).astype(np.float32)
    W[3, :3] = -2.0                              # (the first bag is ids 1, 2, 3 in that order)
    W[1, 0] = W[2, 0] = 3.5                      # a tie across positions: the first wins
    W[1, 1], W[2, 1] = -0.0, 0.0                 # -0 then +0: the -0 stays
    W[1, 2], W[2, 2] = 0.0, -0.0                 # +0 then -0: the +0 stays
    W[4, 3] = nan                                # NaN first (id 4 opens its bag)
    W[6, 4] = nan                                # NaN later (id 6 is not first in its bag)
    W[5, 5], W[6, 5] = inf, -inf
    W[7, 6], W[8, 6] = -inf, -inf                # all -inf: the first
    ids = np.array([1, 2, 3,   4, 5, 6,   7, 8,   9, 10, 9, 11,   0], np.int64)   # the fourth bag holds id 9 twice; the fifth bag is empty
    off = np.array([0, 3, 6, 8, 12, 12, 13], np.int64)
    return W, ids, off


def test_reference_is_torch_embedding_bag_max_bit_for_bit():
    W, ids, off = crafted()
    out, arg = pooled_max(W[ids], off)
    # the inputs hold every case
    assert arg[0, 0] == 0 and out[0, 0] == 3.5                                            # the tie went to the first position
    assert bits(out)[0, 1] == 0x80000000 and arg[0, 1] == 0                               # -0 then +0
    assert bits(out)[0, 2] == 0 and arg[0, 2] == 0                                        # +0 then -0
    assert np.isnan(out[1, 3]) and arg[1, 3] == 3                                         # NaN first stays
    assert not np.isnan(out[1, 4]) and arg[1, 4] in (3, 4) and np.isnan(W[ids[5], 4])     # NaN later is never taken
    assert out[1, 5] == np.inf and arg[1, 5] == 4
    assert out[2, 6] == -np.inf and arg[2, 6] == 6
    assert (out[4] == 0).all() and (bits(out)[4] == 0).all() and (arg[4] == NO_ARGMAX).all()   # the empty bag
    assert set(arg[3].tolist()) <= {8, 9, 11} and 10 not in arg[3].tolist()               # a duplicate id: its first position wins over its second
    Wt = torch.from_numpy(W.copy()).requires_grad_(True)
    tout, _, _, tidx = torch._embedding_bag(Wt, torch.from_numpy(ids), torch.from_numpy(off), False, 2, False, None, True)
    assert np.array_equal(bits(tout.detach().numpy()), bits(out)), "the scan is not torch's max"
    fout = torch.nn.functional.embedding_bag(torch.from_numpy(ids), Wt, torch.from_numpy(off), mode="max", include_last_offset=True)
    assert np.array_equal(bits(fout.detach().numpy()), bits(out))
    live = arg != NO_ARGMAX
    assert np.array_equal(ids[arg[live].astype(np.int64)], tidx.numpy()[live]), "torch's max_indices name the weight rows of our batch positions"
    # backward: exactly summable gradients (small integers), so the order of torch's scatter does not matter
    G = np.random.default_rng(6).integers(-8, 9, size=out.shape).astype(np.float32)
    fout.backward(torch.from_numpy(G))
    grads = pooled_max_backward(off, arg, G, np.full((ids.size, DIM), 777.0, np.float32))
    assert (grads != 777.0).all()                                                        # the bags cover every position
    dense = np.zeros_like(W)
    np.add.at(dense, ids, grads)
    assert np.array_equal(bits(dense), bits(Wt.grad.numpy())), "the scattered grads are not torch's weight gradient"


def test_reference_backward_copies_bits_and_leaves_uncovered_positions():
    off = np.array([1, 3, 3, 4], np.int64)          # position 0 and positions 4.. are in no bag
    arg = np.array([[1, 2], [NO_ARGMAX, NO_ARGMAX], [3, 3]], np.uint32)
    G = np.array([[-0.0, 2.0], [9.0, 9.0], [np.nan, -0.0]], np.float32)
    grads = pooled_max_backward(off, arg, G, np.full((6, 2), 777.0, np.float32))
    assert (grads[[0, 4, 5]] == 777.0).all()
    assert bits(grads)[1].tolist() == [0x80000000, 0] and bits(grads)[2].tolist() == [0, bits(np.float32(2.0))]
    assert np.isnan(grads[3, 0]) and bits(grads)[3, 1] == 0x80000000


# ---- the layer over a CPU fake ---------------------------------------------------------------------------------------------------------------------
class FakeMaxTable:
    """a dense weight matrix behind LookupTable's max-pooling methods; the step records what it is handed"""
    dim = DIM

    def __init__(self, W):
        self.W, self.applied, self.created = torch.from_numpy(W.copy()), [], []

    def find(self, keys):
        return self.W[keys], torch.ones(keys.numel(), dtype=torch.uint8)

    def find_or_insert(self, keys, min_count=None):
        self.created.append(keys.clone())
        return self.find(keys)

    def find_pooled(self, keys, bag_offsets, mode="sum", out=None, found=None, weights=None, located=None):
        raise AssertionError("mode='max' must not come through find_pooled")

    def find_pooled_max(self, keys, bag_offsets, out=None, found=None, argmax=None, out_dtype=torch.float32, with_argmax=False):
        o, a = pooled_max(self.W[keys].numpy(), bag_offsets.numpy())
        argmax.copy_(torch.from_numpy(a.view(np.int32)))
        return torch.from_numpy(o), torch.ones(keys.numel(), dtype=torch.uint8), argmax

    def pooled_max_backward(self, bag_offsets, argmax, bag_grads, n, grads=None):
        g = pooled_max_backward(bag_offsets.numpy(), argmax.numpy().view(np.uint32), bag_grads.numpy(), np.zeros((n, DIM), np.float32))
        return torch.from_numpy(g)

    def apply_adagrad(self, keys, grads, lr, eps=1e-10, grad_index=None, slots=None):
        assert grad_index is None and slots is None
        self.applied.append((keys.clone(), grads.clone(), lr, eps))

    apply_adam = apply_adagrad


class FakeSumOnlyTable:
    dim = DIM

    def find(self, keys):
        return torch.zeros((keys.numel(), DIM)), torch.zeros(keys.numel(), dtype=torch.uint8)

    find_or_insert = find

    def find_pooled(self, keys, bag_offsets, mode="sum", out=None, found=None, weights=None, located=None):
        return torch.zeros((bag_offsets.numel() - 1, DIM)), torch.zeros(keys.numel(), dtype=torch.uint8)

    def apply_adagrad(self, keys, grads, lr, eps=1e-10, grad_index=None, slots=None):
        pass

    apply_adam = apply_adagrad


class FakeMaxGroup(FakeMaxTable):
    """the same with a group's step: apply_pooled marks it as a group, the max step is apply_adagrad(keys, member offsets, grads)"""

    def __init__(self, W):
        super().__init__(W)
        self.tables = [None, None]

    def find_or_insert(self, keys, offsets, min_count=None):
        self.created.append((keys.clone(), offsets.clone()))
        return self.find(keys)

    def apply_pooled(self, *a, **kw):
        raise AssertionError("the max step takes per-position grads, not bag grads")

    def apply_adagrad(self, keys, offsets, grads, lr, eps=1e-10):
        self.applied.append((keys.clone(), offsets.clone(), grads.clone(), lr, eps))


def test_layer_wiring_over_a_cpu_fake(built):
    from meepoembedding_amd.nn import DynamicEmbeddingBag, lookup_pooled_max
    W, ids, off = crafted()
    keys, offsets = torch.from_numpy(ids), torch.from_numpy(off)
    t = FakeMaxTable(W)
    layer = DynamicEmbeddingBag(t, mode="max", lr=0.25, create_missing=True)
    out = layer(keys, offsets)
    ref, arg = pooled_max(W[ids], off)
    assert np.array_equal(bits(out.detach().numpy()), bits(ref))
    assert len(t.created) == 1 and torch.equal(t.created[0], keys)          # the creation pass in front, as for sum
    G = np.random.default_rng(7).standard_normal(ref.shape).astype(np.float32)
    out.backward(torch.from_numpy(G))
    (k, g, lr, eps), = t.applied
    assert torch.equal(k, keys) and lr == 0.25
    want = pooled_max_backward(off, arg, G, np.zeros((ids.size, DIM), np.float32))
    assert np.array_equal(bits(g.numpy()), bits(want)), "the grads handed to the step"
    layer.eval()
    layer(keys, offsets)
    assert len(t.created) == 1                                              # eval mode creates nothing
    # a group: the step is the grouped one over the members' key segments
    gt = FakeMaxGroup(W)
    goff = torch.tensor([0, 3, 6, 8, 12, 12, 13])                           # 2 members x 3 bags
    glayer = DynamicEmbeddingBag(gt, mode="max", lr=0.5)
    gout = glayer(keys, goff)
    gout.backward(torch.from_numpy(G))
    (k, mo, g, lr, eps), = gt.applied
    assert torch.equal(mo, torch.tensor([0, 8, 13])) and lr == 0.5 and np.array_equal(bits(g.numpy()), bits(want))
    # refusals
    with pytest.raises(ValueError, match="per_sample_weights"):
        layer(keys, offsets, per_sample_weights=torch.ones(ids.size))
    with pytest.raises(ValueError, match="keyed"):
        DynamicEmbeddingBag(gt, mode="max", layout="keyed")
    with pytest.raises(ValueError, match="FakeSumOnlyTable"):
        DynamicEmbeddingBag(FakeSumOnlyTable(), mode="max")
    with pytest.raises(ValueError, match="mode must be 'sum' or 'mean'"):
        DynamicEmbeddingBag(t, mode="min")
    assert DynamicEmbeddingBag(FakeSumOnlyTable(), mode="sum").mode == "sum"
    # the op traces
    from torch.fx.experimental.proxy_tensor import make_fx
    gm = make_fx(lambda k, o, a: lookup_pooled_max(k, o, a, layer.table_id)[0] * 2, tracing_mode="fake")(keys, offsets, layer._anchor)
    assert "torch.ops.meepo.lookup_pooled_max" in gm.code


def test_ops_pass_opcheck(built):
    from meepoembedding_amd.nn import DynamicEmbeddingBag, apply_grad_pooled_max, lookup_pooled_max
    W, ids, off = crafted()
    keys, offsets = torch.from_numpy(ids), torch.from_numpy(off)
    layer = DynamicEmbeddingBag(FakeMaxTable(W), mode="max")
    torch.library.opcheck(lookup_pooled_max, (keys, offsets, layer._anchor, layer.table_id), test_utils=("test_schema", "test_faketensor", "test_autograd_registration"))
    arg = torch.zeros((off.size - 1, DIM), dtype=torch.int32)
    torch.library.opcheck(apply_grad_pooled_max, (keys, offsets, arg, torch.zeros(off.size - 1, DIM), layer.table_id),
                          test_utils=("test_schema", "test_faketensor", "test_autograd_registration"))
