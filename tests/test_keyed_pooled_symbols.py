"""No GPU: the keyed layout of the pooled group lookups (SPEC.md §3 "Keyed output") as the library exports it and as the Python layer offers it —
the five entry points in the header, the loader and the C++ wrappers, keyed_layout, the new keywords with their defaults, the layer's refusals, and
the layer's composition path (a group without find_pooled(layout="keyed"): the table-major lookup and one permute) over CPU fakes."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mee_group_find_pooled_keyed", "mee_group_find_pooled_tiered_keyed", "mee_mixed_group_find_pooled_keyed", "mee_mixed_group_keyed_grads",
         "mee_mixed_group_keyed_layout"]
DIM = 4


def test_the_five_symbols(built):
    from meepoembedding_amd import _lib
    header = open(os.path.join(ROOT, "include", "meepo_embedding.h")).read()
    assert sorted(set(re.findall(r"\bint\s+(mee_\w*keyed\w*)\(", header))) == NAMES
    L = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name), f"{name} is not exported"
        assert name in _lib.PROTOTYPES, f"{name} is not bound"
        decl = re.sub(r"/\*.*?\*/", "", re.search(r"\bint\s+" + name + r"\(([^;]*)\);", header).group(1), flags=re.S)
        assert len(_lib.PROTOTYPES[name][1]) == decl.count(",") + 1, f"{name}: bound with another number of arguments than declared"
    p = _lib.PROTOTYPES
    for name in NAMES[:3]:   # ..., d_out, out_dtype, out_row_stride, ...
        i = 6 if name != "mee_group_find_pooled_tiered_keyed" else 7
        assert p[name][1][i] is C.c_uint32 and p[name][1][i + 1] is C.c_size_t, name
    assert _lib.lib().mee_abi_version() == 2 == _lib.ABI_VERSION
    assert re.search(r"#define\s+MEE_ABI_VERSION\s+2\b", header)


def test_cpp_wrappers_present():
    hpp = open(os.path.join(ROOT, "include", "meepo_embedding.hpp")).read()
    for name in NAMES:
        assert re.search(r"check\(" + name + r"\(", hpp), f"include/meepo_embedding.hpp has no wrapper around {name}"


def test_keyed_layout_hand_computed():
    from meepoembedding_amd import keyed_layout
    assert keyed_layout([8, 64, 128, 100]) == ([0, 8, 72, 200], 300)
    assert keyed_layout([64, 64, 64]) == ([0, 64, 128], 192)   # a uniform group: j * dim
    assert keyed_layout([100]) == ([0], 100)
    assert keyed_layout([]) == ([], 0)


def test_signatures_carry_the_new_keywords():
    from meepoembedding_amd import MixedTableGroup, TableGroup, TieredTableGroup
    from meepoembedding_amd.nn import DynamicEmbeddingBag, _Traits
    for cls in (TableGroup, TieredTableGroup, MixedTableGroup):
        sig = inspect.signature(cls.find_pooled).parameters
        assert sig["layout"].default == "table" and sig["step_index"].default is None, cls.__name__
        assert list(sig)[-2:] == ["layout", "step_index"], cls.__name__   # behind every existing parameter: positional callers are untouched
        assert cls.keyed_bags is True
    sig = inspect.signature(MixedTableGroup.apply_pooled).parameters
    assert sig["layout"].default == "table" and sig["mean_offsets"].default is None and list(sig)[-2:] == ["layout", "mean_offsets"]
    assert inspect.signature(DynamicEmbeddingBag.__init__).parameters["layout"].default == "table"
    assert _Traits._fields[-1] == "native_keyed" and _Traits._field_defaults["native_keyed"] is False


# ---- CPU fakes: groups WITHOUT keyed_bags, so the layer composes ---------------------------------------------------------------------------
class FakeGroup:
    """two members of dim DIM; the pooled row of bag b is a function of b, so a permute shows"""
    dim = DIM

    def __init__(self):
        self.tables, self.applied = [None, None], []

    def find_or_insert(self, keys, offsets, min_count=None):
        return torch.zeros((keys.numel(), DIM)), torch.zeros(keys.numel(), dtype=torch.uint8)

    def find_pooled(self, keys, bag_offsets, mode="sum", out=None, found=None, located=None, weights=None):
        nb = bag_offsets.numel() - 1
        if located is not None:
            located.zero_()
        return (torch.arange(nb * DIM, dtype=torch.float32).view(nb, DIM) + 0.5), torch.zeros(keys.numel(), dtype=torch.uint8)

    def apply_pooled(self, keys, bag_offsets, bag_grads, bag_of_position, optimizer, lr, eps=None, beta1=0.9, beta2=0.999, step=1, located=None):
        self.applied.append((keys.clone(), bag_offsets.clone(), bag_grads.clone(), bag_of_position.clone(), optimizer, lr, eps, beta1, beta2, step))


class FakeMixedGroup:
    weighted_bags = False
    mixed_dims = True
    dims = [DIM, 2 * DIM]

    def __init__(self):
        self.tables, self.applied = [None, None], []

    def views(self, flat, bags_per_table):
        from meepoembedding_amd.table import mixed_layout
        _, offs, _ = mixed_layout(self.dims, bags_per_table)
        return [flat[o:o + bags_per_table * d].view(bags_per_table, d) for o, d in zip(offs, self.dims)]

    def find_pooled(self, keys, bag_offsets, mode="sum", out=None, found=None, located=None, weights=None, out_dtype=torch.float32, insert_missing=False):
        out.copy_(torch.arange(out.numel(), dtype=torch.float32) + 0.25)
        located.zero_()
        return self.views(out, (bag_offsets.numel() - 1) // 2), torch.zeros(keys.numel(), dtype=torch.uint8)

    def apply_pooled(self, keys, bag_offsets, bag_grads, bag_of_position, optimizer, lr, eps=None, beta1=0.9, beta2=0.999, step=1, located=None):
        self.applied.append((keys.clone(), bag_offsets.clone(), bag_grads.clone(), bag_of_position.clone(), optimizer, lr, eps, beta1, beta2, step))


class FakeTable:
    dim = DIM

    def find(self, keys):
        return torch.zeros((keys.numel(), DIM)), torch.zeros(keys.numel(), dtype=torch.uint8)

    find_or_insert = find

    def find_pooled(self, keys, bag_offsets, mode="sum", out=None, found=None, weights=None, located=None):
        return torch.zeros((bag_offsets.numel() - 1, DIM)), torch.zeros(keys.numel(), dtype=torch.uint8)

    def apply_adagrad(self, keys, grads, lr, eps=1e-10, grad_index=None, slots=None):
        pass

    apply_adam = apply_adagrad


B = 3
KEYS = torch.arange(11, dtype=torch.int64)
OFFSETS = torch.tensor([0, 2, 2, 5, 6, 10, 11], dtype=torch.int64)   # 2 members x 3 bags; one empty


def test_layer_refusals(built):
    from meepoembedding_amd.nn import DynamicEmbeddingBag
    with pytest.raises(ValueError, match="layout"):
        DynamicEmbeddingBag(FakeGroup(), layout="sample")
    with pytest.raises(ValueError, match="keyed"):
        DynamicEmbeddingBag(FakeTable(), layout="keyed")   # a single table (a pair looks the same to the layer: no apply_pooled)
    layer = DynamicEmbeddingBag(FakeGroup(), layout="keyed")
    with pytest.raises(ValueError, match="per_sample_weights"):
        layer(KEYS, OFFSETS, per_sample_weights=torch.ones(KEYS.numel()))
    assert DynamicEmbeddingBag(FakeGroup()).layout == "table" and not layer.traits.native_keyed


def _equal_applied(a, b):
    assert len(a) == len(b) == 1
    for x, y in zip(a[0], b[0]):
        assert torch.equal(x, y) if isinstance(x, torch.Tensor) else x == y, (x, y)


@pytest.mark.parametrize("mode", ["sum", "mean"])
def test_composition_over_a_uniform_fake(built, mode):
    """keyed = the default layer's rows permuted; the SAME apply_pooled call receives the inverse-permuted gradient"""
    from meepoembedding_amd.nn import DynamicEmbeddingBag
    ga, gb = FakeGroup(), FakeGroup()
    plain, keyed = DynamicEmbeddingBag(ga, mode=mode, lr=0.5), DynamicEmbeddingBag(gb, mode=mode, lr=0.5, layout="keyed")
    pa, kb = plain(KEYS, OFFSETS), keyed(KEYS, OFFSETS)
    assert pa.shape == (2 * B, DIM) and kb.shape == (B, 2 * DIM)
    assert torch.equal(kb, pa.view(2, B, DIM).transpose(0, 1).reshape(B, 2 * DIM))
    gk = torch.arange(B * 2 * DIM, dtype=torch.float32).view(B, 2 * DIM) * 0.125 - 1.0   # a non-uniform keyed gradient
    kb.backward(gk)
    pa.backward(gk.view(B, 2, DIM).transpose(0, 1).reshape(2 * B, DIM))
    _equal_applied(ga.applied, gb.applied)


def test_composition_over_a_mixed_fake(built):
    from meepoembedding_amd.nn import DynamicEmbeddingBag
    ga, gb = FakeMixedGroup(), FakeMixedGroup()
    plain, keyed = DynamicEmbeddingBag(ga, mode="mean"), DynamicEmbeddingBag(gb, mode="mean", layout="keyed")
    views, kb = plain(KEYS, OFFSETS), keyed(KEYS, OFFSETS)
    assert isinstance(kb, torch.Tensor) and kb.shape == (B, 3 * DIM)
    assert torch.equal(kb, torch.cat(list(views), dim=1))
    gk = torch.arange(B * 3 * DIM, dtype=torch.float32).view(B, 3 * DIM) * 0.25 + 1.0
    kb.backward(gk)
    torch.autograd.backward(list(views), list(torch.split(gk, FakeMixedGroup.dims, dim=1)))
    _equal_applied(ga.applied, gb.applied)
