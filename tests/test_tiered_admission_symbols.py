"""No GPU: the built library exports the entry points of admission over hot/cold pairs, the ctypes loader declares them with the header's argument
lists, the Python classes carry the keywords, and a pair over objects that are not native tables refuses min_count."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"mee_find_or_insert_admit_missing": 8, "mee_group_find_or_insert_admit_tiered": 13, "mee_group_ensure_admit_tiered": 11}


def test_library_exports_and_loader_declares_tiered_admission(built):
    from meepoembedding_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "meepo_embedding.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)   # (the comments behind the arguments hold commas and semicolons)
    for name, n_args in SYMBOLS.items():
        assert hasattr(raw, name), f"{name} is not exported by {_lib.LIB_PATH}"
        fn = getattr(_lib.lib(), name)
        assert fn.restype is C.c_int and len(fn.argtypes) == n_args, name
        proto = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert proto, f"{name}: prototype missing from include/meepo_embedding.h"
        assert len(proto.group(1).split(",")) == n_args, f"{name}: the header's arity differs"


def test_python_surface(built):
    from meepoembedding_amd import TieredLookupTable, TieredTableGroup
    for cls in (TieredLookupTable, TieredTableGroup):
        assert "min_count" in inspect.signature(cls.find_or_insert).parameters, cls
        assert "min_count" in inspect.signature(cls.find_pooled).parameters, cls
        assert hasattr(cls, "admission_decay"), cls
    assert isinstance(TieredLookupTable.admission, property)


def test_pairs_of_other_objects_refuse_min_count(built):
    """admission counts in the hot table's sketch on the device: a pair of CPU adapters has none.  Nothing is looked up or created by the refused calls,
    and the same pair keeps serving the calls without min_count."""
    import oracle
    from _cpu_backend import CpuTable
    from meepoembedding_amd import TieredLookupTable, TieredTableGroup
    from meepoembedding_amd.nn import DynamicEmbeddingBag, DynamicEmbeddingCollection
    pair = TieredLookupTable(CpuTable(256, 8, optimizer=oracle.OPT_ADAGRAD), CpuTable(256, 8, optimizer=oracle.OPT_ADAGRAD))
    assert pair.admission is False
    keys = torch.arange(1, 9, dtype=torch.int64)
    bags = torch.tensor([0, 4, 8], dtype=torch.int64)
    with pytest.raises(ValueError, match="native"):
        pair.find_or_insert(keys, min_count=2)
    with pytest.raises(ValueError, match="native"):
        pair.find_pooled(keys, bags, insert_missing=True, min_count=2)
    with pytest.raises(ValueError, match="native"):
        pair.admission_decay()
    with pytest.raises(ValueError, match="insert_missing"):
        pair.find_pooled(keys, bags, min_count=2)
    group = TieredTableGroup([pair])
    off = torch.tensor([0, 8], dtype=torch.int64)
    with pytest.raises(ValueError, match="native"):
        group.find_or_insert(keys, off, min_count=2)
    with pytest.raises(ValueError, match="native"):
        group.find_pooled(keys, bags, insert_missing=True, min_count=[2])
    with pytest.raises(ValueError, match="native"):
        group.admission_decay()
    with pytest.raises(ValueError, match="native"):
        DynamicEmbeddingCollection(group, min_count=2)
    with pytest.raises(ValueError, match="native"):
        DynamicEmbeddingBag(pair, create_missing=True, min_count=2)
    assert pair.size() == 0
    _, found = group.find_or_insert(keys, off)
    assert not found.any() and pair.size() == 8


def test_layers_name_the_way_and_keep_sharded_refused(built):
    """DynamicEmbedding over a pair stays refused and now says what to use; a sharded group of pairs is refused as sharded, not as tiered"""
    import oracle
    from _cpu_backend import CpuTable
    from meepoembedding_amd import TieredLookupTable
    from meepoembedding_amd.nn import DynamicEmbedding, DynamicEmbeddingCollection
    from meepoembedding_amd.sharded import ShardedTieredTableGroup
    pair = TieredLookupTable(CpuTable(256, 8, optimizer=oracle.OPT_ADAGRAD), CpuTable(256, 8, optimizer=oracle.OPT_ADAGRAD))
    with pytest.raises(ValueError, match="hot/cold") as ei:
        DynamicEmbedding(pair, min_count=2)
    assert "DynamicEmbeddingCollection" in str(ei.value) and "TieredTableGroup([pair])" in str(ei.value)
    sharded = ShardedTieredTableGroup.__new__(ShardedTieredTableGroup)   # only its type is looked at
    with pytest.raises(ValueError, match="sharded") as ei:
        DynamicEmbeddingCollection(sharded, min_count=2)
    assert "hot/cold pair has no admission" not in str(ei.value)
