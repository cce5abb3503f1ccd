"""No GPU: the built library exports the padded sequence lookup, the ctypes loader declares it with the header's argument lists, the Python
classes carry the keywords, and DynamicEmbeddingSequence over CPU adapters (tables without find_padded: the composition path) computes and
trains what the oracle does."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from _padded_cases import EMPTY, expected_padded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"mee_find_padded_as": 14, "mee_group_find_padded_as": 14}


def test_library_exports_and_loader_declares_find_padded(built):
    from meepoembedding_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "meepo_embedding.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"MEE_PAD_KEEP_FIRST\s*=\s*0\s*,\s*MEE_PAD_KEEP_LAST\s*=\s*1", header)
    assert (_lib.PAD_KEEP_FIRST, _lib.PAD_KEEP_LAST) == (0, 1)
    for name, n_args in SYMBOLS.items():
        assert hasattr(raw, name), f"{name} is not exported by {_lib.LIB_PATH}"
        fn = getattr(_lib.lib(), name)
        assert fn.restype is C.c_int and len(fn.argtypes) == n_args, name
        proto = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert proto, f"{name}: prototype missing from include/meepo_embedding.h"
        assert len(proto.group(1).split(",")) == n_args, f"{name}: the header's arity differs"
    hpp = open(os.path.join(ROOT, "include", "meepo_embedding.hpp")).read()
    assert "mee_find_padded_as(" in hpp and "mee_group_find_padded_as(" in hpp


def test_python_surface(built):
    from meepoembedding_amd import LookupTable, TableGroup
    from meepoembedding_amd.nn import DynamicEmbeddingSequence
    for cls in (LookupTable, TableGroup):
        p = inspect.signature(cls.find_padded).parameters
        assert list(p)[1:4] == ["keys", "bag_offsets", "max_len"], cls
        assert p["keep"].default == "first" and p["out"].default is None and p["found"].default is None, cls
        assert p["out_dtype"].default is torch.float32 and p["with_step"].default is False, cls
    p = inspect.signature(DynamicEmbeddingSequence.__init__).parameters
    assert list(p)[1:3] == ["table_or_group", "max_len"]
    assert p["keep"].default == "first" and p["optimizer"].default == "adagrad" and p["create_missing"].default is True
    assert p["out_dtype"].default is torch.float32 and {"lr", "eps", "betas"} <= set(p)
    with pytest.raises(ValueError, match="keep"):
        DynamicEmbeddingSequence(object(), 4, keep="middle")
    with pytest.raises(ValueError, match="max_len"):
        DynamicEmbeddingSequence(object(), 0)


DIM, L = 8, 4
STORED = np.arange(100, 140, dtype=np.int64)
# bags of 0, 2 (< L), 4 (= L), 7 (> L) and 1 keys; stored keys, absent ones (900..), one key twice inside a bag and across bags
KEYS = np.array([100, 901,   102, 103, 104, 105,   106, 107, 108, 902, 110, 111, 106,   100], np.int64)
OFFSETS = np.array([0, 0, 2, 6, 13, 14], np.int64)
# the same shape without a duplicate among the kept keys, for the bit-exact step
KEYS_DISTINCT = np.array([100, 901,   102, 103, 104, 105,   106, 107, 108, 902, 110, 111, 112,   113], np.int64)


def _rows(keys, seed):
    from meepoembedding_amd import synth
    return synth.rows_np(np.asarray(keys, np.int64), DIM, seed)


def _pair(optimizer):
    """a CpuTable for the layer and an oracle twin holding the same pairs"""
    import oracle
    from _cpu_backend import CpuTable
    kw = dict(optimizer=optimizer, default_value=0.25, initial_accumulator=0.1)
    t, o = CpuTable(512, DIM, **kw), oracle.OracleTable(512, DIM, **kw)
    rows = _rows(STORED, 3)
    t.insert(torch.from_numpy(STORED), torch.from_numpy(rows))
    o.insert(STORED, rows)
    return t, o


def _table_of(o):
    k, v, a, b = o.export(with_state=True)
    order = np.argsort(k)
    return k[order], v[order], a[order], (b[order] if b is not None else None)


@pytest.mark.parametrize("keep", ["first", "last"])
def test_layer_forward_over_cpu_table(built, keep):
    import oracle
    from meepoembedding_amd.nn import DynamicEmbeddingSequence
    t, o = _pair(oracle.OPT_ADAGRAD)
    layer = DynamicEmbeddingSequence(t, L, keep=keep, create_missing=False)
    assert not layer.traits.native_padded
    for mode in (layer.train, layer.eval):
        mode()
        padded, lengths = layer(torch.from_numpy(KEYS), torch.from_numpy(OFFSETS))
        exp, _, exp_len, _, _ = expected_padded(lambda b: o.find, KEYS, OFFSETS, L, keep, DIM)
        assert padded.shape == (5, L, DIM) and padded.dtype == torch.float32
        assert np.array_equal(padded.detach().numpy().view(np.uint32), exp.view(np.uint32))
        assert np.array_equal(lengths.numpy(), exp_len) and exp_len.tolist() == [0, 2, 4, 4, 1]
    assert t.size() == o.size() == STORED.size   # create_missing=False creates nothing


@pytest.mark.parametrize("optimizer", ["adagrad", "adam"])
@pytest.mark.parametrize("keep", ["first", "last"])
@pytest.mark.parametrize("keys", [KEYS, KEYS_DISTINCT], ids=["duplicates", "distinct"])
def test_layer_step_over_cpu_table(built, optimizer, keep, keys):
    """two steps with non-uniform grads: the table holds exactly what the oracle's apply_* leaves on the kept keys with their slots' grad rows"""
    import oracle
    from meepoembedding_amd.nn import DynamicEmbeddingSequence
    t, o = _pair(oracle.OPT_ADAGRAD if optimizer == "adagrad" else oracle.OPT_ADAM)
    layer = DynamicEmbeddingSequence(t, L, keep=keep, optimizer=optimizer, lr=0.05, create_missing=False)
    layer.train()
    n_bags = OFFSETS.size - 1
    _, _, _, step_keys, grad_index = expected_padded(lambda b: o.find, keys, OFFSETS, L, keep, DIM)
    kept = np.nonzero(step_keys != EMPTY)[0]   # (the bags cover every position, and no key of the batch is EMPTY)
    cut_only = sorted(set(keys[step_keys == EMPTY].tolist()))
    for step in (1, 2):
        w = torch.from_numpy((_rows(np.arange(n_bags * L), 10 + step) * 0.1).reshape(n_bags, L, DIM))
        padded, _ = layer(torch.from_numpy(keys), torch.from_numpy(OFFSETS))
        (padded * w).sum().backward()
        g = w.numpy().reshape(-1, DIM)[grad_index[kept].astype(np.int64)]
        if optimizer == "adagrad":
            o.apply_adagrad(keys[kept], g, 0.05, 1e-10)
        else:
            o.apply_adam(keys[kept], g, 0.05, 0.9, 0.999, 1e-8, step)
    got, exp = _table_of(t.o), _table_of(o)
    for a, b in zip(got, exp):
        assert (a is None) == (b is None)
        if a is not None:
            assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
    # keys that were only ever cut off still hold their inserted rows; absent keys were not created
    kept_keys = set(keys[kept].tolist())
    untouched = np.array([k for k in cut_only if k not in kept_keys and k < 900], np.int64)
    assert untouched.size > 0
    rows, found = t.find(torch.from_numpy(untouched))
    assert found.all() and np.array_equal(rows.numpy(), _rows(untouched, 3))
    assert t.size() == STORED.size and not t.find(torch.tensor([901, 902]))[1].any()


def test_layer_creates_unseen_ids_in_training_only(built):
    import oracle
    from meepoembedding_amd.nn import DynamicEmbeddingSequence
    t, _ = _pair(oracle.OPT_ADAGRAD)
    layer = DynamicEmbeddingSequence(t, L)   # create_missing defaults to True
    layer.eval()
    layer(torch.from_numpy(KEYS), torch.from_numpy(OFFSETS))
    assert t.size() == STORED.size
    layer.train()
    layer(torch.from_numpy(KEYS), torch.from_numpy(OFFSETS))
    assert t.size() == STORED.size + 2 and t.find(torch.tensor([901, 902]))[1].all()


@pytest.mark.parametrize("keep", ["first", "last"])
def test_kept_reserved_keys_read_the_default_row(built, keep):
    """a kept position whose key is EMPTY or RECLAIMED fills its slot with the table's default row (0.25 here, not the padding's zero), as the
    operator does; it takes no step"""
    import oracle
    from _padded_cases import RECLAIMED
    from meepoembedding_amd.nn import DynamicEmbeddingSequence
    t, o = _pair(oracle.OPT_ADAGRAD)
    keys = KEYS.copy()
    keys[[2, 7, 12]] = [EMPTY, RECLAIMED, EMPTY]   # kept under both `keep` values (bag 2), cut or kept in bag 3
    layer = DynamicEmbeddingSequence(t, L, keep=keep, create_missing=False)
    layer.train()
    padded, lengths = layer(torch.from_numpy(keys), torch.from_numpy(OFFSETS))
    exp, _, exp_len, _, _ = expected_padded(lambda b: o.find, keys, OFFSETS, L, keep, DIM)
    assert (exp[2, 0] == 0.25).all()               # the expectation itself: the EMPTY key of bag 2 reads the default row
    assert np.array_equal(padded.detach().numpy().view(np.uint32), exp.view(np.uint32)) and np.array_equal(lengths.numpy(), exp_len)
    before = _table_of(t.o)
    padded.sum().backward()
    assert t.size() == STORED.size and np.array_equal(_table_of(t.o)[0], before[0])
