"""No GPU: the built library exports the padded sequence lookup of a hot/cold pair and of a group of pairs, the ctypes loader declares both with
the header's argument lists, TieredLookupTable / TieredTableGroup carry find_padded, and over CPU adapters (tiers that are not native tables: the
composition inside the method) the methods and DynamicEmbeddingSequence compute and train what the oracle of the union does."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from _padded_cases import EMPTY, RECLAIMED, expected_padded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"mee_find_padded_tiered": 16, "mee_group_find_padded_tiered": 16}


def test_library_exports_and_loader_declares_the_tiered_forms(built):
    from meepoembedding_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "meepo_embedding.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    hpp = open(os.path.join(ROOT, "include", "meepo_embedding.hpp")).read()
    for name, n_args in SYMBOLS.items():
        assert hasattr(raw, name), f"{name} is not exported by {_lib.LIB_PATH}"
        fn = getattr(_lib.lib(), name)
        assert fn.restype is C.c_int and len(fn.argtypes) == n_args, name
        proto = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert proto, f"{name}: prototype missing from include/meepo_embedding.h"
        args = [a.strip() for a in proto.group(1).split(",")]
        assert len(args) == n_args, f"{name}: the header's arity differs"
        assert args[7] == "uint32_t flags" and args[8] == "uint32_t count_flags", f"{name}: two separate flag words, PAD_KEEP_* then TIER_COUNT_*"
        assert name + "(" in hpp, f"{name}: no wrapper in include/meepo_embedding.hpp"


def test_python_surface(built):
    from meepoembedding_amd import LookupTable
    from meepoembedding_amd.sharded import ShardedTieredTableGroup
    from meepoembedding_amd.tiered import TieredLookupTable, TieredTableGroup
    want = list(inspect.signature(LookupTable.find_padded).parameters)
    for cls in (TieredLookupTable, TieredTableGroup):
        p = inspect.signature(cls.find_padded).parameters
        assert list(p) == want == ["self", "keys", "bag_offsets", "max_len", "keep", "out", "found", "out_dtype", "with_step"], cls
        assert p["keep"].default == "first" and p["out"].default is None and p["found"].default is None, cls
        assert p["out_dtype"].default is torch.float32 and p["with_step"].default is False, cls
    assert not hasattr(ShardedTieredTableGroup, "find_padded")   # the sharded forms stay on the layer's composition


def test_padded_places_lives_in_one_place(built):
    from meepoembedding_amd import nn, table
    assert nn._padded_places is table._padded_places


DIM, L = 8, 3
HOT_DEFAULT, COLD_DEFAULT = 0.5, 0.25
STORED = np.arange(100, 160, dtype=np.int64)
ABSENT = np.array([901, 902, 903], np.int64)
# bags of 0, 1, 2 (< L), 3 (= L), 4 (= L + 1) and 9 keys, then one position in no bag; a key twice inside a bag (106) and across bags (100),
# absent keys, EMPTY and the tombstone value among the kept and among the cut-off positions
LENS = [0, 1, 2, 3, 4, 9]
KEYS = np.array([100,   101, 901,   102, EMPTY, 104,   105, 106, 106, RECLAIMED,   107, 108, 902, 110, 111, EMPTY, 112, 100, 113,   114], np.int64)
OFFSETS = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
# ... without a duplicate or a reserved key among the kept keys, for the bit-exact step
KEYS_DISTINCT = np.array([100,   101, 901,   102, 103, 104,   105, 106, 115, 116,   107, 108, 902, 110, 111, 117, 112, 118, 113,   114], np.int64)


def _rows(keys, seed):
    from meepoembedding_amd import synth
    return synth.rows_np(np.asarray(keys, np.int64), DIM, seed)


def _cpu_pair(optimizer, hot_keys, seed=3, hot_default=HOT_DEFAULT, plain=False):
    """a pair of CPU adapters — `hot_keys` of STORED in the hot tier, the rest in the cold one — and an oracle of the union with the HOT default.
    plain: adapters whose apply_* take no grad_index (the pair gathers the grad rows for them)"""
    import oracle
    from meepoembedding_amd.tiered import TieredLookupTable
    from test_tiered_bags import _CpuTable
    if plain:
        from _cpu_backend import CpuTable as _CpuTable  # noqa: N811
    kw = dict(optimizer=optimizer, initial_accumulator=0.1)
    hot, cold = _CpuTable(512, DIM, default_value=hot_default, **kw), _CpuTable(512, DIM, default_value=COLD_DEFAULT, **kw)
    union = oracle.OracleTable(1024, DIM, default_value=hot_default, **kw)
    in_hot = np.isin(STORED, hot_keys)
    for t, k in ((hot, STORED[in_hot]), (cold, STORED[~in_hot])):
        if k.size:
            t.insert(torch.from_numpy(k), torch.from_numpy(_rows(k, seed)))
    union.insert(STORED, _rows(STORED, seed))
    return TieredLookupTable(hot, cold), union


PLACEMENTS = {"all_hot": STORED, "all_cold": STORED[:0], "split": STORED[::2]}


def _check(got, exp, what):
    out, found, lengths, step_keys, grad_index = got
    eo, ef, el, ek, eg = exp
    assert out.shape == eo.shape and np.array_equal(out.numpy().view(np.uint32), eo.view(np.uint32)), f"{what}: out"
    assert np.array_equal(found.numpy(), ef), f"{what}: found"
    assert np.array_equal(lengths.numpy(), el), f"{what}: lengths"
    assert np.array_equal(step_keys.numpy(), ek), f"{what}: step_keys"
    assert np.array_equal(grad_index.numpy().astype(np.uint32), eg), f"{what}: grad_index"


def _expected(find_of_bag, keys, offsets, keep):
    """expected_padded with the sentinels of the positions in no bag replaced by what the Python methods pre-set there: not found, EMPTY, index 0"""
    eo, ef, el, ek, eg = expected_padded(find_of_bag, keys, offsets, L, keep, DIM)
    n = len(keys)
    covered = np.zeros(n, bool)
    for b in range(len(offsets) - 1):
        covered[min(offsets[b], offsets[b + 1], n):min(offsets[b + 1], n)] = True
    ef[~covered], ek[~covered], eg[~covered] = 0, EMPTY, 0
    return eo, ef, el, ek, eg


@pytest.mark.parametrize("keep", ["first", "last"])
@pytest.mark.parametrize("placement", list(PLACEMENTS))
def test_pair_of_cpu_tables(built, placement, keep):
    import oracle
    pair, union = _cpu_pair(oracle.OPT_ADAGRAD, PLACEMENTS[placement])
    got = pair.find_padded(torch.from_numpy(KEYS), torch.from_numpy(OFFSETS), L, keep=keep, with_step=True)
    exp = _expected(lambda b: union.find, KEYS, OFFSETS, keep)
    _check(got, exp, f"{placement} {keep}")
    assert (exp[0][2, 1] == HOT_DEFAULT).all() and exp[2].tolist() == [0, 1, 2, 3, 3, 3]   # the expectation itself: an absent key reads the HOT default
    short = pair.find_padded(torch.from_numpy(KEYS), torch.from_numpy(OFFSETS), L, keep=keep)
    assert len(short) == 3 and torch.equal(short[0], got[0]) and torch.equal(short[1], got[1]) and torch.equal(short[2], got[2])
    bf = pair.find_padded(torch.from_numpy(KEYS), torch.from_numpy(OFFSETS), L, keep=keep, out_dtype=torch.bfloat16)[0]
    assert bf.dtype == torch.bfloat16 and torch.equal(bf, got[0].to(torch.bfloat16))
    with pytest.raises(ValueError):
        pair.find_padded(torch.from_numpy(KEYS), torch.from_numpy(OFFSETS), L, keep="middle")
    with pytest.raises(ValueError):
        pair.find_padded(torch.from_numpy(KEYS), torch.from_numpy(OFFSETS), 0)
    # a caller's buffers are refused as the native path refuses them, not converted
    from meepoembedding_amd import MeepoError
    n_bags = OFFSETS.size - 1
    with pytest.raises(ValueError):
        pair.find_padded(torch.from_numpy(KEYS), torch.from_numpy(OFFSETS), L, out=torch.zeros(n_bags, L, DIM, dtype=torch.bfloat16))
    with pytest.raises(MeepoError):
        pair.find_padded(torch.from_numpy(KEYS), torch.from_numpy(OFFSETS), L, out=torch.zeros(n_bags, L + 1, DIM))
    with pytest.raises(MeepoError):
        pair.find_padded(torch.from_numpy(KEYS), torch.from_numpy(OFFSETS), L, found=torch.zeros(KEYS.size, dtype=torch.int32))
    with pytest.raises(MeepoError):
        pair.find_padded(torch.from_numpy(KEYS), torch.from_numpy(OFFSETS), L, found=torch.zeros(KEYS.size - 1, dtype=torch.uint8))
    mine_out, mine_found = torch.full((n_bags, L, DIM), float("nan")), torch.full((KEYS.size,), 0xA5, dtype=torch.uint8)
    res = pair.find_padded(torch.from_numpy(KEYS), torch.from_numpy(OFFSETS), L, keep=keep, out=mine_out, found=mine_found)
    assert res[0].data_ptr() == mine_out.data_ptr() and torch.equal(mine_out, got[0]) and res[1].data_ptr() == mine_found.data_ptr()
    assert mine_found[-1] == 0xA5 and torch.equal(mine_found[:-1], got[1][:-1])   # the position in no bag keeps the caller's byte


def _cpu_group(optimizer):
    """three pairs with their own rows and hot defaults — member 0 all hot, member 1 all cold, member 2 split — and the oracles of their unions"""
    from meepoembedding_amd.tiered import TieredTableGroup
    made = [_cpu_pair(optimizer, PLACEMENTS[p], seed=3 + j, hot_default=0.5 + 0.125 * j) for j, p in enumerate(("all_hot", "all_cold", "split"))]
    return TieredTableGroup([m[0] for m in made]), [m[1] for m in made]


def _group_batch(keys):
    """two bags per member out of the six bags of the batch above (bags_per_table = 2); the trailing position lies in no bag"""
    return keys, OFFSETS, 2


@pytest.mark.parametrize("keep", ["first", "last"])
def test_group_of_cpu_pairs(built, keep):
    import oracle
    grp, unions = _cpu_group(oracle.OPT_ADAGRAD)
    keys, off, bpt = _group_batch(KEYS)
    got = grp.find_padded(torch.from_numpy(keys), torch.from_numpy(off), L, keep=keep, with_step=True)
    _check(got, _expected(lambda b: unions[b // bpt].find, keys, off, keep), f"group {keep}")
    for j, pair in enumerate(grp.tables):   # by definition: the pair's own find_padded on its bags
        s = int(off[j * bpt])
        own = pair.find_padded(torch.from_numpy(keys[s:int(off[(j + 1) * bpt])]), torch.from_numpy(off[j * bpt:(j + 1) * bpt + 1] - s), L, keep=keep)
        assert torch.equal(own[0], got[0][j * bpt:(j + 1) * bpt]) and torch.equal(own[2], got[2][j * bpt:(j + 1) * bpt])


def _table_of(o):
    k, v, a, b = o.export(with_state=True)
    order = np.argsort(k)
    return [x[order] for x in (k, v, a, b) if x is not None]


def _pair_table(pair):
    e = [x.numpy() for x in pair.export(with_state=True) if x is not None]
    order = np.argsort(e[0])
    return [x[order] for x in e]


def _oracle_step(o, optimizer, keys, g, step):
    if optimizer == "adagrad":
        o.apply_adagrad(keys, g, 0.05, 1e-10)
    else:
        o.apply_adam(keys, g, 0.05, 0.9, 0.999, 1e-8, step)


@pytest.mark.parametrize("plain", [False, True], ids=["takes_grad_index", "plain_adapters"])
@pytest.mark.parametrize("optimizer", ["adagrad", "adam"])
@pytest.mark.parametrize("keep", ["first", "last"])
def test_layer_over_a_cpu_pair(built, optimizer, keep, plain):
    """the layer takes the method (native_padded) and trains the pair as the oracle's apply_* trains the union: kept keys with their slots' grad
    rows, cut-off keys untouched, absent keys not created — over adapters that take grad_index and over ones that do not"""
    import oracle
    from meepoembedding_amd.nn import DynamicEmbeddingSequence
    from meepoembedding_amd.tiered import _takes_grad_index
    pair, union = _cpu_pair(oracle.OPT_ADAGRAD if optimizer == "adagrad" else oracle.OPT_ADAM, PLACEMENTS["split"], plain=plain)
    assert _takes_grad_index(pair.hot) == (not plain)
    layer = DynamicEmbeddingSequence(pair, L, keep=keep, optimizer=optimizer, lr=0.05, create_missing=False)
    layer.train()
    assert layer.traits.native_padded and not layer.traits.grouped
    keys, n_bags = KEYS_DISTINCT, OFFSETS.size - 1
    for step in (1, 2):
        exp = _expected(lambda b: union.find, keys, OFFSETS, keep)
        w = torch.from_numpy((_rows(np.arange(n_bags * L), 10 + step) * 0.1).reshape(n_bags, L, DIM))
        padded, lengths = layer(torch.from_numpy(keys), torch.from_numpy(OFFSETS))
        assert np.array_equal(padded.detach().numpy().view(np.uint32), exp[0].view(np.uint32)) and np.array_equal(lengths.numpy(), exp[2])
        (padded * w).sum().backward()
        kept = np.nonzero(exp[3] != EMPTY)[0]
        _oracle_step(union, optimizer, keys[kept], w.numpy().reshape(-1, DIM)[exp[4][kept].astype(np.int64)], step)
    for a, b in zip(_pair_table(pair), _table_of(union)):
        assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
    assert pair.size() == STORED.size


@pytest.mark.parametrize("optimizer", ["adagrad", "adam"])
def test_layer_over_a_group_of_cpu_pairs(built, optimizer):
    import oracle
    from meepoembedding_amd.nn import DynamicEmbeddingSequence
    grp, unions = _cpu_group(oracle.OPT_ADAGRAD if optimizer == "adagrad" else oracle.OPT_ADAM)
    keys, off, bpt = _group_batch(KEYS_DISTINCT)
    layer = DynamicEmbeddingSequence(grp, L, keep="last", optimizer=optimizer, lr=0.05, create_missing=False)
    layer.train()
    assert layer.traits.native_padded and layer.traits.grouped
    n_bags = off.size - 1
    for step in (1, 2):
        exp = _expected(lambda b: unions[b // bpt].find, keys, off, "last")
        w = torch.from_numpy((_rows(np.arange(n_bags * L), 20 + step) * 0.1).reshape(n_bags, L, DIM))
        padded, lengths = layer(torch.from_numpy(keys), torch.from_numpy(off))
        assert np.array_equal(padded.detach().numpy().view(np.uint32), exp[0].view(np.uint32)) and np.array_equal(lengths.numpy(), exp[2])
        (padded * w).sum().backward()
        for j, o in enumerate(unions):
            pos = np.arange(off[j * bpt], off[(j + 1) * bpt])
            pos = pos[exp[3][pos] != EMPTY]
            _oracle_step(o, optimizer, keys[pos], w.numpy().reshape(-1, DIM)[exp[4][pos].astype(np.int64)], step)
    for j, (pair, o) in enumerate(zip(grp.tables, unions)):
        for a, b in zip(_pair_table(pair), _table_of(o)):
            assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b), f"member {j}"
