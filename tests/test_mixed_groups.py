"""Mixed groups (SPEC.md §3 "Mixed groups"): a collection whose tables differ in dim — one pooled lookup, class-major output, grouped step.
CPU: the layout function and the library's exports.  GPU: every operator against TWIN tables (each member has an identically filled
LookupTable of its own that runs the single-table operator), which is the definition; bit-exact except the step over duplicate keys
(SPEC.md §4: rtol 1e-6, atol 1e-9)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL, ATOL = 1e-6, 1e-9   # tests/test_gpu_parity.py
DIMS = (8, 64, 128, 100, 64, 8)   # DIM4 16, 32 and run-time; a width below one tile's 64 floats; a repeated width that is not adjacent
# A member wider than 128 floats switches the whole group's lookup to the instance whose run-time row shape holds 16 float4 per lane (any dim up to
# 1024) instead of 2 (dims up to 128): 132 is the first such width, 256 fills lanes 0..15 of four register columns, 516 = 8 columns and a ninth
# that only lane 0 uses.  The dim-8 and dim-64 members then run inside that wide instance.
WIDE = (8, 64, 132, 256, 516)


# ---- CPU ------------------------------------------------------------------------------------------------------------------------
def test_mixed_layout_hand_computed():
    from meepoembedding_amd import mixed_layout
    # dims (64, 8, 64, 128, 8), B = 3: classes 8 -> members 1, 4; 64 -> members 0, 2; 128 -> member 3
    order, offs, total = mixed_layout((64, 8, 64, 128, 8), 3)
    assert order == [1, 4, 0, 2, 3]
    assert offs == [48, 0, 48 + 192, 48 + 384, 24]   # blocks: 1 @ 0 (24 elements), 4 @ 24, 0 @ 48 (192), 2 @ 240, 3 @ 432 (384)
    assert total == 3 * (64 + 8 + 64 + 128 + 8)
    # one class: the uniform group's [T * B, dim]
    assert mixed_layout((64, 64, 64), 5) == ([0, 1, 2], [0, 320, 640], 960)
    # T = 1
    assert mixed_layout((100,), 7) == ([0], [0], 700)
    # B = 0: every block is empty
    assert mixed_layout((64, 8, 64, 128, 8), 0) == ([1, 4, 0, 2, 3], [0, 0, 0, 0, 0], 0)


def test_library_exports_mixed_group_symbols(built):
    """every mee_mixed_group_* entry point of the header is exported by the built library and bound with its signature"""
    import re

    from meepoembedding_amd import _lib
    header = open(os.path.join(ROOT, "include", "meepo_embedding.h")).read()
    names = sorted(set(re.findall(r"\bint (mee_mixed_group_\w+)\(", header)))
    assert names == ["mee_mixed_group_apply_adagrad_pooled", "mee_mixed_group_apply_adam_pooled", "mee_mixed_group_create", "mee_mixed_group_destroy",
                     "mee_mixed_group_find_pooled", "mee_mixed_group_layout", "mee_mixed_group_set_tuning"]
    L = C.CDLL(_lib.LIB_PATH)
    for name in names:
        assert hasattr(L, name), f"{name} is not exported"
        assert name in _lib.PROTOTYPES, f"{name} is not bound"
        decl = re.sub(r"/\*.*?\*/", "", re.search(r"\bint " + name + r"\(([^;]*)\);", header).group(1), flags=re.S)
        assert len(_lib.PROTOTYPES[name][1]) == decl.count(",") + 1, f"{name}: bound with another number of arguments than declared"
    p = _lib.PROTOTYPES
    assert p["mee_mixed_group_find_pooled"][1][6] is C.c_uint32 and p["mee_mixed_group_find_pooled"][1][-3:-1] == [C.c_int, C.c_int]
    assert p["mee_mixed_group_apply_adam_pooled"][1][-2] is C.c_uint64


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _members(dev, dims, opt=0, cap=512, fill=200, seed=0, **kw):
    """-> (members of the group, their twins, the stored keys of every member)"""
    from meepoembedding_amd import LookupTable, synth
    rng = np.random.default_rng(seed)
    a, b, univ = [], [], []
    for j, d in enumerate(dims):
        u = synth.keys_np(700 + j, 0, fill)
        rows = rng.standard_normal((fill, d)).astype(np.float32)
        kws = dict(default_value=0.125 * (j + 1), initial_accumulator=0.1, init_seed=5 + j, **kw)
        for lst in (a, b):
            t = LookupTable(cap, d, device=dev, optimizer=opt, max_batch=4096, **kws)
            t.insert(T(u, dev), T(rows, dev))
            lst.append(t)
        univ.append(u)
    return a, b, univ


def _batch(rng, univ, B, long_avg=False, empty_member=None, specials=True, unique=False, reclaimed=True):
    """bags: empty, of length 1, short, at and above kPoolLong = 16; keys repeated within and across bags, an absent key, EMPTY and RECLAIMED"""
    from meepoembedding_amd import EMPTY_KEY, RECLAIMED_KEY, synth
    n_t = len(univ)
    lens = rng.integers(8, 40, n_t * B) if long_avg else rng.choice([0, 0, 1, 1, 2, 3, 5, 16, 23], n_t * B)   # average 24 | 5.7 (the launch shape flips at 12)
    if long_avg:
        lens[0], lens[-1] = 0, 1
    else:
        lens[:4] = [0, 1, 16, 15][:min(4, lens.size)]
    if unique:
        lens = np.minimum(lens, univ[0].size // B)
    if empty_member is not None:
        lens[empty_member * B:(empty_member + 1) * B] = 0
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    segs = []
    for j in range(n_t):
        m = int(off[(j + 1) * B] - off[j * B])
        k = (rng.permutation(univ[j])[:m] if unique else univ[j][rng.integers(0, univ[j].size, m)]).copy()
        if specials and m > 6:
            k[1] = synth.keys_np(997, j, 1)[0]   # absent
            k[2] = EMPTY_KEY
            if reclaimed:
                k[3] = RECLAIMED_KEY
            if not unique:
                k[4] = k[0]
        segs.append(k)
    return np.concatenate(segs) if segs else np.zeros(0, np.int64), off


def _check_lookup(grp, twins, keys, off, B, mode, dev, out_dtype=torch.float32):
    """twins: the rows, found.  located: the slots locate() reports on the group's OWN members (where a key sits inside its bucket depends on the
    order in which the insert's tiles claimed slots, so a twin's slots may differ)"""
    from _pooled_cases import assert_out
    from meepoembedding_amd import EMPTY_KEY, _lib
    for t in list(grp.tables) + list(twins):
        t.clear_status()
    located = torch.full((keys.size,), 7, dtype=torch.int64, device=dev)
    views, found = grp.find_pooled(T(keys, dev), T(off, dev), mode, located=located, out_dtype=out_dtype)
    assert len(views) == len(twins)
    base = views[0]._base if views[0]._base is not None else views[0]
    for j, t in enumerate(twins):
        lo, hi = int(off[j * B]), int(off[(j + 1) * B])
        eo, ef = t.find_pooled(T(keys[lo:hi], dev), T(off[j * B:(j + 1) * B + 1] - lo, dev), mode)
        assert views[j].shape == (B, t.dim) and views[j].dtype == out_dtype
        assert views[j].data_ptr() == base.data_ptr() + grp.layout(B)[0][j] * base.element_size()   # a view of the one buffer, at the library's offset
        assert_out(views[j], eo.cpu().numpy(), f"member {j} (dim {t.dim})")   # bitwise; bf16: the fp32 row rounded by SPEC.md §3's integer rule
        assert torch.equal(found[lo:hi], ef), f"found of member {j}"
    assert [t.status() for t in grp.tables] == [t.status() for t in twins]   # (before locate below, which flags a RECLAIMED key on its own)
    for j in range(len(twins)):
        lo, hi = int(off[j * B]), int(off[(j + 1) * B])
        if hi > lo:
            slots, _ = grp.tables[j].locate(T(keys[lo:hi], dev))
            expect = torch.where(slots >= 0, (slots & _lib.HANDLE_SLOT_MASK) | (j << 48), torch.full_like(slots, EMPTY_KEY))
            assert torch.equal(located[lo:hi], expect), f"located of member {j}"
    return views, found


def _assert_same_tables(a, b, exact, what=""):
    for j, (x, y) in enumerate(zip(a, b)):
        assert x.size() == y.size(), f"{what} member {j}: size"
        assert x.status() == y.status(), f"{what} member {j}: status {x.status()} vs {y.status()}"
        ex = [p.cpu().numpy() for p in x.export(with_state=True) if p is not None]
        ey = [p.cpu().numpy() for p in y.export(with_state=True) if p is not None]
        ix, iy = np.argsort(ex[0]), np.argsort(ey[0])
        assert np.array_equal(ex[0][ix], ey[0][iy]), f"{what} member {j}: keys"
        for p, q in zip(ex[1:], ey[1:]):
            if exact:
                assert np.array_equal(p[ix], q[iy]), f"{what} member {j}: planes differ"
            else:
                np.testing.assert_allclose(p[ix], q[iy], rtol=RTOL, atol=ATOL, err_msg=f"{what} member {j}")


@pytest.fixture(scope="module")
def plain(dev):
    """tables without optimizer behind one mixed group, and their twins: shared by the read-only tests"""
    from meepoembedding_amd import MixedTableGroup
    a, b, univ = _members(dev, DIMS)
    grp = MixedTableGroup(a)
    yield grp, a, b, univ
    grp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["sum", "mean"])
@pytest.mark.parametrize("B", [1, 5, 8])
def test_lookup_equals_per_member_find_pooled(dev, plain, B, mode):
    """fp32, the tile-per-bag launch shape: views, found, located and status bits are those of LookupTable.find_pooled / locate per member"""
    grp, a, b, univ = plain
    rng = np.random.default_rng(B)
    keys, off = _batch(rng, univ, B, empty_member=2)
    assert 0 < keys.size < 12 * len(a) * B
    _check_lookup(grp, b, keys, off, B, mode, dev)
    assert grp.layout(B) == tuple(__import__("meepoembedding_amd").mixed_layout(DIMS, B)[1:])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["sum", "mean"])
def test_lookup_wave_per_bag_shape(dev, plain, mode):
    """a batch whose average bag is long takes the wave-per-bag launch shape"""
    grp, a, b, univ = plain
    rng = np.random.default_rng(11)
    keys, off = _batch(rng, univ, 5, long_avg=True, empty_member=4)
    assert keys.size >= 12 * len(a) * 5
    _check_lookup(grp, b, keys, off, 5, mode, dev)


@pytest.mark.gpu
@pytest.mark.parametrize("long_avg", [False, True])
def test_lookup_bf16_is_the_rounded_fp32_result(dev, plain, long_avg):
    grp, a, b, univ = plain
    rng = np.random.default_rng(12)
    keys, off = _batch(rng, univ, 5, long_avg=long_avg, empty_member=0)
    v32, f32 = grp.find_pooled(T(keys, dev), T(off, dev), "mean")
    v16, f16 = _check_lookup(grp, b, keys, off, 5, "mean", dev, out_dtype=torch.bfloat16)
    for x, y in zip(v32, v16):
        assert y.dtype == torch.bfloat16 and torch.equal(y, x.to(torch.bfloat16))
    assert torch.equal(f32, f16)


@pytest.fixture(scope="module")
def wide(dev):
    """as `plain`, with members wider than 128 floats"""
    from meepoembedding_amd import MixedTableGroup
    a, b, univ = _members(dev, WIDE, seed=3)
    grp = MixedTableGroup(a)
    yield grp, a, b, univ
    grp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("long_avg", [False, True], ids=["tile_per_bag", "wave_per_bag"])
@pytest.mark.parametrize("mode", ["sum", "mean"])
def test_lookup_wide_rows(dev, wide, mode, long_avg, out_dtype):
    """dims above 128 (the lookup instance with 16 float4 per lane on its run-time path), both launch shapes, fp32 and bf16: every member,
    the narrow ones included, equals LookupTable.find_pooled on its twin"""
    grp, a, b, univ = wide
    rng = np.random.default_rng(31 + long_avg)
    B = 5
    keys, off = _batch(rng, univ, B, long_avg=long_avg, empty_member=1)
    assert (keys.size >= 12 * len(a) * B) == long_avg
    _check_lookup(grp, b, keys, off, B, mode, dev, out_dtype=out_dtype)
    assert grp.layout(B) == tuple(__import__("meepoembedding_amd").mixed_layout(WIDE, B)[1:])


@pytest.mark.gpu
def test_zero_bags_and_zero_keys(dev, plain):
    grp, a, b, univ = plain
    e = torch.zeros(0, dtype=torch.int64, device=dev)
    views, found = grp.find_pooled(e, torch.zeros(1, dtype=torch.int64, device=dev))
    assert [tuple(v.shape) for v in views] == [(0, d) for d in DIMS] and found.numel() == 0
    views, _ = grp.find_pooled(e, torch.zeros(2 * len(DIMS) + 1, dtype=torch.int64, device=dev))   # two bags per member, all empty
    assert all(v.shape == (2, d) and not bool(v.any()) for v, d in zip(views, DIMS))


@pytest.mark.gpu
def test_insert_missing(dev):
    """tables and found afterwards == the twins' find_or_insert followed by find_pooled; a full member reports TABLE_FULL, alone"""
    from meepoembedding_amd import (INIT_UNIFORM, OPT_ADAGRAD, STATUS_RESERVED_KEY, STATUS_TABLE_FULL, LookupTable, MixedTableGroup, synth)
    dims = (8, 64, 100, 128)
    a, b, univ = _members(dev, dims, opt=OPT_ADAGRAD, initializer=INIT_UNIFORM, init_scale=0.05)
    cap = LookupTable(16, 64, device=dev).capacity          # (the smallest table the library makes)
    full_keys = synth.keys_np(55, 0, cap)
    for lst in (a, b):   # member 4: every slot taken — exactly `capacity` keys, so both twins hold the same set whatever the claiming order was
        t = LookupTable(16, 64, device=dev, optimizer=OPT_ADAGRAD, max_batch=4096, initializer=INIT_UNIFORM, init_scale=0.05, init_seed=9)
        t.insert(T(full_keys, dev), torch.ones(cap, 64, device=dev))
        assert t.size() == t.capacity == cap and t.status() == 0
        lst.append(t)
    univ.append(full_keys)
    grp = MixedTableGroup(a)
    rng = np.random.default_rng(4)
    B = 5
    keys, off = _batch(rng, univ, B)
    fresh = synth.keys_np(4242, 0, 40)
    for j in range(len(a)):   # unseen keys, some twice in one member, the same key values in every member
        lo, hi = int(off[j * B]), int(off[(j + 1) * B])
        idx = rng.choice(np.arange(lo, hi), size=min(14, hi - lo), replace=False)
        keys[idx] = fresh[rng.integers(0, 10, idx.size)]
    located = torch.empty(keys.size, dtype=torch.int64, device=dev)
    views, found = grp.find_pooled(T(keys, dev), T(off, dev), "sum", located=located, insert_missing=True)
    for j, t in enumerate(b):
        lo, hi = int(off[j * B]), int(off[(j + 1) * B])
        _, ef = t.find_or_insert(T(keys[lo:hi], dev))
        eo, _ = t.find_pooled(T(keys[lo:hi], dev), T(off[j * B:(j + 1) * B + 1] - lo, dev), "sum")
        assert torch.equal(found[lo:hi], ef), f"found (present before the call) of member {j}"
        assert torch.equal(views[j], eo), f"member {j}"
    assert not bool(found.all()) and bool(found.any())
    _assert_same_tables(a, b, exact=True, what="after insert_missing")
    assert a[4].status() & STATUS_TABLE_FULL and all(not (t.status() & STATUS_TABLE_FULL) for t in a[:4])
    assert a[0].status() & STATUS_RESERVED_KEY   # the RECLAIMED key of its batch (equal to the twin's: checked above)
    assert a[0].size() > 200
    grp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("use_located", [True, False], ids=["located", "probe"])
@pytest.mark.parametrize("opt", ["adagrad", "adam"])
@pytest.mark.parametrize("dims", [DIMS, WIDE], ids=["narrow", "wide"])
def test_step_equals_per_member_indexed_apply(dev, dims, opt, use_located):
    """two steps (unique keys, then duplicates; both launch shapes of the forward), then a reserve() of one member and a third step.
    The RESERVED_KEY status bit of a step comes from its probe path only: with located handles the select launch reads no key (a RECLAIMED
    key has no handle and is skipped silently, as in TableGroup.apply_pooled), while the per-member apply of the twins probes and flags it.
    So the located runs keep RECLAIMED keys out of their batches; the probe runs carry them and compare the status bits too."""
    from meepoembedding_amd import OPT_ADAGRAD, OPT_ADAM, MixedTableGroup
    a, b, univ = _members(dev, dims, opt=OPT_ADAGRAD if opt == "adagrad" else OPT_ADAM)
    grp = MixedTableGroup(a, max_apply_batch=4096)
    rng = np.random.default_rng(21)
    B = 5

    def step(no, unique):
        keys, off = _batch(rng, univ, B, long_avg=(no == 2), unique=unique, reclaimed=not use_located)
        located = torch.empty(keys.size, dtype=torch.int64, device=dev) if use_located else None
        grp.find_pooled(T(keys, dev), T(off, dev), "sum", located=located)
        lens = np.diff(off)
        bag_of = np.repeat(np.arange(lens.size), lens).astype(np.int64)
        grads = [(rng.standard_normal((B, d)) * 0.05).astype(np.float32) for d in dims]
        flat = torch.empty(grp.layout(B)[1], device=dev)
        for v, g in zip(grp.views(flat, B), grads):
            v.copy_(T(g, dev))
        kw = dict(lr=0.05) if opt == "adagrad" else dict(lr=0.01, step=no)
        grp.apply_pooled(T(keys, dev), T(off, dev), flat, T(bag_of, dev), opt, located=located, **kw)
        for j, t in enumerate(b):
            lo, hi = int(off[j * B]), int(off[(j + 1) * B])
            if hi > lo:
                fn = t.apply_adagrad if opt == "adagrad" else t.apply_adam
                fn(T(keys[lo:hi], dev), T(grads[j], dev), grad_index=T(bag_of[lo:hi] - j * B, dev), **kw)

    step(1, unique=True)
    _assert_same_tables(a, b, exact=True, what="unique keys:")      # no duplicate reduction: bit-identical to the per-member calls
    step(2, unique=False)
    _assert_same_tables(a, b, exact=False, what="duplicates:")
    a[3].reserve(2048); b[3].reserve(2048)                           # member 3's planes move: the descriptors must follow
    step(3, unique=False)
    _assert_same_tables(a, b, exact=False, what="after reserve:")
    grp.close()


@pytest.mark.gpu
def test_70_small_tables_of_three_widths(dev):
    """past the 64 descriptors the grouped apply stages in LDS: the dim-8 class alone has 66 members"""
    from meepoembedding_amd import OPT_ADAGRAD, MixedTableGroup
    dims = tuple([8] * 30 + [64, 16] + [8] * 36 + [16, 64])
    assert len(dims) == 70 and dims.count(8) == 66
    a, b, univ = _members(dev, dims, opt=OPT_ADAGRAD, cap=64, fill=40)
    grp = MixedTableGroup(a, max_apply_batch=4096)
    rng = np.random.default_rng(70)
    B = 3
    keys, off = _batch(rng, univ, B, unique=True, specials=False)
    located = torch.empty(keys.size, dtype=torch.int64, device=dev)
    views, found = grp.find_pooled(T(keys, dev), T(off, dev), "sum", located=located)
    bag_of = np.repeat(np.arange(off.size - 1), np.diff(off)).astype(np.int64)
    grads = [(rng.standard_normal((B, d)) * 0.05).astype(np.float32) for d in dims]
    flat = torch.empty(grp.layout(B)[1], device=dev)
    for v, g in zip(grp.views(flat, B), grads):
        v.copy_(T(g, dev))
    grp.apply_pooled(T(keys, dev), T(off, dev), flat, T(bag_of, dev), "adagrad", lr=0.05, located=located)
    for j, t in enumerate(b):
        lo, hi = int(off[j * B]), int(off[(j + 1) * B])
        eo, ef = t.find_pooled(T(keys[lo:hi], dev), T(off[j * B:(j + 1) * B + 1] - lo, dev), "sum")
        assert torch.equal(views[j], eo) and torch.equal(found[lo:hi], ef), f"member {j}"
        if hi > lo:
            t.apply_adagrad(T(keys[lo:hi], dev), T(grads[j], dev), lr=0.05, grad_index=T(bag_of[lo:hi] - j * B, dev))
    _assert_same_tables(a, b, exact=True, what="70 tables:")
    grp.close()


@pytest.mark.gpu
def test_uniform_dims_delegate_to_table_group(dev):
    """equal dims: lookup and step are TableGroup's, bit for bit"""
    from meepoembedding_amd import OPT_ADAM, MixedTableGroup, TableGroup
    dims = (64, 64, 64)
    a, b, univ = _members(dev, dims, opt=OPT_ADAM)
    mg, tg = MixedTableGroup(a, max_apply_batch=4096), TableGroup(b, max_apply_batch=4096)
    rng = np.random.default_rng(5)
    B = 6
    for no, mode in ((1, "sum"), (2, "mean")):
        keys, off = _batch(rng, univ, B, long_avg=(no == 2))
        l1, l2 = (torch.empty(keys.size, dtype=torch.int64, device=dev) for _ in range(2))
        views, found = mg.find_pooled(T(keys, dev), T(off, dev), mode, located=l1)
        eo, ef = tg.find_pooled(T(keys, dev), T(off, dev), mode, located=l2)
        assert torch.equal(views[0]._base.view(len(dims) * B, 64), eo) and torch.equal(found, ef)
        # (where a key sits inside its bucket depends on the claiming order of each twin's insert: the handles agree in member and presence)
        assert torch.equal(l1 >> 48, l2 >> 48) and torch.equal(l1 < 0, l2 < 0)
        bag_of = T(np.repeat(np.arange(off.size - 1), np.diff(off)).astype(np.int64), dev)
        g = T((rng.standard_normal((len(dims) * B, 64)) * 0.05).astype(np.float32), dev)
        mg.apply_pooled(T(keys, dev), T(off, dev), g, bag_of, "adam", lr=0.01, step=no, located=l1 if no == 1 else None)
        tg.apply_pooled(T(keys, dev), T(off, dev), g, bag_of, "adam", lr=0.01, step=no, located=l2 if no == 1 else None)
        _assert_same_tables(a, b, exact=True, what=f"uniform step {no}:")
    mg.close(); tg.close()


@pytest.mark.gpu
def test_refusals_happen_before_any_launch(dev):
    """mixed optimizers with a step, mixed devices, a batch beyond max_apply_batch, weighted bags, a sharded group over a mixed group, a wrong
    output size: all refused, and the tables are untouched.
    The mixed-devices refusal needs a table on a second GPU.  On a machine with one GPU that branch does NOT run, and the device comparison
    in mee_mixed_group_create is then exercised by no test (the other refusals do not depend on it)."""
    from meepoembedding_amd import OPT_ADAGRAD, OPT_ADAM, LookupTable, MeepoError, MixedTableGroup, _lib
    from meepoembedding_amd.nn import DynamicEmbeddingBag
    from meepoembedding_amd.sharded import ShardedTableGroup
    t8 = LookupTable(64, 8, device=dev, optimizer=OPT_ADAGRAD, max_batch=256)
    t64 = LookupTable(64, 64, device=dev, optimizer=OPT_ADAGRAD, max_batch=256)
    tadam = LookupTable(64, 64, device=dev, optimizer=OPT_ADAM, max_batch=256)
    with pytest.raises(MeepoError) as e:   # mixed optimizers with a step
        MixedTableGroup([t8, tadam], max_apply_batch=64)
    assert e.value.code == _lib.ERR_INVALID_ARG
    MixedTableGroup([t8, tadam]).close()   # lookups only: allowed, as TableGroup
    if torch.cuda.device_count() > 1:      # mixed devices (a table on another device needs a second GPU)
        other = LookupTable(64, 64, device=torch.device("cuda", 1))
        with pytest.raises(MeepoError) as e:
            MixedTableGroup([t8, other])
        assert e.value.code == _lib.ERR_INVALID_ARG
    grp = MixedTableGroup([t8, t64], max_apply_batch=8)
    keys = torch.arange(1, 13, dtype=torch.int64, device=dev)
    off = torch.tensor([0, 3, 6, 9, 12], dtype=torch.int64, device=dev)
    before = [t.export(with_state=True) for t in (t8, t64)]
    with pytest.raises(MeepoError) as e:   # a batch beyond max_apply_batch
        grp.apply_pooled(keys, off, torch.zeros(2 * 72, device=dev), torch.arange(4, device=dev).repeat_interleave(3), "adagrad", lr=0.1)
    assert e.value.code == _lib.ERR_BATCH_TOO_LARGE
    with pytest.raises(ValueError, match="weighted"):   # weighted bags
        grp.find_pooled(keys, off, "sum", weights=torch.ones(12, device=dev))
    layer = DynamicEmbeddingBag(grp, mode="sum")
    with pytest.raises(ValueError, match="per_sample_weights"):
        layer(keys, off, per_sample_weights=torch.ones(12, device=dev))
    with pytest.raises(ValueError, match="different dims"):   # a mixed group under a sharded group
        ShardedTableGroup(grp, router=None)
    with pytest.raises(MeepoError):   # wrong output size
        grp.find_pooled(keys, off, "sum", out=torch.empty(7, device=dev))
    assert [t.size() for t in (t8, t64)] == [0, 0] and [t.status() for t in (t8, t64)] == [0, 0]
    for x, y in zip(before, [t.export(with_state=True) for t in (t8, t64)]):
        assert all(torch.equal(p, q) for p, q in zip(x, y) if p is not None)
    grp.close()
