"""Sparse FTRL-Proximal (SPEC.md §4 "FTRL-Proximal"): the reference's own sanity, SparseStep's ftrl kind, the header / loader sync, and — on the
GPU — every form of the step bit for bit against tests/_ftrl_ref.py through the sorted export of all three planes (row, z, n)."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

from _ftrl_ref import FtrlRefTable, ftrl_update, reduce_duplicates
from meepoembedding_amd import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL, ATOL = 1e-6, 1e-9   # SPEC.md §4: duplicates with ordinary gradients (the order of the fp64 sum is free)
ENTRY_POINTS = ["mee_apply_ftrl", "mee_apply_ftrl_located", "mee_apply_ftrl_indexed", "mee_group_apply_ftrl", "mee_group_apply_ftrl_pooled",
                "mee_group_apply_ftrl_indexed", "mee_mixed_group_apply_ftrl_pooled"]
PARAMS = [(b, l1, l2) for b in (1.0, 0.5) for l1 in (0.0, 0.02) for l2 in (0.0, 0.001)]


# ---- no GPU: the reference, SparseStep, the declarations -------------------------------------------------------------------------------------------
def test_reference_without_regularisation_is_per_coordinate_gradient_descent():
    """fp64, l1 = l2 = 0, w0 = 0: 50 steps equal w -= lr / (beta + sqrt(n_t)) * g_t to 1e-12 (McMahan et al. 2013, §3: the two are the same algorithm)"""
    rng = np.random.default_rng(1)
    lr, beta = 0.1, 1.0
    w = z = np.zeros((64, 16)); n = np.zeros((64, 16))
    wd, nd = np.zeros((64, 16)), np.zeros((64, 16))
    for _ in range(50):
        g = rng.standard_normal((64, 16)) * 0.1
        w, z, n = ftrl_update(w, z, n, g, lr, beta, 0.0, 0.0, dtype=np.float64)
        nd = nd + g * g
        wd = wd - lr / (beta + np.sqrt(nd)) * g
    err = float(np.abs(w - wd).max())
    print(f"max |ftrl - ogd| after 50 fp64 steps: {err:.3g}")
    assert err <= 1e-12 and float(np.abs(wd).max()) > 1e-3


def test_reference_l1_gives_exact_zeros():
    rng = np.random.default_rng(2)
    w = (rng.standard_normal((256, 16)) * 0.01).astype(np.float32)
    z = np.zeros_like(w); n = np.full_like(w, 0.1)
    for _ in range(3):
        g = (rng.standard_normal(w.shape) * 0.02).astype(np.float32)
        w, z, n = ftrl_update(w, z, n, g, 0.05, 1.0, 0.02, 0.001)
    small = np.abs(z) <= np.float32(0.02)
    assert np.array_equal(w[small].view(np.uint32), np.zeros(int(small.sum()), dtype=np.uint32))   # exactly +0.0, not -0.0
    assert small.mean() >= 0.1 and (~small).mean() >= 0.1 and bool((w[~small] != 0).all())


def test_reference_tells_a_fused_step_apart():
    """what a contracting compiler would make of `z' = (z + g) - sig*w` (one fma) or of `n' = n + g*g` gives other bits on the inputs of the GPU
    tests below: the bit-for-bit comparisons there can tell"""
    keys, rows, batch, grads = distinct_case(64)
    for fused in ("sw", "nn"):
        a, b = FtrlRefTable(64, 0.1), FtrlRefTable(64, 0.1)
        for t in (a, b):
            t.insert(keys, rows)
        for g in grads:
            a.apply(batch, g, 0.05, 1.0, 0.02, 0.001)
            b.apply(batch, g, 0.05, 1.0, 0.02, 0.001, fused=(fused,))
        differing = sum(int((x.view(np.uint32) != y.view(np.uint32)).sum()) for x, y in zip(a.export_sorted()[1:], b.export_sorted()[1:]))
        print(f"fused {fused}: {differing} elements differ")
        assert differing >= 1


def test_reduce_duplicates_rounds_once_and_copies_singles():
    keys = np.array([5, 7, 5, 9, 5, _lib.EMPTY_KEY, 7], dtype=np.int64)
    g = np.array([[1.0], [2.0 ** -30], [2.0 ** -25], [np.float32(0.1)], [-1.0], [99.0], [1.0]], dtype=np.float32)
    uk, ug = reduce_duplicates(keys, g)
    assert uk.tolist() == [5, 7, 9]
    assert ug[0, 0] == np.float32(2.0 ** -25) and ug[1, 0] == np.float32(1.0 + 2.0 ** -30) == np.float32(1.0) and ug[2, 0] == np.float32(0.1)


def test_sparse_step_of_ftrl(built, monkeypatch):
    from meepoembedding_amd import table as tm
    S = tm.SparseStep
    s = S.of("ftrl", 0.1)
    assert s.kind == "ftrl" and s.eps == 1.0 and (s.l1, s.l2) == (0.0, 0.0) and s.tail() == (0.1, 1.0, 0.0, 0.0)
    s = S.of("ftrl", 0.1, 0.5, l1=0.02, l2=0.001)
    assert (s.eps, s.l1, s.l2) == (0.5, 0.02, 0.001) and s.tail() == (0.1, 0.5, 0.02, 0.001) and s.tail() == (s.lr, s.eps, s.beta1, s.beta2)
    assert S.of("ftrl", 0.1, beta1=0.9, beta2=0.999).tail() == (0.1, 1.0, 0.0, 0.0)   # Adam's defaults never become regularisation strengths
    assert S.of("ftrl", 0.1, None, 0.9, 0.999, 7, l1=0.25).tail() == (0.1, 1.0, 0.25, 0.0)
    assert S._fields == ("kind", "lr", "eps", "beta1", "beta2", "step")
    assert S.of("ftrl", 0.1, l1=0.02, l2=0.5).loose_kw() == {"l1": 0.02, "l2": 0.5} and S.of("adam", 0.1).loose_kw() == {} and S.of("adagrad", 0.1).loose_kw() == {}
    with pytest.raises(AttributeError):
        s.l1 = 1.0
    calls = []

    class Recorder:
        def __getattr__(self, name):
            return lambda *a: calls.append((name, a)) or 0

    monkeypatch.setattr(tm._lib, "lib", lambda: Recorder())
    step = S.of("ftrl", 0.1, 0.5, l1=0.02, l2=0.001)
    tail = (0.1, 0.5, 0.02, 0.001, 9)
    for stem, form in (("mee_apply", ""), ("mee_apply", "_located"), ("mee_apply", "_indexed"), ("mee_group_apply", ""), ("mee_group_apply", "_pooled"),
                       ("mee_group_apply", "_indexed"), ("mee_mixed_group_apply", "_pooled")):
        step.launch(stem, form, 1, 2, stream=9)
    assert [c[0] for c in calls] == ENTRY_POINTS and all(c[1] == (1, 2) + tail for c in calls)
    assert all(name in _lib.PROTOTYPES for name in ENTRY_POINTS)

    class Three:
        def apply_ftrl(self, keys, grads, lr, beta=1.0, l1=0.0, l2=0.0, grad_index=None):
            self.got = (lr, beta, l1, l2, grad_index)

    three = Three()
    step.apply_to(three, "k", "g", grad_index="gi")
    assert three.got == (0.1, 0.5, 0.02, 0.001, "gi")


def test_entry_points_are_declared_and_bound(built):
    header = open(os.path.join(ROOT, "include", "meepo_embedding.h")).read()
    assert re.search(r"MEE_OPT_FTRL\s*=\s*3\b", header) and _lib.OPT_FTRL == 3
    import meepoembedding_amd
    assert meepoembedding_amd.OPT_FTRL == 3 and "OPT_FTRL" in meepoembedding_amd.__all__
    L = C.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        m = re.search(r"\bint\s+" + name + r"\(([^;]*)\);", header)
        assert m, f"{name} is not declared in the header"
        decl = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        assert hasattr(L, name), f"{name} is not exported"
        args = _lib.PROTOTYPES[name][1]
        assert len(args) == decl.count(",") + 1, f"{name}: bound with another number of arguments than declared"
        assert args[-5:-1] == [C.c_float] * 4 and "float lr, float beta" in re.sub(r"\s+", " ", decl) and re.sub(r"\s+", " ", decl).rstrip().endswith("float l2, void* stream")
        twin = _lib.PROTOTYPES[name.replace("ftrl", "adagrad")][1]
        assert args == twin[:-3] + [C.c_float] * 4 + twin[-1:], f"{name} is not its Adagrad twin plus (beta, l1, l2) after lr"


def test_layers_and_loose_forms_take_the_keywords(built):
    import inspect

    from meepoembedding_amd import LookupTable, MixedTableGroup, TableGroup, TieredLookupTable, TieredTableGroup, nn
    for cls in (LookupTable, TableGroup, TieredLookupTable, TieredTableGroup):
        p = inspect.signature(cls.apply_ftrl).parameters
        assert [p[k].default for k in ("beta", "l1", "l2")] == [1.0, 0.0, 0.0], cls
    for fn in (TableGroup.apply_pooled, TableGroup.apply_indexed, MixedTableGroup.apply_pooled, TieredTableGroup.apply_pooled, TieredTableGroup.apply_indexed):
        p = inspect.signature(fn).parameters
        assert p["l1"].default == 0.0 and p["l2"].default == 0.0, fn
    for layer in (nn.DynamicEmbedding, nn.DynamicEmbeddingBag, nn.DynamicEmbeddingCollection, nn.DynamicEmbeddingSequence):
        p = inspect.signature(layer.__init__).parameters
        assert p["l1"].default == 0.0 and p["l2"].default == 0.0, layer


def test_a_layer_over_a_table_without_apply_ftrl_is_refused_by_name(built):
    """no GPU needed: the refusal is read off the object's methods at construction"""
    from meepoembedding_amd import nn

    class TwoOptimizers:
        dim = 8
        def find(self, keys): ...
        def find_or_insert(self, keys): ...
        def apply_adagrad(self, keys, grads, lr, eps=1e-10, grad_index=None): ...
        def apply_adam(self, keys, grads, lr, beta1=0.9, beta2=0.999, eps=1e-8, step=1, grad_index=None): ...

    class OldGroup(TwoOptimizers):
        tables = ()
        def apply_ftrl(self, keys, offsets, grads, lr, beta=1.0, l1=0.0, l2=0.0): ...
        def apply_pooled(self, keys, bag_offsets, bag_grads, bag_of_position, optimizer, lr, eps=None, beta1=0.9, beta2=0.999, step=1, located=None): ...

    for obj in (TwoOptimizers(), OldGroup()):
        for make in (lambda t: nn.DynamicEmbeddingBag(t, optimizer="ftrl", l1=0.02), lambda t: nn.DynamicEmbedding(t, optimizer="ftrl")):
            with pytest.raises(ValueError, match=r"optimizer='ftrl' needs a table with apply_ftrl.*" + type(obj).__name__):
                make(obj)
        nn.DynamicEmbeddingBag(obj, optimizer="adagrad")   # the other two are served as before
    with pytest.raises(ValueError, match="optimizer must be 'adagrad' or 'adam' or 'ftrl'"):
        nn.DynamicEmbeddingBag(TwoOptimizers(), optimizer="sgd")


# ---- shared inputs (host side, computed once, read-only) -------------------------------------------------------------------------------------------
def T(a, dev):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).to(dev)


def frozen(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays


@functools.lru_cache(maxsize=None)
def distinct_case(dim):
    """600 stored keys with small rows; a batch of 512 of them and 64 absent keys, all distinct; three steps of ordinary gradients"""
    keys = synth.keys_np(41, 0, 700)
    rows = (synth.rows_np(keys[:600], dim, 2) * 0.05).astype(np.float32)
    rng = np.random.default_rng(100 + dim)
    batch = rng.permutation(np.concatenate([keys[:512], keys[600:664]]))
    grads = [(rng.standard_normal((batch.size, dim)) * 0.05).astype(np.float32) for _ in range(3)]
    return frozen(keys[:600], rows, batch, *grads)[:3] + (grads,)


def export_sorted(t):
    e = [x.cpu().numpy() for x in t.export(with_state=True) if x is not None]
    order = np.argsort(e[0])
    return [x[order] for x in e]


def assert_table_bits(t, ref, what=""):
    """keys, rows, z and n of the table == the reference's, bit for bit (NaN where the reference is NaN)"""
    from _apply_cases import assert_bits_equal_nan_aware
    e, r = export_sorted(t), (ref.export_sorted() if isinstance(ref, FtrlRefTable) else ref)
    assert len(e) == len(r) == 4, f"{what}: an FTRL table exports keys and three planes"
    assert np.array_equal(e[0], r[0]), f"{what}: keys"
    for name, x, y in zip(("rows", "z", "n"), e[1:], r[1:]):
        assert_bits_equal_nan_aware(x, y, f"{what} {name}")


def ftrl_table(dev, dim, keys=None, rows=None, capacity=4096, max_batch=4096, acc=0.1, **kw):
    from meepoembedding_amd import OPT_FTRL, LookupTable
    t = LookupTable(capacity, dim, device=dev, optimizer=OPT_FTRL, max_batch=max_batch, initial_accumulator=acc, **kw)
    if keys is not None:
        t.insert(T(keys, dev), T(rows, dev))
    return t


def ref_table(dim, keys, rows, acc=0.1):
    r = FtrlRefTable(dim, acc)
    r.insert(keys, rows)
    return r


# ---- GPU: one table -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dim", [24, 64, 128])
def test_distinct_keys_by_key_located_and_indexed(dev, dim):
    """the three row shapes (DIM4 = 0, 16, 32) x every (beta, l1, l2): by key, on find_located's handles, through grad_index; absent keys change nothing"""
    keys, rows, batch, grads = distinct_case(dim)
    bt = T(batch, dev)
    perm = np.random.default_rng(7).permutation(batch.size)
    for beta, l1, l2 in PARAMS:
        ref = ref_table(dim, keys, rows)
        plain, located, indexed = (ftrl_table(dev, dim, keys, rows) for _ in range(3))
        for s, g in enumerate(grads):
            ref.apply(batch, g, 0.05, beta, l1, l2)
            plain.apply_ftrl(bt, T(g, dev), 0.05, beta, l1, l2)
            _, found, slots = located.find_located(bt, prepare_apply=(s == 1))
            assert int(found.sum()) == 512
            located.apply_ftrl(bt, T(g, dev), lr=0.05, beta=beta, l1=l1, l2=l2, slots=slots)
            pool = np.ascontiguousarray(g[perm])                       # row perm[i] of g sits at pool row i: position p reads pool row inv[p]
            indexed.apply_ftrl(bt, T(pool, dev), 0.05, beta, l1, l2, grad_index=T(np.argsort(perm).astype(np.int32), dev))
        for t, form in ((plain, "by key"), (located, "located"), (indexed, "indexed")):
            assert t.status() == 0 and t.size() == 600 and t.optimizer == 3   # (mee_table_info.optimizer)
            assert_table_bits(t, ref, f"dim {dim} beta {beta} l1 {l1} l2 {l2} {form}")
        if l1 > 0:
            w = export_sorted(plain)[1]
            assert 0.02 < float((w.view(np.uint32) == 0).mean()) < 0.98   # the L1 term produced exact +0.0 elements, and not only those


@pytest.mark.gpu
def test_created_keys_start_at_zero_z_and_the_initial_accumulator(dev):
    """find_or_insert on a table with a hashed initializer: z = +0.0, n = initial_accumulator, the row stays until the first step, which then
    computes w' from z' alone (the old row enters only through sig * w); insert() creates the same state"""
    from meepoembedding_amd import INIT_UNIFORM
    dim = 24
    keys = synth.keys_np(43, 0, 300)
    t = ftrl_table(dev, dim, acc=0.25, initializer=INIT_UNIFORM, init_scale=0.05, init_seed=3)
    out, found = t.find_or_insert(T(keys, dev))
    assert int(found.sum()) == 0 and float(out.abs().max()) > 0
    e = export_sorted(t)
    assert np.array_equal(e[2].view(np.uint32), np.zeros_like(e[2]).view(np.uint32)) and np.array_equal(e[3], np.full_like(e[3], 0.25))
    order = np.argsort(keys)
    assert np.array_equal(e[1], out.cpu().numpy()[order])
    ref = ref_table(dim, keys, out.cpu().numpy(), acc=0.25)
    g = (np.random.default_rng(3).standard_normal((300, dim)) * 0.05).astype(np.float32)
    t.apply_ftrl(T(keys, dev), T(g, dev), 0.05, 1.0, 0.01, 0.0)
    ref.apply(keys, g, 0.05, 1.0, 0.01, 0.0)
    assert_table_bits(t, ref, "first step after find_or_insert")
    assert not np.array_equal(export_sorted(t)[1], e[1])


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["clustered", "spread", "mixed"])
@pytest.mark.parametrize("dim", [24, 64])
def test_every_group_size_exact(dev, dim, layout):
    """a key of every multiplicity 1..44, 64, 65, 100, 333, 2100 with exactly summable gradients: bit for bit, by key and located (a partial sum kept
    in fp32 or a second rounding would show)"""
    from _apply_cases import every_group_size_batch, exact_grads_np
    rng = np.random.default_rng(11)
    keys, rows, _, batch = every_group_size_batch(rng, dim, layout)
    rows = (rows * 0.05).astype(np.float32)
    n = batch.size
    ref = ref_table(dim, keys, rows)
    ta, tb = (ftrl_table(dev, dim, keys, rows, max_batch=n) for _ in range(2))
    bt = T(batch, dev)
    for s in range(3):
        g = exact_grads_np(rng, n, dim)
        ref.apply(batch, g, 0.05, 1.0, 0.02, 0.001)
        ta.apply_ftrl(bt, T(g, dev), 0.05, 1.0, 0.02, 0.001)
        _, _, slots = tb.find_located(bt, prepare_apply=(s == 1))
        tb.apply_ftrl(bt, T(g, dev), 0.05, 1.0, 0.02, 0.001, slots=slots)
    for t, form in ((ta, "by key"), (tb, "located")):
        assert t.status() == _lib.STATUS_RESERVED_KEY or t.status() == 0   # (the padding positions are EMPTY keys)
        assert_table_bits(t, ref, f"{layout} dim {dim} {form}")


def extreme_batch(case, dim):
    """the constructions of _apply_cases.bucketed_apply_extremes (which steps Adagrad and Adam against the oracle): -> (stored keys, rows, batch)"""
    from _apply_cases import keys_of_apply_bucket_zero
    n_bg = 20000
    rng = np.random.default_rng(5)
    bg = synth.keys_np(321, 0, n_bg)
    if case == "one_key":
        hot = synth.keys_np(322, 0, 1); reps = np.array([400_000]); n_fill = 10_000
    elif case == "one_bucket_many_keys":
        hot = keys_of_apply_bucket_zero(3000, 7); reps = rng.integers(100, 140, size=3000); n_fill = 20_000
    elif case == "forty_hot_keys":
        hot = synth.keys_np(323, 0, 40); reps = rng.integers(5000, 7000, size=40); n_fill = 30_000
    elif case == "one_bucket_two_keys":
        hot = keys_of_apply_bucket_zero(2, 9); reps = np.array([150_000, 150_001]); n_fill = 5_000
    elif case == "bucket_of_900_distinct":
        hot = keys_of_apply_bucket_zero(900, 11); reps = np.ones(900, dtype=np.int64); n_fill = 5_000
    else:
        hot = keys_of_apply_bucket_zero(300, 12); reps = rng.integers(1, 7, size=300); n_fill = 3_000
    keys = np.unique(np.concatenate([bg, hot]))
    rows = (synth.rows_np(keys, dim, 2) * 0.05).astype(np.float32)
    bk = np.concatenate([np.repeat(hot, reps), bg[rng.integers(0, n_bg, n_fill)], synth.keys_np(324, 0, 50)])   # + 50 absent keys
    rng.shuffle(bk)
    return keys, rows, bk


@pytest.mark.gpu
@pytest.mark.parametrize("kernel,dim", [("lean", 24), ("full", 64)])
@pytest.mark.parametrize("case", ["one_key", "one_bucket_many_keys", "forty_hot_keys", "one_bucket_two_keys", "bucket_of_900_distinct", "bucket_of_300_warm"])
def test_rare_ways_through_the_bucketed_apply_exact(dev, case, kernel, dim):
    """EXTREME_CASES: slabs, pending records, merges, hot keys' own buckets (FULL, three steps) and the split bucket taken by one block (LEAN), with
    exactly summable gradients: by key and located, bit for bit.  These batches are as large as the paths need (up to 410K positions)."""
    from _apply_cases import EXTREME_CASES, exact_grads_dev
    assert case in EXTREME_CASES
    keys, rows, bk = extreme_batch(case, dim)
    n = bk.size
    ref = ref_table(dim, keys, rows)
    ta, tb = (ftrl_table(dev, dim, keys, rows, capacity=1 << 17, max_batch=max(n, keys.size)) for _ in range(2))
    for t in (ta, tb):
        t.set_tuning("apply_kernel", {"lean": 0, "full": 1}[kernel])
    bkt = T(bk, dev)
    gen = torch.Generator(device=dev); gen.manual_seed(dim)
    for s in range(3 if kernel == "full" else 2):
        torch.cuda.synchronize()   # (the host sizes step s + 1 by what step s reported)
        gt, g = exact_grads_dev(gen, n, dim, dev)
        ref.apply(bk, g, 0.05, 1.0, 0.02, 0.001)
        _, _, slots = tb.find_located(bkt, prepare_apply=(s == 1))
        ta.apply_ftrl(bkt, gt, 0.05, 1.0, 0.02, 0.001)
        tb.apply_ftrl(bkt, gt, 0.05, 1.0, 0.02, 0.001, slots=slots)
    for t, form in ((ta, "by key"), (tb, "located")):
        assert t.status() == 0
        assert_table_bits(t, ref, f"{case} {kernel} dim {dim} {form}")


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [24, 64])
def test_duplicates_with_ordinary_gradients_within_the_contract(dev, dim):
    """Zipf ids, l1 = 0 (the threshold is a discontinuity: with l1 > 0 only bit-exact cases are compared): <= 1e-6 relative + 1e-9"""
    keys = synth.keys_np(45, 0, 600)
    rows = (synth.rows_np(keys, dim, 2) * 0.05).astype(np.float32)
    rng = np.random.default_rng(dim)
    ref, t = ref_table(dim, keys, rows), ftrl_table(dev, dim, keys, rows)
    worst = 0.0
    for s in range(3):
        batch = keys[np.minimum(rng.zipf(1.3, size=4096) - 1, 599)]
        g = (rng.standard_normal((4096, dim)) * 0.05).astype(np.float32)
        ref.apply(batch, g, 0.05, 1.0, 0.0, 0.001)
        t.apply_ftrl(T(batch, dev), T(g, dev), 0.05, 1.0, 0.0, 0.001)
    e, r = export_sorted(t), ref.export_sorted()
    for x, y in zip(e[1:], r[1:]):
        worst = max(worst, float((np.abs(x - y) / np.maximum(np.abs(y), 1e-30)).max()))
    print(f"dim {dim}: max relative difference {worst:.3g}")
    for x, y in zip(e[1:], r[1:]):
        np.testing.assert_allclose(x, y, rtol=RTOL, atol=ATOL)


@functools.lru_cache(maxsize=None)
def edge_case(dim, l1):
    """132 distinct keys whose elements walk through (gradient, n, z, w) grids: g = +-0, subnormal, overflowing g*g, inf, NaN, +-l1 (with z = 0 and
    w = 0: z' lands exactly on the threshold); n = 0 (with beta = 0: 0/0); z = +-0"""
    from _apply_cases import EDGE_GRADS, EDGE_WEIGHTS
    rng = np.random.default_rng(900 + dim)
    shape = (132, dim)
    G = np.concatenate([EDGE_GRADS, np.array([l1, -l1, 0.5 * l1, np.nextafter(np.float32(l1), np.float32(1))], dtype=np.float32)])
    N = np.array([0.0, 1e-41, 0.1, 3e38], dtype=np.float32)
    Z = np.array([0.0, -0.0, 1e-41, 0.01, -0.5], dtype=np.float32)
    g, n, z, w = G[rng.integers(0, G.size, shape)], N[rng.integers(0, N.size, shape)], Z[rng.integers(0, Z.size, shape)], EDGE_WEIGHTS[rng.integers(0, EDGE_WEIGHTS.size, shape)].copy()
    # the first 32 rows: z and w zero, so z' = g exactly — the gradients +-l1 sit on the threshold, +-0 give z' = +-0
    z[:32] = np.where(rng.random((32, dim)) < 0.5, np.float32(0.0), np.float32(-0.0)); w[:32] = 0.0
    n[:32] = np.where(n[:32] > 1.0, np.float32(0.1), n[:32])
    return frozen(synth.keys_np(777, 0, 132), w, z, n, g)


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [24, 64])
def test_numeric_edges_on_distinct_keys(dev, dim):
    for beta, l1, l2 in ((0.0, 0.0, 0.0), (1.0, 0.02, 0.001), (0.0, 0.02, 0.0), (1.0, 0.0, 0.0)):
        keys, w, z, n, g = edge_case(dim, np.float32(0.02))
        ref = ref_table(dim, keys, w)
        ref.set_state(keys, z, n)
        t = ftrl_table(dev, dim, keys, w)
        kt = T(keys, dev)
        assert bool(t.assign_plane(1, kt, T(z, dev)).all()) and bool(t.assign_plane(2, kt, T(n, dev)).all())
        ref.apply(keys, g, 0.05, beta, l1, l2)
        t.apply_ftrl(kt, T(g, dev), 0.05, beta, l1, l2)
        assert t.status() == 0
        assert_table_bits(t, ref, f"edges dim {dim} beta {beta} l1 {l1} l2 {l2}")
        r = ref.export_sorted()
        assert np.isnan(r[1]).any() and np.isinf(r[3]).any()
        if l1 > 0:   # the threshold itself: z' == +-l1 gives +0.0, one ulp beyond does not
            order = np.argsort(keys)
            on = (np.abs(g[order]) == np.float32(l1)) & (np.arange(132)[order] < 32)[:, None]
            assert on.any() and np.array_equal(r[1][on].view(np.uint32), np.zeros(int(on.sum()), dtype=np.uint32)) and np.array_equal(np.abs(r[2][on]), np.abs(g[order][on]))


# ---- GPU: groups ----------------------------------------------------------------------------------------------------------------------------------------
def bag_case(n_tables, bags_per_table, seed, n_keys=200, max_len=7):
    """Zipf ids per member, bags of 0..max_len ids, duplicates inside and across a member's bags -> (per-member stored keys, keys, bag offsets)"""
    rng = np.random.default_rng(seed)
    stored = [synth.keys_np(60 + j, 0, n_keys) for j in range(n_tables)]
    lens = rng.integers(0, max_len + 1, size=n_tables * bags_per_table)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    keys = np.concatenate([stored[b // bags_per_table][np.minimum(rng.zipf(1.3, size=l) - 1, n_keys - 1)] for b, l in enumerate(lens)] + [np.empty(0, dtype=np.int64)])
    return stored, keys.astype(np.int64), off


def exact_rows(rng, rows, dim, positions):
    from _apply_cases import exact_grads_np
    return exact_grads_np(rng, rows, dim, positions=positions)


@pytest.mark.gpu
def test_group_steps_equal_the_members_single_table_steps(dev):
    """TableGroup.apply_ftrl / apply_pooled("ftrl") / apply_indexed("ftrl") over three dim-16 members == LookupTable.apply_ftrl per member == the reference"""
    from meepoembedding_amd import TableGroup
    dim, nt, B = 16, 3, 64
    stored, keys, off = bag_case(nt, B, seed=1)
    n = keys.size
    rows = [(synth.rows_np(k, dim, 2) * 0.05).astype(np.float32) for k in stored]
    sets = {name: [ftrl_table(dev, dim, stored[j], rows[j]) for j in range(nt)] for name in ("jagged", "pooled", "indexed", "single")}
    groups = {name: TableGroup(sets[name], max_apply_batch=4096) for name in ("jagged", "pooled", "indexed")}
    refs = [ref_table(dim, stored[j], rows[j]) for j in range(nt)]
    kt, ot = T(keys, dev), T(off, dev)
    seg = off[::B]
    bag_of = np.repeat(np.arange(nt * B), np.diff(off))
    rng = np.random.default_rng(2)
    par = (0.05, 0.5, 0.02, 0.001)
    for s in range(3):
        bag_g = exact_rows(rng, nt * B, dim, n)
        pos_g = bag_g[bag_of]
        groups["jagged"].apply_ftrl(kt, T(seg, dev), T(pos_g, dev), *par)
        loc = torch.empty(n, dtype=torch.int64, device=dev)
        groups["pooled"].find_pooled(kt, ot, "sum", located=loc)
        groups["pooled"].apply_pooled(kt, ot, T(bag_g, dev), T(bag_of, dev), "ftrl", par[0], par[1], l1=par[2], l2=par[3], located=loc if s else None)
        groups["indexed"].apply_indexed(kt, T(seg, dev), T(bag_g, dev), T(bag_of.astype(np.int32), dev), "ftrl", par[0], par[1], l1=par[2], l2=par[3])
        for j in range(nt):
            a, b = int(seg[j]), int(seg[j + 1])
            sets["single"][j].apply_ftrl(kt[a:b], T(bag_g, dev), *par, grad_index=T(bag_of[a:b].astype(np.int32), dev))
            refs[j].apply(keys[a:b], pos_g[a:b], *par)
    for name in sets:
        for j in range(nt):
            assert sets[name][j].status() == 0
            assert_table_bits(sets[name][j], refs[j], f"{name} member {j}")
    for g in groups.values():
        g.close()


@pytest.mark.gpu
def test_mixed_group_and_keyed_layout_steps(dev):
    """MixedTableGroup.apply_pooled("ftrl") over dims 8 / 64 / 100 == its members' steps (table-major and layout="keyed"); a uniform group's keyed-layout
    step through the step index == the table-major one"""
    from meepoembedding_amd import MixedTableGroup, TableGroup
    dims, B = [8, 64, 100], 32
    nt = len(dims)
    stored, keys, off = bag_case(nt, B, seed=3)
    n = keys.size
    rows = [(synth.rows_np(stored[j], d, 2) * 0.05).astype(np.float32) for j, d in enumerate(dims)]
    a, b = ([ftrl_table(dev, d, stored[j], rows[j]) for j, d in enumerate(dims)] for _ in range(2))
    ga, gb = MixedTableGroup(a, max_apply_batch=4096), MixedTableGroup(b, max_apply_batch=4096)
    refs = [ref_table(d, stored[j], rows[j]) for j, d in enumerate(dims)]
    kt, ot = T(keys, dev), T(off, dev)
    seg = off[::B]
    bag_of = np.repeat(np.arange(nt * B), np.diff(off))
    rng = np.random.default_rng(4)
    par = dict(lr=0.05, eps=1.0, l1=0.02, l2=0.001)
    for s in range(2):
        per_member = [exact_rows(rng, B, d, n) for d in dims]
        loc = torch.empty(n, dtype=torch.int64, device=dev)
        views, _ = ga.find_pooled(kt, ot, "sum", located=loc)
        flat = torch.empty_like(views[0]._base if views[0]._base is not None else views[0]).view(-1)
        for j, v in enumerate(ga.views(flat, B)):
            v.copy_(T(per_member[j], dev))
        ga.apply_pooled(kt, ot, flat, T(bag_of, dev), "ftrl", located=loc, **par)
        loc2, idx = torch.empty_like(loc), torch.zeros(n, dtype=torch.int32, device=dev)
        gb.find_pooled(kt, ot, "sum", located=loc2, layout="keyed", step_index=idx)
        gb.apply_pooled(kt, ot, torch.cat([T(p, dev) for p in per_member], dim=1), idx, "ftrl", located=loc2, layout="keyed", **par)
        for j in range(nt):
            lo, hi = int(seg[j]), int(seg[j + 1])
            refs[j].apply(keys[lo:hi], per_member[j][bag_of[lo:hi] - j * B], 0.05, 1.0, 0.02, 0.001)
    for name, tabs in (("table-major", a), ("keyed", b)):
        for j in range(nt):
            assert tabs[j].status() == 0
            assert_table_bits(tabs[j], refs[j], f"mixed {name} member {j} (dim {dims[j]})")
    ga.close(); gb.close()
    # a uniform group: the keyed gradient [B, T * dim] read where it lies
    dim = 16
    rows = [(synth.rows_np(stored[j], dim, 2) * 0.05).astype(np.float32) for j in range(nt)]
    p, k = ([ftrl_table(dev, dim, stored[j], rows[j]) for j in range(nt)] for _ in range(2))
    gp, gk = TableGroup(p, max_apply_batch=4096), TableGroup(k, max_apply_batch=4096)
    for s in range(2):
        grads = T(exact_rows(rng, nt * B, dim, n), dev)
        gp.apply_pooled(kt, ot, grads, T(bag_of, dev), "ftrl", 0.05, l1=0.02, l2=0.001)
        loc2, idx = torch.empty(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
        gk.find_pooled(kt, ot, "sum", located=loc2, layout="keyed", step_index=idx)
        keyed = grads.view(nt, B, dim).transpose(0, 1).contiguous()
        gk.apply_pooled(kt, ot, keyed.view(B * nt, dim), idx, "ftrl", 0.05, l1=0.02, l2=0.001, located=loc2)
    for j in range(nt):
        assert_table_bits(k[j], export_sorted(p[j]), f"keyed uniform member {j}")
        assert float(np.abs(export_sorted(p[j])[2]).max()) > 0
    gp.close(); gk.close()


@pytest.mark.gpu
def test_tiered_pair_and_tiered_group_steps(dev):
    """TieredTableGroup.apply_ftrl / apply_pooled("ftrl") / apply_indexed("ftrl") and TieredLookupTable.apply_ftrl(grad_index=) over two pairs (hot in
    HBM, cold in pinned host memory, keys in both tiers) == the reference of the union, bit for bit; a demote in between carries z and n"""
    from meepoembedding_amd import TieredLookupTable, TieredTableGroup
    dim, nt, B = 16, 2, 32
    stored, keys, off = bag_case(nt, B, seed=9)
    n = keys.size
    rows = [(synth.rows_np(k, dim, 2) * 0.05).astype(np.float32) for k in stored]
    pairs = [TieredLookupTable(ftrl_table(dev, dim, stored[j][:100], rows[j][:100]),
                               ftrl_table(dev, dim, stored[j][100:], rows[j][100:], value_memory=_lib.MEM_HOST_PINNED), hot_key_limit=150) for j in range(nt)]
    group = TieredTableGroup(pairs, max_apply_batch=4096)
    refs = [ref_table(dim, stored[j], rows[j]) for j in range(nt)]
    kt, ot = T(keys, dev), T(off, dev)
    seg = off[::B]
    bag_of = np.repeat(np.arange(nt * B), np.diff(off))
    rng = np.random.default_rng(10)
    par = (0.05, 0.5, 0.02, 0.001)
    for s in range(4):
        bag_g = exact_rows(rng, nt * B, dim, n)
        pos_g = bag_g[bag_of]
        if s == 0:
            group.apply_ftrl(kt, T(seg, dev), T(pos_g, dev), *par)
        elif s == 1:
            group.apply_pooled(kt, ot, T(bag_g, dev), T(bag_of, dev), "ftrl", par[0], par[1], l1=par[2], l2=par[3])
        elif s == 2:
            group.apply_indexed(kt, T(seg, dev), T(bag_g, dev), T(bag_of.astype(np.int32), dev), "ftrl", par[0], par[1], l1=par[2], l2=par[3])
        else:
            for j in range(nt):
                a, b = int(seg[j]), int(seg[j + 1])
                pairs[j].apply_ftrl(kt[a:b], T(bag_g, dev), *par, grad_index=T(bag_of[a:b].astype(np.int32), dev))
        for j in range(nt):
            a, b = int(seg[j]), int(seg[j + 1])
            refs[j].apply(keys[a:b], pos_g[a:b], *par)
        if s == 1:
            assert pairs[0].demote(T(stored[0][:40], dev)) == 40
    for j in range(nt):
        assert pairs[j].hot.status() == pairs[j].cold.status() == 0 and pairs[j].hot.size() > 0 and pairs[j].cold.size() > 0
        assert_table_bits(pairs[j], refs[j], f"pair {j}")
        assert float(np.abs(export_sorted(pairs[j].cold)[2]).max()) > 0
    group.close()


# ---- GPU: the state travels -----------------------------------------------------------------------------------------------------------------------------
def stepped_table(dev, dim=24, **kw):
    """a table after two steps (all three planes hold something), its reference, and the inputs of a third step"""
    keys, rows, batch, grads = distinct_case(dim)
    t, ref = ftrl_table(dev, dim, keys, rows, **kw), ref_table(dim, keys, rows)
    for g in grads[:2]:
        t.apply_ftrl(T(batch, dev), T(g, dev), 0.05, 0.5, 0.02, 0.001)
        ref.apply(batch, g, 0.05, 0.5, 0.02, 0.001)
    return t, ref, batch, grads[2]


def third_step(t, ref, batch, g, dev):
    t.apply_ftrl(T(batch, dev), T(g, dev), 0.05, 0.5, 0.02, 0.001)
    if ref is not None:
        ref.apply(batch, g, 0.05, 0.5, 0.02, 0.001)


@pytest.mark.gpu
def test_export_import_reserve_and_move_keep_all_three_planes(dev):
    t, ref, batch, g = stepped_table(dev)
    assert_table_bits(t, ref, "before")
    e = t.export(with_state=True)
    assert len(e) == 4 and e[2] is not None and e[3] is not None and float(e[2].abs().max()) > 0 and float(e[3].min()) >= 0.1
    pieces = list(t.iter_export(1024))
    assert sum(p[0].numel() for p in pieces) == 600 and all(p[3] is not None for p in pieces)
    fresh = ftrl_table(dev, 24, capacity=2048)
    fresh.import_(*e)
    assert_table_bits(fresh, ref, "imported")
    t.reserve(2 * t.capacity)
    assert t.capacity >= 8192
    assert_table_bits(t, ref, "reserved")
    other = ftrl_table(dev, 24)
    kt = T(ref.keys, dev)
    n_moved, _ = t.move_to(other, kt)
    assert int(n_moved.item()) == 600 and t.size() == 0
    assert_table_bits(other, ref, "moved")
    other.move_to(t, kt)
    assert other.size() == 0
    assert_table_bits(t, ref, "moved back")
    third_step(t, ref, batch, g, dev)
    third_step(fresh, None, batch, g, dev)
    assert_table_bits(t, ref, "the step after reserve and two moves")
    assert_table_bits(fresh, ref, "the step after import")
    p2, f2 = t.find_plane(2, kt)
    assert bool(f2.all()) and np.array_equal(p2.cpu().numpy(), ref.n)


@pytest.mark.gpu
def test_evict_spill_hands_z_and_n_out(dev):
    t, ref, _, _ = stepped_table(dev, track_hits=True)
    k, v, s1, s2, hits = t.evict(0, limit=4096, spill=True)
    assert t.size() == 0 and k.numel() == 600 and s1 is not None and s2 is not None
    order = np.argsort(k.cpu().numpy())
    got = [k.cpu().numpy()[order], v.cpu().numpy()[order], s1.cpu().numpy()[order], s2.cpu().numpy()[order]]
    for name, x, y in zip(("keys", "rows", "z", "n"), got, ref.export_sorted()):
        assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y), name


@pytest.mark.gpu
def test_checkpoint_round_trip_and_load_into_another_kind(dev, tmp_path):
    import json

    from meepoembedding_amd import OPT_ADAM, LookupTable, checkpoint
    t, ref, batch, g = stepped_table(dev)
    path = str(tmp_path / "ckpt")
    assert t.save(path) == 600
    meta = json.load(open(os.path.join(path, "meta.json")))
    assert meta["optimizer"] == 3 and meta["planes"] == ["values", "state1", "state2"]
    back = ftrl_table(dev, 24, capacity=2048)
    assert back.load(path) == 600
    assert_table_bits(back, ref, "loaded")
    third_step(back, ref, batch, g, dev)
    assert_table_bits(back, ref, "the step after load")
    adam = LookupTable(2048, 24, device=dev, optimizer=OPT_ADAM, max_batch=4096)
    assert checkpoint.load_into(adam, path) == 600   # another kind: rows only, the state planes stay at their initial values
    e = export_sorted(adam)
    saved = export_sorted(t)
    assert np.array_equal(e[1].view(np.uint32), saved[1].view(np.uint32)) and not e[2].any() and not e[3].any()


# ---- GPU: refusals, nothing written ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_leave_the_tables_as_they_were(dev):
    from meepoembedding_amd import OPT_ADAGRAD, OPT_ADAM, LookupTable, MeepoError, TableGroup
    dim = 16
    keys = synth.keys_np(47, 0, 100)
    rows = (synth.rows_np(keys, dim, 2) * 0.05).astype(np.float32)
    kt, gt = T(keys, dev), T((synth.rows_np(keys, dim, 6) * 0.05).astype(np.float32), dev)
    tabs = {}
    for name, kind in (("adagrad", OPT_ADAGRAD), ("adam", OPT_ADAM)):
        tabs[name] = LookupTable(1024, dim, device=dev, optimizer=kind, max_batch=1024, initial_accumulator=0.1)
        tabs[name].insert(kt, T(rows, dev))
    tabs["ftrl"] = ftrl_table(dev, dim, keys, rows, capacity=1024, max_batch=1024)
    tabs["adagrad"].apply_adagrad(kt, gt, 0.05); tabs["adam"].apply_adam(kt, gt, 0.05); tabs["ftrl"].apply_ftrl(kt, gt, 0.05, l1=0.01)
    before = {name: export_sorted(t) for name, t in tabs.items()}

    def unchanged():
        for name, t in tabs.items():
            for x, y in zip(export_sorted(t), before[name]):
                assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y), name
            assert t.status() == 0

    for call in (lambda: tabs["adagrad"].apply_ftrl(kt, gt, 0.05), lambda: tabs["adam"].apply_ftrl(kt, gt, 0.05),
                 lambda: tabs["ftrl"].apply_adagrad(kt, gt, 0.05), lambda: tabs["ftrl"].apply_adam(kt, gt, 0.05)):
        with pytest.raises(MeepoError) as ei:
            call()
        assert ei.value.code == _lib.ERR_UNSUPPORTED
    slots = tabs["ftrl"].find_located(kt)[2]
    gi = torch.arange(100, dtype=torch.int32, device=dev)
    for bad in (dict(lr=0.0), dict(lr=-1.0), dict(lr=float("inf")), dict(lr=float("nan")), dict(lr=0.05, l1=-1.0), dict(lr=0.05, beta=float("nan")),
                dict(lr=0.05, l2=float("nan")), dict(lr=0.05, beta=-0.5), dict(lr=0.05, l2=-1e-3)):
        for form in ({}, {"slots": slots}, {"grad_index": gi}):
            with pytest.raises(MeepoError) as ei:
                tabs["ftrl"].apply_ftrl(kt, gt, **bad, **form)
            assert ei.value.code == _lib.ERR_INVALID_ARG, (bad, form)
    unchanged()
    with pytest.raises(MeepoError) as ei:   # a group of mixed kinds has no step at all
        TableGroup([tabs["ftrl"], tabs["adam"]], max_apply_batch=1024)
    assert ei.value.code == _lib.ERR_INVALID_ARG
    two = ftrl_table(dev, dim, keys, rows, capacity=1024, max_batch=1024)
    g = TableGroup([tabs["ftrl"], two], max_apply_batch=1024)
    both, seg = torch.cat([kt, kt]), torch.tensor([0, 100, 200], dtype=torch.int64, device=dev)
    gg = torch.cat([gt, gt])
    two_before = export_sorted(two)
    with pytest.raises(MeepoError) as ei:
        g.apply_adagrad(both, seg, gg, 0.05)
    assert ei.value.code == _lib.ERR_UNSUPPORTED
    for bad in (dict(lr=0.0), dict(lr=0.05, l1=-1.0), dict(lr=0.05, beta=float("nan"))):
        with pytest.raises(MeepoError) as ei:
            g.apply_ftrl(both, seg, gg, **bad)
        assert ei.value.code == _lib.ERR_INVALID_ARG
    with pytest.raises(MeepoError) as ei:
        g.apply_indexed(both, seg, gg, torch.arange(200, dtype=torch.int32, device=dev), "ftrl", 0.05, l1=-1.0)
    assert ei.value.code == _lib.ERR_INVALID_ARG
    unchanged()
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(export_sorted(two), two_before))
    g.close()
