"""bf16 output of the lookup family (SPEC.md §3 "Output type"): find, the located / training forward, find_or_insert, bags, groups, layers.

The reference of every case is NOT the code under test: it is the oracle's fp32 result (or a numpy-float32 restatement of the SPEC
accumulation) rounded by torch.Tensor.to(torch.bfloat16) on the CPU, compared on the raw 16-bit patterns; positions where the reference
is a NaN are compared with isnan.  CPU half: symbols, argument checks before any launch, fake kernels, the rounding rule itself."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import oracle
from meepoembedding_amd import _lib, synth
from meepoembedding_amd.nn import DynamicEmbedding, DynamicEmbeddingBag, DynamicEmbeddingCollection

BF16 = torch.bfloat16
NEW_SYMBOLS = ("mee_find_as", "mee_find_located_as", "mee_find_located_prepare_as", "mee_find_or_insert_as", "mee_find_or_insert_located_as",
               "mee_find_or_insert_located_prepare_as", "mee_find_pooled_as", "mee_find_grouped_as", "mee_group_find_or_insert_as",
               "mee_group_find_pooled_as")
RTOL, ATOL = 1e-6, 1e-9   # SPEC.md §4 (duplicate keys: the order of the fp64 sums is free)
# special values a row may hold: zeros, infinities, NaN, fp32 denormals (bf16 keeps denormals), the largest finite range, exact ties
SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-40, 2.0 ** -133, 2.0 ** -134, 1.5 * 2.0 ** -134, -1e-40, 3.3895e38, 3.4e38, -3.4e38,
                     1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 0.1, -7.3], dtype=np.float32)


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def to_bf16_ref(a) -> torch.Tensor:
    """the yardstick: torch's CPU cast of the fp32 reference"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(BF16)


def assert_bf16_equal(got: torch.Tensor, ref_f32, what=""):
    """got (bf16, any device) == bf16(ref_f32) bit for bit, NaN positions by isnan"""
    assert got.dtype == BF16, (what, got.dtype)
    ref = to_bf16_ref(ref_f32).reshape(-1)
    got = got.detach().cpu().contiguous().reshape(-1)
    assert got.numel() == ref.numel(), (what, got.shape, ref.shape)
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan), what
    gb, rb = got.view(torch.int16)[~nan], ref.view(torch.int16)[~nan]
    bad = int((gb != rb).sum())
    assert bad == 0, f"{what}: {bad} of {rb.numel()} bf16 patterns differ"


def formula_bits(u: np.ndarray) -> np.ndarray:
    """SPEC.md §3: bf16_bits(x) = (u + 0x7FFF + ((u >> 16) & 1)) >> 16 on the fp32 bit patterns u (not for NaNs)"""
    u = u.astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_new_symbols_declared_and_exported(built):
    from test_abi_load import _declared
    names = _declared()
    L = C.CDLL(_lib.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s in names and s in _lib.PROTOTYPES and hasattr(L, s), s
    assert _lib.lib().mee_abi_version() == 2     # additive: the ABI version stays
    assert (_lib.DTYPE_F32, _lib.DTYPE_BF16) == (0, 1)


def test_rounding_rule_is_torch_cpu_cast():
    """The integer formula of SPEC.md against torch.to(bfloat16) on the CPU: 4M random 32-bit patterns, every special value, every
    pattern around the ties and the overflow edge.  Independent of any kernel."""
    rng = np.random.default_rng(5)
    u = np.concatenate([rng.integers(0, 1 << 32, 1 << 22, dtype=np.uint64).astype(np.uint32), SPECIALS.view(np.uint32),
                        np.arange(0x3F7F0000, 0x3F830000, dtype=np.uint32),              # around 1.0: every tie and its neighbours
                        np.arange(0x7F7E0000, 0x7F800001, dtype=np.uint32),              # the largest finite values -> inf
                        np.arange(0x00000000, 0x00030000, dtype=np.uint32),              # denormals
                        np.arange(0x80000000, 0x80030000, dtype=np.uint32)])
    x = u.view(np.float32)
    got = torch.from_numpy(x.copy()).to(BF16).view(torch.int16).numpy().view(np.uint16)
    nan = np.isnan(x)
    assert np.array_equal(got[~nan], formula_bits(u[~nan]))
    back = torch.from_numpy(got[nan].view(np.int16).copy()).view(BF16)
    assert bool(torch.isnan(back).all())
    # the named cases
    one = lambda v: float(torch.tensor([v], dtype=torch.float32).to(BF16).float()[0])
    assert one(1 + 2.0 ** -8) == 1.0 and one(1 + 3 * 2.0 ** -8) == 1.015625 and one(3.4e38) == float("inf") and one(3.3895e38) < float("inf")
    assert one(1e-40) != 0.0 and one(2.0 ** -133) == 2.0 ** -133 and one(2.0 ** -134) == 0.0 and one(1.5 * 2.0 ** -134) == 2.0 ** -133


class Recorder:   # stands in for the library: records what would have been launched
    def __init__(self, calls):
        self.calls = calls

    def __getattr__(self, name):
        self.calls.append(name)
        return lambda *a: 0


def _cpu_stubs(monkeypatch):
    from meepoembedding_amd import LookupTable, TableGroup
    from meepoembedding_amd import table as tm
    calls = []
    monkeypatch.setattr(tm._lib, "lib", lambda: Recorder(calls))
    monkeypatch.setattr(tm, "_stream_ptr", lambda device: 0)
    t = LookupTable.__new__(LookupTable)
    t._h, t.device, t.dim = None, torch.device("cpu"), 8
    g = TableGroup.__new__(TableGroup)
    g._h, g.tables, g.device, g.dim = None, [t, t], torch.device("cpu"), 8
    return t, g, calls


def test_wrappers_reject_before_any_launch(built, monkeypatch):
    t, g, calls = _cpu_stubs(monkeypatch)
    keys = torch.arange(6, dtype=torch.int64)
    off, goff, seg = torch.tensor([0, 2, 6]), torch.tensor([0, 1, 3, 4, 6]), torch.tensor([0, 3, 6])
    f32, b16, f16 = torch.empty(6, 8), torch.empty(6, 8, dtype=BF16), torch.empty(6, 8, dtype=torch.float16)
    found = torch.empty(6, dtype=torch.uint8)
    lookups = [lambda **kw: t.find(keys, **kw), lambda **kw: t.find_located(keys, **kw), lambda **kw: t.find_located(keys, prepare_apply=True, **kw),
               lambda **kw: t.find_or_insert(keys, **kw), lambda **kw: t.find_or_insert_located(keys, **kw),
               lambda **kw: t.find_pooled(keys, off, **kw), lambda **kw: g.find(keys, seg, **kw), lambda **kw: g.find_or_insert(keys, seg, **kw),
               lambda **kw: g.find_pooled(keys, goff, **kw)]
    for f in lookups:
        with pytest.raises(ValueError):
            f(out_dtype=torch.float16)
        with pytest.raises(ValueError):
            f(out_dtype=torch.float64)
        with pytest.raises(ValueError):
            f(out=f32, out_dtype=BF16)          # an `out` of the wrong dtype, either way round
        with pytest.raises(ValueError):
            f(out=b16)
        with pytest.raises(ValueError):
            f(out=f16, out_dtype=torch.float16)
    # bf16 on the operators that have no bf16 form
    with pytest.raises(ValueError):
        t.find(keys, unordered=True, out_dtype=BF16)
    with pytest.raises(ValueError):
        t.find_or_insert(keys, min_count=2, out_dtype=BF16)
    with pytest.raises(ValueError):
        t.find_missing(keys, b16, found)
    with pytest.raises(ValueError):
        t.find_counted(keys, out=b16)
    with pytest.raises(ValueError):
        t.find_or_insert_missing(keys, b16, found)
    with pytest.raises(ValueError):
        t.find_many([(keys, b16, None)])
    for name in ("find_missing", "find_counted", "find_plane", "find_many", "find_or_insert_missing", "export"):
        import inspect
        assert "out_dtype" not in inspect.signature(getattr(type(t), name)).parameters, name
    assert calls == []
    # and what a good call launches
    t.find(keys, out_dtype=BF16); t.find(keys, flags=_lib.FIND_STREAM_STORES, out=b16, out_dtype=BF16)
    t.find_located(keys, out_dtype=BF16); t.find_located(keys, prepare_apply=True, out_dtype=BF16)
    t.find_or_insert(keys, out_dtype=BF16); t.find_or_insert_located(keys, out_dtype=BF16); t.find_or_insert_located(keys, prepare_apply=True, out_dtype=BF16)
    t.find_pooled(keys, off, "mean", out_dtype=BF16); t.find_pooled(keys, off, weights=torch.ones(6), out_dtype=BF16)
    g.find(keys, seg, out_dtype=BF16); g.find_or_insert(keys, seg, out_dtype=BF16); g.find_pooled(keys, goff, out_dtype=BF16)
    assert calls == ["mee_find_as", "mee_find_as", "mee_find_located_as", "mee_find_located_prepare_as", "mee_find_or_insert_as",
                     "mee_find_or_insert_located_as", "mee_find_or_insert_located_prepare_as", "mee_find_pooled_as", "mee_find_pooled_as",
                     "mee_find_grouped_as", "mee_group_find_or_insert_as", "mee_group_find_pooled_as"]
    calls.clear()
    t.find(keys); t.find(keys, out_dtype=torch.float32, out=f32); g.find(keys, seg)      # the defaults are the existing entry points
    assert calls == ["mee_find", "mee_find", "mee_find_grouped"]


def test_c_abi_null_arguments_are_errors_not_faults(built):
    """the typed entry points refuse null arguments like their fp32 twins (no GPU needed to get that far; the unknown-dtype and the
    alignment checks need a table and are exercised in test_find_bf16 / test_output_bounds_and_alignment)"""
    L = _lib.lib()
    assert L.mee_find_as(None, None, 0, None, 7, None, 0, None) == _lib.ERR_INVALID_ARG
    assert L.mee_find_located_as(None, None, 0, None, 1, None, None, None) == _lib.ERR_INVALID_ARG
    assert L.mee_find_pooled_as(None, None, 0, None, 0, None, None, 1, None, None, 0, None) == _lib.ERR_INVALID_ARG
    assert L.mee_find_grouped_as(None, None, None, 0, None, 1, None, None) == _lib.ERR_INVALID_ARG


def test_layers_report_bf16_to_the_tracer_and_refuse_tables_without_it(built):
    from _cpu_backend import CpuTable
    from meepoembedding_amd import LookupTable, TableGroup
    from meepoembedding_amd import nn as mnn
    from meepoembedding_amd.tiered import TieredLookupTable
    t = LookupTable.__new__(LookupTable)
    t._h, t.device, t.dim = None, torch.device("cpu"), 8
    g = TableGroup.__new__(TableGroup)
    g._h, g.tables, g.device, g.dim = None, [t, t], torch.device("cpu"), 8
    from torch.fx.experimental.proxy_tensor import make_fx
    keys, off, goff, w = torch.arange(6, dtype=torch.int64), torch.tensor([0, 2, 6]), torch.tensor([0, 1, 3, 4, 6]), torch.ones(6)

    def traced(fn, *args):
        """dtype and shape of fn's first output as the tracer sees it (fake kernels only: the stub tables are never called)"""
        gm = make_fx(fn, tracing_mode="fake")(*args)
        out = [n for n in gm.graph.nodes if n.op == "output"][0].args[0]
        val = (out[0] if isinstance(out, (tuple, list)) else out).meta["val"]
        return val.dtype, tuple(val.shape)

    for dt in (torch.float32, BF16):
        e, b, c, gb = DynamicEmbedding(t, out_dtype=dt), DynamicEmbeddingBag(t, out_dtype=dt), DynamicEmbeddingCollection(g, out_dtype=dt), DynamicEmbeddingBag(g, out_dtype=dt)
        assert traced(lambda k, a: mnn.lookup_located(k, a, e.table_id, True, True)[0], keys.view(2, 3), e._anchor) == (dt, (2, 3, 8))
        assert traced(lambda k, o, a: mnn.lookup_pooled(k, o, a, b.table_id, False)[0], keys, off, b._anchor) == (dt, (2, 8))
        assert traced(lambda k, o, a: mnn.lookup_pooled(k, o, a, gb.table_id, True)[0], keys, goff, gb._anchor) == (dt, (4, 8))
        assert traced(lambda k, o, ww, a: mnn.lookup_pooled_weighted(k, o, ww, a, b.table_id)[0], keys, off, w, b._anchor) == (dt, (2, 8))
        assert traced(lambda k, o, a: mnn.lookup_jagged(k, o, a, c.table_id, False), keys, off, c._anchor) == (dt, (6, 8))
    # tables without a bf16 lookup: refused at construction, fp32 accepted as before
    tiered = TieredLookupTable.__new__(TieredLookupTable)
    cpu = CpuTable(64, 8)
    for table in (tiered, cpu):
        for layer in (DynamicEmbedding, DynamicEmbeddingBag):
            layer(table)
            with pytest.raises(ValueError):
                layer(table, out_dtype=BF16)
    for layer, table in ((DynamicEmbedding, t), (DynamicEmbeddingBag, t), (DynamicEmbeddingCollection, g)):
        with pytest.raises(ValueError):
            layer(table, out_dtype=torch.float16)


# ---- GPU ----------------------------------------------------------------------------------------------------------------
def _pair(dev, dim, n_keys, seed, load=0.5, default_value=0.1, **kw):
    """a GPU table and its oracle twin with the same n_keys rows"""
    from meepoembedding_amd import LookupTable
    rng = np.random.default_rng(seed)
    cap = int(n_keys / load)
    t = LookupTable(cap, dim, device=dev, max_batch=1 << 15, default_value=default_value, **kw)
    o = oracle.OracleTable(cap, dim, optimizer=kw.get("optimizer", 0), default_value=default_value,
                           initial_accumulator=kw.get("initial_accumulator", 0.0), initializer=kw.get("initializer", 0),
                           init_scale=kw.get("init_scale", 0.0), init_seed=kw.get("init_seed", 0))
    u = synth.keys_np(seed, 0, n_keys)
    rows = rng.standard_normal((n_keys, dim)).astype(np.float32)
    for s in range(0, n_keys, 1 << 15):
        t.insert(T(u[s:s + (1 << 15)], dev), T(rows[s:s + (1 << 15)], dev))
    o.insert(u, rows)
    return t, o, u, rng


def _mixed_batch(rng, u, n, seed):
    """hits, misses, EMPTY and RECLAIMED"""
    keys = u[rng.integers(0, u.size, n)].copy()
    if n >= 7:
        keys[1::5] = synth.keys_np(seed + 999, 0, keys[1::5].size)   # absent
        keys[2] = oracle.EMPTY_KEY
        keys[n - 2] = oracle.RECLAIMED_KEY
    return keys


FLAG_SETS = [s | r | b for s in (0, _lib.FIND_STREAM_STORES, _lib.FIND_CACHED_STORES) for r in (0, _lib.FIND_STREAM_ROWS) for b in (0, _lib.FIND_STREAM_BUCKETS)]


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [4, 8, 16, 24, 40, 64, 128, 256, 1024])
def test_find_bf16(dev, dim):
    n_keys = 6000 if dim <= 256 else 1500
    t, o, u, rng = _pair(dev, dim, n_keys, 100 + dim, load=0.9, default_value=0.1)   # 0.1 is not a bf16 value
    assert to_bf16_ref([0.1]).float()[0] != np.float32(0.1)
    for n in (1, 3, 7, 8193):
        keys = _mixed_batch(rng, u, n, dim + n)
        eo, ef = o.find(keys)
        out, found = t.find(T(keys, dev), out_dtype=BF16)
        assert out.shape == (n, dim) and np.array_equal(found.cpu().numpy(), ef)
        assert_bf16_equal(out, eo, f"find dim {dim} n {n}")
        out32, _ = t.find(T(keys, dev))
        assert np.array_equal(out32.cpu().numpy(), eo)
    keys = _mixed_batch(rng, u, 4099, dim)
    eo, ef = o.find(keys)
    all_hit = u[rng.integers(0, u.size, 4096)]                       # the straight-line all-hit path of whole wave steps
    for flags in FLAG_SETS:
        out, found = t.find(T(keys, dev), flags=flags, out_dtype=BF16)
        assert np.array_equal(found.cpu().numpy(), ef)
        assert_bf16_equal(out, eo, f"find_as flags {flags}")
        out, _ = t.find(T(all_hit, dev), flags=flags, out_dtype=BF16, want_found=False)
        assert_bf16_equal(out, o.find(all_hit)[0], f"find_as all-hit flags {flags}")
        o32, f32 = t.find(T(keys, dev), flags=flags)                 # fp32 through mee_find_ex is unchanged
        assert np.array_equal(o32.cpu().numpy(), eo)
    # out_dtype = fp32 through the new entry point is the existing operator
    L, k = _lib.lib(), T(keys, dev)
    a, fa = torch.empty((keys.size, dim), device=dev), torch.empty(keys.size, dtype=torch.uint8, device=dev)
    for flags in (0, _lib.FIND_STREAM_STORES | _lib.FIND_STREAM_ROWS):
        a.fill_(-5.0)
        _lib.check(L.mee_find_as(t._h, k.data_ptr(), keys.size, a.data_ptr(), _lib.DTYPE_F32, fa.data_ptr(), flags, 0))
        torch.cuda.synchronize()
        assert np.array_equal(a.cpu().numpy(), eo) and np.array_equal(fa.cpu().numpy(), ef)
    assert L.mee_find_as(t._h, k.data_ptr(), keys.size, a.data_ptr(), 2, fa.data_ptr(), 0, 0) == _lib.ERR_INVALID_ARG   # unknown dtype
    assert t.status() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [8, 64, 128, 24])
def test_special_values_round_like_torch(dev, dim):
    """rows of zeros, infinities, NaN, denormals, overflow and exact ties, inserted then looked up: decides between the packed convert
    instruction and the integer formula"""
    from meepoembedding_amd import LookupTable
    n = 256
    rng = np.random.default_rng(3)
    rows = SPECIALS[rng.integers(0, SPECIALS.size, (n, dim))]
    rows[:SPECIALS.size, 0] = SPECIALS
    rows[0, :] = np.resize(SPECIALS, dim)
    u = synth.keys_np(77, 0, n)
    for default in (1e-40, float("nan"), 3.4e38):
        t = LookupTable(1024, dim, device=dev, default_value=default)
        t.insert(T(u, dev), T(rows, dev))
        keys = np.concatenate([u, synth.keys_np(78, 0, 9)])
        ref = np.concatenate([rows, np.full((9, dim), default, np.float32)])
        out, found = t.find(T(keys, dev), out_dtype=BF16)
        assert_bf16_equal(out, ref, f"specials dim {dim} default {default}")
        out, _, _ = t.find_located(T(keys, dev), out_dtype=BF16)
        assert_bf16_equal(out, ref, "specials located")
        off = np.arange(keys.size + 1, dtype=np.int64)              # bags of one key: the pooled store
        out, _ = t.find_pooled(T(keys, dev), T(off, dev), out_dtype=BF16)
        assert_bf16_equal(out, ref, "specials pooled")


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [4, 64, 24])
def test_output_bounds_and_alignment(dev, dim):
    t, o, u, rng = _pair(dev, dim, 2000, 31)
    n = 1001
    keys = _mixed_batch(rng, u, n, 5)
    eo, _ = o.find(keys)
    L, k = _lib.lib(), T(keys, dev)
    found = torch.empty(n, dtype=torch.uint8, device=dev)
    pad = 64
    for shift in (0, 4, 8, 12):                                     # element offsets: 8- but not 16-byte aligned for 4 and 12
        buf = torch.full((pad + n * dim + pad + 16,), -3.0, dtype=BF16, device=dev)
        view = buf[pad + shift: pad + shift + n * dim]
        assert view.data_ptr() % 8 == 0 and (view.data_ptr() % 16 == 0) == (shift % 8 == 0)
        t.find(k, out=view.view(n, dim), out_dtype=BF16)
        assert_bf16_equal(view, eo, f"aligned shift {shift}")
        rest = torch.cat([buf[:pad + shift], buf[pad + shift + n * dim:]]).float()
        assert bool((rest == -3.0).all()), "the lookup wrote outside its n * dim bf16"
    buf = torch.full((n * dim + 16,), -3.0, dtype=BF16, device=dev)
    for shift in (1, 2, 3):                                        # 2-, 4- and 6-byte aligned: refused, nothing written
        p = buf.data_ptr() + 2 * shift
        assert L.mee_find_as(t._h, k.data_ptr(), n, p, _lib.DTYPE_BF16, found.data_ptr(), 0, 0) == _lib.ERR_INVALID_ARG
        assert L.mee_find_located_as(t._h, k.data_ptr(), n, p, _lib.DTYPE_BF16, found.data_ptr(), found.data_ptr(), 0) == _lib.ERR_INVALID_ARG
        assert L.mee_find_or_insert_as(t._h, k.data_ptr(), n, p, _lib.DTYPE_BF16, found.data_ptr(), 0) == _lib.ERR_INVALID_ARG
        assert L.mee_find_pooled_as(t._h, k.data_ptr(), n, k.data_ptr(), 1, None, p, _lib.DTYPE_BF16, found.data_ptr(), None, 0, 0) == _lib.ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert bool((buf.float() == -3.0).all())


def _export_sorted(t):
    e = t.export(with_state=True)
    i = torch.argsort(e[0])
    return [x[i] if x is not None else None for x in e]


def _assert_tables(a, b, exact):
    ea, eb = _export_sorted(a), _export_sorted(b)
    assert torch.equal(ea[0], eb[0]) and a.status() == b.status()
    for x, y in zip(ea[1:], eb[1:]):
        if x is None:
            assert y is None
        elif exact:
            assert torch.equal(x, y)
        else:
            torch.testing.assert_close(x, y, rtol=RTOL, atol=ATOL)


@pytest.mark.gpu
@pytest.mark.parametrize("dim,opt", [(64, "adagrad"), (128, "adam"), (24, "adagrad"), (64, "adam")])
def test_located_forward_and_training_step(dev, dim, opt):
    """find_located / find_or_insert_located (+ prepare) with bf16 rows: rows, found and handles as the fp32 call's on a twin; after
    the same apply the twins' exports agree (bit for bit without duplicate keys, SPEC §4's contract on a Zipf batch)"""
    kind = oracle.OPT_ADAGRAD if opt == "adagrad" else oracle.OPT_ADAM
    kw = dict(optimizer=kind, initial_accumulator=0.1, initializer=1, init_scale=0.05, init_seed=9)
    a, o, u, rng = _pair(dev, dim, 5000, 7, **kw)        # the bf16-forward table
    b, _, _, _ = _pair(dev, dim, 5000, 7, **kw)          # its fp32-forward twin
    step = [0]

    def apply(t, keys, grads, slots):
        if opt == "adagrad":
            t.apply_adagrad(keys, grads, lr=0.05, slots=slots)
        else:
            t.apply_adam(keys, grads, lr=0.01, step=step[0], slots=slots)

    uniq = np.concatenate([u[rng.permutation(u.size)[:3000]], synth.keys_np(4711, 0, 77)])   # no duplicates; 77 absent keys
    uniq[5] = oracle.EMPTY_KEY
    zipf = u[np.minimum((rng.pareto(1.05, 4001)).astype(np.int64), u.size - 1)]
    new_keys = synth.keys_np(90210, 0, 501)
    for keys, exact in ((uniq, True), (zipf, False)):
        k = T(keys, dev)
        g = T((rng.standard_normal((keys.size, dim)) * 0.1).astype(np.float32), dev)
        eo, ef = o.find(keys)
        for prepare, located in itertools.product((False, True), (True, False)):
            step[0] += 1
            _, _, s32 = a.find_located(k)
            oa, fa, sa = a.find_located(k, prepare_apply=prepare, out_dtype=BF16)
            ob, fb, sb = b.find_located(k, prepare_apply=prepare)
            # handles: the fp32 call's on the same table (where a key sits inside its bucket is decided by the inserts' races, so the twin's
            # slot numbers may differ: there, the same positions have one)
            assert torch.equal(fa, fb) and torch.equal(sa, s32) and torch.equal(sa >= 0, sb >= 0)
            assert_bf16_equal(oa, ob.cpu().numpy(), f"find_located prepare={prepare}")
            if step[0] == 1:
                assert_bf16_equal(oa, eo, "find_located against the oracle"); assert np.array_equal(fa.cpu().numpy(), ef)
            if prepare and not located:                  # the probing apply cannot use the forward's partition of a located step: drop it
                a.apply_discard(); b.apply_discard()
            apply(a, k, g, sa if located else None)
            apply(b, k, g, sb if located else None)
            _assert_tables(a, b, exact)
    # a growing vocabulary: new keys are created in fp32 in both tables; only the returned copy is rounded
    for prepare in (False, True):
        keys = np.concatenate([new_keys[prepare * 250: prepare * 250 + 250], uniq[:300]])
        k = T(keys, dev)
        g = T((rng.standard_normal((keys.size, dim)) * 0.1).astype(np.float32), dev)
        step[0] += 1
        oa, fa, sa = a.find_or_insert_located(k, prepare_apply=prepare, out_dtype=BF16)
        ob, fb, sb = b.find_or_insert_located(k, prepare_apply=prepare)
        assert torch.equal(fa, fb) and torch.equal(sa >= 0, sb >= 0) and torch.equal(sa >= 0, k > oracle.RECLAIMED_KEY)   # every real key lives somewhere now
        assert_bf16_equal(oa, ob.cpu().numpy(), f"find_or_insert_located prepare={prepare}")
        _assert_tables(a, b, True)
        apply(a, k, g, sa); apply(b, k, g, sb)
        _assert_tables(a, b, True)
        assert torch.equal(sa, a.find_located(k)[2])     # the handles are where the keys live now
    keys = np.concatenate([synth.keys_np(5150, 0, 333), uniq[:100], [oracle.RECLAIMED_KEY]])
    oa, fa = a.find_or_insert(T(keys, dev), out_dtype=BF16)
    ob, fb = b.find_or_insert(T(keys, dev))
    assert torch.equal(fa, fb)
    assert_bf16_equal(oa, ob.cpu().numpy(), "find_or_insert")
    _assert_tables(a, b, True)
    assert a.status() == _lib.STATUS_RESERVED_KEY
    # fp32 through the typed entry points == the existing entry points
    L, k = _lib.lib(), T(uniq, dev)
    n = uniq.size
    for fn, twin in (("mee_find_located_as", a.find_located), ("mee_find_or_insert_located_as", a.find_or_insert_located)):
        ref = twin(k)
        if fn == "mee_find_or_insert_located_as":       # (its first call created the batch's absent keys: found = present before)
            ref = twin(k)
        out, fo, so = torch.empty((n, dim), device=dev), torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.int64, device=dev)
        _lib.check(getattr(L, fn)(a._h, k.data_ptr(), n, out.data_ptr(), _lib.DTYPE_F32, fo.data_ptr(), so.data_ptr(), 0))
        torch.cuda.synchronize()
        assert torch.equal(out, ref[0]) and torch.equal(fo, ref[1]) and torch.equal(so, ref[2]), fn
    for fn, ref in (("mee_find_located_prepare_as", None), ("mee_find_or_insert_located_prepare_as", None)):
        out, fo, so = torch.empty((n, dim), device=dev), torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.int64, device=dev)
        _lib.check(getattr(L, fn)(a._h, k.data_ptr(), n, out.data_ptr(), _lib.DTYPE_F32, fo.data_ptr(), so.data_ptr(), 0))
        a.apply_discard()
        ref = a.find_located(k)
        assert torch.equal(out, ref[0]) and torch.equal(fo, ref[1]) and torch.equal(so, ref[2]), fn
    out = torch.empty((n, dim), device=dev)
    _lib.check(L.mee_find_or_insert_as(a._h, k.data_ptr(), n, out.data_ptr(), _lib.DTYPE_F32, None, 0))
    torch.cuda.synchronize()
    assert torch.equal(out, a.find(k)[0])


def spec_pool(rows, off, mode="sum", w=None):
    """SPEC.md §3 in numpy float32: position order, the first (weighted) row is the initial sum, every product and sum rounded, mean =
    one division by the length; an empty bag is zeros"""
    off = np.asarray(off, np.int64)
    lens = off[1:] - off[:-1]
    out = np.zeros((lens.size, rows.shape[1]), np.float32)
    with np.errstate(all="ignore"):
        for s in range(int(lens.max()) if lens.size else 0):
            m = lens > s
            p = off[:-1][m] + s
            r = rows[p] if w is None else (w[p][:, None] * rows[p]).astype(np.float32)
            out[m] = r if s == 0 else (out[m] + r).astype(np.float32)
        if mode == "mean":
            nz = lens > 0
            out[nz] = (out[nz] / lens[nz, None].astype(np.float32)).astype(np.float32)
    return out


BAG_SHAPES = (np.array([0, 1, 15, 16, 17, 40, 200, 0, 3, 1, 2, 5] + [2, 0, 7, 1] * 20),      # short average: four bags per wave (tile per bag, long bags shared)
              np.array([0, 1, 15, 16, 17, 40, 200, 33, 64, 12, 90, 31]))                     # long average: a wave per bag
assert BAG_SHAPES[0].sum() // BAG_SHAPES[0].size < 12 <= BAG_SHAPES[1].sum() // BAG_SHAPES[1].size


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [24, 40, 64, 128])
def test_find_pooled_bf16(dev, dim):
    t, o, u, rng = _pair(dev, dim, 4000, 200 + dim)
    for lens in BAG_SHAPES:
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        keys = _mixed_batch(rng, u, int(off[-1]), dim)                       # absent and reserved keys inside bags
        rows, ef = o.find(keys)
        w = rng.standard_normal(keys.size).astype(np.float32)
        k, f = T(keys, dev), T(off, dev)
        for mode in ("sum", "mean"):
            out, found = t.find_pooled(k, f, mode, out_dtype=BF16)
            assert np.array_equal(found.cpu().numpy(), ef)
            assert_bf16_equal(out, spec_pool(rows, off, mode), f"pooled {mode} dim {dim}")
            assert np.array_equal(t.find_pooled(k, f, mode)[0].cpu().numpy(), oracle.pool_rows(rows, off, mode))
        loc = torch.empty(keys.size, dtype=torch.int64, device=dev)
        out, found = t.find_pooled(k, f, weights=T(w, dev), located=loc, out_dtype=BF16)
        assert_bf16_equal(out, spec_pool(rows, off, "sum", w), f"weighted dim {dim}")
        assert torch.equal(loc, t.find_located(k)[2]) and np.array_equal(found.cpu().numpy(), ef)
        # fp32 through the typed entry point == the existing operators
        L = _lib.lib()
        for weights, mode in ((None, 0), (None, 1), (T(w, dev), 0)):
            a = torch.empty((lens.size, dim), device=dev)
            _lib.check(L.mee_find_pooled_as(t._h, k.data_ptr(), keys.size, f.data_ptr(), lens.size, weights.data_ptr() if weights is not None else None,
                                            a.data_ptr(), _lib.DTYPE_F32, None, None, mode, 0))
            torch.cuda.synchronize()
            ref = t.find_pooled(k, f, "mean" if mode else "sum", weights=weights)[0]
            assert torch.equal(a, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [24, 64, 128])
def test_bag_is_rounded_once(dev, dim):
    """1.0 followed by sixteen rows of 2^-9: the fp32 sum is 1.03125; a running sum kept in bf16 would stay at 1.0"""
    from meepoembedding_amd import LookupTable
    t = LookupTable(256, dim, device=dev)
    u = synth.keys_np(3, 0, 17)
    rows = np.full((17, dim), 2.0 ** -9, np.float32)
    rows[0] = 1.0
    t.insert(T(u, dev), T(rows, dev))
    for reps in (1, 40):                                            # one bag (four bags per wave), many bags of 17 (a wave per bag)
        keys = np.tile(u, reps)
        off = np.arange(0, keys.size + 1, 17, dtype=np.int64)
        out, _ = t.find_pooled(T(keys, dev), T(off, dev), out_dtype=BF16)
        assert bool((out.float() == 1.03125).all())
        assert_bf16_equal(out, spec_pool(rows[np.tile(np.arange(17), reps)], off))
        out, _ = t.find_pooled(T(keys, dev), T(off, dev), weights=torch.ones(keys.size, device=dev), out_dtype=BF16)
        assert bool((out.float() == 1.03125).all())
        out, _ = t.find_pooled(T(keys, dev), T(off, dev), "mean", out_dtype=BF16)
        assert_bf16_equal(out, spec_pool(rows[np.tile(np.arange(17), reps)], off, "mean"))


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [64, 128, 40])
def test_table_group_bf16(dev, dim):
    from meepoembedding_amd import TableGroup
    kw = dict(optimizer=oracle.OPT_ADAGRAD, initial_accumulator=0.1, initializer=1, init_scale=0.05)
    members = [_pair(dev, dim, n, 300 + j, init_seed=j, **kw) for j, n in enumerate((3000, 50, 700))]    # three sizes
    twins = [_pair(dev, dim, n, 300 + j, init_seed=j, **kw) for j, n in enumerate((3000, 50, 700))]
    ga, gb = TableGroup([m[0] for m in members], max_apply_batch=1 << 14), TableGroup([m[0] for m in twins], max_apply_batch=1 << 14)
    rng = members[0][3]
    for seg_lens in ((1500, 0, 333), (0, 77, 1), (5, 5, 0)):        # one empty segment each
        segs = [_mixed_batch(rng, m[2], n, 17) if n else np.empty(0, np.int64) for m, n in zip(members, seg_lens)]
        keys = np.concatenate(segs)
        off = np.concatenate([[0], np.cumsum(seg_lens)]).astype(np.int64)
        ref = np.concatenate([m[1].find(s)[0] for m, s in zip(members, segs)])
        ef = np.concatenate([m[1].find(s)[1] for m, s in zip(members, segs)])
        out, found = ga.find(T(keys, dev), T(off, dev), out_dtype=BF16)
        assert np.array_equal(found.cpu().numpy(), ef)
        assert_bf16_equal(out, ref, f"group find {seg_lens}")
        L, k, f = _lib.lib(), T(keys, dev), T(off, dev)
        a = torch.empty((keys.size, dim), device=dev)
        _lib.check(L.mee_find_grouped_as(ga._h, k.data_ptr(), f.data_ptr(), keys.size, a.data_ptr(), _lib.DTYPE_F32, None, 0))
        torch.cuda.synchronize()
        assert np.array_equal(a.cpu().numpy(), ref)
    # pooled: bags_per_table bags per member
    bpt = 6
    lens = np.array([0, 1, 16, 3, 40, 2] + [0] * 6 + [5, 0, 17, 1, 1, 2])                    # the second member's bags are all empty
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    keys = np.concatenate([_mixed_batch(rng, m[2], int(lens[j * bpt:(j + 1) * bpt].sum()), 3) if lens[j * bpt:(j + 1) * bpt].sum() else np.empty(0, np.int64)
                           for j, m in enumerate(members)])
    rows = np.concatenate([m[1].find(keys[off[j * bpt]:off[(j + 1) * bpt]])[0] for j, m in enumerate(members)])
    w = rng.standard_normal(keys.size).astype(np.float32)
    for mode in ("sum", "mean"):
        loc_a, loc_b = torch.empty(keys.size, dtype=torch.int64, device=dev), torch.empty(keys.size, dtype=torch.int64, device=dev)
        out, _ = ga.find_pooled(T(keys, dev), T(off, dev), mode, located=loc_a, out_dtype=BF16)
        ref32, _ = ga.find_pooled(T(keys, dev), T(off, dev), mode, located=loc_b)
        assert_bf16_equal(out, spec_pool(rows, off, mode), f"group pooled {mode}")
        assert torch.equal(loc_a, loc_b) and np.array_equal(ref32.cpu().numpy(), spec_pool(rows, off, mode))
    out, _ = ga.find_pooled(T(keys, dev), T(off, dev), weights=T(w, dev), out_dtype=BF16)
    assert_bf16_equal(out, spec_pool(rows, off, "sum", w), "group weighted")
    L, k, f = _lib.lib(), T(keys, dev), T(off, dev)
    a = torch.empty((lens.size, dim), device=dev)
    _lib.check(L.mee_group_find_pooled_as(ga._h, k.data_ptr(), keys.size, f.data_ptr(), bpt, None, a.data_ptr(), _lib.DTYPE_F32, None, None, 1, 0))
    torch.cuda.synchronize()
    assert torch.equal(a, ga.find_pooled(k, f, "mean")[0])
    # find_or_insert: new keys enter both groups in fp32; the returned copy is rounded
    seg_lens = (400, 0, 90)
    segs = [np.concatenate([synth.keys_np(8000 + j, 0, n // 2), m[2][:n - n // 2]]) if n else np.empty(0, np.int64) for j, (m, n) in enumerate(zip(members, seg_lens))]
    keys, off = np.concatenate(segs), np.concatenate([[0], np.cumsum(seg_lens)]).astype(np.int64)
    oa, fa = ga.find_or_insert(T(keys, dev), T(off, dev), out_dtype=BF16)
    ob, fb = gb.find_or_insert(T(keys, dev), T(off, dev))
    assert torch.equal(fa, fb)
    assert_bf16_equal(oa, ob.cpu().numpy(), "group find_or_insert")
    ref = np.concatenate([m[1].find_or_insert(s)[0] for m, s in zip(members, segs) if s.size])
    assert_bf16_equal(oa, ref, "group find_or_insert against the oracle")
    for m, tw in zip(members, twins):
        _assert_tables(m[0], tw[0], True)
    a = torch.empty((keys.size, dim), device=dev)
    _lib.check(L.mee_group_find_or_insert_as(ga._h, T(keys, dev).data_ptr(), T(off, dev).data_ptr(), keys.size, a.data_ptr(), _lib.DTYPE_F32, None, 0))
    torch.cuda.synchronize()
    assert torch.equal(a, ob)


def _layer_tables(dev, dim, opt, n=3):
    kind = oracle.OPT_ADAGRAD if opt == "adagrad" else oracle.OPT_ADAM
    kw = dict(optimizer=kind, initial_accumulator=0.1, initializer=1, init_scale=0.05, init_seed=4)
    return [_pair(dev, dim, 2000, 500, **kw) for _ in range(n)]


@pytest.mark.gpu
@pytest.mark.parametrize("opt", ["adagrad", "adam"])
def test_layers_bf16_forward_and_step(dev, opt):
    """a bf16 layer == the fp32 layer followed by .to(bfloat16) in the model: same output bits, and after one step with the same bf16
    upstream grad on a duplicate-free batch the same table, bit for bit"""
    from meepoembedding_amd import TableGroup
    dim = 64
    (ta, o, u, rng), (tb, _, _, _) = _layer_tables(dev, dim, opt, 2)
    keys = T(np.concatenate([u[rng.permutation(u.size)[:900]], synth.keys_np(31337, 0, 100)]).reshape(20, 50), dev)   # 100 new ids
    G = torch.randn(20, 50, dim, device=dev).to(BF16)
    la, lb = DynamicEmbedding(ta, optimizer=opt, lr=0.05, out_dtype=BF16).to(dev), DynamicEmbedding(tb, optimizer=opt, lr=0.05).to(dev)
    ya, yb = la(keys), lb(keys).to(BF16)
    assert ya.dtype == BF16 and ya.shape == (20, 50, dim) and torch.equal(ya.view(torch.int16), yb.view(torch.int16))
    (ya * G).sum().backward(); (yb * G).sum().backward()
    _assert_tables(ta, tb, True)
    la.eval(); lb.eval()
    assert torch.equal(la(keys).view(torch.int16), lb(keys).to(BF16).view(torch.int16))
    # bags: sum, mean, weighted (with the grad of the weights)
    lens = np.array([3, 0, 17, 1, 40, 2, 16, 5])
    off = T(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), dev)
    bk = T(u[rng.permutation(u.size)[:int(lens.sum())]], dev)
    Gb = torch.randn(lens.size, dim, device=dev).to(BF16)
    for mode in ("sum", "mean"):
        ba, bb = DynamicEmbeddingBag(ta, mode=mode, optimizer=opt, lr=0.05, out_dtype=BF16).to(dev), DynamicEmbeddingBag(tb, mode=mode, optimizer=opt, lr=0.05).to(dev)
        ya, yb = ba(bk, off), bb(bk, off).to(BF16)
        assert ya.dtype == BF16 and torch.equal(ya.view(torch.int16), yb.view(torch.int16))
        (ya * Gb).sum().backward(); (yb * Gb).sum().backward()
        _assert_tables(ta, tb, True)
    wa = torch.randn(int(lens.sum()), device=dev, requires_grad=True)
    wb = wa.detach().clone().requires_grad_(True)
    ba, bb = DynamicEmbeddingBag(ta, optimizer=opt, lr=0.05, out_dtype=BF16).to(dev), DynamicEmbeddingBag(tb, optimizer=opt, lr=0.05).to(dev)
    ya, yb = ba(bk, off, wa), bb(bk, off, wb).to(BF16)
    assert ya.dtype == BF16 and torch.equal(ya.view(torch.int16), yb.view(torch.int16))
    (ya * Gb).sum().backward(); (yb * Gb).sum().backward()
    assert torch.equal(wa.grad, wb.grad)
    _assert_tables(ta, tb, True)
    # the collection (one grouped lookup, one grouped step) and the bag collection
    A, B = _layer_tables(dev, dim, opt, 3), _layer_tables(dev, dim, opt, 3)
    ga, gb = TableGroup([m[0] for m in A], max_apply_batch=1 << 14), TableGroup([m[0] for m in B], max_apply_batch=1 << 14)
    seg = (300, 0, 120)
    ck = T(np.concatenate([np.concatenate([m[2][rng.permutation(2000)[:n - 10]], synth.keys_np(600 + j, 0, 10)]) if n else np.empty(0, np.int64)
                           for j, (m, n) in enumerate(zip(A, seg))]), dev)
    coff = T(np.concatenate([[0], np.cumsum(seg)]).astype(np.int64), dev)
    Gc = torch.randn(sum(seg), dim, device=dev).to(BF16)
    ca, cb = DynamicEmbeddingCollection(ga, optimizer=opt, lr=0.05, out_dtype=BF16).to(dev), DynamicEmbeddingCollection(gb, optimizer=opt, lr=0.05).to(dev)
    ya, yb = ca(ck, coff), cb(ck, coff).to(BF16)
    assert ya.dtype == BF16 and torch.equal(ya.view(torch.int16), yb.view(torch.int16))
    (ya * Gc).sum().backward(); (yb * Gc).sum().backward()
    for m, tw in zip(A, B):
        _assert_tables(m[0], tw[0], True)
    blens = np.array([3, 0, 17, 1] + [0, 0, 0, 0] + [40, 2, 16, 5])
    boff = T(np.concatenate([[0], np.cumsum(blens)]).astype(np.int64), dev)
    bkeys = T(np.concatenate([m[2][rng.permutation(2000)[:int(blens[4 * j:4 * j + 4].sum())]] for j, m in enumerate(A)]), dev)
    Gg = torch.randn(blens.size, dim, device=dev).to(BF16)
    for mode in ("sum", "mean"):
        ba, bb = DynamicEmbeddingBag(ga, mode=mode, optimizer=opt, lr=0.05, out_dtype=BF16).to(dev), DynamicEmbeddingBag(gb, mode=mode, optimizer=opt, lr=0.05).to(dev)
        ya, yb = ba(bkeys, boff), bb(bkeys, boff).to(BF16)
        assert ya.dtype == BF16 and torch.equal(ya.view(torch.int16), yb.view(torch.int16))
        (ya * Gg).sum().backward(); (yb * Gg).sum().backward()
        for m, tw in zip(A, B):
            _assert_tables(m[0], tw[0], True)


@pytest.mark.gpu
def test_bf16_training_forward_under_graph_capture(dev):
    """the bf16 training forward with the fused partition plus its apply, captured and replayed twice, equals the eager twin"""
    from meepoembedding_amd import OPT_ADAGRAD, LookupTable
    n_keys, batch, dim = 200_000, 1 << 15, 64
    tables = []
    for _ in range(2):
        t = LookupTable(int(n_keys / 0.75), dim, device=dev, optimizer=OPT_ADAGRAD, max_batch=1 << 16, initial_accumulator=0.1)
        k = synth.keys_t(21, 0, n_keys, dev)
        for s in range(0, n_keys, 1 << 16):
            t.insert(k[s:s + (1 << 16)], synth.rows_t(k[s:s + (1 << 16)], dim, 2))
        tables.append(t)
    eager, graphed = tables
    rng = np.random.default_rng(2)
    all_keys = synth.keys_t(21, 0, n_keys, dev)
    batches = [all_keys[torch.from_numpy(rng.integers(0, n_keys, batch)).to(dev)] for _ in range(4)]
    g = torch.randn(batch, dim, device=dev) * 0.01
    kb = torch.empty(batch, dtype=torch.int64, device=dev)
    bufs = lambda: (torch.empty((batch, dim), dtype=BF16, device=dev), torch.empty(batch, dtype=torch.uint8, device=dev), torch.empty(batch, dtype=torch.int64, device=dev))
    (oe, fe, se), (og, fg, sg) = bufs(), bufs()

    def step(t, keys, o, f, s):
        t.find_located(keys, out=o, found=f, slots=s, prepare_apply=True, out_dtype=BF16)
        t.apply_adagrad(keys, g, lr=0.01, slots=s)

    for b in batches[:2]:
        kb.copy_(b)
        step(eager, b, oe, fe, se); step(graphed, kb, og, fg, sg)
        torch.cuda.synchronize()
    kb.copy_(batches[1])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(graphed, kb, og, fg, sg)
    for b in batches[2:]:
        step(eager, b, oe, fe, se)
        kb.copy_(b)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(fe, fg) and torch.equal(se >= 0, sg >= 0) and torch.equal(oe.view(torch.int16), og.view(torch.int16))   # (twins: slot numbers may differ)
    _assert_tables(eager, graphed, False)
