"""bf16 row storage (SPEC.md §3 "Row storage type"): LookupTable(value_dtype=torch.bfloat16), the C-ABI's MEE_FLAG_BF16_ROWS.

By definition a bf16-row table is indistinguishable from an fp32 table that was handed bf16(values) and created with bf16(default_value).
So every GPU case here is a BIT-FOR-BIT comparison against such a twin: an fp32 LookupTable on the same device, fed
rows.to(torch.bfloat16).float() computed on the CPU (the cast tests/test_bf16_out.py pins to the spec's integer rule).  No tolerance
anywhere; positions where the reference is a NaN are compared with isnan.  CPU half: the flag, the symbols, the constructor's argument
checks before any device is needed, the wrappers' refusal of a bf16-row table."""
import ctypes as C
import json
import os
import types

import numpy as np
import pytest
import torch

from meepoembedding_amd import _lib, synth
from meepoembedding_amd._lib import MeepoError

BF16 = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mee_insert_as", "mee_assign_as", "mee_table_value_dtype")
SENT_F32, SENT_BF16, SENT_U8 = -777.25, -768.0, 0xAB   # guard values behind every result buffer (both exact in their type)


def rnd(x: torch.Tensor) -> torch.Tensor:
    """what a bf16-row table stores for fp32 rows x, as fp32: torch's CPU cast, the spec's rule"""
    return x.detach().cpu().to(torch.float32).to(BF16).to(torch.float32)


def bits32(x):
    return x.detach().cpu().contiguous().view(torch.int32)


def bits16(x):
    return x.detach().cpu().contiguous().view(torch.int16)


def assert_same_f32(got, ref, what=""):
    """two fp32 tensors, bit for bit; NaN positions: both NaN"""
    got, ref = got.detach().cpu(), ref.detach().cpu()
    assert got.dtype == ref.dtype == torch.float32 and got.shape == ref.shape, (what, got.dtype, got.shape, ref.shape)
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan), what
    bad = int((bits32(got)[~nan] != bits32(ref)[~nan]).sum())
    assert bad == 0, f"{what}: {bad} of {got.numel()} fp32 patterns differ"


def assert_same_bf16(got, ref_f32, what=""):
    """a bf16 tensor against bf16(ref_f32) (CPU cast), bit for bit; NaN positions: both NaN"""
    got, ref = got.detach().cpu(), ref_f32.detach().cpu().to(BF16)
    assert got.dtype == BF16 and got.shape == ref.shape, (what, got.dtype, got.shape, ref.shape)
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan), what
    bad = int((bits16(got)[~nan] != bits16(ref)[~nan]).sum())
    assert bad == 0, f"{what}: {bad} of {got.numel()} bf16 patterns differ"


def K(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def rows_for(keys_np, dim, seed):
    """rows with full fp32 mantissas (the rounding has something to do), a function of the key"""
    return torch.from_numpy(synth.rows_np(keys_np, dim, seed).astype(np.float32) * np.float32(1.37))


def pair(dev, capacity, dim, default_value=0.0, max_batch=4096):
    """(bf16-row table, its fp32 twin)"""
    from meepoembedding_amd import LookupTable
    t = LookupTable(capacity, dim, device=dev, max_batch=max_batch, default_value=default_value, value_dtype=BF16)
    tw = LookupTable(capacity, dim, device=dev, max_batch=max_batch, default_value=float(rnd(torch.tensor(default_value))))
    assert t.capacity == tw.capacity
    return t, tw


def insert_both(t, tw, keys_np, rows, dev):
    for s in range(0, len(keys_np), t.max_batch):
        k = K(keys_np[s:s + t.max_batch], dev)
        t.insert(k, rows[s:s + t.max_batch].to(dev))
        tw.insert(k, rnd(rows[s:s + t.max_batch]).to(dev))


def guarded(n, dim, dtype, dev):
    """a result buffer of n rows with two guard rows of a sentinel behind it -> (whole buffer, the n-row view handed to the lookup)"""
    buf = torch.full((n + 2, dim), SENT_BF16 if dtype == BF16 else SENT_F32, dtype=dtype, device=dev)
    return buf, buf[:n]


def guards_intact(buf, n):
    sent = SENT_BF16 if buf.dtype == BF16 else SENT_F32
    return bool((buf[n:].float() == sent).all())


def sorted_export(t):
    k, v = t.export()
    o = torch.argsort(k)
    return k[o].cpu(), v[o].cpu()


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_flag_and_symbols(built):
    """fails on the parent commit: neither the flag nor the entry points exist there"""
    assert _lib.FLAG_BF16_ROWS == 4
    with open(os.path.join(ROOT, "include", "meepo_embedding.h")) as f:
        header = f.read()
    assert "MEE_FLAG_BF16_ROWS = 4u" in header
    L = C.CDLL(_lib.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s in _lib.PROTOTYPES and hasattr(L, s) and s + "(" in header, s
    assert _lib.lib().mee_abi_version() == 2 and C.sizeof(_lib.Config) == 64 and C.sizeof(_lib.TableInfo) == 48   # additive: nothing pinned moved


def test_constructor_checks_come_before_the_device(built):
    """every ValueError of LookupTable(value_dtype=...) fires before a device (or the library) is needed: device='cpu' would be a MeepoError"""
    from meepoembedding_amd import OPT_ADAGRAD, OPT_ADAM, LookupTable
    bad = [dict(optimizer=OPT_ADAGRAD), dict(optimizer=OPT_ADAM), dict(track_hits=True), dict(admission=True), dict(value_memory=_lib.MEM_HOST_PINNED)]
    for kw in bad:
        with pytest.raises(ValueError, match="bfloat16"):
            LookupTable(1024, 64, device="cpu", value_dtype=BF16, **kw)
    for dim in (4, 12, 36, 1020):
        with pytest.raises(ValueError, match="multiple of 8"):
            LookupTable(1024, dim, device="cpu", value_dtype=BF16)
    for dt in (torch.float16, torch.float64, torch.int8, None):
        with pytest.raises(ValueError, match="value_dtype"):
            LookupTable(1024, 64, device="cpu", value_dtype=dt)
    with pytest.raises(MeepoError):   # the arguments are fine: now it is the device that is missing
        LookupTable(1024, 64, device="cpu", value_dtype=BF16)


def test_wrappers_refuse_a_bf16_row_table():
    """groups, tiers, shards, peers and layers refuse a table with value_dtype == bfloat16 at construction, before they touch it"""
    from meepoembedding_amd import MixedTableGroup, TableGroup
    from meepoembedding_amd.nn import DynamicEmbedding, DynamicEmbeddingBag, DynamicEmbeddingCollection
    from meepoembedding_amd.p2p import PeerShardedFind
    from meepoembedding_amd.sharded import RcclShardedTable, ShardedLookupTable, ShardedTableGroup
    from meepoembedding_amd.tiered import TieredLookupTable
    b = types.SimpleNamespace(value_dtype=BF16, dim=64)        # anything else it lacks: nobody may get that far
    f = types.SimpleNamespace(value_dtype=torch.float32, dim=64)
    grp = types.SimpleNamespace(tables=[f, b], dim=64)
    makers = [lambda: TableGroup([f, b]), lambda: MixedTableGroup([b]), lambda: TieredLookupTable(b, f), lambda: TieredLookupTable(f, b),
              lambda: ShardedLookupTable(b, None), lambda: ShardedTableGroup(grp, None), lambda: RcclShardedTable(b, 16),
              lambda: RcclShardedTable(f, 16, cold=b), lambda: PeerShardedFind(b, None, 16), lambda: DynamicEmbedding(b),
              lambda: DynamicEmbeddingBag(b), lambda: DynamicEmbeddingBag(grp), lambda: DynamicEmbeddingCollection(grp)]
    for mk in makers:
        with pytest.raises(MeepoError, match="bf16-row table") as e:
            mk()
        assert e.value.code == _lib.ERR_UNSUPPORTED


# ---- GPU ----------------------------------------------------------------------------------------------------------------
# 1. rounding on write
SPECIAL_BITS = np.array([0x3F808000, 0x3F818000,              # ties: to even downwards, to even upwards
                         0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001,   # just below / above them
                         0xBF808000, 0xBF818000,
                         0x00000000, 0x80000000,              # +-0
                         0x00000001, 0x00007FFF, 0x00008000, 0x00008001, 0x007FFFFF, 0x807FFFFF,   # fp32 denormals (some round to bf16 denormals, some to 0)
                         0x00010000, 0x007F0000, 0x80010000,  # bf16 denormals: kept
                         0x7F7FFFFF, 0xFF7FFFFF,              # the largest finite fp32 -> inf
                         0x7F7F0000, 0x7F7F7FFF, 0x7F7F8000, 0xFF7F8000,   # the largest bf16, just below half an ulp more, exactly half an ulp more (-> inf)
                         0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001, 0xFFC12345,   # +-inf, NaNs
                         0x3DCCCCCD, 0xC0E9999A], dtype=np.uint32)


@pytest.mark.gpu
def test_rounding_on_write(dev):
    dim = 8
    vals = SPECIAL_BITS.view(np.float32)
    n = (len(vals) + dim - 1) // dim
    rows = torch.from_numpy(np.resize(vals, n * dim).reshape(n, dim).copy())
    keys = synth.keys_np(3, 0, n)
    from meepoembedding_amd import LookupTable
    t = LookupTable(256, dim, device=dev, max_batch=64, value_dtype=BF16)
    t.insert(K(keys, dev), rows.to(dev))
    out32, found = t.find(K(keys, dev))
    out16, _ = t.find(K(keys, dev), out_dtype=BF16)
    assert bool(found.all()) and t.status() == 0
    assert_same_f32(out32, rnd(rows), "fp32 out")
    assert_same_bf16(out16, rows, "bf16 out")
    a = torch.zeros_like(rows)      # the same through assign
    t.insert(K(keys, dev), a.to(dev))
    assert bool(t.assign(K(keys, dev), rows.to(dev)).all())
    assert_same_bf16(t.find(K(keys, dev), out_dtype=BF16)[0], rows, "assign, bf16 out")


# 2. lookup parity with the twin
_FIND_FLAGS = [f for f in range(16) if (f & 3) != 3]   # every mee_find_ex combination (stream and cached stores exclude each other)


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [8, 64, 128, 200, 1024])
def test_find_parity_with_twin(dev, dim):
    t, tw = pair(dev, 2100, dim, default_value=0.3)          # 0.3 is no bf16 value: the default row is the rounded one
    n_keys = int(0.92 * t.capacity)
    allk = synth.keys_np(11, 0, 2 * n_keys)
    stored = allk[:n_keys]
    insert_both(t, tw, stored, rows_for(stored, dim, 5), dev)
    assert t.size() == tw.size() == n_keys and t.status() == tw.status() == 0
    assert n_keys / t.capacity >= 0.9 and t.probe_length(K(stored, dev)) > 1.05   # probes go beyond the home bucket
    rng = np.random.default_rng(dim)
    for n in (1, 7, 1003):
        batch = np.where(rng.random(n) < 0.67, rng.choice(stored, n), rng.choice(allk[n_keys:], n))
        if n >= 7:
            batch[2], batch[n - 2] = _lib.EMPTY_KEY, _lib.RECLAIMED_KEY
        k = K(batch, dev)
        ref, ref_found = tw.find(k)
        for out_dtype, flag_list in ((torch.float32, [None] + (_FIND_FLAGS if dim == 64 else [])), (BF16, [None] + (_FIND_FLAGS if dim == 64 else []))):
            for flags in flag_list:
                buf, out = guarded(n, dim, out_dtype, dev)
                fbuf = torch.full((n + 3,), SENT_U8, dtype=torch.uint8, device=dev)
                found = fbuf[1:1 + n]        # one byte off any alignment: the unaligned found path
                t.find(k, out=out, found=found, flags=flags, out_dtype=out_dtype)
                what = f"dim {dim} n {n} {out_dtype} flags {flags}"
                (assert_same_bf16 if out_dtype == BF16 else assert_same_f32)(out, ref, what)
                assert torch.equal(found, ref_found), what
                assert guards_intact(buf, n) and int(fbuf[0]) == SENT_U8 and bool((fbuf[1 + n:] == SENT_U8).all()), what
        for out_dtype in (torch.float32, BF16):   # aligned found, and no found at all
            buf, out = guarded(n, dim, out_dtype, dev)
            _, found = t.find(k, out=out, out_dtype=out_dtype)
            assert torch.equal(found, ref_found)
            buf2, out2 = guarded(n, dim, out_dtype, dev)
            assert t.find(k, out=out2, want_found=False, out_dtype=out_dtype)[1] is None
            for b, o in ((buf, out), (buf2, out2)):
                (assert_same_bf16 if out_dtype == BF16 else assert_same_f32)(o, ref, f"dim {dim} n {n} {out_dtype}")
                assert guards_intact(b, n)
    assert t.status() == tw.status()


# 3. mutators against the twin.  The movers see a bf16 row as dim / 8 opaque 16-byte groups: dim 8 -> 1 group and dim 200 -> 25 (run-time
# shape), dim 128 -> 16 and dim 256 -> 32 (the two compiled shapes)
def _compare(t, tw, probe, dev, what):
    assert t.size() == tw.size(), what
    assert t.status() == tw.status(), what
    (o, f), (ro, rf) = t.find(probe), tw.find(probe)
    assert torch.equal(f, rf), what
    assert_same_f32(o, ro, what)
    (k1, v1), (k2, v2) = sorted_export(t), sorted_export(tw)
    assert torch.equal(k1, k2), what
    assert_same_f32(v1, v2, what + ": export")
    cuts = [0, t.capacity // 3, t.capacity // 3 * 2 + 5, t.capacity]
    pieces = [t.export_range(a, b) for a, b in zip(cuts[:-1], cuts[1:])]
    pk, pv = torch.cat([p[0] for p in pieces]), torch.cat([p[1] for p in pieces])
    o = torch.argsort(pk)
    assert torch.equal(pk[o].cpu(), k1), what
    assert_same_f32(pv[o], v1, what + ": export_range")


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [8, 128, 200, 256])
def test_mutators_against_twin(dev, dim):
    t, tw = pair(dev, 1500, dim, default_value=-1.7)
    keys = synth.keys_np(21, 0, 1600)
    probe = K(np.concatenate([keys, [_lib.EMPTY_KEY, _lib.RECLAIMED_KEY]]), dev)
    rng = np.random.default_rng(7 + dim)

    def both(fn):
        return fn(t, False), fn(tw, True)

    def rows_of(batch, seed, twin):
        r = rows_for(batch, dim, seed)
        return (rnd(r) if twin else r).to(dev)

    # insert with duplicate keys in the batch (different rows: the last occurrence wins)
    b1 = np.concatenate([keys[:600], keys[100:300], keys[250:260]])
    r1 = torch.from_numpy(rng.standard_normal((len(b1), dim)).astype(np.float32))
    both(lambda x, twin: x.insert(K(b1, dev), (rnd(r1) if twin else r1).to(dev)))
    _compare(t, tw, probe, dev, "insert with duplicates")
    # insert with present keys (overwrite) and new ones, a reserved key in the batch
    b2 = np.concatenate([keys[500:900], [_lib.RECLAIMED_KEY], keys[0:50]])
    both(lambda x, twin: x.insert(K(b2, dev), rows_of(b2, 31, twin)))
    _compare(t, tw, probe, dev, "insert with present keys")
    t.clear_status(); tw.clear_status()
    # assign with absent keys and duplicates
    b3 = np.concatenate([keys[850:1000], keys[860:870]])
    f1, f2 = both(lambda x, twin: x.assign(K(b3, dev), rows_of(b3, 32, twin)))
    assert torch.equal(f1, f2) and 0 < int(f1.sum()) < len(b3)
    _compare(t, tw, probe, dev, "assign")
    # remove (present, absent, duplicate)
    b4 = np.concatenate([keys[0:400:2], keys[1200:1210], keys[0:10]])
    f1, f2 = both(lambda x, twin: x.remove(K(b4, dev)))
    assert torch.equal(f1, f2)
    _compare(t, tw, probe, dev, "remove")
    # insert again: tombstones are reused
    b5 = keys[900:1400]
    both(lambda x, twin: x.insert(K(b5, dev), rows_of(b5, 33, twin)))
    _compare(t, tw, probe, dev, "insert after remove")
    # reserve up and down: rows move bit for bit
    for cap in (5000, 1400):
        both(lambda x, twin: x.reserve(cap))
        assert t.capacity == tw.capacity and t.table_bytes == t.capacity * (8 + 2 * dim)
        _compare(t, tw, probe, dev, f"reserve({cap})")
    both(lambda x, twin: x.clear())
    _compare(t, tw, probe, dev, "clear")
    assert t.size() == 0


@pytest.mark.gpu
def test_full_table_against_twin(dev):
    """A table that runs full: TABLE_FULL and size == capacity on both.  WHICH keys of the batch found room is decided by the race of the
    claims, on either table, so the contents are checked against the batch (every stored key holds its own rounded row), not against the twin."""
    dim = 64
    t, tw = pair(dev, 32, dim)
    keys = synth.keys_np(23, 0, 3 * t.capacity)
    rows = rows_for(keys, dim, 9)
    insert_both(t, tw, keys, rows, dev)
    assert t.status() == tw.status() == _lib.STATUS_TABLE_FULL
    assert t.size() == tw.size() == t.capacity
    ek, ev = sorted_export(t)
    pos = {int(k): i for i, k in enumerate(keys)}
    assert_same_f32(ev, rnd(rows[[pos[int(k)] for k in ek]]), "stored rows of a full table")


# 4. verbatim bf16 input
@pytest.mark.gpu
def test_bf16_input_is_stored_verbatim(dev):
    from meepoembedding_amd import LookupTable
    dim, n = 64, 300
    rng = np.random.default_rng(4)
    pat = rng.integers(0, 1 << 16, (n, dim), dtype=np.uint16)      # every kind of bf16 pattern: NaN payloads, infinities, denormals
    pat[0, :8] = [0x7FC1, 0xFFFF, 0x7F80, 0xFF80, 0x0001, 0x8001, 0x0000, 0x8000]
    rows = torch.from_numpy(pat.view(np.int16)).view(BF16)
    keys = K(synth.keys_np(5, 0, n), dev)
    t = LookupTable(1000, dim, device=dev, max_batch=512, value_dtype=BF16)
    t.insert(keys, rows.to(dev))
    out16, found = t.find(keys, out_dtype=BF16)
    assert bool(found.all())
    nan = torch.isnan(rows)
    assert torch.equal(torch.isnan(out16.cpu()), nan) and torch.equal(bits16(out16)[~nan], bits16(rows)[~nan])
    assert_same_f32(t.find(keys)[0], rows.float(), "widened")
    rows2 = torch.from_numpy(rng.integers(0, 1 << 16, (n, dim), dtype=np.uint16).view(np.int16)).view(BF16)
    assert bool(t.assign(keys, rows2.to(dev)).all())
    out16 = t.find(keys, out_dtype=BF16)[0]
    nan = torch.isnan(rows2)
    assert torch.equal(torch.isnan(out16.cpu()), nan) and torch.equal(bits16(out16)[~nan], bits16(rows2)[~nan])
    # an fp32 table refuses bf16 input, in Python and in the library; so does a misaligned buffer on a bf16-row table
    f = LookupTable(1000, dim, device=dev, max_batch=512)
    with pytest.raises(MeepoError) as e:
        f.insert(keys, rows.to(dev))
    assert e.value.code == _lib.ERR_UNSUPPORTED
    L, d_rows = _lib.lib(), rows.to(dev)
    assert L.mee_insert_as(f._h, keys.data_ptr(), d_rows.data_ptr(), _lib.DTYPE_BF16, n, None) == _lib.ERR_UNSUPPORTED
    assert L.mee_assign_as(f._h, keys.data_ptr(), d_rows.data_ptr(), _lib.DTYPE_BF16, n, None, None) == _lib.ERR_UNSUPPORTED
    assert f.size() == 0
    assert L.mee_insert_as(t._h, keys.data_ptr(), d_rows.data_ptr() + 8, _lib.DTYPE_BF16, n - 1, None) == _lib.ERR_INVALID_ARG
    assert L.mee_insert_as(t._h, keys.data_ptr(), d_rows.data_ptr(), 7, n, None) == _lib.ERR_INVALID_ARG
    # MEE_DTYPE_F32 is mee_insert
    r32 = rows_for(synth.keys_np(5, 0, n), dim, 2)
    d32 = r32.to(dev)
    assert L.mee_insert_as(t._h, keys.data_ptr(), d32.data_ptr(), _lib.DTYPE_F32, n, None) == 0
    assert_same_bf16(t.find(keys, out_dtype=BF16)[0], r32, "mee_insert_as(F32)")


# 5. pooled parity with the twin
def _bags(lengths, n_extra_past, dev):
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    n = int(off[-1])
    # then: a bag that runs past n (cut at n), a decreasing pair (an empty bag), a bag wholly past n
    off = np.concatenate([off[:-1], [n - 3, n + n_extra_past, n - 5, n + 9, n + 20]]).astype(np.int64)
    return off, n


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [8, 64, 128, 200])
def test_pooled_parity_with_twin(dev, dim):
    t, tw = pair(dev, 3000, dim, default_value=0.3)
    allk = synth.keys_np(13, 0, 3000)
    stored = allk[:2000]
    insert_both(t, tw, stored, rows_for(stored, dim, 6), dev)
    rng = np.random.default_rng(100 + dim)
    base = [0, 1, 3, 15, 16, 17, 40]                      # 16 = kPoolLong
    shapes = {"wave per bag": base + [40, 33, 64],        # mean length >= 12
              "tile per bag": base + [2, 0, 1, 5, 3, 2, 1, 4, 2, 6, 1, 3, 2]}   # mean length < 12
    for name, lengths in shapes.items():
        off, n = _bags(lengths, 7, dev)
        n_bags = len(off) - 1
        assert (n // n_bags >= 12) == (name == "wave per bag")
        batch = np.where(rng.random(n) < 0.67, rng.choice(stored, n), rng.choice(allk[2000:], n))
        batch[5], batch[n - 20], batch[n - 1] = _lib.EMPTY_KEY, _lib.RECLAIMED_KEY, _lib.EMPTY_KEY
        k, o = K(batch, dev), K(off, dev)
        for mode in ("sum", "mean"):
            ref, ref_found = tw.find_pooled(k, o, mode=mode)
            for out_dtype in (torch.float32, BF16):
                buf, out = guarded(n_bags, dim, out_dtype, dev)
                _, found = t.find_pooled(k, o, mode=mode, out=out, out_dtype=out_dtype)
                what = f"dim {dim} {name} {mode} {out_dtype}"
                (assert_same_bf16 if out_dtype == BF16 else assert_same_f32)(out, ref, what)
                assert torch.equal(found, ref_found), what
                assert guards_intact(buf, n_bags), what


# 6. memory
@pytest.mark.gpu
@pytest.mark.parametrize("dim", [8, 64, 200])
def test_memory_accounting(dev, dim):
    t, tw = pair(dev, 5000, dim, max_batch=1000)
    assert t.value_dtype == BF16 and tw.value_dtype == torch.float32
    assert t.table_bytes == t.capacity * (8 + 2 * dim) and tw.table_bytes == tw.capacity * (8 + 4 * dim)
    assert t.workspace_bytes == tw.workspace_bytes + 1000 * dim * 2        # the pack scratch: one batch of rounded rows
    L = _lib.lib()
    for x, want in ((t, _lib.DTYPE_BF16), (tw, _lib.DTYPE_F32)):
        d = C.c_uint32(99)
        assert L.mee_table_value_dtype(x._h, C.byref(d)) == 0 and d.value == want
    ptr, stride, mem = C.c_void_p(), C.c_uint64(), C.c_uint32()
    assert L.mee_table_plane(t._h, 0, C.byref(ptr), C.byref(stride), C.byref(mem)) == 0
    assert stride.value == 2 * dim and mem.value == _lib.MEM_HBM and ptr.value
    assert L.mee_table_plane(t._h, 1, C.byref(ptr), C.byref(stride), C.byref(mem)) == _lib.ERR_UNSUPPORTED
    t.set_tuning("find_nt", 3)
    t.set_tuning("find_nt", -1)
    keys = K(synth.keys_np(2, 0, 100), dev)
    assert t.probe_length(keys) == tw.probe_length(keys) and t.probe_histogram(keys) == tw.probe_histogram(keys)
    u1, i1 = t.dedup_keys(torch.cat([keys, keys[:10]]))
    assert int((u1 != _lib.EMPTY_KEY).sum()) == 100 and torch.equal(u1[i1], torch.cat([keys, keys[:10]]))
    s1, f1 = t.locate(keys)
    assert not bool(f1.any()) and bool((s1 == -1).all())


# 7. refusals
_REFUSED = ["mee_find_located", "mee_find_located_as", "mee_find_located_prepare", "mee_find_located_prepare_as", "mee_find_many", "mee_find_unordered",
            "mee_find_missing", "mee_find_counted", "mee_find_pooled_weighted", "mee_find_pooled_as", "mee_pooled_weighted_backward", "mee_find_plane",
            "mee_assign_plane", "mee_find_or_insert", "mee_find_or_insert_as", "mee_find_or_insert_located", "mee_find_or_insert_located_as",
            "mee_find_or_insert_located_prepare", "mee_find_or_insert_located_prepare_as", "mee_find_or_insert_admit", "mee_find_or_insert_missing",
            "mee_insert_missing", "mee_hits_scan", "mee_apply_adagrad", "mee_apply_adam", "mee_apply_adagrad_located", "mee_apply_adam_located",
            "mee_apply_adagrad_indexed", "mee_apply_adam_indexed", "mee_apply_prepare", "mee_apply_discard", "mee_admission_decay", "mee_dedup_sum"]


@pytest.mark.gpu
def test_refusals(dev):
    """Every operator outside the supported list: MEE_ERR_UNSUPPORTED, a message that names the operator and the bf16-row table, and not one
    byte written.  The calls are made on the C-ABI with arguments built from the prototypes: every pointer argument is a device buffer of
    its own, pre-filled with a sentinel (so a call that was NOT refused would find valid memory), every count is 4."""
    from meepoembedding_amd import LookupTable
    L, dim, n = _lib.lib(), 64, 4
    t = LookupTable(1000, dim, device=dev, max_batch=64, value_dtype=BF16)
    f = LookupTable(1000, dim, device=dev, max_batch=64)
    keys = K(synth.keys_np(8, 0, n), dev)
    t.insert(keys, torch.ones(n, dim, device=dev))
    before = sorted_export(t)
    bufs = []

    def args_for(name, handles):
        res, argtypes = _lib.PROTOTYPES[name]
        out, handles = [], list(handles)
        for i, a in enumerate(argtypes):
            if i == len(argtypes) - 1:
                out.append(None)                                   # the stream
            elif handles and a is C.c_void_p and i < len(handles):
                out.append(handles[i])
            elif a is C.c_void_p:
                b = torch.full((1 << 14,), SENT_U8, dtype=torch.uint8, device=dev)
                bufs.append(b)
                out.append(b.data_ptr())
            elif a in (C.c_size_t,):
                out.append(n)
            elif a in (C.c_uint64, C.c_int, C.c_uint32):
                out.append(1 if a is C.c_uint64 else 0)            # step 1, plane 0, MEE_DTYPE_F32, MEE_POOL_SUM
            elif a is C.c_int64:
                out.append(-1)
            elif a is C.c_float:
                out.append(0.5)
            elif a is C.POINTER(C.c_size_t):
                out.append(C.byref(C.c_size_t(0)))
            elif a is C.POINTER(_lib.FindRequest):
                out.append((_lib.FindRequest * 1)())
            else:
                raise AssertionError((name, a))
        return out

    def refused(name, rc):
        msg = L.mee_last_error().decode()
        assert rc == _lib.ERR_UNSUPPORTED, (name, rc, msg)
        assert msg.startswith(name + ":") and "bf16-row table" in msg, (name, msg)     # the operator that was called, by its exact name

    for name in _REFUSED:
        refused(name, getattr(L, name)(*args_for(name, [t._h])))
    for hot, cold in ((t._h, f._h), (f._h, t._h)):                # the tiered lookup: either argument
        refused("mee_find_pooled_tiered", L.mee_find_pooled_tiered(*args_for("mee_find_pooled_tiered", [hot, cold])))
    # the creates that take tables: a bf16-row member is refused, which covers their whole families
    h = C.c_void_p()
    arr = (C.c_void_p * 2)(f._h, t._h)
    refused("mee_group_create", L.mee_group_create(arr, 2, 0, C.byref(h)))
    refused("mee_mixed_group_create", L.mee_mixed_group_create(arr, 2, 0, C.byref(h)))
    assert not h.value
    fake_comm = C.c_void_p(16)                                     # never looked at: the refusal comes first
    refused("mee_sharded_create", L.mee_sharded_create(t._h, fake_comm, 64, 0.0, C.byref(h)))
    opt = _lib.ShardedOptions(struct_size=C.sizeof(_lib.ShardedOptions), max_batch=64, cold=t._h)
    refused("mee_sharded_create", L.mee_sharded_create_ex(f._h, fake_comm, C.byref(opt), C.byref(h)))
    assert not h.value
    p = C.c_void_p()
    assert L.mee_p2p_create(dev.index, 1, 0, 64, 64, dim, 0, C.byref(p)) == 0
    refused("mee_p2p_find", L.mee_p2p_find(p, t._h, None))
    assert L.mee_p2p_destroy(p) == 0
    torch.cuda.synchronize(dev)
    for b in bufs:
        assert bool((b == SENT_U8).all())
    after = sorted_export(t)
    assert torch.equal(before[0], after[0]) and torch.equal(bits32(before[1]), bits32(after[1])) and t.status() == 0 and f.size() == 0
    # the Python methods surface the same error
    with pytest.raises(MeepoError) as e:
        t.find_or_insert(keys)
    assert e.value.code == _lib.ERR_UNSUPPORTED
    with pytest.raises(MeepoError) as e:
        t.find_pooled(keys, K(np.array([0, n]), dev), weights=torch.ones(n, device=dev))
    assert e.value.code == _lib.ERR_UNSUPPORTED


@pytest.mark.gpu
def test_create_time_combinations(dev):
    L = _lib.lib()
    base = dict(struct_size=C.sizeof(_lib.Config), device=dev.index, capacity=1000, dim=64, max_batch=64, flags=_lib.FLAG_BF16_ROWS)
    bad = {"optimizer": dict(optimizer=_lib.OPT_ADAGRAD), "multiple of 8": dict(dim=12), "TRACK_HITS": dict(flags=_lib.FLAG_BF16_ROWS | _lib.FLAG_TRACK_HITS),
           "ADMISSION": dict(flags=_lib.FLAG_BF16_ROWS | _lib.FLAG_ADMISSION), "MEE_MEM_HBM": dict(value_memory=_lib.MEM_HOST_PINNED)}
    for why, kw in bad.items():
        h = C.c_void_p()
        cfg = _lib.Config(**{**base, **kw})
        assert L.mee_table_create(C.byref(cfg), C.byref(h)) == _lib.ERR_INVALID_ARG and not h.value, why
        assert why in L.mee_last_error().decode(), (why, L.mee_last_error())
    h = C.c_void_p()
    cfg = _lib.Config(**base)
    assert L.mee_table_create(C.byref(cfg), C.byref(h)) == 0 and h.value
    assert L.mee_table_destroy(h) == 0


# 8. capture
@pytest.mark.gpu
def test_captured_lookups(dev):
    dim, n = 64, 777
    t, tw = pair(dev, 3000, dim, default_value=0.3)
    allk = synth.keys_np(17, 0, 3000)
    insert_both(t, tw, allk[:2000], rows_for(allk[:2000], dim, 4), dev)
    rng = np.random.default_rng(1)
    batches = [K(rng.choice(allk, n), dev) for _ in range(3)]
    off = K(np.arange(0, n + 1, 7, dtype=np.int64), dev)
    n_bags = off.numel() - 1
    kb = batches[0].clone()
    o32 = torch.empty(n, dim, device=dev); o16 = torch.empty(n, dim, dtype=BF16, device=dev)
    p32 = torch.empty(n_bags, dim, device=dev); p16 = torch.empty(n_bags, dim, dtype=BF16, device=dev)
    fnd = torch.empty(n, dtype=torch.uint8, device=dev); pf = torch.empty(n, dtype=torch.uint8, device=dev)

    def run():
        t.find(kb, out=o32, found=fnd)
        t.find(kb, out=o16, want_found=False, out_dtype=BF16)
        t.find_pooled(kb, off, mode="mean", out=p32, found=pf)
        t.find_pooled(kb, off, mode="sum", out=p16, found=pf, out_dtype=BF16)

    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream(dev).wait_stream(s)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for b in batches[1:]:
        kb.copy_(b)
        graph.replay()
        torch.cuda.synchronize(dev)
        e32, ef = t.find(b)
        assert torch.equal(bits32(o32), bits32(e32)) and torch.equal(fnd, ef)
        assert torch.equal(bits16(o16), bits16(t.find(b, out_dtype=BF16)[0]))
        assert torch.equal(bits32(p32), bits32(t.find_pooled(b, off, mode="mean")[0]))
        assert torch.equal(bits16(p16), bits16(t.find_pooled(b, off, mode="sum", out_dtype=BF16)[0]))
        assert_same_f32(o32, tw.find(b)[0], "replayed find against the twin")


# 9. train -> serve
@pytest.mark.gpu
def test_train_then_serve(dev, tmp_path):
    from meepoembedding_amd import OPT_ADAGRAD, LookupTable, checkpoint
    dim, n = 64, 700
    keys_np = synth.keys_np(31, 0, n)
    keys = K(keys_np, dev)
    train = LookupTable(2000, dim, device=dev, optimizer=OPT_ADAGRAD, max_batch=1024)
    train.insert(keys, rows_for(keys_np, dim, 3).to(dev))
    train.apply_adagrad(keys, (rows_for(keys_np, dim, 8) * 0.05).to(dev), lr=0.1)
    assert train.save(str(tmp_path / "fp32")) == n
    serve = LookupTable(5000, dim, device=dev, max_batch=256, value_dtype=BF16)   # another capacity, batches smaller than the checkpoint
    assert serve.load(str(tmp_path / "fp32")) == n and serve.size() == n
    probe = K(np.concatenate([keys_np, synth.keys_np(32, 0, 50)]), dev)
    want, want_found = train.find(probe)
    got, found = serve.find(probe, out_dtype=BF16)
    assert torch.equal(found, want_found)
    assert_same_bf16(got, want, "serve.find == bf16(train.find)")
    assert serve.save(str(tmp_path / "bf16")) == n
    with open(tmp_path / "bf16" / "meta.json") as fh:
        meta = json.load(fh)
    assert meta["extra"] == {"value_dtype": "bfloat16"} and meta["planes"] == ["values"] and meta["format"] == checkpoint.FORMAT
    assert os.path.getsize(tmp_path / "bf16" / "values.f32") == n * dim * 4          # the format is unchanged: fp32 rows
    second = LookupTable(1500, dim, device=dev, max_batch=1024, value_dtype=BF16)
    assert second.load(str(tmp_path / "bf16")) == n
    (k1, v1), (k2, v2) = sorted_export(serve), sorted_export(second)
    assert torch.equal(k1, k2) and torch.equal(bits32(v1), bits32(v2))
    resized = serve.resized(3000)
    assert resized.value_dtype == BF16 and torch.equal(bits32(sorted_export(resized)[1]), bits32(v1))
