"""int8 row storage (SPEC.md §3 "Row storage type"): LookupTable(int8_rows=True) (its .value_dtype is torch.int8), the C-ABI's MEE_FLAG_INT8_ROWS.

By definition an int8-row table is, bit for bit, an fp32 table that was handed D(Q(row)) instead of row, with the same (fp32, unquantized)
default_value.  Q and D are written here in numpy, in fp32 and nothing contracted:

    scale = max|x_i| / 127            one correctly rounded division
    q_i   = clamp(rint(x_i / scale), -127, 127), ties to even; every code 0 when scale == 0
    y_i   = (float)q_i * scale        one multiply

Every GPU case is a comparison of bit patterns against such a twin — an fp32 LookupTable of the same capacity and default on the same device,
fed D(Q(rows)) — or, for the stored bytes, against Q itself.  A bf16 result is compared with the twin's own bf16-out lookup (the library's
rounding) and with torch's CPU cast of the fp32 reference.  CPU half: the flag, the dtype constant, the create-time rules of the library (they
come before any device is asked for), the constructor's checks, the wrappers' refusal, the reference's own error bound.

An int8-row table has no pooled lookup (mee_find_pooled / _as are refused): test_refusals pins that."""
import ctypes as C
import json
import os
import types

import numpy as np
import pytest
import torch

from meepoembedding_amd import _lib, synth
from meepoembedding_amd._lib import MeepoError

I8, BF16 = torch.int8, torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT_F32, SENT_BF16, SENT_U8 = -777.25, -768.0, 0xAB   # guard values behind every result buffer (both exact in their type)
GIB = 1 << 30


# ---- the reference ------------------------------------------------------------------------------------------------------
def Q(x):
    """fp32 rows [n, dim] -> (int8 codes [n, dim], fp32 scales [n])"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    scale = (np.abs(x).max(axis=1) / np.float32(127.0)).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.rint(x / scale[:, None])            # fp32 division, ties to even
    q = np.clip(q, np.float32(-127.0), np.float32(127.0))
    q = np.where(scale[:, None] == 0, np.float32(0.0), q)
    return q.astype(np.int8), scale


def D(q, scale):
    return (q.astype(np.float32) * scale[:, None].astype(np.float32)).astype(np.float32)


def DQ(rows: torch.Tensor) -> torch.Tensor:
    """what the twin is fed"""
    return torch.from_numpy(D(*Q(rows.detach().cpu().numpy())))


# ---- helpers --------------------------------------------------------------------------------------------------------------
def bits32(x):
    return x.detach().cpu().contiguous().view(torch.int32)


def bits16(x):
    return x.detach().cpu().contiguous().view(torch.int16)


def assert_same_f32(got, ref, what=""):
    got, ref = got.detach().cpu(), ref.detach().cpu()
    assert got.dtype == ref.dtype == torch.float32 and got.shape == ref.shape, (what, got.dtype, got.shape, ref.shape)
    bad = int((bits32(got) != bits32(ref)).sum())
    assert bad == 0, f"{what}: {bad} of {got.numel()} fp32 patterns differ"


def assert_same_bf16(got, ref_bf16, ref_f32, what=""):
    """a bf16 result against the twin's bf16 result and against torch's CPU cast of the twin's fp32 result, bit for bit"""
    got = got.detach().cpu()
    assert got.dtype == BF16 and got.shape == ref_bf16.shape, (what, got.dtype, got.shape)
    bad = int((bits16(got) != bits16(ref_bf16)).sum())
    assert bad == 0, f"{what}: {bad} of {got.numel()} bf16 patterns differ from the twin's"
    assert torch.equal(bits16(got), bits16(ref_f32.detach().cpu().to(BF16))), f"{what}: differs from the CPU cast"


def K(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def rows_for(keys_np, dim, seed):
    """rows with full fp32 mantissas, a function of the key; every row at a magnitude of its own (1e-3 .. 1e3)"""
    r = synth.rows_np(keys_np, dim, seed).astype(np.float32) * np.float32(1.37)
    mag = np.float32(10.0) ** ((keys_np.astype(np.uint64) % np.uint64(7)).astype(np.float32) - np.float32(3.0))
    return torch.from_numpy((r * mag[:, None]).astype(np.float32))


def pair(dev, capacity, dim, default_value=0.0, max_batch=4096):
    """(int8-row table, its fp32 twin: same capacity, same default)"""
    from meepoembedding_amd import LookupTable
    t = LookupTable(capacity, dim, device=dev, max_batch=max_batch, default_value=default_value, int8_rows=True)
    tw = LookupTable(capacity, dim, device=dev, max_batch=max_batch, default_value=default_value)
    assert t.capacity == tw.capacity and t.default_value == tw.default_value
    return t, tw


def insert_both(t, tw, keys_np, rows, dev):
    for s in range(0, len(keys_np), t.max_batch):
        k = K(keys_np[s:s + t.max_batch], dev)
        t.insert(k, rows[s:s + t.max_batch].to(dev))
        tw.insert(k, DQ(rows[s:s + t.max_batch]).to(dev))


def guarded(n, dim, dtype, dev):
    buf = torch.full((n + 2, dim), SENT_BF16 if dtype == BF16 else SENT_F32, dtype=dtype, device=dev)
    return buf, buf[:n]


def guards_intact(buf, n):
    return bool((buf[n:].float() == (SENT_BF16 if buf.dtype == BF16 else SENT_F32)).all())


def sorted_export(t):
    k, v = t.export()
    o = torch.argsort(k)
    return k[o].cpu(), v[o].cpu()


def plane_of(t):
    """the value plane of a table as it lies in HBM: (uint8 [capacity, stride], stride)"""
    L = _lib.lib()
    ptr, stride, mem = C.c_void_p(), C.c_uint64(), C.c_uint32()
    assert L.mee_table_plane(t._h, 0, C.byref(ptr), C.byref(stride), C.byref(mem)) == 0 and ptr.value and mem.value == _lib.MEM_HBM
    torch.cuda.synchronize(t.device)
    host = np.empty((t.capacity, stride.value), dtype=np.uint8)
    copy = C.CDLL(_lib.LIB_PATH).hipMemcpy           # (the HIP runtime the library is linked against)
    copy.restype, copy.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert copy(host.ctypes.data, ptr, host.nbytes, 2) == 0    # hipMemcpyDeviceToHost
    return host, stride.value


def stored_rows(t, keys_np, dev):
    """the stored bytes of every key -> (codes int8 [n, dim], scale bits uint32 [n], the twelve reserved bytes [n, 12])"""
    slots, found = t.locate(K(keys_np, dev))
    assert bool(found.all())
    plane, stride = plane_of(t)
    assert stride == t.dim + 16
    raw = plane[(slots & _lib.HANDLE_SLOT_MASK).cpu().numpy()]
    return raw[:, :t.dim].view(np.int8), np.ascontiguousarray(raw[:, t.dim:t.dim + 4]).view(np.uint32)[:, 0], raw[:, t.dim + 4:]


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_flag_dtype_and_create_rules(built):
    """fails on the parent commit: the flag is an unknown bit there.  The create-time rules are checked on the C-ABI: mee_table_create looks at
    its arguments before it asks for a device, so each violation is MEE_ERR_INVALID_ARG with a message that names the rule — on any machine."""
    assert _lib.FLAG_INT8_ROWS == 8 and _lib.DTYPE_INT8 == 2
    with open(os.path.join(ROOT, "include", "meepo_embedding.h")) as f:
        header = f.read()
    assert "MEE_FLAG_INT8_ROWS = 8u" in header and "MEE_DTYPE_INT8 = 2" in header
    with open(os.path.join(ROOT, "include", "meepo_embedding.hpp")) as f:
        assert "int8_rows" in f.read()
    L = _lib.lib()
    for s in ("mee_insert_as", "mee_assign_as", "mee_table_value_dtype", "mee_find_as", "mee_table_plane", "mee_reserve"):
        assert hasattr(L, s), s
    assert L.mee_abi_version() == 2 and C.sizeof(_lib.Config) == 64 and C.sizeof(_lib.TableInfo) == 48   # additive: nothing pinned moved
    with open(_lib.LIB_PATH, "rb") as f:
        blob = f.read()
    assert b"quantize_rows_kernel" in blob        # the new pack instance is in the built library
    base = dict(struct_size=C.sizeof(_lib.Config), device=0, capacity=1000, dim=64, max_batch=64, flags=_lib.FLAG_INT8_ROWS)
    bad = {"optimizer": dict(optimizer=_lib.OPT_ADAGRAD), "multiple of 16": dict(dim=24), "TRACK_HITS": dict(flags=_lib.FLAG_INT8_ROWS | _lib.FLAG_TRACK_HITS),
           "ADMISSION": dict(flags=_lib.FLAG_INT8_ROWS | _lib.FLAG_ADMISSION), "MEE_MEM_HBM": dict(value_memory=_lib.MEM_HOST_PINNED),
           "MEE_FLAG_BF16_ROWS": dict(flags=_lib.FLAG_INT8_ROWS | _lib.FLAG_BF16_ROWS)}
    for why, kw in bad.items():
        h = C.c_void_p()
        cfg = _lib.Config(**{**base, **kw})
        assert L.mee_table_create(C.byref(cfg), C.byref(h)) == _lib.ERR_INVALID_ARG and not h.value, why
        msg = L.mee_last_error().decode()
        assert "MEE_FLAG_INT8_ROWS" in msg and why in msg, (why, msg)
    h = C.c_void_p()
    cfg = _lib.Config(**{**base, "dim": 8, "flags": _lib.FLAG_INT8_ROWS})
    assert L.mee_table_create(C.byref(cfg), C.byref(h)) == _lib.ERR_INVALID_ARG and "multiple of 16" in L.mee_last_error().decode()


def test_constructor_checks_come_before_the_device(built):
    """every ValueError of LookupTable(int8_rows=True) fires before a device (or the library) is needed: device='cpu' would be a MeepoError"""
    from meepoembedding_amd import OPT_ADAGRAD, OPT_ADAM, LookupTable
    bad = [dict(optimizer=OPT_ADAGRAD), dict(optimizer=OPT_ADAM), dict(track_hits=True), dict(admission=True), dict(value_memory=_lib.MEM_HOST_PINNED)]
    for kw in bad:
        with pytest.raises(ValueError, match="int8"):
            LookupTable(1024, 64, device="cpu", int8_rows=True, **kw)
    for dim in (24, 8, 4, 40, 1016):
        with pytest.raises(ValueError, match="multiple of 16"):
            LookupTable(1024, dim, device="cpu", int8_rows=True)
    with pytest.raises(ValueError, match="one row storage type"):      # both row types at once
        LookupTable(1024, 64, device="cpu", int8_rows=True, value_dtype=BF16)
    with pytest.raises(ValueError, match="int8_rows=True"):            # value_dtype stays fp32 | bf16: the message points to the keyword
        LookupTable(1024, 64, device="cpu", value_dtype=I8)
    with pytest.raises(MeepoError):   # the arguments are fine: now it is the device that is missing
        LookupTable(1024, 64, device="cpu", int8_rows=True)


def test_wrappers_refuse_an_int8_row_table():
    """groups (uniform ones too: there is no int8-row group), tiers, shards, peers and layers refuse a table with value_dtype == int8 at
    construction, before they touch it, through _lib's one helper; the message names the row type"""
    from meepoembedding_amd import MixedTableGroup, TableGroup
    from meepoembedding_amd.nn import DynamicEmbedding, DynamicEmbeddingBag, DynamicEmbeddingCollection
    from meepoembedding_amd.p2p import PeerShardedFind
    from meepoembedding_amd.sharded import RcclShardedTable, ShardedLookupTable, ShardedTableGroup
    from meepoembedding_amd.tiered import TieredLookupTable
    q = types.SimpleNamespace(value_dtype=I8, dim=64)           # anything else it lacks: nobody may get that far
    f = types.SimpleNamespace(value_dtype=torch.float32, dim=64)
    b = types.SimpleNamespace(value_dtype=BF16, dim=64)
    grp = types.SimpleNamespace(tables=[f, q], dim=64)
    makers = [lambda: TableGroup([f, q]), lambda: TableGroup([q, q]), lambda: TableGroup([q]), lambda: TableGroup([b, q]), lambda: MixedTableGroup([q]),
              lambda: TieredLookupTable(q, f), lambda: TieredLookupTable(f, q), lambda: ShardedLookupTable(q, None), lambda: ShardedTableGroup(grp, None),
              lambda: RcclShardedTable(q, 16), lambda: RcclShardedTable(f, 16, cold=q), lambda: PeerShardedFind(q, None, 16), lambda: DynamicEmbedding(q),
              lambda: DynamicEmbeddingBag(q), lambda: DynamicEmbeddingBag(grp), lambda: DynamicEmbeddingCollection(grp)]
    for i, mk in enumerate(makers):
        with pytest.raises(MeepoError, match="int8-row table") as e:
            mk()
        assert e.value.code == _lib.ERR_UNSUPPORTED, i
    with pytest.raises(MeepoError, match="bf16-row table"):     # the generalised helper still names the other serving type
        _lib.refuse_narrow_rows("X", b)
    _lib.refuse_narrow_rows("X", f, None)


def test_reference_error_bound():
    """|D(Q(x)) - x| <= (0.5 + 2^-10) * scale on random rows at magnitudes 1e-38 .. 1e30; codes stay in [-127, 127], the extreme has |code| 127"""
    rng = np.random.default_rng(5)
    for dim in (16, 64):
        x = rng.standard_normal((20000, dim)).astype(np.float32)
        x *= (np.float32(10.0) ** rng.uniform(-38, 30, (20000, 1))).astype(np.float32)
        q, s = Q(x)
        err = np.abs(D(q, s).astype(np.float64) - x.astype(np.float64))
        assert bool((err <= (0.5 + 2.0 ** -10) * s.astype(np.float64)[:, None]).all())
        assert q.min() >= -127 and bool((np.abs(q.astype(np.int32)).max(axis=1) == 127).all())
    z, s = Q(np.zeros((2, 16), np.float32))
    assert not z.any() and not s.any() and not D(z, s).any()
    t, s = Q(np.array([[0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 126.5, 127.0] * 2], np.float32))
    assert s[0] == 1.0 and t[0, :8].tolist() == [0, 2, 2, 0, -2, -2, 126, 127]      # ties to even


# ---- GPU ----------------------------------------------------------------------------------------------------------------
# 1. what a write stores
def _special_rows(dim, rng):
    n_rand = 40
    rows = [rng.standard_normal((n_rand, dim)).astype(np.float32) * (np.float32(10.0) ** rng.uniform(-6, 6, (n_rand, 1))).astype(np.float32)]
    rows.append(np.zeros((1, dim), np.float32))                                               # all zero: scale 0, codes 0
    neg = rng.uniform(-1, 1, (1, dim)).astype(np.float32); neg[0, dim // 3] = np.float32(-3.7)   # the extreme is negative: code -127
    rows.append(neg)
    ties = (rng.integers(-126, 126, (1, dim)).astype(np.float32) + np.float32(0.5)); ties[0, 0] = np.float32(127.0); ties[0, 1:7] = [0.5, 1.5, 2.5, -0.5, -1.5, -2.5]
    rows.append(ties)                                                                         # scale == 1, x.5 values: ties to even
    rows.append((rng.standard_normal((2, dim)) * 1e-39).astype(np.float32))                   # denormal magnitudes (the scale is a denormal too)
    rows.append((rng.uniform(-1, 1, (2, dim)) * 3.0e38).astype(np.float32))                   # near the top of fp32
    one = np.zeros((1, dim), np.float32); one[0, dim - 1] = np.float32(-1e-3)                 # one element only, the last
    rows.append(one)
    return np.concatenate(rows)


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [16, 64, 208, 1024])
def test_quantize_on_write(dev, dim):
    from meepoembedding_amd import LookupTable
    rng = np.random.default_rng(dim)
    rows = _special_rows(dim, rng)
    assert np.isfinite(rows).all() and (np.abs(rows[-3:-1]).max() > 1e38) and np.abs(rows[-5:-3]).max() < 1.2e-38
    n = len(rows)
    keys = synth.keys_np(3, 0, n)
    wq, ws = Q(rows)
    t = LookupTable(256, dim, device=dev, max_batch=64, int8_rows=True)
    for how in ("insert", "assign"):
        if how == "insert":
            t.insert(K(keys, dev), torch.from_numpy(rows).to(dev))
        else:
            t.insert(K(keys, dev), torch.ones(n, dim, device=dev))
            assert bool(t.assign(K(keys, dev), torch.from_numpy(rows).to(dev)).all())
        codes, scale_bits, tail = stored_rows(t, keys, dev)
        for i in np.flatnonzero((scale_bits != ws.view(np.uint32)) | (codes != wq).any(axis=1)):
            print(f"dim {dim} {how} row {i}: scale {ws[i]!r} stored {scale_bits[i:i + 1].view(np.float32)[0]!r}, {int((codes[i] != wq[i]).sum())} codes differ")
        assert np.array_equal(scale_bits, ws.view(np.uint32)), how
        assert np.array_equal(codes, wq), how
        assert not tail.any(), how
        out, found = t.find(K(keys, dev))
        assert bool(found.all()) and t.status() == 0
        assert_same_f32(out, torch.from_numpy(D(wq, ws)), how)
    assert ws[40] == 0 and not wq[40].any() and wq[41].min() == -127 and ws[42] == 1.0


# 2. lookup parity with the twin
_FIND_FLAGS = [f for f in range(16) if (f & 3) != 3]   # every mee_find_ex combination (stream and cached stores exclude each other)


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [16, 48, 64, 128, 208, 1024])
def test_find_parity_with_twin(dev, dim):
    t, tw = pair(dev, 3300, dim, default_value=0.3)
    n_keys = int(0.92 * t.capacity)
    allk = synth.keys_np(11, 0, 2 * n_keys)
    stored = allk[:n_keys]
    insert_both(t, tw, stored, rows_for(stored, dim, 5), dev)
    assert t.size() == tw.size() == n_keys and t.status() == tw.status() == 0
    assert n_keys / t.capacity >= 0.9 and t.probe_length(K(stored, dev)) > 1.05   # probes go beyond the home bucket
    rng = np.random.default_rng(dim)
    flagged = dim in (48, 64, 128)             # every policy bit on both compiled shapes and on the run-time one
    for n in (1, 7, 1003):                     # none a multiple of the wave step (4 or 8 positions)
        batch = np.where(rng.random(n) < 0.67, rng.choice(stored, n), rng.choice(allk[n_keys:], n))
        if n >= 7:
            batch[2], batch[n - 2] = _lib.EMPTY_KEY, _lib.RECLAIMED_KEY
        k = K(batch, dev)
        ref, ref_found = tw.find(k)
        ref16 = tw.find(k, out_dtype=BF16)[0].cpu()
        if n == 1003:
            assert 0 < int(ref_found.sum()) < n

        def same(out, what):
            if out.dtype == BF16:
                assert_same_bf16(out, ref16, ref, what)
            else:
                assert_same_f32(out, ref, what)

        for out_dtype in (torch.float32, BF16):
            for flags in [None] + (_FIND_FLAGS if flagged else []):
                buf, out = guarded(n, dim, out_dtype, dev)
                fbuf = torch.full((n + 3,), SENT_U8, dtype=torch.uint8, device=dev)
                found = fbuf[1:1 + n]        # one byte off any alignment: the unaligned found path
                t.find(k, out=out, found=found, flags=flags, out_dtype=out_dtype)
                what = f"dim {dim} n {n} {out_dtype} flags {flags}"
                same(out, what)
                assert torch.equal(found, ref_found), what
                assert guards_intact(buf, n) and int(fbuf[0]) == SENT_U8 and bool((fbuf[1 + n:] == SENT_U8).all()), what
        for out_dtype in (torch.float32, BF16):   # aligned found, and no found at all
            buf, out = guarded(n, dim, out_dtype, dev)
            _, found = t.find(k, out=out, out_dtype=out_dtype)
            assert torch.equal(found, ref_found)
            buf2, out2 = guarded(n, dim, out_dtype, dev)
            assert t.find(k, out=out2, want_found=False, out_dtype=out_dtype)[1] is None
            for b, o in ((buf, out), (buf2, out2)):
                same(o, f"dim {dim} n {n} {out_dtype}")
                assert guards_intact(b, n)
    # a hit-only batch of whole wave steps: the wave-uniform fast path alone
    k = K(stored[:1024], dev)
    assert_same_f32(t.find(k)[0], tw.find(k)[0], "all hits")
    assert t.status() == tw.status()


@pytest.mark.gpu
def test_full_table_against_twin(dev):
    """A table that runs full: TABLE_FULL and size == capacity on both.  WHICH keys of the batch found room is decided by the race of the
    claims, on either table, so the contents are checked against the batch (every stored key holds its own quantized row), not against the twin."""
    dim = 64
    t, tw = pair(dev, 32, dim)
    keys = synth.keys_np(23, 0, 3 * t.capacity)
    rows = rows_for(keys, dim, 9)
    insert_both(t, tw, keys, rows, dev)
    assert t.status() == tw.status() == _lib.STATUS_TABLE_FULL
    assert t.size() == tw.size() == t.capacity
    ek, ev = sorted_export(t)
    pos = {int(k): i for i, k in enumerate(keys)}
    want = DQ(rows[[pos[int(k)] for k in ek]])
    assert_same_f32(ev, want, "stored rows of a full table")
    out, found = t.find(K(ek.numpy(), dev))
    assert bool(found.all())
    assert_same_f32(out, want, "find on a full table")


# 3. mutators against the twin.  The movers see an int8 row as dim / 16 + 1 opaque 16-byte groups: dim 16 -> 2 and dim 64 -> 5 (run-time shape),
# dim 240 -> 16 and dim 496 -> 32 (the two compiled shapes)
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
@pytest.mark.parametrize("dim", [16, 64, 240, 496])
def test_mutators_against_twin(dev, dim):
    t, tw = pair(dev, 1500, dim, default_value=-1.7)
    keys = synth.keys_np(21, 0, 1600)
    probe = K(np.concatenate([keys, [_lib.EMPTY_KEY, _lib.RECLAIMED_KEY]]), dev)
    rng = np.random.default_rng(7 + dim)

    def both(fn):
        return fn(t, False), fn(tw, True)

    def rows_of(batch, seed, twin):
        r = rows_for(batch, dim, seed)
        return (DQ(r) if twin else r).to(dev)

    # insert with duplicate keys in the batch (different rows: the last occurrence wins)
    b1 = np.concatenate([keys[:600], keys[100:300], keys[250:260]])
    r1 = torch.from_numpy(rng.standard_normal((len(b1), dim)).astype(np.float32))
    both(lambda x, twin: x.insert(K(b1, dev), (DQ(r1) if twin else r1).to(dev)))
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
    # reserve up and down: rows move verbatim — the same lookups, and the same stored bytes for every key
    held = sorted_export(t)[0].numpy()
    before = stored_rows(t, held, dev)
    for cap in (5000, 1400):
        both(lambda x, twin: x.reserve(cap))
        assert t.capacity == tw.capacity and t.table_bytes == t.capacity * (8 + dim + 16)
        _compare(t, tw, probe, dev, f"reserve({cap})")
        after = stored_rows(t, held, dev)
        assert all(np.array_equal(a, b) for a, b in zip(before, after)), f"reserve({cap}): stored bytes"
    both(lambda x, twin: x.clear())
    _compare(t, tw, probe, dev, "clear")
    assert t.size() == 0


# 5. memory
@pytest.mark.gpu
@pytest.mark.parametrize("dim", [16, 64, 208])
def test_memory_accounting(dev, dim):
    t, tw = pair(dev, 5000, dim, max_batch=1000)
    assert t.value_dtype == I8 and tw.value_dtype == torch.float32
    L = _lib.lib()
    for cap in (None, 9000, 2000):
        if cap:
            t.reserve(cap); tw.reserve(cap)
        assert t.capacity == tw.capacity
        assert t.table_bytes == t.capacity * (8 + dim + 16) and tw.table_bytes == tw.capacity * (8 + 4 * dim), cap
        assert t.workspace_bytes == tw.workspace_bytes + 1000 * (dim + 16), cap      # the pack scratch: one batch of quantized rows
        info = _lib.TableInfo()
        assert L.mee_table_info_get(t._h, C.byref(info)) == 0
        assert info.table_bytes == t.capacity * (8 + dim + 16) and info.workspace_bytes == t.workspace_bytes and info.capacity == t.capacity
    for x, want in ((t, _lib.DTYPE_INT8), (tw, _lib.DTYPE_F32)):
        d = C.c_uint32(99)
        assert L.mee_table_value_dtype(x._h, C.byref(d)) == 0 and d.value == want
    ptr, stride, mem = C.c_void_p(), C.c_uint64(), C.c_uint32()
    assert L.mee_table_plane(t._h, 0, C.byref(ptr), C.byref(stride), C.byref(mem)) == 0
    assert stride.value == dim + 16 and mem.value == _lib.MEM_HBM and ptr.value
    assert L.mee_table_plane(t._h, 1, C.byref(ptr), C.byref(stride), C.byref(mem)) == _lib.ERR_UNSUPPORTED
    keys = K(synth.keys_np(2, 0, 100), dev)
    assert t.probe_length(keys) == tw.probe_length(keys) and t.probe_histogram(keys) == tw.probe_histogram(keys)
    s1, f1 = t.locate(keys)
    assert not bool(f1.any()) and bool((s1 == -1).all())


# 6. refusals
_REFUSED = ["mee_find_pooled", "mee_find_located", "mee_find_located_as", "mee_find_located_prepare", "mee_find_located_prepare_as", "mee_find_many", "mee_find_unordered",
            "mee_find_missing", "mee_find_counted", "mee_find_pooled_weighted", "mee_find_pooled_as", "mee_pooled_weighted_backward", "mee_find_plane",
            "mee_assign_plane", "mee_find_or_insert", "mee_find_or_insert_as", "mee_find_or_insert_located", "mee_find_or_insert_located_as",
            "mee_find_or_insert_located_prepare", "mee_find_or_insert_located_prepare_as", "mee_find_or_insert_admit", "mee_find_or_insert_missing",
            "mee_insert_missing", "mee_hits_scan", "mee_apply_adagrad", "mee_apply_adam", "mee_apply_adagrad_located", "mee_apply_adam_located",
            "mee_apply_adagrad_indexed", "mee_apply_adam_indexed", "mee_apply_prepare", "mee_apply_discard", "mee_admission_decay", "mee_dedup_sum"]


@pytest.mark.gpu
def test_refusals(dev):
    """Every operator outside the supported list: MEE_ERR_UNSUPPORTED, a message that names the operator and the int8-row table, and not one
    byte written.  The calls are made on the C-ABI with arguments built from the prototypes: every pointer argument is a device buffer of
    its own, pre-filled with a sentinel (so a call that was NOT refused would find valid memory), every count is 4.  The pooled lookups are
    among them, weighted or not: an int8-row table has none.  Then the typed forms: bf16 input is UNSUPPORTED, MEE_DTYPE_INT8 as an in / out dtype INVALID_ARG."""
    from meepoembedding_amd import LookupTable, MixedTableGroup, TableGroup
    L, dim, n = _lib.lib(), 64, 4
    t = LookupTable(1000, dim, device=dev, max_batch=64, int8_rows=True)
    f = LookupTable(1000, dim, device=dev, max_batch=64)
    b = LookupTable(1000, dim, device=dev, max_batch=64, value_dtype=BF16)
    keys = K(synth.keys_np(8, 0, n), dev)
    t.insert(keys, torch.ones(n, dim, device=dev))
    before = sorted_export(t)
    plane_before = plane_of(t)[0]
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
                buf = torch.full((1 << 14,), SENT_U8, dtype=torch.uint8, device=dev)
                bufs.append(buf)
                out.append(buf.data_ptr())
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
        assert msg.startswith(name + ":") and "int8-row table" in msg, (name, msg)     # the operator that was called, by its exact name

    for name in _REFUSED:
        refused(name, getattr(L, name)(*args_for(name, [t._h])))
    for hot, cold in ((t._h, f._h), (f._h, t._h)):                # the tiered lookup: either argument
        refused("mee_find_pooled_tiered", L.mee_find_pooled_tiered(*args_for("mee_find_pooled_tiered", [hot, cold])))
    # the creates that take tables: an int8-row member is refused — beside fp32 members, beside bf16-row members, and alone
    h = C.c_void_p()
    for members in ((f._h, t._h), (b._h, t._h), (t._h, t._h)):
        arr = (C.c_void_p * 2)(*members)
        refused("mee_group_create", L.mee_group_create(arr, 2, 0, C.byref(h)))
        if members[0] != b._h:
            refused("mee_mixed_group_create", L.mee_mixed_group_create(arr, 2, 0, C.byref(h)))
        else:      # (a mixed group takes neither serving type: the bf16-row member in front is the one the message names)
            assert L.mee_mixed_group_create(arr, 2, 0, C.byref(h)) == _lib.ERR_UNSUPPORTED
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
    # typed input and output
    rows16 = torch.ones(n, dim, dtype=BF16, device=dev)
    rows32 = torch.full((n, dim), 2.0, device=dev)
    out = torch.full((n, dim), SENT_F32, device=dev)
    assert L.mee_insert_as(t._h, keys.data_ptr(), rows16.data_ptr(), _lib.DTYPE_BF16, n, None) == _lib.ERR_UNSUPPORTED
    assert L.mee_assign_as(t._h, keys.data_ptr(), rows16.data_ptr(), _lib.DTYPE_BF16, n, None, None) == _lib.ERR_UNSUPPORTED
    assert L.mee_insert_as(t._h, keys.data_ptr(), rows32.data_ptr(), _lib.DTYPE_INT8, n, None) == _lib.ERR_INVALID_ARG
    assert L.mee_assign_as(t._h, keys.data_ptr(), rows32.data_ptr(), _lib.DTYPE_INT8, n, None, None) == _lib.ERR_INVALID_ARG
    assert L.mee_find_as(t._h, keys.data_ptr(), n, out.data_ptr(), _lib.DTYPE_INT8, None, 0, None) == _lib.ERR_INVALID_ARG
    off = K(np.array([0, n], dtype=np.int64), dev)
    refused("mee_find_pooled_as", L.mee_find_pooled_as(t._h, keys.data_ptr(), n, off.data_ptr(), 1, None, out.data_ptr(), _lib.DTYPE_F32, None, None, 0, None))   # unweighted too
    assert L.mee_find_pooled_as(f._h, keys.data_ptr(), n, off.data_ptr(), 1, None, out.data_ptr(), _lib.DTYPE_INT8, None, None, 0, None) == _lib.ERR_INVALID_ARG
    assert L.mee_find_as(f._h, keys.data_ptr(), n, out.data_ptr(), _lib.DTYPE_INT8, None, 0, None) == _lib.ERR_INVALID_ARG      # on any table
    torch.cuda.synchronize(dev)
    assert bool((out == SENT_F32).all())
    for buf in bufs:
        assert bool((buf == SENT_U8).all())
    after = sorted_export(t)
    assert torch.equal(before[0], after[0]) and torch.equal(bits32(before[1]), bits32(after[1])) and t.status() == 0 and f.size() == 0 and b.size() == 0
    assert np.array_equal(plane_before, plane_of(t)[0])
    # the Python methods and wrappers surface the same error
    for call in (lambda: t.find_or_insert(keys), lambda: t.find_pooled(keys, off, weights=torch.ones(n, device=dev)), lambda: t.find_pooled(keys, off),
                 lambda: t.insert(keys, rows16),
                 lambda: TableGroup([t]), lambda: TableGroup([f, t]), lambda: MixedTableGroup([t, f])):
        with pytest.raises(MeepoError) as e:
            call()
        assert e.value.code == _lib.ERR_UNSUPPORTED
    # MEE_DTYPE_F32 is mee_insert / mee_assign
    assert L.mee_insert_as(t._h, keys.data_ptr(), rows32.data_ptr(), _lib.DTYPE_F32, n, None) == 0
    assert bool((t.find(keys)[0] == 2.0).all())
    fnd = torch.zeros(n, dtype=torch.uint8, device=dev)
    assert L.mee_assign_as(t._h, keys.data_ptr(), (rows32 * 2).data_ptr(), _lib.DTYPE_F32, n, fnd.data_ptr(), None) == 0
    assert bool((t.find(keys)[0] == 4.0).all()) and bool(fnd.all())


# 7. capture
@pytest.mark.gpu
def test_captured_lookups(dev):
    dim, n = 64, 777
    t, tw = pair(dev, 3000, dim, default_value=0.3)
    allk = synth.keys_np(17, 0, 3000)
    insert_both(t, tw, allk[:2000], rows_for(allk[:2000], dim, 4), dev)
    rng = np.random.default_rng(1)
    batches = [K(rng.choice(allk, n), dev) for _ in range(3)]
    kb = batches[0].clone()
    o32 = torch.empty(n, dim, device=dev); o16 = torch.empty(n, dim, dtype=BF16, device=dev)
    fnd = torch.empty(n, dtype=torch.uint8, device=dev)

    def run():
        t.find(kb, out=o32, found=fnd)
        t.find(kb, out=o16, want_found=False, out_dtype=BF16)

    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream(dev).wait_stream(s)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for bt in batches[1:]:
        kb.copy_(bt)
        graph.replay()
        torch.cuda.synchronize(dev)
        e32, ef = t.find(bt)
        assert torch.equal(bits32(o32), bits32(e32)) and torch.equal(fnd, ef)
        assert torch.equal(bits16(o16), bits16(t.find(bt, out_dtype=BF16)[0]))
        assert_same_f32(o32, tw.find(bt)[0], "replayed find against the twin")
        assert_same_bf16(o16, tw.find(bt, out_dtype=BF16)[0].cpu(), tw.find(bt)[0], "replayed bf16 find against the twin")


# 8. train -> serve
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
    serve = LookupTable(5000, dim, device=dev, max_batch=256, int8_rows=True)   # another capacity, batches smaller than the checkpoint
    assert serve.load(str(tmp_path / "fp32")) == n and serve.size() == n
    # the twin: an fp32 table fed D(Q(.)) of the same checkpoint's rows
    ck = np.fromfile(tmp_path / "fp32" / "keys.i64", dtype=np.int64)
    cv = np.fromfile(tmp_path / "fp32" / "values.f32", dtype=np.float32).reshape(n, dim)
    twin = LookupTable(5000, dim, device=dev, max_batch=1024)
    twin.insert(K(ck, dev), DQ(torch.from_numpy(cv)).to(dev))
    probe = K(np.concatenate([keys_np, synth.keys_np(32, 0, 50)]), dev)
    want, want_found = twin.find(probe)
    got, found = serve.find(probe)
    assert torch.equal(found, want_found) and int(found.sum()) == n
    assert_same_f32(got, want, "serve.find == twin.find")
    assert_same_bf16(serve.find(probe, out_dtype=BF16)[0], twin.find(probe, out_dtype=BF16)[0].cpu(), want, "bf16 out")
    trained = train.find(probe)[0].cpu()
    scale = (trained.abs().max(dim=1).values / 127.0).double()
    assert bool(((got.cpu().double() - trained.double()).abs() <= (0.5 + 2.0 ** -10) * scale[:, None]).all())      # and it is the trained table, to half a step
    assert serve.save(str(tmp_path / "int8")) == n
    with open(tmp_path / "int8" / "meta.json") as fh:
        meta = json.load(fh)
    assert meta["extra"] == {"value_dtype": "int8"} and meta["planes"] == ["values"] and meta["format"] == checkpoint.FORMAT
    assert os.path.getsize(tmp_path / "int8" / "values.f32") == n * dim * 4          # the format is unchanged: fp32 rows
    (k1, v1), (k2, v2) = sorted_export(serve), sorted_export(twin)
    assert torch.equal(k1, k2) and torch.equal(bits32(v1), bits32(v2))
    resized = serve.resized(3000)
    assert resized.value_dtype == I8 and resized.size() == n
    assert_same_f32(resized.find(probe)[0], want, "resized")


# 9. rows past the 4 GiB mark of the plane (the pattern of tests/test_far_rows.py: a sparse table, keys chosen by their home bucket)
@pytest.mark.gpu
def test_far_rows(dev):
    """dim 1024: a row is 1040 bytes, so the plane passes 2^32 bytes at slot 4 129 776.  A sparse table of 1.09 x that many slots (4.7 GB; the
    planes are allocated, never cleared) holds 2048 keys whose home bucket lies behind the wall and 2048 below 2^31 bytes; a 16K-key batch of both
    (with duplicates and absent keys) is looked up and the table exported, and both are compared with a small fp32 twin fed D(Q(rows)).  Rows are key-derived: a
    read that wraps to a near slot returns another key's row or unwritten memory.  Skips only when 5.4 GiB + 8 GiB of HBM are not free."""
    from meepoembedding_amd import LookupTable, hash_batch
    dim, stride = 1024, 1024 + 16
    wall = (1 << 32) // stride
    capacity = int(wall * 1.09)
    need = capacity * (8 + stride) + (1 << 14) * stride + GIB
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info(dev)
    if free < need + 8 * GIB:
        pytest.skip(f"needs {need / GIB:.1f} GiB of HBM plus 8 GiB of headroom; {free / GIB:.1f} GiB are free")
    t = LookupTable(capacity, dim, device=dev, max_batch=1 << 14, default_value=0.25, int8_rows=True)
    tw = LookupTable(1 << 14, dim, device=dev, max_batch=1 << 14, default_value=0.25)
    try:
        assert t.capacity * stride > (1 << 32) and 0.90 < wall / t.capacity < 0.95 and t.table_bytes == t.capacity * (8 + stride)
        pool = synth.keys_t(9001, 0, 1 << 20, dev)
        _, bkt, _ = hash_batch(pool, t.n_buckets, 1)
        first = bkt.cpu().numpy().astype(np.int64) * 16
        pool = pool.cpu().numpy()
        far, near = pool[first >= wall][:2048], pool[(first + 16) * stride <= (1 << 31)][:2048]
        assert far.size == near.size == 2048
        keys = np.random.default_rng(1).permutation(np.concatenate([near, far]))
        rows = torch.from_numpy(synth.rows_np(keys, dim, 2).astype(np.float32))
        t.insert(K(keys, dev), rows.to(dev))
        tw.insert(K(keys, dev), DQ(rows).to(dev))
        s_far = (t.locate(K(far, dev))[0] & _lib.HANDLE_SLOT_MASK).cpu().numpy()
        s_near = (t.locate(K(near, dev))[0] & _lib.HANDLE_SLOT_MASK).cpu().numpy()
        assert int((s_far >= wall).sum()) >= 512 and int(((s_near + 1) * stride <= (1 << 31)).sum()) >= 512      # proven, not assumed
        rng = np.random.default_rng(2)
        absent = synth.keys_np(9002, 0, 512)
        u = np.concatenate([near, far])
        q = np.concatenate([u[rng.integers(0, u.size, (1 << 14) - 80 - 64)], np.repeat(far[7], 80), absent[:64]])
        rng.shuffle(q)
        qt = K(q, dev)
        ref, ref_found = tw.find(qt)
        out, found = t.find(qt)
        assert torch.equal(found, ref_found)
        assert_same_f32(out, ref, "find")
        assert_same_bf16(t.find(qt, out_dtype=BF16)[0], tw.find(qt, out_dtype=BF16)[0].cpu(), ref, "find, bf16 out")
        (k1, v1), (k2, v2) = sorted_export(t), sorted_export(tw)      # the export walks the whole plane
        assert torch.equal(k1, k2)
        assert_same_f32(v1, v2, "export")
        assert t.status() == 0
    finally:
        t.close(); tw.close()
