"""bf16-row table groups (SPEC.md §3 "Row storage type"): a TableGroup / mee_group whose members are ALL bf16-row tables, the serving form of a collection.

By definition each lookup of such a group is, bit for bit, the per-member lookup of the bf16-row tables, and therefore the fp32 group over the members'
fp32 twins (tables handed bf16(values), created with bf16(default_value)).  Every GPU case compares against BOTH: (i) the fp32 TableGroup over the
twins, fed rows.to(bfloat16).float() computed on the CPU, whole result buffers including what lies outside the segments; (ii) LookupTable.find /
find_pooled of each bf16-row member.  No tolerance anywhere, NaN positions compared with isnan; every result buffer is followed by two guard rows of
a sentinel.  CPU half: the new symbol, _lib.group_row_dtype, the constructor's check before any device is needed."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

from meepoembedding_amd import _lib, synth
from meepoembedding_amd._lib import MeepoError

BF16 = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT_F32, SENT_BF16, SENT_U8 = -777.25, -768.0, 0xAB   # guard values behind every result buffer (both exact in their type)
CAPS = (1000, 5000, 20000)          # requested slots: three different bucket counts, so a descriptor mix-up shows
DEFAULTS = (0.0, 0.3, -1.7)         # each member's own default row (0.3 and -1.7 are no bf16 values: the default row is the rounded one)
BPT = 5                             # bags per table: no multiple of 4, so one wave's four bags straddle two members


# ---- helpers (as in tests/test_bf16_rows.py) ------------------------------------------------------------------------------
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


def assert_same_bf16(got, ref, what=""):
    """two bf16 tensors, bit for bit; NaN positions: both NaN"""
    got, ref = got.detach().cpu(), ref.detach().cpu()
    assert got.dtype == ref.dtype == BF16 and got.shape == ref.shape, (what, got.dtype, ref.dtype, got.shape, ref.shape)
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan), what
    bad = int((bits16(got)[~nan] != bits16(ref)[~nan]).sum())
    assert bad == 0, f"{what}: {bad} of {got.numel()} bf16 patterns differ"


def assert_same(got, ref, what=""):
    (assert_same_bf16 if ref.dtype == BF16 else assert_same_f32)(got, ref, what)


def K(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def rows_for(keys_np, dim, seed):
    """rows with full fp32 mantissas spread over nine binades (a function of the key): the order of a bag's additions and the one rounding matter"""
    r = synth.rows_np(keys_np, dim, seed).astype(np.float32) * np.float32(1.37)
    scale = np.exp2(((keys_np.view(np.uint64) >> np.uint64(7)) % np.uint64(9)).astype(np.float32) - 4.0).astype(np.float32)
    return torch.from_numpy(r * scale[:, None])


def guarded(n, dim, dtype, dev):
    """a result buffer of n rows with two guard rows of a sentinel behind it -> (whole buffer, the n-row view handed to the lookup).  The n rows
    hold the sentinel too: what a lookup leaves unwritten is compared as well."""
    buf = torch.full((n + 2, dim), SENT_BF16 if dtype == BF16 else SENT_F32, dtype=dtype, device=dev)
    return buf, buf[:n]


def guards_intact(buf, n):
    sent = SENT_BF16 if buf.dtype == BF16 else SENT_F32
    return bool((buf[n:].float() == sent).all())


def found_buf(n, dev):
    return torch.full((n,), SENT_U8, dtype=torch.uint8, device=dev)


def sorted_export(t, with_state=False):
    """(keys, rows[, state planes that exist]) in key order, on the CPU"""
    k, *planes = t.export(with_state=with_state)
    o = torch.argsort(k)
    return (k[o].cpu(), *[p[o].cpu() for p in planes if p is not None])


# ---- the members: three bf16-row tables and their fp32 twins, built once per (dim, empty) and never changed afterwards ------------
POOL = synth.keys_np(41, 0, 40000)
STORED = (POOL[0:912], POOL[1000:3600], POOL[4000:7000])    # member 0: 912 of 1072 slots = 0.85 (probes go past the home bucket)
REMOVED = POOL[1000:1400]                                     # removed from member 1 again: tombstones on its probe paths
ABSENT = POOL[20000:40000]
_built = {}


def build_members(dev, dim, empty_last=False):
    from meepoembedding_amd import LookupTable
    bf, tw = [], []
    for j, (cap, dv) in enumerate(zip(CAPS, DEFAULTS)):
        t = LookupTable(cap, dim, device=dev, max_batch=4096, default_value=dv, value_dtype=BF16)
        w = LookupTable(cap, dim, device=dev, max_batch=4096, default_value=float(rnd(torch.tensor(dv))))
        assert t.capacity == w.capacity
        if not (empty_last and j == 2):
            rows = rows_for(STORED[j], dim, 5 + j)
            for s in range(0, len(STORED[j]), 4096):
                k = K(STORED[j][s:s + 4096], dev)
                t.insert(k, rows[s:s + 4096].to(dev))
                w.insert(k, rnd(rows[s:s + 4096]).to(dev))
        if j == 1:
            assert bool(t.remove(K(REMOVED, dev)).all()) and bool(w.remove(K(REMOVED, dev)).all())
        assert t.size() == w.size() and t.status() == w.status() == 0
        bf.append(t)
        tw.append(w)
    assert len({t.n_buckets for t in bf}) == 3 and bf[0].size() / bf[0].capacity >= 0.85
    return bf, tw


def members(dev, dim, empty_last=False):
    from meepoembedding_amd import TableGroup
    key = (dim, empty_last)
    if key not in _built:
        bf, tw = build_members(dev, dim, empty_last)
        _built[key] = (TableGroup(bf), TableGroup(tw), bf, tw)
    return _built[key]


def draw(rng, j, n):
    """n keys for member j's segment: two thirds stored there (removed ones among them for member 1), a third absent everywhere"""
    return np.where(rng.random(n) < 0.67, rng.choice(STORED[j], n), rng.choice(ABSENT, n))


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_group_value_dtype_symbol(built):
    """fails on the parent commit: the entry point does not exist there"""
    with open(os.path.join(ROOT, "include", "meepo_embedding.h")) as f:
        header = f.read()
    L = C.CDLL(_lib.LIB_PATH)
    assert "mee_group_value_dtype" in _lib.PROTOTYPES and hasattr(L, "mee_group_value_dtype") and "mee_group_value_dtype(" in header
    assert "#define MEE_ABI_VERSION 2 " in header
    assert _lib.lib().mee_abi_version() == 2 and _lib.ABI_VERSION == 2
    assert C.sizeof(_lib.Config) == 64 and C.sizeof(_lib.TableInfo) == 48 and C.sizeof(_lib.FindRequest) == 32   # additive: nothing pinned moved


def test_group_row_dtype():
    """fails on the parent commit: the helper does not exist there"""
    b = types.SimpleNamespace(value_dtype=BF16, dim=64)
    f = types.SimpleNamespace(value_dtype=torch.float32, dim=64)
    plain = types.SimpleNamespace(dim=64)                      # no attribute: fp32
    assert _lib.group_row_dtype("TableGroup", b, b) == BF16
    assert _lib.group_row_dtype("TableGroup", b) == BF16
    assert _lib.group_row_dtype("TableGroup", f, f) == torch.float32
    assert _lib.group_row_dtype("TableGroup", f, plain) == torch.float32
    for mix in ([f, b], [b, f], [b, b, plain]):
        with pytest.raises(MeepoError, match="bf16-row table") as e:
            _lib.group_row_dtype("TableGroup", *mix)
        assert e.value.code == _lib.ERR_UNSUPPORTED and "TableGroup" in str(e.value)


def test_serving_group_has_no_apply_batch():
    """TableGroup([b, b], max_apply_batch=16) is refused before a device (or a table handle) is needed; a mixed list likewise"""
    from meepoembedding_amd import TableGroup
    b = types.SimpleNamespace(value_dtype=BF16, dim=64)        # anything else it lacks: nobody may get that far
    f = types.SimpleNamespace(value_dtype=torch.float32, dim=64)
    with pytest.raises(ValueError, match="max_apply_batch"):
        TableGroup([b, b], max_apply_batch=16)
    for mix in ([f, b], [b, f]):
        with pytest.raises(MeepoError, match="bf16-row table") as e:
            TableGroup(mix)
        assert e.value.code == _lib.ERR_UNSUPPORTED


# ---- GPU ----------------------------------------------------------------------------------------------------------------
# 1. grouped find
@pytest.mark.gpu
@pytest.mark.parametrize("dim,empty_last", [(64, False), (128, False), (8, True), (200, False)])
def test_grouped_find(dev, dim, empty_last):
    g, gw, bf, tw = members(dev, dim, empty_last)
    assert g.value_dtype == BF16 and gw.value_dtype == torch.float32
    d = C.c_uint32(99)
    assert _lib.lib().mee_group_value_dtype(g._h, C.byref(d)) == 0 and d.value == _lib.DTYPE_BF16
    assert _lib.lib().mee_group_value_dtype(gw._h, C.byref(d)) == 0 and d.value == _lib.DTYPE_F32
    rng = np.random.default_rng(dim)
    n = 611                                                    # no multiple of 4 R; positions [0, 5) and [600, 611) lie outside every segment
    for bounds in ([5, 205, 405, 600], [5, 205, 205, 600], [5, 5, 330, 600]):    # all three served; member 1's segment empty; member 0's empty
        batch = rng.choice(ABSENT, n)
        for j in range(3):
            a, b = bounds[j], bounds[j + 1]
            batch[a:b] = draw(rng, j, b - a)
        batch[0], batch[603] = STORED[0][0], STORED[2][0]      # stored keys outside the segments
        batch[210], batch[211] = _lib.EMPTY_KEY, _lib.RECLAIMED_KEY
        batch[450], batch[599] = _lib.RECLAIMED_KEY, _lib.EMPTY_KEY
        batch[220] = STORED[0][3]                              # stored in member 0, asked of another member: a miss
        batch[221] = STORED[0][4]
        k, o = K(batch, dev), K(np.array(bounds, dtype=np.int64), dev)
        miss_at = 220 if bounds[1] <= 220 < bounds[3] else None
        for out_dtype in (torch.float32, BF16):
            what = f"dim {dim} bounds {bounds} {out_dtype}"
            rbuf, rout = guarded(n, dim, out_dtype, dev)
            rfound = found_buf(n, dev)
            gw.find(k, o, out=rout, found=rfound, out_dtype=out_dtype)
            buf, out = guarded(n, dim, out_dtype, dev)
            found = found_buf(n, dev)
            g.find(k, o, out=out, found=found, out_dtype=out_dtype)
            assert_same(buf, rbuf, what + ": (i) the twin group's buffer, guards and untouched rows included")
            assert torch.equal(found, rfound), what
            assert guards_intact(buf, n), what
            if miss_at is not None:
                assert int(found[miss_at]) == 0 and int(found[miss_at + 1]) == 0, what
            for j in range(3):                                 # (ii) the members' own finds
                a, b = bounds[j], bounds[j + 1]
                if a == b:
                    continue
                mo, mf = bf[j].find(k[a:b], out_dtype=out_dtype)
                assert_same(out[a:b], mo, what + f": (ii) member {j}")
                assert torch.equal(found[a:b], mf), what
            assert 0 < int(found[5:600].sum()) < 595
        for t, w in zip(bf, tw):
            assert t.status() == w.status()


# 2. pooled lookups
def pooled_batch(rng, lengths):
    """15 bags (BPT per member) -> (keys, offsets): the last offset lies beyond n (clamped to n) and one pair decreases (an empty bag)"""
    assert len(lengths) == 3 * BPT
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    n = int(off[-1])
    batch = np.empty(n, dtype=np.int64)
    for j in range(3):
        a, b = int(off[j * BPT]), int(off[(j + 1) * BPT])
        batch[a:b] = draw(rng, j, b - a)
    batch[3], batch[n - 9], batch[n // 2] = _lib.EMPTY_KEY, _lib.RECLAIMED_KEY, _lib.EMPTY_KEY
    off[-1] = n + 7                    # beyond the key array
    off[12] = off[11] - 2              # bag 11 = [off[11], off[11] - 2): a decreasing pair
    return batch, off, n


LENGTHS = {"tile per bag": [0, 1, 2, 15, 16, 17, 40, 3, 1, 2, 5, 0, 7, 16, 4],          # mean < 12: four bags per wave; both sides of kPoolLong = 16
           "wave per bag": [40, 33, 64, 1, 0, 20, 16, 17, 30, 12, 25, 15, 13, 50, 18]}    # mean >= 12


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [8, 64, 128, 200, 1024])
def test_pooled(dev, dim):
    g, gw, bf, tw = members(dev, dim)
    rng = np.random.default_rng(1000 + dim)
    for name, lengths in LENGTHS.items():
        batch, off, n = pooled_batch(rng, lengths)
        n_bags = len(off) - 1
        assert (n // n_bags >= 12) == (name == "wave per bag")
        k, o = K(batch, dev), K(off, dev)
        for mode in ("sum", "mean"):
            for out_dtype in (torch.float32, BF16):
                what = f"dim {dim} {name} {mode} {out_dtype}"
                rbuf, rout = guarded(n_bags, dim, out_dtype, dev)
                rfound = found_buf(n, dev)
                gw.find_pooled(k, o, mode=mode, out=rout, found=rfound, out_dtype=out_dtype)
                buf, out = guarded(n_bags, dim, out_dtype, dev)
                found = found_buf(n, dev)
                g.find_pooled(k, o, mode=mode, out=out, found=found, out_dtype=out_dtype)
                assert_same(buf, rbuf, what + ": (i) the twin group")
                assert torch.equal(found, rfound), what
                assert guards_intact(buf, n_bags), what
                for j in range(3):                             # (ii) the members' own pooled lookups over the same key array and offsets
                    mo, _ = bf[j].find_pooled(k, o[j * BPT:(j + 1) * BPT + 1].contiguous(), mode=mode, out_dtype=out_dtype)
                    assert_same(out[j * BPT:(j + 1) * BPT], mo, what + f": (ii) member {j}")
        assert float(out.float().abs().max()) > 0


# 3. the jagged bag -> member map
@pytest.mark.gpu
@pytest.mark.parametrize("dim", [8, 64, 128, 200])
def test_pooled_jagged(dev, dim):
    g, gw, bf, tw = members(dev, dim)
    rng = np.random.default_rng(2000 + dim)
    member_bags = np.array([2, 6, 6, 13], dtype=np.int64)      # member 1 has no bags; bags 0, 1, 13 and 14 lie outside the map
    for name, lengths in LENGTHS.items():
        off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        n = int(off[-1])
        batch = rng.choice(ABSENT, n)
        for j in (0, 2):
            a, b = int(off[member_bags[j]]), int(off[member_bags[j + 1]])
            batch[a:b] = draw(rng, j, b - a)
        batch[int(off[3])], batch[int(off[8])] = _lib.EMPTY_KEY, _lib.RECLAIMED_KEY
        k, o, mb = K(batch, dev), K(off, dev), K(member_bags, dev)
        n_bags = len(off) - 1
        for mode in ("sum", "mean"):
            what = f"dim {dim} {name} {mode}"
            rbuf, rout = guarded(n_bags, dim, torch.float32, dev)
            rfound = found_buf(n, dev)
            gw.find_pooled_jagged(k, o, mb, mode=mode, out=rout, found=rfound)
            buf, out = guarded(n_bags, dim, torch.float32, dev)
            found = found_buf(n, dev)
            g.find_pooled_jagged(k, o, mb, mode=mode, out=out, found=found)
            assert_same_f32(buf, rbuf, what + ": (i) the twin group")
            assert torch.equal(found, rfound), what
            assert guards_intact(buf, n_bags), what
            for j in (0, 2):
                a, b = int(member_bags[j]), int(member_bags[j + 1])
                mo, _ = bf[j].find_pooled(k, o[a:b + 1].contiguous(), mode=mode)
                assert_same_f32(out[a:b], mo, what + f": (ii) member {j}")
            assert not bool(out[:2].any()) and not bool(out[13:].any()), what      # bags outside the map: rows of zeros


# 4. reserve on a member between two lookups
@pytest.mark.gpu
def test_reserve_between_lookups(dev):
    from meepoembedding_amd import TableGroup
    dim = 64
    bf, tw = build_members(dev, dim)                           # its own members: this test moves planes
    g, gw = TableGroup(bf), TableGroup(tw)
    rng = np.random.default_rng(5)
    batch, off, n = pooled_batch(rng, LENGTHS["tile per bag"])
    k, o = K(batch, dev), K(off, dev)
    seg = K(np.array([off[0], off[BPT], off[2 * BPT], n], dtype=np.int64), dev)

    def compare(what):
        for out_dtype in (torch.float32, BF16):
            assert_same(g.find_pooled(k, o, mode="mean", out_dtype=out_dtype)[0], gw.find_pooled(k, o, mode="mean", out_dtype=out_dtype)[0], what)
            (a, fa), (b, fb) = g.find(k, seg, out_dtype=out_dtype), gw.find(k, seg, out_dtype=out_dtype)
            assert_same(a, b, what)
            assert torch.equal(fa, fb), what

    compare("before reserve")
    for cap in (9000, 3000):
        bf[1].reserve(cap)
        tw[1].reserve(cap)
        assert bf[1].capacity == tw[1].capacity and bf[1].table_bytes == bf[1].capacity * (8 + 2 * dim)
        compare(f"after reserve({cap})")
    bf[0].reserve(4000)
    tw[0].reserve(4000)
    compare("after reserve on member 0")
    assert_same_f32(g.find(k, seg)[0][:int(off[BPT])], bf[0].find(k[:int(off[BPT])])[0], "member 0 after its reserve")


# 5. refusals
_REFUSED = ["mee_group_find_or_insert", "mee_group_find_or_insert_as", "mee_group_apply_adagrad", "mee_group_apply_adam", "mee_group_apply_adagrad_pooled",
            "mee_group_apply_adam_pooled", "mee_group_apply_adagrad_indexed", "mee_group_apply_adam_indexed", "mee_group_find_pooled_weighted",
            "mee_group_pooled_weighted_backward",
            "mee_group_find_pooled_as",          # every pointer non-null: d_weights
            "mee_group_find_pooled", "mee_group_find_pooled_jagged"]   # every pointer non-null: d_located_out


@pytest.mark.gpu
def test_refusals(dev):
    """Every operator a bf16-row group does not have: MEE_ERR_UNSUPPORTED, a message that starts with the operator's name and names the bf16-row table,
    and not one byte written.  The calls are made on the C-ABI with arguments built from the prototypes: every pointer argument is a device buffer
    of its own, pre-filled with a sentinel (a call that was NOT refused would find valid memory), every count is 4."""
    from meepoembedding_amd import LookupTable, MixedTableGroup, TableGroup
    L, dim, n = _lib.lib(), 64, 4
    t = LookupTable(1000, dim, device=dev, max_batch=64, value_dtype=BF16)
    t2 = LookupTable(2000, dim, device=dev, max_batch=64, value_dtype=BF16)
    f = LookupTable(1000, dim, device=dev, max_batch=64)
    keys = K(synth.keys_np(8, 0, n), dev)
    t.insert(keys, torch.ones(n, dim, device=dev))
    t2.insert(keys, torch.full((n, dim), 2.0, device=dev))
    g = TableGroup([t, t2])
    before = [sorted_export(x) for x in (t, t2)]
    bufs = []

    def args_for(name, handle, null_at=()):
        res, argtypes = _lib.PROTOTYPES[name]
        out = []
        for i, a in enumerate(argtypes):
            if i == len(argtypes) - 1 or i in null_at:
                out.append(None)                                   # the stream; an argument left out on purpose
            elif i == 0:
                out.append(handle)
            elif a is C.c_void_p:
                b = torch.full((1 << 14,), SENT_U8, dtype=torch.uint8, device=dev)
                bufs.append(b)
                out.append(b.data_ptr())
            elif a is C.c_size_t:
                out.append(n)
            elif a in (C.c_uint64, C.c_int, C.c_uint32):
                out.append(1 if a is C.c_uint64 else 0)            # step 1, MEE_DTYPE_F32, MEE_POOL_SUM
            elif a is C.c_float:
                out.append(0.5)
            else:
                raise AssertionError((name, a))
        return out

    def refused(name, rc):
        msg = L.mee_last_error().decode()
        assert rc == _lib.ERR_UNSUPPORTED, (name, rc, msg)
        assert msg.startswith(name + ":") and "bf16-row table" in msg, (name, msg)     # the operator that was called, by its exact name

    for name in _REFUSED:
        refused(name, getattr(L, name)(*args_for(name, g._h)))
    refused("mee_group_find_pooled_as", L.mee_group_find_pooled_as(*args_for("mee_group_find_pooled_as", g._h, null_at=(5,))))   # no weights: d_located_out alone
    rc = L.mee_group_set_tuning(g._h, b"apply_kernel", 0)
    assert rc == _lib.ERR_UNSUPPORTED                               # as for any group without an apply
    # creation
    h = C.c_void_p()
    for pair in ((f._h, t._h), (t._h, f._h)):
        refused("mee_group_create", L.mee_group_create((C.c_void_p * 2)(*pair), 2, 0, C.byref(h)))
        assert not h.value
    arr = (C.c_void_p * 2)(t._h, t2._h)
    assert L.mee_group_create(arr, 2, 8, C.byref(h)) == _lib.ERR_INVALID_ARG and not h.value
    assert L.mee_last_error().decode().startswith("mee_group_create:") and "max_apply_batch" in L.mee_last_error().decode()
    refused("mee_mixed_group_create", L.mee_mixed_group_create(arr, 2, 0, C.byref(h)))
    assert not h.value
    with pytest.raises(MeepoError, match="bf16-row table"):
        MixedTableGroup([t, t2])
    torch.cuda.synchronize(dev)
    for b in bufs:
        assert bool((b == SENT_U8).all())
    for x, (bk, bv) in zip((t, t2), before):
        ak, av = sorted_export(x)
        assert torch.equal(bk, ak) and torch.equal(bits32(bv), bits32(av)) and x.status() == 0
    assert f.size() == 0
    # the Python methods surface the same error
    off = K(np.array([0, 2, n], dtype=np.int64), dev)
    ones, grads = torch.ones(n, device=dev), torch.zeros(n, dim, device=dev)
    idx, loc = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int64, device=dev)
    calls = [lambda: g.find_or_insert(keys, off), lambda: g.find_or_insert(keys, off, out_dtype=BF16), lambda: g.apply_adagrad(keys, off, grads, lr=0.1),
             lambda: g.apply_adam(keys, off, grads, lr=0.1), lambda: g.apply_pooled(keys, off, grads[:2], idx, "adagrad", lr=0.1),
             lambda: g.apply_pooled(keys, off, grads[:2], idx, "adam", lr=0.1), lambda: g.apply_indexed(keys, off, grads, idx, "adagrad", lr=0.1),
             lambda: g.apply_indexed(keys, off, grads, idx, "adam", lr=0.1), lambda: g.pooled_weighted_backward(keys, off, ones, grads[:2]),
             lambda: g.find_pooled(keys, off, weights=ones), lambda: g.find_pooled(keys, off, weights=ones, out_dtype=BF16),
             lambda: g.find_pooled(keys, off, located=loc), lambda: g.find_pooled(keys, off, located=loc, out_dtype=BF16),
             lambda: g.find_pooled_jagged(keys, off, off, located=loc)]
    for i, call in enumerate(calls):
        with pytest.raises(MeepoError, match="bf16-row table") as e:
            call()
        assert e.value.code == _lib.ERR_UNSUPPORTED, i
    assert bool((loc == 0).all())
    out, found = g.find_pooled(keys, off)                           # and what it has still works
    assert_same_f32(out, torch.tensor([[2.0] * dim, [4.0] * dim]), "the serving lookups after the refusals")


# 6. train -> serve in memory
@pytest.mark.gpu
def test_serving_copy(dev):
    from meepoembedding_amd import OPT_ADAGRAD, LookupTable, TableGroup
    dim = 64
    src, tw = [], []
    for j, (cap, dv) in enumerate(zip((1000, 3000, 6000), DEFAULTS)):
        s = LookupTable(cap, dim, device=dev, optimizer=OPT_ADAGRAD, max_batch=2048, default_value=dv, initial_accumulator=0.1)
        w = LookupTable(cap, dim, device=dev, max_batch=2048, default_value=float(rnd(torch.tensor(dv))))
        keys = STORED[j][:800 + 700 * j]
        rows = rows_for(keys, dim, 70 + j)
        for a in range(0, len(keys), 2048):
            s.insert(K(keys[a:a + 2048], dev), rows[a:a + 2048].to(dev))
            w.insert(K(keys[a:a + 2048], dev), rnd(rows[a:a + 2048]).to(dev))
        src.append(s)
        tw.append(w)
    train, twins = TableGroup(src, max_apply_batch=1024), TableGroup(tw)
    before = [sorted_export(s, with_state=True) for s in src]
    serve = train.serving_copy(chunk=700)                         # several export pieces per member
    assert serve.value_dtype == BF16 and train.value_dtype == torch.float32 and len(serve.tables) == 3
    for s, c in zip(src, serve.tables):
        assert c.value_dtype == BF16 and c.capacity == s.capacity and c.size() == s.size() and c.status() == 0 and c.optimizer == _lib.OPT_NONE
        assert c.table_bytes == c.capacity * (8 + 2 * dim) and c.device == s.device and c is not s
    rng = np.random.default_rng(6)
    for name, lengths in LENGTHS.items():
        batch, off, n = pooled_batch(rng, lengths)
        k, o = K(batch, dev), K(off, dev)
        for mode in ("sum", "mean"):
            for out_dtype in (torch.float32, BF16):
                (a, fa), (b, fb) = serve.find_pooled(k, o, mode=mode, out_dtype=out_dtype), twins.find_pooled(k, o, mode=mode, out_dtype=out_dtype)
                assert_same(a, b, f"{name} {mode} {out_dtype}")
                assert torch.equal(fa, fb) and 0 < int(fa.sum()) < n
    for s, b4 in zip(src, before):                                # the source group is untouched: keys, rows and accumulators
        af = sorted_export(s, with_state=True)
        assert len(af) == len(b4) == 3 and torch.equal(af[0], b4[0]) and all(torch.equal(bits32(x), bits32(y)) for x, y in zip(af[1:], b4[1:]))
    assert train.tables[0].status() == 0
    odd = TableGroup([LookupTable(100, 12, device=dev, max_batch=64)])
    with pytest.raises(ValueError, match="multiple of 8"):
        odd.serving_copy()
