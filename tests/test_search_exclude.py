"""search(exclude=...) (SPEC.md §3 "Search", "Exclusion") against NumPy in float64: scores over the live rows, the excluded keys masked, sorted by
(score descending, key ascending).  Integer rows in twins under different keys: every sum is exact and every score has a tie for the key order."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
from test_search import I64_MIN, SEED, bf16
from test_search_cosine import BF16, F32, same

pytestmark = pytest.mark.gpu
I64_MAX = np.iinfo(np.int64).max


@functools.cache
def table(dev, value_dtype, dim, capacity=20_000, n=3_000, gone=300):
    """keys with negatives and INT64_MAX (all fours: every query's best); rows in twins, every other twin doubled -> (table, live keys, rows, removed keys)"""
    from meepoembedding_amd import LookupTable
    rng = np.random.default_rng(SEED + dim)
    keys = rng.permutation(np.unique(rng.integers(-2**62, 2**62, 2 * n)))[:n]
    rows = rng.integers(-2, 3, (n, dim)).astype(np.float32)
    rows[1::2] = rows[0::2]
    rows[1::4] *= 2
    keys[0], rows[0] = I64_MAX, 4
    t = LookupTable(capacity, dim, device=dev, max_batch=n, value_dtype=value_dtype)
    t.insert(torch.from_numpy(keys).to(dev), torch.from_numpy(rows).to(dev))
    t.remove(torch.from_numpy(keys[n - gone:]).to(dev))
    return t, keys[:n - gone], rows[:n - gone], keys[n - gone:]


def reference(keys, rows, queries, k, metric, exclude=None):
    q, r, f32 = bf16(queries), bf16(rows), np.float32
    scores = q @ r.T + 0.0
    if metric == "cosine":   # the contract's four float32 operations on exact sums
        scores = scores.astype(f32) / (np.sqrt((q * q).sum(1).astype(f32))[:, None] * np.sqrt((r * r).sum(1).astype(f32))[None, :]) + f32(0)
    out_k, out_s, cnt = np.full((len(q), k), I64_MIN), np.full((len(q), k), -np.inf), np.zeros(len(q), dtype=np.int32)
    for i, s in enumerate(scores):
        ok = ~np.isnan(s) & (True if exclude is None else ~np.isin(keys, exclude[i if len(exclude) > 1 else 0]))
        order = np.lexsort((keys[ok], -s[ok]))[:k]
        out_k[i, :len(order)], out_s[i, :len(order)], cnt[i] = keys[ok][order], s[ok][order], len(order)
    return out_k, out_s, cnt


def queries_of(nq, dim):
    q = np.random.default_rng(SEED + nq).integers(1, 4, (nq, dim)).astype(np.float32)   # positive: the all-fours row of INT64_MAX is every query's best
    return q, torch.from_numpy(q)


def mixed_rows(keys, rows, removed, q, metric, rows_n, ne, top):
    """[rows_n, ne]: the query's own `top` best except INT64_MAX, then removed, absent and reserved keys and duplicates, as far as ne reaches"""
    best = reference(keys, rows, q[:rows_n], min(top, ne) + 1, metric)[0]
    fill, own = np.r_[removed[:5], 2**62 + 1, -2**62 - 3, I64_MIN, I64_MIN + 1], [b[b != I64_MAX][:min(top, ne)] for b in best]
    return np.stack([np.resize(np.r_[o, fill, np.full(max(ne - len(o) - len(fill), 1), o[0])], ne) if ne > len(o) else o for o in own])


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("ne", [1, 3, 64, 4096])
@pytest.mark.parametrize("metric", ["ip", "cosine"])
@pytest.mark.parametrize("value_dtype", [F32, BF16])
@pytest.mark.parametrize("dim", [16, 64, 272])
def test_core(dev, dim, value_dtype, metric, ne, shared):
    """5 queries, k = 6, up to 40 of a query's true winners in its row: the filter bites on what would be returned; INT64_MAX is never listed and comes first"""
    t, keys, rows, removed = table(dev, value_dtype, dim)
    q, qt = queries_of(5, dim)
    ex = mixed_rows(keys, rows, removed, q, metric, 1 if shared else 5, ne, 40)
    got = t.search(qt.to(dev), 6, counts=True, metric=metric, exclude=torch.from_numpy(ex).to(dev))
    want = reference(keys, rows, q, 6, metric, ex)
    assert (want[0][:, 0] == I64_MAX).all() and not np.array_equal(want[0], reference(keys, rows, q, 6, metric)[0])
    same(got, *want)


def test_tiles_and_seed(dev):
    """Q = 70 at k = 10, dim 16, 70 000 slots: tiles of 32, 32 and 6 queries behind a seed pass; every query excludes its own top 20"""
    t, keys, rows, removed = table(dev, F32, 16, capacity=70_000)
    q, qt = queries_of(70, 16)
    ex = mixed_rows(keys, rows, removed, q, "ip", 70, 20, 20)
    assert t.capacity >= 65_536 and len({tuple(r) for r in ex}) > 60
    same(t.search(qt.to(dev), 10, counts=True, exclude=torch.from_numpy(ex).to(dev)), *reference(keys, rows, q, 10, "ip", ex))


@pytest.mark.parametrize("metric", ["ip", "cosine"])
def test_short_answers(dev, metric):
    """40 live rows, k = 8: the exclude rows leave 40, 5 and 0 candidates; the tail is INT64_MIN / -inf and the counts say so"""
    from meepoembedding_amd import LookupTable
    keys, rows = (x[:40] for x in table(dev, F32, 32)[1:3])
    t = LookupTable(1000, 32, device=dev, max_batch=64)
    t.insert(torch.from_numpy(keys).to(dev), torch.from_numpy(rows).to(dev))
    q, qt = queries_of(3, 32)
    ex = np.stack([np.full(40, 12345), np.r_[keys[:35], keys[:5]], keys])
    got = t.search(qt.to(dev), 8, counts=True, metric=metric, exclude=torch.from_numpy(ex).to(dev))
    assert got[2].tolist() == [8, 5, 0] and (got[0][2] == I64_MIN).all() and torch.isneginf(got[1][1, 5:]).all()
    same(got, *reference(keys, rows, q, 8, metric, ex))


@pytest.mark.parametrize("metric", ["ip", "cosine"])
def test_paging(dev, metric):
    """k = 32: the search that excludes page one's keys is ranks 32 .. 63 of the k = 64 search, bit for bit"""
    t, *_ = table(dev, BF16, 64)
    qt = queries_of(9, 64)[1].to(dev)
    page1 = t.search(qt, 32, metric=metric)[0]
    k2, s2 = t.search(qt, 32, metric=metric, exclude=page1)
    k64, s64 = t.search(qt, 64, metric=metric)
    assert torch.equal(k2, k64[:, 32:]) and torch.equal(s2.view(torch.int32), s64[:, 32:].contiguous().view(torch.int32))


def test_interface(dev):
    """exclude=None is the unfiltered call; a captured filtered search replays to the eager answer; every refusal comes with its code before any output"""
    from meepoembedding_amd import LookupTable, MeepoError, _lib
    t, keys, rows, removed = table(dev, F32, 64)
    q, qt = queries_of(5, 64)[0], queries_of(5, 64)[1].to(dev)
    same(t.search(qt, 6, counts=True, exclude=None), *reference(keys, rows, q, 6, "ip"))
    ex = torch.from_numpy(mixed_rows(keys, rows, removed, q, "ip", 5, 64, 40)).to(dev)
    eager = t.search(qt, 6, exclude=ex)
    ok, osc = torch.empty_like(eager[0]), torch.empty_like(eager[1])
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        t.search(qt, 6, out_keys=ok, out_scores=osc, exclude=ex)   # the workspace of the capturing stream exists before the capture
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            t.search(qt, 6, out_keys=ok, out_scores=osc, exclude=ex)
    for _ in range(3):
        ok.fill_(0), osc.fill_(0)
        g.replay()
        torch.cuda.synchronize(dev)
        assert torch.equal(ok, eager[0]) and torch.equal(osc, eager[1])
    ok.fill_(7), osc.fill_(7)
    int8 = LookupTable(1000, 64, device=dev, max_batch=64, int8_rows=True)
    i64 = lambda *shape: torch.ones(*shape, dtype=torch.int64, device=dev)   # noqa: E731
    bad = [(t, dict(exclude=i64(5, 0))), (t, dict(exclude=i64(5, 4097))), (t, dict(exclude=i64(2, 4))), (t, dict(exclude=i64(5, 4).int())),
           (t, dict(exclude=i64(5, 4).cpu())), (t, dict(exclude=i64(5, 4), metric="l2")), (int8, dict(exclude=i64(5, 4)))]
    for tab, kw in bad:
        with pytest.raises(MeepoError) as e:
            tab.search(qt, 6, out_keys=ok, out_scores=osc, **kw)
        assert e.value.code == (_lib.ERR_UNSUPPORTED if tab is int8 else _lib.ERR_INVALID_ARG)
    L, need, base, ws = _lib.lib(), C.c_uint64(), C.c_uint64(), torch.empty(1 << 22, dtype=torch.uint8, device=dev)
    args = lambda metric=0, e=ex.data_ptr(), er=5, ne=64, w=ws.data_ptr(): (t._h, metric, qt.data_ptr(), 5, 6, e, er, ne, ok.data_ptr(), osc.data_ptr(), None, w, None)   # noqa: E731
    assert L.mee_search_filtered_workspace_bytes(t._h, 0, 5, 6, 5, 64, C.byref(need)) == L.mee_search_metric_workspace_bytes(t._h, 0, 5, 6, C.byref(base)) == _lib.OK
    assert need.value == 5 * 64 * 8 + 24 + base.value <= ws.numel()   # the documented formula
    for a in [args(e=None), args(e=ex.data_ptr() + 4), args(w=None), args(w=ws.data_ptr() + 4), args(metric=2), args(ne=0), args(ne=4097), args(er=2)]:
        assert L.mee_search_filtered(*a) == _lib.ERR_INVALID_ARG
    assert L.mee_search_filtered_workspace_bytes(int8._h, 0, 5, 6, 5, 64, C.byref(need)) == _lib.ERR_UNSUPPORTED
    torch.cuda.synchronize(dev)
    assert (ok == 7).all() and (osc == 7).all()
    assert L.mee_search_filtered(*args()) == _lib.OK
    torch.cuda.synchronize(dev)
    assert torch.equal(ok, eager[0]) and torch.equal(osc, eager[1])
