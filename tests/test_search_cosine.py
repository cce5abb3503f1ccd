"""search / score with metric="cosine" (SPEC.md §3 "Search" and "Score", "Metric") against a dozen lines of NumPy: operands through bf16 to float64,
dot, rr and qq in float64 (exact on the integer data), then the contract's four operations in float32 — two square roots, a multiply, a divide."""
import numpy as np
import pytest
import torch
from test_search import I64_MIN, SEED, bf16

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16
_tables, _expected = {}, {}


def reference(keys, rows, queries, k, exact=True):
    """-> keys [Q, k], scores [Q, k], counts [Q], all scores [Q, N]; exact: the four float32 operations (the sums must be exact), else float64 throughout"""
    q, r = bf16(queries), bf16(rows)
    dot, qq, rr = q @ r.T, (q * q).sum(1), (r * r).sum(1)
    ft = np.float32 if exact else np.float64
    with np.errstate(all="ignore"):
        cos = dot.astype(ft) / (np.sqrt(qq.astype(ft))[:, None] * np.sqrt(rr.astype(ft))[None, :]) + ft(0)
    out_k, out_s, cnt = np.full((len(q), k), I64_MIN), np.full((len(q), k), -np.inf), np.zeros(len(q), dtype=np.int32)
    for i, s in enumerate(cos):
        ok = ~np.isnan(s)
        order = np.lexsort((keys[ok], -s[ok]))[:k]
        out_k[i, :len(order)], out_s[i, :len(order)], cnt[i] = keys[ok][order], s[ok][order], len(order)
    return out_k, out_s, cnt, cos


def table(dev, value_dtype, dim, kind):
    """sparse: 200 000 slots, 2 700 keys (a seed pass, mostly empty steps); small: 1 000 slots (no seed pass); dense: 300 000 slots at load 0.7;
    normal: sparse with standard-normal rows.  Negative keys, removed keys; every row has a twin under the next key — the same row, or twice it —
    whose cosine is the same in every bit -> (table, keys, rows), shared"""
    from meepoembedding_amd import LookupTable
    if (value_dtype, dim, kind) not in _tables:
        capacity, n, gone = {"small": (1_000, 600, 100), "dense": (300_000, 232_000, 22_000)}.get(kind, (200_000, 3_000, 300))
        rng = np.random.default_rng(SEED)
        keys = rng.permutation(np.unique(rng.integers(-2**62, 2**62, 2 * n)))[:n]
        rows = (rng.standard_normal((n, dim)) if kind == "normal" else rng.integers(-4, 5, (n, dim))).astype(np.float32)
        rows[1::2] = rows[0::2]
        rows[1::4] *= 2
        t = LookupTable(capacity, dim, device=dev, max_batch=n, value_dtype=value_dtype)
        t.insert(torch.from_numpy(keys).to(dev), torch.from_numpy(rows).to(dev))
        t.remove(torch.from_numpy(keys[n - gone:]).to(dev))
        assert t.size() == n - gone and (keys < 0).any()
        _tables[value_dtype, dim, kind] = t, keys[:n - gone], rows[:n - gone]
    return _tables[value_dtype, dim, kind]


def same(got, ek, es, ec):
    gk, gs, gc = (x.cpu().numpy() for x in got)
    assert np.array_equal(gk, ek) and np.array_equal(gc, ec)
    assert np.array_equal(gs.view(np.uint32), es.astype(np.float32).view(np.uint32))


CASES = [(vd, kind, dim, nq, k) for vd in (F32, BF16) for kind in ("sparse", "small") for dim in (16, 48, 256) for nq, k in [(1, 1), (33, 9), (70, 63)]]
CASES += [(F32, "dense", 16, 3, 1), (F32, "dense", 16, 34, 9)]   # thresholds at work: every block's buffers fill and prune with risen thresholds


@pytest.mark.parametrize("value_dtype,kind,dim,nq,k", CASES)
def test_bit_for_bit(dev, value_dtype, kind, dim, nq, k):
    """integers in [-4, 4] (twins twice that): the three sums are exact, so keys, score bits and counts are the reference's; k is odd and every
    score comes in pairs, so a tie crosses the k-th place for every query"""
    t, keys, rows = table(dev, value_dtype, dim, kind)
    queries = np.random.default_rng(SEED + nq).integers(-4, 5, (nq, dim)).astype(np.float32)
    if (kind, dim, nq, k) not in _expected:
        ek, es, ec, cos = reference(keys, rows, queries, k)
        kth = -np.partition(-cos, (k - 1, k), axis=1)[:, k - 1:k + 1]
        assert (kth[:, 0] == kth[:, 1]).all() and (ec == k).all(), "no tie across the k-th place"
        _expected[kind, dim, nq, k] = ek, es, ec
    same(t.search(torch.from_numpy(queries).to(dev), k, counts=True, metric="cosine"), *_expected[kind, dim, nq, k])


def test_signs_and_zeros(dev):
    """non-negative rows; an all-negative query (every threshold negative), a query orthogonal to all rows but one (scores of +0.0), a zero query
    (count 0, all padding); two zero rows and a NaN row are never returned, 6 candidates are fewer than k = 8.  A row scaled by 2^55 and a query
    by 2^-55 have norms outside the range the product compare is argued for; the cosine does not move by a bit"""
    from meepoembedding_amd import LookupTable
    dim, k = 32, 8
    keys = np.array([7, -3, 11, 5, -9, 2, 40, -41, 13])
    rows = np.zeros((9, dim), dtype=np.float32)
    rows[:6, :16] = np.random.default_rng(SEED).integers(0, 5, (6, 16)) + np.eye(6, 16)
    rows[5, 20], rows[8, 3], rows[4] = 3, np.nan, rows[4] * 2.0**55   # row 5 alone is not orthogonal to query 1; rows 6 and 7 stay zero
    queries = np.zeros((3, dim), dtype=np.float32)
    queries[0], queries[1, 16:] = -np.arange(1, dim + 1), 2.0**-55
    t = LookupTable(1000, dim, device=dev, max_batch=64)
    t.insert(torch.from_numpy(keys).to(dev), torch.from_numpy(rows).to(dev))
    ek, es, ec, _ = reference(keys, rows, queries, k)
    assert ec.tolist() == [6, 6, 0] and (es[0, :6] < 0).all() and (es[1, 1:6] == 0).all() and es[1, 0] > 0
    same(t.search(torch.from_numpy(queries).to(dev), k, counts=True, metric="cosine"), ek, es, ec)
    same(t.search(torch.from_numpy(queries).to(dev), 1, counts=True, metric="cosine"), ek[:, :1], es[:, :1], np.minimum(ec, 1))
    sc, found = t.score(torch.from_numpy(queries).to(dev), torch.from_numpy(np.tile(keys[[0, 6, 8]], (3, 1))).to(dev), metric="cosine")
    assert found.all() and torch.isnan(sc[:, 1:]).all() and torch.isnan(sc[2]).all() and not torch.isnan(sc[:2, 0]).any()   # a zero row, a NaN row, a zero query


@pytest.mark.parametrize("dim", [64, 256])
@pytest.mark.parametrize("value_dtype", [F32, BF16])
def test_general_values(dev, value_dtype, dim):
    """standard-normal operands: every returned score, and score()'s of the same keys, within the contract's bound of that key's float64 cosine —
    (dim - 1) 2^-24 sum |products| / (|q| |row|) + (dim + 4) 2^-24 |cos| — and the set bound as tests/test_search.py::test_general_values states it"""
    t, keys, rows = table(dev, value_dtype, dim, "normal")
    nq, k = 40, 16
    queries = np.random.default_rng(SEED + 1).standard_normal((nq, dim)).astype(np.float32)
    ek, es, _, cos = reference(keys, rows, queries, k, exact=False)
    q, r = bf16(queries), bf16(rows)
    den = np.sqrt((q * q).sum(1))[:, None] * np.sqrt((r * r).sum(1))[None, :]
    bound = (dim - 1) * 2.0**-24 * (np.abs(q) @ np.abs(r).T) / den + (dim + 4) * 2.0**-24 * np.abs(cos)
    qt = torch.from_numpy(queries).to(dev)
    gk_t, gs_t = t.search(qt, k, metric="cosine")
    gk, gs, rs = gk_t.cpu().numpy(), gs_t.cpu().numpy(), t.score(qt, gk_t, metric="cosine")[0].cpu().numpy()
    pos = {int(key): i for i, key in enumerate(keys)}
    for i in range(nq):
        at = [pos[int(key)] for key in gk[i]]   # (a key that is not in the table fails here)
        assert len(set(at)) == k and (np.diff(gs[i]) <= 0).all()
        assert (np.abs(gs[i].astype(np.float64) - cos[i, at]) <= bound[i, at]).all() and (np.abs(rs[i].astype(np.float64) - cos[i, at]) <= bound[i, at]).all()
        assert (cos[i, at] >= es[i, k - 1] - bound[i, at] - bound[i, [pos[int(key)] for key in ek[i]]].max()).all()


@pytest.mark.parametrize("dim", [16, 48, 80, 256])
@pytest.mark.parametrize("value_dtype", [F32, BF16])
def test_score(dev, value_dtype, dim):
    """score of search's own keys is search's score bit for bit, the padded tail included; absent and removed keys: -inf, found 0"""
    from meepoembedding_amd import LookupTable
    rng = np.random.default_rng(SEED + dim)
    keys, rows = rng.permutation(np.arange(-30, 30))[:50], rng.integers(-4, 5, (50, dim)).astype(np.float32)
    t = LookupTable(1000, dim, device=dev, max_batch=64, value_dtype=value_dtype)
    t.insert(torch.from_numpy(keys).to(dev), torch.from_numpy(rows).to(dev))
    t.remove(torch.from_numpy(keys[40:]).to(dev))
    queries = torch.from_numpy(rng.integers(-4, 5, (5, dim)).astype(np.float32)).to(dev)
    gk, gs, gc = t.search(queries, 64, counts=True, metric="cosine")
    same((gk, gs, gc), *reference(keys[:40], rows[:40], queries.cpu().numpy(), 64)[:3])
    sc, found = t.score(queries, gk, metric="cosine")
    assert (gc == 40).all() and torch.equal(sc.view(torch.int32), gs.view(torch.int32)) and torch.equal(found, (gk != I64_MIN).to(torch.uint8))
    sc, found = t.score(queries, torch.from_numpy(np.tile(np.r_[keys[40:], 1000], (5, 1))).to(dev), metric="cosine")
    assert torch.isneginf(sc).all() and not found.any()


def test_interface(dev):
    from meepoembedding_amd import LookupTable, MeepoError
    t, keys, _ = table(dev, F32, 16, "small")
    q = torch.from_numpy(np.random.default_rng(SEED).integers(-4, 5, (70, 16)).astype(np.float32)).to(dev)
    for nq in (3, 70):   # one mee_search call, and the batched route
        assert all(torch.equal(a, b) for a, b in zip(t.search(q[:nq], 9, counts=True, metric="ip"), t.search(q[:nq], 9, counts=True)))
    slate = torch.from_numpy(np.tile(keys[:20], (70, 1))).to(dev)
    assert all(torch.equal(a, b) for a, b in zip(t.score(q, slate, metric="ip"), t.score(q, slate)))
    int8 = LookupTable(1000, 16, device=dev, max_batch=64, int8_rows=True)
    for tab, k, metric in [(t, 9, "l2"), (t, 9, 1), (int8, 9, "cosine"), (t, 0, "cosine"), (t, 65, "cosine"), (t, None, "l2"), (int8, None, "cosine")]:
        with pytest.raises(MeepoError):   # k None: score
            tab.score(q, slate, metric=metric) if k is None else tab.search(q, k, metric=metric)
    torch.cuda.synchronize(dev)
    assert t.find(torch.from_numpy(keys[:5]).to(dev))[1].all()


def test_graph_replay(dev):
    """search(metric="cosine") captured in a graph and replayed gives the eager result every time — nothing in the call synchronises"""
    t, _, _ = table(dev, F32, 48, "sparse")
    nq, k = 70, 9
    queries = torch.from_numpy(np.random.default_rng(SEED + nq).integers(-4, 5, (nq, 48)).astype(np.float32)).to(dev)
    out = [torch.zeros(nq, k, dtype=torch.int64, device=dev), torch.zeros(nq, k, device=dev)]
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        eager = t.search(queries, k, metric="cosine")   # (also the warm-up: the stream's workspace exists before the capture)
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            t.search(queries, k, out_keys=out[0], out_scores=out[1], metric="cosine")
    for _ in range(3):
        out[0].zero_(), out[1].zero_()
        graph.replay()
        torch.cuda.synchronize(dev)
        assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1])
