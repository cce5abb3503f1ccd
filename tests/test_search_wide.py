"""search and score at row widths 272 .. 1024 (SPEC.md §3 "Search", "Score", "Metric"; DESIGN.md §4 "Wide rows") against the references of
tests/test_search.py and tests/test_search_cosine.py: operands through bf16 to float64, exact on the integer data."""
import ctypes as C

import numpy as np
import pytest
import torch
from test_search import I64_MIN, SEED, bf16, reference
from test_search_cosine import reference as cosine_reference

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16
REFERENCE = {"ip": reference, "cosine": cosine_reference}
_tables, _expected = {}, {}


def table(dev, value_dtype, dim, kind="sparse"):
    """sparse: 20 000 slots, 3 000 keys, the last 300 removed again; dense: 200 000 slots, 141 000 keys, 3 000 removed (load 0.69); normal: sparse with
    standard-normal rows.  Negative keys among them.  Integer rows come in TRIPLES of identical rows under consecutive keys of the list (whole triples
    are removed), so every query's scores come in threes and ranks k and k + 1 tie whenever k % 3 != 0 -> (table, live keys, live rows, removed keys)"""
    from meepoembedding_amd import LookupTable
    if (value_dtype, dim, kind) not in _tables:
        capacity, n, gone = (200_000, 141_000, 3_000) if kind == "dense" else (20_000, 3_000, 300)
        rng = np.random.default_rng(SEED + dim)
        keys = rng.permutation(np.unique(rng.integers(-2**62, 2**62, 2 * n)))[:n]
        rows = (rng.standard_normal((n, dim)) if kind == "normal" else rng.integers(-4, 5, (n, dim))).astype(np.float32)
        if kind != "normal":
            rows[1::3], rows[2::3] = rows[0::3], rows[0::3]
        t = LookupTable(capacity, dim, device=dev, max_batch=n, value_dtype=value_dtype)
        t.insert(torch.from_numpy(keys).to(dev), torch.from_numpy(rows).to(dev))
        t.remove(torch.from_numpy(keys[n - gone:]).to(dev))
        assert t.size() == n - gone and (keys < 0).any()
        _tables[value_dtype, dim, kind] = t, keys[:n - gone], rows[:n - gone], keys[n - gone:]
    return _tables[value_dtype, dim, kind]


def expected(kind, metric, dim, keys, rows, queries, k):
    """the reference's answer, computed once for both row types (the integer rows are the same in fp32 and bf16); a tie crosses every k-th place"""
    nq = len(queries)
    if (kind, metric, dim, nq, k) not in _expected:
        ek, es, ec, scores = REFERENCE[metric](keys, rows, queries, k)
        kth = -np.partition(-scores, (k - 1, k), axis=1)[:, k - 1:k + 1]
        assert (kth[:, 0] == kth[:, 1]).all() and (ec == k).all(), "no tie across the k-th place"
        _expected[kind, metric, dim, nq, k] = ek, es, ec
    return _expected[kind, metric, dim, nq, k]


def same(got, ek, es, ec):
    gk, gs, gc = (x.cpu().numpy() for x in got)
    assert np.array_equal(gk, ek) and np.array_equal(gc, ec)
    assert np.array_equal(gs.view(np.uint32), es.astype(np.float32).view(np.uint32))


@pytest.mark.parametrize("nq,k", [(1, 1), (33, 10), (5, 64)])
@pytest.mark.parametrize("dim", [272, 512, 1008, 1024])   # a chunk and one k-step | two chunks | three and a short one | four
@pytest.mark.parametrize("metric", ["ip", "cosine"])
@pytest.mark.parametrize("value_dtype", [F32, BF16])
def test_bit_for_bit(dev, value_dtype, metric, dim, nq, k):
    """integers in [-4, 4]: every partial sum is at most 16 * 1024 = 16 384, far inside 2^24, so keys, score bits and counts equal the reference.
    (33, 10): tiles of 32 + 1 queries at dim 272, of 16 + 16 + 1 at dims 1008 and 1024 (a tile's LDS budget holds 17 queries of such a row at
    k = 10, rounded down to a multiple of 8), of 24 + 9 at dim 512; (1, 1) is a one-query tile at every width.  (5, 64): two entries per lane in
    the prune."""
    t, keys, rows, _ = table(dev, value_dtype, dim)
    queries = np.random.default_rng(SEED + nq).integers(-4, 5, (nq, dim)).astype(np.float32)
    same(t.search(torch.from_numpy(queries).to(dev), k, counts=True, metric=metric), *expected("sparse", metric, dim, keys, rows, queries, k))


def test_dense(dev):
    """dim 272, fp32 rows, k = 8, Q = 3 on 200 000 slots at load 0.69: 6 250 steps of 32 slots, 195 of them the seed pass, the other 6 055 over the
    CUs * 8 = 2 048 blocks of a 256-CU device — three steps a block, some 66 live slots against a candidate buffer of 2 * max(k, 8) = 16 entries.
    Buffers fill and prunes run in the seed pass's blocks (one step each, 22 live slots, no threshold to start from); the main scan's blocks
    start from the seed's thresholds and reject nearly everything.  Bit for bit, a tie across the 8th place for every query."""
    t, keys, rows, _ = table(dev, F32, 272, "dense")
    queries = np.random.default_rng(SEED + 3).integers(-4, 5, (3, 272)).astype(np.float32)
    same(t.search(torch.from_numpy(queries).to(dev), 8, counts=True), *expected("dense", "ip", 272, keys, rows, queries, 8))


@pytest.mark.parametrize("dim", [272, 1008, 1024])   # passes of 64 element groups: one and four lanes of a second | three and 60 lanes | four
@pytest.mark.parametrize("metric", ["ip", "cosine"])
@pytest.mark.parametrize("value_dtype", [F32, BF16])
def test_score(dev, value_dtype, metric, dim):
    """a slate of present, absent, removed, repeated and INT64_MIN keys (37 a query: no multiple of a wave step): score bits and found bytes equal
    the reference; the scores of search's own keys are search's scores bit for bit, the padded tail of a 40-row table at k = 64 included"""
    from meepoembedding_amd import LookupTable
    t, keys, rows, removed = table(dev, value_dtype, dim)
    rng = np.random.default_rng(SEED + dim)
    queries = rng.integers(-4, 5, (5, dim)).astype(np.float32)
    at = rng.integers(0, len(keys), (5, 20))
    slate = np.concatenate([keys[at], keys[at[:, :5]], np.tile(np.r_[removed[:6], 2**62 + 1, 2**62 + 2, I64_MIN, I64_MIN, -2**62 - 7, removed[-1]], (5, 1))], axis=1)
    assert slate.shape == (5, 37)
    scores = REFERENCE[metric](keys, rows, queries, 1)[3]
    want = np.full(slate.shape, -np.inf)
    want[:, :25] = np.take_along_axis(scores, np.concatenate([at, at[:, :5]], axis=1), axis=1)
    sc, found = t.score(torch.from_numpy(queries).to(dev), torch.from_numpy(slate).to(dev), metric=metric)
    assert np.array_equal(sc.cpu().numpy().view(np.uint32), want.astype(np.float32).view(np.uint32))
    assert np.array_equal(found.cpu().numpy(), np.isfinite(want).astype(np.uint8))

    small = LookupTable(1000, dim, device=dev, max_batch=64, value_dtype=value_dtype)
    small.insert(torch.from_numpy(keys[:40]).to(dev), torch.from_numpy(rows[:40]).to(dev))
    qt = torch.from_numpy(queries).to(dev)
    for tab, k in ((t, 10), (small, 64)):
        gk, gs, gc = tab.search(qt, k, counts=True, metric=metric)
        sc, found = tab.score(qt, gk, metric=metric)
        assert (gc == min(k, tab.size())).all() and torch.equal(sc.view(torch.int32), gs.view(torch.int32))
        assert torch.equal(found, (gk != I64_MIN).to(torch.uint8))
    same(small.search(qt, 64, counts=True, metric=metric), *REFERENCE[metric](keys[:40], rows[:40], queries, 64)[:3])


@pytest.mark.parametrize("value_dtype", [F32, BF16])
def test_general_values(dev, value_dtype):
    """standard-normal operands at dim 768: the two bounds of SPEC.md §3 "Search" exactly as tests/test_search.py::test_general_values states them,
    and for cosine — search's scores and score()'s of the same keys — the bounds of "Metric" as tests/test_search_cosine.py applies them"""
    dim, nq, k = 768, 40, 16
    t, keys, rows, _ = table(dev, value_dtype, dim, "normal")
    queries = np.random.default_rng(SEED + 1).standard_normal((nq, dim)).astype(np.float32)
    qt = torch.from_numpy(queries).to(dev)
    q, r = bf16(queries), bf16(rows)
    pos = {int(key): i for i, key in enumerate(keys)}
    den = np.sqrt((q * q).sum(1))[:, None] * np.sqrt((r * r).sum(1))[None, :]
    dot_bound = (dim - 1) * 2.0**-24 * (np.abs(q) @ np.abs(r).T)
    for metric in ("ip", "cosine"):
        if metric == "ip":
            ek, es, _, scores = reference(keys, rows, queries, k)
            bound = dot_bound
        else:
            ek, es, _, scores = cosine_reference(keys, rows, queries, k, exact=False)
            bound = dot_bound / den + (dim + 4) * 2.0**-24 * np.abs(scores)
        gk_t, gs_t = t.search(qt, k, metric=metric)
        gk, gs, rs = gk_t.cpu().numpy(), gs_t.cpu().numpy(), t.score(qt, gk_t, metric=metric)[0].cpu().numpy()
        for i in range(nq):
            at = [pos[int(key)] for key in gk[i]]   # (a key that is not in the table fails here)
            assert len(set(at)) == k and (np.diff(gs[i]) <= 0).all()
            assert (np.abs(gs[i].astype(np.float64) - scores[i, at]) <= bound[i, at]).all() and (np.abs(rs[i].astype(np.float64) - scores[i, at]) <= bound[i, at]).all()
            assert (scores[i, at] >= es[i, k - 1] - bound[i, at] - bound[i, [pos[int(key)] for key in ek[i]]].max()).all()


def test_interface(dev):
    """dim 272 with Q = 1 goes through LookupTable.search; a table of dim 1040 cannot be created at all (mee_create stops at 1024); an int8-row table
    at dim 512 and k = 65 are still refused; mee_search itself, the per-call entry, answers INVALID_ARG at dim 272; a find still works afterwards"""
    from meepoembedding_amd import LookupTable, MeepoError, _lib
    t, keys, rows, _ = table(dev, F32, 272)
    q = torch.from_numpy(np.random.default_rng(SEED).integers(-4, 5, (1, 272)).astype(np.float32)).to(dev)
    gk, gs = t.search(q, 4)
    assert np.array_equal(gk.cpu().numpy(), reference(keys, rows, q.cpu().numpy(), 4)[0])
    with pytest.raises(MeepoError):
        LookupTable(1000, 1040, device=dev, max_batch=64)
    int8 = LookupTable(1000, 512, device=dev, max_batch=64, int8_rows=True)
    q512 = torch.ones(1, 512, device=dev)
    for tab, queries, k, metric in [(int8, q512, 4, "ip"), (int8, q512, 4, "cosine"), (t, q, 65, "ip"), (t, q, 65, "cosine")]:
        with pytest.raises(MeepoError) as e:
            tab.search(queries, k, metric=metric)
        assert e.value.code == (_lib.ERR_UNSUPPORTED if tab is int8 else _lib.ERR_INVALID_ARG)
    with pytest.raises(MeepoError) as e:
        int8.score(q512, torch.ones(1, 3, dtype=torch.int64, device=dev))
    assert e.value.code == _lib.ERR_UNSUPPORTED
    need, ws = C.c_uint64(), torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    assert _lib.lib().mee_search_workspace_bytes(t._h, 1, 4, C.byref(need)) == _lib.ERR_INVALID_ARG
    assert _lib.lib().mee_search(t._h, q.data_ptr(), 1, 4, gk.data_ptr(), gs.data_ptr(), None, ws.data_ptr(), None) == _lib.ERR_INVALID_ARG
    torch.cuda.synchronize(dev)
    assert t.find(torch.from_numpy(keys[:5]).to(dev))[1].all()
