"""LookupTable.search (SPEC.md §3 "Search") against a dozen lines of NumPy: both operands rounded to bf16, scores in float64, greater score first,
equal scores by the smaller key, NaN scores dropped, the tail padded with INT64_MIN / -inf."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
I64_MIN = np.iinfo(np.int64).min
SEED = 553   # with it the reference sees a tie across the k-th place in every case of test_bit_for_bit (asserted there)


def bf16(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).to(torch.float64).numpy()


def reference(keys, rows, queries, k):
    scores = bf16(queries) @ bf16(rows).T + 0.0 if len(keys) else np.zeros((len(queries), 0))
    out_k, out_s, cnt = np.full((len(queries), k), I64_MIN), np.full((len(queries), k), -np.inf), np.zeros(len(queries), dtype=np.int32)
    for i, s in enumerate(scores):
        ok = ~np.isnan(s)
        if ok.sum() > k:
            ok &= s >= np.partition(s[ok], -k)[-k]   # (only what reaches the k-th score needs sorting)
        order = np.lexsort((keys[ok], -s[ok]))[:k]
        out_k[i, :len(order)], out_s[i, :len(order)], cnt[i] = keys[ok][order], s[ok][order], len(order)
    return out_k, out_s, cnt, scores


def filled(dev, value_dtype, dim, rows_of, capacity=200_000, n=3000, gone=300, same=300):
    """a table of `capacity` slots (a prime, so odd, bucket count; thousands of wave steps, most of them with few or no live slots) holding n - gone
    keys, negative ones among them, `same` pairs of which carry identical rows; `gone` more keys were inserted and removed again -> (table, keys, rows)"""
    from meepoembedding_amd import LookupTable
    rng = np.random.default_rng(SEED)
    keys = rng.permutation(np.unique(rng.integers(-2**62, 2**62, 2 * n)))[:n]
    rows = rows_of(rng, (n, dim)).astype(np.float32)
    rows[1:2 * same:2] = rows[0:2 * same:2]
    t = LookupTable(capacity, dim, device=dev, max_batch=max(n, 4096), value_dtype=value_dtype)
    t.insert(torch.from_numpy(keys).to(dev), torch.from_numpy(rows).to(dev))
    t.remove(torch.from_numpy(keys[n - gone:]).to(dev))
    assert t.size() == n - gone and t.n_buckets % 2 == 1 and (keys < 0).any()
    return t, keys[:n - gone], rows[:n - gone]


_tables = {}


def shared_table(dev, value_dtype, dim, kind):
    if (value_dtype, dim, kind) not in _tables:
        rows_of = (lambda rng, shape: rng.integers(-4, 5, shape)) if kind != "normal" else (lambda rng, shape: rng.standard_normal(shape))
        # "dense": a million slots at load 0.675 — a one-wave block of the scan walks ~16 steps and some 350 live slots per query, so candidate
        # buffers fill, prunes run and raised thresholds reject and tie many times in every block
        size = dict(capacity=1_000_000, n=750_000, gone=75_000) if kind == "dense" else {}
        _tables[value_dtype, dim, kind] = filled(dev, value_dtype, dim, rows_of, **size)
    return _tables[value_dtype, dim, kind]


SPARSE = [(dim, nq, k, "int") for dim in (16, 64, 256) for nq, k in [(1, 1), (33, 10), (64, 64), (200, 8)]]   # (64, 64), (200, 8): several native calls
DENSE = [(16, 3, 1, "dense"), (16, 34, 10, "dense"), (16, 6, 64, "dense"), (64, 3, 33, "dense")]   # the selection protocol at work: k = 64 prunes two entries per lane


@pytest.mark.parametrize("dim,nq,k,kind", SPARSE + DENSE)
@pytest.mark.parametrize("value_dtype", [torch.float32, torch.bfloat16])
def test_bit_for_bit(dev, value_dtype, dim, nq, k, kind):
    """integers in [-4, 4]: exact in bf16, every partial sum below 2^24 — keys, score bits and counts equal the reference"""
    from meepoembedding_amd import _lib
    t, keys, rows = shared_table(dev, value_dtype, dim, kind)
    queries = np.random.default_rng(SEED + nq).integers(-4, 5, (nq, dim)).astype(np.float32)
    ek, es, ec, scores = reference(keys, rows, queries, k)
    kth = -np.partition(-scores, (k - 1, k), axis=1)[:, k - 1:k + 1]
    assert (kth[:, 0] == kth[:, 1]).any(), "the case has no tie across the k-th place"
    if (nq, k) in ((64, 64), (200, 8)):
        assert nq * max(k, 8) > _lib.SEARCH_MAX_QK
    gk, gs, gc = t.search(torch.from_numpy(queries).to(dev), k, counts=True)
    assert np.array_equal(gk.cpu().numpy(), ek)
    assert np.array_equal(gs.cpu().numpy().view(np.uint32), es.astype(np.float32).view(np.uint32))
    assert np.array_equal(gc.cpu().numpy(), ec) and (ec == k).all()


def test_fewer_candidates_than_k_and_nan(dev):
    from meepoembedding_amd import LookupTable
    t = LookupTable(1000, 32, device=dev, max_batch=64)
    queries = torch.ones(3, 32, device=dev)
    gk, gs, gc = t.search(queries, 8, counts=True)   # an empty table
    assert (gc == 0).all() and (gk == I64_MIN).all() and torch.isneginf(gs).all()
    keys, rows = np.array([7, -3, 11, 5, -9]), np.arange(5 * 32, dtype=np.float32).reshape(5, 32) % 7 - 3
    rows[2, 13] = np.nan
    t.insert(torch.from_numpy(keys).to(dev), torch.from_numpy(rows).to(dev))
    ek, es, ec, _ = reference(keys, rows, queries.cpu().numpy(), 8)
    gk, gs, gc = t.search(queries, 8, counts=True)
    assert (ec == 4).all() and np.array_equal(gc.cpu().numpy(), ec) and np.array_equal(gk.cpu().numpy(), ek) and 11 not in ek
    assert np.array_equal(gs.cpu().numpy().view(np.uint32), es.astype(np.float32).view(np.uint32))


@pytest.mark.parametrize("dim", [64, 256])
@pytest.mark.parametrize("value_dtype", [torch.float32, torch.bfloat16])
def test_general_values(dev, value_dtype, dim):
    """standard-normal operands: every returned score within the contract's bound, (dim - 1) 2^-24 sum |products|, of that key's float64 score; every
    returned key's float64 score at least the reference's k-th minus that key's bound and the largest bound among the reference's k keys — a kept
    key r can only displace a reference key x whose COMPUTED score it reaches, and the two computed scores are off by up to bound_r and bound_x
    (SPEC.md §3 "Search"); no key twice"""
    t, keys, rows = shared_table(dev, value_dtype, dim, "normal")
    nq, k = 40, 16
    queries = np.random.default_rng(SEED + 1).standard_normal((nq, dim)).astype(np.float32)
    ek, es, _, scores = reference(keys, rows, queries, k)
    bound = (dim - 1) * 2.0**-24 * (np.abs(bf16(queries)) @ np.abs(bf16(rows)).T)
    gk, gs = (x.cpu().numpy() for x in t.search(torch.from_numpy(queries).to(dev), k))
    pos = {int(key): i for i, key in enumerate(keys)}
    for i in range(nq):
        at = [pos[int(key)] for key in gk[i]]   # (a key that is not in the table fails here)
        assert len(set(at)) == k
        assert (np.abs(gs[i].astype(np.float64) - scores[i, at]) <= bound[i, at]).all()
        assert (scores[i, at] >= es[i, k - 1] - bound[i, at] - bound[i, [pos[int(key)] for key in ek[i]]].max()).all()
        assert (np.diff(gs[i]) <= 0).all()


def test_refusals(dev):
    from meepoembedding_amd import LookupTable, MeepoError
    t = LookupTable(1000, 32, device=dev, max_batch=64)
    keys = torch.arange(1, 9, device=dev)
    t.insert(keys, torch.ones(8, 32, device=dev))
    q = torch.ones(2, 32, device=dev)
    for table, queries, k in [(LookupTable(1000, 32, device=dev, max_batch=64, int8_rows=True), q, 4), (LookupTable(1000, 24, device=dev, max_batch=64), torch.ones(2, 24, device=dev), 4),
                              (t, q, 0), (t, q, 65), (t, q.double(), 4), (t, q.cpu(), 4)]:
        with pytest.raises(MeepoError):
            table.search(queries, k)
    torch.cuda.synchronize(dev)
    out, found = t.find(torch.arange(0, 10, device=dev))
    assert found.tolist() == [0] + [1] * 8 + [0] and (out[1:9] == 1).all()
