"""LookupTable.score (SPEC.md §3 "Score") against a dozen lines of NumPy: both operands rounded to bf16, the inner products in float64, -inf and
found 0 for a key the table does not hold."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
I64_MIN = np.iinfo(np.int64).min
SEED = 811
DTYPES = [torch.float32, torch.bfloat16]


def bf16(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).to(torch.float64).numpy()


def reference(keys, rows, queries, slates):
    """-> (scores [Q, C] float64: -inf where the table has no such key, found [Q, C], sum_j |product_j| [Q, C])"""
    pos = {int(k): i for i, k in enumerate(keys)}
    at = np.array([[pos.get(int(k), -1) for k in slate] for slate in slates])
    products = bf16(queries)[:, None, :] * bf16(rows)[at]
    return np.where(at >= 0, products.sum(-1) + 0.0, -np.inf), at >= 0, np.abs(products).sum(-1)


_tables = {}


def filled(dev, value_dtype, dim, kind, n=3000, n_gone=300):
    """a table of 20011 slots' worth of buckets (odd count) holding n - n_gone keys, negative ones among them; n_gone more were inserted and removed
    again.  kind "int": elements in [-4, 4], exact in bf16 with every partial sum below 2^24; "normal": standard normal -> (table, keys, rows, gone)"""
    from meepoembedding_amd import LookupTable
    if (value_dtype, dim, kind) not in _tables:
        rng = np.random.default_rng(SEED)
        keys = rng.permutation(np.unique(rng.integers(-2**62, 2**62, 2 * n)))[:n]
        rows = (rng.integers(-4, 5, (n, dim)) if kind == "int" else rng.standard_normal((n, dim))).astype(np.float32)
        t = LookupTable(20_000, dim, device=dev, max_batch=4096, value_dtype=value_dtype)
        t.insert(torch.from_numpy(keys).to(dev), torch.from_numpy(rows).to(dev))
        t.remove(torch.from_numpy(keys[n - n_gone:]).to(dev))
        assert t.size() == n - n_gone and t.n_buckets % 2 == 1 and (keys < 0).any()
        _tables[value_dtype, dim, kind] = t, keys[:n - n_gone], rows[:n - n_gone], keys[n - n_gone:]
    return _tables[value_dtype, dim, kind]


def mixed_slates(rng, keys, gone, nq, width):
    """[nq, width >= 5] candidates: present keys, and in every row an absent key, a removed one, search's padding key and a repeated key, shuffled"""
    s = rng.choice(keys, (nq, width))
    s[:, 1], s[:, 2], s[:, 3], s[:, 4] = rng.integers(2**62, 2**63 - 1, nq), rng.choice(gone, nq), I64_MIN, s[:, 0]
    return rng.permuted(s, axis=1)


def scored(t, dev, queries, slates, nc):
    """t.score over the slates in column chunks of nc (a chunk is a strided view), side by side again -> (scores, found) as NumPy"""
    q = torch.from_numpy(queries).to(dev)
    parts = [t.score(q, torch.from_numpy(slates).to(dev)[:, c:c + nc]) for c in range(0, slates.shape[1], nc)]
    return torch.cat([p[0] for p in parts], 1).cpu().numpy(), torch.cat([p[1] for p in parts], 1).cpu().numpy()


@pytest.mark.parametrize("nq,nc", [(1, 1), (3, 5), (2, 67), (5, 300)])
@pytest.mark.parametrize("dim", [16, 48, 64, 80, 256])
@pytest.mark.parametrize("value_dtype", DTYPES)
def test_bit_for_bit(dev, value_dtype, dim, nq, nc):
    """exactly summable data: score bits, -inf and found equal the reference.  A slate narrower than the five kinds of candidate is scored as several
    calls of that shape, so that every case holds all of them."""
    t, keys, rows, gone = filled(dev, value_dtype, dim, "int")
    rng = np.random.default_rng(SEED + 1000 * nq + nc)
    queries = rng.integers(-4, 5, (nq, dim)).astype(np.float32)
    slates = mixed_slates(rng, keys, gone, nq, nc * -(-5 // nc))
    es, ef, _ = reference(keys, rows, queries, slates)
    assert ef.any(axis=1).all() and (~ef).any(axis=1).all() and (es[~ef] == -np.inf).all()
    gs, gf = scored(t, dev, queries, slates, nc)
    assert np.array_equal(gs.view(np.uint32), es.astype(np.float32).view(np.uint32))
    assert np.array_equal(gf.astype(bool), ef)


@pytest.mark.parametrize("few", [False, True])
@pytest.mark.parametrize("value_dtype", DTYPES)
def test_agrees_with_search(dev, value_dtype, few):
    """the scores of search's own keys are search's scores, bit for bit; with fewer than k live keys the padded tail is -inf, found 0"""
    from meepoembedding_amd import LookupTable
    t, k = filled(dev, value_dtype, 64, "int")[0], 10
    if few:
        t = LookupTable(1000, 64, device=dev, max_batch=64, value_dtype=value_dtype)
        t.insert(torch.tensor([7, -3, 11, 5, -9], device=dev), torch.from_numpy(np.random.default_rng(SEED).integers(-4, 5, (5, 64)).astype(np.float32)).to(dev))
    q = torch.from_numpy(np.random.default_rng(SEED + 2).integers(-4, 5, (6, 64)).astype(np.float32)).to(dev)
    sk, ss = t.search(q, k)
    gs, gf = t.score(q, sk)
    assert torch.equal(gs.view(torch.int32), ss.view(torch.int32)) and torch.equal(gf.bool(), sk != I64_MIN)
    assert bool((sk == I64_MIN).any()) == few and bool(torch.isneginf(gs).any()) == few


@pytest.mark.parametrize("dim", [64, 256])
@pytest.mark.parametrize("value_dtype", DTYPES)
def test_general_values(dev, value_dtype, dim):
    """standard-normal operands: every score within the contract's bound, (dim - 1) 2^-24 sum |products|, of the float64 value"""
    t, keys, rows, gone = filled(dev, value_dtype, dim, "normal")
    rng = np.random.default_rng(SEED + dim)
    queries, slates = rng.standard_normal((7, dim)).astype(np.float32), mixed_slates(rng, keys, gone, 7, 150)
    es, ef, mag = reference(keys, rows, queries, slates)
    gs, gf = scored(t, dev, queries, slates, 150)
    assert np.array_equal(gf.astype(bool), ef) and np.isneginf(gs[~ef]).all()
    assert (np.abs(gs[ef].astype(np.float64) - es[ef]) <= (dim - 1) * 2.0**-24 * mag[ef]).all()


def test_specials(dev):
    from meepoembedding_amd import LookupTable
    t = LookupTable(1000, 32, device=dev, max_batch=64)
    rows = np.zeros((2, 32), dtype=np.float32)
    rows[0, 13] = np.nan
    rows[1, :6] = [-1, -1, 2, 0, -3, -5]   # against (1, 1, 1, 1, 0, ...): products -1, -1, 2, 0 and negative zeros
    t.insert(torch.tensor([21, 22], device=dev), torch.from_numpy(rows).to(dev))
    q = torch.zeros(1, 32, device=dev)
    q[0, :4] = 1
    gs, gf = t.score(q, torch.tensor([[21, 22]], device=dev))
    assert gf.tolist() == [[1, 1]] and bool(torch.isnan(gs[0, 0])) and gs.view(torch.int32)[0, 1].item() == 0


def test_refusals(dev):
    from meepoembedding_amd import LookupTable, MeepoError
    t = LookupTable(1000, 32, device=dev, max_batch=64)
    t.insert(torch.arange(1, 9, device=dev), torch.ones(8, 32, device=dev))
    q, k = torch.ones(2, 32, device=dev), torch.arange(1, 7, device=dev).view(2, 3)
    for table, queries, keys, out in [(LookupTable(1000, 32, device=dev, max_batch=64, int8_rows=True), q, k, None),
                                      (LookupTable(1000, 24, device=dev, max_batch=64), torch.ones(2, 24, device=dev), k, None),
                                      (t, q.double(), k, None), (t, q.cpu(), k.cpu(), None), (t, q, k.int(), None), (t, q, k[:1], None),
                                      (t, q, k, torch.empty(2, 4, device=dev))]:
        with pytest.raises(MeepoError):
            table.score(queries, keys, out=out)
    torch.cuda.synchronize(dev)
    out, found = t.find(torch.arange(0, 10, device=dev))
    assert found.tolist() == [0] + [1] * 8 + [0] and (out[1:9] == 1).all()
