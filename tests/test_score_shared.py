"""LookupTable.score with a shared slate, keys [C] (SPEC.md §3 "Score", "Shared slate"; mee_score_shared), against NumPy in float64: both operands
rounded to bf16, -inf and found 0 for a key the table does not hold — and against the per-query path over keys.expand(Q, C)."""
import numpy as np
import pytest
import torch

from test_score import DTYPES, I64_MIN, SEED, bf16, filled

pytestmark = pytest.mark.gpu
METRICS = ["ip", "cosine"]


def reference(keys, rows, queries, slate, metric, exact):
    """-> (scores [Q, C]: -inf where the table has no such key, found [C], the contract's bound [Q, C]).  exact: float64 sums cast to float32 and,
    for cosine, the four float32 operations; otherwise float64 throughout"""
    pos = {int(k): i for i, k in enumerate(keys)}
    at = np.array([pos.get(int(k), -1) for k in slate])
    q, r = bf16(queries), bf16(rows)[at]
    dim, ft = q.shape[1], np.float32 if exact else np.float64
    dot, mag = q @ r.T, np.abs(q) @ np.abs(r).T
    if metric == "ip":
        s, bound = dot.astype(ft) + ft(0), (dim - 1) * 2.0**-24 * mag
    else:
        with np.errstate(all="ignore"):
            den = np.sqrt((q * q).sum(1).astype(ft))[:, None] * np.sqrt((r * r).sum(1).astype(ft))[None, :]
            s = dot.astype(ft) / den + ft(0)
            bound = (dim - 1) * 2.0**-24 * mag / den + (dim + 4) * 2.0**-24 * np.abs(s)
    return np.where(at >= 0, s, ft(-np.inf)), at >= 0, bound


def mixed_slate(rng, keys, gone, width):
    """[width >= 5] candidates: present keys, a repeated one, a removed one, a never-inserted one and search's padding key, shuffled"""
    s = rng.choice(keys, width)
    s[1], s[2], s[3], s[4] = rng.integers(2**62, 2**63 - 1), rng.choice(gone), I64_MIN, s[0]
    return rng.permutation(s)


@pytest.mark.parametrize("nq,nc", [(1, 1), (33, 70), (200, 37), (5, 32)])
@pytest.mark.parametrize("dim", [16, 48, 256, 272, 1024])
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("value_dtype", DTYPES)
def test_bit_for_bit(dev, value_dtype, metric, dim, nq, nc):
    """exactly summable data: score bits, -inf columns and found equal the reference and the per-query path.  A slate narrower than the five kinds
    of candidate is scored as several calls of that width, so that every case holds all of them."""
    t, keys, rows, gone = filled(dev, value_dtype, dim, "int")
    rng = np.random.default_rng(SEED + 1000 * nq + nc)
    queries = rng.integers(-4, 5, (nq, dim)).astype(np.float32)
    slate = mixed_slate(rng, keys, gone, nc * -(-5 // nc))
    es, ef, _ = reference(keys, rows, queries, slate, metric, exact=True)
    assert ef.any() and (~ef).sum() == 3
    q, k = torch.from_numpy(queries).to(dev), torch.from_numpy(slate).to(dev)
    parts = [t.score(q, k[c:c + nc], metric=metric) for c in range(0, len(slate), nc)]
    gs, gf = torch.cat([p[0] for p in parts], 1), torch.cat([p[1] for p in parts])
    assert all(p[0].shape == (nq, nc) and p[1].shape == (nc,) and p[1].dtype == torch.uint8 for p in parts)
    assert np.array_equal(gf.cpu().numpy().astype(bool), ef)
    assert np.array_equal(gs.cpu().numpy().view(np.uint32), es.view(np.uint32))
    assert torch.isneginf(gs[:, torch.from_numpy(~ef).to(dev)]).all()
    per_query = t.score(q, k.expand(nq, len(slate)).contiguous(), metric=metric)[0]
    assert torch.equal(gs.view(torch.int32), per_query.view(torch.int32))


@pytest.mark.parametrize("nc", [12288, 25000])
@pytest.mark.parametrize("dim", [16, 48, 256])
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("value_dtype", DTYPES)
def test_bit_for_bit_tiles(dev, value_dtype, metric, dim, nc):
    """a slate long enough that the host keeps tiles of several row blocks (on 256 CUs: 64 queries a tile at C = 12288, 96 at C = 25000, which
    is dim 256's whole tile): 200 queries cross row blocks inside a tile, whole tiles and a short last tile, over many spans"""
    test_bit_for_bit(dev, value_dtype, metric, dim, 200, nc)


@pytest.mark.parametrize("dim", [64, 768])
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("value_dtype", DTYPES)
def test_general_values(dev, value_dtype, metric, dim):
    """standard-normal operands: every score within the contract's per-key bound of the float64 value — (dim - 1) 2^-24 sum |products|, and for
    cosine that over |q| |row| plus (dim + 4) 2^-24 |cos|"""
    t, keys, rows, gone = filled(dev, value_dtype, dim, "normal")
    rng = np.random.default_rng(SEED + dim)
    queries, slate = rng.standard_normal((40, dim)).astype(np.float32), mixed_slate(rng, keys, gone, 150)
    es, ef, bound = reference(keys, rows, queries, slate, metric, exact=False)
    gs, gf = (x.cpu().numpy() for x in t.score(torch.from_numpy(queries).to(dev), torch.from_numpy(slate).to(dev), metric=metric))
    assert np.array_equal(gf.astype(bool), ef) and np.isneginf(gs[:, ~ef]).all()
    assert (np.abs(gs[:, ef].astype(np.float64) - es[:, ef]) <= bound[:, ef]).all()


def test_specials(dev):
    from meepoembedding_amd import LookupTable
    t = LookupTable(1000, 32, device=dev, max_batch=64)
    rows = np.zeros((3, 32), dtype=np.float32)
    rows[0, 13] = np.nan
    rows[1, :6] = [-1, -1, 2, 0, -3, -5]   # against (1, 1, 1, 1, 0, ...): products -1, -1, 2, 0 and negative zeros; row 2 is a zero row
    t.insert(torch.tensor([21, 22, 23], device=dev), torch.from_numpy(rows).to(dev))
    q = torch.zeros(2, 32, device=dev)   # query 1 is a zero query
    q[0, :4] = 1
    keys = torch.tensor([21, 22, 23], device=dev)
    gs, gf = t.score(q, keys)
    assert gf.tolist() == [1, 1, 1] and torch.isnan(gs[:, 0]).all() and gs.view(torch.int32)[:, 1:].eq(0).all()
    gs, gf = t.score(q, keys, metric="cosine")
    assert gf.tolist() == [1, 1, 1] and torch.isnan(gs[:, 0]).all() and torch.isnan(gs[:, 2]).all() and torch.isnan(gs[1]).all()
    assert gs.view(torch.int32)[0, 1].item() == 0


def test_interface_and_refusals(dev):
    from meepoembedding_amd import LookupTable, MeepoError, _lib
    t = LookupTable(1000, 32, device=dev, max_batch=64)
    t.insert(torch.arange(1, 9, device=dev), torch.ones(8, 32, device=dev))
    q, k = torch.ones(2, 32, device=dev), torch.arange(0, 5, device=dev)
    out, found = torch.zeros(2, 5, device=dev), torch.zeros(5, dtype=torch.uint8, device=dev)
    got = t.score(q, k, out=out, found=found)
    assert got[0] is out and got[1] is found and found.tolist() == [0, 1, 1, 1, 1] and torch.isneginf(out[:, 0]).all() and (out[:, 1:] == 32).all()
    for table, keys, kw in [(t, k.int(), {}), (t, k.cpu(), {}), (t, k, {"out": torch.empty(2, 6, device=dev)}),
                            (t, k, {"found": torch.empty(2, 5, dtype=torch.uint8, device=dev)}), (t, k, {"metric": "l2"}),
                            (LookupTable(1000, 32, device=dev, max_batch=64, int8_rows=True), k, {})]:
        with pytest.raises(MeepoError):
            table.score(q, keys, **kw)
    L, args = _lib.lib(), [q.data_ptr(), 2, k.data_ptr(), 5, out.data_ptr(), None, None]
    for metric, null in [(0, 0), (0, 2), (0, 4), (2, None)]:
        a = [None if i == null else v for i, v in enumerate(args)]
        assert L.mee_score_shared(t._h, metric, *a) == _lib.ERR_INVALID_ARG and L.mee_last_error().startswith(b"mee_score_shared:")
    assert L.mee_score_shared(t._h, 0, q.data_ptr(), 2, None, 0, None, None, None) == _lib.OK
    torch.cuda.synchronize(dev)
    rows, f = t.find(torch.arange(0, 10, device=dev))
    assert f.tolist() == [0] + [1] * 8 + [0] and (rows[1:9] == 1).all()


def test_graph_replay(dev):
    """one launch, no workspace, no allocation: captured once, replayed, equal to the eager result"""
    t, keys, _, gone = filled(dev, torch.float32, 48, "int")
    rng = np.random.default_rng(SEED)
    q = torch.from_numpy(rng.integers(-4, 5, (70, 48)).astype(np.float32)).to(dev)
    k = torch.from_numpy(mixed_slate(rng, keys, gone, 100)).to(dev)
    out, found = torch.zeros(70, 100, device=dev), torch.zeros(100, dtype=torch.uint8, device=dev)
    eager = t.score(q, k, metric="cosine")
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        t.score(q, k, out=out, found=found, metric="cosine")
    for _ in range(2):
        out.zero_(), found.zero_()
        graph.replay()
        torch.cuda.synchronize(dev)
        assert torch.equal(out.view(torch.int32), eager[0].view(torch.int32)) and torch.equal(found, eager[1])
