"""mee_search_batch (SPEC.md §3 "Search", DESIGN.md §4 "Search" / "Batched") against tests/test_search.py's float64 reference: tiled queries, a seed
pass over the first n_steps / 32 steps of a table of at least 64 such steps, a main scan that starts from the seed's thresholds."""
import ctypes as C

import numpy as np
import pytest
import torch
from test_search import SEED, bf16, filled, reference, shared_table

pytestmark = pytest.mark.gpu
SEED_DIV, SEED_MIN_STEPS = 32, 64   # kSearchSeedDiv, kSearchSeedMinSteps
_expected = {}


def batch(t, queries, k, n=None, ws=True, shift=0):
    """the native entry point called directly -> (return code, keys, scores, counts)"""
    from meepoembedding_amd import _lib
    q = torch.from_numpy(np.ascontiguousarray(queries, dtype=np.float32)).to(t.device)
    n = len(q) if n is None else n
    need = C.c_uint64()
    _lib.lib().mee_search_batch_workspace_bytes(t._h, n, k, C.byref(need))
    space = torch.empty(max(need.value, 8), dtype=torch.uint8, device=t.device)
    keys, scores = torch.empty(len(q), max(k, 1), dtype=torch.int64, device=t.device), torch.empty(len(q), max(k, 1), device=t.device)
    counts = torch.empty(len(q), dtype=torch.int32, device=t.device)
    rc = _lib.lib().mee_search_batch(t._h, q.data_ptr() + shift, n, k, keys.data_ptr(), scores.data_ptr(), counts.data_ptr(), space.data_ptr() if ws else None, None)
    return rc, keys.cpu().numpy(), scores.cpu().numpy(), counts.cpu().numpy()


def same(got, ek, es, ec):
    rc, gk, gs, gc = got
    assert rc == 0 and np.array_equal(gk, ek) and np.array_equal(gc, ec)
    assert np.array_equal(gs.view(np.uint32), es.astype(np.float32).view(np.uint32))


@pytest.mark.parametrize("dim,nq,k", [(16, 154, 10), (16, 50, 64), (256, 70, 8), (64, 200, 33)])   # tiles of 4 x 32 + 26; 24 + 24 + 2; 32 + 32 + 6; 6 x 32 + 8
@pytest.mark.parametrize("kind", ["int", "dense"])   # dense: the prefix holds ~20 000 live rows, the seed bites from the main scan's first step
@pytest.mark.parametrize("value_dtype", [torch.float32, torch.bfloat16])
def test_bit_for_bit(dev, value_dtype, kind, dim, nq, k):
    """integers in [-4, 4] (duplicate rows, removed keys, negative keys): keys, score bits and counts equal the reference, ties across the k-th place included"""
    from meepoembedding_amd import _lib
    t, keys, rows = shared_table(dev, value_dtype, dim, kind)
    assert nq > min(_lib.SEARCH_MAX_QK // max(k, 8), _lib.SEARCH_MAX_QUERY_ELEMS // dim // 32 * 32)   # past one mee_search call: several tiles
    queries = np.random.default_rng(SEED + nq).integers(-4, 5, (nq, dim)).astype(np.float32)
    if (kind, dim, nq, k) not in _expected:   # (the keys and rows of a kind do not depend on the row type: one reference serves both)
        ek, es, ec, scores = reference(keys, rows, queries, k)
        kth = -np.partition(-scores, (k - 1, k), axis=1)[:, k - 1:k + 1]
        assert (kth[:, 0] == kth[:, 1]).any(), "the case has no tie across the k-th place"
        _expected[kind, dim, nq, k] = ek, es, ec
    ek, es, ec = _expected[kind, dim, nq, k]
    same(batch(t, queries, k), ek, es, ec)
    assert (ec == k).all()


@pytest.mark.parametrize("case", ["empty", "nan", "no_seed_pass", "thin_prefix"])
def test_seed_edges(dev, case):
    """empty: nothing but padding.  nan: five keys, one NaN row, k = 8 — no seed pass, a padded tail, counts of 4.  no_seed_pass: 20 000 slots are
    fewer than 64 * 32 steps.  thin_prefix: the seed pass runs and leaves queries WITHOUT a threshold (image 0 in place k - 1) — at 200 000 slots
    the prefix is 6240 slots, which hold ~84 of test_search's 2700 keys, more than k = 64, so this table holds 1350 keys at the same capacity
    (~42 in the prefix); the live rows of the prefix are counted below from the slots locate reports."""
    from meepoembedding_amd import LookupTable, _lib
    ints = lambda rng, shape: rng.integers(-4, 5, shape)   # noqa: E731
    dim, nq, k = 16, 161, 10   # five tiles of 32 and one of a single query
    if case in ("empty", "nan"):
        dim, nq, k = 32, 3, 8
        t, keys, rows = LookupTable(1000, dim, device=dev, max_batch=64), np.zeros(0, dtype=np.int64), np.zeros((0, dim), dtype=np.float32)
        if case == "nan":
            keys, rows = np.array([7, -3, 11, 5, -9]), np.arange(5 * dim, dtype=np.float32).reshape(5, dim) % 7 - 3
            rows[2, 13] = np.nan
            t.insert(torch.from_numpy(keys).to(dev), torch.from_numpy(rows).to(dev))
    elif case == "no_seed_pass":
        t, keys, rows = filled(dev, torch.float32, dim, ints, capacity=20_000)
        assert (t.capacity + 31) // 32 // SEED_DIV < SEED_MIN_STEPS
    else:
        dim, nq, k = 16, 50, 64
        t, keys, rows = filled(dev, torch.float32, dim, ints, n=1500, gone=150, same=150)
        prefix_slots = (t.capacity + 31) // 32 // SEED_DIV * 32
        slots = t.locate(torch.from_numpy(keys).to(dev))[0].cpu().numpy() & _lib.HANDLE_SLOT_MASK
        assert prefix_slots >= SEED_MIN_STEPS * 32 and 0 < (slots < prefix_slots).sum() < k < len(keys)
    queries = np.ones((nq, dim), dtype=np.float32) if nq == 3 else np.random.default_rng(SEED).integers(-4, 5, (nq, dim))
    ek, es, ec, _ = reference(keys, rows, queries, k)
    same(batch(t, queries, k), ek, es, ec)
    assert (ec == {"empty": 0, "nan": 4}.get(case, k)).all() and 11 not in ek


def test_through_search(dev):
    """LookupTable.search past the per-call limits (mee_search_batch over row ranges of the outputs) equals the same queries issued one at a time
    (mee_search); captured in a graph and replayed, it gives the eager result every time — nothing in the call synchronises"""
    t, keys, rows = shared_table(dev, torch.float32, 64, "int")
    nq, k = 200, 33
    queries = torch.from_numpy(np.random.default_rng(SEED).integers(-4, 5, (nq, 64)).astype(np.float32)).to(dev)
    single = [torch.cat(x) for x in zip(*[t.search(queries[i:i + 1], k, counts=True) for i in range(nq)])]
    out = [torch.zeros(nq, k, dtype=torch.int64, device=dev), torch.zeros(nq, k, device=dev)]
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        eager = t.search(queries, k, counts=True)   # (also the warm-up: the stream's workspace exists before the capture)
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            t.search(queries, k, out_keys=out[0], out_scores=out[1])
    assert all(torch.equal(a, b) for a, b in zip(eager, single))
    for _ in range(3):
        out[0].zero_(), out[1].zero_()
        graph.replay()
        torch.cuda.synchronize(dev)
        assert torch.equal(out[0], single[0]) and torch.equal(out[1], single[1])


@pytest.mark.parametrize("dim", [64, 256])
@pytest.mark.parametrize("value_dtype", [torch.float32, torch.bfloat16])
def test_general_values(dev, value_dtype, dim):
    """standard-normal operands, both bounds of SPEC.md §3 "Search" exactly as tests/test_search.py::test_general_values states them"""
    t, keys, rows = shared_table(dev, value_dtype, dim, "normal")
    nq, k = 100, 16
    queries = np.random.default_rng(SEED + 1).standard_normal((nq, dim)).astype(np.float32)
    ek, es, _, scores = reference(keys, rows, queries, k)
    bound = (dim - 1) * 2.0**-24 * (np.abs(bf16(queries)) @ np.abs(bf16(rows)).T)
    rc, gk, gs, _ = batch(t, queries, k)
    pos = {int(key): i for i, key in enumerate(keys)}
    for i in range(nq):
        at = [pos[int(key)] for key in gk[i]]   # (a key that is not in the table fails here)
        assert rc == 0 and len(set(at)) == k
        assert (np.abs(gs[i].astype(np.float64) - scores[i, at]) <= bound[i, at]).all()
        assert (scores[i, at] >= es[i, k - 1] - bound[i, at] - bound[i, [pos[int(key)] for key in ek[i]]].max()).all()
        assert (np.diff(gs[i]) <= 0).all()


def test_refusals(dev):
    from meepoembedding_amd import LookupTable, _lib
    t = LookupTable(1000, 32, device=dev, max_batch=64)
    t.insert(torch.arange(1, 9, device=dev), torch.ones(8, 32, device=dev))
    q, q24 = np.ones((2, 32)), np.ones((2, 24))
    invalid = [(t, q, 4, dict(n=0)), (t, q, 4, dict(n=_lib.SEARCH_BATCH_MAX_QUERIES + 1)), (t, q, 0, {}), (t, q, 65, {}), (t, q, 4, dict(ws=False)),
               (t, q, 4, dict(shift=4)), (LookupTable(1000, 24, device=dev, max_batch=64), q24, 4, {})]
    for table, queries, k, how in invalid:
        assert batch(table, queries, k, **how)[0] == _lib.ERR_INVALID_ARG
    assert batch(LookupTable(1000, 32, device=dev, max_batch=64, int8_rows=True), q, 4)[0] == _lib.ERR_UNSUPPORTED
    torch.cuda.synchronize(dev)
    out, found = t.find(torch.arange(0, 10, device=dev))
    assert found.tolist() == [0] + [1] * 8 + [0] and (out[1:9] == 1).all()
