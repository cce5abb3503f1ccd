"""TableGroup.search / mee_group_search (SPEC.md §3 "Search", "Groups") against the float64 references of tests/test_search.py and test_search_cosine.py and each member's own search, bit for bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
from test_search import I64_MIN, SEED, reference
from test_search_cosine import reference as cosine_reference, table as shared_table

_members, _expected = {}, {}


def small(dev, value_dtype, dim, capacity, n, gone, seed):
    """a table of its own: n integer rows in [-4, 4] under keys of both signs, the last `gone` removed again -> (table, live keys, live rows)"""
    from meepoembedding_amd import LookupTable
    rng = np.random.default_rng(SEED + seed)
    keys, rows = rng.permutation(np.arange(-n, n))[:n], rng.integers(-4, 5, (n, dim)).astype(np.float32)
    t = LookupTable(capacity, dim, device=dev, max_batch=max(n, 64), value_dtype=value_dtype)
    t.insert(torch.from_numpy(keys).to(dev), torch.from_numpy(rows).to(dev))
    t.remove(torch.from_numpy(keys[n - gone:]).to(dev))
    assert t.size() == n - gone
    return t, keys[:n - gone], rows[:n - gone]


def members(dev, value_dtype, dim):
    """1 000 slots, 500 keys | 200 000 slots, 2 700 keys: several ranges, most steps empty | 50 keys inserted and all removed: counts 0, all padding | 40 000 slots,
    40 keys: fewer than k = 64.  Some 7 500 steps: with 2 048 blocks S is 4, and the emptied member — 80 slots, 3 steps — is the one with exactly one range, shorter than S."""
    if (value_dtype, dim) not in _members:
        _members[value_dtype, dim] = [shared_table(dev, value_dtype, dim, "small"), shared_table(dev, value_dtype, dim, "sparse"),
                                      small(dev, value_dtype, dim, 64, 50, 50, 1), small(dev, value_dtype, dim, 40_000, 40, 0, 2)]
    return _members[value_dtype, dim]


def same_as_members(tabs, nq, k, metric, group=None):
    """the group of `tabs` (a new one unless given), integer queries: each member's block against its reference and its own search -> the answer"""
    from meepoembedding_amd import TableGroup
    dev, dim = tabs[0][0].device, tabs[0][0].dim
    queries = torch.from_numpy(np.random.default_rng(SEED + nq).integers(-4, 5, (len(tabs), nq, dim)).astype(np.float32)).to(dev)
    group = group or TableGroup([t for t, _, _ in tabs])
    got = group.search(queries, k, counts=True, metric=metric)
    for j, (t, keys, rows) in enumerate(tabs):
        qj = queries[j].cpu().numpy()
        tag = (metric, keys.tobytes(), qj.shape, qj.tobytes(), k)
        ek, es, ec = _expected[tag] = _expected.get(tag) or (reference if metric == "ip" else cosine_reference)(keys, rows, qj, k)[:3]
        gk, gs, gc = (x[j] for x in got)
        assert np.array_equal(gk.cpu().numpy(), ek) and np.array_equal(gc.cpu().numpy(), ec), j
        assert np.array_equal(gs.cpu().numpy().view(np.uint32), es.astype(np.float32).view(np.uint32)), j
        own = t.search(queries[j], k, counts=True, metric=metric)
        assert torch.equal(gk, own[0]) and torch.equal(gs.view(torch.int32), own[1].view(torch.int32)) and torch.equal(gc, own[2]), j
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("dim,nq,k", [(16, 1, 1), (64, 33, 10), (64, 5, 64), (272, 9, 4)])
@pytest.mark.parametrize("metric", ["ip", "cosine"])
@pytest.mark.parametrize("value_dtype", [torch.float32, torch.bfloat16])
def test_bit_for_bit(dev, value_dtype, metric, dim, nq, k):
    """integers in [-4, 4]: exact sums, so every bit is the references' and the members' own; Q = 33 is two tiles (a tile: at most a row block of 32 queries)"""
    from meepoembedding_amd import _lib
    assert nq != 33 or nq > min(32, _lib.SEARCH_MAX_QK // max(k, 8), _lib.SEARCH_MAX_QUERY_ELEMS // dim // 32 * 32)
    gk, gs, gc = same_as_members(members(dev, value_dtype, dim), nq, k, metric)
    assert (gc[2] == 0).all() and (gk[2] == I64_MIN).all() and torch.isneginf(gs[2]).all() and (gc[3] == min(k, 40)).all() and (gc[:2] == k).all()


@pytest.mark.gpu
def test_single_member_and_reserve(dev):
    """a group of one table; then three members — 80 slots with live keys (one range, shorter than the step length the 200 000-slot member forces),
    that member, and 1 000 slots — before and after reserve() doubles the last: the descriptors are re-read and the plan follows on the device"""
    tabs = [small(dev, torch.float32, 64, 64, 40, 5, 3), shared_table(dev, torch.float32, 64, "sparse"), small(dev, torch.float32, 64, 1000, 500, 50, 4)]
    from meepoembedding_amd import TableGroup
    same_as_members(tabs[2:], 5, 10, "ip")
    group = TableGroup([t for t, _, _ in tabs])
    same_as_members(tabs, 5, 10, "cosine", group)
    tabs[2][0].reserve(2 * tabs[2][0].capacity)
    assert tabs[2][0].capacity >= 2000
    same_as_members(tabs, 5, 10, "cosine", group)


@pytest.mark.gpu
def test_graph_replay(dev):
    """captured after a warm-up call (the stream's workspace exists) and replayed into preallocated outputs: the eager result every time"""
    from meepoembedding_amd import TableGroup
    group, nq, k = TableGroup([t for t, _, _ in members(dev, torch.float32, 64)]), 33, 10
    queries = torch.from_numpy(np.random.default_rng(SEED).integers(-4, 5, (4, nq, 64)).astype(np.float32)).to(dev)
    out = [torch.zeros(4, nq, k, dtype=torch.int64, device=dev), torch.zeros(4, nq, k, device=dev)]
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        eager = group.search(queries, k)
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            group.search(queries, k, out_keys=out[0], out_scores=out[1])
    for _ in range(3):
        out[0].zero_(), out[1].zero_()
        graph.replay()
        torch.cuda.synchronize(dev)
        assert torch.equal(out[0], eager[0]) and torch.equal(out[1].view(torch.int32), eager[1].view(torch.int32))


@pytest.mark.gpu
def test_refusals(dev):
    from meepoembedding_amd import LookupTable, MeepoError, TableGroup, _lib
    L, dim, nq, k, tables = _lib.lib(), 32, 40, 4, [LookupTable(1000, 32, device=dev, max_batch=64) for _ in range(3)]
    tables[1].insert(torch.arange(1, 9, device=dev), torch.ones(8, dim, device=dev))
    group, q = TableGroup(tables), torch.ones(3, nq, dim, device=dev)
    g24, too_many = TableGroup([LookupTable(1000, 24, device=dev, max_batch=64)]), torch.ones(3, _lib.SEARCH_BATCH_MAX_QUERIES // 3 + 1, dim, device=dev)
    for g, queries, kk, metric in [(group, q, 0, "ip"), (group, q, 65, "ip"), (group, q, k, "l2"), (group, q[:, :0], k, "ip"), (group, too_many, k, "ip"),
                                   (group, q[0], k, "ip"), (group, q.double(), k, "ip"), (group, q.cpu(), k, "ip"), (g24, torch.ones(1, 2, 24, device=dev), k, "ip")]:
        with pytest.raises(MeepoError) as e:
            g.search(queries, kk, metric=metric)
        assert e.value.code == _lib.ERR_INVALID_ARG
    need, cus = C.c_uint64(), torch.cuda.get_device_properties(dev).multi_processor_count
    assert L.mee_group_search_workspace_bytes(group._h, _lib.METRIC_IP, nq, k, C.byref(need)) == 0
    ranges = max(1, 8 * cus // -(-nq // 32))   # dim 32, k = 4: a tile is one row block of 32 queries
    assert need.value == (8 + 4 * (3 + 1) + 15) // 16 * 16 + (ranges + 3) * nq * k * 12
    ws, keys, scores = torch.empty(need.value + 8, dtype=torch.uint8, device=dev), torch.zeros(3, nq, k, dtype=torch.int64, device=dev), torch.zeros(3, nq, k, device=dev)
    call = lambda metric, space: L.mee_group_search(group._h, metric, q.data_ptr(), nq, k, keys.data_ptr(), scores.data_ptr(), None, space, None)   # noqa: E731
    assert L.mee_group_search_workspace_bytes(group._h, 2, nq, k, C.byref(need)) == _lib.ERR_INVALID_ARG and need.value == 0
    for metric, space in [(2, ws.data_ptr()), (_lib.METRIC_IP, None), (_lib.METRIC_IP, ws.data_ptr() + 4)]:
        assert call(metric, space) == _lib.ERR_INVALID_ARG and L.mee_last_error().startswith(b"mee_group_search:")
    torch.cuda.synchronize(dev)
    assert not keys.any() and not scores.any()   # nothing was written
    assert call(_lib.METRIC_IP, ws.data_ptr()) == 0 and (keys[1, :, 0] == 1).all() and (keys[0] == I64_MIN).all()
    out, found = group.find(torch.arange(0, 10, device=dev), torch.tensor([0, 0, 10, 10], device=dev))
    assert found.tolist() == [0] + [1] * 8 + [0] and (out[1:9] == 1).all()


def test_symbols(built):
    """both entry points are declared, exported and bound with the declared number of arguments; a null group is refused under the operator's name"""
    from meepoembedding_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "meepo_embedding.h")).read(), flags=re.S)
    raw, L, need = C.CDLL(_lib.LIB_PATH), _lib.lib(), C.c_uint64(7)
    for name in ("mee_group_search_workspace_bytes", "mee_group_search"):
        declared = re.search(r"\b%s\s*\(([^)]*)\)" % name, header)
        assert declared and hasattr(raw, name) and len(_lib.PROTOTYPES[name][1]) == len(declared.group(1).split(","))
    assert L.mee_group_search_workspace_bytes(None, 0, 1, 1, C.byref(need)) == _lib.ERR_INVALID_ARG and need.value == 0 and L.mee_last_error().startswith(b"mee_group_search_workspace_bytes:")
    assert L.mee_group_search(None, 0, None, 1, 1, None, None, None, None, None) == _lib.ERR_INVALID_ARG and L.mee_last_error().startswith(b"mee_group_search:")
