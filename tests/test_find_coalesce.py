"""GPU: captured finds — consecutive plain finds of one table under stream capture share ONE kernel node (find_captured, meepo_find.hip).
Every case captures a sequence of calls with torch.cuda.graph on a side stream, replays it, and compares every buffer BIT FOR BIT with the same
calls issued eagerly into buffers of their own; mee_find_capture_stats says how many calls got a node and how many joined one."""
import numpy as np
import pytest
import torch

import oracle
from meepoembedding_amd import LookupTable, _lib, synth

pytestmark = pytest.mark.gpu
N_KEYS, BATCH = 20000, 1003   # a batch is no multiple of 8 (a wave step of dim 64) or 32


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def make_table(dev, dim, seed):
    keys = synth.keys_np(seed, 0, N_KEYS)
    t = LookupTable(65536, dim, device=dev, max_batch=N_KEYS, default_value=0.25)
    t.insert(T(keys, dev), T(synth.rows_np(keys, dim, 2), dev))
    return t, keys


@pytest.fixture(scope="module")
def tables(dev):
    """{dim: (table, its keys)}: dim 64 and dim 16 (compiled row shapes), dim 24 (the run-time shape)"""
    return {dim: make_table(dev, dim, 40 + dim) for dim in (64, 16, 24)}


def batch(keys, seed, dev, n=BATCH):
    """n keys of the table, about 10 % absent ones and a few reserved keys among them"""
    rng = np.random.default_rng(seed)
    q = keys[rng.integers(0, keys.size, n)].copy()
    absent = rng.random(n) < 0.1
    q[absent] = synth.keys_np(1000 + seed, 0, int(absent.sum()))
    if n > 8:
        q[rng.integers(0, n, 3)] = oracle.EMPTY_KEY
        q[rng.integers(0, n, 2)] = oracle.EMPTY_KEY + 1   # the tombstone
    return T(q, dev)


def buffers(dev, dim, count, n=BATCH):
    """`count` (out, found) pairs holding values no lookup writes"""
    return [(torch.full((n, dim), -7.0, device=dev), torch.full((n,), 9, dtype=torch.uint8, device=dev)) for _ in range(count)]


def replayed(dev, prog):
    """prog() captured on a side stream (as bench.py captures its steps) and replayed once -> the graph"""
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        prog()
    g.replay()
    torch.cuda.synchronize(dev)
    return g


def stats_of(prog, table):
    """(nodes, merged) that prog() adds to the table's counters"""
    n0, m0 = table.find_capture_stats()
    prog()
    n1, m1 = table.find_capture_stats()
    return n1 - n0, m1 - m0


def same(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) and torch.equal(fx, fy) for (x, fx), (y, fy) in zip(a, b))


@pytest.mark.parametrize("dim", [64, 16, 24])
def test_five_finds_one_node(dev, tables, dim):
    t, keys = tables[dim]
    qs = [batch(keys, 10 + i, dev) for i in range(5)]
    eager, cap = buffers(dev, dim, 5), buffers(dev, dim, 5)
    for q, (o, f) in zip(qs, eager):
        t.find(q, out=o, found=f)
    graph = []
    got = stats_of(lambda: graph.append(replayed(dev, lambda: [t.find(q, out=o, found=f) for q, (o, f) in zip(qs, cap)])), t)
    assert got == (1, 4)
    assert same(eager, cap)
    assert cap[0][1].sum().item() < BATCH and cap[0][1].any()   # the batches do hold absent keys, and present ones
    # the node reads the key TENSORS: new keys written in place, a second replay follows them
    for i, q in enumerate(qs):
        q.copy_(batch(keys, 70 + i, dev))
    for q, (o, f) in zip(qs, eager):
        t.find(q, out=o, found=f)
    graph[0].replay()
    torch.cuda.synchronize(dev)
    assert same(eager, cap)


def test_rotating_buffers_last_writer_wins(dev, tables):
    """bench.py's shape in small: 13 finds rotate over 3 buffers; a call that would write a buffer of its node starts the next node"""
    t, keys = tables[64]
    qs = [batch(keys, 100 + i, dev) for i in range(13)]
    eager, cap = buffers(dev, 64, 3), buffers(dev, 64, 3)
    for i, q in enumerate(qs):
        t.find(q, out=eager[i % 3][0], found=eager[i % 3][1], flags=_lib.FIND_STREAM_STORES | _lib.FIND_STREAM_ROWS)
    got = stats_of(lambda: replayed(dev, lambda: [t.find(q, out=cap[i % 3][0], found=cap[i % 3][1], flags=_lib.FIND_STREAM_STORES | _lib.FIND_STREAM_ROWS)
                                                  for i, q in enumerate(qs)]), t)
    assert got == (5, 8)
    assert same(eager, cap)


def two_calls(dev, t, first, second, between=None):
    """first(bufs) [between()] second(bufs) eagerly and captured -> (nodes, merged) of the capture; asserts equal buffers"""
    eager, cap = buffers(dev, t.dim, 2), buffers(dev, t.dim, 2)

    def prog(bufs):
        first(bufs)
        if between:
            between(bufs)
        second(bufs)

    prog(eager)
    got = stats_of(lambda: replayed(dev, lambda: prog(cap)), t)
    assert same(eager, cap)
    return got


def test_keys_inside_an_earlier_output_do_not_merge(dev, tables):
    """the second call's keys are a view into the first call's output: inside one kernel the read would race with the write"""
    t, keys = tables[64]
    q = batch(keys, 200, dev)

    def second(bufs):
        k2 = bufs[0][0].view(-1)[: 2 * 500].view(torch.int64)   # 500 int64 keys made of the first 1000 floats of out 0 (rows of floats: absent keys)
        t.find(k2, out=bufs[1][0][:500], found=bufs[1][1][:500])

    assert two_calls(dev, t, lambda b: t.find(q, out=b[0][0], found=b[0][1]), second) == (2, 0)


def test_foreign_kernel_between_two_finds(dev, tables):
    t, keys = tables[64]
    q1, q2 = batch(keys, 210, dev), batch(keys, 211, dev)
    got = two_calls(dev, t, lambda b: t.find(q1, out=b[0][0], found=b[0][1]), lambda b: t.find(q2, out=b[1][0], found=b[1][1]),
                    between=lambda b: b[0][0].add_(0))
    assert got == (2, 0)


def test_different_flags_do_not_merge(dev, tables):
    t, keys = tables[64]
    q1, q2 = batch(keys, 220, dev), batch(keys, 221, dev)
    got = two_calls(dev, t, lambda b: t.find(q1, out=b[0][0], found=b[0][1], flags=_lib.FIND_STREAM_STORES),
                    lambda b: t.find(q2, out=b[1][0], found=b[1][1], flags=_lib.FIND_STREAM_STORES | _lib.FIND_STREAM_ROWS))
    assert got == (2, 0)


def test_two_tables_alternate(dev, tables):
    (t, keys), (u, ukeys) = tables[64], make_table(dev, 64, 77)
    qs = [batch(keys if i % 2 == 0 else ukeys, 230 + i, dev) for i in range(4)]
    eager, cap = buffers(dev, 64, 4), buffers(dev, 64, 4)

    def prog(bufs):
        for i, q in enumerate(qs):
            (t if i % 2 == 0 else u).find(q, out=bufs[i][0], found=bufs[i][1])

    prog(eager)
    u0 = u.find_capture_stats()
    assert stats_of(lambda: replayed(dev, lambda: prog(cap)), t) == (2, 0)
    assert u.find_capture_stats() == (u0[0] + 2, u0[1])
    assert same(eager, cap)


def test_insert_between_two_finds(dev):
    """the second find must see the rows an insert captured in front of it wrote (twin tables: one runs eagerly, one replays)"""
    (a, keys), (b, _) = make_table(dev, 64, 90), make_table(dev, 64, 90)
    q = batch(keys, 240, dev)
    new_keys = T(synth.keys_np(1240, 0, 100), dev)   # the absent keys of q come from this stream: some of them are found afterwards
    new_rows = torch.full((100, 64), 3.5, device=dev)
    eager, cap = buffers(dev, 64, 2), buffers(dev, 64, 2)

    def prog(t, bufs):
        t.find(q, out=bufs[0][0], found=bufs[0][1])
        t.insert(new_keys, new_rows)
        t.find(q, out=bufs[1][0], found=bufs[1][1])

    prog(a, eager)
    assert stats_of(lambda: replayed(dev, lambda: prog(b, cap)), b) == (2, 0)
    assert same(eager, cap)
    assert cap[1][1].sum().item() > cap[0][1].sum().item()


def test_found_on_one_call_only(dev, tables):
    """found = None on one call and not on the other: merged or not, the results are the eager ones"""
    t, keys = tables[64]
    q1, q2 = batch(keys, 250, dev), batch(keys, 251, dev)
    nodes, merged = two_calls(dev, t, lambda b: t.find(q1, out=b[0][0], found=None, want_found=False), lambda b: t.find(q2, out=b[1][0], found=b[1][1]))
    assert nodes + merged == 2


def test_empty_call(dev, tables):
    """an n = 0 call launches nothing and ends no node"""
    t, keys = tables[64]
    q1, q2, none = batch(keys, 260, dev), batch(keys, 261, dev), torch.empty(0, dtype=torch.int64, device=dev)
    got = two_calls(dev, t, lambda b: t.find(q1, out=b[0][0], found=b[0][1]), lambda b: t.find(q2, out=b[1][0], found=b[1][1]),
                    between=lambda b: t.find(none, out=b[1][0][:0], found=b[1][1][:0]))
    assert got == (1, 1)


def test_eighteen_finds_two_nodes(dev, tables):
    """a node holds at most 16 requests (kMaxFindRequests): the 17th call starts the second node"""
    t, keys = tables[16]
    qs = [batch(keys, 300 + i, dev, n=203) for i in range(18)]
    eager, cap = buffers(dev, 16, 18, n=203), buffers(dev, 16, 18, n=203)
    for q, (o, f) in zip(qs, eager):
        t.find(q, out=o, found=f)
    assert stats_of(lambda: replayed(dev, lambda: [t.find(q, out=o, found=f) for q, (o, f) in zip(qs, cap)]), t) == (2, 16)
    assert same(eager, cap)


def test_two_captures_one_after_the_other(dev, tables):
    """a capture id is never reused: the first find of the next capture gets a node of its own, in ITS graph"""
    t, keys = tables[64]
    qs = [batch(keys, 400 + i, dev) for i in range(4)]
    eager, cap = buffers(dev, 64, 4), buffers(dev, 64, 4)
    for q, (o, f) in zip(qs, eager):
        t.find(q, out=o, found=f)
    graphs = []
    for half in (0, 2):
        got = stats_of(lambda: graphs.append(replayed(dev, lambda: [t.find(qs[i], out=cap[i][0], found=cap[i][1]) for i in (half, half + 1)])), t)
        assert got == (1, 1)
    assert same(eager, cap)
    for o, f in cap:
        o.fill_(-7.0); f.fill_(9)
    for g in graphs:   # both graphs still replay what they captured
        g.replay()
    torch.cuda.synchronize(dev)
    assert same(eager, cap)


def test_coalescing_off_one_node_per_call(dev):
    t, keys = make_table(dev, 64, 91)
    t.set_tuning("find_coalesce", 0)
    qs = [batch(keys, 500 + i, dev) for i in range(4)]
    eager, cap = buffers(dev, 64, 4), buffers(dev, 64, 4)
    for q, (o, f) in zip(qs, eager):
        t.find(q, out=o, found=f)
    assert stats_of(lambda: replayed(dev, lambda: [t.find(q, out=o, found=f) for q, (o, f) in zip(qs, cap)]), t) == (4, 0)
    assert same(eager, cap)
    t.set_tuning("find_coalesce", 1)
    assert stats_of(lambda: replayed(dev, lambda: [t.find(q, out=o, found=f) for q, (o, f) in zip(qs, cap)]), t) == (1, 3)


def test_eager_calls_change_no_counter(dev, tables):
    t, keys = tables[64]
    bufs = buffers(dev, 64, 3)
    assert stats_of(lambda: [t.find(batch(keys, 600 + i, dev), out=o, found=f) for i, (o, f) in enumerate(bufs)], t) == (0, 0)
