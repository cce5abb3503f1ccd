"""GPU: admission over a table group (SPEC.md §3 group_find_or_insert_admit) — TableGroup.find_or_insert(min_count=), TableGroup.admission_decay and the
min_count of the three nn layers.  By definition the grouped operator is find_or_insert_admit of every member on its segment, each member counting in
its own sketch, so the expected behaviour is recomputed per member the way tests/test_gpu_parity.py::test_admission_policy does it for one table: a
numpy count-min sketch (oracle.pyspec.mix64, the three constants of SPEC §3) and one oracle.OracleTable per member.  Lookups copy rows: bit for bit."""
import numpy as np
import pytest
import torch

import oracle
from oracle import pyspec
from meepoembedding_amd import (INIT_UNIFORM, OPT_ADAGRAD, STATUS_RESERVED_KEY, STATUS_TABLE_FULL, LookupTable, MeepoError, TableGroup, _lib, synth)

pytestmark = pytest.mark.gpu
A = (0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9)
RTOL, ATOL = 1e-6, 1e-9   # SPEC.md §4: fp32 optimizer state
OUT_SENTINEL, FOUND_SENTINEL = 7.5, 9
N_MEMBERS, CAP, UNIVERSE = 3, 8192, 600
INIT_ACC = 0.125


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _sorted(planes):
    order = np.argsort(planes[0])
    return tuple(p[order] if p is not None else None for p in planes)


def _tables(dev, dim, caps=(CAP,) * N_MEMBERS, admission=True, max_batch=4096):
    """member j: UNIFORM initializer with its own seed and default row, Adagrad state"""
    return [LookupTable(c, dim, device=dev, optimizer=OPT_ADAGRAD, max_batch=max_batch, admission=admission, initializer=INIT_UNIFORM, init_scale=0.1,
                        init_seed=5 + j, default_value=-1.0 - j, initial_accumulator=INIT_ACC) for j, c in enumerate(caps)]


class Model:
    """find_or_insert_admit per member: its own sketch (width from ITS capacity) and its own oracle table"""

    def __init__(self, tables):
        self.dim = tables[0].dim
        self.oracles = [oracle.OracleTable(t.capacity, t.dim, optimizer=oracle.OPT_ADAGRAD, initializer=oracle.INIT_UNIFORM, init_scale=0.1,
                                           init_seed=5 + j, default_value=-1.0 - j, initial_accumulator=INIT_ACC) for j, t in enumerate(tables)]
        self.log2w = []
        for t in tables:
            w = 12
            while (1 << w) < (t.capacity + 15) // 16:
                w += 1
            self.log2w.append(w)
        self.sketch = [np.zeros((3, 1 << w), dtype=np.int64) for w in self.log2w]
        self._idx = {}
        self.created = [0] * len(tables)

    def idx(self, j, k):
        got = self._idx.get((j, int(k)))
        if got is None:
            got = self._idx[(j, int(k))] = tuple(pyspec.mix64((int(k) & (2**64 - 1)) ^ A[r]) >> (64 - self.log2w[j]) for r in range(3))
        return got

    def step(self, keys, offsets, min_counts):
        """-> (out, found) with the sentinels wherever the operator may not write, and the set of members whose segment held RECLAIMED"""
        n = keys.size
        out = np.full((n, self.dim), OUT_SENTINEL, np.float32)
        found = np.full(n, FOUND_SENTINEL, np.uint8)
        tomb = set()
        for j, o in enumerate(self.oracles):
            s, e = min(int(offsets[j]), n), min(int(offsets[j + 1]), n)
            if e <= s:
                continue
            seg = keys[s:e]
            _, ef = o.find(seg)                                   # present before the call
            absent = [k for k, f in zip(seg, ef) if not f and k > oracle.RECLAIMED_KEY]
            for k in absent:
                for r, c in enumerate(self.idx(j, k)):
                    self.sketch[j][r, c] += 1
            admit = sorted({int(k) for k in absent if min(self.sketch[j][r, c] for r, c in enumerate(self.idx(j, k))) >= min_counts[j]})
            if admit:
                o.find_or_insert(np.array(admit, dtype=np.int64))
                self.created[j] += len(admit)
            out[s:e], _ = o.find(seg)                             # rows after the admitted keys were created; the others: the default row
            found[s:e] = ef
            if (seg == oracle.RECLAIMED_KEY).any():
                tomb.add(j)
        return out, found, tomb

    def decay(self, shift):
        for s in self.sketch:
            s >>= shift


def _buffers(dev, n, dim, dtype=torch.float32):
    return (torch.full((n, dim), OUT_SENTINEL, dtype=dtype, device=dev), torch.full((n,), FOUND_SENTINEL, dtype=torch.uint8, device=dev))


def _batch(rng, universe, seg_lens, tomb_member, lead=5, tail=7):
    """a jagged Zipf(1.6) batch: offsets[0] = lead, offsets[T] = n - tail (the positions outside hold universe keys too), three EMPTY keys and one
    RECLAIMED key inside member tomb_member's segment"""
    n = lead + sum(seg_lens) + tail
    keys = universe[np.minimum(rng.zipf(1.6, size=n) - 1, universe.size - 1)].copy()
    offsets = np.concatenate([[lead], lead + np.cumsum(seg_lens)]).astype(np.int64)
    inside = np.arange(offsets[0], offsets[-1])
    keys[rng.choice(inside, 3, replace=False)] = oracle.EMPTY_KEY
    keys[int(offsets[tomb_member]) + 3] = oracle.RECLAIMED_KEY
    return keys, offsets


def _assert_exports(tables, model):
    for j, (t, o) in enumerate(zip(tables, model.oracles)):
        got, exp = _sorted([x.cpu().numpy() if x is not None else None for x in t.export(with_state=True)]), _sorted(o.export(with_state=True))
        assert np.array_equal(got[0], exp[0]), (j, got[0].size, exp[0].size)
        assert np.array_equal(got[1].view(np.uint32), exp[1].view(np.uint32)), j
        assert np.array_equal(got[2].view(np.uint32), exp[2].view(np.uint32)), j
        if got[0].size:
            assert np.all(got[2] == np.float32(INIT_ACC)), j   # the created keys carry the initial accumulator


def _parity(dev, dim, alternate):
    tables = _tables(dev, dim)
    group = TableGroup(tables)
    model = Model(tables)
    universe = synth.keys_np(61, 0, UNIVERSE)   # every member draws from the SAME keys: a wrong member's sketch or table shows
    rng = np.random.default_rng(8 + dim)
    seg_lens = (900, 0, 1200)
    for rnd in range(10):
        tomb_member = 2 if rnd % 2 else 0
        keys, offsets = _batch(rng, universe, seg_lens, tomb_member)
        n = keys.size
        out, found = _buffers(dev, n, dim)
        dk, doff = T(keys, dev), T(offsets, dev)
        if alternate and rnd % 2:   # the members' own operator on their segments: the group keeps no state of its own
            for j, t in enumerate(tables):
                s, e = int(offsets[j]), int(offsets[j + 1])
                if e > s:
                    t.find_or_insert(dk[s:e], out=out[s:e], found=found[s:e], min_count=3)
        else:
            group.find_or_insert(dk, doff, out=out, found=found, min_count=3)
        eo, ef, tomb = model.step(keys, offsets, [3] * N_MEMBERS)
        assert np.array_equal(found.cpu().numpy(), ef), rnd
        assert np.array_equal(out.cpu().numpy().view(np.uint32), eo.view(np.uint32)), rnd
        assert [t.size() for t in tables] == [o.size() for o in model.oracles], rnd
        if not (alternate and rnd % 2):
            assert tomb == {tomb_member}
            assert [t.status() for t in tables] == [STATUS_RESERVED_KEY if j == tomb_member else 0 for j in range(N_MEMBERS)], rnd
        for t in tables:
            t.clear_status()
        if rnd == 6:
            group.admission_decay(1)
            model.decay(1)
    _assert_exports(tables, model)
    assert 0 < model.created[0] < UNIVERSE and model.created[1] == 0 and 0 < model.created[2] < UNIVERSE   # neither all nor nothing admitted


@pytest.mark.parametrize("dim", [16, 64, 100])
def test_model_parity(dev, dim):
    """10 jagged Zipf rounds (900 / 0 / 1200 positions, 5 + 7 positions outside the segments, EMPTY and RECLAIMED keys), min_count = 3, a grouped decay
    after round 6: out bit for bit, found = present before, sizes, RESERVED_KEY on the member of the RECLAIMED key only, exports with state at the end.
    dim 16: one element group per row; 64: the dim-64 instance of the find; 100: the run-time width, two column steps."""
    _parity(dev, dim, alternate=False)


def test_group_uses_the_members_own_sketches(dev):
    """odd rounds through LookupTable.find_or_insert(min_count=) of the members, even rounds through the group: the same model keeps matching"""
    _parity(dev, 16, alternate=True)


def test_per_member_thresholds(dev):
    """[1, 3, 2^32 - 1]: member 0's segment is a twin group's find_or_insert bit for bit, member 1 follows the model, member 2 never creates; a scalar
    min_count = 0 behaves as 1 (= find_or_insert)."""
    dim, thr = 16, [1, 3, 2**32 - 1]
    tables, twins = _tables(dev, dim), _tables(dev, dim)
    group, twin = TableGroup(tables), TableGroup(twins)
    model = Model(tables)
    universe = synth.keys_np(62, 0, UNIVERSE)
    rng = np.random.default_rng(21)
    for rnd in range(5):
        keys, offsets = _batch(rng, universe, (500, 700, 600), 1)
        out, found = _buffers(dev, keys.size, dim)
        group.find_or_insert(T(keys, dev), T(offsets, dev), out=out, found=found, min_count=thr)
        eo, ef, _ = model.step(keys, offsets, thr)
        assert np.array_equal(found.cpu().numpy(), ef) and np.array_equal(out.cpu().numpy().view(np.uint32), eo.view(np.uint32)), rnd
        tout, tfound = twin.find_or_insert(T(keys, dev), T(offsets, dev))
        s, e = int(offsets[0]), int(offsets[1])
        assert torch.equal(out[s:e].view(torch.int32), tout[s:e].view(torch.int32)) and torch.equal(found[s:e], tfound[s:e]), rnd
        assert tables[0].size() == twins[0].size() and tables[1].size() == model.oracles[1].size() and tables[2].size() == 0, rnd
    assert 0 < tables[1].size() < twins[1].size()
    _assert_exports(tables, model)
    # scalar 0: at first sight, as 1 — and as the twin's find_or_insert
    zero, one = TableGroup(_tables(dev, dim)), TableGroup(_tables(dev, dim))
    keys, offsets = _batch(rng, universe, (300, 200, 100), 0)
    ref = TableGroup(_tables(dev, dim))
    eo, ef = ref.find_or_insert(T(keys, dev), T(offsets, dev))
    for g, c in ((zero, 0), (one, 1)):
        out, found = g.find_or_insert(T(keys, dev), T(offsets, dev), min_count=c)
        s, e = int(offsets[0]), int(offsets[-1])
        assert torch.equal(out[s:e].view(torch.int32), eo[s:e].view(torch.int32)) and torch.equal(found[s:e], ef[s:e]), c
        assert [t.size() for t in g.tables] == [t.size() for t in ref.tables], c


def test_one_batch_crosses_the_threshold(dev):
    """a new key that occurs three times in ONE batch (min_count = 3) is created in that call, all three occurrences return its initial row with
    found = 0; a key that occurs twice returns the default row and is absent afterwards"""
    dim = 16
    tables = _tables(dev, dim)
    group, model = TableGroup(tables), Model(tables)
    three, two = 1001, 2002
    keys = np.array([11, three, 12, two, three, 13, two, three, 14], dtype=np.int64)
    offsets = np.array([0, 1, 8, 9], dtype=np.int64)   # both keys in member 1's segment
    out, found = group.find_or_insert(T(keys, dev), T(offsets, dev), min_count=3)
    out, found = out.cpu().numpy(), found.cpu().numpy()
    assert not found.any()
    init, default = model.oracles[1].initial_row(three), np.full(dim, -2.0, np.float32)
    for i, k in enumerate(keys):
        assert np.array_equal(out[i], init if k == three else np.full(dim, -1.0 - (0 if i == 0 else 2 if i == 8 else 1), np.float32)), i
    assert [t.size() for t in tables] == [0, 1, 0]
    rows, present = tables[1].find(T(np.array([three, two], dtype=np.int64), dev))
    assert present.cpu().numpy().tolist() == [1, 0]
    assert np.array_equal(rows.cpu().numpy(), np.stack([init, default]))


def test_bf16_out_is_the_rounded_fp32_result(dev):
    dim = 64
    a, b = _tables(dev, dim), _tables(dev, dim)
    ga, gb = TableGroup(a), TableGroup(b)
    universe = synth.keys_np(63, 0, UNIVERSE)
    rng = np.random.default_rng(5)
    for rnd in range(4):
        keys, offsets = _batch(rng, universe, (700, 0, 900), 2)
        o16, f16 = _buffers(dev, keys.size, dim, torch.bfloat16)
        o32, f32 = _buffers(dev, keys.size, dim)
        ga.find_or_insert(T(keys, dev), T(offsets, dev), out=o16, found=f16, out_dtype=torch.bfloat16, min_count=2)
        gb.find_or_insert(T(keys, dev), T(offsets, dev), out=o32, found=f32, min_count=2)
        assert torch.equal(o16.view(torch.int16), o32.to(torch.bfloat16).view(torch.int16)) and torch.equal(f16, f32), rnd
    assert 0 < a[0].size() < UNIVERSE
    for ta, tb in zip(a, b):
        x, y = _sorted([p.cpu().numpy() for p in ta.export(with_state=True)[:3]]), _sorted([p.cpu().numpy() for p in tb.export(with_state=True)[:3]])
        assert all(np.array_equal(p.view(np.uint8), q.view(np.uint8)) for p, q in zip(x, y))


def test_full_member(dev):
    """a member of capacity 32 offered 100 admitted keys: TABLE_FULL on that member only, size == capacity, every row of its segment is the key's
    initial row or the default row (which keys found room is not asserted)"""
    dim = 16
    tables = _tables(dev, dim, caps=(CAP, 32, CAP))
    group, model = TableGroup(tables), Model(tables)
    keys = synth.keys_np(64, 0, 140)
    offsets = np.array([0, 20, 120, 140], dtype=np.int64)
    out, found = group.find_or_insert(T(keys, dev), T(offsets, dev), min_count=1)
    assert [t.status() for t in tables] == [0, STATUS_TABLE_FULL, 0]
    assert [t.size() for t in tables] == [20, tables[1].capacity, 20] and tables[1].capacity < 100
    out = out.cpu().numpy()
    assert not found.cpu().numpy().any()
    default, created = np.full(dim, -2.0, np.float32), 0
    for i in range(20, 120):
        init = model.oracles[1].initial_row(int(keys[i]))
        assert np.array_equal(out[i], init) or np.array_equal(out[i], default), i
        created += np.array_equal(out[i], init)
    assert created == tables[1].capacity
    for j in (0, 2):
        s, e = int(offsets[j]), int(offsets[j + 1])
        assert np.array_equal(out[s:e], np.stack([model.oracles[j].initial_row(int(k)) for k in keys[s:e]]))


def test_refusals_leave_everything_untouched(dev):
    dim = 16
    universe = synth.keys_np(65, 0, UNIVERSE)
    rng = np.random.default_rng(3)
    keys, offsets = _batch(rng, universe, (40, 30, 50), 0)
    dk, doff = T(keys, dev), T(offsets, dev)
    n = keys.size
    L = _lib.lib()

    def untouched(out, found, tables):
        assert bool((out == OUT_SENTINEL).all()) and bool((found == FOUND_SENTINEL).all()) and all(t.size() == 0 and t.status() == 0 for t in tables)

    # a member without admission: the message names it
    mixed = _tables(dev, dim)
    mixed[1] = LookupTable(CAP, dim, device=dev, optimizer=OPT_ADAGRAD, max_batch=4096)
    out, found = _buffers(dev, n, dim)
    with pytest.raises(MeepoError, match="member 1") as ei:
        TableGroup(mixed).find_or_insert(dk, doff, out=out, found=found, min_count=2)
    assert ei.value.code == _lib.ERR_UNSUPPORTED
    with pytest.raises(MeepoError, match="member 1"):
        TableGroup(mixed).admission_decay(1)
    untouched(out, found, mixed)
    # a bf16-row group
    serving = [LookupTable(CAP, dim, device=dev, max_batch=4096, value_dtype=torch.bfloat16) for _ in range(N_MEMBERS)]
    with pytest.raises(MeepoError) as ei:
        TableGroup(serving).find_or_insert(dk, doff, out=out, found=found, min_count=2)
    assert ei.value.code == _lib.ERR_UNSUPPORTED
    untouched(out, found, serving)
    # null out, n > max_apply_batch without a found buffer, a threshold list of the wrong length — on a group that then serves a valid call
    tables = _tables(dev, dim)
    group, model = TableGroup(tables, max_apply_batch=64), Model(tables)
    stream = torch.cuda.current_stream(dev).cuda_stream
    rc = L.mee_group_find_or_insert_admit(group._h, dk.data_ptr(), doff.data_ptr(), n, None, _lib.DTYPE_F32, found.data_ptr(), 2, None, stream)
    assert rc == _lib.ERR_INVALID_ARG
    assert n > 64
    rc = L.mee_group_find_or_insert_admit(group._h, dk.data_ptr(), doff.data_ptr(), n, out.data_ptr(), _lib.DTYPE_F32, None, 1, None, stream)
    assert rc == _lib.ERR_BATCH_TOO_LARGE
    with pytest.raises(ValueError, match="3 values"):
        group.find_or_insert(dk, doff, out=out, found=found, min_count=[2, 2])
    untouched(out, found, tables)
    for _ in range(2):   # the refused calls counted nothing: with min_count = 2 the first valid call admits only what it sees twice itself
        out, found = _buffers(dev, n, dim)
        group.find_or_insert(dk, doff, out=out, found=found, min_count=2)
        eo, ef, _ = model.step(keys, offsets, [2] * N_MEMBERS)
        assert np.array_equal(found.cpu().numpy(), ef) and np.array_equal(out.cpu().numpy().view(np.uint32), eo.view(np.uint32))
        assert [t.size() for t in tables] == [o.size() for o in model.oracles]
    # without a found buffer inside the limit: the group's own mask serves
    small = dk[:60].contiguous()
    soff = T(np.array([0, 20, 40, 60], dtype=np.int64), dev)
    out = torch.full((60, dim), OUT_SENTINEL, device=dev)
    rc = L.mee_group_find_or_insert_admit(group._h, small.data_ptr(), soff.data_ptr(), 60, out.data_ptr(), _lib.DTYPE_F32, None, 1, None, stream)
    assert rc == _lib.OK
    eo, _, _ = model.step(keys[:60], np.array([0, 20, 40, 60]), [1] * N_MEMBERS)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), eo.view(np.uint32))


def test_capture_and_replay(dev):
    """one warm-up call, then one captured call replayed twice (a linear chain of three launches): the model advanced by the same calls matches"""
    dim = 64
    tables = _tables(dev, dim)
    group, model = TableGroup(tables), Model(tables)
    universe = synth.keys_np(66, 0, UNIVERSE)
    keys, offsets = _batch(np.random.default_rng(17), universe, (800, 0, 700), 2)
    dk, doff = T(keys, dev), T(offsets, dev)
    out, found = _buffers(dev, keys.size, dim)
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        group.find_or_insert(dk, doff, out=out, found=found, min_count=3)   # warm-up, outside the capture
        model.step(keys, offsets, [3] * N_MEMBERS)
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            group.find_or_insert(dk, doff, out=out, found=found, min_count=3)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize(dev)
        eo, ef, _ = model.step(keys, offsets, [3] * N_MEMBERS)
        assert np.array_equal(found.cpu().numpy(), ef) and np.array_equal(out.cpu().numpy().view(np.uint32), eo.view(np.uint32))
        assert [t.size() for t in tables] == [o.size() for o in model.oracles]
    assert 0 < model.created[0] < UNIVERSE


# ---- the layers ------------------------------------------------------------------------------------------------------------------------------
LR, EPS = 0.05, 1e-10


def _layer_case(dev, dim, n_members, seed):
    tables = _tables(dev, dim, caps=(CAP,) * n_members)
    model = Model(tables)
    ids = synth.keys_np(seed, 0, 4 * n_members)        # no duplicates: every member gets 4 unseen ids
    other = synth.keys_np(seed + 1, 0, 4 * n_members)
    w = (np.arange(4 * n_members * dim, dtype=np.float32).reshape(-1, dim) % 13 - 6) / 8   # the grad of every row: loss = sum(out * w)
    return tables, model, ids, other, w


def _expect_after_two_steps(tables, model, ids, w):
    """step 2 created the ids and stepped them once: the oracle's find_or_insert + Adagrad step on the initial rows"""
    for j, (t, o) in enumerate(zip(tables, model.oracles)):
        seg = slice(4 * j, 4 * j + 4)
        o.find_or_insert(ids[seg])
        o.apply_adagrad(ids[seg], w[seg], LR, EPS)
        got, exp = _sorted([x.cpu().numpy() for x in t.export(with_state=True)[:3]]), _sorted(o.export(with_state=True)[:3])
        assert np.array_equal(got[0], exp[0]), j
        np.testing.assert_allclose(got[1], exp[1], rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(got[2], exp[2], rtol=RTOL, atol=ATOL)
        assert not np.array_equal(got[1], np.stack([o.initial_row(int(k)) for k in got[0]])), "the rows were trained"


def _two_steps(dev, layer, tables, model, ids, other, w, call, rows_of):
    """the same unseen ids stepped twice with min_count = 2, an eval forward (of these and of other unseen ids) in between"""
    defaults = np.concatenate([np.full((4, tables[0].dim), -1.0 - j, np.float32) for j in range(len(tables))])
    layer.train()
    out = call(layer, ids)
    assert np.array_equal(rows_of(out).detach().float().cpu().numpy(), defaults)   # step 1: default rows ...
    (out * T(w, dev).reshape(out.shape)).sum().backward()
    assert all(t.size() == 0 and t.status() == 0 for t in tables)                  # ... nothing created, the backward left nothing
    layer.eval()
    with torch.no_grad():
        assert np.array_equal(rows_of(call(layer, ids)).float().cpu().numpy(), defaults)
        call(layer, other)
    assert all(t.size() == 0 for t in tables)
    layer.train()
    out = call(layer, ids)                                                          # step 2: the second sighting admits
    inits = np.stack([model.oracles[i // 4].initial_row(int(k)) for i, k in enumerate(ids)])
    assert np.array_equal(rows_of(out).detach().float().cpu().numpy(), inits)
    (out * T(w, dev).reshape(out.shape)).sum().backward()
    _expect_after_two_steps(tables, model, ids, w)
    call(layer, other)                                                              # the eval forward counted nothing: a first training sighting
    assert all(t.size() == 4 for t in tables)


def test_collection_layer(dev):
    from meepoembedding_amd.nn import DynamicEmbeddingCollection
    tables, model, ids, other, w = _layer_case(dev, 16, N_MEMBERS, 70)
    group = TableGroup(tables, max_apply_batch=256)
    offsets = T(np.arange(0, 4 * N_MEMBERS + 1, 4, dtype=np.int64), dev)
    layer = DynamicEmbeddingCollection(group, optimizer="adagrad", lr=LR, eps=EPS, min_count=2)
    _two_steps(dev, layer, tables, model, ids, other, w, lambda m, k: m(T(k, dev), offsets), lambda o: o)


def test_bag_layer_over_a_group(dev):
    from meepoembedding_amd.nn import DynamicEmbeddingBag
    tables, model, ids, other, w = _layer_case(dev, 16, N_MEMBERS, 72)
    group = TableGroup(tables, max_apply_batch=256)
    bag_offsets = T(np.arange(0, 4 * N_MEMBERS + 1, dtype=np.int64), dev)   # one id per bag, four bags per member
    layer = DynamicEmbeddingBag(group, mode="sum", optimizer="adagrad", lr=LR, eps=EPS, create_missing=True, min_count=2)
    _two_steps(dev, layer, tables, model, ids, other, w, lambda m, k: m(T(k, dev), bag_offsets), lambda o: o)


def test_bag_layer_weighted_and_over_one_table(dev):
    """the creation call in front of the pooled lookup admits over a LookupTable too, and in the weighted path (weights of 1: the same sums)"""
    from meepoembedding_amd.nn import DynamicEmbeddingBag
    tables, model, ids, other, w = _layer_case(dev, 16, 1, 74)
    bag_offsets = T(np.arange(0, 5, dtype=np.int64), dev)
    layer = DynamicEmbeddingBag(tables[0], mode="sum", optimizer="adagrad", lr=LR, eps=EPS, create_missing=True, min_count=2)
    ones = torch.ones(4, device=dev)
    _two_steps(dev, layer, tables, model, ids, other, w, lambda m, k: m(T(k, dev), bag_offsets, per_sample_weights=ones), lambda o: o)


def test_embedding_layer(dev):
    from meepoembedding_amd.nn import DynamicEmbedding
    tables, model, ids, other, w = _layer_case(dev, 16, 1, 76)
    layer = DynamicEmbedding(tables[0], optimizer="adagrad", lr=LR, eps=EPS, min_count=2)
    _two_steps(dev, layer, tables, model, ids, other, w, lambda m, k: m(T(k, dev)), lambda o: o)


def test_layers_refuse_min_count_at_construction(dev):
    from meepoembedding_amd import MixedTableGroup, TieredLookupTable
    from meepoembedding_amd.nn import DynamicEmbedding, DynamicEmbeddingBag, DynamicEmbeddingCollection
    from meepoembedding_amd.sharded import ShardedTableGroup
    dim = 16
    tables = _tables(dev, dim)
    group = TableGroup(tables, max_apply_batch=64)
    with pytest.raises(ValueError, match="create_missing"):
        DynamicEmbeddingBag(group, min_count=2)
    plain = _tables(dev, dim, admission=False)
    with pytest.raises(ValueError, match="admission=True"):
        DynamicEmbedding(plain[0], min_count=2)
    with pytest.raises(ValueError, match="member 2"):
        DynamicEmbeddingCollection(TableGroup(tables[:2] + plain[2:]), min_count=2)
    with pytest.raises(ValueError, match="hot/cold"):
        DynamicEmbedding(TieredLookupTable(tables[0], tables[1]), min_count=2)
    wide = LookupTable(CAP, 32, device=dev, optimizer=OPT_ADAGRAD, max_batch=4096, admission=True)
    with pytest.raises(ValueError, match="mixed-width"):
        DynamicEmbeddingBag(MixedTableGroup([tables[0], wide], max_apply_batch=64), create_missing=True, min_count=2)
    sharded = ShardedTableGroup.__new__(ShardedTableGroup)   # only its type is looked at: the refusal comes before anything is exchanged
    with pytest.raises(ValueError, match="sharded"):
        DynamicEmbeddingCollection(sharded, min_count=2)
    with pytest.raises(ValueError, match="bf16"):
        DynamicEmbedding(tables[0], min_count=2, out_dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="2\\^32"):
        DynamicEmbeddingCollection(group, min_count=-1)
    assert all(t.size() == 0 for t in tables)
    # what is allowed: bf16 rows from the collection layer
    assert DynamicEmbeddingCollection(group, min_count=2, out_dtype=torch.bfloat16).min_count == 2
