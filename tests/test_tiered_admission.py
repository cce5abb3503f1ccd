"""GPU: admission over hot/cold pairs and collections of pairs (SPEC.md §3 "Tiering": the pair's sketch is its HOT table's) —
TieredLookupTable.find_or_insert / find_pooled(min_count=), TieredTableGroup.find_or_insert / find_pooled(min_count=), admission_decay,
mee_find_or_insert_admit_missing and the min_count of the layers.  The expected behaviour is recomputed as tests/test_group_admission.py does it:
per pair a numpy count-min sketch of the HOT table's width (oracle.pyspec.mix64, the three constants of SPEC §3) and ONE oracle.OracleTable holding
the union of both tiers.  Lookups copy rows: bit for bit."""
import numpy as np
import pytest
import torch

import oracle
from oracle import pyspec
from meepoembedding_amd import (INIT_UNIFORM, OPT_ADAGRAD, STATUS_RESERVED_KEY, STATUS_TABLE_FULL, LookupTable, TableGroup, TieredLookupTable,
                                TieredTableGroup, _lib, synth)

pytestmark = pytest.mark.gpu
A = (0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9)
RTOL, ATOL = 1e-6, 1e-9   # SPEC.md §4: fp32 optimizer state
OUT_SENTINEL, FOUND_SENTINEL = 7.5, 9
N_MEMBERS, UNIVERSE = 3, 240
HOT_CAPS, COLD_CAPS = (3000, 70000, 9000), (5000, 2000, 40000)   # member 1: hot sketch 2^13 wide, cold 2^12 — a sketch from the wrong tier shows
HOT_DEFAULT, COLD_DEFAULT = (-1.0, -2.0, -3.0), (9.0, 10.0, 11.0)   # a cold default row must never show
INIT_ACC = 0.125
HEAD, TAIL = 3, 2               # positions in front of offsets[0] and behind offsets[n_tables]: no segment holds them
SEGMENTS = ((37, 70, 5), (1, 0, 41))


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _sorted(planes):
    planes = [p.cpu().numpy() if isinstance(p, torch.Tensor) else p for p in planes]
    order = np.argsort(planes[0])
    return tuple(p[order] if p is not None else None for p in planes)


def _log2w(capacity):
    w = 12
    while (1 << w) < (capacity + 15) // 16:
        w += 1
    return w


def _universe():
    return synth.keys_np(91, 0, UNIVERSE)


def _placement(j):
    """member j's keys of the universe before the first call: (stored hot, stored cold); the rest is absent.  The classes rotate with j, so one key
    value is hot in one member, cold in the next and absent in the third"""
    u = _universe()
    cls = (np.arange(u.size) + j) % 3
    return u[cls == 0], u[cls == 1]


def _sequence(seed, rounds=6):
    """`rounds` jagged Zipf(1.3) batches over the universe, segments 37 / 70 / 5 and 1 / 0 / 41 in turn behind HEAD and in front of TAIL positions that
    no segment holds (they hold universe keys too); EMPTY and RECLAIMED inside the longest segment; in the first batch an absent key of member 1 twice"""
    rng = np.random.default_rng(seed)
    u = _universe()
    batches = []
    for rnd in range(rounds):
        lens = SEGMENTS[rnd % 2]
        n = HEAD + sum(lens) + TAIL
        keys = u[np.minimum(rng.zipf(1.3, size=n) - 1, u.size - 1)].copy()
        off = (HEAD + np.concatenate([[0], np.cumsum(lens)])).astype(np.int64)
        p = int(off[int(np.argmax(lens))])
        keys[p + 1], keys[p + 3] = oracle.EMPTY_KEY, oracle.RECLAIMED_KEY
        if rnd == 0:
            absent_in_1 = u[(np.arange(u.size) + 1) % 3 == 2]
            keys[p + 10] = keys[p + 30] = absent_in_1[-1]   # a rare key: it crosses min_count = 2 by repetition inside this batch
        batches.append((keys, off))
    return batches


class Model:
    """find_or_insert_admit per pair: a sketch of the HOT table's width and one oracle table holding the union of both tiers"""

    def __init__(self, dim, hot_capacities, seeds=(5, 6, 7), defaults=HOT_DEFAULT):
        self.dim = dim
        self.oracles = [oracle.OracleTable(1 << 16, dim, optimizer=oracle.OPT_ADAGRAD, initializer=oracle.INIT_UNIFORM, init_scale=0.1, init_seed=s,
                                           default_value=d, initial_accumulator=INIT_ACC) for s, d in zip(seeds, defaults)]
        self.log2w = [_log2w(c) for c in hot_capacities]
        self.sketch = [np.zeros((3, 1 << w), dtype=np.int64) for w in self.log2w]
        self._idx = {}
        self.counted_not_admitted, self.admitted_later, self.admitted_by_repetition = set(), set(), set()

    def idx(self, j, k):
        got = self._idx.get((j, int(k)))
        if got is None:
            got = self._idx[(j, int(k))] = tuple(pyspec.mix64((int(k) & (2**64 - 1)) ^ A[r]) >> (64 - self.log2w[j]) for r in range(3))
        return got

    def est(self, j, k):
        return min(self.sketch[j][r, c] for r, c in enumerate(self.idx(j, k)))

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
            _, ef = o.find(seg)                                   # present in either tier before the call
            absent = [int(k) for k, f in zip(seg, ef) if not f and k > oracle.RECLAIMED_KEY]
            before = {k: self.est(j, k) for k in set(absent)}
            for k in absent:
                for r, c in enumerate(self.idx(j, k)):
                    self.sketch[j][r, c] += 1
            admit = sorted(k for k in set(absent) if self.est(j, k) >= min_counts[j])
            for k in set(absent):
                if k not in admit:
                    self.counted_not_admitted.add((j, k))
                elif before[k] > 0 and (j, k) in self.counted_not_admitted:
                    self.admitted_later.add((j, k))
                elif before[k] == 0 and min_counts[j] > 1:
                    self.admitted_by_repetition.add((j, k))
            if admit:
                o.find_or_insert(np.array(admit, dtype=np.int64))
            out[s:e], _ = o.find(seg)                             # rows after the admitted keys were created; the others: the hot default row
            found[s:e] = ef
            if (seg == oracle.RECLAIMED_KEY).any():
                tomb.add(j)
        return out, found, tomb

    def decay(self, shift, members=None):
        for j in (range(len(self.sketch)) if members is None else members):
            self.sketch[j] >>= shift


def _pairs(dev, dim, hot_caps=HOT_CAPS, cold_caps=COLD_CAPS, fill=True, cold_seeds=(5, 6, 7), hot_key_limits=(None,) * N_MEMBERS, hot_admission=True,
           max_batch=4096):
    """pair j: hot in HBM with a sketch, cold rows in pinned host memory with a sketch of ITS OWN (never the pair's), one UNIFORM initializer seed per
    pair (5 + j; cold_seeds may differ), Adagrad state; with `fill` the hot and the cold keys of _placement stored with rows of their own"""
    pairs = []
    for j in range(len(hot_caps)):
        kw = dict(device=dev, optimizer=OPT_ADAGRAD, max_batch=max_batch, initializer=INIT_UNIFORM, init_scale=0.1, initial_accumulator=INIT_ACC)
        hot = LookupTable(hot_caps[j], dim, admission=hot_admission, init_seed=5 + j, default_value=HOT_DEFAULT[j], **kw)
        cold = LookupTable(cold_caps[j], dim, admission=True, init_seed=cold_seeds[j], default_value=COLD_DEFAULT[j], value_memory=_lib.MEM_HOST_PINNED, **kw)
        if fill:
            for t, k in zip((hot, cold), _placement(j)):
                t.insert(T(k, dev), T(synth.rows_np(k, dim, 3 + j), dev))
        pairs.append(TieredLookupTable(hot, cold, hot_key_limit=hot_key_limits[j]))
    return pairs


def _model(dim, pairs, fill=True, **kw):
    m = Model(dim, [p.hot.capacity for p in pairs], **kw)
    if fill:
        for j, o in enumerate(m.oracles):
            for k in _placement(j):
                o.insert(k, synth.rows_np(k, dim, 3 + j))
    return m


def _buffers(dev, n, dim, dtype=torch.float32):
    return (torch.full((n, dim), OUT_SENTINEL, dtype=dtype, device=dev), torch.full((n,), FOUND_SENTINEL, dtype=torch.uint8, device=dev))


def _assert_union(pairs, model, what=None):
    """the key-sorted union export with state is the model's, and no key sits in both tiers"""
    for j, (p, o) in enumerate(zip(pairs, model.oracles)):
        got, exp = _sorted(p.export(with_state=True)[:3]), _sorted(o.export(with_state=True)[:3])
        assert np.unique(got[0]).size == got[0].size, (what, j, "a key sits in both tiers")
        assert np.array_equal(got[0], exp[0]), (what, j, got[0].size, exp[0].size)
        assert np.array_equal(got[1].view(np.uint32), exp[1].view(np.uint32)), (what, j)
        assert np.array_equal(got[2].view(np.uint32), exp[2].view(np.uint32)), (what, j)


def _assert_status(pairs, hot_expected, what=None):
    assert [p.hot.status() for p in pairs] == hot_expected and [p.cold.status() for p in pairs] == [0] * len(pairs), what
    for p in pairs:
        p.hot.clear_status()


# ---- 1. the unpooled group against the model ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_count", [2, [1, 2, 3]])
@pytest.mark.parametrize("dim", [16, 64])
def test_group_against_the_model(dev, dim, min_count):
    """6 jagged Zipf batches: out and found bit for bit with the sentinels outside the segments, after every call the union export, one tier per key
    and the status words; a bf16 twin returns the fp32 result rounded once and leaves the same tables"""
    pairs, twins = _pairs(dev, dim), _pairs(dev, dim)
    group, twin = TieredTableGroup(pairs), TieredTableGroup(twins)
    model = _model(dim, pairs)
    assert model.log2w[1] == 13 and _log2w(pairs[1].cold.capacity) == 12 and len({p.hot.capacity for p in pairs}) == N_MEMBERS
    thr = [min_count] * N_MEMBERS if isinstance(min_count, int) else min_count
    for rnd, (keys, offsets) in enumerate(_sequence(17 + dim)):
        n = keys.size
        out, found = _buffers(dev, n, dim)
        o16, f16 = _buffers(dev, n, dim, torch.bfloat16)
        group.find_or_insert(T(keys, dev), T(offsets, dev), out=out, found=found, min_count=min_count)
        twin.find_or_insert(T(keys, dev), T(offsets, dev), out=o16, found=f16, out_dtype=torch.bfloat16, min_count=min_count)
        eo, ef, tomb = model.step(keys, offsets, thr)
        assert np.array_equal(found.cpu().numpy(), ef), rnd
        got = out.cpu().numpy()
        assert np.array_equal(got.view(np.uint32), eo.view(np.uint32)), rnd
        for j in range(N_MEMBERS):
            s, e = int(offsets[j]), int(offsets[j + 1])
            assert not (got[s:e] == np.float32(COLD_DEFAULT[j])).all(axis=1).any(), (rnd, j)   # a cold default row is never returned
        assert torch.equal(o16.view(torch.int16), out.to(torch.bfloat16).view(torch.int16)) and torch.equal(f16, found), rnd
        _assert_union(pairs, model, rnd)
        _assert_status(pairs, [STATUS_RESERVED_KEY if j in tomb else 0 for j in range(N_MEMBERS)], rnd)   # the hot table was asked to create
        _assert_status(twins, [STATUS_RESERVED_KEY if j in tomb else 0 for j in range(N_MEMBERS)], rnd)
    _assert_union(twins, model, "bf16 twin")
    # the sequence held all three: counted but not admitted, admitted on a later call, admitted inside one call by repetition
    assert model.counted_not_admitted and model.admitted_later and model.admitted_by_repetition
    assert all(p.cold.size() == _placement(j)[1].size for j, p in enumerate(pairs))   # room in every hot tier: nothing was created cold
    # the cold tables' own sketches were never counted in: a fresh key asked for twice through the group (hot count 2, threshold 3) is at count 1 in
    # the cold table's own sketch after one direct request there
    fresh = T(np.array([424242], dtype=np.int64), dev)
    off = T(np.array([0, 0, 1, 1], dtype=np.int64), dev)
    for _ in range(2):
        group.find_or_insert(fresh, off, min_count=3)
    before = pairs[1].cold.size()
    pairs[1].cold.find_or_insert(fresh, min_count=2)
    assert pairs[1].cold.size() == before


# ---- 2. placement ---------------------------------------------------------------------------------------------------------------------------------
def test_admitted_keys_go_to_the_tier_the_pair_picks(dev):
    """member 1's hot_key_limit is 0: its admitted keys are created cold, with the COLD table's initial rows (another seed), while the counts sit in
    its HOT sketch (a decay of the hot table alone takes them back); the other members create hot"""
    dim = 16
    pairs = _pairs(dev, dim, fill=False, cold_seeds=(5, 99, 7), hot_key_limits=(None, 0, None))
    group = TieredTableGroup(pairs)
    cold_init = oracle.OracleTable(64, dim, optimizer=oracle.OPT_ADAGRAD, initializer=oracle.INIT_UNIFORM, init_scale=0.1, init_seed=99, initial_accumulator=INIT_ACC)
    hot_init = [oracle.OracleTable(64, dim, optimizer=oracle.OPT_ADAGRAD, initializer=oracle.INIT_UNIFORM, init_scale=0.1, init_seed=5 + j,
                                   initial_accumulator=INIT_ACC) for j in range(N_MEMBERS)]
    keys = synth.keys_np(92, 0, 30)
    dk, off = T(keys, dev), T(np.array([0, 10, 20, 30], dtype=np.int64), dev)
    defaults = np.concatenate([np.full((10, dim), HOT_DEFAULT[j], np.float32) for j in range(N_MEMBERS)])
    out, found = group.find_or_insert(dk, off, min_count=2)
    assert np.array_equal(out.cpu().numpy(), defaults) and not found.any() and group.size() == 0
    pairs[1].hot.admission_decay(32)          # member 1's counts were in its hot sketch: gone
    out, found = group.find_or_insert(dk, off, min_count=2)
    exp = defaults.copy()
    for j in (0, 2):
        exp[10 * j:10 * j + 10] = np.stack([hot_init[j].initial_row(int(k)) for k in keys[10 * j:10 * j + 10]])
    assert np.array_equal(out.cpu().numpy().view(np.uint32), exp.view(np.uint32)) and not found.any()
    assert [(p.hot.size(), p.cold.size()) for p in pairs] == [(10, 0), (0, 0), (10, 0)]
    out, found = group.find_or_insert(dk, off, min_count=2)
    exp[10:20] = np.stack([cold_init.initial_row(int(k)) for k in keys[10:20]])     # the cold table's initial rows
    assert np.array_equal(out.cpu().numpy().view(np.uint32), exp.view(np.uint32))
    assert found.cpu().numpy().tolist() == [1] * 10 + [0] * 10 + [1] * 10
    assert [(p.hot.size(), p.cold.size()) for p in pairs] == [(10, 0), (0, 10), (10, 0)]
    ck, cv, cs = _sorted(pairs[1].cold.export(with_state=True)[:3])
    assert np.array_equal(ck, np.sort(keys[10:20])) and np.all(cs == np.float32(INIT_ACC))
    assert np.array_equal(cv.view(np.uint32), np.stack([cold_init.initial_row(int(k)) for k in ck]).view(np.uint32))
    assert all(p.hot.status() == 0 and p.cold.status() == 0 for p in pairs)


# ---- 3. min_count 0 and 1 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_count", [0, 1])
def test_first_sight_is_the_non_admitting_operator(dev, min_count):
    """on independent copies of the pairs: rows, found, both tiers' exports and every status word; and the sketch was still counted"""
    dim = 16
    limits = (None, 0, None)   # member 1 creates cold
    a, b = _pairs(dev, dim, hot_key_limits=limits), _pairs(dev, dim, hot_key_limits=limits)
    ga, gb = TieredTableGroup(a), TieredTableGroup(b)
    for rnd, (keys, offsets) in enumerate(_sequence(5, rounds=2)):
        oa, fa = _buffers(dev, keys.size, dim)
        ob, fb = _buffers(dev, keys.size, dim)
        ga.find_or_insert(T(keys, dev), T(offsets, dev), out=oa, found=fa, min_count=min_count)
        gb.find_or_insert(T(keys, dev), T(offsets, dev), out=ob, found=fb)
        assert torch.equal(oa.view(torch.int32), ob.view(torch.int32)) and torch.equal(fa, fb), rnd
        for j, (pa, pb) in enumerate(zip(a, b)):
            for tier in ("hot", "cold"):
                x, y = _sorted(getattr(pa, tier).export(with_state=True)[:3]), _sorted(getattr(pb, tier).export(with_state=True)[:3])
                assert all(np.array_equal(p.view(np.uint8), q.view(np.uint8)) for p, q in zip(x, y)), (rnd, j, tier)
                assert getattr(pa, tier).status() == getattr(pb, tier).status(), (rnd, j, tier)
        assert any(p.hot.status() | p.cold.status() for p in a), "a RECLAIMED key was flagged somewhere"
        for p in a + b:
            p.hot.clear_status(); p.cold.clear_status()
    # a key the calls created at first sight was counted once: removed, ONE more request with min_count = 2 admits it — a key never asked for is not
    keys, offsets = _sequence(5, rounds=1)[0]
    s, e = int(offsets[0]), int(offsets[1])
    ref = _model(dim, a)
    _, ef = ref.oracles[0].find(keys[s:e])
    k = int(next(k for k, f in zip(keys[s:e], ef) if not f and k > oracle.RECLAIMED_KEY and np.sum(keys[s:e] == k) == 1))
    dk = T(np.array([k, 424242], dtype=np.int64), dev)
    assert a[0].remove(dk).cpu().numpy().tolist() == [1, 0]
    size = a[0].size()
    out, found = ga.find_or_insert(dk, T(np.array([0, 2, 2, 2], dtype=np.int64), dev), min_count=2)
    assert found.cpu().numpy().tolist() == [0, 0] and a[0].size() == size + 1
    assert np.array_equal(out.cpu().numpy(), np.stack([ref.oracles[0].initial_row(k), np.full(dim, HOT_DEFAULT[0], np.float32)]))


# ---- 4. admission_decay, and the group keeps no counters -------------------------------------------------------------------------------------------
def test_decay_and_interleaving_with_the_pairs_own_calls(dev):
    """group calls, the pairs' own find_or_insert(min_count=) on their segments, the group's decay and one pair's decay: one model keeps matching"""
    dim = 16
    pairs = _pairs(dev, dim)
    group, model = TieredTableGroup(pairs), _model(dim, pairs)
    batches = _sequence(29, rounds=4)
    for rnd in range(8):
        keys, offsets = batches[rnd % 4]
        dk = T(keys, dev)
        out, found = _buffers(dev, keys.size, dim)
        if rnd % 2:
            for j, p in enumerate(pairs):
                s, e = int(offsets[j]), int(offsets[j + 1])
                if e > s:
                    o, f = p.find_or_insert(dk[s:e], min_count=3)
                    out[s:e], found[s:e] = o, f
        else:
            group.find_or_insert(dk, T(offsets, dev), out=out, found=found, min_count=3)
        eo, ef, _ = model.step(keys, offsets, [3] * N_MEMBERS)
        assert np.array_equal(found.cpu().numpy(), ef) and np.array_equal(out.cpu().numpy().view(np.uint32), eo.view(np.uint32)), rnd
        if rnd == 2:
            group.admission_decay(1); model.decay(1)
        if rnd == 4:
            pairs[2].admission_decay(1); model.decay(1, members=[2])
        for p in pairs:
            p.hot.clear_status()
    _assert_union(pairs, model)
    assert model.counted_not_admitted and model.admitted_later


# ---- 5. pooled ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["sum", "mean"])
def test_pooled_lookup_admits_in_its_creation_pass(dev, mode):
    """find_pooled(insert_missing=True, min_count=2) on the group (two bags per member) and on one pair: bags that span admitted keys (asked for once
    before, or twice in this batch), keys not yet admitted (they pool as the hot default row) and cold keys; found = present before"""
    dim = 64
    pairs = _pairs(dev, dim)
    group, model = TieredTableGroup(pairs), _model(dim, pairs)
    segs = []
    for j in range(N_MEMBERS):
        hot, cold = _placement(j)
        absent = np.setdiff1d(_universe(), np.concatenate([hot, cold]))
        # bag 0: cold, absent a (seen before), hot, absent b twice, absent c (first sight), cold — 20 keys, a long bag; bag 1: absent c again is NOT here
        bag0 = np.concatenate([cold[:3], absent[:1], hot[:4], absent[1:2], cold[3:9], absent[1:2], absent[2:3], hot[4:6], cold[9:10]])
        bag1 = np.concatenate([hot[6:8], absent[3:4]])
        segs.append((bag0, bag1, absent))
    keys = np.concatenate([np.concatenate([b0, b1]) for b0, b1, _ in segs])
    lens = np.concatenate([[b0.size, b1.size] for b0, b1, _ in segs])
    bag_offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    member_offsets = bag_offsets[::2]
    # `absent a` of every member is asked for once before (unpooled, through the group): counted, not admitted
    first = np.array([a[0] for _, _, a in segs], dtype=np.int64)
    foff = np.arange(N_MEMBERS + 1, dtype=np.int64)
    group.find_or_insert(T(first, dev), T(foff, dev), min_count=2)
    model.step(first, foff, [2] * N_MEMBERS)
    assert group.size() == sum(o.size() for o in model.oracles)
    out, found = group.find_pooled(T(keys, dev), T(bag_offsets, dev), mode, insert_missing=True, min_count=2)
    rows, ef, _ = model.step(keys, member_offsets, [2] * N_MEMBERS)
    exp = oracle.pool_rows(rows, bag_offsets, mode)
    assert np.array_equal(found.cpu().numpy(), ef)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), exp.view(np.uint32))
    _assert_union(pairs, model)
    for j, (_, _, absent) in enumerate(segs):   # a and b were admitted, c and the key of bag 1 were not
        _, f = pairs[j].find(T(absent[:4], dev))
        assert f.cpu().numpy().tolist() == [1, 1, 0, 0], j
    # one pair on its own bags, one call later: c is admitted now, bit for bit the model's rows pooled
    j = 1
    b0, b1, _ = segs[j]
    pk, poff = np.concatenate([b0, b1]), np.array([0, b0.size, b0.size + b1.size], dtype=np.int64)
    out, found = pairs[j].find_pooled(T(pk, dev), T(poff, dev), mode, insert_missing=True, min_count=2)
    solo = Model(dim, [pairs[j].hot.capacity])
    solo.oracles, solo.sketch = [model.oracles[j]], [model.sketch[j]]
    rows, ef, _ = solo.step(pk, np.array([0, pk.size]), [2])
    assert np.array_equal(found.cpu().numpy(), ef)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), oracle.pool_rows(rows, poff, mode).view(np.uint32))
    _assert_union(pairs, model)


# ---- 6. a full tier -------------------------------------------------------------------------------------------------------------------------------
def test_full_tier(dev):
    """member 1's hot table has 32 slots and is asked to create 100 admitted keys: TABLE_FULL on that hot table only, the keys that found no room read
    the hot default row and are absent afterwards — from both tiers"""
    dim = 16
    pairs = _pairs(dev, dim, hot_caps=(3000, 32, 9000), fill=False, hot_key_limits=(None, 1 << 20, None))
    group = TieredTableGroup(pairs)
    init = oracle.OracleTable(64, dim, optimizer=oracle.OPT_ADAGRAD, initializer=oracle.INIT_UNIFORM, init_scale=0.1, init_seed=6, initial_accumulator=INIT_ACC)
    keys = synth.keys_np(93, 0, 140)
    dk, off = T(keys, dev), T(np.array([0, 20, 120, 140], dtype=np.int64), dev)
    out, found = group.find_or_insert(dk, off, min_count=1)
    assert [p.hot.status() for p in pairs] == [0, STATUS_TABLE_FULL, 0] and [p.cold.status() for p in pairs] == [0, 0, 0]
    assert [(p.hot.size(), p.cold.size()) for p in pairs] == [(20, 0), (pairs[1].hot.capacity, 0), (20, 0)] and pairs[1].hot.capacity < 100
    out = out.cpu().numpy()
    assert not found.cpu().numpy().any()
    default = np.full(dim, HOT_DEFAULT[1], np.float32)
    created = np.array([np.array_equal(out[i], init.initial_row(int(keys[i]))) for i in range(20, 120)])
    assert all(c or np.array_equal(out[i], default) for i, c in zip(range(20, 120), created)) and created.sum() == pairs[1].hot.capacity
    _, present = pairs[1].find(dk[20:120])
    assert np.array_equal(present.cpu().numpy().astype(bool), created)   # default row <=> stayed absent


# ---- 7. the C-ABI's admitting creation on a found mask ---------------------------------------------------------------------------------------------
def test_admit_missing_counts_in_one_table_and_creates_in_another(dev):
    dim = 16
    L = _lib.lib()
    kw = dict(device=dev, optimizer=OPT_ADAGRAD, max_batch=64, initializer=INIT_UNIFORM, init_scale=0.1, initial_accumulator=INIT_ACC)
    counts = LookupTable(4096, dim, admission=True, init_seed=1, default_value=-1.0, **kw)
    t = LookupTable(2048, dim, init_seed=2, default_value=-5.0, **kw)                      # creates; has no sketch of its own
    init = oracle.OracleTable(64, dim, optimizer=oracle.OPT_ADAGRAD, initializer=oracle.INIT_UNIFORM, init_scale=0.1, init_seed=2, initial_accumulator=INIT_ACC)
    stored = synth.keys_np(94, 0, 4)
    counts.insert(T(stored, dev), T(synth.rows_np(stored, dim, 1), dev))
    new = synth.keys_np(95, 0, 5)
    keys = np.concatenate([stored[:2], new[:3], [oracle.RECLAIMED_KEY, oracle.EMPTY_KEY], new[2:3], new[3:5]])   # new[2] twice: admitted in call 1
    dk = T(keys, dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def call(table, sketch_of, min_count, n=keys.size):
        out, found = counts.find(dk)
        rows = out.clone()
        rc = L.mee_find_or_insert_admit_missing(table._h, sketch_of._h, dk.data_ptr(), n, out.data_ptr(), found.data_ptr(), min_count, stream)
        return rc, rows.cpu().numpy(), out.cpu().numpy(), found.cpu().numpy()

    rc, rows, out, found = call(t, counts, 2)
    assert rc == _lib.OK and found.tolist() == [1, 1] + [0] * 8
    twice = [i for i, k in enumerate(keys) if k == new[2]]
    for i in range(keys.size):   # everything but the admitted key's positions is left as the find wrote it
        assert np.array_equal(out[i], init.initial_row(int(new[2])) if i in twice else rows[i]), i
    assert t.size() == 1 and counts.size() == 4 and t.status() == STATUS_RESERVED_KEY and counts.status() == 0
    t.clear_status()
    rc, rows, out, found = call(t, counts, 2)      # second sighting of the others; new[2] is in t, which this find did not ask: found says 0, the row is met
    assert rc == _lib.OK and t.size() == 5
    for i, k in enumerate(keys):
        assert np.array_equal(out[i], init.initial_row(int(k)) if k in new else rows[i]), i
    ek, ev, es = _sorted(t.export(with_state=True)[:3])
    assert np.array_equal(ek, np.sort(new)) and np.all(es == np.float32(INIT_ACC))
    assert np.array_equal(ev.view(np.uint32), np.stack([init.initial_row(int(k)) for k in ek]).view(np.uint32))
    # counts == t is legal: the single table's admission on a found mask
    fresh = T(synth.keys_np(96, 0, 3), dev)
    for expect in (4, 7):
        out, found = counts.find(fresh)
        assert L.mee_find_or_insert_admit_missing(counts._h, counts._h, fresh.data_ptr(), 3, out.data_ptr(), found.data_ptr(), 2, stream) == _lib.OK
        assert counts.size() == expect


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_untouched(dev):
    dim = 16
    L = _lib.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    keys, offsets = _sequence(3, rounds=1)[0]
    dk, doff = T(keys, dev), T(offsets, dev)
    n = keys.size

    def untouched(out, found, tables):
        assert bool((out == OUT_SENTINEL).all()) and bool((found == FOUND_SENTINEL).all()) and all(t.size() == 0 and t.status() == 0 for t in tables)

    # a hot member without a sketch: the message names it; a cold member without one is fine
    pairs = _pairs(dev, dim, fill=False)
    pairs[1] = TieredLookupTable(LookupTable(4096, dim, device=dev, optimizer=OPT_ADAGRAD, max_batch=4096), pairs[1].cold)
    group = TieredTableGroup(pairs)
    tables = [t for p in pairs for t in (p.hot, p.cold)]
    out, found = _buffers(dev, n, dim)
    with pytest.raises(ValueError, match="member 1"):
        group.find_or_insert(dk, doff, out=out, found=found, min_count=2)
    with pytest.raises(ValueError, match="member 1"):
        group.find_pooled(dk[:4], T(np.array([0, 1, 2, 4], dtype=np.int64), dev), insert_missing=True, min_count=2)
    with pytest.raises(ValueError, match="member 1"):
        group.admission_decay()
    with pytest.raises(ValueError, match="hot table"):
        pairs[1].find_or_insert(dk, min_count=2)
    assert not pairs[1].admission and pairs[0].admission
    hot, cold = group.hot_group._h, group.cold_group._h
    rc = L.mee_group_find_or_insert_admit_tiered(hot, cold, dk.data_ptr(), doff.data_ptr(), n, out.data_ptr(), _lib.DTYPE_F32, found.data_ptr(), None, 2, None, 0, stream)
    assert rc == _lib.ERR_UNSUPPORTED and "member 1" in L.mee_last_error().decode()
    rc = L.mee_group_ensure_admit_tiered(hot, cold, dk.data_ptr(), 4, doff.data_ptr(), 1, found.data_ptr(), None, 2, None, stream)
    assert rc == _lib.ERR_UNSUPPORTED and "member 1" in L.mee_last_error().decode()
    untouched(out, found, tables)
    nosketch = TieredTableGroup([TieredLookupTable(p.hot, LookupTable(4096, dim, device=dev, optimizer=OPT_ADAGRAD, max_batch=4096)) for p in _pairs(dev, dim, fill=False)])
    nosketch.find_or_insert(dk, doff, min_count=1)
    assert nosketch.size() > 0
    # bf16-row groups, bf16-row and int8-row tables
    full = _pairs(dev, dim, fill=False)
    good = TableGroup([p.hot for p in full])
    serving = TableGroup([LookupTable(4096, dim, device=dev, max_batch=4096, value_dtype=torch.bfloat16) for _ in range(N_MEMBERS)])
    for h, c in ((serving._h, good._h), (good._h, serving._h)):
        rc = L.mee_group_find_or_insert_admit_tiered(h, c, dk.data_ptr(), doff.data_ptr(), n, out.data_ptr(), _lib.DTYPE_F32, found.data_ptr(), None, 2, None, 0, stream)
        assert rc == _lib.ERR_UNSUPPORTED
        rc = L.mee_group_ensure_admit_tiered(h, c, dk.data_ptr(), 4, doff.data_ptr(), 1, found.data_ptr(), None, 2, None, stream)
        assert rc == _lib.ERR_UNSUPPORTED
    narrow = [LookupTable(4096, dim, device=dev, max_batch=4096, value_dtype=torch.bfloat16), LookupTable(4096, dim, device=dev, max_batch=4096, int8_rows=True)]
    for t in narrow:
        for a, b in ((t, full[0].hot), (full[0].hot, t)):
            assert L.mee_find_or_insert_admit_missing(a._h, b._h, dk.data_ptr(), n, out.data_ptr(), found.data_ptr(), 2, stream) == _lib.ERR_UNSUPPORTED
    # the counting table has no sketch; n over the creating table's batch limit; a null found mask
    assert L.mee_find_or_insert_admit_missing(full[0].hot._h, narrow[0]._h, dk.data_ptr(), n, out.data_ptr(), found.data_ptr(), 2, stream) == _lib.ERR_UNSUPPORTED
    plain = LookupTable(4096, dim, device=dev, optimizer=OPT_ADAGRAD, max_batch=4096)
    assert L.mee_find_or_insert_admit_missing(full[0].hot._h, plain._h, dk.data_ptr(), n, out.data_ptr(), found.data_ptr(), 2, stream) == _lib.ERR_UNSUPPORTED
    small = LookupTable(4096, dim, device=dev, optimizer=OPT_ADAGRAD, max_batch=64)
    assert n > small.max_batch
    assert L.mee_find_or_insert_admit_missing(small._h, full[0].hot._h, dk.data_ptr(), n, out.data_ptr(), found.data_ptr(), 2, stream) == _lib.ERR_BATCH_TOO_LARGE
    assert L.mee_find_or_insert_admit_missing(full[0].cold._h, full[0].hot._h, dk.data_ptr(), n, out.data_ptr(), None, 2, stream) == _lib.ERR_INVALID_ARG
    cold_group = TableGroup([p.cold for p in full])
    rc = L.mee_group_find_or_insert_admit_tiered(good._h, cold_group._h, dk.data_ptr(), doff.data_ptr(), n, out.data_ptr(), _lib.DTYPE_F32, None,
                                                 None, 2, None, 0, stream)
    assert rc == _lib.ERR_INVALID_ARG   # the found mask is required
    untouched(out, found, [t for p in full for t in (p.hot, p.cold)] + narrow + [plain, small])
    # the refused calls counted nothing: with min_count = 2 the first valid call admits only what it sees twice itself
    model = _model(dim, full, fill=False)
    valid = TieredTableGroup(full)
    for _ in range(2):
        out, found = _buffers(dev, n, dim)
        valid.find_or_insert(dk, doff, out=out, found=found, min_count=2)
        eo, ef, _ = model.step(keys, offsets, [2] * N_MEMBERS)
        assert np.array_equal(found.cpu().numpy(), ef) and np.array_equal(out.cpu().numpy().view(np.uint32), eo.view(np.uint32))
    _assert_union(full, model)


def test_capture_and_replay(dev):
    """no host synchronisation and no allocation: one warm-up call, then one captured call replayed twice (a linear chain of three launches); the
    model advanced by the same calls matches"""
    dim = 64
    pairs = _pairs(dev, dim)
    group, model = TieredTableGroup(pairs), _model(dim, pairs)
    keys, offsets = _sequence(41, rounds=1)[0]
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
    _assert_union(pairs, model)
    assert model.admitted_later


# ---- 9. the layers --------------------------------------------------------------------------------------------------------------------------------
LR, EPS = 0.05, 1e-10


def _layer_case(dev, dim, seed):
    pairs = _pairs(dev, dim, fill=False, hot_key_limits=(None, 0, None))   # member 1 creates cold
    model = _model(dim, pairs, fill=False)
    ids = synth.keys_np(seed, 0, 4 * N_MEMBERS)        # no duplicates: every member gets 4 unseen ids
    w = (np.arange(4 * N_MEMBERS * dim, dtype=np.float32).reshape(-1, dim) % 13 - 6) / 8   # the grad of every row: loss = sum(out * w)
    return pairs, model, ids, w


def _two_steps(dev, layer, pairs, model, ids, w, call):
    """the same unseen ids stepped twice with min_count = 2: default rows and no update first, then the initial rows and one Adagrad step"""
    dim = pairs[0].dim
    defaults = np.concatenate([np.full((4, dim), HOT_DEFAULT[j], np.float32) for j in range(len(pairs))])
    layer.train()
    out = call(layer, ids)
    assert np.array_equal(out.detach().float().cpu().numpy(), defaults)
    (out * T(w, dev).reshape(out.shape)).sum().backward()
    assert all(p.size() == 0 and p.hot.status() == 0 and p.cold.status() == 0 for p in pairs)   # an unadmitted id receives no update: there is no row
    layer.eval()
    with torch.no_grad():
        assert np.array_equal(call(layer, ids).float().cpu().numpy(), defaults)   # eval counts nothing
    layer.train()
    out = call(layer, ids)                                                        # the second training sighting admits
    for j, o in enumerate(model.oracles):
        o.find_or_insert(ids[4 * j:4 * j + 4])
    inits = np.stack([model.oracles[i // 4].initial_row(int(k)) for i, k in enumerate(ids)])
    assert np.array_equal(out.detach().float().cpu().numpy(), inits)
    (out * T(w, dev).reshape(out.shape)).sum().backward()
    for j, (p, o) in enumerate(zip(pairs, model.oracles)):
        o.apply_adagrad(ids[4 * j:4 * j + 4], w[4 * j:4 * j + 4], LR, EPS)
        got, exp = _sorted(p.export(with_state=True)[:3]), _sorted(o.export(with_state=True)[:3])
        assert np.array_equal(got[0], exp[0]), j
        np.testing.assert_allclose(got[1], exp[1], rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(got[2], exp[2], rtol=RTOL, atol=ATOL)
        assert not np.array_equal(got[1], np.stack([o.initial_row(int(k)) for k in got[0]])), "the rows were trained"
    assert [(p.hot.size(), p.cold.size()) for p in pairs] == [(4, 0), (0, 4), (4, 0)][:len(pairs)]


def test_collection_layer(dev):
    from meepoembedding_amd.nn import DynamicEmbeddingCollection
    pairs, model, ids, w = _layer_case(dev, 16, 70)
    group = TieredTableGroup(pairs, max_apply_batch=256)
    offsets = T(np.arange(0, 4 * N_MEMBERS + 1, 4, dtype=np.int64), dev)
    layer = DynamicEmbeddingCollection(group, optimizer="adagrad", lr=LR, eps=EPS, min_count=2)
    _two_steps(dev, layer, pairs, model, ids, w, lambda m, k: m(T(k, dev), offsets))


def test_bag_layer_over_the_group(dev):
    from meepoembedding_amd.nn import DynamicEmbeddingBag
    pairs, model, ids, w = _layer_case(dev, 16, 72)
    group = TieredTableGroup(pairs, max_apply_batch=256)
    bag_offsets = T(np.arange(0, 4 * N_MEMBERS + 1, dtype=np.int64), dev)   # one id per bag, four bags per member
    layer = DynamicEmbeddingBag(group, mode="sum", optimizer="adagrad", lr=LR, eps=EPS, create_missing=True, min_count=2)
    _two_steps(dev, layer, pairs, model, ids, w, lambda m, k: m(T(k, dev), bag_offsets))


def test_bag_layer_over_one_pair_and_the_refusals(dev):
    from meepoembedding_amd.nn import DynamicEmbedding, DynamicEmbeddingBag, DynamicEmbeddingCollection
    pairs, model, ids, w = _layer_case(dev, 16, 74)
    pairs, model.oracles, model.sketch = pairs[:1], model.oracles[:1], model.sketch[:1]
    bag_offsets = T(np.arange(0, 5, dtype=np.int64), dev)
    layer = DynamicEmbeddingBag(pairs[0], mode="sum", optimizer="adagrad", lr=LR, eps=EPS, create_missing=True, min_count=2)
    _two_steps(dev, layer, pairs, model, ids[:4], w[:4], lambda m, k: m(T(k, dev), bag_offsets))
    with pytest.raises(ValueError, match="hot/cold") as ei:
        DynamicEmbedding(pairs[0], min_count=2)
    assert "TieredTableGroup([pair])" in str(ei.value)
    plain = TieredLookupTable(LookupTable(4096, 16, device=dev, optimizer=OPT_ADAGRAD), pairs[0].cold)
    with pytest.raises(ValueError, match="member 1"):
        DynamicEmbeddingCollection(TieredTableGroup([pairs[0], plain]), min_count=2)
    with pytest.raises(ValueError, match="hot table has no sketch"):
        DynamicEmbeddingBag(plain, create_missing=True, min_count=2)
    with pytest.raises(ValueError, match="create_missing"):
        DynamicEmbeddingBag(pairs[0], min_count=2)
    assert DynamicEmbeddingCollection(TieredTableGroup(pairs), min_count=2, out_dtype=torch.bfloat16).min_count == 2
