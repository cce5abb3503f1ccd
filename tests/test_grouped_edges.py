"""One hostile jagged batch through every operator that finds a position's member and creates (or moves) its key there: TableGroup.find_or_insert
(with and without min_count, fp32 and bf16 rows out), the collection of hot/cold pairs (unpooled find_or_insert, pooled lookup with insert_missing),
the mixed-width collection's insert_missing and the grouped move.  Each operator is, by definition, the single-table operator per member on its
segment; the reference is that call sequence on twin tables, compared bit for bit.  The operators have tests of their own with batches of their
own; here the SAME edges pin the segment staging, the segment search and the creation write on every path.

The batch: n = 85 positions, three members, offsets [3, 8, 8, 78] — three positions in front of the first segment, an empty middle member, seven
positions behind the last (where the operator cuts its offsets at n, also [3, 8, 8, 200]).  Row widths 4 (one lane of a tile writes) and 68 (the
16-lane loop takes a second trip for one lane only); 64 slots asked for per table."""
import numpy as np
import pytest
import torch

from meepoembedding_amd import (INIT_UNIFORM, OPT_ADAGRAD, OPT_ADAM, STATUS_RESERVED_KEY, STATUS_TABLE_FULL, LookupTable, MixedTableGroup, TableGroup,
                                TieredTableGroup, synth)
from meepoembedding_amd.table import hash_batch
from meepoembedding_amd.tiered import TieredLookupTable

pytestmark = pytest.mark.gpu

EMPTY_KEY = -(1 << 63)
RECLAIMED_KEY = EMPTY_KEY + 1
N, N_MEMBERS, SLOTS, B = 85, 3, 64, 2
OFFSETS, OFFSETS_PAST_N = [3, 8, 8, 78], [3, 8, 8, 200]
BAG_OFFSETS, BAG_OFFSETS_PAST_N = [3, 5, 8, 8, 8, 40, 78], [3, 5, 8, 8, 8, 40, 200]   # two bags per member: the members' bounds are every second entry
SENTINEL = -7.0
BF16 = torch.bfloat16
MIN_COUNT = 2    # a missing key asked for once in its segment stays out, one asked for twice or more is created


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _stored(dev, nb, full0):
    """the keys every member holds before the call.  Member 0 filled to its last slot: 16 keys per home bucket, so each sits in its own bucket
    whatever the order of the claims, and the twin holds the same set."""
    stored = [synth.keys_np(500 + j, 0, 24) for j in range(N_MEMBERS)]
    if full0:
        pool = synth.keys_np(600, 0, 64 * nb)
        home = hash_batch(T(pool, dev), nb, 1)[1].cpu().numpy()
        stored[0] = np.concatenate([pool[home == b][:16] for b in range(nb)])
        assert stored[0].size == 16 * nb
    return stored


def _batch(stored):
    """-> keys [N]"""
    new = synth.keys_np(700, 0, 40)
    shared, twice, thrice, cold4, pairs, outside = new[0], new[1], new[2], new[3:7], new[7:19], new[19:29]
    s0, s2 = stored[0], stored[2]
    k = np.empty(N, dtype=np.int64)
    k[0:3] = outside[0:3]                                       # in front of the first segment: never created
    k[3:8] = [s0[0], shared, new[30], new[30], s0[1]]            # member 0: stored, the key member 2 also asks for, a new key twice, stored
    k[8:12] = s2[0:4]                                           # member 2.  A wave step with nothing missing
    k[12:16] = [s2[4], s2[5], s2[6], RECLAIMED_KEY]             # a wave step whose only work is the tombstone's flag: no tile creates
    k[16:20] = cold4                                            # a wave step of four new keys asked for once each: under admission nobody is admitted
    k[20:24] = [shared, twice, s2[7], twice]
    k[24:28] = [thrice, thrice, s2[8], thrice]                  # one creator, three equal initial rows out
    k[28:30] = [EMPTY_KEY, RECLAIMED_KEY]                       # padding (silent) and a second tombstone, beside tiles that create
    rest = np.concatenate([pairs, pairs, s2[9:24], s2[0:9]])    # 12 new keys twice each among 24 stored ones
    k[30:78] = rest[np.random.default_rng(11).permutation(rest.size)]
    k[78:85] = outside[3:10]                                    # behind the last segment: created only where the offsets reach past them
    return k


def _table(dev, dim, j, opt, stored, tier=0, **kw):
    t = LookupTable(SLOTS, dim, device=dev, optimizer=opt, max_batch=256, default_value=0.5 + j + 4 * tier, initial_accumulator=0.1,
                    initializer=INIT_UNIFORM, init_scale=0.05, init_seed=10 * tier + j, **kw)
    if stored.size:
        t.insert(T(stored, dev), T(synth.rows_np(stored, dim, 3 + j), dev))
    assert t.size() == stored.size and t.status() == 0
    return t


def _members(dev, dims, opt, full0=False, **kw):
    """-> (tables, their twins, the batch)"""
    nb = LookupTable(SLOTS, 4, device=dev).n_buckets
    stored = _stored(dev, nb, full0)
    make = lambda: [_table(dev, dims[j], j, opt, stored[j], **kw) for j in range(N_MEMBERS)]  # noqa: E731
    a, b = make(), make()
    if full0:
        assert a[0].size() == a[0].capacity
    return a, b, _batch(stored)


def _segments(offsets):
    cut = [min(o, N) for o in offsets]
    return [(cut[j], max(cut[j], cut[j + 1])) for j in range(N_MEMBERS)]


def _sorted_export(t):
    planes = [x.cpu().numpy() for x in t.export(with_state=True) if x is not None]
    order = np.argsort(planes[0])
    return [p[order] for p in planes]


def _assert_same_tables(got, exp, what, status=True):
    for j, (a, b) in enumerate(zip(got, exp)):
        assert a.size() == b.size(), (what, j, a.size(), b.size())
        for x, y in zip(_sorted_export(a), _sorted_export(b)):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (what, j)
        assert not status or a.status() == b.status(), (what, j, a.status(), b.status())


def _assert_flags(tables, reserved, full, what):
    """RESERVED_KEY on the tables `reserved` names and on no other, TABLE_FULL likewise"""
    for j, t in enumerate(tables):
        assert bool(t.status() & STATUS_RESERVED_KEY) == (j in reserved), (what, "RESERVED_KEY", j, t.status())
        assert bool(t.status() & STATUS_TABLE_FULL) == (j in full), (what, "TABLE_FULL", j, t.status())


def _assert_rows(out, found, exp, segs, what):
    """inside the segments the twins' rows and found bytes, bit for bit; outside them the sentinel bytes the buffers were filled with"""
    inside = torch.zeros(N, dtype=torch.bool)
    for j, ((s, e), (eo, ef)) in enumerate(zip(segs, exp)):
        inside[s:e] = True
        assert torch.equal(out[s:e].view(torch.uint8), eo.to(out.dtype).view(torch.uint8)), (what, "rows", j)
        assert torch.equal(found[s:e], ef), (what, "found", j)
    assert bool((out[~inside.to(out.device)] == SENTINEL).all()) and bool((found[~inside.to(found.device)] == 7).all()), (what, "outside the segments")


def _no_hits(t, keys):
    return int(t.hits_of(keys).to(torch.int64).sum()) == 0


def _buffers(dev, dim, dtype):
    return torch.full((N, dim), SENTINEL, dtype=dtype, device=dev), torch.full((N,), 7, dtype=torch.uint8, device=dev)


# ---- TableGroup.find_or_insert --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,opt,min_count,dtype,full0", [
    (4, OPT_ADAGRAD, None, torch.float32, False), (68, OPT_ADAGRAD, None, torch.float32, False), (4, OPT_ADAGRAD, None, BF16, False),
    (68, OPT_ADAGRAD, None, BF16, False), (4, OPT_ADAGRAD, MIN_COUNT, torch.float32, False), (68, OPT_ADAGRAD, MIN_COUNT, torch.float32, False),
    (4, OPT_ADAGRAD, MIN_COUNT, BF16, False), (68, OPT_ADAGRAD, MIN_COUNT, BF16, False), (68, OPT_ADAM, None, torch.float32, False),
    (68, OPT_ADAM, MIN_COUNT, torch.float32, False), (68, OPT_ADAGRAD, None, torch.float32, True), (4, OPT_ADAGRAD, MIN_COUNT, BF16, True)])
def test_table_group_find_or_insert(dev, dim, opt, min_count, dtype, full0):
    a, b, keys = _members(dev, [dim] * N_MEMBERS, opt, full0, admission=True, track_hits=True)
    group = TableGroup(a)
    segs = _segments(OFFSETS)
    out, found = _buffers(dev, dim, dtype)
    kw = {} if min_count is None else {"min_count": min_count}
    group.find_or_insert(T(keys, dev), T(np.array(OFFSETS), dev), out=out, found=found, out_dtype=dtype, **kw)
    exp = [t.find_or_insert(T(keys[s:e], dev), **kw) for t, (s, e) in zip(b, segs)]    # (fp32: a bf16 copy is that row rounded once)
    what = f"dim {dim} min_count {min_count} {dtype}"
    _assert_rows(out, found, exp, segs, what)
    _assert_same_tables(a, b, what, status=min_count is None)   # (the single table's admission pass does not flag a tombstone in the batch)
    _assert_flags(a, reserved={2}, full={0} if full0 else set(), what=what)
    rows = out[24:28]
    assert torch.equal(rows[0], rows[1]) and torch.equal(rows[0], rows[3]) and not bool(found[24]) and bool(found[26]), "the key asked for three times"
    assert not torch.equal(out[4], out[20]) or full0, "the key of members 0 and 2: two tables, two initializers"
    created = [t.size() - s for t, s in zip(a, [a[0].capacity if full0 else 24, 24, 24])]
    assert created == [0 if full0 else (1 if min_count else 2), 0, 14 if min_count else 19], created    # nothing outside the segments was created
    for t, (s, e) in zip(a, segs):   # a created key starts its window with a zero hit counter
        new = T(keys[s:e], dev)[found[s:e] == 0]
        assert _no_hits(t, new)
    group.close()


# ---- the collection of hot/cold pairs ----------------------------------------------------------------------------------------------------------
def _pairs(dev, dim, opt, full0):
    """three pairs and their twins: member 0 creates hot, member 2 — whose stored keys are split over both tiers — creates cold (its hot tier is at
    its limit).  -> (pairs, twins, batch)"""
    nb = LookupTable(SLOTS, 4, device=dev).n_buckets
    stored = _stored(dev, nb, full0)
    none = np.empty(0, dtype=np.int64)

    def make():
        out = []
        for j in range(N_MEMBERS):
            in_hot = stored[j] if j == 0 else stored[j][::2]
            in_cold = none if j == 0 else stored[j][1::2]
            out.append(TieredLookupTable(_table(dev, dim, j, opt, in_hot), _table(dev, dim, j, opt, in_cold, tier=1), hot_key_limit=0 if j == 2 else 1 << 20))
        return out
    return make(), make(), _batch(stored)


def _tiers(pairs):
    return [p.hot for p in pairs] + [p.cold for p in pairs]   # index j: member j's hot table, N_MEMBERS + j: its cold table


@pytest.mark.parametrize("dim,opt,dtype,offsets,full0", [
    (4, OPT_ADAGRAD, torch.float32, OFFSETS, False), (68, OPT_ADAGRAD, BF16, OFFSETS, False), (68, OPT_ADAM, torch.float32, OFFSETS_PAST_N, False),
    (4, OPT_ADAGRAD, BF16, OFFSETS_PAST_N, False), (68, OPT_ADAGRAD, torch.float32, OFFSETS, True)])
def test_tiered_group_find_or_insert(dev, dim, opt, dtype, offsets, full0):
    a, b, keys = _pairs(dev, dim, opt, full0)
    group = TieredTableGroup(a)
    segs = _segments(offsets)
    out, found = _buffers(dev, dim, dtype)
    group.find_or_insert(T(keys, dev), T(np.array(offsets), dev), out=out, found=found, out_dtype=dtype)
    exp = [p.find_or_insert(T(keys[s:e], dev)) for p, (s, e) in zip(b, segs)]
    what = f"dim {dim} {dtype} offsets {offsets}"
    _assert_rows(out, found, exp, segs, what)
    _assert_same_tables(_tiers(a), _tiers(b), what)
    _assert_flags(_tiers(a), reserved={N_MEMBERS + 2}, full={0} if full0 else set(), what=what)   # member 2's COLD table, member 0's HOT table
    new_in_2 = 19 + (7 if offsets is OFFSETS_PAST_N else 0)
    assert [t.size() for t in _tiers(a)] == [a[0].hot.capacity if full0 else 26, 12, 12, 0, 12, 12 + new_in_2]
    group.close()


@pytest.mark.parametrize("dim,opt,bag_offsets,full0", [(4, OPT_ADAGRAD, BAG_OFFSETS, False), (68, OPT_ADAM, BAG_OFFSETS_PAST_N, False),
                                                     (68, OPT_ADAGRAD, BAG_OFFSETS, True)])
def test_tiered_group_pooled_insert_missing(dev, dim, opt, bag_offsets, full0):
    a, b, keys = _pairs(dev, dim, opt, full0)
    group = TieredTableGroup(a)
    segs = _segments(bag_offsets[::B])
    found = torch.full((N,), 7, dtype=torch.uint8, device=dev)
    pooled, _ = group.find_pooled(T(keys, dev), T(np.array(bag_offsets), dev), "sum", found=found, insert_missing=True)
    what = f"dim {dim} bag offsets {bag_offsets}"
    inside = torch.zeros(N, dtype=torch.bool, device=dev)
    for j, (p, (s, e)) in enumerate(zip(b, segs)):
        local = np.clip(np.array(bag_offsets[j * B:(j + 1) * B + 1]), 0, N) - s
        eo, ef = p.find_pooled(T(keys[s:e], dev), T(local, dev), "sum", insert_missing=True)
        inside[s:e] = True
        assert torch.equal(found[s:e], ef), (what, "found", j)
        assert torch.equal(pooled[j * B:(j + 1) * B].view(torch.uint8), eo.view(torch.uint8)), (what, "bags", j)
    assert bool((found[~inside] == 7).all()), (what, "found bytes outside the segments")
    _assert_same_tables(_tiers(a), _tiers(b), what, status=False)   # (the pair's own found pass is a locate of both tiers, which flags a tombstone on both)
    _assert_flags(_tiers(a), reserved={N_MEMBERS + 2}, full={0} if full0 else set(), what=what)
    new_in_2 = 19 + (7 if bag_offsets is BAG_OFFSETS_PAST_N else 0)
    assert [t.size() for t in _tiers(a)] == [a[0].hot.capacity if full0 else 26, 12, 12, 0, 12, 12 + new_in_2]
    group.close()


# ---- the mixed-width collection -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,opt,full0", [([4, 68, 64], OPT_ADAGRAD, False), ([4, 68, 64], OPT_ADAM, False), ([4, 68, 64], OPT_ADAGRAD, True),
                                            ([64, 4, 68], OPT_ADAM, False)])   # (the last: the non-empty members at 64 and 68)
def test_mixed_group_insert_missing(dev, dims, opt, full0):
    a, b, keys = _members(dev, dims, opt, full0, track_hits=True)
    group = MixedTableGroup(a)
    segs = _segments(BAG_OFFSETS[::B])
    found = torch.full((N,), 7, dtype=torch.uint8, device=dev)
    views, _ = group.find_pooled(T(keys, dev), T(np.array(BAG_OFFSETS), dev), "sum", found=found, insert_missing=True)
    inside = torch.zeros(N, dtype=torch.bool, device=dev)
    for j, (t, (s, e)) in enumerate(zip(b, segs)):
        _, ef = t.find_or_insert(T(keys[s:e], dev))
        eo, _ = t.find_pooled(T(keys[s:e], dev), T(np.array(BAG_OFFSETS[j * B:(j + 1) * B + 1]) - s, dev), "sum")
        inside[s:e] = True
        assert torch.equal(found[s:e], ef), ("found", j)
        assert torch.equal(views[j].view(torch.uint8), eo.view(torch.uint8)), ("bags", j)
        assert _no_hits(a[j], T(keys[s:e], dev)[ef == 0]), ("a created key's hit counter", j)
    assert not bool(found[~inside].any()), "outside the segments: this operator's found pass reports every position of the batch, those as absent"
    _assert_same_tables(a, b, "mixed")
    _assert_flags(a, reserved={2}, full={0} if full0 else set(), what="mixed")
    assert [t.size() for t in a] == [a[0].capacity if full0 else 26, 24, 43]
    group.close()


# ---- the grouped move -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,opt,offsets,full0", [(4, OPT_ADAGRAD, OFFSETS, False), (68, OPT_ADAM, OFFSETS_PAST_N, False), (68, OPT_ADAGRAD, OFFSETS, True)])
def test_group_move(dev, dim, opt, offsets, full0):
    """src holds the stored keys, and the keys behind the last segment in member 2 (they move only where the offsets reach them); the batch's new
    keys are in no table: nothing moves, nothing is created.  dst member 0 full: its keys stay in src."""
    nb = LookupTable(SLOTS, 4, device=dev).n_buckets
    stored = _stored(dev, nb, False)
    keys = _batch(stored)
    stored[2] = np.concatenate([stored[2], keys[78:85]])
    filler = _stored(dev, nb, True)[0] if full0 else np.empty(0, dtype=np.int64)
    none = np.empty(0, dtype=np.int64)

    def make():
        src = [_table(dev, dim, j, opt, stored[j], track_hits=True) for j in range(N_MEMBERS)]
        dst = [_table(dev, dim, j, opt, filler if j == 0 else none, tier=1, track_hits=True) for j in range(N_MEMBERS)]
        return src, dst
    (src, dst), (tsrc, tdst) = make(), make()
    gs, gd = TableGroup(src), TableGroup(dst)
    segs = _segments(offsets)
    n_moved, moved = gs.move_to(gd, T(keys, dev), T(np.array(offsets), dev), want_moved=True)
    for j, (s, e) in enumerate(segs):
        en, em = tsrc[j].move_to(tdst[j], T(keys[s:e], dev), want_moved=True)
        assert int(n_moved[j]) == int(en), ("distinct keys moved", j, int(n_moved[j]), int(en))
        assert torch.equal(moved[s:e], em), ("moved mask", j)
    what = f"move dim {dim} offsets {offsets}"
    _assert_same_tables(src + dst, tsrc + tdst, what)
    _assert_flags(src + dst, reserved={2}, full={N_MEMBERS} if full0 else set(), what=what)      # src member 2, dst member 0
    assert [int(x) for x in n_moved] == [0 if full0 else 2, 0, 24 + (7 if offsets is OFFSETS_PAST_N else 0)]
    for t in dst:
        assert _no_hits(t, T(keys, dev)), "a moved key starts a new window in dst"
    gs.close(); gd.close()


# ---- n = 1 and n = 0 --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 0])
def test_one_position_and_none(dev, n):
    dim, none = 68, np.empty(0, dtype=np.int64)
    key = synth.keys_np(900, 0, 1)[:n]
    off, bag_off = T(np.array([0, 0, 0, n]), dev), T(np.array([0, 0, 0, 0, 0, 0, n]), dev)

    def tables(dims=(dim,) * N_MEMBERS, tier=0, **kw):
        return [_table(dev, dims[j], j, OPT_ADAGRAD, none, tier=tier, **kw) for j in range(N_MEMBERS)]
    twin = tables()[2]
    eo, ef = twin.find_or_insert(T(key, dev))
    for dtype, kw in ((torch.float32, {}), (BF16, {}), (torch.float32, {"min_count": 1})):
        a = tables(admission=True)
        out, found = TableGroup(a).find_or_insert(T(key, dev), off, out_dtype=dtype, **kw)
        assert torch.equal(out, eo.to(dtype)) and torch.equal(found, ef) and [t.size() for t in a] == [0, 0, n]
        _assert_same_tables(a[2:], [twin], "TableGroup")
    hot, cold = tables(), tables(tier=1)
    pairs = [TieredLookupTable(h, c, hot_key_limit=1 << 20) for h, c in zip(hot, cold)]
    out, found = TieredTableGroup(pairs).find_or_insert(T(key, dev), off)
    assert torch.equal(out, eo) and torch.equal(found, ef) and [t.size() for t in hot + cold] == [0, 0, n, 0, 0, 0]
    _assert_same_tables(hot[2:], [twin], "TieredTableGroup.find_or_insert")
    hot, cold = tables(), tables(tier=1)
    pairs = [TieredLookupTable(h, c, hot_key_limit=1 << 20) for h, c in zip(hot, cold)]
    pooled, found = TieredTableGroup(pairs).find_pooled(T(key, dev), bag_off, "sum", insert_missing=True)
    assert torch.equal(found, ef) and [t.size() for t in hot + cold] == [0, 0, n, 0, 0, 0]
    assert torch.equal(pooled[5], eo[0] if n else torch.zeros(dim, device=dev)) and not bool(pooled[:5].any())
    _assert_same_tables(hot[2:], [twin], "TieredTableGroup.find_pooled")
    a = tables(dims=(4, 64, dim))
    views, found = MixedTableGroup(a).find_pooled(T(key, dev), bag_off, "sum", insert_missing=True)
    assert torch.equal(found, ef) and [t.size() for t in a] == [0, 0, n]
    assert torch.equal(views[2][1], eo[0] if n else torch.zeros(dim, device=dev))
    _assert_same_tables(a[2:], [twin], "MixedTableGroup")
    src, dst = tables(), tables(tier=1)
    rows = T(synth.rows_np(key, dim, 5), dev)
    if n:
        src[2].insert(T(key, dev), rows)
    n_moved, moved = TableGroup(src).move_to(TableGroup(dst), T(key, dev), off, want_moved=True)
    assert [int(x) for x in n_moved] == [0, 0, n] and bool(moved.all()) and [t.size() for t in src + dst] == [0, 0, 0, 0, 0, n]
    if n:
        assert torch.equal(dst[2].find(T(key, dev))[0], rows)
