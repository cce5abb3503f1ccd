"""Embedding bags over a COLLECTION of hot/cold pairs (TieredTableGroup, mee_group_find_pooled_tiered, mee_group_ensure_tiered): by definition
(SPEC.md §3 "Tiering") the group's pooled lookup is TieredLookupTable.find_pooled of member b // bags_per_table on its bags, its step the pair's
step per member, and creation goes per member into the tier its pair would pick.  CPU: the host logic over oracle-backed tiers.  GPU: three pairs
(hot in HBM, cold rows in pinned host memory) of different sizes, bags_per_table = 5 — no multiple of 4, so one wave serves two members."""
import numpy as np
import pytest
import torch

import oracle
from _apply_cases import assert_bits_equal_nan_aware, exact_grads_np
from _cpu_backend import CpuTable
from meepoembedding_amd import synth

EMPTY_KEY = -(1 << 63)
RECLAIMED_KEY = EMPTY_KEY + 1
ABSENT_KEY = 123456789          # in no table of this file
N_KEYS = 400                    # the distinct keys the batches draw from (every non-empty member stores all of them, with rows of its own)
N_MEMBERS, BPT = 3, 5
# requested slots per member (hot, cold): all different, so that a descriptor taken from the wrong member or the wrong tier shows
CAPS = [(1000, 5000), (6000, 2000), (20000, 3000)]
EMPTY_MEMBER = 2                # holds no key in either tier
HOT_DEFAULT = [0.5, 0.75, 1.5]
COLD_DEFAULT = [0.25, 0.125, 2.0]   # a cold table's default row must never show
INIT = dict(initial_accumulator=0.1, initializer=oracle.INIT_UNIFORM, init_scale=0.05)

# batch A: 8.6 keys per bag on average, the tile-per-bag instance, with long bags (>= 16 keys: the four tiles together) inside it
LENS_A = [0, 1, 2, 15, 16, 17, 40, 3, 0, 5, 16, 1, 7, 4, 2]
# batch B: every bag >= 12 keys: the wave-per-bag instance
LENS_B = [12, 13, 16, 17, 33, 40, 12, 12, 20, 16, 13, 12, 17, 12, 14]


def _offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def _np(x):
    return None if x is None else x.cpu().numpy()


def _sorted(exp):
    exp = [_np(x) if isinstance(x, torch.Tensor) else x for x in exp]
    order = np.argsort(exp[0])
    return [None if x is None else x[order] for x in exp]


def _universe():
    return synth.keys_np(71, 0, N_KEYS)


def _batches():
    """-> {name: (keys, offsets)}: distinct stored keys, then a key repeated two positions on, an absent key and the two reserved keys, planted in
    one short bag (member 0) and one long bag (member 1) of each batch"""
    universe = _universe()
    out, at = {}, 0
    for name, lens in (("A", LENS_A), ("B", LENS_B)):
        off = _offsets(lens)
        keys = universe[at:at + off[-1]].copy()
        at += int(off[-1])
        long_bag = int(np.argmax(lens))
        p = int(off[long_bag])
        keys[p + 6] = keys[p + 4]
        keys[p + 9], keys[p + 20], keys[p + 31] = ABSENT_KEY, EMPTY_KEY, RECLAIMED_KEY
        short_bag = lens.index(15) if 15 in lens else 1
        q = int(off[short_bag])
        keys[q + 3], keys[q + 8], keys[q + 11] = RECLAIMED_KEY, ABSENT_KEY, EMPTY_KEY
        keys[q + 6] = keys[q + 4]
        out[name] = (keys, off)
    assert at <= N_KEYS
    return out


def _hot_masks(batches):
    """the four placements of the N_KEYS keys: name -> bool[N_KEYS], True = the key sits in the hot tier"""
    universe = _universe()
    half = np.random.default_rng(7).random(N_KEYS) < 0.5
    alt = half.copy()
    index_of = {int(k): i for i, k in enumerate(universe)}
    for keys, off in batches.values():       # alternating hot / cold by position inside every bag
        for b in range(off.size - 1):
            for j, k in enumerate(keys[off[b]:off[b + 1]]):
                if int(k) in index_of:
                    alt[index_of[int(k)]] = (j % 2 == 0)
    return {"all_hot": np.ones(N_KEYS, bool), "all_cold": np.zeros(N_KEYS, bool), "half": half, "alternating": alt}


def _member(keys, off, j):
    """member j's slice of a batch: (its keys, its BPT + 1 offsets rebased to the slice)"""
    s, e = int(off[j * BPT]), int(off[(j + 1) * BPT])
    return keys[s:e], off[j * BPT:(j + 1) * BPT + 1] - s, s, e


class _CpuTable(CpuTable):
    """tests/_cpu_backend.CpuTable whose apply_* take grad_index, as the LookupTable's do (position i takes row grad_index[i] of grads)"""

    def apply_adagrad(self, keys, grads, lr, eps=1e-10, grad_index=None):
        super().apply_adagrad(keys, grads if grad_index is None else grads[grad_index], lr, eps)

    def apply_adam(self, keys, grads, lr, beta1=0.9, beta2=0.999, eps=1e-8, step=1, grad_index=None):
        super().apply_adam(keys, grads if grad_index is None else grads[grad_index], lr, beta1, beta2, eps, step)


# ---- CPU: the host logic -----------------------------------------------------------------------------------------------------
def test_constructor_refusals_need_no_device(built):
    from meepoembedding_amd import TieredTableGroup
    from meepoembedding_amd.tiered import TieredLookupTable
    pair = lambda dim, **kw: TieredLookupTable(_CpuTable(256, dim, **kw), _CpuTable(256, dim, **kw))  # noqa: E731
    with pytest.raises(ValueError, match="at least one"):
        TieredTableGroup([])
    with pytest.raises(ValueError, match="one dim"):
        TieredTableGroup([pair(8), pair(16)])
    with pytest.raises(ValueError, match="policy"):
        TieredTableGroup([pair(8, track_hits=True), pair(8), pair(8, track_hits=True)])
    g = TieredTableGroup([pair(8), pair(8)])
    assert g.pools_with_insert is True and g.weighted_bags is False and g.supports_pooled_out_dtype is True and not g.policy
    assert g.dim == 8 and len(g.tables) == 2 and g.device == torch.device("cpu") and g.size() == 0
    assert TieredTableGroup([pair(8, track_hits=True), pair(8, track_hits=True)]).policy
    with pytest.raises(ValueError):
        g.find_pooled(torch.arange(4), torch.tensor([0, 2, 4]), "max")
    g.close()


@pytest.mark.parametrize("opt", [oracle.OPT_ADAGRAD, oracle.OPT_ADAM])
def test_tiered_group_cpu_logic(built, opt):
    from meepoembedding_amd import TieredTableGroup
    from meepoembedding_amd.nn import DynamicEmbeddingBag
    from meepoembedding_amd.tiered import TieredLookupTable
    dim = 16
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    universe = _universe()
    pairs, refs = [], []
    for j in range(N_MEMBERS):
        kw = dict(optimizer=opt, init_seed=9 + j, **INIT)
        hot = _CpuTable(1024, dim, default_value=HOT_DEFAULT[j], **kw)
        cold = _CpuTable(2048, dim, default_value=COLD_DEFAULT[j], **kw)
        # member 0 keeps room in its hot tier, member 1's is at its limit after the first 200 keys, member 2 starts empty with room
        pair = TieredLookupTable(hot, cold, hot_key_limit=[900, 200, 900][j])
        ref = oracle.OracleTable(8192, dim, default_value=HOT_DEFAULT[j], **kw)
        if j != EMPTY_MEMBER:
            rows = synth.rows_np(universe, dim, 3 + j)       # the same keys in every member, rows of its own
            for s in (slice(0, 200), slice(200, N_KEYS)):
                pair.insert(T(universe[s]), T(rows[s])); ref.insert(universe[s], rows[s])
        pairs.append(pair); refs.append(ref)
    assert [p.hot.size() for p in pairs] == [N_KEYS, 200, 0] and [p.cold.size() for p in pairs] == [0, 200, 0]
    group = TieredTableGroup(pairs)

    for keys, off in _batches().values():
        rows = np.concatenate([refs[j].find(_member(keys, off, j)[0])[0] for j in range(N_MEMBERS)])
        ef = np.concatenate([refs[j].find(_member(keys, off, j)[0])[1] for j in range(N_MEMBERS)])
        for mode in ("sum", "mean"):
            out, found = group.find_pooled(T(keys), T(off), mode)
            assert out.dtype == torch.float32 and np.array_equal(out.numpy(), oracle.pool_rows(rows, off, mode)), mode
            assert np.array_equal(found.numpy(), ef)
            for j in range(N_MEMBERS):
                mk, mo, s, e = _member(keys, off, j)
                po, pf = pairs[j].find_pooled(T(mk), T(mo), mode)
                assert torch.equal(out[j * BPT:(j + 1) * BPT], po) and torch.equal(found[s:e], pf)
        o16, _ = group.find_pooled(T(keys), T(off), "sum", out_dtype=torch.bfloat16)
        assert o16.dtype == torch.bfloat16 and torch.equal(o16, torch.from_numpy(oracle.pool_rows(rows, off, "sum")).to(torch.bfloat16))

    # insert_missing: new keys, each twice in its member's segment (inside a bag and across bags); member 0 has room (hot), member 1 has none (cold)
    new = synth.keys_np(72, 0, 12)
    seg = np.concatenate([universe[:20], new, universe[300:310], new])          # 54 keys per member
    keys = np.concatenate([seg, seg, seg])
    off = _offsets([7, 0, 30, 13, 4] * N_MEMBERS)
    er, ef = zip(*[refs[j].find_or_insert(seg) for j in range(N_MEMBERS)])
    out, found = group.find_pooled(T(keys), T(off), "mean", insert_missing=True)
    assert np.array_equal(found.numpy(), np.concatenate(ef)) and np.array_equal(out.numpy(), oracle.pool_rows(np.concatenate(er), off, "mean"))
    f = found.numpy().reshape(N_MEMBERS, -1)
    assert not f[:, 20:32].any() and not f[:, 42:].any()            # 0 for every occurrence of a new key, the repeated one included
    assert f[0, :20].all() and f[1, 32:42].all() and not f[EMPTY_MEMBER].any()
    in_hot = [p.hot.find(T(new))[1].numpy() for p in pairs]
    in_cold = [p.cold.find(T(new))[1].numpy() for p in pairs]
    assert in_hot[0].all() and not in_cold[0].any(), "member 0 has room: hot"
    assert in_cold[1].all() and not in_hot[1].any(), "member 1 has none: cold"
    assert in_hot[2].all() and not in_cold[2].any()
    assert [p.size() for p in pairs] == [r.size() for r in refs] == [N_KEYS + 12, N_KEYS + 12, 42]   # (the empty member creates all 42 distinct keys of its segment)

    # the step: duplicates inside and across bags; the union of every pair ends as the oracle's table of that member
    rng = np.random.default_rng(5)
    keys, off = _batches()["A"]
    keys = keys.copy()
    keys[off[10]:off[10] + 8] = keys[off[3]:off[3] + 8]               # member 2's bag repeats keys of member 0's: different tables, not duplicates
    keys[off[6] + 12:off[6] + 16] = keys[off[5]:off[5] + 4]           # member 1: a key in two bags
    bag_of = np.repeat(np.arange(off.size - 1), np.diff(off))
    bag_grads = exact_grads_np(rng, off.size - 1, dim, positions=keys.size)
    if opt == oracle.OPT_ADAGRAD:
        group.apply_pooled(T(keys), T(off), T(bag_grads), T(bag_of), "adagrad", lr=0.02)
    else:
        group.apply_pooled(T(keys), T(off), T(bag_grads), T(bag_of), "adam", lr=0.002, step=1)
    for j in range(N_MEMBERS):
        mk, _, s, e = _member(keys, off, j)
        if opt == oracle.OPT_ADAGRAD:
            refs[j].apply_adagrad(mk, bag_grads[bag_of[s:e]], 0.02, 1e-10)
        else:
            refs[j].apply_adam(mk, bag_grads[bag_of[s:e]], 0.002, 0.9, 0.999, 1e-8, 1)
        got, exp = _sorted(pairs[j].export(with_state=True)), _sorted(refs[j].export(with_state=True))
        for a, b in zip(got, exp):
            assert (a is None and b is None) or np.array_equal(a, b), j
    assert group.size() == sum(r.size() for r in refs) and len(group.layout_epoch) == 2 * N_MEMBERS

    # the bag layer: the pools_with_insert path, per_sample_weights refused by name
    layer = DynamicEmbeddingBag(group, mode="sum", optimizer="adagrad" if opt == oracle.OPT_ADAGRAD else "adam", create_missing=True).train()
    keys, off = _batches()["B"]
    out = layer(T(keys), T(off))
    out.sum().backward()
    assert out.shape == (N_MEMBERS * BPT, dim)
    with pytest.raises(ValueError, match="TieredTableGroup"):
        layer(T(keys), T(off), per_sample_weights=torch.ones(keys.size))
    with pytest.raises(RuntimeError):
        group.rebalance()      # pairs without the policy: each pair's own refusal


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
_SETUPS = {}


def _T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _fill(table, stored, n_live, stream, dim, seed, dev, tombstones=0):
    """`stored` (keys the lookups may ask for) plus filler keys up to n_live live keys; `tombstones` more keys are inserted and removed again, so
    that RECLAIMED slots lie on the probe paths of the keys that stay"""
    filler = synth.keys_np(stream, 0, n_live - stored.size + tombstones)
    keys = np.concatenate([stored, filler])
    table.insert(_T(keys, dev), _T(synth.rows_np(keys, dim, seed), dev))
    if tombstones:
        table.remove(_T(filler[-tombstones:], dev))
    return keys[:n_live]


def _make_pairs(dim, dev, hot_mask, **kw):
    """three pairs of CAPS' sizes: members 0 and 1 hold the universe split by hot_mask (member 1 by its complement where the mask is mixed), each tier
    topped up to a load of 0.86 with filler keys, member 0 with tombstones on its probe paths; EMPTY_MEMBER holds nothing.  -> (pairs, union keys per member)"""
    from meepoembedding_amd import LookupTable, _lib
    from meepoembedding_amd.tiered import TieredLookupTable
    universe = _universe()
    pairs, unions = [], []
    for j, (hc, cc) in enumerate(CAPS):
        hot = LookupTable(hc, dim, device=dev, max_batch=8192, default_value=HOT_DEFAULT[j], **kw)
        cold = LookupTable(cc, dim, device=dev, max_batch=8192, default_value=COLD_DEFAULT[j], value_memory=_lib.MEM_HOST_PINNED, **kw)
        union = np.zeros(0, np.int64)
        if j != EMPTY_MEMBER:
            mask = ~hot_mask if (j == 1 and hot_mask.any() and not hot_mask.all()) else hot_mask
            nh, nc = int(np.ceil(0.86 * hot.capacity)), int(np.ceil(0.86 * cold.capacity))
            hk = _fill(hot, universe[mask], nh, 80 + 2 * j, dim, 3 + j, dev, tombstones=40 if j == 0 else 0)
            ck = _fill(cold, universe[~mask], nc, 81 + 2 * j, dim, 3 + j, dev, tombstones=200 if j == 0 else 0)
            assert hot.size() == nh >= 0.85 * hot.capacity and cold.size() == nc >= 0.85 * cold.capacity
            union = np.concatenate([hk, ck])
        pairs.append(TieredLookupTable(hot, cold))
        unions.append(union)
    return pairs, unions


def _setup(dim, dev):
    """per dim, built once and only read afterwards: per placement the three pairs and their TieredTableGroup; an untiered TableGroup of three tables
    holding each member's union; per batch the keys, the offsets and the oracle's rows and found mask"""
    if dim in _SETUPS:
        return _SETUPS[dim]
    from meepoembedding_amd import LookupTable, TableGroup, TieredTableGroup
    batches = _batches()
    groups = {}
    all_keys = [np.zeros(0, np.int64)] * N_MEMBERS
    for name, mask in _hot_masks(batches).items():
        pairs, unions = _make_pairs(dim, dev, mask)
        groups[name] = (TieredTableGroup(pairs), pairs)
        all_keys = [np.union1d(a, u) for a, u in zip(all_keys, unions)]   # (a placement's filler keys are never asked for: any superset serves)
    refs, flat = [], []
    for j in range(N_MEMBERS):
        ref = oracle.OracleTable(32768, dim, default_value=HOT_DEFAULT[j])
        one = LookupTable(32768, dim, device=dev, max_batch=1 << 14, default_value=HOT_DEFAULT[j])
        if all_keys[j].size:
            rows = synth.rows_np(all_keys[j], dim, 3 + j)
            ref.insert(all_keys[j], rows)
            one.insert(_T(all_keys[j], dev), _T(rows, dev))
        refs.append(ref); flat.append(one)
    exp = {}
    for name, (keys, off) in batches.items():
        got = [refs[j].find(_member(keys, off, j)[0]) for j in range(N_MEMBERS)]
        exp[name] = (_T(keys, dev), _T(off, dev), np.concatenate([g[0] for g in got]), np.concatenate([g[1] for g in got]), keys, off)
    _SETUPS[dim] = (groups, TableGroup(flat), exp)
    return _SETUPS[dim]


def _guarded(shape, dtype, dev, fill):
    """a buffer with one guard row (or 64 guard bytes) behind it -> (the view to hand in, the guard)"""
    rows = shape[0] + (1 if len(shape) == 2 else 64)
    buf = torch.full((rows, *shape[1:]), fill, dtype=dtype, device=dev)
    return buf[:shape[0]], buf[shape[0]:]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["sum", "mean"])
@pytest.mark.parametrize("dim", [16, 64, 128, 100, 260])
def test_group_lookup_is_the_pairs_lookup_bit_for_bit(dev, dim, mode):
    groups, flat, exp = _setup(dim, dev)
    for bname, (keys, off, rows, ef, hkeys, hoff) in exp.items():
        want = oracle.pool_rows(rows, hoff, mode)
        fo, ff = flat.find_pooled(keys, off, mode)
        assert_bits_equal_nan_aware(_np(fo), want, f"untiered group {bname}")
        assert np.array_equal(_np(ff), ef)
        for pname, (group, pairs) in groups.items():
            out, og = _guarded((N_MEMBERS * BPT, dim), torch.float32, dev, -7.0)
            found, fg = _guarded((keys.numel(),), torch.uint8, dev, 7)
            group.find_pooled(keys, off, mode, out=out, found=found)
            assert_bits_equal_nan_aware(_np(out), want, f"{pname} {bname} against the oracle")
            assert_bits_equal_nan_aware(_np(out), _np(fo), f"{pname} {bname} against the untiered group")
            assert np.array_equal(_np(found), ef) and np.array_equal(_np(found), _np(ff)), (pname, bname)
            assert bool((og == -7.0).all()) and bool((fg == 7).all()), "bytes behind out / found were written"
            for j, pair in enumerate(pairs):
                mk, mo, s, e = _member(hkeys, hoff, j)
                po, pf = pair.find_pooled(_T(mk, dev), _T(mo, dev), mode)
                assert_bits_equal_nan_aware(_np(out[j * BPT:(j + 1) * BPT]), _np(po), f"{pname} {bname} member {j} against its pair")
                assert torch.equal(found[s:e], pf)
    keys, off = exp["A"][0], exp["A"][1]
    n = keys.numel()
    # offsets are the caller's: bags past the key array are cut at its end, a decreasing pair is an empty bag.  Per member (5 bags each):
    # [0,10) [10,5)=empty [5,40) [40,40) [40,60) | [60,60) [60,100) [100,90)=empty [90,120) [120,125) | [125,n) and four empty ones
    bad = torch.tensor([0, 10, 5, 40, 40, 60, 60, 100, 90, 120, 125, n + 3, 1 << 40, 1 << 41, 5, 3], dtype=torch.int64, device=dev)
    for pname, (group, pairs) in groups.items():
        out, _ = group.find_pooled(keys, off[:1], mode)           # zero bags: nothing is written
        assert out.shape == (0, dim)
        out, found = group.find_pooled(keys[:0], torch.zeros(N_MEMBERS * BPT + 1, dtype=torch.int64, device=dev), mode)    # bags over no keys
        assert out.shape == (N_MEMBERS * BPT, dim) and not out.any() and found.numel() == 0
        out, _ = group.find_pooled(keys, torch.full((N_MEMBERS * BPT + 1,), 5, dtype=torch.int64, device=dev), mode)
        assert not out.any()
        out, og = _guarded((N_MEMBERS * BPT, dim), torch.float32, dev, -7.0)
        found, fg = _guarded((n,), torch.uint8, dev, 7)
        group.find_pooled(keys, bad, mode, out=out, found=found)
        want_found = torch.full((n,), 7, dtype=torch.uint8, device=dev)
        for j, pair in enumerate(pairs):       # the per-pair lookup over the same key array with the member's six offsets as they are
            po, pf = pair.find_pooled(keys, bad[j * BPT:(j + 1) * BPT + 1].contiguous(), mode, found=torch.full((n,), 7, dtype=torch.uint8, device=dev))
            assert_bits_equal_nan_aware(_np(out[j * BPT:(j + 1) * BPT]), _np(po), f"{pname} clamped offsets, member {j}")
            want_found = torch.where(pf != 7, pf, want_found)
        assert torch.equal(found, want_found) and bool((og == -7.0).all()) and bool((fg == 7).all()), pname


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [64, 100])
def test_group_lookup_bf16_rounds_the_finished_row_once(dev, dim):
    groups, _, exp = _setup(dim, dev)
    for pname in ("alternating", "all_cold", "half"):
        group = groups[pname][0]
        for keys, off, _, ef, _, _ in exp.values():
            for mode in ("sum", "mean"):
                o32, _ = group.find_pooled(keys, off, mode)
                out, og = _guarded((N_MEMBERS * BPT, dim), torch.bfloat16, dev, -7.0)
                _, found = group.find_pooled(keys, off, mode, out=out, out_dtype=torch.bfloat16)
                assert torch.equal(out.view(torch.int16), o32.to(torch.bfloat16).view(torch.int16)), (pname, mode)
                assert np.array_equal(_np(found), ef) and bool((og == -7.0).all())


def _policy_pairs(dev, dim=16):
    """three small pairs with hit counters, every member holding the universe (rows of its own), keys of even index hot and of odd index cold"""
    from meepoembedding_amd import LookupTable, _lib
    from meepoembedding_amd.tiered import TieredLookupTable
    universe = _universe()
    pairs = []
    for j, (hc, cc) in enumerate([(1000, 3000), (2000, 1000), (3000, 2000)]):
        hot = LookupTable(hc, dim, device=dev, max_batch=4096, track_hits=True, default_value=HOT_DEFAULT[j])
        cold = LookupTable(cc, dim, device=dev, max_batch=4096, track_hits=True, value_memory=_lib.MEM_HOST_PINNED, default_value=COLD_DEFAULT[j])
        hot.insert(_T(universe[0::2], dev), _T(synth.rows_np(universe[0::2], dim, 3 + j), dev))
        cold.insert(_T(universe[1::2], dev), _T(synth.rows_np(universe[1::2], dim, 3 + j), dev))
        pairs.append(TieredLookupTable(hot, cold, hot_key_limit=3000, sample_every=4))
    return pairs


def _hit_sets(pairs):
    """per pair and tier, the keys with at least 1, 2, 3 and 4 hits"""
    return [[np.sort(_np(t.hits_scan(k, 0xFFFFFFFF, 4096))) for k in (1, 2, 3, 4)] for p in pairs for t in (p.hot, p.cold)]


@pytest.mark.gpu
@pytest.mark.parametrize("bname", ["A", "B"])
def test_group_lookup_counts_hits_like_the_pairs(dev, bname):
    """the launch with neither, one and both count flags leaves, in every member, the counters that per-pair launches with the same flags leave;
    a member none of whose bags holds a key keeps zeros"""
    from meepoembedding_amd import TieredTableGroup, _lib
    L = _lib.lib()
    keys, off = _batches()[bname]
    keys, off = keys.copy(), off.copy()
    off[2 * BPT + 1:] = off[2 * BPT]                  # member 2's bags are all empty: nothing of it is touched
    keys[off[6] + 1] = keys[off[6] + 3] = keys[off[6]]     # a key three times in one bag: counted three times
    a, b = _policy_pairs(dev), _policy_pairs(dev)
    group = TieredTableGroup(a)
    assert group.policy
    dk, do = _T(keys, dev), _T(off, dev)
    out = torch.empty(N_MEMBERS * BPT, 16, device=dev)
    ref = torch.empty(N_MEMBERS * BPT, 16, device=dev)
    for flags in (0, _lib.TIER_COUNT_COLD, _lib.TIER_COUNT_HOT, _lib.TIER_COUNT_COLD | _lib.TIER_COUNT_HOT, _lib.TIER_COUNT_COLD):
        _lib.check(L.mee_group_find_pooled_tiered(group.hot_group._h, group.cold_group._h, dk.data_ptr(), keys.size, do.data_ptr(), BPT, out.data_ptr(),
                                                  _lib.DTYPE_F32, None, 0, flags, None))
        for j, pair in enumerate(b):
            mk, mo, _, _ = _member(keys, off, j)
            mk, mo = _T(mk, dev), _T(mo, dev)
            _lib.check(L.mee_find_pooled_tiered(pair.hot._h, pair.cold._h, mk.data_ptr(), mk.numel(), mo.data_ptr(), BPT, ref[j * BPT:].data_ptr(),
                                                _lib.DTYPE_F32, None, 0, flags, None))
        torch.cuda.synchronize(dev)
        assert torch.equal(out, ref)
        got, want = _hit_sets(a), _hit_sets(b)
        for g, w in zip(got, want):
            for x, y in zip(g, w):
                assert np.array_equal(x, y), flags
        if flags == 0:
            assert all(x.size == 0 for g in got for x in g), "no flag, no count"
    got = _hit_sets(a)
    assert got[0][0].size and got[1][0].size and got[2][0].size and got[3][0].size, "both tiers of members 0 and 1 were counted"
    assert int(keys[off[6]]) in got[2][2].tolist() + got[3][2].tolist(), "three occurrences, at least three hits"
    assert all(x.size == 0 for x in got[4] + got[5]), "member 2 was not touched"
    # the Python method: cold hits on every call, hot hits on every sample_every-th, as the pair does
    fresh = _policy_pairs(dev)
    g2 = TieredTableGroup(fresh, sample_every=4)
    for _ in range(8):
        g2.find_pooled(dk, do)
    hot_twice, cold_8 = np.sort(_np(fresh[0].hot.hits_scan(2, 0xFFFFFFFF, 4096))), np.sort(_np(fresh[0].cold.hits_scan(8, 0xFFFFFFFF, 4096)))
    mk = _member(keys, off, 0)[0]
    universe = _universe()
    assert np.array_equal(hot_twice, np.sort(np.intersect1d(mk, universe[0::2]))) and np.array_equal(cold_8, np.sort(np.intersect1d(mk, universe[1::2])))


def _train_pairs(dev, dim, opt):
    """three pairs for insert_missing and training: member 0 has room in its hot tier, member 1's hot tier is at its limit (new keys go cold), member 2
    starts empty with room.  The universe's first half is hot, the second cold."""
    from meepoembedding_amd import LookupTable, _lib
    from meepoembedding_amd.tiered import TieredLookupTable
    universe = _universe()
    pairs = []
    for j, (hc, cc) in enumerate([(1000, 3000), (2000, 1000), (3000, 2000)]):
        kw = dict(device=dev, optimizer=opt, max_batch=4096, init_seed=9 + j, **INIT)
        hot = LookupTable(hc, dim, default_value=HOT_DEFAULT[j], **kw)
        cold = LookupTable(cc, dim, default_value=COLD_DEFAULT[j], value_memory=_lib.MEM_HOST_PINNED, **kw)
        if j != EMPTY_MEMBER:
            hot.insert(_T(universe[:200], dev), _T(synth.rows_np(universe[:200], dim, 3 + j), dev))
            cold.insert(_T(universe[200:], dev), _T(synth.rows_np(universe[200:], dim, 3 + j), dev))
        pair = TieredLookupTable(hot, cold, hot_key_limit=200 if j == 1 else 10 * hot.capacity)
        pair._hot_keys_ub = hot.size()      # (the tiers were filled directly: the pair's bound on its hot keys starts at what is there)
        pairs.append(pair)
    return pairs


def _assert_same_tiers(a, b, what):
    """every tier of every pair: the key-sorted export with the state planes, bit for bit"""
    for j, (pa, pb) in enumerate(zip(a, b)):
        for tier in ("hot", "cold"):
            ta, tb = getattr(pa, tier), getattr(pb, tier)
            got, exp = _sorted(ta.export(with_state=True)), _sorted(tb.export(with_state=True))
            assert np.array_equal(got[0], exp[0]), (what, j, tier, got[0].size, exp[0].size)
            for x, y in zip(got[1:], exp[1:]):
                assert (x is None and y is None) or np.array_equal(x.view(np.uint32), y.view(np.uint32)), (what, j, tier)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["sum", "mean"])
def test_group_insert_missing_creates_like_the_pairs(dev, mode):
    from meepoembedding_amd import OPT_ADAM, STATUS_RESERVED_KEY, TieredTableGroup
    dim = 64
    a, b = _train_pairs(dev, dim, OPT_ADAM), _train_pairs(dev, dim, OPT_ADAM)
    group = TieredTableGroup(a, max_apply_batch=4096)
    universe = _universe()
    new = synth.keys_np(72, 0, 20)
    seg = np.concatenate([universe[150:190], new, [RECLAIMED_KEY, EMPTY_KEY], universe[220:250], new])     # 112 keys per member
    keys = np.concatenate([seg, seg, seg])
    off = _offsets([17, 0, 50, 5, 40] * N_MEMBERS)
    out, og = _guarded((N_MEMBERS * BPT, dim), torch.float32, dev, -7.0)
    found, fg = _guarded((keys.size,), torch.uint8, dev, 7)
    group.find_pooled(_T(keys, dev), _T(off, dev), mode, out=out, found=found, insert_missing=True)
    for j, pair in enumerate(b):
        mk, mo, s, e = _member(keys, off, j)
        po, pf = pair.find_pooled(_T(mk, dev), _T(mo, dev), mode, insert_missing=True)
        assert torch.equal(out[j * BPT:(j + 1) * BPT], po), j       # the pooled rows include the created rows
        assert torch.equal(found[s:e], pf), j                       # "present before the call"
    assert bool((og == -7.0).all()) and bool((fg == 7).all())
    f = _np(found).reshape(N_MEMBERS, -1)
    assert not f[:, 40:62].any() and not f[:, 92:].any() and f[0, :40].all() and f[1, 62:92].all() and not f[EMPTY_MEMBER].any()
    dn = _T(new, dev)
    for j, (want_hot, pair) in enumerate(zip((True, False, True), a)):     # exactly one tier, the one the rule picks
        in_hot, in_cold = pair.hot.find(dn)[1], pair.cold.find(dn)[1]
        assert bool(in_hot.all() and not in_cold.any()) if want_hot else bool(in_cold.all() and not in_hot.any()), j
    _assert_same_tiers(a, b, "insert_missing")      # hashed initial rows, initial optimizer state, nothing else touched
    # the tombstone value in the batch is flagged on the status word of the table that was asked to create, as mee_find_or_insert_missing flags it
    # (the pairs of the reference carry the bit in both tiers: their found pass is mee_locate on each tier, which flags it too)
    assert [(p.hot.status(), p.cold.status()) for p in a] == [(STATUS_RESERVED_KEY, 0), (0, STATUS_RESERVED_KEY), (STATUS_RESERVED_KEY, 0)]
    # a second call creates nothing and finds everything but the reserved keys
    _, found = group.find_pooled(_T(keys, dev), _T(off, dev), mode, insert_missing=True)
    f = _np(found).reshape(N_MEMBERS, -1)
    assert f[:, :60].all() and not f[:, 60:62].any() and f[:, 62:].all()
    _assert_same_tiers(a, b, "second call")


@pytest.mark.gpu
@pytest.mark.parametrize("optimizer,mode,create", [("adagrad", "sum", False), ("adagrad", "sum", True), ("adam", "mean", False), ("adam", "mean", True)])
def test_bag_layer_trains_the_group_like_the_pairs(dev, optimizer, mode, create):
    """DynamicEmbeddingBag over the tiered group against three DynamicEmbeddingBags over the pairs, the same bags and grads, three steps: every
    tier's key-sorted export with the state planes is bit-identical — also the check of a grouped step over members whose rows sit in pinned host
    memory.  The gradients are exactly summable (tests/_apply_cases.py); the mean's bags have power-of-two lengths, so that grad / length only
    moves the exponent (by at most 5: sums of at most 2^9 positions stay multiples of 2^-41 below 2^2, exact in fp64 in any order)."""
    from meepoembedding_amd import OPT_ADAGRAD, OPT_ADAM, TieredTableGroup
    from meepoembedding_amd.nn import DynamicEmbeddingBag
    dim = 64
    opt = OPT_ADAGRAD if optimizer == "adagrad" else OPT_ADAM
    a, b = _train_pairs(dev, dim, opt), _train_pairs(dev, dim, opt)
    group = TieredTableGroup(a, max_apply_batch=4096)
    lens = LENS_A if mode == "sum" else [0, 1, 2, 16, 16, 32, 4, 8, 0, 4, 16, 1, 8, 4, 2]
    off = _offsets(lens)
    n = int(off[-1])
    kw = dict(mode=mode, optimizer=optimizer, lr=0.05, create_missing=create)
    layer = DynamicEmbeddingBag(group, **kw).to(dev).train()
    refs = [DynamicEmbeddingBag(p, **kw).to(dev).train() for p in b]
    universe = _universe()
    rng = np.random.default_rng(11)
    for step in range(3):
        keys = universe[rng.integers(0, N_KEYS, n)]              # duplicates inside and across bags, keys of both tiers
        keys[off[6] + 2] = keys[off[6]]
        keys[3] = ABSENT_KEY if not create else keys[3]
        if create:      # ids no table has seen, twice each, in every member's bags
            fresh = synth.keys_np(90 + step, 0, 6)
            for j in range(N_MEMBERS):
                s = int(off[j * BPT]) + 4
                keys[s:s + 6] = fresh
                keys[s + 8:s + 14] = fresh
        head = _T(exact_grads_np(rng, len(lens), dim, positions=n), dev)
        out = layer(_T(keys, dev), _T(off, dev))
        (out * head).sum().backward()
        for j, ref in enumerate(refs):
            mk, mo, _, _ = _member(keys, off, j)
            po = ref(_T(mk, dev), _T(mo, dev))
            (po * head[j * BPT:(j + 1) * BPT]).sum().backward()
            assert torch.equal(out[j * BPT:(j + 1) * BPT].detach(), po.detach()), (step, j)
    _assert_same_tiers(a, b, f"{optimizer} {mode} create={create}")
    assert all(t.status() == 0 for p in a + b for t in (p.hot, p.cold))
    if create:
        assert a[1].cold.size() == N_KEYS - 200 + 18 and a[1].hot.size() == 200, "member 1's hot tier is at its limit: its 18 new ids went cold"
        assert a[0].cold.size() == N_KEYS - 200 and a[0].hot.size() == 200 + 18 and a[2].cold.size() == 0 and a[2].hot.size() >= 18


@pytest.mark.gpu
def test_group_entry_points_refuse(dev):
    """every refusal of the two entry points: the named code, a message, and no byte written"""
    from meepoembedding_amd import LookupTable, TableGroup, _lib
    L = _lib.lib()
    mk = lambda dim=16, **kw: LookupTable(256, dim, device=dev, max_batch=256, **kw)  # noqa: E731
    h0, h1, c0, c1, counted = mk(), mk(), mk(), mk(), mk(track_hits=True)
    hot, cold = TableGroup([h0, h1]), TableGroup([c0, c1])
    wide, three = TableGroup([mk(32), mk(32)]), TableGroup([mk(), mk(), mk()])
    shares = TableGroup([c0, h1])                         # member 1 is the hot group's member 1
    some_counted = TableGroup([counted, mk()])            # one member without counters
    bf16_rows = TableGroup([mk(64, value_dtype=torch.bfloat16), mk(64, value_dtype=torch.bfloat16)])
    f64 = TableGroup([mk(64), mk(64)])
    keys = torch.arange(8, dtype=torch.int64, device=dev)
    off = torch.tensor([0, 3, 5, 8, 8], dtype=torch.int64, device=dev)     # member 0: keys [0, 5), member 1: keys [5, 8)
    out = torch.full((4, 64), -7.0, device=dev)
    found = torch.zeros(8, dtype=torch.uint8, device=dev)

    def lookup(h, c, out_dtype=_lib.DTYPE_F32, mode=0, flags=0, out_ptr=None):
        return L.mee_group_find_pooled_tiered(h, c, keys.data_ptr(), 8, off.data_ptr(), 2, out.data_ptr() if out_ptr is None else out_ptr, out_dtype,
                                              None, mode, flags, None)

    def ensure(h, c):
        return L.mee_group_ensure_tiered(h, c, keys.data_ptr(), 8, off.data_ptr(), 2, found.data_ptr(), None, None)

    def refused(rc, code=_lib.ERR_INVALID_ARG, name=None):
        msg = L.mee_last_error().decode()
        assert rc == code and msg and (name is None or msg.startswith(name + ":")), (rc, msg)

    for fn, name in ((lookup, "mee_group_find_pooled_tiered"), (ensure, "mee_group_ensure_tiered")):
        refused(fn(None, cold._h), name=name); refused(fn(hot._h, None), name=name)                     # a null group
        refused(fn(hot._h, hot._h), name=name)                                                          # hot is cold
        refused(fn(hot._h, wide._h), name=name); refused(fn(hot._h, three._h), name=name)               # another dim, another number of tables
        refused(fn(hot._h, shares._h), name=name)                                                       # one table as both tiers of a member
        refused(fn(bf16_rows._h, f64._h), _lib.ERR_UNSUPPORTED, name); refused(fn(f64._h, bf16_rows._h), _lib.ERR_UNSUPPORTED, name)
    refused(lookup(hot._h, cold._h, mode=2)); refused(lookup(hot._h, cold._h, out_dtype=2)); refused(lookup(hot._h, cold._h, flags=4))
    refused(lookup(hot._h, cold._h, out_dtype=_lib.DTYPE_BF16, out_ptr=out.data_ptr() + 4))             # a bf16 row group is one 8-byte store
    refused(lookup(hot._h, some_counted._h, flags=_lib.TIER_COUNT_COLD)); refused(lookup(some_counted._h, cold._h, flags=_lib.TIER_COUNT_HOT))
    torch.cuda.synchronize(dev)
    assert bool((out == -7.0).all()) and all(t.size() == 0 for t in (h0, h1, c0, c1, counted))
    assert lookup(hot._h, some_counted._h, flags=_lib.TIER_COUNT_HOT) == _lib.ERR_INVALID_ARG            # the HOT tier has no counters at all
    # what is not refused: no bags (nothing written, null buffers), and the plain calls
    assert L.mee_group_find_pooled_tiered(hot._h, cold._h, keys.data_ptr(), 8, None, 0, None, _lib.DTYPE_F32, None, 0, 0, None) == _lib.OK
    assert L.mee_group_ensure_tiered(hot._h, cold._h, keys.data_ptr(), 8, None, 0, found.data_ptr(), None, None) == _lib.OK
    torch.cuda.synchronize(dev)
    assert bool((out == -7.0).all()) and all(t.size() == 0 for t in (h0, h1, c0, c1))
    assert lookup(hot._h, cold._h) == _lib.OK and ensure(hot._h, cold._h) == _lib.OK
    torch.cuda.synchronize(dev)
    assert bool((out.view(-1)[:64] == 0).all()) and bool((out.view(-1)[64:] == -7.0).all())      # four bag rows of dim 16, default rows of 0
    assert h0.size() == 5 and h1.size() == 3 and c0.size() == c1.size() == 0                      # null d_to_cold: all hot


@pytest.mark.gpu
def test_group_lookup_follows_reserve_on_members(dev):
    groups, _, exp = _setup(64, dev)
    keys, off = exp["B"][0], exp["B"][1]
    pairs, _ = _make_pairs(64, dev, _hot_masks(_batches())["half"])
    from meepoembedding_amd import TieredTableGroup
    group = TieredTableGroup(pairs)
    before, fb = group.find_pooled(keys, off, "mean")
    assert torch.equal(before, groups["half"][0].find_pooled(keys, off, "mean")[0])
    pairs[0].hot.reserve(4 * pairs[0].hot.capacity)       # the planes of one hot and of one cold member move
    pairs[1].cold.reserve(3 * pairs[1].cold.capacity)
    after, fa = group.find_pooled(keys, off, "mean")
    assert torch.equal(before, after) and torch.equal(fb, fa)


@pytest.mark.gpu
def test_group_lookup_is_graph_capturable(dev):
    """one launch, no allocation, no host synchronisation: captured on one stream and replayed, it follows the members' rows"""
    pairs, _ = _make_pairs(64, dev, _hot_masks(_batches())["alternating"])
    from meepoembedding_amd import TieredTableGroup
    group = TieredTableGroup(pairs)
    hkeys, hoff = _batches()["A"]
    keys, off = _T(hkeys, dev), _T(hoff, dev)
    out = torch.zeros(N_MEMBERS * BPT, 64, device=dev)
    found = torch.zeros(keys.numel(), dtype=torch.uint8, device=dev)
    eager, ef = group.find_pooled(keys, off, "sum")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        group.find_pooled(keys, off, "sum", out=out, found=found)
    out.zero_(); found.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager) and torch.equal(found, ef)
    # the members' rows are reassigned (one hot-heavy, one cold-heavy member): the replay reads the new rows
    universe = _T(_universe(), dev)
    for j in (0, 1):
        pairs[j].assign(universe, torch.full((N_KEYS, 64), float(j + 2), device=dev))
    eager, _ = group.find_pooled(keys, off, "sum")
    assert not torch.equal(eager, out)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager) and torch.equal(found, ef)
