"""Embedding bags over the hot/cold pair (TieredLookupTable.find_pooled, mee_find_pooled_tiered): the pair must pool like ONE table holding
the union (SPEC.md §3 "Tiering"), bit for bit, wherever a key sits.  CPU: the host logic over two oracle-backed tiers.  GPU: a hot table in HBM
and a cold table whose rows live in pinned host memory, against the oracle AND against one GPU table of the union."""
import numpy as np
import pytest
import torch

import oracle
from _apply_cases import assert_bits_equal_nan_aware
from _cpu_backend import CpuTable
from meepoembedding_amd import synth
from meepoembedding_amd.tiered import TieredLookupTable

EMPTY_KEY = -(1 << 63)
RECLAIMED_KEY = EMPTY_KEY + 1
ABSENT_KEY = 123456789          # in no table of this file
N_KEYS = 3000                   # the distinct keys the batches draw from
HOT_CAP, COLD_CAP = 4096, 8192  # rounded up by the tables to 4112 / 8336 slots
HOT_FILL, COLD_FILL = 3500, 7100   # keys stored per tier: load 0.85 in each, so that probes reach a second bucket in both indexes
INIT = dict(initial_accumulator=0.1, initializer=oracle.INIT_UNIFORM, init_scale=0.05, init_seed=9)

# batch A: the tile-per-bag instance (9.5 keys per bag on average) with long bags (>= 16 keys: the four tiles together) inside it; 13 bags
LENS_A = [0, 1, 2, 15, 16, 17, 40, 3, 0, 5, 16, 1, 7]
# batch B: every bag >= 12 keys: the wave-per-bag instance; 7 bags
LENS_B = [12, 13, 16, 17, 33, 40, 12]


def _offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def _sorted(exp):
    order = np.argsort(exp[0])
    return [None if x is None else x[order] for x in exp]


def _np(x):
    return None if x is None else x.cpu().numpy()


def _batches():
    """-> {name: (keys, offsets)}: distinct stored keys (so that a key has ONE position parity inside its bag), then a repeated key two
    positions on, an absent key and the two reserved keys, planted in short and in long bags"""
    universe = synth.keys_np(61, 0, N_KEYS)
    out, at = {}, 0
    for name, lens in (("A", LENS_A), ("B", LENS_B)):
        off = _offsets(lens)
        keys = universe[at:at + off[-1]].copy()
        at += int(off[-1])
        long_bag = int(np.argmax(lens))
        p = int(off[long_bag])
        keys[p + 6] = keys[p + 4]                       # a duplicate inside a bag, same parity
        keys[p + 9], keys[p + 20], keys[p + 31] = ABSENT_KEY, EMPTY_KEY, RECLAIMED_KEY
        short_bag = lens.index(15) if 15 in lens else 1
        q = int(off[short_bag])
        keys[q + 3], keys[q + 8], keys[q + 11] = RECLAIMED_KEY, ABSENT_KEY, EMPTY_KEY
        out[name] = (keys, off)
    return out


def _hot_masks(batches):
    """the four placements of the N_KEYS keys: name -> bool[N_KEYS], True = the key sits in the hot tier"""
    universe = synth.keys_np(61, 0, N_KEYS)
    rng = np.random.default_rng(7)
    half = rng.random(N_KEYS) < 0.5
    alt = half.copy()
    index_of = {int(k): i for i, k in enumerate(universe)}
    for keys, off in batches.values():       # alternating hot / cold by position inside every bag
        for b in range(off.size - 1):
            for j, k in enumerate(keys[off[b]:off[b + 1]]):
                if int(k) in index_of:
                    alt[index_of[int(k)]] = (j % 2 == 0)
    return {"all_hot": np.ones(N_KEYS, bool), "all_cold": np.zeros(N_KEYS, bool), "half": half, "alternating": alt}


def _tier_keys(hot_mask):
    """-> (hot keys, cold keys): the placement's share of the universe, topped up with filler keys to HOT_FILL / COLD_FILL"""
    universe = synth.keys_np(61, 0, N_KEYS)
    hk, ck = universe[hot_mask], universe[~hot_mask]
    return (np.concatenate([hk, synth.keys_np(61, N_KEYS, HOT_FILL - hk.size)]),
            np.concatenate([ck, synth.keys_np(61, N_KEYS + HOT_FILL, COLD_FILL - ck.size)]))


def _union_keys():
    return synth.keys_np(61, 0, N_KEYS + HOT_FILL + COLD_FILL)   # the universe and every filler key any placement uses


class _CpuTable(CpuTable):
    """tests/_cpu_backend.CpuTable whose apply_* take grad_index, as the LookupTable's do (position i takes row grad_index[i] of grads)"""

    def apply_adagrad(self, keys, grads, lr, eps=1e-10, grad_index=None):
        super().apply_adagrad(keys, grads if grad_index is None else grads[grad_index], lr, eps)

    def apply_adam(self, keys, grads, lr, beta1=0.9, beta2=0.999, eps=1e-8, step=1, grad_index=None):
        super().apply_adam(keys, grads if grad_index is None else grads[grad_index], lr, beta1, beta2, eps, step)


# ---- CPU: the host logic ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt", [oracle.OPT_ADAGRAD, oracle.OPT_ADAM])
def test_tiered_bags_cpu_logic(built, opt):
    dim = 16
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    hot = _CpuTable(HOT_CAP, dim, optimizer=opt, default_value=0.5, **INIT)
    cold = _CpuTable(COLD_CAP, dim, optimizer=opt, default_value=0.25, **INIT)    # its default row must never show
    ref = oracle.OracleTable(16384, dim, optimizer=opt, default_value=0.5, **INIT)
    pair = TieredLookupTable(hot, cold, hot_key_limit=1500)
    universe = synth.keys_np(61, 0, N_KEYS)
    rows = synth.rows_np(universe, dim, 3)
    for s in (slice(0, 1500), slice(1500, N_KEYS)):     # the first half fills the hot tier to its limit, the second goes cold
        pair.insert(T(universe[s]), T(rows[s])); ref.insert(universe[s], rows[s])
    assert hot.size() == 1500 and cold.size() == 1500
    rng = np.random.default_rng(3)

    def check_lookups():
        for keys, off in _batches().values():
            keys = keys.copy()
            keys[::3] = universe[rng.integers(0, N_KEYS, keys[::3].size)]    # keys of both tiers, repeats included
            er, ef = ref.find(keys)
            for mode in ("sum", "mean"):
                out, found = pair.find_pooled(T(keys), T(off), mode)
                assert out.dtype == torch.float32 and np.array_equal(out.numpy(), oracle.pool_rows(er, off, mode)), mode
                assert np.array_equal(found.numpy(), ef)

    check_lookups()
    assert pair.promote(T(universe[1500:1800])) == 0      # the hot tier is at its limit
    assert pair.demote(T(universe[:400])) == 400
    assert pair.promote(T(universe[1500:1800])) == 300
    check_lookups()

    # the step of a pooled lookup: grad_index goes to both tiers (§3 apply_*_indexed on the union)
    keys, off = _batches()["A"]
    bag_of = np.repeat(np.arange(off.size - 1), np.diff(off))
    bag_grads = (rng.standard_normal((off.size - 1, dim)) * 0.01).astype(np.float32)
    if opt == oracle.OPT_ADAGRAD:
        pair.apply_adagrad(T(keys), T(bag_grads), lr=0.02, grad_index=T(bag_of)); ref.apply_adagrad(keys, bag_grads[bag_of], 0.02, 1e-10)
    else:
        pair.apply_adam(T(keys), T(bag_grads), lr=0.002, step=1, grad_index=T(bag_of)); ref.apply_adam(keys, bag_grads[bag_of], 0.002, 0.9, 0.999, 1e-8, 1)

    # insert_missing: new keys (each twice) are created as find_or_insert creates them; found = "present before the call"
    new = synth.keys_np(62, 0, 40)
    keys = np.concatenate([universe[100:160], new, universe[2000:2030], new])
    off = _offsets([7, 0, 50, 13, 60, 40])
    er, ef = ref.find_or_insert(keys)
    out, found = pair.find_pooled(T(keys), T(off), "mean", insert_missing=True)
    assert np.array_equal(found.numpy(), ef) and not ef[60:100].any() and not ef[130:].any()
    assert np.array_equal(out.numpy(), oracle.pool_rows(er, off, "mean"))
    assert pair.size() == ref.size() == N_KEYS + 40
    got, exp = _sorted([_np(x) for x in pair.export(with_state=True)]), _sorted(list(ref.export(with_state=True)))
    assert np.array_equal(got[0], exp[0])
    for a, b in zip(got[1:], exp[1:]):    # both sides are the oracle's arithmetic, a key's duplicates reduced inside the one tier that holds it: equal
        if b is not None:
            assert np.array_equal(a, b)


def test_layer_refusals_over_the_pair(built):
    """per_sample_weights are refused over the pair by name; the bag layer takes bf16, the unpooled layer keeps refusing it"""
    from meepoembedding_amd.nn import DynamicEmbedding, DynamicEmbeddingBag
    pair = TieredLookupTable(_CpuTable(256, 8, optimizer=oracle.OPT_ADAGRAD), _CpuTable(256, 8, optimizer=oracle.OPT_ADAGRAD))
    assert pair.weighted_bags is False and not getattr(pair, "supports_out_dtype", False)
    keys, off = torch.arange(6), torch.tensor([0, 2, 6])
    with pytest.raises(ValueError, match="TieredLookupTable"):
        DynamicEmbeddingBag(pair, mode="sum")(keys, off, per_sample_weights=torch.ones(6))
    with pytest.raises(ValueError, match="TieredLookupTable"):
        DynamicEmbedding(pair, out_dtype=torch.bfloat16)
    layer = DynamicEmbeddingBag(pair, mode="sum", out_dtype=torch.bfloat16)
    out = layer(keys, off)
    assert out.dtype == torch.bfloat16 and out.shape == (2, 8)
    with pytest.raises(ValueError):
        TieredLookupTable(_CpuTable(256, 8), _CpuTable(256, 16))
    with pytest.raises(ValueError):
        pair.find_pooled(keys, off, "max")


# ---- GPU -------------------------------------------------------------------------------------------------------------------
_SETUPS = {}


def _setup(dim, dev):
    """per dim, built once and only read afterwards: the four placements as pairs (hot in HBM, cold rows in pinned host memory), one GPU
    table of the union, and per batch the keys, the offsets and the oracle's rows and found mask"""
    if dim in _SETUPS:
        return _SETUPS[dim]
    from meepoembedding_amd import LookupTable, _lib
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    batches = _batches()
    union_keys = _union_keys()
    ref = oracle.OracleTable(16384, dim, default_value=0.5)
    ref.insert(union_keys, synth.rows_np(union_keys, dim, 3))
    union = LookupTable(16384, dim, device=dev, max_batch=16384, default_value=0.5)
    union.insert(T(union_keys), T(synth.rows_np(union_keys, dim, 3)))
    pairs = {}
    for name, mask in _hot_masks(batches).items():
        hk, ck = _tier_keys(mask)
        hot = LookupTable(HOT_CAP, dim, device=dev, max_batch=8192, default_value=0.5)
        cold = LookupTable(COLD_CAP, dim, device=dev, max_batch=8192, default_value=0.25, value_memory=_lib.MEM_HOST_PINNED)
        hot.insert(T(hk), T(synth.rows_np(hk, dim, 3)))
        cold.insert(T(ck), T(synth.rows_np(ck, dim, 3)))
        assert hot.size() == HOT_FILL >= 0.85 * hot.capacity and cold.size() == COLD_FILL >= 0.85 * cold.capacity
        pairs[name] = TieredLookupTable(hot, cold)
    exp = {}
    for name, (keys, off) in batches.items():
        rows, found = ref.find(keys)
        exp[name] = (T(keys), T(off), rows, found)
    _SETUPS[dim] = (pairs, union, exp)
    return _SETUPS[dim]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["sum", "mean"])
@pytest.mark.parametrize("dim", [16, 64, 128, 100, 260])
def test_tiered_find_pooled_is_the_union_bit_for_bit(dev, dim, mode):
    pairs, union, exp = _setup(dim, dev)
    for bname, (keys, off, rows, ef) in exp.items():
        want = oracle.pool_rows(rows, off.cpu().numpy(), mode)
        uo, uf = union.find_pooled(keys, off, mode)
        assert_bits_equal_nan_aware(_np(uo), want, f"union {bname}")
        assert np.array_equal(_np(uf), ef)
        for pname, pair in pairs.items():
            out, found = pair.find_pooled(keys, off, mode)
            assert_bits_equal_nan_aware(_np(out), want, f"{pname} {bname}")
            assert_bits_equal_nan_aware(_np(out), _np(uo), f"{pname} {bname} against the union")
            assert np.array_equal(_np(found), _np(uf)) and np.array_equal(_np(found), ef), (pname, bname)
    keys, off, _, _ = exp["A"]
    for pname, pair in pairs.items():
        # zero bags: nothing is written
        out, _ = pair.find_pooled(keys, off[:1], mode)
        assert out.shape == (0, dim)
        # three empty bags, over no keys and over keys no bag covers
        out, found = pair.find_pooled(keys[:0], torch.zeros(4, dtype=torch.int64, device=dev), mode)
        assert out.shape == (3, dim) and not out.any() and found.numel() == 0
        out, _ = pair.find_pooled(keys, torch.full((4,), 5, dtype=torch.int64, device=dev), mode)
        assert out.shape == (3, dim) and not out.any()
        # offsets are the caller's: bags past the key array are cut at its end, a decreasing pair is an empty bag
        bad = torch.tensor([0, 10, 5, 90, 1 << 40, 1 << 41], dtype=torch.int64, device=dev)   # [0,10) [10,5)=empty [5,90) [90,n) empty
        out, found = pair.find_pooled(keys, bad, mode, found=torch.full((keys.numel(),), 7, dtype=torch.uint8, device=dev))
        uo, uf = union.find_pooled(keys, bad, mode, found=torch.full((keys.numel(),), 7, dtype=torch.uint8, device=dev))
        n = keys.numel()
        clamped = np.array([0, 10, 10, 10, 5, 90, 90, n, n, n], dtype=np.int64)   # the five bags as (begin, end) runs of a plain offset list
        want = oracle.pool_rows(exp["A"][2], clamped, mode)[[0, 1, 4, 6, 8]]
        assert np.array_equal(_np(out), want) and np.array_equal(_np(out), _np(uo)) and np.array_equal(_np(found), _np(uf)), pname


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [64, 100])
def test_tiered_find_pooled_bf16_rounds_the_finished_row_once(dev, dim):
    pairs, _, exp = _setup(dim, dev)
    for pname in ("alternating", "all_cold"):
        for keys, off, _, ef in exp.values():
            for mode in ("sum", "mean"):
                o32, _ = pairs[pname].find_pooled(keys, off, mode)
                o16, found = pairs[pname].find_pooled(keys, off, mode, out_dtype=torch.bfloat16)
                assert o16.dtype == torch.bfloat16 and torch.equal(o16.view(torch.int16), o32.to(torch.bfloat16).view(torch.int16)), (pname, mode)
                assert np.array_equal(_np(found), ef)


@pytest.mark.gpu
@pytest.mark.parametrize("room", [True, False])
def test_tiered_find_pooled_insert_missing(dev, room):
    """new keys, each occurring twice, with room in the hot tier and with hot_key_limit already reached: the pair ends as ONE table does
    after find_or_insert + find_pooled, `found` says "present before the call", and the new keys sit in the tier find_or_insert would pick"""
    from meepoembedding_amd import LookupTable, _lib
    dim = 64
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    hot = LookupTable(HOT_CAP, dim, device=dev, max_batch=4096, default_value=0.5, **INIT)
    cold = LookupTable(COLD_CAP, dim, device=dev, max_batch=4096, default_value=0.5, value_memory=_lib.MEM_HOST_PINNED, **INIT)
    one = LookupTable(16384, dim, device=dev, max_batch=4096, default_value=0.5, **INIT)
    pair = TieredLookupTable(hot, cold, hot_key_limit=3000 if room else 500)
    universe = synth.keys_np(61, 0, 1000)
    rows = synth.rows_np(universe, dim, 3)
    for s in (slice(0, 500), slice(500, 1000)):
        pair.insert(T(universe[s]), T(rows[s])); one.insert(T(universe[s]), T(rows[s]))
    if room:
        pair.demote(T(universe[500:]))
    assert hot.size() == 500 and cold.size() == 500
    new = synth.keys_np(62, 0, 60)
    keys = np.concatenate([universe[100:160], new, universe[700:760], new])
    off = T(_offsets([0, 17, 43, 1, 60, 119]))
    for mode in ("sum", "mean"):
        if mode == "mean":      # a second batch of new keys, so that both modes create some
            new = synth.keys_np(63, 0, 60)
            keys = np.concatenate([universe[100:160], new, universe[700:760], new])
        _, ef = one.find_or_insert(T(keys))
        want, _ = one.find_pooled(T(keys), off, mode)
        out, found = pair.find_pooled(T(keys), off, mode, insert_missing=True)
        assert torch.equal(out, want) and torch.equal(found, ef)
        assert not found[60:120].any() and not found[180:].any() and found[:60].all() and found[120:180].all()
        in_hot, in_cold = hot.find(T(new))[1], cold.find(T(new))[1]
        assert bool(in_hot.all() and not in_cold.any()) if room else bool(in_cold.all() and not in_hot.any())
    assert pair.size() == one.size() == 1120 and hot.status() == 0 and cold.status() == 0
    got, exp = _sorted([_np(x) for x in pair.export()]), _sorted([_np(x) for x in one.export()])
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])


@pytest.mark.gpu
def test_tiered_find_pooled_feeds_the_policy_like_find(dev):
    """two identical policy pairs, sample_every = 4: eight find(keys) on one, eight find_pooled(keys, offsets) on the other leave the same
    hit counters on both tiers (cold hits always, hot hits on every 4th call), and rebalance() then moves the same keys"""
    from meepoembedding_amd import LookupTable, _lib
    dim = 16
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    universe = synth.keys_np(61, 0, 1000)
    once, twice = np.concatenate([universe[:100], universe[500:600]]), np.concatenate([universe[100:130], universe[600:630]])
    keys = np.concatenate([once, twice, [ABSENT_KEY, EMPTY_KEY], twice])
    off = T(_offsets([3, 0, 40, 17] + [10] * 26 + [2]))    # 10.4 keys per bag: a tile per bag, two long bags on the four tiles together
    assert int(off[-1]) == keys.size

    def make():
        hot = LookupTable(HOT_CAP, dim, device=dev, max_batch=4096, track_hits=True)
        cold = LookupTable(COLD_CAP, dim, device=dev, max_batch=4096, value_memory=_lib.MEM_HOST_PINNED, track_hits=True)
        hot.insert(T(universe[:500]), T(synth.rows_np(universe[:500], dim, 3)))
        cold.insert(T(universe[500:]), T(synth.rows_np(universe[500:], dim, 3)))
        return TieredLookupTable(hot, cold, hot_key_limit=3000, sample_every=4)

    a, b = make(), make()
    assert a.policy and b.policy
    for _ in range(8):
        ra, fa = a.find(T(keys))
        ob, fb = b.find_pooled(T(keys), off)
        assert torch.equal(fa, fb) and np.array_equal(_np(ob), oracle.pool_rows(_np(ra), _np(off), "sum"))
    sets = {}
    for k_hot, k_cold in ((1, 1), (3, 9)):    # hot: 2 sampled calls, cold: 8 calls — 3 / 9 hits need a key that occurs twice in the batch
        for name, pair in (("find", a), ("pooled", b)):
            sets[name] = (np.sort(_np(pair.hot.hits_scan(k_hot, 0xFFFFFFFF, 4096))), np.sort(_np(pair.cold.hits_scan(k_cold, 0xFFFFFFFF, 4096))))
        want_hot = np.sort(np.concatenate([once[:100], twice[:30]]) if k_hot == 1 else twice[:30])
        want_cold = np.sort(np.concatenate([once[100:], twice[30:]]) if k_cold == 1 else twice[30:])
        for name in ("find", "pooled"):
            assert np.array_equal(sets[name][0], want_hot) and np.array_equal(sets[name][1], want_cold), (name, k_hot, k_cold)
    assert a.rebalance() == b.rebalance() == (130, 0)
    assert np.array_equal(np.sort(_np(a.hot.export()[0])), np.sort(_np(b.hot.export()[0]))) and a.hot.size() == 630


@pytest.mark.gpu
@pytest.mark.parametrize("optimizer,mode,create,dups", [("adagrad", "sum", False, False), ("adam", "mean", True, True),
                                                        ("adagrad", "mean", True, False), ("adam", "sum", False, True),
                                                        ("adam", "sum", True, False), ("adagrad", "mean", False, True)])
def test_bag_layer_trains_the_pair_like_one_table(dev, optimizer, mode, create, dups):
    """DynamicEmbeddingBag over the pair and over ONE table of the union, 6 steps, keys moving between the tiers (with their optimizer state)
    between steps: the key-sorted exports with state are bit-identical without duplicate keys in a batch, within SPEC.md §4's tolerance with"""
    from meepoembedding_amd import OPT_ADAGRAD, OPT_ADAM, LookupTable, _lib
    from meepoembedding_amd.nn import DynamicEmbeddingBag
    dim = 64
    opt = OPT_ADAGRAD if optimizer == "adagrad" else OPT_ADAM
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    kw = dict(device=dev, optimizer=opt, max_batch=4096, default_value=0.5, **INIT)
    hot, cold = LookupTable(HOT_CAP, dim, **kw), LookupTable(COLD_CAP, dim, value_memory=_lib.MEM_HOST_PINNED, **kw)
    one = LookupTable(16384, dim, **kw)
    pair = TieredLookupTable(hot, cold, hot_key_limit=1000)
    universe = synth.keys_np(61, 0, 2000)
    rows = synth.rows_np(universe, dim, 3)
    for s in (slice(0, 1000), slice(1000, 2000)):
        pair.insert(T(universe[s]), T(rows[s])); one.insert(T(universe[s]), T(rows[s]))
    layers = [DynamicEmbeddingBag(t, mode=mode, optimizer=optimizer, lr=0.05, create_missing=create).to(dev).train() for t in (pair, one)]
    rng = np.random.default_rng(11)
    lens = [0, 1, 2, 15, 16, 17, 40, 3, 9, 5, 12]
    off = T(_offsets(lens))
    n = int(sum(lens))
    head = torch.from_numpy(rng.standard_normal((len(lens), dim)).astype(np.float32)).to(dev)
    for step in range(6):
        idx = rng.integers(0, 2000, n) if dups else rng.permutation(2000)[:n]
        keys = universe[idx]
        if dups:
            keys[n // 2:n // 2 + 20] = keys[:20]
        if create:      # ids no table has seen (with create_missing they enter; the pair picks the tier)
            keys[5:25:2] = synth.keys_np(70 + step, 0, 10)
            if dups:
                keys[60:70] = keys[5:25:2]
        else:
            keys[7] = ABSENT_KEY      # reads the default row and is not trained
        outs = []
        for layer in layers:
            out = layer(T(keys), off)
            (out * head).sum().backward()
            outs.append(out.detach())
        if dups:    # rows within rtol 1e-6 / atol 1e-9 of each other (SPEC.md §4), up to 40 of them (|x| < 1) added per bag
            torch.testing.assert_close(outs[0], outs[1], rtol=1e-5, atol=5e-5)
        else:
            assert torch.equal(outs[0], outs[1]), step
        if step % 2 == 0:
            pair.demote(T(universe[100 * step:100 * step + 150]))
        else:
            pair.promote(T(universe[1000 + 100 * step:1000 + 100 * step + 150]))
    assert pair.size() == one.size() and hot.size() > 0 and cold.size() > 0 and hot.status() == cold.status() == one.status() == 0
    got, exp = _sorted([_np(x) for x in pair.export(with_state=True)]), _sorted([_np(x) for x in one.export(with_state=True)])
    assert np.array_equal(got[0], exp[0])
    for a, b in zip(got[1:], exp[1:]):
        if b is not None:
            if dups:
                np.testing.assert_allclose(a, b, rtol=1e-6, atol=1e-9)
            else:
                assert np.array_equal(a, b)


@pytest.mark.gpu
def test_tiered_find_pooled_refusals(dev):
    from meepoembedding_amd import LookupTable, MeepoError, _lib
    from meepoembedding_amd.nn import DynamicEmbedding, DynamicEmbeddingBag
    L = _lib.lib()
    a, b = LookupTable(256, 16, device=dev, max_batch=256), LookupTable(256, 16, device=dev, max_batch=256, track_hits=True)
    wide = LookupTable(256, 32, device=dev, max_batch=256)
    keys = torch.arange(8, dtype=torch.int64, device=dev)
    off = torch.tensor([0, 3, 8], dtype=torch.int64, device=dev)
    out = torch.zeros(2, 16, device=dev)

    def call(hot, cold, out_dtype=_lib.DTYPE_F32, mode=0, flags=0, out_ptr=None):
        return L.mee_find_pooled_tiered(hot, cold, keys.data_ptr(), 8, off.data_ptr(), 2, out.data_ptr() if out_ptr is None else out_ptr, out_dtype, None,
                                        mode, flags, None)

    assert call(a._h, b._h) == _lib.OK
    assert call(a._h, wide._h) == _lib.ERR_INVALID_ARG and b"dim" in L.mee_last_error()        # mismatched dims
    assert call(a._h, a._h) == _lib.ERR_INVALID_ARG                                              # hot is cold
    assert call(None, b._h) == _lib.ERR_INVALID_ARG and call(a._h, None) == _lib.ERR_INVALID_ARG
    assert call(a._h, b._h, flags=_lib.TIER_COUNT_HOT) == _lib.ERR_INVALID_ARG                   # the hot tier keeps no counters
    assert call(b._h, a._h, flags=_lib.TIER_COUNT_COLD) == _lib.ERR_INVALID_ARG                  # nor does this cold tier
    assert call(a._h, b._h, flags=_lib.TIER_COUNT_COLD) == _lib.OK and call(b._h, a._h, flags=_lib.TIER_COUNT_HOT) == _lib.OK
    assert call(a._h, b._h, flags=4) == _lib.ERR_INVALID_ARG                                     # unknown flag bits
    assert call(a._h, b._h, mode=2) == _lib.ERR_INVALID_ARG and call(a._h, b._h, out_dtype=2) == _lib.ERR_INVALID_ARG
    assert call(a._h, b._h, out_dtype=_lib.DTYPE_BF16, out_ptr=out.data_ptr() + 4) == _lib.ERR_INVALID_ARG   # a bf16 row group is one 8-byte store
    torch.cuda.synchronize(dev)
    with pytest.raises(ValueError):
        TieredLookupTable(a, wide)
    pair = TieredLookupTable(a, b)
    with pytest.raises(ValueError):
        pair.find_pooled(keys, off, out=torch.zeros(2, 16, device=dev), out_dtype=torch.bfloat16)
    with pytest.raises(MeepoError):
        pair.find_pooled(keys, off.cpu())
    opt_pair = TieredLookupTable(LookupTable(256, 16, device=dev, max_batch=256, optimizer=1), LookupTable(256, 16, device=dev, max_batch=256, optimizer=1))
    with pytest.raises(ValueError, match="TieredLookupTable"):
        DynamicEmbeddingBag(opt_pair, mode="sum").to(dev)(keys, off, per_sample_weights=torch.ones(8, device=dev))
    with pytest.raises(ValueError, match="TieredLookupTable"):
        DynamicEmbedding(opt_pair, out_dtype=torch.bfloat16)
    assert DynamicEmbeddingBag(opt_pair, mode="mean", out_dtype=torch.bfloat16).to(dev)(keys, off).dtype == torch.bfloat16


@pytest.mark.gpu
def test_tiered_find_pooled_is_graph_capturable(dev):
    """one launch, no allocation, no host synchronisation: the pooled lookup of the pair is captured and replayed like mee_find_pooled"""
    pairs, _, exp = _setup(64, dev)
    keys, off, rows, ef = exp["A"]
    pair = pairs["alternating"]
    out = torch.zeros(off.numel() - 1, 64, device=dev)
    found = torch.zeros(keys.numel(), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pair.find_pooled(keys, off, "sum", out=out, found=found)
    for _ in range(2):
        out.zero_(); found.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_np(out), oracle.pool_rows(rows, _np(off), "sum")) and np.array_equal(_np(found), ef)
