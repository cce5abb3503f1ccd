"""The UNPOOLED operators over a collection of hot/cold pairs (TieredTableGroup.find / find_or_insert / apply_adagrad / apply_adam,
mee_group_find_tiered, mee_group_find_or_insert_tiered): by definition (SPEC.md §3 "Tiering") each is the pair's operator per member on its segment
of the jagged batch.  The reference everywhere is that call sequence on the pairs themselves (lookups, which change nothing) or on independent
copies of the pairs (everything that changes a table); on the CPU also the oracle.  CPU: the host logic over oracle-backed tiers.  GPU: three pairs
(hot in HBM, cold rows in pinned host memory) of different sizes; the segments start behind position 0, end before n and are no multiples of 4,
so one wave's tiles serve two members."""
import numpy as np
import pytest
import torch

import oracle
from _apply_cases import exact_grads_np
from _cpu_backend import CpuTable
from meepoembedding_amd import synth

EMPTY_KEY = -(1 << 63)
RECLAIMED_KEY = EMPTY_KEY + 1
ABSENT_KEY = 123456789          # in no table of this file
N_KEYS = 400                    # the distinct keys the batches draw from (every non-empty member stores all of them, with rows of its own)
N_MEMBERS = 3
CAPS = [(1000, 3000), (4000, 2000), (6000, 1500)]   # requested slots per member (hot, cold): all different
EMPTY_MEMBER = 2                # holds no key in either tier
HOT_DEFAULT = [0.5, 0.75, 1.5]
COLD_DEFAULT = [0.25, 0.125, 2.0]   # a cold table's default row must never show
INIT = dict(initial_accumulator=0.1, initializer=oracle.INIT_UNIFORM, init_scale=0.05)
HEAD, TAIL = 3, 2               # positions in front of offsets[0] and behind offsets[n_tables]: no segment holds them
# segment lengths per member: 0, 1, 5, 37 and lengths past a wave step (8 positions at dim 64, 4 otherwise) and past a block (32 / 16 positions)
SEGMENTS = {"A": [37, 70, 5], "B": [1, 0, 41], "C": [5, 37, 0]}
BF16 = torch.bfloat16


def _offsets(lens):
    return (HEAD + np.concatenate([[0], np.cumsum(lens)])).astype(np.int64)


def _np(x):
    return None if x is None else x.cpu().numpy()


def _sorted(exp):
    exp = [_np(x) if isinstance(x, torch.Tensor) else x for x in exp]
    order = np.argsort(exp[0])
    return [None if x is None else x[order] for x in exp]


def _universe():
    return synth.keys_np(71, 0, N_KEYS)


def _batches():
    """-> {name: (keys [HEAD + sum(lens) + TAIL], offsets [N_MEMBERS + 1])}: distinct stored keys (also in the head and the tail, which no segment
    holds), and in the longest segment a key repeated two positions on, an absent key and the two reserved keys"""
    universe = _universe()
    out, at = {}, 0
    for name, lens in SEGMENTS.items():
        off = _offsets(lens)
        n = int(off[-1]) + TAIL
        keys = universe[at:at + n].copy()
        at += n
        p = int(off[int(np.argmax(lens))])
        keys[p + 6] = keys[p + 4]
        keys[p + 9], keys[p + 20], keys[p + 31] = ABSENT_KEY, EMPTY_KEY, RECLAIMED_KEY
        keys[p + 1], keys[p + 2] = RECLAIMED_KEY, ABSENT_KEY       # ... and inside the segment's first wave step
        out[name] = (keys, off)
    assert at <= N_KEYS
    return out


def _hot_masks(batches):
    """the four placements of the N_KEYS keys: name -> bool[N_KEYS], True = the key sits in the hot tier"""
    universe = _universe()
    half = np.random.default_rng(7).random(N_KEYS) < 0.5
    alt = half.copy()
    index_of = {int(k): i for i, k in enumerate(universe)}
    for keys, off in batches.values():       # alternating hot / cold by position inside every segment
        for j in range(N_MEMBERS):
            for q, k in enumerate(keys[off[j]:off[j + 1]]):
                if int(k) in index_of:
                    alt[index_of[int(k)]] = (q % 2 == 0)
    return {"all_hot": np.ones(N_KEYS, bool), "all_cold": np.zeros(N_KEYS, bool), "half": half, "alternating": alt}


class _CpuTable(CpuTable):
    """tests/_cpu_backend.CpuTable whose apply_* take grad_index, as the LookupTable's do"""

    def apply_adagrad(self, keys, grads, lr, eps=1e-10, grad_index=None):
        super().apply_adagrad(keys, grads if grad_index is None else grads[grad_index], lr, eps)

    def apply_adam(self, keys, grads, lr, beta1=0.9, beta2=0.999, eps=1e-8, step=1, grad_index=None):
        super().apply_adam(keys, grads if grad_index is None else grads[grad_index], lr, beta1, beta2, eps, step)


# ---- CPU: the host logic -----------------------------------------------------------------------------------------------------
def _cpu_pairs(dim, opt, fill=True, track_hits=False):
    """three oracle-backed pairs: member 0 keeps room in its hot tier, member 1's is at its limit after the first 200 keys, member 2 starts empty with
    room -> (pairs, the oracle's one table per member)"""
    from meepoembedding_amd.tiered import TieredLookupTable
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    universe = _universe()
    pairs, refs = [], []
    for j in range(N_MEMBERS):
        kw = dict(optimizer=opt, init_seed=9 + j, **INIT)
        hot = _CpuTable(1024, dim, default_value=HOT_DEFAULT[j], track_hits=track_hits, **kw)
        cold = _CpuTable(2048, dim, default_value=COLD_DEFAULT[j], track_hits=track_hits, **kw)
        pair = TieredLookupTable(hot, cold, hot_key_limit=[900, 200, 900][j], sample_every=2)
        ref = oracle.OracleTable(8192, dim, default_value=HOT_DEFAULT[j], **kw)
        if fill and j != EMPTY_MEMBER:
            rows = synth.rows_np(universe, dim, 3 + j)
            for s in (slice(0, 200), slice(200, N_KEYS)):
                pair.insert(T(universe[s]), T(rows[s])); ref.insert(universe[s], rows[s])
        pairs.append(pair); refs.append(ref)
    return pairs, refs


def _assert_same_pairs(a, b, what):
    for j, (pa, pb) in enumerate(zip(a, b)):
        for tier in ("hot", "cold"):
            got, exp = _sorted(getattr(pa, tier).export(with_state=True)), _sorted(getattr(pb, tier).export(with_state=True))
            assert np.array_equal(got[0], exp[0]), (what, j, tier, got[0].size, exp[0].size)
            for x, y in zip(got[1:], exp[1:]):
                assert (x is None and y is None) or np.array_equal(x.view(np.uint32), y.view(np.uint32)), (what, j, tier)


def test_constructor_attributes_and_offsets_validation(built):
    from meepoembedding_amd import TieredTableGroup
    from meepoembedding_amd.nn import DynamicEmbeddingCollection
    pairs, _ = _cpu_pairs(8, oracle.OPT_ADAGRAD, fill=False)
    g = TieredTableGroup(pairs)
    assert TieredTableGroup.supports_out_dtype is True and g.supports_out_dtype is True and g.supports_pooled_out_dtype is True
    assert g.weighted_bags is False and g.pools_with_insert is True
    keys = torch.arange(6)
    for bad in (torch.tensor([0, 2, 4]), torch.tensor([0, 1, 2, 3, 6]), torch.tensor([[0, 2], [4, 6]])):
        for op in (g.find, g.find_or_insert):
            with pytest.raises(ValueError, match="n_tables"):
                op(keys, bad)
        with pytest.raises(ValueError, match="n_tables"):
            g.apply_adagrad(keys, bad, torch.zeros(6, 8), 0.1)
        with pytest.raises(ValueError, match="n_tables"):
            g.apply_adam(keys, bad, torch.zeros(6, 8), 0.1)
    with pytest.raises(ValueError, match="out_dtype"):
        g.find(keys, torch.tensor([0, 2, 4, 6]), out_dtype=torch.float16)
    assert g.size() == 0, "a refused call creates nothing"
    # no keys, and offsets past the keys (cut at n)
    out, found = g.find(keys[:0], torch.zeros(4, dtype=torch.int64))
    assert out.shape == (0, 8) and found.numel() == 0
    out, found = g.find(keys, torch.tensor([0, 2, 4, 60]))
    assert out.shape == (6, 8) and not found.any()
    assert DynamicEmbeddingCollection(g, out_dtype=BF16).out_dtype == BF16        # the layer takes the group, bf16 rows included


def test_sharded_group_over_a_tiered_group_is_refused_by_name(built):
    """ShardedTableGroup over a group of pairs is not part of the unpooled operators: the constructor says so, before it looks at a process group"""
    from meepoembedding_amd import TieredTableGroup
    from meepoembedding_amd.sharded import ShardedTableGroup
    pairs, _ = _cpu_pairs(8, oracle.OPT_ADAGRAD, fill=False)
    with pytest.raises(ValueError, match="TieredTableGroup is a group of hot/cold pairs"):
        ShardedTableGroup(TieredTableGroup(pairs), router=None)


@pytest.mark.parametrize("opt", [oracle.OPT_ADAGRAD, oracle.OPT_ADAM])
def test_tiered_group_find_cpu_logic(built, opt):
    from meepoembedding_amd import TieredTableGroup
    from meepoembedding_amd.nn import DynamicEmbeddingBag, DynamicEmbeddingCollection
    dim = 16
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    universe = _universe()
    pairs, oracles = _cpu_pairs(dim, opt)
    refs, _ = _cpu_pairs(dim, opt)            # independent copies: the per-pair loop runs on these
    group = TieredTableGroup(pairs)

    def loop(fn, keys, off, rows=None):
        """the reference: pair.<fn> per member on its slice"""
        outs = []
        for j, ref in enumerate(refs):
            s, e = int(off[j]), int(off[j + 1])
            outs.append(getattr(ref, fn)(T(keys[s:e])) if rows is None else getattr(ref, fn)(T(keys[s:e]), T(rows[s:e])))
        return outs

    # find: equal to the per-pair loop and to the oracle's table of each member; positions outside the segments are not touched
    for keys, off in _batches().values():
        out = torch.full((keys.size, dim), -7.0)
        found = torch.full((keys.size,), 7, dtype=torch.uint8)
        group.find(T(keys), T(off), out=out, found=found)
        for j, (po, pf) in enumerate(loop("find", keys, off)):
            s, e = int(off[j]), int(off[j + 1])
            eo, ef = oracles[j].find(keys[s:e])
            assert torch.equal(out[s:e], po) and torch.equal(found[s:e], pf) and np.array_equal(out[s:e].numpy(), eo) and np.array_equal(found[s:e].numpy(), ef)
        assert bool((out[:HEAD] == -7.0).all() and (out[int(off[-1]):] == -7.0).all() and (found[:HEAD] == 7).all() and (found[int(off[-1]):] == 7).all())
        o16, f16 = group.find(T(keys), T(off), out_dtype=BF16)
        o32, f32 = group.find(T(keys), T(off))
        assert o16.dtype == BF16 and torch.equal(o16, o32.to(BF16)) and torch.equal(f16, f32)     # the fp32 rows rounded once

    # find_or_insert: new keys, one of them twice in its segment; member 0 has room (hot), member 1 has none (cold), member 2 is empty (creates all)
    new = synth.keys_np(72, 0, 12)
    seg = np.concatenate([universe[:20], new, [RECLAIMED_KEY, EMPTY_KEY], universe[300:310], new[:5]])          # 49 keys per member
    keys = np.concatenate([universe[390:390 + HEAD], seg, seg, seg, universe[395:395 + TAIL]])
    off = _offsets([seg.size] * N_MEMBERS)
    out, found = group.find_or_insert(T(keys), T(off))
    for j, (po, pf) in enumerate(loop("find_or_insert", keys, off)):
        s, e = int(off[j]), int(off[j + 1])
        eo, ef = oracles[j].find_or_insert(seg)
        ok = ~np.isin(seg, [RECLAIMED_KEY, EMPTY_KEY])     # (the CPU adapter's creation pass hands a reserved key the COLD default; the kernels leave it alone)
        assert torch.equal(out[s:e], po) and torch.equal(found[s:e], pf) and np.array_equal(out[s:e].numpy()[ok], eo[ok]) and np.array_equal(found[s:e].numpy(), ef), j
    f = found[HEAD:HEAD + 3 * seg.size].numpy().reshape(N_MEMBERS, -1)
    assert not f[:, 20:34].any() and not f[:, 44:].any() and f[0, :20].all() and f[1, 34:44].all() and not f[EMPTY_MEMBER].any()
    rows = out[HEAD:HEAD + 3 * seg.size].reshape(N_MEMBERS, seg.size, dim)
    assert torch.equal(rows[:, 20:25], rows[:, 44:49]), "a repeated new key returns the same initial row at every occurrence"
    in_hot = [p.hot.find(T(new))[1].numpy() for p in pairs]
    in_cold = [p.cold.find(T(new))[1].numpy() for p in pairs]
    assert in_hot[0].all() and not in_cold[0].any() and in_cold[1].all() and not in_hot[1].any() and in_hot[2].all() and not in_cold[2].any()
    _assert_same_pairs(pairs, refs, "find_or_insert")
    o16, _ = group.find_or_insert(T(keys), T(off), out_dtype=BF16)
    assert o16.dtype == BF16 and torch.equal(o16[HEAD:int(off[-1])], out[HEAD:int(off[-1])].to(BF16))
    loop("find_or_insert", keys, off)     # (the copies make the same second call: nothing new)
    _assert_same_pairs(pairs, refs, "second find_or_insert")

    # the step over the jagged batch: duplicates, keys of both tiers, an absent and a reserved key; every pair ends as its copy and as the oracle's table
    rng = np.random.default_rng(5)
    keys, off = _batches()["A"]
    keys = keys.copy()
    keys[off[1]:off[1] + 8] = keys[off[0]:off[0] + 8]                 # member 1 repeats keys of member 0: different tables, not duplicates
    keys[off[1] + 40:off[1] + 44] = keys[off[1] + 10:off[1] + 14]     # member 1: keys twice in its segment
    grads = exact_grads_np(rng, keys.size, dim)
    for step in (1, 2):
        if opt == oracle.OPT_ADAGRAD:
            group.apply_adagrad(T(keys), T(off), T(grads), 0.02)
        else:
            group.apply_adam(T(keys), T(off), T(grads), 0.002, step=step)
        for j, ref in enumerate(refs):
            s, e = int(off[j]), int(off[j + 1])
            if opt == oracle.OPT_ADAGRAD:
                ref.apply_adagrad(T(keys[s:e]), T(grads[s:e]), 0.02)
                oracles[j].apply_adagrad(keys[s:e], grads[s:e], 0.02, 1e-10)
            else:
                ref.apply_adam(T(keys[s:e]), T(grads[s:e]), 0.002, step=step)
                oracles[j].apply_adam(keys[s:e], grads[s:e], 0.002, 0.9, 0.999, 1e-8, step)
    _assert_same_pairs(pairs, refs, "step")
    for j in range(N_MEMBERS):
        got, exp = _sorted(pairs[j].export(with_state=True)), _sorted(oracles[j].export(with_state=True))
        for a, b in zip(got, exp):
            assert (a is None and b is None) or np.array_equal(a, b), j

    # the layer: DynamicEmbeddingCollection over the group, three training steps against the per-pair loop, bf16 rows; eval creates nothing
    name = "adagrad" if opt == oracle.OPT_ADAGRAD else "adam"
    layer = DynamicEmbeddingCollection(group, optimizer=name, lr=0.05, out_dtype=BF16).train()
    for step in range(1, 4):
        fresh = synth.keys_np(90 + step, 0, 6)
        seg = np.concatenate([universe[rng.integers(0, N_KEYS, 20)], fresh, fresh[:3]])
        keys = np.concatenate([seg, seg, seg])
        off = np.arange(N_MEMBERS + 1, dtype=np.int64) * seg.size
        head = exact_grads_np(rng, keys.size, dim)
        out = layer(T(keys), T(off))
        (out.float() * T(head)).sum().backward()
        assert out.dtype == BF16
        for j, ref in enumerate(refs):
            s, e = int(off[j]), int(off[j + 1])
            po, _ = ref.find_or_insert(T(keys[s:e]))
            assert torch.equal(out[s:e].detach(), po.to(BF16)), (step, j)
            if name == "adagrad":
                ref.apply_adagrad(T(keys[s:e]), T(head[s:e]), 0.05, 1e-10)
            else:
                ref.apply_adam(T(keys[s:e]), T(head[s:e]), 0.05, 0.9, 0.999, 1e-8, step)
    _assert_same_pairs(pairs, refs, "layer")
    sizes = [p.size() for p in pairs]
    unseen = synth.keys_np(99, 0, 9)
    out = layer.eval()(T(np.concatenate([unseen, unseen, unseen])), T(np.arange(N_MEMBERS + 1, dtype=np.int64) * 9))
    assert [p.size() for p in pairs] == sizes and torch.equal(out[:9], torch.full((9, dim), HOT_DEFAULT[0]).to(BF16))
    # weighted bags over the group stay refused, by name
    bag = DynamicEmbeddingBag(group, mode="sum", optimizer=name).train()
    with pytest.raises(ValueError, match="TieredTableGroup"):
        bag(T(keys), T(np.arange(0, keys.size + 1, keys.size // N_MEMBERS, dtype=np.int64)), per_sample_weights=torch.ones(keys.size))


def test_tiered_group_find_cpu_counts_like_the_pairs(built):
    """with the policy on, a fixed sequence of calls leaves the counters the pairs' own calls leave: cold hits always, hot hits on every second call"""
    from meepoembedding_amd import TieredTableGroup
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    pairs, _ = _cpu_pairs(8, oracle.OPT_NONE, track_hits=True)
    refs, _ = _cpu_pairs(8, oracle.OPT_NONE, track_hits=True)
    group = TieredTableGroup(pairs, sample_every=2)
    assert group.policy
    keys, off = _batches()["A"]
    keys = keys.copy()
    keys[off[1]:off[2]] = _universe()[180:250]       # member 1's segment: 20 keys of its hot tier, 50 of its cold tier
    for call in ("find", "find", "find_or_insert", "find", "find"):
        getattr(group, call)(T(keys), T(off))
        for j, ref in enumerate(refs):
            getattr(ref, call)(T(keys[off[j]:off[j + 1]]))
    for a, b in zip(pairs, refs):
        assert a.hot.hits == b.hot.hits and a.cold.hits == b.cold.hits
    assert len(pairs[1].cold.hits) == 50 and set(pairs[1].cold.hits.values()) == {5}, "cold hits: every call"
    assert len(pairs[1].hot.hits) == 20 and set(pairs[1].hot.hits.values()) == {2}, "hot hits: the second and the fourth call"


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


def _make_pairs(dim, dev, hot_mask, **kw):
    """three pairs of CAPS' sizes: members 0 and 1 hold the universe split by hot_mask (member 1 by its complement where the mask is mixed), each tier
    topped up to a load of 0.86 with filler keys, member 0 with tombstones on its probe paths; EMPTY_MEMBER holds nothing"""
    from meepoembedding_amd import LookupTable, _lib
    from meepoembedding_amd.tiered import TieredLookupTable
    universe = _universe()
    pairs = []
    for j, (hc, cc) in enumerate(CAPS):
        hot = LookupTable(hc, dim, device=dev, max_batch=8192, default_value=HOT_DEFAULT[j], **kw)
        cold = LookupTable(cc, dim, device=dev, max_batch=8192, default_value=COLD_DEFAULT[j], value_memory=_lib.MEM_HOST_PINNED, **kw)
        if j != EMPTY_MEMBER:
            mask = ~hot_mask if (j == 1 and hot_mask.any() and not hot_mask.all()) else hot_mask
            _fill(hot, universe[mask], int(np.ceil(0.86 * hot.capacity)), 80 + 2 * j, dim, 3 + j, dev, tombstones=40 if j == 0 else 0)
            _fill(cold, universe[~mask], int(np.ceil(0.86 * cold.capacity)), 81 + 2 * j, dim, 3 + j, dev, tombstones=200 if j == 0 else 0)
        pairs.append(TieredLookupTable(hot, cold))
    return pairs


def _setup(dim, dev):
    """per dim, built once and only read afterwards: per placement the three pairs and their TieredTableGroup, and per batch, per placement, the rows
    and found mask of pair.find per member (fp32, on the device), computed once"""
    if dim in _SETUPS:
        return _SETUPS[dim]
    from meepoembedding_amd import TieredTableGroup
    batches = {name: (_T(k, dev), _T(o, dev), k, o) for name, (k, o) in _batches().items()}
    groups, want = {}, {}
    for pname, mask in _hot_masks(_batches()).items():
        pairs = _make_pairs(dim, dev, mask)
        groups[pname] = (TieredTableGroup(pairs), pairs)
        for bname, (keys, _, _, off) in batches.items():
            want[pname, bname] = [pair.find(keys[int(off[j]):int(off[j + 1])]) for j, pair in enumerate(pairs)]
    _SETUPS[dim] = (groups, batches, want)
    return _SETUPS[dim]


def _guarded(shape, dtype, dev, fill):
    """a buffer with one guard row (or 64 guard bytes) behind it -> (the view to hand in, the guard)"""
    rows = shape[0] + (1 if len(shape) == 2 else 64)
    buf = torch.full((rows, *shape[1:]), fill, dtype=dtype, device=dev)
    return buf[:shape[0]], buf[shape[0]:]


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("with_found", [True, False])
@pytest.mark.parametrize("out_dtype", [torch.float32, BF16])
@pytest.mark.parametrize("dim", [64, 128, 100])
def test_group_find_is_the_pairs_find_bit_for_bit(dev, dim, out_dtype, with_found):
    from meepoembedding_amd import _lib
    L = _lib.lib()
    groups, batches, want = _setup(dim, dev)
    dt = _lib.DTYPE_BF16 if out_dtype == BF16 else _lib.DTYPE_F32
    for bname, (keys, off, hkeys, hoff) in batches.items():
        n = keys.numel()
        # what TableGroup.find leaves of sentinel-filled buffers outside the segments: the same bytes (none written)
        flat_out, _ = _guarded((n, dim), out_dtype, dev, -7.0)
        flat_found, _ = _guarded((n,), torch.uint8, dev, 7)
        groups["all_hot"][0].hot_group.find(keys, off, out=flat_out, found=flat_found, out_dtype=out_dtype)
        outside = np.r_[0:HEAD, int(hoff[-1]):n]
        for pname, (group, pairs) in groups.items():
            out, og = _guarded((n, dim), out_dtype, dev, -7.0)
            found, fg = _guarded((n,), torch.uint8, dev, 7)
            if with_found:
                group.find(keys, off, out=out, found=found, out_dtype=out_dtype)
            else:
                _lib.check(L.mee_group_find_tiered(group.hot_group._h, group.cold_group._h, keys.data_ptr(), off.data_ptr(), n, out.data_ptr(), dt, None, 0, None))
            torch.cuda.synchronize(dev)
            exp_out = torch.full((n, dim), -7.0, dtype=out_dtype, device=dev)
            exp_found = torch.full((n,), 7, dtype=torch.uint8, device=dev)
            for j, (po, pf) in enumerate(want[pname, bname]):
                s, e = int(hoff[j]), int(hoff[j + 1])
                exp_out[s:e] = po.to(out_dtype)      # (bf16: the pair's fp32 rows rounded once)
                if with_found:
                    exp_found[s:e] = pf
            bad = (_bits(out) != _bits(exp_out)).any(dim=1).nonzero().view(-1).tolist()
            assert not bad, f"{pname} {bname}: rows {bad[:8]} differ from the pairs' (segments at {hoff.tolist()})"
            assert torch.equal(found, exp_found), (pname, bname)
            assert torch.equal(_bits(out[outside]), _bits(flat_out[outside])) and torch.equal(found[outside], flat_found[outside])
            assert bool((og == -7.0).all()) and bool((fg == 7).all()), "bytes behind out / found were written"
    # n == 0 succeeds and writes nothing; offsets that hold no position
    group = groups["half"][0]
    keys, off = batches["A"][0], batches["A"][1]
    out, found = group.find(keys[:0], torch.zeros(N_MEMBERS + 1, dtype=torch.int64, device=dev), out_dtype=out_dtype)
    assert out.shape == (0, dim) and found.numel() == 0
    out = torch.full((keys.numel(), dim), -7.0, dtype=out_dtype, device=dev)
    group.find(keys, torch.full((N_MEMBERS + 1,), 5, dtype=torch.int64, device=dev), out=out, out_dtype=out_dtype)
    assert bool((out == -7.0).all())


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
        pairs.append(TieredLookupTable(hot, cold, hot_key_limit=3000, sample_every=2))
    return pairs


def _hit_sets(pairs):
    """per pair and tier, the keys with at least 1 .. 6 hits"""
    return [[np.sort(_np(t.hits_scan(k, 0xFFFFFFFF, 4096))) for k in range(1, 7)] for p in pairs for t in (p.hot, p.cold)]


@pytest.mark.gpu
def test_group_find_counts_hits_like_the_pairs(dev):
    """track_hits pairs, sample_every = 2: a fixed sequence of calls leaves every member's hot and cold counters as the pairs' own calls leave them"""
    from meepoembedding_amd import TieredTableGroup
    a, b = _policy_pairs(dev), _policy_pairs(dev)
    group = TieredTableGroup(a, sample_every=2)
    assert group.policy
    keys, off = _batches()["A"]
    keys = keys.copy()
    keys[off[1] + 1] = keys[off[1] + 3] = keys[off[1]]     # a key three times in one segment: counted three times per call
    dk, do = _T(keys, dev), _T(off, dev)
    for call in ("find", "find", "find_or_insert", "find", "find"):
        out, found = getattr(group, call)(dk, do)
        for j, pair in enumerate(b):
            s, e = int(off[j]), int(off[j + 1])
            po, pf = getattr(pair, call)(dk[s:e])
            assert torch.equal(out[s:e], po) and torch.equal(found[s:e], pf), (call, j)
    got, want = _hit_sets(a), _hit_sets(b)
    for t, (g, w) in enumerate(zip(got, want)):
        for k, (x, y) in enumerate(zip(g, w)):
            assert np.array_equal(x, y), f"tier {t}: the keys with at least {k + 1} hits differ"
    assert got[0][0].size and got[1][0].size and got[2][0].size and got[3][0].size, "both tiers of members 0 and 1 were counted"
    assert got[1][4].size and not got[1][5].size, "cold hits: once per call, five calls"
    assert int(keys[off[1]]) in got[2][5].tolist() + got[3][5].tolist(), "three occurrences: at least six hits even in the sampled tier"


def _train_pairs(dev, dim, opt, limits=None):
    """three pairs for creation and training: member 0 has room in its hot tier, member 1's hot tier is at its limit (new keys go cold), member 2
    starts empty with room (or with `limits[2]`).  The universe's first half is hot, the second cold."""
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
        limit = (limits or {}).get(j, 200 if j == 1 else 10 * hot.capacity)
        pair = TieredLookupTable(hot, cold, hot_key_limit=limit)
        pair._hot_keys_ub = hot.size()      # (the tiers were filled directly: the pair's bound on its hot keys starts at what is there)
        pairs.append(pair)
    return pairs


def _assert_same_tiers(a, b, what):
    """every tier of every pair: the key-sorted export with the state planes, bit for bit"""
    for j, (pa, pb) in enumerate(zip(a, b)):
        for tier in ("hot", "cold"):
            got, exp = _sorted(getattr(pa, tier).export(with_state=True)), _sorted(getattr(pb, tier).export(with_state=True))
            assert np.array_equal(got[0], exp[0]), (what, j, tier, got[0].size, exp[0].size)
            for x, y in zip(got[1:], exp[1:]):
                assert (x is None and y is None) or np.array_equal(x.view(np.uint32), y.view(np.uint32)), (what, j, tier)


def _creation_batch(stream):
    """-> (keys, offsets, new keys per member): segments of 10, 12 and 80 positions.  Members 0 and 1: stored keys of both tiers, new keys, two of
    them repeated, RECLAIMED and EMPTY; member 2 (empty in both tiers): 76 new keys, two of them repeated, RECLAIMED and EMPTY."""
    universe = _universe()
    new = synth.keys_np(stream, 0, 100)
    s0 = np.concatenate([universe[10:12], universe[210:212], new[0:2], new[0:2], [RECLAIMED_KEY, EMPTY_KEY]])
    s1 = np.concatenate([universe[20:23], universe[220:223], new[2:4], [RECLAIMED_KEY], new[2:4], [EMPTY_KEY]])
    s2 = np.concatenate([new[4:42], [RECLAIMED_KEY, EMPTY_KEY], new[42:80], new[4:6]])
    keys = np.concatenate([new[90:90 + HEAD], s0, s1, s2, new[95:95 + TAIL]])     # (the head and the tail hold new keys: they must not be created)
    return keys, _offsets([s0.size, s1.size, s2.size]), [new[0:2], new[2:4], new[4:80]], new[90:100]


@pytest.mark.gpu
@pytest.mark.parametrize("out_dtype", [torch.float32, BF16])
def test_group_find_or_insert_creates_like_the_pairs(dev, out_dtype):
    """rows, the found mask and every tier's export equal the pairs' after the same two calls.  Member 2's hot_key_limit of 120 holds for the first
    call (107 positions in the batch, 80 in its slice) and for neither side in the second (76 keys stored: 76 + 107 and 76 + 80 are past it)."""
    from meepoembedding_amd import OPT_ADAM, STATUS_RESERVED_KEY, TieredTableGroup
    dim = 64
    a, b = _train_pairs(dev, dim, OPT_ADAM, {2: 120}), _train_pairs(dev, dim, OPT_ADAM, {2: 120})
    group = TieredTableGroup(a, max_apply_batch=4096)
    for call, want_tier in ((1, ("hot", "cold", "hot")), (2, ("hot", "cold", "cold"))):
        keys, off, new, outside = _creation_batch(72 + call)
        n = keys.size
        assert n == 107
        dk = _T(keys, dev)
        out, og = _guarded((n, dim), out_dtype, dev, -7.0)
        found, fg = _guarded((n,), torch.uint8, dev, 7)
        group.find_or_insert(dk, _T(off, dev), out=out, found=found, out_dtype=out_dtype)
        for j, pair in enumerate(b):
            s, e = int(off[j]), int(off[j + 1])
            po, pf = pair.find_or_insert(dk[s:e])
            assert torch.equal(_bits(out[s:e]), _bits(po.to(out_dtype))), (call, j)     # created rows included; bf16: the returned copy is rounded
            assert torch.equal(found[s:e], pf), (call, j)                               # "present before the call"
        assert bool((og == -7.0).all()) and bool((fg == 7).all())
        assert bool((out[:HEAD] == -7.0).all() and (out[int(off[-1]):] == -7.0).all() and (found[:HEAD] == 7).all() and (found[int(off[-1]):] == 7).all())
        f = _np(found)
        s0, s1, s2 = (int(x) for x in off[:3])
        assert f[s0:s0 + 4].all() and not f[s0 + 4:s0 + 10].any() and f[s1:s1 + 6].all() and not f[s1 + 6:s1 + 12].any() and not f[s2:s2 + 80].any()
        assert torch.equal(_bits(out[s0 + 4:s0 + 6]), _bits(out[s0 + 6:s0 + 8])), "a repeated new key: the same initial row at every occurrence"
        assert torch.equal(_bits(out[s1 + 6:s1 + 8]), _bits(out[s1 + 9:s1 + 11])) and torch.equal(_bits(out[s2:s2 + 2]), _bits(out[s2 + 78:s2 + 80]))
        assert not torch.equal(_bits(out[s0 + 4]), _bits(torch.full((dim,), HOT_DEFAULT[0], dtype=out_dtype, device=dev))), "an initial row, not the default"
        for j, pair in enumerate(a):      # exactly one tier, the one the rule picks; nothing of the head and the tail
            dn = _T(new[j], dev)
            in_hot, in_cold = pair.hot.find(dn)[1], pair.cold.find(dn)[1]
            assert bool(in_hot.all() and not in_cold.any()) if want_tier[j] == "hot" else bool(in_cold.all() and not in_hot.any()), (call, j)
            assert not pair.hot.find(_T(outside, dev))[1].any() and not pair.cold.find(_T(outside, dev))[1].any()
        _assert_same_tiers(a, b, f"call {call}")      # hashed initial rows (fp32 also for a bf16 out), initial optimizer state, nothing else touched
        # the tombstone value in the batch: RESERVED_KEY on the status word of the table that was asked to create, and on no other
        for j, pair in enumerate(a):
            asked, other = (pair.hot, pair.cold) if want_tier[j] == "hot" else (pair.cold, pair.hot)
            assert asked.status() == STATUS_RESERVED_KEY and other.status() == 0, (call, j)
            asked.clear_status()
    # a third call over the second batch creates nothing and finds everything but the reserved keys
    out, found = group.find_or_insert(dk, _T(off, dev), out_dtype=out_dtype)
    f = _np(found)
    reserved = (keys == RECLAIMED_KEY) | (keys == EMPTY_KEY)
    assert f[HEAD:int(off[-1])][~reserved[HEAD:int(off[-1])]].all() and not f[reserved].any()
    for pair in b:
        pair.hot.clear_status(); pair.cold.clear_status()
    for j, pair in enumerate(b):
        pair.find_or_insert(dk[int(off[j]):int(off[j + 1])])
    _assert_same_tiers(a, b, "third call")


@pytest.mark.gpu
def test_group_find_or_insert_flags_a_full_hot_table(dev):
    """a hot table too small for its new keys: TABLE_FULL on that table's status word and nowhere else"""
    from meepoembedding_amd import OPT_NONE, STATUS_TABLE_FULL, LookupTable, TieredTableGroup, _lib
    from meepoembedding_amd.tiered import TieredLookupTable
    dim = 64
    pairs = []
    for j, hc in enumerate([2000, 48, 2000]):
        hot = LookupTable(hc, dim, device=dev, optimizer=OPT_NONE, max_batch=4096)
        cold = LookupTable(2000, dim, device=dev, optimizer=OPT_NONE, max_batch=4096, value_memory=_lib.MEM_HOST_PINNED)
        pairs.append(TieredLookupTable(hot, cold, hot_key_limit=1 << 20))
    group = TieredTableGroup(pairs)
    new = synth.keys_np(75, 0, 3 * 600)
    off = torch.tensor([0, 600, 1200, 1800], dtype=torch.int64, device=dev)
    _, found = group.find_or_insert(_T(new, dev), off)
    assert not found.any()
    status = [(p.hot.status(), p.cold.status()) for p in pairs]
    assert status == [(0, 0), (STATUS_TABLE_FULL, 0), (0, 0)], status
    assert pairs[0].hot.size() == 600 and pairs[2].hot.size() == 600 and 0 < pairs[1].hot.size() < 600 and all(p.cold.size() == 0 for p in pairs)


@pytest.mark.gpu
@pytest.mark.parametrize("optimizer", ["adagrad", "adam"])
def test_group_steps_are_the_pairs_steps(dev, optimizer):
    """apply_adagrad / apply_adam over the jagged batch against the pairs' steps on independent copies, exactly summable gradients: every tier's
    key-sorted export with the state planes is bit-identical, with duplicates and keys of both tiers in a segment"""
    from meepoembedding_amd import OPT_ADAGRAD, OPT_ADAM, TieredTableGroup
    dim = 64
    opt = OPT_ADAGRAD if optimizer == "adagrad" else OPT_ADAM
    a, b = _train_pairs(dev, dim, opt), _train_pairs(dev, dim, opt)
    group = TieredTableGroup(a, max_apply_batch=4096)
    universe = _universe()
    rng = np.random.default_rng(17)
    off = _offsets([37, 70, 5])
    n = int(off[-1]) + TAIL
    for step in (1, 2, 3):
        keys = universe[rng.integers(0, N_KEYS, n)]          # duplicates, keys of both tiers (the first 200 are hot)
        keys[off[1] + 2] = keys[off[1] + 40] = keys[off[1]]
        keys[off[0] + 3], keys[off[1] + 5], keys[off[1] + 6] = ABSENT_KEY, EMPTY_KEY, ABSENT_KEY
        grads = exact_grads_np(rng, n, dim)
        dk, dg = _T(keys, dev), _T(grads, dev)
        if optimizer == "adagrad":
            group.apply_adagrad(dk, _T(off, dev), dg, 0.05)
        else:
            group.apply_adam(dk, _T(off, dev), dg, 0.01, step=step)
        for j, pair in enumerate(b):
            s, e = int(off[j]), int(off[j + 1])
            if optimizer == "adagrad":
                pair.apply_adagrad(dk[s:e], dg[s:e], 0.05)
            else:
                pair.apply_adam(dk[s:e], dg[s:e], 0.01, step=step)
    _assert_same_tiers(a, b, optimizer)
    assert all(t.status() == 0 for p in a + b for t in (p.hot, p.cold))
    moved = _sorted(a[0].cold.export(with_state=True))[1]
    assert not np.array_equal(moved, synth.rows_np(np.sort(universe[200:]), dim, 3)), "the cold rows were trained"


@pytest.mark.gpu
@pytest.mark.parametrize("optimizer", ["adagrad", "adam"])
def test_collection_layer_trains_the_group_like_the_pairs(dev, optimizer):
    """DynamicEmbeddingCollection over the tiered group, bf16 rows, three steps against the per-pair loop (find_or_insert, then the pair's step on the
    same exactly summable gradients — every element a 6-bit integer times a power of two, so the bf16 grad the layer widens is the fp32 one): every
    tier ends bit-identical.  eval creates nothing."""
    from meepoembedding_amd import OPT_ADAGRAD, OPT_ADAM, TieredTableGroup
    from meepoembedding_amd.nn import DynamicEmbeddingCollection
    dim = 64
    opt = OPT_ADAGRAD if optimizer == "adagrad" else OPT_ADAM
    a, b = _train_pairs(dev, dim, opt), _train_pairs(dev, dim, opt)
    group = TieredTableGroup(a, max_apply_batch=4096)
    layer = DynamicEmbeddingCollection(group, optimizer=optimizer, lr=0.05, out_dtype=BF16).to(dev).train()
    universe = _universe()
    rng = np.random.default_rng(11)
    off = (np.concatenate([[0], np.cumsum([37, 70, 5])])).astype(np.int64)
    n = int(off[-1])
    for step in (1, 2, 3):
        keys = universe[rng.integers(0, N_KEYS, n)]
        keys[off[1] + 2] = keys[off[1]]
        fresh = synth.keys_np(90 + step, 0, 2)      # ids no table has seen, twice each, in every member's segment
        for j in range(N_MEMBERS):
            s = int(off[j])
            keys[s:s + 2] = fresh
            keys[s + 3:s + 5] = fresh
        head = exact_grads_np(rng, n, dim)
        dk, dh = _T(keys, dev), _T(head, dev)
        out = layer(dk, _T(off, dev))
        assert out.dtype == BF16 and out.shape == (n, dim)
        (out.float() * dh).sum().backward()
        for j, pair in enumerate(b):
            s, e = int(off[j]), int(off[j + 1])
            po, _ = pair.find_or_insert(dk[s:e])
            assert torch.equal(_bits(out[s:e].detach()), _bits(po.to(BF16))), (step, j)
            if optimizer == "adagrad":
                pair.apply_adagrad(dk[s:e], dh[s:e], 0.05, 1e-10)
            else:
                pair.apply_adam(dk[s:e], dh[s:e], 0.05, 0.9, 0.999, 1e-8, step)
    _assert_same_tiers(a, b, optimizer)
    assert all(t.status() == 0 for p in a + b for t in (p.hot, p.cold))
    assert a[1].cold.size() == N_KEYS - 200 + 6 and a[1].hot.size() == 200, "member 1's hot tier is at its limit: its 6 new ids went cold"
    assert a[0].hot.size() == 200 + 6 and 6 < a[2].hot.size() <= 9 and a[2].cold.size() == 0      # (member 2 also creates the stored key of its segment)
    sizes = [p.size() for p in a]
    unseen = _T(np.tile(synth.keys_np(99, 0, 5), N_MEMBERS), dev)
    out = layer.eval()(unseen, torch.arange(0, 16, 5, dtype=torch.int64, device=dev))
    assert [p.size() for p in a] == sizes, "eval creates nothing"
    assert torch.equal(out[5:10], torch.full((5, dim), HOT_DEFAULT[1], device=dev).to(BF16))


@pytest.mark.gpu
def test_group_find_follows_reserve_on_members(dev):
    from meepoembedding_amd import TieredTableGroup
    groups, batches, want = _setup(64, dev)
    keys, off = batches["A"][0], batches["A"][1]
    pairs = _make_pairs(64, dev, _hot_masks(_batches())["half"])
    group = TieredTableGroup(pairs)
    before, fb = group.find(keys, off)
    assert torch.equal(before[HEAD:-TAIL], groups["half"][0].find(keys, off)[0][HEAD:-TAIL])
    pairs[0].hot.reserve(4 * pairs[0].hot.capacity)       # the planes of one hot and of one cold member move
    pairs[1].cold.reserve(3 * pairs[1].cold.capacity)
    after, fa = group.find(keys, off)
    assert torch.equal(before[HEAD:-TAIL], after[HEAD:-TAIL]) and torch.equal(fb[HEAD:-TAIL], fa[HEAD:-TAIL])
    for j, (po, pf) in enumerate(want["half", "A"]):
        s, e = int(batches["A"][3][j]), int(batches["A"][3][j + 1])
        assert torch.equal(after[s:e], po) and torch.equal(fa[s:e], pf), j


@pytest.mark.gpu
def test_group_find_is_graph_capturable(dev):
    """one launch, no allocation, no host synchronisation: captured on one stream, replayed twice after the keys changed in place"""
    from meepoembedding_amd import TieredTableGroup
    pairs = _make_pairs(64, dev, _hot_masks(_batches())["alternating"])
    group = TieredTableGroup(pairs)
    hkeys, hoff = _batches()["A"]
    keys, off = _T(hkeys, dev), _T(hoff, dev)
    n = keys.numel()
    out = torch.zeros(n, 64, device=dev)
    found = torch.zeros(n, dtype=torch.uint8, device=dev)
    group.find(keys, off)     # (warm: nothing is loaded or uploaded inside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        group.find(keys, off, out=out, found=found)
    s, e = int(hoff[0]), int(hoff[-1])
    universe = _universe()
    for shift in (0, 150, 280):
        keys[s:e] = _T(universe[shift:shift + e - s], dev)      # in place: the graph reads the same buffer
        eager, ef = group.find(keys, off)
        out.zero_(); found.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[s:e], eager[s:e]) and torch.equal(found[s:e], ef[s:e]) and bool(found[s:e].any()), shift
        assert not out[:s].any() and not out[e:].any()


@pytest.mark.gpu
def test_group_find_entry_points_refuse(dev):
    """every refusal of the two entry points: the named code, a message, and no byte written to out, found or a table"""
    from meepoembedding_amd import LookupTable, TableGroup, _lib
    L = _lib.lib()
    mk = lambda dim=16, **kw: LookupTable(256, dim, device=dev, max_batch=256, **kw)  # noqa: E731
    h0, h1, c0, c1, counted = mk(), mk(), mk(), mk(), mk(track_hits=True)
    hot, cold = TableGroup([h0, h1]), TableGroup([c0, c1])
    wide, three = TableGroup([mk(32), mk(32)]), TableGroup([mk(), mk(), mk()])
    shares = TableGroup([c0, h1])                         # member 1 is the hot group's member 1
    some_counted = TableGroup([counted, mk()])            # one member without counters
    bf16_rows = TableGroup([mk(64, value_dtype=BF16), mk(64, value_dtype=BF16)])
    f64 = TableGroup([mk(64), mk(64)])
    keys = torch.arange(8, dtype=torch.int64, device=dev)
    off = torch.tensor([0, 5, 8], dtype=torch.int64, device=dev)     # member 0: keys [0, 5), member 1: keys [5, 8)
    out = torch.full((8, 64), -7.0, device=dev)
    found = torch.full((8,), 7, dtype=torch.uint8, device=dev)
    NULL = object()

    def find(h, c, out_dtype=_lib.DTYPE_F32, flags=0, out_ptr=None, keys_ptr=None, off_ptr=None):
        return L.mee_group_find_tiered(h, c, None if keys_ptr is NULL else keys.data_ptr(), None if off_ptr is NULL else off.data_ptr(), 8,
                                       None if out_ptr is NULL else (out.data_ptr() if out_ptr is None else out_ptr), out_dtype, found.data_ptr(), flags, None)

    def foi(h, c, out_dtype=_lib.DTYPE_F32, flags=0, out_ptr=None, keys_ptr=None, off_ptr=None, found_ptr=None):
        return L.mee_group_find_or_insert_tiered(h, c, None if keys_ptr is NULL else keys.data_ptr(), None if off_ptr is NULL else off.data_ptr(), 8,
                                                 None if out_ptr is NULL else (out.data_ptr() if out_ptr is None else out_ptr), out_dtype,
                                                 None if found_ptr is NULL else found.data_ptr(), None, flags, None)

    def refused(rc, code=_lib.ERR_INVALID_ARG, name=None):
        msg = L.mee_last_error().decode()
        assert rc == code and msg and (name is None or msg.startswith(name + ":")), (rc, msg)

    for fn, name in ((find, "mee_group_find_tiered"), (foi, "mee_group_find_or_insert_tiered")):
        refused(fn(None, cold._h), name=name); refused(fn(hot._h, None), name=name)                     # a null group
        refused(fn(hot._h, cold._h, keys_ptr=NULL), name=name); refused(fn(hot._h, cold._h, off_ptr=NULL), name=name)     # null keys, offsets, out
        refused(fn(hot._h, cold._h, out_ptr=NULL), name=name)
        refused(fn(hot._h, hot._h), name=name)                                                          # hot is cold
        refused(fn(hot._h, wide._h), name=name); refused(fn(hot._h, three._h), name=name)               # another dim, another number of tables
        refused(fn(hot._h, shares._h), name=name)                                                       # one table as both tiers of a member
        refused(fn(hot._h, cold._h, flags=4), name=name)                                                # unknown flag bits
        refused(fn(hot._h, cold._h, out_dtype=2), name=name)                                            # an unknown out_dtype
        refused(fn(hot._h, cold._h, out_dtype=_lib.DTYPE_BF16, out_ptr=out.data_ptr() + 4), name=name)  # a bf16 row group is one 8-byte store
        refused(fn(hot._h, some_counted._h, flags=_lib.TIER_COUNT_COLD), name=name)                     # a count flag, a member without counters
        refused(fn(some_counted._h, cold._h, flags=_lib.TIER_COUNT_HOT), name=name)
        refused(fn(bf16_rows._h, f64._h), _lib.ERR_UNSUPPORTED, name); refused(fn(f64._h, bf16_rows._h), _lib.ERR_UNSUPPORTED, name)
    refused(foi(hot._h, cold._h, found_ptr=NULL), name="mee_group_find_or_insert_tiered")               # its found mask is required
    torch.cuda.synchronize(dev)
    assert bool((out == -7.0).all()) and bool((found == 7).all()) and all(t.size() == 0 for t in (h0, h1, c0, c1, counted))
    # what is not refused: n == 0 (nothing written, null buffers), and the plain calls
    assert L.mee_group_find_tiered(hot._h, cold._h, None, off.data_ptr(), 0, None, _lib.DTYPE_F32, None, 0, None) == _lib.OK
    assert L.mee_group_find_or_insert_tiered(hot._h, cold._h, None, off.data_ptr(), 0, None, _lib.DTYPE_F32, None, None, 0, None) == _lib.OK
    torch.cuda.synchronize(dev)
    assert bool((out == -7.0).all()) and bool((found == 7).all()) and all(t.size() == 0 for t in (h0, h1, c0, c1))
    assert find(hot._h, cold._h) == _lib.OK
    torch.cuda.synchronize(dev)
    assert bool((out.view(-1)[:8 * 16] == 0).all()) and bool((out.view(-1)[8 * 16:] == -7.0).all()) and not found.any()    # eight rows of dim 16, default rows of 0
    assert foi(hot._h, cold._h) == _lib.OK
    torch.cuda.synchronize(dev)
    assert h0.size() == 5 and h1.size() == 3 and c0.size() == c1.size() == 0 and not found.any()      # null d_to_cold: all hot; found = present before
