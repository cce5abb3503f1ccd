"""The padded sequence lookup over a hot/cold pair and over a group of pairs on the GPU (SPEC.md §3 "Tiering"): mee_find_padded_tiered,
mee_group_find_padded_tiered, TieredLookupTable.find_padded, TieredTableGroup.find_padded and nn.DynamicEmbeddingSequence over them.
The expectation is tests/_padded_cases.py's loop over an oracle table holding the UNION of the pair's two tiers with the hot default; the
outputs are pre-filled with that file's sentinels.  The tables are small (at most 4096 slots per tier), the cold tier's rows in pinned host memory.

One batch of ten bags reaches every path at L = 3: lengths 0, 1, 2 (< L), 3 (= L), 4 (= L + 1) and 200 — the truncated share of the long bag is
(200 - 3) / 3 = 66 positions per slot, five 16-lane rounds."""
import numpy as np
import pytest
import torch

import oracle
from _apply_cases import T, exact_grads_np
from _padded_cases import EMPTY, FOUND_SENTINEL, I64_SENTINEL, RECLAIMED, U32_SENTINEL, bf16_bits, expected_padded, spans
from meepoembedding_amd import OPT_ADAGRAD, OPT_ADAM, LookupTable, MeepoError, TableGroup, _lib, synth
from meepoembedding_amd.tiered import TieredLookupTable, TieredTableGroup
from test_find_padded import Outs, check_all

BF16 = torch.bfloat16
L = 3
LENS = [0, 1, 2, 3, 4, 200, 1, 0, 3, 5]
HOT_DEFAULT, COLD_DEFAULT = 0.5, 0.25
N_KEYS = 300
UNIVERSE = synth.keys_np(61, 0, N_KEYS)
NEVER = synth.keys_np(991, 0, 8)          # keys no table of this file holds
CAP = 1024


def _offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def _batch(lens, seed=5):
    """keys for bags of the given lengths: drawn from a pool of 60 universe keys (so keys repeat inside and across bags), absent keys, EMPTY and
    the tombstone value.  Planted on top, wherever the batch has such a bag: the head of the long bag (kept under keep='first') and its tail (kept
    under 'last') get a stored key, an absent or a reserved one, the bag of one key and the first bag of three (kept whole) a hot, a cold and an
    absent key, the first bag of five a key that 'split_absent' stores nowhere in its middle (kept under both), and the long bag's cut-off part
    two stored keys that occur nowhere else"""
    rng = np.random.default_rng(seed)
    pool = np.concatenate([UNIVERSE[:40], UNIVERSE[260:280], NEVER, [EMPTY, RECLAIMED]]).astype(np.int64)
    lens = list(lens)
    keys = pool[rng.integers(0, pool.size, int(np.sum(lens)))]
    off = _offsets(lens)
    big = int(np.argmax(lens))
    if lens[big] >= 20:
        b, e = int(off[big]), int(off[big + 1])
        keys[b:b + 3] = [UNIVERSE[0], EMPTY, UNIVERSE[0]]              # a key twice inside the kept head
        keys[e - 3:e] = [RECLAIMED, NEVER[0], UNIVERSE[1]]
        keys[b + 10:b + 14] = [UNIVERSE[299], UNIVERSE[298], EMPTY, UNIVERSE[299]]   # only ever cut off (the pool does not draw 298 / 299)
    if 1 in lens:
        keys[off[lens.index(1)]] = UNIVERSE[0]                          # ... and once more in another bag
    if 3 in lens:
        b = int(off[lens.index(3)])
        keys[b:b + 3] = [UNIVERSE[3], UNIVERSE[2], NEVER[1]]            # cold and hot under the split placements, and a key in no table
    if 5 in lens:
        keys[off[lens.index(5)] + 2] = UNIVERSE[270]
    return keys, off


def _placements():
    """name -> (hot keys, cold keys, union keys) of the same key set"""
    idx = np.arange(N_KEYS)
    even = idx % 2 == 0
    stored = ~((idx >= 268) & (idx < 280))          # 'split_absent': twelve keys of the pool are in neither tier
    return {"all_hot": (UNIVERSE, UNIVERSE[:0], UNIVERSE), "all_cold": (UNIVERSE[:0], UNIVERSE, UNIVERSE),
            "split": (UNIVERSE[even], UNIVERSE[~even], UNIVERSE),
            "split_absent": (UNIVERSE[even & stored], UNIVERSE[~even & stored], UNIVERSE[stored])}


def _fill(t, keys, dim, dev, seed=3):
    if keys.size:
        t.insert(T(keys, dev), T(synth.rows_np(keys, dim, seed), dev))


def _make_pair(dim, dev, hot_keys, cold_keys, seed=3, hot_default=HOT_DEFAULT, **kw):
    hot = LookupTable(CAP, dim, device=dev, max_batch=4096, default_value=hot_default, **kw)
    cold = LookupTable(CAP, dim, device=dev, max_batch=4096, default_value=COLD_DEFAULT, value_memory=_lib.MEM_HOST_PINNED, **kw)
    _fill(hot, hot_keys, dim, dev, seed)
    _fill(cold, cold_keys, dim, dev, seed)
    return TieredLookupTable(hot, cold, hot_key_limit=CAP)


def _make_oracle(dim, keys, seed=3, default=HOT_DEFAULT, **kw):
    o = oracle.OracleTable(CAP, dim, default_value=default, **kw)
    o.insert(keys, synth.rows_np(keys, dim, seed))
    return o


_SETUPS = {}


def _setup(dim, dev):
    """per dim, built once and only read afterwards: placement -> (pair, oracle of the union, native table of the union)"""
    if dim not in _SETUPS:
        made = {}
        for name, (hk, ck, uk) in _placements().items():
            union = LookupTable(CAP, dim, device=dev, max_batch=4096, default_value=HOT_DEFAULT)
            _fill(union, uk, dim, dev)
            made[name] = (_make_pair(dim, dev, hk, ck), _make_oracle(dim, uk), union)
        _SETUPS[dim] = made
    return _SETUPS[dim]


def raw(hot, cold, keys_t, off_t, bags_arg, max_len, keep, o, dev, group=False, count=0, **nulls):
    """the C entry point on pre-filled outputs -> its return code.  nulls: names of arguments to pass as NULL"""
    fn = _lib.lib().mee_group_find_padded_tiered if group else _lib.lib().mee_find_padded_tiered
    p = lambda name, t: None if nulls.get(name) else t.data_ptr()  # noqa: E731
    return fn(hot, cold, p("keys", keys_t), keys_t.numel(), p("off", off_t), bags_arg, max_len, {"first": 0, "last": 1}.get(keep, keep), count, p("out", o.out),
              nulls.get("dtype", _lib.DTYPE_BF16 if o.out.dtype == BF16 else _lib.DTYPE_F32), p("found", o.found), p("lengths", o.lengths),
              p("step_keys", o.step_keys), p("grad_index", o.grad_index), torch.cuda.current_stream(dev).cuda_stream)


def _as_outs(res, dev):
    """the 5-tuple of a Python find_padded(with_step=True) as an Outs, for check_all"""
    o = Outs.__new__(Outs)
    o.out, o.found, o.lengths, o.step_keys, o.grad_index = res
    return o


# ---- 1. the pair, bit for bit ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("keep", ["first", "last"])
@pytest.mark.parametrize("dim", [8, 64, 128, 100, 1024])
def test_pair_is_the_union_bit_for_bit(dev, dim, keep):
    """dims 8 / 100 / 1024 take the run-time row shape; four placements of one key set; against the oracle of the union and against ONE native
    table of the union through find_padded"""
    keys, off = _batch(LENS)
    kd, od = T(keys, dev), T(off, dev)
    for name, (pair, o, union) in _setup(dim, dev).items():
        exp = expected_padded(lambda b: o.find, keys, off, L, keep, dim)
        outs = Outs(dev, keys.size, len(LENS), L, dim)
        assert raw(pair.hot._h, pair.cold._h, kd, od, len(LENS), L, keep, outs, dev) == 0
        check_all(outs, exp, f"dim {dim} {name} {keep}")
        uo, uf, ul, uk, ug = union.find_padded(kd, od, L, keep=keep, with_step=True)
        po, pf, pl, pk, pg = pair.find_padded(kd, od, L, keep=keep, with_step=True)       # the Python form: the same launch
        assert torch.equal(po.view(torch.int32), uo.view(torch.int32)) and torch.equal(po.view(torch.int32), outs.out.view(torch.int32)), name
        assert torch.equal(pf, uf) and torch.equal(pl, ul) and torch.equal(pk, uk) and torch.equal(pg, ug), name
        if name == "split_absent":
            assert (exp[1] == 0).sum() > (expected_padded(lambda b: _setup(dim, dev)["split"][1].find, keys, off, L, keep, dim)[1] == 0).sum()
    assert pair.hot.status() == pair.cold.status() == 0
    first_absent = int(np.nonzero((exp[3] != EMPTY) & (exp[3] != I64_SENTINEL) & (exp[1] == 0) & (exp[3] != RECLAIMED))[0][0])
    assert (outs.out.view(-1, dim)[int(exp[4][first_absent])] == HOT_DEFAULT).all()      # a miss reads the HOT default, never the cold one


# ---- 2. bf16 out ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("keep", ["first", "last"])
@pytest.mark.parametrize("dim", [64, 100])
def test_bf16_out_is_the_fp32_expectation_rounded_once(dev, dim, keep):
    keys, off = _batch(LENS)
    pair, o, _ = _setup(dim, dev)["split_absent"]
    outs = Outs(dev, keys.size, len(LENS), L, dim, dtype=BF16)
    assert raw(pair.hot._h, pair.cold._h, T(keys, dev), T(off, dev), len(LENS), L, keep, outs, dev) == 0
    exp = expected_padded(lambda b: o.find, keys, off, L, keep, dim)
    check_all(outs, exp, f"bf16 out dim {dim} {keep}", bf16=True)
    pad = np.arange(L)[None, :] >= exp[2][:, None]
    assert pad.any() and not outs.out.cpu().view(torch.int16).numpy()[pad].any()   # padding is the bit pattern 0x0000


# ---- 3. caller offsets ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("keep", ["first", "last"])
def test_caller_offsets(dev, keep):
    """an offset past n, a decreasing pair, a first offset above 0: the clamped spans are used and positions in no bag keep the sentinels"""
    dim = 64
    pair, o, _ = _setup(dim, dev)["split"]
    keys, _ = _batch([60])
    n = keys.size
    cases = {"lead and trail": [3, 10, 10, 31, 52], "past n": [0, 20, 45, 1 << 40, 1 << 41], "decreasing": [2, 19, 40, 25]}
    for name, off in cases.items():
        off = np.array(off, np.int64)
        outs = Outs(dev, n, off.size - 1, L, dim)
        assert raw(pair.hot._h, pair.cold._h, T(keys, dev), T(off, dev), off.size - 1, L, keep, outs, dev) == 0
        exp = expected_padded(lambda b: o.find, keys, off, L, keep, dim)
        covered = np.zeros(n, bool)
        for begin, end in spans(off, n):
            covered[begin:end] = True
        assert (~covered).any() or name == "past n"
        assert (exp[1][~covered] == FOUND_SENTINEL).all() and (exp[3][~covered] == I64_SENTINEL).all() and (exp[4][~covered] == U32_SENTINEL).all()
        check_all(outs, exp, f"offsets '{name}' {keep}")


# ---- 4. hit counters -----------------------------------------------------------------------------------------------------------------------------
def _kept_counts(exp, of_keys):
    """how many KEPT positions hold each of `of_keys`"""
    kept = exp[3][(exp[3] != EMPTY) & (exp[3] != I64_SENTINEL)]
    return np.array([(kept == k).sum() for k in of_keys], np.int64)


def _hits(t, keys, dev):
    return t.hits_of(T(keys, dev)).cpu().numpy().astype(np.int64) if keys.size else np.zeros(0, np.int64)


@pytest.mark.gpu
def test_hit_counters(dev):
    dim = 64
    hk, ck, _ = _placements()["split"]
    pair = _make_pair(dim, dev, hk, ck, track_hits=True)
    o = _make_oracle(dim, UNIVERSE)
    keys, off = _batch(LENS)
    kd, od = T(keys, dev), T(off, dev)
    cut_only = UNIVERSE[[298, 299]]
    for keep in ("first", "last"):
        exp = expected_padded(lambda b: o.find, keys, off, L, keep, dim)
        want_hot, want_cold = _kept_counts(exp, hk), _kept_counts(exp, ck)
        assert want_hot.max() >= (3 if keep == "first" else 1) and want_cold.sum() > 0     # (a hot key kept three times: twice in one bag, once in another)
        assert not _kept_counts(exp, cut_only).any() and np.isin(cut_only, keys).all()     # keys that occur only in cut-off positions
        for count in (0, _lib.TIER_COUNT_COLD, _lib.TIER_COUNT_HOT, _lib.TIER_COUNT_COLD | _lib.TIER_COUNT_HOT):
            before = _hits(pair.hot, hk, dev), _hits(pair.cold, ck, dev)
            outs = Outs(dev, keys.size, len(LENS), L, dim)
            assert raw(pair.hot._h, pair.cold._h, kd, od, len(LENS), L, keep, outs, dev, count=count) == 0
            check_all(outs, exp, f"count_flags {count} {keep}")
            dh, dc = _hits(pair.hot, hk, dev) - before[0], _hits(pair.cold, ck, dev) - before[1]
            assert np.array_equal(dh, want_hot if count & _lib.TIER_COUNT_HOT else 0 * want_hot), f"hot counters, count_flags {count} {keep}"
            assert np.array_equal(dc, want_cold if count & _lib.TIER_COUNT_COLD else 0 * want_cold), f"cold counters, count_flags {count} {keep}"
    # the Python path: cold hits always, hot hits on every sample_every-th call
    policy = TieredLookupTable(pair.hot, pair.cold, hot_key_limit=CAP, sample_every=2)
    assert policy.policy
    exp = expected_padded(lambda b: o.find, keys, off, L, "first", dim)
    want_hot, want_cold = _kept_counts(exp, hk), _kept_counts(exp, ck)
    for call, hot_counted in ((1, False), (2, True)):
        before = _hits(pair.hot, hk, dev), _hits(pair.cold, ck, dev)
        policy.find_padded(kd, od, L)
        assert np.array_equal(_hits(pair.cold, ck, dev) - before[1], want_cold), call
        assert np.array_equal(_hits(pair.hot, hk, dev) - before[0], want_hot if hot_counted else 0 * want_hot), call


# ---- 5. a group of three pairs -------------------------------------------------------------------------------------------------------------------
GROUP_DEFAULTS = [0.5, 0.625, 0.75]
GROUP_LENS = {1: [200, 2, 4], 5: [0, 1, 2, 3, 4,   200, 1, 0, 3, 5,   4, 4, 2, 0, 7]}


def _make_group(dim, dev, **kw):
    """member 0 all hot, member 1 all cold, member 2 split; own rows and hot default per member -> (group, pairs, oracles of the unions)"""
    P = _placements()
    pairs = [_make_pair(dim, dev, *P[name][:2], seed=3 + j, hot_default=GROUP_DEFAULTS[j], **kw) for j, name in enumerate(("all_hot", "all_cold", "split"))]
    oracles = [_make_oracle(dim, UNIVERSE, seed=3 + j, default=GROUP_DEFAULTS[j]) for j in range(3)]
    return TieredTableGroup(pairs, sample_every=1 << 30), pairs, oracles


@pytest.mark.gpu
@pytest.mark.parametrize("bpt", [1, 5])
@pytest.mark.parametrize("dim", [64, 24])
def test_group_of_pairs(dev, dim, bpt):
    """bags_per_table 1 and 5 at L = 3: a wave's four tiles serve different pairs.  Each member's block is its own pair's find_padded on its bags;
    both count bits feed every member's counters; after mee_reserve on a cold member the next call gives the same block"""
    grp, pairs, oracles = _make_group(dim, dev, track_hits=True)
    lens = GROUP_LENS[bpt]
    keys, off = _batch(lens, seed=7)
    kd, od = T(keys, dev), T(off, dev)
    both = _lib.TIER_COUNT_COLD | _lib.TIER_COUNT_HOT
    P = _placements()
    hot_keys, cold_keys = [P[name][0] for name in ("all_hot", "all_cold", "split")], [P[name][1] for name in ("all_hot", "all_cold", "split")]
    for keep in ("first", "last"):
        exp = expected_padded(lambda b: oracles[b // bpt].find, keys, off, L, keep, dim)
        before = [(_hits(p.hot, hk, dev), _hits(p.cold, ck, dev)) for p, hk, ck in zip(pairs, hot_keys, cold_keys)]
        outs = Outs(dev, keys.size, 3 * bpt, L, dim)
        assert raw(grp.hot_group._h, grp.cold_group._h, kd, od, bpt, L, keep, outs, dev, group=True, count=both) == 0
        check_all(outs, exp, f"group dim {dim} bpt {bpt} {keep}")
        for j, (p, hk, ck) in enumerate(zip(pairs, hot_keys, cold_keys)):   # every kept position counted once, in its member's tier
            member_kept = exp[3][int(off[j * bpt]):int(off[(j + 1) * bpt])]
            member_kept = member_kept[member_kept != EMPTY]
            want = lambda ks: np.array([(member_kept == k).sum() for k in ks], np.int64)  # noqa: E731
            assert np.array_equal(_hits(p.hot, hk, dev) - before[j][0], want(hk)) and np.array_equal(_hits(p.cold, ck, dev) - before[j][1], want(ck)), f"member {j}"
        b16 = Outs(dev, keys.size, 3 * bpt, L, dim, dtype=BF16)
        assert raw(grp.hot_group._h, grp.cold_group._h, kd, od, bpt, L, keep, b16, dev, group=True) == 0
        check_all(b16, exp, f"group bf16 dim {dim} bpt {bpt} {keep}", bf16=True)
        for j, (p, hk, ck) in enumerate(zip(pairs, hot_keys, cold_keys)):
            s, e = int(off[j * bpt]), int(off[(j + 1) * bpt])
            own_off = T(off[j * bpt:(j + 1) * bpt + 1] - s, dev)
            for dtype, whole in ((torch.float32, outs), (BF16, b16)):   # the pair's own lookup on its bags: every output, bit for bit
                oo, of, ol, ok, og = p.find_padded(kd[s:e].contiguous(), own_off, L, keep=keep, out_dtype=dtype, with_step=True)
                bits = torch.int16 if dtype == BF16 else torch.int32
                assert torch.equal(oo.view(bits), whole.out[j * bpt:(j + 1) * bpt].view(bits)), f"member {j} {dtype}"
                assert torch.equal(of, whole.found[s:e]) and torch.equal(ol, whole.lengths[j * bpt:(j + 1) * bpt]) and torch.equal(ok, whole.step_keys[s:e])
                kept = torch.zeros(e - s, dtype=torch.bool, device=dev)     # the member's kept positions: its bags' first / last `lengths`
                for b in range(j * bpt, (j + 1) * bpt):
                    n_kept = int(ol[b - j * bpt])
                    first_kept = int(off[b]) - s if keep == "first" else int(off[b + 1]) - s - n_kept
                    kept[first_kept:first_kept + n_kept] = True
                assert torch.equal(og[kept] + j * bpt * L, whole.grad_index[s:e][kept]) and not whole.grad_index[s:e][~kept].any() and not og[~kept].any()
    # the Python form, then the same block after a cold member's planes moved
    first = grp.find_padded(kd, od, L, keep="last", with_step=True)
    check_all(_as_outs(first, dev), expected_padded(lambda b: oracles[b // bpt].find, keys, off, L, "last", dim), "TieredTableGroup.find_padded")
    pairs[2].cold.reserve(2 * CAP)
    again = Outs(dev, keys.size, 3 * bpt, L, dim)
    assert raw(grp.hot_group._h, grp.cold_group._h, kd, od, bpt, L, "last", again, dev, group=True) == 0
    assert torch.equal(again.out.view(torch.int32), first[0].view(torch.int32)) and torch.equal(again.found, first[1]) and torch.equal(again.grad_index, first[4])
    assert all(p.hot.status() == p.cold.status() == 0 for p in pairs)
    grp.close()


# ---- 6. refusals: before anything is launched or written -----------------------------------------------------------------------------------------
def _refused(rc, outs, name, what, code=None):
    assert rc == (_lib.ERR_INVALID_ARG if code is None else code), f"{what}: rc {rc}"
    assert name in _lib.lib().mee_last_error().decode(), f"{what}: the message names the operator"
    assert outs.untouched(), f"{what}: outputs written"


@pytest.mark.gpu
def test_pair_refusals_and_zero_bags(dev):
    dim, name = 64, "mee_find_padded_tiered"
    plain_h, plain_c = LookupTable(256, dim, device=dev, max_batch=256), LookupTable(256, dim, device=dev, max_batch=256)
    hits_h, hits_c = LookupTable(256, dim, device=dev, max_batch=256, track_hits=True), LookupTable(256, dim, device=dev, max_batch=256, track_hits=True)
    wide = LookupTable(256, 128, device=dev, max_batch=256)
    narrow = LookupTable(256, dim, device=dev, max_batch=256, value_dtype=BF16)
    int8 = LookupTable(256, dim, device=dev, max_batch=256, int8_rows=True)
    keys, off = _batch([3, 9])
    kd, od = T(keys, dev), T(off, dev)

    def call(hot=plain_h._h, cold=plain_c._h, max_len=4, keep="first", bags=2, count=0, outs=None, **nulls):
        outs = outs or Outs(dev, keys.size, 2, 4, dim)
        return raw(hot, cold, kd, od, bags, max_len, keep, outs, dev, count=count, **nulls), outs

    assert call()[0] == 0 and call(hits_h._h, hits_c._h, count=3)[0] == 0
    for what, (rc, oo) in {
        "null hot": call(hot=None), "null cold": call(cold=None), "hot == cold": call(cold=plain_h._h), "tiers of different dims": call(cold=wide._h),
        "unknown keep bit": call(keep=2), "unknown keep bit 2": call(keep=0x80000001), "unknown count bit": call(count=4), "unknown count bit 2": call(count=0x80000000),
        "COUNT_COLD without the cold tier's counters": call(hits_h._h, plain_c._h, count=_lib.TIER_COUNT_COLD),
        "COUNT_HOT without the hot tier's counters": call(plain_h._h, hits_c._h, count=_lib.TIER_COUNT_HOT),
        "max_len 0": call(max_len=0), "more than 2^56 slots": call(max_len=1 << 56, grad_index=True), "2^31 slots with grad_index": call(max_len=1 << 30),
        "unknown out_dtype": call(dtype=7), "int8 out_dtype": call(dtype=_lib.DTYPE_INT8),
        "null bag_offsets": call(off=True), "null out": call(out=True), "null keys": call(keys=True),
    }.items():
        _refused(rc, oo, name, what)
    for what, (rc, oo) in {"bf16-row hot": call(hot=narrow._h), "bf16-row cold": call(cold=narrow._h), "int8-row cold": call(cold=int8._h)}.items():
        _refused(rc, oo, name, what, _lib.ERR_UNSUPPORTED)
    whole = torch.full((2 * 4 * dim + 4,), float("nan"), dtype=BF16, device=dev)
    rc, oo = call(outs=Outs(dev, keys.size, 2, 4, dim, out=whole[1:1 + 2 * 4 * dim]))   # a bf16 out that is 2 bytes off an 8-byte boundary
    assert whole.data_ptr() % 8 == 0 and bool(torch.isnan(whole.float()).all())
    _refused(rc, oo, name, "misaligned bf16 out")
    for kw in (dict(bags=0), dict(bags=0, off=True, out=True)):
        rc, oo = call(**kw)
        assert rc == 0 and oo.untouched(), "zero bags succeed and write nothing"
    empty = Outs(dev, 0, 2, 4, dim)   # n == 0: two empty bags, a block of zeros
    assert raw(plain_h._h, plain_c._h, kd[:0], T(np.zeros(3, np.int64), dev), 2, 4, "first", empty, dev, keys=True) == 0
    assert not empty.out.view(torch.int32).any() and empty.lengths.tolist() == [0, 0]
    pair = TieredLookupTable(plain_h, plain_c)
    with pytest.raises(ValueError):
        pair.find_padded(kd, od, 4, keep="middle")
    with pytest.raises(ValueError):
        pair.find_padded(kd, od, 0)
    with pytest.raises(MeepoError):
        pair.find_padded(kd, od.cpu(), 4)


@pytest.mark.gpu
def test_group_refusals_and_zero_bags(dev):
    dim, name = 64, "mee_group_find_padded_tiered"
    mk = lambda d=dim, **kw: LookupTable(256, d, device=dev, max_batch=256, **kw)  # noqa: E731
    hot, cold, other = TableGroup([mk(), mk()]), TableGroup([mk(), mk()]), TableGroup([mk(), mk(), mk()])
    shared = mk()
    share_a, share_b = TableGroup([mk(), shared]), TableGroup([mk(), shared])
    wide = TableGroup([mk(128), mk(128)])
    hits, hits_cold = TableGroup([mk(track_hits=True), mk(track_hits=True)]), TableGroup([mk(track_hits=True), mk(track_hits=True)])
    half_hits = TableGroup([mk(track_hits=True), mk()])
    narrow = TableGroup([mk(value_dtype=BF16), mk(value_dtype=BF16)])
    keys, off = _batch([3, 9])
    kd, od = T(keys, dev), T(off, dev)

    def call(h=hot._h, c=cold._h, max_len=4, keep="first", bpt=1, count=0, outs=None, **nulls):
        outs = outs or Outs(dev, keys.size, 2, 4, dim)
        return raw(h, c, kd, od, bpt, max_len, keep, outs, dev, group=True, count=count, **nulls), outs

    assert call()[0] == 0 and call(hits._h, hits_cold._h, count=3)[0] == 0
    for what, (rc, oo) in {
        "null hot": call(h=None), "null cold": call(c=None), "hot == cold": call(c=hot._h), "a table that is member 1 of both": call(share_a._h, share_b._h),
        "groups of different dims": call(c=wide._h), "groups of different sizes": call(c=other._h),
        "unknown keep bit": call(keep=2), "unknown count bit": call(count=4),
        "COUNT_COLD with a cold member without counters": call(hits._h, half_hits._h, count=_lib.TIER_COUNT_COLD),
        "COUNT_HOT with a hot member without counters": call(half_hits._h, hits._h, count=_lib.TIER_COUNT_HOT),
        "COUNT_HOT without any counters": call(count=_lib.TIER_COUNT_HOT),
        "max_len 0": call(max_len=0), "more than 2^56 slots": call(max_len=1 << 56, grad_index=True), "2^31 slots with grad_index": call(max_len=1 << 30),
        "unknown out_dtype": call(dtype=7), "null bag_offsets": call(off=True), "null out": call(out=True), "null keys": call(keys=True),
    }.items():
        _refused(rc, oo, name, what)
    for what, (rc, oo) in {"bf16-row hot group": call(h=narrow._h), "bf16-row cold group": call(c=narrow._h)}.items():
        _refused(rc, oo, name, what, _lib.ERR_UNSUPPORTED)
    whole = torch.full((2 * 4 * dim + 4,), float("nan"), dtype=BF16, device=dev)
    rc, oo = call(outs=Outs(dev, keys.size, 2, 4, dim, out=whole[1:1 + 2 * 4 * dim]))
    _refused(rc, oo, name, "misaligned bf16 out")
    for kw in (dict(bpt=0), dict(bpt=0, off=True, out=True)):
        rc, oo = call(**kw)
        assert rc == 0 and oo.untouched(), "zero bags succeed and write nothing"
    empty = Outs(dev, 0, 2, 4, dim)
    assert raw(hot._h, cold._h, kd[:0], T(np.zeros(3, np.int64), dev), 1, 4, "first", empty, dev, group=True, keys=True) == 0
    assert not empty.out.view(torch.int32).any() and empty.lengths.tolist() == [0, 0]


# ---- 7. training through the layer ---------------------------------------------------------------------------------------------------------------
def _sorted_export(t):
    e = [x.cpu().numpy() for x in t.export(with_state=True) if x is not None]
    order = np.argsort(e[0])
    return [x[order] for x in e]


def _assert_same_tables(a, b, what):
    ea, eb = _sorted_export(a), _sorted_export(b)
    assert len(ea) == len(eb) and len(ea) >= 3, what
    for name, x, y in zip(("keys", "values", "state1", "state2"), ea, eb):
        assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y), f"{what}: {name}"


@pytest.mark.gpu
@pytest.mark.parametrize("keep", ["first", "last"])
@pytest.mark.parametrize("optimizer", ["adagrad", "adam"])
def test_layer_trains_the_pair_like_one_table(dev, optimizer, keep):
    """DynamicEmbeddingSequence over the pair and over ONE native table of the union, two steps on exactly summable gradients (tests/test_apply_exact.py:
    small integers times a power of two, so the kept keys' duplicates add up the same in any order): the blocks and the exported rows and state are
    equal bit for bit; keys that were only ever cut off are untrained"""
    from meepoembedding_amd.nn import DynamicEmbeddingSequence
    dim = 64
    opt = OPT_ADAGRAD if optimizer == "adagrad" else OPT_ADAM
    hk, ck, uk = _placements()["split_absent"]
    kw = dict(optimizer=opt, initial_accumulator=0.1)
    pair = _make_pair(dim, dev, hk, ck, **kw)
    one = LookupTable(CAP, dim, device=dev, max_batch=4096, default_value=HOT_DEFAULT, **kw)
    _fill(one, uk, dim, dev)
    keys, off = _batch(LENS)
    kd, od = T(keys, dev), T(off, dev)
    layers = [DynamicEmbeddingSequence(t, L, keep=keep, optimizer=optimizer, lr=0.05, create_missing=False).to(dev).train() for t in (pair, one)]
    assert all(layer.traits.native_padded for layer in layers)
    rng = np.random.default_rng(3)
    for step in (1, 2):
        w = T(exact_grads_np(rng, len(LENS) * L, dim).reshape(len(LENS), L, dim), dev)
        blocks = []
        for layer in layers:
            padded, lengths = layer(kd, od)
            (padded * w).sum().backward()
            blocks.append((padded.detach(), lengths))
        assert torch.equal(blocks[0][0].view(torch.int32), blocks[1][0].view(torch.int32)) and torch.equal(blocks[0][1], blocks[1][1]), step
    _assert_same_tables(pair, one, f"{optimizer} {keep}")
    assert pair.size() == uk.size and pair.hot.size() == hk.size       # nothing created, nothing moved
    cut_only = UNIVERSE[[298, 299]]
    rows, found = pair.find(T(cut_only, dev))
    assert found.all() and np.array_equal(rows.cpu().numpy(), synth.rows_np(cut_only, dim, 3))   # cut-off ids took no step


@pytest.mark.gpu
@pytest.mark.parametrize("keep,create", [("last", False), ("first", True)], ids=["last", "first-create_missing"])
@pytest.mark.parametrize("optimizer", ["adagrad", "adam"])
def test_layer_trains_the_group_of_pairs_like_a_table_group(dev, optimizer, keep, create):
    """create: create_missing=True, as examples/tiered_collection.py runs the layer — the grouped find_or_insert over both tiers in front of the one
    padded launch; the unseen ids (cut-off ones too) enter each pair's hot tier with the hashed initial row the union's table gives them"""
    from meepoembedding_amd.nn import DynamicEmbeddingSequence
    dim, bpt = 64, 5
    opt = OPT_ADAGRAD if optimizer == "adagrad" else OPT_ADAM
    P = _placements()
    kws = [dict(optimizer=opt, initial_accumulator=0.1, initializer=oracle.INIT_UNIFORM, init_scale=0.05, init_seed=9 + j) for j in range(3)]
    names = ("all_hot", "all_cold", "split_absent")
    pairs = [_make_pair(dim, dev, *P[name][:2], seed=3 + j, hot_default=GROUP_DEFAULTS[j], **kws[j]) for j, name in enumerate(names)]
    unions = []
    for j, name in enumerate(names):
        u = LookupTable(CAP, dim, device=dev, max_batch=4096, default_value=GROUP_DEFAULTS[j], **kws[j])
        _fill(u, P[name][2], dim, dev, seed=3 + j)
        unions.append(u)
    sizes = [u.size() for u in unions]
    tiered, plain = TieredTableGroup(pairs, max_apply_batch=4096), TableGroup(unions, max_apply_batch=4096)
    lens = GROUP_LENS[bpt]
    keys, off = _batch(lens, seed=7)
    kd, od = T(keys, dev), T(off, dev)
    layers = [DynamicEmbeddingSequence(g, L, keep=keep, optimizer=optimizer, lr=0.05, create_missing=create).to(dev).train() for g in (tiered, plain)]
    assert all(layer.traits.native_padded and layer.traits.grouped for layer in layers)
    rng = np.random.default_rng(4)
    for step in (1, 2):
        w = T(exact_grads_np(rng, len(lens) * L, dim).reshape(len(lens), L, dim), dev)
        blocks = []
        for layer in layers:
            padded, lengths = layer(kd, od)
            (padded * w).sum().backward()
            blocks.append((padded.detach(), lengths))
        assert torch.equal(blocks[0][0].view(torch.int32), blocks[1][0].view(torch.int32)) and torch.equal(blocks[0][1], blocks[1][1]), step
    for j, (p, u) in enumerate(zip(pairs, unions)):
        _assert_same_tables(p, u, f"member {j} {optimizer}")
        assert (u.size() > sizes[j]) == create and p.size() == u.size(), f"member {j}: unseen ids enter with create_missing only"
    tiered.close(); plain.close()


# ---- 8. capture ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_capture_and_replay_on_one_stream(dev):
    """a linear capture of the pair form and of the group form (no member reserved since the group's last call); the replay writes the eager block"""
    dim = 64
    pair, o, _ = _setup(dim, dev)["split_absent"]
    grp, pairs, oracles = _make_group(dim, dev)
    keys, off = _batch(GROUP_LENS[5], seed=7)
    kd, od = T(keys, dev), T(off, dev)
    n_bags = len(GROUP_LENS[5])
    cases = {"pair": (lambda oo: raw(pair.hot._h, pair.cold._h, kd, od, n_bags, L, "last", oo, dev), lambda b: o.find),
             "group": (lambda oo: raw(grp.hot_group._h, grp.cold_group._h, kd, od, 5, L, "last", oo, dev, group=True), lambda b: oracles[b // 5].find)}
    for name, (launch, find_of_bag) in cases.items():
        eager, outs = Outs(dev, keys.size, n_bags, L, dim), Outs(dev, keys.size, n_bags, L, dim)
        assert launch(eager) == 0     # (the group: this call uploads the members' descriptors)
        torch.cuda.synchronize(dev)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            rc = launch(outs)
        assert rc == 0
        exp = expected_padded(find_of_bag, keys, off, L, "last", dim)
        for _ in range(2):
            outs.out.fill_(float("nan")); outs.found.fill_(FOUND_SENTINEL); outs.step_keys.fill_(I64_SENTINEL)
            outs.lengths.fill_(I64_SENTINEL); outs.grad_index.fill_(U32_SENTINEL)
            assert outs.untouched()
            graph.replay()
            torch.cuda.synchronize(dev)
            check_all(outs, exp, f"replay {name}")
            assert torch.equal(outs.out.view(torch.int32), eager.out.view(torch.int32))
    grp.close()
