"""GPU: max pooling (SPEC.md §3 find_pooled_max / pooled_max_backward and their group forms) against the NumPy restatement of the scan
(tests/_pooled_max_ref.py, which tests/test_pooled_max_symbols.py pins to torch's embedding_bag(mode="max")) — bit for bit, argmax exactly — and the
layer against torch.nn.EmbeddingBag(mode="max") + torch.optim.Adagrad on the CPU."""
import functools

import numpy as np
import pytest
import torch

from _pooled_max_ref import NO_ARGMAX, bits, clamp_offsets, pooled_max, pooled_max_backward
from meepoembedding_amd import _lib, synth
from test_weighted_bags import SHAPES, wave_per_bag

pytestmark = pytest.mark.gpu

DIMS = [4, 24, 64, 128, 100, 1024]
DEFAULT = 9.0        # above every stored finite value, so an absent key's default row wins columns
N_STORED = 600
SENTINEL = 777.0


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def u32(t):
    return t.cpu().view(torch.int32).numpy().view(np.uint32)


# The crafted keys: every special value sits in the columns j = case (mod 4) of EVERY element group, so the groups behind the first (and the column chunks
# of the run-time row shape) meet them too.  Ordinary rows lie in [-3, 3].
TIE_A, TIE_B, NEGZ, POSZ, NANK, INFK, LOW = range(7)


def _special_rows(dim):
    r = np.random.default_rng(3).uniform(-3, 3, size=(7, dim)).astype(np.float32)
    r[TIE_A, 0::4] = r[TIE_B, 0::4] = 5.0
    r[TIE_A, 1::4] = r[TIE_B, 1::4] = r[TIE_A, 2::4] = r[TIE_B, 2::4] = -7.0   # (they share a bag with the signed zeros: below them there)
    r[NEGZ, 1::4], r[POSZ, 1::4] = -0.0, 0.0
    r[NEGZ, 2::4], r[POSZ, 2::4] = 0.0, -0.0
    r[NANK, 3::4] = np.nan
    r[INFK, 0::4], r[INFK, 1::4] = np.inf, -np.inf
    r[LOW] = -7.0
    return r


@functools.lru_cache(maxsize=None)
def _table(dev, dim):
    """one table per dim for the whole module: N_STORED ordinary keys, the seven crafted ones, a default row above them all"""
    from meepoembedding_amd import LookupTable
    rng = np.random.default_rng(100 + dim)
    t = LookupTable(4096, dim, device=dev, max_batch=1 << 12, default_value=DEFAULT)
    stored = synth.keys_np(41, 0, N_STORED + 7)
    rows = rng.uniform(-3, 3, size=(N_STORED + 7, dim)).astype(np.float32)
    rows[N_STORED:] = _special_rows(dim)
    t.insert(T(stored, dev), T(rows, dev))
    absent = synth.keys_np(42, 0, 16)
    assert not np.intersect1d(stored, absent).size
    return t, stored[:N_STORED], stored[N_STORED:], absent


def _batch(dev, dim, lens, seed):
    """keys and offsets for the bag lengths `lens`, with every case planted twice: in bags a tile walks alone (partners next to each other) and in bags
    the four tiles walk together (partners in different tiles and rounds) -> (keys, off, planted: tag -> positions by name)"""
    t, stored, special, absent = _table(dev, dim)
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    keys = stored[rng.integers(0, N_STORED, size=int(off[-1]))].copy()   # with replacement: duplicate ids inside bags
    shared_walk = wave_per_bag(lens)   # a wave per bag: every bag is walked by the four tiles together
    used, planted = set(), {}

    def bag_with(min_len, long):
        for b in np.argsort(lens, kind="stable"):   # the shortest bag that fits
            n = lens[b]
            if b not in used and n >= min_len and (shared_walk or (n >= 16) == long):
                used.add(b)
                return int(b), int(off[b]), int(n)
        raise AssertionError(f"no unused {'long' if long else 'short'} bag of {min_len}+ keys: the cases cannot be planted")

    for tag, long, far in (("near", False, 1), ("far", True, 6)):
        p = {}
        # ties and signed zeros: everything else in the bag lies below them
        b, s, n = bag_with(far + 3 + (far == 1), long)
        keys[s:s + n] = special[LOW]
        p.update(bag_a=b, tie1=s + 1, tie2=s + 1 + far, negz=s + 2 + (far == 1), posz=s + 2 + (far == 1) + far)
        keys[p["tie1"]], keys[p["tie2"]], keys[p["negz"]], keys[p["posz"]] = special[TIE_A], special[TIE_B], special[NEGZ], special[POSZ]
        # NaN at the first position, +inf / -inf at the last
        b, s, n = bag_with(2, long)
        p.update(bag_b=b, nan_first=s, inf=s + n - 1)
        keys[s], keys[s + n - 1] = special[NANK], special[INFK]
        # NaN at a later position; an absent key, EMPTY and RECLAIMED: the default row; an id twice in one bag
        b, s, n = bag_with(far + 5, long)
        p.update(bag_c=b, absent=s + 1, empty=s + 2, reclaimed=s + 3, nan_later=s + 3 + far, twin=(s, s + n - 1))
        keys[s + 1], keys[s + 2], keys[s + 3], keys[s + 3 + far], keys[s + n - 1] = absent[0], _lib.EMPTY_KEY, _lib.RECLAIMED_KEY, special[NANK], keys[s]
        planted[tag] = p
    return keys, off, planted


def _assert_cases_present(planted, keys, rows, out, arg, lens):
    """the reference's own results show that the inputs contain every case (a missing one fails, it does not skip)"""
    assert (np.asarray(lens) == 0).any() and (arg[np.asarray(lens) == 0] == NO_ARGMAX).all() and (bits(out)[np.asarray(lens) == 0] == 0).all()   # empty bags
    for p in (planted["near"], planted["far"]):
        b = p["bag_a"]
        assert rows[p["tie1"], 0] == rows[p["tie2"], 0] == out[b, 0] == 5.0 and arg[b, 0] == p["tie1"]            # the first of equal values
        assert bits(out)[b, 1] == 0x80000000 and arg[b, 1] == p["negz"] and bits(rows)[p["posz"], 1] == 0         # +0.0 behind -0.0 does not replace it
        assert bits(out)[b, 2] == 0 and arg[b, 2] == p["negz"] and bits(rows)[p["posz"], 2] == 0x80000000         # nor -0.0 behind +0.0
        b = p["bag_b"]
        assert np.isnan(out[b, 3]) and arg[b, 3] == p["nan_first"]                                                  # a NaN at the first position stays
        assert out[b, 0] == np.inf and arg[b, 0] == p["inf"] and rows[p["inf"], 1] == -np.inf and arg[b, 1] != p["inf"]
        b = p["bag_c"]
        assert np.isnan(rows[p["nan_later"], 3]) and not np.isnan(out[b, 3]) and arg[b, 3] != p["nan_later"]       # a later one is never taken
        for q in ("absent", "empty", "reclaimed"):
            assert (rows[p[q]] == DEFAULT).all()
        assert (arg[b] == p["absent"]).all() and (out[b] == DEFAULT).all()                                          # the default row wins, its first position
        assert keys[p["twin"][0]] == keys[p["twin"][1]]


def _bf16_equal(got, ref):
    """a bf16 tensor against the fp32 reference rounded once: bit for bit, a NaN against any NaN"""
    g = got.cpu().view(torch.int16).numpy()
    w = torch.from_numpy(ref).to(torch.bfloat16).view(torch.int16).numpy()
    nan = np.isnan(ref)
    return got.dtype == torch.bfloat16 and np.array_equal(g[~nan], w[~nan]) and bool(torch.isnan(got.cpu().float())[torch.from_numpy(nan)].all())


@pytest.mark.parametrize("dim", DIMS)
def test_forward_bit_exact(dev, dim):
    t, _, _, _ = _table(dev, dim)
    for si, lens in enumerate(SHAPES):
        keys, off, planted = _batch(dev, dim, lens, 7 * dim + si)
        kt, ot = T(keys, dev), T(off, dev)
        rows_t, ef = t.find(kt)
        rows = rows_t.cpu().numpy()
        ref, rarg = pooled_max(rows, off)
        _assert_cases_present(planted, keys, rows, ref, rarg, lens)
        nb, n = lens.size, keys.size
        # sentinel-prefilled buffers with a guard row in front and behind: nothing outside the outputs is written
        obuf = torch.full((nb + 2, dim), SENTINEL, device=dev)
        abuf = torch.full((nb + 2, dim), 12345, dtype=torch.int32, device=dev)
        fbuf = torch.full((n + 2,), 99, dtype=torch.uint8, device=dev)
        out, found, arg = t.find_pooled_max(kt, ot, out=obuf[1:-1], found=fbuf[1:-1], argmax=abuf[1:-1])
        tag = f"dim {dim} shape {si} ({'a wave per bag' if wave_per_bag(lens) else 'four bags per wave'})"
        assert np.array_equal(bits(out.cpu().numpy()), bits(ref)), tag
        assert np.array_equal(u32(arg), rarg), tag
        assert torch.equal(found, ef), tag
        assert bool((obuf[[0, -1]] == SENTINEL).all()) and bool((abuf[[0, -1]] == 12345).all()) and fbuf[0] == 99 and fbuf[-1] == 99, tag
        # without argmax: the same rows
        out2, found2, none = t.find_pooled_max(kt, ot)
        assert none is None and torch.equal(out2.view(torch.int32), out.view(torch.int32)) and torch.equal(found2, ef), tag
        # find_pooled(mode="max") is the same call
        out3, found3 = t.find_pooled(kt, ot, "max")
        assert torch.equal(out3.view(torch.int32), out.view(torch.int32)) and torch.equal(found3, ef), tag
        # bf16 out: the fp32 maximum rounded once, argmax still decided on the fp32 values
        hb, fb, ab = t.find_pooled_max(kt, ot, out_dtype=torch.bfloat16, with_argmax=True)
        assert _bf16_equal(hb, ref), tag
        assert ab.dtype == torch.uint32 and np.array_equal(u32(ab), rarg) and torch.equal(fb, ef), tag
    assert t.status() == 0   # reserved keys in a lookup raise nothing


def test_offset_clamps_and_no_bags(dev):
    """Offsets past the key array are cut at its end, a decreasing pair is an empty bag (the clamps of find_pooled); zero bags write nothing."""
    t, stored, _, _ = _table(dev, 64)
    keys = stored[:100].copy()
    off = torch.tensor([0, 10, 10, 90, 1 << 40, 1 << 41, 3], dtype=torch.int64, device=dev)
    begin, end = clamp_offsets(off.cpu().numpy(), 100)
    assert begin.tolist() == [0, 10, 10, 90, 100, 3] and end.tolist() == [10, 10, 90, 100, 100, 3]
    rows = t.find(T(keys, dev))[0].cpu().numpy()
    ref, rarg = pooled_max(rows, off.cpu().numpy())
    out, _, arg = t.find_pooled_max(T(keys, dev), off, with_argmax=True)
    assert np.array_equal(bits(out.cpu().numpy()), bits(ref)) and np.array_equal(u32(arg), rarg)
    bg = np.random.default_rng(1).standard_normal((6, 64)).astype(np.float32)
    g = t.pooled_max_backward(off, arg, T(bg, dev), 100, grads=torch.full((100, 64), SENTINEL, device=dev))
    assert np.array_equal(bits(g.cpu().numpy()), bits(pooled_max_backward(off.cpu().numpy(), rarg, bg, np.full((100, 64), SENTINEL, np.float32))))
    none = torch.zeros(1, dtype=torch.int64, device=dev)
    o0 = torch.full((1, 64), SENTINEL, device=dev)
    out, _, arg = t.find_pooled_max(T(keys, dev), none, out=o0[:0], with_argmax=True)
    assert out.shape == (0, 64) and arg.shape == (0, 64) and bool((o0 == SENTINEL).all())
    g0 = torch.full((100, 64), SENTINEL, device=dev)
    t.pooled_max_backward(none, arg, torch.empty((0, 64), device=dev), 100, grads=g0)
    assert bool((g0 == SENTINEL).all())


@pytest.mark.parametrize("dim", DIMS)
def test_backward_bit_exact(dev, dim):
    """grads against the reference bit for bit (signs of zeros and a NaN gradient included); positions that no bag covers keep the sentinel"""
    t, _, _, _ = _table(dev, dim)
    for si, lens in enumerate(SHAPES):
        rng = np.random.default_rng(11 * dim + si)
        lead, trail = 3, 5
        off = (np.concatenate([[0], np.cumsum(lens)]) + lead).astype(np.int64)
        n = int(off[-1]) + trail
        rows = rng.uniform(-3, 3, size=(n, dim)).astype(np.float32)
        _, rarg = pooled_max(rows, off)                       # any valid argmax: the backward reads no row and no key
        bg = rng.standard_normal((lens.size, dim)).astype(np.float32)
        bg[:, 0] = -0.0
        bg[1, 1] = np.nan
        want = pooled_max_backward(off, rarg, bg, np.full((n, dim), SENTINEL, np.float32))
        assert (want[:lead] == SENTINEL).all() and (want[n - trail:] == SENTINEL).all() and (bits(want)[lead:n - trail, 0] == 0x80000000).any()
        g = t.pooled_max_backward(T(off, dev), T(rarg.view(np.int32), dev), T(bg, dev), n, grads=torch.full((n, dim), SENTINEL, device=dev))
        assert np.array_equal(bits(g.cpu().numpy()), bits(want)), f"dim {dim} shape {si}"


@pytest.mark.parametrize("dim", [64, 128, 24])
def test_group_equals_members(dev, dim):
    """the group is the member's operator on its bags: rows, found and argmax rebased by the member's first position; each member its own default row"""
    from meepoembedding_amd import LookupTable, TableGroup
    rng = np.random.default_rng(dim)
    members, stored = [], []
    for j in range(3):
        m = LookupTable(2048, dim, device=dev, max_batch=1 << 12, default_value=4.0 + j)
        u = synth.keys_np(50 + j, 0, 300)
        m.insert(T(u, dev), T(rng.uniform(-3, 3, size=(300, dim)).astype(np.float32), dev))
        members.append(m); stored.append(u)
    group = TableGroup(members)
    absent = synth.keys_np(60, 0, 8)
    for si, lens1 in enumerate((SHAPES[0][:20], SHAPES[1][:10])):   # four bags per wave (20 is no multiple of 4: a wave serves two members) | a wave per bag
        lens = np.concatenate([lens1, lens1[::-1], lens1])
        assert wave_per_bag(lens) == bool(si)
        bpt = lens1.size
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        keys = np.concatenate([stored[j][rng.integers(0, 300, size=int(off[(j + 1) * bpt] - off[j * bpt]))] for j in range(3)])
        keys[rng.integers(0, keys.size, size=40)] = absent[rng.integers(0, 8, size=40)]   # default rows: each member's own
        out, found, arg = group.find_pooled_max(T(keys, dev), T(off, dev), with_argmax=True)
        bg = rng.standard_normal((lens.size, dim)).astype(np.float32)
        grads = group.pooled_max_backward(T(off, dev), arg, T(bg, dev), keys.size)
        for j, m in enumerate(members):
            b0, b1 = j * bpt, (j + 1) * bpt
            k0, k1 = int(off[b0]), int(off[b1])
            mo, mf, ma = m.find_pooled_max(T(keys[k0:k1], dev), T(off[b0:b1 + 1] - k0, dev), with_argmax=True)
            assert torch.equal(out[b0:b1].view(torch.int32), mo.view(torch.int32)) and torch.equal(found[k0:k1], mf), (dim, si, j)
            ma = u32(ma)
            assert np.array_equal(u32(arg)[b0:b1], np.where(ma == NO_ARGMAX, NO_ARGMAX, ma + np.uint32(k0))), (dim, si, j)
            mg = m.pooled_max_backward(T(off[b0:b1 + 1] - k0, dev), T(ma.view(np.int32), dev), T(bg[b0:b1], dev), k1 - k0)
            assert torch.equal(grads[k0:k1].view(torch.int32), mg.view(torch.int32)), (dim, si, j)
        rows = group.find(T(keys, dev), T(off[::bpt].copy(), dev))[0].cpu().numpy()
        ref, rarg = pooled_max(rows, off)
        assert np.array_equal(bits(out.cpu().numpy()), bits(ref)) and np.array_equal(u32(arg), rarg)
        assert (ref == 4.0).any() and (ref == 5.0).any() and (ref == 6.0).any()        # every member's default row won somewhere
        out2, found2 = group.find_pooled(T(keys, dev), T(off, dev), "max", out_dtype=torch.bfloat16)
        assert _bf16_equal(out2, ref) and torch.equal(found2, found)


@functools.lru_cache(maxsize=None)
def _trained(dev, n_members):
    """Three training steps of DynamicEmbeddingBag(mode="max") over a table (1) or over a 3-member group, run once for the tests below, beside two CPU
    twins fed the same batches and bag gradients: torch.nn.EmbeddingBag(mode="max", sparse=False) + torch.optim.Adagrad, and the oracle's SPEC.md §4 step
    on the reference backward of the layer's own rows.  -> per member: the layer's forwards, torch's embedding_bag on the layer's rows at each step, torch's
    module's forwards, and the rows at the end (layer, torch, oracle, initial)."""
    import oracle
    from meepoembedding_amd import OPT_ADAGRAD, LookupTable, TableGroup
    from meepoembedding_amd.nn import DynamicEmbeddingBag
    # lr: torch's Adagrad and SPEC.md §4 round the update lr * g / (sqrt(acc) + eps) at different places (the spec's step ends in one fma), so two correct
    # steps differ by a few ulp of the UPDATE, whatever the size of the row element it lands on — and where update and element cancel, that is far more
    # than 1e-6 of what is left.  The bound's atol of 1e-9 covers it only while three steps' worth of such ulps stay below it: |update| <= lr (|g| /
    # sqrt(acc) < 1), ulp(1e-3) = 1.2e-10, three steps of two to three ulps = 1e-9 at most.  At lr = 0.05 (ulp 3.7e-9) the oracle's own step misses the
    # bound against torch by a factor of up to 3.9 on these batches.  A gradient routed to the wrong position still shows: it moves an element by ~lr / 2.
    dim, V, lr, acc0, bpt = (64, 120, 1e-3, 0.1, 24) if n_members == 1 else (24, 80, 1e-3, 0.1, 13)
    rng = np.random.default_rng(90 + n_members)
    lens1 = SHAPES[0][:bpt]
    W0 = [rng.standard_normal((V, dim)).astype(np.float32) for _ in range(n_members)]
    vocab = [synth.keys_np(70 + j, 0, V) for j in range(n_members)]
    tables, oracles = [], []
    for j in range(n_members):
        m = LookupTable(1024, dim, device=dev, optimizer=OPT_ADAGRAD, initial_accumulator=acc0, max_batch=1 << 12)
        m.insert(T(vocab[j], dev), T(W0[j], dev))
        tables.append(m)
        o = oracle.OracleTable(1024, dim, optimizer=oracle.OPT_ADAGRAD, initial_accumulator=acc0)
        o.insert(vocab[j], W0[j])
        oracles.append(o)
    target = tables[0] if n_members == 1 else TableGroup(tables, max_apply_batch=1 << 12)
    layer = DynamicEmbeddingBag(target, mode="max", optimizer="adagrad", lr=lr, eps=1e-10)
    bags = [torch.nn.EmbeddingBag(V, dim, mode="max", sparse=False, include_last_offset=True, _weight=torch.from_numpy(W0[j].copy())) for j in range(n_members)]
    opts = [torch.optim.Adagrad(b.parameters(), lr=lr, initial_accumulator_value=acc0, eps=1e-10) for b in bags]
    off1 = np.concatenate([[0], np.cumsum(lens1)]).astype(np.int64)
    ids = [rng.integers(0, V, size=int(off1[-1])) for _ in range(n_members)]
    keys = np.concatenate([vocab[j][ids[j]] for j in range(n_members)])
    off = np.concatenate([[0]] + [off1[1:] + j * off1[-1] for j in range(n_members)]).astype(np.int64)
    Gs = [[rng.standard_normal((bpt, dim)).astype(np.float32) for _ in range(n_members)] for _ in range(3)]
    kt, ot = T(keys, dev), T(off, dev)
    res = [dict(got=[], own=[], torch=[]) for _ in range(n_members)]
    for s in range(3):
        out = layer(kt, ot)
        got = out.detach().cpu().numpy()
        for j in range(n_members):
            mine = tables[j].find(T(vocab[j], dev))[0].cpu()
            tid, toff = torch.from_numpy(ids[j]), torch.from_numpy(off1)
            res[j]["got"].append(got[j * bpt:(j + 1) * bpt])
            res[j]["own"].append(torch.nn.functional.embedding_bag(tid, mine, toff, mode="max", include_last_offset=True).numpy())
            opts[j].zero_grad()
            o = bags[j](tid, toff)
            (o * torch.from_numpy(Gs[s][j])).sum().backward()
            opts[j].step()
            res[j]["torch"].append(o.detach().numpy())
            _, rarg = pooled_max(mine.numpy()[ids[j]], off1)   # the step by definition: apply_adagrad(keys, the backward's grads)
            oracles[j].apply_adagrad(vocab[j][ids[j]], pooled_max_backward(off1, rarg, Gs[s][j], np.zeros((ids[j].size, dim), np.float32)), lr, 1e-10)
        (out * T(np.concatenate(Gs[s]), dev)).sum().backward()
    for j in range(n_members):
        res[j].update(rows=tables[j].find(T(vocab[j], dev))[0].cpu().numpy(), torch_rows=bags[j].weight.detach().numpy().copy(),
                      oracle_rows=oracles[j].find(vocab[j])[0], initial=W0[j])
    return res


def _excess(got, want):
    """max |got - want| / (1e-9 + 1e-6 |want|): at most 1 inside SPEC.md §4's bound"""
    return float((np.abs(got - want) / (1e-9 + 1e-6 * np.abs(want))).max())


@pytest.mark.parametrize("n_members", [1, 3])
def test_three_training_steps_forward_and_step(dev, n_members):
    """The forward bit for bit — the first step's against torch's module, every step's against torch's embedding_bag(mode="max") on the layer's own rows
    (later steps start from rows that already differ in the last place from torch's trajectory) — and the rows after the three steps against the SPEC.md §4
    step of the oracle on pooled_max_backward's grads, within 1e-6 relative, atol 1e-9."""
    for j, r in enumerate(_trained(dev, n_members)):
        assert np.array_equal(bits(r["got"][0]), bits(r["torch"][0])), f"member {j}: first forward against torch's module"
        for s in range(3):
            assert np.array_equal(bits(r["got"][s]), bits(r["own"][s])), f"step {s} member {j}: forward against torch on the layer's rows"
            print(f"members {n_members} member {j} step {s}: forward against torch's own trajectory, excess {_excess(r['got'][s], r['torch'][s]):.3g}")
        assert np.abs(r["rows"] - r["initial"]).max() > 1e-3   # the steps moved rows by a thousand times the bound
        print(f"members {n_members} member {j}: rows against the oracle's step, excess {_excess(r['rows'], r['oracle_rows']):.3g}")
        np.testing.assert_allclose(r["rows"], r["oracle_rows"], rtol=1e-6, atol=1e-9)


@pytest.mark.parametrize("n_members", [1, 3])
def test_three_training_steps_rows_against_torch(dev, n_members):
    """The rows after three steps against torch.nn.EmbeddingBag(mode="max", sparse=False) + torch.optim.Adagrad on the CPU, within SPEC.md §4's 1e-6
    relative, atol 1e-9."""
    for j, r in enumerate(_trained(dev, n_members)):
        print(f"members {n_members} member {j}: rows against torch, excess {_excess(r['rows'], r['torch_rows']):.3g} "
              f"(the oracle's SPEC step against torch: {_excess(r['oracle_rows'], r['torch_rows']):.3g})")
    for j, r in enumerate(_trained(dev, n_members)):
        np.testing.assert_allclose(r["rows"], r["torch_rows"], rtol=1e-6, atol=1e-9)


def test_layer_creates_missing_and_writes_bf16(dev):
    from meepoembedding_amd import INIT_UNIFORM, OPT_ADAGRAD, LookupTable
    from meepoembedding_amd.nn import DynamicEmbeddingBag
    t = LookupTable(1024, 64, device=dev, optimizer=OPT_ADAGRAD, initial_accumulator=0.1, max_batch=1 << 12, initializer=INIT_UNIFORM, init_scale=0.5, init_seed=3)
    keys = T(synth.keys_np(80, 0, 40), dev)
    off = torch.tensor([0, 3, 3, 20, 40], device=dev)
    layer = DynamicEmbeddingBag(t, mode="max", create_missing=True, out_dtype=torch.bfloat16)
    out = layer(keys, off)
    assert t.size() == 40 and out.dtype == torch.bfloat16
    ref, _ = pooled_max(t.find(keys)[0].cpu().numpy(), off.cpu().numpy())
    assert _bf16_equal(out.detach(), ref)
    before = t.find(keys)[0].clone()
    out.float().sum().backward()
    assert not torch.equal(before, t.find(keys)[0])
    with pytest.raises(ValueError, match="per_sample_weights"):
        layer(keys, off, per_sample_weights=torch.ones(40, device=dev))


def test_refusals(dev):
    from meepoembedding_amd import LookupTable, MeepoError, TableGroup
    keys = T(synth.keys_np(81, 0, 8), dev)
    off = torch.tensor([0, 3, 8], device=dev)
    narrow = [LookupTable(256, 64, device=dev, value_dtype=torch.bfloat16), LookupTable(256, 64, device=dev, int8_rows=True)]
    bf16_group = TableGroup([LookupTable(256, 64, device=dev, value_dtype=torch.bfloat16)])
    for t in narrow + [bf16_group]:
        out = torch.full((2, 64), SENTINEL, device=dev)
        with pytest.raises(MeepoError) as e:
            t.find_pooled_max(keys, off, out=out)
        assert e.value.code == _lib.ERR_UNSUPPORTED and bool((out == SENTINEL).all())
        with pytest.raises(MeepoError) as e:
            t.pooled_max_backward(off, torch.zeros((2, 64), dtype=torch.int32, device=dev), torch.zeros((2, 64), device=dev), 8)
        assert e.value.code == _lib.ERR_UNSUPPORTED
    t, _, _, _ = _table(dev, 64)
    with pytest.raises(ValueError, match="max"):
        t.find_pooled(keys, off, "max", weights=torch.ones(8, device=dev))
    # n = 2^32 through the C entry points, with small valid buffers: refused before anything is read or launched
    L, s = _lib.lib(), torch.cuda.current_stream(dev).cuda_stream
    out, arg = torch.full((2, 64), SENTINEL, device=dev), torch.zeros((2, 64), dtype=torch.int32, device=dev)
    bg, grads = torch.zeros((2, 64), device=dev), torch.full((8, 64), SENTINEL, device=dev)
    group = TableGroup([t])
    for rc in (L.mee_find_pooled_max(t._h, keys.data_ptr(), 1 << 32, off.data_ptr(), 2, out.data_ptr(), _lib.DTYPE_F32, None, arg.data_ptr(), s),
               L.mee_group_find_pooled_max(group._h, keys.data_ptr(), 1 << 32, off.data_ptr(), 2, out.data_ptr(), _lib.DTYPE_F32, None, arg.data_ptr(), s),
               L.mee_pooled_max_backward(t._h, 1 << 32, off.data_ptr(), 2, arg.data_ptr(), bg.data_ptr(), grads.data_ptr(), s),
               L.mee_group_pooled_max_backward(group._h, 1 << 32, off.data_ptr(), 2, arg.data_ptr(), bg.data_ptr(), grads.data_ptr(), s),
               L.mee_find_pooled_max(t._h, keys.data_ptr(), 8, off.data_ptr(), 2, out.data_ptr(), 7, None, None, s),                     # an unknown out_dtype
               L.mee_find_pooled_max(t._h, keys.data_ptr(), 8, off.data_ptr(), 2, out.data_ptr() + 4, _lib.DTYPE_BF16, None, None, s),   # a misaligned bf16 out
               L.mee_find_pooled_max(t._h, keys.data_ptr(), 8, off.data_ptr(), 2, None, _lib.DTYPE_F32, None, None, s),                  # no rows to write to
               L.mee_pooled_max_backward(t._h, 8, off.data_ptr(), 2, None, bg.data_ptr(), grads.data_ptr(), s)):
        assert rc == _lib.ERR_INVALID_ARG, L.mee_last_error()
    torch.cuda.synchronize(dev)
    assert bool((out == SENTINEL).all()) and bool((grads == SENTINEL).all())
