"""Bit-exact optimizer steps (SPEC.md §4) on inputs that leave no rounding freedom.

The tolerance of the other optimizer tests exists only because §4 leaves the order of the fp64 sum of a duplicate key's gradients free.
Here the gradients are exactly summable (tests/_apply_cases.py: every subset sum is exact in fp64, its rounding to fp32 is a real one), so
the oracle's result is the only correct one and every path through the step — LEAN and FULL kernels, inline lists, filed groups, fp64
partial rows, slabs, pending records, prefix-split merges, located, indexed and grouped forms, dedup_sum — is held to it bit for bit:
a partial sum kept in fp32, a second rounding, an approximate reciprocal or square root, a contracted multiply-add or a flushed subnormal
all show.  The last part runs one step over a grid of numeric edges (zeros, subnormals, overflow of g*g, inf, NaN, a zero denominator,
large Adam step numbers) on distinct keys, again bit for bit.

The first three tests need no GPU: they check the generator and the reference themselves (order invariance, teeth, the edge table)."""
import functools

import numpy as np
import pytest
import torch

import oracle
from _apply_cases import (EDGE_GRADS, EDGE_KEYS, EDGE_LR, EXTREME_CASES, T, assert_bits_equal_nan_aware, assert_tables_bit_equal,
                          bucketed_apply_extremes, check_exact_grads, edge_inputs, edge_reference, edge_runs, every_group_size_batch,
                          exact_grads_np, export_sorted)
from meepoembedding_amd import OPT_ADAGRAD, OPT_ADAM, LookupTable, synth

gpu = pytest.mark.gpu
FLT_MIN = np.float32(1.17549435e-38)


def _kinds(opt):
    return (OPT_ADAGRAD, oracle.OPT_ADAGRAD) if opt == "adagrad" else (OPT_ADAM, oracle.OPT_ADAM)


def _oracle_step(o, opt, keys, grads, step, eps=None):
    if opt == "adagrad":
        o.apply_adagrad(keys, grads, EDGE_LR[opt], 1e-10 if eps is None else eps)
    else:
        o.apply_adam(keys, grads, EDGE_LR[opt], 0.9, 0.999, 1e-8 if eps is None else eps, step)


def _step_kwargs(opt, step):
    return dict(lr=EDGE_LR[opt]) if opt == "adagrad" else dict(lr=EDGE_LR[opt], step=step)


# ---- CPU half: the generator and the reference --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cpu_case():
    """the every-group-size batch (dim 24, 'mixed') plus one key of 131072 occurrences, shuffled, and three steps of exact gradients"""
    dim = 24
    rng = np.random.default_rng(31)
    keys, rows, _, batch = every_group_size_batch(rng, dim, "mixed")
    big = synth.keys_np(125, 0, 1)
    bk = np.concatenate([batch, np.repeat(big, 131072)])
    rng.shuffle(bk)
    grads = [exact_grads_np(rng, bk.size, dim) for _ in range(3)]
    keys, rows = np.concatenate([keys, big]), np.concatenate([rows, synth.rows_np(big, dim, 2)])
    for a in (keys, rows, bk, *grads):
        a.flags.writeable = False
    return dim, keys, rows, bk, grads


def test_exact_gradients_are_what_they_claim():
    rng = np.random.default_rng(1)
    g = exact_grads_np(rng, 4096, 24)
    a = np.ldexp(g.astype(np.float64), 36)
    for e in (12, 24, 36):   # every exponent is drawn, with odd multipliers (a lower exponent's values would pass as a higher one's otherwise)
        m = a / 2.0 ** (36 - e)
        assert ((m == np.rint(m)) & (np.abs(m) <= 32) & (np.rint(m) % 2 == 1)).any()
    assert g.min() == -32 * 2.0 ** -12 and g.max() == 32 * 2.0 ** -12
    with pytest.raises(AssertionError):
        check_exact_grads(g, (1 << 19) + 1)                  # the batch bound
    with pytest.raises(AssertionError):
        check_exact_grads(np.full((1, 1), 2.0 ** -37, np.float32), 1)


@pytest.mark.parametrize("opt", ["adagrad", "adam"])
def test_reference_is_order_invariant(opt):
    """the oracle gives the same bits for two shuffles of one batch: with these gradients the fp64 sum has no order left in it"""
    dim, keys, rows, bk, grads = _cpu_case()
    rng = np.random.default_rng(2)
    tables = [oracle.OracleTable(4096, dim, optimizer=_kinds(opt)[1], initial_accumulator=0.1) for _ in range(2)]
    for o in tables:
        o.insert(keys, rows)
    for s, g in enumerate(grads):
        for o in tables:
            p = rng.permutation(bk.size)
            _oracle_step(o, opt, bk[p], g[p], s + 1)
    a, b = export_sorted(tables[0]), export_sorted(tables[1])
    assert len(a) == (3 if opt == "adagrad" else 4)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert not np.array_equal(a[1], rows[np.argsort(keys)])       # (the steps did move the rows)


def test_exact_gradients_have_teeth():
    """On the generator, not on a kernel: a sum carried in fp32, and a sum rounded twice, must differ from fl32(fp64 sum) — in every class
    of group sizes — or a kernel that did the same would pass the bit-exact tests."""
    dim, _, _, bk, grads = _cpu_case()
    g = grads[0]
    valid = bk != oracle.EMPTY_KEY
    uniq, inv, counts = np.unique(bk[valid], return_inverse=True, return_counts=True)
    gv = g[valid]
    sum64 = np.zeros((uniq.size, dim), np.float64)
    np.add.at(sum64, inv, gv.astype(np.float64))
    ref = sum64.astype(np.float32)
    back = np.zeros_like(sum64)                                   # another order and a partial grouping: the same fp64 bits
    np.add.at(back, inv[::-1], gv[::-1].astype(np.float64))
    half = np.zeros_like(sum64)
    np.add.at(half, inv[1::2], gv[1::2].astype(np.float64))
    even = np.zeros_like(sum64)
    np.add.at(even, inv[0::2], gv[0::2].astype(np.float64))
    assert np.array_equal(back, sum64) and np.array_equal(half + even, sum64)
    ou, ogs, _, ocnt = oracle.dedup_sum(bk, g, dim)               # the oracle's reduction is this sum
    oo = np.argsort(ou)
    assert np.array_equal(ou[oo], uniq) and np.array_equal(ocnt[oo], counts) and np.array_equal(ogs[oo], ref)
    sum32 = np.zeros((uniq.size, dim), np.float32)
    np.add.at(sum32, inv, gv)                                     # carried in fp32
    assert sum32.dtype == np.float32
    assert np.array_equal(sum32[counts == 1], ref[counts == 1])   # a single occurrence is a copy either way
    for lo, hi in ((2, 8), (9, 32), (33, 400), (401, 1 << 19)):
        m = (counts >= lo) & (counts <= hi)
        assert m.any()
        assert (sum64[m] != ref[m]).any(), f"groups of {lo}..{hi}: no sum needs a rounding to fp32"
        assert (sum32[m] != ref[m]).any(), f"groups of {lo}..{hi}: a sum carried in fp32 is not told from the fp64 sum"
    big = int(np.argmax(counts))
    assert counts[big] == 131072
    rows = gv[inv == big]
    partials = rows.reshape(-1, 32, dim).astype(np.float64).sum(axis=1)            # fp64 partial sums of 32 rows, exact
    twice = partials.astype(np.float32).astype(np.float64).sum(axis=0).astype(np.float32)   # ... each stored as float, then summed
    assert np.array_equal(partials.sum(axis=0).astype(np.float32), ref[big])
    assert (twice != ref[big]).any(), "a partial row stored as float is not told from the single rounding"


def test_reference_keeps_the_sign_of_a_single_zero_gradient():
    """'A key that occurs once uses its grad row unchanged' (SPEC §4) holds for -0 too: the reference copies such a row (0.0 + -0.0 would
    be +0.0).  Two or more occurrences are summed from +0.0, as every kernel sums them: a group of -0 alone gives +0.  The step then
    follows IEEE: fma(-lr, -0, -0) is +0."""
    keys = np.array([5, 6, 6, 7, 7, oracle.EMPTY_KEY], dtype=np.int64)
    g = np.repeat(np.array([[-0.0], [-0.0], [-0.0], [-0.0], [0.0], [1.0]], dtype=np.float32), 4, axis=1)
    uniq, gs, _, cnt = oracle.dedup_sum(keys, g, 4)
    assert uniq.tolist() == [5, 6, 7] and cnt.tolist() == [1, 2, 2]
    assert np.array_equal(gs.view(np.uint32)[:, 0], np.array([0x80000000, 0, 0], dtype=np.uint32))
    o = oracle.OracleTable(64, 4, optimizer=oracle.OPT_ADAGRAD, initial_accumulator=0.1)
    o.insert(keys[:2], np.full((2, 4), -0.0, dtype=np.float32))
    o.apply_adagrad(keys[:3], g[:3], 0.05, 1e-10)
    got = o.find(keys[:2])[0].view(np.uint32)
    assert (got[0] == 0).all()               # key 5, once: g = -0, fma(-lr, -0, -0) = +0
    assert (got[1] == 0x80000000).all()      # key 6, twice: g = +0, w stays -0


def _classes(x):
    zero, neg = x == 0, np.signbit(x)
    return {"+0": (zero & ~neg).any(), "-0": (zero & neg).any(), "subnormal": ((np.abs(x) > 0) & (np.abs(x) < FLT_MIN)).any(),
            "normal": (np.isfinite(x) & (np.abs(x) >= FLT_MIN)).any(), "+inf": (x == np.inf).any(), "-inf": (x == -np.inf).any(),
            "nan": np.isnan(x).any()}


@pytest.mark.parametrize("dim", [16, 100])
@pytest.mark.parametrize("opt", ["adagrad", "adam"])
def test_edge_table_reference(opt, dim):
    """What the edge grid asks of a kernel, read off the oracle: every class of value is among the expected outputs, NaN stays a minority
    (so that 'NaN compares by isnan' cannot hide a failure), and the sentences of SPEC §4 hold in the reference itself."""
    keys, w, s1, s2, g = edge_inputs(opt, dim)
    assert keys.size == EDGE_KEYS == np.unique(keys).size and 64 <= keys.size <= 256
    assert np.isfinite(w[:-4]).all() and not np.isfinite(w[-4:, 0][:3]).any()
    for v in EDGE_GRADS:       # every gradient of the grid is there (NaN by isnan, the zeros by sign)
        assert (np.isnan(g).any() if np.isnan(v) else ((g == v) & (np.signbit(g) == np.signbit(v))).any())
    order = np.argsort(keys)
    w, g, s1 = w[order], g[order], s1[order]
    acc = s1 if opt == "adagrad" else s2[order]
    for eps, step in edge_runs(opt):
        ref = edge_reference(opt, dim, eps, step)
        assert np.array_equal(ref[0], keys[order])
        for plane in ref[1:]:
            assert np.isnan(plane).mean() < 0.5
        seen = _classes(np.concatenate([p.ravel() for p in ref[1:]]))
        assert all(seen.values()), f"eps {eps} step {step}: missing among the expected outputs: {[k for k, v in seen.items() if not v]}"
        wn = ref[1]
        fin = np.isfinite(w)
        pos_zero_g = (g == 0) & ~np.signbit(g) & fin
        if eps == 0:       # 0 / 0 is NaN: a zero gradient over a zero denominator
            m = (g == 0) & (acc == 0) & fin & ((s1 == 0) if opt == "adam" else True)
            assert m.any() and np.isnan(wn[m]).all()
        else:              # a zero gradient leaves w as it is, the sign of -0 included (Adam: where m is zero too)
            m = pos_zero_g & ((s1 == 0) if opt == "adam" else True)
            assert m.any() and ((w[m] == 0) & np.signbit(w[m])).any()
            assert np.array_equal(wn[m].view(np.uint32), w[m].view(np.uint32))
            if opt == "adagrad":   # a -0 gradient reaches the step as -0, and IEEE makes fma(-lr, -0, -0) a +0 (Adam's m' is +0 by then: w stays)
                m = (g == 0) & np.signbit(g) & (w == 0) & np.signbit(w) & (acc > 0)
                assert m.any() and np.array_equal(wn[m].view(np.uint32), np.zeros(int(m.sum()), np.uint32))
        if opt == "adagrad":
            sub = (np.abs(ref[2]) > 0) & (np.abs(ref[2]) < FLT_MIN)          # a subnormal acc' is kept, and its square root is taken
            assert sub.any()
            if eps == 0:
                m = sub & (g > 0) & np.isfinite(g) & (w == 1)
                q = g[m] / np.sqrt(ref[2][m])
                assert m.any() and np.array_equal(wn[m], (np.float32(1) + np.float32(-EDGE_LR[opt]) * q.astype(np.float64)).astype(np.float32))
            m = np.isinf(ref[2]) & np.isfinite(g) & fin                      # g*g overflowed: g / inf is 0, w stays
            assert m.any() and np.array_equal(wn[m], w[m])
        assert np.isnan(wn[np.isnan(g)]).all() and np.isnan(ref[2][np.isnan(g)]).all()      # NaN propagates
        assert np.isnan(wn[np.isnan(w)]).all()
        m = np.isinf(w) & np.isfinite(g) & (g != 0) & (acc == np.float32(0.1)) & ((s1 == 0) if opt == "adam" else True)
        assert m.any() and np.array_equal(wn[m], w[m])                       # an infinite weight stays what it is under a finite step


# ---- GPU: every group size ----------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("layout", ["clustered", "spread", "mixed"])
@pytest.mark.parametrize("dim", [64, 128, 24, 100])
@pytest.mark.parametrize("opt", ["adagrad", "adam"])
def test_every_group_size_bit_exact(dev, opt, dim, layout):
    """The batch of test_optimizer_every_group_size (a key of every multiplicity 1..44, 64, 65, 100, 333, 2100, three times over, single keys,
    EMPTY_KEY padding) plus 100 absent keys, with exactly summable gradients: plain, located and indexed applies leave the oracle's bits.
    Dims: the compile-time instances DIM4 = 16 and 32 (64, 128), and the run-time instance with a full last chunk (24) and a partial one (100)."""
    rng = np.random.default_rng(7 + dim)
    keys, rows, filler, batch = every_group_size_batch(rng, dim, layout)
    batch = batch.copy()
    free = np.flatnonzero(batch == oracle.EMPTY_KEY)[::7][:100]
    batch[free] = synth.keys_np(124, 0, 100)                 # absent keys, spread over the padding
    assert free.size == 100 and (batch == oracle.EMPTY_KEY).sum() > 100 and not np.isin(batch[free], keys).any()
    n = batch.size
    kind, okind = _kinds(opt)
    mk = lambda: LookupTable(4096, dim, device=dev, optimizer=kind, max_batch=n, initial_accumulator=0.1)
    ta, tb, tc = mk(), mk(), mk()
    o = oracle.OracleTable(4096, dim, optimizer=okind, initial_accumulator=0.1)
    for t in (ta, tb, tc):
        t.insert(T(keys, dev), T(rows, dev))
    o.insert(keys, rows)
    bkt = T(batch, dev)
    for s in (1, 2):
        pool = exact_grads_np(rng, n // 3 + 1, dim, positions=n)      # indexed apply: three positions share a grad row
        gi = rng.integers(0, pool.shape[0], n).astype(np.int64)
        g = pool[gi]
        _, _, slots = tb.find_located(bkt)
        kw = _step_kwargs(opt, s)
        fn = (lambda t: t.apply_adagrad) if opt == "adagrad" else (lambda t: t.apply_adam)
        fn(ta)(bkt, T(g, dev), **kw)
        fn(tb)(bkt, T(g, dev), slots=slots, **kw)
        fn(tc)(bkt, T(pool, dev), grad_index=T(gi, dev), **kw)
        _oracle_step(o, opt, batch, g, s)
        for t, form in ((ta, "plain"), (tb, "located"), (tc, "indexed")):
            assert t.status() == 0
            assert_tables_bit_equal(t, o, f"step {s}, {form}:")
    g1 = exact_grads_np(rng, filler.size, dim)               # the scratch is left clean: a batch of distinct keys right behind it
    (ta.apply_adagrad if opt == "adagrad" else ta.apply_adam)(T(filler, dev), T(g1, dev), **_step_kwargs(opt, 3))
    _oracle_step(o, opt, filler, g1, 3)
    assert ta.status() == 0
    assert_tables_bit_equal(ta, o, "the distinct-key batch behind it:")


# ---- GPU: the rare ways through the bucketed apply ----------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("opt", ["adagrad", "adam"])
@pytest.mark.parametrize("kernel", ["auto", "lean", "full"])
@pytest.mark.parametrize("case", EXTREME_CASES)
def test_bucketed_apply_extremes_bit_exact(dev, case, opt, kernel):
    """test_bucketed_apply_extremes (tests/_apply_cases.py: bucketed_apply_extremes) on exactly summable gradients, dim 64: slabs, pending
    records, mono_pass and prefix-split merges, split buckets, the one-block bucket — every one bit for bit, plain and located."""
    bucketed_apply_extremes(dev, case, opt, kernel, 64, grads="exact")


@gpu
@pytest.mark.parametrize("opt,dim", [("adagrad", 128), ("adam", 100)])
@pytest.mark.parametrize("kernel", ["lean", "full"])
@pytest.mark.parametrize("case", EXTREME_CASES)
def test_bucketed_apply_extremes_wide_bit_exact(dev, case, kernel, opt, dim):
    """one wide pass each: DIM4 = 32 (fp64 partial rows in memory) and the run-time instance with a partial last chunk; gradients drawn on the device"""
    bucketed_apply_extremes(dev, case, opt, kernel, dim, grads="exact")


# ---- GPU: dedup_sum -----------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("compact", [True, False], ids=["compact", "padded"])
def test_dedup_sum_bit_exact(dev, compact):
    dim, n = 64, 40000
    rng = np.random.default_rng(7)
    keys = np.concatenate([rng.integers(0, 3000, size=n - 5200), np.arange(5000, 5200), np.full(5000, 77)]).astype(np.int64)  # one heavy key, 200 single ones
    rng.shuffle(keys)
    keys[123] = oracle.EMPTY_KEY
    grads = exact_grads_np(rng, n, dim)
    t = LookupTable(64, dim, device=dev, max_batch=n)
    uniq, gs, cnt, inv = [x.cpu().numpy() for x in t.dedup_sum(T(keys, dev), T(grads, dev), compact=compact)]
    assert t.status() == 0
    if not compact:                                          # padded: every distinct key once, EMPTY and count 0 elsewhere
        assert uniq.size == n and np.array_equal(uniq == oracle.EMPTY_KEY, cnt == 0)
    live = np.flatnonzero(cnt > 0)
    ou, ogs, _, ocnt = oracle.dedup_sum(keys, grads, dim)
    order, oorder = live[np.argsort(uniq[live])], np.argsort(ou)
    assert np.array_equal(uniq[order], ou[oorder]) and np.array_equal(cnt[order], ocnt[oorder])
    assert np.array_equal(gs[order], ogs[oorder])
    assert inv[123] == -1 and np.array_equal(uniq[inv[inv >= 0]], keys[inv >= 0])
    once = np.flatnonzero(inv >= 0)[cnt[inv[inv >= 0]] == 1]                # single occurrences are copies
    assert once.size >= 190 and np.array_equal(gs[inv[once]], grads[once])
    assert int(cnt.max()) == int((keys == 77).sum()) >= 4999


# ---- GPU: groups --------------------------------------------------------------------------------------------------------------------------------
def _segment(rng, u, shared):
    """one member's share of a step: a heavy group (700), groups past the partial-row and chunk thresholds (100, 40, 33), 36 small groups of
    2..8, 200 single keys, ten keys that the other members hold too (1..29 times each), three absent keys, EMPTY_KEY padding; shuffled"""
    k = np.concatenate([np.repeat(u[:4], [700, 100, 40, 33]), np.repeat(u[4:40], rng.integers(2, 9, 36)), u[40:240],
                        np.repeat(shared[:10], rng.integers(1, 30, 10)), synth.keys_np(998, int(rng.integers(0, 1000)), 3),
                        np.full(2, oracle.EMPTY_KEY)])
    rng.shuffle(k)
    return k


def _bags(rng, seg_sizes, bpt):
    """bag offsets that cut every member's segment into bpt bags (some empty; all empty for an empty segment)"""
    lens = []
    for m in seg_sizes:
        cuts = np.sort(rng.integers(0, m + 1, bpt - 1)) if m else np.zeros(bpt - 1, np.int64)
        lens.append(np.diff(np.concatenate([[0], cuts, [m]])))
    lens = np.concatenate(lens).astype(np.int64)
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), np.repeat(np.arange(lens.size), lens).astype(np.int64)


def _group_members(dev, rng, dims, opt, shared):
    kind, okind = _kinds(opt)
    tables, oracles, univ = [], [], []
    for j, dim in enumerate(dims):
        u = np.concatenate([synth.keys_np(600 + j, 0, 600), shared])            # the shared keys: other rows in every member
        rows = rng.standard_normal((u.size, dim)).astype(np.float32)
        t = LookupTable(2048, dim, device=dev, optimizer=kind, max_batch=1 << 14, initial_accumulator=0.1)
        o = oracle.OracleTable(2048, dim, optimizer=okind, initial_accumulator=0.1)
        t.insert(T(u, dev), T(rows, dev)); o.insert(u, rows)
        tables.append(t); oracles.append(o); univ.append(u)
    return tables, oracles, univ


@gpu
@pytest.mark.parametrize("form", ["apply", "indexed", "pooled_located", "pooled"])
@pytest.mark.parametrize("dim", [64, 24])
@pytest.mark.parametrize("opt", ["adagrad", "adam"])
def test_table_group_steps_bit_exact(dev, opt, dim, form):
    """A TableGroup of three members that all hold the same ten keys (never to be merged across members), heavy and small groups in every
    segment, one segment empty per step: each grouped form of the step against one oracle table per member fed that member's segment."""
    from meepoembedding_amd import TableGroup
    rng = np.random.default_rng(dim + len(form))
    shared = synth.keys_np(555, 0, 10)
    tables, oracles, univ = _group_members(dev, rng, (dim,) * 3, opt, shared)
    grp = TableGroup(tables, max_apply_batch=1 << 14)
    bpt = 11
    for s in (1, 2):
        empty = (2, 0)[s - 1]
        segs = [np.zeros(0, np.int64) if j == empty else _segment(rng, univ[j], shared) for j in range(3)]
        keys = np.concatenate(segs)
        n = keys.size
        bounds = np.concatenate([[0], np.cumsum([k.size for k in segs])]).astype(np.int64)
        kw = _step_kwargs(opt, s)
        if form == "apply":
            gpos = exact_grads_np(rng, n, dim)
            (grp.apply_adagrad if opt == "adagrad" else grp.apply_adam)(T(keys, dev), T(bounds, dev), T(gpos, dev), **kw)
        elif form == "indexed":
            pool = exact_grads_np(rng, n // 3 + 1, dim, positions=n)
            gi = rng.integers(0, pool.shape[0], n).astype(np.int64)
            gpos = pool[gi]
            grp.apply_indexed(T(keys, dev), T(bounds, dev), T(pool, dev), T(gi, dev), opt, **kw)
        else:
            off, bag_of = _bags(rng, [k.size for k in segs], bpt)
            assert np.array_equal(off[::bpt], bounds)
            bag_grads = exact_grads_np(rng, 3 * bpt, dim, positions=n)
            gpos = bag_grads[bag_of]
            located = None
            if form == "pooled_located":
                located = torch.empty(n, dtype=torch.int64, device=dev)
                grp.find_pooled(T(keys, dev), T(off, dev), "sum", located=located)
            grp.apply_pooled(T(keys, dev), T(off, dev), T(bag_grads, dev), T(bag_of, dev), opt, located=located, **kw)
        for j in range(3):
            lo, hi = bounds[j], bounds[j + 1]
            if hi > lo:
                _oracle_step(oracles[j], opt, keys[lo:hi], gpos[lo:hi], s)
            assert tables[j].status() == 0
            assert_tables_bit_equal(tables[j], oracles[j], f"step {s}, member {j}:")
    grp.close()


@gpu
@pytest.mark.parametrize("opt", ["adagrad", "adam"])
def test_mixed_group_step_bit_exact(dev, opt):
    """A MixedTableGroup over dims (8, 64, 100, 128): apply_pooled with the forward's located rows (step 1) and without (step 2), one member
    without keys per step, against one oracle table per member."""
    from meepoembedding_amd import MixedTableGroup
    dims = (8, 64, 100, 128)
    rng = np.random.default_rng(17)
    shared = synth.keys_np(555, 0, 10)
    tables, oracles, univ = _group_members(dev, rng, dims, opt, shared)
    grp = MixedTableGroup(tables, max_apply_batch=1 << 14)
    bpt = 16
    for s in (1, 2):
        empty = (3, 1)[s - 1]
        segs = [np.zeros(0, np.int64) if j == empty else _segment(rng, univ[j], shared) for j in range(len(dims))]
        keys = np.concatenate(segs)
        n = keys.size
        off, bag_of = _bags(rng, [k.size for k in segs], bpt)
        grads = [exact_grads_np(rng, bpt, d, positions=n) for d in dims]
        flat = torch.empty(grp.layout(bpt)[1], device=dev)
        for v, g in zip(grp.views(flat, bpt), grads):
            v.copy_(T(g, dev))
        located = None
        if s == 1:
            located = torch.empty(n, dtype=torch.int64, device=dev)
            grp.find_pooled(T(keys, dev), T(off, dev), "sum", located=located)
        grp.apply_pooled(T(keys, dev), T(off, dev), flat, T(bag_of, dev), opt, located=located, **_step_kwargs(opt, s))
        for j in range(len(dims)):
            lo, hi = off[j * bpt], off[(j + 1) * bpt]
            if hi > lo:
                _oracle_step(oracles[j], opt, keys[lo:hi], grads[j][bag_of[lo:hi] - j * bpt], s)
            assert tables[j].status() == 0
            assert_tables_bit_equal(tables[j], oracles[j], f"step {s}, member {j} (dim {dims[j]}):")
    grp.close()


# ---- GPU: numeric edges, distinct keys ----------------------------------------------------------------------------------------------------------
def _place(t, keys, w, s1, s2, dev):
    kt = T(keys, dev)
    t.insert(kt, T(w, dev))
    assert bool(t.assign_plane(1, kt, T(s1, dev)).all())
    if s2 is not None:
        assert bool(t.assign_plane(2, kt, T(s2, dev)).all())


def _compare_with_edge_reference(tables, opt, dim, eps, step, what):
    """the tables' pairs together are the reference's: bitwise, NaN by isnan"""
    parts = [export_sorted(t) for t in tables]
    got = [np.concatenate([p[i] for p in parts]) for i in range(len(parts[0]))]
    order = np.argsort(got[0])
    ref = edge_reference(opt, dim, eps, step)
    assert len(got) == len(ref) and np.array_equal(got[0][order], ref[0])
    for name, x, z in zip(("values", "state1", "state2"), got[1:], ref[1:]):
        assert_bits_equal_nan_aware(x[order], z, f"{what}, eps {eps}, step {step}: {name}")


@gpu
@pytest.mark.parametrize("entry", ["lean", "full", "located", "indexed", "group"])
@pytest.mark.parametrize("dim", [16, 100])
@pytest.mark.parametrize("opt", ["adagrad", "adam"])
def test_numeric_edges_bit_exact(dev, opt, dim, entry):
    """One step over the edge grid (tests/_apply_cases.py: edge_inputs) through one entry point, for every eps and Adam step number: weights
    and state planes carry the oracle's bits — 0/0 is NaN, -0 survives, subnormals are kept, sqrt and / are correctly rounded, g/inf is 0,
    inf and NaN propagate (test_edge_table_reference reads these off the reference).
    'lean' / 'full': set_tuning("apply_kernel", 0 / 1) decides the plan's kernel at any batch size, this one of 132 keys included
    (part_plan_for in meepo_apply_part.h: `full = kernel_choice >= 0 ? kernel_choice != 0 : ...`; tests/test_part_plan.py holds the forced
    plans at n = 127 .. 5M), so the grid reaches both kernels' update code."""
    from meepoembedding_amd import TableGroup
    keys, w, s1, s2, g = edge_inputs(opt, dim)
    n = keys.size
    kind, _ = _kinds(opt)
    mk = lambda: LookupTable(512, dim, device=dev, optimizer=kind, max_batch=1024)
    cut = n // 2 - 3
    tables = [mk(), mk()] if entry == "group" else [mk()]
    parts = [slice(0, cut), slice(cut, n)] if entry == "group" else [slice(0, n)]
    grp = TableGroup(tables, max_apply_batch=1024) if entry == "group" else None
    if entry in ("lean", "full"):
        tables[0].set_tuning("apply_kernel", {"lean": 0, "full": 1}[entry])
    kt, gt = T(keys, dev), T(g, dev)
    for eps, step in edge_runs(opt):
        for t, p in zip(tables, parts):
            _place(t, keys[p], w[p], s1[p], None if s2 is None else s2[p], dev)
        kw = dict(_step_kwargs(opt, step), eps=eps)
        t = tables[0]
        fn = t.apply_adagrad if opt == "adagrad" else t.apply_adam
        if entry in ("lean", "full"):
            fn(kt, gt, **kw)
        elif entry == "located":
            _, found, slots = t.find_located(kt)
            assert bool(found.all())
            fn(kt, gt, slots=slots, **kw)
        elif entry == "indexed":
            fn(kt, T(g[::-1], dev), grad_index=T(np.arange(n - 1, -1, -1, dtype=np.int64), dev), **kw)
        else:
            (grp.apply_adagrad if opt == "adagrad" else grp.apply_adam)(kt, T(np.array([0, cut, n], dtype=np.int64), dev), gt, **kw)
        assert all(t.status() == 0 for t in tables)
        _compare_with_edge_reference(tables, opt, dim, eps, step, entry)
    if grp is not None:
        grp.close()


@gpu
@pytest.mark.parametrize("opt", ["adagrad", "adam"])
def test_numeric_edges_mixed_group_bit_exact(dev, opt):
    """the same grid through MixedTableGroup.apply_pooled: members of dim 16 and dim 100, every key a bag of its own"""
    from meepoembedding_amd import MixedTableGroup
    dims = (16, 100)
    kind, _ = _kinds(opt)
    inputs = [edge_inputs(opt, d) for d in dims]
    n = EDGE_KEYS
    tables = [LookupTable(512, d, device=dev, optimizer=kind, max_batch=1024) for d in dims]
    grp = MixedTableGroup(tables, max_apply_batch=1024)
    keys = T(np.concatenate([i[0] for i in inputs]), dev)
    off = torch.arange(2 * n + 1, dtype=torch.int64, device=dev)
    bag_of = torch.arange(2 * n, dtype=torch.int64, device=dev)
    flat = torch.empty(grp.layout(n)[1], device=dev)
    for v, i in zip(grp.views(flat, n), inputs):
        v.copy_(T(i[4], dev))
    for eps, step in edge_runs(opt):
        for t, i in zip(tables, inputs):
            _place(t, *i[:4], dev)
        grp.apply_pooled(keys, off, flat, bag_of, opt, eps=eps, **_step_kwargs(opt, step))
        for t, d in zip(tables, dims):
            assert t.status() == 0
            _compare_with_edge_reference([t], opt, d, eps, step, f"mixed group, dim {d}")
    grp.close()
