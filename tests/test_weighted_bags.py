"""Weighted embedding bags (SPEC.md §3: find_pooled_weighted, pooled_weighted_backward and their group forms): the C-ABI symbols,
the Python wrappers' argument checks and the custom-op registration on the CPU; on the GPU the kernels against a numpy
restatement of the SPEC rule, the table step against the oracle and the layer against torch.nn.EmbeddingBag(per_sample_weights)."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle
from _apply_cases import assert_bits_equal_nan_aware
from meepoembedding_amd import _lib, synth
from meepoembedding_amd.nn import DynamicEmbeddingBag, apply_grad_pooled_weighted, lookup_pooled_weighted

NEW_SYMBOLS = ("mee_find_pooled_weighted", "mee_pooled_weighted_backward", "mee_group_find_pooled_weighted",
               "mee_group_pooled_weighted_backward")
RTOL, ATOL = 1e-6, 1e-9


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def weighted_pool(rows, off, w):
    """SPEC.md §3 find_pooled_weighted on find's rows: acc = w_first * row_first, then acc = acc + (w_i * row_i), every product and
    every sum rounded to fp32 (numpy float32 arithmetic rounds each operation once); an empty bag is zeros."""
    off = np.asarray(off, np.int64)
    lens = off[1:] - off[:-1]
    out = np.zeros((lens.size, rows.shape[1]), np.float32)
    for step in range(int(lens.max()) if lens.size else 0):
        m = lens > step
        p = off[:-1][m] + step
        prod = w[p][:, None] * rows[p]
        out[m] = prod if step == 0 else out[m] + prod
    return out


def bag_of_positions(off):
    off = np.asarray(off, np.int64)
    return np.repeat(np.arange(off.size - 1), off[1:] - off[:-1])


def weight_grads_ref(bag_grads, rows, off):
    """fp64 reference of weight_grads and the SPEC bound 1e-6 * sum |products|"""
    b = bag_of_positions(off)
    prod = bag_grads[b].astype(np.float64) * rows.astype(np.float64)
    return prod.sum(1), 1e-6 * np.abs(prod).sum(1) + 1e-30


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_new_symbols_declared_and_exported(built):
    from test_abi_load import _declared
    names = _declared()
    L = C.CDLL(_lib.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s in names and s in _lib.PROTOTYPES and hasattr(L, s), s
    assert _lib.lib().mee_abi_version() == 2     # additive: the ABI version stays


def test_wrappers_reject_bad_weights_before_any_launch(built, monkeypatch):
    from meepoembedding_amd import LookupTable, MeepoError, TableGroup
    from meepoembedding_amd import table as tm
    calls = []

    class Recorder:   # stands in for the library: records what would have been launched
        def __getattr__(self, name):
            calls.append(name)
            return lambda *a: 0

    monkeypatch.setattr(tm._lib, "lib", lambda: Recorder())
    monkeypatch.setattr(tm, "_stream_ptr", lambda device: 0)
    t = LookupTable.__new__(LookupTable)
    t._h, t.device, t.dim = None, torch.device("cpu"), 8
    g = TableGroup.__new__(TableGroup)
    g._h, g.tables, g.device, g.dim = None, [t, t], torch.device("cpu"), 8
    keys = torch.arange(6, dtype=torch.int64)
    off, goff = torch.tensor([0, 2, 6]), torch.tensor([0, 1, 3, 4, 6])
    good = torch.ones(6)
    with pytest.raises(ValueError):
        t.find_pooled(keys, off, "mean", weights=good)
    with pytest.raises(ValueError):
        g.find_pooled(keys, goff, "mean", weights=good)
    with pytest.raises(ValueError):
        DynamicEmbeddingBag(t, mode="mean")(keys, off, per_sample_weights=good)
    for bad in (torch.ones(5), torch.ones(7), torch.ones(6, dtype=torch.float64), torch.ones(6, dtype=torch.float16),
                torch.ones(6, device="meta"), torch.ones(12)[::2]):
        with pytest.raises(MeepoError):
            t.find_pooled(keys, off, "sum", weights=bad)
        with pytest.raises(MeepoError):
            g.find_pooled(keys, goff, "sum", weights=bad)
        with pytest.raises(MeepoError):
            t.pooled_weighted_backward(keys, off, bad, torch.zeros(2, 8))
        with pytest.raises(MeepoError):
            g.pooled_weighted_backward(keys, goff, bad, torch.zeros(4, 8))
    with pytest.raises(ValueError):   # located is the weighted form's output
        t.find_pooled(keys, off, "sum", located=torch.empty(6, dtype=torch.int64))
    assert calls == []
    t.find_pooled(keys, off, "sum", weights=good)
    t.pooled_weighted_backward(keys, off, good, torch.zeros(2, 8), want_weight_grads=False)
    g.find_pooled(keys, goff, "sum", weights=good)
    g.pooled_weighted_backward(keys, goff, good, torch.zeros(4, 8))
    assert calls == list(NEW_SYMBOLS)


class WeightedCpuTable:
    """Test adapter: the oracle-backed CPU table plus the two weighted methods, in plain torch."""

    def __new__(cls, *a, **kw):
        from _cpu_backend import CpuTable

        class _T(CpuTable):
            def find_pooled(self, keys, bag_offsets, mode="sum", weights=None, located=None):
                rows, found = self.find(keys)
                if located is not None:
                    located.fill_(-1)            # no handles on the CPU: the backward reads the rows itself
                out = weighted_pool(rows.numpy(), bag_offsets.numpy(), weights.numpy()) if weights is not None \
                    else oracle.pool_rows(rows.numpy(), bag_offsets.numpy(), mode)
                return torch.from_numpy(out), found

            def pooled_weighted_backward(self, keys, bag_offsets, weights, bag_grads, located=None, want_weight_grads=True):
                b = torch.from_numpy(bag_of_positions(bag_offsets.numpy()))
                g = bag_grads[b]
                wg = (g.double() * self.find(keys)[0].double()).sum(1).float() if want_weight_grads else None
                return weights[:, None] * g, wg

            def apply_adagrad(self, keys, grads, lr, eps=1e-10, slots=None):
                super().apply_adagrad(keys, grads, lr, eps)

        return _T(*a, **kw)


def test_weighted_bag_ops_on_cpu_adapter(built):
    """The torch.library registration of meepo::lookup_pooled_weighted / apply_grad_pooled_weighted (schema, fake kernels,
    autograd) and the grad of per_sample_weights, on an oracle-backed table."""
    torch.manual_seed(0)
    dim = 16
    t = WeightedCpuTable(4096, dim, optimizer=oracle.OPT_ADAGRAD, initial_accumulator=0.1)
    keys = torch.from_numpy(synth.keys_np(8, 0, 40))
    t.insert(keys, torch.rand(40, dim) - 0.5)
    layer = DynamicEmbeddingBag(t, mode="sum", lr=0.05)
    off = torch.tensor([0, 3, 3, 10, 25, 40])
    w = torch.randn(40, requires_grad=True)
    rows0, _ = t.find(keys)
    out = layer(keys, off, per_sample_weights=w)
    bag = torch.from_numpy(bag_of_positions(off.numpy()))
    ref = torch.zeros(5, dim, dtype=torch.float64).index_add_(0, bag, w.detach().double()[:, None] * rows0.double())
    torch.testing.assert_close(out.double(), ref, rtol=1e-5, atol=1e-6)
    G = torch.randn(5, dim)
    (out * G).sum().backward()
    torch.testing.assert_close(w.grad, (G[bag].double() * rows0.double()).sum(1).float(), rtol=1e-6, atol=1e-7)
    rows1, _ = t.find(keys)
    assert not torch.equal(rows0, rows1)                        # the backward made the table step
    # no grad for the weights is asked: the table still takes its step
    w2 = torch.randn(40)
    layer(keys, off, per_sample_weights=w2).sum().backward()
    assert not torch.equal(rows1, t.find(keys)[0])
    torch.library.opcheck(lookup_pooled_weighted, (keys, off, w, layer._anchor, layer.table_id),
                          test_utils=("test_schema", "test_faketensor", "test_autograd_registration"))
    torch.library.opcheck(apply_grad_pooled_weighted, (keys, off, w.detach(), G, torch.empty(0, dtype=torch.int64), layer.table_id, True),
                          test_utils=("test_schema", "test_faketensor", "test_autograd_registration"))
    from torch.fx.experimental.proxy_tensor import make_fx
    gm = make_fx(lambda k, o, ww, a: lookup_pooled_weighted(k, o, ww, a, layer.table_id)[0] * 2, tracing_mode="fake")(keys, off, w, layer._anchor)
    assert "torch.ops.meepo.lookup_pooled_weighted" in gm.code


# ---- GPU ----------------------------------------------------------------------------------------------------------------
def _filled_table(dev, dim, n_keys, seed, **kw):
    from meepoembedding_amd import LookupTable
    rng = np.random.default_rng(seed)
    t = LookupTable(2 * n_keys, dim, device=dev, max_batch=1 << 14, default_value=0.125, **kw)
    u = synth.keys_np(seed, 0, n_keys)
    t.insert(T(u, dev), T(rng.standard_normal((n_keys, dim)).astype(np.float32), dev))
    _bump_layout_epoch(t)                                       # handles then carry a non-zero epoch tag
    return t, u, rng


def _bump_layout_epoch(t):
    """mee_remove of a key the table does not hold: no row moves, but slot handles taken before are stale"""
    t.remove(T(synth.keys_np(4242, 0, 1), t.device))


def _batch(rng, u, lens):
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    keys = u[rng.integers(0, u.size, off[-1])].copy()
    keys[5] = oracle.EMPTY_KEY; keys[9] = synth.keys_np(777, 0, 1)[0]; keys[30] = oracle.RECLAIMED_KEY   # reserved, absent, reserved
    w = rng.standard_normal(off[-1]).astype(np.float32)
    w[::7] = 0.0; w[3::11] = -np.abs(w[3::11])                   # zero and negative weights
    return keys, off, w


# the launch shape is picked on the host from the average bag: four bags per wave below 12 keys per bag (a tile per short bag, the
# wave's four tiles on a bag of 16 or more), a wave per bag from 12 on
SHAPES = (np.concatenate([[0, 1, 2, 3, 0, 57, 1, 16, 17, 15], np.arange(60) % 12, [0]]),   # 442 keys in 71 bags: four bags per wave
          np.concatenate([[0, 1, 2, 3, 0, 57, 400, 1], np.arange(30) % 12, [0]]),          # 611 in 39 (one 400-key bag): a wave per bag
          np.concatenate([[0, 1, 33], np.arange(40) % 55 + 5, [0, 16, 15, 17]]))           # 1062 in 47: a wave per bag


def wave_per_bag(lens):
    return int(np.sum(lens)) // lens.size >= 12


assert [wave_per_bag(x) for x in SHAPES] == [False, True, True] and max(SHAPES[0]) >= 16


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [4, 24, 64, 128, 1024, 100, 1020])
def test_weighted_forward_bit_exact(dev, dim):
    t, u, rng = _filled_table(dev, dim, 3000, 60 + dim)
    for lens in SHAPES:
        keys, off, w = _batch(rng, u, lens)
        loc = torch.empty(keys.size, dtype=torch.int64, device=dev)
        out, found = t.find_pooled(T(keys, dev), T(off, dev), weights=T(w, dev), located=loc)
        rows, ef = t.find(T(keys, dev))
        rows = rows.cpu().numpy()
        assert np.array_equal(found.cpu().numpy(), ef.cpu().numpy())
        assert_bits_equal_nan_aware(out.cpu().numpy(), weighted_pool(rows, off, w), f"weighted find_pooled dim {dim}")
        # the handles are mee_find_located's, epoch tag included
        _, _, slots = t.find_located(T(keys, dev))
        assert torch.equal(loc, slots)
        assert bool(((loc[loc >= 0] & ~_lib.HANDLE_SLOT_MASK) != 0).all()) and bool((loc >= 0).any())
        # all-ones weights: bit-identical to the unweighted sum
        ones, _ = t.find_pooled(T(keys, dev), T(off, dev), weights=torch.ones(keys.size, device=dev))
        plain, _ = t.find_pooled(T(keys, dev), T(off, dev), "sum")
        assert_bits_equal_nan_aware(ones.cpu().numpy(), plain.cpu().numpy(), f"all-ones weights dim {dim}")
    e_out, _ = t.find_pooled(T(keys[:0], dev), torch.zeros(4, dtype=torch.int64, device=dev), weights=torch.ones(0, device=dev))
    assert e_out.shape == (3, dim) and not bool(e_out.any())


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [64, 128, 24, 100])
def test_group_weighted_ops_equal_per_member(dev, dim):
    """mee_group_find_pooled_weighted / mee_group_pooled_weighted_backward == the single-table operators per member, bit-exact, in
    both launch shapes; the group backward gives the same results through the forward's handles and by probe."""
    from meepoembedding_amd import TableGroup
    n_tables, bpt = 3, 30
    members = [_filled_table(dev, dim, 1500, 80 + j) for j in range(n_tables)]
    grp = TableGroup([m[0] for m in members], max_apply_batch=1 << 14)
    rng = np.random.default_rng(dim)
    for long_bags in (False, True):
        lens = rng.integers(8, 40, n_tables * bpt) if long_bags else rng.integers(0, 7, n_tables * bpt)
        lens[3] = 0; lens[bpt] = 25
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        keys = np.concatenate([members[j][1][rng.integers(0, 1500, int(off[(j + 1) * bpt] - off[j * bpt]))] for j in range(n_tables)])
        keys[1] = synth.keys_np(997, 0, 1)[0]
        w = rng.standard_normal(keys.size).astype(np.float32)
        loc, loc_plain = (torch.empty(keys.size, dtype=torch.int64, device=dev) for _ in range(2))
        out, found = grp.find_pooled(T(keys, dev), T(off, dev), weights=T(w, dev), located=loc)
        grp.find_pooled(T(keys, dev), T(off, dev), located=loc_plain)
        assert torch.equal(loc, loc_plain)                      # the group's handle format
        for j in range(n_tables):
            lo, hi = off[j * bpt], off[(j + 1) * bpt]
            eo, ef = members[j][0].find_pooled(T(keys[lo:hi], dev), T(off[j * bpt:(j + 1) * bpt + 1] - lo, dev), weights=T(w[lo:hi], dev))
            assert torch.equal(out[j * bpt:(j + 1) * bpt], eo) and torch.equal(found[lo:hi], ef)
        ones, _ = grp.find_pooled(T(keys, dev), T(off, dev), weights=torch.ones(keys.size, device=dev))
        assert torch.equal(ones, grp.find_pooled(T(keys, dev), T(off, dev), "sum")[0])
        assert wave_per_bag(lens) == long_bags
        bg = rng.standard_normal((lens.size, dim)).astype(np.float32)
        g_loc, wg_loc = grp.pooled_weighted_backward(T(keys, dev), T(off, dev), T(w, dev), T(bg, dev), located=loc)
        g_probe, wg_probe = grp.pooled_weighted_backward(T(keys, dev), T(off, dev), T(w, dev), T(bg, dev))
        assert torch.equal(g_loc, g_probe) and torch.equal(wg_loc, wg_probe)
        for j in range(n_tables):
            lo, hi = off[j * bpt], off[(j + 1) * bpt]
            eg, ewg = members[j][0].pooled_weighted_backward(T(keys[lo:hi], dev), T(off[j * bpt:(j + 1) * bpt + 1] - lo, dev), T(w[lo:hi], dev),
                                                             T(bg[j * bpt:(j + 1) * bpt], dev))
            assert torch.equal(g_probe[lo:hi], eg) and torch.equal(wg_probe[lo:hi], ewg)
        rows = torch.cat([members[j][0].find(T(keys[off[j * bpt]:off[(j + 1) * bpt]], dev))[0] for j in range(n_tables)]).cpu().numpy()
        ref, tol = weight_grads_ref(bg, rows, off)
        assert np.all(np.abs(wg_probe.cpu().numpy().astype(np.float64) - ref) <= tol)
    grp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [64, 128, 24, 1024, 100, 1020])
def test_weighted_backward(dev, dim):
    """grads bit-exact, weight_grads within the SPEC bound of fp64, identical with and without handles, none without weight_grads."""
    t, u, rng = _filled_table(dev, dim, 3000, 90 + dim)
    for lens in SHAPES:
        keys, off, w = _batch(rng, u, lens)
        bg = rng.standard_normal((lens.size, dim)).astype(np.float32)
        loc = torch.empty(keys.size, dtype=torch.int64, device=dev)
        t.find_pooled(T(keys, dev), T(off, dev), weights=T(w, dev), located=loc)
        g_probe, wg_probe = t.pooled_weighted_backward(T(keys, dev), T(off, dev), T(w, dev), T(bg, dev))
        g_loc, wg_loc = t.pooled_weighted_backward(T(keys, dev), T(off, dev), T(w, dev), T(bg, dev), located=loc)
        g_only, none = t.pooled_weighted_backward(T(keys, dev), T(off, dev), T(w, dev), T(bg, dev), want_weight_grads=False)
        assert none is None
        assert np.array_equal(g_probe.cpu().numpy(), w[:, None] * bg[bag_of_positions(off)])
        assert torch.equal(g_probe, g_loc) and torch.equal(g_probe, g_only) and torch.equal(wg_probe, wg_loc)
        ref, tol = weight_grads_ref(bg, t.find(T(keys, dev))[0].cpu().numpy(), off)
        assert np.all(np.abs(wg_probe.cpu().numpy().astype(np.float64) - ref) <= tol)
        # handles of an earlier layout epoch: the backward probes again and gives the same results
        _bump_layout_epoch(t)
        g_stale, wg_stale = t.pooled_weighted_backward(T(keys, dev), T(off, dev), T(w, dev), T(bg, dev), located=loc)
        assert torch.equal(g_stale, g_probe) and torch.equal(wg_stale, wg_probe)


@pytest.mark.gpu
def test_weighted_ops_tolerate_bad_offsets(dev):
    """Offsets past the key array are cut at its end, a decreasing pair is an empty bag (the clamps of find_pooled)."""
    t, u, rng = _filled_table(dev, 64, 100, 33)
    keys = u.copy()
    w = rng.standard_normal(100).astype(np.float32)
    off = torch.tensor([0, 10, 10, 90, 1 << 40, 1 << 41, 3], dtype=torch.int64, device=dev)
    clamped = np.array([0, 10, 10, 90, 100, 100, 100])        # the same bags: [90, 2^40) -> [90, 100), the last two empty
    bg = rng.standard_normal((6, 64)).astype(np.float32)
    out, _ = t.find_pooled(T(keys, dev), off, weights=T(w, dev))
    rows = t.find(T(keys, dev))[0].cpu().numpy()
    assert np.array_equal(out.cpu().numpy(), weighted_pool(rows, clamped, w))
    g, wg = t.pooled_weighted_backward(T(keys, dev), off, T(w, dev), T(bg, dev))
    assert np.array_equal(g.cpu().numpy(), w[:, None] * bg[bag_of_positions(clamped)])
    ref, tol = weight_grads_ref(bg, rows, clamped)
    assert np.all(np.abs(wg.cpu().numpy().astype(np.float64) - ref) <= tol)


@pytest.mark.gpu
@pytest.mark.parametrize("opt", ["adagrad", "adam"])
def test_weighted_backward_then_apply_equals_oracle(dev, opt):
    """The step after the backward is exactly apply_*(keys, w_i * G[bag(i)]): with the forward's handles (apply_*_located) and
    probing, both against the oracle on the same grads."""
    from meepoembedding_amd import OPT_ADAGRAD, OPT_ADAM, LookupTable
    rng = np.random.default_rng(4)
    dim, n_keys = 64, 2000
    kind, okind = (OPT_ADAGRAD, oracle.OPT_ADAGRAD) if opt == "adagrad" else (OPT_ADAM, oracle.OPT_ADAM)
    a, b = (LookupTable(4096, dim, device=dev, optimizer=kind, max_batch=1 << 14, initial_accumulator=0.1) for _ in range(2))
    o = oracle.OracleTable(4096, dim, optimizer=okind, initial_accumulator=0.1)
    u = synth.keys_np(46, 0, n_keys)
    rows = rng.standard_normal((n_keys, dim)).astype(np.float32)
    for x in (a, b):
        x.insert(T(u, dev), T(rows, dev))
    o.insert(u, rows)
    for step, lens in ((1, rng.integers(0, 9, 1500)), (2, rng.integers(5, 40, 200))):
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        keys = u[np.minimum(rng.zipf(1.2, off[-1]) - 1, n_keys - 1)].copy()
        keys[3] = synth.keys_np(998, 0, 1)[0]                   # absent: no update
        w = rng.standard_normal(keys.size).astype(np.float32)
        bg = (rng.standard_normal((lens.size, dim)) * 0.05).astype(np.float32)
        loc = torch.empty(keys.size, dtype=torch.int64, device=dev)
        a.find_pooled(T(keys, dev), T(off, dev), weights=T(w, dev), located=loc)
        ga, _ = a.pooled_weighted_backward(T(keys, dev), T(off, dev), T(w, dev), T(bg, dev), located=loc)
        gb, _ = b.pooled_weighted_backward(T(keys, dev), T(off, dev), T(w, dev), T(bg, dev), want_weight_grads=False)
        go = w[:, None] * bg[bag_of_positions(off)]
        if opt == "adagrad":
            a.apply_adagrad(T(keys, dev), ga, lr=0.05, slots=loc); b.apply_adagrad(T(keys, dev), gb, lr=0.05)
            o.apply_adagrad(keys, go, 0.05, 1e-10)
        else:
            a.apply_adam(T(keys, dev), ga, lr=0.01, step=step, slots=loc); b.apply_adam(T(keys, dev), gb, lr=0.01, step=step)
            o.apply_adam(keys, go, 0.01, 0.9, 0.999, 1e-8, step)
        assert a.status() == 0 and b.status() == 0             # the single-table handles were accepted (no stale-handle bit)
    eo = o.export(with_state=True)
    io = np.argsort(eo[0])
    for x in (a, b):
        ex = x.export(with_state=True)
        ix = torch.argsort(ex[0]).cpu()
        for p, z in zip(ex[1:], eo[1:]):
            if p is not None:
                np.testing.assert_allclose(p.cpu()[ix].numpy(), z[io], rtol=RTOL, atol=ATOL)


@pytest.mark.gpu
@pytest.mark.parametrize("grouped,create", [(False, False), (False, True), (True, False), (True, True)])
def test_weighted_bag_layer_trains_like_torch_embedding_bag(dev, grouped, create):
    """DynamicEmbeddingBag(mode='sum') with per_sample_weights == torch.nn.EmbeddingBag(sparse=True) + Adagrad: rows and the grad of
    the weights, over one table and over a TableGroup, with a preloaded vocabulary or one the layer creates (create_missing)."""
    from meepoembedding_amd import INIT_UNIFORM, OPT_ADAGRAD, LookupTable, TableGroup
    torch.manual_seed(5)
    dim, vocab, bpt, steps = 16, 200, 24, 4
    n_tables = 3 if grouped else 1
    tables, refs, opts, univ = [], [], [], []
    for j in range(n_tables):
        t = LookupTable(2048, dim, device=dev, optimizer=OPT_ADAGRAD, max_batch=4096, initial_accumulator=0.1,
                        initializer=INIT_UNIFORM, init_scale=0.5, init_seed=j)
        u = torch.from_numpy(synth.keys_np(300 + j, 0, vocab))
        if create:   # the layer creates every id at its first training forward: the reference starts from the same initial rows
            o = oracle.OracleTable(16, dim, initializer=oracle.INIT_UNIFORM, init_scale=0.5, init_seed=j)
            w0 = torch.from_numpy(np.stack([o.initial_row(int(k)) for k in u]))
        else:
            w0 = torch.rand(vocab, dim) - 0.5
            t.insert(u.to(dev), w0.to(dev))
        ref = torch.nn.EmbeddingBag(vocab, dim, mode="sum", sparse=True)
        with torch.no_grad():
            ref.weight.copy_(w0)
        tables.append(t); refs.append(ref); univ.append(u)
        opts.append(torch.optim.Adagrad(ref.parameters(), lr=0.05, eps=1e-10, initial_accumulator_value=0.1))
    layer = DynamicEmbeddingBag(TableGroup(tables, max_apply_batch=4096) if grouped else tables[0], mode="sum", lr=0.05, eps=1e-10,
                                create_missing=create).to(dev)
    head = torch.randn(dim, 1) * 0.1
    seen = [set() for _ in range(n_tables)]
    for s in range(steps):
        lens = torch.randint(0, 9, (n_tables * bpt,))
        lens[1] = 20                                            # a long bag: the wave-shared path
        off = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(lens, 0)])
        ids = [torch.randint(0, vocab, (int(lens[j * bpt:(j + 1) * bpt].sum()),)) for j in range(n_tables)]
        psw = torch.randn(int(lens.sum()))
        target = torch.randn(n_tables * bpt, 1)
        for o in opts:
            o.zero_grad()
        wr = psw.clone().requires_grad_()
        pooled = [refs[j](ids[j], off[j * bpt:(j + 1) * bpt] - off[j * bpt], per_sample_weights=wr[off[j * bpt]:off[(j + 1) * bpt]])
                  for j in range(n_tables)]
        ((torch.cat(pooled) @ head - target) ** 2).mean().backward()
        for o in opts:
            o.step()
        keys = torch.cat([univ[j][ids[j]] for j in range(n_tables)]).to(dev)
        wl = psw.to(dev).requires_grad_()
        ((layer(keys, off.to(dev), per_sample_weights=wl) @ head.to(dev) - target.to(dev)) ** 2).mean().backward()
        torch.testing.assert_close(wl.grad.cpu(), wr.grad, rtol=1e-5, atol=1e-7)
        for j in range(n_tables):
            seen[j].update(ids[j].tolist())
    for j in range(n_tables):
        idx = torch.tensor(sorted(seen[j]))
        got, found = tables[j].find(univ[j][idx].to(dev))
        assert bool(found.all())
        np.testing.assert_allclose(got.cpu().numpy(), refs[j].weight.detach()[idx].numpy(), rtol=2e-5, atol=1e-6)


@pytest.mark.gpu
def test_weighted_step_is_graph_capturable(dev):
    """Weighted forward (with handles) + backward (with weight grads) + apply_adagrad_located capture into a hipGraph and replay
    with the results of an eager twin."""
    from meepoembedding_amd import OPT_ADAGRAD, LookupTable
    rng = np.random.default_rng(78)
    dim = 64
    a, b = (LookupTable(4096, dim, device=dev, optimizer=OPT_ADAGRAD, max_batch=8192, initial_accumulator=0.1) for _ in range(2))
    u = synth.keys_np(131, 0, 1500)
    rows = T(rng.standard_normal((1500, dim)).astype(np.float32), dev)
    a.insert(T(u, dev), rows); b.insert(T(u, dev), rows)
    lens = np.concatenate([rng.integers(0, 9, 150), [30, 17]])
    off = T(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), dev)
    n = int(lens.sum())
    keys = T(u[rng.integers(0, 1500, n)], dev)
    w = T(rng.standard_normal(n).astype(np.float32), dev)
    bg = T((rng.standard_normal((lens.size, dim)) * 0.05).astype(np.float32), dev)

    def bufs():
        return (torch.empty((lens.size, dim), device=dev), torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.int64, device=dev),
                torch.empty((n, dim), device=dev), torch.empty(n, device=dev))

    def step(t, out, found, loc, grads, wg):
        t.find_pooled(keys, off, out=out, found=found, weights=w, located=loc)
        t.pooled_weighted_backward(keys, off, w, bg, located=loc, grads=grads, weight_grads=wg)
        t.apply_adagrad(keys, grads, lr=0.05, slots=loc)

    ba, bb = bufs(), bufs()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(a, *ba)
    for _ in range(3):
        step(b, *bb)
        graph.replay()
        torch.cuda.synchronize()
        for j in (0, 1, 3, 4):   # out, found, grads, weight grads (the handles name slots: two tables place their keys differently)
            assert torch.equal(ba[j], bb[j])
        assert bool((ba[2] >= 0).all())
    assert torch.equal(a.find(T(u, dev))[0], b.find(T(u, dev))[0])
