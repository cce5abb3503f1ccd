"""optimizer="ftrl" through the nn layers: the gradient autograd hands a layer is read with a hook and fed to tests/_ftrl_ref.py, whose tables
must then equal the library's — within SPEC.md §4's tolerance where a batch has duplicate ids (l1 = 0), bit for bit and with the same set of
exactly-zero elements where it has none (l1 > 0: the threshold is a discontinuity, so only bit-exact cases are compared)."""
import numpy as np
import pytest
import torch

from _ftrl_ref import FtrlRefTable
from meepoembedding_amd import synth

RTOL, ATOL = 1e-6, 1e-9
LR, BETA, L2 = 0.05, 1.0, 0.001
N_KEYS = 400


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def export_sorted(t):
    e = [x.cpu().numpy() for x in t.export(with_state=True) if x is not None]
    order = np.argsort(e[0])
    return [x[order] for x in e]


def member(dev, dim, j, **kw):
    """an FTRL table holding N_KEYS small rows, and its reference"""
    from meepoembedding_amd import OPT_FTRL, LookupTable
    keys = synth.keys_np(80 + j, 0, N_KEYS)
    rows = (synth.rows_np(keys, dim, 2) * 0.05).astype(np.float32)
    t = LookupTable(4096, dim, device=dev, optimizer=OPT_FTRL, max_batch=4096, initial_accumulator=0.1, **kw)
    t.insert(T(keys, dev), T(rows, dev))
    ref = FtrlRefTable(dim, 0.1)
    ref.insert(keys, rows)
    return t, ref, keys


def bags(rng, stored, bags_per_table, dups, max_len=6):
    """bags of 0..max_len ids per member -> (keys, bag offsets); dups: Zipf draws (duplicates inside and across bags), else every id at most once"""
    lens = rng.integers(0, max_len + 1, size=len(stored) * bags_per_table)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    parts = []
    for j, keys in enumerate(stored):
        m = int(off[(j + 1) * bags_per_table] - off[j * bags_per_table])
        parts.append(keys[np.minimum(rng.zipf(1.3, size=m) - 1, N_KEYS - 1)] if dups else keys[rng.permutation(N_KEYS)[:m]])
    return np.concatenate(parts).astype(np.int64), off


def loss_of(dense_in, rng, dev):
    """a small dense head and a squared-error loss, scaled so that a bag's gradient is a few hundredths"""
    w = T(rng.standard_normal((dense_in.shape[1], 4)).astype(np.float32), dev)
    y = T(rng.standard_normal((dense_in.shape[0], 4)).astype(np.float32), dev)
    return ((dense_in @ w * 0.1 - y) ** 2).sum() / dense_in.shape[0]


def compare(tables, refs, l1, what):
    zeros = 0.0
    for j, (t, ref) in enumerate(zip(tables, refs)):
        assert t.status() == 0
        e, r = export_sorted(t), ref.export_sorted()
        assert np.array_equal(e[0], r[0])
        if l1 == 0:
            worst = max(float((np.abs(x - y) / np.maximum(np.abs(y), 1e-30)).max()) for x, y in zip(e[1:], r[1:]))
            print(f"{what} member {j}: max relative difference {worst:.3g}")
            for x, y in zip(e[1:], r[1:]):
                np.testing.assert_allclose(x, y, rtol=RTOL, atol=ATOL)
        else:
            assert np.array_equal(e[1].view(np.uint32) == 0, r[1].view(np.uint32) == 0), f"{what} member {j}: the sets of exactly-zero elements differ"
            for x, y in zip(e[1:], r[1:]):
                assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), f"{what} member {j}: no duplicates in any batch, so every plane is bit-exact"
            zeros = max(zeros, float((e[1].view(np.uint32) == 0).mean()))
        assert float(np.abs(e[2]).max()) > 0, "the layer trained nothing"
    if l1 > 0:
        assert 0.0 < zeros < 1.0, f"{what}: l1 produced {zeros:.0%} zeros — the comparison of the zero sets shows nothing"


@pytest.mark.gpu
@pytest.mark.parametrize("l1", [0.0, 0.02])
def test_bag_layer_over_one_table(dev, l1):
    from meepoembedding_amd.nn import DynamicEmbeddingBag
    dim, B = 24, 48
    t, ref, keys = member(dev, dim, 0)
    layer = DynamicEmbeddingBag(t, optimizer="ftrl", lr=LR, l1=l1, l2=L2).to(dev).train()
    assert layer.eps == 1.0 and (layer.l1, layer.l2) == (l1, L2)
    rng = np.random.default_rng(5)
    for _ in range(4):
        k, off = bags(rng, [keys], B, dups=(l1 == 0))
        got = []
        out = layer(T(k, dev), T(off, dev))
        out.register_hook(lambda g: got.append(g.detach().clone()))
        loss_of(out, rng, dev).backward()
        bag_of = np.repeat(np.arange(B), np.diff(off))
        ref.apply(k, got[0].cpu().numpy()[bag_of], LR, BETA, l1, L2)
    compare([t], [ref], l1, "bag layer, one table")


@pytest.mark.gpu
@pytest.mark.parametrize("l1", [0.0, 0.02])
@pytest.mark.parametrize("kind", ["table", "keyed", "mixed", "mixed-keyed"])
def test_bag_layer_over_groups(dev, kind, l1):
    from meepoembedding_amd import MixedTableGroup, TableGroup
    from meepoembedding_amd.nn import DynamicEmbeddingBag
    mixed = kind.startswith("mixed")
    dims, B = ([8, 64, 100] if mixed else [16, 16, 16]), 32
    nt = len(dims)
    made = [member(dev, d, j) for j, d in enumerate(dims)]
    tables, refs, stored = [m[0] for m in made], [m[1] for m in made], [m[2] for m in made]
    group = (MixedTableGroup if mixed else TableGroup)(tables, max_apply_batch=4096)
    layer = DynamicEmbeddingBag(group, optimizer="ftrl", lr=LR, l1=l1, l2=L2, layout="keyed" if kind.endswith("keyed") else "table").to(dev).train()
    rng = np.random.default_rng(6)
    col = np.concatenate([[0], np.cumsum(dims)])
    for _ in range(4):
        k, off = bags(rng, stored, B, dups=(l1 == 0))
        got = {}
        out = layer(T(k, dev), T(off, dev))
        outs = out if isinstance(out, (list, tuple)) else [out]
        for i, o in enumerate(outs):
            o.register_hook(lambda g, i=i: got.__setitem__(i, g.detach().clone()))
        dense = torch.cat(list(outs), dim=1) if kind == "mixed" else out.view(nt, B, -1).transpose(0, 1).reshape(B, -1) if kind == "table" else out
        loss_of(dense, rng, dev).backward()
        bag_of = np.repeat(np.arange(nt * B), np.diff(off))
        for j in range(nt):
            lo, hi = int(off[j * B]), int(off[(j + 1) * B])
            if kind == "table":
                gj = got[0].cpu().numpy()[j * B:(j + 1) * B]
            elif kind == "mixed":
                gj = got[j].cpu().numpy()
            else:   # one [B, sum of dims] block: member j's columns
                gj = got[0].cpu().numpy()[:, col[j]:col[j + 1]]
            refs[j].apply(k[lo:hi], np.ascontiguousarray(gj)[bag_of[lo:hi] - j * B], LR, BETA, l1, L2)
    compare(tables, refs, l1, f"bag layer, {kind} group")
    group.close()


@pytest.mark.gpu
@pytest.mark.parametrize("l1", [0.0, 0.02])
def test_collection_and_sequence_layers(dev, l1):
    from meepoembedding_amd import TableGroup
    from meepoembedding_amd.nn import DynamicEmbeddingCollection, DynamicEmbeddingSequence
    dim, nt = 16, 3
    rng = np.random.default_rng(7)
    # the collection layer: one row per position
    made = [member(dev, dim, j) for j in range(nt)]
    tables, refs, stored = [m[0] for m in made], [m[1] for m in made], [m[2] for m in made]
    group = TableGroup(tables, max_apply_batch=4096)
    layer = DynamicEmbeddingCollection(group, optimizer="ftrl", lr=LR, eps=BETA, l1=l1, l2=L2).to(dev).train()
    for _ in range(4):
        counts = rng.integers(20, 60, size=nt)
        seg = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        k = np.concatenate([stored[j][np.minimum(rng.zipf(1.3, size=c) - 1, N_KEYS - 1)] if l1 == 0 else stored[j][rng.permutation(N_KEYS)[:c]]
                            for j, c in enumerate(counts)])
        got = []
        out = layer(T(k, dev), T(seg, dev))
        out.register_hook(lambda g: got.append(g.detach().clone()))
        loss_of(out, rng, dev).backward()
        g = got[0].cpu().numpy()
        for j in range(nt):
            refs[j].apply(k[seg[j]:seg[j + 1]], g[seg[j]:seg[j + 1]], LR, BETA, l1, L2)
    compare(tables, refs, l1, "collection layer")
    group.close()
    # the sequence layer, keep="last": histories longer than max_len lose their oldest ids, which are neither looked up nor trained
    made = [member(dev, dim, 10 + j) for j in range(nt)]
    tables, refs, stored = [m[0] for m in made], [m[1] for m in made], [m[2] for m in made]
    group = TableGroup(tables, max_apply_batch=4096)
    max_len, B = 5, 16
    layer = DynamicEmbeddingSequence(group, max_len, keep="last", optimizer="ftrl", lr=LR, l1=l1, l2=L2, create_missing=False).to(dev).train()
    for _ in range(4):
        k, off = bags(rng, stored, B, dups=(l1 == 0), max_len=9)
        assert int(np.diff(off).max()) > max_len
        got = []
        padded, lengths = layer(T(k, dev), T(off, dev))
        padded.register_hook(lambda g: got.append(g.detach().clone()))
        loss_of(padded.reshape(nt * B, -1), rng, dev).backward()
        g = got[0].cpu().numpy()
        assert np.array_equal(lengths.cpu().numpy(), np.minimum(np.diff(off), max_len))
        for j in range(nt):
            kk, gg = [], []
            for b in range(j * B, (j + 1) * B):
                lo, hi = int(off[b]), int(off[b + 1])
                lo = max(lo, hi - max_len)
                kk.append(k[lo:hi]); gg.append(g[b, :hi - lo])
            refs[j].apply(np.concatenate(kk), np.concatenate(gg), LR, BETA, l1, L2)
    compare(tables, refs, l1, "sequence layer")
    group.close()


@pytest.mark.gpu
def test_bag_layer_trains_a_hot_cold_pair_like_one_table(dev):
    """DynamicEmbeddingBag over a TieredLookupTable (hot in HBM, cold in pinned host memory) and over ONE table of the union: 6 steps without duplicate
    ids, keys changing tier in between (demote, promote, rebalance: z and n travel with the row): bit-equal outputs and exports"""
    from meepoembedding_amd import OPT_FTRL, LookupTable, TieredLookupTable, _lib
    from meepoembedding_amd.nn import DynamicEmbeddingBag
    dim = 64
    kw = dict(device=dev, optimizer=OPT_FTRL, max_batch=4096, initial_accumulator=0.1, track_hits=True)
    hot, cold = LookupTable(4096, dim, **kw), LookupTable(8192, dim, value_memory=_lib.MEM_HOST_PINNED, **kw)
    one = LookupTable(16384, dim, **kw)
    pair = TieredLookupTable(hot, cold, hot_key_limit=1000)
    universe = synth.keys_np(61, 0, 2000)
    rows = (synth.rows_np(universe, dim, 3) * 0.05).astype(np.float32)
    for s in (slice(0, 1000), slice(1000, 2000)):
        pair.insert(T(universe[s], dev), T(rows[s], dev)); one.insert(T(universe[s], dev), T(rows[s], dev))
    layers = [DynamicEmbeddingBag(t, mode="sum", optimizer="ftrl", lr=LR, l1=0.02, l2=L2).to(dev).train() for t in (pair, one)]
    rng = np.random.default_rng(11)
    lens = [0, 1, 2, 15, 16, 17, 40, 3, 9, 5, 12]
    off = T(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), dev)
    n = int(sum(lens))
    head = T(rng.standard_normal((len(lens), dim)).astype(np.float32) * 0.05, dev)
    moved = 0
    for step in range(6):
        keys = T(universe[rng.permutation(2000)[:n]], dev)
        outs = []
        for layer in layers:
            out = layer(keys, off)
            (out * head).sum().backward()
            outs.append(out.detach())
        assert torch.equal(outs[0], outs[1]), step
        if step == 2:
            p, d = pair.rebalance()
            moved += int(p) + int(d)
        elif step % 2 == 0:
            moved += pair.demote(T(universe[100 * step:100 * step + 150], dev))
        else:
            moved += pair.promote(T(universe[1000 + 100 * step:1000 + 100 * step + 150], dev))
    assert moved > 0 and pair.size() == one.size() == 2000 and hot.size() > 0 and cold.size() > 0 and hot.status() == cold.status() == one.status() == 0
    got, exp = export_sorted(pair), export_sorted(one)
    assert len(got) == len(exp) == 4 and np.array_equal(got[0], exp[0])
    for name, a, b in zip(("rows", "z", "n"), got[1:], exp[1:]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), name
    zeros = float((exp[1].view(np.uint32) == 0).mean())
    assert float(np.abs(exp[2]).max()) > 0 and 0.0 < zeros < 1.0


def test_a_layer_over_a_sharded_table_refuses_ftrl_at_construction(built):
    """the Python sharded classes keep Adagrad and Adam: no apply_ftrl, so the layer says so by name when it is built"""
    from meepoembedding_amd.nn import DynamicEmbeddingBag
    from meepoembedding_amd.sharded import ShardedLookupTable, ShardedTableGroup
    for cls in (ShardedLookupTable, ShardedTableGroup):
        assert not hasattr(cls, "apply_ftrl")
        obj = cls.__new__(cls)
        with pytest.raises(ValueError, match="optimizer='ftrl' needs a table with apply_ftrl.*" + cls.__name__):
            DynamicEmbeddingBag(obj, optimizer="ftrl", l1=0.02)
