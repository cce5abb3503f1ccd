"""GPU: the keyed layout of the pooled group lookups (SPEC.md §3 "Keyed output") — [bags_per_table, sum of dims], one row per sample — against the
table-major operators already in the tree, permuted on the host: bit for bit, compared as integer views.  Uniform groups (fp32 rows and bf16 rows), mixed
groups, groups of hot/cold pairs, the step through the emitted index, the layer, the refusals, and one output past the 2^32-element mark.
Inputs come from tests/_pooled_cases.py: its two bag lists (102 short bags, 99 long ones) split over the members, its grid of edge values as rows."""
import numpy as np
import pytest
import torch

from _pooled_cases import N_ROWS, edge_rows, exact_bag_grads, grid_case, stored_keys

BF16 = torch.bfloat16
SENT = 12345.0        # fills every output buffer before a launch: what is not written keeps it
SENT_I = 0x5A5A5A5A
GIB = 1 << 30


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def bits(t):
    """a tensor as integers: equality of these is equality bit for bit (NaN payloads and the sign of a zero included)"""
    t = t.contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def permuted(ref, n_tables):
    """the table-major [T * B, dim] block as the keyed [B, T * dim] one, on the host"""
    r = ref.cpu()
    return r.view(n_tables, -1, r.shape[1]).transpose(0, 1).reshape(-1, n_tables * r.shape[1])


HEAD = 3   # key positions in front of the first bag: no bag covers them


def edge_batch(c):
    """the case's keys behind HEAD keys that no bag covers, and its offsets with one offset past n and one decreasing pair (bag 50 becomes empty, bag 51
    reaches back into bag 49) -> (keys, offsets)"""
    off = c.off + HEAD
    off[-1] = off[-1] + 5
    assert off[50] > HEAD + 2
    off[51] = off[50] - 1
    return np.concatenate([c.keys[5:5 + HEAD], c.keys]), off


def coverage(off, n, n_tables):
    """-> (how many bags cover every position, the keyed step index of a position's last covering bag), spans clamped as the walk clamps them"""
    B = (off.size - 1) // n_tables
    cover, val = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for b in range(off.size - 1):
        e = min(int(off[b + 1]), n)
        s = min(int(off[b]), e)
        cover[s:e] += 1
        val[s:e] = (b % B) * n_tables + b // B
    return cover, val


def framed(B, width, stride, dtype, dev):
    """a sentinel-filled buffer with one row in front of and one behind the [B, width] view (row stride `stride`) a keyed launch writes"""
    big = torch.full(((B + 2) * stride,), SENT, dtype=dtype, device=dev)
    return big, big[stride:stride + B * stride].view(B, stride)[:, :width]


def assert_frame_intact(big, B, width, stride):
    rows = big.view(B + 2, stride)
    assert bool((rows[0] == SENT).all()) and bool((rows[-1] == SENT).all()), "a row outside the block was written"
    assert bool((rows[1:-1, width:] == SENT).all()), "a gap column was written"


# ---- uniform groups ------------------------------------------------------------------------------------------------------------------------
def uniform_members(dev, dim, n_tables=3, opt=0, seed=0, edge=True, **kw):
    """n_tables tables holding the first two thirds of the grid's keys (a third of a batch's keys are absent), every member rows of its own"""
    from meepoembedding_amd import LookupTable
    keys = stored_keys(seed)[:N_ROWS * 2 // 3]
    out = []
    for j in range(n_tables):
        rows = np.roll(edge_rows(dim, N_ROWS, seed), 7 * j, axis=0)[:keys.size] if edge else \
            np.random.default_rng([dim, j, seed]).standard_normal((keys.size, dim)).astype(np.float32)
        t = LookupTable(4096, dim, device=dev, optimizer=opt, max_batch=4096, default_value=0.125 * (j + 1), initial_accumulator=0.1, init_seed=5 + j, **kw)
        t.insert(T(keys, dev), T(rows, dev))
        out.append(t)
    return out


@pytest.fixture(scope="module")
def groups(dev):
    """per dim: (the fp32-row group, its serving copy with bf16 rows), shared by the read-only forward tests"""
    from meepoembedding_amd import TableGroup
    made = {}

    def get(dim):
        if dim not in made:
            g = TableGroup(uniform_members(dev, dim))
            made[dim] = (g, g.serving_copy())
        return made[dim]
    yield get
    for g, s in made.values():
        g.close()
        s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("brows", [False, True], ids=["f32rows", "bf16rows"])
@pytest.mark.parametrize("out_dtype", [torch.float32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("which", ["short", "long"])
@pytest.mark.parametrize("dim", [64, 128, 8])
def test_uniform_forward(dev, groups, dim, which, out_dtype, brows):
    """rows = the permuted table-major rows; found, located = the table-major launch's; step_index = s * T + j on covered positions; every sentinel intact"""
    g = groups(dim)[1 if brows else 0]
    c = grid_case(dim, which, fill=2 / 3)
    nt = 3
    all_keys, off = edge_batch(c)
    n = all_keys.size
    B = (off.size - 1) // nt
    assert (which, B) in (("short", 34), ("long", 33))
    keys, offs = T(all_keys, dev), T(off, dev)
    cover, val = coverage(off, n, nt)
    assert (cover[:HEAD] == 0).all() and (cover[HEAD:] >= 1).all() and (cover == 2).any()
    for mode in ("sum", "mean"):
        for gap in ((0, 12) if (mode == "mean" and which == "short") else (0,)):
            W = nt * dim
            stride = W + gap
            rf = torch.full((n + 8,), 7, dtype=torch.uint8, device=dev)
            rl = torch.full((n + 8,), SENT_I, dtype=torch.int64, device=dev)
            ref, _ = g.find_pooled(keys, offs, mode, found=rf[4:4 + n], located=None if brows else rl[4:4 + n], out_dtype=out_dtype)
            big, out = framed(B, W, stride, out_dtype, dev)
            kf, kl = torch.full_like(rf, 7), torch.full_like(rl, SENT_I)
            ki = torch.full((n + 8,), SENT_I, dtype=torch.int32, device=dev)
            got, _ = g.find_pooled(keys, offs, mode, out=out, found=kf[4:4 + n], located=None if brows else kl[4:4 + n], out_dtype=out_dtype,
                                   layout="keyed", step_index=None if brows else ki[4:4 + n])
            what = f"dim {dim} {which} {mode} stride {stride}"
            assert got.data_ptr() == out.data_ptr() and got.shape == (B, W)
            assert torch.equal(bits(got.cpu()), bits(permuted(ref, nt))), what
            assert_frame_intact(big, B, W, stride)
            assert torch.equal(kf, rf) and torch.equal(kl, rl), what + ": found / located"
            idx = ki.cpu().numpy()
            assert (idx[:4] == SENT_I).all() and (idx[-4:] == SENT_I).all()
            if not brows:
                assert np.array_equal(idx[4:4 + n][cover == 1], val[cover == 1]), what + ": step_index"
                assert (idx[4:4 + n][cover == 0] == SENT_I).all(), what + ": an uncovered position was written"
            else:
                assert (idx == SENT_I).all()
    assert all(t.status() == 0 for t in g.tables)


def step_both_ways(dev, plain, keyed, keys, off, nt, dim_of_grads, mode, opt, steps=2):
    """`plain` is stepped the present way (table-major lookup, bag_of_position, [T * B, dim] gradient), `keyed` through the keyed lookup, its index and
    the [B, T * dim] gradient; -> nothing, the caller compares the tables"""
    n, B = keys.numel(), (off.numel() - 1) // nt
    lens = (off[1:] - off[:-1]).clamp(min=1).to(torch.float32)
    bag_of = torch.repeat_interleave(torch.arange(nt * B, device=dev), off[1:] - off[:-1], output_size=n)
    for s in range(1, steps + 1):
        grads = T(exact_bag_grads(dim_of_grads, nt * B, seed=s), dev)   # non-uniform, exactly summable: duplicates reduce to the same sum in any order
        loc = torch.empty(n, dtype=torch.int64, device=dev)
        plain.find_pooled(keys, off, mode, located=loc)
        gp = grads / lens[:, None] if mode == "mean" else grads
        plain.apply_pooled(keys, off, gp, bag_of, opt, 0.05, step=s, located=loc)
        loc2, idx = torch.empty_like(loc), torch.zeros(n, dtype=torch.int32, device=dev)
        keyed.find_pooled(keys, off, mode, located=loc2, layout="keyed", step_index=idx)
        gk = grads.view(nt, B, -1).transpose(0, 1).contiguous()         # [B, T, dim] = the keyed gradient [B, T * dim]
        if mode == "mean":
            gk = gk / lens.view(nt, B).t()[:, :, None]
        keyed.apply_pooled(keys, off, gk.view(B * nt, -1), idx, opt, 0.05, step=s, located=loc2)


def assert_same_tables(a, b, what=""):
    for j, (x, y) in enumerate(zip(a, b)):
        assert x.size() == y.size() and x.status() == y.status(), f"{what} member {j}: size / status"
        ex = [p.cpu().numpy() for p in x.export(with_state=True) if p is not None]
        ey = [p.cpu().numpy() for p in y.export(with_state=True) if p is not None]
        ix, iy = np.argsort(ex[0]), np.argsort(ey[0])
        assert np.array_equal(ex[0][ix], ey[0][iy]), f"{what} member {j}: keys"
        for p, q in zip(ex[1:], ey[1:]):
            assert np.array_equal(p[ix].view(np.uint32), q[iy].view(np.uint32)), f"{what} member {j}: a plane differs"


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["sum", "mean"])
@pytest.mark.parametrize("opt", ["adagrad", "adam"])
def test_uniform_step(dev, opt, mode):
    from meepoembedding_amd import OPT_ADAGRAD, OPT_ADAM, TableGroup
    kind = OPT_ADAGRAD if opt == "adagrad" else OPT_ADAM
    a, b = uniform_members(dev, 64, opt=kind, edge=False), uniform_members(dev, 64, opt=kind, edge=False)
    ga, gb = TableGroup(a, max_apply_batch=4096), TableGroup(b, max_apply_batch=4096)
    c = grid_case(64, "short", fill=2 / 3)
    step_both_ways(dev, ga, gb, T(c.keys, dev), T(c.off, dev), 3, 64, mode, opt)
    assert_same_tables(a, b, f"{opt} {mode}")
    ga.close()
    gb.close()


# ---- mixed groups --------------------------------------------------------------------------------------------------------------------------
MIXED = {"long": (100, 64, 128), "short": (8, 64, 128, 100, 64, 8)}


def mixed_members(dev, dims, opt=0):
    from meepoembedding_amd import LookupTable
    keys = stored_keys(0)[:N_ROWS * 2 // 3]
    out = []
    for j, d in enumerate(dims):
        rows = np.random.default_rng([d, j]).standard_normal((keys.size, d)).astype(np.float32)
        t = LookupTable(4096, d, device=dev, optimizer=opt, max_batch=4096, default_value=0.125 * (j + 1), initial_accumulator=0.1, init_seed=5 + j)
        t.insert(T(keys, dev), T(rows, dev))
        out.append(t)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("insert_missing", [False, True])
@pytest.mark.parametrize("out_dtype", [torch.float32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("which", ["long", "short"])
def test_mixed_forward(dev, which, out_dtype, insert_missing):
    """keyed == torch.cat(views, dim=1) of a twin's table-major lookup; found the twin's, located the group's own table-major launch's, the bag as step
    index; with insert_missing the twins end alike"""
    from meepoembedding_amd import MixedTableGroup, keyed_layout
    dims = MIXED[which]
    a, b = mixed_members(dev, dims), mixed_members(dev, dims)
    ga, gb = MixedTableGroup(a), MixedTableGroup(b)
    c = grid_case(64, which, fill=2 / 3)
    n, nt = c.keys.size, len(dims)
    B = (c.off.size - 1) // nt
    assert B == {"long": 33, "short": 17}[which]
    keys, offs = T(c.keys, dev), T(c.off, dev)
    cols, W = keyed_layout(dims)
    assert gb.keyed_layout() == (cols, W)
    for mode in ("sum", "mean"):
        rl, kl = torch.full((n,), SENT_I, dtype=torch.int64, device=dev), torch.full((n,), SENT_I, dtype=torch.int64, device=dev)
        views, rf = ga.find_pooled(keys, offs, mode, located=rl, out_dtype=out_dtype, insert_missing=insert_missing)
        stride = W + 12
        big, out = framed(B, W, stride, out_dtype, dev)
        ki = torch.full((n,), SENT_I, dtype=torch.int32, device=dev)
        got, kf = gb.find_pooled(keys, offs, mode, out=out, located=kl, out_dtype=out_dtype, insert_missing=insert_missing, layout="keyed", step_index=ki)
        assert torch.equal(bits(got.cpu()), bits(torch.cat([v.cpu() for v in views], dim=1))), f"{which} {mode}"
        assert_frame_intact(big, B, W, stride)
        assert torch.equal(kf, rf), f"{which} {mode}: found"
        # located: against the SAME group's table-major launch (where a key sits inside its bucket depends on the order in which the insert's tiles
        # claimed slots, so a twin's slots may differ)
        gb.find_pooled(keys, offs, mode, located=rl, out_dtype=out_dtype)
        assert torch.equal(kl, rl), f"{which} {mode}: located"
        assert np.array_equal(ki.cpu().numpy(), np.repeat(np.arange(nt * B), np.diff(c.off)))
    if insert_missing:
        assert_same_tables(a, b, "insert_missing")
    ga.close()
    gb.close()


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["long", "short"])
def test_mixed_keyed_grads(dev, which):
    """mee_mixed_group_keyed_grads == the class-major buffer built from torch.split, from fp32 and bf16 input, SUM and MEAN (a division by the length)"""
    from meepoembedding_amd import MixedTableGroup, _lib, mixed_layout
    from meepoembedding_amd.table import _stream_ptr
    dims = MIXED[which]
    g = MixedTableGroup(mixed_members(dev, dims))
    c = grid_case(64, which, fill=2 / 3)
    nt = len(dims)
    B = (c.off.size - 1) // nt
    W, offs = sum(dims), T(c.off, dev)
    total = mixed_layout(dims, B)[2]
    lens = (offs[1:] - offs[:-1]).clamp(min=1).to(torch.float32)
    for dtype in (torch.float32, BF16):
        stride = W + 12
        src = torch.randn((B, stride), device=dev).to(dtype)
        keyed = src[:, :W]
        for mode in (0, 1):
            want = torch.full((total,), SENT, device=dev)
            for j, (v, piece) in enumerate(zip(g.views(want, B), torch.split(keyed.to(torch.float32), list(dims), dim=1))):
                v.copy_(piece / lens[j * B:(j + 1) * B, None] if mode else piece)
            got = torch.full((total + 8,), SENT, device=dev)
            _lib.check(_lib.lib().mee_mixed_group_keyed_grads(g._h, keyed.data_ptr(), _lib.DTYPE_BF16 if dtype == BF16 else _lib.DTYPE_F32, stride, B,
                                                              offs.data_ptr() if mode else None, mode, got[4:].data_ptr(), _stream_ptr(dev)))
            assert torch.equal(bits(got[4:4 + total]), bits(want)), (which, dtype, mode)
            assert bool((got[:4] == SENT).all()) and bool((got[4 + total:] == SENT).all())
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["sum", "mean"])
@pytest.mark.parametrize("opt", ["adagrad", "adam"])
def test_mixed_step(dev, opt, mode):
    from meepoembedding_amd import OPT_ADAGRAD, OPT_ADAM, MixedTableGroup
    dims = MIXED["short"]
    kind = OPT_ADAGRAD if opt == "adagrad" else OPT_ADAM
    a, b = mixed_members(dev, dims, kind), mixed_members(dev, dims, kind)
    ga, gb = MixedTableGroup(a, max_apply_batch=4096), MixedTableGroup(b, max_apply_batch=4096)
    c = grid_case(64, "short", fill=2 / 3)
    keys, off, nt = T(c.keys, dev), T(c.off, dev), len(dims)
    n, B = keys.numel(), (off.numel() - 1) // nt
    lens = (off[1:] - off[:-1]).clamp(min=1).to(torch.float32)
    bag_of = torch.repeat_interleave(torch.arange(nt * B, device=dev), off[1:] - off[:-1], output_size=n)
    for s in (1, 2):
        per_member = [T(exact_bag_grads(d, B, seed=10 * s + j), dev) for j, d in enumerate(dims)]
        loc = torch.empty(n, dtype=torch.int64, device=dev)
        views, _ = ga.find_pooled(keys, off, mode, located=loc)
        flat = torch.empty_like(views[0]._base if views[0]._base is not None else views[0]).view(-1)
        for j, v in enumerate(ga.views(flat, B)):
            v.copy_(per_member[j] / lens[j * B:(j + 1) * B, None] if mode == "mean" else per_member[j])
        ga.apply_pooled(keys, off, flat, bag_of, opt, 0.05, step=s, located=loc)
        loc2, idx = torch.empty_like(loc), torch.zeros(n, dtype=torch.int32, device=dev)
        gb.find_pooled(keys, off, mode, located=loc2, layout="keyed", step_index=idx)
        gb.apply_pooled(keys, off, torch.cat(per_member, dim=1), idx, opt, 0.05, step=s, located=loc2, layout="keyed", mean_offsets=off if mode == "mean" else None)
    assert_same_tables(a, b, f"mixed {opt} {mode}")
    ga.close()
    gb.close()


# ---- groups of hot/cold pairs ------------------------------------------------------------------------------------------------------------------
def tiered_pairs(dev, dim):
    """3 pairs with both tiers counting hits: a third of the grid's keys in hot, a third in cold (pinned host memory), a third in neither"""
    from meepoembedding_amd import LookupTable, TieredLookupTable, _lib
    keys = stored_keys(0)
    third = N_ROWS // 3
    pairs = []
    for j in range(3):
        rows = np.roll(edge_rows(dim, N_ROWS, 0), 5 * j, axis=0)
        hot = LookupTable(4096, dim, device=dev, max_batch=4096, track_hits=True, default_value=0.25 * (j + 1))
        cold = LookupTable(4096, dim, device=dev, max_batch=4096, track_hits=True, value_memory=_lib.MEM_HOST_PINNED, default_value=-1.0)
        hot.insert(T(keys[:third], dev), T(rows[:third], dev))
        cold.insert(T(keys[third:2 * third], dev), T(rows[third:2 * third], dev))
        pairs.append(TieredLookupTable(hot, cold, hot_key_limit=10 * 4096))
    return pairs


@pytest.mark.gpu
@pytest.mark.parametrize("out_dtype", [torch.float32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("which", ["short", "long"])
def test_tiered_forward(dev, which, out_dtype):
    """rows = the permuted TieredTableGroup.find_pooled of a twin; both tiers' hit counters equal the twin's (the count flags are on in every call)"""
    from meepoembedding_amd import TieredTableGroup
    dim = 64
    pa, pb = tiered_pairs(dev, dim), tiered_pairs(dev, dim)
    ga, gb = TieredTableGroup(pa, sample_every=1), TieredTableGroup(pb, sample_every=1)
    assert ga.policy and gb.policy
    c = grid_case(dim, which, fill=1.0)
    n, nt = c.keys.size, 3
    B = (c.off.size - 1) // nt
    keys, offs = T(c.keys, dev), T(c.off, dev)
    cover, val = coverage(c.off, n, nt)
    for mode in ("sum", "mean"):
        ref, rf = ga.find_pooled(keys, offs, mode, out_dtype=out_dtype)
        W = nt * dim
        big, out = framed(B, W, W + 12, out_dtype, dev)
        ki = torch.full((n,), SENT_I, dtype=torch.int32, device=dev)
        got, kf = gb.find_pooled(keys, offs, mode, out=out, out_dtype=out_dtype, layout="keyed", step_index=ki)
        assert torch.equal(bits(got.cpu()), bits(permuted(ref, nt))), f"{which} {mode}"
        assert_frame_intact(big, B, W, W + 12)
        assert torch.equal(kf, rf)
        assert np.array_equal(ki.cpu().numpy(), val) and (cover == 1).all()
    allk = T(stored_keys(0), dev)
    for x, y in zip(pa, pb):
        hx, hy, cx, cy = x.hot.hits_of(allk), y.hot.hits_of(allk), x.cold.hits_of(allk), y.cold.hits_of(allk)
        assert torch.equal(hx, hy) and torch.equal(cx, cy)
        assert int(hx.sum()) > 0 and int(cx.sum()) > 0
    ga.close()
    gb.close()


# ---- the layer -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["uniform", "mixed"])
@pytest.mark.parametrize("mode", ["sum", "mean"])
def test_layer(dev, kind, mode):
    """DynamicEmbeddingBag(group, layout="keyed", out_dtype=bf16) == the default layer plus a permute on a twin: outputs, and the tables after backward()"""
    from meepoembedding_amd import OPT_ADAGRAD, MixedTableGroup, TableGroup
    from meepoembedding_amd.nn import DynamicEmbeddingBag
    if kind == "uniform":
        dims = (64, 64, 64)
        a, b = uniform_members(dev, 64, opt=OPT_ADAGRAD, edge=False), uniform_members(dev, 64, opt=OPT_ADAGRAD, edge=False)
        ga, gb = TableGroup(a, max_apply_batch=4096), TableGroup(b, max_apply_batch=4096)
    else:
        dims = MIXED["long"]
        a, b = mixed_members(dev, dims, OPT_ADAGRAD), mixed_members(dev, dims, OPT_ADAGRAD)
        ga, gb = MixedTableGroup(a, max_apply_batch=4096), MixedTableGroup(b, max_apply_batch=4096)
    c = grid_case(64, "long", fill=2 / 3)
    keys, off = T(c.keys, dev), T(c.off, dev)
    B = (c.off.size - 1) // 3
    plain = DynamicEmbeddingBag(ga, mode=mode, lr=0.05, out_dtype=BF16, create_missing=True).to(dev)
    keyed = DynamicEmbeddingBag(gb, mode=mode, lr=0.05, out_dtype=BF16, create_missing=True, layout="keyed").to(dev)
    assert keyed.traits.native_keyed
    gk = T(np.concatenate([exact_bag_grads(d, B, seed=j) for j, d in enumerate(dims)], axis=1), dev).to(BF16)   # (exact in bf16: |m| <= 31)
    for _ in range(2):
        po, ko = plain(keys, off), keyed(keys, off)
        want = torch.cat(list(po), dim=1) if kind == "mixed" else po.view(3, B, 64).transpose(0, 1).reshape(B, 192)
        assert ko.dtype == BF16 and ko.shape == (B, sum(dims)) and torch.equal(bits(ko), bits(want))
        ko.backward(gk)
        want.backward(gk)
    assert_same_tables(a, b, f"layer {kind} {mode}")
    ga.close()
    gb.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals(dev):
    """every INVALID_ARG / UNSUPPORTED case of the header: its code, the entry point's name in mee_last_error, nothing written, status() 0"""
    from meepoembedding_amd import MixedTableGroup, TableGroup, _lib
    L, n, B = _lib.lib(), 8, 2
    ts = uniform_members(dev, 64, n_tables=2)
    g = TableGroup(ts)
    serving = g.serving_copy()
    cold = TableGroup(uniform_members(dev, 64, n_tables=2))
    mixed = MixedTableGroup(mixed_members(dev, (8, 64)))
    keys = T(stored_keys(0)[:n], dev)
    off = T(np.array([0, 2, 4, 6, 8], np.int64), dev)
    bufs = {k: torch.full((4096,), 0x5A, dtype=torch.uint8, device=dev) for k in ("out", "found", "located", "index", "grads")}
    p = {k: v.data_ptr() for k, v in bufs.items()}
    INV, UNS = _lib.ERR_INVALID_ARG, _lib.ERR_UNSUPPORTED

    def refused(name, code, *args):
        rc = getattr(L, name)(*args)
        msg = L.mee_last_error().decode()
        assert rc == code and msg.startswith(name + ":"), (name, rc, code, msg)

    def uni(out=p["out"], dt=0, stride=0, located=p["located"], index=p["index"], mode=0, k=keys.data_ptr(), o=off.data_ptr(), h=None, bpt=B):
        return ((g._h if h is None else h), k, n, o, bpt, out, dt, stride, p["found"], located, index, mode, None)
    name = "mee_group_find_pooled_keyed"
    refused(name, INV, *uni(out=None))
    refused(name, INV, *uni(k=None))
    refused(name, INV, *uni(o=None))
    refused(name, INV, *uni(mode=2))
    refused(name, INV, *uni(dt=2))
    refused(name, INV, *uni(stride=124))            # below the width 128
    refused(name, INV, *uni(stride=130))            # no multiple of 4
    refused(name, INV, *uni(out=p["out"] + 8))      # fp32: 16-byte alignment
    refused(name, INV, *uni(out=p["out"] + 4, dt=1))   # bf16: 8-byte alignment
    refused(name, INV, *uni(bpt=1 << 31))           # T * B = 2^32 with a step index
    refused(name, UNS, *uni(h=serving._h, index=None))    # located rows on a bf16-row group
    refused(name, UNS, *uni(h=serving._h, located=None))  # a step index on a bf16-row group
    assert L.mee_group_find_pooled_keyed(*uni(bpt=0)) == 0   # no bags: succeeds, writes nothing
    name = "mee_group_find_pooled_tiered_keyed"

    def tier(out=p["out"], dt=0, stride=0, mode=0, flags=0, hot=g._h, c=cold._h, bpt=B):
        return (hot, c, keys.data_ptr(), n, off.data_ptr(), bpt, out, dt, stride, p["found"], p["index"], mode, flags, None)
    refused(name, INV, *tier(out=None))
    refused(name, INV, *tier(mode=3))
    refused(name, INV, *tier(dt=7))
    refused(name, INV, *tier(stride=64))
    refused(name, INV, *tier(out=p["out"] + 4))
    refused(name, INV, *tier(flags=8))
    refused(name, INV, *tier(c=g._h))               # one group as both tiers, as mee_group_find_pooled_tiered refuses it
    refused(name, INV, *tier(bpt=1 << 31))
    refused(name, UNS, *tier(hot=serving._h))
    assert L.mee_group_find_pooled_tiered_keyed(*tier(bpt=0)) == 0
    name = "mee_mixed_group_find_pooled_keyed"

    def mix(out=p["out"], dt=0, stride=0, mode=0, ins=0, found=p["found"], bpt=B):
        return (mixed._h, keys.data_ptr(), n, off.data_ptr(), bpt, out, dt, stride, found, p["located"], p["index"], mode, ins, None)
    refused(name, INV, *mix(out=None))
    refused(name, INV, *mix(mode=-1))
    refused(name, INV, *mix(dt=2))
    refused(name, INV, *mix(stride=68))             # below the width 72
    refused(name, INV, *mix(stride=74))
    refused(name, INV, *mix(out=p["out"] + 8))
    refused(name, INV, *mix(ins=1, found=None))
    refused(name, INV, *mix(bpt=1 << 31))
    assert L.mee_mixed_group_find_pooled_keyed(*mix(bpt=0)) == 0
    name = "mee_mixed_group_keyed_grads"

    def kg(src=p["grads"], dt=0, stride=0, offs=off.data_ptr(), mode=1, out=p["out"]):
        return (mixed._h, src, dt, stride, B, offs, mode, out, None)
    refused(name, INV, *kg(src=None))
    refused(name, INV, *kg(out=None))
    refused(name, INV, *kg(dt=2))
    refused(name, INV, *kg(stride=70))
    refused(name, INV, *kg(mode=2))
    refused(name, INV, *kg(offs=None))              # MEAN without the offsets
    refused(name, INV, *kg(src=p["grads"] + 4))
    refused("mee_mixed_group_keyed_layout", INV, None, None, None)
    torch.cuda.synchronize(dev)
    for k, v in bufs.items():
        assert bool((v == 0x5A).all()), f"a refused call wrote to `{k}`"
    assert all(t.status() == 0 for t in ts + list(cold.tables) + list(mixed.tables))
    for x in (g, serving, cold, mixed):
        x.close()


# ---- far rows ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("out_dtype", [torch.float32, BF16], ids=["f32", "bf16"])
def test_far_rows(dev, groups, out_dtype):
    """out_row_stride = 2^30 elements, 5 samples: the last sample's row starts at element 2^32 (64-bit row arithmetic).  torch.empty only, never cleared."""
    stride, B, nt, dim = 1 << 30, 5, 3, 64
    need = (4 * stride + nt * dim) * (4 if out_dtype == torch.float32 else 2)
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info(dev)
    if free < need + 8 * GIB:
        pytest.skip(f"needs {need / GIB:.1f} GiB of HBM plus 8 GiB of headroom; {free / GIB:.1f} GiB are free")
    g = groups(dim)[0]
    c = grid_case(dim, "short", fill=2 / 3)
    off = c.off[:nt * B + 1]
    keys, offs = T(c.keys[:off[-1]], dev), T(off, dev)
    ref, _ = g.find_pooled(keys, offs, "mean", out_dtype=out_dtype)
    big = torch.empty(4 * stride + nt * dim, dtype=out_dtype, device=dev)
    out = torch.as_strided(big, (B, nt * dim), (stride, 1))
    got, _ = g.find_pooled(keys, offs, "mean", out=out, out_dtype=out_dtype, layout="keyed")
    assert torch.equal(bits(got.cpu()), bits(permuted(ref, nt)))
    del big, out, got
    torch.cuda.empty_cache()
