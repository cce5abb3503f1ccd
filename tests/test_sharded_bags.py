"""Embedding bags on sharded tables (SPEC.md §5 "Pooled lookups"): mee_bag_runs / mee_run_offsets / mee_combine_bag_runs, Router's methods over them,
ShardedLookupTable.find_pooled / apply_*(grad_index=) / traffic(), and DynamicEmbeddingBag over a sharded table.

The yardstick of every pooled result is `ref_pooled` below, numpy float32 adds one at a time: per bag, for every owner rank p in rank order the rows of
the bag's positions owned by p added up in batch order (first row copied), then those partial rows added up in rank order (first one copied), then the
division by float32(length) for "mean".  The comparison is on the raw bits; a bf16 result is compared with torch's rounding of that fp32 reference."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist

import oracle
from _apply_cases import assert_bits_equal_nan_aware
from meepoembedding_amd import _lib, synth
from meepoembedding_amd.sharded import ShardedLookupTable
from test_sharded_bf16 import _launch, assert_bf16_of

BF16 = torch.bfloat16
NKEYS, BATCH, DEFAULT = 6000, 4000, 0.1
LENGTHS = (0, 0, 1, 2, 3, 7, 40)
NEW_SYMBOLS = ("mee_bag_runs", "mee_run_offsets", "mee_combine_bag_runs")


# ---- the fixture and the reference model (numpy only) ---------------------------------------------------------------------------
def make_batch(seed: int, G: int):
    """-> (keys [n ~ 4000] int64, bag_offsets [n_bags + 1] int64).  Keys drawn from the NKEYS stored ones, ~5 % absent, both reserved keys, duplicates
    inside and across bags.  Bag lengths from LENGTHS plus one bag of 1500; a leading and a trailing empty bag, two consecutive empty bags in the
    middle, one bag whose keys all have ONE owner and one bag that SKIPS an owner (under G shards; picked with oracle.hash_batch)."""
    rng = np.random.default_rng(seed)
    stored = synth.keys_np(1, 0, NKEYS)
    owner = oracle.hash_batch(stored, 1, G)[2]
    bags = []
    while sum(l for l, _ in bags) < BATCH - 1500 - 47:
        bags.append((int(rng.choice(LENGTHS)), "plain"))
    bags.insert(len(bags) // 2, (0, "plain"))
    bags.insert(len(bags) // 2, (0, "plain"))                    # two consecutive empty bags in the middle
    bags.insert(len(bags) // 3, (1500, "plain"))
    bags.insert(len(bags) // 4, (7, "one"))
    bags.insert(2 * len(bags) // 3, (40, "skip"))
    bags = [(0, "plain")] + bags + [(0, "plain")]               # a leading and a trailing empty bag
    keys, plain_pos, at = [], [], 0
    for l, kind in bags:
        if kind == "one":
            k = rng.choice(stored[owner == G - 1], l)
        elif kind == "skip" and G > 1:
            k = rng.choice(stored[owner != 1], l)
        else:
            k = stored[rng.integers(0, NKEYS, l)]
            plain_pos.extend(range(at, at + l))
        keys.append(k)
        at += l
    keys = np.concatenate(keys).astype(np.int64)
    lens = np.array([l for l, _ in bags], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(lens)])
    forty = [b for b, (l, kind) in enumerate(bags) if l == 40 and kind == "plain"]
    keys[off[forty[0]] + 1] = keys[off[forty[0]]]               # a duplicate inside a bag
    keys[off[forty[1]] + 5] = keys[off[forty[0]]]               # ... and across bags
    plain_pos = np.setdiff1d(np.array(plain_pos), [off[forty[0]], off[forty[0]] + 1, off[forty[1]] + 5])
    n_absent = len(keys) // 20
    pick = rng.choice(plain_pos, n_absent + 2, replace=False)
    keys[pick[:n_absent]] = synth.keys_np(9, seed * 1000, n_absent)
    keys[pick[n_absent]], keys[pick[n_absent + 1]] = oracle.EMPTY_KEY, oracle.EMPTY_KEY + 1
    return keys, off


def ones_batch(seed: int, n: int = 1500):
    """every bag has length 1: as many runs as keys, the worst case"""
    rng = np.random.default_rng(seed)
    return synth.keys_np(1, 0, NKEYS)[rng.integers(0, NKEYS, n)], np.arange(n + 1, dtype=np.int64)


def seq_pool(rows: np.ndarray, off: np.ndarray) -> np.ndarray:
    """per bag: the first row copied, every further row added in float32, in position order; an empty bag is zeros"""
    lens = off[1:] - off[:-1]
    out = np.zeros((lens.size, rows.shape[1]), dtype=np.float32)
    for l in range(int(lens.max()) if lens.size else 0):
        m = lens > l
        r = rows[off[:-1][m] + l]
        out[m] = r if l == 0 else (out[m] + r).astype(np.float32)
    return out


def ref_pooled(rows: np.ndarray, owner: np.ndarray, off: np.ndarray, G: int, mode: str) -> np.ndarray:
    lens = off[1:] - off[:-1]
    n_bags = lens.size
    bag_of = np.repeat(np.arange(n_bags), lens)
    out = np.zeros((n_bags, rows.shape[1]), dtype=np.float32)
    seen = np.zeros(n_bags, dtype=bool)
    for p in range(G):
        sel = np.flatnonzero(owner == p)                             # batch order
        cnt = np.bincount(bag_of[sel], minlength=n_bags)
        part = seq_pool(rows[sel], np.concatenate([[0], np.cumsum(cnt)]))
        has = cnt > 0
        out[has & ~seen] = part[has & ~seen]
        out[has & seen] = (out[has & seen] + part[has & seen]).astype(np.float32)
        seen |= has
    if mode == "mean":
        nz = lens > 0
        out[nz] = (out[nz] / lens[nz, None].astype(np.float32)).astype(np.float32)
    return out


def np_runs(keys: np.ndarray, off: np.ndarray, G: int):
    """-> (perm, counts, run_bag, run_len, run_counts) of the stable partition of keys under G shards"""
    _, counts, perm = oracle.partition(keys, G)
    lens = off[1:] - off[:-1]
    bag_of = np.repeat(np.arange(lens.size), lens)
    run_bag, run_len, run_counts, base = [], [], np.zeros(G, dtype=np.int64), 0
    for p in range(G):
        b = bag_of[perm[base:base + counts[p]]]
        base += counts[p]
        if b.size:
            heads = np.flatnonzero(np.concatenate([[True], b[1:] != b[:-1]]))
            run_bag.append(b[heads])
            run_len.append(np.diff(np.concatenate([heads, [b.size]])))
            run_counts[p] = heads.size
    cat = lambda x: np.concatenate(x).astype(np.int64) if x else np.zeros(0, dtype=np.int64)
    return perm, counts, cat(run_bag), cat(run_len), run_counts


def oracle_table(dim: int, optimizer=oracle.OPT_NONE):
    o = oracle.OracleTable(16384, dim, optimizer=optimizer, default_value=DEFAULT, initial_accumulator=0.1, initializer=oracle.INIT_UNIFORM,
                           init_scale=0.05, init_seed=7)
    k = synth.keys_np(1, 0, NKEYS)
    o.insert(k, synth.rows_np(k, dim, 2))
    return o


def same_bits(got: np.ndarray, ref: np.ndarray, what=""):
    assert got.dtype == ref.dtype == np.float32 and got.shape == ref.shape, (what, got.dtype, got.shape, ref.shape)
    bad = int((got.view(np.int32) != ref.view(np.int32)).sum())
    assert bad == 0, f"{what}: {bad} of {got.size} fp32 patterns differ, max |diff| {np.abs(got - ref).max():.3g}"


# ---- CPU ------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_declared_exported_and_prototyped(built):
    from test_abi_load import _declared
    names = _declared()
    L = C.CDLL(_lib.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s in names and s in _lib.PROTOTYPES and hasattr(L, s), s
    assert _lib.lib().mee_abi_version() == 2     # additive: the ABI version stays
    from meepoembedding_amd import Router
    for m in ("bag_runs", "run_offsets", "combine_bag_runs"):
        assert callable(getattr(Router, m))


def test_null_router_or_arguments_are_errors_not_faults(built):
    L = _lib.lib()
    buf = (C.c_uint64 * 8)()
    assert L.mee_bag_runs(None, None, None, 0, None, 0, None, None, None, None) == _lib.ERR_INVALID_ARG
    assert L.mee_bag_runs(None, buf, buf, 4, buf, 1, buf, buf, buf, None) == _lib.ERR_INVALID_ARG
    assert L.mee_run_offsets(None, buf, 2, buf, None, 0, None) == _lib.ERR_INVALID_ARG
    assert L.mee_run_offsets(None, None, 0, None, None, 0, None) == _lib.ERR_INVALID_ARG
    assert L.mee_combine_bag_runs(None, buf, buf, buf, 1, buf, 1, 16, 0, buf, _lib.DTYPE_F32, None) == _lib.ERR_INVALID_ARG
    assert L.mee_combine_bag_runs(None, None, None, None, 0, None, 0, 16, 0, None, _lib.DTYPE_BF16, None) == _lib.ERR_INVALID_ARG
    assert b"null argument" in L.mee_last_error()


@pytest.mark.parametrize("G", [1, 2, 3, 8])
def test_reference_model_on_the_fixture(G):
    """the model the GPU results are compared with: within the recursive-summation bound of the exact sum, and at one shard the plain position-order sum"""
    dim = 16
    keys, off = make_batch(11, G)
    lens = off[1:] - off[:-1]
    assert abs(keys.size - BATCH) < 100 and lens[0] == 0 and lens[-1] == 0 and 1500 in lens and set(lens) <= set(LENGTHS) | {1500}
    assert np.any((lens[:-1] == 0) & (lens[1:] == 0) & (np.arange(lens.size - 1) > 1) & (np.arange(lens.size - 1) < lens.size - 3))
    owner = oracle.hash_batch(keys, 1, G)[2]
    per_bag = [set(owner[off[b]:off[b + 1]]) for b in range(lens.size) if lens[b] >= 7]
    assert any(len(s) == 1 for s in per_bag)
    if G > 1:
        assert any(1 < len(s) < G or (G == 2 and s == {0}) for s in per_bag)        # a bag that skips an owner
    assert np.unique(keys).size < keys.size and (keys == oracle.EMPTY_KEY).sum() == 1 and (keys == oracle.EMPTY_KEY + 1).sum() == 1
    rows, found = oracle_table(dim).find(keys)
    assert 0.03 < 1 - found.mean() < 0.08
    ref = ref_pooled(rows, owner, off, G, "sum")
    bag_of = np.repeat(np.arange(lens.size), lens)
    exact = np.zeros(ref.shape, dtype=np.float64)
    mag = np.zeros(ref.shape, dtype=np.float64)
    np.add.at(exact, bag_of, rows.astype(np.float64))
    np.add.at(mag, bag_of, np.abs(rows.astype(np.float64)))
    # L - 1 additions, each within 2^-24 relative of a partial sum that is itself at most sum|row_i| (1 + (L - 1) 2^-24): the standard bound, first order
    assert np.all(np.abs(ref - exact) <= lens[:, None] * 2.0 ** -24 * mag)
    assert np.all(ref[lens == 0] == 0)
    mean = ref_pooled(rows, owner, off, G, "mean")
    nz = lens > 0
    same_bits(mean[nz], (ref[nz] / lens[nz, None].astype(np.float32)).astype(np.float32))
    if G == 1:
        same_bits(ref, oracle.pool_rows(rows, off, "sum"), "one shard = the position-order sum")
        same_bits(mean, oracle.pool_rows(rows, off, "mean"))
    perm, counts, run_bag, run_len, run_counts = np_runs(keys, off, G)
    assert run_len.sum() == keys.size and run_counts.sum() == run_bag.size
    assert run_bag.size == len({(b, p) for b, p in zip(bag_of, owner)})       # one run per (bag, owner) pair


def _cpu_rank(rank, world, port, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        from _cpu_backend import CpuRouter, CpuTable
        dist.init_process_group("gloo", rank=rank, world_size=world)
        dim = 16
        sh = ShardedLookupTable(CpuTable(8192, dim), CpuRouter(world))
        assert sh.traffic() == (0, 0)
        k = synth.keys_np(1, 0, NKEYS)
        sh.insert(torch.from_numpy(k[rank::world]), torch.from_numpy(synth.rows_np(k[rank::world], dim, 2)))
        keys, off = make_batch(20 + rank, world)
        kt, ot = torch.from_numpy(keys), torch.from_numpy(off)
        # a shard without find_pooled (and a router without the run kernels): refused on every rank before anything is exchanged
        t0 = sh.traffic()
        with pytest.raises(ValueError):
            sh.find_pooled(kt, ot)
        with pytest.raises(ValueError):
            sh.find_pooled(kt, ot, out_dtype=torch.float16)
        bag_of = torch.repeat_interleave(torch.arange(off.size - 1), torch.from_numpy(off[1:] - off[:-1]))
        grads = torch.zeros(off.size - 1, dim)
        for f, kw in ((sh.apply_adagrad, {}), (sh.apply_adam, {})):
            with pytest.raises(ValueError):
                f(kt, grads, 0.01, dedup=True, grad_index=bag_of, **kw)
            with pytest.raises(ValueError):                                # not the pooled backward's convention: decreasing
                f(kt, grads, 0.01, grad_index=bag_of.flip(0), **kw)
        assert sh.traffic() == t0
        # traffic() of a plain find: 8 B per key out, 4 dim + 1 B per key in, and the counts
        owner = oracle.hash_batch(keys, 1, world)[2]
        to = np.bincount(owner, minlength=world)
        every = [None] * world
        dist.all_gather_object(every, to.tolist())
        k_out = int(to.sum() - to[rank])
        k_in = int(sum(every[s][rank] for s in range(world) if s != rank))
        sh.find(kt)
        t1 = sh.traffic()
        d = (t1[0] - t0[0], t1[1] - t0[1])
        assert d == (8 * k_out + (4 * dim + 1) * k_in + 8 * (world - 1), 8 * k_in + (4 * dim + 1) * k_out + 8 * (world - 1)), (d, k_out, k_in)
        q.put((rank, d))
        dist.barrier()
        dist.destroy_process_group()
    except BaseException as e:
        import traceback
        q.put(("error", rank, "".join(traceback.format_exception(type(e), e, e.__traceback__))))
        raise


def test_torch_path_refusals_and_traffic_without_a_gpu(built):
    res = _launch(_cpu_rank, 2, (), first_timeout=120)
    assert sum(r[1][0] for r in res) == sum(r[1][1] for r in res)


# ---- GPU, one process -----------------------------------------------------------------------------------------------------------
def _i64(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(dev)


@pytest.mark.gpu
@pytest.mark.parametrize("G", [1, 2, 3, 8])
def test_router_bag_runs_and_run_offsets_against_numpy(dev, G):
    from meepoembedding_amd import Router
    r = Router(G, 8192, device=dev)
    for name, (keys, off) in {"fixture": make_batch(5, G), "ones": ones_batch(6), "n = 0": (np.zeros(0, dtype=np.int64), np.zeros(4, dtype=np.int64))}.items():
        perm_e, counts_e, bag_e, len_e, rc_e = np_runs(keys, off, G)
        kt, ot = _i64(keys, dev), _i64(off, dev)
        _, counts, perm = r.partition(kt)
        assert np.array_equal(perm.cpu().numpy(), perm_e) and np.array_equal(counts.cpu().numpy(), counts_e), name
        run_bag, run_len, run_counts = r.bag_runs(perm, counts, ot)
        assert run_bag.dtype == run_len.dtype == torch.int32 and run_bag.numel() == run_len.numel() == keys.size
        R = int(run_counts.sum())
        assert np.array_equal(run_counts.cpu().numpy(), rc_e) and R == bag_e.size <= keys.size, name
        assert np.array_equal(run_bag[:R].cpu().numpy(), bag_e) and np.array_equal(run_len[:R].cpu().numpy(), len_e), name
        offsets, rok = r.run_offsets(run_len[:R], keys.size)
        assert offsets.dtype == torch.int64 and np.array_equal(offsets.cpu().numpy(), np.concatenate([[0], np.cumsum(len_e)])), name
        assert np.array_equal(rok.cpu().numpy(), np.repeat(np.arange(R), len_e)), name
        assert r.run_offsets(run_len[:R])[1] is None
    # more runs than one block of the scan holds, with long runs among them; and nothing behind the outputs is touched
    rng = np.random.default_rng(3)
    lens = rng.choice([1, 2, 3, 700], size=5000, p=[0.5, 0.3, 0.19, 0.01]).astype(np.int32)
    n_keys = int(lens.sum())
    rl = torch.from_numpy(lens).to(dev)
    offs = torch.full((lens.size + 3,), -7, dtype=torch.int64, device=dev)
    rok = torch.full((n_keys + 2,), -7, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    _lib.check(_lib.lib().mee_run_offsets(r._h, rl.data_ptr(), lens.size, offs.data_ptr(), rok.data_ptr(), n_keys, st))
    assert np.array_equal(offs.cpu().numpy(), np.concatenate([[0], np.cumsum(lens.astype(np.int64)), [-7, -7]]))
    assert np.array_equal(rok.cpu().numpy(), np.concatenate([np.repeat(np.arange(lens.size), lens), [-7, -7]]))
    keys, off = make_batch(5, G)
    perm_e, counts_e, bag_e, len_e, rc_e = np_runs(keys, off, G)
    n, R = keys.size, bag_e.size
    rb = torch.full((n + 2,), -7, dtype=torch.int32, device=dev)
    rn = torch.full((n + 2,), -7, dtype=torch.int32, device=dev)
    rc = torch.full((G + 2,), -7, dtype=torch.int64, device=dev)
    pt, ct, ot = _i64(perm_e, dev), _i64(counts_e, dev), _i64(off, dev)
    _lib.check(_lib.lib().mee_bag_runs(r._h, pt.data_ptr(), ct.data_ptr(), n, ot.data_ptr(), off.size - 1, rb.data_ptr(), rn.data_ptr(), rc.data_ptr(), st))
    assert np.array_equal(rb[:R].cpu().numpy(), bag_e) and np.array_equal(rn[:R].cpu().numpy(), len_e) and np.array_equal(rc[:G].cpu().numpy(), rc_e)
    assert bool((rb[R:] == -7).all()) and bool((rn[R:] == -7).all()) and bool((rc[G:] == -7).all())
    # arguments refused before any launch
    L = _lib.lib()
    assert L.mee_bag_runs(r._h, rb.data_ptr(), rc.data_ptr(), 8193, offs.data_ptr(), 4, rb.data_ptr(), rn.data_ptr(), rc.data_ptr(), st) == _lib.ERR_BATCH_TOO_LARGE
    assert L.mee_bag_runs(r._h, rb.data_ptr(), rc.data_ptr(), 5, offs.data_ptr(), 0, rb.data_ptr(), rn.data_ptr(), rc.data_ptr(), st) == _lib.ERR_INVALID_ARG
    assert L.mee_bag_runs(r._h, None, rc.data_ptr(), 5, offs.data_ptr(), 2, rb.data_ptr(), rn.data_ptr(), rc.data_ptr(), st) == _lib.ERR_INVALID_ARG
    assert L.mee_run_offsets(r._h, None, 5, offs.data_ptr(), None, 0, st) == _lib.ERR_INVALID_ARG
    f = torch.zeros(64, device=dev)
    assert L.mee_combine_bag_runs(r._h, f.data_ptr(), rb.data_ptr(), rc.data_ptr(), 1, offs.data_ptr(), 1, 6, 0, f.data_ptr(), _lib.DTYPE_F32, st) == _lib.ERR_INVALID_ARG
    assert L.mee_combine_bag_runs(r._h, f.data_ptr(), rb.data_ptr(), rc.data_ptr(), 1, offs.data_ptr(), 1, 16, 2, f.data_ptr(), _lib.DTYPE_F32, st) == _lib.ERR_INVALID_ARG
    assert L.mee_combine_bag_runs(r._h, f.data_ptr(), rb.data_ptr(), rc.data_ptr(), 1, offs.data_ptr(), 1, 16, 0, f.data_ptr(), 7, st) == _lib.ERR_INVALID_ARG
    assert L.mee_combine_bag_runs(r._h, f.data_ptr() + 4, rb.data_ptr(), rc.data_ptr(), 1, offs.data_ptr(), 1, 16, 0, f.data_ptr(), _lib.DTYPE_F32, st) == _lib.ERR_INVALID_ARG
    torch.cuda.synchronize(dev)


def emulated_find_pooled(tables, router, kt, ot, mode, out_dtype, out=None):
    """the exchange in one process: tables[p] is owner p's shard; what crosses the link in ShardedLookupTable.find_pooled is sliced and concatenated here"""
    G = len(tables)
    send, counts, perm = router.partition(kt)
    run_bag, run_len, run_counts = router.bag_runs(perm, counts, ot)
    c, rc = counts.tolist(), run_counts.tolist()
    parts, founds, kb, rb = [], [], 0, 0
    for p in range(G):
        offsets, _ = router.run_offsets(run_len[rb:rb + rc[p]])
        part, f = tables[p].find_pooled(send[kb:kb + c[p]], offsets, "sum")
        parts.append(part); founds.append(f)
        kb += c[p]; rb += rc[p]
    out = router.combine_bag_runs(torch.cat(parts), run_bag[:rb], run_counts, ot, mode, out=out, out_dtype=out_dtype)
    return out, router.scatter_rows(torch.cat(founds), perm)


def _shards(G, dim, dev):
    from meepoembedding_amd import LookupTable
    k = synth.keys_np(1, 0, NKEYS)
    rows = synth.rows_np(k, dim, 2)
    owner = oracle.hash_batch(k, 1, G)[2]
    tables = []
    for p in range(G):
        t = LookupTable(16384, dim, device=dev, max_batch=8192, default_value=DEFAULT)
        t.insert(_i64(k[owner == p], dev), torch.from_numpy(rows[owner == p]).to(dev))
        tables.append(t)
    return tables


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [4, 16, 64, 100, 260])
@pytest.mark.parametrize("G", [2, 3, 8])
def test_emulated_exchange_against_the_reference(dev, G, dim):
    from meepoembedding_amd import Router
    tables, router = _shards(G, dim, dev), Router(G, 8192, device=dev)
    o = oracle_table(dim)
    for name, (keys, off) in {"fixture": make_batch(7, G), "ones": ones_batch(8)}.items():
        rows, found = o.find(keys)
        owner = oracle.hash_batch(keys, 1, G)[2]
        kt, ot = _i64(keys, dev), _i64(off, dev)
        for mode in ("sum", "mean"):
            ref = ref_pooled(rows, owner, off, G, mode)
            out, f = emulated_find_pooled(tables, router, kt, ot, mode, torch.float32)
            same_bits(out.cpu().numpy(), ref, f"{name} G={G} dim={dim} {mode}")
            assert np.array_equal(f.cpu().numpy(), found)
            o16, _ = emulated_find_pooled(tables, router, kt, ot, mode, BF16)
            assert_bf16_of(o16, torch.from_numpy(ref), f"{name} G={G} dim={dim} {mode} bf16")
    # a batch without keys: every bag is empty
    z, _ = emulated_find_pooled(tables, router, _i64([], dev), _i64([0, 0, 0], dev), "mean", torch.float32)
    assert z.shape == (2, dim) and bool((z == 0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [16, 64, 100])
def test_one_shard_is_bit_identical_to_find_pooled(dev, dim):
    from meepoembedding_amd import Router
    tables, router = _shards(1, dim, dev), Router(1, 8192, device=dev)
    keys, off = make_batch(9, 1)
    kt, ot = _i64(keys, dev), _i64(off, dev)
    n_bags = off.size - 1
    for mode in ("sum", "mean"):
        e32, ef = tables[0].find_pooled(kt, ot, mode)
        e16, _ = tables[0].find_pooled(kt, ot, mode, out_dtype=BF16)
        b32 = torch.full((n_bags + 2, dim), 7.5, dtype=torch.float32, device=dev)
        b16 = torch.full((n_bags + 2, dim), 7.5, dtype=BF16, device=dev)
        o32, f = emulated_find_pooled(tables, router, kt, ot, mode, torch.float32, out=b32[:n_bags])
        o16, _ = emulated_find_pooled(tables, router, kt, ot, mode, BF16, out=b16[:n_bags])
        assert_bits_equal_nan_aware(o32.cpu().numpy(), e32.cpu().numpy(), mode)
        assert torch.equal(f, ef), mode
        assert torch.equal(o16.view(torch.int16), e16.view(torch.int16)), mode
        assert bool((b32[n_bags:] == 7.5).all()) and bool((b16[n_bags:] == 7.5).all())     # nothing behind the outputs is touched


# ---- GPU, ranks spawned on one GPU ----------------------------------------------------------------------------------------------
def _export_sorted(sh):
    e = sh.export_local(with_state=True)
    i = torch.argsort(e[0])
    return [e[0][i].cpu().numpy()] + [x[i].cpu().numpy() for x in e[1:] if x is not None]


def _same_tables(a, b, what):
    ea, eb = _export_sorted(a), _export_sorted(b)
    assert np.array_equal(ea[0], eb[0]), what
    for x, y in zip(ea[1:], eb[1:]):
        same_bits(x, y, what)


def _gpu_rank(rank, world, port, q, backend, dim):
    try:
        _gpu_rank_body(rank, world, port, q, backend, dim)
    except BaseException as e:   # report at once: the parent must not sit out its queue timeout
        import traceback
        q.put(("error", rank, "".join(traceback.format_exception(type(e), e, e.__traceback__))))
        raise


def _gpu_rank_body(rank, world, port, q, backend, dim):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    from meepoembedding_amd import INIT_UNIFORM, OPT_ADAGRAD, OPT_ADAM, LookupTable, Router
    from meepoembedding_amd.nn import DynamicEmbeddingBag
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        stored = synth.keys_np(1, 0, NKEYS)
        stored_rows = synth.rows_np(stored, dim, 2)

        def make(optimizer=OPT_ADAGRAD):
            local = LookupTable(16384, dim, device=dev, optimizer=optimizer, initial_accumulator=0.1, max_batch=max(world * (BATCH + 100), 8192), default_value=DEFAULT,
                                initializer=INIT_UNIFORM, init_scale=0.05, init_seed=7)
            sh = ShardedLookupTable(local, Router(world, 8192, device=dev))
            sh.insert(_i64(stored[rank::world], dev), torch.from_numpy(stored_rows[rank::world]).to(dev))
            return sh

        sh = make()
        dist.barrier()
        assert sh.dim == dim and sh.device == dev
        o = oracle_table(dim)
        batches = [make_batch(40 + r, world) for r in range(world)]          # every rank can rebuild every rank's batch
        keys, off = batches[rank]
        lens = off[1:] - off[:-1]
        n_bags = lens.size
        kt, ot = _i64(keys, dev), _i64(off, dev)
        report = {}

        # ---- lookup: sum, mean, bf16; the found mask is sharded find's ----
        _, found_find = sh.find(kt)
        for name, (k_np, o_np) in {"fixture": (keys, off), "ones": ones_batch(60 + rank)}.items():
            rows, found = o.find(k_np)
            owner = oracle.hash_batch(k_np, 1, world)[2]
            k_t, o_t = _i64(k_np, dev), _i64(o_np, dev)
            for mode in ("sum", "mean"):
                ref = ref_pooled(rows, owner, o_np, world, mode)
                out, f = sh.find_pooled(k_t, o_t, mode)
                same_bits(out.cpu().numpy(), ref, f"{name} {mode}")
                assert np.array_equal(f.cpu().numpy(), found)
                o16, f16 = sh.find_pooled(k_t, o_t, mode, out_dtype=BF16)
                assert_bf16_of(o16, torch.from_numpy(ref), f"{name} {mode} bf16")
                assert torch.equal(f16, f)
                if name == "fixture":
                    assert torch.equal(f, found_find)
                if world == 1:
                    e, ef = sh.local.find_pooled(k_t, o_t, mode)
                    assert torch.equal(out.view(torch.int32), e.view(torch.int32)) and torch.equal(f, ef)
        # ---- a rank without keys (n_bags > 0), then without bags, still takes part ----
        k0, o0 = (kt[:0], torch.zeros(4, dtype=torch.int64, device=dev)) if rank == 0 else (kt, ot)
        out, f = sh.find_pooled(k0, o0, "mean")
        if rank == 0:
            assert out.shape == (3, dim) and bool((out == 0).all()) and f.numel() == 0
        else:
            same_bits(out.cpu().numpy(), ref_pooled(o.find(keys)[0], oracle.hash_batch(keys, 1, world)[2], off, world, "mean"), "beside an empty rank")
        out, f = sh.find_pooled(k0, o0[:1] if rank == 0 else o0, "sum", out_dtype=BF16)
        if rank == 0:
            assert out.shape == (0, dim) and out.dtype == BF16 and f.numel() == 0
        with pytest.raises(ValueError):
            sh.find_pooled(kt, ot, "max")
        with pytest.raises(ValueError):
            sh.find_pooled(kt, ot, out_dtype=torch.float16)
        dist.barrier()

        # ---- wire bytes of one pooled lookup and of its backward ----
        bag_of_np = np.repeat(np.arange(n_bags), lens)
        bag_of = _i64(bag_of_np, dev)
        owner = oracle.hash_batch(keys, 1, world)[2]
        k_to = np.bincount(owner, minlength=world)
        r_to = np.bincount(np.array(sorted({(int(p), int(b)) for p, b in zip(owner, bag_of_np)}), dtype=np.int64).reshape(-1, 2)[:, 0], minlength=world)
        every = [None] * world
        dist.all_gather_object(every, (k_to.tolist(), r_to.tolist()))
        k_out, r_out = int(k_to.sum() - k_to[rank]), int(r_to.sum() - r_to[rank])
        k_in = int(sum(every[s][0][rank] for s in range(world) if s != rank))
        r_in = int(sum(every[s][1][rank] for s in range(world) if s != rank))
        wire = make(OPT_ADAGRAD)
        t0 = wire.traffic(); wire.find_pooled(kt, ot, "sum")
        t1 = wire.traffic(); wire.apply_adagrad(kt, torch.zeros(n_bags, dim, device=dev), 0.01, grad_index=bag_of)
        t2 = wire.traffic()
        fwd, bwd = (t1[0] - t0[0], t1[1] - t0[1]), (t2[0] - t1[0], t2[1] - t1[1])
        plain = (8 * k_out + (4 * dim + 1) * k_in, 8 * k_in + (4 * dim + 1) * k_out)
        print(f"[wire] world {world} dim {dim} rank {rank}: k_out {k_out} k_in {k_in} r_out {r_out} r_in {r_in} | pooled lookup sent/recv {fwd} "
              f"backward sent/recv {bwd} | plain find sent/recv {plain} plain backward sent {(8 + 4 * dim) * k_out}", flush=True)
        report["wire"] = dict(k_out=k_out, k_in=k_in, r_out=r_out, r_in=r_in, fwd=fwd, bwd=bwd, plain=plain)
        cnt = 16 * (world - 1)
        assert fwd == (8 * k_out + 4 * r_out + 4 * dim * r_in + k_in + cnt, 8 * k_in + 4 * r_in + 4 * dim * r_out + k_out + cnt), (fwd, k_out, k_in, r_out, r_in)
        assert bwd == (8 * k_out + 4 * r_out + 4 * dim * r_out + cnt, 8 * k_in + 4 * r_in + 4 * dim * r_in + cnt), (bwd, k_out, k_in, r_out, r_in)

        # ---- insert_missing: the owners create the keys inside the pooled lookup ----
        fresh = synth.keys_np(78, rank * 200, 300)                            # the ranks' fresh keys overlap
        mix = np.concatenate([fresh, keys[:200], fresh[:50]])
        mix_off = np.concatenate([[0], np.sort(np.random.default_rng(rank).integers(0, mix.size, 60)), [mix.size]])
        mt, mo = _i64(mix, dev), _i64(mix_off, dev)
        a, b = make(), make()
        dist.barrier()
        oa, fa = a.find_pooled(mt, mo, "sum", insert_missing=True)
        _, fb = b.find_or_insert(mt)
        ob, _ = b.find_pooled(mt, mo, "sum")
        assert torch.equal(fa, fb) and torch.equal(oa.view(torch.int32), ob.view(torch.int32))
        assert a.size() == b.size() > NKEYS
        _same_tables(a, b, "insert_missing")
        dist.barrier()

        # ---- training: two steps of the pooled backward against one oracle table that got every rank's pairs expanded ----
        def bag_grads(r, step):
            return (np.random.default_rng(1000 * step + r).standard_normal((batches[r][1].size - 1, dim)) * 0.02).astype(np.float32)

        def expanded(step):
            ks, gs = [], []
            for r in range(world):
                k_r, o_r = batches[r]
                ks.append(k_r)
                gs.append(bag_grads(r, step)[np.repeat(np.arange(o_r.size - 1), o_r[1:] - o_r[:-1])])
            return np.concatenate(ks), np.concatenate(gs)

        for opt in ("adagrad", "adam"):
            t = make(OPT_ADAGRAD if opt == "adagrad" else OPT_ADAM)
            ot_ = oracle_table(dim, oracle.OPT_ADAGRAD if opt == "adagrad" else oracle.OPT_ADAM)
            dist.barrier()
            apply = t.apply_adagrad if opt == "adagrad" else t.apply_adam
            with pytest.raises(ValueError):
                apply(kt, torch.from_numpy(bag_grads(rank, 1)).to(dev), 0.01, dedup=True, grad_index=bag_of)
            for step in (1, 2):
                g = torch.from_numpy(bag_grads(rank, step)).to(dev)
                ek, eg = expanded(step)
                if opt == "adagrad":
                    t.apply_adagrad(kt, g, 0.01, 1e-10, grad_index=bag_of)
                    ot_.apply_adagrad(ek, eg, 0.01, 1e-10)
                else:
                    t.apply_adam(kt, g, 0.01, 0.9, 0.999, 1e-8, step, grad_index=bag_of)
                    ot_.apply_adam(ek, eg, 0.01, 0.9, 0.999, 1e-8, step)
            got = _export_sorted(t)
            exp = ot_.export(with_state=True)
            mine = oracle.hash_batch(exp[0], 1, world)[2] == rank
            order = np.argsort(exp[0][mine])
            assert np.array_equal(got[0], exp[0][mine][order]), opt
            for x, y in zip(got[1:], [e for e in exp[1:] if e is not None]):
                np.testing.assert_allclose(x, y[mine][order], rtol=1e-6, atol=1e-9, err_msg=opt)     # SPEC.md §4's contract
            dist.barrier()

        # ---- the layer over a sharded table == the manual sequence on a twin, bit for bit ----
        a, b = make(), make()
        dist.barrier()
        layer = DynamicEmbeddingBag(a, mode="sum", optimizer="adagrad", lr=0.05, create_missing=True).to(dev)
        layer.train()
        lk = _i64(np.concatenate([keys, synth.keys_np(79, rank * 50, 80)]), dev)            # with ids the table has not seen
        lo = torch.cat([ot, ot[-1:] + 80])
        l_bag_of = torch.repeat_interleave(torch.arange(lo.numel() - 1, device=dev), lo[1:] - lo[:-1])
        for step in (1, 2):
            w = torch.from_numpy(np.random.default_rng(7 * step + rank).standard_normal((lo.numel() - 1, dim)).astype(np.float32)).to(dev)
            out = layer(lk, lo)
            (out * w).sum().backward()
            mo_, _ = b.find_pooled(lk, lo, "sum", insert_missing=True)
            assert torch.equal(out.detach().view(torch.int32), mo_.view(torch.int32))
            b.apply_adagrad(lk, w, 0.05, 1e-10, grad_index=l_bag_of)
        _same_tables(a, b, "layer")
        assert a.size() == b.size() > NKEYS
        dist.barrier()
        if world == 1:
            assert sh.traffic() == (0, 0)      # one rank keeps every segment for itself
        q.put((rank, report))
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.parametrize("world,dim", [(2, 16), (3, 64), (4, 64), (2, 100)])
def test_sharded_bags_multi_rank_on_one_gpu(dev, world, dim):
    """ShardedLookupTable over gloo (staged through host memory), 2-4 ranks on one GPU: lookup, empty ranks, wire bytes, insert_missing, training, the layer"""
    res = _launch(_gpu_rank, world, ("gloo", dim))
    assert [r[0] for r in res] == list(range(world))
    for kind in ("fwd", "bwd"):      # what all ranks sent is what all ranks received
        assert sum(r[1]["wire"][kind][0] for r in res) == sum(r[1]["wire"][kind][1] for r in res)
    for r in res:
        w = r[1]["wire"]
        print(f"[wire table] world {world} dim {dim} rank {r[0]}: pooled lookup sent {w['fwd'][0]} B, plain find sent {w['plain'][0]} B "
              f"({w['fwd'][0] / w['plain'][0]:.3f}); pooled backward sent {w['bwd'][0]} B, plain {(8 + 4 * dim) * w['k_out']} B")


@pytest.mark.gpu
def test_sharded_bags_rccl_single_gpu(dev):
    """world 1 over real RCCL, as tests/test_sharded.py::test_sharded_rccl_single_gpu"""
    res = _launch(_gpu_rank, 1, ("nccl", 64))
    assert [r[0] for r in res] == [0]
