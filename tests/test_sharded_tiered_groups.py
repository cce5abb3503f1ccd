"""Sharded collections of hot/cold pairs (SPEC.md §5 "Groups of pairs"): mee_group_find_pooled_tiered_jagged, TieredTableGroup.find_pooled_jagged /
apply_indexed, ShardedTieredTableGroup and the nn layers over it.

The yardsticks are code that is not under test: the pair's own find_pooled and apply_*(grad_index=), TableGroup.find_pooled_jagged,
mee_group_find_pooled_tiered, one LookupTable per member that holds the union of the member's shards and tiers (`full[j]`), and numpy (ref_bags: fp32
adds in rank order, division by float32(length), the bf16 formula of SPEC.md §3).  Every member stores the SAME key values with different rows, so
a bag served by the wrong member gives a wrong row; the hot and the cold default rows differ, so a cold default that shows is caught."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist

import oracle
import test_tiered_groups as ttg
from _apply_cases import exact_grads_np
from meepoembedding_amd import _lib, synth
from test_sharded_bags import _i64, same_bits
from test_sharded_bf16 import _launch
from test_sharded_group_bags import (NpBagRouter, _bag_rows, _emulate_bags, _gpu_find_rows, _reference_step, assert_rows, bag_batch, distinct_batches,
                                     ref_bags, run_counts_of, with_fresh_bags)
from test_sharded_groups import DEFAULT, NK, NpRouter, _emulate, _members, _per_member, _sorted_export, make_batch, stored_keys, with_fresh
from test_tiered_group_find import HOT_DEFAULT, INIT, _cpu_pairs
from test_tiered_groups import LENS_A, LENS_B

BF16 = torch.bfloat16
NEW_SYMBOL = "mee_group_find_pooled_tiered_jagged"
EMPTY_KEY = -(1 << 63)
RECLAIMED_KEY = EMPTY_KEY + 1
ABSENT_KEY = 123456789                               # in no table of this file
CAPS = [(3000, 5000), (6000, 4000), (4500, 3500)]    # requested slots per member (hot, cold): all different, as in test_tiered_groups.py
COLD_DEFAULT = 2.0                                   # a cold table's default row must never show
T3 = 3


# ---- CPU ------------------------------------------------------------------------------------------------------------------------
def test_new_entry_methods_and_class_exist(built):
    """fails on the parent commit: the entry, the two TieredTableGroup methods and the class are this feature"""
    from test_abi_load import _declared
    assert NEW_SYMBOL in _declared() and NEW_SYMBOL in _lib.PROTOTYPES and hasattr(C.CDLL(_lib.LIB_PATH), NEW_SYMBOL)
    assert _lib.lib().mee_abi_version() == 2 == _lib.ABI_VERSION     # additive: the ABI version stays
    import meepoembedding_amd as pkg
    from meepoembedding_amd import TieredTableGroup
    from meepoembedding_amd.sharded import ShardedTableGroup, ShardedTieredTableGroup
    for m in ("find_pooled_jagged", "apply_indexed"):
        assert callable(getattr(TieredTableGroup, m))
    assert pkg.ShardedTieredTableGroup is ShardedTieredTableGroup and "ShardedTieredTableGroup" in pkg.__all__
    assert issubclass(ShardedTieredTableGroup, ShardedTableGroup)
    for m in ("find", "find_or_insert", "apply_adagrad", "apply_adam", "find_pooled", "apply_pooled", "traffic"):      # ShardedTableGroup's, unchanged
        assert getattr(ShardedTieredTableGroup, m) is getattr(ShardedTableGroup, m)
    assert ShardedTieredTableGroup.weighted_bags is False and ShardedTieredTableGroup.pools_with_insert is True
    for m in ("rebalance", "size"):
        assert callable(getattr(ShardedTieredTableGroup, m))


def test_null_groups_are_errors_not_faults(built):
    L = _lib.lib()
    fn, buf = L.mee_group_find_pooled_tiered_jagged, (C.c_uint64 * 8)()
    for mode in (0, 7):
        assert fn(None, None, None, 0, None, 0, None, None, None, mode, 0, None) == _lib.ERR_INVALID_ARG
        assert L.mee_last_error().decode().startswith(NEW_SYMBOL + ": null argument")
        assert fn(None, None, buf, 2, buf, 1, buf, buf, buf, mode, 3, None) == _lib.ERR_INVALID_ARG
        assert L.mee_last_error().decode().startswith(NEW_SYMBOL + ": null argument")


def test_refusals_need_no_process_group(built):
    """a local group that is no TieredTableGroup, a narrow-row tier and weights through the bag layer: refused before a process group is looked at"""
    from meepoembedding_amd import MeepoError, TieredTableGroup
    from meepoembedding_amd import nn as mnn
    from meepoembedding_amd.sharded import ShardedTieredTableGroup
    pairs, _ = _cpu_pairs(4, oracle.OPT_ADAGRAD, fill=False)
    plain = type("G", (), {"dim": 4, "tables": [p.hot for p in pairs]})()
    for bad in (plain, pairs, pairs[0], None):
        with pytest.raises(ValueError, match="is no TieredTableGroup"):
            ShardedTieredTableGroup(bad, router=None)
    group = TieredTableGroup(pairs)
    pairs[1].cold.value_dtype = torch.bfloat16
    with pytest.raises(MeepoError, match="ShardedTieredTableGroup: a bf16-row table"):
        ShardedTieredTableGroup(group, router=None)
    del pairs[1].cold.value_dtype
    sg = ShardedTieredTableGroup.__new__(ShardedTieredTableGroup)      # (no process group: the refusal must not need one)
    sg.local = sg.local_group = group
    sg.dim, sg.n_tables, sg.collectives = 4, 3, 0
    layer = mnn.DynamicEmbeddingBag(sg, mode="sum")
    with pytest.raises(ValueError, match="per_sample_weights"):
        layer(torch.zeros(3, dtype=torch.int64), torch.tensor([0, 1, 2, 3]), per_sample_weights=torch.ones(3))
    assert sg.collectives == 0
    assert mnn.DynamicEmbeddingBag(sg, out_dtype=BF16).out_dtype == BF16 and mnn.DynamicEmbeddingCollection(sg, out_dtype=BF16).out_dtype == BF16


def _cpu_world(rank, world, dim, opt):
    """-> (this rank's three oracle-backed pairs: the stored keys it owns, a third of them hot, and one union table per member)"""
    from _cpu_backend import CpuTable
    st = stored_keys()
    mine = st[oracle.hash_batch(st, 1, world)[2] == rank]
    pairs, _ = _cpu_pairs(dim, opt, fill=False)
    full = []
    for j, pair in enumerate(pairs):
        hot = (np.arange(mine.size) + j) % 3 == 0
        rows = synth.rows_np(mine, dim, 3 + j)
        pair.hot.insert(torch.from_numpy(mine[hot]), torch.from_numpy(rows[hot]))
        pair.cold.insert(torch.from_numpy(mine[~hot]), torch.from_numpy(rows[~hot]))
        pair._hot_keys_ub = pair.hot.size()
        u = CpuTable(8192, dim, optimizer=opt, init_seed=9 + j, default_value=HOT_DEFAULT[j], **INIT)
        u.insert(torch.from_numpy(st), torch.from_numpy(synth.rows_np(st, dim, 3 + j)))
        full.append(u)
    return pairs, full


def _cpu_rank(rank, world, port, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        from meepoembedding_amd import TieredTableGroup
        from meepoembedding_amd.sharded import ShardedTieredTableGroup
        dist.init_process_group("gloo", rank=rank, world_size=world)
        dim, T = 4, T3
        pairs, full = _cpu_world(rank, world, dim, oracle.OPT_ADAGRAD)
        sg = ShardedTieredTableGroup(TieredTableGroup(pairs), NpBagRouter(world))
        assert sg.traffic() == (0, 0) and sg.collectives == 0 and sg.n_tables == T and sg.dim == dim and sg.tables is sg.local_group.tables
        find_rows = lambda j, k: tuple(x.numpy() for x in full[j].find(torch.from_numpy(k)))      # noqa: E731
        tn = torch.from_numpy

        def wire(batches):
            """-> (k_out, k_in, r_out, r_in) of this rank for the pooled batches of all ranks"""
            to = [np.bincount(oracle.hash_batch(k, 1, world)[2], minlength=world) if k.size else np.zeros(world, dtype=np.int64) for k, _ in batches]
            ro = [run_counts_of(k, o, world) for k, o in batches]
            return (int(to[rank].sum() - to[rank][rank]), int(sum(to[s][rank] for s in range(world) if s != rank)),
                    int(ro[rank].sum() - ro[rank][rank]), int(sum(ro[s][rank] for s in range(world) if s != rank)))

        def assert_shards(what):
            """this rank's pairs hold the union's keys it owns, each in one tier, rows and state bit for bit"""
            for j in range(T):
                ek, ev, ea, _ = full[j].export(with_state=True)
                sel = tn(oracle.hash_batch(ek.numpy(), 1, world)[2] == rank)
                gk, gv, ga, _ = sg.tables[j].export(with_state=True)      # (the pair's export: hot, then cold)
                io, ig = torch.argsort(ek[sel]), torch.argsort(gk)
                assert torch.equal(ek[sel][io], gk[ig]) and gk.unique().numel() == gk.numel(), (what, j)
                assert torch.equal(gv[ig].view(torch.int32), ev[sel][io].view(torch.int32)) and torch.equal(ga[ig].view(torch.int32), ea[sel][io].view(torch.int32)), (what, j)

        # ---- the unpooled operators: 4 collectives per lookup, 3 per step ----
        ub = [make_batch("plain", 30 + r, world, T) for r in range(world)]
        keys, off = ub[rank] if rank else make_batch("n = 0", 0, world, T)      # rank 0 has an empty batch
        kt, ot = tn(keys), tn(off)
        for bad in (lambda: sg.find(kt, ot[:-1]), lambda: sg.find(kt, ot, out_dtype=torch.float16),
                    lambda: ShardedTieredTableGroup(sg.local_group, NpRouter(world + 1)),
                    lambda: sg.find_pooled(kt, ot, "max"), lambda: sg.find_pooled(kt, ot, out_dtype=torch.float16), lambda: sg.find_pooled(kt, ot[:-2]),
                    lambda: ShardedTieredTableGroup(sg.local_group, NpRouter(world)).find_pooled(kt, ot),                     # no bag_runs
                    lambda: sg.apply_pooled(kt, ot, torch.zeros(T, dim), torch.zeros(keys.size, dtype=torch.int64), "sgd", 0.01)):
            with pytest.raises(ValueError):
                bad()
        assert sg.traffic() == (0, 0) and sg.collectives == 0
        rows, found = sg.find(kt, ot)
        assert sg.collectives == 4
        for j in range(T):
            er, ef = full[j].find(kt[off[j]:off[j + 1]])
            assert torch.equal(rows[off[j]:off[j + 1]].view(torch.int32), er.view(torch.int32)) and torch.equal(found[off[j]:off[j + 1]], ef), j
        to = np.bincount(oracle.hash_batch(keys, 1, world)[2], minlength=world) if keys.size else np.zeros(world, dtype=np.int64)
        every = [None] * world
        dist.all_gather_object(every, to.tolist())
        k_out, k_in = int(to.sum() - to[rank]), int(sum(every[s][rank] for s in range(world) if s != rank))
        cnt = 8 * T * (world - 1)
        assert sg.traffic() == (8 * k_out + (4 * dim + 1) * k_in + cnt, 8 * k_in + (4 * dim + 1) * k_out + cnt)      # SPEC §5: keys out, rows and found bytes back, the cells
        # find_or_insert: keys no table has seen, overlapping between the ranks and meeting every member; found = present before
        # (no padding keys here: the oracle adapter's find_or_insert_missing hands a reserved key the default row of the table it asks, which for
        # the cold tier is not the pair's — the HIP creation launch leaves such a row as find wrote it, and the GPU tests below keep the padding)
        fb = [with_fresh(np.where(ub[r][0] == EMPTY_KEY, stored_keys()[0], ub[r][0]), ub[r][1], synth.keys_np(77, 10 * r, 40)) for r in range(world)]
        fk, fo = fb[rank]
        before = [full[j].find(tn(fk[fo[j]:fo[j + 1]]))[1] for j in range(T)]
        rows, found = sg.find_or_insert(tn(fk), tn(fo))
        assert sg.collectives == 8
        for k, o in fb:       # the reference creates every rank's keys
            for j in range(T):
                full[j].find_or_insert(tn(k[o[j]:o[j + 1]]))
        for j in range(T):
            er, _ = full[j].find(tn(fk[fo[j]:fo[j + 1]]))
            assert torch.equal(rows[fo[j]:fo[j + 1]].view(torch.int32), er.view(torch.int32)) and torch.equal(found[fo[j]:fo[j + 1]], before[j]), j
        dist.barrier()
        assert_shards("find_or_insert")
        assert sg.size() == sum(t.size() for t in full) and full[0].size() > NK      # one all-reduce, no all-to-all
        assert sg.collectives == 8
        t0 = sg.traffic()
        rng = np.random.default_rng(5)       # the same on every rank
        db = distinct_batches(rng, world, T, [2 + r for r in range(world)])
        dk, do = db[rank]
        B = (do.size - 1) // T
        g = tn((synth.rows_np(dk, dim, 6 + rank) * 0.02).astype(np.float32))
        sg.apply_adagrad(tn(dk), tn(do[::B].copy()), g, 0.01)
        assert sg.collectives == 11
        for j in range(T):
            for r, (k, o) in enumerate(db):
                b = (o.size - 1) // T
                s, e = o[j * b], o[(j + 1) * b]
                full[j].apply_adagrad(tn(k[s:e]), tn((synth.rows_np(k, dim, 6 + r) * 0.02).astype(np.float32)[s:e]), 0.01)
        to = [np.bincount(oracle.hash_batch(k, 1, world)[2], minlength=world) for k, _ in db]
        k_out, k_in = int(to[rank].sum() - to[rank][rank]), int(sum(to[s][rank] for s in range(world) if s != rank))
        t1 = sg.traffic()
        assert (t1[0] - t0[0], t1[1] - t0[1]) == ((8 + 4 * dim) * k_out + cnt, (8 + 4 * dim) * k_in + cnt)
        dist.barrier()
        assert_shards("apply_adagrad")

        # ---- the pooled operators: 5 collectives per lookup, 4 per step ----
        pb = [bag_batch(30 + r, T, 2 + r) for r in range(world)]      # B differs from rank to rank
        keys, off = pb[rank] if rank else (np.zeros(0, dtype=np.int64), np.zeros(T + 1, dtype=np.int64))      # rank 0: a bag per member and no keys
        pb[0] = (np.zeros(0, dtype=np.int64), np.zeros(T + 1, dtype=np.int64))
        kt, ot = tn(keys), tn(off)
        c0 = sg.collectives
        for n_call, mode in enumerate(("sum", "mean")):
            t0 = sg.traffic()
            rows, found = sg.find_pooled(kt, ot, mode)
            assert sg.collectives - c0 == 5 * (n_call + 1)
            er, ef = ref_bags(find_rows, keys, off, world, T, mode)
            same_bits(rows.numpy(), er, mode)
            assert np.array_equal(found.numpy().astype(bool), ef)
            t1 = sg.traffic()
        k_out, k_in, r_out, r_in = wire(pb)
        cnt = 16 * T * (world - 1)
        assert (t1[0] - t0[0], t1[1] - t0[1]) == (8 * k_out + 4 * r_out + 4 * dim * r_in + k_in + cnt, 8 * k_in + 4 * r_in + 4 * dim * r_out + k_out + cnt)
        rows, _ = sg.find_pooled(kt, ot, "mean", out_dtype=BF16)
        assert_rows(rows, ref_bags(find_rows, keys, off, world, T, "mean")[0], BF16, "bf16 mean")
        # insert_missing: found = present before; afterwards the keys exist in one tier of one owner
        fresh = [with_fresh_bags(*pb[r], T, synth.keys_np(78, 10 * r, 40)) for r in range(world)]
        fk, fo = fresh[rank]
        before = ref_bags(find_rows, fk, fo, world, T, "sum")[1]
        c0 = sg.collectives
        rows, found = sg.find_pooled(tn(fk), tn(fo), "sum", insert_missing=True)
        assert sg.collectives - c0 == 5
        for k, o in fresh:
            b = (o.size - 1) // T
            for j in range(T):
                full[j].find_or_insert(tn(k[o[j * b]:o[(j + 1) * b]]))
        same_bits(rows.numpy(), ref_bags(find_rows, fk, fo, world, T, "sum")[0], "insert_missing")
        assert np.array_equal(found.numpy().astype(bool), before)
        dist.barrier()
        assert_shards("insert_missing")
        # apply_pooled: no key twice in a member over all ranks -> bit for bit
        db = distinct_batches(rng, world, T, [2 + r for r in range(world)])
        dk, do = db[rank]
        n_bags = do.size - 1
        g = tn((synth.rows_np(np.arange(n_bags, dtype=np.int64), dim, 16 + rank) * 0.02).astype(np.float32)).view(n_bags, dim)
        bag_of = tn(np.repeat(np.arange(n_bags), np.diff(do)))
        c0, t0 = sg.collectives, sg.traffic()
        sg.apply_pooled(tn(dk), tn(do), g, bag_of, "adagrad", 0.01, located=torch.zeros(3))      # located: accepted and ignored
        assert sg.collectives - c0 == 4
        k_out, k_in, r_out, r_in = wire(db)
        t1 = sg.traffic()
        assert (t1[0] - t0[0], t1[1] - t0[1]) == (8 * k_out + (4 + 4 * dim) * r_out + cnt, 8 * k_in + (4 + 4 * dim) * r_in + cnt)
        for j in range(T):
            for r, (k, o) in enumerate(db):
                b = (o.size - 1) // T
                g_r = (synth.rows_np(np.arange(o.size - 1, dtype=np.int64), dim, 16 + r) * 0.02).astype(np.float32).reshape(-1, dim)
                s, e = o[j * b], o[(j + 1) * b]
                full[j].apply_adagrad(tn(k[s:e]), tn(g_r[np.repeat(np.arange(o.size - 1), np.diff(o))][s:e]), 0.01)
        dist.barrier()
        assert_shards("apply_pooled")
        # rebalance: the local group's, no collective in it (a group with the placement policy on)
        policy_pairs, _ = _cpu_pairs(dim, oracle.OPT_ADAGRAD, track_hits=True)
        sp = ShardedTieredTableGroup(TieredTableGroup(policy_pairs), NpBagRouter(world))
        if rank:      # rank-local: the ranks need not call it together
            moves = sp.rebalance(16)
            assert len(moves) == T and all(len(m) == 2 for m in moves)
        assert sp.collectives == 0 and sp.traffic() == (0, 0)
        q.put((rank, sg.traffic()))
        dist.barrier()
        dist.destroy_process_group()
    except BaseException as e:
        import traceback
        q.put(("error", rank, "".join(traceback.format_exception(type(e), e, e.__traceback__))))
        raise


def test_host_logic_collectives_traffic_and_refusals_without_a_gpu(built):
    res = _launch(_cpu_rank, 2, (), first_timeout=120)
    assert sum(r[1][0] for r in res) == sum(r[1][1] for r in res)     # what all ranks sent is what all ranks received


# ---- GPU fixtures -----------------------------------------------------------------------------------------------------------------
def _pairs(T, dim, dev, optimizer, part, max_batch, hot_defaults=None, all_hot=False):
    """T hot/cold pairs (hot in HBM, cold rows in pinned host memory; CAPS' sizes) over the keys `part` of the stored ones: the SAME key values in
    every member, member j's rows from seed 2 + j as test_sharded_groups._members stores them, and the same initializer — so one union table per
    member (_members) is the model.  Keys alternate between the tiers by index, shifted per member (all_hot: the cold tables stay empty)."""
    from meepoembedding_amd import INIT_UNIFORM, LookupTable
    from meepoembedding_amd.tiered import TieredLookupTable
    st = stored_keys()[part]
    pairs = []
    for j in range(T):
        hc, cc = CAPS[j % len(CAPS)]
        kw = dict(device=dev, optimizer=optimizer, initial_accumulator=0.1, max_batch=max_batch, initializer=INIT_UNIFORM, init_scale=0.05, init_seed=7)
        hot = LookupTable(hc, dim, default_value=DEFAULT if hot_defaults is None else hot_defaults[j], **kw)
        cold = LookupTable(cc, dim, default_value=COLD_DEFAULT, value_memory=_lib.MEM_HOST_PINNED, **kw)
        in_hot = np.ones(st.size, bool) if all_hot else (np.arange(st.size) + j) % 2 == 0
        rows = synth.rows_np(st, dim, 2 + j)
        hot.insert(_i64(st[in_hot], dev), torch.from_numpy(rows[in_hot]).to(dev))
        if not all_hot:
            cold.insert(_i64(st[~in_hot], dev), torch.from_numpy(rows[~in_hot]).to(dev))
        pair = TieredLookupTable(hot, cold)
        pair._hot_keys_ub = hot.size()      # (the tiers were filled directly: the pair's bound on its hot keys starts at what is there)
        pairs.append(pair)
    return pairs


def _tiers(group_or_pairs, j):
    pairs = getattr(group_or_pairs, "tables", group_or_pairs)
    return [pairs[j].hot, pairs[j].cold]


def _lookup_batch(lens, first):
    """-> (keys, offsets) for bags of `lens`: consecutive stored keys — hot and cold alternate by index, so they interleave inside every bag — and in the
    longest bag and one other a key repeated two positions on, an absent key, RECLAIMED and EMPTY"""
    lens = list(lens)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    keys = stored_keys()[first:first + int(off[-1])].copy()
    p = int(off[int(np.argmax(lens))])
    keys[p + 6] = keys[p + 4]
    keys[p + 9], keys[p + 20], keys[p + 31] = ABSENT_KEY, EMPTY_KEY, RECLAIMED_KEY
    q = int(off[lens.index(15) if 15 in lens else lens.index(33)])
    keys[q + 3], keys[q + 8], keys[q + 11] = RECLAIMED_KEY, ABSENT_KEY, EMPTY_KEY
    keys[q + 6] = keys[q + 4]
    return keys, off


def _sentinels(n_bags, n, dim, dev):
    return torch.full((n_bags + 2, dim), -3.5, device=dev), torch.full((n + 5,), 7, dtype=torch.uint8, device=dev)


# ---- GPU, one process: the jagged tiered launch against the pair's find_pooled per member -----------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("dim", [4, 24, 64])
def test_jagged_tiered_lookup_against_the_pairs(dev, dim, T):
    """14 bags in each launch shape (LENS_A: a tile per bag, with empty bags and bags of 15 / 16 / 17 / 40 keys; LENS_B: a wave per bag).  T = 3, map
    [2, 7, 7, 12]: two bags below the map, a member without bags, two bags beyond it, and no bound a multiple of 4 — a wave's four bags straddle members
    and the map's edge."""
    from meepoembedding_amd import OPT_NONE, TieredTableGroup
    hd = [0.5, 0.75, 1.5]
    pairs = _pairs(T, dim, dev, OPT_NONE, slice(None), 4096, hot_defaults=hd)
    group = TieredTableGroup(pairs)
    n_bags = 14
    maps = {1: ([0, 14], [3, 13]), 3: ([2, 7, 7, 12], [0, 3, 9, 14])}[T]
    for bname, lens in (("A", LENS_A[:n_bags]), ("B", LENS_B[:n_bags])):
        keys, off = _lookup_batch(lens, 100)
        n = keys.size
        assert (n // n_bags >= 12) == (bname == "B")      # the launch shape: mee_group_find_pooled_tiered_jagged picks it as every pooled lookup does
        kt, ot = _i64(keys, dev), _i64(off, dev)
        # offsets are the caller's: bags past the key array are cut at its end, a decreasing pair is an empty bag
        bad = _i64([0, 10, 5, 40, 40, 60, 60, 100, 90, 120, 125, n + 3, 1 << 40, 1 << 41, 5], dev)
        for mb in maps:
            mbt = _i64(mb, dev)
            inside = np.zeros(n, bool)
            inside[off[mb[0]]:off[mb[-1]]] = True
            for mode in ("sum", "mean"):
                what = (bname, mb, mode, dim)
                out, found = _sentinels(n_bags, n, dim, dev)
                r_out, r_found = group.find_pooled_jagged(kt, ot, mbt, mode, out=out[:n_bags], found=found[:n])
                assert r_out.shape == (n_bags, dim) and r_found.shape == (n,)
                assert bool((out[n_bags:] == -3.5).all()) and bool((found[n:] == 7).all()), what      # nothing behind the outputs
                for j in range(T):
                    lo, hi = mb[j], mb[j + 1]
                    if hi <= lo:
                        continue
                    a, b = int(off[lo]), int(off[hi])
                    er, ef = pairs[j].find_pooled(kt[a:b], (ot[lo:hi + 1] - a).contiguous(), mode)
                    same_bits(out[lo:hi].cpu().numpy(), er.cpu().numpy(), str(what + (j,)))
                    assert torch.equal(found[a:b], ef), what + (j,)
                # bags outside the map: rows of zeros, nothing probed — their found bytes are what TableGroup.find_pooled_jagged leaves on the same batch
                f2 = torch.full((n,), 7, dtype=torch.uint8, device=dev)
                group.hot_group.find_pooled_jagged(kt, ot, mbt, mode, found=f2)
                outside = torch.from_numpy(~inside).to(dev)
                assert torch.equal(found[:n][outside], f2[outside]) and bool((f2[outside] == 7).all()), what
                for lo, hi in ((0, mb[0]), (mb[-1], n_bags)):
                    assert not out[lo:hi].any(), what
                # the clamped offsets: per member the pair's lookup over the same key array with the member's offsets as they are
                out, found = _sentinels(n_bags, n, dim, dev)
                group.find_pooled_jagged(kt, bad, mbt, mode, out=out[:n_bags], found=found[:n])
                want_found = torch.full((n,), 7, dtype=torch.uint8, device=dev)
                for j in range(T):
                    lo, hi = mb[j], mb[j + 1]
                    if hi > lo:
                        po, pf = pairs[j].find_pooled(kt, bad[lo:hi + 1].contiguous(), mode, found=torch.full((n,), 7, dtype=torch.uint8, device=dev))
                        same_bits(out[lo:hi].cpu().numpy(), po.cpu().numpy(), f"{what} clamped offsets, member {j}")
                        want_found = torch.where(pf != 7, pf, want_found)
                assert torch.equal(found[:n], want_found) and bool((out[n_bags:] == -3.5).all()) and bool((found[n:] == 7).all()), what
                for lo, hi in ((0, mb[0]), (mb[-1], n_bags)):
                    assert not out[lo:hi].any(), what
    if T > 1:      # a cold default never shows, a member's own hot default does: a bag of one absent key per member
        out, _ = group.find_pooled_jagged(_i64([ABSENT_KEY] * T, dev), _i64(np.arange(T + 1), dev), _i64(np.arange(T + 1), dev))
        assert torch.equal(out, torch.tensor(hd, device=dev)[:, None].expand(T, dim))
    torch.cuda.synchronize(dev)


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [4, 64])
def test_jagged_tiered_lookup_against_the_untiered_and_the_regular_launch(dev, dim):
    """every key hot and the cold tables empty: TableGroup.find_pooled_jagged of the hot group on the same arguments, bit for bit, found included;
    the regular map [0, B, 2B, 3B] over mixed tiers: mee_group_find_pooled_tiered(bags_per_table = B), bit for bit.  B = 5."""
    from meepoembedding_amd import OPT_NONE, TieredTableGroup
    T, B = T3, 5
    hot_only = TieredTableGroup(_pairs(T, dim, dev, OPT_NONE, slice(None), 4096, all_hot=True))
    mixed = TieredTableGroup(_pairs(T, dim, dev, OPT_NONE, slice(None), 4096))
    assert all(p.cold.size() == 0 for p in hot_only.tables) and all(p.cold.size() > 1000 for p in mixed.tables)
    for lens in (LENS_A, LENS_B):
        keys, off = _lookup_batch(lens, 300)
        n, n_bags = keys.size, T * B
        kt, ot = _i64(keys, dev), _i64(off, dev)
        for mode in ("sum", "mean"):
            for mb in ([0, B, 2 * B, 3 * B], [2, 7, 7, 12], [0, 0, 15, 15]):
                mbt = _i64(mb, dev)
                o1, f1 = _sentinels(n_bags, n, dim, dev)
                o2, f2 = _sentinels(n_bags, n, dim, dev)
                hot_only.find_pooled_jagged(kt, ot, mbt, mode, out=o1[:n_bags], found=f1[:n])
                hot_only.hot_group.find_pooled_jagged(kt, ot, mbt, mode, out=o2[:n_bags], found=f2[:n])
                assert torch.equal(o1.view(torch.int32), o2.view(torch.int32)) and torch.equal(f1, f2), (mode, mb)
            o1, f1 = _sentinels(n_bags, n, dim, dev)
            o2, f2 = _sentinels(n_bags, n, dim, dev)
            mixed.find_pooled_jagged(kt, ot, _i64(np.arange(T + 1) * B, dev), mode, out=o1[:n_bags], found=f1[:n])
            mixed.find_pooled(kt, ot, mode, out=o2[:n_bags], found=f2[:n])
            assert torch.equal(o1.view(torch.int32), o2.view(torch.int32)) and torch.equal(f1, f2), mode
            assert bool(f1[:n].any()) and not bool(f1[:n].all())
    torch.cuda.synchronize(dev)


@pytest.mark.gpu
@pytest.mark.parametrize("bname", ["A", "B"])
def test_jagged_tiered_lookup_counts_hits_like_the_regular_launch(dev, bname):
    """with both count flags the members' counters after the jagged launch at the regular map are those after the regular launch on a twin; flags 0
    leave them untouched"""
    from meepoembedding_amd import TieredTableGroup
    L = _lib.lib()
    keys, off = ttg._batches()[bname]
    a, b = ttg._policy_pairs(dev), ttg._policy_pairs(dev)
    ga, gb = TieredTableGroup(a), TieredTableGroup(b)
    T, B, dim = ttg.N_MEMBERS, ttg.BPT, 16
    dk, do, mb = _i64(keys, dev), _i64(off, dev), _i64(np.arange(T + 1) * B, dev)
    out, ref = torch.empty(T * B, dim, device=dev), torch.empty(T * B, dim, device=dev)
    both = _lib.TIER_COUNT_COLD | _lib.TIER_COUNT_HOT
    for flags in (0, both, both):
        _lib.check(L.mee_group_find_pooled_tiered_jagged(ga.hot_group._h, ga.cold_group._h, dk.data_ptr(), keys.size, do.data_ptr(), T * B, mb.data_ptr(),
                                                         out.data_ptr(), None, 0, flags, None))
        _lib.check(L.mee_group_find_pooled_tiered(gb.hot_group._h, gb.cold_group._h, dk.data_ptr(), keys.size, do.data_ptr(), B, ref.data_ptr(),
                                                  _lib.DTYPE_F32, None, 0, flags, None))
        torch.cuda.synchronize(dev)
        assert torch.equal(out, ref)
        got, want = ttg._hit_sets(a), ttg._hit_sets(b)
        for g, w in zip(got, want):
            for x, y in zip(g, w):
                assert np.array_equal(x, y), flags
        if flags == 0:
            assert all(x.size == 0 for g in got for x in g), "no flag, no count"
    assert got[0][1].size and got[1][1].size and got[2][1].size and got[3][1].size, "both tiers of members 0 and 1 were counted, twice"
    # the Python method: cold hits on every call, hot hits on every sample_every-th, as find_pooled counts them
    fresh = ttg._policy_pairs(dev)
    g2 = TieredTableGroup(fresh, sample_every=4)
    for _ in range(8):
        g2.find_pooled_jagged(dk, do, mb)
    hot_twice, cold_8 = np.sort(fresh[0].hot.hits_scan(2, 0xFFFFFFFF, 4096).cpu().numpy()), np.sort(fresh[0].cold.hits_scan(8, 0xFFFFFFFF, 4096).cpu().numpy())
    mk, universe = keys[off[0]:off[B]], ttg._universe()
    assert np.array_equal(hot_twice, np.sort(np.intersect1d(mk, universe[0::2]))) and np.array_equal(cold_8, np.sort(np.intersect1d(mk, universe[1::2])))


@pytest.mark.gpu
def test_jagged_tiered_entry_point_refuses(dev):
    from meepoembedding_amd import MeepoError, OPT_NONE, TieredTableGroup
    T, dim = T3, 4
    group = TieredTableGroup(_pairs(T, dim, dev, OPT_NONE, slice(None), 4096))
    keys, off = bag_batch(3, T, 2)
    kt, ot, mb = _i64(keys, dev), _i64(off, dev), _i64([0, 2, 4, 6], dev)
    L, st = _lib.lib(), torch.cuda.current_stream(dev).cuda_stream
    out = torch.full((6, dim), -3.5, device=dev)
    h, c = group.hot_group._h, group.cold_group._h

    def call(hot=h, cold=c, k=kt.data_ptr(), n=kt.numel(), o=ot.data_ptr(), m=mb.data_ptr(), dst=out.data_ptr(), n_bags=6, mode=0, flags=0):
        return L.mee_group_find_pooled_tiered_jagged(hot, cold, k, n, o, n_bags, m, dst, None, mode, flags, st)
    for rc in (call(hot=None), call(cold=None), call(k=None), call(o=None), call(m=None), call(dst=None), call(mode=2), call(mode=-1), call(flags=4),
               call(cold=h), call(flags=_lib.TIER_COUNT_COLD), call(flags=_lib.TIER_COUNT_HOT)):      # (the tables have no hit counters)
        assert rc == _lib.ERR_INVALID_ARG and L.mee_last_error().decode().startswith(NEW_SYMBOL + ":"), L.mee_last_error()
    torch.cuda.synchronize(dev)
    assert bool((out == -3.5).all()), "a refused call writes nothing"
    assert call(k=None, n=0, o=None, m=None, dst=None, n_bags=0) == _lib.OK      # no bags: nothing to do
    with pytest.raises(MeepoError):
        group.find_pooled_jagged(kt, ot, mb[:-1])
    with pytest.raises(MeepoError):
        group.find_pooled_jagged(kt, ot[:0], mb)
    with pytest.raises(MeepoError):
        group.find_pooled_jagged(kt, ot, mb, "max")
    with pytest.raises(ValueError):
        group.find_pooled_jagged(kt, ot, mb, out=torch.empty((6, dim), dtype=BF16, device=dev))
    o1, _ = group.find_pooled_jagged(kt, ot, mb)      # found is optional
    assert call() == _lib.OK
    assert torch.equal(o1, out)
    torch.cuda.synchronize(dev)


# ---- GPU, one process: the indexed step against the pairs' apply_*(grad_index=) ----------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("optimizer", ["adagrad", "adam"])
def test_tiered_apply_indexed_is_the_pairs_indexed_step(dev, optimizer):
    """exactly summable gradients (tests/test_apply_exact.py's recipe) read through an index, with duplicates and keys of both tiers in a segment:
    every tier of every pair ends bit-identical to independent copies stepped pair by pair"""
    from meepoembedding_amd import OPT_ADAGRAD, OPT_ADAM, TieredTableGroup
    dim, R = 64, 37
    opt = OPT_ADAGRAD if optimizer == "adagrad" else OPT_ADAM
    a, b = ttg._train_pairs(dev, dim, opt), ttg._train_pairs(dev, dim, opt)
    group = TieredTableGroup(a, max_apply_batch=4096)
    universe = ttg._universe()
    rng = np.random.default_rng(23)
    off = np.concatenate([[0], np.cumsum([37, 70, 5])]).astype(np.int64)
    n = int(off[-1])
    for step in (1, 2, 3):
        keys = universe[rng.integers(0, ttg.N_KEYS, n)]          # duplicates, keys of both tiers (the first 200 are hot)
        keys[off[1] + 2] = keys[off[1] + 40] = keys[off[1]]
        keys[off[0] + 3], keys[off[1] + 5], keys[off[1] + 6] = ABSENT_KEY, EMPTY_KEY, ABSENT_KEY
        gi = rng.integers(0, R, n).astype(np.int32)
        dk, dg, dgi, do = _i64(keys, dev), torch.from_numpy(exact_grads_np(rng, R, dim, positions=n)).to(dev), torch.from_numpy(gi).to(dev), _i64(off, dev)
        group.apply_indexed(dk, do, dg, dgi, optimizer, 0.05 if optimizer == "adagrad" else 0.01, step=step)
        for j, pair in enumerate(b):
            s, e = int(off[j]), int(off[j + 1])
            if optimizer == "adagrad":
                pair.apply_adagrad(dk[s:e], dg, 0.05, 1e-10, grad_index=dgi[s:e])
            else:
                pair.apply_adam(dk[s:e], dg, 0.01, 0.9, 0.999, 1e-8, step, grad_index=dgi[s:e])
    ttg._assert_same_tiers(a, b, optimizer)
    assert all(t.status() == 0 for p in a + b for t in (p.hot, p.cold))
    moved = ttg._sorted(a[0].cold.export(with_state=True))[1]
    assert not np.array_equal(moved, synth.rows_np(np.sort(universe[200:]), dim, 3)), "the cold rows were trained"
    with pytest.raises(ValueError):
        group.apply_indexed(dk, do, dg, dgi, "sgd", 0.01)
    torch.cuda.synchronize(dev)


# ---- GPU, one process: the operators with every owner played in turn -------------------------------------------------------------
def _tiered_world(G, T, dim, dev, optimizer):
    """-> (groups[p] = owner p's TieredTableGroup of its T shards, each shard's keys split between hot and cold; full[j] = member j's union table)"""
    from meepoembedding_amd import TieredTableGroup
    owner = oracle.hash_batch(stored_keys(), 1, G)[2]
    mb = max(G * 2048, 4096)
    groups = [TieredTableGroup(_pairs(T, dim, dev, optimizer, owner == p, mb), max_apply_batch=mb if optimizer else 0) for p in range(G)]
    return groups, _members(T, dim, dev, optimizer, slice(None), mb)


def _assert_union(groups, full, G, T, what, exact=True):
    """every member: the tiers of all owners together hold the union table's keys, each once, rows and state bit for bit"""
    for j in range(T):
        got, exp = _sorted_export([t for p in range(G) for t in _tiers(groups[p], j)]), _sorted_export([full[j]])
        assert np.array_equal(got[0], exp[0]) and len(got) == len(exp), (what, j, got[0].size, exp[0].size)      # (equal sorted keys: no key twice)
        for x, y in zip(got[1:], exp[1:]):
            same_bits(x, y, f"{what} member {j}")


EMULATED = [(2, 3, 4), (3, 3, 64)]


@pytest.mark.gpu
@pytest.mark.parametrize("G,T,dim", EMULATED)
def test_emulated_lookups_against_the_union_tables(dev, G, T, dim):
    from meepoembedding_amd import OPT_NONE, Router
    router = Router(G, 2048, device=dev)
    groups, full = _tiered_world(G, T, dim, dev, OPT_NONE)
    # ---- find / find_or_insert, fp32 and bf16 ----
    kinds = ["plain", "empty middle", "skip owner"]
    base = [make_batch(kinds[s % len(kinds)], 50 + s, G, T) for s in range(G)]
    base[0] = (np.tile(stored_keys()[:7], T), np.arange(T + 1, dtype=np.int64) * 7)      # the same key values in every member
    for op, dt, fresh in (("find", torch.float32, None), ("find", BF16, None), ("find_or_insert", torch.float32, 77), ("find_or_insert", BF16, 78)):
        batches_np = base if fresh is None else [with_fresh(k, o, synth.keys_np(fresh, 10 * s, 40)) for s, (k, o) in enumerate(base)]
        batches = [(_i64(k, dev), _i64(o, dev)) for k, o in batches_np]
        kw = {} if dt == torch.float32 else {"out_dtype": dt}
        before = [_per_member(full, kt, ot, "find")[1] for kt, ot in batches]
        got = _emulate(router, groups, batches, lambda p, k, o, order, pay: getattr(groups[p], op)(k, o, **kw))
        bits = torch.int32 if dt == torch.float32 else torch.int16
        for s, (kt, ot) in enumerate(batches):
            er, _ = _per_member(full, kt, ot, op, **kw)
            rows, found = got[s]
            assert rows.dtype == dt and rows.shape == (kt.numel(), dim)
            assert torch.equal(rows.view(bits), er.view(bits)) and torch.equal(found, before[s]), (op, dt, s)
        assert not torch.equal(got[0][0][:7].float(), got[0][0][-7:].float())
    _assert_union(groups, full, G, T, "find_or_insert")
    assert full[0].size() > NK
    # ---- find_pooled: sum / mean, fp32 / bf16 ----
    find_rows = _gpu_find_rows(full, dev, dim)
    batches_np = [bag_batch(50 + s, T, 2 + s) for s in range(G)]      # B differs from rank to rank
    batches_np[-1] = (np.tile(stored_keys()[:9], T), np.arange(3 * T + 1, dtype=np.int64) * 3)    # the same key values in every member
    batches_np[0] = (np.zeros(0, dtype=np.int64), np.zeros(2 * T + 1, dtype=np.int64))            # a rank with bags and no keys
    batches = [(_i64(k, dev), _i64(o, dev)) for k, o in batches_np]

    def lookup(p, k, o, run_len, member_bags, pay):
        run_off, _ = router.run_offsets(run_len)
        return groups[p].find_pooled_jagged(k, run_off, member_bags, "sum")
    got = _emulate_bags(router, groups, batches, lookup)
    for s, ((k, o), (kt, ot)) in enumerate(zip(batches_np, batches)):
        partial, found, run_bag, run_counts = got[s]
        for mode in ("sum", "mean"):
            er, ef = ref_bags(find_rows, k, o, G, T, mode)
            for dt in (torch.float32, BF16):
                assert_rows(router.combine_bag_runs(partial, run_bag, run_counts, ot, mode, out_dtype=dt), er, dt, f"G={G} dim={dim} rank {s} {mode} {dt}")
            assert np.array_equal(found.cpu().numpy().astype(bool), ef)
    out = router.combine_bag_runs(got[-1][0], got[-1][2], got[-1][3], batches[-1][1], "sum")
    assert not torch.equal(out[:3], out[-3:])
    # ---- insert_missing: keys no table has seen, overlapping between the ranks and meeting every member; found = present before ----
    fresh_np = [with_fresh_bags(k, o, T, synth.keys_np(79, 10 * s, 40)) for s, (k, o) in enumerate(batches_np)]
    fresh = [(_i64(k, dev), _i64(o, dev)) for k, o in fresh_np]
    before = [ref_bags(find_rows, k, o, G, T, "sum")[1] for k, o in fresh_np]

    def lookup_insert(p, k, o, run_len, member_bags, pay):
        run_off, _ = router.run_offsets(run_len)
        _, found = groups[p].find_or_insert(k, o)
        return groups[p].find_pooled_jagged(k, run_off, member_bags, "sum")[0], found
    got = _emulate_bags(router, groups, fresh, lookup_insert)
    for (kt, ot) in fresh:      # the reference creates every rank's keys
        B = (ot.numel() - 1) // T
        o = ot.tolist()
        for j in range(T):
            if o[(j + 1) * B] > o[j * B]:
                full[j].find_or_insert(kt[o[j * B]:o[(j + 1) * B]])
    for s, ((k, o), (kt, ot)) in enumerate(zip(fresh_np, fresh)):
        partial, found, run_bag, run_counts = got[s]
        er, _ = ref_bags(find_rows, k, o, G, T, "mean")
        assert_rows(router.combine_bag_runs(partial, run_bag, run_counts, ot, "mean"), er, torch.float32, f"insert_missing rank {s}")
        assert np.array_equal(found.cpu().numpy().astype(bool), before[s]), s
    # afterwards every key exists in exactly one tier of exactly one owner, and that owner is the one the router names
    _assert_union(groups, full, G, T, "insert_missing")
    for j in range(T):
        ek = full[j].export()[0].cpu().numpy()
        per = np.bincount(oracle.hash_batch(ek, 1, G)[2], minlength=G)
        assert [groups[p].tables[j].size() for p in range(G)] == per.tolist()
    torch.cuda.synchronize(dev)


@pytest.mark.gpu
@pytest.mark.parametrize("opt", ["adagrad", "adam"])
@pytest.mark.parametrize("G,T,dim", EMULATED)
def test_emulated_steps_against_the_union_tables(dev, G, T, dim, opt):
    """steps without duplicate keys (no key twice in a member over all ranks): apply_pooled's owner side (apply_indexed), then apply_adagrad /
    apply_adam, end bit-identical to the union tables, state planes included"""
    from meepoembedding_amd import OPT_ADAGRAD, OPT_ADAM, Router
    router = Router(G, 2048, device=dev)
    groups, full = _tiered_world(G, T, dim, dev, OPT_ADAGRAD if opt == "adagrad" else OPT_ADAM)
    rng = np.random.default_rng(G * 10 + T)
    # the pooled step
    batches_np = distinct_batches(rng, G, T, [2 + s for s in range(G)])
    batches = [(_i64(k, dev), _i64(o, dev)) for k, o in batches_np]
    pays = [torch.from_numpy(_bag_rows(o.size - 1, dim, 21 + s)).to(dev) for s, (_, o) in enumerate(batches_np)]

    def pooled_owner(p, k, o, run_len, member_bags, rows):
        _, run_of_key = router.run_offsets(run_len, k.numel())
        groups[p].apply_indexed(k, o, rows, run_of_key, opt, 0.01, beta1=0.9, beta2=0.999, step=1)
    assert _emulate_bags(router, groups, batches, pooled_owner, pays) is None
    _reference_step(full, batches_np, T, dim, dev, opt, 1, 21)
    _assert_union(groups, full, G, T, f"apply_pooled {opt}")
    # the unpooled step: the member offsets are every B-th bag offset
    batches_np = [(k, o[::(o.size - 1) // T].copy()) for k, o in distinct_batches(rng, G, T, [3 + s for s in range(G)])]
    batches = [(_i64(k, dev), _i64(o, dev)) for k, o in batches_np]
    grads = [(synth.rows_np(k, dim, 8 + s) * 0.02).astype(np.float32) for s, (k, _) in enumerate(batches_np)]

    def owner(p, k, o, order, pay):
        g = router.gather_rows(pay, order)
        if opt == "adagrad":
            groups[p].apply_adagrad(k, o, g, 0.01, 1e-10)
        else:
            groups[p].apply_adam(k, o, g, 0.01, 0.9, 0.999, 1e-8, 2)
    assert _emulate(router, groups, batches, owner, [torch.from_numpy(g).to(dev) for g in grads]) is None
    for j in range(T):
        ks = np.concatenate([k[o[j]:o[j + 1]] for k, o in batches_np])
        gs = np.concatenate([g[o[j]:o[j + 1]] for g, (_, o) in zip(grads, batches_np)])
        if opt == "adagrad":
            full[j].apply_adagrad(_i64(ks, dev), torch.from_numpy(gs).to(dev), 0.01, 1e-10)
        else:
            full[j].apply_adam(_i64(ks, dev), torch.from_numpy(gs).to(dev), 0.01, 0.9, 0.999, 1e-8, 2)
    _assert_union(groups, full, G, T, f"apply {opt}")
    torch.cuda.synchronize(dev)


# ---- GPU, ranks spawned on one GPU ----------------------------------------------------------------------------------------------
def _gpu_rank(rank, world, port, q, backend, dim):
    try:
        _gpu_rank_body(rank, world, port, q, backend, dim)
    except BaseException as e:   # report at once: the parent must not sit out its queue timeout
        import traceback
        q.put(("error", rank, "".join(traceback.format_exception(type(e), e, e.__traceback__))))
        raise


def _gpu_rank_body(rank, world, port, q, backend, dim):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    from meepoembedding_amd import OPT_ADAGRAD, OPT_ADAM, Router, ShardedTieredTableGroup, TableGroup, TieredTableGroup
    from meepoembedding_amd.nn import DynamicEmbeddingBag, DynamicEmbeddingCollection
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        T = T3
        mine = oracle.hash_batch(stored_keys(), 1, world)[2] == rank
        mb = max(world * 2048, 4096)

        def make(optimizer=OPT_ADAGRAD):
            sg = ShardedTieredTableGroup(TieredTableGroup(_pairs(T, dim, dev, optimizer, mine, mb), max_apply_batch=mb), Router(world, 2048, device=dev))
            return sg, _members(T, dim, dev, optimizer, slice(None), mb)

        def assert_shards(sg, full, what):
            """this rank's pairs hold the union's keys it owns, each in one tier, rows and state bit for bit"""
            for j in range(T):
                got, exp = _sorted_export(_tiers(sg, j)), _sorted_export([full[j]])
                sel = oracle.hash_batch(exp[0], 1, world)[2] == rank
                assert np.array_equal(got[0], exp[0][sel]), (what, j)
                for x, y in zip(got[1:], exp[1:]):
                    same_bits(x, y[sel], f"{what} member {j}")

        def wire(batches):
            to = [np.bincount(oracle.hash_batch(k, 1, world)[2], minlength=world) if k.size else np.zeros(world, dtype=np.int64) for k, _ in batches]
            ro = [run_counts_of(k, o, world) for k, o in batches]
            return (int(to[rank].sum() - to[rank][rank]), int(sum(to[s][rank] for s in range(world) if s != rank)),
                    int(ro[rank].sum() - ro[rank][rank]), int(sum(ro[s][rank] for s in range(world) if s != rank)))

        sg, full = make()
        find_rows = _gpu_find_rows(full, dev, dim)
        dist.barrier()
        # ---- find (fp32, bf16: the owners round before the rows travel) and find_or_insert: 4 collectives each ----
        ub = [make_batch("plain", 40 + r, world, T) for r in range(world)]
        kt, ot = _i64(ub[rank][0], dev), _i64(ub[rank][1], dev)
        for dt, bits in ((torch.float32, torch.int32), (BF16, torch.int16)):
            c0 = sg.collectives
            rows, found = sg.find(kt, ot, out_dtype=dt)
            assert sg.collectives - c0 == 4
            er, ef = _per_member(full, kt, ot, "find", **({} if dt == torch.float32 else {"out_dtype": dt}))
            assert rows.dtype == dt and torch.equal(rows.view(bits), er.view(bits)) and torch.equal(found, ef), dt
        fb = [with_fresh(*ub[r], synth.keys_np(77, 10 * r, 40)) for r in range(world)]      # the ranks' fresh keys overlap
        fkt, fot = _i64(fb[rank][0], dev), _i64(fb[rank][1], dev)
        before = _per_member(full, fkt, fot, "find")[1]
        c0 = sg.collectives
        rows, found = sg.find_or_insert(fkt, fot)
        assert sg.collectives - c0 == 4
        for k, o in fb:       # the reference creates every rank's keys
            _per_member(full, _i64(k, dev), _i64(o, dev), "find_or_insert")
        er, _ = _per_member(full, fkt, fot, "find")
        assert torch.equal(rows.view(torch.int32), er.view(torch.int32)) and torch.equal(found, before)
        dist.barrier()
        assert_shards(sg, full, "find_or_insert")
        assert sg.size() == sum(t.size() for t in full) and full[0].size() > NK      # the sum over ranks and tiers
        # ---- find_pooled: sum and mean, fp32 and bf16; 5 collectives whatever T is; wire bytes ----
        pb = [bag_batch(80 + r, T, 2 + r) for r in range(world)]      # B differs per rank
        keys, off = pb[rank]
        kt, ot = _i64(keys, dev), _i64(off, dev)
        k_out, k_in, r_out, r_in = wire(pb)
        cnt = 16 * T * (world - 1)
        for mode in ("sum", "mean"):
            er, ef = ref_bags(find_rows, keys, off, world, T, mode)
            for dt in (torch.float32, BF16):
                c0, t0 = sg.collectives, sg.traffic()
                rows, found = sg.find_pooled(kt, ot, mode, out_dtype=dt)
                assert sg.collectives - c0 == 5
                t1 = sg.traffic()
                assert (t1[0] - t0[0], t1[1] - t0[1]) == (8 * k_out + 4 * r_out + 4 * dim * r_in + k_in + cnt,
                                                          8 * k_in + 4 * r_in + 4 * dim * r_out + k_out + cnt), (mode, dt)
                assert_rows(rows, er, dt, f"{mode} {dt}")
                assert np.array_equal(found.cpu().numpy().astype(bool), ef)
        # insert_missing: fresh keys overlap between the ranks; found = present before
        fresh = [with_fresh_bags(*pb[r], T, synth.keys_np(78, 10 * r, 40)) for r in range(world)]
        fk, fo = fresh[rank]
        before = ref_bags(find_rows, fk, fo, world, T, "sum")[1]
        c0 = sg.collectives
        rows, found = sg.find_pooled(_i64(fk, dev), _i64(fo, dev), "sum", insert_missing=True, out_dtype=BF16)
        assert sg.collectives - c0 == 5
        for k, o in fresh:
            B = (o.size - 1) // T
            for j in range(T):
                full[j].find_or_insert(_i64(k[o[j * B]:o[(j + 1) * B]], dev))
        assert_rows(rows, ref_bags(find_rows, fk, fo, world, T, "sum")[0], BF16, "insert_missing")
        assert np.array_equal(found.cpu().numpy().astype(bool), before)
        dist.barrier()
        assert_shards(sg, full, "insert_missing")
        report = dict(traffic=sg.traffic(), collectives=sg.collectives)
        # ---- apply_pooled (4 collectives) and apply_adagrad / apply_adam (3): no key twice in a member over all ranks -> bit for bit ----
        for opt in ("adagrad", "adam"):
            sg, full = make(OPT_ADAGRAD if opt == "adagrad" else OPT_ADAM)
            dist.barrier()
            rng = np.random.default_rng(5)       # the same on every rank
            db = distinct_batches(rng, world, T, [2 + r for r in range(world)])
            keys, off = db[rank]
            kt, ot = _i64(keys, dev), _i64(off, dev)
            g = torch.from_numpy(_bag_rows(off.size - 1, dim, 21 + rank)).to(dev)
            bag_of = torch.repeat_interleave(torch.arange(off.size - 1, device=dev), ot[1:] - ot[:-1])
            c0, t0 = sg.collectives, sg.traffic()
            sg.apply_pooled(kt, ot, g, bag_of, opt, 0.01, beta1=0.9, beta2=0.999, step=1)
            assert sg.collectives - c0 == 4
            k_out, k_in, r_out, r_in = wire(db)
            t1 = sg.traffic()
            assert (t1[0] - t0[0], t1[1] - t0[1]) == (8 * k_out + (4 + 4 * dim) * r_out + cnt, 8 * k_in + (4 + 4 * dim) * r_in + cnt)
            _reference_step(full, db, T, dim, dev, opt, 1, 21)
            db = [(k, o[::(o.size - 1) // T].copy()) for k, o in distinct_batches(rng, world, T, [3 + r for r in range(world)])]
            grads = [(synth.rows_np(k, dim, 8 + r) * 0.02).astype(np.float32) for r, (k, _) in enumerate(db)]
            c0 = sg.collectives
            args = (_i64(db[rank][0], dev), _i64(db[rank][1], dev), torch.from_numpy(grads[rank]).to(dev), 0.01)
            if opt == "adagrad":
                sg.apply_adagrad(*args)
            else:
                sg.apply_adam(*args, step=2)
            assert sg.collectives - c0 == 3
            for j in range(T):
                ks = _i64(np.concatenate([k[o[j]:o[j + 1]] for k, o in db]), dev)
                gs = torch.from_numpy(np.concatenate([g_[o[j]:o[j + 1]] for g_, (_, o) in zip(grads, db)])).to(dev)
                if opt == "adagrad":
                    full[j].apply_adagrad(ks, gs, 0.01)
                else:
                    full[j].apply_adam(ks, gs, 0.01, step=2)
            dist.barrier()
            assert_shards(sg, full, f"steps {opt}")

        # ---- the layers over the sharded tiered group == the same layers over the plain group of union tables, bit for bit (no duplicate keys
        # in a member); the loss gradient reaches the rows of both tiers ----
        if world == 1:
            st = stored_keys()
            for opt, code, dt, mode in (("adagrad", OPT_ADAGRAD, torch.float32, "mean"), ("adam", OPT_ADAM, BF16, "sum")):
                rng = np.random.default_rng(9)
                B = 6
                lens = rng.choice((0, 1, 2, 3, 7, 15, 40), T * B)
                lens[-1] = 7
                cut = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
                ks = np.concatenate([st[rng.permutation(NK)[:cut[(j + 1) * B] - cut[j * B]]] for j in range(T)]).astype(np.int64)
                fresh_at = cut[-2] + np.arange(5)      # ids no table has seen, in the last bag
                ks[fresh_at] = synth.keys_np(79, 0, fresh_at.size)
                kt = _i64(ks, dev)
                for kind in ("bag", "collection"):
                    sg, full = make(code)
                    plain = TableGroup(full, max_apply_batch=mb)
                    rows_before = [[_sorted_export([t]) for t in _tiers(sg, j)] for j in range(T)]
                    if kind == "bag":
                        la = DynamicEmbeddingBag(sg, mode=mode, optimizer=opt, lr=0.05, create_missing=True, out_dtype=dt).to(dev).train()
                        lb = DynamicEmbeddingBag(plain, mode=mode, optimizer=opt, lr=0.05, create_missing=True, out_dtype=dt).to(dev).train()
                        ot, n_out, per_step = _i64(cut, dev), T * B, 9      # 5 for the forward, 4 for the step
                        with pytest.raises(ValueError):
                            la(kt, ot, per_sample_weights=torch.ones(ks.size, device=dev))
                    else:
                        la = DynamicEmbeddingCollection(sg, optimizer=opt, lr=0.05, out_dtype=dt).to(dev).train()
                        lb = DynamicEmbeddingCollection(plain, optimizer=opt, lr=0.05, out_dtype=dt).to(dev).train()
                        ot, n_out, per_step = _i64(cut[::B].copy(), dev), ks.size, 7      # 4 for the forward, 3 for the step
                    w = torch.from_numpy(np.random.default_rng(3).standard_normal((n_out, dim)).astype(np.float32)).to(dev)
                    c0 = sg.collectives
                    oa, ob = la(kt, ot), lb(kt, ot)
                    assert oa.dtype == ob.dtype == dt and oa.shape == (n_out, dim) and torch.equal(oa.detach().float(), ob.detach().float()), (kind, opt)
                    (oa.float() * w).sum().backward()
                    (ob.float() * w).sum().backward()
                    assert sg.collectives - c0 == per_step, (kind, sg.collectives - c0)
                    assert_shards(sg, full, f"{kind} layer {opt}")
                    assert full[T - 1].size() == NK + fresh_at.size
                    moved = [False, False]      # the loss gradient reached rows of the hot and of the cold tier
                    for j in range(T):
                        for i, (tier, was) in enumerate(zip(_tiers(sg, j), rows_before[j])):
                            now = _sorted_export([tier])
                            kept = np.isin(now[0], was[0])      # (nothing was removed: the keys from before the step are all there)
                            assert int(kept.sum()) == was[0].size
                            moved[i] = moved[i] or not np.array_equal(now[1][kept], was[1])
                    assert moved == [True, True], (kind, opt)
                assert sg.traffic() == (0, 0)      # one rank keeps every segment for itself
        q.put((rank, report))
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
def test_sharded_tiered_group_two_ranks_on_one_gpu(dev):
    """ShardedTieredTableGroup over gloo (staged through host memory), two ranks on one GPU.  Collectives per call, whatever the number of pairs:
    find / find_or_insert 4, apply_adagrad / apply_adam 3, find_pooled 5, apply_pooled 4."""
    res = _launch(_gpu_rank, 2, ("gloo", 64))
    assert [r[0] for r in res] == [0, 1]
    assert sum(r[1]["traffic"][0] for r in res) == sum(r[1]["traffic"][1] for r in res)     # what all ranks sent is what all ranks received


@pytest.mark.gpu
def test_sharded_tiered_group_rccl_single_gpu_and_the_layers(dev):
    """world 1 over real RCCL; DynamicEmbeddingBag and DynamicEmbeddingCollection train one step over the sharded tiered group exactly as over the
    plain TableGroup of union tables"""
    res = _launch(_gpu_rank, 1, ("nccl", 64))
    assert [r[0] for r in res] == [0]
