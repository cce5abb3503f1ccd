"""Embedding bags over sharded table groups (SPEC.md §5 "Pooled lookups over a group"): mee_group_find_pooled_jagged, mee_group_apply_*_indexed,
TableGroup.find_pooled_jagged / apply_indexed, ShardedTableGroup.find_pooled / apply_pooled and DynamicEmbeddingBag over a ShardedTableGroup.

The yardsticks are code that is not under test: one LookupTable per member that holds the union of the member's shards (`full[j]`: find, find_pooled,
apply_*(grad_index=)), TableGroup.find_pooled on the regular layout, and numpy (fp32 adds in rank order, division by float32(length), the bf16 formula
of SPEC.md §3).  Every member stores the SAME key values with different rows, so a bag served by the wrong member gives a wrong row."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist

import oracle
from meepoembedding_amd import _lib, synth
from test_sharded_bags import _i64, np_runs, ref_pooled, same_bits
from test_sharded_bf16 import _launch
from test_sharded_groups import CAP, CONFIGS, DEFAULT, NK, CpuGroup, NpRouter, _members, _sorted_export, _world, make_batch, stored_keys

BF16 = torch.bfloat16
NEW_SYMBOLS = ("mee_group_find_pooled_jagged", "mee_group_apply_adagrad_indexed", "mee_group_apply_adam_indexed")
SHORT = (0, 0, 1, 2, 3, 7, 15)      # empty bags and bags of 1 to 15 keys: a tile per bag
LONG = 40                           # >= kPoolLong = 16: the four tiles of a wave share the bag


# ---- fixtures and the reference model -------------------------------------------------------------------------------------------
def bag_batch(seed: int, T: int, B: int, long_bags: int = 1, absent: bool = True, lens=None):
    """-> (keys int64 [n], bag_offsets int64 [T B + 1]): short and empty bags, `long_bags` bags of LONG keys, keys drawn from the stored ones with
    duplicates, ~5 % absent keys and two padding keys"""
    rng = np.random.default_rng(77 * seed + 5 * T + B)
    if lens is None:
        lens = rng.choice(SHORT, T * B)
        if T * B:
            lens[rng.choice(T * B, min(long_bags, T * B), replace=False)] = LONG
    lens = np.asarray(lens, dtype=np.int64)
    n = int(lens.sum())
    keys = stored_keys()[rng.integers(0, NK, n)].astype(np.int64)
    if absent and n > 40:
        pick = rng.choice(n, n // 20 + 2, replace=False)
        keys[pick[:-2]] = synth.keys_np(9, seed * 1000, pick.size - 2)
        keys[pick[-2:]] = oracle.EMPTY_KEY
    return keys, np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def distinct_batches(rng, G: int, T: int, Bs):
    """one batch per rank in which no key appears twice inside a member, over all ranks: no duplicate keys in any apply, inside a run or across runs"""
    lens = [rng.choice(SHORT[2:], T * B) for B in Bs]
    keys = [[] for _ in range(G)]
    for j in range(T):
        perm, at = rng.permutation(NK), 0
        for s, B in enumerate(Bs):
            m = int(lens[s][j * B:(j + 1) * B].sum())
            keys[s].append(stored_keys()[perm[at:at + m]])
            at += m
        assert at <= NK
    return [(np.concatenate(keys[s]).astype(np.int64), np.concatenate([[0], np.cumsum(lens[s])]).astype(np.int64)) for s in range(G)]


def with_fresh_bags(keys: np.ndarray, off: np.ndarray, T: int, fresh: np.ndarray):
    """the batch with `fresh` put in front of every member's keys (they join the member's first bag): the same unseen key values meet every member"""
    B = (off.size - 1) // T
    if not B:
        return keys, off
    oo = off.copy()
    for j in range(T):
        oo[j * B + 1:] += fresh.size
    return np.concatenate([np.concatenate([fresh, keys[off[j * B]:off[(j + 1) * B]]]) for j in range(T)]).astype(np.int64), oo


def ref_bags(find_rows, keys: np.ndarray, off: np.ndarray, G: int, T: int, mode: str):
    """ShardedLookupTable.find_pooled of every member with its B bags, in numpy: find_rows(j, keys) -> member j's (rows, found) for the keys;
    per bag the owners' partial sums (position order) added in rank order, the mean's division last.  -> (rows [T B, dim], found [n])"""
    B = (off.size - 1) // T
    outs, founds = [], []
    for j in range(T):
        o = off[j * B:(j + 1) * B + 1]
        kj = keys[o[0]:o[-1]]
        rows, found = find_rows(j, kj)
        owner = oracle.hash_batch(kj, 1, G)[2] if kj.size else np.zeros(0, dtype=np.int64)
        outs.append(ref_pooled(rows, owner, o - o[0], G, mode))
        founds.append(np.asarray(found).astype(bool))
    return np.concatenate(outs), np.concatenate(founds)


def np_bf16_bits(a: np.ndarray) -> np.ndarray:
    """SPEC.md §3: bf16_bits(x) = (u + 0x7FFF + ((u >> 16) & 1)) >> 16 on the fp32 bit patterns u"""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def assert_rows(got: torch.Tensor, ref: np.ndarray, dt, what):
    assert got.dtype == dt and tuple(got.shape) == ref.shape, (what, got.dtype, got.shape, ref.shape)
    if dt == torch.float32:
        same_bits(got.cpu().numpy(), ref, what)
    else:
        assert np.array_equal(got.cpu().view(torch.int16).numpy().view(np.uint16), np_bf16_bits(ref)), what


def run_counts_of(keys: np.ndarray, off: np.ndarray, G: int) -> np.ndarray:
    return np_runs(keys, off, G)[4] if keys.size else np.zeros(G, dtype=np.int64)


# ---- CPU ------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_declared_exported_and_prototyped(built):
    from test_abi_load import _declared
    names = _declared()
    L = C.CDLL(_lib.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s in names and s in _lib.PROTOTYPES and hasattr(L, s), s
    assert _lib.lib().mee_abi_version() == 2     # additive: the ABI version stays
    from meepoembedding_amd import TableGroup
    from meepoembedding_amd.sharded import ShardedTableGroup
    for m in ("find_pooled_jagged", "apply_indexed"):
        assert callable(getattr(TableGroup, m))
    for m in ("find_pooled", "apply_pooled"):
        assert callable(getattr(ShardedTableGroup, m))
    assert ShardedTableGroup.pools_with_insert is True


def test_null_arguments_are_errors_not_faults(built):
    L = _lib.lib()
    buf = (C.c_uint64 * 8)()
    assert L.mee_group_find_pooled_jagged(None, None, 0, None, 0, None, None, None, None, 0, None) == _lib.ERR_INVALID_ARG
    assert L.mee_group_find_pooled_jagged(None, buf, 2, buf, 1, buf, buf, buf, buf, 0, None) == _lib.ERR_INVALID_ARG
    assert b"null argument" in L.mee_last_error()
    assert L.mee_group_apply_adagrad_indexed(None, None, None, None, 0, None, 0, 0.01, 1e-10, None) == _lib.ERR_INVALID_ARG
    assert L.mee_group_apply_adagrad_indexed(None, buf, buf, buf, 2, buf, 2, 0.01, 1e-10, None) == _lib.ERR_INVALID_ARG
    assert L.mee_group_apply_adam_indexed(None, buf, buf, buf, 2, buf, 2, 0.01, 0.9, 0.999, 1e-8, 1, None) == _lib.ERR_INVALID_ARG
    assert L.mee_group_apply_adam_indexed(None, buf, buf, buf, 2, buf, 2, 0.01, 0.9, 0.999, 1e-8, 0, None) == _lib.ERR_INVALID_ARG      # step 0
    assert L.mee_group_apply_adagrad_indexed(None, buf, buf, buf, 0, buf, 2, 0.01, 1e-10, None) == _lib.ERR_INVALID_ARG                 # no grad rows
    assert L.mee_group_apply_adagrad_indexed(None, buf, buf, buf, 2, None, 2, 0.01, 1e-10, None) == _lib.ERR_INVALID_ARG                # null index


class NpBagRouter(NpRouter):
    """NpRouter plus the three bag steps in numpy: the host logic of ShardedTableGroup's pooled forms runs without a GPU"""

    def bag_runs(self, perm, counts, bag_offsets):
        n, off, c = perm.numel(), bag_offsets.numpy(), counts.numpy()
        run_bag, run_len, run_counts = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros(self.n_shards, dtype=np.int64)
        base = at = 0
        for p in range(self.n_shards):
            b = np.searchsorted(off, perm.numpy()[base:base + c[p]], side="right") - 1
            base += c[p]
            if b.size:
                heads = np.flatnonzero(np.concatenate([[True], b[1:] != b[:-1]]))
                run_bag[at:at + heads.size] = b[heads]
                run_len[at:at + heads.size] = np.diff(np.concatenate([heads, [b.size]]))
                run_counts[p] = heads.size
                at += heads.size
        return torch.from_numpy(run_bag), torch.from_numpy(run_len), torch.from_numpy(run_counts)

    def run_offsets(self, run_len, n_keys=None):
        rl = run_len.numpy().astype(np.int64)
        off = torch.from_numpy(np.concatenate([[0], np.cumsum(rl)]).astype(np.int64))
        return off, (None if n_keys is None else torch.from_numpy(np.repeat(np.arange(rl.size), rl).astype(np.int32)))

    def combine_bag_runs(self, partials, run_bag, run_counts, bag_offsets, mode="sum", out=None, out_dtype=torch.float32):
        off, p, rb = bag_offsets.numpy(), partials.numpy(), run_bag.numpy()
        res, seen, at = np.zeros((off.size - 1, p.shape[1]), dtype=np.float32), np.zeros(off.size - 1, dtype=bool), 0
        for c in run_counts.tolist():        # rank order; an owner has at most one run per bag
            for r in range(at, at + c):
                res[rb[r]] = (res[rb[r]] + p[r]).astype(np.float32) if seen[rb[r]] else p[r]
                seen[rb[r]] = True
            at += c
        if mode == "mean":
            lens = np.diff(off)
            res[lens > 0] = (res[lens > 0] / lens[lens > 0, None].astype(np.float32)).astype(np.float32)
        return torch.from_numpy(res).to(out_dtype)


class CpuBagGroup(CpuGroup):
    """the definitions: LookupTable.find_pooled / apply_*(grad_index=) per member, over CpuTable"""

    def find_or_insert(self, keys, offsets):
        parts = [t.find_or_insert(keys[a:b]) for t, a, b in self._each(offsets)]
        return torch.cat([x[0] for x in parts]), torch.cat([x[1] for x in parts])

    def find_pooled_jagged(self, keys, bag_offsets, member_bags, mode="sum"):
        off, mb = bag_offsets.numpy(), member_bags.tolist()
        outs, founds = [], []
        for j, t in enumerate(self.tables):
            o = off[mb[j]:mb[j + 1] + 1]
            rows, found = t.find(keys[o[0]:o[-1]])
            outs.append(torch.from_numpy(oracle.pool_rows(rows.numpy(), o - o[0], mode)))
            founds.append(found)
        return torch.cat(outs), torch.cat(founds)

    def apply_indexed(self, keys, offsets, grads, grad_index, optimizer, lr, eps=None, beta1=0.9, beta2=0.999, step=1):
        assert optimizer == "adagrad"      # the CPU run checks the host logic, which does not depend on the optimizer; Adam runs in the GPU tests
        for t, a, b in self._each(offsets):
            t.apply_adagrad(keys[a:b], grads[grad_index[a:b].to(torch.int64)], lr, 1e-10 if eps is None else eps)


def _cpu_rank(rank, world, port, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        from _cpu_backend import CpuTable
        from meepoembedding_amd.sharded import ShardedTableGroup
        dist.init_process_group("gloo", rank=rank, world_size=world)
        dim, st = 4, stored_keys()
        mine = oracle.hash_batch(st, 1, world)[2] == rank
        for T in (1, 5):
            def member(j, part):
                t = CpuTable(CAP, dim, optimizer=oracle.OPT_ADAGRAD, default_value=DEFAULT, initial_accumulator=0.1)
                t.insert(torch.from_numpy(st[part]), torch.from_numpy(synth.rows_np(st[part], dim, 2 + j)))
                return t
            sg = ShardedTableGroup(CpuBagGroup([member(j, mine) for j in range(T)]), NpBagRouter(world))
            full = [member(j, slice(None)) for j in range(T)]
            batches = [bag_batch(30 + r, T, 2 + r) for r in range(world)]      # B differs from rank to rank
            keys, off = batches[rank] if rank else (np.zeros(0, dtype=np.int64), np.zeros(1, dtype=np.int64))     # rank 0: no keys and no bags
            kt, ot = torch.from_numpy(keys), torch.from_numpy(off)
            n_bags = off.size - 1
            g = torch.from_numpy((synth.rows_np(np.arange(n_bags, dtype=np.int64), dim, 6 + rank) * 0.02).astype(np.float32)).view(n_bags, dim)
            bag_of = torch.from_numpy(np.repeat(np.arange(n_bags), np.diff(off)))
            # refused on every rank alike, before anything is exchanged
            bad_off = torch.cat([ot, ot[-1:]]) if T > 1 else ot[:0]
            for bad in (lambda: sg.find_pooled(kt, ot, "max"), lambda: sg.find_pooled(kt, ot, out_dtype=torch.float16),
                        lambda: sg.find_pooled(kt, bad_off),
                        lambda: ShardedTableGroup(sg.local_group, NpRouter(world)).find_pooled(kt, ot),                        # no bag_runs
                        lambda: ShardedTableGroup(CpuGroup(sg.tables), sg.router).find_pooled(kt, ot),                         # no find_pooled_jagged
                        lambda: ShardedTableGroup(CpuGroup(sg.tables), sg.router).apply_pooled(kt, ot, g, bag_of, "adagrad", 0.01),      # no apply_indexed
                        lambda: sg.apply_pooled(kt, ot, g, torch.cat([bag_of, bag_of.new_zeros(1)]), "adagrad", 0.01),
                        lambda: sg.apply_pooled(kt, bad_off, g, bag_of, "adagrad", 0.01),
                        lambda: sg.apply_pooled(kt, ot, g, bag_of, "sgd", 0.01)):
                with pytest.raises(ValueError):
                    bad()
            assert sg.traffic() == (0, 0) and sg.collectives == 0
            find_rows = lambda j, k: tuple(x.numpy() for x in full[j].find(torch.from_numpy(k)))
            for n_call, mode in enumerate(("sum", "mean")):
                t0 = sg.traffic()
                rows, found = sg.find_pooled(kt, ot, mode)
                assert sg.collectives == 5 * (n_call + 1), (T, sg.collectives)      # the cells, keys out, run lengths out, partial rows back, found back
                er, ef = ref_bags(find_rows, keys, off, world, T, mode)
                same_bits(rows.numpy(), er, f"T={T} {mode}")
                assert np.array_equal(found.numpy().astype(bool), ef)
                t1 = sg.traffic()
            # traffic(): keys 8 B and run lengths 4 B out, a partial row per run and a byte per key back, and the [G, 2 T] cells
            to = np.bincount(oracle.hash_batch(keys, 1, world)[2], minlength=world) if keys.size else np.zeros(world, dtype=np.int64)
            ro = run_counts_of(keys, off, world)
            every = [None] * world
            dist.all_gather_object(every, (to.tolist(), ro.tolist()))
            k_out, r_out = int(to.sum() - to[rank]), int(ro.sum() - ro[rank])
            k_in = sum(every[s][0][rank] for s in range(world) if s != rank)
            r_in = sum(every[s][1][rank] for s in range(world) if s != rank)
            cnt = 16 * T * (world - 1)
            assert (t1[0] - t0[0], t1[1] - t0[1]) == (8 * k_out + 4 * r_out + 4 * dim * r_in + k_in + cnt,
                                                      8 * k_in + 4 * r_in + 4 * dim * r_out + k_out + cnt), (T, k_out, r_out, k_in, r_in)
            t0 = sg.traffic()
            sg.apply_pooled(kt, ot, g, bag_of, "adagrad", 0.01, located=torch.zeros(3))      # located: accepted and ignored
            assert sg.collectives == 14                                                      # + the cells, keys out, run lengths out, run rows out
            t1 = sg.traffic()
            assert (t1[0] - t0[0], t1[1] - t0[1]) == (8 * k_out + (4 + 4 * dim) * r_out + cnt, 8 * k_in + (4 + 4 * dim) * r_in + cnt)
            for j in range(T):       # the reference gets every rank's keys of member j, each with its bag's gradient row
                kk, gg = [], []
                for r in range(1, world):
                    k_r, o_r = batches[r]
                    B = (o_r.size - 1) // T
                    g_r = (synth.rows_np(np.arange(o_r.size - 1, dtype=np.int64), dim, 6 + r) * 0.02).astype(np.float32).reshape(-1, dim)
                    kk.append(k_r[o_r[j * B]:o_r[(j + 1) * B]])
                    gg.append(g_r[np.repeat(np.arange(o_r.size - 1), np.diff(o_r))][o_r[j * B]:o_r[(j + 1) * B]])
                full[j].apply_adagrad(torch.from_numpy(np.concatenate(kk)), torch.from_numpy(np.concatenate(gg)), 0.01)
                ek, ev, ea, _ = full[j].export(with_state=True)
                gk, gv, ga, _ = sg.tables[j].export(with_state=True)
                sel = torch.from_numpy(oracle.hash_batch(ek.numpy(), 1, world)[2] == rank)
                io, ig = torch.argsort(ek[sel]), torch.argsort(gk)
                assert torch.equal(ek[sel][io], gk[ig])
                np.testing.assert_allclose(gv[ig].numpy(), ev[sel][io].numpy(), rtol=1e-6, atol=1e-9)
                np.testing.assert_allclose(ga[ig].numpy(), ea[sel][io].numpy(), rtol=1e-6, atol=1e-9)
        q.put((rank, sg.traffic()))
        dist.barrier()
        dist.destroy_process_group()
    except BaseException as e:
        import traceback
        q.put(("error", rank, "".join(traceback.format_exception(type(e), e, e.__traceback__))))
        raise


@pytest.mark.parametrize("world", [2, 3])
def test_host_logic_collectives_traffic_and_refusals_without_a_gpu(built, world):
    res = _launch(_cpu_rank, world, (), first_timeout=120)
    assert sum(r[1][0] for r in res) == sum(r[1][1] for r in res)     # what all ranks sent is what all ranks received


def test_the_layer_refuses_weights_over_a_sharded_group_before_any_exchange(built):
    from meepoembedding_amd import nn as mnn
    from meepoembedding_amd.sharded import ShardedTableGroup
    sg = ShardedTableGroup.__new__(ShardedTableGroup)      # (no process group: the refusal must not need one)
    sg.local = sg.local_group = type("G", (), {"dim": 4, "tables": [None], "supports_out_dtype": False})()
    sg.dim, sg.n_tables, sg.collectives = 4, 1, 0
    layer = mnn.DynamicEmbeddingBag(sg, mode="sum")
    with pytest.raises(ValueError, match="per_sample_weights"):
        layer(torch.zeros(3, dtype=torch.int64), torch.tensor([0, 3]), per_sample_weights=torch.ones(3))
    assert sg.collectives == 0


# ---- GPU, one process: the jagged lookup against LookupTable.find_pooled per member ------------------------------------------------
def _member_maps(T: int, n_bags: int, rng):
    """name -> member_bags [T + 1] over n_bags bags"""
    def from_counts(active):
        counts = np.zeros(T, dtype=np.int64)
        counts[active] = np.diff(np.concatenate([[0], np.sort(rng.integers(0, n_bags + 1, len(active) - 1)), [n_bags]]))
        return np.concatenate([[0], np.cumsum(counts)])
    maps = {"random": from_counts(list(range(T))), "one member has all": from_counts([T // 2])}
    if n_bags % T == 0:
        maps["regular"] = np.arange(T + 1) * (n_bags // T)
    if T >= 3:       # members without bags at both ends and in the middle
        maps["empty ends"] = from_counts(list(range(1, T - 1)))
        maps["empty middle"] = from_counts([j for j in range(T) if j != T // 2])
    if T >= 5:
        maps["empty ends and middle"] = from_counts([j for j in range(T) if j not in (0, T // 2, T - 1)])
    maps["outside"] = np.clip(maps["random"], 2, max(n_bags - 3, 2))      # bags below the first and at or beyond the last offset: empty bags
    return {k: np.asarray(v, dtype=np.int64) for k, v in maps.items()}


def _bag_sets(T: int, seed: int):
    """name -> (keys, bag_offsets)"""
    rng = np.random.default_rng(seed)
    # empty bags, every short length and long bags side by side, shuffled: the hybrid shape
    sets = {"mixed": bag_batch(seed, T, 12, lens=rng.permutation(np.resize(SHORT + (LONG,), T * 12))),
            # the four tiles of a wave serve four different members, one of them with a long bag
            "one bag per member": bag_batch(seed + 1, T, 1, lens={1: [7], 3: [3, 16, 1], 5: [3, 16, 0, 7, 15]}[T]),
            "no keys": (np.zeros(0, dtype=np.int64), np.zeros(T * 3 + 1, dtype=np.int64)),
            "no bags": (np.zeros(0, dtype=np.int64), np.zeros(1, dtype=np.int64))}
    lens = rng.integers(12, 30, T * 4)                                                    # an average bag >= 12 keys: the wave-per-bag shape
    lens[1] = 0
    lens[2] = 70
    k = stored_keys()[rng.integers(0, NK, int(lens.sum()))].astype(np.int64)
    k[5], k[17] = synth.keys_np(9, seed, 1)[0], oracle.EMPTY_KEY
    sets["long average"] = (k, np.concatenate([[0], np.cumsum(lens)]).astype(np.int64))
    return sets


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 3, 5])
@pytest.mark.parametrize("dim", [4, 64, 24])
def test_jagged_lookup_against_find_pooled_per_member(dev, dim, T):
    from meepoembedding_amd import OPT_NONE, TableGroup
    full = _members(T, dim, dev, OPT_NONE, slice(None), 4096)
    group = TableGroup(full)
    rng = np.random.default_rng(dim + T)
    CAN = -3.5
    for sname, (keys, off) in _bag_sets(T, 40 + T).items():
        n, n_bags = keys.size, off.size - 1
        if sname == "long average":
            assert n // n_bags >= 12
        elif sname in ("mixed", "one bag per member"):      # the hybrid launch shape; "mixed": empty, short and long bags side by side
            assert n // n_bags < 12 and (sname != "mixed" or ((np.diff(off) >= 16).any() and (np.diff(off) == 0).any() and (np.diff(off) == 1).any()))
        kt, ot = _i64(keys, dev), _i64(off, dev)
        for mname, mb in _member_maps(T, n_bags, rng).items():
            for mode in ("sum", "mean"):
                out = torch.full((n_bags + 2, dim), CAN, device=dev)
                found = torch.full((n + 5,), 7, dtype=torch.uint8, device=dev)
                loc = torch.full((n + 3,), -7, dtype=torch.int64, device=dev)
                r_out, r_found = group.find_pooled_jagged(kt, ot, _i64(mb, dev), mode, out=out[:n_bags], found=found[:n], located=loc[:n])
                what = (sname, mname, mode, dim, T, mb.tolist())
                assert r_out.shape == (n_bags, dim) and r_found.shape == (n,)      # the caller's buffers, checked below with their canaries
                # canaries behind every output
                assert bool((out[n_bags:] == CAN).all()) and bool((found[n:] == 7).all()) and bool((loc[n:] == -7).all()), what
                lo_all, hi_all = min(int(mb[0]), n_bags), min(int(mb[-1]), n_bags)
                for j in range(T):
                    lo, hi = min(int(mb[j]), n_bags), min(int(mb[j + 1]), n_bags)
                    if hi <= lo:
                        continue
                    a, b = int(off[lo]), int(off[hi])
                    er, ef = full[j].find_pooled(kt[a:b], (ot[lo:hi + 1] - a).contiguous(), mode)
                    same_bits(out[lo:hi].cpu().numpy(), er.cpu().numpy(), str(what + (j,)))
                    assert torch.equal(found[a:b], ef), what + (j,)
                # bags outside the map: rows of zeros, nothing probed (their found bytes and handles are left alone)
                for lo, hi in ((0, lo_all), (hi_all, n_bags)):
                    if hi > lo:
                        assert bool((out[lo:hi] == 0).all()) and bool((found[off[lo]:off[hi]] == 7).all()) and bool((loc[off[lo]:off[hi]] == -7).all()), what
                if mname == "regular":      # == mee_group_find_pooled(bags_per_table = B) bit for bit, handles included
                    loc2 = torch.full((n,), -7, dtype=torch.int64, device=dev)
                    o2, f2 = group.find_pooled(kt, ot, mode, located=loc2)
                    assert torch.equal(o2.view(torch.int32), out[:n_bags].view(torch.int32)) and torch.equal(f2, found[:n]) and torch.equal(loc2, loc[:n]), what
    torch.cuda.synchronize(dev)


@pytest.mark.gpu
def test_jagged_lookup_refusals_on_the_device(dev):
    from meepoembedding_amd import MeepoError, OPT_NONE, TableGroup
    T, dim = 3, 4
    group = TableGroup(_members(T, dim, dev, OPT_NONE, slice(None), 4096))
    keys, off = bag_batch(3, T, 2)
    kt, ot, mb = _i64(keys, dev), _i64(off, dev), _i64([0, 2, 4, 6], dev)
    L, st = _lib.lib(), torch.cuda.current_stream(dev).cuda_stream
    out = torch.empty((6, dim), device=dev)
    assert L.mee_group_find_pooled_jagged(group._h, kt.data_ptr(), kt.numel(), ot.data_ptr(), 6, None, out.data_ptr(), None, None, 0, st) == _lib.ERR_INVALID_ARG
    assert L.mee_group_find_pooled_jagged(group._h, kt.data_ptr(), kt.numel(), ot.data_ptr(), 6, mb.data_ptr(), None, None, None, 0, st) == _lib.ERR_INVALID_ARG
    assert L.mee_group_find_pooled_jagged(group._h, kt.data_ptr(), kt.numel(), ot.data_ptr(), 6, mb.data_ptr(), out.data_ptr(), None, None, 2, st) == _lib.ERR_INVALID_ARG
    assert L.mee_group_find_pooled_jagged(group._h, None, 0, None, 0, None, None, None, None, 0, st) == _lib.OK      # no bags: nothing to do
    with pytest.raises(MeepoError):
        group.find_pooled_jagged(kt, ot, mb[:-1])
    with pytest.raises(ValueError):
        group.find_pooled_jagged(kt, ot, mb, out=torch.empty((6, dim), dtype=BF16, device=dev))
    # found and located are optional
    o1, _ = group.find_pooled_jagged(kt, ot, mb)
    _lib.check(L.mee_group_find_pooled_jagged(group._h, kt.data_ptr(), kt.numel(), ot.data_ptr(), 6, mb.data_ptr(), out.data_ptr(), None, None, 0, st))
    assert torch.equal(o1, out)
    torch.cuda.synchronize(dev)


# ---- GPU, one process: the indexed group apply against apply_*(grad_index=) per member --------------------------------------------
def _apply_both(group, full, opt, kt, ot, g, gi, n_step):
    group.apply_indexed(kt, ot, g, gi, opt, 0.01, beta1=0.9, beta2=0.999, step=n_step)
    o = ot.tolist()
    for j, t in enumerate(full):
        if o[j + 1] > o[j]:
            if opt == "adagrad":
                t.apply_adagrad(kt[o[j]:o[j + 1]], g, 0.01, 1e-10, grad_index=gi[o[j]:o[j + 1]])
            else:
                t.apply_adam(kt[o[j]:o[j + 1]], g, 0.01, 0.9, 0.999, 1e-8, n_step, grad_index=gi[o[j]:o[j + 1]])


@pytest.mark.gpu
@pytest.mark.parametrize("opt", ["adagrad", "adam"])
@pytest.mark.parametrize("T,dim", [(3, 4), (5, 64), (1, 24)])
def test_indexed_group_apply_against_the_member_tables(dev, T, dim, opt):
    from meepoembedding_amd import OPT_ADAGRAD, OPT_ADAM
    groups, full = _world(1, T, dim, dev, OPT_ADAGRAD if opt == "adagrad" else OPT_ADAM)
    rng = np.random.default_rng(T + dim)
    st = stored_keys()
    R = 37
    g = torch.from_numpy(rng.standard_normal((R, dim)).astype(np.float32) * 0.02).to(dev)
    for n_step in (1, 2):      # no duplicate keys inside a member: bit-identical, state planes included
        lens = rng.integers(0, 400, T)
        lens[rng.integers(0, T)] = 0 if T > 1 else 300
        keys = np.concatenate([st[rng.permutation(NK)[:l]] for l in lens]).astype(np.int64)
        gi = rng.integers(0, R, keys.size).astype(np.int32)
        gi[:3] = R + 5                                   # indices >= n_grad_rows clamp, in the group as in a table
        _apply_both(groups[0], full, opt, _i64(keys, dev), _i64(np.concatenate([[0], np.cumsum(lens)]), dev), g, torch.from_numpy(gi).to(dev), n_step)
    for j in range(T):
        got, exp = _sorted_export([groups[0].tables[j]]), _sorted_export([full[j]])
        assert np.array_equal(got[0], exp[0]) and len(got) == len(exp) == (3 if opt == "adagrad" else 4)
        for x, y in zip(got[1:], exp[1:]):
            same_bits(x, y, f"{opt} T={T} member {j}")
    keys, off = make_batch("plain", 60, 1, T)           # duplicates inside and across segments, absent and padding keys
    gi = torch.from_numpy(rng.integers(0, R, keys.size).astype(np.int32)).to(dev)
    _apply_both(groups[0], full, opt, _i64(keys, dev), _i64(off, dev), g, gi, 3)
    for j in range(T):
        got, exp = _sorted_export([groups[0].tables[j]]), _sorted_export([full[j]])
        assert np.array_equal(got[0], exp[0])
        for x, y in zip(got[1:], exp[1:]):
            np.testing.assert_allclose(x, y, rtol=1e-6, atol=1e-9, err_msg=f"{opt} member {j}")      # SPEC.md §4's contract
    # the refusals of mee_group_apply_* and of mee_apply_*_indexed
    from meepoembedding_amd import MeepoError
    kt, ot = _i64(keys, dev), _i64(off, dev)
    with pytest.raises(MeepoError):
        groups[0].apply_indexed(kt, ot, g, gi, "adam" if opt == "adagrad" else "adagrad", 0.01)      # the other optimizer's planes
    with pytest.raises(MeepoError):
        groups[0].apply_indexed(kt, ot[:-1], g, gi, opt, 0.01)
    with pytest.raises(MeepoError):
        groups[0].apply_indexed(kt, ot, g, gi[:-1], opt, 0.01)
    with pytest.raises(MeepoError):
        groups[0].apply_indexed(kt, ot, g[:0], gi, opt, 0.01)
    torch.cuda.synchronize(dev)


# ---- GPU, one process: the operators with every owner played in turn -------------------------------------------------------------
def _emulate_bags(router, groups, batches, on_owner, run_payload=None):
    """the exchange in one process: batches[s] = rank s's (keys, bag_offsets) on the device.  What crosses the link in ShardedTableGroup's pooled
    forms is sliced and concatenated here; on_owner(p, keys_tm, offsets_tm, run_len_tm, member_bags, run rows table-major or None) -> (partial rows
    per table-major run, found per table-major key) or None.  -> per rank (partial rows in run order, found in batch order, run_bag, run_counts)"""
    G, T = len(groups), len(groups[0].tables)
    routed = []
    for s, (kt, ot) in enumerate(batches):
        B = (ot.numel() - 1) // T
        send, counts, perm = router.partition(kt)
        run_bag, run_len, run_counts = router.bag_runs(perm, counts, ot)
        kc = router.segment_counts(perm, counts, ot[::B].contiguous() if B else ot.new_zeros(T + 1))
        rc = router.segment_counts(run_bag.to(torch.int64), run_counts, torch.arange(T + 1, dtype=torch.int64, device=kt.device) * B)
        r = int(run_counts.sum())
        assert int(kc.sum()) == kt.numel() and int(rc.sum()) == r and torch.equal(rc.sum(dim=1), run_counts) and torch.equal(kc.sum(dim=1), counts)
        pay = None if run_payload is None else router.gather_rows(run_payload[s], run_bag[:r].to(torch.int64))
        routed.append(dict(send=send, perm=perm, c=counts.tolist(), rn=run_counts.tolist(), run_bag=run_bag[:r], run_len=run_len[:r],
                           run_counts=run_counts, kc=kc, rc=rc, pay=pay))
    back = [[None] * G for _ in range(G)]
    for p in range(G):
        klo, rlo = [sum(x["c"][:p]) for x in routed], [sum(x["rn"][:p]) for x in routed]
        recv = torch.cat([x["send"][a:a + x["c"][p]] for x, a in zip(routed, klo)])
        recv_len = torch.cat([x["run_len"][a:a + x["rn"][p]] for x, a in zip(routed, rlo)])
        pay = None if run_payload is None else torch.cat([x["pay"][a:a + x["rn"][p]] for x, a in zip(routed, rlo)])
        keys_tm, order, off_tm = router.regroup(recv, torch.stack([x["kc"][p] for x in routed]))
        _, order_r, member_bags = router.regroup(recv[:recv_len.numel()], torch.stack([x["rc"][p] for x in routed]))
        run_len_tm = router.gather_rows(recv_len, order_r)
        res = on_owner(p, keys_tm, off_tm, run_len_tm, member_bags, None if pay is None else router.gather_rows(pay, order_r))
        if res is not None:
            pb, fb = router.scatter_rows(res[0], order_r), router.scatter_rows(res[1], order)
            ka = ra = 0
            for s, x in enumerate(routed):
                back[s][p] = (pb[ra:ra + x["rn"][p]], fb[ka:ka + x["c"][p]])
                ka += x["c"][p]
                ra += x["rn"][p]
    if back[0][0] is None:
        return None
    return [(torch.cat([back[s][p][0] for p in range(G)]), router.scatter_rows(torch.cat([back[s][p][1] for p in range(G)]), x["perm"]),
             x["run_bag"], x["run_counts"]) for s, x in enumerate(routed)]


def _gpu_find_rows(full, dev, dim):
    def find_rows(j, k):
        if not k.size:
            return np.zeros((0, dim), dtype=np.float32), np.zeros(0, dtype=bool)
        return tuple(x.cpu().numpy() for x in full[j].find(_i64(k, dev)))
    return find_rows


def _bag_rows(n_bags, dim, seed):
    return (synth.rows_np(np.arange(n_bags, dtype=np.int64), dim, seed).reshape(n_bags, dim) * 0.02).astype(np.float32)


def _reference_step(full, batches_np, T, dim, dev, opt, n_step, seed0):
    """member j of the reference: every rank's keys of member j in rank order, each with its bag's gradient row (apply_*(grad_index=))"""
    for j in range(T):
        ks, gs, gis, base = [], [], [], 0
        for s, (k, o) in enumerate(batches_np):
            B = (o.size - 1) // T
            ks.append(k[o[j * B]:o[(j + 1) * B]])
            gs.append(_bag_rows(o.size - 1, dim, seed0 + s)[j * B:(j + 1) * B])
            gis.append(base + np.repeat(np.arange(B), np.diff(o[j * B:(j + 1) * B + 1])))
            base += B
        ks, gs, gis = np.concatenate(ks), np.concatenate(gs), np.concatenate(gis)
        if not ks.size:
            continue
        args = (_i64(ks, dev), torch.from_numpy(gs).to(dev))
        gi = torch.from_numpy(gis.astype(np.int32)).to(dev)
        if opt == "adagrad":
            full[j].apply_adagrad(*args, 0.01, 1e-10, grad_index=gi)
        else:
            full[j].apply_adam(*args, 0.01, 0.9, 0.999, 1e-8, n_step, grad_index=gi)


@pytest.mark.gpu
@pytest.mark.parametrize("G,T,dim", CONFIGS)
def test_emulated_find_pooled_against_the_member_tables(dev, G, T, dim):
    from meepoembedding_amd import OPT_NONE, Router
    router = Router(G, 2048, device=dev)
    groups, full = _world(G, T, dim, dev, OPT_NONE)
    find_rows = _gpu_find_rows(full, dev, dim)
    batches_np = [bag_batch(50 + s, T, 2 + s) for s in range(G)]      # B differs from rank to rank
    if G > 1:
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
                out = router.combine_bag_runs(partial, run_bag, run_counts, ot, mode, out_dtype=dt)
                assert_rows(out, er, dt, f"G={G} T={T} dim={dim} rank {s} {mode} {dt}")
            assert np.array_equal(found.cpu().numpy().astype(bool), ef)
        if G == 1:      # one rank: TableGroup.find_pooled, bit for bit
            o1, f1 = groups[0].find_pooled(kt, ot, "mean")
            assert torch.equal(o1.view(torch.int32), router.combine_bag_runs(partial, run_bag, run_counts, ot, "mean").view(torch.int32)) and torch.equal(f1, found)
    if T > 1 and G > 1:
        out = router.combine_bag_runs(got[-1][0], got[-1][2], got[-1][3], batches[-1][1], "sum")
        assert not torch.equal(out[:3], out[-3:])
    # insert_missing: keys no table has seen, overlapping between the ranks and meeting every member; found = present before
    fresh_np = [with_fresh_bags(k, o, T, synth.keys_np(77, 10 * s, 40)) for s, (k, o) in enumerate(batches_np)]
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
    for j in range(T):      # afterwards every shard holds exactly the union's keys that it owns
        ek = full[j].export()[0].cpu().numpy()
        per = np.bincount(oracle.hash_batch(ek, 1, G)[2], minlength=G)
        assert [groups[p].tables[j].size() for p in range(G)] == per.tolist() and full[j].size() > NK
    torch.cuda.synchronize(dev)


@pytest.mark.gpu
@pytest.mark.parametrize("opt", ["adagrad", "adam"])
@pytest.mark.parametrize("G,T,dim", CONFIGS)
def test_emulated_apply_pooled_against_the_member_tables(dev, G, T, dim, opt):
    """a step without duplicate keys (the keys of every bag distinct, no key twice in a member over all ranks): bit-identical to the member tables,
    state planes included; a second step that repeats keys inside a rank and across ranks: within SPEC §4's tolerance"""
    from meepoembedding_amd import OPT_ADAGRAD, OPT_ADAM, Router
    router = Router(G, 2048, device=dev)
    groups, full = _world(G, T, dim, dev, OPT_ADAGRAD if opt == "adagrad" else OPT_ADAM)
    rng = np.random.default_rng(G * 10 + T)

    def step(batches_np, n_step):
        batches = [(_i64(k, dev), _i64(o, dev)) for k, o in batches_np]
        pays = [torch.from_numpy(_bag_rows(o.size - 1, dim, 20 + n_step + s)).to(dev) for s, (_, o) in enumerate(batches_np)]

        def on_owner(p, k, o, run_len, member_bags, rows):
            _, run_of_key = router.run_offsets(run_len, k.numel())
            groups[p].apply_indexed(k, o, rows, run_of_key, opt, 0.01, beta1=0.9, beta2=0.999, step=n_step)
        assert _emulate_bags(router, groups, batches, on_owner, pays) is None
        _reference_step(full, batches_np, T, dim, dev, opt, n_step, 20 + n_step)

    step(distinct_batches(rng, G, T, [2 + s for s in range(G)]), 1)
    for j in range(T):
        got, exp = _sorted_export([groups[p].tables[j] for p in range(G)]), _sorted_export([full[j]])
        assert np.array_equal(got[0], exp[0]) and len(got) == len(exp) == (3 if opt == "adagrad" else 4)
        for x, y in zip(got[1:], exp[1:]):
            same_bits(x, y, f"{opt} G={G} T={T} member {j}")
    dup = [bag_batch(70 + s, T, 2 + s) for s in range(G)]
    dup = [(np.concatenate([dup[0][0][:30], k]), np.concatenate([[0], o[1:] + 30])) for k, o in dup]      # every rank repeats rank 0's first keys
    step(dup, 2)
    for j in range(T):
        got, exp = _sorted_export([groups[p].tables[j] for p in range(G)]), _sorted_export([full[j]])
        assert np.array_equal(got[0], exp[0])
        for x, y in zip(got[1:], exp[1:]):
            np.testing.assert_allclose(x, y, rtol=1e-6, atol=1e-9, err_msg=f"{opt} member {j}")      # SPEC.md §4's contract
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
    from meepoembedding_amd import OPT_ADAGRAD, OPT_ADAM, Router, TableGroup
    from meepoembedding_amd.nn import DynamicEmbeddingBag
    from meepoembedding_amd.sharded import ShardedTableGroup
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        mine = oracle.hash_batch(stored_keys(), 1, world)[2] == rank
        mb = max(world * 2048, 4096)

        def make(T, optimizer=OPT_ADAGRAD):
            sg = ShardedTableGroup(TableGroup(_members(T, dim, dev, optimizer, mine, mb), max_apply_batch=mb), Router(world, 2048, device=dev))
            return sg, _members(T, dim, dev, optimizer, slice(None), mb)

        def wire(batches):
            """-> (k_out, k_in, r_out, r_in) of this rank for the batches of all ranks"""
            to = [np.bincount(oracle.hash_batch(k, 1, world)[2], minlength=world) if k.size else np.zeros(world, dtype=np.int64) for k, _ in batches]
            ro = [run_counts_of(k, o, world) for k, o in batches]
            return (int(to[rank].sum() - to[rank][rank]), int(sum(to[s][rank] for s in range(world) if s != rank)),
                    int(ro[rank].sum() - ro[rank][rank]), int(sum(ro[s][rank] for s in range(world) if s != rank)))

        report = {}
        for T in (1, 5):
            sg, full = make(T)
            find_rows = _gpu_find_rows(full, dev, dim)
            dist.barrier()
            batches = [bag_batch(80 + r, T, 2 + r) for r in range(world)]      # every rank can rebuild every rank's batch; B differs per rank
            keys, off = batches[rank]
            kt, ot = _i64(keys, dev), _i64(off, dev)
            # ---- refusals: on every rank alike, before any collective ----
            bag_of = torch.repeat_interleave(torch.arange(off.size - 1, device=dev), ot[1:] - ot[:-1])
            g = torch.from_numpy(_bag_rows(off.size - 1, dim, 6)).to(dev)
            for bad in (lambda: sg.find_pooled(kt, ot, "max"), lambda: sg.find_pooled(kt, ot, out_dtype=torch.float16),
                        lambda: sg.find_pooled(kt, torch.cat([ot, ot[-1:]]) if T > 1 else ot[:0]),
                        lambda: sg.apply_pooled(kt, ot, g, bag_of[:-1], "adagrad", 0.01), lambda: sg.apply_pooled(kt, ot, g[:-1], bag_of, "adagrad", 0.01)):
                with pytest.raises(ValueError):
                    bad()
            assert sg.collectives == 0 and sg.traffic() == (0, 0)
            # ---- find_pooled: sum and mean, fp32 and bf16; 5 collectives whatever T is; wire bytes ----
            k_out, k_in, r_out, r_in = wire(batches)
            cnt = 16 * T * (world - 1)
            for mode in ("sum", "mean"):
                er, ef = ref_bags(find_rows, keys, off, world, T, mode)
                for dt in (torch.float32, BF16):
                    c0, t0 = sg.collectives, sg.traffic()
                    rows, found = sg.find_pooled(kt, ot, mode, out_dtype=dt)
                    assert sg.collectives - c0 == 5, (T, sg.collectives - c0)
                    t1 = sg.traffic()
                    assert (t1[0] - t0[0], t1[1] - t0[1]) == (8 * k_out + 4 * r_out + 4 * dim * r_in + k_in + cnt,
                                                              8 * k_in + 4 * r_in + 4 * dim * r_out + k_out + cnt), (T, mode, dt)
                    assert_rows(rows, er, dt, f"T={T} {mode} {dt}")
                    assert np.array_equal(found.cpu().numpy().astype(bool), ef)
            if world == 1:      # one rank: TableGroup.find_pooled, bit for bit
                o1, f1 = TableGroup(full).find_pooled(kt, ot, "mean", out_dtype=BF16)
                o2, f2 = sg.find_pooled(kt, ot, "mean", out_dtype=BF16)
                assert torch.equal(o1.view(torch.int16), o2.view(torch.int16)) and torch.equal(f1, f2)
            # ---- rank 0 has no keys (and, for T = 5, no bags either) ----
            if rank == 0:
                k0, o0 = np.zeros(0, dtype=np.int64), np.zeros(1 if T == 5 else 3 * T + 1, dtype=np.int64)
            else:
                k0, o0 = keys, off
            rows, found = sg.find_pooled(_i64(k0, dev), _i64(o0, dev), "mean")
            er, ef = ref_bags(find_rows, k0, o0, world, T, "mean")
            assert_rows(rows, er, torch.float32, f"T={T} rank 0 empty")
            assert np.array_equal(found.cpu().numpy().astype(bool), ef)
            # ---- insert_missing: fresh keys overlap between the ranks; found = present before; sizes afterwards ----
            def with_fresh(r):
                return with_fresh_bags(*batches[r], T, synth.keys_np(77, 10 * r, 40))
            fk, fo = with_fresh(rank)
            before = ref_bags(find_rows, fk, fo, world, T, "sum")[1]
            c0 = sg.collectives
            rows, found = sg.find_pooled(_i64(fk, dev), _i64(fo, dev), "sum", insert_missing=True, out_dtype=BF16)
            assert sg.collectives - c0 == 5
            for r in range(world):       # the reference creates every rank's keys
                k, o = with_fresh(r)
                B = (o.size - 1) // T
                for j in range(T):
                    full[j].find_or_insert(_i64(k[o[j * B]:o[(j + 1) * B]], dev))
            assert_rows(rows, ref_bags(find_rows, fk, fo, world, T, "sum")[0], BF16, f"T={T} insert_missing")
            assert np.array_equal(found.cpu().numpy().astype(bool), before)
            dist.barrier()
            for j in range(T):
                ek = full[j].export()[0].cpu().numpy()
                assert sg.tables[j].size() == int((oracle.hash_batch(ek, 1, world)[2] == rank).sum())
            report[T] = dict(traffic=sg.traffic(), collectives=sg.collectives)

        # ---- apply_pooled: 4 collectives (the cells, keys out, run lengths out, run rows out: nothing comes back) ----
        for T, opt in ((5, "adagrad"), (5, "adam"), (1, "adagrad")):
            sg, full = make(T, OPT_ADAGRAD if opt == "adagrad" else OPT_ADAM)
            dist.barrier()
            rng = np.random.default_rng(5)       # the same on every rank
            for n_step in (1, 2):
                if n_step == 1:      # no key twice inside a member, over all ranks
                    batches = distinct_batches(rng, world, T, [2 + r for r in range(world)])
                else:                # duplicates inside a rank and across ranks
                    batches = [bag_batch(95 + r, T, 2 + r) for r in range(world)]
                    batches = [(np.concatenate([batches[0][0][:30], k]), np.concatenate([[0], o[1:] + 30])) for k, o in batches]
                keys, off = batches[rank]
                kt, ot = _i64(keys, dev), _i64(off, dev)
                c0, t0 = sg.collectives, sg.traffic()
                g = torch.from_numpy(_bag_rows(off.size - 1, dim, 20 + n_step + rank)).to(dev)
                bag_of = torch.repeat_interleave(torch.arange(off.size - 1, device=dev), ot[1:] - ot[:-1])
                sg.apply_pooled(kt, ot, g, bag_of, opt, 0.01, beta1=0.9, beta2=0.999, step=n_step, located=None)
                assert sg.collectives - c0 == 4, (T, sg.collectives - c0)
                k_out, k_in, r_out, r_in = wire(batches)
                t1, cnt = sg.traffic(), 16 * T * (world - 1)
                assert (t1[0] - t0[0], t1[1] - t0[1]) == (8 * k_out + (4 + 4 * dim) * r_out + cnt, 8 * k_in + (4 + 4 * dim) * r_in + cnt)
                _reference_step(full, batches, T, dim, dev, opt, n_step, 20 + n_step)
                for j in range(T):
                    got, exp = _sorted_export([sg.tables[j]]), _sorted_export([full[j]])
                    sel = oracle.hash_batch(exp[0], 1, world)[2] == rank
                    assert np.array_equal(got[0], exp[0][sel])
                    for x, y in zip(got[1:], exp[1:]):
                        if n_step == 1:
                            same_bits(x, y[sel], f"{opt} member {j}")
                        else:
                            np.testing.assert_allclose(x, y[sel], rtol=1e-6, atol=1e-9, err_msg=f"{opt} member {j}")      # SPEC.md §4's contract
            dist.barrier()

        # ---- the layer over a sharded group == the same layer over the plain group, bit for bit (no duplicate keys in a member) ----
        if world == 1:
            T, st = 5, stored_keys()
            for opt, code, dt, mode in (("adagrad", OPT_ADAGRAD, torch.float32, "mean"), ("adam", OPT_ADAM, BF16, "sum")):
                sg, full = make(T, code)
                plain = TableGroup(full, max_apply_batch=mb)
                la = DynamicEmbeddingBag(sg, mode=mode, optimizer=opt, lr=0.05, create_missing=True, out_dtype=dt).to(dev)
                lb = DynamicEmbeddingBag(plain, mode=mode, optimizer=opt, lr=0.05, create_missing=True, out_dtype=dt).to(dev)
                la.train(), lb.train()
                rng = np.random.default_rng(9)
                B = 6
                lens = rng.choice(SHORT + (LONG,), T * B)
                lens[-1] = 7
                cut = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
                ks = np.concatenate([st[rng.permutation(NK)[:cut[(j + 1) * B] - cut[j * B]]] for j in range(T)]).astype(np.int64)
                fresh_at = cut[-2] + np.arange(5)      # ids no table has seen, in the last bag
                ks[fresh_at] = synth.keys_np(79, 0, fresh_at.size)
                kt, ot = _i64(ks, dev), _i64(cut, dev)
                w = torch.from_numpy(np.random.default_rng(3).standard_normal((T * B, dim)).astype(np.float32)).to(dev)
                with pytest.raises(ValueError):
                    la(kt, ot, per_sample_weights=torch.ones(ks.size, device=dev))
                c0 = sg.collectives
                oa, ob = la(kt, ot), lb(kt, ot)
                assert oa.dtype == ob.dtype == dt and torch.equal(oa.detach().float(), ob.detach().float())
                (oa.float() * w).sum().backward()
                (ob.float() * w).sum().backward()
                assert sg.collectives - c0 == 9      # 5 for the forward, 4 for the step
                for j in range(T):
                    got, exp = _sorted_export([sg.tables[j]]), _sorted_export([full[j]])
                    assert np.array_equal(got[0], exp[0])
                    for x, y in zip(got[1:], exp[1:]):
                        same_bits(x, y, f"layer {opt} member {j}")
                assert full[T - 1].size() == NK + fresh_at.size
            assert sg.traffic() == (0, 0)      # one rank keeps every segment for itself
        q.put((rank, report))
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.parametrize("world,dim", [(2, 4), (3, 64)])
def test_sharded_group_bags_multi_rank_on_one_gpu(dev, world, dim):
    """ShardedTableGroup's pooled forms over gloo (staged through host memory), 2 and 3 ranks on one GPU.  Collectives per call, whatever the number
    of tables: find_pooled 5 (the [G, 2 T] cells, keys out, run lengths out, partial rows back, found back); apply_pooled 4 (the cells, keys out,
    run lengths out, run rows out)."""
    res = _launch(_gpu_rank, world, ("gloo", dim))
    assert [r[0] for r in res] == list(range(world))
    for T in (1, 5):      # what all ranks sent is what all ranks received
        assert sum(r[1][T]["traffic"][0] for r in res) == sum(r[1][T]["traffic"][1] for r in res)


@pytest.mark.gpu
def test_sharded_group_bags_rccl_single_gpu_and_the_layer(dev):
    """world 1 over real RCCL; and DynamicEmbeddingBag over the sharded group against the same layer over the plain TableGroup"""
    res = _launch(_gpu_rank, 1, ("nccl", 64))
    assert [r[0] for r in res] == [0]
