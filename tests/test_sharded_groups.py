"""Sharded table groups (SPEC.md §5 "Groups"): mee_segment_counts / mee_regroup, Router's methods over them, ShardedTableGroup.find / find_or_insert /
apply_adagrad / apply_adam / traffic() / collectives, and DynamicEmbeddingCollection over a ShardedTableGroup.

The yardsticks are code that is not under test: numpy (searchsorted on perm for the cells, a stable argsort by table id for the regrouping) and one
LookupTable per member that holds the union of the member's shards (`full[j]`), called once per segment.  Every member stores the SAME key values with
different rows, so a regrouping that mixes segments returns a wrong row for every key."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist

import oracle
from meepoembedding_amd import _lib, synth
from test_sharded_bags import _i64, same_bits
from test_sharded_bf16 import _launch

BF16 = torch.bfloat16
NK, CAP, DEFAULT = 3000, 8192, 0.1
NEW_SYMBOLS = ("mee_segment_counts", "mee_regroup")
KINDS = ("plain", "n = 0", "empty middle", "empty ends", "one owner", "skip owner", "outside")


# ---- fixtures and the reference model (numpy only) ------------------------------------------------------------------------------
def stored_keys():
    return synth.keys_np(1, 0, NK)


def make_batch(kind: str, seed: int, G: int, T: int):
    """-> (keys int64 [n <= 2000], offsets int64 [T + 1]).  Keys drawn from the NK stored ones (every member stores the same key values), ~5 % absent,
    two EMPTY padding keys, duplicates inside and across segments."""
    rng = np.random.default_rng(1000 * seed + 10 * G + T)
    st = stored_keys()
    owner = oracle.hash_batch(st, 1, G)[2]
    if kind == "n = 0":
        return np.zeros(0, dtype=np.int64), np.zeros(T + 1, dtype=np.int64)
    lens = rng.integers(1, 1200 // T + 2, T) + (50 if kind in ("plain", "outside") else 0)
    pool = st
    if kind == "empty middle":
        lens[T // 2] = 0
    elif kind == "empty ends":
        lens[0] = lens[-1] = 0
    elif kind == "one owner":          # a cell longer than one block's tile (member 0: 1500 keys of ONE owner) next to cells of length 1
        lens[:] = 1
        lens[0] = 1500
    elif kind == "skip owner" and G > 1:
        pool = st[owner != 1]          # owner 1 receives nothing
    keys = pool[rng.integers(0, pool.size, int(lens.sum()))].astype(np.int64)
    if kind == "one owner":
        keys[:1500] = rng.choice(st[owner == G - 1], 1500)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = keys.size
    if kind in ("plain", "outside"):
        keys[3] = keys[n - 2]                                               # a duplicate across segments (or inside the only one)
        pick = rng.choice(np.arange(4, n - 2), n // 20 + 2, replace=False)
        keys[pick[:-2]] = synth.keys_np(9, seed * 1000, pick.size - 2)      # absent keys
        keys[pick[-2:]] = oracle.EMPTY_KEY                                  # padding keys
    if kind == "outside":              # positions in no segment at both ends
        off[0], off[-1] = 7, n - 5
        off = np.clip(off, 7, n - 5)
    return keys, off


def with_fresh(keys: np.ndarray, off: np.ndarray, fresh: np.ndarray):
    """the batch with `fresh` put in front of every member's segment: the same unseen key values meet every member"""
    T = off.size - 1
    k = np.concatenate([np.concatenate([fresh, keys[off[j]:off[j + 1]]]) for j in range(T)]).astype(np.int64)
    return k, (off + np.arange(T + 1) * fresh.size).astype(np.int64)


def np_route(keys: np.ndarray, off: np.ndarray, G: int, skip_padding: bool = False):
    """-> (send, counts, perm, cells [G, T]) of the stable partition, the cells by searchsorted on every owner's segment of perm"""
    if skip_padding:
        pos = np.flatnonzero(keys != oracle.EMPTY_KEY)
        send, counts, perm = oracle.partition(keys[pos], G)
        perm = pos[perm]
    else:
        send, counts, perm = oracle.partition(keys, G)
    cells = np.zeros((G, off.size - 1), dtype=np.int64)
    base = 0
    for p in range(G):
        cells[p] = np.diff(np.searchsorted(perm[base:base + counts[p]], off, side="left"))
        base += counts[p]
    return send, counts.astype(np.int64), perm.astype(np.int64), cells


def np_regroup(recv: np.ndarray, recv_cells: np.ndarray):
    """source-major -> table-major: a stable argsort by table id"""
    T = recv_cells.shape[1]
    table_id = np.concatenate([np.repeat(np.arange(T), row) for row in recv_cells]) if recv.size else np.zeros(0, dtype=np.int64)
    order = np.argsort(table_id, kind="stable").astype(np.int64)
    return recv[order], order, np.concatenate([[0], np.cumsum(np.bincount(table_id, minlength=T))]).astype(np.int64)


def np_inbox(sources, p: int):
    """what owner p receives from the sources [(send, counts, perm, cells, off)]: -> (keys source-major, cells [G_src, T], per source the positions of
    its owner segment p that lie in a segment)"""
    recv, rows, picks = [], [], []
    for send, counts, perm, cells, off in sources:
        b = int(counts[:p].sum())
        seg = perm[b:b + counts[p]]
        inside = b + np.flatnonzero((seg >= off[0]) & (seg < off[-1]))
        recv.append(send[inside])
        rows.append(cells[p])
        picks.append(inside)
    return np.concatenate(recv).astype(np.int64), np.stack(rows), picks


# ---- CPU ------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_declared_exported_and_prototyped(built):
    from test_abi_load import _declared
    names = _declared()
    L = C.CDLL(_lib.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s in names and s in _lib.PROTOTYPES and hasattr(L, s), s
    assert _lib.lib().mee_abi_version() == 2     # additive: the ABI version stays
    from meepoembedding_amd import Router
    from meepoembedding_amd.sharded import ShardedTableGroup
    for m in ("segment_counts", "regroup"):
        assert callable(getattr(Router, m))
    for m in ("find", "find_or_insert", "apply_adagrad", "apply_adam", "traffic"):
        assert callable(getattr(ShardedTableGroup, m))


def test_null_router_or_arguments_are_errors_not_faults(built):
    L = _lib.lib()
    buf = (C.c_uint64 * 8)()
    assert L.mee_segment_counts(None, None, None, 0, None, 0, None, None) == _lib.ERR_INVALID_ARG
    assert L.mee_segment_counts(None, buf, buf, 4, buf, 1, buf, None) == _lib.ERR_INVALID_ARG
    assert L.mee_regroup(None, None, None, 0, 0, None, None, None, None) == _lib.ERR_INVALID_ARG
    assert L.mee_regroup(None, buf, buf, 4, 1, buf, buf, buf, None) == _lib.ERR_INVALID_ARG
    assert b"null argument" in L.mee_last_error()


@pytest.mark.parametrize("G", [1, 2, 3, 8])
@pytest.mark.parametrize("T", [1, 3, 5])
def test_reference_model_on_the_fixture(G, T):
    """the numpy model the kernels are compared with agrees with a plain per-position count, and the fixture holds the cases it promises"""
    for kind in KINDS:
        keys, off = make_batch(kind, 3, G, T)
        assert keys.size <= 2000 and off.size == T + 1 and np.all(np.diff(off) >= 0)
        send, counts, perm, cells = np_route(keys, off, G)
        owner = oracle.hash_batch(keys, 1, G)[2]
        seg = np.searchsorted(off, np.arange(keys.size), side="right") - 1
        ok = (np.arange(keys.size) >= off[0]) & (np.arange(keys.size) < off[-1])
        brute = np.zeros((G, T), dtype=np.int64)
        np.add.at(brute, (owner[ok], seg[ok]), 1)
        assert np.array_equal(cells, brute), kind
        if kind == "one owner":
            assert cells[G - 1, 0] == 1500 and (T == 1 or cells[:, 1:].sum() == T - 1)
        if kind == "skip owner" and G > 1:
            assert cells[1].sum() == 0 and cells.sum() == keys.size
        if kind == "outside":
            assert off[0] > 0 and off[-1] < keys.size and cells.sum() == off[-1] - off[0]
        if kind == "plain":
            assert (keys == oracle.EMPTY_KEY).sum() == 2 and np.unique(keys).size < keys.size
        if T >= 3:
            assert kind != "empty middle" or np.diff(off)[T // 2] == 0
            assert kind != "empty ends" or (np.diff(off)[0] == 0 and np.diff(off)[-1] == 0 and keys.size > 0)
    # the regrouping: every received key lands in its member's segment, sources in rank order, arrival order inside
    srcs = [np_route(*make_batch("plain", 5 + s, G, T), G) + (make_batch("plain", 5 + s, G, T)[1],) for s in range(G)]
    for p in range(G):
        recv, rc, _ = np_inbox(srcs, p)
        k_tm, order, off_tm = np_regroup(recv, rc)
        assert np.array_equal(np.sort(order), np.arange(recv.size)) and off_tm[-1] == recv.size
        at = np.concatenate([[0], np.cumsum(rc.reshape(-1))])
        for j in range(T):
            want = np.concatenate([recv[at[s * T + j]:at[s * T + j + 1]] for s in range(G)])
            assert np.array_equal(k_tm[off_tm[j]:off_tm[j + 1]], want)


class NpRouter:
    """the CPU router of tests/_cpu_backend.py plus the two planning steps in numpy: the host logic of ShardedTableGroup runs without a GPU"""

    def __init__(self, n_shards):
        from _cpu_backend import CpuRouter
        self.n_shards, self._r = n_shards, CpuRouter(n_shards)
        self.partition, self.scatter_rows, self.gather_rows = self._r.partition, self._r.scatter_rows, self._r.gather_rows

    def segment_counts(self, perm, counts, offsets):
        c, o, out, base = counts.numpy(), offsets.numpy(), [], 0
        for p in range(self.n_shards):
            out.append(np.diff(np.searchsorted(perm.numpy()[base:base + c[p]], o, side="left")))
            base += c[p]
        return torch.from_numpy(np.stack(out).astype(np.int64))

    def regroup(self, recv_keys, recv_cells):
        return tuple(torch.from_numpy(x) for x in np_regroup(recv_keys.numpy(), recv_cells.numpy()))


class CpuGroup:
    """CpuTable per member, one call per segment: the definition of a grouped operator"""

    def __init__(self, tables):
        self.tables, self.dim = tables, tables[0].dim

    def _each(self, offsets):
        o = offsets.tolist()
        return [(t, o[j], o[j + 1]) for j, t in enumerate(self.tables)]

    def find(self, keys, offsets):
        parts = [t.find(keys[a:b]) for t, a, b in self._each(offsets)]
        return torch.cat([x[0] for x in parts]), torch.cat([x[1] for x in parts])

    def apply_adagrad(self, keys, offsets, grads, lr, eps=1e-10):
        for t, a, b in self._each(offsets):
            t.apply_adagrad(keys[a:b], grads[a:b], lr, eps)


def _cpu_rank(rank, world, port, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        from _cpu_backend import CpuRouter, CpuTable
        from meepoembedding_amd.sharded import ShardedTableGroup
        dist.init_process_group("gloo", rank=rank, world_size=world)
        dim, st = 4, stored_keys()
        mine = oracle.hash_batch(st, 1, world)[2] == rank
        for T in (1, 5):
            def member(j, part, opt=oracle.OPT_ADAGRAD):
                t = CpuTable(CAP, dim, optimizer=opt, default_value=DEFAULT, initial_accumulator=0.1)
                t.insert(torch.from_numpy(st[part]), torch.from_numpy(synth.rows_np(st[part], dim, 2 + j)))
                return t
            sg = ShardedTableGroup(CpuGroup([member(j, mine) for j in range(T)]), NpRouter(world))
            full = [member(j, slice(None)) for j in range(T)]
            assert sg.traffic() == (0, 0) and sg.collectives == 0 and sg.n_tables == T and sg.dim == dim
            batches = [make_batch("plain", 30 + r, world, T) for r in range(world)]
            keys, off = batches[rank] if rank else make_batch("n = 0", 0, world, T)     # rank 0 has an empty batch
            kt, ot = torch.from_numpy(keys), torch.from_numpy(off)
            # refused on every rank alike, before anything is exchanged
            for bad in (lambda: sg.find(kt, ot[:-1]), lambda: sg.find(kt, ot, out_dtype=BF16), lambda: sg.find(kt, ot, out_dtype=torch.float16),
                        lambda: sg.find_or_insert(kt, ot), lambda: sg.apply_adam(kt, ot, torch.zeros(keys.size, dim), 0.01),
                        lambda: ShardedTableGroup(sg.local_group, CpuRouter(world)).find(kt, ot),
                        lambda: ShardedTableGroup(sg.local_group, NpRouter(world + 1))):
                with pytest.raises(ValueError):
                    bad()
            assert sg.traffic() == (0, 0) and sg.collectives == 0
            rows, found = sg.find(kt, ot)
            assert sg.collectives == 4, (T, sg.collectives)      # one count exchange, keys out, rows back, found back — whatever T is
            for j in range(T):
                er, ef = full[j].find(kt[off[j]:off[j + 1]])
                assert torch.equal(rows[off[j]:off[j + 1]].view(torch.int32), er.view(torch.int32)) and torch.equal(found[off[j]:off[j + 1]], ef), (T, j)
            # traffic(): 8 B per key out, 4 dim + 1 B per key in, and the cells
            owner = oracle.hash_batch(keys, 1, world)[2]
            to = np.bincount(owner, minlength=world)
            every = [None] * world
            dist.all_gather_object(every, to.tolist())
            k_out = int(to.sum() - to[rank])
            k_in = int(sum(every[s][rank] for s in range(world) if s != rank))
            cnt = 8 * T * (world - 1)
            assert sg.traffic() == (8 * k_out + (4 * dim + 1) * k_in + cnt, 8 * k_in + (4 * dim + 1) * k_out + cnt), (sg.traffic(), k_out, k_in)
            t0 = sg.traffic()
            g = torch.from_numpy((synth.rows_np(keys, dim, 6) * 0.02).astype(np.float32))
            sg.apply_adagrad(kt, ot, g, 0.01)
            assert sg.collectives == 7                           # + one count exchange, keys out, gradient rows out
            t1 = sg.traffic()
            assert (t1[0] - t0[0], t1[1] - t0[1]) == ((8 + 4 * dim) * k_out + cnt, (8 + 4 * dim) * k_in + cnt)
            for j in range(T):       # the reference gets every rank's pairs of member j
                ks = [batches[r][0][batches[r][1][j]:batches[r][1][j + 1]] for r in range(1, world)]
                kk = np.concatenate(ks)
                full[j].apply_adagrad(torch.from_numpy(kk), torch.from_numpy((synth.rows_np(kk, dim, 6) * 0.02).astype(np.float32)), 0.01)
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


# ---- GPU, one process: the two kernels against numpy ----------------------------------------------------------------------------
def _np(t):
    return t.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 3, 5])
@pytest.mark.parametrize("G", [1, 2, 3, 8])
def test_segment_counts_and_regroup_against_numpy(dev, G, T):
    from meepoembedding_amd import Router
    r = Router(G, 2048, device=dev)
    for kind in KINDS:
        batches = [make_batch(kind, 11 + s, G, T) for s in range(G)]
        srcs = []
        for keys, off in batches:
            send_e, counts_e, perm_e, cells_e = np_route(keys, off, G)
            kt, ot = _i64(keys, dev), _i64(off, dev)
            send, counts, perm = r.partition(kt)
            assert np.array_equal(_np(perm), perm_e) and np.array_equal(_np(counts), counts_e), kind
            cells = r.segment_counts(perm, counts, ot)
            assert cells.dtype == torch.int64 and cells.shape == (G, T) and np.array_equal(_np(cells), cells_e), (kind, _np(cells), cells_e)
            assert np.array_equal(_np(r.segment_counts(perm, counts, ot.view(torch.uint64))), cells_e)
            # padding left out by the partition: the counts, not n, bound the segments
            _, c_pad, p_pad, cells_pad = np_route(keys, off, G, skip_padding=True)
            _, counts2, perm2 = r.partition(kt, skip_padding=True)
            assert np.array_equal(_np(counts2), c_pad) and np.array_equal(_np(perm2)[:p_pad.size], p_pad)
            assert np.array_equal(_np(r.segment_counts(perm2, counts2, ot)), cells_pad), kind
            srcs.append((_np(send), counts_e, perm_e, cells_e, off))
        for p in range(G):           # every owner in turn
            recv, rc, _ = np_inbox(srcs, p)
            k_e, order_e, off_e = np_regroup(recv, rc)
            rk, rct = _i64(recv, dev), _i64(rc, dev)
            k_tm, order, off_tm = r.regroup(rk, rct)
            what = (kind, G, T, p, recv.size)
            assert k_tm.dtype == order.dtype == off_tm.dtype == torch.int64 and off_tm.numel() == T + 1
            assert np.array_equal(_np(off_tm), off_e), what
            assert np.array_equal(_np(order), order_e) and np.array_equal(_np(k_tm), k_e), what
            # the 8-byte path (a source that is not 16-byte aligned) writes the same
            shifted = torch.cat([rk.new_zeros(1), rk])[1:]
            k1, o1, f1 = r.regroup(shifted, rct)
            assert (recv.size == 0 or shifted.data_ptr() % 16 == 8) and np.array_equal(_np(k1), k_e) and np.array_equal(_np(o1), order_e) and np.array_equal(_np(f1), off_e), what
            # rows follow through the existing permutation kernels
            rows = torch.arange(recv.size * 4, dtype=torch.float32, device=dev).view(-1, 4)
            assert torch.equal(r.gather_rows(rows, order), rows[order]) and torch.equal(r.scatter_rows(rows[order], order), rows)
    torch.cuda.synchronize(dev)


@pytest.mark.gpu
def test_kernels_touch_nothing_behind_their_outputs_and_refuse_bad_arguments(dev):
    from meepoembedding_amd import Router
    G, T = 3, 5
    r = Router(G, 2048, device=dev)
    L, st = _lib.lib(), torch.cuda.current_stream(dev).cuda_stream
    srcs = []
    for s in range(G):
        keys, off = make_batch("plain", 21 + s, G, T)
        send_e, counts_e, perm_e, cells_e = np_route(keys, off, G)
        cells = torch.full((G * T + 2,), -7, dtype=torch.int64, device=dev)
        pt, ct, ot = _i64(perm_e, dev), _i64(counts_e, dev), _i64(off, dev)
        _lib.check(L.mee_segment_counts(r._h, pt.data_ptr(), ct.data_ptr(), keys.size, ot.data_ptr(), T, cells.data_ptr(), st))
        assert np.array_equal(_np(cells), np.concatenate([cells_e.reshape(-1), [-7, -7]]))
        srcs.append((send_e, counts_e, perm_e, cells_e, off))
    recv, rc, _ = np_inbox(srcs, 1)
    k_e, order_e, off_e = np_regroup(recv, rc)
    n = recv.size
    rk, rct = _i64(recv, dev), _i64(rc, dev)
    ko = torch.full((n + 3,), -7, dtype=torch.int64, device=dev)
    oo = torch.full((n + 3,), -7, dtype=torch.int64, device=dev)
    fo = torch.full((T + 3,), -7, dtype=torch.int64, device=dev)
    _lib.check(L.mee_regroup(r._h, rk.data_ptr(), rct.data_ptr(), n, T, ko.data_ptr(), oo.data_ptr(), fo.data_ptr(), st))
    assert np.array_equal(_np(ko), np.concatenate([k_e, [-7] * 3])) and np.array_equal(_np(oo), np.concatenate([order_e, [-7] * 3]))
    assert np.array_equal(_np(fo), np.concatenate([off_e, [-7, -7]]))
    # cells that promise more than arrived: every position stays inside the arrays, the offsets inside [0, n_recv]
    big = torch.full((G, T), 1 << 40, dtype=torch.int64, device=dev)
    ko.fill_(-7), oo.fill_(-7), fo.fill_(-7)
    _lib.check(L.mee_regroup(r._h, rk.data_ptr(), big.data_ptr(), n, T, ko.data_ptr(), oo.data_ptr(), fo.data_ptr(), st))
    assert bool((ko[n:] == -7).all()) and bool((oo[n:] == -7).all()) and bool((fo[T + 1:] == -7).all())
    assert int(fo[:T + 1].max()) <= n and int(fo[:T + 1].min()) >= 0 and int(oo[:n].max()) < n
    # arguments refused before any launch
    assert L.mee_segment_counts(r._h, pt.data_ptr(), ct.data_ptr(), 2049, ot.data_ptr(), T, cells.data_ptr(), st) == _lib.ERR_BATCH_TOO_LARGE
    assert L.mee_segment_counts(r._h, pt.data_ptr(), ct.data_ptr(), 5, ot.data_ptr(), 0, cells.data_ptr(), st) == _lib.ERR_INVALID_ARG
    assert L.mee_segment_counts(r._h, pt.data_ptr(), ct.data_ptr(), 5, ot.data_ptr(), 1025, cells.data_ptr(), st) == _lib.ERR_INVALID_ARG
    assert L.mee_segment_counts(r._h, None, ct.data_ptr(), 5, ot.data_ptr(), T, cells.data_ptr(), st) == _lib.ERR_INVALID_ARG
    assert L.mee_segment_counts(r._h, pt.data_ptr(), ct.data_ptr(), 5, None, T, cells.data_ptr(), st) == _lib.ERR_INVALID_ARG
    assert L.mee_regroup(r._h, rk.data_ptr(), rct.data_ptr(), G * 2048 + 1, T, ko.data_ptr(), oo.data_ptr(), fo.data_ptr(), st) == _lib.ERR_BATCH_TOO_LARGE
    assert L.mee_regroup(r._h, rk.data_ptr(), rct.data_ptr(), n, 0, ko.data_ptr(), oo.data_ptr(), fo.data_ptr(), st) == _lib.ERR_INVALID_ARG
    assert L.mee_regroup(r._h, rk.data_ptr(), rct.data_ptr(), n, 8128 // G + 1, ko.data_ptr(), oo.data_ptr(), fo.data_ptr(), st) == _lib.ERR_INVALID_ARG
    assert L.mee_regroup(r._h, None, rct.data_ptr(), n, T, ko.data_ptr(), oo.data_ptr(), fo.data_ptr(), st) == _lib.ERR_INVALID_ARG
    assert L.mee_regroup(r._h, rk.data_ptr(), None, n, T, ko.data_ptr(), oo.data_ptr(), fo.data_ptr(), st) == _lib.ERR_INVALID_ARG
    torch.cuda.synchronize(dev)


# ---- GPU, one process: the operators with every owner played in turn ------------------------------------------------------------
def _table(dim, dev, optimizer, max_batch):
    from meepoembedding_amd import INIT_UNIFORM, LookupTable
    return LookupTable(CAP, dim, device=dev, optimizer=optimizer, initial_accumulator=0.1, max_batch=max_batch, default_value=DEFAULT,
                       initializer=INIT_UNIFORM, init_scale=0.05, init_seed=7)


def _members(T, dim, dev, optimizer, part, max_batch):
    """T tables that store the keys `part` of the stored ones: the SAME key values in every member, member j's rows from seed 2 + j"""
    st = stored_keys()[part]
    tables = []
    for j in range(T):
        t = _table(dim, dev, optimizer, max_batch)
        t.insert(_i64(st, dev), torch.from_numpy(synth.rows_np(st, dim, 2 + j)).to(dev))
        tables.append(t)
    return tables


def _world(G, T, dim, dev, optimizer):
    """-> (groups[p] = owner p's TableGroup of its T shards, full[j] = member j's union table)"""
    from meepoembedding_amd import TableGroup
    owner = oracle.hash_batch(stored_keys(), 1, G)[2]
    mb = max(G * 2048, 4096)
    groups = [TableGroup(_members(T, dim, dev, optimizer, owner == p, mb), max_apply_batch=mb if optimizer else 0) for p in range(G)]
    return groups, _members(T, dim, dev, optimizer, slice(None), mb)


def _emulate(router, groups, batches, on_owner, payloads=None):
    """the exchange in one process: batches[s] = rank s's (keys, offsets) on the device.  What crosses the link in ShardedTableGroup is sliced and
    concatenated here; on_owner(p, keys_tm, offsets_tm, order, received payload rows or None) -> rows per table-major position or None.
    -> per rank the returned rows in batch order (None without)."""
    G = len(groups)
    routed = []
    for s, (kt, ot) in enumerate(batches):
        send, counts, perm = router.partition(kt)
        cells = router.segment_counts(perm, counts, ot)
        assert int(cells.sum()) == kt.numel()
        routed.append((send, perm, counts.tolist(), cells, None if payloads is None else router.gather_rows(payloads[s], perm)))
    back = [[None] * G for _ in range(G)]
    for p in range(G):
        lo = [sum(c[:p]) for _, _, c, _, _ in routed]
        recv = torch.cat([send[a:a + c[p]] for (send, _, c, _, _), a in zip(routed, lo)])
        pay = None if payloads is None else torch.cat([rows[a:a + c[p]] for (_, _, c, _, rows), a in zip(routed, lo)])
        keys_tm, order, off_tm = router.regroup(recv, torch.stack([cells[p] for _, _, _, cells, _ in routed]))
        res = on_owner(p, keys_tm, off_tm, order, pay)
        if res is not None:
            sm = [router.scatter_rows(x, order) for x in res]
            at = 0
            for s in range(G):
                back[s][p] = [x[at:at + routed[s][2][p]] for x in sm]
                at += routed[s][2][p]
    if back[0][0] is None:
        return None
    return [[router.scatter_rows(torch.cat([back[s][p][i] for p in range(G)]), routed[s][1]) for i in range(len(back[s][0]))] for s in range(G)]


def _per_member(full, kt, ot, op, **kw):
    o = ot.tolist()
    parts = [getattr(full[j], op)(kt[o[j]:o[j + 1]], **kw) for j in range(len(full))]
    return torch.cat([x[0] for x in parts]), torch.cat([x[1] for x in parts])


def _sorted_export(tables):
    e = [t.export(with_state=True) for t in tables]
    k = torch.cat([x[0] for x in e])
    i = torch.argsort(k)
    return [k[i].cpu().numpy()] + [torch.cat([x[c] for x in e])[i].cpu().numpy() for c in (1, 2, 3) if e[0][c] is not None]


CONFIGS = [(2, 3, 4), (3, 5, 64), (8, 3, 64), (1, 1, 4)]


@pytest.mark.gpu
@pytest.mark.parametrize("G,T,dim", CONFIGS)
def test_emulated_find_and_find_or_insert_against_the_member_tables(dev, G, T, dim):
    from meepoembedding_amd import OPT_NONE, Router
    router = Router(G, 2048, device=dev)
    groups, full = _world(G, T, dim, dev, OPT_NONE)
    kinds = ["plain", "empty middle", "one owner", "skip owner", "n = 0"]
    base = [make_batch(kinds[s % len(kinds)], 50 + s, G, T) for s in range(G)]
    # the same key value in every member: each segment must come back with its OWN member's row
    base[0] = (np.tile(stored_keys()[:7], T), np.arange(T + 1, dtype=np.int64) * 7)
    for op, dt, fresh in (("find", torch.float32, None), ("find", BF16, None), ("find_or_insert", torch.float32, 77), ("find_or_insert", BF16, 78)):
        # find_or_insert: keys no table has seen; the ranks' fresh keys overlap, and every member meets the same ones
        batches_np = base if fresh is None else [with_fresh(k, o, synth.keys_np(fresh, 10 * s, 40)) for s, (k, o) in enumerate(base)]
        batches = [(_i64(k, dev), _i64(o, dev)) for k, o in batches_np]
        kw = {} if dt == torch.float32 else {"out_dtype": dt}
        before = [_per_member(full, kt, ot, "find")[1] for kt, ot in batches]      # found = present before the call, on every rank alike
        got = _emulate(router, groups, batches, lambda p, k, o, order, pay: getattr(groups[p], op)(k, o, **kw))
        bits = torch.int32 if dt == torch.float32 else torch.int16
        for s, (kt, ot) in enumerate(batches):
            er, _ = _per_member(full, kt, ot, op, **kw)
            rows, found = got[s]
            assert rows.dtype == dt and rows.shape == (kt.numel(), dim)
            assert torch.equal(rows.view(bits), er.view(bits)) and torch.equal(found, before[s]), (op, dt, s)
        if T > 1:
            assert not torch.equal(got[0][0][:7].float(), got[0][0][-7:].float())
    # afterwards every shard holds exactly the union's keys that it owns
    for j in range(T):
        ek = full[j].export()[0].cpu().numpy()
        per = np.bincount(oracle.hash_batch(ek, 1, G)[2], minlength=G)
        assert [groups[p].tables[j].size() for p in range(G)] == per.tolist() and full[j].size() > NK
    torch.cuda.synchronize(dev)


def _grads(keys_np, dim, seed):
    return (synth.rows_np(keys_np, dim, seed) * 0.02).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("opt", ["adagrad", "adam"])
@pytest.mark.parametrize("G,T,dim", CONFIGS[:3])
def test_emulated_apply_against_the_member_tables(dev, G, T, dim, opt):
    """two steps without duplicate keys: bit-identical to the member tables, state planes included; a third step with duplicates inside a rank and
    across ranks: within SPEC §4's tolerance (the owner's fp64 sum may run in a different order)"""
    from meepoembedding_amd import OPT_ADAGRAD, OPT_ADAM, Router
    router = Router(G, 2048, device=dev)
    groups, full = _world(G, T, dim, dev, OPT_ADAGRAD if opt == "adagrad" else OPT_ADAM)
    st = stored_keys()
    rng = np.random.default_rng(G * 10 + T)

    def step(batches_np, n_step):
        batches = [(_i64(k, dev), _i64(o, dev)) for k, o in batches_np]
        pays = [torch.from_numpy(_grads(k, dim, 6 + n_step + s)).to(dev) for s, (k, _) in enumerate(batches_np)]

        def on_owner(p, k, o, order, pay):
            g = router.gather_rows(pay, order)
            if opt == "adagrad":
                groups[p].apply_adagrad(k, o, g, 0.01, 1e-10)
            else:
                groups[p].apply_adam(k, o, g, 0.01, 0.9, 0.999, 1e-8, n_step)
        assert _emulate(router, groups, batches, on_owner, pays) is None
        for j in range(T):       # member j of the reference: every rank's pairs, in rank order
            ks = np.concatenate([k[o[j]:o[j + 1]] for k, o in batches_np])
            gs = np.concatenate([_grads(k, dim, 6 + n_step + s)[o[j]:o[j + 1]] for s, (k, o) in enumerate(batches_np)])
            if opt == "adagrad":
                full[j].apply_adagrad(_i64(ks, dev), torch.from_numpy(gs).to(dev), 0.01, 1e-10)
            else:
                full[j].apply_adam(_i64(ks, dev), torch.from_numpy(gs).to(dev), 0.01, 0.9, 0.999, 1e-8, n_step)

    def distinct_batches():
        out = []
        for s in range(G):
            lens = rng.integers(0, 900 // T, T)
            lens[rng.integers(0, T)] = 0
            # per member a slice of a permutation: no key twice inside a member, over all ranks (the same key in different members is no duplicate)
            out.append((lens, np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)))
        keys = [[] for _ in range(G)]
        for j in range(T):
            perm, at = rng.permutation(NK), 0
            for s in range(G):
                keys[s].append(st[perm[at:at + out[s][0][j]]])
                at += out[s][0][j]
            assert at <= NK
        return [(np.concatenate(keys[s]).astype(np.int64), out[s][1]) for s in range(G)]

    for n_step in (1, 2):
        step(distinct_batches(), n_step)
    for j in range(T):
        got, exp = _sorted_export([groups[p].tables[j] for p in range(G)]), _sorted_export([full[j]])
        assert np.array_equal(got[0], exp[0]) and len(got) == len(exp) == (3 if opt == "adagrad" else 4)
        for x, y in zip(got[1:], exp[1:]):
            same_bits(x, y, f"{opt} G={G} T={T} member {j}")
    dup = [make_batch("plain", 70 + s, G, T) for s in range(G)]
    dup = [(np.concatenate([k, dup[0][0][:50]]), np.concatenate([o[:-1], [o[-1] + 50]])) for k, o in dup]      # every rank repeats rank 0's first keys
    step(dup, 3)
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
    from meepoembedding_amd.nn import DynamicEmbeddingCollection
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

        report = {}
        for T in (1, 5):
            sg, full = make(T)
            dist.barrier()
            assert sg.dim == dim and sg.device == dev and sg.n_tables == T and sg.supports_out_dtype and sg.collectives == 0
            kinds = ["plain", "one owner", "skip owner"]
            batches = [make_batch(kinds[r % 3], 80 + r, world, T) for r in range(world)]      # every rank can rebuild every rank's batch
            keys, off = batches[rank]
            kt, ot = _i64(keys, dev), _i64(off, dev)
            # ---- refusals: on every rank alike, before any collective ----
            with pytest.raises(ValueError):
                sg.find(kt, ot[:-1])
            with pytest.raises(ValueError):
                sg.find(kt, torch.cat([ot, ot[-1:]]))
            with pytest.raises(ValueError):
                sg.find(kt, ot, out_dtype=torch.float16)
            with pytest.raises(ValueError):
                ShardedTableGroup(sg.local_group, Router(world + 1, 2048, device=dev))
            with pytest.raises(ValueError):
                ShardedTableGroup(full[0], sg.router)      # (a single table is no group)
            assert sg.collectives == 0 and sg.traffic() == (0, 0)
            # ---- find: fp32, bf16; 4 collectives whatever T is; wire bytes ----
            owner = oracle.hash_batch(keys, 1, world)[2]
            to = np.bincount(owner, minlength=world)
            every = [None] * world
            dist.all_gather_object(every, to.tolist())
            k_out = int(to.sum() - to[rank])
            k_in = int(sum(every[s][rank] for s in range(world) if s != rank))
            cnt = 8 * T * (world - 1)
            for dt, row_bytes in ((torch.float32, 4 * dim), (BF16, 2 * dim)):
                c0, t0 = sg.collectives, sg.traffic()
                rows, found = sg.find(kt, ot, out_dtype=dt)
                assert sg.collectives - c0 == 4, (T, sg.collectives - c0)
                t1 = sg.traffic()
                assert (t1[0] - t0[0], t1[1] - t0[1]) == (8 * k_out + (row_bytes + 1) * k_in + cnt, 8 * k_in + (row_bytes + 1) * k_out + cnt), (T, dt)
                er, ef = _per_member(full, kt, ot, "find", **({} if dt == torch.float32 else {"out_dtype": dt}))
                bits = torch.int32 if dt == torch.float32 else torch.int16
                assert rows.dtype == dt and torch.equal(rows.view(bits), er.view(bits)) and torch.equal(found, ef), (T, dt)
            # ---- one rank has an empty batch, and one rank's offsets leave positions out ----
            if rank == 0:
                k0, o0 = kt[:0], torch.zeros(T + 1, dtype=torch.int64, device=dev)
            elif rank == 1:
                k0, o0 = tuple(_i64(x, dev) for x in make_batch("outside", 90, world, T))
            else:
                k0, o0 = kt, ot
            rows, found = sg.find(k0, o0)
            er, ef = _per_member(full, k0, o0, "find")
            a, b = int(o0[0]), int(o0[-1])
            assert rows.shape == (k0.numel(), dim) and torch.equal(rows[a:b].view(torch.int32), er.view(torch.int32)) and torch.equal(found[a:b], ef)
            assert not bool(found[:a].any()) and not bool(found[b:].any()) and not bool(rows[:a].any()) and not bool(rows[b:].any())
            # ---- find_or_insert: fresh keys overlap between the ranks; sizes afterwards ----
            fk, fo = with_fresh(keys, off, synth.keys_np(77, 10 * rank, 40))
            _, before = _per_member(full, _i64(fk, dev), _i64(fo, dev), "find")      # found = present before the call, on every rank alike
            c0 = sg.collectives
            rows, found = sg.find_or_insert(_i64(fk, dev), _i64(fo, dev), out_dtype=BF16)
            assert sg.collectives - c0 == 4
            for r in range(world):       # the reference creates every rank's keys
                _per_member(full, *[_i64(x, dev) for x in with_fresh(*batches[r], synth.keys_np(77, 10 * r, 40))], "find_or_insert")
            er, _ = _per_member(full, _i64(fk, dev), _i64(fo, dev), "find", out_dtype=BF16)
            assert torch.equal(rows.view(torch.int16), er.view(torch.int16)) and torch.equal(found, before)
            dist.barrier()
            for j in range(T):
                ek = full[j].export()[0].cpu().numpy()
                assert sg.tables[j].size() == int((oracle.hash_batch(ek, 1, world)[2] == rank).sum())
            report[T] = dict(k_out=k_out, k_in=k_in, traffic=sg.traffic(), collectives=sg.collectives)

        # ---- apply: 3 collectives (one count exchange, keys out, gradient rows out: nothing comes back) ----
        T = 5
        st = stored_keys()
        for opt in ("adagrad", "adam"):
            sg, full = make(T, OPT_ADAGRAD if opt == "adagrad" else OPT_ADAM)
            dist.barrier()
            rng = np.random.default_rng(5)       # the same on every rank
            for n_step in (1, 2, 3):
                if n_step < 3:       # no key twice inside a member, over all ranks
                    lens = rng.integers(0, 150, (world, T))
                    perms = [rng.permutation(NK) for _ in range(T)]
                    at = np.concatenate([np.zeros((1, T), dtype=np.int64), np.cumsum(lens, axis=0)])
                    batches = [(np.concatenate([st[perms[j][at[r, j]:at[r + 1, j]]] for j in range(T)]).astype(np.int64),
                                np.concatenate([[0], np.cumsum(lens[r])]).astype(np.int64)) for r in range(world)]
                else:                # duplicates inside a rank and across ranks
                    batches = [make_batch("plain", 95 + r, world, T) for r in range(world)]
                    batches = [(np.concatenate([k, batches[0][0][:50]]), np.concatenate([o[:-1], [o[-1] + 50]])) for k, o in batches]
                keys, off = batches[rank]
                c0, t0 = sg.collectives, sg.traffic()
                g = torch.from_numpy(_grads(keys, dim, 6 + n_step + rank)).to(dev)
                if opt == "adagrad":
                    sg.apply_adagrad(_i64(keys, dev), _i64(off, dev), g, 0.01, 1e-10)
                else:
                    sg.apply_adam(_i64(keys, dev), _i64(off, dev), g, 0.01, 0.9, 0.999, 1e-8, n_step)
                assert sg.collectives - c0 == 3
                owner = oracle.hash_batch(keys, 1, world)[2]
                k_out = int((owner != rank).sum())
                k_in = int(sum((oracle.hash_batch(batches[r][0], 1, world)[2] == rank).sum() for r in range(world) if r != rank))
                t1, cnt = sg.traffic(), 8 * T * (world - 1)
                assert (t1[0] - t0[0], t1[1] - t0[1]) == ((8 + 4 * dim) * k_out + cnt, (8 + 4 * dim) * k_in + cnt)
                for j in range(T):
                    ks = np.concatenate([k[o[j]:o[j + 1]] for k, o in batches])
                    gs = np.concatenate([_grads(k, dim, 6 + n_step + r)[o[j]:o[j + 1]] for r, (k, o) in enumerate(batches)])
                    if opt == "adagrad":
                        full[j].apply_adagrad(_i64(ks, dev), torch.from_numpy(gs).to(dev), 0.01, 1e-10)
                    else:
                        full[j].apply_adam(_i64(ks, dev), torch.from_numpy(gs).to(dev), 0.01, 0.9, 0.999, 1e-8, n_step)
                if n_step == 1:
                    continue
                for j in range(T):
                    got, exp = _sorted_export([sg.tables[j]]), _sorted_export([full[j]])
                    sel = oracle.hash_batch(exp[0], 1, world)[2] == rank
                    assert np.array_equal(got[0], exp[0][sel])
                    for x, y in zip(got[1:], exp[1:]):
                        if n_step == 2:
                            same_bits(x, y[sel], f"{opt} member {j}")
                        else:
                            np.testing.assert_allclose(x, y[sel], rtol=1e-6, atol=1e-9, err_msg=f"{opt} member {j}")      # SPEC.md §4's contract
            dist.barrier()

        # ---- the layer over a sharded group == the same layer over the plain group, bit for bit (no duplicate keys) ----
        if world == 1:
            for opt, code in (("adagrad", OPT_ADAGRAD), ("adam", OPT_ADAM)):
                sg, full = make(T, code)
                plain = TableGroup(full, max_apply_batch=mb)
                la = DynamicEmbeddingCollection(sg, optimizer=opt, lr=0.05, out_dtype=BF16 if opt == "adam" else torch.float32).to(dev)
                lb = DynamicEmbeddingCollection(plain, optimizer=opt, lr=0.05, out_dtype=BF16 if opt == "adam" else torch.float32).to(dev)
                la.train(), lb.train()
                rng = np.random.default_rng(9)
                lens = rng.integers(0, 300, T)
                ks = np.concatenate([st[rng.permutation(NK)[:l]] for l in lens] + [synth.keys_np(79, 0, 30)]).astype(np.int64)     # with ids no table has seen
                lens[-1] += 30
                kt, ot = _i64(ks, dev), _i64(np.concatenate([[0], np.cumsum(lens)]), dev)
                w = torch.from_numpy(np.random.default_rng(3).standard_normal((ks.size, dim)).astype(np.float32)).to(dev)
                c0 = sg.collectives
                oa, ob = la(kt, ot), lb(kt, ot)
                assert oa.dtype == ob.dtype and torch.equal(oa.detach().float(), ob.detach().float())
                (oa.float() * w).sum().backward()
                (ob.float() * w).sum().backward()
                assert sg.collectives - c0 == 7      # 4 for the forward, 3 for the step
                for j in range(T):
                    got, exp = _sorted_export([sg.tables[j]]), _sorted_export([full[j]])
                    assert np.array_equal(got[0], exp[0]) and got[0].size > NK - 1
                    for x, y in zip(got[1:], exp[1:]):
                        same_bits(x, y, f"layer {opt} member {j}")
            assert sg.traffic() == (0, 0)      # one rank keeps every segment for itself
        q.put((rank, report))
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.parametrize("world,dim", [(2, 4), (3, 64)])
def test_sharded_group_multi_rank_on_one_gpu(dev, world, dim):
    """ShardedTableGroup over gloo (staged through host memory), 2 and 3 ranks on one GPU.  Collectives per call, whatever the number of tables:
    find / find_or_insert 4 (one exchange of the [G, T] cells, keys out, rows back, found back); apply_adagrad / apply_adam 3 (the cells, keys out,
    gradient rows out — an apply returns nothing, so nothing comes back)."""
    res = _launch(_gpu_rank, world, ("gloo", dim))
    assert [r[0] for r in res] == list(range(world))
    for T in (1, 5):      # what all ranks sent is what all ranks received
        assert sum(r[1][T]["traffic"][0] for r in res) == sum(r[1][T]["traffic"][1] for r in res)


@pytest.mark.gpu
def test_sharded_group_rccl_single_gpu_and_the_layer(dev):
    """world 1 over real RCCL, as tests/test_sharded.py::test_sharded_rccl_single_gpu; and DynamicEmbeddingCollection over the sharded group"""
    res = _launch(_gpu_rank, 1, ("nccl", 64))
    assert [r[0] for r in res] == [0]
