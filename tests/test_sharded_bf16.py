"""bf16 result rows for the sharded lookups (SPEC.md §3 "Output type", §5): mee_sharded_find_as / mee_sharded_find_or_insert_as /
mee_sharded_traffic, RcclShardedTable and ShardedLookupTable with out_dtype.

The yardstick of every bf16 result is the fp32 result of the SAME call on the same state, rounded by torch.Tensor.to(torch.bfloat16) on the
CPU and compared on the raw 16-bit patterns (NaN positions by isnan), as in tests/test_bf16_out.py.  The tables hold fp32 rows throughout.

Wire bytes (test 6 of the issue).  mee_sharded_traffic counts every byte handed to ncclSend / ncclRecv.  For one exact-layout lookup without
dedup, with k_out of the rank's keys owned by other ranks, k_in keys arriving from other ranks and e bytes per element:
    sent     = 8·k_out + (e·dim + 1)·k_in  + 8·(G - 1)
    received = 8·k_in  + (e·dim + 1)·k_out + 8·(G - 1)
The issue writes the fp32 `sent` without the `+ k_in` found bytes; they are handed to ncclSend like the rows they travel with (the issue's own
"8 + 4·dim + 1 bytes a lookup puts on the wire" counts them, and summed over the ranks sent must equal received), so the formula asserted here —
and stated above mee_sharded_traffic in the header — has them on both sides.  The fp32 - bf16 deltas are the issue's: 2·dim·k_in and 2·dim·k_out."""
import ctypes as C
import os
import queue as queue_mod

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import oracle
from meepoembedding_amd import _lib, synth
from meepoembedding_amd.sharded import RcclShardedTable, ShardedLookupTable
from test_sharded import _free_port

BF16 = torch.bfloat16
NKEYS, BATCH = 6000, 4000
NEW_SYMBOLS = ("mee_sharded_find_as", "mee_sharded_find_or_insert_as", "mee_sharded_traffic")
# values whose rounding shows: round up, exact ties (to even, both ways), denormals (bf16 keeps them), ±inf, finite values beyond the largest bf16 (-> inf), NaN
SPECIALS = np.array([1 + 3 * 2.0 ** -9, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 1e-40, -1e-40, 2.0 ** -133, 2.0 ** -134, 1.5 * 2.0 ** -134,
                     np.inf, -np.inf, 3.4e38, -3.4e38, 3.3895e38, np.nan, 0.0, -0.0, 0.1, -7.3], dtype=np.float32)


def assert_bf16_of(got: torch.Tensor, ref_f32: torch.Tensor, what=""):
    """got (bf16) == bf16(ref_f32) bit for bit, the reference rounded by torch on the CPU; NaN positions by isnan"""
    assert got.dtype == BF16 and got.shape == ref_f32.shape, (what, got.dtype, got.shape, ref_f32.shape)
    ref = ref_f32.detach().cpu().contiguous().to(BF16).reshape(-1)
    got = got.detach().cpu().contiguous().reshape(-1)
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan), what
    bad = int((got.view(torch.int16)[~nan] != ref.view(torch.int16)[~nan]).sum())
    assert bad == 0, f"{what}: {bad} of {int((~nan).sum())} bf16 patterns differ"


def assert_same_bits(a: torch.Tensor, b: torch.Tensor, what=""):
    assert a.dtype == b.dtype == torch.float32 and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)), what


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_new_symbols_declared_and_exported(built):
    from test_abi_load import _declared
    names = _declared()
    L = C.CDLL(_lib.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s in names and s in _lib.PROTOTYPES and hasattr(L, s), s
    assert _lib.lib().mee_abi_version() == 2     # additive: the ABI version stays


def test_c_abi_null_arguments_are_errors_not_faults(built):
    """a null context — with or without keys — is refused with a code (a context needs a GPU: null keys on a live one are in the GPU half)"""
    L = _lib.lib()
    sent, recv = C.c_uint64(), C.c_uint64()
    for dt in (_lib.DTYPE_F32, _lib.DTYPE_BF16):
        assert L.mee_sharded_find_as(None, None, 0, None, dt, None, None) == _lib.ERR_INVALID_ARG
        assert L.mee_sharded_find_as(None, None, 5, None, dt, None, None) == _lib.ERR_INVALID_ARG
        assert L.mee_sharded_find_or_insert_as(None, None, 5, None, dt, None, None) == _lib.ERR_INVALID_ARG
    assert L.mee_sharded_traffic(None, C.byref(sent), C.byref(recv)) == _lib.ERR_INVALID_ARG
    assert b"null context" in L.mee_last_error()


class Recorder:   # stands in for the library: records what would have been called
    def __init__(self, calls):
        self.calls = calls

    def __getattr__(self, name):
        self.calls.append(name)
        return lambda *a: 0


def test_rccl_wrapper_rejects_before_any_call(built, monkeypatch):
    import inspect
    from meepoembedding_amd import sharded as sm
    calls = []
    monkeypatch.setattr(sm.RcclShardedTable, "_s", lambda self: 0)
    t = RcclShardedTable.__new__(RcclShardedTable)
    t._lib, t._check, t._C, t._h, t._comm = _lib, _lib.check, C, None, None
    monkeypatch.setattr(_lib, "lib", lambda: Recorder(calls))
    t.device, t.dim = torch.device("cpu"), 8
    keys = torch.arange(6, dtype=torch.int64)
    f32, b16, f16 = torch.empty(6, 8), torch.empty(6, 8, dtype=BF16), torch.empty(6, 8, dtype=torch.float16)
    for f in (t.find, t.find_or_insert):
        assert inspect.signature(f).parameters["out_dtype"].default is torch.float32
        for kw in (dict(out_dtype=torch.float16), dict(out_dtype=torch.float64), dict(out=f32, out_dtype=BF16), dict(out=b16),
                   dict(out=f16, out_dtype=torch.float16)):
            with pytest.raises(ValueError):
                f(keys, **kw)
    assert calls == []
    o, _ = t.find(keys, out_dtype=BF16)
    assert o.dtype == BF16 and o.shape == (6, 8)
    t.find_or_insert(keys, out=b16, out_dtype=BF16)
    t.find(keys); t.find_or_insert(keys, out=f32, out_dtype=torch.float32)      # the defaults are the existing entry points
    assert calls == ["mee_sharded_find_as", "mee_sharded_find_or_insert_as", "mee_sharded_find", "mee_sharded_find_or_insert"]
    assert t.traffic() == (0, 0) and calls[-1] == "mee_sharded_traffic"


def _cpu_rank(rank, world, port, q, tiered):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        from _cpu_backend import CpuRouter, CpuTable
        dist.init_process_group("gloo", rank=rank, world_size=world)
        dim = 16
        local = CpuTable(4096, dim)
        if tiered:
            from meepoembedding_amd.tiered import TieredLookupTable
            local = TieredLookupTable(CpuTable(512, dim), local, hot_key_limit=300)
        sh = ShardedLookupTable(local, CpuRouter(world))
        keys = synth.keys_np(3, rank * 500, 800)        # ranks overlap: last-wins across ranks
        rows = synth.rows_np(keys, dim, 2 + rank)
        sh.insert(torch.from_numpy(keys), torch.from_numpy(rows))
        dist.barrier()
        probe = torch.from_numpy(np.concatenate([synth.keys_np(3, 0, 1300)[rank::2], synth.keys_np(9, 0, 40)]))
        for dd in (False, True):
            for f in (sh.find, sh.find_or_insert):
                with pytest.raises(ValueError):     # no bf16 lookup behind this table: refused on every rank alike, before anything is exchanged
                    f(probe, dedup=dd, out_dtype=BF16)
                with pytest.raises(ValueError):
                    f(probe, dedup=dd, out_dtype=torch.float16)
        # the bf16 leg of the exchange itself, over gloo: rows travel as their bytes and arrive bit for bit (rank r sends r + 1 rows to every peer)
        mine = torch.from_numpy(synth.rows_np(keys[: world * (rank + 1)], dim, 9)).to(BF16)
        back = sh._a2a(mine, [rank + 1] * world, [s + 1 for s in range(world)])
        assert back.dtype == BF16 and back.shape == (world * (world + 1) // 2, dim)
        at = 0
        for s in range(world):
            sent = torch.from_numpy(synth.rows_np(synth.keys_np(3, s * 500, 800)[: world * (s + 1)], dim, 9)).to(BF16)[rank * (s + 1):(rank + 1) * (s + 1)]
            assert torch.equal(back[at:at + s + 1].view(torch.int16), sent.view(torch.int16))
            at += s + 1
        out, found = sh.find(probe)                  # ... and the same table still answers at fp32
        o2, f2 = sh.find(probe, dedup=True, out_dtype=torch.float32)
        assert torch.equal(out, o2) and torch.equal(found, f2)
        q.put((rank, probe.numpy(), out.numpy(), found.numpy()))
        dist.barrier()
        dist.destroy_process_group()
    except BaseException as e:
        import traceback
        q.put(("error", rank, "".join(traceback.format_exception(type(e), e, e.__traceback__))))
        raise


def _launch(target, world, args, first_timeout=300):
    """ranks spawned as tests/test_sharded.py::_launch does: every wait has its own time limit, a failed rank is reported at once and nobody is left running"""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=target, args=(r, world, port, q) + tuple(args)) for r in range(world)]
    for p in procs:
        p.start()

    def stop_all():
        for p in procs:   # the other ranks may be waiting for the failed one in a collective
            p.join(timeout=5)
            if p.is_alive():
                p.kill()

    results = []
    for _ in range(world):
        try:
            r = q.get(timeout=first_timeout)
        except queue_mod.Empty:
            stop_all()
            pytest.fail(f"no answer from a rank within {first_timeout} s")
        if r[0] == "error":
            stop_all()
            pytest.fail(f"rank {r[1]} failed:\n{r[2]}")
        results.append(r)
    for p in procs:
        p.join(timeout=60)
        if p.is_alive():
            p.kill()
            pytest.fail("a rank did not exit")
        assert p.exitcode == 0
    return sorted(results, key=lambda x: x[0])


@pytest.mark.parametrize("tiered", [False, True], ids=["flat", "tiered"])
def test_torch_path_refuses_bf16_without_a_bf16_lookup_and_answers_fp32(built, tiered):
    world, dim = 2, 16
    res = _launch(_cpu_rank, world, (tiered,), first_timeout=120)
    o = oracle.OracleTable(8192, dim)
    for r in range(world):
        k = synth.keys_np(3, r * 500, 800)
        o.insert(k, synth.rows_np(k, dim, 2 + r))
    for rank, probe, out, found in res:
        eo, ef = o.find(probe)
        assert np.array_equal(found, ef) and np.array_equal(out, eo)


# ---- GPU ----------------------------------------------------------------------------------------------------------------
def _rows_with_specials(rng, n, dim):
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    for i in range(min(64, n)):
        rows[i] = np.resize(np.roll(SPECIALS, i), dim)
    return rows


def _find_checks(t, name, queries):
    """checks 1 and 2: the same call at fp32, at bf16, at fp32 again on one context and one state"""
    for qn, qk in queries.items():
        what = f"{name}/{qn}"
        s0 = t.status()
        o32, f32 = t.find(qk)
        s32 = t.status()
        o16, f16 = t.find(qk, out_dtype=BF16)
        s16 = t.status()
        o32b, f32b = t.find(qk)
        assert_bf16_of(o16, o32, what)
        assert torch.equal(f16, f32) and s16 == s32 == s0, what
        assert_same_bits(o32b, o32, what + " (fp32 after bf16)")
        assert torch.equal(f32b, f32), what
        # caller buffers: the bf16 call writes [n, dim] bf16 and nothing behind it
        n = qk.numel()
        buf = torch.full((n + 2, t.dim), 7.5, dtype=BF16, device=qk.device)
        t.find(qk, out=buf[:n], out_dtype=BF16)
        assert torch.equal(buf[:n].view(torch.int16), o16.view(torch.int16)) and bool((buf[n:] == 7.5).all()), what


def _gpu_rank(rank, world, port, q, backend, dim):
    try:
        _gpu_rank_body(rank, world, port, q, backend, dim)
    except BaseException as e:   # report at once: the parent must not sit out its queue timeout
        import traceback
        q.put(("error", rank, "".join(traceback.format_exception(type(e), e, e.__traceback__))))
        raise


def _gpu_rank_body(rank, world, port, q, backend, dim):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if backend == "fake-rccl":   # several ranks share one GPU: the exchange behind the C-ABI binds the shared-memory stand-in for librccl
        os.environ["MEE_RCCL_LIB"] = os.path.join(root, "build", "libfake_rccl.so")
    from meepoembedding_amd import INIT_UNIFORM, OPT_ADAGRAD, LookupTable, MeepoError, Router
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        rng = np.random.default_rng(100 + rank)
        allk = synth.keys_np(1, 0, NKEYS)
        keys_np = allk[rng.integers(0, NKEYS, size=BATCH)]
        keys_np[:64] = allk[rank * 64:(rank + 1) * 64]          # the rows with the special values: keys of this rank's own, stored once
        keys, rows = torch.from_numpy(keys_np).to(dev), torch.from_numpy(_rows_with_specials(rng, BATCH, dim)).to(dev)
        probe = torch.from_numpy(np.concatenate([allk[: world * 64], allk[rank::3], synth.keys_np(9, rank * 50, 50)])).to(dev)
        res_keys = torch.tensor([oracle.EMPTY_KEY, oracle.EMPTY_KEY + 1], device=dev)
        queries = {"probe": probe,
                   "dup": torch.cat([probe[:500].repeat(7), probe[-60:], res_keys[:1]]),
                   "reserved": torch.cat([probe[:300], res_keys, torch.from_numpy(synth.keys_np(11, rank * 40, 40)).to(dev), res_keys, probe[:5]])}
        cap_pad = int(np.ceil(BATCH / world * 1.5)) + 1024
        big = max(world * BATCH, world * cap_pad)
        mk = lambda cap=16384, **kw: LookupTable(cap, dim, device=dev, optimizer=OPT_ADAGRAD, initial_accumulator=0.1, max_batch=big, default_value=0.1,
                                                 initializer=INIT_UNIFORM, init_scale=0.05, init_seed=7, **kw)

        def contexts(which):
            made = {}
            for name in which:
                if name == "tiered":
                    made[name] = RcclShardedTable(mk(cap=8192), BATCH, pad_slack=0.0, cold=mk(value_memory=_lib.MEM_HOST_PINNED), hot_key_limit=3000, dedup=True)
                else:
                    made[name] = RcclShardedTable(mk(), BATCH, pad_slack=1.5 if "pad" in name else 0.0, dedup=name.startswith("dd"))
                made[name].insert(keys, rows)
            return made

        names = ("exact", "padded", "dd_exact", "dd_pad", "tiered")
        ctxs = contexts(names)
        assert ctxs["padded"].segment_capacity == cap_pad
        report = {}
        for name in names:
            _find_checks(ctxs[name], name, queries)
            assert ctxs[name].status() == 0, name
        # null keys with n > 0 on a live context; an unknown dtype; a bf16 buffer that is not 8-byte aligned — all before anything is exchanged
        L, ex = _lib.lib(), ctxs["exact"]
        tmp = torch.empty((8, dim), dtype=BF16, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        assert L.mee_sharded_find_as(ex._h, None, 4, tmp.data_ptr(), _lib.DTYPE_BF16, None, st) == _lib.ERR_INVALID_ARG
        assert L.mee_sharded_find_as(ex._h, probe.data_ptr(), 4, tmp.data_ptr(), 7, None, st) == _lib.ERR_INVALID_ARG
        assert L.mee_sharded_find_or_insert_as(ex._h, probe.data_ptr(), 4, tmp.data_ptr() + 2, _lib.DTYPE_BF16, None, st) == _lib.ERR_INVALID_ARG
        # 4: an empty batch on one rank is still collective
        qe = probe[:0] if rank == 0 else probe
        for name in ("exact", "dd_pad", "tiered"):
            o32, f32 = ctxs[name].find(qe)
            o16, f16 = ctxs[name].find(qe, out_dtype=BF16)
            assert o16.shape == (qe.numel(), dim) and o16.dtype == BF16 and torch.equal(f16, f32)
            assert_bf16_of(o16, o32, name + "/empty on rank 0")
        # 6: wire bytes of one exact-layout lookup without dedup (the formulas: module docstring)
        if world > 1:
            owner = oracle.hash_batch(probe.cpu().numpy(), 1, world)[2]
            to = np.bincount(owner, minlength=world)
            every = [None] * world
            dist.all_gather_object(every, to.tolist())
            k_out = int(to.sum() - to[rank])
            k_in = int(sum(every[s][rank] for s in range(world) if s != rank))
            t0 = ex.traffic(); ex.find(probe)
            t1 = ex.traffic(); ex.find(probe, out_dtype=BF16)
            t2 = ex.traffic()
            d32, d16 = (t1[0] - t0[0], t1[1] - t0[1]), (t2[0] - t1[0], t2[1] - t1[1])
            print(f"[wire] world {world} dim {dim} rank {rank}: k_out {k_out} k_in {k_in} fp32 sent/recv {d32} bf16 sent/recv {d16}", flush=True)
            report["wire"] = dict(k_out=k_out, k_in=k_in, fp32=d32, bf16=d16)
            assert d32 == (8 * k_out + (4 * dim + 1) * k_in + 8 * (world - 1), 8 * k_in + (4 * dim + 1) * k_out + 8 * (world - 1)), (d32, k_out, k_in)
            assert (d32[0] - d16[0], d32[1] - d16[1]) == (2 * dim * k_in, 2 * dim * k_out), (d32, d16, k_out, k_in)
        else:
            assert ex.traffic() == (0, 0)      # one rank keeps every segment for itself: device copies, nothing handed to RCCL
        # 5: padded layout, overflow: every copy of one key goes to one owner, whose segment holds cap_pad positions
        if BATCH > cap_pad:
            pad = ctxs["padded"]
            hot = probe[:1].repeat(BATCH)
            o_1, f_1 = ctxs["exact"].find(probe[:1])
            assert int(f_1[0]) == 1
            o_h = torch.full((BATCH, dim), 7.5, dtype=BF16, device=dev); f_h = torch.full((BATCH,), 9, dtype=torch.uint8, device=dev)
            pad.find(hot, out=o_h, found=f_h, out_dtype=BF16)
            assert pad.status() & 1
            served = f_h == 1
            dropped = ~served
            assert int(served.sum()) == cap_pad and bool((f_h[dropped] == 0).all())
            assert_bf16_of(o_h[served], o_1.expand(int(served.sum()), dim), "overflow: served")
            assert_bf16_of(o_h[dropped], torch.full((int(dropped.sum()), dim), 0.1), "overflow: dropped = bf16(default_value)")
            pad.clear_status()
            assert pad.status() == 0
            o_d, f_d = ctxs["dd_pad"].find(hot, out_dtype=BF16)          # de-duplicated: ONE key travels, nothing overflows
            assert ctxs["dd_pad"].status() == 0 and bool((f_d == 1).all())
            assert_bf16_of(o_d, o_1.expand(BATCH, dim), "overflow batch, dedup")
        dist.barrier()
        # 3: find_or_insert at bf16 on these contexts, at fp32 on twins with the same op sequence (lookups change nothing)
        fresh = torch.from_numpy(synth.keys_np(78, rank * 300, 300)).to(dev)
        mix = torch.cat([fresh, probe[:200], fresh[:50]])
        twin_names = ("exact", "padded", "dd_pad", "tiered")
        twins = contexts(twin_names)
        for name in twin_names:
            a, b = ctxs[name], twins[name]
            o16, f16 = a.find_or_insert(mix, out_dtype=BF16)
            o32, f32 = b.find_or_insert(mix)
            assert_bf16_of(o16, o32, name + "/find_or_insert")
            assert torch.equal(f16, f32), name
            assert a.size() == b.size() and a.status() == b.status() == 0, name
            ea, eb = a.export_local(with_state=True), b.export_local(with_state=True)
            ia, ib = torch.argsort(ea[0]), torch.argsort(eb[0])
            assert torch.equal(ea[0][ia], eb[0][ib]), name
            for xa, xb in zip(ea[1:3], eb[1:3]):      # rows and the Adagrad accumulator: the tables stay fp32, bit for bit
                assert_same_bits(xa[ia], xb[ib], name + "/export")
            o16b, _ = a.find_or_insert(mix, out_dtype=BF16)      # now every key is stored: the same rows again, through the first pass alone
            assert torch.equal(o16b.view(torch.int16), o16.view(torch.int16)), name
        dist.barrier()
        # 7: the torch.distributed path, plain and with pre-exchange dedup
        if backend != "nccl" or world == 1:
            local = mk()
            sh = ShardedLookupTable(local, Router(world, BATCH, device=dev))
            sh.insert(keys, rows)
            dist.barrier()
            for qn, qk in queries.items():
                for dd in (False, True):
                    o32, f32 = sh.find(qk, dedup=dd)
                    o16, f16 = sh.find(qk, dedup=dd, out_dtype=BF16)
                    assert_bf16_of(o16, o32, f"torch path/{qn}/dedup={dd}")
                    assert torch.equal(f16, f32)
            o16, f16 = sh.find_or_insert(mix, dedup=True, out_dtype=BF16)
            o32, f32 = sh.find(mix)
            assert_bf16_of(o16, o32, "torch path/find_or_insert")
            with pytest.raises(ValueError):
                sh.find(probe, out_dtype=torch.float16)
            dist.barrier()
        for t in list(ctxs.values()) + list(twins.values()):
            t.close()
        q.put((rank, report))
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.parametrize("world,dim", [(2, 16), (3, 64), (4, 100), (2, 260), (4, 64), (3, 16)])
def test_native_exchange_bf16_multi_rank_on_one_gpu(dev, world, dim):
    """checks 1-7 of the issue through the exchange behind the C-ABI: 2-4 ranks on one GPU over the shared-memory stand-in for librccl
    (tests/cabi/fake_rccl.cpp), exact / padded / dedup / tiered contexts"""
    res = _launch(_gpu_rank, world, ("fake-rccl", dim))
    assert [r[0] for r in res] == list(range(world))
    # what all ranks sent is what all ranks received, in either type
    for kind in ("fp32", "bf16"):
        assert sum(r[1]["wire"][kind][0] for r in res) == sum(r[1]["wire"][kind][1] for r in res)


@pytest.mark.gpu
@pytest.mark.parametrize("world,dim", [(2, 64), (2, 100)])
def test_torch_exchange_bf16_multi_rank_on_one_gpu(dev, world, dim):
    """the same rank body without the stand-in bound: ShardedLookupTable over gloo with the exchange staged through host memory (gloo-gpu)
    is what differs; mee_sharded_* then runs over whatever librccl resolves to and is left out at world > 1"""
    res = _launch(_torch_rank, world, (dim,))
    assert [r[0] for r in res] == list(range(world))


def _torch_rank(rank, world, port, q, dim):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        from meepoembedding_amd import LookupTable, Router
        from meepoembedding_amd.tiered import TieredLookupTable
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        rng = np.random.default_rng(100 + rank)
        allk = synth.keys_np(1, 0, NKEYS)
        keys_np = allk[rng.integers(0, NKEYS, size=BATCH)]
        keys_np[:64] = allk[rank * 64:(rank + 1) * 64]
        keys, rows = torch.from_numpy(keys_np).to(dev), torch.from_numpy(_rows_with_specials(rng, BATCH, dim)).to(dev)
        probe = torch.from_numpy(np.concatenate([allk[: world * 64], allk[rank::3], synth.keys_np(9, rank * 50, 50)])).to(dev)
        dup = torch.cat([probe[:500].repeat(7), probe[-60:], torch.tensor([oracle.EMPTY_KEY, oracle.EMPTY_KEY + 1], device=dev)])
        mk = lambda cap=16384: LookupTable(cap, dim, device=dev, max_batch=world * BATCH, default_value=0.1)
        sh = ShardedLookupTable(mk(), Router(world, BATCH, device=dev))
        sh.insert(keys, rows)
        dist.barrier()
        for qk in (probe, dup, probe[:0] if rank == 0 else probe[:777]):
            for dd in (False, True):
                o32, f32 = sh.find(qk, dedup=dd)
                o16, f16 = sh.find(qk, dedup=dd, out_dtype=BF16)
                assert_bf16_of(o16, o32, f"gloo-gpu dedup={dd}")
                assert torch.equal(f16, f32)
                assert_same_bits(sh.find(qk, dedup=dd)[0], o32)
        fresh = torch.from_numpy(synth.keys_np(78, rank * 300, 300)).to(dev)
        o16, f16 = sh.find_or_insert(torch.cat([fresh, probe[:100]]), out_dtype=BF16)
        o32, f32 = sh.find(torch.cat([fresh, probe[:100]]))
        assert_bf16_of(o16, o32, "gloo-gpu find_or_insert")
        assert bool(f32.all())
        # a tiered shard has no bf16 lookup: refused on every rank before anything is exchanged, fp32 as before
        tsh = ShardedLookupTable(TieredLookupTable(mk(2048), mk(), hot_key_limit=1200), Router(world, BATCH, device=dev))
        with pytest.raises(ValueError):
            tsh.find(probe, out_dtype=BF16)
        tsh.find(probe)
        dist.barrier()
        q.put((rank, None))
        dist.destroy_process_group()
    except BaseException as e:
        import traceback
        q.put(("error", rank, "".join(traceback.format_exception(type(e), e, e.__traceback__))))
        raise


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [16, 64])
def test_sharded_bf16_rccl_single_gpu(dev, dim):
    """world 1 over real RCCL, as tests/test_sharded.py::test_sharded_rccl_single_gpu: bf16 equals the fp32 result rounded"""
    res = _launch(_gpu_rank, 1, ("nccl", dim))
    assert [r[0] for r in res] == [0]
