"""The result stores of the find family (RowStore, meepo_device.h): a 16-byte element group of an fp32 result row leaves through one helper,
as a streaming store under the streaming policy, as a plain store under the cached one.  (The cases were written for write-through
streaming stores, which were measured and not kept — profiles/find_write_through.md; they hold for any store form.)

The policy may change where a line lives, never a byte of the result: every case compares bit for bit (torch.equal) against the CACHED_STORES
result AND against what the table was fed (synth.rows_t / the default value).  Dims 64 and 128 are the compiled row shapes the store acts in,
48 is the run-time shape, which stores cached whatever the flags say.  A wave step is 8 positions at dim 64 and 4 at dim 128: the batch sizes
hit a lone key, a short last step and a full one."""
import pytest
import torch

from meepoembedding_amd import LookupTable, _lib, synth
from test_bf16_rows import rnd
from test_int8_rows import DQ

pytestmark = pytest.mark.gpu

N_KEYS, SEED, DEFAULT = 20_000, 11, 0.625
DIMS = (64, 128, 48)
NS = (1, 7, 8, 9, 31, 4097)
MIXES = ("present", "absent", "reserved")
STREAM3 = _lib.FIND_STREAM_STORES | _lib.FIND_STREAM_ROWS | _lib.FIND_STREAM_BUCKETS
FLAG_SETS = (_lib.FIND_DEFAULT, _lib.FIND_STREAM_STORES, _lib.FIND_STREAM_STORES | _lib.FIND_STREAM_ROWS, STREAM3, _lib.FIND_CACHED_STORES)
SENT, SENT_U8 = -777.25, 0xAB
BF16 = torch.bfloat16
# the serving row types: how such a table is made, and what it stores of fp32 rows, as fp32 (what its fp32 twin is fed)
NARROW_ROWS = {"int8": (dict(int8_rows=True), DQ), "bf16": (dict(value_dtype=BF16), rnd)}


def make_tables(dev):
    """one populated table per dim, and the keys it holds"""
    keys = synth.keys_t(1, 0, N_KEYS, dev)
    out = {}
    for dim in DIMS:
        t = LookupTable(2 * N_KEYS, dim, device=dev, default_value=DEFAULT, max_batch=1 << 15)
        t.insert(keys, synth.rows_t(keys, dim, SEED))
        out[dim] = t
    return keys, out


@pytest.fixture(scope="module")
def tables(dev):
    keys, out = make_tables(dev)
    yield keys, out
    for t in out.values():
        t.close()


def batch_of(keys, n, mix, dev, start=0):
    """n looked-up keys from position `start` of the stored ones; `mix` plants one key that is not stored in the middle of a wave step"""
    k = keys[start:start + n].clone()
    if mix == "absent":
        k[n // 2] = synth.keys_t(99, 5, 1, dev)[0]      # a key of another stream
    elif mix == "reserved":
        k[n // 2] = _lib.EMPTY_KEY
    return k


def expected(k, mix, dim):
    rows = synth.rows_t(k, dim, SEED)
    found = torch.ones(k.numel(), dtype=torch.uint8, device=k.device)
    if mix != "present":
        rows[k.numel() // 2] = DEFAULT
        found[k.numel() // 2] = 0
    return rows, found


@pytest.mark.parametrize("dim", DIMS)
def test_every_policy_gives_the_same_bytes(tables, dev, dim):
    keys, ts = tables
    t = ts[dim]
    for n in NS:
        for mix in MIXES:
            k = batch_of(keys, n, mix, dev, start=n)
            ref_rows, ref_found = expected(k, mix, dim)
            cached, cfound = t.find(k, flags=_lib.FIND_CACHED_STORES)
            for flags in FLAG_SETS:
                out, found = t.find(k, flags=flags)
                what = f"dim {dim} n {n} {mix} flags {flags}"
                assert torch.equal(out, cached) and torch.equal(found, cfound), what
                assert torch.equal(out, ref_rows) and torch.equal(found, ref_found), what


@pytest.mark.parametrize("dim", DIMS)
def test_other_entry_points_give_the_same_rows(tables, dev, dim):
    """the located find, several requests in one launch, the unordered launch"""
    keys, ts = tables
    t = ts[dim]
    for n in NS:
        for mix in MIXES:
            k = batch_of(keys, n, mix, dev, start=3 * n)
            ref_rows, ref_found = expected(k, mix, dim)
            out, found, slots = t.find_located(k)
            assert torch.equal(out, ref_rows) and torch.equal(found, ref_found), (dim, n, mix)
            assert torch.equal(slots >= 0, ref_found.bool()), (dim, n, mix)
            torch.cuda.synchronize(dev)   # (an unordered launch does not wait for the kernels that made `k`)
            out, found = t.find(k, unordered=True)
            assert torch.equal(out, ref_rows) and torch.equal(found, ref_found), (dim, n, mix)
    reqs = [batch_of(keys, n, mix, dev, start=100 * (q + 1)) for q, (n, mix) in enumerate(((9, "absent"), (4097, "present"), (31, "reserved")))]
    for (out, found), k, mix in zip(t.find_many(reqs), reqs, ("absent", "present", "reserved")):
        ref_rows, ref_found = expected(k, mix, dim)
        assert torch.equal(out, ref_rows) and torch.equal(found, ref_found), (dim, mix)


@pytest.mark.parametrize("out_dtype", (torch.float32, BF16), ids=("f32_out", "bf16_out"))
@pytest.mark.parametrize("rows", sorted(NARROW_ROWS))
@pytest.mark.parametrize("dim", DIMS)
def test_narrow_rows_give_the_twins_bytes_under_every_policy(dev, dim, rows, out_dtype):
    """An int8-row table dequantizes in registers, a bf16-row table widens (or hands its 8 bytes on as they are): under every flag set the same
    bytes as under CACHED_STORES, and those are the bytes of the fp32 twin (tests/test_int8_rows.py, tests/test_bf16_rows.py: an fp32 table of
    the same default, fed what the narrow table stores) looked up into the same output type.  The planted position is the default row, found 0."""
    table_kw, stored = NARROW_ROWS[rows]
    keys = synth.keys_t(1, 0, N_KEYS, dev)
    fed = synth.rows_t(keys, dim, SEED)
    t = LookupTable(2 * N_KEYS, dim, device=dev, default_value=DEFAULT, **table_kw)
    tw = LookupTable(2 * N_KEYS, dim, device=dev, default_value=DEFAULT)   # (0.625 is a bf16 value)
    t.insert(keys, fed)
    tw.insert(keys, stored(fed).to(dev))
    bits = (lambda x: x.view(torch.int16)) if out_dtype == BF16 else (lambda x: x.view(torch.int32))
    for n in NS:
        for mix in MIXES:
            k = batch_of(keys, n, mix, dev, start=n)
            ref, ref_found = tw.find(k, flags=_lib.FIND_CACHED_STORES, out_dtype=out_dtype)
            assert torch.equal(ref_found, expected(k, mix, dim)[1])
            if mix != "present":
                assert torch.equal(ref[n // 2], torch.full((dim,), DEFAULT, dtype=out_dtype, device=dev))
            cached, cfound = t.find(k, flags=_lib.FIND_CACHED_STORES, out_dtype=out_dtype)
            for flags in FLAG_SETS:
                out, found = t.find(k, flags=flags, out_dtype=out_dtype)
                what = f"{rows} rows dim {dim} {out_dtype} n {n} {mix} flags {flags}"
                assert out.dtype == out_dtype and torch.equal(bits(out), bits(cached)) and torch.equal(found, cfound), what
                assert torch.equal(bits(out), bits(ref)) and torch.equal(found, ref_found), what
    t.close()
    tw.close()


@pytest.mark.parametrize("dim", DIMS)
def test_nothing_outside_the_result_is_written(tables, dev, dim):
    """`out` starts at row 1 of a larger buffer (aligned to a row and no more) and ends one row before its end"""
    keys, ts = tables
    t = ts[dim]
    for n in NS:
        for mix in MIXES:
            for flags in FLAG_SETS:
                big = torch.full((n + 2, dim), SENT, dtype=torch.float32, device=dev)
                bigf = torch.full((n + 8,), SENT_U8, dtype=torch.uint8, device=dev)
                k = batch_of(keys, n, mix, dev, start=2 * n)
                ref_rows, ref_found = expected(k, mix, dim)
                t.find(k, out=big[1:n + 1], found=bigf[4:n + 4], flags=flags)
                what = f"dim {dim} n {n} {mix} flags {flags}"
                assert torch.equal(big[1:n + 1], ref_rows) and torch.equal(bigf[4:n + 4], ref_found), what
                assert bool((big[0] == SENT).all()) and bool((big[n + 1] == SENT).all()), what
                assert bool((bigf[:4] == SENT_U8).all()) and bool((bigf[n + 4:] == SENT_U8).all()), what


@pytest.mark.parametrize("side_stream", (False, True))
@pytest.mark.parametrize("dim", (64, 128))
def test_no_stale_line(tables, dev, dim, side_stream):
    """A buffer written by streaming stores, read, overwritten by another kernel's plain stores and then by a cached find: every reader
    sees the last writer's bytes.  side_stream: the find runs on a stream of its own, the reader on the main stream behind an event."""
    keys, ts = tables
    t = ts[dim]
    n = 4097
    bufs = [torch.empty((n, dim), dtype=torch.float32, device=dev) for _ in range(2)]
    founds = [torch.empty(n, dtype=torch.uint8, device=dev) for _ in range(2)]
    side = torch.cuda.Stream(device=dev) if side_stream else None
    main = torch.cuda.current_stream(dev)

    def find(k, out, found, flags):
        if side is None:
            t.find(k, out=out, found=found, flags=flags)
            return
        side.wait_stream(main)
        with torch.cuda.stream(side):
            t.find(k, out=out, found=found, flags=flags)
            done = torch.cuda.Event()
            done.record(side)
        main.wait_event(done)

    ok = []
    for rnd in range(12):
        out, found = bufs[rnd % 2], founds[rnd % 2]
        k1 = batch_of(keys, n, "absent", dev, start=rnd * 64)
        k2 = batch_of(keys, n, "present", dev, start=5000 + rnd * 64)
        find(k1, out, found, _lib.FIND_STREAM_STORES)
        r1, f1 = expected(k1, "absent", dim)
        ok.append((out == r1).all() & (found == f1).all())
        out.fill_(float("nan"))
        ok.append(torch.isnan(out).all())
        find(k2, out, found, _lib.FIND_CACHED_STORES)
        r2, f2 = expected(k2, "present", dim)
        ok.append((out == r2).all() & (found == f2).all())
    assert [bool(x) for x in ok] == [True] * len(ok)


@pytest.mark.parametrize("dim", (64, 128))
def test_graph_of_chained_finds(tables, dev, dim):
    """6 chained finds with STREAM_STORES into 3 buffers, captured once, replayed twice: each buffer holds its last batch"""
    keys, ts = tables
    t = ts[dim]
    n = 4097
    ks = [batch_of(keys, n, MIXES[q % 3], dev, start=1000 * q) for q in range(6)]
    bufs = [torch.empty((n, dim), dtype=torch.float32, device=dev) for _ in range(3)]
    founds = [torch.empty(n, dtype=torch.uint8, device=dev) for _ in range(3)]
    t.find(ks[0], out=bufs[0], found=founds[0], flags=_lib.FIND_STREAM_STORES)   # (nothing is allocated lazily inside the capture)
    torch.cuda.synchronize(dev)
    s = torch.cuda.Stream(device=dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            for q in range(6):
                t.find(ks[q], out=bufs[q % 3], found=founds[q % 3], flags=_lib.FIND_STREAM_STORES)
    for _ in range(2):
        for b in bufs:
            b.fill_(SENT)
        g.replay()
        torch.cuda.synchronize(dev)
        for q in (3, 4, 5):
            ref_rows, ref_found = expected(ks[q], MIXES[q % 3], dim)
            assert torch.equal(bufs[q % 3], ref_rows) and torch.equal(founds[q % 3], ref_found), (dim, q)
