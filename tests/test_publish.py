"""GPU: publish (SPEC.md §3 "Publish") — mee_publish_changed / mee_group_publish_changed and LookupTable.publish_to / TableGroup.publish_to.

References: (1) the composition the operator replaces, run on a twin destination: ChangeLog.export_changed(with_state=False), then insert of the
upserts, then remove of the removed keys; (2) the definition: the destination's key-sorted export equals the source's, the rows rounded to bf16 on the
CPU (.to(torch.bfloat16).float(), the rule tests/test_bf16_out.py pins) for a bf16-row destination and bit for bit for an fp32-row one.  Every
comparison of rows is a comparison of bit patterns."""
import numpy as np
import pytest
import torch

from _apply_cases import T, export_sorted
from meepoembedding_amd import OPT_ADAGRAD, OPT_FTRL, OPT_NONE, ChangeLog, LookupTable, MeepoError, TableGroup, _lib, synth

pytestmark = pytest.mark.gpu

FP32, BF16 = "fp32", "bf16"


def bits(x):
    return x.view(np.uint32) if x.dtype == np.float32 else x


def rounded(values, rows):
    """what a destination of that row type holds of fp32 rows"""
    return values if rows == FP32 else torch.from_numpy(values).to(torch.bfloat16).float().numpy()


def serving_table(rows, capacity, dim, dev, **kw):
    return LookupTable(capacity, dim, device=dev, max_batch=4096, value_dtype=torch.bfloat16 if rows == BF16 else torch.float32, **kw)


def filled_from(src, rows, capacity, dev, **kw):
    """a destination that equals `src` (rounded) now"""
    d = serving_table(rows, capacity, src.dim, dev, **kw)
    k, v = src.export()
    d.import_(k, v)
    return d


def raw_publish(src, log, dst, begin, end, counts=None):
    counts = torch.full((4,), -1, dtype=torch.int64, device=dst.device) if counts is None else counts
    rc = _lib.lib().mee_publish_changed(src._h, log._h, dst._h, begin, end, counts.data_ptr(), torch.cuda.current_stream(dst.device).cuda_stream)
    return rc, counts


def compose(src, log, dst, ranges=None):
    """the composition over a partition of the log's slots -> (upserts, removed)"""
    n = r = 0
    for b, e in ranges or [(0, log.capacity)]:
        k, v, _, _, gone = log.export_changed(src, b, e, with_state=False)
        for s in range(0, k.numel(), dst.max_batch):
            dst.insert(k[s:s + dst.max_batch], v[s:s + dst.max_batch])
        for s in range(0, gone.numel(), dst.max_batch):
            dst.remove(gone[s:s + dst.max_batch])
        n, r = n + k.numel(), r + gone.numel()
    return n, r


def assert_same_tables(a, b, what):
    ea, eb = export_sorted(a), export_sorted(b)
    assert len(ea) == len(eb) == 2
    assert np.array_equal(ea[0], eb[0]), f"{what}: keys"
    assert np.array_equal(bits(ea[1]), bits(eb[1])), f"{what}: values"
    assert a.size() == b.size() == ea[0].size and a.status() == b.status(), f"{what}: size or status"


def assert_is_rounded_source(dst, src, rows, what):
    ed, es = export_sorted(dst), export_sorted(src)
    assert np.array_equal(ed[0], es[0]), f"{what}: the key sets differ"
    assert np.array_equal(bits(ed[1]), bits(rounded(es[1], rows))), f"{what}: a row is not the source's row" + (" rounded once" if rows == BF16 else "")
    assert dst.size() == src.size()


def step(t, k, dev, seed):
    g = T((synth.rows_np(k, t.dim, seed) * 0.02).astype(np.float32), dev)
    if t.optimizer == OPT_ADAGRAD:
        t.apply_adagrad(T(k, dev), g, lr=0.05)
    elif t.optimizer == OPT_FTRL:
        t.apply_ftrl(T(k, dev), g, lr=0.05, l1=0.001)


# ---- 1. bit for bit against the composition and against the definition ---------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [FP32, BF16])
@pytest.mark.parametrize("opt", [OPT_NONE, OPT_ADAGRAD, OPT_FTRL])
@pytest.mark.parametrize("dim", [8, 64, 104, 128])
def test_publish_bit_for_bit(dev, rows, opt, dim):
    rng = np.random.default_rng(dim * 7 + opt)
    t = LookupTable(8192, dim, device=dev, optimizer=opt, max_batch=4096, initial_accumulator=0.1, initializer=_lib.INIT_UNIFORM, init_scale=0.05, init_seed=3)
    pool = synth.keys_np(13, 0, 5000)
    old, new, unseen, never = pool[:3000], pool[3000:3500], pool[3500:3600], pool[3600:3650]
    t.insert(T(old, dev), T(synth.rows_np(old, dim, 2), dev))
    step(t, old, dev, 5)
    d1, d2 = (filled_from(t, rows, 12288, dev) for _ in range(2))          # another capacity: every key sits in another slot than in t
    log = t.track_changes(6000)
    want = set()

    def did(k):
        want.update(k.tolist())

    t.insert(T(new, dev), T(synth.rows_np(new, dim, 3), dev)); did(new)
    a = old[rng.choice(3000, 300, replace=False)]
    t.assign(T(a, dev), T(synth.rows_np(a, dim, 4), dev)); did(a)
    if opt != OPT_NONE:
        s = np.concatenate([old[rng.integers(0, 3000, 800)], new[:50], new[:50]])   # duplicates
        step(t, s, dev, 6); did(s)
    gone = np.concatenate([old[rng.choice(3000, 200, replace=False)], never])       # `never` was never stored
    t.remove(T(gone, dev)); did(gone)
    back = gone[:1]
    t.insert(T(back, dev), T(synth.rows_np(back, dim, 8), dev)); did(back)          # removed, then inserted again
    t.find_or_insert(T(unseen, dev)); did(unseen)
    assert not log.invalid and log.size() == len(want)
    src_before, noted_before = export_sorted(t), log.size()
    third = log.capacity // 3
    ranges = [(0, third - 5), (third - 5, 2 * third + 3), (2 * third + 3, log.capacity + 1000)]   # uneven; the last end lies beyond the log
    assert (third - 5) % 64 and (2 * third + 3) % 64
    total = np.zeros(4, dtype=np.int64)
    for b, e in ranges:
        rc, counts = raw_publish(t, log, d1, b, e)
        assert rc == 0, _lib.lib().mee_last_error()
        total += np.array(counts.tolist())
    compose(t, log, d2, ranges)
    assert_same_tables(d1, d2, "publish against the composition")
    assert_is_rounded_source(d1, t, rows, "publish against the definition")
    assert d1.status() == 0
    held = len(want & set(src_before[0].tolist()))
    assert total.tolist() == [held, len(want) - held, 0, 0]
    after = export_sorted(t)
    assert len(after) == len(src_before) and all(np.array_equal(bits(x), bits(z)) for x, z in zip(after, src_before)), "the source was written"
    assert log.size() == noted_before and not log.invalid, "the log was written"


# ---- 2. refusals, before anything is launched or written -----------------------------------------------------------------------------------------
REFUSALS = ["null_src", "null_log", "null_dst", "null_counts", "same_table", "dim", "device", "dst_optimizer", "src_bf16", "src_int8", "dst_int8"]


@pytest.mark.parametrize("case", REFUSALS)
def test_refusals_leave_everything_untouched(dev, case):
    dim = 16
    keys = synth.keys_np(50, 0, 120)
    vals = T(synth.rows_np(keys, dim, 2), dev)
    plain = dict(device=dev, max_batch=256)
    src = LookupTable(256, dim, optimizer=OPT_ADAGRAD, **plain)
    dst = LookupTable(256, dim, **plain)
    log = ChangeLog(256, dev)
    if case == "same_table":
        src = dst
    elif case == "dim":
        dst = LookupTable(256, 32, **plain)
        vals = T(synth.rows_np(keys, 32, 2), dev)
    elif case == "device":
        if torch.cuda.device_count() < 2:
            pytest.skip("needs a second GPU")
        dst = LookupTable(256, dim, device=torch.device("cuda", 1), max_batch=256)
        vals = vals.to(dst.device)
    elif case == "dst_optimizer":
        dst = LookupTable(256, dim, optimizer=OPT_ADAGRAD, **plain)
    elif case == "src_bf16":
        src = LookupTable(256, dim, value_dtype=torch.bfloat16, **plain)
    elif case == "src_int8":
        src = LookupTable(256, dim, int8_rows=True, **plain)
    elif case == "dst_int8":
        dst = LookupTable(256, dim, int8_rows=True, **plain)
    dst.insert(T(keys[:60], dev).to(dst.device), vals[:60])
    if src is not dst:
        src.insert(T(keys[40:], dev), T(synth.rows_np(keys[40:], src.dim, 3), dev))
    log.note(T(keys, dev))
    before = export_sorted(dst)
    counts = torch.full((4,), -1, dtype=torch.int64, device=dst.device)
    L, st = _lib.lib(), torch.cuda.current_stream(dev).cuda_stream
    args = [src._h, log._h, dst._h, 0, log.capacity, counts.data_ptr(), st]
    for name, i in (("null_src", 0), ("null_log", 1), ("null_dst", 2), ("null_counts", 5)):
        if case == name:
            args[i] = None
    rc = L.mee_publish_changed(*args)
    unsupported = case in ("dst_optimizer", "src_bf16", "src_int8", "dst_int8")
    assert rc == (_lib.ERR_UNSUPPORTED if unsupported else _lib.ERR_INVALID_ARG), case
    assert L.mee_last_error().startswith(b"mee_publish_changed:")
    torch.cuda.synchronize()
    after = export_sorted(dst)
    assert counts.tolist() == [-1] * 4 and all(np.array_equal(bits(x), bits(z)) for x, z in zip(before, after)) and log.size() == 120


def test_an_empty_range_zeroes_the_counts(dev):
    dim = 16
    keys = synth.keys_np(51, 0, 50)
    src, dst, log = LookupTable(256, dim, device=dev, max_batch=256), LookupTable(256, dim, device=dev, max_batch=256), ChangeLog(256, dev)
    src.insert(T(keys, dev), T(synth.rows_np(keys, dim, 2), dev))
    log.note(T(keys, dev))
    for b, e in ((7, 7), (9, 3), (log.capacity, log.capacity + 5)):
        rc, counts = raw_publish(src, log, dst, b, e)
        assert rc == 0 and counts.tolist() == [0, 0, 0, 0]
    assert dst.size() == 0


def test_group_refusals(dev):
    dim = 16
    mk = lambda **kw: LookupTable(256, dim, device=dev, max_batch=256, **kw)
    src = TableGroup([mk(), mk(optimizer=OPT_ADAGRAD)])
    src.track_changes(64)
    ok = TableGroup([mk(), mk()])
    counts = torch.full((2, 4), -1, dtype=torch.int64, device=dev)
    L, st = _lib.lib(), torch.cuda.current_stream(dev).cuda_stream
    call = lambda s, d, c=counts: L.mee_group_publish_changed(s._h, src._change_group._h, d._h, None if c is None else c.data_ptr(), st)
    assert call(src, ok, None) == _lib.ERR_INVALID_ARG and L.mee_last_error().startswith(b"mee_group_publish_changed:")
    assert call(src, src) == _lib.ERR_INVALID_ARG
    one, wide = TableGroup([mk()]), TableGroup([LookupTable(256, 32, device=dev, max_batch=256) for _ in range(2)])
    assert call(src, one) == _lib.ERR_INVALID_ARG and call(src, wide) == _lib.ERR_INVALID_ARG          # another number of tables, another dim
    shared = TableGroup([mk(), src.tables[0]])
    assert call(src, shared) == _lib.ERR_INVALID_ARG                                                    # a table on both sides
    trained = TableGroup([mk(), mk(optimizer=OPT_ADAGRAD)])
    assert call(src, trained) == _lib.ERR_UNSUPPORTED
    bf = TableGroup([mk(value_dtype=torch.bfloat16), mk(value_dtype=torch.bfloat16)])
    assert call(bf, ok) == _lib.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert counts.tolist() == [[-1] * 4] * 2 and all(t.size() == 0 for t in ok.tables)
    assert call(src, ok) == 0 and counts.tolist() == [[0] * 4] * 2
    assert call(src, bf) == 0


# ---- 3. tombstones made and reused in one call sequence ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [FP32, BF16])
def test_tombstones_are_reused(dev, rows):
    dim = 64
    pool = synth.keys_np(52, 0, 120)
    src = LookupTable(1024, dim, device=dev, optimizer=OPT_ADAGRAD, max_batch=256)
    src.insert(T(pool[:40], dev), T(synth.rows_np(pool[:40], dim, 2), dev))
    d1, d2 = (filled_from(src, rows, 64, dev) for _ in range(2))
    assert d1.capacity == 80                                              # 16 x the smallest prime >= 64 / 16: the nearest a table gets to 64 slots
    log = src.track_changes(256)

    def publish_and_compare(what, expect):
        assert src.publish_to(d1) == expect
        assert compose(src, log, d2) == expect[:2]
        log.clear()
        assert_same_tables(d1, d2, what)
        assert_is_rounded_source(d1, src, rows, what)
        ks, vs = src.export()
        got, found = d1.find(ks)
        assert bool(found.all()), f"{what}: a key of the source is not found behind the tombstones"
        assert np.array_equal(bits(got.cpu().numpy()), bits(rounded(vs.cpu().numpy(), rows)))

    src.remove(T(pool[:30], dev))
    src.insert(T(pool[40:70], dev), T(synth.rows_np(pool[40:70], dim, 3), dev))
    publish_and_compare("30 leave, 30 others arrive", (30, 30, 0))      # 70 of 80 slots are keys or tombstones now
    src.insert(T(pool[:10], dev), T(synth.rows_np(pool[:10], dim, 4), dev))
    publish_and_compare("10 of the removed come back", (10, 0, 0))
    src.insert(T(pool[70:95], dev), T(synth.rows_np(pool[70:95], dim, 5), dev))
    publish_and_compare("25 more than the EMPTY slots left: tombstones take them", (25, 0, 0))   # at most 10 slots were still EMPTY
    assert d1.size() == 75 and d1.status() == 0


# ---- 4. no room ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [FP32, BF16])
def test_no_room_drops_and_reports(dev, rows):
    dim = 64
    keys = synth.keys_np(53, 0, 100)
    src = LookupTable(1024, dim, device=dev, optimizer=OPT_ADAGRAD, max_batch=256)
    log = src.track_changes(512)
    src.insert(T(keys, dev), T(synth.rows_np(keys, dim, 2), dev))
    dst = serving_table(rows, 16, dim, dev)
    assert dst.capacity == 32
    src_before = export_sorted(src)
    rc, counts = raw_publish(src, log, dst, 0, log.capacity)
    assert rc == 0
    c = counts.tolist()
    assert c[0] + c[2] == 100 and c[0] == dst.size() == 32 and c[2] == 68 and c[1] == 0 and c[3] == 0
    assert dst.status() & _lib.STATUS_TABLE_FULL and not src.status() & _lib.STATUS_TABLE_FULL
    # which 32 keys made it is decided by a race; each of them has its row
    k, v = (x.cpu().numpy() for x in dst.export())
    pos = {int(key): i for i, key in enumerate(src_before[0])}
    assert all(int(key) in pos for key in k)
    assert np.array_equal(bits(v), bits(rounded(src_before[1][[pos[int(key)] for key in k]], rows)))
    assert all(np.array_equal(bits(x), bits(z)) for x, z in zip(export_sorted(src), src_before))
    with pytest.raises(MeepoError, match="68 keys"):
        src.publish_to(dst, check=True)                                   # the 32 are found again, the 68 dropped again
    assert dst.size() == 32


# ---- 5. an invalid log ---------------------------------------------------------------------------------------------------------------------------
def test_invalid_log_is_reported_not_synchronised(dev):
    dim = 64
    keys = synth.keys_np(54, 0, 200)
    src = LookupTable(1024, dim, device=dev, optimizer=OPT_ADAGRAD, max_batch=256)
    log = src.track_changes(16)
    src.insert(T(keys, dev), T(synth.rows_np(keys, dim, 2), dev))
    assert log.invalid and 0 < log.size() <= log.capacity == 32
    dst = serving_table(BF16, 1024, dim, dev)
    counts = src.publish_to(dst, check=False)
    assert isinstance(counts, torch.Tensor) and counts.is_cuda and counts.dtype == torch.int64 and tuple(counts.shape) == (4,)
    c = counts.tolist()
    assert c[3] != 0 and c[0] == log.size() and c[1] == 0 and c[2] == 0
    with pytest.raises(RuntimeError, match="rebuild the serving copy") as err:
        src.publish_to(dst, check=True)
    assert not isinstance(err.value, MeepoError)
    # the keys the log does name are published correctly
    named = torch.cat([p[0] for p in log.iter_changed(src, with_state=False)])
    ed = export_sorted(dst)
    assert np.array_equal(ed[0], np.sort(named.cpu().numpy()))
    want, found = src.find(T(ed[0], dev))
    assert bool(found.all()) and np.array_equal(bits(ed[1]), bits(rounded(want.cpu().numpy(), BF16)))


# ---- 6. groups -----------------------------------------------------------------------------------------------------------------------------------
def test_group_publish(dev):
    from meepoembedding_amd.nn import DynamicEmbeddingBag
    dim, nt = 64, 3
    caps, log_caps = (2048, 4096, 1024), (100, 3000, 1500)
    tables = [LookupTable(c, dim, device=dev, optimizer=OPT_ADAGRAD, max_batch=4096, initial_accumulator=0.1, initializer=_lib.INIT_UNIFORM, init_scale=0.05,
                          init_seed=j) for j, c in enumerate(caps)]
    member_keys = [synth.keys_np(60 + j, 0, 900) for j in range(nt)]
    for j, t in enumerate(tables):
        t.insert(T(member_keys[j][:300], dev), T(synth.rows_np(member_keys[j][:300], dim, 2), dev))
    g = TableGroup(tables, max_apply_batch=4096)
    logs = g.track_changes(list(log_caps))
    assert [lg.capacity for lg in logs] == [112, 3056, 1552] and all(lg.capacity % 64 for lg in logs)
    serving = g.serving_copy()
    plain = TableGroup([filled_from(t, FP32, t.capacity + 512, dev) for t in tables])
    rng = np.random.default_rng(6)
    want = [set() for _ in range(nt)]
    # the bag layer: 20 bags per member; member 0 draws on few keys (its log is small), member 2's bags are all empty
    bags = [member_keys[0][280 + rng.integers(0, 40, 60)], member_keys[1][rng.integers(200, 700, 60)], member_keys[2][:0]]
    bag_offsets = np.concatenate([np.arange(0, 121, 3), np.full(20, 120)]).astype(np.int64)
    layer = DynamicEmbeddingBag(g, mode="sum", optimizer="adagrad", lr=0.05, create_missing=True)
    out = layer(T(np.concatenate(bags), dev), T(bag_offsets, dev))
    out.backward(T(synth.rows_np(np.arange(out.shape[0], dtype=np.int64), dim, 7) * 0.1, dev))
    # a plain grouped step on a jagged batch
    segs = [member_keys[0][290 + rng.integers(0, 20, 50)], member_keys[1][rng.integers(0, 300, 400)], member_keys[2][:0]]
    flat = np.concatenate(segs)
    offsets = np.cumsum([0] + [s.size for s in segs]).astype(np.int64)
    g.apply_adagrad(T(flat, dev), T(offsets, dev), T((synth.rows_np(flat, dim, 8) * 0.02).astype(np.float32), dev), lr=0.05)
    gone = np.concatenate([member_keys[1][100:160], member_keys[1][880:890]])     # 60 stored keys and 10 that never were
    tables[1].remove(T(gone, dev))
    for j in range(nt):
        want[j] |= set(bags[j].tolist()) | set(segs[j].tolist())
    want[1] |= set(gone.tolist())
    assert not any(lg.invalid for lg in logs) and [lg.size() for lg in logs] == [len(w) for w in want] and logs[2].size() == 0
    expect = []
    for j in range(nt):
        stored = set(export_sorted(tables[j])[0].tolist())
        held = len(want[j] & stored)
        expect.append((held, len(want[j]) - held, 0))
    assert expect[2] == (0, 0, 0) and expect[1][1] == 70 and expect[0][0] > 0
    fresh = g.serving_copy()                                              # the definition: the trained group, rounded, now
    q = [member_keys[j][rng.integers(0, 900, 90)] for j in range(nt)]
    q_off = T(np.arange(0, 271, 3, dtype=np.int64), dev)
    for dst, rows in ((serving, BF16), (plain, FP32)):
        assert g.publish_to(dst) == expect, rows
        for j in range(nt):
            assert_is_rounded_source(dst.tables[j], tables[j], rows, f"member {j} ({rows})")
            assert dst.tables[j].status() == 0
        got, found = dst.find_pooled(T(np.concatenate(q), dev), q_off)
        for j in range(nt):
            ref = fresh.tables[j] if rows == BF16 else tables[j]
            exp, efound = ref.find_pooled(T(q[j], dev), T(np.arange(0, 91, 3, dtype=np.int64), dev))
            assert np.array_equal(bits(got[30 * j:30 * (j + 1)].cpu().numpy()), bits(exp.cpu().numpy())), f"pooled lookup, member {j} ({rows})"
            assert torch.equal(found[90 * j:90 * (j + 1)], efound)
        # again, without further training: over-noting is harmless and the counts repeat
        before = [export_sorted(t) for t in dst.tables]
        assert g.publish_to(dst) == expect
        for j in range(nt):
            assert all(np.array_equal(bits(x), bits(z)) for x, z in zip(before[j], export_sorted(dst.tables[j])))
    counts = g.publish_to(serving, check=False, clear=True)
    assert counts.is_cuda and tuple(counts.shape) == (nt, 4) and [tuple(c[:3]) for c in counts.tolist()] == expect
    assert [lg.size() for lg in logs] == [0, 0, 0]


# ---- 7. capture ----------------------------------------------------------------------------------------------------------------------------------
def test_note_and_publish_under_stream_capture(dev):
    dim = 64
    pool = synth.keys_np(70, 0, 1600)
    src = LookupTable(4096, dim, device=dev, optimizer=OPT_ADAGRAD, max_batch=1024, initial_accumulator=0.1)
    src.insert(T(pool[:1000], dev), T(synth.rows_np(pool[:1000], dim, 2), dev))
    d1, d2 = (filled_from(src, BF16, 2048, dev) for _ in range(2))
    log = ChangeLog(2048, dev)                                            # the captured note is the only one: src itself is not tracked
    batches = [np.concatenate([pool[100:250], pool[1000:1100]]), np.concatenate([pool[197:300], pool[1100:1247]])]   # both of 250 keys
    buf = T(batches[0], dev)
    assert buf.numel() == batches[1].size
    log.publish(src, d1)                                                  # (an empty log: nothing happens; the kernels are loaded before the capture)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        log.note(buf)
        counts = log.publish(src, d1)
    for i, batch in enumerate(batches):
        buf.copy_(T(batch, dev))
        src.find_or_insert(T(batch, dev))                                 # new ids enter
        step(src, batch, dev, 20 + i)                                     # every row of the batch changes
        src.remove(T(batch[:30], dev))                                    # ... and some leave
        graph.replay()
        torch.cuda.synchronize(dev)
        n, r = compose(src, log, d2)
        noted_now = log.size()
        assert counts.tolist() == [n, r, 0, 0] and n + r == noted_now
        assert_same_tables(d1, d2, f"replay {i}")
        assert_is_rounded_source(d1, src, BF16, f"replay {i}")


# ---- 8. an int8-row destination, by composition --------------------------------------------------------------------------------------------------
def test_int8_destination_by_composition(dev):
    dim = 64
    pool = synth.keys_np(80, 0, 1500)
    src = LookupTable(4096, dim, device=dev, optimizer=OPT_ADAGRAD, max_batch=1024, initial_accumulator=0.1)
    src.insert(T(pool[:1000], dev), T(synth.rows_np(pool[:1000], dim, 2), dev))
    mk = lambda: LookupTable(4096, dim, device=dev, max_batch=300, int8_rows=True)
    serving = mk()
    serving.import_(*src.export())
    src.track_changes(4096)
    src.insert(T(pool[1000:1400], dev), T(synth.rows_np(pool[1000:1400], dim, 3), dev))
    step(src, pool[500:1200], dev, 4)
    gone = pool[:120]
    src.remove(T(gone, dev))
    up, rem, dropped = src.publish_to(serving)
    assert dropped is None and rem == 120 and up == 400 + 500 and serving.status() == 0   # 1000..1399 new, 500..999 stepped (1000..1199 both), 0..119 gone
    fresh = mk()
    fresh.import_(*src.export())
    ks = src.export()[0]
    got, found = serving.find(ks)
    exp, efound = fresh.find(ks)
    assert bool(found.all()) and bool(efound.all()) and np.array_equal(bits(got.cpu().numpy()), bits(exp.cpu().numpy()))
    assert not bool(serving.find(T(gone, dev))[1].any()) and serving.size() == src.size()


# ---- a destination that counts hits --------------------------------------------------------------------------------------------------------------
def test_created_slots_start_at_counter_zero(dev):
    dim = 64
    keys = synth.keys_np(90, 0, 60)
    src = LookupTable(1024, dim, device=dev, optimizer=OPT_ADAGRAD, max_batch=256)
    src.insert(T(keys[:40], dev), T(synth.rows_np(keys[:40], dim, 2), dev))
    d1, d2 = (filled_from(src, FP32, 64, dev, track_hits=True) for _ in range(2))
    nine = torch.full((40,), 9, dtype=torch.int32, device=dev)
    for d in (d1, d2):
        d.set_hits(T(keys[:40], dev), nine)
    log = src.track_changes(256)
    src.remove(T(keys[:20], dev))                                         # their slots become tombstones whose counters still read 9
    assert src.publish_to(d1) == (0, 20, 0) and compose(src, log, d2) == (0, 20)
    log.clear()
    src.insert(T(keys[:60], dev), T(synth.rows_np(keys[:60], dim, 3), dev))   # 20 come back, 20 are overwritten, 20 are new
    assert src.publish_to(d1) == (60, 0, 0) and compose(src, log, d2) == (60, 0)
    assert_same_tables(d1, d2, "a destination with hit counters")
    h1, h2 = d1.hits_of(T(keys, dev)).cpu().numpy(), d2.hits_of(T(keys, dev)).cpu().numpy()
    assert np.array_equal(h1, h2) and (h1[:20] == 0).all() and (h1[20:40] == 9).all() and (h1[40:] == 0).all()
