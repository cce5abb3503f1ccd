"""GPU: the change log and the delta export (SPEC.md §3 "Change log") — mee_changes_note / _group_note, mee_export_changed, the mutators' hooks in
LookupTable and TableGroup, and checkpoint.save_base / save_delta / restore on top of them.

References: the set a log must hold is computed on the host from the batches the test handed to the mutators; an exported row is compared, as bit
patterns, with find / find_plane of the same key; the contract is checked end to end: a table restored from base + deltas equals the trained table in
key-sorted export(with_state=True), bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from _apply_cases import T, export_sorted
from meepoembedding_amd import OPT_ADAGRAD, OPT_ADAM, OPT_FTRL, OPT_NONE, ChangeLog, LookupTable, MeepoError, TableGroup, _lib, checkpoint, synth

pytestmark = pytest.mark.gpu

EMPTY, RECLAIMED = _lib.EMPTY_KEY, _lib.RECLAIMED_KEY
KEY_SENTINEL = 0x5A5A5A5A5A5A5A5A
ROW_SENTINEL = 777.0
WAVE_STEP = 8   # keys a wave of the note kernel takes per step (4 tiles x 2)


def bits(x):
    return x.view(np.uint32) if x.dtype == np.float32 else x


def raw_export(log, t, begin, end, pad=7, cap=None, with_state=True):
    """mee_export_changed into sentinel-filled buffers `pad` entries longer than the range -> (keys, values, s1, s2, removed) as numpy, cut at the
    counts, after checking that nothing was written at or past them"""
    end = min(end, log.capacity)
    slots = max(end - begin, 0)
    cap = slots if cap is None else cap
    dev, dim = t.device, t.dim
    rows = lambda: torch.full((cap + pad, dim), ROW_SENTINEL, dtype=torch.float32, device=dev)
    keys = torch.full((cap + pad,), KEY_SENTINEL, dtype=torch.int64, device=dev)
    removed = torch.full((cap + pad,), KEY_SENTINEL, dtype=torch.int64, device=dev)
    vals = rows()
    s1 = rows() if with_state and t.optimizer != OPT_NONE else None
    s2 = rows() if with_state and t.optimizer in (OPT_ADAM, OPT_FTRL) else None
    counts = torch.full((2,), -1, dtype=torch.int64, device=dev)
    rc = _lib.lib().mee_export_changed(t._h, log._h, begin, end, keys.data_ptr(), vals.data_ptr(), s1.data_ptr() if s1 is not None else None,
                                       s2.data_ptr() if s2 is not None else None, cap, removed.data_ptr(), cap, counts.data_ptr(),
                                       torch.cuda.current_stream(dev).cuda_stream)
    bufs = [keys, vals, s1, s2, removed]
    if rc != 0:
        return rc, bufs, counts
    n, r = (int(x) for x in counts.tolist())
    assert 0 <= n <= slots and 0 <= r <= slots
    assert bool((keys[n:] == KEY_SENTINEL).all()) and bool((removed[r:] == KEY_SENTINEL).all()), "written at or past the counts"
    for p in (vals, s1, s2):
        assert p is None or bool((p[n:] == ROW_SENTINEL).all()), "a row written at or past the count"
    return tuple(None if b is None else b[: (r if b is removed else n)].cpu().numpy() for b in bufs)


def noted(log, t, ranges=None):
    """every key the log holds, through export_changed over `ranges` of its slots (default: one range) -> sorted numpy array"""
    ranges = ranges or [(0, log.capacity)]
    out = []
    for b, e in ranges:
        k, _, _, _, r = raw_export(log, t, b, e, with_state=False)
        out += [k, r]
    return np.sort(np.concatenate(out))


@pytest.fixture(scope="module")
def empty_table(dev):
    return LookupTable(64, 4, device=dev, max_batch=64)


# ---- set semantics ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity,pool", [(1, 24), (4000, 1500)])
def test_note_is_a_set(dev, empty_table, capacity, pool):
    log = ChangeLog(capacity, dev)
    assert log.capacity == {1: 32, 4000: 16 * 251}[capacity] and log.size() == 0 and not log.invalid
    rng = np.random.default_rng(capacity)
    keys = synth.keys_np(11, 0, pool)
    keys[:3] = [-1, -(1 << 62), 5]
    assert (keys < 0).any() and (keys > 0).any()
    want = set()
    for n in (1, 63, 4 * WAVE_STEP * 5 + 3):   # no multiple of the wave step
        batch = keys[rng.integers(0, pool, n)]
        log.note(T(batch, dev))
        want |= set(batch.tolist())
    # every key twice, the second occurrence in another wave, with padding in between
    big = np.concatenate([keys, [EMPTY, RECLAIMED, EMPTY], keys[::-1], [RECLAIMED]]).astype(np.int64)
    assert big.size % WAVE_STEP
    log.note(T(big, dev))
    want |= set(keys.tolist())
    assert len(want) == pool and log.size() == pool and not log.invalid
    log.note(T(big, dev))                                       # noting again changes nothing
    log.note(torch.empty(0, dtype=torch.int64, device=dev))     # n = 0
    assert log.size() == pool and not log.invalid
    got = noted(log, empty_table, [(0, 7), (7, 40), (40, log.capacity)])
    assert np.array_equal(got, np.sort(np.array(sorted(want), dtype=np.int64))), "every noted key exactly once, reserved keys never"
    pieces = list(log.iter_changed(empty_table, chunk_slots=13, with_state=False))
    assert np.array_equal(np.sort(torch.cat([p[4] for p in pieces]).cpu().numpy()), got) and all(p[0].numel() == 0 for p in pieces)


def test_refusals_before_any_launch(dev, empty_table):
    L, log = _lib.lib(), ChangeLog(64, dev)
    assert L.mee_changes_note(None, None, 0, None) == _lib.ERR_INVALID_ARG
    assert L.mee_changes_note(log._h, None, 5, None) == _lib.ERR_INVALID_ARG
    assert L.mee_changes_note(log._h, None, 0, None) == 0
    assert L.mee_changes_group_note(None, None, None, 0, None) == _lib.ERR_INVALID_ARG
    assert L.mee_export_changed(None, log._h, 0, 1, None, None, None, None, 0, None, 0, None, None) == _lib.ERR_INVALID_ARG
    log.note(T(np.arange(1, 41, dtype=np.int64), dev))
    # a cap below the number of slots in the range: refused, outputs untouched
    rc, bufs, counts = raw_export(log, empty_table, 0, 48, cap=47)
    assert rc == _lib.ERR_INVALID_ARG and b"cap" in L.mee_last_error()
    assert bool((bufs[0] == KEY_SENTINEL).all()) and bool((bufs[4] == KEY_SENTINEL).all()) and bool((bufs[1] == ROW_SENTINEL).all()) and counts.tolist() == [-1, -1]
    # serving tables have no training delta
    for kw in (dict(value_dtype=torch.bfloat16), dict(int8_rows=True)):
        narrow = LookupTable(64, 16, device=dev, max_batch=64, **kw)
        rc, bufs, counts = raw_export(log, narrow, 0, 48)
        assert rc == _lib.ERR_UNSUPPORTED and bool((bufs[0] == KEY_SENTINEL).all()) and bool((bufs[1] == ROW_SENTINEL).all()) and counts.tolist() == [-1, -1]
        with pytest.raises(MeepoError):
            narrow.track_changes(64)
    # an empty range is fine and zeroes the counts
    k, v, s1, s2, r = raw_export(log, empty_table, 48, 48)
    assert k.size == 0 and r.size == 0
    assert log.size() == 40


# ---- overflow -----------------------------------------------------------------------------------------------------------------------------------
def test_overflow_sets_invalid_and_touches_nothing_else(dev, empty_table, tmp_path):
    before, log, after = ChangeLog(1, dev), ChangeLog(1, dev), ChangeLog(1, dev)   # the key plane's neighbours
    t = LookupTable(512, 4, device=dev, optimizer=OPT_ADAGRAD, max_batch=512)
    t.change_log = log
    n = 10 * log.capacity
    buf = torch.full((n + 64,), KEY_SENTINEL, dtype=torch.int64, device=dev)        # guards around the batch
    keys = synth.keys_np(12, 0, n)
    buf[32:32 + n] = T(keys, dev)
    log.note(buf[32:32 + n])
    assert log.invalid and 0 < log.size() <= log.capacity
    assert bool((buf[:32] == KEY_SENTINEL).all()) and bool((buf[32 + n:] == KEY_SENTINEL).all()) and np.array_equal(buf[32:32 + n].cpu().numpy(), keys)
    got = noted(log, empty_table)
    assert got.size == log.size() and np.isin(got, keys).all() and np.unique(got).size == got.size
    for other in (before, after):
        assert other.size() == 0 and not other.invalid and noted(other, empty_table).size == 0
    log.save_id = "0" * 16
    with pytest.raises(RuntimeError, match="invalid"):
        checkpoint.save_delta(t, str(tmp_path / "d"))
    assert not os.path.exists(tmp_path / "d" / "meta.json")
    log.clear()
    assert log.size() == 0 and not log.invalid and noted(log, empty_table).size == 0
    log.note(T(keys[:20], dev))
    assert log.size() == 20 and not log.invalid
    log.invalidate()
    assert log.invalid and log.size() == 20


# ---- export_changed, bit for bit ----------------------------------------------------------------------------------------------------------------
def step(t, k, dev, seed):
    g = T((synth.rows_np(k, t.dim, seed) * 0.02).astype(np.float32), dev)
    if t.optimizer == OPT_ADAGRAD:
        t.apply_adagrad(T(k, dev), g, lr=0.05)
    elif t.optimizer == OPT_ADAM:
        t.apply_adam(T(k, dev), g, lr=0.01, step=3)
    elif t.optimizer == OPT_FTRL:
        t.apply_ftrl(T(k, dev), g, lr=0.05, l1=0.001)


@pytest.mark.parametrize("opt", [OPT_NONE, OPT_ADAGRAD, OPT_ADAM, OPT_FTRL])
@pytest.mark.parametrize("dim", [4, 64, 100, 128])
def test_export_changed_bit_for_bit(dev, opt, dim):
    rng = np.random.default_rng(dim * 7 + opt)
    t = LookupTable(8192, dim, device=dev, optimizer=opt, max_batch=4096, initial_accumulator=0.1, initializer=_lib.INIT_UNIFORM, init_scale=0.05, init_seed=3)
    pool = synth.keys_np(13, 0, 5000)
    old, new, unseen, never = pool[:3000], pool[3000:3500], pool[3500:3600], pool[3600:3650]
    t.insert(T(old, dev), T(synth.rows_np(old, dim, 2), dev))
    step(t, old, dev, 5)                                          # state planes are not their initial values
    log = t.track_changes(6000)
    assert t.change_log is log and log.size() == 0
    want = set()

    def did(k):
        want.update(k.tolist())

    t.insert(T(new, dev), T(synth.rows_np(new, dim, 3), dev)); did(new)
    a = old[rng.choice(3000, 300, replace=False)]
    t.assign(T(a, dev), T(synth.rows_np(a, dim, 4), dev)); did(a)
    if opt != OPT_NONE:
        s = np.concatenate([old[rng.integers(0, 3000, 800)], new[:50], new[:50]])   # duplicates
        step(t, s, dev, 6); did(s)
    gone = np.concatenate([old[rng.choice(3000, 200, replace=False)], never])       # `never` was never stored: removed from nowhere
    t.remove(T(gone, dev)); did(gone)
    back = gone[:1]
    t.insert(T(back, dev), T(synth.rows_np(back, dim, 8), dev)); did(back)          # removed, then inserted again
    t.find_or_insert(T(unseen, dev)); did(unseen)
    assert not log.invalid and log.size() == len(want)
    third = log.capacity // 3
    ups, rem = [], []
    for b, e in ((0, third - 5), (third - 5, 2 * third + 3), (2 * third + 3, log.capacity)):
        k, v, s1, s2, r = raw_export(log, t, b, e)
        rem.append(r)
        if not k.size:
            continue
        kt = T(k, dev)
        rows, found = t.find(kt)
        assert bool(found.all()), "an upsert key the table does not hold"
        assert np.array_equal(bits(v), bits(rows.cpu().numpy())), "values"
        for plane, got in ((1, s1), (2, s2)):
            assert (got is None) == (plane > {OPT_NONE: 0, OPT_ADAGRAD: 1, OPT_ADAM: 2, OPT_FTRL: 2}[opt])
            if got is not None:
                assert np.array_equal(bits(got), bits(t.find_plane(plane, kt)[0].cpu().numpy())), f"state{plane}"
        ups.append(k)
    ups, rem = np.concatenate(ups), np.concatenate(rem)
    assert not bool(t.locate(T(rem, dev))[1].any()), "a removed key the table holds"
    both = np.concatenate([ups, rem])
    assert np.unique(both).size == both.size == len(want) and set(both.tolist()) == want, "the two lists partition the noted set"
    assert set(rem.tolist()) == set(gone[1:].tolist())
    # without state: the same keys, values alone
    k2, v2, n1, n2, r2 = raw_export(log, t, 0, log.capacity, with_state=False)
    assert n1 is None and n2 is None and np.array_equal(np.sort(k2), np.sort(ups)) and np.array_equal(np.sort(r2), np.sort(rem))


# ---- the contract, end to end -------------------------------------------------------------------------------------------------------------------
def assert_exports_equal(a, b, what):
    ea, eb = export_sorted(a), export_sorted(b)
    assert len(ea) == len(eb)
    for name, x, z in zip(("keys", "values", "state1", "state2"), ea, eb):
        assert x.shape == z.shape and np.array_equal(bits(x), bits(z)), f"{what}: {name}"


def test_restore_from_base_and_deltas_equals_the_trained_table(dev, tmp_path):
    from meepoembedding_amd.nn import DynamicEmbedding, DynamicEmbeddingBag
    dim = 64
    A = LookupTable(1 << 13, dim, device=dev, optimizer=OPT_ADAGRAD, max_batch=4096, initial_accumulator=0.1, initializer=_lib.INIT_UNIFORM, init_scale=0.05,
                    init_seed=9, track_hits=True)
    pool = synth.keys_np(14, 0, 4000)
    A.insert(T(pool[:1500], dev), T(synth.rows_np(pool[:1500], dim, 2), dev))
    A.track_changes(1 << 13)
    bag = DynamicEmbeddingBag(A, mode="sum", optimizer="adagrad", lr=0.05, create_missing=True)
    emb = DynamicEmbedding(A, optimizer="adagrad", lr=0.05)
    rng = np.random.default_rng(1)

    def train(lo, hi, seed):
        k = T(pool[rng.integers(lo, hi, 600)], dev)
        off = T(np.arange(0, 601, 3, dtype=np.int64), dev)
        out = bag(k, off)
        out.backward(T(synth.rows_np(np.arange(out.shape[0], dtype=np.int64), dim, seed) * 0.1, dev))
        k2 = T(pool[rng.integers(lo, hi, 500)].reshape(50, 10), dev)
        rows = emb(k2)
        rows.backward(T(synth.rows_np(np.arange(500, dtype=np.int64), dim, seed + 1).reshape(50, 10, dim) * 0.1, dev))

    base, d1, d2 = (str(tmp_path / x) for x in ("base", "d1", "d2"))
    train(0, 1500, 20)                                       # changes in front of the base are the base's business
    assert checkpoint.save_base(A, base) == A.size() and A.change_log.size() == 0
    train(1000, 2500, 30)                                    # known and unseen ids
    A.remove(T(pool[rng.integers(0, 2500, 200)], dev))
    train(1200, 2600, 40)
    n1, r1 = checkpoint.save_delta(A, d1)
    assert n1 > 0 and r1 > 0 and A.change_log.size() == 0
    train(2000, 3500, 50)
    assert A.evict(0, 150, reset=False) == 150              # the hit counters are all 0: any 150 keys leave
    spilled = A.evict(0, 40, reset=False, spill=True)
    assert spilled[0].numel() == 40
    train(0, 4000, 60)
    n2, r2 = checkpoint.save_delta(A, d2)
    assert n2 > 0 and r2 > 0 and not A.change_log.invalid
    assert max(n1, n2) < A.size(), "a delta carries less than the table"
    B = LookupTable(3 << 12, dim, device=dev, optimizer=OPT_ADAGRAD, max_batch=1024)     # another capacity, another max_batch
    checkpoint.restore(B, base, [d1, d2])
    assert_exports_equal(A, B, "base + delta1 + delta2")
    with pytest.raises(ValueError, match="parent"):
        checkpoint.restore(LookupTable(64, dim, device=dev, optimizer=OPT_ADAGRAD, max_batch=64), base, [d2])
    # clear() is nothing a key set can name
    A.clear()
    assert A.change_log.invalid
    with pytest.raises(RuntimeError, match="invalid"):
        checkpoint.save_delta(A, str(tmp_path / "d3"))


# ---- groups -------------------------------------------------------------------------------------------------------------------------------------
def test_group_steps_note_every_member_in_its_own_log(dev, empty_table):
    from meepoembedding_amd.nn import DynamicEmbeddingBag, DynamicEmbeddingCollection
    dim, nt = 64, 3
    tables = [LookupTable(4096, dim, device=dev, optimizer=OPT_ADAGRAD, max_batch=4096, initial_accumulator=0.1, initializer=_lib.INIT_UNIFORM, init_scale=0.05,
                          init_seed=j) for j in range(nt)]
    g = TableGroup(tables, max_apply_batch=4096)
    logs = g.track_changes([2048, 1024, 2048])
    assert [t.change_log for t in tables] == logs
    member_keys = [synth.keys_np(20 + j, 0, 400) for j in range(nt)]       # disjoint key sets: a key in the wrong log would show
    outside = synth.keys_np(30, 0, 5)
    rng = np.random.default_rng(2)
    want = [set() for _ in range(nt)]
    # the collection: positions in front of offsets[0] and behind offsets[nt] belong to no member
    segs = [member_keys[j][rng.integers(0, 400, n)] for j, n in enumerate((130, 0 + 77, 201))]
    keys = np.concatenate([outside[:2], *segs, outside[2:]])
    offsets = np.cumsum([2] + [s.size for s in segs]).astype(np.int64)
    coll = DynamicEmbeddingCollection(g, optimizer="adagrad", lr=0.05)
    rows = coll(T(keys, dev), T(offsets, dev))
    rows.backward(torch.ones_like(rows))
    for j in range(nt):
        want[j] |= set(segs[j].tolist())
    # the bag layer: 3 members x 20 bags
    bags = [member_keys[j][rng.integers(200, 400, 60)] for j in range(nt)]
    bag_offsets = np.arange(0, 181, 3, dtype=np.int64)
    layer = DynamicEmbeddingBag(g, mode="sum", optimizer="adagrad", lr=0.05, create_missing=True)
    out = layer(T(np.concatenate(bags), dev), T(bag_offsets, dev))
    out.backward(torch.ones_like(out))
    for j in range(nt):
        want[j] |= set(bags[j].tolist())
    for j in range(nt):
        assert not logs[j].invalid
        k, _, _, _, r = raw_export(logs[j], tables[j], 0, logs[j].capacity, with_state=False)
        assert r.size == 0 and set(k.tolist()) == want[j] and k.size == len(want[j]) == logs[j].size(), f"member {j}"
    # a member's own mutator notes in the same object
    tables[1].remove(T(member_keys[1][:7], dev))
    assert set(noted(logs[1], tables[1]).tolist()) == want[1] | set(member_keys[1][:7].tolist())


# ---- capture ------------------------------------------------------------------------------------------------------------------------------------
def test_note_under_stream_capture(dev, empty_table):
    log = ChangeLog(1024, dev)
    first, second = synth.keys_np(40, 0, 203), synth.keys_np(41, 0, 203)
    buf = T(first, dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        log.note(buf)
    graph.replay()
    buf.copy_(T(second, dev))
    graph.replay()
    torch.cuda.synchronize(dev)
    assert log.size() == 406 and not log.invalid
    assert np.array_equal(noted(log, empty_table), np.sort(np.concatenate([first, second])))
