"""Native eviction (SPEC.md §3 evict): mee_evict by threshold or least-hit with the evicted rows handed out, the counters by key (mee_hits_find /
mee_hits_assign / mee_hits_decay), LookupTable.evict / hits_of / set_hits / hits_decay and evict_cold of the hot/cold pair and the collection of pairs.

The oracle has no counters and no evict.  The reference everywhere is the oracle table built by the same calls as the table under test and then
mirrored with remove(evicted keys), plus numpy on the counters the test itself placed.  Everything is compared bit for bit: keys, rows, every state
plane, counters, sizes, status words.  Every table takes one optimizer step with key-derived gradients first, so acc, m and v differ per key."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import oracle
from _apply_cases import T, assert_tables_bit_equal, export_sorted
from _cpu_backend import CpuTable
from meepoembedding_amd import OPT_ADAGRAD, OPT_ADAM, OPT_NONE, LookupTable, MeepoError, _lib, synth
from meepoembedding_amd.tiered import TieredLookupTable, TieredTableGroup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM, PINNED = _lib.MEM_HBM, _lib.MEM_HOST_PINNED
ALL = 0xFFFFFFFF
NEW_SYMBOLS = ("mee_evict", "mee_hits_find", "mee_hits_assign", "mee_hits_decay")
OPTS = {"none": (OPT_NONE, oracle.OPT_NONE), "adagrad": (OPT_ADAGRAD, oracle.OPT_ADAGRAD), "adam": (OPT_ADAM, oracle.OPT_ADAM)}
# counters on both sides of every digit boundary of the selection (10 + 11 + 11 bits from the top: 2^11 and 2^22; an 8-bit split would cut at 2^8,
# 2^16 and 2^24), the extremes, and values that differ in the top bit only
VALUES = np.array([0, 1, 2, 255, 256, 257, 2047, 2048, 65535, 65536, (1 << 22) - 1, 1 << 22, (1 << 24) - 1, 1 << 24, 1 << 31, (1 << 32) - 1], dtype=np.uint32)


# ---- CPU: the interface exists (these fail on the parent) ----------------------------------------------------------------------------------
def test_symbols_declared_bound_and_exported(built):
    src = open(os.path.join(ROOT, "include", "meepo_embedding.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    L = C.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(rf"\bint {name}\s*\(", src), f"{name} is not declared in the header"
        assert name in _lib.PROTOTYPES and hasattr(L, name), name
        decl = re.search(rf"\bint {name}\s*\((.*?)\)\s*;", src, flags=re.S).group(1)
        assert len(_lib.PROTOTYPES[name][1]) == decl.count(",") + 1, f"{name}: bound with another number of arguments than declared"
    assert re.search(r"MEE_EVICT_LEAST\s*=\s*1u?\b", src) and re.search(r"MEE_EVICT_RESET\s*=\s*2u?\b", src)
    assert (_lib.EVICT_LEAST, _lib.EVICT_RESET) == (1, 2)
    assert "MEE_ABI_VERSION 2" in src and _lib.lib().mee_abi_version() == _lib.ABI_VERSION == 2
    hpp = open(os.path.join(ROOT, "include", "meepo_embedding.hpp")).read()
    for name in NEW_SYMBOLS:
        assert name + "(t_" in hpp, f"{name} has no wrapper in the C++ layer"


def test_null_tables_are_refused(built):
    L = _lib.lib()
    assert L.mee_evict(None, 0, 0, 0, None, None, None, None, None, 0, None, None) == _lib.ERR_INVALID_ARG
    assert L.mee_last_error().startswith(b"mee_evict:")
    for name, args in (("mee_hits_find", (None, None, 0, None, None)), ("mee_hits_assign", (None, None, 0, None, None)), ("mee_hits_decay", (None, 1, None))):
        assert getattr(L, name)(*args) == _lib.ERR_INVALID_ARG
        assert L.mee_last_error().startswith(name.encode() + b":")


def test_wrappers_reject_bad_arguments_before_any_launch(built, monkeypatch):
    from meepoembedding_amd import table as tm
    calls = []

    class Recorder:   # stands in for the library: records what would have been launched
        def __getattr__(self, name):
            calls.append(name)
            return lambda *a: 0

    monkeypatch.setattr(tm._lib, "lib", lambda: Recorder())
    monkeypatch.setattr(tm, "_stream_ptr", lambda device: 0)
    t = LookupTable.__new__(LookupTable)
    t._h, t.device, t.dim, t.capacity, t.optimizer, t.layout_epoch = None, torch.device("cpu"), 8, 64, OPT_NONE, 0
    keys = torch.arange(6, dtype=torch.int64)
    good = torch.zeros(6, dtype=torch.uint32)
    for kw in (dict(limit=-1), dict(max_hits=-1), dict(limit=-5, least=True, spill=True)):
        with pytest.raises(ValueError):
            t.evict(**kw)
    with pytest.raises(ValueError):
        t.hits_decay(-1)
    for bad in (torch.zeros(5, dtype=torch.uint32), torch.zeros(7, dtype=torch.uint32), torch.zeros(6, dtype=torch.int64), torch.zeros(6, dtype=torch.float32),
                torch.zeros(12, dtype=torch.uint32)[::2], torch.zeros(6, dtype=torch.uint32, device="meta")):
        with pytest.raises(MeepoError):
            t.set_hits(keys, bad)
    for bad in (keys.to(torch.int32), keys.to(torch.float32), keys.to("meta")):
        with pytest.raises(MeepoError):
            t.hits_of(bad)
        with pytest.raises(MeepoError):
            t.set_hits(bad, good)
    assert calls == [], f"refused calls reached the library: {calls}"
    t.set_hits(keys, good); t.set_hits(keys, good.view(torch.int32)); t.hits_of(keys); t.hits_decay(40)   # well-formed calls do
    assert calls == ["mee_hits_assign", "mee_hits_assign", "mee_hits_find", "mee_hits_decay"]


class EvictingCpuTable(CpuTable):
    """CpuTable with LookupTable.evict, from its `hits` dict: what evict_cold needs of a cold tier"""

    def evict(self, max_hits=0, limit=1 << 20, reset=True, *, least=False, spill=False, with_state=True):
        k, v, a, b = self.o.export(with_state=True)
        h = np.array([self.hits.get(int(x), 0) for x in k], dtype=np.int64)
        cand = np.flatnonzero(h <= max_hits)
        if least:
            cand = cand[np.argsort(h[cand], kind="stable")]
        e = cand[:limit]
        self.o.remove(k[e])
        left = set(k[e].tolist())
        self.hits = {} if reset else {x: c for x, c in self.hits.items() if x not in left}
        if not spill:
            return int(e.size)
        tt = lambda x: None if x is None else torch.from_numpy(x[e].copy())
        return tt(k), tt(v), tt(a) if with_state else None, tt(b) if with_state else None, torch.from_numpy(h[e].astype(np.uint32))


def _cpu_pair(seed, track=True):
    hot = EvictingCpuTable(256, 8, optimizer=oracle.OPT_ADAGRAD, initial_accumulator=0.1, track_hits=track)
    cold = EvictingCpuTable(1024, 8, optimizer=oracle.OPT_ADAGRAD, initial_accumulator=0.1, track_hits=track)
    pair = TieredLookupTable(hot, cold, hot_key_limit=100)
    keys = synth.keys_np(seed, 0, 400)
    pair.insert(torch.from_numpy(keys[:100]), torch.from_numpy(synth.rows_np(keys[:100], 8, 2)))      # fills the hot tier ...
    pair.insert(torch.from_numpy(keys[100:]), torch.from_numpy(synth.rows_np(keys[100:], 8, 2)))      # ... the rest goes cold
    pair.apply_adagrad(torch.from_numpy(keys), torch.from_numpy((synth.rows_np(keys, 8, 6) * 0.02).astype(np.float32)), lr=0.05)
    assert hot.size() == 100 and cold.size() == 300
    if track:
        for r in range(1, 4):   # cold keys 100..174 are never found, the next 75 once, then twice, then three times
            pair.find(torch.from_numpy(keys[100 + 75 * r:]))
    return pair, keys


def test_evict_cold_over_cpu_tables():
    pair, keys = _cpu_pair(31)
    hot_before = [x.clone() for x in pair.hot.export(with_state=True) if x is not None]
    ck, cv, ca = (x.numpy() for x in pair.cold.export(with_state=True)[:3])
    order = np.argsort(ck)
    ek, ev, ea, eb, eh = pair.evict_cold(100, spill=True)
    assert eb is None and ek.numel() == 100 and pair.cold.size() == 200 and pair.hot.size() == 100
    ek = ek.numpy()
    assert set(ek[eh.numpy() == 0].tolist()) == set(keys[100:175].tolist()), "every never-hit cold key goes first"
    assert np.array_equal(np.sort(eh.numpy()), np.repeat([0, 1], [75, 25])) and set(ek.tolist()) <= set(keys[175:250].tolist()) | set(keys[100:175].tolist())
    at = order[np.searchsorted(ck[order], ek)]
    assert np.array_equal(ck[at], ek) and np.array_equal(cv[at], ev.numpy()) and np.array_equal(ca[at], ea.numpy()), "the spilled rows are the cold rows"
    assert not bool(pair.find(torch.from_numpy(ek))[1].any()) and bool(pair.find(torch.from_numpy(keys[:100]))[1].all())
    for a, b in zip(hot_before, [x for x in pair.hot.export(with_state=True) if x is not None]):
        assert torch.equal(a, b), "hot keys are untouched"
    assert pair.cold.hits[int(keys[399])] == 3, "evict_cold keeps the counters of the keys that stay"
    assert pair.evict_cold(50) == 50 and pair.cold.size() == 150
    # the collection of pairs: the per-pair loop
    pairs = [_cpu_pair(32)[0], _cpu_pair(33)[0]]
    grp = TieredTableGroup(pairs)
    assert grp.evict_cold(40) == [40, 40] and [p.cold.size() for p in pairs] == [260, 260] and [p.hot.size() for p in pairs] == [100, 100]
    spilled = grp.evict_cold(10, spill=True)
    assert [s[0].numel() for s in spilled] == [10, 10] and all(bool((s[4] == 0).all()) for s in spilled)
    # a cold tier without counters has nothing to evict by
    with pytest.raises(RuntimeError):
        _cpu_pair(34, track=False)[0].evict_cold(10)
    with pytest.raises(RuntimeError):
        TieredTableGroup([_cpu_pair(35, track=False)[0]]).evict_cold(10)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------------
def _np(x):
    return x.cpu().numpy()


def make(dev, opt, dim, keys, slots=4096, mem=HBM, max_batch=4096):
    """the table under test and its oracle mirror: the same inserts, one optimizer step with key-derived gradients"""
    kind, okind = OPTS[opt]
    t = LookupTable(slots, dim, device=dev, optimizer=kind, max_batch=max_batch, value_memory=mem, track_hits=True, initial_accumulator=0.1)
    o = oracle.OracleTable(2 * slots, dim, optimizer=okind, initial_accumulator=0.1)
    rows = synth.rows_np(keys, dim, 2)
    g = (synth.rows_np(keys, dim, 6) * 0.02).astype(np.float32)
    for s in range(0, keys.size, max_batch):
        k, r, gg = keys[s:s + max_batch], rows[s:s + max_batch], g[s:s + max_batch]
        t.insert(T(k, dev), T(r, dev)); o.insert(k, r)
        if opt == "adagrad":
            t.apply_adagrad(T(k, dev), T(gg, dev), lr=0.05); o.apply_adagrad(k, gg, 0.05, 1e-10)
        elif opt == "adam":
            t.apply_adam(T(k, dev), T(gg, dev), lr=0.01, step=3); o.apply_adam(k, gg, 0.01, 0.9, 0.999, 1e-8, 3)
    assert t.status() == 0 and t.size() == o.size() == keys.size
    return t, o


def evict_checked(t, o, keys, dev, max_hits, limit, least, reset, what=""):
    """t.evict(..., spill=True) held to the definition; `keys`: every key the table may hold (a superset is fine).  Mirrors the oracle.  -> evicted keys"""
    kt = T(keys, dev)
    stored = _np(t.locate(kt)[1]) != 0
    hb = _np(t.hits_of(kt))
    assert not hb[~stored].any(), f"{what}: hits_of of an absent key"
    pre = export_sorted(t)
    assert_tables_bit_equal(t, o, what + " (before)")
    size0, status0 = t.size(), t.status()
    ek, ev, e1, e2, eh = t.evict(max_hits, limit, reset, least=least, spill=True)
    assert (e1 is None) == (t.optimizer == OPT_NONE) and (e2 is None) == (t.optimizer != OPT_ADAM), what
    ek, eh = _np(ek), _np(eh)
    cand = stored & (hb <= max_hits)
    m = min(int(cand.sum()), limit)
    print(f"{what}: |C| = {int(cand.sum())}, limit = {limit}, evicted {ek.size}")
    assert ek.size == eh.size == m and np.unique(ek).size == m, f"{what}: |E| = {ek.size}, min(|C|, limit) = {m}"
    assert np.isin(ek, keys[cand]).all(), f"{what}: E is no subset of C"
    # what was handed out is what the table held: rows and state against the export taken before the call, counters against hits_of
    at = np.searchsorted(pre[0], ek)
    assert np.array_equal(pre[0][at], ek), what
    for name, got, plane in zip(("values", "state1", "state2"), (ev, e1, e2), pre[1:] + [None, None]):
        if got is not None:
            assert np.array_equal(_np(got).view(np.uint32), plane[at].view(np.uint32)), f"{what}: spilled {name}"
    pos = {int(k): i for i, k in enumerate(keys)}
    idx = np.array([pos[int(k)] for k in ek], dtype=np.int64)
    assert np.array_equal(eh, hb[idx]), f"{what}: spilled counters"
    if least and m:
        want = np.sort(hb[cand])[:m]
        assert np.array_equal(np.sort(eh), want), f"{what}: the evicted counters are not the {m} smallest of C"
        cut = want[-1]
        gone = np.zeros(keys.size, dtype=bool); gone[idx] = True
        assert gone[cand & (hb < cut)].all(), f"{what}: a candidate under the cut value {cut} stayed"
        assert not gone[cand & (hb > cut)].any(), f"{what}: a candidate above the cut value {cut} left"
    # the table afterwards: the oracle after remove(E)
    if m:
        assert o.remove(ek).all()
    assert_tables_bit_equal(t, o, what + " (after)")
    assert t.size() == o.size() == size0 - m and t.status() == status0, what
    after = _np(t.locate(kt)[1]) != 0
    gone = np.zeros(keys.size, dtype=bool); gone[idx] = True
    assert np.array_equal(after, stored & ~gone), f"{what}: found mask"
    ha = _np(t.hits_of(kt))
    assert np.array_equal(ha, np.where(after & (not reset), hb, 0).astype(np.uint32)), f"{what}: counters of the keys that stay"
    return ek


@pytest.mark.gpu
@pytest.mark.parametrize("opt", ["none", "adagrad", "adam"])
@pytest.mark.parametrize("dim", [16, 128])
def test_threshold_form_gpu(dev, dim, opt):
    keys = synth.keys_np(50 + dim, 0, 2000)
    t, o = make(dev, opt, dim, keys)
    for lo in (500, 1000, 1500):   # 500 keys each at 0, 1, 2 and 3 hits
        t.find_counted(T(keys[lo:], dev))
    assert np.array_equal(_np(t.hits_of(T(keys, dev))), np.repeat([0, 1, 2, 3], 500).astype(np.uint32))
    probe = np.concatenate([keys, synth.keys_np(7, 5000, 100)])
    first = evict_checked(t, o, probe, dev, max_hits=1, limit=300, least=False, reset=False, what="binding limit")     # 300 of the 1000 at or under 1
    rest = evict_checked(t, o, probe, dev, max_hits=1, limit=1 << 20, least=False, reset=True, what="no limit, reset")  # the other 700; counters zeroed
    assert first.size == 300 and rest.size == 700 and t.size() == 1000
    assert np.array_equal(np.sort(np.concatenate([first, rest])), np.sort(keys[:1000]))
    assert t.hits_scan(1, ALL, 10).numel() == 0
    # without spill the count alone comes back, and nothing is left at or under the threshold but what a new window counts
    assert t.evict(max_hits=0, limit=10, reset=False) == 10 and t.size() == 990


def _placed(dev, opt="adagrad", dim=16, mem=HBM, seed=77):
    """2000 keys whose counters are VALUES in turn (125 keys per value), in a shuffled order"""
    keys = synth.keys_np(seed, 0, 2000)
    t, o = make(dev, opt, dim, keys, mem=mem)
    hits = VALUES[np.random.default_rng(seed).permutation(2000) % VALUES.size]
    t.set_hits(T(keys, dev), T(hits, dev))
    assert np.array_equal(_np(t.hits_of(T(keys, dev))), hits)
    return t, o, keys, hits


LEAST_CASES = {   # name -> (max_hits, n): 125 keys per value of VALUES
    "between_two_values": (ALL, 3 * 125),              # the cut falls between 2 and 255
    "inside_a_tied_class": (ALL, 4 * 125 + 60),        # 60 of the 125 keys at 256
    "inside_class_2048": (ALL, 7 * 125 + 1),           # one key of the first class behind the low digit's boundary
    "inside_class_2_22": (ALL, 11 * 125 + 124),        # all but one key at 2^22, the first class behind the middle digit's boundary
    "inside_top_bit_class": (ALL, 14 * 125 + 17),      # 17 keys at 2^31
    "inside_the_largest": (ALL, 15 * 125 + 100),       # 100 keys at 2^32 - 1
    "n_is_zero": (ALL, 0),
    "n_beyond_size": (ALL, 5000),
    "max_hits_binds_first": (65535, 1900),             # |C| = 9 * 125 < n
    "max_hits_inside_and_tie": (2047, 6 * 125 + 5),    # C ends at 2047, the cut takes 5 of its keys
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(LEAST_CASES))
def test_least_form_gpu(dev, case):
    max_hits, n = LEAST_CASES[case]
    t, o, keys, hits = _placed(dev)
    probe = np.concatenate([keys, synth.keys_np(7, 5000, 64)])
    reset = case in ("inside_a_tied_class", "n_is_zero")   # n = 0 still starts a new window
    ek = evict_checked(t, o, probe, dev, max_hits=max_hits, limit=n, least=True, reset=reset, what=case)
    assert ek.size == min(int((hits <= max_hits).sum()), n)
    if case == "n_beyond_size":
        assert t.size() == 0 and t.export()[0].numel() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("least", [False, True])
def test_only_stored_keys_are_candidates_gpu(dev, least):
    keys = synth.keys_np(91, 0, 2000)
    t, o = make(dev, "adagrad", 16, keys)
    t.find_counted(T(keys[:800], dev))
    removed = keys[100:600]                       # tombstones whose counter words still hold 1, and tombstones at 0
    assert bool(t.remove(T(removed, dev)).all()) and o.remove(removed).all()
    ek = evict_checked(t, o, keys, dev, max_hits=ALL, limit=1 << 40, least=least, reset=False, what="everything")
    assert ek.size == 1500 and not np.isin(ek, removed).any() and t.size() == 0
    again = t.evict(ALL, 1 << 40, least=least, spill=True)   # an empty table: nothing is written, the count is 0
    assert again[0].numel() == 0 and again[4].numel() == 0 and t.evict(ALL, 100, least=least) == 0 and t.size() == 0


@pytest.mark.gpu
def test_extent_gpu(dev):
    """~300K slots of dim 4 (a wave of the scans takes more than one span and the last one is partial), and a table of two buckets"""
    keys = synth.keys_np(93, 0, 200_000)
    t, o = make(dev, "none", 4, keys, slots=300_000, max_batch=1 << 18)
    assert t.capacity % 1024 != 0 and t.capacity > 2 * 4 * 1024 * 4
    rng = np.random.default_rng(93)
    hits = np.where(rng.random(keys.size) < 0.9, rng.integers(0, 4, keys.size), rng.integers(0, 1 << 32, keys.size)).astype(np.uint32)   # nearly all tiny
    for s in range(0, keys.size, 1 << 18):
        t.set_hits(T(keys[s:s + (1 << 18)], dev), T(hits[s:s + (1 << 18)], dev))
    small = LookupTable(20, 4, device=dev, max_batch=64, track_hits=True)
    assert small.n_buckets == 2 and small.capacity == 32
    # (evict_checked probes with batches of at most max_batch keys: the big table in pieces)
    kt = [T(keys[s:s + (1 << 18)], dev) for s in range(0, keys.size, 1 << 18)]
    pre = export_sorted(t)
    ek, ev, _, _, eh = t.evict(ALL, 100_000, reset=False, least=True, spill=True)
    ek, eh, ev = _np(ek), _np(eh), _np(ev)
    assert ek.size == 100_000 and np.unique(ek).size == 100_000
    want = np.sort(hits)[:100_000]
    assert np.array_equal(np.sort(eh), want)
    srt = np.argsort(keys)
    idx = srt[np.searchsorted(keys[srt], ek)]
    assert np.array_equal(keys[idx], ek) and np.array_equal(hits[idx], eh)
    gone = np.zeros(keys.size, dtype=bool); gone[idx] = True
    assert gone[hits < want[-1]].all() and not gone[hits > want[-1]].any()
    at = np.searchsorted(pre[0], ek)
    assert np.array_equal(pre[0][at], ek) and np.array_equal(pre[1][at].view(np.uint32), ev.view(np.uint32))
    assert o.remove(ek).all()
    assert_tables_bit_equal(t, o, "300K slots")
    assert t.size() == 100_000 and t.status() == 0
    ha = np.concatenate([_np(t.hits_of(k)) for k in kt])
    assert np.array_equal(ha, np.where(gone, 0, hits).astype(np.uint32))
    # two buckets
    k2 = synth.keys_np(94, 0, 20)
    o2 = oracle.OracleTable(64, 4)
    small.insert(T(k2, dev), T(synth.rows_np(k2, 4, 2), dev)); o2.insert(k2, synth.rows_np(k2, 4, 2))
    small.set_hits(T(k2, dev), T(np.arange(20, dtype=np.uint32) * 3, dev))
    e2 = evict_checked(small, o2, k2, dev, max_hits=ALL, limit=10, least=True, reset=False, what="two buckets")
    assert np.array_equal(np.sort(e2), np.sort(k2[:10]))


@pytest.mark.gpu
def test_pinned_host_gpu(dev):
    t, o, keys, hits = _placed(dev, "adagrad", 16, mem=PINNED, seed=95)
    evict_checked(t, o, keys, dev, max_hits=ALL, limit=6 * 125 + 33, least=True, reset=False, what="pinned host, least")
    evict_checked(t, o, keys, dev, max_hits=65536, limit=1 << 20, least=False, reset=True, what="pinned host, threshold")


@pytest.mark.gpu
def test_room_after_table_full_gpu(dev):
    """a full table drops keys; evicting the n least-hit ones makes room for n new keys, in the tombstones"""
    t = LookupTable(256, 8, device=dev, optimizer=OPT_ADAGRAD, max_batch=1024, track_hits=True, initial_accumulator=0.1)
    keys = synth.keys_np(96, 0, 1000)
    t.find_or_insert(T(keys[:400], dev))
    assert t.status() & _lib.STATUS_TABLE_FULL
    full = t.size()
    assert full > t.capacity - 16, "a key is dropped only once its whole probe sequence is taken"
    held = keys[:400][_np(t.locate(T(keys[:400], dev))[1]) != 0]
    t.find_counted(T(held[50:], dev))
    n = 50
    ek = _np(t.evict(ALL, n, reset=False, least=True, spill=True)[0])
    assert np.array_equal(np.sort(ek), np.sort(held[:50])) and t.size() == full - n
    t.clear_status()
    _, found = t.find_or_insert(T(keys[500:500 + n], dev))
    assert not bool(found.any()) and t.status() == 0 and t.size() == full          # every new key found room: size is back where it was
    assert bool(t.locate(T(keys[500:500 + n], dev))[1].all()) and bool(t.locate(T(held[50:], dev))[1].all())
    assert not _np(t.hits_of(T(keys[500:500 + n], dev))).any(), "a reused slot starts a new window"


def _same_bits(a, b, what):
    for x, y in zip(export_sorted(a), export_sorted(b)):
        assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y), what


@pytest.mark.gpu
def test_handles_taken_before_an_evict_are_stale_gpu(dev):
    """Host side as mee_remove (SPEC.md §3): the evict bumps the layout epoch, so handles of before it are ignored by the located apply — no row
    is updated through them, MEE_STATUS_STALE_HANDLE is raised — and handles taken after it serve the step as an apply by keys does."""
    keys = synth.keys_np(97, 0, 2000)
    tabs = []
    for _ in range(2):
        t, _o = make(dev, "adagrad", 16, keys)
        t.find_counted(T(keys[700:], dev))
        tabs.append(t)
    a, b = tabs
    batch = T(keys[300:1200], dev)                     # evicted keys and keys that stay
    g = T((synth.rows_np(keys[300:1200], 16, 8) * 0.02).astype(np.float32), dev)
    _, _, old = a.find_located(batch)
    epoch = a.layout_epoch
    for t in tabs:
        assert t.evict(0, 1 << 20, reset=False) == 700
    assert a.layout_epoch != epoch
    a.apply_adagrad(batch, g, lr=0.05, slots=old)      # the handles name slots of before the evict: they must not be trusted
    assert a.status() == _lib.STATUS_STALE_HANDLE
    a.clear_status()
    _same_bits(a, b, "stale handles update nothing")
    _, found, new = a.find_located(batch)
    assert np.array_equal(_np(found), np.repeat([0, 1], [400, 500]).astype(np.uint8)) and bool((new[:400] == -1).all())
    a.apply_adagrad(batch, g, lr=0.05, slots=new)
    b.apply_adagrad(batch, g, lr=0.05)
    _same_bits(a, b, "handles taken after the evict == the apply by keys")
    assert a.size() == 1300 and a.status() == b.status() == 0


@pytest.mark.gpu
def test_capture_gpu(dev):
    """one mee_evict (least, spill, the count on the device) captured on one stream and replayed once == the eager call on a twin"""
    (t, o, keys, hits), (twin, _o, _k, _h) = _placed(dev, "adam", 16, seed=98), _placed(dev, "adam", 16, seed=98)
    n, cap = 9 * 125, 1200                               # the cut falls between 65535 and 65536: E is determined
    bufs = [torch.zeros(cap, dtype=torch.int64, device=dev)] + [torch.zeros((cap, 16), dtype=torch.float32, device=dev) for _ in range(3)] + \
           [torch.zeros(cap, dtype=torch.int32, device=dev).view(torch.uint32)]
    n_out = torch.full((1,), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _lib.check(_lib.lib().mee_evict(t._h, ALL, n, _lib.EVICT_LEAST, *[b.data_ptr() for b in bufs], cap, n_out.data_ptr(), t._s()))
    torch.cuda.synchronize(dev)
    assert t.size() == 2000 and int(n_out.item()) == -1, "capturing runs nothing"
    graph.replay()
    torch.cuda.synchronize(dev)
    want = twin.evict(ALL, n, reset=False, least=True, spill=True)
    assert int(n_out.item()) == n == want[0].numel()
    order, worder = np.argsort(_np(bufs[0][:n])), np.argsort(_np(want[0]))
    assert np.array_equal(np.sort(_np(want[0])), np.sort(keys[hits <= 65535]))
    for got, ref in zip(bufs, want):
        x, y = _np(got[:n])[order], _np(ref)[worder]
        assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
    assert not any(_np(b[n:]).any() for b in bufs), "positions behind the count stay untouched"
    for x, y in zip(export_sorted(t), export_sorted(twin)):
        assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
    kt = T(keys, dev)
    assert np.array_equal(_np(t.hits_of(kt)), _np(twin.hits_of(kt))) and t.size() == twin.size() == 2000 - n and t.status() == twin.status() == 0
    o.remove(_np(want[0]))
    assert_tables_bit_equal(t, o, "replayed")


@pytest.mark.gpu
def test_small_operators_gpu(dev):
    t, _o, keys, hits = _placed(dev, "none", 16, seed=99)
    absent = synth.keys_np(7, 9000, 50)
    probe = np.concatenate([absent[:25], [_lib.EMPTY_KEY, _lib.RECLAIMED_KEY], keys[:100], absent[25:]]).astype(np.int64)
    want = np.concatenate([np.zeros(27, np.uint32), hits[:100], np.zeros(25, np.uint32)])
    assert np.array_equal(_np(t.hits_of(T(probe, dev))), want)
    assert t.hits_of(T(probe[:0], dev)).numel() == 0
    # set_hits ignores absent and reserved keys (no key appears, no status bit), and round-trips on the present ones
    new = np.random.default_rng(5).integers(0, 1 << 32, probe.size).astype(np.uint32)
    t.set_hits(T(probe, dev), T(new, dev))
    assert t.size() == 2000 and t.status() == 0 and not bool(t.locate(T(absent, dev))[1].any())
    hits = hits.copy(); hits[:100] = new[27:127]
    assert np.array_equal(_np(t.hits_of(T(keys, dev))), hits)
    assert np.array_equal(_np(t.hits_of(T(probe, dev))), np.concatenate([np.zeros(27, np.uint32), new[27:127], np.zeros(25, np.uint32)]))
    t.set_hits(T(keys, dev), T(hits.view(np.int32), dev))           # int32 tensors carry the same bits
    assert np.array_equal(_np(t.hits_of(T(keys, dev))), hits)
    for shift in (1, 31, 40):
        t.set_hits(T(keys, dev), T(hits, dev))
        t.hits_decay(shift)
        ref = (hits.astype(np.uint64) >> np.uint64(min(shift, 63))).astype(np.uint32)
        assert np.array_equal(_np(t.hits_of(T(keys, dev))), ref), f"hits_decay({shift})"
    # the counters are what the counting lookups feed: find_counted adds one on top of a placed value
    t.set_hits(T(keys[:10], dev), T(np.full(10, 41, np.uint32), dev))
    t.find_counted(T(keys[:5], dev))
    assert _np(t.hits_of(T(keys[:10], dev))).tolist() == [42] * 5 + [41] * 5
    # refusals of the library itself: a table without counters, a batch beyond max_batch, unknown flag bits
    plain = LookupTable(256, 16, device=dev, max_batch=64)
    for call in (lambda: plain.evict(), lambda: plain.hits_of(T(keys[:4], dev)), lambda: plain.set_hits(T(keys[:4], dev), T(hits[:4], dev)), lambda: plain.hits_decay(1)):
        with pytest.raises(MeepoError) as e:
            call()
        assert e.value.code == _lib.ERR_UNSUPPORTED
    small = LookupTable(256, 16, device=dev, max_batch=64, track_hits=True)
    with pytest.raises(MeepoError) as e:
        small.hits_of(T(keys[:65], dev))
    assert e.value.code == _lib.ERR_BATCH_TOO_LARGE
    assert _lib.lib().mee_evict(small._h, 0, 1, 4, None, None, None, None, None, 0, None, None) == _lib.ERR_INVALID_ARG
    assert small.evict(ALL, 0) == 0
