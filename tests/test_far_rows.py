"""Every operator on rows that lie past the 4 GiB and the 2^32-element marks of a plane.

The row kernels address a stored row as plane[slot * dim4 + column] in 16-byte groups.  Arithmetic that is narrowed to 32 bits anywhere on the
way — a byte offset, an fp32 element index, a bf16 element index — does nothing wrong until a plane grows past 2^31 / 2^32 bytes or 2^31 / 2^32
elements.  A table does not have to be FULL to have such rows: with a large capacity and a few thousand keys the hash spreads the keys over the
whole plane (the planes are allocated, never cleared), so a sparse 18 GB table and a 16K-key batch cost milliseconds.

far_table() builds such a table — the last ~8 % of its slots beyond the wall — next to a small C-oracle twin with the same options, and picks its
keys BEFORE inserting: the home bucket of every key of a 1M-key pool is hashed, far keys are those whose home bucket starts at or behind the wall's
first slot, near keys those whose bucket ends below 2^31 bytes.  After the insert locate() PROVES it (>= 512 keys beyond the wall, >= 512 below
2^31 bytes: a hard assert); the CPU test at the top checks with the oracle's hash that every parametrised (shape, wall) pair has the candidates.
Rows are key-derived (synth.rows_*), so a read that wraps to a near slot returns another key's row or uninitialised memory, never the right one, and
a write that wraps shows as a lost update of the far key or as a corrupted near row.  Every test compares, bit for bit and keyed by key: the far
keys' observables, the near keys, size(), status() and the key-sorted export (state planes included) against the twin.

Walls (first slot behind them): fp32 rows — bytes 2^32 / (4·dim), elements 2^32 / dim; bf16 rows — bytes 2^32 / (2·dim), elements 2^32 / dim.
Row shapes: dim 64, dim 128 and dim 1024 (the run-time-width instance), the three with_row_shape distinguishes.  The element-wall tables also lie
past the byte wall.  Adam tables (three planes) get the element wall at dim 1024 only.  Section 3 tests the CALLER's buffers past the same walls
(position × dim4, bag × dim4) on a small table.

Out of scope: host-pinned cold tiers (multi-GB pinned allocations on a shared host); the sharded and peer paths (their local shards run these same
kernels, their own buffers are batch-sized); the hits plane and the sketch planes (4 B per slot: no wall at these capacities); the 2^31-float4
wall (a 32 GiB plane), which stays with test_full_size_configs_properties.

A test skips only when torch.cuda.mem_get_info shows less than its own need plus 8 GiB; the message states the need."""
import contextlib
import types

import numpy as np
import pytest
import torch

import oracle
from _apply_cases import T, assert_tables_bit_equal, exact_grads_dev, export_sorted
from meepoembedding_amd import INIT_UNIFORM, OPT_ADAGRAD, OPT_ADAM, OPT_NONE, LookupTable, MixedTableGroup, TableGroup, _lib, hash_batch, synth
from test_weighted_bags import bag_of_positions, weight_grads_ref, weighted_pool

assert (OPT_NONE, OPT_ADAGRAD, OPT_ADAM, INIT_UNIFORM) == (oracle.OPT_NONE, oracle.OPT_ADAGRAD, oracle.OPT_ADAM, oracle.INIT_UNIFORM)

BF16 = torch.bfloat16
POOL_SEED, POOL = 9001, 1 << 20      # the key pool the near / far keys are chosen from
N_KEYS = 2048                        # near keys and far keys stored in every far table, each
N_FRESH = 1024                       # further far-home keys, not stored: what find_or_insert creates
MAX_BATCH = 1 << 14                  # the workspace grows with max_batch × dim
SLOT_MASK = (1 << 40) - 1            # a located handle = layout tag << 40 | slot
GIB = 1 << 30
SHAPES = (64, 128, 1024)
CASES = [(d, w) for w in ("byte", "elem") for d in SHAPES]                       # tables of one or two planes
CASES_3 = [(d, "byte") for d in SHAPES] + [(1024, "elem")]                         # three planes (Adam): the element wall on one shape only
IDS = lambda c: f"{c[0]}-{c[1]}"
OPT_CASES = [("adagrad",) + c for c in CASES] + [("adam",) + c for c in CASES_3]


# ---- the geometry: where the wall is, how large the table must be, which keys are far ----------------------------------------------------
def row_bytes(dim, bf16=False):
    return dim * (2 if bf16 else 4)


def wall_slot(dim, wall, bf16=False):
    """the first slot whose row starts at or behind the wall"""
    return (1 << 32) // (row_bytes(dim, bf16) if wall == "byte" else dim)


def capacity_for(dim, wall, bf16=False):
    """requested slots: ~8 % of the table lies beyond the wall (dim 1024, element wall: 4.57M slots, 18.7 GB per fp32 plane)"""
    return int(wall_slot(dim, wall, bf16) * 1.09)


def n_buckets_for(capacity):
    """SPEC.md §2: the smallest prime >= ceil(capacity / 16)"""
    return int(oracle.lib().meo_next_prime((capacity + 15) // 16))


def split_by_home(bucket, dim, wall, bf16=False):
    """home buckets (16 slots each) of the pool's keys -> (indices of near candidates, of far candidates), in pool order"""
    first = bucket.astype(np.int64) * 16
    far = first >= wall_slot(dim, wall, bf16)
    near = (first + 16) * row_bytes(dim, bf16) <= (1 << 31)
    return np.flatnonzero(near), np.flatnonzero(far)


def table_bytes(dim, wall, planes, bf16=False, capacity=None):
    cap = 16 * n_buckets_for(capacity or capacity_for(dim, wall, bf16))
    return cap * (8 + planes * row_bytes(dim, bf16))


def require_hbm(dev, need):
    """the skip rule: this test's own need (tables + 1 GiB of workspace and batch buffers) plus 8 GiB"""
    need += GIB
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info(dev)
    if free < need + 8 * GIB:
        pytest.skip(f"needs {need / GIB:.1f} GiB of HBM plus 8 GiB of headroom; {free / GIB:.1f} GiB are free")


def rnd(x):
    """what a bf16-row table stores for fp32 rows x (numpy), as fp32: torch's CPU cast, the spec's rule (tests/test_bf16_rows.py)"""
    return torch.from_numpy(np.ascontiguousarray(x)).to(BF16).to(torch.float32).numpy()


def test_pool_has_far_and_near_candidates():
    """CPU: for every (shape, wall, row type) the file parametrises, the pool holds the keys far_table() takes — by the oracle's hash and the
    bucket-count rule of SPEC.md §2, the rule the device's hash_batch and the table follow."""
    pool = synth.keys_np(POOL_SEED, 0, POOL)
    for bf16 in (False, True):
        for dim, wall in CASES:
            for grow in (1.0, 1.01, 1.2):       # the second table of the import test, the table behind reserve()
                nb = n_buckets_for(int(capacity_for(dim, wall, bf16) * grow))
                if grow == 1.0:
                    assert 0.05 < 1 - wall_slot(dim, wall, bf16) / (16 * nb) < 0.10      # the last 5-10 % of the slots lie beyond the wall
                _, bkt, _ = oracle.hash_batch(pool, nb, 1)
                near, far = split_by_home(bkt, dim, wall, bf16)
                assert far.size >= N_KEYS + N_FRESH >= 512 and near.size >= N_KEYS >= 512, (dim, wall, bf16, grow, near.size, far.size)


# ---- the helper: a sparse table with a proven set of far keys, and its twin ----------------------------------------------------------------
class Far(types.SimpleNamespace):
    def rows(self, keys, seed=2):
        """key-derived rows (what the twin is fed: rounded once for a bf16-row table)"""
        r = synth.rows_np(np.ascontiguousarray(keys), self.dim, seed)
        return rnd(r) if self.bf16 else r

    def batch(self, rng, n=6000, absent=64):
        """n positions that mix near and far keys with duplicates (one key 80 times over), + absent keys, shuffled"""
        u = np.concatenate([self.near, self.far])
        b = np.concatenate([u[rng.integers(0, u.size, n - 80)], np.repeat(self.far[7], 80), self.absent[:absent]])
        rng.shuffle(b)
        return b

    def slots_of(self, keys):
        slots, found = self.t.locate(T(keys, self.dev))
        assert bool(found.all())
        return (slots & SLOT_MASK).cpu().numpy()

    def prove(self, far=None, near=None, what=""):
        """the hard assert: at least 512 far keys are stored beyond the wall and at least 512 near keys below 2^31 bytes"""
        s = self.slots_of(self.far if far is None else far)
        n_far = int((s >= self.wall_slot).sum())
        assert n_far >= 512, f"{what}: only {n_far} keys lie beyond the wall (slot {self.wall_slot})"
        if near is not False:
            s = self.slots_of(self.near if near is None else near)
            n_near = int(((s + 1) * row_bytes(self.dim, self.bf16) <= (1 << 31)).sum())
            assert n_near >= 512, f"{what}: only {n_near} keys lie below 2^31 bytes"

    def check(self, what=""):
        """size(), status(), the key-sorted export with every state plane, and a find of every stored and some absent keys == the twin's"""
        assert self.t.size() == self.o.size(), what
        assert self.t.status() == self.o.status(), what
        assert_tables_bit_equal(self.t, self.o, what)
        q = np.concatenate([self.near, self.far, self.fresh[:64], self.absent[:64]])
        out, found = self.t.find(T(q, self.dev))
        er, ef = self.o.find(q)
        assert np.array_equal(found.cpu().numpy(), ef) and np.array_equal(out.cpu().numpy(), er), what


def choose_keys(dev, t, dim, wall, bf16):
    pool = synth.keys_t(POOL_SEED, 0, POOL, dev)
    _, bkt, _ = hash_batch(pool, t.n_buckets, 1)
    near, far = split_by_home(bkt.cpu().numpy(), dim, wall, bf16)
    pool = pool.cpu().numpy()
    assert far.size >= N_KEYS + N_FRESH and near.size >= N_KEYS
    return pool[near[:N_KEYS]], pool[far[:N_KEYS]], pool[far[N_KEYS:N_KEYS + N_FRESH]]


@contextlib.contextmanager
def far_table(dev, dim, wall, *, bf16=False, fill=True, capacity=None, hbm_extra=0, **opts):
    """(row shape, table options, wall) -> Far: .t the sparse LookupTable, .o its oracle twin (same options, load <= 0.5), .near / .far the stored
    keys, .fresh far-home keys that are not stored, .absent keys of another stream.  Both tables are closed on the way out."""
    planes = 1 + {OPT_NONE: 0, OPT_ADAGRAD: 1, OPT_ADAM: 2}[opts.get("optimizer", OPT_NONE)]
    capacity = capacity or capacity_for(dim, wall, bf16)
    require_hbm(dev, table_bytes(dim, wall, planes, bf16, capacity) + hbm_extra)
    t = LookupTable(capacity, dim, device=dev, max_batch=MAX_BATCH, value_dtype=BF16 if bf16 else torch.float32, **opts)
    oo = dict(opts)
    if bf16:
        oo["default_value"] = float(rnd(np.float32([opts.get("default_value", 0.0)]))[0])
    o = oracle.OracleTable(4 * (2 * N_KEYS + N_FRESH), dim, **oo)
    try:
        assert t.capacity * row_bytes(dim, bf16) > (1 << 32) and 0.90 < wall_slot(dim, wall, bf16) / t.capacity < 0.95
        near, far, fresh = choose_keys(dev, t, dim, wall, bf16)
        F = Far(t=t, o=o, dev=dev, dim=dim, wall=wall, bf16=bf16, wall_slot=wall_slot(dim, wall, bf16), near=near, far=far, fresh=fresh,
                absent=synth.keys_np(POOL_SEED + 1, 0, 512))
        if fill:
            keys = np.random.default_rng(dim).permutation(np.concatenate([near, far]))
            t.insert(T(keys, dev), T(synth.rows_np(keys, dim, 2), dev))   # (a bf16-row table rounds once)
            o.insert(keys, F.rows(keys))
            F.prove(what="after the insert")
        yield F
    finally:
        t.close(); o.close()


def same_rows(out, found, er, ef, what):
    assert np.array_equal(found.cpu().numpy(), ef), f"{what}: found mask"
    assert np.array_equal(out.cpu().numpy(), er), f"{what}: rows"


def same_bf16(out, ref_f32, what):
    """a bf16 result against bf16(reference) (CPU cast), bit for bit"""
    ref = torch.from_numpy(np.ascontiguousarray(ref_f32)).to(BF16)
    assert out.dtype == BF16 and out.shape == ref.shape, what
    assert torch.equal(out.cpu().view(torch.int16), ref.view(torch.int16)), f"{what}: bf16 rows"


def offsets_of(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def bags_over(rng, universe, absent, n_small=300):
    """bags that mix the keys of `universe` (near and far) with absent keys: empty bags, bags of one, odd lengths, long bags"""
    lens = np.concatenate([[0, 1, 2, 3, 0, 57, 400, 1], rng.integers(0, 12, n_small), [0]])
    off = offsets_of(lens)
    keys = universe[rng.integers(0, universe.size, off[-1])].copy()
    keys[rng.integers(0, keys.size, 40)] = absent[:40]
    return keys, off


# ---- 2. operators, single fp32 table --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dim,wall", CASES, ids=[IDS(c) for c in CASES])
def test_insert_and_every_find_form(dev, dim, wall):
    """insert, find (plain / flags / unordered / bf16 out), find_many, find_located"""
    rng = np.random.default_rng(1)
    with far_table(dev, dim, wall, default_value=0.25) as F:
        q = F.batch(rng)
        qt = T(q, dev)
        er, ef = F.o.find(q)
        for form, kw in (("plain", {}), ("flags", dict(flags=_lib.FIND_STREAM_STORES | _lib.FIND_STREAM_ROWS)), ("unordered", dict(unordered=True))):
            torch.cuda.synchronize()          # (an unordered find is not ordered behind the copy of its keys)
            out, found = F.t.find(qt, **kw)
            same_rows(out, found, er, ef, f"find {form}")
        out, found = F.t.find(qt, out_dtype=BF16)
        assert np.array_equal(found.cpu().numpy(), ef)
        same_bf16(out, er, "find bf16 out")
        reqs = [F.far[:700], F.near[:300], q[:1001]]
        for (out, found), k in zip(F.t.find_many([T(k, dev) for k in reqs]), reqs):
            same_rows(out, found, *F.o.find(k), "find_many")
        out, found, slots = F.t.find_located(qt)
        same_rows(out, found, er, ef, "find_located")
        slots = slots.cpu().numpy()
        assert np.array_equal(slots >= 0, ef.astype(bool))
        assert np.array_equal(slots[ef > 0] & SLOT_MASK, F.slots_of(q[ef > 0]))
        # a second batch of new far keys: the insert kernel's row store beyond the wall, duplicates (last wins) included
        k2 = np.concatenate([F.fresh[:600], F.fresh[:50], F.near[:100]])
        r2 = synth.rows_np(k2, dim, 4) + np.arange(k2.size, dtype=np.float32)[:, None]   # (a duplicate's two rows differ)
        F.t.insert(T(k2, dev), T(r2, dev)); F.o.insert(k2, r2)
        F.prove(far=F.fresh[:600], near=False, what="second insert")
        out, found = F.t.find(T(k2, dev))
        same_rows(out, found, *F.o.find(k2), "find after the second insert")
        F.check("insert / find")


@pytest.mark.gpu
@pytest.mark.parametrize("dim,wall", CASES, ids=[IDS(c) for c in CASES])
def test_find_or_insert_creates_far_rows(dev, dim, wall):
    """find_or_insert and find_or_insert_located on new keys whose home is far: the initial row (INIT_UNIFORM) and initial_accumulator land far"""
    rng = np.random.default_rng(2)
    with far_table(dev, dim, wall, optimizer=OPT_ADAGRAD, default_value=0.25, initial_accumulator=0.1, initializer=INIT_UNIFORM, init_scale=0.05,
                   init_seed=7) as F:
        half = N_FRESH // 2
        for form, new in (("find_or_insert", F.fresh[:half]), ("find_or_insert_located", F.fresh[half:])):
            q = np.concatenate([new, new[:40], F.near[:200], F.far[:200], [oracle.EMPTY_KEY]])
            rng.shuffle(q)
            er, ef = F.o.find_or_insert(q)
            if form == "find_or_insert":
                out, found = F.t.find_or_insert(T(q, dev))
            else:
                out, found, slots = F.t.find_or_insert_located(T(q, dev))
                slots = slots.cpu().numpy()
                assert np.array_equal(slots >= 0, q != oracle.EMPTY_KEY)
                assert np.array_equal(slots[slots >= 0] & SLOT_MASK, F.slots_of(q[slots >= 0]))
            same_rows(out, found, er, ef, form)
        F.prove(far=F.fresh, what="the created keys")
        g, gh = exact_grads_dev(torch.Generator(device=dev).manual_seed(dim), F.fresh.size, dim, dev)   # the new rows and their state take a step
        F.t.apply_adagrad(T(F.fresh, dev), g, lr=0.05); F.o.apply_adagrad(F.fresh, gh, 0.05, 1e-10)
        F.check("find_or_insert")


@pytest.mark.gpu
@pytest.mark.parametrize("dim,wall", CASES_3, ids=[IDS(c) for c in CASES_3])
def test_assign_planes_remove_clear(dev, dim, wall):
    """assign, assign_plane / find_plane for planes 1 and 2, remove (find misses; the re-inserted keys take slots beyond the wall again: the
    tombstones of their home buckets, SPEC.md §2), clear and re-insert"""
    rng = np.random.default_rng(3)
    with far_table(dev, dim, wall, optimizer=OPT_ADAM, default_value=0.25) as F:
        q = np.concatenate([F.far, F.near[:500], F.absent[:50], F.far[:30]])
        rng.shuffle(q)
        rows = synth.rows_np(q, dim, 5) + np.arange(q.size, dtype=np.float32)[:, None]   # (duplicates: the last occurrence wins)
        assert np.array_equal(F.t.assign(T(q, dev), T(rows, dev)).cpu().numpy(), F.o.assign(q, rows))
        u = np.unique(q)
        for plane in (1, 2):
            st = synth.rows_np(u, dim, 5 + plane)
            assert np.array_equal(F.t.assign_plane(plane, T(u, dev), T(st, dev)).cpu().numpy(), F.o.assign_plane(plane, u, st))
            out, found = F.t.find_plane(plane, T(q, dev))
            same_rows(out, found, *F.o.find_plane(plane, q), f"find_plane {plane}")
        F.check("assign / assign_plane")
        gone = np.concatenate([F.far[:1200], F.near[:300], F.absent[:20], F.far[:10]])
        epoch = F.t.layout_epoch
        assert np.array_equal(F.t.remove(T(gone, dev)).cpu().numpy(), F.o.remove(gone)) and F.t.layout_epoch != epoch
        out, found = F.t.find(T(gone, dev))
        same_rows(out, found, *F.o.find(gone), "find after remove")
        assert not bool(found.any())
        F.check("remove")
        back = np.unique(gone)
        rows = synth.rows_np(back, dim, 8)
        F.t.insert(T(back, dev), T(rows, dev)); F.o.insert(back, rows)      # the far tombstones are taken again (SPEC.md §2 placement)
        F.prove(far=F.far[:1200], near=False, what="re-insert after remove")
        F.check("re-insert after remove")
        F.t.clear(); F.o.clear()
        assert F.t.size() == 0 and not bool(F.t.find(T(F.far, dev))[1].any())
        keys = np.concatenate([F.far, F.near])
        rows = synth.rows_np(keys, dim, 9)
        F.t.insert(T(keys, dev), T(rows, dev)); F.o.insert(keys, rows)
        F.prove(what="re-insert after clear")
        F.check("clear and re-insert")


# ---- pooled ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dim,wall", CASES, ids=[IDS(c) for c in CASES])
def test_pooled_lookups_and_weighted_backward(dev, dim, wall):
    """find_pooled sum / mean / weighted / bf16 out and pooled_weighted_backward over bags that mix near, far and absent keys"""
    rng = np.random.default_rng(4)
    with far_table(dev, dim, wall, default_value=0.125) as F:
        keys, off = bags_over(rng, np.concatenate([F.near, F.far]), F.absent)
        kt, ot = T(keys, dev), T(off, dev)
        er, ef = F.o.find(keys)
        for mode in ("sum", "mean"):
            out, found = F.t.find_pooled(kt, ot, mode)
            same_rows(out, found, oracle.pool_rows(er, off, mode), ef, f"find_pooled {mode}")
            out, found = F.t.find_pooled(kt, ot, mode, out_dtype=BF16)
            assert np.array_equal(found.cpu().numpy(), ef)
            same_bf16(out, oracle.pool_rows(er, off, mode), f"find_pooled {mode} bf16 out")
        w = rng.standard_normal(keys.size).astype(np.float32)
        wt = T(w, dev)
        loc = torch.empty(keys.size, dtype=torch.int64, device=dev)
        out, found = F.t.find_pooled(kt, ot, weights=wt, located=loc)
        same_rows(out, found, weighted_pool(er, off, w), ef, "find_pooled weighted")
        assert np.array_equal(loc.cpu().numpy()[ef > 0] & SLOT_MASK, F.slots_of(keys[ef > 0]))
        out, found = F.t.find_pooled(kt, ot, weights=wt, out_dtype=BF16)
        same_bf16(out, weighted_pool(er, off, w), "find_pooled weighted bf16 out")
        bg = rng.standard_normal((off.size - 1, dim)).astype(np.float32)
        ref, tol = weight_grads_ref(bg, er, off)
        for form, kw in (("probing", {}), ("located", dict(located=loc))):
            g, wg = F.t.pooled_weighted_backward(kt, ot, wt, T(bg, dev), **kw)
            assert np.array_equal(g.cpu().numpy(), w[:, None] * bg[bag_of_positions(off)]), form
            assert np.all(np.abs(wg.cpu().numpy().astype(np.float64) - ref) <= tol), form     # SPEC.md §3: within 1e-6 · Σ|products| of fp64
        F.check("pooled lookups")


# ---- optimizer steps ---------------------------------------------------------------------------------------------------------------------------
def oracle_step(o, opt, keys, grads, step):
    if opt == "adagrad":
        o.apply_adagrad(keys, grads, 0.05, 1e-10)
    else:
        o.apply_adam(keys, grads, 0.01, 0.9, 0.999, 1e-8, step)


def table_step(t, opt, keys, grads, step, **kw):
    if opt == "adagrad":
        t.apply_adagrad(keys, grads, lr=0.05, **kw)
    else:
        t.apply_adam(keys, grads, lr=0.01, step=step, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("opt,dim,wall", OPT_CASES, ids=["-".join(map(str, c)) for c in OPT_CASES])
def test_optimizer_steps_bit_exact(dev, opt, dim, wall):
    """apply_adagrad / apply_adam, probing, located (handles of find_located, and of the training forward) and indexed, on batches that mix near
    and far keys with duplicates; exactly summable gradients, so rows and state planes are held bit for bit after every step"""
    rng = np.random.default_rng(5)
    gen = torch.Generator(device=dev).manual_seed(dim)
    with far_table(dev, dim, wall, optimizer=OPT_ADAGRAD if opt == "adagrad" else OPT_ADAM, initial_accumulator=0.1) as F:
        for step, form in enumerate(("probing", "located", "located_prepare", "indexed"), 1):
            q = F.batch(rng)
            qt = T(q, dev)
            if form == "indexed":
                pool, ph = exact_grads_dev(gen, 1500, dim, dev, positions=q.size)
                idx = rng.integers(0, 1500, q.size)
                table_step(F.t, opt, qt, pool, step, grad_index=T(idx, dev))
                gh = ph[idx]
            else:
                g, gh = exact_grads_dev(gen, q.size, dim, dev)
                if form == "probing":
                    table_step(F.t, opt, qt, g, step)
                else:
                    out, found, slots = F.t.find_located(qt, prepare_apply=form == "located_prepare")
                    same_rows(out, found, *F.o.find(q), form)
                    table_step(F.t, opt, qt, g, step, slots=slots)
            oracle_step(F.o, opt, q, gh, step)
            assert F.t.status() == 0
            assert_tables_bit_equal(F.t, F.o, f"{opt} dim {dim} {wall} {form}:")
        F.check("optimizer steps")


# ---- export, import, reserve -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dim,wall", CASES, ids=[IDS(c) for c in CASES])
def test_export_ranges_and_import(dev, dim, wall):
    """export_range(with_state=True) over slot ranges that bracket the wall and the table's end, then import_ of the whole export into a second
    far table (created after the first is closed)"""
    span = 1 << 16 if dim == 1024 else 1 << 20      # an export piece is span × dim × 4 bytes per plane
    with far_table(dev, dim, wall, optimizer=OPT_ADAGRAD, initial_accumulator=0.1, hbm_extra=3 * span * dim * 4) as F:
        keys = np.concatenate([F.near, F.far])
        st = synth.rows_np(keys, dim, 3)
        assert bool(F.t.assign_plane(1, T(keys, dev), T(st, dev)).all()) and F.o.assign_plane(1, keys, st).all()
        slots = F.slots_of(keys)
        cap, ws = F.t.capacity, F.wall_slot
        for b, e in ((ws - span // 2, ws + span // 2), (cap - span, cap + 5), (0, span)):
            ek, ev, e1, e2 = F.t.export_range(b, e, with_state=True)
            inside = keys[(slots >= b) & (slots < e)]
            assert e2 is None and inside.size > 0, (b, e)
            order = torch.argsort(ek).cpu()
            assert np.array_equal(ek.cpu()[order].numpy(), np.sort(inside)), (b, e)
            assert np.array_equal(ev.cpu()[order].numpy(), F.o.find(np.sort(inside))[0]), (b, e)
            assert np.array_equal(e1.cpu()[order].numpy(), F.o.find_plane(1, np.sort(inside))[0]), (b, e)
            del ek, ev, e1
        pieces = [tuple(x.clone() for x in p[:3]) for p in F.t.iter_export(span, with_state=True)]
        assert sum(p[0].numel() for p in pieces) == keys.size
        twin = export_sorted(F.o)
    with far_table(dev, dim, wall, optimizer=OPT_ADAGRAD, initial_accumulator=0.1, fill=False, capacity=int(capacity_for(dim, wall) * 1.01)) as G:
        for ek, ev, e1 in pieces:
            G.t.import_(ek, ev, e1)
        s = (G.t.locate(T(F.far, dev))[0] & SLOT_MASK).cpu().numpy()
        assert int((s >= G.wall_slot).sum()) >= 512
        assert G.t.size() == keys.size and G.t.status() == 0
        for name, x, z in zip(("keys", "values", "state1"), export_sorted(G.t), twin):
            assert np.array_equal(x, z), f"import_: {name} differ from the twin"


@pytest.mark.gpu
@pytest.mark.parametrize("dim", SHAPES)
def test_reserve_keeps_far_rows(dev, dim):
    """reserve past the byte wall (old and new planes coexist: a 5.1 GB plane grows to 6.1 GB): far keys keep rows and state, layout_epoch moves"""
    grown = int(capacity_for(dim, "byte") * 1.2)
    with far_table(dev, dim, "byte", optimizer=OPT_ADAGRAD, initial_accumulator=0.1, hbm_extra=table_bytes(dim, "byte", 2, capacity=grown)) as F:
        keys = np.concatenate([F.near, F.far])
        st = np.abs(synth.rows_np(keys, dim, 3)) + np.float32(0.1)      # (an accumulator: not negative)
        assert bool(F.t.assign_plane(1, T(keys, dev), T(st, dev)).all()) and F.o.assign_plane(1, keys, st).all()
        epoch, cap = F.t.layout_epoch, F.t.capacity
        F.t.reserve(grown)
        assert F.t.layout_epoch != epoch and F.t.capacity == 16 * n_buckets_for(grown) > cap
        F.prove(what="after reserve")      # (a key's home keeps its relative place in the table: far keys stay far)
        F.check("reserve")
        g, gh = exact_grads_dev(torch.Generator(device=dev).manual_seed(dim), keys.size, dim, dev)
        F.t.apply_adagrad(T(keys, dev), g, lr=0.05); F.o.apply_adagrad(keys, gh, 0.05, 1e-10)
        F.check("a step after reserve")


# ---- the bf16-row table ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dim,wall", CASES, ids=[IDS(c) for c in CASES])
def test_bf16_row_table(dev, dim, wall):
    """insert (fp32 rounded once, bf16 verbatim), find (fp32 / bf16 out), find_pooled, assign, remove, export on rows of 2·dim bytes; the
    reference is the fp32 oracle twin fed the rounded rows"""
    rng = np.random.default_rng(6)
    with far_table(dev, dim, wall, bf16=True, default_value=0.3) as F:
        k2 = F.fresh[:600]
        r2 = torch.from_numpy(synth.rows_np(k2, dim, 4)).to(BF16)
        F.t.insert(T(k2, dev), r2.to(dev)); F.o.insert(k2, r2.float().numpy())          # bf16 input: stored verbatim
        F.prove(far=k2, near=False, what="bf16 input")
        q = np.concatenate([F.batch(rng), k2])
        er, ef = F.o.find(q)
        out, found = F.t.find(T(q, dev))
        same_rows(out, found, er, ef, "find")
        out, found = F.t.find(T(q, dev), out_dtype=BF16)
        assert np.array_equal(found.cpu().numpy(), ef)
        same_bf16(out, er, "find bf16 out")
        keys, off = bags_over(rng, np.concatenate([F.near, F.far]), F.absent)
        pr, pf = F.o.find(keys)
        for mode in ("sum", "mean"):
            out, found = F.t.find_pooled(T(keys, dev), T(off, dev), mode)
            same_rows(out, found, oracle.pool_rows(pr, off, mode), pf, f"find_pooled {mode}")
            out, found = F.t.find_pooled(T(keys, dev), T(off, dev), mode, out_dtype=BF16)
            same_bf16(out, oracle.pool_rows(pr, off, mode), f"find_pooled {mode} bf16 out")
        a = np.concatenate([F.far[:900], F.near[:300], F.absent[:30]])
        rows = synth.rows_np(a, dim, 5)
        assert np.array_equal(F.t.assign(T(a, dev), T(rows, dev)).cpu().numpy(), F.o.assign(a, rnd(rows)))
        b = np.concatenate([F.far[900:1500], F.near[300:400]])
        rb = torch.from_numpy(synth.rows_np(b, dim, 6)).to(BF16)
        assert np.array_equal(F.t.assign(T(b, dev), rb.to(dev)).cpu().numpy(), F.o.assign(b, rb.float().numpy()))
        F.check("insert / assign")
        gone = np.concatenate([F.far[:1000], F.near[:200], F.absent[:10]])
        assert np.array_equal(F.t.remove(T(gone, dev)).cpu().numpy(), F.o.remove(gone))
        F.check("remove")
        back = gone[:1200]
        rows = synth.rows_np(back, dim, 8)
        F.t.insert(T(back, dev), T(rows, dev)); F.o.insert(back, rnd(rows))
        F.prove(far=F.far[:1000], near=False, what="re-insert after remove")
        F.check("re-insert after remove")


@pytest.mark.gpu
@pytest.mark.parametrize("dim", SHAPES)
def test_bf16_row_table_reserve(dev, dim):
    grown = int(capacity_for(dim, "byte", True) * 1.2)
    with far_table(dev, dim, "byte", bf16=True, default_value=0.3, hbm_extra=table_bytes(dim, "byte", 1, True, grown)) as F:
        epoch = F.t.layout_epoch
        F.t.reserve(grown)
        assert F.t.layout_epoch != epoch and F.t.capacity == 16 * n_buckets_for(grown)
        F.prove(what="after reserve")
        F.check("reserve")


# ---- groups: member 0 small, member 1 the far table, so the member bases differ ---------------------------------------------------------------
SMALL_KEYS = 1500


@contextlib.contextmanager
def small_member(dev, dim, *, bf16=False, **opts):
    """(small table, its twin, its keys): member 0 of the groups"""
    t = LookupTable(4000, dim, device=dev, max_batch=MAX_BATCH, value_dtype=BF16 if bf16 else torch.float32, **opts)
    oo = dict(opts)
    if bf16:
        oo["default_value"] = float(rnd(np.float32([opts.get("default_value", 0.0)]))[0])
    o = oracle.OracleTable(8000, dim, **oo)
    u = synth.keys_np(POOL_SEED + 2, 0, SMALL_KEYS)
    rows = synth.rows_np(u, dim, 12)
    t.insert(T(u, dev), T(rows, dev)); o.insert(u, rnd(rows) if bf16 else rows)
    try:
        yield t, o, u
    finally:
        t.close(); o.close()


def member_bags(rng, universes, absent, bpt):
    """bag_offsets of len(universes) × bpt bags and their keys: the bags of member j draw on universes[j] (+ a few absent keys)"""
    lens = rng.integers(0, 9, len(universes) * bpt)
    lens[3] = 0; lens[bpt] = 45; lens[2 * bpt - 1] = 33
    off = offsets_of(lens)
    segs = []
    for j, u in enumerate(universes):
        k = u[rng.integers(0, u.size, off[(j + 1) * bpt] - off[j * bpt])].copy()
        k[::97] = absent[:k[::97].size]
        segs.append(k)
    return np.concatenate(segs), off, lens


@pytest.mark.gpu
@pytest.mark.parametrize("opt,dim,wall", OPT_CASES, ids=["-".join(map(str, c)) for c in OPT_CASES])
def test_table_group_with_a_far_member(dev, opt, dim, wall):
    """TableGroup of a small member and the far table: find, find_or_insert, apply_adagrad / apply_adam, find_pooled, apply_pooled,
    find_pooled_jagged, apply_indexed, pooled_weighted_backward — against the per-member twins"""
    rng = np.random.default_rng(7)
    gen = torch.Generator(device=dev).manual_seed(dim)
    kw = dict(optimizer=OPT_ADAGRAD if opt == "adagrad" else OPT_ADAM, initial_accumulator=0.1, initializer=INIT_UNIFORM, init_scale=0.05, init_seed=3)
    with far_table(dev, dim, wall, default_value=0.25, **kw) as F, small_member(dev, dim, default_value=-0.5, **kw) as (t0, o0, u0):
        grp = TableGroup([t0, F.t], max_apply_batch=MAX_BATCH)
        twins, univ = (o0, F.o), (u0, np.concatenate([F.near, F.far]))
        try:
            def per_member(keys, off2):
                return [(twins[j], keys[off2[j]:off2[j + 1]], off2[j], off2[j + 1]) for j in range(2)]

            # find, fp32 and bf16 out
            seg = [np.concatenate([u0[rng.integers(0, u0.size, 900)], F.absent[:9]]), F.batch(rng, 5000)]
            keys, off2 = np.concatenate(seg), offsets_of([s.size for s in seg])
            kt, o2t = T(keys, dev), T(off2, dev)
            er = np.concatenate([o.find(k)[0] for o, k, _, _ in per_member(keys, off2)])
            ef = np.concatenate([o.find(k)[1] for o, k, _, _ in per_member(keys, off2)])
            out, found = grp.find(kt, o2t)
            same_rows(out, found, er, ef, "group find")
            out, found = grp.find(kt, o2t, out_dtype=BF16)
            assert np.array_equal(found.cpu().numpy(), ef)
            same_bf16(out, er, "group find bf16 out")
            # find_or_insert: new keys in both members, the far member's with a far home
            seg = [np.concatenate([synth.keys_np(POOL_SEED + 3, 0, 200), u0[:300]]), np.concatenate([F.fresh, F.fresh[:30], F.near[:200], F.far[:200]])]
            for s in seg:
                rng.shuffle(s)
            k2, off_b = np.concatenate(seg), offsets_of([s.size for s in seg])
            res = [o.find_or_insert(k) for o, k, _, _ in per_member(k2, off_b)]
            out, found = grp.find_or_insert(T(k2, dev), T(off_b, dev))
            same_rows(out, found, np.concatenate([r[0] for r in res]), np.concatenate([r[1] for r in res]), "group find_or_insert")
            F.prove(far=F.fresh, near=False, what="group find_or_insert")
            # one step per position
            g, gh = exact_grads_dev(gen, keys.size, dim, dev)
            if opt == "adagrad":
                grp.apply_adagrad(kt, o2t, g, lr=0.05)
            else:
                grp.apply_adam(kt, o2t, g, lr=0.01, step=1)
            for o, k, lo, hi in per_member(keys, off2):
                oracle_step(o, opt, k, gh[lo:hi], 1)
            for t, o in ((t0, o0), (F.t, F.o)):
                assert_tables_bit_equal(t, o, f"group apply_{opt}:")
            # the embedding-bag collection: pooled forward (located rows handed over) and its step
            bpt = 37
            bk, off, lens = member_bags(rng, univ, F.absent, bpt)
            bkt, boff = T(bk, dev), T(off, dev)
            m2 = off[::bpt]                                   # member offsets of the pooled batch
            for mode in ("mean", "sum"):
                located = torch.empty(bk.size, dtype=torch.int64, device=dev)
                out, found = grp.find_pooled(bkt, boff, mode, located=located)
                out, found = out.cpu().numpy(), found.cpu().numpy()
                for j, (o, k, lo, hi) in enumerate(per_member(bk, m2)):
                    r, f = o.find(k)
                    assert np.array_equal(found[lo:hi], f), mode
                    assert np.array_equal(out[j * bpt:(j + 1) * bpt], oracle.pool_rows(r, off[j * bpt:(j + 1) * bpt + 1] - lo, mode)), (mode, j)
            bag_of = bag_of_positions(off)
            bgr, bgh = exact_grads_dev(gen, 2 * bpt, dim, dev, positions=bk.size)
            grp.apply_pooled(bkt, boff, bgr, T(bag_of, dev), opt, located=located, **(dict(lr=0.05) if opt == "adagrad" else dict(lr=0.01, step=2)))
            for o, k, lo, hi in per_member(bk, m2):
                oracle_step(o, opt, k, bgh[bag_of[lo:hi]], 2)
            for t, o in ((t0, o0), (F.t, F.o)):
                assert_tables_bit_equal(t, o, f"group apply_pooled {opt}:")
            # the jagged bag -> member map: member 0 owns 5 bags, member 1 the rest
            nb, own0 = 2 * bpt, 5
            mb = np.array([0, own0, nb], dtype=np.int64)
            jk = np.concatenate([u0[rng.integers(0, u0.size, off[own0])], univ[1][rng.integers(0, univ[1].size, off[-1] - off[own0])]])
            out, found = grp.find_pooled_jagged(T(jk, dev), boff, T(mb, dev), "sum")
            out, found = out.cpu().numpy(), found.cpu().numpy()
            for j, (lo_b, hi_b) in enumerate(((0, own0), (own0, nb))):
                lo, hi = off[lo_b], off[hi_b]
                r, f = twins[j].find(jk[lo:hi])
                assert np.array_equal(found[lo:hi], f)
                assert np.array_equal(out[lo_b:hi_b], oracle.pool_rows(r, off[lo_b:hi_b + 1] - lo, "sum")), j
            # indexed step over the per-position batch
            pool, ph = exact_grads_dev(gen, 1200, dim, dev, positions=keys.size)
            idx = rng.integers(0, 1200, keys.size)
            grp.apply_indexed(kt, o2t, pool, T(idx, dev), opt, **(dict(lr=0.05) if opt == "adagrad" else dict(lr=0.01, step=3)))
            for o, k, lo, hi in per_member(keys, off2):
                oracle_step(o, opt, k, ph[idx[lo:hi]], 3)
            for t, o in ((t0, o0), (F.t, F.o)):
                assert_tables_bit_equal(t, o, f"group apply_indexed {opt}:")
            # weighted bags: forward with handles, backward
            w = rng.standard_normal(bk.size).astype(np.float32)
            located = torch.empty(bk.size, dtype=torch.int64, device=dev)
            out, found = grp.find_pooled(bkt, boff, weights=T(w, dev), located=located)
            rows = np.concatenate([o.find(k)[0] for o, k, _, _ in per_member(bk, m2)])
            for j, (o, k, lo, hi) in enumerate(per_member(bk, m2)):
                assert np.array_equal(out.cpu().numpy()[j * bpt:(j + 1) * bpt], weighted_pool(rows[lo:hi], off[j * bpt:(j + 1) * bpt + 1] - lo, w[lo:hi])), j
            bg = rng.standard_normal((2 * bpt, dim)).astype(np.float32)
            ref, tol = weight_grads_ref(bg, rows, off)
            for form, kw2 in (("probing", {}), ("located", dict(located=located))):
                gr, wg = grp.pooled_weighted_backward(bkt, boff, T(w, dev), T(bg, dev), **kw2)
                assert np.array_equal(gr.cpu().numpy(), w[:, None] * bg[bag_of]), form
                assert np.all(np.abs(wg.cpu().numpy().astype(np.float64) - ref) <= tol), form
            F.check("group")
            assert_tables_bit_equal(t0, o0, "group, the small member:")
        finally:
            grp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dim,wall", CASES, ids=[IDS(c) for c in CASES])
def test_bf16_row_serving_group(dev, dim, wall):
    """the bf16-row serving group: find and find_pooled, fp32 and bf16 out"""
    rng = np.random.default_rng(8)
    with far_table(dev, dim, wall, bf16=True, default_value=0.3) as F, small_member(dev, dim, bf16=True, default_value=-1.7) as (t0, o0, u0):
        grp = TableGroup([t0, F.t])
        try:
            seg = [np.concatenate([u0[rng.integers(0, u0.size, 900)], F.absent[:9]]), F.batch(rng, 5000)]
            keys, off2 = np.concatenate(seg), offsets_of([s.size for s in seg])
            res = [o.find(k) for o, k in zip((o0, F.o), seg)]
            er, ef = np.concatenate([r[0] for r in res]), np.concatenate([r[1] for r in res])
            out, found = grp.find(T(keys, dev), T(off2, dev))
            same_rows(out, found, er, ef, "serving group find")
            out, found = grp.find(T(keys, dev), T(off2, dev), out_dtype=BF16)
            assert np.array_equal(found.cpu().numpy(), ef)
            same_bf16(out, er, "serving group find bf16 out")
            bpt = 37
            bk, off, _ = member_bags(rng, (u0, np.concatenate([F.near, F.far])), F.absent, bpt)
            m2 = off[::bpt]
            for mode in ("sum", "mean"):
                exp, ef = [], []
                for j, o in enumerate((o0, F.o)):
                    r, f = o.find(bk[m2[j]:m2[j + 1]])
                    exp.append(oracle.pool_rows(r, off[j * bpt:(j + 1) * bpt + 1] - m2[j], mode)); ef.append(f)
                exp, ef = np.concatenate(exp), np.concatenate(ef)
                out, found = grp.find_pooled(T(bk, dev), T(off, dev), mode)
                same_rows(out, found, exp, ef, f"serving group find_pooled {mode}")
                out, found = grp.find_pooled(T(bk, dev), T(off, dev), mode, out_dtype=BF16)
                assert np.array_equal(found.cpu().numpy(), ef)
                same_bf16(out, exp, f"serving group find_pooled {mode} bf16 out")
            F.check("serving group")
        finally:
            grp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("wall", ["byte", "elem"])
def test_mixed_group_with_a_far_member(dev, wall):
    """MixedTableGroup over a small dim-128 member and the far dim-64 member: find_pooled and apply_pooled"""
    rng = np.random.default_rng(9)
    gen = torch.Generator(device=dev).manual_seed(64)
    kw = dict(optimizer=OPT_ADAGRAD, initial_accumulator=0.1)
    with far_table(dev, 64, wall, default_value=0.25, **kw) as F, small_member(dev, 128, default_value=-0.5, **kw) as (t0, o0, u0):
        grp = MixedTableGroup([t0, F.t], max_apply_batch=MAX_BATCH)
        try:
            bpt, dims = 37, (128, 64)
            bk, off, _ = member_bags(rng, (u0, np.concatenate([F.near, F.far])), F.absent, bpt)
            m2, bag_of = off[::bpt], bag_of_positions(off)
            located = torch.empty(bk.size, dtype=torch.int64, device=dev)
            for mode in ("mean", "sum"):
                views, found = grp.find_pooled(T(bk, dev), T(off, dev), mode, located=located)
                for j, o in enumerate((o0, F.o)):
                    r, f = o.find(bk[m2[j]:m2[j + 1]])
                    assert np.array_equal(found.cpu().numpy()[m2[j]:m2[j + 1]], f)
                    assert np.array_equal(views[j].cpu().numpy(), oracle.pool_rows(r, off[j * bpt:(j + 1) * bpt + 1] - m2[j], mode)), (mode, j)
            flat = torch.zeros(bpt * sum(dims), dtype=torch.float32, device=dev)
            hosts = []
            for v, d in zip(grp.views(flat, bpt), dims):
                g, gh = exact_grads_dev(gen, bpt, d, dev, positions=bk.size)
                v.copy_(g); hosts.append(gh)
            grp.apply_pooled(T(bk, dev), T(off, dev), flat, T(bag_of, dev), "adagrad", lr=0.05, located=located)
            for j, o in enumerate((o0, F.o)):
                o.apply_adagrad(bk[m2[j]:m2[j + 1]], hosts[j][bag_of[m2[j]:m2[j + 1]] - j * bpt], 0.05, 1e-10)
            F.check("mixed group")
            assert_tables_bit_equal(t0, o0, "mixed group, the small member:")
        finally:
            grp.close()


# ---- 3. the output side of the same walls: the caller's buffers, indexed by position × dim4 and bag × dim4 --------------------------------------
OUT_DIM, OUT_N = 1024, (1 << 22) + 4096       # n · dim just over 2^32 elements: a 17.2 GB fp32 out
OUT_DEFAULT = 0.25


def wall_positions(n):
    """positions on both sides of every wall of an [n, 1024] fp32 or bf16 buffer (2^31 / 2^32 bytes and elements: positions 2^19 .. 2^22), the
    first and the last position, and 300 seeded ones in between"""
    p = [0, 1, n - 2, n - 1] + [w + d for w in (1 << 19, 1 << 20, 1 << 21, 1 << 22) for d in (-1, 0, 1)]
    return np.unique(np.concatenate([p, np.random.default_rng(10).integers(0, n, 300)])).astype(np.int64)


@contextlib.contextmanager
def output_tables(dev, n_tables=1):
    """small tables of 1000 key-derived rows each, default 0.25"""
    require_hbm(dev, OUT_N * OUT_DIM * 4 + 2 * GIB)
    ts = [LookupTable(4096, OUT_DIM, device=dev, max_batch=4096, default_value=OUT_DEFAULT) for _ in range(n_tables)]
    us = [synth.keys_np(POOL_SEED + 10 + j, 0, 1000) for j in range(n_tables)]
    for t, u in zip(ts, us):
        t.insert(T(u, dev), T(synth.rows_np(u, OUT_DIM, 2), dev))
    try:
        yield ts, us
    finally:
        for t in ts:
            t.close()


def rows_off_default(out, expect_rows, chunk=1 << 18):
    """on the GPU: bool [n], True where a row of `out` differs from its expected constant row (expect_rows: a float, or fp32 [n] per-row constants)"""
    bad = []
    for s in range(0, out.shape[0], chunk):
        e = expect_rows if isinstance(expect_rows, float) else expect_rows[s:s + chunk, None].to(out.dtype)
        bad.append((out[s:s + chunk] != e).any(dim=1))
    return torch.cat(bad)


def check_output(out, found, pos, default_rows, rows_ref, dev, what):
    """found == the expected mask; rows at the present positions bit-equal; every other row equals its default (a GPU reduction)"""
    mask = torch.zeros(out.shape[0], dtype=torch.bool, device=dev)
    mask[T(pos, dev)] = True
    if found is not None:
        assert torch.equal(found.bool(), mask), f"{what}: found mask"
    bits = torch.int16 if out.dtype == BF16 else torch.int32
    got, ref = out[T(pos, dev)].cpu(), torch.from_numpy(rows_ref).to(out.dtype)
    assert torch.equal(got.view(bits), ref.view(bits)), f"{what}: rows at the present positions"
    off = rows_off_default(out, default_rows)
    assert torch.equal(off, mask), f"{what}: {int((off & ~mask).sum())} rows that should hold the default do not, {int((~off & mask).sum())} present rows hold it"


@pytest.mark.gpu
@pytest.mark.parametrize("out_dtype", [torch.float32, BF16], ids=["fp32", "bf16"])
def test_find_output_past_the_walls(dev, out_dtype):
    """find with n · dim just over 2^32 elements, mostly absent keys: present keys at positions on both sides of each wall"""
    with output_tables(dev) as ((t,), (u,)):
        pos = wall_positions(OUT_N)
        keys = synth.keys_t(POOL_SEED + 20, 0, OUT_N, dev)          # absent
        present = u[np.arange(pos.size) % u.size]
        keys[T(pos, dev)] = T(present, dev)
        out, found = t.find(keys, out_dtype=out_dtype)
        check_output(out, found, pos, OUT_DEFAULT, synth.rows_np(present, OUT_DIM, 2), dev, f"find {out_dtype}")


@pytest.mark.gpu
def test_group_find_output_past_the_walls(dev):
    """TableGroup.find with the same shape: two members, the boundary between their segments at an odd position"""
    with output_tables(dev, 2) as (ts, us):
        grp = TableGroup(ts)
        try:
            pos = wall_positions(OUT_N)
            cut = (1 << 21) + 12345
            keys = synth.keys_t(POOL_SEED + 20, 0, OUT_N, dev)
            member = (pos >= cut).astype(np.int64)
            present = np.where(member == 0, us[0][np.arange(pos.size) % 1000], us[1][np.arange(pos.size) % 1000])
            keys[T(pos, dev)] = T(present, dev)
            out, found = grp.find(keys, torch.tensor([0, cut, OUT_N], dtype=torch.int64, device=dev))
            check_output(out, found, pos, OUT_DEFAULT, synth.rows_np(present, OUT_DIM, 2), dev, "group find")
        finally:
            grp.close()


@pytest.mark.gpu
def test_find_pooled_output_past_the_walls(dev):
    """find_pooled with n_bags · dim over 2^32 elements; bags hold 0-2 keys.  A bag of absent keys is 0, 0.25 or 0.5 in every element; the bags
    at the wall positions hold one present key (after one absent key where the bag has two)"""
    with output_tables(dev) as ((t,), (u,)):
        n_bags = OUT_N
        lens = torch.arange(n_bags, dtype=torch.int64, device=dev) % 3
        pos = wall_positions(n_bags)
        pos = pos[pos % 3 != 0]                                        # (the empty bags stay empty)
        off = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(lens, 0)])
        n = int(off[-1])
        keys = synth.keys_t(POOL_SEED + 20, 0, n, dev)
        present = u[np.arange(pos.size) % u.size]
        last = (off[1:][T(pos, dev)] - 1)                              # the last position of each chosen bag
        keys[last] = T(present, dev)
        out, found = t.find_pooled(keys, off, "sum")
        fmask = torch.zeros(n, dtype=torch.bool, device=dev); fmask[last] = True
        assert torch.equal(found.bool(), fmask)
        rows = synth.rows_np(present, OUT_DIM, 2)
        two = (pos % 3 == 2)
        rows[two] = np.float32(OUT_DEFAULT) + rows[two]               # position order: the absent key's default row first
        check_output(out, None, pos, lens.to(torch.float32) * OUT_DEFAULT, rows, dev, "find_pooled")
