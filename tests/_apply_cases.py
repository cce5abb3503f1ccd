"""Test-only builders shared by test_gpu_parity.py and test_apply_exact.py: the batches that force each way through the sparse
optimizer step, and the two kinds of gradients they are fed.

grads="normal": seeded normals, as the tolerance tests have always drawn them.  SPEC.md §4 leaves the order of the fp64 sum free, so a
batch with duplicate keys can be held to the oracle only within rtol 1e-6.
grads="exact": exactly summable gradients (exact_grads_np / exact_grads_dev).  Their sums are exact in fp64 in every order and every
partial grouping, so the oracle's result is the only correct one and every comparison is bit for bit, duplicates included."""
import functools

import numpy as np
import torch

import oracle
from meepoembedding_amd import OPT_ADAGRAD, OPT_ADAM, LookupTable, synth

RTOL, ATOL = 1e-6, 1e-9
EXACT_MAX_POSITIONS = 1 << 19
EXACT_EXPONENTS = (-12, -24, -36)


def T(a, dev):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).to(dev)   # (the cached inputs are read-only)


def check_exact_grads(g, positions):
    """What makes a gradient array exactly summable: every element is a * 2^e with an integer |a| <= 32 and e in {-12, -24, -36}, and at
    most 2^19 batch positions draw on it.  Any subset sum is then a multiple of 2^-36 below 32 * 2^-12 * 2^19 = 2^12: 48 bits, exact in
    fp64 whatever the order or the grouping — while its rounding to fp32 (24 bits) is a real rounding."""
    assert positions <= EXACT_MAX_POSITIONS, f"{positions} positions: a sum could need more than 48 bits"
    assert g.dtype == np.float32
    scaled = np.ldexp(g.astype(np.float64), 36)
    assert np.array_equal(scaled, np.rint(scaled)) and float(np.abs(g).max(initial=0.0)) <= 32.0 * 2.0 ** -12
    return g


def exact_grads_np(rng, rows, dim, positions=None):
    """[rows, dim] fp32 exactly summable gradients drawn on the host.  positions: how many batch positions read these rows (an indexed
    apply reads a pool of fewer rows through an index); default = one per row."""
    a = rng.integers(-32, 33, size=(rows, dim)).astype(np.float32)
    e = np.asarray(EXACT_EXPONENTS, dtype=np.int32)[rng.integers(0, 3, size=(rows, dim))]
    return check_exact_grads(np.ldexp(a, e).astype(np.float32), rows if positions is None else positions)


def exact_grads_dev(gen, rows, dim, dev, positions=None):
    """The same draw on the device (wide rows: a host draw of 100M values costs seconds per step) -> (device tensor, host copy)."""
    a = torch.randint(-32, 33, (rows, dim), device=dev, generator=gen).to(torch.float32)
    e = -12 * torch.randint(1, 4, (rows, dim), device=dev, generator=gen, dtype=torch.int32)
    gt = torch.ldexp(a, e)
    assert gt.dtype == torch.float32
    return gt, check_exact_grads(gt.cpu().numpy(), rows if positions is None else positions)


def export_sorted(t):
    """(keys, values, state planes that exist) of a LookupTable or an OracleTable, as numpy arrays sorted by key"""
    e = [x.cpu().numpy() if isinstance(x, torch.Tensor) else x for x in t.export(with_state=True) if x is not None]
    order = np.argsort(e[0])
    return [x[order] for x in e]


def assert_tables_bit_equal(t, o, what=""):
    """keys, values and every state plane of table t == those of the oracle o, bit for bit"""
    e, eo = export_sorted(t), export_sorted(o)
    assert len(e) == len(eo)
    for name, x, z in zip(("keys", "values", "state1", "state2"), e, eo):
        same = np.array_equal(x, z)
        if not same and name != "keys" and x.shape == z.shape:
            bad = x.view(np.uint32) != z.view(np.uint32)
            raise AssertionError(f"{what} {name}: {int(bad.sum())} of {bad.size} elements differ from the oracle, in {int(bad.any(axis=1).sum())} rows; "
                                 f"max relative difference {float(np.max(np.abs(x[bad] - z[bad]) / np.maximum(np.abs(z[bad]), 1e-30))):.3g}")
        assert same, f"{what} {name} differ from the oracle"


GROUP_SIZES = list(range(1, 45)) + [64, 65, 100, 333, 2100]


def every_group_size_batch(rng, dim, layout):
    """One batch with a key of EVERY multiplicity 1..44 plus 64, 65, 100, 333 and 2100, three times over, 400 single keys between the groups,
    EMPTY_KEY padding where nothing lands.  'clustered' keeps a key's occurrences adjacent (one block
    of the grouping kernel sees them all), 'spread' puts them 1031 positions apart (every occurrence in another block), 'mixed' does both at
    random.  -> (keys to store, their rows, the 400 single keys, the batch)"""
    sizes = GROUP_SIZES
    n_keys = len(sizes) * 3
    keys = synth.keys_np(123, 0, n_keys + 500); rows = synth.rows_np(keys, dim, 2)
    reps = np.array(sizes * 3)
    bk = np.repeat(keys[:n_keys], reps)
    filler = keys[n_keys:n_keys + 400]                       # single keys between the groups
    n = 1031 * ((bk.size + filler.size) // 1031 + 1)
    batch = np.full(n, oracle.EMPTY_KEY, dtype=np.int64)    # padding where nothing lands
    if layout == "clustered":
        order = np.arange(bk.size)
    elif layout == "spread":
        k = np.arange(bk.size)
        order = (k % (n // 1031)) * 1031 + k // (n // 1031)  # neighbours in bk land 1031 positions apart
        assert np.unique(order).size == bk.size
    else:
        order = rng.permutation(n)[:bk.size]
        half = rng.random(bk.size) < 0.5                     # half of the occurrences stay next to their neighbours
        order[half] = np.sort(order[half])
    batch[order] = bk
    free = np.flatnonzero(batch == oracle.EMPTY_KEY)
    batch[free[:filler.size]] = filler
    return keys[:n_keys + 400], rows[:n_keys + 400], filler, batch


@functools.lru_cache(maxsize=None)
def keys_of_apply_bucket_zero(count, seed):
    """Distinct keys whose mix64 has 13 leading zero bits: for ANY bucket count up to 8192 the bucketed apply puts them all into bucket 0
    (and the table into the first 1/8192 of its buckets).  Cached per (count, seed), read-only: the search hashes millions of candidates."""
    rng = np.random.default_rng(seed)
    got = []
    while sum(len(g) for g in got) < count:
        cand = rng.integers(-(1 << 62), 1 << 62, size=1 << 22, dtype=np.int64)
        mix, _, _ = oracle.hash_batch(cand, 1, 1)
        got.append(cand[mix < (np.uint64(1) << np.uint64(51))])
    keys = np.unique(np.concatenate(got))[:count]
    keys.flags.writeable = False
    return keys


EXTREME_CASES = ["one_key", "one_bucket_many_keys", "forty_hot_keys", "one_bucket_two_keys", "bucket_of_900_distinct", "bucket_of_300_warm"]


def bucketed_apply_extremes(dev, case, opt, kernel, dim, grads="normal"):
    """The rare ways through the bucketed apply (meepo_apply.hip), each forced by construction, plain and located, against the oracle:
    one_key — a single key fills 400K of a 410K-position batch: ~780 slabs of one bucket each emit a record of that key, more records of ONE key
    than a merge pass holds (mono_pass);  one_bucket_many_keys — 3000 keys that all fall into apply bucket 0, 100+ occurrences each: every slab
    emits hundreds of records, the merge has far more records than one pass holds and splits them by hash prefix (the DFS stack);
    forty_hot_keys — 40 keys of ~6000 occurrences in a uniform batch: forty split buckets merge side by side, spare blocks loop over slabs;
    one_bucket_two_keys — two keys of one bucket, 150K occurrences each: the prefix split must separate exactly two keys;
    bucket_of_900_distinct — 900 keys of apply bucket 0, once each, in a small batch: ONE block takes a bucket of ~1000 positions whole (two positions
    per thread) with its LDS hash table filled almost to the last slot;  bucket_of_300_warm — 300 keys of bucket 0 with 1..6 occurrences each: the
    same path with runs.
    kernel: which apply kernel takes the batches — "lean" (block = bucket; a split bucket is taken by its own block one key at a time: what the
    FIRST skewed batch of a stream gets), "full" (slabs, pending records, merges; from the second step on also the hot keys' own buckets, which the
    first step's kernel reported), "auto" (the library's choice: lean for step 0, full for step 1).
    Rows wider than 64 draw their gradients on the device (host normals of 100M values cost seconds per step) and forty_hot_keys gets a smaller
    uniform part; the hot keys' counts, which make each case what it is, are the same at every dim.
    grads: "normal" — seeded normals, compared within RTOL / ATOL;  "exact" — exactly summable gradients (see the module's docstring), every
    comparison bit for bit."""
    assert grads in ("normal", "exact")
    exact = grads == "exact"
    n_bg = 20000
    rng = np.random.default_rng(5)
    bg = synth.keys_np(321, 0, n_bg)
    if case == "one_key":
        hot = synth.keys_np(322, 0, 1); reps = np.array([400_000]); n_fill = 10_000
    elif case == "one_bucket_many_keys":
        hot = keys_of_apply_bucket_zero(3000, 7); reps = rng.integers(100, 140, size=3000); n_fill = 20_000
    elif case == "forty_hot_keys":
        hot = synth.keys_np(323, 0, 40); reps = rng.integers(5000, 7000, size=40); n_fill = 150_000 if dim <= 64 else 30_000
    elif case == "one_bucket_two_keys":
        hot = keys_of_apply_bucket_zero(2, 9); reps = np.array([150_000, 150_001]); n_fill = 5_000
    elif case == "bucket_of_900_distinct":
        hot = keys_of_apply_bucket_zero(900, 11); reps = np.ones(900, dtype=np.int64); n_fill = 5_000
    else:
        hot = keys_of_apply_bucket_zero(300, 12); reps = rng.integers(1, 7, size=300); n_fill = 3_000
    keys = np.unique(np.concatenate([bg, hot]))
    rows = synth.rows_np(keys, dim, 2)
    bk = np.concatenate([np.repeat(hot, reps), bg[rng.integers(0, n_bg, n_fill)], synth.keys_np(324, 0, 50)])   # + 50 absent keys
    rng.shuffle(bk)
    n = bk.size
    kind, okind = (OPT_ADAGRAD, oracle.OPT_ADAGRAD) if opt == "adagrad" else (OPT_ADAM, oracle.OPT_ADAM)
    mk = lambda: LookupTable(1 << 17, dim, device=dev, optimizer=kind, max_batch=max(n, keys.size), initial_accumulator=0.1)
    ta, tb = mk(), mk()
    o = oracle.OracleTable(1 << 17, dim, optimizer=okind, initial_accumulator=0.1)
    for t in (ta, tb):
        t.insert(T(keys, dev), T(rows, dev))
        t.set_tuning("apply_kernel", {"auto": -1, "lean": 0, "full": 1}[kernel])
    o.insert(keys, rows)
    bkt = T(bk, dev)
    gen = torch.Generator(device=dev); gen.manual_seed(dim)
    for s in range(3 if kernel == "full" else 2):
        torch.cuda.synchronize()   # (the host sizes step s + 1 by what step s reported: hot keys' buckets exist from the second full step on)
        if exact and dim <= 64:
            g = exact_grads_np(rng, n, dim)
            gt = T(g, dev)
        elif exact:
            gt, g = exact_grads_dev(gen, n, dim, dev)
        elif dim <= 64:
            g = (rng.standard_normal((n, dim)) * 0.01).astype(np.float32)
            gt = T(g, dev)
        else:
            gt = torch.randn(n, dim, device=dev, generator=gen) * 0.01
            g = gt.cpu().numpy()
        _, _, slots = tb.find_located(bkt, prepare_apply=(s == 1))
        if opt == "adagrad":
            ta.apply_adagrad(bkt, gt, lr=0.05); tb.apply_adagrad(bkt, gt, lr=0.05, slots=slots); o.apply_adagrad(bk, g, 0.05, 1e-10)
        else:
            ta.apply_adam(bkt, gt, lr=0.01, step=s + 1); tb.apply_adam(bkt, gt, lr=0.01, step=s + 1, slots=slots)
            o.apply_adam(bk, g, 0.01, 0.9, 0.999, 1e-8, s + 1)
    if exact:
        for t, form in ((ta, "plain"), (tb, "located")):
            assert t.status() == 0
            assert_tables_bit_equal(t, o, f"{case} {kernel} {opt} dim {dim} {form}:")
    else:
        eo = o.export(with_state=True)
        io = np.argsort(eo[0])
        for t in (ta, tb):
            assert t.status() == 0
            e = [x.cpu().numpy() if x is not None else None for x in t.export(with_state=True)]
            it = np.argsort(e[0])
            assert np.array_equal(e[0][it], eo[0][io])
            for x, z in zip(e[1:], eo[1:]):
                if z is not None:
                    np.testing.assert_allclose(x[it], z[io], rtol=RTOL, atol=ATOL)
    # the scratch is left clean: a batch of distinct keys right behind it, bit-exact
    g1 = exact_grads_np(rng, n_bg, dim) if exact else (rng.standard_normal((n_bg, dim)) * 0.02).astype(np.float32)
    if opt == "adagrad":
        ta.apply_adagrad(T(bg, dev), T(g1, dev), lr=0.05); o.apply_adagrad(bg, g1, 0.05, 1e-10)
    else:
        ta.apply_adam(T(bg, dev), T(g1, dev), lr=0.01, step=3); o.apply_adam(bg, g1, 0.01, 0.9, 0.999, 1e-8, 3)
    got, found = ta.find(T(bg, dev))
    exp, _ = o.find(bg)
    assert bool(found.all()) and ta.status() == 0
    if exact:
        assert np.array_equal(got.cpu().numpy(), exp)
        assert_tables_bit_equal(ta, o, f"{case} {kernel} {opt} dim {dim}, the distinct-key batch behind it:")
    else:
        np.testing.assert_allclose(got.cpu().numpy(), exp, rtol=RTOL, atol=ATOL)


# ---- numeric edges (SPEC.md §4 as written), distinct keys, one step ---------------------------------------------------------------------------
EDGE_GRADS = np.array([0.0, -0.0, 1e-45, 1e-40, 1.17549435e-38, 1e-20, 1e19, 1.8446743e19, 2e19, 3e38, -3e38, np.inf, -np.inf, np.nan],
                      dtype=np.float32)                                        # 1e19 .. 2e19: g*g crosses FLT_MAX
EDGE_STATE = np.array([0.0, 1e-41, 0.1, 3e38], dtype=np.float32)              # Adagrad's accumulator, Adam's v
EDGE_WEIGHTS = np.array([0.0, -0.0, 1e-42, 1.0, -1.0, 3.4e38], dtype=np.float32)
EDGE_MOMENT = np.array([0.0, 1e-41, -0.1, 0.5], dtype=np.float32)            # Adam's m (the issue's grid leaves it free)
EDGE_NONFINITE_WEIGHTS = np.array([np.inf, -np.inf, np.nan, -3.4e38], dtype=np.float32)   # the last four rows: one such weight each
EDGE_EPS = (0.0, 1e-10)
EDGE_ADAM_STEPS = (1, 2, 1000, 10 ** 6, 2 ** 31 + 5)   # a large step: the host's 1 - beta^t in fp64 and its cast to fp32
EDGE_KEYS = 132
EDGE_LR = {"adagrad": 0.05, "adam": 0.01}


def edge_runs(opt):
    """the (eps, step) pairs one entry point is run with"""
    return [(eps, 1) for eps in EDGE_EPS] if opt == "adagrad" else [(eps, step) for eps in EDGE_EPS for step in EDGE_ADAM_STEPS]


@functools.lru_cache(maxsize=None)
def edge_inputs(opt, dim):
    """-> (keys, weights, state1, state2 or None, grads), read-only: 132 distinct keys whose elements walk through every combination of
    (gradient, accumulator or v, weight) of the grid, each cycle of the 336 combinations in another seeded order so that a combination meets
    different columns.  The last four rows carry the non-finite weights (and -3.4e38), one value per row."""
    rng = np.random.default_rng(1000 + dim + (0 if opt == "adagrad" else 1))
    total = EDGE_KEYS * dim
    n_combo = EDGE_GRADS.size * EDGE_STATE.size * EDGE_WEIGHTS.size
    combo = np.concatenate([rng.permutation(n_combo) for _ in range(total // n_combo + 1)])[:total].reshape(EDGE_KEYS, dim)
    g = EDGE_GRADS[combo % EDGE_GRADS.size]
    s = EDGE_STATE[(combo // EDGE_GRADS.size) % EDGE_STATE.size]
    w = EDGE_WEIGHTS[combo // (EDGE_GRADS.size * EDGE_STATE.size)].copy()
    w[-4:] = EDGE_NONFINITE_WEIGHTS[:, None]
    keys = synth.keys_np(777, 0, EDGE_KEYS)
    if opt == "adagrad":
        out = (keys, w, s, None, g)
    else:
        out = (keys, w, EDGE_MOMENT[rng.integers(0, EDGE_MOMENT.size, size=(EDGE_KEYS, dim))], s, g)
    for a in out:
        if a is not None:
            a.flags.writeable = False
    return out


@functools.lru_cache(maxsize=None)
def edge_reference(opt, dim, eps, step):
    """the oracle's table after one step on edge_inputs(opt, dim): [keys, values, state planes], sorted by key, read-only; computed once"""
    keys, w, s1, s2, g = edge_inputs(opt, dim)
    o = oracle.OracleTable(512, dim, optimizer=oracle.OPT_ADAGRAD if opt == "adagrad" else oracle.OPT_ADAM)
    o.insert(keys, w)
    assert o.assign_plane(1, keys, s1).all() and (s2 is None or o.assign_plane(2, keys, s2).all())
    if opt == "adagrad":
        o.apply_adagrad(keys, g, EDGE_LR[opt], eps)
    else:
        o.apply_adam(keys, g, EDGE_LR[opt], 0.9, 0.999, eps, step)
    assert o.status() == 0
    e = export_sorted(o)
    for a in e:
        a.flags.writeable = False
    return e


def assert_bits_equal_nan_aware(got, ref, what=""):
    """bitwise equality wherever the reference is a number (the sign of a zero included); where it is NaN, got must be NaN (payload and sign
    of a NaN are not specified)"""
    assert got.shape == ref.shape and got.dtype == ref.dtype == np.float32
    nan = np.isnan(ref)
    bad = np.where(nan, ~np.isnan(got), got.view(np.uint32) != ref.view(np.uint32))
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ from the oracle; the first at {i}: got {got[i]!r} "
                             f"(0x{int(got.view(np.uint32)[i]):08x}), expected {ref[i]!r} (0x{int(ref.view(np.uint32)[i]):08x})")
