"""The pooled lookups (embedding bags) bit for bit on signed zeros, subnormals, overflow, infinities and NaN (SPEC.md §3): the first row of a bag
is copied, every further one added as acc = acc + row, a weighted row is w * row rounded before the add (no fma), mean is one IEEE division by
(float)length, an empty bag is +0, a bf16 result rounds the finished row once.

The reference is ONE numpy restatement of that (_pooled_cases.pool_ref), run on a grid whose columns each follow a regime of edge values, and every
comparison is on the raw bits, the sign of a zero included; where the reference is a NaN the result must be a NaN (which one is not specified).
The CPU half checks the reference against oracle.pool_rows, that its output holds every class of value, that the grid tells deliberately wrong
bodies from the right one, and — with integers — that the inputs of the bit-exact weight_grads test are exactly summable.
The GPU half runs every body that holds the "first row" logic: the shared pooled_bags walk (table, weighted, tiered, bf16-row, jagged, mixed, a wave
per bag), the uniform group's own four-bags-per-wave copy, combine_bag_runs, and the weighted backward."""
import numpy as np
import pytest
import torch

import oracle
import _pooled_cases as P
from _apply_cases import assert_bits_equal_nan_aware
from _pooled_cases import assert_f32, assert_out, grid_case

BF16 = torch.bfloat16
DIMS = [64, 128, 24, 100, 260]          # 64 and 128: instances of their own; 24, 100, 260: the run-time width (partial chunk, ragged second chunk, > 4 chunks)
BROW_DIMS = [64, 128, 40, 104]
EXACT_DIMS = [64, 128, 24, 100]
LISTS = ("short", "long")
SUBNORMAL_DEFAULT = float(np.float32(1e-40))
BROW_SUBNORMAL_DEFAULT = float(P.bf16_round(np.array([1e-40], np.float32))[0])
MEMBER_DEFAULTS = (SUBNORMAL_DEFAULT, -0.0, 0.25)
MEMBER_FILL = (1.0, 0.5, 1.0)           # the second member stores half of its grid: the other half reads its default row, -0.0 (a long bag of
                                        # such a member always holds an absent key: with another default no -0.0 column would survive)


def T(a, dev):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).to(dev)


def cat_cases(cases):
    """the batch of a group: the members' batches one after the other -> (keys, bag offsets, weights)"""
    keys = np.concatenate([c.keys for c in cases])
    w = np.concatenate([c.w for c in cases])
    base = np.concatenate([[0], np.cumsum([c.keys.size for c in cases])])
    off = np.concatenate([c.off[:-1] + b for c, b in zip(cases, base)] + [[base[-1]]]).astype(np.int64)
    return keys, off, w


# ---- CPU: the reference, the grid, its teeth --------------------------------------------------------------------------------------------
ALL_MODES, PLAIN_MODES = (("sum", False), ("mean", False), ("sum", True)), (("sum", False), ("mean", False))
MIXED_DIMS, MIXED_DEFAULTS = (64, 128, 24, 100), (SUBNORMAL_DEFAULT, -0.0, 0.25, -0.0)


def member_cases(dim, which, bf16=False):
    """the three members of a group: different default rows, the second one stores only half of its grid"""
    defaults = MEMBER_DEFAULTS if not bf16 else (BROW_SUBNORMAL_DEFAULT, -0.0, 0.25)
    return [grid_case(dim, which, j, defaults[j], MEMBER_FILL[j], bf16) for j in range(3)]


def mixed_cases(which):
    return [grid_case(d, which, j, MIXED_DEFAULTS[j], 0.5 if j == 3 else 1.0) for j, d in enumerate(MIXED_DIMS)]


def gpu_cases():
    """every (case, modes) whose reference a GPU test compares with: single tables at both defaults, the members of the groups, bf16 rows (unweighted)"""
    seen = set()
    for which in LISTS:
        for dim in DIMS:
            for c in [grid_case(dim, which, 0, -0.0)] + member_cases(dim, which):
                yield c, ALL_MODES
        for c in mixed_cases(which):
            if id(c) not in seen:
                yield c, PLAIN_MODES
            seen.add(id(c))
        for dim in BROW_DIMS:
            for c in member_cases(dim, which, True):
                yield c, PLAIN_MODES


def test_reference_is_the_oracles_pool_rows():
    """the numpy reference == oracle.pool_rows bit for bit on the grid (unweighted: the oracle has no weights)"""
    for c, _ in gpu_cases():
        for mode in ("sum", "mean"):
            with np.errstate(all="ignore"):
                want = oracle.pool_rows(c.rows, c.off, mode)
            assert_bits_equal_nan_aware(c.ref(mode), want, f"dim {c.dim} {c.which} {mode}")


def test_bf16_rule_is_torchs_cast():
    """the integer rule of SPEC.md §3 on every value of the grid and on reference outputs == torch's CPU cast (NaN aside)"""
    c = grid_case(64, "short")
    for a in (c.srows, c.ref("sum"), c.ref("mean"), c.ref("sum", True)):
        ok = ~np.isnan(a)
        want = torch.from_numpy(a.copy()).to(BF16).view(torch.int16).numpy().view(np.uint16)
        assert np.array_equal(P.bf16_bits(a)[ok], want[ok])
    b = grid_case(64, "short", 0, -0.0, 1.0, True).srows
    assert_bits_equal_nan_aware(P.bf16_round(b), b, "the bf16 grid is bf16-representable")
    nz = b[(b != 0) & ~np.isnan(b)]
    assert np.abs(nz).min() >= 9.18e-41 and (np.abs(nz) < P.FLT_MIN).any()


def test_edge_grid_reference():
    """Conditions on the INPUTS, checked on the reference output alone: every class of value makes up at least 0.2 % of the elements of every reference
    a GPU test uses and NaN less than half — and SPEC.md §3's sentences hold in the reference itself."""
    for c, modes in gpu_cases():
        for mode, weighted in modes:
            ref = c.ref(mode, weighted)
            shares = P.class_shares(ref)
            what = f"dim {c.dim} {c.which} default {c.default!r} {mode}{' weighted' if weighted else ''}: {shares}"
            assert min(shares.values()) >= 0.002 and shares["nan"] < 0.5, what
            empty = c.lens == 0
            assert not ref[empty].view(np.uint32).any(), f"{what}: an empty bag is +0"
            if weighted:
                continue
            cols = np.flatnonzero(P.column_regimes(c.dim) == 1)       # the -0.0 columns: -0.0 wherever every row of the bag holds it
            all_minus = np.array([l > 0 and (c.rows[a:a + l][:, cols].view(np.uint32) == 0x80000000).all() for a, l in zip(c.off[:-1], c.lens)])
            assert all_minus.sum() >= 10
            assert (ref[np.ix_(all_minus, cols)].view(np.uint32) == 0x80000000).all(), f"{what}: a bag of -0.0 is -0.0"
            if np.signbit(c.default):
                assert (ref[c.all_absent_bag].view(np.uint32) == 0x80000000).all(), f"{what}: a bag of absent keys on a -0.0 default"
            if c.one_key_bag is not None:   # (x / 1.0f is x: the mean too)
                row = c.rows[c.off[c.one_key_bag]]
                assert np.isnan(row).any() and ((np.abs(row) < P.FLT_MIN) & (row != 0)).any()
                assert_bits_equal_nan_aware(ref[c.one_key_bag], row, f"{what}: a bag of one key is its row's bits")


@pytest.mark.parametrize("variant", P.VARIANTS)
def test_grid_has_teeth(variant):
    """each deliberately wrong body differs from the reference in at least one element, for every dim and bag list it applies to"""
    for c, modes in gpu_cases():
        hit = False
        for mode, weighted in modes:
            if (variant == "fma" and not weighted) or (variant == "reciprocal_mean" and mode != "mean"):
                continue
            hit = True
            ref, wrong = c.ref(mode, weighted), c.ref(mode, weighted, variant)
            differ = np.where(np.isnan(ref), ~np.isnan(wrong), ref.view(np.uint32) != wrong.view(np.uint32))
            assert differ.any(), f"the grid does not tell the wrong body '{variant}' from the reference: dim {c.dim} {c.which} {mode} weighted={weighted}"
        assert hit or variant == "fma"   # (bf16 rows have no weighted bags)


def backward_cases(dim, which, exact):
    """the three members of the backward tests: edge rows at the members' defaults, or exactly summable rows (the second member half empty in both)"""
    if exact:
        return [grid_case(dim, which, j, P.EXACT_DEFAULT, MEMBER_FILL[j], False, True) for j in range(3)]
    return [grid_case(dim, which, j, MEMBER_DEFAULTS[j], MEMBER_FILL[j]) for j in range(3)]


def exact_backward_inputs(dim, which):
    """(find's rows per position, bag offsets, bag grads) of the exact backward test: the first member alone, then the group"""
    cases = backward_cases(dim, which, True)
    n_bags = cases[0].lens.size
    yield cases[0].rows, cases[0].off, P.exact_bag_grads(dim, n_bags, 0)
    yield np.concatenate([c.rows for c in cases]), cat_cases(cases)[1], P.exact_bag_grads(dim, 3 * n_bags, 1)


@pytest.mark.parametrize("dim", EXACT_DIMS)
def test_exact_weight_grad_inputs_are_exactly_summable(dim):
    """The proof, in integers, that test_weight_grads_bit_for_bit's inputs leave weight_grads no freedom: every row element and every bag grad is
    m * 2^e with odd |m| <= 31 and e in {0, -8, -16}, so in units of 2^-32 every product is an integer and the sum of the |products| of a position
    stays below 2^53 — every partial sum, in any order and any grouping, is an integer below 2^53 in those units: exact in fp64.  The rounding to fp32
    is a real one: a good share of the sums needs more than 24 significant bits, and a sequential fp32 accumulation of the same products misses the
    reference.  (Dims up to 128 only: at 260 the same budget would leave fewer exponents; the wide run-time widths are covered by 100.)"""
    for which in LISTS:
        for rows, off, bg in exact_backward_inputs(dim, which):      # what the GPU test feeds the table, then the group
            for a in (rows, bg):
                scaled = np.ldexp(a.astype(np.float64), 16)
                ints = scaled.astype(np.int64)
                assert np.array_equal(ints, scaled) and (ints % 2 != 0).any() and int(np.abs(ints).max()) <= P.EXACT_M << 16
            ri = np.ldexp(rows.astype(np.float64), 16).astype(np.int64).astype(object)     # Python integers from here on
            gi = np.ldexp(bg.astype(np.float64), 16).astype(np.int64).astype(object)[P.bag_of_positions(off)]
            prod = ri * gi
            assert all(isinstance(x, int) for x in prod[0])
            assert max(int(sum(abs(x) for x in p)) for p in prod) < 1 << 53
            sums = [int(sum(p)) for p in prod]
            ref, _ = P.weight_grads_ref(bg, rows, off)
            assert all(float(s) * 2.0 ** -32 == r for s, r in zip(sums, ref))                # numpy's fp64 sum is that exact value
            wide = np.mean([len(bin(abs(s)).rstrip("0")) - 2 > 24 for s in sums if s])
            assert wide >= 0.25, f"only {wide:.0%} of the sums need more than 24 bits"
            seq = np.zeros(prod.shape[0], np.float32)
            p32 = (bg[P.bag_of_positions(off)] * rows).astype(np.float32)                    # (a product has at most 10 bits: exact in fp32)
            for j in range(dim):
                seq = (seq + p32[:, j]).astype(np.float32)
            assert (seq.view(np.uint32) != ref.astype(np.float32).view(np.uint32)).any(), f"dim {dim} {which}: an fp32 accumulation would pass"


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
def make_table(dev, c, **kw):
    from meepoembedding_amd import LookupTable
    t = LookupTable(P.CAPACITY, c.dim, device=dev, max_batch=1 << 14, default_value=float(c.default), **kw)
    t.insert(T(c.skeys, dev), T(c.srows, dev))
    assert t.status() == 0 and t.size() == c.skeys.size
    return t


def check_found(found, c_found, what):
    assert np.array_equal(found.cpu().numpy(), c_found), f"{what}: found mask"


@pytest.mark.gpu
@pytest.mark.parametrize("dim", DIMS)
def test_table_find_pooled_on_the_grid(dev, dim):
    """LookupTable.find_pooled — the shared walk, a tile per bag (short list) and a wave per bag (long list): sum, mean and weighted, fp32 and bf16"""
    for default in (-0.0, SUBNORMAL_DEFAULT):
        t = make_table(dev, grid_case(dim, "short", 0, default))
        for which in LISTS:
            c = grid_case(dim, which, 0, default)
            k, f, w = T(c.keys, dev), T(c.off, dev), T(c.w, dev)
            what = f"dim {dim} {which} default {default!r}"
            for dt in (torch.float32, BF16):
                for mode in ("sum", "mean"):
                    out, found = t.find_pooled(k, f, mode, out_dtype=dt)
                    assert_out(out, c.ref(mode), f"{what} {mode} {dt}")
                    check_found(found, c.found, what)
                loc = torch.full((c.keys.size,), -7, dtype=torch.int64, device=dev)
                out, found = t.find_pooled(k, f, weights=w, located=loc, out_dtype=dt)
                assert_out(out, c.ref("sum", True), f"{what} weighted {dt}")
                check_found(found, c.found, what)
                assert torch.equal(loc >= 0, found.bool()), f"{what}: located handles"
                ones, _ = t.find_pooled(k, f, weights=torch.ones(c.keys.size, device=dev), out_dtype=dt)
                assert_out(ones, c.ref("sum"), f"{what} all weights 1.0 {dt}")
            if np.signbit(c.default):
                out, _ = t.find_pooled(k, f, "mean")
                assert bool((out[c.all_absent_bag].view(torch.int32) == -(1 << 31)).all()), f"{what}: a bag of absent keys keeps the default's sign"
        assert t.status() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("dim", DIMS)
def test_group_find_pooled_on_the_grid(dev, dim):
    """TableGroup.find_pooled over three members with different default rows, one of them half empty, each member against the reference.  The short
    list runs the uniform group's OWN four-bags-per-wave copy of the walk, the long list the shared one; then the jagged map, both shapes."""
    from meepoembedding_amd import TableGroup
    tables = [make_table(dev, c) for c in member_cases(dim, "short")]
    grp = TableGroup(tables, max_apply_batch=1 << 14)
    nb = {w: P.BAG_LISTS[w].size for w in LISTS}
    for which in LISTS:
        cases = member_cases(dim, which)
        keys, off, w = cat_cases(cases)
        k, f, wt = T(keys, dev), T(off, dev), T(w, dev)
        B = nb[which]
        found_ref = np.concatenate([c.found for c in cases])
        for dt in (torch.float32, BF16):
            results = [(mode, False, grp.find_pooled(k, f, mode, out_dtype=dt)) for mode in ("sum", "mean")]
            loc = torch.empty(keys.size, dtype=torch.int64, device=dev)
            results.append(("sum", True, grp.find_pooled(k, f, weights=wt, located=loc, out_dtype=dt)))
            for mode, weighted, (out, found) in results:
                check_found(found, found_ref, f"group dim {dim} {which}")
                for j, c in enumerate(cases):
                    assert_out(out[j * B:(j + 1) * B], c.ref(mode, weighted), f"group dim {dim} {which} {mode} weighted={weighted} {dt} member {j}")
            ones, _ = grp.find_pooled(k, f, weights=torch.ones(keys.size, device=dev), out_dtype=dt)
            for j, c in enumerate(cases):
                assert_out(ones[j * B:(j + 1) * B], c.ref("sum"), f"group dim {dim} {which} all weights 1.0 {dt} member {j}")
    # jagged: (a) member 0 has no bags, member 1 all the long bags, member 2 the short list — a wave per bag;  (b) the short list for members 0
    # and 2, none for member 1 — four bags per wave, the group's own copy of the walk
    short, long_ = member_cases(dim, "short"), member_cases(dim, "long")
    for name, picked in (("a", [None, long_[1], short[2]]), ("b", [short[0], None, short[2]])):
        used = [c for c in picked if c is not None]
        keys, off, _ = cat_cases(used)
        mb = np.concatenate([[0], np.cumsum([0 if c is None else c.lens.size for c in picked])]).astype(np.int64)
        assert (keys.size // (off.size - 1) >= 12) == (name == "a")
        for mode in ("sum", "mean"):
            out, found = grp.find_pooled_jagged(T(keys, dev), T(off, dev), T(mb, dev), mode)
            check_found(found, np.concatenate([c.found for c in used]), f"jagged {name}")
            for j, c in enumerate(picked):
                if c is not None:
                    assert_f32(out[mb[j]:mb[j + 1]], c.ref(mode), f"jagged ({name}) dim {dim} {mode} member {j}")
    assert all(t.status() == 0 for t in tables)
    grp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("which", LISTS)
def test_mixed_group_find_pooled_on_the_grid(dev, which):
    """MixedTableGroup.find_pooled: members of dims 64, 128, 24 and 100 in one launch, fp32 and bf16, each member's view against the reference"""
    from meepoembedding_amd import MixedTableGroup
    cases = mixed_cases(which)
    tables = [make_table(dev, c) for c in cases]
    grp = MixedTableGroup(tables)
    keys, off, _ = cat_cases(cases)
    for dt in (torch.float32, BF16):
        for mode in ("sum", "mean"):
            views, found = grp.find_pooled(T(keys, dev), T(off, dev), mode, out_dtype=dt)
            check_found(found, np.concatenate([c.found for c in cases]), f"mixed {which}")
            for j, c in enumerate(cases):
                assert_out(views[j], c.ref(mode), f"mixed {which} {mode} {dt} member {j} (dim {c.dim})")
    grp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dim", DIMS)
def test_tiered_find_pooled_on_the_grid(dev, dim):
    """TieredLookupTable.find_pooled: the grid's keys split between a hot table in HBM and a cold one in pinned host memory, so a bag's positions
    alternate tiers; the absent row is the HOT table's -0.0 default (the cold table's 0.25 never shows)"""
    from meepoembedding_amd import LookupTable, _lib
    from meepoembedding_amd.tiered import TieredLookupTable
    c0 = grid_case(dim, "short", 0, -0.0)
    hot = LookupTable(P.CAPACITY, dim, device=dev, max_batch=1 << 14, default_value=-0.0)
    cold = LookupTable(P.CAPACITY, dim, device=dev, max_batch=1 << 14, default_value=0.25, value_memory=_lib.MEM_HOST_PINNED)
    hot.insert(T(c0.skeys[0::2], dev), T(c0.srows[0::2], dev))
    cold.insert(T(c0.skeys[1::2], dev), T(c0.srows[1::2], dev))
    pair = TieredLookupTable(hot, cold)
    for which in LISTS:
        c = grid_case(dim, which, 0, -0.0)
        for dt in (torch.float32, BF16):
            for mode in ("sum", "mean"):
                out, found = pair.find_pooled(T(c.keys, dev), T(c.off, dev), mode, out_dtype=dt)
                assert_out(out, c.ref(mode), f"tiered dim {dim} {which} {mode} {dt}")
                check_found(found, c.found, f"tiered dim {dim} {which}")
    assert hot.status() == 0 and cold.status() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("dim", BROW_DIMS)
def test_bf16_row_find_pooled_on_the_grid(dev, dim):
    """bf16-row tables and a bf16-row group: the same regimes in bf16-representable values (stored verbatim, widened exactly), accumulated in fp32"""
    from meepoembedding_amd import TableGroup
    tables = [make_table(dev, c, value_dtype=BF16) for c in member_cases(dim, "short", True)]
    grp = TableGroup(tables)
    for which in LISTS:
        cases = member_cases(dim, which, True)
        B = cases[0].lens.size
        keys, off, _ = cat_cases(cases)
        for dt in (torch.float32, BF16):
            for mode in ("sum", "mean"):
                for j in (0, 1):
                    out, found = tables[j].find_pooled(T(cases[j].keys, dev), T(cases[j].off, dev), mode, out_dtype=dt)
                    assert_out(out, cases[j].ref(mode), f"bf16 rows dim {dim} {which} {mode} {dt} table {j}")
                    check_found(found, cases[j].found, f"bf16 rows dim {dim} {which}")
                out, found = grp.find_pooled(T(keys, dev), T(off, dev), mode, out_dtype=dt)
                check_found(found, np.concatenate([c.found for c in cases]), f"bf16-row group dim {dim} {which}")
                for j, c in enumerate(cases):
                    assert_out(out[j * B:(j + 1) * B], c.ref(mode), f"bf16-row group dim {dim} {which} {mode} {dt} member {j}")
    grp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("G", [1, 5, 20])
def test_combine_bag_runs_on_the_grid(dev, dim, G):
    """Router.combine_bag_runs alone: partial rows from the grid; bags with no, one and several partials; the mean of a bag whose only partial is all
    -0.0 (-0.0 / length = -0.0); a bag that has keys but no partial stays +0.  Against a numpy loop in ascending segment order, the first partial copied."""
    from meepoembedding_amd import Router
    rng = np.random.default_rng([dim, G])
    n_bags = 90
    lens = rng.choice([0, 1, 2, 3, 7, 40], size=n_bags)
    lens[:3] = (0, 5, 4)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    # which segments hold a run of bag b: none for an empty bag (and for bag 1, which has keys), one for bag 2, up to min(G, length) otherwise
    runs = []
    for p in range(G):
        for b in range(n_bags):
            want = lens[b] > 0 and b != 1 and (rng.random() < 0.5 or (p == G - 1 and not any(rb == b for _, rb in runs)))
            if b == 2:
                want = p == G // 2
            if want:
                runs.append((p, b))
    run_bag = np.array([b for _, b in runs], dtype=np.int32)
    run_counts = np.bincount([p for p, _ in runs], minlength=G).astype(np.int64)
    counts = np.bincount(run_bag, minlength=n_bags)
    assert counts[0] == counts[1] == 0 and counts[2] == 1 and (counts[lens > 0][2:] >= 1).all() and (G == 1 or counts.max() > 1)
    partials = P.edge_rows(dim, len(runs), 50 + G).copy()
    partials[np.flatnonzero(run_bag == 2)[0]] = -0.0
    r = Router(G, 8192, device=dev)
    for mode in ("sum", "mean"):
        ref = P.combine_ref(partials, run_bag, lens, n_bags, mode)
        assert (ref[2].view(np.uint32) == 0x80000000).all() and not ref[:2].view(np.uint32).any()
        for dt in (torch.float32, BF16):
            out = r.combine_bag_runs(T(partials, dev), T(run_bag, dev), T(run_counts, dev), T(off, dev), mode, out_dtype=dt)
            assert_out(out, ref, f"combine_bag_runs dim {dim} G {G} {mode} {dt}")
    r.close()


def backward_checks(t, rows, bg, keys, off, w, loc, dev, what, exact):
    """grads bit for bit, weight_grads by SPEC.md §3 (or, exact inputs, bit for bit), through the forward's handles and by probing"""
    bag = P.bag_of_positions(off)
    with np.errstate(all="ignore"):
        grads_ref = (w[:, None] * bg[bag]).astype(np.float32)
    for name, located in (("probing", None), ("located", loc)):
        g, wg = t.pooled_weighted_backward(T(keys, dev), T(off, dev), T(w, dev), T(bg, dev), located=located)
        assert_f32(g, grads_ref, f"{what} grads {name}")
        wg = wg.cpu().numpy()
        if exact:
            ref, _ = P.weight_grads_ref(bg, rows, off)
            assert_bits_equal_nan_aware(wg, ref.astype(np.float32), f"{what} weight_grads {name}")
        else:
            P.assert_weight_grads_in_spec(wg, bg, rows, off, f"{what} weight_grads {name}")


def run_backward(dev, dim, exact):
    from meepoembedding_amd import TableGroup
    tables = [make_table(dev, c) for c in backward_cases(dim, "short", exact)]
    grp = TableGroup(tables, max_apply_batch=1 << 14)
    for which in LISTS:
        cases = backward_cases(dim, which, exact)
        n_bags = cases[0].lens.size
        draw = P.exact_bag_grads if exact else (lambda d, n, s: P.edge_rows(d, n, 900 + s))
        # one table
        c = cases[0]
        bg = draw(dim, n_bags, 0)
        loc = torch.empty(c.keys.size, dtype=torch.int64, device=dev)
        tables[0].find_pooled(T(c.keys, dev), T(c.off, dev), weights=T(c.w, dev), located=loc)
        backward_checks(tables[0], c.rows, bg, c.keys, c.off, c.w, loc, dev, f"table dim {dim} {which}", exact)
        # the group
        keys, off, w = cat_cases(cases)
        rows = np.concatenate([c.rows for c in cases])
        bg = draw(dim, 3 * n_bags, 1)
        loc = torch.empty(keys.size, dtype=torch.int64, device=dev)
        grp.find_pooled(T(keys, dev), T(off, dev), weights=T(w, dev), located=loc)
        backward_checks(grp, rows, bg, keys, off, w, loc, dev, f"group dim {dim} {which}", exact)
    grp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dim", DIMS)
def test_weighted_backward_on_the_grid(dev, dim):
    """pooled_weighted_backward of a table and of a group on edge rows, edge weights and bag grads drawn from the regimes: grads = w * bag_grad is one
    fp32 multiply, bit for bit; weight_grads is NaN / the same inf where the fp64 sum is, otherwise within the SPEC bound"""
    run_backward(dev, dim, exact=False)


@pytest.mark.gpu
@pytest.mark.parametrize("dim", EXACT_DIMS)
def test_weight_grads_bit_for_bit(dev, dim):
    """weight_grads == float32(fp64 sum) BITWISE on exactly summable rows and bag grads (test_exact_weight_grad_inputs_are_exactly_summable proves
    they are): an fp32 accumulation, which the SPEC bound lets through at these dims, fails here.  Table and group, located and probing, both lists."""
    run_backward(dev, dim, exact=True)
