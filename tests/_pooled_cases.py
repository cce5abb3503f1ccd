"""Test-only builders of test_pooled_edges.py: the numpy reference of the pooled lookups (SPEC.md §3), the grid of edge values they are run on,
the bags, and the comparisons.

The grid gives every COLUMN of a table a regime (zeros of both signs, only -0.0, subnormals, values around FLT_MIN, ordinary values that cancel, values
whose running sum overflows, +inf among finite values, sparse +-inf and NaN): a uniform mix of such values would overflow most sums of a long bag and
leave hardly a zero.  Every array handed out here is cached and read-only."""
import functools

import numpy as np
import torch

import oracle
from _apply_cases import assert_bits_equal_nan_aware
from meepoembedding_amd import synth

F32 = np.float32
FLT_MIN = F32(1.17549435e-38)
N_ROWS = 1500          # rows of the grid: the keys a table stores (capacity 4096)
CAPACITY = 4096

# ---- the regimes: (values, probabilities) -----------------------------------------------------------------------------------------
_BELOW_MIN = np.nextafter(FLT_MIN, F32(0))
REGIMES = (
    ("zeros", [-0.0, 0.0], [0.75, 0.25]),
    ("minus_zero", [-0.0], [1.0]),
    ("subnormal", [1e-45, -1e-45, 1e-40, -1e-40, 7e-42, 3e-39, -3e-39, 0.0], [0.15, 0.15, 0.15, 0.15, 0.1, 0.1, 0.1, 0.1]),
    ("flt_min", [FLT_MIN, -FLT_MIN, 2 * FLT_MIN, -1.5 * FLT_MIN, _BELOW_MIN, -_BELOW_MIN, 0.75 * FLT_MIN, 3 * FLT_MIN], [0.125] * 8),
    ("cancel", [1.0, -1.0, 0.333, 1e-8, 2.0 ** 24, -(2.0 ** 24 - 1)], [0.2, 0.2, 0.2, 0.2, 0.1, 0.1]),
    ("overflow", [3e38, -3e38, 2e38, -1e38, 1e30], [0.2] * 5),
    ("plus_inf", [np.inf, 1.0, -2.5, 1e10, -1e-3], [0.12, 0.22, 0.22, 0.22, 0.22]),
    ("sparse_nonfinite", [np.inf, -np.inf, np.nan, 0.5, -1.25, 3.0, 1e-3], [0.07, 0.07, 0.06, 0.2, 0.2, 0.2, 0.2]),
)
# per-sample weights: 0 * inf, the overflow of a product (3e38) and its underflow (1e-30) occur
WEIGHTS = np.array([0.0, -0.0, 1.0, -1.0, 0.5, 1e-30, 2.0, 3e38], dtype=F32)
WEIGHT_P = np.array([0.05, 0.04, 0.3, 0.1, 0.2, 0.1, 0.13, 0.08])
_POSITIVE = np.array([w == 0 and not np.signbit(w) or w > 0 for w in WEIGHTS])   # a third of the bags draw from these: a -0.0 column stays -0.0

# ---- the bags ---------------------------------------------------------------------------------------------------------------------
# short average: four bags per wave — a tile per bag, bags of one wave that end at different rounds, bags of kPoolLong = 16 keys or more shared by the
# four tiles, and 102 = 4 * 25 + 2 bags, so the last wave step has two
SHORT_LENS = np.array([0, 1, 2, 3, 15, 16, 17, 40, 5, 0, 7, 1, 3, 9, 2, 14, 16, 1, 0, 31, 4, 4] + [2, 0, 7, 1, 6, 3, 11, 5] * 10)
# long average: a wave per bag; 50, 33, 21, 15 ... are no multiple of 4 * U for any unroll U
LONG_LENS = np.array([12, 15, 16, 17, 33, 64, 50, 13, 21] * 11)
BAG_LISTS = {"short": SHORT_LENS, "long": LONG_LENS}
assert SHORT_LENS.size % 4 == 2 and SHORT_LENS.sum() // SHORT_LENS.size < 12 <= LONG_LENS.sum() // LONG_LENS.size


def frozen(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays if len(arrays) > 1 else arrays[0]


# ---- bf16 by SPEC.md §3 "Output type" -----------------------------------------------------------------------------------------------
def bf16_bits(a: np.ndarray) -> np.ndarray:
    """bf16_bits(x) = (u + 0x7FFF + ((u >> 16) & 1)) >> 16 on the fp32 patterns (what it gives for a NaN is not used by any comparison)"""
    u = np.ascontiguousarray(a, dtype=F32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_round(a: np.ndarray) -> np.ndarray:
    """fp32 -> the nearest bf16, as fp32; a NaN stays a NaN"""
    a = np.ascontiguousarray(a, dtype=F32)
    r = (bf16_bits(a).astype(np.uint32) << 16).view(F32)
    return np.where(np.isnan(a), F32(np.nan), r).astype(F32)


def assert_bf16_bits_equal_nan_aware(got: torch.Tensor, ref_f32: np.ndarray, what=""):
    """got (a bf16 tensor) == the fp32 reference rounded by the integer rule, on the 16-bit patterns, the sign of a zero included; where the
    reference is a NaN, got must be a NaN (which one is not specified)"""
    assert got.dtype == torch.bfloat16, (what, got.dtype)
    g = got.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    assert g.shape == ref_f32.shape, (what, g.shape, ref_f32.shape)
    nan = np.isnan(ref_f32)
    got_nan = (g & 0x7FFF) > 0x7F80
    bad = np.where(nan, ~got_nan, g != bf16_bits(ref_f32).reshape(g.shape))
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} bf16 patterns differ from the reference; the first at {i}: got 0x{int(g[i]):04x}, "
                             f"expected {ref_f32[i]!r} -> 0x{int(bf16_bits(ref_f32).reshape(g.shape)[i]):04x}")


def assert_f32(got: torch.Tensor, ref: np.ndarray, what=""):
    assert got.dtype == torch.float32, (what, got.dtype)
    assert_bits_equal_nan_aware(got.detach().cpu().numpy(), ref, what)


def assert_out(got: torch.Tensor, ref: np.ndarray, what=""):
    (assert_bf16_bits_equal_nan_aware if got.dtype == torch.bfloat16 else assert_f32)(got, ref, what)


# ---- the reference --------------------------------------------------------------------------------------------------------------------
def pool_ref(rows, off, mode="sum", w=None, variant=None):
    """SPEC.md §3 in numpy float32: per bag in position order, the first (weighted) row is COPIED, every further one added, every product and every sum
    rounded once; mean = one division by float32(length); an empty bag is +0.
    variant: None = the specification.  The others are deliberately WRONG bodies that the grid has to tell apart from it (test_grid_has_teeth):
    "zero_start" — the sum starts from +0 and adds the first row too;  "flush" — subnormal inputs and results become zeros;  "reciprocal_mean" — the
    mean multiplies by 1 / length;  "fma" — the weighted row joins the sum through a fused multiply-add (the product is not rounded);  "padding" — a bag is
    walked in rounds of four positions and the positions past its end contribute 0 * row."""
    off = np.asarray(off, np.int64)
    lens = off[1:] - off[:-1]
    rows = np.ascontiguousarray(rows, dtype=F32)
    out = np.zeros((lens.size, rows.shape[1]), F32)
    with np.errstate(all="ignore"):
        if variant == "flush":
            rows = np.where(np.abs(rows) < FLT_MIN, np.copysign(F32(0), rows), rows)
        steps = int(lens.max()) if lens.size else 0
        if variant == "padding":
            steps = -(-steps // 4) * 4
        for s in range(steps):
            m = lens > s
            if variant == "padding":
                m = -(-lens // 4) * 4 > s
            p = np.minimum(off[:-1][m] + s, max(rows.shape[0] - 1, 0))
            wp = None if w is None else w[p][:, None].astype(F32)
            if variant == "padding":
                wp = np.where((lens[m] > s)[:, None], F32(1) if w is None else wp, F32(0)).astype(F32)
            if variant == "fma" and wp is not None:   # the exact product (48 bits fit fp64) joins the sum before any rounding to fp32
                prod = wp.astype(np.float64) * rows[p].astype(np.float64)
                out[m] = prod.astype(F32) if s == 0 else (out[m].astype(np.float64) + prod).astype(F32)
                continue
            r = rows[p] if wp is None else (wp * rows[p]).astype(F32)
            if variant == "zero_start":
                out[m] = (out[m] + r).astype(F32)
            else:
                out[m] = r if s == 0 else (out[m] + r).astype(F32)
        nz = lens > 0
        if mode == "mean" and variant == "reciprocal_mean":
            out[nz] = (out[nz] * (F32(1) / lens[nz, None].astype(F32)).astype(F32)).astype(F32)
        elif mode == "mean":
            out[nz] = (out[nz] / lens[nz, None].astype(F32)).astype(F32)
        if variant == "flush":
            out = np.where(np.abs(out) < FLT_MIN, np.copysign(F32(0), out), out).astype(F32)
    return out


VARIANTS = ("zero_start", "flush", "reciprocal_mean", "fma", "padding")


def combine_ref(partials, run_bag, lens, n_bags, mode):
    """the owners' partial rows of a bag in ascending segment order (= the order of the runs), the first one copied, each further one added in fp32;
    mean divides a bag that has keys and a partial by float32(length); a bag without a partial is +0"""
    out = np.zeros((n_bags, partials.shape[1]), F32)
    seen = np.zeros(n_bags, bool)
    with np.errstate(all="ignore"):
        for r, b in enumerate(run_bag):
            out[b] = partials[r] if not seen[b] else (out[b] + partials[r]).astype(F32)
            seen[b] = True
        if mode == "mean":
            nz = seen & (lens > 0)
            out[nz] = (out[nz] / lens[nz, None].astype(F32)).astype(F32)
    return out


# ---- the grid ---------------------------------------------------------------------------------------------------------------------------
def _regime_values(r, bf16):
    v = np.array(REGIMES[r][1], dtype=F32)
    if bf16:   # the bf16-representable neighbour; a value that would round to zero becomes the smallest bf16 subnormal, 2^-133 = 9.2e-41
        b = bf16_round(v)
        v = np.where((b == 0) & (v != 0), np.copysign(F32(2.0 ** -133), v), b).astype(F32)
    return v


@functools.lru_cache(maxsize=None)
def column_regimes(dim):
    """the regime of every column: the eight cycled over the columns, shuffled with a fixed seed per dim"""
    return frozen(np.random.default_rng(4000 + dim).permutation(np.arange(dim) % len(REGIMES)))


@functools.lru_cache(maxsize=None)
def edge_rows(dim, n_rows=N_ROWS, seed=0, bf16=False):
    """[n_rows, dim] fp32: every element of a column drawn from its regime's short list.  bf16: every value is bf16-representable."""
    rng = np.random.default_rng([dim, n_rows, seed, int(bf16)])
    reg = column_regimes(dim)
    out = np.empty((n_rows, dim), F32)
    for c in range(dim):
        out[:, c] = rng.choice(_regime_values(reg[c], bf16), size=n_rows, p=REGIMES[reg[c]][2])
    return frozen(out)


@functools.lru_cache(maxsize=None)
def stored_keys(seed, count=N_ROWS):
    return frozen(synth.keys_np(77000 + seed, 0, count))


def lookup_ref(keys, skeys, srows, default):
    """find in numpy -> (rows, found): the stored row, the default row for an absent or reserved key"""
    order = np.argsort(skeys)
    sk = skeys[order]
    pos = np.minimum(np.searchsorted(sk, keys), sk.size - 1)
    hit = (sk[pos] == keys) & (keys != oracle.EMPTY_KEY) & (keys != oracle.RECLAIMED_KEY)
    rows = np.where(hit[:, None], srows[order][pos], F32(default)).astype(F32)
    return rows, hit.astype(np.uint8)


class Case:
    """one table's worth of the grid and one batch of bags on it: what is stored (skeys, srows, default), the batch (keys, off, w) and what find gives
    for it in numpy (rows, found)"""

    def ref(self, mode="sum", weighted=False, variant=None):
        return _case_ref(self, mode, weighted, variant)


@functools.lru_cache(maxsize=None)
def _case_ref(case, mode, weighted, variant):
    return frozen(pool_ref(case.rows, case.off, mode, case.w if weighted else None, variant))


@functools.lru_cache(maxsize=None)
def grid_case(dim, which, seed=0, default=-0.0, fill=1.0, bf16=False, exact=False):
    """The grid's rows under distinct keys (only the first `fill` of them stored: the rest are absent) and a batch of the bag list `which` on them: keys
    drawn from the grid with repeats, about one position in sixteen an absent key, EMPTY_KEY or RECLAIMED_KEY.  Forced: the first bag of three keys holds
    (long list: 13) absent keys only, the first bag of 17 starts with an absent key, the first bag of 40 (33) with EMPTY_KEY, the first bag of one
    key holds a stored key.  exact: the rows are exactly summable (exact_rows) instead of edge values."""
    c = Case()
    rng = np.random.default_rng([dim, seed, which == "long", int(bf16), int(exact)])
    lens = BAG_LISTS[which]
    c.dim, c.which, c.default, c.lens = dim, which, F32(default), lens
    c.off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(c.off[-1])
    all_keys = stored_keys(seed)
    all_rows = exact_rows(dim, N_ROWS, seed) if exact else edge_rows(dim, N_ROWS, seed, bf16)
    n_stored = int(N_ROWS * fill)
    c.skeys, c.srows = all_keys[:n_stored], all_rows[:n_stored]
    keys = all_keys[rng.integers(0, N_ROWS, n)].copy()
    absent = synth.keys_np(88000 + seed, 0, n)
    assert not np.isin(absent, all_keys).any()
    special = np.flatnonzero(rng.random(n) < 1 / 16)
    for j, i in enumerate(special):
        keys[i] = (absent[i], oracle.EMPTY_KEY, oracle.RECLAIMED_KEY)[j % 3]
    first = lambda l: int(c.off[np.flatnonzero(lens == l)[0]])  # noqa: E731
    gone = 3 if which == "short" else 13
    keys[first(gone):first(gone) + gone] = absent[:gone]
    keys[first(17)] = absent[gone]
    keys[first(40 if which == "short" else 33)] = oracle.EMPTY_KEY
    if which == "short":   # ... one whose row holds a NaN and a subnormal, where the grid has such a row
        with np.errstate(all="ignore"):
            rich = np.isnan(c.srows).any(1) & ((np.abs(c.srows) < FLT_MIN) & (c.srows != 0)).any(1)
        keys[first(1)] = c.skeys[int(np.argmax(rich)) if rich.any() else 5]
    c.keys = keys
    # weights: a third of the bags draw from the weights of positive sign only
    positive_bag = np.repeat(rng.random(lens.size) < 1 / 3, lens)
    w_all = rng.choice(WEIGHTS, size=n, p=WEIGHT_P)
    w_pos = rng.choice(WEIGHTS[_POSITIVE], size=n, p=WEIGHT_P[_POSITIVE] / WEIGHT_P[_POSITIVE].sum())
    c.w = np.where(positive_bag, w_pos, w_all).astype(F32)
    c.rows, c.found = lookup_ref(keys, c.skeys, c.srows, c.default)
    c.all_absent_bag = int(np.flatnonzero(lens == gone)[0])
    c.one_key_bag = int(np.flatnonzero(lens == 1)[0]) if which == "short" else None
    frozen(c.off, c.keys, c.w, c.rows, c.found)
    return c


# ---- classes of fp32 values ---------------------------------------------------------------------------------------------------------
def class_shares(a):
    """the share of +0, -0, subnormal, normal, +-inf and NaN elements of an fp32 array"""
    a = np.ascontiguousarray(a, dtype=F32)
    zero, neg = a == 0, np.signbit(a)
    with np.errstate(all="ignore"):
        sub = (np.abs(a) < FLT_MIN) & ~zero
        normal = np.isfinite(a) & (np.abs(a) >= FLT_MIN)
    return {"+0": float((zero & ~neg).mean()), "-0": float((zero & neg).mean()), "subnormal": float(sub.mean()), "normal": float(normal.mean()),
            "inf": float(np.isinf(a).mean()), "nan": float(np.isnan(a).mean())}


# ---- exactly summable rows and bag grads (weight_grads bit for bit) ---------------------------------------------------------------------
EXACT_M = 31                       # |m| <= 31, odd
EXACT_EXPONENTS = (0, -8, -16)     # a product is (m1 m2) 2^(e1 + e2): below 2^10, a multiple of 2^-32; the sum of up to 128 of them stays below 2^17
EXACT_MAX_DIM = 128                # 17 + 32 = 49 bits: exact in fp64 in every order and every grouping, while 24 bits do not hold it
EXACT_DEFAULT = 3 * 2.0 ** -8      # the default row of the tables is of the same form


def _exact_draw(rng, shape):
    m = (2 * rng.integers(0, (EXACT_M + 1) // 2, size=shape) + 1) * rng.choice([-1, 1], size=shape)
    e = np.asarray(EXACT_EXPONENTS)[rng.integers(0, len(EXACT_EXPONENTS), size=shape)]
    return np.ldexp(m.astype(F32), e).astype(F32)


@functools.lru_cache(maxsize=None)
def exact_rows(dim, n_rows=N_ROWS, seed=0):
    assert dim <= EXACT_MAX_DIM
    return frozen(_exact_draw(np.random.default_rng([7, dim, n_rows, seed]), (n_rows, dim)))


@functools.lru_cache(maxsize=None)
def exact_bag_grads(dim, n_bags, seed=0):
    assert dim <= EXACT_MAX_DIM
    return frozen(_exact_draw(np.random.default_rng([8, dim, n_bags, seed]), (n_bags, dim)))


def bag_of_positions(off):
    return np.repeat(np.arange(off.size - 1), off[1:] - off[:-1])


def weight_grads_ref(bag_grads, rows, off):
    """-> (the fp64 sum of the fp64 products per position, sum of |products|)"""
    with np.errstate(all="ignore"):
        prod = bag_grads[bag_of_positions(off)].astype(np.float64) * rows.astype(np.float64)
        return prod.sum(1), np.abs(prod).sum(1)


def assert_weight_grads_in_spec(got, bag_grads, rows, off, what=""):
    """SPEC.md §3: products and sum in fp64, rounded once to fp32.  Where the fp64 sum is a NaN, a NaN; where it is +-inf, or finite and beyond the
    largest fp32 (its rounding is the same inf), exactly that; otherwise within 1e-6 * sum |products| of it."""
    ref, mag = weight_grads_ref(bag_grads, rows, off)
    with np.errstate(all="ignore"):
        ref32 = ref.astype(F32)
    nan, inf = np.isnan(ref), np.isinf(ref32)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN positions differ"
    assert np.array_equal(got[inf], ref32[inf]), f"{what}: infinities differ"
    fin = ~nan & ~inf
    with np.errstate(all="ignore"):
        err = np.abs(got[fin].astype(np.float64) - ref[fin])
    bad = ~(err <= 1e-6 * mag[fin] + 1e-30)
    assert not bad.any(), f"{what}: {int(bad.sum())} weight grads beyond 1e-6 * sum |products| (largest error {err[bad].max():.3g})"
