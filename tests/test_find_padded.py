"""The padded sequence lookup on the GPU (SPEC.md §3 "find_padded"): mee_find_padded_as / mee_group_find_padded_as, LookupTable.find_padded,
TableGroup.find_padded and nn.DynamicEmbeddingSequence.  The expectation is always the in-repo oracle holding the same pairs plus the numpy loop
of tests/_padded_cases.py, never the library's own find.  Outputs are pre-filled — `out` with NaN, the others with byte patterns — so that an
element the call should have written and did not, or one it should have left alone and did not, shows."""

import numpy as np
import pytest
import torch

import oracle
from _apply_cases import T, assert_tables_bit_equal, export_sorted
from _padded_cases import EMPTY, FOUND_SENTINEL, I64_SENTINEL, RECLAIMED, U32_SENTINEL, bf16_bits, expected_padded, spans
from meepoembedding_amd import OPT_ADAGRAD, OPT_ADAM, LookupTable, MeepoError, TableGroup, _lib, synth

BF16 = torch.bfloat16
DEFAULT = 0.375
LENS = [33, 0, 17, 1, 16, 2, 15, 0, 5]   # 16 = kPoolLong; the first n_bags of them make a batch


def rnd(x):
    """fp32 -> what a bf16-row table stores, as fp32 (torch's CPU cast: round to nearest even)"""
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(BF16).to(torch.float32).numpy()


class Outs:
    """the outputs of one raw call, pre-filled"""
    def __init__(self, dev, n, n_bags, L, dim, dtype=torch.float32, out=None):
        self.out = torch.full((n_bags, L, dim), float("nan"), dtype=dtype, device=dev) if out is None else out
        self.found = torch.full((n,), FOUND_SENTINEL, dtype=torch.uint8, device=dev)
        self.lengths = torch.full((n_bags,), I64_SENTINEL, dtype=torch.int64, device=dev)
        self.step_keys = torch.full((n,), I64_SENTINEL, dtype=torch.int64, device=dev)
        self.grad_index = torch.full((n,), U32_SENTINEL, dtype=torch.int32, device=dev)   # (uint32 to the library; the pattern is positive)

    def untouched(self):
        o = self.out.float()
        return bool(torch.isnan(o).all()) and bool((self.found == FOUND_SENTINEL).all()) and bool((self.lengths == I64_SENTINEL).all()) \
            and bool((self.step_keys == I64_SENTINEL).all()) and bool((self.grad_index == U32_SENTINEL).all())


def raw(handle, keys_t, off_t, bags_arg, L, keep, o, dev, group=False, **nulls):
    """the C entry point on pre-filled outputs -> its return code.  nulls: names of arguments to pass as NULL"""
    fn = _lib.lib().mee_group_find_padded_as if group else _lib.lib().mee_find_padded_as
    p = lambda name, t: None if nulls.get(name) else t.data_ptr()
    return fn(handle, p("keys", keys_t), keys_t.numel(), p("off", off_t), bags_arg, L, {"first": 0, "last": 1}.get(keep, keep), p("out", o.out),
              nulls.get("dtype", _lib.DTYPE_BF16 if o.out.dtype == BF16 else _lib.DTYPE_F32), p("found", o.found), p("lengths", o.lengths),
              p("step_keys", o.step_keys), p("grad_index", o.grad_index), torch.cuda.current_stream(dev).cuda_stream)


def check_all(o, exp, what, bf16=False):
    eo, ef, el, ek, eg = exp
    if bf16:
        assert np.array_equal(o.out.cpu().view(torch.int16).numpy().view(np.uint16), bf16_bits(eo)), f"{what}: out (bf16 bits)"
    else:
        assert np.array_equal(o.out.cpu().numpy().view(np.uint32), eo.view(np.uint32)), f"{what}: out (every element, the padding's +0 bits too)"
    assert np.array_equal(o.found.cpu().numpy(), ef), f"{what}: found"
    assert np.array_equal(o.lengths.cpu().numpy(), el), f"{what}: lengths"
    assert np.array_equal(o.step_keys.cpu().numpy(), ek), f"{what}: step_keys"
    assert np.array_equal(o.grad_index.cpu().numpy().view(np.uint32), eg), f"{what}: grad_index"


def make_table(dev, dim, seed=2, default=DEFAULT, n_stored=600, bf16_rows=False, **opts):
    """a table of n_stored key-derived rows and its oracle twin -> (table, oracle, stored keys)"""
    u = synth.keys_np(77, 0, n_stored)
    rows = synth.rows_np(u, dim, seed)
    t = LookupTable(2048, dim, device=dev, max_batch=8192, default_value=default, value_dtype=BF16 if bf16_rows else torch.float32, **opts)
    oo = {k: v for k, v in opts.items() if k != "value_memory"}
    o = oracle.OracleTable(2048, dim, default_value=float(rnd([default])[0]) if bf16_rows else default, **oo)
    t.insert(T(u, dev), T(rows, dev))
    o.insert(u, rnd(rows) if bf16_rows else rows)
    return t, o, u


def make_batch(rng, stored, lens, lead=0, trail=0):
    """keys for bags of the given lengths (with `lead` / `trail` positions in no bag): stored keys, absent keys, EMPTY and RECLAIMED, drawn from a
    small pool so that keys repeat inside and across bags -> (keys, offsets)"""
    pool = np.concatenate([stored[:40], synth.keys_np(991, 0, 12), [EMPTY, RECLAIMED]]).astype(np.int64)
    n = lead + int(np.sum(lens)) + trail
    keys = pool[rng.integers(0, pool.size, n)]
    if n >= 4:
        keys[rng.integers(0, n, 2)] = [EMPTY, RECLAIMED]
    off = (lead + np.concatenate([[0], np.cumsum(lens)])).astype(np.int64)
    return keys, off


# ---- bit-exact forward: every row shape, both ends, partial waves ------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("keep", ["first", "last"])
@pytest.mark.parametrize("dim", [8, 40, 64, 128, 1024])
def test_forward_bit_exact(dev, dim, keep):
    """dims 8 / 40 / 1024 take the run-time row shape (fewer live lanes than a tile, a partial lane mask, all 16 groups per lane).  The grid
    depends on n_bags * max_len only (no host switch on the bag lengths); 1 .. 180 slots cover partial waves and several blocks.  ONE host value does
    pick the instance: a block of more than 128 MiB is written by the streaming-store instances — every batch here is on the near side of that switch,
    test_streaming_store_instances is the far side."""
    t, o, u = make_table(dev, dim)
    twin, _, _ = make_table(dev, dim)
    rng = np.random.default_rng(dim)
    for n_bags in (1, 3, 5, 9):
        keys, off = make_batch(rng, u, LENS[:n_bags])
        kd, od = T(keys, dev), T(off, dev)
        for L in (1, 4, 16, 20):
            outs = Outs(dev, keys.size, n_bags, L, dim)
            assert raw(t._h, kd, od, n_bags, L, keep, outs, dev) == 0
            check_all(outs, expected_padded(lambda b: o.find, keys, off, L, keep, dim), f"dim {dim} n_bags {n_bags} L {L} {keep}")
        twin.find_pooled(kd, od)
        assert t.status() == twin.status() == 0   # neither touches the status word, reserved keys or not
    for x in (t, twin, o):
        x.close()


@pytest.mark.gpu
@pytest.mark.parametrize("keep", ["first", "last"])
@pytest.mark.parametrize("dim", [64, 40])
def test_bf16_out(dev, dim, keep):
    t, o, u = make_table(dev, dim)
    keys, off = make_batch(np.random.default_rng(5), u, LENS)
    for L in (4, 20):
        outs = Outs(dev, keys.size, len(LENS), L, dim, dtype=BF16)
        assert raw(t._h, T(keys, dev), T(off, dev), len(LENS), L, keep, outs, dev) == 0
        exp = expected_padded(lambda b: o.find, keys, off, L, keep, dim)
        check_all(outs, exp, f"bf16 out dim {dim} L {L} {keep}", bf16=True)
        pad = np.arange(L)[None, :] >= exp[2][:, None]
        assert pad.any() and not outs.out.cpu().view(torch.int16).numpy()[pad].any()   # padding is the bit pattern 0x0000
    t.close(); o.close()


# ---- the far side of the store-policy switch: a block of more than 128 MiB leaves through the streaming-store instances ---------------------------
STREAM_BYTES = 128 << 20          # kCachedOutputBytes (meepo_host.h): out_bytes <= this -> plain stores, beyond -> streaming stores
STREAM_L = 64
STREAM_CYCLE = [1, 2, 15, 16, 17, 33, 64, 65, 90]   # the lengths of the bags that hold keys (every 7th bag; the rest are empty): below, at and past L


def _stream_batch(rng, stored, dim, elem):
    """the smallest odd number of bags whose [n_bags, STREAM_L, dim] block passes the switch, most of them empty -> (keys, offsets, n_bags)"""
    n_bags = STREAM_BYTES // (STREAM_L * dim * elem) + 1
    n_bags += 1 - n_bags % 2
    assert n_bags * STREAM_L * dim * elem > STREAM_BYTES >= (n_bags - 2) * STREAM_L * dim * elem
    lens = np.zeros(n_bags, np.int64)
    lens[::7] = np.resize(STREAM_CYCLE, lens[::7].size)
    keys, off = make_batch(rng, stored, lens)
    return keys, off, n_bags


def _check_on_device(o, exp, what, dev, bf16):
    """check_all for a large block: `out` is compared on the device (every element, bit for bit), the small outputs on the host"""
    eo, ef, el, ek, eg = exp
    if bf16:
        ref = torch.from_numpy(bf16_bits(eo).view(np.int16)).to(dev)
        assert torch.equal(o.out.view(torch.int16), ref), f"{what}: out (bf16 bits)"
    else:
        assert torch.equal(o.out.view(torch.int32), torch.from_numpy(eo.view(np.int32)).to(dev)), f"{what}: out (every element)"
    assert np.array_equal(o.found.cpu().numpy(), ef) and np.array_equal(o.lengths.cpu().numpy(), el), f"{what}: found / lengths"
    assert np.array_equal(o.step_keys.cpu().numpy(), ek) and np.array_equal(o.grad_index.cpu().numpy().view(np.uint32), eg), f"{what}: step_keys / grad_index"


@pytest.mark.gpu
@pytest.mark.parametrize("dim,out_dtype,bf16_rows", [(d, o, r) for d in (64, 128, 40) for o in (torch.float32, BF16) for r in (False, True)] + [(1024, torch.float32, False)],
                         ids=lambda v: {torch.float32: "fp32out", BF16: "bf16out", False: "fp32rows", True: "bf16rows"}.get(v, str(v)))
def test_streaming_store_instances(dev, dim, out_dtype, bf16_rows):
    """a block just past 128 MiB (the host switch to streaming stores), one table: every element against the oracle, both ends — every streaming
    instance of the table form (row shape x out type x row type; dim 40 and 1024 are the run-time shape)"""
    t, o, u = make_table(dev, dim, bf16_rows=bf16_rows)
    elem = 2 if out_dtype == BF16 else 4
    keys, off, n_bags = _stream_batch(np.random.default_rng(dim + elem), u, dim, elem)
    for keep in ("first", "last"):
        outs = Outs(dev, keys.size, n_bags, STREAM_L, dim, dtype=out_dtype)
        assert outs.out.numel() * elem > STREAM_BYTES
        assert raw(t._h, T(keys, dev), T(off, dev), n_bags, STREAM_L, keep, outs, dev) == 0
        _check_on_device(outs, expected_padded(lambda b: o.find, keys, off, STREAM_L, keep, dim), f"streaming dim {dim} {out_dtype} bf16_rows={bf16_rows} {keep}",
                         dev, out_dtype == BF16)
        del outs
    t.close(); o.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dim,out_dtype,bf16_rows", [(d, o, r) for d in (64, 128, 24) for o in (torch.float32, BF16) for r in (False, True)],
                         ids=lambda v: {torch.float32: "fp32out", BF16: "bf16out", False: "fp32rows", True: "bf16rows"}.get(v, str(v)))
def test_streaming_store_instances_group(dev, dim, out_dtype, bf16_rows):
    """the same for every streaming instance of the group form: 3 members with different rows and defaults, a number of bags per member that is no
    multiple of 4"""
    n_members = 3
    made = [make_table(dev, dim, seed=2 + j, default=0.25 * (j + 1), bf16_rows=bf16_rows) for j in range(n_members)]
    grp = TableGroup([m[0] for m in made])
    elem = 2 if out_dtype == BF16 else 4
    bpt = STREAM_BYTES // (STREAM_L * dim * elem * n_members) + 1
    bpt += 1 - bpt % 2
    n_bags = bpt * n_members
    lens = np.zeros(n_bags, np.int64)
    lens[::7] = np.resize(STREAM_CYCLE, lens[::7].size)
    keys, off = make_batch(np.random.default_rng(dim), made[0][2], lens)
    outs = Outs(dev, keys.size, n_bags, STREAM_L, dim, dtype=out_dtype)
    assert outs.out.numel() * elem > STREAM_BYTES
    assert raw(grp._h, T(keys, dev), T(off, dev), bpt, STREAM_L, "last", outs, dev, group=True) == 0
    _check_on_device(outs, expected_padded(lambda b: made[b // bpt][1].find, keys, off, STREAM_L, "last", dim), f"streaming group dim {dim} {out_dtype}", dev,
                     out_dtype == BF16)
    grp.close()
    for t, o, _ in made:
        t.close(); o.close()


# ---- caller offsets ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("keep", ["first", "last"])
def test_caller_offsets(dev, keep):
    """bag_offsets[0] > 0, a bag cut at n, a bag wholly past n, a decreasing pair at the end, bag_offsets[-1] < n: the clamped spans are used,
    positions in no bag keep their sentinel in every per-position output.  The keys sit at the very end of their allocation."""
    dim = 64
    t, o, u = make_table(dev, dim)
    keys, _ = make_batch(np.random.default_rng(9), u, [60])
    n = keys.size
    buf = torch.empty(4096 + n, dtype=torch.int64, device=dev)
    kd = buf[-n:]
    kd.copy_(T(keys, dev))
    cases = {"lead and trail": [3, 10, 10, 31, 52],           # positions 0-2 and 52-59 lie in no bag; an empty bag in between
             "past n": [0, 20, 45, 1 << 40, 1 << 41],          # bag 2 is cut at n, bag 3 lies wholly past it
             "decreasing": [2, 19, 40, 25]}                    # the last pair goes down: an empty bag, positions 40-59 in no bag
    for name, off in cases.items():
        off = np.array(off, np.int64)
        for L in (4, 20):
            outs = Outs(dev, n, off.size - 1, L, dim)
            assert raw(t._h, kd, T(off, dev), off.size - 1, L, keep, outs, dev) == 0
            exp = expected_padded(lambda b: o.find, keys, off, L, keep, dim)
            covered = np.zeros(n, bool)
            for begin, end in spans(off, n):
                covered[begin:end] = True
            assert (~covered).any() or name == "past n"
            assert (exp[1][~covered] == FOUND_SENTINEL).all() and (exp[3][~covered] == I64_SENTINEL).all()
            check_all(outs, exp, f"offsets '{name}' L {L} {keep}")
    t.close(); o.close()


# ---- row storage types -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("out_dtype", [torch.float32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("dim", [64, 128, 24])
def test_bf16_row_table(dev, dim, out_dtype):
    """fp32 out = the widened stored rows, bf16 out = the stored bits: both are the fp32 twin handed bf16(values)"""
    t, o, u = make_table(dev, dim, bf16_rows=True)
    keys, off = make_batch(np.random.default_rng(dim), u, LENS)
    for keep in ("first", "last"):
        outs = Outs(dev, keys.size, len(LENS), 16, dim, dtype=out_dtype)
        assert raw(t._h, T(keys, dev), T(off, dev), len(LENS), 16, keep, outs, dev) == 0
        check_all(outs, expected_padded(lambda b: o.find, keys, off, 16, keep, dim), f"bf16 rows dim {dim} {out_dtype} {keep}", bf16=out_dtype == BF16)
    po, pf, pl = t.find_padded(T(keys, dev), T(off, dev), 16, keep="last", out_dtype=out_dtype)   # the Python form: the same call
    bits = torch.int16 if out_dtype == BF16 else torch.int32
    assert torch.equal(po.view(bits), outs.out.view(bits)) and torch.equal(pf, outs.found)
    assert po.dtype == out_dtype and po.shape == (len(LENS), 16, dim) and pl.tolist() == [min(x, 16) for x in LENS]
    t.close(); o.close()


@pytest.mark.gpu
def test_rows_in_pinned_host_memory(dev):
    """a cold-tier table (value_memory = MEM_HOST_PINNED): the rows are read over the host link, the result is the same"""
    t, o, u = make_table(dev, 64, value_memory=_lib.MEM_HOST_PINNED)
    keys, off = make_batch(np.random.default_rng(2), u, LENS)
    outs = Outs(dev, keys.size, len(LENS), 16, 64)
    assert raw(t._h, T(keys, dev), T(off, dev), len(LENS), 16, "last", outs, dev) == 0
    check_all(outs, expected_padded(lambda b: o.find, keys, off, 16, "last", 64), "pinned host rows")
    t.close(); o.close()


@pytest.mark.gpu
def test_int8_row_table_is_refused(dev):
    t = LookupTable(1024, 64, device=dev, max_batch=4096, int8_rows=True)
    keys = T(np.arange(1, 21, dtype=np.int64), dev)
    off = T(np.array([0, 5, 20], np.int64), dev)
    outs = Outs(dev, 20, 2, 4, 64)
    assert raw(t._h, keys, off, 2, 4, "first", outs, dev) == _lib.ERR_UNSUPPORTED
    assert "mee_find_padded_as" in _lib.lib().mee_last_error().decode() and outs.untouched()
    with pytest.raises(MeepoError) as ei:
        t.find_padded(keys, off, 4)
    assert ei.value.code == _lib.ERR_UNSUPPORTED and "mee_find_padded_as" in str(ei.value)
    t.close()


# ---- groups ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("out_dtype", [torch.float32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("bf16_rows", [False, True], ids=["fp32rows", "bf16rows"])
@pytest.mark.parametrize("dim", [64, 24])
def test_group(dev, dim, bf16_rows, out_dtype):
    """3 members x 5 bags (a wave serves two members): the same key values stored in every member with different rows and another default value;
    each member's block equals that member's own expectation"""
    n_members, bpt = 3, 5
    made = [make_table(dev, dim, seed=2 + j, default=0.25 * (j + 1), bf16_rows=bf16_rows) for j in range(n_members)]
    grp = TableGroup([m[0] for m in made])
    lens = [33, 0, 17, 1, 16,   2, 15, 0, 5, 21,   16, 16, 3, 0, 40]
    keys, off = make_batch(np.random.default_rng(3), made[0][2], lens)
    for keep in ("first", "last"):
        for L in (4, 20):
            outs = Outs(dev, keys.size, n_members * bpt, L, dim, dtype=out_dtype)
            assert raw(grp._h, T(keys, dev), T(off, dev), bpt, L, keep, outs, dev, group=True) == 0
            exp = expected_padded(lambda b: made[b // bpt][1].find, keys, off, L, keep, dim)
            check_all(outs, exp, f"group dim {dim} L {L} {keep}", bf16=out_dtype == BF16)
    po, pf, pl, sk, gi = grp.find_padded(T(keys, dev), T(off, dev), 20, keep="last", out_dtype=out_dtype, with_step=True)   # the Python form
    assert torch.equal(po.view(torch.int16 if out_dtype == BF16 else torch.int32), outs.out.view(torch.int16 if out_dtype == BF16 else torch.int32))
    assert torch.equal(pf, outs.found) and torch.equal(pl, outs.lengths) and torch.equal(sk, outs.step_keys) and torch.equal(gi, outs.grad_index)
    grp.close()
    for t, o, _ in made:
        t.close(); o.close()


# ---- refusals: before anything is launched or written -------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_and_zero_bags(dev):
    dim = 64
    t, o, u = make_table(dev, dim)
    grp = TableGroup([t])
    keys, off = make_batch(np.random.default_rng(1), u, [3, 9])
    kd, od = T(keys, dev), T(off, dev)
    for handle, group in ((t._h, False), (grp._h, True)):
        bad = lambda outs=None, h=handle, L=4, keep="first", bags=2, **nulls: (
            lambda oo: (raw(h, kd, od, bags, L, keep, oo, dev, group=group, **nulls), oo))(outs or Outs(dev, keys.size, 2, 4, dim))
        for what, (rc, oo) in {
            "null table / group": bad(h=None), "null bag_offsets": bad(off=True), "null out": bad(out=True), "null keys": bad(keys=True),
            "max_len 0": bad(L=0), "unknown flag bit": bad(keep=2), "unknown flag bit 2": bad(keep=0x80000001),
            "unknown out_dtype": bad(dtype=7), "int8 out_dtype": bad(dtype=_lib.DTYPE_INT8),
            # n_bags * max_len = 2^31 with a grad_index output (returns before it looks at any buffer)
            "2^31 slots with grad_index": bad(L=1 << 30),
        }.items():
            assert rc == _lib.ERR_INVALID_ARG, f"{what} ({'group' if group else 'table'}): rc {rc}"
            assert oo.untouched(), what
        whole = torch.full((2 * 4 * dim + 4,), float("nan"), dtype=BF16, device=dev)
        rc, oo = bad(Outs(dev, keys.size, 2, 4, dim, out=whole[1:1 + 2 * 4 * dim]))   # a bf16 out that is 2 bytes off an 8-byte boundary
        assert whole.data_ptr() % 8 == 0 and rc == _lib.ERR_INVALID_ARG and oo.untouched() and bool(torch.isnan(whole.float()).all())
        rc, oo = bad(bags=0)
        assert rc == 0 and oo.untouched(), "zero bags succeed and write nothing"
        rc, oo = bad(bags=0, off=True, out=True)
        assert rc == 0 and oo.untouched()
    with pytest.raises(ValueError):
        t.find_padded(kd, od, 4, keep="middle")
    with pytest.raises(ValueError):
        t.find_padded(kd, od, 0)
    grp.close(); t.close(); o.close()


# ---- far output and far rows -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_output_past_the_walls(dev):
    """n_bags * max_len * dim just over 2^32 elements (a 17.2 GB fp32 block): bags of 0-5 keys, max_len 4 (the bags of 5 are cut); slots that hold
    a row on both sides of every wall hold a present key's row, the other live slots an absent key's default row, everything else +0"""
    from test_far_rows import OUT_DEFAULT, OUT_DIM, OUT_N, POOL_SEED, check_output, output_tables, wall_positions
    with output_tables(dev) as ((t,), (u,)):
        L = 4
        n_bags = OUT_N // L
        lens = torch.arange(n_bags, dtype=torch.int64, device=dev) % 6
        off = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(lens, 0)])
        n = int(off[-1])
        slots = wall_positions(OUT_N)
        slots = slots[(slots % L) < np.minimum((slots // L) % 6, L)]     # the slots that hold a row: j < min(len(b), L)
        assert slots.size > 100 and (slots > (1 << 22)).any()            # (of the test's own construction: 14 of 24 slots hold a row)
        keys = synth.keys_t(POOL_SEED + 20, 0, n, dev)                   # absent
        present = u[np.arange(slots.size) % u.size]
        at = off[:-1][T(slots // L, dev)] + T(slots % L, dev)            # keep="first": slot j holds position begin + j
        keys[at] = T(present, dev)
        out, found, lengths = t.find_padded(keys, off, L)
        fmask = torch.zeros(n, dtype=torch.bool, device=dev); fmask[at] = True
        assert torch.equal(found.bool(), fmask) and torch.equal(lengths, lens.clamp(max=L))
        live = (torch.arange(L, device=dev)[None, :] < lens[:, None]).reshape(-1)
        check_output(out.view(-1, OUT_DIM), None, slots, live.to(torch.float32) * OUT_DEFAULT, synth.rows_np(present, OUT_DIM, 2), dev, "find_padded")


@pytest.mark.gpu
def test_rows_past_the_byte_wall(dev):
    """a dim-64 table whose value plane passes 2^32 bytes (tests/test_far_rows.py's helper): near and far keys in one padded batch"""
    from test_far_rows import far_table
    with far_table(dev, 64, "byte", default_value=DEFAULT) as F:
        rng = np.random.default_rng(12)
        lens = rng.integers(0, 40, 200)
        keys = F.batch(rng, n=int(lens.sum()) - 64 + 0, absent=64)
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        assert keys.size == off[-1]
        for keep in ("first", "last"):
            outs = Outs(dev, keys.size, lens.size, 20, 64)
            assert raw(F.t._h, T(keys, dev), T(off, dev), lens.size, 20, keep, outs, dev) == 0
            check_all(outs, expected_padded(lambda b: F.o.find, keys, off, 20, keep, 64), f"far rows {keep}")


# ---- training through the layer ----------------------------------------------------------------------------------------------------------------
def _opt(optimizer):
    return (OPT_ADAGRAD, oracle.OPT_ADAGRAD) if optimizer == "adagrad" else (OPT_ADAM, oracle.OPT_ADAM)


def _oracle_step(o, optimizer, keys, g, lr, step):
    if optimizer == "adagrad":
        o.apply_adagrad(keys, g, lr, 1e-10)
    else:
        o.apply_adam(keys, g, lr, 0.9, 0.999, 1e-8, step)


def _assert_tables_close(t, o, what):
    """SPEC.md §4's tolerance for steps on duplicate keys: 1e-6 relative, atol 1e-9"""
    e, eo = export_sorted(t), export_sorted(o)
    assert len(e) == len(eo) and np.array_equal(e[0], eo[0]), what
    for x, z in zip(e[1:], eo[1:]):
        np.testing.assert_allclose(x, z, rtol=1e-6, atol=1e-9, err_msg=what)


@pytest.mark.gpu
@pytest.mark.parametrize("duplicates", [False, True], ids=["distinct", "duplicates"])
@pytest.mark.parametrize("keep", ["first", "last"])
@pytest.mark.parametrize("optimizer", ["adagrad", "adam"])
def test_layer_trains_a_table(dev, optimizer, keep, duplicates):
    from meepoembedding_amd.nn import DynamicEmbeddingSequence
    dim, L, lr = 64, 8, 0.05
    opt, oopt = _opt(optimizer)
    t, o, u = make_table(dev, dim, optimizer=opt, initial_accumulator=0.1)
    assert opt == oopt
    lens = [0, 3, 8, 19, 1, 12]
    n = sum(lens)
    absent = synth.keys_np(991, 0, 4)
    keys = np.concatenate([u[:n - 4], absent]) if not duplicates else np.concatenate([u[:10], u[:10], u[5:5 + n - 24], absent])
    keys = np.random.default_rng(4).permutation(keys)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    layer = DynamicEmbeddingSequence(t, L, keep=keep, optimizer=optimizer, lr=lr, create_missing=False).to(dev)
    layer.train()
    assert layer.traits.native_padded
    _, _, _, step_keys, grad_index = expected_padded(lambda b: o.find, keys, off, L, keep, dim)
    kept = np.nonzero(step_keys != EMPTY)[0]
    assert (len(set(keys[kept].tolist())) < kept.size) == duplicates
    before = {int(k): r.copy() for k, r in zip(*[x for x in export_sorted(o)[:2]])}
    for step in (1, 2):
        w = (synth.rows_np(np.arange(len(lens) * L), dim, 20 + step) * 0.1).reshape(len(lens), L, dim)
        padded, lengths = layer(T(keys, dev), T(off, dev))
        exp = expected_padded(lambda b: o.find, keys, off, L, keep, dim)
        if not duplicates or step == 1:
            assert np.array_equal(padded.detach().cpu().numpy().view(np.uint32), exp[0].view(np.uint32))
        assert np.array_equal(lengths.cpu().numpy(), exp[2])
        (padded * T(w, dev)).sum().backward()
        _oracle_step(o, optimizer, keys[kept], w.reshape(-1, dim)[grad_index[kept].astype(np.int64)], lr, step)
    if duplicates:
        _assert_tables_close(t, o, "after two steps with duplicate kept keys")
    else:
        assert_tables_bit_equal(t, o, "after two steps without duplicate kept keys")
    assert t.size() == u.size and not t.find(T(absent, dev))[1].any()       # absent keys with create_missing=False: not created
    cut_only = [int(k) for k in set(keys[step_keys == EMPTY].tolist()) - set(keys[kept].tolist()) if int(k) in before]
    assert cut_only
    rows, _ = t.find(T(np.array(cut_only, np.int64), dev))
    assert np.array_equal(rows.cpu().numpy(), np.stack([before[k] for k in cut_only]))   # cut-off keys took no step
    t.close(); o.close()


@pytest.mark.gpu
def test_layer_creates_unseen_ids_in_training_only(dev):
    from meepoembedding_amd.nn import DynamicEmbeddingSequence
    t, o, u = make_table(dev, 64, optimizer=OPT_ADAGRAD)
    fresh = synth.keys_np(991, 0, 6)
    keys = np.concatenate([u[:10], fresh])
    off = np.array([0, 4, 16], np.int64)        # the second bag is cut: unseen ids beyond max_len are created too
    layer = DynamicEmbeddingSequence(t, 5).to(dev)
    layer.eval()
    layer(T(keys, dev), T(off, dev))
    assert t.size() == u.size and not t.find(T(fresh, dev))[1].any()
    layer.train()
    padded, _ = layer(T(keys, dev), T(off, dev))
    padded.sum().backward()
    assert t.size() == u.size + fresh.size and t.find(T(fresh, dev))[1].all() and t.status() == 0
    t.close(); o.close()


@pytest.mark.gpu
@pytest.mark.parametrize("duplicates", [False, True], ids=["distinct", "duplicates"])
@pytest.mark.parametrize("optimizer", ["adagrad", "adam"])
def test_layer_trains_a_group(dev, optimizer, duplicates):
    """per member what test_layer_trains_a_table checks: bit-identical without duplicate kept keys inside a member, SPEC.md §4's tolerance with them"""
    from meepoembedding_amd.nn import DynamicEmbeddingSequence
    dim, L, lr, n_members, bpt = 64, 6, 0.05, 3, 3
    opt, oopt = _opt(optimizer)
    tables, oracles = [], []
    u = synth.keys_np(77, 0, 300)
    for j in range(n_members):
        t = LookupTable(1024, dim, device=dev, max_batch=4096, optimizer=opt, default_value=0.25 * j, initial_accumulator=0.1)
        o = oracle.OracleTable(1024, dim, optimizer=oopt, default_value=0.25 * j, initial_accumulator=0.1)
        rows = synth.rows_np(u, dim, 2 + j)
        t.insert(T(u, dev), T(rows, dev)); o.insert(u, rows)
        tables.append(t); oracles.append(o)
    grp = TableGroup(tables, max_apply_batch=4096)
    lens = [2, 0, 9,   6, 13, 1,   0, 7, 4]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    seg = off[::bpt]
    keys = np.concatenate([np.random.default_rng(j).permutation(u)[:seg[j + 1] - seg[j]] for j in range(n_members)])   # distinct inside a member, shared across members
    if duplicates:
        for j in range(n_members):   # the second half of every member's positions repeats its first half
            m = seg[j + 1] - seg[j]
            keys[seg[j] + m - m // 2:seg[j + 1]] = keys[seg[j]:seg[j] + m // 2]
    keys[3] = synth.keys_np(991, 0, 1)[0]     # absent
    kept0 = expected_padded(lambda b: oracles[b // bpt].find, keys, off, L, "last", dim)[3]
    dup_kept = [len(set(k.tolist())) < k.size for k in (kept0[seg[j]:seg[j + 1]][kept0[seg[j]:seg[j + 1]] != EMPTY] for j in range(n_members))]
    assert any(dup_kept) == duplicates
    layer = DynamicEmbeddingSequence(grp, L, keep="last", optimizer=optimizer, lr=lr, create_missing=False).to(dev)
    layer.train()
    for step in (1, 2):
        w = (synth.rows_np(np.arange(len(lens) * L), dim, 30 + step) * 0.1).reshape(len(lens), L, dim)
        exp = expected_padded(lambda b: oracles[b // bpt].find, keys, off, L, "last", dim)
        padded, lengths = layer(T(keys, dev), T(off, dev))
        if not duplicates or step == 1:
            assert np.array_equal(padded.detach().cpu().numpy().view(np.uint32), exp[0].view(np.uint32))
        assert np.array_equal(lengths.cpu().numpy(), exp[2])
        (padded * T(w, dev)).sum().backward()
        for j, o in enumerate(oracles):
            pos = np.arange(seg[j], seg[j + 1])
            pos = pos[exp[3][pos] != EMPTY]
            _oracle_step(o, optimizer, keys[pos], w.reshape(-1, dim)[exp[4][pos].astype(np.int64)], lr, step)
    for j, (t, o) in enumerate(zip(tables, oracles)):
        if duplicates:
            _assert_tables_close(t, o, f"member {j}, duplicate kept keys")
        else:
            assert_tables_bit_equal(t, o, f"member {j}")
        assert t.size() == u.size    # the absent key of member 0 was not created (create_missing=False), nothing else was either
    grp.close()
    for x in tables + oracles:
        x.close()


@pytest.mark.gpu
def test_layer_over_a_group_creates_unseen_ids_in_training_only(dev):
    """create_missing=True over a group: the grouped find_or_insert runs in front of the padded lookup with the members' offsets, so an unseen id is
    created in ITS member only — cut-off ones too — and an eval forward creates nothing"""
    from meepoembedding_amd.nn import DynamicEmbeddingSequence
    dim, L, n_members, bpt = 64, 3, 3, 2
    u = synth.keys_np(77, 0, 100)
    tables = [LookupTable(1024, dim, device=dev, max_batch=4096, optimizer=OPT_ADAGRAD) for _ in range(n_members)]
    for t in tables:
        t.insert(T(u, dev), T(synth.rows_np(u, dim, 2), dev))
    grp = TableGroup(tables, max_apply_batch=4096)
    fresh = synth.keys_np(991, 0, 6)
    lens = [2, 5,   0, 4,   6, 1]          # the bags of 5, 4 and 6 are cut at L = 3
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    keys = u[:off[-1]].copy()
    fresh_at = {0: [0, 5], 1: [8, 9], 2: [11, 17]}   # member -> positions of its fresh ids (kept and cut-off ones)
    for i, p in enumerate(q for ps in fresh_at.values() for q in ps):
        keys[p] = fresh[i]
    layer = DynamicEmbeddingSequence(grp, L).to(dev)
    layer.eval()
    layer(T(keys, dev), T(off, dev))
    assert all(t.size() == u.size for t in tables)
    layer.train()
    padded, _ = layer(T(keys, dev), T(off, dev))
    padded.sum().backward()
    for j, t in enumerate(tables):
        mine = keys[fresh_at[j]]
        others = np.setdiff1d(fresh, mine)
        assert t.size() == u.size + 2 and t.find(T(mine, dev))[1].all() and not t.find(T(others, dev))[1].any() and t.status() == 0, f"member {j}"
    grp.close()
    for t in tables:
        t.close()


# ---- capture -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_capture_and_replay(dev):
    """one torch.cuda.graph capture and two replays of the table form give the eager result: the call neither synchronises nor allocates"""
    dim, L = 64, 8
    t, o, u = make_table(dev, dim)
    keys, off = make_batch(np.random.default_rng(21), u, LENS)
    kd, od = T(keys, dev), T(off, dev)
    outs = Outs(dev, keys.size, len(LENS), L, dim)
    eager = Outs(dev, keys.size, len(LENS), L, dim)
    assert raw(t._h, kd, od, len(LENS), L, "last", eager, dev) == 0
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rc = raw(t._h, kd, od, len(LENS), L, "last", outs, dev)
    assert rc == 0
    exp = expected_padded(lambda b: o.find, keys, off, L, "last", dim)
    for _ in range(2):
        outs.out.fill_(float("nan")); outs.found.fill_(FOUND_SENTINEL); outs.step_keys.fill_(I64_SENTINEL)
        outs.lengths.fill_(I64_SENTINEL); outs.grad_index.fill_(U32_SENTINEL)
        assert outs.untouched()
        graph.replay()
        torch.cuda.synchronize(dev)
        check_all(outs, exp, "replay")
        assert torch.equal(outs.out.view(torch.int32), eager.out.view(torch.int32))
    t.close(); o.close()
