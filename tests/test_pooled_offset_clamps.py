"""Bag offsets are caller data (SPEC.md §3): a bag that runs past the key array is cut at its end, a bag wholly past it and a decreasing
pair are empty bags.  The clamp lives in the one bag walk all pooled lookups share; tests/test_gpu_parity.py, test_weighted_bags.py,
test_tiered_bags.py, test_bf16_rows.py and test_bf16_row_groups.py pin it for one table, the weighted form, the tiered pair and bf16 rows.
Here: the fp32 uniform group, the jagged member map and the mixed group.  The result with the bad offsets is bit-identical to the same call
with the offsets clamped by hand, `found` included."""
import numpy as np
import pytest
import torch

N_MEMBERS, BPT = 3, 5   # 5 bags per member: with four bags per wave a wave straddles two members


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _members(dev, dims):
    from meepoembedding_amd import LookupTable, synth
    rng = np.random.default_rng(sum(dims))
    tables, univ = [], []
    for j, d in enumerate(dims):
        u = synth.keys_np(640 + j, 0, 200)
        t = LookupTable(512, d, device=dev, max_batch=4096, default_value=0.25 * (j + 1))
        t.insert(T(u, dev), T(rng.standard_normal((u.size, d)).astype(np.float32), dev))
        tables.append(t); univ.append(u)
    return tables, univ


def _batches(univ):
    """-> [(keys, bad offsets, the same bags clamped by hand)] for both launch shapes.  The last three bags are the bad ones: bag 12 runs past the
    key array (to 2^40), bag 13 lies wholly past it, bag 14 is a decreasing pair."""
    from meepoembedding_amd import synth
    rng = np.random.default_rng(7)
    out = []
    # tile per bag: lengths 0, 1, 15 (the longest short bag), 16 (kPoolLong) and 23 (four tiles on one bag); bag 12 keeps 15 keys — a short bag only
    # if its end is clamped.  Wave per bag: every bag of 16 .. 40 keys, bag 12 keeps 30.
    for lens in ([0, 1, 15, 16, 23, 23, 16, 15, 1, 0, 16, 0, 15], list(rng.integers(16, 41, 12)) + [30]):
        good = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        n = int(good[-1])
        assert (n // (N_MEMBERS * BPT) >= 12) == (min(lens) >= 16)   # the launch shape this batch is meant to take
        bad = np.concatenate([good[:-1], [1 << 40, 1 << 41, 3]]).astype(np.int64)
        clamped = np.concatenate([good, [n, n]]).astype(np.int64)
        member = np.searchsorted(clamped[::BPT][1:], np.arange(n), side="right")   # of every key position
        keys = np.array([univ[m][rng.integers(0, univ[m].size)] for m in member], np.int64)
        keys[5] = synth.keys_np(996, 0, 1)[0]   # absent: found has both values
        out.append((keys, bad, clamped))
    return out


def _lookup(call, keys, off, dev):
    found = torch.full((keys.size,), 7, dtype=torch.uint8, device=dev)
    out, f = call(T(keys, dev), T(off, dev), found)
    assert f.data_ptr() == found.data_ptr()
    return out, found


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["sum", "mean"])
@pytest.mark.parametrize("dim", [64, 24])
def test_uniform_group_tolerates_bad_offsets(dev, dim, mode):
    from meepoembedding_amd import TableGroup
    tables, univ = _members(dev, (dim,) * N_MEMBERS)
    grp = TableGroup(tables)
    for keys, bad, clamped in _batches(univ):
        call = lambda k, o, f: grp.find_pooled(k, o, mode, found=f)
        out_bad, found_bad = _lookup(call, keys, bad, dev)
        out_ok, found_ok = _lookup(call, keys, clamped, dev)
        assert torch.equal(out_bad, out_ok) and torch.equal(found_bad, found_ok)
        assert not out_bad[13:].any() and set(found_bad.tolist()) == {0, 1}   # the bags past the array are rows of zeros; every key was reported
    grp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["sum", "mean"])
@pytest.mark.parametrize("dim", [64, 24])
def test_jagged_group_tolerates_bad_offsets(dev, dim, mode):
    from meepoembedding_amd import TableGroup
    tables, univ = _members(dev, (dim,) * N_MEMBERS)
    grp = TableGroup(tables)
    member_bags = T(np.arange(N_MEMBERS + 1, dtype=np.int64) * BPT, dev)
    for keys, bad, clamped in _batches(univ):
        call = lambda k, o, f: grp.find_pooled_jagged(k, o, member_bags, mode, found=f)
        out_bad, found_bad = _lookup(call, keys, bad, dev)
        out_ok, found_ok = _lookup(call, keys, clamped, dev)
        assert torch.equal(out_bad, out_ok) and torch.equal(found_bad, found_ok)
        assert not out_bad[13:].any() and set(found_bad.tolist()) == {0, 1}
        uni, found_uni = _lookup(lambda k, o, f: grp.find_pooled(k, o, mode, found=f), keys, clamped, dev)   # the same map, spelled bags_per_table
        assert torch.equal(out_bad, uni) and torch.equal(found_bad, found_uni)
    grp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["sum", "mean"])
def test_mixed_group_tolerates_bad_offsets(dev, mode):
    from meepoembedding_amd import MixedTableGroup
    tables, univ = _members(dev, (8, 64, 100))
    grp = MixedTableGroup(tables)
    for keys, bad, clamped in _batches(univ):
        call = lambda k, o, f: grp.find_pooled(k, o, mode, found=f)
        views_bad, found_bad = _lookup(call, keys, bad, dev)
        views_ok, found_ok = _lookup(call, keys, clamped, dev)
        assert torch.equal(found_bad, found_ok) and set(found_bad.tolist()) == {0, 1}
        for j, t in enumerate(tables):   # ... and equals find_pooled of every member on its bags
            lo, hi = int(clamped[j * BPT]), int(clamped[(j + 1) * BPT])
            eo, ef = t.find_pooled(T(keys[lo:hi], dev), T(clamped[j * BPT:(j + 1) * BPT + 1] - lo, dev), mode)
            assert torch.equal(views_bad[j], views_ok[j]) and torch.equal(views_bad[j], eo), f"member {j} (dim {t.dim})"
            assert torch.equal(found_bad[lo:hi], ef)
        assert not views_bad[2][3:].any()
    grp.close()
