"""What the padded-lookup tests share: the expectation of find_padded (SPEC.md §3) as a plain loop over bags on top of a `find` callable —
the oracle's — and the byte patterns the tests pre-fill outputs with.  No product code is used here."""
import numpy as np

EMPTY = -(1 << 63)
RECLAIMED = EMPTY + 1
FOUND_SENTINEL = 0xA5
I64_SENTINEL = 0x5A5A5A5A5A5A5A5A
U32_SENTINEL = 0x5A5A5A5A


def spans(offsets, n):
    """the clamped span of every bag: end = min(off[b+1], n), begin = min(off[b], end)"""
    out = []
    for b in range(len(offsets) - 1):
        end = min(int(offsets[b + 1]), n)
        begin = min(int(offsets[b]), end)
        out.append((begin, end))
    return out


def expected_padded(find_of_bag, keys, offsets, max_len, keep, dim):
    """-> (out [n_bags, max_len, dim] fp32, found [n] uint8, lengths [n_bags] int64, step_keys [n] int64, grad_index [n] uint32).
    find_of_bag(b) -> a callable keys -> (rows, found): the find of the table bag b belongs to.  Positions in no bag keep the sentinels."""
    keys = np.asarray(keys, np.int64)
    n, n_bags = keys.size, len(offsets) - 1
    out = np.zeros((n_bags, max_len, dim), np.float32)
    found = np.full(n, FOUND_SENTINEL, np.uint8)
    lengths = np.zeros(n_bags, np.int64)
    step_keys = np.full(n, I64_SENTINEL, np.int64)
    grad_index = np.full(n, U32_SENTINEL, np.uint32)
    for b, (begin, end) in enumerate(spans(offsets, n)):
        kept = min(end - begin, max_len)
        lengths[b] = kept
        first = begin if keep == "first" else end - kept
        for i in range(begin, end):   # every position of the bag: cut off unless kept below
            found[i], step_keys[i], grad_index[i] = 0, EMPTY, 0
        if kept:
            rows, f = find_of_bag(b)(keys[first:first + kept])
            out[b, :kept] = rows
            found[first:first + kept] = f
            step_keys[first:first + kept] = keys[first:first + kept]
            grad_index[first:first + kept] = b * max_len + np.arange(kept)
    return out, found, lengths, step_keys, grad_index


def bf16_bits(x):
    """fp32 array -> the uint16 bits of its round-to-nearest-even bf16 (finite values)"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
