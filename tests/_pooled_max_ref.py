"""The NumPy restatement of max pooling (SPEC.md §3 find_pooled_max / pooled_max_backward): the sequential scan, written down once for the tests.

For every element the bag is scanned in ascending position: the first position is assigned, a later one replaces the running value iff it is greater by
the IEEE comparison (numpy's `>` on float32: false whenever a NaN is involved).  Values are copied, never computed."""
import numpy as np

NO_ARGMAX = np.uint32(0xFFFFFFFF)


def clamp_offsets(off, n):
    """the bags as the kernels clamp them: end = min(off[b + 1], n), begin = min(off[b], end) -> (begin, end) per bag"""
    off = np.asarray(off).astype(np.uint64)
    end = np.minimum(off[1:], np.uint64(n)).astype(np.int64)
    begin = np.minimum(off[:-1], end.astype(np.uint64)).astype(np.int64)
    return begin, end


def pooled_max(rows, off):
    """rows [n, dim] float32 = what find returns per position -> (out [n_bags, dim] float32, argmax [n_bags, dim] uint32: absolute positions)"""
    rows = np.ascontiguousarray(rows, np.float32)
    begin, end = clamp_offsets(off, rows.shape[0])
    lens = end - begin
    out = np.zeros((lens.size, rows.shape[1]), np.float32)            # an empty bag: +0.0 ...
    arg = np.full((lens.size, rows.shape[1]), NO_ARGMAX, np.uint32)   # ... and no position
    with np.errstate(invalid="ignore"):
        for step in range(int(lens.max()) if lens.size else 0):
            live = np.nonzero(lens > step)[0]
            p = begin[live] + step
            v = rows[p]
            take = np.ones(v.shape, bool) if step == 0 else v > out[live]
            out[live] = np.where(take, v, out[live])
            arg[live] = np.where(take, p[:, None].astype(np.uint32), arg[live])
    return out, arg


def pooled_max_backward(off, argmax, bag_grads, grads):
    """writes into grads [n, dim] (prefilled by the caller: positions no bag covers keep what they hold) and returns it: position i of bag b gets
    bag_grads[b, j] where argmax[b, j] == i, +0.0 elsewhere"""
    begin, end = clamp_offsets(off, grads.shape[0])
    for b in range(begin.size):
        for p in range(int(begin[b]), int(end[b])):
            grads[p] = np.where(argmax[b] == np.uint32(p), bag_grads[b], np.float32(0.0))
    return grads


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
