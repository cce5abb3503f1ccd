"""Weighted pooled lookup (mee_find_pooled_weighted) against the unweighted mee_find_pooled, and the backward kernel
(mee_pooled_weighted_backward) with and without weight grads: 100M keys, dim 64, 256K keys per step, bag lengths 1-40.
usage: python tools/weighted_bag_bench.py [n_keys]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
from meepoembedding_amd import LookupTable, synth

dev = torch.device("cuda", 0)
N, dim, B = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000, 64, 1 << 18
HBM = 8000.0   # GB/s
t = LookupTable(int(N / 0.75), dim, device=dev, max_batch=1 << 20)
bench.populate(t, synth, N, dim, dev, 1 << 20)
batches = bench.lookup_batches(synth, N, B, 8, "uniform", dev, seed=3)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def timed(fn, reps=100):
    for i in range(10):
        fn(i)
    torch.cuda.synchronize()
    e0.record()
    for i in range(reps):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


g = torch.Generator(device=dev)
g.manual_seed(5)
print(f"table {N} keys dim {dim}, {B} keys per step; algorithmic bytes per position: forward 8 key + 128 bucket line + 256 row (+ 4 weight) "
      f"read + 256/L out; backward 4 weight read + 256 grads write (+ 8 handle + 256 row read + 4 weight-grad write)", flush=True)
for name, lens in (("L=1-40 uniform", torch.randint(1, 41, (B // 22,), device=dev, generator=g)),   # mean 20.5: about 244K keys
                   ("L=1", torch.ones(B, dtype=torch.int64, device=dev)),
                   ("L=5", torch.full((B // 5,), 5, dtype=torch.int64, device=dev)),
                   ("L=10", torch.full((B // 10,), 10, dtype=torch.int64, device=dev)),
                   ("L=40", torch.full((B // 40,), 40, dtype=torch.int64, device=dev))):
    off = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(lens, 0)])
    n, nb = int(off[-1]), lens.numel()
    keys = [b[:n].contiguous() for b in batches]
    w = torch.rand(n, device=dev, generator=g) * 2 - 1
    out = torch.empty((nb, dim), device=dev)
    found = torch.empty(n, dtype=torch.uint8, device=dev)
    loc = torch.empty(n, dtype=torch.int64, device=dev)
    bg = torch.randn((nb, dim), device=dev, generator=g)
    grads = torch.empty((n, dim), device=dev)
    wg = torch.empty(n, device=dev)
    t_plain = timed(lambda i: t.find_pooled(keys[i % 8], off, "sum", out=out, found=found))
    t_w = timed(lambda i: t.find_pooled(keys[i % 8], off, out=out, found=found, weights=w))
    t_wl = timed(lambda i: t.find_pooled(keys[i % 8], off, out=out, found=found, weights=w, located=loc))
    t.find_pooled(keys[0], off, out=out, found=found, weights=w, located=loc)
    t_b = timed(lambda i: t.pooled_weighted_backward(keys[0], off, w, bg, grads=grads, want_weight_grads=False))
    t_bw = timed(lambda i: t.pooled_weighted_backward(keys[0], off, w, bg, grads=grads, weight_grads=wg))
    t_bwl = timed(lambda i: t.pooled_weighted_backward(keys[0], off, w, bg, located=loc, grads=grads, weight_grads=wg))
    f_bytes = n * (8 + 128 + 256) + nb * 256
    b_bytes, bw_bytes = n * (4 + 256), n * (4 + 256 + 8 + 256 + 4)
    print(f"{name:15s} ({nb} bags, {n} keys): find_pooled sum {t_plain:.1f} us ({f_bytes / t_plain / 1e3 / HBM:.2f} of HBM), weighted "
          f"{t_w:.1f} us ({(t_w / t_plain - 1) * 100:+.1f} %), weighted + handles {t_wl:.1f} us | backward: grads only {t_b:.1f} us "
          f"({b_bytes / t_b / 1e3 / HBM:.2f} of HBM), + weight grads probing {t_bw:.1f} us ({bw_bytes / t_bw / 1e3 / HBM:.2f} of HBM, the "
          f"probe's 128 B not counted), + weight grads through handles {t_bwl:.1f} us ({bw_bytes / t_bwl / 1e3 / HBM:.2f} of HBM)", flush=True)
