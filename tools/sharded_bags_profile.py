"""usage (GPU box): rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python3 tools/sharded_bags_profile.py
The three bag-run kernels at 1M keys, 64K bags (16 keys each), dim 64, 8 owners emulated in one process; run under rocprofv3 --kernel-trace --stats"""
import sys, os
sys.path.insert(0, os.getcwd())
import numpy as np, torch
from meepoembedding_amd import Router, synth
dev = torch.device("cuda", 0)
G, n, n_bags, dim = 8, 1 << 20, 1 << 16, 64
rng = np.random.default_rng(1)
keys = torch.from_numpy(synth.keys_np(1, 0, 1 << 22)[rng.integers(0, 1 << 22, n)]).to(dev)
off = torch.arange(0, n + 1, n // n_bags, dtype=torch.int64, device=dev)
r = Router(G, n, device=dev)
send, counts, perm = r.partition(keys)
run_bag, run_len, run_counts = r.bag_runs(perm, counts, off)
R = int(run_counts.sum())
partials = torch.randn(R, dim, device=dev)
for it in range(20):
    send, counts, perm = r.partition(keys)
    run_bag, run_len, run_counts = r.bag_runs(perm, counts, off)
    offsets, rok = r.run_offsets(run_len[:R], n)
    out = r.combine_bag_runs(partials, run_bag[:R], run_counts, off, "sum")
    o16 = r.combine_bag_runs(partials, run_bag[:R], run_counts, off, "mean", out_dtype=torch.bfloat16)
torch.cuda.synchronize()
assert int(offsets[-1]) == n and int(rok[-1]) == R - 1
print(f"n {n} bags {n_bags} dim {dim} G {G} runs {R}: combine moves {R * dim * 4 + n_bags * dim * 4 + R * 4} B (fp32 out), {R * dim * 4 + n_bags * dim * 2 + R * 4} B (bf16 out)")
