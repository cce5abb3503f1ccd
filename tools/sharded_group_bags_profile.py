"""usage (GPU box):
    python3 tools/sharded_group_bags_profile.py kernel
    python3 tools/sharded_group_bags_profile.py step
kernel: mee_group_find_pooled_jagged with the regular member map [0, B, 2B, …] against mee_group_find_pooled of the same build on the same batch:
        26 tables x 4096 bags, dim 64, about 20 keys per bag (the wave-per-bag launch shape), and about 6 keys per bag (the tile-per-bag shape).
        The two alternate in one process; device time by events, 7 rounds of 20 launches each: the median round and the spread of the rounds.
step:   world 1 over the nccl backend: find_pooled + Adagrad apply_pooled of ONE ShardedTableGroup against a loop of 26 ShardedLookupTable
        find_pooled + apply_adagrad(grad_index=) calls on the same bags; medians of host-clock times that end in a device synchronise."""
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

from meepoembedding_amd import OPT_ADAGRAD, LookupTable, Router, TableGroup, synth

dev = torch.device("cuda", 0)
T, dim = 26, 64


def tables_of(stored, n_max, optimizer=0):
    out = []
    for j in range(T):
        kw = dict(optimizer=OPT_ADAGRAD, initial_accumulator=0.1) if optimizer else {}
        t = LookupTable(1 << 18, dim, device=dev, max_batch=n_max, **kw)
        t.insert(torch.from_numpy(stored).to(dev), torch.from_numpy(synth.rows_np(stored, dim, 2 + j)).to(dev))
        out.append(t)
    return out


def bags(B, mean_len, rng, stored):
    lens = rng.poisson(mean_len, T * B)
    keys = torch.from_numpy(stored[rng.integers(0, stored.size, int(lens.sum()))]).to(dev)
    return keys, torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)).to(dev)


def kernel():
    rng = np.random.default_rng(1)
    stored = synth.keys_np(1, 0, 100_000)
    group = TableGroup(tables_of(stored, 1 << 17))
    B = 4096
    for mean_len in (20, 6):
        keys, off = bags(B, mean_len, rng, stored)
        n, n_bags = keys.numel(), T * B
        member_bags = torch.arange(T + 1, dtype=torch.int64, device=dev) * B
        out = torch.empty((n_bags, dim), device=dev)
        found = torch.empty(n, dtype=torch.uint8, device=dev)
        forms = {"regular": lambda: group.find_pooled(keys, off, "sum", out=out, found=found),
                 "jagged": lambda: group.find_pooled_jagged(keys, off, member_bags, "sum", out=out, found=found)}
        ref = group.find_pooled(keys, off, "sum")[0].clone()
        assert torch.equal(group.find_pooled_jagged(keys, off, member_bags, "sum")[0], ref)
        rounds = {k: [] for k in forms}
        for r in range(2 + 7):      # 2 warm-up rounds
            for name, fn in forms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(20):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                if r >= 2:
                    rounds[name].append(e0.elapsed_time(e1) / 20 * 1e3)
        med = {k: float(np.median(v)) for k, v in rounds.items()}
        for name, v in rounds.items():
            print(f"{n_bags} bags x ~{mean_len} keys ({n} keys) dim {dim} {name}: median {med[name]:.1f} us per launch, rounds {min(v):.1f} … {max(v):.1f} us "
                  f"(spread {(max(v) - min(v)) / med[name] * 100:.1f} %)")
        print(f"~{mean_len} keys per bag: jagged / regular = {med['jagged'] / med['regular']:.3f}")


def step():
    import torch.distributed as dist

    from meepoembedding_amd.sharded import ShardedLookupTable, ShardedTableGroup
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29534")
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    rng = np.random.default_rng(2)
    stored = synth.keys_np(1, 0, 100_000)
    n_max = 1 << 22
    tables = tables_of(stored, n_max, optimizer=1)
    router = Router(1, n_max, device=dev)
    singles = [ShardedLookupTable(t, router) for t in tables]
    sg = ShardedTableGroup(TableGroup(tables, max_apply_batch=n_max), router)
    for B in (256, 4096):
        keys, off = bags(B, 20, rng, stored)
        n = keys.numel()
        grads = torch.randn(T * B, dim, device=dev) * 0.01
        bag_of = torch.repeat_interleave(torch.arange(T * B, device=dev), off[1:] - off[:-1])
        o = off.tolist()
        segs = []
        for j in range(T):
            a, b = o[j * B], o[(j + 1) * B]
            segs.append((keys[a:b].contiguous(), (off[j * B:(j + 1) * B + 1] - a).contiguous(), grads[j * B:(j + 1) * B].contiguous(),
                         (bag_of[a:b] - j * B).contiguous()))

        def loop_step():
            for sh, (k, bo, g, gi) in zip(singles, segs):
                sh.find_pooled(k, bo, "sum")
                sh.apply_adagrad(k, g, 0.01, grad_index=gi)

        def group_step():
            sg.find_pooled(keys, off, "sum")
            sg.apply_pooled(keys, off, grads, bag_of, "adagrad", 0.01)

        times = {"loop": [], "group": []}
        for it in range(3 + 15):      # 3 warm-up rounds, then 15 timed ones, the two forms alternating
            for name, fn in (("loop", loop_step), ("group", group_step)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if it >= 3:
                    times[name].append((time.perf_counter() - t0) * 1e3)
        c0 = sg.collectives
        group_step()
        for name, ts in times.items():
            ts = np.array(ts)
            print(f"{T} x {B} bags x ~20 keys ({n} keys) dim {dim} world 1 {name}: median {np.median(ts):.3f} ms, min {ts.min():.3f}, max {ts.max():.3f} over {ts.size} steps")
        print(f"B {B}: collectives per group step {sg.collectives - c0} (loop: {9 * T}); median loop / group = {np.median(times['loop']) / np.median(times['group']):.2f}")
    dist.destroy_process_group()


if __name__ == "__main__":
    {"kernel": kernel, "step": step}[sys.argv[1]]()
