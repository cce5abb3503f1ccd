"""bf16 rows for the sharded lookups, timed at world 1 over real RCCL: mee_sharded_find (fp32), the same followed by .to(bfloat16) (what a
bf16 model does today), mee_sharded_find_as(bf16).  10M keys, dim 64, 1M-key batches, padded layout, HIP events.

    python tools/bench_sharded_bf16.py --out profiles/sharded_bf16_timing.md          # the three timings
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_sharded_bf16.py --trace   # 20 calls of (a) and of (c) for the per-kernel times

World 1 keeps every segment on the device: the run prices the kernels of both forms, not the link (see profiles/sharded_bf16.md)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.distributed as dist

from meepoembedding_amd import LookupTable, synth
from meepoembedding_amd.sharded import RcclShardedTable


def timed(fn, warmup, calls):
    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    torch.cuda.synchronize()
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
    return t[len(t) // 2], t[0], t[int(len(t) * 0.9)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=10_000_000)
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--pad-slack", type=float, default=1.5)
    ap.add_argument("--trace", action="store_true", help="20 calls of the fp32 and of the bf16 lookup and nothing else (for rocprofv3 --kernel-trace --stats)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29577")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    local = LookupTable(2 * a.keys, a.dim, device=dev, max_batch=int(a.batch * a.pad_slack) + 2048)
    for s in range(0, a.keys, a.batch):
        k = synth.keys_t(1, s, min(a.batch, a.keys - s), dev)
        local.insert(k, synth.rows_t(k, a.dim, 2))
    sh = RcclShardedTable(local, a.batch, pad_slack=a.pad_slack)
    g = torch.Generator(device="cpu").manual_seed(5)
    batches = [synth.keys_t(1, 0, a.keys, dev)[torch.randint(0, a.keys, (a.batch,), generator=g).to(dev)] for _ in range(4)]
    o32 = torch.empty((a.batch, a.dim), device=dev)
    o16 = torch.empty((a.batch, a.dim), dtype=torch.bfloat16, device=dev)
    found = torch.empty(a.batch, dtype=torch.uint8, device=dev)
    it = [0]

    def nxt():
        it[0] += 1
        return batches[it[0] % len(batches)]

    f_a = lambda: sh.find(nxt(), out=o32, found=found)
    f_b = lambda: sh.find(nxt(), out=o32, found=found)[0].to(torch.bfloat16)
    f_c = lambda: sh.find(nxt(), out=o16, found=found, out_dtype=torch.bfloat16)
    if a.trace:
        for f in (f_a, f_c):
            for _ in range(20):
                f()
        torch.cuda.synchronize()
    else:
        # correctness of what is timed: (c) is (a) rounded, bit for bit
        k = batches[0]
        ra = sh.find(k)[0].to(torch.bfloat16)
        rc = sh.find(k, out_dtype=torch.bfloat16)[0]
        assert torch.equal(ra.view(torch.int16), rc.view(torch.int16)) and sh.status() == 0
        rows = []
        for rep in range(2):     # twice, interleaved: drift between the forms shows as a difference between the rounds
            for name, f in (("(a) mee_sharded_find, fp32", f_a), ("(b) (a) + .to(torch.bfloat16)", f_b), ("(c) mee_sharded_find_as, bf16", f_c)):
                med, lo, p90 = timed(f, a.warmup, a.calls)
                rows.append((rep, name, med, lo, p90))
        lines = [f"world 1 over RCCL, {a.keys} keys, dim {a.dim}, {a.batch}-key batches, padded layout (pad_slack {a.pad_slack}), {a.warmup} warm-up + {a.calls} timed calls, HIP events, us per call",
                 f"device: {torch.cuda.get_device_name(dev)}", "", "| round | form | median | min | p90 |", "|---|---|---|---|---|"]
        lines += [f"| {rep} | {name} | {med:.1f} | {lo:.1f} | {p90:.1f} |" for rep, name, med, lo, p90 in rows]
        txt = "\n".join(lines) + "\n"
        print(txt)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            open(a.out, "w").write(txt)
    sh.close()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
