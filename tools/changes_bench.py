"""Change log and delta export (SPEC.md §3 "Change log"): what tracking costs a training step, what the native delta export gains over the
composition it replaces, and what a delta checkpoint saves over a full one.  Numbers go to profiles/changes.md.

  step     the configs[2]-shaped step — 256K keys, dim 64, located find (its launch partitions the batch) + sparse Adagrad on the slots — on a uniform
           and a Zipf(1.05) stream over --keys keys, without a log and with one attached, the two taking turns; median and min .. max of --regions
           HIP-event windows of --steps steps.  --untracked-only: the untracked step alone (run it under MEE_LIB_PATH=<another build>
           MEE_LIB_OLDER_BUILD=1 for the same step on another commit's library).
  export   ChangeLog.iter_changed of 256K and 4M changed keys on the same table against the composition on the same tree: per chunk of max_batch raw
           noted keys dedup_keys + find + find_plane(1) + a boolean-mask compaction in torch (one host synchronisation per chunk, three [n, dim]
           buffers); both deliver (keys, values, state1, removed) on the device; the forms take turns.
  size     save_delta against save_table: bytes on disk and wall time for a --size-keys table after --size-steps tracked steps.

usage: python tools/changes_bench.py step|export|size [--keys 25000000] [--out DIR]"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("what", choices=["step", "export", "size"])
ap.add_argument("--keys", type=int, default=25_000_000)
ap.add_argument("--batch", type=int, default=1 << 18)
ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--regions", type=int, default=7)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--untracked-only", action="store_true")
ap.add_argument("--size-keys", type=int, default=2_000_000)
ap.add_argument("--size-steps", type=int, default=100)
ap.add_argument("--tmp", type=str, default=None, help="directory for the checkpoints of `size` (default: a temporary directory)")
args = ap.parse_args()
DIM, MB = 64, 1 << 20


def filled(n_keys, dev):
    import torch  # noqa: F401

    from meepoembedding_amd import OPT_ADAGRAD, LookupTable, synth
    t = LookupTable(int(n_keys / 0.75), DIM, device=dev, optimizer=OPT_ADAGRAD, max_batch=MB, initial_accumulator=0.1)
    for s in range(0, n_keys, MB):
        k = synth.keys_t(1, s, min(MB, n_keys - s), dev)
        t.insert(k, synth.rows_t(k, DIM, 2))
    return t


def batches(n_keys, n, dist, dev, seed):
    """bench.py's key streams: uniform, or Zipf(1.05) by key index"""
    import torch

    from meepoembedding_amd import synth
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    out = []
    for _ in range(n):
        if dist == "zipf":
            a = 1.05
            u = torch.rand(args.batch, device=dev, generator=g, dtype=torch.float64)
            r = (1 + u * (float(n_keys) ** (1 - a) - 1)) ** (1 / (1 - a))
            idx = (r.floor().to(torch.int64) - 1).clamp_(0, n_keys - 1)
        else:
            idx = torch.randint(0, n_keys, (args.batch,), device=dev, generator=g)
        out.append(synth.mix64_t((idx + 1) * synth._s64(synth._GOLDEN) + synth._s64(1)))
    return out


def spread(vs):
    return {"median_us": statistics.median(vs), "min_us": min(vs), "max_us": max(vs)}


def bench_step(dev):
    import torch

    from meepoembedding_amd.changes import ChangeLog
    t = filled(args.keys, dev)
    log = ChangeLog(8 * args.batch * 2, dev)
    out = torch.empty((args.batch, DIM), device=dev)
    found = torch.empty(args.batch, dtype=torch.uint8, device=dev)
    slots = torch.empty(args.batch, dtype=torch.int64, device=dev)
    grads = [torch.randn(args.batch, DIM, device=dev) * 0.01 for _ in range(4)]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    res = {}
    for dist in ("uniform", "zipf"):
        bs = batches(args.keys, 8, dist, dev, seed=11)

        def step(i):
            t.find_located(bs[i % 8], out=out, found=found, slots=slots, prepare_apply=True)
            t.apply_adagrad(bs[i % 8], grads[i % 4], lr=0.01, eps=1e-10, slots=slots)

        modes = {"untracked": None} if args.untracked_only else {"untracked": None, "tracked": log}
        ts = {m: [] for m in modes}
        for region in range(args.regions + 1):     # the first region warms up
            for m, lg in modes.items():            # the modes take turns
                t.change_log = lg
                for i in range(5):
                    step(i)
                torch.cuda.synchronize(dev)
                e0.record()
                for i in range(args.steps):
                    step(i)
                e1.record()
                torch.cuda.synchronize(dev)
                if region:
                    ts[m].append(e0.elapsed_time(e1) * 1e3 / args.steps)
        t.change_log = None
        res[dist] = {m: spread(v) for m, v in ts.items()}
        if not args.untracked_only:
            res[dist]["added_us"] = res[dist]["tracked"]["median_us"] - res[dist]["untracked"]["median_us"]
            res[dist]["log_size"] = log.size()
            assert not log.invalid
            log.clear()
    assert t.status() == 0
    return res


def bench_export(dev):
    import torch

    from meepoembedding_amd import _lib, synth
    from meepoembedding_amd.changes import ChangeLog
    t = filled(args.keys, dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        e0.record()
        r = fn()
        e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1) * 1e3, r

    def composed(raw):
        """the delta of the raw noted stream with the operators the tree had before: per chunk 4 library launches, torch's compaction, one sync"""
        pieces = []
        for s in range(0, raw.numel(), MB):
            uniq, _ = t.dedup_keys(raw[s:s + MB])
            vals, found = t.find(uniq)
            acc, _ = t.find_plane(1, uniq)
            held, gone = found.bool(), (uniq != _lib.EMPTY_KEY) & ~found.bool()
            pieces.append((uniq[held], vals[held], acc[held], uniq[gone]))       # (a key that two chunks hold comes out twice: the caller's problem)
        return sum(p[0].numel() + p[3].numel() for p in pieces)

    res = {}
    for n in (1 << 18, 1 << 22):
        if n > args.keys:
            continue
        idx = torch.randperm(args.keys, device=dev)[:n]
        present = synth.mix64_t((idx + 1) * synth._s64(synth._GOLDEN) + synth._s64(1))
        absent = synth.keys_t(77, 0, n // 16, dev)                                  # noted, not held: the removed list
        changed = torch.cat([present, absent])
        raw = torch.cat([changed, changed[: n // 4]])[torch.randperm(changed.numel() + n // 4, device=dev)]   # the stream as the mutators saw it: 25 % repeats
        log = ChangeLog(2 * changed.numel(), dev)
        for s in range(0, raw.numel(), MB):
            log.note(raw[s:s + MB])
        assert log.size() == changed.numel() and not log.invalid
        forms = {"native iter_changed": lambda: sum(p[0].numel() + p[4].numel() for p in log.iter_changed(t, 1 << 22)),
                 "composition": lambda: composed(raw)}
        ts = {f: [] for f in forms}
        for rep in range(args.reps + 2):           # two warm-up rounds
            for f, fn in forms.items():
                us, m = timed(fn)
                assert m >= changed.numel() if f == "composition" else m == changed.numel(), (f, m)
                if rep >= 2:
                    ts[f].append(us)
        chunks_native, chunks_comp = -(-log.capacity // (1 << 22)), -(-raw.numel() // MB)
        res[f"{n} changed keys"] = {
            "native iter_changed": {**spread(ts["native iter_changed"]), "library_launches": 2 * chunks_native, "syncs": chunks_native,
                                    "n_dim_buffers_per_chunk": 2},
            "composition": {**spread(ts["composition"]), "library_launches": 4 * chunks_comp, "syncs": chunks_comp, "n_dim_buffers_per_chunk": 4,
                            "note": "plus torch's mask compaction: 2 [n, dim] gathers and 2 key gathers per chunk"},
            "log_slots": log.capacity}
    return res


def dir_bytes(path):
    return sum(os.path.getsize(os.path.join(path, f)) for f in os.listdir(path))


def bench_size(dev):
    import torch

    from meepoembedding_amd import checkpoint
    t = filled(args.size_keys, dev)
    tmp = args.tmp or tempfile.mkdtemp(prefix="changes_bench_")
    res = {}
    grads = torch.randn(args.batch, DIM, device=dev) * 0.01
    try:
        for dist in ("zipf", "uniform"):
            t.change_log = None
            t.track_changes(min(args.size_keys, args.size_steps * args.batch) * 2)
            base, delta, full = (os.path.join(tmp, f"{dist}_{x}") for x in ("base", "delta", "full"))
            checkpoint.save_base(t, base)
            bs = batches(args.size_keys, 8, dist, dev, seed=5)
            for i in range(args.size_steps):
                t.apply_adagrad(bs[i % 8], grads, lr=0.01)
            torch.cuda.synchronize(dev)
            changed = t.change_log.size()
            t0 = time.perf_counter()
            n, r = checkpoint.save_delta(t, delta)
            t1 = time.perf_counter()
            pairs = checkpoint.save_table(t, full)
            t2 = time.perf_counter()
            assert n == changed and r == 0
            res[dist] = {"steps": args.size_steps, "table_keys": pairs, "changed_keys": n,
                         "save_delta": {"bytes": dir_bytes(delta), "wall_s": t1 - t0}, "save_table": {"bytes": dir_bytes(full), "wall_s": t2 - t1}}
            for d in (base, delta, full):
                shutil.rmtree(d)
    finally:
        if not args.tmp:
            shutil.rmtree(tmp, ignore_errors=True)
    return res


def main():
    import torch
    assert torch.cuda.is_available(), "changes_bench.py measures on the GPU: there is nothing to report without one"
    dev = torch.device("cuda", 0)
    res = {"step": bench_step, "export": bench_export, "size": bench_size}[args.what](dev)
    print("RESULT " + json.dumps({args.what: res, "keys": args.size_keys if args.what == "size" else args.keys, "batch": args.batch, "dim": DIM,
                                  "lib": os.environ.get("MEE_LIB_PATH", "this tree")}), flush=True)


if __name__ == "__main__":
    main()
