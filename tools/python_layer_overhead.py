"""Host cost of the Python layer on the training step, for A/B runs of two trees in one session (profiles/python_layer_refactor.md):
    python tools/python_layer_overhead.py TREE LABEL        (TREE: a checkout with its built libmeepo_hip.so; one process per run, parent / new / parent)
1. enqueue-only loops, tiny batches (the host is the bottleneck): find_located(prepare_apply=True) + apply_adagrad / apply_adam(slots=)
2. one DynamicEmbeddingCollection step (forward + backward) over 26 small tables
3. bench.py's own training step (train_streams) on an 8M-key table, both optimizers
One JSON line: RESULT {...}"""
import json, os, statistics, sys, time
tree, label = os.path.abspath(sys.argv[1]), sys.argv[2]
sys.path.insert(0, tree)
import torch
import bench
import meepoembedding_amd as m
from meepoembedding_amd import LookupTable, TableGroup, OPT_ADAGRAD, OPT_ADAM, synth
from meepoembedding_amd.nn import DynamicEmbeddingCollection
assert os.path.dirname(os.path.abspath(m.__file__)) == os.path.join(tree, "meepoembedding_amd"), m.__file__
dev = torch.device("cuda", 0)
res = {"label": label, "tree": tree}

def enqueue_us(fn, iters=20000, reps=7, warm=2000):
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(iters): fn()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        out.append((t1 - t0) / iters * 1e6)
    return {"median_us": round(statistics.median(out), 3), "min_us": round(min(out), 3), "max_us": round(max(out), 3)}

# 1. enqueue-only: the training step's two wrapper calls on a tiny batch (the GPU side is shorter than the host side: the loop times the host)
for opt, name in ((OPT_ADAGRAD, "adagrad"), (OPT_ADAM, "adam")):
    t = LookupTable(1 << 16, 64, device=dev, max_batch=1 << 12, optimizer=opt)
    k = synth.keys_t(1, 0, 64, dev)
    t.insert(k, torch.zeros(64, 64, device=dev))
    out = torch.empty((64, 64), device=dev); found = torch.empty(64, dtype=torch.uint8, device=dev); slots = torch.empty(64, dtype=torch.int64, device=dev)
    g = torch.zeros(64, 64, device=dev)
    if name == "adagrad":
        def step():
            t.find_located(k, out=out, found=found, slots=slots, prepare_apply=True)
            t.apply_adagrad(k, g, lr=0.01, eps=1e-10, slots=slots)
    else:
        def step():
            t.find_located(k, out=out, found=found, slots=slots, prepare_apply=True)
            t.apply_adam(k, g, lr=0.001, step=3, slots=slots)
    res[f"enqueue_find_located_prepare+apply_{name}_slots"] = enqueue_us(step)
    t.close()

# 2. one DynamicEmbeddingCollection step (forward + backward) over 26 small tables
tables = [LookupTable(1 << 12, 16, device=dev, max_batch=1 << 12, optimizer=OPT_ADAGRAD) for _ in range(26)]
group = TableGroup(tables, max_apply_batch=1 << 12)
layer = DynamicEmbeddingCollection(group, lr=0.01).to(dev)
keys = synth.keys_t(2, 0, 26 * 8, dev)
offs = torch.arange(0, 26 * 8 + 1, 8, dtype=torch.int64, device=dev)
def coll_step():
    layer(keys, offs).sum().backward()
res["collection_step_26_tables"] = enqueue_us(coll_step, iters=2000, reps=7, warm=200)
group.close()

# 3. bench.py's own training step (train_streams: find_located(prepare) + apply on the slots), both optimizers, on a small table
n_keys, batch, dim = 8_000_000, 1 << 18, 64
for opt, name in ((OPT_ADAGRAD, "adagrad"), (OPT_ADAM, "adam")):
    t = LookupTable(int(n_keys / 0.75), dim, device=dev, max_batch=1 << 20, optimizer=opt)
    bench.populate(t, synth, n_keys, dim, dev, 1 << 20)
    out = torch.empty((batch, dim), device=dev); found = torch.empty(batch, dtype=torch.uint8, device=dev)
    rows = bench.train_streams(t, synth, n_keys, batch, dim, dev, out, found, 528, opt=name)
    sfx = "" if name == "adagrad" else "_adam"
    res[f"bench_train_streams_{name}"] = {s: {lab: round(rows[s][lab]["us"], 2) for lab in ("step" + sfx, "apply_alone" + sfx)} for s in ("uniform", "zipf_1.05")}
    t.close(); torch.cuda.empty_cache()
print("RESULT " + json.dumps(res), flush=True)
