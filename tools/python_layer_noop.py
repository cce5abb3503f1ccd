"""Host cost of the Python wrappers alone, with a no-op library (profiles/python_buffers.md): python tools/python_layer_noop.py TREE LABEL [cuda]
TREE: a checkout (its meepoembedding_amd/*.py are what is timed; nothing is built or loaded).  The objects are made with __new__ on the CPU device
(with `cuda`: on cuda:0, the tensors there too — their attribute reads are what the checks cost in production; still nothing is launched),
every mee_* call returns 0.  Microseconds per call: the median, min and max of 9 loops of 20 000 calls.  One JSON line: RESULT {...}"""
import json, os, statistics, sys, time
tree, label = os.path.abspath(sys.argv[1]), sys.argv[2]
sys.path.insert(0, tree)
import torch
import meepoembedding_amd as m
from meepoembedding_amd import LookupTable, TableGroup, _lib
from meepoembedding_amd import table as tm
assert os.path.dirname(os.path.abspath(m.__file__)) == os.path.join(tree, "meepoembedding_amd"), m.__file__


class NoOp:
    def __getattr__(self, name):
        fn = lambda *a: 0
        setattr(self, name, fn)
        return fn


noop = NoOp()
_lib.lib = lambda: noop
tm._stream_ptr = lambda device: 0
dev, n, dim = torch.device("cuda", 0) if sys.argv[3:] == ["cuda"] else torch.device("cpu"), 64, 64
t = LookupTable.__new__(LookupTable)
t._h, t.device, t.dim = None, dev, dim
g = TableGroup.__new__(TableGroup)
g._h, g.tables, g.device, g.dim = None, [t, t], dev, dim
keys = torch.arange(n, dtype=torch.int64, device=dev)
out, found, slots = torch.empty(n, dim, device=dev), torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.int64, device=dev)
bags, gbags = torch.arange(0, n + 1, 8, device=dev), torch.arange(0, n + 1, 4, device=dev)
pooled, gpooled = torch.empty(8, dim, device=dev), torch.empty(16, dim, device=dev)
rows = {"find(out=, found=)": lambda: t.find(keys, out=out, found=found),
        "find_located(out=, found=, slots=)": lambda: t.find_located(keys, out=out, found=found, slots=slots),
        "table.find_pooled(out=, found=)": lambda: t.find_pooled(keys, bags, "sum", out=pooled, found=found),
        "group.find_pooled(out=, found=)": lambda: g.find_pooled(keys, gbags, "sum", out=gpooled, found=found),
        "table.find_pooled()": lambda: t.find_pooled(keys, bags, "sum"),
        "find()": lambda: t.find(keys)}
res = {"label": label, "tree": tree, "device": str(dev)}
for name, fn in rows.items():
    for _ in range(2000):
        fn()
    per = []
    for _ in range(9):
        t0 = time.perf_counter()
        for _ in range(20000):
            fn()
        per.append((time.perf_counter() - t0) / 20000 * 1e6)
    res[name] = {"median_us": round(statistics.median(per), 3), "min_us": round(min(per), 3), "max_us": round(max(per), 3)}
print("RESULT " + json.dumps(res), flush=True)
