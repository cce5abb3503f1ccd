"""Incremental checkpoints of a trained collection on one MI355X: a base, two deltas that carry only what changed, and a restore into tables of
another capacity (run on the GPU box: python examples/incremental_checkpoint.py)."""
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import __graft_entry__

__graft_entry__.build()
from meepoembedding_amd import INIT_UNIFORM, OPT_ADAGRAD, LookupTable, TableGroup, checkpoint  # noqa: E402
from meepoembedding_amd.nn import DynamicEmbeddingBag  # noqa: E402

dev = torch.device("cuda", 0)
n_tables, dim, batch, ids_per_bag, vocab = 3, 64, 1024, 4, 200_000


def make_tables(capacity):
    return [LookupTable(capacity, dim, device=dev, optimizer=OPT_ADAGRAD, max_batch=1 << 16, initializer=INIT_UNIFORM, init_scale=0.05, init_seed=j)
            for j in range(n_tables)]


tables = make_tables(2 * vocab)
group = TableGroup(tables, max_apply_batch=n_tables * batch * ids_per_bag)
group.track_changes(vocab)                 # one change log per member; the group's steps note a whole jagged batch in all of them with one launch
sparse = DynamicEmbeddingBag(group, mode="sum", optimizer="adagrad", lr=0.05, create_missing=True).to(dev)


def train(steps, lo, hi):
    for _ in range(steps):
        offsets = torch.arange(0, n_tables * batch * ids_per_bag + 1, ids_per_bag, device=dev)
        ids = torch.randint(lo, hi, (n_tables * batch * ids_per_bag,), device=dev)
        sparse(ids, offsets).square().sum().backward()      # the sparse update happens in here


def sorted_export(t):
    e = [x.cpu().numpy() for x in t.export(with_state=True) if x is not None]
    order = np.argsort(e[0])
    return [x[order] for x in e]


with tempfile.TemporaryDirectory() as root:
    path = lambda kind, j: os.path.join(root, f"{kind}-table{j}")
    train(20, 0, vocab // 2)
    for j, t in enumerate(tables):
        print(f"table {j}: base of {checkpoint.save_base(t, path('base', j))} keys")
    for d, (lo, hi) in enumerate([(vocab // 4, 3 * vocab // 4), (vocab // 2, vocab)], start=1):
        train(5, lo, hi)
        tables[0].remove(torch.arange(lo, lo + 100, device=dev))          # a member's own mutators note in the same log
        for j, t in enumerate(tables):
            n, r = checkpoint.save_delta(t, path(f"delta{d}", j))
            print(f"table {j}: delta {d} carries {n} of {t.size()} keys and {r} removed keys")
    restored = make_tables(3 * vocab)      # another capacity: a delta names keys, not slots
    for j, t in enumerate(restored):
        checkpoint.restore(t, path("base", j), [path("delta1", j), path("delta2", j)])
        same = all(np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
                   for a, b in zip(sorted_export(tables[j]), sorted_export(t)))
        print(f"table {j}: restored {t.size()} keys, rows and accumulators bit for bit equal to the trained table: {same}")
        assert same
