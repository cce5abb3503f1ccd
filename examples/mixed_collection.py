"""A recommender's sparse part with per-feature embedding widths on one MI355X: six tables of widths 8 / 64 / 128 behind one MixedTableGroup —
one pooled lookup launch for all of them, which writes the [batch, sum(dims)] block the dense network reads (run on the GPU box:
python examples/mixed_collection.py)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import __graft_entry__

__graft_entry__.build()
from meepoembedding_amd import INIT_UNIFORM, OPT_ADAGRAD, LookupTable, MixedTableGroup  # noqa: E402
from meepoembedding_amd.nn import DynamicEmbeddingBag  # noqa: E402

dev = torch.device("cuda", 0)
dims = (8, 64, 128, 64, 8, 128)          # a tiny categorical, id features, a wide one: the caller's order is kept for ids and results
batch, ids_per_bag, vocab = 512, 5, 10**5

tables = [LookupTable(2 * vocab, d, device=dev, optimizer=OPT_ADAGRAD, max_batch=1 << 16, initializer=INIT_UNIFORM,
                      init_scale=0.05, init_seed=j) for j, d in enumerate(dims)]
group = MixedTableGroup(tables, max_apply_batch=len(dims) * batch * 2 * ids_per_bag)   # an upper bound on the ids of one step
sparse = DynamicEmbeddingBag(group, mode="sum", optimizer="adagrad", lr=0.05, create_missing=True, layout="keyed").to(dev)   # bag b -> table b // batch
dense = torch.nn.Sequential(torch.nn.Linear(sum(dims), 128), torch.nn.ReLU(), torch.nn.Linear(128, 1)).to(dev)
dense_opt = torch.optim.SGD(dense.parameters(), lr=0.01)

for step in range(4):
    lens = torch.randint(1, 2 * ids_per_bag, (len(dims) * batch,), device=dev)
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(lens, 0)])
    ids = torch.randint(0, vocab, (int(offsets[-1]),), device=dev)
    labels = torch.rand(batch, 1, device=dev)
    features = sparse(ids, offsets)                                      # [batch, sum(dims)]: table j's pooled rows in columns sum(dims[:j]) ...
    loss = torch.nn.functional.binary_cross_entropy_with_logits(dense(features), labels)
    dense_opt.zero_grad()
    loss.backward()                                                      # the sparse update — one launch takes the gradient apart, then per width a select launch and the grouped step
    dense_opt.step()
    print(f"step {step}: loss {loss.item():.4f}, ids {ids.numel()}, keys stored {[t.size() for t in tables]}")
group.close()
