"""Sequence features on one MI355X: 4 history tables, ONE padded lookup launch writes the [tables * batch, max_len, dim] block an attention layer
reads, and one indexed optimizer step trains the ids that were kept (run on the GPU box: python examples/sequence_collection.py)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import __graft_entry__

__graft_entry__.build()
from meepoembedding_amd import INIT_UNIFORM, OPT_ADAGRAD, LookupTable, TableGroup  # noqa: E402
from meepoembedding_amd.nn import DynamicEmbeddingSequence  # noqa: E402

dev = torch.device("cuda", 0)
n_tables, dim, batch, max_len, mean_len, vocab = 4, 64, 512, 20, 8, 10**5

tables = [LookupTable(2 * vocab, dim, device=dev, optimizer=OPT_ADAGRAD, max_batch=1 << 18, initializer=INIT_UNIFORM,
                      init_scale=0.05, init_seed=j) for j in range(n_tables)]
group = TableGroup(tables, max_apply_batch=1 << 18)
# histories run oldest -> newest: keep="last" keeps the recent end of one that is longer than max_len; new ids enter their tables in forward
sparse = DynamicEmbeddingSequence(group, max_len, keep="last", optimizer="adagrad", lr=0.05, create_missing=True).to(dev)
query = torch.nn.Parameter(torch.randn(dim, device=dev) * 0.1)
head = torch.nn.Linear(n_tables * dim, 1).to(dev)
dense_opt = torch.optim.SGD([query, *head.parameters()], lr=0.01)

for step in range(5):
    # the input pipeline's "jagged" format: all ids concatenated table by table, one offset per (table, sample) history; some are longer than max_len
    lens = torch.poisson(torch.full((n_tables * batch,), float(mean_len), device=dev)).to(torch.int64) * (1 + 3 * (torch.rand(n_tables * batch, device=dev) < 0.05))
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(lens, 0)])
    ids = torch.randint(0, vocab, (int(offsets[-1]),), device=dev)
    labels = torch.rand(batch, 1, device=dev)
    padded, lengths = sparse(ids, offsets)                               # [n_tables * batch, max_len, dim], [n_tables * batch]
    mask = torch.arange(max_len, device=dev)[None, :] < lengths[:, None]
    scores = (padded @ query).masked_fill(~mask, float("-inf"))          # one attention query over every history
    weights = torch.nan_to_num(torch.softmax(scores, dim=1))              # (an empty history attends to nothing)
    summary = (weights[:, :, None] * padded).sum(1)                      # [n_tables * batch, dim]
    features = summary.view(n_tables, batch, dim).transpose(0, 1).reshape(batch, n_tables * dim)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(head(features), labels)
    dense_opt.zero_grad()
    loss.backward()                                                      # the sparse update (one indexed grouped step) happens in here
    dense_opt.step()
    print(f"step {step}: loss {loss.item():.4f}, ids {ids.numel()}, kept {int(lengths.sum())}, keys stored {sum(t.size() for t in tables)}")
