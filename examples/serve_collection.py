"""Train -> serve for a recommender's sparse part on one MI355X: a collection trained in fp32 is copied into bf16-row tables, half the row
bytes per key, and served by ONE pooled lookup launch that writes bf16 bag rows straight into the columns of a preallocated feature block (run on
the GPU box: python examples/serve_collection.py)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import __graft_entry__

__graft_entry__.build()
from meepoembedding_amd import INIT_UNIFORM, OPT_ADAGRAD, LookupTable, TableGroup  # noqa: E402

dev = torch.device("cuda", 0)
n_tables, dim, batch, ids_per_bag, vocab = 26, 64, 2048, 5, 10**5

# the trained collection, as examples/recsys_collection.py builds it: fp32 rows + Adagrad state; a few steps' ids enter their tables
tables = [LookupTable(2 * vocab, dim, device=dev, optimizer=OPT_ADAGRAD, max_batch=1 << 18, initializer=INIT_UNIFORM,
                      init_scale=0.05, init_seed=j) for j in range(n_tables)]
train = TableGroup(tables, max_apply_batch=n_tables * batch * 2 * ids_per_bag)


def request():
    """the input pipeline's "jagged" format: all ids concatenated table by table, one offset per (table, sample) bag"""
    lens = torch.randint(1, 2 * ids_per_bag, (n_tables * batch,), device=dev)
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(lens, 0)])
    return torch.randint(0, vocab, (int(offsets[-1]),), device=dev), offsets


for step in range(3):
    ids, offsets = request()
    train.find_or_insert(ids, offsets[::batch].contiguous())            # member offsets = every batch-th bag offset

serve = train.serving_copy()                                             # 26 bf16-row tables in a group of their own; `train` is untouched
ids, offsets = request()
# the server's feature block, allocated once: 16 dense features in front, then the sparse part — the lookup writes its columns in place
n_dense = 16
feature_block = torch.zeros((batch, n_dense + n_tables * dim), dtype=torch.bfloat16, device=dev)
sparse_part = feature_block[:, n_dense:]                                 # a strided view: stride(1) == 1, row stride = the block's width
_, found = serve.find_pooled(ids, offsets, mode="sum", out=sparse_part, out_dtype=torch.bfloat16, layout="keyed")   # ONE launch for the 26 tables
want, _ = train.find_pooled(ids, offsets, mode="sum", layout="keyed")    # the trained fp32 rows, the same [batch, n_tables * dim] layout
print(f"served {ids.numel()} ids in {n_tables * batch} bags -> features {tuple(feature_block.shape)} {feature_block.dtype}, {int(found.sum())} ids known; "
      f"max |bf16-row sum - fp32 sum| = {(sparse_part.float() - want).abs().max().item():.3g}; dense columns untouched: {bool((feature_block[:, :n_dense] == 0).all())}")
print(f"table_bytes: trained fp32 group {sum(t.table_bytes for t in train.tables)} (+ optimizer state), "
      f"bf16-row serving group {sum(t.table_bytes for t in serve.tables)}; keys stored {sum(t.size() for t in serve.tables)}")
