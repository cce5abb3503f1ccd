"""Online learning on one MI355X: a collection trains on a stream while a bf16-row serving copy of it answers lookups, and every few steps the
ids the training touched are published into the serving copy — device to device, no [n, dim] buffer, one launch sequence for the whole collection
(run on the GPU box: python examples/online_serving.py)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import __graft_entry__

__graft_entry__.build()
from meepoembedding_amd import INIT_UNIFORM, OPT_ADAGRAD, LookupTable, TableGroup  # noqa: E402
from meepoembedding_amd.nn import DynamicEmbeddingBag  # noqa: E402

dev = torch.device("cuda", 0)
n_tables, dim, batch, ids_per_bag, vocab = 4, 64, 1024, 4, 100_000

tables = [LookupTable(2 * vocab, dim, device=dev, optimizer=OPT_ADAGRAD, max_batch=1 << 16, initializer=INIT_UNIFORM, init_scale=0.05, init_seed=j)
          for j in range(n_tables)]
trainer = TableGroup(tables, max_apply_batch=n_tables * batch * ids_per_bag)
sparse = DynamicEmbeddingBag(trainer, mode="sum", optimizer="adagrad", lr=0.05, create_missing=True).to(dev)
offsets = torch.arange(0, n_tables * batch * ids_per_bag + 1, ids_per_bag, device=dev)


def train(steps, lo, hi):
    for _ in range(steps):
        ids = torch.randint(lo, hi, (n_tables * batch * ids_per_bag,), device=dev)
        sparse(ids, offsets).square().sum().backward()      # the sparse update happens in here


train(10, 0, vocab // 2)
trainer.track_changes(vocab)               # from here on every step notes its ids, one launch for all members
serving = trainer.serving_copy()           # the replica that answers lookups: bf16 rows, no optimizer state; equal to the trainer (rounded) NOW

for round_ in range(4):
    lo = round_ * vocab // 8
    train(3, lo, lo + vocab // 2)          # known ids move, unseen ids enter
    tables[0].remove(torch.arange(lo, lo + 50, device=dev))               # ... and some leave
    counts = trainer.publish_to(serving, clear=True)                      # one read-back: [(upserts, removed, dropped)] per member
    # the serving copy answers as the trainer would, rows rounded to bf16 once
    ids = torch.randint(0, vocab, (n_tables * batch * ids_per_bag,), device=dev)
    got, found = serving.find_pooled(ids, offsets)
    want, _ = trainer.serving_copy().find_pooled(ids, offsets)            # the full rebuild the publish replaces
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), "the published serving copy differs from a fresh one"
    print(f"round {round_}: published {sum(c[0] for c in counts)} changed rows and {sum(c[1] for c in counts)} removals into "
          f"{sum(t.size() for t in serving.tables)} served keys; {int(found.sum())} of {ids.numel()} requested ids known; pooled lookup equals a fresh serving copy bit for bit")
