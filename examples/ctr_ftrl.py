"""A CTR model's sparse part trained with FTRL-Proximal on one MI355X: dim-8 and dim-16 tables (different widths: a MixedTableGroup) with zero
initial rows behind one DynamicEmbeddingBag(optimizer="ftrl"); the L1 term leaves the coordinates of rarely seen ids at exactly 0.0 (run on the
GPU box: python examples/ctr_ftrl.py)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import __graft_entry__

__graft_entry__.build()
from meepoembedding_amd import OPT_FTRL, LookupTable, MixedTableGroup, synth  # noqa: E402
from meepoembedding_amd.nn import DynamicEmbeddingBag  # noqa: E402

dev = torch.device("cuda", 0)
dims, batch, ids_per_bag, vocab = (8, 16, 8, 16), 512, 4, 20_000
tables = [LookupTable(2 * vocab, d, device=dev, optimizer=OPT_FTRL, max_batch=1 << 16, initial_accumulator=0.1) for d in dims]   # new ids: row 0, z 0, n 0.1
group = MixedTableGroup(tables, max_apply_batch=len(dims) * batch * ids_per_bag)
sparse = DynamicEmbeddingBag(group, optimizer="ftrl", lr=0.05, eps=1.0, l1=5e-4, l2=0.001, create_missing=True, layout="keyed").to(dev)   # eps = FTRL's beta
dense = torch.nn.Sequential(torch.nn.Linear(sum(dims), 32), torch.nn.ReLU(), torch.nn.Linear(32, 1)).to(dev)
dense_opt = torch.optim.SGD(dense.parameters(), lr=0.005)
offsets = torch.arange(0, len(dims) * batch * ids_per_bag + 1, ids_per_bag, device=dev)
for step in range(20):
    u = torch.rand(len(dims) * batch * ids_per_bag, device=dev)
    ids = synth.keys_t(1, 0, vocab, dev)[(u ** 3 * vocab).long()]           # skewed: a few ids are seen at every step, most of them rarely
    labels = (ids.view(len(dims), batch, ids_per_bag)[0, :, :1] % 2).float()
    loss = torch.nn.functional.binary_cross_entropy_with_logits(dense(sparse(ids, offsets)), labels, reduction="sum") / 32
    dense_opt.zero_grad()
    loss.backward()                                                        # the FTRL step of every table happens in here
    dense_opt.step()
for d, t in zip(dims, tables):
    rows = t.export()[1]
    print(f"dim {d}: {t.size()} ids stored, {(rows == 0).float().mean().item():.1%} of their elements exactly zero; loss {loss.item():.4f}")
group.close()
