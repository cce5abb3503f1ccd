"""A recommender's sparse part whose tables do not fit HBM: 8 tables, each a hot/cold pair (hot rows in HBM, cold rows in pinned host
memory), served by ONE pooled lookup launch and trained by two grouped optimizer steps per batch, whatever the number of tables; then the
same pairs behind a DynamicEmbeddingCollection, which returns a row per id (a sequence feature) from one launch, and behind a
DynamicEmbeddingSequence, which returns the padded [n_bags, max_len, dim] block of histories of different lengths from one launch.  The first two layers admit: an unseen id enters its pair only once the pair's hot table's sketch has
seen it asked for min_count times — a skewed stream's once-seen tail stays out of both tiers
(run on the GPU box: python examples/tiered_collection.py [min_count, default 2; 0 = create at first sight, no admission])."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import __graft_entry__

__graft_entry__.build()
from meepoembedding_amd import INIT_UNIFORM, OPT_ADAGRAD, LookupTable, TieredLookupTable, TieredTableGroup, _lib  # noqa: E402
from meepoembedding_amd.nn import DynamicEmbeddingBag, DynamicEmbeddingCollection, DynamicEmbeddingSequence  # noqa: E402

dev = torch.device("cuda", 0)
n_tables, dim, batch, ids_per_bag, vocab = 8, 64, 2048, 5, 400_000
max_ids = n_tables * batch * 2 * ids_per_bag       # an upper bound on the ids of one step
min_count = (int(sys.argv[1]) if len(sys.argv) > 1 else 2) or None


def table(capacity, j, **kw):
    return LookupTable(capacity, dim, device=dev, optimizer=OPT_ADAGRAD, max_batch=max_ids, initializer=INIT_UNIFORM, init_scale=0.05,
                       init_seed=j, track_hits=True, **kw)      # track_hits on both tiers: the placement policy


# New ids are created hot while a pair has room for a whole batch of them (the host's only bound on a member's new ids is the size of the batch:
# conservative, and free of synchronisation), then cold; rebalance() promotes the cold ids the lookups keep hitting.
# Admission: the pair's sketch is its HOT table's, so only the hot tables are created with one.
pairs = [TieredLookupTable(table(1 << 18, j, admission=True), table(2 * vocab, j, value_memory=_lib.MEM_HOST_PINNED), hot_key_limit=120_000)
         for j in range(n_tables)]
group = TieredTableGroup(pairs, max_apply_batch=max_ids)
sparse = DynamicEmbeddingBag(group, mode="sum", optimizer="adagrad", lr=0.05, create_missing=True, min_count=min_count).to(dev)   # bag b -> pair b // batch
dense = torch.nn.Sequential(torch.nn.Linear(n_tables * dim, 256), torch.nn.ReLU(), torch.nn.Linear(256, 1)).to(dev)
dense_opt = torch.optim.SGD(dense.parameters(), lr=0.01)

for step in range(8):
    lens = torch.randint(1, 2 * ids_per_bag, (n_tables * batch,), device=dev)
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(lens, 0)])
    ids = (torch.rand(int(offsets[-1]), device=dev) ** 3 * vocab).long()      # a skewed stream: small ids are popular
    labels = torch.rand(batch, 1, device=dev)
    pooled = sparse(ids, offsets)        # found mask, count + creation of the admitted unseen ids (hot while there is room, else cold), pooled lookup
    features = pooled.view(n_tables, batch, dim).transpose(0, 1).reshape(batch, n_tables * dim)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(dense(features), labels)
    dense_opt.zero_grad()
    loss.backward()                      # the sparse update: one grouped step over the hot tables, one over the cold tables
    dense_opt.step()
    moved = group.rebalance() if step % 2 == 1 else None      # between steps: promote the cold ids the lookups hit — at most two grouped moves for all pairs
    print(f"step {step}: loss {loss.item():.4f}, ids {ids.numel()}, keys hot {sum(p.hot.size() for p in pairs)} / cold {sum(p.cold.size() for p in pairs)}"
          + (f", rebalanced: promoted {sum(m[0] for m in moved)}, demoted {sum(m[1] for m in moved)}" if moved else ""))

# A sequence feature over the same pairs: a row per id (a behaviour history fed to attention), bf16 rows.  Forward is the one-launch find over both
# tiers of every pair, the count and one gated creation launch, backward the same two grouped steps.
history = DynamicEmbeddingCollection(group, optimizer="adagrad", lr=0.05, out_dtype=torch.bfloat16, min_count=min_count).to(dev)
seq_len = 8
scorer = torch.nn.Linear(dim, 1).to(dev).to(torch.bfloat16)
seq_offsets = torch.arange(n_tables + 1, dtype=torch.int64, device=dev) * batch * seq_len      # segment j: the ids of pair j
for step in range(4):
    ids = (torch.rand(n_tables * batch * seq_len, device=dev) ** 3 * vocab).long()
    rows = history(ids, seq_offsets)                                  # [n_tables * batch * seq_len, dim] bf16
    loss = scorer(rows).float().view(n_tables, batch, seq_len).mean(dim=2).square().mean()
    loss.backward()                                                   # the sparse update happens here; the scorer is not trained in this sketch
    print(f"sequence step {step}: loss {loss.item():.5f}, rows {tuple(rows.shape)} {rows.dtype}, keys hot {sum(p.hot.size() for p in pairs)} / cold "
          f"{sum(p.cold.size() for p in pairs)}")

# Histories of different lengths, as a sequence model reads them: one padded [n_bags, max_len, dim] block and the lengths for the mask.  Forward is ONE
# launch over both tiers of every pair (no [n, dim] rows in between; an id that is cut off is neither looked up nor counted nor trained), backward
# two grouped indexed steps on the dense grad of the block.
padded_history = DynamicEmbeddingSequence(group, max_len=6, keep="last", optimizer="adagrad", lr=0.05, create_missing=True).to(dev)
for step in range(4):
    lens = torch.randint(0, 12, (n_tables * batch,), device=dev)          # bag b -> pair b // batch; histories past max_len keep their last 6 ids
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(lens, 0)])
    ids = (torch.rand(int(offsets[-1]), device=dev) ** 3 * vocab).long()
    block, lengths = padded_history(ids, offsets)                           # [n_tables * batch, 6, dim] fp32, [n_tables * batch]
    mask = (torch.arange(6, device=dev)[None, :] < lengths[:, None]).unsqueeze(-1)
    loss = (block * mask).sum(dim=1).square().mean()
    loss.backward()
    print(f"padded step {step}: loss {loss.item():.5f}, block {tuple(block.shape)}, mean kept length {lengths.float().mean().item():.2f}")
