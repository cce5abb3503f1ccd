"""Candidate generation on one MI355X: an item table trains, a bf16-row serving copy of it answers "which items match this user vector best" by
an exact top-k inner-product search of the table in place, and after a publish the same search sees the new and the removed items — no [N, dim]
matrix is ever built (run on the GPU box: python examples/retrieval.py)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import __graft_entry__

__graft_entry__.build()
from meepoembedding_amd import INIT_UNIFORM, OPT_ADAGRAD, LookupTable, TableGroup  # noqa: E402

dev = torch.device("cuda", 0)
dim, items, k = 64, 50_000, 10

trainer = LookupTable(2 * items, dim, device=dev, optimizer=OPT_ADAGRAD, max_batch=1 << 16, initializer=INIT_UNIFORM, init_scale=0.1, init_seed=1)
for step in range(5):                                           # a stand-in for training: items appear and move
    ids = torch.randint(0, items // 2, (1 << 15,), device=dev)
    rows, _ = trainer.find_or_insert(ids)
    trainer.apply_adagrad(ids, 0.1 * torch.randn_like(rows), lr=0.05)

trainer.track_changes(items)                                    # from here on every mutator notes its ids
serving = LookupTable(trainer.capacity, dim, device=dev, max_batch=1 << 16, value_dtype=torch.bfloat16)
serving.import_(*trainer.export())                              # the replica that answers: bf16 rows, equal to the trainer (rounded) NOW

users = torch.randn(32, dim, device=dev)                        # the other tower's output
keys, scores, counts = serving.search(users, k, counts=True)
rows, found = serving.find(keys.view(-1))
check = (users.to(torch.bfloat16).float()[:, None, :] * rows.view(32, k, dim)).sum(-1)
assert found.all() and torch.allclose(check, scores, rtol=1e-4, atol=1e-4) and (scores[:, :-1] >= scores[:, 1:]).all()
print(f"{serving.size()} items served; user 0's best: item {int(keys[0, 0])} at {float(scores[0, 0]):.4f}, {int(counts[0])} candidates returned")

page2, scores2p = serving.search(users, k, exclude=keys)         # "more like this": the best k EXCEPT page one's keys, filtered inside the scan — ranks k .. 2k - 1
twice = serving.search(users, 2 * k)[0]
assert torch.equal(page2, twice[:, k:]) and not (page2[:, :, None] == keys[:, None, :]).any()
print(f"user 0's page two starts at item {int(page2[0, 0])} ({float(scores2p[0, 0]):.4f}); a seen list of up to 4096 ids per user goes the same way")

wide, wide_scores = serving.search(users, 4 * k)               # re-ranking: a wider candidate set, mixed with ids from elsewhere (some unknown here) ...
slate = torch.cat([wide, torch.randint(items, 2 * items, (32, k), device=dev)], dim=1)
rescored, known = serving.score(users, slate)                   # ... scored in one launch: probe, row gather and dot product, no [32, 5k, dim] block
assert known[:, :4 * k].all() and torch.allclose(rescored[:, :4 * k], wide_scores, rtol=1e-4, atol=1e-4)   # search's own keys score search's scores (to the bit on exactly summable data)
assert not known[:, 4 * k:].any() and torch.isneginf(rescored[:, 4 * k:]).all()     # an id the table does not hold: -inf, found 0
top = torch.gather(slate, 1, rescored.argsort(dim=1, descending=True)[:, :k])
print(f"re-ranked a slate of {slate.shape[1]} ids per user ({int((~known.bool()).sum())} unknown ones scored -inf); user 0's best of it: item {int(top[0, 0])}")

promoted = wide[0].contiguous()                                 # ONE slate for the whole batch — today's promoted items: keys of dimension 1, no [32, 4k] key block;
boost, listed = serving.score(users, promoted)                  # a row is gathered once per tile of queries and the [32, 4k] block is a matrix product
assert listed.all() and boost.shape == (32, 4 * k) and torch.allclose(boost[0], wide_scores[0], rtol=1e-4, atol=1e-4)
print(f"scored {promoted.numel()} promoted items against all 32 users in one launch; user 1's best of them: item {int(promoted[boost[1].argmax()])}")

seeds = keys[:4, 0].contiguous()                               # item to item: "items similar to these", asked in cosine — the norms of a trained table's
seed_rows, _ = serving.find(seeds)                              # rows are very unequal, and the table cannot be normalised without a second copy of it
near, cos = serving.search(seed_rows, k, metric="cosine")       # both norms are taken inside the scan, from the row bytes it reads anyway
again, known = serving.score(seed_rows, near, metric="cosine")  # the same four fp32 operations on the same operands
assert (near[:, 0] == seeds).all() and torch.allclose(cos[:, 0], torch.ones(4, device=dev), atol=1e-5) and known.all() and torch.allclose(again, cos, atol=1e-5)
print(f"item {int(seeds[0])}'s nearest other item by cosine: item {int(near[0, 1])} at {float(cos[0, 1]):.4f}")

best = keys[:, 0].unique()                                     # the current winners leave the catalogue, a new item made for user 0 enters
trainer.remove(best)
new_id = torch.tensor([items + 7], device=dev)
trainer.insert(new_id, users[:1] * 4)
upserts, removed, dropped = trainer.publish_to(serving, clear=True)
keys2, scores2 = serving.search(users, k)
assert int(keys2[0, 0]) == items + 7 and not torch.isin(keys2, best).any()
print(f"published {upserts} changed rows and {removed} removals; user 0's best is now item {int(keys2[0, 0])} at {float(scores2[0, 0]):.4f}; "
      f"none of the {best.numel()} removed items is returned any more")

creators = LookupTable(4096, dim, device=dev, max_batch=1 << 12, value_dtype=torch.bfloat16)   # a second, small corpus: items plus creators, searched with the
creators.insert(torch.arange(1000, device=dev), torch.randn(1000, dim, device=dev))            # same user vectors in ONE call of three launches (TableGroup.search)
both = TableGroup([serving, creators])
gkeys, gscores = both.search(torch.stack([users, users]), k)    # queries [n_tables, Q, dim] -> [n_tables, Q, k]: block j is member j's own search, bit for bit
assert torch.equal(gkeys[0], keys2) and torch.equal(gscores[0], scores2) and torch.equal(gkeys[1], creators.search(users, k)[0])
print(f"both corpora in one call: user 0's best item {int(gkeys[0, 0, 0])}, best creator {int(gkeys[1, 0, 0])}")
