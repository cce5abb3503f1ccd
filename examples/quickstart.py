"""Quick tour of the Python host layer on one MI355X (run on the GPU box: python examples/quickstart.py)."""
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import __graft_entry__

__graft_entry__.build()
from meepoembedding_amd import INIT_UNIFORM, OPT_ADAGRAD, LookupTable, _lib  # noqa: E402
from meepoembedding_amd.nn import DynamicEmbedding, DynamicEmbeddingBag  # noqa: E402
from meepoembedding_amd.tiered import TieredLookupTable  # noqa: E402

dev = torch.device("cuda", 0)

# 1. a table: int64 key -> fp32[64] row, Adagrad state, unseen keys get a hashed uniform(-0.05, 0.05) row
table = LookupTable(1 << 20, 64, device=dev, optimizer=OPT_ADAGRAD, max_batch=1 << 16, initializer=INIT_UNIFORM, init_scale=0.05)
keys = torch.randint(0, 10**12, (50_000,), device=dev)
rows, existed = table.find_or_insert(keys)               # forward lookup of a training step
table.apply_adagrad(keys, torch.randn_like(rows) * 0.01, lr=0.01)   # duplicate keys are reduced, one update per key
print("stored keys:", table.size(), "| new in this batch:", int((existed == 0).sum()))

out, found = table.find(torch.cat([keys[:5], torch.tensor([42], device=dev)]))   # inference lookup: absent -> default row
print("found mask:", found.tolist())
out16, _ = table.find(keys[:5], out_dtype=torch.bfloat16)   # bf16 rows for a bf16 model: rounded once by the lookup, no cast behind it
print("bf16 rows equal the cast fp32 rows:", torch.equal(out16, out[:5].to(torch.bfloat16)))
table.remove(keys[:1000])
ek, ev = table.export()                                    # checkpoint: int64 keys[N], fp32 values[N, 64]
print("after remove:", table.size(), "exported", tuple(ev.shape))

# 1b. train -> serve: the trained fp32 table, saved, loaded into a table that stores its rows as bf16 (half the bytes per key) and served in bf16
with tempfile.TemporaryDirectory() as ckpt:
    table.save(ckpt)
    serving = LookupTable(1 << 20, 64, device=dev, max_batch=1 << 16, value_dtype=torch.bfloat16)
    serving.load(ckpt)                                     # every row rounded once to bf16 on the way in; optimizer state stays behind
    serving8 = LookupTable(1 << 20, 64, device=dev, max_batch=1 << 16, int8_rows=True)   # ... or as int8 codes + one fp32 scale per row
    serving8.load(ckpt)                                    # every row quantized once (scale = max|x| / 127)
rows8, rows32 = serving8.find(keys[1000:1005])[0], table.find(keys[1000:1005])[0]
print("int8-row table:", serving8.table_bytes >> 20, "MiB | largest error in units of the row's step:",
      float(((rows8 - rows32).abs().max(dim=1).values / (rows32.abs().max(dim=1).values / 127)).max()))
served, _ = serving.find(keys[1000:1005], out_dtype=torch.bfloat16)            # the stored bits, no second rounding
print("serving table:", serving.size(), "keys,", serving.table_bytes >> 20, "MiB against", table.table_bytes >> 20, "MiB | same bf16 rows:",
      torch.equal(served, table.find(keys[1000:1005], out_dtype=torch.bfloat16)[0]))

# 2. the same table as a torch layer (forward = find_or_insert, backward = the table's sparse Adagrad)
layer = DynamicEmbedding(table, optimizer="adagrad", lr=0.01)
ids = torch.randint(0, 10**12, (256, 8), device=dev)
loss = layer(ids).sum(1).pow(2).mean()
loss.backward()
print("layer output", tuple(layer(ids).shape), "| table now holds", table.size())

# 3. hot/cold pair: rows of the cold table live in pinned host DRAM, the kernels read them over PCIe
hot = LookupTable(1 << 16, 64, device=dev, max_batch=1 << 16, track_hits=True)
cold = LookupTable(1 << 20, 64, device=dev, max_batch=1 << 16, value_memory=_lib.MEM_HOST_PINNED, track_hits=True)
tiered = TieredLookupTable(hot, cold, hot_key_limit=40_000)
tiered.insert(keys, rows)                                   # 50K new keys > the hot room of 40K: the batch goes to the cold tier
for _ in range(8):
    tiered.find(keys[torch.randint(0, 5000, (20_000,), device=dev)])   # a hot working set of 5000 keys
print("rebalance (promoted, demoted):", tiered.rebalance(), "| hot", hot.size(), "cold", cold.size())
for _ in range(2):
    tiered.find(keys[torch.randint(0, 25_000, (20_000,), device=dev)])  # a new window (rebalance restarted it): half of the keys may be hit
sk, sv, _, _, sh = tiered.evict_cold(10_000, spill=True)    # the cold tier is filling up: its 10K least-hit keys leave, rows handed out for a tier behind it
print("evicted from the cold tier:", sk.numel(), "keys with rows", tuple(sv.shape), "| most hits among them:", int(sh.cpu().numpy().max()), "| cold", cold.size())

# 4. embedding bags over the pair: one launch probes both tiers per position; the backward is the sparse Adagrad step on both tiers
hot_t = LookupTable(1 << 16, 64, device=dev, max_batch=1 << 16, optimizer=OPT_ADAGRAD, initializer=INIT_UNIFORM, init_scale=0.05)
cold_t = LookupTable(1 << 20, 64, device=dev, max_batch=1 << 16, optimizer=OPT_ADAGRAD, initializer=INIT_UNIFORM, init_scale=0.05,
                     value_memory=_lib.MEM_HOST_PINNED)
bags = DynamicEmbeddingBag(TieredLookupTable(hot_t, cold_t, hot_key_limit=8192), mode="mean", lr=0.05, create_missing=True).to(dev).train()
bag_ids = keys[torch.randint(0, 5000, (4096,), device=dev)]                  # ids no tier has seen: created on the way, hot while there is room
offsets = torch.arange(0, 4097, 8, dtype=torch.int64, device=dev)           # 512 bags of 8
pooled = bags(bag_ids, offsets)
pooled.square().mean().backward()
print("bag layer output", tuple(pooled.shape), "| hot", hot_t.size(), "cold", cold_t.size())
