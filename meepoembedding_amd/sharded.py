"""Row-sharded lookup table over one node's GPUs: owner(key) routing + all-to-all exchange (SPEC.md §5).

One process per GPU; `torch.distributed` carries the exchange (backend "nccl" is RCCL over xGMI on ROCm; "gloo"
is used by the CPU tests of this host logic).  Per sharded find:

    partition(keys) by owner  ->  all-to-all counts  ->  all-to-all keys (8 B each)
    local find on the received keys (HIP kernel)     ->  all-to-all rows (dim*4 B each) + found-mask back
    scatter through perm into batch order

out_dtype=torch.bfloat16 on find / find_or_insert: the owner's lookup writes bf16 rows (rounded once, SPEC.md §3 "Output type") and those travel:
dim*2 B per row on the way back.

Embedding bags (find_pooled, apply_*(grad_index=...); SPEC.md §5 "Pooled lookups"): the partition is stable, so the positions of one bag that one
owner holds are a contiguous run of that owner's segment.  The owner pools each run and ONE fp32 row per run travels (back in the lookup, out in
the backward) instead of one per key:

    partition(keys)  ->  bag_runs  ->  all-to-all key counts + run counts  ->  all-to-all keys (8 B) and run lengths (4 B)
    owner: run_offsets, local find_pooled(sum) over the runs  ->  all-to-all partial rows (dim*4 B per RUN) + found-mask back
    combine_bag_runs: the partial rows of a bag added up in rank order (mean / bf16 rounding here, at the source)

Reference anchor: /root/reference/README.md:2 ("A distributed … Embedding"); the snapshot has no code.

Table groups (ShardedTableGroup; SPEC.md §5 "Groups"): one partition and ONE exchange per operator serve the jagged batch of a whole collection of
sharded tables — 4 collectives per find, 3 per apply, whatever the number of tables (segment_counts on the source, regroup on the owner).
ShardedTieredTableGroup (SPEC.md §5 "Groups of pairs") is the same over a collection of hot/cold pairs (a TieredTableGroup per rank).

This module is host logic only: `local` is any object with the LookupTable operator methods and `router` any
object with partition / gather_rows / scatter_rows (the HIP-backed LookupTable / Router in production).
"""
from __future__ import annotations

import math

import torch
import torch.distributed as dist

from ._lib import refuse_narrow_rows
from .table import SparseStep, _buffer, _out_dtype


class _Exchange:
    """What ShardedLookupTable and ShardedTableGroup share: the process group, the all-to-alls and their counters."""

    def __init__(self, router, group=None):
        self.router, self.group = router, group
        self.world = dist.get_world_size(group)
        self.rank = dist.get_rank(group)
        # a gloo group cannot move device tensors: stage them through host memory (rehearsals of the multi-rank GPU
        # path on a single-GPU box; production uses the "nccl" backend = RCCL over xGMI, no staging)
        self._stage = dist.get_backend(group) == "gloo"
        self._sent = self._received = 0   # traffic()
        self.collectives = 0              # every all_to_all_single this object issued
        if router.n_shards != self.world:
            raise ValueError(f"router has {router.n_shards} shards, process group has {self.world} ranks")

    # -- exchange plumbing -------------------------------------------------------------------------------
    def _swap_counts(self, counts: torch.Tensor):
        """all-to-all of per-destination counts ([G] or [G, m] int64: m values for every rank) -> (sent, received) on the host"""
        self._sent += counts.numel() // self.world * (self.world - 1) * 8
        self._received += counts.numel() // self.world * (self.world - 1) * 8
        self.collectives += 1
        if self._stage and counts.is_cuda:
            c_host = counts.cpu()
            r_host = torch.empty_like(c_host)
            dist.all_to_all_single(r_host, c_host, group=self.group)
            return c_host, r_host
        recv_counts = torch.empty_like(counts)
        dist.all_to_all_single(recv_counts, counts, group=self.group)
        both = torch.stack([counts, recv_counts]).cpu()  # the one host sync of the exchange
        return both[0], both[1]

    def traffic(self) -> tuple[int, int]:
        """(sent, received): bytes handed to the process group for OTHER ranks since this table was made — every _a2a and every count exchange;
        the rank's own segment never leaves the device and is not counted, and staging through host memory (gloo) counts the same bytes.
        Mirrors RcclShardedTable.traffic()."""
        return self._sent, self._received

    def _a2a(self, t: torch.Tensor, in_splits, out_splits) -> torch.Tensor:
        if t.dtype == torch.bfloat16:   # bf16 rows travel as their bytes, so that no backend's dtype support matters (gloo moves neither bf16 nor int16)
            return self._a2a(t.contiguous().view(torch.uint8), in_splits, out_splits).view(torch.bfloat16)
        row_bytes = t.element_size() * math.prod(t.shape[1:])
        self._sent += (sum(in_splits) - in_splits[self.rank]) * row_bytes
        self._received += (sum(out_splits) - out_splits[self.rank]) * row_bytes
        self.collectives += 1
        if self._stage and t.is_cuda:
            src = t.contiguous().cpu()
            dst = torch.empty((sum(out_splits),) + tuple(t.shape[1:]), dtype=t.dtype)
            dist.all_to_all_single(dst, src, output_split_sizes=out_splits, input_split_sizes=in_splits, group=self.group)
            return dst.to(t.device)
        out = torch.empty((sum(out_splits),) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
        dist.all_to_all_single(out, t.contiguous(), output_split_sizes=out_splits, input_split_sizes=in_splits, group=self.group)
        return out

    def admission_refusal(self) -> str:
        return "admission exists on one device — a LookupTable, a TableGroup, a hot/cold pair or a TieredTableGroup — not on sharded or peer-mapped tables"

    def _typed(self, out_dtype: torch.dtype) -> dict:
        """the local lookup's out_dtype keyword (none at fp32: a `local` without the keyword keeps working); refused before anything is exchanged"""
        if _out_dtype(out_dtype) == 0:
            return {}
        if not getattr(self.local, "supports_out_dtype", False):
            raise ValueError(f"{type(self.local).__name__} has no bf16 lookup: use out_dtype=torch.float32 and cast the result")
        return {"out_dtype": out_dtype}


class ShardedLookupTable(_Exchange):
    def __init__(self, local, router, group=None):
        refuse_narrow_rows("ShardedLookupTable", local)
        self.local = local
        self.dim = local.dim
        super().__init__(router, group)

    def _route(self, keys: torch.Tensor):
        """partition + counts exchange. Returns (send_keys, perm, send_splits, recv_splits)."""
        send_keys, counts, perm = self.router.partition(keys)
        sent, received = self._swap_counts(counts)
        return send_keys, perm, sent.tolist(), received.tolist()

    # -- operators ---------------------------------------------------------------------------------------
    def _lookup(self, keys: torch.Tensor, insert_missing: bool, dedup: bool = False, out_dtype: torch.dtype = torch.float32):
        typed = self._typed(out_dtype)
        keys = keys.contiguous().view(-1)
        if dedup:
            return self._lookup_dedup(keys, insert_missing, out_dtype, typed)
        send_keys, perm, ss, rs = self._route(keys)
        recv_keys = self._a2a(send_keys, ss, rs)
        if insert_missing:
            rows, found = self.local.find_or_insert(recv_keys, **typed)
        else:
            rows, found = self.local.find(recv_keys, **typed)
        rows_back = self._a2a(rows, rs, ss)
        found_back = self._a2a(found, rs, ss)
        return self.router.scatter_rows(rows_back, perm), self.router.scatter_rows(found_back, perm)

    def _lookup_dedup(self, keys: torch.Tensor, insert_missing: bool, out_dtype: torch.dtype = torch.float32, typed: dict | None = None):
        """Pre-exchange duplicate elimination: only the batch's DISTINCT keys cross xGMI (keys out, rows back); every
        occurrence is then served from its distinct key's row.  On skewed streams the link traffic scales with the
        number of unique keys while the metric counts lookups (SURVEY §7 hard part 1)."""
        uniq, _, _, inverse = self.local.dedup_sum(keys, compact=True)   # (this path synchronises for its split sizes anyway)
        rows_u, found_u = self._lookup(uniq, insert_missing, out_dtype=out_dtype)
        # reserved keys have inverse -1: point them at an extra all-default "missing" row
        miss_row, _ = self.local.find(keys.new_full((1,), -(1 << 63)), **(typed or {}))
        rows_u = torch.cat([rows_u, miss_row])
        found_u = torch.cat([found_u, found_u.new_zeros(1)])
        inverse = torch.where(inverse < 0, torch.full_like(inverse, uniq.numel()), inverse)
        return self.router.gather_rows(rows_u, inverse, n_out=keys.numel()), self.router.gather_rows(found_u, inverse, n_out=keys.numel())

    def find(self, keys: torch.Tensor, dedup: bool = False, out_dtype: torch.dtype = torch.float32):
        """out_dtype=torch.bfloat16: the fp32 result rounded once to bf16 — by each key's owner, so bf16 rows cross the link (`local` must have a
        bf16 lookup: a LookupTable; a tiered table has none and is refused with ValueError)."""
        return self._lookup(keys, False, dedup, out_dtype)

    def find_or_insert(self, keys: torch.Tensor, dedup: bool = False, out_dtype: torch.dtype = torch.float32):
        return self._lookup(keys, True, dedup, out_dtype)

    def remove(self, keys: torch.Tensor) -> torch.Tensor:
        keys = keys.contiguous().view(-1)
        send_keys, perm, ss, rs = self._route(keys)
        rk = self._a2a(send_keys, ss, rs)
        found = torch.cat([self.local.remove(rk[s:e]) for s, e in self._chunks(rk.numel())])
        return self.router.scatter_rows(self._a2a(found, rs, ss), perm)

    def _push(self, keys: torch.Tensor, payload: torch.Tensor):
        """Route (key, row) pairs to their owners; received pairs are ordered by source rank, then batch position."""
        keys = keys.contiguous().view(-1)
        send_keys, perm, ss, rs = self._route(keys)
        send_rows = self.router.gather_rows(payload.contiguous().view(keys.numel(), -1), perm)
        return self._a2a(send_keys, ss, rs), self._a2a(send_rows, ss, rs), perm, ss, rs

    # An owner may receive more pairs than its table's max_batch (skew, or simply world x batch).  insert / assign /
    # remove are sequentially consistent, so the received pairs are applied max_batch at a time (order preserved =
    # last-wins preserved).  apply_* is ONE update per distinct key and cannot be chunked: size the local table's
    # max_batch for the largest received batch (<= world x per-rank batch).
    def _chunks(self, n: int):
        step = int(getattr(self.local, "max_batch", n) or n) or 1
        return [(s, min(n, s + step)) for s in range(0, n, step)] or [(0, 0)]

    def insert(self, keys: torch.Tensor, values: torch.Tensor) -> None:
        rk, rv, *_ = self._push(keys, values)
        for s, e in self._chunks(rk.numel()):
            self.local.insert(rk[s:e], rv[s:e])

    def assign(self, keys: torch.Tensor, values: torch.Tensor) -> torch.Tensor:
        rk, rv, perm, ss, rs = self._push(keys, values)
        found = torch.cat([self.local.assign(rk[s:e], rv[s:e]) for s, e in self._chunks(rk.numel())])
        return self.router.scatter_rows(self._a2a(found, rs, ss), perm)

    def _aggregate(self, keys: torch.Tensor, grads: torch.Tensor):
        """Pre-exchange gradient aggregation: one (key, summed row) pair per distinct key of this rank's batch (fp64 sums rounded once, mee_dedup_sum) —
        on skewed streams the backward's bytes on xGMI scale with the distinct keys.  The owner's apply adds the ranks' partial sums up in fp64 again:
        within 1e-6 of the un-aggregated update (one extra rounding per rank and key).  Adagrad only (see apply_adam)."""
        keys = keys.contiguous().view(-1)
        uniq, gsum, _, _ = self.local.dedup_sum(keys, grads.contiguous().view(keys.numel(), -1), compact=True)   # (this path synchronises for its split sizes anyway)
        return uniq, gsum

    # -- embedding bags (SPEC.md §5 "Pooled lookups") ------------------------------------------------------
    def _bag_route(self, keys: torch.Tensor, bag_offsets: torch.Tensor):
        """partition + the runs of the batch + ONE exchange of key counts and run counts.
        Returns (send_keys, perm, key splits out / in, run_bag [R], run_len [R], run_counts, run splits out / in)."""
        send_keys, counts, perm = self.router.partition(keys)
        run_bag, run_len, run_counts = self.router.bag_runs(perm, counts, bag_offsets)
        sent, received = self._swap_counts(torch.stack([counts, run_counts], dim=1))
        ss, rss = sent[:, 0].tolist(), sent[:, 1].tolist()
        rs, rrs = received[:, 0].tolist(), received[:, 1].tolist()
        r = sum(rss)
        return send_keys, perm, ss, rs, run_bag[:r], run_len[:r], run_counts, rss, rrs

    def _check_bags(self, keys: torch.Tensor, bag_offsets: torch.Tensor) -> None:
        if not hasattr(self.router, "bag_runs"):
            raise ValueError(f"{type(self.router).__name__} has no bag_runs / run_offsets / combine_bag_runs: pooled lookups need the HIP Router")
        if bag_offsets.numel() < 1 or (keys.numel() and bag_offsets.numel() < 2):
            raise ValueError("bag_offsets must hold n_bags + 1 entries, and at least one bag when there are keys (the bags partition the batch)")

    def find_pooled(self, keys: torch.Tensor, bag_offsets: torch.Tensor, mode: str = "sum", insert_missing: bool = False,
                    out_dtype: torch.dtype = torch.float32):
        """Embedding-bag lookup over the sharded table -> ([n_bags, dim] sums or means, per-key found mask as find reports it).  Bags are defined
        on this rank's batch as in LookupTable.find_pooled and must partition it.  Every owner pools its part of every bag in batch order (one
        row per run travels back), the parts are added up here in rank order, then mean divides and bf16 rounds — once, at the source.  One rank:
        bit-identical to LookupTable.find_pooled; more: a different, fixed summation order of the same terms.
        insert_missing: the owners find_or_insert the received keys first (found = existed before).  Collective, also for a rank without keys
        or without bags."""
        if mode not in ("sum", "mean"):
            raise ValueError(f"mode must be 'sum' or 'mean' (got {mode!r})")
        _out_dtype(out_dtype)
        if not hasattr(self.local, "find_pooled"):   # refused on every rank alike, before anything is exchanged
            raise ValueError(f"{type(self.local).__name__} has no find_pooled: pooled lookups need a LookupTable shard")
        keys = keys.contiguous().view(-1)
        self._check_bags(keys, bag_offsets)
        send_keys, perm, ss, rs, run_bag, run_len, run_counts, rss, rrs = self._bag_route(keys, bag_offsets)
        recv_keys = self._a2a(send_keys, ss, rs)
        recv_len = self._a2a(run_len, rss, rrs)
        offsets, _ = self.router.run_offsets(recv_len)
        if insert_missing:
            _, found = self.local.find_or_insert(recv_keys)
            partial, _ = self.local.find_pooled(recv_keys, offsets, "sum")
        else:
            partial, found = self.local.find_pooled(recv_keys, offsets, "sum")
        partial_back = self._a2a(partial, rrs, rss)       # fp32: rounding at the owner would round twice
        found_back = self._a2a(found, rs, ss)
        out = self.router.combine_bag_runs(partial_back, run_bag, run_counts, bag_offsets, mode, out_dtype=out_dtype)
        return out, self.router.scatter_rows(found_back, perm)

    def _apply_bags(self, keys: torch.Tensor, grads: torch.Tensor, grad_index: torch.Tensor, dedup: bool):
        """The pooled backward: one gradient row per run travels to the owner.  -> (received keys, received run rows, run of every received key)"""
        if dedup:
            raise ValueError("dedup=True aggregates one row per key and cannot be combined with grad_index (one row per bag)")
        keys = keys.contiguous().view(-1)
        g = grads.contiguous().view(-1, self.dim)
        gi = grad_index.contiguous().view(-1)
        if gi.numel() != keys.numel():
            raise ValueError("grad_index must hold one entry per key")
        # the calling convention of the pooled backward: grad_index is the bag of every position (checked before anything is exchanged)
        if gi.numel() and bool((gi[1:] < gi[:-1]).any() | (gi[0] < 0) | (gi[-1] >= g.shape[0])):
            raise ValueError("sharded apply_*(grad_index=...) takes the pooled backward: grad_index non-decreasing over the batch, inside [0, rows of grads)")
        bag_offsets = torch.searchsorted(gi.to(torch.int64), torch.arange(g.shape[0] + 1, device=gi.device))
        self._check_bags(keys, bag_offsets)
        send_keys, perm, ss, rs, run_bag, run_len, run_counts, rss, rrs = self._bag_route(keys, bag_offsets)
        run_rows = self.router.gather_rows(g, run_bag.to(torch.int64))
        rk = self._a2a(send_keys, ss, rs)
        recv_len = self._a2a(run_len, rss, rrs)
        recv_rows = self._a2a(run_rows, rss, rrs)
        _, run_of_key = self.router.run_offsets(recv_len, rk.numel())
        return rk, recv_rows, run_of_key

    def apply_adagrad(self, keys: torch.Tensor, grads: torch.Tensor, lr: float, eps: float = 1e-10, dedup: bool = False,
                      grad_index: torch.Tensor | None = None) -> None:
        """grad_index (the pooled backward): position i takes row grad_index[i] of grads, the bag's gradient row — non-decreasing over the batch.
        One row per (bag, owner) run travels; the owner reduces duplicates over all ranks' contributions in one indexed apply."""
        self._apply(SparseStep("adagrad", lr, eps), keys, grads, dedup, grad_index, aggregate=dedup)

    def apply_adam(self, keys: torch.Tensor, grads: torch.Tensor, lr: float, beta1: float = 0.9, beta2: float = 0.999,
                   eps: float = 1e-8, step: int = 1, dedup: bool = False, grad_index: torch.Tensor | None = None) -> None:
        """dedup is accepted like apply_adagrad's, but Adam's pairs are never aggregated before the exchange: its update barely depends on the size of
        g, so the rounding of a rank's partial sum, where the ranks' sums cancel, would reach the row as a large relative error (SPEC.md §5).
        grad_index: as apply_adagrad's."""
        self._apply(SparseStep("adam", lr, eps, beta1, beta2, step), keys, grads, dedup, grad_index, aggregate=False)

    def _apply(self, step: SparseStep, keys, grads, dedup: bool, grad_index, aggregate: bool) -> None:
        if grad_index is not None:
            rk, rg, run_of_key = self._apply_bags(keys, grads, grad_index, dedup)
            step.apply_to(self.local, rk, rg, grad_index=run_of_key)
            return
        if aggregate:
            keys, grads = self._aggregate(keys, grads)
        rk, rg, *_ = self._push(keys, grads)
        step.apply_to(self.local, rk, rg)

    def size(self) -> int:
        t = torch.tensor([self.local.size()], dtype=torch.int64, device="cpu" if self._stage else self._dev())
        dist.all_reduce(t, group=self.group)
        return int(t.item())

    def save(self, path: str, chunk_slots: int = 1 << 22) -> int:
        """Checkpoint: every rank writes its shard under path/shard-<rank>-of-<world> (checkpoint.py); collective."""
        from . import checkpoint
        n = checkpoint.save_sharded(self, path, chunk_slots)
        dist.barrier(group=self.group)
        return n

    def load(self, path: str, chunk_pairs: int | None = None) -> int:
        """Load a checkpoint written by ANY world size: each rank keeps the pairs it owns now (re-sharding on load)."""
        from . import checkpoint
        n = checkpoint.load_sharded(self, path, self.router.owner, chunk_pairs)
        dist.barrier(group=self.group)
        return n

    def export_local(self, with_state: bool = False):
        return self.local.export(with_state=with_state)

    def _dev(self):
        return getattr(self.local, "device", torch.device("cpu"))

    @property
    def device(self):
        return self._dev()

    pools_with_insert = True   # find_pooled(insert_missing=True): what DynamicEmbeddingBag(create_missing=True) calls instead of a find_or_insert of its own



class ShardedTableGroup(_Exchange):
    """A whole collection of row-sharded tables behind ONE exchange per operator (SPEC.md §5 "Groups"): every rank holds one TableGroup of its T local
    shards (`local_group`), a call takes the rank's jagged batch (keys, offsets[T + 1] on the device, as TableGroup's operators) and is, by
    definition, the sharded single-table operator applied to every member with its segment.  owner(key) does not depend on the table and the
    partition is stable, so the batch is partitioned once and the members' keys stay in member order inside every owner's segment:

        partition(keys)  ->  segment_counts: the [G, T] cells  ->  ONE all-to-all of the cells (the key splits are their row sums)  ->  all-to-all keys
        owner: regroup (source-major -> table-major keys, order, member offsets), ONE local_group operator over the regrouped batch
        find: scatter_rows(rows, order), all-to-all rows + found-mask back, scatter through perm
        apply: the gradient rows gathered through perm, sent, gathered through order

    4 collectives per find and 3 per apply whatever T is, where T ShardedLookupTable calls make 4 T and 3 T (and T host syncs); the bytes are the same
    plus 8 T (G - 1) count bytes each way instead of 8 T (G - 1) in T pieces.  Collective: every rank calls, also with an empty batch.
    `router`: the HIP Router (segment_counts / regroup); dedup= and grad_index= are not offered.

    Embedding bags (find_pooled / apply_pooled; SPEC.md §5 "Pooled lookups over a group"): the collection's bags, B per member, bag b belonging to
    member b // B — ShardedLookupTable.find_pooled of every member with its B bags.  The owners pool, one fp32 row per (bag, owner) run travels:

        partition(keys)  ->  bag_runs  ->  segment_counts twice: the key cells and the run cells  ->  ONE all-to-all of the [G, 2 T] cells
        all-to-all keys (8 B) and run lengths (4 B);  owner: regroup the keys AND the runs, run_offsets, ONE find_pooled_jagged over the runs
        lookup: all-to-all partial rows (4 dim B per RUN) + found-mask back, combine_bag_runs (rank order; mean / bf16 here, at the source)
        step: the runs' gradient rows travel with the keys, ONE apply_indexed on the owner; nothing comes back

    5 collectives per pooled lookup and 4 per pooled step, whatever T is; weighted bags and dedup= are not offered."""

    _over_pairs = False   # ShardedTieredTableGroup: the local group is a TieredTableGroup

    def __init__(self, local_group, router, group=None):
        if not hasattr(local_group, "tables"):
            raise ValueError(f"{type(local_group).__name__} is no group of tables (a TableGroup of the rank's local shards)")
        if getattr(local_group, "mixed_dims", False):
            raise ValueError(f"{type(local_group).__name__} has members of different dims: a sharded group exchanges rows of one width "
                             "(one ShardedTableGroup per width, each over a TableGroup)")
        if hasattr(local_group, "cold_group") and not self._over_pairs:   # a TieredTableGroup
            raise ValueError(f"{type(local_group).__name__} is a group of hot/cold pairs: the sharded group over tiers is a class of its own, "
                             "ShardedTieredTableGroup (a ShardedLookupTable over a TieredLookupTable shards one pair)")
        refuse_narrow_rows("ShardedTableGroup", local_group)
        self.local = self.local_group = local_group
        self.dim = local_group.dim
        self.n_tables = len(local_group.tables)
        super().__init__(router, group)

    @property
    def tables(self):
        return self.local_group.tables

    @property
    def supports_out_dtype(self) -> bool:
        return bool(getattr(self.local_group, "supports_out_dtype", False))

    @property
    def device(self):
        return getattr(self.local_group, "device", torch.device("cpu"))

    def _check(self, op: str, keys: torch.Tensor, offsets: torch.Tensor) -> torch.Tensor:
        """what every rank can decide alone, before anything is exchanged"""
        if not callable(getattr(self.local_group, op, None)):
            raise ValueError(f"{type(self.local_group).__name__} has no {op}")
        if not hasattr(self.router, "segment_counts") or not hasattr(self.router, "regroup"):
            raise ValueError(f"{type(self.router).__name__} has no segment_counts / regroup: sharded groups need the HIP Router")
        if offsets.dim() != 1 or offsets.numel() != self.n_tables + 1:
            raise ValueError(f"offsets must hold n_tables + 1 = {self.n_tables + 1} entries (got {tuple(offsets.shape)})")
        return keys.contiguous().view(-1)

    def _route(self, keys: torch.Tensor, offsets: torch.Tensor):
        """partition + cells + ONE count exchange -> (send_keys, perm, key splits out / in, the received cells [G, T] on the keys' device)"""
        send_keys, counts, perm = self.router.partition(keys)
        cells = self.router.segment_counts(perm, counts, offsets)
        sent, received = self._swap_counts(cells)
        ss, rs = sent.sum(dim=1).tolist(), received.sum(dim=1).tolist()
        if sum(ss) != keys.numel():   # positions in no segment (offsets[0] > 0 or offsets[T] < n) are not sent; inside an owner segment the others stay contiguous
            off = offsets.view(torch.int64)
            inside = (perm >= off[0]) & (perm < off[-1])
            send_keys, perm = send_keys[inside], perm[inside]
        return send_keys, perm, ss, rs, received.to(keys.device)

    def _lookup(self, op: str, keys: torch.Tensor, offsets: torch.Tensor, out_dtype: torch.dtype):
        typed = self._typed(out_dtype)
        keys = self._check(op, keys, offsets)
        n = keys.numel()
        send_keys, perm, ss, rs, recv_cells = self._route(keys, offsets)
        recv_keys = self._a2a(send_keys, ss, rs)
        keys_tm, order, offsets_tm = self.router.regroup(recv_keys, recv_cells)
        rows, found = getattr(self.local_group, op)(keys_tm, offsets_tm, **typed)
        rows_back = self._a2a(self.router.scatter_rows(rows, order), rs, ss)
        found_back = self._a2a(self.router.scatter_rows(found, order), rs, ss)
        if perm.numel() == n:
            return self.router.scatter_rows(rows_back, perm), self.router.scatter_rows(found_back, perm)
        out = rows_back.new_zeros((n, self.dim))   # positions in no segment: zeros, not found
        fnd = found_back.new_zeros(n)
        return self.router.scatter_rows(rows_back, perm, out=out), self.router.scatter_rows(found_back, perm, out=fnd)

    def find(self, keys: torch.Tensor, offsets: torch.Tensor, out_dtype: torch.dtype = torch.float32):
        """-> (rows [n, dim], found [n]) in batch order: ShardedLookupTable.find of every member with its segment.  out_dtype=torch.bfloat16: the
        owners round before the rows travel."""
        return self._lookup("find", keys, offsets, out_dtype)

    def find_or_insert(self, keys: torch.Tensor, offsets: torch.Tensor, out_dtype: torch.dtype = torch.float32):
        return self._lookup("find_or_insert", keys, offsets, out_dtype)

    def _push(self, op: str, keys: torch.Tensor, offsets: torch.Tensor, grads: torch.Tensor):
        """-> (keys, member offsets, gradient rows) of everything this rank owns, table-major; duplicates are reduced by the local apply, per member,
        over all ranks' contributions"""
        keys = self._check(op, keys, offsets)
        g = grads.contiguous().view(-1, self.dim)
        if g.shape[0] != keys.numel():
            raise ValueError(f"grads must hold one row of {self.dim} per key")
        send_keys, perm, ss, rs, recv_cells = self._route(keys, offsets)
        send_rows = self.router.gather_rows(g, perm)
        recv_keys = self._a2a(send_keys, ss, rs)
        recv_rows = self._a2a(send_rows, ss, rs)
        keys_tm, order, offsets_tm = self.router.regroup(recv_keys, recv_cells)
        return keys_tm, offsets_tm, self.router.gather_rows(recv_rows, order)

    # -- embedding bags over the collection (SPEC.md §5 "Pooled lookups over a group") ----------------------------------------------
    pools_with_insert = True   # find_pooled(insert_missing=True): what DynamicEmbeddingBag(create_missing=True) calls instead of a find_or_insert of its own
    weighted_bags = False      # no per_sample_weights over a sharded group: DynamicEmbeddingBag refuses them before anything is exchanged

    def _check_bags(self, ops, keys: torch.Tensor, bag_offsets: torch.Tensor):
        """what every rank can decide alone, before anything is exchanged -> (keys [n], bags per member)"""
        for op in ops:
            if not callable(getattr(self.local_group, op, None)):
                raise ValueError(f"{type(self.local_group).__name__} has no {op}: pooled forms over a sharded group need a TableGroup of the local shards")
        for m in ("bag_runs", "run_offsets", "combine_bag_runs", "segment_counts", "regroup"):
            if not hasattr(self.router, m):
                raise ValueError(f"{type(self.router).__name__} has no {m}: pooled forms over a sharded group need the HIP Router")
        n_bags = bag_offsets.numel() - 1
        if bag_offsets.dim() != 1 or n_bags < 0 or n_bags % self.n_tables:
            raise ValueError(f"bag_offsets must hold n_tables x bags_per_table + 1 entries, n_tables = {self.n_tables} (got {tuple(bag_offsets.shape)})")
        if keys.numel() and n_bags == 0:
            raise ValueError("there are keys but no bags (the bags partition the batch)")
        return keys.contiguous().view(-1), n_bags // self.n_tables

    def _bag_route(self, keys: torch.Tensor, bag_offsets: torch.Tensor, bpt: int):
        """partition + the runs + the key cells and the run cells + ONE count exchange of [G, 2 T].
        -> (send_keys, perm, key splits out / in, run_bag [R], run_len [R], run_counts, run splits out / in, received key cells, received run cells)"""
        T = self.n_tables
        send_keys, counts, perm = self.router.partition(keys)
        run_bag, run_len, run_counts = self.router.bag_runs(perm, counts, bag_offsets)
        member_off = bag_offsets[::bpt].contiguous() if bpt else bag_offsets.new_zeros(T + 1)
        key_cells = self.router.segment_counts(perm, counts, member_off)
        # the runs of an owner segment ascend by bag as its positions do: the same operator counts the runs per member (it only compares the entries)
        member_bags = torch.arange(T + 1, dtype=torch.int64, device=keys.device) * bpt
        run_cells = self.router.segment_counts(run_bag.to(torch.int64), run_counts, member_bags)
        sent, received = self._swap_counts(torch.cat([key_cells, run_cells], dim=1))
        ss, rss = sent[:, :T].sum(dim=1).tolist(), sent[:, T:].sum(dim=1).tolist()
        rs, rrs = received[:, :T].sum(dim=1).tolist(), received[:, T:].sum(dim=1).tolist()
        r = sum(rss)
        received = received.to(keys.device)
        return send_keys, perm, ss, rs, run_bag[:r], run_len[:r], run_counts, rss, rrs, received[:, :T].contiguous(), received[:, T:].contiguous()

    def _regroup_runs(self, recv_keys: torch.Tensor, recv_len: torch.Tensor, key_cells: torch.Tensor, run_cells: torch.Tensor):
        """the owner's side: keys and runs source-major -> table-major.  A run's keys are contiguous in keys_tm, in the runs' table-major order.
        -> (keys_tm, order, offsets_tm, order_r, member_bags, run_len_tm)"""
        keys_tm, order, offsets_tm = self.router.regroup(recv_keys, key_cells)
        # only the order and the offsets of the runs' regrouping are used: any int64 array of R entries serves as its keys (R <= received keys)
        _, order_r, member_bags = self.router.regroup(recv_keys[:recv_len.numel()], run_cells)
        return keys_tm, order, offsets_tm, order_r, member_bags, self.router.gather_rows(recv_len, order_r)

    def find_pooled(self, keys: torch.Tensor, bag_offsets: torch.Tensor, mode: str = "sum", insert_missing: bool = False,
                    out_dtype: torch.dtype = torch.float32):
        """Embedding-bag lookup over the sharded collection -> ([T B, dim] sums or means, per-key found mask [n]): bag_offsets holds T B + 1 offsets
        that partition this rank's batch, bag b belongs to member b // B (B may differ from rank to rank).  ShardedLookupTable.find_pooled of every
        member with its B bags: the same partial rows, added up in rank order; one rank: bit-identical to TableGroup.find_pooled.
        insert_missing: the owners find_or_insert the received keys first (found = existed before).  Collective, also without keys or bags."""
        if mode not in ("sum", "mean"):
            raise ValueError(f"mode must be 'sum' or 'mean' (got {mode!r})")
        _out_dtype(out_dtype)
        keys, bpt = self._check_bags(("find_pooled_jagged",) + (("find_or_insert",) if insert_missing else ()), keys, bag_offsets)
        send_keys, perm, ss, rs, run_bag, run_len, run_counts, rss, rrs, key_cells, run_cells = self._bag_route(keys, bag_offsets, bpt)
        recv_keys = self._a2a(send_keys, ss, rs)
        recv_len = self._a2a(run_len, rss, rrs)
        keys_tm, order, offsets_tm, order_r, member_bags, run_len_tm = self._regroup_runs(recv_keys, recv_len, key_cells, run_cells)
        run_off, _ = self.router.run_offsets(run_len_tm)
        if insert_missing:
            _, found = self.local_group.find_or_insert(keys_tm, offsets_tm)
            partial, _ = self.local_group.find_pooled_jagged(keys_tm, run_off, member_bags, "sum")
        else:
            partial, found = self.local_group.find_pooled_jagged(keys_tm, run_off, member_bags, "sum")
        partial_back = self._a2a(self.router.scatter_rows(partial, order_r), rrs, rss)      # fp32: rounding at the owner would round twice
        found_back = self._a2a(self.router.scatter_rows(found, order), rs, ss)
        out = self.router.combine_bag_runs(partial_back, run_bag, run_counts, bag_offsets, mode, out_dtype=out_dtype)
        return out, self.router.scatter_rows(found_back, perm)

    def apply_pooled(self, keys: torch.Tensor, bag_offsets: torch.Tensor, bag_grads: torch.Tensor, bag_of_position: torch.Tensor,
                     optimizer: str, lr: float, eps: float | None = None, beta1: float = 0.9, beta2: float = 0.999, step: int = 1,
                     located: torch.Tensor | None = None) -> None:
        """Backward of find_pooled, with the signature of TableGroup.apply_pooled: one optimizer step, every key of bag b takes row b of bag_grads
        [T B, dim] (pre-scaled by 1 / length for a mean).  One gradient row per run travels with the keys; the owner reduces duplicates per member
        over all ranks' contributions in one indexed apply.  bag_of_position [n] is the bag of every position as bag_offsets defines it;
        `located` is accepted and ignored (handles do not cross the two exchanges)."""
        step = SparseStep.of(optimizer, lr, eps, beta1, beta2, step, error=ValueError)
        keys, bpt = self._check_bags(("apply_indexed",), keys, bag_offsets)
        if bag_of_position.numel() != keys.numel():
            raise ValueError("bag_of_position must hold one entry per key")
        g = bag_grads.contiguous().view(-1, self.dim)
        if g.shape[0] != bpt * self.n_tables:
            raise ValueError(f"bag_grads must hold one row of {self.dim} per bag")
        send_keys, perm, ss, rs, run_bag, run_len, run_counts, rss, rrs, key_cells, run_cells = self._bag_route(keys, bag_offsets, bpt)
        run_rows = self.router.gather_rows(g, run_bag.to(torch.int64))
        recv_keys = self._a2a(send_keys, ss, rs)
        recv_len = self._a2a(run_len, rss, rrs)
        recv_rows = self._a2a(run_rows, rss, rrs)
        keys_tm, _, offsets_tm, order_r, _, run_len_tm = self._regroup_runs(recv_keys, recv_len, key_cells, run_cells)
        _, run_of_key = self.router.run_offsets(run_len_tm, keys_tm.numel())
        self.local_group.apply_indexed(keys_tm, offsets_tm, self.router.gather_rows(recv_rows, order_r), run_of_key, *step)

    def apply_adagrad(self, keys: torch.Tensor, offsets: torch.Tensor, grads: torch.Tensor, lr: float, eps: float = 1e-10) -> None:
        SparseStep("adagrad", lr, eps).apply_to(self.local_group, *self._push("apply_adagrad", keys, offsets, grads))

    def apply_adam(self, keys: torch.Tensor, offsets: torch.Tensor, grads: torch.Tensor, lr: float, beta1: float = 0.9, beta2: float = 0.999,
                   eps: float = 1e-8, step: int = 1) -> None:
        SparseStep("adam", lr, eps, beta1, beta2, step).apply_to(self.local_group, *self._push("apply_adam", keys, offsets, grads))


class ShardedTieredTableGroup(ShardedTableGroup):
    """ShardedTableGroup whose local members are hot/cold PAIRS (SPEC.md §5 "Groups of pairs"): every rank holds one TieredTableGroup of its T local
    shards, each shard an HBM table in front of a table whose rows live in pinned host memory.  A pair is indistinguishable from one table holding
    the union of its tiers (SPEC.md §3 "Tiering"), so this is, by definition, the sharded group over the T union tables: every operator, the exchange,
    the collectives (4 per find, 3 per step, 5 per pooled lookup, 4 per pooled step, whatever T is) and traffic() are ShardedTableGroup's, unchanged;
    the owner's calls land on the tiered group's operators of the same names — find / find_or_insert (one / two launches over both tiers of every
    member, bf16 rows rounded before they travel), apply_adagrad / apply_adam and apply_indexed (two grouped steps), find_pooled_jagged (ONE launch
    over the runs of every member, mee_group_find_pooled_tiered_jagged).  Weighted bags, dedup= and located rows are not offered.

    Creation: the owner's pair picks the tier of a new key, and is charged with the size of the whole regrouped batch the owner received
    (TieredTableGroup.find_or_insert's conservative bound: a member goes cold earlier than the pair on its own segment would, never later).
    Placement policy: with find_pooled(insert_missing=True) the owner looks the received keys up twice — the unpooled find_or_insert in front, then
    the pooled launch — and both feed the hit counters: that step's hits count twice (as under nn.DynamicEmbeddingBag(create_missing=True) over a pair).

    rebalance() and size() are passed through; the pairs stay usable on their own (promote, demote, export, checkpoints) between steps."""
    _over_pairs = True

    def __init__(self, local_group, router, group=None):
        from .tiered import TieredTableGroup
        if not isinstance(local_group, TieredTableGroup):
            raise ValueError(f"{type(local_group).__name__} is no TieredTableGroup: ShardedTieredTableGroup shards a collection of hot/cold pairs "
                             "(a TableGroup of HBM-only shards goes under ShardedTableGroup)")
        # a pair carries no row type of its own: its two tables are looked at
        refuse_narrow_rows("ShardedTieredTableGroup", *[t for p in local_group.tables for t in (p.hot, p.cold)])
        super().__init__(local_group, router, group)

    def rebalance(self, max_moves: int = 1 << 20) -> list[tuple[int, int]]:
        """TieredTableGroup.rebalance of this rank's pairs -> [(promoted, demoted)] per pair.  Between steps; rank-local: there is no collective in it,
        so the ranks need not call it together."""
        return self.local_group.rebalance(max_moves)

    def size(self) -> int:
        """keys over all ranks and both tiers (collective: one all-reduce), like ShardedLookupTable.size"""
        t = torch.tensor([self.local_group.size()], dtype=torch.int64, device="cpu" if self._stage else self.device)
        dist.all_reduce(t, group=self.group)
        return int(t.item())


class RcclShardedTable:
    """The same row-sharded table with the whole exchange behind the C-ABI (`mee_sharded_*`, csrc/meepo_sharded.hip):
    partition, grouped ncclSend/ncclRecv of keys (+ rows), the local operator, ONE grouped exchange of rows + found bytes
    back and the un-permute all run inside the library on the caller's stream.  `torch.distributed` is only used once, to
    hand rank 0's ncclUniqueId to the other ranks; per step there is no Python-side collective at all.

    pad_slack = 0: exact message sizes (one host synchronisation per operator, for the split sizes).
    pad_slack >= 1: fixed-capacity EMPTY-padded segments, no host synchronisation (see include/meepo_embedding.h).
    cold: the cold table of a hot/cold pair (`local` = the hot one): BASELINE configs[4] behind the C-ABI (mee_sharded_create_ex).
    dedup: lookups exchange only the batch's distinct keys, applies one summed gradient row per distinct key (MEE_SHARDED_DEDUP)."""

    def __init__(self, local, max_batch: int, group=None, pad_slack: float = 0.0, cold=None, dedup: bool = False, hot_key_limit: int = 0):
        import ctypes as C

        from . import _lib
        from ._lib import check
        self._lib, self._check, self._C = _lib, check, C
        refuse_narrow_rows("RcclShardedTable", local, cold)
        self.local, self.group = local, group
        self.dedup = bool(dedup)
        self.world, self.rank = dist.get_world_size(group), dist.get_rank(group)
        self.device, self.dim, self.max_batch = local.device, local.dim, int(max_batch)
        L = _lib.lib()
        self._comm = self._h = None
        # rank 0 makes the ncclUniqueId; everybody joins the communicator (collective)
        ident = (C.c_char * 128)()
        if self.rank == 0:
            check(L.mee_comm_unique_id(ident))
        box = [bytes(ident)]
        dist.broadcast_object_list(box, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
        comm = C.c_void_p()
        check(L.mee_comm_create(box[0], self.world, self.rank, self.device.index, C.byref(comm)))
        self._comm = comm
        h = C.c_void_p()
        self.cold = cold
        opt = _lib.ShardedOptions(struct_size=C.sizeof(_lib.ShardedOptions), flags=_lib.SHARDED_DEDUP if dedup else 0, max_batch=self.max_batch,
                                  pad_slack=float(pad_slack), cold=cold._h if cold is not None else None, hot_key_limit=int(hot_key_limit))
        check(L.mee_sharded_create_ex(local._h, self._comm, C.byref(opt), C.byref(h)))
        self._h = h
        cap = C.c_uint64()
        check(L.mee_sharded_info(self._h, None, None, C.byref(cap)))
        self.segment_capacity = cap.value

    def close(self) -> None:
        L = self._lib.lib()
        if getattr(self, "_h", None):
            L.mee_sharded_destroy(self._h)
            self._h = None
        if getattr(self, "_comm", None):
            L.mee_comm_destroy(self._comm)
            self._comm = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _s(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    def _k(self, keys: torch.Tensor) -> torch.Tensor:
        if keys.dtype != torch.int64 or keys.device != self.device:
            raise self._lib.MeepoError(self._lib.ERR_INVALID_ARG, f"keys must be int64 on {self.device}")
        return keys.contiguous().view(-1)

    def _r(self, rows: torch.Tensor, n: int) -> torch.Tensor:
        if rows.dtype != torch.float32 or rows.device != self.device or rows.numel() != n * self.dim:
            raise self._lib.MeepoError(self._lib.ERR_INVALID_ARG, f"rows must be float32 [{n},{self.dim}] on {self.device}")
        return rows.contiguous()

    def _lookup(self, name, keys, out, found, out_dtype):
        dt = _out_dtype(out_dtype, out)   # (ValueError before any call)
        k = self._k(keys)
        n = k.numel()
        out, found = _buffer(out, "out", out_dtype, (n, self.dim), self.device), _buffer(found, "found", torch.uint8, n, self.device)
        L = self._lib.lib()
        if dt == self._lib.DTYPE_F32:   # the fp32 entry points keep their code path
            self._check(getattr(L, name)(self._h, k.data_ptr(), n, out.data_ptr(), found.data_ptr(), self._s()))
        else:
            self._check(getattr(L, name + "_as")(self._h, k.data_ptr(), n, out.data_ptr(), dt, found.data_ptr(), self._s()))
        return out, found

    def find(self, keys: torch.Tensor, out: torch.Tensor | None = None, found: torch.Tensor | None = None, out_dtype: torch.dtype = torch.float32):
        """out_dtype=torch.bfloat16 (mee_sharded_find_as): every row rounded once by its key's OWNER, so half the row bytes come back over the
        link.  Collective: every rank passes the same out_dtype to a given call."""
        return self._lookup("mee_sharded_find", keys, out, found, out_dtype)

    def find_or_insert(self, keys: torch.Tensor, out: torch.Tensor | None = None, found: torch.Tensor | None = None,
                       out_dtype: torch.dtype = torch.float32):
        """out_dtype=torch.bfloat16 (mee_sharded_find_or_insert_as): only the returned copy is rounded, the shards create their rows in fp32."""
        return self._lookup("mee_sharded_find_or_insert", keys, out, found, out_dtype)

    def traffic(self) -> tuple[int, int]:
        """(sent, received): bytes this context has handed to ncclSend / ncclRecv since it was created (mee_sharded_traffic; no synchronisation)"""
        s, r = self._C.c_uint64(), self._C.c_uint64()
        self._check(self._lib.lib().mee_sharded_traffic(self._h, self._C.byref(s), self._C.byref(r)))
        return s.value, r.value

    def insert(self, keys: torch.Tensor, values: torch.Tensor) -> None:
        k = self._k(keys)
        v = self._r(values, k.numel())
        self._check(self._lib.lib().mee_sharded_insert(self._h, k.data_ptr(), v.data_ptr(), k.numel(), self._s()))

    def assign(self, keys: torch.Tensor, values: torch.Tensor) -> torch.Tensor:
        k = self._k(keys)
        v = self._r(values, k.numel())
        found = torch.empty(k.numel(), dtype=torch.uint8, device=self.device)
        self._check(self._lib.lib().mee_sharded_assign(self._h, k.data_ptr(), v.data_ptr(), k.numel(), found.data_ptr(), self._s()))
        return found

    def remove(self, keys: torch.Tensor) -> torch.Tensor:
        k = self._k(keys)
        found = torch.empty(k.numel(), dtype=torch.uint8, device=self.device)
        self._check(self._lib.lib().mee_sharded_remove(self._h, k.data_ptr(), k.numel(), found.data_ptr(), self._s()))
        return found

    def apply_adagrad(self, keys: torch.Tensor, grads: torch.Tensor, lr: float, eps: float = 1e-10) -> None:
        self._apply(SparseStep("adagrad", lr, eps), keys, grads)

    def apply_adam(self, keys: torch.Tensor, grads: torch.Tensor, lr: float, beta1: float = 0.9, beta2: float = 0.999,
                   eps: float = 1e-8, step: int = 1) -> None:
        self._apply(SparseStep("adam", lr, eps, beta1, beta2, step), keys, grads)

    def _apply(self, step: SparseStep, keys, grads) -> None:
        k = self._k(keys)
        g = self._r(grads, k.numel())
        step.launch("mee_sharded_apply", "", self._h, k.data_ptr(), g.data_ptr(), k.numel(), stream=self._s())

    def size(self) -> int:
        n = self._C.c_size_t()
        self._check(self._lib.lib().mee_sharded_size(self._h, self._C.byref(n), self._s()))
        return n.value

    def status(self) -> int:
        b = self._C.c_uint32()
        self._check(self._lib.lib().mee_sharded_status(self._h, self._C.byref(b), self._s()))
        return b.value

    def clear_status(self) -> None:
        self._check(self._lib.lib().mee_sharded_clear_status(self._h, self._s()))

    def export_local(self, with_state: bool = False):
        a = self.local.export(with_state=with_state)
        if getattr(self, "cold", None) is None:
            return a
        b = self.cold.export(with_state=with_state)
        return tuple(None if x is None else torch.cat([x, y]) for x, y in zip(a, b))
