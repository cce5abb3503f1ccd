"""Hot/cold tiering of one shard: an HBM table for hot keys in front of a table whose rows live in pinned host DRAM.

BASELINE.json configs[4] ("hot/cold tier: HBM + pinned host-DRAM spill"); reference anchor /root/reference/README.md:2
("Supports GPU, CPU … backends" — a GPU backend backed by a CPU-memory one).  The snapshot has no code for it.

Design (host logic only; every row still moves through the HIP kernels):
  * `hot`  = LookupTable(value_memory=MEM_HBM)          keys + rows in HBM
  * `cold` = LookupTable(value_memory=MEM_HOST_PINNED)  keys (the index) in HBM, rows/state in pinned, device-mapped host
             DRAM — the same find/insert/apply kernels read and write them over PCIe (zero-copy), asynchronously on the
             caller's stream, so a cold access costs PCIe bandwidth but no host thread and no staging copy.
  * a key lives in exactly ONE tier, so the pair behaves like one table (tests compare it with a single oracle table).
  * new keys go to the hot tier while it has room (`hot_key_limit`), else to the cold tier; `promote` / `demote` move
    keys (values AND optimizer state) between tiers.
  * placement policy (tables created with track_hits=True): every cold hit and every `sample_every`-th hot lookup bumps
    a per-slot counter inside the find kernel; `rebalance()` promotes the cold keys that were hit at least
    `promote_threshold` times in the window and, when the hot tier is full, first demotes hot keys that no sampled
    lookup touched.  It runs BETWEEN steps, on the stream the steps run on: its moves are mutators of both tables (they share the tables'
    per-batch scratch with the step's operators and read rows the next update writes), so they are ordered with them, not beside them.
  * in a training loop (`rebalance_every` = K): the pair runs `rebalance()` itself behind every K-th optimizer step — the
    forward lookups of those K steps are the observation window.
  * embedding bags (`find_pooled`): ONE launch that probes both tiers per position (mee_find_pooled_tiered) — a bag is summed in
    position order and hot and cold keys interleave inside it, so two pooled passes, one per tier, could not rebuild the result bit
    for bit.  The launch feeds the policy's counters like `find` does (cold hits always, hot hits on every sample_every-th call).

  * admission (`find_or_insert(min_count=)`, `find_pooled(insert_missing=True, min_count=)`, `admission_decay`; native tables): the pair's sketch is
    its HOT table's — an id in neither tier is counted there and created, in the tier find_or_insert would pick, only once it has been asked for
    min_count times (mee_find_or_insert_admit_missing); a sketch the cold table may have is never touched.

`hot` / `cold` are any objects with the LookupTable methods, so the logic also runs on the CPU test adapters.
"""
from __future__ import annotations

import torch

from .table import SparseStep, _pool_mode


def _pool_rows(rows: torch.Tensor, bag_offsets: torch.Tensor, mode: str) -> torch.Tensor:
    """SPEC.md §3 find_pooled given find's rows [n, dim]: per bag fp32 additions in position order (the first row copied, each later one
    added), 'mean' divides by (float)length, an empty bag is zeros; offsets past n are cut at n, a decreasing pair is an empty bag.
    Only the path of tiers that are not native tables takes it (the native pair pools inside its one launch)."""
    n = rows.shape[0]
    off = bag_offsets.to(torch.int64)
    end = off[1:].clamp(0, n)
    begin = torch.minimum(off[:-1].clamp(min=0), end)
    lens = end - begin
    out = torch.zeros((lens.numel(), rows.shape[1]), dtype=torch.float32, device=rows.device)
    for j in range(int(lens.max()) if lens.numel() else 0):
        m = lens > j
        r = rows[begin[m] + j]
        out[m] = r if j == 0 else out[m] + r
    if mode == "mean":
        nz = lens > 0
        out[nz] = out[nz] / lens[nz].to(torch.float32)[:, None]
    return out


def _takes_grad_index(table) -> bool:
    """the table's apply_adagrad declares grad_index (LookupTable's does; an adapter's need not)"""
    import inspect
    try:
        return "grad_index" in inspect.signature(table.apply_adagrad).parameters
    except (TypeError, ValueError):
        return False


class TieredLookupTable:
    weighted_bags = False   # no per_sample_weights over the pair (nn.DynamicEmbeddingBag refuses them)
    hot_cold_pair = True    # nn.DynamicEmbedding has no admitting forward over a pair

    def __init__(self, hot, cold, hot_key_limit: int | None = None, sample_every: int = 8, promote_threshold: int = 2,
                 rebalance_every: int = 0, rebalance_max_moves: int = 1 << 20):
        from ._lib import refuse_narrow_rows
        refuse_narrow_rows("TieredLookupTable", hot, cold)
        if hot.dim != cold.dim:
            raise ValueError("hot and cold tables must have the same dim")
        self.hot, self.cold, self.dim = hot, cold, hot.dim
        # find_pooled can write bf16 bag rows (a bag layer may ask for them); find / find_or_insert return fp32 rows, so there is no
        # supports_out_dtype.  An instance attribute only because tests/test_bf16_out.py makes a pair with __new__ (no __init__) and expects
        # the bag layer to refuse bf16 over it: on the class, that object would be accepted
        self.supports_pooled_out_dtype = True
        self.optimizer = getattr(hot, "optimizer", 0)
        # keep the hot table at a load it probes fast at (SPEC.md §2: probe length grows with load)
        self.hot_key_limit = int(hot_key_limit if hot_key_limit is not None else getattr(hot, "capacity", 0) * 0.75)
        self._hot_keys_ub = 0  # upper bound on hot.size(), maintained without synchronising
        self.policy = bool(getattr(hot, "track_hits", False) and getattr(cold, "track_hits", False))
        self.sample_every, self.promote_threshold = max(1, sample_every), promote_threshold
        self._calls = 0
        # the training loop's policy knob: a rebalance behind every rebalance_every-th apply_* (0 = the caller runs rebalance() itself)
        self.rebalance_every, self.rebalance_max_moves = max(0, int(rebalance_every)), int(rebalance_max_moves)
        self._train_steps = 0
        self.rebalance_log: list[tuple[int, int, int]] = []   # (optimizer step, promoted, demoted)

    # -- helpers -----------------------------------------------------------------------------------------
    @staticmethod
    def _idx(mask: torch.Tensor) -> torch.Tensor:
        return torch.nonzero(mask, as_tuple=False).view(-1)

    def _room_for(self, n_new: int) -> bool:
        if self._hot_keys_ub + n_new > self.hot_key_limit:
            self._hot_keys_ub = self.hot.size()  # refresh the bound (synchronises; only when the bound is hit)
        return self._hot_keys_ub + n_new <= self.hot_key_limit

    # -- operators (SPEC.md §3 on the union of both tiers) ---------------------------------------------------
    def find(self, keys: torch.Tensor):
        keys = keys.contiguous().view(-1)
        if not self.policy:
            out, found = self.hot.find(keys)
            # second pass on the same buffers: the cold table fills what the hot one missed — no host sync, no compaction
            self.cold.find_missing(keys, out, found)
            return out, found
        self._calls += 1
        if self._calls % self.sample_every == 0:
            out, found = self.hot.find_counted(keys)          # sampled: hot keys that are still in use get marked
        else:
            out, found = self.hot.find(keys)
        self.cold.find_counted(keys, out, found, missing_only=True)  # cold hits are always counted (they are PCIe-bound anyway)
        return out, found

    def _native(self) -> bool:
        from .table import LookupTable
        return isinstance(self.hot, LookupTable) and isinstance(self.cold, LookupTable)

    def find_pooled(self, keys: torch.Tensor, bag_offsets: torch.Tensor, mode: str = "sum", out: torch.Tensor | None = None,
                    found: torch.Tensor | None = None, insert_missing: bool = False, out_dtype: torch.dtype = torch.float32,
                    min_count: int | None = None):
        """Embedding-bag lookup over the pair (SPEC.md §3 find_pooled on the union): bag b = keys[bag_offsets[b]:bag_offsets[b+1]] ->
        ([n_bags, dim] sums or means in position order, per-key found mask).  An absent key reads the HOT table's default row, as in find.
        Two native tables: one launch (mee_find_pooled_tiered), which also feeds the placement policy's hit counters.
        insert_missing: absent keys are created first, in the tier find_or_insert would pick; `found` stays "present before the call".
        min_count (with insert_missing): that creation admits as find_or_insert(min_count=) does; a key not yet admitted pools as the hot default row.
        out_dtype=torch.bfloat16: the finished bag row is rounded once."""
        m = _pool_mode(mode, ValueError)
        if min_count is not None:
            if not insert_missing:
                raise ValueError("min_count needs insert_missing=True (admission decides when an absent key is created)")
            min_count = self._check_min_count(min_count)
        if not self._native():   # any objects with the LookupTable methods: their find, pooled here in position order
            if out_dtype not in (torch.float32, torch.bfloat16):
                raise ValueError(f"out_dtype must be torch.float32 or torch.bfloat16 (got {out_dtype})")
            flat = keys.contiguous().view(-1)
            rows, fnd = self.find_or_insert(flat) if insert_missing else self.find(flat)
            pooled = _pool_rows(rows, bag_offsets, mode).to(out_dtype)
            if out is not None:
                out.copy_(pooled)
            if found is not None:
                found.copy_(fnd)
            return (out if out is not None else pooled), (found if found is not None else fnd)
        from . import _lib
        from .table import _n_bags, _out_dtype, _pooled_args
        hot, cold = self.hot, self.cold
        dt = _out_dtype(out_dtype, out)
        k = hot._bag_keys(keys)
        n_bags = _n_bags(bag_offsets, hot.device)
        n, _, _, out, _, found = _pooled_args(k, hot.device, out, (n_bags, self.dim), out_dtype, found)
        if insert_missing and n:
            # the found mask alone, from a probe of both indexes (no row is read, nothing is written to a table) ...
            found.copy_(hot.locate(k)[1] | cold.locate(k)[1])
            # ... then the absent keys are created exactly as find_or_insert creates them (their rows land in a scratch nobody reads)
            rows = torch.empty((n, self.dim), dtype=torch.float32, device=hot.device)
            self._create_missing(k, rows, found, min_count)
        flags = 0
        if self.policy:
            self._calls += 1
            flags = _lib.TIER_COUNT_COLD | (_lib.TIER_COUNT_HOT if self._calls % self.sample_every == 0 else 0)
        # with insert_missing the launch writes no found bytes: `found` keeps meaning "present before the call", also for a key repeated in the batch
        _lib.check(_lib.lib().mee_find_pooled_tiered(hot._h, cold._h, k.data_ptr(), n, bag_offsets.data_ptr(), n_bags, out.data_ptr(), dt,
                                                     None if (insert_missing and n) else found.data_ptr(), m, flags, hot._s()))
        return out, found

    def find_padded(self, keys: torch.Tensor, bag_offsets: torch.Tensor, max_len: int, keep: str = "first", out: torch.Tensor | None = None,
                    found: torch.Tensor | None = None, out_dtype: torch.dtype = torch.float32, with_step: bool = False):
        """Padded sequence lookup over the pair (SPEC.md §3 "Tiering"): LookupTable.find_padded on the union of the two tiers, bit for bit ->
        (out [n_bags, max_len, dim], per-key found, lengths [n_bags]) and, with_step=True, (step_keys [n], grad_index [n]) for apply_*(grad_index=).
        A kept position reads the hot table's row, else the cold table's, else the HOT table's default row; a cut-off position is not probed.
        Two native tables: ONE launch (mee_find_padded_tiered), which feeds the placement policy's hit counters like find_pooled does (cold hits
        always, hot hits on every sample_every-th call; a cut-off position counts nothing).  Other tiers: find on the kept keys, placed into a
        zeroed block."""
        if not self._native():
            from .table import _find_padded_composed
            return _find_padded_composed(lambda kk, pos: self.find(kk), self.dim, keys, bag_offsets, max_len, keep, out, found, out_dtype, with_step)
        from . import _lib
        from .table import _find_padded, _n_bags
        hot, cold = self.hot, self.cold
        k = hot._bag_keys(keys)
        n_bags = _n_bags(bag_offsets, hot.device)

        def launch(h, *args):   # _find_padded's call with the cold table and the count bits put in: (hot, cold, ..., flags, count_flags, ...)
            count = 0
            if self.policy:   # (here, behind _find_padded's checks: a refused call is not one of the policy's calls)
                self._calls += 1
                count = _lib.TIER_COUNT_COLD | (_lib.TIER_COUNT_HOT if self._calls % self.sample_every == 0 else 0)
            return _lib.lib().mee_find_padded_tiered(h, cold._h, *args[:6], count, *args[6:])
        return _find_padded(launch, hot._h, hot.device, self.dim, k, bag_offsets, n_bags, n_bags, max_len, keep, out, found, out_dtype, with_step)

    def rebalance(self, max_moves: int = 1 << 20) -> tuple[int, int]:
        """One policy step: promote cold keys hit >= promote_threshold times since the last call, demoting untouched hot
        keys first if the hot tier is full.  Returns (promoted, demoted).  Starts a new observation window."""
        if not self.policy:
            raise RuntimeError("rebalance() needs both tiers created with track_hits=True")
        cand = self.cold.hits_scan(self.promote_threshold, 0xFFFFFFFF, max_moves, reset=True)
        self._hot_keys_ub = self.hot.size()
        room = max(0, self.hot_key_limit - self._hot_keys_ub)
        need = max(0, int(cand.numel()) - room)
        demoted = 0
        victims = self.hot.hits_scan(0, 0, need, reset=True)   # also restarts the hot tier's window
        if need and victims.numel():
            demoted = self._move(self.hot, self.cold, victims)
            self._hot_keys_ub -= demoted
            room += demoted
        promoted = self._move(self.cold, self.hot, cand[:room]) if room and cand.numel() else 0
        self._hot_keys_ub += promoted
        return promoted, demoted

    # Mutators exploit "a key lives in exactly one tier": overwrite / delete passes simply go to BOTH tables (the one
    # that does not hold the key ignores it) and the found masks are OR-ed; only the creation of new keys needs the
    # combined mask, through the *_missing operators.  Nothing here synchronises except the rare refresh of the
    # hot-tier fill bound.
    def insert(self, keys: torch.Tensor, values: torch.Tensor) -> None:
        keys = keys.contiguous().view(-1)
        values = values.contiguous().view(keys.numel(), self.dim)
        found = self.hot.assign(keys, values) | self.cold.assign(keys, values)   # present somewhere: overwritten (last wins)
        n = keys.numel()
        if self._room_for(n):                                                   # n bounds the number of new keys
            self.hot.insert_missing(keys, values, found)
            self._hot_keys_ub += n
        else:
            self.cold.insert_missing(keys, values, found)

    def assign(self, keys: torch.Tensor, values: torch.Tensor) -> torch.Tensor:
        keys = keys.contiguous().view(-1)
        values = values.contiguous().view(keys.numel(), self.dim)
        return self.hot.assign(keys, values) | self.cold.assign(keys, values)

    def remove(self, keys: torch.Tensor) -> torch.Tensor:
        keys = keys.contiguous().view(-1)
        return self.hot.remove(keys) | self.cold.remove(keys)

    @property
    def admission(self) -> bool:
        """the pair admits iff its HOT table was created with admission=True: the pair's sketch is the hot table's (SPEC.md §3 "Tiering")"""
        return bool(getattr(self.hot, "_opts", {}).get("admission", False))

    def admission_refusal(self) -> str | None:
        """why an admitting call (min_count) is refused on this pair, or None: its own operators and the nn layers ask here"""
        if not self._native():
            return ("admission needs a hot/cold pair of native LookupTables (it counts in the hot table's sketch on the device); "
                    f"this pair holds {type(self.hot).__name__} / {type(self.cold).__name__}")
        if not self.admission:
            return "a hot/cold pair counts in its hot table's sketch, so the hot table needs admission=True (this pair's hot table has no sketch)"
        return None

    def _check_min_count(self, min_count) -> int:
        """the threshold of an admitting call on this pair, or the reason there is none"""
        reason = self.admission_refusal()
        if reason:
            raise ValueError("min_count: " + reason)
        if isinstance(min_count, bool) or not isinstance(min_count, int) or not 0 <= min_count < 1 << 32:
            raise ValueError(f"min_count must be an int in [0, 2^32) (got {min_count!r})")
        return min_count

    def _create_missing(self, keys: torch.Tensor, out: torch.Tensor, found: torch.Tensor, min_count) -> None:
        """the creation pass of find_or_insert / find_pooled(insert_missing=True) on buffers a lookup over both tiers filled: the positions `found`
        leaves missing create their key in ONE tier — hot while _room_for(n) holds, charged with the whole n — and receive its initial row.
        min_count: only the keys the HOT table's sketch admits (mee_find_or_insert_admit_missing), whichever tier creates."""
        n = keys.numel()
        room = self._room_for(n)
        target = self.hot if room else self.cold
        if room:
            self._hot_keys_ub += n
        if min_count is None:
            target.find_or_insert_missing(keys, out, found)   # inserts the hashed initial row once per distinct new key
            return
        from . import _lib
        k = target._keys(keys)
        _lib.check(_lib.lib().mee_find_or_insert_admit_missing(target._h, self.hot._h, k.data_ptr(), k.numel(), out.data_ptr(), found.data_ptr(),
                                                               int(min_count), target._s()))

    def find_or_insert(self, keys: torch.Tensor, min_count: int | None = None):
        """min_count (native tables, the hot one created with admission=True; SPEC.md §3 "Tiering"): an absent key is created — in the tier
        find_or_insert would pick — only once the HOT table's sketch has seen it asked for min_count times, this batch included; until then its
        positions return the hot default row.  0 and 1 admit at first sight (and still count)."""
        if min_count is not None:
            min_count = self._check_min_count(min_count)
        keys = keys.contiguous().view(-1)
        out, found = self.find(keys)
        self._create_missing(keys, out, found, min_count)
        return out, found

    def admission_decay(self, shift: int = 1) -> None:
        """admission_decay of the hot table: the pair's sketch (a sketch the cold table may have is not the pair's)"""
        self._check_min_count(0)
        self.hot.admission_decay(shift)

    def _after_optimizer_step(self) -> None:
        if not (self.policy and self.rebalance_every):
            return
        self._train_steps += 1
        if self._train_steps % self.rebalance_every == 0:
            p, d = self.rebalance(self.rebalance_max_moves)
            self.rebalance_log.append((self._train_steps, int(p), int(d)))

    def apply_adagrad(self, keys: torch.Tensor, grads: torch.Tensor, lr: float, eps: float = 1e-10, grad_index: torch.Tensor | None = None) -> None:
        self._apply(SparseStep("adagrad", lr, eps), keys, grads, grad_index)

    def apply_adam(self, keys: torch.Tensor, grads: torch.Tensor, lr: float, beta1: float = 0.9, beta2: float = 0.999,
                   eps: float = 1e-8, step: int = 1, grad_index: torch.Tensor | None = None) -> None:
        self._apply(SparseStep("adam", lr, eps, beta1, beta2, step), keys, grads, grad_index)

    def apply_ftrl(self, keys: torch.Tensor, grads: torch.Tensor, lr: float, beta: float = 1.0, l1: float = 0.0, l2: float = 0.0,
                   grad_index: torch.Tensor | None = None) -> None:
        """The FTRL-Proximal step (tiers created with OPT_FTRL) on the tier that holds each key; z and n travel with a row when it changes tier."""
        self._apply(SparseStep.ftrl(lr, beta, l1, l2), keys, grads, grad_index)

    def _apply(self, step: SparseStep, keys, grads, grad_index) -> None:
        # a key lives in one tier and each table ignores keys it does not hold: both see the whole batch.  grad_index (one int per key: position i
        # takes row grad_index[i] of grads — a pooled lookup's bag) goes to both as well; a key's duplicates are reduced in the one tier that holds it
        kw = {} if grad_index is None else {"grad_index": grad_index}
        if grad_index is not None and not all(_takes_grad_index(t) for t in (self.hot, self.cold)):
            # only for tiers whose apply_* have no grad_index (plain adapters; whichever lookup the index came from, padded or pooled): the rows
            # gathered here, padding (EMPTY) left out.  Tiers that take the index — native tables, adapters that declare it — get it as before
            live = keys != -(1 << 63)
            keys, grads, kw = keys[live], grads[grad_index[live].to(torch.int64)], {}
        step.apply_to(self.hot, keys, grads, **kw)
        step.apply_to(self.cold, keys, grads, **kw)
        self._after_optimizer_step()

    # duplicate reductions touch no table row, only a table's per-batch scratch: the hot table lends its own
    def dedup_keys(self, keys: torch.Tensor, miss_index: int = -1):
        return self.hot.dedup_keys(keys, miss_index=miss_index)

    def dedup_sum(self, keys: torch.Tensor, grads: torch.Tensor | None = None, **kw):
        return self.hot.dedup_sum(keys, grads, **kw)

    def size(self) -> int:
        return self.hot.size() + self.cold.size()

    def export(self, with_state: bool = False):
        a, b = self.hot.export(with_state=with_state), self.cold.export(with_state=with_state)
        return tuple(None if x is None else torch.cat([x, y]) for x, y in zip(a, b))

    # -- checkpoint (checkpoint.py works on anything with iter_export / import_) ----------------------------------
    @property
    def device(self) -> torch.device:
        return getattr(self.hot, "device", torch.device("cpu"))

    @property
    def max_batch(self) -> int:
        return min(int(getattr(self.hot, "max_batch", 1 << 20)), int(getattr(self.cold, "max_batch", 1 << 20)))

    def iter_export(self, chunk_slots: int = 1 << 22, with_state: bool = True):
        yield from self.hot.iter_export(chunk_slots, with_state)
        yield from self.cold.iter_export(chunk_slots, with_state)

    def assign_plane(self, plane: int, keys: torch.Tensor, values: torch.Tensor) -> torch.Tensor:
        return self.hot.assign_plane(plane, keys, values) | self.cold.assign_plane(plane, keys, values)

    def import_(self, keys: torch.Tensor, values: torch.Tensor, state1: torch.Tensor | None = None,
                state2: torch.Tensor | None = None) -> None:
        """Bulk-load pairs + optimizer planes (hot while there is room, then cold), max_batch at a time."""
        keys = keys.contiguous().view(-1)
        step = self.max_batch
        for s in range(0, keys.numel(), step):
            k = keys[s:s + step]
            self.insert(k, values[s:s + step])
            for plane, st in ((1, state1), (2, state2)):
                if st is not None:
                    self.assign_plane(plane, k, st[s:s + step])

    def save(self, path: str, chunk_slots: int = 1 << 22) -> int:
        from . import checkpoint
        return checkpoint.save_table(self, path, chunk_slots)

    def load(self, path: str, chunk_pairs: int | None = None, keep=None) -> int:
        from . import checkpoint
        return checkpoint.load_into(self, path, chunk_pairs, keep)

    # -- tier migration ------------------------------------------------------------------------------------
    def _moves_natively(self) -> bool:
        """migration goes through mee_move (two native tables); otherwise through the operator sequence of _move_by_operators"""
        return self._native()

    def _move(self, src, dst, keys: torch.Tensor) -> int:
        """Move the keys that `src` holds into `dst`, rows and optimizer state; returns how many (distinct keys) were moved.  Two native tables: ONE
        move (SPEC.md §3 move, LookupTable.move_to: no [n, dim] buffer, a key `dst` has no room for stays in `src`) and one read-back, the count."""
        if not self._moves_natively():
            return self._move_by_operators(src, dst, keys)
        n_moved, _ = src.move_to(dst, keys.contiguous().view(-1))
        return int(n_moved.item())

    def _move_by_operators(self, src, dst, keys: torch.Tensor) -> int:
        """_move for tiers that are not native tables (any objects with the LookupTable methods): find, insert, find_plane / assign_plane per state
        plane, remove — the definition SPEC.md §3 gives move, spelled out with the generic operators."""
        keys = torch.unique(keys.contiguous().view(-1))
        vals, found = src.find(keys)
        idx = self._idx(found != 0)
        if not idx.numel():
            return 0
        k = keys[idx]
        dst.insert(k, vals[idx])                         # state planes of new keys start at their initial values …
        n_planes = {0: 0, 1: 1, 2: 2, 3: 2}[self.optimizer]   # (Adam and FTRL keep two state planes)
        for plane in range(1, n_planes + 1):             # … and are then overwritten with the migrated state
            st, _ = src.find_plane(plane, k)
            dst.assign_plane(plane, k, st)
        src.remove(k)
        return int(k.numel())

    def _move_staged(self, keys: torch.Tensor) -> int:
        """cold -> hot through a staged transfer (BASELINE configs[4] "async hipMemcpy side stream"): probe the cold index for the slots,
        gather the rows (and state planes) out of the pinned host planes ON THE HOST into one contiguous pinned staging buffer, ship it with
        ONE asynchronous copy on a side stream, insert into the hot table.  The alternative `_move` lets the find kernel read the same
        rows straight over PCIe (zero-copy); tools/tier_bench.py measures the two against each other."""
        import numpy as np
        keys = torch.unique(keys.contiguous().view(-1))
        slots, found = self.cold.locate(keys)
        idx = self._idx(found != 0)
        if not idx.numel():
            return 0
        k = keys[idx]
        hs = slots[idx].cpu().numpy()                     # synchronises: the host needs the slot list
        n_planes = {0: 0, 1: 1, 2: 2, 3: 2}[self.optimizer]   # (Adam and FTRL keep two state planes)
        if not hasattr(self, "_side"):
            self._side = torch.cuda.Stream(self.device)
        staged = []
        for plane in range(0, n_planes + 1):
            host = torch.empty((hs.size, self.dim), dtype=torch.float32, pin_memory=True)
            np.take(self.cold.plane_host_view(plane), hs, axis=0, out=host.numpy())   # host-side gather of scattered 256-B rows
            with torch.cuda.stream(self._side):
                staged.append(host.to(self.device, non_blocking=True))                # one hipMemcpyAsync per plane on the side stream
        torch.cuda.current_stream(self.device).wait_stream(self._side)
        self.hot.insert(k, staged[0])
        for plane in range(1, n_planes + 1):
            self.hot.assign_plane(plane, k, staged[plane])
        self.cold.remove(k)
        return int(k.numel())

    def promote(self, keys: torch.Tensor, staged: bool = False) -> int:
        """cold -> hot for the given keys (those that are cold), as many as the hot tier has room for.  staged=True: host-side gather +
        one asynchronous copy on a side stream instead of zero-copy reads by the find kernel (see _move_staged)."""
        keys = torch.unique(keys.contiguous().view(-1))
        if self._moves_natively() and not staged:
            # the move serves the first `room` cold keys in sorted order itself (max_moves): no lookup of the cold rows for their found mask, no compaction
            if not keys.numel():
                return 0
            self._hot_keys_ub = self.hot.size()
            room = max(0, self.hot_key_limit - self._hot_keys_ub)
            moved = int(self.cold.move_to(self.hot, keys, max_moves=room)[0].item()) if room else 0
            self._hot_keys_ub += moved
            return moved
        _, in_cold = self.cold.find(keys)
        cand = keys[self._idx(in_cold != 0)]
        if not cand.numel():
            return 0
        self._hot_keys_ub = self.hot.size()
        room = max(0, self.hot_key_limit - self._hot_keys_ub)
        cand = cand[:room]
        moved = (self._move_staged(cand) if staged else self._move(self.cold, self.hot, cand)) if cand.numel() else 0
        self._hot_keys_ub += moved
        return moved

    def demote(self, keys: torch.Tensor) -> int:
        """hot -> cold for the given keys (those that are hot)."""
        moved = self._move(self.hot, self.cold, keys)
        self._hot_keys_ub = max(0, self._hot_keys_ub - moved)
        return moved

    def evict_cold(self, n: int, spill: bool = False):
        """When the cold tier is full too: its `n` least-hit keys leave the pair (LookupTable.evict(least=True) on the cold table; the counters stay
        as they are, age them with cold.hits_decay).  -> how many left; spill=True: (keys, values, state1 | None, state2 | None, hits) of the evicted
        keys, for a tier behind this pair.  Needs a cold table with hit counters."""
        if not getattr(self.cold, "track_hits", False):
            raise RuntimeError("evict_cold() needs a cold table created with track_hits=True")
        return self.cold.evict(0xFFFFFFFF, int(n), reset=False, least=True, spill=spill)


class TieredTableGroup:
    """An embedding-bag COLLECTION of hot/cold pairs (SPEC.md §3 "Tiering"): `pairs` are TieredLookupTables of one device and one dim, bag b of a
    batch of n_tables * bags_per_table bags belongs to pair b // bags_per_table, and the group's pooled lookup is, by definition,
    pairs[b // bags_per_table].find_pooled on that pair's bags — in ONE launch for the whole collection (mee_group_find_pooled_tiered) where a loop
    over the pairs pays one launch per table.  Underneath: a TableGroup over the hot tables and one over the cold tables (`hot_group`, `cold_group`,
    both with max_apply_batch), so the step is two grouped steps whatever the number of tables.

    The same collection without pooling — a row per id, for sequence features: find / find_or_insert / apply_adagrad / apply_adam over a jagged batch
    (keys, offsets[n_tables + 1] on the device) with TableGroup's signatures, each by definition the pair's operator per member on its segment: one
    launch (mee_group_find_tiered), two (mee_group_find_or_insert_tiered) and two grouped steps.  nn.DynamicEmbeddingCollection trains over it.
    Weighted bags and located rows are not offered over tiers.

    Admission (every pair's hot table created with admission=True): find_or_insert(min_count=) and find_pooled(insert_missing=True, min_count=) are
    the pair's admitting operators per member, each member counting in its own hot sketch, in three launches (mee_group_find_or_insert_admit_tiered)
    and four (mee_group_ensure_admit_tiered in front of the pooled launch); admission_decay() is the hot group's.  The group keeps no counters.

    The owner's side of a sharded group of pairs (ShardedTieredTableGroup): find_pooled_jagged — the pooled lookup with the members' bag counts read
    from the device, one launch (mee_group_find_pooled_tiered_jagged) — and apply_indexed, two grouped indexed steps.

    The placement policy is on when EVERY pair has it (both tiers created with track_hits=True); the launch then counts cold hits always and hot
    hits on every sample_every-th call, as a pair does.  Some pairs with it and some without is a ValueError.

    Migration over the collection: promote / demote over a jagged batch and rebalance() are the pair's per member, with all members' keys moved by
    ONE grouped move per direction (mee_group_move: the hot group and the cold group are its two sides).

    The pairs stay usable on their own (rebalance, promote, demote, export, checkpoints).  Pairs that are not native tables (any objects with the
    LookupTable methods) are served by a loop over the pairs with the same results."""
    pools_with_insert = True            # nn.DynamicEmbeddingBag: unseen ids are created inside find_pooled(insert_missing=True)
    weighted_bags = False               # no per_sample_weights over the tiers
    supports_pooled_out_dtype = True    # find_pooled can write bf16 bag rows
    supports_out_dtype = True           # ... and find / find_or_insert bf16 rows (nn.DynamicEmbeddingCollection(out_dtype=torch.bfloat16))
    keyed_bags = True                   # find_pooled(layout="keyed", step_index=)

    def __init__(self, pairs, max_apply_batch: int = 0, sample_every: int = 8):
        self.tables = list(pairs)
        if not self.tables:
            raise ValueError("a tiered group needs at least one hot/cold pair")
        if len({int(p.dim) for p in self.tables}) != 1:
            raise ValueError(f"the pairs of a tiered group must have one dim (got {[int(p.dim) for p in self.tables]})")
        with_policy = [bool(p.policy) for p in self.tables]
        if any(with_policy) and not all(with_policy):
            raise ValueError("the placement policy is a property of the whole tiered group: every pair needs both tiers created with track_hits=True, "
                             f"or none (pairs with it: {[j for j, w in enumerate(with_policy) if w]})")
        if len({str(p.device) for p in self.tables}) != 1:
            raise ValueError("the pairs of a tiered group must live on one device")
        self.dim, self.policy = int(self.tables[0].dim), all(with_policy)
        self.optimizer = self.tables[0].optimizer
        self.sample_every, self._calls = max(1, int(sample_every)), 0
        self.hot_group = self.cold_group = None
        self._native = all(p._native() for p in self.tables)
        if self._native:
            from .table import TableGroup
            self.hot_group = TableGroup([p.hot for p in self.tables], max_apply_batch)
            self.cold_group = TableGroup([p.cold for p in self.tables], max_apply_batch)
            # where member j's new keys go (1 = cold): on the device for the creation launch, rewritten only when a member's choice changes
            self._goes_cold = [False] * len(self.tables)
            self._d_goes_cold = torch.zeros(len(self.tables), dtype=torch.uint8, device=self.device)

    @property
    def device(self) -> torch.device:
        return self.tables[0].device

    @property
    def layout_epoch(self):
        """Changes whenever a tier of a member removed, cleared or rehashed rows."""
        return tuple(getattr(t, "layout_epoch", None) for p in self.tables for t in (p.hot, p.cold))

    def close(self) -> None:
        for g in (self.hot_group, self.cold_group):
            if g is not None:
                g.close()
        self.hot_group = self.cold_group = None

    def size(self) -> int:
        return sum(p.size() for p in self.tables)

    def evict_cold(self, n_per_pair: int, spill: bool = False) -> list:
        """TieredLookupTable.evict_cold(n_per_pair, spill) of every pair -> its result per pair.  A loop over the pairs: eviction is rare, unlike
        the step, and every member scans its own cold table anyway."""
        return [p.evict_cold(n_per_pair, spill) for p in self.tables]

    def rebalance(self, max_moves: int = 1 << 20) -> list[tuple[int, int]]:
        """TieredLookupTable.rebalance() of every pair -> [(promoted, demoted)] per pair.  Between steps, like the pair's own.  Native pairs: every
        member still scans its two tiers' counters (hits_scan), then ALL members' victims move in one grouped move and all their sliced candidates in
        another (mee_group_move): at most two launch sequences and two read-backs for the collection, the list and the placement those of the loop."""
        if not (self._native and self.policy and all(p._moves_natively() for p in self.tables)):
            return [p.rebalance(max_moves) for p in self.tables]
        cands, victims, rooms = [], [], []
        for p in self.tables:
            cand = p.cold.hits_scan(p.promote_threshold, 0xFFFFFFFF, max_moves, reset=True)
            p._hot_keys_ub = p.hot.size()
            room = max(0, p.hot_key_limit - p._hot_keys_ub)
            need = max(0, int(cand.numel()) - room)
            vict = p.hot.hits_scan(0, 0, need, reset=True)   # also restarts the hot tier's window
            cands.append(cand)
            victims.append(vict if need else vict[:0])
            rooms.append(room)
        demoted = self._move_lists(self.hot_group, self.cold_group, victims)
        for p, d in zip(self.tables, demoted):
            p._hot_keys_ub -= d
        rooms = [r + d for r, d in zip(rooms, demoted)]
        promoted = self._move_lists(self.cold_group, self.hot_group, [c[:r] for c, r in zip(cands, rooms)])
        for p, m in zip(self.tables, promoted):
            p._hot_keys_ub += m
        return list(zip(promoted, demoted))

    def _move_lists(self, src_group, dst_group, lists) -> list[int]:
        """member j's key list moves from src_group.tables[j] to dst_group.tables[j]: the lists concatenated into one jagged batch, ONE grouped move, one
        read-back -> distinct keys moved per member.  A batch beyond a member's max_batch goes member by member instead."""
        sizes = [int(k.numel()) for k in lists]
        total = sum(sizes)
        if total == 0:
            return [0] * len(lists)
        if not self._moves_grouped(total):
            return [int(s.move_to(d, k)[0].item()) if k.numel() else 0 for s, d, k in zip(src_group.tables, dst_group.tables, lists)]
        bounds = [0]
        for s in sizes:
            bounds.append(bounds[-1] + s)
        offsets = torch.tensor(bounds, dtype=torch.int64).to(self.device)
        n_moved, _ = src_group.move_to(dst_group, torch.cat([k.view(-1) for k in lists]), offsets)
        return [int(m) for m in n_moved.tolist()]

    def _moves_grouped(self, n: int) -> bool:
        """a jagged batch of n keys can go through one grouped move: native pairs, and n within every member's max_batch (mee_group_move's bound)"""
        return bool(self._native and all(p._moves_natively() for p in self.tables) and n <= min(p.max_batch for p in self.tables))

    def _dedup_segments(self, keys: torch.Tensor, offsets: torch.Tensor):
        """every segment's keys sorted and made distinct (what TieredLookupTable.promote does to its batch), for all members at once -> (keys, offsets)"""
        flat = keys.contiguous().view(-1)
        n, nt = flat.numel(), len(self.tables)
        off = offsets.to(torch.int64).clamp(0, n)
        pos = torch.arange(n, device=flat.device)
        seg = torch.searchsorted(off[1:].contiguous(), pos, right=True)   # the member whose segment holds the position; n_tables: behind the last one
        inside = (pos >= off[0]) & (seg < nt)
        k, s = flat[inside], seg[inside]
        order = torch.argsort(k, stable=True)
        order = order[torch.argsort(s[order], stable=True)]             # by member, then by key
        k, s = k[order], s[order]
        keep = torch.ones_like(k, dtype=torch.bool)
        keep[1:] = (k[1:] != k[:-1]) | (s[1:] != s[:-1])
        k, s = k[keep], s[keep]
        bounds = torch.zeros(nt + 1, dtype=torch.int64, device=flat.device)
        bounds[1:] = torch.cumsum(torch.bincount(s, minlength=nt), 0)
        return k, bounds

    def promote(self, keys: torch.Tensor, offsets: torch.Tensor) -> list[int]:
        """TieredLookupTable.promote of every pair on its segment of the jagged batch (keys, offsets[n_tables + 1] on the device) -> keys moved per pair:
        cold -> hot, per member the first keys in sorted order that its hot tier has room for.  Native pairs: one grouped move with the members' room as
        device-side limits and one read-back of the counts (each member's hot size is refreshed first, as the pair's promote does)."""
        if not self._moves_grouped(keys.numel()):
            flat = keys.contiguous().view(-1)
            return [pair.promote(flat[s:e]) for pair, (s, e) in zip(self.tables, self._segments(offsets, flat.numel()))]
        self.hot_group._check_offsets(offsets)
        k, bounds = self._dedup_segments(keys, offsets)
        if not k.numel():
            return [0] * len(self.tables)
        rooms = []
        for p in self.tables:
            p._hot_keys_ub = p.hot.size()
            rooms.append(max(0, p.hot_key_limit - p._hot_keys_ub))
        moved = [int(m) for m in self.cold_group.move_to(self.hot_group, k, bounds, max_moves=rooms)[0].tolist()]
        for p, m in zip(self.tables, moved):
            p._hot_keys_ub += m
        return moved

    def demote(self, keys: torch.Tensor, offsets: torch.Tensor) -> list[int]:
        """TieredLookupTable.demote of every pair on its segment of the jagged batch -> keys moved per pair (hot -> cold).  Native pairs: one grouped
        move and one read-back."""
        if not self._moves_grouped(keys.numel()):
            flat = keys.contiguous().view(-1)
            return [pair.demote(flat[s:e]) for pair, (s, e) in zip(self.tables, self._segments(offsets, flat.numel()))]
        moved = [int(m) for m in self.hot_group.move_to(self.cold_group, keys, offsets)[0].tolist()]
        for p, m in zip(self.tables, moved):
            p._hot_keys_ub = max(0, p._hot_keys_ub - m)
        return moved

    def _member_slices(self, bag_offsets: torch.Tensor, n: int):
        """(non-native path) -> bags_per_table, [(first bag, key begin, key end)] per member; offsets past n are cut at n"""
        nb = bag_offsets.numel() - 1
        if nb < 0 or nb % len(self.tables):
            raise ValueError("bag_offsets must hold n_tables * bags_per_table + 1 entries")
        bpt = nb // len(self.tables)
        cut = bag_offsets.to(torch.int64).clamp(0, n).tolist()
        return bpt, [(j * bpt, cut[j * bpt], max(cut[j * bpt], cut[(j + 1) * bpt])) for j in range(len(self.tables))]

    def admission_refusal(self) -> str | None:
        """TieredLookupTable.admission_refusal of the first member that has one, named"""
        return next((f"member {j}: {r}" for j, r in enumerate(p.admission_refusal() for p in self.tables) if r), None)

    def _admission(self, min_count):
        """-> (scalar threshold, device list | None) of an admitting call over the group, TableGroup._min_counts's rules and caching; or the reason
        there is no such call"""
        reason = self.admission_refusal()
        if reason:
            raise ValueError("min_count: " + reason)
        return self.hot_group._min_counts(min_count)

    def admission_decay(self, shift: int = 1) -> None:
        """TieredLookupTable.admission_decay of every pair, one launch: the hot group's (the pairs' sketches are their hot tables')"""
        self._admission(0)
        self.hot_group.admission_decay(shift)

    def _place_new_keys(self, n: int) -> None:
        """where every member's new keys of a batch of n go: hot while pairs[j]._room_for(n) holds (charged with the whole n), else cold — onto the
        device for the creation launch, rewritten only when a member's choice changes"""
        goes_cold = []
        for p in self.tables:
            room = p._room_for(n)
            if room:
                p._hot_keys_ub += n
            goes_cold.append(not room)
        if goes_cold != self._goes_cold:
            self._d_goes_cold.copy_(torch.tensor(goes_cold, dtype=torch.uint8))
            self._goes_cold = goes_cold

    def find_pooled(self, keys: torch.Tensor, bag_offsets: torch.Tensor, mode: str = "sum", out: torch.Tensor | None = None,
                    found: torch.Tensor | None = None, insert_missing: bool = False, out_dtype: torch.dtype = torch.float32, min_count=None,
                    layout: str = "table", step_index: torch.Tensor | None = None):
        """TieredLookupTable.find_pooled of every pair on its bags, in one launch -> ([n_tables * bags_per_table, dim] sums or means in position
        order, per-key found mask).  An absent key reads its member's HOT table's default row.  With the policy on the launch feeds the
        members' hit counters (cold hits always, hot hits on every sample_every-th call).
        insert_missing: three launches whatever the number of tables, and no [n, dim] tensor — the found pass (it finishes before anything is
        created, so `found` means "present before the call" also for a key repeated in the batch), ONE creation launch (member j's new keys go
        to its hot table while pairs[j]._room_for(n) holds, else to its cold table, created as find_or_insert_missing creates them), then the
        pooled launch, which writes no found bytes.  n, the size of the WHOLE batch, is the only bound the host has on a member's new keys:
        it is conservative — a member is charged n keys per call, goes cold (after one refresh of its hot table's size, which synchronises)
        earlier than the pair on its own slice would, never later.
        min_count (with insert_missing; an int or one threshold per member): the creation admits, each member counting in its hot table's sketch
        (mee_group_ensure_admit_tiered: one launch more, the count); a key not yet admitted pools as its member's hot default row.
        out_dtype=torch.bfloat16: the finished bag row is rounded once.
        layout="keyed": the same rows as [bags_per_table, n_tables * dim], sample s of every pair side by side in row s, written by the launch itself
        (mee_group_find_pooled_tiered_keyed; `out` may be any 2-D view with stride(1) == 1); step_index (uint32 / int32 [n], keyed only) receives
        the bag_of_position with which apply_pooled reads the keyed gradient, viewed [bags_per_table * n_tables, dim], in place."""
        from .table import _check_layout
        keyed = _check_layout(layout)
        if step_index is not None and not keyed:
            raise ValueError("step_index is the keyed layout's (layout='keyed')")
        m = _pool_mode(mode, ValueError)
        if keyed and not self._native:   # the loop below, then one permute: what the launch writes directly over native pairs
            pooled, fnd = self.find_pooled(keys, bag_offsets, mode, None, found, insert_missing, out_dtype, min_count)
            nt, bpt = len(self.tables), pooled.shape[0] // len(self.tables)
            rows = pooled.view(nt, bpt, self.dim).transpose(0, 1).reshape(bpt, nt * self.dim)
            if step_index is not None:
                o = bag_offsets.to(torch.int64).clamp(0, keys.numel())
                lens = (o[1:] - o[:-1]).clamp(min=0)
                bag = torch.repeat_interleave(torch.arange(lens.numel(), device=lens.device), lens)
                step_index[int(o[0]):int(o[0]) + bag.numel()] = ((bag % bpt) * nt + bag // bpt).to(step_index.dtype)
            if out is not None:
                out.copy_(rows)
            return (out if out is not None else rows), fnd
        admits = None
        if min_count is not None:
            if not insert_missing:
                raise ValueError("min_count needs insert_missing=True (admission decides when an absent key is created)")
            admits = self._admission(min_count)
        if not self._native:   # a loop over the pairs, member j on its slice of the keys and its bags_per_table bags
            if out_dtype not in (torch.float32, torch.bfloat16):
                raise ValueError(f"out_dtype must be torch.float32 or torch.bfloat16 (got {out_dtype})")
            flat = keys.contiguous().view(-1)
            bpt, members = self._member_slices(bag_offsets, flat.numel())
            pooled = torch.zeros((bpt * len(self.tables), self.dim), dtype=out_dtype, device=flat.device)
            fnd = torch.zeros(flat.numel(), dtype=torch.uint8, device=flat.device)
            for pair, (b0, s, e) in zip(self.tables, members):
                o, f = pair.find_pooled(flat[s:e], bag_offsets[b0:b0 + bpt + 1].to(torch.int64) - s, mode, insert_missing=insert_missing, out_dtype=out_dtype)
                pooled[b0:b0 + bpt] = o
                fnd[s:e] = f
            if out is not None:
                out.copy_(pooled)
            if found is not None:
                found.copy_(fnd)
            return (out if out is not None else pooled), (found if found is not None else fnd)
        from . import _lib
        from .table import _out_dtype, _pooled_args, _ptr, _step_index, _stream_ptr
        dt = _out_dtype(out_dtype, None if keyed else out)
        bpt = self.hot_group._check_bags(bag_offsets)
        k = self.tables[0].hot._bag_keys(keys)
        rows = (bpt * len(self.tables), self.dim)
        n, _, _, out, stride, found = _pooled_args(k, self.device, out, (bpt, len(self.tables) * self.dim) if keyed else rows, out_dtype, found, keyed=keyed)
        index = _step_index(step_index, n, self.device)
        L, s = _lib.lib(), _stream_ptr(self.device)
        hot, cold = self.hot_group._h, self.cold_group._h
        creates = bool(insert_missing and n and bpt)

        def create(block):
            """the found mask of the whole batch first, its rows written to `block` (no counters: this pass is not a lookup of the model's), then
            every member creates its absent keys in the tier its pair would pick — those that its hot sketch admits, with min_count"""
            _lib.check(L.mee_group_find_pooled_tiered(hot, cold, k.data_ptr(), n, bag_offsets.data_ptr(), bpt, block.data_ptr(), dt, found.data_ptr(), m, 0, s))
            self._place_new_keys(n)
            if admits is None:
                _lib.check(L.mee_group_ensure_tiered(hot, cold, k.data_ptr(), n, bag_offsets.data_ptr(), bpt, found.data_ptr(), self._d_goes_cold.data_ptr(), s))
            else:
                _lib.check(L.mee_group_ensure_admit_tiered(hot, cold, k.data_ptr(), n, bag_offsets.data_ptr(), bpt, found.data_ptr(), self._d_goes_cold.data_ptr(),
                                                           admits[0], _ptr(admits[1]), s))
        if creates:   # (keyed: the found pass writes no rows the caller sees — they go to a scratch block, the keyed launch writes `out`)
            create(torch.empty(rows, dtype=out_dtype, device=self.device) if keyed else out)
        if keyed:
            _lib.check(L.mee_group_find_pooled_tiered_keyed(hot, cold, k.data_ptr(), n, bag_offsets.data_ptr(), bpt, out.data_ptr(), dt, stride,
                                                            None if creates else found.data_ptr(), index, m, self._count_flags(), s))
        else:
            _lib.check(L.mee_group_find_pooled_tiered(hot, cold, k.data_ptr(), n, bag_offsets.data_ptr(), bpt, out.data_ptr(), dt,
                                                      None if creates else found.data_ptr(), m, self._count_flags(), s))
        return out, found

    # -- the unpooled collection: a row per position of the jagged batch (keys = the members' id batches concatenated, offsets = n_tables + 1 bounds) ----
    def _segments(self, offsets: torch.Tensor, n: int):
        """(non-native path) -> [(key begin, key end)] per member; offsets past n are cut at n"""
        if offsets.dim() != 1 or offsets.numel() != len(self.tables) + 1:
            raise ValueError(f"offsets must hold n_tables + 1 = {len(self.tables) + 1} entries (got {tuple(offsets.shape)})")
        cut = offsets.to(torch.int64).clamp(0, n).tolist()
        return [(cut[j], max(cut[j], cut[j + 1])) for j in range(len(self.tables))]

    def _count_flags(self) -> int:
        """the count bits of one lookup of the model's: cold hits always, hot hits on every sample_every-th call (the counter find_pooled shares)"""
        if not self.policy:
            return 0
        from . import _lib
        self._calls += 1
        return _lib.TIER_COUNT_COLD | (_lib.TIER_COUNT_HOT if self._calls % self.sample_every == 0 else 0)

    def _find_loop(self, keys, offsets, out, found, out_dtype, insert: bool):
        """pairs that are not native tables: member j's find / find_or_insert on its slice; the fp32 rows are rounded once for bf16"""
        if out_dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"out_dtype must be torch.float32 or torch.bfloat16 (got {out_dtype})")
        flat = keys.contiguous().view(-1)
        n = flat.numel()
        if out is None:
            out = torch.zeros((n, self.dim), dtype=out_dtype, device=flat.device)
        if found is None:
            found = torch.zeros(n, dtype=torch.uint8, device=flat.device)
        for pair, (s, e) in zip(self.tables, self._segments(offsets, n)):
            if e > s:
                rows, fnd = pair.find_or_insert(flat[s:e]) if insert else pair.find(flat[s:e])
                out[s:e] = rows.to(out.dtype)
                found[s:e] = fnd
        return out, found

    def _lookup_args(self, keys, offsets, out, found, out_dtype):
        from .table import _out_dtype
        dt = _out_dtype(out_dtype, out)
        self.hot_group._check_offsets(offsets)
        k = self.tables[0].hot._bag_keys(keys)
        n = k.numel()
        return (dt, k, n, *self.tables[0].hot._rows_found(out, found, n, out_dtype))

    def find(self, keys: torch.Tensor, offsets: torch.Tensor, out: torch.Tensor | None = None, found: torch.Tensor | None = None,
             out_dtype: torch.dtype = torch.float32):
        """TieredLookupTable.find of every pair on its segment, in ONE launch (mee_group_find_tiered) -> (rows [n, dim], found [n]).  An absent key
        reads its member's HOT table's default row; positions outside the segments are left alone, as TableGroup.find leaves them.  With the policy
        on the launch feeds the members' hit counters (cold hits always, hot hits on every sample_every-th call).
        out_dtype=torch.bfloat16: every element rounded once."""
        if not self._native:
            return self._find_loop(keys, offsets, out, found, out_dtype, insert=False)
        from . import _lib
        from .table import _stream_ptr
        dt, k, n, out, found = self._lookup_args(keys, offsets, out, found, out_dtype)
        _lib.check(_lib.lib().mee_group_find_tiered(self.hot_group._h, self.cold_group._h, k.data_ptr(), offsets.data_ptr(), n, out.data_ptr(), dt,
                                                    found.data_ptr(), self._count_flags(), _stream_ptr(self.device)))
        return out, found

    def find_padded(self, keys: torch.Tensor, bag_offsets: torch.Tensor, max_len: int, keep: str = "first", out: torch.Tensor | None = None,
                    found: torch.Tensor | None = None, out_dtype: torch.dtype = torch.float32, with_step: bool = False):
        """TieredLookupTable.find_padded of every pair on its bags_per_table bags, in ONE launch (mee_group_find_padded_tiered) ->
        (out [n_tables * bags_per_table, max_len, dim], found [n], lengths) and, with_step=True, (step_keys, grad_index) for apply_indexed.  An absent
        key reads its member's HOT table's default row.  With the policy on the launch feeds the members' hit counters (cold hits always, hot hits on
        every sample_every-th call; a cut-off position counts nothing).  Pairs that are not native tables: member j's find on its kept keys, placed
        into a zeroed block."""
        if not self._native:
            from .table import _find_padded_composed
            flat = keys.contiguous().view(-1)
            bpt, members = self._member_slices(bag_offsets, flat.numel())

            def find_kept(kk, pos):   # the kept keys are in position order: member j's are those inside its key slice
                rows = torch.zeros((kk.numel(), self.dim), dtype=torch.float32, device=kk.device)
                fnd = torch.zeros(kk.numel(), dtype=torch.uint8, device=kk.device)
                for pair, (_, s, e) in zip(self.tables, members):
                    m = (pos >= s) & (pos < e)
                    if bool(m.any()):
                        r, f = pair.find(kk[m])
                        rows[m], fnd[m] = r.to(rows.device), f.to(fnd.device).to(torch.uint8)
                return rows, fnd
            return _find_padded_composed(find_kept, self.dim, flat, bag_offsets, max_len, keep, out, found, out_dtype, with_step)
        from . import _lib
        from .table import _find_padded
        bpt = self.hot_group._check_bags(bag_offsets)
        k = self.tables[0].hot._bag_keys(keys)
        cold = self.cold_group._h

        def launch(h, *args):   # _find_padded's call with the cold group and the count bits put in: (hot, cold, ..., flags, count_flags, ...)
            return _lib.lib().mee_group_find_padded_tiered(h, cold, *args[:6], self._count_flags(), *args[6:])
        return _find_padded(launch, self.hot_group._h, self.device, self.dim, k, bag_offsets, bpt * len(self.tables), bpt, max_len, keep, out, found, out_dtype,
                            with_step)

    def find_or_insert(self, keys: torch.Tensor, offsets: torch.Tensor, out: torch.Tensor | None = None, found: torch.Tensor | None = None,
                       out_dtype: torch.dtype = torch.float32, min_count=None):
        """TieredLookupTable.find_or_insert of every pair on its segment, in TWO launches whatever the number of tables
        (mee_group_find_or_insert_tiered): find, then one creation launch that also returns the created keys' initial rows.  found = present before
        the call.  Member j's new keys go to its hot table while pairs[j]._room_for(n) holds, else to its cold table; n is the size of the WHOLE
        batch, as in find_pooled(insert_missing=True): conservative, a member goes cold earlier than the pair on its own slice would, never later.
        min_count (every pair's hot table created with admission=True; mee_group_find_or_insert_admit_tiered, THREE launches):
        TieredLookupTable.find_or_insert(min_count=) per member on its segment, each member counting in its own hot sketch — an int, or one
        threshold per member (TableGroup.find_or_insert's rules); the members are charged with n as without it, admitted or not."""
        admits = None if min_count is None else self._admission(min_count)
        if not self._native:
            return self._find_loop(keys, offsets, out, found, out_dtype, insert=True)
        from . import _lib
        from .table import _stream_ptr
        dt, k, n, out, found = self._lookup_args(keys, offsets, out, found, out_dtype)
        if n:
            self._place_new_keys(n)
        hot, cold, to_cold = self.hot_group._h, self.cold_group._h, self._d_goes_cold.data_ptr()
        if admits is None:
            _lib.check(_lib.lib().mee_group_find_or_insert_tiered(hot, cold, k.data_ptr(), offsets.data_ptr(), n, out.data_ptr(), dt, found.data_ptr(), to_cold,
                                                                  self._count_flags(), _stream_ptr(self.device)))
        else:
            _lib.check(_lib.lib().mee_group_find_or_insert_admit_tiered(hot, cold, k.data_ptr(), offsets.data_ptr(), n, out.data_ptr(), dt, found.data_ptr(), to_cold,
                                                                        admits[0], admits[1].data_ptr() if admits[1] is not None else None,
                                                                        self._count_flags(), _stream_ptr(self.device)))
        return out, found

    def apply_adagrad(self, keys: torch.Tensor, offsets: torch.Tensor, grads: torch.Tensor, lr: float, eps: float = 1e-10) -> None:
        """The pair's sparse-Adagrad step per member over the jagged batch, as TWO grouped steps — the hot group's, then the cold group's: a key lives in
        one tier and a group ignores the keys its member does not hold — then every pair's rebalance_every bookkeeping."""
        self._apply(SparseStep("adagrad", lr, eps), keys, offsets, grads)

    def apply_adam(self, keys: torch.Tensor, offsets: torch.Tensor, grads: torch.Tensor, lr: float, beta1: float = 0.9, beta2: float = 0.999,
                   eps: float = 1e-8, step: int = 1) -> None:
        self._apply(SparseStep("adam", lr, eps, beta1, beta2, step), keys, offsets, grads)

    def apply_ftrl(self, keys: torch.Tensor, offsets: torch.Tensor, grads: torch.Tensor, lr: float, beta: float = 1.0, l1: float = 0.0,
                   l2: float = 0.0) -> None:
        """The pairs' FTRL-Proximal step per member over the jagged batch, as the two grouped steps of apply_adagrad."""
        self._apply(SparseStep.ftrl(lr, beta, l1, l2), keys, offsets, grads)

    def apply_pooled(self, keys: torch.Tensor, bag_offsets: torch.Tensor, bag_grads: torch.Tensor, bag_of_position: torch.Tensor,
                     optimizer: str, lr: float, eps: float | None = None, beta1: float = 0.9, beta2: float = 0.999, step: int = 1,
                     located: torch.Tensor | None = None, *, l1: float = 0.0, l2: float = 0.0) -> None:
        """Backward of find_pooled: the pair's step per member — position i takes row bag_of_position[i] of bag_grads — as TWO grouped steps, the hot
        group's and the cold group's (a key lives in one tier, and a group ignores the keys its member does not hold), then every pair's
        rebalance_every bookkeeping.  `located` is accepted for the bag layer's sake and not used: the tiered lookup hands out no located rows.
        optimizer "ftrl": eps is FTRL's beta (default 1.0), l1 / l2 its regularisation strengths."""
        self._apply(SparseStep.of(optimizer, lr, eps, beta1, beta2, step, error=ValueError, l1=l1, l2=l2), keys, bag_offsets, bag_grads, bag_of_position, pooled=True)

    def _apply(self, step: SparseStep, keys, offsets, grads, index=None, pooled: bool = False) -> None:
        """the step's three forms (TableGroup._apply's) on both tiers; pairs that are not native tables take the pair's step on their slices"""
        if not self._native:
            flat = keys.contiguous().view(-1)
            slices = [m[1:] for m in self._member_slices(offsets, flat.numel())[1]] if pooled else self._segments(offsets, flat.numel())
            for pair, (s, e) in zip(self.tables, slices):
                if index is None:
                    step.apply_to(pair, flat[s:e], grads[s:e])
                else:
                    step.apply_to(pair, flat[s:e], grads, grad_index=index[s:e])
            return
        for g in (self.hot_group, self.cold_group):
            if index is None:
                step.apply_to(g, keys, offsets, grads)
            elif pooled:
                g.apply_pooled(keys, offsets, grads, index, *step, **step.loose_kw())
            else:
                g.apply_indexed(keys, offsets, grads, index, *step, **step.loose_kw())
        for p in self.tables:
            p._after_optimizer_step()

    # -- the owner's side of a sharded group of pairs (sharded.py, ShardedTieredTableGroup): the runs that arrive per member differ in number ----
    def find_pooled_jagged(self, keys: torch.Tensor, bag_offsets: torch.Tensor, member_bags: torch.Tensor, mode: str = "sum",
                           out: torch.Tensor | None = None, found: torch.Tensor | None = None):
        """find_pooled where bag b belongs to the pair j with member_bags[j] <= b < member_bags[j + 1] (n_tables + 1 non-decreasing int64 on the
        device; a pair may have no bags; a bag outside the map is empty: a row of zeros, nothing probed, its positions' found bytes not written)
        -> ([n_bags, dim] fp32, per-key found mask).  TableGroup.find_pooled_jagged's arguments and checks without `located`; on every bag inside the
        map the pair's find_pooled on that bag, bit for bit.  ONE launch (mee_group_find_pooled_tiered_jagged), sync-free, which feeds the members'
        hit counters as find_pooled does."""
        from . import _lib
        from .table import _fp32_only
        _fp32_only(out, "find_pooled_jagged")
        nb = bag_offsets.numel() - 1
        if not self._native:   # a loop over the pairs, member j on its bags (a host read of member_bags)
            _pool_mode(mode, ValueError)
            if member_bags.dim() != 1 or member_bags.numel() != len(self.tables) + 1:
                raise ValueError(f"member_bags must hold n_tables + 1 = {len(self.tables) + 1} entries (got {tuple(member_bags.shape)})")
            flat = keys.contiguous().view(-1)
            n = flat.numel()
            if nb < 0 or (n and nb == 0):
                raise ValueError("bag_offsets must hold n_bags + 1 entries, and keys need bags to report them")
            off = bag_offsets.to(torch.int64)
            cut = off.clamp(0, n).tolist()
            mb = member_bags.to(torch.int64).clamp(0, nb).tolist()
            pooled = torch.zeros((nb, self.dim), dtype=torch.float32, device=flat.device)
            fnd = torch.zeros(n, dtype=torch.uint8, device=flat.device)
            for j, pair in enumerate(self.tables):
                b0, b1 = mb[j], max(mb[j], mb[j + 1])
                if b1 == b0:
                    continue
                s, e = min(cut[b0:b1 + 1]), max(cut[b0:b1 + 1])
                o, f = pair.find_pooled(flat[s:e], off[b0:b1 + 1] - s, mode)
                pooled[b0:b1] = o
                fnd[s:e] = f
            if out is not None:
                out.copy_(pooled)
            if found is not None:
                found.copy_(fnd)
            return (out if out is not None else pooled), (found if found is not None else fnd)
        from .table import _n_bags, _no_bags_for_keys, _pooled_args, _stream_ptr
        self.hot_group._check_offsets(member_bags)
        nb, m = _n_bags(bag_offsets, self.device), _pool_mode(mode)
        k = self.tables[0].hot._bag_keys(keys)
        _no_bags_for_keys(k.numel(), nb)
        n, _, _, out, _, found = _pooled_args(k, self.device, out, (nb, self.dim), torch.float32, found)
        _lib.check(_lib.lib().mee_group_find_pooled_tiered_jagged(self.hot_group._h, self.cold_group._h, k.data_ptr(), n, bag_offsets.data_ptr(), nb,
                                                                  member_bags.data_ptr(), out.data_ptr(), found.data_ptr(), m, self._count_flags(),
                                                                  _stream_ptr(self.device)))
        return out, found

    def apply_indexed(self, keys: torch.Tensor, offsets: torch.Tensor, grads: torch.Tensor, grad_index: torch.Tensor, optimizer: str, lr: float,
                      eps: float | None = None, beta1: float = 0.9, beta2: float = 0.999, step: int = 1, *, l1: float = 0.0, l2: float = 0.0) -> None:
        """One optimizer step over the jagged batch == the pair's apply_*(grad_index=...) per member with its segment: position i takes row
        grad_index[i] of grads [rows, dim].  TWO grouped indexed steps, the hot group's and the cold group's (a key lives in one tier, and a group
        ignores the keys its member does not hold — apply_pooled's argument), then every pair's rebalance_every bookkeeping."""
        self._apply(SparseStep.of(optimizer, lr, eps, beta1, beta2, step, error=ValueError, l1=l1, l2=l2), keys, offsets, grads, grad_index)
