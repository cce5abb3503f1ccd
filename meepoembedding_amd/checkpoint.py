"""Checkpoint format of a table: export's arrays, written as they come.

A checkpoint is a DIRECTORY:

    meta.json     {"format": "meepo-table-v1", "dim", "optimizer", "n", "planes": ["values", "state1", ...], "extra": {...}}
                  ("extra" carries "value_dtype": "bfloat16" when a bf16-row table wrote it; values.f32 holds its rows widened, and
                  loading an fp32 checkpoint into a bf16-row table — train, then serve — rounds every row once; "int8" when an
                  int8-row table wrote it: values.f32 holds its rows dequantized, and loading into one quantizes every row once)
    keys.i64      n little-endian int64 keys, in export order (unspecified, stable within the checkpoint)
    values.f32    n x dim little-endian fp32 rows, same order
    state1.f32    n x dim Adagrad accumulator / Adam m / FTRL z   (tables with an optimizer)
    state2.f32    n x dim Adam v / FTRL n                    (Adam and FTRL tables)

The table is walked in slot ranges (`mee_export_range`), so saving needs scratch for one range, not a second copy of the
table, and the pieces go to disk in order; loading reads the files back `chunk_pairs` at a time and re-inserts them
(`insert` + `assign_plane`), so a checkpoint loads into a table of ANY capacity, and — with a `keep` filter — into any
sharding: a rank of a G'-way job keeps the pairs whose owner(key, G') is itself, whatever G wrote them.

Incremental checkpoints (SPEC.md §3 "Change log"): a table with a change log (`track_changes`) is saved as a BASE — `save_base`, a checkpoint as
above whose "extra" carries a random "id" — followed by DELTAS, `save_delta`: directories of the same files holding only the keys noted since the
save before, plus the keys that are gone:

    meta.json     {"format": "meepo-delta-v1", "dim", "optimizer", "planes", "n", "n_removed", "id", "parent": the id of the save before it}
    keys.i64, values.f32, state*.f32     the n upserts: noted keys the table holds, with their rows and optimizer planes, as above
    removed.i64   n_removed little-endian int64 keys: noted keys the table no longer holds

`load_delta` is import_ of the upserts, then remove of the removed keys; `restore` loads a base and its deltas after checking the parent chain.

Reference anchor: /root/reference/README.md:2 ("dynamic lookuptable-style"); the snapshot defines no on-disk format, so this
one is simply the arrays `mee_export` returns.
"""
from __future__ import annotations

import json
import os

import numpy as np
import torch

FORMAT = "meepo-table-v1"
DELTA_FORMAT = "meepo-delta-v1"
_PLANES = ("values", "state1", "state2")


def _n_planes(optimizer: int) -> int:
    return 1 + (optimizer != 0) + (optimizer in (2, 3))   # Adam and FTRL keep two state planes


def save_table(table, path: str, chunk_slots: int = 1 << 22, extra: dict | None = None) -> int:
    os.makedirs(path, exist_ok=True)
    planes = _PLANES[: _n_planes(table.optimizer)]
    n = 0
    files = [open(os.path.join(path, "keys.i64"), "wb")] + [open(os.path.join(path, p + ".f32"), "wb") for p in planes]
    try:
        for piece in table.iter_export(chunk_slots, with_state=True):
            arrays = [piece[0]] + [x for x in piece[1:] if x is not None]
            for f, a in zip(files, arrays):
                a.cpu().numpy().tofile(f)
            n += piece[0].numel()
    finally:
        for f in files:
            f.close()
    # the files hold fp32 rows whatever the table stores (a bf16-row table's export widens, exactly): the format is the same; that the rows came out of
    # a bf16-row table is a note in "extra" (absent = fp32 rows)
    extra = dict(extra or {})
    if getattr(table, "value_dtype", torch.float32) == torch.bfloat16:
        extra["value_dtype"] = "bfloat16"
    if getattr(table, "value_dtype", torch.float32) == torch.int8:   # (values.f32 holds its rows dequantized)
        extra["value_dtype"] = "int8"
    meta = {"format": FORMAT, "dim": table.dim, "optimizer": int(table.optimizer), "n": n, "planes": list(planes), "extra": extra}
    tmp = os.path.join(path, "meta.json.tmp")
    with open(tmp, "w") as f:
        json.dump(meta, f)
    os.replace(tmp, os.path.join(path, "meta.json"))   # meta.json appears last: a directory without it is an unfinished save
    return n


def read_meta(path: str) -> dict:
    with open(os.path.join(path, "meta.json")) as f:
        meta = json.load(f)
    if meta.get("format") != FORMAT:
        raise ValueError(f"{path}: not a {FORMAT} checkpoint")
    return meta


def iter_pairs(path: str, chunk_pairs: int):
    """Yield (keys, values, state1 | None, state2 | None) numpy pieces of at most chunk_pairs pairs."""
    yield from _iter_pairs(path, read_meta(path), chunk_pairs)


def _iter_pairs(path: str, meta: dict, chunk_pairs: int):
    """iter_pairs over the arrays of a table checkpoint or of a delta's upserts (the same files)"""
    n, dim = meta["n"], meta["dim"]
    if os.path.getsize(os.path.join(path, "keys.i64")) != 8 * n:
        raise ValueError(f"{path}: keys.i64 does not hold the {n} keys meta.json promises")
    kf = open(os.path.join(path, "keys.i64"), "rb")
    pfs = [open(os.path.join(path, p + ".f32"), "rb") for p in meta["planes"]]
    try:
        for s in range(0, n, chunk_pairs):
            m = min(chunk_pairs, n - s)
            keys = np.fromfile(kf, dtype="<i8", count=m)
            rows = [np.fromfile(f, dtype="<f4", count=m * dim).reshape(m, dim) for f in pfs]
            if keys.size != m or any(r.shape[0] != m for r in rows):
                raise ValueError(f"{path}: truncated checkpoint")
            yield (keys, *rows, *([None] * (3 - len(rows))))
    finally:
        kf.close()
        for f in pfs:
            f.close()


def load_into(table, path: str, chunk_pairs: int | None = None, keep=None) -> int:
    """Load `path` into `table`; keep(keys_tensor) -> bool mask restricts what is loaded (re-sharding)."""
    return _load_pairs(table, path, read_meta(path), chunk_pairs, keep)


def _load_pairs(table, path: str, meta: dict, chunk_pairs: int | None, keep) -> int:
    """import_ of the pairs of a table checkpoint, or of a delta's upserts"""
    if meta["dim"] != table.dim:
        raise ValueError(f"checkpoint dim {meta['dim']} != table dim {table.dim}")
    chunk_pairs = chunk_pairs or int(getattr(table, "max_batch", 1 << 20))
    dev = getattr(table, "device", torch.device("cpu"))
    same_opt = int(meta["optimizer"]) == int(table.optimizer)   # state planes only mean something to the same optimizer
    loaded = 0
    for keys, vals, s1, s2 in _iter_pairs(path, meta, chunk_pairs):
        k = torch.from_numpy(keys).to(dev)
        parts = [torch.from_numpy(x).to(dev) if x is not None and (i == 0 or same_opt) else None for i, x in enumerate((vals, s1, s2))]
        if keep is not None:
            idx = torch.nonzero(keep(k)).view(-1)
            k = k[idx]
            parts = [p[idx] if p is not None else None for p in parts]
        if k.numel():
            table.import_(k, *parts)
            loaded += k.numel()
    return loaded


def save_sharded(sharded, path: str, chunk_slots: int = 1 << 22) -> int:
    """Every rank writes its shard under path/shard-<rank>-of-<world>; returns this rank's pair count."""
    d = os.path.join(path, f"shard-{sharded.rank:05d}-of-{sharded.world:05d}")
    return save_table(sharded.local, d, chunk_slots, extra={"rank": sharded.rank, "world": sharded.world})


def load_sharded(sharded, path: str, owner_of, chunk_pairs: int | None = None) -> int:
    """Load a sharded checkpoint written by ANY world size: this rank reads every shard directory and keeps the pairs
    it owns under the CURRENT world size (owner_of(keys) -> owner ranks); when the world size is unchanged it reads only
    its own directory.  Returns the pairs this rank loaded."""
    dirs = sorted(x for x in os.listdir(path) if x.startswith("shard-"))
    if not dirs:
        raise ValueError(f"{path}: no shard-* directories")
    mine = f"shard-{sharded.rank:05d}-of-{sharded.world:05d}"
    if mine in dirs and all(x.endswith(f"-of-{sharded.world:05d}") for x in dirs) and len(dirs) == sharded.world:
        return load_into(sharded.local, os.path.join(path, mine), chunk_pairs)
    n = 0
    for x in dirs:
        n += load_into(sharded.local, os.path.join(path, x), chunk_pairs, keep=lambda k: owner_of(k) == sharded.rank)
    return n


# ---- incremental checkpoints: a base, then deltas over the table's change log (SPEC.md §3 "Change log") ----------------------------------------
def _new_id() -> str:
    import secrets
    return secrets.token_hex(8)


def _log_of(table, who: str):
    log = getattr(table, "change_log", None)
    if log is None:
        raise ValueError(f"{who}: the table has no change log (call track_changes(capacity) before the first mutation to be saved)")
    return log


def save_base(table, path: str, chunk_slots: int = 1 << 22, extra: dict | None = None) -> int:
    """A full save that starts a chain of deltas: save_table with extra["id"] = a random hex id, then the table's change log is cleared — the log
    from here on holds what the next save_delta must carry.  Returns the number of pairs written."""
    log = _log_of(table, "save_base")
    sid = _new_id()
    n = save_table(table, path, chunk_slots, extra={**(extra or {}), "id": sid})
    log.clear()
    log.save_id = sid
    return n


def save_delta(table, path: str, chunk_slots: int = 1 << 22):
    """Write what changed in `table` since its last save_base / save_delta -> (n_upserts, n_removed): the noted keys the table holds, with their rows
    and optimizer planes, and the noted keys it no longer holds, one slot range of the log at a time (ChangeLog.iter_changed).  meta.json is written
    last, with this save's id and its parent's.  Raises, and writes no meta.json, when the log is invalid (it overflowed, or the table was cleared):
    the delta would be incomplete and the next save must be a save_base.  The log is cleared at the end."""
    log = _log_of(table, "save_delta")
    parent = getattr(log, "save_id", None)
    if parent is None:
        raise ValueError("save_delta: there is no save to be the delta's parent (call save_base first)")
    if log.invalid:
        raise RuntimeError("save_delta: the change log is invalid — it had no room for a changed key, or the table was cleared — so a delta would be "
                           "incomplete: write a full checkpoint with save_base (which clears the log)")
    os.makedirs(path, exist_ok=True)
    stale = os.path.join(path, "meta.json")
    if os.path.exists(stale):   # a directory without meta.json is an unfinished save, from the first byte written
        os.remove(stale)
    planes = _PLANES[: _n_planes(table.optimizer)]
    n = n_removed = 0
    files = [open(os.path.join(path, "keys.i64"), "wb")] + [open(os.path.join(path, p + ".f32"), "wb") for p in planes]
    removed_file = open(os.path.join(path, "removed.i64"), "wb")
    try:
        for piece in log.iter_changed(table, chunk_slots, with_state=True):
            arrays = [piece[0]] + [x for x in piece[1:4] if x is not None]
            for f, a in zip(files, arrays):
                a.cpu().numpy().tofile(f)
            piece[4].cpu().numpy().tofile(removed_file)
            n += piece[0].numel()
            n_removed += piece[4].numel()
    finally:
        for f in files + [removed_file]:
            f.close()
    sid = _new_id()
    meta = {"format": DELTA_FORMAT, "dim": table.dim, "optimizer": int(table.optimizer), "planes": list(planes), "n": n, "n_removed": n_removed,
            "id": sid, "parent": parent}
    tmp = os.path.join(path, "meta.json.tmp")
    with open(tmp, "w") as f:
        json.dump(meta, f)
    os.replace(tmp, os.path.join(path, "meta.json"))
    log.clear()
    log.save_id = sid
    return n, n_removed


def read_delta_meta(path: str) -> dict:
    with open(os.path.join(path, "meta.json")) as f:
        meta = json.load(f)
    if meta.get("format") != DELTA_FORMAT:
        raise ValueError(f"{path}: not a {DELTA_FORMAT} delta")
    if os.path.getsize(os.path.join(path, "removed.i64")) != 8 * meta["n_removed"]:
        raise ValueError(f"{path}: removed.i64 does not hold the {meta['n_removed']} keys meta.json promises")
    return meta


def load_delta(table, path: str, chunk_pairs: int | None = None, keep=None):
    """Apply a delta to `table` -> (upserts loaded, keys removed): import_ of the upserts (state planes only for the same optimizer), then remove of
    the removed keys.  keep(keys_tensor) -> bool mask restricts both lists (re-sharding), as in load_into."""
    meta = read_delta_meta(path)
    loaded = _load_pairs(table, path, meta, chunk_pairs, keep)
    chunk = chunk_pairs or int(getattr(table, "max_batch", 1 << 20))
    dev = getattr(table, "device", torch.device("cpu"))
    removed = 0
    with open(os.path.join(path, "removed.i64"), "rb") as f:
        for s in range(0, meta["n_removed"], chunk):
            k = torch.from_numpy(np.fromfile(f, dtype="<i8", count=min(chunk, meta["n_removed"] - s))).to(dev)
            if keep is not None:
                k = k[torch.nonzero(keep(k)).view(-1)]
            if k.numel():
                table.remove(k)
                removed += k.numel()
    return loaded, removed


def restore(table, base_path: str, delta_paths, chunk_pairs: int | None = None, keep=None) -> int:
    """Load a base and its deltas, in order, into `table` (of any capacity; `keep` as in load_into).  The chain is checked before anything is loaded:
    delta i's "parent" must be the id of the save in front of it — a gap, a reordering or a delta of another base is refused.  Returns the pairs
    the base loaded."""
    delta_paths = list(delta_paths)
    prev = read_meta(base_path).get("extra", {}).get("id")
    if delta_paths and prev is None:
        raise ValueError(f"{base_path}: a checkpoint without an id (save_table) is no base of a delta chain: write it with save_base")
    for p in delta_paths:
        meta = read_delta_meta(p)
        if meta.get("parent") != prev:
            raise ValueError(f"{p}: its parent is save {meta.get('parent')}, but the save in front of it in this chain is {prev} (a delta is missing, "
                             "the deltas are out of order, or it belongs to another base)")
        prev = meta["id"]
    n = load_into(table, base_path, chunk_pairs, keep)
    for p in delta_paths:
        load_delta(table, p, chunk_pairs, keep)
    return n


def _shard_dir(sharded, path: str) -> str:
    return os.path.join(path, f"shard-{sharded.rank:05d}-of-{sharded.world:05d}")


def save_sharded_base(sharded, path: str, chunk_slots: int = 1 << 22) -> int:
    """save_sharded as the base of a delta chain: every rank's local table (a LookupTable: sharded.local.track_changes(capacity)) keeps its own log"""
    return save_base(sharded.local, _shard_dir(sharded, path), chunk_slots, extra={"rank": sharded.rank, "world": sharded.world})


def save_sharded_delta(sharded, path: str, chunk_slots: int = 1 << 22):
    """Every rank writes the delta of its shard under path/shard-<rank>-of-<world> -> this rank's (n_upserts, n_removed)."""
    return save_delta(sharded.local, _shard_dir(sharded, path), chunk_slots)


def load_sharded_delta(sharded, path: str, owner_of, chunk_pairs: int | None = None):
    """Apply a sharded delta written by ANY world size, as load_sharded loads a checkpoint: with the world size unchanged a rank reads its own
    directory; otherwise every directory, keeping the keys it owns now (owner_of(keys) -> owner ranks).  -> this rank's (upserts loaded, keys removed)."""
    dirs = sorted(x for x in os.listdir(path) if x.startswith("shard-"))
    if not dirs:
        raise ValueError(f"{path}: no shard-* directories")
    mine = os.path.basename(_shard_dir(sharded, path))
    if mine in dirs and all(x.endswith(f"-of-{sharded.world:05d}") for x in dirs) and len(dirs) == sharded.world:
        return load_delta(sharded.local, os.path.join(path, mine), chunk_pairs)
    n = r = 0
    for x in dirs:
        dn, dr = load_delta(sharded.local, os.path.join(path, x), chunk_pairs, keep=lambda k: owner_of(k) == sharded.rank)
        n, r = n + dn, r + dr
    return n, r
